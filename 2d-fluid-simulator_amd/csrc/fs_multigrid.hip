// fs_multigrid.hip - C-ABI entry points of the multigrid pressure updater (fs_mg.h): the level hierarchy as a device object and one W-cycle
// as a sequence of launches on the context's stream - capturable, no synchronisation, no allocation.
#include "fs_launch.h"
#include "fs_mg.h"

// the hierarchy of one updater (fs_mg_create): five concatenated arrays over the cells of levels 1 .. n, level after level
struct fs_mg {
    int n = 0;                                   // levels 1 .. n (index 0 .. n - 1 below)
    int nx[fs::MG_MAX_LEVELS], ny[fs::MG_MAX_LEVELS];
    size_t off[fs::MG_MAX_LEVELS];               // first cell of the level
    size_t cells = 0;
    fs::DevBuf<void> d_E, d_R, d_cx, d_cy, d_diag;
    int tail = -1;                               // index of the first level the tail kernel holds in LDS (-1: none)
    size_t tail_bytes = 0;
    int coarse_sweeps = 2, coarsest_sweeps = 64;
    int launches = 0;                            // kernel launches of one fs_mg_cycle (counted while it runs)
    // an exact solve attached to the LAST level (fs_mg_set_direct): E[active] = M R[active] instead of coarsest_sweeps sweeps
    bool direct = false;
    int direct_n = 0, direct_stride = 0;         // active cells; elements per row of M (64 ceil(n / 64))
    fs::DevBuf<int> d_cells;                     // their indices J * nx + I in the level, ascending
    fs::DevBuf<void> d_M;                        // [n][stride] in the field dtype
};

FS_OBJECT(fs_mg, OBJ_MG, "multigrid", "multigrid hierarchy from another context or freed");

using namespace fs;

template <typename T>
static MgLevel<T> mg_level(const fs_mg *m, int k)
{
    MgLevel<T> l;
    l.E = (T *)m->d_E + m->off[k]; l.R = (T *)m->d_R + m->off[k];
    l.cx = (const T *)m->d_cx + m->off[k]; l.cy = (const T *)m->d_cy + m->off[k]; l.diag = (const T *)m->d_diag + m->off[k];
    l.nx = m->nx[k]; l.ny = m->ny[k];
    return l;
}

static dim3 mg_grid(int nx, int ny) { return dim3((nx + 255) / 256, ny); }

template <typename T>
static int mg_sweeps(fs_ctx *ctx, fs_mg *m, int k, int sweeps)
{
    const MgLevel<T> l = mg_level<T>(m, k);
    const dim3 grid = mg_grid((l.nx + 1) / 2, l.ny);
    for (int s = 0; s < 2 * sweeps; ++s) {
        const int parity = (s & 1) ^ 1;
        int rc = launch(ctx, "mg_halfsweep", [=] { klaunch(k_mg_halfsweep<T>, grid, dim3(256), ctx->stream, l, parity); });
        if (rc) return rc;
        ++m->launches;
    }
    return FS_OK;
}

template <typename T>
static int mg_tail_launch(fs_ctx *ctx, fs_mg *m)
{
    MgTail tl;
    tl.n = m->n - m->tail;
    for (int k = 0; k < tl.n; ++k) { tl.nx[k] = m->nx[m->tail + k]; tl.ny[k] = m->ny[m->tail + k]; tl.off[k] = (int)(m->off[m->tail + k] - m->off[m->tail]); }
    tl.coarse_sweeps = m->coarse_sweeps; tl.coarsest_sweeps = m->coarsest_sweeps;
    const size_t o = m->off[m->tail], bytes = m->tail_bytes;
    const T *cx = (const T *)m->d_cx + o, *cy = (const T *)m->d_cy + o, *dg = (const T *)m->d_diag + o, *R = (const T *)m->d_R + o;
    T *E = (T *)m->d_E + o;
    ++m->launches;
    return launch(ctx, "mg_tail", [=] {
        if (kernel_notes.n < 4) kernel_notes.fn[kernel_notes.n++] = (const void *)k_mg_tail<T>;
        k_mg_tail<T><<<dim3(1), dim3(MG_TAIL_THREADS), bytes, ctx->stream>>>(tl, cx, cy, dg, R, E);
    });
}

// the last level's exact solve: one launch (none when the level has no active cell: its E stays 0)
template <typename T>
static int mg_direct_launch(fs_ctx *ctx, fs_mg *m)
{
    if (m->direct_n == 0) return FS_OK;
    const MgLevel<T> l = mg_level<T>(m, m->n - 1);
    const T *M = (const T *)m->d_M;
    const int *cells = m->d_cells;
    const int n = m->direct_n, stride = m->direct_stride;
    ++m->launches;
    return launch(ctx, "mg_direct", [=] {
        klaunch(k_mg_direct<T>, dim3((n + MG_DIRECT_ROWS - 1) / MG_DIRECT_ROWS), dim3(64 * MG_DIRECT_ROWS), ctx->stream, M, cells, (const T *)l.R, l.E, n, stride);
    });
}

// W(k, R_k): E_k is zero on entry (the kernel that wrote R_k zeroed it)
template <typename T>
static int mg_w(fs_ctx *ctx, fs_mg *m, int k)
{
    if (k == m->tail) return mg_tail_launch<T>(ctx, m);
    if (k == m->n - 1) return m->direct ? mg_direct_launch<T>(ctx, m) : mg_sweeps<T>(ctx, m, k, m->coarsest_sweeps);
    int rc = mg_sweeps<T>(ctx, m, k, m->coarse_sweeps);
    if (rc) return rc;
    const MgLevel<T> f = mg_level<T>(m, k), c = mg_level<T>(m, k + 1);
    for (int visit = 0; visit < 2; ++visit) {
        rc = launch(ctx, "mg_restrict", [=] { klaunch(k_mg_restrict<T>, mg_grid(c.nx, c.ny), dim3(256), ctx->stream, f, c.R, c.E, c.nx, c.ny); });
        if (rc) return rc;
        rc = mg_w<T>(ctx, m, k + 1);
        if (rc) return rc;
        rc = launch(ctx, "mg_prolong", [=] { klaunch(k_mg_prolong<T>, mg_grid(f.nx, f.ny), dim3(256), ctx->stream, f, (const T *)c.E, c.nx); });
        if (rc) return rc;
        m->launches += 2;
        rc = mg_sweeps<T>(ctx, m, k, m->coarse_sweeps);
        if (rc) return rc;
    }
    return FS_OK;
}

extern "C" {

int fs_mg_create(fs_ctx *ctx, int nlevels, const int *dims, const void *cx, const void *cy, const void *diag, long long tail_cells,
                 int coarse_sweeps, int coarsest_sweeps, fs_mg **out)
{
    FS_REQUIRE(ctx && dims && cx && cy && diag && out, "null argument");
    FS_REQUIRE(nlevels >= 1 && nlevels <= MG_MAX_LEVELS, "nlevels must be 1 .. 24");
    FS_REQUIRE(coarse_sweeps >= 0 && coarsest_sweeps >= 0, "sweep counts must be >= 0");
    FS_REQUIRE(ctx->halo == 0 && ctx->nyl == ctx->Y, "the multigrid updater runs on a single-GPU context (no slabs)");
    FS_REQUIRE(dims[0] * 2 == ctx->X && dims[1] * 2 == ctx->Y, "level 1 must be half the grid in both directions");
    for (int k = 1; k < nlevels; ++k)
        FS_REQUIRE(dims[2 * k] * 2 == dims[2 * k - 2] && dims[2 * k + 1] * 2 == dims[2 * k - 1] && dims[2 * k] >= 1 && dims[2 * k + 1] >= 1, "every level must be half the level above it");
    FS_NO_CAPTURE(fs_mg, "create");
    FS_HIP(hipSetDevice(ctx->device));
    auto mg = std::make_unique<fs_mg>();
    fs_mg *m = mg.get();
    m->n = nlevels; m->coarse_sweeps = coarse_sweeps; m->coarsest_sweeps = coarsest_sweeps;
    for (int k = 0; k < nlevels; ++k) {
        m->nx[k] = dims[2 * k]; m->ny[k] = dims[2 * k + 1];
        m->off[k] = m->cells;
        m->cells += (size_t)m->nx[k] * m->ny[k];
    }
    // the tail: the first level of at most `tail_cells` cells whose levels, five arrays each, fit the LDS one workgroup may have (< 0: whatever fits)
    int lds_max = 0;
    hipError_t e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device);
    if (e != hipSuccess || lds_max < 0) lds_max = 0;
    if (tail_cells != 0 && lds_max > 0) {
        for (int k = 0; k < nlevels; ++k) {
            const size_t below = m->cells - m->off[k], bytes = below * 5 * ctx->esize;
            const size_t top = (size_t)m->nx[k] * m->ny[k];
            if (bytes <= (size_t)lds_max && (tail_cells < 0 || top <= (size_t)tail_cells)) { m->tail = k; m->tail_bytes = (bytes + 7) & ~(size_t)7; break; }
        }
    }
    if (m->tail >= 0 && m->tail_bytes > 48 * 1024) {
        e = ctx->dtype == 0 ? hipFuncSetAttribute((const void *)k_mg_tail<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->tail_bytes)
                            : hipFuncSetAttribute((const void *)k_mg_tail<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->tail_bytes);
        if (e != hipSuccess) return hip_fail(e, "fs_mg_create: hipFuncSetAttribute", __FILE__, __LINE__);
    }
    const size_t bytes = m->cells * ctx->esize;
    e = m->d_E.alloc(bytes);
    if (e == hipSuccess) e = m->d_R.alloc(bytes);
    if (e == hipSuccess) e = m->d_cx.alloc(bytes);
    if (e == hipSuccess) e = m->d_cy.alloc(bytes);
    if (e == hipSuccess) e = m->d_diag.alloc(bytes);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_E, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_R, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_cx, cx, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_cy, cy, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_diag, diag, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "fs_mg_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(mg));
    return FS_OK;
}

int fs_mg_set_direct(fs_ctx *ctx, fs_mg *m, int n, const int *cells, const void *M, long long row_stride)
{
    FS_REQUIRE(ctx && m && cells && M, "null argument");
    FS_HANDLE(m);
    FS_REQUIRE(n >= 0 && n <= MG_DIRECT_MAX, "a direct solve holds 0 .. 4096 active cells");
    FS_REQUIRE(row_stride == 64ll * ((n + 63) / 64), "row_stride must be 64 * ceil(n / 64)");
    const long long level_cells = (long long)m->nx[m->n - 1] * m->ny[m->n - 1];
    for (int j = 0; j < n; ++j)
        FS_REQUIRE(cells[j] >= 0 && cells[j] < level_cells && (j == 0 || cells[j] > cells[j - 1]), "cells must be strictly ascending indices of the last level");
    if (m->tail >= 0) { set_error("a direct solve needs a hierarchy without a tail kernel (tail_cells = 0)"); return FS_ERR_STATE; }
    if (m->direct) { set_error("this hierarchy already has a direct solve"); return FS_ERR_STATE; }
    FS_NO_CAPTURE(fs_mg, "set_direct");
    FS_HIP(hipSetDevice(ctx->device));
    DevBuf<int> d_cells;      // (the hierarchy takes the two over only when both are filled)
    DevBuf<void> d_M;
    if (n > 0) {
        const size_t mbytes = (size_t)n * (size_t)row_stride * ctx->esize;
        hipError_t e = d_cells.alloc((size_t)n * sizeof(int));
        if (e == hipSuccess) e = d_M.alloc(mbytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_cells, cells, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_M, M, mbytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "fs_mg_set_direct", __FILE__, __LINE__);
    }
    m->direct = true; m->direct_n = n; m->direct_stride = (int)row_stride; m->d_cells = std::move(d_cells); m->d_M = std::move(d_M);
    return FS_OK;
}

int fs_mg_direct_info(fs_ctx *ctx, fs_mg *m, int *direct_level, int *direct_cells)
{
    FS_REQUIRE(ctx && m && direct_level && direct_cells, "null argument");
    FS_HANDLE(m);
    *direct_level = m->direct ? m->n : 0;
    *direct_cells = m->direct_n;
    return FS_OK;
}

int fs_mg_cycle(fs_ctx *ctx, fs_mg *m, double dt, double dx, fs_field *pc, fs_field *pn, const fs_field *vc)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_FIELD(pc, 1); FS_FIELD(pn, 1); FS_FIELD(vc, 2);
    FS_REQUIRE(pc != pn, "the correction needs the two distinct pressure buffers of the red-black pair");
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    m->launches = 0;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        const auto k = make_konst<T>(ctx, dt, dx, 1.0);
        const MgLevel<T> l1 = mg_level<T>(m, 0);
        int rc = launch(ctx, "mg_fine_residual", [=] {
            klaunch(k_mg_fine_residual<T>, mg_grid(l1.nx, l1.ny), dim3(256), ctx->stream, ctx->grid(), k, (const T *)pc->d, (const T *)vc->d, l1.R, l1.E, l1.nx, l1.ny);
        });
        if (rc) return rc;
        rc = mg_w<T>(ctx, m, 0);
        if (rc) return rc;
        m->launches += 2;
        return launch(ctx, "mg_fine_correct", [=] {
            klaunch(k_mg_fine_correct<T>, mg_grid(ctx->X, ctx->rows), dim3(256), ctx->stream, ctx->grid(), (T *)pc->d, (T *)pn->d, (const T *)l1.E, l1.nx);
        });
    });
}

int fs_mg_info(fs_ctx *ctx, fs_mg *m, int *levels, int *tail_level, int *launches)
{
    FS_REQUIRE(ctx && m && levels && tail_level && launches, "null argument");
    FS_HANDLE(m);
    *levels = m->n;
    *tail_level = m->tail < 0 ? 0 : m->tail + 1;
    *launches = m->launches;
    return FS_OK;
}

int fs_mg_free(fs_ctx *ctx, fs_mg *m) { return object_free(ctx, m); }

}  // extern "C"
