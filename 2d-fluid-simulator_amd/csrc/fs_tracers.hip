// fs_tracers.hip - C-ABI entry points of the tracer particles (fs_tracer.h): the sets that ride the step, their sort by cell, the per-cell
// fields, the inertial sets with wall deposits and the accumulated occupancy.
#include "fs_launch.h"
#include "fs_tracer.h"

FS_OBJECT(fs_tracer, OBJ_TRACER, "tracer", "tracer set from another context or freed");

using namespace fs;

extern "C" {

static_assert(TR_LEFT == FS_TRACER_LEFT && TR_WALL == FS_TRACER_WALL && TR_EXPIRED == FS_TRACER_EXPIRED && TRACER_SORT_W == FS_TRACER_SORT_BIN_CELLS,
              "fs_tracer.h and include/fs_hip.h disagree");

static TracerDev tracer_dev(const fs_tracer *t)
{
    const size_t n = (size_t)t->n;
    return TracerDev{t->n, t->d_pos, t->d_pos + n, t->d_int, t->d_int + n, t->d_int + 2 * n, t->d_pos + 2 * n, t->d_pos + 3 * n, t->d_count, t->d_int + 3 * n};
}

int fs_tracer_create(fs_ctx *ctx, int n, const double *seeds_xy, int respawn, int max_age, fs_tracer **out)
{
    FS_REQUIRE(ctx && seeds_xy && out, "null argument");
    FS_REQUIRE(n >= 1, "a tracer set needs at least one particle");
    FS_REQUIRE(max_age >= 0, "max_age must be >= 0");
    FS_NO_CAPTURE(fs_tracer, "create");
    if (ctx->comm || ctx->halo != 0 || ctx->y0 != 0 || ctx->nyl != ctx->Y) {
        set_error("tracer particles need a single-context grid: on slabs they would have to migrate between ranks");
        return FS_ERR_UNSUPPORTED;
    }
    // (fs_create admits no grid below 4 x 4: the corner index range [0, X - 2] x [0, Y - 2] of the interpolation is never empty)
    std::vector<double> pos(4 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const double x = seeds_xy[2 * k], y = seeds_xy[2 * k + 1];
        FS_REQUIRE(x >= 0.0 && x < (double)ctx->X && y >= 0.0 && y < (double)ctx->Y, "tracer seed outside the domain");
        pos[k] = pos[2 * (size_t)n + k] = x;
        pos[(size_t)n + k] = pos[3 * (size_t)n + k] = y;
    }
    std::vector<int> ints(4 * (size_t)n);      // age, status, respawns 0; id the identity (with the set: a graph captured before the first sort stays valid)
    for (int k = 0; k < n; ++k) ints[3 * (size_t)n + k] = k;
    FS_HIP(hipSetDevice(ctx->device));
    auto t = std::make_unique<fs_tracer>();
    t->n = n; t->respawn = respawn ? 1 : 0; t->max_age = max_age;
    const hipError_t e = fill_buffers(ctx, {{t->d_pos, pos.size() * sizeof(double), pos.data()}, {t->d_int, ints.size() * sizeof(int), ints.data()},
                                            {t->d_count, sizeof(long long)}});
    if (e != hipSuccess) return hip_fail(e, "fs_tracer_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(t));
    return FS_OK;
}

int fs_tracer_advance(fs_ctx *ctx, fs_tracer *t, double h, double limit, const fs_field *v)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_FIELD(v, 2);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launch needs is in `t` and the field: no allocation, copy or synchronisation here (the closure is captured)
    const TracerDev td = tracer_dev(t);
    const dim3 grid((t->n + TRACER_WG - 1) / TRACER_WG);
    const int Y = ctx->Y, respawn = t->respawn, max_age = t->max_age;
    if (t->inertial) {
        const size_t n = (size_t)t->n;
        const TracerInertial q{t->d_vel, t->d_vel + n, t->d_vel + 2 * n, t->d_vel + 3 * n, t->gx, t->gy, t->d_dep};
        return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
            return launch(ctx, "tracer_advance_inertial", [=] {
                if (limit > 0.0)
                    klaunch(k_tracer_advance_inertial<T, true>, grid, dim3(TRACER_WG), ctx->stream, ctx->grid(), Y, h, limit, respawn, max_age, td, q, (const T *)v->d);
                else
                    klaunch(k_tracer_advance_inertial<T, false>, grid, dim3(TRACER_WG), ctx->stream, ctx->grid(), Y, h, limit, respawn, max_age, td, q, (const T *)v->d);
            });
        });
    }
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "tracer_advance", [=] {
            if (limit > 0.0)
                klaunch(k_tracer_advance<T, true>, grid, dim3(TRACER_WG), ctx->stream, ctx->grid(), Y, h, limit, respawn, max_age, td, (const T *)v->d);
            else
                klaunch(k_tracer_advance<T, false>, grid, dim3(TRACER_WG), ctx->stream, ctx->grid(), Y, h, limit, respawn, max_age, td, (const T *)v->d);
        });
    });
}

// id (slot -> seed index) on the host, synchronised; FS_ERR_STATE when an entry lies outside 0 .. n - 1
static int tracer_ids(fs_ctx *ctx, const fs_tracer *t, const char *who, std::vector<int> &id)
{
    const size_t n = (size_t)t->n;
    id.resize(n);
    FS_HIP(hipMemcpyAsync(id.data(), t->d_int + 3 * n, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < n; ++k)
        if (id[k] < 0 || (size_t)id[k] >= n) { set_error(std::string(who) + ": the slot -> seed index array is not a permutation"); return FS_ERR_STATE; }
    return FS_OK;
}

// `rows` arrays of n doubles from slot order into seed order (out[id[k]] = in[k]) or back (out[k] = in[id[k]])
static void tracer_reorder(const std::vector<int> &id, int rows, const double *in, double *out, bool to_seed)
{
    const size_t n = id.size();
    for (int r = 0; r < rows; ++r)
        for (size_t k = 0; k < n; ++k) {
            if (to_seed) out[r * n + (size_t)id[k]] = in[r * n + k];
            else out[r * n + k] = in[r * n + (size_t)id[k]];
        }
}

int fs_tracer_read(fs_ctx *ctx, fs_tracer *t, double *pos, int *ints, long long *launches)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_NO_CAPTURE(fs_tracer, "read");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)t->n;
    if (launches) FS_HIP(hipMemcpyAsync(launches, t->d_count, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (!t->permuted || (!pos && !ints)) {
        if (pos) FS_HIP(hipMemcpyAsync(pos, t->d_pos, 4 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (ints) FS_HIP(hipMemcpyAsync(ints, t->d_int, 3 * n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(hipStreamSynchronize(ctx->stream));
        return FS_OK;
    }
    // slot order on the device, seed order for the caller: out[id[k]] = in[k] on the host (the seeds are in seed order already)
    std::vector<double> hp(pos ? 2 * n : 0);
    std::vector<int> hi((ints ? 3 * n : 0) + n);
    int *id = hi.data() + (ints ? 3 * n : 0);
    if (pos) {
        FS_HIP(hipMemcpyAsync(hp.data(), t->d_pos, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(hipMemcpyAsync(pos + 2 * n, t->d_pos + 2 * n, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (ints) FS_HIP(hipMemcpyAsync(hi.data(), t->d_int, 3 * n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemcpyAsync(id, t->d_int + 3 * n, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < n; ++k) {
        const size_t s = (size_t)id[k];
        if (id[k] < 0 || s >= n) { set_error("fs_tracer_read: the slot -> seed index array is not a permutation"); return FS_ERR_STATE; }
        if (pos) { pos[s] = hp[k]; pos[n + s] = hp[n + k]; }
        if (ints) { ints[s] = hi[k]; ints[n + s] = hi[n + k]; ints[2 * n + s] = hi[2 * n + k]; }
    }
    return FS_OK;
}

int fs_tracer_write(fs_ctx *ctx, fs_tracer *t, const double *pos, const int *ints, long long launches)
{
    FS_REQUIRE(ctx && t && pos && ints, "null argument");
    FS_HANDLE(t);
    FS_REQUIRE(launches >= 0, "launches must be >= 0");
    FS_NO_CAPTURE(fs_tracer, "write");
    const size_t n = (size_t)t->n;
    for (size_t k = 0; k < n; ++k)
        FS_REQUIRE(ints[k] >= 0 && ints[n + k] >= 0 && ints[n + k] <= 3 && ints[2 * n + k] >= 0, "tracer state: age / respawns < 0 or status outside 0 .. 3");
    FS_HIP(hipSetDevice(ctx->device));
    std::vector<double> hv;
    if (t->inertial && t->permuted) {      // pu, pw follow their particles back into seed order; alpha, tau from the host copy.  Staged
        hv.resize(4 * n);                  // on the host first: no upload is issued before the last step here that can fail
        std::vector<double> sv(2 * n);
        std::vector<int> id;
        FS_HIP(hipMemcpyAsync(sv.data(), t->d_vel, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        int rc = tracer_ids(ctx, t, "fs_tracer_write", id); if (rc) return rc;
        tracer_reorder(id, 2, sv.data(), hv.data(), true);
        std::copy(t->h_resp.begin(), t->h_resp.end(), hv.begin() + 2 * n);
    }
    if (!hv.empty()) FS_HIP(hipMemcpyAsync(t->d_vel, hv.data(), 4 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(t->d_pos, pos, 4 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(t->d_int, ints, 3 * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(t->d_count, &launches, sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int> ident;
    if (t->permuted) {      // the state arrives in seed order: slot k holds seed k again
        ident.resize(n);
        for (size_t k = 0; k < n; ++k) ident[k] = (int)k;
        FS_HIP(hipMemcpyAsync(t->d_int + 3 * n, ident.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (the sources are the caller's / this frame's memory)
    t->permuted = false;
    return FS_OK;
}

// Scratch of the sort, allocated at the first one: the arrays in the new order, the keys and the bins.
static int tracer_sort_scratch(fs_ctx *ctx, fs_tracer *t)
{
    if (t->d_bins) return FS_OK;
    const size_t n = (size_t)t->n;
    const int NB = (ctx->X + TRACER_SORT_W - 1) / TRACER_SORT_W;
    FS_REQUIRE((long long)ctx->Y * NB + 1 < (1ll << 30), "grid too large for the tracer sort");
    const int nbins = ctx->Y * NB + 1, nblocks = (nbins + TRACER_SCAN_TILE - 1) / TRACER_SCAN_TILE;
    hipError_t e = t->d_spos.alloc(2 * n * sizeof(double));
    if (e == hipSuccess) e = t->d_sint.alloc(5 * n * sizeof(int));
    if (e == hipSuccess && t->inertial) e = t->d_svel.alloc(4 * n * sizeof(double));
    if (e == hipSuccess) e = t->d_bins.alloc(((size_t)nbins + nblocks) * sizeof(int));
    if (e != hipSuccess) {      // (all or nothing: d_bins stays null, the next sort tries again)
        t->d_spos.reset(); t->d_sint.reset(); t->d_svel.reset();
        return hip_fail(e, "fs_tracer_sort (scratch)", __FILE__, __LINE__);
    }
    t->nbins = nbins; t->nblocks = nblocks;
    return FS_OK;
}

int fs_tracer_sort(fs_ctx *ctx, fs_tracer *t)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_NO_CAPTURE(fs_tracer, "sort");
    FS_HIP(hipSetDevice(ctx->device));
    int rc = tracer_sort_scratch(ctx, t); if (rc) return rc;
    const TracerDev td = tracer_dev(t);
    const size_t n = (size_t)t->n;
    const int X = ctx->X, Y = ctx->Y, NB = (X + TRACER_SORT_W - 1) / TRACER_SORT_W, nbins = t->nbins, nblocks = t->nblocks;
    const dim3 grid((t->n + TRACER_WG - 1) / TRACER_WG), wg(TRACER_WG);
    double *sx = t->d_spos, *sy = t->d_spos + n;
    int *si = t->d_sint, *key = t->d_sint + 4 * n, *bins = t->d_bins, *sums = t->d_bins + nbins;
    hipStream_t st = ctx->stream;
    FS_HIP(hipMemsetAsync(bins, 0, (size_t)nbins * sizeof(int), st));      // (a failed zeroing must not pass for a sort)
    rc = launch(ctx, "tracer_sort_count", [=] {
        klaunch(k_tracer_sort_count, grid, wg, st, X, Y, NB, td, key, bins);
    });
    if (rc) return rc;
    rc = launch(ctx, "tracer_sort_scan", [=] {
        klaunch(k_tracer_scan_blocks, dim3(nblocks), wg, st, nbins, bins, sums);
        klaunch(k_tracer_scan_sums, dim3(1), wg, st, nblocks, sums);
        klaunch(k_tracer_scan_add, dim3((nbins + TRACER_WG - 1) / TRACER_WG), wg, st, nbins, bins, (const int *)sums);
    });
    if (rc) return rc;
    double *vel = t->d_vel, *sv = t->d_svel;
    const bool carry = t->inertial;
    rc = launch(ctx, "tracer_sort_scatter", [=] {
        if (carry) klaunch(k_tracer_sort_scatter_inertial, grid, wg, st, td, (const int *)key, bins, sx, sy, si, (const double *)vel, sv);
        else klaunch(k_tracer_sort_scatter, grid, wg, st, td, (const int *)key, bins, sx, sy, si);
    });
    if (rc) return rc;
    rc = launch(ctx, "tracer_sort_copy", [=] {
        if (carry) klaunch(k_tracer_sort_copy_inertial, grid, wg, st, td, (const double *)sx, (const double *)sy, (const int *)si, vel, (const double *)sv);
        else klaunch(k_tracer_sort_copy, grid, wg, st, td, (const double *)sx, (const double *)sy, (const int *)si);
    });
    if (rc) return rc;
    t->permuted = true;
    return FS_OK;
}

int fs_tracer_order(fs_ctx *ctx, fs_tracer *t, int *ids)
{
    FS_REQUIRE(ctx && t && ids, "null argument");
    FS_HANDLE(t);
    FS_NO_CAPTURE(fs_tracer, "order");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(ids, t->d_int + 3 * (size_t)t->n, (size_t)t->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_tracer_fields(fs_ctx *ctx, fs_tracer *t, int *count, long long *age_sum)
{
    FS_REQUIRE(ctx && t && count && age_sum, "null argument");
    FS_HANDLE(t);
    FS_NO_CAPTURE(fs_tracer, "fields");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ctx->X * ctx->Y;
    // one allocation for the call: the 8-byte sums first, then the counts
    unsigned long long *d_age = nullptr;
    FS_HIP(hipMalloc(&d_age, cells * (sizeof(unsigned long long) + sizeof(int))));
    int *d_cnt = (int *)(d_age + cells);
    const TracerDev td = tracer_dev(t);
    const dim3 grid((t->n + TRACER_WG - 1) / TRACER_WG);
    const int X = ctx->X, Y = ctx->Y;
    hipStream_t st = ctx->stream;
    const hipError_t ez = hipMemsetAsync(d_age, 0, cells * (sizeof(unsigned long long) + sizeof(int)), st);
    if (ez != hipSuccess) { hipFree(d_age); return hip_fail(ez, "fs_tracer_fields (zeroing)", __FILE__, __LINE__); }
    int rc = launch(ctx, "tracer_fields", [=] {
        klaunch(k_tracer_fields, grid, dim3(TRACER_WG), st, X, Y, td, d_cnt, d_age);
    });
    hipError_t e = hipSuccess;
    if (rc == FS_OK) {
        e = hipMemcpyAsync(count, d_cnt, cells * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(age_sum, d_age, cells * sizeof(long long), hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);
    hipFree(d_age);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "fs_tracer_fields (download)", __FILE__, __LINE__);
    if (es != hipSuccess) return hip_fail(es, "fs_tracer_fields", __FILE__, __LINE__);
    return FS_OK;
}

int fs_tracer_draw(fs_ctx *ctx, fs_tracer *t, double r, double g, double b, fs_field *rgb)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_FIELD(rgb, 3);
    const TracerDev td = tracer_dev(t);
    const dim3 grid((t->n + TRACER_WG - 1) / TRACER_WG);
    const int Y = ctx->Y;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "tracer_draw", [=] {
            klaunch(k_tracer_draw<T>, grid, dim3(TRACER_WG), ctx->stream, ctx->grid(), Y, td, (T)r, (T)g, (T)b, (T *)rgb->d);
        });
    });
}

// ---- inertial sets ------------------------------------------------------------------------------------------
int fs_tracer_create_inertial(fs_ctx *ctx, int n, const double *seeds_xy, const double *alpha, const double *tau, double gx, double gy, int respawn,
                              int max_age, int deposits, fs_tracer **out)
{
    FS_REQUIRE(ctx && seeds_xy && alpha && tau && out, "null argument");
    FS_REQUIRE(n >= 1, "a tracer set needs at least one particle");
    FS_REQUIRE(std::isfinite(gx) && std::isfinite(gy), "gravity must be finite");
    for (int k = 0; k < n; ++k) {
        FS_REQUIRE(alpha[k] > 0.0 && alpha[k] <= 1.0, "alpha must lie in (0, 1]");
        FS_REQUIRE(tau[k] >= 0.0 && std::isfinite(tau[k]), "tau must be finite and >= 0");
    }
    fs_tracer *t = nullptr;
    int rc = fs_tracer_create(ctx, n, seeds_xy, respawn, max_age, &t);
    if (rc) return rc;
    const size_t N = (size_t)n, cells = (size_t)ctx->X * ctx->Y;
    std::vector<double> vel(4 * N, 0.0);
    std::copy(alpha, alpha + N, vel.begin() + 2 * N);
    std::copy(tau, tau + N, vel.begin() + 3 * N);
    const hipError_t e = fill_buffers(ctx, {{t->d_vel, vel.size() * sizeof(double), vel.data()}, {t->d_dep, deposits ? cells * sizeof(int) : 0}});
    if (e != hipSuccess) { object_free(ctx, t); return hip_fail(e, "fs_tracer_create_inertial", __FILE__, __LINE__); }
    t->inertial = true; t->gx = gx; t->gy = gy;
    t->h_resp.assign(vel.begin() + 2 * N, vel.end());
    *out = t;
    return FS_OK;
}

#define FS_TRACER_INERTIAL(t) FS_REQUIRE((t)->inertial, "not an inertial tracer set (fs_tracer_create_inertial)")

int fs_tracer_read_vel(fs_ctx *ctx, fs_tracer *t, double *vel)
{
    FS_REQUIRE(ctx && t && vel, "null argument");
    FS_HANDLE(t);
    FS_TRACER_INERTIAL(t);
    FS_NO_CAPTURE(fs_tracer, "read_vel");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)t->n;
    if (!t->permuted) {
        FS_HIP(hipMemcpyAsync(vel, t->d_vel, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(hipStreamSynchronize(ctx->stream));
        return FS_OK;
    }
    std::vector<double> sv(2 * n);
    std::vector<int> id;
    FS_HIP(hipMemcpyAsync(sv.data(), t->d_vel, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    int rc = tracer_ids(ctx, t, "fs_tracer_read_vel", id); if (rc) return rc;
    tracer_reorder(id, 2, sv.data(), vel, true);
    return FS_OK;
}

int fs_tracer_write_vel(fs_ctx *ctx, fs_tracer *t, const double *vel)
{
    FS_REQUIRE(ctx && t && vel, "null argument");
    FS_HANDLE(t);
    FS_TRACER_INERTIAL(t);
    FS_NO_CAPTURE(fs_tracer, "write_vel");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)t->n;
    if (!t->permuted) {
        FS_HIP(hipMemcpyAsync(t->d_vel, vel, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(hipStreamSynchronize(ctx->stream));      // (the source is the caller's memory)
        return FS_OK;
    }
    std::vector<double> sv(2 * n);
    std::vector<int> id;
    int rc = tracer_ids(ctx, t, "fs_tracer_write_vel", id); if (rc) return rc;
    tracer_reorder(id, 2, vel, sv.data(), false);
    FS_HIP(hipMemcpyAsync(t->d_vel, sv.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_tracer_deposits(fs_ctx *ctx, fs_tracer *t, int *out)
{
    FS_REQUIRE(ctx && t && out, "null argument");
    FS_HANDLE(t);
    FS_REQUIRE(t->d_dep, "the tracer set records no deposits (fs_tracer_create_inertial with deposits != 0)");
    FS_NO_CAPTURE(fs_tracer, "deposits");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(out, t->d_dep, (size_t)ctx->X * ctx->Y * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_tracer_deposits_write(fs_ctx *ctx, fs_tracer *t, const int *in)
{
    FS_REQUIRE(ctx && t && in, "null argument");
    FS_HANDLE(t);
    FS_REQUIRE(t->d_dep, "the tracer set records no deposits (fs_tracer_create_inertial with deposits != 0)");
    FS_NO_CAPTURE(fs_tracer, "deposits_write");
    const size_t cells = (size_t)ctx->X * ctx->Y;
    for (size_t c = 0; c < cells; ++c) FS_REQUIRE(in[c] >= 0, "deposit counts must be >= 0");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(t->d_dep, in, cells * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (the source is the caller's memory)
    return FS_OK;
}

// ---- accumulated occupancy ----------------------------------------------------------------------------------
#define FS_TRACER_ACCUM(t) FS_REQUIRE((t)->d_acc, "the tracer set has no accumulator (fs_tracer_accum_create)")

int fs_tracer_accum_create(fs_ctx *ctx, fs_tracer *t, long long every, long long start)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_tracer, "accum_create");
    if (t->d_acc) { set_error("the tracer set has an accumulator already: fs_tracer_accum_free first"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ctx->X * ctx->Y;
    hipError_t e = fill_buffers(ctx, {{t->d_acc, 2 * cells * sizeof(unsigned long long)}, {t->d_acc_state, 2 * sizeof(long long)}});
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_acc_state, t->d_count, sizeof(long long), hipMemcpyDeviceToDevice, ctx->stream);      // base
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { t->d_acc.reset(); t->d_acc_state.reset(); return hip_fail(e, "fs_tracer_accum_create", __FILE__, __LINE__); }
    t->acc_every = every; t->acc_start = start;
    return FS_OK;
}

int fs_tracer_accum_add(fs_ctx *ctx, fs_tracer *t)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_TRACER_ACCUM(t);
    const TracerDev td = tracer_dev(t);
    const dim3 grid((t->n + TRACER_WG - 1) / TRACER_WG);
    const int X = ctx->X, Y = ctx->Y;
    const long long every = t->acc_every, start = t->acc_start;
    long long *state = t->d_acc_state;
    unsigned long long *occ = t->d_acc, *age = t->d_acc + (size_t)X * Y;
    return launch(ctx, "tracer_accumulate", [=] {
        klaunch(k_tracer_accumulate, grid, dim3(TRACER_WG), ctx->stream, X, Y, td, start, every, state, occ, age);
    });
}

int fs_tracer_accum_read(fs_ctx *ctx, fs_tracer *t, long long *occupancy, long long *age_sum, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_TRACER_ACCUM(t);
    FS_NO_CAPTURE(fs_tracer, "accum_read");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ctx->X * ctx->Y;
    long long st[2] = {0, 0}, count = 0;
    if (occupancy) FS_HIP(hipMemcpyAsync(occupancy, t->d_acc, cells * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (age_sum) FS_HIP(hipMemcpyAsync(age_sum, t->d_acc + cells, cells * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemcpyAsync(st, t->d_acc_state, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemcpyAsync(&count, t->d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    if (launches) *launches = count - st[0];
    if (samples) *samples = st[1];
    return FS_OK;
}

int fs_tracer_accum_write(fs_ctx *ctx, fs_tracer *t, const long long *occupancy, const long long *age_sum, long long launches, long long samples)
{
    FS_REQUIRE(ctx && t && occupancy && age_sum, "null argument");
    FS_HANDLE(t);
    FS_TRACER_ACCUM(t);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_tracer, "accum_write");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ctx->X * ctx->Y;
    for (size_t c = 0; c < cells; ++c) FS_REQUIRE(occupancy[c] >= 0 && age_sum[c] >= 0, "accumulated counts must be >= 0");
    long long count = 0;
    FS_HIP(hipMemcpyAsync(&count, t->d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    FS_REQUIRE(launches <= count, "the accumulator cannot be older than the set: launches exceeds the set's launch count (fs_tracer_write first)");
    const long long st[2] = {count - launches, samples};
    FS_HIP(hipMemcpyAsync(t->d_acc, occupancy, cells * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(t->d_acc + cells, age_sum, cells * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipMemcpyAsync(t->d_acc_state, st, sizeof st, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (the sources are the caller's / this frame's memory)
    return FS_OK;
}

int fs_tracer_accum_reset(fs_ctx *ctx, fs_tracer *t)
{
    FS_REQUIRE(ctx && t, "null argument");
    FS_HANDLE(t);
    FS_TRACER_ACCUM(t);
    FS_NO_CAPTURE(fs_tracer, "accum_reset");
    // (the base stays: the phase runs on; this reset returns with the stream idle)
    return counted_reset(ctx, t->d_acc_state, dense_zero(ctx, t->d_acc, 2 * (size_t)ctx->X * ctx->Y * sizeof(unsigned long long)), true);
}

int fs_tracer_accum_free(fs_ctx *ctx, fs_tracer *t)
{
    if (!t) return FS_OK;
    FS_HANDLE(t);
    if (!t->d_acc) return FS_OK;
    if (ctx->capturing) {      // (no synchronisation / hipFree inside a capture: the two buffers move onto the deferred list)
        ctx->objects.deferred.push_back([acc = t->d_acc.release(), state = t->d_acc_state.release()] { hipFree(acc); hipFree(state); });
        return FS_OK;
    }
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    t->d_acc.reset(); t->d_acc_state.reset();
    return FS_OK;
}

int fs_tracer_free(fs_ctx *ctx, fs_tracer *t) { return object_free(ctx, t); }

}  // extern "C"
