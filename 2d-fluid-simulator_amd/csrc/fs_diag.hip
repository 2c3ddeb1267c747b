// fs_diag.hip - C-ABI entry points of what reads the flow without changing it: the flow diagnostics (fs_stats.h), the per-step history ring
// (fs_history.h), the body surface loads (fs_loads.h), the time averages (fs_mean.h), the harmonic modes (fs_modes.h), the snapshot POD
// (fs_pod.h), the flow maps through its snapshots (fs_lcs.h), the vortex identification (fs_vortex.h), the field distributions (fs_dist.h), the energy spectra (fs_spec.h), the cross-spectra (fs_xspec.h), the scale-to-scale fluxes (fs_flux.h) and the kinetic-energy budget (fs_budget.h).  Their objects live in the context's
// registry (fs_host.h: FS_OBJECT, FS_HANDLE, FS_NO_CAPTURE, object_free).  What the accumulators share on the host is there as well: fill_buffers
// builds every object, counted_read / counted_set / counted_reset move a payload behind its counters, FS_BOX checks a cell box, and the two
// spectral riders are one SpecPlan each (spec_plan_create, spec_forward, spec_finish below).  An entry point keeps its own argument checks, in its
// own order, and its kernels.
#include "fs_launch.h"
#include "fs_stats.h"
#include "fs_mean.h"
#include "fs_modes.h"
#include "fs_pod.h"
#include "fs_lcs.h"
#include "fs_loads.h"
#include "fs_vortex.h"
#include "fs_dist.h"
#include "fs_spec.h"
#include "fs_xspec.h"
#include "fs_flux.h"
#include "fs_budget.h"

static_assert(fs::STATS_N == FS_FLOW_NSTAT, "fs_stats.h and include/fs_hip.h disagree on the slots");
static_assert(fs::LOADS_REC == FS_LOADS_NREC && fs::LOADS_SUMS == FS_LOADS_NSUM, "fs_loads.h and include/fs_hip.h disagree on the record / the sums");
static_assert(fs::MEAN_PLANES == FS_MEAN_NPLANE, "fs_mean.h and include/fs_hip.h disagree on the planes");
static_assert(fs::MODES_MAX_FREQ == FS_MODES_MAX_FREQ && fs::modes_scalars(FS_MODES_MAX_FREQ) == FS_MODES_NSCALAR(FS_MODES_MAX_FREQ),
              "fs_modes.h and include/fs_hip.h disagree on the frequencies / the scalars");

static_assert(fs::POD_MAX == FS_POD_MAX, "fs_pod.h and include/fs_hip.h disagree on the slots");
static_assert(fs::FM_LEFT == FS_TRACER_LEFT && fs::FM_WALL == FS_TRACER_WALL && fs::FM_UNSEEDED == FS_FLOWMAP_UNSEEDED && fs::FM_MAX_SUBSTEPS == FS_FLOWMAP_MAX_SUBSTEPS, "fs_lcs.h and include/fs_hip.h disagree");

static_assert(fs::VX_NACC == FS_VORTEX_NACC && fs::VX_REC == FS_VORTEX_NREC && fs::VX_HEAD == FS_VORTEX_NHEAD && fs::VX_MAX_VORTICES == FS_VORTEX_MAX_VORTICES,
              "fs_vortex.h and include/fs_hip.h disagree");

static_assert(fs::DIST_MAX_BINS == FS_DIST_MAX_BINS && fs::DIST_MAX_CHANNELS == FS_DIST_MAX_CHANNELS && fs::DIST_MAX_RANKS == FS_DIST_MAX_RANKS && fs::DIST_TAILS == FS_DIST_NTAIL,
              "fs_dist.h and include/fs_hip.h disagree");
static_assert(fs::SPEC_MIN_N == FS_SPEC_MIN_N && fs::SPEC_MAX_N == FS_SPEC_MAX_N, "fs_spec.h and include/fs_hip.h disagree");
static_assert(fs::XSPEC_PLANES == FS_XSPEC_NPLANE && fs::XSPEC_NQ == fs::DIST_NQ, "fs_xspec.h, fs_dist.h and include/fs_hip.h disagree");
static_assert(fs::FLUX_NQ == FS_FLUX_NQ && fs::FLUX_SUMS == FS_FLUX_NSUM && fs::FLUX_MAX_WIDTHS == FS_FLUX_MAX_WIDTHS && fs::FLUX_MAX_R == FS_FLUX_MAX_R,
              "fs_flux.h and include/fs_hip.h disagree");
static_assert(fs::BUDGET_PLANES == FS_BUDGET_NPLANE, "fs_budget.h and include/fs_hip.h disagree on the planes");

FS_OBJECT(fs_history, OBJ_HISTORY, "history", "history from another context or freed");
FS_OBJECT(fs_loads, OBJ_LOADS, "loads", "loads from another context or freed");
FS_OBJECT(fs_mean, OBJ_MEAN, "mean", "mean from another context or freed");
FS_OBJECT(fs_modes, OBJ_MODES, "modes", "modes from another context or freed");
FS_OBJECT(fs_pod, OBJ_POD, "pod", "pod from another context or freed");
FS_OBJECT(fs_vortex, OBJ_VORTEX, "vortex", "vortex tracker from another context or freed");
FS_OBJECT(fs_dist, OBJ_DIST, "distributions", "distributions from another context or freed");
FS_OBJECT(fs_spec, OBJ_SPEC, "spectrum", "spectrum from another context or freed");
FS_OBJECT(fs_xspec, OBJ_XSPEC, "cross-spectrum", "cross-spectrum from another context or freed");
FS_OBJECT(fs_flux, OBJ_FLUX, "scale fluxes", "scale fluxes from another context or freed");
FS_OBJECT(fs_budget, OBJ_BUDGET, "budget", "budget from another context or freed");
FS_OBJECT(fs_flowmap, OBJ_FLOWMAP, "flow map", "flow map from another context or freed");

using namespace fs;

// `planes` planes of nyl rows, elements of `es` bytes: device rows of pitch P (planes `plane` elements apart) <-> dense host rows of X.  Queued on the
// stream; the caller synchronises
static int copy_planes(fs_ctx *ctx, int planes, size_t es, void *dev, size_t plane, void *host, hipMemcpyKind kind)
{
    const size_t dense = (size_t)ctx->nyl * ctx->X * es, wp = (size_t)ctx->P * es, wx = (size_t)ctx->X * es, ny = (size_t)ctx->nyl;
    for (int k = 0; k < planes; ++k) {
        char *d = (char *)dev + k * plane * es, *h = (char *)host + k * dense;
        if (kind == hipMemcpyDeviceToHost) FS_HIP(hipMemcpy2DAsync(h, wx, d, wp, wx, ny, kind, ctx->stream));
        else FS_HIP(hipMemcpy2DAsync(d, wp, h, wx, wx, ny, kind, ctx->stream));
    }
    return FS_OK;
}
// ... as the callable of counted_read / counted_set
static auto planes_copy(fs_ctx *ctx, int planes, size_t es, void *dev, size_t plane, const void *host, hipMemcpyKind kind)
{
    return [=] { return copy_planes(ctx, planes, es, dev, plane, const_cast<void *>(host), kind); };
}

extern "C" {

// rows per workgroup of k_flow_stats: STATS_G on small grids, up to STATS_ROWS (fs_launch.h diag_rows)
static int stats_rows(const fs_ctx *ctx) { return diag_rows(ctx, (ctx->X + 255) / 256, ctx->nyl, STATS_G, STATS_ROWS); }

int fs_flow_stats(fs_ctx *ctx, double dx, const fs_field *v, const fs_field *p, const int *box, double *out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (ctx->capturing || ctx->tape_rec) { set_error("flow stats during graph capture / tape recording"); return FS_ERR_STATE; }
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    int b[4] = {0, 0, 0, 0};      // empty box: no force
    if (box) {
        FS_REQUIRE(0 <= box[0] && box[0] <= box[2] && box[2] <= ctx->X && 0 <= box[1] && box[1] <= box[3] && box[3] <= ctx->Y,
                   "body box must satisfy 0 <= x0 <= x1 <= X and 0 <= y0 <= y1 <= Y");
        for (int k = 0; k < 4; ++k) b[k] = box[k];
    }
    const int row_begin = ctx->halo, row_end = ctx->halo + ctx->nyl;
    const int nx = (ctx->X + 255) / 256, ny = row_end - row_begin;
    const int rpw = stats_rows(ctx);
    const dim3 grid(nx, (ny + rpw - 1) / rpw);
    const size_t nblocks = (size_t)grid.x * grid.y;
    if (nblocks + 1 > ctx->stats_cap) {
        if (ctx->d_stats) { FS_HIP(hipStreamSynchronize(ctx->stream)); FS_HIP(hipFree(ctx->d_stats)); ctx->d_stats = nullptr; ctx->stats_cap = 0; }
        FS_HIP(hipMalloc(&ctx->d_stats, (nblocks + 1) * STATS_N * sizeof(double)));
        ctx->stats_cap = nblocks + 1;
    }
    double *partial = ctx->d_stats, *total = ctx->d_stats + nblocks * STATS_N;
    const int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "flow_stats", [=] {
            klaunch(k_flow_stats<T>, grid, dim3(256), ctx->stream, ctx->grid(), row_begin, row_end, rpw, dx, b[0], b[1], b[2], b[3],
                       (const T *)v->d, (const T *)p->d, partial);
            klaunch(k_flow_stats_final, dim3(1), dim3(256), ctx->stream, (const double *)partial, (int)nblocks, total);
        });
    });
    if (rc) return rc;
    FS_HIP(hipMemcpyAsync(out, total, STATS_N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_history_create(fs_ctx *ctx, int npoints, const int *points, int nfaces, const int *faces, int capacity, int every, fs_history **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(npoints >= 0 && nfaces >= 0 && (points || npoints == 0) && (faces || nfaces == 0), "bad point / face list");
    FS_REQUIRE(capacity >= 1 && every >= 1, "capacity and every must be >= 1");
    FS_REQUIRE((2 + 3 * (long long)npoints) * capacity < (1LL << 40), "ring too large");
    FS_NO_CAPTURE(fs_history, "create");
    // a probe / face outside the owned rows would read a ghost row (stale between exchanges) or count a face twice across slabs
    const int jo = ctx->y0, je = ctx->y0 + ctx->nyl;
    auto local = [&](int x, int y) -> long long { return (long long)(y - ctx->y0 + ctx->halo) * ctx->P + x; };      // row-major element of (x, y)
    std::vector<HistProbe> hp(npoints);
    for (int k = 0; k < npoints; ++k) {
        const int x = points[2 * k], y = points[2 * k + 1];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "probe outside this context's owned rows");
        const int j = y - ctx->y0 + ctx->halo;
        hp[k].u = (unsigned)(((long long)j * 2 + 0) * ctx->P + x);      // fs_device.h idx<2>
        hp[k].w = (unsigned)(((long long)j * 2 + 1) * ctx->P + x);
        hp[k].p = (unsigned)local(x, y);
    }
    std::vector<HistFace> hf(nfaces);
    for (int k = 0; k < nfaces; ++k) {
        const int x = faces[3 * k], y = faces[3 * k + 1], d = faces[3 * k + 2];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "face outside this context's owned rows");
        FS_REQUIRE(0 <= d && d <= 3, "face direction must be 0 (+x), 1 (-x), 2 (+y) or 3 (-y)");
        hf[k].p = (unsigned)local(x, y);
        hf[k].dir = d;
    }
    FS_HIP(hipSetDevice(ctx->device));
    auto h = std::make_unique<fs_history>();
    h->np = npoints; h->nf = nfaces; h->cap = capacity; h->every = every;
    h->nparts = nfaces > HIST_SPLIT ? (nfaces + HIST_FACES_PER_WG - 1) / HIST_FACES_PER_WG : 0;
    const size_t ring = (size_t)capacity * (2 + 3 * (size_t)npoints) * sizeof(double);
    // (an empty list still gets a buffer, of one zeroed entry)
    const hipError_t e = fill_buffers(ctx, {{h->d_state, HIST_STATE * sizeof(long long)}, {h->d_ring, ring},
                                            {h->d_partial, 2 * (size_t)h->nparts * sizeof(double)},
                                            {h->d_probes, std::max<size_t>(1, hp.size()) * sizeof(HistProbe), npoints ? hp.data() : nullptr},
                                            {h->d_faces, std::max<size_t>(1, hf.size()) * sizeof(HistFace), nfaces ? hf.data() : nullptr}});
    if (e != hipSuccess) return hip_fail(e, "fs_history_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(h));
    return FS_OK;
}

int fs_history_record(fs_ctx *ctx, fs_history *h, double dx, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && h, "null argument");
    FS_HANDLE(h);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    // everything the launch needs is in `h` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const HistProbe *pr = h->d_probes;
    const HistFace *fc = h->d_faces;
    const int np = h->np, nf = h->nf, every = h->every, cap = h->cap, threads = h->threads, nparts = h->nparts;
    double *ring = h->d_ring, *partial = h->d_partial;
    long long *state = h->d_state;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "history_record", [=] {
            if (nparts)
                klaunch(k_history_faces<T>, dim3(nparts), dim3(HIST_FACES_PER_WG), ctx->stream, (const T *)p->d, fc, nf, dx, every, cap,
                           (const long long *)state, partial);
            klaunch(k_history_record<T>, dim3(1), dim3(threads), ctx->stream, (const T *)v->d, (const T *)p->d, pr, np, fc, nf,
                       (const double *)partial, nparts, dx, limit, every, cap, ring, state);
        });
    });
}

int fs_history_read(fs_ctx *ctx, fs_history *h, double *out, int max_records, int *n_records, long long *launches, int *dropped)
{
    FS_REQUIRE(ctx && h && n_records, "null argument");
    FS_HANDLE(h);
    FS_NO_CAPTURE(fs_history, "read");
    long long st[HIST_STATE];
    if (int rc = read_counters(ctx, h->d_state, st)) return rc;
    *n_records = (int)st[1];
    if (launches) *launches = st[0];
    if (dropped) *dropped = (int)st[2];
    if (!out) return FS_OK;
    FS_REQUIRE(max_records >= st[1], "out holds fewer records than the ring");
    if (st[1] > 0)
        FS_HIP(hipMemcpyAsync(out, h->d_ring, (size_t)st[1] * (2 + 3 * (size_t)h->np) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemsetAsync(h->d_state + 1, 0, 2 * sizeof(long long), ctx->stream));       // written, dropped; the launch count runs on
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_history_free(fs_ctx *ctx, fs_history *h) { return object_free(ctx, h); }

// ---- body surface loads (fs_loads.h) -----------------------------------------------------------------------------------------------------

int fs_loads_create(fs_ctx *ctx, int nfaces, const int *faces, const double *centre_xy, int capacity, long long every, long long start,
                    fs_loads **out)
{
    FS_REQUIRE(ctx && out && faces && centre_xy, "null argument");
    FS_REQUIRE(nfaces >= 1, "nfaces must be >= 1");
    FS_REQUIRE(capacity >= 1 && every >= 1 && start >= 0, "capacity and every must be >= 1 and start >= 0");
    FS_REQUIRE(std::isfinite(centre_xy[0]) && std::isfinite(centre_xy[1]), "the centre must be finite");
    FS_NO_CAPTURE(fs_loads, "create");
    // a face outside the owned rows would read a ghost row (stale between exchanges) or be counted twice across slabs
    const int jo = ctx->y0, je = ctx->y0 + ctx->nyl;
    const double cx = centre_xy[0], cy = centre_xy[1];
    std::vector<LoadFace> lf(nfaces);
    for (int k = 0; k < nfaces; ++k) {
        const int x = faces[3 * k], y = faces[3 * k + 1], d = faces[3 * k + 2];
        FS_REQUIRE(0 <= x && x < ctx->X && jo <= y && y < je, "face outside this context's owned rows");
        FS_REQUIRE(0 <= d && d <= 3, "face direction must be 0 (+x), 1 (-x), 2 (+y) or 3 (-y)");
        const long long j = y - ctx->y0 + ctx->halo;
        lf[k].u = (unsigned)((j * 2 + 0) * ctx->P + x);      // fs_device.h idx<2>
        lf[k].w = (unsigned)((j * 2 + 1) * ctx->P + x);
        lf[k].p = (unsigned)(j * ctx->P + x);
        lf[k].dir = d;
        const double xm = d == 0 ? (double)x : d == 1 ? (double)x + 1.0 : (double)x + 0.5;      // the face midpoint, cell units
        const double ym = d == 2 ? (double)y : d == 3 ? (double)y + 1.0 : (double)y + 0.5;
        lf[k].rx = xm - cx;
        lf[k].ry = ym - cy;
    }
    FS_HIP(hipSetDevice(ctx->device));
    auto l = std::make_unique<fs_loads>();
    l->nf = nfaces; l->cap = capacity; l->every = every; l->start = start;
    l->nparts = nfaces > LOADS_SPLIT ? (nfaces + LOADS_WG - 1) / LOADS_WG : 0;
    const size_t ring = (size_t)capacity * LOADS_REC * sizeof(double), sums = (size_t)LOADS_SUMS * nfaces * sizeof(double);
    const hipError_t e = fill_buffers(ctx, {{l->d_state, LOADS_STATE * sizeof(long long)}, {l->d_ring, ring}, {l->d_sums, sums},
                                            {l->d_partial, (size_t)LOADS_REC * l->nparts * sizeof(double)},
                                            {l->d_faces, lf.size() * sizeof(LoadFace), lf.data()}});
    if (e != hipSuccess) return hip_fail(e, "fs_loads_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(l));
    return FS_OK;
}

int fs_loads_record(fs_ctx *ctx, fs_loads *l, double dx, double inv_re, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && l, "null argument");
    FS_HANDLE(l);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    // everything the launches need is in `l` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const LoadFace *fc = l->d_faces;
    const int nf = l->nf, cap = l->cap, nparts = l->nparts;
    const size_t stride = (size_t)l->nf;
    const long long every = l->every, start = l->start;
    double *sums = l->d_sums, *ring = l->d_ring, *partial = l->d_partial;
    long long *state = l->d_state;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "loads_record", [=] {
            if (nparts) {
                klaunch(k_loads_faces<T>, dim3(nparts), dim3(LOADS_WG), ctx->stream, (const T *)v->d, (const T *)p->d, fc, nf, stride, dx,
                           inv_re, limit, start, every, (const long long *)state, sums, partial);
                klaunch(k_loads_record, dim3(1), dim3(LOADS_WG), ctx->stream, (const double *)partial, nparts, start, every, cap, ring, state);
            } else {
                klaunch(k_loads_one<T>, dim3(1), dim3(LOADS_WG), ctx->stream, (const T *)v->d, (const T *)p->d, fc, nf, stride, dx, inv_re,
                           limit, start, every, cap, sums, ring, state);
            }
        });
    });
}

int fs_loads_read(fs_ctx *ctx, fs_loads *l, double *ring_out, int max_records, int *n_records, long long *launches, long long *samples,
                  int *dropped)
{
    FS_REQUIRE(ctx && l && n_records, "null argument");
    FS_HANDLE(l);
    FS_NO_CAPTURE(fs_loads, "read");
    long long st[LOADS_STATE];
    if (int rc = read_counters(ctx, l->d_state, st)) return rc;
    *n_records = (int)st[2];
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    if (dropped) *dropped = (int)st[3];
    if (!ring_out) return FS_OK;
    FS_REQUIRE(max_records >= st[2], "ring_out holds fewer records than the ring");
    if (st[2] > 0)
        FS_HIP(hipMemcpyAsync(ring_out, l->d_ring, (size_t)st[2] * LOADS_REC * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemsetAsync(l->d_state + 2, 0, 2 * sizeof(long long), ctx->stream));       // written, dropped; launches and samples run on
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_loads_sums_read(fs_ctx *ctx, fs_loads *l, double *sums_out)
{
    FS_REQUIRE(ctx && l && sums_out, "null argument");
    FS_HANDLE(l);
    FS_NO_CAPTURE(fs_loads, "sums_read");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(sums_out, l->d_sums, (size_t)LOADS_SUMS * l->nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_loads_sums_write(fs_ctx *ctx, fs_loads *l, const double *sums_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && l && sums_in, "null argument");
    FS_HANDLE(l);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_loads, "sums_write");
    return counted_set(ctx, l->d_state, launches, samples,
                       dense_copy(ctx, l->d_sums, sums_in, (size_t)LOADS_SUMS * l->nf * sizeof(double), hipMemcpyHostToDevice));
}

int fs_loads_reset(fs_ctx *ctx, fs_loads *l)
{
    FS_REQUIRE(ctx && l, "null argument");
    FS_HANDLE(l);
    FS_NO_CAPTURE(fs_loads, "reset");
    return counted_reset(ctx, l->d_state, dense_zero(ctx, l->d_sums, (size_t)LOADS_SUMS * l->nf * sizeof(double)));
}

int fs_loads_free(fs_ctx *ctx, fs_loads *l) { return object_free(ctx, l); }

// ---- time averages (fs_mean.h) ---------------------------------------------------------------------------------------------------------

// workgroups of 256 lanes x `w` columns and `rpw` rows over the owned rows: rows per workgroup from `g0` up to MEAN_ROWS (fs_launch.h
// diag_rows) - a non-sampling launch is a counter read per workgroup, so the grid stays in the thousands
static int mean_width(const fs_ctx *ctx) { return ctx->X % 2 == 0 ? 2 : 1; }      // columns per lane: W of k_mean_accumulate / k_mean_finalize
static dim3 mean_grid(const fs_ctx *ctx, int w, int g0, int *rpw)
{
    const int nx = (ctx->X + 256 * w - 1) / (256 * w), ny = ctx->nyl;
    const int r = diag_rows(ctx, nx, ny, g0, MEAN_ROWS);
    *rpw = r;
    return dim3(nx, (ny + r - 1) / r);
}

// diagnostic: the rows per workgroup the next fs_flow_stats / fs_mean_accumulate / fs_mean_finalize launches of this context take
int fs_diag_rows(fs_ctx *ctx, int *flow_stats_rows, int *mean_accumulate_rows, int *mean_finalize_rows)
{
    FS_REQUIRE(ctx && flow_stats_rows && mean_accumulate_rows && mean_finalize_rows, "null argument");
    *flow_stats_rows = stats_rows(ctx);
    mean_grid(ctx, mean_width(ctx), MEAN_G, mean_accumulate_rows);
    mean_grid(ctx, mean_width(ctx), 1, mean_finalize_rows);
    return FS_OK;
}

int fs_mean_create(fs_ctx *ctx, long long every, long long start, fs_mean **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_mean, "create");
    FS_HIP(hipSetDevice(ctx->device));
    auto m = std::make_unique<fs_mean>();
    m->every = every; m->start = start;
    m->plane = (size_t)ctx->nyl * ctx->P + MEAN_PAD;
    const size_t bytes = MEAN_PLANES * m->plane * sizeof(double);
    const hipError_t e = fill_buffers(ctx, {{m->d_state, MEAN_STATE * sizeof(long long)}, {m->d_sums, bytes}});
    if (e != hipSuccess) return hip_fail(e, "fs_mean_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(m));
    return FS_OK;
}

int fs_mean_accumulate(fs_ctx *ctx, fs_mean *m, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `m` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx);
    int rpw;
    const dim3 grid = mean_grid(ctx, w, MEAN_G, &rpw);
    const long long every = m->every, start = m->start;
    long long *state = m->d_state;
    double *sums = m->d_sums;
    const size_t plane = m->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "mean_accumulate", [=] {
            const bool found = pick<1, 2>(w, [&](auto W) {
                klaunch(k_mean_accumulate<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, limit, start, every, (const long long *)state, (const T *)v->d,
                        (const T *)p->d, sums, plane);
            });
            klaunch(k_mean_tick, dim3(1), dim3(64), ctx->stream, start, every, state);
            return found;
        });
    });
}

int fs_mean_finalize(fs_ctx *ctx, fs_mean *m, fs_field *v_out, fs_field *p_out)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_FIELD(v_out, 2); FS_FIELD(p_out, 1);
    FS_NO_CAPTURE(fs_mean, "finalize");
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    long long st[MEAN_STATE];
    if (int rc = read_counters(ctx, m->d_state, st)) return rc;
    if (st[1] < 1) { set_error("mean finalize: no sample accumulated yet"); return FS_ERR_STATE; }
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx);
    int rpw;
    const dim3 grid = mean_grid(ctx, w, 1, &rpw);
    const long long *state = m->d_state;
    const double *sums = m->d_sums;
    const size_t plane = m->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "mean_finalize", [=] {
            return pick<1, 2>(w, [&](auto W) {
                klaunch(k_mean_finalize<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, state, sums, plane, (T *)v_out->d, (T *)p_out->d, v_out->hot);
            });
        });
    });
}

int fs_mean_read(fs_ctx *ctx, fs_mean *m, double *sums_out, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_NO_CAPTURE(fs_mean, "read");
    return counted_read(ctx, m->d_state, launches, samples, sums_out != nullptr,
                        planes_copy(ctx, MEAN_PLANES, sizeof(double), m->d_sums, m->plane, sums_out, hipMemcpyDeviceToHost));
}

int fs_mean_write(fs_ctx *ctx, fs_mean *m, const double *sums_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && m && sums_in, "null argument");
    FS_HANDLE(m);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_mean, "write");
    return counted_set(ctx, m->d_state, launches, samples,
                       planes_copy(ctx, MEAN_PLANES, sizeof(double), m->d_sums, m->plane, sums_in, hipMemcpyHostToDevice));
}

int fs_mean_reset(fs_ctx *ctx, fs_mean *m)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_NO_CAPTURE(fs_mean, "reset");
    return counted_reset(ctx, m->d_state, dense_zero(ctx, m->d_sums, MEAN_PLANES * m->plane * sizeof(double)));
}

int fs_mean_free(fs_ctx *ctx, fs_mean *m) { return object_free(ctx, m); }

// ---- harmonic flow modes (fs_modes.h) ----------------------------------------------------------------------------------------------------

// as mean_grid: rows per workgroup from `g0` up to `rmax` (fs_launch.h diag_rows)
static dim3 modes_grid(const fs_ctx *ctx, int w, int g0, int rmax, int *rpw)
{
    const int nx = (ctx->X + 256 * w - 1) / (256 * w), ny = ctx->nyl;
    const int r = diag_rows(ctx, nx, ny, g0, rmax);
    *rpw = r;
    return dim3(nx, (ny + r - 1) / r);
}

int fs_modes_rows(fs_ctx *ctx, int nfreq, int *accumulate_rows, int *combine_rows)
{
    FS_REQUIRE(ctx && accumulate_rows && combine_rows, "null argument");
    FS_REQUIRE(nfreq >= 1 && nfreq <= MODES_MAX_FREQ, "nfreq must be 1 .. FS_MODES_MAX_FREQ");
    modes_grid(ctx, mean_width(ctx), modes_group(nfreq), modes_rows(nfreq), accumulate_rows);
    modes_grid(ctx, mean_width(ctx), 1, MEAN_ROWS, combine_rows);
    return FS_OK;
}

// the scalars of a fresh or reset object: every phasor (1, 0), the Gram matrix zero
static void modes_fresh_scalars(int nfreq, double *sc)
{
    for (int k = 0; k < modes_scalars(nfreq); ++k) sc[k] = 0.0;
    for (int k = 0; k < nfreq; ++k) sc[2 * k] = 1.0;
}

int fs_modes_create(fs_ctx *ctx, int nfreq, const double *cos_sin, long long every, long long start, fs_modes **out)
{
    FS_REQUIRE(ctx && cos_sin && out, "null argument");
    FS_REQUIRE(nfreq >= 1 && nfreq <= MODES_MAX_FREQ, "nfreq must be 1 .. FS_MODES_MAX_FREQ");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_modes, "create");
    FS_HIP(hipSetDevice(ctx->device));
    auto m = std::make_unique<fs_modes>();
    m->nfreq = nfreq; m->every = every; m->start = start;
    for (int k = 0; k < nfreq; ++k) { m->cd[k] = cos_sin[2 * k]; m->sd[k] = cos_sin[2 * k + 1]; }
    m->plane = (size_t)ctx->nyl * ctx->P + MEAN_PAD;
    const size_t bytes = 3 * (size_t)modes_basis(nfreq) * m->plane * sizeof(double);
    double sc[modes_scalars(MODES_MAX_FREQ)];
    modes_fresh_scalars(nfreq, sc);
    const hipError_t e = fill_buffers(ctx, {{m->d_state, MODES_STATE * sizeof(long long)}, {m->d_scal, modes_scalars(nfreq) * sizeof(double), sc},
                                            {m->d_sums, bytes}});
    if (e != hipSuccess) return hip_fail(e, "fs_modes_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(m));
    return FS_OK;
}

int fs_modes_accumulate(fs_ctx *ctx, fs_modes *m, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `m` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx), nfreq = m->nfreq;
    int rpw;
    const dim3 grid = modes_grid(ctx, w, modes_group(nfreq), modes_rows(nfreq), &rpw);
    const long long every = m->every, start = m->start;
    long long *state = m->d_state;
    double *scal = m->d_scal, *sums = m->d_sums;
    const size_t plane = m->plane;
    ModesRot rot;
    for (int k = 0; k < MODES_MAX_FREQ; ++k) { rot.cd[k] = m->cd[k]; rot.sd[k] = m->sd[k]; }
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "modes_accumulate", [=] {
            const bool found = pick<1, 2>(w, [&](auto W) { return pick<1, 2, 3, 4>(nfreq, [&](auto NFREQ) {
                klaunch(k_modes_accumulate<T, W, NFREQ>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, limit, start, every, (const long long *)state,
                        (const double *)scal, (const T *)v->d, (const T *)p->d, sums, plane);
            }); });
            klaunch(k_modes_tick, dim3(1), dim3(64), ctx->stream, nfreq, rot, start, every, state, scal);
            return found;
        });
    });
}

int fs_modes_combine(fs_ctx *ctx, fs_modes *m, const double *weights, fs_field *v_out, fs_field *p_out)
{
    FS_REQUIRE(ctx && m && weights, "null argument");
    FS_HANDLE(m);
    FS_FIELD(v_out, 2); FS_FIELD(p_out, 1);
    FS_NO_CAPTURE(fs_modes, "combine");
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx), B = modes_basis(m->nfreq);
    int rpw;
    const dim3 grid = modes_grid(ctx, w, 1, MEAN_ROWS, &rpw);
    ModesWeights wgt;
    for (int k = 0; k < 3 * MODES_MAX_B; ++k) wgt.w[k] = k < 3 * B ? weights[k] : 0.0;
    const double *sums = m->d_sums;
    const size_t plane = m->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "modes_combine", [=] {
            return pick<1, 2>(w, [&](auto W) {
                klaunch(k_modes_combine<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, B, wgt, sums, plane, (T *)v_out->d, (T *)p_out->d, v_out->hot);
            });
        });
    });
}

int fs_modes_read(fs_ctx *ctx, fs_modes *m, double *sums_out, double *scalars_out, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_NO_CAPTURE(fs_modes, "read");
    return counted_read(ctx, m->d_state, launches, samples, sums_out || scalars_out, [=]() -> int {
        if (scalars_out) FS_HIP(hipMemcpyAsync(scalars_out, m->d_scal, modes_scalars(m->nfreq) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return sums_out ? copy_planes(ctx, 3 * modes_basis(m->nfreq), sizeof(double), m->d_sums, m->plane, sums_out, hipMemcpyDeviceToHost) : FS_OK;
    });
}

int fs_modes_write(fs_ctx *ctx, fs_modes *m, const double *sums_in, const double *scalars_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && m && sums_in && scalars_in, "null argument");
    FS_HANDLE(m);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_modes, "write");
    return counted_set(ctx, m->d_state, launches, samples, [=]() -> int {
        FS_HIP(hipMemcpyAsync(m->d_scal, scalars_in, modes_scalars(m->nfreq) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return copy_planes(ctx, 3 * modes_basis(m->nfreq), sizeof(double), m->d_sums, m->plane, const_cast<double *>(sums_in), hipMemcpyHostToDevice);
    });
}

int fs_modes_reset(fs_ctx *ctx, fs_modes *m)
{
    FS_REQUIRE(ctx && m, "null argument");
    FS_HANDLE(m);
    FS_NO_CAPTURE(fs_modes, "reset");
    double sc[modes_scalars(MODES_MAX_FREQ)];
    modes_fresh_scalars(m->nfreq, sc);
    return counted_reset(ctx, m->d_state, [=, &sc]() -> int {
        FS_HIP(hipMemsetAsync(m->d_sums, 0, 3 * (size_t)modes_basis(m->nfreq) * m->plane * sizeof(double), ctx->stream));
        FS_HIP(hipMemcpyAsync(m->d_scal, sc, modes_scalars(m->nfreq) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return FS_OK;
    }, true);      // (sc is this frame's memory)
}

int fs_modes_free(fs_ctx *ctx, fs_modes *m) { return object_free(ctx, m); }

// ---- snapshot POD (fs_pod.h) ---------------------------------------------------------------------------------------------------------------

static size_t pod_slot_bytes(const fs_ctx *ctx, const fs_pod *p) { return 3 * p->plane * ctx->esize; }

int fs_pod_create(fs_ctx *ctx, int M, long long every, long long start, fs_pod **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(M >= 2 && M <= POD_MAX, "M must be 2 .. FS_POD_MAX");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_pod, "create");
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) {
        set_error("snapshot POD needs a single-GPU context: on a slab the Gram matrix needs a rank-ordered reduction (not implemented)");
        return FS_ERR_UNSUPPORTED;
    }
    FS_HIP(hipSetDevice(ctx->device));
    auto p = std::make_unique<fs_pod>();
    p->M = M; p->every = every; p->start = start;
    p->plane = (size_t)ctx->nyl * ctx->P + MEAN_PAD;
    const size_t bytes = (size_t)M * pod_slot_bytes(ctx, p.get());
    const hipError_t e = fill_buffers(ctx, {{p->d_state, POD_STATE * sizeof(long long)}, {p->d_slots, bytes}});
    if (e != hipSuccess) return hip_fail(e, "fs_pod_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(p));
    return FS_OK;
}

int fs_pod_launch(fs_ctx *ctx, fs_pod *pod, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && pod, "null argument");
    FS_HANDLE(pod);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `pod` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx), M = pod->M;
    int rpw;
    const dim3 grid = mean_grid(ctx, w, MEAN_G, &rpw);
    const long long every = pod->every, start = pod->start;
    long long *state = pod->d_state;
    void *slots = pod->d_slots;
    const size_t plane = pod->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "pod_capture", [=] {
            const bool found = pick<1, 2>(w, [&](auto W) {
                klaunch(k_pod_capture<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, limit, start, every, M, (const long long *)state,
                        (const T *)v->d, (const T *)p->d, (T *)slots, plane);
            });
            klaunch(k_pod_tick, dim3(1), dim3(64), ctx->stream, start, every, state);
            return found;
        });
    });
}

int fs_pod_read(fs_ctx *ctx, fs_pod *pod, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && pod, "null argument");
    FS_HANDLE(pod);
    FS_NO_CAPTURE(fs_pod, "read");
    long long st[POD_STATE];
    if (int rc = read_counters(ctx, pod->d_state, st)) return rc;
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    return FS_OK;
}

int fs_pod_gram(fs_ctx *ctx, fs_pod *pod, double *out, int max_n, int *n_out, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && pod && n_out, "null argument");
    FS_HANDLE(pod);
    FS_NO_CAPTURE(fs_pod, "gram");
    long long st[POD_STATE];
    if (int rc = read_counters(ctx, pod->d_state, st)) return rc;
    const int n = (int)std::min<long long>(st[1], pod->M);
    if (out) FS_REQUIRE(max_n >= n, "out holds fewer rows than there are resident samples");
    *n_out = n;
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    if (!out || n == 0) return FS_OK;
    // the geometry of csrc/fs_pod.h: nt tiles of POD_T slots, the diagonal tiles and the pairs ta < tb over blockIdx.z, 256 columns and rpw rows
    const int nt = (n + POD_T - 1) / POD_T, noff = nt * (nt - 1) / 2;
    const int nx = (ctx->X + 255) / 256, ny = ctx->nyl;
    const int rpw = diag_rows(ctx, nx, ny, POD_GRAM_G, POD_GRAM_ROWS);
    const int nby = (ny + rpw - 1) / rpw;
    const size_t nblocks = (size_t)nx * nby;
    const size_t need = (size_t)(nt + noff) * POD_TT * nblocks + (size_t)n * n;
    if (need > pod->gram_cap) {
        pod->gram_cap = 0;
        FS_HIP(pod->d_gram.alloc(need * sizeof(double)));      // (frees the smaller one first; the stream is idle: read_counters)
        pod->gram_cap = need;
    }
    double *partial = pod->d_gram, *total = pod->d_gram + (size_t)(nt + noff) * POD_TT * nblocks;
    const int X = ctx->X, P = ctx->P, jb = ctx->halo, je = ctx->halo + ctx->nyl;
    const void *slots = pod->d_slots;
    const size_t plane = pod->plane;
    const int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "pod_gram", [=] {
            klaunch(k_pod_gram<T, true>, dim3(nx, nby, nt), dim3(256), ctx->stream, X, P, jb, je, rpw, n, nt, 0, (const T *)slots, plane, partial);
            if (noff)
                klaunch(k_pod_gram<T, false>, dim3(nx, nby, noff), dim3(256), ctx->stream, X, P, jb, je, rpw, n, nt, nt, (const T *)slots, plane, partial);
            klaunch(k_pod_gram_final, dim3((nt + noff) * POD_TT), dim3(256), ctx->stream, (const double *)partial, (int)nblocks, n, nt, total);
        });
    });
    if (rc) return rc;
    FS_HIP(hipMemcpyAsync(out, total, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_pod_combine(fs_ctx *ctx, fs_pod *pod, const double *weights, fs_field *v_out, fs_field *p_out)
{
    FS_REQUIRE(ctx && pod && weights, "null argument");
    FS_HANDLE(pod);
    FS_FIELD(v_out, 2); FS_FIELD(p_out, 1);
    FS_NO_CAPTURE(fs_pod, "combine");
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    const int jb = ctx->halo, je = ctx->halo + ctx->nyl, w = mean_width(ctx), M = pod->M;
    int rpw;
    const dim3 grid = mean_grid(ctx, w, 1, &rpw);
    PodWeights wgt;
    for (int k = 0; k < POD_MAX; ++k) wgt.w[k] = k < M ? weights[k] : 0.0;
    const void *slots = pod->d_slots;
    const size_t plane = pod->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "pod_combine", [=] {
            return pick<1, 2>(w, [&](auto W) {
                klaunch(k_pod_combine<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), jb, je, rpw, M, wgt, (const T *)slots, plane, (T *)v_out->d, (T *)p_out->d, v_out->hot);
            });
        });
    });
}

int fs_pod_get(fs_ctx *ctx, fs_pod *pod, void *slots_out)
{
    FS_REQUIRE(ctx && pod && slots_out, "null argument");
    FS_HANDLE(pod);
    FS_NO_CAPTURE(fs_pod, "get");
    FS_HIP(hipSetDevice(ctx->device));
    if (int rc = copy_planes(ctx, 3 * pod->M, ctx->esize, pod->d_slots, pod->plane, slots_out, hipMemcpyDeviceToHost)) return rc;
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_pod_set(fs_ctx *ctx, fs_pod *pod, const void *slots_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && pod && slots_in, "null argument");
    FS_HANDLE(pod);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_pod, "set");
    return counted_set(ctx, pod->d_state, launches, samples,
                       planes_copy(ctx, 3 * pod->M, ctx->esize, pod->d_slots, pod->plane, slots_in, hipMemcpyHostToDevice));
}

int fs_pod_reset(fs_ctx *ctx, fs_pod *pod)
{
    FS_REQUIRE(ctx && pod, "null argument");
    FS_HANDLE(pod);
    FS_NO_CAPTURE(fs_pod, "reset");
    return counted_reset(ctx, pod->d_state, dense_zero(ctx, pod->d_slots, (size_t)pod->M * pod_slot_bytes(ctx, pod)));
}

int fs_pod_free(fs_ctx *ctx, fs_pod *pod) { return object_free(ctx, pod); }

// ---- vortex identification (fs_vortex.h) ----------------------------------------------------------------------------------------------------
#define FS_VORTEX_SINGLE_GPU() \
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) { \
        set_error("vortex identification needs a single-GPU context: on a slab the components would have to be united across ranks (not implemented)"); \
        return FS_ERR_UNSUPPORTED; \
    }

// the three launches that turn a flag plane into labels (fs_vortex.h b); counts: the roots per block of the compression, or nullptr
static int vortex_label_launches(fs_ctx *ctx, VxWhen when, const uint8_t *flags, int *labels, int *counts)
{
    const int X = ctx->X, Y = ctx->Y, n = X * Y;
    const int ntx = (X + VX_TX - 1) / VX_TX, nty = (Y + VX_TY - 1) / VX_TY;
    const long long pairs = (long long)(ntx - 1) * Y + (long long)(nty - 1) * X;
    int rc = launch(ctx, "vortex_local", [=] { klaunch(k_vortex_local, dim3(ntx, nty), dim3(256), ctx->stream, X, Y, when, flags, labels); });
    if (rc) return rc;
    rc = launch(ctx, "vortex_seam", [=] {
        klaunch(k_vortex_seam, dim3((unsigned)std::max<long long>(1, (pairs + 255) / 256)), dim3(256), ctx->stream, X, Y, when, flags, labels);
    });
    if (rc) return rc;
    return launch(ctx, "vortex_compress", [=] {
        klaunch(k_vortex_compress, dim3((n + VX_BLOCK - 1) / VX_BLOCK), dim3(256), ctx->stream, n, when, labels, counts);
    });
}

static dim3 vortex_flags_grid(const fs_ctx *ctx, int *rpw)
{
    const int nx = (ctx->X + 255) / 256;
    *rpw = diag_rows(ctx, nx, ctx->Y, VX_G, VX_ROWS);
    return dim3(nx, (ctx->Y + *rpw - 1) / *rpw);
}

int fs_vortex_create(fs_ctx *ctx, int criterion, double threshold, double scale, long long every, long long start, int min_area, int max_vortices,
                     int max_components, int capacity, fs_vortex **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(criterion >= 0 && criterion <= 2, "criterion must be 0 (q), 1 (swirl) or 2 (vorticity)");
    FS_REQUIRE(std::isfinite(threshold), "threshold must be finite");
    FS_REQUIRE(std::isfinite(scale) && scale > 0.0, "scale must be finite and positive");
    FS_EVERY_START(every, start);
    FS_REQUIRE(min_area >= 1, "min_area must be >= 1");
    FS_REQUIRE(max_vortices >= 1 && max_vortices <= VX_MAX_VORTICES, "max_vortices must be 1 .. FS_VORTEX_MAX_VORTICES");
    FS_REQUIRE(max_components >= 1 && max_components <= (1 << 24), "max_components must be 1 .. 2^24");
    FS_REQUIRE(capacity >= 1, "capacity must be >= 1");
    FS_NO_CAPTURE(fs_vortex, "create");
    FS_VORTEX_SINGLE_GPU()
    FS_HIP(hipSetDevice(ctx->device));
    auto x = std::make_unique<fs_vortex>();
    x->criterion = criterion; x->threshold = threshold; x->scale = scale; x->every = every; x->start = start;
    x->min_area = min_area; x->maxv = max_vortices; x->maxc = max_components; x->cap = capacity;
    x->cells = ctx->X * ctx->Y;
    x->nblocks = (x->cells + VX_BLOCK - 1) / VX_BLOCK;
    x->words = VX_HEAD + VX_REC * max_vortices;
    const size_t n = (size_t)x->cells, table = (size_t)VX_NACC * max_components * sizeof(long long);
    // (the labels start at -1; the counts need no initial value and get zero)
    const hipError_t e = fill_buffers(ctx, {{x->d_state, VX_STATE * sizeof(long long)}, {x->d_tmp, VX_TMP * sizeof(long long)}, {x->d_flags, n},
                                            {x->d_labels, n * sizeof(int), nullptr, 0xff}, {x->d_ids, n * sizeof(int)},
                                            {x->d_counts, (size_t)x->nblocks * sizeof(int)}, {x->d_table, table},
                                            {x->d_ring, (size_t)capacity * x->words * sizeof(long long)}});
    if (e != hipSuccess) return hip_fail(e, "fs_vortex_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(x));
    return FS_OK;
}

int fs_vortex_launch(fs_ctx *ctx, fs_vortex *vx, double limit, double dx, const fs_field *v)
{
    FS_REQUIRE(ctx && vx, "null argument");
    FS_HANDLE(vx);
    FS_FIELD(v, 2);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `vx` and the field: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int criterion = vx->criterion, min_area = vx->min_area, maxv = vx->maxv, maxc = vx->maxc, cap = vx->cap, cells = vx->cells, nblocks = vx->nblocks, words = vx->words;
    const double threshold = vx->threshold, scale = vx->scale;
    const long long every = vx->every, start = vx->start;
    uint8_t *flags = vx->d_flags;
    int *labels = vx->d_labels, *ids = vx->d_ids, *counts = vx->d_counts;
    long long *table = vx->d_table, *tmp = vx->d_tmp, *ring = vx->d_ring, *state = vx->d_state;
    const VxWhen when{state, start, every, cap};
    int rpw;
    const dim3 fgrid = vortex_flags_grid(ctx, &rpw);
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        int rc = launch(ctx, "vortex_flags", [=] {
            klaunch(k_vortex_flags<T, false>, fgrid, dim3(256), ctx->stream, ctx->grid(), ctx->Y, rpw, when, criterion, threshold, dx, limit,
                    (const T *)v->d, flags, (double *)nullptr, table, maxc, tmp);
        });
        if (rc) return rc;
        rc = vortex_label_launches(ctx, when, flags, labels, counts);
        if (rc) return rc;
        rc = launch(ctx, "vortex_scan", [=] { klaunch(k_vortex_scan, dim3(1), dim3(256), ctx->stream, nblocks, when, counts, tmp); });
        if (rc) return rc;
        rc = launch(ctx, "vortex_ids", [=] {
            klaunch(k_vortex_ids, dim3(nblocks), dim3(256), ctx->stream, cells, when, maxc, (const int *)labels, (const int *)counts, ids,
                    table);
        });
        if (rc) return rc;
        rc = launch(ctx, "vortex_reduce", [=] {
            klaunch(k_vortex_reduce<T>, dim3((cells + 255) / 256), dim3(256), ctx->stream, ctx->grid(), cells, when, dx, limit, scale, maxc,
                    (const T *)v->d, (const uint8_t *)flags, (const int *)labels, (const int *)ids, table, tmp);
        });
        if (rc) return rc;
        rc = launch(ctx, "vortex_records", [=] {
            klaunch(k_vortex_records, dim3(1), dim3(1024), ctx->stream, when, maxc, min_area, maxv, words, (const uint8_t *)flags,
                    (const long long *)table, (const long long *)tmp, ring);
        });
        if (rc) return rc;
        return launch(ctx, "vortex_tick", [=] { klaunch(k_vortex_tick, dim3(1), dim3(64), ctx->stream, start, every, cap, state); });
    });
}

int fs_vortex_read(fs_ctx *ctx, fs_vortex *vx, long long *out, int max_samples, int *n_out, long long *launches, long long *lost)
{
    FS_REQUIRE(ctx && vx && n_out, "null argument");
    FS_HANDLE(vx);
    FS_NO_CAPTURE(fs_vortex, "read");
    long long st[VX_STATE];
    if (int rc = read_counters(ctx, vx->d_state, st)) return rc;
    const int n = (int)st[1];
    FS_REQUIRE(n == 0 || (out && max_samples >= n), "out holds fewer samples than the ring");
    if (n) FS_HIP(hipMemcpyAsync(out, vx->d_ring, (size_t)n * vx->words * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipMemsetAsync(vx->d_state + 1, 0, 2 * sizeof(long long), ctx->stream));      // the ring is empty again, nothing lost since
    FS_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    if (launches) *launches = st[0];
    if (lost) *lost = st[2];
    return FS_OK;
}

int fs_vortex_get_labels(fs_ctx *ctx, fs_vortex *vx, unsigned char *flags, int *labels)
{
    FS_REQUIRE(ctx && vx, "null argument");
    FS_HANDLE(vx);
    FS_NO_CAPTURE(fs_vortex, "get_labels");
    FS_HIP(hipSetDevice(ctx->device));
    if (flags) FS_HIP(hipMemcpyAsync(flags, vx->d_flags, (size_t)vx->cells, hipMemcpyDeviceToHost, ctx->stream));
    if (labels) FS_HIP(hipMemcpyAsync(labels, vx->d_labels, (size_t)vx->cells * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_vortex_set(fs_ctx *ctx, fs_vortex *vx, long long launches)
{
    FS_REQUIRE(ctx && vx, "null argument");
    FS_HANDLE(vx);
    FS_REQUIRE(launches >= 0, "launches must be >= 0");
    FS_NO_CAPTURE(fs_vortex, "set");
    FS_HIP(hipSetDevice(ctx->device));
    const long long st[VX_STATE] = {launches, 0, 0, 0};
    FS_HIP(hipMemcpyAsync(vx->d_state, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));      // (the source is this frame's memory)
    return FS_OK;
}

int fs_vortex_label(fs_ctx *ctx, const unsigned char *flags, int *labels)
{
    FS_REQUIRE(ctx && flags && labels, "null argument");
    FS_NO_CAPTURE(fs_vortex, "label");
    FS_VORTEX_SINGLE_GPU()
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->X * ctx->Y;
    uint8_t *d_flags = nullptr;
    int *d_labels = nullptr;
    hipError_t e = hipMalloc(&d_flags, n);
    if (e == hipSuccess) e = hipMalloc(&d_labels, n * sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, ctx->stream);
    int rc = FS_OK;
    if (e == hipSuccess) {
        const VxWhen always{nullptr, 0, 1, 0};
        rc = vortex_label_launches(ctx, always, d_flags, d_labels, nullptr);
    }
    if (e == hipSuccess && rc == FS_OK) e = hipMemcpyAsync(labels, d_labels, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (d_flags) hipFree(d_flags);
    if (d_labels) hipFree(d_labels);
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? FS_OK : hip_fail(e, "fs_vortex_label", __FILE__, __LINE__);
}

int fs_vortex_criterion(fs_ctx *ctx, int which, double limit, double dx, const fs_field *v, double *out)
{
    FS_REQUIRE(ctx && out, "null argument");
    FS_REQUIRE(which >= 0 && which <= 2, "criterion must be 0 (q), 1 (swirl) or 2 (vorticity)");
    FS_FIELD(v, 2);
    FS_NO_CAPTURE(fs_vortex, "criterion");
    FS_VORTEX_SINGLE_GPU()
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->X * ctx->Y;
    double *d_crit = nullptr;
    FS_HIP(hipMalloc(&d_crit, n * sizeof(double)));
    const VxWhen always{nullptr, 0, 1, 0};
    int rpw;
    const dim3 fgrid = vortex_flags_grid(ctx, &rpw);
    const int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "vortex_criterion", [=] {
            klaunch(k_vortex_flags<T, true>, fgrid, dim3(256), ctx->stream, ctx->grid(), ctx->Y, rpw, always, which, 0.0, dx, limit, (const T *)v->d,
                    (uint8_t *)nullptr, d_crit, (long long *)nullptr, 0, (long long *)nullptr);
        });
    });
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(out, d_crit, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    hipFree(d_crit);
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? FS_OK : hip_fail(e, "fs_vortex_criterion", __FILE__, __LINE__);
}

int fs_vortex_free(fs_ctx *ctx, fs_vortex *vx) { return object_free(ctx, vx); }

// ---- field distributions (fs_dist.h) ---------------------------------------------------------------------------------------------------------
#define FS_DIST_SINGLE_GPU() \
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) { \
        set_error("field distributions need a single-GPU context: on a slab the tables would have to be added across ranks (not implemented)"); \
        return FS_ERR_UNSUPPORTED; \
    }
#define FS_DIST_BOX(box) FS_BOX(box, ctx->X, ctx->Y, "distribution box must satisfy 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y")

// the walk of a pass over `box`: the workgroups of the whole grid's tiling (256 columns, rows from diag_rows) that meet the box
static DistWalk dist_walk_of(const fs_ctx *ctx, const int *box, int need, double dx, double limit, dim3 *grid)
{
    const int rpw = diag_rows(ctx, (ctx->X + 255) / 256, ctx->Y, DIST_G, DIST_ROWS);
    const int bx0 = box[0] / 256, bx1 = (box[2] + 255) / 256, by0 = box[1] / rpw, by1 = (box[3] + rpw - 1) / rpw;
    *grid = dim3(bx1 - bx0, by1 - by0);
    return DistWalk{ctx->Y, rpw, bx0, by0, box[0], box[1], box[2], box[3], need, dx, limit};
}

int fs_dist_create(fs_ctx *ctx, int nchan, const fs_dist_spec *specs, long long every, long long start, fs_dist **out)
{
    FS_REQUIRE(ctx && specs && out, "null argument");
    FS_REQUIRE(nchan >= 1 && nchan <= DIST_MAX_CHANNELS, "nchan must be 1 .. FS_DIST_MAX_CHANNELS");
    FS_EVERY_START(every, start);
    auto d = std::make_unique<fs_dist>();
    d->nchan = nchan; d->every = every; d->start = start;
    for (int c = 0; c < nchan; ++c) {
        const fs_dist_spec &s = specs[c];
        FS_REQUIRE(s.quantity >= 0 && s.quantity < DIST_NQ && s.quantity_b < DIST_NQ, "quantity must be 0 (u) .. 6 (swirl)");
        FS_REQUIRE(s.bins >= 1 && s.bins <= DIST_MAX_BINS, "bins must be 1 .. FS_DIST_MAX_BINS");
        FS_REQUIRE(std::isfinite(s.lo) && std::isfinite(s.hi) && s.lo < s.hi, "range must be finite with lo < hi");
        d->inv[c] = (double)s.bins / (s.hi - s.lo);
        FS_REQUIRE(std::isfinite(d->inv[c]) && d->inv[c] > 0.0, "range too narrow or too wide: bins / (hi - lo) must be finite and positive");
        size_t words = (size_t)s.bins;
        if (s.quantity_b >= 0) {
            FS_REQUIRE(s.bins_b >= 1 && (long long)s.bins * s.bins_b <= DIST_MAX_BINS, "a joint table holds at most FS_DIST_MAX_BINS bins");
            FS_REQUIRE(std::isfinite(s.lo_b) && std::isfinite(s.hi_b) && s.lo_b < s.hi_b, "range must be finite with lo < hi");
            d->inv_b[c] = (double)s.bins_b / (s.hi_b - s.lo_b);
            FS_REQUIRE(std::isfinite(d->inv_b[c]) && d->inv_b[c] > 0.0, "range too narrow or too wide: bins / (hi - lo) must be finite and positive");
            words *= (size_t)s.bins_b;
        }
        FS_DIST_BOX(s.box);
        d->spec[c] = s;
        d->offset[c + 1] = d->offset[c] + words + DIST_TAILS;
    }
    FS_NO_CAPTURE(fs_dist, "create");
    FS_DIST_SINGLE_GPU()
    FS_HIP(hipSetDevice(ctx->device));
    const size_t bytes = d->offset[nchan] * sizeof(long long);
    const hipError_t e = fill_buffers(ctx, {{d->d_state, DIST_STATE * sizeof(long long)}, {d->d_tables, bytes}});
    if (e != hipSuccess) return hip_fail(e, "fs_dist_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(d));
    return FS_OK;
}

int fs_dist_launch(fs_ctx *ctx, fs_dist *d, double limit, double dx, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && d, "null argument");
    FS_HANDLE(d);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `d` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const long long every = d->every, start = d->start;
    long long *state = d->d_state;
    const DistWhen when{state, start, every};
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        for (int c = 0; c < d->nchan; ++c) {
            const fs_dist_spec &s = d->spec[c];
            const bool joint = s.quantity_b >= 0;
            const DistChan ch{s.quantity, joint ? s.quantity_b : -1, s.bins, joint ? s.bins_b : 1, s.lo, s.hi, d->inv[c], s.lo_b, s.hi_b, d->inv_b[c]};
            dim3 grid;
            const DistWalk walk = dist_walk_of(ctx, s.box, dist_need(ch.qa) | dist_need(ch.qb), dx, limit, &grid);
            long long *counts = d->d_tables + d->offset[c];
            const int rc = launch(ctx, "dist_accumulate", [=] {
                if (joint) klaunch(k_dist_accumulate<T, true>, grid, dim3(256), ctx->stream, ctx->grid(), walk, when, ch, (const T *)v->d, (const T *)p->d, counts);
                else klaunch(k_dist_accumulate<T, false>, grid, dim3(256), ctx->stream, ctx->grid(), walk, when, ch, (const T *)v->d, (const T *)p->d, counts);
            });
            if (rc) return rc;
        }
        return launch(ctx, "dist_tick", [=] { klaunch(k_dist_tick, dim3(1), dim3(64), ctx->stream, start, every, state); });
    });
}

int fs_dist_read(fs_ctx *ctx, fs_dist *d, int chan, long long *counts, long long *tails, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && d, "null argument");
    FS_HANDLE(d);
    FS_REQUIRE(chan >= 0 && chan < d->nchan, "channel outside 0 .. nchan - 1");
    FS_NO_CAPTURE(fs_dist, "read");
    const size_t bins = d->offset[chan + 1] - d->offset[chan] - DIST_TAILS;
    const long long *table = d->d_tables + d->offset[chan];
    return counted_read(ctx, d->d_state, launches, samples, counts || tails, [=]() -> int {
        if (counts) FS_HIP(hipMemcpyAsync(counts, table, bins * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (tails) FS_HIP(hipMemcpyAsync(tails, table + bins, DIST_TAILS * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        return FS_OK;
    });
}

int fs_dist_get(fs_ctx *ctx, fs_dist *d, long long *words_out)
{
    FS_REQUIRE(ctx && d && words_out, "null argument");
    FS_HANDLE(d);
    FS_NO_CAPTURE(fs_dist, "get");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(words_out, d->d_tables, d->offset[d->nchan] * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_dist_set(fs_ctx *ctx, fs_dist *d, const long long *words_in, long long launches, long long samples)
{
    FS_REQUIRE(ctx && d && words_in, "null argument");
    FS_HANDLE(d);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_dist, "set");
    return counted_set(ctx, d->d_state, launches, samples,
                       dense_copy(ctx, d->d_tables, words_in, d->offset[d->nchan] * sizeof(long long), hipMemcpyHostToDevice));
}

int fs_dist_reset(fs_ctx *ctx, fs_dist *d)
{
    FS_REQUIRE(ctx && d, "null argument");
    FS_HANDLE(d);
    FS_NO_CAPTURE(fs_dist, "reset");
    return counted_reset(ctx, d->d_state, dense_zero(ctx, d->d_tables, d->offset[d->nchan] * sizeof(long long)));
}

int fs_dist_free(fs_ctx *ctx, fs_dist *d) { return object_free(ctx, d); }

int fs_dist_select(fs_ctx *ctx, int quantity, const int *box, double limit, double dx, const fs_field *v, const fs_field *p,
                   const long long *ranks, int nranks, double *values_out, long long *n_out, long long *nan_out)
{
    FS_REQUIRE(ctx && box && n_out && nan_out, "null argument");
    FS_REQUIRE(quantity >= 0 && quantity < DIST_NQ, "quantity must be 0 (u) .. 6 (swirl)");
    FS_REQUIRE(nranks >= 0 && nranks <= DIST_MAX_RANKS && (nranks == 0 || (ranks && values_out)), "nranks must be 0 .. FS_DIST_MAX_RANKS");
    for (int r = 0; r < nranks; ++r) FS_REQUIRE(ranks[r] >= 0 && (r == 0 || ranks[r - 1] <= ranks[r]), "ranks must be >= 0 and ascending");
    FS_DIST_BOX(box);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    FS_NO_CAPTURE(fs_dist, "select");
    FS_DIST_SINGLE_GPU()
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    // the temporary objects of the call: the plane of the box's values, the digit tables of every prefix behind two counters
    const size_t cells = (size_t)(box[2] - box[0]) * (box[3] - box[1]);
    const size_t twords = 2 + (size_t)DIST_MAX_RANKS * DIST_DIGITS;
    DevBuf<double> plane;
    DevBuf<long long> tables;
    if (nranks) FS_HIP(plane.alloc(cells * sizeof(double)));
    FS_HIP(tables.alloc(twords * sizeof(long long)));
    double *d_plane = plane;
    long long *d_tot = tables, *d_tab = tables + 2;
    dim3 grid;
    const DistWalk walk = dist_walk_of(ctx, box, dist_need(quantity), dx, limit, &grid);
    FS_HIP(hipMemsetAsync(d_tot, 0, 2 * sizeof(long long), ctx->stream));
    int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "dist_values", [=] {
            klaunch(k_dist_values<T>, grid, dim3(256), ctx->stream, ctx->grid(), walk, quantity, (const T *)v->d, (const T *)p->d, d_plane, d_tot);
        });
    });
    long long tot[2] = {0, 0};
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream);
    hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "fs_dist_select", __FILE__, __LINE__);
    *n_out = tot[0];
    *nan_out = tot[1];
    if (nranks == 0) return FS_OK;
    FS_REQUIRE(tot[0] > 0, "no selected cell holds a value that is not NaN: there is no order statistic");
    FS_REQUIRE(ranks[nranks - 1] < tot[0], "rank must be below n, the number of selected cells whose value is not NaN");
    // one launch per digit: a table per DISTINCT prefix (ranks that still agree share theirs), downloaded, and every rank's digit picked
    unsigned long long prefix[DIST_MAX_RANKS];
    long long rest[DIST_MAX_RANKS];
    std::vector<long long> host((size_t)DIST_MAX_RANKS * DIST_DIGITS);
    for (int r = 0; r < nranks; ++r) { prefix[r] = 0; rest[r] = ranks[r]; }
    for (int pass = 0; pass < DIST_PASSES; ++pass) {
        DistPrefixes pre;
        int slot[DIST_MAX_RANKS], np = 0;
        for (int r = 0; r < nranks; ++r) {      // ascending ranks: equal prefixes are neighbours
            if (r > 0 && prefix[r] == prefix[r - 1]) { slot[r] = slot[r - 1]; continue; }
            pre.p[np] = prefix[r];
            slot[r] = np++;
        }
        for (int k = np; k < DIST_MAX_RANKS; ++k) pre.p[k] = 0;
        const size_t bytes = (size_t)np * DIST_DIGITS * sizeof(long long);
        FS_HIP(hipMemsetAsync(d_tab, 0, bytes, ctx->stream));
        const dim3 dgrid((unsigned)((cells + DIST_VALUES_PER_WG - 1) / DIST_VALUES_PER_WG), np);
        rc = launch(ctx, "dist_digits", [=] { klaunch(k_dist_digits, dgrid, dim3(256), ctx->stream, (const double *)d_plane, cells, pass, pre, d_tab); });
        e = rc ? hipSuccess : hipMemcpyAsync(host.data(), d_tab, bytes, hipMemcpyDeviceToHost, ctx->stream);
        es = hipStreamSynchronize(ctx->stream);
        if (rc) return rc;
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return hip_fail(e, "fs_dist_select", __FILE__, __LINE__);
        for (int r = 0; r < nranks; ++r) {
            long long within = 0;
            const int digit = dist_pick(host.data() + (size_t)slot[r] * DIST_DIGITS, 1 << dist_width(pass), rest[r], &within);
            if (digit < 0) { set_error("fs_dist_select: the digit counts do not hold the rank (internal)"); return FS_ERR_STATE; }
            prefix[r] |= (unsigned long long)digit << dist_shift(pass);
            rest[r] = within;
        }
    }
    for (int r = 0; r < nranks; ++r) values_out[r] = dist_unkey(prefix[r]);
    return FS_OK;
}

// ---- energy spectra (fs_spec.h) and cross-spectra (fs_xspec.h): one plan each (fs_host.h SpecPlan) and an accumulator of their own ------------
#define FS_SPEC_BOX(box)                                                                                             \
    FS_BOX(box, ctx->X, ctx->Y, "spectrum box must satisfy 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y");                \
    FS_REQUIRE(spec_log2((box)[2] - (box)[0]) > 0 && spec_log2((box)[3] - (box)[1]) > 0,                             \
               "the sides of a spectrum box must be powers of two in FS_SPEC_MIN_N .. FS_SPEC_MAX_N")

static dim3 spec_chunks(size_t cells) { return dim3((unsigned)((cells + SPEC_CHUNK - 1) / SPEC_CHUNK)); }

extern "C++" {
// What both creates do behind the argument checks of their own: the checks they share, the plan's members, its buffers and `acc`, the kind's
// accumulator.  `riders`: the kind as the slab refusal names it; `who`: the entry point, for a HIP error.
template <typename T>
static int spec_plan_create(fs_ctx *ctx, T &s, const char *riders, const char *who, const int *box, const double *wx, const double *wy, const double *twx,
                            const double *twy, double c1x, double c1y, int detrend, long long every, long long start, Fill acc)
{
    FS_REQUIRE(std::isfinite(c1x) && std::isfinite(c1y), "the detrend pair must be finite");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(T, "create");
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) {
        set_error(std::string(riders) + " need a single-GPU context: on a slab the transform along y crosses the ranks (not implemented)");
        return FS_ERR_UNSUPPORTED;
    }
    FS_HIP(hipSetDevice(ctx->device));
    for (int k = 0; k < 4; ++k) s.box[k] = box[k];
    const int nx = s.nx = box[2] - box[0], ny = s.ny = box[3] - box[1];
    s.detrend = detrend ? 1 : 0; s.c1x = c1x; s.c1y = c1y; s.every = every; s.start = start;
    const size_t plane = s.cells() * sizeof(double2);
    const hipError_t e = fill_buffers(ctx, {{s.d_state, SPEC_STATE * sizeof(long long)}, {s.d_wx, nx * sizeof(double), wx}, {s.d_wy, ny * sizeof(double), wy},
                                            {s.d_twx, nx * sizeof(double), twx}, {s.d_twy, ny * sizeof(double), twy}, {s.d_a, plane}, {s.d_b, plane}, acc});
    return e == hipSuccess ? FS_OK : hip_fail(e, who, __FILE__, __LINE__);
}

// The launches both samplings share behind their first: `load` - the caller's kernel: the box's rows into d_a, transformed along x -, the transpose
// into d_b, the transform along y back into d_a.  Every closure holds values copied out of the plan here: captured into graphs and tapes, it reads
// nothing through the object when it is replayed.
template <typename Load>
static int spec_forward(fs_ctx *ctx, const SpecPlan &s, const SpecWhen when, Load load)
{
    const int nx = s.nx, ny = s.ny, logny = spec_log2(ny);
    const size_t cells = s.cells();
    const dim3 chunks = spec_chunks(cells);
    const double *twy = s.d_twy;
    double2 *A = s.d_a, *B = s.d_b;
    int rc = load();
    if (rc) return rc;
    rc = launch(ctx, "spec_transpose", [=] {
        klaunch(k_spec_transpose, dim3((nx + SPEC_TILE - 1) / SPEC_TILE, (ny + SPEC_TILE - 1) / SPEC_TILE), dim3(256), ctx->stream, when, ny, nx,
                (const double2 *)A, B);
    });
    if (rc) return rc;
    return launch(ctx, "spec_rows", [=] { klaunch(k_spec_rows, chunks, dim3(256), ctx->stream, when, ny, logny, cells, (const double2 *)B, twy, A); });
}

// Z' of the last sampling launch
template <typename T>
static int spec_plane(fs_ctx *ctx, T *s, double *plane)
{
    FS_REQUIRE(ctx && s && plane, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(T, "plane");
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(plane, s->d_b, s->cells() * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}
}  // extern "C++"

// the last launch of a sampling (the fluxes' too): the counters advance
static int spec_finish(fs_ctx *ctx, const SpecWhen when)
{
    long long *state = const_cast<long long *>(when.state);
    const long long start = when.start, every = when.every;
    return launch(ctx, "spec_tick", [=] { klaunch(k_spec_tick, dim3(1), dim3(64), ctx->stream, start, every, state); });
}

int fs_spec_create(fs_ctx *ctx, const int *box, const double *wx, const double *wy, const double *twx, const double *twy, double c1x, double c1y,
                   int detrend, long long every, long long start, fs_spec **out)
{
    FS_REQUIRE(ctx && box && wx && wy && twx && twy && out, "null argument");
    FS_SPEC_BOX(box);
    auto s = std::make_unique<fs_spec>();
    const size_t power = (size_t)(box[2] - box[0]) * (box[3] - box[1]) * sizeof(double);
    if (int rc = spec_plan_create(ctx, *s, "energy spectra", "fs_spec_create", box, wx, wy, twx, twy, c1x, c1y, detrend, every, start, {s->d_power, power}))
        return rc;
    *out = adopt(ctx, std::move(s));
    return FS_OK;
}

int fs_spec_launch(fs_ctx *ctx, fs_spec *s, double limit, const fs_field *v)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_FIELD(v, 2);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `s` and the field: no allocation, copy or synchronisation here (the closures are captured / taped)
    const int x0 = s->box[0], y0 = s->box[1], nx = s->nx, ny = s->ny, lognx = spec_log2(nx), logny = spec_log2(ny), detrend = s->detrend;
    const double c1x = s->c1x, c1y = s->c1y;
    const SpecWhen when{s->d_state, s->start, s->every};
    const size_t cells = s->cells();
    const dim3 chunks = spec_chunks(cells);
    const double *wx = s->d_wx, *wy = s->d_wy, *twx = s->d_twx;
    double2 *A = s->d_a, *B = s->d_b;
    double *P = s->d_power;
    int rc = spec_forward(ctx, *s, when, [&] {
        return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
            return launch(ctx, "spec_load_rows", [=] {
                klaunch(k_spec_load_rows<T>, chunks, dim3(256), ctx->stream, ctx->grid(), when, x0, y0, nx, ny, lognx, limit, (const T *)v->d, wx, wy, twx, A);
            });
        });
    });
    if (rc) return rc;
    rc = launch(ctx, "spec_power", [=] {
        klaunch(k_spec_power, dim3((unsigned)((cells + 255) / 256)), dim3(256), ctx->stream, when, nx, ny, logny, detrend, c1x, c1y, (const double2 *)A, B, P);
    });
    if (rc) return rc;
    return spec_finish(ctx, when);
}

int fs_spec_read(fs_ctx *ctx, fs_spec *s, double *power, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_spec, "read");
    return counted_read(ctx, s->d_state, launches, samples, power != nullptr,
                        dense_copy(ctx, power, s->d_power, s->cells() * sizeof(double), hipMemcpyDeviceToHost));
}

int fs_spec_plane(fs_ctx *ctx, fs_spec *s, double *plane) { return spec_plane(ctx, s, plane); }

int fs_spec_get(fs_ctx *ctx, fs_spec *s, double *power, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s && power && launches && samples, "null argument");
    return fs_spec_read(ctx, s, power, launches, samples);
}

int fs_spec_set(fs_ctx *ctx, fs_spec *s, const double *power, long long launches, long long samples)
{
    FS_REQUIRE(ctx && s && power, "null argument");
    FS_HANDLE(s);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_spec, "set");
    return counted_set(ctx, s->d_state, launches, samples, dense_copy(ctx, s->d_power, power, s->cells() * sizeof(double), hipMemcpyHostToDevice));
}

int fs_spec_reset(fs_ctx *ctx, fs_spec *s)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_spec, "reset");
    return counted_reset(ctx, s->d_state, dense_zero(ctx, s->d_power, s->cells() * sizeof(double)));
}

int fs_spec_free(fs_ctx *ctx, fs_spec *s) { return object_free(ctx, s); }

int fs_xspec_create(fs_ctx *ctx, const int *box, int qa, int qb, double dx, const double *wx, const double *wy, const double *twx, const double *twy,
                    double c1x, double c1y, int detrend, long long every, long long start, fs_xspec **out)
{
    FS_REQUIRE(ctx && box && wx && wy && twx && twy && out, "null argument");
    FS_SPEC_BOX(box);
    FS_REQUIRE(0 <= qa && qa < XSPEC_NQ && -1 <= qb && qb < XSPEC_NQ, "the quantities of a cross-spectrum must satisfy 0 <= qa <= 6 and -1 <= qb <= 6");
    FS_REQUIRE(std::isfinite(dx) && dx > 0.0, "dx must be finite and > 0");
    auto s = std::make_unique<fs_xspec>();
    s->qa = qa; s->qb = qb; s->planes = qb >= 0 ? XSPEC_PLANES : 1; s->dx = dx;
    const size_t acc = (size_t)s->planes * (box[2] - box[0]) * (box[3] - box[1]) * sizeof(double);
    if (int rc = spec_plan_create(ctx, *s, "cross-spectra", "fs_xspec_create", box, wx, wy, twx, twy, c1x, c1y, detrend, every, start, {s->d_acc, acc}))
        return rc;
    *out = adopt(ctx, std::move(s));
    return FS_OK;
}

int fs_xspec_launch(fs_ctx *ctx, fs_xspec *s, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `s` and the fields: no allocation, copy or synchronisation here (the closures are captured / taped)
    const int x0 = s->box[0], y0 = s->box[1], nx = s->nx, ny = s->ny, lognx = spec_log2(nx), logny = spec_log2(ny), detrend = s->detrend;
    const int qa = s->qa, qb = s->qb, need = dist_need(qa) | dist_need(qb), pair = qb >= 0 ? 1 : 0;
    const double c1x = s->c1x, c1y = s->c1y, two_dx = 2.0 * s->dx;
    const SpecWhen when{s->d_state, s->start, s->every};
    const size_t cells = s->cells();
    const dim3 chunks = spec_chunks(cells);
    const double *wx = s->d_wx, *wy = s->d_wy, *twx = s->d_twx;
    double2 *A = s->d_a, *B = s->d_b;
    double *acc = s->d_acc;
    int rc = spec_forward(ctx, *s, when, [&] {
        return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
            return launch(ctx, "xspec_load_rows", [=] {
                klaunch(k_xspec_load_rows<T>, chunks, dim3(256), ctx->stream, ctx->grid(), when, x0, y0, nx, ny, lognx, qa, qb, need, limit, two_dx,
                        (const T *)v->d, (const T *)p->d, wx, wy, twx, A);
            });
        });
    });
    if (rc) return rc;
    rc = launch(ctx, "xspec_accumulate", [=] {
        klaunch(k_xspec_accumulate, dim3((unsigned)((cells + 255) / 256)), dim3(256), ctx->stream, when, nx, ny, logny, detrend, pair, c1x, c1y,
                (const double2 *)A, B, acc);
    });
    if (rc) return rc;
    return spec_finish(ctx, when);
}

static size_t xspec_bytes(const fs_xspec *s) { return (size_t)s->planes * s->cells() * sizeof(double); }

int fs_xspec_read(fs_ctx *ctx, fs_xspec *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_xspec, "read");
    return counted_read(ctx, s->d_state, launches, samples, sums != nullptr, dense_copy(ctx, sums, s->d_acc, xspec_bytes(s), hipMemcpyDeviceToHost));
}

int fs_xspec_plane(fs_ctx *ctx, fs_xspec *s, double *plane) { return spec_plane(ctx, s, plane); }

int fs_xspec_get(fs_ctx *ctx, fs_xspec *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s && sums && launches && samples, "null argument");
    return fs_xspec_read(ctx, s, sums, launches, samples);
}

int fs_xspec_set(fs_ctx *ctx, fs_xspec *s, const double *sums, long long launches, long long samples)
{
    FS_REQUIRE(ctx && s && sums, "null argument");
    FS_HANDLE(s);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_xspec, "set");
    return counted_set(ctx, s->d_state, launches, samples, dense_copy(ctx, s->d_acc, sums, xspec_bytes(s), hipMemcpyHostToDevice));
}

int fs_xspec_reset(fs_ctx *ctx, fs_xspec *s)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_xspec, "reset");
    return counted_reset(ctx, s->d_state, dense_zero(ctx, s->d_acc, xspec_bytes(s)));
}

int fs_xspec_free(fs_ctx *ctx, fs_xspec *s) { return object_free(ctx, s); }

// ---- scale-to-scale fluxes (fs_flux.h) -------------------------------------------------------------------------------------------------------
// the valid cells of half-width r inside the box, half-open (empty: x0 >= x1 or y0 >= y1)
static void flux_valid(const fs_ctx *ctx, const int *box, int r, int *out)
{
    out[0] = std::max(box[0], r + 1); out[1] = std::max(box[1], r + 1);
    out[2] = std::min(box[2], ctx->X - 1 - r); out[3] = std::min(box[3], ctx->Y - 1 - r);
}

int fs_flux_create(fs_ctx *ctx, const int *box, int nr, const int *half_widths, double dx, long long every, long long start, fs_flux **out)
{
    FS_REQUIRE(ctx && box && half_widths && out, "null argument");
    FS_BOX(box, ctx->X, ctx->Y, "flux box must satisfy 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y");
    FS_REQUIRE(1 <= nr && nr <= FLUX_MAX_WIDTHS, "the number of half-widths must be 1 .. FS_FLUX_MAX_WIDTHS");
    for (int k = 0; k < nr; ++k) {
        FS_REQUIRE(1 <= half_widths[k] && half_widths[k] <= FLUX_MAX_R, "a half-width must be 1 .. FS_FLUX_MAX_R");
        FS_REQUIRE(k == 0 || half_widths[k] > half_widths[k - 1], "the half-widths must be strictly increasing");
        int val[4];
        flux_valid(ctx, box, half_widths[k], val);
        FS_REQUIRE(val[0] < val[2] && val[1] < val[3], "a half-width has no valid cell inside the box (valid: r + 1 <= i <= X - 2 - r, r + 1 <= j <= Y - 2 - r)");
    }
    FS_REQUIRE(std::isfinite(dx) && dx > 0.0, "dx must be finite and > 0");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_flux, "create");
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) {
        set_error("scale fluxes need a single-GPU context: on a slab the filter along y crosses the ranks (not implemented)");
        return FS_ERR_UNSUPPORTED;
    }
    FS_HIP(hipSetDevice(ctx->device));
    auto s = std::make_unique<fs_flux>();
    for (int k = 0; k < 4; ++k) s->box[k] = box[k];
    s->nx = box[2] - box[0]; s->ny = box[3] - box[1]; s->nr = nr; s->dx = dx; s->every = every; s->start = start;
    for (int k = 0; k < nr; ++k) s->r[k] = half_widths[k];
    const int d = half_widths[nr - 1] + 1;
    s->dx0 = std::max(0, box[0] - d); s->dy0 = std::max(0, box[1] - d);
    s->DW = std::min(ctx->X, box[2] + d) - s->dx0; s->DH = std::min(ctx->Y, box[3] + d) - s->dy0;
    const size_t work = (size_t)FLUX_NQ * s->DW * s->DH * sizeof(double), acc = (size_t)nr * FLUX_SUMS * s->nx * s->ny * sizeof(double);
    const hipError_t e = fill_buffers(ctx, {{s->d_state, (SPEC_STATE + 1) * sizeof(long long)}, {s->d_base, work}, {s->d_rows, work}, {s->d_filt, work},
                                            {s->d_acc, acc}});
    if (e != hipSuccess) return hip_fail(e, "fs_flux_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(s));
    return FS_OK;
}

// passes 2 and 3 of half-width r: base -> R -> F
static int flux_filter(fs_ctx *ctx, const fs_flux *s, const SpecWhen when, int r)
{
    const int DW = s->DW, DH = s->DH, n = 2 * r + 1;
    const double inv = 1.0 / (double)(n * n);
    const double *base = s->d_base;
    double *R = s->d_rows, *F = s->d_filt;
    const int rx = (DW + FLUX_STRIP - 1) / FLUX_STRIP, cx = (DW + FLUX_COL_LANES - 1) / FLUX_COL_LANES;
    const dim3 rows(rx, flux_groups_y(rx, (DH + FLUX_ROW_WAVES - 1) / FLUX_ROW_WAVES), FLUX_NQ);
    const dim3 cols(cx, flux_groups_y(cx, (DH + FLUX_COL_V - 1) / FLUX_COL_V), FLUX_NQ);
    int rc = launch(ctx, "flux_rows", [=] { klaunch(k_flux_rows, rows, dim3(64 * FLUX_ROW_WAVES), ctx->stream, when, DW, DH, r, base, R); });
    if (rc) return rc;
    return launch(ctx, "flux_cols", [=] {
        klaunch(k_flux_cols, cols, dim3(FLUX_COL_LANES), ctx->stream, when, DW, DH, r, inv, (const double *)R, F);
    });
}

int fs_flux_launch(fs_ctx *ctx, fs_flux *s, double limit, const fs_field *v)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_FIELD(v, 2);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `s` and the field: no allocation, copy or synchronisation here (the closures are captured / taped)
    const FluxGeom f{s->dx0, s->dy0, s->DW, s->DH, s->box[0], s->box[1], s->nx, s->ny};
    const double two_dx = 2.0 * s->dx;
    const SpecWhen when{s->d_state, s->start, s->every};
    const size_t dcells = (size_t)s->DW * s->DH, cells = (size_t)s->nx * s->ny;
    const int X = ctx->X, Y = ctx->Y;
    double *base = s->d_base, *F = s->d_filt;
    int rc = by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "flux_base", [=] {
            klaunch(k_flux_base<T>, dim3(flux_groups(dcells)), dim3(256), ctx->stream, ctx->grid(), when, f, limit, two_dx, (const T *)v->d, base);
        });
    });
    if (rc) return rc;
    for (int k = 0; k < s->nr; ++k) {
        const int r = s->r[k];
        if ((rc = flux_filter(ctx, s, when, r))) return rc;
        double *acc = s->d_acc + (size_t)k * FLUX_SUMS * cells;
        rc = launch(ctx, "flux_accumulate", [=] {
            klaunch(k_flux_accumulate, dim3(flux_groups(cells)), dim3(256), ctx->stream, when, f, X, Y, r, two_dx, (const double *)F, acc);
        });
        if (rc) return rc;
    }
    return spec_finish(ctx, when);
}

static size_t flux_bytes(const fs_flux *s) { return (size_t)s->nr * FLUX_SUMS * s->nx * s->ny * sizeof(double); }

int fs_flux_read(fs_ctx *ctx, fs_flux *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_flux, "read");
    return counted_read(ctx, s->d_state, launches, samples, sums != nullptr, dense_copy(ctx, sums, s->d_acc, flux_bytes(s), hipMemcpyDeviceToHost));
}

int fs_flux_filtered(fs_ctx *ctx, fs_flux *s, int width, double *planes)
{
    FS_REQUIRE(ctx && s && planes, "null argument");
    FS_HANDLE(s);
    FS_REQUIRE(0 <= width && width < s->nr, "width must be an index into the object's half-widths");
    FS_NO_CAPTURE(fs_flux, "filtered");
    FS_HIP(hipSetDevice(ctx->device));
    const SpecWhen always{s->d_state + SPEC_STATE, 0, 1};      // (a word that stays 0: samples_at(0, 0, 1))
    if (int rc = flux_filter(ctx, s, always, s->r[width])) return rc;
    const size_t plane = (size_t)s->DW * s->DH, cells = (size_t)s->nx * s->ny;
    const double *F = s->d_filt + (size_t)(s->box[1] - s->dy0) * s->DW + (s->box[0] - s->dx0);
    for (int k = 0; k < FLUX_NQ; ++k)
        FS_HIP(hipMemcpy2DAsync(planes + k * cells, s->nx * sizeof(double), F + k * plane, s->DW * sizeof(double), s->nx * sizeof(double), s->ny,
                                hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_flux_get(fs_ctx *ctx, fs_flux *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s && sums && launches && samples, "null argument");
    return fs_flux_read(ctx, s, sums, launches, samples);
}

int fs_flux_set(fs_ctx *ctx, fs_flux *s, const double *sums, long long launches, long long samples)
{
    FS_REQUIRE(ctx && s && sums, "null argument");
    FS_HANDLE(s);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_flux, "set");
    return counted_set(ctx, s->d_state, launches, samples, dense_copy(ctx, s->d_acc, sums, flux_bytes(s), hipMemcpyHostToDevice));
}

int fs_flux_reset(fs_ctx *ctx, fs_flux *s)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_flux, "reset");
    return counted_reset(ctx, s->d_state, dense_zero(ctx, s->d_acc, flux_bytes(s)));
}

int fs_flux_free(fs_ctx *ctx, fs_flux *s) { return object_free(ctx, s); }

// ---- kinetic-energy budget (fs_budget.h) ---------------------------------------------------------------------------------------------------
// columns per lane: W of k_budget_accumulate (16-byte plane accesses need rows of an even number of doubles)
static int budget_width(const fs_budget *s) { return s->nx % 2 == 0 ? 2 : 1; }
static dim3 budget_grid(const fs_ctx *ctx, const fs_budget *s, int *rpw)
{
    const int w = budget_width(s), gx = (s->nx + 256 * w - 1) / (256 * w);
    const int r = diag_rows(ctx, gx, s->ny, BUDGET_ROWS0, BUDGET_ROWS);
    *rpw = r;
    return dim3(gx, (s->ny + r - 1) / r);
}
// the dense host planes [BUDGET_PLANES][ny][nx] <-> the staggered device planes; queued on the stream
static auto budget_copy(fs_ctx *ctx, const fs_budget *s, const double *host, hipMemcpyKind kind)
{
    return [=]() -> int {
        const size_t cells = (size_t)s->nx * s->ny;
        for (int k = 0; k < BUDGET_PLANES; ++k) {
            double *d = s->d_sums + k * s->plane, *h = const_cast<double *>(host) + k * cells;
            if (kind == hipMemcpyDeviceToHost) FS_HIP(hipMemcpyAsync(h, d, cells * sizeof(double), kind, ctx->stream));
            else FS_HIP(hipMemcpyAsync(d, h, cells * sizeof(double), kind, ctx->stream));
        }
        return FS_OK;
    };
}

int fs_budget_create(fs_ctx *ctx, int x0, int y0, int x1, int y1, double dx, long long every, long long start, fs_budget **out)
{
    FS_REQUIRE(ctx && out, "null argument");
    const int box[4] = {x0, y0, x1, y1};
    FS_BOX(box, ctx->X, ctx->Y, "budget box must satisfy 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y");
    FS_REQUIRE(std::isfinite(dx) && dx > 0.0, "dx must be finite and > 0");
    FS_EVERY_START(every, start);
    FS_NO_CAPTURE(fs_budget, "create");
    if (ctx->halo != 0 || ctx->nyl != ctx->Y) {
        set_error("the budget needs a single-GPU context: on a slab the gradient along y crosses the ranks (not implemented)");
        return FS_ERR_UNSUPPORTED;
    }
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    const int nx = x1 - x0, ny = y1 - y0;
    std::vector<uint8_t> mk((size_t)nx * ny);
    FS_HIP(hipMemcpy2DAsync(mk.data(), nx, ctx->d_mask + (size_t)y0 * ctx->Pm + x0, ctx->Pm, nx, ny, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    FS_REQUIRE(std::find(mk.begin(), mk.end(), (uint8_t)0) != mk.end(), "budget box holds no fluid cell (mask == 0)");
    auto s = std::make_unique<fs_budget>();
    for (int k = 0; k < 4; ++k) s->box[k] = box[k];
    s->nx = nx; s->ny = ny; s->dx = dx; s->every = every; s->start = start;
    s->plane = (size_t)nx * ny + BUDGET_PAD;
    const hipError_t e = fill_buffers(ctx, {{s->d_state, BUDGET_STATE * sizeof(long long)}, {s->d_sums, BUDGET_PLANES * s->plane * sizeof(double)}});
    if (e != hipSuccess) return hip_fail(e, "fs_budget_create", __FILE__, __LINE__);
    *out = adopt(ctx, std::move(s));
    return FS_OK;
}

int fs_budget_launch(fs_ctx *ctx, fs_budget *s, double limit, const fs_field *v, const fs_field *p)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_FIELD(v, 2); FS_FIELD(p, 1);
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    // everything the launches need is in `s` and the fields: no allocation, copy or synchronisation here (the closure is captured / taped)
    const int w = budget_width(s);
    int rpw;
    const dim3 grid = budget_grid(ctx, s, &rpw);
    const BudgetBox b{s->box[0], s->box[1], s->nx, s->ny};
    const double two_dx = 2.0 * s->dx;
    const long long every = s->every, start = s->start;
    long long *state = s->d_state;
    double *sums = s->d_sums;
    const size_t plane = s->plane;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        return launch(ctx, "budget_accumulate", [=] {
            const bool found = pick<1, 2>(w, [&](auto W) {
                klaunch(k_budget_accumulate<T, W>, grid, dim3(256), ctx->stream, ctx->grid(), b, rpw, limit, two_dx, start, every, (const long long *)state,
                        (const T *)v->d, (const T *)p->d, sums, plane);
            });
            klaunch(k_budget_tick, dim3(1), dim3(64), ctx->stream, start, every, state);
            return found;
        });
    });
}

int fs_budget_read(fs_ctx *ctx, fs_budget *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_budget, "read");
    return counted_read(ctx, s->d_state, launches, samples, sums != nullptr, budget_copy(ctx, s, sums, hipMemcpyDeviceToHost));
}

int fs_budget_get(fs_ctx *ctx, fs_budget *s, double *sums, long long *launches, long long *samples)
{
    FS_REQUIRE(ctx && s && sums && launches && samples, "null argument");
    return fs_budget_read(ctx, s, sums, launches, samples);
}

int fs_budget_set(fs_ctx *ctx, fs_budget *s, const double *sums, long long launches, long long samples)
{
    FS_REQUIRE(ctx && s && sums, "null argument");
    FS_HANDLE(s);
    FS_COUNTERS(launches, samples);
    FS_NO_CAPTURE(fs_budget, "set");
    return counted_set(ctx, s->d_state, launches, samples, budget_copy(ctx, s, sums, hipMemcpyHostToDevice));
}

int fs_budget_reset(fs_ctx *ctx, fs_budget *s)
{
    FS_REQUIRE(ctx && s, "null argument");
    FS_HANDLE(s);
    FS_NO_CAPTURE(fs_budget, "reset");
    return counted_reset(ctx, s->d_state, dense_zero(ctx, s->d_sums, BUDGET_PLANES * s->plane * sizeof(double)));
}

int fs_budget_free(fs_ctx *ctx, fs_budget *s) { return object_free(ctx, s); }

// ---- flow maps through the resident snapshots (fs_lcs.h) ----------------------------------------------------------------------------------

static FlowMapDev flowmap_dev(const fs_flowmap *f)
{
    const size_t n = (size_t)f->nx * f->ny;
    return FlowMapDev{f->nx, f->ny, f->box[0], f->box[1], f->r, f->d_pos, f->d_pos + n, f->d_status, f->d_pos + 2 * n};
}
static dim3 flowmap_grid(const fs_flowmap *f) { return dim3((unsigned)(((size_t)f->nx * f->ny + FM_WG - 1) / FM_WG)); }

static int flowmap_seed(fs_ctx *ctx, fs_flowmap *fm)
{
    const FlowMapDev fd = flowmap_dev(fm);
    const dim3 grid = flowmap_grid(fm);
    return launch(ctx, "flowmap_seed", [=] { klaunch(k_flowmap_seed, grid, dim3(FM_WG), ctx->stream, ctx->grid(), fd); });
}

int fs_flowmap_create(fs_ctx *ctx, const int *box, int refine, fs_flowmap **out)
{
    FS_REQUIRE(ctx && box && out, "null argument");
    FS_BOX(box, ctx->X, ctx->Y, "flow-map box must satisfy 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y");
    FS_REQUIRE(refine == 1 || refine == 2 || refine == 4 || refine == 8, "refine must be 1, 2, 4 or 8");
    const long long nx = (long long)refine * (box[2] - box[0]), ny = (long long)refine * (box[3] - box[1]);
    FS_REQUIRE(nx * ny <= (1LL << 30), "flow map of more than 2^30 nodes");
    FS_NO_CAPTURE(fs_flowmap, "create");
    if (ctx->comm || ctx->halo != 0 || ctx->y0 != 0 || ctx->nyl != ctx->Y) {
        set_error("flow maps need a single-GPU context: on a slab the particles would have to migrate between ranks (not implemented)");
        return FS_ERR_UNSUPPORTED;
    }
    if (!ctx->mask_set) { set_error("mask not uploaded"); return FS_ERR_STATE; }
    FS_HIP(hipSetDevice(ctx->device));
    auto f = std::make_unique<fs_flowmap>();
    f->r = refine; f->nx = (int)nx; f->ny = (int)ny;
    for (int k = 0; k < 4; ++k) f->box[k] = box[k];
    const size_t n = (size_t)(nx * ny);
    hipError_t e = f->d_pos.alloc(3 * n * sizeof(double));      // (no fill_buffers: the seeding launch below writes every node, and nothing waits)
    if (e == hipSuccess) e = f->d_status.alloc(n * sizeof(int));
    if (e != hipSuccess) return hip_fail(e, "fs_flowmap_create", __FILE__, __LINE__);
    if (int rc = flowmap_seed(ctx, f.get())) { hipStreamSynchronize(ctx->stream); return rc; }
    *out = adopt(ctx, std::move(f));
    return FS_OK;
}

int fs_flowmap_advance(fs_ctx *ctx, fs_flowmap *fm, const fs_pod *pod, int slot_from, int slot_to, double h, int substeps)
{
    FS_REQUIRE(ctx && fm && pod, "null argument");
    FS_HANDLE(fm);
    FS_HANDLE(pod);
    FS_REQUIRE(0 <= slot_from && slot_from < pod->M && 0 <= slot_to && slot_to < pod->M, "slot outside 0 .. M - 1");
    FS_REQUIRE(slot_from != slot_to, "slot_from and slot_to must differ");
    FS_REQUIRE(substeps >= 1 && substeps <= FM_MAX_SUBSTEPS, "substeps must be 1 .. FS_FLOWMAP_MAX_SUBSTEPS");
    FS_REQUIRE(std::isfinite(h) && h != 0.0, "h must be finite and not 0");
    FS_NO_CAPTURE(fs_flowmap, "advance");
    const FlowMapDev fd = flowmap_dev(fm);
    const dim3 grid = flowmap_grid(fm);
    const int Y = ctx->Y;
    const size_t plane = pod->plane;
    const void *slots = pod->d_slots;
    return by_dtype(ctx, [&](auto tag) -> int { using T = typename decltype(tag)::type;
        const T *from = (const T *)slots + (size_t)slot_from * 3 * plane, *to = (const T *)slots + (size_t)slot_to * 3 * plane;
        return launch(ctx, "flowmap_advance", [=] {
            klaunch(k_flowmap_advance<T>, grid, dim3(FM_WG), ctx->stream, ctx->grid(), Y, h, substeps, fd, from, to, plane);
        });
    });
}

int fs_flowmap_cauchy_green(fs_ctx *ctx, fs_flowmap *fm)
{
    FS_REQUIRE(ctx && fm, "null argument");
    FS_HANDLE(fm);
    FS_NO_CAPTURE(fs_flowmap, "cauchy_green");
    const FlowMapDev fd = flowmap_dev(fm);
    const dim3 grid = flowmap_grid(fm);
    return launch(ctx, "flowmap_cauchy_green", [=] { klaunch(k_flowmap_cauchy_green, grid, dim3(FM_WG), ctx->stream, fd); });
}

int fs_flowmap_get(fs_ctx *ctx, fs_flowmap *fm, double *x, double *y, int *status, double *lam)
{
    FS_REQUIRE(ctx && fm, "null argument");
    FS_HANDLE(fm);
    FS_NO_CAPTURE(fs_flowmap, "get");
    FS_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)fm->nx * fm->ny;
    double *const dst[3] = {x, y, lam};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) FS_HIP(hipMemcpyAsync(dst[k], fm->d_pos + k * n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (status) FS_HIP(hipMemcpyAsync(status, fm->d_status, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

int fs_flowmap_reset(fs_ctx *ctx, fs_flowmap *fm)
{
    FS_REQUIRE(ctx && fm, "null argument");
    FS_HANDLE(fm);
    FS_NO_CAPTURE(fs_flowmap, "reset");
    return flowmap_seed(ctx, fm);
}

int fs_flowmap_free(fs_ctx *ctx, fs_flowmap *fm)
{
    if (!fm) return FS_OK;
    FS_HANDLE(fm);
    FS_NO_CAPTURE(fs_flowmap, "free");      // (the one free that a capture refuses instead of deferring)
    return object_free(ctx, fm);
}

}  // extern "C"
