// fs_launch.h - host-side launch plumbing shared by the translation units behind the C-ABI (fs_core.hip: contexts, fields, scene upload,
// boundary kernels, graphs / tapes / profiling; fs_transport.hip: K2 - K6, K10 - K13; fs_pressure.hip: K7 - K8, the Poisson residual;
// fs_diag.hip: flow diagnostics, history, body loads, time averages, harmonic modes, snapshot POD, flow maps, vortices, distributions, spectra; fs_tracers.hip: tracer
// particles; fs_multigrid.hip: the multigrid updater):
// the launch wrapper (profiling events, tape recording), XCD-band launch geometry with compact tile lists, the typed kernel dispatch,
// argument checks.
//
// A launch site reads:   return launch(ctx, "name", [=] { return with_dm_all<T>(dm, [&](auto DM) { klaunch(k_foo<2, 4, DM, T>, og, ctx->stream, k, jb, je, ...); }); });
//   launch()           runs the callable (captures BY VALUE) under the profile name, records it on an open tape, turns "no variant" into an error;
//   pick / pick_bool / with_dm_* (fs_pick.h)   make a run-time value a template argument, for the values listed there and no others;
//   klaunch()          notes the kernel for fs_prof_kernels and launches it - with explicit grid and block (fs_host.h), from an OvGrid (a tile
//                      kernel: grid, threads, Grid, nbx, nby come from the object), or one cell per lane over a row range (klaunch_cells);
//   by_dtype()         runs a callable with T = float or double, by the context's dtype.
// How to add a kernel variant: add its value to the list of the pick<...> at the launch site (a new rows-per-tile: pick<2, 4, 8>(rt, ...)) or one
// more branch where the variant exists for some combinations only.  Nothing else names the instantiation.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fs_host.h"
#include "fs_pick.h"

namespace fs {

hipEvent_t prof_event(fs_ctx *c);      // fs_core.hip


// f(): true unless it returns the false of a pick (fs_pick.h) that found no kernel for its value
template <typename F>
inline bool launched(const F &f)
{
    if constexpr (std::is_void<decltype(f())>::value) { f(); return true; }
    else return f();
}
int no_variant(const char *name);      // fs_core.hip: sets the error text, returns FS_ERR_UNSUPPORTED

// Every kernel launch of the library goes through here.  The callable captures its arguments BY VALUE: while a tape is being
// recorded (fs_tape_begin) a copy is kept and re-issued by fs_tape_replay without going back through the caller.
template <typename F>
inline int launch(fs_ctx *c, const char *name, F &&f)
{
    if (c->tape_rec) {
        c->tape_rec->ops.emplace_back([f, name]() -> int {
            if (!launched(f)) return no_variant(name);
            hipError_t e = hipGetLastError();
            return e == hipSuccess ? FS_OK : hip_fail(e, "tape replay", __FILE__, __LINE__);
        });
        if (!c->tape_execute) return FS_OK;
    }
    const bool prof = c->prof_on && !c->capturing;
    ProfRec rec{};
    if (prof) {
        auto it = c->prof_ids.find(name);
        if (it == c->prof_ids.end()) {
            it = c->prof_ids.emplace(name, (int)c->prof_names.size()).first;
            c->prof_names.push_back(name);
            c->prof_launches.push_back(0);
            c->prof_ms.push_back(0.0);
            c->prof_kernels.emplace_back();
        }
        rec.name_id = it->second;
        rec.start = prof_event(c);
        rec.stop = prof_event(c);
        (void)hipEventRecord(rec.start, c->stream);
    }
    kernel_notes.n = 0;
    const bool found = launched(f);
    if (prof) {
        (void)hipEventRecord(rec.stop, c->stream);
        c->prof_recs.push_back(rec);
        auto &ks = c->prof_kernels[rec.name_id];
        for (int i = 0; i < kernel_notes.n; ++i)
            if (std::find(ks.begin(), ks.end(), kernel_notes.fn[i]) == ks.end()) ks.push_back(kernel_notes.fn[i]);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, name, __FILE__, __LINE__);
    return found ? FS_OK : no_variant(name);
}

// Grids below 2 M cells have few waves per SIMD: a launch takes as long as ONE wave's chain of loads, stages and stores, and
// tiles of half the height halve that chain (round 4, tools/r4_chain.py; env FS_SMALL_CELLS=0: the big grids' tile heights everywhere)
static inline bool small_tiles(const fs_ctx *c) { return (size_t)c->X * c->Y < c->small_cells; }

// Rows per workgroup of the diagnostics' kernels (k_flow_stats, k_mean_accumulate, k_mean_finalize, k_modes_accumulate, k_modes_combine: `nx` workgroups across, `ny` owned rows):
// doubled from `r0` while the grid keeps >= diag_wgs workgroups (2048: 8 per CU; env FS_DIAG_WGS), at most `rmax`
static inline int diag_rows(const fs_ctx *c, int nx, int ny, int r0, int rmax)
{
    int r = r0;
    while (r < rmax && (size_t)nx * ((ny + 2 * r - 1) / (2 * r)) >= c->diag_wgs) r *= 2;
    return r;
}

// a launch over every row of a single-GPU grid (what may clear a buffer's "hot" word [3], fs_device.h)
static inline int whole_grid(const fs_ctx *c, int jb, int je) { return c->halo == 0 && jb == 0 && je == c->rows ? 1 : 0; }

static inline dim3 cells_grid(const fs_ctx *c, int jb, int je) { return dim3((c->X + 255) / 256, je - jb, 1); }

// plain and boundary workgroups as two compact launches (fs_ctx::rbpair_split): always, or from `threshold` cells on
static inline bool split_launch(const fs_ctx *c, size_t cells, size_t threshold) { return c->rbpair_split == 2 || (c->rbpair_split == 1 && cells >= threshold); }

// one-cell-per-lane kernels over rows [jb, je): k_foo(Grid, Konst<T>, jb, ...) and k_foo(Grid, jb, ...)
template <typename K, typename... P, typename... A>
inline void klaunch_cells(void (*kern)(Grid, Konst<K>, int, P...), const fs_ctx *c, int jb, int je, const Konst<K> &k, A... args)
{
    klaunch(kern, cells_grid(c, jb, je), dim3(256), c->stream, c->grid(), k, jb, args...);
}
template <typename... P, typename... A>
inline void klaunch_cells(void (*kern)(Grid, int, P...), const fs_ctx *c, int jb, int je, A... args)
{
    klaunch(kern, cells_grid(c, jb, je), dim3(256), c->stream, c->grid(), jb, args...);
}
// ... as a launch of their own
template <typename Kern, typename... A>
inline int launch_cells(fs_ctx *c, const char *name, Kern kern, int jb, int je, A... args)
{
    return launch(c, name, [=] { klaunch_cells(kern, c, jb, je, args...); });
}

// overlapped-wave tile kernels: nbx blocks of `threads / 64` waves across, nby tile rows, XCD-band 1-D launch
struct OvGrid {
    int nbx, nby; dim3 grid; Grid g; int threads = 256;      // threads: 64 x waves per workgroup
    const fs_ctx::TileList *list = nullptr;                  // the launch list behind g.tiles (until the next mask), or null: a dense launch
    OvGrid with_threads(int n) const { OvGrid o = *this; o.threads = n; return o; }      // (kernels whose list entry is a tile of several component waves)
};
// tile kernels take their geometry from the OvGrid handed in: k_foo(Grid, Konst<T>, nbx, nby, ...) and k_foo(Grid, nbx, nby, ...)
template <typename K, typename... P, typename... A>
inline void klaunch(void (*kern)(Grid, Konst<K>, int, int, P...), const OvGrid &og, hipStream_t stream, const Konst<K> &k, A... args)
{
    klaunch(kern, og.grid, dim3(og.threads), stream, og.g, k, og.nbx, og.nby, args...);
}
template <typename... P, typename... A>
inline void klaunch(void (*kern)(Grid, int, int, P...), const OvGrid &og, hipStream_t stream, A... args)
{
    klaunch(kern, og.grid, dim3(og.threads), stream, og.g, og.nbx, og.nby, args...);
}
enum { XCD_RBSOR = 1, XCD_VORT = 2, XCD_ADVECT = 4, XCD_NONADV = 8, XCD_GRAD = 16, XCD_JACOBI = 32 };

// A tile kernel's launch, said in words at the call site: tiles(family, lanes) and what differs from a dense-or-skipping launch of 4-wave
// workgroups on 1-row tiles.  The *_within(reach) forms pick which tiles the launch list holds and which hints its entries carry (fs_tiles.h).
struct TileLaunch {
    int family, lanes;            // XCD_* bit of the kernel family; wave geometry (fs_tiles.h LANES_*)
    int rt = 1, zgroups = 1, wgw = 4;
    bool compact = true;
    int cls = TILES_ALL, reach = 0, parent_rt = 0;
    bool slab_classes = false;

    TileLaunch rows(int n) const { TileLaunch l = *this; l.rt = n; return l; }                          // rows per tile
    TileLaunch channel_groups(int n) const { TileLaunch l = *this; l.zgroups = n; return l; }           // passes over the same tile, adjacent in dispatch order
    TileLaunch waves(int n) const { TileLaunch l = *this; l.wgw = n; return l; }                        // waves per workgroup
    TileLaunch dense_if(bool dense) const { TileLaunch l = *this; l.compact = !dense; return l; }       // no list: every workgroup of the grid
    // every workgroup with work; bit w of an entry: wave w sees nothing but fluid within `reach` rows of its tile and its halo lanes ("plain")
    TileLaunch hints_within(int reach_) const { TileLaunch l = *this; l.cls = TILES_ALL; l.reach = reach_; return l; }
    // the two parts of a split launch: the plain tiles, the others
    TileLaunch plain_within(int reach_) const { TileLaunch l = *this; l.cls = TILES_PLAIN; l.reach = reach_; return l; }
    TileLaunch boundary_within(int reach_) const { TileLaunch l = *this; l.cls = TILES_BOUNDARY; l.reach = reach_; return l; }
    // the one-launch red-black pair: 8-row units, a plain parent tile as one entry
    TileLaunch mixed_within(int reach_) const { TileLaunch l = *this; l.cls = TILES_MIXED; l.reach = reach_; return l; }
    TileLaunch parent_rows(int n) const { TileLaunch l = *this; l.parent_rt = n; return l; }            // plain is decided per parent tile of n rows
    // plain / boundary / mixed lists for a row range of a slab too (fs_cip_step, the one-launch pair); without it a slab's ranges get TILES_ALL lists only
    TileLaunch classes_on_slabs(bool on) const { TileLaunch l = *this; l.slab_classes = on; return l; }
};
static inline TileLaunch tiles(int family, int lanes) { return TileLaunch{family, lanes}; }

// Round 6: the hinted single-launch kernels of the pressure families run as ONE-wave workgroups - a list entry is then one tile, and the entries whose tile
// takes the masked body stand first in every XCD's list (fs_tiles.h masked_first), the all-fluid tiles fill in behind them: the four-sweep Jacobi pass at bc2 res
// 1600 30.2 -> 23.9 us (configs[1] 2 057 -> 2 472 steps/s), the finishing pass 24.2 -> 21.2, the small grids' red-black pair 12.7 -> 12.0 (res 400) / 12.3 ->
// 11.6 (configs[0]: 59.6 -> 62.0 k steps/s), the graded literal sweep 73.6 -> 72.1 (three A/B rounds).  Vorticity confinement and K2' measured no gain
// (85.5 against 84.9; 155.4 against 154.8) and keep their 4-wave workgroups (column-by-column locality).
static inline TileLaunch one_wave_where_hinted(const fs_ctx *c, TileLaunch l)
{
    if (c->dtype == 0 && (l.family & (XCD_RBSOR | XCD_JACOBI)) && l.wgw == 4 && l.cls == TILES_ALL && l.reach > 0 && l.compact) l.wgw = 1;      // (f32: the f64 bodies were not measured)
    return l;
}
// from the launch to the list it takes its work from: the workgroup shape and the dense grid's extents over rows [jb, je)
static inline TileSpec list_spec(const fs_ctx *c, const TileLaunch &l, int jb, int je)
{
    TileSpec s;
    s.lanes = l.lanes; s.rt = l.rt; s.wgw = l.wgw; s.cls = l.cls; s.reach = l.reach; s.parent_rt = l.parent_rt; s.jb = jb; s.je = je;
    const int waves = geo_waves(c->X, l.lanes), tile_rows = (je - jb + l.rt - 1) / l.rt;
    s.stacked = (c->stack_mask & l.family) != 0 && l.wgw > 1;    // the waves of a workgroup: tile rows of one wave column
    s.nbx = s.stacked ? waves : (waves + l.wgw - 1) / l.wgw;
    s.nby = s.stacked ? (tile_rows + l.wgw - 1) / l.wgw : tile_rows;
    // Groups of 8 tile rows per XCD measured best for every family (2 / 4 / 16 / 32 / per-family sizes: rounds 2 - 4)
    constexpr int xg = 8;
    s.group = s.stacked ? std::max(1, xg / l.wgw) : xg;     // the same number of field rows per XCD group
    return s;
}
const fs_ctx::TileList *tile_list(fs_ctx *c, TileSpec spec);      // fs_core.hip

// XCD-band launch geometry of a tile kernel family (fs_march.h band_coords).  When the launch covers the whole single-GPU grid - or a row range
// of a slab - the workgroups without anything to do are left out (compact list, Grid::tiles).
static inline OvGrid ov_grid(fs_ctx *c, int jb, int je, const TileLaunch &asked)
{
    const TileLaunch l = one_wave_where_hinted(c, asked);
    const TileSpec s = list_spec(c, l, jb, je);
    OvGrid o;
    o.g = c->grid();
    o.threads = 64 * l.wgw;
    o.nbx = s.nbx;
    o.nby = s.nby;
    const bool listed = l.compact && (c->tile_list_mask & l.family) && ((jb == 0 && je == c->rows) || (c->halo != 0 && (l.cls == TILES_ALL || l.slab_classes)));
    o.list = listed ? tile_list(c, s) : nullptr;
    // dense: (8 * block columns, rows per XCD group * channel groups, groups per XCD), decoded without a division (fs_march.h band_coords)
    const int groups = (o.nby + s.group - 1) / s.group;
    if (o.list) { o.grid = dim3(8 * o.list->per_xcd * l.zgroups, 1, 1); o.g.tiles = o.list->d; }
    else o.grid = dim3(8 * o.nbx, s.group * l.zgroups, (groups + 7) / 8);
    o.nby |= (s.group - 1) << 24;
    if (l.zgroups > 1 && o.list) o.nby |= FS_CG_INNER;
    if (s.stacked) o.nby |= FS_STACKED;
    return o;
}

int check_rows(const fs_ctx *c, int jb, int je);                               // fs_core.hip
int check_field(const fs_ctx *c, const fs_field *f, int C, const char *what);
int ensure_stage(fs_ctx *c, size_t bytes);

#define FS_FIELD(f, C)                                             \
    do {                                                           \
        int rc__ = fs::check_field(ctx, f, C, #f);                 \
        if (rc__) return rc__;                                     \
    } while (0)
#define FS_ROWS()                                                  \
    do {                                                           \
        int rc__ = fs::check_rows(ctx, row_begin, row_end);        \
        if (rc__) return rc__;                                     \
        if (!ctx->mask_set) { fs::set_error("mask not uploaded"); return FS_ERR_STATE; } \
        if (row_begin == row_end) return FS_OK;                    \
    } while (0)

// dispatch on ctx dtype: f(Type<float>{}) or f(Type<double>{}), whose int it returns (`using T = typename decltype(tag)::type;`)
template <typename T> struct Type { using type = T; };
template <typename F>
inline int by_dtype(const fs_ctx *c, F &&f) { return c->dtype == 0 ? f(Type<float>{}) : f(Type<double>{}); }

}  // namespace fs
