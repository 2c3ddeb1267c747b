// fs_host.h - host-side objects behind the opaque C-ABI handles (include/fs_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <cmath>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fs_hip.h"
#include "fs_device.h"
#include "fs_kernels.h"
#include "fs_march.h"      // (with fs_tiles.h: the launch lists' host side)
#include "fs_rbpair.h"
#include "fs_jquad.h"
#include "fs_k34n.h"
#include "fs_history.h"
#include "fs_objects.h"

namespace fs {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define FS_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return fs::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define FS_REQUIRE(cond, msg)                  \
    do {                                       \
        if (!(cond)) {                         \
            fs::set_error(msg);                \
            return FS_ERR_ARG;                 \
        }                                      \
    } while (0)

// Owner of one hipMalloc'd buffer: move-only, freed with whatever holds it.  It converts to the raw pointer, so kernel arguments, pointer
// arithmetic and the copies read as before; an untyped buffer also casts to the element type of the field, `(T *)d_slots`, like a void *.
template <typename T>
class DevBuf {
    T *p = nullptr;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept { reset(o.release()); return *this; }
    ~DevBuf() { reset(); }
    void reset(T *q = nullptr) { if (p) hipFree(p); p = q; }
    T *release() { T *q = p; p = nullptr; return q; }      // hands the buffer out: the caller frees it
    hipError_t alloc(size_t bytes)                         // (what it held is freed first)
    {
        reset();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    T *get() const { return p; }
    operator T *() const { return p; }
    template <typename U, typename V = T, typename = std::enable_if_t<std::is_void<V>::value>>
    explicit operator U *() const { return (U *)p; }
};

struct BcOpsDev {
    int nsimple = 0, npair = 0, ncomp = 0, nops = 0;
    int4 *simple = nullptr, *pair = nullptr;
    int *comp_begin = nullptr, *comp_rlo = nullptr, *comp_rhi = nullptr;
    int *kind = nullptr, *tgt = nullptr, *s1 = nullptr, *s2 = nullptr, *row = nullptr, *srow = nullptr;
    int lanes() const { return nsimple + npair + ncomp; }
    BcOps view() const { return BcOps{nsimple, simple, npair, pair, ncomp, comp_begin, comp_rlo, comp_rhi, kind, tgt, s1, s2, row, srow}; }
};

// Which __global__ functions a profiled launch name stands for (fs_prof_kernels: bench.py quotes the demangled symbols instead of string
// literals).  Every kernel launch of the library is written klaunch(kernel, grid, block, stream, args...): the host stub's address
// is noted per thread, and fs::launch() (fs_launch.h) files the notes of the callable it just ran under the launch's profile name.
struct KernelNotes { const void *fn[4]; int n; };
extern thread_local KernelNotes kernel_notes;      // fs_core.hip
template <typename... P, typename... A>
inline void klaunch(void (*kern)(P...), dim3 grid, dim3 block, hipStream_t stream, A... args)
{
    if (kernel_notes.n < 4) kernel_notes.fn[kernel_notes.n++] = (const void *)kern;
    kern<<<grid, block, 0, stream>>>(args...);
}

struct ProfRec {
    int name_id;
    hipEvent_t start, stop;
};

struct Comm;  // fs_comm.hip

// recorded launch sequence (fs_tape_*): closures that re-issue a kernel launch / an exchange step with the arguments of the recording
struct Tape {
    std::vector<std::function<int()>> ops;
};

}  // namespace fs

struct fs_ctx {
    int device = 0;
    int X = 0, Y = 0, dtype = 0, y0 = 0, nyl = 0, halo = 0;
    int rows = 0, P = 0, Pm = 0;
    size_t esize = 4;
    hipStream_t stream = nullptr;
    uint8_t *d_mask = nullptr;
    uint8_t *d_bcmap = nullptr;    // [rows][Pm] recipe byte of the pressure boundary condition per cell (fs_march.h k_jacobi_lazy)
    uint8_t *d_lazyflags = nullptr;   // [nwx][rows] tile needs the lazy evaluation
    std::vector<uint8_t> h_bcmap;  // host copy between build_bc_ops and the upload
    bool lazy_ok = false;                    // mask admits the lazy pressure BC
    bool rb_pair_ok = false;                 // mask admits the two-iteration red-black pass (fs_rbpair.h; decided in build_bc_ops)
    bool jq_ok = false;                      // mask admits the four-sweep Jacobi pass (fs_jquad.h)
    int rbpair_split = 1;                    // plain and boundary workgroups of that pass (and of the four-sweep Jacobi pass) as two compact
                                             // launches: env FS_RBPAIR_SPLIT = 0 never, 1 on grids of 8 M cells or more, 2 always
    size_t small_cells = (size_t)1 << 21;    // 2-row tiles on grids below this many cells (env FS_SMALL_CELLS; 0: never): res 800 +4.7 %, res 1024 (2 M cells) +0.3 %
    size_t diag_wgs = 2048;                  // fs_flow_stats and the averages take more rows per workgroup while the grid keeps this many workgroups
                                             // (8 per CU; env FS_DIAG_WGS, values below 1 are 1: the most rows on every grid; fs_launch.h diag_rows)
    uint32_t *d_pairlist = nullptr; int n_pairlist[2] = {0, 0};   // wave-tile rows of the two-sweep kernel's general path, without / with its
                                                                   // vertical-recipe tile path (fs_march.h k_pair_list): [2][nwx * rows] + 2 counters
    int nwx = 0;                   // wave columns of 62 quads across a row
    void *d_bc_const = nullptr, *d_bc_dye = nullptr;
    bool mask_set = false, bc_incomplete = false;
    int bc_radius_vel = 0, bc_radius_prs = 0;   // rows of pre-kernel data a rewritten boundary cell depends on
    fs::BcOpsDev ops_vel, ops_prs, ops_dye;
    void *d_stage = nullptr;
    size_t stage_bytes = 0;
    double *d_acc = nullptr;  // 2 doubles (residual)
    int barrier_wgs = 0;          // workgroups of 256 threads of those kernels this device keeps resident at once, with headroom (fs_create): the bound of their grids
    unsigned *d_sync = nullptr;   // k_velocity_bc_limit / k_dye_bc_limit: arrive / depart counters of the grid barrier of their rare path [0, 1] (zero between launches)
    double *d_partial = nullptr;   // per-block partial (sum, count) pairs of the residual reduction
    size_t partial_cap = 0;        // pairs
    double *d_stats = nullptr;     // fs_flow_stats: per-workgroup partial vectors of FS_FLOW_NSTAT doubles, then the combined vector
    size_t stats_cap = 0;          // vectors
    // graphs
    bool capturing = false;
    std::vector<hipGraphExec_t> graphs;
    // tapes
    fs::Tape *tape_rec = nullptr;      // open recording
    bool tape_execute = true;          // ... that also executes what it records (false: record only)
    std::vector<fs::Tape *> tapes;
    // profiling
    bool prof_on = false;
    std::vector<std::string> prof_names;
    std::map<std::string, int> prof_ids;
    std::vector<fs::ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    std::vector<int> prof_launches;
    std::vector<double> prof_ms;
    int tile_list_misses = 0;     // launches that wanted a launch list and could not build one (capture / tape recording / cap): fs_tile_list_stats
    std::vector<std::vector<const void *>> prof_kernels;      // per name: the host stubs of the __global__ functions launched under it (fs_prof_kernels)
    hipEvent_t span_ev[2] = {nullptr, nullptr};      // fs_span_begin / fs_span_end
    // comm
    fs::Comm *comm = nullptr;
    std::set<fs_field *> fields;  // live fields, released with the context
    fs::Objects objects;          // every other live object (fs::ObjKind), released with the context; the releases a capture defers (fs_objects.h)
    // tuning knobs (env FS_MARCH=0: one-cell-per-lane kernels only)
    bool use_march = true;
    bool use_pairs = true;     // lanes of 2 cells: even widths (every `res`); use_march: the quad kernels, X % 4 == 0
    int fuse_k2 = 2;           // env FS_FUSE_K2: 0 - fs_cip_step as its two calls, K2 then the fused K3 + K4 pass; 1 - K2 in registers on every tile, two launches
                               // (all-fluid tiles, the others); 2 - the same in ONE launch over both kinds of tile.  Same observable results.
    bool limit_gate = true;    // env FS_LIMIT_GATE=0: limit_field always reads the whole field (A/B; the results are the same)
    int stack_mask = 0;       // kernel families (XCD_* bits) launched with stacked workgroups (fs_create)

    // compact launches (fs_device.h Grid::tiles): the scene's activity per (wave column, local row) on the host, and the lists built from it per launch
    // geometry at first use (fs_tiles.h: the maps, the list specification, the builder; fs_core.hip tile_list: upload and cache)
    int tile_list_mask = 1 | 2 | 4 | 8 | 32;              // env FS_TILE_LIST: kernel families (XCD_* bits) launched compactly.  Measured at bc5 res 4096:
                                             // K3+K4 363 -> 346 us, red-black pair 215 -> 192, vorticity confinement (2-cell lanes) 97 -> 95, K2 (2-cell lanes) 105 -> 102, the plain Jacobi sweeps 87.2 -> 85.8 (reading v) / 75.5 -> 74.1 (source pair)
    fs::ActivityMaps act;         // empty: no lists for this scene (odd width, FS_TILE_LIST=0, more rows than an entry holds)
    struct TileList { uint32_t *d = nullptr; int per_xcd = 0; int count = 0; };      // count: listed workgroups (without the padding)
    using TileKey = decltype(fs::TileSpec().key());
    std::map<TileKey, TileList> tile_lists;

    fs::Grid grid() const
    {
        fs::Grid g;
        g.tiles = nullptr;
        g.X = X; g.P = P; g.Pm = Pm; g.rows = rows;
        int jlo = halo - y0, jhi = halo - y0 + (Y - 1);
        g.jlo = jlo < 0 ? 0 : jlo;
        g.jhi = jhi > rows - 1 ? rows - 1 : jhi;
        g.ybase = y0 - halo;
        g.mask = d_mask;
        return g;
    }
};

// d and hot stay raw pointers: every launch site of every unit hands them to a kernel by value.  The field owns both and frees them when deleted.
struct fs_field {
    fs_ctx *ctx = nullptr;
    int C = 1;
    void *d = nullptr;
    size_t bytes = 0;
    unsigned *hot = nullptr;   // device words: [0] "may hold a speed above 9.95" (fs_device.h; meaningful for 2-channel fields), [1], [2] the same, raised by the op list of a k_velocity_bc_limit launch of parity 0 / 1
    fs_field() = default;
    fs_field(const fs_field &) = delete;
    ~fs_field() { if (d) hipFree(d); if (hot) hipFree(hot); }
};

// per-step history ring (fs_history_*, fs_history.h): probe and face lists of this context's owned rows, the ring and its device counters
struct fs_history {
    int np = 0, nf = 0, cap = 0, every = 1, threads = 256;
    int nparts = 0;                 // workgroups of the split face sum (HIST_SPLIT; 0: the record launch sums the faces)
    fs::DevBuf<double> d_partial;    // [nparts][2]
    fs::DevBuf<fs::HistProbe> d_probes;
    fs::DevBuf<fs::HistFace> d_faces;
    fs::DevBuf<double> d_ring;       // [cap][2 + 3 np]
    fs::DevBuf<long long> d_state;   // [HIST_STATE]
};

// time averages (fs_mean_*, fs_mean.h): the accumulator planes over this context's owned rows and the device counters
struct fs_mean {
    long long every = 1, start = 0;
    size_t plane = 0;               // doubles from one plane to the next: nyl * P + MEAN_PAD
    fs::DevBuf<double> d_sums;       // [MEAN_PLANES][plane]
    fs::DevBuf<long long> d_state;   // [MEAN_STATE]
};

// harmonic flow modes (fs_modes_*, fs_modes.h): the Fourier-sum planes over this context's owned rows, the device counters and scalars
struct fs_modes {
    int nfreq = 1;
    long long every = 1, start = 0;
    double cd[4] = {1, 1, 1, 1}, sd[4] = {0, 0, 0, 0};      // cos / sin of the phase step per sample of each frequency (MODES_MAX_FREQ)
    size_t plane = 0;               // doubles from one plane to the next: nyl * P + MEAN_PAD
    fs::DevBuf<double> d_sums;       // [3 (1 + 2 nfreq)][plane]
    fs::DevBuf<long long> d_state;   // [MODES_STATE]
    fs::DevBuf<double> d_scal;       // [2 nfreq] phasors, then the upper triangle of the Gram matrix
};

// snapshot POD (fs_pod_*, fs_pod.h): the ring of resident snapshots over this context's owned rows, the device counters, the Gram scratch
struct fs_pod {
    int M = 2;
    long long every = 1, start = 0;
    size_t plane = 0;               // elements of the field type from one plane to the next: nyl * P + MEAN_PAD
    fs::DevBuf<void> d_slots;        // [M][3][plane] of the field type: u, w, p
    fs::DevBuf<long long> d_state;   // [POD_STATE]
    fs::DevBuf<double> d_gram;       // fs_pod_gram: the workgroups' partial sums, then the n x n matrix (allocated at the first call)
    size_t gram_cap = 0;            // doubles
};

// flow map through the resident snapshots (fs_flowmap_*, fs_lcs.h): the lattice of nodes over a cell box
struct fs_flowmap {
    int box[4] = {0, 0, 0, 0};      // x0, y0, x1, y1 (cells)
    int r = 1, nx = 0, ny = 0;      // nodes per cell and direction; the lattice
    fs::DevBuf<double> d_pos;        // [3][ny][nx]: x, y, lam
    fs::DevBuf<int> d_status;        // [ny][nx]
};

// vortex identification (fs_vortex_*, fs_vortex.h): the flag, label and id planes of the whole grid, the accumulator table, the ring of samples
struct fs_vortex {
    int criterion = 0, min_area = 4, maxv = 64, maxc = 65536, cap = 1;
    double threshold = 0.0, scale = 1.0;    // scale: 2^(30 - e), what turns om into the integer q
    long long every = 1, start = 0;
    int cells = 0, nblocks = 0, words = 0;  // X * Y; workgroups of the compression / id passes; long long words per sample
    fs::DevBuf<uint8_t> d_flags;     // [Y][X]
    fs::DevBuf<int> d_labels;        // [Y][X]
    fs::DevBuf<int> d_ids;           // [Y][X]: the dense id of every root
    fs::DevBuf<int> d_counts;        // [nblocks]: roots per block, then their exclusive offsets
    fs::DevBuf<long long> d_table;   // [VX_NACC][maxc]
    fs::DevBuf<long long> d_tmp;     // [VX_TMP]
    fs::DevBuf<long long> d_ring;    // [cap][words]
    fs::DevBuf<long long> d_state;   // [VX_STATE]
};

// field distributions (fs_dist_*, fs_dist.h): the tables of every channel - each its bins, then DIST_TAILS words - and the device counters
struct fs_dist {
    int nchan = 0;
    long long every = 1, start = 0;
    fs_dist_spec spec[4];           // as given to fs_dist_create (DIST_MAX_CHANNELS)
    double inv[4] = {0, 0, 0, 0}, inv_b[4] = {0, 0, 0, 0};      // bins / (hi - lo) of both sides
    size_t offset[5] = {0, 0, 0, 0, 0};      // the first word of every channel's table; [nchan]: all words
    fs::DevBuf<long long> d_tables;  // [offset[nchan]]
    fs::DevBuf<long long> d_state;   // [DIST_STATE]
};

// what the two spectral riders share (fs_spec.h): the box, the uploaded tables, the two complex work planes, the cadence and the device counters
namespace fs {
struct SpecPlan {
    int box[4] = {0, 0, 0, 0};      // x0, y0, x1, y1 (cells)
    int nx = 0, ny = 0;             // the box's sides, powers of two
    int detrend = 0;
    double c1x = 0.0, c1y = 0.0;    // the detrend pair
    long long every = 1, start = 0;
    DevBuf<double> d_wx, d_wy;       // [nx], [ny]: the windows
    DevBuf<double> d_twx, d_twy;     // [nx], [ny]: N / 2 pairs (cos, -sin) per axis
    DevBuf<double2> d_a, d_b;        // [nx * ny] each: the work planes; after a sampling launch d_b holds Z', [a][b]
    DevBuf<long long> d_state;       // [SPEC_STATE]
    size_t cells() const { return (size_t)nx * ny; }
};
}  // namespace fs

// energy spectra (fs_spec_*, fs_spec.h): a plan and the power plane
struct fs_spec : fs::SpecPlan {
    fs::DevBuf<double> d_power;      // [nx * ny], [a][b]
};

// cross-spectra (fs_xspec_*, fs_xspec.h): a plan, the pair of quantities and the accumulator planes
struct fs_xspec : fs::SpecPlan {
    int qa = 0, qb = -1;            // the quantities (fs_dist.h); qb -1: one scalar
    int planes = 1;                 // accumulator planes: XSPEC_PLANES for a pair, 1 for one scalar
    double dx = 0.0;
    fs::DevBuf<double> d_acc;        // [planes][nx * ny]: Paa, Pbb, Cre, Cim, each [a][b]
};

// scale-to-scale fluxes (fs_flux_*, fs_flux.h): the box, the region D of the work planes, the half-widths, the three sets of eight work planes
// and the accumulators
struct fs_flux {
    int box[4] = {0, 0, 0, 0};      // x0, y0, x1, y1 (cells)
    int nx = 0, ny = 0;             // the box's sides
    int dx0 = 0, dy0 = 0, DW = 0, DH = 0;      // D: the box dilated by r_max + 1, clipped to the grid
    int nr = 0, r[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // the half-widths, increasing (FLUX_MAX_WIDTHS)
    double dx = 0.0;
    long long every = 1, start = 0;
    fs::DevBuf<double> d_base, d_rows, d_filt;      // [FLUX_NQ][DW * DH] each: q, R and F of the last half-width that ran
    fs::DevBuf<double> d_acc;        // [nr][FLUX_SUMS][nx * ny]: PI, ZF, K, each [b][a]
    fs::DevBuf<long long> d_state;   // [SPEC_STATE + 1]: launches, samples, and a zero (the `when` of fs_flux_filtered)
};

// kinetic-energy budget (fs_budget_*, fs_budget.h): the box, the staggered accumulator planes and the device counters
struct fs_budget {
    int box[4] = {0, 0, 0, 0};      // x0, y0, x1, y1 (cells)
    int nx = 0, ny = 0;             // the box's sides
    double dx = 0.0;
    long long every = 1, start = 0;
    size_t plane = 0;               // doubles from one plane to the next: nx * ny + BUDGET_PAD
    fs::DevBuf<double> d_sums;       // [BUDGET_PLANES][plane], each [b][a]
    fs::DevBuf<long long> d_state;   // [BUDGET_STATE]
};

namespace fs { struct LoadFace; }      // fs_loads.h (included by fs_diag.hip alone)
// body surface loads (fs_loads_*, fs_loads.h): the face list of this context's owned rows, the per-face sums, the ring and the device counters
struct fs_loads {
    int nf = 0, cap = 0;
    long long every = 1, start = 0;
    int nparts = 0;                 // workgroups of the split form (LOADS_SPLIT; 0: one workgroup does the whole launch)
    fs::DevBuf<double> d_partial;    // [nparts][LOADS_REC]
    fs::DevBuf<fs::LoadFace> d_faces;
    fs::DevBuf<double> d_sums;       // [LOADS_SUMS][nf]
    fs::DevBuf<double> d_ring;       // [cap][LOADS_REC]
    fs::DevBuf<long long> d_state;   // [LOADS_STATE]
};

// tracer particles (fs_tracer_*, fs_tracer.h): the particle arrays and the launch counter
struct fs_tracer {
    int n = 0, respawn = 1, max_age = 0;
    fs::DevBuf<double> d_pos;        // [4][n]: x, y, x_seed, y_seed
    fs::DevBuf<int> d_int;           // [4][n]: age, status, respawns, id (slot -> seed index)
    fs::DevBuf<long long> d_count;   // launches since creation
    // fs_tracer_sort (allocated at the first sort, freed with the set)
    bool permuted = false;          // a sort has run since creation / the last write: id may differ from the identity
    fs::DevBuf<double> d_spos;       // [2][n]: x, y in the new order
    fs::DevBuf<int> d_sint;          // [5][n]: age, status, respawns, id in the new order; the key of every slot
    fs::DevBuf<int> d_bins;          // [nbins] counts / cursors, then [nblocks] totals of the scan's tiles
    int nbins = 0, nblocks = 0;
    // inertial sets (fs_tracer_create_inertial)
    bool inertial = false;
    double gx = 0.0, gy = 0.0;
    fs::DevBuf<double> d_vel;        // [4][n]: pu, pw, alpha, tau (slot order)
    fs::DevBuf<double> d_svel;       // [4][n]: the same in the new order (with the sort's scratch)
    std::vector<double> h_resp;     // [2][n]: alpha, tau in SEED order (fs_tracer_write puts the slots back into seed order)
    fs::DevBuf<int> d_dep;           // [Y][X] deposit counts, or nullptr (deposits off)
    // accumulated occupancy (fs_tracer_accum_*): one per set
    fs::DevBuf<unsigned long long> d_acc;      // [2][Y][X]: occupancy, age_sum
    fs::DevBuf<long long> d_acc_state;         // [0] base: the launch count when attached, [1] samples
    long long acc_every = 1, acc_start = 0;
};

namespace fs {

// ---- the objects behind the other handles: one registry (fs_ctx::objects, fs_objects.h), one guard, one no-capture check, one free -------------
enum ObjKind { OBJ_HISTORY, OBJ_LOADS, OBJ_MEAN, OBJ_MODES, OBJ_POD, OBJ_VORTEX, OBJ_FLOWMAP, OBJ_TRACER, OBJ_MG, OBJ_DIST, OBJ_SPEC, OBJ_XSPEC, OBJ_FLUX, OBJ_BUDGET };
// kind, noun and stale-handle text of an object type: FS_OBJECT(type, kind, noun, text), once, in the unit that implements the type
template <typename T> struct ObjInfo;
#define FS_OBJECT(T, KIND, NOUN, STALE) \
    template <> struct fs::ObjInfo<T> { static constexpr int kind = fs::KIND; static constexpr const char *noun = NOUN, *stale = STALE; }

// a create hands its finished object to the context's registry and its caller the handle
template <typename T>
inline T *adopt(fs_ctx *ctx, std::unique_ptr<T> obj) { return ctx->objects.adopt(std::move(obj), ObjInfo<T>::kind); }
// the guard of every entry point that takes a handle (const ones too): a registry lookup that never reads through `h`; only after it may `h` be used
template <typename T>
inline bool handle_ok(const fs_ctx *ctx, const T *h)
{
    if (ctx && ctx->objects.holds(h, ObjInfo<T>::kind)) return true;
    set_error(ObjInfo<T>::stale);
    return false;
}
#define FS_HANDLE(h) do { if (!fs::handle_ok(ctx, h)) return FS_ERR_ARG; } while (0)
// what allocates, copies or synchronises has no place in a capture or on a tape
#define FS_NO_CAPTURE(T, what)                                                                                                        \
    do {                                                                                                                              \
        if (ctx->capturing || ctx->tape_rec) {                                                                                        \
            fs::set_error(std::string(fs::ObjInfo<T>::noun) + " " what " during graph capture / tape recording");                     \
            return FS_ERR_STATE;                                                                                                      \
        }                                                                                                                             \
    } while (0)
// every fs_*_free: null is fine; a live handle leaves the registry and is deleted once the stream is idle - or, inside a capture, when it ends
template <typename T>
inline int object_free(fs_ctx *ctx, T *h)
{
    if (!h) return FS_OK;
    FS_HANDLE(h);
    ctx->objects.free(h, ObjInfo<T>::kind, ctx->capturing, [ctx] { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); });
    return FS_OK;
}

// the small repeats of the riders' entry points
#define FS_EVERY_START(every, start) FS_REQUIRE((every) >= 1 && (start) >= 0, "every must be >= 1 and start >= 0")
#define FS_COUNTERS(launches, samples) \
    FS_REQUIRE((launches) >= 0 && (samples) >= 0 && (samples) <= (launches), "counters must satisfy 0 <= samples <= launches")
// an object's device counters on the host, synchronised
template <int N>
inline int read_counters(fs_ctx *ctx, const long long *d_state, long long (&st)[N])
{
    FS_HIP(hipSetDevice(ctx->device));
    FS_HIP(hipMemcpyAsync(st, d_state, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

// the half-open cell box of an entry point: not empty, inside the X x Y grid
#define FS_BOX(box, X, Y, msg) \
    FS_REQUIRE(0 <= (box)[0] && (box)[0] < (box)[2] && (box)[2] <= (X) && 0 <= (box)[1] && (box)[1] < (box)[3] && (box)[3] <= (Y), msg)

// One buffer of a create: `bytes` of device memory (0: none, the buffer stays null) filled from the host's `src` or, without one, with the byte `fill`.
struct Fill {
    void *buf;
    hipError_t (*alloc)(void *buf, size_t bytes, void **dev);
    size_t bytes;
    const void *src;
    int fill;
    template <typename T>
    Fill(DevBuf<T> &b, size_t bytes, const void *src = nullptr, int fill = 0)
        : buf(&b), alloc([](void *b, size_t n, void **dev) { auto *d = (DevBuf<T> *)b; const hipError_t e = d->alloc(n); *dev = (void *)d->get(); return e; }),
          bytes(bytes), src(src), fill(fill) {}
};
// The buffers of a create: allocated, their fills queued on the stream, one synchronisation (the sources are the caller's / the frame's memory);
// -> the first error.  The caller's unique_ptr destroys what a failed create had built.
inline hipError_t fill_buffers(fs_ctx *ctx, const std::vector<Fill> &list)
{
    hipError_t e = hipSuccess;
    for (const Fill &f : list) {
        void *dev = nullptr;
        if (e == hipSuccess && f.bytes) e = f.alloc(f.buf, f.bytes, &dev);
        if (e == hipSuccess && f.bytes)
            e = f.src ? hipMemcpyAsync(dev, f.src, f.bytes, hipMemcpyHostToDevice, ctx->stream) : hipMemsetAsync(dev, f.fill, f.bytes, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? es : e;
}

// ---- an accumulator's payload behind its counters {launches, samples}: read, set and reset.  `copy` / `zero` queue the payload's transfer on the
// stream and return an FS_* code: dense_copy / dense_zero, or a call of their own.  The argument checks stay with the entry points. ----------------
inline auto dense_copy(fs_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    return [=]() -> int { FS_HIP(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream)); return FS_OK; };
}
inline auto dense_zero(fs_ctx *ctx, void *dst, size_t bytes)
{
    return [=]() -> int { FS_HIP(hipMemsetAsync(dst, 0, bytes, ctx->stream)); return FS_OK; };
}
// the counters, and with `payload` what `copy` downloads
template <typename F>
inline int counted_read(fs_ctx *ctx, const long long *d_state, long long *launches, long long *samples, bool payload, F copy)
{
    long long st[2];
    if (int rc = read_counters(ctx, d_state, st)) return rc;
    if (payload) {
        if (int rc = copy()) return rc;
        FS_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (launches) *launches = st[0];
    if (samples) *samples = st[1];
    return FS_OK;
}
// what `copy` uploads, then the counters; synchronised: the sources are the caller's / this frame's memory
template <typename F>
inline int counted_set(fs_ctx *ctx, long long *d_state, long long launches, long long samples, F copy)
{
    FS_HIP(hipSetDevice(ctx->device));
    const long long st[2] = {launches, samples};
    if (int rc = copy()) return rc;
    FS_HIP(hipMemcpyAsync(d_state, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}
// what `zero` clears, and the samples; the launch count runs on.  Queued only, unless `sync`: for a `zero` that also copied from its caller's frame
template <typename F>
inline int counted_reset(fs_ctx *ctx, long long *d_state, F zero, bool sync = false)
{
    FS_HIP(hipSetDevice(ctx->device));
    if (int rc = zero()) return rc;
    FS_HIP(hipMemsetAsync(d_state + 1, 0, sizeof(long long), ctx->stream));
    if (sync) FS_HIP(hipStreamSynchronize(ctx->stream));
    return FS_OK;
}

// HIP-event pair around a span of stream work that is not one kernel launch (fs_core.hip; the ghost-row exchange chain of fs_comm.hip)
ProfRec prof_span_begin(fs_ctx *c, const char *name, hipStream_t stream);
void prof_span_end(fs_ctx *c, const ProfRec &rec, hipStream_t stream);

// dx (as rounded to T) is an exact power of two: division by it may be replaced by multiplication
template <typename T>
inline bool is_pow2(T x)
{
    int e;
    return x > 0 && std::frexp(x, &e) == (T)0.5;
}

template <typename T>
inline Konst<T> make_konst(fs_ctx *ctx, double dt, double dx, double re, double weight = 0.0, double omega = 0.0)
{
    Konst<T> k;
    k.dt = (T)dt; k.dx = (T)dx; k.re = (T)re;
    k.two_dx = (T)(2.0 * dx);
    k.dx2_fold = (T)std::pow(dx, 2.0);   // Python's float ** int is libm pow()
    k.dx3_fold = (T)std::pow(dx, 3.0);
    k.dx_sq = k.dx * k.dx;
    k.six_dx = (T)6 * k.dx;
    k.eight_dt = (T)8 * k.dt;
    k.dtw = (T)(dt * weight);
    k.om = (T)omega;
    k.om1 = (T)(1.0 - omega);
    // exact-reciprocal shortcut: only when every dx-derived divisor is a power of two and its inverse is finite
    k.p2 = is_pow2(k.dx) && is_pow2(k.dx2_fold) && is_pow2(k.dx3_fold) && std::isfinite((double)((T)1 / k.dx3_fold)) ? 1 : 0;
    k.inv_dx = (T)1 / k.dx;
    k.inv_two_dx = (T)1 / k.two_dx;
    k.inv_dx_sq = (T)1 / k.dx_sq;
    k.inv_dx2_fold = (T)1 / k.dx2_fold;
    k.inv_dx3_fold = (T)1 / k.dx3_fold;
    k.r_dx = 1.0 / (double)k.dx; k.r_two_dx = 1.0 / (double)k.two_dx; k.r_dx_sq = 1.0 / (double)k.dx_sq; k.r_dx2_fold = 1.0 / (double)k.dx2_fold;
    k.r_dx3_fold = 1.0 / (double)k.dx3_fold; k.r_six_dx = 1.0 / (double)k.six_dx; k.r_eight_dt = 1.0 / (double)k.eight_dt; k.r_re = 1.0 / (double)k.re;
    return k;
}

// fs_device.h f64div: x / d can be EXACTLY a tie between two f32 denormals iff d is an even integer (d = D 2^e, D odd, e >= 1); the plain
// f64-multiply division is used only for divisors that admit no such tie
inline bool tie_free(double d)
{
    if (!(d == d) || d == 0.0 || std::isinf(d)) return false;
    int e;
    double m = std::frexp(std::fabs(d), &e);          // |d| = m 2^e, 0.5 <= m < 1
    while (m != std::floor(m)) { m *= 2.0; --e; }     // -> odd integer m times 2^e
    return e < 1;
}
// division mode of a launch (fs_device.h DM_*): which kinds of divisors a kernel has decides how many modes it instantiates
template <typename T> inline int f64_mode(const fs_ctx *c, const Konst<T> &k)      // f32 fields: the f64-multiply division, if every dx- / dt-derived divisor is tie-free
{
    const bool ok = tie_free(k.dx) && tie_free(k.two_dx) && tie_free(k.dx_sq) && tie_free(k.dx2_fold) && tie_free(k.dx3_fold) && tie_free(k.six_dx) && tie_free(k.eight_dt);
    return sizeof(T) == 4 && ok ? DM_F64 : DM_IEEE;
}
template <typename T> inline int dm_all(const fs_ctx *c, const Konst<T> &k) { return (k.p2 ? DM_P2 : 0) | f64_mode<T>(c, k); }   // dx-derived AND other divisors
template <typename T> inline int dm_dx(const fs_ctx *c, const Konst<T> &k) { return k.p2 ? DM_P2 : f64_mode<T>(c, k); }          // dx-derived divisors only
template <typename T> inline int dm_const(const fs_ctx *c, const Konst<T> &k) { return f64_mode<T>(c, k); }                      // no dx-derived divisor

}  // namespace fs
