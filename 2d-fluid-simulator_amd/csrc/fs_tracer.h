// fs_tracer.h - passive tracer particles (new; the reference has none): N fluid parcels advanced by one launch per step that is part of the
// captured step, so that pathlines (respawn off), streaklines (respawn on) and residence times need no velocity download per step.
//
// State (fs_tracer, fs_host.h), structure of arrays: x, y (double, cell units: cell (i, j) covers [i, i + 1) x [j, j + 1), its stored value
// sits at (i + 0.5, j + 0.5)), age (int, steps), status (int: 0 alive, 1 LEFT, 2 WALL, 3 EXPIRED), respawns (int), the constant seeds
// x_seed, y_seed (double) and one launch counter (long long).  Positions are double on purpose: at X = 8192 an f32 position resolves 2^-11
// cell, the size of a slow region's displacement per step.
//
// k_tracer_advance: one lane per particle, one midpoint (RK2) step h = dt / dx in the velocity the solver step just left:
//   V(x, y): bilinear in the four stored values around (x - 0.5, y - 0.5), corner index clamped to [0, X - 2] x [0, Y - 2], weights clamped to
//            [0, 1] (constant extrapolation in the outer half cells); wall cells take part with what they store.  limit > 0: v owes a
//            deferred limit_field - every corner's (u, w) goes through limit_cell in T first, as the pass would store it.
//   k1 = V(x, y); (xm, ym) = (x, y) + (0.5 h) k1; outside the domain -> LEFT.  k2 = V(xm, ym); (xn, yn) = (x, y) + h k2; outside -> LEFT; the
//   mask byte of cell (floor xn, floor yn): wall -> WALL, outflow -> LEFT, else the particle moves.  age += 1; max_age > 0 and age >= max_age
//   and no other fate -> EXPIRED.  A fate either respawns the particle at its seed (age 0, respawns + 1, status stays 0) or sets its status
//   (LEFT / WALL keep the last valid position, EXPIRED keeps (xn, yn)); a particle with status != 0 is never touched again.
// Every operation is ONE correctly rounded double operation in the order written (-ffp-contract=off, no fma): a NumPy float64 restatement
// gives the same bits in f32 and in f64 runs (tests/tracers_ref.py).  inside() is false for NaN, so a NaN velocity ends in LEFT before any
// index is formed from it.  No atomics, a lane writes its own particle only: legal in a hipGraph and bit-identical from run to run.
//
// Shape: three dependent gather rounds (8 corner values, 8 corner values, 1 mask byte) with a handful of f64 operations between them - the
// launch is as long as the chain of one wave, so one particle per lane and as many waves as the registers allow: 256-lane workgroups, the
// eight loads of a stage are issued before the first use (the limit's inputs are those same loads).  Resources and times: DESIGN.md 4aa.
//
// Slots and identity.  The particle arrays are indexed by SLOT; id[slot] is the particle's seed index (the identity until the first sort).
// The seeds stay in seed order and are read as xs[id[k]] on the respawn path only.  fs_tracer_sort reorders the slots by a coarse cell key
// so that the gathers of neighbouring lanes fall into the same cache lines (4aa: 2 759 -> 240 us per advance of 2^24 particles):
//   key = floor(y) * NB + floor(x) / W, NB = ceil(X / W), W = TRACER_SORT_W cells (one 128-byte line of an f32 row); a particle that is
//   not alive, or not inside the domain (NaN included), has key = Y * NB and goes last.
// A counting sort in separate launches, none of which waits for another workgroup: zero the bins (a memset), k_tracer_sort_count (key per
// slot + one integer atomic per particle), an exclusive scan of the Y * NB + 1 bins in three launches (k_tracer_scan_blocks: every
// workgroup scans TRACER_SCAN_TILE bins and stores its total; k_tracer_scan_sums: ONE workgroup scans the totals; k_tracer_scan_add),
// k_tracer_sort_scatter (a returning integer atomic on the bin's cursor gives the destination slot in scratch arrays; the order inside a
// bin is whatever the atomics make it - nothing observable depends on it, every reader goes through id) and k_tracer_sort_copy back into
// the arrays the captured advance launches point to.  k_tracer_fields bins the alive, inside particles by CELL: count (int) and the sum of
// their ages (64-bit) with integer atomics - exact and the same from run to run.  Resources and times: DESIGN.md 4ab.
//
// Inertial sets (fs_tracer_create_inertial).  Beyond the passive state a particle carries its velocity pu, pw (double, the field's velocity
// units), alpha in (0, 1] and tau >= 0 (double); the set carries gravity (gx, gy).  alpha = -expm1(-dt / tau) comes from the host (1 for
// tau == 0): the device evaluates no transcendental function.  k_tracer_advance_inertial, one launch per step, one lane per alive particle:
//   (U, W) = V(x, y)                       tracer_velocity<T, LIM>, as above
//   age == 0: pu = U; pw = W               a particle is released with the fluid's velocity at its position (creation and every respawn)
//   su = tau gx; sw = tau gy               settling velocity
//   pu = pu + alpha ((U + su) - pu)        the exact integral of dv/dt = (U - v) / tau + g over one step with U frozen
//   pw = pw + alpha ((W + sw) - pw)
//   xn = x + h pu; yn = y + h pw           with the NEW velocity; not inside (NaN included) -> LEFT before any index is formed
//   mask(floor xn, floor yn): 1 -> WALL, 3 -> LEFT, else the particle moves; age += 1; max_age as above
// Fates as for passive sets; a respawn also stores pu = pw = 0 (never read: age 0 overwrites them), without respawn the updated pu, pw are
// stored in every case.  One gather stage and one mask byte, not two gather stages: as tau -> 0 (alpha = 1) the scheme is the forward-Euler
// tracer x + h V(x), NOT the passive set's midpoint rule.  A particle may cross more than one cell per step, as a passive one may.
// Deposition (dep != nullptr): a particle whose fate is WALL adds 1 to cell (floor xn, floor yn) of an int plane [Y][X] with one integer
// atomic, respawn or not - exact and the same from run to run.  The sort carries pu, pw, alpha, tau with the slots (32 more bytes of scratch).
//
// k_tracer_accumulate (fs_tracer_accum_*; passive and inertial sets): behind the advance, gated ON THE DEVICE from the set's launch counter
// by fs_mean_accumulate's rule - with n1 = count - base (launches since the accumulator was attached, this step's included) the launch
// samples when n1 > start and (n1 - start) % every == 0.  A sampling launch does what k_tracer_fields does, into resident 64-bit planes
// occupancy and age_sum [Y][X]; lane 0 counts the sample.  A launch that does not sample reads the two counters per workgroup and returns.
// Resources and times: DESIGN.md 4ac.
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int TRACER_WG = 256;
constexpr int TR_ALIVE = 0, TR_LEFT = 1, TR_WALL = 2, TR_EXPIRED = 3;
constexpr int TRACER_SORT_W = 32;                                   // cells per sort bin along x (FS_TRACER_SORT_BIN_CELLS)
constexpr int TRACER_SCAN_ITEMS = 8, TRACER_SCAN_TILE = TRACER_WG * TRACER_SCAN_ITEMS;      // bins per lane / per workgroup of the scan

struct TracerDev {
    int n;
    double *x, *y;
    int *age, *status, *respawns;
    const double *xs, *ys;
    long long *count;
    int *id;      // slot -> seed index
};

__device__ __forceinline__ bool tracer_inside(double x, double y, double X, double Y) { return x >= 0.0 && x < X && y >= 0.0 && y < Y; }

// limit_cell behind a test on the squared speed: s = x x + y y <= 0.98 lim^2 gives RN(sqrt(s)) <= 0.99 lim (1 + 2^-24) < lim, where limit_cell
// changes nothing; NaN fails the test as it fails limit_cell's.  Saves the square root of the sixteen corners of a healthy flow.
template <typename T>
__device__ __forceinline__ void tracer_limit(T &x, T &y, T lim, T safe_sq)
{
    if (x * x + y * y > safe_sq) limit_cell(x, y, lim);
}

// V(x, y) for a point inside the domain
template <typename T, bool LIM>
__device__ __forceinline__ void tracer_velocity(const Grid &g, int Y, const T *__restrict__ v, T lim, double x, double y, double &u, double &w)
{
    const double fx = x - 0.5, fy = y - 0.5;
    const int i0 = min(max((int)floor(fx), 0), g.X - 2), j0 = min(max((int)floor(fy), 0), Y - 2);
    const double tx = fmin(fmax(fx - (double)i0, 0.0), 1.0), ty = fmin(fmax(fy - (double)j0, 0.0), 1.0);
    const size_t o0 = idx<2, T>(g, 0, i0, j0), o1 = idx<2, T>(g, 0, i0, j0 + 1);
    // the eight loads before the first use
    T u00 = v[o0], u10 = v[o0 + 1], w00 = v[o0 + g.P], w10 = v[o0 + g.P + 1];
    T u01 = v[o1], u11 = v[o1 + 1], w01 = v[o1 + g.P], w11 = v[o1 + g.P + 1];
    if (LIM) {
        const T safe_sq = (T)0.98 * lim * lim;
        tracer_limit(u00, w00, lim, safe_sq);
        tracer_limit(u10, w10, lim, safe_sq);
        tracer_limit(u01, w01, lim, safe_sq);
        tracer_limit(u11, w11, lim, safe_sq);
    }
    const double sx = 1.0 - tx, sy = 1.0 - ty;
    u = sy * (sx * (double)u00 + tx * (double)u10) + ty * (sx * (double)u01 + tx * (double)u11);
    w = sy * (sx * (double)w00 + tx * (double)w10) + ty * (sx * (double)w01 + tx * (double)w11);
}

template <typename T, bool LIM>
__global__ __launch_bounds__(TRACER_WG) void k_tracer_advance(Grid g, int Y, double h, double limit, int respawn, int max_age, TracerDev t,
                                                              const T *__restrict__ v)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k == 0) t.count[0] = t.count[0] + 1;        // (nothing in the kernel depends on it)
    if (k >= t.n || t.status[k] != TR_ALIVE) return;
    const double x = t.x[k], y = t.y[k];
    const int age = t.age[k] + 1;
    const double X = (double)g.X, Yd = (double)Y;
    const T lim = (T)limit;
    double px = x, py = y;      // where the particle stays when it is not respawned
    int fate = TR_ALIVE;
    double ku, kw;
    tracer_velocity<T, LIM>(g, Y, v, lim, x, y, ku, kw);
    const double hh = 0.5 * h;
    const double xm = x + hh * ku, ym = y + hh * kw;
    if (!tracer_inside(xm, ym, X, Yd)) fate = TR_LEFT;
    else {
        tracer_velocity<T, LIM>(g, Y, v, lim, xm, ym, ku, kw);
        const double xn = x + h * ku, yn = y + h * kw;
        if (!tracer_inside(xn, yn, X, Yd)) fate = TR_LEFT;
        else {
            const uint8_t m = mask_at(g, (int)floor(xn), (int)floor(yn));
            if (m == 1) fate = TR_WALL;
            else if (m == 3) fate = TR_LEFT;
            else { px = xn; py = yn; }
        }
    }
    if (fate == TR_ALIVE && max_age > 0 && age >= max_age) fate = TR_EXPIRED;
    if (fate != TR_ALIVE && respawn) {
        const int s = t.id[k];
        t.x[k] = t.xs[s];
        t.y[k] = t.ys[s];
        t.age[k] = 0;
        t.respawns[k] = t.respawns[k] + 1;
        return;
    }
    t.x[k] = px;
    t.y[k] = py;
    t.age[k] = age;
    if (fate != TR_ALIVE) t.status[k] = fate;
}

// the additional state of an inertial set: slot-indexed pu, pw, alpha, tau; gravity; the deposit plane [Y][X] or nullptr
struct TracerInertial {
    double *pu, *pw;
    const double *alpha, *tau;
    double gx, gy;
    int *dep;
};

template <typename T, bool LIM>
__global__ __launch_bounds__(TRACER_WG) void k_tracer_advance_inertial(Grid g, int Y, double h, double limit, int respawn, int max_age, TracerDev t,
                                                                       TracerInertial q, const T *__restrict__ v)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k == 0) t.count[0] = t.count[0] + 1;        // (nothing in the kernel depends on it)
    if (k >= t.n || t.status[k] != TR_ALIVE) return;
    const double x = t.x[k], y = t.y[k];
    const int age0 = t.age[k];
    double pu = q.pu[k], pw = q.pw[k];
    const double alpha = q.alpha[k], tau = q.tau[k];
    const double X = (double)g.X, Yd = (double)Y;
    double px = x, py = y;      // where the particle stays when it is not respawned
    int fate = TR_ALIVE;
    double U, W;
    tracer_velocity<T, LIM>(g, Y, v, (T)limit, x, y, U, W);
    if (age0 == 0) { pu = U; pw = W; }
    const double su = tau * q.gx, sw = tau * q.gy;
    pu = pu + alpha * ((U + su) - pu);
    pw = pw + alpha * ((W + sw) - pw);
    const double xn = x + h * pu, yn = y + h * pw;
    if (!tracer_inside(xn, yn, X, Yd)) fate = TR_LEFT;
    else {
        const int i = (int)floor(xn), j = (int)floor(yn);
        const uint8_t m = mask_at(g, i, j);
        if (m == 1) {
            fate = TR_WALL;
            if (q.dep) atomicAdd(&q.dep[(size_t)j * g.X + i], 1);      // (inside: 0 <= i < X, 0 <= j < Y)
        } else if (m == 3) fate = TR_LEFT;
        else { px = xn; py = yn; }
    }
    const int age = age0 + 1;
    if (fate == TR_ALIVE && max_age > 0 && age >= max_age) fate = TR_EXPIRED;
    if (fate != TR_ALIVE && respawn) {
        const int s = t.id[k];
        t.x[k] = t.xs[s];
        t.y[k] = t.ys[s];
        t.age[k] = 0;
        t.respawns[k] = t.respawns[k] + 1;
        q.pu[k] = 0.0;
        q.pw[k] = 0.0;
        return;
    }
    t.x[k] = px;
    t.y[k] = py;
    t.age[k] = age;
    q.pu[k] = pu;
    q.pw[k] = pw;
    if (fate != TR_ALIVE) t.status[k] = fate;
}

// overlay: every alive particle stores the colour into pixel (floor x, floor y) of the 3-channel image field.  All writers of a pixel store
// the same value: the race is benign, the image deterministic.
template <typename T>
__global__ __launch_bounds__(TRACER_WG) void k_tracer_draw(Grid g, int Y, TracerDev t, T r, T gg, T b, T *rgb)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n || t.status[k] != TR_ALIVE) return;
    const double x = t.x[k], y = t.y[k];
    if (!tracer_inside(x, y, (double)g.X, (double)Y)) return;      // (a state written by fs_tracer_write may hold anything)
    const int i = (int)floor(x), j = (int)floor(y);
    rgb[idx<3, T>(g, 0, i, j)] = r;
    rgb[idx<3, T>(g, 1, i, j)] = gg;
    rgb[idx<3, T>(g, 2, i, j)] = b;
}

// ---- fs_tracer_sort: counting sort of the slots by the coarse cell key ------------------------------------------------------------------
__device__ __forceinline__ int tracer_sort_key(double x, double y, int status, int X, int Y, int NB)
{
    if (status != TR_ALIVE || !tracer_inside(x, y, (double)X, (double)Y)) return Y * NB;
    return (int)floor(y) * NB + (int)floor(x) / TRACER_SORT_W;
}

// key[k] and bins[key] += 1 (bins zeroed before)
__global__ __launch_bounds__(TRACER_WG) void k_tracer_sort_count(int X, int Y, int NB, TracerDev t, int *__restrict__ key, int *__restrict__ bins)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n) return;
    const int b = tracer_sort_key(t.x[k], t.y[k], t.status[k], X, Y, NB);
    key[k] = b;
    atomicAdd(&bins[b], 1);
}

// exclusive scan of one workgroup's values (one per lane) through LDS -> the lane's prefix; total: the workgroup's sum
__device__ __forceinline__ int tracer_wg_scan(int v, int *lds, int &total)
{
    const int l = threadIdx.x;
    lds[l] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < TRACER_WG; d <<= 1) {
        const int a = l >= d ? lds[l - d] : 0;
        __syncthreads();
        lds[l] += a;
        __syncthreads();
    }
    total = lds[TRACER_WG - 1];
    const int incl = lds[l];
    __syncthreads();
    return incl - v;
}

// bins[b * TILE ..) -> their exclusive prefix inside the tile, sums[b] = the tile's total
__global__ __launch_bounds__(TRACER_WG) void k_tracer_scan_blocks(int nbins, int *__restrict__ bins, int *__restrict__ sums)
{
    __shared__ int lds[TRACER_WG];
    const int base = blockIdx.x * TRACER_SCAN_TILE + threadIdx.x * TRACER_SCAN_ITEMS;
    int v[TRACER_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int q = 0; q < TRACER_SCAN_ITEMS; ++q) {
        v[q] = base + q < nbins ? bins[base + q] : 0;
        s += v[q];
    }
    int total;
    int run = tracer_wg_scan(s, lds, total);
#pragma unroll
    for (int q = 0; q < TRACER_SCAN_ITEMS; ++q) {
        if (base + q < nbins) bins[base + q] = run;
        run += v[q];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ONE workgroup: sums[0 .. m) -> their exclusive prefix, in rounds of 256 with a running carry
__global__ __launch_bounds__(TRACER_WG) void k_tracer_scan_sums(int m, int *__restrict__ sums)
{
    __shared__ int lds[TRACER_WG];
    int carry = 0;
    for (int b0 = 0; b0 < m; b0 += TRACER_WG) {
        const int i = b0 + threadIdx.x;
        const int v = i < m ? sums[i] : 0;
        int total;
        const int ex = tracer_wg_scan(v, lds, total);
        if (i < m) sums[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(TRACER_WG) void k_tracer_scan_add(int nbins, int *__restrict__ bins, const int *__restrict__ sums)
{
    const int i = blockIdx.x * TRACER_WG + threadIdx.x;
    if (i < nbins) bins[i] += sums[i / TRACER_SCAN_TILE];
}

// slot k -> slot bins[key[k]]++ of the scratch arrays (sx, sy: doubles; si: [4][n] ints age, status, respawns, id)
__global__ __launch_bounds__(TRACER_WG) void k_tracer_sort_scatter(TracerDev t, const int *__restrict__ key, int *__restrict__ bins,
                                                                   double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ si)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n) return;
    const double x = t.x[k], y = t.y[k];
    const int age = t.age[k], status = t.status[k], respawns = t.respawns[k], id = t.id[k];
    const int d = atomicAdd(&bins[key[k]], 1);
    if (d < 0 || d >= t.n) return;      // (cannot happen: the cursors end at the next bin's start; never store outside the arrays)
    const size_t n = (size_t)t.n;
    sx[d] = x;
    sy[d] = y;
    si[d] = age;
    si[n + d] = status;
    si[2 * n + d] = respawns;
    si[3 * n + d] = id;
}

__global__ __launch_bounds__(TRACER_WG) void k_tracer_sort_copy(TracerDev t, const double *__restrict__ sx, const double *__restrict__ sy,
                                                                const int *__restrict__ si)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n) return;
    const size_t n = (size_t)t.n;
    t.x[k] = sx[k];
    t.y[k] = sy[k];
    t.age[k] = si[k];
    t.status[k] = si[n + k];
    t.respawns[k] = si[2 * n + k];
    t.id[k] = si[3 * n + k];
}

// the same for an inertial set: pu, pw, alpha, tau (vel [4][n]) travel with the slot through sv [4][n]
__global__ __launch_bounds__(TRACER_WG) void k_tracer_sort_scatter_inertial(TracerDev t, const int *__restrict__ key, int *__restrict__ bins,
                                                                            double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ si,
                                                                            const double *__restrict__ vel, double *__restrict__ sv)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n) return;
    const size_t n = (size_t)t.n;
    const double x = t.x[k], y = t.y[k];
    const int age = t.age[k], status = t.status[k], respawns = t.respawns[k], id = t.id[k];
    const double q0 = vel[k], q1 = vel[n + k], q2 = vel[2 * n + k], q3 = vel[3 * n + k];
    const int d = atomicAdd(&bins[key[k]], 1);
    if (d < 0 || d >= t.n) return;      // (cannot happen: the cursors end at the next bin's start; never store outside the arrays)
    sx[d] = x;
    sy[d] = y;
    si[d] = age;
    si[n + d] = status;
    si[2 * n + d] = respawns;
    si[3 * n + d] = id;
    sv[d] = q0;
    sv[n + d] = q1;
    sv[2 * n + d] = q2;
    sv[3 * n + d] = q3;
}

__global__ __launch_bounds__(TRACER_WG) void k_tracer_sort_copy_inertial(TracerDev t, const double *__restrict__ sx, const double *__restrict__ sy,
                                                                         const int *__restrict__ si, double *__restrict__ vel, const double *__restrict__ sv)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n) return;
    const size_t n = (size_t)t.n;
    t.x[k] = sx[k];
    t.y[k] = sy[k];
    t.age[k] = si[k];
    t.status[k] = si[n + k];
    t.respawns[k] = si[2 * n + k];
    t.id[k] = si[3 * n + k];
    vel[k] = sv[k];
    vel[n + k] = sv[n + k];
    vel[2 * n + k] = sv[2 * n + k];
    vel[3 * n + k] = sv[3 * n + k];
}

// ---- fs_tracer_fields: per-cell count and age sum of the alive particles inside the domain (arrays [Y][X], zeroed before) ----------------
__global__ __launch_bounds__(TRACER_WG) void k_tracer_fields(int X, int Y, TracerDev t, int *__restrict__ count, unsigned long long *__restrict__ age_sum)
{
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k >= t.n || t.status[k] != TR_ALIVE) return;
    const double x = t.x[k], y = t.y[k];
    if (!tracer_inside(x, y, (double)X, (double)Y)) return;
    const size_t c = (size_t)(int)floor(y) * X + (int)floor(x);
    atomicAdd(&count[c], 1);
    atomicAdd(&age_sum[c], (unsigned long long)(long long)t.age[k]);
}


// ---- fs_tracer_accum_*: the same binning into resident 64-bit planes, on the launches the rule selects ----------------------------------
// state: [0] base - the set's launch count when the accumulator was attached, [1] samples.  Runs behind the advance: count is final here.
__global__ __launch_bounds__(TRACER_WG) void k_tracer_accumulate(int X, int Y, TracerDev t, long long start, long long every, long long *state,
                                                                 unsigned long long *__restrict__ occupancy, unsigned long long *__restrict__ age_sum)
{
    // (its own copy of the rule, fs_device.h samples_at: the advance has counted itself, and samples_at(n1 - 1, ...) compiles to other instructions)
    const long long n1 = t.count[0] - state[0];
    if (!(n1 > start && (n1 - start) % every == 0)) return;      // (the same in every lane of every workgroup)
    const int k = blockIdx.x * TRACER_WG + threadIdx.x;
    if (k == 0) state[1] = state[1] + 1;            // (no lane reads it)
    if (k >= t.n || t.status[k] != TR_ALIVE) return;
    const double x = t.x[k], y = t.y[k];
    if (!tracer_inside(x, y, (double)X, (double)Y)) return;
    const size_t c = (size_t)(int)floor(y) * X + (int)floor(x);
    atomicAdd(&occupancy[c], 1ull);
    atomicAdd(&age_sum[c], (unsigned long long)(long long)t.age[k]);
}

}  // namespace fs
