// fs_dist.h - field distributions (new; the reference has none): histograms and joint histograms of a quantity over the fluid cells, accumulated
// over a run on the device, and exact order statistics of the current fields.  Counts are integers and an order statistic is
// one stored value: both are exact, independent of the order of any atomic, and compared with == against NumPy (tests/dist_ref.py).  No float
// atomic appears anywhere in this header.  Single-GPU contexts.
//
// THE VALUE OF A CELL.  Quantities by index: 0 "u", 1 "w", 2 "p", 3 "speed", 4 "vorticity", 5 "q", 6 "swirl".  All are doubles, every operation
// rounded on its own (-ffp-contract=off):
//     u, w        the stored values promoted to double - through limit_cell while v still owes a deferred limit_field (limit > 0, the
//                 convention of fs_vortex_launch / fs_pod_*).  p is taken as stored.
//     speed       t = u * u;  t = t + w * w;  sqrt(t), correctly rounded (u, w as above)
//     vorticity   VxGrad::om of fs_vortex.h (signed);  q, swirl: vortex_criterion(0 / 1, ...) of fs_vortex.h.  vortex_grad and
//                 vortex_criterion are used as they stand: on a fluid cell the value equals fs_vortex_criterion's bit for bit.
// SELECTION: the fluid cells (mask == 0) inside a half-open box (x0, y0, x1, y1) of global cells.
// CLASSIFICATION: NaN is counted in `nan` and takes no further part.  +-Inf are values: a histogram puts them below / above, the order
// statistics rank them.
//
// THE BIN RULE (dist_bin, compiled by the host compiler too): a range [lo, hi) of B bins, inv = B / (hi - lo) computed by the host in double.
//     x < lo -> below;  x >= hi -> above (x itself is compared, never a scaled value);  otherwise floor((x - lo) * inv), clamped to B - 1.
// The clamp matters: with lo = -1, hi = 1, B = 4096 the largest double below 1 scales to exactly 4096.0.  This is not np.histogram's rule
// (which closes the last bin on the right).  A joint table of quantities a, b has Ba * Bb <= DIST_MAX_BINS bins, bin bb * Ba + ba; a value
// outside either range is counted in one `outside` counter.
//
// a. k_dist_accumulate<T, JOINT> - one pass over the workgroups that meet the box, shaped like the flag pass of fs_vortex.h: a lane takes one
//    column and DIST_G rows at a time, the masks of the group first, then - unless no cell of the group is selected - every load of the group
//    before the first use.  A workgroup keeps a private table of 32-bit counters in LDS (it sees at most 256 x DIST_ROWS = 8192 cells: no
//    counter overflows), zeroes the words it uses, counts with LDS integer atomics, and ends by adding its non-zero bins to the global table
//    of 64-bit counters with integer atomics.  The tails and nan are summed per lane, then over the wave by shuffles, then over the
//    workgroup in the table's last words, and added with one atomic each.  A launch that does not sample (samples_at) returns at once;
//    k_dist_tick, one lane behind the channels' launches, advances the counters [0] launches, [1] samples.
// b. fs_dist_select - radix select on the order-preserving 64-bit key of the double: bits ^ 0x8000... for a clear sign bit, ~bits for a set
//    one (-0.0 sorts below +0.0: distinct keys, equal values).  k_dist_values writes the selection's values into a dense plane of doubles over
//    the box (NaN on cells that are not selected) and counts n (selected, not NaN) and nan.  k_dist_digits reads only that plane: for every
//    distinct prefix found so far (blockIdx.y) it counts one digit of the keys that match the prefix - LDS-private table, integer atomics,
//    as above.  Digits are 11 bits from the top, six passes, the last of 9 bits; between two passes the host downloads the tables and
//    picks every rank's digit (dist_pick).
//
// No instantiation may use scratch (tests/test_build_metadata_dist.py).
#pragma once

#if defined(__HIPCC__)
#define FS_DIST_HD __host__ __device__ inline
#else
#define FS_DIST_HD inline
#endif

#include <math.h>
#include <string.h>

namespace fs {

constexpr int DIST_NQ = 7;                // quantities
constexpr int DIST_MAX_BINS = 4096;       // bins of a table, Ba * Bb of a joint one (FS_DIST_MAX_BINS)
constexpr int DIST_MAX_CHANNELS = 4;      // tables of one object (FS_DIST_MAX_CHANNELS)
constexpr int DIST_MAX_RANKS = 8;         // ranks of one fs_dist_select (FS_DIST_MAX_RANKS)
constexpr int DIST_TAILS = 4;             // words behind a table (FS_DIST_NTAIL): [0] below (joint: outside), [1] above, [2] nan, [3] 0
constexpr int DIST_BELOW = -1, DIST_ABOVE = -2, DIST_NAN = -3;      // what dist_bin returns for a value without a bin
constexpr int DIST_PASSES = 6;            // digits of a key
constexpr int DIST_DIGITS = 2048;         // counters of a digit table: 2^11

FS_DIST_HD int dist_bin(double x, double lo, double hi, double inv, int B)
{
    if (x != x) return DIST_NAN;
    if (x < lo) return DIST_BELOW;
    if (x >= hi) return DIST_ABOVE;
    const double s = floor((x - lo) * inv);
    return s < (double)B ? (int)(long long)s : B - 1;
}

FS_DIST_HD unsigned long long dist_key(double x)
{
    unsigned long long b;
    memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
FS_DIST_HD double dist_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? k ^ 0x8000000000000000ull : ~k;
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}
// digit `pass` (0 .. 5) of a key: bits [shift, shift + width)
FS_DIST_HD int dist_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
FS_DIST_HD int dist_width(int pass) { return pass < 5 ? 11 : 9; }
FS_DIST_HD int dist_digit(unsigned long long key, int pass) { return (int)((key >> dist_shift(pass)) & ((1u << dist_width(pass)) - 1u)); }
// whether `key` agrees with `prefix` in the digits above digit `pass`
FS_DIST_HD bool dist_match(unsigned long long key, unsigned long long prefix, int pass)
{
    const int hb = dist_shift(pass) + dist_width(pass);
    return hb >= 64 || (key >> hb) == (prefix >> hb);
}
// the digit that holds rank `rank` (0-based) of a table of `nd` counts -> the digit, *within: the rank among the keys of that digit; -1: rank >= total
inline int dist_pick(const long long *table, int nd, long long rank, long long *within)
{
    long long before = 0;
    for (int d = 0; d < nd; ++d) {
        if (rank < before + table[d]) { *within = rank - before; return d; }
        before += table[d];
    }
    return -1;
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_vortex.h"

namespace fs {

constexpr int DIST_G = 4;                 // rows per load group
constexpr int DIST_ROWS = 32;             // most rows per workgroup: 256 x 32 cells, far below 2^32 per counter
constexpr int DIST_STATE = 2;             // device counters (long long): [0] launches, [1] samples
constexpr int DIST_VALUES_PER_WG = 8192;  // plane values per workgroup of k_dist_digits: 32 per lane
enum { DIST_NEED_UW = 1, DIST_NEED_P = 2, DIST_NEED_GRAD = 4 };
inline int dist_need(int q) { return q < 0 ? 0 : q == 2 ? DIST_NEED_P : q >= 4 ? DIST_NEED_GRAD : DIST_NEED_UW; }

// when a launch of the accumulation works: when launch state[0] samples (histogram()'s temporary object: its launch 0, every 1 from 0)
struct DistWhen { const long long *state; long long start, every; };
__device__ __forceinline__ bool dist_on(const DistWhen &w) { return samples_at(w.state[0], w.start, w.every); }

// what a pass walks: the workgroups from (bx0, by0) on, of 256 columns and rpw rows of the whole grid, and the box that selects
struct DistWalk { int Y, rpw, bx0, by0, x0, y0, x1, y1, need; double dx, limit; };
struct DistChan { int qa, qb, Ba, Bb; double loa, hia, inva, lob, hib, invb; };

template <typename T>
struct DistLoads { T u, w, p, ul, wl, ur, wr, um, wm, un, wn; };

template <typename T>
__device__ __forceinline__ double dist_quantity(int q, T u, T w, T p, const VxGrad &d)
{
    if (q == 0) return (double)u;
    if (q == 1) return (double)w;
    if (q == 2) return (double)p;
    if (q == 3) {
        double t = (double)u * (double)u;
        t = t + (double)w * (double)w;
        return __dsqrt_rn(t);
    }
    if (q == 4) return d.om;
    return vortex_criterion(q == 5 ? 0 : 1, d);
}

// the walk of every pass (its callers' lambdas are always_inline: a call that stays a call keeps the captured counters in scratch):
// cell(i, j, selected, a, b) for every cell of the workgroup's columns and rows that lies in the grid, in every lane
// alike (lanes beyond the grid's width stay in the loop with nothing selected, so the callers may use barriers and wave operations)
template <typename T, typename F>
__device__ __forceinline__ void dist_walk(const Grid &g, const DistWalk &k, int qa, int qb, const T *v, const T *p, F cell)
{
    const int i = (k.bx0 + blockIdx.x) * 256 + threadIdx.x;
    const bool inx = i >= k.x0 && i < k.x1;      // (x1 <= X)
    const int ic = i < g.X ? i : g.X - 1;
    const int il = clampx(g, ic - 1), ir = clampx(g, ic + 1);
    const double two_dx = 2.0 * k.dx;
    const T limit = (T)k.limit;
    const int j0 = (k.by0 + blockIdx.y) * k.rpw;
    const int j1 = j0 + k.rpw < k.Y ? j0 + k.rpw : k.Y;
    for (int jg = j0; jg < j1; jg += DIST_G) {
        unsigned sel = 0;      // bit r: row jg + r is selected (rows of the group beyond j1 are not)
#pragma unroll
        for (int r = 0; r < DIST_G; ++r) {
            const int j = jg + r;
            if (inx && j < j1 && j >= k.y0 && j < k.y1 && mask_at(g, ic, j) == 0) sel |= 1u << r;
        }
        const bool any = sel != 0;
        DistLoads<T> c[DIST_G];
        if (any) {
#pragma unroll
            for (int r = 0; r < DIST_G; ++r) {
                const int j = min(jg + r, j1 - 1), jm = clampy(g, j - 1), jn = clampy(g, j + 1);
                if (k.need & DIST_NEED_UW) { c[r].u = at<2>(v, g, 0, ic, j); c[r].w = at<2>(v, g, 1, ic, j); }
                if (k.need & DIST_NEED_P) c[r].p = at<1>(p, g, 0, ic, j);
                if (k.need & DIST_NEED_GRAD) {
                    c[r].ul = at<2>(v, g, 0, il, j); c[r].wl = at<2>(v, g, 1, il, j);
                    c[r].ur = at<2>(v, g, 0, ir, j); c[r].wr = at<2>(v, g, 1, ir, j);
                    c[r].um = at<2>(v, g, 0, ic, jm); c[r].wm = at<2>(v, g, 1, ic, jm);
                    c[r].un = at<2>(v, g, 0, ic, jn); c[r].wn = at<2>(v, g, 1, ic, jn);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < DIST_G; ++r) {
            const int j = jg + r;
            if (j >= j1) continue;
            double a = 0.0, b = 0.0;
            const bool s = (sel >> r) & 1u;
            if (s) {
                T u = (T)0, w = (T)0, pp = (T)0;
                VxGrad d = {0.0, 0.0, 0.0, 0.0, 0.0};
                if (k.need & DIST_NEED_UW) {
                    u = c[r].u; w = c[r].w;
                    if (limit > (T)0) limit_cell(u, w, limit);
                }
                if (k.need & DIST_NEED_P) pp = c[r].p;
                if (k.need & DIST_NEED_GRAD) d = vortex_grad(c[r].ul, c[r].wl, c[r].ur, c[r].wr, c[r].um, c[r].wm, c[r].un, c[r].wn, limit, two_dx);
                a = dist_quantity(qa, u, w, pp, d);
                if (qb >= 0) b = dist_quantity(qb, u, w, pp, d);
            }
            cell(i, j, s, a, b);
        }
    }
}

__device__ __forceinline__ int dist_wave_sum(int x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
__device__ __forceinline__ void dist_add(long long *p, long long x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); }

#ifndef FS_DIST_COMBINE
#define FS_DIST_COMBINE 0      // (A/B) 1: the lanes of a wave whose cells all fall into one bin combine before the LDS atomic
#endif
// counts: the channel's table of Ba (JOINT: Ba * Bb) words, the DIST_TAILS words behind it
template <typename T, bool JOINT>
__global__ __launch_bounds__(256) void k_dist_accumulate(Grid g, DistWalk k, DistWhen when, DistChan ch, const T *v, const T *p, long long *counts)
{
    __shared__ unsigned table[DIST_MAX_BINS + DIST_TAILS];
    if (!dist_on(when)) return;      // (the same in every lane of every workgroup: k_dist_tick writes behind the channels' launches)
    const int nb = JOINT ? ch.Ba * ch.Bb : ch.Ba;
    for (int b = threadIdx.x; b < nb; b += 256) table[b] = 0;
    if (threadIdx.x < DIST_TAILS) table[DIST_MAX_BINS + threadIdx.x] = 0;
    __syncthreads();
    int below = 0, above = 0, nan = 0;
    dist_walk<T>(g, k, ch.qa, JOINT ? ch.qb : -1, v, p, [&](int, int, bool s, double a, double b) __attribute__((always_inline)) {
        int bin = -1;      // the cell's word of the table; -1: none (not selected, a tail, NaN)
        if (s) {
            const int ba = dist_bin(a, ch.loa, ch.hia, ch.inva, ch.Ba);
            // (sums of comparisons, not an if-chain of increments: the compiler turns that into an indexed counter array in scratch)
            if (JOINT) {
                const int bb = dist_bin(b, ch.lob, ch.hib, ch.invb, ch.Bb);
                const bool none = ba == DIST_NAN || bb == DIST_NAN, out = !none && (ba < 0 || bb < 0);
                nan += none;
                below += out;      // outside
                if (!none && !out) bin = bb * ch.Ba + ba;
            } else {
                nan += ba == DIST_NAN;
                below += ba == DIST_BELOW;
                above += ba == DIST_ABOVE;
                if (ba >= 0) bin = ba;
            }
        }
        if (FS_DIST_COMBINE) {      // (every lane of the wave is here: dist_walk keeps them together)
            const unsigned long long m = __ballot(bin >= 0);
            if (!m) return;
            const int first = __ffsll((long long)m) - 1, bin0 = __shfl(bin, first, 64);
            if (__all(bin < 0 || bin == bin0)) {      // one bin in the whole wave: one lane adds the count
                if ((int)(threadIdx.x & 63) == first) atomicAdd(&table[bin0], (unsigned)__popcll(m));
                return;
            }
        }
        if (bin >= 0) atomicAdd(&table[bin], 1u);
    });
    below = dist_wave_sum(below); above = dist_wave_sum(above); nan = dist_wave_sum(nan);
    if ((threadIdx.x & 63) == 0) {
        if (below) atomicAdd(&table[DIST_MAX_BINS + 0], (unsigned)below);
        if (above) atomicAdd(&table[DIST_MAX_BINS + 1], (unsigned)above);
        if (nan) atomicAdd(&table[DIST_MAX_BINS + 2], (unsigned)nan);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 256) {
        const unsigned c = table[b];
        if (c) dist_add(counts + b, c);
    }
    if (threadIdx.x < 3) {
        const unsigned c = table[DIST_MAX_BINS + threadIdx.x];
        if (c) dist_add(counts + nb + threadIdx.x, c);
    }
}

// behind the channels' launches on the same stream: the launch count, and the sample count when the launch sampled
__global__ __launch_bounds__(64) void k_dist_tick(long long start, long long every, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) state[1] = state[1] + 1;
    state[0] = n + 1;
}

// plane: the values of the box, dense, row (j - y0) of x1 - x0 doubles - NaN on cells that are not selected; nullptr: the counts alone.
// tot: [0] selected cells whose value is not NaN, [1] selected cells whose value is NaN
template <typename T>
__global__ __launch_bounds__(256) void k_dist_values(Grid g, DistWalk k, int q, const T *v, const T *p, double *plane, long long *tot)
{
    __shared__ unsigned part[2];
    if (threadIdx.x < 2) part[threadIdx.x] = 0;
    __syncthreads();
    int n = 0, nan = 0;
    const size_t bw = (size_t)(k.x1 - k.x0);
    dist_walk<T>(g, k, q, -1, v, p, [&](int i, int j, bool s, double a, double) __attribute__((always_inline)) {
        if (s) { if (a != a) ++nan; else ++n; }
        if (plane && i >= k.x0 && i < k.x1 && j >= k.y0 && j < k.y1) plane[(size_t)(j - k.y0) * bw + (size_t)(i - k.x0)] = s ? a : __longlong_as_double(0x7ff8000000000000ll);
    });
    n = dist_wave_sum(n); nan = dist_wave_sum(nan);
    if ((threadIdx.x & 63) == 0) {
        if (n) atomicAdd(&part[0], (unsigned)n);
        if (nan) atomicAdd(&part[1], (unsigned)nan);
    }
    __syncthreads();
    if (threadIdx.x < 2 && part[threadIdx.x]) dist_add(tot + threadIdx.x, part[threadIdx.x]);
}

// tables[blockIdx.y][digit]: how many keys of the plane's `n` values that match prefix[blockIdx.y] above digit `pass` hold each value of it
struct DistPrefixes { unsigned long long p[DIST_MAX_RANKS]; };
__global__ __launch_bounds__(256) void k_dist_digits(const double *plane, size_t n, int pass, DistPrefixes pre, long long *tables)
{
    __shared__ unsigned table[DIST_DIGITS];
    const int nd = 1 << dist_width(pass);
    for (int d = threadIdx.x; d < nd; d += 256) table[d] = 0;
    __syncthreads();
    const unsigned long long prefix = pre.p[blockIdx.y];
    const size_t base = (size_t)blockIdx.x * DIST_VALUES_PER_WG;
    const size_t end = base + DIST_VALUES_PER_WG < n ? base + DIST_VALUES_PER_WG : n;
    for (size_t e = base + threadIdx.x; e < end; e += 256) {
        const double x = plane[e];
        if (x != x) continue;
        const unsigned long long key = dist_key(x);
        if (dist_match(key, prefix, pass)) atomicAdd(&table[dist_digit(key, pass)], 1u);
    }
    __syncthreads();
    long long *out = tables + (size_t)blockIdx.y * DIST_DIGITS;
    for (int d = threadIdx.x; d < nd; d += 256) {
        const unsigned c = table[d];
        if (c) dist_add(out + d, c);
    }
}

}  // namespace fs
#endif  // __HIPCC__
