// fs_vortex.h - vortex identification (new; the reference has none): a criterion field of the velocity gradient, its connected components
// labelled on the device in a FIXED number of launches, one record of integer sums per component, appended to a ring of samples that stays on
// the device.  The whole sequence can sit in a hipGraph: whether a launch samples is decided on the device (samples_at,
// fs_device.h), and a launch that does not sample returns at once in every kernel.  Single-GPU contexts.
//
// THE INVARIANT THAT MAKES EVERY LOOP HERE FINITE: in a parent plane L, L[x] <= x for every cell x that takes part, at every moment.  A plane
// starts as the identity; the only write a union makes is uf_min(&L[a], b) with b < a (an atomic minimum: it can only lower L[a]), and the only
// other write is the compression's L[x] = uf_find(L, x) <= x.  uf_find therefore walks a strictly decreasing chain of non-negative integers,
// and stops by itself on a value that does not decrease (which the invariant rules out for anything but a root).  uf_union attaches the
// larger of two roots under the smaller and RETRIES ONLY ON THE VALUE THE ATOMIC RETURNED: when L[a] was not a any more, another union got
// there first, the old parent `old` < a of a has still to meet b, and the pair (old, b) is smaller than (a, b) - the sum of the pair falls
// with every round.  The minimum of a component does not depend on the order of the atomics: the labels are unique, and tested exactly.
// uf_find / uf_union are plain functions over an int*, with the atomic and the load behind uf_min / uf_load: the same text is compiled by
// the host compiler into libfs_vortex_host.so (fs_vortex_host.cpp), where tests/test_vortex_cpu.py runs the unions of all seams in shuffled
// sequential orders before any kernel sees a GPU.
//
// a. k_vortex_flags - criterion and flags, one pass over v and the mask, in double on the stored values promoted to double (through limit_cell
//    while v still owes a deferred limit_field), neighbour indices clamped at the domain edge as in k_flow_stats.  With two_dx = 2.0 * dx and
//    every product, sum and quotient rounded on its own (-ffp-contract=off):
//        ux = (ur - ul) / two_dx   uy = (un - um) / two_dx   wx = (wr - wl) / two_dx   wy = (wn - wm) / two_dx
//        om = ((wr - wl) - (un - um)) / two_dx                                    (the om of k_flow_stats)
//        "q" (0):          t = ux * ux;  t = t + wy * wy;  c = (-0.5 * t) - uy * wx
//        "swirl" (1):      s = ux + wy;  c = (ux * wy - uy * wx) - 0.25 * (s * s)
//        "vorticity" (2):  c = om * om
//    flag = 1 (om >= 0) or 2 (otherwise) on a fluid cell (mask 0) with c > threshold (false for NaN), else 0.  A lane takes one column and
//    VX_G rows at a time: the masks of the group first, then - unless no cell of the group is fluid - every load of the group before the
//    first use.  The same kernel writes the criterion itself as a double plane (0 on cells that are not fluid) for fs_vortex_criterion.
//    Its lanes also reset the accumulator table and the sample's counters (a grid-stride loop).  Planes are dense: cell (i, j) at j * X + i.
// b. labels: k_vortex_local resolves a tile of VX_TX x VX_TY = 32 x 8 cells in LDS (one cell per lane; unions with the left and the lower
//    neighbour of equal flag) and writes each cell's tile-local root as a GLOBAL index j * X + i (row-major order inside a tile agrees with
//    the global order, so the invariant carries over); k_vortex_seam unites across every tile edge, one lane per pair of cells that face each
//    other over an edge; k_vortex_compress replaces every parent by its root - the smallest j * X + i of the 4-connected component of equal
//    flag - and counts the roots (label == index) of its 1024 cells.  Cells without a flag hold -1.
// c. dense ids: k_vortex_scan (one workgroup) turns the per-block root counts into exclusive offsets and the total; k_vortex_ids numbers the
//    roots 0, 1, 2, ... in ascending label order (ids[root]) and notes the label of every id < max_components in the table.
// d. k_vortex_reduce - integer accumulators only, so that the order of the atomics does not matter and a NumPy restatement gives the same
//    integers: q = llrint(om * 2^(30 - e)) clamped to +-2^30 (a clamped cell, and a NaN, which takes q = 0, adds 1 to `clipped`), per
//    component (table[word][id], long long, max_components ids):
//        0 area  1 sum q  2 sum |q|  3 sum (2i+1)  4 sum (2j+1)  5, 6 sum |q|(2i+1): low 32 bits / the rest of every term  7, 8 the same for
//        |q|(2j+1)  9 min i  10 max i  11 min j  12 max j  13 peak = max of (|q| << 32) | (0xFFFFFFFF - index)  14 label
//    BOUNDS (the largest grid is res 8192: 2^27 cells, 2i+1 < 2^15): area <= 2^27; |sum q|, sum |q| <= 2^27 2^30 = 2^57; sum (2i+1) < 2^42;
//    a term |q|(2i+1) < 2^45: its low word < 2^32 sums below 2^59, the rest < 2^13 sums below 2^40; |q| << 32 <= 2^62.  Nothing reaches 2^63.
//    Cells of roots beyond max_components are counted (`dropped` cells of the sample) and not accumulated.  Lanes of a wave whose cells all
//    belong to one component combine by shuffles before the atomics (integer sums: the same result).
// e. k_vortex_records (one workgroup) walks the table in id order, keeps the components with area >= min_area and writes the first
//    max_vortices of them into sample state[1] of the ring: VX_HEAD words (launch index, components, passed, count, clipped, dropped), then
//    VX_REC words per record (label, words 0 .. 13 of the table, the flag of the root).  k_vortex_tick, one lane behind them, advances the
//    counters: [0] launches, [1] samples in the ring, [2] samples lost to a full ring.  A sampling launch that finds the ring full does nothing.
//
// No instantiation may use scratch (tests/test_build_metadata_vortex.py).
#pragma once

#if defined(__HIPCC__)
#define FS_UF __host__ __device__ inline
#else
#define FS_UF inline
#endif

namespace fs {

constexpr int VX_TX = 32, VX_TY = 8;      // the tile of k_vortex_local: one cell per lane of a 256-lane workgroup

FS_UF int uf_load(const int *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (never a stale line of this CU's cache, never hoisted)
#else
    return *p;
#endif
}
// *p = min(*p, v) -> the value before
FS_UF int uf_min(int *p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}
// the root of x: strictly decreasing by the invariant; a parent that does not decrease (a root: L[x] == x) ends the walk
FS_UF int uf_find(const int *L, int x)
{
    for (;;) {
        const int p = uf_load(L + x);
        if (p >= x || p < 0) return x;
        x = p;
    }
}
FS_UF void uf_union(int *L, int a, int b)
{
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = uf_min(L + a, b);      // a > b: the larger root under the smaller
        if (old >= a) return;                  // a was a root: done
        a = old;                               // it was not any more: its parent of then, old < a, has still to meet b
    }
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_kernels.h"

namespace fs {

constexpr int VX_G = 4;                   // rows per load group of k_vortex_flags
constexpr int VX_ROWS = 32;               // most rows per workgroup of k_vortex_flags
constexpr int VX_BLOCK = 1024;            // cells per workgroup of k_vortex_compress / k_vortex_ids: 4 consecutive ones per lane
constexpr int VX_NACC = 15;               // words per component of the table (FS_VORTEX_NACC)
constexpr int VX_REC = 16;                // words per record (FS_VORTEX_NREC)
constexpr int VX_HEAD = 8;                // words in front of a sample's records (FS_VORTEX_NHEAD)
constexpr int VX_STATE = 4;               // device counters (long long): [0] launches, [1] samples in the ring, [2] samples lost
constexpr int VX_SLOTS = 256;             // the clipped / dropped counters are spread over this many words each: every wave adds to the word of
                                          // its workgroup (blockIdx % VX_SLOTS) - one word for all waves of a large grid serialises them
constexpr int VX_TMP = 2 + 2 * VX_SLOTS;  // per-sample scratch (long long): [0] components, [2 ..) clipped, [2 + VX_SLOTS ..) dropped cells
constexpr int VX_MAX_VORTICES = 1024;     // most records per sample (FS_VORTEX_MAX_VORTICES)
constexpr long long VX_QMAX = 1ll << 30;

// when a launch of the sequence works: always (state == nullptr: the one-shot primitives), or when launch state[0] samples and the ring has room
struct VxWhen { const long long *state; long long start, every; int cap; };
__device__ __forceinline__ bool vortex_on(const VxWhen &w)
{
    return !w.state || (samples_at(w.state[0], w.start, w.every) && w.state[1] < w.cap);
}

// the gradient terms of a cell from its four neighbours' (u, w), in the order of the header: VxGrad and vortex_grad of fs_cell.h
__device__ __forceinline__ double vortex_criterion(int which, const VxGrad &d)
{
    if (which == 0) {
        double t = d.ux * d.ux;
        t = t + d.wy * d.wy;
        return (-0.5 * t) - d.uy * d.wx;
    }
    if (which == 1) {
        const double s = d.ux + d.wy;
        return (d.ux * d.wy - d.uy * d.wx) - 0.25 * (s * s);
    }
    return d.om * d.om;
}
// the gradient of cell (i, j) by direct loads (k_vortex_reduce: flagged cells only)
template <typename T>
__device__ __forceinline__ VxGrad vortex_grad_at(const Grid &g, const T *v, int i, int j, T limit, double two_dx)
{
    const int il = clampx(g, i - 1), ir = clampx(g, i + 1), jm = clampy(g, j - 1), jn = clampy(g, j + 1);
    return vortex_grad(at<2>(v, g, 0, il, j), at<2>(v, g, 1, il, j), at<2>(v, g, 0, ir, j), at<2>(v, g, 1, ir, j), at<2>(v, g, 0, i, jm),
                       at<2>(v, g, 1, i, jm), at<2>(v, g, 0, i, jn), at<2>(v, g, 1, i, jn), limit, two_dx);
}

// FIELD: the criterion as a double plane `crit` (0 where the cell is not fluid); otherwise the flag plane, and the reset of the table
// (`nacc` words of `maxc` ids: the minima to INT_MAX, the rest to 0) and of the sample's scratch counters.  A workgroup takes 256 columns and
// `rpw` rows of the whole single-GPU grid (local row = global row).
template <typename T, bool FIELD>
__global__ __launch_bounds__(256) void k_vortex_flags(Grid g, int Y, int rpw, VxWhen when, int which, double threshold, double dx, double limit,
                                                      const T *v, uint8_t *flags, double *crit, long long *table, int maxc, long long *tmp)
{
    if (!vortex_on(when)) return;
    if (!FIELD) {
        const size_t nthreads = (size_t)gridDim.x * gridDim.y * 256, me = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        const size_t words = (size_t)VX_NACC * maxc;
        for (size_t w = me; w < words; w += nthreads) {
            const int f = (int)(w / maxc);
            table[w] = f == 9 || f == 11 ? 0x7fffffffll : 0ll;
        }
        for (size_t w = me; w < VX_TMP; w += nthreads) tmp[w] = 0;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.X) return;
    const int il = clampx(g, i - 1), ir = clampx(g, i + 1);
    const double two_dx = 2.0 * dx;
    const int j0 = blockIdx.y * rpw;
    const int j1 = j0 + rpw < Y ? j0 + rpw : Y;
    for (int jg = j0; jg < j1; jg += VX_G) {
        uint8_t mk[VX_G];
        bool any = false;
#pragma unroll
        for (int r = 0; r < VX_G; ++r) {      // rows of the group beyond j1 re-load row j1 - 1 and are not stored
            mk[r] = mask_at(g, i, min(jg + r, j1 - 1));
            any = any || mk[r] == 0;
        }
        T ul[VX_G], wl[VX_G], ur[VX_G], wr[VX_G], um[VX_G], wm[VX_G], un[VX_G], wn[VX_G];
        if (any) {
#pragma unroll
            for (int r = 0; r < VX_G; ++r) {
                const int j = min(jg + r, j1 - 1), jm = clampy(g, j - 1), jn = clampy(g, j + 1);
                ul[r] = at<2>(v, g, 0, il, j); wl[r] = at<2>(v, g, 1, il, j);
                ur[r] = at<2>(v, g, 0, ir, j); wr[r] = at<2>(v, g, 1, ir, j);
                um[r] = at<2>(v, g, 0, i, jm); wm[r] = at<2>(v, g, 1, i, jm);
                un[r] = at<2>(v, g, 0, i, jn); wn[r] = at<2>(v, g, 1, i, jn);
            }
        }
#pragma unroll
        for (int r = 0; r < VX_G; ++r) {
            const int j = jg + r;
            if (j >= j1) continue;
            double c = 0.0;
            uint8_t f = 0;
            if (any && mk[r] == 0) {
                const VxGrad d = vortex_grad(ul[r], wl[r], ur[r], wr[r], um[r], wm[r], un[r], wn[r], (T)limit, two_dx);
                c = vortex_criterion(which, d);
                if (c > threshold) f = d.om >= 0.0 ? 1 : 2;
            }
            const size_t e = (size_t)j * g.X + i;
            if (FIELD) crit[e] = c;
            else flags[e] = f;
        }
    }
}

// one tile of VX_TX x VX_TY cells per workgroup, resolved in LDS; labels: the tile-local root as a global index, -1 without a flag
__global__ __launch_bounds__(256) void k_vortex_local(int X, int Y, VxWhen when, const uint8_t *flags, int *labels)
{
    __shared__ int L[VX_TX * VX_TY];
    __shared__ uint8_t F[VX_TX * VX_TY];
    if (!vortex_on(when)) return;      // (the same in every lane: no barrier is left waiting)
    const int t = threadIdx.x, lx = t % VX_TX, ly = t / VX_TX;
    const int i = blockIdx.x * VX_TX + lx, j = blockIdx.y * VX_TY + ly;
    const bool in = i < X && j < Y;
    const uint8_t f = in ? flags[(size_t)j * X + i] : 0;
    F[t] = f;
    L[t] = t;
    __syncthreads();
    if (f) {
        if (lx > 0 && F[t - 1] == f) uf_union(L, t, t - 1);
        if (ly > 0 && F[t - VX_TX] == f) uf_union(L, t, t - VX_TX);
    }
    __syncthreads();
    if (in) {
        int lab = -1;
        if (f) {
            const int r = uf_find(L, t);
            lab = (blockIdx.y * VX_TY + r / VX_TX) * X + blockIdx.x * VX_TX + r % VX_TX;
        }
        labels[(size_t)j * X + i] = lab;
    }
}

// one lane per pair of cells that face each other over a tile edge: the (ntx - 1) Y pairs over vertical edges, then the (nty - 1) X over horizontal ones
__global__ __launch_bounds__(256) void k_vortex_seam(int X, int Y, VxWhen when, const uint8_t *flags, int *labels)
{
    if (!vortex_on(when)) return;
    const int ntx = (X + VX_TX - 1) / VX_TX, nty = (Y + VX_TY - 1) / VX_TY;
    const long long nv = (long long)(ntx - 1) * Y, nh = (long long)(nty - 1) * X;
    long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    int a, b;
    if (k < nv) {
        const int s = (int)(k / Y), j = (int)(k % Y);
        a = j * X + (s + 1) * VX_TX;
        b = a - 1;
    } else if (k < nv + nh) {
        k -= nv;
        const int s = (int)(k / X), i = (int)(k % X);
        a = (s + 1) * VX_TY * X + i;
        b = a - X;
    } else return;
    const uint8_t f = flags[a];
    if (f && flags[b] == f) uf_union(labels, a, b);
}

// sum of `x` over the 256 lanes of the workgroup -> every lane of wave 0 ... (lane 0 is what the callers use); lds: 4 ints
__device__ __forceinline__ int vortex_block_sum(int x, int *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// every parent -> its root; counts[block]: the roots among the block's VX_BLOCK cells (counts == nullptr: not wanted)
__global__ __launch_bounds__(256) void k_vortex_compress(int n, VxWhen when, int *labels, int *counts)
{
    __shared__ int lds[4];
    if (!vortex_on(when)) return;
    const int base = blockIdx.x * VX_BLOCK + threadIdx.x * 4;
    int roots = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int x = base + c;
        if (x >= n) continue;
        const int p = uf_load(labels + x);
        if (p < 0) continue;
        if (p == x) { ++roots; continue; }
        labels[x] = uf_find(labels, p);      // (another lane may read the old or the new parent: both lie on its chain)
    }
    const int total = vortex_block_sum(roots, lds);
    if (counts && threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup: counts[nb] -> exclusive offsets in place, tmp[0] = the number of roots
__global__ __launch_bounds__(256) void k_vortex_scan(int nb, VxWhen when, int *counts, long long *tmp)
{
    __shared__ int part[256];
    if (!vortex_on(when)) return;
    const int chunk = (nb + 255) / 256, b0 = min(nb, (int)threadIdx.x * chunk), b1 = min(nb, b0 + chunk);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < 256; ++k) { const int x = part[k]; part[k] = run; run += x; }
        tmp[0] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) { const int x = counts[b]; counts[b] = run; run += x; }
}

// ids[root] = its number in ascending label order; table word 14 of every id < maxc: the label
__global__ __launch_bounds__(256) void k_vortex_ids(int n, VxWhen when, int maxc, const int *labels, const int *offsets, int *ids, long long *table)
{
    __shared__ int wsum[4];
    if (!vortex_on(when)) return;
    const int base = blockIdx.x * VX_BLOCK + threadIdx.x * 4, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool root[4];
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        root[c] = base + c < n && labels[base + c] == base + c;
        cnt += root[c];
    }
    int inc = cnt;      // inclusive scan over the wave, then the waves before this one
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int x = __shfl_up(inc, off, 64);
        if (lane >= off) inc += x;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int id = offsets[blockIdx.x] + inc - cnt;
    for (int k = 0; k < w; ++k) id += wsum[k];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (root[c]) {
            ids[base + c] = id;
            if (id < maxc) table[(size_t)14 * maxc + id] = base + c;
            ++id;
        }
}

#ifndef FS_VORTEX_COMBINE
#define FS_VORTEX_COMBINE 1      // (A/B) 0: every lane's own atomics, also where a whole wave lies in one component
#endif
__device__ __forceinline__ long long vx_shfl_down(long long x, int off) { return __shfl_down(x, off, 64); }
__device__ __forceinline__ void vx_add(long long *p, long long x) { atomicAdd((unsigned long long *)p, (unsigned long long)x); }

// one lane per cell; scale = 2^(30 - e)
template <typename T>
__global__ __launch_bounds__(256) void k_vortex_reduce(Grid g, int n, VxWhen when, double dx, double limit, double scale, int maxc, const T *v,
                                                       const uint8_t *flags, const int *labels, const int *ids, long long *table, long long *tmp)
{
    if (!vortex_on(when)) return;
    const int x = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool flagged = x < n && flags[x] != 0;
    int id = -1, i = 0, j = 0;
    long long q = 0;
    bool clip = false;
    if (flagged) {
        i = x % g.X; j = x / g.X;
        const double s = vortex_grad_at(g, v, i, j, (T)limit, 2.0 * dx).om * scale;
        if (s >= (double)VX_QMAX) { q = VX_QMAX; clip = true; }
        else if (s <= -(double)VX_QMAX) { q = -VX_QMAX; clip = true; }
        else if (s != s) { q = 0; clip = true; }
        else q = llrint(s);
        id = ids[labels[x]];
    }
    const bool acc = flagged && id < maxc;
    const unsigned long long mclip = __ballot(clip), mdrop = __ballot(flagged && !acc), macc = __ballot(acc);
    if (lane == 0) {
        if (mclip) vx_add(tmp + 2 + blockIdx.x % VX_SLOTS, __popcll(mclip));
        if (mdrop) vx_add(tmp + 2 + VX_SLOTS + blockIdx.x % VX_SLOTS, __popcll(mdrop));
    }
    if (!macc) return;      // (the same in every lane of the wave)
    const long long aq = q < 0 ? -q : q, xi = 2 * i + 1, yj = 2 * j + 1, tx = aq * xi, ty = aq * yj;
    long long s[9] = {1, q, aq, xi, yj, tx & 0xffffffffll, tx >> 32, ty & 0xffffffffll, ty >> 32};
    long long lo[2] = {i, j}, hi[2] = {i, j};
    unsigned long long peak = ((unsigned long long)aq << 32) | (0xffffffffull - (unsigned)x);
    const int id0 = __shfl(id, __ffsll((long long)macc) - 1, 64);
    if (FS_VORTEX_COMBINE && __all(!acc || id == id0)) {      // one component in the whole wave: combine, then one lane's atomics
        if (!acc) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] = 0;
            lo[0] = lo[1] = 0x7fffffffll; hi[0] = hi[1] = 0; peak = 0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += vx_shfl_down(s[k], off);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const long long a = vx_shfl_down(lo[k], off), b = vx_shfl_down(hi[k], off);
                lo[k] = a < lo[k] ? a : lo[k];
                hi[k] = b > hi[k] ? b : hi[k];
            }
            const unsigned long long p = (unsigned long long)vx_shfl_down((long long)peak, off);
            peak = p > peak ? p : peak;
        }
        if (lane != 0) return;
        id = id0;
    } else if (!acc) return;
    long long *t = table + id;
#pragma unroll
    for (int k = 0; k < 9; ++k) vx_add(t + (size_t)k * maxc, s[k]);
    atomicMin(t + (size_t)9 * maxc, lo[0]);
    atomicMax(t + (size_t)10 * maxc, hi[0]);
    atomicMin(t + (size_t)11 * maxc, lo[1]);
    atomicMax(t + (size_t)12 * maxc, hi[1]);
    atomicMax((unsigned long long *)(t + (size_t)13 * maxc), peak);
}

// one workgroup of 1024: the components of area >= min_area in id order, the first maxv of them into the sample; `words` per sample
__global__ __launch_bounds__(1024) void k_vortex_records(VxWhen when, int maxc, int min_area, int maxv, int words, const uint8_t *flags,
                                                         const long long *table, const long long *tmp, long long *ring)
{
    __shared__ int wsum[16];
    __shared__ long long counters[2];
    if (!vortex_on(when)) return;
    const long long found = tmp[0];
    const int nc = (int)(found < maxc ? found : maxc);
    const int chunk = (nc + 1023) / 1024, c0 = min(nc, (int)threadIdx.x * chunk), c1 = min(nc, c0 + chunk);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cnt = 0;
    for (int c = c0; c < c1; ++c) cnt += table[c] >= min_area;
    int inc = cnt;      // inclusive scan over the wave, then the waves before this one
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int x = __shfl_up(inc, off, 64);
        if (lane >= off) inc += x;
    }
    if (lane == 63) wsum[w] = inc;
    if (w < 2) {      // the spread counters: wave 0 sums the clipped cells, wave 1 the dropped ones
        long long s = 0;
        for (int k = lane; k < VX_SLOTS; k += 64) s += tmp[2 + w * VX_SLOTS + k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += vx_shfl_down(s, off);
        if (lane == 0) counters[w] = s;
    }
    __syncthreads();
    int pos = inc - cnt, passed = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < w) pos += wsum[k];
        passed += wsum[k];
    }
    long long *sample = ring + (size_t)(when.state ? when.state[1] : 0) * words;
    for (int c = c0; c < c1 && pos < maxv; ++c) {
        if (table[c] < min_area) continue;
        long long *r = sample + VX_HEAD + (size_t)pos * VX_REC;
        const long long label = table[(size_t)14 * maxc + c];
        r[0] = label;
#pragma unroll
        for (int k = 0; k < 14; ++k) r[1 + k] = table[(size_t)k * maxc + c];
        r[15] = flags[label];
        ++pos;
    }
    if (threadIdx.x == 0) {
        sample[0] = when.state ? when.state[0] : 0;
        sample[1] = found;
        sample[2] = passed;
        sample[3] = passed < maxv ? passed : maxv;
        sample[4] = counters[0];
        sample[5] = counters[1];
        sample[6] = 0;
        sample[7] = 0;
    }
}

// behind the sequence on the same stream: the launch count; a sampling launch adds a sample, or a lost one when the ring was full
__global__ __launch_bounds__(64) void k_vortex_tick(long long start, long long every, int cap, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) {
        if (state[1] < cap) state[1] = state[1] + 1;
        else state[2] = state[2] + 1;
    }
    state[0] = n + 1;
}

}  // namespace fs
#endif  // __HIPCC__
