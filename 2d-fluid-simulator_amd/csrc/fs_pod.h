// fs_pod.h - snapshot POD (new; the reference has none): the last M sampled flow fields kept resident on the device by a launch that is part
// of the captured step, the M x M Gram matrix of those snapshots reduced on the device, and linear combinations of them written back as
// fields.  The host sees the Gram matrix alone: eigenvectors, energies and mode weights are M x M algebra (fs/pod.py).
//
// State (fs_pod, fs_host.h): M slots (2 <= M <= POD_MAX), each three planes of the FIELD type T - u, w, p - over the OWNED rows with the pitch
// P of a 1-channel field and the plane padding of fs_mean.h: element (i, j) of plane c of slot s at ((s * 3 + c) * plane + (j - first owned
// row) * P + i, plane = nyl * P + MEAN_PAD.  12 bytes per cell and slot in f32, 24 in f64; zeroed at creation.  Counters (long long):
// [0] launches, [1] samples.
//
// k_pod_capture: launch n samples by samples_at (fs_device.h), as every rider, into slot samples % M - a ring that always holds the last
// min(samples, M) samples.  Not-wall cells (mask != 1) take u, w (through limit_cell when v still owes a deferred limit_field) and p as
// stored; wall cells take +0; pad columns are never written.  The kernel only READS the counters - the one-lane k_pod_tick behind it on the
// same stream advances them: no grid barrier, no atomics, and the pair can sit in a hipGraph.  The structure is k_mean_accumulate's: W = 2
// columns per lane for even X (16-byte accesses in f64, 8-byte in f32), W = 1 for odd X; the masks of a group of MEAN_G rows first, then -
// unless every cell of the lane in the group is wall, which stores zeros without reading the flow - every load of the group before the
// first use; rows of a group beyond the workgroup's range re-load its last row and are not stored.  3 sizeof(T) + 1 bytes in and
// 3 sizeof(T) out per not-wall cell: 25 B in f32.
//
// k_pod_gram - for the n = min(samples, M) resident slots, G[a][b] = sum over the owned rows j and the columns i < X of
//     t = (double)u_a * (double)u_b;  t = t + (double)w_a * (double)w_b
// every product and sum rounded on its own (-ffp-contract=off).  Wall cells hold zeros: the kernel reads no mask.  THE GEOMETRY, which fixes
// the order of every sum and is the specification a restatement has to follow to reproduce the bits:
//   * the slots are cut into tiles of POD_T = 8; a workgroup of 256 lanes takes one pair of tiles (ta <= tb), 256 columns (one per lane) and
//     `rpw` rows (POD_GRAM_G = 4 doubled up to POD_GRAM_ROWS = 64 while the grid keeps its workgroups, fs_launch.h diag_rows), and holds the
//     POD_T x POD_T sums of its pairs in registers (a diagonal tile: the 36 with a <= b);
//   * a lane adds the t of its column to each sum row after row, j ascending, from 0.0; a lane beyond X holds 0.0;
//   * the 256 lanes of the workgroup combine as block_stats (fs_stats.h) does: within a wave by __shfl_down over 32, 16, ..., 1, then lane 0
//     adds the four waves' values in wave order; the workgroup writes its sums as one partial each, block = blockIdx.y * gridDim.x + blockIdx.x;
//   * k_pod_gram_final, one workgroup of 256 per sum: lane l folds the partials of blocks l, l + 256, ... in this order from 0.0, and the
//     lanes combine by the same tree (the order of k_flow_stats_final).  G[b][a] is a copy of G[a][b].
// A slot index beyond n - 1 inside the last tile reads slot n - 1 instead; its sums are never written out.  The tile pairs are spread over
// blockIdx.z in two launches: the diagonal tiles (z = tile), then the pairs ta < tb row by row (pod_offdiag).  Every snapshot is read once
// per tile pair its tile belongs to - the diagonal one and nt - 1 others: nt = ceil(n / 8) times, 8 times the resident u and w planes at
// M = 64 - against n (n + 1) multiplications and as many additions in double per cell (a diagonal tile forms a <= b only).
//
// k_pod_combine: vo, po = (T) sum_m wgt[m] * slot_m, m = 0 .. M - 1 in this order from 0.0, product then add in double, for u, w into the
// 2-channel vo and p into the 1-channel po; 0 on wall cells; raises vo's flag like every kernel that writes a velocity.
//
// No instantiation may use scratch (tests/test_build_metadata_pod.py).
#pragma once
#include "fs_mean.h"

namespace fs {

constexpr int POD_MAX = 64;            // most slots of an object (FS_POD_MAX)
constexpr int POD_STATE = 2;           // device counters (long long): [0] launches, [1] samples
constexpr int POD_T = 8;               // slots per tile of the Gram kernel: POD_T x POD_T sums of double per lane
constexpr int POD_GRAM_G = 4;          // rows per workgroup of the Gram kernel: from this ...
constexpr int POD_GRAM_ROWS = 64;      // ... up to this
constexpr int POD_TT = POD_T * POD_T;

struct PodWeights { double w[POD_MAX]; };      // kernel argument

// local rows [jb, je) are the owned rows; a workgroup takes `rpw` of them and 256 W columns.  limit > 0: v owes limit_field(limit)
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pod_capture(Grid g, int jb, int je, int rpw, double limit, long long start, long long every, int M,
                                                     const long long *state, const T *v, const T *p, T *slots, size_t plane)
{
    if (!samples_at(state[0], start, every)) return;      // (the same in every lane of every workgroup: k_pod_tick writes behind this launch)
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using MP = MeanPack<uint8_t, W>;
    T *slot = slots + (size_t)(state[1] % M) * 3 * plane;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    for (int jg = j0; jg < j1; jg += MEAN_G) {
        MP mk[MEAN_G];
        bool any = false;
#pragma unroll
        for (int r = 0; r < MEAN_G; ++r) {      // rows of the group beyond j1 re-load row j1 - 1 and are not stored
            const int j = min(jg + r, j1 - 1);
            mk[r] = *(const MP *)(g.mask + (size_t)j * g.Pm + i);
#pragma unroll
            for (int c = 0; c < W; ++c) any = any || mk[r].v[c] != 1;
        }
        TP u[MEAN_G], w[MEAN_G], q[MEAN_G];
        if (any) {
#pragma unroll
            for (int r = 0; r < MEAN_G; ++r) {
                const int j = min(jg + r, j1 - 1);
                u[r] = *(const TP *)(v + idx<2, T>(g, 0, i, j));
                w[r] = *(const TP *)(v + idx<2, T>(g, 1, i, j));
                q[r] = *(const TP *)(p + idx<1, T>(g, 0, i, j));
            }
        }
#pragma unroll
        for (int r = 0; r < MEAN_G; ++r) {
            const int j = jg + r;
            if (j >= j1) continue;
            TP ou, ow, oq;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                ou.v[c] = (T)0; ow.v[c] = (T)0; oq.v[c] = (T)0;
                if (!any || mk[r].v[c] == 1) continue;
                T uc = u[r].v[c], wc = w[r].v[c];
                if (limit > 0.0) limit_cell(uc, wc, (T)limit);
                ou.v[c] = uc; ow.v[c] = wc; oq.v[c] = q[r].v[c];
            }
            const size_t e = (size_t)(j - jb) * g.P + i;
            *(TP *)(slot + e) = ou;
            *(TP *)(slot + plane + e) = ow;
            *(TP *)(slot + 2 * plane + e) = oq;
        }
    }
}

// behind k_pod_capture on the same stream: the launch count, and the sample count when that launch sampled
__global__ __launch_bounds__(64) void k_pod_tick(long long start, long long every, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) state[1] = state[1] + 1;
    state[0] = n + 1;
}

// N sums of a workgroup combined in the tree of block_stats (fs_stats.h): lanes by shuffles, then the waves in LDS in wave order; the
// result is in lane 0.  lds: N doubles per wave
template <int N>
__device__ __forceinline__ void pod_block_sum(double (&a)[N], double *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int s = 0; s < N; ++s) a[s] = a[s] + __shfl_down(a[s], off, 64);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int s = 0; s < N; ++s) lds[N * w + s] = a[s];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < N; ++s) a[s] = lds[s];
        for (int k = 1; k < nw; ++k)
#pragma unroll
            for (int s = 0; s < N; ++s) a[s] = a[s] + lds[N * k + s];
    }
}

// pair z of the tile pairs ta < tb of nt tiles, row by row: (0, 1), (0, 2), ..., (0, nt - 1), (1, 2), ...
__host__ __device__ inline void pod_offdiag(int z, int nt, int &ta, int &tb)
{
    ta = 0;
    while (z >= nt - 1 - ta) { z -= nt - 1 - ta; ++ta; }
    tb = ta + 1 + z;
}

// DIAG: blockIdx.z is the tile ta = tb and only the sums a <= b are formed; otherwise pair blockIdx.z of pod_offdiag.  partial:
// [pair][POD_TT][nblocks], the pairs counted from pair0 (the diagonal tiles first, the others behind them)
template <typename T, bool DIAG>
__global__ __launch_bounds__(256) void k_pod_gram(int X, int P, int jb, int je, int rpw, int n, int nt, int pair0, const T *slots, size_t plane,
                                                  double *partial)
{
    __shared__ double lds[4 * POD_TT];
    int ta = blockIdx.z, tb = blockIdx.z;
    if (!DIAG) pod_offdiag((int)blockIdx.z, nt, ta, tb);
    double acc[POD_TT];
#pragma unroll
    for (int s = 0; s < POD_TT; ++s) acc[s] = 0.0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    if (i < X) {
        const T *pa[POD_T], *pb[POD_T];
#pragma unroll
        for (int k = 0; k < POD_T; ++k) {      // slots beyond n - 1: slot n - 1 again (never written out)
            pa[k] = slots + (size_t)min(ta * POD_T + k, n - 1) * 3 * plane + i;
            pb[k] = slots + (size_t)min(tb * POD_T + k, n - 1) * 3 * plane + i;
        }
        for (int j = j0; j < j1; ++j) {
            const size_t e = (size_t)(j - jb) * P;
            T ua[POD_T], wa[POD_T], ub[POD_T], wb[POD_T];
#pragma unroll
            for (int k = 0; k < POD_T; ++k) {      // every load of the row before the first use
                ua[k] = pa[k][e];
                wa[k] = pa[k][plane + e];
                if (!DIAG) { ub[k] = pb[k][e]; wb[k] = pb[k][plane + e]; }
            }
#pragma unroll
            for (int a = 0; a < POD_T; ++a)
#pragma unroll
                for (int b = DIAG ? a : 0; b < POD_T; ++b) {
                    double t = (double)ua[a] * (double)(DIAG ? ua[b] : ub[b]);
                    t = t + (double)wa[a] * (double)(DIAG ? wa[b] : wb[b]);
                    acc[a * POD_T + b] = acc[a * POD_T + b] + t;
                }
        }
    }
    pod_block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        double *out = partial + (size_t)(pair0 + blockIdx.z) * POD_TT * nb;
#pragma unroll
        for (int a = 0; a < POD_T; ++a)
#pragma unroll
            for (int b = DIAG ? a : 0; b < POD_T; ++b) out[(size_t)(a * POD_T + b) * nb + blk] = acc[a * POD_T + b];
    }
}

// one workgroup per sum: blockIdx.x = pair * POD_TT + a * POD_T + b in the layout of k_pod_gram's partials -> G[a][b] and G[b][a] of the
// dense n x n matrix `out`; sums the first stage did not form or that lie beyond n are left alone
__global__ __launch_bounds__(256) void k_pod_gram_final(const double *partial, int nblocks, int n, int nt, double *out)
{
    __shared__ double lds[4];
    const int pair = blockIdx.x / POD_TT, ia = blockIdx.x % POD_TT / POD_T, ib = blockIdx.x % POD_T;
    int ta = pair, tb = pair;
    if (pair >= nt) pod_offdiag(pair - nt, nt, ta, tb);
    const int a = ta * POD_T + ia, b = tb * POD_T + ib;
    if (a > b || b >= n) return;      // (the same in every lane)
    double s[1] = {0.0};
    const double *src = partial + (size_t)blockIdx.x * nblocks;
    for (int k = threadIdx.x; k < nblocks; k += blockDim.x) s[0] = s[0] + src[k];
    pod_block_sum(s, lds);
    if (threadIdx.x == 0) {
        out[(size_t)a * n + b] = s[0];
        out[(size_t)b * n + a] = s[0];
    }
}

// local rows [jb, je) are the owned rows; a workgroup takes `rpw` of them and 256 W columns
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pod_combine(Grid g, int jb, int je, int rpw, int M, PodWeights wgt, const T *slots, size_t plane, T *vo,
                                                     T *po, unsigned *hot)
{
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using MP = MeanPack<uint8_t, W>;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    for (int j = j0; j < j1; ++j) {
        const MP mk = *(const MP *)(g.mask + (size_t)j * g.Pm + i);
        const size_t e = (size_t)(j - jb) * g.P + i;
        double acc[3][W];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < W; ++c) acc[a][c] = 0.0;
        for (int m = 0; m < M; ++m) {
            const T *slot = slots + (size_t)m * 3 * plane + e;
            const TP su = *(const TP *)slot, sw = *(const TP *)(slot + plane), sq = *(const TP *)(slot + 2 * plane);
            const double wm = wgt.w[m];
#pragma unroll
            for (int c = 0; c < W; ++c) {
                acc[0][c] += wm * (double)su.v[c];
                acc[1][c] += wm * (double)sw.v[c];
                acc[2][c] += wm * (double)sq.v[c];
            }
        }
        TP u, w, q;
        bool h = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const bool wall = mk.v[c] == 1;
            u.v[c] = wall ? (T)0 : (T)acc[0][c];
            w.v[c] = wall ? (T)0 : (T)acc[1][c];
            q.v[c] = wall ? (T)0 : (T)acc[2][c];
            h = h || hot2(u.v[c], w.v[c]);
        }
        *(TP *)(vo + idx<2, T>(g, 0, i, j)) = u;
        *(TP *)(vo + idx<2, T>(g, 1, i, j)) = w;
        *(TP *)(po + idx<1, T>(g, 0, i, j)) = q;
        raise_hot(hot, h);
    }
}

}  // namespace fs
