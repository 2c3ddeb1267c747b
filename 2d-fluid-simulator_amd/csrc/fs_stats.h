// fs_stats.h - flow diagnostics (new; the reference has none): one pass over v, p and the mask of the owned rows that reduces to the
// FS_FLOW_NSTAT slots of include/fs_hip.h (energy, enstrophy, divergence, maxima, non-finite count, pressure force on a body box).
//
// Two deterministic stages, no atomics, like the residual (fs_kernels.h k_residual): a workgroup owns up to STATS_ROWS rows x 256 columns and
// writes ONE partial vector; a single workgroup then combines the partials in a fixed tree order.  Each lane marches down its column and
// keeps rows j-1, j, j+1 of u, w and p in registers, so every row of HBM is read once (13 B per cell in f32: 2 velocity planes, p, mask);
// the i+-1 neighbours are the adjacent lanes' cache lines.  Neighbour indices are clamped at the domain edge like
// fs/differentiation.py:4-9 sample(); on a slab row j+-1 of an owned edge row is a ghost row (the caller exchanges v and p to depth 1).
// All arithmetic is double, on the stored values promoted to double, in the order the header states (a NumPy f64 restatement reproduces
// every per-cell term bit for bit).  Maxima propagate NaN: `b > a || b != b`, never fmax.
#pragma once
#include "fs_device.h"

namespace fs {

constexpr int STATS_N = 10;          // FS_FLOW_NSTAT
constexpr int STATS_G = 4;           // rows per load group
constexpr int STATS_ROWS = 32;       // most rows per workgroup (2 extra rows of u, w, p per 32: 6 % re-read); small grids take fewer, down to
                                     // STATS_G, so that the grid keeps enough workgroups in flight (fs_flow_stats)
__device__ __forceinline__ constexpr bool stat_is_max(int s) { return s >= 4 && s <= 6; }
__device__ __forceinline__ double stat_max(double a, double b) { return (b > a || b != b) ? b : a; }

// the 10 slots of a workgroup / of the whole grid, combined in a fixed tree: lanes by shuffles, then the waves in LDS in wave order
__device__ __forceinline__ void block_stats(double (&a)[STATS_N], double *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) {
            const double b = __shfl_down(a[s], off, 64);
            a[s] = stat_is_max(s) ? stat_max(a[s], b) : a[s] + b;
        }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) lds[STATS_N * w + s] = a[s];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) a[s] = lds[s];
        for (int k = 1; k < nw; ++k)
#pragma unroll
            for (int s = 0; s < STATS_N; ++s) a[s] = stat_is_max(s) ? stat_max(a[s], lds[STATS_N * k + s]) : a[s] + lds[STATS_N * k + s];
    }
}

__device__ __forceinline__ bool nonfinite(double x) { return !(fabs(x) < __builtin_huge_val()); }   // NaN or +-Inf

// box: body box [bx0, bx1) x [by0, by1) in global cells (empty: no force).  Local rows [jb, je) are the owned rows; a workgroup takes `rpw`
// of them (a multiple of STATS_G).  The loads of a group of STATS_G rows are issued together before any of them is used (one memory
// round trip per group instead of two per row: the neighbours of a fluid cell are not loaded behind a branch on its mask).  Rows of a group
// beyond the workgroup's range re-load its last rows (j1 - 1, and j1 for the row above) and are not evaluated: every row read lies in
// [j0 - 1, j1], inside the allocation on a slab (halo >= 1) and clamped to the domain on one GPU.  partial: slot-major, [STATS_N][nblocks].
template <typename T>
__global__ __launch_bounds__(256) void k_flow_stats(Grid g, int jb, int je, int rpw, double dx, int bx0, int by0, int bx1, int by1, const T *v,
                                                    const T *p, double *partial)
{
    __shared__ double lds[4 * STATS_N];
    double a[STATS_N];
#pragma unroll
    for (int s = 0; s < STATS_N; ++s) a[s] = 0.0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    if (i < g.X) {
        const int il = clampx(g, i - 1), ir = clampx(g, i + 1);
        const double two_dx = 2.0 * dx;
        const bool in_x = bx0 <= i && i < bx1;
        const int jm = clampy(g, j0 - 1);
        T um = at<2>(v, g, 0, i, jm), wm = at<2>(v, g, 1, i, jm), pm = at<1>(p, g, 0, i, jm);      // row j - 1
        T uc = at<2>(v, g, 0, i, j0), wc = at<2>(v, g, 1, i, j0), pc = at<1>(p, g, 0, i, j0);      // row j
        for (int jg = j0; jg < j1; jg += STATS_G) {
            T un[STATS_G], wn[STATS_G], pn[STATS_G], ul[STATS_G], ur[STATS_G], wl[STATS_G], wr[STATS_G];
            uint8_t mk[STATS_G];
#pragma unroll
            for (int r = 0; r < STATS_G; ++r) {
                // clamped to the domain edge first, then to the workgroup's rows plus the one row below / above them: a row of the
                // group beyond j1 is never evaluated, and on a slab the rows past j1 + 1 may lie beyond the allocation (halo 2 or 3)
                const int jn = min(clampy(g, jg + r + 1), j1), jr = min(clampy(g, jg + r), j1 - 1);
                un[r] = at<2>(v, g, 0, i, jn); wn[r] = at<2>(v, g, 1, i, jn); pn[r] = at<1>(p, g, 0, i, jn);
                ul[r] = at<2>(v, g, 0, il, jr); ur[r] = at<2>(v, g, 0, ir, jr);
                wl[r] = at<2>(v, g, 1, il, jr); wr[r] = at<2>(v, g, 1, ir, jr);
                mk[r] = mask_at(g, i, jr);
            }
#pragma unroll
            for (int r = 0; r < STATS_G; ++r) {
                const int j = jg + r;
                if (j < j1) {
                    const double u = (double)uc, w = (double)wc;
                    if (mk[r] == 0) {
                        const double s2 = u * u + w * w;
                        const double om = (((double)wr[r] - (double)wl[r]) - ((double)un[r] - (double)um)) / two_dx;
                        const double dv = (((double)ur[r] - (double)ul[r]) + ((double)wn[r] - (double)wm)) / two_dx;
                        const double av = fabs(u) + fabs(w);
                        a[0] += 1.0;
                        a[1] += s2;
                        a[2] += om * om;
                        a[3] += dv * dv;
                        a[4] = stat_max(a[4], s2);
                        a[5] = stat_max(a[5], av);
                        a[6] = stat_max(a[6], fabs(dv));
                    }
                    if (mk[r] != 1) {
                        if (nonfinite(u) || nonfinite(w) || nonfinite((double)pc)) a[7] += 1.0;
                    } else if (in_x) {
                        const int gy = g.ybase + j;
                        if (by0 <= gy && gy < by1) {
                            // the pressure of each fluid neighbour pushes on this wall cell; neighbours beyond the domain edge do not exist
                            // (rows outside the domain hold mask 1, and j +- 1 of an owned row is a local row whenever it lies inside)
                            if (i + 1 < g.X && mask_at(g, i + 1, j) == 0) a[8] -= (double)at<1>(p, g, 0, i + 1, j) * dx;
                            if (i > 0 && mask_at(g, i - 1, j) == 0) a[8] += (double)at<1>(p, g, 0, i - 1, j) * dx;
                            if (j < g.jhi && mask_at(g, i, j + 1) == 0) a[9] -= (double)pn[r] * dx;
                            if (j > g.jlo && mask_at(g, i, j - 1) == 0) a[9] += (double)pm * dx;
                        }
                    }
                }
                um = uc; wm = wc; pm = pc;
                uc = un[r]; wc = wn[r]; pc = pn[r];
            }
        }
    }
    block_stats(a, lds);
    if (threadIdx.x == 0) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) partial[s * nb + b] = a[s];
    }
}

// partial[STATS_N][nblocks] -> out[STATS_N]; every thread folds its blocks b = tid, tid + 256, ... in order, then the tree of block_stats
__global__ __launch_bounds__(256) void k_flow_stats_final(const double *partial, int nblocks, double *out)
{
    __shared__ double lds[4 * STATS_N];
    double a[STATS_N];
#pragma unroll
    for (int s = 0; s < STATS_N; ++s) a[s] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) a[s] = stat_is_max(s) ? stat_max(a[s], partial[(size_t)s * nblocks + b]) : a[s] + partial[(size_t)s * nblocks + b];
    block_stats(a, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int s = 0; s < STATS_N; ++s) out[s] = a[s];
}

}  // namespace fs
