// fs_mean.h - time averages of the flow (new; the reference has none): first and second moments of u, w and p accumulated on the device by a
// launch that is part of the captured step, so that a mean wake or the Reynolds stresses of a long run need no field download per sample.
//
// State (fs_mean, fs_host.h): MEAN_PLANES planes of double over the OWNED rows of the context, pitch P like a 1-channel field (element
// (i, j) of plane s at s * plane + (j - first owned row) * P + i): S_u, S_w, S_p, S_uu, S_ww, S_uw, S_pp; and device counters (long long):
// [0] launches since creation, [1] samples accumulated.  Launch n (from 0) samples when n + 1 > start and (n + 1 - start) % every == 0.
// k_mean_accumulate only READS the counters - every workgroup takes the decision from the same value - and the one-lane k_mean_tick
// behind it on the same stream advances them: no grid barrier, no atomics, and the pair can sit in a hipGraph or a slab tape.
//
// Per sampled not-wall cell (mask != 1): the stored u, w (through limit_cell when v still owes a deferred limit_field) and p are promoted to
// double, multiplied in double and added in double (-ffp-contract=off: no FMA).  One lane owns a cell and the samples arrive in stream
// order, so a NumPy f64 loop over downloads reproduces every sum bit for bit, in f32 and in f64 runs.
//
// A streaming read-modify-write: 3 sizeof(T) + 1 bytes in and 7 x 16 bytes of accumulator traffic per cell.  A lane takes W = 2 adjacent
// columns (X even: every `res`; the planes move as 16-byte accesses, the pitch of 64 elements keeps every row aligned; odd X takes the
// scalar instantiation W = 1) and marches down `rpw` rows in groups of MEAN_G: the masks of a group first, then - unless all of the
// lane's cells in the group are wall - every load of the group before the first use, then the arithmetic and the stores.  A third of scene
// 5 is solid: those lanes move the mask bytes only.  bc5 res 4096 f32: 629 us per sampling launch, 0.80 of the GPU's copy rate; tile
// shapes of 1 - 8 rows per group and 2 - 64 rows per workgroup measured within the run-to-run spread of each other.  A wall cell inside a pair that is accumulated gets its own sums stored back as
// loaded (they are 0 unless fs_mean_write put something else there).
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int MEAN_PLANES = 7;      // S_u, S_w, S_p, S_uu, S_ww, S_uw, S_pp
constexpr int MEAN_STATE = 2;       // device counters (long long): [0] launches, [1] samples
#ifndef FS_MEAN_G
#define FS_MEAN_G 4                 // rows per load group (A/B builds)
#endif
constexpr int MEAN_G = FS_MEAN_G;
#ifndef FS_MEAN_ROWS
#define FS_MEAN_ROWS 8
#endif
constexpr int MEAN_ROWS = FS_MEAN_ROWS;      // most rows per workgroup (fs_mean_accumulate takes fewer on small grids)

#ifndef FS_MEAN_PAD
#define FS_MEAN_PAD 544
#endif
// doubles between two planes beyond the rows: at res 4096 a plane is exactly 2^28 bytes, and seven streams at the same offset of equally
// aligned planes would meet in the same memory channel at the same time; 4 KiB + 256 B staggers them
constexpr size_t MEAN_PAD = FS_MEAN_PAD;

template <typename S, int W>
struct alignas(sizeof(S) * W) MeanPack { S v[W]; };

// local rows [jb, je) are the owned rows; a workgroup takes `rpw` of them and 256 W columns.  limit > 0: v owes limit_field(limit)
template <typename T, int W>
__global__ __launch_bounds__(256) void k_mean_accumulate(Grid g, int jb, int je, int rpw, double limit, long long start, long long every,
                                                         const long long *state, const T *v, const T *p, double *sums, size_t plane)
{
    if (!samples_at(state[0], start, every)) return;      // (the same in every lane of every workgroup: k_mean_tick writes behind this launch)
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using DP = MeanPack<double, W>;
    using MP = MeanPack<uint8_t, W>;
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
        if (!any) continue;
        TP u[MEAN_G], w[MEAN_G], q[MEAN_G];
        DP s[MEAN_G][MEAN_PLANES];
#pragma unroll
        for (int r = 0; r < MEAN_G; ++r) {
            const int j = min(jg + r, j1 - 1);
            u[r] = *(const TP *)(v + idx<2, T>(g, 0, i, j));
            w[r] = *(const TP *)(v + idx<2, T>(g, 1, i, j));
            q[r] = *(const TP *)(p + idx<1, T>(g, 0, i, j));
            const size_t e = (size_t)(j - jb) * g.P + i;
#pragma unroll
            for (int k = 0; k < MEAN_PLANES; ++k) s[r][k] = *(const DP *)(sums + k * plane + e);
        }
#pragma unroll
        for (int r = 0; r < MEAN_G; ++r) {
            const int j = jg + r;
            bool row = false;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (j >= j1 || mk[r].v[c] == 1) continue;
                row = true;
                T uc = u[r].v[c], wc = w[r].v[c];
                if (limit > 0.0) limit_cell(uc, wc, (T)limit);
                const double du = (double)uc, dw = (double)wc, dq = (double)q[r].v[c];
                s[r][0].v[c] += du;
                s[r][1].v[c] += dw;
                s[r][2].v[c] += dq;
                s[r][3].v[c] += du * du;
                s[r][4].v[c] += dw * dw;
                s[r][5].v[c] += du * dw;
                s[r][6].v[c] += dq * dq;
            }
            if (row) {
                const size_t e = (size_t)(j - jb) * g.P + i;
#pragma unroll
                for (int k = 0; k < MEAN_PLANES; ++k) *(DP *)(sums + k * plane + e) = s[r][k];
            }
        }
    }
}

// behind k_mean_accumulate on the same stream: the launch count, and the sample count when that launch sampled
__global__ __launch_bounds__(64) void k_mean_tick(long long start, long long every, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) state[1] = state[1] + 1;
    state[0] = n + 1;
}

// the means as fields: (T)(S_u / n), (T)(S_w / n) into the 2-channel vo and (T)(S_p / n) into the 1-channel po on the not-wall cells of
// the owned rows, 0 on the wall cells; n = state[1] (the host refuses n == 0).  Raises vo's flag like every kernel that writes a velocity.
template <typename T, int W>
__global__ __launch_bounds__(256) void k_mean_finalize(Grid g, int jb, int je, int rpw, const long long *state, const double *sums, size_t plane,
                                                       T *vo, T *po, unsigned *hot)
{
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using DP = MeanPack<double, W>;
    using MP = MeanPack<uint8_t, W>;
    const double n = (double)state[1];
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    for (int j = j0; j < j1; ++j) {
        const MP mk = *(const MP *)(g.mask + (size_t)j * g.Pm + i);
        const size_t e = (size_t)(j - jb) * g.P + i;
        const DP su = *(const DP *)(sums + e), sw = *(const DP *)(sums + plane + e), sp = *(const DP *)(sums + 2 * plane + e);
        TP u, w, q;
        bool h = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const bool wall = mk.v[c] == 1;
            u.v[c] = wall ? (T)0 : (T)(su.v[c] / n);
            w.v[c] = wall ? (T)0 : (T)(sw.v[c] / n);
            q.v[c] = wall ? (T)0 : (T)(sp.v[c] / n);
            h = h || hot2(u.v[c], w.v[c]);
        }
        *(TP *)(vo + idx<2, T>(g, 0, i, j)) = u;
        *(TP *)(vo + idx<2, T>(g, 1, i, j)) = w;
        *(TP *)(po + idx<1, T>(g, 0, i, j)) = q;
        raise_hot(hot, h);
    }
}

}  // namespace fs
