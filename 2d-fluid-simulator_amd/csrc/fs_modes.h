// fs_modes.h - harmonic flow modes (new; the reference has none): per-cell Fourier sums of u, w and p at up to MODES_MAX_FREQ frequencies,
// accumulated on the device by a launch that is part of the captured step, so that the amplitude and phase of the shedding
// mode in every cell, or the phase-averaged cycle, need no field download per sample.
//
// State (fs_modes, fs_host.h): with K frequencies and B = 1 + 2K basis entries b = [1, c_1, s_1, ..., c_K, s_K], 3B planes of double over
// the OWNED rows with the pitch and the plane padding of fs_mean.h - plane a * B + j holds the sum over the samples of x_a * b_j for field a
// of (u, w, p); the counters (long long) [0] launches, [1] samples; and the scalars (double): the 2K phasor entries c_1, s_1, ..., then the
// upper triangle of the Gram matrix G[i][j] += b_i * b_j (i <= j, row major).  Launch n samples by samples_at (fs_device.h), as every rider.
// Sample m carries the phasors (c_k, s_k): (1, 0) for m = 0, rotated after every sampling launch by the host's (cd_k, sd_k) = (cos, sin)
// of 2 pi f_k every dt: c' = c cd - s sd, s' = s cd + c sd, every product rounded on its own (-ffp-contract=off).  No sin / cos on the device.
//
// k_modes_accumulate only READS counters and phasors - wave-uniform scalar loads, the same in every workgroup - and the one-lane k_modes_tick
// behind it on the same stream adds to the Gram matrix with the phasors just applied, counts, and rotates: no grid barrier, no atomics, and
// the pair can sit in a hipGraph or a slab tape.  One lane owns a cell and the samples arrive in stream order, so a NumPy f64 loop over
// downloads reproduces every sum bit for bit: j = 0 adds the promoted value as it is, j > 0 adds x * b_j (multiply in double, then add).
//
// A streaming read-modify-write of 3 sizeof(T) + 1 + 16 * 3B bytes per not-wall cell.  The structure is k_mean_accumulate's (W = 2 columns per
// lane and 16-byte plane accesses, W = 1 for odd X; the masks of a row group first, an all-wall group skipped; rows beyond j1 re-load row
// j1 - 1 and are not stored; a wall cell inside a stored pair gets its sums back as loaded) with one difference: 9 - 27 planes do not fit in
// registers the way the mean's 7 do, so a row group is taken in three passes, one per field, each over the B planes of that field with every
// load of the pass issued before its first use; and the group has 4 rows for K <= 2, 2 rows for K >= 3 (B * G * 2 W registers of sums:
// 48, 80, 56, 72).  No instantiation may use scratch (tests/test_build_metadata_modes.py).
#pragma once
#include "fs_mean.h"

namespace fs {

constexpr int MODES_MAX_FREQ = 4;
constexpr int MODES_MAX_B = 1 + 2 * MODES_MAX_FREQ;
constexpr int MODES_STATE = 2;       // device counters (long long): [0] launches, [1] samples
constexpr int modes_basis(int K) { return 1 + 2 * K; }
constexpr int modes_scalars(int K) { return 2 * K + modes_basis(K) * (modes_basis(K) + 1) / 2; }      // phasors, Gram triangle
#ifndef FS_MODES_G_LO
#define FS_MODES_G_LO 4              // rows per load group for K <= 2 (A/B builds)
#endif
#ifndef FS_MODES_G_HI
#define FS_MODES_G_HI 2              // ... and for K >= 3
#endif
constexpr int modes_group(int K) { return K <= 2 ? FS_MODES_G_LO : FS_MODES_G_HI; }
constexpr int modes_rows(int K) { return 2 * modes_group(K); }        // most rows per workgroup: two load groups

struct ModesRot { double cd[MODES_MAX_FREQ], sd[MODES_MAX_FREQ]; };      // kernel argument: constant for the life of the object
struct ModesWeights { double w[3 * MODES_MAX_B]; };

// local rows [jb, je) are the owned rows; a workgroup takes `rpw` of them and 256 W columns.  limit > 0: v owes limit_field(limit)
template <typename T, int W, int K>
__global__ __launch_bounds__(256) void k_modes_accumulate(Grid g, int jb, int je, int rpw, double limit, long long start, long long every,
                                                          const long long *__restrict__ count, const double *__restrict__ scal, const T *v,
                                                          const T *p, double *sums, size_t plane)
{
    if (!samples_at(count[0], start, every)) return;      // (the same in every lane of every workgroup: k_modes_tick writes behind this launch)
    constexpr int B = modes_basis(K), G = modes_group(K);
    double b[B];                                          // wave-uniform: scalar loads, once per workgroup
    b[0] = 1.0;
#pragma unroll
    for (int j = 1; j < B; ++j) b[j] = scal[j - 1];
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using DP = MeanPack<double, W>;
    using MP = MeanPack<uint8_t, W>;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    for (int jg = j0; jg < j1; jg += G) {
        MP mk[G];
        bool any = false;
#pragma unroll
        for (int r = 0; r < G; ++r) {      // rows of the group beyond j1 re-load row j1 - 1 and are not stored
            const int j = min(jg + r, j1 - 1);
            mk[r] = *(const MP *)(g.mask + (size_t)j * g.Pm + i);
#pragma unroll
            for (int c = 0; c < W; ++c) any = any || mk[r].v[c] != 1;
        }
        if (!any) continue;
        TP x[3][G];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const int j = min(jg + r, j1 - 1);
            x[0][r] = *(const TP *)(v + idx<2, T>(g, 0, i, j));
            x[1][r] = *(const TP *)(v + idx<2, T>(g, 1, i, j));
            x[2][r] = *(const TP *)(p + idx<1, T>(g, 0, i, j));
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            DP s[G][B];
#pragma unroll
            for (int r = 0; r < G; ++r) {
                const size_t e = (size_t)(min(jg + r, j1 - 1) - jb) * g.P + i;
#pragma unroll
                for (int k = 0; k < B; ++k) s[r][k] = *(const DP *)(sums + (size_t)(a * B + k) * plane + e);
            }
            if (a == 0 && limit > 0.0) {
#pragma unroll
                for (int r = 0; r < G; ++r)
#pragma unroll
                    for (int c = 0; c < W; ++c)
                        if (mk[r].v[c] != 1) limit_cell(x[0][r].v[c], x[1][r].v[c], (T)limit);
            }
#pragma unroll
            for (int r = 0; r < G; ++r) {
                const int j = jg + r;
                bool row = false;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    if (j >= j1 || mk[r].v[c] == 1) continue;
                    row = true;
                    const double d = (double)x[a][r].v[c];
                    s[r][0].v[c] += d;
#pragma unroll
                    for (int k = 1; k < B; ++k) s[r][k].v[c] += d * b[k];
                }
                if (row) {
                    const size_t e = (size_t)(j - jb) * g.P + i;
#pragma unroll
                    for (int k = 0; k < B; ++k) *(DP *)(sums + (size_t)(a * B + k) * plane + e) = s[r][k];
                }
            }
        }
    }
}

// behind k_modes_accumulate on the same stream.  A sampling launch: the Gram matrix takes the phasors that launch applied, the sample
// count goes up, the phasors rotate - in this order; every launch counts
__global__ __launch_bounds__(64) void k_modes_tick(int nfreq, ModesRot rot, long long start, long long every, long long *count, double *scal)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = count[0];
    if (samples_at(n, start, every)) {
        const int B = 1 + 2 * nfreq;
        double *gram = scal + 2 * nfreq;
        int t = 0;
        for (int i = 0; i < B; ++i) {
            const double bi = i == 0 ? 1.0 : scal[i - 1];
            for (int j = i; j < B; ++j, ++t) {
                const double bj = j == 0 ? 1.0 : scal[j - 1];
                gram[t] = gram[t] + bi * bj;
            }
        }
        count[1] = count[1] + 1;
        for (int k = 0; k < nfreq; ++k) {
            const double c = scal[2 * k], s = scal[2 * k + 1], cd = rot.cd[k], sd = rot.sd[k];
            scal[2 * k] = c * cd - s * sd;
            scal[2 * k + 1] = s * cd + c * sd;
        }
    }
    count[0] = n + 1;
}

// the planes reduced to fields: (T) sum_j wgt[a B + j] * plane[a B + j], j = 0 .. B - 1 in this order from 0.0, product then add in double,
// for a = u, w into the 2-channel vo and a = p into the 1-channel po on the not-wall cells of the owned rows; 0 on the wall cells.  With the
// right weights: the fitted mean, a cos / sin coefficient field, or the phase-averaged flow at a phase (fs/modes.py reconstruct_weights).
// Raises vo's flag like every kernel that writes a velocity.
template <typename T, int W>
__global__ __launch_bounds__(256) void k_modes_combine(Grid g, int jb, int je, int rpw, int B, ModesWeights wgt, const double *sums, size_t plane,
                                                       T *vo, T *po, unsigned *hot)
{
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= g.X) return;
    using TP = MeanPack<T, W>;
    using DP = MeanPack<double, W>;
    using MP = MeanPack<uint8_t, W>;
    const int j0 = jb + blockIdx.y * rpw;
    const int j1 = j0 + rpw < je ? j0 + rpw : je;
    for (int j = j0; j < j1; ++j) {
        const MP mk = *(const MP *)(g.mask + (size_t)j * g.Pm + i);
        const size_t e = (size_t)(j - jb) * g.P + i;
        DP acc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < W; ++c) acc[a].v[c] = 0.0;
            for (int k = 0; k < B; ++k) {
                const DP s = *(const DP *)(sums + (size_t)(a * B + k) * plane + e);
                const double wk = wgt.w[a * B + k];
#pragma unroll
                for (int c = 0; c < W; ++c) acc[a].v[c] += wk * s.v[c];
            }
        }
        TP u, w, q;
        bool h = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const bool wall = mk.v[c] == 1;
            u.v[c] = wall ? (T)0 : (T)acc[0].v[c];
            w.v[c] = wall ? (T)0 : (T)acc[1].v[c];
            q.v[c] = wall ? (T)0 : (T)acc[2].v[c];
            h = h || hot2(u.v[c], w.v[c]);
        }
        *(TP *)(vo + idx<2, T>(g, 0, i, j)) = u;
        *(TP *)(vo + idx<2, T>(g, 1, i, j)) = w;
        *(TP *)(po + idx<1, T>(g, 0, i, j)) = q;
        raise_hot(hot, h);
    }
}

}  // namespace fs
