// fs_loads.h - surface loads on a body (new; the reference has none): per sampling step the pressure and the viscous force on the body's faces,
// their moments about a centre, and running first and second moments of the per-face pressure and wall shear - what Cp, Cf, drag, lift and
// torque are made of.  Rides the step like fs_history.h: the counters live on the device, so the launches can be captured into a hipGraph or
// recorded into a slab tape and replayed; the host drains the ring of records between replays (fs_loads_read).
//
// A face (LoadFace, 32 bytes) is the fluid cell's element offsets, the direction wall -> fluid and the lever arm of the face midpoint about
// the centre in CELL units (formed on the host in double; the kernel multiplies by dx, one IEEE operation, so ax = (xm - cx) * dx is what a
// host loop gets).  One lane per face: it gathers u, w and p of its fluid cell, adds pk, pk pk, tk, tk tk to the face's four sums (planes of
// `stride` doubles: S_p, S_pp, S_t, S_tt; nobody else touches them - no atomics) and forms the six terms of the record
// [Fpx, Fpy, Fvx, Fvy, Mp, Mv].  Every operation is one double operation in the order include/fs_hip.h states (the build has
// -ffp-contract=off).  Wall shear: tk = (inv_re ut) / dx with ut the tangential velocity of the fluid cell - the no-slip point is the centre
// of the wall cell, one dx away, which is the distance the solver's own Laplacian uses.
//
// Reduction, fixed order, no atomics: the 64 lanes of a wave fold by shuffles, lane 0 of the workgroup adds the waves in order
// (block_sum6, the tree of fs_kernels.h block_sum2), and k_loads_record folds the workgroups' partials - lane t takes t, t + 256, ... in
// order - through the same tree.  Repeated launches on the same state give identical bits.
//
// Two forms.  Up to LOADS_SPLIT faces ONE launch of one workgroup does everything (k_loads_one: each lane walks tid, tid + 256): at
// 512 faces that is two dependent gathers per lane, the point up to which fs_history.h found a single workgroup no slower than a second
// launch (HIST_SPLIT).  Longer lists (scenes 3 and 5 at res 4096: 35 - 42 k faces) take k_loads_faces over ceil(nf / 256) workgroups and then
// the one-workgroup k_loads_record.  A launch that does not sample reads the counters and returns; k_loads_record / k_loads_one advance
// them by one lane behind a barrier.
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int LOADS_WG = 256;            // lanes per workgroup, faces per workgroup of the split form
constexpr int LOADS_SPLIT = 512;         // faces up to which one workgroup does the whole launch (2 rounds of gathers per lane)
constexpr int LOADS_REC = 6;             // doubles per record: Fpx, Fpy, Fvx, Fvy, Mp, Mv
constexpr int LOADS_SUMS = 4;            // per-face planes: S_p, S_pp, S_t, S_tt
constexpr int LOADS_STATE = 4;           // device counters (long long): [0] launches, [1] samples, [2] records in the ring, [3] records dropped

struct LoadFace { unsigned u, w, p; int dir; double rx, ry; };      // element offsets of the fluid cell; midpoint - centre in cell units
static_assert(sizeof(LoadFace) == 32, "LoadFace is the 32-byte face record of the byte model");

// one face on a sampling launch: the four sums of face k, and the six terms added to t[]
template <typename T>
__device__ __forceinline__ void loads_face(const T *v, const T *p, const LoadFace f, int k, size_t stride, double dx, double inv_re, double limit,
                                           double *sums, double (&t)[LOADS_REC])
{
    const double pk = (double)p[f.p];
    T u = v[f.u], w = v[f.w];
    if (limit > 0.0) limit_cell(u, w, (T)limit);
    const bool xdir = f.dir < 2;                      // the wall's normal is along x: the tangent is y
    const double ut = xdir ? (double)w : (double)u;
    const double tv = inv_re * ut;
    const double tk = tv / dx;
    sums[k] += pk;
    sums[stride + k] += pk * pk;
    sums[2 * stride + k] += tk;
    sums[3 * stride + k] += tk * tk;
    const double tp = pk * dx;
    double fpx = 0.0, fpy = 0.0;
    if (f.dir == 0) fpx = -tp;
    else if (f.dir == 1) fpx = tp;
    else if (f.dir == 2) fpy = -tp;
    else fpy = tp;
    const double fvx = xdir ? 0.0 : tv, fvy = xdir ? tv : 0.0;
    const double ax = f.rx * dx, ay = f.ry * dx;
    t[0] += fpx; t[1] += fpy; t[2] += fvx; t[3] += fvy;
    t[4] += ax * fpy - ay * fpx;
    t[5] += ax * fvy - ay * fvx;
}

// lanes -> lane 0 of the workgroup, in the fixed tree of block_sum2; lds: LOADS_REC doubles per wave.  Holds a barrier.
__device__ __forceinline__ void block_sum6(double (&t)[LOADS_REC], double *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < LOADS_REC; ++c) t[c] += __shfl_down(t[c], off, 64);
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < LOADS_REC; ++c) lds[LOADS_REC * w + c] = t[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < nw; ++k) {
#pragma unroll
            for (int c = 0; c < LOADS_REC; ++c) t[c] += lds[LOADS_REC * k + c];
        }
    }
}

// lane 0, behind the reduction: the record into the ring (or counted as dropped), and the counters
__device__ __forceinline__ void loads_tick(bool sample, long long n, const double (&t)[LOADS_REC], int cap, double *ring, long long *state)
{
    state[0] = n + 1;
    if (!sample) return;
    state[1] = state[1] + 1;
    const long long slot = state[2];
    if (slot < cap) {
#pragma unroll
        for (int c = 0; c < LOADS_REC; ++c) ring[(size_t)slot * LOADS_REC + c] = t[c];
        state[2] = slot + 1;
    } else {
        state[3] = state[3] + 1;
    }
}

// short lists: one workgroup, everything
template <typename T>
__global__ __launch_bounds__(LOADS_WG) void k_loads_one(const T *v, const T *p, const LoadFace *faces, int nf, size_t stride, double dx, double inv_re,
                                                        double limit, long long start, long long every, int cap, double *sums, double *ring,
                                                        long long *state)
{
    __shared__ double lds[LOADS_REC * LOADS_WG / 64];
    const long long n = state[0];                      // (every lane reads it before lane 0 writes it, behind the barrier below)
    const bool sample = samples_at(n, start, every);
    double t[LOADS_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (sample) {                                      // (the same branch in every lane: block_sum6 holds a barrier)
        for (int k = threadIdx.x; k < nf; k += LOADS_WG) loads_face(v, p, faces[k], k, stride, dx, inv_re, limit, sums, t);
        block_sum6(t, lds);
    }
    __syncthreads();
    if (threadIdx.x == 0) loads_tick(sample, n, t, cap, ring, state);
}

// split form, first launch: workgroup b takes faces [b LOADS_WG, (b + 1) LOADS_WG) and leaves its six sums in partial[6 b ..]
template <typename T>
__global__ __launch_bounds__(LOADS_WG) void k_loads_faces(const T *v, const T *p, const LoadFace *faces, int nf, size_t stride, double dx, double inv_re,
                                                          double limit, long long start, long long every, const long long *state, double *sums,
                                                          double *partial)
{
    __shared__ double lds[LOADS_REC * LOADS_WG / 64];
    if (!samples_at(state[0], start, every)) return;      // (the same in every lane of every workgroup)
    double t[LOADS_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int k = blockIdx.x * LOADS_WG + threadIdx.x;
    if (k < nf) loads_face(v, p, faces[k], k, stride, dx, inv_re, limit, sums, t);
    block_sum6(t, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < LOADS_REC; ++c) partial[(size_t)LOADS_REC * blockIdx.x + c] = t[c];
    }
}

// split form, second launch: the partials in workgroup order, the record, the counters
__global__ __launch_bounds__(LOADS_WG) void k_loads_record(const double *partial, int nparts, long long start, long long every, int cap, double *ring,
                                                           long long *state)
{
    __shared__ double lds[LOADS_REC * LOADS_WG / 64];
    const long long n = state[0];
    const bool sample = samples_at(n, start, every);
    double t[LOADS_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (sample) {
        for (int b = threadIdx.x; b < nparts; b += LOADS_WG) {
#pragma unroll
            for (int c = 0; c < LOADS_REC; ++c) t[c] += partial[(size_t)LOADS_REC * b + c];
        }
        block_sum6(t, lds);
    }
    __syncthreads();
    if (threadIdx.x == 0) loads_tick(sample, n, t, cap, ring, state);
}

}  // namespace fs
