// fs_history.h - per-step history of probe values and the pressure force on a body (new; the reference has none): ONE single-workgroup launch
// per step gathers u, w and p at a few probe cells and the pressure on the fluid side of a body's faces, and appends one record to a ring of
// doubles that stays on the device.  The launch counter and the write position live on the device too, so the launch can be captured into a
// hipGraph or recorded into a slab tape and replayed any number of times; the host drains the ring between replays (fs_history_read).
//
// Record layout (doubles): [force_x, force_y, u0, w0, p0, u1, w1, p1, ...].  A face term is the one k_flow_stats (fs_stats.h) adds for the
// same face, (double)p[fluid cell] * dx with the sign of the direction wall -> fluid; the face list is sorted by (row, column, direction) on
// the host, every lane folds the faces k = tid, tid + blockDim, ... in order, and block_sum2 (fs_kernels.h) combines the lanes in a fixed
// tree: repeated launches on the same state give identical bits.  No atomics; the counters are advanced by one lane behind a barrier.
// Long face lists (more than HIST_SPLIT faces: scene 1 at res 4096 has 1.8 k, scenes 3 and 5 35 - 42 k) take a first launch of one workgroup per
// HIST_FACES_PER_WG faces, one face per lane, whose partial sums the record launch then folds in workgroup order with the same tree: one
// workgroup walking 35 k faces took 55 us at bc5 res 4096 (a dependent gather per 1024 faces), 10 % of the step.
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int HIST_SPLIT = 512;          // faces up to which the record launch sums them itself (2 rounds of gathers per lane)
constexpr int HIST_FACES_PER_WG = 256;   // faces per workgroup of the split form
constexpr int HIST_STATE = 4;       // device counters (long long): [0] launches, [1] records in the ring, [2] records dropped (ring full)

// element offsets into the fields (fs_create bounds a context's rows x pitch below 2^31: the 2-channel offsets fit in 32 bits unsigned)
struct HistProbe { unsigned u, w, p; };
struct HistFace { unsigned p; int dir; };       // dir: 0 +x (force_x -= p dx), 1 -x (force_x += p dx), 2 +y (force_y -= p dx), 3 -y (force_y += p dx)

__device__ __forceinline__ void face_term(const HistFace f, double t, double &fx, double &fy)
{
    if (f.dir == 0) fx -= t;
    else if (f.dir == 1) fx += t;
    else if (f.dir == 2) fy -= t;
    else fy += t;
}

// split form, first launch: workgroup b sums faces [b HIST_FACES_PER_WG, (b + 1) HIST_FACES_PER_WG) into partial[2b], partial[2b + 1]; nothing when
// this step writes no record
template <typename T>
__global__ __launch_bounds__(HIST_FACES_PER_WG) void k_history_faces(const T *p, const HistFace *faces, int nf, double dx, int every, int cap,
                                                                     const long long *state, double *partial)
{
    __shared__ double lds[2 * HIST_FACES_PER_WG / 64];
    if ((state[0] + 1) % every != 0 || state[1] >= cap) return;      // (the same in every lane)
    double fx = 0.0, fy = 0.0;
    const int k = blockIdx.x * HIST_FACES_PER_WG + threadIdx.x;
    if (k < nf) {
        const HistFace f = faces[k];
        face_term(f, (double)p[f.p] * dx, fx, fy);
    }
    block_sum2(fx, fy, lds);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = fx; partial[2 * blockIdx.x + 1] = fy; }
}

// nparts > 0: the faces were summed by k_history_faces into `partial`.  limit > 0: v still owes limit_field(limit) - the probe's (u, w) go
// through limit_cell first, as the pass would store them
template <typename T>
__global__ __launch_bounds__(1024) void k_history_record(const T *v, const T *p, const HistProbe *probes, int np, const HistFace *faces, int nf,
                                                         const double *partial, int nparts, double dx, double limit, int every, int cap,
                                                         double *ring, long long *state)
{
    __shared__ double lds[32];
    const long long n = state[0], slot = state[1];      // (every lane reads them before lane 0 writes them, behind the barrier below)
    const bool rec = (n + 1) % every == 0;
    if (rec && slot < cap) {                            // (the same branch in every lane: block_sum2 holds a barrier)
        double *r = ring + (size_t)slot * (2 + 3 * (size_t)np);
        for (int k = threadIdx.x; k < np; k += blockDim.x) {
            const HistProbe q = probes[k];
            T u = v[q.u], w = v[q.w];
            if (limit > 0.0) limit_cell(u, w, (T)limit);
            r[2 + 3 * k] = (double)u;
            r[3 + 3 * k] = (double)w;
            r[4 + 3 * k] = (double)p[q.p];
        }
        double fx = 0.0, fy = 0.0;
        if (nparts > 0) {                               // split form: the first launch's partials, in workgroup order
            for (int k = threadIdx.x; k < nparts; k += blockDim.x) { fx += partial[2 * k]; fy += partial[2 * k + 1]; }
        } else {
            for (int k = threadIdx.x; k < nf; k += blockDim.x) {
                const HistFace f = faces[k];
                face_term(f, (double)p[f.p] * dx, fx, fy);
            }
        }
        block_sum2(fx, fy, lds);
        if (threadIdx.x == 0) { r[0] = fx; r[1] = fy; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = n + 1;
        if (rec) {
            if (slot < cap) state[1] = slot + 1;
            else state[2] = state[2] + 1;
        }
    }
}

}  // namespace fs
