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
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int TRACER_WG = 256;
constexpr int TR_ALIVE = 0, TR_LEFT = 1, TR_WALL = 2, TR_EXPIRED = 3;

struct TracerDev {
    int n;
    double *x, *y;
    int *age, *status, *respawns;
    const double *xs, *ys;
    long long *count;
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
        t.x[k] = t.xs[k];
        t.y[k] = t.ys[k];
        t.age[k] = 0;
        t.respawns[k] = t.respawns[k] + 1;
        return;
    }
    t.x[k] = px;
    t.y[k] = py;
    t.age[k] = age;
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

}  // namespace fs
