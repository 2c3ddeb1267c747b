// fs_lcs.h - flow maps through the resident snapshots (new; the reference has none): a lattice of particles carried through the ring of the
// snapshot POD (fs_pod.h), forwards or backwards in time, and the largest eigenvalue of the Cauchy-Green tensor of the map they end in - the
// finite-time Lyapunov exponent is log(lam) / (2 |T|), taken on the host (fs/lcs.py).  Only READS the ring; nothing here is part of a step
// or of a captured graph.
//
// State (fs_flowmap, fs_host.h): a lattice of nx = r (x1 - x0) by ny = r (y1 - y0) nodes over the cell box [x0, x1) x [y0, y1) with
// refinement r in {1, 2, 4, 8}; node (a, b) starts at (x0 + (a + 0.5) / r, y0 + (b + 0.5) / r) in the tracers' cell units (fs_tracer.h:
// cell (i, j) covers [i, i + 1) x [j, j + 1)) - exact in binary.  Structure of arrays indexed [b][a], a fastest, so that neighbouring lanes
// read neighbouring columns of the snapshot planes: x, y (double), status (int: 0 alive, 1 LEFT, 2 WALL as fs_tracer.h, 4 UNSEEDED), lam
// (double).
//
// k_flowmap_seed: the start positions; status 0, or UNSEEDED for a node whose start cell (floor x, floor y) has mask 1 (wall); lam NaN.  An
// UNSEEDED node is never moved.
//
// k_flowmap_advance<T>: one launch carries every alive node across ONE interval of the ring, from slot `from` to slot `to`, in S midpoint
// sub-steps (1 <= S <= 16) of signed size h (h = +- every dt / (dx S); the host swaps the slots and the sign to run backwards).  For
// sub-step k = 0 .. S - 1, with everything in double and every operation rounded on its own in the order written (-ffp-contract=off):
//   tau0 = (double)k / (double)S;  tau1 = ((double)k + 0.5) / (double)S
//   V(x, y, tau) = (1.0 - tau) * V_from(x, y) + tau * V_to(x, y)      per component; BOTH slots are always read, also at tau = 0
//   V_slot(x, y): tracer_velocity's bilinear interpolation (fs_tracer.h) of the slot's u and w planes as the ring stores them - the same
//                 corner clamp [0, X - 2] x [0, Y - 2], the same weight clamp [0, 1], the same expression
//                     sy * (sx * a00 + tx * a10) + ty * (sx * a01 + tx * a11).   Wall cells hold 0 in the ring; no limit pass is owed.
//   k1 = V(x, y, tau0);  (xm, ym) = (x, y) + (0.5 h) k1;  not inside the domain -> LEFT
//   k2 = V(xm, ym, tau1);  (xn, yn) = (x, y) + h k2;  not inside -> LEFT
//   the mask byte of cell (floor xn, floor yn): 1 -> WALL;  3 (outflow) -> LEFT when h > 0;  2 (inflow) -> LEFT when h < 0 (a particle
//   followed backwards into the inflow came from outside);  otherwise (x, y) = (xn, yn).
// A node with a fate keeps its last valid position and is never touched again.  inside() is false for NaN: no index is ever formed from a
// NaN.  A NumPy float64 restatement gives the same bits in f32 and in f64 runs (tests/lcs_ref.py).
//
// One launch per interval, not a lane-side loop over all intervals: every workgroup then gathers from the same two snapshots (at res 4096
// 537 MB of u, w in f32) instead of spreading over the whole ring.  The price is the state traffic: 20 B read and 20 B written per node and
// launch, against 32 gathered values per node and sub-step.  Shape: as k_tracer_advance - one node per lane, 256-lane workgroups, the 16
// loads of a stage issued before the first use, no atomics, a lane writes its own node only.
//
// k_flowmap_cauchy_green: for every node with status != UNSEEDED the flow-map gradient from the FINAL positions of its lattice neighbours.
// Per lattice direction (a, then b): with both neighbours present (inside the lattice and not UNSEEDED) the central difference
// (p_plus - p_minus) * (0.5 r); with exactly one the one-sided difference (p_plus - p) * r or (p - p_minus) * r; with neither lam = NaN.
// Dead neighbours (LEFT, WALL) take part with their frozen positions.  With dxx = dx/da, dyx = dy/da, dxy = dx/db, dyy = dy/db:
//   c11 = dxx * dxx + dyx * dyx;  c12 = dxx * dxy + dyx * dyy;  c22 = dxy * dxy + dyy * dyy
//   d = c11 - c22;  lam = 0.5 * (c11 + c22) + sqrt(0.25 * (d * d) + c12 * c12)
// every product, sum and the (correctly rounded) f64 square root rounded on its own.  UNSEEDED nodes get NaN.  No logarithm on the device.
//
// No kernel may use scratch (tests/test_build_metadata_lcs.py).
#pragma once
#include "fs_kernels.h"

namespace fs {

constexpr int FM_WG = 256;
constexpr int FM_ALIVE = 0, FM_LEFT = 1, FM_WALL = 2, FM_UNSEEDED = 4;      // 0 .. 2: the tracers' (fs_tracer.h TR_*; 3, EXPIRED, does not occur)
constexpr int FM_MAX_SUBSTEPS = 16;

struct FlowMapDev {
    int nx, ny;              // lattice nodes across / down
    int x0, y0, r;           // the box's first cell; nodes per cell and direction
    double *x, *y;
    int *status;
    double *lam;
};

// (fs_tracer.h tracer_inside: that header defines kernels of fs_tracers.hip and is included there alone)
__device__ __forceinline__ bool flowmap_inside(double x, double y, double X, double Y) { return x >= 0.0 && x < X && y >= 0.0 && y < Y; }

__global__ __launch_bounds__(FM_WG) void k_flowmap_seed(Grid g, FlowMapDev f)
{
    const int k = blockIdx.x * FM_WG + threadIdx.x;
    if (k >= f.nx * f.ny) return;
    const int a = k % f.nx, b = k / f.nx;
    const double r = (double)f.r;
    f.x[k] = (double)f.x0 + ((double)a + 0.5) / r;
    f.y[k] = (double)f.y0 + ((double)b + 0.5) / r;
    f.status[k] = mask_at(g, f.x0 + a / f.r, f.y0 + b / f.r) == 1 ? FM_UNSEEDED : FM_ALIVE;      // (the box lies inside the grid: fs_flowmap_create)
    f.lam[k] = __builtin_nan("");
}

// V(x, y, tau) for a point inside the domain; ua / ub: the u planes of the two slots (row pitch P), the w planes `plane` elements behind them
template <typename T>
__device__ __forceinline__ void flowmap_velocity(int X, int Y, int P, size_t plane, const T *__restrict__ ua, const T *__restrict__ ub, double x,
                                                 double y, double tau, double &u, double &w)
{
    const double fx = x - 0.5, fy = y - 0.5;
    const int i0 = min(max((int)floor(fx), 0), X - 2), j0 = min(max((int)floor(fy), 0), Y - 2);
    const double tx = fmin(fmax(fx - (double)i0, 0.0), 1.0), ty = fmin(fmax(fy - (double)j0, 0.0), 1.0);
    const size_t o0 = (size_t)j0 * P + i0, o1 = o0 + P;
    // the sixteen loads before the first use
    const T au00 = ua[o0], au10 = ua[o0 + 1], aw00 = ua[plane + o0], aw10 = ua[plane + o0 + 1];
    const T au01 = ua[o1], au11 = ua[o1 + 1], aw01 = ua[plane + o1], aw11 = ua[plane + o1 + 1];
    const T bu00 = ub[o0], bu10 = ub[o0 + 1], bw00 = ub[plane + o0], bw10 = ub[plane + o0 + 1];
    const T bu01 = ub[o1], bu11 = ub[o1 + 1], bw01 = ub[plane + o1], bw11 = ub[plane + o1 + 1];
    const double sx = 1.0 - tx, sy = 1.0 - ty;
    const double uA = sy * (sx * (double)au00 + tx * (double)au10) + ty * (sx * (double)au01 + tx * (double)au11);
    const double wA = sy * (sx * (double)aw00 + tx * (double)aw10) + ty * (sx * (double)aw01 + tx * (double)aw11);
    const double uB = sy * (sx * (double)bu00 + tx * (double)bu10) + ty * (sx * (double)bu01 + tx * (double)bu11);
    const double wB = sy * (sx * (double)bw00 + tx * (double)bw10) + ty * (sx * (double)bw01 + tx * (double)bw11);
    const double st = 1.0 - tau;
    u = st * uA + tau * uB;
    w = st * wA + tau * wB;
}

template <typename T>
__global__ __launch_bounds__(FM_WG) void k_flowmap_advance(Grid g, int Y, double h, int S, FlowMapDev f, const T *__restrict__ from,
                                                           const T *__restrict__ to, size_t plane)
{
    const int k = blockIdx.x * FM_WG + threadIdx.x;
    if (k >= f.nx * f.ny || f.status[k] != FM_ALIVE) return;
    double x = f.x[k], y = f.y[k];
    const double X = (double)g.X, Yd = (double)Y, hh = 0.5 * h, Sd = (double)S;
    const uint8_t gone = h > 0.0 ? 3 : 2;      // outflow ahead of a forward step, inflow ahead of a backward one
    int fate = FM_ALIVE;
#pragma unroll 1
    for (int s = 0; s < S && fate == FM_ALIVE; ++s) {
        const double tau0 = (double)s / Sd, tau1 = ((double)s + 0.5) / Sd;
        double ku, kw;
        flowmap_velocity<T>(g.X, Y, g.P, plane, from, to, x, y, tau0, ku, kw);
        const double xm = x + hh * ku, ym = y + hh * kw;
        if (!flowmap_inside(xm, ym, X, Yd)) { fate = FM_LEFT; break; }
        flowmap_velocity<T>(g.X, Y, g.P, plane, from, to, xm, ym, tau1, ku, kw);
        const double xn = x + h * ku, yn = y + h * kw;
        if (!flowmap_inside(xn, yn, X, Yd)) { fate = FM_LEFT; break; }
        const uint8_t m = mask_at(g, (int)floor(xn), (int)floor(yn));
        if (m == 1) fate = FM_WALL;
        else if (m == gone) fate = FM_LEFT;
        else { x = xn; y = yn; }
    }
    f.x[k] = x;
    f.y[k] = y;
    if (fate != FM_ALIVE) f.status[k] = fate;
}

// the difference of p along one lattice direction: `lo` / `hi` - the neighbour below / above is present; r = nodes per cell
__device__ __forceinline__ double flowmap_diff(bool lo, bool hi, double pm, double p, double pp, double r)
{
    if (lo && hi) return (pp - pm) * (0.5 * r);
    if (hi) return (pp - p) * r;
    return (p - pm) * r;
}

__global__ __launch_bounds__(FM_WG) void k_flowmap_cauchy_green(FlowMapDev f)
{
    const int k = blockIdx.x * FM_WG + threadIdx.x;
    if (k >= f.nx * f.ny) return;
    const double nan = __builtin_nan("");
    if (f.status[k] == FM_UNSEEDED) { f.lam[k] = nan; return; }
    const int a = k % f.nx, b = k / f.nx;
    // neighbours outside the lattice re-read the node itself (never used)
    const int kl = a > 0 ? k - 1 : k, kr = a < f.nx - 1 ? k + 1 : k, kd = b > 0 ? k - f.nx : k, ku = b < f.ny - 1 ? k + f.nx : k;
    const bool l = a > 0 && f.status[kl] != FM_UNSEEDED, r = a < f.nx - 1 && f.status[kr] != FM_UNSEEDED;
    const bool d = b > 0 && f.status[kd] != FM_UNSEEDED, u = b < f.ny - 1 && f.status[ku] != FM_UNSEEDED;
    const double x = f.x[k], y = f.y[k];
    const double xl = f.x[kl], xr = f.x[kr], xd = f.x[kd], xu = f.x[ku];
    const double yl = f.y[kl], yr = f.y[kr], yd = f.y[kd], yu = f.y[ku];
    if ((!l && !r) || (!d && !u)) { f.lam[k] = nan; return; }
    const double rd = (double)f.r;
    const double dxx = flowmap_diff(l, r, xl, x, xr, rd), dyx = flowmap_diff(l, r, yl, y, yr, rd);
    const double dxy = flowmap_diff(d, u, xd, x, xu, rd), dyy = flowmap_diff(d, u, yd, y, yu, rd);
    const double c11 = dxx * dxx + dyx * dyx, c12 = dxx * dxy + dyx * dyy, c22 = dxy * dxy + dyy * dyy;
    const double df = c11 - c22;
    f.lam[k] = 0.5 * (c11 + c22) + sqrt(0.25 * (df * df) + c12 * c12);
}

}  // namespace fs
