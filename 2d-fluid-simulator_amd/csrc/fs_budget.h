// fs_budget.h - the budget of the fluctuation kinetic energy k = (<u'u'> + <w'w'>) / 2 (new; the reference has none): the raw moments that
// production, dissipation, the transports and the pressure terms need, accumulated per cell of a box by a launch that rides the step
// (the algebra is host work, fs/budgets.py).  Single-GPU contexts.
//
// State (fs_budget, fs_host.h): BUDGET_PLANES planes of double over the half-open cell box (x0, y0, x1, y1), dense rows of nx = x1 - x0
// (cell (a, b) of the box in plane s at s * plane + b * nx + a, plane = nx * ny + BUDGET_PAD), and the device counters (long long)
// [0] launches, [1] samples.  Launch n samples by samples_at (fs_device.h), as every rider: k_budget_accumulate only READS the counters
// and the one-lane k_budget_tick behind it advances them, so the pair can sit in a hipGraph.
//
// Per sampled FLUID cell (mask == 0) of the box, budget_cell below: u, w (through limit_cell while v still owes a deferred limit_field) and
// p promoted to double; ux, uy, wx, wy of vortex_grad (fs_cell.h: central differences, neighbour indices clamped at the grid's edge,
// neighbours taken as stored - through limit_cell as well when the limit is owed); a = u u, b = u w, c = w w, d = ux + wy; and
//     0-2 u w p | 3-5 a c b | 6-7 p u, p w | 8-11 a u, a w, c u, c w | 12-15 ux uy wx wy | 16-19 ux ux, uy uy, wx wx, wy wy | 20 p d
// added to the planes in this order, every operation rounded on its own (-ffp-contract=off).  One lane owns a cell and the samples arrive in
// stream order: no atomics, no LDS, and a NumPy f64 loop over downloads (tests/budget_ref.py) reproduces every plane with ==.  Planes 0 - 5
// are the averager's S_u, S_w, S_p, S_uu, S_ww, S_uw on those cells bit for bit (the same expressions).  A cell of the box that is not
// fluid keeps +0.
//
// THE KERNEL is a streaming read-modify-write whose traffic is the accumulators: 21 x 16 bytes per fluid cell against 3 field values, a
// mask byte and the re-read halo.  A lane takes W adjacent columns of the box: W = 2 when nx is even (every row of a plane is then 16-byte
// aligned and the planes move as 16-byte accesses; BUDGET_PAD is even), else the scalar W = 1.  The planes are staggered by BUDGET_PAD
// doubles for MEAN_PAD's reason: equally aligned planes of a power-of-two size would meet in one memory channel.  A workgroup takes 256 W
// columns and `rpw` rows and marches down them in groups of G = BUDGET_CELLS / W rows - the accumulators of a group are 84 VGPRs, which is
// what fixes G -: the mask bytes of the group first; then, unless all of the lane's cells in the group are not fluid, rows jg - 1 .. jg + G
// of u and w at the lane's own columns - the last two rows of the group before stay in registers, so a row of v comes from HBM once per
// workgroup column, plus two halo rows per `rpw` -, the columns i - 1 and i + W of the group's rows by loads of their own (they hit the
// lines the neighbouring lanes fetch; no shuffle, so a lane that skips a group of wall cells owes its neighbours nothing), p, and every
// accumulator of the group before the first use.  Field loads are scalar: x0 may be odd.
//
// No instantiation may use scratch or LDS (tests/test_build_metadata_budget.py).
#pragma once

#include "fs_cell.h"

namespace fs {

constexpr int BUDGET_PLANES = 21;         // FS_BUDGET_NPLANE
constexpr int BUDGET_STATE = 2;           // device counters (long long): [0] launches, [1] samples
constexpr int BUDGET_INPUTS = 11;         // u, w, p of the cell and (u, w) of its x - 1, x + 1, y - 1, y + 1 neighbours
constexpr int BUDGET_CELLS = 2;           // cells whose accumulators a lane holds at once: W columns x G rows (84 VGPRs)
constexpr int BUDGET_ROWS0 = 4;           // fewest rows per workgroup (small grids)
constexpr int BUDGET_ROWS = 32;           // most rows per workgroup: two halo rows are re-read per workgroup
constexpr int BUDGET_PAD = 544;           // doubles between two planes beyond the cells (even: 16-byte accesses stay aligned)
static_assert(BUDGET_PAD % 2 == 0 && BUDGET_ROWS0 % BUDGET_CELLS == 0, "fs_budget.h: pad and rows");

// the 21 values of a cell: (u, w, p) its own stored values, (ul, wl) .. (un, wn) those of its x - 1, x + 1, y - 1, y + 1 neighbours (indices
// clamped by the caller); limit > 0: v owes limit_field(limit)
template <typename T>
FS_CELL_HD void budget_cell(T u, T w, T p, T ul, T wl, T ur, T wr, T um, T wm, T un, T wn, T limit, double two_dx, double (&out)[BUDGET_PLANES])
{
    const VxGrad g = vortex_grad(ul, wl, ur, wr, um, wm, un, wn, limit, two_dx);
    if (limit > (T)0) limit_cell(u, w, limit);
    const double du = (double)u, dw = (double)w, dp = (double)p;
    const double a = du * du, b = du * dw, c = dw * dw, d = g.ux + g.wy;
    out[0] = du; out[1] = dw; out[2] = dp;
    out[3] = a; out[4] = c; out[5] = b;
    out[6] = dp * du; out[7] = dp * dw;
    out[8] = a * du; out[9] = a * dw; out[10] = c * du; out[11] = c * dw;
    out[12] = g.ux; out[13] = g.uy; out[14] = g.wx; out[15] = g.wy;
    out[16] = g.ux * g.ux; out[17] = g.uy * g.uy; out[18] = g.wx * g.wx; out[19] = g.wy * g.wy;
    out[20] = dp * d;
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_mean.h"

namespace fs {

struct BudgetBox { int x0, y0, nx, ny; };

// a workgroup takes 256 W columns and `rpw` rows of the box (rpw a multiple of BUDGET_CELLS / W); single-GPU grid: local row = global row
template <typename T, int W>
__global__ __launch_bounds__(256) void k_budget_accumulate(Grid g, BudgetBox b, int rpw, double limit, double two_dx, long long start, long long every,
                                                           const long long *state, const T *v, const T *p, double *sums, size_t plane)
{
    if (!samples_at(state[0], start, every)) return;      // (the same in every lane of every workgroup: k_budget_tick writes behind this launch)
    const int a = (blockIdx.x * 256 + threadIdx.x) * W;
    if (a >= b.nx) return;                                // (W = 2: nx is even, so a + 1 < nx as well)
    constexpr int G = BUDGET_CELLS / W;
    using DP = MeanPack<double, W>;
    const int i = b.x0 + a, il = clampx(g, i - 1), ir = clampx(g, i + W);
    const int r0 = blockIdx.y * rpw;
    const int r1 = r0 + rpw < b.ny ? r0 + rpw : b.ny;
    const T lim = (T)limit;
    T cu[G + 2][W], cw[G + 2][W];      // rows jg - 1 .. jg + G at the lane's columns
    bool have = false;                 // the group before this one loaded its rows
    for (int rg = r0; rg < r1; rg += G) {
        uint8_t mk[G][W];
        bool any = false;
#pragma unroll
        for (int r = 0; r < G; ++r) {      // rows of the group beyond r1 re-load row r1 - 1 and are not stored
            const int j = b.y0 + min(rg + r, r1 - 1);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                mk[r][c] = mask_at(g, i + c, j);
                any = any || mk[r][c] == 0;
            }
        }
        if (!any) { have = false; continue; }
#pragma unroll
        for (int k = 0; k < G + 2; ++k) {
            if (k < 2 && have) {
#pragma unroll
                for (int c = 0; c < W; ++c) { cu[k][c] = cu[k + G][c]; cw[k][c] = cw[k + G][c]; }
            } else {
                const int j = clampy(g, b.y0 + rg - 1 + k);
#pragma unroll
                for (int c = 0; c < W; ++c) { cu[k][c] = at<2>(v, g, 0, i + c, j); cw[k][c] = at<2>(v, g, 1, i + c, j); }
            }
        }
        have = true;
        T lu[G], lw[G], ru[G], rw[G], q[G][W];
        DP s[G][BUDGET_PLANES];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const int rr = min(rg + r, r1 - 1), j = b.y0 + rr;
            lu[r] = at<2>(v, g, 0, il, j); lw[r] = at<2>(v, g, 1, il, j);
            ru[r] = at<2>(v, g, 0, ir, j); rw[r] = at<2>(v, g, 1, ir, j);
#pragma unroll
            for (int c = 0; c < W; ++c) q[r][c] = at<1>(p, g, 0, i + c, j);
            const size_t e = (size_t)rr * b.nx + a;
#pragma unroll
            for (int k = 0; k < BUDGET_PLANES; ++k) s[r][k] = *(const DP *)(sums + k * plane + e);
        }
#pragma unroll
        for (int r = 0; r < G; ++r) {
            if (rg + r >= r1) continue;
            bool row = false;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (mk[r][c] != 0) continue;
                row = true;
                const T ul = c == 0 ? lu[r] : cu[r + 1][c > 0 ? c - 1 : 0], wl = c == 0 ? lw[r] : cw[r + 1][c > 0 ? c - 1 : 0];
                const T ur = c == W - 1 ? ru[r] : cu[r + 1][c < W - 1 ? c + 1 : c], wr = c == W - 1 ? rw[r] : cw[r + 1][c < W - 1 ? c + 1 : c];
                double out[BUDGET_PLANES];
                budget_cell(cu[r + 1][c], cw[r + 1][c], q[r][c], ul, wl, ur, wr, cu[r][c], cw[r][c], cu[r + 2][c], cw[r + 2][c], lim, two_dx, out);
#pragma unroll
                for (int k = 0; k < BUDGET_PLANES; ++k) s[r][k].v[c] += out[k];
            }
            if (row) {
                const size_t e = (size_t)(rg + r) * b.nx + a;
#pragma unroll
                for (int k = 0; k < BUDGET_PLANES; ++k) *(DP *)(sums + k * plane + e) = s[r][k];
            }
        }
    }
}

// behind k_budget_accumulate on the same stream: the launch count, and the sample count when that launch sampled
__global__ __launch_bounds__(64) void k_budget_tick(long long start, long long every, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) state[1] = state[1] + 1;
    state[0] = n + 1;
}

}  // namespace fs
#endif  // __HIPCC__
