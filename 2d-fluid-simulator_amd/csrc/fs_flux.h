// fs_flux.h - scale-to-scale fluxes by filtering (new; the reference has none): the velocity and the vorticity box-filtered at up to FLUX_MAX_R
// widths, the sub-filter stresses, and the accumulated energy flux PI, enstrophy flux ZF and sub-filter energy K of every cell of a box, by
// launches that ride the step.  Everything is double, every operation rounded on its own (-ffp-contract=off), and the order of
// the operations that reach a value is fixed, so a plane is compared with == against the NumPy restatement (tests/flux_ref.py).  Single-GPU
// contexts.
//
// THE QUANTITIES of cell (i, j): U, W = (double) u, w where mask != 1 (fs_spec.h's rule), else +0 - through limit_cell while v still owes a
// deferred limit_field -; OM = vortex_grad_at(g, v, i, j, limit, 2 dx).om where mask == 0 (fs_dist.h's rule), else +0.  Eight base planes
// q0 .. q7 = U, W, OM, U U, U W, W W, U OM, W OM.
//
// THE FILTER of half-width r, n = 2 r + 1, inv = 1.0 / (double)(n n):
//   R_k(i, j) = (..((q_k(i - r, j) + q_k(i - r + 1, j)) + q_k(i - r + 2, j)) .. + q_k(i + r, j))      r <= i <= X - 1 - r   (flux_window_sum)
//   F_k(i, j) = ((..(R_k(i, j - r) + R_k(i, j - r + 1)) .. + R_k(i, j + r))) * inv                    r <= j <= Y - 1 - r
// The additions run strictly left to right: no running window, no summed-area table - they would change the rounding.
//
// THE FLUXES at a valid cell, r + 1 <= i <= X - 2 - r and r + 1 <= j <= Y - 2 - r (flux_cell; c the centre, l, r, m, n its x - 1, x + 1,
// y - 1, y + 1 neighbours, two_dx = 2.0 * dx):
//   tuu = F3 - F0 F0    tuw = F4 - F0 F1    tww = F5 - F1 F1    su = F6 - F0 F2    sw = F7 - F1 F2                      (at c)
//   ux = (F0r - F0l) / two_dx   uy = (F0n - F0m) / two_dx   wx, wy from F1 and ox, oy from F2 likewise   s12 = 0.5 (uy + wx)
//   PI = -((tuu ux + tww wy) + (2.0 tuw) s12)       ZF = -(su ox + sw oy)       K = 0.5 (tuu + tww)
// and S_PI[r][cell] += PI, S_ZF[r][cell] += ZF, S_K[r][cell] += K for the cells of the box: one owner lane per cell, so the order over the
// samples is fixed.  A cell of the box that is not valid for r keeps +0 for ever.  The filter reads outside the box, never outside the grid.
//
// THE WORK PLANES cover the region D: the box dilated by r_max + 1 and clipped to the grid, DW x DH cells, cell (i, j) at (j - dy0) DW + (i - dx0).
// Three sets of eight: base, R and F.  A valid cell of the box and its four neighbours find every value their windows need inside D; R and F
// hold +0 where the window leaves D (there it leaves the grid too, or no cell of the box asks).
//
// A SAMPLING LAUNCH (samples_at on the launch count, as every rider; the kernels of any other launch return at once):
//   1. k_flux_base<T>: the eight base planes over D - the only loads of v, the mask and the gradient's neighbours, once per sample.
//   per half-width:
//   2. k_flux_rows: R over D.  A workgroup of FLUX_ROW_WAVES waves takes a strip of FLUX_STRIP cells of FLUX_ROW_WAVES rows of ONE plane
//      (blockIdx.z); every wave stages its row's strip and a halo of r on each side (zeros outside D) in LDS.  A lane produces FLUX_ROW_V
//      ADJACENT outputs: it reads the n + FLUX_ROW_V - 1 staged values they cover once each and adds every one to the accumulators whose
//      window holds it (flux_window_multi) - the outputs share no partial sum, each is the ordered sum above.  BANKS: ds_read_b64 serves 32
//      lanes per cycle over 64 banks of 4 bytes, 32 doubles; lane l reads double l FLUX_ROW_V + t at step t, and FLUX_ROW_V is ODD, so 32
//      consecutive lanes hit 32 different doubles modulo 32: conflict-free without a padding word.  The outputs go back through LDS (lane
//      stride FLUX_ROW_V again) so that the stores to R are coalesced.
//   3. k_flux_cols: F over D.  A lane owns a column and FLUX_COL_V adjacent rows; the n + FLUX_COL_V - 1 loads of R it needs are coalesced
//      across the lanes; the same register reuse, then * inv.
//   4. k_flux_accumulate: one lane per cell of the box; the valid ones read F at c, l, r, m, n and add PI, ZF, K to their three sums.
//   5. k_spec_tick (fs_spec.h: [0] launches, [1] samples).
// 2 + 3 n_r launches per step, whatever the launch does: the sequence sits in replayed graphs.  fs_flux_filtered runs 2 and 3 of one
// half-width once more on the base planes of the last sampling launch, outside any capture.
//
// No kernel may use scratch; k_flux_rows holds FLUX_ROWS_LDS_BYTES of LDS, the others none (tests/test_build_metadata_flux.py).
#pragma once

#include <cstddef>

#include "fs_spec.h"

#if defined(__clang__)
#define FS_FLUX_UNROLL _Pragma("unroll")
#else
#define FS_FLUX_UNROLL
#endif

namespace fs {

constexpr int FLUX_NQ = 8;                // base planes (FS_FLUX_NQ)
constexpr int FLUX_SUMS = 3;              // accumulators per half-width: PI, ZF, K (FS_FLUX_NSUM)
constexpr int FLUX_MAX_WIDTHS = 8;        // half-widths per object (FS_FLUX_MAX_WIDTHS)
constexpr int FLUX_MAX_R = 64;            // largest half-width (FS_FLUX_MAX_R)
constexpr int FLUX_ROW_V = 7;             // adjacent outputs of a lane of k_flux_rows: odd (the bank argument above)
constexpr int FLUX_ROW_WAVES = 4;         // rows of a workgroup of k_flux_rows, one wave each
constexpr int FLUX_STRIP = 64 * FLUX_ROW_V;                        // outputs of a wave
constexpr int FLUX_ROW_PITCH = FLUX_STRIP + 2 * FLUX_MAX_R;        // staged doubles of a row
constexpr int FLUX_ROWS_LDS_BYTES = FLUX_ROW_WAVES * FLUX_ROW_PITCH * 8;
constexpr int FLUX_COL_V = 16;            // adjacent rows of a lane of k_flux_cols
constexpr int FLUX_COL_LANES = 256;       // columns of a workgroup of k_flux_cols
constexpr int FLUX_MAX_GROUPS = 4096;    // workgroups of a launch at most: the launches of a step that does not sample cost their dispatch alone
static_assert(FLUX_ROW_V % 2 == 1, "an even FLUX_ROW_V brings bank conflicts into k_flux_rows");

// workgroups of a one-dimensional launch over `items` items, 256 each (the kernels stride by the grid)
FS_SPEC_HD unsigned flux_groups(size_t items)
{
    const size_t g = (items + 255) / 256;
    return (unsigned)(g < (size_t)FLUX_MAX_GROUPS ? g : (size_t)FLUX_MAX_GROUPS);
}
// gridDim.y of a launch of gx x (up to `blocks`) x FLUX_NQ workgroups (the kernels stride by it)
FS_SPEC_HD unsigned flux_groups_y(int gx, int blocks)
{
    const int cap = FLUX_MAX_GROUPS / (gx * FLUX_NQ);
    return (unsigned)(blocks < cap ? blocks : (cap < 1 ? 1 : cap));
}

// the ordered sum of q[0 .. n - 1], `stride` doubles apart
FS_SPEC_HD double flux_window_sum(const double *q, long stride, int n)
{
    double s = q[0];
    for (int t = 1; t < n; ++t) s = s + q[t * stride];
    return s;
}

// V adjacent windows at once: acc[o] = the ordered sum of fetch(o) .. fetch(o + n - 1).  Every value is fetched once, t ascending, and added
// to the accumulators whose window holds it; an accumulator starts as its first value (no 0 + x).  Three phases so that the long middle
// one carries no condition: t < V - 1 (windows still opening), V - 1 <= t < n (all V), t >= n (windows closing).  n >= 1.
template <int V, typename F>
FS_SPEC_HD void flux_window_multi(F fetch, int n, double (&acc)[V])
{
FS_FLUX_UNROLL
    for (int t = 0; t < V - 1; ++t) {
        if (t < n + V - 1) {
            const double x = fetch(t);
FS_FLUX_UNROLL
            for (int o = 0; o < V; ++o) {
                if (o == t) acc[o] = x;
                else if (o < t && t - o < n) acc[o] = acc[o] + x;
            }
        }
    }
    if (V - 1 < n) {
        const double x = fetch(V - 1);
FS_FLUX_UNROLL
        for (int o = 0; o < V - 1; ++o) acc[o] = acc[o] + x;
        acc[V - 1] = x;
    }
    for (int t = V; t < n; ++t) {
        const double x = fetch(t);
FS_FLUX_UNROLL
        for (int o = 0; o < V; ++o) acc[o] = acc[o] + x;
    }
    const int t0 = n > V - 1 ? n : V - 1;
FS_FLUX_UNROLL
    for (int e = 0; e < V - 1; ++e) {
        const int t = t0 + e;
        if (t < n + V - 1) {
            const double x = fetch(t);
FS_FLUX_UNROLL
            for (int o = 1; o < V; ++o) {
                if (o == t) acc[o] = x;
                else if (o < t && t - o < n) acc[o] = acc[o] + x;
            }
        }
    }
}

// the eight filtered values of the centre, F0 .. F2 of its four neighbours -> (PI, ZF, K)
FS_SPEC_HD void flux_cell(const double (&c)[FLUX_NQ], const double (&l)[3], const double (&r)[3], const double (&m)[3], const double (&n)[3],
                          double two_dx, double &pi, double &zf, double &k)
{
    const double tuu = c[3] - c[0] * c[0], tuw = c[4] - c[0] * c[1], tww = c[5] - c[1] * c[1];
    const double su = c[6] - c[0] * c[2], sw = c[7] - c[1] * c[2];
    const double ux = (r[0] - l[0]) / two_dx, uy = (n[0] - m[0]) / two_dx;
    const double wx = (r[1] - l[1]) / two_dx, wy = (n[1] - m[1]) / two_dx;
    const double ox = (r[2] - l[2]) / two_dx, oy = (n[2] - m[2]) / two_dx;
    const double s12 = 0.5 * (uy + wx);
    pi = -((tuu * ux + tww * wy) + (2.0 * tuw) * s12);
    zf = -(su * ox + sw * oy);
    k = 0.5 * (tuu + tww);
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_vortex.h"

namespace fs {

// the region D of the work planes and the box inside it
struct FluxGeom { int dx0, dy0, DW, DH, x0, y0, nx, ny; };

// pass 1: the eight base planes over D.  limit > 0: v owes limit_field(limit).  flux_groups(cells of D) workgroups, a lane strides by the grid
template <typename T>
__global__ __launch_bounds__(256) void k_flux_base(Grid g, SpecWhen when, FluxGeom f, double limit, double two_dx, const T *v, double *base)
{
    if (!spec_on(when)) return;
    const size_t cells = (size_t)f.DW * f.DH;
    const T lim = (T)limit;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (size_t)gridDim.x * 256) {
        const int b = (int)(e / (size_t)f.DW), a = (int)(e - (size_t)b * f.DW);
        const int i = f.dx0 + a, j = f.dy0 + b;
        const int m = mask_at(g, i, j);
        double U = 0.0, W = 0.0, OM = 0.0;
        if (m != 1) {
            T u = at<2>(v, g, 0, i, j), w = at<2>(v, g, 1, i, j);
            if (lim > (T)0) limit_cell(u, w, lim);
            U = (double)u; W = (double)w;
        }
        if (m == 0) OM = vortex_grad_at(g, v, i, j, lim, two_dx).om;
        base[e] = U;
        base[cells + e] = W;
        base[2 * cells + e] = OM;
        base[3 * cells + e] = U * U;
        base[4 * cells + e] = U * W;
        base[5 * cells + e] = W * W;
        base[6 * cells + e] = U * OM;
        base[7 * cells + e] = W * OM;
    }
}

// pass 2: R over D, plane blockIdx.z.  grid (ceil(DW / FLUX_STRIP), flux_groups_y(..), FLUX_NQ), 64 FLUX_ROW_WAVES lanes; a workgroup walks the
// row blocks blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(64 * FLUX_ROW_WAVES) void k_flux_rows(SpecWhen when, int DW, int DH, int r, const double *base, double *R)
{
    __shared__ double st[FLUX_ROW_WAVES][FLUX_ROW_PITCH];
    if (!spec_on(when)) return;      // (the same in every lane of every workgroup: no barrier is left waiting)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int a0 = blockIdx.x * FLUX_STRIP, n = 2 * r + 1, blocks = (DH + FLUX_ROW_WAVES - 1) / FLUX_ROW_WAVES;
    double *s = st[wv];
    const double *mine = s + lane * FLUX_ROW_V;
    for (int rb = blockIdx.y; rb < blocks; rb += gridDim.y) {      // (the same trip count in every lane of the workgroup)
        const int b = rb * FLUX_ROW_WAVES + wv;
        const bool row = b < DH;
        const size_t off = (size_t)blockIdx.z * DW * DH + (size_t)(row ? b : 0) * DW;
        // slot t of the row holds column a0 - r + t of D; zeros outside D
        for (int t = lane; t < FLUX_STRIP + 2 * r; t += 64) {
            const int a = a0 - r + t;
            s[t] = row && a >= 0 && a < DW ? base[off + a] : 0.0;
        }
        __syncthreads();
        double acc[FLUX_ROW_V];
        flux_window_multi<FLUX_ROW_V>([=](int t) { return mine[t]; }, n, acc);
        __syncthreads();
FS_FLUX_UNROLL
        for (int o = 0; o < FLUX_ROW_V; ++o) {
            const int a = a0 + lane * FLUX_ROW_V + o;      // the centre of window o: columns a - r .. a + r
            s[lane * FLUX_ROW_V + o] = a - r >= 0 && a + r < DW ? acc[o] : 0.0;
        }
        __syncthreads();
        if (row)
            for (int t = lane; t < FLUX_STRIP; t += 64) {
                const int a = a0 + t;
                if (a < DW) R[off + a] = s[t];
            }
        __syncthreads();
    }
}

// pass 3: F over D, plane blockIdx.z.  grid (ceil(DW / FLUX_COL_LANES), flux_groups_y(..), FLUX_NQ), FLUX_COL_LANES lanes; a workgroup walks the
// blocks of FLUX_COL_V rows blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(FLUX_COL_LANES) void k_flux_cols(SpecWhen when, int DW, int DH, int r, double inv, const double *R, double *F)
{
    if (!spec_on(when)) return;
    const int a = blockIdx.x * FLUX_COL_LANES + threadIdx.x, n = 2 * r + 1, blocks = (DH + FLUX_COL_V - 1) / FLUX_COL_V;
    if (a >= DW) return;
    const size_t off = (size_t)blockIdx.z * DW * DH;
    const double *col = R + off + a;
    for (int cb = blockIdx.y; cb < blocks; cb += gridDim.y) {
        const int b0 = cb * FLUX_COL_V;
        double acc[FLUX_COL_V];
        // slot t is row b0 - r + t of D; zeros outside D (the outputs they reach are not stored)
        flux_window_multi<FLUX_COL_V>([=](int t) { const int b = b0 - r + t; return b >= 0 && b < DH ? col[(size_t)b * DW] : 0.0; }, n, acc);
FS_FLUX_UNROLL
        for (int o = 0; o < FLUX_COL_V; ++o) {
            const int b = b0 + o;
            if (b < DH) F[off + (size_t)b * DW + a] = b - r >= 0 && b + r < DH ? acc[o] * inv : 0.0;
        }
    }
}

// pass 4: the stencil on F and the three sums of half-width r; flux_groups(cells of the box) workgroups, a lane strides by the grid: one owner
// lane per cell.  acc: FLUX_SUMS planes of nx * ny doubles, [b][a]
__global__ __launch_bounds__(256) void k_flux_accumulate(SpecWhen when, FluxGeom f, int X, int Y, int r, double two_dx, const double *F, double *acc)
{
    if (!spec_on(when)) return;
    const size_t cells = (size_t)f.nx * f.ny, plane = (size_t)f.DW * f.DH;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (size_t)gridDim.x * 256) {
        const int b = (int)(e / (size_t)f.nx), a = (int)(e - (size_t)b * f.nx);
        const int i = f.x0 + a, j = f.y0 + b;
        if (i < r + 1 || i > X - 2 - r || j < r + 1 || j > Y - 2 - r) continue;      // not valid for r: +0 for ever
        const size_t c0 = (size_t)(j - f.dy0) * f.DW + (i - f.dx0);
        double c[FLUX_NQ], l[3], rr[3], m[3], n[3];
FS_FLUX_UNROLL
        for (int k = 0; k < FLUX_NQ; ++k) c[k] = F[k * plane + c0];
FS_FLUX_UNROLL
        for (int k = 0; k < 3; ++k) {
            l[k] = F[k * plane + c0 - 1];
            rr[k] = F[k * plane + c0 + 1];
            m[k] = F[k * plane + c0 - f.DW];
            n[k] = F[k * plane + c0 + f.DW];
        }
        double pi, zf, kk;
        flux_cell(c, l, rr, m, n, two_dx, pi, zf, kk);
        acc[e] = acc[e] + pi;
        acc[cells + e] = acc[cells + e] + zf;
        acc[2 * cells + e] = acc[2 * cells + e] + kk;
    }
}

}  // namespace fs
#endif  // __HIPCC__
