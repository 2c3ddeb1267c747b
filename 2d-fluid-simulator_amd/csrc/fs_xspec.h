// fs_xspec.h - cross-spectra of two flow quantities (new; the reference has none): the windowed 2-D FFT of the packed plane a + i b over a box
// of cells - a, b two of the seven quantities of fs_dist.h - split into the transforms A, B of the two real fields, and the accumulated
// |A|^2, |B|^2 and A conj(B) of every bin, by launches that ride the step.  The transform is fs_spec.h's: spec_stages, spec_slot,
// spec_chunk, k_spec_transpose, k_spec_rows and k_spec_tick are used as they stand.  Everything is double, every operation rounded on its own
// (-ffp-contract=off), and the order of the operations that reach a value is fixed, so a plane is compared with == against the NumPy
// restatement (tests/xspec_ref.py).  Single-GPU contexts.
//
// THE BOX, THE TABLES, THE SAMPLING RULE: those of fs_spec.h.  THE QUANTITIES qa, qb: indices 0 "u", 1 "w", 2 "p", 3 "speed", 4 "vorticity",
// 5 "q", 6 "swirl" (dist_quantity of fs_dist.h, vortex_grad / vortex_criterion of fs_vortex.h); qb = -1: one scalar, the imaginary part is +0.
//
// A SAMPLING LAUNCH (the kernels of any other launch return at once):
//   1. k_xspec_load_rows<T>: z = (a wx[i]) wy[j] + i (b wx[i]) wy[j] and the transform of every row along x - k_spec_load_rows with more loads
//      per point.  u, w go through limit_cell and the gradient through vortex_grad(..., limit, 2 dx) while v still owes a deferred limit_field;
//      p is taken as stored; neighbours are clamped (clampx / clampy).  Only the loads the pair needs are issued (dist_need).  WHICH CELLS:
//      u, w, p, speed contribute where mask != 1 (fs_spec.h's rule: the pair (u, w) loads what k_spec_load_rows loads, bit for bit);
//      vorticity, q, swirl where mask == 0 (fs_dist.h's rule: the gradient is defined for fluid cells).  Any other cell takes +0.  qa, qb
//      are run-time arguments, the same in every lane.  -> plane A, [b][a].
//   2. k_spec_transpose, 3. k_spec_rows (along y) -> plane A again, [a][b]: the (Nx, Ny) plane Z.
//   4. k_xspec_accumulate: one lane per bin e = (a, b), its mirror m = ((Nx - a) mod Nx, (Ny - b) mod Ny).  The lane detrends BOTH Z[e] and
//      Z[m] from Z and Z00 (xspec_detrend: the nine-bin rule of k_spec_power; the mirror of one of the nine is one of the nine) - no lane
//      reads another's output -, writes Z'[e] to plane B (what fs_xspec_plane returns) and adds, with Z = Z'[e] and M = Z'[m]
//      (xspec_split_add):
//          A.re = 0.5 (Z.re + M.re)    A.im = 0.5 (Z.im - M.im)            A = (Z + conj M) / 2
//          B.re = 0.5 (Z.im + M.im)    B.im = 0.5 (M.re - Z.re)            B = (Z - conj M) / 2i
//          Paa += A.re A.re + A.im A.im        Pbb += B.re B.re + B.im B.im
//          Cre += A.re B.re + A.im B.im        Cim += A.im B.re - A.re B.im            C = A conj(B)
//      Four full (Nx, Ny) planes of doubles, one lane per bin: the sum over samples has a fixed order.  qb = -1: Paa alone.
//   5. k_spec_tick.
// Five launches per step, whatever the launch does: the sequence sits in replayed graphs.
//
// No kernel may use scratch; k_xspec_load_rows holds SPEC_LDS_BYTES of LDS, k_xspec_accumulate none (tests/test_build_metadata_xspec.py).
#pragma once

#include "fs_spec.h"

namespace fs {

constexpr int XSPEC_NQ = 7;               // quantities (DIST_NQ)
constexpr int XSPEC_PLANES = 4;           // accumulators of a pair: Paa, Pbb, Cre, Cim (FS_XSPEC_NPLANE); one scalar keeps the first

// the mirror of index a on an axis of n bins (n a power of two)
FS_SPEC_HD int xspec_mirror(int a, int n) { return (n - a) & (n - 1); }

// the detrend of bin (a, b) from Z00, per component: the nine-bin rule of k_spec_power
FS_SPEC_HD void xspec_detrend(double &re, double &im, int a, int b, int nx, int ny, int detrend, double z00re, double z00im, double c1x, double c1y)
{
    if (detrend && (a <= 1 || a == nx - 1) && (b <= 1 || b == ny - 1)) {
        const double ca = a == 0 ? 1.0 : c1x, cb = b == 0 ? 1.0 : c1y;
        re = re - (z00re * ca) * cb;
        im = im - (z00im * ca) * cb;
    }
}

// Z = Z'[e], M = Z'[m] -> the four sums of the bin; pair == false: paa alone (the other three are not touched)
FS_SPEC_HD void xspec_split_add(double zre, double zim, double mre, double mim, bool pair, double &paa, double &pbb, double &cre, double &cim)
{
    const double are = 0.5 * (zre + mre), aim = 0.5 * (zim - mim);
    paa = paa + (are * are + aim * aim);
    if (!pair) return;
    const double bre = 0.5 * (zim + mim), bim = 0.5 * (mre - zre);
    pbb = pbb + (bre * bre + bim * bim);
    cre = cre + (are * bre + aim * bim);
    cim = cim + (aim * bre - are * bim);
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_dist.h"

namespace fs {

// where quantity q contributes: the gradient quantities on fluid cells, the others everywhere but inside the walls
__device__ __forceinline__ bool xspec_selected(int q, int mask) { return q >= 4 ? mask == 0 : mask != 1; }

// pass 1: load the pair, window and transform along x.  out: [Ny][Nx].  limit > 0: v owes limit_field(limit).  need: dist_need(qa) | dist_need(qb)
template <typename T>
__global__ __launch_bounds__(256) void k_xspec_load_rows(Grid g, SpecWhen when, int x0, int y0, int nx, int ny, int lognx, int qa, int qb, int need,
                                                         double limit, double two_dx, const T *v, const T *p, const double *__restrict__ wx,
                                                         const double *__restrict__ wy, const double *__restrict__ tw, double2 *out)
{
    __shared__ double re[SPEC_CHUNK], im[SPEC_CHUNK];
    if (!spec_on(when)) return;      // (the same in every lane of every workgroup: k_spec_tick writes behind these launches)
    size_t base;
    const int npts = spec_chunk((size_t)nx * ny, base);
    const T lim = (T)limit;
    for (int e = threadIdx.x; e < npts; e += 256) {
        const size_t ge = base + e;
        const int b = (int)(ge >> lognx), a = (int)(ge & (size_t)(nx - 1));
        const int i = x0 + a, j = y0 + b;
        const int m = mask_at(g, i, j);
        const bool sa = xspec_selected(qa, m), sb = qb >= 0 && xspec_selected(qb, m);
        double zre = 0.0, zim = 0.0;
        if (sa || sb) {
            T u = (T)0, w = (T)0, pp = (T)0;
            VxGrad d = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (need & DIST_NEED_UW) {
                u = at<2>(v, g, 0, i, j); w = at<2>(v, g, 1, i, j);
                if (lim > (T)0) limit_cell(u, w, lim);
            }
            if (need & DIST_NEED_P) pp = at<1>(p, g, 0, i, j);
            if ((need & DIST_NEED_GRAD) && m == 0) d = vortex_grad_at(g, v, i, j, lim, two_dx);
            if (sa) zre = (dist_quantity(qa, u, w, pp, d) * wx[a]) * wy[b];
            if (sb) zim = (dist_quantity(qb, u, w, pp, d) * wx[a]) * wy[b];
        }
        const int s = spec_slot((e & ~(nx - 1)) | spec_bitrev(a, lognx));
        re[s] = zre; im[s] = zim;
    }
    spec_stages(re, im, npts, nx, tw);
    for (int e = threadIdx.x; e < npts; e += 256) {
        const int s = spec_slot(e);
        out[base + e] = make_double2(re[s], im[s]);
    }
}

// pass 4: z [Nx][Ny] -> zp = Z' and the sums of the bin, one lane per bin.  acc: XSPEC_PLANES planes of nx * ny doubles (pair == 0: one)
__global__ __launch_bounds__(256) void k_xspec_accumulate(SpecWhen when, int nx, int ny, int logny, int detrend, int pair, double c1x, double c1y,
                                                          const double2 *z, double2 *zp, double *acc)
{
    if (!spec_on(when)) return;
    const size_t cells = (size_t)nx * ny;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int a = (int)(e >> logny), b = (int)(e & (size_t)(ny - 1));
    const int ma = xspec_mirror(a, nx), mb = xspec_mirror(b, ny);
    const double2 z00 = z[0];
    double2 c = z[e], m = z[((size_t)ma << logny) | (size_t)mb];
    xspec_detrend(c.x, c.y, a, b, nx, ny, detrend, z00.x, z00.y, c1x, c1y);
    xspec_detrend(m.x, m.y, ma, mb, nx, ny, detrend, z00.x, z00.y, c1x, c1y);
    zp[e] = c;
    double paa = acc[e], pbb = 0.0, cre = 0.0, cim = 0.0;
    if (pair) { pbb = acc[cells + e]; cre = acc[2 * cells + e]; cim = acc[3 * cells + e]; }
    xspec_split_add(c.x, c.y, m.x, m.y, pair != 0, paa, pbb, cre, cim);
    acc[e] = paa;
    if (pair) { acc[cells + e] = pbb; acc[2 * cells + e] = cre; acc[3 * cells + e] = cim; }
}

}  // namespace fs
#endif  // __HIPCC__
