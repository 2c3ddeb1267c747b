// fs_xspec_host.cpp - the mirror index, the detrend of a bin and the split-and-accumulate of fs_xspec.h, the text the kernels run, compiled by
// the host compiler for the CPU tests (tests/test_xspec_cpu.py).  Test infrastructure: libfs_hip.so does not link it.
#include "fs_xspec.h"

extern "C" {

void fs_xspec_host_limits(int *nq, int *planes) { *nq = fs::XSPEC_NQ; *planes = fs::XSPEC_PLANES; }

// Z (re, im: nx * ny doubles, bin (a, b) at a * ny + b) -> Z' by xspec_detrend on every bin
void fs_xspec_host_detrend(const double *re, const double *im, int nx, int ny, int detrend, double c1x, double c1y, double *out_re, double *out_im)
{
    for (int a = 0; a < nx; ++a)
        for (int b = 0; b < ny; ++b) {
            const long long e = (long long)a * ny + b;
            double r = re[e], i = im[e];
            fs::xspec_detrend(r, i, a, b, nx, ny, detrend, re[0], im[0], c1x, c1y);
            out_re[e] = r; out_im[e] = i;
        }
}

// what one sampling launch of k_xspec_accumulate does with Z: Z' -> out_re / out_im, the sums of every bin added to acc (4 planes; pair == 0: 1)
void fs_xspec_host_accumulate(const double *re, const double *im, int nx, int ny, int detrend, int pair, double c1x, double c1y, double *out_re,
                              double *out_im, double *acc)
{
    const long long cells = (long long)nx * ny;
    for (int a = 0; a < nx; ++a)
        for (int b = 0; b < ny; ++b) {
            const int ma = fs::xspec_mirror(a, nx), mb = fs::xspec_mirror(b, ny);
            const long long e = (long long)a * ny + b, m = (long long)ma * ny + mb;
            double zr = re[e], zi = im[e], mr = re[m], mi = im[m];
            fs::xspec_detrend(zr, zi, a, b, nx, ny, detrend, re[0], im[0], c1x, c1y);
            fs::xspec_detrend(mr, mi, ma, mb, nx, ny, detrend, re[0], im[0], c1x, c1y);
            out_re[e] = zr; out_im[e] = zi;
            double paa = acc[e], pbb = 0.0, cre = 0.0, cim = 0.0;
            if (pair) { pbb = acc[cells + e]; cre = acc[2 * cells + e]; cim = acc[3 * cells + e]; }
            fs::xspec_split_add(zr, zi, mr, mi, pair != 0, paa, pbb, cre, cim);
            acc[e] = paa;
            if (pair) { acc[cells + e] = pbb; acc[2 * cells + e] = cre; acc[3 * cells + e] = cim; }
        }
}

}  // extern "C"
