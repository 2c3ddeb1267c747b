// fs_flux_host.cpp - the ordered window sum (one window, and the kernels' several-adjacent-windows form) and the per-cell flux function of
// fs_flux.h, the text the kernels run, compiled by the host compiler for the CPU tests (tests/test_flux_cpu.py).  Test infrastructure:
// libfs_hip.so does not link it.
#include "fs_flux.h"

extern "C" {

void fs_flux_host_limits(int *nq, int *sums, int *max_widths, int *max_r, int *row_v, int *col_v, int *strip, int *row_waves, int *col_lanes,
                         int *lds_bytes)
{
    *nq = fs::FLUX_NQ; *sums = fs::FLUX_SUMS; *max_widths = fs::FLUX_MAX_WIDTHS; *max_r = fs::FLUX_MAX_R; *row_v = fs::FLUX_ROW_V;
    *col_v = fs::FLUX_COL_V; *strip = fs::FLUX_STRIP; *row_waves = fs::FLUX_ROW_WAVES; *col_lanes = fs::FLUX_COL_LANES;
    *lds_bytes = fs::FLUX_ROWS_LDS_BYTES;
}

// out[c] = the ordered sum of q[c .. c + n - 1] for c = 0 .. count - 1 (q: count + n - 1 doubles), one window after the other
void fs_flux_host_window(const double *q, int count, int n, double *out)
{
    for (int c = 0; c < count; ++c) out[c] = fs::flux_window_sum(q + c, 1, n);
}

// the same sums as the kernels take them: `v` adjacent windows per call of flux_window_multi (v: FLUX_ROW_V or FLUX_COL_V; else -1).  count
// must be a multiple of v
int fs_flux_host_window_multi(const double *q, int count, int n, int v, double *out)
{
    if ((v != fs::FLUX_ROW_V && v != fs::FLUX_COL_V) || count % v) return -1;
    for (int c = 0; c < count; c += v) {
        const double *mine = q + c;
        if (v == fs::FLUX_ROW_V) {
            double acc[fs::FLUX_ROW_V];
            fs::flux_window_multi<fs::FLUX_ROW_V>([=](int t) { return mine[t]; }, n, acc);
            for (int o = 0; o < v; ++o) out[c + o] = acc[o];
        } else {
            double acc[fs::FLUX_COL_V];
            fs::flux_window_multi<fs::FLUX_COL_V>([=](int t) { return mine[t]; }, n, acc);
            for (int o = 0; o < v; ++o) out[c + o] = acc[o];
        }
    }
    return 0;
}

// flux_cell on `cells` cells: c [cells][8], l, r, m, n [cells][3] -> pi, zf, k [cells]
void fs_flux_host_cell(const double *c, const double *l, const double *r, const double *m, const double *n, long long cells, double two_dx, double *pi,
                       double *zf, double *k)
{
    for (long long e = 0; e < cells; ++e) {
        double cc[fs::FLUX_NQ], ll[3], rr[3], mm[3], nn[3];
        for (int q = 0; q < fs::FLUX_NQ; ++q) cc[q] = c[e * fs::FLUX_NQ + q];
        for (int q = 0; q < 3; ++q) { ll[q] = l[e * 3 + q]; rr[q] = r[e * 3 + q]; mm[q] = m[e * 3 + q]; nn[q] = n[e * 3 + q]; }
        fs::flux_cell(cc, ll, rr, mm, nn, two_dx, pi[e], zf[e], k[e]);
    }
}

}  // extern "C"
