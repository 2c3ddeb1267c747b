// fs_spec.h - energy spectra (new; the reference has none): the windowed 2-D FFT of the velocity over a box of cells and the accumulated
// power |Z'|^2 of every bin, by launches that ride the step.  The library links no FFT: the transform is this header.
// Everything is double, every operation rounded on its own (-ffp-contract=off), and the order of the operations that reach a value is fixed,
// so a plane is compared with == against the NumPy restatement (tests/spec_ref.py).  Single-GPU contexts.
//
// THE BOX: half-open cells (x0, y0, x1, y1), Nx = x1 - x0 and Ny = y1 - y0 powers of two in SPEC_MIN_N .. SPEC_MAX_N.  The host uploads the
// four tables - the windows wx[Nx], wy[Ny] and per axis N / 2 twiddles (cos, -sin) of 2 pi k / N as pairs of doubles - the device calls no
// sin or cos (as fs_modes.h).
//
// A SAMPLING LAUNCH (samples_at on the launch count, as every rider; the kernels of any other launch return at once):
//   1. k_spec_load_rows<T>: z = (u wx[a]) wy[b] + i (w wx[a]) wy[b] for cell (x0 + a, y0 + b) - u, w the stored values through limit_cell
//      while v still owes a deferred limit_field (limit > 0), promoted to double; wall cells (mask == 1) take +0 - and the transform of
//      every row along x.  One complex transform carries both components: |U|^2 + |W|^2 = (|Z[k]|^2 + |Z[-k]|^2) / 2.  -> plane A, [b][a].
//   2. k_spec_transpose: A [Ny][Nx] -> B [Nx][Ny] through a padded LDS tile of 32 x 32.
//   3. k_spec_rows: the transform of every row of B (along y) -> A, [a][b]: the (Nx, Ny) plane Z.
//   4. k_spec_power: one lane per bin.  Detrend (when on): Z'[a, b] = Z[a, b] - (Z00 c[a]) c[b] per component on the nine bins a, b in
//      {0, 1, N - 1}, c[0] = 1, c[1] = c[N - 1] = c1 of the axis (periodic Hann: W[0] = N / 2, W[+-1] = -N / 4 exactly, so c1 = -0.5 removes
//      the window-weighted mean without a reduction; boxcar: c1 = 0).  Z' -> B (what fs_spec_plane returns), P = P + (Z'.re Z'.re + Z'.im Z'.im).
//      One lane owns a bin: the sum over samples has a fixed order.  P is not symmetrised here.
//   5. k_spec_tick: one lane advances the counters [0] launches, [1] samples.
// Five launches per step, whatever the launch does: the sequence sits in replayed graphs.
//
// THE ROW TRANSFORM: radix 2, decimation in time - element n of a row is stored at the bit reversal of n, then log2 N stages of half-width
// h = 1, 2, ... N / 2.  Butterfly q (0 .. N / 2 - 1) of a stage works on i = (q / h) 2 h + q % h and j = i + h with twiddle table entry
// (q % h) (N / 2 h) (spec_pair), as spec_butterfly writes it.  The butterflies of a stage are independent, so their order does not reach the
// result: spec_row_transform (one row after the other, compiled by the host compiler too: csrc/fs_spec_host.cpp, the CPU tests) and the
// kernels run the same text and give the same bits.
//
// ON THE DEVICE a workgroup of 256 lanes takes SPEC_CHUNK = 4096 consecutive points of the plane - one row of 4096, two of 2048, ... 512 of 8
// (a plane below 4096 points: all of it) - and keeps them in LDS as two planes of doubles, 64 KB, through every stage: one read and one write
// of HBM per axis.  Because N divides the chunk and 2 h <= N, butterfly q of the CHUNK (0 .. 2047, lane l takes q = l, l + 256, ...) is the
// same formula with the chunk's point index for i: rows never mix and every row length runs the same code - what changes with N is the
// number of rows per workgroup alone.  BANKS: ds_read_b64 serves 32 lanes per cycle over 64 banks of 4 bytes, 32 doubles; the lanes of such
// a group read the 32 points out of 64 consecutive ones whose bit log2 h is clear (or set).  Point i lives at slot i ^ 31 when its bit 5 is
// set, else at i (spec_slot): two points of a group that differ in bit 5 would need complementary low bits to share a bank pair, which the
// common bit forbids - every stage reads conflict-free without a padding word, and stages of h >= 32 touch 32 consecutive points, a
// permutation of one bank row.
//
// No kernel may use scratch; the row kernels hold SPEC_LDS_BYTES of LDS (tests/test_build_metadata_spec.py).
#pragma once

#if defined(__HIPCC__)
#define FS_SPEC_HD __host__ __device__ inline
#else
#define FS_SPEC_HD inline
#endif

namespace fs {

constexpr int SPEC_MIN_N = 8;             // shortest side of a box (FS_SPEC_MIN_N)
constexpr int SPEC_MAX_N = 4096;          // longest (FS_SPEC_MAX_N): a row of complex doubles fills the LDS planes
constexpr int SPEC_CHUNK = 4096;          // points of a workgroup
constexpr int SPEC_LDS_BYTES = 2 * SPEC_CHUNK * 8;      // the re and the im plane of a chunk

// log2 of a power of two in SPEC_MIN_N .. SPEC_MAX_N; -1: anything else
FS_SPEC_HD int spec_log2(int n)
{
    for (int b = 3; b <= 12; ++b)
        if (n == (1 << b)) return b;
    return -1;
}
// the `bits` low bits of n in reverse order
FS_SPEC_HD int spec_bitrev(int n, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; ++b) r = (r << 1) | ((n >> b) & 1);
    return r;
}
// butterfly q of the stage of half-width h over rows of N points laid end to end: its upper point i (the lower one is i + h), its twiddle entry
FS_SPEC_HD void spec_pair(int q, int h, int N, int &i, int &k)
{
    const int m = q & (h - 1);
    i = ((q - m) << 1) + m;
    k = m * (N / (2 * h));
}
// a' = a + w b, b' = a - w b
FS_SPEC_HD void spec_butterfly(double &are, double &aim, double &bre, double &bim, double wre, double wim)
{
    const double tre = wre * bre - wim * bim;
    const double tim = wre * bim + wim * bre;
    const double xre = are, xim = aim;
    are = xre + tre; aim = xim + tim;
    bre = xre - tre; bim = xim - tim;
}
// one row in place, sequentially: tw holds N / 2 pairs (cos, -sin)
inline void spec_row_transform(double *re, double *im, int N, const double *tw)
{
    const int bits = spec_log2(N);
    for (int n = 0; n < N; ++n) {
        const int r = spec_bitrev(n, bits);
        if (n < r) {
            const double a = re[n], b = im[n];
            re[n] = re[r]; im[n] = im[r];
            re[r] = a; im[r] = b;
        }
    }
    for (int h = 1; h < N; h *= 2)
        for (int q = 0; q < N / 2; ++q) {
            int i, k;
            spec_pair(q, h, N, i, k);
            spec_butterfly(re[i], im[i], re[i + h], im[i + h], tw[2 * k], tw[2 * k + 1]);
        }
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_kernels.h"

namespace fs {

constexpr int SPEC_STATE = 2;             // device counters (long long): [0] launches, [1] samples
constexpr int SPEC_TILE = 32;             // side of the transpose's tile

struct SpecWhen { const long long *state; long long start, every; };
__device__ __forceinline__ bool spec_on(const SpecWhen &w) { return samples_at(w.state[0], w.start, w.every); }

__device__ __forceinline__ int spec_slot(int i) { return i ^ (((i >> 5) & 1) * 31); }

// the points of workgroup blockIdx.x: from `base`, `npts` of them (a power of two, a multiple of every row length)
__device__ __forceinline__ int spec_chunk(size_t total, size_t &base)
{
    base = (size_t)blockIdx.x * SPEC_CHUNK;
    return total - base < (size_t)SPEC_CHUNK ? (int)(total - base) : SPEC_CHUNK;
}

// every stage over the npts points in LDS (rows of N, bit-reversed already); leaves behind a barrier
__device__ __forceinline__ void spec_stages(double *re, double *im, int npts, int N, const double *__restrict__ tw)
{
    for (int h = 1; h < N; h <<= 1) {
        __syncthreads();
        for (int q = threadIdx.x; q < npts / 2; q += 256) {
            int i, k;
            spec_pair(q, h, N, i, k);
            const int si = spec_slot(i), sj = spec_slot(i + h);
            double are = re[si], aim = im[si], bre = re[sj], bim = im[sj];
            spec_butterfly(are, aim, bre, bim, tw[2 * k], tw[2 * k + 1]);
            re[si] = are; im[si] = aim;
            re[sj] = bre; im[sj] = bim;
        }
    }
    __syncthreads();
}

// pass 1: load, window and transform along x.  out: [Ny][Nx].  limit > 0: v owes limit_field(limit)
template <typename T>
__global__ __launch_bounds__(256) void k_spec_load_rows(Grid g, SpecWhen when, int x0, int y0, int nx, int ny, int lognx, double limit,
                                                        const T *v, const double *__restrict__ wx, const double *__restrict__ wy,
                                                        const double *__restrict__ tw, double2 *out)
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
        double zre = 0.0, zim = 0.0;
        if (mask_at(g, i, j) != 1) {
            T u = at<2>(v, g, 0, i, j), w = at<2>(v, g, 1, i, j);
            if (lim > (T)0) limit_cell(u, w, lim);
            zre = ((double)u * wx[a]) * wy[b];
            zim = ((double)w * wx[a]) * wy[b];
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

// pass 3: the transform of every row of `in` (rows of n points, `total` points) -> out, the same layout
__global__ __launch_bounds__(256) void k_spec_rows(SpecWhen when, int n, int logn, size_t total, const double2 *in, const double *__restrict__ tw,
                                                   double2 *out)
{
    __shared__ double re[SPEC_CHUNK], im[SPEC_CHUNK];
    if (!spec_on(when)) return;
    size_t base;
    const int npts = spec_chunk(total, base);
    for (int e = threadIdx.x; e < npts; e += 256) {
        const double2 z = in[base + e];
        const int s = spec_slot((e & ~(n - 1)) | spec_bitrev(e & (n - 1), logn));
        re[s] = z.x; im[s] = z.y;
    }
    spec_stages(re, im, npts, n, tw);
    for (int e = threadIdx.x; e < npts; e += 256) {
        const int s = spec_slot(e);
        out[base + e] = make_double2(re[s], im[s]);
    }
}

// pass 2: in [R][C] -> out [C][R]; grid (ceil(C / 32), ceil(R / 32))
__global__ __launch_bounds__(256) void k_spec_transpose(SpecWhen when, int R, int C, const double2 *in, double2 *out)
{
    __shared__ double tre[SPEC_TILE][SPEC_TILE + 1], tim[SPEC_TILE][SPEC_TILE + 1];
    if (!spec_on(when)) return;
    const int c0 = blockIdx.x * SPEC_TILE, r0 = blockIdx.y * SPEC_TILE, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < SPEC_TILE; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < R && c < C) {
            const double2 z = in[(size_t)r * C + c];
            tre[k][tx] = z.x; tim[k][tx] = z.y;
        }
    }
    __syncthreads();
    for (int k = ty; k < SPEC_TILE; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < R && c < C) out[(size_t)c * R + r] = make_double2(tre[tx][k], tim[tx][k]);
    }
}

// pass 4: z [Nx][Ny] -> zp = Z' and P += |Z'|^2, one lane per bin
__global__ __launch_bounds__(256) void k_spec_power(SpecWhen when, int nx, int ny, int logny, int detrend, double c1x, double c1y,
                                                    const double2 *z, double2 *zp, double *P)
{
    if (!spec_on(when)) return;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nx * ny) return;
    const int a = (int)(e >> logny), b = (int)(e & (size_t)(ny - 1));
    double2 c = z[e];
    if (detrend && (a <= 1 || a == nx - 1) && (b <= 1 || b == ny - 1)) {
        const double2 z00 = z[0];
        const double ca = a == 0 ? 1.0 : c1x, cb = b == 0 ? 1.0 : c1y;
        c.x = c.x - (z00.x * ca) * cb;
        c.y = c.y - (z00.y * ca) * cb;
    }
    zp[e] = c;
    P[e] = P[e] + (c.x * c.x + c.y * c.y);
}

// behind them on the same stream: the launch count, and the sample count when the launch sampled
__global__ __launch_bounds__(64) void k_spec_tick(long long start, long long every, long long *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = state[0];
    if (samples_at(n, start, every)) state[1] = state[1] + 1;
    state[0] = n + 1;
}

}  // namespace fs
#endif  // __HIPCC__
