// fs_spec_host.cpp - the bit reversal, the butterfly, the pairing of a stage and the sequential row transform of fs_spec.h, the text the
// kernels run, compiled by the host compiler for the CPU tests (tests/test_spec_cpu.py).  Test infrastructure: libfs_hip.so does not link it.
#include "fs_spec.h"

extern "C" {

void fs_spec_host_limits(int *min_n, int *max_n, int *chunk, int *lds_bytes)
{
    *min_n = fs::SPEC_MIN_N; *max_n = fs::SPEC_MAX_N; *chunk = fs::SPEC_CHUNK; *lds_bytes = fs::SPEC_LDS_BYTES;
}

int fs_spec_host_log2(int n) { return fs::spec_log2(n); }

void fs_spec_host_bitrev(int bits, int *out)
{
    for (int n = 0; n < (1 << bits); ++n) out[n] = fs::spec_bitrev(n, bits);
}

// every butterfly of the stage of half-width h over rows of N points, `nq` of them: i and the twiddle entry
void fs_spec_host_pairs(int nq, int h, int N, int *i_out, int *k_out)
{
    for (int q = 0; q < nq; ++q) fs::spec_pair(q, h, N, i_out[q], k_out[q]);
}

// ab: are, aim, bre, bim in place
void fs_spec_host_butterfly(double *ab, double wre, double wim) { fs::spec_butterfly(ab[0], ab[1], ab[2], ab[3], wre, wim); }

// `rows` rows of N points each, in place
void fs_spec_host_rows(double *re, double *im, int rows, int N, const double *tw)
{
    for (int r = 0; r < rows; ++r) fs::spec_row_transform(re + (long long)r * N, im + (long long)r * N, N, tw);
}

}  // extern "C"
