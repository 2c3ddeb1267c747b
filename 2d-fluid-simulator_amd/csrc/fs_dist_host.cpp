// fs_dist_host.cpp - libfs_dist_host.so: the bin rule, the order-preserving key and the digit pick of fs_dist.h (the text the kernels and
// fs_dist_select run) behind C functions, for tests/test_dist_cpu.py.  Host compiler only, no HIP; test infrastructure - the product never
// loads it.
#include "fs_dist.h"

extern "C" {

void fs_dist_host_limits(int *max_bins, int *max_channels, int *max_ranks, int *passes)
{
    *max_bins = fs::DIST_MAX_BINS; *max_channels = fs::DIST_MAX_CHANNELS; *max_ranks = fs::DIST_MAX_RANKS; *passes = fs::DIST_PASSES;
}

// out[k]: the bin of x[k], or -1 below, -2 above, -3 NaN; inv as fs_dist_create computes it
void fs_dist_host_bins(const double *x, int n, double lo, double hi, int B, int *out)
{
    const double inv = (double)B / (hi - lo);
    for (int k = 0; k < n; ++k) out[k] = fs::dist_bin(x[k], lo, hi, inv, B);
}

void fs_dist_host_keys(const double *x, int n, unsigned long long *keys)
{
    for (int k = 0; k < n; ++k) keys[k] = fs::dist_key(x[k]);
}

void fs_dist_host_unkeys(const unsigned long long *keys, int n, double *x)
{
    for (int k = 0; k < n; ++k) x[k] = fs::dist_unkey(keys[k]);
}

// the geometry of digit `pass`
void fs_dist_host_digit(int pass, int *shift, int *width) { *shift = fs::dist_shift(pass); *width = fs::dist_width(pass); }

// digit `pass` of every key that matches `prefix` above it, -1 for the others
void fs_dist_host_digits(const unsigned long long *keys, int n, unsigned long long prefix, int pass, int *out)
{
    for (int k = 0; k < n; ++k) out[k] = fs::dist_match(keys[k], prefix, pass) ? fs::dist_digit(keys[k], pass) : -1;
}

int fs_dist_host_pick(const long long *table, int nd, long long rank, long long *within) { return fs::dist_pick(table, nd, rank, within); }

}  // extern "C"
