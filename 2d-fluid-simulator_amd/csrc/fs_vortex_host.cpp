// fs_vortex_host.cpp - libfs_vortex_host.so: the union-find of fs_vortex.h (uf_find / uf_union, the text the kernels run) behind C functions,
// for tests/test_vortex_cpu.py.  Host compiler only, no HIP; test infrastructure - the product never loads it.
#include "fs_vortex.h"

extern "C" {

void fs_vortex_host_tile(int *tx, int *ty) { *tx = fs::VX_TX; *ty = fs::VX_TY; }

int fs_vortex_host_find(const int *parent, int x) { return fs::uf_find(parent, x); }

// the unions of `n` pairs (a, b) in the order given
void fs_vortex_host_unions(int *parent, const int *pairs, int n)
{
    for (int k = 0; k < n; ++k) fs::uf_union(parent, pairs[2 * k], pairs[2 * k + 1]);
}

// every parent >= 0 of the `n` cells -> its root (what k_vortex_compress does); returns the number of roots
int fs_vortex_host_compress(int *parent, int n)
{
    int roots = 0;
    for (int x = 0; x < n; ++x) {
        if (parent[x] < 0) continue;
        parent[x] = fs::uf_find(parent, x);
        roots += parent[x] == x;
    }
    return roots;
}

}  // extern "C"
