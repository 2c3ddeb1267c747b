// fs_tiles_host.cpp - libfs_tiles_host.so: fs_tiles.h behind two C functions, for the CPU tests (tests/test_tile_lists_cpu.py).  Host compiler only,
// no HIP; test infrastructure - the product never loads it.
#include <cstring>

#include "fs_tiles.h"

extern "C" {

// The three activity maps of a scene: mask and bcmap in host layout (X, Y), `rows` local rows from global row g0.  Each output holds
// fs::geo_waves-many columns of `rows` bytes: ceil(X / 248), ceil(X / 120), ceil(X / 124).
void fs_tiles_activity(const uint8_t *mask_xy, const uint8_t *bcmap_xy, int X, int Y, int rows, int g0, uint8_t *quad, uint8_t *pair, uint8_t *pair_wide)
{
    const fs::ActivityMaps m = fs::activity_maps(mask_xy, bcmap_xy, X, Y, rows, g0);
    std::memcpy(quad, m.quad.data(), m.quad.size());
    std::memcpy(pair, m.pair.data(), m.pair.size());
    std::memcpy(pair_wide, m.pair_wide.data(), m.pair_wide.size());
}

// The list of spec[12] = {lanes, rt, wgw, stacked, group, cls, reach, parent_rt, jb, je, nbx, nby} over the activity map of that lane geometry.
// Returns the number of words (per_xcd x 8; 0: no list needed), -1 for a spec the builder does not define, -2 when `capacity` words do not hold it.
int fs_tiles_build(const int *spec, const uint8_t *act, int X, int rows, uint32_t *words, int capacity, int *per_xcd, int *count)
{
    fs::TileSpec s;
    s.lanes = spec[0]; s.rt = spec[1]; s.wgw = spec[2]; s.stacked = spec[3] != 0; s.group = spec[4]; s.cls = spec[5]; s.reach = spec[6];
    s.parent_rt = spec[7]; s.jb = spec[8]; s.je = spec[9]; s.nbx = spec[10]; s.nby = spec[11];
    *per_xcd = *count = 0;
    if (!fs::tile_spec_ok(s, rows)) return -1;
    const fs::TileWords t = fs::build_tile_list(s, act, X, rows);
    if ((int)t.words.size() > capacity) return -2;
    if (!t.words.empty()) std::memcpy(words, t.words.data(), t.words.size() * sizeof(uint32_t));
    *per_xcd = t.per_xcd; *count = t.count;
    return (int)t.words.size();
}

}  // extern "C"
