// fs_tiles_host.cpp - libfs_tiles_host.so: fs_tiles.h behind two C functions and fs_pick.h behind four, for the CPU tests
// (tests/test_tile_lists_cpu.py, tests/test_pick_cpu.py).  Host compiler only, no HIP; test infrastructure - the product never loads it.
#include <cstring>

#include "fs_pick.h"
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

// The division mode a launch takes (fs_pick.h), by kernel family: 0 - no dx-derived divisor, 1 - dx-derived divisors only, 2 - both kinds.  Through
// with_dm_*, so that what the launch sites call is what is tested; -1: the family called nothing.
int fs_pick_dm(int family, int f32, int dm)
{
    int got = -1;
    auto note = [&](auto DM) { got = DM; };
    bool found = false;
    if (f32) found = family == 0 ? fs::with_dm_const<float>(dm, note) : (family == 1 ? fs::with_dm_dx<float>(dm, note) : fs::with_dm_all<float>(dm, note));
    else found = family == 0 ? fs::with_dm_const<double>(dm, note) : (family == 1 ? fs::with_dm_dx<double>(dm, note) : fs::with_dm_all<double>(dm, note));
    return found ? got : -1;
}
// ... and the pure selection behind them
int fs_pick_dm_table(int family, int f32, int dm)
{
    return family == 0 ? fs::dm_pick_const(f32 != 0, dm) : (family == 1 ? fs::dm_pick_dx(f32 != 0, dm) : fs::dm_pick_all(f32 != 0, dm));
}
// pick over the list {2, 4, 8} nested in pick_bool: *called = 100 * flag + the value the callable saw (-1: none); returns what pick returned
int fs_pick_probe(int flag, int v, int *called)
{
    *called = -1;
    return fs::pick_bool(flag != 0, [&](auto FLAG) { return fs::pick<2, 4, 8>(v, [&](auto V) { *called = (FLAG ? 100 : 0) + V; }); }) ? 1 : 0;
}

}  // extern "C"
