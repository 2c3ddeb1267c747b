// fs_tiles.h - the pure part of the compact launches: the scene's activity maps and the launch lists built from them.  Standard library only
// (no HIP header): fs_core.hip uploads and caches what build_tile_list() returns, fs_tiles_host.cpp hands the same functions to the CPU tests
// (tests/test_tile_lists_cpu.py compares every list word for word with a restatement and checks each plain bit against the mask itself).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cstddef>
#include <vector>

namespace fs {

// ---- the entry format ---------------------------------------------------------------------------------------------------------------------
// A launch list is K x 8 words: word [k * 8 + xcd] is the k-th workgroup of that XCD (fs_march.h band_coords),
//   entry = hints << 28 | by << 12 | bx        bx: block column (12 bits), by: block row (16 bits), hints: 4 bits whose meaning the class gives
// and the tails of the shorter lists are padded with TILE_PAD.  A real entry never equals the padding: tile_spec_ok() admits nbx <= 0xfff, so
// bx <= 0xffe even where every hint bit is set and by = 0xffff.
constexpr uint32_t TILE_PAD = 0xffffffffu;
constexpr int TILE_MAX_NBX = 0xfff, TILE_MAX_NBY = 0xffff, TILE_MAX_ROWS = 0xffff;
constexpr uint32_t tile_entry(uint32_t hints, int by, int bx) { return (hints << 28) | ((uint32_t)by << 12) | (uint32_t)bx; }
constexpr int tile_entry_bx(uint32_t e) { return (int)(e & 0xfffu); }
constexpr int tile_entry_by(uint32_t e) { return (int)((e >> 12) & 0xffffu); }
constexpr unsigned tile_entry_hints(uint32_t e) { return e >> 28; }
// hint bits by class (TileSpec::cls):
//   TILES_ALL       bit w: wave w of the workgroup is plain (one-wave workgroups: bit 0 = the tile is)
//   TILES_BOUNDARY  bit 1: a fluid cell in the tile's own rows, halo lanes included (one-wave workgroups)
//   TILES_MIXED     bit 0: an all-fluid parent tile, listed once at its lower unit; else bits 1, 2: fluid in the unit's first / second 4 rows
constexpr uint32_t HINT_PLAIN = 1u, HINT_FLUID = 2u;

// ---- wave geometries ----------------------------------------------------------------------------------------------------------------------
// `lanes` names how a wave of 64 lanes covers a row: owner lanes between halo lanes that re-read the neighbouring wave column's cells
enum { LANES_PAIR = 2, LANES_PAIR_WIDE = 3, LANES_QUAD = 4 };      // 60 owners x 2 cells (120, 4 halo cells per side), 62 x 2 (124, 2), 62 x 4 (248, 4)
constexpr int geo_cells(int lanes) { return lanes == LANES_QUAD ? 4 : 2; }
constexpr int geo_owners(int lanes) { return lanes == LANES_PAIR ? 60 : 62; }
constexpr int geo_width(int lanes) { return geo_cells(lanes) * geo_owners(lanes); }            // cells per wave column
constexpr int geo_halo(int lanes) { return (64 - geo_owners(lanes)) / 2 * geo_cells(lanes); }   // halo cells per side
inline int geo_waves(int X, int lanes) { return (X / geo_cells(lanes) + geo_owners(lanes) - 1) / geo_owners(lanes); }

// ---- activity maps ------------------------------------------------------------------------------------------------------------------------
// One byte per (wave column, LOCAL row) of each geometry, [wave column][row]:
//   ACT_WORK      some cell of the wave column's own cells is not deep wall (deep wall: a wall cell that no boundary kernel writes)
//   ACT_NONFLUID  a cell that is not fluid - or a row outside the domain - among the own cells or the halo lanes
//   ACT_FLUID     a fluid cell among the own cells or the halo lanes
enum : uint8_t { ACT_WORK = 1, ACT_NONFLUID = 2, ACT_FLUID = 4 };
struct ActivityMaps {
    std::vector<uint8_t> quad, pair, pair_wide;
    const std::vector<uint8_t> &of(int lanes) const { return lanes == LANES_QUAD ? quad : (lanes == LANES_PAIR ? pair : pair_wide); }
    std::vector<uint8_t> &of(int lanes) { return lanes == LANES_QUAD ? quad : (lanes == LANES_PAIR ? pair : pair_wide); }
    void clear() { quad.clear(); pair.clear(); pair_wide.clear(); }
};

// mask and bcmap in host layout (X, Y); `rows` local rows of which the first is global row g0 (a slab: its ghost rows included; rows outside
// the domain count as deep wall that is not fluid)
inline std::vector<uint8_t> activity_map(const uint8_t *mask_xy, const uint8_t *bcmap_xy, int X, int Y, int rows, int g0, int lanes)
{
    const int w = geo_width(lanes), halo = geo_halo(lanes), n = (X + w - 1) / w;
    std::vector<uint8_t> act((size_t)n * rows, 0);
    for (int i = 0; i < X; ++i) {
        const uint8_t *m = mask_xy + (size_t)i * Y, *b = bcmap_xy + (size_t)i * Y;
        uint8_t *a = act.data() + (size_t)(i / w) * rows;
        // the neighbouring wave column whose halo lanes cover column i, if any
        const int r = i % w;
        uint8_t *h = r < halo && i / w > 0 ? a - rows : (r >= w - halo && i / w + 1 < n ? a + rows : nullptr);
        for (int lr = 0; lr < rows; ++lr) {
            const int j = g0 + lr;
            if (j < 0 || j >= Y) { a[lr] |= ACT_NONFLUID; if (h) h[lr] |= ACT_NONFLUID; continue; }
            const uint8_t nf = m[j] != 0 ? ACT_NONFLUID : ACT_FLUID;
            a[lr] |= (uint8_t)((m[j] != 1 || b[j] != 0) ? ACT_WORK : 0) | nf;
            if (h) h[lr] |= nf;
        }
    }
    return act;
}
inline ActivityMaps activity_maps(const uint8_t *mask_xy, const uint8_t *bcmap_xy, int X, int Y, int rows, int g0)
{
    ActivityMaps m;
    for (int lanes : {LANES_QUAD, LANES_PAIR, LANES_PAIR_WIDE}) m.of(lanes) = activity_map(mask_xy, bcmap_xy, X, Y, rows, g0, lanes);
    return m;
}

// ---- the list specification ---------------------------------------------------------------------------------------------------------------
enum { TILES_ALL = 0, TILES_PLAIN = 1, TILES_BOUNDARY = 2, TILES_MIXED = 3 };
struct TileSpec {
    int lanes = LANES_QUAD;      // wave geometry
    int rt = 1;                  // rows per tile
    int wgw = 4;                 // waves per workgroup: side by side, or
    bool stacked = false;        // ... wgw tile rows of one wave column
    int group = 8;               // block rows per XCD group (fs_march.h band_coords)
    int cls = TILES_ALL;         // ALL: every workgroup with work; PLAIN / BOUNDARY: those whose tile sees nothing but fluid within reach ("plain": no mask
                                 // loads, no boundary views - their own kernel and register budget) / the others; MIXED: the one-launch red-black pair's units
    int reach = 0;               // rows above and below a tile that a plain tile must find all fluid (halo lanes included); ALL: 0 = no hints
    int parent_rt = 0;           // BOUNDARY / MIXED: plain is decided per parent tile of this many rows (the tiles of the launch's plain part); 0: per tile
    int jb = 0, je = 0;          // row range of the launch (slab launches cover varying ranges: one list per range)
    int nbx = 0, nby = 0;        // blocks of the dense grid the list replaces

    std::array<int, 10> key() const { return {{lanes, rt, stacked ? 1 : 0, group, cls, reach, wgw, parent_rt, jb, je}}; }      // (nbx, nby follow from these)
};
// what a list can express (the entry format's limits) and what the builder defines; a parent tile of the tile's own height is none
inline bool tile_spec_ok(TileSpec &s, int rows)
{
    if (s.parent_rt == s.rt) s.parent_rt = 0;
    if (s.nbx > TILE_MAX_NBX || s.nby > TILE_MAX_NBY || rows > TILE_MAX_ROWS || s.lanes > LANES_QUAD) return false;
    if (s.parent_rt && (s.wgw != 1 || s.parent_rt % s.rt != 0 || s.parent_rt > 64)) return false;      // (a coarser plain tiling is defined for one-wave workgroups)
    if (s.cls == TILES_MIXED && !(s.rt == 8 && s.parent_rt == 16 && s.wgw == 1 && s.lanes == LANES_PAIR)) return false;
    return true;
}

// ---- the builder --------------------------------------------------------------------------------------------------------------------------
struct TileWords {
    std::vector<uint32_t> words;      // per_xcd x 8, interleaved, padded; empty when the dense grid needs no list
    int per_xcd = 0, count = 0;       // count: listed workgroups (without the padding)
    bool needed = false;
};

namespace tiles_detail {

struct Act {      // one geometry's map with its extents
    const uint8_t *a; int waves, rows;
    bool any(int wx0, int wx1, int j0, int j1, uint8_t bit) const
    {
        for (int wx = wx0; wx < wx1; ++wx)
            for (int j = j0; j < j1; ++j)
                if (a[(size_t)wx * rows + j] & bit) return true;
        return false;
    }
};
struct Tile { int bx, by, wx0, wx1, j0, j1; };      // a workgroup: wave columns [wx0, wx1), rows [j0, j1) as the row range cuts them

// wave columns / rows of workgroup (bx, by): wgw waves side by side, or stacked = wgw tile rows of one column
inline Tile workgroup(const TileSpec &s, const Act &act, int bx, int by)
{
    const int wgw = s.wgw;
    return {bx, by, s.stacked ? bx : bx * wgw, std::min(act.waves, s.stacked ? bx + 1 : bx * wgw + wgw),
            s.jb + (s.stacked ? by * wgw : by) * s.rt, std::min(s.je, s.jb + (s.stacked ? by * wgw + wgw : by + 1) * s.rt)};
}
// No non-fluid cell in wave columns [wx0, wx1) within `reach` rows of rows [p0, p1) - and the whole box inside the domain: a wave column at
// the domain's first / last column clamps its halo lanes onto the edge cells, a row range that leaves the slab has rows nobody classified
// (the reference's scenes keep walls there; an uploaded mask need not).
inline bool plain_box(const TileSpec &s, const Act &act, int wx0, int wx1, int p0, int p1)
{
    if (wx0 <= 0 || wx1 >= act.waves || p0 - s.reach < 0 || p1 + s.reach > act.rows) return false;
    return !act.any(wx0, wx1, p0 - s.reach, p1 + s.reach, ACT_NONFLUID);
}
// ... of the rows that decide for tile t: its own, or the parent tile's it lies in.  A tile (or parent tile) the row range cuts short is
// never plain: the plain kernels may store every row of their tile, the kernels with masks guard `je`.
inline bool plain_tile(const TileSpec &s, const Act &act, const Tile &t)
{
    int p0 = t.j0, p1 = t.j1, full_rows = (s.stacked ? s.wgw : 1) * s.rt;
    if (s.parent_rt) { p0 = s.jb + (t.j0 - s.jb) / s.parent_rt * s.parent_rt; p1 = std::min(s.je, p0 + s.parent_rt); full_rows = s.parent_rt; }
    return p1 - p0 == full_rows && plain_box(s, act, t.wx0, t.wx1, p0, p1);
}

// Which workgroups a list holds and with which hints, one function per kind of list: false = not listed.
// TILES_ALL: every workgroup with work; with a reach, bit w says that wave w - ITS tile, halo lanes included - is plain: a kernel that holds
// both paths skips that wave's mask loads and the classification (band_coords cls)
inline bool entry_all(const TileSpec &s, const Act &act, const Tile &t, uint32_t &e)
{
    if (!act.any(t.wx0, t.wx1, t.j0, t.j1, ACT_WORK)) return false;
    uint32_t hints = 0u;
    if (s.reach > 0 && s.wgw <= 4)
        for (int w = 0; w < s.wgw; ++w) {
            const int wx = s.stacked ? t.bx : t.bx * s.wgw + w;
            const int t0 = s.jb + (s.stacked ? t.by * s.wgw + w : t.by) * s.rt, t1 = std::min(s.je, t0 + s.rt);
            if (wx >= act.waves || t0 >= s.je) continue;
            if (plain_box(s, act, wx, wx + 1, t0, t1)) hints |= HINT_PLAIN << w;
        }
    e = tile_entry(hints, t.by, t.bx);
    return true;
}
// TILES_PLAIN / TILES_BOUNDARY: the workgroups with work that are / are not plain.  The boundary list of one-wave workgroups says whether the
// tile's own rows hold a fluid cell: the general kernels then request their window without waiting for the masks that would tell them so
inline bool entry_split(const TileSpec &s, const Act &act, const Tile &t, uint32_t &e)
{
    if (!act.any(t.wx0, t.wx1, t.j0, t.j1, ACT_WORK)) return false;
    if (plain_tile(s, act, t) != (s.cls == TILES_PLAIN)) return false;
    const bool fluid = s.cls == TILES_BOUNDARY && s.wgw == 1 && act.any(t.bx, t.bx + 1, t.j0, t.j1, ACT_FLUID);
    e = tile_entry(fluid ? HINT_FLUID : 0u, t.by, t.bx);
    return true;
}
// TILES_MIXED (fs_rbpair.h k_rbsor_pair_all): units of rt = 8 rows; an all-fluid parent tile of parent_rt = 16 rows is ONE entry at its lower
// unit, any other unit with work an entry with the per-4-row-tile "fluid in its own rows" bits
inline bool entry_mixed(const TileSpec &s, const Act &act, const Tile &t, uint32_t &e)
{
    if (plain_tile(s, act, t)) {
        if ((t.j0 - s.jb) % s.parent_rt != 0) return false;
        e = tile_entry(HINT_PLAIN, t.by, t.bx);
        return true;
    }
    if (!act.any(t.wx0, t.wx1, t.j0, t.j1, ACT_WORK)) return false;
    uint32_t hints = 0u;
    for (int sub = 0; sub < 2; ++sub)
        if (act.any(t.bx, t.bx + 1, t.j0 + 4 * sub, std::min(t.j1, t.j0 + 4 * sub + 4), ACT_FLUID)) hints |= HINT_FLUID << sub;
    e = tile_entry(hints, t.by, t.bx);
    return true;
}

using PerXcd = std::array<std::vector<uint32_t>, 8>;

// One launch over both kinds of tile: the entries whose tile takes the longer, masked body go FIRST in each XCD's list - the all-fluid tiles
// fill in behind them and the launch does not end on the slow ones (fs_cip_step: 281.5-282.7 -> 279.1-280.7 us; the other way round 283.6-284.6)
inline void masked_first(PerXcd &per)
{
    for (auto &v : per) std::stable_partition(v.begin(), v.end(), [](uint32_t e) { return (tile_entry_hints(e) & HINT_PLAIN) == 0u; });
}
// The geometry deals a class of tiles unevenly (bc5 res 4096: the boundary tiles of the red-black pair 1003 .. 1365 per XCD) and a compact
// launch lasts as long as its fullest XCD.  An entry names its tile, so any XCD may run it: the surplus of an XCD - the END of its list, whole
// runs of vertically adjacent tiles - goes to the end of the emptiest lists.  Those tiles read their halo rows through another L2; they are
// a few per cent of the list.  Lists of fewer than 64 entries stay as dealt.
inline void balance_xcds(PerXcd &per, size_t total)
{
    if (total < 64) return;
    const size_t target = (total + 7) / 8;
    for (int d = 0; d < 8; ++d)
        while (per[d].size() > target) {
            int r = 0;
            for (int x = 1; x < 8; ++x) if (per[x].size() < per[r].size()) r = x;
            if (per[r].size() >= target) break;
            const size_t n = std::min(per[d].size() - target, target - per[r].size());
            per[r].insert(per[r].end(), per[d].end() - n, per[d].end());
            per[d].resize(per[d].size() - n);
        }
}
inline std::vector<uint32_t> interleave(const PerXcd &per, size_t K)
{
    std::vector<uint32_t> h(K * 8, TILE_PAD);
    for (int xcd = 0; xcd < 8; ++xcd)
        for (size_t k = 0; k < per[xcd].size(); ++k) h[k * 8 + xcd] = per[xcd][k];
    return h;
}

}  // namespace tiles_detail

// The list of spec `s` (tile_spec_ok) over `act`, the activity map of s.lanes for a grid X cells wide with `rows` local rows.
inline TileWords build_tile_list(const TileSpec &s, const uint8_t *act_map, int X, int rows)
{
    using namespace tiles_detail;
    const Act act{act_map, geo_waves(X, s.lanes), rows};
    const auto entry = s.cls == TILES_MIXED ? entry_mixed : (s.cls == TILES_ALL ? entry_all : entry_split);
    // XCD x takes the block-row groups x, x + 8, ... as the dense grid deals them; inside a group the workgroups are listed column by column:
    // vertically adjacent workgroups, which re-read each other's halo rows, are neighbours in dispatch order (bc5 res 4096: K3+K4 333 -> 319 us,
    // the red-black pair 195 -> 191 against row by row)
    PerXcd per;
    const int groups = (s.nby + s.group - 1) / s.group;
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int g = xcd; g < groups; g += 8)
            for (int bx = 0; bx < s.nbx; ++bx)
                for (int by = g * s.group; by < std::min(s.nby, (g + 1) * s.group); ++by) {
                    uint32_t e;
                    if (entry(s, act, workgroup(s, act, bx, by), e)) per[xcd].push_back(e);
                }
    size_t K = 0, total = 0;
    bool any_hint = s.cls == TILES_MIXED;
    for (auto &v : per) {
        total += v.size();
        if (s.cls == TILES_ALL) for (uint32_t e : v) any_hint = any_hint || tile_entry_hints(e) != 0u;
    }
    if ((s.cls == TILES_ALL || s.cls == TILES_MIXED) && any_hint && s.wgw == 1) masked_first(per);
    balance_xcds(per, total);
    for (auto &v : per) K = std::max(K, v.size());
    TileWords out;
    out.needed = K > 0 && (s.cls != TILES_ALL || any_hint || total < (size_t)s.nbx * s.nby);      // (nothing to skip, no hint to give: the dense grid needs no list)
    if (out.needed) { out.words = interleave(per, K); out.per_xcd = (int)K; out.count = (int)total; }
    return out;
}

}  // namespace fs
