"""The launch-list builder (csrc/fs_tiles.h) entry by entry, without a GPU: libfs_tiles_host.so hands the header's two functions to ctypes.
(a) every list equals the restatement tests/tiles_ref.py word for word; (b) properties that hold whether or not the restatement is right - above
all every "plain" bit against the mask itself: a tile wrongly marked plain computes wrong values, a dropped tile is fluid that is never updated.

Scenes at res 256 (512 x 256 cells): the smallest size at which tiles of every kind exist at once (at res 128 no tile is plain: a wave column at
the domain's edge never is) - plain and masked tiles in all four scenes, deep-wall tiles left out and XCD balancing at work in bc5."""
import ctypes
import os

import numpy as np
import pytest

import tiles_ref as R
from conftest import REPO

RES = 256
RANGES = [(0, RES), (3, 117), (130, 253)]      # the whole grid, and two ranges that cut tiles of every height at both ends
# (id, lanes, rows per tile, waves per workgroup, stacked, class, reach, parent tile rows): every list a launch site can ask for
SPECS = [
    ("pair-r2-all4", R.PAIR, 4, 1, False, R.ALL, 2, 0),               # fs_cip_step, one launch
    ("pair-r2-plain4", R.PAIR, 4, 1, False, R.PLAIN, 2, 0),           # ... two launches
    ("pair-r2-bnd4", R.PAIR, 4, 1, False, R.BOUNDARY, 2, 0),
    ("pair-r2-all2", R.PAIR, 2, 1, False, R.ALL, 2, 0),               # small grids
    ("pair-r2-plain2", R.PAIR, 2, 1, False, R.PLAIN, 2, 0),           # fs_cip_step_tiles there
    ("pair-r2-bnd2", R.PAIR, 2, 1, False, R.BOUNDARY, 2, 0),
    ("pair-r4-all2", R.PAIR, 2, 1, False, R.ALL, 4, 0),               # red-black pair / four-sweep Jacobi, hinted
    ("pair-r4-all4", R.PAIR, 4, 1, False, R.ALL, 4, 0),
    ("pair-r4-plain4", R.PAIR, 4, 1, False, R.PLAIN, 4, 0),           # f64 pair: plain part on 4-row tiles,
    ("pair-r4-bnd2-under4", R.PAIR, 2, 1, False, R.BOUNDARY, 4, 4),   # ... the rest on 2-row tiles under those
    ("pair-r4-mixed8-under16", R.PAIR, 8, 1, False, R.MIXED, 4, 16),  # the one-launch pair
    ("pair-r4-all2-4waves", R.PAIR, 2, 4, False, R.ALL, 4, 0),        # f64 pair, one launch
    ("wide-r1-all4-4waves", R.PAIR_WIDE, 4, 4, False, R.ALL, 1, 0),   # K2 of CIP, f64 Jacobi
    ("wide-r1-all2-4waves", R.PAIR_WIDE, 2, 4, False, R.ALL, 1, 0),
    ("wide-r2-all4-4waves", R.PAIR_WIDE, 4, 4, False, R.ALL, 2, 0),   # vorticity confinement, K2'
    ("wide-r2-all2-4waves", R.PAIR_WIDE, 2, 4, False, R.ALL, 2, 0),
    ("wide-r1-all4", R.PAIR_WIDE, 4, 1, False, R.ALL, 1, 0),          # the literal f32 Jacobi sweep
    ("wide-r0-all4-4waves", R.PAIR_WIDE, 4, 4, False, R.ALL, 0, 0),   # Poisson source, the carrying K3 + K4 pass: deep wall skipped, no hints
    ("wide-r2-plain4", R.PAIR_WIDE, 4, 1, False, R.PLAIN, 2, 0),      # K3 + K4 in two parts
    ("wide-r2-bnd4", R.PAIR_WIDE, 4, 1, False, R.BOUNDARY, 2, 0),
    ("quad-r2-plain2", R.QUAD, 2, 1, False, R.PLAIN, 2, 0),
    ("quad-r2-bnd2", R.QUAD, 2, 1, False, R.BOUNDARY, 2, 0),
    ("quad-r0-all1-4waves", R.QUAD, 1, 4, False, R.ALL, 0, 0),        # quads without hints: a list only where whole rows are deep wall
    ("quad-r0-all4-4waves", R.QUAD, 4, 4, False, R.ALL, 0, 0),
    ("wide-r2-all4-stacked", R.PAIR_WIDE, 4, 4, True, R.ALL, 2, 0),   # the stacked workgroup shape: 4 tile rows of one wave column
    ("wide-r0-all4-stacked", R.PAIR_WIDE, 4, 4, True, R.ALL, 0, 0),
    ("quad-r0-all1-stacked", R.QUAD, 1, 4, True, R.ALL, 0, 0),
]
INPUTS = ["bc1", "bc2", "bc3", "bc5", "random0", "random1", "random2"]

_lib = None


def shim():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_tiles_host.so"))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _lib.fs_tiles_activity.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
        _lib.fs_tiles_activity.restype = None
        _lib.fs_tiles_build.argtypes = [vp, vp, ci, ci, vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        _lib.fs_tiles_build.restype = ci
    return _lib


def lib_activity(mask, bcmap, rows, g0):
    X, Y = mask.shape
    out = {lanes: np.zeros(((X + R.WIDTH[lanes] - 1) // R.WIDTH[lanes], rows), np.uint8) for lanes in (R.QUAD, R.PAIR, R.PAIR_WIDE)}
    shim().fs_tiles_activity(mask.ctypes.data, bcmap.ctypes.data, X, Y, rows, g0, out[R.QUAD].ctypes.data, out[R.PAIR].ctypes.data, out[R.PAIR_WIDE].ctypes.data)
    return out


def lib_build(act, X, lanes, rt, wgw, stacked, group, cls, reach, parent_rt, jb, je, nbx, nby):
    """-> (words, per_xcd, count, needed), as tiles_ref.build"""
    spec = np.array([lanes, rt, wgw, int(stacked), group, cls, reach, parent_rt, jb, je, nbx, nby], np.int32)
    words = np.zeros(8 * (nbx * nby + 1), np.uint32)
    per_xcd, count = ctypes.c_int(), ctypes.c_int()
    n = shim().fs_tiles_build(spec.ctypes.data, act.ctypes.data, X, act.shape[1], words.ctypes.data, words.size, ctypes.byref(per_xcd), ctypes.byref(count))
    assert n >= 0, (n, spec)
    return words[:n].copy(), per_xcd.value, count.value, n > 0


def _random_scene(seed):
    """Cells of all four kinds on the scenes' grid: wall blobs large enough to hold deep wall, fluid areas large enough to leave plain tiles,
    a band of scattered wall cells, inflow / outflow cells at the edges and inside; random recipe bytes on some wall cells."""
    rng = np.random.default_rng(4200 + seed)
    X, Y = 2 * RES, RES
    mask = np.zeros((X, Y), np.uint8)
    for _ in range(5 + 3 * seed):
        i, j, w, h = rng.integers(0, X - 8), rng.integers(0, Y - 8), rng.integers(4, 150), rng.integers(4, 60)
        mask[i:i + w, j:j + h] = 1
    i0 = int(rng.integers(0, X - 130))
    band = mask[i0:i0 + 130, :]
    band[rng.random(band.shape) < 0.004] = 1
    mask[0:2, :] = 2
    mask[X - 1, Y // 3:2 * Y // 3] = 3
    for code in (2, 3):
        i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
        mask[i:i + 3, j:j + 5] = code
    bcmap = np.where((mask == 1) & (rng.random((X, Y)) < 0.3), rng.integers(1, 256, (X, Y)), 0).astype(np.uint8)
    return np.ascontiguousarray(mask), bcmap


_scenes = {}


def scene(name):
    """-> (mask, bcmap, {lanes: activity map of the restatement}), built once"""
    if name not in _scenes:
        if name.startswith("bc"):
            from fs.boundary_condition import create_scene_arrays
            mask = np.ascontiguousarray(create_scene_arrays(int(name[2:]), RES)[1].astype(np.uint8))
            bcmap = np.zeros_like(mask)      # (the recipe bytes come from the library's op lists: none here - wall cells inside a body are deep wall)
        else:
            mask, bcmap = _random_scene(int(name[6:]))
        assert mask.shape == (2 * RES, RES)
        _scenes[name] = (mask, bcmap, {lanes: R.activity(mask, bcmap, lanes) for lanes in (R.QUAD, R.PAIR, R.PAIR_WIDE)})
    return _scenes[name]


def cases(name):
    """every (spec, range) with its dense geometry and the library's answer"""
    mask, bcmap, acts = scene(name)
    X = mask.shape[0]
    for sid, lanes, rt, wgw, stacked, cls, reach, parent_rt in SPECS:
        for jb, je in RANGES:
            nbx, nby, group = R.launch_geometry(X, lanes, rt, wgw, stacked, jb, je)
            assert R.spec_ok(RES, lanes, rt, wgw, cls, parent_rt, nbx, nby), sid
            args = (acts[lanes], X, lanes, rt, wgw, stacked, group, cls, reach, parent_rt, jb, je, nbx, nby)
            yield f"{name} {sid} rows [{jb}, {je})", args, lib_build(*args)


def decode(words):
    """-> per XCD the list of (hints, by, bx), padding dropped"""
    return [[(int(e) >> 28, (int(e) >> 12) & 0xFFFF, int(e) & 0xFFF) for e in words[xcd::8] if e != R.PAD] for xcd in range(8)]


@pytest.mark.parametrize("name", INPUTS)
def test_activity_maps_equal_restatement(name):
    mask, bcmap, acts = scene(name)
    got = lib_activity(mask, bcmap, RES, 0)
    for lanes in acts:
        assert np.array_equal(got[lanes], acts[lanes]), (name, lanes)
    # slabs: ghost rows below the domain, a window inside it, rows past its top
    for rows, g0 in [(100, -3), (64, 97), (90, 200)]:
        got = lib_activity(mask, bcmap, rows, g0)
        for lanes in acts:
            assert np.array_equal(got[lanes], R.activity(mask, bcmap, lanes, rows, g0)), (name, lanes, rows, g0)


def test_activity_bits_by_hand():
    # one fluid cell at x = 120 (first cell of pair wave column 1, within column 0's halo lanes) in a field of deep wall; a recipe byte at x = 300
    mask = np.ones((512, 8), np.uint8)
    bcmap = np.zeros_like(mask)
    mask[120, 5] = 0
    bcmap[300, 2] = 7
    got = lib_activity(mask, bcmap, 8, 0)[R.PAIR]
    exp = np.full((5, 8), R.NONFLUID, np.uint8)
    exp[1, 5] |= R.WORK | R.FLUID
    exp[0, 5] |= R.FLUID              # (halo lanes see it; nothing to do there)
    exp[2, 2] |= R.WORK
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("name", INPUTS)
def test_lists_equal_restatement(name):
    n = 0
    for label, args, (words, per_xcd, count, needed) in cases(name):
        rwords, rper, rcount, rneeded = R.build(*args)
        assert needed == rneeded and per_xcd == rper and count == rcount, label
        assert np.array_equal(words, rwords), (label, int((words != rwords).sum()) if words.shape == rwords.shape else "sizes differ")
        n += 1
    assert n == len(SPECS) * len(RANGES)


def _plain_by_mask(mask, lanes, reach, wx0, wx1, p0, p1):
    """all cells that wave columns [wx0, wx1) touch - halo lanes included - within `reach` rows of rows [p0, p1) are fluid, the box inside the domain"""
    X, Y = mask.shape
    w, halo = R.WIDTH[lanes], R.HALO[lanes]
    if wx0 <= 0 or wx1 >= R.waves(X, lanes) or p0 - reach < 0 or p1 + reach > Y:
        return False
    return bool((mask[wx0 * w - halo:min(X, wx1 * w + halo), p0 - reach:p1 + reach] == 0).all())


def _work_tiles(name, lanes, rt, wgw, stacked, jb, je):
    """the workgroups (by, bx) with a cell of their own that is not deep wall, from mask and bcmap"""
    mask, bcmap, _ = scene(name)
    X, w = mask.shape[0], R.WIDTH[lanes]
    own = (mask != 1) | (bcmap != 0)
    nbx, nby, _ = R.launch_geometry(X, lanes, rt, wgw, stacked, jb, je)
    cols, rows = (1, wgw * rt) if stacked and wgw > 1 else (wgw, rt)
    return {(by, bx) for by in range(nby) for bx in range(nbx)
            if own[bx * cols * w:(bx + 1) * cols * w, jb + by * rows:min(je, jb + (by + 1) * rows)].any()}


@pytest.mark.parametrize("name", INPUTS)
def test_list_properties(name):
    mask = scene(name)[0]
    listed = {}
    for label, args, (words, per_xcd, count, needed) in cases(name):
        _, X, lanes, rt, wgw, stacked, group, cls, reach, parent_rt, jb, je, nbx, nby = args
        per = decode(words)
        tiles = [(by, bx) for v in per for _, by, bx in v]
        # (no list: a dense launch over every workgroup - or, for a class of tiles, nothing to launch)
        listed[(lanes, rt, wgw, stacked, cls, reach, parent_rt, jb, je)] = set(tiles) if needed or cls != R.ALL else {(by, bx) for by in range(nby) for bx in range(nbx)}
        if not needed:
            assert words.size == 0 and count == 0 and per_xcd == 0, label
            continue
        # no tile twice, every tile inside the dense grid, padding only at the tails
        assert len(tiles) == len(set(tiles)) == count, label
        assert all(by < nby and bx < nbx for by, bx in tiles), label
        assert words.size == per_xcd * 8 and per_xcd == max(len(v) for v in per), label
        for xcd in range(8):
            assert (words[xcd::8][len(per[xcd]):] == R.PAD).all(), label
        if count >= 64:
            assert per_xcd == (count + 7) // 8, label

        def rows_of(by, w=0):      # rows of wave w's tile as the range cuts them, and the uncut height
            t0 = jb + ((by * wgw + w) if stacked else by) * rt
            return t0, min(je, t0 + rt)

        def parent(j0, j1):        # the rows that decide "plain" for classes 1 - 3, and whether the range cuts them
            if parent_rt:
                p0 = jb + (j0 - jb) // parent_rt * parent_rt
                return p0, min(je, p0 + parent_rt), min(je, p0 + parent_rt) - p0 == parent_rt
            return j0, j1, j1 - j0 == (wgw if stacked else 1) * rt

        nw = R.waves(X, lanes)
        for xcd, v in enumerate(per):
            for hints, by, bx in v:
                if cls == R.ALL:
                    for w in range(4):
                        wx, (t0, t1) = (bx if stacked else bx * wgw + w), rows_of(by, w)
                        exp = reach > 0 and w < wgw and wx < nw and t0 < je and _plain_by_mask(mask, lanes, reach, wx, wx + 1, t0, t1)
                        assert bool(hints >> w & 1) == exp, (label, by, bx, w)
                    continue
                assert wgw == 1 and not stacked
                j0, j1 = rows_of(by)
                p0, p1, uncut = parent(j0, j1)
                plain = uncut and _plain_by_mask(mask, lanes, reach, bx, bx + 1, p0, p1)      # (a cut tile or cut parent is never plain)
                if cls == R.PLAIN:
                    assert plain and hints == 0, (label, by, bx)
                elif cls == R.BOUNDARY:
                    assert not plain and hints in (0, 2), (label, by, bx)
                else:
                    assert bool(hints & 1) == plain, (label, by, bx)
                    assert not plain or (hints == 1 and j0 == p0), (label, by, bx)
            # the entries that take the masked body stand first - among the XCD's own tiles: what balancing appends is the tail of another such list
            if (cls == R.ALL and wgw == 1 and any(h for u in per for h, _, _ in u)) or cls == R.MIXED:
                own = [h & 1 for h, by, bx in v if (by // group) % 8 == xcd]
                assert own == sorted(own), (label, xcd)
                if count < 64:
                    assert [h & 1 for h, _, _ in v] == own, (label, xcd)

    # a list of every workgroup with work holds exactly those (by the mask itself); the two parts of a split launch hold them too, each once
    for (lanes, rt, wgw, stacked, cls, reach, parent_rt, jb, je), tiles in listed.items():
        everything = _work_tiles(name, lanes, rt, wgw, stacked, jb, je)
        where = (name, lanes, rt, wgw, stacked, reach, jb, je)
        if cls == R.ALL:
            assert tiles == everything, where
        if cls != R.PLAIN:
            continue
        if (lanes, rt, wgw, stacked, R.BOUNDARY, reach, 0, jb, je) in listed:
            boundary = listed[(lanes, rt, wgw, stacked, R.BOUNDARY, reach, 0, jb, je)]
            assert tiles | boundary == everything and not tiles & boundary, where
        else:      # the boundary part on tiles of half the height under these parents
            boundary = listed[(lanes, rt // 2, wgw, stacked, R.BOUNDARY, reach, rt, jb, je)]
            halves = _work_tiles(name, lanes, rt // 2, wgw, stacked, jb, je)
            assert boundary <= halves and not {(by // 2, bx) for by, bx in boundary} & tiles, where
            assert all((by, bx) in boundary or (by // 2, bx) in tiles for by, bx in halves), where


def test_scenes_exercise_every_step():
    """What makes res 256 the right size: plain and masked tiles in every scene, deep wall skipped and entries moved between XCDs in bc5, both
    kinds of entry in the mixed list."""
    for name in ("bc1", "bc2", "bc3", "bc5"):
        by_label = {label: out for label, _, out in cases(name)}
        words, per_xcd, count, _ = by_label[f"{name} pair-r2-all4 rows [0, {RES})"]
        hints = [h for v in decode(words) for h, _, _ in v]
        assert 0 in hints and 1 in hints, name
        mixed = [h for v in decode(by_label[f"{name} pair-r4-mixed8-under16 rows [0, {RES})"][0]) for h, _, _ in v]
        assert 1 in mixed and any(h != 1 for h in mixed), name
        # quads, 4-row tiles, no hints: every workgroup spans the width and has work - the dense grid needs no list (1-row tiles: the scenes' outermost
        # wall rows are deep wall, and a list skips them)
        assert not by_label[f"{name} quad-r0-all4-4waves rows [0, {RES})"][3], name
        if name == "bc5":
            assert count == 320 - 38 and per_xcd == 36      # 38 of the 320 tiles are deep wall; dealt 40/37/32/32/32/32/37/40, balanced to <= 36
            own = [sum(1 for _, by, _ in v if (by // 8) % 8 == xcd) for xcd, v in enumerate(decode(words))]
            assert any(o < len(v) for o, v in zip(own, decode(words))), "no entry changed its XCD"
    for name in ("random0", "random1", "random2"):
        words = {label: out for label, _, out in cases(name)}[f"{name} pair-r2-all4 rows [0, {RES})"][0]
        hints = [h for v in decode(words) for h, _, _ in v]
        assert 0 in hints and 1 in hints, name
