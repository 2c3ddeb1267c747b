"""The vortex identification without a GPU: (a) the union-find the kernels run (csrc/fs_vortex.h uf_find / uf_union, compiled by the host
compiler into libfs_vortex_host.so) against the breadth-first search of tests/vortex_ref.py - the tile-local roots as k_vortex_local leaves
them, then the unions of ALL seams in several shuffled sequential orders, then the compression; and the same from the identity with the unions
of all neighbour pairs; (b) the restatement against scipy.ndimage.label where SciPy exists; (c) the host conversions of fs.vortices against
the restatement's on random integers; (d) link / convection_velocity / street_spacing on synthetic records with known answers.

Grids: (37, 12) - odd X, one and a partial tile across; (1030, 8) - 33 column tiles of the 32 x 8 tile, the last partial, one tile row;
(300, 70) - more than one tile each way, neither extent a multiple of the tile."""
import ctypes
import os

import numpy as np
import pytest
from conftest import REPO

import vortex_ref as R

GRIDS = [(37, 12), (1030, 8), (300, 70)]
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_vortex_host.so"))
        ip = ctypes.POINTER(ctypes.c_int)
        _lib.fs_vortex_host_tile.argtypes = [ip, ip]
        _lib.fs_vortex_host_tile.restype = None
        _lib.fs_vortex_host_find.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.fs_vortex_host_find.restype = ctypes.c_int
        _lib.fs_vortex_host_unions.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        _lib.fs_vortex_host_unions.restype = None
        _lib.fs_vortex_host_compress.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.fs_vortex_host_compress.restype = ctypes.c_int
    return _lib


def tile():
    tx, ty = ctypes.c_int(), ctypes.c_int()
    lib().fs_vortex_host_tile(ctypes.byref(tx), ctypes.byref(ty))
    return tx.value, ty.value


def unions(parent, pairs):
    """parent: int32 (Y, X) plane (cell j * X + i), pairs (n, 2) -> in place."""
    pairs = np.ascontiguousarray(pairs, np.int32)
    lib().fs_vortex_host_unions(parent.ctypes.data, pairs.ctypes.data, len(pairs))


def compress(parent):
    return lib().fs_vortex_host_compress(parent.ctypes.data, parent.size)


def tile_local(flags, tx, ty):
    """What k_vortex_local leaves: per tile the smallest global index of the cell's component INSIDE the tile; int32 (Y, X)."""
    X, Y = flags.shape
    out = np.full((Y, X), -1, np.int32)
    for x0 in range(0, X, tx):
        for y0 in range(0, Y, ty):
            sub = flags[x0:x0 + tx, y0:y0 + ty]
            lab = R.label_plane(sub)
            w = sub.shape[0]
            glob = np.where(lab >= 0, (y0 + lab // w) * X + x0 + lab % w, -1)
            out[y0:y0 + ty, x0:x0 + tx] = glob.T
    return out


def seam_pairs(flags, tx, ty):
    X, Y = flags.shape
    idx = (np.arange(Y)[None, :] * X + np.arange(X)[:, None])
    pairs = []
    for i in range(tx, X, tx):
        m = (flags[i] != 0) & (flags[i] == flags[i - 1])
        pairs.append(np.stack([idx[i][m], idx[i - 1][m]], axis=1))
    for j in range(ty, Y, ty):
        m = (flags[:, j] != 0) & (flags[:, j] == flags[:, j - 1])
        pairs.append(np.stack([idx[:, j][m], idx[:, j - 1][m]], axis=1))
    return np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)


def all_pairs(flags):
    X, Y = flags.shape
    idx = (np.arange(Y)[None, :] * X + np.arange(X)[:, None])
    mx = (flags[1:] != 0) & (flags[1:] == flags[:-1])
    my = (flags[:, 1:] != 0) & (flags[:, 1:] == flags[:, :-1])
    return np.concatenate([np.stack([idx[1:][mx], idx[:-1][mx]], axis=1), np.stack([idx[:, 1:][my], idx[:, :-1][my]], axis=1)])


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_union_find_of_the_kernels_labels_every_pattern_in_any_order(grid):
    X, Y = grid
    tx, ty = tile()
    assert (tx, ty) == (32, 8)
    for name, flags in R.patterns(X, Y, tx, ty).items():
        want = R.label_plane(flags).T      # (Y, X)
        local = tile_local(flags, tx, ty)
        assert np.all(local <= np.where(local >= 0, np.arange(X * Y).reshape(Y, X), 0)), "a parent above its cell"
        seams = seam_pairs(flags, tx, ty)
        for seed in range(4):
            rng = np.random.default_rng(seed)
            parent = local.copy()
            order = rng.permutation(len(seams))
            flip = rng.random(len(seams)) < 0.5
            pairs = np.where(flip[:, None], seams[order][:, ::-1], seams[order])
            unions(parent, pairs)
            cells = np.arange(X * Y).reshape(Y, X)
            assert np.all((parent <= cells) | (parent < 0)), f"{name}: the invariant parent <= cell broke"
            roots = compress(parent)
            assert np.array_equal(parent, want), f"{grid} {name} seed {seed}: labels differ from the search"
            assert roots == len(np.unique(want[want >= 0]))
        # from the identity: every neighbour pair, shuffled
        parent = np.where(flags.T != 0, np.arange(X * Y).reshape(Y, X), -1).astype(np.int32)
        pairs = all_pairs(flags)
        unions(parent, pairs[np.random.default_rng(7).permutation(len(pairs))])
        compress(parent)
        assert np.array_equal(parent, want), f"{grid} {name}: labels from the identity differ from the search"


def test_patterns_are_what_the_tests_say():
    tx, ty = tile()
    p = R.patterns(1030, 8, tx, ty)
    lab = R.label_plane(p["serpentine"])
    assert set(np.unique(lab)) == {-1, 0} and (p["serpentine"][::2] == 1).all(), "the serpentine is not one component rooted at cell 0"
    assert p["serpentine"].sum() == 515 * 8 + 514
    p = R.patterns(300, 70, tx, ty)
    lab = R.label_plane(p["spiral"])
    assert set(np.unique(lab)) == {-1, 0} and p["spiral"].sum() > 300 * 70 // 3
    lab = R.label_plane(p["checkerboard"])
    on = p["checkerboard"] != 0
    idx = np.arange(70)[None, :] * 300 + np.arange(300)[:, None]
    assert np.array_equal(lab[on], idx[on]), "a checkerboard cell is not its own root"
    lab = R.label_plane(p["stripes"])
    assert len(np.unique(lab)) == 300, "the stripes joined"
    # U-shape: one component; each arm's tile-local root in the first tile row is not the component's minimum
    u = p["u_shape"]
    lab = R.label_plane(u)
    assert len(np.unique(lab[lab >= 0])) == 1
    local = tile_local(u, tx, ty)
    assert len(np.unique(local[:ty][local[:ty] >= 0])) == 2
    # random one sign: one component spans the grid from edge to edge; two signs: small components
    one = R.label_plane(p["random_one_sign"])
    ids, counts = np.unique(one[one >= 0], return_counts=True)
    big = one == ids[np.argmax(counts)]
    assert big[0].any() and big[-1].any() and big[:, 0].any() and big[:, -1].any(), "the largest component does not touch all four edges"
    assert counts.max() > 0.8 * (p["random_one_sign"] != 0).sum()
    two = R.label_plane(p["random_two_signs"])
    _, counts = np.unique(two[two >= 0], return_counts=True)
    assert 50 < counts.max() < 1000


def test_restatement_agrees_with_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for X, Y in ((37, 12), (520, 140)):
        for name, flags in R.patterns(X, Y).items():
            lab = R.label_plane(flags)
            for f in (1, 2):
                sl, n = ndi.label(flags == f)
                assert len(np.unique(lab[flags == f])) == n, (name, f)
                for k in range(1, n + 1):
                    m = sl == k
                    idx = (np.arange(Y)[None, :] * X + np.arange(X)[:, None])[m]
                    assert np.all(lab[m] == idx.min()), (name, f, k)


def test_conversions_equal_the_restatement():
    from fs import vortices as V
    assert V.RECORD == R.RECORD and (V.NHEAD, V.NREC) == (R.NHEAD, R.NREC)
    for om, want in ((1.0, 0), (2.0, 1), (2.1, 2), (0.75, 0), (0.5, -1), (2560.0, 12), (4096.0, 12), (4097.0, 13)):
        assert V.omega_exponent(om) == R.omega_exponent(om) == want, om
    rng = np.random.default_rng(3)
    n, nx = 200, 8192
    area = rng.integers(1, 1 << 27, n)
    raw = {"label": rng.integers(0, 1 << 26, n), "area": area, "sum_q": rng.integers(-(1 << 57), 1 << 57, n), "sum_aq": rng.integers(0, 1 << 57, n),
           "sum_x": rng.integers(1, 1 << 42, n), "sum_y": rng.integers(1, 1 << 42, n), "mx_lo": rng.integers(0, 1 << 59, n),
           "mx_hi": rng.integers(0, 1 << 40, n), "my_lo": rng.integers(0, 1 << 59, n), "my_hi": rng.integers(0, 1 << 40, n),
           "xmin": rng.integers(0, 100, n), "xmax": rng.integers(100, 200, n), "ymin": rng.integers(0, 100, n), "ymax": rng.integers(100, 200, n),
           "peak": (rng.integers(0, (1 << 30) + 1, n) << 32) | (0xFFFFFFFF - rng.integers(0, 1 << 26, n)), "flag": rng.integers(1, 3, n),
           "sample": np.zeros(n, np.int64)}
    raw["sum_aq"][:5] = 0
    for e in (-3, 0, 13):
        got, want = V.convert(raw, e, 1.0 / 4096, nx), R.convert(raw, e, 1.0 / 4096, nx)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (e, k)


def _street(n_samples=6, speed=(0.75, -0.125), a=10.0, h=3.0, n=4):
    """Two rows of n points each, spacing a, the negative row h below the positive one and staggered by a / 2, all moving at `speed` cells
    per sample; records in (sample, label) order with labels that keep the row-major order."""
    rec = {k: [] for k in ("sample", "label", "sign", "x", "y")}
    for s in range(n_samples):
        pts = [(20.0 + a * k + speed[0] * s, 10.0 + speed[1] * s, -1) for k in range(n)]
        pts += [(20.0 + a * (k + 0.5) + speed[0] * s, 10.0 + h + speed[1] * s, 1) for k in range(n)]
        for x, y, sg in sorted(pts, key=lambda q: (int(q[1]), q[0])):
            rec["sample"].append(s); rec["label"].append(int(y) * 1000 + int(x)); rec["sign"].append(sg); rec["x"].append(x); rec["y"].append(y)
    return {k: np.array(v) for k, v in rec.items()}


def test_link_velocity_and_spacing_on_a_synthetic_street():
    from fs import vortices as V
    rec = _street()
    tracks = V.link(rec, max_distance=2.0, dt=1.0)
    assert tracks.min() == 0 and tracks.max() == 7, "8 points, 8 tracks"
    for t in range(8):
        m = tracks == t
        assert m.sum() == 6 and len(set(rec["sign"][m])) == 1
        assert np.allclose(np.diff(rec["x"][m]), 0.75) and np.allclose(np.diff(rec["y"][m]), -0.125)
    dx, dt = 0.5, 0.25
    cv = V.convection_velocity(rec, tracks, dx, dt)
    assert np.allclose(cv["ux"], 0.75 * dx / dt, rtol=1e-12) and np.allclose(cv["uy"], -0.125 * dx / dt, rtol=1e-12) and (cv["n"] == 6).all()
    sp = V.street_spacing(rec, tracks, dx)
    assert np.isclose(sp["a"], 10.0 * dx) and np.isclose(sp["a_pos"], 10.0 * dx) and np.isclose(sp["a_neg"], 10.0 * dx)
    assert np.isclose(sp["h"], 3.0 * dx) and np.isclose(sp["ratio"], 0.3)
    # too small a reach: nothing links, every record its own track; the opposite sign is never linked however near
    assert len(np.unique(V.link(rec, max_distance=0.1))) == len(rec["x"])
    near = {"sample": np.array([0, 1]), "label": np.array([5, 5]), "sign": np.array([1, -1]), "x": np.array([3.0, 3.0]), "y": np.array([4.0, 4.0])}
    assert V.link(near, 5.0).tolist() == [0, 1]
    # a tie in distance goes to the smaller label; each record is used once
    tie = {"sample": np.array([0, 1, 1]), "label": np.array([7, 3, 9]), "sign": np.array([1, 1, 1]), "x": np.array([5.0, 4.0, 6.0]),
           "y": np.array([5.0, 5.0, 5.0])}
    assert V.link(tie, 2.0).tolist() == [0, 0, 1]
    # the prediction: a fast track is followed past a nearer newcomer
    fast = {"sample": np.array([0, 1, 2, 2]), "label": np.array([1, 2, 3, 4]), "sign": np.ones(4, np.int64), "x": np.array([0.0, 4.0, 8.0, 4.5]),
            "y": np.zeros(4)}
    assert V.link(fast, 4.5).tolist() == [0, 0, 0, 1]
    empty = {k: np.zeros(0) for k in ("sample", "label", "sign", "x", "y")}
    assert len(V.link(empty, 1.0)) == 0


def test_abi_table_holds_the_new_entries():
    from fs import _lib as L
    for name in ("create", "launch", "read", "get_labels", "set", "label", "criterion", "free"):
        assert "fs_vortex_" + name in L.EXPORTS
    assert L.ABI_VERSION >= 23


def test_restatement_sample_on_a_hand_made_field():
    """Two counter-rotating Rankine-like patches on a 24 x 16 grid: two records of opposite sign, circulation of opposite sign, centroids at
    the patches' centres; the caps keep the components of smallest label."""
    X, Y, dx = 24, 16, 0.25
    i, j = np.meshgrid(np.arange(X) + 0.5, np.arange(Y) + 0.5, indexing="ij")
    v = np.zeros((X, Y, 2), np.float32)
    for cx, cy, s in ((6.0, 8.0, 1.0), (18.0, 8.0, -1.0)):
        r2 = (i - cx) ** 2 + (j - cy) ** 2
        g = s * np.exp(-r2 / 8.0)
        v[..., 0] += (-(j - cy) * g).astype(np.float32)
        v[..., 1] += ((i - cx) * g).astype(np.float32)
    mask = np.zeros((X, Y), np.uint8)
    e = R.omega_exponent(2 * 10.0 / dx)
    s = R.sample(v, mask, dx, "q", 0.5, e)
    assert s["count"] == 2 and s["components"] == s["passed"] == 2 and s["clipped"] == 0
    out = R.convert(s["raw"], e, dx, X)
    assert sorted(out["sign"].tolist()) == [-1, 1]
    for k in range(2):
        cx = 6.0 if out["sign"][k] == 1 else 18.0
        assert abs(out["x"][k] - cx) < 0.05 and abs(out["y"][k] - 8.0) < 0.05
        assert out["circulation"][k] * out["sign"][k] > 0
    one = R.sample(v, mask, dx, "q", 0.5, e, max_vortices=1)
    assert one["count"] == 1 and one["passed"] == 2 and one["raw"]["label"][0] == s["raw"]["label"].min()
    capped = R.sample(v, mask, dx, "q", 0.5, e, max_components=1)
    assert capped["components"] == 2 and capped["count"] == 1 and capped["dropped_cells"] == s["raw"]["area"][1]
    clip = R.sample(v, mask, dx, "vorticity", 0.5, R.omega_exponent(1.0))
    assert clip["clipped"] > 0 and np.abs(clip["raw"]["sum_q"]).max() > 0
