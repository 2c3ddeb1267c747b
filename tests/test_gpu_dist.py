"""The field distributions on the GPU (csrc/fs_dist.h, host code in csrc/fs_diag.hip, fs/dist.py): every count and every order statistic
exactly against the restatement (tests/dist_ref.py) - integer equality and == on doubles, no tolerance anywhere.

Part one, the histogram: the grid (1030, 262) of tests/vortex_cases.py - five workgroup columns, the last of 6 lanes, a partial last
workgroup down the grid - with the random field (spread) and the rotation field (two bins of about 134,000 cells: the contention case, far
beyond 2^16 per bin), all seven quantities, boxes that cut workgroups on all four sides, planted NaN / Inf / edge values, joint tables, a
deferred limit_field.  Part two, the select: the same fields, ties by the hundred thousand, -0.0, +-Inf, NaN, denormals, the quantile
methods against np.quantile, and the threshold of find_vortices.  Part three, the rider: eager steps, replayed graphs and a resumed run
give identical tables, equal to the sum of one-shot histograms on a twin; the trajectory is unchanged; the refusals."""
import ctypes
import functools
import os

import numpy as np
import pytest
from helpers import diag_floor, make_product, traj_config
from test_gpu_vortices import GOLDEN, _close, _make, _sampled_steps

import dist_ref as D
import vortex_cases as C

pytestmark = pytest.mark.gpu

X, Y, _ = C.TALL
DX = 1.0 / Y
NP_DTYPE = {"f32": "float32", "f64": "float64"}
BOX = (255, 3, 770, 259)             # cuts workgroups on all four sides
ONE = (605, 131, 606, 132)           # one cell, fluid
WGS_16_ROWS = diag_floor(-(-X // 256), Y, 4, 16)
N_STEPS = 20


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _sim(scene, dx, dtype):
    """A simulator on (const, mask) as tests/test_gpu_vortices_large.py builds it; no step is taken."""
    import fs
    const, mask = scene
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask)


def _load(sim, v, p=None):
    """Upload v (and p) -> what the device holds."""
    sim._solver.v.current.from_numpy(np.array(v))
    if p is not None:
        sim._solver.p.current.from_numpy(np.array(p))
    out = sim.field_to_numpy()
    return out["v"], out["p"]


@functools.lru_cache(maxsize=None)
def _pressure(dtype):
    p = np.random.default_rng(9).normal(0, 2, (X, Y)).astype(dtype)
    p.setflags(write=False)
    return p


def _range(x):
    """A range that leaves values on both sides of it (from the restatement's values alone)."""
    x = x[np.isfinite(x)]
    lo, hi = float(np.quantile(x, 0.04)), float(np.quantile(x, 0.93))
    return (lo, hi) if lo < hi else (lo - 1.0, lo + 1.0)


def _assert_hist(got, want, what):
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want["counts"]), (what, int(np.abs(got["counts"] - want["counts"]).sum()))
    for k in ("below", "above", "outside", "nan"):
        if k in want:
            assert got[k] == want[k], (what, k, got[k], want[k])


def _check_histograms(sim, v, p, mask, dx, dtype):
    """Every quantity, B in {1, 63, 64, 4096}, the whole grid and the box; a one-cell box; a box inside the wall."""
    total = 0
    for q in D.QUANTITIES:
        x = D.values(q, v, p, mask, dx)
        rng = _range(x[mask == 0])
        for box in (None, BOX):
            sel = D.selection(mask, box)
            for B in (1, 63, 64, 4096):
                want = D.histogram(x[sel], rng[0], rng[1], B)
                got = sim.histogram(q, B, rng, box=box)
                _assert_hist(got, want, f"{dtype} {q} B={B} box={box}")
                assert got["counts"].sum() + got["below"] + got["above"] + got["nan"] == int(sel.sum())
                assert got["below"] > 0 and got["above"] > 0, "nothing outside the range: the case degraded"
                assert got["quantity"] == q and got["samples"] == 1 and got["box"] == (box or (0, 0, X, Y)) and len(got["edges"]) == B + 1
                total += 1
        assert mask[ONE[0], ONE[1]] == 0
        _assert_hist(sim.histogram(q, 63, rng, box=ONE), D.histogram(x[D.selection(mask, ONE)], rng[0], rng[1], 63), f"{dtype} {q} one cell")
    return total


# ---- part one: the histogram ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_histograms_of_every_quantity_on_the_tall_grid(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.tall_scene(), DX, dtype)
    try:
        assert sim._dev.diag_rows()["flow_stats"] == 4
        v, p = _load(sim, C.random_field(NP_DTYPE[dtype]), _pressure(NP_DTYPE[dtype]))
        assert _check_histograms(sim, v, p, mask, DX, dtype) == 7 * 2 * 4
        # the criterion quantities are fs_vortex_criterion's values bit for bit
        for q in ("q", "swirl"):
            assert np.array_equal(sim.vortex_criterion(q)[mask == 0], D.values(q, v, p, mask, DX)[mask == 0])
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_histograms_with_sixteen_rows_per_workgroup(dtype, hip_lib, monkeypatch):
    monkeypatch.setenv("FS_DIAG_WGS", str(WGS_16_ROWS))
    sim, mask = _sim(C.tall_scene(), DX, dtype)
    try:
        assert sim._dev.diag_rows()["flow_stats"] == 16, "the pass does not take 16 rows per workgroup: the test does not cover it"
        v, p = _load(sim, C.random_field(NP_DTYPE[dtype]), _pressure(NP_DTYPE[dtype]))
        _check_histograms(sim, v, p, mask, DX, dtype)
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rotation_field_two_bins_hold_everything(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.rotation_scene(), C.ROT_DX, dtype)
    try:
        v, p = _load(sim, C.rotation_field(NP_DTYPE[dtype]))
        om = D.values("vorticity", v, p, mask, C.ROT_DX)[mask == 0]
        want = D.histogram(om, -256.0, 256.0, 4096)
        got = sim.histogram("vorticity", 4096, (-256.0, 256.0))
        _assert_hist(got, want, f"rotation {dtype}")
        top = np.sort(got["counts"])[-2:]
        assert (top > 130000).all() and top.sum() > 260000, "the two bins are not that full: the case degraded"
        assert got["counts"][D.bins_of([128.0], -256.0, 256.0, 4096)[0]] == top.max() or got["counts"][D.bins_of([-128.0], -256.0, 256.0, 4096)[0]] == top.max()
        n = int((mask == 0).sum())
        below = sim.histogram("vorticity", 4096, (200.0, 300.0))
        assert below["below"] == n and below["counts"].sum() == 0 and below["above"] == 0
        _assert_hist(below, D.histogram(om, 200.0, 300.0, 4096), "everything below")
        above = sim.histogram("vorticity", 4096, (-300.0, -200.0))
        assert above["above"] == n and above["counts"].sum() == 0 and above["below"] == 0
        _assert_hist(above, D.histogram(om, -300.0, -200.0, 4096), "everything above")
        # a box wholly inside the wall block: all zeros
        wall = (C.ROT_WALL[0].start, C.ROT_WALL[1].start, C.ROT_WALL[0].stop, C.ROT_WALL[1].stop)
        assert (mask[wall[0]:wall[2], wall[1]:wall[3]] != 0).all()
        w = sim.histogram("u", 64, (-100.0, 100.0), box=wall)
        assert w["counts"].sum() == 0 and (w["below"], w["above"], w["nan"]) == (0, 0, 0)
        # ranks just below, at both ends of and inside the run of tied values
        s = np.sort(om)
        lo, hi = int(np.searchsorted(s, 128.0, "left")), int(np.searchsorted(s, 128.0, "right")) - 1
        assert hi - lo > 130000
        ranks = [lo - 1, lo, (lo + hi) // 2, hi] + ([hi + 1] if hi + 1 < len(s) else [])
        out = sim.order_statistics("vorticity", ranks)
        assert out["n"] == len(s) and out["nan"] == 0 and np.array_equal(out["values"], s[ranks]) and out["values"][0] < 128.0
        lo2, hi2 = int(np.searchsorted(s, -128.0, "left")), int(np.searchsorted(s, -128.0, "right")) - 1
        ranks = [0, lo2, hi2, hi2 + 1]
        assert np.array_equal(sim.order_statistics("vorticity", ranks)["values"], s[ranks])
        # every quantity of this field (long runs of ties in each: u and w are multiples of 0.25, q and swirl +-4096 or 0, p is 0)
        for q in D.QUANTITIES:
            for box in (None, BOX):
                sq, nan = D.sorted_values(q, v, p, mask, C.ROT_DX, box)
                m = len(sq)
                ranks = [0, 1, m // 2, m - 2, m - 1]
                out = sim.order_statistics(q, ranks, box=box)
                assert (out["n"], out["nan"]) == (m, nan) and np.array_equal(out["values"], sq[ranks]), (dtype, q, box)
    finally:
        _close(sim)


def _planted(dtype):
    """A small grid with NaN, +-Inf and the edge values of the range (-1, 1) planted in u at fluid cells, and NaN / Inf at wall cells."""
    sim, mask, dx = _make("multi", dtype)
    T = np.dtype(NP_DTYPE[dtype]).type
    v = np.random.default_rng(11).uniform(-0.9, 0.9, mask.shape + (2,)).astype(T)
    fluid = np.argwhere(mask == 0)
    wall = np.argwhere(mask != 0)
    planted = [np.nan, np.inf, -np.inf, np.nextafter(T(1.0), T(0.0)), T(-1.0), T(1.0), np.nextafter(T(-1.0), T(-2.0)), T(0.0), -T(0.0),
               np.finfo(T).tiny / 4, -np.finfo(T).tiny / 4, np.nan, np.inf]
    for k, val in enumerate(planted):
        i, j = fluid[17 + 97 * k]
        v[i, j, 0] = val
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        i, j = wall[5 + 11 * k]
        v[i, j, 0] = val
    return sim, mask, dx, v


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_planted_values(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask, dx, v = _planted(dtype)
    T = np.dtype(NP_DTYPE[dtype]).type
    try:
        v, p = _load(sim, v)
        u = D.values("u", v, p, mask, dx)[mask == 0]
        assert np.isnan(u).sum() == 2 and np.isinf(u).sum() == 3
        for B in (4096, 63):
            want = D.histogram(u, -1.0, 1.0, B)
            got = sim.histogram("u", B, (-1.0, 1.0))
            _assert_hist(got, want, f"planted {dtype} B={B}")
            assert got["nan"] == 2 and got["above"] == 3 and got["below"] == 2          # +Inf twice and hi; -Inf and nextafter(lo, -inf)
            assert got["counts"][B - 1] >= 1 and got["counts"][0] >= 1                 # nextafter(hi, 0) by the clamp (f64); lo itself
        # the quantities that read the neighbours see the planted values too: NaN and Inf spread, and are counted, not dropped
        for q in ("speed", "vorticity", "q", "swirl"):
            x = D.values(q, v, p, mask, dx)[mask == 0]
            assert np.isnan(x).any()
            _assert_hist(sim.histogram(q, 64, (-50.0, 50.0)), D.histogram(x, -50.0, 50.0, 64), f"planted {dtype} {q}")
        # the select: +-Inf are values, NaN is counted apart, the denormals and both zeros keep their places
        s = np.sort(u[~np.isnan(u)])
        n = len(s)
        out = sim.order_statistics("u", [0, 1, 2, n // 2, n - 3, n - 2, n - 1])
        assert (out["n"], out["nan"]) == (n, 2)
        assert np.array_equal(out["values"], s[[0, 1, 2, n // 2, n - 3, n - 2, n - 1]])
        assert out["values"][0] == -np.inf and out["values"][-1] == np.inf and out["values"][-2] == np.inf
        z = int(np.searchsorted(s, 0.0, "left"))
        ranks = [z - 2, z - 1, z, z + 1, z + 2, z + 3]             # a value, the negative denormal, both zeros, the positive denormal, a value
        got = sim.order_statistics("u", ranks)["values"]
        tiny = float(np.finfo(T).tiny)
        assert np.array_equal(got, s[ranks]) and (got[2:4] == 0.0).all() and -tiny < got[1] < 0 < got[4] < tiny and got[0] < -tiny and got[5] > tiny
        with pytest.raises(ValueError, match="infinite|finite"):
            sim.histogram("u", 16)                                                     # range=None with infinite extremes
    finally:
        _close(sim)


def test_field_of_zeros_with_negative_zero(hip_lib):
    sim, mask, dx = _make("odd", "f32")
    try:
        v = np.zeros(mask.shape + (2,), np.float32)
        fluid = np.argwhere(mask == 0)
        for i, j in fluid[::7]:
            v[i, j, 0] = -0.0
        v, p = _load(sim, v)
        assert np.signbit(v[..., 0]).sum() == len(fluid[::7])
        n = int((mask == 0).sum())
        out = sim.order_statistics("u", [0, len(fluid[::7]) - 1, len(fluid[::7]), n - 1])
        assert out["n"] == n and (out["values"] == 0.0).all()
        assert np.signbit(out["values"]).tolist() == [True, True, False, False]         # (-0.0 sorts first: distinct keys, equal values)
        h = sim.histogram("u", 8, (0.0, 1.0))
        assert h["counts"][0] == n and h["below"] == 0
        assert sim.quantile("u", 0.5) == 0.0
        with pytest.raises(ValueError, match="narrow"):
            sim.histogram("u", 8)                  # range=None on a constant field: [0, 5e-324) is too narrow for a finite bins / (hi - lo)
    finally:
        _close(sim)


def test_joint_tables(hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.tall_scene(), DX, "f32")
    try:
        v, p = _load(sim, C.random_field("float32"), _pressure("float32"))
        for box in (None, BOX):
            got = sim.histogram("u", 64, (-0.9, 0.95), box=box, against={"quantity": "w", "bins": 64, "range": (-1.0, 0.5)})
            want = D.field_joint("u", "w", v, p, mask, DX, (-0.9, 0.95, 64), (-1.0, 0.5, 64), box)
            assert got["counts"].shape == (64, 64) and got["quantity"] == ("u", "w") and len(got["edges_b"]) == 65
            _assert_hist(got, want, f"(u, w) box={box}")
            assert got["outside"] > 0 and got["counts"].sum() + got["outside"] + got["nan"] == int(D.selection(mask, box).sum())
        qv = D.values("q", v, p, mask, DX)[mask == 0]
        med = float(np.median(qv))
        ra, rb = (-600.0, 600.0, 8), (med, float(qv.max()) + 1.0, 512)                  # the second side leaves out half the cells
        got = sim.histogram("vorticity", 8, ra[:2], against={"quantity": "q", "bins": 512, "range": rb[:2]})
        want = D.field_joint("vorticity", "q", v, p, mask, DX, ra, rb)
        _assert_hist(got, want, "(vorticity, q)")
        assert got["counts"].shape == (8, 512) and abs(got["outside"] - len(qv) // 2) < len(qv) // 50
        assert (got["counts"].sum(axis=1) > 0).sum() > 2 and (got["counts"].sum(axis=0) > 0).sum() > 20
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_tables_and_the_select(hip_lib):
    """The case tests/test_gpu_vortices.py uses: the MAC solver's end-of-step limit_field is deferred, and the flag is up."""
    import fs
    from fs.solver import VELOCITY_LIMIT
    g = np.load(os.path.join(GOLDEN, "traj_bc1_upwind_vc0.npz"))
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, traj_config(g))
    dev = sim._dev
    try:
        mask = g["bc_mask"]
        i = np.arange(mask.shape[0])[:, None] * np.ones(mask.shape[1])[None, :]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[..., 0] = 3.0 * VELOCITY_LIMIT * np.sin(i / 3.0)
        v[..., 1] = -2.0 * VELOCITY_LIMIT * np.cos(i / 5.0)
        v[mask != 0] = 0
        sim._solver.v.current.from_numpy(v)
        dx = sim._solver.dx
        sim.start_distributions([{"quantity": "speed", "bins": 128, "range": (0.0, 10.5)},
                                 {"quantity": "u", "bins": 64, "range": (-10.0, 10.0), "against": {"quantity": "vorticity", "bins": 64, "range": (-500.0, 500.0)}}])
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        ranks = [0, 10, 100]
        got = {q: sim.histogram(q, 128, r) for q, r in (("speed", (0.0, 10.5)), ("u", (-10.0, 10.0)), ("w", (-10.0, 10.0)), ("q", (-1e4, 1e4)))}
        sel = {q: sim.order_statistics(q, ranks) for q in ("speed", "vorticity")}
        top = sim.quantile("speed", 1.0)
        rider = sim.distributions()
        assert cur.pending_limit is not None, "reading the tables flushed the owed pass"
        down = sim.field_to_numpy()                           # (the download launches the owed pass first)
        speed = np.hypot(down["v"][..., 0], down["v"][..., 1])
        assert speed.max() > 0.99 * VELOCITY_LIMIT, "no cell at the limit: the owed pass changed nothing and the test does not cover it"
        for q, r in (("speed", (0.0, 10.5)), ("u", (-10.0, 10.0)), ("w", (-10.0, 10.0)), ("q", (-1e4, 1e4))):
            _assert_hist(got[q], D.field_histogram(q, down["v"], down["p"], mask, dx, 128, r), f"deferred {q}")
        for q in sel:
            s, _ = D.sorted_values(q, down["v"], down["p"], mask, dx)
            assert np.array_equal(sel[q]["values"], s[ranks]), q
        assert top == D.sorted_values("speed", down["v"], down["p"], mask, dx)[0][-1]
        _assert_hist(rider[0], D.field_histogram("speed", down["v"], down["p"], mask, dx, 128, (0.0, 10.5)), "deferred rider speed")
        _assert_hist(rider[1], D.field_joint("u", "vorticity", down["v"], down["p"], mask, dx, (-10.0, 10.0, 64), (-500.0, 500.0, 64)), "deferred rider joint")
    finally:
        _close(sim)


# ---- part two: the select ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_order_statistics_of_every_quantity(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.tall_scene(), DX, dtype)
    try:
        v, p = _load(sim, C.random_field(NP_DTYPE[dtype]), _pressure(NP_DTYPE[dtype]))
        for q in D.QUANTITIES:
            for box in (None, BOX):
                s, nan = D.sorted_values(q, v, p, mask, DX, box)
                n = len(s)
                ranks = [0, 1, n // 2, n - 2, n - 1]
                out = sim.order_statistics(q, ranks, box=box)
                assert (out["n"], out["nan"]) == (n, nan) and out["values"].dtype == np.float64
                assert np.array_equal(out["values"], s[ranks]), (dtype, q, box, out["values"], s[ranks])
            s, _ = D.sorted_values(q, v, p, mask, DX)
            n = len(s)
            eight = [0, 7, n // 5, n // 3, n // 2, n // 2 + 1, n - 9, n - 1]
            assert np.array_equal(sim.order_statistics(q, eight)["values"], s[eight]), (dtype, q, "eight ranks")
            twice = [n // 4, n // 4, n // 4 + 1]
            assert np.array_equal(sim.order_statistics(q, twice)["values"], s[twice]), (dtype, q, "equal ranks")
        s, _ = D.sorted_values("u", v, p, mask, DX, ONE)
        assert sim.order_statistics("u", [0], box=ONE)["values"].tolist() == s.tolist()
        # no ranks: the counts alone
        out = sim.order_statistics("p", ())
        assert out["n"] == int((mask == 0).sum()) and len(out["values"]) == 0
    finally:
        _close(sim)


def test_quantiles_and_the_threshold_of_find_vortices(hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.tall_scene(), DX, "f32")
    try:
        v, p = _load(sim, C.random_field("float32"), _pressure("float32"))
        qs = [0.0, 0.1, 0.5, 0.85, 0.9, 1.0]
        for name in ("q", "speed", "p"):
            x, _ = D.sorted_values(name, v, p, mask, DX)
            for method in ("lower", "higher"):
                got = sim.quantile(name, qs, method=method)
                want = np.quantile(x, qs, method=method)
                assert got.dtype == np.float64 and np.array_equal(got, want), (name, method, got, want)
                for q in qs:
                    assert sim.quantile(name, q, method=method) == np.quantile(x, q, method=method)
            n = len(x)
            for q in qs + [1 / 3]:
                pos = (n - 1) * q
                k = int(np.floor(pos))
                a, b, g = x[k], x[min(k + 1, n - 1)], pos - k
                assert sim.quantile(name, q) == a + (b - a) * g, (name, q)
                assert sim.quantile(name, q, method="nearest") == (a if g <= 0.5 else b)
            xb, _ = D.sorted_values(name, v, p, mask, DX, BOX)
            assert sim.quantile(name, 0.9, box=BOX, method="lower") == np.quantile(xb, 0.9, method="lower")
        # the threshold every caller of find_vortices took from a download and np.quantile: the same sample either way
        c = sim.vortex_criterion("q")
        host = float(np.quantile(c[mask == 0], 0.85))
        mine = sim.quantile("q", 0.85)
        a = sim.find_vortices(mine, "q")
        b = sim.find_vortices(host, "q")
        assert a["count"][0] > 0 and a["components"][0] == b["components"][0]
        for k in a["raw"]:
            assert np.array_equal(a["raw"][k], b["raw"][k]), k
        # range=None: the exact extremes give the range, nothing falls outside it
        x, _ = D.sorted_values("speed", v, p, mask, DX)
        h = sim.histogram("speed", 63)
        assert h["edges"][0] == x[0] and h["edges"][-1] == np.nextafter(x[-1], np.inf) and (h["below"], h["above"], h["nan"]) == (0, 0, 0)
        _assert_hist(h, D.histogram(x, x[0], np.nextafter(x[-1], np.inf), 63), "range=None")
        assert h["counts"][-1] >= 1 and h["counts"].sum() == len(x)
    finally:
        _close(sim)


# ---- part three: the rider ----------------------------------------------------------------------------------------------------------------------
CHANNELS = [{"quantity": "speed", "bins": 100, "range": (0.0, 1.5)},
            {"quantity": "u", "bins": 32, "range": (-0.5, 1.5), "box": (3, 2, 30, 18), "against": {"quantity": "vorticity", "bins": 128, "range": (-20.0, 20.0)}}]
EVERY, START = 2, 3


def _one_shots(sim):
    return [sim.histogram("speed", 100, (0.0, 1.5)),
            sim.histogram("u", 32, (-0.5, 1.5), box=(3, 2, 30, 18), against={"quantity": "vorticity", "bins": 128, "range": (-20.0, 20.0)})]


@functools.lru_cache(maxsize=None)
def _twin_tables(grid, dtype):
    """The one-shot histograms after each eager step of a twin without the rider, and its final fields; computed once, never changed."""
    b, _, _ = _make(grid, dtype)
    try:
        out = []
        for _ in range(N_STEPS):
            b.step()
            out.append(_one_shots(b))
        return out, b.field_to_numpy()
    finally:
        _close(b)


def _assert_tables(got, twin, steps, what):
    for c in range(2):
        want = sum(twin[s - 1][c]["counts"] for s in steps)
        assert np.array_equal(got[c]["counts"], want), (what, c)
        for k in ("below", "above", "outside", "nan"):
            if k in got[c]:
                assert got[c][k] == sum(twin[s - 1][c][k] for s in steps), (what, c, k)
        assert got[c]["samples"] == len(steps) and got[c]["sample_steps"].tolist() == steps, (what, got[c]["sample_steps"], steps)
    assert got[0]["counts"].sum() > 0 and got[1]["counts"].sum() > 0 and (got[0]["counts"] > 0).sum() > 3, "the tables are empty: the test covers nothing"


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rider_eager_graph_and_resumed_give_the_sum_of_one_shots(dtype, hip_lib):
    twin, final = _twin_tables("scene1", dtype)
    steps = _sampled_steps(N_STEPS, EVERY, START)
    tables = {}
    for mode in ("eager", "graph", "resumed"):
        a, _, _ = _make("scene1", dtype)
        try:
            a.start_distributions(CHANNELS, every=EVERY, start_step=START)
            if mode == "eager":
                for _ in range(N_STEPS):
                    a.step()
            elif mode == "graph":
                a.run(N_STEPS, graph=True)
                assert a._graphs, "the run replayed no graph"
            else:
                a.run(9, graph=False)
                z = {k: np.array(x) for k, x in a._distr.checkpoint().items()}
                assert int(z["dist.launches"]) == 9 and int(z["dist.samples"]) == 3
                a.stop_distributions()
                a.start_distributions(CHANNELS[:1], every=EVERY, start_step=START)
                with pytest.raises(ValueError, match="channels"):
                    a._distr.restore(z)                              # other channels: refused before any device work
                a.stop_distributions()
                a.start_distributions(CHANNELS, every=EVERY, start_step=START + 1)
                with pytest.raises(ValueError, match="every"):
                    a._distr.restore(z)
                a.stop_distributions()
                a.start_distributions(CHANNELS, every=EVERY, start_step=START)
                a._distr.restore(z)
                a.run(N_STEPS - 9, graph=False)
            got = a.distributions()
            _assert_tables(got, twin, steps, f"{dtype} {mode}")
            tables[mode] = got
            fa = a.field_to_numpy()
            for k in fa:
                assert np.array_equal(fa[k], final[k]), f"{mode}: {k}: the rider changed the trajectory"
            if mode == "eager":
                a.reset_distributions()
                zero = a.distributions()
                assert zero[0]["counts"].sum() == 0 and zero[1]["outside"] == 0 and zero[0]["samples"] == 0
                a.step()                                             # step 21 samples: 21 - 3 = 9 * 2
                again, now = a.distributions(), _one_shots(a)
                assert again[0]["samples"] == 1 and again[0]["sample_steps"].tolist() == [21] and again[0]["counts"].sum() > 0
                for c in range(2):
                    _assert_hist(again[c], now[c], "after the reset")
            a.stop_distributions()
            assert a._distr is None
            with pytest.raises(RuntimeError):
                a.distributions()
        finally:
            _close(a)
    for mode in ("graph", "resumed"):
        for c in range(2):
            assert np.array_equal(tables[mode][c]["counts"], tables["eager"][c]["counts"])


def test_fields_are_bit_identical_with_every_other_rider_attached(hip_lib):
    def run(with_dist):
        a, mask, dx = _make("scene1", "f32")
        try:
            a.record_history(probes=[(5, 5)], every=1)
            a.start_averaging(every=2)
            a.start_pod(4, every=3)
            a.track_vortices(1.0, "q", every=2)
            if with_dist:
                a.start_distributions(CHANNELS, every=1)
                toks = [t for r in a._riders() for t in r.tokens()]
                kinds = [t[0] for t in toks]
                assert kinds.index("pod") < kinds.index("dist") < kinds.index("vortices"), kinds
            a.run(N_STEPS, graph=True)
            assert a._graphs, "the run replayed no graph"
            if with_dist:
                d = a.distributions()
                assert d[0]["samples"] == N_STEPS and d[0]["counts"].sum() + d[0]["below"] + d[0]["above"] + d[0]["nan"] == N_STEPS * int((mask == 0).sum())
            return a.field_to_numpy()
        finally:
            _close(a)
    with_, without = run(True), run(False)
    for k in with_:
        assert np.array_equal(with_[k], without[k]), k


def test_refusals(hip_lib):
    from fs import _lib
    sim, mask, dx = _make("scene1", "f32")
    dev = sim._dev
    ok = {"quantity": "u", "bins": 8, "range": (0.0, 1.0)}
    try:
        n = int((mask == 0).sum())
        for bad, msg in ((dict(ok, quantity="nope"), "quantity"), (dict(ok, bins=0), "bins"), (dict(ok, bins=4097), "bins"),
                         (dict(ok, against={"quantity": "w", "bins": 513, "range": (0, 1)}), "joint"), (dict(ok, range=(1.0, 1.0)), "lo < hi"),
                         (dict(ok, range=(2.0, 1.0)), "lo < hi"), (dict(ok, range=(0.0, float("inf"))), "finite"),
                         (dict(ok, range=(float("nan"), 1.0)), "finite"), ([ok] * 5, "channels"), (dict(ok, box=(0, 0, 10 ** 6, 2)), "box")):
            with pytest.raises(ValueError, match=msg):
                sim.start_distributions(bad)
        assert sim._distr is None
        with pytest.raises(ValueError, match="quantity"):
            sim.histogram("nope", 8, (0, 1))
        with pytest.raises(ValueError, match="ranks"):
            sim.order_statistics("u", list(range(9)))
        for ranks in ([n], [0, n + 5]):
            with pytest.raises(ValueError, match="rank"):
                sim.order_statistics("u", ranks)
        with pytest.raises(ValueError):
            sim.quantile("u", 1.5)
        with pytest.raises(ValueError, match="method"):
            sim.quantile("u", 0.5, method="cubic")
        with pytest.raises(ValueError, match="joint"):
            sim.histogram("u", 8, against={"quantity": "w", "bins": 8, "range": (0, 1)})
        with pytest.raises(RuntimeError):
            sim.distributions()
        sim.start_distributions(ok)
        with pytest.raises(RuntimeError, match="attached"):
            sim.start_distributions(ok)
        # during a capture: everything but the launch and the stop
        for call in (sim.distributions, sim.reset_distributions, lambda: sim.histogram("u", 8, (0, 1)), lambda: sim.quantile("u", 0.5),
                     lambda: sim.order_statistics("u", [0]), lambda: sim.start_distributions(ok)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        d = sim._distr.dist
        h, box = d._h, (ctypes.c_int * 4)(0, 0, mask.shape[0], mask.shape[1])
        v, p = sim._solver.get_fields()[:2]
        ll = ctypes.c_longlong
        r, out, nn, nan = (ll * 1)(0), (ctypes.c_double * 1)(), ll(), ll()
        for call in (lambda: _lib.call("fs_dist_read", dev._ctx, h, 0, None, None, None, None), lambda: _lib.call("fs_dist_reset", dev._ctx, h),
                     lambda: _lib.call("fs_dist_select", dev._ctx, 0, box, 0.0, dx, v._h, p._h, r, 1, out, ctypes.byref(nn), ctypes.byref(nan))):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        # the library's own argument checks
        from fs.ride_ops import _DistSpec
        hh = ctypes.c_void_p()

        def create(ctx, nchan=1, **kw):
            s = (_DistSpec * 4)()
            for k in range(4):
                s[k].quantity, s[k].bins, s[k].quantity_b, s[k].bins_b, s[k].lo, s[k].hi, s[k].lo_b, s[k].hi_b = 0, 8, -1, 0, 0.0, 1.0, 0.0, 1.0
                s[k].box[:] = (0, 0, 4, 4)
                for name, val in kw.items():
                    if name == "box":
                        s[k].box[:] = val
                    else:
                        setattr(s[k], name, val)
            return dev._lib.fs_dist_create(ctx, nchan, ctypes.cast(s, ctypes.c_void_p), 1, 0, ctypes.byref(hh))
        assert create(dev._ctx) == 0 and hh.value
        _lib.call("fs_dist_free", dev._ctx, hh)
        with pytest.raises(_lib.FsError, match="freed"):
            _lib.call("fs_dist_reset", dev._ctx, hh)                      # a stale handle
        hh = ctypes.c_void_p()
        for kw in (dict(nchan=0), dict(nchan=5), dict(quantity=7), dict(quantity=-1), dict(bins=0), dict(bins=4097), dict(lo=1.0), dict(lo=2.0),
                   dict(hi=float("inf")), dict(lo=float("nan")), dict(lo=-1e308, hi=1e308), dict(hi=5e-324), dict(quantity_b=1, bins_b=513),
                   dict(quantity_b=1, bins_b=0), dict(quantity_b=7, bins_b=2), dict(quantity_b=1, bins_b=2, lo_b=1.0), dict(box=(0, 0, 0, 4)),
                   dict(box=(0, 0, 4, 10 ** 6)), dict(box=(-1, 0, 4, 4))):
            assert create(dev._ctx, **kw) == -1 and not hh.value, kw      # FS_ERR_ARG
            assert dev._lib.fs_last_error()
        r9 = (ll * 9)(*range(9))
        o9 = (ctypes.c_double * 9)()
        sel = lambda rr, k: dev._lib.fs_dist_select(dev._ctx, 0, box, 0.0, dx, v._h, p._h, rr, k, o9, ctypes.byref(nn), ctypes.byref(nan))
        assert sel(r9, 9) == -1 and "RANKS" in dev._lib.fs_last_error().decode()
        assert sel((ll * 2)(5, 4), 2) == -1 and "ascending" in dev._lib.fs_last_error().decode()
        assert sel((ll * 1)(n), 1) == -1 and "rank" in dev._lib.fs_last_error().decode() and nn.value == n
        assert sel((ll * 1)(n - 1), 1) == 0
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert create(slab) == -5 and not hh.value                   # FS_ERR_UNSUPPORTED
            assert "slab" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)

        class _Slab:
            nranks, capturing = 2, False
        from fs.runtime import DeviceBase
        with pytest.raises(_lib.FsError, match="single-GPU"):
            DeviceBase.dist_create(_Slab(), ok)
        with pytest.raises(_lib.FsError, match="single-GPU"):
            DeviceBase.dist_select(_Slab(), "u", None, dx, None, None, [0])
    finally:
        _close(sim)
