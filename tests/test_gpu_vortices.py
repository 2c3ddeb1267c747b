"""Vortex identification on the GPU (csrc/fs_vortex.h, include/fs_hip.h fs_vortex_*, FluidSimulator.track_vortices / find_vortices): the
labelling primitive on uploaded flag planes against the breadth-first search of tests/vortex_ref.py, exactly; the criterion field bit for bit
for the three criteria in f32 and f64; the whole pipeline - every integer of every record, the counters, the planes and the derived floats -
exactly against the restatement, with both caps biting, a clipped field and min_area at its boundary; the rider in eager steps and replayed
graphs against find_vortices on an eagerly stepped twin, with the ring wrapped, a cadence, an unchanged trajectory, a resumed run and the
deferred limit pass; the refusals.

Grids, by the geometry of the kernels (tiles of 32 x 8 cells in k_vortex_local, 256 columns x 4-row groups in k_vortex_flags, 1024 cells
per workgroup in the compression and id passes): scene 1 at res 20 (40 x 20); (37, 12) - odd X, a partial second tile each way; (1030, 8) -
past four 256-column blocks and 32 tiles with a partial last one, one tile row, a 9th block of the id pass; (300, 70) - more than one tile and
more than one block each way, neither extent a multiple of the tile, 21 blocks of the id pass; (102, 13) with FS_DIAG_WGS=1 - the flag pass
takes all 13 rows in one workgroup: three full row groups and a partial one (on the others it takes 4 rows per workgroup).  The forms the
kernels take only on large grids - several blocks per lane of the scans, wrapped counter slots, sums near their bounds, 16 rows per
workgroup of the flag pass, the full ring - are in tests/test_gpu_vortices_large.py on (1030, 262)."""
import ctypes
import functools
import os

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config

import vortex_ref as R

pytestmark = pytest.mark.gpu

N_STEPS = 20      # (run(graph=True) captures from 16 steps on)
GRIDS = {"scene1": None, "odd": (37, 12, 0.3), "wide": (1030, 8, 0.15), "multi": (300, 70, 0.15), "rows": (102, 13, 0.15)}
LABEL_GRIDS = ("odd", "wide", "multi")
CRITERIA = ("q", "swirl", "vorticity")
HEAD = ("components", "passed", "count", "clipped", "dropped_cells")
FLOATS = ("sign", "circulation", "x", "y", "xg", "yg", "peak_omega", "peak_cell", "bbox")


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _close(sim):
    sim._solver._bc.device.close()


def _diag_env(grid, monkeypatch):
    if grid == "rows":
        monkeypatch.setenv("FS_DIAG_WGS", "1")
    else:
        monkeypatch.delenv("FS_DIAG_WGS", raising=False)


def _scene(grid):
    if GRIDS[grid] is None:
        from fs.boundary_condition import create_scene_arrays
        const, mask, _ = create_scene_arrays(1, 20)
        return const, mask, 1.0 / 20
    from multigrid_cases import scene
    X, Y, wall_p = GRIDS[grid]
    const, mask = scene(X, Y, wall_p)
    return const, mask, 1.0 / Y


def _make(grid, dtype):
    """A running flow on the grid, as tests/test_gpu_pod.py builds it: the upwind MAC solver (any width) with two red-black iterations."""
    import fs
    const, mask, dx = _scene(grid)
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask), dx


@functools.lru_cache(maxsize=None)
def _twin(grid, dtype):
    """The velocity after each of N_STEPS eager steps of a simulator without the rider, and its final fields: computed once per grid and
    dtype, shared, never changed."""
    b, _, _ = _make(grid, dtype)
    try:
        out = []
        for _ in range(N_STEPS):
            b.step()
            out.append(b.field_to_numpy()["v"])
        for v in out:
            assert np.isfinite(v).all(), "the flow of the test blew up"
        return out, b.field_to_numpy()
    finally:
        _close(b)


@functools.lru_cache(maxsize=None)
def _threshold(grid, dtype, which):
    """A quantile of the restatement's criterion over the fluid cells of the last step - the highest of 0.85, 0.7, 0.5, 0.3 at which the
    restatement finds at least two components of 4 cells in the last step (on the small random masks the flagged cells of a high quantile
    are scattered singles)."""
    _, mask, dx = _scene(grid)
    v = _twin(grid, dtype)[0][-1]
    c, _ = R.criterion(which, v, mask, dx)
    for quantile in (0.85, 0.7, 0.5, 0.3):
        thr = float(np.quantile(c[np.asarray(mask) == 0], quantile))
        if R.sample(v, mask, dx, which, thr, _exponent(dx))["count"] >= 2:
            return thr
    raise AssertionError(f"{grid} {dtype} {which}: no quantile leaves two components of 4 cells: the tests would cover nothing")


def _exponent(dx):
    return R.omega_exponent(2.0 * 10.0 / dx)


def _assert_sample(out, k, ref, e, dx, nx, what):
    """Sample k of a vortices() / find_vortices() result against a restatement sample: every integer, then the floats bit for bit."""
    for name in HEAD:
        assert int(out[name][k]) == ref[name], (what, name, int(out[name][k]), ref[name])
    m = out["sample"] == k
    for name in R.RECORD:
        assert np.array_equal(out["raw"][name][m], ref["raw"][name]), (what, name, out["raw"][name][m], ref["raw"][name])
    conv = R.convert(ref["raw"], e, dx, nx)
    for name in FLOATS:
        assert out[name][m].dtype == conv[name].dtype and np.array_equal(out[name][m], conv[name]), (what, name)
    assert np.array_equal(out["label"][m], ref["raw"]["label"]) and np.array_equal(out["area"][m], ref["raw"]["area"])


# ---- the labelling primitive ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", LABEL_GRIDS)
def test_labels_of_uploaded_flag_planes_equal_the_search(grid, hip_lib):
    sim, mask, _ = _make(grid, "f32")
    try:
        X, Y = mask.shape
        for name, flags in R.patterns(X, Y).items():
            want = R.label_plane(flags)
            got = sim._dev.vortex_label(flags)
            assert got.dtype == np.int32 and got.shape == (X, Y)
            assert np.array_equal(got, want), f"{grid} {name}: {(got != want).sum()} labels differ"
            if name == "serpentine":
                assert set(np.unique(want)) == {-1, 0}
            if name == "random_one_sign" and grid == "multi":
                ids, counts = np.unique(want[want >= 0], return_counts=True)
                big = want == ids[np.argmax(counts)]
                assert big[0].any() and big[-1].any() and big[:, 0].any() and big[:, -1].any(), "no spanning component: the case degraded"
        # any non-zero byte is a flag, and only equal bytes join
        flags = np.full((X, Y), 7, np.uint8)
        flags[X // 2:] = 200
        assert np.array_equal(sim._dev.vortex_label(flags), R.label_plane(flags))
    finally:
        _close(sim)


# ---- the criterion field ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_criterion_field_bit_for_bit(grid, dtype, hip_lib, monkeypatch):
    _diag_env(grid, monkeypatch)
    sim, mask, dx = _make(grid, dtype)
    try:
        for _ in range(N_STEPS):
            sim.step()
        v = sim.field_to_numpy()["v"]
        assert np.array_equal(v, _twin(grid, dtype)[0][-1])
        for which in CRITERIA:
            want, _ = R.criterion(which, v, mask, dx)
            got = sim.vortex_criterion(which)
            assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), f"{grid} {dtype} {which}: {(got != want).sum()} cells differ"
            assert np.abs(want).max() > 0 and np.all(got[mask != 0] == 0)
    finally:
        _close(sim)


# ---- the whole pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_find_vortices_equals_the_restatement(grid, dtype, hip_lib, monkeypatch):
    _diag_env(grid, monkeypatch)
    sim, mask, dx = _make(grid, dtype)
    try:
        X = mask.shape[0]
        for _ in range(N_STEPS):
            sim.step()
        v = sim.field_to_numpy()["v"]
        e = _exponent(dx)
        for which in CRITERIA:
            thr = _threshold(grid, dtype, which)
            ref = R.sample(v, mask, dx, which, thr, e)
            assert ref["count"] >= 2 and (ref["raw"]["sum_q"] != 0).any(), f"{grid} {which}: no vortex found: the test covers nothing"
            out = sim.find_vortices(thr, which)
            assert out["exponent"] == e and len(out["step"]) == 1
            what = f"{grid} {dtype} {which}"
            _assert_sample(out, 0, ref, e, dx, X, what)
            planes = sim.vortex_labels()
            assert np.array_equal(planes["flags"], ref["flags"]) and np.array_equal(planes["labels"], ref["labels"]), what
        # both caps bite: the kept ones are those of smallest label
        thr = _threshold(grid, dtype, "q")
        full = R.sample(v, mask, dx, "q", thr, e, min_area=1, max_vortices=1 << 20)
        assert full["components"] > 3 and full["passed"] == full["count"] == full["components"]
        ref = R.sample(v, mask, dx, "q", thr, e, min_area=1, max_vortices=2, max_components=3)
        assert ref["count"] == 2 and ref["dropped_cells"] > 0 and np.array_equal(ref["raw"]["label"], full["raw"]["label"][:2])
        _assert_sample(sim.find_vortices(thr, "q", min_area=1, max_vortices=2, max_components=3), 0, ref, e, dx, X, "caps")
        # min_area at the boundary: the area of the largest component passes, one more does not
        top = int(full["raw"]["area"].max())
        for min_area in (top, top + 1):
            ref = R.sample(v, mask, dx, "q", thr, e, min_area=min_area)
            assert ref["passed"] == (int((full["raw"]["area"] == top).sum()) if min_area == top else 0)
            _assert_sample(sim.find_vortices(thr, "q", min_area=min_area), 0, ref, e, dx, X, f"min_area {min_area}")
    finally:
        _close(sim)


def test_clipped_counts_the_cells_beyond_omega_max(hip_lib):
    sim, mask, dx = _make("odd", "f32")
    try:
        X, Y = mask.shape
        v = np.random.default_rng(5).uniform(-1, 1, (X, Y, 2)).astype(np.float32)
        sim._solver.v.current.from_numpy(v)
        v = sim.field_to_numpy()["v"]
        omega_max = 4.0
        e = R.omega_exponent(omega_max)
        ref = R.sample(v, mask, dx, "vorticity", 1.0, e, min_area=1)
        assert ref["clipped"] > 0 and ref["count"] > 0
        out = sim.find_vortices(1.0, "vorticity", min_area=1, omega_max=omega_max)
        assert out["exponent"] == e == 2
        _assert_sample(out, 0, ref, e, dx, X, "clipped")
        assert (np.abs(out["peak_omega"]) == 4.0).any(), "no peak at the clamp"
    finally:
        _close(sim)


# ---- the rider ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin_samples(grid, dtype, which):
    """find_vortices after each eager step of a twin without the rider -> (threshold, [result per step])."""
    thr = _threshold(grid, dtype, which)
    b, _, _ = _make(grid, dtype)
    try:
        out = []
        for _ in range(N_STEPS):
            b.step()
            out.append(b.find_vortices(thr, which))
        return thr, out
    finally:
        _close(b)


def _sampled_steps(n, every, start):
    return [k for k in range(1, n + 1) if k > start and (k - start) % every == 0]


def _assert_equals_twin(out, steps, twin, what):
    assert out["step"].tolist() == steps, (what, out["step"], steps)
    for k, step in enumerate(steps):
        t = twin[step - 1]
        for name in HEAD:
            assert out[name][k] == t[name][0], (what, step, name)
        m = out["sample"] == k
        for name in R.RECORD:
            assert np.array_equal(out["raw"][name][m], t["raw"][name]), (what, step, name)
        for name in FLOATS:
            assert np.array_equal(out[name][m], t[name]), (what, step, name)
    assert sum(int(c) for c in out["count"]) > 0, "no vortex in any sample: the test covers nothing"


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("grid,dtype", [("scene1", "f32"), ("scene1", "f64"), ("odd", "f32"), ("multi", "f32")])
def test_rider_equals_find_vortices_on_a_twin_and_leaves_the_trajectory(grid, dtype, graph, hip_lib):
    thr, twin = _twin_samples(grid, dtype, "q")
    _, final = _twin(grid, dtype)
    _, mask, dx = _scene(grid)
    # every step into a ring of 4 (it wraps: run() cuts and drains, eager steps drain when it is full); a cadence with a start
    for every, start, capacity in ((1, 0, 4), (3, 2, None)):
        a, _, _ = _make(grid, dtype)
        try:
            a.track_vortices(thr, "q", every=every, start_step=start, capacity=capacity)
            if graph:
                a.run(N_STEPS, graph=True)
                assert a._graphs or capacity is not None, "the run replayed no graph"
            else:
                for _ in range(N_STEPS):
                    a.step()
            out = a.vortices()
            what = f"{grid} {dtype} every={every} start={start} graph={graph}"
            _assert_equals_twin(out, _sampled_steps(N_STEPS, every, start), twin, what)
            assert np.allclose(out["time"], out["step"] * a._solver.dt)
            # the planes are those of the last sample; the last sample against the restatement itself
            last = _sampled_steps(N_STEPS, every, start)[-1]
            ref = R.sample(_twin(grid, dtype)[0][last - 1], mask, dx, "q", thr, _exponent(dx))
            planes = a.vortex_labels()
            assert np.array_equal(planes["flags"], ref["flags"]) and np.array_equal(planes["labels"], ref["labels"]), what
            _assert_sample(out, len(out["step"]) - 1, ref, _exponent(dx), dx, mask.shape[0], what)
            fa = a.field_to_numpy()
            for k in fa:
                assert np.array_equal(fa[k], final[k]), f"{what}: {k}: the rider changed the trajectory"
            a.stop_vortices()
            assert a._vortexr is None and np.array_equal(a.vortices()["raw"]["sum_q"], out["raw"]["sum_q"])      # kept after the stop
            assert np.array_equal(a.vortex_labels()["labels"], ref["labels"])
        finally:
            _close(a)


def test_graph_replays_the_sequence_and_the_ring_wraps(hip_lib):
    """run(graph=True) with a ring larger than the run: one uncut chunk, graphs replayed; then a ring of 2 under run(): cut and drained."""
    thr, twin = _twin_samples("scene1", "f32", "q")
    a, _, _ = _make("scene1", "f32")
    try:
        a.track_vortices(thr, every=2)
        a.run(N_STEPS, graph=True)
        assert a._graphs, "the run replayed no graph"
        _assert_equals_twin(a.vortices(), _sampled_steps(N_STEPS, 2, 0), twin, "graph, every=2")
    finally:
        _close(a)
    a, _, _ = _make("scene1", "f32")
    try:
        a.track_vortices(thr, capacity=2)
        a.run(N_STEPS, graph=True)
        _assert_equals_twin(a.vortices(), list(range(1, N_STEPS + 1)), twin, "ring of 2")
    finally:
        _close(a)


def test_resumed_run_gives_the_same_records(hip_lib):
    thr, twin = _twin_samples("odd", "f32", "q")
    a, _, _ = _make("odd", "f32")
    try:
        a.track_vortices(thr, every=3, start_step=1)
        a.run(10, graph=False)
        z = a._vortexr.checkpoint()
        assert int(z["vortex.launches"]) == 10 and len(z["vortex.words"]) == 3
        a.stop_vortices()
        a.track_vortices(thr, every=3, start_step=1)
        a._vortexr.restore({k: np.array(v) for k, v in z.items()})
        a.run(N_STEPS - 10, graph=False)
        _assert_equals_twin(a.vortices(), _sampled_steps(N_STEPS, 3, 1), twin, "resumed")
    finally:
        _close(a)


def test_deferred_limit_reaches_the_records(hip_lib):
    """The case tests/test_gpu_pod.py uses: the MAC solver's end-of-step limit_field is always deferred, and the flag is up."""
    import fs
    from fs.solver import VELOCITY_LIMIT
    g = np.load(os.path.join(GOLDEN, "traj_bc1_upwind_vc0.npz"))
    cfg = traj_config(g)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    try:
        mask = g["bc_mask"]
        X = mask.shape[0]
        i = np.arange(X)[:, None] * np.ones(mask.shape[1])[None, :]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[..., 0] = 3.0 * VELOCITY_LIMIT * np.sin(i / 3.0)
        v[..., 1] = -2.0 * VELOCITY_LIMIT * np.cos(i / 5.0)
        v[mask != 0] = 0
        sim._solver.v.current.from_numpy(v)
        dx = sim._solver.dx
        e = _exponent(dx)
        sim.track_vortices(1.0, "vorticity")
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        crit = sim.vortex_criterion("vorticity")
        out = sim.vortices()
        assert cur.pending_limit is not None, "reading the records flushed the owed pass"
        down = sim.field_to_numpy()["v"]                     # (the download launches the owed pass first)
        speed = np.hypot(down[..., 0], down[..., 1])
        assert speed.max() > 0.99 * VELOCITY_LIMIT, "no cell at the limit: the owed pass changed nothing and the test does not cover it"
        ref = R.sample(down, mask, dx, "vorticity", 1.0, e)
        assert ref["count"] > 0
        _assert_sample(out, 0, ref, e, dx, X, "deferred limit")
        assert np.array_equal(crit, R.criterion("vorticity", down, mask, dx)[0], equal_nan=True)
    finally:
        _close(sim)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    from fs import _lib
    sim, mask, dx = _make("scene1", "f32")
    dev = sim._dev
    try:
        with pytest.raises(TypeError):
            sim.track_vortices()                                         # no default threshold
        for bad in (None, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                sim.track_vortices(bad)
        with pytest.raises(ValueError):
            sim.track_vortices(1.0, criterion="lambda2")
        for bad in (0, 1025):
            with pytest.raises(ValueError):
                sim.track_vortices(1.0, max_vortices=bad)
        with pytest.raises(ValueError):
            sim.track_vortices(1.0, every=0)
        with pytest.raises(RuntimeError):
            sim.vortices()
        with pytest.raises(RuntimeError):
            sim.vortex_labels()
        assert sim._vortexr is None
        sim.track_vortices(1.0)
        with pytest.raises(RuntimeError):
            sim.track_vortices(1.0)                                      # a second attach
        sim.step()
        for call in (sim.vortices, sim.vortex_labels, lambda: sim.find_vortices(1.0), lambda: sim.vortex_criterion("q"), sim.stop_vortices,
                     lambda: sim.track_vortices(1.0)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        vx = sim._vortexr.vx
        n, launches, lost = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        words = np.zeros((vx.capacity, 8 + 16 * vx.max_vortices), np.int64)
        lp = words.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))

        def c_read():
            _lib.call("fs_vortex_read", dev._ctx, vx._h, lp, vx.capacity, ctypes.byref(n), ctypes.byref(launches), ctypes.byref(lost))
        for call in (c_read, lambda: _lib.call("fs_vortex_get_labels", dev._ctx, vx._h, None, None), lambda: _lib.call("fs_vortex_set", dev._ctx, vx._h, 0)):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        hh = ctypes.c_void_p()
        for args in ((3, 1.0, 1.0, 1, 0, 4, 64, 100, 4), (0, float("nan"), 1.0, 1, 0, 4, 64, 100, 4), (0, 1.0, 0.0, 1, 0, 4, 64, 100, 4),
                     (0, 1.0, 1.0, 0, 0, 4, 64, 100, 4), (0, 1.0, 1.0, 1, 0, 0, 64, 100, 4), (0, 1.0, 1.0, 1, 0, 4, 1025, 100, 4),
                     (0, 1.0, 1.0, 1, 0, 4, 64, 0, 4), (0, 1.0, 1.0, 1, 0, 4, 64, 100, 0)):
            assert dev._lib.fs_vortex_create(dev._ctx, *args, ctypes.byref(hh)) == -1 and not hh.value, args      # FS_ERR_ARG
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert dev._lib.fs_vortex_create(slab, 0, 1.0, 1.0, 1, 0, 4, 64, 100, 4, ctypes.byref(hh)) == -5 and not hh.value      # FS_ERR_UNSUPPORTED
            assert "slab" in dev._lib.fs_last_error().decode()
            f, lab = np.zeros((32, 64), np.uint8), np.zeros((32, 64), np.int32)
            assert dev._lib.fs_vortex_label(slab, f.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -5
        finally:
            _lib.call("fs_destroy", slab)

        class _Slab:
            nranks, capturing = 2, False
        from fs.runtime import DeviceBase
        with pytest.raises(_lib.FsError):
            DeviceBase.vortex_create(_Slab(), "q", 1.0, 0)
        tok = sim._vortexr.token
        sim.run(N_STEPS, graph=True)
        assert sim._graphs and len(sim.vortices()["step"]) == N_STEPS + 1
        sim.stop_vortices()                                              # the graphs that hold its launches go first
        assert sim._vortexr is None and vx._h is None and not [k for k in sim._graphs if tok in k]
        sim.run(N_STEPS, graph=True)                                     # (and the run goes on without it)
        assert len(sim.vortices()["step"]) == N_STEPS + 1
    finally:
        _close(sim)
