"""Snapshot POD on the GPU (csrc/fs_pod.h k_pod_capture / k_pod_tick / k_pod_gram / k_pod_gram_final / k_pod_combine, include/fs_hip.h
fs_pod_*, FluidSimulator.start_pod): every resident snapshot bit for bit against the download of an eagerly stepped twin taken after the same
step, in eager steps and in replayed graphs, f32 and f64, with the ring wrapped and partly filled, unchanged trajectories; the Gram matrix
against the float64 sum over the downloaded snapshots below, at and past the 8-slot tile; the combine pass against the restatement
(tests/pod_ref.py) bit for bit; the deferred limit pass; the capture rules, the refusals and the life cycle.

The grids are the smallest at which the kernels can go wrong: scene 1 at res 20; a random mask at (37, 12) - odd X, the one-column path;
(1030, 8) - beyond two 256 x 2 column blocks with a partial last one; (102, 13) with FS_DIAG_WGS=1 - 8 rows per workgroup of the capture, so
the second workgroup ends in a partial row group, and the Gram kernel's 64 rows in one workgroup (on the others both take 4 rows per
workgroup: 2 to 5 workgroups down the grid).  The Gram matrix alone also on (1030, 262), 269,860 cells, with uploaded snapshots: at the default
floor 4 rows per workgroup, 5 x 66 = 330 workgroups with a last one of 2 rows, so that k_pod_gram_final folds a second, partial round of
partials (nblocks > 256); with FS_DIAG_WGS=85 16 rows per workgroup, 17 workgroups down the grid, the last of 6 rows.

Gram tolerance (set by the issue that introduced the feature): |G[a][b] - G_numpy[a][b]| <= 1e-12 sqrt(G[a][a] G[b][b]) - the tolerance
tests/flow_stats_ref.py gives the same kind of reduction: column chains of at most a few hundred terms followed by trees, and the sum of |t|
is at most sqrt(G_aa G_bb).  (On the tall grid the column chains are 4 or 16 terms: the same argument.)"""
import ctypes
import functools
import os

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config
from pod_ref import combine_ref, gram_ref, sampling_launches

pytestmark = pytest.mark.gpu

N_STEPS = 20      # (run(graph=True) captures from 16 steps on)
GRIDS = {"scene1": None, "odd": (37, 12, 0.3), "wide": (1030, 8, 0.15), "rows": (102, 13, 0.15)}
GRAM_TOL = 1e-12


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
    """(const, mask, dx) of a grid of GRIDS."""
    if GRIDS[grid] is None:
        from fs.boundary_condition import create_scene_arrays
        const, mask, _ = create_scene_arrays(1, 20)
        return const, mask, 1.0 / 20
    from multigrid_cases import scene
    X, Y, wall_p = GRIDS[grid]
    const, mask = scene(X, Y, wall_p)
    return const, mask, 1.0 / Y


def _make(grid, dtype):
    """A running flow on the grid: the upwind MAC solver (any width) with two red-black iterations."""
    import fs
    const, mask, dx = _scene(grid)
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask)


@functools.lru_cache(maxsize=None)
def _twin(grid, dtype):
    """(v, p) after each of N_STEPS eager steps of a simulator without the rider, and its final fields: computed once per grid and dtype,
    shared by every case, never changed.  (The rows per workgroup of the riders do not matter to it.)"""
    b, _ = _make(grid, dtype)
    try:
        out = []
        for _ in range(N_STEPS):
            b.step()
            d = b.field_to_numpy()
            out.append((d["v"], d["p"]))
        for v, p in out:
            assert np.isfinite(v).all() and np.isfinite(p).all(), "the flow of the test blew up"
        return out, b.field_to_numpy()
    finally:
        _close(b)


def _assert_snapshots(sim, mask, downloads, want_steps, what):
    out = sim.pod()
    assert out["sample_steps"].tolist() == want_steps, (what, out["sample_steps"], want_steps)
    wall = mask == 1
    snaps = []
    for m, step in enumerate(want_steps):
        v, p = sim.pod_snapshot(m)
        v, p = v.to_numpy(), p.to_numpy()
        ev, ep = downloads[step - 1]
        assert v.dtype == ev.dtype and np.array_equal(v, np.where(wall[..., None], 0, ev)), f"{what}: sample {m} (step {step}): v differs from the download"
        assert np.array_equal(p, np.where(wall, 0, ep)), f"{what}: sample {m} (step {step}): p differs from the download"
        assert np.all(v[wall] == 0) and np.all(p[wall] == 0)
        snaps.append(np.stack([v[..., 0], v[..., 1]]))
    assert any(np.abs(s).max() > 0 for s in snaps), "the snapshots are all zero: the test covers nothing"
    return out, np.array(snaps)


def _assert_gram(G, ref, what):
    d = np.sqrt(np.diag(ref))
    err = np.abs(G - ref) / np.maximum(np.outer(d, d), np.finfo(np.float64).tiny)
    print(f"{what}: n {len(G)}, max |G - G_numpy| / sqrt(G_aa G_bb) = {err.max():.3g}")
    assert G.shape == ref.shape and err.max() <= GRAM_TOL, (what, err.max())
    assert np.array_equal(G, G.T), f"{what}: G is not exactly symmetric"


# M, every, start_step: a ring wrap (11 samples in 4 slots: slots 0 .. 2 written three times, slot 3 twice), a partly filled ring with a
# cadence (6 of 8: steps 5, 8, ..., 20)
PARAMS = [(4, 1, 9), (8, 3, 2)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_snapshots_equal_the_downloads_and_trajectory_unchanged(grid, dtype, graph, hip_lib, monkeypatch):
    _diag_env(grid, monkeypatch)
    downloads, final = _twin(grid, dtype)
    for M, every, start in PARAMS + ([(2, 1, 0), (64, 1, 0)] if grid == "odd" else []):
        a, mask = _make(grid, dtype)
        try:
            if grid == "rows":
                assert a._dev.diag_rows()["mean_accumulate"] == 8, "the capture does not take 8 rows per workgroup: the test does not cover it"
            a.start_pod(M, every=every, start_step=start)
            if graph:
                a.run(N_STEPS, graph=True)
                assert a._graphs, "the run replayed no graph"
            else:
                for _ in range(N_STEPS):
                    a.step()
            want = [n + 1 for n in sampling_launches(N_STEPS, every, start)]
            what = f"{grid} {dtype} M={M} every={every} start={start}"
            assert a._dev.pod_read(a._podr.pod) == (N_STEPS, len(want)), what
            out, snaps = _assert_snapshots(a, mask, downloads, want[-M:], what)
            assert (out["samples"], out["steps"]) == (len(want), N_STEPS)
            _assert_gram(out["gram"], gram_ref(snaps), what)          # chronological, whatever the ring's phase
            fa = a.field_to_numpy()
            for k in fa:
                assert np.array_equal(fa[k], final[k]), f"{what}: {k}: the POD changed the trajectory"
        finally:
            _close(a)


def test_deferred_limit_reaches_the_snapshots(hip_lib):
    """The case tests/test_gpu_modes.py uses: the MAC solver's end-of-step limit_field is always deferred, and the flag is up."""
    import fs
    from fs.solver import VELOCITY_LIMIT
    g = np.load(os.path.join(GOLDEN, "traj_bc1_upwind_vc0.npz"))
    cfg = traj_config(g)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    try:
        mask = g["bc_mask"]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[mask == 0] = (3.0 * VELOCITY_LIMIT, -2.0 * VELOCITY_LIMIT)
        sim._solver.v.current.from_numpy(v)
        sim.start_pod(4)
        sim.step()
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        assert dev.pod_read(sim._podr.pod) == (2, 2) and cur.pending_limit is not None      # (reading the counters launches nothing)
        twin = make_product(g, cfg)
        try:
            twin._solver.v.current.from_numpy(v)
            downloads = []
            for _ in range(2):
                twin.step()
                d = twin.field_to_numpy()          # (the download launches the owed pass first)
                downloads.append((d["v"], d["p"]))
        finally:
            _close(twin)
        _, snaps = _assert_snapshots(sim, mask, downloads, [1, 2], "deferred limit")
        speed = np.hypot(snaps[:, 0], snaps[:, 1])
        assert speed.max() > 0.99 * VELOCITY_LIMIT and np.all(speed <= VELOCITY_LIMIT * (1 + 1e-6))
        assert cur.pending_limit is not None, "reading the snapshots flushed the owed pass"
    finally:
        _close(sim)


# ---- the Gram matrix: below, at and one past the 8-slot tile, a second tile row, the full 64 ----------------------------------------------
GRAM_N = (2, 5, 7, 8, 9, 15, 16, 17, 63, 64)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_gram_against_numpy_around_the_tile(grid, dtype, hip_lib, monkeypatch):
    from fs.runtime import Device
    _diag_env(grid, monkeypatch)
    const, mask, _ = _scene(grid)
    mask = np.array(mask)
    X, Y = mask.shape
    dt_ = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(X * 1000 + Y)
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        v, p = dev.alloc(2), dev.alloc(1)
        pod = dev.pod_create(64)
        wall = mask == 1
        ups = []
        for n in range(1, 65):
            # (amplitudes that differ from snapshot to snapshot: the entries of G span two decades)
            va, pa = (rng.standard_normal((X, Y, 2)) * (0.1 + 3.0 * rng.random())).astype(dt_), rng.standard_normal((X, Y)).astype(dt_)
            v.from_numpy(va)
            p.from_numpy(pa)
            dev.pod_launch(pod, v, p)
            ups.append(np.stack([np.where(wall, 0, va[..., 0]), np.where(wall, 0, va[..., 1])]))
            if n in GRAM_N:
                G, launches, samples = dev.pod_gram(pod)
                assert (launches, samples) == (n, n) and G.dtype == np.float64
                _assert_gram(G, gram_ref(np.array(ups)), f"{grid} {dtype}")
                again = dev.pod_gram(pod)[0]
                assert np.array_equal(G, again), "two calls return different bits"
        slots = dev.pod_get(pod)[0]
        assert np.array_equal(slots[:, :2], np.array(ups)), "the slots differ from the masked uploads"
        dev.pod_free(pod)
    finally:
        dev.close()


# ---- the Gram matrix on the tall grid: a second round of k_pod_gram_final, several workgroups of 16 rows with a short last one ---------------
TALL = (1030, 262, 0.15)
TALL_N = (7, 9, 17)      # one tile; two tiles; three tiles with all three off-diagonal pairs


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("rows", [4, 16])
def test_gram_on_the_tall_grid(rows, dtype, hip_lib, monkeypatch):
    """rows = 4 (the default floor of 2048 workgroups): 5 x 66 = 330 workgroups, the last of 2 rows - k_pod_gram_final's lanes 0 .. 73 fold
    a second partial, the others one.  rows = 16 (FS_DIAG_WGS = 85): 5 x 17 workgroups, the last of 6 rows."""
    from fs.runtime import Device
    from helpers import diag_floor
    from multigrid_cases import scene
    X, Y, wall_p = TALL
    if rows == 4:
        monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    else:
        monkeypatch.setenv("FS_DIAG_WGS", str(diag_floor(-(-X // 256), Y, 4, rows)))
    mask = np.array(scene(X, Y, wall_p)[1])
    dt_ = np.float32 if dtype == "f32" else np.float64
    rng = np.random.default_rng(X * 1000 + Y)
    dev = Device(X, Y, dtype)
    try:
        # the Gram kernel's rows: diag_rows (csrc/fs_launch.h) with nx = ceil(X / 256), ny = Y, from 4 up to 64; flow_stats is the same rule
        # with the same inputs from 4 up to 32, and both stop at 4 or 16 here
        assert dev.diag_rows()["flow_stats"] == rows, "the Gram kernel does not take the rows this case is about"
        assert (-(-X // 256) * -(-Y // rows) > 256) == (rows == 4)
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        v, p = dev.alloc(2), dev.alloc(1)
        pod = dev.pod_create(max(TALL_N))
        wall = mask == 1
        p.from_numpy(np.zeros((X, Y), dt_))
        ups = []
        for n in range(1, max(TALL_N) + 1):
            va = (rng.standard_normal((X, Y, 2)) * (0.1 + 3.0 * rng.random())).astype(dt_)
            v.from_numpy(va)
            dev.pod_launch(pod, v, p)
            ups.append(np.stack([np.where(wall, 0, va[..., 0]), np.where(wall, 0, va[..., 1])]))
            if n in TALL_N:
                G, launches, samples = dev.pod_gram(pod)
                assert (launches, samples) == (n, n) and G.dtype == np.float64
                _assert_gram(G, gram_ref(np.array(ups)), f"tall, {rows} rows, {dtype}")
                again = dev.pod_gram(pod)[0]
                assert np.array_equal(G, again), "two calls return different bits"
        dev.pod_free(pod)
    finally:
        dev.close()


def test_partly_filled_ring_and_counter_only_calls(hip_lib, monkeypatch):
    """3 of 8 slots: the 3 x 3 matrix; no sample: n = 0 and nothing launched; the library's own checks of out / max_n."""
    from fs import _lib
    from fs.runtime import Device
    _diag_env("odd", monkeypatch)
    const, mask, _ = _scene("odd")
    mask = np.array(mask)
    X, Y = mask.shape
    rng = np.random.default_rng(5)
    dev = Device(X, Y, "f32")
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), np.float32))
        v, p = dev.alloc(2), dev.alloc(1)
        pod = dev.pod_create(8, every=2, start=1)
        G, launches, samples = dev.pod_gram(pod)
        assert G.shape == (0, 0) and (launches, samples) == (0, 0)
        ups = []
        for n in range(7):                              # launches 2, 4, 6 (counted from 0) sample
            va = rng.standard_normal((X, Y, 2)).astype(np.float32)
            v.from_numpy(va)
            p.from_numpy(va[..., 0])
            dev.pod_launch(pod, v, p)
            if n in (2, 4, 6):
                ups.append(np.where((mask == 1)[None], 0, va.transpose(2, 0, 1)))
        G, launches, samples = dev.pod_gram(pod)
        assert G.shape == (3, 3) and (launches, samples) == (7, 3)
        _assert_gram(G, gram_ref(np.array(ups)), "3 of 8")
        n = ctypes.c_int(-1)
        out = (ctypes.c_double * 4)()
        assert dev._lib.fs_pod_gram(dev._ctx, pod._h, out, 2, ctypes.byref(n), None, None) == -1          # FS_ERR_ARG: out too small
        _lib.call("fs_pod_gram", dev._ctx, pod._h, None, 0, ctypes.byref(n), None, None)
        assert n.value == 3
        dev.pod_free(pod)
    finally:
        dev.close()


# ---- the combine pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["odd", "wide", "rows"])
def test_pod_fields_equal_the_restatement(grid, dtype, hip_lib, monkeypatch):
    _diag_env(grid, monkeypatch)
    a, mask = _make(grid, dtype)
    try:
        a.start_pod(6, every=2)
        for _ in range(N_STEPS):          # 10 samples in 6 slots: the ring has wrapped, slot order is not chronological
            a.step()
        out = a.pod()
        slots = a._dev.pod_get(a._podr.pod)[0]
        r = len(out["energies"])
        assert r >= 2 and out["weights"].shape == (r, 6)
        dt_ = np.float32 if dtype == "f32" else np.float64
        for k in [None] + list(range(r)):
            w = np.full(6, 1.0 / 6) if k is None else out["weights"][k]
            v, p = a.pod_fields(k)
            ev, ep = combine_ref(slots, w, mask, dt_)
            assert np.array_equal(v.to_numpy(), ev) and np.array_equal(p.to_numpy(), ep), (grid, dtype, k)
            assert np.all(ev[mask == 1] == 0) and np.abs(ev).max() > 0
        st = a._dev.flow_stats(a._solver.dx, *a.pod_fields(0))          # (usable wherever fields are, as mean_fields())
        assert st["nonfinite"] == 0 and st["sum_s2"] > 0.0
        # the leading modes are orthonormal under the cell sum.  For lambda_k / lambda_0 >= 1e-2: the Gram tolerance of 1e-12 sqrt(G_aa G_bb)
        # is worth at most 6 * 1e-12 * 1e2 = 6e-10 here, eps * cond 2e-14; storing a unit mode in f32 moves an inner product by <= 1.2e-7
        phi = np.array([a.pod_fields(k)[0].to_numpy().astype(np.float64).ravel() for k in range(min(r, 3))])
        big = out["energies"][:len(phi)] / out["energies"][0] >= 1e-2
        err = np.abs(phi @ phi.T - np.eye(len(phi)))[np.ix_(big, big)].max()
        print(f"{grid} {dtype}: {big.sum()} leading modes, orthonormality error {err:.3g}")
        assert err <= (1e-6 if dtype == "f32" else 1e-9)
    finally:
        _close(a)


# ---- life cycle -------------------------------------------------------------------------------------------------------------------------------
def test_capture_rules_refusals_reset_and_stop(hip_lib, monkeypatch):
    from fs import _lib
    _diag_env("scene1", monkeypatch)
    sim, mask = _make("scene1", "f32")
    dev = sim._dev
    try:
        with pytest.raises(RuntimeError):
            sim.pod()                                                    # not attached
        for bad in (1, 65):
            with pytest.raises(ValueError):
                sim.start_pod(bad)
        sim.start_pod(4, every=2)
        dev.profile(True)
        sim.run(3, graph=False)
        assert dev.profile_report()["pod_capture"][0] == 3               # (while attached: one launch per step, under this name)
        dev.profile(False)
        with pytest.raises(RuntimeError):
            sim.pod()                                                    # one sample
        with pytest.raises(RuntimeError):
            sim.pod_fields(0)
        for call in (sim.pod, sim.reset_pod, sim.pod_fields, lambda: sim.pod_snapshot(0)):
            with pytest.raises((_lib.FsError, RuntimeError)) as e:
                dev.capture(call)
            assert isinstance(e.value, _lib.FsError), call
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.start_pod(4))
        with pytest.raises(RuntimeError):
            sim.start_pod(4)                                             # a second attach without stop_pod()
        pod = sim._podr.pod
        h = pod._h
        v, p = sim._solver.get_fields()[:2]
        # the library refuses on its own as well (FS_ERR_STATE = -3), and checks its arguments (FS_ERR_ARG = -1)
        n, launches, samples = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        w = (ctypes.c_double * 4)(*([0.0] * 4))
        out = (ctypes.c_double * 16)()
        buf = np.zeros((4, 3) + mask.shape[::-1], np.float32)
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_pod_gram(dev._ctx, h, out, 4, ctypes.byref(n), None, None),
                  dev._lib.fs_pod_combine(dev._ctx, h, w, v._h, p._h),
                  dev._lib.fs_pod_read(dev._ctx, h, ctypes.byref(launches), ctypes.byref(samples)),
                  dev._lib.fs_pod_get(dev._ctx, h, buf.ctypes.data_as(ctypes.c_void_p)),
                  dev._lib.fs_pod_set(dev._ctx, h, buf.ctypes.data_as(ctypes.c_void_p), 0, 0),
                  dev._lib.fs_pod_reset(dev._ctx, h),
                  dev._lib.fs_pod_create(dev._ctx, 4, 1, 0, ctypes.byref(ctypes.c_void_p()))]
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3] * 7
        hh = ctypes.c_void_p()
        for M, every, start in ((1, 1, 0), (65, 1, 0), (4, 0, 0), (4, 1, -1)):
            assert dev._lib.fs_pod_create(dev._ctx, M, every, start, ctypes.byref(hh)) == -1 and not hh.value, (M, every, start)
        assert dev._lib.fs_pod_create(dev._ctx, 4, 1, 0, None) == -1 and dev._lib.fs_pod_launch(dev._ctx, None, 0.0, v._h, p._h) == -1
        assert dev._lib.fs_pod_gram(dev._ctx, h, out, 4, None, None, None) == -1 and dev._lib.fs_pod_combine(dev._ctx, h, None, v._h, p._h) == -1
        with pytest.raises(_lib.FsError):
            _lib.call("fs_pod_launch", dev._ctx, h, 0.0, p._h, v._h)          # channel counts
        with pytest.raises(_lib.FsError):
            _lib.call("fs_pod_combine", dev._ctx, h, w, p._h, v._h)
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert dev._lib.fs_pod_create(slab, 4, 1, 0, ctypes.byref(hh)) == -5 and not hh.value          # FS_ERR_UNSUPPORTED
            assert "slab" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)

        class _Slab:
            nranks, capturing = 2, False
        from fs.runtime import DeviceBase
        with pytest.raises(_lib.FsError):
            DeviceBase.pod_create(_Slab(), 4)
        assert dev.pod_read(pod) == (3, 1)                               # nothing of the above counted or cleared anything
        snap = sim.pod_snapshot(0)[0].to_numpy()
        assert np.abs(snap).max() > 0
        # reset: slots and samples to zero, the phase of every runs on (steps 4 and 6 sample next)
        sim.reset_pod()
        assert dev.pod_read(pod) == (3, 0) and not dev.pod_get(pod)[0].any()
        sim.run(3, graph=False)
        assert dev.pod_read(pod) == (6, 2) and sim.pod()["sample_steps"].tolist() == [4, 6]
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        gid = dev.capture(lambda: (dev.pod_launch(pod, v, p), sim.stop_pod()))
        dev.free_graph(gid)
        assert sim._podr is None and pod._h is None
        with pytest.raises(_lib.FsError):                                # the handle is gone
            _lib.call("fs_pod_read", dev._ctx, h, ctypes.byref(launches), ctypes.byref(samples))
        sim.start_pod(3)
        sim.run(N_STEPS, graph=True)
        assert sim.pod()["samples"] == N_STEPS and sim._graphs
        tok = sim._podr.token
        sim.stop_pod()                                                   # outside a capture: the graphs that hold its launch go first
        assert sim._podr is None and not [k for k in sim._graphs if tok in k]
        sim.run(N_STEPS, graph=True)                                     # (and the run goes on without it)
    finally:
        _close(sim)


def test_get_set_round_trip_continues_the_ring(hip_lib, monkeypatch):
    _diag_env("odd", monkeypatch)
    a, mask = _make("odd", "f64")
    b = None
    try:
        a.start_pod(4, every=2, start_step=1)
        for _ in range(11):
            a.step()
        z = a._podr.checkpoint()
        assert z["pod.slots"].shape == (4, 3) + mask.shape and z["pod.slots"].dtype == np.float64 and int(z["pod.samples"]) == 5
        b, _ = _make("odd", "f64")
        b.start_pod(4, every=2, start_step=1)
        b._podr.restore(z)
        got = b._dev.pod_get(b._podr.pod)
        assert np.array_equal(got[0], z["pod.slots"]) and got[1:] == (11, 5)
        assert b.pod()["sample_steps"].tolist() == a.pod()["sample_steps"].tolist() == [5, 7, 9, 11]
        assert np.array_equal(a.pod()["gram"], b.pod()["gram"])
    finally:
        _close(a)
        if b is not None:
            _close(b)
