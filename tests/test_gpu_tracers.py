"""Tracer particles on the GPU (csrc/fs_tracer.h k_tracer_advance / k_tracer_draw, include/fs_hip.h fs_tracer_*, FluidSimulator.seed_tracers):
the particle state bit for bit against the NumPy float64 restatement (tests/tracers_ref.py) on synthetic fields - every fate by
construction, f32 and f64, odd widths, particle counts that are no multiple of the workgroup, a deferred limit pass - and on golden
trajectories replayed as hipGraphs against an eagerly stepped twin; unchanged trajectories and launch counts, the checkpoint round trip,
the overlay, the refusals."""
import ctypes
import os

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config
from tracers_ref import (ALIVE, EXPIRED, LEFT, WALL_HIT, advance_ref, assert_state_equal, fate_scene, new_state, run_reference)

pytestmark = pytest.mark.gpu


def _load(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    return g, traj_config(g)


def _close(sim):
    sim._solver._bc.device.close()


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


# ---- device level: synthetic fields -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("respawn", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_fate_on_the_device(dtype, respawn, hip_lib):
    """The constructed scene of tests/test_tracers_cpu.py (X = 33: odd) plus 300 random seeds - 305 particles, no multiple of 256."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask, v, seeds, expected = fate_scene(dtype=dt_)
    X, Y = mask.shape
    seeds = np.concatenate([seeds, seed_random(mask, 300, 11)])
    assert X % 2 == 1 and len(seeds) % 256 != 0
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        tr = dev.tracer_create(seeds, respawn=respawn, max_age=20)
        exp = new_state(seeds)
        seen = set()
        for _ in range(50):
            dev.tracer_advance(tr, 0.5, vf)
            seen |= set(advance_ref(exp, v, mask, 0.5, respawn, 20).tolist())
        assert seen == {ALIVE, LEFT, WALL_HIT, EXPIRED}, "a fate code did not occur"
        got = dev.tracer_read(tr)
        assert got["x"].dtype == np.float64 and got["age"].dtype == np.int32 and got["steps"] == 50
        assert_state_equal(got, exp)
        if respawn:
            assert not got["status"].any() and np.all(got["respawns"][:5] > 0)
        else:
            assert np.array_equal(got["status"][:5], expected) and not got["respawns"].any()
        dev.tracer_free(tr)
    finally:
        dev.close()


def _random_scene(rng, X, Y):
    mask = (rng.random((X, Y)) < 0.12).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.03] = 2
    mask[rng.random((X, Y)) < 0.03] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


@pytest.mark.parametrize("X,Y,dtype,n,respawn,max_age", [(101, 51, "f32", 1000, True, 0), (67, 33, "f64", 257, False, 9), (250, 125, "f32", 5000, False, 0),
                                                         (1026, 37, "f64", 255, True, 7), (4, 4, "f32", 3, True, 0)])
def test_random_fields_and_masks(X, Y, dtype, n, respawn, max_age, hip_lib):
    """Random velocities (changed between launches) on random masks: wall hits, outflow cells, exits through every edge and expiry as they
    come; the smallest grid the interpolation admits."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    rng = np.random.default_rng(X * 1000 + Y)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = _random_scene(rng, X, Y) if X > 8 else np.zeros((X, Y), np.uint8)
    seeds = seed_random(mask, n, 5)
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        tr = dev.tracer_create(seeds, respawn=respawn, max_age=max_age)
        exp = new_state(seeds)
        fates = set()
        for k in range(50):
            if k % 10 == 0:
                v = (rng.standard_normal((X, Y, 2)) * 1.5).astype(dt_)
                vf.from_numpy(v)
            dev.tracer_advance(tr, 0.4, vf)
            fates |= set(advance_ref(exp, v, mask, 0.4, respawn, max_age).tolist())
        assert_state_equal(dev.tracer_read(tr), exp)
        if X > 8:
            assert {LEFT, WALL_HIT} <= fates and (max_age == 0 or EXPIRED in fates)
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_deferred_limit_reaches_the_corners(dtype, hip_lib):
    """Speeds above the limit in the buffer while a deferred limit_field is owed: the particles see the limited values, the pass stays owed."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    from mean_ref import limit_ref
    X, Y = 130, 65
    rng = np.random.default_rng(17)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = np.zeros((X, Y), np.uint8)
    mask[0, :] = mask[:, 0] = mask[:, -1] = 1
    mask[-1, :] = 3
    seeds = seed_random(mask, 700, 2)
    v = (rng.standard_normal((X, Y, 2)) * 9.0).astype(dt_)
    assert (np.hypot(v[..., 0], v[..., 1]) > 10.0).mean() > 0.2
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        dev.limit_field(10.0, vf, defer=True)
        assert vf.pending_limit == 10.0, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(vf)
        tr = dev.tracer_create(seeds, respawn=True)
        exp, unlimited = new_state(seeds), new_state(seeds)
        for _ in range(50):
            dev.tracer_advance(tr, 0.05, vf)
            advance_ref(exp, v, mask, 0.05, limit=10.0)
            advance_ref(unlimited, v, mask, 0.05)
        assert vf.pending_limit == 10.0                       # (advancing launches nothing else)
        got = dev.tracer_read(tr)
        assert_state_equal(got, exp)
        assert not np.array_equal(got["x"], unlimited["x"]), "the limit made no difference: the test does not cover it"
        stored = vf.to_numpy()                                # the download launches the owed pass
        assert vf.pending_limit is None and np.array_equal(stored, limit_ref(v, 10.0))
        for _ in range(3):                                    # ... and from then on the stored values are the limited ones
            dev.tracer_advance(tr, 0.05, vf)
            advance_ref(exp, stored, mask, 0.05)
        assert_state_equal(dev.tracer_read(tr), exp)
    finally:
        dev.close()


# ---- simulator level: golden trajectories -------------------------------------------------------------------------------------------------
CASES = ["traj_bc5_cip_vc5.npz", "traj_bc1_upwind_jacobi4_vc0.npz", "traj_dye_bc2_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"]


def _seeds(mask):
    from fs.tracers import fluid_only, seed_line, seed_random
    X, Y = mask.shape
    line, _ = fluid_only(mask, seed_line((1.5, 0.25), (1.5, Y - 0.25), 2 * Y))      # across the inflow side
    assert len(line) >= 8
    return np.concatenate([seed_random(mask, 500, 1), line])


@pytest.mark.parametrize("respawn", [True, False])
@pytest.mark.parametrize("fname", CASES)
def test_state_bit_for_bit_and_trajectory_unchanged(fname, respawn, hip_lib):
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        seeds = _seeds(mask)
        max_age = 0 if respawn else 30
        a.seed_tracers(seeds, respawn=respawn, max_age=max_age)
        n = 43                      # (odd: no multiple of a graph period)
        a.run(n, graph=True)
        assert a._graphs, "the run replayed no graph"
        exp = run_reference(b, n, new_state(seeds), respawn, max_age)
        got = a.tracers()
        assert set(got) == {"x", "y", "age", "status", "respawns", "seeds", "steps"} and got["steps"] == 43
        assert_state_equal(got, exp)
        moved = np.hypot(got["x"] - seeds[:, 0], got["y"] - seeds[:, 1])
        assert moved.max() > 1.0, "no particle moved by more than a cell"
        if not respawn:
            assert EXPIRED in got["status"]
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        assert set(fa) == set(fb) and ("dye" in fa) == cfg["dye"]
        for k in fa:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{k}: the tracers changed the trajectory"
    finally:
        _close(a)
        _close(b)


def test_launches_after_stop_equal_a_run_that_never_had_tracers(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    reports, fields = {}, {}
    for traced in (False, True):
        sim = make_product(g, cfg)
        dev = sim._dev
        try:
            if traced:
                sim.seed_tracers(_seeds(g["bc_mask"]))
            sim.run(30, graph=True)
            sim.step()
            if traced:
                assert sim.tracers()["steps"] == 31
                sim.stop_tracers()
                with pytest.raises(RuntimeError):
                    sim.tracers()
                assert not [k for k in sim._graphs if any(isinstance(t, tuple) and t and t[0] == "tracer" for t in k)]
            dev.profile(True)
            sim.run(12, graph=False)
            reports[traced] = {k: v[0] for k, v in dev.profile_report().items()}
            dev.profile(False)
            sim.run(25, graph=True)          # (graphs captured after the stop hold no advance either: same fields)
            fields[traced] = sim.field_to_numpy()
        finally:
            _close(sim)
    assert reports[True] == reports[False], (reports[True], reports[False])
    assert not [k for k in reports[True] if "tracer" in k]
    for k in fields[False]:
        assert np.array_equal(fields[True][k], fields[False][k]), k


def test_checkpoint_round_trip_continues_bit_for_bit(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b, c = make_product(g, cfg), make_product(g, cfg), None
    try:
        seeds = _seeds(g["bc_mask"])
        a.seed_tracers(seeds, respawn=True, max_age=35)
        a.run(50, graph=True)
        b.seed_tracers(seeds, respawn=True, max_age=35)
        b.run(23, graph=True)
        state = b._dev.tracer_read(b._tracers.set)
        assert state["steps"] == 23
        fields = {}
        s = b._solver
        for name in ("v", "p", "vx", "vy"):
            fields[name] = (getattr(s, name).current.to_numpy(), getattr(s, name).next.to_numpy())
        vort = (s.vorticity_confinement.vorticity.to_numpy(), s.vorticity_confinement.vorticity_abs.to_numpy())
        c = make_product(g, cfg)
        for name, (cur, nxt) in fields.items():
            getattr(c._solver, name).current.from_numpy(cur)
            getattr(c._solver, name).next.from_numpy(nxt)
        c._solver.vorticity_confinement.vorticity.from_numpy(vort[0])
        c._solver.vorticity_confinement.vorticity_abs.from_numpy(vort[1])
        c.seed_tracers(seeds[::-1], respawn=True, max_age=35)      # (other seeds: the write restores them too)
        c._dev.tracer_write(c._tracers.set, state)
        assert_state_equal(c.tracers(), state, "written ")
        c.run(27, graph=True)
        ra, rc = a.tracers(), c.tracers()
        assert ra["steps"] == rc["steps"] == 50
        assert_state_equal(rc, ra, "resumed ")
        assert ra["respawns"].min() >= 1 and not ra["status"].any()      # (every particle expired once, in the resumed part of the run)
        fa, fc = a.field_to_numpy(), c.field_to_numpy()
        assert all(np.array_equal(fa[k], fc[k]) for k in fa)
        bad = dict(state, status=np.full_like(state["status"], 4))
        with pytest.raises(ValueError):
            c._dev.tracer_write(c._tracers.set, bad)
        with pytest.raises(ValueError):
            c._dev.tracer_write(c._tracers.set, dict(state, x=state["x"][:-1]))
    finally:
        for sim in (a, b, c):
            if sim is not None:
                _close(sim)


@pytest.mark.parametrize("fname", ["traj_bc5_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"])
def test_draw_tracers_equals_a_numpy_overlay(fname, hip_lib):
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    sim = make_product(g, cfg)
    try:
        sim.seed_tracers(_seeds(g["bc_mask"]), respawn=False)
        sim.run(20, graph=False)
        st = sim.tracers()
        st["status"][::3] = LEFT                              # a third of the particles dead: they are not drawn
        sim._dev.tracer_write(sim._tracers.set, st)
        alive = st["status"] == ALIVE
        assert alive.any() and not alive.all()
        base = sim.get_norm_field().to_numpy().copy()
        out = sim.draw_tracers(color=(1.0, 0.25, 0.0))
        assert out is sim.rgb_buf
        exp = base.copy()
        exp[np.floor(st["x"][alive]).astype(int), np.floor(st["y"][alive]).astype(int)] = (1.0, 0.25, 0.0)
        got = out.to_numpy()
        assert np.array_equal(got, exp) and not np.array_equal(got, base)
        other = sim._dev.alloc(3)
        other.fill(0.0)
        assert sim.draw_tracers(other) is other
        img = other.to_numpy()
        assert int((img == 1.0).all(axis=-1).sum()) == len(np.unique(np.floor(np.stack([st["x"][alive], st["y"][alive]], 1)), axis=0))
        assert np.array_equal(sim.tracers()["x"], st["x"])        # drawing moves nothing
    finally:
        _close(sim)


def test_refusals_and_capture_rules(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    mask = g["bc_mask"]
    X, Y = mask.shape
    wall = np.argwhere(mask == 1)[0] + 0.5
    fluid = np.argwhere(mask == 0)[0] + 0.5
    try:
        with pytest.raises(RuntimeError):
            sim.tracers()
        with pytest.raises(RuntimeError):
            sim.draw_tracers()
        sim.stop_tracers()                                   # nothing attached: nothing happens
        for seeds, word in (([fluid, wall], "seed 1"), ([[X + 0.5, 1.0]], "outside"), ([[1.0, -0.5]], "outside"), (np.zeros((0, 2)), "at least one")):
            with pytest.raises(ValueError) as e:
                sim.seed_tracers(seeds)
            assert word in str(e.value)
        with pytest.raises(ValueError):
            sim.seed_tracers([fluid], max_age=-1)
        assert sim._tracers is None
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.seed_tracers([fluid]))
        sim.seed_tracers([fluid, fluid + 0.25])
        with pytest.raises(RuntimeError):
            sim.seed_tracers([fluid])                        # attached already
        dev.profile(True)
        sim.run(3, graph=False)
        assert dev.profile_report()["tracer_advance"][0] == 3          # (while attached: one launch per step, under this name)
        assert any("k_tracer_advance" in k for k in dev.profile_kernels("tracer_advance"))
        dev.profile(False)
        with pytest.raises((_lib.FsError, RuntimeError)) as e:
            dev.capture(sim.tracers)
        assert isinstance(e.value, _lib.FsError)
        tr = sim._tracers.set
        h = tr._h
        v = sim._solver.get_fields()[0]
        p = sim._solver.get_fields()[1]
        # the library refuses on its own as well (FS_ERR_STATE = -3), and checks channel counts and seeds (FS_ERR_ARG = -1)
        launches = ctypes.c_longlong()
        one = (ctypes.c_double * 2)(*fluid)
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_tracer_read(dev._ctx, h, None, None, ctypes.byref(launches)),
                  dev._lib.fs_tracer_create(dev._ctx, 1, one, 1, 0, ctypes.byref(ctypes.c_void_p()))]
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3, -3]
        with pytest.raises(_lib.FsError):
            _lib.call("fs_tracer_advance", dev._ctx, h, 0.05, 0.0, p._h)
        with pytest.raises(_lib.FsError):
            _lib.call("fs_tracer_draw", dev._ctx, h, 1.0, 1.0, 1.0, v._h)
        with pytest.raises(_lib.FsError):
            _lib.call("fs_tracer_create", dev._ctx, 0, one, 1, 0, ctypes.byref(ctypes.c_void_p()))
        outside = (ctypes.c_double * 2)(float(X), 1.0)
        with pytest.raises(_lib.FsError):
            _lib.call("fs_tracer_create", dev._ctx, 1, outside, 1, 0, ctypes.byref(ctypes.c_void_p()))
        assert sim.tracers()["steps"] == 3                   # nothing of the above advanced anything
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        gid = dev.capture(lambda: (dev.tracer_advance(tr, 0.05, v), sim.stop_tracers()))
        dev.free_graph(gid)
        assert sim._tracers is None and tr._h is None
        with pytest.raises(_lib.FsError):                    # the handle is gone
            _lib.call("fs_tracer_read", dev._ctx, h, None, None, ctypes.byref(launches))
        sim.seed_tracers([fluid])
        sim.run(20, graph=True)
        assert sim.tracers()["steps"] == 20
    finally:
        _close(sim)


def test_slab_contexts_refuse(hip_lib):
    """A slab context (one of two ranks; no communicator is needed to ask): creation is refused by the runtime and by the library."""
    from fs import _lib
    from fs.runtime import Device
    dev = Device(64, 32, "f32", gpu=0, rank=0, nranks=1)
    slab = ctypes.c_void_p()
    _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
    try:
        one = (ctypes.c_double * 2)(3.5, 3.5)
        rc = dev._lib.fs_tracer_create(slab, 1, one, 1, 0, ctypes.byref(ctypes.c_void_p()))
        assert rc == -5, rc                                   # FS_ERR_UNSUPPORTED
        assert "slab" in dev._lib.fs_last_error().decode()
    finally:
        _lib.call("fs_destroy", slab)
        dev.close()

    class _Slab:
        nranks, capturing = 2, False
    from fs.runtime import DeviceBase
    with pytest.raises(_lib.FsError):
        DeviceBase.tracer_create(_Slab(), np.array([[1.5, 1.5]]))

    import fs

    class _Sim:
        _tracers = None
    sim = _Sim()
    sim._dev = _Slab()
    sim._solver = None
    with pytest.raises(_lib.FsError):
        fs.FluidSimulator.seed_tracers(sim, np.array([[1.5, 1.5]]))
