"""Harmonic flow modes on the GPU (csrc/fs_modes.h k_modes_accumulate / k_modes_tick / k_modes_combine, include/fs_hip.h fs_modes_*,
FluidSimulator.start_modes): planes, Gram matrix, phasors and counters bit for bit against the NumPy f64 restatement over the downloads of an
eagerly stepped twin (tests/modes_ref.py), unchanged trajectories and launch counts, the combine pass, the deferred limit pass, odd sizes and
random masks, the capture rules, resume through modes_read / modes_write, slab contexts on one GPU with tape replays, the large-grid row
counts forced onto small grids by FS_DIAG_WGS, and the recovery of a phase-locked signal uploaded launch by launch."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config
from modes_ref import State, combine_ref, launch_ref, sampling_launches

pytestmark = pytest.mark.gpu

N_STEPS = 43      # (odd, 43 % 3 == 1, 43 % 4 == 3: no multiple of `every` or of a graph period)


def _load(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    return g, traj_config(g)


def _close(sim):
    sim._solver._bc.device.close()


def _read(sim):
    return sim._dev.modes_read(sim._moder.modes)


def _freqs(dt, K):
    """K frequencies below the Nyquist limit of every = 4: 0.12, 0.2, 0.44, 0.3 cycles per sample there."""
    return [c / dt for c in (0.03, 0.05, 0.11, 0.075)[:K]]


def _assert_state_equal(got, st, what=""):
    sums, scalars, launches, samples = got
    assert (launches, samples) == (st.launches, st.samples), what
    assert np.array_equal(scalars[:2 * st.K], st.scalars()[:2 * st.K]), f"{what}the phasors differ from the recurrence in NumPy"
    assert np.array_equal(scalars[2 * st.K:], st.gram), f"{what}the Gram matrix differs"
    for k in range(3 * st.B):
        assert np.array_equal(sums[k], st.sums[k]), f"{what}plane {k} (field {'uwp'[k // st.B]}, basis entry {k % st.B}) differs from the NumPy f64 loop"


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


CASES = ["traj_bc5_cip_vc5.npz", "traj_bc1_upwind_jacobi4_vc0.npz", "traj_dye_bc2_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"]


@functools.lru_cache(maxsize=None)
def _twin_downloads(fname):
    """The fields after each of N_STEPS eager steps of an un-instrumented simulator, and its final fields: computed once, shared by every
    case of the trajectory, never changed."""
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    b = make_product(g, cfg)
    try:
        out = []
        for _ in range(N_STEPS):
            b.step()
            d = b.field_to_numpy()
            out.append((d["v"], d["p"]))
        return out, b.field_to_numpy()
    finally:
        _close(b)


def _reference(fname, freqs, every, start, dt, mask):
    from fs.modes import phasor_steps
    downloads, final = _twin_downloads(fname)
    st = State(mask.shape, *phasor_steps(freqs, every, dt))
    for v, p in downloads:
        launch_ref(st, v, p, mask, every, start)
    return st, final


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("every,start", [(1, 0), (3, 0), (4, 10)])
@pytest.mark.parametrize("fname", CASES)
def test_state_bit_for_bit_and_trajectory_unchanged(fname, every, start, K, hip_lib):
    import fs
    g, cfg = _load(fname)
    mask = g["bc_mask"]
    freqs = _freqs(cfg["dt"], K)
    st, final = _reference(fname, freqs, every, start, cfg["dt"], mask)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    a = make_product(g, cfg)
    try:
        a.start_modes(freqs, every=every, start_step=start)
        a.run(N_STEPS, graph=True)
        assert a._graphs, "the run replayed no graph"
        got = _read(a)
        assert st.launches == N_STEPS and st.samples == len(sampling_launches(N_STEPS, every, start)) > 2 * K
        assert got[0].dtype == np.float64 and got[0].shape == (3 * (1 + 2 * K),) + mask.shape
        _assert_state_equal(got, st)
        assert np.all(got[0][:, mask == 1] == 0.0), "a wall cell was touched"
        assert all(np.abs(got[0][k]).max() > 0.0 for k in (0, 1, 2 * K, 3 * (1 + 2 * K) - 1))
        out = a.modes()
        assert (out["samples"], out["steps"]) == (st.samples, N_STEPS) and out["u"]["amplitude"].shape == (K,) + mask.shape
        fa = a.field_to_numpy()
        assert set(fa) == set(final) and ("dye" in fa) == cfg["dye"]
        for k in fa:
            assert np.array_equal(fa[k], final[k], equal_nan=True), f"{k}: the modes changed the trajectory"
    finally:
        _close(a)


def test_launches_after_stop_equal_a_run_that_never_attached(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    reports, fields = {}, {}
    for attached in (False, True):
        sim = make_product(g, cfg)
        dev = sim._dev
        try:
            if attached:
                sim.start_modes(_freqs(cfg["dt"], 2), every=2)
            sim.run(30, graph=True)
            sim.step()
            if attached:
                assert sim.modes()["samples"] == 15
                sim.stop_modes()
                with pytest.raises(RuntimeError):
                    sim.modes()
            dev.profile(True)
            sim.run(12, graph=False)
            reports[attached] = {k: v[0] for k, v in dev.profile_report().items()}
            dev.profile(False)
            sim.run(25, graph=True)          # (graphs captured after the stop hold no accumulation either: same fields)
            fields[attached] = sim.field_to_numpy()
        finally:
            _close(sim)
    assert reports[True] == reports[False], (reports[True], reports[False])
    assert not [k for k in reports[True] if "modes" in k]
    for k in fields[False]:
        assert np.array_equal(fields[True][k], fields[False][k]), k


def _random_scene(rng, X, Y):
    mask = (rng.random((X, Y)) < 0.3).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.05] = 2
    mask[rng.random((X, Y)) < 0.05] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


def _cos_sin(rng, K):
    delta = rng.uniform(0.2, 2.8, K)
    return np.stack([np.cos(delta), np.sin(delta)], axis=1)


SIZES = [(102, 51, "f32"), (150, 75, "f32"), (162, 81, "f64"), (101, 51, "f32"), (67, 33, "f64"), (1026, 37, "f32")]


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("X,Y,dtype", SIZES)
def test_odd_sizes_and_random_masks(X, Y, dtype, K, hip_lib):
    """Uploads of random fields on random masks, 7 launches of which 3 sample, against NumPy: widths that are no multiples of 4, odd widths
    (the one-column path), a width of more than two workgroups; then the combine pass, the write / read round trip and the reset."""
    _odd_sizes_case(X, Y, dtype, K)


def _odd_sizes_case(X, Y, dtype, K, want_rows=None):
    from fs.runtime import Device
    rng = np.random.default_rng(X * 1000 + Y * 10 + K)
    dt_ = np.float32 if dtype == "f32" else np.float64
    B = 1 + 2 * K
    dev = Device(X, Y, dtype)
    try:
        if want_rows is not None:
            rows = dev.modes_rows(K)
            assert rows == want_rows, f"{X} x {Y}, {K} frequencies: {rows}, not {want_rows} rows per workgroup: the test does not cover it"
        mask = _random_scene(rng, X, Y)
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        v, p = dev.alloc(2), dev.alloc(1)
        cs = _cos_sin(rng, K)
        m = dev.modes_create(cs, every=2, start=1)
        st = State((X, Y), cs[:, 0], cs[:, 1])
        for n in range(7):                              # launches 2, 4, 6 (counted from 0) sample
            va, pa = rng.standard_normal((X, Y, 2)).astype(dt_) * 3, rng.standard_normal((X, Y)).astype(dt_)
            v.from_numpy(va)
            p.from_numpy(pa)
            dev.modes_accumulate(m, v, p)
            launch_ref(st, va, pa, mask, 2, 1)
        got = dev.modes_read(m)
        assert got[2:] == (7, 3) == (st.launches, st.samples)
        _assert_state_equal(got, st)
        sums = got[0]
        assert np.all(sums[:, mask == 1] == 0.0)
        # the combine pass with random weights
        w = rng.standard_normal((3, B))
        vo, po = dev.alloc(2), dev.alloc(1)
        dev.modes_combine(m, w, vo, po)
        ev, ep = combine_ref(sums, w, mask, dt_)
        assert np.array_equal(vo.to_numpy(), ev) and np.array_equal(po.to_numpy(), ep)
        assert np.abs(ev).max() > 0.0 and np.all(ev[mask == 1] == 0.0)
        # write / read round trip, reset
        back, sc = rng.standard_normal(sums.shape), rng.standard_normal(got[1].shape)
        dev.modes_write(m, back, sc, 11, 5)
        again = dev.modes_read(m)
        assert np.array_equal(again[0], back) and np.array_equal(again[1], sc) and again[2:] == (11, 5)
        dev.modes_reset(m)
        again = dev.modes_read(m)
        assert not again[0].any() and again[2:] == (11, 0)
        assert again[1].tolist() == [1.0, 0.0] * K + [0.0] * (B * (B + 1) // 2)
        dev.modes_free(m)
    finally:
        dev.close()


# ---- the forms of large grids, forced onto small ones by FS_DIAG_WGS ----------------------------------------------------------------------
# k_modes_accumulate takes row groups of 4 (K <= 2) or 2 (K >= 3) rows and at most two groups per workgroup; k_modes_combine 1 to 8 rows.
# Without the switch every grid below 2048 workgroups takes one group and one row.
def _most_rows(K):
    return {"accumulate": 8 if K <= 2 else 4, "combine": 8}


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("X,Y,dtype", [(102, 9, "f32"), (102, 13, "f32"), (101, 13, "f32"), (101, 37, "f32"), (1026, 37, "f32"),
                                       (102, 13, "f64"), (101, 37, "f64")])
def test_odd_sizes_two_groups_per_workgroup(X, Y, dtype, K, hip_lib, monkeypatch):
    """Heights of 9, 13 and 37 rows: a workgroup holds two load groups, the last workgroup is a partial one (1 or 5 rows of 8; 1 of 4)."""
    monkeypatch.setenv("FS_DIAG_WGS", "1")
    _odd_sizes_case(X, Y, dtype, K, want_rows=_most_rows(K))


def test_default_rows_on_small_grids(hip_lib, monkeypatch):
    from fs.runtime import Device
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    dev = Device(102, 51, "f32")
    try:
        assert [dev.modes_rows(K) for K in (1, 2, 3, 4)] == [{"accumulate": 4, "combine": 1}] * 2 + [{"accumulate": 2, "combine": 1}] * 2
        assert dev.diag_rows() == {"flow_stats": 4, "mean_accumulate": 4, "mean_finalize": 1}
    finally:
        dev.close()


def test_deferred_limit_reaches_the_sums(hip_lib):
    _deferred_limit_case(1)


def test_deferred_limit_reaches_the_sums_two_groups(hip_lib, monkeypatch):
    monkeypatch.setenv("FS_DIAG_WGS", "1")
    _deferred_limit_case(3, want_rows=_most_rows(3))


def _deferred_limit_case(K, want_rows=None):
    import fs
    from fs.modes import phasor_steps
    from fs.solver import VELOCITY_LIMIT
    g, cfg = _load("traj_bc1_upwind_vc0.npz")          # (MacSolver: its end-of-step limit_field is always deferred)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    try:
        if want_rows is not None:
            assert dev.modes_rows(K) == want_rows, f"{dev.modes_rows(K)}: the test does not cover {want_rows}"
        mask = g["bc_mask"]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[mask == 0] = (3.0 * VELOCITY_LIMIT, -2.0 * VELOCITY_LIMIT)
        sim._solver.v.current.from_numpy(v)
        freqs = _freqs(cfg["dt"], K)
        sim.start_modes(freqs)
        sim.step()
        sim.step()                                   # (the second sample carries rotated phasors: the sine planes are not 0)
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        got = _read(sim)
        assert cur.pending_limit is not None and got[2:] == (2, 2)      # (reading the sums launches nothing)
        # the twin downloads after each step: the download launches the owed pass first
        twin = make_product(g, cfg)
        try:
            twin._solver.v.current.from_numpy(v)
            st = State(mask.shape, *phasor_steps(freqs, 1, cfg["dt"]))
            for _ in range(2):
                twin.step()
                d = twin.field_to_numpy()
                launch_ref(st, d["v"], d["p"], mask, 1, 0)
        finally:
            _close(twin)
        _assert_state_equal(got, st)
        B = 1 + 2 * K
        speed = np.hypot(got[0][0], got[0][B]) / 2.0          # |mean of two limited samples| <= the limit
        assert speed.max() > 0.0 and np.all(speed <= VELOCITY_LIMIT * (1 + 1e-6))
        assert np.abs(got[0][2]).max() > 0.0
    finally:
        _close(sim)


def test_capture_rules_and_refusals(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    freqs = _freqs(cfg["dt"], 1)
    try:
        sim.start_modes(freqs)
        dev.profile(True)
        sim.run(3, graph=False)
        assert dev.profile_report()["modes_accumulate"][0] == 3          # (while attached: one launch per step, under this name)
        dev.profile(False)
        for call in (sim.modes, sim.reset_modes, sim.mode_fields):
            with pytest.raises((_lib.FsError, RuntimeError)) as e:
                dev.capture(call)
            assert isinstance(e.value, _lib.FsError), call
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.start_modes(freqs))
        with pytest.raises(RuntimeError):
            sim.start_modes(freqs)                                       # a second attach without stop_modes()
        modes = sim._moder.modes
        h = modes._h
        v, p = sim._solver.get_fields()[:2]
        # the library refuses on its own as well (FS_ERR_STATE = -3), and checks channel counts
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        cs = (ctypes.c_double * 2)(1.0, 0.0)
        w = (ctypes.c_double * 9)(*([0.0] * 9))
        sc = (ctypes.c_double * 8)()
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_modes_read(dev._ctx, h, None, None, ctypes.byref(launches), ctypes.byref(samples)),
                  dev._lib.fs_modes_reset(dev._ctx, h), dev._lib.fs_modes_combine(dev._ctx, h, w, v._h, p._h),
                  dev._lib.fs_modes_write(dev._ctx, h, sc, sc, 0, 0)]
            hh = ctypes.c_void_p()
            st.append(dev._lib.fs_modes_create(dev._ctx, 1, cs, 1, 0, ctypes.byref(hh)))
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3, -3, -3, -3, -3]
        with pytest.raises(_lib.FsError):
            _lib.call("fs_modes_accumulate", dev._ctx, h, 0.0, p._h, v._h)
        with pytest.raises(_lib.FsError):
            _lib.call("fs_modes_combine", dev._ctx, h, w, p._h, v._h)
        for nfreq, every in ((0, 1), (5, 1), (1, 0)):
            with pytest.raises(_lib.FsError):
                _lib.call("fs_modes_create", dev._ctx, nfreq, cs, every, 0, ctypes.byref(ctypes.c_void_p()))
        assert _read(sim)[2:] == (3, 3)                         # nothing of the above counted or cleared anything
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        gid = dev.capture(lambda: (dev.modes_accumulate(modes, v, p), sim.stop_modes()))
        dev.free_graph(gid)
        assert sim._moder is None and modes._h is None
        with pytest.raises(_lib.FsError):                       # the handle is gone
            _lib.call("fs_modes_read", dev._ctx, h, None, None, ctypes.byref(launches), ctypes.byref(samples))
        sim.start_modes(freqs)
        sim.run(5, graph=True)
        assert sim.modes()["samples"] == 5
    finally:
        _close(sim)


def test_resume_equals_uninterrupted_run(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b, c = make_product(g, cfg), make_product(g, cfg), None
    freqs = _freqs(cfg["dt"], 2)
    try:
        every, start = 3, 5
        a.start_modes(freqs, every=every, start_step=start)
        a.run(50, graph=True)
        b.start_modes(freqs, every=every, start_step=start)
        b.run(23, graph=True)
        sums, scalars, launches, samples = _read(b)
        assert (launches, samples) == (23, 6)
        state = {}
        s = b._solver
        for name in ("v", "p", "vx", "vy"):
            if hasattr(s, name):
                state[name] = (getattr(s, name).current.to_numpy(), getattr(s, name).next.to_numpy())
        vort = (s.vorticity_confinement.vorticity.to_numpy(), s.vorticity_confinement.vorticity_abs.to_numpy())
        c = make_product(g, cfg)
        for name, (cur, nxt) in state.items():
            getattr(c._solver, name).current.from_numpy(cur)
            getattr(c._solver, name).next.from_numpy(nxt)
        c._solver.vorticity_confinement.vorticity.from_numpy(vort[0])
        c._solver.vorticity_confinement.vorticity_abs.from_numpy(vort[1])
        c.start_modes(freqs, every=every, start_step=start)
        c._dev.modes_write(c._moder.modes, sums, scalars, launches, samples)
        c.run(27, graph=True)
        ra, rc = _read(a), _read(c)
        assert ra[2:] == rc[2:] == (50, 15)
        assert np.array_equal(ra[0], rc[0]) and np.array_equal(ra[1], rc[1]), "the resumed run differs"
        assert np.abs(ra[0][4]).max() > 0.0
        fa, fc = a.field_to_numpy(), c.field_to_numpy()
        assert all(np.array_equal(fa[k], fc[k]) for k in fa)
    finally:
        for sim in (a, b, c):
            if sim is not None:
                _close(sim)


# ---- slab contexts on one GPU (the thread harness of test_gpu_slab_threads.py), tape replays -------------------------------------
def _slab_modes(const, mask, cfg, freqs, world, halo, every, start, steps):
    import fs
    from test_gpu_slab_threads import _make_device_cls
    shared = {"barrier": threading.Barrier(world), "box": [None] * world, "radii": [None] * world}
    Dev = _make_device_cls(world, shared)
    results, errors = [None] * world, []

    def work(rank):
        try:
            dt, dx, re = cfg["dt"], cfg["dx"], cfg["re"]
            X, Y = mask.shape
            dev = Dev(X, Y, np.float32, rank, halo)
            bc = fs.BoundaryCondition(const, mask, device=dev)
            vc = fs.VorticityConfinement(bc, dt, dx, cfg["vor_eps"])
            pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
            sim = fs.FluidSimulator(fs.CipMacSolver(bc, pu, dt, dx, re, vc))
            sim.start_modes(freqs, every=every, start_step=start)
            sim.run(steps)
            sums, scalars, launches, samples = dev.modes_read(sim._moder.modes, local=True)
            out = sim.modes(local=True)
            results[rank] = (sums, scalars, launches, samples, len(sim._tapes), dev.nyl, out["u"]["amplitude"])
            dev.close()
        except BaseException as e:   # noqa: BLE001 - surface in the main thread
            errors.append((rank, repr(e)))
            shared["barrier"].abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    return results


@functools.lru_cache(maxsize=None)
def _slab_single_context():
    import fs
    from fs.boundary_condition import BoundaryCondition, create_scene_arrays
    res = 45
    const, mask, _ = create_scene_arrays(5, res)
    cfg = dict(dt=0.05 / res, dx=1.0 / res, re=1.0e6, vor_eps=5.0)
    freqs = tuple(_freqs(cfg["dt"], 2))
    fs.runtime.init(gpu=0, dtype="f32")
    bc = BoundaryCondition(const, mask)
    one = fs.FluidSimulator(fs.CipMacSolver(bc, fs.RedBlackSorPressureUpdater(bc, cfg["dt"], cfg["dx"], 1.3, 2), cfg["dt"], cfg["dx"], cfg["re"],
                                            fs.VorticityConfinement(bc, cfg["dt"], cfg["dx"], cfg["vor_eps"])))
    try:
        one.start_modes(freqs, every=3, start_step=7)
        one.run(70, graph=False)
        return const, mask, cfg, freqs, _read(one), one.modes()["u"]["amplitude"]
    finally:
        _close(one)


@pytest.mark.parametrize("world,halo", [(2, 4), (3, 4)])
def test_slab_contexts_match_single_context(world, halo, hip_lib):
    """bc5 at res 45: 90 x 45 cells, slabs of 23 + 22 / 15 + 15 + 15 rows - partial row groups of the kernel in every slab layout."""
    const, mask, cfg, freqs, exp, amp = _slab_single_context()
    assert exp[2:] == (70, 21) and np.abs(exp[0][3]).max() > 0.0
    res_ = _slab_modes(const, mask, cfg, freqs, world, halo, 3, 7, 70)
    assert all(r[4] > 0 for r in res_), "no tape was replayed"
    assert any(r[5] % 2 for r in res_), "every slab holds whole row groups: the partial group is not covered"
    for r in res_:
        assert r[2:4] == exp[2:] and np.array_equal(r[1], exp[1]), "a rank's counters, phasors or Gram matrix differ from the single context"
    got = np.concatenate([r[0] for r in res_], axis=2)
    assert np.array_equal(got, exp[0]), "the assembled planes differ from the single context"
    assert np.array_equal(np.concatenate([r[6] for r in res_], axis=2), amp)


# ---- a phase-locked signal, uploaded launch by launch ----------------------------------------------------------------------------------
def test_phase_locked_recovery(hip_lib):
    """x_m = m0 + A cos(m delta) + B sin(m delta) per cell and field, 37 samples of 14.8 per period, stored as f32: the fit recovers A and B
    within 1e-6 max|x| (tests/test_modes_cpu.py derives the bound), and mode_fields equals the NumPy combination of the planes bit for bit."""
    import fs
    from fs.modes import reconstruct_weights
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        rng = np.random.default_rng(37)
        n, per_period = 37, 14.8
        f = 1.0 / (per_period * cfg["dt"])
        delta = 2.0 * np.pi * f * cfg["dt"]
        m0, A, B = (rng.uniform(-1.5, 1.5, (3,) + mask.shape) for _ in range(3))
        sim.start_modes([f])
        vf, pf = sim._solver.get_fields()[:2]
        xmax = 0.0
        for m in range(n):
            x = m0 + A * np.cos(m * delta) + B * np.sin(m * delta)
            xmax = max(xmax, np.abs(x).max())
            vf.from_numpy(np.stack([x[0], x[1]], axis=-1).astype(np.float32))
            pf.from_numpy(x[2].astype(np.float32))
            sim._moder.launch(sim)
        out = sim.modes()
        assert (out["samples"], out["steps"]) == (n, n)
        fluid = mask != 1
        err = 0.0
        for a, name in enumerate(("u", "w", "p")):
            fit = out[name]
            err = max(err, np.abs(fit["mean"] - m0[a])[fluid].max(), np.abs(fit["cos"][0] - A[a])[fluid].max(), np.abs(fit["sin"][0] - B[a])[fluid].max())
            assert np.all(fit["amplitude"][0][~fluid] == 0.0)
        print(f"phase-locked recovery: error {err:.3g}, bound {1e-6 * xmax:.3g}")
        assert err <= 1e-6 * xmax
        sums, scalars = _read(sim)[:2]
        for phase in (None, 0.0, 1.9):
            w = reconstruct_weights(scalars, 1, None if phase is None else [phase])
            v, p = sim.mode_fields(phase)
            ev, ep = combine_ref(sums, np.tile(w, (3, 1)), mask, np.float32)
            assert np.array_equal(v.to_numpy(), ev) and np.array_equal(p.to_numpy(), ep), phase
        # at phase 0 the phase-averaged flow is mean + cos coefficient
        v0 = sim.mode_fields(0.0)[0].to_numpy()[..., 0]
        # (the errors of mean and cos coefficient, each within the bound above, add; the cast to f32 rounds by 6e-8 |x|)
        assert np.abs(v0 - (m0[0] + A[0]))[fluid].max() <= 2.1e-6 * xmax
        st = sim._dev.flow_stats(cfg["dx"], *sim.mode_fields(0.5))          # (usable wherever fields are, as mean_fields())
        assert st["nonfinite"] == 0 and st["sum_s2"] > 0.0
    finally:
        _close(sim)
