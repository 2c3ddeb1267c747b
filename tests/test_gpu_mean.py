"""Time averages on the GPU (csrc/fs_mean.h k_mean_accumulate / k_mean_tick / k_mean_finalize, include/fs_hip.h fs_mean_*,
FluidSimulator.start_averaging): the seven sums bit for bit against a NumPy f64 loop over the downloads of an eagerly stepped twin
(tests/mean_ref.py), unchanged trajectories and launch counts, the finalized mean fields, the deferred limit pass, odd sizes and random
masks, the capture rules, slab contexts on one GPU with tape replays, resume through mean_read / mean_write; and the kernels with 8 rows
per workgroup (finalize: 2, 4 and 8) - the forms of large grids - forced onto small grids by FS_DIAG_WGS."""
import ctypes
import os
import threading

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import diag_floor, make_product, traj_config
from mean_ref import accumulate_ref, new_sums, run_reference, sampling_launches

pytestmark = pytest.mark.gpu

SUM_NAMES = ("S_u", "S_w", "S_p", "S_uu", "S_ww", "S_uw", "S_pp")


def _load(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    return g, traj_config(g)


def _close(sim):
    sim._solver._bc.device.close()


def _read(sim):
    return sim._dev.mean_read(sim._averager.mean)


def _assert_sums_equal(got, exp, what=""):
    for k, name in enumerate(SUM_NAMES):
        assert np.array_equal(got[k], exp[k]), f"{what}{name} differs from the NumPy f64 loop"


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


CASES = ["traj_bc5_cip_vc5.npz", "traj_bc1_upwind_jacobi4_vc0.npz", "traj_dye_bc2_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"]


@pytest.mark.parametrize("every,start", [(1, 0), (3, 0), (4, 10)])
@pytest.mark.parametrize("fname", CASES)
def test_sums_bit_for_bit_and_trajectory_unchanged(fname, every, start, hip_lib):
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        a.start_averaging(every=every, start_step=start)
        n = 43                      # (odd, 43 % 3 == 1, 43 % 4 == 3: no multiple of `every` or of a graph period)
        a.run(n, graph=True)
        assert a._graphs, "the run replayed no graph"
        exp, launches, samples = run_reference(b, n, every, start)
        sums, got_launches, got_samples = _read(a)
        assert (got_launches, got_samples) == (launches, samples) == (n, len(sampling_launches(n, every, start)))
        assert samples > 0 and sums.dtype == np.float64 and sums.shape == (7,) + g["bc_mask"].shape
        _assert_sums_equal(sums, exp)
        assert np.all(sums[:, g["bc_mask"] == 1] == 0.0), "a wall cell was touched"
        assert np.abs(sums[0]).max() > 0.0 and np.abs(sums[6]).max() > 0.0
        out = a.averages()
        assert (out["samples"], out["steps"]) == (samples, n)
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        assert set(fa) == set(fb) and ("dye" in fa) == cfg["dye"]
        for k in fa:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{k}: averaging changed the trajectory"
    finally:
        _close(a)
        _close(b)


def test_launches_after_stop_equal_a_run_that_never_averaged(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    reports = {}
    fields = {}
    for averaged in (False, True):
        sim = make_product(g, cfg)
        dev = sim._dev
        try:
            if averaged:
                sim.start_averaging(every=2)
            sim.run(30, graph=True)
            if averaged:
                sim.step()
                assert sim.averages()["samples"] == 15
                sim.stop_averaging()
                with pytest.raises(RuntimeError):
                    sim.averages()
            else:
                sim.step()
            dev.profile(True)
            sim.run(12, graph=False)
            reports[averaged] = {k: v[0] for k, v in dev.profile_report().items()}
            dev.profile(False)
            sim.run(25, graph=True)          # (graphs captured after the stop hold no accumulation either: same fields)
            fields[averaged] = sim.field_to_numpy()
        finally:
            _close(sim)
    assert reports[True] == reports[False], (reports[True], reports[False])
    assert not [k for k in reports[True] if "mean" in k]
    for k in fields[False]:
        assert np.array_equal(fields[True][k], fields[False][k]), k


@pytest.mark.parametrize("fname", ["traj_bc5_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"])
def test_finalize_and_mean_flow_stats(fname, hip_lib):
    import fs
    from flow_stats_ref import SLOTS, compare, flow_stats_ref
    from fs.boundary_condition import default_body_box
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    sim = make_product(g, cfg)
    dt_ = np.float64 if cfg["fp64"] else np.float32
    try:
        sim.start_averaging(every=2, start_step=1)
        sim.run(31, graph=True)
        sums, _, n = _read(sim)
        assert n == 15
        mask = g["bc_mask"]
        v, p = sim.mean_fields()
        va, pa = v.to_numpy(), p.to_numpy()
        assert va.dtype == dt_ and pa.dtype == dt_
        wall = mask == 1
        for got, k in ((va[..., 0], 0), (va[..., 1], 1), (pa, 2)):
            assert np.array_equal(got, np.where(wall, dt_(0), (sums[k] / np.float64(n)).astype(dt_))), SUM_NAMES[k]
        assert np.abs(va).max() > 0.0
        out = sim.averages()
        assert np.array_equal(out["u"].astype(dt_), va[..., 0]) and np.array_equal(out["p"].astype(dt_), pa)
        box = default_body_box(cfg["bc"], cfg["res"])
        dev = sim._dev
        raw = dev.flow_stats(cfg["dx"], v, p, box)
        exp = flow_stats_ref(va, pa, mask, cfg["dx"], box)
        assert not compare(raw, exp), compare(raw, exp)
        st = sim.mean_flow_stats(box)
        assert st["fluid_cells"] == int(exp["fluid_cells"]) and st["nonfinite"] == 0
        assert st["kinetic_energy"] == 0.5 * cfg["dx"] * cfg["dx"] * raw["sum_s2"] and st["force_x"] == raw["force_x"]
        assert set(SLOTS) == set(raw)
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_sums(hip_lib):
    _deferred_limit_case()


def _deferred_limit_case(want_rows=None):
    import fs
    from fs.solver import VELOCITY_LIMIT
    g, cfg = _load("traj_bc1_upwind_vc0.npz")          # (MacSolver: its end-of-step limit_field is always deferred)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    try:
        if want_rows is not None:
            assert dev.diag_rows()["mean_accumulate"] == want_rows, f"{dev.diag_rows()}: the test does not cover {want_rows} rows per workgroup"
        mask = g["bc_mask"]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[mask == 0] = (3.0 * VELOCITY_LIMIT, -2.0 * VELOCITY_LIMIT)
        sim._solver.v.current.from_numpy(v)
        sim.start_averaging()
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        sums, launches, samples = _read(sim)
        assert cur.pending_limit is not None and (launches, samples) == (1, 1)      # (reading the sums launches nothing)
        d = sim.field_to_numpy()                     # the download launches the owed pass first
        exp = accumulate_ref(new_sums(mask.shape), d["v"], d["p"], mask)
        _assert_sums_equal(sums, exp)
        speed = np.hypot(sums[0], sums[1])
        assert speed.max() > 0.99 * VELOCITY_LIMIT and np.all(speed <= VELOCITY_LIMIT * (1 + 1e-6))
    finally:
        _close(sim)


def _random_scene(rng, X, Y):
    mask = (rng.random((X, Y)) < 0.3).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.05] = 2
    mask[rng.random((X, Y)) < 0.05] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


@pytest.mark.parametrize("X,Y,dtype", [(102, 51, "f32"), (150, 75, "f32"), (162, 81, "f64"), (250, 125, "f32"), (250, 125, "f64"),
                                       (101, 51, "f32"), (67, 33, "f64"), (1026, 37, "f32")])
def test_odd_sizes_and_random_masks(X, Y, dtype, hip_lib):
    """Uploads of random fields on random masks, three samples against NumPy: the widths of tests/test_gpu_odd_res.py (2 res for res 51, 75,
    81, 125: not multiples of 4, odd heights), odd widths (the one-column path) and a width of more than two workgroups."""
    _odd_sizes_case(X, Y, dtype)


def _odd_sizes_case(X, Y, dtype, want_rows=None):
    from fs.runtime import Device
    rng = np.random.default_rng(X * 1000 + Y)
    dt_ = np.float32 if dtype == "f32" else np.float64
    dev = Device(X, Y, dtype)
    try:
        if want_rows is not None:
            rows = dev.diag_rows()
            assert (rows["mean_accumulate"], rows["mean_finalize"]) == want_rows, (f"{X} x {Y}: {rows}, not {want_rows} rows per workgroup "
                                                                                   "(accumulate, finalize): the test does not cover it")
        mask = _random_scene(rng, X, Y)
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        v, p = dev.alloc(2), dev.alloc(1)
        m = dev.mean_create(every=2, start=1)
        exp = new_sums((X, Y))
        for n in range(7):                              # launches 2, 4, 6 (n = 2, 4, 6 counted from 0 -> steps 3, 5, 7) sample
            va, pa = rng.standard_normal((X, Y, 2)).astype(dt_) * 3, rng.standard_normal((X, Y)).astype(dt_)
            v.from_numpy(va)
            p.from_numpy(pa)
            dev.mean_accumulate(m, v, p)
            if n in sampling_launches(7, 2, 1):
                accumulate_ref(exp, va, pa, mask)
        sums, launches, samples = dev.mean_read(m)
        assert (launches, samples) == (7, 3)
        _assert_sums_equal(sums, exp)
        assert np.all(sums[:, mask == 1] == 0.0)
        vo, po = dev.alloc(2), dev.alloc(1)
        dev.mean_finalize(m, vo, po)
        assert np.array_equal(vo.to_numpy()[..., 0], np.where(mask == 1, dt_(0), (sums[0] / 3.0).astype(dt_)))
        assert np.array_equal(vo.to_numpy()[..., 1], np.where(mask == 1, dt_(0), (sums[1] / 3.0).astype(dt_)))
        assert np.array_equal(po.to_numpy(), np.where(mask == 1, dt_(0), (sums[2] / 3.0).astype(dt_)))
        # write / read round trip, reset
        back = rng.standard_normal(sums.shape)
        dev.mean_write(m, back, 11, 5)
        got = dev.mean_read(m)
        assert np.array_equal(got[0], back) and got[1:] == (11, 5)
        dev.mean_reset(m)
        got = dev.mean_read(m)
        assert not got[0].any() and got[1:] == (11, 0)
        dev.mean_free(m)
    finally:
        dev.close()


def test_capture_rules_and_refusals(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    try:
        sim.start_averaging()
        dev.profile(True)
        sim.run(3, graph=False)
        assert dev.profile_report()["mean_accumulate"][0] == 3          # (while attached: one launch per step, under this name)
        dev.profile(False)
        for call in (sim.averages, sim.reset_averages, sim.mean_flow_stats):
            with pytest.raises((_lib.FsError, RuntimeError)) as e:
                dev.capture(call)
            assert isinstance(e.value, _lib.FsError), call
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.start_averaging())
        mean = sim._averager.mean
        h = mean._h
        v, p = sim._solver.get_fields()[:2]
        # the library refuses on its own as well (FS_ERR_STATE = -3), and checks channel counts
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_mean_read(dev._ctx, h, None, ctypes.byref(launches), ctypes.byref(samples)),
                  dev._lib.fs_mean_reset(dev._ctx, h), dev._lib.fs_mean_finalize(dev._ctx, h, v._h, p._h)]
            hh = ctypes.c_void_p()
            st.append(dev._lib.fs_mean_create(dev._ctx, 1, 0, ctypes.byref(hh)))
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3, -3, -3, -3]
        with pytest.raises(_lib.FsError):
            _lib.call("fs_mean_accumulate", dev._ctx, h, 0.0, p._h, v._h)
        with pytest.raises(_lib.FsError):
            _lib.call("fs_mean_create", dev._ctx, 0, 0, ctypes.byref(ctypes.c_void_p()))
        assert sim.averages()["samples"] == 3                   # nothing of the above counted or cleared anything
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        gid = dev.capture(lambda: (dev.mean_accumulate(mean, v, p), sim.stop_averaging()))
        dev.free_graph(gid)
        assert sim._averager is None and mean._h is None
        with pytest.raises(_lib.FsError):                       # the handle is gone
            _lib.call("fs_mean_read", dev._ctx, h, None, ctypes.byref(launches), ctypes.byref(samples))
        m2 = dev.mean_create()
        with pytest.raises(_lib.FsError):                       # no sample yet: finalize has nothing to divide by
            dev.mean_finalize(m2, dev.alloc(2), dev.alloc(1))
        dev.mean_free(m2)
        sim.start_averaging()
        sim.run(5, graph=True)
        assert sim.averages()["samples"] == 5
    finally:
        _close(sim)


def test_resume_equals_uninterrupted_run(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b, c = make_product(g, cfg), make_product(g, cfg), None
    try:
        every, start = 3, 5
        a.start_averaging(every=every, start_step=start)
        a.run(50, graph=True)
        b.start_averaging(every=every, start_step=start)
        b.run(23, graph=True)
        sums, launches, samples = _read(b)
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
        c.start_averaging(every=every, start_step=start)
        c._dev.mean_write(c._averager.mean, sums, launches, samples)
        c.run(27, graph=True)
        ra, rc = _read(a), _read(c)
        assert ra[1:] == rc[1:] == (50, 15)
        _assert_sums_equal(rc[0], ra[0], "resumed ")
        fa, fc = a.field_to_numpy(), c.field_to_numpy()
        assert all(np.array_equal(fa[k], fc[k]) for k in fa)
    finally:
        for sim in (a, b, c):
            if sim is not None:
                _close(sim)


# ---- slab contexts on one GPU (the thread harness of test_gpu_slab_threads.py), tape replays -------------------------------------
def _slab_means(const, mask, cfg, world, halo, every, start, steps, want_rows=None):
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
            if want_rows is not None:
                rows = dev.diag_rows()
                assert (rows["mean_accumulate"], rows["mean_finalize"]) == want_rows, f"rank {rank}: {rows}: the test does not cover {want_rows}"
            bc = fs.BoundaryCondition(const, mask, device=dev)
            vc = fs.VorticityConfinement(bc, dt, dx, cfg["vor_eps"])
            pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
            sim = fs.FluidSimulator(fs.CipMacSolver(bc, pu, dt, dx, re, vc))
            sim.start_averaging(every=every, start_step=start)
            sim.run(steps)
            sums, launches, samples = dev.mean_read(sim._averager.mean, local=True)
            avg = sim.averages(local=True)
            results[rank] = (sums, launches, samples, len(sim._tapes), dev.nyl, avg["u"])
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


@pytest.mark.parametrize("world,halo", [(2, 4), (3, 4)])
def test_slab_contexts_match_single_context(world, halo, hip_lib):
    """bc5 at res 45: 90 x 45 cells, slabs of 23 + 22 / 15 + 15 + 15 rows - partial row groups of the kernel in every slab layout."""
    _slab_case(world, halo)


def _slab_case(world, halo, want_rows=None):
    import fs
    from fs.averages import derive_averages
    from fs.boundary_condition import BoundaryCondition, create_scene_arrays
    res = 45
    const, mask, _ = create_scene_arrays(5, res)
    cfg = dict(dt=0.05 / res, dx=1.0 / res, re=1.0e6, vor_eps=5.0)
    every, start, steps = 3, 7, 70
    fs.runtime.init(gpu=0, dtype="f32")
    bc = BoundaryCondition(const, mask)
    one = fs.FluidSimulator(fs.CipMacSolver(bc, fs.RedBlackSorPressureUpdater(bc, cfg["dt"], cfg["dx"], 1.3, 2), cfg["dt"], cfg["dx"], cfg["re"],
                                            fs.VorticityConfinement(bc, cfg["dt"], cfg["dx"], cfg["vor_eps"])))
    try:
        one.start_averaging(every=every, start_step=start)
        one.run(steps, graph=False)
        exp, launches, samples = _read(one)
    finally:
        _close(one)
    assert (launches, samples) == (70, 21) and np.abs(exp[5]).max() > 0.0
    res_ = _slab_means(const, mask, cfg, world, halo, every, start, steps, want_rows)
    assert all(r[3] > 0 for r in res_), "no tape was replayed"
    assert any(r[4] % 2 for r in res_), "every slab holds whole row groups: the partial group is not covered"
    assert all(r[1:3] == (launches, samples) for r in res_)
    got = np.concatenate([r[0] for r in res_], axis=2)
    _assert_sums_equal(got, exp, "assembled slab ")
    u = np.concatenate([r[5] for r in res_], axis=1)
    assert np.array_equal(u, derive_averages(exp, samples, mask)["u"])


# ---- 8 rows per workgroup: the forms of large grids, forced onto small ones by FS_DIAG_WGS ------------------------------------------------
# k_mean_accumulate takes 4 or 8 rows per workgroup in load groups of 4 (csrc/fs_mean.h MEAN_G), k_mean_finalize 1, 2, 4 or 8; without the
# switch every grid below 2048 workgroups takes 4 and 1.  Both kernels double by the same rule, so that the accumulation takes 8 rows exactly
# where the finalize pass does: the floors for 2 and 4 rows of the finalize pass leave the accumulation at 4.
MEAN_G, MEAN_ROWS = 4, 8


def _mean_floor(X, Y, finalize_rows):
    return diag_floor(-(-X // (512 if X % 2 == 0 else 256)), Y, 1, finalize_rows)


@pytest.mark.parametrize("finalize_rows", [2, 4, 8])
@pytest.mark.parametrize("X,Y,dtype", [(102, 9, "f32"), (102, 13, "f32"), (101, 13, "f32"), (101, 37, "f32"), (1026, 37, "f32"),
                                       (102, 13, "f64"), (101, 37, "f64")])
def test_odd_sizes_rows_per_workgroup(X, Y, dtype, finalize_rows, hip_lib, monkeypatch):
    """Heights of 9, 13 and 37 rows: a workgroup of 8 rows holds two load groups, the last workgroup a partial one (1 and 5 rows)."""
    monkeypatch.setenv("FS_DIAG_WGS", str(_mean_floor(X, Y, finalize_rows)))
    _odd_sizes_case(X, Y, dtype, want_rows=(MEAN_ROWS if finalize_rows == MEAN_ROWS else MEAN_G, finalize_rows))


def test_deferred_limit_reaches_the_sums_eight_rows(hip_lib, monkeypatch):
    monkeypatch.setenv("FS_DIAG_WGS", "1")
    _deferred_limit_case(want_rows=MEAN_ROWS)


def test_slab_contexts_eight_rows(hip_lib, monkeypatch):
    """Three slabs of 15 rows: a whole workgroup of 8 rows and one of 7, whose second group holds 3."""
    monkeypatch.setenv("FS_DIAG_WGS", "1")
    _slab_case(3, 4, want_rows=(MEAN_ROWS, MEAN_ROWS))


def test_simulator_with_the_most_rows_per_workgroup(hip_lib, monkeypatch):
    """FS_DIAG_WGS=1 through FluidSimulator (32 / 8 / 8 rows per workgroup) against a twin with the switch unset (4 / 4 / 1): the averages
    and the fields bit for bit, flow_stats within the reduction order."""
    import fs
    from flow_stats_ref import compare, flow_stats_ref
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    b = make_product(g, cfg)
    monkeypatch.setenv("FS_DIAG_WGS", "1")
    a = make_product(g, cfg)
    try:
        assert a._dev.diag_rows() == {"flow_stats": 32, "mean_accumulate": 8, "mean_finalize": 8}, "the switch did not reach the context"
        assert b._dev.diag_rows() == {"flow_stats": 4, "mean_accumulate": 4, "mean_finalize": 1}
        for sim in (a, b):
            sim.start_averaging(every=3)
            sim.run(43, graph=True)
        assert a._graphs, "the run replayed no graph"
        oa, ob = a.averages(), b.averages()
        assert set(oa) == set(ob) and oa["samples"] == 14
        for k in oa:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), f"averages: {k}"
        sa, sb = _read(a), _read(b)
        assert sa[1:] == sb[1:] == (43, 14)
        _assert_sums_equal(sa[0], sb[0], "most rows per workgroup: ")
        assert np.abs(sa[0][5]).max() > 0.0
        box = default_body_box(cfg["bc"], cfg["res"])
        va, pa = a._solver.get_fields()[:2]
        vb, pb = b._solver.get_fields()[:2]
        ra, rb = a._dev.flow_stats(cfg["dx"], va, pa, box), b._dev.flow_stats(cfg["dx"], vb, pb, box)
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        ref = flow_stats_ref(fb["v"], fb["p"], g["bc_mask"], cfg["dx"], box)
        assert not compare(rb, ref), compare(rb, ref)
        assert not compare(ra, dict(rb, _force_scale=ref["_force_scale"])), compare(ra, rb)
        assert rb["force_x"] != 0.0 and rb["sum_om2"] > 0.0
        for k in fa:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{k}: the fields differ"
    finally:
        _close(a)
        _close(b)
