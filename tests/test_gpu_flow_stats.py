"""Flow diagnostics on the GPU (include/fs_hip.h fs_flow_stats, FluidSimulator.flow_stats): the kernel against the NumPy f64 restatement
(tests/flow_stats_ref.py) on golden and developed states, closed forms uploaded by hand, NaN handling, determinism, no side effect on the
trajectory (eager, replayed graphs, a pending deferred limit pass), refusal during a capture, and slab contexts on one GPU; and the kernel
with 8, 16 and 32 rows per workgroup - the forms of large grids - forced onto small grids by FS_DIAG_WGS."""
import os
import threading

import numpy as np
import pytest
from conftest import GOLDEN
from flow_stats_ref import SLOTS, compare, flow_stats_ref
from helpers import dead_buffers, diag_floor, make_product, traj_config

pytestmark = pytest.mark.gpu

_STATE = ("v", "p", "vx", "vy", "dye", "dyex", "dyey")


def _raw(sim, box=None):
    s = sim._solver
    v, p = s.get_fields()[:2]
    return s._bc.device.flow_stats(s.dx, v, p, box)


def _check_against_ref(sim, box):
    s = sim._solver
    got = _raw(sim, box)
    out = sim.field_to_numpy()
    exp = flow_stats_ref(out["v"], out["p"], s._bc._host_mask, s.dx, box)
    bad = compare(got, exp)
    assert not bad, bad
    return got, exp


TRAJ = ["traj_bc1_upwind_vc0.npz", "traj_bc1_cip_vc5.npz", "traj_bc2_kk_vc5.npz", "traj_bc3_kk_vc5.npz", "traj_bc4_cip_vc5.npz",
        "traj_bc5_cip_vc5.npz", "traj_bc5_upwind_vc5.npz", "traj_dye_bc5_kk_vc5.npz", "traj_f64_bc1_cip_vc0.npz",
        "traj_f64_bc3_kk_vc0_re1e8.npz", "traj_cfg5_bc3_res96_kk_vc10_re1e8.npz"]


@pytest.mark.parametrize("fname", TRAJ)
def test_kernel_matches_reference_on_developed_states(fname, hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g = np.load(os.path.join(GOLDEN, fname))
    cfg = traj_config(g)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    sim = make_product(g, cfg)
    try:
        box = default_body_box(cfg["bc"], cfg["res"]) if cfg["bc"] in (1, 3, 5) else (3, 3, cfg["res"], cfg["res"] - 3)
        for steps in (0, 3, 12):
            for _ in range(steps):
                sim.step()
            _check_against_ref(sim, None)
            got, exp = _check_against_ref(sim, box)
            if steps and cfg["bc"] in (1, 3, 5):
                assert got["force_x"] != 0.0
        assert got["fluid_cells"] == float((g["bc_mask"] == 0).sum())
    finally:
        sim._solver._bc.device.close()


@pytest.mark.parametrize("bc,res,scheme,dtype", [(1, 33, "cip", "f32"), (5, 45, "kk", "f64"), (3, 64, "upwind", "f32"), (5, 256, "cip", "f32")])
def test_kernel_matches_reference_on_created_scenes(bc, res, scheme, dtype, hip_lib):
    """Odd widths, a width that is not a multiple of 256 lanes, several row blocks of the kernel."""
    import fs
    from fs.boundary_condition import default_body_box
    fs.runtime.init(gpu=0, dtype=dtype)
    sim = fs.FluidSimulator.create(bc, res, 0.05 / res, 1.0 / res, 1e6, 5.0, scheme)
    try:
        for _ in range(10):
            sim.step()
        _check_against_ref(sim, None)
        _check_against_ref(sim, default_body_box(bc, res))
    finally:
        sim._solver._bc.device.close()


def test_golden_kernel_inputs(hip_lib):
    """The per-kernel golden inputs (states drawn by the fixture generator, not by a run) on every scene."""
    import fs
    from fs.boundary_condition import BoundaryCondition
    for n in (1, 2, 3, 4, 5):
        g = np.load(os.path.join(GOLDEN, f"kernels_bc{n}.npz"))
        dx = float(g["params"][2])          # (params: res, dt, dx, Re, vorticity weight, omega)
        fs.runtime.init(gpu=0)
        bc = BoundaryCondition(g["bc_const"], g["bc_mask"])
        dev = bc.device
        try:
            v, p = dev.alloc(2), dev.alloc(1)
            v.from_numpy(g["mac_update_kk.in.vc"])
            p.from_numpy(g["mac_update_kk.in.pc"])
            for box in (None, (0, 0) + g["bc_mask"].shape):
                got = dev.flow_stats(dx, v, p, box)
                exp = flow_stats_ref(v.to_numpy(), p.to_numpy(), g["bc_mask"], dx, box)
                assert not compare(got, exp), (n, box, compare(got, exp))
        finally:
            dev.close()


def _custom(mask, dtype="f32"):
    import fs
    from fs.boundary_condition import BoundaryCondition
    fs.runtime.init(gpu=0, dtype=dtype)
    X, Y = mask.shape
    return BoundaryCondition(np.zeros((X, Y, 2), np.float32), mask).device


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_closed_forms_uploaded(dtype, hip_lib):
    X, Y, dx = 300, 40, 1.0 / 64          # (300: two column blocks, the second partly outside the grid)
    mask = np.ones((X, Y), np.uint8)
    mask[1:-1, 1:-1] = 0
    dev = _custom(mask, dtype)
    try:
        i, j = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), indexing="ij")
        v, p = dev.alloc(2), dev.alloc(1)
        v.from_numpy(np.stack([-(j * dx), i * dx], axis=2))
        p.fill(0.0)
        d = dev.flow_stats(dx, v, p)
        n = (X - 2) * (Y - 2)
        assert d["fluid_cells"] == n and d["sum_om2"] == 4.0 * n and d["sum_dv2"] == 0.0 and d["max_abs_dv"] == 0.0
        assert d["nonfinite"] == 0 and d["force_x"] == 0.0 and d["force_y"] == 0.0
    finally:
        dev.close()
    # a square body of side L in p = c i
    L, c = 5, 0.25
    mask = np.zeros((X, Y), np.uint8)
    mask[100:100 + L, 20:20 + L] = 1
    dev = _custom(mask, dtype)
    try:
        v, p = dev.alloc(2), dev.alloc(1)
        v.fill(0.0)
        p.from_numpy(c * np.arange(X, dtype=np.float64)[:, None] * np.ones((1, Y)))
        d = dev.flow_stats(dx, v, p, (98, 18, 100 + L + 2, 20 + L + 2))
        assert d["force_x"] == -(L + 1) * L * c * dx and d["force_y"] == 0.0
        assert dev.flow_stats(dx, v, p)["force_x"] == 0.0            # no box
        p.fill(3.5)
        d = dev.flow_stats(dx, v, p, (0, 0, X, Y))
        assert d["force_x"] == 0.0 and d["force_y"] == 0.0
    finally:
        dev.close()


def test_nan_and_inf(hip_lib):
    import math
    X, Y, dx = 128, 64, 1.0 / 64
    mask = np.zeros((X, Y), np.uint8)
    mask[40:50, 20:30] = 1
    dev = _custom(mask)
    try:
        rng = np.random.default_rng(5)
        v0 = rng.standard_normal((X, Y, 2)).astype(np.float32)
        p0 = rng.standard_normal((X, Y)).astype(np.float32)
        v, p = dev.alloc(2), dev.alloc(1)
        v.from_numpy(v0)
        pp = p0.copy()
        pp[10, 10] = np.nan          # fluid cell, read by no sum
        pp[45, 25] = np.nan          # wall cell inside the body: not counted
        p.from_numpy(pp)
        box = (38, 18, 52, 32)
        d = dev.flow_stats(dx, v, p, box)
        assert d["nonfinite"] == 1 and math.isfinite(d["sum_s2"]) and math.isfinite(d["force_x"])
        pp[39, 25] = np.nan          # fluid neighbour of the body: the force reads it
        p.from_numpy(pp)
        d = dev.flow_stats(dx, v, p, box)
        assert d["nonfinite"] == 2 and math.isnan(d["force_x"]) and math.isfinite(d["force_y"])
        vv = v0.copy()
        vv[70, 30, 1] = np.nan
        v.from_numpy(vv)
        d = dev.flow_stats(dx, v, p, box)
        exp = flow_stats_ref(vv, pp, mask, dx, box)
        assert not compare(d, exp), compare(d, exp)
        for k in ("sum_s2", "sum_om2", "sum_dv2", "max_s2", "max_a", "max_abs_dv"):
            assert math.isnan(d[k]), k
        vv[70, 30, 1] = np.inf
        v.from_numpy(vv)
        d = dev.flow_stats(dx, v, p, box)
        assert d["max_s2"] == math.inf and d["max_a"] == math.inf and d["nonfinite"] == 3
    finally:
        dev.close()


def test_deterministic(hip_lib):
    import fs
    fs.runtime.init(gpu=0)
    sim = fs.FluidSimulator.create(5, 256, 0.05 / 256, 1.0 / 256, 1e6, 5.0, "cip")
    try:
        for _ in range(20):
            sim.step()
        from fs.boundary_condition import default_body_box
        box = default_body_box(5, 256)
        a, b = sim.flow_stats(box), sim.flow_stats(box)
        assert repr(a) == repr(b)
        assert set(a) == {"kinetic_energy", "enstrophy", "max_speed", "cfl", "div_rms", "div_max", "nonfinite", "fluid_cells", "force_x", "force_y"}
        assert a["nonfinite"] == 0 and a["kinetic_energy"] > 0 and 0 < a["cfl"] < 1
    finally:
        sim._solver._bc.device.close()


def _full_state(sim):
    s = sim._solver
    out = {}
    for name in _STATE:
        if hasattr(s, name):
            for which in ("current", "next"):
                if f"{name}.{which}" not in dead_buffers(s):
                    out[f"{name}.{which}"] = getattr(getattr(s, name), which).to_numpy()
    vc = s.vorticity_confinement
    if vc is not None:
        out["vorticity"], out["vorticity_abs"] = vc.vorticity.to_numpy(), vc.vorticity_abs.to_numpy()
    return out


@pytest.mark.parametrize("bc,res,scheme,vc,dye,mode", [(5, 64, "cip", 5.0, False, "eager"), (5, 64, "cip", 5.0, False, "graph"),
                                                      (1, 96, "upwind", None, False, "eager"), (2, 64, "kk", 5.0, True, "graph"),
                                                      (5, 512, "cip", 5.0, False, "graph")])
def test_no_side_effects(bc, res, scheme, vc, dye, mode, hip_lib, monkeypatch):
    """200 steps with flow_stats() after every step (eager) / 16 chunks of 20 steps with a sample in front of each (graph) against the same steps without it: the full state is
    bit-identical.  With deferred limit passes the velocity still owes its limit pass when flow_stats is called."""
    import fs
    monkeypatch.setenv("FS_LIMIT_DEFER", "1")
    states, pending, ncached = [], 0, []
    for with_stats in (True, False):
        fs.runtime.init(gpu=0)
        cls = fs.DyeFluidSimulator if dye else fs.FluidSimulator
        sim = cls.create(bc, res, 0.05 / res, 1.0 / res, 1e6, vc, scheme)
        try:
            if mode == "eager":
                for _ in range(200):
                    sim.step()
                    if with_stats:
                        pending += sim._solver.v.current.pending_limit is not None
                        sim.flow_stats()
            else:
                dev, captures = sim._solver._bc.device, []
                real_capture = dev.capture
                dev.capture = lambda fn: captures.append(1) or real_capture(fn)
                per_chunk = []
                for _ in range(16):
                    if with_stats:
                        pending += sim._solver.v.current.pending_limit is not None
                        sim.flow_stats()
                    n0 = len(captures)
                    sim.run(20, graph=True)
                    per_chunk.append(len(captures) - n0)
                ncached.append(per_chunk)
            states.append(_full_state(sim))
        finally:
            sim._solver._bc.device.close()
    for k in states[1]:
        assert np.array_equal(states[0][k], states[1][k], equal_nan=True), k
    if not dye:
        assert pending > 0, "no call met a pending limit pass"
    if mode == "graph":
        # a sample leaves the velocity's deferred limit pass deferred (the flag is down): the chunks find the graphs they would find without it
        assert ncached[0] == ncached[1], f"sampling changed which chunks capture a graph: captures per chunk {ncached}"


def test_refused_during_capture(hip_lib):
    import fs
    from fs._lib import FsError
    fs.runtime.init(gpu=0)
    sim = fs.FluidSimulator.create(5, 64, 0.05 / 64, 1.0 / 64, 1e6, 5.0, "cip")
    ref = fs.FluidSimulator.create(5, 64, 0.05 / 64, 1.0 / 64, 1e6, 5.0, "cip")
    try:
        for s in (sim, ref):
            for _ in range(3):
                s.step()
        dev = sim._solver._bc.device
        with pytest.raises(FsError):
            dev.capture(lambda: sim.flow_stats())
        v, p = sim._solver.get_fields()[:2]
        with pytest.raises(FsError, match="status -3"):          # the library's own refusal: FS_ERR_STATE
            dev.capture(lambda: dev._p_flow_stats(1.0 / 64, v._h, p._h, None))
        assert sim.flow_stats() == ref.flow_stats()          # the context still works and nothing was lost
        for s in (sim, ref):
            for _ in range(3):
                s.step()
        a, b = sim.field_to_numpy(), ref.field_to_numpy()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    finally:
        sim._solver._bc.device.close()
        ref._solver._bc.device.close()


# ---- slab contexts on one GPU, driven by threads (the exchange through host memory, as tests/test_gpu_slab_threads.py) -------------------
def _slab_device_cls(world, shared):
    from test_gpu_slab_threads import _make_device_cls
    Base = _make_device_cls(world, shared)

    class StatsThreadSlabDevice(Base):
        def _p_allreduce(self, values):
            shared["sums"][self.rank] = list(values)
            shared["barrier"].wait()
            out = tuple(_ordered_sum(col) for col in zip(*shared["sums"]))
            shared["barrier"].wait()
            return out

    return StatsThreadSlabDevice


def _ordered_sum(col):
    t = 0.0
    for x in col:
        t += x
    return t


def _slab_worker(rank, world, halo, g, cfg, steps, box, Dev, results, errors, want_rows=None):
    try:
        from fs.boundary_condition import BoundaryCondition
        X, Y = g["bc_mask"].shape
        dev = Dev(X, Y, np.float64 if cfg["fp64"] else np.float32, rank, halo)
        if want_rows is not None:
            assert dev.diag_rows()["flow_stats"] == want_rows, (f"rank {rank} ({dev.nyl} rows): {dev.diag_rows()['flow_stats']} rows per "
                                                                f"workgroup, not {want_rows}: the test does not cover it")
        bc = BoundaryCondition(g["bc_const"], g["bc_mask"], device=dev)
        import fs
        dt, dx, re = cfg["dt"], cfg["dx"], cfg["re"]
        vc = fs.VorticityConfinement(bc, dt, dx, cfg["vor_eps"]) if cfg["vor_eps"] is not None else None
        u = cfg["updater"]
        pu = (fs.RedBlackSorPressureUpdater(bc, dt, dx, u[1], u[2]) if u[0] == "rbsor" else fs.JacobiPressureUpdater(bc, dt, dx, u[1]))
        if cfg["scheme"] == "cip":
            solver = fs.CipMacSolver(bc, pu, dt, dx, re, vc)
        else:
            solver = fs.MacSolver(bc, pu, fs.advect_upwind if cfg["scheme"] == "upwind" else fs.advect_kk_scheme, dt, dx, re, vc)
        for _ in range(steps):
            solver.update()
        v, p = solver.get_fields()[:2]
        results[rank] = dev.flow_stats(dx, v, p, box)
        dev.close()
    except BaseException as e:   # noqa: BLE001 - surface in the main thread
        errors.append((rank, repr(e)))
        try:
            shared = threading.current_thread()._fs_shared
            shared["barrier"].abort()
        except Exception:
            pass


def _scene_case(bc, res):
    """(arrays, config) of a created scene in the form of a golden trajectory's (CIP + VC 5, RB-SOR(1.3, 2), f32)."""
    from fs.boundary_condition import create_scene_arrays
    const, mask, dye = create_scene_arrays(bc, res)
    cfg = dict(bc=bc, res=res, dt=0.05 / res, dx=1.0 / res, re=1e6, vor_eps=5.0, scheme="cip", updater=("rbsor", 1.3, 2), dye=False,
               fp64=False, snaps=[])
    return {"bc_const": const, "bc_mask": mask, "bc_dye": dye}, cfg


# Y = 32 on 2 / 4 ranks gives slabs of 16 / 8 rows, a whole number of the kernel's 4-row load groups.  Y = 64 on 3 ranks (22, 21, 21 rows)
# and on 5 ranks (13, 13, 13, 13, 12) end the lower slabs' last workgroup in a partial group, with ghost rows of depth 2 and 3 only beyond it.
@pytest.mark.parametrize("fname,world,halo", [("traj_bc5_cip_vc5.npz", 2, 2), ("traj_bc5_cip_vc5.npz", 4, 4),
                                              ("traj_bc1_upwind_vc0.npz", 4, 2), ("traj_f64_bc1_cip_vc0.npz", 2, 4),
                                              ((5, 64), 3, 2), ((5, 64), 3, 3), ((1, 64), 5, 2)])
def test_slab_contexts_match_single_context(fname, world, halo, hip_lib):
    _slab_case(fname, world, halo)


def _slab_case(fname, world, halo, want_rows=None):
    import fs
    from fs.boundary_condition import default_body_box
    if isinstance(fname, tuple):
        g, cfg = _scene_case(*fname)
    else:
        g = np.load(os.path.join(GOLDEN, fname))
        cfg = traj_config(g)
    steps = 8
    box = default_body_box(cfg["bc"], cfg["res"])
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    single = make_product(g, cfg)
    for _ in range(steps):
        single.step()
    exp = _raw(single, box)
    out = single.field_to_numpy()
    assert not compare(exp, flow_stats_ref(out["v"], out["p"], g["bc_mask"], cfg["dx"], box))
    single._solver._bc.device.close()
    shared = {"barrier": threading.Barrier(world), "box": [None] * world, "radii": [None] * world, "sums": [None] * world}
    Dev = _slab_device_cls(world, shared)
    results, errors, threads = [None] * world, [], []
    for r in range(world):
        t = threading.Thread(target=_slab_worker, args=(r, world, halo, g, cfg, steps, box, Dev, results, errors, want_rows))
        t._fs_shared = shared
        threads.append(t)
        t.start()
    for t in threads:
        t.join(timeout=900)
    assert not errors, errors
    for r in range(world):
        bad = compare(results[r], dict(exp, _force_scale=flow_stats_ref(out["v"], out["p"], g["bc_mask"], cfg["dx"], box)["_force_scale"]))
        assert not bad, (r, bad)
    assert [results[r] for r in range(world)] == [results[0]] * world      # every rank holds the same global values
    assert set(results[0]) == set(SLOTS)


# ---- 8, 16 and 32 rows per workgroup: the forms of large grids, forced onto small ones by FS_DIAG_WGS ------------------------------------
# A workgroup takes `rpw` rows in load groups of 4 (csrc/fs_stats.h STATS_G) and carries rows j - 1 and j in registers from one group to the
# next; without the switch every grid below 2048 workgroups takes rpw = 4, one group per workgroup.
STATS_G, STATS_ROWS = 4, 32
RPW = (4, 8, 16, 32)
# the smallest heights at which a workgroup of 8 / 16 / 32 rows has two groups, its last group 1, 3 or 4 rows, the last workgroup one row
HEIGHTS = (9, 12, 13, 16, 17, 33, 37, 64, 65, 70)
WIDTHS = (33, 300)          # (300: two column blocks, the second partly outside the grid)


def _forced_device(monkeypatch, mask, dtype, rpw):
    """A device on `mask` whose fs_flow_stats launches take `rpw` rows per workgroup."""
    X, Y = mask.shape
    monkeypatch.setenv("FS_DIAG_WGS", str(diag_floor(-(-X // 256), Y, STATS_G, rpw)))
    dev = _custom(mask, dtype)
    got = dev.diag_rows()["flow_stats"]
    if got != rpw:
        dev.close()
        raise AssertionError(f"{X} x {Y}: k_flow_stats would take {got} rows per workgroup, not {rpw}: the test does not cover it")
    return dev


def _rpws(Y):
    return [r for r in RPW if r == STATS_G or Y > r]          # (Y <= rpw: one workgroup, one partial group - nothing to distinguish)


def _random_mask(rng, X, Y):
    """Walls, inflow and outflow cells, and a solid block."""
    mask = (rng.random((X, Y)) < 0.25).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.05] = 2
    mask[rng.random((X, Y)) < 0.05] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


def _thin_wall_mask(rng, X, Y):
    """Fluid with a few inflow / outflow cells and one-cell-thin horizontal walls in the first and the last row of every load group - among
    them the first and the last row of every workgroup of 8, 16 and 32 rows - with fluid above and below (the two kinds of rows use
    different columns).  Wider grids carry a second set across the edge of the first column block."""
    mask = np.zeros((X, Y), np.uint8)
    mask[rng.random((X, Y)) < 0.02] = 2
    mask[rng.random((X, Y)) < 0.02] = 3
    spans = [((2, 12), (16, 26))] + ([((250, 258), (262, 270))] if X >= 272 else [])
    for j in range(Y):
        for last_row, first_row in spans:
            for (a, b), rem in ((first_row, 0), (last_row, STATS_G - 1)):
                if j % STATS_G == rem:
                    mask[a:b, j] = 1
                    mask[(a + b) // 2:(a + b) // 2 + 2, j] = 0          # (a gap of two cells: more faces that push along x)
                    for jn in (j - 1, j + 1):
                        if 0 <= jn < Y:
                            mask[a:b, jn] = 0
    return mask


def _boxes(X, Y):
    """Body boxes over the walls whose y0 / y1 lie on multiples of 4, 8 and 32, one row above and one row below them."""
    ys = sorted({0, Y} | {m + d for m in (4, 8, 32) for d in (-1, 0, 1) if m + d < Y})
    return [(1, y0, X - 1, y1) for y0 in ys for y1 in ys if y0 < y1]


def _integer_fields(rng, X, Y, dtype):
    dt_ = np.float32 if dtype == "f32" else np.float64
    return rng.integers(-8, 9, (X, Y, 2)).astype(dt_), rng.integers(-8, 9, (X, Y)).astype(dt_)


def _slots(d):
    return [float(d[k]) for k in SLOTS]


@pytest.mark.parametrize("Y", HEIGHTS)
@pytest.mark.parametrize("X", WIDTHS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rows_per_workgroup_random_fields(dtype, X, Y, hip_lib, monkeypatch):
    rng = np.random.default_rng(X * 1000 + Y)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = _random_mask(rng, X, Y)
    va, pa = (rng.standard_normal((X, Y, 2)) * 3).astype(dt_), rng.standard_normal((X, Y)).astype(dt_)
    dx = 1.0 / 48
    boxes = [None, (0, 0, X, Y), (3, 3, X - 2, Y - 2)]
    exp = [flow_stats_ref(va, pa, mask, dx, box) for box in boxes]
    assert exp[1]["force_x"] != 0.0 and exp[1]["force_y"] != 0.0 and exp[0]["fluid_cells"] > 0
    for rpw in _rpws(Y):
        dev = _forced_device(monkeypatch, mask, dtype, rpw)
        try:
            v, p = dev.alloc(2), dev.alloc(1)
            v.from_numpy(va)
            p.from_numpy(pa)
            for box, e in zip(boxes, exp):
                got = dev.flow_stats(dx, v, p, box)
                print(f"rpw {rpw} box {box}: {_slots(got)}")
                assert not compare(got, e), (rpw, box, compare(got, e))
        finally:
            dev.close()


@pytest.mark.parametrize("Y", HEIGHTS)
@pytest.mark.parametrize("X", WIDTHS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rows_per_workgroup_integer_fields_exact(dtype, X, Y, hip_lib, monkeypatch):
    """u, w, p integers in [-8, 8] and dx = 1/64: every term and every sum is exact in double, whatever the order - the ten slots equal the
    reference's and each other's across the rows per workgroup."""
    rng = np.random.default_rng(X * 1000 + Y + 7)
    mask = _thin_wall_mask(rng, X, Y)
    va, pa = _integer_fields(rng, X, Y, dtype)
    dx = 1.0 / 64
    boxes = _boxes(X, Y)
    exp = [flow_stats_ref(va, pa, mask, dx, box) for box in boxes]
    whole = boxes.index((1, 0, X - 1, Y))
    assert exp[whole]["force_x"] != 0.0 and exp[whole]["force_y"] != 0.0, "the forces vanish: the case does not cover them"
    results = {}
    for rpw in _rpws(Y):
        dev = _forced_device(monkeypatch, mask, dtype, rpw)
        try:
            v, p = dev.alloc(2), dev.alloc(1)
            v.from_numpy(va)
            p.from_numpy(pa)
            results[rpw] = [_slots(dev.flow_stats(dx, v, p, box)) for box in boxes]
        finally:
            dev.close()
        for box, got, e in zip(boxes, results[rpw], exp):
            assert got == _slots(e), (rpw, box, got, _slots(e))
    assert all(r == results[STATS_G] for r in results.values())


def test_natural_size_takes_eight_rows(hip_lib, monkeypatch):
    """16384 x 264 with the switch unset: 64 * ceil(264 / 8) = 2112 >= 2048 > 64 * ceil(264 / 16) - 8 rows per workgroup by the rule itself;
    1024 x 512 stays at 4 / 4 / 1: the default floor."""
    from fs.runtime import Device
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    small = Device(1024, 512, "f32")
    try:
        assert small.diag_rows() == {"flow_stats": 4, "mean_accumulate": 4, "mean_finalize": 1}
    finally:
        small.close()
    X, Y = 16384, 264
    rng = np.random.default_rng(16384)
    mask = _thin_wall_mask(rng, X, Y)
    va, pa = _integer_fields(rng, X, Y, "f32")
    dx, box = 1.0 / 64, (1, 7, X - 1, Y - 9)
    dev = _custom(mask, "f32")
    try:
        assert dev.diag_rows()["flow_stats"] == 8, f"{dev.diag_rows()}: not 8 rows per workgroup: the test does not cover it"
        v, p = dev.alloc(2), dev.alloc(1)
        v.from_numpy(va)
        p.from_numpy(pa)
        got = dev.flow_stats(dx, v, p, box)
    finally:
        dev.close()
    exp = flow_stats_ref(va, pa, mask, dx, box)
    assert exp["force_x"] != 0.0 and exp["force_y"] != 0.0
    assert _slots(got) == _slots(exp), (_slots(got), _slots(exp))


def test_the_switch_reaches_the_launch(hip_lib, monkeypatch):
    """Random f32 fields summed by workgroups of 32 rows and of 4: the terms are the same, the trees are not - at least one of the three
    sums differs in its last bits.  If none does, the forced rows did not reach the kernel."""
    X, Y, dx = 300, 70, 1.0 / 48
    rng = np.random.default_rng(300070)
    mask = _random_mask(rng, X, Y)
    va, pa = (rng.standard_normal((X, Y, 2)) * 3).astype(np.float32), rng.standard_normal((X, Y)).astype(np.float32)
    got = {}
    for rpw in (4, 32):
        dev = _forced_device(monkeypatch, mask, "f32", rpw)
        try:
            v, p = dev.alloc(2), dev.alloc(1)
            v.from_numpy(va)
            p.from_numpy(pa)
            got[rpw] = dev.flow_stats(dx, v, p, (0, 0, X, Y))
        finally:
            dev.close()
    assert not compare(got[32], got[4]), compare(got[32], got[4])
    sums = ("sum_s2", "sum_om2", "sum_dv2")
    assert any(got[32][k] != got[4][k] for k in sums), "32 and 4 rows per workgroup gave the same bits in every sum"


# slabs of 22 / 21 rows (3 ranks) and 13 / 12 rows (5 ranks): partial last groups behind whole ones, ghost rows of depth 2 and 3 beyond them
@pytest.mark.parametrize("rpw", [8, 32])
@pytest.mark.parametrize("fname,world,halo", [((5, 64), 3, 2), ((5, 64), 3, 3), ((1, 64), 5, 2)])
def test_slab_contexts_rows_per_workgroup(fname, world, halo, rpw, hip_lib, monkeypatch):
    from fs.boundary_condition import create_scene_arrays
    from fs.runtime import slab_rows
    X, Y = create_scene_arrays(*fname)[1].shape
    heights = [slab_rows(Y, r, world)[1] for r in range(world)]
    floors = {diag_floor(-(-X // 256), n, STATS_G, rpw) for n in heights}
    assert len(floors) == 1, f"slabs of {heights} rows need different floors for {rpw} rows per workgroup: {floors}"
    monkeypatch.setenv("FS_DIAG_WGS", str(floors.pop()))
    _slab_case(fname, world, halo, want_rows=rpw)
