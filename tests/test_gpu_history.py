"""Per-step history on the GPU (csrc/fs_history.h k_history_record, include/fs_hip.h fs_history_*, FluidSimulator.record_history):
probe values bit for bit against downloads of an eagerly stepped twin, forces against flow_stats and a NumPy sum, unchanged trajectories,
a tiny ring across graph replays, the deferred limit pass, slab contexts on one GPU with tape replays, refusals."""
import ctypes
import os
import threading

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config

pytestmark = pytest.mark.gpu


def _load(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    return g, traj_config(g)


def _probes(mask, n=6, seed=0):
    fluid = np.argwhere(np.asarray(mask) == 0)
    idx = np.random.default_rng(seed).choice(len(fluid), n, replace=False)
    return [tuple(int(c) for c in fluid[k]) for k in sorted(idx)]


def _at(sim, probes):
    d = sim.field_to_numpy()
    return np.array([[d["v"][x, y, 0], d["v"][x, y, 1], d["p"][x, y]] for x, y in probes], np.float64)


def _rows(h):
    return np.stack([h["u"], h["w"], h["p"]], axis=2)          # (n, P, 3)


def _close(sim):
    sim._solver._bc.device.close()


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


PROBE_CASES = ["traj_bc5_cip_vc5.npz", "traj_bc1_upwind_jacobi4_vc0.npz", "traj_dye_bc2_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"]


@pytest.mark.parametrize("fname", PROBE_CASES)
def test_probe_values_equal_eager_downloads(fname, hip_lib):
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    probes = _probes(g["bc_mask"])
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        a.record_history(probes)
        n = 40
        a.run(n, graph=True)
        assert a._graphs, "the run replayed no graph"
        exp = []
        for _ in range(n):
            b.step()
            exp.append(_at(b, probes))
        h = a.history()
        assert h["step"].tolist() == list(range(1, n + 1))
        assert np.array_equal(_rows(h), np.array(exp)), "recorded probe values differ from the downloads"
    finally:
        _close(a)
        _close(b)


def _force_bound(p, faces, dx):
    return len(faces) * 2.0 ** -52 * float(np.sum(np.abs(p[faces[:, 0], faces[:, 1]].astype(np.float64) * dx)))


@pytest.mark.parametrize("bc,res", [(1, 64), (3, 64), (5, 64), (3, 400), (5, 256)])
def test_forces_match_flow_stats_and_numpy(bc, res, hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    from fs.history import SIGNS, body_faces
    fs.runtime.init(gpu=0, dtype="f32")
    sim = fs.FluidSimulator.create(bc, res, 0.05 / res, 1.0 / res, 1e6, 5.0, "cip")
    try:
        box = default_body_box(bc, res)
        sim.record_history([], box)
        sim.run(30, graph=True)
        h = sim.history()
        p = sim.field_to_numpy()["p"]
        faces = body_faces(sim._solver._bc.mask, box)
        terms = p[faces[:, 0], faces[:, 1]].astype(np.float64) * (1.0 / res)
        np_f = [sum(SIGNS[d] * t for t, d in zip(terms, faces[:, 2]) if d // 2 == c) for c in (0, 1)]
        st = sim.flow_stats(box)
        tol = _force_bound(p, faces, 1.0 / res)
        got = (h["force_x"][-1], h["force_y"][-1])
        assert abs(got[0]) > 0.0
        for c, k in enumerate(("force_x", "force_y")):
            assert abs(got[c] - st[k]) <= tol, (k, got[c], st[k])
            assert abs(got[c] - np_f[c]) <= tol, (k, got[c], np_f[c])
    finally:
        _close(sim)
    if len(faces) > 512:            # (the split form of the face sum, csrc/fs_history.h HIST_SPLIT): the same bits from eager steps
        twin = fs.FluidSimulator.create(bc, res, 0.05 / res, 1.0 / res, 1e6, 5.0, "cip")
        try:
            twin.record_history([], box)
            twin.run(30, graph=False)
            h2 = twin.history()
        finally:
            _close(twin)
        assert np.array_equal(h["force_x"], h2["force_x"]) and np.array_equal(h["force_y"], h2["force_y"])


def test_trajectory_and_records_unchanged(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    probes = _probes(g["bc_mask"])
    box = default_body_box(5, cfg["res"])
    out = {}
    for graph in (False, True):
        for rec in (False, True):
            sim = make_product(g, cfg)
            try:
                if rec:
                    sim.record_history(probes, box)
                sim.run(37, graph=graph)
                out[graph, rec] = (sim.field_to_numpy(), sim.history() if rec else None)
            finally:
                _close(sim)
    base = out[False, False][0]
    for key, (f, _) in out.items():
        for k in base:
            assert np.array_equal(f[k], base[k]), f"{k} changed with graph, recorder = {key}"
    he, hg = out[False, True][1], out[True, True][1]
    for k in ("u", "w", "p", "force_x", "force_y"):
        assert np.array_equal(he[k], hg[k]), f"{k}: eager and graph records differ"
    # repeated runs: two fresh simulators recording the same 37 steps give the same bits
    sim = make_product(g, cfg)
    try:
        sim.record_history(probes, box)
        sim.run(20, graph=True)
        sim.run(17, graph=True)
        h2 = sim.history()
    finally:
        _close(sim)
    for k in ("u", "w", "p", "force_x", "force_y"):
        assert np.array_equal(h2[k], hg[k]), k


@pytest.mark.parametrize("every,expect", [(1, list(range(1, 101))), (3, list(range(3, 100, 3)))])
def test_tiny_ring_across_graph_replays(every, expect, hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    probes = _probes(g["bc_mask"])
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        a.record_history(probes, capacity=7, every=every)
        b.record_history(probes, every=every)
        a.run(100, graph=True)
        b.run(100, graph=True)
        ha, hb = a.history(), b.history()
        assert ha["step"].tolist() == expect
        assert np.array_equal(_rows(ha), _rows(hb))
        assert np.array_equal(_rows(ha)[-1], _at(a, probes)) if every == 1 else True
    finally:
        _close(a)
        _close(b)


def test_deferred_limit_reaches_probes(hip_lib):
    import fs
    from fs.solver import VELOCITY_LIMIT
    g, cfg = _load("traj_bc1_upwind_vc0.npz")          # (MacSolver: its end-of-step limit_field is always deferred)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        probes = _probes(mask, n=8)
        v = np.zeros(mask.shape + (2,), np.float32)
        v[mask == 0] = (3.0 * VELOCITY_LIMIT, -2.0 * VELOCITY_LIMIT)
        sim._solver.v.current.from_numpy(v)
        sim.record_history(probes)
        sim.step()
        assert sim._solver.v.current.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        h = sim.history()
        exp = _at(sim, probes)                       # the download launches the owed pass first
        assert np.array_equal(_rows(h)[-1], exp)
        assert np.all(np.hypot(exp[:, 0], exp[:, 1]) <= VELOCITY_LIMIT * (1 + 1e-6))
    finally:
        _close(sim)


def test_refusals(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._solver._bc.device
    try:
        X, Y = g["bc_mask"].shape
        with pytest.raises(_lib.FsError):                      # a face (and a probe) outside the owned rows
            dev._p_history_create(np.zeros((0, 2), np.int32), np.array([[1, Y, 0]], np.int32), 4, 1)
        with pytest.raises(_lib.FsError):
            dev._p_history_create(np.array([[X, 1]], np.int32), np.zeros((0, 3), np.int32), 4, 1)
        probes = _probes(g["bc_mask"])
        sim.record_history(probes)
        sim.step()
        h = sim._recorder.hist
        v, p = sim._solver.get_fields()[:2]
        with pytest.raises(_lib.FsError):                      # wrong channel counts
            _lib.call("fs_history_record", dev._ctx, h._h, 0.1, 0.0, p._h, v._h)
        n, launches, dropped = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = dev._lib.fs_history_read(dev._ctx, h._h, None, 0, ctypes.byref(n), ctypes.byref(launches), ctypes.byref(dropped))
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == -3, "fs_history_read during a capture must be refused with FS_ERR_STATE"
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.record_history(probes))
        assert sim.history()["step"].tolist() == [1]
    finally:
        _close(sim)


# ---- slab contexts on one GPU (the thread harness of test_gpu_slab_threads.py), tape replays -------------------------------------
def _slab_history(g, cfg, world, halo, probes, box, steps):
    import fs
    from test_gpu_slab_threads import _make_device_cls
    shared = {"barrier": threading.Barrier(world), "box": [None] * world, "radii": [None] * world, "sum": [None] * world}
    Base = _make_device_cls(world, shared)

    class Dev(Base):
        def _p_allreduce_array(self, a):
            shared["sum"][self.rank] = np.asarray(a, np.float64)
            shared["barrier"].wait()
            tot = shared["sum"][0].copy()
            for r in range(1, world):
                tot = tot + shared["sum"][r]
            shared["barrier"].wait()
            return tot

    results, errors = [None] * world, []

    def work(rank):
        try:
            dt, dx, re = cfg["dt"], cfg["dx"], cfg["re"]
            X, Y = g["bc_mask"].shape
            dev = Dev(X, Y, np.float64 if cfg["fp64"] else np.float32, rank, halo)
            bc = fs.BoundaryCondition(g["bc_const"], g["bc_mask"], device=dev)
            vc = fs.VorticityConfinement(bc, dt, dx, cfg["vor_eps"]) if cfg["vor_eps"] is not None else None
            u = cfg["updater"]
            pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, u[1], u[2]) if u[0] == "rbsor" else fs.JacobiPressureUpdater(bc, dt, dx, u[1])
            solver = fs.CipMacSolver(bc, pu, dt, dx, re, vc)
            sim = fs.FluidSimulator(solver)
            sim.record_history(probes, box, capacity=40)
            sim.run(steps)
            results[rank] = (sim.history(), len(sim._tapes))
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


@pytest.mark.parametrize("world,halo", [(2, 4), (3, 4), (4, 4)])
def test_slab_contexts_match_single_context(world, halo, hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    from fs.history import body_faces
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    probes = _probes(g["bc_mask"], n=9, seed=world)
    box = default_body_box(5, cfg["res"])
    steps = 70
    one = make_product(g, cfg)
    try:
        one.record_history(probes, box)
        one.run(steps, graph=False)
        exp = one.history()
        p_end = one.field_to_numpy()["p"]
    finally:
        _close(one)
    res = _slab_history(g, cfg, world, halo, probes, box, steps)
    assert all(n > 0 for _, n in res), "no tape was replayed"
    for h, _ in res:
        assert h["step"].tolist() == list(range(1, steps + 1))
        assert np.array_equal(_rows(h), _rows(exp)), "slab probes differ from the single context"
    faces = body_faces(g["bc_mask"], box)
    tol = 4 * _force_bound(p_end, faces, cfg["dx"])
    for k in ("force_x", "force_y"):
        assert abs(res[0][0][k][-1] - exp[k][-1]) <= tol, k          # (the last record: the state whose p bounds the terms)
