"""Body surface loads on the GPU (csrc/fs_loads.h k_loads_one / k_loads_faces / k_loads_record, include/fs_hip.h fs_loads_*,
FluidSimulator.track_body / body_loads / body_surface / body_snapshot): per-face sums bit for bit against the NumPy restatement
(tests/loads_ref.py) fed with the downloads of an eagerly stepped twin, records within the derived rounding bound and identical between
runs, unchanged trajectories, a tiny ring across graph replays, the deferred limit pass, snapshots, refusals, slab contexts on one GPU."""
import ctypes
import os
import threading

import numpy as np
import pytest
from conftest import GOLDEN
from helpers import make_product, traj_config
from loads_ref import record_bound, sample_ref, samples

pytestmark = pytest.mark.gpu

SERIES = ("pressure_x", "pressure_y", "viscous_x", "viscous_y", "moment_pressure", "moment_viscous")
# (bc, res, dtype): 24, 432, 640 faces (f32), 432 (f64), 2160 and 4096 = 16 x 256 faces - both launch forms (csrc/fs_loads.h LOADS_SPLIT = 512),
# a last workgroup that is full and ones that are not
SUM_CASES = [(1, 64, "f32"), (5, 64, "f32"), (3, 64, "f32"), (5, 64, "f64"), (5, 256, "f32"), (3, 400, "f32")]
REC_CASES = SUM_CASES[:3] + [(5, 128, "f32")] + SUM_CASES[4:]          # the six face counts: 24, 432, 640, 1080, 2160, 4096
FACES = {(1, 64): 24, (5, 64): 432, (3, 64): 640, (5, 128): 1080, (5, 256): 2160, (3, 400): 4096}
VARIANTS = [(1, 0), (3, 4)]          # (every, start_step)
STEPS = 40


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


def _create(bc, res, dtype):
    import fs
    fs.runtime.init(gpu=0, dtype=dtype)
    re = 100.0 if res <= 128 else 1000.0           # friction visible, dt / (re dx^2) <= 0.05
    return fs.FluidSimulator.create(bc, res, 0.05 / res, 1.0 / res, re, 5.0, "cip"), re


_REF, _RUN = {}, {}


def _reference(bc, res, dtype):
    """The restatement fed with the downloads of an eagerly stepped twin, for every sampling variant: computed once per case."""
    key = (bc, res, dtype)
    if key in _REF:
        return _REF[key]
    from fs.boundary_condition import default_body_box
    from fs.history import body_faces
    from fs.loads import body_centroid
    twin, re = _create(bc, res, dtype)
    try:
        mask = twin._solver._bc.mask
        box = default_body_box(bc, res)
        faces, centre = body_faces(mask, box), body_centroid(mask, box)
        assert len(faces) == FACES[bc, res]
        out = {v: {"sums": np.zeros((4, len(faces))), "rec": [], "scale": [], "step": []} for v in VARIANTS}
        for n in range(STEPS):
            twin.step()
            d = twin.field_to_numpy()
            for (every, start), o in out.items():
                if samples(n, start, every):
                    rec, scale = sample_ref(o["sums"], d["v"], d["p"], faces, centre, 1.0 / res, 1.0 / re)
                    o["rec"].append(rec), o["scale"].append(scale), o["step"].append(n + 1)
        st = twin.flow_stats(box)
        assert st["nonfinite"] == 0
    finally:
        _close(twin)
    _REF[key] = {"variants": out, "faces": faces, "centre": centre, "box": box, "stats": st}
    return _REF[key]


def _tracked(bc, res, dtype, every, start):
    """A tracked simulator after run(STEPS, graph=True): its series, surface and flow_stats; computed once per case and variant."""
    key = (bc, res, dtype, every, start)
    if key in _RUN:
        return _RUN[key]
    from fs.boundary_condition import default_body_box
    sim, _ = _create(bc, res, dtype)
    try:
        box = default_body_box(bc, res)
        sim.track_body(box, every=every, start_step=start)
        sim.run(STEPS, graph=True)
        assert sim._graphs, "the run replayed no graph"
        st = sim.flow_stats(box)
        assert st["nonfinite"] == 0
        _RUN[key] = {"loads": sim.body_loads(), "surface": sim.body_surface(), "stats": st}
    finally:
        _close(sim)
    return _RUN[key]


# ---- 1. per-face sums, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every,start", VARIANTS)
@pytest.mark.parametrize("bc,res,dtype", SUM_CASES)
def test_per_face_sums_equal_the_restatement(bc, res, dtype, every, start, hip_lib):
    ref = _reference(bc, res, dtype)
    got = _tracked(bc, res, dtype, every, start)
    exp = ref["variants"][every, start]
    s = got["surface"]
    assert np.array_equal(s["faces"], ref["faces"])
    assert s["samples"] == len(exp["step"]) and got["loads"]["step"].tolist() == exp["step"]
    assert np.abs(exp["sums"][2]).max() > 0.0, "no wall shear in the reference: the case shows nothing"
    for k, name in enumerate(("S_p", "S_pp", "S_t", "S_tt")):
        assert np.array_equal(s["sums"][k], exp["sums"][k]), f"{name} differs from the restatement"


# ---- 2. records ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc,res,dtype", REC_CASES)
def test_records_within_the_rounding_bound_and_repeatable(bc, res, dtype, hip_lib):
    ref = _reference(bc, res, dtype)
    nf = len(ref["faces"])
    for every, start in VARIANTS:
        got, exp = _tracked(bc, res, dtype, every, start)["loads"], ref["variants"][every, start]
        rec, tol = np.array(exp["rec"]), record_bound(nf, np.array(exp["scale"]))
        assert got["step"].tolist() == exp["step"]
        for c, k in enumerate(SERIES):
            err = np.abs(got[k] - rec[:, c])
            assert np.all(err <= tol[:, c]), (k, every, float(err.max()), float(tol[:, c].min()))
        assert np.abs(got["viscous_x"]).max() > 0.0 and np.abs(got["pressure_x"]).max() > 0.0
    # the last step's pressure force against flow_stats (the same faces and terms, another summation order)
    run = _tracked(bc, res, dtype, 1, 0)
    tol = record_bound(nf, ref["variants"][1, 0]["scale"][-1])
    for c, (k, s) in enumerate((("pressure_x", "force_x"), ("pressure_y", "force_y"))):
        assert abs(run["loads"][k][-1] - run["stats"][s]) <= tol[c], (k, run["loads"][k][-1], run["stats"][s], tol[c])
        assert run["stats"][s] == ref["stats"][s]
    # a second fresh simulator: the same bits in every record
    from fs.boundary_condition import default_body_box
    sim, _ = _create(bc, res, dtype)
    try:
        sim.track_body(default_body_box(bc, res))
        sim.run(STEPS, graph=True)
        again = sim.body_loads()
    finally:
        _close(sim)
    for k in SERIES:
        assert np.array_equal(again[k], run["loads"][k]), f"{k}: two runs differ"


# ---- 3. the trajectory and the other riders are unchanged ---------------------------------------------------------------------------------
def test_trajectory_history_averages_and_tracers_unchanged(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    box = default_body_box(5, cfg["res"])
    fluid = np.argwhere(np.asarray(g["bc_mask"]) == 0)
    probes = [tuple(int(c) for c in fluid[k]) for k in np.linspace(0, len(fluid) - 1, 5).astype(int)]
    seeds = fluid[np.linspace(0, len(fluid) - 1, 50).astype(int)] + 0.5
    out = {}
    for riders, tracker in ((False, False), (True, False), (True, True)):
        sim = make_product(g, cfg)
        try:
            if riders:
                sim.record_history(probes, box)
                sim.start_averaging()
                sim.seed_tracers(seeds)
            if tracker:
                sim.track_body(box)
            sim.run(37, graph=True)
            assert sim._graphs
            res = {"fields": sim.field_to_numpy()}
            if riders:
                res.update(history=sim.history(), averages=sim.averages(), tracers=sim.tracers())
            if tracker:
                assert sim.body_loads()["step"].tolist() == list(range(1, 38))
            out[riders, tracker] = res
        finally:
            _close(sim)
    base = out[False, False]["fields"]
    for key, res in out.items():
        for k in base:
            assert np.array_equal(res["fields"][k], base[k]), f"{k} changed with riders, tracker = {key}"
    a, b = out[True, False], out[True, True]
    for part in ("history", "averages", "tracers"):
        for k, x in a[part].items():
            assert np.array_equal(np.asarray(x), np.asarray(b[part][k])), f"{part}[{k}] changed with the tracker"


# ---- 4. a ring of 3 records across graph replays -----------------------------------------------------------------------------------------
# every = 8: the ring holds 31 steps, enough for run() to capture and replay graphs between two drains; every = 1: chunks of 3 eager steps
@pytest.mark.parametrize("every", [8, 1])
def test_capacity_3_ring_across_graph_replays(every, hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    box = default_body_box(5, cfg["res"])
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        a.track_body(box, capacity=3, every=every)
        b.track_body(box, every=every)
        a.run(100, graph=True)
        b.run(100, graph=True)
        assert b._graphs and (a._graphs or every == 1), "the run replayed no graph"
        ha, hb = a.body_loads(), b.body_loads()
        assert ha["step"].tolist() == list(range(every, 101, every))
        for k in SERIES:
            assert np.array_equal(ha[k], hb[k]), k
        assert np.array_equal(a.body_surface()["sums"], b.body_surface()["sums"]) and a.body_surface()["samples"] == 100 // every
    finally:
        _close(a)
        _close(b)


# ---- 5. a deferred limit_field reaches tau -----------------------------------------------------------------------------------------------
def test_deferred_limit_reaches_tau(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    from fs.solver import VELOCITY_LIMIT
    g, cfg = _load("traj_bc1_upwind_vc0.npz")          # (MacSolver: its end-of-step limit_field is always deferred)
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[mask == 0] = (3.0 * VELOCITY_LIMIT, -2.0 * VELOCITY_LIMIT)
        sim._solver.v.current.from_numpy(v)
        box = default_body_box(cfg["bc"], cfg["res"])
        sim.track_body(box)
        sim.step()
        assert sim._solver.v.current.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        s, loads = sim.body_surface(), sim.body_loads()
        d = sim.field_to_numpy()                         # the download launches the owed pass first
        sums = np.zeros((4, len(s["faces"])))
        rec, scale = sample_ref(sums, d["v"], d["p"], s["faces"], sim._tracker.centre, cfg["dx"], 1.0 / cfg["re"])
        assert np.array_equal(s["sums"], sums)
        near = d["v"][s["faces"][:, 0], s["faces"][:, 1]].astype(np.float64)
        assert np.all(np.hypot(near[:, 0], near[:, 1]) <= VELOCITY_LIMIT * (1 + 1e-6)) and np.abs(sums[2]).max() > 0.0
        tol = record_bound(len(s["faces"]), scale)
        for c, k in enumerate(SERIES):
            assert abs(loads[k][-1] - rec[c]) <= tol[c], k
    finally:
        _close(sim)


# ---- 6. body_snapshot ----------------------------------------------------------------------------------------------------------------
def test_snapshot_equals_a_one_sample_tracker_and_changes_nothing(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc1_upwind_vc0.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    box = default_body_box(cfg["bc"], cfg["res"])
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        a.track_body(box, start_step=19, every=1)
        a.run(20, graph=True)
        b.run(20, graph=True)
        graphs = set(a._graphs)
        pend = a._solver.v.current.pending_limit
        assert pend is not None, "no pending limit: the test does not cover it"
        snap = a.body_snapshot(box)
        assert a._solver.v.current.pending_limit == pend and set(a._graphs) == graphs and a._tracker is not None
        loads, surf = a.body_loads(), a.body_surface()
        assert loads["step"].tolist() == [20] and surf["samples"] == 1
        for k in SERIES + ("force_x", "force_y", "moment"):
            assert snap[k] == loads[k][0], k
        assert np.array_equal(snap["p"], surf["sums"][0]) and np.array_equal(snap["tau"], surf["sums"][2])
        assert np.array_equal(snap["theta"], surf["theta"]) and np.array_equal(snap["faces"], surf["faces"])
        snap_b = b.body_snapshot(box)                   # without any tracker: the same numbers
        for k in SERIES:
            assert snap_b[k] == snap[k], k
        a.run(17, graph=True)
        b.run(17, graph=True)
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        for k in fa:
            assert np.array_equal(fa[k], fb[k]), k
        assert a.body_loads()["step"].tolist() == list(range(20, 38))
    finally:
        _close(a)
        _close(b)


def test_snapshot_on_manufactured_fields(hip_lib):
    import fs
    from fs.loads import RECORD
    from loads_ref import DX, RE, manufactured
    g, cfg = _load("traj_bc1_upwind_vc0.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    gd = {k: g[k] for k in g.files}
    mask = np.array(g["bc_mask"])
    inner = mask[1:-1, 1:-1]
    inner[inner == 1] = 0                               # the cylinder out, one 6 x 5 rectangle in
    box = (20, 10, 26, 15)
    mask[box[0]:box[2], box[1]:box[3]] = 1
    gd["bc_mask"] = mask
    sim = make_product(gd, dict(cfg, dx=DX, re=RE))
    try:
        faces, centre, cases = manufactured(mask, box)
        assert len(faces) == 22
        for name, v, p, check in cases:
            sim._solver.v.current.from_numpy(v)
            sim._solver.p.current.from_numpy(p)
            snap = sim.body_snapshot(box)
            sums = np.zeros((4, len(faces)))
            rec, scale = sample_ref(sums, v, p, faces, centre, DX, 1.0 / RE)
            b = record_bound(len(faces), scale)
            check({k: snap[k] for k in RECORD}, dict(zip(RECORD, b)))
            assert np.array_equal(snap["p"], sums[0]) and np.array_equal(snap["tau"], sums[2]), name
            for c, k in enumerate(RECORD):
                assert abs(snap[k] - rec[c]) <= b[c], (name, k)
    finally:
        _close(sim)


# ---- 7. reset, stop, refusals ------------------------------------------------------------------------------------------------------------
def test_reset_stop_and_refusals(hip_lib):
    import fs
    from fs import _lib
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._solver._bc.device
    try:
        X, Y = g["bc_mask"].shape
        box = default_body_box(5, cfg["res"])
        with pytest.raises(RuntimeError):
            sim.body_loads()
        sim.track_body(box, every=2)
        with pytest.raises(RuntimeError):
            sim.track_body(box)                                 # a second tracker
        sim.run(20, graph=True)
        assert sim.body_surface()["samples"] == 10
        sim.reset_body_surface()
        s = sim.body_surface()
        assert s["samples"] == 0 and not s["sums"].any()
        sim.run(5, graph=True)                                  # steps 21 - 25: the phase of `every` runs on, the series too
        assert sim.body_surface()["samples"] == 2 and sim.body_loads()["step"].tolist() == list(range(2, 25, 2))
        # C-ABI: every host entry is refused during a capture; a capture of the facade's entries raises
        lo = sim._tracker.loads
        n, launches, smp, dropped = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        buf = (ctypes.c_double * (4 * lo.nfaces))()
        face = (ctypes.c_int * 3)(*[int(c) for c in sim._tracker.faces[0]])
        centre = (ctypes.c_double * 2)(1.0, 1.0)
        h = ctypes.c_void_p()
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_loads_read(dev._ctx, lo._h, None, 0, ctypes.byref(n), ctypes.byref(launches), ctypes.byref(smp), ctypes.byref(dropped)),
                  dev._lib.fs_loads_sums_read(dev._ctx, lo._h, buf),
                  dev._lib.fs_loads_sums_write(dev._ctx, lo._h, buf, 0, 0),
                  dev._lib.fs_loads_reset(dev._ctx, lo._h),
                  dev._lib.fs_loads_create(dev._ctx, 1, face, centre, 4, 1, 0, ctypes.byref(h))]
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3] * 5, f"host entries during a capture must be refused with FS_ERR_STATE, got {st}"
        for entry in (lambda: sim.track_body(box), lambda: sim.body_snapshot(box), sim.body_loads, sim.body_surface, sim.reset_body_surface,
                      sim.stop_body):
            with pytest.raises(RuntimeError):
                dev.capture(entry)
        # bad arguments at the C-ABI: FS_ERR_ARG
        bad = [dict(nf=0), dict(cap=0), dict(every=0), dict(start=-1), dict(c=(float("nan"), 1.0)), dict(c=(1.0, float("inf"))),
               dict(f=(1, Y, 0)), dict(f=(X, 1, 0)), dict(f=(1, 1, 4))]
        for kw in bad:
            f = (ctypes.c_int * 3)(*kw.get("f", tuple(face)))
            c = (ctypes.c_double * 2)(*kw.get("c", (1.0, 1.0)))
            got = dev._lib.fs_loads_create(dev._ctx, kw.get("nf", 1), f, c, kw.get("cap", 4), kw.get("every", 1), kw.get("start", 0), ctypes.byref(h))
            assert got == -1, (kw, got)
        with pytest.raises(_lib.FsError):                      # a face outside the owned rows, through the runtime's primitive
            dev._p_loads_create(np.array([[1, Y, 0]], np.int32), (1.0, 1.0), 4, 1, 0)
        v, p = sim._solver.get_fields()[:2]
        with pytest.raises(_lib.FsError):                      # wrong channel counts
            _lib.call("fs_loads_record", dev._ctx, lo._h, 0.1, 0.01, 0.0, p._h, v._h)
        # stop: the graphs that hold the launches go, the results stay, and the run goes on
        tok = sim._tracker.token
        assert any(tok in k for k in sim._graphs)
        before = sim.body_loads()
        sim.stop_body()
        assert not any(tok in k for k in sim._graphs) and sim._tracker is None
        sim.run(20, graph=True)
        after = sim.body_loads()
        assert after["step"].tolist() == before["step"].tolist() and np.array_equal(after["force_x"], before["force_x"])
        assert sim.body_surface()["samples"] == 2
        sim.track_body(box)
        sim.run(3, graph=True)
        assert sim.body_loads()["step"].tolist() == [1, 2, 3]
    finally:
        _close(sim)


# ---- 8. slab contexts on one GPU (the thread harness of test_gpu_slab_threads.py), tape replays -------------------------------------------
def _slab_loads(g, cfg, world, halo, box, steps):
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
            sim = fs.FluidSimulator(fs.CipMacSolver(bc, pu, dt, dx, re, vc))
            sim.track_body(box, capacity=40)
            sim.run(steps)
            results[rank] = (sim.body_loads(), sim.body_surface(), len(sim._tapes))
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


def test_two_slab_contexts_match_the_single_context(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    box = default_body_box(5, cfg["res"])
    steps = 70
    one = make_product(g, cfg)
    try:
        one.track_body(box)
        d, sums, scales = None, None, []
        for _ in range(steps):                               # eager, with the restatement's scale of every record
            one.step()
            d = one.field_to_numpy()
            scales.append(sample_ref(np.zeros((4, len(one._tracker.faces))), d["v"], d["p"], one._tracker.faces, one._tracker.centre,
                                     cfg["dx"], 1.0 / cfg["re"])[1])
        exp, surf = one.body_loads(), one.body_surface()
    finally:
        _close(one)
    res = _slab_loads(g, cfg, 2, 2, box, steps)
    assert all(n > 0 for _, _, n in res), "no tape was replayed"
    tol = record_bound(len(surf["faces"]), np.array(scales))
    for loads, s, _ in res:
        assert loads["step"].tolist() == list(range(1, steps + 1)) and s["samples"] == steps
        assert np.array_equal(s["sums"], surf["sums"]), "per-face sums differ from the single context"
        for c, k in enumerate(SERIES):
            assert np.all(np.abs(loads[k] - exp[k]) <= tol[:, c]), k
