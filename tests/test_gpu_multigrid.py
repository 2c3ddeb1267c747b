"""GPU parity of the multigrid pressure updater (fs.pressure_updater.MultigridPressureUpdater, csrc/fs_mg.h) against its NumPy restatement
(tests/multigrid_ref.py): every comparison is bit for bit.

Shapes: res 32 (64 x 32; levels 32 x 16 ... 2 x 1, all of them in the one-workgroup tail by default), res 48 (levels down to 6 x 3: a coarsest
level that is no power of two and has an odd height), res 80 (160 columns: level 1 has 80, the fine kernels' partial wave).  FS_MG_TAIL moves
the boundary between one launch per half sweep and the tail kernel: 0, the default and a value that splits the hierarchy in the middle, each
in a fresh process."""
import functools
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from conftest import REPO, golden

import multigrid_ref as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RE, VC = 1.0e6, 5.0


@functools.lru_cache(maxsize=None)
def scene(num, res):
    if num == 6:      # the image scene, from the arrays the reference builder produced (the package ships no copy of the image)
        g = golden("scenes.npz")
        return g[f"bc6_res{res}_bc_const"], g[f"bc6_res{res}_bc_mask"]
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(num, res)
    return const, mask


@functools.lru_cache(maxsize=None)
def developed(num, res, dtype):
    """(p.current, p.next, v) after 12 oracle steps of the default solver (CIP, vorticity confinement, RB-SOR(1.3, 2)); read-only."""
    const, mask = scene(num, res)
    sim = O.make_simulator(const, mask, None, scheme="cip", dt=0.05 / res, dx=1.0 / res, re=RE, vor_eps=VC, dtype=np.dtype(dtype))
    for _ in range(12):
        sim.update()
    out = (sim.p.current.copy(), sim.p.next.copy(), sim.v.current.copy())
    for a in out:
        a.setflags(write=False)
    return out


def make_ref(num, res, dtype, scheme="cip", vc=VC, **kw):
    const, mask = scene(num, res)
    dt, dx = 0.05 / res, 1.0 / res
    bc = O.OracleBC(const, mask, None, np.dtype(dtype))
    pu = M.MultigridRef(bc, dt, dx, **kw)
    vort = O.OracleVorticity(bc, dt, dx, vc) if vc is not None else None
    if scheme == "cip":
        return O.OracleCipSolver(bc, pu, dt, dx, RE, vort)
    return O.OracleMacSolver(bc, pu, scheme, dt, dx, RE, vort)


def make_sim(num, res, dtype, scheme="cip", vc=VC, **kw):
    import fs
    const, mask = scene(num, res)
    dt, dx = 0.05 / res, 1.0 / res
    fs.runtime.init(gpu=0, dtype="f64" if np.dtype(dtype) == np.float64 else "f32")
    bc = fs.BoundaryCondition(const, mask)
    pu = fs.MultigridPressureUpdater(bc, dt, dx, **kw)
    vort = fs.VorticityConfinement(bc, dt, dx, vc) if vc is not None else None
    if scheme == "cip":
        solver = fs.CipMacSolver(bc, pu, dt, dx, RE, vort)
    else:
        solver = fs.MacSolver(bc, pu, fs.advect_upwind if scheme == "upwind" else fs.advect_kk_scheme, dt, dx, RE, vort)
    return fs.FluidSimulator(solver)


def one_update(num, res, dtype, **kw):
    """updater.update() on the developed state, product and restatement -> ((p.current, p.next) of each, the updater's info)."""
    pc, pn, v = developed(num, res, np.dtype(dtype).name)
    ref = make_ref(num, res, dtype, **kw)
    p = O.Buf2(pc.shape, 1, pc.dtype)
    p.current[...], p.next[...] = pc, pn
    ref.pu.update(p, v.copy())
    sim = make_sim(num, res, dtype, **kw)
    try:
        s = sim._solver
        s.v.current.from_numpy(v)
        s.p.current.from_numpy(pc)
        s.p.next.from_numpy(pn)
        s.pressure_updater.update(s.p, s.v.current)
        return (s.p.current.to_numpy(), s.p.next.to_numpy()), (p.current, p.next), s.pressure_updater.info()
    finally:
        sim._solver._bc.device.close()


def check_update(num, res, dtype, **kw):
    got, exp, info = one_update(num, res, dtype, **kw)
    pc0 = developed(num, res, np.dtype(dtype).name)[0]
    assert not np.array_equal(exp[0], pc0) and np.isfinite(exp[0]).all()
    for name, a, e in zip(("p.current", "p.next"), got, exp):
        assert a.dtype == e.dtype
        assert np.array_equal(a, e), f"bc{num} res {res} {np.dtype(dtype).name} {name}: {int((a != e).sum())} cells differ, max {np.abs(a - e).max():.3e}"
    return info


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("num", [1, 2, 3, 4, 5, 6])
def test_one_update_on_a_developed_state(num, dtype, hip_lib):
    info = check_update(num, 32, dtype)
    assert info["levels"] == 5 and info["tail_level"] == 1 and info["launches"] == 3      # residual, the tail, the correction


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("num,res,levels", [(5, 48, 4), (3, 48, 4), (5, 80, 4), (2, 80, 4)])
def test_odd_coarsest_level_and_partial_waves(num, res, levels, dtype, hip_lib):
    assert check_update(num, res, dtype)["levels"] == levels


def test_two_cycles_equal_two_restatement_cycles(hip_lib):
    check_update(5, 32, "float32", n_cycles=2)
    check_update(2, 48, "float64", n_cycles=2, pre=1, post=3, coarse_sweeps=1, coarsest_sweeps=5)


@pytest.mark.parametrize("num,scheme,vc,dtype", [(2, "cip", VC, "float32"), (5, "cip", None, "float32"), (5, "upwind", None, "float32"),
                                                 (5, "upwind", VC, "float64"), (2, "cip", VC, "float64")])
def test_five_step_trajectories(num, scheme, vc, dtype, hip_lib):
    """From rest, v and p after every step.  (CIP with vorticity confinement: scene 2, where these five steps stay finite although the speed
    limit is already at work in the fourth - with a converged pressure that combination goes unstable within a few steps)"""
    ref = make_ref(num, 32, dtype, scheme=scheme, vc=vc)
    sim = make_sim(num, 32, dtype, scheme=scheme, vc=vc)
    try:
        for step in range(1, 6):
            sim.step()
            ref.update()
            out = sim.field_to_numpy()
            for k, e in ref.fields().items():
                assert np.isfinite(e).all(), f"the restatement's {k} is not finite at step {step}"
                assert np.array_equal(out[k], e), f"bc{num} {scheme} step {step} {k}"
        assert float(np.abs(out["p"]).max()) > 0.0
    finally:
        sim._solver._bc.device.close()


def test_create_accepts_the_multigrid_spec_and_the_residual_falls(hip_lib):
    """FluidSimulator.create(..., pressure_updater=("multigrid", n)) builds the updater; after the same 40 upwind steps from rest the pressure of
    the multigrid run is closer to solving its equation (pressure_residual) than that of the default run (the CPU restatement: 6.0e-2 against
    2.5e-1; during the first 20 steps of the impulsive start it is not - the first cycle on a new defect raises the residual)."""
    import fs
    res, out = 32, {}
    for spec in (None, ("multigrid", 1), ("multigrid", 1, 1.2)):
        fs.runtime.init(gpu=0, dtype="f32")
        sim = fs.FluidSimulator.create(5, res, 0.05 / res, 1.0 / res, RE, None, "upwind", pressure_updater=spec)
        try:
            assert isinstance(sim._solver.pressure_updater, fs.MultigridPressureUpdater) == (spec is not None)
            sim.run(40)
            out[spec] = sim.pressure_residual()
        finally:
            sim._solver._bc.device.close()
    print("rms residual after 40 steps:", out)
    assert 0.0 < out[("multigrid", 1)] < out[None]
    with pytest.raises(ValueError):
        fs.runtime.init(gpu=0, dtype="f32")
        fs.FluidSimulator.create(5, 33, 0.05 / 33, 1.0 / 33, RE, VC, "cip", pressure_updater=("multigrid", 1))


def test_graph_replay_equals_eager_stepping(hip_lib):
    n = 30
    eager = make_sim(5, 32, "float32", vc=None)
    try:
        for _ in range(n):
            eager.step()
        exp = eager.field_to_numpy()
    finally:
        eager._solver._bc.device.close()
    sim = make_sim(5, 32, "float32", vc=None)
    try:
        sim.run(n, graph=True)
        assert sim._graph is not None, "no period of the multigrid step was captured"
        out = sim.field_to_numpy()
    finally:
        sim._solver._bc.device.close()
    for k in exp:
        assert np.isfinite(exp[k]).all() and np.array_equal(out[k], exp[k]), k


def test_history_recorder_leaves_the_trajectory_alone(hip_lib):
    n = 24
    plain = make_sim(2, 32, "float32", vc=None)
    try:
        plain.run(n, graph=True)
        exp = plain.field_to_numpy()
    finally:
        plain._solver._bc.device.close()
    sim = make_sim(2, 32, "float32", vc=None)
    try:
        _, mask = scene(2, 32)
        probe = tuple(int(c) for c in np.argwhere(mask == 0)[len(np.argwhere(mask == 0)) // 2])
        sim.record_history(probes=[probe], every=1)
        sim.run(n, graph=True)
        h = sim.history()
        out = sim.field_to_numpy()
    finally:
        sim._solver._bc.device.close()
    for k in exp:
        assert np.isfinite(exp[k]).all() and np.array_equal(out[k], exp[k]), k
    assert len(h["step"]) == n and h["p"][-1, 0] == float(exp["p"][probe])


def test_refused_on_a_slab_context(hip_lib):
    import fs
    from test_gpu_slab_threads import _make_device_cls
    const, mask = scene(5, 32)
    world, halo = 2, 4
    shared = {"barrier": threading.Barrier(world), "box": [None] * world, "radii": [None] * world}
    Dev = _make_device_cls(world, shared)
    seen, errors = [None] * world, []

    def work(rank):
        try:
            dev = Dev(mask.shape[0], mask.shape[1], np.float32, rank, halo)
            bc = fs.BoundaryCondition(const, mask, device=dev)
            try:
                fs.MultigridPressureUpdater(bc, 0.05 / 32, 1.0 / 32)
            except NotImplementedError as e:
                seen[rank] = str(e)
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
    assert all(s and "single GPU" in s for s in seen), seen


def test_every_tail_size_gives_the_same_bits(hip_lib):
    """FS_MG_TAIL = 0 (one launch per half sweep on every level), the default (res 32: every level in the one-workgroup kernel) and 40 (levels
    1 - 2 as launches, 8 x 4 and below in the kernel), each in a fresh process: the hashes of (p.current, p.next) equal each other and the
    restatement's."""
    pc, pn, v = developed(4, 32, "float32")
    ref = make_ref(4, 32, "float32")
    p = O.Buf2(pc.shape, 1, pc.dtype)
    p.current[...], p.next[...] = pc, pn
    ref.pu.update(p, v.copy())
    want = hashlib.sha256(p.current.tobytes() + p.next.tobytes()).hexdigest()
    seen = {}
    for tail, level in (("0", 0), (None, 1), ("40", 3)):
        env = {k: val for k, val in os.environ.items() if k != "FS_MG_TAIL"}
        if tail is not None:
            env["FS_MG_TAIL"] = tail
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "multigrid_worker.py"), "4", "32"], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        tail_level, digest = r.stdout.split()[-2:]
        assert int(tail_level) == level, (tail, tail_level)
        seen[tail] = digest
    assert len(set(seen.values())) == 1, seen
    assert seen["0"] == want
