"""Inertial tracer particles, wall deposition and accumulated occupancy on the GPU (csrc/fs_tracer.h k_tracer_advance_inertial /
k_tracer_accumulate / k_tracer_sort_*_inertial, include/fs_hip.h fs_tracer_create_inertial ... fs_tracer_accum_*, FluidSimulator.
seed_tracers(tau=...) / tracer_deposits / accumulate_tracers): the particle state, the deposit plane and the accumulator bit for bit against
the NumPy float64 restatement (tests/inertial_ref.py) on synthetic fields and on golden trajectories replayed as hipGraphs against an
eagerly stepped twin; unchanged trajectories and launch counts; sorting changes nothing; checkpoints; the refusals.  Every comparison is
np.array_equal; nothing here looks at a time."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
from conftest import GOLDEN, REPO
from helpers import make_product, traj_config
from inertial_ref import (accumulate_ref, advance_ref, assert_state_equal, band_scene, new_accumulator, new_state, response_ref, run_reference,
                          samples_step)
from tracer_fields_ref import assert_order_contract
from tracers_ref import ALIVE, EXPIRED, LEFT, WALL_HIT, fate_scene
import tracers_ref

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


def _device_state(dev, tr):
    got = dev.tracer_read(tr)
    got["pu"], got["pw"] = dev.tracer_read_vel(tr)
    return got


def _random_scene(rng, X, Y):
    """The masks of tests/test_gpu_tracers.py test_random_fields_and_masks."""
    mask = (rng.random((X, Y)) < 0.12).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.03] = 2
    mask[rng.random((X, Y)) < 0.03] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


def _taus(rng, n):
    """Per-particle response times over six decades, with tau = 0 (alpha = 1) among them."""
    tau = 10.0 ** rng.uniform(-4.0, 2.0, n)
    tau[::7] = 0.0
    return tau


# ---- device level: synthetic fields -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("respawn", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_fate_on_the_device(dtype, respawn, hip_lib):
    """The constructed scene of tests/tracers_ref.py (X = 33: odd) with alpha = 1 for the five constructed seeds plus 300 random seeds with
    random response times and gravity - 305 particles, no multiple of 256."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask, v, seeds, expected = fate_scene(dtype=dt_)
    X, Y = mask.shape
    seeds = np.concatenate([seeds, seed_random(mask, 300, 11)])
    assert X % 2 == 1 and len(seeds) % 256 != 0
    rng = np.random.default_rng(4)
    tau = np.concatenate([np.zeros(5), _taus(rng, 300)])
    alpha = response_ref(tau, 0.05)
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        tr = dev.tracer_create_inertial(seeds, alpha, tau, gravity=(0.0, 0.0), respawn=respawn, max_age=20, deposits=True)
        exp = new_state(seeds, alpha, tau)
        dep = np.zeros((X, Y), np.int32)
        seen = set()
        for _ in range(50):
            dev.tracer_advance(tr, 0.5, vf)
            seen |= set(advance_ref(exp, v, mask, 0.5, (0.0, 0.0), respawn, 20, deposits=dep).tolist())
        assert seen == {ALIVE, LEFT, WALL_HIT, EXPIRED}, "a fate code did not occur"
        got = _device_state(dev, tr)
        assert got["pu"].dtype == np.float64 and got["steps"] == 50
        assert_state_equal(got, exp)
        got_dep = dev.tracer_deposits(tr)
        assert got_dep.dtype == np.int32 and got_dep.shape == (X, Y)
        assert np.array_equal(got_dep, dep) and dep.sum() > 0 and np.all(mask[np.nonzero(dep)] == 1)
        if respawn:
            assert not got["status"].any() and np.all(got["respawns"][:5] > 0)
        else:
            assert np.array_equal(got["status"][:5], expected) and not got["respawns"].any()
        dev.tracer_free(tr)
    finally:
        dev.close()


@pytest.mark.parametrize("X,Y,dtype,n,respawn,max_age,gravity", [(101, 51, "f32", 1000, True, 0, (0.0, -3.0)), (67, 33, "f64", 257, False, 9, (1.5, 0.5)),
                                                                 (250, 125, "f32", 5000, False, 0, (0.0, 0.0)), (1026, 37, "f64", 255, True, 7, (0.0, -40.0)),
                                                                 (4, 4, "f32", 3, True, 0, (0.25, 0.0))])
def test_random_fields_and_masks(X, Y, dtype, n, respawn, max_age, gravity, hip_lib):
    """Random velocities (changed between launches) on random masks, per-particle response times, gravity: wall hits and their deposits,
    outflow cells, exits through every edge and expiry as they come; the smallest grid the interpolation admits."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    rng = np.random.default_rng(X * 1000 + Y)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = _random_scene(rng, X, Y) if X > 8 else np.zeros((X, Y), np.uint8)
    seeds = seed_random(mask, n, 5)
    tau = _taus(rng, n)
    alpha = response_ref(tau, 0.02)
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        tr = dev.tracer_create_inertial(seeds, alpha, tau, gravity=gravity, respawn=respawn, max_age=max_age, deposits=True)
        exp = new_state(seeds, alpha, tau)
        dep = np.zeros((X, Y), np.int32)
        fates = set()
        for k in range(50):
            if k % 10 == 0:
                v = (rng.standard_normal((X, Y, 2)) * 1.5).astype(dt_)
                vf.from_numpy(v)
            dev.tracer_advance(tr, 0.4, vf)
            fates |= set(advance_ref(exp, v, mask, 0.4, gravity, respawn, max_age, deposits=dep).tolist())
        assert_state_equal(_device_state(dev, tr), exp)
        assert np.array_equal(dev.tracer_deposits(tr), dep)
        if X > 8:
            assert {LEFT, WALL_HIT} <= fates and (max_age == 0 or EXPIRED in fates) and dep.sum() > 0
    finally:
        dev.close()


def test_inertia_decides_the_fate_on_the_device(hip_lib):
    """tests/test_inertial_cpu.py test_inertia_decides_the_fate: light particles leave through the top edge, heavy ones deposit."""
    from fs.runtime import Device
    mask, v, seeds = band_scene()
    X, Y = mask.shape
    dev = Device(X, Y, "f32")
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), np.float32))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        light = dev.tracer_create_inertial(seeds, np.ones(3), np.zeros(3), respawn=False, deposits=True)
        heavy = dev.tracer_create_inertial(seeds, np.full(3, 0.05), np.ones(3), respawn=False, deposits=True)
        for _ in range(80):
            dev.tracer_advance(light, 0.5, vf)
            dev.tracer_advance(heavy, 0.5, vf)
        assert np.all(dev.tracer_read(light)["status"] == LEFT) and not dev.tracer_deposits(light).any()
        assert np.all(dev.tracer_read(heavy)["status"] == WALL_HIT)
        exp = np.zeros((X, Y), np.int32)
        exp[20, 7] = exp[20, 8] = exp[20, 9] = 1
        assert np.array_equal(dev.tracer_deposits(heavy), exp)
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_deferred_limit_reaches_the_corners(dtype, hip_lib):
    """Speeds above the limit in the buffer while a deferred limit_field is owed: the particles see the limited values, the pass stays owed."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    X, Y = 130, 65
    rng = np.random.default_rng(17)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = np.zeros((X, Y), np.uint8)
    mask[0, :] = mask[:, 0] = mask[:, -1] = 1
    mask[-1, :] = 3
    seeds = seed_random(mask, 700, 2)
    tau = _taus(rng, 700)
    alpha = response_ref(tau, 0.01)
    v = (rng.standard_normal((X, Y, 2)) * 9.0).astype(dt_)
    assert (np.hypot(v[..., 0], v[..., 1]) > 10.0).mean() > 0.2
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        dev.limit_field(10.0, vf, defer=True)
        assert vf.pending_limit == 10.0, "the limit pass was not deferred: the test does not cover it"
        tr = dev.tracer_create_inertial(seeds, alpha, tau, gravity=(0.0, -1.0), respawn=True)
        exp, unlimited = new_state(seeds, alpha, tau), new_state(seeds, alpha, tau)
        for _ in range(50):
            dev.tracer_advance(tr, 0.05, vf)
            advance_ref(exp, v, mask, 0.05, (0.0, -1.0), limit=10.0)
            advance_ref(unlimited, v, mask, 0.05, (0.0, -1.0))
        assert vf.pending_limit == 10.0                       # (advancing launches nothing else)
        got = _device_state(dev, tr)
        assert_state_equal(got, exp)
        assert not np.array_equal(got["x"], unlimited["x"]), "the limit made no difference: the test does not cover it"
        with pytest.raises(ValueError):
            dev.tracer_deposits(tr)                           # no plane without the flag
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


def _sim_taus(sim, n):
    """Response times from 0 to 300 steps, cycling over the particles."""
    return np.resize(np.array([0.0, 0.5, 3.0, 30.0, 300.0]) * sim._solver.dt, n)


@pytest.mark.parametrize("respawn", [True, False])
@pytest.mark.parametrize("fname", CASES)
def test_state_bit_for_bit_and_trajectory_unchanged(fname, respawn, hip_lib):
    """run(graph=True) with an inertial set, deposits and an accumulation against an eagerly stepped twin without any of them plus the
    restatement: particles, deposits and accumulator equal, and so do the fields."""
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        X, Y = mask.shape
        seeds = _seeds(mask)
        tau = _sim_taus(a, len(seeds))
        dt, dx = a._solver.dt, a._solver.dx
        gravity = (0.0, -0.5 * dx / dt / (50 * dt))      # (half a cell per step after 50 steps of free fall)
        max_age = 0 if respawn else 30
        a.seed_tracers(seeds, respawn=respawn, max_age=max_age, tau=tau, gravity=gravity, deposits=True)
        a.accumulate_tracers(every=3, start_step=4)
        n = 43                      # (odd: no multiple of a graph period)
        a.run(n, graph=True)
        assert a._graphs, "the run replayed no graph"
        exp = new_state(seeds, response_ref(tau, dt), tau)
        dep = np.zeros((X, Y), np.int32)
        acc = new_accumulator(X, Y, 3, 4)
        run_reference(b, n, exp, gravity, respawn, max_age, deposits=dep, acc=acc)
        got = a.tracers()
        assert set(got) == {"x", "y", "age", "status", "respawns", "seeds", "steps", "u", "w", "tau"} and got["steps"] == 43
        assert_state_equal(got, exp)
        assert np.array_equal(got["tau"], tau)
        moved = np.hypot(got["x"] - seeds[:, 0], got["y"] - seeds[:, 1])
        assert moved.max() > 1.0, "no particle moved by more than a cell"
        if not respawn:
            assert EXPIRED in got["status"]
        assert np.array_equal(a.tracer_deposits(), dep)
        ga = a.tracer_accumulation()
        assert set(ga) == {"occupancy", "age_sum", "samples", "steps"}
        assert ga["occupancy"].dtype == np.int64 and ga["occupancy"].shape == (X, Y) and ga["steps"] == 43 and ga["samples"] == acc["samples"] == 13
        assert np.array_equal(ga["occupancy"], acc["occupancy"]) and np.array_equal(ga["age_sum"], acc["age_sum"]) and ga["occupancy"].sum() > 0
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        assert set(fa) == set(fb) and ("dye" in fa) == cfg["dye"]
        for k in fa:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{k}: the particles changed the trajectory"
    finally:
        _close(a)
        _close(b)


def test_launch_count_of_the_flow_kernels_is_unchanged(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    reports, fields = {}, {}
    for traced in (False, True):
        sim = make_product(g, cfg)
        dev = sim._dev
        try:
            if traced:
                seeds = _seeds(g["bc_mask"])
                sim.seed_tracers(seeds, tau=_sim_taus(sim, len(seeds)), gravity=(0.0, -1.0), deposits=True)
                sim.accumulate_tracers(every=2)
            sim.run(30, graph=True)
            sim.step()
            dev.profile(True)
            sim.run(12, graph=False)
            reports[traced] = {k: v[0] for k, v in dev.profile_report().items()}
            if traced:
                assert any("k_tracer_advance_inertial" in k for k in dev.profile_kernels("tracer_advance_inertial"))
                assert any("k_tracer_accumulate" in k for k in dev.profile_kernels("tracer_accumulate"))
            dev.profile(False)
            if traced:
                assert sim.tracers()["steps"] == 43 and sim.tracer_accumulation()["samples"] == 21
                sim.stop_tracers()
                with pytest.raises(RuntimeError):
                    sim.tracer_accumulation()
                assert not [k for k in sim._graphs if any(isinstance(t, tuple) and t and t[0] in ("tracer", "tracer_accum") for t in k)]
            sim.run(25, graph=True)
            fields[traced] = sim.field_to_numpy()
        finally:
            _close(sim)
    mine = {k: v for k, v in reports[True].items() if "tracer" in k}
    assert mine == {"tracer_advance_inertial": 12, "tracer_accumulate": 12}, mine      # one launch each per step; no passive advance
    assert {k: v for k, v in reports[True].items() if "tracer" not in k} == reports[False]
    for k in fields[False]:
        assert np.array_equal(fields[True][k], fields[False][k]), k


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["traj_bc5_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"])
def test_sorting_changes_nothing(fname, hip_lib):
    """sort_every = 16 and an explicit sort_tracers() against a twin that never sorts: tracers(), tracer_deposits() and
    tracer_accumulation() are equal; tracer_order is a permutation with non-decreasing keys after a sort."""
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        X, Y = mask.shape
        seeds = _seeds(mask)
        tau = _sim_taus(a, len(seeds))
        kw = dict(respawn=True, max_age=25, tau=tau, gravity=(0.0, -2.0), deposits=True)
        a.seed_tracers(seeds, sort_every=16, **kw)
        b.seed_tracers(seeds, **kw)
        for sim in (a, b):
            sim.accumulate_tracers(every=3, start_step=2)
        a.run(21, graph=True)
        a.sort_tracers()
        ids = a._dev.tracer_order(a._tracers.set)
        assert np.array_equal(np.sort(ids), np.arange(len(seeds))) and not np.array_equal(ids, np.arange(len(seeds)))
        raw = a._dev.tracer_read(a._tracers.set, raw=True)
        assert_order_contract(raw, X, Y)
        a.run(40, graph=True)
        assert a._tracers.sorts >= 4
        b.run(61, graph=True)
        ta, tb = a.tracers(), b.tracers()
        assert set(ta) == set(tb)
        for k in ta:
            assert np.array_equal(ta[k], tb[k], equal_nan=True), k
        assert np.array_equal(a.tracer_deposits(), b.tracer_deposits())
        ga, gb = a.tracer_accumulation(), b.tracer_accumulation()
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), k
        assert ga["samples"] == 19 and ga["occupancy"].sum() == 19 * len(seeds)
        # the velocities come back in seed order, and a written state lands on the right particles while the slots are permuted
        dev, tr = a._dev, a._tracers.set
        pu, pw = dev.tracer_read_vel(tr)
        dev.tracer_write_vel(tr, pu[::-1].copy(), pw[::-1].copy())
        qu, qw = dev.tracer_read_vel(tr)
        assert np.array_equal(qu, pu[::-1]) and np.array_equal(qw, pw[::-1])
        dev.tracer_write_vel(tr, pu, pw)
        st = dev.tracer_read(tr)
        dev.tracer_write(tr, st)                              # (the slots go back to seed order: pu, pw, alpha, tau follow)
        assert np.array_equal(dev.tracer_order(tr), np.arange(len(seeds)))
        qu, qw = dev.tracer_read_vel(tr)
        assert np.array_equal(qu, pu) and np.array_equal(qw, pw)
        a.run(20, graph=True)
        b.run(20, graph=True)
        ta, tb = a.tracers(), b.tracers()
        for k in ta:
            assert np.array_equal(ta[k], tb[k], equal_nan=True), f"after tracer_write on sorted slots: {k}"
    finally:
        _close(a)
        _close(b)


# ---- accumulator --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every,start", [(1, 5), (3, 4)])
@pytest.mark.parametrize("inertial", [False, True])
def test_accumulator_equals_the_sum_of_the_snapshots(inertial, every, start, hip_lib):
    """Inside graphs, against an eager twin's tracer_fields() at the sampled steps; reset keeps the phase."""
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b = make_product(g, cfg), make_product(g, cfg)
    try:
        seeds = _seeds(g["bc_mask"])
        kw = dict(tau=_sim_taus(a, len(seeds)), gravity=(0.0, -1.0)) if inertial else {}
        for sim in (a, b):
            sim.seed_tracers(seeds, respawn=True, max_age=20, **kw)
        a.run(7, graph=False)       # (the accumulation starts later than the set: its steps count from accumulate_tracers)
        b.run(7, graph=False)
        a.accumulate_tracers(every=every, start_step=start)
        with pytest.raises(RuntimeError):
            a.accumulate_tracers()                            # a second accumulator
        X, Y = g["bc_mask"].shape
        occ, age, ns = np.zeros((X, Y), np.int64), np.zeros((X, Y), np.int64), 0
        occ2, age2, ns2 = occ.copy(), age.copy(), 0
        for k in range(1, 73):
            b.step()
            if samples_step(k, every, start):
                f = b.tracer_fields()
                if k <= 41:
                    occ, age, ns = occ + f["count"], age + f["age_sum"], ns + 1
                else:
                    occ2, age2, ns2 = occ2 + f["count"], age2 + f["age_sum"], ns2 + 1
        a.run(41, graph=True)
        assert a._graphs, "the run replayed no graph"
        got = a.tracer_accumulation()
        assert got["steps"] == 41 and got["samples"] == ns > 0
        assert np.array_equal(got["occupancy"], occ) and np.array_equal(got["age_sum"], age)
        a.reset_tracer_accumulation()
        z = a.tracer_accumulation()
        assert z["samples"] == 0 and not z["occupancy"].any() and not z["age_sum"].any() and z["steps"] == 41
        a.run(31, graph=True)
        got = a.tracer_accumulation()
        assert got["steps"] == 72 and got["samples"] == ns2 > 0
        assert np.array_equal(got["occupancy"], occ2) and np.array_equal(got["age_sum"], age2)
        from fs.tracers import concentration, residence_map
        assert concentration(got["occupancy"], got["samples"]).sum() == pytest.approx(len(seeds))
        assert np.nanmax(residence_map(got["occupancy"], got["age_sum"], a._solver.dt)) <= 20 * a._solver.dt
        a.stop_tracer_accumulation()
        with pytest.raises(RuntimeError):
            a.tracer_accumulation()
        a.run(20, graph=True)                                 # (graphs without the launch again)
        b.run(20, graph=True)
        ta, tb = a.tracers(), b.tracers()
        for k in ta:
            assert np.array_equal(ta[k], tb[k], equal_nan=True), k
    finally:
        _close(a)
        _close(b)


def test_checkpoint_round_trip_continues_bit_for_bit(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b, c = make_product(g, cfg), make_product(g, cfg), None
    try:
        seeds = _seeds(g["bc_mask"])
        tau = _sim_taus(a, len(seeds))
        kw = dict(respawn=True, max_age=35, tau=tau, gravity=(0.0, -1.0), deposits=True)
        a.seed_tracers(seeds, **kw)
        a.accumulate_tracers(every=3, start_step=4)
        a.run(50, graph=True)
        b.seed_tracers(seeds, sort_every=16, **kw)            # (the checkpoint is written from sorted slots)
        b.accumulate_tracers(every=3, start_step=4)
        b.run(23, graph=True)
        dev, tr = b._dev, b._tracers.set
        state = dev.tracer_read(tr)
        vel = dev.tracer_read_vel(tr)
        dep = dev.tracer_deposits(tr)
        occ, age, launches, samples = dev.tracer_accum_read(tr)
        assert state["steps"] == 23 and launches == 23 and samples == 6
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
        c.seed_tracers(seeds, **kw)
        cd, ct = c._dev, c._tracers.set
        cd.tracer_write(ct, state)
        cd.tracer_write_vel(ct, *vel)
        cd.tracer_deposits_write(ct, dep)
        c.accumulate_tracers(every=3, start_step=4)
        cd.tracer_accum_write(ct, occ, age, launches, samples)
        back = cd.tracer_accum_read(ct)
        assert np.array_equal(back[0], occ) and np.array_equal(back[1], age) and back[2:] == (23, 6)
        c.run(27, graph=True)
        ra, rc = a.tracers(), c.tracers()
        assert ra["steps"] == rc["steps"] == 50
        for k in ra:
            assert np.array_equal(ra[k], rc[k], equal_nan=True), f"resumed {k}"
        assert np.array_equal(a.tracer_deposits(), c.tracer_deposits())
        ga, gc = a.tracer_accumulation(), c.tracer_accumulation()
        for k in ga:
            assert np.array_equal(ga[k], gc[k]), f"resumed accumulator {k}"
        assert ga["samples"] == 15
        from fs import _lib
        with pytest.raises(_lib.FsError):
            cd.tracer_accum_write(ct, occ, age, 51, 6)        # older than the set
    finally:
        for sim in (a, b, c):
            if sim is not None:
                _close(sim)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_capture_rules(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, cfg)
    dev = sim._dev
    mask = g["bc_mask"]
    fluid = np.argwhere(mask == 0)[0] + 0.5
    try:
        for kw in (dict(gravity=(0.0, -1.0)), dict(deposits=True), dict(tau=-0.5), dict(tau=[0.1, 0.2, 0.3])):
            with pytest.raises(ValueError):
                sim.seed_tracers([fluid, fluid + 0.25], **kw)
        assert sim._tracers is None
        with pytest.raises(RuntimeError):
            sim.accumulate_tracers()                          # no set
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.seed_tracers([fluid], tau=0.1))
        sim.seed_tracers([fluid, fluid + 0.25], tau=0.1)
        with pytest.raises(RuntimeError):
            sim.tracer_deposits()                             # no plane without the flag
        with pytest.raises(RuntimeError):
            dev.capture(lambda: sim.accumulate_tracers())
        sim.accumulate_tracers(every=2)
        with pytest.raises(RuntimeError):
            sim.accumulate_tracers()                          # attached already
        for bad in (dict(every=0), dict(start_step=-1)):
            with pytest.raises((ValueError, RuntimeError)):
                sim.accumulate_tracers(**bad)
        sim.run(3, graph=False)
        tr = sim._tracers.set
        h = tr._h
        # the library refuses on its own as well (FS_ERR_STATE = -3, FS_ERR_ARG = -1)
        one = (ctypes.c_double * 2)(*fluid)
        a1, t1 = (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(0.0)
        vel = (ctypes.c_double * 4)()
        ll = ctypes.c_longlong()
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_tracer_create_inertial(dev._ctx, 1, one, a1, t1, 0.0, 0.0, 1, 0, 0, ctypes.byref(ctypes.c_void_p())),
                  dev._lib.fs_tracer_read_vel(dev._ctx, h, vel),
                  dev._lib.fs_tracer_write_vel(dev._ctx, h, vel),
                  dev._lib.fs_tracer_accum_read(dev._ctx, h, None, None, ctypes.byref(ll), ctypes.byref(ll)),
                  dev._lib.fs_tracer_accum_reset(dev._ctx, h),
                  dev._lib.fs_tracer_accum_create(dev._ctx, h, 1, 0)]
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", dev._ctx, gid.value)
        assert st == [-3] * 6, st
        assert dev._lib.fs_tracer_accum_create(dev._ctx, h, 1, 0) == -3            # a second accumulator
        for alpha, tau_ in ((0.0, 0.1), (1.5, 0.1), (float("nan"), 0.1), (0.5, -1.0), (0.5, float("inf"))):
            a1[0], t1[0] = alpha, tau_
            assert dev._lib.fs_tracer_create_inertial(dev._ctx, 1, one, a1, t1, 0.0, 0.0, 1, 0, 0, ctypes.byref(ctypes.c_void_p())) == -1
        a1[0], t1[0] = 1.0, 0.0
        assert dev._lib.fs_tracer_create_inertial(dev._ctx, 1, one, a1, t1, float("nan"), 0.0, 1, 0, 0, ctypes.byref(ctypes.c_void_p())) == -1
        assert dev._lib.fs_tracer_deposits(dev._ctx, h, (ctypes.c_int * 1)()) == -1      # no plane
        passive = dev.tracer_create(np.array([fluid]))
        assert dev._lib.fs_tracer_read_vel(dev._ctx, passive._h, vel) == -1              # not an inertial set
        assert dev._lib.fs_tracer_accum_add(dev._ctx, passive._h) == -1                  # no accumulator
        dev.tracer_free(passive)
        assert sim.tracers()["steps"] == 3 and sim.tracer_accumulation()["samples"] == 1
        # stop inside a capture: the releases wait for the end of the capture; the graph is never replayed
        v = sim._solver.get_fields()[0]
        gid = dev.capture(lambda: (dev.tracer_advance(tr, 0.05, v), dev.tracer_accum_add(tr), sim.stop_tracer_accumulation(), sim.stop_tracers()))
        dev.free_graph(gid)
        assert sim._tracers is None and tr._h is None and tr.accum is None
        sim.seed_tracers([fluid], tau=0.0, deposits=True)
        sim.accumulate_tracers()
        sim.run(20, graph=True)
        assert sim.tracers()["steps"] == 20 and sim.tracer_accumulation()["samples"] == 20
    finally:
        _close(sim)


def test_slab_contexts_refuse(hip_lib):
    """A slab context (one of two ranks; no communicator is needed to ask): creation is refused by the library and by the runtime."""
    from fs import _lib
    from fs.runtime import Device, DeviceBase
    dev = Device(64, 32, "f32", gpu=0, rank=0, nranks=1)
    slab = ctypes.c_void_p()
    _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
    try:
        one = (ctypes.c_double * 2)(3.5, 3.5)
        a1, t1 = (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(0.0)
        rc = dev._lib.fs_tracer_create_inertial(slab, 1, one, a1, t1, 0.0, 0.0, 1, 0, 1, ctypes.byref(ctypes.c_void_p()))
        assert rc == -5, rc                                   # FS_ERR_UNSUPPORTED
        assert "slab" in dev._lib.fs_last_error().decode()
    finally:
        _lib.call("fs_destroy", slab)
        dev.close()

    class _Slab:
        nranks, capturing = 2, False
    with pytest.raises(_lib.FsError):
        DeviceBase.tracer_create_inertial(_Slab(), np.array([[1.5, 1.5]]), [1.0], [0.0])


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_gpu_inertial", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_files_and_resume(tmp_path, capsys, hip_lib):
    """tracers.npz and tracer_fields.npz carry the extra keys; 9 + 12 steps over a checkpoint equal 21 uninterrupted ones bit for bit."""
    cli = _cli()
    common = ["-bc", "5", "-res", "64", "--tracers", "300", "--tracer-seed", "9", "--tracer-tau", "0,0.002,0.05", "--tracer-gravity", "0,-4",
              "--tracer-deposits", "--tracer-accumulate-every", "2", "--tracer-accumulate-start", "3", "--tracer-fields", "--tracer-max-age", "15",
              "--graph"]
    a, b = tmp_path / "a", tmp_path / "b"
    cli.main(common + ["--steps", "21", "--out", str(a)])
    t = np.load(a / "tracers.npz")
    assert sorted(t.files) == sorted(["age", "respawns", "seeds", "status", "steps", "x", "y", "u", "w", "tau"]) and int(t["steps"]) == 21
    assert np.array_equal(t["tau"], np.resize([0.0, 0.002, 0.05], 300))
    f = np.load(a / "tracer_fields.npz")
    assert {"count", "age_sum", "residence", "step", "deposits", "occupancy", "accumulated_age_sum", "samples"} == set(f.files)
    assert int(f["samples"]) == 9 and f["occupancy"].sum() == 9 * 300 and f["deposits"].dtype == np.int32
    b.mkdir()
    cli.main(common + ["--steps", "9", "--out", str(b), "--save-state", str(b / "ck.npz")])
    ck = np.load(b / "ck.npz")
    assert {"tracer.u", "tracer.w", "tracer.tau", "tracer.gravity", "tracer.deposits", "tracer.accum.occupancy", "tracer.accum.samples"} <= set(ck.files)
    cli.main(common + ["--steps", "12", "--out", str(b), "--load-state", str(b / "ck.npz")])
    r, rf = np.load(b / "tracers.npz"), np.load(b / "tracer_fields.npz")
    for k in t.files:
        assert np.array_equal(r[k], t[k], equal_nan=True), f"{k}: the resumed particles differ from the uninterrupted run's"
    for k in ("deposits", "occupancy", "accumulated_age_sum", "samples", "count", "age_sum"):
        assert np.array_equal(rf[k], f[k]), f"{k}: the resumed run differs from the uninterrupted one"
    capsys.readouterr()
    # a passive run keeps its files as they were
    p = tmp_path / "p"
    p.mkdir()
    cli.main(["-bc", "5", "-res", "64", "--tracers", "50", "--tracer-fields", "--steps", "4", "--out", str(p), "--save-state", str(p / "ck.npz")])
    assert sorted(np.load(p / "tracers.npz").files) == ["age", "respawns", "seeds", "status", "steps", "x", "y"]
    assert sorted(np.load(p / "tracer_fields.npz").files) == ["age_sum", "count", "residence", "step"]
    assert not [k for k in np.load(p / "ck.npz").files if k.startswith("tracer.") and k.split(".", 1)[1] in ("u", "w", "tau", "gravity", "deposits")]
