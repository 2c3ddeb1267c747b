"""Inertial tracer particles, wall deposition and accumulated occupancy without a device: the NumPy restatement (tests/inertial_ref.py) on
flows with a known answer and with every fate produced by construction, the host helpers of fs/tracers.py, the argument checks of the
runtime and the simulator, the command line and the checkpoint key sets."""
import importlib.util
import os
import re

import numpy as np
import pytest
from conftest import REPO
from inertial_ref import (accumulate_ref, advance_ref, band_scene, fields_ref, new_accumulator, new_state, response_ref, samples_step)
from test_build_metadata import kernels  # noqa: F401  (the fixture that reads the code objects of the built library)
from tracers_ref import ALIVE, EXPIRED, LEFT, WALL_HIT, fate_scene
import tracers_ref


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_inertial", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the restatement on flows with a known answer -----------------------------------------------------------------------------------------
def test_relaxation_to_the_settling_velocity():
    """Uniform flow u = 0.25 and gravity (0, -2): pw_n = tau gy (1 - (1 - alpha)^n) and pu_n = 0.25 exactly.  The bound 1e-12 on the
    relative error of pw is the issue's; the recurrence itself loses a few ulp (measured 2.1e-16)."""
    X = Y = 64
    v = np.zeros((X, Y, 2), np.float32)
    v[..., 0] = 0.25
    mask = np.zeros((X, Y), np.uint8)
    tau, dt, h, gy = 0.05, 0.01, 0.5, -2.0
    alpha = float(response_ref(tau, dt))
    st = new_state([[5.5, 60.5]], alpha, tau)
    worst = 0.0
    for n in range(1, 41):
        advance_ref(st, v, mask, h, gravity=(0.0, gy), respawn=False)
        exact = tau * gy * (1.0 - (1.0 - alpha) ** n)
        worst = max(worst, abs(st["pw"][0] / exact - 1.0))
        assert st["pu"][0] == 0.25, n
    print(f"relative error of pw over 40 steps: {worst:.3g}")
    assert worst <= 1e-12
    assert st["status"][0] == ALIVE and st["age"][0] == 40 and st["x"][0] == 5.5 + 40 * h * 0.25 and st["y"][0] < 60.5


def _run_band(alpha, tau):
    mask, v, seeds = band_scene()
    st = new_state(seeds, alpha, tau)
    dep = np.zeros(mask.shape, np.int32)
    for _ in range(80):
        advance_ref(st, v, mask, 0.5, respawn=False, deposits=dep)
    return mask, st, dep


def test_inertia_decides_the_fate():
    """The same seeds in the same flow: light particles turn with the band and leave through the top edge, heavy ones cross it and
    deposit on the block behind - one count in each of the cells (20, 7), (20, 8), (20, 9)."""
    mask, st, dep = _run_band(1.0, 0.0)
    assert np.all(st["status"] == LEFT) and not dep.any()
    assert np.all(st["y"] > 15.0) and np.all(st["x"] < 20.0)            # (LEFT keeps the last valid position: below the top edge, in the band)
    mask, st, dep = _run_band(0.05, 1.0)
    assert np.all(st["status"] == WALL_HIT)
    exp = np.zeros_like(dep)
    exp[20, 7] = exp[20, 8] = exp[20, 9] = 1
    assert np.array_equal(dep, exp)
    assert np.all(mask[np.nonzero(dep)] == 1)


def test_alpha_one_is_the_forward_euler_tracer():
    """tau = 0: x + h V(x) - one gather, not the passive set's midpoint rule."""
    rng = np.random.default_rng(5)
    X, Y = 40, 24
    v = rng.standard_normal((X, Y, 2)).astype(np.float32)
    mask = np.zeros((X, Y), np.uint8)
    seeds = rng.uniform(8.0, 16.0, (50, 2))
    st = new_state(seeds, 1.0, 0.0)
    U, W = tracers_ref.velocity_ref(v, seeds[:, 0], seeds[:, 1])
    advance_ref(st, v, mask, 0.25, respawn=False)
    assert np.array_equal(st["x"], seeds[:, 0] + 0.25 * U) and np.array_equal(st["y"], seeds[:, 1] + 0.25 * W)
    assert np.array_equal(st["pu"], U) and np.array_equal(st["pw"], W)
    mid = tracers_ref.new_state(seeds)
    tracers_ref.advance_ref(mid, v, mask, 0.25, respawn=False)
    assert not np.array_equal(mid["x"], st["x"])


@pytest.mark.parametrize("respawn", [False, True])
def test_every_fate_with_and_without_respawn(respawn):
    """tracers_ref.fate_scene with alpha = 1: the particles follow the flow with one Euler step; every fate occurs, the NaN cell gives
    LEFT on the first step, a wall hit is deposited whether the particle respawns or not."""
    mask, v, seeds, expected = fate_scene()
    st = new_state(seeds, 1.0, 0.0)
    dep = np.zeros(mask.shape, np.int32)
    seen = set()
    for _ in range(25):
        seen |= set(advance_ref(st, v, mask, 0.5, respawn=respawn, max_age=20, deposits=dep).tolist())
    assert seen == {ALIVE, LEFT, WALL_HIT, EXPIRED}
    assert st["steps"] == 25
    if not respawn:
        assert np.array_equal(st["status"], expected) and not st["respawns"].any()
        assert st["x"][0] == 19.5 and st["age"][0] == 19 and st["pu"][0] == 1.0         # WALL: the last valid position, the velocity it hit with
        assert st["x"][3] == 3.5 and st["y"][3] == 1.5 and st["age"][3] == 1             # NaN: LEFT where it was ...
        assert np.isnan(st["pu"][3]) and np.isnan(st["pw"][3])                           # ... and the updated velocity is stored in every case
        assert st["x"][4] == 12.5 and st["age"][4] == 20                                 # EXPIRED keeps the step it took
        assert dep.sum() == 1 and dep[20, 5] == 1
        frozen = {k: st[k].copy() for k in ("x", "y", "age", "status", "pu", "pw")}
        advance_ref(st, v, mask, 0.5, respawn=False, max_age=20, deposits=dep)
        assert all(np.array_equal(st[k], frozen[k], equal_nan=True) for k in frozen), "a dead particle was touched"
        assert dep.sum() == 1
    else:
        assert np.all(st["status"] == ALIVE) and np.array_equal(st["respawns"], [1, 1, 6, 25, 1])
        assert dep.sum() == 1 and dep[20, 5] == 1
        assert st["age"][3] == 0 and st["pu"][3] == 0.0 and st["pw"][3] == 0.0           # a respawn stores pu = pw = 0 ...
        advance_ref(st, v, mask, 0.5, respawn=True, max_age=20, deposits=dep)
        assert st["respawns"][3] == 26                                                   # ... and age 0 takes the fluid's (NaN here) again


def test_heavy_particle_keeps_its_velocity_over_a_respawn_only_through_the_fluid():
    """After a respawn the particle starts with the fluid's velocity at its seed, not with what it had."""
    X, Y = 16, 8
    v = np.zeros((X, Y, 2), np.float64)
    v[:8, :, 0] = 2.0          # fast at the seed ...
    v[8:, :, 0] = 0.5          # ... slow further on
    mask = np.zeros((X, Y), np.uint8)
    mask[X - 1, :] = 3
    st = new_state([[1.5, 3.5]], 0.1, 1.0)
    resp = 0
    for _ in range(60):
        advance_ref(st, v, mask, 0.5)
        if st["respawns"][0] > resp:
            resp = st["respawns"][0]
            assert st["age"][0] == 0 and st["pu"][0] == 0.0
            advance_ref(st, v, mask, 0.5)
            assert st["pu"][0] == 2.0 and st["age"][0] == 1
    assert resp >= 1


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------
def test_sampling_rule_is_the_time_averages():
    assert [k for k in range(1, 12) if samples_step(k, 1, 0)] == list(range(1, 12))
    assert [k for k in range(1, 12) if samples_step(k, 3, 0)] == [3, 6, 9]
    assert [k for k in range(1, 12) if samples_step(k, 3, 4)] == [7, 10]
    assert [k for k in range(1, 8) if samples_step(k, 1, 5)] == [6, 7]


@pytest.mark.parametrize("every,start", [(1, 0), (3, 4)])
def test_accumulator_is_the_sum_of_the_snapshots(every, start):
    mask, v, seeds = band_scene()
    X, Y = mask.shape
    rng = np.random.default_rng(2)
    seeds = np.concatenate([seeds, rng.uniform(1.0, 12.0, (40, 2))])
    st = new_state(seeds, 0.3, 0.2)
    acc = new_accumulator(X, Y, every, start)
    occ, age, n = np.zeros((X, Y), np.int64), np.zeros((X, Y), np.int64), 0
    for k in range(1, 31):
        advance_ref(st, v, mask, 0.5, respawn=True, max_age=25)
        accumulate_ref(acc, st)
        if k > start and (k - start) % every == 0:
            c, a = fields_ref(st, X, Y)
            occ, age, n = occ + c, age + a, n + 1
    assert acc["steps"] == 30 and acc["samples"] == n > 0
    assert np.array_equal(acc["occupancy"], occ) and np.array_equal(acc["age_sum"], age)
    assert acc["occupancy"].sum() == n * len(seeds)            # (with respawn every particle is alive and inside at every sample)


# ---- host helpers -------------------------------------------------------------------------------------------------------------------------
def test_response_endpoints_and_monotonicity():
    from fs.tracers import concentration, response, stokes_number
    assert response(0.0, 0.01) == 1.0
    assert response(1e-9, 0.01) == 1.0                          # exp(-1e7) rounds away
    assert response(0.05, 0.01) == -np.expm1(-(0.01 / 0.05)) and abs(response(0.05, 0.01) - (1.0 - np.exp(-0.2))) < 1e-15
    big = response(1e12, 0.01)
    assert 0.0 < big < 1.1e-14 and big == -np.expm1(-(0.01 / 1e12))     # (no cancellation for tau >> dt)
    taus = np.concatenate([[0.0], np.logspace(-6, 6, 200)])
    a = response(taus, 0.01)
    assert a.shape == taus.shape and a.dtype == np.float64 and np.all((a > 0) & (a <= 1)) and np.all(np.diff(a) <= 0) and a[-1] < a[0]
    assert np.array_equal(a, response_ref(taus, 0.01))
    for bad in (lambda: response(-1.0, 0.01), lambda: response(np.nan, 0.01), lambda: response(np.inf, 0.01), lambda: response(1.0, 0.0),
                lambda: response([0.1, -0.1], 0.01)):
        with pytest.raises(ValueError):
            bad()
    assert stokes_number(0.5, 2.0, 4.0) == 0.25 and np.array_equal(stokes_number([0.0, 1.0], 1.0, 0.5), [0.0, 2.0])
    with pytest.raises(ValueError):
        stokes_number(1.0, 1.0, 0.0)
    occ = np.array([[0, 6], [3, 0]], np.int64)
    assert np.array_equal(concentration(occ, 3), [[0.0, 2.0], [1.0, 0.0]])
    with pytest.raises(ValueError):
        concentration(occ, 0)


def test_tokens_and_keys():
    from fs import tracers

    class _Set:
        serial = 41

    class _Acc:
        serial = 77
    t = tracers.Tracers(None, _Set(), np.zeros((2, 2)), True, 0, 0, tau=np.array([0.1, 0.2]), gravity=(0.0, -1.0), deposits=True)
    assert t.token == ("tracer", 41) and t.gravity == (0.0, -1.0) and t.deposits is True and t.accumulation is None
    p = tracers.Tracers(None, _Set(), np.zeros((2, 2)), True, 0)
    assert p.tau is None and p.gravity == (0.0, 0.0) and p.deposits is False
    a = tracers.TracerAccumulation(_Acc(), 3, 5)
    assert a.token == ("tracer_accum", 77) and (a.every, a.start_step) == (3, 5)
    assert tracers.INERTIAL_KEYS == ("u", "w", "tau") and not set(tracers.INERTIAL_KEYS) & set(tracers.KEYS)


# ---- argument refusals (no device is reached) ---------------------------------------------------------------------------------------------
class _NoDevice:
    nranks, capturing, nx, ny = 1, False, 8, 4
    _handle_serial = {}

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the device ({name})")


def test_runtime_refuses_bad_arguments_before_the_device():
    from fs import _lib
    from fs.runtime import DeviceBase, TracerSet
    dev = _NoDevice()
    seeds = np.array([[1.5, 1.5], [2.5, 1.5]])
    ok = dict(alpha=[1.0, 0.5], tau=[0.0, 0.1])
    for kw in (dict(ok, alpha=[1.0, 0.0]), dict(ok, alpha=[1.0, 1.5]), dict(ok, alpha=[np.nan, 1.0]), dict(ok, tau=[0.0, -1.0]),
               dict(ok, tau=[0.0, np.inf]), dict(ok, alpha=[1.0]), dict(ok, tau=[[0.0, 0.1]]), dict(ok, gravity=(0.0, np.nan)),
               dict(ok, gravity=(0.0,)), dict(ok, max_age=-1)):
        with pytest.raises(ValueError):
            DeviceBase.tracer_create_inertial(dev, seeds, **kw)
    with pytest.raises(ValueError):
        DeviceBase.tracer_create_inertial(dev, np.zeros((0, 2)), [], [])

    class _Slab(_NoDevice):
        nranks = 2

    class _Capturing(_NoDevice):
        capturing = True
    for d in (_Slab(), _Capturing()):
        with pytest.raises(_lib.FsError):
            DeviceBase.tracer_create_inertial(d, seeds, **ok)
        with pytest.raises(_lib.FsError):
            DeviceBase.tracer_accum_create(d, TracerSet(None, 2, True, 0))
    passive = TracerSet(None, 2, True, 0)
    for call in (lambda: DeviceBase.tracer_read_vel(dev, passive), lambda: DeviceBase.tracer_write_vel(dev, passive, [0, 0], [0, 0]),
                 lambda: DeviceBase.tracer_deposits(dev, passive), lambda: DeviceBase.tracer_deposits_write(dev, passive, np.zeros((8, 4))),
                 lambda: DeviceBase.tracer_accum_create(dev, passive, every=0), lambda: DeviceBase.tracer_accum_create(dev, passive, start=-1)):
        with pytest.raises(ValueError):
            call()
    inert = TracerSet(None, 2, True, 0)
    inert.inertial = inert.deposits = True
    with pytest.raises(ValueError):
        DeviceBase.tracer_write_vel(dev, inert, [0.0], [0.0, 0.0])
    with pytest.raises(ValueError):
        DeviceBase.tracer_deposits_write(dev, inert, np.zeros((4, 8)))
    with pytest.raises(ValueError):
        DeviceBase.tracer_deposits_write(dev, inert, -np.ones((8, 4)))
    with pytest.raises(ValueError):
        DeviceBase.tracer_accum_write(dev, inert, np.zeros((8, 4)), np.zeros((8, 4)), 3, 4)
    with pytest.raises(ValueError):
        DeviceBase.tracer_accum_write(dev, inert, np.zeros((8, 3)), np.zeros((8, 4)), 4, 3)
    inert.accum = object()
    with pytest.raises(RuntimeError):
        DeviceBase.tracer_accum_create(dev, inert)            # a second accumulator


def test_simulator_refuses_gravity_or_deposits_without_tau():
    import fs

    class _Bc:
        mask = np.zeros((8, 4), np.uint8)

    class _Solver:
        _bc, dt, dx = _Bc(), 0.01, 0.125

    class _Sim(fs.FluidSimulator):
        def __init__(self):
            self._tracers = None
    sim = _Sim()
    sim._dev, sim._solver = _NoDevice(), _Solver()
    seeds = np.array([[1.5, 1.5]])
    for kw in (dict(gravity=(0.0, -1.0)), dict(deposits=True), dict(tau=-1.0), dict(tau=np.nan), dict(tau=[0.1, 0.2]), dict(tau=0.1, gravity=(1.0,)),
               dict(tau=0.1, gravity=(0.0, np.inf))):
        with pytest.raises(ValueError):
            fs.FluidSimulator.seed_tracers(sim, seeds, **kw)
    assert sim._tracers is None
    for call in (fs.FluidSimulator.accumulate_tracers, fs.FluidSimulator.tracer_accumulation, fs.FluidSimulator.reset_tracer_accumulation,
                 fs.FluidSimulator.tracer_deposits):
        with pytest.raises(RuntimeError):
            call(sim)                                          # no tracer set
    fs.FluidSimulator.stop_tracer_accumulation(sim)            # nothing attached: nothing happens


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.tracer_tau, a.tracer_gravity, a.tracer_deposits, a.tracer_accumulate_every, a.tracer_accumulate_start) == (None, None, False, 0, None)
    a = cli.build_parser().parse_args(["--tracers", "100", "--tracer-tau", "0.01,0.1,1", "--tracer-gravity", "0,-9.8", "--tracer-deposits",
                                       "--tracer-accumulate-every", "4", "--tracer-accumulate-start", "100"])
    assert (a.tracer_tau, a.tracer_gravity, a.tracer_deposits, a.tracer_accumulate_every, a.tracer_accumulate_start) == ("0.01,0.1,1", "0,-9.8", True, 4, 100)
    assert np.array_equal(cli.tracer_taus([0.01, 0.1, 1.0], 7), [0.01, 0.1, 1.0, 0.01, 0.1, 1.0, 0.01])
    for argv in (["--tracer-tau", "0.1"],                           # without --tracers / --tracer-line
                 ["--tracer-gravity", "0,-1"],
                 ["--tracer-deposits"],
                 ["--tracer-accumulate-every", "2"],
                 ["--tracer-accumulate-start", "2"],
                 ["--tracers", "10", "--tracer-gravity", "0,-1"],   # without --tracer-tau
                 ["--tracers", "10", "--tracer-deposits"],
                 ["--tracers", "10", "--tracer-tau", "-0.1"],
                 ["--tracers", "10", "--tracer-tau", "a"],
                 ["--tracers", "10", "--tracer-tau", "0.1,nan"],
                 ["--tracers", "10", "--tracer-tau", "0.1", "--tracer-gravity", "1"],
                 ["--tracers", "10", "--tracer-tau", "0.1", "--tracer-gravity", "1,2,3"],
                 ["--tracers", "10", "--tracer-accumulate-every", "-1"],
                 ["--tracers", "10", "--tracer-accumulate-every", "x"],
                 ["--tracers", "10", "--tracer-accumulate-start", "5"]):      # the start without --tracer-accumulate-every
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2, argv


def _checkpoint(path, n=4, inertial=True, deposits=True, accum=True):
    arrays = {"step": np.array(10), "tracer.x": np.ones(n), "tracer.y": np.ones(n), "tracer.age": np.zeros(n, np.int32),
              "tracer.status": np.zeros(n, np.int32), "tracer.respawns": np.zeros(n, np.int32), "tracer.seeds": np.ones((n, 2)),
              "tracer.steps": np.array(10), "tracer.respawn": np.array(True), "tracer.max_age": np.array(0)}
    if inertial:
        arrays.update({"tracer.u": np.zeros(n), "tracer.w": np.zeros(n), "tracer.tau": np.resize([0.1, 0.2], n), "tracer.gravity": np.array([0.0, -1.0])})
        if deposits:
            arrays["tracer.deposits"] = np.zeros((8, 4), np.int32)
    if accum:
        arrays.update({"tracer.accum.occupancy": np.zeros((8, 4), np.int64), "tracer.accum.age_sum": np.zeros((8, 4), np.int64),
                       "tracer.accum.steps": np.array(10), "tracer.accum.samples": np.array(5), "tracer.accum.every": np.array(2),
                       "tracer.accum.start": np.array(0)})
    np.savez(str(path), **arrays)


def test_checkpoint_with_other_inertial_parameters_is_refused(tmp_path, capsys):
    """--load-state of a checkpoint whose set has another tau, gravity, deposit plane or accumulation schedule: exit status 2 before any
    device work; Tracers.held keeps the return value the set always had."""
    from fs.tracers import Tracers
    cli = _cli()
    ck = tmp_path / "ck.npz"
    _checkpoint(ck)
    assert Tracers.held(np.load(str(ck))) == (True, 0, 4)
    more = Tracers.held_inertial(np.load(str(ck)))
    assert np.array_equal(more["tau"], [0.1, 0.2, 0.1, 0.2]) and more["gravity"] == (0.0, -1.0) and more["deposits"] is True and more["accumulate"] == (2, 0)
    right = ["--tracers", "4", "--tracer-tau", "0.1,0.2", "--tracer-gravity", "0,-1", "--tracer-deposits"]
    for argv in (["--tracers", "4"],                                                              # passive flags, inertial checkpoint
                 ["--tracers", "4", "--tracer-tau", "0.1", "--tracer-gravity", "0,-1", "--tracer-deposits"],
                 ["--tracers", "4", "--tracer-tau", "0.1,0.2", "--tracer-deposits"],
                 ["--tracers", "4", "--tracer-tau", "0.1,0.2", "--tracer-gravity", "0,-1"],
                 right,                                                                            # the checkpoint's accumulation would be dropped
                 right + ["--tracer-accumulate-every", "3"],
                 right + ["--tracer-accumulate-every", "2", "--tracer-accumulate-start", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--load-state", str(ck), "--out", str(tmp_path)])
        assert e.value.code == 2, argv
        assert "--load-state" in capsys.readouterr().err
    passive = tmp_path / "passive.npz"
    _checkpoint(passive, inertial=False, accum=False)
    assert Tracers.held(np.load(str(passive))) == (True, 0, 4)
    more = Tracers.held_inertial(np.load(str(passive)))
    assert more["tau"] is None and more["deposits"] is False and more["accumulate"] is None
    with pytest.raises(SystemExit) as e:
        cli.main(["--tracers", "4", "--tracer-tau", "0.1", "--load-state", str(passive), "--out", str(tmp_path)])
    assert e.value.code == 2 and "passive tracers" in capsys.readouterr().err
    plain = tmp_path / "plain.npz"
    np.savez(str(plain), step=np.array(10))
    assert Tracers.held_inertial(np.load(str(plain))) is None


class _StateDev:
    """Stands in for the device behind fs.tracers.Tracers.checkpoint."""

    def tracer_read(self, tr):
        n = 3
        return {"x": np.zeros(n), "y": np.zeros(n), "age": np.zeros(n, np.int32), "status": np.zeros(n, np.int32), "respawns": np.zeros(n, np.int32),
                "seeds": np.zeros((n, 2)), "steps": 5}

    def tracer_write(self, tr, arrays):
        self.written = arrays

    def tracer_read_vel(self, tr):
        return np.zeros(3), np.zeros(3)

    def tracer_deposits(self, tr):
        return np.zeros((8, 4), np.int32)

    def tracer_accum_read(self, tr):
        return np.zeros((8, 4), np.int64), np.zeros((8, 4), np.int64), 5, 2


def test_checkpoint_key_sets():
    """A passive set's checkpoint keeps exactly the keys it had; an inertial set, its deposits and an accumulation add theirs."""
    from fs.tracers import TracerAccumulation, Tracers

    class _Acc:
        serial = 3
    passive_keys = {f"tracer.{k}" for k in ("x", "y", "age", "status", "respawns", "seeds", "steps", "respawn", "max_age")}
    inertial_keys = passive_keys | {"tracer.u", "tracer.w", "tracer.tau", "tracer.gravity"}
    accum_keys = {f"tracer.accum.{k}" for k in ("occupancy", "age_sum", "steps", "samples", "every", "start")}
    dev = _StateDev()
    t = Tracers(dev, object(), np.zeros((3, 2)), True, 0)
    assert set(t.checkpoint()) == passive_keys
    assert t.restore(t.checkpoint()) == len(dev.written["seeds"]) == 3          # (-> the particles taken over: the CLI's "continuing" line)
    t.accumulation = TracerAccumulation(_Acc(), 2, 1)
    got = t.checkpoint()
    assert set(got) == passive_keys | accum_keys and int(got["tracer.accum.every"]) == 2 and int(got["tracer.accum.start"]) == 1
    t = Tracers(dev, object(), np.zeros((3, 2)), True, 0, tau=np.array([0.1, 0.2, 0.3]), gravity=(0.0, -1.0))
    got = t.checkpoint()
    assert set(got) == inertial_keys and np.array_equal(got["tracer.gravity"], [0.0, -1.0]) and got["tracer.tau"].dtype == np.float64
    t = Tracers(dev, object(), np.zeros((3, 2)), True, 0, tau=np.array([0.1, 0.2, 0.3]), deposits=True)
    t.accumulation = TracerAccumulation(_Acc(), 1, 0)
    assert set(t.checkpoint()) == inertial_keys | {"tracer.deposits"} | accum_keys


# ---- the binding table and the build ------------------------------------------------------------------------------------------------------
def test_abi_table_holds_the_new_entries():
    from fs import _lib
    assert _lib.ABI_VERSION >= 15
    for name in ("fs_tracer_create_inertial", "fs_tracer_read_vel", "fs_tracer_write_vel", "fs_tracer_deposits", "fs_tracer_deposits_write",
                 "fs_tracer_accum_create", "fs_tracer_accum_add", "fs_tracer_accum_read", "fs_tracer_accum_write", "fs_tracer_accum_reset",
                 "fs_tracer_accum_free"):
        assert name in _lib.EXPORTS, name


def test_inertial_advance_keeps_eight_waves_per_simd_without_scratch(kernels):  # noqa: F811
    """512 VGPRs per SIMD lane: 8 waves need <= 64 each.  All four instantiations (f32 / f64, with and without the deferred limit)."""
    got = {k: v for k, v in kernels.items() if re.search(r"25k_tracer_advance_inertialI[fd]Lb[01]E", k)}
    assert len(got) == 4, sorted(got)
    for name, k in got.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)


@pytest.mark.parametrize("pattern", [r"19k_tracer_accumulateE", r"30k_tracer_sort_scatter_inertialE", r"27k_tracer_sort_copy_inertialE"])
def test_accumulate_and_sort_kernels_have_no_scratch(pattern, kernels):  # noqa: F811
    got = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(got) == 1, (pattern, sorted(got))
    for name, k in got.items():
        assert k["scratch"] == 0 and k["vgprs"] <= 64, (name, k)
