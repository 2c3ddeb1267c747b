"""The vortex rider's host logic on the NumPy stand-in device (tests/vortex_standin.py on top of the POD's): the sampling rule, the ring's
wrap and drain under run() and eager steps, the checkpoint round trip, find_vortices / vortex_labels / vortex_criterion, the launch and token
order, the refusals.  The device kernels themselves: tests/test_gpu_vortices.py; the union-find they run: tests/test_vortex_cpu.py."""
import functools

import numpy as np
import pytest

import vortex_ref as R

FNAME = "traj_bc3_upwind_vc0.npz"


class _Thr:
    """The threshold of the tests: the highest of the 0.85, 0.7, 0.5, 0.3 quantiles of the "q" criterion over the fluid cells after 8 steps at
    which the restatement finds at least four components (of any size) and two of 4 cells.  Computed once, on the stand-in."""

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def value():
        b, _ = _sim()
        b.run(8)
        mask, dx = np.asarray(b._solver._bc.mask), b._solver.dx
        v = b.field_to_numpy()["v"].copy()
        c, _ = R.criterion("q", v, mask, dx)
        for quantile in (0.85, 0.7, 0.5, 0.3):
            thr = float(np.quantile(c[mask == 0], quantile))
            s = R.sample(v, mask, dx, "q", thr, R.omega_exponent(2 * 10.0 / dx))
            if s["count"] >= 2 and s["components"] >= 4:
                return thr
        raise AssertionError("no quantile leaves components: the tests would cover nothing")

    def __float__(self):
        return self.value()


THR = _Thr()


@pytest.fixture(scope="module")
def standin():
    import fs
    from vortex_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from vortex_standin import make_sim
    return make_sim(FNAME)


def _reference(steps, want, **kw):
    """{step: restatement sample of a twin's download after that step}."""
    b, _ = _sim()
    mask, dx = np.asarray(b._solver._bc.mask), b._solver.dx
    e = R.omega_exponent(2 * 10.0 / dx)
    out = {}
    for n in range(1, steps + 1):
        b.step()
        if n in want:
            out[n] = R.sample(b.field_to_numpy()["v"].copy(), mask, dx, "q", float(THR), e, **kw)
    return out, e, dx, mask.shape[0], b.field_to_numpy()


def _assert_samples(out, ref, e, dx, nx):
    steps = sorted(ref)
    assert out["step"].tolist() == steps
    assert out["exponent"] == e
    for k, step in enumerate(steps):
        r = ref[step]
        for name in ("components", "passed", "count", "clipped", "dropped_cells"):
            assert out[name][k] == r[name], (step, name)
        m = out["sample"] == k
        for name in R.RECORD:
            assert np.array_equal(out["raw"][name][m], r["raw"][name]), (step, name)
        conv = R.convert(r["raw"], e, dx, nx)
        for name, w in conv.items():
            assert np.array_equal(out[name][m], w), (step, name)
    assert sum(int(c) for c in out["count"]) > 0, "no vortex in any sample: the test covers nothing"


@pytest.mark.parametrize("every,start,capacity,eager", [(1, 0, 3, False), (1, 0, 3, True), (3, 2, None, False), (2, 5, 2, True)])
def test_rider_follows_the_sampling_rule_and_the_ring_wraps(every, start, capacity, eager, standin):
    steps = 14
    want = [k for k in range(1, steps + 1) if k > start and (k - start) % every == 0]
    ref, e, dx, nx, final = _reference(steps, want)
    a, _ = _sim()
    a.track_vortices(THR, every=every, start_step=start, capacity=capacity)
    if eager:
        for _ in range(steps):
            a.step()
    else:
        a.run(steps // 2)
        a.run(steps - steps // 2)
    r = a._vortexr
    if capacity is not None:
        assert r.drained > 0 and r.room() >= 0, "the ring never filled: the test does not cover the drain"
    out = a.vortices()
    _assert_samples(out, ref, e, dx, nx)
    assert np.allclose(out["time"], out["step"] * a._solver.dt)
    planes = a.vortex_labels()
    assert np.array_equal(planes["flags"], ref[want[-1]]["flags"]) and np.array_equal(planes["labels"], ref[want[-1]]["labels"])
    fa = a.field_to_numpy()
    assert all(np.array_equal(fa[k], final[k]) for k in fa), "the rider changed the trajectory"
    a.stop_vortices()
    assert a._vortexr is None and a.vortices()["step"].tolist() == want      # kept after the stop
    assert np.array_equal(a.vortex_labels()["labels"], planes["labels"])


def test_ring_room_counts_steps_until_the_ring_is_full(standin):
    a, _ = _sim()
    a.track_vortices(THR, every=3, start_step=2, capacity=2)
    r = a._vortexr
    assert r.room() == 10                    # the samples of steps 5 and 8 fit the ring; the launch of step 11 would find it full
    a.run(10)
    assert r.room() == 0 and r.drained == 0
    a.run(1)                                 # drains first
    assert r.drained == 2 and r.issued == 11
    assert a.vortices()["step"].tolist() == [5, 8, 11]


def test_launch_order_token_and_caps(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    base = sim._signature()
    # attached before the others, rides behind them
    sim.track_vortices(THR, max_vortices=2, max_components=3, min_area=1)
    sim.track_body(default_body_box(cfg["bc"], cfg["res"]), every=2, capacity=10)
    sim.start_pod(3)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    assert names[-3:] == ["pod_launch", "loads_record", "vortex_launch"] and names.count("vortex_launch") == 1, names[-4:]
    marker = type("T", (), {})()
    sim._tracers = marker                    # (this stand-in has no tracer primitives: only the order is asked)
    assert sim._riders()[-2:] == [marker, sim._vortexr], "the vortex tracker does not ride last, behind the tracers"
    sim._tracers = None
    sig = sim._signature()
    assert sig[-1] == ("vortices", sim._vortexr.vx.serial) and len(sig) > len(base)
    r = sim._vortexr
    assert not r.replaces_attached and not r.stop_in_capture and r.keeps_last
    out = sim.vortices()
    ref, e, dx, nx, _ = _reference(1, [1], max_vortices=2, max_components=3, min_area=1)
    _assert_samples(out, ref, e, dx, nx)
    assert ref[1]["count"] == 2 and ref[1]["passed"] == 3 and ref[1]["components"] > 3 and ref[1]["dropped_cells"] > 0, "the caps do not bite"


def test_checkpoint_and_restore(standin):
    steps, every, start = 16, 3, 1
    want = [k for k in range(1, steps + 1) if k > start and (k - start) % every == 0]
    ref, e, dx, nx, _ = _reference(steps, want)
    a, _ = _sim()
    a.track_vortices(THR, every=every, start_step=start, capacity=2)
    a.run(9)
    z = a._vortexr.checkpoint()
    assert set(z) == {"vortex.words", "vortex.launches", "vortex.every", "vortex.start", "vortex.criterion", "vortex.threshold", "vortex.exponent",
                      "vortex.min_area", "vortex.max_vortices", "vortex.max_components"}
    assert int(z["vortex.launches"]) == 9 and len(z["vortex.words"]) == 2 and z["vortex.words"].dtype == np.int64
    a.stop_vortices()
    a.track_vortices(THR, every=every, start_step=start, capacity=2)
    assert a._vortexr.restore(z) == len(a._vortexr._words[0]) == 2          # (-> the samples taken over: the CLI's "samples so far")
    assert a._vortexr.room() == 6            # the samples of steps 10 and 13 fit the ring of 2; the launch of step 16 would find it full
    a.run(steps - 9)
    _assert_samples(a.vortices(), ref, e, dx, nx)
    with pytest.raises(ValueError):
        b, _ = _sim()
        b.track_vortices(THR, max_vortices=8)
        b._vortexr.restore(z)


def test_find_vortices_criterion_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    with pytest.raises(RuntimeError):
        sim.vortices()
    with pytest.raises(RuntimeError):
        sim.vortex_labels()
    with pytest.raises(TypeError):
        sim.track_vortices()
    for bad in (dict(threshold=None), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=1.0, criterion="lambda2"),
                dict(threshold=1.0, max_vortices=0), dict(threshold=1.0, max_vortices=1025), dict(threshold=1.0, every=0),
                dict(threshold=1.0, start_step=-1), dict(threshold=1.0, min_area=0), dict(threshold=1.0, omega_max=0.0),
                dict(threshold=1.0, capacity=0)):
        with pytest.raises(ValueError):
            sim.track_vortices(**bad)
    assert sim._vortexr is None
    sim.run(6)
    mask, dx = np.asarray(sim._solver._bc.mask), sim._solver.dx
    v = sim.field_to_numpy()["v"].copy()
    for which in R.CRITERIA:
        assert np.array_equal(sim.vortex_criterion(which), R.criterion(which, v, mask, dx)[0])
    e = R.omega_exponent(2 * 10.0 / dx)
    sig = sim._signature()
    out = sim.find_vortices(THR, "swirl", min_area=2)
    assert sim._signature() == sig and sim._vortexr is None          # nothing attached
    ref = R.sample(v, mask, dx, "swirl", float(THR), e, min_area=2)
    _assert_samples(out, {0: ref}, e, dx, mask.shape[0])
    assert np.array_equal(sim.vortex_labels()["labels"], ref["labels"]) and np.array_equal(sim.vortex_labels()["flags"], ref["flags"])
    sim.track_vortices(THR)
    with pytest.raises(RuntimeError):
        sim.track_vortices(THR)                                      # a second attach
    sim.run(2)
    dev = sim._dev
    dev.capturing = True
    try:
        for call in (sim.vortices, sim.vortex_labels, lambda: sim.find_vortices(THR), lambda: sim.vortex_criterion("q"), sim.stop_vortices,
                     lambda: sim.track_vortices(THR)):
            with pytest.raises((RuntimeError, _lib.FsError)):
                call()
        for call in (lambda: dev.vortex_read(sim._vortexr.vx), lambda: dev.vortex_labels(sim._vortexr.vx), lambda: dev.vortex_set(sim._vortexr.vx, 0),
                     lambda: dev.vortex_label(np.zeros(mask.shape, np.uint8)), lambda: dev.vortex_criterion("q", dx, sim._solver.get_fields()[0]),
                     lambda: dev.vortex_create("q", 1.0, 0)):
            with pytest.raises(_lib.FsError):
                call()
    finally:
        dev.capturing = False
    assert sim._vortexr is not None and len(sim.vortices()["step"]) == 2
    saved = dev.nranks
    dev.nranks = 2
    try:
        for call in (lambda: sim.find_vortices(THR), lambda: sim.vortex_criterion("q"), lambda: dev.vortex_label(np.zeros(mask.shape, np.uint8))):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
    # a ring that fills outside run() / step(): the lost samples are reported, not hidden
    sim.stop_vortices()
    sim.track_vortices(THR, capacity=1)
    v_f = sim._solver.get_fields()[0]
    for _ in range(3):
        dev.vortex_launch(sim._vortexr.vx, dx, v_f)
    with pytest.raises(RuntimeError, match="2 vortex sample"):
        sim.vortices()
