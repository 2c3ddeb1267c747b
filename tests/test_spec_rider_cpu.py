"""The host logic of the energy spectra without a GPU: FluidSimulator.start_spectra / spectra / reset_spectra / stop_spectra / spectrum /
box_fft on the NumPy stand-in device (tests/spec_standin.py): launch and token order beside the other riders, the cadence, the reset, the
checkpoint round trip and its refusals, the refusals of bad boxes, run() not cut by the rider."""
import numpy as np
import pytest

import spec_ref as S

FNAME = "traj_bc3_upwind_vc0.npz"
BOX = (2, 1, 34, 17)


@pytest.fixture(scope="module")
def standin():
    import fs
    from spec_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from spec_standin import make_sim
    return make_sim(FNAME)


def _tabs(box, window):
    from fs import spectra
    return spectra.tables(box[2] - box[0], box[3] - box[1], window)


@pytest.mark.parametrize("every,start,steps", [(1, 0, 5), (2, 3, 16)])
def test_power_follows_the_steps(every, start, steps, standin):
    """run() in two chunks (graphs are not captured on the stand-in; the chunks are not cut) against the restatement on a twin's downloads."""
    from fs.riders import is_sampling_launch
    (a, _), (b, _) = _sim(), _sim()
    mask, dx = np.asarray(a._solver._bc.mask), a._solver.dx
    assert BOX[2] <= mask.shape[0] and BOX[3] <= mask.shape[1]
    a.start_spectra(BOX, every=every, start_step=start, window="hann", detrend=True)
    a.run(steps // 2)
    a.run(steps - steps // 2)
    ref = S.State(BOX, _tabs(BOX, "hann"), True, every, start)
    want = []
    for n in range(steps):
        b.step()
        ref.launch(b.field_to_numpy()["v"], mask)
        if is_sampling_launch(n, every, start):
            want.append(n + 1)
    out = a.spectra()
    assert set(out) == {"power", "energy", "kx", "ky", "k", "E", "samples", "sample_steps", "box", "window", "detrend", "sums"}
    assert out["samples"] == ref.samples == len(want) and out["sample_steps"].tolist() == want
    assert np.array_equal(out["sums"], ref.power) and out["sums"].shape == (32, 16) and out["sums"].max() > 0
    assert (out["box"], out["window"], out["detrend"]) == (BOX, "hann", True)
    from fs import spectra
    assert np.array_equal(out["power"], 0.5 * (ref.power + spectra.mirrored(ref.power)) / len(want))
    kx, ky = spectra.wavenumbers(32, 16, dx)
    assert np.array_equal(out["kx"], kx) and np.array_equal(out["ky"], ky)
    fa, fb = a.field_to_numpy(), b.field_to_numpy()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa), "the spectrum changed the trajectory"
    # the one-shot calls on the same state
    for window, detrend in (("hann", True), ("boxcar", False)):
        re, im = S.plane(fb["v"], mask, BOX, _tabs(BOX, window), detrend)
        Z = a.box_fft(BOX, window=window, detrend=detrend)
        assert Z.dtype == np.complex128 and np.array_equal(Z.real, re) and np.array_equal(Z.imag, im)
        sp = a.spectrum(BOX, window=window, detrend=detrend)
        assert np.array_equal(sp["sums"], S.power_of(re, im)) and sp["samples"] == 1 and sp["sample_steps"].tolist() == [0]
    assert a.spectra()["samples"] == len(want), "the one-shot calls touched the attached rider"


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_spectra(BOX)
    sim.start_distributions({"quantity": "speed", "bins": 50, "range": (0.0, 2.0)})
    sim.start_pod(3)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["pod_launch", "dist_launch", "spec_launch", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4 and [t[0] for t in sig[-4:]] == ["pod", "dist", "spec", "loads"]
    sp = sim._spectrar
    assert sp.token == ("spec", sp.spec.serial) and sig[-2] == sp.token
    assert not sp.replaces_attached and sp.stop_in_capture and not sp.keeps_last
    assert sp.room() is None and sp.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)
    assert [type(r).__name__ for r in sim._riders()] == ["Pod", "Distributions", "Spectra", "Tracker"]


def test_start_reset_stop_checkpoint_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    X, Y = np.asarray(sim._solver._bc.mask).shape
    for call in (sim.spectra, sim.reset_spectra):
        with pytest.raises(RuntimeError):
            call()
    for bad in ((0, 0, 12, 8), (0, 0, 24, 8), (0, 0, 4, 8), (0, 0, 8, 4), (0, 0, 8192, 8), (X - 4, 0, X + 4, 8), (0, Y - 4, 8, Y + 4), (-8, 0, 0, 8),
                (8, 0, 0, 8), (0, 0, 8), None):
        for call in (sim.start_spectra, sim.spectrum, sim.box_fft):
            with pytest.raises(ValueError):
                call(bad)
    for bad in (dict(every=0), dict(start_step=-1), dict(window="kaiser")):
        with pytest.raises(ValueError):
            sim.start_spectra(BOX, **bad)
    assert sim._spectrar is None
    sim.start_spectra(BOX, every=2, start_step=1, window="boxcar", detrend=False)
    with pytest.raises(RuntimeError, match="attached"):
        sim.start_spectra(BOX)                               # a second attach without stop_spectra()
    sim.run(9)                                               # steps 3, 5, 7, 9 sampled
    out = sim.spectra()
    assert out["samples"] == 4 and out["sample_steps"].tolist() == [3, 5, 7, 9] and out["window"] == "boxcar" and out["detrend"] is False
    z = {k: np.array(v) for k, v in sim._spectrar.checkpoint().items()}
    assert set(z) == {"spec.power", "spec.launches", "spec.samples", "spec.base", "spec.box", "spec.window", "spec.detrend", "spec.every", "spec.start"}
    assert (int(z["spec.launches"]), int(z["spec.samples"])) == (9, 4) and z["spec.power"].shape == (32, 16)
    assert sim._spectrar.held(z) == (BOX, "boxcar", False, 2, 1) and sim._spectrar.held({}) is None
    sim.reset_spectra()
    zero = sim.spectra()
    assert zero["sums"].max() == 0 and zero["samples"] == 0 and not zero["power"].any()
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim.spectra()["sample_steps"].tolist() == [11, 13]
    # the round trip into a freshly attached spectrum; another box, window, detrend or cadence is refused before any device work
    tok = sim._spectrar.token
    sim.stop_spectra()
    assert sim._spectrar is None and tok not in sim._signature()
    sim.stop_spectra()                                       # (a second stop is a no-op)
    same = dict(every=2, start_step=1, window="boxcar", detrend=False)
    for box, kw, msg in (((3, 1, 35, 17), same, "box"), ((2, 1, 18, 17), same, "box"), (BOX, dict(same, window="hann"), "window"),
                         (BOX, dict(same, detrend=True), "detrend"), (BOX, dict(same, every=3), "every"), (BOX, dict(same, start_step=2), "every")):
        sim.start_spectra(box, **kw)
        st = sim._spectrar.spec._h
        with pytest.raises(ValueError, match=msg):
            sim._spectrar.restore(z)
        assert st.power.max() == 0 and st.launches == 0
        sim.stop_spectra()
    sim.start_spectra(BOX, **same)
    assert sim._spectrar.restore(z) == sim.spectra()["samples"] == 4
    back = sim.spectra()
    assert np.array_equal(out["sums"], back["sums"]) and out["sample_steps"].tolist() == back["sample_steps"].tolist()
    assert np.array_equal(out["E"], back["E"])
    # a slab context: refused with a message
    dev = sim._dev
    saved = dev.nranks
    dev.nranks = 2
    try:
        sim.stop_spectra()
        for call in (lambda: sim.start_spectra(BOX), lambda: sim.spectrum(BOX), lambda: sim.box_fft(BOX)):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
