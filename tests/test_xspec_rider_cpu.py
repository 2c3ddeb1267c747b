"""The host logic of the cross-spectra without a GPU: FluidSimulator.start_cross_spectra / cross_spectra / reset_cross_spectra /
stop_cross_spectra / cross_spectrum / pair_fft on the NumPy stand-in device (tests/xspec_standin.py): the rider alone and beside
start_spectra, launch and token order, the cadence, the reset, the checkpoint round trip and every refusal of restore, the refusals of bad
boxes and pairs."""
import numpy as np
import pytest

import xspec_ref as XR

FNAME = "traj_bc3_upwind_vc0.npz"
BOX = (2, 1, 34, 17)
Q = {name: k for k, name in enumerate(XR.QUANTITIES)}


@pytest.fixture(scope="module")
def standin():
    import fs
    from xspec_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from xspec_standin import make_sim
    return make_sim(FNAME)


def _tabs(box, window):
    from fs import spectra
    return spectra.tables(box[2] - box[0], box[3] - box[1], window)


@pytest.mark.parametrize("pair,every,start,steps", [(("vorticity", "p"), 1, 0, 5), (("speed", None), 2, 3, 16)])
def test_planes_follow_the_steps_alone_and_beside_the_energy_spectrum(pair, every, start, steps, standin):
    """a: the cross-spectrum alone; b: beside start_spectra; c: start_spectra alone; d: the twin whose downloads feed the restatement."""
    from fs.riders import is_sampling_launch
    (a, _), (b, _), (c, _), (d, _) = _sim(), _sim(), _sim(), _sim()
    mask, dx = np.asarray(a._solver._bc.mask), a._solver.dx
    a.start_cross_spectra(BOX, pair, every=every, start_step=start, window="hann", detrend=True)
    b.start_spectra(BOX, every=every, start_step=start)
    b.start_cross_spectra(BOX, pair, every=every, start_step=start, window="hann", detrend=True)
    c.start_spectra(BOX, every=every, start_step=start)
    for sim in (a, b, c):
        sim.run(steps // 2)
        sim.run(steps - steps // 2)
    qa, qb = Q[pair[0]], (-1 if pair[1] is None else Q[pair[1]])
    ref = XR.State(BOX, qa, qb, dx, _tabs(BOX, "hann"), True, every, start)
    want = []
    for n in range(steps):
        d.step()
        f = d.field_to_numpy()
        ref.launch(f["v"], f["p"], mask)
        if is_sampling_launch(n, every, start):
            want.append(n + 1)
    out, beside = a.cross_spectra(), b.cross_spectra()
    assert out["quantities"] == pair and out["samples"] == ref.samples == len(want) and out["sample_steps"].tolist() == want
    assert out["sums"].shape == ((4 if qb >= 0 else 1), 32, 16) and np.array_equal(out["sums"], ref.sums) and out["sums"][0].max() > 0
    assert (out["box"], out["window"], out["detrend"]) == (BOX, "hann", True)
    assert np.array_equal(beside["sums"], out["sums"]) and np.array_equal(b.spectra()["sums"], c.spectra()["sums"])
    fa, fd = a.field_to_numpy(), d.field_to_numpy()
    assert all(np.array_equal(fa[k], fd[k]) for k in fa), "the cross-spectrum changed the trajectory"
    # the one-shot calls on the same state
    for window, detrend in (("hann", True), ("boxcar", False)):
        re, im = XR.plane(qa, qb, fd["v"], fd["p"], mask, dx, BOX, _tabs(BOX, window), detrend)
        Z = a.pair_fft(BOX, pair, window=window, detrend=detrend)
        assert Z.dtype == np.complex128 and np.array_equal(Z.real, re) and np.array_equal(Z.imag, im)
        x = a.cross_spectrum(BOX, pair, window=window, detrend=detrend)
        assert np.array_equal(x["sums"], XR.accumulate(np.zeros_like(ref.sums), re, im)) and x["samples"] == 1 and x["sample_steps"].tolist() == [0]
    assert a.cross_spectra()["samples"] == len(want), "the one-shot calls touched the attached rider"
    if qb < 0:
        assert not Z.imag[0, 0] and out["spectrum_b"] is None
    # the pair (u, w) is the packed plane of the energy spectrum
    Zuw, Zbox = a.pair_fft(BOX, ("u", "w"), detrend=True), a.box_fft(BOX, detrend=True)
    assert np.array_equal(Zuw.real, Zbox.real) and np.array_equal(Zuw.imag, Zbox.imag)


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_cross_spectra(BOX, ("q", "swirl"))
    sim.start_spectra(BOX)
    sim.start_distributions({"quantity": "speed", "bins": 50, "range": (0.0, 2.0)})
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["dist_launch", "spec_launch", "xspec_launch", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4 and [t[0] for t in sig[-4:]] == ["dist", "spec", "xspec", "loads"]
    xs = sim._xspectrar
    assert xs.token == ("xspec", xs.xspec.serial) and sig[-2] == xs.token
    assert not xs.replaces_attached and xs.stop_in_capture and not xs.keeps_last
    assert xs.room() is None and xs.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)
    assert [type(r).__name__ for r in sim._riders()] == ["Distributions", "Spectra", "CrossSpectra", "Tracker"]


def test_start_reset_stop_checkpoint_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    X, Y = np.asarray(sim._solver._bc.mask).shape
    for call in (sim.cross_spectra, sim.reset_cross_spectra):
        with pytest.raises(RuntimeError):
            call()
    for bad in ((0, 0, 12, 8), (0, 0, 4, 8), (0, 0, 8192, 8), (X - 4, 0, X + 4, 8), (0, Y - 4, 8, Y + 4), (-8, 0, 0, 8), (0, 0, 8), None):
        for call in (sim.start_cross_spectra, sim.cross_spectrum, sim.pair_fft):
            with pytest.raises(ValueError, match="box|sides"):
                call(bad)
    for bad in (("u", "dye"), ("vort", "p"), (None, "u"), ("u",), ("u", "w", "p"), 3, ("u", 1)):
        for call in (sim.start_cross_spectra, sim.cross_spectrum, sim.pair_fft):
            with pytest.raises(ValueError, match="quantity|pair"):
                call(BOX, bad)
    for bad in (dict(every=0), dict(start_step=-1), dict(window="kaiser")):
        with pytest.raises(ValueError):
            sim.start_cross_spectra(BOX, **bad)
    assert sim._xspectrar is None
    same = dict(pair=("vorticity", "u"), every=2, start_step=1, window="boxcar", detrend=False)
    sim.start_cross_spectra(BOX, **same)
    with pytest.raises(RuntimeError, match="attached"):
        sim.start_cross_spectra(BOX)                         # a second attach without stop_cross_spectra()
    sim.run(9)                                               # steps 3, 5, 7, 9 sampled
    out = sim.cross_spectra()
    assert out["samples"] == 4 and out["sample_steps"].tolist() == [3, 5, 7, 9] and out["window"] == "boxcar" and out["detrend"] is False
    z = {k: np.array(v) for k, v in sim._xspectrar.checkpoint().items()}
    assert set(z) == {"xspec.sums", "xspec.launches", "xspec.samples", "xspec.base", "xspec.box", "xspec.quantities", "xspec.window",
                      "xspec.detrend", "xspec.every", "xspec.start"}
    assert (int(z["xspec.launches"]), int(z["xspec.samples"])) == (9, 4) and z["xspec.sums"].shape == (4, 32, 16)
    assert z["xspec.quantities"].tolist() == [4, 0]
    assert sim._xspectrar.held(z) == (BOX, ("vorticity", "u"), "boxcar", False, 2, 1) and sim._xspectrar.held({}) is None
    sim.reset_cross_spectra()
    zero = sim.cross_spectra()
    assert not zero["sums"].any() and zero["samples"] == 0 and not zero["spectrum_a"].any()
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim.cross_spectra()["sample_steps"].tolist() == [11, 13]
    # the round trip into a freshly attached rider; another box, pair, window, detrend or cadence is refused before any device work
    tok = sim._xspectrar.token
    sim.stop_cross_spectra()
    assert sim._xspectrar is None and tok not in sim._signature()
    sim.stop_cross_spectra()                                 # (a second stop is a no-op)
    for box, kw, msg in (((3, 1, 35, 17), same, "box"), ((2, 1, 18, 17), same, "box"), (BOX, dict(same, pair=("vorticity", "w")), "pair"),
                         (BOX, dict(same, pair=("u", "vorticity")), "pair"), (BOX, dict(same, pair=("vorticity", None)), "pair"),
                         (BOX, dict(same, window="hann"), "window"), (BOX, dict(same, detrend=True), "detrend"),
                         (BOX, dict(same, every=3), "every"), (BOX, dict(same, start_step=2), "every")):
        sim.start_cross_spectra(box, **kw)
        st = sim._xspectrar.xspec._h
        with pytest.raises(ValueError, match=msg):
            sim._xspectrar.restore(z)
        assert not st.sums.any() and st.launches == 0
        sim.stop_cross_spectra()
    sim.start_cross_spectra(BOX, **same)
    st = sim._xspectrar.xspec._h
    for bad, msg in (({}, "holds no"), (dict(z, **{"xspec.quantities": np.array([4, 9])}), "quantities"),
                     (dict(z, **{"xspec.sums": z["xspec.sums"][:1]}), "shape"), (dict(z, **{"xspec.samples": np.array(10)}), "counters")):
        with pytest.raises(ValueError, match=msg):
            sim._xspectrar.restore(bad)
        assert not st.sums.any() and st.launches == 0
    assert sim._xspectrar.restore(z) == sim.cross_spectra()["samples"] == 4
    back = sim.cross_spectra()
    assert np.array_equal(out["sums"], back["sums"]) and out["sample_steps"].tolist() == back["sample_steps"].tolist()
    assert np.array_equal(out["Co"], back["Co"]) and np.array_equal(out["coherence"], back["coherence"], equal_nan=True)
    # the checkpoint of the simulator carries both spectra riders' keys
    sim.start_spectra(BOX)
    keys = set()
    for r in sim._riders():
        keys |= set(r.checkpoint())
    assert {"spec.power", "xspec.sums"} <= keys
    # a slab context: refused with a message
    dev = sim._dev
    saved = dev.nranks
    dev.nranks = 2
    try:
        sim.stop_cross_spectra()
        for call in (lambda: sim.start_cross_spectra(BOX), lambda: sim.cross_spectrum(BOX), lambda: sim.pair_fft(BOX)):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
