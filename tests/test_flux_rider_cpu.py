"""The host logic of the scale-to-scale fluxes without a GPU: FluidSimulator.start_scale_fluxes / scale_fluxes / reset_scale_fluxes /
stop_scale_fluxes / scale_flux / filtered_fields on the NumPy stand-in device (tests/flux_standin.py): the rider alone and beside the two
spectra riders, launch and token order, the cadence, the reset, the checkpoint round trip and every refusal of restore, the refusals of bad
boxes and half-widths."""
import numpy as np
import pytest

import flux_ref as FR

FNAME = "traj_bc3_upwind_vc0.npz"            # a 64 x 32 grid
BOX = (3, 2, 60, 29)
HW = (1, 3, 9)
SBOX = (2, 1, 34, 17)                        # the spectra's (powers of two)


@pytest.fixture(scope="module")
def standin():
    import fs
    from flux_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from flux_standin import make_sim
    return make_sim(FNAME)


@pytest.mark.parametrize("every,start,steps", [(1, 0, 5), (2, 3, 16)])
def test_planes_follow_the_steps_alone_and_beside_the_spectra(every, start, steps, standin):
    """a: the fluxes alone; b: beside start_spectra and start_cross_spectra; c: those two alone; d: the twin whose downloads feed the
    restatement."""
    from fs.riders import is_sampling_launch, samples_after
    (a, _), (b, _), (c, _), (d, _) = _sim(), _sim(), _sim(), _sim()
    mask, dx = np.asarray(a._solver._bc.mask), a._solver.dx
    assert mask.shape == (64, 32)
    a.start_scale_fluxes(BOX, HW, every=every, start_step=start)
    b.start_scale_fluxes(BOX, HW, every=every, start_step=start)
    for sim in (b, c):
        sim.start_spectra(SBOX, every=every, start_step=start)
        sim.start_cross_spectra(SBOX, ("vorticity", "p"), every=every, start_step=start)
    for sim in (a, b, c):
        sim.run(steps // 2)
        sim.run(steps - steps // 2)
    ref = FR.State(BOX, HW, dx, every, start)
    want = []
    for n in range(steps):
        d.step()
        ref.launch(d.field_to_numpy()["v"], mask)
        if is_sampling_launch(n, every, start):
            want.append(n + 1)
    out, beside = a.scale_fluxes(), b.scale_fluxes()
    assert out["samples"] == ref.samples == len(want) == samples_after(steps, every, start) and out["sample_steps"].tolist() == want
    assert out["sums"].shape == (3, 3, 57, 27) and np.array_equal(out["sums"], ref.sums)
    assert all(np.abs(out["sums"][k]).max() > 0 for k in range(3))
    assert out["half_widths"] == HW and out["box"] == BOX and np.array_equal(out["widths"], np.array([3 * dx, 7 * dx, 19 * dx]))
    assert out["valid"] == [FR.valid_rect(mask.shape, r, BOX) for r in HW] == [(3, 2, 60, 29), (4, 4, 60, 28), (10, 10, 54, 22)]
    assert np.array_equal(out["pi"], ref.sums[:, 0] / ref.samples) and np.array_equal(out["k"], ref.sums[:, 2] / ref.samples)
    assert np.array_equal(beside["sums"], out["sums"])
    assert np.array_equal(b.spectra()["sums"], c.spectra()["sums"]) and np.array_equal(b.cross_spectra()["sums"], c.cross_spectra()["sums"])
    fa, fd = a.field_to_numpy(), d.field_to_numpy()
    assert all(np.array_equal(fa[k], fd[k]) for k in fa), "the rider changed the trajectory"
    # the one-shot calls on the same state
    Fs, fl = FR.sample(fd["v"], mask, dx, HW)
    x = a.scale_flux(BOX, HW)
    assert np.array_equal(x["sums"], fl[:, :, BOX[0]:BOX[2], BOX[1]:BOX[3]]) and x["samples"] == 1 and x["sample_steps"].tolist() == [0]
    for F, r in zip(Fs, HW):
        got = a.filtered_fields(BOX, r)
        assert set(got) == set(FR.NAMES) | {"defined"} and got["defined"] == (max(3, r), max(2, r), min(60, 64 - r), min(29, 32 - r))
        for k, name in enumerate(FR.NAMES):
            assert np.array_equal(got[name], F[k, BOX[0]:BOX[2], BOX[1]:BOX[3]]), (r, name)
    assert a.scale_fluxes()["samples"] == len(want), "the one-shot calls touched the attached rider"


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_scale_fluxes(BOX, HW)
    sim.start_cross_spectra(SBOX, ("q", "swirl"))
    sim.start_spectra(SBOX)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["spec_launch", "xspec_launch", "flux_launch", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4 and [t[0] for t in sig[-4:]] == ["spec", "xspec", "flux", "loads"]
    fx = sim._fluxr
    assert fx.token == ("flux", fx.flux.serial) and sig[-2] == fx.token
    assert not fx.replaces_attached and fx.stop_in_capture and not fx.keeps_last
    assert fx.room() is None and fx.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)
    assert [type(r).__name__ for r in sim._riders()] == ["Spectra", "CrossSpectra", "ScaleFluxes", "Tracker"]
    sim.stop_scale_fluxes()
    assert sim._fluxr is None and fx.token not in sim._signature() and len(sim._signature()) == len(base) + 3
    assert [type(r).__name__ for r in sim._riders()] == ["Spectra", "CrossSpectra", "Tracker"]


def test_start_reset_stop_checkpoint_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    X, Y = np.asarray(sim._solver._bc.mask).shape
    for call in (sim.scale_fluxes, sim.reset_scale_fluxes):
        with pytest.raises(RuntimeError):
            call()
    calls = (sim.start_scale_fluxes, sim.scale_flux)
    for bad in ((0, 0, 0, 8), (5, 0, 4, 8), (X - 4, 0, X + 4, 8), (0, Y - 4, 8, Y + 4), (-8, 0, 8, 8), (0, 0, 8), None):
        for call in calls:
            with pytest.raises(ValueError, match="box"):
                call(bad, (1,))
        with pytest.raises(ValueError, match="box"):
            sim.filtered_fields(bad, 1)
    for bad, msg in (((0,), "1 .. 64"), ((65,), "1 .. 64"), ((1, 65), "1 .. 64"), ((-1,), "1 .. 64"), ((1.5,), "integer"), (("a",), "integer"),
                     ((2, 2), "increasing"), ((3, 1), "increasing"), ((), "1 .. 8"), (tuple(range(1, 10)), "1 .. 8"), (None, "sequence")):
        for call in calls:
            with pytest.raises(ValueError, match=msg):
                call(BOX, bad)
    for r in (0, 65, 2.5):
        with pytest.raises(ValueError, match="1 .. 64|integer"):
            sim.filtered_fields(BOX, r)
    # no valid cell inside the box: the grid is 64 x 32, so r = 14 leaves the rows j = 15 and 16, r = 15 none; a box beside the valid rectangle
    for box, hw in ((BOX, (15,)), (BOX, (1, 20)), ((0, 0, 64, 15), (14,)), ((0, 0, 2, 32), (1,)), ((62, 0, 64, 32), (1,))):
        for call in calls:
            with pytest.raises(ValueError, match="no valid cell"):
                call(box, hw)
    assert sim.scale_flux((0, 0, 64, 32), (14,))["valid"] == [(15, 15, 49, 17)]
    for bad in (dict(every=0), dict(start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_scale_fluxes(BOX, HW, **bad)
    assert sim._fluxr is None
    same = dict(half_widths=HW, every=2, start_step=1)
    sim.start_scale_fluxes(BOX, **same)
    with pytest.raises(RuntimeError, match="attached"):
        sim.start_scale_fluxes(BOX, HW)                      # a second attach without stop_scale_fluxes()
    sim.run(9)                                               # steps 3, 5, 7, 9 sampled
    out = sim.scale_fluxes()
    assert out["samples"] == 4 and out["sample_steps"].tolist() == [3, 5, 7, 9]
    z = {k: np.array(v) for k, v in sim._fluxr.checkpoint().items()}
    assert set(z) == {"flux.sums", "flux.launches", "flux.samples", "flux.base", "flux.box", "flux.half_widths", "flux.every", "flux.start"}
    assert (int(z["flux.launches"]), int(z["flux.samples"])) == (9, 4) and z["flux.sums"].shape == (3, 3, 57, 27)
    assert sim._fluxr.held(z) == (BOX, HW, 2, 1) and sim._fluxr.held({}) is None
    sim.reset_scale_fluxes()
    zero = sim.scale_fluxes()
    assert not zero["sums"].any() and zero["samples"] == 0 and not zero["pi"].any()
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim.scale_fluxes()["sample_steps"].tolist() == [11, 13]
    # the round trip into a freshly attached rider; another box, half-widths or cadence is refused before any device work
    tok = sim._fluxr.token
    sim.stop_scale_fluxes()
    assert sim._fluxr is None and tok not in sim._signature()
    sim.stop_scale_fluxes()                                  # (a second stop is a no-op)
    for box, kw, msg in (((4, 2, 61, 29), same, "box"), ((3, 2, 59, 29), same, "box"), (BOX, dict(same, half_widths=(1, 3)), "half_widths"),
                         (BOX, dict(same, half_widths=(1, 3, 8)), "half_widths"), (BOX, dict(same, every=3), "every"),
                         (BOX, dict(same, start_step=2), "every")):
        sim.start_scale_fluxes(box, **kw)
        st = sim._fluxr.flux._h
        with pytest.raises(ValueError, match=msg):
            sim._fluxr.restore(z)
        assert not st.sums.any() and st.launches == 0
        sim.stop_scale_fluxes()
    sim.start_scale_fluxes(BOX, **same)
    st = sim._fluxr.flux._h
    for bad, msg in (({}, "holds no"), (dict(z, **{"flux.sums": z["flux.sums"][:1]}), "shape"), (dict(z, **{"flux.samples": np.array(10)}), "counters")):
        with pytest.raises(ValueError, match=msg):
            sim._fluxr.restore(bad)
        assert not st.sums.any() and st.launches == 0
    assert sim._fluxr.restore(z) == sim.scale_fluxes()["samples"] == 4
    back = sim.scale_fluxes()
    assert np.array_equal(out["sums"], back["sums"]) and out["sample_steps"].tolist() == back["sample_steps"].tolist()
    assert np.array_equal(out["mean_pi"], back["mean_pi"]) and np.array_equal(out["mean_own"]["zf"], back["mean_own"]["zf"])
    # the checkpoint of the simulator carries the keys of every attached rider
    sim.start_spectra(SBOX)
    keys = set()
    for r in sim._riders():
        keys |= set(r.checkpoint())
    assert {"spec.power", "flux.sums"} <= keys
    # a slab context: refused with a message
    dev = sim._dev
    saved = dev.nranks
    dev.nranks = 2
    try:
        sim.stop_scale_fluxes()
        for call in (lambda: sim.start_scale_fluxes(BOX, HW), lambda: sim.scale_flux(BOX, HW), lambda: sim.filtered_fields(BOX, 1)):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
