"""The host logic of the field distributions without a GPU: FluidSimulator.start_distributions / distributions / reset_distributions /
stop_distributions / histogram / quantile / order_statistics on the NumPy stand-in device (tests/dist_standin.py): launch and token order
beside the other riders, the cadence, the reset, the checkpoint round trip and its refusals, run() not cut by the rider."""
import numpy as np
import pytest

import dist_ref as D

FNAME = "traj_bc3_upwind_vc0.npz"
CHANNELS = [{"quantity": "speed", "bins": 50, "range": (0.0, 2.0)},
            {"quantity": "u", "bins": 16, "range": (-1.0, 2.0), "box": (2, 1, 30, 20), "against": {"quantity": "vorticity", "bins": 32, "range": (-30.0, 30.0)}}]


@pytest.fixture(scope="module")
def standin():
    import fs
    from dist_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from dist_standin import make_sim
    return make_sim(FNAME)


def _sampled(n, every, start):
    return [k for k in range(1, n + 1) if k > start and (k - start) % every == 0]


def _want(b, mask, dx):
    d = b.field_to_numpy()
    v, p = d["v"].copy(), d["p"].copy()
    return [D.field_histogram("speed", v, p, mask, dx, 50, (0.0, 2.0)),
            D.field_joint("u", "vorticity", v, p, mask, dx, (-1.0, 2.0, 16), (-30.0, 30.0, 32), (2, 1, 30, 20))]


@pytest.mark.parametrize("every,start,steps", [(1, 0, 5), (2, 3, 36)])
def test_tables_follow_the_steps(every, start, steps, standin):
    """run() in two chunks (graphs are not captured on the stand-in; the chunks are not cut) against the restatement on a twin's downloads."""
    (a, _), (b, _) = _sim(), _sim()
    mask, dx = np.asarray(a._solver._bc.mask), a._solver.dx
    a.start_distributions(CHANNELS, every=every, start_step=start)
    a.run(steps // 2)
    a.run(steps - steps // 2)
    want = _sampled(steps, every, start)
    sums = None
    for n in range(1, steps + 1):
        b.step()
        if n in want:
            w = _want(b, mask, dx)
            sums = w if sums is None else [{k: s[k] + x[k] for k in s} for s, x in zip(sums, w)]
    out = a.distributions()
    assert len(out) == 2 and out[0]["quantity"] == "speed" and out[1]["quantity"] == ("u", "vorticity")
    assert set(out[0]) == {"counts", "below", "above", "nan", "edges", "samples", "sample_steps", "quantity", "box"}
    assert set(out[1]) == {"counts", "outside", "nan", "edges", "edges_b", "samples", "sample_steps", "quantity", "box"}
    assert out[0]["counts"].shape == (50,) and out[1]["counts"].shape == (16, 32) and out[1]["box"] == (2, 1, 30, 20)
    for o, s in zip(out, sums):
        assert o["samples"] == len(want) and o["sample_steps"].tolist() == want
        for k in s:
            assert np.array_equal(o[k], s[k]), k
    assert out[0]["counts"].sum() > 0 and out[1]["counts"].sum() > 0
    fa, fb = a.field_to_numpy(), b.field_to_numpy()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa), "the distributions changed the trajectory"
    # the one-shot calls on the same state
    h = a.histogram("speed", 50, (0.0, 2.0))
    last = _want(b, mask, dx)
    assert np.array_equal(h["counts"], last[0]["counts"]) and h["samples"] == 1 and h["sample_steps"].tolist() == [0]
    s, _ = D.sorted_values("speed", fb["v"], fb["p"], mask, dx)
    assert a.quantile("speed", 0.9, method="lower") == np.quantile(s, 0.9, method="lower")
    assert np.array_equal(a.quantile("speed", [0.0, 0.5, 1.0], method="higher"), np.quantile(s, [0.0, 0.5, 1.0], method="higher"))
    o = a.order_statistics("speed", [0, len(s) - 1])
    assert o["n"] == len(s) and o["nan"] == 0 and o["values"].tolist() == [s[0], s[-1]]
    auto = a.histogram("speed", 7)
    assert auto["edges"][0] == s[0] and auto["edges"][-1] == np.nextafter(s[-1], np.inf) and auto["counts"].sum() == len(s)
    with pytest.raises(ValueError, match="rank"):
        a.order_statistics("speed", [len(s)])


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_vortices(1.0)
    sim.track_body(box, every=2, capacity=10)
    sim.start_distributions(CHANNELS[0])
    sim.start_pod(3)
    sim.start_averaging(every=3)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["mean_accumulate", "pod_launch", "dist_launch", "loads_record", "vortex_launch"]
    assert names[-5:] == riding and not set(names[:-5]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 5
    assert [t[0] for t in sig[-5:]] == ["mean", "pod", "dist", "loads", "vortices"]
    di = sim._distr
    assert di.token == ("dist", di.dist.serial) and sig[-3] == di.token
    assert not di.replaces_attached and di.stop_in_capture and not di.keeps_last
    assert di.room() is None and di.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)


def test_start_reset_stop_checkpoint_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    for call in (sim.distributions, sim.reset_distributions):
        with pytest.raises(RuntimeError):
            call()
    ok = CHANNELS[0]
    for bad in ([], [ok] * 5, dict(ok, bins=0), dict(ok, bins=4097), dict(ok, quantity="k"), dict(ok, range=(1, 1)), dict(ok, range=None),
                dict(ok, against={"quantity": "w", "bins": 100, "range": (0, 1)})):
        with pytest.raises(ValueError):
            sim.start_distributions(bad)
    for bad in (dict(every=0), dict(start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_distributions(ok, **bad)
    assert sim._distr is None
    sim.start_distributions(CHANNELS, every=2, start_step=1)
    with pytest.raises(RuntimeError):
        sim.start_distributions(ok)                          # a second attach without stop_distributions()
    sim.run(9)                                               # steps 3, 5, 7, 9 sampled
    out = sim.distributions()
    assert out[0]["samples"] == 4 and out[1]["sample_steps"].tolist() == [3, 5, 7, 9]
    z = {k: np.array(v) for k, v in sim._distr.checkpoint().items()}
    assert set(z) == {"dist.tables", "dist.launches", "dist.samples", "dist.base", "dist.channels", "dist.every", "dist.start"}
    assert (int(z["dist.launches"]), int(z["dist.samples"])) == (9, 4) and len(z["dist.tables"]) == 50 + 4 + 16 * 32 + 4
    sim.reset_distributions()
    zero = sim.distributions()
    assert zero[0]["counts"].sum() == 0 and zero[0]["samples"] == 0 and zero[1]["outside"] == 0
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim.distributions()[0]["sample_steps"].tolist() == [11, 13]
    # the round trip into freshly attached distributions; other channels, every or start_step are refused before any device work
    tok = sim._distr.token
    sim.stop_distributions()
    assert sim._distr is None and tok not in sim._signature()
    sim.stop_distributions()                                 # (a second stop is a no-op)
    for chans, kw, msg in ((CHANNELS[:1], dict(every=2, start_step=1), "channels"), (CHANNELS[::-1], dict(every=2, start_step=1), "channels"),
                           ([CHANNELS[0], dict(CHANNELS[1], box=(2, 1, 30, 19))], dict(every=2, start_step=1), "channels"),
                           (CHANNELS, dict(every=3, start_step=1), "every"), (CHANNELS, dict(every=2, start_step=2), "every")):
        sim.start_distributions(chans, **kw)
        before = np.concatenate(sim._distr.dist._h.tables).copy()
        with pytest.raises(ValueError, match=msg):
            sim._distr.restore(z)
        assert np.array_equal(np.concatenate(sim._distr.dist._h.tables), before) and sim._distr.dist._h.launches == 0
        sim.stop_distributions()
    sim.start_distributions(CHANNELS, every=2, start_step=1)
    assert sim._distr.restore(z) == sim.distributions()[0]["samples"] == 4          # (-> the samples taken over: the CLI's "samples so far")
    back = sim.distributions()
    for o, b in zip(out, back):
        assert np.array_equal(o["counts"], b["counts"]) and o["samples"] == b["samples"] and o["sample_steps"].tolist() == b["sample_steps"].tolist()
    # a slab context: refused with a message
    dev = sim._dev
    saved = dev.nranks
    dev.nranks = 2
    try:
        sim.stop_distributions()
        for call in (lambda: sim.start_distributions(ok), lambda: sim.histogram("u", 4, (0, 1)), lambda: sim.quantile("u", 0.5)):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
