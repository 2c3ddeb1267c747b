"""The host logic of the kinetic-energy budget without a GPU: FluidSimulator.start_budget / budget / reset_budget / stop_budget /
budget_sample on the NumPy stand-in device (tests/budget_standin.py): the rider alone and beside the averager and the scale fluxes, launch
and token order, the cadence, the reset, the checkpoint round trip and every refusal of restore, the refusals of bad boxes, of a second
start_budget, of calls during a capture and of slabs."""
import numpy as np
import pytest

import budget_ref as BR

FNAME = "traj_bc3_upwind_vc0.npz"            # a 64 x 32 grid
BOX = (3, 2, 60, 29)
HW = (1, 3)


@pytest.fixture(scope="module")
def standin():
    import fs
    from budget_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from budget_standin import make_sim
    return make_sim(FNAME)


@pytest.mark.parametrize("every,start,steps", [(1, 0, 5), (2, 3, 16)])
def test_planes_follow_the_steps_alone_and_beside_the_averager_and_the_fluxes(every, start, steps, standin):
    """a: the budget alone; b: beside start_averaging and start_scale_fluxes; c: those two alone; d: the twin whose downloads feed the
    restatement."""
    from fs.budgets import PLANES
    from fs.riders import is_sampling_launch, samples_after
    (a, _), (b, _), (c, _), (d, _) = _sim(), _sim(), _sim(), _sim()
    mask, dx = np.asarray(a._solver._bc.mask), a._solver.dx
    assert mask.shape == (64, 32)
    a.start_budget(BOX, every=every, start_step=start)
    b.start_budget(BOX, every=every, start_step=start)
    for sim in (b, c):
        sim.start_averaging(every=every, start_step=start)
        sim.start_scale_fluxes(BOX, HW, every=every, start_step=start)
    for sim in (a, b, c):
        sim.run(steps // 2)
        sim.run(steps - steps // 2)
    ref = BR.State(BOX, dx, every, start)
    want = []
    for n in range(steps):
        d.step()
        f = d.field_to_numpy()
        ref.launch(f["v"], f["p"], mask)
        if is_sampling_launch(n, every, start):
            want.append(n + 1)
    out, beside = a.budget(), b.budget()
    assert out["samples"] == ref.samples == len(want) == samples_after(steps, every, start) and out["sample_steps"].tolist() == want
    assert out["sums"].shape == (21, 57, 27) and np.array_equal(out["sums"], ref.sums)
    fluid = mask[BOX[0]:BOX[2], BOX[1]:BOX[3]] == 0
    assert np.array_equal(out["fluid"], fluid) and fluid.sum() == 1411 and out["valid"].sum() == 1019
    for k, name in enumerate(PLANES):
        assert np.abs(out["sums"][k]).max() > 0 and not out["sums"][k][~fluid].any(), name
    assert out["box"] == BOX and out["dx"] == dx and out["re"] == a._solver.re
    assert np.array_equal(beside["sums"], out["sums"]) and np.array_equal(beside["residual"], out["residual"])
    # planes 0 - 5 are the averager's sums on the fluid cells of the box
    sums_of = lambda sim: sim._dev.mean_read(sim._averager.mean)[0]
    avg = sums_of(b)[:, BOX[0]:BOX[2], BOX[1]:BOX[3]]
    for k in range(6):
        assert np.array_equal(out["sums"][k][fluid], avg[k][fluid]), k
    assert np.array_equal(sums_of(b), sums_of(c)) and np.array_equal(b.scale_fluxes()["sums"], c.scale_fluxes()["sums"])
    fa, fd = a.field_to_numpy(), d.field_to_numpy()
    assert all(np.array_equal(fa[k], fd[k]) for k in fa), "the rider changed the trajectory"
    # the one-shot call on the same state
    x = a.budget_sample(BOX)
    one = BR.State(BOX, dx, 1, 0)
    one.launch(fd["v"], fd["p"], mask)
    assert np.array_equal(x["sums"], one.sums) and x["samples"] == 1 and x["sample_steps"].tolist() == [0]
    whole = a.budget_sample()
    assert whole["box"] == (0, 0, 64, 32) and np.array_equal(whole["sums"][:, BOX[0]:BOX[2], BOX[1]:BOX[3]], one.sums)
    assert a.budget()["samples"] == len(want), "the one-shot call touched the attached rider"


def test_every_plane_is_non_zero_on_the_golden_snapshots(standin):
    """On the golden file's own snapshots (steps 1, 2, 5, 10 added up): 1411 selected cells, and every plane is far from empty - the
    smallest maximum magnitude is S_www's 0.23998, so no plane passes a comparison by being all zeros.  (This runs the restatement alone:
    it proves the fixture that the other tests compare on, not the feature.)"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FNAME))
    sim, _ = _sim()
    mask, dx = np.asarray(sim._solver._bc.mask), sim._solver.dx
    st = BR.State(BOX, dx, 1, 0)
    for n in g["snaps"]:
        st.launch(np.asarray(g[f"step{int(n)}.v"]), np.asarray(g[f"step{int(n)}.p"]), mask)
    assert st.samples == len(g["snaps"]) >= 1
    assert (st.sums[0] != 0).sum() == 1411
    tops = [float(np.abs(st.sums[k]).max()) for k in range(BR.NPLANE)]
    assert min(tops) > 0.2399 and int(np.argmin(tops)) == 11, tops


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_budget(BOX)
    sim.start_scale_fluxes(BOX, HW)
    sim.start_averaging()
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["mean_accumulate", "flux_launch", "budget_launch", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4 and [t[0] for t in sig[-4:]] == ["mean", "flux", "budget", "loads"]
    bg = sim._budgetr
    assert bg.token == ("budget", bg.budget.serial) and sig[-2] == bg.token
    assert not bg.replaces_attached and bg.stop_in_capture and not bg.keeps_last
    assert bg.room() is None and bg.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)
    assert [type(r).__name__ for r in sim._riders()] == ["Averager", "ScaleFluxes", "Budget", "Tracker"]
    sim.stop_budget()
    assert sim._budgetr is None and bg.token not in sim._signature() and len(sim._signature()) == len(base) + 3
    assert [type(r).__name__ for r in sim._riders()] == ["Averager", "ScaleFluxes", "Tracker"]
    sim.stop_body()
    sim.start_budget()
    assert [t[0] for t in sim._signature()[-3:]] == ["mean", "flux", "budget"]


def test_start_reset_stop_checkpoint_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    mask = np.asarray(sim._solver._bc.mask)
    X, Y = mask.shape
    for call in (sim.budget, sim.reset_budget):
        with pytest.raises(RuntimeError):
            call()
    for bad in ((0, 0, 0, 8), (5, 0, 4, 8), (X - 4, 0, X + 4, 8), (0, Y - 4, 8, Y + 4), (-8, 0, 8, 8), (0, 0, 8), 5):
        for call in (sim.start_budget, sim.budget_sample):
            with pytest.raises(ValueError, match="box"):
                call(bad)
    solid = np.argwhere(mask != 0)
    assert len(solid)
    i, j = (int(x) for x in solid[0])
    for call in (sim.start_budget, sim.budget_sample):
        with pytest.raises(ValueError, match="no fluid cell"):
            call((i, j, i + 1, j + 1))
    for bad in (dict(every=0), dict(start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_budget(BOX, **bad)
    assert sim._budgetr is None
    same = dict(every=2, start_step=1)
    sim.start_budget(BOX, **same)
    with pytest.raises(RuntimeError, match="attached"):
        sim.start_budget(BOX)                                # a second attach without stop_budget()
    sim.run(9)                                               # steps 3, 5, 7, 9 sampled
    out = sim.budget()
    assert out["samples"] == 4 and out["sample_steps"].tolist() == [3, 5, 7, 9]
    # during a capture: every call but stop_budget is refused
    dev = sim._dev
    dev.capturing = True
    try:
        for call in (sim.budget, sim.reset_budget, sim.budget_sample, lambda: sim.start_budget(BOX)):
            with pytest.raises(RuntimeError, match="capture"):
                call()
        for call in (lambda: dev.budget_read(sim._budgetr.budget), lambda: dev.budget_get(sim._budgetr.budget), lambda: dev.budget_reset(sim._budgetr.budget),
                     lambda: dev.budget_set(sim._budgetr.budget, out["sums"], 9, 4), lambda: dev.budget_create(BOX, 1.0)):
            with pytest.raises(_lib.FsError, match="capture"):
                call()
    finally:
        dev.capturing = False
    z = {k: np.array(v) for k, v in sim._budgetr.checkpoint().items()}
    assert set(z) == {"budget.sums", "budget.launches", "budget.samples", "budget.base", "budget.box", "budget.every", "budget.start"}
    assert (int(z["budget.launches"]), int(z["budget.samples"])) == (9, 4) and z["budget.sums"].shape == (21, 57, 27)
    assert sim._budgetr.held(z) == (BOX, 2, 1) and sim._budgetr.held({}) is None
    sim.reset_budget()
    zero = sim.budget()
    assert not zero["sums"].any() and zero["samples"] == 0 and not zero["production"].any()
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim.budget()["sample_steps"].tolist() == [11, 13]
    # the round trip into a freshly attached rider; another box or cadence is refused before any device work
    tok = sim._budgetr.token
    sim.stop_budget()
    assert sim._budgetr is None and tok not in sim._signature()
    sim.stop_budget()                                        # (a second stop is a no-op)
    for box, kw, msg in (((4, 2, 61, 29), same, "box"), ((3, 2, 59, 29), same, "box"), (BOX, dict(same, every=3), "every"),
                         (BOX, dict(same, start_step=2), "every")):
        sim.start_budget(box, **kw)
        st = sim._budgetr.budget._h
        with pytest.raises(ValueError, match=msg):
            sim._budgetr.restore(z)
        assert not st.sums.any() and st.launches == 0
        sim.stop_budget()
    sim.start_budget(BOX, **same)
    st = sim._budgetr.budget._h
    for bad, msg in (({}, "holds no"), (dict(z, **{"budget.sums": z["budget.sums"][:1]}), "shape"), (dict(z, **{"budget.samples": np.array(10)}), "counters")):
        with pytest.raises(ValueError, match=msg):
            sim._budgetr.restore(bad)
        assert not st.sums.any() and st.launches == 0
    assert sim._budgetr.restore(z) == sim.budget()["samples"] == 4
    back = sim.budget()
    assert np.array_equal(out["sums"], back["sums"]) and out["sample_steps"].tolist() == back["sample_steps"].tolist()
    assert np.array_equal(out["residual"], back["residual"]) and out["totals"] == back["totals"]
    # the checkpoint of the simulator carries the keys of every attached rider
    sim.start_averaging()
    keys = set()
    for r in sim._riders():
        keys |= set(r.checkpoint())
    assert "budget.sums" in keys and len(keys) > 7
    # a slab context: refused with a message
    saved = dev.nranks
    dev.nranks = 2
    try:
        sim.stop_budget()
        for call in (lambda: sim.start_budget(BOX), lambda: sim.budget_sample(BOX)):
            with pytest.raises(_lib.FsError, match="single-GPU"):
                call()
    finally:
        dev.nranks = saved
