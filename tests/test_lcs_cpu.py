"""Flow maps and FTLE without a GPU: the host functions of fs/lcs.py (the order in which a full, wrapped or partly filled ring is walked, the
window, the FTLE's edge values), the analytic cases of tests/test_gpu_lcs.py on the NumPy restatement itself (tests/lcs_ref.py) - so that a
wrong expectation shows here and not as a device failure - and FluidSimulator.flow_map / ftle / ftle_fields with their refusals on the NumPy
stand-in device (tests/lcs_standin.py).

Bounds: the uniform, time-linear flow is integrated exactly (equality); the steady strain gives lam = g^(2N) within 1e-10 relative (set by the
issue that introduced the feature: bilinear interpolation reproduces a linear field, what remains is N <= 64 steps of a few eps each)."""
import numpy as np
import pytest
from lcs_cases import (DT, DX, LATTICE_CASES, LATTICE_DT, LATTICE_DX, LATTICE_RINGS, LATTICE_SUBSTEPS, install_ring, lattice_geometry, lattice_rings,
                       make_sim, missing_neighbours, strain_expectation, strain_rings, uniform_rings)
from lcs_ref import ALIVE, LEFT, UNSEEDED, WALL_HIT, assert_state_equal, chronological, fate_rings, flow_map_ref


# ---- fs/lcs.py -----------------------------------------------------------------------------------------------------------------------------
def test_intervals_walk_the_ring_chronologically():
    from fs.lcs import intervals, window
    assert intervals(4, 4, direction="forward") == [(0, 1), (1, 2), (2, 3)]                     # full, not wrapped
    assert intervals(4, 4) == intervals(4, 4, direction="backward") == [(3, 2), (2, 1), (1, 0)]
    assert intervals(7, 4, direction="forward") == [(3, 0), (0, 1), (1, 2)]                     # wrapped: sample 3 .. 6 in slots 3, 0, 1, 2
    assert intervals(7, 4, direction="backward") == [(2, 1), (1, 0), (0, 3)]
    assert intervals(3, 8, direction="forward") == [(0, 1), (1, 2)]                             # partly filled
    assert intervals(7, 4, 1, -1, "forward") == [(0, 1), (1, 2)] and intervals(7, 4, 1, -1, "backward") == [(2, 1), (1, 0)]
    assert intervals(7, 4, None, -2, "forward") == [(3, 0), (0, 1)] and intervals(7, 4, -2, None, "backward") == [(2, 1)]
    assert window(7, 4) == (0, 3) and window(3, 8, 1, None) == (1, 2) and window(9, 4, -3, -1) == (1, 3)
    # every ring state against a plain loop over the samples the ring has seen
    for M in (2, 3, 5):
        for samples in range(2, 3 * M + 1):
            order = chronological(samples, M)
            assert intervals(samples, M, direction="forward") == list(zip(order[:-1], order[1:])), (samples, M)
            assert intervals(samples, M, direction="backward") == list(zip(order[::-1][:-1], order[::-1][1:])), (samples, M)
    with pytest.raises(ValueError):
        intervals(4, 4, direction="sideways")
    for first, last in ((2, 2), (3, 1), (-1, 0)):
        with pytest.raises(ValueError):
            intervals(4, 4, first, last)
    for first, last in ((4, None), (None, -5), (0, 4)):
        with pytest.raises(IndexError):
            intervals(4, 4, first, last)
    for samples in (0, 1):
        with pytest.raises(RuntimeError):
            intervals(samples, 4)


def test_ftle_edge_values_and_ridges():
    from fs.lcs import ftle, ridges, step_size
    lam = np.array([[np.nan, 0.0], [1.0, np.exp(2.0)]])
    for span in (0.5, -0.5):
        f = ftle(lam, span)
        assert np.isnan(f[0, 0]) and f[0, 1] == -np.inf and f[1, 0] == 0.0 and abs(f[1, 1] - 2.0) <= 4e-16
    r = ridges(np.array([np.nan, -np.inf, 1.0, 7.9, 8.1, 10.0]))
    assert r.tolist() == [False, False, False, False, True, True] and r.dtype == bool
    assert ridges(np.array([1.0, 4.0, 10.0]), fraction=0.3).tolist() == [False, True, True]
    assert not ridges(np.full((2, 2), np.nan)).any()
    assert step_size(2, DT, DX, 4, "forward") == 0.25 and step_size(2, DT, DX, 4, "backward") == -0.25


# ---- the analytic cases, on the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [1, 2])
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_every_fate_occurs_in_the_fate_scene(direction, substeps, refine):
    mask, slots = fate_rings()
    st = flow_map_ref(slots, 4, mask, 1, 0.5, 0.25, direction, refine, None, substeps)          # h = 2 / substeps cells per unit velocity
    assert st["x"].shape == (33 * refine, 16 * refine) and st["x"].size in (528, 2112)
    assert set(np.unique(st["status"])) == {ALIVE, LEFT, WALL_HIT, UNSEEDED}
    assert np.isnan(st["lam"][st["status"] == UNSEEDED]).all() and np.isfinite(st["lam"][st["status"] != UNSEEDED]).sum() > 100
    assert np.isfinite(st["x"]).all() and np.isfinite(st["y"]).all(), "a node kept a position formed from the NaN cell"


@pytest.mark.parametrize("substeps", [1, 2, 4])
def test_time_linear_uniform_flow_is_integrated_exactly(substeps):
    mask, slots = uniform_rings()
    for direction, sign in (("forward", 1.0), ("backward", -1.0)):
        st = flow_map_ref(slots, 5, mask, 1, DT, DX, direction, 1, None, substeps)
        x0 = np.arange(64)[:, None] + 0.5
        stay = st["status"] == ALIVE
        # h_total c sum_m (m + (m + 1)) / 2 = 0.5 * 0.25 * 8 = 1 cell
        assert stay.sum() == 63 * 16 and np.all((st["x"] - x0)[stay] == sign * 1.0) and np.all(st["y"] == np.arange(16) + 0.5)
        assert np.all(st["status"][~stay] == LEFT) and np.all(st["lam"][2:-2] == 1.0)
    st = flow_map_ref(slots, 5, mask, 1, DT, DX, "forward", 1, None, substeps, first=2, last=-1)          # snapshots 2 .. 4
    assert np.all((st["x"] - (np.arange(64)[:, None] + 0.5))[st["status"] == ALIVE] == 0.5 * 0.25 * 6)


@pytest.mark.parametrize("substeps,refine", [(1, 1), (4, 2), (16, 1)])
def test_steady_strain_stretches_by_the_analytic_factor(substeps, refine):
    from fs.lcs import start_positions
    a = 0.1
    mask, slots = strain_rings(a=a)
    for direction in ("forward", "backward"):
        st = flow_map_ref(slots, 5, mask, 1, DT, DX, direction, refine, None, substeps)
        st["x0"], st["y0"] = start_positions((0, 0, 64, 32), refine)
        N = substeps * 4
        inner, lam, _ = strain_expectation(st, 64, 32, a, 0.5 / substeps, N)
        assert inner.sum() > 100 * refine * refine and np.all(st["status"][inner] == ALIVE)
        err = np.abs(st["lam"][inner] / lam - 1.0).max()
        print(f"{direction} S={substeps} r={refine}: {inner.sum()} nodes, max |lam / g^2N - 1| = {err:.3g}")
        assert err <= 1e-10


# ---- host logic on the NumPy stand-in --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    import fs
    from lcs_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


KEYS = {"x", "y", "x0", "y0", "status", "lam", "ftle", "span", "sample_steps", "direction", "refine", "box"}


def test_flow_map_on_an_installed_ring_equals_the_restatement(standin):
    from fs.lcs import ftle
    mask, slots = fate_rings()
    sim = make_sim(mask, dt=0.5 * 0.25, dx=0.25)
    install_ring(sim, slots, every=2, samples=6)          # wrapped: samples 2 .. 5 sit in slots 2, 3, 0, 1
    ring = sim._dev.pod_get(sim._podr.pod)[0]
    for kw in (dict(), dict(direction="forward", substeps=3), dict(refine=2, first=1, last=-1), dict(direction="forward", box=(2, 1, 30, 15), refine=4)):
        m = sim.flow_map(**kw)
        assert set(m) == KEYS
        exp = flow_map_ref(ring, 6, mask, 2, 0.125, 0.25, **kw)
        assert_state_equal(m, exp, f"{kw}: ")
        steps = [8, 10, 12] if "first" in kw else [6, 8, 10, 12]
        assert m["span"] == (len(steps) - 1) * 2 * 0.125 and m["sample_steps"].tolist() == steps
        assert np.array_equal(m["ftle"], ftle(exp["lam"], m["span"]), equal_nan=True) and m["direction"] == kw.get("direction", "backward")
        assert m["x0"].shape == m["x"].shape and np.array_equal(m["x0"][m["status"] == UNSEEDED], m["x"][m["status"] == UNSEEDED])
        assert np.array_equal(sim.ftle(**kw), m["ftle"], equal_nan=True)
    assert sim.flow_map(first=1, last=-1)["sample_steps"].tolist() == [8, 10, 12]
    assert type(sim._dev).live_flowmaps == 0, "flow_map left a device lattice behind"
    assert np.array_equal(sim._dev.pod_get(sim._podr.pod)[0], ring, equal_nan=True), "the flow map changed the ring"
    # as fields: p the cast FTLE with the non-finite values as 0, v the displacement
    v, p = sim.ftle_fields(direction="forward", substeps=2)
    m = sim.flow_map(direction="forward", substeps=2)
    assert np.array_equal(p.to_numpy(), np.where(np.isfinite(m["ftle"]), m["ftle"], 0.0).astype(np.float32))
    assert np.array_equal(v.to_numpy(), np.stack([m["x"] - m["x0"], m["y"] - m["y0"]], -1).astype(np.float32)) and np.abs(v.to_numpy()).max() > 0
    sim.stop_pod()


def test_refusals_change_nothing(standin):
    from fs import _lib
    mask, slots = fate_rings()
    sim = make_sim(mask)
    for call in (sim.flow_map, sim.ftle, sim.ftle_fields):
        with pytest.raises(RuntimeError):
            call()                                             # no POD attached
    sim.start_pod(4)
    with pytest.raises(RuntimeError):
        sim.flow_map()                                         # no sample
    install = sim._dev.pod_set
    install(sim._podr.pod, slots, 1, 1)
    with pytest.raises(RuntimeError):
        sim.flow_map()                                         # one sample
    install(sim._podr.pod, slots, 4, 4)
    before = sim._dev.pod_get(sim._podr.pod)
    for bad in (dict(refine=3), dict(refine=0), dict(refine=16), dict(substeps=0), dict(substeps=17), dict(box=(0, 0, 34, 16)), dict(box=(5, 5, 5, 9)),
                dict(box=(-1, 0, 4, 4)), dict(box=(0, 0, 4)), dict(direction="up"), dict(first=2, last=1), dict(first=3)):
        with pytest.raises(ValueError):
            sim.flow_map(**bad)
    for bad in (dict(first=4), dict(last=-5)):
        with pytest.raises(IndexError):
            sim.flow_map(**bad)
    dev = sim._dev
    dev.capturing = True
    try:
        for call in (sim.flow_map, sim.ftle, sim.ftle_fields):
            with pytest.raises(_lib.FsError):
                call()
    finally:
        dev.capturing = False
    saved = dev.nranks
    dev.nranks = 2
    try:
        with pytest.raises(_lib.FsError, match="single-GPU"):
            sim.flow_map()
    finally:
        dev.nranks = saved
    after = dev.pod_get(sim._podr.pod)
    assert np.array_equal(before[0], after[0], equal_nan=True) and before[1:] == after[1:] and type(dev).live_flowmaps == 0
    # the device calls check their own arguments
    fm = dev.flowmap_create(None, 1)
    for args in ((0, 0, 0.5, 1), (0, 4, 0.5, 1), (-1, 0, 0.5, 1), (0, 1, 0.0, 1), (0, 1, np.inf, 1), (0, 1, np.nan, 1), (0, 1, 0.5, 0), (0, 1, 0.5, 17)):
        with pytest.raises(ValueError):
            dev.flowmap_advance(fm, sim._podr.pod, *args)
    dev.flowmap_advance(fm, sim._podr.pod, 0, 1, 0.5, 2)
    moved = dev.flowmap_get(fm)
    dev.flowmap_reset(fm)
    fresh = dev.flowmap_get(fm)
    assert not np.array_equal(moved[0], fresh[0]) and np.isnan(fresh[3]).all() and set(np.unique(fresh[2])) == {ALIVE, UNSEEDED}
    dev.flowmap_free(fm)
    assert fm._h is None and type(dev).live_flowmaps == 0
    assert sim.flow_map()["x"].shape == (33, 16)               # a second call works, and stop_pod after it
    sim.stop_pod()
    assert sim._podr is None


# ---- the boxed, refined lattices of tests/test_gpu_lcs.py: what each case must contain to reach what it is meant to reach ---------------------------
@pytest.mark.parametrize("substeps", LATTICE_SUBSTEPS)
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("ring", sorted(LATTICE_RINGS))
@pytest.mark.parametrize("box,refine", LATTICE_CASES)
def test_boxed_lattice_cases_reach_every_branch(box, refine, ring, direction, substeps, standin):
    from fs.lcs import start_positions
    mask, slots = lattice_rings()
    assert mask.shape == (70, 40) and -(-70 // 64) * 64 == 128          # two 64-column pitch units
    nx, ny, groups, last = lattice_geometry(box, refine)
    assert (nx * ny, groups, last) == {8: (45120, 177, 64), 4: (36960, 145, 96)}[refine]
    assert box[0] > 0 and box[1] > 0 and box[2] < 70 and box[3] < 40     # no lattice edge is a domain edge
    sim = make_sim(mask, dt=LATTICE_DT, dx=LATTICE_DX)
    state = LATTICE_RINGS[ring]
    install_ring(sim, slots, samples=state["samples"])
    m = sim.flow_map(direction, refine, box, substeps, **state["window"])          # (the stand-in IS the restatement: tested above, with a box)
    assert m["x"].shape == (nx, ny) and m["box"] == box and m["refine"] == refine
    x0, y0 = start_positions(box, refine)
    assert np.array_equal(m["x0"], x0) and np.array_equal(m["y0"], y0) and x0[0, 0] == box[0] + 0.5 / refine and y0[0, 0] == box[1] + 0.5 / refine
    assert m["sample_steps"].tolist() == ([1, 2, 3, 4] if ring == "full" else [4, 5, 6])
    fates = set(np.unique(m["status"]).tolist())
    if ring == "full":
        assert fates == {ALIVE, LEFT, WALL_HIT, UNSEEDED}
    else:
        assert {ALIVE, WALL_HIT, UNSEEDED} <= fates          # (the inner box loses LEFT forwards: two intervals do not reach the outflow)
    # UNSEEDED is the wall block seen through the box offset and the refinement
    block = np.repeat(np.repeat(mask[box[0]:box[2], box[1]:box[3]] == 1, refine, 0), refine, 1)
    assert np.array_equal(m["status"] == UNSEEDED, block) and block.sum() == 6 * 8 * refine * refine
    alive = m["status"] == ALIVE
    assert np.abs(m["x"] - m["x0"])[alive].min() > 0 and np.abs(m["y"] - m["y0"])[alive].max() > 1.0, "the nodes hardly moved"
    # all four quadrants of a cell: the four bilinear weights all vary
    fx, fy = m["x"][alive] - np.floor(m["x"][alive]), m["y"][alive] - np.floor(m["y"][alive])
    for lo_x in (True, False):
        for lo_y in (True, False):
            assert (((fx < 0.5) == lo_x) & ((fy < 0.5) == lo_y)).sum() > 1000
    # one-sided differences on all four sides, at lattice edges that are not domain edges and around the block
    finite = np.isfinite(m["lam"])
    assert finite.sum() > 30000 and not finite[m["status"] == UNSEEDED].any()
    beside = {"lower a": box[0] < 30, "upper a": box[2] > 36, "lower b": box[3] > 20, "upper b": box[1] < 12}      # fluid on that side of the block
    for side, absent in zip(("lower a", "upper a", "lower b", "upper b"), missing_neighbours(m["status"])):
        assert (absent & finite).sum() >= (ny if "a" in side else nx) // 2, side          # the lattice edge, which is not the domain's
        inner = absent & finite
        inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
        assert inner.sum() >= 6 * refine or not beside[side], f"{side}: no one-sided difference beside the block"
    assert sum(beside.values()) >= 3
    sim.stop_pod()
