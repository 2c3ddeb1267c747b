"""Riders of the step attached at once.

The first test: the history recorder, time averages, body tracker, tracer particles and their accumulated occupancy - a run() on replayed
graphs, cut into chunks by the two rings and the sort schedule, gathers bit for bit what eager steps gather, and after the stop_* calls no
cached graph holds a rider's launch.

The second, in f32 and f64: all the kinds - twelve since the scale fluxes and the budget joined; the test names still say ten -
(tests/rider_cases.py: history, averages, modes, POD with the FTLE over its snapshots, distributions, spectra, cross-spectra, scale fluxes
with their filtered planes, the kinetic-energy budget, body tracker, inertial tracers with deposits and accumulated occupancy, vortex tracker) at pairwise
different cadences, the run cut by three rings and the sort schedule.  Every reader returns on replayed graphs what it returns after eager
steps and what the simulator that carries that kind alone returns; the mean, the modes, the distributions and both spectra of eager steps
equal their NumPy restatements on per-step downloads; the trajectory is that of the simulator without a rider; every cached signature holds
every rider's token in the documented order; after the stop_* calls none does.  == everywhere.

The third: the same ten with larger rings, so that a chunk behind the first is long enough for run() to give the cached period its long
form there (_run_chunk(reuse=True)); graphs against eager steps."""
import numpy as np
import pytest

import rider_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


RIDER_TOKENS = ("history", "mean", "loads", "tracer", "tracer_accum")


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}[{k}]"


def _rider_signatures(sim):
    return [sig for sig in sim._graphs if any(isinstance(t, tuple) and t and t[0] in RIDER_TOKENS for t in sig)]


def test_all_riders_on_graphs_equal_eager_steps(hip_lib):
    import fs
    from fs.boundary_condition import default_body_box
    from fs.tracers import seed_line
    res = 64
    dt, dx, re = 0.05 / res, 1.0 / res, 1e6
    box = default_body_box(3, res)
    fs.runtime.init(gpu=0, dtype="f32")
    sims = [fs.FluidSimulator.create(3, res, dt, dx, re, 5.0, "cip") for _ in range(2)]
    try:
        for sim in sims:
            sim.record_history([(5, 30)], box, every=1, capacity=20)
            sim.start_averaging(every=3)
            sim.track_body(box, every=2, capacity=10)
            sim.seed_tracers(seed_line((4.5, 2.5), (4.5, 61.5), 256), sort_every=32)
            sim.accumulate_tracers(every=3)
        graph, eager = sims
        graph.run(100)
        eager.run(100, graph=False)
        assert len(graph._graphs) >= 1 and len(_rider_signatures(graph)) == len(graph._graphs)
        assert len(eager._graphs) == 0
        _same(graph.field_to_numpy(), eager.field_to_numpy(), "fields")
        h = graph.history()
        assert h["step"].tolist() == list(range(1, 101)) and np.abs(h["force_x"]).max() > 0.0
        _same(h, eager.history(), "history")
        a = graph.averages()
        assert a["samples"] == 33 and np.abs(a["u"]).max() > 0.0
        _same(a, eager.averages(), "averages")
        b = graph.body_loads()
        assert b["step"].tolist() == list(range(2, 101, 2))
        _same(b, eager.body_loads(), "body_loads")
        assert np.array_equal(graph.body_surface()["sums"], eager.body_surface()["sums"])
        t = graph.tracers()
        assert t["steps"] == 100 and graph._tracers.sorts == 3
        _same(t, eager.tracers(), "tracers")
        acc = graph.tracer_accumulation()
        assert acc["samples"] == 33 and acc["occupancy"].sum() > 0
        _same(acc, eager.tracer_accumulation(), "tracer_accumulation")
        graph.stop_history()
        graph.stop_body()
        graph.stop_averaging()
        graph.stop_tracers()
        assert _rider_signatures(graph) == []
        graph.run(20)
        eager.run(20, graph=False)
        _same(graph.field_to_numpy(), eager.field_to_numpy(), "fields after the stop_* calls")
        _same(graph.history(), h, "history kept after stop_history")
    finally:
        for sim in sims:
            sim._solver._bc.device.close()


# ---- all ten kinds ---------------------------------------------------------------------------------------------------------------------------
def _bare_fields(dtype):
    """The fields of the scene without a rider after STEPS and after STEPS + MORE steps of run()."""
    bare = RC.make(dtype)
    try:
        bare.run(RC.STEPS)
        at_stops = bare.field_to_numpy()
        bare.run(RC.MORE)
        return at_stops, bare.field_to_numpy()
    finally:
        RC.close(bare)


def _alone(dtype):
    """{kind: its readers} of one fresh simulator per kind of rider, with only that kind attached, under run(STEPS)."""
    out = {}
    for kind in RC.KINDS:
        sim = RC.attach(RC.make(dtype), (kind,))
        try:
            assert len(sim._riders()) == 1
            sim.run(RC.STEPS)
            assert sim._graphs, f"{kind} alone: the run replayed no graph"
            out[kind] = RC.read(sim, kind)
        finally:
            RC.close(sim)
    return out


class _Restatements:
    """The NumPy side of the downloading simulator: the mean, the modes, the distributions and both spectra, fed one download per step."""

    def __init__(self, sim):
        import dist_ref as D
        import mean_ref
        import modes_ref
        import spec_ref
        import xspec_ref
        from fs import spectra
        from fs.modes import phasor_steps
        self.D, self.mean_ref, self.modes_ref = D, mean_ref, modes_ref
        self.mask = np.array(sim._solver._bc.mask)
        self.dx = sim._solver.dx
        self.step = 0
        self.mean = mean_ref.new_sums(self.mask.shape)
        self.modes = modes_ref.State(self.mask.shape, *phasor_steps(RC.frequencies(), RC.MODES["every"], sim._solver.dt))
        nx, ny = RC.SPEC_BOX[2] - RC.SPEC_BOX[0], RC.SPEC_BOX[3] - RC.SPEC_BOX[1]
        tabs = spectra.tables(nx, ny, "hann")
        self.spec = spec_ref.State(RC.SPEC_BOX, tabs, True, RC.SPEC["every"], RC.SPEC["start_step"])
        qa, qb = (xspec_ref.QUANTITIES.index(q) for q in RC.XSPEC_PAIR)
        self.xspec = xspec_ref.State(RC.SPEC_BOX, qa, qb, self.dx, tabs, True, RC.XSPEC["every"], RC.XSPEC["start_step"])
        one, two = RC.CHANNELS
        self.hist = {"counts": np.zeros(one["bins"], np.int64), "below": 0, "above": 0, "nan": 0}
        self.joint = {"counts": np.zeros((two["bins"], two["against"]["bins"]), np.int64), "outside": 0, "nan": 0}

    def launch(self, v, p):
        D, mask, dx = self.D, self.mask, self.dx
        self.step += 1
        if self.step in RC.samples(**RC.MEAN):
            self.mean_ref.accumulate_ref(self.mean, v, p, mask)
        self.modes_ref.launch_ref(self.modes, v, p, mask, RC.MODES["every"], RC.MODES["start_step"])
        if self.step in RC.samples(**RC.DIST):
            one, two = RC.CHANNELS
            b = two["against"]
            for acc, new in ((self.hist, D.field_histogram(one["quantity"], v, p, mask, dx, one["bins"], one["range"])),
                             (self.joint, D.field_joint(two["quantity"], b["quantity"], v, p, mask, dx, two["range"] + (two["bins"],),
                                                        b["range"] + (b["bins"],), box=two["box"]))):
                for k in acc:
                    acc[k] = acc[k] + new[k]
        self.spec.launch(v, mask)
        self.xspec.launch(v, p, mask)

    def assert_equal(self, sim):
        dev = sim._dev
        sums, launches, n = dev.mean_read(sim._averager.mean)
        assert (launches, n) == (RC.STEPS, len(RC.samples(**RC.MEAN))) and np.array_equal(sums, self.mean), "the mean differs from its restatement"
        sums, scalars, launches, n = dev.modes_read(sim._moder.modes)
        st = self.modes
        assert (launches, n) == (st.launches, st.samples) == (RC.STEPS, len(RC.samples(**RC.MODES)))
        assert np.array_equal(scalars, st.scalars()) and np.array_equal(sums, st.sums), "the modes differ from their restatement"
        got = sim.distributions()
        for g, want in zip(got, (self.hist, self.joint)):
            assert g["samples"] == len(RC.samples(**RC.DIST)) and g["sample_steps"].tolist() == RC.samples(**RC.DIST)
            assert g["counts"].dtype == np.int64 and np.array_equal(g["counts"], want["counts"]), "the distributions differ from their restatement"
            for k in ("below", "above", "outside", "nan"):
                if k in want:
                    assert g[k] == want[k], k
        got = sim.spectra()
        assert got["samples"] == self.spec.samples == len(RC.samples(**RC.SPEC)) and got["sample_steps"].tolist() == RC.samples(**RC.SPEC)
        assert np.array_equal(got["sums"], self.spec.power), "the spectrum differs from its restatement"
        Z = dev.spec_plane(sim._spectrar.spec)
        assert np.array_equal(Z.real, self.spec.re) and np.array_equal(Z.imag, self.spec.im)
        got = sim.cross_spectra()
        assert got["samples"] == self.xspec.samples == len(RC.samples(**RC.XSPEC)) and got["sample_steps"].tolist() == RC.samples(**RC.XSPEC)
        assert np.array_equal(got["sums"], self.xspec.sums), "the cross-spectrum differs from its restatement"
        Z = dev.xspec_plane(sim._xspectrar.xspec)
        assert np.array_equal(Z.real, self.xspec.re) and np.array_equal(Z.imag, self.xspec.im)


def _assert_not_empty(r, mask):
    """Each rider took its samples and holds something: guards against a pass that compares nothing."""
    h = r["history"]["history"]
    assert h["step"].tolist() == RC.samples(**RC.HISTORY) and np.abs(h["force_x"]).max() > 0 and np.abs(h["u"]).max() > 0
    a = r["mean"]["averages"]
    assert a["samples"] == len(RC.samples(**RC.MEAN)) and np.abs(a["u"]).max() > 0
    m = r["modes"]["modes"]
    assert m["samples"] == len(RC.samples(**RC.MODES)) and m["u"]["amplitude"].max() > 0 and np.abs(r["modes"]["mode_fields"]["v"]).max() > 0
    p = r["pod"]["pod"]
    assert p["samples"] == len(RC.samples(**RC.POD)) and p["sample_steps"].tolist() == RC.samples(**RC.POD)[-RC.POD["snapshots"]:]
    assert p["energies"][0] > 0 and np.isfinite(r["pod"]["ftle"]).any() and np.nanmax(np.abs(r["pod"]["ftle"])) > 0
    assert all(np.abs(r["pod"][f"pod_snapshot({k})"]["v"]).max() > 0 for k in range(RC.POD["snapshots"]))
    d = r["dist"]["distributions"]
    assert d[0]["samples"] == len(RC.samples(**RC.DIST)) and d[0]["counts"].sum() > 0 and d[1]["counts"].sum() > 0
    s = r["spec"]["spectra"]
    assert s["samples"] == len(RC.samples(**RC.SPEC)) and s["sums"].max() > 0 and np.abs(r["spec"]["plane"]).max() > 0
    x = r["xspec"]["cross_spectra"]
    assert x["samples"] == len(RC.samples(**RC.XSPEC)) and all(np.abs(x["sums"][k]).max() > 0 for k in range(4))
    assert np.abs(r["xspec"]["plane"]).max() > 0
    f = r["flux"]["scale_fluxes"]
    assert f["samples"] == len(RC.samples(**RC.FLUX)) and f["sample_steps"].tolist() == RC.samples(**RC.FLUX)
    assert all(np.abs(f["sums"][k, n]).max() > 0 for k in range(len(RC.FLUX_WIDTHS)) for n in range(3))
    assert all(np.abs(r["flux"]["filtered"][w]).max() > 0 for w in RC.FLUX_WIDTHS)
    g = r["budget"]["budget"]
    assert g["samples"] == len(RC.samples(**RC.BUDGET)) == 14 and g["sample_steps"].tolist() == RC.samples(**RC.BUDGET)
    fluid = mask[RC.SPEC_BOX[0]:RC.SPEC_BOX[2], RC.SPEC_BOX[1]:RC.SPEC_BOX[3]] == 0
    assert fluid.any() and not fluid.all() and np.array_equal(g["fluid"], fluid)
    assert g["sums"].shape == (21,) + fluid.shape
    for n in range(21):
        assert g["sums"][n][fluid].any() and not g["sums"][n][~fluid].any(), f"budget plane {n}"
    b = r["loads"]["body_loads"]
    assert b["step"].tolist() == RC.samples(**RC.LOADS) and np.abs(b["pressure_x"]).max() > 0 and np.abs(b["viscous_x"]).max() > 0
    assert np.abs(r["loads"]["body_surface.sums"]).max() > 0
    t = r["tracers"]
    assert t["tracers"]["steps"] == RC.STEPS and (t["tracers"]["x"] != t["tracers"]["seeds"][:, 0]).any() and np.abs(t["tracers"]["u"]).max() > 0
    assert t["tracer_fields"]["count"].sum() > 0 and t["tracer_deposits"].shape == mask.shape
    assert t["tracer_accumulation"]["samples"] == len(RC.samples(**RC.TRACER_ACCUM)) and t["tracer_accumulation"]["occupancy"].sum() > 0
    v = r["vortices"]["vortices"]
    assert v["step"].tolist() == RC.samples(**RC.VORTICES) and v["count"].sum() > 0 and (r["vortices"]["vortex_labels"]["flags"] != 0).any()
    box = RC.SPEC_BOX
    assert (mask[box[0]:box[2], box[1]:box[3]] == 1).any(), "the box of the spectra holds no body cell"


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_all_ten_kinds_on_graphs_equal_eager_steps_each_alone_and_the_restatements(dtype, hip_lib):
    at_stops, at_end = _bare_fields(dtype)
    alone = _alone(dtype)
    sims = [RC.attach(RC.make(dtype)) for _ in range(3)]
    graph, eager, ref = sims
    try:
        mask = np.array(graph._solver._bc.mask)
        # the launch order and the tokens, before anything runs
        assert [type(r).__name__ for r in graph._riders()] == RC.RIDER_ORDER
        assert all(len(r.tokens()) >= 1 for r in graph._riders())
        tokens = [t for r in graph._riders() for t in r.tokens()]
        assert [t[0] for t in tokens] == RC.TOKEN_KINDS and RC.rider_tokens(graph._signature()) == tokens
        graph.run(RC.STEPS)
        eager.run(RC.STEPS, graph=False)
        # the rings were drained inside run() (no reader has drained them yet), the sort schedule was kept, graphs were replayed
        for r, cfg, total in ((graph._recorder, RC.HISTORY, RC.samples(**RC.HISTORY)), (graph._tracker, RC.LOADS, RC.samples(**RC.LOADS)),
                              (graph._vortexr, RC.VORTICES, RC.samples(**RC.VORTICES))):
            assert cfg["capacity"] <= r.drained <= len(total) and len(total) > cfg["capacity"], type(r).__name__
            assert r.issued == RC.STEPS, type(r).__name__
        assert graph._tracers.sorts == eager._tracers.sorts == RC.STEPS // RC.SORT_EVERY == 3 and graph._tracers.issued == RC.STEPS
        assert len(graph._graphs) >= 1 and len(eager._graphs) == 0
        for sig in graph._graphs:
            assert RC.rider_tokens(sig) == tokens, "a cached signature without the token of every rider, in the order of the launches"
        got = {kind: RC.read(graph, kind) for kind in RC.KINDS}
        _assert_not_empty(got, mask)
        for kind in RC.KINDS:
            RC.same(got[kind], RC.read(eager, kind), f"graph against eager: {kind}")
            RC.same(got[kind], alone[kind], f"beside the others against alone: {kind}")
        # eager steps with a download after each, against the restatements
        rest = _Restatements(ref)
        for _ in range(RC.STEPS):
            ref.step()
            d = ref.field_to_numpy()
            rest.launch(d["v"], d["p"])
        rest.assert_equal(ref)
        for kind in ("mean", "modes", "dist", "spec", "xspec"):
            RC.same(RC.read(ref, kind), got[kind], f"downloading against graph: {kind}")
        for name, sim in (("graph", graph), ("eager", eager), ("ref", ref)):
            RC.same(sim.field_to_numpy(), at_stops, f"{name}: the riders changed the trajectory")
        # after the stops
        for sim in (graph, eager):
            sim.stop_history()
            sim.stop_averaging()
            sim.stop_modes()
            sim.stop_pod()
            sim.stop_distributions()
            sim.stop_spectra()
            sim.stop_cross_spectra()
            sim.stop_scale_fluxes()
            sim.stop_budget()
            sim.stop_body()
            sim.stop_tracer_accumulation()
            sim.stop_tracers()
            sim.stop_vortices()
            assert sim._riders() == []
        assert all(RC.rider_tokens(sig) == [] for sig in graph._graphs), "a cached graph holds the launch of a stopped rider"
        assert graph._graph is None or RC.rider_tokens(graph._graph[0]) == []
        for kind in ("history", "loads", "vortices"):
            RC.same(RC.read(graph, kind), got[kind], f"kept after the stop: {kind}")
        graph.run(RC.MORE)
        eager.run(RC.MORE, graph=False)
        assert graph._graphs, "the run after the stops replayed no graph"
        RC.same(graph.field_to_numpy(), at_end, "graph after the stops")
        RC.same(eager.field_to_numpy(), at_end, "eager after the stops")
    finally:
        for sim in sims:
            RC.close(sim)


LONG_FORM_CAPACITIES = (30, 16, 11)     # rooms of 30, 33 and 35 steps


def test_all_ten_kinds_through_the_long_form_recapture(hip_lib):
    """With the rings of the test above no chunk behind the first has the 18 steps of a long-form graph (three periods of 6), so run() never
    takes the path that gives a cached period its long form later.  Rings of 30, 16 and 11 records: the first chunk, 30 steps, pays for the
    search and the period of 6 but not for 18 more; the chunk from step 35 to step 60 starts in the cached phase and has them.  f32: in
    f64 the rotation has 4 steps and the first chunk holds its long form."""
    sims = [RC.attach(RC.make("f32"), capacities=LONG_FORM_CAPACITIES) for _ in range(2)]
    graph, eager = sims
    try:
        tokens = [t for r in graph._riders() for t in r.tokens()]
        graph.run(30)
        assert [(e[1], e[2]) for e in graph._graphs.values()] == [(6, None)], "the first chunk cached something else than a bare period of 6"
        graph.run(RC.STEPS - 30)
        eager.run(RC.STEPS, graph=False)
        assert [(e[1], e[2] is not None and e[2][1]) for e in graph._graphs.values()] == [(6, 18)], "no chunk gave the cached period its long form"
        for r, cap in zip((graph._recorder, graph._tracker, graph._vortexr), LONG_FORM_CAPACITIES):
            assert cap <= r.drained and r.issued == RC.STEPS, type(r).__name__
        assert graph._tracers.sorts == eager._tracers.sorts == 3 and graph._tracers.issued == RC.STEPS
        for sig in graph._graphs:
            assert RC.rider_tokens(sig) == tokens
        for kind in RC.KINDS:
            RC.same(RC.read(graph, kind), RC.read(eager, kind), f"graph against eager: {kind}")
        assert graph.history()["step"].tolist() == RC.samples(**RC.HISTORY) and graph.vortices()["count"].sum() > 0
        RC.same(graph.field_to_numpy(), eager.field_to_numpy(), "fields")
    finally:
        for sim in sims:
            RC.close(sim)
