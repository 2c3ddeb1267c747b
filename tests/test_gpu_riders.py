"""Every rider of the step attached at once (history recorder, time averages, body tracker, tracer particles and their accumulated
occupancy): a run() on replayed graphs, cut into chunks by the two rings and the sort schedule, gathers bit for bit what eager steps gather,
and after the stop_* calls no cached graph holds a rider's launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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
