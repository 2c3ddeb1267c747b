"""Cost of the multigrid pressure updater: microseconds per step of the same simulator with the default RB-SOR(1.3, 2) and with
("multigrid", cycles), each as FluidSimulator.run(graph=True) and as eager step() calls, one JSON line per configuration, with the rms
Poisson residual the run ends on (FluidSimulator.pressure_residual) and the updater's launch count.  FS_MG_TAIL in the environment moves the
one-workgroup tail (fs/pressure_updater.py); the record is profiles/mg_cost.txt.  The default scheme is upwind without vorticity
confinement: the CIP solver goes unstable under a converged pressure, and a run full of NaN times nothing worth knowing.
--coarsest direct adds (or, with --only direct, runs alone) the updater with the exact last level (coarsest="direct", --direct-cells); each
multigrid line then also carries "kernels_us": per launch name, (launches, microseconds) of one eager step under the library's event
profile - the mg_direct launch alone among them; the record is profiles/mg_direct_cost.txt.  Timed runs are repeated --repeats times after
the warm-up and every repeat is printed: compare medians.

  python tools/mg_cost.py --bc 5 --res 4096 --steps 40 --eager 10
  python tools/mg_cost.py --bc 1 --res 400 --steps 400 --eager 100
  python tools/mg_cost.py --bc 5 --res 4096 --steps 40 --eager 10 --coarsest direct --direct-cells 2048
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bc", type=int, default=1)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200, help="timed steps of the graph replay")
    ap.add_argument("--eager", type=int, default=50, help="timed eager steps")
    ap.add_argument("--cycles", type=int, default=1)
    ap.add_argument("--scheme", default="upwind")
    ap.add_argument("--vc", type=float, default=0.0)
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--only", choices=["rbsor", "multigrid", "direct"], default=None)
    ap.add_argument("--coarsest", choices=["sweeps", "direct"], default="sweeps", help="direct: also time the updater with the exact last level")
    ap.add_argument("--direct-cells", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats of the graph and of the eager run")
    a = ap.parse_args()
    import fs
    res, dt = a.res, 0.05 / a.res
    configs = [("rbsor", None), ("multigrid", ("multigrid", a.cycles))]
    if a.coarsest == "direct" or a.only == "direct":
        configs.append(("direct", ("multigrid", a.cycles, dict(coarsest="direct", direct_cells=a.direct_cells))))
    for name, spec in configs:
        if a.only and a.only != name:
            continue
        fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
        sim = fs.FluidSimulator.create(a.bc, res, dt, 1.0 / res, 1e6, a.vc or None, a.scheme, pressure_updater=spec)
        dev = sim._solver._bc.device
        sim.run(48)                      # (captures the graphs)
        dev.sync()
        graph, eager = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            graph.append(round(1e6 * (time.perf_counter() - t0) / a.steps, 1))
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.eager):
                sim.step()
            dev.sync()
            eager.append(round(1e6 * (time.perf_counter() - t0) / a.eager, 1))
        out = {"bc": a.bc, "res": res, "dtype": "f64" if a.f64 else "f32", "scheme": a.scheme, "vc": a.vc, "updater": name,
               "graph_us_per_step": sorted(graph)[len(graph) // 2], "eager_us_per_step": sorted(eager)[len(eager) // 2], "graph_used": sim._graph is not None,
               "p_residual_rms": sim.pressure_residual(), "FS_MG_TAIL": os.environ.get("FS_MG_TAIL", "default")}
        if a.repeats > 1:
            out.update(graph_us_repeats=graph, eager_us_repeats=eager)
        if spec:
            out.update(cycles=a.cycles, **sim._solver.pressure_updater.info())
            if a.coarsest == "direct" or a.only == "direct":      # one eager step under the event profile: (launches, us) per launch name
                dev.profile(True)
                dev.profile_reset()
                sim.step()
                dev.sync()
                out["kernels_us"] = {k: (n, round(1e3 * ms, 1)) for k, (n, ms) in dev.profile_report().items() if k.startswith("mg_")}
                dev.profile(False)
        print(json.dumps(out), flush=True)
        dev.close()


if __name__ == "__main__":
    main()
