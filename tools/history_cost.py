"""Cost of the per-step history: steps/s of FluidSimulator.run(graph=True) without and with record_history(every=1) (3 probes and the
scene's body box), alternated in one process so that clock drift hits both alike.  One JSON line per configuration.

  python tools/history_cost.py --bc 1 --res 400 --steps 4000 --reps 3
  rocprofv3 --kernel-trace --stats -- python tools/history_cost.py --bc 5 --res 4096 --steps 200 --reps 1 --only-on   (kernel time)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bc", type=int, default=1)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--only-on", action="store_true", help="time the runs with the recorder only (profiling)")
    a = ap.parse_args()
    import fs
    from fs.boundary_condition import default_body_box
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    mask = sim._solver._bc.mask
    box = default_body_box(a.bc, res) if a.bc in (1, 3, 5, 6) else None
    fluid = np.argwhere(mask == 0)
    probes = [tuple(int(c) for c in fluid[k]) for k in (len(fluid) // 4, len(fluid) // 2, 3 * len(fluid) // 4)]
    sim.run(64)
    rates = {False: [], True: []}
    for _ in range(a.reps):
        for on in ((True,) if a.only_on else (False, True)):
            if on:
                sim.record_history(probes, box)
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[on].append(a.steps / (time.perf_counter() - t0))
            if on:
                n = len(sim.history()["step"])
                sim.stop_history()
                assert n == a.steps + 64, n
    out = {"bc": a.bc, "res": res, "steps": a.steps, "faces": int(len(fs.history.body_faces(mask, box))) if box else 0,
           "on_steps_per_s": [round(r, 1) for r in rates[True]]}
    if not a.only_on:
        off, on = np.median(rates[False]), np.median(rates[True])
        out.update(off_steps_per_s=[round(r, 1) for r in rates[False]], us_per_step_off=round(1e6 / off, 3), us_per_step_on=round(1e6 / on, 3),
                   cost_percent=round(100.0 * (off / on - 1.0), 2))
    print(json.dumps(out), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
