"""Cost of the body tracker: steps/s of FluidSimulator.run(graph=True) without and with track_body(every=K) on the scene's body box,
alternated in one process so that clock drift hits both alike.  One JSON line per configuration; --out appends them to a text file
(profiles/loads_cost.txt).

  python tools/loads_cost.py --bc 5 --res 4096 --steps 300 --reps 3 --every 1 --out profiles/loads_cost.txt
  python tools/loads_cost.py --bc 1 --res 400 --steps 4000 --reps 3 --every 10 --out profiles/loads_cost.txt
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
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--re", type=float, default=1e6)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import fs
    from fs.boundary_condition import default_body_box
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, a.re, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    box = default_body_box(a.bc, res)
    sim.run(64)
    rates = {False: [], True: []}
    faces = 0
    for _ in range(a.reps):
        for on in (False, True):
            if on:
                sim.track_body(box, every=a.every)
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[on].append(a.steps / (time.perf_counter() - t0))
            if on:
                n, faces = len(sim.body_loads()["step"]), len(sim.body_surface()["faces"])
                sim.stop_body()
                assert n == (a.steps + 64) // a.every, n
    off, on = np.median(rates[False]), np.median(rates[True])
    out = {"tool": "loads_cost", "bc": a.bc, "res": res, "steps": a.steps, "every": a.every, "faces": int(faces),
           "off_steps_per_s": [round(r, 1) for r in rates[False]], "on_steps_per_s": [round(r, 1) for r in rates[True]],
           "us_per_step_off": round(1e6 / off, 3), "us_per_step_on": round(1e6 / on, 3), "us_per_step_cost": round(1e6 / on - 1e6 / off, 3),
           "cost_percent": round(100.0 * (off / on - 1.0), 2)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
