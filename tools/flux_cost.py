"""Cost of the scale-to-scale fluxes: steps/s of FluidSimulator.run(graph=True) without the rider, with start_scale_fluxes(box, half_widths,
every=1) and with every=K (default 10), alternated in one process so that clock drift hits all three alike; the median of --reps runs each.
One JSON line per set of half-widths (--half-widths may be repeated); --out appends them to a text file (profiles/flux_cost.txt).
"us_per_sampled_step": the microseconds a sampling step adds - the cost per step at every=1, K times the cost per step at every=K (whose
other K - 1 steps pay the launches that return at once: "us_per_idle_step", from the two).

  python tools/flux_cost.py --bc 5 --res 4096 --box 0,0,4096,2048 --steps 200 --half-widths 1,4,16,64 --half-widths 64 --out profiles/flux_cost.txt
  python tools/flux_cost.py --bc 1 --res 400 --box 0,0,256,128 --steps 4000 --half-widths 1,4,16,64 --half-widths 64 --out profiles/flux_cost.txt
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
    ap.add_argument("--box", default=None, help="x0,y0,x1,y1 (default: the whole grid)")
    ap.add_argument("--half-widths", action="append", default=[], metavar="R,R,..", help="a set of half-widths; may be repeated")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, default=10, help="the sparse cadence measured beside every=1")
    ap.add_argument("--re", type=float, default=1e6)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, a.re, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    box = tuple(int(x) for x in a.box.split(",")) if a.box else (0, 0, dev.nx, dev.ny)
    sets = [tuple(int(r) for r in s.split(",")) for s in (a.half_widths or ["1,4,16,64"])]
    sim.run(64)
    for hw in sets:
        modes = (0, 1, a.every)                          # 0: no rider
        rates = {m: [] for m in modes}
        for _ in range(a.reps):
            for m in modes:
                if m:
                    sim.start_scale_fluxes(box, hw, every=m)
                sim.run(64)                              # (captures the graphs of this mode)
                dev.sync()
                t0 = time.perf_counter()
                sim.run(a.steps)
                dev.sync()
                rates[m].append(a.steps / (time.perf_counter() - t0))
                if m:
                    n = sim.scale_fluxes()["samples"]
                    sim.stop_scale_fluxes()
                    assert n == (a.steps + 64) // m, n
        us = {m: 1e6 / np.median(rates[m]) for m in modes}
        cost1, costk = us[1] - us[0], us[a.every] - us[0]
        idle = (a.every * costk - cost1) / (a.every - 1) if a.every > 1 else 0.0
        out = {"tool": "flux_cost", "bc": a.bc, "res": res, "grid": [dev.nx, dev.ny], "box": list(box), "half_widths": list(hw), "steps": a.steps,
               "every": a.every, "off_steps_per_s": [round(r, 1) for r in rates[0]], "every1_steps_per_s": [round(r, 1) for r in rates[1]],
               "everyK_steps_per_s": [round(r, 1) for r in rates[a.every]], "us_per_step_off": round(us[0], 3),
               "us_per_step_every1": round(us[1], 3), "us_per_step_everyK": round(us[a.every], 3),
               "us_per_sampled_step": round(cost1, 3), "us_per_sampled_step_from_everyK": round(a.every * costk, 3),
               "us_per_idle_step": round(idle, 3), "cost_percent_every1": round(100.0 * cost1 / us[0], 2),
               "cost_percent_everyK": round(100.0 * costk / us[0], 2)}
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
