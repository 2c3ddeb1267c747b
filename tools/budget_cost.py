"""Cost of the kinetic-energy budget: steps/s of FluidSimulator.run(graph=True) without the rider, with start_budget(box, every=1) and with
every=K (default 10), alternated in one process so that clock drift hits all three alike; the median of --reps runs each.  Then one launch in
isolation (HIP events around eager launches): a sampling and a non-sampling launch of the budget and of the averager, the bytes each sampling
launch moves - one convention for both: 16 bytes per accumulator of every cell that accumulates (fluid cells of the box; not-wall cells
of the grid) and 3 field values and a mask byte for EVERY cell of the box / the grid, walls included -, the achieved bytes per second of
both, and the copy rate of this GPU measured in the same process.  Two JSON lines; --out appends them to a text file
(profiles/budget_cost.txt).

  python tools/budget_cost.py --bc 5 --res 4096 --steps 200 --out profiles/budget_cost.txt
  python tools/budget_cost.py --bc 1 --res 400 --steps 4000 --out profiles/budget_cost.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))


def _launch_us(dev, name, create, launch, free):
    """Microseconds of a sampling and of a non-sampling launch of a rider: 20 eager launches each between HIP events."""
    out = {}
    for label, kw in (("sampling", dict(every=1)), ("idle", dict(every=1, start=1 << 40))):
        h = create(**kw)
        for _ in range(3):
            launch(h)
        dev.sync()
        dev.profile_reset()
        dev.profile(True)
        for _ in range(20):
            launch(h)
        dev.sync()
        n, ms = dev.profile_report()[name]
        dev.profile(False)
        dev.profile_reset()
        free(h)
        out[label] = 1e3 * ms / n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bc", type=int, default=1)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--box", default=None, help="x0,y0,x1,y1 (default: the whole grid)")
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
    mask = np.asarray(sim._solver._bc.mask)
    sub = mask[box[0]:box[2], box[1]:box[3]]
    lines = []
    sim.run(64)
    modes = (0, 1, a.every)                              # 0: no rider
    rates = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:
            if m:
                sim.start_budget(box, every=m)
            sim.run(64)                                  # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[m].append(a.steps / (time.perf_counter() - t0))
            if m:
                n = sim.budget()["samples"] if sub.size <= 1 << 22 else dev.budget_read(sim._budgetr.budget, sums=False)[2]
                sim.stop_budget()
                assert n == (a.steps + 64) // m, n
    us = {m: 1e6 / np.median(rates[m]) for m in modes}
    cost1, costk = us[1] - us[0], us[a.every] - us[0]
    idle = (a.every * costk - cost1) / (a.every - 1) if a.every > 1 else 0.0
    lines.append({"tool": "budget_cost", "bc": a.bc, "res": res, "grid": [dev.nx, dev.ny], "box": list(box), "steps": a.steps, "every": a.every,
                  "off_steps_per_s": [round(r, 1) for r in rates[0]], "every1_steps_per_s": [round(r, 1) for r in rates[1]],
                  "everyK_steps_per_s": [round(r, 1) for r in rates[a.every]], "us_per_step_off": round(us[0], 3),
                  "us_per_step_every1": round(us[1], 3), "us_per_step_everyK": round(us[a.every], 3), "us_per_sampled_step": round(cost1, 3),
                  "us_per_idle_step": round(idle, 3), "cost_percent_every1": round(100.0 * cost1 / us[0], 2),
                  "cost_percent_everyK": round(100.0 * costk / us[0], 2)})
    # one launch in isolation, the budget's and the averager's in the same process
    v, p = sim._solver.get_fields()[:2]
    dx = sim._solver.dx
    bud = _launch_us(dev, "budget_accumulate", lambda **kw: dev.budget_create(box, dx, **kw), lambda h: dev.budget_launch(h, v, p), dev.budget_free)
    mean = _launch_us(dev, "mean_accumulate", lambda **kw: dev.mean_create(**kw), lambda h: dev.mean_accumulate(h, v, p), dev.mean_free)
    fluid, cells, notwall = int((sub == 0).sum()), int(sub.size), int((mask != 1).sum())
    bud_bytes = fluid * 21 * 16 + cells * (3 * 4 + 1)
    mean_bytes = notwall * 7 * 16 + int(mask.size) * (3 * 4 + 1)
    rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)
    bud_gbs, mean_gbs = bud_bytes / (bud["sampling"] * 1e-6) / 1e9, mean_bytes / (mean["sampling"] * 1e-6) / 1e9
    lines.append({"tool": "budget_cost", "bc": a.bc, "res": res, "box": list(box), "fluid_cells": fluid,
                  "note": "both launches of a rider (accumulation + counter tick) between two HIP events; bytes: 16 per accumulator of an accumulating cell, "
                          "13 per cell of the box / grid, walls included, for both riders",
                  "budget_launch_us_sampling": round(bud["sampling"], 2), "budget_launch_us_idle": round(bud["idle"], 2),
                  "budget_sample_MB": round(bud_bytes / 1e6, 1), "budget_GBps": round(bud_gbs, 1),
                  "mean_launch_us_sampling": round(mean["sampling"], 2), "mean_launch_us_idle": round(mean["idle"], 2),
                  "mean_sample_MB": round(mean_bytes / 1e6, 1), "mean_GBps": round(mean_gbs, 1),
                  "box_copy_GBps": round(cp, 1), "budget_frac_of_box_copy": round(bud_gbs / cp, 4), "mean_frac_of_box_copy": round(mean_gbs / cp, 4),
                  "budget_over_mean": round(bud_gbs / mean_gbs, 4)})
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(text + "\n")
    dev.close()


if __name__ == "__main__":
    main()
