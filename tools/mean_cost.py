"""Cost of the time averages: steps/s of FluidSimulator.run(graph=True) without an averager and with start_averaging(every=1) and
(every=10), alternated in one process so that clock drift hits all alike; median of the repetitions, one JSON line per configuration.  A
last line gives the time of a sampling and of a non-sampling accumulation launch (HIP events around eager launches), the bytes a sampling
launch moves, and the float4 copy rate of this GPU measured in the same process.

  python tools/mean_cost.py --bc 1 --res 400 --steps 4000 --reps 3
  python tools/mean_cost.py --bc 5 --res 4096 --steps 300 --reps 3
  rocprofv3 --kernel-trace --stats -- python tools/mean_cost.py --bc 5 --res 4096 --steps 100 --reps 1 --only-on   (kernel time)
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
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--every", type=int, nargs="*", default=[1, 10], help="the averaged configurations")
    ap.add_argument("--only-on", action="store_true", help="run with the averager only, every = the first of --every (profiling)")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    cells = int((np.asarray(sim._solver._bc.mask) != 1).sum())
    esize = 8 if a.f64 else 4
    sample_bytes = cells * (3 * esize + 1 + 7 * 16)
    configs = [a.every[0]] if a.only_on else [0] + list(a.every)
    sim.run(64)
    rates = {c: [] for c in configs}
    for _ in range(a.reps):
        for every in configs:
            if every:
                sim.start_averaging(every=every)
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[every].append(a.steps / (time.perf_counter() - t0))
            if every:
                n = dev.mean_read(sim._averager.mean)[2]
                sim.stop_averaging()
                assert n == (a.steps + 64) // every, n
    base = float(np.median(rates[0])) if 0 in rates else None
    for every in configs:
        med = float(np.median(rates[every]))
        out = {"bc": a.bc, "res": res, "dtype": "f64" if a.f64 else "f32", "steps": a.steps, "every": every, "not_wall_cells": cells,
               "steps_per_s": [round(r, 1) for r in rates[every]], "us_per_step": round(1e6 / med, 3)}
        if every and base:
            out.update(cost_us_per_step=round(1e6 / med - 1e6 / base, 3), cost_percent=round(100.0 * (base / med - 1.0), 2))
        print(json.dumps(out), flush=True)
    # one launch in isolation: 20 sampling launches (every = 1) and 20 that do not sample (start beyond them), timed by HIP events
    v, p = sim._solver.get_fields()[:2]
    launch_us = {}
    for label, kw in (("sampling", dict(every=1)), ("idle", dict(every=1, start=1 << 40))):
        m = dev.mean_create(**kw)
        for _ in range(3):
            dev.mean_accumulate(m, v, p)
        dev.sync()
        dev.profile_reset()
        dev.profile(True)
        for _ in range(20):
            dev.mean_accumulate(m, v, p)
        dev.sync()
        n, ms = dev.profile_report()["mean_accumulate"]
        dev.profile(False)
        dev.profile_reset()
        dev.mean_free(m)
        launch_us[label] = 1e3 * ms / n
    rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)
    gbs = sample_bytes / (launch_us["sampling"] * 1e-6) / 1e9
    print(json.dumps({"bc": a.bc, "res": res, "launch_us_sampling": round(launch_us["sampling"], 2), "launch_us_idle": round(launch_us["idle"], 2),
                      "note": "both launches of mean_accumulate (accumulation + counter tick) between two HIP events",
                      "sample_MB": round(sample_bytes / 1e6, 1), "sampling_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000.0, 4),
                      "box_read_GBps": round(rd, 1), "box_copy_GBps": round(cp, 1), "frac_of_box_copy": round(gbs / cp, 4)}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
