"""Cost of the harmonic modes: steps/s of FluidSimulator.run(graph=True) without modes and with start_modes of K frequencies every N steps
- by default (K, every) = (1, 1), (1, 10), (2, 10) - alternated in one process so that clock drift hits all alike; median of the repetitions,
one JSON line per configuration.  A last line gives, for every K, the time of a sampling and of a non-sampling accumulation launch (HIP
events around eager launches) and its fraction of this GPU's float4 copy rate on the kernel's own byte model, next to the same numbers of
k_mean_accumulate measured in the same process: the yardstick (the same access pattern with fewer planes).

  python tools/modes_cost.py --bc 1 --res 400 --steps 4000 --reps 3
  python tools/modes_cost.py --bc 5 --res 4096 --steps 300 --reps 3
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
    ap.add_argument("--configs", type=str, nargs="*", default=["1:1", "1:10", "2:10"], help="K:every of the configurations with modes")
    ap.add_argument("--launch-k", type=int, nargs="*", default=[1, 2, 3, 4], help="frequency counts of the isolated launches")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
    res = a.res
    dt = 0.05 / res
    sim = fs.FluidSimulator.create(a.bc, res, dt, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    cells = int((np.asarray(sim._solver._bc.mask) != 1).sum())
    esize = 8 if a.f64 else 4

    def freqs(K, every):      # 0.02 .. 0.08 cycles per sample: far below the Nyquist limit
        return [0.02 * (k + 1) / (every * dt) for k in range(K)]

    configs = [None] + [tuple(int(x) for x in c.split(":")) for c in a.configs]
    sim.run(64)
    rates = {c: [] for c in configs}
    for _ in range(a.reps):
        for c in configs:
            if c:
                sim.start_modes(freqs(*c), every=c[1])
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[c].append(a.steps / (time.perf_counter() - t0))
            if c:
                n = dev.modes_read_scalars(sim._moder.modes)[3]
                sim.stop_modes()
                assert n == (a.steps + 64) // c[1], n
    base = float(np.median(rates[None]))
    for c in configs:
        med = float(np.median(rates[c]))
        out = {"bc": a.bc, "res": res, "dtype": "f64" if a.f64 else "f32", "steps": a.steps, "frequencies": c[0] if c else 0,
               "every": c[1] if c else 0, "not_wall_cells": cells, "steps_per_s": [round(r, 1) for r in rates[c]], "us_per_step": round(1e6 / med, 3)}
        if c:
            out.update(cost_us_per_step=round(1e6 / med - 1e6 / base, 3), cost_percent=round(100.0 * (base / med - 1.0), 2))
        print(json.dumps(out), flush=True)
    # one launch in isolation: 20 sampling launches (every = 1) and 20 that do not sample (start beyond them), timed by HIP events
    v, p = sim._solver.get_fields()[:2]
    rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)

    def timed(name, create, launch, free):
        us = {}
        for label, kw in (("sampling", dict(every=1)), ("idle", dict(every=1, start=1 << 40))):
            m = create(**kw)
            for _ in range(3):
                launch(m)
            dev.sync()
            dev.profile_reset()
            dev.profile(True)
            for _ in range(20):
                launch(m)
            dev.sync()
            n, ms = dev.profile_report()[name]
            dev.profile(False)
            dev.profile_reset()
            free(m)
            us[label] = 1e3 * ms / n
        return us

    def line(what, us, planes):
        nbytes = cells * (3 * esize + 1 + planes * 16)
        gbs = nbytes / (us["sampling"] * 1e-6) / 1e9
        return {"launch": what, "planes": planes, "launch_us_sampling": round(us["sampling"], 2), "launch_us_idle": round(us["idle"], 2),
                "sample_MB": round(nbytes / 1e6, 1), "bytes_per_cell": 3 * esize + 1 + planes * 16, "sampling_GBps": round(gbs, 1),
                "frac_of_box_copy": round(gbs / cp, 4)}

    out = {"bc": a.bc, "res": res, "box_read_GBps": round(rd, 1), "box_copy_GBps": round(cp, 1),
           "note": "both launches of an accumulation (planes + tick) between two HIP events; mean_accumulate before and after the modes: its spread",
           "launches": []}
    mean = lambda: timed("mean_accumulate", dev.mean_create, lambda m: dev.mean_accumulate(m, v, p), dev.mean_free)      # noqa: E731
    out["launches"].append(line("mean_accumulate", mean(), 7))
    for K in a.launch_k:
        cs = np.array([[np.cos(0.3 * (k + 1)), np.sin(0.3 * (k + 1))] for k in range(K)])
        us = timed("modes_accumulate", lambda **kw: dev.modes_create(cs, **kw), lambda m: dev.modes_accumulate(m, v, p), dev.modes_free)
        out["launches"].append(dict(line(f"modes_accumulate K={K}", us, 3 * (1 + 2 * K)), rows_per_workgroup=dev.modes_rows(K)["accumulate"]))
    out["launches"].append(line("mean_accumulate (again)", mean(), 7))
    print(json.dumps(out), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
