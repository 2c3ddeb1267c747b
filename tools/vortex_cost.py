"""Cost of the vortex tracker: steps/s of FluidSimulator.run(graph=True) without and with track_vortices(every=K), alternated in one process
so that clock drift hits both alike; then, in eager steps under the library's event profiling, the time of every launch of a sampling
sequence and of a sequence that does not sample, next to the bytes each launch has to move (the model of DESIGN.md 4ai).  The threshold is
a quantile (--quantile, default 0.9) of the "q" criterion over the fluid cells after the warm-up.  One JSON line per scene; --out appends it to a text file
(profiles/vortex_cost.txt).

  python tools/vortex_cost.py --bc 5 --res 4096 --steps 200 --reps 3 --out profiles/vortex_cost.txt
  python tools/vortex_cost.py --bc 1 --res 400 --steps 4000 --reps 3 --out profiles/vortex_cost.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))

LAUNCHES = ("vortex_flags", "vortex_local", "vortex_seam", "vortex_compress", "vortex_scan", "vortex_ids", "vortex_reduce", "vortex_records",
            "vortex_tick")


def byte_model(cells, flagged, roots, max_components, esize=4):
    """Bytes per launch of a sampling sequence: v is read once per cell by the flag pass (the neighbours come from cache), the planes are
    dense; `flagged` cells carry the per-cell work of the compression and the reduction."""
    return {"vortex_flags": cells * (2 * esize + 1 + 1) + 8 * 15 * max_components, "vortex_local": cells * (1 + 4), "vortex_seam": 0,
            "vortex_compress": cells * 4 + flagged * 8, "vortex_scan": 0, "vortex_ids": cells * 4 + roots * 12,
            "vortex_reduce": cells * 1 + flagged * (4 + 4 + 8 * esize), "vortex_records": 8 * min(roots, max_components), "vortex_tick": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bc", type=int, default=1)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--re", type=float, default=1e6)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--quantile", type=float, default=0.9, help="the threshold: this quantile of Q over the fluid cells after the warm-up")
    ap.add_argument("--note", default=None, help="a word about the build, kept in the JSON line")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, a.re, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    sim.run(a.warmup)
    mask = np.asarray(sim._solver._bc.mask)
    crit = sim.vortex_criterion("q")
    thr = float(np.quantile(crit[mask == 0], a.quantile))
    found = sim.find_vortices(thr)
    flagged = int((sim.vortex_labels()["flags"] != 0).sum())
    cells, roots = int(mask.size), int(found["components"][0])
    out = {"tool": "vortex_cost", "note": a.note, "bc": a.bc, "res": res, "steps": a.steps, "quantile": a.quantile, "threshold": thr, "cells": cells, "flagged_cells": flagged,
           "components": roots, "passed": int(found["passed"][0]), "runs": []}
    for every in a.every:
        rates = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                if on:
                    sim.track_vortices(thr, every=every)
                sim.run(64)                              # (captures the graphs of this mode)
                dev.sync()
                t0 = time.perf_counter()
                sim.run(a.steps)
                dev.sync()
                rates[on].append(a.steps / (time.perf_counter() - t0))
                if on:
                    n = len(sim.vortices()["step"])
                    sim.stop_vortices()
                    assert n == (a.steps + 64) // every, n
        off, on = np.median(rates[False]), np.median(rates[True])
        out["runs"].append({"every": every, "off_steps_per_s": [round(r, 1) for r in rates[False]], "on_steps_per_s": [round(r, 1) for r in rates[True]],
                            "us_per_step_off": round(1e6 / off, 3), "us_per_step_on": round(1e6 / on, 3),
                            "us_per_step_cost": round(1e6 / on - 1e6 / off, 3), "cost_percent": round(100.0 * (off / on - 1.0), 2)})
    # per launch, eager steps under the event profile: a sequence that samples (every=1) and one that does not (start_step beyond the run)
    model = byte_model(cells, flagged, roots, 65536)
    for name, kwargs in (("sampling", {"every": 1}), ("not_sampling", {"every": 1, "start_step": 1 << 40})):
        sim.track_vortices(thr, **kwargs)
        for _ in range(4):
            sim.step()
        dev.profile(True)
        dev.profile_reset()
        for _ in range(32):
            sim.step()
        dev.sync()
        rep = dev.profile_report()
        dev.profile(False)
        sim.stop_vortices()
        us = {k: round(1e3 * rep[k][1] / rep[k][0], 2) for k in LAUNCHES}
        out[name + "_us"] = us
        out[name + "_us_total"] = round(sum(us.values()), 2)
        out[name + "_step_us"] = round(1e3 * sum(ms for n, ms in rep.values()) / 32, 2)
        if name == "sampling":
            out["model_bytes"] = model
            out["model_gb_per_s"] = {k: round(model[k] / (us[k] * 1e3), 1) for k in LAUNCHES if model[k] and us[k] > 0}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
