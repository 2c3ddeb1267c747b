"""Cost of the energy spectrum: steps/s of FluidSimulator.run(graph=True) without and with start_spectra(box, every=K), alternated in one
process so that clock drift hits both alike.  One JSON line per configuration; --out appends them to a text file
(profiles/spectra_cost.txt).  --box x0,y0,x1,y1 (default: the largest power-of-two box that fits, from the grid's origin).
--pair QA,QB (may be repeated): the same for start_cross_spectra(box, (QA, QB), every=K), alternated with the other two in the same session; the
line gains "pairs": per pair the rates, us_per_step_on and us_per_step_cost, and cost_over_spectra, the ratio to the energy spectrum's cost
(profiles/xspectra_cost.txt).

  python tools/spectra_cost.py --bc 5 --res 4096 --box 0,0,4096,2048 --steps 300 --reps 3 --every 1 --out profiles/spectra_cost.txt
  python tools/spectra_cost.py --bc 1 --res 400 --box 0,0,256,128 --steps 4000 --reps 3 --every 10 --out profiles/spectra_cost.txt
  python tools/spectra_cost.py --bc 5 --res 4096 --box 0,0,4096,2048 --steps 300 --reps 3 --pair u,w --pair vorticity,p --out profiles/xspectra_cost.txt
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
    ap.add_argument("--box", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--pair", action="append", default=[], metavar="QA,QB", help="also measure the cross-spectrum of this pair; may be repeated")
    ap.add_argument("--re", type=float, default=1e6)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, a.re, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    if a.box:
        box = tuple(int(x) for x in a.box.split(","))
    else:
        box = (0, 0, min(4096, 1 << (dev.nx.bit_length() - 1)), min(4096, 1 << (dev.ny.bit_length() - 1)))
    pairs = [tuple(q or None for q in (spec.split(",") + [""])[:2]) for spec in a.pair]
    sim.run(64)
    rates = {False: [], True: []}
    rates.update({pair: [] for pair in pairs})
    for _ in range(a.reps):
        for on in [False, True] + pairs:
            if on is True:
                sim.start_spectra(box, every=a.every)
            elif on:
                sim.start_cross_spectra(box, on, every=a.every)
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[on].append(a.steps / (time.perf_counter() - t0))
            if on is True:
                n = sim.spectra()["samples"]
                sim.stop_spectra()
                assert n == (a.steps + 64) // a.every, n
            elif on:
                n = sim.cross_spectra()["samples"]
                sim.stop_cross_spectra()
                assert n == (a.steps + 64) // a.every, n
    off, on = np.median(rates[False]), np.median(rates[True])
    out = {"tool": "spectra_cost", "bc": a.bc, "res": res, "box": list(box), "steps": a.steps, "every": a.every,
           "off_steps_per_s": [round(r, 1) for r in rates[False]], "on_steps_per_s": [round(r, 1) for r in rates[True]],
           "us_per_step_off": round(1e6 / off, 3), "us_per_step_on": round(1e6 / on, 3), "us_per_step_cost": round(1e6 / on - 1e6 / off, 3),
           "cost_percent": round(100.0 * (off / on - 1.0), 2)}
    if pairs:
        out["tool"], out["pairs"] = "spectra_cost --pair", {}
        for pair in pairs:
            r = np.median(rates[pair])
            out["pairs"][",".join(q for q in pair if q)] = {
                "on_steps_per_s": [round(x, 1) for x in rates[pair]], "us_per_step_on": round(1e6 / r, 3),
                "us_per_step_cost": round(1e6 / r - 1e6 / off, 3), "cost_over_spectra": round((1e6 / r - 1e6 / off) / (1e6 / on - 1e6 / off), 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
