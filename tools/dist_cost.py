"""Cost of the field distributions (csrc/fs_dist.h), one JSON line per scene; --out appends it to a text file (profiles/dist_cost.txt).

  passes       the histogram pass of every quantity (4096 bins) under the library's event profiling, next to the flag pass of the vortex
               tracker on the same fields in the same process, and the bytes each has to move
  contention   --contention: the same pass on the grid of tests/vortex_cases.py with the spread field (uniform random) and the one-bin field
               (solid rotation: the vorticity of about 267,000 cells is exactly +-128), for A/B builds of FS_DIST_COMBINE (FS_LIB selects the
               library, --note names it)
  quantile     sim.quantile("q", 0.9) end to end against the path it replaces - vortex_criterion's download and np.quantile - alternated,
               median of --reps; the split into the value pass, the digit passes and the rest
  rider        steps/s of run(graph=True) without and with start_distributions(every=K), alternated in one process

  python tools/dist_cost.py --bc 5 --res 4096 --steps 200 --reps 3 --out profiles/dist_cost.txt
  python tools/dist_cost.py --bc 1 --res 400 --steps 4000 --reps 3 --out profiles/dist_cost.txt
  python tools/dist_cost.py --contention --reps 3 --note plain --out profiles/dist_cost.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))

QUANTITIES = ("u", "w", "p", "speed", "vorticity", "q", "swirl")
BINS = 4096


def byte_model(cells, fluid, quantity, esize=4):
    """Bytes of one histogram pass: the mask byte of every cell; on the fluid cells p, or u and w once (the four neighbours of the gradient
    quantities come from cache, as in the flag pass of the vortex tracker).  The tables stay in LDS and L2."""
    return cells + fluid * esize * (1 if quantity == "p" else 2)


def profiled(dev, call, names, n):
    """us per launch of `names` over n calls of call()."""
    call()
    dev.profile(True)
    dev.profile_reset()
    for _ in range(n):
        call()
    dev.sync()
    rep = dev.profile_report()
    dev.profile(False)
    return {k: round(1e3 * rep[k][1] / rep[k][0], 2) for k in names if k in rep and rep[k][0]}


def wall(dev, call):
    dev.sync()
    t0 = time.perf_counter()
    call()
    dev.sync()
    return 1e6 * (time.perf_counter() - t0)


def ranges_of(sim, mask):
    """A range per quantity that holds the bulk of the current values (the 1 % and 99 % quantiles, from the select itself)."""
    out = {}
    for q in QUANTITIES:
        lo, hi = sim.quantile(q, [0.01, 0.99])
        out[q] = (float(lo), float(hi)) if lo < hi else (float(lo) - 1.0, float(lo) + 1.0)
    return out


def contention(a):
    import fs
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import vortex_cases as C
    fs.runtime.init(gpu=0, dtype="f32")
    out = {"tool": "dist_cost", "part": "contention", "note": a.note, "grid": list(C.TALL[:2]), "bins": BINS, "fields": {}}
    for name, scene, field, dx in (("spread", C.tall_scene(), C.random_field("float32"), 1.0 / C.TALL[1]),
                                   ("one_bin", C.rotation_scene(), C.rotation_field("float32"), C.ROT_DX)):
        const, mask = scene
        bc = fs.BoundaryCondition(np.array(const), np.array(mask))
        dt = 0.05 * dx
        sim = fs.FluidSimulator(fs.MacSolver(bc, fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2), fs.advect_upwind, dt, dx, 1.0e3, None))
        dev = sim._dev
        sim._solver.v.current.from_numpy(np.array(field))
        lo, hi = (-256.0, 256.0) if name == "one_bin" else (-600.0, 600.0)
        us = [profiled(dev, lambda: sim.histogram("vorticity", BINS, (lo, hi)), ("dist_accumulate",), 32)["dist_accumulate"] for _ in range(a.reps)]
        h = sim.histogram("vorticity", BINS, (lo, hi))
        out["fields"][name] = {"dist_accumulate_us": us, "median_us": float(np.median(us)), "bins_in_use": int((h["counts"] > 0).sum()),
                               "largest_bin": int(h["counts"].max())}
        dev.close()
    return out


def scene(a):
    import fs
    fs.runtime.init(gpu=0, dtype="f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, a.re, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    sim.run(a.warmup)
    mask = np.asarray(sim._solver._bc.mask)
    cells, fluid = int(mask.size), int((mask == 0).sum())
    out = {"tool": "dist_cost", "part": "scene", "note": a.note, "bc": a.bc, "res": res, "steps": a.steps, "cells": cells, "fluid_cells": fluid,
           "bins": BINS}
    rng = ranges_of(sim, mask)
    # the histogram pass per quantity, beside the flag pass of the vortex tracker
    thr = sim.quantile("q", 0.9)
    flags = [profiled(dev, lambda: sim.find_vortices(thr), ("vortex_flags",), 8)["vortex_flags"] for _ in range(a.reps)]
    out["vortex_flags_us"] = float(np.median(flags))
    out["passes"] = {}
    for q in QUANTITIES:
        us = [profiled(dev, lambda: sim.histogram(q, BINS, rng[q]), ("dist_accumulate",), 8)["dist_accumulate"] for _ in range(a.reps)]
        model = byte_model(cells, fluid, q)
        out["passes"][q] = {"us": float(np.median(us)), "all_us": us, "model_bytes": model, "model_gb_per_s": round(model / (np.median(us) * 1e3), 1)}
    joint = [profiled(dev, lambda: sim.histogram("u", 64, rng["u"], against={"quantity": "w", "bins": 64, "range": rng["w"]}),
                      ("dist_accumulate",), 8)["dist_accumulate"] for _ in range(a.reps)]
    out["passes"]["u,w 64x64"] = {"us": float(np.median(joint)), "all_us": joint}
    # the quantile end to end against the download and np.quantile, alternated
    mine, host = [], []
    for _ in range(a.reps):
        mine.append(wall(dev, lambda: sim.quantile("q", 0.9)))
        host.append(wall(dev, lambda: np.quantile(sim.vortex_criterion("q")[mask == 0], 0.9)))
    split = profiled(dev, lambda: sim.quantile("q", 0.9), ("dist_values", "dist_digits"), 4)
    out["quantile"] = {"device_us": [round(x) for x in mine], "download_us": [round(x) for x in host], "device_median_us": round(float(np.median(mine))),
                       "download_median_us": round(float(np.median(host))), "dist_values_us_per_launch": split.get("dist_values"),
                       "dist_digits_us_per_launch": split.get("dist_digits"), "launches": "2 value passes (n, then the plane), 6 digit passes"}
    out["quantile"]["kernels_us"] = round(2 * split.get("dist_values", 0.0) + 6 * split.get("dist_digits", 0.0), 1)
    # the rider: run(graph=True) off / on, alternated
    chan = [{"quantity": "u", "bins": 256, "range": rng["u"]}, {"quantity": "vorticity", "bins": BINS, "range": rng["vorticity"]},
            {"quantity": "u", "bins": 64, "range": rng["u"], "against": {"quantity": "w", "bins": 64, "range": rng["w"]}}]
    out["rider_channels"] = "u 256, vorticity 4096, (u, w) 64 x 64"
    out["runs"] = []
    for every in a.every:
        rates = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                if on:
                    sim.start_distributions(chan, every=every)
                sim.run(64)                              # (captures the graphs of this mode)
                dev.sync()
                t0 = time.perf_counter()
                sim.run(a.steps)
                dev.sync()
                rates[on].append(a.steps / (time.perf_counter() - t0))
                if on:
                    n = sim.distributions()[0]["samples"]
                    sim.stop_distributions()
                    assert n == (a.steps + 64) // every, n
        off, on = np.median(rates[False]), np.median(rates[True])
        out["runs"].append({"every": every, "off_steps_per_s": [round(r, 1) for r in rates[False]], "on_steps_per_s": [round(r, 1) for r in rates[True]],
                            "us_per_step_off": round(1e6 / off, 3), "us_per_step_on": round(1e6 / on, 3),
                            "us_per_step_cost": round(1e6 / on - 1e6 / off, 3), "cost_percent": round(100.0 * (off / on - 1.0), 2)})
    dev.close()
    return out


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
    ap.add_argument("--contention", action="store_true", help="the spread / one-bin comparison on the grid of tests/vortex_cases.py instead of a scene")
    ap.add_argument("--note", default=None, help="a word about the build, kept in the JSON line")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    line = json.dumps(contention(a) if a.contention else scene(a))
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
