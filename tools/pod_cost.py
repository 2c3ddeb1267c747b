"""Cost of the snapshot POD: steps/s of FluidSimulator.run(graph=True) without the rider and with start_pod(M) every N steps - by default
every = 1 and 10 - alternated in one process so that clock drift hits all alike; median of the repetitions, one JSON line per configuration.
Then, for every M asked for (default 16 and 32): the wall time of one sim.pod() on a full ring (Gram matrix on the device, download of
M x M doubles, eigh on the host) and of one sim.pod_fields(0); and the launches alone, timed by HIP events: k_pod_gram's two stages
(profile name pod_gram) against the model of csrc/fs_pod.h - every resident u and w plane read nt = ceil(n / 8) times, n (n + 1)
multiplications and as many additions in double per cell - and a sampling / a non-sampling capture launch against its byte model
(3 sizeof(T) + 1 in and 3 sizeof(T) out per not-wall cell, 1 in and 3 sizeof(T) out per wall cell) and this GPU's copy rate.

  python tools/pod_cost.py --bc 1 --res 400 --steps 4000 --reps 3
  python tools/pod_cost.py --bc 5 --res 4096 --steps 300 --reps 3
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
    ap.add_argument("--every", type=int, nargs="*", default=[1, 10], help="sampling intervals of the configurations with the rider")
    ap.add_argument("--ride-slots", type=int, default=16, help="M of the configurations that measure the surcharge per step")
    ap.add_argument("--slots", type=int, nargs="*", default=[16, 32], help="M of the timed pod() calls and of the isolated launches")
    a = ap.parse_args()
    import fs
    fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
    res = a.res
    dt = 0.05 / res
    sim = fs.FluidSimulator.create(a.bc, res, dt, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    mask = np.asarray(sim._solver._bc.mask)
    cells, fluid = int(mask.size), int((mask != 1).sum())
    esize = 8 if a.f64 else 4
    dtype = "f64" if a.f64 else "f32"

    configs = [None] + list(a.every)
    sim.run(64)
    rates = {c: [] for c in configs}
    for _ in range(a.reps):
        for c in configs:
            if c:
                sim.start_pod(a.ride_slots, every=c)
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[c].append(a.steps / (time.perf_counter() - t0))
            if c:
                n = dev.pod_read(sim._podr.pod)[1]
                sim.stop_pod()
                assert n == (a.steps + 64) // c, n
    base = float(np.median(rates[None]))
    for c in configs:
        med = float(np.median(rates[c]))
        out = {"bc": a.bc, "res": res, "dtype": dtype, "steps": a.steps, "snapshots": a.ride_slots if c else 0, "every": c or 0,
               "cells": cells, "not_wall_cells": fluid, "steps_per_s": [round(r, 1) for r in rates[c]], "us_per_step": round(1e6 / med, 3)}
        if c:
            out.update(cost_us_per_step=round(1e6 / med - 1e6 / base, 3), cost_percent=round(100.0 * (base / med - 1.0), 2))
        print(json.dumps(out), flush=True)

    rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)
    v, p = sim._solver.get_fields()[:2]

    def launches(name, fn, n):
        fn()
        dev.sync()
        dev.profile_reset()
        dev.profile(True)
        for _ in range(n):
            fn()
        dev.sync()
        count, ms = dev.profile_report()[name]
        dev.profile(False)
        dev.profile_reset()
        return 1e3 * ms / count

    # the capture launch in isolation: sampling launches (every = 1) and launches that do not sample (start beyond them)
    cap = {}
    for label, kw in (("sampling", dict(every=1)), ("idle", dict(every=1, start=1 << 40))):
        pod = dev.pod_create(4, **kw)
        cap[label] = launches("pod_capture", lambda: dev.pod_launch(pod, v, p), 20)
        dev.pod_free(pod)
    nbytes = fluid * (6 * esize + 1) + (cells - fluid) * (3 * esize + 1)
    gbs = nbytes / (cap["sampling"] * 1e-6) / 1e9
    print(json.dumps({"bc": a.bc, "res": res, "dtype": dtype, "launch": "pod_capture (capture + tick)", "box_read_GBps": round(rd, 1),
                      "box_copy_GBps": round(cp, 1), "launch_us_sampling": round(cap["sampling"], 2), "launch_us_idle": round(cap["idle"], 2),
                      "model_bytes_per_not_wall_cell": 6 * esize + 1, "sample_MB": round(nbytes / 1e6, 1), "sampling_GBps": round(gbs, 1),
                      "frac_of_box_copy": round(gbs / cp, 4)}), flush=True)

    # pod() on a full ring: wall time of the call, and the Gram launches alone against the model
    for M in a.slots:
        sim.start_pod(M, every=1)
        sim.run(M + 3, graph=False)
        dev.sync()
        po = sim._podr
        walls = []
        for _ in range(3):
            po._cache = None
            t0 = time.perf_counter()
            out = sim.pod()
            walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sim.pod_fields(0)
        dev.sync()
        t_fields = time.perf_counter() - t0
        gram_us = launches("pod_gram", lambda: dev.pod_gram(po.pod), 3)
        comb_us = launches("pod_combine", lambda: sim.pod_snapshot(0), 3)
        nt = (M + 7) // 8
        read = 2 * esize * cells * M * nt                           # u and w of every slot, once per tile pair its tile belongs to
        flops = 2 * M * (M + 1) * cells                             # n (n + 1) / 2 pairs x (2 multiplications + 2 additions)
        print(json.dumps({"bc": a.bc, "res": res, "dtype": dtype, "snapshots": M, "resident_MB": round(3 * esize * cells * M / 1e6, 1),
                          "pod_wall_ms": [round(1e3 * w, 2) for w in walls], "pod_fields_wall_ms": round(1e3 * t_fields, 2),
                          "modes": len(out["energies"]), "gram_us": round(gram_us, 1), "gram_model_read_MB": round(read / 1e6, 1),
                          "gram_read_GBps": round(read / (gram_us * 1e-6) / 1e9, 1), "gram_frac_of_box_read": round(read / (gram_us * 1e-6) / 1e9 / rd, 4),
                          "gram_model_GFLOP": round(flops / 1e9, 2), "gram_f64_TFLOPs": round(flops / (gram_us * 1e-6) / 1e12, 3),
                          "combine_us": round(comb_us, 1), "combine_GBps": round((3 * esize * cells * (M + 1) + cells) / (comb_us * 1e-6) / 1e9, 1)}),
              flush=True)
        sim.stop_pod()
    dev.close()


if __name__ == "__main__":
    main()
