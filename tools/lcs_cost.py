"""Cost of the flow maps through the resident snapshots (csrc/fs_lcs.h): on a ring filled by a running flow, the time of one interval launch
(k_flowmap_advance, HIP events, median over the intervals of three maps), of the Cauchy-Green pass, and the wall time of one whole
FluidSimulator.flow_map() - lattice allocation, seeding, the launches, the download of the lattice and the logarithm on the host.  Beside the
numbers the models of the header: 32 gathered values per node and sub-step, 40 B of lattice state per node and launch - and, for
comparison, the tracer advance's measured time per particle and step (0.17 ns in random order, about 0.015 ns in cell order;
the lattice starts in cell order).  One JSON line per configuration.

  python tools/lcs_cost.py --bc 5 --res 4096 --snapshots 16 --refine 1
  python tools/lcs_cost.py --bc 1 --res 400 --snapshots 16 --refine 1 4
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
    ap.add_argument("--snapshots", type=int, default=16)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--refine", type=int, nargs="*", default=[1])
    ap.add_argument("--substeps", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--spinup", type=int, default=200, help="steps before the first snapshot")
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--f64", action="store_true")
    a = ap.parse_args()
    import fs
    from fs import lcs
    fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
    res = a.res
    dt = 0.05 / res
    sim = fs.FluidSimulator.create(a.bc, res, dt, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    mask = np.asarray(sim._solver._bc.mask)
    cells = int(mask.size)
    esize = 8 if a.f64 else 4
    M = a.snapshots
    sim.start_pod(M, every=a.every, start_step=a.spinup)
    sim.run(a.spinup + M * a.every, graph=True)
    dev.sync()
    po = sim._podr
    assert dev.pod_read(po.pod)[1] == M

    for refine in a.refine:
        for substeps in a.substeps:
            for direction in ("forward", "backward"):
                pairs = lcs.intervals(M, M, None, None, direction)
                h = lcs.step_size(a.every, dt, 1.0 / res, substeps, direction)
                fm = dev.flowmap_create(None, refine)
                nodes = fm.shape[0] * fm.shape[1]
                adv, cg = [], []
                for rep in range(4):          # (the first map warms up and is left out)
                    dev.flowmap_reset(fm)
                    dev.sync()
                    dev.profile_reset()
                    dev.profile(True)
                    for s0, s1 in pairs:
                        dev.flowmap_advance(fm, po.pod, s0, s1, h, substeps)
                    dev.flowmap_cauchy_green(fm)
                    dev.sync()
                    rep_ = dev.profile_report()
                    dev.profile(False)
                    if rep:
                        adv.append(1e3 * rep_["flowmap_advance"][1] / rep_["flowmap_advance"][0])
                        cg.append(1e3 * rep_["flowmap_cauchy_green"][1])
                status = dev.flowmap_get(fm)[2]
                dev.flowmap_free(fm)
                walls = []
                for _ in range(3):
                    dev.sync()
                    t0 = time.perf_counter()
                    sim.flow_map(direction, refine=refine, substeps=substeps)
                    walls.append(time.perf_counter() - t0)
                adv_us, cg_us = float(np.median(adv)), float(np.median(cg))
                gathered = 32 * esize * nodes * substeps
                print(json.dumps({"bc": a.bc, "res": res, "dtype": "f64" if a.f64 else "f32", "snapshots": M, "every": a.every, "cells": cells,
                                  "refine": refine, "nodes": nodes, "substeps": substeps, "direction": direction, "intervals": len(pairs),
                                  "alive_at_end": int((status == 0).sum()), "unseeded": int((status == 4).sum()),
                                  "advance_us_per_interval": round(adv_us, 1), "ns_per_node_substep": round(1e3 * adv_us / (nodes * substeps), 4),
                                  "model_gathered_MB_per_launch": round(gathered / 1e6, 1), "model_state_MB_per_launch": round(40 * nodes / 1e6, 1),
                                  "gathered_GBps": round(gathered / (adv_us * 1e-6) / 1e9, 1), "two_snapshots_uw_MB": round(4 * esize * cells / 1e6, 1),
                                  "cauchy_green_us": round(cg_us, 1), "flow_map_wall_ms": [round(1e3 * w, 2) for w in walls],
                                  "tracer_advance_ns_per_particle_step": {"random_order": 0.17, "cell_order": 0.015}}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
