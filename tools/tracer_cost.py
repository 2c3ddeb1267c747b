"""Cost of the tracer particles: us per step of FluidSimulator.run(graph=True) without tracers and with N particles, alternated in one
process so that clock drift hits both alike; median of the repetitions, one JSON line per configuration.  A last line gives the time of one
advance launch (HIP events around eager launches) for seeds in random order and for the same seeds sorted by cell, the bytes the byte model
counts for it and the float4 copy rate of this GPU measured in the same process.

--sort-every K[,K...] adds one configuration per interval (FluidSimulator.seed_tracers(sort_every=K); 0 is the unsorted set), alternated
with the others, and two more lines: the time of one device sort (HIP events around one tracer_sort: of the randomly ordered set, and of
the set it has just sorted), the advance right after it and 1, 8, 32, ... steps of the running flow later, each pass of the sort from the
launch profile; and the time of one tracer_fields call with the share that is not the launch (allocation, zeroing, download).

--tau T makes a further configuration of the same particles as an INERTIAL set (seed_tracers(tau=T, deposits=True)), --accumulate-every K
one of the inertial set with the accumulated occupancy attached (accumulate_tracers(every=K)); a last line then gives, alternated in one
process between HIP events, the inertial advance launch next to the passive launch of the same particles (random and cell-sorted order)
and the accumulate launch, sampling and not sampling.  Byte model of the inertial launch: 92 B of state per alive particle (the passive 44
plus pu, pw, alpha, tau read - 32 B - and pu, pw written - 16 B) and ONE gather stage instead of two (the second stage of the passive launch
mostly stays on the first stage's lines: the line counts are the same).

Byte model of one launch: 44 B of state per alive particle (x, y, age, status read; x, y, age written) plus the cache lines its gathers
touch - the eight corner values of a stage (four row segments of the velocity field) and one mask byte.  The second stage moves the point by
a fraction of a cell and mostly stays on the first stage's lines; lines are 128 B.  Two counts frame the traffic: every particle fetching
its own lines (no reuse between particles) and every distinct line fetched once (perfect reuse).

  python tools/tracer_cost.py --bc 1 --res 400 --n 16384 --steps 4000 --reps 3
  python tools/tracer_cost.py --bc 5 --res 4096 --n 1048576 --steps 300 --reps 3
  python tools/tracer_cost.py --bc 5 --res 4096 --n 16777216 --steps 1024 --reps 3 --sort-every 0,8,32,128,512
  rocprofv3 --kernel-trace --stats -- python tools/tracer_cost.py --bc 5 --res 4096 --n 1048576 --steps 100 --reps 1 --only-on   (kernel time)
  python tools/tracer_cost.py --bc 5 --res 4096 --n 1048576 --steps 300 --reps 3 --tau 0.001 --accumulate-every 4
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-fluid-simulator_amd"))

LINE = 128


def gather_lines(seeds, X, Y, pitch, esize):
    """(lines summed over the particles, distinct lines) of the first stage's gathers and the mask byte, from the field layout
    [row][channel][pitch] (csrc/fs_device.h) and a mask pitch of `pitch` bytes."""
    fx, fy = seeds[:, 0] - 0.5, seeds[:, 1] - 0.5
    i0 = np.clip(np.floor(fx).astype(np.int64), 0, X - 2)
    j0 = np.clip(np.floor(fy).astype(np.int64), 0, Y - 2)
    ids = []
    for dj in (0, 1):
        for c in (0, 1):
            base = ((j0 + dj) * 2 + c) * pitch + i0
            ids.append(np.stack([base * esize // LINE, (base + 1) * esize // LINE], 1))
    ids = np.concatenate(ids, 1)                                    # (n, 8) line ids of the velocity field
    per = int(((np.diff(np.sort(ids, 1), axis=1) != 0).sum(1) + 1).sum())      # distinct lines of each particle, summed
    m = (np.floor(seeds[:, 1]).astype(np.int64) * pitch + np.floor(seeds[:, 0]).astype(np.int64)) // LINE
    return per + len(seeds), len(np.unique(ids)) + len(np.unique(m))


def _profiled(dev, fn):
    """{profile name: us per launch} of what fn() launches."""
    dev.sync()
    dev.profile_reset()
    dev.profile(True)
    fn()
    dev.sync()
    rep = dev.profile_report()
    dev.profile(False)
    dev.profile_reset()
    return {k: 1e3 * ms / n for k, (n, ms) in rep.items() if n}


def sort_lines(sim, dev, seeds, a):
    """One device sort in isolation, the advance after it as the flow carries the particles on, and one tracer_fields call."""
    sim.seed_tracers(seeds)
    sim.run(64)
    tr = sim._tracers.set
    before = _profiled(dev, sim.step)["tracer_advance"]
    spans = []
    for _ in range(2):                       # the randomly ordered set, then the set just sorted
        dev.sync()
        dev.span_begin()
        dev.tracer_sort(tr)
        spans.append(1e3 * dev.span_end())
    passes = {k: round(v, 2) for k, v in _profiled(dev, lambda: dev.tracer_sort(tr)).items() if k.startswith("tracer_sort")}
    decay, done = {}, 0
    for after in (1, 8, 32, 128, 512, 2048):
        if after - done - 1 > a.steps * 4:
            break
        sim.run(after - done - 1)
        decay[str(after)] = round(_profiled(dev, sim.step)["tracer_advance"], 2)
        done = after
    print(json.dumps({"bc": a.bc, "res": a.res, "tracers": a.n, "note": "one tracer_sort between two HIP events; tracer_advance of one eager step",
                      "sort_us_random_order": round(spans[0], 2), "sort_us_sorted_order": round(spans[1], 2), "sort_passes_us_sorted_order": passes,
                      "advance_us_before_sort": round(before, 2), "advance_us_steps_after_sort": decay}), flush=True)
    dev.sync()
    t0 = time.perf_counter()
    f = sim.tracer_fields()
    wall = 1e6 * (time.perf_counter() - t0)
    launch = _profiled(dev, sim.tracer_fields)["tracer_fields"]
    print(json.dumps({"bc": a.bc, "res": a.res, "tracers": a.n, "note": "one tracer_fields call (host clock) and its launch (zeroing + kernel, HIP events)",
                      "fields_call_us": round(wall, 1), "fields_launch_us": round(launch, 2), "fields_other_share": round(1.0 - launch / wall, 4),
                      "cells_occupied": int((f["count"] > 0).sum())}), flush=True)
    sim.stop_tracers()


def _launch_us(dev, name, fn, reps=20):
    for _ in range(3):
        fn()
    dev.sync()
    dev.profile_reset()
    dev.profile(True)
    for _ in range(reps):
        fn()
    dev.sync()
    n, ms = dev.profile_report()[name]
    dev.profile(False)
    dev.profile_reset()
    return 1e3 * ms / n


def _accumulate_us(dev, tr, h, v, sampling, reps=20):
    """One tracer_accumulate launch behind an advance (the gate counts advances: without one no launch samples), from the launch profile;
    the sample counter afterwards says which path was timed."""
    dev.tracer_accum_create(tr, every=1, start=0 if sampling else 1 << 40)
    step = lambda: (dev.tracer_advance(tr, h, v), dev.tracer_accum_add(tr))
    us = _launch_us(dev, "tracer_accumulate", step, reps)
    launches, samples = dev.tracer_accum_read(tr)[2:]
    assert launches == reps + 3 and samples == (reps + 3 if sampling else 0), (launches, samples, sampling)
    dev.tracer_accum_free(tr)
    return us


def inertial_lines(sim, dev, seeds, a, X, Y, pitch, esize):
    """The inertial advance next to the passive advance of the same particles, alternated three times, and the accumulate launch."""
    from fs.tracers import response
    v = sim._solver.get_fields()[0]
    h = sim._solver.dt / sim._solver.dx
    n = len(seeds)
    tau = np.full(n, a.tau)
    alpha = response(tau, sim._solver.dt)
    order = np.lexsort((np.floor(seeds[:, 0]), np.floor(seeds[:, 1])))
    out = {"bc": a.bc, "res": a.res, "tracers": n, "tau": a.tau, "note": "launches between two HIP events, passive and inertial alternated x3 (medians)"}
    for label, s in (("random", seeds), ("sorted", seeds[order])):
        pas = dev.tracer_create(s, respawn=True)
        ine = dev.tracer_create_inertial(s, alpha, tau, gravity=(0.0, -1.0), respawn=True, deposits=True)
        tp, ti = [], []
        for _ in range(3):
            tp.append(_launch_us(dev, "tracer_advance", lambda: dev.tracer_advance(pas, h, v)))
            ti.append(_launch_us(dev, "tracer_advance_inertial", lambda: dev.tracer_advance(ine, h, v)))
        out[f"passive_us_{label}"] = [round(t, 2) for t in tp]
        out[f"inertial_us_{label}"] = [round(t, 2) for t in ti]
        out[f"inertial_over_passive_{label}"] = round(float(np.median(ti) / np.median(tp)), 3)
        out[f"accumulate_us_sampling_{label}"] = round(_accumulate_us(dev, ine, h, v, True), 2)
        if label == "sorted":
            out["accumulate_us_not_sampling"] = round(_accumulate_us(dev, ine, h, v, False), 2)
        dev.tracer_free(pas)
        dev.tracer_free(ine)
    per, distinct = gather_lines(seeds, X, Y, pitch, esize)
    out.update(model_state_B_per_particle_passive=44, model_state_B_per_particle_inertial=92,
               model_MB_passive_distinct_lines=round((44 * n + distinct * LINE) / 1e6, 3), model_MB_inertial_distinct_lines=round((92 * n + distinct * LINE) / 1e6, 3),
               model_MB_passive_no_reuse=round((44 * n + per * LINE) / 1e6, 3), model_MB_inertial_no_reuse=round((92 * n + per * LINE) / 1e6, 3),
               model_MB_accumulate_sampling=round((28 * n + 2 * 8 * 2 * n) / 1e6, 3))      # x, y, age, status read; two 8-byte atomics (read + write) per particle
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bc", type=int, default=1)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--n", type=int, default=1 << 14)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--only-on", action="store_true", help="run with the tracers only (profiling)")
    ap.add_argument("--sort-every", default="", help="comma-separated sort intervals to measure as configurations of their own (0: unsorted)")
    ap.add_argument("--tau", type=float, default=None, help="also measure the same particles as an inertial set of this response time (simulated time)")
    ap.add_argument("--accumulate-every", type=int, default=0, help="with --tau: also measure the inertial set with accumulate_tracers(every=K)")
    a = ap.parse_args()
    intervals = [int(k) for k in a.sort_every.split(",") if k != ""]
    import fs
    from fs.tracers import seed_random
    fs.runtime.init(gpu=0, dtype="f64" if a.f64 else "f32")
    res = a.res
    sim = fs.FluidSimulator.create(a.bc, res, 0.05 / res, 1.0 / res, 1e6, a.vc or None, a.scheme)
    dev = sim._solver._bc.device
    mask = np.asarray(sim._solver._bc.mask)
    X, Y = mask.shape
    seeds = seed_random(mask, a.n, 1)
    # a configuration: ("off",) - no tracers -, ("passive", K) - a passive set sorted every K steps, 0: never -, ("inertial", K) - the same
    # particles as an inertial set with deposits, K > 0: with accumulate_tracers(every=K)
    OFF = ("off",)
    configs = ([] if a.only_on else [OFF]) + [("passive", k) for k in (intervals or [0])]
    if a.tau is not None:
        configs += [("inertial", 0)] + ([("inertial", a.accumulate_every)] if a.accumulate_every > 0 else [])
    sim.run(64)
    rates = {c: [] for c in configs}
    for _ in range(a.reps):
        for on in configs:
            if on[0] == "inertial":
                sim.seed_tracers(seeds, tau=a.tau, gravity=(0.0, -1.0), deposits=True)
                if on[1]:
                    sim.accumulate_tracers(every=on[1])
            elif on[0] == "passive":
                sim.seed_tracers(seeds, sort_every=on[1])
            sim.run(64)                              # (captures the graphs of this mode)
            dev.sync()
            t0 = time.perf_counter()
            sim.run(a.steps)
            dev.sync()
            rates[on].append(a.steps / (time.perf_counter() - t0))
            if on != OFF:
                st = sim.tracers()
                if on[0] == "inertial" and on[1]:
                    assert sim.tracer_accumulation()["samples"] == (a.steps + 64) // on[1]
                sim.stop_tracers()
                assert st["steps"] == a.steps + 64, st["steps"]
    base = float(np.median(rates[OFF])) if OFF in rates else None
    for on in configs:
        med = float(np.median(rates[on]))
        out = {"bc": a.bc, "res": res, "dtype": "f64" if a.f64 else "f32", "steps": a.steps, "tracers": a.n if on != OFF else 0,
               "steps_per_s": [round(r, 1) for r in rates[on]], "us_per_step": round(1e6 / med, 3)}
        if on[0] == "inertial":
            out.update(inertial_tau=a.tau, accumulate_every=on[1])
        elif on[0] == "passive" and intervals:
            out["sort_every"] = on[1]
        if on != OFF and base:
            # the surcharge of every repetition against the same repetition's run without tracers: its spread is the yardstick of a gain
            per_rep = [1e6 / r - 1e6 / b for r, b in zip(rates[on], rates[OFF])]
            out.update(cost_us_per_step=round(1e6 / med - 1e6 / base, 3), cost_percent=round(100.0 * (base / med - 1.0), 2),
                       cost_us_per_step_min=round(min(per_rep), 3), cost_us_per_step_max=round(max(per_rep), 3))
        print(json.dumps(out), flush=True)
    if intervals:
        sort_lines(sim, dev, seeds, a)
    # one launch in isolation: 20 advances timed by HIP events, seeds in random order and sorted by cell (row, then column)
    v = sim._solver.get_fields()[0]
    h = sim._solver.dt / sim._solver.dx
    esize = 8 if a.f64 else 4
    pitch = (X + 63) // 64 * 64
    order = np.lexsort((np.floor(seeds[:, 0]), np.floor(seeds[:, 1])))
    launch_us = {}
    for label, s in (("random", seeds), ("sorted", seeds[order])):
        tr = dev.tracer_create(s, respawn=True)
        for _ in range(3):
            dev.tracer_advance(tr, h, v)
        dev.sync()
        dev.profile_reset()
        dev.profile(True)
        for _ in range(20):
            dev.tracer_advance(tr, h, v)
        dev.sync()
        n, ms = dev.profile_report()["tracer_advance"]
        dev.profile(False)
        dev.profile_reset()
        dev.tracer_free(tr)
        launch_us[label] = 1e3 * ms / n
    per, distinct = gather_lines(seeds, X, Y, pitch, esize)
    state = 44 * a.n
    hi, lo = state + per * LINE, state + distinct * LINE
    rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)
    t = launch_us["random"] * 1e-6
    print(json.dumps({"bc": a.bc, "res": res, "tracers": a.n, "launch_us_random": round(launch_us["random"], 2),
                      "launch_us_sorted": round(launch_us["sorted"], 2), "note": "one tracer_advance launch between two HIP events",
                      "state_MB": round(state / 1e6, 3), "model_MB_no_reuse": round(hi / 1e6, 3), "model_MB_distinct_lines": round(lo / 1e6, 3),
                      "GBps_no_reuse": round(hi / t / 1e9, 1), "GBps_distinct_lines": round(lo / t / 1e9, 1),
                      "ns_per_particle": round(1e3 * launch_us["random"] / a.n, 4),
                      "box_read_GBps": round(rd, 1), "box_copy_GBps": round(cp, 1), "frac_of_box_copy_no_reuse": round(hi / t / 1e9 / cp, 4),
                      "frac_of_box_copy_distinct_lines": round(lo / t / 1e9 / cp, 4)}), flush=True)
    if a.tau is not None:
        inertial_lines(sim, dev, seeds, a, X, Y, pitch, esize)
    dev.close()


if __name__ == "__main__":
    main()
