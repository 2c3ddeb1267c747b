#!/usr/bin/env python3
"""Which kernel runs for which input: for a fixed list of configurations, 3 steps of a simulator with profiling on, then per launch (profile) name
the sorted __global__ symbols that ran under it (fs_prof_kernels) and a SHA-256 of every field of field_to_numpy().

    python tools/record_launch_kernels.py > tests/golden/launch_kernels.json

tests/test_gpu_dispatch_table.py runs the same list and requires both to equal the recording: a change of the host-side kernel selection that is
meant to change nothing is run against a recording of the commit before it.

The list holds one configuration per branch of the launch sites (csrc/fs_transport.hip, fs_pressure.hip), each at the smallest grid that reaches
it: the size-dependent forms through the library's switches (FS_RBPAIR_SPLIT, FS_SMALL_CELLS, FS_FUSE_K2, FS_TILE_LIST), a larger grid only for the
thresholds without a switch - 2^20 cells (res 800: the rows of fs_mac_update, the one-launch red-black pair), 2^21 .. 2^23 (res 1024: the quad
band of the fused K3 + K4 pass), 2^23 (res 2048: its 4-row pair tiles in two parts)."""
import hashlib
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
SWITCHES = ("FS_RBPAIR_SPLIT", "FS_SMALL_CELLS", "FS_FUSE_K2", "FS_TILE_LIST", "FS_MARCH", "FS_RBSOR_PAIR", "FS_JACOBI_PAIRS", "FS_JACOBI_QUADS",
            "FS_FUSE_TRANSPORT", "FS_LIMIT_GATE", "FS_LIMIT_DEFER")
BIG = {"FS_SMALL_CELLS": "0", "FS_RBPAIR_SPLIT": "2"}      # the large grids' launch forms on a small grid


def _cfg(dtype, bc, dye, scheme, res, updater=None, vc=5.0, env=None, dx=None):
    env = dict(env or {})
    name = "-".join([dtype, f"bc{bc}" + ("dye" if dye else ""), scheme, "rbsor" if updater is None else f"jacobi{updater[1]}", f"res{res}"]
                    + ([] if vc == 5.0 else [f"vc{vc}"]) + ([] if dx is None else [f"dx{dx}"]) + [f"{k[3:].lower()}{v}" for k, v in sorted(env.items())])
    return {"id": name, "dtype": dtype, "bc": bc, "dye": dye, "scheme": scheme, "res": res, "updater": list(updater) if updater else None,
            "vc": vc, "env": env, "dx": dx}


def configurations():
    c = []
    for dtype in ("f32", "f64"):
        # res 128: power-of-two dx (mode 1; 5 where a kernel has both kinds of divisor); res 200: modes 4 on f32, 0 on f64; res 101: X = 202, pairs but no quads
        for res in (128, 200, 101):
            for scheme in ("cip", "upwind", "kk"):
                c.append(_cfg(dtype, 5, False, scheme, res))
            c.append(_cfg(dtype, 2, True, "cip", res))
            c.append(_cfg(dtype, 2, False, "cip", res, updater=("jacobi", 4)))
            c.append(_cfg(dtype, 2, False, "cip", res, updater=("jacobi", 12)))
        c.append(_cfg(dtype, 2, True, "upwind", 200))
        c.append(_cfg(dtype, 2, True, "kk", 200))
        c.append(_cfg(dtype, 5, False, "cip", 128, vc=None))
        c.append(_cfg(dtype, 5, False, "cip", 64, dx=6.0))       # every divisor admits a tie: mode 0 on f32 too
        c.append(_cfg(dtype, 5, False, "kk", 64, dx=2.0))        # power-of-two dx whose other divisors admit a tie: mode 1 alone
        # the large grids' forms by switch (res 256: the smallest grid with all-fluid tiles)
        c.append(_cfg(dtype, 5, False, "cip", 256, env=BIG))
        c.append(_cfg(dtype, 5, False, "kk", 256, env=BIG))
        c.append(_cfg(dtype, 2, True, "cip", 128, env=BIG))
        c.append(_cfg(dtype, 2, False, "cip", 128, updater=("jacobi", 12), env=BIG))
        c.append(_cfg(dtype, 5, False, "cip", 256, env={"FS_RBPAIR_SPLIT": "0"}))
        c.append(_cfg(dtype, 5, False, "cip", 200, env=BIG))     # ... and without the power-of-two dx
        c.append(_cfg(dtype, 5, False, "kk", 200, env=BIG))
        c.append(_cfg(dtype, 2, True, "cip", 200, env=BIG))
        c.append(_cfg(dtype, 2, False, "cip", 200, updater=("jacobi", 12), env=BIG))
    for fuse in ("1", "0"):
        c.append(_cfg("f32", 5, False, "cip", 256, env=dict(BIG, FS_FUSE_K2=fuse)))
        c.append(_cfg("f32", 2, True, "cip", 256, env=dict(BIG, FS_FUSE_K2=fuse)))
        c.append(_cfg("f32", 2, True, "cip", 128, env={"FS_FUSE_K2": fuse}))
        c.append(_cfg("f32", 5, False, "cip", 200, env=dict(BIG, FS_FUSE_K2=fuse)))
        c.append(_cfg("f32", 2, True, "cip", 200, env=dict(BIG, FS_FUSE_K2=fuse)))
    c.append(_cfg("f32", 5, False, "cip", 256, env=BIG, dx=6.0))
    c.append(_cfg("f32", 2, True, "cip", 128, env=BIG, dx=6.0))
    c.append(_cfg("f32", 5, False, "cip", 256, env={"FS_TILE_LIST": "0"}))
    c.append(_cfg("f32", 2, True, "cip", 256, env={"FS_TILE_LIST": "0"}))
    c.append(_cfg("f32", 5, False, "cip", 256, env={"FS_MARCH": "0"}))
    c.append(_cfg("f32", 2, True, "cip", 128, env={"FS_FUSE_TRANSPORT": "0"}))
    # thresholds without a switch
    c.append(_cfg("f32", 5, False, "cip", 800))
    c.append(_cfg("f32", 5, False, "kk", 800))
    c.append(_cfg("f32", 5, False, "upwind", 800))
    c.append(_cfg("f32", 2, True, "cip", 800))
    c.append(_cfg("f32", 5, False, "cip", 1024))
    c.append(_cfg("f32", 5, False, "cip", 1024, env={"FS_FUSE_K2": "0"}))
    c.append(_cfg("f32", 5, False, "cip", 1024, env={"FS_FUSE_K2": "0", "FS_RBPAIR_SPLIT": "2"}))
    c.append(_cfg("f32", 5, False, "cip", 2048, env={"FS_FUSE_K2": "0"}))
    assert len({x["id"] for x in c}) == len(c)
    return c


def run(cfg):
    """{"kernels": {launch name: sorted symbols}, "digests": {field: sha256}} of one configuration."""
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    importlib.import_module("2d-fluid-simulator_amd")
    import fs
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(cfg["env"])
    try:
        res = cfg["res"]
        dt, dx = 0.05 / res, cfg["dx"] or 1.0 / res
        fs.runtime.init(gpu=0, dtype=cfg["dtype"])
        updater = tuple(cfg["updater"]) if cfg["updater"] else None
        sim = (fs.DyeFluidSimulator if cfg["dye"] else fs.FluidSimulator).create(cfg["bc"], res, dt, dx, 1.0e6, cfg["vc"], cfg["scheme"], pressure_updater=updater)
        dev = sim._solver._bc.device
        try:
            dev.profile(True)
            for _ in range(STEPS):
                sim.step()
            out = sim.field_to_numpy()
            names = sorted(n for n, (count, _) in dev.profile_report().items() if count)
            kernels = {n: sorted(dev.profile_kernels(n)) for n in names}
            digests = {k: hashlib.sha256(memoryview(out[k].copy(order="C")).cast("B")).hexdigest() for k in sorted(out)}
        finally:
            dev.close()
        return {"kernels": kernels, "digests": digests}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    records = []
    for cfg in configurations():
        rec = dict(cfg)
        rec.update(run(cfg))
        records.append(rec)
        print(cfg["id"], len(rec["kernels"]), "launch names", file=sys.stderr, flush=True)
    json.dump({"steps": STEPS, "configurations": records}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
