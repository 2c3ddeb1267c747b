#!/usr/bin/env python3
"""bench.py - steps/sec of FluidSimulator.step() on MI355X (+ Poisson-sweep HBM roofline fraction).

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): scene 5, res 4096
(8192 x 4096 cells, f32), CIP advection + vorticity confinement 5.0, red-black SOR(1.3, 2 iterations),
Re 1e6, dt 0.05/res - exactly what `FluidSimulator.create(5, 4096, ...)` builds in the reference.
Synthetic: the scene comes from the NumPy scene builder, the state starts at zero.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--res R] [--dump-outputs DIR] [--full [--no-cpu] [--sweeps S]]

A plain run sets up, warms up, times the K steps and prints the headline (steps/s, ms_per_step).  --full adds everything else the line
used to carry: the box's stream / issue rates, the spread over extra timed blocks, per-kernel HIP-event profiles and HBM roofline
fractions, the isolated Jacobi sweeps, the state checksum and Poisson residual, and the CPU-oracle leg with its in-run parity check.
--dump-outputs DIR (one GPU) writes the fields the last timed step left (v, p [, dye]) as DIR/<name>.npy; every single-GPU mode starts
its timed steps after W + 40 untimed steps, so the files of two builds run with the same arguments compare field for field.

N > 1, one rank per GPU; the grid is cut into N y-slabs (strong scaling: same res 4096 grid), ghost rows travel over RCCL inside
libfs_hip.  Two ways to start it, same result:
  * `python bench.py --gpus N ...` by itself: with WORLD_SIZE unset this process - which never touches the GPU - starts N copies of
    itself as child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT / FS_RDZV_NONCE set), relays
    rank 0's single JSON line, kills the group if a rank dies or the job exceeds FS_BENCH_TIMEOUT (default 1800 s), and exits with
    the worst child status (spawn_ranks below);
  * `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT from the launcher's env).
The bench process itself imports no torch: the RCCL unique id is shared through a file keyed by the launcher, and the barriers around
the timed region and the max-over-ranks of the elapsed time go through the RCCL communicator (Device.barrier / allgather_scalars).

Prints ONE JSON line on rank 0.
"""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # this pool's driver only supports dmabuf IPC (RCCL P2P needs it)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); 6290 GB/s measured float4 copy


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--bc", type=int, default=5)
    ap.add_argument("--scheme", default="cip")
    ap.add_argument("--vc", type=float, default=5.0)
    ap.add_argument("--re", type=float, default=1.0e6)
    ap.add_argument("--dt", type=float, default=0.0, help="time step (default 0.05 / res, like the reference's main.py)")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32", help="f64: the build's double-precision instantiation (BASELINE configs[4])")
    ap.add_argument("--no-tape", action="store_true", help="N > 1: keep Python in the timed loop instead of replaying the recorded period")
    ap.add_argument("--dye", action="store_true", help="DyeFluidSimulator (what the reference's main.py runs by default)")
    ap.add_argument("--jacobi", type=int, default=0, help="use JacobiPressureUpdater with this many sweeps/step (BASELINE configs[1])")
    ap.add_argument("--sweeps", type=int, default=200, help="isolated Jacobi sweeps for the roofline leg")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU-oracle baseline leg")
    ap.add_argument("--no-graph", action="store_true", help="do not replay the step as a hipGraph (N=1)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--trial-steps", type=int, default=120,
                    help="N > 1 with FS_OVERLAP unset: steps replayed per exchange mode in the trial that picks one (part of the untimed step budget of every N)")
    ap.add_argument("--roofline-kernel", default="cip_step",
                    help="profile name (a key of `kernels`) of the kernel the `roofline` object prices: fixed by name, not by which launch happened to be "
                         "slowest.  Default: cip_step, the headline workload's dominant kernel; a workload that never launches it (upwind / KK / f64 / "
                         "odd widths) falls back to the kernel with the largest share of the step and says so in roofline.selection")
    ap.add_argument("--force-dist", action="store_true",
                    help="debug: take the multi-process code path (gloo rendezvous + RCCL communicator) even with one rank")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: box rates, timed blocks, per-kernel profile and roofline, "
                         "isolated Jacobi sweeps, state checksum, Poisson residual, CPU-oracle baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the fields the last timed step left (what field_to_numpy() returns) as DIR/<name>.npy; one GPU only")
    return ap.parse_args()


DUMP_LIMIT = 64_000_000     # bytes of .npy files --dump-outputs may write in all


def dump_outputs(fields, out_dir, limit=DUMP_LIMIT, seed=0):
    """Write `fields` (name -> (X, Y[, C]) array) as <out_dir>/<name>.npy in their own float type.  When the whole fields exceed `limit`
    bytes, every field keeps the same x columns (axis 0): a sorted sample drawn with `seed`, as many columns as fit.  Same shape and seed,
    same columns."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    nx = next(iter(fields.values())).shape[0]
    keep = min(nx, (limit - 4096) // sum(a[0].nbytes for a in fields.values()))      # (4 KiB for the .npy headers)
    cols = None if keep >= nx else np.sort(np.random.default_rng(seed).choice(nx, keep, replace=False))
    for name, a in fields.items():
        np.save(os.path.join(out_dir, name + ".npy"), a if cols is None else np.ascontiguousarray(a[cols]))


def algorithmic_bytes(mask, esize=4):
    """Algorithmic HBM bytes per launch of each kernel: every distinct array element touched once, no
    stencil re-reads, no write-allocate.  N = cells, nw = not-wall, fl = fluid."""
    import numpy as np
    n = mask.size
    fl = int((mask == 0).sum())
    nw = int((mask != 1).sum())
    e = esize
    return {
        "cip_nonadv": n + nw * (2 * e + e + 2 * e),                      # v, p -> v'
        "cip_nonadv_grad": n + nw * (4 * e + 4 * e + 4 * e),             # vx,vy,v,v' -> vx',vy'  (8+8+8+8+16 B)
        "cip_advect": n + fl * (6 * e + 6 * e),                          # v,vx,vy -> v',vx',vy'
        # fused K3 + K4 (csrc/fs_k34n.h k_cip_grad_advect_n<2>): mask; fc read and v_out written on the cells some kernel writes (not-wall
        # cells and the velocity boundary targets next to them - counted as not-wall; deep wall tiles move nothing since round 3); fn on
        # fluid cells; old gradients read and new gradients written on not-wall cells.  The intermediate gradients the reference's two
        # kernels exchange through HBM (16 B/cell written + read back 3x3) never leave the registers.
        "cip_grad_advect_rt": n + nw * (2 * e + 2 * e) + fl * 2 * e + nw * (4 * e + 4 * e),
        # K2 + K3 + K4 of the velocity as one logical launch (fs_cip_step, csrc/fs_k234.h: K2 is evaluated in registers; "cip_step" over the all-fluid
        # tiles + "cip_step_bnd" over the others): mask; v.current, p and the old gradients read, the advected velocity and the new gradients
        # written - 52 B per not-wall cell.  The post-K2 velocity is no algorithmic byte any more: it reaches HBM only on inflow / outflow cells.
        "cip_step": n + nw * (2 * e + e + 4 * e) + nw * (2 * e + 4 * e),
        # ... and K12 + K3 + K4 of the dye (fs_cip_step_dye): 3 channels + their old gradients read, the advecting velocity on fluid cells, results written
        "cip_step_dye": n + nw * (3 * e + 6 * e) + fl * 2 * e + nw * (3 * e + 6 * e),
        # the same fusion for the dye (k_cip_grad_advect_n<3>): 3 channels + the advecting velocity on fluid cells
        "cip_grad_advect_dye": n + nw * (3 * e + 3 * e) + fl * (3 * e + 2 * e) + nw * (6 * e + 6 * e),
        "vort_calc": n + fl * (2 * e + 2 * e),                           # v -> w, |w|
        "vort_add": n + fl * (2 * e + 2 * e + 2 * e),                    # w,|w|,v -> v'
        "rbsor_iteration": n + fl * (e + e + 2 * e + e),                 # fused odd+even: p.cur, p.next, v -> p.next
        # two iterations + both boundary passes in one pass (csrc/fs_rbpair.h): mask; p.cur, p.next, v read and both results written on fluid cells
        "rbsor_pair": n + fl * (e + e + 2 * e) + fl * (e + e),
        "vort_confine": n + fl * (2 * e + 2 * e),                        # fused K5+K6: v -> v'
        "rbsor_odd": n // 2 + fl * e + (fl // 2) * (2 * e) + (fl // 2) * e,   # p (both colours), v of the other colour, write half
        "rbsor_even": n // 2 + fl * e + (fl // 2) * (2 * e) + (fl // 2) * e,
        "jacobi_sweep": n + nw * (e + 2 * e + e),                        # p, v -> p'   (S = 8: reads v like the reference)
        "jacobi_sweep_src": n + nw * (e + 2 * e + e),                    # p, (s2, s3) -> p'
        "jacobi_sweep_lazy": n + nw * (e + 2 * e + e),                   # the same sweep with K7 evaluated in registers
        "jacobi_pair_lazy": n + nw * (e + 2 * e + e),                    # TWO sweeps per pass: p, (s2, s3) in, p'' out - once
        "jacobi_quad_lazy": n + nw * (e + 2 * e + e),                    # FOUR sweeps per pass: the same bytes once
        "mac_update_upwind": n + fl * (2 * e + e + 2 * e),
        "mac_update_kk": n + fl * (2 * e + e + 2 * e),
        "cip_nonadv_dye": n + nw * (3 * e + 3 * e),
        "cip_nonadv_grad_c3": n + nw * (6 * e + 6 * e + 6 * e),
        "cip_advect_c3": n + fl * (9 * e + 2 * e + 9 * e),
        "clamp_field": n * 6 * e,
        "poisson_source": n * 4 * e,
    }, {"cells": n, "fluid": fl, "not_wall": nw}


def merge_parts(rep, parts=None):
    """Kernels launched in compact parts (the workgroups that see nothing but fluid, then the others: "<name>" + "<name>_bnd", csrc/fs_core.hip
    tile_list; fs_cip_step also "<name>_band": K2 over the rows its boundary tiles read) count as ONE launch of <name>; `parts` (optional dict)
    receives the unmerged (launches, ms) of every part of such a launch."""
    for suffix in ("_bnd", "_band"):
        for name in [n for n in rep if n.endswith(suffix) and n[:-len(suffix)] in rep]:
            base = name[:-len(suffix)]
            if parts is not None:
                parts.setdefault(base, {"plain": rep[base]})[suffix[1:]] = rep[name]
            (l0, m0), (_, m1) = rep[base], rep[name]
            rep[base] = (l0, m0 + m1)
            del rep[name]
    return rep


def cip_step_by_kind(args, res, dt, dx, re, vc, esize, box, steps=12):
    """fs_cip_step as one launch per kind of tile (FS_FUSE_K2=1: k_cip_step_plain over the tiles that see nothing but fluid, k_cip_step_bnd over the
    others) on a second context of the same scene: per-launch HIP-event brackets of `steps` eager steps."""
    import fs
    saved = os.environ.get("FS_FUSE_K2")
    os.environ["FS_FUSE_K2"] = "1"
    sim2 = None
    try:
        sim2 = fs.FluidSimulator.create(args.bc, res, dt, dx, re, vc, args.scheme, pressure_updater=("jacobi", args.jacobi) if args.jacobi else None)
        dev2 = sim2._solver._bc.device
        for _ in range(3):
            sim2.step()
        dev2.profile(True)
        dev2.profile_reset()
        for _ in range(steps):
            sim2.step()
        parts = {}
        merge_parts(dev2.profile_report(), parts)
        dev2.profile(False)
        n_plain, n_bnd, _, t_rows, t_cells = dev2.cip_step_tiles()
        if "cip_step" not in parts or n_plain <= 0:
            return None
        us = {k: v[1] / max(v[0], 1) * 1e3 for k, v in parts["cip_step"].items()}
        pl_bytes = n_plain * t_rows * t_cells * 13 * esize
        gbps = pl_bytes / (us["plain"] * 1e-6) / 1e9
        return {"form": "FS_FUSE_K2=1: k_cip_step_plain over the all-fluid tiles + k_cip_step_bnd over the others, a second context of the same scene, "
                        f"{steps} eager steps", "all_fluid_tiles": n_plain, "other_tiles": n_bnd, "all_fluid_us": round(us["plain"], 2), "others_us": round(us.get("bnd", 0.0), 2),
                "all_fluid_alg_MB": round(pl_bytes / 1e6, 2), "all_fluid_GBps": round(gbps, 1), "all_fluid_frac": round(gbps / HBM_PEAK_GBS, 4),
                "all_fluid_frac_of_box_copy": round(gbps / box["copy_GBps"], 4) if box else None}
    finally:
        if saved is None:
            os.environ.pop("FS_FUSE_K2", None)
        else:
            os.environ["FS_FUSE_K2"] = saved
        if sim2 is not None:
            sim2._solver._bc.device.close()


def usable_cores():
    """Host threads this process can really run on: the affinity mask, capped by the cgroup CPU quota (a container that sees 256
    logical CPUs under a quota of a few cores makes an OpenMP team of 256 spin on its barriers: round 2's 0.7 steps/s)."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                quota, period = int(txt[0]), int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if quota > 0:
                    n = min(n, max(1, quota // period))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(args, scene, sim, dt, abytes_step):
    """The CPU oracle (C restatement of the reference algorithm, OpenMP on the race-free kernels) on this host's cores, on a
    BOUNDED sample of the same workload: it takes over the GPU's developed state (every internal buffer), runs as many steps as
    fit in ~cpu_seconds (>= 2), and the GPU then advances by the same steps - the two must agree bit for bit (parity in the
    same run)."""
    import numpy as np
    # team size: the cores this process may really use, at most one thread per 8 grid columns (the oracle's loops are parallel over x),
    # threads pinned and passive at barriers; set before libgomp starts
    logical = len(os.sched_getaffinity(0))
    cores = int(os.environ.get("OMP_NUM_THREADS", 0)) or max(1, min(usable_cores(), scene[1].shape[0] // 8))
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    from oracle import oracle as O
    O.set_threads(cores)
    const, mask, dye = scene
    res = args.res
    ref = O.make_simulator(const, mask, dye if args.dye else None, scheme=args.scheme, dt=dt, dx=1.0 / res, re=args.re,
                           vor_eps=args.vc if args.vc else None, updater=("jacobi", args.jacobi) if args.jacobi else ("rbsor", 1.3, 2),
                           dtype=np.float32 if args.dtype == "f32" else np.float64)
    s = sim._solver
    for name in ("v", "p", "vx", "vy", "dye", "dyex", "dyey"):
        if hasattr(s, name) and getattr(ref, name, None) is not None:
            getattr(ref, name).current[...] = getattr(s, name).current.to_numpy()
            getattr(ref, name).next[...] = getattr(s, name).next.to_numpy()
    ref.update()                         # untimed: the first step pays the page faults of the oracle's temporaries
    t0 = time.perf_counter()
    n = 0
    while n < 2 or (time.perf_counter() - t0) < args.cpu_seconds:
        ref.update()
        n += 1
        if n >= 200:
            break
    el = time.perf_counter() - t0
    for _ in range(n + 1):
        sim.step()
    out = sim.field_to_numpy()
    same = all(np.array_equal(out[k], e, equal_nan=True) for k, e in ref.fields().items())
    # The graded kernel - the isolated Jacobi sweep the roofline leg times - checked against the oracle's sweep (fs/pressure_updater.py:62-66) on
    # the state just compared: the literal form (reads v) and the source-pair form, whole grid, bit for bit.  (The timed sweeps check no value.)
    dev = s._bc.device
    v_f, p_f = s.get_fields()[:2]
    p_np, v_np = out["p"], out["v"]
    exp = np.zeros_like(p_np)
    O.OracleJacobi(ref.bc, dt, 1.0 / res, 1).sweep(exp, np.ascontiguousarray(p_np), np.ascontiguousarray(v_np))
    pn, src = dev.alloc(1), dev.alloc(2)
    sweeps = {}
    pn.from_numpy(np.zeros_like(p_np))
    dev.jacobi_sweep(dt, 1.0 / res, pn, p_f, v_f)
    sweeps["jacobi_sweep"] = bool(np.array_equal(pn.to_numpy(), exp, equal_nan=True))
    pn.from_numpy(np.zeros_like(p_np))
    dev.poisson_source(dt, 1.0 / res, src, v_f)
    dev.jacobi_sweep_src(pn, p_f, src)
    sweeps["jacobi_sweep_src"] = bool(np.array_equal(pn.to_numpy(), exp, equal_nan=True))
    return {"value": n / el, "unit": "steps/s", "cores": cores, "kind": "port", "host_logical_cpus": logical,
            "GBps": round(abytes_step * n / el / 1e9, 1),
            "sample": f"{n} steps of the same workload (bc{args.bc} res{res} {args.scheme}{' +dye' if args.dye else ''}) continuing from the "
                      f"GPU's state after the timed run, {el:.1f} s, OpenMP C oracle (boundary kernels serial over the boundary cells)",
            "parity_in_run": {"steps": n + 1, "fields": sorted(ref.fields()), "bit_identical": bool(same),
                              "graded_sweep_vs_oracle": sweeps}}


def visible_gpus_without_hip():
    """GPUs this job could use, counted WITHOUT a HIP call (the parent of a self-launched N-rank job must never initialise the GPU): KFD topology
    nodes with SIMDs, capped by the *_VISIBLE_DEVICES lists.  None when the topology cannot be read (then the ranks' own pre-flight decides)."""
    import glob
    import re
    n = 0
    try:
        for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
            m = re.search(r"^simd_count\s+(\d+)", open(path).read(), re.M)
            if m and int(m.group(1)) > 0:
                n += 1
    except OSError:
        return None
    if n == 0:
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        if os.environ.get(var, "").strip():
            n = min(n, len([x for x in os.environ[var].split(",") if x.strip()]))
    return n


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script as CHILD processes and relay rank 0's line.

    This process has not initialised the GPU and never does (replacing a process that has - os.exec* - takes this pool's machines
    down; children are fine).  Rank r gets RANK = LOCAL_RANK = r (FS_BENCH_LOCAL_RANK pins every rank to one device: the single-GPU
    test harness), WORLD_SIZE = N, MASTER_ADDR = 127.0.0.1, a free MASTER_PORT and a per-job FS_RDZV_NONCE that keys the rendezvous
    file of the RCCL unique id.  FS_BENCH_WORKER names another script to run as the rank (tests/bench_socket_worker.py).  A rank
    that exits non-zero dooms the job - the others would wait in a collective for ever - so the rest get 20 s and are then killed;
    the same after FS_BENCH_TIMEOUT seconds (exit status 124).  Returns the worst child status."""
    import socket
    import subprocess
    import threading
    have = visible_gpus_without_hip()
    if have is not None and have < n and "FS_BENCH_LOCAL_RANK" not in os.environ:
        sys.stderr.write(f"bench.py: --gpus {n} but {have} GPU(s) visible on this node (KFD topology / *_VISIBLE_DEVICES); nothing started\n")
        return 2
    worker = os.environ.get("FS_BENCH_WORKER") or os.path.abspath(__file__)
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    nonce = f"{os.getpid()}_{time.time_ns()}"
    deadline = time.time() + float(os.environ.get("FS_BENCH_TIMEOUT", "1800"))
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=os.environ.get("FS_BENCH_LOCAL_RANK", str(r)), WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), FS_RDZV_NONCE=nonce)
        # rank 0's stdout is the job's stdout (captured, relayed at the end: ONE line); the other ranks' stdout joins stderr
        procs.append(subprocess.Popen([sys.executable, worker] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=None))
    captured = []
    reader = threading.Thread(target=lambda: captured.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    doomed_at, timed_out, killed = None, False, set()
    while any(p.poll() is None for p in procs):
        now = time.time()
        if doomed_at is None and any(p.poll() not in (None, 0) for p in procs):
            doomed_at = now + 20.0
        if now > deadline:
            timed_out = True
        if timed_out or (doomed_at is not None and now > doomed_at):
            for r, p in enumerate(procs):
                if p.poll() is None:
                    killed.add(r)
                    p.kill()
            break
        time.sleep(0.05)
    codes = [p.wait() for p in procs]
    reader.join(timeout=10.0)
    out = (captured[0] if captured else b"").decode(errors="replace")
    if out:
        sys.stdout.write(out)
        sys.stdout.flush()
    if timed_out:
        sys.stderr.write(f"bench.py: {n}-rank job exceeded FS_BENCH_TIMEOUT; killed\n")
        return 124
    bad = [c for r, c in enumerate(codes) if c != 0 and r not in killed]        # (the ranks this function killed are the effect, not the cause)
    if bad or killed:
        sys.stderr.write(f"bench.py: rank exit codes {codes}" + (f", ranks {sorted(killed)} killed after another rank failed" if killed else "") + "\n")
        return max([(c if c > 0 else 128 - c) for c in bad] or [1])
    return 0


def main():
    args = parse()
    if args.dump_outputs and (max(args.gpus, int(os.environ.get("WORLD_SIZE", 1))) > 1 or args.force_dist):
        raise SystemExit("bench.py: --dump-outputs needs a single-GPU run (--gpus 1, no --force-dist)")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and not args.force_dist:
        raise SystemExit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        args.gpus = world

    importlib.import_module("2d-fluid-simulator_amd")
    import numpy as np
    import fs
    from fs import _lib
    from fs.boundary_condition import create_scene_arrays
    _lib.load()   # ROCm's HIP runtime is resolved before anything else can bring its own copy

    # N > 1: no torch / MPI in this process.  The only out-of-band datum is the 128-byte RCCL unique id (a file in /tmp
    # keyed by the launcher's pid and MASTER_PORT); barriers and the max-over-ranks go through the RCCL communicator.
    rdzv = None
    bcast = None
    if world > 1 or args.force_dist:
        from fs.rendezvous import FileRendezvous
        rdzv = FileRendezvous(rank, world)
        bcast = rdzv.bcast
        # pre-flight, before any rank can block in ncclCommInitRank: this rank's GPU exists and librccl loads; every rank learns every verdict
        import ctypes
        ndev, rccl_ok = ctypes.c_int(), ctypes.c_int()
        _lib.call("fs_device_count", ctypes.byref(ndev))
        _lib.call("fs_comm_available", ctypes.byref(rccl_ok))
        why = ""
        if local_rank >= ndev.value:
            why = f"rank {rank}: LOCAL_RANK {local_rank} but {ndev.value} GPU(s) visible"
        elif not rccl_ok.value:
            why = f"rank {rank}: {_lib.load().fs_last_error().decode(errors='replace')}"
        failed = rdzv.preflight(not why, why, timeout=float(os.environ.get("FS_PREFLIGHT_TIMEOUT", "120")))
        if failed:
            if rank == 0 or why:
                sys.stderr.write(f"bench.py: --gpus {world} cannot run: " + "; ".join(failed) + "\n")
            raise SystemExit(3)      # (the status files stay for ranks still reading them; they are keyed by this job's launcher / nonce)
        if args.force_dist:
            os.environ["FS_TEST_COMM"] = "1"

    res = args.res
    dt, dx, re = (args.dt or 0.05 / res), 1.0 / res, args.re
    vc = args.vc if args.vc else None
    esize = 4 if args.dtype == "f32" else 8
    fs.runtime.init(gpu=local_rank, dtype=args.dtype, rank=rank, nranks=world, bcast=bcast)
    sim = (fs.DyeFluidSimulator if args.dye else fs.FluidSimulator).create(args.bc, res, dt, dx, re, vc, args.scheme,
                                   pressure_updater=("jacobi", args.jacobi) if args.jacobi else None)
    dev = sim._solver._bc.device
    mask = sim._solver._bc.mask

    # ---- warm-up, then EXACTLY K timed steps between barrier + device sync --------------------------------
    # No Python between two launches of the timed region when it can be avoided:
    #   N = 1: the launches of one PERIOD of the solver's buffer rotation (2 steps when every DoubleBuffer just swaps, 6 for the
    #          default CIP + vorticity-confinement solver: FluidSimulator.capture_period) are captured into a hipGraph after the
    #          warm-up and replayed K // period times (+ K mod period eager steps);
    #   N > 1: a hipGraph cannot carry the RCCL exchange, so the period of the slab step (kernels + exchange begin / wait, 2-4
    #          steps) is logged after the warm-up and replayed from C++ (fs_tape_replay); K mod period steps run eagerly.
    # Every mode advances the state by the same number of steps, so `state_checksum` is comparable across modes and N.
    # what THIS box streams at (the pool's boxes differ by several per cent): ~30 ms of float4 read and of float4 copy on two buffers the
    # size of a 2-channel field of the headline grid (268 MB each: beyond the Infinity Cache), before anything is timed
    box = None
    if args.full and hasattr(dev, "box_rates"):
        rd, cp = dev.box_rates(2 * 8192 * 4096 * 4, 30.0)
        box = {"read_GBps": round(rd, 1), "copy_GBps": round(cp, 1), "buffer_MB": 268.4, "note": "float4 read / copy measured in this run on this GPU before the timed region"}
        if hasattr(dev, "box_valu_rate"):      # what one SIMD of this box issues per second: the issue-bound K3+K4 pass is priced against it (roofline.valu_issue)
            box["valu_ginstr_per_simd"] = round(dev.box_valu_rate(10.0), 3)
        if hasattr(dev, "box_valu_pk_rate"):   # ... and packed f32 instructions (two operations per lane each): the same rate means twice the arithmetic
            box["valu_pk_ginstr_per_simd"] = round(dev.box_valu_pk_rate(10.0), 3)
        if hasattr(dev, "box_mixed_rate"):     # stream + ALU at once, 100 ms: the two pure probes measured alike on boxes whose kernels differed by 5-9 %
            box["mixed_GBps"] = round(dev.box_mixed_rate(2 * 8192 * 4096 * 4, 100.0), 1)
    for _ in range(args.warmup):
        sim.step()
    graph = tape = glong = None
    launch = "eager (python per step)"
    # Untimed steps reserved for finding / capturing the replayable period and - N > 1 - for choosing the exchange mode: what a run does not
    # use of the budget is stepped AFTER the timed region, so every mode and every N takes the same total (state_checksum is comparable).
    #   N > 1, FS_OVERLAP unset: the exchanges of a slab step can run in line on the compute stream or on the communication stream behind the
    #   interior rows of the kernel that needs them - same bits, and which one is faster depends on the links (in loop-back the in-line form wins
    #   by 15 %; on xGMI a transfer is ~40 us of a ~100 us step).  So the run measures: the period is recorded and replayed for TRIAL steps in
    #   each mode, the max-over-ranks times decide (every rank sees the same numbers), a tie within 2 % keeps the simpler in-line form, and the
    #   tape of the chosen mode is the one the timed region replays.  Both timings go into exchange_model.
    SETTLE, TRIAL = 40, max(int(args.trial_steps), 2)
    settle = 3 * SETTLE + 2 * TRIAL     # (every N takes the same budget - state_checksum is compared across --gpus 1/2/4/8 - and `after_steps` says how many)
    later = 0
    exchange_trial = None
    # N = 1: the timed steps start after warmup + SETTLE untimed steps in every mode, whatever the capture took, so what they compute
    # (--dump-outputs) depends on the arguments alone.  The graph starts at the phase of the buffer rotation it was captured in: `lead`
    # eager steps of the timed region bring the padded state back to it.
    phase0 = lead = 0
    if world == 1 and not args.force_dist and not args.no_graph:
        done = sim.capture_period(budget=SETTLE)       # one period of the buffer rotation (2 or 6 steps) as a hipGraph
        for _ in range(SETTLE - done):
            sim.step()
        later = settle - SETTLE
        if sim._graph is not None:
            graph, gperiod = sim._graph[1], sim._graph[2]
            glong = sim._graph_long        # the same period repeated to >= 16 steps in one graph: ~5 us of idle time per replay, whatever it holds
            launch = f"hipGraph replay of {gperiod}-step periods" + (f" ({glong[1]} steps per graph)" if glong else "")
            phase0 = (SETTLE - done) % gperiod
            lead = min((gperiod - phase0) % gperiod, args.steps)
    elif (world > 1 or args.force_dist) and not args.no_tape:
        done = [0]

        def counted():
            sim.step()
            done[0] += 1

        def record():
            return dev.tape_period(counted, nsteps=2, tries=SETTLE // 2)      # returns AT the start of a period: replay must follow directly
        auto = "FS_OVERLAP" not in os.environ and hasattr(dev, "set_overlap") and world > 1
        if auto:
            tape, exchange_trial = dev.choose_exchange_mode(counted, record_tries=SETTLE // 2, trial_steps=TRIAL)
            done[0] += exchange_trial["replayed_steps"]
        else:
            tape = record()
        if tape is not None:
            # One whole period EAGERLY in the mode the timed region runs in (it ends where it began: at the start of a period).  The timed K steps are
            # replays + K mod period eager steps; with the exchanges on the communication stream an eager kernel is split into interior rows and edge
            # strips - row ranges no launch has had yet while the period was logged (the log runs with blocking exchanges).  Their launch lists
            # (one hipMalloc + stream sync each) are built HERE, not inside the timed region (`launch_lists` in the line).
            for _ in range(tape["nsteps"]):
                counted()
        later = settle - done[0]
        if tape is not None:
            launch = f"tape replay of {tape['nsteps']}-step periods ({len(tape['ops'])} operations, C++ loop)"
    else:
        for _ in range(SETTLE):
            sim.step()
        later = settle - SETTLE
    pu = sim._solver.pressure_updater
    launch += "; pressure: " + (getattr(pu, "form", None) or ("two red-black iterations per pass (fs_rbsor_pair)" if getattr(pu, "_pair", False)
                                                              else "one fused red-black iteration per launch"))
    def replay_graphs(nsteps):          # whole periods of `nsteps`: the long graph first, the rest one period at a time
        if glong is not None:
            dev.replay(glong[0], nsteps // glong[1])
            nsteps %= glong[1]
        dev.replay(graph, nsteps // gperiod)

    lists_before = dev.tile_list_stats() if args.full and hasattr(dev, "tile_list_stats") else None
    dev.barrier()                      # device sync + all ranks arrived
    t0 = time.perf_counter()
    if graph is not None:
        for _ in range(lead):
            sim.step()
        if args.steps - lead >= gperiod and sim._signature() != sim._graph[0]:      # (checked while the GPU runs the lead steps)
            raise SystemExit("bench: the state is not at the phase of the captured graph; replaying it would compute garbage")
        replay_graphs(args.steps - lead)
        for _ in range((args.steps - lead) % gperiod):
            sim.step()
    elif tape is not None:
        dev.replay_tape(tape, args.steps // tape["nsteps"])
        for _ in range(args.steps % tape["nsteps"]):
            sim.step()
    else:
        for _ in range(args.steps):
            sim.step()
    dev.barrier()
    elapsed = max(dev.allgather_scalars(time.perf_counter() - t0))      # max over ranks
    steps_per_s = args.steps / elapsed
    lists_after = dev.tile_list_stats() if lists_before else None
    flushed = False
    if args.dump_outputs:
        dump_outputs(sim.field_to_numpy(), args.dump_outputs)
        # (the download launched what a deferred pass still owed: the captured graph no longer starts from this state, --full steps on eagerly)
        flushed = sim._limit_pending() != sim._pending_after_step
    abytes, counts = algorithmic_bytes(mask, esize)
    out = {
        # BASELINE.json's metric string for the headline configuration; `value` is its steps/sec part, the Poisson-sweep
        # GB/s (% of the HBM roofline) part is in `poisson_jacobi_sweep` (and per kernel in `kernels`) of a --full run
        "metric": "simulation steps/sec + Poisson-sweep HBM GB/s (% roofline), res 4096\u00b2, 1/2/4/8 GPU"
                  if (res, args.bc, args.scheme, args.jacobi, args.dye, args.dtype) == (4096, 5, "cip", 0, False, "f32")
                  else f"simulation steps/sec (bc{args.bc} res {res} {args.scheme}{' jacobi' + str(args.jacobi) if args.jacobi else ''}{' +dye' if args.dye else ''}{' f64' if args.dtype == 'f64' else ''})",
        "value": round(steps_per_s, 3), "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 / steps_per_s, 4), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"bc={args.bc} res={res} ({2 * res}x{res} cells) scheme={args.scheme} vc={vc} "
                               f"{'Jacobi(' + str(args.jacobi) + ')' if args.jacobi else 'RB-SOR(1.3, 2 iters)'} Re={re:g} dt={'0.05/res' if not args.dt else args.dt}"
                               + ("; BASELINE.json configs[2]" if (res, args.bc, args.scheme, args.jacobi) == (4096, 5, "cip", 0) else ""),
                   "cells": counts["cells"], "fluid_cells": counts["fluid"], "parallelism": f"y-slab x{world}",
                   "launch": launch},
    }
    if not args.full:
        finish(dev, rdzv, rank, out)
        return

    # Short timed regions (the driver's --steps 20 is 16 ms of work) say little about the spread: for K < 120 another 120 steps follow in
    # blocks of the whole replay periods of K, each timed like the first, and min / median / max per step are reported NEXT TO the
    # contract's numbers (which stay the first block's).  The number of extra steps depends on K alone, so every mode and every N ends
    # after the same number of steps (state_checksum stays comparable).
    period = gperiod if graph is not None else (tape["nsteps"] if tape is not None else 1)

    def timed_block(nsteps):
        dev.barrier()
        t = time.perf_counter()
        if graph is not None:
            replay_graphs(nsteps)
        elif tape is not None:
            dev.replay_tape(tape, nsteps // period)
        else:
            for _ in range(nsteps):
                sim.step()
        dev.barrier()
        return max(dev.allgather_scalars(time.perf_counter() - t))
    spread = [1e3 * elapsed / args.steps]
    extra_steps = 0 if args.steps >= 120 else 120
    used = (period - (phase0 + args.steps) % period) % period          # finish the period the K steps ended in (eager, untimed)
    bsteps = max((args.steps // period) * period, period)
    if used <= extra_steps and not flushed:
        for _ in range(used):
            sim.step()
        while used + bsteps <= extra_steps:
            spread.append(1e3 * timed_block(bsteps) / bsteps)
            used += bsteps
    else:
        used = 0
    for _ in range(extra_steps - used):
        sim.step()
    spread.sort()
    blocks = spread
    for _ in range(later):
        sim.step()

    # ---- per-kernel durations with HIP events on the kernels' own stream (same K steps again) -------------
    sim.step()          # one eager step outside the measurement: launch geometries seen for the first time build their tile lists here
    dev.profile(True)
    dev.profile_reset()
    prof_steps = min(args.steps, 50)
    for _ in range(prof_steps):
        sim.step()
    rep = dev.profile_report()
    dev.profile(False)
    # order-independent exact checksum of the final state (sum of the f32 bit patterns mod 2^64 over the whole grid):
    # equal numbers from the --gpus 1/2/4/8 runs of the same command line mean the slab runs are bit-identical.
    total_steps = args.warmup + settle + args.steps + extra_steps + 1 + prof_steps
    checksum = {"after_steps": total_steps}
    for name, f in zip(("v", "p", "dye"), sim._solver.get_fields()):
        local = int(np.ascontiguousarray(f.to_numpy(local=True)).view(np.uint32).astype(np.uint64).sum(dtype=np.uint64))
        parts = [dev.allgather_scalars(float((local >> sh) & 0x1FFFFF)) for sh in (0, 21, 42, 63)]
        tot = sum(int(parts[k][r]) << sh for k, sh in enumerate((0, 21, 42, 63)) for r in range(world))
        checksum[name] = f"{tot & 0xFFFFFFFFFFFFFFFF:016x}"
    # Poisson residual of the final state (new diagnostic, not in the reference): wave-level reduction per slab + one
    # ncclAllReduce of 2 doubles over the node; rms over the not-wall cells of the global grid
    v_f, p_f = sim._solver.get_fields()[:2]
    r_sum, r_cnt = dev.poisson_residual(dt, dx, p_f, v_f)
    residual = {"rms": float(np.sqrt(r_sum / max(r_cnt, 1.0))), "cells": int(r_cnt)}
    # HBM bytes per launch from rocprofv3 PMC passes of this same workload (tools/profile.sh -> profiles/*.json), if present
    pmc_traffic, pmc_valu, traffic_source = {}, {}, None
    pmc_file = os.path.join(REPO, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc_file) and (res, args.bc, args.scheme, args.dye, args.dtype) == (4096, 5, "cip", False, "f32") and world == 1:
        # counters of ANOTHER run of this workload: quoted only when they were taken on the very library this process loaded (tools/profile.sh stamps
        # the file with the library's sha256); a kernel edited since then gives `traffic: null`, not a number that no longer belongs to it
        import hashlib
        pm = json.load(open(pmc_file))
        lib_sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
        if pm.get("lib_sha256") == lib_sha:
            pmc_traffic = pm.get("bytes_per_launch", {})
            pmc_valu = pm.get("valu_wave_insts_per_launch", {})
            traffic_source = ("profiles/pmc_traffic.json: rocprofv3 --pmc passes of this workload on this build of libfs_hip.so (sha256 " + lib_sha[:16] +
                              ", tools/profile.sh), NOT measured in this run")
        else:
            traffic_source = ("stale: profiles/pmc_traffic.json was taken on another build of libfs_hip.so (" + str(pm.get("lib_sha256"))[:16] + " != " + lib_sha[:16] +
                              "); re-run tools/profile.sh")
    parts = {}
    merge_parts(rep, parts)
    frac_rows = dev.nyl / dev.ny
    kernels = {}
    for name, (launches, ms) in rep.items():
        if launches == 0:
            continue
        avg_ms = ms / launches
        entry = {"launches_per_step": launches / prof_steps, "avg_us": round(avg_ms * 1e3, 2),
                 "share": round(ms / max(sum(m for _, m in rep.values()), 1e-12), 4)}
        if name in abytes:
            entry["alg_MB"] = round(abytes[name] * frac_rows / 1e6, 2)
            entry["GBps"] = round(abytes[name] * frac_rows / (avg_ms * 1e-3) / 1e9, 1)
            entry["frac"] = round(entry["GBps"] / HBM_PEAK_GBS, 4)
            if box:
                entry["frac_of_box_copy"] = round(entry["GBps"] / box["copy_GBps"], 4)
        if name in parts:        # the unmerged parts of a multi-part launch (per-launch HIP-event brackets of each)
            entry["parts_us"] = {k: round(v[1] / max(v[0], 1) * 1e3, 2) for k, v in parts[name].items()}
        kernels[name] = entry
    # The kernel `roofline` prices is chosen BY NAME (--roofline-kernel, default cip_step = the headline's dominant kernel), not by which launch
    # happened to take longest in this run: on small grids two kernels of ~10 us trade places from box to box (round 5's red GPU suite).
    priced = [k for k in kernels if "GBps" in kernels[k]]
    if args.roofline_kernel in priced:
        dominant, selection = args.roofline_kernel, f"--roofline-kernel {args.roofline_kernel}"
    else:
        dominant = max(priced, key=lambda k: kernels[k]["share"], default=None)
        selection = f"{args.roofline_kernel} is not launched by this workload: the kernel with the largest share of the profiled step"
    # the __global__ functions behind every profile name, as the library launched them (fs_prof_kernels: demangled symbols, what a kernel trace shows)
    if hasattr(dev, "profile_kernels"):
        for name in kernels:
            names = dev.profile_kernels(name) + [n_ for sfx in ("_bnd", "_band") for n_ in dev.profile_kernels(name + sfx)]
            if names:
                kernels[name]["gpu_kernels"] = names
    # slab runs: what an exchange costs in line (pack -> grouped RCCL send / recv -> unpack, one HIP-event span on the stream it is queued
    # on) against the longest kernel that could cover it if the exchange ran on the communication stream (FS_OVERLAP=1): the model the
    # overlap decision is taken from - not from a loop-back run, where the RCCL kernel competes with the compute kernels for the same CUs
    exchange_model = None
    if "halo_exchange" in kernels:
        ex = kernels["halo_exchange"]
        compute = {k: v for k, v in kernels.items() if k != "halo_exchange"}
        longest = max(compute, key=lambda k: compute[k]["avg_us"]) if compute else None
        chain_step = ex["avg_us"] * ex["launches_per_step"]
        exchange_model = {
            "chain_us": ex["avg_us"], "exchanges_per_step": ex["launches_per_step"], "chain_us_per_step": round(chain_step, 2),
            "compute_us_per_step": round(sum(v["avg_us"] * v["launches_per_step"] for v in compute.values()), 2),
            "longest_kernel": longest, "longest_kernel_us": compute[longest]["avg_us"] if longest else None,
            "coverable_us_per_step": round(min(ex["avg_us"], compute[longest]["avg_us"]) * ex["launches_per_step"], 2) if longest else 0.0,
            "overlap": "on (communication stream)" if dev.overlap_stream else "off (in line on the compute stream)",
            "trial": exchange_trial,
            "reading": "an exchange on the communication stream can hide at most min(chain, longest kernel) per exchange, and costs two more strip "
                       "launches and three stream hand-offs (~8 us each, DESIGN.md 6): worth it when coverable_us_per_step exceeds ~25 us x exchanges_per_step"}

    # ---- isolated Poisson Jacobi sweep (the roofline-graded kernel): S sweeps ping-ponging two p buffers ---
    # Two bit-identical forms: reading v like the reference, and reading the per-step precomputed source pair
    # (what JacobiPressureUpdater uses from 5 sweeps/step on).  Both move S = 8 source bytes per cell.
    jac = None
    if args.sweeps > 0:
        v, p = sim._solver.get_fields()
        pa, pb, src = dev.alloc(1), dev.alloc(1), dev.alloc(2)
        dev._p_upload(pa._h, 1, p.local_window(), dev.g_lo - (dev.y0 - dev.halo), dev.g_hi - dev.g_lo)   # this slab's rows of p
        pa.valid = 0
        dev.poisson_source(dt, dx, src, v)
        dev.profile_reset()
        dev.profile(True)
        for _ in range(args.sweeps // 2):
            dev.jacobi_sweep(dt, dx, pb, pa, v)
            dev.jacobi_sweep(dt, dx, pa, pb, v)
        for _ in range(args.sweeps // 2):
            dev.jacobi_sweep_src(pb, pa, src)
            dev.jacobi_sweep_src(pa, pb, src)
        if dev.lazy_bc_ok and world == 1:       # two sweeps per pass, K7 evaluated in registers (what Jacobi runs of 6+ sweeps issue)
            for k in range(args.sweeps // 2):
                dev.jacobi_pair_lazy(pb, pa, src, swapped=False)
                dev.jacobi_pair_lazy(pa, pb, src, swapped=True)
            if getattr(dev, "jacobi_quad_ok", False):   # four sweeps per pass (what Jacobi runs of 10+ sweeps issue where the mask admits it)
                for k in range(args.sweeps // 4):
                    dev.jacobi_quad_lazy(pb, pa, src)
                    dev.jacobi_quad_lazy(pa, pb, src)
        rj = merge_parts(dev.profile_report())
        dev.profile(False)
        # SURVEY.md 8d's definition - bytes / HIP-event time averaged over >= 200 consecutive sweeps: ONE event pair around the whole ping-pong
        # (launch boundaries between dependent sweeps included, no per-launch event records in between); the per-launch brackets above stay
        # next to it as `per_launch_*`
        span = {}
        if hasattr(dev, "span_begin") and world == 1:      # (slabs: the ghost-row exchanges between sweeps would be inside the span - the per-launch brackets there)
            for name, fn in (("jacobi_sweep", lambda a, b: dev.jacobi_sweep(dt, dx, a, b, v)), ("jacobi_sweep_src", lambda a, b: dev.jacobi_sweep_src(a, b, src))):
                fn(pb, pa); fn(pa, pb)
                dev.span_begin()
                for _ in range(args.sweeps // 2):
                    fn(pb, pa); fn(pa, pb)
                span[name] = dev.span_end() / (2 * (args.sweeps // 2)) * 1e-3        # seconds per sweep

        def leg(name, label):
            n_, ms_ = rj[name]
            per_launch_s = max(dev.allgather_scalars(ms_ / n_ * 1e-3))     # slowest slab
            avg_s = max(dev.allgather_scalars(span[name])) if name in span else per_launch_s
            slab_bytes = abytes[name] * frac_rows                     # PER DEVICE: this slab's share of the grid against ONE GPU's peak
            gbs = slab_bytes / avg_s / 1e9
            return {"kernel": label, "sweeps": n_, "avg_us": round(avg_s * 1e6, 2), "alg_MB": round(slab_bytes / 1e6, 2),
                    "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                    "timing": "one HIP-event pair around the whole ping-pong of sweeps (span / sweeps)" if name in span else "mean of per-launch HIP-event brackets",
                    "per_launch_avg_us": round(per_launch_s * 1e6, 2), "per_launch_frac": round(slab_bytes / per_launch_s / 1e9 / HBM_PEAK_GBS, 4),
                    "frac_of_box_copy": round(gbs / box["copy_GBps"], 4) if box else None,
                    "per": "device" if world > 1 else "grid", "traffic": pmc_traffic.get(name)}
        # The graded kernel first: the literal sweep that reads v like the reference (S = 8 B of source per cell).  Then the two build-side
        # forms with the same bits: the per-step precomputed source pair, and two sweeps per pass - each with what it amounts to per
        # REFERENCE sweep in SURVEY.md 8d's two accountings (S = 8: the sweep reads v or the pair (s2, s3); S = 4: a single fused source).
        s8 = abytes["jacobi_sweep"] * frac_rows
        s4 = (counts["cells"] + counts["not_wall"] * 3 * esize) * frac_rows

        def equiv(us_per_sweep):
            return {"per_sweep_equiv_frac_S8": round(s8 / (us_per_sweep * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                    "per_sweep_equiv_frac_S4": round(s4 / (us_per_sweep * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
        def gk(name):       # the __global__ function(s) the library launched under this profile name
            return dev.profile_kernels(name) if hasattr(dev, "profile_kernels") else []
        jac = leg("jacobi_sweep", "jacobi_sweep: reads p and v like fs/pressure_updater.py:62-66 (the literal sweep)")
        jac["gpu_kernels"] = gk("jacobi_sweep")
        jac.update(equiv(jac["avg_us"]))
        jac["source_pair_form"] = leg("jacobi_sweep_src", "jacobi_sweep_src: p + per-step precomputed source pair, same bits")
        jac["source_pair_form"]["gpu_kernels"] = gk("jacobi_sweep_src")
        jac["source_pair_form"].update(equiv(jac["source_pair_form"]["avg_us"]))
        if "jacobi_pair_lazy" in rj and rj["jacobi_pair_lazy"][0]:
            n_, ms_ = rj["jacobi_pair_lazy"]
            us = ms_ / n_ * 1e3
            two = {"kernel": "jacobi_pair_lazy: two sweeps + both pressure boundary passes per launch, first sweep in registers", "gpu_kernels": gk("jacobi_pair_lazy"),
                   "passes": n_, "avg_us": round(us, 2), "us_per_sweep": round(us / 2, 2), "alg_MB_per_pass": round(s8 / 1e6, 2),
                   "frac_of_one_pass_bytes": round(s8 / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
            two.update(equiv(us / 2))
            jac["two_sweeps_per_pass"] = two
        if "jacobi_quad_lazy" in rj and rj["jacobi_quad_lazy"][0]:
            n_, ms_ = rj["jacobi_quad_lazy"]
            us = ms_ / n_ * 1e3
            four = {"kernel": "jacobi_quad_lazy: four sweeps + the pressure boundary pass in front of each per launch, all in registers",
                    "gpu_kernels": gk("jacobi_quad_lazy") + gk("jacobi_quad_lazy_bnd"),
                    "passes": n_, "avg_us": round(us, 2), "us_per_sweep": round(us / 4, 2), "alg_MB_per_pass": round(s8 / 1e6, 2),
                    "frac_of_one_pass_bytes": round(s8 / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
            four.update(equiv(us / 4))
            jac["four_sweeps_per_pass"] = four

    out.update({
        "ms_per_step_min": round(spread[0], 4), "ms_per_step_median": round(spread[len(spread) // 2], 4),
        "ms_per_step_max": round(spread[-1], 4), "timed_blocks": len(blocks),
        "box": box,
        # compact launch lists (one hipMalloc + stream sync each, at the first launch of a geometry / slab row range): all built during the warm-up -
        # none inside the timed region, and no launch of the captured / taped period had to fall back to its dense grid
        "launch_lists": None if not lists_before else {"built_before_timed_region": lists_before[0], "built_in_timed_region": lists_after[0] - lists_before[0],
                                                       "dense_fallbacks": max(dev.allgather_scalars(float(lists_after[1])))},
        "state_checksum": checksum,
        "poisson_residual": residual,
        "exchange_model": exchange_model,
        "exchange_mode_trial": exchange_trial,
        "halo_exchanges_per_step": None if world == 1 else {
            "grouped_launches": round(dev.n_exchanges / max(total_steps, 1), 2),
            "fields": round(dev.n_exchanged_fields / max(total_steps, 1), 2),
            "KB_per_neighbour": round(dev.n_exchanged_bytes / max(total_steps, 1) / 1024, 1),
            "overlapped_fraction": round(dev.n_overlapped / max(dev.n_exchanges, 1), 2),
            "halo_rows": dev.halo},
    })
    if dominant:
        kd = kernels[dominant]
        if dominant in ("cip_grad_advect_rt", "cip_step"):
            # what the reference's launches (K3: 49 B/cell, K4: 49 B/cell; cip_step: + K2's 21) would have moved for the same result
            unfused = (abytes["cip_nonadv_grad"] + abytes["cip_advect"] + (abytes["cip_nonadv"] if dominant == "cip_step" else 0)) * frac_rows
            kd["unfused_equiv_MB"] = round(unfused / 1e6, 2)
            kd["unfused_equiv_frac"] = round(unfused / (kd["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        if dominant == "jacobi_pair_lazy":
            # the reference issues these two sweeps as 2 x (K7 + sweep): twice the sweep's bytes (K7's are negligible)
            kd["unfused_equiv_MB"] = round(2 * abytes[dominant] * frac_rows / 1e6, 2)
            kd["unfused_equiv_frac"] = round(2 * abytes[dominant] * frac_rows / (kd["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        out["roofline"] = {"kernel": dominant, "gpu_kernels": kd.get("gpu_kernels"), "selection": selection,
                           "bound": "hbm", "achieved": kd["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(kd["GBps"] / HBM_PEAK_GBS, 4), "frac_of_box_copy": kd.get("frac_of_box_copy"),
                           "traffic": pmc_traffic.get(dominant), "traffic_source": traffic_source,
                           "alg_bytes_per_launch": int(abytes[dominant] * frac_rows), "avg_us": kd["avg_us"]}
        if dominant == "cip_step" and "parts_us" not in kd:
            out["roofline"]["what"] = "K2 + K3 + K4 of the velocity over every tile in one launch (csrc/fs_k234.h); gpu_kernels names the instantiation that ran"
            if world == 1 and not args.dye and args.dtype == "f32" and hasattr(dev, "cip_step_tiles"):
                # diagnostic: the same step with one launch per KIND of tile (FS_FUSE_K2=1) on a second context - what the all-fluid body reaches on the bytes
                # of its own tiles (52 B per cell: it reads no mask), and what the masked body costs; `frac` above stays the one launch's
                try:
                    out["roofline"]["by_kind_of_tile"] = cip_step_by_kind(args, res, dt, dx, re, vc, esize, box)
                except Exception as e:      # (a diagnostic must not cost the line)
                    out["roofline"]["by_kind_of_tile"] = {"error": repr(e)[:200]}
        if "unfused_equiv_frac" in kd:
            out["roofline"]["note"] = (
                "two Jacobi sweeps (and both pressure boundary passes) per launch, the first sweep's rows in registers: `frac` counts what "
                "ONE pass has to move (p in, source pair in, p out); the reference's 2 x (K7 + sweep) move twice that"
                if dominant == "jacobi_pair_lazy" else
                ("K2 + K3 + K4 of the velocity as one logical launch (csrc/fs_k234.h; `gpu_kernels` lists what was launched for it): `frac` counts the bytes the step has to move through "
                 "it (mask 1 + 28 read + 24 written = 53 B per fluid cell); the reference's three kernels move 119 B per fluid cell for the same result"
                 if dominant == "cip_step" else
                 "fused gradient-update + advection pass: `frac` counts the bytes the fused kernel has to move "
                 "(mask 1 + 32 read + 24 written = 57 B per fluid cell); the reference's two kernels move 98 B per fluid cell for the same result"))
            out["roofline"]["unfused_equiv_frac"] = kd["unfused_equiv_frac"]
        if dominant in pmc_valu and box and box.get("valu_ginstr_per_simd"):
            # how much of the kernel's time the issue of its VALU instructions alone accounts for: SQ_INSTS_VALU of one launch of this workload on
            # this build (profiles/pmc_traffic.json, stamped) / 1024 SIMDs / what one SIMD of THIS box issues per second (measured in this run;
            # packed f32 instructions issue at the same rate, box.valu_pk_ginstr_per_simd)
            winst = float(pmc_valu[dominant])
            issue_us = winst / 1024.0 / (box["valu_ginstr_per_simd"] * 1e9) * 1e6
            out["roofline"]["valu_issue"] = {"wave_insts_per_launch": winst, "per_simd": round(winst / 1024.0), "box_ginstr_per_simd": box["valu_ginstr_per_simd"],
                                             "issue_us": round(issue_us, 1), "frac_of_kernel_time": round(issue_us / kd["avg_us"], 3),
                                             "note": "VALU wave-instructions of one launch (PMC, stamped file) / 1024 SIMDs / the box's measured issue rate"}
    if jac:
        out["poisson_jacobi_sweep"] = jac
    out["kernels"] = kernels
    if rank == 0 and world == 1 and not args.no_cpu:
        # algorithmic bytes of one step as launched (sum over the profiled kernels), for the CPU leg's GB/s
        step_bytes = sum(abytes[k] * kernels[k]["launches_per_step"] for k in kernels if k in abytes)
        out["cpu_baseline"] = cpu_baseline(args, create_scene_arrays(args.bc, res), sim, dt, step_bytes)
        if not (out["cpu_baseline"]["parity_in_run"]["bit_identical"] and all(out["cpu_baseline"]["parity_in_run"]["graded_sweep_vs_oracle"].values())):
            raise SystemExit("bench: GPU and CPU oracle disagree after the same steps from the same state: " + json.dumps(out["cpu_baseline"]))
    finish(dev, rdzv, rank, out)


def finish(dev, rdzv, rank, out):
    dev.barrier()
    dev.close()
    if rdzv is not None:
        rdzv.cleanup()
    if rank == 0:
        print(json.dumps(out), flush=True)      # the ONE line on stdout, after everything else is torn down


if __name__ == "__main__":
    main()
