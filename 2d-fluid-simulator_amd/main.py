#!/usr/bin/env python3
"""Headless counterpart of the reference's main.py (argparse flags of main.py:11-63, same defaults).

The reference opens a GGUI window and steps forever; here the loop runs `--steps` steps on the GPU and can
  * dump fields exactly like the reference's `d` key (main.py:129-132):  output/step_{step:06}.npz  with v, p[, dye]
  * write the visualisation the window would show (`-vis`, main.py:94-107) as PNG frames every `--frame-every` steps
  * write / read a full-state checkpoint (new: the reference cannot resume - its dump lacks the CIP gradient
    fields and the `next` buffers).
  * sample scalar flow diagnostics (energy, enstrophy, CFL, divergence, non-finite cells, pressure force on a body) into a CSV
    every `--stats-every` steps, and stop at the first non-finite sample (`--stop-on-nonfinite`, exit status 3).
  * record u, w, p at probe cells (`--probe x,y`) and the pressure force on a body (`--body`) every `--history-every` steps on the
    GPU, written to `--history-file` (.npz) at the end of the run.
  * average u, w, p and their second moments over time on the GPU (`--mean-every`, `--mean-start`), written to `--mean-file` (.npz) at
    the end of the run; the sums travel with `--save-state` / `--load-state`, so an average continues over restarts.
  * accumulate the harmonic content of u, w, p at given frequencies on the GPU (`--modes-freq f[,f2,...]`, `--modes-every`, `--modes-start`):
    mean, amplitude and phase per cell written to `--modes-file` (.npz) at the end of the run, the phase-averaged cycle of the first frequency
    as `--modes-frames N` images; the sums travel with `--save-state` / `--load-state`.
  * proper orthogonal decomposition of the flow by the method of snapshots (`--pod-snapshots M`, `--pod-every`, `--pod-start`, `--pod-modes K`):
    the last M sampled fields stay on the GPU, their Gram matrix is reduced there; energies, temporal coefficients and the first K modes are
    written to `--pod-file` (.npz) at the end of the run, with -vis (or --frame-every) the modes as `pod_mode_<k>.png`; the snapshots travel with
    `--save-state` / `--load-state`.
  * finite-time Lyapunov exponent fields from those resident snapshots (`--ftle forward|backward|both`, `--ftle-refine R`, `--ftle-substeps S`;
    needs `--pod-snapshots`): a lattice of particles is carried through the snapshots on the GPU, forwards or backwards in time; FTLE, final
    positions and statuses are written to `--ftle-file` (.npz) at the end of the run, with -vis (or --frame-every) also `ftle_<direction>.png`.
  * follow tracer particles on the GPU (`--tracers N`, `--tracer-line x0,y0,x1,y1,n`): pathlines (`--tracer-once`) or streaklines, written
    to `--tracer-file` (.npz) at the end of the run and every `--tracer-dump-every` steps, drawn into the `-vis` frames; the particle state
    travels with `--save-state` / `--load-state`.  `--tracer-sort-every K` sorts the particles by cell on the GPU every K steps (large sets
    stay fast; no result changes); `--tracer-fields` writes the per-cell particle count, age sum and residence time (`--tracer-fields-file`).
  * give the particles inertia (`--tracer-tau T[,T2,...]`: response times that cycle over the particles as size classes, `--tracer-gravity
    gx,gy`), count where they hit the walls (`--tracer-deposits`) and accumulate the per-cell occupancy over the run on the GPU
    (`--tracer-accumulate-every K`, `--tracer-accumulate-start S`); all of it travels with `--save-state` / `--load-state`.
  * identify and track the vortices (`--vortices-every N --vortex-threshold T`, `--vortex-criterion`, `--vortex-min-area`, `--vortex-max`):
    criterion, connected components and per-vortex integer records on the GPU (csrc/fs_vortex.h), written with the track id of every
    record to `--vortices-file` (.npz) at the end of the run; the samples travel with `--save-state` / `--load-state`
  * accumulate histograms of the flow over the fluid cells on the GPU (`--dist quantity:bins:lo:hi`, up to 4 times; `qa:ba:lo:hi,qb:bb:lo:hi`
    for a joint table; `--dist-every`, `--dist-start`, `--dist-box x0,y0,x1,y1`): integer counts (csrc/fs_dist.h), written to `--dist-file`
    (.npz) at the end of the run; the tables travel with `--save-state` / `--load-state`.
  * track the complete load on a body (`--body` with `--loads-every N`): pressure and viscous force, their moments about `--loads-center`,
    and the mean / rms pressure and wall shear of every face of the surface, gathered on the GPU and written to `--loads-file` (.npz) at
    the end of the run, with Cd, Cl, Cm, Cp and Cf when `--loads-ref U,L` gives the reference speed and length; the per-face sums and
    counters travel with `--save-state` / `--load-state`.
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import fs  # noqa: E402
from fs.fluid_simulator import DyeFluidSimulator, FluidSimulator  # noqa: E402

_STATE = ("v", "p", "vx", "vy", "dye", "dyex", "dyey")


def build_parser():
    p = argparse.ArgumentParser(description="Fluid Simulator (headless, MI355X)")
    p.add_argument("-bc", "--boundary_condition", type=int, choices=[1, 2, 3, 4, 5, 6], default=1, help="Boundary condition number")
    p.add_argument("-re", "--reynolds_num", type=float, default=1000000.0, help="Reynolds number")
    p.add_argument("-res", "--resolution", type=int, default=400, help="Resolution of y-axis")
    p.add_argument("-dt", "--time_step", type=float, default=0.0, help="Time step")
    p.add_argument("-vis", "--visualization", type=int, choices=[0, 1, 2, 3], default=0, help="Flow visualization type")
    p.add_argument("-vc", "--vorticity_confinement", type=float, default=5.0, help="Vorticity Confinement. 0.0 is disable.")
    p.add_argument("-scheme", "--advection_scheme", type=str, choices=["upwind", "kk", "cip"], default="cip", help="Advection Scheme")
    p.add_argument("-no_dye", "--no_dye", action="store_true", help="No dye calculation")
    p.add_argument("-cpu", "--cpu", action="store_true", help="accepted for compatibility; there is no CPU path (HIP only)")
    # headless additions
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--f64", action="store_true", help="double precision (the reference is f32 only)")
    p.add_argument("--dump-every", type=int, default=0, help="np.savez v, p[, dye] every N steps (reference key 'd')")
    p.add_argument("--frame-every", type=int, default=0, help="write the -vis image as PNG every N steps")
    p.add_argument("--graph", action="store_true",
                   help="replay the steps between two dumps / frames as a hipGraph (no Python between kernels; same results)")
    p.add_argument("--out", type=str, default="output")
    p.add_argument("--save-state", type=str, default=None, help="write a full-state checkpoint (.npz) after the last step")
    p.add_argument("--load-state", type=str, default=None, help="resume from a checkpoint written by --save-state")
    p.add_argument("--stats-every", type=int, default=0,
                   help="sample the flow diagnostics (FluidSimulator.flow_stats) at the first step and every N steps into --stats-file")
    p.add_argument("--stats-file", type=str, default=None, help="CSV of the samples: step,time,<keys> (default: <out>/stats.csv)")
    p.add_argument("--pressure", type=str, choices=["rbsor", "multigrid"], default=None,
                   help="pressure updater: rbsor - the reference's red-black SOR(1.3, 2), the default; multigrid - W-cycles around it "
                        "(fs.pressure_updater.MultigridPressureUpdater).  Given, --stats-every also writes a p_residual column")
    p.add_argument("--mg-cycles", type=int, default=None, help="W-cycles per step of --pressure multigrid (default 1)")
    p.add_argument("--mg-coarsest", type=str, choices=["sweeps", "direct"], default=None,
                   help="last level of --pressure multigrid: sweeps - 64 red-black sweeps where an extent turns odd, the default; direct - the "
                        "hierarchy is cut at a level of at most --mg-direct-cells cells and that level is solved exactly (converges at any even -res)")
    p.add_argument("--mg-direct-cells", type=int, default=None, help="cells of the level --mg-coarsest direct solves exactly (default 2048)")
    p.add_argument("--body", type=str, default=None,
                   help="x0,y0,x1,y1 (global cells, half-open): add the pressure force on the wall cells in this box to the samples "
                        "and the history; 'auto': the scene's obstacle (scenes 1, 3, 5, 6; fs.boundary_condition.default_body_box)")
    p.add_argument("--stop-on-nonfinite", action="store_true",
                   help="exit with status 3 at the first sample that finds NaN / Inf in v or p")
    p.add_argument("--history-every", type=int, default=0,
                   help="record the probes (--probe) and the body force (--body) after every N-th step on the GPU (FluidSimulator.record_history)")
    p.add_argument("--probe", type=str, action="append", default=[], metavar="X,Y",
                   help="a fluid cell (global x,y) whose u, w, p go into the history; may be repeated")
    p.add_argument("--history-file", type=str, default=None,
                   help=".npz of the history: step, time, probes, u, w, p[, force_x, force_y] (default: <out>/history.npz)")
    p.add_argument("--mean-every", type=int, default=0,
                   help="accumulate time averages of u, w, p and their second moments after every N-th step on the GPU "
                        "(FluidSimulator.start_averaging; 0: off)")
    p.add_argument("--mean-start", type=int, default=0, help="steps of the averaged run (restarts included) to leave out before the first sample")
    p.add_argument("--mean-file", type=str, default=None,
                   help=".npz of the averages: samples, steps, u, w, p, uu, ww, uw, p_rms, tke, mask, dt, dx, every, start "
                        "(default: <out>/mean.npz)")
    p.add_argument("--modes-freq", type=str, default=None, metavar="F[,F2,...]",
                   help="accumulate the harmonic content of u, w, p at these 1 to 4 frequencies (1 / simulated time) on the GPU "
                        "(FluidSimulator.start_modes); each must stay below the Nyquist limit f * N * dt < 0.5 of --modes-every N")
    p.add_argument("--modes-every", type=int, default=None, help="sample the modes after every N-th step (default 1)")
    p.add_argument("--modes-start", type=int, default=None, help="steps of the run (restarts included) to leave out before the first sample (default 0)")
    p.add_argument("--modes-file", type=str, default=None,
                   help=".npz of the modes: frequencies, mean_u / _w / _p, amplitude_u / _w / _p, phase_u / _w / _p, samples, steps, mask, dt, "
                        "dx, every, start (default: <out>/modes.npz)")
    p.add_argument("--modes-frames", type=int, default=0,
                   help="write N -vis images modes_phase_<i>.png of the phase-averaged flow over one period of the first frequency")
    p.add_argument("--pod-snapshots", type=int, default=0, metavar="M",
                   help="keep the last M (2 .. 64) sampled flow fields on the GPU and decompose them into POD modes at the end of the run "
                        "(FluidSimulator.start_pod; 0: off); 12 M bytes per cell in f32")
    p.add_argument("--pod-every", type=int, default=None, help="take a snapshot after every N-th step (default 1)")
    p.add_argument("--pod-start", type=int, default=None, help="steps of the run (restarts included) to leave out before the first snapshot (default 0)")
    p.add_argument("--pod-modes", type=int, default=None, metavar="K", help="modes written to --pod-file as fields (default 4)")
    p.add_argument("--pod-file", type=str, default=None,
                   help=".npz of the POD: energies, fraction, coefficients, gram, sample_steps, samples, steps, u, w, p (the first K modes, "
                        "(K, X, Y) each), mean_u / _w / _p, mask, dt, dx, every, start (default: <out>/pod.npz); "
                        "with -vis 0 / 1 / 2 given, or --frame-every, also the images pod_mode_<k>.png")
    p.add_argument("--dist", type=str, action="append", default=[], metavar="SPEC",
                   help="accumulate a histogram over the fluid cells on the GPU (FluidSimulator.start_distributions): SPEC is quantity:bins:lo:hi "
                        "with quantity one of u, w, p, speed, vorticity, q, swirl, bins 1 .. 4096 over [lo, hi); qa:ba:lo:hi,qb:bb:lo:hi is the "
                        "joint table of two quantities (ba * bb <= 4096); may be repeated up to 4 times")
    p.add_argument("--dist-every", type=int, default=None, help="sample after every N-th step (default 1)")
    p.add_argument("--dist-start", type=int, default=None, help="steps of the run (restarts included) to leave out before the first sample (default 0)")
    p.add_argument("--dist-box", type=str, default=None, metavar="X0,Y0,X1,Y1", help="cells of every --dist table, half-open (default: the whole grid)")
    p.add_argument("--dist-file", type=str, default=None,
                   help=".npz of the tables: per channel k c<k>.counts, c<k>.edges, c<k>.nan, c<k>.quantity, c<k>.box and c<k>.below / c<k>.above "
                        "(a joint one: c<k>.outside, c<k>.edges_b), then samples, sample_steps, every, start, dt, dx (default: <out>/dist.npz)")
    p.add_argument("--ftle", choices=("forward", "backward", "both"), default=None,
                   help="at the end of the run, carry a lattice of particles through the resident POD snapshots on the GPU (needs --pod-snapshots) and "
                        "write the finite-time Lyapunov exponent field (FluidSimulator.flow_map): backward marks the attracting structures - dye "
                        "streaks -, forward the repelling ones")
    p.add_argument("--ftle-refine", type=int, default=None, metavar="R", help="lattice nodes per cell and direction: 1, 2, 4 or 8 (default 1)")
    p.add_argument("--ftle-substeps", type=int, default=None, metavar="S", help="midpoint steps per snapshot interval, 1 .. 16 (default 1)")
    p.add_argument("--ftle-file", type=str, default=None,
                   help=".npz of the flow maps: ftle_<direction>, status_<direction>, x_<direction>, y_<direction> ((R X, R Y) each), span, "
                        "sample_steps, refine (default: <out>/ftle.npz); with -vis 0 / 1 / 2 given, or --frame-every, also the images "
                        "ftle_<direction>.png")
    p.add_argument("--tracers", type=int, default=0,
                   help="follow N tracer particles seeded at random in fluid cells (FluidSimulator.seed_tracers; 0: none unless --tracer-line)")
    p.add_argument("--tracer-seed", type=int, default=None, help="seed of the random generator behind --tracers (default 0)")
    p.add_argument("--tracer-line", type=str, action="append", default=[], metavar="X0,Y0,X1,Y1,N",
                   help="N tracer seeds on the line from (X0, Y0) to (X1, Y1), cell units; seeds that are not in a fluid cell are dropped; "
                        "may be repeated")
    p.add_argument("--tracer-once", action="store_true",
                   help="a particle that leaves, hits a wall or expires stays where it was (pathlines); default: it starts again at its seed "
                        "(streaklines)")
    p.add_argument("--tracer-max-age", type=int, default=None, help="a particle expires after this many steps (default 0: never)")
    p.add_argument("--tracer-file", type=str, default=None,
                   help=".npz of the particles after the last step: x, y, age, status, respawns, seeds, steps (default: <out>/tracers.npz)")
    p.add_argument("--tracer-dump-every", type=int, default=0, help="also write <out>/tracers_<step>.npz every N steps")
    p.add_argument("--tracer-sort-every", type=int, default=0,
                   help="sort the particles by cell on the GPU every K steps, which keeps the advance of large sets (from about 2^20 particles) "
                        "fast while the flow mixes them; changes no result.  32 measured best; below 16 --graph replays nothing (default 0: never)")
    p.add_argument("--tracer-fields", action="store_true",
                   help="write the per-cell particle count, age sum and residence time (count, age_sum, residence, step) after the last step, "
                        "and <out>/tracer_fields_<step>.npz next to every --tracer-dump-every dump")
    p.add_argument("--tracer-fields-file", type=str, default=None, help=".npz of --tracer-fields (default: <out>/tracer_fields.npz)")
    p.add_argument("--tracer-tau", type=str, default=None, metavar="T[,T2,...]",
                   help="inertial particles: response time(s) >= 0 in simulated time; several values cycle over the particles (size classes); "
                        "0: no inertia (FluidSimulator.seed_tracers(tau=...)); the particle files gain u, w, tau")
    p.add_argument("--tracer-gravity", type=str, default=None, metavar="GX,GY", help="gravity on the inertial particles, velocity per time (needs --tracer-tau)")
    p.add_argument("--tracer-deposits", action="store_true",
                   help="count the wall hits of the inertial particles per wall cell (needs --tracer-tau); written as `deposits` with --tracer-fields")
    p.add_argument("--tracer-accumulate-every", type=int, default=0,
                   help="accumulate the per-cell particle count and age sum on the GPU after every K-th step (FluidSimulator.accumulate_tracers); "
                        "written as occupancy, accumulated_age_sum, samples with --tracer-fields (default 0: off)")
    p.add_argument("--tracer-accumulate-start", type=int, default=None, help="steps to skip before --tracer-accumulate-every samples (default 0)")
    p.add_argument("--vortices-every", type=int, default=0, metavar="N",
                   help="identify the vortices after every N-th step on the GPU (FluidSimulator.track_vortices; 0: off); needs --vortex-threshold")
    p.add_argument("--vortex-threshold", type=float, default=None, metavar="T",
                   help="a cell belongs to a vortex where the criterion exceeds T (1 / time^2): a fraction of (U / L)^2 of the scene")
    p.add_argument("--vortex-criterion", choices=("q", "swirl", "vorticity"), default="q", help="the criterion field (default: q)")
    p.add_argument("--vortex-min-area", type=int, default=4, metavar="A", help="components of fewer cells are not recorded (default 4)")
    p.add_argument("--vortex-max", type=int, default=64, metavar="M", help="most records per sample, those of smallest label (default 64, at most 1024)")
    p.add_argument("--vortex-link", type=float, default=4.0, metavar="D", help="reach of the tracking between two samples, cells (default 4)")
    p.add_argument("--vortices-file", type=str, default=None,
                   help=".npz of the vortices: the arrays of FluidSimulator.vortices and the track id of every record (default: <out>/vortices.npz)")
    p.add_argument("--loads-every", type=int, default=0,
                   help="track the loads on the --body after every N-th step on the GPU (FluidSimulator.track_body): pressure + viscous "
                        "force, moments, per-face pressure and wall shear statistics (0: off)")
    p.add_argument("--loads-start", type=int, default=0, help="steps of the tracked run (restarts included) to leave out before the first sample")
    p.add_argument("--loads-center", type=str, default=None, metavar="X,Y", help="reference point of the moments, cell units (default: the body's centroid)")
    p.add_argument("--loads-ref", type=str, default=None, metavar="U,L",
                   help="reference speed and length (in the units of dx): adds cd, cl, cm, cp_mean, cf_mean to the loads file")
    p.add_argument("--loads-file", type=str, default=None,
                   help=".npz of the loads: the series of FluidSimulator.body_loads, the arrays of body_surface, center, box, re, dx "
                        "(default: <out>/loads.npz)")
    return p


def _npz_path(path):
    """np.savez appends '.npz' to a name without it; use the same name for writing and reading."""
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


def saved_mean(path):
    """(every, start) of the time average a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    return (int(z["mean.every"]), int(z["mean.start"])) if "mean.sums" in z.files else None


def load_mean(sim, path):
    """Restore the sums and counters of the checkpoint's time average into the attached one -> whether the checkpoint held any."""
    z = np.load(_npz_path(path))
    if "mean.sums" not in z.files:
        return False
    sim._averager.restore(z)
    return True


def saved_modes(path):
    """(frequencies, every, start) of the harmonic modes a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    if "modes.sums" not in z.files:
        return None
    return (tuple(float(f) for f in z["modes.frequencies"]), int(z["modes.every"]), int(z["modes.start"]))


def load_modes(sim, path):
    """Restore the planes, scalars and counters of the checkpoint's modes into the attached ones -> whether the checkpoint held any."""
    z = np.load(_npz_path(path))
    if "modes.sums" not in z.files:
        return False
    sim._moder.restore(z)
    return True


def saved_pod(path):
    """(snapshots, every, start) of the POD a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    if "pod.slots" not in z.files:
        return None
    return (int(z["pod.snapshots"]), int(z["pod.every"]), int(z["pod.start"]))


def load_pod(sim, path):
    """Restore the snapshots and counters of the checkpoint's POD into the attached one -> whether the checkpoint held any."""
    z = np.load(_npz_path(path))
    if "pod.slots" not in z.files:
        return False
    sim._podr.restore(z)
    return True


def pod_file_arrays(sim, n_modes):
    """The arrays of --pod-file: FluidSimulator.pod() and the first n_modes modes, downloaded from pod_fields()."""
    pod = sim.pod(n_modes)
    out = {k: np.asarray(pod[k]) for k in ("energies", "fraction", "coefficients", "gram", "sample_steps", "samples", "steps")}
    u, w, q = [], [], []
    for k in range(pod["coefficients"].shape[1]):
        v, p = sim.pod_fields(k)
        a = v.to_numpy()
        u.append(a[..., 0]); w.append(a[..., 1]); q.append(p.to_numpy())
    shape = (0,) + np.asarray(sim._solver._bc.mask).shape
    out["u"], out["w"], out["p"] = (np.stack(x) if x else np.zeros(shape) for x in (u, w, q))
    v, p = sim.pod_fields(None)
    a = v.to_numpy()
    out["mean_u"], out["mean_w"], out["mean_p"] = a[..., 0], a[..., 1], p.to_numpy()
    out["mask"] = np.asarray(sim._solver._bc.mask).copy()
    return out


def saved_loads(path):
    """(box, centre, every, start) of the body tracker a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    if "loads.sums" not in z.files:
        return None
    return (tuple(int(b) for b in z["loads.box"]), tuple(float(c) for c in z["loads.center"]), int(z["loads.every"]), int(z["loads.start"]))


def saved_vortices(path):
    """(criterion, threshold, every, min_area, max_vortices) of the vortex tracker a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    if "vortex.words" not in z.files:
        return None
    return (str(z["vortex.criterion"]), float(z["vortex.threshold"]), int(z["vortex.every"]), int(z["vortex.min_area"]), int(z["vortex.max_vortices"]))


def parse_dist(parser, specs, box, nx, ny):
    """The --dist flags -> the channel dicts of FluidSimulator.start_distributions, checked against a grid of (nx, ny) cells."""
    from fs.ride_ops import RideOps

    class _Grid:
        pass
    grid = _Grid()
    grid.nx, grid.ny = nx, ny
    if len(specs) > RideOps.DIST_MAX_CHANNELS:
        parser.error(f"--dist: at most {RideOps.DIST_MAX_CHANNELS} tables")
    if box is not None:
        try:
            box = tuple(int(c) for c in box.split(","))
            if len(box) != 4:
                raise ValueError
        except ValueError:
            parser.error(f"--dist-box {box}: expected X0,Y0,X1,Y1")
    chans = []
    for spec in specs:
        sides = []
        for side in spec.split(","):
            part = side.split(":")
            try:
                if len(part) != 4:
                    raise ValueError
                sides.append({"quantity": part[0], "bins": int(part[1]), "range": (float(part[2]), float(part[3]))})
            except ValueError:
                parser.error(f"--dist {spec}: expected quantity:bins:lo:hi, or two of them separated by a comma")
        if len(sides) > 2:
            parser.error(f"--dist {spec}: a joint table has two quantities")
        chan = dict(sides[0], box=box)
        if len(sides) == 2:
            chan["against"] = sides[1]
        try:
            RideOps.dist_channel(grid, chan)
        except ValueError as e:
            parser.error(f"--dist {spec}: {e}")
        chans.append(chan)
    return chans, [RideOps.dist_channel(grid, c) for c in chans]


def saved_dist(path):
    """(channels array, every, start) of the distributions a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    if "dist.tables" not in z.files:
        return None
    return (np.asarray(z["dist.channels"], np.float64), int(z["dist.every"]), int(z["dist.start"]))


def dist_flags(held):
    """The flags that continue the distributions of a checkpoint (saved_dist), for the refusal's message."""
    from fs.ride_ops import RideOps
    names = RideOps.DIST_QUANTITIES
    out = []
    for row in held[0]:
        side = f"{names[int(row[0])]}:{int(row[1])}:{float(row[2])!r}:{float(row[3])!r}"
        if row[4] >= 0:
            side += f",{names[int(row[4])]}:{int(row[5])}:{float(row[6])!r}:{float(row[7])!r}"
        out.append(f"--dist {side}")
    out.append("--dist-box " + ",".join(str(int(b)) for b in held[0][0][8:12]))
    return " ".join(out) + f" --dist-every {held[1]} --dist-start {held[2]}"


def load_dist(sim, path):
    """Restore the tables and counters of the checkpoint's distributions into the attached ones -> whether the checkpoint held any."""
    z = np.load(_npz_path(path))
    if "dist.tables" not in z.files:
        return False
    sim._distr.restore(z)
    return True


def dist_file_arrays(sim):
    """The arrays of --dist-file from FluidSimulator.distributions()."""
    out = {}
    for k, d in enumerate(sim.distributions()):
        for name in ("counts", "edges", "edges_b", "below", "above", "outside", "nan", "quantity", "box"):
            if name in d:
                out[f"c{k}.{name}"] = np.asarray(d[name])
        out["samples"], out["sample_steps"] = np.array(d["samples"]), d["sample_steps"]
    return out


def _lib_error():
    from fs._lib import FsError
    return (FsError, ValueError)


def load_loads(sim, path):
    """Restore the per-face sums and counters of the checkpoint's body tracker into the attached one -> whether the checkpoint held any."""
    z = np.load(_npz_path(path))
    if "loads.sums" not in z.files:
        return False
    sim._tracker.restore(z)
    return True


def saved_tracers(path):
    """(respawn, max_age, N) of the tracer set a checkpoint holds, or None."""
    z = np.load(_npz_path(path))
    return (bool(z["tracer.respawn"]), int(z["tracer.max_age"]), len(z["tracer.x"])) if "tracer.x" in z.files else None


def saved_inertial(path):
    """What a checkpoint's tracer set holds beyond a passive one's: {"tau": (N,) array or None, "gravity": (gx, gy), "deposits": bool,
    "accumulate": (every, start) or None}, or None without a tracer set."""
    z = np.load(_npz_path(path))
    if "tracer.x" not in z.files:
        return None
    inertial = "tracer.tau" in z.files
    return {"tau": np.asarray(z["tracer.tau"], np.float64) if inertial else None,
            "gravity": tuple(float(g) for g in z["tracer.gravity"]) if inertial else (0.0, 0.0),
            "deposits": "tracer.deposits" in z.files,
            "accumulate": (int(z["tracer.accum.every"]), int(z["tracer.accum.start"])) if "tracer.accum.occupancy" in z.files else None}


def tracer_taus(values, n):
    """--tracer-tau's values cycled over n particles (size classes): particle k has values[k % len(values)]."""
    return np.resize(np.asarray(values, np.float64), n)


def load_tracers(sim, path, sort_every=0, accumulate=None):
    """Seed the checkpoint's tracer set and restore its state -> whether the checkpoint held one.  The state is in seed order: whether the
    run that wrote it sorted its particles, and whether this one will (sort_every), makes no difference.  An inertial set comes back with
    its response times, gravity, particle velocities and deposit plane; accumulate = (every, start): the accumulation is attached and, when
    the checkpoint holds one, continued."""
    z = np.load(_npz_path(path))
    if "tracer.x" not in z.files:
        return False
    inertial = {}
    if "tracer.tau" in z.files:
        inertial = {"tau": z["tracer.tau"], "gravity": tuple(float(g) for g in z["tracer.gravity"]), "deposits": "tracer.deposits" in z.files}
    sim.seed_tracers(z["tracer.seeds"], respawn=bool(z["tracer.respawn"]), max_age=int(z["tracer.max_age"]), sort_every=sort_every, **inertial)
    sim._tracers.restore(z)
    if accumulate is not None:
        sim.accumulate_tracers(every=accumulate[0], start_step=accumulate[1])
        sim._tracers.accumulation.restore(z)        # (nothing when the checkpoint holds none: a fresh accumulation)
    return True


def tracer_state_arrays(tr):
    """The checkpoint's arrays for a tracer set (fs.tracers.Tracers.checkpoint)."""
    return tr.checkpoint()


def tracer_seeds(mask, n_random, rng_seed, lines):
    """The seeds the flags ask for: --tracers N random ones, then every --tracer-line (x0, y0, x1, y1, n) without the points that do not
    lie in a fluid cell -> (seeds (N, 2), messages about dropped points)."""
    from fs.tracers import fluid_only, seed_line, seed_random
    parts, notes = [], []
    if n_random > 0:
        parts.append(seed_random(mask, n_random, rng_seed))
    for x0, y0, x1, y1, n in lines:
        kept, dropped = fluid_only(mask, seed_line((x0, y0), (x1, y1), n))
        if dropped:
            notes.append(f"--tracer-line {x0:g},{y0:g},{x1:g},{y1:g},{n}: dropped {dropped} of {n} seeds (not in a fluid cell)")
        parts.append(kept)
    return (np.concatenate(parts) if parts else np.zeros((0, 2))), notes


def save_state(sim, path, step):
    s = sim._solver
    arrays = {"step": np.array(step)}
    for rider in sim._riders():
        arrays.update(rider.checkpoint())       # (a history recorder has nothing to resume: its records are written as they come)
    for name in _STATE:
        if hasattr(s, name):
            arrays[f"{name}.current"] = getattr(s, name).current.to_numpy()
            arrays[f"{name}.next"] = getattr(s, name).next.to_numpy()
    vc = s.vorticity_confinement
    if vc is not None:
        arrays["vorticity"] = vc.vorticity.to_numpy()
        arrays["vorticity_abs"] = vc.vorticity_abs.to_numpy()
    np.savez(_npz_path(path), **arrays)


def load_state(sim, path):
    s = sim._solver
    z = np.load(_npz_path(path))
    for name in _STATE:
        if hasattr(s, name):
            getattr(s, name).current.from_numpy(z[f"{name}.current"])
            getattr(s, name).next.from_numpy(z[f"{name}.next"])
    vc = s.vorticity_confinement
    if vc is not None and "vorticity" in z:
        vc.vorticity.from_numpy(z["vorticity"])
        vc.vorticity_abs.from_numpy(z["vorticity_abs"])
    return int(z["step"])


def mean_frame(sim, vis):
    """The -vis 0 / 1 / 2 image of the mean flow (FluidSimulator.mean_fields), downloaded as an (X, Y, 3) array."""
    return fields_frame(sim, vis, *sim.mean_fields())


def modes_file_arrays(modes):
    """The arrays of --modes-file from FluidSimulator.modes()."""
    out = {"frequencies": modes["frequencies"], "samples": np.array(modes["samples"]), "steps": np.array(modes["steps"]), "mask": modes["mask"]}
    for name in ("u", "w", "p"):
        out[f"mean_{name}"], out[f"amplitude_{name}"], out[f"phase_{name}"] = modes[name]["mean"], modes[name]["amplitude"], modes[name]["phase"]
    return out


def fields_frame(sim, vis, v, p):
    """The -vis 0 / 1 / 2 image of the flow in the fields v, p, downloaded as an (X, Y, 3) array."""
    dev = sim._dev
    if vis == 0:
        dev.vis_norm(sim.rgb_buf, v, p)
    elif vis == 1:
        dev.vis_pressure(sim.rgb_buf, p)
    else:
        dev.vis_vorticity(sim._solver.dx, sim.rgb_buf, v)
    return sim.rgb_buf.to_numpy()


def save_png(img, path):
    from PIL import Image
    img = np.clip(img, 0.0, 1.0)
    Image.fromarray((np.flip(img.transpose(1, 0, 2), axis=0) * 255).astype(np.uint8)).save(path)


def frame(sim, vis):
    """The image the reference's window would show (main.py:93-107), with the tracer particles on top when there are any, downloaded as an
    (X, Y, 3) array."""
    if vis == 0:
        img = sim.get_norm_field()
    elif vis == 1:
        img = sim.get_pressure_field()
    elif vis == 2:
        img = sim.get_vorticity_field()
    else:
        img = sim.get_dye_field()
    if getattr(sim, "_tracers", None) is not None:
        sim.draw_tracers(img)
    return img.to_numpy()


class StatsWriter:
    """--stats-every: one CSV row per sample (step, simulated time, the keys of FluidSimulator.flow_stats; floats at full precision)."""

    def __init__(self, sim, path, dt, box, stop_on_nonfinite, p_residual=False):
        self.sim, self.dt, self.box, self.stop = sim, dt, box, stop_on_nonfinite
        self.p_residual = p_residual      # --pressure given: one more column, FluidSimulator.pressure_residual
        path.parent.mkdir(parents=True, exist_ok=True)
        self.fh = open(path, "w")
        self.keys = None

    def sample(self, step):
        """Write one row -> the number of non-finite cells found."""
        d = self.sim.flow_stats(self.box)
        if self.p_residual:
            d["p_residual"] = self.sim.pressure_residual()
        if self.keys is None:
            self.keys = list(d)
            self.fh.write(",".join(["step", "time"] + self.keys) + "\n")
        self.fh.write(",".join([str(step), repr(step * self.dt)] + [repr(d[k]) for k in self.keys]) + "\n")
        self.fh.flush()
        return d["nonfinite"]

    def close(self):
        self.fh.close()


def _body_box(parser, spec, num, res):
    if spec is None:
        return None
    if spec == "auto":
        from fs.boundary_condition import default_body_box
        try:
            return default_body_box(num, res)
        except ValueError as e:
            parser.error(f"--body auto: {e}")
    try:
        box = tuple(int(x) for x in spec.split(","))
    except ValueError:
        box = ()
    if len(box) != 4 or not (0 <= box[0] <= box[2] <= 2 * res and 0 <= box[1] <= box[3] <= res):
        parser.error(f"--body {spec}: expected x0,y0,x1,y1 with 0 <= x0 <= x1 <= {2 * res} and 0 <= y0 <= y1 <= {res}, or 'auto'")
    return box


def _tracer_line(parser, spec):
    c = spec.split(",")
    try:
        x0, y0, x1, y1, n = float(c[0]), float(c[1]), float(c[2]), float(c[3]), int(c[4])
        if len(c) != 5 or n < 1:
            raise ValueError
    except (ValueError, IndexError):
        parser.error(f"--tracer-line {spec}: expected x0,y0,x1,y1,n (cell units, n >= 1)")
    return x0, y0, x1, y1, n


def _tracer_floats(parser, flag, spec, count=None):
    try:
        vals = [float(c) for c in spec.split(",")]
        if not vals or (count is not None and len(vals) != count) or not all(np.isfinite(v) for v in vals):
            raise ValueError
    except ValueError:
        parser.error(f"{flag} {spec}: expected {'%d finite numbers' % count if count else 'finite numbers'} separated by commas")
    return vals


def _probe(parser, spec):
    try:
        x, y = (int(c) for c in spec.split(","))
    except ValueError:
        parser.error(f"--probe {spec}: expected x,y (global cell)")
    return x, y


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    vis_given = any(a in ("-vis", "--visualization") or a.startswith("--visualization=") for a in (sys.argv[1:] if argv is None else argv))
    if args.cpu:
        print("note: -cpu ignored; this build runs on the GPU only", file=sys.stderr)
    res = args.resolution
    dt = args.time_step if args.time_step != 0.0 else 0.05 / res
    dx = 1 / res
    vor_eps = args.vorticity_confinement if args.vorticity_confinement != 0.0 else None
    enable_dye = not args.no_dye
    if args.visualization == 3 and not enable_dye:
        raise SystemExit("-vis 3 (dye) needs dye transport (drop -no_dye)")
    if args.boundary_condition == 6:
        from fs.boundary_condition import _find_obstacle_image
        try:
            _find_obstacle_image()
        except FileNotFoundError as e:      # the obstacle image is an asset of the reference repository and is not shipped here
            parser.error(f"-bc 6: {e}")
    if (args.stop_on_nonfinite or args.stats_file) and args.stats_every <= 0:
        parser.error("--stats-file and --stop-on-nonfinite need --stats-every N")
    if args.mg_cycles is not None and (args.pressure != "multigrid" or args.mg_cycles < 1):
        parser.error("--mg-cycles N needs --pressure multigrid and N >= 1")
    if args.mg_coarsest is not None and args.pressure != "multigrid":
        parser.error("--mg-coarsest needs --pressure multigrid")
    if args.mg_direct_cells is not None and (args.pressure != "multigrid" or args.mg_direct_cells < 1):
        parser.error("--mg-direct-cells N needs --pressure multigrid and N >= 1")
    if args.pressure == "multigrid" and res % 2:
        parser.error("--pressure multigrid needs an even -res (no coarse level otherwise)")
    if args.body is not None and args.stats_every <= 0 and args.history_every <= 0 and args.loads_every <= 0:
        parser.error("--body needs --stats-every N, --history-every N or --loads-every N")
    if args.vortices_every < 0:
        parser.error("--vortices-every must be >= 0")
    if args.vortices_every > 0 and (args.vortex_threshold is None or not np.isfinite(args.vortex_threshold)):
        parser.error("--vortices-every needs a finite --vortex-threshold T (1 / time^2)")
    if args.vortices_every > 0 and not (1 <= args.vortex_max <= 1024 and args.vortex_min_area >= 1 and args.vortex_link >= 0.0):
        parser.error("--vortex-max must be 1 .. 1024, --vortex-min-area >= 1 and --vortex-link >= 0")
    if (args.vortex_threshold is not None or args.vortices_file) and args.vortices_every <= 0:
        parser.error("--vortex-threshold and --vortices-file need --vortices-every N")
    if args.loads_every < 0 or args.loads_start < 0:
        parser.error("--loads-every and --loads-start must be >= 0")
    if (args.loads_start or args.loads_center or args.loads_ref or args.loads_file) and args.loads_every <= 0:
        parser.error("--loads-start, --loads-center, --loads-ref and --loads-file need --loads-every N")
    if args.loads_every > 0 and args.body is None:
        parser.error("--loads-every needs --body")
    loads_center = tuple(_tracer_floats(parser, "--loads-center", args.loads_center, 2)) if args.loads_center else None
    loads_ref = tuple(_tracer_floats(parser, "--loads-ref", args.loads_ref, 2)) if args.loads_ref else None
    if loads_ref is not None and (loads_ref[0] == 0.0 or loads_ref[1] <= 0.0):
        parser.error(f"--loads-ref {args.loads_ref}: the speed must not be 0 and the length must be > 0")
    if (args.probe or args.history_file) and args.history_every <= 0:
        parser.error("--probe and --history-file need --history-every N")
    if args.history_every > 0 and not args.probe and args.body is None:
        parser.error("--history-every needs --probe X,Y or --body")
    if args.mean_every < 0 or args.mean_start < 0:
        parser.error("--mean-every and --mean-start must be >= 0")
    if (args.mean_start or args.mean_file) and args.mean_every <= 0:
        parser.error("--mean-start and --mean-file need --mean-every N")
    if args.mean_every > 0 and args.load_state:
        held = saved_mean(args.load_state)
        if held is not None and held != (args.mean_every, args.mean_start):
            print(f"--load-state {args.load_state}: its time average was taken with --mean-every {held[0]} --mean-start {held[1]}, "
                  f"not {args.mean_every} / {args.mean_start}; continue with those or average without the checkpoint's sums", file=sys.stderr)
            sys.exit(2)
    modes_freqs = None
    if args.modes_freq is None:
        if args.modes_every is not None or args.modes_start is not None or args.modes_file or args.modes_frames:
            parser.error("--modes-every, --modes-start, --modes-file and --modes-frames need --modes-freq F")
    else:
        from fs.modes import phasor_steps
        modes_freqs = _tracer_floats(parser, "--modes-freq", args.modes_freq)
        modes_every, modes_start = (1 if args.modes_every is None else args.modes_every), args.modes_start or 0
        if modes_every < 1 or modes_start < 0 or args.modes_frames < 0:
            parser.error("--modes-every must be >= 1, --modes-start and --modes-frames >= 0")
        if args.modes_frames and args.visualization == 3:
            parser.error("--modes-frames: -vis 3 is the dye, which has no modes (use -vis 0, 1 or 2)")
        try:
            phasor_steps(modes_freqs, modes_every, dt)
        except ValueError as e:
            parser.error(f"--modes-freq {args.modes_freq}: {e}")
        if args.load_state:
            held = saved_modes(args.load_state)
            if held is not None and held != (tuple(modes_freqs), modes_every, modes_start):
                print(f"--load-state {args.load_state}: its modes were taken with --modes-freq {','.join(repr(f) for f in held[0])} --modes-every "
                      f"{held[1]} --modes-start {held[2]}; continue with those or accumulate without the checkpoint's sums", file=sys.stderr)
                sys.exit(2)
    pod_every, pod_start, pod_modes = (1 if args.pod_every is None else args.pod_every), args.pod_start or 0, (4 if args.pod_modes is None else args.pod_modes)
    if args.pod_snapshots == 0:
        if args.pod_every is not None or args.pod_start is not None or args.pod_modes is not None or args.pod_file:
            parser.error("--pod-every, --pod-start, --pod-modes and --pod-file need --pod-snapshots M")
    else:
        if not 2 <= args.pod_snapshots <= 64:
            parser.error("--pod-snapshots must be 2 .. 64")
        if pod_every < 1 or pod_start < 0 or pod_modes < 0:
            parser.error("--pod-every must be >= 1, --pod-start and --pod-modes >= 0")
        if args.load_state:
            held = saved_pod(args.load_state)
            if held is not None and held != (args.pod_snapshots, pod_every, pod_start):
                print(f"--load-state {args.load_state}: its POD snapshots were taken with --pod-snapshots {held[0]} --pod-every {held[1]} --pod-start "
                      f"{held[2]}; continue with those or sample without the checkpoint's snapshots", file=sys.stderr)
                sys.exit(2)
    dist_every, dist_start = (1 if args.dist_every is None else args.dist_every), args.dist_start or 0
    dist_channels = None
    if not args.dist:
        if args.dist_every is not None or args.dist_start is not None or args.dist_box or args.dist_file:
            parser.error("--dist-every, --dist-start, --dist-box and --dist-file need --dist SPEC")
    else:
        if dist_every < 1 or dist_start < 0:
            parser.error("--dist-every must be >= 1 and --dist-start >= 0")
        dist_channels, checked = parse_dist(parser, args.dist, args.dist_box, 2 * res, res)
        if args.load_state:
            held = saved_dist(args.load_state)
            from fs.dist import channels_array
            mine = channels_array(checked)
            if held is not None and (held[0].shape != mine.shape or not np.array_equal(held[0], mine) or held[1:] != (dist_every, dist_start)):
                print(f"--load-state {args.load_state}: its distributions were accumulated with {dist_flags(held)}; continue with those or "
                      "accumulate without the checkpoint's tables", file=sys.stderr)
                sys.exit(2)
    ftle_refine, ftle_substeps = (1 if args.ftle_refine is None else args.ftle_refine), (1 if args.ftle_substeps is None else args.ftle_substeps)
    if args.ftle is None:
        if args.ftle_refine is not None or args.ftle_substeps is not None or args.ftle_file:
            parser.error("--ftle-refine, --ftle-substeps and --ftle-file need --ftle forward|backward|both")
    else:
        if args.pod_snapshots == 0:
            parser.error("--ftle needs --pod-snapshots M: the flow map is integrated through the resident snapshots")
        if ftle_refine not in (1, 2, 4, 8) or not 1 <= ftle_substeps <= 16:
            parser.error("--ftle-refine must be 1, 2, 4 or 8 and --ftle-substeps 1 .. 16")
    tracing = args.tracers > 0 or bool(args.tracer_line)
    if args.tracers < 0 or args.tracer_dump_every < 0 or (args.tracer_max_age is not None and args.tracer_max_age < 0) or args.tracer_sort_every < 0:
        parser.error("--tracers, --tracer-max-age, --tracer-dump-every and --tracer-sort-every must be >= 0")
    if not tracing and (args.tracer_seed is not None or args.tracer_once or args.tracer_max_age is not None or args.tracer_file
                        or args.tracer_dump_every):
        parser.error("--tracer-seed, --tracer-once, --tracer-max-age, --tracer-file and --tracer-dump-every need --tracers N or --tracer-line")
    if not tracing and (args.tracer_sort_every or args.tracer_fields or args.tracer_fields_file):
        parser.error("--tracer-sort-every, --tracer-fields and --tracer-fields-file need --tracers N or --tracer-line")
    if args.tracer_fields_file and not args.tracer_fields:
        parser.error("--tracer-fields-file needs --tracer-fields")
    if not tracing and (args.tracer_tau is not None or args.tracer_gravity is not None or args.tracer_deposits or args.tracer_accumulate_every
                        or args.tracer_accumulate_start is not None):
        parser.error("--tracer-tau, --tracer-gravity, --tracer-deposits, --tracer-accumulate-every and --tracer-accumulate-start need --tracers N "
                     "or --tracer-line")
    if args.tracer_tau is None and (args.tracer_gravity is not None or args.tracer_deposits):
        parser.error("--tracer-gravity and --tracer-deposits need --tracer-tau (0 for particles without inertia)")
    if args.tracer_accumulate_every < 0 or (args.tracer_accumulate_start is not None and args.tracer_accumulate_start < 0):
        parser.error("--tracer-accumulate-every and --tracer-accumulate-start must be >= 0")
    if args.tracer_accumulate_start is not None and not args.tracer_accumulate_every:
        parser.error("--tracer-accumulate-start needs --tracer-accumulate-every K")
    taus = _tracer_floats(parser, "--tracer-tau", args.tracer_tau) if args.tracer_tau is not None else None
    if taus is not None and min(taus) < 0:
        parser.error(f"--tracer-tau {args.tracer_tau}: response times must be >= 0")
    gravity = tuple(_tracer_floats(parser, "--tracer-gravity", args.tracer_gravity, 2)) if args.tracer_gravity is not None else (0.0, 0.0)
    accumulate = (args.tracer_accumulate_every, args.tracer_accumulate_start or 0) if args.tracer_accumulate_every else None
    lines = [_tracer_line(parser, spec) for spec in args.tracer_line]
    max_age = args.tracer_max_age or 0
    if tracing and args.load_state:
        held = saved_tracers(args.load_state)
        if held is not None and held[:2] != (not args.tracer_once, max_age):
            print(f"--load-state {args.load_state}: its tracers ran with{'out' if held[0] else ''} --tracer-once and --tracer-max-age {held[1]}; "
                  "continue with those or drop the tracer flags", file=sys.stderr)
            sys.exit(2)
        more = saved_inertial(args.load_state)
        if more is not None:
            want_tau = tracer_taus(taus, held[2]) if taus is not None else None
            same_tau = (want_tau is None) == (more["tau"] is None) and (want_tau is None or np.array_equal(want_tau, more["tau"]))
            if not same_tau or more["gravity"] != gravity or more["deposits"] != bool(args.tracer_deposits):
                was = "passive tracers" if more["tau"] is None else (f"inertial tracers (--tracer-tau of {len(np.unique(more['tau']))} value(s), "
                                                                     f"--tracer-gravity {more['gravity'][0]:g},{more['gravity'][1]:g}, "
                                                                     f"with{'' if more['deposits'] else 'out'} --tracer-deposits)")
                print(f"--load-state {args.load_state}: it holds {was}; continue with those flags or drop the tracer flags", file=sys.stderr)
                sys.exit(2)
            if more["accumulate"] is not None and more["accumulate"] != accumulate:
                now = "no accumulation" if accumulate is None else f"{accumulate[0]} / {accumulate[1]}"
                print(f"--load-state {args.load_state}: it holds an occupancy accumulated with --tracer-accumulate-every {more['accumulate'][0]} "
                      f"--tracer-accumulate-start {more['accumulate'][1]}, not {now}; continue with those flags (the sums would be lost otherwise) "
                      "or drop the tracer flags", file=sys.stderr)
                sys.exit(2)
    box = _body_box(parser, args.body, args.boundary_condition, res)
    probes = [_probe(parser, spec) for spec in args.probe]
    print(f"Boundary Condition: {args.boundary_condition}\ndt: {dt}\nRe: {args.reynolds_num}\nResolution: {res}\n"
          f"Scheme: {args.advection_scheme}\nVorticity confinement: {vor_eps}")
    fs.runtime.init(gpu=args.gpu, dtype="f64" if args.f64 else "f32")
    cls = DyeFluidSimulator if enable_dye else FluidSimulator
    updater = None      # (the reference's red-black SOR(1.3, 2))
    if args.pressure == "multigrid":
        mg_kw = {k: v for k, v in (("coarsest", args.mg_coarsest), ("direct_cells", args.mg_direct_cells)) if v is not None}
        updater = ("multigrid", args.mg_cycles or 1) + ((mg_kw,) if mg_kw else ())
    sim = cls.create(args.boundary_condition, res, dt, dx, args.reynolds_num, vor_eps, args.advection_scheme, pressure_updater=updater)
    out = Path(args.out)
    step0 = load_state(sim, args.load_state) if args.load_state else 0
    dev = sim._solver._bc.device
    history_file = None
    if args.history_every > 0:
        history_file = Path(args.history_file) if args.history_file else out / "history.npz"
        try:
            sim.record_history(probes, box, every=args.history_every, start_step=step0)
        except ValueError as e:
            parser.error(f"--probe: {e}")

    def write_history():
        if history_file is not None:
            history_file.parent.mkdir(parents=True, exist_ok=True)
            np.savez(str(history_file), **sim.history())

    mean_file = None
    if args.mean_every > 0:
        mean_file = Path(args.mean_file) if args.mean_file else out / "mean.npz"
        sim.start_averaging(every=args.mean_every, start_step=args.mean_start)
        if args.load_state and load_mean(sim, args.load_state):
            print(f"time average: continuing the checkpoint's ({sim._dev.mean_read(sim._averager.mean)[2]} samples so far)")

    def write_mean():
        if mean_file is None:
            return
        try:
            avg = sim.averages()
        except RuntimeError as e:
            print(f"time average: {e}; no file written", file=sys.stderr)
            return
        mean_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(mean_file), dt=np.array(dt), dx=np.array(dx), every=np.array(args.mean_every), start=np.array(args.mean_start), **avg)
        if args.frame_every and args.visualization != 3:      # (-vis 3 is the dye: it is not averaged)
            out.mkdir(exist_ok=True)
            save_png(mean_frame(sim, args.visualization), out / "mean_vis.png")

    modes_file = None
    if modes_freqs is not None:
        modes_file = Path(args.modes_file) if args.modes_file else out / "modes.npz"
        sim.start_modes(modes_freqs, every=modes_every, start_step=modes_start)
        if args.load_state and load_modes(sim, args.load_state):
            print(f"modes: continuing the checkpoint's ({sim._dev.modes_read_scalars(sim._moder.modes)[3]} samples so far)")

    def write_modes():
        if modes_file is None:
            return
        try:
            modes = sim.modes()
        except RuntimeError as e:
            print(f"modes: {e}; no file written", file=sys.stderr)
            return
        modes_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(modes_file), dt=np.array(dt), dx=np.array(dx), every=np.array(modes_every), start=np.array(modes_start),
                 **modes_file_arrays(modes))
        if args.modes_frames:
            out.mkdir(exist_ok=True)
            for i in range(args.modes_frames):
                v, p = sim.mode_fields(2.0 * np.pi * i / args.modes_frames, 0)
                save_png(fields_frame(sim, args.visualization, v, p), out / f"modes_phase_{i}.png")

    pod_file = None
    if args.pod_snapshots:
        pod_file = Path(args.pod_file) if args.pod_file else out / "pod.npz"
        sim.start_pod(args.pod_snapshots, every=pod_every, start_step=pod_start)
        if args.load_state and load_pod(sim, args.load_state):
            print(f"POD: continuing the checkpoint's ({sim._dev.pod_read(sim._podr.pod)[1]} samples so far)")

    def write_pod():
        if pod_file is None:
            return
        try:
            arrays = pod_file_arrays(sim, pod_modes)
        except (RuntimeError, ValueError) as e:
            print(f"POD: {e}; no file written", file=sys.stderr)
            return
        pod_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(pod_file), dt=np.array(dt), dx=np.array(dx), every=np.array(pod_every), start=np.array(pod_start), **arrays)
        if (vis_given or args.frame_every) and args.visualization != 3:      # (-vis 3 is the dye: it has no modes)
            out.mkdir(exist_ok=True)
            for k in range(arrays["coefficients"].shape[1]):
                save_png(fields_frame(sim, args.visualization, *sim.pod_fields(k)), out / f"pod_mode_{k}.png")

    dist_file = None
    if dist_channels:
        dist_file = Path(args.dist_file) if args.dist_file else out / "dist.npz"
        sim.start_distributions(dist_channels, every=dist_every, start_step=dist_start)
        if args.load_state and load_dist(sim, args.load_state):
            print(f"distributions: continuing the checkpoint's ({sim.distributions()[0]['samples']} samples so far)")

    def write_dist():
        if dist_file is None:
            return
        dist_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(dist_file), dt=np.array(dt), dx=np.array(dx), every=np.array(dist_every), start=np.array(dist_start), **dist_file_arrays(sim))

    def write_ftle():
        if args.ftle is None:
            return
        arrays = {}
        try:
            for direction in ("forward", "backward") if args.ftle == "both" else (args.ftle,):
                m = sim.flow_map(direction, refine=ftle_refine, substeps=ftle_substeps)
                arrays.update({f"ftle_{direction}": m["ftle"], f"status_{direction}": m["status"], f"x_{direction}": m["x"], f"y_{direction}": m["y"],
                               "span": np.array(m["span"]), "sample_steps": m["sample_steps"], "refine": np.array(m["refine"])})
        except RuntimeError as e:
            print(f"FTLE: {e}; no file written", file=sys.stderr)
            return
        ftle_file = Path(args.ftle_file) if args.ftle_file else out / "ftle.npz"
        ftle_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(ftle_file), **arrays)
        if vis_given or args.frame_every:
            out.mkdir(exist_ok=True)
            for direction in ("forward", "backward") if args.ftle == "both" else (args.ftle,):
                save_png(fields_frame(sim, 1, *sim.ftle_fields(direction, substeps=ftle_substeps)), out / f"ftle_{direction}.png")      # (the pressure renderer)

    loads_file = None
    if args.loads_every > 0:
        loads_file = Path(args.loads_file) if args.loads_file else out / "loads.npz"
        try:
            sim.track_body(box, center=loads_center, every=args.loads_every, start_step=args.loads_start)
        except ValueError as e:
            parser.error(f"--body / --loads-center: {e}")
        if args.load_state:
            held = saved_loads(args.load_state)
            bt = sim._tracker
            if held is not None and held != (tuple(bt.box), tuple(bt.centre), bt.every, bt.start_step):
                print(f"--load-state {args.load_state}: its body loads were tracked with --body {','.join(map(str, held[0]))} --loads-center "
                      f"{held[1][0]!r},{held[1][1]!r} --loads-every {held[2]} --loads-start {held[3]}; continue with those or track without "
                      "the checkpoint's sums", file=sys.stderr)
                dev.close()
                sys.exit(2)
            if load_loads(sim, args.load_state):
                print(f"body loads: continuing the checkpoint's ({sim._tracker.samples} samples so far)")

    def write_loads():
        if loads_file is None:
            return
        from fs.loads import coefficients, pressure_coefficient, skin_friction
        loads, surf = sim.body_loads(), sim.body_surface()
        more = {}
        if loads_ref is not None:
            u_ref, length = loads_ref
            more = {"cd": coefficients(loads["force_x"], u_ref, length), "cl": coefficients(loads["force_y"], u_ref, length),
                    "cm": coefficients(loads["moment"], u_ref, length * length), "cp_mean": pressure_coefficient(surf["p_mean"], u_ref),
                    "cf_mean": skin_friction(surf["tau_mean"], u_ref), "ref": np.array(loads_ref)}
        loads_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(loads_file), center=np.array(sim._tracker.centre), box=np.array(sim._tracker.box), re=np.array(args.reynolds_num),
                 dx=np.array(dx), dt=np.array(dt), every=np.array(args.loads_every), start=np.array(args.loads_start), **loads, **surf, **more)

    vortices_file = None
    if args.vortices_every > 0:
        vortices_file = Path(args.vortices_file) if args.vortices_file else out / "vortices.npz"
        try:
            sim.track_vortices(args.vortex_threshold, criterion=args.vortex_criterion, every=args.vortices_every, min_area=args.vortex_min_area,
                               max_vortices=args.vortex_max)
        except _lib_error() as e:
            print(f"--vortices-every: {e}", file=sys.stderr)
            dev.close()
            sys.exit(2)
        if args.load_state:
            held = saved_vortices(args.load_state)
            vx = sim._vortexr.vx
            mine = (vx.criterion, vx.threshold, vx.every, vx.min_area, vx.max_vortices)
            if held is not None and held != mine:
                print(f"--load-state {args.load_state}: its vortices were tracked with --vortex-criterion {held[0]} --vortex-threshold {held[1]!r} "
                      f"--vortices-every {held[2]} --vortex-min-area {held[3]} --vortex-max {held[4]}; continue with those or track without the "
                      "checkpoint's samples", file=sys.stderr)
                dev.close()
                sys.exit(2)
            if held is not None:
                sim._vortexr.restore(np.load(_npz_path(args.load_state)))
                print(f"vortices: continuing the checkpoint's ({len(sim._vortexr._words[0]) if sim._vortexr._words else 0} samples so far)")

    def write_vortices():
        if vortices_file is None:
            return
        from fs.vortices import link
        data = sim.vortices()
        raw = data.pop("raw")
        tracks = link(data, args.vortex_link)
        vortices_file.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(vortices_file), track=tracks, dx=np.array(dx), dt=np.array(dt), every=np.array(args.vortices_every),
                 threshold=np.array(args.vortex_threshold), criterion=np.array(args.vortex_criterion), **{f"raw_{k}": a for k, a in raw.items()},
                 **data)

    tracer_file = None
    if tracing:
        tracer_file = Path(args.tracer_file) if args.tracer_file else out / "tracers.npz"
        if args.load_state and load_tracers(sim, args.load_state, args.tracer_sort_every, accumulate):
            print(f"tracers: continuing the checkpoint's {sim._tracers.set.n} particles (the seed flags are not used)")
        else:
            seeds, notes = tracer_seeds(np.asarray(sim._solver._bc.mask), args.tracers, args.tracer_seed or 0, lines)
            for note in notes:
                print(note)
            if len(seeds) == 0:
                print("tracers: no seed lies in a fluid cell", file=sys.stderr)
                dev.close()
                sys.exit(2)
            if taus is None:
                sim.seed_tracers(seeds, respawn=not args.tracer_once, max_age=max_age, sort_every=args.tracer_sort_every)
            else:
                sim.seed_tracers(seeds, respawn=not args.tracer_once, max_age=max_age, sort_every=args.tracer_sort_every,
                                 tau=tracer_taus(taus, len(seeds)), gravity=gravity, deposits=args.tracer_deposits)
            if accumulate is not None:
                sim.accumulate_tracers(every=accumulate[0], start_step=accumulate[1])
    fields_file = None
    if tracing and args.tracer_fields:
        fields_file = Path(args.tracer_fields_file) if args.tracer_fields_file else out / "tracer_fields.npz"

    def write_tracers(path, fields_path=None, step=None):
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(path), **sim.tracers())
        if fields_path is not None:
            from fs.tracers import residence_map
            f = sim.tracer_fields()
            fields_path.parent.mkdir(parents=True, exist_ok=True)
            more = {}
            if sim._tracers.deposits:
                more["deposits"] = sim.tracer_deposits()
            if sim._tracers.accumulation is not None:
                acc = sim.tracer_accumulation()
                more.update(occupancy=acc["occupancy"], accumulated_age_sum=acc["age_sum"], samples=np.array(acc["samples"]))
            np.savez(str(fields_path), count=f["count"], age_sum=f["age_sum"], residence=residence_map(f["count"], f["age_sum"], dt),
                     step=np.array(step), **more)

    stats = None
    if args.stats_every > 0:
        stats = StatsWriter(sim, Path(args.stats_file) if args.stats_file else out / "stats.csv", dt, box, args.stop_on_nonfinite,
                            p_residual=args.pressure is not None)

    def sample(step):
        if stats.sample(step) > 0 and stats.stop:
            stats.close()
            print(f"step {step}: non-finite values (NaN / Inf) in v or p; stopping (--stop-on-nonfinite)", file=sys.stderr)
            write_history()
            write_mean()
            write_modes()
            write_pod()
            write_dist()
            write_ftle()
            write_loads()
            write_vortices()
            if tracer_file is not None:
                write_tracers(tracer_file, fields_file, step)
            dev.close()
            sys.exit(3)

    t0 = time.perf_counter()
    step, last = step0, step0 + args.steps
    if stats:
        sample(step)
    while step < last:
        if args.frame_every and step % args.frame_every == 0:
            out.mkdir(exist_ok=True)
            save_png(frame(sim, args.visualization), out / f"{step:06}.png")
        # steps until the next frame / dump / end: one chunk (a hipGraph replay with --graph, a plain loop otherwise)
        nxt = last
        if args.frame_every:
            nxt = min(nxt, (step // args.frame_every + 1) * args.frame_every)
        if args.dump_every:
            nxt = min(nxt, (step // args.dump_every + 1) * args.dump_every)
        if stats:
            nxt = min(nxt, (step // args.stats_every + 1) * args.stats_every)
        if args.tracer_dump_every:
            nxt = min(nxt, (step // args.tracer_dump_every + 1) * args.tracer_dump_every)
        sim.run(nxt - step, graph=args.graph)
        step = nxt
        if stats and step % args.stats_every == 0:
            sample(step)
        if args.dump_every and step % args.dump_every == 0:
            out.mkdir(exist_ok=True)
            np.savez(str(out / f"step_{step:06}.npz"), **sim.field_to_numpy())
        if args.tracer_dump_every and step % args.tracer_dump_every == 0:
            write_tracers(out / f"tracers_{step:06}.npz", out / f"tracer_fields_{step:06}.npz" if fields_file is not None else None, step)
    dev.sync()
    el = time.perf_counter() - t0
    print(f"{args.steps} steps in {el:.3f} s = {args.steps / el:.1f} steps/s")
    if args.save_state:
        save_state(sim, args.save_state, step0 + args.steps)
    if stats:
        stats.close()
    write_history()
    write_mean()
    write_modes()
    write_pod()
    write_dist()
    write_ftle()
    write_loads()
    write_vortices()
    if tracer_file is not None:
        write_tracers(tracer_file, fields_file, step0 + args.steps)
    dev.close()


if __name__ == "__main__":
    main()
