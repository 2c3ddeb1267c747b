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
from cli_outputs import OUTPUTS, Run, parse_dist, save_png, tracer_seeds, tracer_taus  # noqa: E402, F401 (the tests reach them through this module)
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
    for output in sorted(OUTPUTS, key=lambda cls: cls.help_rank):      # (stable: the order of OUTPUTS within a rank)
        output().add_flags(p)
    return p


def _npz_path(path):
    """np.savez appends '.npz' to a name without it; use the same name for writing and reading."""
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


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


def load_state(sim, z):
    """z: the checkpoint's mapping, or the path of its file."""
    s = sim._solver
    if isinstance(z, (str, os.PathLike)):
        z = np.load(_npz_path(z))
    for name in _STATE:
        if hasattr(s, name):
            getattr(s, name).current.from_numpy(z[f"{name}.current"])
            getattr(s, name).next.from_numpy(z[f"{name}.next"])
    vc = s.vorticity_confinement
    if vc is not None and "vorticity" in z:
        vc.vorticity.from_numpy(z["vorticity"])
        vc.vorticity_abs.from_numpy(z["vorticity_abs"])
    return int(z["step"])


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


def _base_checks(parser, args):
    """The checks that belong to no output."""
    if args.visualization == 3 and args.no_dye:
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
    if args.pressure == "multigrid" and args.resolution % 2:
        parser.error("--pressure multigrid needs an even -res (no coarse level otherwise)")
    if args.body is not None and args.stats_every <= 0 and args.history_every <= 0 and args.loads_every <= 0:
        parser.error("--body needs --stats-every N, --history-every N or --loads-every N")


def write_outputs(outputs, sim, step, run):
    """The end-of-run files of the outputs that are on, in their order; both exits of main() end here."""
    for output in outputs:
        output.write(sim, step, run)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    vis_given = any(a in ("-vis", "--visualization") or a.startswith("--visualization=") for a in (sys.argv[1:] if argv is None else argv))
    if args.cpu:
        print("note: -cpu ignored; this build runs on the GPU only", file=sys.stderr)
    run = Run(args, parser, vis_given)
    res, dt, out = run.res, run.dt, run.out
    vor_eps = args.vorticity_confinement if args.vorticity_confinement != 0.0 else None
    _base_checks(parser, args)
    outputs = [output for output in (cls() for cls in OUTPUTS) if output.configure(args, parser, run)]
    z = np.load(_npz_path(args.load_state)) if args.load_state else None       # (the one time the checkpoint is opened)
    if z is not None:
        for output in outputs:
            output.check_held(z, run)
    run.box = _body_box(parser, args.body, args.boundary_condition, res)
    print(f"Boundary Condition: {args.boundary_condition}\ndt: {dt}\nRe: {args.reynolds_num}\nResolution: {res}\n"
          f"Scheme: {args.advection_scheme}\nVorticity confinement: {vor_eps}")
    fs.runtime.init(gpu=args.gpu, dtype="f64" if args.f64 else "f32")
    cls = FluidSimulator if args.no_dye else DyeFluidSimulator
    updater = None      # (the reference's red-black SOR(1.3, 2))
    if args.pressure == "multigrid":
        mg_kw = {k: v for k, v in (("coarsest", args.mg_coarsest), ("direct_cells", args.mg_direct_cells)) if v is not None}
        updater = ("multigrid", args.mg_cycles or 1) + ((mg_kw,) if mg_kw else ())
    sim = cls.create(args.boundary_condition, res, dt, run.dx, args.reynolds_num, vor_eps, args.advection_scheme, pressure_updater=updater)
    step0 = run.step0 = load_state(sim, z) if z is not None else 0
    dev = sim._solver._bc.device
    for output in outputs:
        output.attach(sim, z, run)
    dumps = [output for output in outputs if output.dump_every]      # (the outputs with a periodic file as well)
    stats = None
    if args.stats_every > 0:
        stats = StatsWriter(sim, Path(args.stats_file) if args.stats_file else out / "stats.csv", dt, run.box, args.stop_on_nonfinite,
                            p_residual=args.pressure is not None)

    def sample(step):
        if stats.sample(step) > 0 and stats.stop:
            stats.close()
            print(f"step {step}: non-finite values (NaN / Inf) in v or p; stopping (--stop-on-nonfinite)", file=sys.stderr)
            write_outputs(outputs, sim, step, run)
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
        for every in [args.frame_every, args.dump_every, args.stats_every if stats else 0] + [output.dump_every for output in dumps]:
            if every:
                nxt = min(nxt, (step // every + 1) * every)
        sim.run(nxt - step, graph=args.graph)
        step = nxt
        if stats and step % args.stats_every == 0:
            sample(step)
        if args.dump_every and step % args.dump_every == 0:
            out.mkdir(exist_ok=True)
            np.savez(str(out / f"step_{step:06}.npz"), **sim.field_to_numpy())
        for output in dumps:
            if step % output.dump_every == 0:
                output.dump(sim, step, run)
    dev.sync()
    el = time.perf_counter() - t0
    print(f"{args.steps} steps in {el:.3f} s = {args.steps / el:.1f} steps/s")
    if args.save_state:
        save_state(sim, args.save_state, step0 + args.steps)
    if stats:
        stats.close()
    write_outputs(outputs, sim, step0 + args.steps, run)
    dev.close()


if __name__ == "__main__":
    main()
