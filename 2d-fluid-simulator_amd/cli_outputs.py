"""What main.py writes at the end of a run, one class per output: its flags, their checks, what a --load-state checkpoint must hold for it
to continue, the rider it attaches to the simulator and its file(s).  main() walks OUTPUTS and names none of them: a new output is one
class here and one entry in that list.  What a checkpoint holds is read by the rider classes (held(z), next to the checkpoint() that
writes the same keys); every refusal of a checkpoint taken with other parameters has exit status 2."""
import sys
from pathlib import Path

import numpy as np


class Run:
    """What the outputs share of one main() call: the parsed flags and their parser, the grid and time step, the folder and the image
    flags, the body box (set once the flags are checked) and the step a checkpoint resumes from."""

    def __init__(self, args, parser, vis_given):
        self.args, self.parser, self.vis_given = args, parser, vis_given
        self.res = args.resolution
        self.dt = args.time_step if args.time_step != 0.0 else 0.05 / self.res
        self.dx = 1 / self.res
        self.out, self.vis, self.frame_every, self.re = Path(args.out), args.visualization, args.frame_every, args.reynolds_num
        self.box, self.step0 = None, 0


def _floats(parser, flag, spec, count=None):
    try:
        vals = [float(c) for c in spec.split(",")]
        if not vals or (count is not None and len(vals) != count) or not all(np.isfinite(v) for v in vals):
            raise ValueError
    except ValueError:
        parser.error(f"{flag} {spec}: expected {'%d finite numbers' % count if count else 'finite numbers'} separated by commas")
    return vals


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


class Output:
    """One output.  configure() answers whether the flags turn it on; main() calls the other members of those that are on, in the order
    of OUTPUTS: check_held() before the simulator exists, attach() after load_state, write() at either exit, and dump() every
    `dump_every` steps where that is not 0."""
    name = None          # the default file is <out>/<name>.npz
    help_rank = 0        # --help lists the flags of OUTPUTS in this order, and those of equal rank in the list's
    dump_every = 0

    def add_flags(self, parser):
        raise NotImplementedError

    def configure(self, args, parser, run):
        """Check the flags (parser.error) and keep their values -> whether the output is on."""
        raise NotImplementedError

    def check_held(self, z, run):
        """Refuse (status 2) a checkpoint z that holds this output's rider with other parameters than the flags'."""

    def attach(self, sim, z, run):
        """Attach the rider; continue from the checkpoint z (None without --load-state) when it holds one."""

    def write(self, sim, step, run):
        raise NotImplementedError

    def path(self, run, given):
        return Path(given) if given else run.out / f"{self.name}.npz"

    @staticmethod
    def save(path, **arrays):
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(str(path), **arrays)

    @staticmethod
    def sampling(run, every, start):
        """The keys the files of the sampled fields begin with."""
        return {"dt": np.array(run.dt), "dx": np.array(run.dx), "every": np.array(every), "start": np.array(start)}

    @staticmethod
    def refuse(run, text, sim=None):
        print(f"--load-state {run.args.load_state}: {text}", file=sys.stderr)
        if sim is not None:
            sim._solver._bc.device.close()
        sys.exit(2)

    @staticmethod
    def resume(rider, z, label):
        """restore() the freshly attached rider from the checkpoint when it holds one of its kind."""
        if z is not None and rider.held(z) is not None:
            print(f"{label}: continuing the checkpoint's ({rider.restore(z)} samples so far)")


class History(Output):
    name = "history"

    def add_flags(self, p):
        p.add_argument("--history-every", type=int, default=0,
                       help="record the probes (--probe) and the body force (--body) after every N-th step on the GPU (FluidSimulator.record_history)")
        p.add_argument("--probe", type=str, action="append", default=[], metavar="X,Y",
                       help="a fluid cell (global x,y) whose u, w, p go into the history; may be repeated")
        p.add_argument("--history-file", type=str, default=None,
                       help=".npz of the history: step, time, probes, u, w, p[, force_x, force_y] (default: <out>/history.npz)")

    def configure(self, args, parser, run):
        if (args.probe or args.history_file) and args.history_every <= 0:
            parser.error("--probe and --history-file need --history-every N")
        if args.history_every > 0 and not args.probe and args.body is None:
            parser.error("--history-every needs --probe X,Y or --body")
        self.probes = []
        for spec in args.probe:
            try:
                x, y = (int(c) for c in spec.split(","))
            except ValueError:
                parser.error(f"--probe {spec}: expected x,y (global cell)")
            self.probes.append((x, y))
        return args.history_every > 0

    def attach(self, sim, z, run):
        try:        # (a history recorder has nothing to resume: it starts at the checkpoint's step)
            sim.record_history(self.probes, run.box, every=run.args.history_every, start_step=run.step0)
        except ValueError as e:
            run.parser.error(f"--probe: {e}")

    def write(self, sim, step, run):
        self.save(self.path(run, run.args.history_file), **sim.history())


class Mean(Output):
    name = "mean"

    def add_flags(self, p):
        p.add_argument("--mean-every", type=int, default=0,
                       help="accumulate time averages of u, w, p and their second moments after every N-th step on the GPU "
                            "(FluidSimulator.start_averaging; 0: off)")
        p.add_argument("--mean-start", type=int, default=0, help="steps of the averaged run (restarts included) to leave out before the first sample")
        p.add_argument("--mean-file", type=str, default=None,
                       help=".npz of the averages: samples, steps, u, w, p, uu, ww, uw, p_rms, tke, mask, dt, dx, every, start "
                            "(default: <out>/mean.npz)")

    def configure(self, args, parser, run):
        if args.mean_every < 0 or args.mean_start < 0:
            parser.error("--mean-every and --mean-start must be >= 0")
        if (args.mean_start or args.mean_file) and args.mean_every <= 0:
            parser.error("--mean-start and --mean-file need --mean-every N")
        self.every, self.start = args.mean_every, args.mean_start
        return self.every > 0

    def check_held(self, z, run):
        from fs.averages import Averager
        held = Averager.held(z)
        if held is not None and held != (self.every, self.start):
            self.refuse(run, f"its time average was taken with --mean-every {held[0]} --mean-start {held[1]}, "
                             f"not {self.every} / {self.start}; continue with those or average without the checkpoint's sums")

    def attach(self, sim, z, run):
        sim.start_averaging(every=self.every, start_step=self.start)
        self.resume(sim._averager, z, "time average")

    def write(self, sim, step, run):
        try:
            avg = sim.averages()
        except RuntimeError as e:
            print(f"time average: {e}; no file written", file=sys.stderr)
            return
        self.save(self.path(run, run.args.mean_file), **self.sampling(run, self.every, self.start), **avg)
        if run.frame_every and run.vis != 3:      # (-vis 3 is the dye: it is not averaged)
            run.out.mkdir(exist_ok=True)
            save_png(fields_frame(sim, run.vis, *sim.mean_fields()), run.out / "mean_vis.png")


class Modes(Output):
    name = "modes"

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        if args.modes_freq is None:
            if args.modes_every is not None or args.modes_start is not None or args.modes_file or args.modes_frames:
                parser.error("--modes-every, --modes-start, --modes-file and --modes-frames need --modes-freq F")
            return False
        from fs.modes import phasor_steps
        self.freqs = _floats(parser, "--modes-freq", args.modes_freq)
        self.every, self.start = (1 if args.modes_every is None else args.modes_every), args.modes_start or 0
        if self.every < 1 or self.start < 0 or args.modes_frames < 0:
            parser.error("--modes-every must be >= 1, --modes-start and --modes-frames >= 0")
        if args.modes_frames and args.visualization == 3:
            parser.error("--modes-frames: -vis 3 is the dye, which has no modes (use -vis 0, 1 or 2)")
        try:
            phasor_steps(self.freqs, self.every, run.dt)
        except ValueError as e:
            parser.error(f"--modes-freq {args.modes_freq}: {e}")
        return True

    def check_held(self, z, run):
        from fs.modes import Modes as Rider
        held = Rider.held(z)
        if held is not None and held != (tuple(self.freqs), self.every, self.start):
            self.refuse(run, f"its modes were taken with --modes-freq {','.join(repr(f) for f in held[0])} --modes-every "
                             f"{held[1]} --modes-start {held[2]}; continue with those or accumulate without the checkpoint's sums")

    def attach(self, sim, z, run):
        sim.start_modes(self.freqs, every=self.every, start_step=self.start)
        self.resume(sim._moder, z, "modes")

    def write(self, sim, step, run):
        try:
            modes = sim.modes()
        except RuntimeError as e:
            print(f"modes: {e}; no file written", file=sys.stderr)
            return
        arrays = {"frequencies": modes["frequencies"], "samples": np.array(modes["samples"]), "steps": np.array(modes["steps"]), "mask": modes["mask"]}
        for name in ("u", "w", "p"):
            arrays[f"mean_{name}"], arrays[f"amplitude_{name}"], arrays[f"phase_{name}"] = modes[name]["mean"], modes[name]["amplitude"], modes[name]["phase"]
        self.save(self.path(run, run.args.modes_file), **self.sampling(run, self.every, self.start), **arrays)
        frames = run.args.modes_frames
        if frames:
            run.out.mkdir(exist_ok=True)
            for i in range(frames):
                v, p = sim.mode_fields(2.0 * np.pi * i / frames, 0)
                save_png(fields_frame(sim, run.vis, v, p), run.out / f"modes_phase_{i}.png")


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


class Pod(Output):
    name = "pod"

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        self.snapshots = args.pod_snapshots
        self.every, self.start, self.modes = (1 if args.pod_every is None else args.pod_every), args.pod_start or 0, (4 if args.pod_modes is None else args.pod_modes)
        if self.snapshots == 0:
            if args.pod_every is not None or args.pod_start is not None or args.pod_modes is not None or args.pod_file:
                parser.error("--pod-every, --pod-start, --pod-modes and --pod-file need --pod-snapshots M")
            return False
        if not 2 <= self.snapshots <= 64:
            parser.error("--pod-snapshots must be 2 .. 64")
        if self.every < 1 or self.start < 0 or self.modes < 0:
            parser.error("--pod-every must be >= 1, --pod-start and --pod-modes >= 0")
        return True

    def check_held(self, z, run):
        from fs.pod import Pod as Rider
        held = Rider.held(z)
        if held is not None and held != (self.snapshots, self.every, self.start):
            self.refuse(run, f"its POD snapshots were taken with --pod-snapshots {held[0]} --pod-every {held[1]} --pod-start "
                             f"{held[2]}; continue with those or sample without the checkpoint's snapshots")

    def attach(self, sim, z, run):
        sim.start_pod(self.snapshots, every=self.every, start_step=self.start)
        self.resume(sim._podr, z, "POD")

    def write(self, sim, step, run):
        try:
            arrays = pod_file_arrays(sim, self.modes)
        except (RuntimeError, ValueError) as e:
            print(f"POD: {e}; no file written", file=sys.stderr)
            return
        self.save(self.path(run, run.args.pod_file), **self.sampling(run, self.every, self.start), **arrays)
        if (run.vis_given or run.frame_every) and run.vis != 3:      # (-vis 3 is the dye: it has no modes)
            run.out.mkdir(exist_ok=True)
            for k in range(arrays["coefficients"].shape[1]):
                save_png(fields_frame(sim, run.vis, *sim.pod_fields(k)), run.out / f"pod_mode_{k}.png")


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


def dist_flags(held):
    """The flags that continue the distributions of a checkpoint (fs.dist.Distributions.held), for the refusal's message."""
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


class Dist(Output):
    name = "dist"

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        self.every, self.start = (1 if args.dist_every is None else args.dist_every), args.dist_start or 0
        if not args.dist:
            if args.dist_every is not None or args.dist_start is not None or args.dist_box or args.dist_file:
                parser.error("--dist-every, --dist-start, --dist-box and --dist-file need --dist SPEC")
            return False
        if self.every < 1 or self.start < 0:
            parser.error("--dist-every must be >= 1 and --dist-start >= 0")
        self.channels, self.checked = parse_dist(parser, args.dist, args.dist_box, 2 * run.res, run.res)
        return True

    def check_held(self, z, run):
        from fs.dist import Distributions, channels_array
        held, mine = Distributions.held(z), channels_array(self.checked)
        if held is not None and (held[0].shape != mine.shape or not np.array_equal(held[0], mine) or held[1:] != (self.every, self.start)):
            self.refuse(run, f"its distributions were accumulated with {dist_flags(held)}; continue with those or "
                             "accumulate without the checkpoint's tables")

    def attach(self, sim, z, run):
        sim.start_distributions(self.channels, every=self.every, start_step=self.start)
        self.resume(sim._distr, z, "distributions")

    def write(self, sim, step, run):
        arrays = {}
        for k, d in enumerate(sim.distributions()):
            for name in ("counts", "edges", "edges_b", "below", "above", "outside", "nan", "quantity", "box"):
                if name in d:
                    arrays[f"c{k}.{name}"] = np.asarray(d[name])
            arrays["samples"], arrays["sample_steps"] = np.array(d["samples"]), d["sample_steps"]
        self.save(self.path(run, run.args.dist_file), **self.sampling(run, self.every, self.start), **arrays)


class Ftle(Output):
    """No rider of its own: the flow maps are integrated through the POD's resident snapshots when the run ends."""
    name = "ftle"

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        self.refine, self.substeps = (1 if args.ftle_refine is None else args.ftle_refine), (1 if args.ftle_substeps is None else args.ftle_substeps)
        if args.ftle is None:
            if args.ftle_refine is not None or args.ftle_substeps is not None or args.ftle_file:
                parser.error("--ftle-refine, --ftle-substeps and --ftle-file need --ftle forward|backward|both")
            return False
        if args.pod_snapshots == 0:
            parser.error("--ftle needs --pod-snapshots M: the flow map is integrated through the resident snapshots")
        if self.refine not in (1, 2, 4, 8) or not 1 <= self.substeps <= 16:
            parser.error("--ftle-refine must be 1, 2, 4 or 8 and --ftle-substeps 1 .. 16")
        self.directions = ("forward", "backward") if args.ftle == "both" else (args.ftle,)
        return True

    def write(self, sim, step, run):
        arrays = {}
        try:
            for direction in self.directions:
                m = sim.flow_map(direction, refine=self.refine, substeps=self.substeps)
                arrays.update({f"ftle_{direction}": m["ftle"], f"status_{direction}": m["status"], f"x_{direction}": m["x"], f"y_{direction}": m["y"],
                               "span": np.array(m["span"]), "sample_steps": m["sample_steps"], "refine": np.array(m["refine"])})
        except RuntimeError as e:
            print(f"FTLE: {e}; no file written", file=sys.stderr)
            return
        self.save(self.path(run, run.args.ftle_file), **arrays)
        if run.vis_given or run.frame_every:
            run.out.mkdir(exist_ok=True)
            for direction in self.directions:      # (the pressure renderer)
                save_png(fields_frame(sim, 1, *sim.ftle_fields(direction, substeps=self.substeps)), run.out / f"ftle_{direction}.png")


class Loads(Output):
    name = "loads"
    help_rank = 3

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        if args.loads_every < 0 or args.loads_start < 0:
            parser.error("--loads-every and --loads-start must be >= 0")
        if (args.loads_start or args.loads_center or args.loads_ref or args.loads_file) and args.loads_every <= 0:
            parser.error("--loads-start, --loads-center, --loads-ref and --loads-file need --loads-every N")
        if args.loads_every > 0 and args.body is None:
            parser.error("--loads-every needs --body")
        self.center = tuple(_floats(parser, "--loads-center", args.loads_center, 2)) if args.loads_center else None
        self.ref = tuple(_floats(parser, "--loads-ref", args.loads_ref, 2)) if args.loads_ref else None
        if self.ref is not None and (self.ref[0] == 0.0 or self.ref[1] <= 0.0):
            parser.error(f"--loads-ref {args.loads_ref}: the speed must not be 0 and the length must be > 0")
        self.every, self.start = args.loads_every, args.loads_start
        return self.every > 0

    def attach(self, sim, z, run):
        try:
            sim.track_body(run.box, center=self.center, every=self.every, start_step=self.start)
        except ValueError as e:
            run.parser.error(f"--body / --loads-center: {e}")
        bt = sim._tracker       # (the refusal waits for the tracker: it compares with the centre track_body worked out)
        held = bt.held(z) if z is not None else None
        if held is not None and held != (tuple(bt.box), tuple(bt.centre), bt.every, bt.start_step):
            self.refuse(run, f"its body loads were tracked with --body {','.join(map(str, held[0]))} --loads-center "
                             f"{held[1][0]!r},{held[1][1]!r} --loads-every {held[2]} --loads-start {held[3]}; continue with those or track without "
                             "the checkpoint's sums", sim)
        self.resume(bt, z, "body loads")

    def write(self, sim, step, run):
        from fs.loads import coefficients, pressure_coefficient, skin_friction
        loads, surf = sim.body_loads(), sim.body_surface()
        more = {}
        if self.ref is not None:
            u_ref, length = self.ref
            more = {"cd": coefficients(loads["force_x"], u_ref, length), "cl": coefficients(loads["force_y"], u_ref, length),
                    "cm": coefficients(loads["moment"], u_ref, length * length), "cp_mean": pressure_coefficient(surf["p_mean"], u_ref),
                    "cf_mean": skin_friction(surf["tau_mean"], u_ref), "ref": np.array(self.ref)}
        self.save(self.path(run, run.args.loads_file), center=np.array(sim._tracker.centre), box=np.array(sim._tracker.box), re=np.array(run.re),
                  dx=np.array(run.dx), dt=np.array(run.dt), every=np.array(self.every), start=np.array(self.start), **loads, **surf, **more)


class Vortices(Output):
    name = "vortices"
    help_rank = 2

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
        if args.vortices_every < 0:
            parser.error("--vortices-every must be >= 0")
        if args.vortices_every > 0 and (args.vortex_threshold is None or not np.isfinite(args.vortex_threshold)):
            parser.error("--vortices-every needs a finite --vortex-threshold T (1 / time^2)")
        if args.vortices_every > 0 and not (1 <= args.vortex_max <= 1024 and args.vortex_min_area >= 1 and args.vortex_link >= 0.0):
            parser.error("--vortex-max must be 1 .. 1024, --vortex-min-area >= 1 and --vortex-link >= 0")
        if (args.vortex_threshold is not None or args.vortices_file) and args.vortices_every <= 0:
            parser.error("--vortex-threshold and --vortices-file need --vortices-every N")
        return args.vortices_every > 0

    def attach(self, sim, z, run):
        from fs._lib import FsError
        a = run.args
        try:
            sim.track_vortices(a.vortex_threshold, criterion=a.vortex_criterion, every=a.vortices_every, min_area=a.vortex_min_area,
                               max_vortices=a.vortex_max)
        except (FsError, ValueError) as e:
            print(f"--vortices-every: {e}", file=sys.stderr)
            sim._solver._bc.device.close()
            sys.exit(2)
        vx = sim._vortexr.vx    # (the refusal waits for the device object: it compares with the threshold as the device holds it)
        held = sim._vortexr.held(z) if z is not None else None
        if held is not None and held != (vx.criterion, vx.threshold, vx.every, vx.min_area, vx.max_vortices):
            self.refuse(run, f"its vortices were tracked with --vortex-criterion {held[0]} --vortex-threshold {held[1]!r} "
                             f"--vortices-every {held[2]} --vortex-min-area {held[3]} --vortex-max {held[4]}; continue with those or track without the "
                             "checkpoint's samples", sim)
        self.resume(sim._vortexr, z, "vortices")

    def write(self, sim, step, run):
        from fs.vortices import link
        a = run.args
        data = sim.vortices()
        raw = data.pop("raw")
        tracks = link(data, a.vortex_link)
        self.save(self.path(run, a.vortices_file), track=tracks, dx=np.array(run.dx), dt=np.array(run.dt), every=np.array(a.vortices_every),
                  threshold=np.array(a.vortex_threshold), criterion=np.array(a.vortex_criterion), **{f"raw_{k}": x for k, x in raw.items()}, **data)


def tracer_taus(values, n):
    """--tracer-tau's values cycled over n particles (size classes): particle k has values[k % len(values)]."""
    return np.resize(np.asarray(values, np.float64), n)


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


def _tracer_line(parser, spec):
    c = spec.split(",")
    try:
        x0, y0, x1, y1, n = float(c[0]), float(c[1]), float(c[2]), float(c[3]), int(c[4])
        if len(c) != 5 or n < 1:
            raise ValueError
    except (ValueError, IndexError):
        parser.error(f"--tracer-line {spec}: expected x0,y0,x1,y1,n (cell units, n >= 1)")
    return x0, y0, x1, y1, n


class Tracers(Output):
    """The one output with a periodic dump as well (--tracer-dump-every)."""
    name = "tracers"
    help_rank = 1

    def add_flags(self, p):
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

    def configure(self, args, parser, run):
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
        self.taus = _floats(parser, "--tracer-tau", args.tracer_tau) if args.tracer_tau is not None else None
        if self.taus is not None and min(self.taus) < 0:
            parser.error(f"--tracer-tau {args.tracer_tau}: response times must be >= 0")
        self.gravity = tuple(_floats(parser, "--tracer-gravity", args.tracer_gravity, 2)) if args.tracer_gravity is not None else (0.0, 0.0)
        self.accumulate = (args.tracer_accumulate_every, args.tracer_accumulate_start or 0) if args.tracer_accumulate_every else None
        self.lines = [_tracer_line(parser, spec) for spec in args.tracer_line]
        self.max_age, self.dump_every = args.tracer_max_age or 0, args.tracer_dump_every
        return tracing

    def check_held(self, z, run):
        from fs.tracers import Tracers as Rider
        a = run.args
        held, more = Rider.held(z), Rider.held_inertial(z)
        if held is None:
            return
        if held[:2] != (not a.tracer_once, self.max_age):
            self.refuse(run, f"its tracers ran with{'out' if held[0] else ''} --tracer-once and --tracer-max-age {held[1]}; "
                             "continue with those or drop the tracer flags")
        want_tau = tracer_taus(self.taus, held[2]) if self.taus is not None else None
        same_tau = (want_tau is None) == (more["tau"] is None) and (want_tau is None or np.array_equal(want_tau, more["tau"]))
        if not same_tau or more["gravity"] != self.gravity or more["deposits"] != bool(a.tracer_deposits):
            was = "passive tracers" if more["tau"] is None else (f"inertial tracers (--tracer-tau of {len(np.unique(more['tau']))} value(s), "
                                                                 f"--tracer-gravity {more['gravity'][0]:g},{more['gravity'][1]:g}, "
                                                                 f"with{'' if more['deposits'] else 'out'} --tracer-deposits)")
            self.refuse(run, f"it holds {was}; continue with those flags or drop the tracer flags")
        if more["accumulate"] is not None and more["accumulate"] != self.accumulate:
            now = "no accumulation" if self.accumulate is None else f"{self.accumulate[0]} / {self.accumulate[1]}"
            self.refuse(run, f"it holds an occupancy accumulated with --tracer-accumulate-every {more['accumulate'][0]} "
                             f"--tracer-accumulate-start {more['accumulate'][1]}, not {now}; continue with those flags (the sums would be lost otherwise) "
                             "or drop the tracer flags")

    def attach(self, sim, z, run):
        from fs.tracers import Tracers as Rider
        a = run.args
        self.file = self.path(run, a.tracer_file)
        self.fields_file = (Path(a.tracer_fields_file) if a.tracer_fields_file else run.out / "tracer_fields.npz") if a.tracer_fields else None
        if z is not None and Rider.held(z) is not None:
            # the checkpoint's set, in seed order: whether the run that wrote it sorted its particles, and whether this one will, makes no
            # difference; an inertial set comes back with its response times, gravity, particle velocities and deposit plane
            more = Rider.held_inertial(z)
            inertial = {} if more["tau"] is None else {"tau": z["tracer.tau"], "gravity": more["gravity"], "deposits": more["deposits"]}
            sim.seed_tracers(z["tracer.seeds"], respawn=bool(z["tracer.respawn"]), max_age=int(z["tracer.max_age"]), sort_every=a.tracer_sort_every,
                             **inertial)
            print(f"tracers: continuing the checkpoint's {sim._tracers.restore(z)} particles (the seed flags are not used)")
        else:
            seeds, notes = tracer_seeds(np.asarray(sim._solver._bc.mask), a.tracers, a.tracer_seed or 0, self.lines)
            for note in notes:
                print(note)
            if len(seeds) == 0:
                print("tracers: no seed lies in a fluid cell", file=sys.stderr)
                sim._solver._bc.device.close()
                sys.exit(2)
            inertial = {} if self.taus is None else {"tau": tracer_taus(self.taus, len(seeds)), "gravity": self.gravity, "deposits": a.tracer_deposits}
            sim.seed_tracers(seeds, respawn=not a.tracer_once, max_age=self.max_age, sort_every=a.tracer_sort_every, **inertial)
            z = None
        if self.accumulate is not None:
            sim.accumulate_tracers(every=self.accumulate[0], start_step=self.accumulate[1])
            if z is not None:
                sim._tracers.accumulation.restore(z)        # (nothing when the checkpoint holds none: a fresh accumulation)

    def write(self, sim, step, run):
        self._write(sim, step, run, self.file, self.fields_file)

    def dump(self, sim, step, run):
        self._write(sim, step, run, run.out / f"tracers_{step:06}.npz", run.out / f"tracer_fields_{step:06}.npz" if self.fields_file is not None else None)

    def _write(self, sim, step, run, path, fields_path):
        self.save(path, **sim.tracers())
        if fields_path is not None:
            from fs.tracers import residence_map
            f = sim.tracer_fields()
            more = {}
            if sim._tracers.deposits:
                more["deposits"] = sim.tracer_deposits()
            if sim._tracers.accumulation is not None:
                acc = sim.tracer_accumulation()
                more.update(occupancy=acc["occupancy"], accumulated_age_sum=acc["age_sum"], samples=np.array(acc["samples"]))
            self.save(fields_path, count=f["count"], age_sum=f["age_sum"], residence=residence_map(f["count"], f["age_sum"], run.dt),
                      step=np.array(step), **more)


# the order of the attachments and of the files written
OUTPUTS = [History, Mean, Modes, Pod, Dist, Ftle, Loads, Vortices, Tracers]
