"""Facade (reference: fs/fluid_simulator.py): FluidSimulator / DyeFluidSimulator.

`create()` composes boundary condition + vorticity confinement + red-black SOR(omega 1.3, 2 iterations)
+ solver exactly like the reference (fs/fluid_simulator.py:60-108, 129-176); `step()` is the hot path.
`pressure_updater=` is an extension (the reference hard-codes RB-SOR): ("jacobi", n_iter) or
("rbsor", omega, n_iter) or ("multigrid", n_cycles[, omega][, {keyword arguments of MultigridPressureUpdater}]) or a ready
PressureUpdater factory.
"""
import math
import operator

import numpy as np

from .advection import advect_kk_scheme, advect_upwind
from .averages import Averager, derive_averages
from .boundary_condition import get_boundary_condition
from .history import Recorder, body_faces, check_probes
from .loads import Tracker, body_centroid, face_geometry
from .modes import Modes, fit as fit_modes, gram_matrix, phasor_steps, reconstruct_weights
from .pod import Pod
from . import dist as _dist
from . import spectra as _spectra
from . import fluxes as _fluxes
from . import budgets as _budgets
from .vortices import VELOCITY_LIMIT, Vortices, assemble, omega_exponent
from .pressure_updater import JacobiPressureUpdater, MultigridPressureUpdater, RedBlackSorPressureUpdater
from .solver import CipMacSolver, DyeCipMacSolver, DyeMacSolver, MacSolver
from .tracers import TracerAccumulation, Tracers, check_seeds, response
from .vorticity_confinement import VorticityConfinement

_WALL_COLOR = (0.5, 0.7, 0.5)   # fs/fluid_simulator.py:17 (applied by the visualisation kernels, csrc/fs_kernels.h k_visualize)

# The attributes of a FluidSimulator that hold its riders (fs.riders.Rider; None while the kind is not attached), in THE order of the
# riders: that of their launches behind the solver step and of their tokens in _signature().
RIDER_ATTRS = (
    "_recorder",       # fs.history.Recorder while record_history() is on
    "_averager",       # fs.averages.Averager while start_averaging() is on
    "_moder",          # fs.modes.Modes while start_modes() is on
    "_podr",           # fs.pod.Pod while start_pod() is on
    "_distr",          # fs.dist.Distributions while start_distributions() is on
    "_spectrar",       # fs.spectra.Spectra while start_spectra() is on
    "_xspectrar",      # fs.spectra.CrossSpectra while start_cross_spectra() is on
    "_fluxr",          # fs.fluxes.ScaleFluxes while start_scale_fluxes() is on
    "_budgetr",        # fs.budgets.Budget while start_budget() is on
    "_tracker",        # fs.loads.Tracker while track_body() is on
    "_tracers",        # fs.tracers.Tracers while seed_tracers() is on
    "_vortexr",        # fs.vortices.Vortices while track_vortices() is on
)
_rider_slots = operator.attrgetter(*RIDER_ATTRS)


def _make_updater(spec, bc, dt, dx):
    if spec is None:
        return RedBlackSorPressureUpdater(bc, dt, dx, relaxation_factor=1.3, n_iter=2)
    if callable(spec):
        return spec(bc, dt, dx)
    kind = spec[0]
    if kind == "rbsor":
        return RedBlackSorPressureUpdater(bc, dt, dx, relaxation_factor=float(spec[1]), n_iter=int(spec[2]))
    if kind == "jacobi":
        return JacobiPressureUpdater(bc, dt, dx, int(spec[1]))
    if kind == "multigrid":       # ("multigrid", n_cycles[, omega][, {keyword arguments}])
        kw = dict(spec[-1]) if isinstance(spec[-1], dict) else {}
        rest = spec[:-1] if isinstance(spec[-1], dict) else spec
        return MultigridPressureUpdater(bc, dt, dx, relaxation_factor=float(rest[2]) if len(rest) > 2 else 1.3, n_cycles=int(rest[1]), **kw)
    raise ValueError(f"Unknown pressure updater: {spec!r}")


def _compose(num, resolution, dt, dx, re, vor_eps, scheme, enable_dye, pressure_updater):
    if scheme not in ("cip", "upwind", "kk"):
        msg = f"Unknown scheme: {scheme}"
        raise ValueError(msg)
    bc = get_boundary_condition(num, resolution, enable_dye=enable_dye)
    vc = VorticityConfinement(bc, dt, dx, vor_eps) if vor_eps is not None else None
    pu = _make_updater(pressure_updater, bc, dt, dx)
    if scheme == "cip":
        cls = DyeCipMacSolver if enable_dye else CipMacSolver
        return cls(bc, pu, dt, dx, re, vc)
    cls = DyeMacSolver if enable_dye else MacSolver
    adv = advect_upwind if scheme == "upwind" else advect_kk_scheme
    return cls(bc, pu, adv, dt, dx, re, vc)


def derive_flow_stats(raw, dx, dt, with_force):
    """The public diagnostics from the slots of runtime.DeviceBase.flow_stats (see FluidSimulator.flow_stats)."""
    n = raw["fluid_cells"]
    out = {
        "kinetic_energy": 0.5 * dx * dx * raw["sum_s2"],
        "enstrophy": 0.5 * dx * dx * raw["sum_om2"],
        "max_speed": math.sqrt(raw["max_s2"]),          # (sums of squares and maxima are >= 0, NaN or +Inf: math.sqrt passes NaN / Inf on)
        "cfl": raw["max_a"] * dt / dx,
        "div_rms": math.sqrt(raw["sum_dv2"] / n) if n > 0 else 0.0,
        "div_max": raw["max_abs_dv"],
        "nonfinite": int(raw["nonfinite"]),
        "fluid_cells": int(n),
    }
    if with_force:
        out["force_x"], out["force_y"] = raw["force_x"], raw["force_y"]
    return out


class FluidSimulator:
    def __init__(self, solver):
        self._solver = solver
        self._dev = solver._dev
        self.rgb_buf = self._dev.alloc(3)      # image buffer (fs/fluid_simulator.py:16), device resident
        self._wall_color = _WALL_COLOR
        self._graph = None         # (signature, graph id, period) of the most recent capture
        self._graph_long = None    # (graph id, steps) of the same capture's long form: several periods in one graph (capture_period)
        self._graphs = {}          # signature -> (graph id, period, long form or None)
        self._tapes = {}           # (signature, ghost-row bookkeeping state) -> tape
        self._steps = 0
        self._eager_seen = False   # one step has run outside a capture (the library's compact launch lists exist)
        self._pending_after_step = (False, False)
        self._since_hot_check = 0
        for attr in RIDER_ATTRS:
            setattr(self, attr, None)
        self._last_recorder = None  # the recorder after stop_history(): what history() still returns
        self._last_tracker = None  # the body tracker after stop_body(): what body_loads() / body_surface() still return
        self._last_vortexr = None  # the vortex tracker after stop_vortices(): what vortices() / vortex_labels() still return
        self._found_planes = None  # the planes of the last find_vortices()

    def _riders(self):
        """The attached riders (fs.riders.Rider) in their fixed order, that of RIDER_ATTRS."""
        return [r for r in _rider_slots(self) if r is not None]

    def _capturing(self):
        return getattr(self._dev, "capturing", False)

    def _not_capturing(self, name):
        if getattr(self._dev, "capturing", False):
            raise RuntimeError(f"{name} during a graph capture")

    @staticmethod
    def _cadence(every, start_step=0):
        every, start_step = int(every), int(start_step)
        if every < 1:
            raise ValueError("every must be >= 1")
        if start_step < 0:
            raise ValueError("start_step must be >= 0")
        return every, start_step

    def _attached(self, attr, what, start):
        """The attached rider of a kind, or RuntimeError "no `what`: call `start`() first"."""
        r = getattr(self, attr)
        if r is None:
            raise RuntimeError(f"no {what}: call {start}() first")
        return r

    def _once(self, name, create, launch, read, free):
        """The one-shot calls (body_snapshot, find_vortices, histogram, spectrum, ...): refused during a graph capture under the caller's
        `name`; then a temporary device object from create(), one eager launch(obj) that is never part of a logged period, read(obj), and
        free(obj) whatever happened -> (what read returned, the freed object: its parameters stay readable)."""
        dev = self._dev
        self._not_capturing(name)
        obj = create()
        try:
            saved, dev._oplog = getattr(dev, "_oplog", None), None
            try:
                launch(obj)
            finally:
                dev._oplog = saved
            return read(obj), obj
        finally:
            free(obj)

    def _update(self):
        """One solver step, then the launches of every attached rider: what step(), the periods capture_period() captures and the slab
        periods tape_period() logs all run (so a graph or tape holds these launches exactly when _signature() says so)."""
        self._solver.update()
        for r in self._riders():
            r.launch(self)

    def _between_chunks(self):
        """What the riders do between launch sequences - never inside a capture (the scheduled sort of the tracer particles)."""
        if not self._capturing():
            for r in self._riders():
                r.between_chunks()

    def step(self):
        self._update()
        self._between_chunks()
        self._eager_seen = True        # (captures call the solver directly: see capture_period)
        self._pending_after_step = self._limit_pending()
        self._since_hot_check += 1
        if self._since_hot_check >= 256:
            self._check_hot()

    def _check_hot(self):
        """Deferred limit passes are for runs that never need them.  Once a velocity buffer's flag is up (a speed above 9.95 - or one component above 7.04 - was stored; it stays
        up) the pass runs on every step, and as its own full-grid launch it is three times faster than inside a boundary launch at res 4096:
        looked at between launch sequences - at the start of run() / capture_period() and every 256 eager steps (one 12-byte download)."""
        dev = self._dev
        if self._capturing():
            return            # (a user capture of step() in progress: the look is a download - it waits for the next eager step)
        self._since_hot_check = 0
        if not getattr(dev, "limit_deferral", False):
            return
        s = self._solver
        target = getattr(getattr(s, "v", None), "current", None)      # the buffer limit_field is applied to at a step boundary - the others' flags do not
        if target is not None and dev.field_hot(target):             # decide whether a pass runs (a K3+K4 output carries word [3] until it is rewritten)
            bufs = [f for f in (target, getattr(getattr(s, "v", None), "next", None), getattr(s, "_v_spare", None)) if f is not None]
            dev.stop_limit_deferral(bufs)
            self._pending_after_step = self._limit_pending()

    def _limit_pending(self):
        """What the solver's fields owe: a deferred limit_field of the velocity (runtime.DeviceBase.limit_field; after a step of the plain
        solvers - the dye solvers' boundary kernel has taken it along), a deferred clamp_inflow of the dye (DeviceBase.clamp_inflow)."""
        v, dye = getattr(self._solver, "v", None), getattr(self._solver, "dye", None)
        return (v is not None and v.current.pending_limit is not None, dye is not None and dye.current.pending_clamp is not None)

    def _counted_step(self):
        self.step()
        self._steps += 1

    # -- replay of the step as a hipGraph (new; the reference steps from a Python GUI loop) --------------------------
    def _signature(self):
        """Identity of every device buffer behind the solver's DoubleBuffers + the flags that select kernel variants: a
        captured launch sequence is valid exactly while this is what it was at capture time."""
        s, sig = self._solver, []
        for name in ("v", "p", "vx", "vy", "dye", "dyex", "dyey"):
            db = getattr(s, name, None)
            if db is not None:
                for f in (db.current, db.next):
                    # serial: a Field's identity for life (id() is recycled); static_id: which carry decisions the capture baked in
                    sig.append((f.serial, f.user_data, f.static_id, f.pending_limit, f.pending_clamp, f.bc_parity))      # (pending_limit: a deferred limit_field, runtime.DeviceBase.limit_field)
        for spare in (getattr(s, "_v_spare", None), getattr(s, "_dye_spare", None)) + tuple(getattr(s.pressure_updater, "_spare", None) or ()):
            sig.append((spare.serial, spare.static_id, spare.bc_parity) if spare is not None else 0)
        for r in self._riders():
            sig.extend(r.tokens())      # (graphs / tapes with a rider's launches in them are never replayed without it, or vice versa)
        return tuple(sig)

    _LONG_STEPS = 16     # steps per long-form graph (capture_period)
    _MAX_CACHED = 8      # captured graphs / tapes kept per simulator (one per phase of the buffer rotation; the oldest is freed first)

    def run(self, nsteps, graph=True):
        """`nsteps` x step().  With graph=True (single GPU) the launches of a whole number of steps are captured once into a
        hipGraph and replayed, so no Python runs between kernels - for small grids (res 200: 8 kernels of ~3 us per step) that
        is the difference between launch-bound and GPU-bound.  Results are identical to calling step() nsteps times.

        A graph is valid for one phase of the solver's buffer rotation (self._signature()).  A chunk that is not a multiple of the
        period ends in another phase; graphs are therefore cached per phase (at most `period` of them exist) instead of being
        re-captured - and leaked - chunk after chunk, and a capture is only started when the chunk is long enough to pay for it.

        With a history recorder (record_history) or a body tracker (track_body) attached the run is cut into chunks that fit their
        rings - the smaller room of the two - and whichever is full is drained between them: no record is ever dropped.  With a sort
        schedule for the tracer particles (seed_tracers(sort_every=K)) it is also cut at every K-th step since seed_tracers, where the
        particles are sorted between two chunks; the two cuts compose."""
        riders = self._riders()
        rings = [r for r in riders if r.room() is not None]      # (each with a device ring: room() / drain())
        cutters = [r for r in riders if r.next_cut() is not None]
        if not rings and not cutters:
            return self._run_chunk(nsteps, graph)
        while nsteps > 0:
            full = [r for r in rings if r.room() <= 0]
            if full:
                for r in full:
                    r.drain()
                continue
            m = min([nsteps] + [r.room() for r in rings] + [r.next_cut() for r in cutters])
            self._run_chunk(m, graph, reuse=bool(cutters))       # (its eager steps sort when they land on the K-th step themselves)
            nsteps -= m
            self._between_chunks()

    def _replayed(self, steps):
        for r in self._riders():
            r.replayed(steps)

    def _run_chunk(self, nsteps, graph, reuse=False):
        """reuse (the chunks a sort schedule cuts): a chunk that starts in a phase of the buffer rotation no cached graph belongs to takes
        eager steps until it reaches one that has a graph, instead of capturing a graph per phase; and a cached period without its long
        form - the first chunk was too short for it - gets it when a later chunk has the steps.  So the chunked run caches what the
        uncut run caches."""
        dev = self._dev
        self._check_hot()
        if graph and dev.nranks > 1 and nsteps >= 24:
            # slab run: a hipGraph cannot carry the RCCL exchange; the period of the step (launches + exchanges) is logged
            # once and replayed from C++ instead (runtime.py tape_period / replay_tape)
            key = (self._signature(), dev._state_signature())
            tape = self._tapes.get(key)
            if tape is None:
                before = self._steps
                # the search executes the steps it logs: at most 2 * tries of them, never more than this call was asked for (ADVICE r3:
                # with the default of 14 blocks a run(24 .. 27) that found no period took 28 steps)
                tape = dev.tape_period(self._counted_step, nsteps=2, tries=min(14, nsteps // 2))
                nsteps -= self._steps - before
                assert nsteps >= 0, "tape_period executed more steps than run() was asked for"
                if tape is not None:
                    self._remember(self._tapes, (self._signature(), dev._state_signature()), tape, lambda t: dev.free_tape(t))
            if tape is not None:
                per = tape["nsteps"]
                dev.replay_tape(tape, nsteps // per)
                self._replayed(nsteps - nsteps % per)
                self._steps += nsteps - nsteps % per
                nsteps %= per
        if not graph or dev.nranks > 1 or not hasattr(dev, "capture"):
            for _ in range(nsteps):
                self._counted_step()
            return
        if nsteps > 0 and self._eager_seen and self._limit_pending() != self._pending_after_step:
            self._counted_step()        # (the cached graphs start from the state a step leaves behind, see capture_period)
            nsteps -= 1
        entry = self._graphs.get(self._signature())
        if reuse and entry is None and self._graphs:
            seek = max(e[1] for e in self._graphs.values()) - 1
            while entry is None and seek > 0 and nsteps > 0:
                self.step()
                nsteps -= 1
                seek -= 1
                entry = self._graphs.get(self._signature())
        if reuse and entry is not None and entry[2] is None:
            gid, period = entry[:2]
            reps = -(-self._LONG_STEPS // period)
            if reps > 1 and nsteps >= reps * period:
                sig = self._signature()
                lid = dev.capture(lambda: [self._update() for _ in range(reps * period)])
                dev.replay(lid, 1)
                nsteps -= reps * period
                entry = (gid, period, (lid, reps * period))
                self._graphs[sig] = entry
        if entry is None and nsteps >= 16:          # (periods 1 - 6 need at most 16 steps to be found; 12 - an odd red-black count with the pair pass
            # on top of the fused transport - is only tried when the chunk has 28)
            nsteps -= self.capture_period(budget=nsteps)
            entry = self._graphs.get(self._signature())
        if entry is not None:
            gid, period, long = entry
            self._graph, self._graph_long = (self._signature(), gid, period), long
            if long is not None:
                dev.replay(long[0], nsteps // long[1])
                self._replayed(nsteps - nsteps % long[1])
                nsteps %= long[1]
            dev.replay(gid, nsteps // period)
            self._replayed(nsteps - nsteps % period)
            nsteps %= period
        for _ in range(nsteps):
            self.step()

    def _remember(self, cache, key, value, free):
        if key in cache:
            free(cache.pop(key))
        while len(cache) >= self._MAX_CACHED:
            free(cache.pop(next(iter(cache))))
        cache[key] = value

    def capture_period(self, budget=24):
        """Capture the launches of one PERIOD of the step into a hipGraph -> number of steps this took (they are executed).

        A replayed graph re-issues kernels on fixed device buffers, so it must cover a whole period of the solver's buffer
        rotation: 2 steps when every DoubleBuffer just swaps (two swaps restore it), 6 steps for the CIP solver with its fused
        gradient + advection pass and vorticity confinement (the velocity rotates through three buffers, the gradients and - with the
        two-iteration red-black pass - the pressure pairs through two).  Periods are tried in increasing order; a capture whose steps
        do not bring every buffer back to its place is still executed once (the host-side swaps have happened) and freed.  Leaves
        self._graph = (signature, graph id, period) - also cached for run() - or None if nothing within the budget repeats.

        Round 4: every replay of a graph costs ~5 us of GPU idle time whatever it holds (tools/r4_chain.py) - a quarter of a res-200 step
        when the graph is a 2-step period.  Where the budget allows, the same period is therefore captured a second time, repeated to
        >= 16 steps (self._graph_long = (graph id, steps)); run() and bench.py replay that one and finish with the short one."""
        dev, done = self._dev, 0
        self._check_hot()
        self._graph = self._graph_long = None
        if (not self._eager_seen or self._limit_pending() != self._pending_after_step) and budget >= 2:
            # (also: the steady state of a run with deferred limit passes starts every step with one pending - after a download there is
            #  none, and a period captured from there would not close)
            # libfs_hip builds the compact tile lists of a launch geometry the first time the geometry is launched EAGERLY (building one
            # synchronises the stream, which a capture forbids): a graph captured before any eager step would carry the dense launches for
            # life.  One eager step first - it counts as one of the steps this call takes.
            self.step()
            done = 1
        for period in (1, 2, 3, 4, 6, 12):
            if done + period > budget:
                break
            sig = self._signature()
            gid = dev.capture(lambda: [self._update() for _ in range(period)])       # host-side swaps happen, nothing executes
            back = self._signature() == sig
            dev.replay(gid, 1)                                                    # now the captured steps run once
            done += period
            if back:
                long, reps = None, -(-self._LONG_STEPS // period)
                if reps > 1 and done + reps * period <= budget:
                    lid = dev.capture(lambda: [self._update() for _ in range(reps * period)])
                    dev.replay(lid, 1)
                    done += reps * period
                    long = (lid, reps * period)
                self._remember(self._graphs, sig, (gid, period, long), lambda e: [dev.free_graph(e[0])] + ([dev.free_graph(e[2][0])] if e[2] else []))
                self._graph, self._graph_long = (sig, gid, period), long
                break
            dev.free_graph(gid)
        return done

    def field_to_numpy(self):
        fields = self._solver.get_fields()
        return {"v": fields[0].to_numpy(), "p": fields[1].to_numpy()}

    # -- diagnostics (new; the reference's user watches the window instead) ----------------------------------------------
    def pressure_residual(self):
        """rms over the not-wall cells of predict_p(p) - p for the fields get_fields() returns (include/fs_hip.h fs_poisson_residual): how far
        the pressure is from solving its own equation.  A download: not inside a graph capture."""
        self._not_capturing("pressure_residual")
        v, p = self._solver.get_fields()[:2]
        s, n = self._dev.poisson_residual(self._solver.dt, self._solver.dx, p, v)
        return math.sqrt(s / n) if n > 0 else 0.0

    def flow_stats(self, body_box=None):
        """Scalar diagnostics of the fields get_fields() returns, computed on the GPU in one pass (include/fs_hip.h fs_flow_stats):
          kinetic_energy = 0.5 dx^2 sum_F (u^2 + w^2)     enstrophy = 0.5 dx^2 sum_F omega^2 (central differences)
          max_speed, cfl = max_F (|u| + |w|) dt / dx     div_rms, div_max: central-difference divergence over the fluid cells
          nonfinite: not-wall cells whose u, w or p is NaN or +-Inf (a blown-up run also shows NaN / Inf in the other values)
          fluid_cells; and with body_box = (x0, y0, x1, y1) (global cells, half-open; fs.boundary_condition.default_body_box gives one
          per obstacle scene) force_x / force_y: the PRESSURE force per unit depth on the wall cells inside the box, summed over the faces
          they share with fluid cells.  The viscous part is not in these two numbers: body_snapshot() / track_body() give the friction
          force, the moment and the distributions along the surface (at -re 100 about a fifth of a cylinder's drag is friction).
        Changes nothing the trajectory depends on: no field, no swap, no captured graph (a deferred limit_field of v stays deferred unless
        it would change a cell, runtime.DeviceBase.flow_stats).  Not allowed during a graph capture."""
        s = self._solver
        v, p = s.get_fields()[:2]
        return derive_flow_stats(self._dev.flow_stats(s.dx, v, p, body_box), s.dx, s.dt, body_box is not None)

    # -- per-step history (new): probe values and the pressure force on a body, recorded on the device -----------------------------
    def record_history(self, probes=(), body_box=None, every=1, capacity=None, start_step=0):
        """From the next step on, record after every step k (counted from here, k = 1, 2, ...) with k % every == 0: u, w and p at the
        fluid cells `probes` = [(x, y), ...] and, with body_box = (x0, y0, x1, y1), the pressure force on the body as flow_stats(body_box)
        computes it - gathered by one small launch per step that is captured into the replayed graphs (and recorded into slab tapes), into
        a device ring of `capacity` records (default: 16 MB of them, at least 64) that run() drains between chunks.  Record k is numbered
        start_step + k.  Changes no field and no trajectory; a recorder already attached is stopped first.  history() returns the records.
        Not allowed during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("record_history")
        every, _ = self._cadence(every)
        mask = s._bc.mask
        pts = check_probes(mask, probes)
        if body_box is not None:
            body_box = tuple(int(b) for b in body_box)
            faces = body_faces(mask, body_box)
        else:
            faces = np.zeros((0, 3), np.int32)
        if len(pts) == 0 and body_box is None:
            raise ValueError("record_history needs probes, a body_box or both")
        if capacity is None:
            capacity = max(64, (16 << 20) // (8 * (2 + 3 * len(pts))))
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        self._make_way("_recorder")
        hist = dev.history_create(pts, faces, int(capacity), every)
        self._recorder = Recorder(dev, hist, pts, body_box, every, start_step, s.dt)
        self._last_recorder = None

    def history(self):
        """Everything recorded since record_history(): {"step": int64[n], "time": f64[n] (step * dt), "probes": int32[P, 2],
        "u", "w", "p": f64[n, P], and with a body box "force_x", "force_y": f64[n]}.  Drains the device ring (a download)."""
        rec = self._recorder or self._last_recorder
        if rec is None:
            raise RuntimeError("no history: call record_history() first")
        if rec is self._recorder:
            rec.drain()
        return rec.data()

    def stop_history(self):
        """Drain and detach the recorder: the cached graphs and tapes that hold its launch are freed, then its device ring.  history() still
        returns what it recorded until the next record_history()."""
        self._detach(self, "_recorder", "stop_history")

    def _make_way(self, attr, refusal=None):
        """An attach call that finds a rider of its kind attached: its replaces_attached says whether it is stopped or the call refused."""
        r = getattr(self, attr)
        if r is not None:
            if not r.replaces_attached:
                raise RuntimeError(refusal)
            self._detach(self, attr, None)

    def _detach(self, owner, attr, name):
        """The stop_* methods: drain the rider owner.<attr>, free the cached graphs and tapes that hold its launches, then its device objects.
        Its class says whether this may happen inside a graph capture (stop_in_capture: no graph can be freed there - theirs stay cached,
        never matched again - and the device memory is released when the capture ends) and whether it stays as _last<attr> (keeps_last)."""
        r = getattr(owner, attr)
        if r is None:
            return
        capturing = self._capturing()
        if capturing and not r.stop_in_capture:
            raise RuntimeError(f"{name} during a graph capture")
        try:
            r.drain()
            r.close()
        finally:
            if not capturing:
                for tok in r.tokens():
                    self._drop_cached(tok)
            r.free()
            setattr(owner, attr, None)
            if r.keeps_last:
                setattr(owner, "_last" + attr, r)

    def _drop_cached(self, tok):
        """Free the cached graphs and tapes whose signature holds `tok` (they contain a launch on a device object about to be freed)."""
        dev = self._dev
        for sig in [k for k in self._graphs if tok in k]:
            gid, _, long = self._graphs.pop(sig)
            dev.free_graph(gid)
            if long is not None:
                dev.free_graph(long[0])
        for key in [k for k in self._tapes if tok in k[0]]:
            dev.free_tape(self._tapes.pop(key))
        if self._graph is not None and tok in self._graph[0]:
            self._graph = self._graph_long = None

    # -- body surface loads (new): pressure + viscous force, moment, per-face pressure and wall shear statistics ---------------------------
    def _body_faces(self, body_box, center):
        mask = self._solver._bc.mask
        body_box = tuple(int(b) for b in body_box)
        if len(body_box) != 4:
            raise ValueError("body_box must be (x0, y0, x1, y1)")
        faces = body_faces(mask, body_box)
        if len(faces) == 0:
            raise ValueError(f"body box {body_box} holds no face between a wall cell and a fluid cell")
        centre = body_centroid(mask, body_box) if center is None else tuple(float(c) for c in np.asarray(center, np.float64).ravel())
        if len(centre) != 2 or not all(np.isfinite(c) for c in centre):
            raise ValueError("center must be two finite numbers (cx, cy) in cell units")
        return body_box, faces, centre

    def track_body(self, body_box, center=None, every=1, start_step=0, capacity=None):
        """From the next step on, sample the loads on the body in body_box = (x0, y0, x1, y1) after every step k (counted from here,
        k = 1, 2, ...) with k > start_step and (k - start_step) % every == 0: the pressure force (the faces and terms of flow_stats), the
        VISCOUS force - per face inv_re * u_t, the wall shear tau = u_t / (re dx) times the face length dx, with u_t the fluid cell's
        tangential velocity: the no-slip point is the centre of the wall cell, one dx away, the distance the solver's own Laplacian uses -
        and the moments of both about `center` (cell units; default: fs.loads.body_centroid), positive counter-clockwise.  Each sample
        also adds p, p^2, tau, tau^2 of every face to per-face sums on the device (32 bytes per face).  The launches go behind the history
        and average launches of the step, are captured into the replayed graphs (and recorded into slab tapes), and write 6 doubles per
        sample into a device ring of `capacity` records (default 65536) that run() drains between chunks.  Changes no field and no
        trajectory.  body_loads() returns the series, body_surface() the distributions.  Raises while a tracker is attached already; not
        allowed during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("track_body")
        self._make_way("_tracker", "a body tracker is attached already: stop_body() first")
        every, start_step = self._cadence(every, start_step)
        capacity = 65536 if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        body_box, faces, centre = self._body_faces(body_box, center)
        lo = dev.loads_create(faces, centre, capacity, every, start_step)
        self._tracker = Tracker(dev, lo, faces, body_box, centre, every, start_step, s.dt)
        self._last_tracker = None

    def _body(self):
        bt = self._tracker or self._last_tracker
        if bt is None:
            raise RuntimeError("no body tracker: call track_body() first")
        if bt is self._tracker:
            self._not_capturing("body_loads / body_surface")
            bt.drain()
        return bt

    def body_loads(self):
        """Every sample since track_body(): {"step": int64[n], "time" (step * dt), "pressure_x", "pressure_y", "viscous_x", "viscous_y",
        "force_x", "force_y" (pressure + viscous), "moment_pressure", "moment_viscous", "moment": f64[n]} - forces and moments per unit
        depth at density 1.  Drains the device ring (a download)."""
        return self._body().data()

    def body_surface(self):
        """The distributions along the surface: {"faces": int32 (F, 3), "x", "y" (face midpoints, cell units), "nx", "ny" (normal wall ->
        fluid), "theta" (angle of the midpoint about the centre), "p_mean", "p_rms", "tau_mean", "tau_rms": f64 (F,) over the samples so far
        (rms: root of the central second moment, clipped at 0; NaN before the first sample), "samples", "sums": the raw (4, F) S_p, S_pp,
        S_t, S_tt}.  fs.loads.pressure_coefficient / skin_friction turn them into Cp and Cf."""
        return self._body().surface()

    def reset_body_surface(self):
        """Per-face sums and sample count back to zero; the step count (the phase of `every` / `start_step`) and the series run on."""
        if self._tracker is None:
            raise RuntimeError("no body tracker: call track_body() first")
        self._not_capturing("reset_body_surface")
        self._tracker.drain()
        self._dev.loads_reset(self._tracker.loads)
        self._tracker.samples = 0

    def stop_body(self):
        """Drain and detach the body tracker: the cached graphs and tapes that hold its launches are freed, then its device memory.
        body_loads() and body_surface() still return what it gathered until the next track_body()."""
        self._detach(self, "_tracker", "stop_body")

    def body_snapshot(self, body_box, center=None):
        """The loads of the fields as they are now: the keys of body_loads() without step / time as floats, plus "faces", "x", "y", "nx",
        "ny", "theta" and the per-face "p" and "tau".  One temporary tracker, one eager launch, a read and a free: changes no field, no
        graph and no attached tracker, and leaves a deferred limit_field deferred (the kernel limits the values it reads).  Not allowed
        during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("body_snapshot")      # (before the box is looked at)
        body_box, faces, centre = self._body_faces(body_box, center)
        v, p = s.get_fields()[:2]

        def read(lo):
            one = Tracker(dev, lo, faces, body_box, centre, 1, 0, s.dt)
            one.drain()
            return one.data(), one.sums()
        (data, sums), _ = self._once("body_snapshot", lambda: dev.loads_create(faces, centre, 1, 1, 0),
                                     lambda lo: dev.loads_record(lo, s.dx, 1.0 / s.re, v, p), read, dev.loads_free)
        out = {k: float(a[0]) for k, a in data.items() if k not in ("step", "time")}
        out["faces"] = faces.copy()
        out.update(face_geometry(faces, centre))
        out["p"], out["tau"] = sums[0].copy(), sums[2].copy()
        return out

    # -- time averages (new): means and second moments of u, w, p accumulated on the device -------------------------------------------
    def start_averaging(self, every=1, start_step=0):
        """From the next step on, add u, w, p and their products uu, ww, uw, pp of every not-wall cell to double sums on the device after
        every step k (counted from here, k = 1, 2, ...) with k > start_step and (k - start_step) % every == 0.  The launch is part of the
        step: it is captured into the replayed graphs and recorded into slab tapes, and run() is not cut into chunks by it.  Costs 56 bytes
        per cell of device memory, and a sampling step moves more bytes for the sums than for the flow (choose `every` accordingly).
        Changes no field and no trajectory.  averages() returns the result.  Raises while an average is attached already; not allowed during
        a graph capture."""
        dev = self._dev
        self._not_capturing("start_averaging")
        self._make_way("_averager", "an average is attached already: stop_averaging() first (or reset_averages())")
        every, start_step = self._cadence(every, start_step)
        self._averager = Averager(dev, dev.mean_create(every, start_step), every, start_step)

    def _avg(self):
        return self._attached("_averager", "average", "start_averaging")

    def averages(self, local=False):
        """The averages so far (a download of 56 bytes per cell): {"samples": int, "steps": int (steps since start_averaging), "u", "w",
        "p": means, "uu", "ww", "uw": central second moments <a b> - <a><b> (the Reynolds stresses), "p_rms", "tke": 0.5 (uu + ww),
        "mask"}: float64 arrays of shape (X, Y) (mask: uint8), wall cells 0 (fs.averages.derive_averages).  On slabs the global arrays are
        assembled on every rank (collective); local=True: this rank's owned rows only.  Raises while there is no sample."""
        avg = self._avg()
        dev = self._dev
        sums, launches, samples = dev.mean_read(avg.mean, local=local)
        if samples == 0:
            raise RuntimeError(f"no samples yet ({launches} steps since start_averaging(every={avg.every}, start_step={avg.start_step}))")
        mask = np.asarray(self._solver._bc.mask)
        if local:
            mask = mask[:, dev.y0:dev.y0 + dev.nyl]
        out = {"samples": samples, "steps": launches}
        out.update(derive_averages(sums, samples, mask))
        out["mask"] = mask.copy()
        return out

    def mean_fields(self):
        """The mean flow as device fields (v: 2 channels, p: 1 channel; wall cells 0), for everything that takes fields: the visualisation
        kernels, to_numpy, DeviceBase.flow_stats.  New fields on every call; the caller owns them."""
        from ._lib import FsError
        from .runtime import Field
        avg = self._avg()
        dev = self._dev
        if self._capturing():
            raise FsError("mean_fields / mean_flow_stats during a graph capture: they allocate and download")
        v, p = Field(dev, 2), Field(dev, 1)      # (not dev.alloc: scratch fields stay out of the ghost-row bookkeeping state of the tapes)
        dev.mean_finalize(avg.mean, v, p)
        return v, p

    def mean_flow_stats(self, body_box=None):
        """flow_stats() of the MEAN flow: the kinetic energy of the mean motion, the mean pressure force on a body ... (the CFL number and
        the divergence of a mean field are diagnostics of the average, not of a step).  Not allowed during a graph capture."""
        s = self._solver
        v, p = self.mean_fields()
        return derive_flow_stats(self._dev.flow_stats(s.dx, v, p, body_box), s.dx, s.dt, body_box is not None)

    def reset_averages(self):
        """Sums and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._dev.mean_reset(self._avg().mean)

    def stop_averaging(self):
        """Detach the average and free its device memory; the cached graphs and tapes that hold its launch are freed first.  Nothing is kept
        on the host: call averages() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_averager", "stop_averaging")

    # -- harmonic flow modes (new): Fourier sums of u, w, p at chosen frequencies accumulated on the device ---------------------------------
    def start_modes(self, frequencies, every=1, start_step=0):
        """From the next step on, accumulate the harmonic content of u, w and p at `frequencies` (1 to 4 distinct positive values, in 1 /
        simulated time - history() and fs.history.dominant_frequency give the shedding frequency) in every not-wall cell: after every step k
        (counted from here) with k > start_step and (k - start_step) % every == 0 the fields, multiplied by 1 and by the cosine and sine of
        each frequency's phase, are added to double sums on the device (fs.modes; csrc/fs_modes.h).  The launch is part of the step: it is
        captured into the replayed graphs and recorded into slab tapes, and run() is not cut into chunks by it.  Costs 24 (1 + 2K) bytes
        per cell of device memory (72 for one frequency, 216 for four), and a sampling step moves 16 (3 + 6K) bytes per cell for the sums:
        choose `every` accordingly - ValueError when a frequency reaches the Nyquist limit f every dt >= 0.5.  Changes no field and no
        trajectory.  modes() returns the fit, mode_fields() the phase-averaged flow as fields.  Raises while modes are attached already;
        not allowed during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("start_modes")
        self._make_way("_moder", "modes are attached already: stop_modes() first (or reset_modes())")
        every, start_step = self._cadence(every, start_step)
        cd, sd = phasor_steps(frequencies, every, s.dt)
        freqs = np.atleast_1d(np.asarray(frequencies, np.float64))
        self._moder = Modes(dev, dev.modes_create(np.stack([cd, sd], axis=1), every, start_step), freqs, every, start_step)

    def _modes(self):
        return self._attached("_moder", "modes", "start_modes")

    def modes(self, local=False):
        """The fit so far (a download of 24 (1 + 2K) bytes per cell): {"frequencies", "samples": int, "steps": int (steps since start_modes),
        "u", "w", "p": {"mean": (X, Y), "cos", "sin", "amplitude", "phase": (K, X, Y)} (fs.modes.fit: the signal at a cell is mean +
        sum_k amplitude[k] cos(theta_k - phase[k]), theta_k = 2 pi f_k (t - time of the first sample); wall cells 0), "sums": the raw planes
        (3 (1 + 2K), X, Y), "gram": the Gram matrix of the applied basis, "mask"}.  On slabs the global arrays are assembled on every rank
        (collective); local=True: this rank's owned rows only.  Raises while there are fewer samples than the 1 + 2K unknowns."""
        mo = self._modes()
        dev = self._dev
        sums, scalars, launches, samples = dev.modes_read(mo.modes, local=local)
        K = len(mo.frequencies)
        if samples < 1 + 2 * K:
            raise RuntimeError(f"{samples} samples yet, {1 + 2 * K} needed ({launches} steps since start_modes(every={mo.every}, "
                               f"start_step={mo.start_step}))")
        mask = np.asarray(self._solver._bc.mask)
        if local:
            mask = mask[:, dev.y0:dev.y0 + dev.nyl]
        out = {"frequencies": mo.frequencies.copy(), "samples": samples, "steps": launches}
        out.update(fit_modes(sums, scalars, K, mask))
        out["sums"], out["gram"], out["mask"] = sums, gram_matrix(scalars, K), mask.copy()
        return out

    def mode_fields(self, phase=None, frequency=0):
        """The phase-averaged flow as device fields (v: 2 channels, p: 1 channel; wall cells 0): the fitted mean plus the component of
        frequency number `frequency` at `phase` (radians; 0 is the phase of the first sample); phase=None: the fitted mean alone.  For
        everything that takes fields - the visualisation kernels, to_numpy, DeviceBase.flow_stats - as mean_fields().  One device pass over
        the planes (fs_modes_combine), no download of them.  New fields on every call; the caller owns them."""
        from ._lib import FsError
        from .runtime import Field
        mo = self._modes()
        dev = self._dev
        if self._capturing():
            raise FsError("mode_fields during a graph capture: it allocates and downloads")
        K = len(mo.frequencies)
        frequency = int(frequency)
        if not 0 <= frequency < K:
            raise ValueError(f"frequency must be an index in 0 .. {K - 1}")
        _, scalars, launches, samples = dev.modes_read_scalars(mo.modes)
        if samples < 1 + 2 * K:
            raise RuntimeError(f"{samples} samples yet, {1 + 2 * K} needed ({launches} steps since start_modes)")
        phases = None if phase is None else [float(phase) if k == frequency else None for k in range(K)]
        w = reconstruct_weights(scalars, K, phases)
        v, p = Field(dev, 2), Field(dev, 1)      # (not dev.alloc: scratch fields stay out of the ghost-row bookkeeping state of the tapes)
        dev.modes_combine(mo.modes, np.tile(w, (3, 1)), v, p)
        return v, p

    def reset_modes(self):
        """Sums, Gram matrix and sample count back to zero, the phase back to 0; the step count and the phase of `every` / `start_step` run on."""
        self._dev.modes_reset(self._modes().modes)

    def stop_modes(self):
        """Detach the modes and free their device memory; the cached graphs and tapes that hold their launch are freed first.  Nothing is
        kept on the host: call modes() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_moder", "stop_modes")

    # -- snapshot POD (new): the last M sampled fields resident on the device, their Gram matrix reduced there ------------------------------
    def start_pod(self, snapshots, every=1, start_step=0):
        """From the next step on, keep the last `snapshots` = M (2 .. 64) sampled flow fields resident on the device: after every step k
        (counted from here) with k > start_step and (k - start_step) % every == 0 the fields u, w, p are copied into slot number
        (samples % M) of a ring (csrc/fs_pod.h; wall cells 0).  The launch is part of the step: it is captured into the replayed graphs,
        decides on the device whether it samples, and run() is not cut into chunks by it.  Costs 12 M bytes per cell of device memory in f32,
        24 M in f64 (res 4096: 403 MB per snapshot).  Changes no field and no trajectory.  pod() returns the proper orthogonal decomposition
        of the resident snapshots - energies, temporal coefficients, mode weights - from their M x M Gram matrix, which is reduced on the
        device; pod_fields() the modes as fields.  Raises while a POD is attached already and during a graph capture; single-GPU contexts
        only (FsError on slabs: the Gram matrix would need a rank-ordered reduction)."""
        dev = self._dev
        self._not_capturing("start_pod")
        self._make_way("_podr", "a POD is attached already: stop_pod() first (or reset_pod())")
        every, start_step = self._cadence(every, start_step)
        self._podr = Pod(dev, dev.pod_create(snapshots, every, start_step), every, start_step)

    def _pod(self):
        return self._attached("_podr", "POD", "start_pod")

    def pod(self, n_modes=None, subtract_mean=True):
        """The proper orthogonal decomposition of the n resident snapshots (fs.pod.decompose; the download is the n x n Gram matrix alone):
        {"gram": (n, n) raw, chronological; "energies": eigenvalues descending, (r,) with r the numerical rank; "fraction": energies / their
        sum; "coefficients": (n, k), a_j(m) = sqrt(lambda_j) V[m, j], chronological, k = min(n_modes, r) (n_modes=None: r); "weights":
        (k, n) in SLOT order - mode j is sum_m weights[j, m] * slot m (what pod_fields(j) evaluates); "sample_steps": the step of every
        resident sample, chronological; "samples", "steps": samples and steps since start_pod / reset_pod}.  subtract_mean: decompose the
        fluctuations about the mean of the resident snapshots (the usual POD of a wake) instead of the raw snapshots.  Raises while fewer
        than 2 samples are resident; not allowed during a graph capture."""
        a = self._pod().analyse(subtract_mean)
        k = len(a["energies"]) if n_modes is None else max(0, min(int(n_modes), len(a["energies"])))
        w = np.zeros((k, len(a["slots"])))
        w[:, a["slots"]] = a["weights"][:k]
        return {"gram": a["gram"].copy(), "energies": a["energies"].copy(), "fraction": a["fraction"].copy(),
                "coefficients": a["coefficients"][:, :k].copy(), "weights": w, "sample_steps": a["sample_steps"].copy(),
                "samples": a["samples"], "steps": a["steps"]}

    def _pod_combine(self, chronological):
        from ._lib import FsError
        from .runtime import Field
        po = self._pod()
        dev = self._dev
        if self._capturing():
            raise FsError("pod_fields / pod_snapshot during a graph capture: they allocate and download")
        w = po.slot_weights(chronological)
        v, p = Field(dev, 2), Field(dev, 1)      # (not dev.alloc: scratch fields stay out of the ghost-row bookkeeping state of the tapes)
        dev.pod_combine(po.pod, w, v, p)
        return v, p

    def pod_fields(self, k=None, subtract_mean=True):
        """POD mode k (0: the most energetic) as device fields (v: 2 channels, p: 1 channel; wall cells 0): the combination of the resident
        snapshots with pod()["weights"][k] - p is the extended mode, the same combination of the pressure planes.  k=None: the mean of the
        resident snapshots.  One device pass over the slots (fs_pod_combine), no download of them.  For everything that takes fields - the
        visualisation kernels, to_numpy, DeviceBase.flow_stats - as mean_fields().  New fields on every call; the caller owns them."""
        a = self._pod().analyse(subtract_mean)
        n = len(a["slots"])
        if k is None:
            return self._pod_combine(np.full(n, 1.0 / n))
        k = int(k)
        if not 0 <= k < len(a["energies"]):
            raise ValueError(f"mode must be an index in 0 .. {len(a['energies']) - 1} (the numerical rank of the {n} snapshots)")
        return self._pod_combine(a["weights"][k])

    def pod_snapshot(self, m):
        """Resident sample m (0: the oldest; negative: from the newest) as device fields (v, p): a unit weight through fs_pod_combine."""
        po = self._pod()
        if self._capturing():
            from ._lib import FsError
            raise FsError("pod_fields / pod_snapshot during a graph capture: they allocate and download")
        _, samples = self._dev.pod_read(po.pod)
        n = min(samples, po.pod.slots)
        m = int(m)
        if not -n <= m < n:
            raise IndexError(f"sample {m}: {n} samples are resident")
        w = np.zeros(n)
        w[m] = 1.0
        return self._pod_combine(w)

    def reset_pod(self):
        """Slots and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._pod().reset()

    def stop_pod(self):
        """Detach the POD and free its device memory; the cached graphs that hold its launch are freed first.  Nothing is kept on the host:
        call pod() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_podr", "stop_pod")

    # -- vortex identification (new): criterion, labelled components and per-vortex records, on the device ----------------------------------
    def _vortex_create(self, threshold, criterion, every, start_step, min_area, max_vortices, max_components, omega_max, capacity):
        s = self._solver
        if threshold is None:
            raise ValueError("threshold must be given (1 / time^2): see track_vortices")
        if omega_max is None:
            omega_max = 2.0 * VELOCITY_LIMIT / s.dx
        if capacity is None:
            capacity = max(16, (16 << 20) // (8 * (8 + 16 * int(max_vortices))))
        return self._dev.vortex_create(criterion, threshold, omega_exponent(omega_max), every, start_step, min_area, max_vortices, max_components,
                                       int(capacity))

    def track_vortices(self, threshold, criterion="q", every=1, start_step=0, min_area=4, max_vortices=64, max_components=65536, omega_max=None,
                       capacity=None):
        """From the next step on, identify the vortices after every step k (counted from here, k = 1, 2, ...) with k > start_step and
        (k - start_step) % every == 0, on the device (csrc/fs_vortex.h): a cell is part of a vortex when it is fluid and its criterion c
        exceeds `threshold`; the 4-connected cells of equal rotation sense form a component; every component of at least `min_area` cells
        becomes a record - the first `max_vortices` (at most 1024) in order of their label, the smallest j * X + i of the component - in a
        device ring of `capacity` samples (default: 16 MB of them) that run() drains between chunks.

        criterion, in 1 / time^2 with the central differences of flow_stats: "q" - Q = -(ux^2 + wy^2) / 2 - uy wx, positive where rotation
        outweighs strain; "swirl" - lambda_ci^2 = (ux wy - uy wx) - (ux + wy)^2 / 4, positive where the velocity gradient has complex
        eigenvalues; "vorticity" - om^2.  threshold has no default: with U the free-stream speed and L the size of the body, gradients in
        the wake are of order U / L, so start from a fraction of (U / L)^2 - 0.1 (U / L)^2 for "q" and "swirl" keeps the cores and drops the
        shear layers, for "vorticity" take 1 (U / L)^2 - and look at vortex_criterion() to refine it.  A threshold of 0 flags half the domain.

        The records hold integer sums (vorticity in units of 2^(e - 30), e = ceil(log2(omega_max)); omega_max defaults to 2 * 10 / dx, the
        bound of a limited velocity field; cells beyond it are clamped and counted in `clipped`): they do not depend on the order of the
        device's atomics, and a resumed run continues them exactly.  At most `max_components` components are reduced per sample (those of
        smallest label; the cells of the others are counted in `dropped_cells`).  The launches go behind every other rider's, are captured
        into the replayed graphs, and change no field and no trajectory.  9 bytes per cell of device memory.  Raises while a tracker is
        attached already and during a graph capture; single-GPU contexts.  Out of scope: slabs, 8-connectivity, three dimensions."""
        self._not_capturing("track_vortices")
        self._make_way("_vortexr", "a vortex tracker is attached already: stop_vortices() first")
        every, start_step = self._cadence(every, start_step)
        s = self._solver
        vx = self._vortex_create(threshold, criterion, every, start_step, min_area, max_vortices, max_components, omega_max, capacity)
        self._vortexr = Vortices(self._dev, vx, every, start_step, s.dt, s.dx)
        self._last_vortexr = None

    def vortices(self):
        """Every sample since track_vortices().  Per sample: "step", "time" (step * dt), "components" (roots found), "passed" (those of at
        least min_area cells), "count" (records written), "clipped", "dropped_cells".  Per record, flat over the samples in (sample, label)
        order: "sample" (index into the per-sample arrays), "label", "sign" (+1: counter-clockwise), "area" (cells), "circulation", "x", "y"
        (|om|-weighted centroid, cell units: the centre of cell i is i + 0.5), "xg", "yg" (geometric centroid), "peak_omega", "peak_cell",
        "bbox" (xmin, ymin, xmax, ymax, inclusive).  "raw": the integers of every record (fs.vortices.RECORD), "exponent": e.
        fs.vortices.convert documents the order of every conversion.  Drains the device ring (a download)."""
        r = self._vortexr or self._last_vortexr
        if r is None:
            raise RuntimeError("no vortex tracker: call track_vortices() first")
        if r is self._vortexr:
            self._not_capturing("vortices")
            r.drain()
        return r.data()

    def stop_vortices(self):
        """Drain and detach the vortex tracker: the cached graphs that hold its launches are freed, then its device memory.  vortices() and
        vortex_labels() still return what it gathered until the next track_vortices()."""
        if self._vortexr is not None:
            self._found_planes = None
        self._detach(self, "_vortexr", "stop_vortices")

    def find_vortices(self, threshold, criterion="q", min_area=4, max_vortices=64, max_components=65536, omega_max=None):
        """The vortices of the fields as they are now: what vortices() returns, with one sample whose "step" and "time" are 0 (the call
        counts no steps).  One temporary tracker, one eager launch sequence, a read and a free: changes no field,
        no graph and no attached tracker, and leaves a deferred limit_field deferred.  vortex_labels() returns its planes until the next
        call.  Not allowed during a graph capture."""
        dev, s = self._dev, self._solver

        def read(vx):
            words, _, _ = dev.vortex_read(vx)
            self._found_planes = dev.vortex_labels(vx)
            return words
        words, vx = self._once("find_vortices", lambda: self._vortex_create(threshold, criterion, 1, 0, min_area, max_vortices, max_components, omega_max, 1),
                               lambda vx: dev.vortex_launch(vx, s.dx, s.get_fields()[0]), read, dev.vortex_free)
        return assemble(words, vx.max_vortices, vx.exponent, s.dx, dev.nx, np.zeros(len(words), np.int64), s.dt)

    def vortex_labels(self):
        """{"flags": uint8 (X, Y) - 1: om >= 0, 2: om < 0, 0: no vortex; "labels": int32 (X, Y) - the smallest j * X + i of the cell's
        component, -1 without a flag} of the attached tracker's last sample; without one, of the last find_vortices() or stopped tracker,
        whichever is the more recent."""
        self._not_capturing("vortex_labels")
        if self._vortexr is not None:
            return self._vortexr.planes()
        if self._found_planes is not None:
            return self._found_planes
        if self._last_vortexr is None:
            raise RuntimeError("no labels: call track_vortices() or find_vortices() first")
        return self._last_vortexr.planes()

    def vortex_criterion(self, criterion="q"):
        """The criterion field of the current velocity, float64 (X, Y), 0 on cells that are not fluid: what track_vortices compares with its
        threshold.  Not allowed during a graph capture."""
        self._not_capturing("vortex_criterion")
        s = self._solver
        return self._dev.vortex_criterion(criterion, s.dx, s.get_fields()[0])

    # -- field distributions (new): histograms accumulated on the device, exact quantiles of the current fields ----------------------------------
    def start_distributions(self, channels, every=1, start_step=0):
        """From the next step on, accumulate histograms of the flow over the fluid cells on the device (csrc/fs_dist.h): after every step k
        (counted from here) with k > start_step and (k - start_step) % every == 0 every channel's table of 64-bit counters takes one count
        per selected cell.  channels: one dict or a list of 1 to 4, each {"quantity", "bins", "range"[, "box"][, "against": {"quantity",
        "bins", "range"}]} - quantity one of "u", "w", "p", "speed", "vorticity", "q", "swirl" (the last three as vortex_criterion() and
        flow_stats() difference them); bins 1 .. 4096 over range = (lo, hi), half-open, required: the bins do not move during a run; box =
        (x0, y0, x1, y1) in global cells, half-open (default: the whole grid); against: a second quantity for a joint table of bins x bins
        <= 4096.  The launches are part of the step: they are captured into the replayed graphs, decide on the device whether they sample,
        and run() is not cut into chunks by them.  Counts are integers: identical between eager steps, replayed graphs and resumed runs.
        8 bytes per bin of device memory.  Changes no field and no trajectory.  distributions() returns the tables.  Raises while
        distributions are attached already and during a graph capture; single-GPU contexts only (FsError on slabs)."""
        dev = self._dev
        self._not_capturing("start_distributions")
        self._make_way("_distr", "distributions are attached already: stop_distributions() first (or reset_distributions())")
        every, start_step = self._cadence(every, start_step)
        self._distr = _dist.Distributions(dev, dev.dist_create(channels, every, start_step), every, start_step)

    def _dist(self):
        return self._attached("_distr", "distributions", "start_distributions")

    def distributions(self):
        """The tables so far, one dict per channel: {"counts": int64 (B,) or (Ba, Bb), "below", "above" (joint: "outside"), "nan",
        "edges" (joint: and "edges_b"), "samples", "sample_steps", "quantity" (joint: a pair), "box"}.  fs.dist.density / cdf / moments /
        quantile_from_counts work on a 1-D dict.  A download of the tables; not allowed during a graph capture."""
        self._not_capturing("distributions")
        return self._dist().data()

    def reset_distributions(self):
        """Tables and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._not_capturing("reset_distributions")
        self._dist().reset()

    def stop_distributions(self):
        """Detach the distributions and free their device memory; the cached graphs that hold their launches are freed first.  Nothing is
        kept on the host: call distributions() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_distr", "stop_distributions")

    def histogram(self, quantity, bins, range=None, box=None, against=None):
        """The histogram of the fields as they are now: the dict distributions() returns for one channel, with "samples" 1 and "sample_steps"
        [0] (the call counts no steps).  One temporary object, one eager launch, a read and a free: changes no field, no graph and no
        attached rider, and leaves a deferred limit_field deferred.  range=None (1-D only): the exact minimum and maximum of the values
        (order_statistics ranks 0 and n - 1) give [min, nextafter(max, +inf)) - ValueError when either is infinite or no value is there.
        Not allowed during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("histogram")      # (before order_statistics would refuse under its own name)
        if range is None:
            if against is not None:
                raise ValueError("range=None is for 1-D histograms: a joint table needs both ranges")
            n = self.order_statistics(quantity, (), box)["n"]
            if n == 0:
                raise ValueError(f"no selected cell holds a value of {quantity!r}: there is no range to take")
            lo, hi = self.order_statistics(quantity, (0, n - 1), box)["values"]
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"the values of {quantity!r} reach ({lo}, {hi}): give a finite range")
            range = (float(lo), math.nextafter(float(hi), math.inf))
        spec = {"quantity": quantity, "bins": bins, "range": range, "box": box, "against": against}
        (counts, tails, _, samples), d = self._once("histogram", lambda: dev.dist_create(spec, 1, 0), lambda d: dev.dist_launch(d, s.dx, *s.get_fields()[:2]),
                                                    lambda d: dev.dist_read(d, 0), dev.dist_free)
        return _dist.result(dev, d.channels[0], counts, tails, samples, np.zeros(samples, np.int64))

    def order_statistics(self, quantity, ranks, box=None):
        """Exact order statistics of the fields as they are now: {"values": float64 (R,), the ranks[k]-th smallest (0-based, ascending, at
        most 8 per call) of the values of `quantity` over the fluid cells of `box` that are not NaN - exactly what np.sort would put there;
        "n": how many such values; "nan": selected cells whose value is NaN}.  A radix select on the device over a plane of 8 bytes per
        cell of the box that lives for the call; no field is downloaded.  ValueError for a rank >= n.  Changes nothing, leaves a deferred
        limit_field deferred.  Not allowed during a graph capture."""
        self._not_capturing("order_statistics")
        s = self._solver
        v, p = s.get_fields()[:2]
        values, n, nan = self._dev.dist_select(quantity, box, s.dx, v, p, ranks)
        return {"values": values, "n": n, "nan": nan}

    def quantile(self, quantity, q, box=None, method="linear"):
        """Quantiles of `quantity` over the fluid cells of `box`, from exact order statistics: q a scalar or a sequence in [0, 1] -> float or
        float64 array.  With pos = (n - 1) * q as a Python float, a and b the order statistics at floor(pos) and the next rank and g the
        fractional part: method "lower" a, "higher" b, "nearest" the closer one, "linear" a + (b - a) * g - "lower" / "higher" are
        np.quantile(values, q, method=...) exactly.  sim.quantile("q", 0.9) is the threshold track_vortices wants, without the download."""
        if method not in _dist.METHODS:
            raise ValueError(f"method must be one of {_dist.METHODS}, got {method!r}")
        qs = [float(x) for x in np.atleast_1d(np.asarray(q, np.float64))]
        n = self.order_statistics(quantity, (), box)["n"]
        if n == 0:
            raise ValueError(f"no selected cell holds a value of {quantity!r}: there is no quantile")
        pairs = [_dist.rank_pair(n, x) for x in qs]
        ranks = sorted({k for a, b, _ in pairs for k in (a, b)})
        found = {}
        for c in range(0, len(ranks), self._dev.DIST_MAX_RANKS):
            chunk = ranks[c:c + self._dev.DIST_MAX_RANKS]
            found.update(zip(chunk, self.order_statistics(quantity, chunk, box)["values"].tolist()))
        out = np.array([_dist.interpolate(found[a], found[b], g, method) for a, b, g in pairs], np.float64)
        return float(out[0]) if np.ndim(q) == 0 else out

    # -- energy spectra (new): the windowed FFT of the velocity over a box on the device, the power of every bin accumulated ------------------
    def start_spectra(self, box, every=1, start_step=0, window="hann", detrend=True):
        """From the next step on, accumulate the energy spectrum of the velocity over `box` on the device (csrc/fs_spec.h): after every step
        k (counted from here) with k > start_step and (k - start_step) % every == 0 the box's (u + i w), windowed, goes through a 2-D FFT
        in double and the power of every bin is added to a plane.  box = (x0, y0, x1, y1) in global cells, half-open, inside the grid, both
        sides powers of two in 8 .. 4096 (ValueError otherwise, before any device call); wall cells count as zeros.  window: "hann"
        (periodic) or "boxcar"; detrend: remove the window-weighted mean of u and w in spectral space (the DC bin and, under the Hann
        window, its eight neighbours).  The launches are part of the step: they are captured into the replayed graphs, decide on the device
        whether they sample, and run() is not cut into chunks by them.  A plane is a pure function of the fields: identical between eager
        steps, replayed graphs and resumed runs.  40 bytes per cell of the box of device memory.  Changes no field and no trajectory.
        spectra() returns the result.  Raises while a spectrum is attached already and during a graph capture; single-GPU contexts only
        (FsError on slabs)."""
        dev = self._dev
        self._not_capturing("start_spectra")
        self._make_way("_spectrar", "a spectrum is attached already: stop_spectra() first (or reset_spectra())")
        every, start_step = self._cadence(every, start_step)
        self._spectrar = _spectra.Spectra(dev, _spectra.create(dev, box, window, detrend, every, start_step), window, self._solver.dx)

    def _spectra(self):
        return self._attached("_spectrar", "spectrum", "start_spectra")

    def spectra(self):
        """The spectrum so far: {"power": float64 (Nx, Ny), the mean over the samples of (P[k] + P[-k]) / 2, indexed like np.fft.fft2;
        "energy": power / 2 / (Nx Ny sum(wx^2) sum(wy^2)) - its sum over all bins is the window-weighted mean of (u'^2 + w'^2) / 2;
        "kx", "ky": rad per length; "k", "E": the shell spectrum (fs.spectra.shell_spectrum); "samples", "sample_steps", "box", "window",
        "detrend"; "sums": the device's plane as accumulated}.  fs.spectra.slope / line_spectrum work on it.  A download of the power
        plane; not allowed during a graph capture."""
        self._not_capturing("spectra")
        return self._spectra().data()

    def reset_spectra(self):
        """Power plane and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._not_capturing("reset_spectra")
        self._spectra().reset()

    def stop_spectra(self):
        """Detach the spectrum and free its device memory; the cached graphs that hold its launches are freed first.  Nothing is kept on
        the host: call spectra() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_spectrar", "stop_spectra")

    def _spectrum_once(self, name, box, window, detrend, read):
        dev = self._dev
        return self._once(name, lambda: _spectra.create(dev, box, window, detrend, 1, 0), lambda sp: dev.spec_launch(sp, self._solver.get_fields()[0]),
                          read, dev.spec_free)[0]

    def spectrum(self, box, window="hann", detrend=True):
        """The spectrum of the fields as they are now: the dict spectra() returns, with "samples" 1 and "sample_steps" [0] (the call counts
        no steps).  One temporary object, one eager launch, a read and a free: changes no field, no graph and no attached rider, and
        leaves a deferred limit_field deferred.  Not allowed during a graph capture."""
        sums, _, samples = self._spectrum_once("spectrum", box, window, detrend, self._dev.spec_read)
        return _spectra.result(sums, samples, np.zeros(samples, np.int64), self._dev.spec_box(box), window, detrend, self._solver.dx)

    def box_fft(self, box, window="hann", detrend=False):
        """The transform itself: complex128 (Nx, Ny), Z' = FFT2((u + i w) wx wy) over the box as the device computes it (wall cells as
        zeros; detrend as in start_spectra), indexed like np.fft.fft2.  fs.spectra.split gives the two components.  As spectrum():
        temporary, eager, changes nothing."""
        return self._spectrum_once("box_fft", box, window, detrend, self._dev.spec_plane)

    # -- cross-spectra (new): the packed FFT of two flow quantities over a box, split on the device into both transforms -------------------
    def start_cross_spectra(self, box, pair=("u", "w"), every=1, start_step=0, window="hann", detrend=True):
        """From the next step on, accumulate the spectra and the cross-spectrum of two quantities over `box` on the device
        (csrc/fs_xspec.h).  pair = (qa, qb) or (qa, None), names out of "u", "w", "p", "speed", "vorticity", "q", "swirl" (the quantities of
        start_distributions, same definitions): the windowed plane a + i b goes through the transform of start_spectra, the device splits
        it into the transforms A and B of the two real fields and adds |A|^2, |B|^2 and A conj(B) of every bin to four planes.  u, w, p and
        speed count where the cell is no wall, vorticity, q and swirl on fluid cells; every other cell counts as zero.  box, every,
        start_step, window and detrend as in start_spectra (ValueError before any device call); 64 bytes per cell of the box of device
        memory, 40 for one scalar.  The launches are part of the step and of the replayed graphs; the planes are a pure function of the
        fields.  Changes no field and no trajectory, and may be attached beside start_spectra.  cross_spectra() returns the result.
        Raises while a cross-spectrum is attached already and during a graph capture; single-GPU contexts only (FsError on slabs)."""
        dev = self._dev
        self._not_capturing("start_cross_spectra")
        self._make_way("_xspectrar", "a cross-spectrum is attached already: stop_cross_spectra() first (or reset_cross_spectra())")
        every, start_step = self._cadence(every, start_step)
        xs = _spectra.create_cross(dev, box, pair, self._solver.dx, window, detrend, every, start_step)
        self._xspectrar = _spectra.CrossSpectra(dev, xs, window)

    def _cross_spectra(self):
        return self._attached("_xspectrar", "cross-spectrum", "start_cross_spectra")

    def cross_spectra(self):
        """The cross-spectrum so far: the dict of fs.spectra.cross_result - "spectrum_a", "spectrum_b", "co", "quad" per bin, the shell sums
        "k", "Sa", "Sb", "Co", "Quad", "coherence" and "phase" per shell, "quantities", "samples", "sample_steps", "box", "window",
        "detrend" and the device's planes "sums".  A download of the planes; not allowed during a graph capture."""
        self._not_capturing("cross_spectra")
        return self._cross_spectra().data()

    def reset_cross_spectra(self):
        """Planes and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._not_capturing("reset_cross_spectra")
        self._cross_spectra().reset()

    def stop_cross_spectra(self):
        """Detach the cross-spectrum and free its device memory; the cached graphs that hold its launches are freed first.  Nothing is
        kept on the host: call cross_spectra() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_xspectrar", "stop_cross_spectra")

    def _cross_once(self, name, box, pair, window, detrend, read):
        dev, s = self._dev, self._solver
        return self._once(name, lambda: _spectra.create_cross(dev, box, pair, s.dx, window, detrend, 1, 0),
                          lambda xs: dev.xspec_launch(xs, *s.get_fields()[:2]), read, dev.xspec_free)

    def cross_spectrum(self, box, pair=("u", "w"), window="hann", detrend=True):
        """The cross-spectrum of the fields as they are now: the dict cross_spectra() returns, with "samples" 1 and "sample_steps" [0].
        One temporary object, one eager launch, a read and a free: changes no field, no graph and no attached rider, and leaves a
        deferred limit_field deferred.  Not allowed during a graph capture."""
        (sums, _, samples), xs = self._cross_once("cross_spectrum", box, pair, window, detrend, self._dev.xspec_read)
        return _spectra.cross_result(sums, samples, np.zeros(samples, np.int64), xs.box, _spectra.pair_names(xs.qa, xs.qb), window, detrend,
                                     self._solver.dx)

    def pair_fft(self, box, pair=("u", "w"), window="hann", detrend=False):
        """The transform itself: complex128 (Nx, Ny), Z' = FFT2((a + i b) wx wy) over the box as the device computes it (detrend as in
        start_cross_spectra), indexed like np.fft.fft2; fs.spectra.split gives the transforms of a and b.  For ("u", "w") it is box_fft(),
        bit for bit.  As cross_spectrum(): temporary, eager, changes nothing."""
        return self._cross_once("pair_fft", box, pair, window, detrend, self._dev.xspec_plane)[0]

    # -- scale-to-scale fluxes (new): box filters of the velocity and the vorticity on the device, PI, ZF and K of every cell accumulated -----
    def _grid_shape(self):
        return (self._dev.nx, self._dev.ny)

    def start_scale_fluxes(self, box, half_widths, every=1, start_step=0):
        """From the next step on, accumulate the scale-to-scale fluxes over `box` on the device (csrc/fs_flux.h): after every step k
        (counted from here) with k > start_step and (k - start_step) % every == 0 the velocity and the vorticity are filtered with a box
        of (2 r + 1)^2 cells for every half-width r, and per cell of the box and half-width the energy flux PI = -tau_ij S_ij towards the
        scales below (2 r + 1) dx (tau the sub-filter stress, S the filtered rate of strain), the enstrophy flux ZF and the sub-filter
        energy K are added to three planes.  box = (x0, y0, x1, y1) in global cells, half-open, inside the grid, any sides; half_widths: 1
        to 8 integers in 1 .. 64, strictly increasing (ValueError otherwise, before any device call).  The filter reads outside the box,
        never outside the grid: a cell is valid for r when it keeps r + 1 cells from every edge of the grid, the others stay zero, and a
        half-width without a valid cell in the box is refused.  Solid cells count as fluid at rest.  The launches are part of the step:
        they are captured into the replayed graphs, decide on the device whether they sample, and run() is not cut into chunks by them.
        A plane is a pure function of the fields: identical between eager steps, replayed graphs and resumed runs.  Device memory: 192
        bytes per cell of the box dilated by r_max + 1 and 24 per cell of the box and half-width.  Changes no field and no trajectory.
        scale_fluxes() returns the result.  Raises while scale fluxes are attached already and during a graph capture; single-GPU
        contexts only (FsError on slabs)."""
        dev = self._dev
        self._not_capturing("start_scale_fluxes")
        self._make_way("_fluxr", "scale fluxes are attached already: stop_scale_fluxes() first (or reset_scale_fluxes())")
        every, start_step = self._cadence(every, start_step)
        self._fluxr = _fluxes.ScaleFluxes(dev, dev.flux_create(box, half_widths, self._solver.dx, every, start_step), self._grid_shape())

    def _scale_fluxes(self):
        return self._attached("_fluxr", "scale fluxes", "start_scale_fluxes")

    def scale_fluxes(self):
        """The fluxes so far: {"half_widths"; "widths": (2 r + 1) dx; "samples", "sample_steps", "box"; "valid": per half-width the
        rectangle (x0, y0, x1, y1) of valid cells inside the box; "pi", "zf", "k": float64 (n_r, Nx, Ny), the means over the samples
        (zero outside the valid rectangle); "sums": the device's planes (n_r, 3, Nx, Ny) as accumulated; "mean_pi", "mean_zf", "mean_k":
        per half-width the mean over the COMMON valid rectangle - that of the largest half-width -, so that the widths are compared over
        the same cells; "mean_own": {"pi", "zf", "k"}, the same means over each width's own rectangle}.  PI > 0: energy goes to the
        smaller scales.  A download of the planes; not allowed during a graph capture."""
        self._not_capturing("scale_fluxes")
        return self._scale_fluxes().data()

    def reset_scale_fluxes(self):
        """Planes and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._not_capturing("reset_scale_fluxes")
        self._scale_fluxes().reset()

    def stop_scale_fluxes(self):
        """Detach the scale fluxes and free their device memory; the cached graphs that hold their launches are freed first.  Nothing is
        kept on the host: call scale_fluxes() before.  Inside a graph capture the device memory is released when the capture ends."""
        self._detach(self, "_fluxr", "stop_scale_fluxes")

    def _flux_once(self, name, box, half_widths, read):
        dev, s = self._dev, self._solver
        return self._once(name, lambda: dev.flux_create(box, half_widths, s.dx, 1, 0), lambda fx: dev.flux_launch(fx, s.get_fields()[0]), read,
                          dev.flux_free)

    def scale_flux(self, box, half_widths):
        """The fluxes of the fields as they are now: the dict scale_fluxes() returns, with "samples" 1 and "sample_steps" [0] (the call
        counts no steps).  One temporary object, one eager launch, a read and a free: changes no field, no graph and no attached rider,
        and leaves a deferred limit_field deferred.  Not allowed during a graph capture."""
        (sums, _, samples), fx = self._flux_once("scale_flux", box, half_widths, self._dev.flux_read)
        return _fluxes.flux_result(sums, samples, np.zeros(samples, np.int64), fx.box, fx.half_widths, fx.dx, self._grid_shape())

    def filtered_fields(self, box, half_width):
        """The stage before the fluxes: {"u", "w", "om", "uu", "uw", "ww", "uom", "wom"}, float64 (Nx, Ny) each - the box filter of
        half-width `half_width` of u, w, the vorticity and their products over the box as the device computes it (zero where the window
        leaves the grid) - and "defined": the rectangle where it does not.  As scale_flux(): temporary, eager, changes nothing."""
        half_width = int(half_width) if isinstance(half_width, (int, np.integer)) and not isinstance(half_width, bool) else half_width
        planes, fx = self._flux_once("filtered_fields", box, (half_width,), lambda fx: self._dev.flux_filtered(fx, half_width))
        out = dict(zip(_fluxes.FILTERED, planes))
        X, Y = self._grid_shape()
        out["defined"] = (max(fx.box[0], half_width), max(fx.box[1], half_width), min(fx.box[2], X - half_width), min(fx.box[3], Y - half_width))
        return out

    # -- kinetic-energy budget (new): 21 raw moments per fluid cell of a box accumulated on the device; the terms are host algebra ------------
    def _budget_box(self, box):
        """The box (None: the whole grid) as a tuple of ints, and its fluid cells (mask == 0); a box without one is refused (ValueError)."""
        dev = self._dev
        box = (0, 0, dev.nx, dev.ny) if box is None else dev.flux_box(box)
        fluid = np.asarray(self._solver._bc.mask)[box[0]:box[2], box[1]:box[3]] == 0
        if not fluid.any():
            raise ValueError(f"the box {box} holds no fluid cell")
        return box, fluid

    def start_budget(self, box=None, every=1, start_step=0):
        """From the next step on, accumulate the budget of the fluctuation kinetic energy k = (<u'u'> + <w'w'>) / 2 over `box` on the device
        (csrc/fs_budget.h): after every step k (counted from here) with k > start_step and (k - start_step) % every == 0, every fluid cell
        of the box adds u, w, p, their second and third moments, the pressure correlations, the velocity gradient (central differences) and
        its squares to 21 planes of double.  box = (x0, y0, x1, y1) in global cells, half-open, anything inside the grid with at least one
        fluid cell (ValueError otherwise, before any device call); None: the whole grid.  The launch is part of the step: captured into
        the replayed graphs, it decides on the device whether it samples, and run() is not cut into chunks by it.  A plane is a pure
        function of the fields: identical between eager steps, replayed graphs and resumed runs.  Device memory: 168 bytes per cell of
        the box.  Changes no field and no trajectory.  budget() returns the result.  Raises while a budget is attached already and during
        a graph capture; single-GPU contexts only (FsError on slabs)."""
        dev = self._dev
        self._not_capturing("start_budget")
        self._make_way("_budgetr", "a budget is attached already: stop_budget() first (or reset_budget())")
        every, start_step = self._cadence(every, start_step)
        box, fluid = self._budget_box(box)
        self._budgetr = _budgets.Budget(dev, dev.budget_create(box, self._solver.dx, every, start_step), fluid, self._solver.re)

    def _budget(self):
        return self._attached("_budgetr", "budget", "start_budget")

    def budget(self):
        """The budget so far (fs.budgets.derive_budget): float64 (Nx, Ny) arrays over the box - the means "U", "W", "P", the central moments
        "uu", "ww", "uw", "k", "pu", "pw", "uuu", "uuw", "wwu", "www", the mean gradients "Ux", "Uy", "Wx", "Wy", and the terms "convection",
        "production", "dissipation" (positive), "turbulent_transport", "pressure_diffusion", "pressure_dilatation", "viscous_diffusion",
        "residual" -; "totals": each term summed over "valid" times dx^2; "fluid", "valid", "samples", "sample_steps", "box", "dx", "re"
        and the raw "sums" (21, Nx, Ny).  In a statistically steady flow -residual is the rate at which the advection scheme, the
        confinement, the velocity limit and the splitting change k.  Every array is there, all zeros, while no sample has been taken.
        fs.budgets.momentum_balance gives the mean momentum equation from the same dict.  A download of the planes; not allowed during a
        graph capture."""
        self._not_capturing("budget")
        return self._budget().data()

    def reset_budget(self):
        """Planes and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        self._not_capturing("reset_budget")
        self._budget().reset()

    def stop_budget(self):
        """Detach the budget and free its device memory (168 bytes per cell of the box); the cached graphs that hold its launches are freed
        first.  Nothing is kept on the host: call budget() before.  Inside a graph capture the device memory is released when the capture
        ends."""
        self._detach(self, "_budgetr", "stop_budget")

    def budget_sample(self, box=None):
        """The budget's planes of the fields as they are now: the dict budget() returns, with "samples" 1 and "sample_steps" [0] (the call
        counts no steps; with one sample every fluctuation is zero - the use is the raw "sums" and the means).  One temporary object of
        168 bytes per cell of the box, one eager launch, a read and a free: changes no field, no graph and no attached rider, and leaves a
        deferred limit_field deferred.  Not allowed during a graph capture."""
        dev, s = self._dev, self._solver
        self._not_capturing("budget_sample")      # (before the box is looked at)
        box, fluid = self._budget_box(box)
        (sums, _, samples), _ = self._once("budget_sample", lambda: dev.budget_create(box, s.dx, 1, 0), lambda bg: dev.budget_launch(bg, *s.get_fields()[:2]),
                                           dev.budget_read, dev.budget_free)
        return _budgets.budget_result(sums, samples, np.zeros(samples, np.int64), box, fluid, self._solver.dx, self._solver.re)

    # -- flow maps and FTLE fields (new): a lattice of particles carried through the POD's resident snapshots on the device --------------
    def flow_map(self, direction="backward", refine=1, box=None, substeps=1, first=None, last=None):
        """The flow map over the resident snapshots of the attached POD (start_pod), integrated on the device (csrc/fs_lcs.h): refine x
        refine particles per cell of the cell box (x0, y0, x1, y1) (None: the whole domain; refine in 1, 2, 4, 8) are carried from resident
        sample `first` to `last` ("forward") or from `last` back to `first` ("backward") - indices into the resident samples, 0 the oldest,
        negative from the newest, None the oldest / newest - with `substeps` (1 .. 16) midpoint steps per interval in the velocity
        interpolated bilinearly in space and linearly in time between consecutive snapshots.  One launch per interval, one pass for the
        Cauchy-Green tensor, one download of the lattice; no field is downloaded.  -> {"x", "y": float64 (nx, ny), the final positions in
        cell units; "x0", "y0": the start positions; "status": int32, 0 arrived, 1 left the domain (forward: through an outflow cell too;
        backward: into an inflow cell too), 2 ran into a wall cell, 4 started in one (never moved) - a node with status 1 or 2 kept its
        last valid position; "lam": the largest eigenvalue of the Cauchy-Green tensor (NaN on status-4 nodes); "ftle": log(lam) / (2 span)
        (fs.lcs.ftle); "span": (window samples - 1) * every * dt; "sample_steps": the steps of the window's samples; "direction", "refine",
        "box"}.  Backward-time FTLE ridges are the attracting structures (where dye collects), forward-time ridges the repelling ones.
        The ring holds 0 in wall cells, so the no-slip point is the wall cell's centre; the time resolution is the snapshot cadence.
        Raises RuntimeError without a POD or with fewer than 2 resident samples; not allowed during a graph capture; single-GPU contexts."""
        from . import lcs
        from ._lib import FsError
        from .pod import sample_steps
        po = self._pod()
        dev = self._dev
        if self._capturing():
            raise FsError("flow_map / ftle / ftle_fields during a graph capture: they allocate and download")
        box, refine, substeps = lcs.check_lattice(box, refine, substeps, (dev.nx, dev.ny))
        _, samples = dev.pod_read(po.pod)
        pairs = lcs.intervals(samples, po.pod.slots, first, last, direction)
        i0, i1 = lcs.window(samples, po.pod.slots, first, last)
        h = lcs.step_size(po.every, self._solver.dt, self._solver.dx, substeps, direction)
        fm = dev.flowmap_create(box, refine)
        try:
            for a, b in pairs:
                dev.flowmap_advance(fm, po.pod, a, b, h, substeps)
            dev.flowmap_cauchy_green(fm)
            x, y, status, lam = dev.flowmap_get(fm)
        finally:
            dev.flowmap_free(fm)
        span = (i1 - i0) * po.every * float(self._solver.dt)
        x0, y0 = lcs.start_positions(box, refine)
        return {"x": x, "y": y, "x0": x0, "y0": y0, "status": status, "lam": lam, "ftle": lcs.ftle(lam, span), "span": span,
                "sample_steps": sample_steps(samples, po.pod.slots, po.every, po.start_step, po.base)[i0:i1 + 1],
                "direction": direction, "refine": refine, "box": box}

    def ftle(self, direction="backward", refine=1, box=None, substeps=1, first=None, last=None):
        """The finite-time Lyapunov exponent field of flow_map() alone: float64 (nx, ny)."""
        return self.flow_map(direction, refine, box, substeps, first, last)["ftle"]

    def ftle_fields(self, direction="backward", substeps=1, first=None, last=None):
        """flow_map() over the whole domain at refine=1 as device fields (v, p), as pod_fields() returns them - for fields_frame and the
        pressure renderer: p holds the FTLE in the fields' precision (non-finite values as 0), v the displacement (x - x0, y - y0).  New
        fields on every call; the caller owns them.  Not a hot path: the lattice is downloaded and the two fields are uploaded."""
        from .runtime import Field
        m = self.flow_map(direction, 1, None, substeps, first, last)
        dev = self._dev
        v, p = Field(dev, 2), Field(dev, 1)      # (not dev.alloc: scratch fields stay out of the ghost-row bookkeeping state of the tapes)
        v.from_numpy(np.stack([m["x"] - m["x0"], m["y"] - m["y0"]], axis=-1).astype(dev.dtype))
        p.from_numpy(np.where(np.isfinite(m["ftle"]), m["ftle"], 0.0).astype(dev.dtype))
        return v, p

    # -- tracer particles (new): pathlines and streaklines advanced on the device ------------------------------------------------------
    def seed_tracers(self, seeds, respawn=True, max_age=0, sort_every=0, tau=None, gravity=(0.0, 0.0), deposits=False):
        """From the next step on, N passive particles ride the step: seeds float64 (N, 2) in CELL units (cell (i, j) covers [i, i + 1) x
        [j, j + 1); fs.tracers.seed_line / seed_grid / seed_random build them), each inside the domain in a fluid or inflow cell
        (ValueError naming the first offender otherwise).  After every step each alive particle takes one midpoint step in the velocity
        the step left (include/fs_hip.h fs_tracer_advance).  A particle that leaves the domain or enters an outflow cell (LEFT), enters a
        wall cell (WALL) or reaches max_age > 0 steps (EXPIRED) starts again at its seed with respawn=True - a steady release: streaklines -
        and keeps its fate as status with respawn=False - pathlines.  The launch is part of the step: it is captured into the replayed
        graphs, and run() is not cut into chunks by it.  52 bytes per particle; changes no field and no trajectory.  tracers() returns the
        state.  Raises while a set is attached already and during a graph capture; single-GPU contexts only (FsError on slabs).

        sort_every = K > 0: after every K-th step counted from here the particle slots are sorted by cell on the device (sort_tracers), so
        that the advance keeps gathering from neighbouring cache lines while the flow mixes the particles - measured worth it from 2^20
        particles on, not below.  The sort runs between launch sequences, never inside a graph: step() sorts after its
        step, run() cuts its chunks at the multiples of K; capture_period() and captured steps never sort.  A run() chunk shorter than 16
        steps does not capture a graph, so an interval below 16 keeps a fresh simulator eager, step by step.  Recommended: K = 32, which
        measured best at 2^20 and 2^24 particles (bc5 res 4096: 2.74 -> 0.30 ms and 165 -> 75 us per step; DESIGN.md 4ab has all the
        measured intervals).  Costs 36 more bytes per particle and 4 per sort bin from the first sort on.  0 (default): never - exactly
        the behaviour without this argument.  Sorting changes nothing tracers(), draw_tracers(), tracer_fields() or a checkpoint shows.

        tau (None: the passive set above, through the same code as ever): a scalar or an (N,) array of response times >= 0 in the solver's
        time units makes the particles INERTIAL - dust, droplets, sediment.  Each carries a velocity v_p that relaxes to the fluid's:
        dv_p/dt = (V - v_p) / tau + gravity, integrated exactly over a step with V frozen at the particle's position (v_p += alpha (V +
        tau gravity - v_p), alpha = fs.tracers.response(tau, dt)), then x += dt / dx * v_p.  A particle is released with the fluid's
        velocity.  One gather per step: as tau -> 0 this is the forward-Euler tracer, not the midpoint rule of the passive set, and a
        particle may cross more than one cell per step, as a passive one may.  gravity = (gx, gy) in velocity per time; fs.tracers.
        stokes_number(tau, speed, length) tells how inertial a tau is.  deposits=True: every wall hit is counted in the wall cell the
        particle would have entered, respawn or not (tracer_deposits()).  84 bytes per particle (68 more from the first sort on), 4 per
        cell with deposits.  gravity or deposits without tau raise ValueError.  tracers() gains "u", "w" and "tau"."""
        from ._lib import FsError
        dev, s = self._dev, self._solver
        # (through the class: the tests check the refusal on slabs with an object that is no FluidSimulator)
        FluidSimulator._not_capturing(self, "seed_tracers")
        FluidSimulator._make_way(self, "_tracers", "a tracer set is attached already: stop_tracers() first")
        if dev.nranks > 1:
            raise FsError("tracer particles need a single-GPU context: on slabs they would have to migrate between ranks (not implemented)")
        max_age, sort_every = int(max_age), int(sort_every)
        if max_age < 0:
            raise ValueError("max_age must be >= 0")
        if sort_every < 0:
            raise ValueError("sort_every must be >= 0")
        gravity = tuple(float(g) for g in np.asarray(gravity, np.float64).ravel())
        if len(gravity) != 2 or not all(np.isfinite(g) for g in gravity):
            raise ValueError("gravity must be two finite numbers (gx, gy)")
        if tau is None and (gravity != (0.0, 0.0) or deposits):
            raise ValueError("gravity and deposits belong to inertial particles: pass tau (0 for particles without inertia)")
        seeds = check_seeds(np.asarray(s._bc.mask), seeds)
        if tau is None:
            self._tracers = Tracers(dev, dev.tracer_create(seeds, respawn, max_age), seeds, respawn, max_age, sort_every)
            return
        tau = np.asarray(tau, np.float64)
        if tau.ndim == 0:
            tau = np.full(len(seeds), tau, np.float64)
        if tau.shape != (len(seeds),):
            raise ValueError(f"tau must be a scalar or have shape {(len(seeds),)}, got {tau.shape}")
        alpha = response(tau, s.dt)          # (ValueError for a tau that is negative or not finite)
        tset = dev.tracer_create_inertial(seeds, alpha, tau, gravity, respawn, max_age, deposits)
        self._tracers = Tracers(dev, tset, seeds, respawn, max_age, sort_every, tau=tau.copy(), gravity=gravity, deposits=deposits)

    def _trc(self):
        return self._attached("_tracers", "tracers", "seed_tracers")

    def tracers(self):
        """The particles now (one download): {"x", "y": float64 (N,) in cell units, "age": int32 steps since the seed or the last respawn
        (fs.tracers.residence_time), "status": int32 fs.tracers.FATE_*, "respawns": int32, "seeds": float64 (N, 2), "steps": steps since
        seed_tracers()}; an inertial set (seed_tracers(tau=...)) adds "u", "w": float64 (N,), the particle velocity in the field's units
        (what the last step left; a particle at age 0 takes the fluid's on its next step), and "tau": float64 (N,).  Not allowed during a
        graph capture."""
        tr = self._trc()
        out = tr.dev.tracer_read(tr.set)
        if tr.tau is not None:
            out["u"], out["w"] = tr.dev.tracer_read_vel(tr.set)
            out["tau"] = tr.tau.copy()
        return out

    def sort_tracers(self):
        """Sort the particle slots by cell on the device now (DeviceBase.tracer_sort): what seed_tracers(sort_every=K) does every K steps.
        Nothing observable changes, and the cached graphs stay valid.  Not allowed during a graph capture."""
        self._not_capturing("sort_tracers")
        self._trc().sort()

    def tracer_fields(self):
        """Where the particles are now, per cell, binned on the device: {"count": int32 (X, Y), alive particles in the cell; "age_sum":
        int64 (X, Y), the sum of their ages in steps (fs.tracers.residence_map(count, age_sum, dt) is the residence-time map); "steps":
        steps since seed_tracers()}.  Exact and repeatable (integer atomics); 12 bytes per cell on the device for the call and in the
        download.  Not allowed during a graph capture."""
        self._not_capturing("tracer_fields")
        tr = self._trc()
        count, age_sum = tr.dev.tracer_fields(tr.set)
        return {"count": count, "age_sum": age_sum, "steps": tr.dev.tracer_read_steps(tr.set)}

    def draw_tracers(self, rgb_field=None, color=(1, 1, 1)):
        """Overlay the alive particles on an image field (default: self.rgb_buf, i.e. after any get_*_field()): pixel (floor x, floor y)
        takes `color`.  Returns the field."""
        tr = self._trc()
        rgb = self.rgb_buf if rgb_field is None else rgb_field
        tr.dev.tracer_draw(tr.set, rgb, color)
        return rgb

    def tracer_deposits(self):
        """Wall hits per wall cell since seed_tracers(tau=..., deposits=True): int32 (X, Y), exact and repeatable (integer atomics).  A
        particle that hits a wall is counted in the wall cell it would have entered, whether it respawns or not."""
        self._not_capturing("tracer_deposits")
        tr = self._trc()
        if not tr.deposits:
            raise RuntimeError("the tracer set records no deposits: seed_tracers(tau=..., deposits=True)")
        return tr.dev.tracer_deposits(tr.set)

    def accumulate_tracers(self, every=1, start_step=0):
        """From the next step on, add the per-cell particle count and age sum (what tracer_fields() snapshots) to 64-bit sums on the device
        after every step k (counted from here, k = 1, 2, ...) with k > start_step and (k - start_step) % every == 0.  The launch goes
        behind the advance and is part of the step: it is captured into the replayed graphs, decides on the device whether it samples, and
        run() is not cut into chunks by it.  16 bytes per cell; exact: the sum of the tracer_fields() snapshots at the sampled steps.
        Passive and inertial sets alike.  tracer_accumulation() returns the result.  Raises without a tracer set, while an accumulation is
        attached already and during a graph capture."""
        dev = self._dev
        self._not_capturing("accumulate_tracers")
        tr = self._trc()
        if tr.accumulation is not None:
            raise RuntimeError("an accumulation is attached already: stop_tracer_accumulation() first (or reset_tracer_accumulation())")
        every, start_step = self._cadence(every, start_step)
        tr.accumulation = TracerAccumulation(dev.tracer_accum_create(tr.set, every, start_step), every, start_step, dev=dev)

    def _tacc(self):
        tr = self._trc()
        if tr.accumulation is None:
            raise RuntimeError("no accumulation: call accumulate_tracers() first")
        return tr

    def tracer_accumulation(self):
        """The accumulated occupancy so far (a download of 16 bytes per cell): {"occupancy": int64 (X, Y), alive particles seen in the cell
        summed over the sampled steps; "age_sum": int64 (X, Y), the sum of their ages (fs.tracers.residence_map(occupancy, age_sum, dt):
        the mean residence time, fs.tracers.concentration(occupancy, samples): the mean particles per cell); "samples": sampled steps;
        "steps": steps since accumulate_tracers()}.  Not allowed during a graph capture."""
        self._not_capturing("tracer_accumulation")
        tr = self._tacc()
        occ, age, launches, samples = tr.dev.tracer_accum_read(tr.set)
        return {"occupancy": occ, "age_sum": age, "samples": samples, "steps": launches}

    def reset_tracer_accumulation(self):
        """Sums and sample count back to zero; the step count and the phase of `every` / `start_step` run on."""
        tr = self._tacc()
        tr.dev.tracer_accum_reset(tr.set)

    def stop_tracer_accumulation(self):
        """Detach the accumulation and free its device memory; the cached graphs that hold its launch are freed first.  Nothing is kept
        on the host: call tracer_accumulation() before.  Inside a graph capture the device memory is released when the capture ends."""
        if self._tracers is not None:
            self._detach(self._tracers, "accumulation", "stop_tracer_accumulation")

    def stop_tracers(self):
        """Detach the tracer set (and its accumulation) and free its device memory; the cached graphs that hold its launch are freed
        first.  Nothing is kept on the host: call tracers() before.  Inside a graph capture the device memory is released when the capture
        ends."""
        self._detach(self, "_tracers", "stop_tracers")

    # -- visualisation (fs/fluid_simulator.py:22-58): device kernels; like the reference these return the image FIELD ----
    def get_norm_field(self):
        v, p = self._solver.get_fields()[:2]
        self._dev.vis_norm(self.rgb_buf, v, p)
        return self.rgb_buf

    def get_pressure_field(self):
        self._dev.vis_pressure(self.rgb_buf, self._solver.get_fields()[1])
        return self.rgb_buf

    def get_vorticity_field(self):
        self._dev.vis_vorticity(self._solver.dx, self.rgb_buf, self._solver.get_fields()[0])
        return self.rgb_buf

    @staticmethod
    def create(num, resolution, dt, dx, re, vor_eps, scheme, pressure_updater=None):
        return FluidSimulator(_compose(num, resolution, dt, dx, re, vor_eps, scheme, False, pressure_updater))


class DyeFluidSimulator(FluidSimulator):
    def field_to_numpy(self):
        fields = self._solver.get_fields()
        return {"v": fields[0].to_numpy(), "p": fields[1].to_numpy(), "dye": fields[2].to_numpy()}

    def get_dye_field(self):
        self._dev.vis_dye(self.rgb_buf, self._solver.get_fields()[2])
        return self.rgb_buf

    @staticmethod
    def create(num, resolution, dt, dx, re, vor_eps, scheme, pressure_updater=None):
        return DyeFluidSimulator(_compose(num, resolution, dt, dx, re, vor_eps, scheme, True, pressure_updater))
