"""Device side of what rides the step and of the diagnostics (new; the reference has none): flow statistics, the per-step history, the
body surface loads, the time averages, the harmonic modes, the snapshot POD, the flow maps through its snapshots, the field distributions, the energy spectra, the cross-spectra, the scale-to-scale fluxes, the kinetic-energy budget and the tracer particles.  Two mixins: RideOps is the
backend-agnostic host logic fs.runtime.DeviceBase inherits (slab partition, combination over ranks, argument checks, the op log of a logged period), NativeRideOps the `_p_*` primitives
fs.runtime.Device binds to libfs_hip.so; the stand-in devices of the CPU tests override those.  fs.runtime re-exports every name here."""
import collections
import ctypes
import itertools
import math

import numpy as np

from . import _lib

_serials = itertools.count(1)      # identities for life of fields and device objects (id() is recycled)


class _Handle:
    """A device object of a rider: `_h`, the library's handle (None once freed), and `serial`, its name in signatures and op keys."""

    def __init__(self, h):
        self._h, self.serial = h, next(_serials)


class TracerSet(_Handle):
    """A device tracer set (DeviceBase.tracer_create): handle, particle count, respawn, max_age."""

    def __init__(self, h, n, respawn, max_age):
        super().__init__(h)
        self.n, self.respawn, self.max_age = n, respawn, max_age
        self.inertial, self.deposits, self.gravity, self.tau, self.alpha = False, False, (0.0, 0.0), None, None      # (tracer_create_inertial)
        self.accum = None          # TracerAccum while tracer_accum_create's planes are attached


class TracerAccum(_Handle):
    """The accumulated-occupancy planes of a tracer set (DeviceBase.tracer_accum_create): every, start and an identity of its own."""

    def __init__(self, tr, every, start):
        super().__init__(None)      # (no handle of its own: the planes hang on the set's)
        self.set, self.every, self.start = tr, every, start


class Mean(_Handle):
    """Device accumulators of a time average (DeviceBase.mean_create): handle, every, start."""

    def __init__(self, h, every, start):
        super().__init__(h)
        self.every, self.start = every, start


class Modes(_Handle):
    """Device accumulators of the harmonic modes (DeviceBase.modes_create): handle, number of frequencies, every, start."""

    def __init__(self, h, nfreq, every, start):
        super().__init__(h)
        self.nfreq, self.every, self.start = nfreq, every, start


class Pod(_Handle):
    """Device snapshots of the POD (DeviceBase.pod_create): handle, number of slots, every, start."""

    def __init__(self, h, slots, every, start):
        super().__init__(h)
        self.slots, self.every, self.start = slots, every, start


class Vortex(_Handle):
    """A device vortex tracker (DeviceBase.vortex_create): handle and the parameters of its samples."""

    def __init__(self, h, criterion, threshold, exponent, every, start, min_area, max_vortices, max_components, capacity):
        super().__init__(h)
        self.criterion, self.threshold, self.exponent, self.every, self.start = criterion, threshold, exponent, every, start
        self.min_area, self.max_vortices, self.max_components, self.capacity = min_area, max_vortices, max_components, capacity


class Dist(_Handle):
    """Device tables of the field distributions (DeviceBase.dist_create): handle, the channels as dist_channel() returns them, every, start."""

    def __init__(self, h, channels, every, start):
        super().__init__(h)
        self.channels, self.every, self.start = tuple(channels), every, start
        self.words = sum(c.bins * max(1, c.bins_b) + RideOps.DIST_NTAIL for c in channels)      # (fs_dist_get / fs_dist_set)


class DistChannel(collections.namedtuple("DistChannel", "quantity bins lo hi quantity_b bins_b lo_b hi_b box")):
    """One table: quantity / quantity_b are indices into RideOps.DIST_QUANTITIES (quantity_b -1 and bins_b 0: a 1-D table), box x0, y0, x1, y1."""
    __slots__ = ()

    @property
    def joint(self):
        return self.quantity_b >= 0

    @property
    def shape(self):
        return (self.bins, self.bins_b) if self.joint else (self.bins,)


class _Planes(_Handle):
    """A device object that accumulates float64 planes over a cell box (RideOps._planes_*): `kind`, the stem of its calls and `_p_*`
    primitives; the box and its sides (nx, ny); `shape`, that of the planes on the host, (..., nx, ny); `y_major`: the device keeps every
    plane (ny, nx) and hands them over flat."""
    kind, y_major = None, False

    def __init__(self, h, box, lead=()):
        super().__init__(h)
        self.box = tuple(box)
        self.nx, self.ny = box[2] - box[0], box[3] - box[1]
        self.shape = tuple(lead) + (self.nx, self.ny)
        self.words = math.prod(self.shape)

    def to_host(self, flat):
        if self.y_major:
            return np.ascontiguousarray(flat.reshape(self.shape[:-2] + (self.ny, self.nx)).swapaxes(-1, -2))
        return flat.reshape(self.shape)

    def to_device(self, planes):
        return np.ascontiguousarray(planes.swapaxes(-1, -2)).ravel() if self.y_major else np.ascontiguousarray(planes)


class Spec(_Planes):
    """Device planes of an energy spectrum (DeviceBase.spec_create): handle, the cell box, its sides (nx, ny), detrend, every, start."""
    kind = "spec"

    def __init__(self, h, box, detrend, every, start):
        super().__init__(h, box)
        self.detrend, self.every, self.start = bool(detrend), every, start


class XSpec(_Planes):
    """Device planes of a cross-spectrum (DeviceBase.xspec_create): handle, the cell box, its sides (nx, ny), the quantity indices (qa, qb; qb -1:
    one scalar), the number of accumulator planes, dx, detrend, every, start."""
    kind = "xspec"

    def __init__(self, h, box, qa, qb, dx, detrend, every, start):
        self.planes = RideOps.XSPEC_NPLANE if qb >= 0 else 1
        super().__init__(h, box, (self.planes,))
        self.qa, self.qb, self.dx, self.detrend, self.every, self.start = qa, qb, dx, bool(detrend), every, start


class Flux(_Planes):
    """Device planes of the scale-to-scale fluxes (DeviceBase.flux_create): handle, the cell box, its sides (nx, ny), the half-widths, dx,
    every, start."""
    kind, y_major = "flux", True

    def __init__(self, h, box, half_widths, dx, every, start):
        super().__init__(h, box, (len(half_widths), RideOps.FLUX_NSUM))
        self.half_widths, self.dx, self.every, self.start = tuple(half_widths), dx, every, start


class Budget(_Planes):
    """Device planes of the kinetic-energy budget (DeviceBase.budget_create): handle, the cell box, its sides (nx, ny), dx, every, start."""
    kind, y_major = "budget", True

    def __init__(self, h, box, dx, every, start):
        super().__init__(h, box, (RideOps.BUDGET_NPLANE,))
        self.dx, self.every, self.start = dx, every, start


class FlowMap(_Handle):
    """A device lattice of flow-map nodes (DeviceBase.flowmap_create): handle, cell box, refine, and the lattice (nx, ny)."""

    def __init__(self, h, box, refine):
        super().__init__(h)
        self.box, self.refine = tuple(box), refine
        self.shape = (refine * (box[2] - box[0]), refine * (box[3] - box[1]))


class Loads(_Handle):
    """A device body tracker (DeviceBase.loads_create): handle (None on a slab that owns no face), the global face count, which faces
    this rank owns, capacity, every, start."""

    def __init__(self, h, nfaces, mine, capacity, every, start):
        super().__init__(h)
        self.nfaces, self.mine, self.capacity, self.every, self.start = nfaces, np.asarray(mine, np.int64), capacity, every, start


class History(_Handle):
    """A device history ring (DeviceBase.history_create): handle, the global probe count, which of them this rank owns, capacity, every."""

    def __init__(self, h, nprobes, mine, capacity, every):
        super().__init__(h)
        self.nprobes, self.mine, self.capacity, self.every = nprobes, np.asarray(mine, np.int64), capacity, every


class RideOps:
    """flow_stats and the history_* / loads_* / mean_* / modes_* / pod_* / flowmap_* / dist_* / spec_* / xspec_* / flux_* / budget_* / tracer_* calls of DeviceBase."""

    # (The tracer calls reach these through the class - RideOps._host_only(self, ...) - as they always reached _tracer_host_call: the CPU
    #  tests check their refusals on objects that are no devices.)
    def _host_only(self, message):
        """Refuse during a graph capture what allocates, downloads or synchronises: FsError(message)."""
        if getattr(self, "capturing", False):
            raise _lib.FsError(message)

    def _single_context(self, what, why):
        """Refuse on slabs what only a single context does: FsError "`what` a single-GPU context: on slabs `why` (not implemented)"."""
        if self.nranks > 1:
            raise _lib.FsError(f"{what} a single-GPU context: on slabs {why} (not implemented)")

    def _tracer_host_call(self, what):
        RideOps._host_only(self, f"{what} during a graph capture")
        RideOps._single_context(self, "tracer particles need", "they would have to migrate between ranks")

    def _cell_box(self, box):
        """(x0, y0, x1, y1) in global cells, half-open, inside the grid -> the tuple of ints (ValueError)."""
        box = tuple(int(b) for b in box)
        if len(box) != 4 or not (0 <= box[0] < box[2] <= self.nx and 0 <= box[1] < box[3] <= self.ny):
            raise ValueError(f"box must be (x0, y0, x1, y1) with 0 <= x0 < x1 <= {self.nx} and 0 <= y0 < y1 <= {self.ny}, got {box}")
        return box

    def _overwritten(self, *fields):
        """What a launch that stored every owned cell of `fields` leaves: nothing owed, on slabs stale ghost rows, a new identity."""
        for f in fields:
            f.pending_limit = f.pending_clamp = None
            f.valid = 0 if self.nranks > 1 else self.halo
            f.user_data = True
            f.static_id = next(_serials)

    def _ride(self, name, args=None):
        """A rider's launch behind the step.  Not a _run: no flush, no exchange, no ghost row, writes no field - in a logged period a kernel
        op of its own.  args=None: a placeholder that launches nothing and keeps the period's shape."""
        if self._oplog is not None:
            self._oplog.append(("k", name, args or (), ()))
        if args is not None:
            self._p_kernel(name, *args)

    @staticmethod
    def _limit_of(v):
        """The limit a deferred limit_field of v still owes, for the kernels that apply it to the values they read; 0: none."""
        return float(v.pending_limit) if v.pending_limit is not None else 0.0

    @staticmethod
    def _check_counters(launches, samples):
        launches, samples = int(launches), int(samples)
        if not 0 <= samples <= launches:
            raise ValueError("counters must satisfy 0 <= samples <= launches")
        return launches, samples

    @staticmethod
    def _check_cadence(every, start, capacity=None):
        every, start = int(every), int(start)
        if capacity is not None and (every < 1 or start < 0 or int(capacity) < 1):
            raise ValueError("every and capacity must be >= 1 and start >= 0")
        if every < 1 or start < 0:
            raise ValueError("every must be >= 1 and start >= 0")
        return every, start

    def _adopt(self, handle, obj):
        """Register a device object's handle under its serial (its name in the op keys of a logged period) -> obj."""
        if handle is not None:
            self._handle_serial[id(handle)] = obj.serial
        return obj

    def _release(self, obj, free):
        if obj._h is not None:
            self._handle_serial.pop(id(obj._h), None)
            free(obj._h)
            obj._h = None

    # slots of fs_flow_stats (include/fs_hip.h), in ABI order; those of _STAT_MAX combine by maximum, the others by sum
    STAT_SLOTS = ("fluid_cells", "sum_s2", "sum_om2", "sum_dv2", "max_s2", "max_a", "max_abs_dv", "nonfinite", "force_x", "force_y")
    _STAT_MAX = (4, 5, 6)

    def flow_stats(self, dx, v, p, box=None):
        """{slot: value} of fs_flow_stats over the GLOBAL grid (include/fs_hip.h): kinetic-energy, enstrophy and divergence sums, maxima,
        the non-finite count and the pressure force on the wall cells of `box` = (x0, y0, x1, y1) in global cells (half-open; None: no force).
        Across slabs the sums add and the maxima take the maximum; a NaN maximum on any rank makes the global one NaN.  Alters no field.
        A limit_field v still owes (limit_field) stays deferred while the buffer's flag is down - the pass would change no cell, and the
        solver's buffers keep the state their captured graphs expect; with the flag up it is launched first, as a download would.  Not
        allowed during a graph capture (FsError; the library refuses as well)."""
        self._host_only("flow_stats during a graph capture: the statistics are a download (sample between captures / replays)")
        # Skipping the owed pass relies on the flag being conservative - up whenever a stored cell may have x*x + y*y > 99 (csrc/fs_device.h,
        # "hot" flag: raised by every kernel that stores such a velocity, by uploads and unpacked ghost rows).  A deferred pass has
        # limit * limit > 99.01 (limit_field), and fs_limit_field exits on the same flag words fs_field_hot reads: with the flag down the
        # pass changes no cell.  Whoever changes the flag's rules must keep this true or flush unconditionally here.
        if v.pending_limit is not None and self.field_hot(v):
            self.flush_limit(v)
        if self.nranks > 1:
            stale = [f for f in (v, p) if f.valid < 1]
            if stale:
                self.exchange_many(stale)
        if box is not None:
            box = tuple(int(b) for b in box)
            if len(box) != 4:
                raise ValueError("box must be (x0, y0, x1, y1)")
        s = [float(x) for x in self._p_flow_stats(dx, v._h, p._h, box)]
        if self.nranks > 1:
            mx = [s[k] for k in self._STAT_MAX]
            sums = [k for k in range(len(s)) if k not in self._STAT_MAX]
            tot = self._p_allreduce([s[k] for k in sums] + [1.0 if m != m else 0.0 for m in mx])     # (+ per maximum: ranks that hold NaN)
            for k, x in zip(sums, tot):
                s[k] = x
            top = self._p_max_over_ranks([0.0 if m != m else m for m in mx])      # (a plain maximum would drop NaN: it is carried by the sum)
            for n, (k, x) in enumerate(zip(self._STAT_MAX, top)):
                s[k] = float("nan") if tot[len(sums) + n] > 0 else float(x)
        return dict(zip(self.STAT_SLOTS, s))

    # ---- per-step history (include/fs_hip.h fs_history_*): probe values and body faces gathered by one launch per step ------------------
    def history_create(self, points, faces, capacity, every):
        """A device ring of `capacity` records for FluidSimulator.record_history: points (P, 2) global probe cells, faces (n, 3) global
        (x, y, dir) of fs.history.body_faces.  A slab keeps the probes and faces whose cell lies in its owned rows: the record reads no ghost
        row, needs no exchange and sits in a tape as an ordinary kernel op.  Not allowed during a graph capture."""
        from .history import owned
        self._host_only("history_create during a graph capture")
        points = np.asarray(points, np.int32).reshape(-1, 2)
        faces = np.asarray(faces, np.int32).reshape(-1, 3)
        mine = owned(points, self.y0, self.nyl)
        h = self._p_history_create(np.ascontiguousarray(points[mine]), np.ascontiguousarray(faces[owned(faces, self.y0, self.nyl)]),
                                   int(capacity), int(every))
        return self._adopt(h, History(h, len(points), mine, int(capacity), int(every)))

    def history_record(self, hist, dx, v, p):
        """Append the record of the current v and p (every `every`-th call).  A limit_field v still owes stays deferred: the kernel limits
        the probe values as the pass would store them.  Not a _run: no flush, no exchange, no ghost row - on slabs a kernel op of its own
        in the logged period (writes no field)."""
        self._ride("history_record", (hist._h, float(dx), self._limit_of(v), v._h, p._h))

    def history_read(self, hist):
        """Empty the ring -> (forces (n, 2), probes (n, P, 3): u, w, p; launches so far, records dropped).  Across slabs the forces add
        and each probe comes from the rank that owns it (the others contribute -0.0, which leaves every value's bits alone).  Collective on
        slab runs; not allowed during a graph capture."""
        self._host_only("history_read during a graph capture: the ring is read between captures / replays")
        rec, launches, dropped = self._p_history_read(hist._h, len(hist.mine), hist.capacity)
        n = rec.shape[0]
        if self.nranks > 1:
            if not self._p_same_over_ranks([n, launches]):
                raise RuntimeError("history_read: the ranks hold different numbers of records")
            full = np.full((n + 1, 2 + 3 * hist.nprobes), -0.0)        # (+ one row: the ranks' dropped counts)
            full[:n, :2] = rec[:, :2]
            cols = (2 + 3 * np.repeat(hist.mine, 3) + np.tile(np.arange(3), len(hist.mine))).astype(np.int64)
            full[:n, cols] = rec[:, 2:]
            full[n, 0] = float(dropped)
            tot = self._p_allreduce_array(full.ravel()).reshape(full.shape)
            dropped, rec = int(tot[n, 0]), tot[:n]
        return rec[:, :2].copy(), rec[:, 2:].reshape(n, hist.nprobes, 3).copy(), int(launches), int(dropped)

    def history_free(self, hist):
        self._release(hist, self._p_history_free)

    # ---- body surface loads (include/fs_hip.h fs_loads_*): force, moment and per-face pressure / shear sums, one launch sequence per step -----
    LOADS_REC = 6       # Fpx, Fpy, Fvx, Fvy, Mp, Mv
    LOADS_SUMS = 4      # S_p, S_pp, S_t, S_tt per face

    def loads_create(self, faces, centre, capacity, every=1, start=0):
        """A device body tracker for FluidSimulator.track_body: faces (F, 3) global (x, y, dir) of fs.history.body_faces, F >= 1, centre
        (cx, cy) in cell units, a ring of `capacity` records.  Launch n (from 0) of loads_record samples when n + 1 > start and
        (n + 1 - start) % every == 0.  A slab keeps the faces whose fluid cell lies in its owned rows: the launch reads no ghost row, needs
        no exchange and sits in a tape as an ordinary kernel op.  Not allowed during a graph capture."""
        from .history import owned
        self._host_only("loads_create during a graph capture")
        faces = np.asarray(faces, np.int32).reshape(-1, 3)
        centre = np.asarray(centre, np.float64).ravel()
        capacity = int(capacity)
        if len(faces) < 1:
            raise ValueError("a body tracker needs at least one face")
        if centre.shape != (2,) or not np.all(np.isfinite(centre)):
            raise ValueError("centre must be two finite numbers (cx, cy)")
        every, start = self._check_cadence(every, start, capacity)
        mine = owned(faces, self.y0, self.nyl)
        # (a slab whose rows touch no face of the body still needs a handle: the counters advance on every rank)
        h = self._p_loads_create(np.ascontiguousarray(faces[mine]), centre, capacity, every, start) if len(mine) else None
        return self._adopt(h, Loads(h, len(faces), mine, capacity, every, start))

    def loads_record(self, lo, dx, inv_re, v, p):
        """One launch sequence of the tracker on the current v and p; whether it samples is decided on the device.  A limit_field v still
        owes stays deferred: the kernel limits the values as the pass would store them.  Not a _run: no flush, no exchange, no ghost row - on
        slabs a kernel op of its own in the logged period (writes no field)."""
        if lo._h is None:
            # this slab owns no face of the body: nothing to launch, but the logged period keeps the shape it has on the other ranks
            # (tape_period compiles a tape only when all ranks' tapes have the same length)
            return self._ride("loads_idle")
        self._ride("loads_record", (lo._h, float(dx), float(inv_re), self._limit_of(v), v._h, p._h))

    def loads_read(self, lo):
        """Empty the ring -> (records (n, 6): Fpx, Fpy, Fvx, Fvy, Mp, Mv; launches, samples, records dropped).  Across slabs the records
        add, and the ranks that hold faces must agree on the counters (a slab without a face of the body holds none).  Collective on slab
        runs; not allowed during a graph capture."""
        self._host_only("loads_read during a graph capture: the ring is read between captures / replays")
        if lo._h is not None:
            rec, launches, samples, dropped = self._p_loads_read(lo._h, lo.capacity)
        else:
            rec, launches, samples, dropped = np.zeros((0, self.LOADS_REC)), 0, 0, 0
        n = rec.shape[0]
        if self.nranks > 1:
            top = [int(x) for x in self._p_max_over_ranks([n, launches, samples])]
            odd = lo._h is not None and top != [n, launches, samples]
            n, launches, samples = top
            full = np.full((n + 1, self.LOADS_REC), -0.0)        # (+ one row: the ranks' dropped counts, and who disagrees)
            if lo._h is not None and not odd:
                full[:n] = rec
            full[n, 0], full[n, 1] = float(dropped), float(odd)
            tot = self._p_allreduce_array(full.ravel()).reshape(full.shape)
            if tot[n, 1] > 0:
                raise RuntimeError("loads_read: the ranks hold different launch / sample / record counts")
            dropped, rec = int(tot[n, 0]), tot[:n]
        return rec.copy(), int(launches), int(samples), int(dropped)

    def loads_sums(self, lo, write=None, launches=None, samples=None):
        """-> the per-face sums, float64 (4, F): S_p, S_pp, S_t, S_tt in the order of the GLOBAL face list.  On slabs every face comes from
        the rank that owns it (the others contribute -0.0, which leaves every value's bits alone; collective).  write=(4, F) array with
        launches, samples: the inverse (resume) - each slab keeps its own faces.  Not allowed during a graph capture."""
        self._host_only("loads_sums during a graph capture")
        if write is not None:
            write = np.asarray(write, np.float64)
            if write.shape != (self.LOADS_SUMS, lo.nfaces):
                raise ValueError(f"expected sums of shape {(self.LOADS_SUMS, lo.nfaces)}, got {write.shape}")
            launches, samples = self._check_counters(launches, samples)
            if lo._h is not None:
                self._p_loads_sums_write(lo._h, np.ascontiguousarray(write[:, lo.mine]), launches, samples)
            return None
        full = np.full((self.LOADS_SUMS, lo.nfaces), -0.0) if self.nranks > 1 else np.zeros((self.LOADS_SUMS, lo.nfaces))
        if lo._h is not None:
            full[:, lo.mine] = self._p_loads_sums_read(lo._h, len(lo.mine))
        if self.nranks > 1:
            full = self._p_allreduce_array(full.ravel()).reshape(full.shape)
        return full

    def loads_reset(self, lo):
        """Sums and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._host_only("loads_reset during a graph capture")
        if lo._h is not None:
            self._p_loads_reset(lo._h)

    def loads_free(self, lo):
        self._release(lo, self._p_loads_free)

    # ---- time averages (include/fs_hip.h fs_mean_*): seven planes of double sums over the owned rows, fed by one launch per step -----------
    MEAN_PLANES = 7     # S_u, S_w, S_p, S_uu, S_ww, S_uw, S_pp (fs.averages.SUMS)

    def mean_create(self, every=1, start=0):
        """Device accumulators for FluidSimulator.start_averaging: 56 bytes per owned cell, zeroed.  Launch n (from 0) of mean_accumulate
        samples when n + 1 > start and (n + 1 - start) % every == 0.  Not allowed during a graph capture."""
        self._host_only("mean_create during a graph capture")
        every, start = self._check_cadence(every, start)
        h = self._p_mean_create(every, start)
        return self._adopt(h, Mean(h, every, start))

    def mean_accumulate(self, mean, v, p):
        """Add the current v and p to the sums when this launch is a sampling one; the counters advance on the device.  A limit_field v
        still owes stays deferred: the kernel limits the values as the pass would store them.  Not a _run: no flush, no exchange, no ghost
        row - on slabs a kernel op of its own in the logged period (writes no field)."""
        self._ride("mean_accumulate", (mean._h, self._limit_of(v), v._h, p._h))

    def mean_read(self, mean, local=False):
        """-> (sums float64 (7, X, Y) in the order of fs.averages.SUMS, launches, samples).  On slabs the ranks' owned rows are assembled
        like Field.to_numpy (allgather; local=True: this slab's rows only) and all ranks must report the same counters.  Collective on
        slab runs; not allowed during a graph capture."""
        self._host_only("mean_read during a graph capture: the sums are a download (read between captures / replays)")
        mine, launches, samples = self._p_mean_read(mean._h)
        launches, samples = int(launches), int(samples)
        if self.nranks > 1 and not self._p_same_over_ranks([launches, samples]):
            raise RuntimeError("mean_read: the ranks hold different launch / sample counts")
        if local or self.nranks == 1:
            return mine, launches, samples
        if self.allgather is None:
            raise RuntimeError("mean_read() on a slab needs runtime.init(allgather=...) or local=True")
        return np.concatenate(self.allgather(mine), axis=2), launches, samples

    def mean_write(self, mean, sums, launches, samples):
        """Restore what mean_read returned (resume): sums is the GLOBAL (7, X, Y) array, each slab keeps its owned rows."""
        self._host_only("mean_write during a graph capture")
        sums = np.asarray(sums, np.float64)
        if sums.shape != (self.MEAN_PLANES, self.nx, self.ny):
            raise ValueError(f"expected sums of shape {(self.MEAN_PLANES, self.nx, self.ny)}, got {sums.shape}")
        launches, samples = self._check_counters(launches, samples)
        self._p_mean_write(mean._h, np.ascontiguousarray(sums[:, :, self.y0:self.y0 + self.nyl]), launches, samples)

    def mean_reset(self, mean):
        """Sums and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._host_only("mean_reset during a graph capture")
        self._p_mean_reset(mean._h)

    def mean_finalize(self, mean, v_out, p_out):
        """The means as fields: S_u / n, S_w / n into the 2-channel v_out, S_p / n into the 1-channel p_out (n = samples, > 0), wall cells
        0, in the fields' precision.  Owned rows only: on slabs the targets' ghost rows are stale afterwards (valid = 0), and whatever reads
        them exchanges first.  Not allowed during a graph capture."""
        self._host_only("mean_finalize during a graph capture")
        self._p_mean_finalize(mean._h, v_out._h, p_out._h)
        self._overwritten(v_out, p_out)

    def mean_free(self, mean):
        self._release(mean, self._p_mean_free)

    # ---- harmonic flow modes (include/fs_hip.h fs_modes_*): 3 (1 + 2K) planes of Fourier sums over the owned rows, one launch per step ----
    MODES_MAX_FREQ = 4

    @staticmethod
    def modes_planes(nfreq):
        """Planes of an accumulator of nfreq frequencies: 3 B, B = 1 + 2 nfreq."""
        return 3 * (1 + 2 * int(nfreq))

    @staticmethod
    def modes_scalars(nfreq):
        """Scalars of an accumulator: the 2 nfreq phasor entries, then the B (B + 1) / 2 entries of the Gram matrix's upper triangle."""
        b = 1 + 2 * int(nfreq)
        return 2 * int(nfreq) + b * (b + 1) // 2

    def modes_create(self, cos_sin, every=1, start=0):
        """Device accumulators for FluidSimulator.start_modes: cos_sin float64 (K, 2), the cosine and sine of each frequency's phase step per
        sample (fs.modes.phasor_steps), 1 <= K <= MODES_MAX_FREQ; 24 (1 + 2K) bytes per owned cell, zeroed, every phasor (1, 0).  Launch n
        (from 0) of modes_accumulate samples when n + 1 > start and (n + 1 - start) % every == 0.  Not allowed during a graph capture."""
        self._host_only("modes_create during a graph capture")
        cos_sin = np.ascontiguousarray(cos_sin, np.float64)
        if cos_sin.ndim != 2 or cos_sin.shape[1] != 2 or not 1 <= len(cos_sin) <= self.MODES_MAX_FREQ:
            raise ValueError(f"cos_sin must have shape (K, 2) with 1 <= K <= {self.MODES_MAX_FREQ}, got {cos_sin.shape}")
        if not np.all(np.isfinite(cos_sin)):
            raise ValueError("cos_sin must be finite")
        every, start = self._check_cadence(every, start)
        h = self._p_modes_create(cos_sin, every, start)
        return self._adopt(h, Modes(h, len(cos_sin), every, start))

    def modes_accumulate(self, modes, v, p):
        """Add the current v and p, weighted by the basis of the current phasors, to the planes when this launch is a sampling one; Gram
        matrix, counters and phasors advance on the device.  A limit_field v still owes stays deferred: the kernel limits the values as the
        pass would store them.  Not a _run: no flush, no exchange, no ghost row - on slabs a kernel op of its own in the logged period
        (writes no field)."""
        self._ride("modes_accumulate", (modes._h, self._limit_of(v), v._h, p._h))

    def modes_read_scalars(self, modes):
        """-> (None, scalars, launches, samples): modes_read without the download of the planes."""
        return self.modes_read(modes, local=True, with_sums=False)

    def modes_read(self, modes, local=False, with_sums=True):
        """-> (sums float64 (3 B, X, Y): plane a B + j of field a in (u, w, p) and basis entry j of [1, c_1, s_1, ...]; scalars float64
        (modes_scalars,): phasors, Gram triangle; launches, samples).  On slabs the ranks' owned rows are assembled like Field.to_numpy
        (allgather; local=True: this slab's rows only) and all ranks must hold the same counters and scalars (RuntimeError otherwise).
        Collective on slab runs; not allowed during a graph capture."""
        self._host_only("modes_read during a graph capture: the sums are a download (read between captures / replays)")
        mine, scalars, launches, samples = self._p_modes_read(modes._h, modes.nfreq, with_sums)
        launches, samples = int(launches), int(samples)
        # (the scalars are compared by their bits, as 32-bit halves: the collective carries integers below 2^40)
        if self.nranks > 1 and not self._p_same_over_ranks([launches, samples] + [int(x) for x in np.ascontiguousarray(scalars).view(np.uint32)]):
            raise RuntimeError("modes_read: the ranks hold different counters, phasors or Gram matrices")
        if local or self.nranks == 1:
            return mine, scalars, launches, samples
        if self.allgather is None:
            raise RuntimeError("modes_read() on a slab needs runtime.init(allgather=...) or local=True")
        return np.concatenate(self.allgather(mine), axis=2), scalars, launches, samples

    def modes_write(self, modes, sums, scalars, launches, samples):
        """Restore what modes_read returned (resume): sums is the GLOBAL (3 B, X, Y) array, each slab keeps its owned rows."""
        self._host_only("modes_write during a graph capture")
        sums, scalars = np.asarray(sums, np.float64), np.ascontiguousarray(scalars, np.float64)
        shape = (self.modes_planes(modes.nfreq), self.nx, self.ny)
        if sums.shape != shape:
            raise ValueError(f"expected sums of shape {shape}, got {sums.shape}")
        if scalars.shape != (self.modes_scalars(modes.nfreq),):
            raise ValueError(f"expected {self.modes_scalars(modes.nfreq)} scalars, got shape {scalars.shape}")
        launches, samples = self._check_counters(launches, samples)
        self._p_modes_write(modes._h, np.ascontiguousarray(sums[:, :, self.y0:self.y0 + self.nyl]), scalars, launches, samples)

    def modes_reset(self, modes):
        """Planes, Gram matrix and sample count to zero, the phasors to (1, 0); the launch count runs on.  Not allowed during a graph capture."""
        self._host_only("modes_reset during a graph capture")
        self._p_modes_reset(modes._h)

    def modes_combine(self, modes, weights, v_out, p_out):
        """The planes reduced to fields: sum_j weights[a, j] * plane[a B + j] (in double, j ascending) for a = u, w into the 2-channel v_out
        and a = p into the 1-channel p_out, wall cells 0, in the fields' precision; weights float64 (3, B).  Owned rows only: on slabs the
        targets' ghost rows are stale afterwards (valid = 0).  Not allowed during a graph capture."""
        self._host_only("modes_combine during a graph capture")
        weights = np.ascontiguousarray(weights, np.float64)
        if weights.shape != (3, 1 + 2 * modes.nfreq):
            raise ValueError(f"expected weights of shape {(3, 1 + 2 * modes.nfreq)}, got {weights.shape}")
        self._p_modes_combine(modes._h, weights, v_out._h, p_out._h)
        self._overwritten(v_out, p_out)

    def modes_rows(self, nfreq):
        """{"accumulate", "combine"}: the rows per workgroup the next launches take on this context (fs_modes_rows; FS_DIAG_WGS moves them)."""
        return dict(zip(("accumulate", "combine"), self._p_modes_rows(int(nfreq))))

    def modes_free(self, modes):
        self._release(modes, self._p_modes_free)

    # ---- snapshot POD (include/fs_hip.h fs_pod_*): a ring of M resident snapshots of u, w, p, one launch per step; Gram matrix on the device ----
    POD_MAX = 64

    def pod_create(self, slots, every=1, start=0):
        """Device snapshots for FluidSimulator.start_pod: a ring of `slots` = M snapshots (2 <= M <= POD_MAX) of u, w, p in the fields'
        precision - 12 M bytes per cell in f32, 24 M in f64 - zeroed.  Launch n (from 0) of pod_launch samples when n + 1 > start and
        (n + 1 - start) % every == 0.  Single-context grids only (FsError on a slab: the Gram matrix would need a rank-ordered reduction of
        per-rank matrices); not allowed during a graph capture."""
        RideOps._host_only(self, "pod_create during a graph capture")      # (through the class, as the tracer calls: the tests ask objects that are no devices)
        RideOps._single_context(self, "snapshot POD needs", "the Gram matrix needs a rank-ordered reduction")
        slots = int(slots)
        if not 2 <= slots <= self.POD_MAX:
            raise ValueError(f"snapshots must be 2 .. {self.POD_MAX}, got {slots}")
        every, start = self._check_cadence(every, start)
        h = self._p_pod_create(slots, every, start)
        return self._adopt(h, Pod(h, slots, every, start))

    def pod_launch(self, pod, v, p):
        """Store the current v and p into slot samples % M when this launch is a sampling one; the counters advance on the device.  A
        limit_field v still owes stays deferred: the kernel limits the values as the pass would store them.  Not a _run: no flush, no
        exchange, no ghost row (writes no field)."""
        self._ride("pod_launch", (pod._h, self._limit_of(v), v._h, p._h))

    def pod_read(self, pod):
        """-> (launches, samples).  Not allowed during a graph capture."""
        self._host_only("pod_read during a graph capture: the counters are a download (read between captures / replays)")
        launches, samples = self._p_pod_read(pod._h)
        return int(launches), int(samples)

    def pod_gram(self, pod):
        """-> (G float64 (n, n) in SLOT order, launches, samples): the Gram matrix of the n = min(samples, M) resident snapshots,
        G[a][b] = sum over the cells of u_a u_b + w_a w_b in double, reduced on the device in a fixed order (csrc/fs_pod.h): only n * n
        doubles are downloaded.  Not allowed during a graph capture."""
        self._host_only("pod_gram during a graph capture: the matrix is a download (read between captures / replays)")
        G, launches, samples = self._p_pod_gram(pod._h, pod.slots)
        return G, int(launches), int(samples)

    def pod_combine(self, pod, weights, v_out, p_out):
        """The slots reduced to fields: sum_m weights[m] * slot_m (in double, m ascending) of u, w into the 2-channel v_out and of p into
        the 1-channel p_out, wall cells 0, in the fields' precision; weights float64 (M,).  Not allowed during a graph capture."""
        self._host_only("pod_combine during a graph capture")
        weights = np.ascontiguousarray(weights, np.float64)
        if weights.shape != (pod.slots,):
            raise ValueError(f"expected weights of shape {(pod.slots,)}, got {weights.shape}")
        self._p_pod_combine(pod._h, weights, v_out._h, p_out._h)
        self._overwritten(v_out, p_out)

    def pod_get(self, pod):
        """-> (slots (M, 3, X, Y) in the fields' dtype: u, w, p of every slot; launches, samples) - the whole ring, for checkpoints."""
        self._host_only("pod_get during a graph capture")
        launches, samples = self.pod_read(pod)
        return self._p_pod_get(pod._h, pod.slots), launches, samples

    def pod_set(self, pod, slots, launches, samples):
        """Restore what pod_get returned (resume)."""
        self._host_only("pod_set during a graph capture")
        slots = np.asarray(slots)
        shape = (pod.slots, 3, self.nx, self.ny)
        if slots.shape != shape:
            raise ValueError(f"expected slots of shape {shape}, got {slots.shape}")
        launches, samples = self._check_counters(launches, samples)
        self._p_pod_set(pod._h, slots.astype(self.dtype, copy=False), launches, samples)

    def pod_reset(self, pod):
        """Slots and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._host_only("pod_reset during a graph capture")
        self._p_pod_reset(pod._h)

    def pod_free(self, pod):
        self._release(pod, self._p_pod_free)

    # ---- vortex identification (include/fs_hip.h fs_vortex_*): criterion, labelled components and integer records; csrc/fs_vortex.h ----
    VORTEX_CRITERIA = ("q", "swirl", "vorticity")
    VORTEX_MAX = 1024

    def _vortex_host_call(self, what):
        RideOps._host_only(self, f"{what} during a graph capture")
        RideOps._single_context(self, "vortex identification needs", "the components would have to be united across ranks")

    def _vortex_criterion(self, criterion):
        if criterion not in self.VORTEX_CRITERIA:
            raise ValueError(f"criterion must be one of {self.VORTEX_CRITERIA}, got {criterion!r}")
        return self.VORTEX_CRITERIA.index(criterion)

    def vortex_create(self, criterion, threshold, exponent, every=1, start=0, min_area=4, max_vortices=64, max_components=65536, capacity=256):
        """A device vortex tracker for FluidSimulator.track_vortices: flag, label and id planes of the grid (9 bytes per cell), a table of
        120 bytes per component and a ring of `capacity` samples of 8 + 16 max_vortices int64 words.  threshold: finite, in 1 / time^2;
        exponent e: q = llrint(ldexp(om, 30 - e)).  Launch n (from 0) of vortex_launch samples when n + 1 > start and (n + 1 - start) %
        every == 0.  Single-context grids only; not allowed during a graph capture."""
        RideOps._vortex_host_call(self, "vortex_create")      # (through the class, as the tracer calls: the tests ask objects that are no devices)
        which = self._vortex_criterion(criterion)
        if threshold is None or not np.isfinite(float(threshold)):
            raise ValueError(f"threshold must be a finite number (1 / time^2), got {threshold!r}")
        every, start = self._check_cadence(every, start, capacity)
        min_area, max_vortices, max_components, exponent = int(min_area), int(max_vortices), int(max_components), int(exponent)
        if not 1 <= max_vortices <= self.VORTEX_MAX:
            raise ValueError(f"max_vortices must be 1 .. {self.VORTEX_MAX}, got {max_vortices}")
        if min_area < 1 or not 1 <= max_components <= 1 << 24:
            raise ValueError("min_area must be >= 1 and max_components 1 .. 2^24")
        if not -900 <= exponent <= 900:
            raise ValueError(f"exponent {exponent} out of range")
        h = self._p_vortex_create(which, float(threshold), exponent, every, start, min_area, max_vortices, max_components, int(capacity))
        return self._adopt(h, Vortex(h, criterion, float(threshold), exponent, every, start, min_area, max_vortices, max_components, int(capacity)))

    def vortex_launch(self, vx, dx, v):
        """The launches of one step: when this launch samples, flag, label and reduce the components of v and append a sample to the ring;
        the counters advance on the device.  A limit_field v still owes stays deferred: the kernels limit the values they read.  Not a
        _run: no flush, no exchange, no ghost row (writes no field)."""
        self._ride("vortex_launch", (vx._h, self._limit_of(v), float(dx), v._h))

    def vortex_read(self, vx):
        """Drain the ring -> (int64 (n, 8 + 16 max_vortices) samples, launches, samples lost to a full ring since the last read)."""
        self._host_only("vortex_read during a graph capture: the ring is a download (read between captures / replays)")
        return self._p_vortex_read(vx._h, vx.capacity, 8 + 16 * vx.max_vortices)

    def vortex_labels(self, vx):
        """-> {"flags": uint8 (X, Y), "labels": int32 (X, Y)} of the last sampling launch: 1 / 2 / 0, and the smallest j * X + i of the cell's
        component (-1 without a flag)."""
        self._host_only("vortex_labels during a graph capture")
        flags, labels = self._p_vortex_get_labels(vx._h)
        return {"flags": flags, "labels": labels}

    def vortex_set(self, vx, launches):
        """The launch count of a resumed run; the ring is emptied."""
        self._host_only("vortex_set during a graph capture")
        if int(launches) < 0:
            raise ValueError("launches must be >= 0")
        self._p_vortex_set(vx._h, int(launches))

    def vortex_label(self, flags):
        """The labels of a flag plane uint8 (X, Y): cells with equal non-zero bytes join over their 4 neighbours -> int32 (X, Y)."""
        self._vortex_host_call("vortex_label")
        flags = np.asarray(flags)
        if flags.shape != (self.nx, self.ny) or flags.dtype != np.uint8:
            raise ValueError(f"expected uint8 flags of shape {(self.nx, self.ny)}, got {flags.dtype} {flags.shape}")
        return self._p_vortex_label(flags)

    def vortex_criterion(self, criterion, dx, v):
        """The criterion field of v -> float64 (X, Y), 0 on cells that are not fluid (csrc/fs_vortex.h a)."""
        self._vortex_host_call("vortex_criterion")
        return self._p_vortex_criterion(self._vortex_criterion(criterion), self._limit_of(v), float(dx), v._h)

    def vortex_free(self, vx):
        self._release(vx, self._p_vortex_free)

    # ---- field distributions (include/fs_hip.h fs_dist_*): histograms accumulated on the device, exact order statistics; csrc/fs_dist.h ----
    DIST_QUANTITIES = ("u", "w", "p", "speed", "vorticity", "q", "swirl")
    DIST_MAX_BINS, DIST_MAX_CHANNELS, DIST_MAX_RANKS, DIST_NTAIL = 4096, 4, 8, 4

    def _dist_host_call(self, what):
        RideOps._host_only(self, f"{what} during a graph capture")
        RideOps._single_context(self, "field distributions need", "the tables would have to be added across ranks")

    def _dist_quantity(self, quantity):
        if quantity not in RideOps.DIST_QUANTITIES:
            raise ValueError(f"quantity must be one of {RideOps.DIST_QUANTITIES}, got {quantity!r}")
        return RideOps.DIST_QUANTITIES.index(quantity)

    def _dist_box(self, box):
        return (0, 0, self.nx, self.ny) if box is None else RideOps._cell_box(self, box)

    def _dist_side(self, spec):
        q = RideOps._dist_quantity(self, spec.get("quantity"))
        bins = int(spec.get("bins", 0))
        if not 1 <= bins <= RideOps.DIST_MAX_BINS:
            raise ValueError(f"bins must be 1 .. {RideOps.DIST_MAX_BINS}, got {bins}")
        if spec.get("range") is None:
            raise ValueError("range = (lo, hi) must be given: the bins of an accumulated table do not move")
        lo, hi = (float(x) for x in spec["range"])
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"range must be finite, got ({lo}, {hi})")
        if not lo < hi:
            raise ValueError(f"range must satisfy lo < hi, got ({lo}, {hi})")
        inv = bins / (hi - lo) if math.isfinite(hi - lo) else 0.0
        if not (math.isfinite(inv) and inv > 0.0):
            raise ValueError(f"range ({lo}, {hi}) is too narrow or too wide: bins / (hi - lo) must be finite and positive")
        return q, bins, lo, hi

    def dist_channel(self, spec):
        """{"quantity", "bins", "range"[, "box"][, "against": {"quantity", "bins", "range"}]} -> DistChannel, checked (ValueError)."""
        if not isinstance(spec, dict):
            raise ValueError(f"a channel is a dict with quantity, bins and range, got {spec!r}")
        unknown = set(spec) - {"quantity", "bins", "range", "box", "against"}
        if unknown:
            raise ValueError(f"unknown channel keys {sorted(unknown)}")
        a = RideOps._dist_side(self, spec)
        b = (-1, 0, 0.0, 0.0)
        if spec.get("against") is not None:
            b = RideOps._dist_side(self, spec["against"])
            if a[1] * b[1] > RideOps.DIST_MAX_BINS:
                raise ValueError(f"a joint table holds at most {RideOps.DIST_MAX_BINS} bins, got {a[1]} x {b[1]}")
        return DistChannel(*a, *b, RideOps._dist_box(self, spec.get("box")))

    def dist_create(self, channels, every=1, start=0):
        """Device tables for FluidSimulator.start_distributions / histogram: 1 .. DIST_MAX_CHANNELS channels (dicts, see dist_channel), 64-bit
        counters, zeroed.  Launch n (from 0) of dist_launch samples when n + 1 > start and (n + 1 - start) % every == 0.  Single-context
        grids only (FsError on a slab); not allowed during a graph capture."""
        RideOps._dist_host_call(self, "dist_create")      # (through the class, as the tracer calls: the tests ask objects that are no devices)
        channels = [channels] if isinstance(channels, dict) else list(channels)
        if not 1 <= len(channels) <= RideOps.DIST_MAX_CHANNELS:
            raise ValueError(f"1 .. {RideOps.DIST_MAX_CHANNELS} channels, got {len(channels)}")
        chans = [RideOps.dist_channel(self, c) for c in channels]
        every, start = RideOps._check_cadence(every, start)
        h = self._p_dist_create(chans, every, start)
        return self._adopt(h, Dist(h, chans, every, start))

    def dist_launch(self, d, dx, v, p):
        """The launches of one step: one pass per channel that adds the cells' bins to its table when this launch samples, then the tick
        that advances the counters on the device.  A limit_field v still owes stays deferred: the kernel limits the values it reads.  Not
        a _run: no flush, no exchange, no ghost row (writes no field)."""
        self._ride("dist_launch", (d._h, self._limit_of(v), float(dx), v._h, p._h))

    def dist_read(self, d, chan):
        """-> (counts int64 of the channel's shape - (B,) or (Ba, Bb) -, tails int64 (4,): below, above, nan, 0 - joint: outside, 0, nan, 0 -,
        launches, samples).  Not allowed during a graph capture."""
        self._host_only("dist_read during a graph capture: the tables are a download (read between captures / replays)")
        c = d.channels[chan]
        counts, tails, launches, samples = self._p_dist_read(d._h, chan, c.bins * max(1, c.bins_b))
        if c.joint:
            counts = np.ascontiguousarray(counts.reshape(c.bins_b, c.bins).T)      # (bin bb * Ba + ba)
        return counts, tails, int(launches), int(samples)

    def dist_get(self, d):
        """-> (every table and its tails as one int64 array, launches, samples), for checkpoints."""
        self._host_only("dist_get during a graph capture")
        _, _, launches, samples = self._p_dist_read(d._h, 0, 0)
        return self._p_dist_get(d._h, d.words), int(launches), int(samples)

    def dist_set(self, d, words, launches, samples):
        """Restore what dist_get returned (resume)."""
        self._host_only("dist_set during a graph capture")
        words = np.ascontiguousarray(words, np.int64)
        if words.shape != (d.words,):
            raise ValueError(f"expected {d.words} table words, got {words.shape}")
        launches, samples = self._check_counters(launches, samples)
        self._p_dist_set(d._h, words, launches, samples)

    def dist_reset(self, d):
        """Tables and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._host_only("dist_reset during a graph capture")
        self._p_dist_reset(d._h)

    def dist_free(self, d):
        self._release(d, self._p_dist_free)

    def dist_select(self, quantity, box, dx, v, p, ranks):
        """Exact order statistics of `quantity` over the fluid cells of `box` (None: the whole grid): -> (values float64 (R,), n, nan) with
        values[k] the ranks[k]-th smallest (0-based, ascending, at most DIST_MAX_RANKS) of the n values that are not NaN, as a full sort
        would place it; nan: selected cells whose value is NaN.  ranks=(): n and nan alone.  ValueError for a rank >= n (and for any rank
        when n == 0).  8 bytes per cell of the box on the device for the duration of the call."""
        RideOps._dist_host_call(self, "dist_select")
        q = RideOps._dist_quantity(self, quantity)
        box = RideOps._dist_box(self, box)
        ranks = [int(r) for r in ranks]
        if len(ranks) > RideOps.DIST_MAX_RANKS:
            raise ValueError(f"at most {RideOps.DIST_MAX_RANKS} ranks per call, got {len(ranks)}")
        if any(r < 0 for r in ranks) or any(a > b for a, b in zip(ranks, ranks[1:])):
            raise ValueError(f"ranks must be >= 0 and ascending, got {ranks}")
        return self._p_dist_select(q, box, self._limit_of(v), float(dx), v._h, p._h, ranks)

    # ---- what the plane accumulators share (_Planes: spec_*, xspec_*, flux_*, budget_*): read, get, set, reset, free ---------------------------
    @staticmethod
    def _check_dx(dx):
        dx = float(dx)
        if not (math.isfinite(dx) and dx > 0.0):
            raise ValueError(f"dx must be finite and > 0, got {dx}")
        return dx

    def _planes_read(self, obj, payload, what):
        self._host_only(f"{obj.kind}_read during a graph capture: {what} a download (read between captures / replays)")
        flat, launches, samples = getattr(self, f"_p_{obj.kind}_read")(obj._h, obj.words if payload else 0)
        return (obj.to_host(flat) if payload else None), int(launches), int(samples)

    def _planes_get(self, obj):
        self._host_only(f"{obj.kind}_get during a graph capture")
        flat, launches, samples = getattr(self, f"_p_{obj.kind}_get")(obj._h, obj.words)
        return obj.to_host(flat), int(launches), int(samples)

    def _planes_set(self, obj, planes, launches, samples, noun):
        self._host_only(f"{obj.kind}_set during a graph capture")
        planes = np.asarray(planes, np.float64)
        if planes.shape != obj.shape:
            raise ValueError(f"expected {noun} of shape {obj.shape}, got {planes.shape}")
        launches, samples = self._check_counters(launches, samples)
        getattr(self, f"_p_{obj.kind}_set")(obj._h, obj.to_device(planes), launches, samples)

    def _planes_reset(self, obj):
        self._host_only(f"{obj.kind}_reset during a graph capture")
        getattr(self, f"_p_{obj.kind}_reset")(obj._h)

    def _planes_free(self, obj):
        self._release(obj, getattr(self, f"_p_{obj.kind}_free"))

    # ---- energy spectra (include/fs_hip.h fs_spec_*): the windowed FFT of the velocity over a box, accumulated power; csrc/fs_spec.h ----
    SPEC_MIN_N, SPEC_MAX_N = 8, 4096

    def _spec_host_call(self, what):
        RideOps._host_only(self, f"{what} during a graph capture")
        RideOps._single_context(self, "energy spectra need", "the transform along y crosses the ranks")

    def spec_box(self, box):
        """(x0, y0, x1, y1) in global cells, half-open, inside the grid, both sides powers of two in SPEC_MIN_N .. SPEC_MAX_N -> the tuple
        of ints (ValueError)."""
        box = RideOps.flux_box(self, box)
        for n in (box[2] - box[0], box[3] - box[1]):
            if n & (n - 1) or not RideOps.SPEC_MIN_N <= n <= RideOps.SPEC_MAX_N:
                raise ValueError(f"the sides of a spectrum box must be powers of two in {RideOps.SPEC_MIN_N} .. {RideOps.SPEC_MAX_N}, "
                                 f"got {box[2] - box[0]} x {box[3] - box[1]}")
        return box

    def _spec_checked(self, box, tables, c1x, c1y, every, start):
        """What spec_create and xspec_create check alike (ValueError) -> (box, the four tables as contiguous float64, c1x, c1y, every, start)."""
        box = RideOps.spec_box(self, box)
        nx, ny = box[2] - box[0], box[3] - box[1]
        tabs = [np.ascontiguousarray(t, np.float64) for t in tables]
        for t, shape, name in zip(tabs, ((nx,), (ny,), (nx // 2, 2), (ny // 2, 2)), ("wx", "wy", "twx", "twy")):
            if t.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {t.shape}")
        c1x, c1y = float(c1x), float(c1y)
        if not (math.isfinite(c1x) and math.isfinite(c1y)):
            raise ValueError("the detrend pair must be finite")
        every, start = RideOps._check_cadence(every, start)
        return box, tabs, c1x, c1y, every, start

    def spec_create(self, box, wx, wy, twx, twy, c1x=0.0, c1y=0.0, detrend=False, every=1, start=0):
        """Device planes for FluidSimulator.start_spectra / spectrum / box_fft: wx (Nx,), wy (Ny,) the windows, twx (Nx / 2, 2), twy
        (Ny / 2, 2) the twiddles (cos, -sin) of 2 pi k / N - fs.spectra.window_table / twiddles -, the detrend pair.  40 bytes per cell of
        the box.  Launch n (from 0) of spec_launch samples when n + 1 > start and (n + 1 - start) % every == 0.  Box and sizes are checked
        (ValueError) before any device call.  Single-context grids only (FsError on a slab); not allowed during a graph capture."""
        box, tabs, c1x, c1y, every, start = RideOps._spec_checked(self, box, (wx, wy, twx, twy), c1x, c1y, every, start)
        RideOps._spec_host_call(self, "spec_create")
        h = self._p_spec_create(box, *tabs, c1x, c1y, bool(detrend), every, start)
        return self._adopt(h, Spec(h, box, detrend, every, start))

    def spec_launch(self, sp, v):
        """The launches of one step: load and transform along x, transpose, transform along y, detrend and power, the tick - all but the
        tick return at once unless this launch samples.  A limit_field v still owes stays deferred: the kernel limits the values it
        reads.  Not a _run: no flush, no exchange, no ghost row (writes no field)."""
        self._ride("spec_launch", (sp._h, self._limit_of(v), v._h))

    def spec_read(self, sp, power=True):
        """-> (power float64 (Nx, Ny): the sums of |Z'|^2 over the samples, not symmetrised - None with power=False -, launches, samples).
        Not allowed during a graph capture."""
        return self._planes_read(sp, power, "the power plane is")

    def spec_plane(self, sp):
        """-> Z' of the last sampling launch, complex128 (Nx, Ny) (zeros before the first).  Not allowed during a graph capture."""
        self._host_only("spec_plane during a graph capture")
        return self._p_spec_plane(sp._h, sp.nx * sp.ny).view(np.complex128).reshape(sp.nx, sp.ny)

    def spec_get(self, sp):
        """-> (the power plane float64 (Nx, Ny), launches, samples), for checkpoints."""
        return self._planes_get(sp)

    def spec_set(self, sp, power, launches, samples):
        """Restore what spec_get returned (resume)."""
        self._planes_set(sp, power, launches, samples, "a power plane")

    def spec_reset(self, sp):
        """Power plane and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._planes_reset(sp)

    def spec_free(self, sp):
        self._planes_free(sp)

    # ---- cross-spectra (include/fs_hip.h fs_xspec_*): the packed FFT of two quantities over a box, split and accumulated; csrc/fs_xspec.h ----
    XSPEC_NPLANE = 4

    def xspec_pair(self, pair):
        """(qa, qb) or (qa, None), names of DIST_QUANTITIES (a single name: (name, None)) -> the indices (qa, qb), qb -1 for None (ValueError)."""
        if isinstance(pair, str):
            pair = (pair, None)
        try:
            pair = tuple(pair)
        except TypeError:
            raise ValueError(f"pair must be (qa, qb) or (qa, None), got {pair!r}") from None
        if len(pair) != 2:
            raise ValueError(f"pair must be (qa, qb) or (qa, None), got {pair!r}")
        qa = RideOps._dist_quantity(self, pair[0])
        return qa, (-1 if pair[1] is None else RideOps._dist_quantity(self, pair[1]))

    def xspec_create(self, box, pair, dx, wx, wy, twx, twy, c1x=0.0, c1y=0.0, detrend=False, every=1, start=0):
        """Device planes for FluidSimulator.start_cross_spectra / cross_spectrum / pair_fft: box and tables as spec_create, pair as
        xspec_pair, dx for the gradients.  64 bytes per cell of the box, 40 for one scalar.  Everything is checked (ValueError) before any
        device call.  Single-context grids only (FsError on a slab); not allowed during a graph capture."""
        box, tabs, c1x, c1y, every, start = RideOps._spec_checked(self, box, (wx, wy, twx, twy), c1x, c1y, every, start)
        qa, qb = RideOps.xspec_pair(self, pair)
        dx = RideOps._check_dx(dx)
        RideOps._host_only(self, "xspec_create during a graph capture")
        RideOps._single_context(self, "cross-spectra need", "the transform along y crosses the ranks")
        h = self._p_xspec_create(box, qa, qb, dx, *tabs, c1x, c1y, bool(detrend), every, start)
        return self._adopt(h, XSpec(h, box, qa, qb, dx, detrend, every, start))

    def xspec_launch(self, xs, v, p):
        """The launches of one step: load the pair and transform along x, transpose, transform along y, split and accumulate, the tick - all
        but the tick return at once unless this launch samples.  A limit_field v still owes stays deferred: the kernel limits the values
        it reads.  Not a _run: no flush, no exchange, no ghost row (writes no field)."""
        self._ride("xspec_launch", (xs._h, self._limit_of(v), v._h, p._h))

    def xspec_read(self, xs, sums=True):
        """-> (sums float64 (planes, Nx, Ny): Paa, Pbb, Cre, Cim over the samples (one scalar: Paa alone) - None with sums=False -, launches,
        samples).  Not allowed during a graph capture."""
        return self._planes_read(xs, sums, "the planes are")

    def xspec_plane(self, xs):
        """-> Z' of the last sampling launch, complex128 (Nx, Ny) (zeros before the first).  Not allowed during a graph capture."""
        self._host_only("xspec_plane during a graph capture")
        return self._p_xspec_plane(xs._h, xs.nx * xs.ny).view(np.complex128).reshape(xs.nx, xs.ny)

    def xspec_get(self, xs):
        """-> (the accumulator planes float64 (planes, Nx, Ny), launches, samples), for checkpoints."""
        return self._planes_get(xs)

    def xspec_set(self, xs, sums, launches, samples):
        """Restore what xspec_get returned (resume)."""
        self._planes_set(xs, sums, launches, samples, "accumulator planes")

    def xspec_reset(self, xs):
        """Accumulators and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._planes_reset(xs)

    def xspec_free(self, xs):
        self._planes_free(xs)

    # ---- scale-to-scale fluxes (include/fs_hip.h fs_flux_*): box filters of u, w and the vorticity, the sub-filter stresses, accumulated
    #      PI, ZF and K per cell of a box; csrc/fs_flux.h ----
    FLUX_NQ, FLUX_NSUM, FLUX_MAX_WIDTHS, FLUX_MAX_R = 8, 3, 8, 64

    def flux_box(self, box):
        """(x0, y0, x1, y1) in global cells, half-open, inside the grid -> the tuple of ints (ValueError)."""
        try:
            return RideOps._cell_box(self, box)
        except TypeError:      # (what is no sequence of numbers; the distributions let this one through)
            raise ValueError(f"box must be (x0, y0, x1, y1), got {box!r}") from None

    def flux_valid(self, box, r):
        """The valid cells of half-width r inside the box, (x0, y0, x1, y1) half-open: r + 1 <= i <= X - 2 - r, r + 1 <= j <= Y - 2 - r."""
        return (max(box[0], r + 1), max(box[1], r + 1), min(box[2], self.nx - 1 - r), min(box[3], self.ny - 1 - r))

    def flux_half_widths(self, box, half_widths):
        """1 .. FLUX_MAX_WIDTHS ints in 1 .. FLUX_MAX_R, strictly increasing, each with a valid cell inside the box -> the tuple (ValueError)."""
        if isinstance(half_widths, (int, np.integer)):
            half_widths = (half_widths,)
        try:
            hw = tuple(half_widths)
        except TypeError:
            raise ValueError(f"half_widths must be a sequence of integers, got {half_widths!r}") from None
        if not 1 <= len(hw) <= RideOps.FLUX_MAX_WIDTHS:
            raise ValueError(f"half_widths must hold 1 .. {RideOps.FLUX_MAX_WIDTHS} half-widths, got {len(hw)}")
        for r in hw:
            if not isinstance(r, (int, np.integer)) or isinstance(r, bool) or not 1 <= r <= RideOps.FLUX_MAX_R:
                raise ValueError(f"a half-width must be an integer in 1 .. {RideOps.FLUX_MAX_R}, got {r!r}")
        hw = tuple(int(r) for r in hw)
        if any(b <= a for a, b in zip(hw, hw[1:])):
            raise ValueError(f"half_widths must be strictly increasing, got {hw}")
        for r in hw:
            v = RideOps.flux_valid(self, box, r)
            if v[0] >= v[2] or v[1] >= v[3]:
                raise ValueError(f"half-width {r} has no valid cell inside the box {box}: a valid cell keeps {r} + 1 cells from every edge of "
                                 f"the {self.nx} x {self.ny} grid")
        return hw

    def flux_create(self, box, half_widths, dx, every=1, start=0):
        """Device planes for FluidSimulator.start_scale_fluxes / scale_flux / filtered_fields.  192 bytes per cell of the box dilated by
        r_max + 1 (clipped to the grid) and 24 per cell of the box and half-width.  Everything is checked (ValueError) before any device
        call.  Single-context grids only (FsError on a slab); not allowed during a graph capture."""
        box = RideOps.flux_box(self, box)
        hw = RideOps.flux_half_widths(self, box, half_widths)
        dx = RideOps._check_dx(dx)
        every, start = RideOps._check_cadence(every, start)
        RideOps._host_only(self, "flux_create during a graph capture")
        RideOps._single_context(self, "scale fluxes need", "the filter along y crosses the ranks")
        h = self._p_flux_create(box, hw, dx, every, start)
        return self._adopt(h, Flux(h, box, hw, dx, every, start))

    def flux_launch(self, fx, v):
        """The launches of one step: the base planes, per half-width the row sums, the column sums and the stencil with its three sums, the
        tick - all but the tick return at once unless this launch samples.  A limit_field v still owes stays deferred: the kernel limits
        the values it reads.  Not a _run: no flush, no exchange, no ghost row (writes no field)."""
        self._ride("flux_launch", (fx._h, self._limit_of(v), v._h))

    def flux_read(self, fx, sums=True):
        """-> (sums float64 (n_r, 3, Nx, Ny): PI, ZF, K over the samples per half-width - None with sums=False -, launches, samples).  Not
        allowed during a graph capture."""
        return self._planes_read(fx, sums, "the planes are")

    def flux_filtered(self, fx, half_width):
        """-> the eight filtered planes of `half_width` (one of the object's) over the box from the last sampling launch, float64
        (8, Nx, Ny); +0 where the window leaves the grid, zeros before the first sample.  Not allowed during a graph capture."""
        self._host_only("flux_filtered during a graph capture")
        if half_width not in fx.half_widths:
            raise ValueError(f"half_width must be one of {fx.half_widths}, got {half_width!r}")
        flat = self._p_flux_filtered(fx._h, fx.half_widths.index(half_width), RideOps.FLUX_NQ * fx.nx * fx.ny)
        return np.ascontiguousarray(flat.reshape(RideOps.FLUX_NQ, fx.ny, fx.nx).transpose(0, 2, 1))

    def flux_get(self, fx):
        """-> (the sums float64 (n_r, 3, Nx, Ny), launches, samples), for checkpoints."""
        return self._planes_get(fx)

    def flux_set(self, fx, sums, launches, samples):
        """Restore what flux_get returned (resume)."""
        self._planes_set(fx, sums, launches, samples, "sums")

    def flux_reset(self, fx):
        """Sums and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._planes_reset(fx)

    def flux_free(self, fx):
        self._planes_free(fx)

    # ---- kinetic-energy budget (include/fs_hip.h fs_budget_*): 21 planes of raw moments over the fluid cells of a box, one launch per step;
    #      csrc/fs_budget.h ----
    BUDGET_NPLANE = 21

    def budget_create(self, box, dx, every=1, start=0):
        """Device planes for FluidSimulator.start_budget / budget_sample: 168 bytes per cell of the box (x0, y0, x1, y1), half-open, anything
        inside the grid with at least one cell.  Everything is checked (ValueError) before any device call; a box without a fluid cell is
        refused by the caller that knows the mask (FluidSimulator) and by the library.  Single-context grids only (FsError on a slab); not
        allowed during a graph capture."""
        box = RideOps.flux_box(self, box)
        dx = RideOps._check_dx(dx)
        every, start = RideOps._check_cadence(every, start)
        RideOps._host_only(self, "budget_create during a graph capture")
        RideOps._single_context(self, "the budget needs", "the gradient along y crosses the ranks")
        h = self._p_budget_create(box, dx, every, start)
        return self._adopt(h, Budget(h, box, dx, every, start))

    def budget_launch(self, bg, v, p):
        """The launches of one step: the accumulation - it returns at once unless this launch samples - and the tick.  A limit_field v still
        owes stays deferred: the kernel limits the values it reads, the neighbours' too.  Not a _run: no flush, no exchange, no ghost row
        (writes no field)."""
        self._ride("budget_launch", (bg._h, self._limit_of(v), v._h, p._h))

    def budget_read(self, bg, sums=True):
        """-> (sums float64 (21, Nx, Ny) in the order of fs.budgets.PLANES - None with sums=False -, launches, samples).  Not allowed during
        a graph capture."""
        return self._planes_read(bg, sums, "the planes are")

    def budget_get(self, bg):
        """-> (the sums float64 (21, Nx, Ny), launches, samples), for checkpoints."""
        return self._planes_get(bg)

    def budget_set(self, bg, sums, launches, samples):
        """Restore what budget_get returned (resume)."""
        self._planes_set(bg, sums, launches, samples, "sums")

    def budget_reset(self, bg):
        """Sums and sample count to zero; the launch count runs on.  Not allowed during a graph capture."""
        self._planes_reset(bg)

    def budget_free(self, bg):
        self._planes_free(bg)

    # ---- flow maps (include/fs_hip.h fs_flowmap_*): a lattice of particles carried through the resident snapshots of a POD; csrc/fs_lcs.h ----
    def flowmap_create(self, box=None, refine=1):
        """A device lattice for FluidSimulator.flow_map: refine x refine nodes per cell of the cell box (x0, y0, x1, y1) (None: the whole
        domain), seeded at (x0 + (a + 0.5) / refine, y0 + (b + 0.5) / refine); nodes that start in a wall cell are UNSEEDED.  28 bytes per
        node.  Single-context grids only (FsError on a slab); not allowed during a graph capture."""
        from .lcs import check_lattice
        RideOps._host_only(self, "flowmap_create during a graph capture")
        RideOps._single_context(self, "flow maps need", "the particles would have to migrate between ranks")
        box, refine, _ = check_lattice(box, refine, 1, (self.nx, self.ny))
        h = self._p_flowmap_create(box, refine)
        return self._adopt(h, FlowMap(h, box, refine))

    def flowmap_advance(self, fm, pod, slot_from, slot_to, h, substeps=1):
        """Every alive node across one interval of the ring, from slot_from to slot_to, in `substeps` midpoint steps of signed size h (cell
        units) in the velocity interpolated linearly in time between the two slots.  One launch; reads the ring, writes the lattice."""
        self._host_only("flowmap_advance during a graph capture")
        slot_from, slot_to, substeps, h = int(slot_from), int(slot_to), int(substeps), float(h)
        if not (0 <= slot_from < pod.slots and 0 <= slot_to < pod.slots) or slot_from == slot_to:
            raise ValueError(f"slots must be two different ones of 0 .. {pod.slots - 1}, got {slot_from} and {slot_to}")
        if not 1 <= substeps <= 16:
            raise ValueError(f"substeps must be 1 .. 16, got {substeps}")
        if not np.isfinite(h) or h == 0.0:
            raise ValueError(f"h must be finite and not 0, got {h}")
        self._p_flowmap_advance(fm._h, pod._h, slot_from, slot_to, h, substeps)

    def flowmap_cauchy_green(self, fm):
        """lam of every node: the largest eigenvalue of the Cauchy-Green tensor of the map, from the positions of the lattice neighbours."""
        self._host_only("flowmap_cauchy_green during a graph capture")
        self._p_flowmap_cauchy_green(fm._h)

    def flowmap_get(self, fm):
        """-> (x, y float64 (nx, ny); status int32 (nx, ny): 0 alive, 1 LEFT, 2 WALL, 4 UNSEEDED; lam float64 (nx, ny))."""
        self._host_only("flowmap_get during a graph capture")
        return self._p_flowmap_get(fm._h, fm.shape)

    def flowmap_reset(self, fm):
        """Seed again: the state after flowmap_create."""
        self._host_only("flowmap_reset during a graph capture")
        self._p_flowmap_reset(fm._h)

    def flowmap_free(self, fm):
        self._host_only("flowmap_free during a graph capture")
        self._release(fm, self._p_flowmap_free)

    # ---- tracer particles (include/fs_hip.h fs_tracer_*): N particles in double cell coordinates, advanced by one launch per step -------
    def tracer_create(self, seeds, respawn=True, max_age=0):
        """A device tracer set for FluidSimulator.seed_tracers: seeds float64 (N, 2) in cell units, N >= 1, inside the domain (whether
        the cells are fluid is fs.tracers.check_seeds' business).  52 bytes per particle (+ 36 and 4 per sort bin once tracer_sort has
        run).  Single-context grids only (FsError on a slab); not allowed during a graph capture."""
        RideOps._tracer_host_call(self, "tracer_create")
        seeds = np.ascontiguousarray(seeds, np.float64)
        if seeds.ndim != 2 or seeds.shape[1] != 2 or len(seeds) < 1:
            raise ValueError(f"seeds must have shape (N, 2) with N >= 1, got {seeds.shape}")
        max_age = int(max_age)
        if max_age < 0:
            raise ValueError("max_age must be >= 0")
        h = self._p_tracer_create(seeds, bool(respawn), max_age)
        return self._adopt(h, TracerSet(h, len(seeds), bool(respawn), max_age))

    def tracer_advance(self, tr, h, v):
        """One midpoint step h = dt / dx of every alive particle in the velocity field v; the launch counter advances on the device.  A
        limit_field v still owes stays deferred: the kernel limits the corner values as the pass would store them.  Not a _run: no flush,
        no exchange (writes no field)."""
        self._ride("tracer_advance", (tr._h, float(h), self._limit_of(v), v._h))

    def tracer_read(self, tr, raw=False):
        """-> {"x", "y": float64 (N,), "age", "status", "respawns": int32 (N,), "seeds": float64 (N, 2), "steps": launches so far}: one
        download, in SEED order (entry k belongs to seed k) whatever tracer_sort has done on the device.  raw=True: x, y, age, status
        and respawns in the device's SLOT order instead, plus "id": int32 (N,), the seed index of the particle in each slot (the seeds
        stay in seed order: the seed of slot k is seeds[id[k]]).  Not allowed during a graph capture."""
        self._host_only("tracer_read during a graph capture: the state is a download (read between captures / replays)")
        pos, ints, launches = self._p_tracer_read(tr._h, tr.n)
        out = {"x": pos[0].copy(), "y": pos[1].copy(), "age": ints[0].copy(), "status": ints[1].copy(), "respawns": ints[2].copy(),
               "seeds": np.ascontiguousarray(pos[2:4].T), "steps": int(launches)}
        if raw:
            ids = self._p_tracer_order(tr._h, tr.n)
            for k in ("x", "y", "age", "status", "respawns"):
                out[k] = out[k][ids]
            out["id"] = ids
        return out

    def tracer_read_steps(self, tr):
        """Launches of the advance so far (the "steps" of tracer_read) without the particle download."""
        self._host_only("tracer_read during a graph capture: the state is a download (read between captures / replays)")
        return int(self._p_tracer_read(tr._h, 0)[2])

    def tracer_sort(self, tr):
        """Reorder the particle slots on the device by cell (fs.tracers.sort_key: rows of bins SORT_BIN_CELLS cells wide; dead and
        outside particles last) so that the advance gathers from neighbouring cache lines.  Changes nothing tracer_read() or any other
        call shows, and no device address: graphs that hold the advance stay valid.  A handful of launches outside any graph (profiled
        as tracer_sort_*); not allowed during a graph capture."""
        RideOps._tracer_host_call(self, "tracer_sort")
        self._p_tracer_sort(tr._h)

    def tracer_order(self, tr):
        """-> int32 (N,): the seed index of the particle in each device slot (arange(N) until the first tracer_sort)."""
        RideOps._tracer_host_call(self, "tracer_order")
        return self._p_tracer_order(tr._h, tr.n)

    def tracer_fields(self, tr):
        """-> (count int32 (X, Y), age_sum int64 (X, Y)): per cell, the number of alive particles inside it and the sum of their ages.
        One launch with integer atomics (exact, repeatable) + the download; 12 bytes per cell of device memory during the call."""
        RideOps._tracer_host_call(self, "tracer_fields")
        return self._p_tracer_fields(tr._h)

    def tracer_write(self, tr, state):
        """Restore what tracer_read returned (checkpoints): the same keys, arrays of the set's N."""
        self._host_only("tracer_write during a graph capture")
        n = tr.n
        seeds = np.asarray(state["seeds"], np.float64)
        if seeds.shape != (n, 2):
            raise ValueError(f"expected seeds of shape {(n, 2)}, got {seeds.shape}")
        pos = np.empty((4, n), np.float64)
        ints = np.empty((3, n), np.int32)
        for row, key in ((0, "x"), (1, "y")):
            a = np.asarray(state[key], np.float64)
            if a.shape != (n,):
                raise ValueError(f"expected {key} of shape {(n,)}, got {a.shape}")
            pos[row] = a
        pos[2], pos[3] = seeds[:, 0], seeds[:, 1]
        for row, key in enumerate(("age", "status", "respawns")):
            a = np.asarray(state[key])
            if a.shape != (n,):
                raise ValueError(f"expected {key} of shape {(n,)}, got {a.shape}")
            ints[row] = a
        if (ints[0] < 0).any() or (ints[2] < 0).any() or (ints[1] < 0).any() or (ints[1] > 3).any() or int(state["steps"]) < 0:
            raise ValueError("tracer state: age, respawns and steps must be >= 0 and status in 0 .. 3")
        self._p_tracer_write(tr._h, pos, ints, int(state["steps"]))

    def tracer_draw(self, tr, rgb, color=(1.0, 1.0, 1.0)):
        """Store `color` into pixel (floor x, floor y) of the 3-channel field rgb for every alive particle."""
        r, g, b = (float(c) for c in color)
        self._p_kernel("tracer_draw", tr._h, r, g, b, rgb._h)

    # ---- inertial tracer sets, deposits, accumulated occupancy (include/fs_hip.h fs_tracer_create_inertial ... fs_tracer_accum_*) ---------
    def tracer_create_inertial(self, seeds, alpha, tau, gravity=(0.0, 0.0), respawn=True, max_age=0, deposits=False):
        """A device set of inertial particles for FluidSimulator.seed_tracers(tau=...): as tracer_create, plus alpha (N,) in (0, 1] (the
        response of one step, fs.tracers.response(tau, dt)), tau (N,) finite and >= 0 in the solver's time units, gravity (gx, gy) in
        velocity per time; deposits: the set owns an int32 plane that counts the wall hits per wall cell.  84 bytes per particle (+ 68 and
        4 per sort bin once tracer_sort has run) and 4 per cell with deposits."""
        RideOps._tracer_host_call(self, "tracer_create_inertial")
        seeds = np.ascontiguousarray(seeds, np.float64)
        if seeds.ndim != 2 or seeds.shape[1] != 2 or len(seeds) < 1:
            raise ValueError(f"seeds must have shape (N, 2) with N >= 1, got {seeds.shape}")
        n = len(seeds)
        alpha, tau = np.ascontiguousarray(alpha, np.float64), np.ascontiguousarray(tau, np.float64)
        if alpha.shape != (n,) or tau.shape != (n,):
            raise ValueError(f"alpha and tau must have shape {(n,)}, got {alpha.shape} and {tau.shape}")
        if not ((alpha > 0.0) & (alpha <= 1.0)).all():
            raise ValueError("alpha must lie in (0, 1]")
        if not (np.isfinite(tau) & (tau >= 0.0)).all():
            raise ValueError("tau must be finite and >= 0")
        gravity = tuple(float(g) for g in gravity)
        if len(gravity) != 2 or not all(np.isfinite(g) for g in gravity):
            raise ValueError("gravity must be two finite numbers (gx, gy)")
        max_age = int(max_age)
        if max_age < 0:
            raise ValueError("max_age must be >= 0")
        h = self._p_tracer_create_inertial(seeds, alpha, tau, gravity, bool(respawn), max_age, bool(deposits))
        tr = TracerSet(h, n, bool(respawn), max_age)
        tr.inertial, tr.deposits, tr.gravity, tr.tau, tr.alpha = True, bool(deposits), gravity, tau.copy(), alpha.copy()
        return self._adopt(h, tr)

    def tracer_read_vel(self, tr):
        """-> (pu, pw) float64 (N,): the particle velocities of an inertial set in SEED order (one download)."""
        RideOps._tracer_host_call(self, "tracer_read_vel")
        if not getattr(tr, "inertial", False):
            raise ValueError("not an inertial tracer set")
        vel = self._p_tracer_read_vel(tr._h, tr.n)
        return vel[0].copy(), vel[1].copy()

    def tracer_write_vel(self, tr, pu, pw):
        """Restore what tracer_read_vel returned (checkpoints; after tracer_write)."""
        RideOps._tracer_host_call(self, "tracer_write_vel")
        if not getattr(tr, "inertial", False):
            raise ValueError("not an inertial tracer set")
        vel = np.empty((2, tr.n), np.float64)
        for row, (key, a) in enumerate((("u", pu), ("w", pw))):
            a = np.asarray(a, np.float64)
            if a.shape != (tr.n,):
                raise ValueError(f"expected {key} of shape {(tr.n,)}, got {a.shape}")
            vel[row] = a
        self._p_tracer_write_vel(tr._h, vel)

    def tracer_deposits(self, tr):
        """-> int32 (X, Y): wall hits per wall cell since creation (a set created with deposits=True)."""
        RideOps._tracer_host_call(self, "tracer_deposits")
        if not getattr(tr, "deposits", False):
            raise ValueError("the tracer set records no deposits (deposits=True)")
        return self._p_tracer_deposits(tr._h)

    def tracer_deposits_write(self, tr, plane):
        """Restore what tracer_deposits returned (checkpoints)."""
        RideOps._tracer_host_call(self, "tracer_deposits_write")
        if not getattr(tr, "deposits", False):
            raise ValueError("the tracer set records no deposits (deposits=True)")
        plane = np.asarray(plane)
        if plane.shape != (self.nx, self.ny) or (plane < 0).any():
            raise ValueError(f"expected deposits >= 0 of shape {(self.nx, self.ny)}, got {plane.shape}")
        self._p_tracer_deposits_write(tr._h, plane.astype(np.int32))

    def tracer_accum_create(self, tr, every=1, start=0):
        """Attach the accumulated-occupancy planes to a set (passive or inertial): 16 bytes per cell, zeroed.  With n advances since this
        call before a step's, tracer_accum_add samples behind that step's advance when n + 1 > start and (n + 1 - start) % every == 0.
        -> TracerAccum (one per set)."""
        RideOps._tracer_host_call(self, "tracer_accum_create")
        every, start = RideOps._check_cadence(every, start)
        if getattr(tr, "accum", None) is not None:
            raise RuntimeError("the tracer set has an accumulator already")
        self._p_tracer_accum("create", tr._h, every, start)
        tr.accum = TracerAccum(tr, every, start)
        return tr.accum

    def tracer_accum_add(self, tr):
        """The accumulation launch behind tracer_advance (gated on the device; part of captured steps).  Not a _run: writes no field."""
        self._ride("tracer_accum_add", (tr._h,))

    def tracer_accum_read(self, tr):
        """-> (occupancy int64 (X, Y), age_sum int64 (X, Y), launches, samples)."""
        RideOps._tracer_host_call(self, "tracer_accum_read")
        return self._p_tracer_accum_read(tr._h)

    def tracer_accum_write(self, tr, occupancy, age_sum, launches, samples):
        """Restore what tracer_accum_read returned (checkpoints; after tracer_write, which sets the launch count the phase hangs on)."""
        RideOps._tracer_host_call(self, "tracer_accum_write")
        occupancy, age_sum = np.asarray(occupancy), np.asarray(age_sum)
        for name, a in (("occupancy", occupancy), ("age_sum", age_sum)):
            if a.shape != (self.nx, self.ny) or (a < 0).any():
                raise ValueError(f"expected {name} >= 0 of shape {(self.nx, self.ny)}, got {a.shape}")
        launches, samples = RideOps._check_counters(launches, samples)
        self._p_tracer_accum_write(tr._h, occupancy.astype(np.int64), age_sum.astype(np.int64), launches, samples)

    def tracer_accum_reset(self, tr):
        """Planes and sample count to zero; the phase of every / start runs on."""
        RideOps._tracer_host_call(self, "tracer_accum_reset")
        self._p_tracer_accum("reset", tr._h)

    def tracer_accum_free(self, tr):
        """Detach the accumulator (inside a capture the device memory is released when the capture ends)."""
        if getattr(tr, "accum", None) is not None and tr._h is not None:
            self._p_tracer_accum("free", tr._h)
        tr.accum = None

    def tracer_free(self, tr):
        if tr._h is not None:
            self._release(tr, self._p_tracer_free)       # (the library releases an attached accumulator with the set)
            tr.accum = None


class _DistSpec(ctypes.Structure):
    """fs_dist_spec of include/fs_hip.h."""
    _fields_ = [("quantity", ctypes.c_int), ("bins", ctypes.c_int), ("quantity_b", ctypes.c_int), ("bins_b", ctypes.c_int), ("box", ctypes.c_int * 4),
                ("lo", ctypes.c_double), ("hi", ctypes.c_double), ("lo_b", ctypes.c_double), ("hi_b", ctypes.c_double)]


def _freer(symbol):
    """A `_p_*_free`: the library's free of a handle, unless the context is gone already."""
    def free(self, h):
        if self._ctx is not None:
            _lib.call(symbol, self._ctx, h)
    return free


def _caller(symbol):
    """A primitive that hands the context, the handle and its arguments to the library and returns nothing."""
    def call(self, h, *args):
        _lib.call(symbol, self._ctx, h, *args)
    return call


def _counted_reader(symbol, optional=False):
    """A `_p_*_read` / `_p_*_get` -> (payload float64 (words,), launches, samples); optional: words == 0 asks for the counters alone."""
    def read(self, h, words):
        out = np.empty(words, np.float64)
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call(symbol, self._ctx, h, None if optional and not words else out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                  ctypes.byref(launches), ctypes.byref(samples))
        return out, launches.value, samples.value
    return read


class NativeRideOps:
    """The primitives of RideOps on libfs_hip.so (self._ctx: the library's context).  Those that differ only in the symbol they call come
    from _freer, _caller and _counted_reader."""

    def _p_flow_stats(self, dx, vh, ph, box):
        out = (ctypes.c_double * len(self.STAT_SLOTS))()
        b = None if box is None else (ctypes.c_int * 4)(*box)
        _lib.call("fs_flow_stats", self._ctx, dx, vh, ph, b, out)
        return list(out)

    def _p_history_create(self, points, faces, capacity, every):
        h = ctypes.c_void_p()
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if a.size else None
        _lib.call("fs_history_create", self._ctx, len(points), ip(points), len(faces), ip(faces), capacity, every, ctypes.byref(h))
        return h

    def _p_history_read(self, h, nlocal, capacity):
        out = np.empty((capacity, 2 + 3 * nlocal), np.float64)
        n, launches, dropped = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
        _lib.call("fs_history_read", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), capacity, ctypes.byref(n),
                  ctypes.byref(launches), ctypes.byref(dropped))
        return out[:n.value], launches.value, dropped.value

    _p_history_free = _freer("fs_history_free")

    def _p_loads_create(self, faces, centre, capacity, every, start):
        h = ctypes.c_void_p()
        c = (ctypes.c_double * 2)(float(centre[0]), float(centre[1]))
        _lib.call("fs_loads_create", self._ctx, len(faces), faces.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if faces.size else None, c,
                  capacity, every, start, ctypes.byref(h))
        return h

    def _p_loads_read(self, h, capacity):
        out = np.empty((capacity, self.LOADS_REC), np.float64)
        n, launches, samples, dropped = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        _lib.call("fs_loads_read", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), capacity, ctypes.byref(n),
                  ctypes.byref(launches), ctypes.byref(samples), ctypes.byref(dropped))
        return out[:n.value], launches.value, samples.value, dropped.value

    def _p_loads_sums_read(self, h, nlocal):
        out = np.empty((self.LOADS_SUMS, nlocal), np.float64)
        _lib.call("fs_loads_sums_read", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return out

    def _p_loads_sums_write(self, h, sums, launches, samples):
        a = np.ascontiguousarray(sums, np.float64)
        _lib.call("fs_loads_sums_write", self._ctx, h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_loads_reset = _caller("fs_loads_reset")
    _p_loads_free = _freer("fs_loads_free")

    def _p_mean_create(self, every, start):
        h = ctypes.c_void_p()
        _lib.call("fs_mean_create", self._ctx, every, start, ctypes.byref(h))
        return h

    def _p_mean_read(self, h):
        out = np.empty((self.MEAN_PLANES, self.nyl, self.nx), np.float64)       # (the library's layout: x contiguous)
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("fs_mean_read", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(launches), ctypes.byref(samples))
        return out.transpose(0, 2, 1), launches.value, samples.value

    def _p_mean_write(self, h, sums, launches, samples):
        a = np.ascontiguousarray(sums.transpose(0, 2, 1), np.float64)
        _lib.call("fs_mean_write", self._ctx, h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_mean_reset = _caller("fs_mean_reset")
    _p_mean_finalize = _caller("fs_mean_finalize")      # (h, vh, ph)
    _p_mean_free = _freer("fs_mean_free")

    def _p_modes_create(self, cos_sin, every, start):
        h = ctypes.c_void_p()
        _lib.call("fs_modes_create", self._ctx, len(cos_sin), cos_sin.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), every, start, ctypes.byref(h))
        return h

    def _p_modes_read(self, h, nfreq, with_sums=True):
        out = np.empty((self.modes_planes(nfreq) if with_sums else 0, self.nyl, self.nx), np.float64)       # (the library's layout: x contiguous)
        scalars = np.empty(self.modes_scalars(nfreq), np.float64)
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_modes_read", self._ctx, h, dp(out) if with_sums else None, dp(scalars), ctypes.byref(launches), ctypes.byref(samples))
        return (out.transpose(0, 2, 1) if with_sums else None), scalars, launches.value, samples.value

    def _p_modes_write(self, h, sums, scalars, launches, samples):
        a = np.ascontiguousarray(sums.transpose(0, 2, 1), np.float64)
        dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_modes_write", self._ctx, h, dp(a), dp(scalars), launches, samples)

    _p_modes_reset = _caller("fs_modes_reset")

    def _p_modes_combine(self, h, weights, vh, ph):
        _lib.call("fs_modes_combine", self._ctx, h, weights.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), vh, ph)

    def _p_modes_rows(self, nfreq):
        a, c = ctypes.c_int(), ctypes.c_int()
        _lib.call("fs_modes_rows", self._ctx, nfreq, ctypes.byref(a), ctypes.byref(c))
        return a.value, c.value

    _p_modes_free = _freer("fs_modes_free")

    def _p_pod_create(self, slots, every, start):
        h = ctypes.c_void_p()
        _lib.call("fs_pod_create", self._ctx, slots, every, start, ctypes.byref(h))
        return h

    def _p_pod_read(self, h):
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("fs_pod_read", self._ctx, h, ctypes.byref(launches), ctypes.byref(samples))
        return launches.value, samples.value

    def _p_pod_gram(self, h, slots):
        out = np.empty((slots, slots), np.float64)
        n, launches, samples = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("fs_pod_gram", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), slots, ctypes.byref(n), ctypes.byref(launches),
                  ctypes.byref(samples))
        return out.ravel()[:n.value * n.value].reshape(n.value, n.value).copy(), launches.value, samples.value

    def _p_pod_combine(self, h, weights, vh, ph):
        _lib.call("fs_pod_combine", self._ctx, h, weights.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), vh, ph)

    def _p_pod_get(self, h, slots):
        out = np.empty((slots, 3, self.nyl, self.nx), self.dtype)       # (the library's layout: x contiguous)
        _lib.call("fs_pod_get", self._ctx, h, out.ctypes.data_as(ctypes.c_void_p))
        return np.ascontiguousarray(out.transpose(0, 1, 3, 2))

    def _p_pod_set(self, h, slots, launches, samples):
        a = np.ascontiguousarray(slots.transpose(0, 1, 3, 2), self.dtype)
        _lib.call("fs_pod_set", self._ctx, h, a.ctypes.data_as(ctypes.c_void_p), launches, samples)

    _p_pod_reset = _caller("fs_pod_reset")
    _p_pod_free = _freer("fs_pod_free")

    def _p_vortex_create(self, which, threshold, exponent, every, start, min_area, max_vortices, max_components, capacity):
        h = ctypes.c_void_p()
        _lib.call("fs_vortex_create", self._ctx, which, threshold, float(np.ldexp(1.0, 30 - exponent)), every, start, min_area, max_vortices,
                  max_components, capacity, ctypes.byref(h))
        return h

    def _p_vortex_read(self, h, capacity, words):
        out = np.empty((capacity, words), np.int64)
        n, launches, lost = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("fs_vortex_read", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), capacity, ctypes.byref(n),
                  ctypes.byref(launches), ctypes.byref(lost))
        return out[:n.value].copy(), launches.value, lost.value

    def _p_vortex_get_labels(self, h):
        flags, labels = np.empty((self.ny, self.nx), np.uint8), np.empty((self.ny, self.nx), np.int32)      # (the library's layout: x contiguous)
        _lib.call("fs_vortex_get_labels", self._ctx, h, flags.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return np.ascontiguousarray(flags.T), np.ascontiguousarray(labels.T)

    _p_vortex_set = _caller("fs_vortex_set")      # (h, launches)

    def _p_vortex_label(self, flags):
        f = np.ascontiguousarray(flags.T)
        labels = np.empty((self.ny, self.nx), np.int32)
        _lib.call("fs_vortex_label", self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return np.ascontiguousarray(labels.T)

    def _p_vortex_criterion(self, which, limit, dx, vh):
        out = np.empty((self.ny, self.nx), np.float64)
        _lib.call("fs_vortex_criterion", self._ctx, which, limit, dx, vh, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return np.ascontiguousarray(out.T)

    _p_vortex_free = _freer("fs_vortex_free")

    def _p_dist_create(self, chans, every, start):
        h = ctypes.c_void_p()
        specs = (_DistSpec * len(chans))()
        for s, c in zip(specs, chans):
            s.quantity, s.bins, s.quantity_b, s.bins_b = c.quantity, c.bins, c.quantity_b, c.bins_b
            s.box[:] = c.box
            s.lo, s.hi, s.lo_b, s.hi_b = c.lo, c.hi, c.lo_b, c.hi_b
        _lib.call("fs_dist_create", self._ctx, len(chans), ctypes.cast(specs, ctypes.c_void_p), every, start, ctypes.byref(h))
        return h

    def _p_dist_read(self, h, chan, bins):
        counts, tails = np.zeros(bins, np.int64), np.zeros(self.DIST_NTAIL, np.int64)
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        lp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        _lib.call("fs_dist_read", self._ctx, h, chan, lp(counts) if bins else None, lp(tails) if bins else None, ctypes.byref(launches),
                  ctypes.byref(samples))
        return counts, tails, launches.value, samples.value

    def _p_dist_get(self, h, words):
        out = np.empty(words, np.int64)
        _lib.call("fs_dist_get", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return out

    def _p_dist_set(self, h, words, launches, samples):
        _lib.call("fs_dist_set", self._ctx, h, words.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), launches, samples)

    _p_dist_reset = _caller("fs_dist_reset")
    _p_dist_free = _freer("fs_dist_free")

    def _p_dist_select(self, q, box, limit, dx, vh, ph, ranks):
        r = (ctypes.c_longlong * max(1, len(ranks)))(*ranks)
        out = np.empty(len(ranks), np.float64)
        n, nan = ctypes.c_longlong(-1), ctypes.c_longlong(0)
        try:
            _lib.call("fs_dist_select", self._ctx, q, (ctypes.c_int * 4)(*box), limit, dx, vh, ph, r, len(ranks),
                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(n), ctypes.byref(nan))
        except _lib.FsError:
            if ranks and 0 <= n.value <= ranks[-1]:      # (the library wrote n before it looked at the ranks)
                raise ValueError(f"rank {ranks[-1]} >= n = {n.value}, the number of selected cells whose value is not NaN") from None
            raise
        return out, n.value, nan.value

    def _p_spec_create(self, box, wx, wy, twx, twy, c1x, c1y, detrend, every, start):
        h = ctypes.c_void_p()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_spec_create", self._ctx, (ctypes.c_int * 4)(*box), dp(wx), dp(wy), dp(twx), dp(twy), c1x, c1y, int(detrend), every, start,
                  ctypes.byref(h))
        return h

    _p_spec_read = _counted_reader("fs_spec_read", optional=True)      # (h, cells)

    def _p_spec_plane(self, h, cells):
        out = np.empty(2 * cells, np.float64)
        _lib.call("fs_spec_plane", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return out

    _p_spec_get = _counted_reader("fs_spec_get")

    def _p_spec_set(self, h, power, launches, samples):
        _lib.call("fs_spec_set", self._ctx, h, power.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_spec_reset = _caller("fs_spec_reset")
    _p_spec_free = _freer("fs_spec_free")

    def _p_xspec_create(self, box, qa, qb, dx, wx, wy, twx, twy, c1x, c1y, detrend, every, start):
        h = ctypes.c_void_p()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_xspec_create", self._ctx, (ctypes.c_int * 4)(*box), qa, qb, dx, dp(wx), dp(wy), dp(twx), dp(twy), c1x, c1y, int(detrend),
                  every, start, ctypes.byref(h))
        return h

    _p_xspec_read = _counted_reader("fs_xspec_read", optional=True)      # (h, words)

    def _p_xspec_plane(self, h, cells):
        out = np.empty(2 * cells, np.float64)
        _lib.call("fs_xspec_plane", self._ctx, h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return out

    _p_xspec_get = _counted_reader("fs_xspec_get")

    def _p_xspec_set(self, h, sums, launches, samples):
        _lib.call("fs_xspec_set", self._ctx, h, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_xspec_reset = _caller("fs_xspec_reset")
    _p_xspec_free = _freer("fs_xspec_free")

    def _p_flux_create(self, box, half_widths, dx, every, start):
        h = ctypes.c_void_p()
        _lib.call("fs_flux_create", self._ctx, (ctypes.c_int * 4)(*box), len(half_widths), (ctypes.c_int * len(half_widths))(*half_widths), dx, every,
                  start, ctypes.byref(h))
        return h

    _p_flux_read = _counted_reader("fs_flux_read", optional=True)      # (h, words)

    def _p_flux_filtered(self, h, index, words):
        out = np.empty(words, np.float64)
        _lib.call("fs_flux_filtered", self._ctx, h, index, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return out

    _p_flux_get = _counted_reader("fs_flux_get")

    def _p_flux_set(self, h, flat, launches, samples):
        _lib.call("fs_flux_set", self._ctx, h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_flux_reset = _caller("fs_flux_reset")
    _p_flux_free = _freer("fs_flux_free")

    def _p_budget_create(self, box, dx, every, start):
        h = ctypes.c_void_p()
        _lib.call("fs_budget_create", self._ctx, *box, dx, every, start, ctypes.byref(h))
        return h

    _p_budget_read = _counted_reader("fs_budget_read", optional=True)      # (h, words)
    _p_budget_get = _counted_reader("fs_budget_get")

    def _p_budget_set(self, h, flat, launches, samples):
        _lib.call("fs_budget_set", self._ctx, h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), launches, samples)

    _p_budget_reset = _caller("fs_budget_reset")
    _p_budget_free = _freer("fs_budget_free")

    def _p_flowmap_create(self, box, refine):
        h = ctypes.c_void_p()
        _lib.call("fs_flowmap_create", self._ctx, (ctypes.c_int * 4)(*box), refine, ctypes.byref(h))
        return h

    _p_flowmap_advance = _caller("fs_flowmap_advance")      # (h, pod_h, slot_from, slot_to, step, substeps)
    _p_flowmap_cauchy_green = _caller("fs_flowmap_cauchy_green")

    def _p_flowmap_get(self, h, shape):
        nx, ny = shape
        x, y, lam = (np.empty((ny, nx), np.float64) for _ in range(3))       # (the library's layout: a contiguous)
        status = np.empty((ny, nx), np.int32)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_flowmap_get", self._ctx, h, dp(x), dp(y), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), dp(lam))
        return tuple(np.ascontiguousarray(a.T) for a in (x, y, status, lam))

    _p_flowmap_reset = _caller("fs_flowmap_reset")
    _p_flowmap_free = _freer("fs_flowmap_free")

    def _p_tracer_create(self, seeds, respawn, max_age):
        h = ctypes.c_void_p()
        _lib.call("fs_tracer_create", self._ctx, len(seeds), seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(respawn), max_age,
                  ctypes.byref(h))
        return h

    def _p_tracer_read(self, h, n):
        launches = ctypes.c_longlong()
        if n == 0:      # the launch counter alone
            _lib.call("fs_tracer_read", self._ctx, h, None, None, ctypes.byref(launches))
            return None, None, launches.value
        pos, ints = np.empty((4, n), np.float64), np.empty((3, n), np.int32)
        _lib.call("fs_tracer_read", self._ctx, h, pos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                  ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(launches))
        return pos, ints, launches.value

    def _p_tracer_write(self, h, pos, ints, launches):
        _lib.call("fs_tracer_write", self._ctx, h, pos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                  ints.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), launches)

    _p_tracer_sort = _caller("fs_tracer_sort")

    def _p_tracer_order(self, h, n):
        ids = np.empty(n, np.int32)
        _lib.call("fs_tracer_order", self._ctx, h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return ids

    def _p_tracer_fields(self, h):
        count, age = np.empty((self.ny, self.nx), np.int32), np.empty((self.ny, self.nx), np.int64)       # (the library's layout: x contiguous)
        _lib.call("fs_tracer_fields", self._ctx, h, count.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                  age.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return np.ascontiguousarray(count.T), np.ascontiguousarray(age.T)

    _p_tracer_free = _freer("fs_tracer_free")

    def _p_tracer_create_inertial(self, seeds, alpha, tau, gravity, respawn, max_age, deposits):
        h = ctypes.c_void_p()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        _lib.call("fs_tracer_create_inertial", self._ctx, len(seeds), dp(seeds), dp(alpha), dp(tau), gravity[0], gravity[1], int(respawn), max_age,
                  int(deposits), ctypes.byref(h))
        return h

    def _p_tracer_read_vel(self, h, n):
        vel = np.empty((2, n), np.float64)
        _lib.call("fs_tracer_read_vel", self._ctx, h, vel.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return vel

    def _p_tracer_write_vel(self, h, vel):
        _lib.call("fs_tracer_write_vel", self._ctx, h, vel.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))

    def _p_tracer_deposits(self, h):
        plane = np.empty((self.ny, self.nx), np.int32)       # (the library's layout: x contiguous)
        _lib.call("fs_tracer_deposits", self._ctx, h, plane.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return np.ascontiguousarray(plane.T)

    def _p_tracer_deposits_write(self, h, plane):
        a = np.ascontiguousarray(plane.T, np.int32)
        _lib.call("fs_tracer_deposits_write", self._ctx, h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def _p_tracer_accum(self, what, h, *args):
        if self._ctx is not None:
            _lib.call("fs_tracer_accum_" + what, self._ctx, h, *args)

    def _p_tracer_accum_read(self, h):
        occ, age = np.empty((self.ny, self.nx), np.int64), np.empty((self.ny, self.nx), np.int64)
        launches, samples = ctypes.c_longlong(), ctypes.c_longlong()
        lp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        _lib.call("fs_tracer_accum_read", self._ctx, h, lp(occ), lp(age), ctypes.byref(launches), ctypes.byref(samples))
        return np.ascontiguousarray(occ.T), np.ascontiguousarray(age.T), launches.value, samples.value

    def _p_tracer_accum_write(self, h, occupancy, age_sum, launches, samples):
        occ, age = np.ascontiguousarray(occupancy.T, np.int64), np.ascontiguousarray(age_sum.T, np.int64)
        lp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        _lib.call("fs_tracer_accum_write", self._ctx, h, lp(occ), lp(age), launches, samples)
