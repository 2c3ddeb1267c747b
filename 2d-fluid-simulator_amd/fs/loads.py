"""Host side of the body surface loads (new; the reference has none): the geometry of a body's faces, the tracker that drains the device
ring, and the coefficients users quote (Cd, Cl, Cm, Cp, Cf).

The sampling itself is a device launch sequence per step (csrc/fs_loads.h, include/fs_hip.h fs_loads_*), driven by
FluidSimulator.track_body / body_loads / body_surface / stop_body."""
import numpy as np

from .history import DIRS, WALL
from .riders import Rider, ring_room, samples_after

RECORD = ("pressure_x", "pressure_y", "viscous_x", "viscous_y", "moment_pressure", "moment_viscous")      # a device record, in order
SUMS = ("p", "pp", "tau", "tautau")                                                                         # the per-face planes, in order
# face midpoint relative to the fluid cell's corner (x, y), per direction wall -> fluid
MIDPOINT = ((0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0))


def face_geometry(faces, centre):
    """faces (F, 3) of fs.history.body_faces, centre (cx, cy) in cell units -> {"x", "y": face midpoints in cell units, "nx", "ny": the
    outward normal (wall -> fluid, fs.history.DIRS), "theta": atan2(ym - cy, xm - cx)}, float64 (F,)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cx, cy = (float(c) for c in centre)
    mid = np.asarray(MIDPOINT, np.float64)[faces[:, 2]]
    nrm = np.asarray(DIRS, np.float64)[faces[:, 2]]
    x, y = faces[:, 0] + mid[:, 0], faces[:, 1] + mid[:, 1]
    return {"x": x, "y": y, "nx": nrm[:, 0].copy(), "ny": nrm[:, 1].copy(), "theta": np.arctan2(y - cy, x - cx)}


def body_centroid(mask, box):
    """Mean of the cell centres (i + 0.5, j + 0.5) of the wall cells inside box = (x0, y0, x1, y1) (half-open): the default centre of the
    moments.  ValueError when the box holds no wall cell."""
    mask = np.asarray(mask)
    x0, y0, x1, y1 = (int(b) for b in box)
    i, j = np.nonzero(mask[x0:x1, y0:y1] == WALL)
    if len(i) == 0:
        raise ValueError(f"body box {tuple(box)} holds no wall cell")
    return float(np.mean(i + x0 + 0.5)), float(np.mean(j + y0 + 0.5))


def coefficients(force, u_ref, length):
    """2 F / (U^2 L): drag / lift coefficient of a force per unit depth (density 1); for a moment pass length = L^2."""
    return 2.0 * np.asarray(force, np.float64) / (float(u_ref) ** 2 * float(length))


def pressure_coefficient(p, u_ref, p_ref=0.0):
    """Cp = (p - p_ref) / (0.5 U^2)."""
    return (np.asarray(p, np.float64) - float(p_ref)) / (0.5 * float(u_ref) ** 2)


def skin_friction(tau, u_ref):
    """Cf = tau / (0.5 U^2)."""
    return np.asarray(tau, np.float64) / (0.5 * float(u_ref) ** 2)


def surface_statistics(sums, samples):
    """The (4, F) sums S_p, S_pp, S_t, S_tt and the sample count -> p_mean, p_rms, tau_mean, tau_rms (F,): the rms is the root of the
    central second moment S_aa / n - mean^2, clipped at 0."""
    sums = np.asarray(sums, np.float64)
    if samples < 1:
        nan = np.full(sums.shape[1], np.nan)
        return nan, nan.copy(), nan.copy(), nan.copy()
    pm, tm = sums[0] / samples, sums[2] / samples
    return pm, np.sqrt(np.maximum(sums[1] / samples - pm * pm, 0.0)), tm, np.sqrt(np.maximum(sums[3] / samples - tm * tm, 0.0))


class Tracker(Rider):
    """One body tracker of a FluidSimulator (track_body): the device object, the records drained from its ring so far, and how many
    launches have been issued - from which the simulator knows how many steps it may run before the ring is full (room)."""
    stop_in_capture, keeps_last = False, True

    def __init__(self, dev, loads, faces, box, centre, every, start_step, dt):
        self.dev, self.loads, self.faces, self.box, self.centre = dev, loads, np.asarray(faces, np.int32).reshape(-1, 3), box, centre
        self.every, self.start_step, self.dt = int(every), int(start_step), float(dt)
        self.issued = 0          # launches issued (captured launches count when their capture runs once)
        self.base = 0            # launches a resumed tracker starts from (its samples before are not in this ring)
        self.drained = 0         # records read back
        self.samples = 0         # samples in the per-face sums at the last drain
        self._records = []
        self._final = None       # (sums, samples) kept by close()

    @property
    def token(self):
        return ("loads", self.loads.serial)

    def _sampled(self, launches):
        """Samples among the first `launches` launches."""
        return samples_after(launches, self.every, self.start_step)

    def room(self):
        """Steps that may run before the next sampling one would find the ring full."""
        return ring_room(self.issued, self.every, self.start_step, self.loads.capacity, self._sampled(self.base) + self.drained)

    def launch(self, sim):
        self._make_room()
        s = sim._solver
        v, p = s.get_fields()[:2]
        self.dev.loads_record(self.loads, s.dx, 1.0 / s.re, v, p)
        self.issued += 1

    def free(self):
        self.dev.loads_free(self.loads)

    def drain(self):
        rec, launches, samples, dropped = self.dev.loads_read(self.loads)
        self.issued, self.samples = launches, samples
        if len(rec):
            self._records.append(rec)
            self.drained += len(rec)
        if dropped:
            raise RuntimeError(f"{dropped} body-load record(s) were dropped: the ring of {self.loads.capacity} records filled up "
                               "(launches replayed outside FluidSimulator.run / step)")

    def checkpoint(self):
        self.drain()
        return {"loads.sums": self.sums(), "loads.launches": np.array(self.issued), "loads.samples": np.array(self.samples),
                "loads.box": np.array(self.box), "loads.center": np.array(self.centre, np.float64), "loads.every": np.array(self.every),
                "loads.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (box, centre, every, start), or None."""
        if "loads.sums" not in z:
            return None
        return (tuple(int(b) for b in z["loads.box"]), tuple(float(c) for c in z["loads.center"]), int(z["loads.every"]), int(z["loads.start"]))

    def restore(self, z):
        """Continue where a checkpoint stopped: its (4, F) sums and both counters go to the device; the records of this ring are numbered
        on from its launches."""
        launches, samples = int(z["loads.launches"]), int(z["loads.samples"])
        self.dev.loads_sums(self.loads, write=z["loads.sums"], launches=launches, samples=samples)
        self.issued = self.base = launches
        self.samples = samples
        return samples

    def sums(self):
        return self.dev.loads_sums(self.loads) if self._final is None else self._final[0]

    def close(self):
        """Keep what body_surface() needs after the device object is gone."""
        self._final = (self.dev.loads_sums(self.loads), self.samples)

    def data(self):
        rec = np.concatenate(self._records) if self._records else np.zeros((0, len(RECORD)))
        k0 = self._sampled(self.base)
        step = self.start_step + self.every * np.arange(k0 + 1, k0 + len(rec) + 1, dtype=np.int64)
        out = {"step": step, "time": step * self.dt}
        for c, name in enumerate(RECORD):
            out[name] = rec[:, c].copy()
        out["force_x"] = out["pressure_x"] + out["viscous_x"]
        out["force_y"] = out["pressure_y"] + out["viscous_y"]
        out["moment"] = out["moment_pressure"] + out["moment_viscous"]
        return out

    def surface(self):
        sums = self.sums()
        samples = self.samples if self._final is None else self._final[1]
        out = {"faces": self.faces.copy()}
        out.update(face_geometry(self.faces, self.centre))
        out["p_mean"], out["p_rms"], out["tau_mean"], out["tau_rms"] = surface_statistics(sums, samples)
        out["samples"], out["sums"] = int(samples), sums
        return out
