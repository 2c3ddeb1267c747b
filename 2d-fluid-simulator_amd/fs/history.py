"""Host side of the per-step history (new; the reference has none): the face list of a body, probe checks, and the frequency of a signal.

The recording itself is a device launch per step (csrc/fs_history.h, include/fs_hip.h fs_history_*), driven by
FluidSimulator.record_history / history / stop_history."""
import numpy as np

from .riders import Rider, ring_room

FLUID, WALL = 0, 1
# direction wall -> fluid of a face: (di, dj) of the fluid cell seen from the wall cell, in the order of the `dir` codes of fs_history_create
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))
SIGNS = (-1.0, 1.0, -1.0, 1.0)          # force_x for dir 0 / 1, force_y for dir 2 / 3: the signs of fs_flow_stats


def body_faces(mask, box):
    """Faces of the body in `box` = (x0, y0, x1, y1) (global cells, half-open): for every wall cell (mask 1) inside the box and each of its 4
    neighbours inside the domain that is fluid (mask 0), (x, y, dir) of the FLUID cell and the direction wall -> fluid.  The same faces whose
    pressure fs_flow_stats sums into force_x / force_y.  -> int32 (n, 3), sorted by (y, x, dir), no duplicates."""
    mask = np.asarray(mask)
    X, Y = mask.shape
    x0, y0, x1, y1 = (int(b) for b in box)
    if not (0 <= x0 <= x1 <= X and 0 <= y0 <= y1 <= Y):
        raise ValueError(f"body box {box} must satisfy 0 <= x0 <= x1 <= {X} and 0 <= y0 <= y1 <= {Y}")
    wall = np.zeros((X, Y), bool)
    wall[x0:x1, y0:y1] = mask[x0:x1, y0:y1] == WALL
    fluid = mask == FLUID
    parts = []
    for d, (di, dj) in enumerate(DIRS):
        fsl = (slice(max(0, di), X + min(0, di)), slice(max(0, dj), Y + min(0, dj)))      # fluid cells f whose wall cell f - (di, dj) exists
        wsl = (slice(max(0, -di), X - max(0, di)), slice(max(0, -dj), Y - max(0, dj)))
        fx, fy = np.nonzero(fluid[fsl] & wall[wsl])
        parts.append(np.stack([fx + max(0, di), fy + max(0, dj), np.full(fx.shape, d)], axis=1))
    faces = np.concatenate(parts).astype(np.int32).reshape(-1, 3)
    return faces[np.lexsort((faces[:, 2], faces[:, 0], faces[:, 1]))]


def check_probes(mask, points):
    """Probe cells (x, y) -> int32 (P, 2).  ValueError for a point outside the domain, on a cell that is not fluid (the lazily bounded
    pressure is not defined on boundary cells), or given twice."""
    mask = np.asarray(mask)
    X, Y = mask.shape
    pts = np.asarray([tuple(int(c) for c in q) for q in points], dtype=np.int32).reshape(-1, 2)
    seen = set()
    for x, y in pts.tolist():
        if not (0 <= x < X and 0 <= y < Y):
            raise ValueError(f"probe ({x}, {y}) lies outside the {X} x {Y} domain")
        if mask[x, y] != FLUID:
            raise ValueError(f"probe ({x}, {y}) is not a fluid cell (mask {int(mask[x, y])})")
        if (x, y) in seen:
            raise ValueError(f"probe ({x}, {y}) is given twice")
        seen.add((x, y))
    return pts


def owned(items, y0, nyl):
    """Indices of the rows of `items` ((n, >= 2) ints: x, y, ...) whose cell lies in the owned rows [y0, y0 + nyl) of a slab."""
    if len(items) == 0:
        return np.zeros(0, np.int64)
    items = np.asarray(items).reshape(len(items), -1)
    return np.nonzero((items[:, 1] >= y0) & (items[:, 1] < y0 + nyl))[0]


def dominant_frequency(signal, dt):
    """Frequency of the highest peak of the spectrum of `signal` sampled every `dt`: mean removed, Hann window, real FFT; the zero bin is
    never the answer.  For a lift signal: the shedding frequency f, and the Strouhal number f D / U."""
    s = np.asarray(signal, np.float64).ravel()
    n = s.size
    if n < 4:
        raise ValueError("dominant_frequency needs at least 4 samples")
    spec = np.abs(np.fft.rfft((s - s.mean()) * np.hanning(n)))
    spec[0] = 0.0
    return int(np.argmax(spec)) / (n * float(dt))


class Recorder(Rider):
    """One history of a FluidSimulator (record_history): the device ring, the records drained from it so far, and how many record launches
    have been issued - from which the simulator knows how many steps it may run before the ring is full (room)."""
    stop_in_capture, keeps_last, replaces_attached = False, True, True

    def __init__(self, dev, hist, probes, box, every, start_step, dt):
        self.dev, self.hist, self.probes, self.box = dev, hist, probes, box
        self.every, self.start_step, self.dt = int(every), int(start_step), float(dt)
        self.issued = 0          # record launches issued (captured launches count when their capture runs once)
        self.drained = 0         # records read back
        self._forces, self._values = [], []

    @property
    def token(self):
        return ("history", self.hist.serial)

    def room(self):
        """Steps that may run before the next one would find the ring full: the ring holds issued // every - drained records."""
        return ring_room(self.issued, self.every, 0, self.hist.capacity, self.drained)

    def launch(self, sim):
        self._make_room()
        v, p = sim._solver.get_fields()[:2]
        self.dev.history_record(self.hist, sim._solver.dx, v, p)
        self.issued += 1

    def free(self):
        self.dev.history_free(self.hist)

    def drain(self):
        forces, values, launches, dropped = self.dev.history_read(self.hist)
        self.issued = launches
        if len(forces):
            self._forces.append(forces)
            self._values.append(values)
            self.drained += len(forces)
        if dropped:
            raise RuntimeError(f"{dropped} history record(s) were dropped: the ring of {self.hist.capacity} records filled up "
                               "(launches replayed outside FluidSimulator.run / step)")

    def data(self):
        P = len(self.probes)
        forces = np.concatenate(self._forces) if self._forces else np.zeros((0, 2))
        values = np.concatenate(self._values) if self._values else np.zeros((0, P, 3))
        step = self.start_step + self.every * np.arange(1, len(forces) + 1, dtype=np.int64)
        out = {"step": step, "time": step * self.dt, "probes": np.asarray(self.probes, np.int32).reshape(P, 2),
               "u": values[..., 0].reshape(len(forces), P), "w": values[..., 1].reshape(len(forces), P),
               "p": values[..., 2].reshape(len(forces), P)}
        if self.box is not None:
            out["force_x"], out["force_y"] = forces[:, 0].copy(), forces[:, 1].copy()
        return out
