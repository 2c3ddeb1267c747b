"""Host side of the vortex identification (new; the reference has none): the rider that keeps the device ring of samples
(csrc/fs_vortex.h, include/fs_hip.h fs_vortex_*), the conversion of its integer records into physical quantities, and the tracking of
vortices from sample to sample.  Pure NumPy apart from the rider class: testable without a device.  Driven by
FluidSimulator.track_vortices / vortices / stop_vortices / find_vortices / vortex_labels / vortex_criterion.

A sample is NHEAD header words and `count` records of NREC words, all int64 (HEAD / RECORD below name them).  Every sum is an integer: a
record does not depend on the order of the device's atomics, and a restatement (tests/vortex_ref.py) reproduces it exactly.  convert()
documents the order of every conversion to floating point."""
import math

import numpy as np

from .riders import Rider, ring_room, samples_after
from .solver import VELOCITY_LIMIT      # noqa: F401 (limit_field's bound on the speed: the default omega_max is 2 * VELOCITY_LIMIT / dx)

CRITERIA = ("q", "swirl", "vorticity")
HEAD = ("launch", "components", "passed", "count", "clipped", "dropped_cells")
RECORD = ("label", "area", "sum_q", "sum_aq", "sum_x", "sum_y", "mx_lo", "mx_hi", "my_lo", "my_hi", "xmin", "xmax", "ymin", "ymax", "peak",
          "flag")
NHEAD, NREC, MAX_VORTICES = 8, 16, 1024


def omega_exponent(omega_max):
    """e = ceil(log2(omega_max)) without a logarithm: omega_max = m 2^k with 0.5 <= m < 1 (math.frexp) gives k - 1 for m == 0.5, else k."""
    omega_max = float(omega_max)
    if not (math.isfinite(omega_max) and omega_max > 0.0):
        raise ValueError(f"omega_max must be finite and positive, got {omega_max}")
    m, k = math.frexp(omega_max)
    return k - 1 if m == 0.5 else k


def split_samples(words, max_vortices):
    """The ring's words (n, NHEAD + NREC * max_vortices) int64 -> ({name: int64 (n,)} of HEAD, {name: int64 (R,)} of RECORD plus "sample":
    the index of each record's sample in `words`), the records of sample 0 first, each sample's in label order."""
    words = np.asarray(words, np.int64).reshape(-1, NHEAD + NREC * int(max_vortices))
    head = {name: words[:, k].copy() for k, name in enumerate(HEAD)}
    rec = words[:, NHEAD:].reshape(len(words), int(max_vortices), NREC)
    keep = np.arange(int(max_vortices))[None, :] < head["count"][:, None]
    raw = {name: rec[..., k][keep] for k, name in enumerate(RECORD)}
    raw["sample"] = np.broadcast_to(np.arange(len(words), dtype=np.int64)[:, None], keep.shape)[keep]
    return head, raw


def convert(raw, e, dx, nx):
    """The integer records `raw` (split_samples) -> the physical quantities, float64 unless said, in this order of operations:
      sign         +1 for flag 1 (om >= 0), -1 for flag 2
      circulation  ldexp(float(sum_q), e - 30) * (dx * dx): the int64 -> float64 conversion rounds to nearest, ldexp is exact
      x, y         float(Mx) / float(2 * sum_aq) with Mx = mx_lo + (mx_hi << 32) as Python integers: the |om|-weighted mean of i + 0.5, in
                   cells; the geometric centroid where sum_aq is 0
      xg, yg       float(sum_x) / float(2 * area)
      peak_omega   sign * ldexp(float(peak >> 32), e - 30)
      peak_cell    int64 (R, 2): (idx % nx, idx // nx) of idx = 0xFFFFFFFF - (peak & 0xFFFFFFFF), the smallest cell index with the largest |q|
      bbox         int64 (R, 4): xmin, ymin, xmax, ymax (inclusive)"""
    n = len(raw["label"])
    out = {"sample": raw["sample"].copy(), "label": raw["label"].copy(), "area": raw["area"].copy(),
           "sign": np.where(raw["flag"] == 1, 1, -1).astype(np.int64)}
    out["circulation"] = np.ldexp(raw["sum_q"].astype(np.float64), e - 30) * (dx * dx)
    xg = raw["sum_x"].astype(np.float64) / (2 * raw["area"]).astype(np.float64)
    yg = raw["sum_y"].astype(np.float64) / (2 * raw["area"]).astype(np.float64)
    x, y = xg.copy(), yg.copy()
    for k in range(n):
        den = 2 * int(raw["sum_aq"][k])
        if den > 0:
            x[k] = float(int(raw["mx_lo"][k]) + (int(raw["mx_hi"][k]) << 32)) / float(den)
            y[k] = float(int(raw["my_lo"][k]) + (int(raw["my_hi"][k]) << 32)) / float(den)
    out["x"], out["y"], out["xg"], out["yg"] = x, y, xg, yg
    out["peak_omega"] = out["sign"] * np.ldexp((raw["peak"] >> 32).astype(np.float64), e - 30)
    idx = 0xFFFFFFFF - (raw["peak"] & 0xFFFFFFFF)
    out["peak_cell"] = np.stack([idx % nx, idx // nx], axis=1).astype(np.int64).reshape(n, 2)
    out["bbox"] = np.stack([raw["xmin"], raw["ymin"], raw["xmax"], raw["ymax"]], axis=1).astype(np.int64).reshape(n, 4)
    return out


def assemble(words, max_vortices, e, dx, nx, steps, dt):
    """What FluidSimulator.vortices() / find_vortices() return, from the ring's words and the step of every sample."""
    head, raw = split_samples(words, max_vortices)
    steps = np.asarray(steps, np.int64)
    out = {"step": steps, "time": steps * float(dt)}
    for name in HEAD[1:]:
        out[name] = head[name]
    out.update(convert(raw, e, dx, nx))
    out["raw"] = raw
    out["exponent"] = int(e)
    return out


# ---- tracking: records of consecutive samples joined into tracks ------------------------------------------------------------------------
def link(records, max_distance, dt=1.0):
    """Join the records of consecutive samples into tracks -> int64 (R,): a track id per record, numbered from 0 in order of first
    appearance (sample, then label).  `records`: a mapping with "sample", "label", "sign", "x", "y" (what vortices() returns) and, when the
    samples are not equally spaced, "time" per SAMPLE with `dt` ignored; otherwise consecutive samples are `dt` apart.  A record of sample
    s + 1 continues the track of a record of sample s when both have the same sign and it is the nearest to the track's predicted position
    (the last position plus the last displacement per unit time, times the time between the samples; no displacement for a track of one
    record) within max_distance (cells).  Candidates are taken in ascending distance, ties by the smaller label of the new record and then
    of the old; each record is used once.  Merging and splitting are not followed: a record that continues nothing starts a new track."""
    sample = np.asarray(records["sample"], np.int64)
    label = np.asarray(records["label"], np.int64)
    sign = np.asarray(records["sign"], np.int64)
    x, y = np.asarray(records["x"], np.float64), np.asarray(records["y"], np.float64)
    times = np.asarray(records["time"], np.float64) if "time" in records else None
    track = np.full(len(sample), -1, np.int64)
    vel = np.zeros((len(sample), 2))
    nxt = 0
    prev = np.zeros(0, np.int64)
    for s in (np.unique(sample) if len(sample) else []):
        cur = np.nonzero(sample == s)[0]
        cur = cur[np.argsort(label[cur], kind="stable")]
        if len(prev) and sample[prev[0]] == s - 1:
            h = float(times[s] - times[s - 1]) if times is not None else float(dt)
            px, py = x[prev] + vel[prev, 0] * h, y[prev] + vel[prev, 1] * h
            cand = []
            for a in cur:
                d = np.hypot(px - x[a], py - y[a])
                for k in np.nonzero((d <= max_distance) & (sign[prev] == sign[a]))[0]:
                    cand.append((d[k], label[a], label[prev[k]], a, prev[k]))
            used_new, used_old = set(), set()
            for d, _, _, a, b in sorted(cand):
                if a in used_new or b in used_old:
                    continue
                used_new.add(a)
                used_old.add(b)
                track[a] = track[b]
                vel[a] = ((x[a] - x[b]) / h, (y[a] - y[b]) / h)
        for a in cur:
            if track[a] < 0:
                track[a] = nxt
                nxt += 1
        prev = cur
    return track


def _record_times(records, dt):
    sample = np.asarray(records["sample"], np.int64)
    if "time" in records:
        return np.asarray(records["time"], np.float64)[sample]
    return sample * float(dt)


def convection_velocity(records, tracks, dx, dt=1.0):
    """Least-squares velocity of every track -> {"track": ids ascending, "n": records per track, "ux", "uy": d(x dx)/dt and d(y dx)/dt of the
    straight line through the track's positions over time (NaN for a track of one record)}.  Time: records["time"] per sample, or sample * dt."""
    tracks = np.asarray(tracks, np.int64)
    t = _record_times(records, dt)
    x, y = np.asarray(records["x"], np.float64) * dx, np.asarray(records["y"], np.float64) * dx
    ids = np.unique(tracks)
    out = {"track": ids, "n": np.zeros(len(ids), np.int64), "ux": np.full(len(ids), np.nan), "uy": np.full(len(ids), np.nan)}
    for k, tid in enumerate(ids):
        m = tracks == tid
        out["n"][k] = m.sum()
        tc = t[m] - t[m].mean()
        den = float((tc * tc).sum())
        if out["n"][k] >= 2 and den > 0.0:
            out["ux"][k] = float((tc * x[m]).sum()) / den
            out["uy"][k] = float((tc * y[m]).sum()) / den
    return out


def street_spacing(records, tracks, dx, sample=None):
    """The geometry of a vortex street in one sample (default: the last) -> {"a": the mean streamwise distance between neighbours of one
    sign, over both signs (NaN when no sign has two), "a_pos", "a_neg": per sign, "h": the lateral offset of the two
    rows, mean y of the positive minus mean y of the negative ones, "ratio": |h| / a}, lengths in units of dx * cells.  `tracks` restricts the
    records to those whose track has at least two records (pass None to take all)."""
    smp = np.asarray(records["sample"], np.int64)
    s = int(smp.max()) if sample is None else int(sample)
    m = smp == s
    if tracks is not None:
        tracks = np.asarray(tracks, np.int64)
        ids, counts = np.unique(tracks, return_counts=True)
        m &= np.isin(tracks, ids[counts >= 2])
    sign = np.asarray(records["sign"], np.int64)[m]
    x, y = np.asarray(records["x"], np.float64)[m] * dx, np.asarray(records["y"], np.float64)[m] * dx
    out = {}
    for name, sg in (("a_pos", 1), ("a_neg", -1)):
        xs = np.sort(x[sign == sg])
        out[name] = float(np.diff(xs).mean()) if len(xs) >= 2 else float("nan")
    gaps = np.concatenate([np.diff(np.sort(x[sign == sg])) for sg in (1, -1)])
    out["a"] = float(gaps.mean()) if len(gaps) else float("nan")
    out["h"] = float(y[sign == 1].mean() - y[sign == -1].mean()) if (sign == 1).any() and (sign == -1).any() else float("nan")
    out["ratio"] = abs(out["h"]) / out["a"]
    return out


class Vortices(Rider):
    """The vortex tracker of a FluidSimulator (track_vortices): the device object, the samples drained from its ring so far, and how many
    launches have been issued - from which the simulator knows how many steps it may run before the ring is full (room)."""
    stop_in_capture, keeps_last = False, True

    def __init__(self, dev, vx, every, start_step, dt, dx):
        self.dev, self.vx, self.every, self.start_step, self.dt, self.dx = dev, vx, int(every), int(start_step), float(dt), float(dx)
        self.issued = 0          # launches issued (captured launches count when their capture runs once)
        self.base = 0            # launches before this ring existed (restore)
        self.drained = 0         # samples read back
        self._words = []
        self._planes = None      # (flags, labels) kept by close()

    @property
    def token(self):
        return ("vortices", self.vx.serial)

    def room(self):
        return ring_room(self.issued, self.every, self.start_step, self.vx.capacity, self.drained + samples_after(self.base, self.every, self.start_step))

    def launch(self, sim):
        self._make_room()
        self.dev.vortex_launch(self.vx, sim._solver.dx, sim._solver.get_fields()[0])
        self.issued += 1

    def drain(self):
        words, launches, lost = self.dev.vortex_read(self.vx)
        self.issued = launches
        if len(words):
            self._words.append(words)
            self.drained += len(words)
        if lost:
            raise RuntimeError(f"{lost} vortex sample(s) were lost: the ring of {self.vx.capacity} samples filled up "
                               "(launches replayed outside FluidSimulator.run / step)")

    def close(self):
        self._planes = self.dev.vortex_labels(self.vx)

    def free(self):
        self.dev.vortex_free(self.vx)

    def planes(self):
        return self.dev.vortex_labels(self.vx) if self._planes is None else self._planes

    def data(self):
        vx = self.vx
        words = np.concatenate(self._words) if self._words else np.zeros((0, NHEAD + NREC * vx.max_vortices), np.int64)
        return assemble(words, vx.max_vortices, vx.exponent, self.dx, self.dev.nx, words[:, 0] + 1, self.dt)

    def checkpoint(self):
        self.drain()
        vx = self.vx
        words = np.concatenate(self._words) if self._words else np.zeros((0, NHEAD + NREC * vx.max_vortices), np.int64)
        return {"vortex.words": words, "vortex.launches": np.array(self.issued), "vortex.every": np.array(self.every),
                "vortex.start": np.array(self.start_step), "vortex.criterion": np.array(vx.criterion), "vortex.threshold": np.array(vx.threshold),
                "vortex.exponent": np.array(vx.exponent), "vortex.min_area": np.array(vx.min_area), "vortex.max_vortices": np.array(vx.max_vortices),
                "vortex.max_components": np.array(vx.max_components)}

    @staticmethod
    def held(z):
        """-> (criterion, threshold, every, min_area, max_vortices), or None."""
        if "vortex.words" not in z:
            return None
        return (str(z["vortex.criterion"]), float(z["vortex.threshold"]), int(z["vortex.every"]), int(z["vortex.min_area"]), int(z["vortex.max_vortices"]))

    def restore(self, z):
        """Continue where a checkpoint stopped: its samples are this tracker's first, the launch count goes to the device."""
        words = np.asarray(z["vortex.words"], np.int64)
        if words.shape[1:] != (NHEAD + NREC * self.vx.max_vortices,):
            raise ValueError("the checkpoint's vortex samples were taken with another max_vortices")
        launches = int(z["vortex.launches"])
        self.dev.vortex_set(self.vx, launches)
        self.issued = self.base = launches
        self.drained = 0
        self._words = [words] if len(words) else []
        return len(words)
