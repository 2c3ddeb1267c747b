"""Host side of the flow maps and FTLE fields (new; the reference has none).  The device (csrc/fs_lcs.h, include/fs_hip.h fs_flowmap_*) carries a
lattice of particles through the resident snapshots of the snapshot POD - linear in time between consecutive snapshots, forwards or backwards -
and returns the largest eigenvalue `lam` of the Cauchy-Green tensor of the map; here are the order in which the ring's slots are walked, the
step size, and the finite-time Lyapunov exponent FTLE = log(lam) / (2 |T|).  Pure NumPy: testable without a device.  Driven by
FluidSimulator.flow_map / ftle / ftle_fields.

Forward-time FTLE ridges mark the repelling Lagrangian coherent structures, backward-time ridges the attracting ones - the lines dye
collects on.  The backward map needs the past velocity, which only the ring still holds."""
import numpy as np

from .pod import ring_slots

REFINES = (1, 2, 4, 8)
MAX_SUBSTEPS = 16
UNSEEDED = 4          # status of a node whose start cell is a wall cell (0 alive, 1 LEFT, 2 WALL: as the tracers')
DIRECTIONS = ("forward", "backward")


def window(samples, slots, first=None, last=None):
    """-> (i0, i1): the resident samples first .. last (chronological indices, 0 the oldest; negative: from the newest; None: the oldest /
    the newest) as a checked pair 0 <= i0 < i1 <= n - 1."""
    n = min(int(samples), int(slots))
    if n < 2:
        raise RuntimeError(f"{n} samples resident, 2 needed for a flow map")
    idx = []
    for name, v, default in (("first", first, 0), ("last", last, n - 1)):
        v = default if v is None else int(v)
        if not -n <= v < n:
            raise IndexError(f"{name} = {v}: {n} samples are resident")
        idx.append(v % n)
    if idx[0] >= idx[1]:
        raise ValueError(f"first must lie before last, got samples {idx[0]} and {idx[1]} of {n}")
    return idx[0], idx[1]


def intervals(samples, slots, first=None, last=None, direction="backward"):
    """-> [(slot_from, slot_to), ...] in integration order: the intervals between consecutive resident samples of the window first .. last
    (window()), by fs.pod.ring_slots - a wrapped ring is walked chronologically.  "forward" walks first -> last, "backward" last -> first."""
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be one of {DIRECTIONS}, got {direction!r}")
    i0, i1 = window(samples, slots, first, last)
    order = [int(s) for s in ring_slots(samples, slots)[i0:i1 + 1]]
    if direction == "backward":
        order.reverse()
    return list(zip(order[:-1], order[1:]))


def step_size(every, dt, dx, substeps, direction):
    """The signed size of one sub-step in cell units: +- every dt / (dx substeps)."""
    h = float(every) * float(dt) / (float(dx) * float(substeps))
    return h if direction == "forward" else -h


def ftle(lam, span):
    """log(lam) / (2 |span|): NaN stays NaN, lam == 0 gives -inf; span = (window samples - 1) * every * dt."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(lam, np.float64)) / (2.0 * abs(float(span)))


def ridges(ftle_map, fraction=0.8):
    """A boolean map of the nodes whose FTLE lies above `fraction` of the finite maximum (a convenience, no ridge extraction)."""
    f = np.asarray(ftle_map, np.float64)
    finite = np.isfinite(f)
    if not finite.any():
        return np.zeros(f.shape, bool)
    with np.errstate(invalid="ignore"):
        return finite & (f > float(fraction) * f[finite].max())


def check_lattice(box, refine, substeps, shape):
    """-> (box as 4 ints - None: the whole domain, refine, substeps), checked against the grid `shape` = (X, Y)."""
    X, Y = shape
    box = (0, 0, X, Y) if box is None else tuple(int(b) for b in box)
    if len(box) != 4 or not (0 <= box[0] < box[2] <= X and 0 <= box[1] < box[3] <= Y):
        raise ValueError(f"box must be (x0, y0, x1, y1) with 0 <= x0 < x1 <= {X} and 0 <= y0 < y1 <= {Y}, got {box}")
    refine, substeps = int(refine), int(substeps)
    if refine not in REFINES:
        raise ValueError(f"refine must be one of {REFINES}, got {refine}")
    if not 1 <= substeps <= MAX_SUBSTEPS:
        raise ValueError(f"substeps must be 1 .. {MAX_SUBSTEPS}, got {substeps}")
    if refine * refine * (box[2] - box[0]) * (box[3] - box[1]) > 1 << 30:
        raise ValueError("a flow map holds at most 2^30 nodes")
    return box, refine, substeps


def start_positions(box, refine):
    """-> (x0, y0) float64 (nx, ny): node (a, b) starts at (box x0 + (a + 0.5) / refine, box y0 + (b + 0.5) / refine), in cell units."""
    a = box[0] + (np.arange(refine * (box[2] - box[0]), dtype=np.float64) + 0.5) / refine
    b = box[1] + (np.arange(refine * (box[3] - box[1]), dtype=np.float64) + 0.5) / refine
    x, y = np.meshgrid(a, b, indexing="ij")
    return np.ascontiguousarray(x), np.ascontiguousarray(y)
