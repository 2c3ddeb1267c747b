"""NumPy restatement of the vortex identification (csrc/fs_vortex.h, include/fs_hip.h fs_vortex_*): criterion and flags in the expression
order of the header, labels by a plain breadth-first search (the label of a component is its smallest j * X + i), the integer accumulators, the
record selection and the host conversions.  Arrays are (X, Y) like every host array of the product: cell (i, j) at [i, j].  No SciPy.

Also the flag patterns the labelling tests share (CPU: tests/test_vortex_cpu.py, GPU: tests/test_gpu_vortices.py)."""
import math
from collections import deque

import numpy as np

QMAX = 1 << 30
NHEAD, NREC = 8, 16
CRITERIA = ("q", "swirl", "vorticity")


# ---- a. criterion and flags ----------------------------------------------------------------------------------------------------------------
def limited(v, limit):
    """limit_field's per-cell function (csrc/fs_kernels.h limit_cell) on every cell, in the field's own precision."""
    v = np.array(v)
    if limit is None:
        return v
    T = v.dtype.type
    x, y = v[..., 0], v[..., 1]
    nrm = np.sqrt(x * x + y * y)
    over = nrm > T(limit)
    with np.errstate(all="ignore"):
        v[..., 0] = np.where(over, T(limit) * (x / nrm), x)
        v[..., 1] = np.where(over, T(limit) * (y / nrm), y)
    return v


def gradient(v, dx, limit=None):
    """-> ux, uy, wx, wy, om, float64 (X, Y): central differences with the neighbour indices clamped at the domain edge, every operation
    rounded on its own."""
    v = limited(v, limit)
    u, w = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
    X, Y = u.shape
    il, ir = np.clip(np.arange(X) - 1, 0, X - 1), np.clip(np.arange(X) + 1, 0, X - 1)
    jm, jn = np.clip(np.arange(Y) - 1, 0, Y - 1), np.clip(np.arange(Y) + 1, 0, Y - 1)
    two_dx = 2.0 * dx
    with np.errstate(all="ignore"):
        ux = (u[ir] - u[il]) / two_dx
        uy = (u[:, jn] - u[:, jm]) / two_dx
        wx = (w[ir] - w[il]) / two_dx
        wy = (w[:, jn] - w[:, jm]) / two_dx
        om = ((w[ir] - w[il]) - (u[:, jn] - u[:, jm])) / two_dx
    return ux, uy, wx, wy, om


def criterion(which, v, mask, dx, limit=None):
    """-> (c, om): c is 0 on cells that are not fluid."""
    ux, uy, wx, wy, om = gradient(v, dx, limit)
    with np.errstate(all="ignore"):
        if which == "q":
            t = ux * ux
            t = t + wy * wy
            c = (-0.5 * t) - uy * wx
        elif which == "swirl":
            s = ux + wy
            c = (ux * wy - uy * wx) - 0.25 * (s * s)
        elif which == "vorticity":
            c = om * om
        else:
            raise ValueError(which)
    return np.where(np.asarray(mask) == 0, c, 0.0), om


def flag_plane(c, om, mask, threshold):
    with np.errstate(invalid="ignore"):
        hit = (np.asarray(mask) == 0) & (c > threshold)
        return np.where(hit, np.where(om >= 0.0, 1, 2), 0).astype(np.uint8)


# ---- b. labels -----------------------------------------------------------------------------------------------------------------------------
def label_plane(flags):
    """int32 (X, Y): the smallest j * X + i of the 4-connected component of equal flag, -1 where the flag is 0.  Cells are visited in
    ascending j * X + i, so the first cell of a component that is met is its minimum."""
    flags = np.asarray(flags)
    X, Y = flags.shape
    lab = np.full((X, Y), -1, np.int32)
    f = flags.tolist()
    out = lab.tolist()
    for j in range(Y):
        for i in range(X):
            if f[i][j] == 0 or out[i][j] >= 0:
                continue
            root, ff = j * X + i, f[i][j]
            out[i][j] = root
            todo = deque([(i, j)])
            while todo:
                a, b = todo.popleft()
                for c, d in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                    if 0 <= c < X and 0 <= d < Y and f[c][d] == ff and out[c][d] < 0:
                        out[c][d] = root
                        todo.append((c, d))
    return np.array(out, np.int32).reshape(X, Y)


# ---- d. the integer accumulators -------------------------------------------------------------------------------------------------------------
def omega_exponent(omega_max):
    m, k = math.frexp(float(omega_max))
    return k - 1 if m == 0.5 else k


def quantise(om, e):
    """-> (q int64, clipped bool): llrint(ldexp(om, 30 - e)) clamped to +-2^30; NaN -> 0, clipped."""
    with np.errstate(all="ignore"):
        s = np.ldexp(np.asarray(om, np.float64), 30 - e)
        hi, lo, nan = s >= QMAX, s <= -QMAX, np.isnan(s)
        q = np.where(hi, QMAX, np.where(lo, -QMAX, np.where(nan, 0, np.rint(np.where(hi | lo | nan, 0.0, s))))).astype(np.int64)
    return q, hi | lo | nan


def accumulate(flags, labels, om, e, max_components):
    """-> (list of per-component dicts of Python integers in ascending label order - all roots, the first max_components of them with sums -
    , clipped, dropped cells)."""
    X, Y = flags.shape
    q, clip = quantise(om, e)
    on = flags != 0
    roots = np.unique(labels[on])      # ascending: the dense ids
    ident = {int(r): k for k, r in enumerate(roots.tolist())}
    comps = [None] * min(len(roots), max_components)
    dropped = 0
    ii, jj = np.nonzero(on)
    for i, j in zip(ii.tolist(), jj.tolist()):
        k = ident[int(labels[i, j])]
        if k >= max_components:
            dropped += 1
            continue
        c = comps[k]
        if c is None:
            c = comps[k] = {"label": int(labels[i, j]), "area": 0, "sum_q": 0, "sum_aq": 0, "sum_x": 0, "sum_y": 0, "mx": 0, "my": 0, "mx_lo": 0,
                            "mx_hi": 0, "my_lo": 0, "my_hi": 0, "xmin": i, "xmax": i, "ymin": j, "ymax": j, "peak": 0,
                            "flag": int(flags[int(labels[i, j]) % X, int(labels[i, j]) // X])}
        qq = int(q[i, j])
        aq = abs(qq)
        tx, ty = aq * (2 * i + 1), aq * (2 * j + 1)
        c["area"] += 1
        c["sum_q"] += qq
        c["sum_aq"] += aq
        c["sum_x"] += 2 * i + 1
        c["sum_y"] += 2 * j + 1
        c["mx_lo"] += tx & 0xFFFFFFFF
        c["mx_hi"] += tx >> 32
        c["my_lo"] += ty & 0xFFFFFFFF
        c["my_hi"] += ty >> 32
        c["xmin"], c["xmax"] = min(c["xmin"], i), max(c["xmax"], i)
        c["ymin"], c["ymax"] = min(c["ymin"], j), max(c["ymax"], j)
        c["peak"] = max(c["peak"], (aq << 32) | (0xFFFFFFFF - (j * X + i)))
    return comps, len(roots), int(clip[on].sum()), dropped


RECORD = ("label", "area", "sum_q", "sum_aq", "sum_x", "sum_y", "mx_lo", "mx_hi", "my_lo", "my_hi", "xmin", "xmax", "ymin", "ymax", "peak", "flag")


# ---- e. the records of a sample ----------------------------------------------------------------------------------------------------------------
def sample(v, mask, dx, which, threshold, e, min_area=4, max_vortices=64, max_components=65536, limit=None):
    """One sample of the fields -> {"components", "passed", "count", "clipped", "dropped_cells", "raw": {name: int64 (count,)}, "flags",
    "labels"}."""
    c, om = criterion(which, v, mask, dx, limit)
    flags = flag_plane(c, om, mask, threshold)
    labels = label_plane(flags)
    comps, found, clipped, dropped = accumulate(flags, labels, om, e, max_components)
    keep = [c for c in comps if c["area"] >= min_area]
    recs = keep[:max_vortices]
    raw = {name: np.array([r[name] for r in recs], np.int64).reshape(len(recs)) for name in RECORD}
    return {"components": found, "passed": len(keep), "count": len(recs), "clipped": clipped, "dropped_cells": dropped, "raw": raw,
            "flags": flags, "labels": labels}


def convert(raw, e, dx, nx):
    """The conversions FluidSimulator.vortices() documents, on the same integers (Python integers and floats throughout)."""
    n = len(raw["label"])
    out = {k: [] for k in ("sign", "circulation", "x", "y", "xg", "yg", "peak_omega", "peak_cell", "bbox")}
    for k in range(n):
        r = {name: int(raw[name][k]) for name in RECORD}
        sign = 1 if r["flag"] == 1 else -1
        out["sign"].append(sign)
        out["circulation"].append(math.ldexp(float(r["sum_q"]), e - 30) * (dx * dx))
        xg, yg = float(r["sum_x"]) / float(2 * r["area"]), float(r["sum_y"]) / float(2 * r["area"])
        if r["sum_aq"] > 0:
            x = float(r["mx_lo"] + (r["mx_hi"] << 32)) / float(2 * r["sum_aq"])
            y = float(r["my_lo"] + (r["my_hi"] << 32)) / float(2 * r["sum_aq"])
        else:
            x, y = xg, yg
        out["x"].append(x); out["y"].append(y); out["xg"].append(xg); out["yg"].append(yg)
        out["peak_omega"].append(sign * math.ldexp(float(r["peak"] >> 32), e - 30))
        idx = 0xFFFFFFFF - (r["peak"] & 0xFFFFFFFF)
        out["peak_cell"].append((idx % nx, idx // nx))
        out["bbox"].append((r["xmin"], r["ymin"], r["xmax"], r["ymax"]))
    return {"sign": np.array(out["sign"], np.int64).reshape(n), "circulation": np.array(out["circulation"], np.float64).reshape(n),
            "x": np.array(out["x"], np.float64).reshape(n), "y": np.array(out["y"], np.float64).reshape(n),
            "xg": np.array(out["xg"], np.float64).reshape(n), "yg": np.array(out["yg"], np.float64).reshape(n),
            "peak_omega": np.array(out["peak_omega"], np.float64).reshape(n), "peak_cell": np.array(out["peak_cell"], np.int64).reshape(n, 2),
            "bbox": np.array(out["bbox"], np.int64).reshape(n, 4)}


# ---- flag patterns of the labelling tests ----------------------------------------------------------------------------------------------------
def serpentine(X, Y):
    """A one-cell-wide path from cell 0 through every second column, up one and down the next: ONE component whose root is cell 0."""
    f = np.zeros((X, Y), np.uint8)
    for k, i in enumerate(range(0, X, 2)):
        f[i, :] = 1
        if i + 2 < X:
            f[i + 1, Y - 1 if k % 2 == 0 else 0] = 1
    return f


def spiral(X, Y):
    """A one-cell-wide rectangular spiral from cell 0 inwards, rings two cells apart: one component."""
    f = np.zeros((X, Y), np.uint8)
    x0, y0, x1, y1 = 0, 0, X - 1, Y - 1
    i, j = 0, 0
    f[0, 0] = 1
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        for ti, tj in ((x1, y0), (x1, y1), (x0, y1), (x0, y0 + 2)):
            while (i, j) != (ti, tj):
                i += (ti > i) - (ti < i)
                j += (tj > j) - (tj < j)
                f[i, j] = 1
        x0 += 2; y0 += 2; x1 -= 2; y1 -= 2
        if x1 - x0 < 2 or y1 - y0 < 2:
            break
        while (i, j) != (x0, y0):
            i += (x0 > i) - (x0 < i)
            f[i, j] = 1
    return f


def u_shape(X, Y, tx, ty):
    """Two vertical arms in the first and in a later column tile, joined only in the last row tile: the seams unite two tile-local roots,
    neither of which is the minimum (the arms start in row 1 of a tile row further down than the first)."""
    f = np.zeros((X, Y), np.uint8)
    a, b = 3, ((X - 1) // tx) * tx + 1 if (X - 1) // tx >= 1 else X - 2
    b = min(b, X - 1)
    f[a, 1:] = 1
    f[b, 1:] = 1
    f[a:b + 1, Y - 1] = 1
    return f


def patterns(X, Y, tx=32, ty=8):
    """{name: uint8 (X, Y)} for a grid."""
    i, j = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    rng = np.random.default_rng(X * 1000 + Y)
    one = (rng.random((X, Y)) < 0.65).astype(np.uint8)
    r = rng.random((X, Y))
    two = np.where(r < 0.59 * 0.85, 1, np.where(r < 0.59, 2, 0)).astype(np.uint8)
    return {"empty": np.zeros((X, Y), np.uint8), "ones": np.ones((X, Y), np.uint8), "checkerboard": ((i + j) % 2 == 0).astype(np.uint8),
            "stripes": (1 + i % 2).astype(np.uint8), "serpentine": serpentine(X, Y), "spiral": spiral(X, Y), "u_shape": u_shape(X, Y, tx, ty),
            "random_one_sign": one, "random_two_signs": two}
