"""NumPy restatement of the kinetic-energy budget's accumulation (csrc/fs_budget.h, include/fs_hip.h fs_budget_*): the 21 values of a cell
from its own (u, w, p) and its four neighbours' (u, w) through the restatement of the vortex identification (tests/vortex_ref.py limited /
gradient), and the accumulation over the fluid cells of a box - every product and sum one NumPy operation in the order the kernel takes.
Arrays are (X, Y) like every host array of the product: cell (i, j) at [i, j]."""
import numpy as np

import vortex_ref as R

NPLANE = 21
NAMES = ("u", "w", "p", "uu", "ww", "uw", "pu", "pw", "uuu", "uuw", "wwu", "www", "ux", "uy", "wx", "wy", "uxux", "uyuy", "wxwx", "wywy", "pd")


def _values(u, w, q, ux, uy, wx, wy):
    with np.errstate(all="ignore"):
        a, b, c, d = u * u, u * w, w * w, ux + wy
        return np.stack([u, w, q, a, c, b, q * u, q * w, a * u, a * w, c * u, c * w, ux, uy, wx, wy, ux * ux, uy * uy, wx * wx, wy * wy, q * d])


def cells(inp, two_dx, limit=None):
    """budget_cell on rows of (u, w, p, ul, wl, ur, wr, um, wm, un, wn) in the fields' precision -> float64 (n, 21)."""
    inp = np.asarray(inp)
    pairs = R.limited(np.stack([inp[:, [0, 1]], inp[:, [3, 4]], inp[:, [5, 6]], inp[:, [7, 8]], inp[:, [9, 10]]]), limit).astype(np.float64)
    (u, w), (ul, wl), (ur, wr), (um, wm), (un, wn) = (pairs[k].T for k in range(5))
    with np.errstate(all="ignore"):
        ux, uy, wx, wy = (ur - ul) / two_dx, (un - um) / two_dx, (wr - wl) / two_dx, (wn - wm) / two_dx
    return _values(u, w, inp[:, 2].astype(np.float64), ux, uy, wx, wy).T


def values(v, p, dx, limit=None):
    """The 21 values of every cell of the grid, float64 (21, X, Y) (the mask is applied by the accumulation)."""
    p = np.asarray(p)
    p = p[..., 0] if p.ndim == 3 else p
    lv = R.limited(v, limit)
    ux, uy, wx, wy, _ = R.gradient(v, dx, limit)
    return _values(lv[..., 0].astype(np.float64), lv[..., 1].astype(np.float64), p.astype(np.float64), ux, uy, wx, wy)


class State:
    """A fresh fs_budget_create."""

    def __init__(self, box, dx, every, start):
        self.box, self.dx, self.every, self.start = tuple(box), dx, every, start
        self.sums = np.zeros((NPLANE, box[2] - box[0], box[3] - box[1]), np.float64)
        self.launches = self.samples = 0

    def launch(self, v, p, mask, limit=None):
        """One fs_budget_launch, sampling or not."""
        n = self.launches
        self.launches = n + 1
        if not (n + 1 > self.start and (n + 1 - self.start) % self.every == 0):
            return
        x0, y0, x1, y1 = self.box
        fluid = np.asarray(mask)[x0:x1, y0:y1] == 0
        with np.errstate(all="ignore"):
            self.sums = np.where(fluid, self.sums + values(v, p, self.dx, limit)[:, x0:x1, y0:y1], self.sums)
        self.samples += 1
