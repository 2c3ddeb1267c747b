"""NumPy restatement of the scale-to-scale fluxes (csrc/fs_flux.h, include/fs_hip.h fs_flux_*): the eight base quantities through the
restatement of the vortex identification (tests/vortex_ref.py limited / gradient), the ordered window sums along x and along y - one NumPy
addition per term of the window, left to right -, the per-cell fluxes and the accumulation, every product and sum one NumPy operation in the
order the kernels take.  Arrays are (X, Y) like every host array of the product: cell (i, j) at [i, j]."""
import numpy as np

import vortex_ref as R

NQ, NSUM, MAX_WIDTHS, MAX_R = 8, 3, 8, 64
NAMES = ("u", "w", "om", "uu", "uw", "ww", "uom", "wom")


def base(v, mask, dx, limit=None):
    """(8, X, Y): U, W, OM, U U, U W, W W, U OM, W OM.  U, W where mask != 1, OM where mask == 0, +0 elsewhere."""
    mask = np.asarray(mask)
    lv = R.limited(v, limit)
    with np.errstate(all="ignore"):
        U = np.where(mask != 1, lv[..., 0].astype(np.float64), 0.0)
        W = np.where(mask != 1, lv[..., 1].astype(np.float64), 0.0)
        OM = np.where(mask == 0, R.gradient(v, dx, limit)[4], 0.0)
        return np.stack([U, W, OM, U * U, U * W, W * W, U * OM, W * OM])


def base_of(U, W, OM):
    """The eight planes from given U, W, OM (float64)."""
    with np.errstate(all="ignore"):
        return np.stack([U, W, OM, U * U, U * W, W * W, U * OM, W * OM])


def window_sums(q, r, axis):
    """The ordered sums of 2 r + 1 consecutive entries along `axis`: out[c] = (..(q[c] + q[c + 1]) .. + q[c + 2 r]), shorter by 2 r."""
    q = np.moveaxis(np.asarray(q, np.float64), axis, 0)
    n = 2 * r + 1
    m = q.shape[0] - n + 1
    assert m >= 1
    s = q[0:m].copy()
    with np.errstate(all="ignore"):
        for t in range(1, n):
            s = s + q[t:t + m]
    return np.moveaxis(s, 0, axis)


def filtered(q, r):
    """F (8, X, Y) of the base planes q: defined for r <= i <= X - 1 - r and r <= j <= Y - 1 - r, +0 elsewhere."""
    n = 2 * r + 1
    inv = 1.0 / float(n * n)
    K, X, Y = q.shape
    F = np.zeros_like(q)
    if X >= n and Y >= n:
        with np.errstate(all="ignore"):
            F[:, r:X - r, r:Y - r] = window_sums(window_sums(q, r, 1), r, 2) * inv
    return F


def valid_rect(shape, r, box=None):
    """(x0, y0, x1, y1), half-open: the valid cells r + 1 <= i <= X - 2 - r, r + 1 <= j <= Y - 2 - r, inside the box when one is given."""
    X, Y = shape
    box = (0, 0, X, Y) if box is None else box
    return max(box[0], r + 1), max(box[1], r + 1), min(box[2], X - 1 - r), min(box[3], Y - 1 - r)


def cell(c, l, r, m, n, two_dx):
    """(PI, ZF, K) from the eight filtered values c[0 .. 7] of the centre and F0 .. F2 of the four neighbours (arrays of any one shape)."""
    with np.errstate(all="ignore"):
        tuu, tuw, tww = c[3] - c[0] * c[0], c[4] - c[0] * c[1], c[5] - c[1] * c[1]
        su, sw = c[6] - c[0] * c[2], c[7] - c[1] * c[2]
        ux, uy = (r[0] - l[0]) / two_dx, (n[0] - m[0]) / two_dx
        wx, wy = (r[1] - l[1]) / two_dx, (n[1] - m[1]) / two_dx
        ox, oy = (r[2] - l[2]) / two_dx, (n[2] - m[2]) / two_dx
        s12 = 0.5 * (uy + wx)
        pi = -((tuu * ux + tww * wy) + (2.0 * tuw) * s12)
        zf = -(su * ox + sw * oy)
        k = 0.5 * (tuu + tww)
    return pi, zf, k


def stresses(F):
    """(tuu, tuw, tww) of the filtered planes."""
    with np.errstate(all="ignore"):
        return F[3] - F[0] * F[0], F[4] - F[0] * F[1], F[5] - F[1] * F[1]


def fluxes(F, r, dx):
    """(3, X, Y): PI, ZF, K at the valid cells of half-width r, +0 elsewhere."""
    K, X, Y = F.shape
    out = np.zeros((NSUM, X, Y), np.float64)
    x0, y0, x1, y1 = valid_rect((X, Y), r)
    if x0 < x1 and y0 < y1:
        sub = lambda di, dj, k=slice(None): F[k, x0 + di:x1 + di, y0 + dj:y1 + dj]
        three = slice(0, 3)
        out[:, x0:x1, y0:y1] = np.stack(cell(sub(0, 0), sub(-1, 0, three), sub(1, 0, three), sub(0, -1, three), sub(0, 1, three), 2.0 * dx))
    return out


def sample(v, mask, dx, half_widths, limit=None):
    """One sampling launch on the whole grid -> ([F of every half-width], (n_r, 3, X, Y) PI, ZF, K)."""
    q = base(v, mask, dx, limit)
    Fs = [filtered(q, r) for r in half_widths]
    return Fs, np.stack([fluxes(F, r, dx) for F, r in zip(Fs, half_widths)])


class State:
    """A fresh fs_flux_create."""

    def __init__(self, box, half_widths, dx, every, start):
        self.box, self.half_widths, self.dx, self.every, self.start = tuple(box), tuple(half_widths), dx, every, start
        nx, ny = box[2] - box[0], box[3] - box[1]
        self.sums = np.zeros((len(self.half_widths), NSUM, nx, ny), np.float64)
        self.filtered = [np.zeros((NQ, nx, ny), np.float64) for _ in self.half_widths]
        self.launches = self.samples = 0

    def launch(self, v, mask, limit=None):
        """One fs_flux_launch, sampling or not."""
        n = self.launches
        self.launches = n + 1
        if not (n + 1 > self.start and (n + 1 - self.start) % self.every == 0):
            return
        x0, y0, x1, y1 = self.box
        Fs, fl = sample(v, mask, self.dx, self.half_widths, limit)
        self.filtered = [F[:, x0:x1, y0:y1].copy() for F in Fs]
        with np.errstate(all="ignore"):
            self.sums = self.sums + fl[:, :, x0:x1, y0:y1]
        self.samples += 1
