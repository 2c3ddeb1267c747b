"""NumPy restatement of the cross-spectra (csrc/fs_xspec.h, include/fs_hip.h fs_xspec_*) on SEPARATE float64 re / im arrays, built on the
restatement of the energy spectra (tests/spec_ref.py: the staged transform, the detrend): the load of a pair of quantities through the
restatements of the distributions and the vortex identification (tests/dist_ref.py values, tests/vortex_ref.py), the split of the packed plane
and the accumulation, every product and sum one NumPy operation in the order the kernel takes.  Arrays are (X, Y) like every host array of
the product; planes are (Nx, Ny), bin (a, b) at [a, b]."""
import numpy as np

import dist_ref as D
import spec_ref as S

QUANTITIES = D.QUANTITIES
NPLANE = 4


def mirrored(P):
    """P read at the mirror bin ((Nx - a) mod Nx, (Ny - b) mod Ny)."""
    return P[(-np.arange(P.shape[0])) % P.shape[0]][:, (-np.arange(P.shape[1])) % P.shape[1]]


def selected(q, mask):
    """Where quantity index q contributes: vorticity, q, swirl on fluid cells, the others everywhere but inside the walls."""
    mask = np.asarray(mask)
    return mask == 0 if q >= 4 else mask != 1


def load(qa, qb, v, p, mask, dx, box, wx, wy, limit=None):
    """(re, im) (Nx, Ny): z = (a wx[i]) wy[j] + i (b wx[i]) wy[j]; +0 where the quantity does not contribute, im +0 throughout for qb = -1."""
    x0, y0, x1, y1 = box

    def side(q):
        if q < 0:
            return np.zeros((x1 - x0, y1 - y0), np.float64)
        val = D.values(QUANTITIES[q], v, p, mask, dx, limit)[x0:x1, y0:y1]
        with np.errstate(all="ignore"):
            z = (val * wx[:, None]) * wy[None, :]
        return np.where(selected(q, mask)[x0:x1, y0:y1], z, 0.0)
    return side(qa), side(qb)


def plane(qa, qb, v, p, mask, dx, box, tabs, detrend_on, limit=None):
    """Z' of one sampling launch, (re, im); tabs = (wx, wy, twx, twy, c1x, c1y) of fs.spectra.tables."""
    wx, wy, twx, twy, c1x, c1y = tabs
    re, im = S.fft2(*load(qa, qb, v, p, mask, dx, box, wx, wy, limit), twx, twy)
    return S.detrend(re, im, c1x, c1y) if detrend_on else (re, im)


def split_products(re, im):
    """(Paa, Pbb, Cre, Cim) of one sample from Z' = re + i im, in the kernel's order."""
    mre, mim = mirrored(re), mirrored(im)
    with np.errstate(all="ignore"):
        are, aim = 0.5 * (re + mre), 0.5 * (im - mim)
        bre, bim = 0.5 * (im + mim), 0.5 * (mre - re)
        return are * are + aim * aim, bre * bre + bim * bim, are * bre + aim * bim, aim * bre - are * bim


def accumulate(sums, re, im):
    """sums (4 or 1, Nx, Ny) + the products of Z' -> the new sums."""
    prods = split_products(re, im)[:sums.shape[0]]
    with np.errstate(all="ignore"):
        return np.stack([s + x for s, x in zip(sums, prods)])


class State:
    """A fresh fs_xspec_create."""

    def __init__(self, box, qa, qb, dx, tabs, detrend_on, every, start):
        self.box, self.qa, self.qb, self.dx, self.tabs = tuple(box), qa, qb, dx, tabs
        self.detrend, self.every, self.start = bool(detrend_on), every, start
        nx, ny = box[2] - box[0], box[3] - box[1]
        self.sums = np.zeros((NPLANE if qb >= 0 else 1, nx, ny), np.float64)
        self.re, self.im = np.zeros((nx, ny), np.float64), np.zeros((nx, ny), np.float64)
        self.launches = self.samples = 0

    def launch(self, v, p, mask, limit=None):
        """One fs_xspec_launch, sampling or not."""
        n = self.launches
        self.launches = n + 1
        if not (n + 1 > self.start and (n + 1 - self.start) % self.every == 0):
            return
        self.re, self.im = plane(self.qa, self.qb, v, p, mask, self.dx, self.box, self.tabs, self.detrend, limit)
        self.sums = accumulate(self.sums, self.re, self.im)
        self.samples += 1
