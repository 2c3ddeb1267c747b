"""NumPy restatement of the energy spectra (csrc/fs_spec.h, include/fs_hip.h fs_spec_*) on SEPARATE float64 re / im arrays - arithmetic on
a complex dtype would round differently: the load, the staged radix-2 transform with the same tables, the detrend, the power, the
accumulation and the counters.  Every product and sum is one NumPy operation, rounded on its own, in the order the kernels take; the
butterflies of a stage are independent, so doing them all at once is the same transform.  Arrays are (X, Y) like every host array of the
product: cell (i, j) at [i, j]; planes are (Nx, Ny), bin (a, b) at [a, b]."""
import numpy as np
import vortex_ref as R


def bitrev(bits):
    """int64 (2^bits,): every index with its `bits` low bits reversed."""
    n = np.arange(1 << bits, dtype=np.int64)
    r = np.zeros_like(n)
    for b in range(bits):
        r = (r << 1) | ((n >> b) & 1)
    return r


def pairs(nq, h, N):
    """(i, k) of the butterflies q = 0 .. nq - 1 of the stage of half-width h over rows of N points laid end to end."""
    q = np.arange(nq, dtype=np.int64)
    m = q & (h - 1)
    return ((q - m) << 1) + m, m * (N // (2 * h))


def butterfly(are, aim, bre, bim, wre, wim):
    tre = wre * bre - wim * bim
    tim = wre * bim + wim * bre
    return are + tre, aim + tim, are - tre, aim - tim


def rows_transform(re, im, tw):
    """The transform of every row (last axis, N points) of re + i im; tw: (N / 2, 2) pairs (cos, -sin).  -> new (re, im)."""
    re, im = np.array(re, np.float64), np.array(im, np.float64)
    N = re.shape[-1]
    perm = bitrev(N.bit_length() - 1)
    re, im = re[..., perm], im[..., perm]      # element n is stored at the reversal of n
    h = 1
    with np.errstate(all="ignore"):
        while h < N:
            i, k = pairs(N // 2, h, N)
            a_re, a_im, b_re, b_im = butterfly(re[..., i], im[..., i], re[..., i + h], im[..., i + h], tw[k, 0], tw[k, 1])
            re[..., i], im[..., i], re[..., i + h], im[..., i + h] = a_re, a_im, b_re, b_im
            h *= 2
    return re, im


def load(v, mask, box, wx, wy, limit=None):
    """(re, im) (Nx, Ny): z = (u wx[a]) wy[b] + i (w wx[a]) wy[b], u and w through the deferred limit and promoted; wall cells +0."""
    x0, y0, x1, y1 = box
    lv = R.limited(v, limit)[x0:x1, y0:y1]
    wall = np.asarray(mask)[x0:x1, y0:y1] == 1
    with np.errstate(all="ignore"):
        re = (lv[..., 0].astype(np.float64) * wx[:, None]) * wy[None, :]
        im = (lv[..., 1].astype(np.float64) * wx[:, None]) * wy[None, :]
    return np.where(wall, 0.0, re), np.where(wall, 0.0, im)


def fft2(re, im, twx, twy):
    """Along x (axis 0), then along y (axis 1)."""
    r, i = rows_transform(re.T, im.T, twx)
    return rows_transform(r.T, i.T, twy)


def detrend(re, im, c1x, c1y):
    """Z'[a, b] = Z[a, b] - (Z00 c[a]) c[b] per component on the nine bins a, b in {0, 1, N - 1}."""
    re, im = re.copy(), im.copy()
    z_re, z_im = re[0, 0], im[0, 0]
    nx, ny = re.shape
    with np.errstate(all="ignore"):
        for a, ca in ((0, 1.0), (1, c1x), (nx - 1, c1x)):
            for b, cb in ((0, 1.0), (1, c1y), (ny - 1, c1y)):
                re[a, b] = re[a, b] - (z_re * np.float64(ca)) * np.float64(cb)
                im[a, b] = im[a, b] - (z_im * np.float64(ca)) * np.float64(cb)
    return re, im


def plane(v, mask, box, tabs, detrend_on, limit=None):
    """Z' of one sampling launch, (re, im); tabs = (wx, wy, twx, twy, c1x, c1y) of fs.spectra.tables."""
    wx, wy, twx, twy, c1x, c1y = tabs
    re, im = fft2(*load(v, mask, box, wx, wy, limit), twx, twy)
    return detrend(re, im, c1x, c1y) if detrend_on else (re, im)


def power_of(re, im):
    with np.errstate(all="ignore"):
        return re * re + im * im


class State:
    """A fresh fs_spec_create."""

    def __init__(self, box, tabs, detrend_on, every, start):
        self.box, self.tabs, self.detrend, self.every, self.start = tuple(box), tabs, bool(detrend_on), every, start
        nx, ny = box[2] - box[0], box[3] - box[1]
        self.power = np.zeros((nx, ny), np.float64)
        self.re, self.im = np.zeros((nx, ny), np.float64), np.zeros((nx, ny), np.float64)
        self.launches = self.samples = 0

    def launch(self, v, mask, limit=None):
        """One fs_spec_launch, sampling or not."""
        n = self.launches
        self.launches = n + 1
        if not (n + 1 > self.start and (n + 1 - self.start) % self.every == 0):
            return
        self.re, self.im = plane(v, mask, self.box, self.tabs, self.detrend, limit)
        with np.errstate(all="ignore"):
            self.power = self.power + power_of(self.re, self.im)
        self.samples += 1
