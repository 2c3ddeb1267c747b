"""Host side of the energy spectra (new; the reference has none): how the kinetic energy of the flow over a box of cells is spread over
wavenumbers.  The device (csrc/fs_spec.h, include/fs_hip.h fs_spec_*) transforms the windowed velocity (u + i w) wx wy with its own radix-2
FFT in double and accumulates the power |Z'|^2 of every bin by launches that ride the step; this module holds the tables it is given (the
windows, the twiddles: the device calls no sin or cos), the rider, the result dict and the NumPy helpers that work on it, without a device.
Driven by FluidSimulator.start_spectra / spectra / reset_spectra / stop_spectra / spectrum / box_fft.

One complex transform carries both components: with Z = FFT2(u + i w), U[k] = (Z[k] + conj(Z[-k])) / 2 and W[k] = (Z[k] - conj(Z[-k])) / 2i
(split), so |U[k]|^2 + |W[k]|^2 = (|Z[k]|^2 + |Z[-k]|^2) / 2.  Planes are (Nx, Ny), indexed like np.fft.fft2 of an array whose first axis is x."""
import numpy as np

from .riders import Rider, samples_after

WINDOWS = ("hann", "boxcar")


def window_table(n, kind):
    """The window of one axis, float64 (n,): "hann" - periodic, 0.5 - 0.5 cos(2 pi m / n) - or "boxcar" (ones)."""
    if kind not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {kind!r}")
    n = int(n)
    if kind == "boxcar":
        return np.ones(n, np.float64)
    return 0.5 - 0.5 * _cos_sin(n, n)[0]


def _cos_sin(n, count):
    """cos and sin of 2 pi m / n for m = 0 .. count - 1, float64, evaluated in extended precision and rounded once."""
    pi = np.longdouble(4) * np.arctan(np.longdouble(1))
    ang = 2 * pi * np.arange(count, dtype=np.longdouble) / np.longdouble(n)
    return np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)


def twiddles(n):
    """The twiddle table of one axis, float64 (n / 2, 2): (cos, -sin) of 2 pi k / n."""
    c, s = _cos_sin(int(n), int(n) // 2)
    return np.ascontiguousarray(np.stack([c, -s], axis=1))


def detrend_pair(window):
    """c1 of the detrend for a window: its transform at bins +-1 over that at bin 0 (hann: W[0] = n / 2, W[+-1] = -n / 4 -> -0.5; boxcar: 0)."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    return -0.5 if window == "hann" else 0.0


def tables(nx, ny, window):
    """Everything spec_create takes for a box of nx x ny cells: (wx, wy, twx, twy, c1x, c1y)."""
    c1 = detrend_pair(window)
    return window_table(nx, window), window_table(ny, window), twiddles(nx), twiddles(ny), c1, c1


def wavenumbers(nx, ny, dx):
    """(kx (nx,), ky (ny,)) in rad per length: 2 pi fftfreq(n, dx)."""
    return 2.0 * np.pi * np.fft.fftfreq(int(nx), float(dx)), 2.0 * np.pi * np.fft.fftfreq(int(ny), float(dx))


def mirrored(P):
    """P[-k]: the plane read at the negated wavenumber indices, modulo the sides."""
    P = np.asarray(P)
    return P[(-np.arange(P.shape[0])) % P.shape[0]][:, (-np.arange(P.shape[1])) % P.shape[1]]


def split(Z):
    """(U, W): the transforms of the two real components from the packed plane Z = FFT2(u + i w)."""
    Z = np.asarray(Z, np.complex128)
    Zm = np.conj(mirrored(Z))
    return 0.5 * (Z + Zm), -0.5j * (Z - Zm)


def shell_spectrum(energy, kx, ky):
    """(k, E): the bins of `energy` (nx, ny) gathered in shells |k| of width dk = the smaller fundamental wavenumber, shell s holding the
    bins with floor(|k| / dk + 0.5) == s at k = s dk; every shell summed and divided by dk, so that sum(E) * dk == energy.sum()."""
    energy, kx, ky = np.asarray(energy, np.float64), np.asarray(kx, np.float64), np.asarray(ky, np.float64)
    dk = min(np.abs(kx[1]), np.abs(ky[1]))
    mag = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
    shell = np.floor(mag / dk + 0.5).astype(np.int64)
    E = np.bincount(shell.ravel(), weights=energy.ravel()) / dk
    return dk * np.arange(len(E), dtype=np.float64), E


def line_spectrum(energy, axis):
    """The energy summed over the OTHER axis: (n,) along `axis` (0: kx, 1: ky), indexed like fftfreq."""
    if axis not in (0, 1):
        raise ValueError(f"axis must be 0 or 1, got {axis!r}")
    return np.asarray(energy, np.float64).sum(axis=1 - axis)


def slope(k, E, k_lo, k_hi):
    """The exponent of a power law through E(k) on k_lo <= k <= k_hi: a least-squares line in log-log over the points with E > 0."""
    k, E = np.asarray(k, np.float64), np.asarray(E, np.float64)
    sel = (k >= k_lo) & (k <= k_hi) & (k > 0) & (E > 0)
    if sel.sum() < 2:
        raise ValueError("a slope needs two points with E > 0 inside [k_lo, k_hi]")
    return float(np.polyfit(np.log(k[sel]), np.log(E[sel]), 1)[0])


def result(sums, samples, sample_steps, box, window, detrend, dx):
    """The dict spectra() / spectrum() return from the accumulated plane `sums` (nx, ny) of `samples` samples."""
    sums = np.asarray(sums, np.float64)
    nx, ny = sums.shape
    with np.errstate(all="ignore"):
        power = 0.5 * (sums + mirrored(sums)) / samples if samples else np.zeros_like(sums)
    wx, wy = window_table(nx, window), window_table(ny, window)
    energy = 0.5 * power / (nx * ny * (wx * wx).sum() * (wy * wy).sum())
    kx, ky = wavenumbers(nx, ny, dx)
    k, E = shell_spectrum(energy, kx, ky)
    return {"power": power, "energy": energy, "kx": kx, "ky": ky, "k": k, "E": E, "samples": int(samples), "sample_steps": sample_steps,
            "box": tuple(box), "window": window, "detrend": bool(detrend), "sums": sums}


class Spectra(Rider):
    """The accumulated spectrum of a FluidSimulator (start_spectra): the device planes and their parameters.  No ring: room() is None
    and run() is not cut by it."""

    def __init__(self, dev, spec, window, dx):
        self.dev, self.spec, self.window, self.dx = dev, spec, window, float(dx)
        self.every, self.start_step = int(spec.every), int(spec.start)
        self.base = 0              # samples taken before the last reset (sample_steps)

    @property
    def token(self):
        return ("spec", self.spec.serial)

    def launch(self, sim):
        self.dev.spec_launch(self.spec, sim._solver.get_fields()[0])

    def free(self):
        self.dev.spec_free(self.spec)

    def sample_steps(self, samples):
        """The step (counted from start_spectra, from 1) of every sample in the plane, int64 (samples,)."""
        k = self.base + np.arange(int(samples), dtype=np.int64)
        return self.start_step + (k + 1) * self.every

    def data(self):
        sums, _, samples = self.dev.spec_read(self.spec)
        return result(sums, samples, self.sample_steps(samples), self.spec.box, self.window, self.spec.detrend, self.dx)

    def reset(self):
        _, launches, _ = self.dev.spec_read(self.spec, power=False)
        self.dev.spec_reset(self.spec)
        self.base = samples_after(launches, self.every, self.start_step)

    def checkpoint(self):
        power, launches, samples = self.dev.spec_get(self.spec)
        return {"spec.power": power, "spec.launches": np.array(launches), "spec.samples": np.array(samples), "spec.base": np.array(self.base),
                "spec.box": np.array(self.spec.box, np.int64), "spec.window": np.array(self.window), "spec.detrend": np.array(self.spec.detrend),
                "spec.every": np.array(self.every), "spec.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (box, window, detrend, every, start), or None."""
        if "spec.power" not in z:
            return None
        return (tuple(int(b) for b in np.asarray(z["spec.box"])), str(np.asarray(z["spec.window"])), bool(np.asarray(z["spec.detrend"])),
                int(z["spec.every"]), int(z["spec.start"]))

    def restore(self, z):
        """Refused (ValueError) before any device work when the checkpoint's box, window, detrend, every or start_step are not the
        attached ones."""
        box, window, detrend, every, start = self.held(z)
        if box != tuple(self.spec.box):
            raise ValueError(f"the checkpoint's spectrum was accumulated over the box {box}, the attached one over {tuple(self.spec.box)}")
        if window != self.window:
            raise ValueError(f"the checkpoint's spectrum was accumulated with the window {window!r}, the attached one with {self.window!r}")
        if detrend != bool(self.spec.detrend):
            raise ValueError(f"the checkpoint's spectrum was accumulated with detrend={detrend}, the attached one with detrend={bool(self.spec.detrend)}")
        if (every, start) != (self.every, self.start_step):
            raise ValueError(f"the checkpoint's spectrum samples every {every} from {start}, the attached one every {self.every} from {self.start_step}")
        self.dev.spec_set(self.spec, z["spec.power"], int(z["spec.launches"]), int(z["spec.samples"]))
        self.base = int(z["spec.base"])
        return int(z["spec.samples"])


def create(dev, box, window, detrend, every=1, start=0):
    """The device object of a box and a window: the tables built here, handed to dev.spec_create."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    box = dev.spec_box(box)
    wx, wy, twx, twy, c1x, c1y = tables(box[2] - box[0], box[3] - box[1], window)
    return dev.spec_create(box, wx, wy, twx, twy, c1x, c1y, bool(detrend), every, start)
