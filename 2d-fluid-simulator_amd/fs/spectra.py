"""Host side of the energy spectra (new; the reference has none): how the kinetic energy of the flow over a box of cells is spread over
wavenumbers.  The device (csrc/fs_spec.h, include/fs_hip.h fs_spec_*) transforms the windowed velocity (u + i w) wx wy with its own radix-2
FFT in double and accumulates the power |Z'|^2 of every bin by launches that ride the step; this module holds the tables it is given (the
windows, the twiddles: the device calls no sin or cos), the rider, the result dict and the NumPy helpers that work on it, without a device.
Driven by FluidSimulator.start_spectra / spectra / reset_spectra / stop_spectra / spectrum / box_fft.

Cross-spectra (csrc/fs_xspec.h, fs_xspec_*): the same transform of the packed plane a + i b of two of the seven quantities of the
distributions, split on the device into the transforms A and B of the two real fields; |A|^2, |B|^2 and A conj(B) of every bin are accumulated.
CrossSpectra is the rider, cross_result the dict; FluidSimulator.start_cross_spectra / cross_spectra / reset_cross_spectra /
stop_cross_spectra / cross_spectrum / pair_fft drive them.

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


# ---- cross-spectra of two quantities (csrc/fs_xspec.h) ----------------------------------------------------------------------------------------
def pair_names(qa, qb):
    """The names of a pair of quantity indices: (name_a, name_b), name_b None for qb = -1."""
    from .ride_ops import RideOps
    return RideOps.DIST_QUANTITIES[qa], (None if qb < 0 else RideOps.DIST_QUANTITIES[qb])


def upper_half(nx, ny):
    """bool (nx, ny): one bin of every mirror pair k, -k - 0 < a < nx / 2, and on the rows a = 0 and a = nx / 2 (their own mirrors along
    x) 0 < b < ny / 2; the bins that are their own mirrors belong to neither half."""
    a, b = np.arange(nx)[:, None], np.arange(ny)[None, :]
    return ((a > 0) & (a < nx // 2)) | (((a == 0) | (a == nx // 2)) & (b > 0) & (b < ny // 2))


def cross_result(sums, samples, sample_steps, box, quantities, window, detrend, dx):
    """The dict cross_spectra() / cross_spectrum() return from the accumulated planes `sums` (4, Nx, Ny) - Paa, Pbb, Cre, Cim with
    C = A conj(B), A and B the transforms of the windowed (detrended) quantities a and b - or (1, Nx, Ny) for one scalar, of `samples` samples.
    With norm = samples Nx Ny sum(wx^2) sum(wy^2):
        "quantities": (name_a, name_b or None);
        "spectrum_a", "spectrum_b": Paa / norm, Pbb / norm (Nx, Ny) - the sum over the bins is the window-weighted mean of a'^2; the enstrophy
            spectrum is half that of "vorticity";
        "co", "quad": Cre / norm, Cim / norm - the sum of "co" over the bins is the window-weighted mean of a' b';
        "kx", "ky": rad per length; "k", "Sa", "Sb", "Co", "Quad": the shell sums of the four planes (shell_spectrum).  "quad" is odd under
            k -> -k (the fields are real: C[-k] = conj C[k]) and a shell holds both bins of every such pair, so its plain sum over a shell is
            zero whatever the fields are: "Quad" sums twice the bins of the upper half (upper_half) instead - the sign convention of a
            one-sided spectrum, positive where b lags a along +x.  "Co" is even and the two ways of summing it agree;
        "coherence": (Co^2 + Quad^2) / (Sa Sb) per shell, NaN where the denominator is 0; "phase": atan2(Quad, Co) per shell;
        "samples", "sample_steps", "box", "window", "detrend", and the raw "sums".
    For one scalar "spectrum_b", "co", "quad", "Sb", "Co", "Quad", "coherence" and "phase" are None.

    The coherence of ONE bin of ONE sample is identically 1 (|A conj B|^2 = |A|^2 |B|^2): coherence means something only over shells or over
    many samples - which is why it is given per shell, from sums over the samples."""
    sums = np.asarray(sums, np.float64)
    planes, nx, ny = sums.shape
    wx, wy = window_table(nx, window), window_table(ny, window)
    norm = samples * (nx * ny * (wx * wx).sum() * (wy * wy).sum())
    with np.errstate(all="ignore"):
        scaled = sums / norm if samples else np.zeros_like(sums)
    kx, ky = wavenumbers(nx, ny, dx)
    k, Sa = shell_spectrum(scaled[0], kx, ky)
    out = {"quantities": tuple(quantities), "spectrum_a": scaled[0], "spectrum_b": None, "co": None, "quad": None, "kx": kx, "ky": ky, "k": k,
           "Sa": Sa, "Sb": None, "Co": None, "Quad": None, "coherence": None, "phase": None, "samples": int(samples),
           "sample_steps": sample_steps, "box": tuple(box), "window": window, "detrend": bool(detrend), "sums": sums}
    if planes > 1:
        Sb, Co = (shell_spectrum(scaled[n], kx, ky)[1] for n in (1, 2))
        Quad = shell_spectrum(np.where(upper_half(nx, ny), 2.0 * scaled[3], 0.0), kx, ky)[1]
        den = Sa * Sb
        with np.errstate(all="ignore"):
            coherence = np.where(den != 0, (Co * Co + Quad * Quad) / den, np.nan)
        out.update({"spectrum_b": scaled[1], "co": scaled[2], "quad": scaled[3], "Sb": Sb, "Co": Co, "Quad": Quad, "coherence": coherence,
                    "phase": np.arctan2(Quad, Co)})
    return out


class CrossSpectra(Rider):
    """The accumulated cross-spectrum of a FluidSimulator (start_cross_spectra): the device planes and their parameters.  No ring: room()
    is None and run() is not cut by it."""

    def __init__(self, dev, xspec, window):
        self.dev, self.xspec, self.window = dev, xspec, window
        self.every, self.start_step = int(xspec.every), int(xspec.start)
        self.base = 0              # samples taken before the last reset (sample_steps)

    @property
    def token(self):
        return ("xspec", self.xspec.serial)

    @property
    def quantities(self):
        return pair_names(self.xspec.qa, self.xspec.qb)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.xspec_launch(self.xspec, v, p)

    def free(self):
        self.dev.xspec_free(self.xspec)

    def sample_steps(self, samples):
        """The step (counted from start_cross_spectra, from 1) of every sample in the planes, int64 (samples,)."""
        k = self.base + np.arange(int(samples), dtype=np.int64)
        return self.start_step + (k + 1) * self.every

    def data(self):
        sums, _, samples = self.dev.xspec_read(self.xspec)
        return cross_result(sums, samples, self.sample_steps(samples), self.xspec.box, self.quantities, self.window, self.xspec.detrend,
                            self.xspec.dx)

    def reset(self):
        _, launches, _ = self.dev.xspec_read(self.xspec, sums=False)
        self.dev.xspec_reset(self.xspec)
        self.base = samples_after(launches, self.every, self.start_step)

    def checkpoint(self):
        sums, launches, samples = self.dev.xspec_get(self.xspec)
        return {"xspec.sums": sums, "xspec.launches": np.array(launches), "xspec.samples": np.array(samples), "xspec.base": np.array(self.base),
                "xspec.box": np.array(self.xspec.box, np.int64), "xspec.quantities": np.array([self.xspec.qa, self.xspec.qb], np.int64),
                "xspec.window": np.array(self.window), "xspec.detrend": np.array(self.xspec.detrend), "xspec.every": np.array(self.every),
                "xspec.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (box, quantities (name_a, name_b or None), window, detrend, every, start), or None."""
        if "xspec.sums" not in z:
            return None
        qa, qb = (int(q) for q in np.asarray(z["xspec.quantities"]))
        from .ride_ops import RideOps
        nq = len(RideOps.DIST_QUANTITIES)
        if not (0 <= qa < nq and -1 <= qb < nq):
            raise ValueError(f"the checkpoint's cross-spectrum names the quantities {qa}, {qb}: not indices of this build's quantities")
        return (tuple(int(b) for b in np.asarray(z["xspec.box"])), pair_names(qa, qb), str(np.asarray(z["xspec.window"])),
                bool(np.asarray(z["xspec.detrend"])), int(z["xspec.every"]), int(z["xspec.start"]))

    def restore(self, z):
        """Refused (ValueError) before any device work when the checkpoint's box, quantities, window, detrend, every or start_step are
        not the attached ones."""
        held = self.held(z)
        if held is None:
            raise ValueError("the checkpoint holds no cross-spectrum")
        box, quantities, window, detrend, every, start = held
        if box != tuple(self.xspec.box):
            raise ValueError(f"the checkpoint's cross-spectrum was accumulated over the box {box}, the attached one over {tuple(self.xspec.box)}")
        if quantities != self.quantities:
            raise ValueError(f"the checkpoint's cross-spectrum was accumulated for the pair {quantities}, the attached one for {self.quantities}")
        if window != self.window:
            raise ValueError(f"the checkpoint's cross-spectrum was accumulated with the window {window!r}, the attached one with {self.window!r}")
        if detrend != bool(self.xspec.detrend):
            raise ValueError(f"the checkpoint's cross-spectrum was accumulated with detrend={detrend}, the attached one with "
                             f"detrend={bool(self.xspec.detrend)}")
        if (every, start) != (self.every, self.start_step):
            raise ValueError(f"the checkpoint's cross-spectrum samples every {every} from {start}, the attached one every {self.every} from "
                             f"{self.start_step}")
        self.dev.xspec_set(self.xspec, z["xspec.sums"], int(z["xspec.launches"]), int(z["xspec.samples"]))
        self.base = int(z["xspec.base"])
        return int(z["xspec.samples"])


def create_cross(dev, box, pair, dx, window, detrend, every=1, start=0):
    """The device object of a box, a pair and a window: the tables built here, handed to dev.xspec_create."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    box = dev.spec_box(box)
    dev.xspec_pair(pair)
    wx, wy, twx, twy, c1x, c1y = tables(box[2] - box[0], box[3] - box[1], window)
    return dev.xspec_create(box, pair, dx, wx, wy, twx, twy, c1x, c1y, bool(detrend), every, start)
