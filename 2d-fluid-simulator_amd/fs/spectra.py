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

from .riders import BOX, CountedRider, Param

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


WINDOW = Param("window", np.array, lambda a: str(np.asarray(a)), "{theirs} accumulated with the window {0!r}, {ours} with {1!r}")
DETREND = Param("detrend", np.array, lambda a: bool(np.asarray(a)), "{theirs} accumulated with detrend={0}, {ours} with detrend={1}")


class Spectra(CountedRider):
    """The accumulated spectrum of a FluidSimulator (start_spectra): the device planes and their parameters.
    held(z) -> (box, window, detrend, every, start), or None."""
    kind, payload, noun = "spec", "power", "spectrum"
    params = (BOX, WINDOW, DETREND)
    refuses_missing = False

    def __init__(self, dev, spec, window, dx):
        super().__init__(dev, spec, spec.every, spec.start)
        self.spec, self.window, self.dx = spec, window, float(dx)

    def attached(self):
        return tuple(self.spec.box), self.window, bool(self.spec.detrend)

    def launch(self, sim):
        self.dev.spec_launch(self.spec, sim._solver.get_fields()[0])

    def data(self):
        sums, _, samples = self.dev.spec_read(self.spec)
        return result(sums, samples, self.sample_steps(samples), self.spec.box, self.window, self.spec.detrend, self.dx)


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


def _pair_indices(names):
    from .ride_ops import RideOps
    return np.array([-1 if n is None else RideOps.DIST_QUANTITIES.index(n) for n in names], np.int64)


def _pair_held(a):
    from .ride_ops import RideOps
    qa, qb = (int(q) for q in np.asarray(a))
    nq = len(RideOps.DIST_QUANTITIES)
    if not (0 <= qa < nq and -1 <= qb < nq):
        raise ValueError(f"the checkpoint's cross-spectrum names the quantities {qa}, {qb}: not indices of this build's quantities")
    return pair_names(qa, qb)


class CrossSpectra(CountedRider):
    """The accumulated cross-spectrum of a FluidSimulator (start_cross_spectra): the device planes and their parameters.
    held(z) -> (box, quantities (name_a, name_b or None), window, detrend, every, start), or None."""
    kind, payload, noun = "xspec", "sums", "cross-spectrum"
    params = (BOX, Param("quantities", _pair_indices, _pair_held, "{theirs} accumulated for the pair {0}, {ours} for {1}"), WINDOW, DETREND)

    def __init__(self, dev, xspec, window):
        super().__init__(dev, xspec, xspec.every, xspec.start)
        self.xspec, self.window = xspec, window
        self.quantities = pair_names(xspec.qa, xspec.qb)

    def attached(self):
        return tuple(self.xspec.box), self.quantities, self.window, bool(self.xspec.detrend)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.xspec_launch(self.xspec, v, p)

    def data(self):
        sums, _, samples = self.dev.xspec_read(self.xspec)
        return cross_result(sums, samples, self.sample_steps(samples), self.xspec.box, self.quantities, self.window, self.xspec.detrend,
                            self.xspec.dx)


def create_cross(dev, box, pair, dx, window, detrend, every=1, start=0):
    """The device object of a box, a pair and a window: the tables built here, handed to dev.xspec_create."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    box = dev.spec_box(box)
    dev.xspec_pair(pair)
    wx, wy, twx, twy, c1x, c1y = tables(box[2] - box[0], box[3] - box[1], window)
    return dev.xspec_create(box, pair, dx, wx, wy, twx, twy, c1x, c1y, bool(detrend), every, start)
