"""Host side of the harmonic flow modes (new; the reference has none): the phase steps the device rotates its phasors by, the Gram matrix of
the basis that was actually applied, the least-squares fit of mean, cosine and sine coefficients per cell, and the reconstruction of the flow at
a phase of the cycle.  Pure NumPy apart from the rider class: testable without a device.

The device (csrc/fs_modes.h, include/fs_hip.h fs_modes_*) keeps, for K frequencies and the basis b = [1, c_1, s_1, ..., c_K, s_K] of B = 1 + 2K
entries, the planes R[a][j] = sum over the samples of x_a * b_j for a in FIELDS, and the Gram matrix G[i][j] = sum of b_i * b_j.  A run never holds
a whole number of periods and the rotated phasors drift by rounding, so nothing here assumes orthogonality: the model
x(t) ~ mean + sum_k cos_k cos(theta_k) + sin_k sin(theta_k) is fitted by solving G X = R, one B x B system shared by all cells, with the phasors
that were applied.  Driven by FluidSimulator.start_modes / modes / mode_fields / reset_modes / stop_modes."""
import numpy as np

from .riders import Rider

WALL = 1
FIELDS = ("u", "w", "p")      # plane a * B + j of fs_modes_read: field a, basis entry j
MODES_MAX_FREQ = 4


def check_frequencies(frequencies):
    """-> float64 (K,): 1 to MODES_MAX_FREQ distinct, finite, positive frequencies (ValueError otherwise)."""
    f = np.atleast_1d(np.asarray(frequencies, np.float64))
    if f.ndim != 1 or len(f) < 1:
        raise ValueError("frequencies must hold at least one value")
    if len(f) > MODES_MAX_FREQ:
        raise ValueError(f"at most MODES_MAX_FREQ = {MODES_MAX_FREQ} frequencies, got {len(f)}")
    if not np.all(np.isfinite(f)) or not np.all(f > 0.0):
        raise ValueError("frequencies must be finite and positive")
    if len(np.unique(f)) != len(f):
        raise ValueError("frequencies must be distinct")
    return f


def phasor_steps(frequencies, every, dt):
    """(cd, sd), float64 (K,) each: cosine and sine of the phase step per sample delta_k = 2 pi f_k every dt, the constants of the device's
    rotation c' = c cd - s sd, s' = s cd + c sd.  ValueError when a frequency reaches the Nyquist limit of the sampling, f_k every dt >= 0.5."""
    f = check_frequencies(frequencies)
    every, dt = int(every), float(dt)
    if every < 1 or not dt > 0.0:
        raise ValueError("every must be >= 1 and dt > 0")
    per_sample = f * every * dt
    if np.any(per_sample >= 0.5):
        k = int(np.argmax(per_sample >= 0.5))
        raise ValueError(f"frequency {f[k]} reaches the Nyquist limit of one sample every {every} steps of dt = {dt} (f every dt = {per_sample[k]:.4g} >= 0.5)")
    delta = 2.0 * np.pi * f * every * dt
    return np.cos(delta), np.sin(delta)


def basis_size(nfreq):
    return 1 + 2 * int(nfreq)


def phasors(scalars, nfreq):
    """-> (c, s), float64 (K,) each: the phasors the NEXT sample will carry."""
    sc = np.asarray(scalars, np.float64)
    return sc[0:2 * nfreq:2].copy(), sc[1:2 * nfreq:2].copy()


def gram_matrix(scalars, nfreq):
    """The symmetric B x B Gram matrix from the scalars of fs_modes_read (2K phasor entries, then the upper triangle, row major)."""
    nfreq = int(nfreq)
    B = basis_size(nfreq)
    sc = np.asarray(scalars, np.float64)
    if sc.shape != (2 * nfreq + B * (B + 1) // 2,):
        raise ValueError(f"expected {2 * nfreq + B * (B + 1) // 2} scalars for {nfreq} frequencies, got shape {sc.shape}")
    G = np.zeros((B, B))
    iu = np.triu_indices(B)
    G[iu] = sc[2 * nfreq:]
    G[(iu[1], iu[0])] = sc[2 * nfreq:]
    return G


def samples_of(scalars, nfreq):
    """The number of samples: G[0][0], the sum of 1 * 1."""
    return int(round(float(np.asarray(scalars, np.float64)[2 * int(nfreq)])))


def _inverse(G):
    # rows and columns scaled to a unit diagonal first: G grows with the sample count, the scaled matrix has a condition number of order 1
    d = np.sqrt(np.diag(G))
    return np.linalg.inv(G / np.outer(d, d)) / np.outer(d, d)


def _apply(W, R):
    """W R with R (B, cells), one cell at a time in the same order of operations: a cell's result does not depend on how many cells there
    are (a slab's rows give the bits of the whole domain's)."""
    out = np.zeros_like(R)
    for i in range(len(W)):
        for j in range(len(W)):
            out[i] = out[i] + W[i, j] * R[j]
    return out


def fit(sums, scalars, nfreq, mask=None):
    """Least-squares coefficients per cell from the planes `sums` (3 B, ...) and the scalars -> {field: {"mean": (...), "cos", "sin",
    "amplitude", "phase": (K, ...)}} for field in FIELDS, float64: the sampled signal is mean + sum_k cos[k] cos(theta_k) + sin[k] sin(theta_k)
    = mean + sum_k amplitude[k] cos(theta_k - phase[k]), theta_k = 2 pi f_k (t - t_0) with t_0 the time of the first sample; amplitude = hypot(cos,
    sin), phase = atan2(sin, cos).  With `mask`, wall cells (mask 1) hold 0 in every array.  ValueError while there are fewer samples than the
    B unknowns."""
    nfreq = int(nfreq)
    B = basis_size(nfreq)
    sums = np.asarray(sums, np.float64)
    if sums.shape[0] != 3 * B:
        raise ValueError(f"expected {3 * B} planes for {nfreq} frequencies, got {sums.shape[0]}")
    G = gram_matrix(scalars, nfreq)
    n = samples_of(scalars, nfreq)
    if n < B:
        raise ValueError(f"{n} samples do not determine the {B} coefficients of {nfreq} frequencies yet")
    cell = sums.shape[1:]
    W = _inverse(G)
    wall = None if mask is None else np.asarray(mask) == WALL
    out = {}
    for a, name in enumerate(FIELDS):
        X = _apply(W, sums[a * B:(a + 1) * B].reshape(B, -1)).reshape((B,) + cell)
        if wall is not None:
            X[:, wall] = 0.0
        c, s = X[1::2], X[2::2]
        out[name] = {"mean": X[0].copy(), "cos": c.copy(), "sin": s.copy(), "amplitude": np.hypot(c, s), "phase": np.arctan2(s, c)}
    return out


def _unit(nfreq, phases):
    """e(phi) = [1, cos phi_1, sin phi_1, ...]; a phase of None leaves that frequency out (both entries 0); phases=None: the mean alone."""
    e = np.zeros(basis_size(nfreq))
    e[0] = 1.0
    if phases is None:
        return e
    phases = list(np.atleast_1d(np.asarray(phases, object)))
    if len(phases) != nfreq:
        raise ValueError(f"expected {nfreq} phases (None: leave the frequency out), got {len(phases)}")
    for k, ph in enumerate(phases):
        if ph is not None:
            e[1 + 2 * k], e[2 + 2 * k] = np.cos(float(ph)), np.sin(float(ph))
    return e


def reconstruct_weights(scalars, nfreq, phases):
    """float64 (B,): w = G^-1 e(phases).  sum_j w[j] * plane[a B + j] is the fitted value of field a at those phases - what fs_modes_combine
    evaluates on the device (the same weights for the three fields)."""
    G = gram_matrix(scalars, nfreq)
    n = samples_of(scalars, nfreq)
    if n < basis_size(nfreq):
        raise ValueError(f"{n} samples do not determine the {basis_size(nfreq)} coefficients of {nfreq} frequencies yet")
    return _apply(_inverse(G), _unit(nfreq, phases)[:, None])[:, 0]


def reconstruct(fitted, phases):
    """{field: array}: mean + sum_k cos[k] cos(phases[k]) + sin[k] sin(phases[k]) from the output of fit(), on the host."""
    out = {}
    for name in FIELDS:
        f = fitted[name]
        e = _unit(len(f["cos"]), phases)
        x = f["mean"] * e[0]
        for k in range(len(f["cos"])):
            x = x + f["cos"][k] * e[1 + 2 * k] + f["sin"][k] * e[2 + 2 * k]
        out[name] = x
    return out


class Modes(Rider):
    """The harmonic modes of a FluidSimulator (start_modes): the device accumulator and its parameters."""

    def __init__(self, dev, modes, frequencies, every, start_step):
        self.dev, self.modes, self.every, self.start_step = dev, modes, int(every), int(start_step)
        self.frequencies = np.array(frequencies, np.float64)

    @property
    def token(self):
        return ("modes", self.modes.serial)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.modes_accumulate(self.modes, v, p)

    def free(self):
        self.dev.modes_free(self.modes)

    def checkpoint(self):
        sums, scalars, launches, samples = self.dev.modes_read(self.modes)
        return {"modes.sums": sums, "modes.scalars": scalars, "modes.launches": np.array(launches), "modes.samples": np.array(samples),
                "modes.frequencies": self.frequencies.copy(), "modes.every": np.array(self.every), "modes.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (frequencies, every, start), or None."""
        if "modes.sums" not in z:
            return None
        return (tuple(float(f) for f in z["modes.frequencies"]), int(z["modes.every"]), int(z["modes.start"]))

    def restore(self, z):
        self.dev.modes_write(self.modes, z["modes.sums"], z["modes.scalars"], int(z["modes.launches"]), int(z["modes.samples"]))
        return int(z["modes.samples"])
