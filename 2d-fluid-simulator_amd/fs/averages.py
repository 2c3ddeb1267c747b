"""Host side of the time averages (new; the reference has none): the sampling rule, the derivation of means, Reynolds stresses and rms
pressure from the seven sums, and the recirculation length of a mean wake.  Pure NumPy: testable without a device.

The accumulation itself is a device launch per step (csrc/fs_mean.h, include/fs_hip.h fs_mean_*), driven by
FluidSimulator.start_averaging / averages / reset_averages / stop_averaging."""
import numpy as np

from .riders import Rider, is_sampling_launch, samples_after      # noqa: F401 (the sampling rule: re-exported)

FLUID, WALL = 0, 1
# plane order of fs_mean_read / fs_mean_write
SUMS = ("S_u", "S_w", "S_p", "S_uu", "S_ww", "S_uw", "S_pp")


def derive_averages(sums, samples, mask=None):
    """The averages from the seven sums (array (7, X, Y), or a sequence of seven (X, Y) arrays in the order SUMS) of `samples` samples ->
    dict of float64 (X, Y) arrays: u, w, p (means S_a / n), uu, ww, uw (central second moments S_ab / n - mean_a * mean_b, evaluated in this
    order), p_rms (sqrt(max(S_pp / n - p * p, 0))) and tke (0.5 * (uu + ww)).  With `mask`, wall cells (mask 1) hold 0 in every array.
    samples == 0 raises ValueError."""
    n = int(samples)
    if n <= 0:
        raise ValueError("no samples accumulated yet")
    s_u, s_w, s_p, s_uu, s_ww, s_uw, s_pp = (np.asarray(s, np.float64) for s in sums)
    nf = np.float64(n)
    u, w, p = s_u / nf, s_w / nf, s_p / nf
    uu = s_uu / nf - u * u
    ww = s_ww / nf - w * w
    uw = s_uw / nf - u * w
    p_rms = np.sqrt(np.maximum(s_pp / nf - p * p, 0.0))
    out = {"u": u, "w": w, "p": p, "uu": uu, "ww": ww, "uw": uw, "p_rms": p_rms, "tke": 0.5 * (uu + ww)}
    if mask is not None:
        wall = np.asarray(mask) == WALL
        for a in out.values():
            a[wall] = 0.0
    return out


def recirculation_length(mean_u, mask, body_box, dx):
    """Length of the mean recirculation bubble behind the body in `body_box` = (x0, y0, x1, y1) (global cells, half-open): on the row
    through the middle of the box, the distance from the box's downstream face (x = x1) to the first fluid cell behind it from which
    mean_u > 0 holds on every fluid cell (mask 0) of the rest of the row, measured to that cell's upstream edge: (x - x1) * dx.  0.0 when
    the flow never reverses on that row; nan when there is no such cell (the reversed flow reaches the end of the row)."""
    mean_u, mask = np.asarray(mean_u), np.asarray(mask)
    x0, y0, x1, y1 = (int(b) for b in body_box)
    X = mean_u.shape[0]
    row = (y0 + y1) // 2
    if not (0 <= x1 <= X and 0 <= row < mean_u.shape[1]):
        raise ValueError(f"body box {body_box} lies outside the domain")
    xs = np.arange(x1, X)
    fluid = mask[x1:, row] == FLUID
    ok = (mean_u[x1:, row] > 0) | ~fluid        # (cells that are not fluid do not break the run)
    bad = np.nonzero(~ok)[0]
    first = 0 if len(bad) == 0 else bad[-1] + 1
    cand = np.nonzero(fluid[first:])[0]
    if len(cand) == 0:
        return float("nan")
    x = xs[first + cand[0]]
    return float((x - x1) * dx)


class Averager(Rider):
    """One time average of a FluidSimulator (start_averaging): the device accumulator and its parameters."""

    def __init__(self, dev, mean, every, start_step):
        self.dev, self.mean, self.every, self.start_step = dev, mean, int(every), int(start_step)

    @property
    def token(self):
        return ("mean", self.mean.serial)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.mean_accumulate(self.mean, v, p)

    def free(self):
        self.dev.mean_free(self.mean)

    def checkpoint(self):
        sums, launches, samples = self.dev.mean_read(self.mean)
        return {"mean.sums": sums, "mean.launches": np.array(launches), "mean.samples": np.array(samples),
                "mean.every": np.array(self.every), "mean.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (every, start), or None."""
        return (int(z["mean.every"]), int(z["mean.start"])) if "mean.sums" in z else None

    def restore(self, z):
        self.dev.mean_write(self.mean, z["mean.sums"], int(z["mean.launches"]), int(z["mean.samples"]))
        return int(z["mean.samples"])
