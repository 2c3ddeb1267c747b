"""Host side of the field distributions (new; the reference has none): histograms, joint histograms and quantiles of u, w, p, the speed, the
vorticity and the vortex criteria over the fluid cells.  The device (csrc/fs_dist.h, include/fs_hip.h fs_dist_*) counts into 64-bit integer
tables - accumulated over a run by launches that ride the step - and finds exact order statistics by a radix select; this module is the
rider, the result dicts and the NumPy helpers that work on them, without a device.  Driven by FluidSimulator.start_distributions /
distributions / reset_distributions / stop_distributions / histogram / quantile / order_statistics.

The bin rule is the device's (csrc/fs_dist.h dist_bin), not np.histogram's: bin k of a range [lo, hi) of B bins holds the values x with
floor((x - lo) * (B / (hi - lo))) == k, the last bin also those that scale to B exactly; x >= hi is `above`.  "edges" are the nominal
lo + k (hi - lo) / B."""
import math

import numpy as np

from .riders import CountedRider, Param

METHODS = ("lower", "higher", "nearest", "linear")


def edges(lo, hi, bins):
    """The nominal bin edges, float64 (bins + 1,): lo and hi exactly at the ends."""
    e = lo + (hi - lo) * (np.arange(bins + 1, dtype=np.float64) / bins)
    e[0], e[-1] = lo, hi
    return e


def result(dev, channel, counts, tails, samples, sample_steps):
    """The dict distributions() / histogram() return for one channel (ride_ops.DistChannel) from what dist_read returned."""
    names = dev.DIST_QUANTITIES
    out = {"counts": counts, "nan": int(tails[2]), "edges": edges(channel.lo, channel.hi, channel.bins), "samples": int(samples),
           "sample_steps": sample_steps, "box": tuple(channel.box)}
    if channel.joint:
        out["quantity"] = (names[channel.quantity], names[channel.quantity_b])
        out["outside"] = int(tails[0])
        out["edges_b"] = edges(channel.lo_b, channel.hi_b, channel.bins_b)
    else:
        out["quantity"] = names[channel.quantity]
        out["below"], out["above"] = int(tails[0]), int(tails[1])
    return out


def rank_pair(n, q):
    """The two order statistics a quantile q of n values lies between: (k, k + 1 clipped to n - 1, the fractional part g) of (n - 1) * q,
    evaluated as a Python float - the ranks np.quantile(..., method="lower" / "higher") picks."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must lie in [0, 1], got {q}")
    pos = (n - 1) * q
    k = int(math.floor(pos))
    return k, min(k + 1, n - 1), pos - k


def interpolate(a, b, g, method):
    """The quantile from its two order statistics a <= b and the fractional part g: "lower" a, "higher" b (a when g == 0), "nearest" the
    closer one (a at g == 0.5), "linear" a + (b - a) * g."""
    if method == "lower" or g == 0.0:
        return a
    if method == "higher":
        return b
    if method == "nearest":
        return a if g <= 0.5 else b
    if method == "linear":
        return a + (b - a) * g
    raise ValueError(f"method must be one of {METHODS}, got {method!r}")


# ---- helpers on a 1-D result dict (NumPy only) ----------------------------------------------------------------------------------------------
def _one_d(d):
    counts = np.asarray(d["counts"])
    if counts.ndim != 1:
        raise ValueError("a 1-D table is needed (use np.sum over an axis of a joint one first)")
    return counts.astype(np.float64), np.asarray(d["edges"], np.float64)


def density(d):
    """The probability density over the range: counts / (total in range * bin width), float64 (B,); NaN while the table is empty."""
    c, e = _one_d(d)
    with np.errstate(all="ignore"):
        return c / (c.sum() * np.diff(e))


def cdf(d):
    """The cumulative distribution at the right edge of every bin, over ALL counted values (below counts from the start, above never
    arrives): float64 (B,)."""
    c, _ = _one_d(d)
    total = c.sum() + d.get("below", 0) + d.get("above", 0)
    with np.errstate(all="ignore"):
        return (d.get("below", 0) + np.cumsum(c)) / total


def moments(d):
    """{"mean", "variance", "skewness", "kurtosis"} of the values in range from the bin centres (kurtosis: the plain fourth standardised
    moment, 3 for a normal distribution)."""
    c, e = _one_d(d)
    x = 0.5 * (e[:-1] + e[1:])
    n = c.sum()
    with np.errstate(all="ignore"):
        mean = (c * x).sum() / n
        m2, m3, m4 = (((x - mean) ** k * c).sum() / n for k in (2, 3, 4))
        return {"mean": float(mean), "variance": float(m2), "skewness": float(m3 / m2 ** 1.5), "kurtosis": float(m4 / (m2 * m2))}


def quantile_from_counts(d, q):
    """APPROXIMATE quantiles of an accumulated table: the cumulative counts of the values in range inverted, linear inside a bin (the error
    is at most a bin width).  q: scalar or sequence in [0, 1] -> float or float64 array.  NaN while the table is empty."""
    c, e = _one_d(d)
    qs = np.atleast_1d(np.asarray(q, np.float64))
    if ((qs < 0) | (qs > 1)).any():
        raise ValueError("q must lie in [0, 1]")
    cum = np.concatenate([[0.0], np.cumsum(c)])
    if cum[-1] == 0:
        out = np.full(len(qs), np.nan)
    else:
        target = qs * cum[-1]
        k = np.clip(np.searchsorted(cum, target, side="left") - 1, 0, len(c) - 1)      # (the smallest x whose cumulative count reaches the target)
        with np.errstate(all="ignore"):
            frac = np.where(c[k] > 0, (target - cum[k]) / c[k], 0.0)
        out = e[k] + np.clip(frac, 0.0, 1.0) * (e[k + 1] - e[k])
    return float(out[0]) if np.ndim(q) == 0 else out


def channels_array(channels):
    """The channels (ride_ops.DistChannel) as the float64 array (n, 12) a checkpoint holds under dist.channels: quantity, bins, lo, hi, the
    same of the second side (-1, 0, 0, 0 for a 1-D table), the box."""
    return np.array([[c.quantity, c.bins, c.lo, c.hi, c.quantity_b, c.bins_b, c.lo_b, c.hi_b, *c.box] for c in channels], np.float64)


class Distributions(CountedRider):
    """The accumulated distributions of a FluidSimulator (start_distributions): the device tables and their parameters.
    held(z) -> (channels array (n, 12), every, start), or None."""
    kind, payload, noun, plural = "dist", "tables", "distributions", True
    params = (Param("channels", np.asarray, lambda a: np.asarray(a, np.float64), "{theirs} accumulated with other channels than {ours}",
                    np.array_equal),)
    refuses_missing = False

    def __init__(self, dev, dist, every, start_step):
        super().__init__(dev, dist, every, start_step)
        self.dist = dist

    def attached(self):
        return (channels_array(self.dist.channels),)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.dist_launch(self.dist, sim._solver.dx, v, p)

    def data(self):
        out = []
        for k, c in enumerate(self.dist.channels):
            counts, tails, _, samples = self.dev.dist_read(self.dist, k)
            out.append(result(self.dev, c, counts, tails, samples, self.sample_steps(samples)))
        return out

    def _launches(self):
        return self.dev.dist_read(self.dist, 0)[2]      # (the read is per channel and has no form without the payload)
