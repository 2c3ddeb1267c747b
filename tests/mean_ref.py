"""NumPy restatement of the time averages (csrc/fs_mean.h, include/fs_hip.h fs_mean_*): the accumulation of one sample in IEEE double, the
sampling rule as a plain loop, and the per-cell limit of a deferred limit_field.  The yardstick of tests/test_mean_cpu.py and
tests/test_gpu_mean.py: every operation below is one correctly rounded operation per cell, as in the kernel, so sums compare with
np.array_equal."""
import numpy as np


def new_sums(shape):
    return np.zeros((7,) + tuple(shape), np.float64)


def limit_ref(v, limit):
    """limit_field (fs/solver.py:38-43) per cell in the array's own precision: (x, y) scaled onto the circle of radius `limit` when outside."""
    v = np.array(v)
    t = v.dtype.type
    x, y = v[..., 0], v[..., 1]
    nrm = np.sqrt(x * x + y * y)
    hot = nrm > t(limit)
    with np.errstate(invalid="ignore", divide="ignore"):
        xs, ys = t(limit) * (x / nrm), t(limit) * (y / nrm)
    v[..., 0] = np.where(hot, xs, x)
    v[..., 1] = np.where(hot, ys, y)
    return v


def accumulate_ref(sums, v, p, mask, limit=None):
    """Add one sample to sums (7, X, Y) in place: on not-wall cells (mask != 1) S_u += u, S_w += w, S_p += p, S_uu += u * u, S_ww += w * w,
    S_uw += u * w, S_pp += p * p, every operand promoted to double first."""
    if limit is not None:
        v = limit_ref(v, limit)
    u, w, q = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64), np.asarray(p).astype(np.float64)
    m = np.asarray(mask) != 1
    for k, term in enumerate((u, w, q, u * u, w * w, u * w, q * q)):
        sums[k][m] = sums[k][m] + term[m]
    return sums


def sampling_launches(launches, every, start):
    """The launches n (from 0) among the first `launches` that sample, by the rule of the issue in a plain loop: step k = n + 1 counts when
    it lies beyond `start` and the steps since `start` are a multiple of `every`."""
    out = []
    since = 0
    for n in range(launches):
        k = n + 1
        if k <= start:
            continue
        since += 1
        if since % every == 0:
            out.append(n)
    return out


def run_reference(sim, steps, every, start, sums=None, launches=0):
    """Step `sim` eagerly `steps` times and accumulate its downloads by the sampling rule -> (sums, launches, samples added)."""
    mask = np.asarray(sim._solver._bc.mask)
    if sums is None:
        sums = new_sums(mask.shape)
    want = set(sampling_launches(launches + steps, every, start))
    added = 0
    for n in range(launches, launches + steps):
        sim.step()
        if n in want:
            d = sim.field_to_numpy()
            accumulate_ref(sums, d["v"], d["p"], mask)
            added += 1
    return sums, launches + steps, added
