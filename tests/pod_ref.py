"""NumPy restatement of the snapshot POD's device side (csrc/fs_pod.h, include/fs_hip.h fs_pod_*): the capture into the ring (slot =
samples % M, wall cells 0, a deferred limit_field applied to u, w), the combine pass in its operation order, and the Gram matrix as a plain
float64 sum over the snapshots.  The yardstick of tests/test_pod_cpu.py and tests/test_gpu_pod.py: capture and combine are one correctly
rounded operation per cell, as in the kernels, and compare with np.array_equal; the Gram matrix is the reference of a tolerance (the device
sums in its own fixed order)."""
import numpy as np
from mean_ref import limit_ref, sampling_launches  # noqa: F401 (the one sampling rule, re-exported)


class State:
    """Slots (M, 3, X, Y) in the fields' dtype - u, w, p - launches and samples, as a fresh fs_pod_create."""

    def __init__(self, shape, slots, dtype, every=1, start=0):
        self.M, self.every, self.start = int(slots), int(every), int(start)
        self.slots = np.zeros((self.M, 3) + tuple(shape), dtype)
        self.launches = self.samples = 0

    def reset(self):
        self.slots[...] = 0
        self.samples = 0

    @property
    def resident(self):
        return min(self.samples, self.M)

    def order(self):
        """The slot of resident sample m = 0 .. n - 1, chronological (a plain loop over the samples the ring has seen)."""
        slot_of = {}
        for k in range(self.samples):
            slot_of[k % self.M] = k
        return [s for s, _ in sorted(slot_of.items(), key=lambda kv: kv[1])]


def capture_ref(st, v, p, mask, limit=None):
    """One SAMPLING launch: slot samples % M takes u, w (limited when a limit_field is owed) and p on the not-wall cells, +0 on the wall
    cells; then the sample count."""
    if limit is not None:
        v = limit_ref(v, limit)
    wall = np.asarray(mask) == 1
    s = st.slots[st.samples % st.M]
    s[0] = np.where(wall, 0, v[..., 0])
    s[1] = np.where(wall, 0, v[..., 1])
    s[2] = np.where(wall, 0, np.asarray(p))
    st.samples += 1
    return st


def launch_ref(st, v, p, mask, limit=None):
    """One launch of fs_pod_launch, sampling or not."""
    n = st.launches
    if n + 1 > st.start and (n + 1 - st.start) % st.every == 0:
        capture_ref(st, v, p, mask, limit)
    st.launches = n + 1
    return st


def combine_ref(slots, weights, mask, dtype):
    """k_pod_combine: per field, from 0.0, acc += weights[m] * slot_m for m ascending, in double; wall cells 0; cast -> (v (X, Y, 2), p)."""
    weights = np.asarray(weights, np.float64)
    assert weights.shape == (len(slots),)
    wall = np.asarray(mask) == 1
    out = []
    for a in range(3):
        acc = np.zeros(slots.shape[2:], np.float64)
        for m in range(len(slots)):
            acc = acc + weights[m] * slots[m, a].astype(np.float64)
        out.append(np.where(wall, 0.0, acc).astype(dtype))
    return np.stack(out[:2], axis=-1), out[2]


def gram_ref(snapshots):
    """G[a][b] = sum over the cells of u_a u_b + w_a w_b, a plain float64 sum; snapshots (n, 3, X, Y) or (n, 2, ...)."""
    x = np.asarray(snapshots)[:, :2].astype(np.float64).reshape(len(snapshots), -1)
    return x @ x.T
