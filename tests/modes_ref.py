"""NumPy float64 restatement of the harmonic flow modes (csrc/fs_modes.h, include/fs_hip.h fs_modes_*): the phasor recurrence, the
accumulation of one sample into the planes and into the Gram matrix in the stated operation order, and a loop over the downloads of an
eagerly stepped simulator.  The yardstick of tests/test_modes_cpu.py and tests/test_gpu_modes.py: every operation below is one correctly
rounded IEEE double operation per cell, as in the kernels, so planes and scalars compare with np.array_equal."""
import numpy as np
from mean_ref import limit_ref, sampling_launches  # noqa: F401 (the one sampling rule, re-exported)


class State:
    """Planes (3 B, X, Y), phasors c, s (K,), the Gram triangle (B (B + 1) / 2,), launches and samples, as a fresh fs_modes_create."""

    def __init__(self, shape, cd, sd):
        self.cd, self.sd = np.array(cd, np.float64), np.array(sd, np.float64)
        self.K = len(self.cd)
        self.B = 1 + 2 * self.K
        self.sums = np.zeros((3 * self.B,) + tuple(shape), np.float64)
        self.launches = 0
        self.reset()

    def reset(self):
        self.sums[...] = 0.0
        self.c, self.s = np.ones(self.K), np.zeros(self.K)
        self.gram = np.zeros(self.B * (self.B + 1) // 2)
        self.samples = 0

    def basis(self):
        b = np.empty(self.B)
        b[0] = 1.0
        b[1::2], b[2::2] = self.c, self.s
        return b

    def scalars(self):
        """In the order of fs_modes_read: c_1, s_1, ..., c_K, s_K, then the Gram triangle."""
        ph = np.empty(2 * self.K)
        ph[0::2], ph[1::2] = self.c, self.s
        return np.concatenate([ph, self.gram])


def rotate(c, s, cd, sd):
    """One rotation of the phasors: every product rounded on its own."""
    return c * cd - s * sd, s * cd + c * sd


def accumulate_ref(st, v, p, mask, limit=None):
    """One SAMPLING launch: the planes on not-wall cells (plane a B of field a takes the promoted value as it is, plane a B + j the product
    x * b_j, rounded, then the sum), then the tick - Gram matrix with the phasors just applied, the sample count, the rotation."""
    if limit is not None:
        v = limit_ref(v, limit)
    fields = (v[..., 0].astype(np.float64), v[..., 1].astype(np.float64), np.asarray(p).astype(np.float64))
    m = np.asarray(mask) != 1
    b, B = st.basis(), st.B
    for a, x in enumerate(fields):
        st.sums[a * B][m] = st.sums[a * B][m] + x[m]
        for j in range(1, B):
            st.sums[a * B + j][m] = st.sums[a * B + j][m] + x[m] * b[j]
    t = 0
    for i in range(B):
        for j in range(i, B):
            st.gram[t] = st.gram[t] + b[i] * b[j]
            t += 1
    st.samples += 1
    st.c, st.s = rotate(st.c, st.s, st.cd, st.sd)
    return st


def launch_ref(st, v, p, mask, every, start, limit=None):
    """One launch of fs_modes_accumulate, sampling or not."""
    n = st.launches
    if n + 1 > start and (n + 1 - start) % every == 0:
        accumulate_ref(st, v, p, mask, limit)
    st.launches = n + 1
    return st


def combine_ref(sums, weights, mask, dtype):
    """k_modes_combine: per field a, from 0.0, acc += weights[a, j] * plane[a B + j] for j ascending, in double; wall cells 0; cast."""
    weights = np.asarray(weights, np.float64)
    B = weights.shape[1]
    wall = np.asarray(mask) == 1
    out = []
    for a in range(3):
        acc = np.zeros(sums.shape[1:], np.float64)
        for j in range(B):
            acc = acc + weights[a, j] * sums[a * B + j]
        out.append(np.where(wall, 0.0, acc).astype(dtype))
    return np.stack(out[:2], axis=-1), out[2]


def run_reference(sim, n, freqs, every, start):
    """Step `sim` eagerly n times and accumulate its downloads by the sampling rule -> State."""
    from fs.modes import phasor_steps
    mask = np.asarray(sim._solver._bc.mask)
    cd, sd = phasor_steps(freqs, every, sim._solver.dt)
    st = State(mask.shape, cd, sd)
    want = set(sampling_launches(n, every, start))
    for k in range(n):
        sim.step()
        if k in want:
            d = sim.field_to_numpy()
            accumulate_ref(st, d["v"], d["p"], mask)
        st.launches += 1
    assert st.samples == len(want)
    return st
