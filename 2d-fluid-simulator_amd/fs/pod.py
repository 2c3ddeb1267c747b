"""Host side of the snapshot POD (new; the reference has none): the proper orthogonal decomposition of the sampled flow by the method of
snapshots.  The device (csrc/fs_pod.h, include/fs_hip.h fs_pod_*) keeps the last M sampled fields resident and reduces their M x M Gram matrix
G[a][b] = sum over the cells of u_a u_b + w_a w_b; everything here is algebra on that matrix.  Pure NumPy apart from the rider class: testable
without a device.  Driven by FluidSimulator.start_pod / pod / pod_fields / pod_snapshot / reset_pod / stop_pod.

With the snapshots x_m as rows, the eigenvectors V[:, k] of G (eigenvalues lambda_k, descending) give the modes phi_k = sum_m V[m, k] x_m /
sqrt(lambda_k) - energy-ranked, orthonormal under the plain cell sum of u_a u_b + w_a w_b - and the temporal coefficients a_k(m) =
sqrt(lambda_k) V[m, k], so that x_m = sum_k a_k(m) phi_k.  A mode is a linear combination of the resident snapshots: the device forms it from
the weights alone (fs_pod_combine), and the pressure planes combined with the same weights give the extended pressure mode."""
import numpy as np

from .riders import Rider, samples_after

POD_MAX = 64


def decompose(gram, subtract_mean=True):
    """The POD of n snapshots from their Gram matrix `gram` (n, n), float64 -> {"energies": lambda_k descending, (r,); "fraction": lambda_k /
    sum of the returned lambda; "coefficients": (n, r), a_k(m) = sqrt(lambda_k) V[m, k]; "weights": (r, n), mode k = sum_m weights[k, m] *
    snapshot m; "mean_weights": (n,), 1 / n each (zeros without subtract_mean): the combination that a_k(m) phi_k is added to}.

    subtract_mean: the decomposition is that of the fluctuations x_m - mean, whose Gram matrix is G' = C G C with C = I - 1 1^T / n; the mode
    weights are pushed through C, so a mode of the fluctuations is still a linear combination of the RAW snapshots.  Eigenvalues by
    numpy.linalg.eigh of the symmetrised matrix.  Modes with lambda_k <= n eps lambda_0 are not returned (r <= n is the numerical rank: the
    rule of numpy.linalg.matrix_rank) - after the mean is subtracted at least one always goes.  The matrix holds the raw snapshots: the
    subtraction leaves rounding of order eps n |mean|^2 behind, and a mode whose lambda_k is not well above that is noise, whatever the
    rank rule says.  The modes are orthonormal under the plain
    cell sum of u_a u_b + w_a w_b, and snapshot m is mean + sum_k a_k(m) phi_k.  With cells of area dx^2 at density 1, dx^2 / 2 turns an
    eigenvalue into kinetic energy per unit depth (summed over the n snapshots; / n: their average)."""
    G = np.array(gram, np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or len(G) < 2:
        raise ValueError(f"gram must be a square matrix of at least 2 snapshots, got shape {G.shape}")
    if not np.all(np.isfinite(G)):
        raise ValueError("gram holds non-finite entries (did the run diverge?)")
    n = len(G)
    C = np.eye(n) - np.full((n, n), 1.0 / n) if subtract_mean else np.eye(n)
    Gc = C @ G @ C
    lam, V = np.linalg.eigh(0.5 * (Gc + Gc.T))
    order = np.argsort(lam)[::-1]
    lam, V = lam[order], V[:, order]
    top = lam[0] if lam[0] > 0.0 else 0.0
    keep = lam > n * np.finfo(np.float64).eps * top
    lam, V = lam[keep], V[:, keep]
    # (the sign of an eigenvector is eigh's to choose: the largest entry is made positive, so that two runs name the same mode)
    for k in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, k])), k] < 0.0:
            V[:, k] = -V[:, k]
    root = np.sqrt(lam)
    total = lam.sum()
    return {"energies": lam, "fraction": lam / total if total > 0.0 else lam.copy(), "coefficients": V * root,
            "weights": (C @ V / root).T.copy(), "mean_weights": np.full(n, 1.0 / n if subtract_mean else 0.0)}


def ring_slots(samples, slots):
    """-> int (n,): the slot of resident sample m = 0 .. n - 1 in chronological order, n = min(samples, slots): sample k of the run sits in
    slot k % slots, and the oldest resident one is sample `samples - n`."""
    n = min(int(samples), int(slots))
    return (int(samples) - n + np.arange(n)) % int(slots)


def sample_steps(samples, slots, every, start, base=0):
    """-> int64 (n,): the step (counted from start_pod, from 1) after which each resident sample was taken, chronological.  base: samples
    taken before the last reset_pod (they left the ring, the step count ran on)."""
    n = min(int(samples), int(slots))
    k = int(base) + int(samples) - n + np.arange(n, dtype=np.int64)
    return int(start) + (k + 1) * int(every)


class Pod(Rider):
    """The snapshot POD of a FluidSimulator (start_pod): the device ring and its parameters."""

    def __init__(self, dev, pod, every, start_step):
        self.dev, self.pod, self.every, self.start_step = dev, pod, int(every), int(start_step)
        self.base = 0              # samples taken before the last reset (sample_steps)
        self._cache = None         # ((launches, samples, subtract_mean), result of the last analyse())

    @property
    def token(self):
        return ("pod", self.pod.serial)

    def launch(self, sim):
        v, p = sim._solver.get_fields()[:2]
        self.dev.pod_launch(self.pod, v, p)

    def free(self):
        self._cache = None
        self.dev.pod_free(self.pod)

    def reset(self):
        launches, _ = self.dev.pod_read(self.pod)
        self.dev.pod_reset(self.pod)
        self.base = samples_after(launches, self.every, self.start_step)
        self._cache = None

    def analyse(self, subtract_mean=True):
        """The Gram matrix from the device (fs_pod_gram) and its decomposition, in chronological order, kept until the counters move."""
        counters = self.dev.pod_read(self.pod)
        key = counters + (bool(subtract_mean),)
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        G, launches, samples = self.dev.pod_gram(self.pod)
        n = len(G)
        if n < 2:
            raise RuntimeError(f"{n} samples resident, 2 needed ({launches} steps since start_pod(every={self.every}, start_step={self.start_step}))")
        order = ring_slots(samples, self.pod.slots)
        out = {"gram": G[np.ix_(order, order)], "slots": order, "samples": samples, "steps": launches,
               "sample_steps": sample_steps(samples, self.pod.slots, self.every, self.start_step, self.base)}
        out.update(decompose(out["gram"], subtract_mean))
        self._cache = (key, out)
        return out

    def slot_weights(self, chronological):
        """Weights over the resident samples in chronological order -> float64 (M,) in slot order (the empty slots 0)."""
        _, samples = self.dev.pod_read(self.pod)
        w = np.zeros(self.pod.slots)
        w[ring_slots(samples, self.pod.slots)] = chronological
        return w

    def checkpoint(self):
        slots, launches, samples = self.dev.pod_get(self.pod)
        return {"pod.slots": slots, "pod.launches": np.array(launches), "pod.samples": np.array(samples), "pod.base": np.array(self.base),
                "pod.snapshots": np.array(self.pod.slots), "pod.every": np.array(self.every), "pod.start": np.array(self.start_step)}

    @staticmethod
    def held(z):
        """-> (snapshots, every, start), or None."""
        return (int(z["pod.snapshots"]), int(z["pod.every"]), int(z["pod.start"])) if "pod.slots" in z else None

    def restore(self, z):
        self.dev.pod_set(self.pod, z["pod.slots"], int(z["pod.launches"]), int(z["pod.samples"]))
        self.base = int(z["pod.base"])
        self._cache = None
        return int(z["pod.samples"])
