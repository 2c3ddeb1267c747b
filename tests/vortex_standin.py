"""NumPy stand-in for the vortex primitives of fs.runtime.Device (_p_vortex_create / _read / _get_labels / _set / _label / _criterion / _free and
the "vortex_launch" kernel op) on the CPU stand-in device of tests/pod_standin.py (history, averages, loads, modes and the POD below it).
Samples, counters and the ring follow include/fs_hip.h fs_vortex_* through tests/vortex_ref.py; everything above the primitives (the rider,
the signature token, the ring's room, the checkpoint, the conversions, the tracking) is the product's own code."""
import os

import numpy as np
import vortex_ref as R


class State:
    """A fresh fs_vortex_create: the ring of at most `capacity` samples, the counters, the planes of the last sampling launch."""

    def __init__(self, shape, which, threshold, exponent, every, start, min_area, max_vortices, max_components, capacity):
        self.which, self.threshold, self.e, self.every, self.start = which, threshold, exponent, every, start
        self.min_area, self.maxv, self.maxc, self.cap = min_area, max_vortices, max_components, capacity
        self.launches = self.lost = 0
        self.ring = []
        self.flags, self.labels = np.zeros(shape, np.uint8), np.full(shape, -1, np.int32)


def launch_ref(st, v, mask, dx, limit=None):
    """One launch of fs_vortex_launch, sampling or not; a sampling launch that finds the ring full is lost and does nothing."""
    n = st.launches
    st.launches = n + 1
    if not (n + 1 > st.start and (n + 1 - st.start) % st.every == 0):
        return
    if len(st.ring) >= st.cap:
        st.lost += 1
        return
    s = R.sample(v, mask, dx, R.CRITERIA[st.which], st.threshold, st.e, st.min_area, st.maxv, st.maxc, limit)
    words = np.zeros(R.NHEAD + R.NREC * st.maxv, np.int64)
    words[:6] = (n, s["components"], s["passed"], s["count"], s["clipped"], s["dropped_cells"])
    rec = words[R.NHEAD:].reshape(st.maxv, R.NREC)
    for k, name in enumerate(R.RECORD):
        rec[:s["count"], k] = s["raw"][name]
    st.ring.append(words)
    st.flags, st.labels = s["flags"], s["labels"]


def vortex_mixin(base):
    class VortexStandIn(base):
        def _p_vortex_create(self, which, threshold, exponent, every, start, min_area, max_vortices, max_components, capacity):
            return State((self.nx, self.nyl), which, threshold, exponent, every, start, min_area, max_vortices, max_components, capacity)

        def _p_kernel(self, name, *args):
            if name != "vortex_launch":
                return super()._p_kernel(name, *args)
            st, limit, dx, vh = args
            launch_ref(st, self._own(vh), self._own_mask, dx, limit if limit > 0.0 else None)

        def _p_vortex_read(self, st, capacity, words):
            assert capacity == st.cap and words == R.NHEAD + R.NREC * st.maxv
            out = np.array(st.ring, np.int64).reshape(len(st.ring), words)
            lost, st.ring, st.lost = st.lost, [], 0
            return out, st.launches, lost

        def _p_vortex_get_labels(self, st):
            return st.flags.copy(), st.labels.copy()

        def _p_vortex_set(self, st, launches):
            st.launches, st.ring, st.lost = launches, [], 0

        def _p_vortex_label(self, flags):
            return R.label_plane(flags)

        def _p_vortex_criterion(self, which, limit, dx, vh):
            return R.criterion(R.CRITERIA[which], self._own(vh), self._own_mask, dx, limit if limit > 0.0 else None)[0]

        def _p_vortex_free(self, st):
            st.ring = None

    return VortexStandIn


def device_cls():
    from pod_standin import device_cls as below
    return vortex_mixin(below())


def make_sim(fname):
    from helpers import make_product, traj_config
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    return make_product(g, cfg), cfg
