"""NumPy stand-in for the snapshot-POD primitives of fs.runtime.Device (_p_pod_create / _read / _gram / _combine / _get / _set / _reset /
_free and the "pod_launch" kernel op) on the CPU stand-in device of tests/modes_standin.py (history, averages, loads and modes below it).
Slots, counters and the operation order follow include/fs_hip.h fs_pod_* through tests/pod_ref.py; everything above the primitives (the
rider, the signature token, the ring order, the checkpoint, the decomposition) is the product's own code."""
import os

import numpy as np
from pod_ref import State, combine_ref, gram_ref, launch_ref


def pod_mixin(base):
    class PodStandIn(base):
        def _p_pod_create(self, slots, every, start):
            return State((self.nx, self.nyl), slots, self.dtype, every, start)

        def _p_kernel(self, name, *args):
            if name != "pod_launch":
                return super()._p_kernel(name, *args)
            st, limit, vh, ph = args
            launch_ref(st, self._own(vh), self._own(ph), self._own_mask, limit if limit > 0.0 else None)

        def _p_pod_read(self, st):
            return st.launches, st.samples

        def _p_pod_gram(self, st, slots):
            assert slots == st.M
            return gram_ref(st.slots[:st.resident]), st.launches, st.samples

        def _p_pod_combine(self, st, weights, vh, ph):
            v, p = combine_ref(st.slots, weights, self._own_mask, self.dtype)
            self._own(vh)[...] = v
            self._own(ph)[...] = p

        def _p_pod_get(self, st, slots):
            return st.slots.copy()

        def _p_pod_set(self, st, slots, launches, samples):
            assert slots.shape == st.slots.shape and slots.dtype == st.slots.dtype
            st.slots[...] = slots
            st.launches, st.samples = launches, samples

        def _p_pod_reset(self, st):
            st.reset()

        def _p_pod_free(self, st):
            st.slots = None

    return PodStandIn


def device_cls():
    from modes_standin import device_cls as below
    return pod_mixin(below())


def make_sim(fname):
    from helpers import make_product, traj_config
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    return make_product(g, cfg), cfg
