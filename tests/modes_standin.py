"""NumPy stand-in for the harmonic-mode primitives of fs.runtime.Device (_p_modes_create / _read / _write / _reset / _combine / _rows / _free
and the "modes_accumulate" kernel op) on the CPU stand-in device of tests/loads_standin.py (history, averages and loads below it).  Planes,
scalars, counters and the operation order follow include/fs_hip.h fs_modes_* through tests/modes_ref.py; everything above the primitives (the
rider, the signature token, the checkpoint, the fit) is the product's own code."""
import os

import numpy as np
from modes_ref import State, combine_ref, launch_ref


def modes_mixin(base):
    class ModesStandIn(base):
        def _p_modes_create(self, cos_sin, every, start):
            st = State((self.nx, self.nyl), cos_sin[:, 0], cos_sin[:, 1])
            st.every, st.start = every, start
            return st

        def _p_kernel(self, name, *args):
            if name != "modes_accumulate":
                return super()._p_kernel(name, *args)
            st, limit, vh, ph = args
            launch_ref(st, self._own(vh), self._own(ph), self._own_mask, st.every, st.start, limit if limit > 0.0 else None)

        def _p_modes_read(self, st, nfreq, with_sums=True):
            assert nfreq == st.K
            return (st.sums.copy() if with_sums else None), st.scalars(), st.launches, st.samples

        def _p_modes_write(self, st, sums, scalars, launches, samples):
            assert sums.shape == st.sums.shape
            st.sums[...] = sums
            st.c, st.s, st.gram = scalars[0:2 * st.K:2].copy(), scalars[1:2 * st.K:2].copy(), scalars[2 * st.K:].copy()
            st.launches, st.samples = launches, samples

        def _p_modes_reset(self, st):
            st.reset()

        def _p_modes_combine(self, st, weights, vh, ph):
            v, p = combine_ref(st.sums, weights, self._own_mask, self.dtype)
            self._own(vh)[...] = v
            self._own(ph)[...] = p

        def _p_modes_rows(self, nfreq):
            return (4 if nfreq <= 2 else 2), 1

        def _p_modes_free(self, st):
            st.sums = None

    return ModesStandIn


def device_cls():
    from loads_standin import device_cls as below
    return modes_mixin(below())


def make_sim(fname):
    from helpers import make_product, traj_config
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    return make_product(g, cfg), cfg
