"""NumPy stand-in for the spectrum primitives of fs.runtime.Device (_p_spec_create / _read / _plane / _get / _set / _reset / _free and the
"spec_launch" kernel op) on the CPU stand-in device of tests/dist_standin.py (history, averages, loads, modes, the POD, the vortex tracker
and the distributions below it).  Planes and counters follow include/fs_hip.h fs_spec_* through tests/spec_ref.py; everything above the
primitives (the tables, the box checks, the rider, the signature token, the checkpoint and its refusals, the result dict) is the product's
own code."""
import os

import numpy as np

import spec_ref as S


def spec_mixin(base):
    class SpecStandIn(base):
        def _p_spec_create(self, box, wx, wy, twx, twy, c1x, c1y, detrend, every, start):
            return S.State(box, (wx.copy(), wy.copy(), twx.copy(), twy.copy(), c1x, c1y), detrend, every, start)

        def _p_kernel(self, name, *args):
            if name != "spec_launch":
                return super()._p_kernel(name, *args)
            st, limit, vh = args
            st.launch(self._own(vh), self._own_mask, limit if limit > 0.0 else None)

        def _p_spec_read(self, st, cells):
            assert cells in (0, st.power.size)
            return (st.power.ravel().copy() if cells else np.empty(0, np.float64)), st.launches, st.samples

        def _p_spec_plane(self, st, cells):
            assert cells == st.power.size
            return np.ascontiguousarray(np.stack([st.re, st.im], axis=-1)).ravel()

        def _p_spec_get(self, st, cells):
            return self._p_spec_read(st, cells)

        def _p_spec_set(self, st, power, launches, samples):
            st.power = power.reshape(st.power.shape).copy()
            st.launches, st.samples = launches, samples

        def _p_spec_reset(self, st):
            st.power = np.zeros_like(st.power)
            st.samples = 0

        def _p_spec_free(self, st):
            st.power = None

    return SpecStandIn


def device_cls():
    from dist_standin import device_cls as below
    return spec_mixin(below())


def make_sim(fname):
    from helpers import make_product, traj_config
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    return make_product(g, cfg), cfg
