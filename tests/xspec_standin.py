"""NumPy stand-in for the cross-spectrum primitives of fs.runtime.Device (_p_xspec_create / _read / _plane / _get / _set / _reset / _free and
the "xspec_launch" kernel op) as a mixin over the CPU stand-in device of tests/spec_standin.py (the energy spectra and everything below
them).  Planes and counters follow include/fs_hip.h fs_xspec_* through tests/xspec_ref.py; everything above the primitives (the tables, the
box and pair checks, the rider, the signature token, the checkpoint and its refusals, the result dict) is the product's own code."""
import numpy as np

import xspec_ref as XR
from spec_standin import make_sim  # noqa: F401 (re-exported)


def xspec_mixin(base):
    class XSpecStandIn(base):
        def _p_xspec_create(self, box, qa, qb, dx, wx, wy, twx, twy, c1x, c1y, detrend, every, start):
            return XR.State(box, qa, qb, dx, (wx.copy(), wy.copy(), twx.copy(), twy.copy(), c1x, c1y), detrend, every, start)

        def _p_kernel(self, name, *args):
            if name != "xspec_launch":
                return super()._p_kernel(name, *args)
            st, limit, vh, ph = args
            st.launch(self._own(vh), self._own(ph), self._own_mask, limit if limit > 0.0 else None)

        def _p_xspec_read(self, st, words):
            assert words in (0, st.sums.size)
            return (st.sums.ravel().copy() if words else np.empty(0, np.float64)), st.launches, st.samples

        def _p_xspec_plane(self, st, cells):
            assert cells == st.re.size
            return np.ascontiguousarray(np.stack([st.re, st.im], axis=-1)).ravel()

        def _p_xspec_get(self, st, words):
            return self._p_xspec_read(st, words)

        def _p_xspec_set(self, st, sums, launches, samples):
            st.sums = sums.reshape(st.sums.shape).copy()
            st.launches, st.samples = launches, samples

        def _p_xspec_reset(self, st):
            st.sums = np.zeros_like(st.sums)
            st.samples = 0

        def _p_xspec_free(self, st):
            st.sums = None

    return XSpecStandIn


def device_cls():
    from spec_standin import device_cls as below
    return xspec_mixin(below())
