"""NumPy stand-in for the budget primitives of fs.runtime.Device (_p_budget_create / _read / _get / _set / _reset / _free and the
"budget_launch" kernel op) as a mixin over the CPU stand-in device of tests/flux_standin.py (the scale fluxes and everything below them).
Planes and counters follow include/fs_hip.h fs_budget_* through tests/budget_ref.py - the planes leave the primitives in the library's
layout, (Ny, Nx) in C order -; everything above the primitives (the box check, the rider, the signature token, the checkpoint and its
refusals, the derivation) is the product's own code."""
import numpy as np

import budget_ref as BR
from spec_standin import make_sim  # noqa: F401 (re-exported)


def _flat(planes):
    """(..., Nx, Ny) -> the library's layout, flat."""
    return np.ascontiguousarray(np.swapaxes(planes, -1, -2)).ravel()


def budget_mixin(base):
    class BudgetStandIn(base):
        def _p_budget_create(self, box, dx, every, start):
            return BR.State(box, dx, every, start)

        def _p_kernel(self, name, *args):
            if name != "budget_launch":
                return super()._p_kernel(name, *args)
            st, limit, vh, ph = args
            st.launch(self._own(vh), self._own(ph), self._own_mask, limit if limit > 0.0 else None)

        def _p_budget_read(self, st, words):
            assert words in (0, st.sums.size)
            return (_flat(st.sums) if words else np.empty(0, np.float64)), st.launches, st.samples

        def _p_budget_get(self, st, words):
            return self._p_budget_read(st, words)

        def _p_budget_set(self, st, flat, launches, samples):
            n, nx, ny = st.sums.shape
            st.sums = np.ascontiguousarray(flat.reshape(n, ny, nx).transpose(0, 2, 1))
            st.launches, st.samples = launches, samples

        def _p_budget_reset(self, st):
            st.sums = np.zeros_like(st.sums)
            st.samples = 0

        def _p_budget_free(self, st):
            st.sums = None

    return BudgetStandIn


def device_cls():
    from flux_standin import device_cls as below
    return budget_mixin(below())
