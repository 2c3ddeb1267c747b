"""NumPy stand-in for the scale-flux primitives of fs.runtime.Device (_p_flux_create / _read / _filtered / _get / _set / _reset / _free and
the "flux_launch" kernel op) as a mixin over the CPU stand-in device of tests/xspec_standin.py (the cross-spectra and everything below them).
Planes and counters follow include/fs_hip.h fs_flux_* through tests/flux_ref.py - the planes leave the primitives in the library's layout,
(Ny, Nx) in C order -; everything above the primitives (the box and half-width checks, the rider, the signature token, the checkpoint and
its refusals, the result dict) is the product's own code."""
import numpy as np

import flux_ref as FR
from spec_standin import make_sim  # noqa: F401 (re-exported)


def _flat(planes):
    """(..., Nx, Ny) -> the library's layout, flat."""
    return np.ascontiguousarray(np.swapaxes(planes, -1, -2)).ravel()


def flux_mixin(base):
    class FluxStandIn(base):
        def _p_flux_create(self, box, half_widths, dx, every, start):
            return FR.State(box, half_widths, dx, every, start)

        def _p_kernel(self, name, *args):
            if name != "flux_launch":
                return super()._p_kernel(name, *args)
            st, limit, vh = args
            st.launch(self._own(vh), self._own_mask, limit if limit > 0.0 else None)

        def _p_flux_read(self, st, words):
            assert words in (0, st.sums.size)
            return (_flat(st.sums) if words else np.empty(0, np.float64)), st.launches, st.samples

        def _p_flux_filtered(self, st, index, words):
            assert words == st.filtered[index].size
            return _flat(st.filtered[index])

        def _p_flux_get(self, st, words):
            return self._p_flux_read(st, words)

        def _p_flux_set(self, st, flat, launches, samples):
            nr, ns, nx, ny = st.sums.shape
            st.sums = np.ascontiguousarray(flat.reshape(nr, ns, ny, nx).transpose(0, 1, 3, 2))
            st.launches, st.samples = launches, samples

        def _p_flux_reset(self, st):
            st.sums = np.zeros_like(st.sums)
            st.samples = 0

        def _p_flux_free(self, st):
            st.sums = None

    return FluxStandIn


def device_cls():
    from xspec_standin import device_cls as below
    return flux_mixin(below())
