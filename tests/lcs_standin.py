"""NumPy stand-in for the flow-map primitives of fs.runtime.Device (_p_flowmap_create / _advance / _cauchy_green / _get / _reset / _free) on the
CPU stand-in device of tests/pod_standin.py (history, averages, loads, modes and the POD below it).  Lattice, fates and operation order follow
csrc/fs_lcs.h through tests/lcs_ref.py; everything above the primitives (the slot order, the window, the step size, the FTLE, the returned
dictionary, the refusals) is the product's own code."""
import numpy as np
from lcs_ref import advance_ref, cauchy_green_ref, seed_ref


def lcs_mixin(base):
    class LcsStandIn(base):
        live_flowmaps = 0          # lattices created and not freed (the tests ask that flow_map leaves none behind)

        def _p_flowmap_create(self, box, refine):
            type(self).live_flowmaps += 1
            return seed_ref(self._own_mask, box, refine)

        def _p_flowmap_advance(self, st, pod_st, slot_from, slot_to, h, substeps):
            advance_ref(st, pod_st.slots[slot_from], pod_st.slots[slot_to], self._own_mask, h, substeps)

        def _p_flowmap_cauchy_green(self, st):
            cauchy_green_ref(st)

        def _p_flowmap_get(self, st, shape):
            assert st["x"].shape == tuple(shape)
            return st["x"].copy(), st["y"].copy(), st["status"].copy(), st["lam"].copy()

        def _p_flowmap_reset(self, st):
            st.update(seed_ref(self._own_mask, st["box"], st["refine"]))

        def _p_flowmap_free(self, st):
            type(self).live_flowmaps -= 1
            st.clear()

    return LcsStandIn


def device_cls():
    from pod_standin import device_cls as below
    return lcs_mixin(below())


def make_sim(fname):
    from pod_standin import make_sim as below
    return below(fname)

