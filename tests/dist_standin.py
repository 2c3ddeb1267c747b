"""NumPy stand-in for the distribution primitives of fs.runtime.Device (_p_dist_create / _read / _get / _set / _reset / _free / _select and
the "dist_launch" kernel op) on the CPU stand-in device of tests/vortex_standin.py (history, averages, loads, modes, the POD and the vortex
tracker below it).  Tables, tails and counters follow include/fs_hip.h fs_dist_* through tests/dist_ref.py; everything above the primitives
(the rider, the signature token, the checkpoint and its refusals, the result dicts, the quantile arithmetic) is the product's own code."""
import os

import numpy as np

import dist_ref as D

NTAIL = 4


class State:
    """A fresh fs_dist_create: every channel's table (bin bb * Ba + ba) and tail words, the counters."""

    def __init__(self, chans, every, start):
        self.chans, self.every, self.start = list(chans), every, start
        self.launches = self.samples = 0
        self.tables = [np.zeros(c.bins * max(1, c.bins_b) + NTAIL, np.int64) for c in chans]


def launch_ref(st, v, p, mask, dx, limit=None):
    """One launch of fs_dist_launch, sampling or not."""
    n = st.launches
    st.launches = n + 1
    if not (n + 1 > st.start and (n + 1 - st.start) % st.every == 0):
        return
    st.samples += 1
    for c, t in zip(st.chans, st.tables):
        qa = D.QUANTITIES[c.quantity]
        if c.joint:
            h = D.field_joint(qa, D.QUANTITIES[c.quantity_b], v, p, mask, dx, (c.lo, c.hi, c.bins), (c.lo_b, c.hi_b, c.bins_b), c.box, limit)
            t[:-NTAIL] += h["counts"].T.ravel()
            t[-NTAIL] += h["outside"]
        else:
            h = D.field_histogram(qa, v, p, mask, dx, c.bins, (c.lo, c.hi), c.box, limit)
            t[:-NTAIL] += h["counts"]
            t[-NTAIL] += h["below"]
            t[-NTAIL + 1] += h["above"]
        t[-NTAIL + 2] += h["nan"]


def dist_mixin(base):
    class DistStandIn(base):
        def _p_dist_create(self, chans, every, start):
            return State(chans, every, start)

        def _p_kernel(self, name, *args):
            if name != "dist_launch":
                return super()._p_kernel(name, *args)
            st, limit, dx, vh, ph = args
            launch_ref(st, self._own(vh), self._own(ph), self._own_mask, dx, limit if limit > 0.0 else None)

        def _p_dist_read(self, st, chan, bins):
            t = st.tables[chan]
            assert bins in (0, len(t) - NTAIL)
            return t[:bins].copy(), (t[-NTAIL:].copy() if bins else np.zeros(NTAIL, np.int64)), st.launches, st.samples

        def _p_dist_get(self, st, words):
            out = np.concatenate(st.tables)
            assert len(out) == words
            return out

        def _p_dist_set(self, st, words, launches, samples):
            at = 0
            for t in st.tables:
                t[...] = words[at:at + len(t)]
                at += len(t)
            st.launches, st.samples = launches, samples

        def _p_dist_reset(self, st):
            for t in st.tables:
                t[...] = 0
            st.samples = 0

        def _p_dist_free(self, st):
            st.tables = None

        def _p_dist_select(self, q, box, limit, dx, vh, ph, ranks):
            s, nan = D.sorted_values(D.QUANTITIES[q], self._own(vh), self._own(ph), self._own_mask, dx, box, limit if limit > 0.0 else None)
            if ranks and ranks[-1] >= len(s):
                raise ValueError(f"rank {ranks[-1]} >= n = {len(s)}, the number of selected cells whose value is not NaN")
            return s[list(ranks)].astype(np.float64), len(s), nan

    return DistStandIn


def device_cls():
    from vortex_standin import device_cls as below
    return dist_mixin(below())


def make_sim(fname):
    from helpers import make_product, traj_config
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", fname))
    cfg = traj_config(g)
    return make_product(g, cfg), cfg
