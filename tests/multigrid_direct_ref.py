"""NumPy restatement of the multigrid pressure updater with coarsest="direct" (fs.pressure_updater.MultigridPressureUpdater; csrc/fs_mg.h
k_mg_direct): tests/multigrid_ref.py's MultigridRef with the hierarchy cut at `level` and that level's sweeps replaced by the product with a
given inverse, in the specified order.  (cells, M) are arguments - the product's own upload (MultigridPressureUpdater.direct_matrix()) or
fs.multigrid.direct_solve's result - so that no comparison rests on two LAPACK calls agreeing bit for bit.

    r[j] = R[cells[j]] for j < n;   r[j] = 0 for n <= j < stride = 64 ceil(n / 64)          (the padded columns take part: 0 * 0)
    row i, lane l = 0 .. 63:   a_l = 0;   for k = 0 .. stride / 64 - 1:   a_l = a_l + M[i][64 k + l] * r[64 k + l]
    for s = 32, 16, 8, 4, 2, 1:   a_l = a_l + a_{l + s}   for l < s
    E[cells[i]] = a_0                                                                       (inactive cells keep 0)

Every operation is one IEEE operation in the field dtype.  Arrays are (nx, ny), indexed [I, J]; a cell index is J * nx + I."""
import numpy as np

import multigrid_ref as M


def direct_apply(cells, Minv, R):
    """E of the level from its right-hand side R (nx, ny) in R's dtype, in the order above."""
    dtype = R.dtype
    nx, ny = R.shape
    cells = np.asarray(cells, np.int64)
    n = cells.size
    E = np.zeros_like(R)
    if n == 0:
        return E
    assert Minv.shape == (n, n) and Minv.dtype == dtype, (Minv.shape, Minv.dtype, n, dtype)
    stride = 64 * ((n + 63) // 64)
    ii, jj = cells % nx, cells // nx
    r = np.zeros(stride, dtype)
    r[:n] = R[ii, jj]
    Mp = np.zeros((n, stride), dtype)
    Mp[:, :n] = Minv
    a = np.zeros((n, 64), dtype)
    for k in range(stride // 64):
        a = a + Mp[:, 64 * k:64 * k + 64] * r[None, 64 * k:64 * k + 64]
    s = 32
    while s >= 1:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    assert a.dtype == dtype
    E[ii, jj] = a[:, 0]
    return E


class MultigridDirectRef(M.MultigridRef):
    """MultigridRef whose hierarchy ends at level `level` (1-based), solved by E = M R on `cells`.  matrix(dtype): fs.multigrid.direct_solve
    of that level, rounded to the field dtype - for the CPU tests; GPU comparisons pass the product's direct_matrix()."""

    def __init__(self, bc, dt, dx, level, cells=None, Minv=None, **kw):
        super().__init__(bc, dt, dx, **kw)
        assert 1 <= level <= len(self.levels), (level, len(self.levels))
        self.levels = self.levels[:level]
        if cells is None:
            cells, Minv = self.matrix()
        self.set_matrix(cells, Minv)

    def matrix(self):
        from fs.multigrid import direct_solve
        lv = self.levels[-1]
        cells, Minv = direct_solve(lv.cx, lv.cy, lv.diag)
        return cells, Minv.astype(self.bc.dtype)

    def set_matrix(self, cells, Minv):
        lv = self.levels[-1]
        cells = np.asarray(cells, np.int64)
        want = np.flatnonzero(lv.active.T.ravel())      # (J major: J * nx + I ascending)
        assert np.array_equal(cells, want), "cells must be the last level's active cells, ascending"
        self.cells, self.Minv = cells, np.ascontiguousarray(Minv, self.bc.dtype)

    def w(self, k, R):
        if k == len(self.levels):
            return direct_apply(self.cells, self.Minv, R)
        return super().w(k, R)
