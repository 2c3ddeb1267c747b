"""NumPy restatement of the multigrid pressure updater (fs.pressure_updater.MultigridPressureUpdater, csrc/fs_mg.h): the specification the
GPU path is compared with bit for bit (tests/test_gpu_multigrid.py) and whose convergence tests/test_multigrid_ref.py checks.

Everything is evaluated in the field dtype, one correctly rounded IEEE operation per written operation, in the written order.  K7, the
Jacobi prediction and the red-black smoother are the CPU oracle's (OracleBC, OracleJacobi.sweep, OracleRedBlackSor); the set of wall cells
that K7 never writes is found by probing K7.  Arrays are (nx, ny), indexed [I, J].

    fine residual   r = 4 (predict_p(p, v) - p) on fluid cells after K7, 0 elsewhere
    restriction     R[I, J] = (r[2I, 2J] + r[2I+1, 2J]) + (r[2I, 2J+1] + r[2I+1, 2J+1])
    prolongation    copies E[i >> 1, j >> 1]
    off(E)[I, J]    = ((cx[I-1, J] E[I-1, J] + cx[I, J] E[I+1, J]) + cy[I, J-1] E[I, J-1]) + cy[I, J] E[I, J+1]
                      (outside the level coefficient and E are 0.0: the products are formed and added like the others)
    half sweep      active cells of one parity of I + J:  E = (off(E) + R) / diag;  a sweep is parity 1, then parity 0
    level residual  R - (diag E - off(E)) on active cells, 0 elsewhere
    W(k, R)         E = 0; last level: coarsest_sweeps sweeps.  Else coarse_sweeps sweeps, then twice:
                    Rc = restrict(level residual); E[active] += prolong(W(k + 1, Rc)); coarse_sweeps sweeps
    update(p, v)    n_cycles x { smoother(pre); K7(p.current); R1; E1 = W(1, R1); p.current[fluid] += prolong(E1);
                                 p.next[fluid] += prolong(E1); K7(p.next); smoother(post) }

Why p.next is corrected too: the reference's red-black iteration is a two-buffer method - its even half sweep blends with the value p.next
held before (the iterate of one iteration earlier) and reads p.next's wall cells as K7 left them then.  Both buffers are iterates of the same
equation, so the error equation asks for the same correction in both; with p.current alone corrected, the first post-smoothing iteration
puts (1 - omega) x (the missing correction) back on every even cell and the cycle does not converge (tests/test_multigrid_ref.py).
"""
import numpy as np

from oracle import oracle as O


def probe_never_written(bc):
    """Wall cells no branch of K7 writes: K7 copies from fluid cells only, so walls at 1 over fluid at 0 stay 1 exactly where nothing fires."""
    p = np.where(bc.mask == 1, 1.0, 0.0).astype(bc.dtype)
    bc.set_pressure_boundary_condition(p)
    return (bc.mask == 1) & (p == 1.0)


def restrict(r):
    return (r[0::2, 0::2] + r[1::2, 0::2]) + (r[0::2, 1::2] + r[1::2, 1::2])


def prolong(e):
    return np.repeat(np.repeat(e, 2, axis=0), 2, axis=1)


class Level:
    def __init__(self, cx, cy, diag, dtype):
        self.cx, self.cy, self.diag = (np.ascontiguousarray(a, dtype) for a in (cx, cy, diag))
        assert all(np.array_equal(a, b) for a, b in zip((self.cx, self.cy, self.diag), (cx, cy, diag))), "coefficients must be exact in the dtype"
        self.shape = self.cx.shape
        self.active = self.diag > 0
        self.cxw, self.cys = np.zeros_like(self.cx), np.zeros_like(self.cy)
        self.cxw[1:, :] = self.cx[:-1, :]
        self.cys[:, 1:] = self.cy[:, :-1]
        self.div = np.where(self.active, self.diag, self.diag.dtype.type(1))
        ii, jj = np.indices(self.shape)
        self.parity = (ii + jj) % 2

    def off(self, E):
        Ep = np.pad(E, 1)
        return ((self.cxw * Ep[:-2, 1:-1] + self.cx * Ep[2:, 1:-1]) + self.cys * Ep[1:-1, :-2]) + self.cy * Ep[1:-1, 2:]

    def half(self, E, R, parity):
        new = (self.off(E) + R) / self.div
        sel = self.active & (self.parity == parity)
        E[sel] = new[sel]

    def sweep(self, E, R):
        self.half(E, R, 1)
        self.half(E, R, 0)

    def residual(self, E, R):
        return np.where(self.active, R - (self.diag * E - self.off(E)), self.diag.dtype.type(0))


def hierarchy(bc, wall_term=True):
    """Levels 1, 2, ... from the mask (float64 arithmetic on dyadic rationals, then cast exactly)."""
    m = bc.mask
    fluid = m == 0
    cx, cy = np.zeros(m.shape), np.zeros(m.shape)
    cx[:-1, :] = fluid[:-1, :] & fluid[1:, :]
    cy[:, :-1] = fluid[:, :-1] & fluid[:, 1:]
    fixed = m == 3
    if wall_term:
        fixed = fixed | probe_never_written(bc)
    nb = np.zeros(m.shape)
    nb[1:, :] += fixed[:-1, :]
    nb[:-1, :] += fixed[1:, :]
    nb[:, 1:] += fixed[:, :-1]
    nb[:, :-1] += fixed[:, 1:]
    d = np.where(fluid, nb, 0.0)
    d0 = d
    levels = []
    while cx.shape[0] % 2 == 0 and cx.shape[1] % 2 == 0:
        cxn = 0.5 * (cx[1::2, 0::2] + cx[1::2, 1::2])
        cyn = 0.5 * (cy[0::2, 1::2] + cy[1::2, 1::2])
        dn = 0.5 * ((d[0::2, 0::2] + d[1::2, 0::2]) + (d[0::2, 1::2] + d[1::2, 1::2]))
        diag = dn + cxn
        diag[1:, :] += cxn[:-1, :]
        diag += cyn
        diag[:, 1:] += cyn[:, :-1]
        levels.append(Level(cxn, cyn, diag, bc.dtype))
        cx, cy, d = cxn, cyn, dn
    if not levels:
        raise ValueError(f"multigrid needs even grid extents, got {m.shape}")
    return levels, d0


class MultigridRef:
    """Has update(p, v) like the oracle's updaters: OracleMacSolver / OracleCipSolver accept it as their pressure updater."""

    def __init__(self, bc, dt, dx, relaxation_factor=1.3, n_cycles=1, pre=2, post=2, coarse_sweeps=2, coarsest_sweeps=64, wall_term=True, correct_next=True):
        self.bc, self.dt, self.dx = bc, dt, dx
        self.n_cycles, self.coarse_sweeps, self.coarsest_sweeps = int(n_cycles), int(coarse_sweeps), int(coarsest_sweeps)
        self.levels, self.d0 = hierarchy(bc, wall_term)
        self.pre = O.OracleRedBlackSor(bc, dt, dx, relaxation_factor, int(pre))
        self.post = O.OracleRedBlackSor(bc, dt, dx, relaxation_factor, int(post))
        self._jacobi = O.OracleJacobi(bc, dt, dx, 1)
        self.fluid = bc.mask == 0
        self.correct_next = correct_next      # (False: the correction on p.current alone, kept for the regression test)

    def fine_residual(self, p, v):
        """4 (predict_p - p) on fluid cells of a p that K7 has been applied to."""
        pred = np.zeros_like(p)
        self._jacobi.sweep(pred, p, v)
        t = p.dtype.type
        return np.where(self.fluid, t(4) * (pred - p), t(0))

    def w(self, k, R):
        """W(k, R) -> E; k = 1 is self.levels[0]."""
        lv = self.levels[k - 1]
        E = np.zeros_like(R)
        if k == len(self.levels):
            for _ in range(self.coarsest_sweeps):
                lv.sweep(E, R)
            return E
        for _ in range(self.coarse_sweeps):
            lv.sweep(E, R)
        for _ in range(2):
            Ec = self.w(k + 1, restrict(lv.residual(E, R)))
            up = prolong(Ec)
            E[lv.active] = E[lv.active] + up[lv.active]
            for _ in range(self.coarse_sweeps):
                lv.sweep(E, R)
        return E

    def cycle(self, p, v):
        self.pre.update(p, v)
        self.bc.set_pressure_boundary_condition(p.current)
        E1 = self.w(1, restrict(self.fine_residual(p.current, v)))
        up = prolong(E1)
        p.current[self.fluid] = p.current[self.fluid] + up[self.fluid]
        if self.correct_next:
            p.next[self.fluid] = p.next[self.fluid] + up[self.fluid]
            self.bc.set_pressure_boundary_condition(p.next)
        self.post.update(p, v)

    def update(self, p, v_current):
        for _ in range(self.n_cycles):
            self.cycle(p, v_current)


def poisson_l2(bc, dt, dx, p, v):
    """l2 norm over fluid cells of predict_p(p) - p, with K7 applied to a copy of p first."""
    q = p.copy()
    bc.set_pressure_boundary_condition(q)
    pred = np.zeros_like(q)
    O.OracleJacobi(bc, dt, dx, 1).sweep(pred, q, v)
    r = (pred - q)[bc.mask == 0].astype(np.float64)
    return float(np.sqrt(np.sum(r * r)))
