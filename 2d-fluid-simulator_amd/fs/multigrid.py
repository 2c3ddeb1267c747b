"""Host side of the multigrid pressure updater (pressure_updater.MultigridPressureUpdater): the mask-aware coefficient hierarchy.

Built once per updater in NumPy and uploaded (include/fs_hip.h fs_mg_create).  Arrays are (nx, ny) like every host array of the package,
indexed [I, J].  Level 0 is the grid itself and exists only to derive level 1:
    cx0[i, j] = 1 where (i, j) and (i + 1, j) are both fluid, cy0 the same for (i, j + 1);
    d0[i, j]  = for a fluid cell the number of its four neighbours that hold a FIXED pressure: outflow cells, and wall cells that no branch
                of set_pressure_boundary_condition (fs/boundary_condition.py:41-65) ever writes (never_written below) - they keep their value, so
                for the error equation they are Dirichlet points like the outflow.  Written walls, inflow cells and the outside insulate.
Level k + 1 exists while both extents of level k are even; every coefficient is a dyadic rational (exact in float32):
    cx[I, J] = 0.5 (cx_k[2I+1, 2J] + cx_k[2I+1, 2J+1])      cy[I, J] = 0.5 (cy_k[2I, 2J+1] + cy_k[2I+1, 2J+1])
    d[I, J]  = 0.5 ((d_k[2I, 2J] + d_k[2I+1, 2J]) + (d_k[2I, 2J+1] + d_k[2I+1, 2J+1]))
    diag     = d + cx[I, J] + cx[I-1, J] + cy[I, J] + cy[I, J-1]   (terms outside the level absent);  a cell is active iff diag > 0.

coarsest="direct" (the updater's option) cuts the hierarchy at direct_level() and solves that level exactly: direct_solve() inverts its operator
on the active cells once, in float64, and the device applies the inverse with one launch per visit (csrc/fs_mg.h k_mg_direct).
"""
import numpy as np

FLUID, WALL, OUTFLOW = 0, 1, 3
DIRECT_MAX = 4096      # active cells of a level that is solved exactly (a dense inverse of at most 64 MB in float32; csrc/fs_mg.h MG_DIRECT_MAX)


def never_written(mask):
    """Wall cells for which no branch of set_pressure_boundary_condition fires (cells outside the grid read as wall there)."""
    m = np.pad(np.asarray(mask, np.uint8), 1, constant_values=WALL)
    w, e, s, n = m[:-2, 1:-1], m[2:, 1:-1], m[1:-1, :-2], m[1:-1, 2:]
    w0, e0, s0, n0 = w == FLUID, e == FLUID, s == FLUID, n == FLUID
    w1, e1, s1, n1 = w == WALL, e == WALL, s == WALL, n == WALL
    written = ((w0 & s1 & n1) | (e0 & s1 & n1) | (s0 & w1 & e1) | (n0 & w1 & e1)
               | (w0 & n0) | (e0 & n0) | (w0 & s0) | (e0 & s0))
    return (np.asarray(mask) == WALL) & ~written


def level0(mask, fixed_walls=None):
    """(cx0, cy0, d0) in float64.  fixed_walls: the never-written set (default: from the mask rules)."""
    mask = np.asarray(mask, np.uint8)
    fluid = mask == FLUID
    cx, cy = np.zeros(mask.shape), np.zeros(mask.shape)
    cx[:-1, :] = fluid[:-1, :] & fluid[1:, :]
    cy[:, :-1] = fluid[:, :-1] & fluid[:, 1:]
    fixed = (mask == OUTFLOW) | (never_written(mask) if fixed_walls is None else np.asarray(fixed_walls, bool))
    nb = np.zeros(mask.shape)
    nb[1:, :] += fixed[:-1, :]
    nb[:-1, :] += fixed[1:, :]
    nb[:, 1:] += fixed[:, :-1]
    nb[:, :-1] += fixed[:, 1:]
    return cx, cy, np.where(fluid, nb, 0.0)


def coarsen(cx, cy, d):
    """(cx, cy, d, diag) of the next level."""
    cxn = 0.5 * (cx[1::2, 0::2] + cx[1::2, 1::2])
    cyn = 0.5 * (cy[0::2, 1::2] + cy[1::2, 1::2])
    dn = 0.5 * ((d[0::2, 0::2] + d[1::2, 0::2]) + (d[0::2, 1::2] + d[1::2, 1::2]))
    diag = dn + cxn
    diag[1:, :] += cxn[:-1, :]
    diag += cyn
    diag[:, 1:] += cyn[:, :-1]
    return cxn, cyn, dn, diag


def build_hierarchy(mask, dtype=np.float32, fixed_walls=None):
    """[(cx, cy, diag), ...] for levels 1, 2, ... as (nx, ny) arrays of `dtype`.  ValueError when the grid admits no coarse level."""
    cx, cy, d = level0(mask, fixed_walls)
    levels = []
    while cx.shape[0] % 2 == 0 and cx.shape[1] % 2 == 0:
        cx, cy, d, diag = coarsen(cx, cy, d)
        lv = tuple(np.ascontiguousarray(a, dtype) for a in (cx, cy, diag))
        if not all(np.array_equal(a, b) for a, b in zip(lv, (cx, cy, diag))):
            raise ValueError("multigrid: a coefficient is not exact in the field dtype")
        levels.append(lv)
    if not levels:
        raise ValueError(f"multigrid needs even grid extents, got {tuple(np.asarray(mask).shape)}")
    return levels


def direct_level(shapes, direct_cells, active=None):
    """1-based index of the level that is solved exactly: the first one with nx * ny <= direct_cells, else the last.  active: the levels'
    active-cell counts (default: every cell); ValueError when the chosen level has more than DIRECT_MAX of them."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if not shapes:
        raise ValueError("direct_level: no levels")
    k = next((k for k, (nx, ny) in enumerate(shapes, start=1) if nx * ny <= direct_cells), len(shapes))
    nx, ny = shapes[k - 1]
    n = nx * ny if active is None else int(active[k - 1])
    if n > DIRECT_MAX:
        raise ValueError(f"multigrid: the level to solve exactly, {nx} x {ny} (level {k} of {len(shapes)}), has {n} active cells; "
                         f"at most {DIRECT_MAX} can be (the hierarchy ends where an extent turns odd: choose a resolution that halves further)")
    return k


def _components(cx, cy, active):
    """Label (0, 1, ...) of the connected component of every active cell, -1 elsewhere; cells connect through non-zero cx / cy."""
    nx, ny = active.shape
    parent = np.arange(nx * ny)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for other, c in ((ny, cx[:-1, :]), (1, cy[:, :-1])):      # (flat index I * ny + J: east is + ny, north + 1)
        ii, jj = np.nonzero(c)
        for a in (ii * ny + jj).tolist():
            ra, rb = find(a), find(a + other)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(a) for a in range(nx * ny)]).reshape(nx, ny)
    _, labels = np.unique(roots[active], return_inverse=True)
    out = np.full(active.shape, -1)
    out[active] = labels
    return out


def direct_solve(cx, cy, diag):
    """(cells, M) of one level: cells (int32) - the indices J * nx + I of the active cells (diag > 0), ascending; M (float64, n x n) - the
    inverse of the level's operator A on them, A[c, c] = diag, A[c, neighbour] = -cx / -cy of the shared face (csrc/fs_mg.h mg_res).
    A connected component of active cells whose rows of A all sum to exactly 0 (the sums are dyadic rationals) has no Dirichlet coupling: its
    block is singular with the constants as null space - a fluid pocket enclosed by a body - and gets the pseudo-inverse,
    M = inv(A + P) - P with P = sum over such components of 1 1^T / n_c.  No active cell: an empty matrix."""
    cx, cy, diag = (np.asarray(a, np.float64) for a in (cx, cy, diag))
    nx, ny = diag.shape
    active = diag > 0
    jj, ii = np.nonzero(active.T)      # (J major, I minor: ascending J * nx + I)
    cells = (jj * nx + ii).astype(np.int32)
    n = cells.size
    if n == 0:
        return cells, np.zeros((0, 0))
    row = np.full((nx, ny), -1)
    row[ii, jj] = np.arange(n)
    A = np.zeros((n, n))
    A[np.arange(n), np.arange(n)] = diag[ii, jj]
    for (di, dj), c in (((1, 0), cx), ((0, 1), cy)):
        i0, j0 = np.nonzero(c[:nx - di, :ny - dj])
        a, b = row[i0, j0], row[i0 + di, j0 + dj]
        assert (a >= 0).all() and (b >= 0).all(), "a coupling reaches an inactive cell"
        A[a, b] = A[b, a] = -c[i0, j0]
    comp = _components(cx, cy, active)[ii, jj]
    sums = A.sum(axis=1)
    P = np.zeros((n, n))
    for label in range(int(comp.max()) + 1):
        sel = comp == label
        if not sums[sel].any():
            idx = np.nonzero(sel)[0]
            P[np.ix_(idx, idx)] = 1.0 / idx.size
    return cells, np.linalg.inv(A + P) - P

