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
"""
import numpy as np

FLUID, WALL, OUTFLOW = 0, 1, 3


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
