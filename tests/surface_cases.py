"""The checkerboard body shared by tests/test_surface_cases_cpu.py, tests/test_gpu_loads_large.py and tests/test_gpu_history_large.py: a face
list long enough that the record launches of csrc/fs_loads.h and csrc/fs_history.h fold more partials than they have lanes, fields on which
every sum is exact, and a vectorised form of loads_ref.sample_ref.

The grid is (192, 192) with a wall border; inside BOX = (4, 4, 186, 186) every cell with (i + j) % 2 == 0 is wall.  Each of the 182 * 182 / 2 =
16,562 wall cells has four fluid neighbours: 66,248 faces, 259 workgroups of 256 (the last of 200), so that lanes 0 .. 2 of a 256-lane record
launch take two partials.  No flow is ever computed on this mask: the fields are loaded.

Exact fields: u, w, p are integers in [-8, 8] (4 bits), dx = 2^-6, inv_re = 2^-7, the centre (95, 95) puts every lever arm at a multiple of
0.5 below 2^8 (9 bits).  Every face term - pk, pk pk, tk = (inv_re ut) / dx = ut / 2, tk tk, pk dx, inv_re ut and their products with an arm
- is then a dyadic number of at most 13 significant bits and of magnitude below 2^4, a multiple of 2^-15; a sum of 66,248 of them, and of three
samples of them, stays far below 2^53 units of 2^-15: every partial sum in any order is exact in double, and records compare with ==."""
import functools

import numpy as np
from loads_ref import MID, NREC, NSUM

X = Y = 192
BOX = (4, 4, 186, 186)
NFACES = 66248
CENTRE = (95.0, 95.0)
DX = 2.0 ** -6
INV_RE = 2.0 ** -7
SEEDS = (11, 12, 13)          # the three exact field triples
NPROBES = 600
WG = 256                      # LOADS_WG, HIST_FACES_PER_WG and the lanes of both record launches


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mask():
    m = np.zeros((X, Y), np.uint8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    i, j = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    x0, y0, x1, y1 = BOX
    inside = (i >= x0) & (i < x1) & (j >= y0) & (j < y1)
    m[inside & ((i + j) % 2 == 0)] = 1
    return _frozen(m)


@functools.lru_cache(maxsize=None)
def faces():
    from fs.history import body_faces
    return _frozen(body_faces(mask(), BOX))


def partition(n, wg=WG):
    """-> (workgroups of wg items, items of the last one, lanes of a wg-lane fold that take two partials)."""
    parts = -(-n // wg)
    return parts, n - (parts - 1) * wg, max(0, parts - wg)


@functools.lru_cache(maxsize=None)
def exact_fields(seed, dtype):
    """(v (X, Y, 2), p (X, Y)) of integers in [-8, 8] in `dtype`, read-only."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, size=(X, Y, 2)).astype(dtype)
    p = rng.integers(-8, 9, size=(X, Y)).astype(dtype)
    return _frozen(v), _frozen(p)


@functools.lru_cache(maxsize=None)
def float_fields(dtype, seed=21):
    """(v, p) of standard normal values in `dtype`, read-only: nothing about them is exact."""
    rng = np.random.default_rng(seed)
    return _frozen(rng.standard_normal((X, Y, 2)).astype(dtype)), _frozen(rng.standard_normal((X, Y)).astype(dtype))


@functools.lru_cache(maxsize=None)
def probes(n=NPROBES, seed=5):
    """n distinct fluid cells of the mask, int32 (n, 2), sorted as np.argwhere lists them."""
    fluid = np.argwhere(mask() == 0)
    idx = np.sort(np.random.default_rng(seed).choice(len(fluid), n, replace=False))
    return _frozen(fluid[idx].astype(np.int32))


def probe_values(v, p, pts):
    """(P, 3) float64: u, w, p at the probe cells - what a history record holds."""
    return np.stack([v[pts[:, 0], pts[:, 1], 0], v[pts[:, 0], pts[:, 1], 1], p[pts[:, 0], pts[:, 1]]], axis=1).astype(np.float64)


def face_terms(v, p, fc, centre, dx, inv_re):
    """Every face's contribution as loads_ref.sample_ref forms it, one IEEE double operation at a time in the same order, for all faces at
    once -> (per-face (4, F): pk, pk pk, tk, tk tk; record terms (F, 6): fpx, fpy, fvx, fvy, mp, mv).  No limit pass, no slab offset."""
    fc = np.asarray(fc)
    x, y, d = fc[:, 0], fc[:, 1], fc[:, 2]
    cx, cy = float(centre[0]), float(centre[1])
    dx, inv_re = np.float64(dx), np.float64(inv_re)
    mid = np.asarray(MID, np.float64)
    ax = ((x.astype(np.float64) + mid[d, 0]) - cx) * dx
    ay = ((y.astype(np.float64) + mid[d, 1]) - cy) * dx
    pk = p[x, y].astype(np.float64)
    xdir = d < 2
    ut = np.where(xdir, v[x, y, 1], v[x, y, 0]).astype(np.float64)
    tv = inv_re * ut
    tk = tv / dx
    tp = pk * dx
    zero = np.zeros(len(fc))
    fpx = np.where(d == 0, -tp, np.where(d == 1, tp, zero))
    fpy = np.where(d == 2, -tp, np.where(d == 3, tp, zero))
    fvx, fvy = np.where(xdir, zero, tv), np.where(xdir, tv, zero)
    mp = ax * fpy - ay * fpx
    mv = ax * fvy - ay * fvx
    return np.stack([pk, pk * pk, tk, tk * tk]), np.stack([fpx, fpy, fvx, fvy, mp, mv], axis=1)


def sample_vec(sums, v, p, fc, centre, dx, inv_re):
    """loads_ref.sample_ref without its Python loop (which takes most of a second per sample at 66,248 faces): the same bits in sums, record
    and scale.  The record is the running sum from 0.0 in face order, as the loop forms it (np.cumsum adds left to right)."""
    per_face, terms = face_terms(v, p, fc, centre, dx, inv_re)
    assert sums.shape == (NSUM, len(terms)) and terms.shape[1] == NREC
    sums += per_face
    lead = np.zeros((1, NREC))
    rec = np.cumsum(np.concatenate([lead, terms]), axis=0)[-1]
    scale = np.cumsum(np.concatenate([lead, np.abs(terms)]), axis=0)[-1]
    return rec, scale


def exact_forces(p, fc, dx):
    """(force_x, force_y) of a history record: sum over the faces of SIGNS[dir] * (double)p * dx, by np.sum (pairwise) - any order gives the
    same value on the exact fields."""
    from fs.history import SIGNS
    fc = np.asarray(fc)
    t = np.asarray(SIGNS)[fc[:, 2]] * (p[fc[:, 0], fc[:, 1]].astype(np.float64) * np.float64(dx))
    return float(np.sum(t[fc[:, 2] < 2])), float(np.sum(t[fc[:, 2] >= 2]))
