"""Grids, masks and start fields shared by the multigrid tests that leave the reference scenes (tests/test_multigrid_ref.py on the CPU,
tests/test_gpu_multigrid_shapes.py on the GPU): the same arrays on both sides, from fixed seeds.

Masks: the random-scene recipe of tests/test_gpu_random_masks.py (Bernoulli walls, a few thick blobs, 3 % inflow and 3 % outflow anywhere,
fluid on the domain edge); on grids with an extent of 8 or less, where its blobs do not fit, Bernoulli walls and the same inflow / outflow
without blobs.  Fields: uniform(-1, 1), drawn in float64 and rounded to the field dtype."""
import functools

import numpy as np

from test_gpu_random_masks import _random_scene

DT, DX = 0.05 / 32, 1.0 / 32

# (X, Y): level shapes
SHAPES = {(1088, 8): [(544, 4), (272, 2), (136, 1)], (1024, 8): [(512, 4), (256, 2), (128, 1)], (2112, 4): [(1056, 2), (528, 1)],
          (520, 16): [(260, 8), (130, 4), (65, 2)], (260, 24): [(130, 12), (65, 6)], (128, 16): [(64, 8), (32, 4), (16, 2), (8, 1)],
          (96, 64): [(48, 32), (24, 16), (12, 8), (6, 4), (3, 2)], (72, 40): [(36, 20), (18, 10), (9, 5)],
          (64, 8): [(32, 4), (16, 2), (8, 1)], (36, 20): [(18, 10), (9, 5)], (44, 6): [(22, 3)],
          (24, 96): [(12, 48), (6, 24), (3, 12)], (8, 8): [(4, 4), (2, 2), (1, 1)]}
DENSITIES = (0.0, 0.05, 0.15, 0.3)
IO_P = 0.03


def _seed(X, Y, wall_p):
    return X * 100000 + Y * 1000 + int(round(wall_p * 100))


@functools.lru_cache(maxsize=None)
def scene(X, Y, wall_p):
    """(const, mask) of the grid at a wall density; read-only."""
    rng = np.random.default_rng(_seed(X, Y, wall_p))
    if min(X, Y) > 8:
        const, mask, _ = _random_scene(rng, X, Y, wall_p, IO_P)
    else:
        mask = (rng.random((X, Y)) < wall_p).astype(np.uint8)
        io = rng.random((X, Y))
        mask[(io < IO_P) & (mask == 0)] = 2
        mask[(io > 1 - IO_P) & (mask == 0)] = 3
        const = np.zeros((X, Y, 2), np.float32)
        const[mask == 2] = rng.uniform(-1, 1, (int((mask == 2).sum()), 2)).astype(np.float32)
    for a in (const, mask):
        a.setflags(write=False)
    return const, mask


@functools.lru_cache(maxsize=None)
def fields(X, Y, wall_p, dtype):
    """(p.current, p.next, v) of dtype (a name), uniform(-1, 1); read-only."""
    rng = np.random.default_rng(_seed(X, Y, wall_p) + 7)
    out = tuple(rng.uniform(-1, 1, s).astype(dtype) for s in ((X, Y), (X, Y), (X, Y, 2)))
    for a in out:
        a.setflags(write=False)
    return out
