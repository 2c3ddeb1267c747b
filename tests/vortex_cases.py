"""The large grid of the vortex tests and its two velocity fields, shared by the CPU test of the cases themselves
(tests/test_vortex_cases_cpu.py) and the GPU tests (tests/test_gpu_vortices_large.py): the same arrays on both sides, from a fixed seed or
a formula.  Imports no fs at module level.

TALL = (1030, 262) with the random scene of tests/multigrid_cases.py at wall density 0.15: 269,860 cells.  By the geometry of
csrc/fs_vortex.h: 264 blocks of 1024 cells (k_vortex_scan: chunk = ceil(264 / 256) = 2, lanes 132 and up are empty); 1055 blocks of
k_vortex_reduce (the slot index blockIdx % 256 wraps four times); 33 x 33 tiles of 32 x 8 cells with a partial last tile each way; 5 column
blocks of 256; 4 rows per workgroup of k_vortex_flags at the default floor (66 workgroups down the grid, the last of 2 rows), 16 under
FS_DIAG_WGS = 85 (17 workgroups, the last of 6 rows: one full row group and a partial one of 2).

random_field: uniform(-1, 1) - tens of thousands of small components (more than 1024 pass, more than any max_components below 2^15 drops
cells).  rotation_field: two counter-rotating solid bodies, every value exact in f32, on an all-fluid mask with one small wall block: two
components of about 134,000 cells each whose waves lie wholly in one component by the thousand, |q| = 2^29 on every interior cell (ties
for the peak by the thousand), sum |q| above 2^46 and a non-zero `>> 32` part of the moment sums."""
import functools

import numpy as np

TALL = (1030, 262, 0.15)
ROT_DX = 1.0 / 256
ROT_OMEGA = 128.0              # |vorticity| of the interior of rotation_field: ((w_r - w_l) - (u_n - u_m)) / (2 dx) = (0.5 + 0.5) * 128
ROT_CX, ROT_CY = 515, 131      # the sense of rotation changes at column ROT_CX
ROT_WALL = (slice(500, 503), slice(100, 140))


def _frozen(a):
    a.setflags(write=False)
    return a


def tall_scene():
    """(const, mask) of the random scene; read-only."""
    from multigrid_cases import scene
    return scene(*TALL)


@functools.lru_cache(maxsize=None)
def random_field(dtype):
    """uniform(-1, 1) of shape (X, Y, 2), drawn in float64 and rounded to dtype (a name); read-only."""
    X, Y, _ = TALL
    return _frozen(np.random.default_rng(5).uniform(-1, 1, (X, Y, 2)).astype(dtype))


@functools.lru_cache(maxsize=None)
def rotation_field(dtype):
    """u = -s 0.25 (j - 131), w = s 0.25 (i - 515) with s = +1 for i < 515 and -1 from there on: multiples of 0.25 below 2^8, exact in f32.
    With dx = 1 / 256 the central differences give a vorticity of exactly +-128 away from column 515 and the domain edge; read-only."""
    X, Y, _ = TALL
    i, j = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    s = np.where(i < ROT_CX, 1.0, -1.0)
    v = np.stack([-s * 0.25 * (j - ROT_CY), s * 0.25 * (i - ROT_CX)], axis=-1)
    out = v.astype(dtype)
    assert np.array_equal(out.astype(np.float64), v)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def rotation_scene():
    """(const, mask) for rotation_field: all fluid but a wall block of 3 x 40 cells; read-only."""
    X, Y, _ = TALL
    mask = np.zeros((X, Y), np.uint8)
    mask[ROT_WALL] = 1
    return _frozen(np.zeros((X, Y, 2), np.float32)), _frozen(mask)


def rotation_exponent():
    """omega_max = 1.5 * 128 -> e = 8: q = om * 2^22, so |q| = 2^29 on the interior cells and nothing clips."""
    from vortex_ref import omega_exponent
    return omega_exponent(1.5 * ROT_OMEGA)
