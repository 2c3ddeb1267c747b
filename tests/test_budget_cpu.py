"""The kinetic-energy budget without a GPU: the per-cell function of csrc/fs_budget.h as the host compiler builds it
(libfs_budget_host.so: the text the kernel runs, with limit_cell and vortex_grad of fs_cell.h behind it) against the NumPy restatement
(tests/budget_ref.py) with ==; the header's constants against fs/budgets.py; and fs.budgets.derive_budget / momentum_balance against a
direct two-pass computation over a synthetic ensemble whose differences and Laplacian are written out in this file, cell by cell."""
import ctypes
import os

import numpy as np
import pytest

import budget_ref as BR
from conftest import REPO

HOST = os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_budget_host.so")


def _lib():
    lib = ctypes.CDLL(HOST)
    for name, t in (("fs_budget_host_cell_f32", ctypes.c_float), ("fs_budget_host_cell_f64", ctypes.c_double)):
        f = getattr(lib, name)
        f.argtypes = [ctypes.POINTER(t), ctypes.c_longlong, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
        f.restype = None
    return lib


def limits(lib=None):
    lib = lib or ctypes.CDLL(HOST)
    names = ("planes", "state", "inputs", "cells", "rows0", "rows", "pad", "lds_bytes")
    v = [ctypes.c_int() for _ in names]
    lib.fs_budget_host_limits(*[ctypes.byref(x) for x in v])
    return dict(zip(names, (x.value for x in v)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("limit", [None, 10.0])
def test_the_exported_cell_function_equals_the_restatement(dtype, limit):
    rng = np.random.default_rng(5)
    n = 4096
    inp = rng.standard_normal((n, 11)).astype(dtype)
    inp[n // 2:] *= dtype(12.0)                     # speeds above 10: the limit bites on the cell and on its neighbours
    two_dx = 2.0 / 24.0
    out = np.empty((n, BR.NPLANE), np.float64)
    ct = ctypes.c_float if dtype == np.float32 else ctypes.c_double
    fn = getattr(_lib(), "fs_budget_host_cell_f32" if dtype == np.float32 else "fs_budget_host_cell_f64")
    fn(inp.ctypes.data_as(ctypes.POINTER(ct)), n, 0.0 if limit is None else limit, two_dx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    want = BR.cells(inp, two_dx, limit)
    assert want.shape == out.shape and np.array_equal(out, want)
    if limit is not None:
        free = BR.cells(inp, two_dx, None)
        assert (np.abs(want[:, 0]) != np.abs(free[:, 0])).sum() > n // 4 and (want[:, 12] != free[:, 12]).sum() > n // 4, "the limit did not bite"
        assert np.all(np.hypot(want[:, 0], want[:, 1]) <= 10.0 * (1 + 1e-6))


def test_the_headers_constants_match_the_host_module():
    import fs
    from fs import budgets
    from fs.ride_ops import RideOps
    lim = limits()
    assert lim["planes"] == budgets.NPLANE == len(budgets.PLANES) == RideOps.BUDGET_NPLANE == BR.NPLANE == 21
    assert budgets.BYTES_PER_CELL == 8 * lim["planes"] == 168 and budgets.PLANES == BR.NAMES
    assert lim["state"] == 2 and lim["inputs"] == 11 and lim["lds_bytes"] == 0
    assert lim["cells"] == 2 and lim["rows0"] % lim["cells"] == 0 and lim["rows"] % lim["rows0"] == 0 and lim["pad"] % 2 == 0
    assert fs._lib.ABI_VERSION >= 28 and {"fs_budget_create", "fs_budget_launch", "fs_budget_read", "fs_budget_get", "fs_budget_set",
                                          "fs_budget_reset", "fs_budget_free"} <= set(fs._lib.EXPORTS)


# ---- derive_budget against a two-pass ensemble computation --------------------------------------------------------------------------------
NS, X, Y, DX, RE = 32, 48, 24, 1.0 / 24.0, 100.0
WALL = (10, 7)


def _smooth(rng, lo=0.1, hi=1.0):
    """A smooth random field on the grid with amplitude in [lo, hi]."""
    x, y = np.meshgrid(np.arange(X) * DX, np.arange(Y) * DX, indexing="ij")
    f = np.zeros((X, Y))
    for _ in range(4):
        kx, ky = rng.integers(1, 4, 2)
        f += rng.uniform(-1, 1) * np.sin(np.pi * kx * x / (X * DX) + rng.uniform(0, 2 * np.pi)) * np.cos(np.pi * ky * y / (Y * DX) + rng.uniform(0, 2 * np.pi))
    return rng.uniform(lo, hi) * f / np.abs(f).max()


@pytest.fixture(scope="module")
def ensemble():
    rng = np.random.default_rng(11)
    mean = [rng.uniform(0.1, 1.0) + _smooth(rng) for _ in range(3)]
    mask = np.zeros((X, Y), np.uint8)
    mask[WALL] = 1
    st = BR.State((0, 0, X, Y), DX, 1, 0)
    raw = []
    for _ in range(NS):
        u, w, p = (m + _smooth(rng) for m in mean)
        v = np.stack([u, w], axis=-1)
        st.launch(v, p, mask)
        raw.append(BR.values(v, p, DX)[[0, 1, 2, 12, 13, 14, 15]])
    return st.sums, mask == 0, np.array(raw)


# The reference's own stencils, written out cell by cell - nothing of fs.budgets is used on this side of the comparison.  x is the first
# index of every (X, Y) array.  Cells at the edge of the box get 0: they are not valid, so no term reads them.
def _dx_of(f):
    out = np.zeros((X, Y))
    for i in range(1, X - 1):
        for j in range(Y):
            out[i, j] = (f[i + 1, j] - f[i - 1, j]) / (2.0 * DX)
    return out


def _dy_of(f):
    out = np.zeros((X, Y))
    for i in range(X):
        for j in range(1, Y - 1):
            out[i, j] = (f[i, j + 1] - f[i, j - 1]) / (2.0 * DX)
    return out


def _lap_of(f):
    out = np.zeros((X, Y))
    for i in range(1, X - 1):
        for j in range(1, Y - 1):
            out[i, j] = (f[i + 1, j] + f[i - 1, j] + f[i, j + 1] + f[i, j - 1] - 4.0 * f[i, j]) / (DX * DX)
    return out


def _valid_of(fluid):
    out = np.zeros((X, Y), bool)
    for i in range(X):
        for j in range(Y):
            out[i, j] = all(0 <= a < X and 0 <= b < Y and fluid[a, b] for a, b in ((i, j), (i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)))
    return out


def test_the_references_stencils_on_fields_with_known_derivatives():
    """What pins the reference itself: on f = 3 x - 5 y + 2 x^2 + 7 y^2 (x = i dx, y = j dx) the central differences are exact - 3 + 4 x
    and -5 + 14 y - and so is the 5-point Laplacian, 4 + 14 = 18."""
    x, y = np.meshgrid(np.arange(X) * DX, np.arange(Y) * DX, indexing="ij")
    f = 3.0 * x - 5.0 * y + 2.0 * x * x + 7.0 * y * y
    inner = np.zeros((X, Y), bool)
    inner[1:-1, 1:-1] = True
    assert np.allclose(_dx_of(f)[inner], (3.0 + 4.0 * x)[inner], rtol=0, atol=1e-11)
    assert np.allclose(_dy_of(f)[inner], (-5.0 + 14.0 * y)[inner], rtol=0, atol=1e-11)
    assert np.allclose(_lap_of(f)[inner], 18.0, rtol=0, atol=1e-9)


def _moments(raw):
    """Two-pass: the ensemble means, then the fluctuations about them."""
    M = raw.mean(axis=0)
    return M, [raw[:, k] - M[k] for k in range(7)]


def _two_pass(raw, fluid):
    M, (u, w, p, ux, uy, wx, wy) = _moments(raw)
    U, W, P, Ux, Uy, Wx, Wy = M
    avg = lambda a: a.mean(axis=0)
    uu, ww, uw = avg(u * u), avg(w * w), avg(u * w)
    k = 0.5 * (uu + ww)
    t = {"production": -(uu * Ux + uw * (Uy + Wx) + ww * Wy),
         "dissipation": (avg(ux * ux) + avg(uy * uy) + avg(wx * wx) + avg(wy * wy)) / RE,
         "pressure_dilatation": avg(p * (ux + wy)),
         "convection": -(U * _dx_of(k) + W * _dy_of(k)),
         "turbulent_transport": -(_dx_of(0.5 * (avg(u * u * u) + avg(w * w * u))) + _dy_of(0.5 * (avg(u * u * w) + avg(w * w * w)))),
         "pressure_diffusion": -(_dx_of(avg(p * u)) + _dy_of(avg(p * w))),
         "viscous_diffusion": _lap_of(k) / RE}
    valid = _valid_of(fluid)
    for name in t:
        t[name] = np.where(fluid if name in ("production", "dissipation", "pressure_dilatation") else valid, t[name], 0.0)
    t["residual"] = np.where(valid, t["convection"] + t["production"] - t["dissipation"] + t["turbulent_transport"] + t["pressure_diffusion"]
                             + t["pressure_dilatation"] + t["viscous_diffusion"], 0.0)
    return t


def _two_pass_momentum(raw, fluid):
    """The mean momentum equation's terms from the ensemble, by the stencils above."""
    M, (u, w, *_rest) = _moments(raw)
    U, W, P, Ux, Uy, Wx, Wy = M
    avg = lambda a: a.mean(axis=0)
    uu, ww, uw = avg(u * u), avg(w * w), avg(u * w)
    valid = _valid_of(fluid)
    t = {"u": {"convection": -(U * Ux + W * Uy), "pressure_gradient": -_dx_of(P), "viscous": _lap_of(U) / RE,
               "reynolds_stress": -(_dx_of(uu) + _dy_of(uw))},
         "w": {"convection": -(U * Wx + W * Wy), "pressure_gradient": -_dy_of(P), "viscous": _lap_of(W) / RE,
               "reynolds_stress": -(_dx_of(uw) + _dy_of(ww))}}
    return {c: {k: np.where(valid, a, 0.0) for k, a in terms.items()} for c, terms in t.items()}


def test_derive_budget_agrees_with_a_two_pass_ensemble_computation(ensemble):
    """Bound 1e-10 max|term|: raw moments of O(1) values over 32 samples carry at most about 32 x 1.1e-16 = 4e-15 of rounding each, a
    difference over 2 dx = 1/12 multiplies that by 12, and the terms are no smaller than about 1e-3: three orders of margin."""
    from fs.budgets import TERMS, derive_budget
    sums, fluid, raw = ensemble
    out = derive_budget(sums, NS, fluid, DX, RE)
    want = _two_pass(raw, fluid)
    assert set(TERMS) == set(want)
    worst = 0.0
    for name in TERMS:
        scale = np.abs(want[name]).max()
        ratio = np.abs(out[name] - want[name]).max() / scale
        print(f"{name}: max|term| {scale:.3e}, largest difference / max|term| {ratio:.3e}")
        worst = max(worst, ratio)
        assert scale >= 1e-3, (name, scale)
        assert ratio <= 1e-10, (name, ratio)
    print(f"largest ratio {worst:.3e}")
    assert np.isclose(out["totals"]["production"], want["production"][out["valid"]].sum() * DX * DX, rtol=1e-9, atol=0.0)
    assert out["k"].min() >= 0.0 and out["dissipation"].min() >= 0.0


def test_where_the_terms_are_defined(ensemble):
    from fs.budgets import derive_budget, momentum_balance
    sums, fluid, raw = ensemble
    out = derive_budget(sums, NS, fluid, DX, RE)
    assert not fluid[WALL] and fluid.sum() == X * Y - 1 and np.array_equal(out["fluid"], fluid)
    for name in ("production", "dissipation", "pressure_dilatation"):
        assert np.all(out[name][fluid] != 0.0) and out[name][WALL] == 0.0, name
    # valid: exactly the cells without a non-fluid or out-of-box neighbour (and fluid themselves)
    want = _valid_of(fluid)
    assert np.array_equal(out["valid"], want) and want.sum() == (X - 2) * (Y - 2) - 5
    for name in ("convection", "turbulent_transport", "pressure_diffusion", "viscous_diffusion", "residual"):
        assert not out[name][~want].any() and np.abs(out[name][want]).max() > 0, name
    mb = momentum_balance(out, DX, RE)
    assert set(mb) == {"u", "w"}
    for t in mb.values():
        assert set(t) == {"convection", "pressure_gradient", "viscous", "reynolds_stress", "residual"}
        assert np.array_equal(t["residual"], t["convection"] + t["pressure_gradient"] + t["viscous"] + t["reynolds_stress"])
        assert not t["residual"][~want].any() and all(np.abs(a[want]).max() > 0 for a in t.values())
    # every term of both components against the ensemble and the test's own stencils, within the bound of the budget's terms
    ref = _two_pass_momentum(raw, fluid)
    for c in ("u", "w"):
        for name, a in ref[c].items():
            scale = np.abs(a).max()
            ratio = np.abs(mb[c][name] - a).max() / scale
            print(f"momentum {c} {name}: max|term| {scale:.3e}, largest difference / max|term| {ratio:.3e}")
            assert scale >= 1e-3 and ratio <= 1e-10, (c, name, scale, ratio)
    # before the first sample the result holds the same keys, all zeros
    from fs.budgets import DERIVED, TERMS, budget_result
    full = budget_result(sums, NS, np.arange(NS), (0, 0, X, Y), fluid, DX, RE)
    empty = budget_result(np.zeros_like(sums), 0, np.zeros(0, np.int64), (0, 0, X, Y), fluid, DX, RE)
    assert set(full) == set(empty) and set(DERIVED + TERMS) <= set(empty) and set(out) == set(DERIVED + TERMS) | {"totals", "fluid", "valid"}
    assert all(empty[k].shape == (X, Y) and not empty[k].any() for k in DERIVED + TERMS) and not any(empty["totals"].values())
    with pytest.raises(ValueError, match="no samples"):
        derive_budget(sums, 0, fluid, DX, RE)
    with pytest.raises(ValueError, match="shape"):
        derive_budget(sums[:20], NS, fluid, DX, RE)
