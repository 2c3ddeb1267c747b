"""The scale-to-scale fluxes without a GPU.  Part one: the ordered window sum - one window, and the several-adjacent-windows form the kernels
run, at both of their register counts - and the per-cell flux function of csrc/fs_flux.h, compiled by the host compiler
(libfs_flux_host.so), against the NumPy restatement (tests/flux_ref.py) with == on random f32-valued and f64 inputs.  Part two, the
restatement itself against three facts derived without it: the exact discrete filter of a Fourier mode, the realisability of the sub-filter
stress of a filter with non-negative weights, and the Galilean invariance of PI and K.  Part three: fs.fluxes.flux_result."""
import ctypes
import os

import numpy as np
import pytest
from conftest import REPO

import flux_ref as FR

EPS = np.finfo(np.float64).eps
RS = (1, 2, 5, 13)


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_flux_host.so"))
    dp, i, d = ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double
    lib.fs_flux_host_limits.argtypes = [ctypes.POINTER(i)] * 10
    lib.fs_flux_host_window.argtypes = [dp, i, i, dp]
    lib.fs_flux_host_window_multi.argtypes = [dp, i, i, i, dp]
    lib.fs_flux_host_cell.argtypes = [dp, dp, dp, dp, dp, ctypes.c_longlong, d, dp, dp, dp]
    return lib


def limits(lib):
    v = [ctypes.c_int() for _ in range(10)]
    lib.fs_flux_host_limits(*[ctypes.byref(x) for x in v])
    return dict(zip(("nq", "sums", "max_widths", "max_r", "row_v", "col_v", "strip", "row_waves", "col_lanes", "lds_bytes"), [x.value for x in v]))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _values(n, kind, seed):
    x = np.random.default_rng(seed).normal(0.3, 1.0, n)
    return x.astype(np.float32).astype(np.float64) if kind == "f32" else x


def _fields(shape, kind, seed=5):
    rng = np.random.default_rng(seed)
    U, W, OM = rng.normal(0.3, 1.0, shape), rng.normal(-0.2, 1.0, shape), rng.normal(0.0, 3.0, shape)
    if kind == "f32":
        U, W, OM = (a.astype(np.float32).astype(np.float64) for a in (U, W, OM))
    return U, W, OM


def test_limits(host):
    L = limits(host)
    assert (L["nq"], L["sums"], L["max_widths"], L["max_r"]) == (FR.NQ, FR.NSUM, FR.MAX_WIDTHS, FR.MAX_R) == (8, 3, 8, 64)
    assert L["row_v"] % 2 == 1 and L["strip"] == 64 * L["row_v"]
    assert L["lds_bytes"] == L["row_waves"] * (L["strip"] + 2 * L["max_r"]) * 8 <= 64 * 1024


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 7, 8, 13, 31, 64])
def test_window_sums_equal_the_restatement(r, kind, host):
    """One window at a time, and 7 and 16 adjacent windows at a time: n below, at and above the number of windows of a lane."""
    L = limits(host)
    n, count = 2 * r + 1, L["row_v"] * L["col_v"] * 2
    q = _values(count + n - 1, kind, 7 + r)
    want = FR.window_sums(q, r, 0)
    assert want.shape == (count,)
    one = np.empty(count)
    host.fs_flux_host_window(_dp(q), count, n, _dp(one))
    assert np.array_equal(one, want)
    for v in (L["row_v"], L["col_v"]):
        got = np.full(count, np.nan)
        assert host.fs_flux_host_window_multi(_dp(q), count, n, v, _dp(got)) == 0
        assert np.array_equal(got, want), (r, v)
    # the order matters: the reversed sum differs somewhere, so == above tells the orders apart (sums of a few f32 values are exact in double)
    if kind == "f64":
        assert (FR.window_sums(q[::-1], r, 0)[::-1] != want).any()


def test_a_window_starts_with_its_first_value(host):
    """No 0 + x: a window of -0.0 alone keeps its sign."""
    v = limits(host)["col_v"]
    q = np.full(2 * v + 2, -0.0)
    out = np.empty(2 * v)
    assert host.fs_flux_host_window_multi(_dp(q), 2 * v, 3, v, _dp(out)) == 0
    assert np.signbit(out).all() and np.signbit(FR.window_sums(q, 1, 0)).all()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_cell_function_equals_the_restatement(kind, host):
    cells = 500
    c = _values(cells * 8, kind, 1).reshape(cells, 8)
    nb = [_values(cells * 3, kind, 2 + k).reshape(cells, 3) for k in range(4)]
    two_dx = 2.0 / 64
    pi, zf, k = np.empty(cells), np.empty(cells), np.empty(cells)
    host.fs_flux_host_cell(_dp(c), *[_dp(a) for a in nb], cells, two_dx, _dp(pi), _dp(zf), _dp(k))
    want = FR.cell(c.T, *[a.T for a in nb], two_dx)
    assert np.array_equal(pi, want[0]) and np.array_equal(zf, want[1]) and np.array_equal(k, want[2])
    assert (pi > 0).any() and (pi < 0).any()


# ---- the restatement against facts derived without it -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 4, 13])
def test_filter_of_a_fourier_mode_is_the_dirichlet_kernel(r):
    """u = sin(kx x) cos(ky y) on the cell centres of a 96 x 64 grid: F0 = D(kx) D(ky) u with D(k) = sin(n k dx / 2) / (n sin(k dx / 2))."""
    X, Y, dx, kx, ky = 96, 64, 1.0 / 64, 6 * np.pi, 10 * np.pi
    x, y = (np.arange(X) + 0.5) * dx, (np.arange(Y) + 0.5) * dx
    u = np.sin(kx * x)[:, None] * np.cos(ky * y)[None, :]
    n = 2 * r + 1
    D = lambda k: np.sin(n * k * dx / 2) / (n * np.sin(k * dx / 2))
    F0 = FR.filtered(FR.base_of(u, np.zeros_like(u), np.zeros_like(u)), r)[0]
    err = np.abs(F0 - D(kx) * D(ky) * u)[r:X - r, r:Y - r].max()
    print("r", r, "error / eps", err / EPS)
    assert err <= 16 * EPS
    assert not F0[:r].any() and not F0[:, Y - r:].any()


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("r", RS)
def test_the_subfilter_stress_is_realisable(r, kind):
    """Non-negative weights: tuu >= 0, tww >= 0 and tuu tww - tuw^2 >= 0."""
    U, W, OM = _fields((64, 32), kind)
    F = FR.filtered(FR.base_of(U, W, OM), r)[:, r:64 - r, r:32 - r]
    tuu, tuw, tww = FR.stresses(F)
    print("r", r, "minima", tuu.min(), tww.min(), (tuu * tww - tuw * tuw).min())
    assert tuu.min() >= 0 and tww.min() >= 0 and (tuu * tww - tuw * tuw).min() >= 0


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("r", RS)
def test_pi_and_k_are_galilean_invariant(r, kind):
    """(U, W) + (3.0, -2.0) with OM unchanged moves PI by at most 8 n eps V^2 S and K by at most 8 n eps V^2."""
    shape, dx = (64, 32), 1.0 / 32
    U, W, OM = _fields(shape, kind)
    n = 2 * r + 1
    Fa = FR.filtered(FR.base_of(U, W, OM), r)
    Fb = FR.filtered(FR.base_of(U + 3.0, W - 2.0, OM), r)
    a, b = FR.fluxes(Fa, r, dx), FR.fluxes(Fb, r, dx)
    x0, y0, x1, y1 = FR.valid_rect(shape, r)
    assert x0 < x1 and y0 < y1 and np.abs(a[0]).max() > 0
    V = 5 + np.abs(U).max() + np.abs(W).max()
    gx = (Fa[:2, x0 + 1:x1 + 1, y0:y1] - Fa[:2, x0 - 1:x1 - 1, y0:y1]) / (2.0 * dx)
    gy = (Fa[:2, x0:x1, y0 + 1:y1 + 1] - Fa[:2, x0:x1, y0 - 1:y1 - 1]) / (2.0 * dx)
    S = max(np.abs(gx).max(), np.abs(gy).max())                  # the largest filtered gradient of the case
    dpi, dk = np.abs(a[0] - b[0]).max(), np.abs(a[2] - b[2]).max()
    print("r", r, "PI moved by", dpi / (n * EPS * V * V * S), "K by", dk / (n * EPS * V * V), "(units of n eps V^2 S, n eps V^2)")
    assert dpi <= 8 * n * EPS * V * V * S and dk <= 8 * n * EPS * V * V


# ---- the result dict ----------------------------------------------------------------------------------------------------------------------------
def test_flux_result_means_over_the_common_and_the_own_rectangle():
    from fs import fluxes
    shape, box, hw, dx = (40, 30), (2, 1, 38, 28), (1, 5), 0.5
    sums = np.zeros((2, 3, 36, 27))
    rects = [fluxes.valid_rect(box, r, shape) for r in hw]
    assert rects == [(2, 2, 38, 28), (6, 6, 34, 24)] == [FR.valid_rect(shape, r, box) for r in hw]
    rng = np.random.default_rng(0)
    for k, (x0, y0, x1, y1) in enumerate(rects):
        sums[k, :, x0 - 2:x1 - 2, y0 - 1:y1 - 1] = rng.normal(size=(3, x1 - x0, y1 - y0))
    out = fluxes.flux_result(sums, 4, np.arange(4), box, hw, dx, shape)
    assert out["half_widths"] == hw and out["widths"].tolist() == [1.5, 5.5] and out["valid"] == rects and out["samples"] == 4
    for n, name in enumerate(fluxes.PLANES):
        assert np.array_equal(out[name], sums[:, n] / 4) and out[name].shape == (2, 36, 27)
        cx0, cy0, cx1, cy1 = rects[1]
        for k, (x0, y0, x1, y1) in enumerate(rects):
            assert out["mean_" + name][k] == pytest.approx((sums[k, n] / 4)[cx0 - 2:cx1 - 2, cy0 - 1:cy1 - 1].mean(), rel=1e-14)
            assert out["mean_own"][name][k] == pytest.approx((sums[k, n] / 4)[x0 - 2:x1 - 2, y0 - 1:y1 - 1].mean(), rel=1e-14)
    zero = fluxes.flux_result(np.zeros_like(sums), 0, np.arange(0), box, hw, dx, shape)
    assert not zero["pi"].any() and zero["samples"] == 0 and not zero["mean_pi"].any()
