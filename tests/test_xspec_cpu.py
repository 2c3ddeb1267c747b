"""The cross-spectra without a GPU.  Part one: the detrend of a bin and the split-and-accumulate of csrc/fs_xspec.h, compiled by the host
compiler (libfs_xspec_host.so), against the NumPy restatement (tests/xspec_ref.py) with == on random planes of 8 x 8, 16 x 8 and 8 x 16 -
the bins a = 0, b = 0 and the Nyquist bins are their own mirrors.  Part two, on the restatement: the exact symmetries of the four planes and
Paa + Pbb against (|Z'[k]|^2 + |Z'[-k]|^2) / 2.  Part three: fs.spectra.cross_result on fields with a known answer."""
import ctypes
import os

import numpy as np
import pytest
from conftest import REPO

import spec_ref as S
import xspec_ref as XR

EPS = np.finfo(np.float64).eps
SHAPES = ((8, 8), (16, 8), (8, 16))


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_xspec_host.so"))
    dp, i, d = ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double
    lib.fs_xspec_host_detrend.argtypes = [dp, dp, i, i, i, d, d, dp, dp]
    lib.fs_xspec_host_accumulate.argtypes = [dp, dp, i, i, i, i, d, d, dp, dp, dp]
    return lib


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _planes(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.2, 1.0, shape), rng.normal(-0.1, 1.0, shape)


def test_limits(host):
    a, b = ctypes.c_int(), ctypes.c_int()
    host.fs_xspec_host_limits(ctypes.byref(a), ctypes.byref(b))
    assert (a.value, b.value) == (len(XR.QUANTITIES), XR.NPLANE) == (7, 4)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("detrend,c1", [(0, 0.0), (1, -0.5), (1, 0.0), (1, 0.37)])
def test_detrend_equals_the_restatement(shape, detrend, c1, host):
    re, im = _planes(shape, 1)
    out_re, out_im = np.empty(shape), np.empty(shape)
    host.fs_xspec_host_detrend(_dp(re), _dp(im), shape[0], shape[1], detrend, c1, 0.5 * c1, _dp(out_re), _dp(out_im))
    want = S.detrend(re, im, c1, 0.5 * c1) if detrend else (re, im)
    assert np.array_equal(out_re, want[0]) and np.array_equal(out_im, want[1])
    if detrend:
        assert out_re[0, 0] == 0 and out_im[0, 0] == 0 and (out_re != re).sum() == (9 if c1 else 1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("detrend,c1", [(0, 0.0), (1, -0.5)])
def test_accumulate_equals_the_restatement_over_three_samples(shape, pair, detrend, c1, host):
    nx, ny = shape
    acc = np.zeros((XR.NPLANE if pair else 1,) + shape)
    want = np.zeros_like(acc)
    for seed in (2, 3, 4):
        re, im = _planes(shape, seed)
        out_re, out_im = np.empty(shape), np.empty(shape)
        host.fs_xspec_host_accumulate(_dp(re), _dp(im), nx, ny, detrend, pair, c1, c1, _dp(out_re), _dp(out_im), _dp(acc))
        zre, zim = S.detrend(re, im, c1, c1) if detrend else (re, im)
        assert np.array_equal(out_re, zre) and np.array_equal(out_im, zim)
        want = XR.accumulate(want, zre, zim)
        assert np.array_equal(acc, want), (shape, pair, seed)
    # the bins that are their own mirrors - a in {0, Nx / 2} and b in {0, Ny / 2} - hold A = Z.re, B = Z.im: P = re^2, im^2, C = re im, 0
    for a in (0, nx // 2):
        for b in (0, ny // 2):
            assert XR.mirrored(np.arange(nx * ny).reshape(shape))[a, b] == a * ny + b
            if pair:
                assert acc[3, a, b] == 0
    assert acc.min() < 0 or not pair                     # (the co- and quadrature planes are signed)
    # the symmetries, on what the library's own text accumulated: a bin and its mirror add the same terms, sample after sample
    assert np.array_equal(acc[0], XR.mirrored(acc[0]))
    if pair:
        assert np.array_equal(acc[1], XR.mirrored(acc[1])) and np.array_equal(acc[2], XR.mirrored(acc[2]))
        assert np.array_equal(acc[3], -XR.mirrored(acc[3])) and np.abs(acc[3]).max() > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_library_sums_add_up_to_the_mirrored_power(shape, host):
    """Paa + Pbb of one sample out of fs_xspec_host_accumulate against (|Z'[k]|^2 + |Z'[-k]|^2) / 2 of the Z' it wrote: within 16 eps."""
    re, im = _planes(shape, 7)
    acc, out_re, out_im = np.zeros((XR.NPLANE,) + shape), np.empty(shape), np.empty(shape)
    host.fs_xspec_host_accumulate(_dp(re), _dp(im), shape[0], shape[1], 1, 1, -0.5, -0.5, _dp(out_re), _dp(out_im), _dp(acc))
    p = S.power_of(out_re, out_im)
    want = 0.5 * (p + XR.mirrored(p))
    assert np.all(np.abs((acc[0] + acc[1]) - want) <= 16 * EPS * want) and want.max() > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_symmetries_of_the_planes_are_exact(shape):
    """A[-k] = conj A[k] and B[-k] = conj B[k] bit for bit (the same sums and differences, commuted), so Paa, Pbb and Cre equal their mirrored
    planes and Cim is minus its mirrored plane; Paa + Pbb is (|Z'[k]|^2 + |Z'[-k]|^2) / 2 within 16 eps: both sides are at most about six
    roundings of sums of non-negative terms."""
    re, im = _planes(shape, 7)
    paa, pbb, cre, cim = XR.split_products(re, im)
    assert np.array_equal(paa, XR.mirrored(paa)) and np.array_equal(pbb, XR.mirrored(pbb)) and np.array_equal(cre, XR.mirrored(cre))
    assert np.array_equal(cim, -XR.mirrored(cim))
    p = S.power_of(re, im)
    want = 0.5 * (p + XR.mirrored(p))
    assert np.all(np.abs((paa + pbb) - want) <= 16 * EPS * want)


# ---- cross_result on fields with a known answer ------------------------------------------------------------------------------------------------
def _sums_of(a, b, window):
    """The accumulated planes of one sample of the real fields a, b (Nx, Ny) through the restatement's transform."""
    from fs import spectra
    nx, ny = a.shape
    wx, wy, twx, twy, _, _ = spectra.tables(nx, ny, window)
    re, im = S.fft2((a * wx[:, None]) * wy[None, :], (b * wx[:, None]) * wy[None, :], twx, twy)
    return XR.accumulate(np.zeros((4, nx, ny)), re, im)


def _result(sums, window="boxcar", dx=0.25, quantities=("u", "w")):
    from fs import spectra
    return spectra.cross_result(sums, 1, np.zeros(1, np.int64), (0, 0) + sums.shape[1:], quantities, window, False, dx)


def test_cross_result_keys_and_a_single_scalar():
    from fs import spectra
    a = np.random.default_rng(1).normal(size=(16, 8))
    sums = _sums_of(a, np.zeros_like(a), "hann")
    r = _result(sums, "hann")
    assert set(r) == {"quantities", "spectrum_a", "spectrum_b", "co", "quad", "kx", "ky", "k", "Sa", "Sb", "Co", "Quad", "coherence", "phase",
                      "samples", "sample_steps", "box", "window", "detrend", "sums"}
    wx, wy = spectra.window_table(16, "hann"), spectra.window_table(8, "hann")
    mean_sq = ((a * wx[:, None] * wy[None, :]) ** 2).sum() / ((wx * wx).sum() * (wy * wy).sum())
    assert abs(r["spectrum_a"].sum() - mean_sq) <= 64 * EPS * mean_sq          # Parseval: the window-weighted mean of a^2
    assert np.isnan(r["coherence"]).all() and not r["spectrum_b"].any()         # b = 0: the denominator is 0 in every shell
    one = spectra.cross_result(sums[:1], 1, np.zeros(1, np.int64), (0, 0, 16, 8), ("vorticity", None), "hann", False, 0.25)
    assert np.array_equal(one["spectrum_a"], r["spectrum_a"]) and np.array_equal(one["Sa"], r["Sa"]) and one["quantities"] == ("vorticity", None)
    for k in ("spectrum_b", "co", "quad", "Sb", "Co", "Quad", "coherence", "phase"):
        assert one[k] is None, k
    none = spectra.cross_result(np.zeros((4, 8, 8)), 0, np.zeros(0, np.int64), (0, 0, 8, 8), ("u", "w"), "hann", True, 0.25)
    assert not none["spectrum_a"].any() and none["samples"] == 0


def _bin_bound(r, nx, ny):
    """What a bin of co / quad / spectrum_b may be off by when both fields have the spectrum r["spectrum_a"] up to a factor: a radix-2
    transform is within 4 eps log2(Nx Ny) of the exact one in relative L2 norm (tests/test_gpu_spec.py), so every bin of A and of B is off by
    at most that times the plane's norm; a product of two such values by twice that times the square of the norm - the sum of spectrum_a -,
    and the split and the products add a few roundings more: (8 log2(Nx Ny) + 8) eps sum(spectrum_a)."""
    return (8 * np.log2(nx * ny) + 8) * EPS * r["spectrum_a"].sum()


def test_proportional_fields_have_coherence_one_and_no_quadrature():
    """b = c a: co = c spectrum_a, quad = 0, spectrum_b = c^2 spectrum_a within _bin_bound times the factor; coherence 1 in every shell."""
    from fs import spectra
    nx = ny = 16
    a = np.random.default_rng(2).normal(size=(nx, ny))
    c = -2.0
    r = _result(_sums_of(a, c * a, "hann"), "hann")
    tol = _bin_bound(r, nx, ny)
    assert np.abs(r["co"] - c * r["spectrum_a"]).max() <= abs(c) * tol
    assert np.abs(r["quad"]).max() <= abs(c) * tol
    assert np.abs(r["spectrum_b"] - c * c * r["spectrum_a"]).max() <= c * c * tol
    # a shell sums at most Nx Ny bins: Co, Quad, Sb are off by at most Nx Ny times the bin's bound (over dk); the coherence is a ratio of
    # products of two of them each, so four relative errors
    dk = r["k"][1]
    shells = np.bincount(np.floor(np.hypot(*np.meshgrid(r["kx"], r["ky"], indexing="ij")) / dk + 0.5).astype(int).ravel())
    live = r["Sa"] > 0
    rel = shells[live] * c * c * tol / dk / (c * c * r["Sa"][live])
    assert live.sum() > 4 and np.all(np.abs(r["coherence"][live] - 1.0) <= 4 * rel + 16 * EPS)
    assert np.all(np.abs(np.abs(r["phase"][live]) - np.pi) <= 2 * rel + 16 * EPS)      # c < 0: the fields are in antiphase
    assert spectra.shell_spectrum(r["co"], r["kx"], r["ky"])[1].tolist() == r["Co"].tolist()
    assert np.abs(spectra.shell_spectrum(r["quad"], r["kx"], r["ky"])[1]).max() <= nx * ny * abs(c) * tol / dk      # (odd: the plain sum cancels)


def test_shifted_field_has_coherence_one_and_phase_kx_s_dx():
    """b(x) = a(x - s dx) on a periodic field, boxcar window: B = A exp(-i kx s dx), so A conj(B) has the phase kx s dx in every bin (mod 2 pi)
    and |A| = |B|: the shell coherence is 1 wherever a shell's bins share one kx - and the coherence of ONE bin of one sample is 1 always."""
    nx, ny, s, dx = 32, 8, 3, 0.25
    a = np.random.default_rng(3).normal(size=(nx, ny))
    r = _result(_sums_of(a, np.roll(a, s, axis=0), "boxcar"), "boxcar", dx)
    tol = _bin_bound(r, nx, ny)
    mag = np.hypot(r["co"], r["quad"])
    big = mag >= 1.0e-3 * mag.max()
    assert big.sum() > nx * ny // 2
    want = (r["kx"][:, None] * s * dx) * np.ones((1, ny))
    diff = np.angle(np.exp(1j * (np.arctan2(r["quad"], r["co"]) - want)))
    assert np.all(np.abs(diff[big]) <= 2 * tol / mag[big])                        # (an error of tol in a value of size mag turns it by tol / mag)
    assert np.abs(r["spectrum_b"] - r["spectrum_a"]).max() <= tol
    # per bin, one sample: |A conj B|^2 = |A|^2 |B|^2 up to the roundings of the six products and sums behind either side
    per_bin = (r["co"] ** 2 + r["quad"] ** 2)[big] / (r["spectrum_a"] * r["spectrum_b"])[big]
    assert np.abs(per_bin - 1.0).max() <= 32 * EPS
    # shell coherence: a shell of the 2-D field holds bins of several kx, whose phases differ - it is 1 where every bin of a shell shares one
    # |kx|: a field that varies along x alone (ky = 0 only; kx's fundamental is the smaller one, so shell s is the pair of bins kx = +-s dk).
    # Quad sums the upper half twice (fs.spectra.upper_half): the plain sum of an odd plane over a shell would be 0 and the coherence cos^2
    line = _result(_sums_of(a[:, :1] * np.ones((1, ny)), np.roll(a[:, :1], s, axis=0) * np.ones((1, ny)), "boxcar"), "boxcar", dx)
    live = line["Sa"] > 1.0e-3 * line["Sa"].max()
    assert live.sum() >= nx // 4
    rel = nx * ny * _bin_bound(line, nx, ny) / line["k"][1] / line["Sa"][live]
    assert np.all(np.abs(line["coherence"][live] - 1.0) <= 4 * rel + 16 * EPS)
    shells = np.flatnonzero(live)
    shells = shells[(shells > 0) & (shells < nx // 2)]
    turn = np.angle(np.exp(1j * (line["phase"][shells] - line["k"][shells] * s * dx)))
    assert len(shells) >= nx // 4 and np.all(np.abs(turn) <= 2 * rel[np.isin(np.flatnonzero(live), shells)] + 16 * EPS)


def test_upper_half_takes_one_bin_of_every_mirror_pair():
    from fs import spectra
    for nx, ny in SHAPES:
        up = spectra.upper_half(nx, ny)
        own = XR.mirrored(np.arange(nx * ny).reshape(nx, ny)) == np.arange(nx * ny).reshape(nx, ny)
        assert own.sum() == 4 and not (up & own).any()
        assert np.array_equal(up ^ XR.mirrored(up), ~own)            # exactly one of k, -k


def test_pair_u_w_adds_up_to_twice_the_energy():
    """spectrum_a + spectrum_b of (u, w) against 2 energy of fs.spectra.result on the same plane: the 16 eps relation above."""
    from fs import spectra
    rng = np.random.default_rng(4)
    u, w = rng.normal(size=(16, 8)), rng.normal(size=(16, 8))
    wx, wy, twx, twy, c1x, c1y = spectra.tables(16, 8, "hann")
    re, im = S.detrend(*S.fft2((u * wx[:, None]) * wy[None, :], (w * wx[:, None]) * wy[None, :], twx, twy), c1x, c1y)
    x = spectra.cross_result(XR.accumulate(np.zeros((4, 16, 8)), re, im), 1, np.zeros(1, np.int64), (0, 0, 16, 8), ("u", "w"), "hann", True, 0.25)
    e = spectra.result(S.power_of(re, im), 1, np.zeros(1, np.int64), (0, 0, 16, 8), "hann", True, 0.25)
    assert np.all(np.abs((x["spectrum_a"] + x["spectrum_b"]) - 2.0 * e["energy"]) <= 16 * EPS * 2.0 * e["energy"])
    assert np.array_equal(x["kx"], e["kx"]) and np.array_equal(x["k"], e["k"])
