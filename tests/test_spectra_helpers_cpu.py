"""The NumPy helpers of fs.spectra, none of which needs a device: the normalisation of the result dict, the shell and line spectra, the
slope fit, the split of the packed plane and the wavenumbers."""
import numpy as np
import pytest


def _field(nx, ny, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(0.5, 1.0, (nx, ny)), rng.normal(-0.2, 1.0, (nx, ny))


@pytest.mark.parametrize("window", ["hann", "boxcar"])
@pytest.mark.parametrize("nx,ny", [(16, 8), (64, 64)])
def test_energy_sums_to_the_weighted_mean_and_shells_keep_it(nx, ny, window):
    from fs import spectra
    u, w = _field(nx, ny)
    wx, wy = spectra.window_table(nx, window), spectra.window_table(ny, window)
    win = wx[:, None] * wy[None, :]
    Z = np.fft.fft2((u + 1j * w) * win)
    dx = 1.0 / 64
    out = spectra.result(np.abs(Z) ** 2, 1, np.zeros(1, np.int64), (0, 0, nx, ny), window, False, dx)
    mean = (0.5 * (u * u + w * w) * win ** 2).sum() / (win ** 2).sum()
    assert out["energy"].sum() == pytest.approx(mean, rel=1e-12)
    assert np.allclose(out["power"], spectra.mirrored(out["power"]), rtol=1e-15, atol=0)
    dk = out["k"][1] - out["k"][0]
    assert dk == pytest.approx(2 * np.pi / (max(nx, ny) * dx)) and out["k"][0] == 0
    assert (out["E"] * dk).sum() == pytest.approx(out["energy"].sum(), rel=1e-12)
    for axis, n in ((0, nx), (1, ny)):
        line = spectra.line_spectrum(out["energy"], axis)
        assert line.shape == (n,) and line.sum() == pytest.approx(out["energy"].sum(), rel=1e-12)
    # two samples of the same plane: the mean is the plane
    two = spectra.result(2 * np.abs(Z) ** 2, 2, np.zeros(2, np.int64), (0, 0, nx, ny), window, False, dx)
    assert np.array_equal(two["power"], out["power"])
    empty = spectra.result(np.zeros((nx, ny)), 0, np.zeros(0, np.int64), (0, 0, nx, ny), window, False, dx)
    assert empty["samples"] == 0 and not empty["power"].any()


def test_power_is_the_two_component_spectrum():
    from fs import spectra
    u, w = _field(32, 16, 3)
    Z = np.fft.fft2(u + 1j * w)
    U, W = spectra.split(Z)
    assert np.allclose(U, np.fft.fft2(u), rtol=0, atol=1e-11) and np.allclose(W, np.fft.fft2(w), rtol=0, atol=1e-11)
    P = np.abs(Z) ** 2
    assert np.allclose(0.5 * (P + spectra.mirrored(P)), np.abs(U) ** 2 + np.abs(W) ** 2, rtol=1e-12, atol=1e-9)


def test_slope_recovers_a_power_law():
    from fs import spectra
    n, dx = 256, 1.0 / 256
    kx, ky = spectra.wavenumbers(n, n, dx)
    mag = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
    with np.errstate(divide="ignore"):
        energy = np.where(mag > 0, mag ** -4.0, 0.0)      # E(k) ~ 2 pi k * k^-4 = k^-3
    k, E = spectra.shell_spectrum(energy, kx, ky)
    assert abs(spectra.slope(k, E, 10 * k[1], 100 * k[1]) + 3.0) < 0.05
    kk = np.arange(1.0, 200.0)
    assert spectra.slope(kk, 7.0 * kk ** -3.0, 2.0, 150.0) == pytest.approx(-3.0, abs=1e-12)
    with pytest.raises(ValueError):
        spectra.slope(kk, kk, 1000.0, 2000.0)


def test_wavenumbers_and_tables():
    from fs import spectra
    kx, ky = spectra.wavenumbers(16, 8, 0.25)
    assert np.array_equal(kx, 2 * np.pi * np.fft.fftfreq(16, 0.25)) and np.array_equal(ky, 2 * np.pi * np.fft.fftfreq(8, 0.25))
    for n in (8, 4096):
        tw = spectra.twiddles(n)
        k = np.arange(n // 2)
        assert tw.shape == (n // 2, 2) and tw.flags.c_contiguous
        assert np.abs(tw[:, 0] - np.cos(2 * np.pi * k / n)).max() <= 2e-16 * 4 and np.abs(tw[:, 1] + np.sin(2 * np.pi * k / n)).max() <= 2e-16 * 4
        assert tw[n // 4].tolist() == [pytest.approx(0.0, abs=1e-19), -1.0]
    assert spectra.detrend_pair("hann") == -0.5 and spectra.detrend_pair("boxcar") == 0.0
    with pytest.raises(ValueError):
        spectra.line_spectrum(np.zeros((8, 8)), 2)
