"""The field distributions without a GPU: the bin rule, the order-preserving key and the digit pick that the kernels and fs_dist_select run
(csrc/fs_dist.h, compiled by the host compiler into libfs_dist_host.so) against the restatement (tests/dist_ref.py) and NumPy's sort; the
binding; the quantile arithmetic of fs.dist."""
import ctypes
import os

import numpy as np
import pytest
from conftest import REPO

import dist_ref as D

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_dist_host.so"))
        vp, i, d, ll, ull = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong, ctypes.c_ulonglong
        ip = ctypes.POINTER(ctypes.c_int)
        for name, args, res in (("fs_dist_host_limits", [ip, ip, ip, ip], None), ("fs_dist_host_bins", [vp, i, d, d, i, vp], None),
                                ("fs_dist_host_keys", [vp, i, vp], None), ("fs_dist_host_unkeys", [vp, i, vp], None),
                                ("fs_dist_host_digit", [i, ip, ip], None), ("fs_dist_host_digits", [vp, i, ull, i, vp], None),
                                ("fs_dist_host_pick", [vp, i, ll, ctypes.POINTER(ll)], i)):
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = args, res
    return _lib


def host_bins(x, lo, hi, B):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty(len(x), np.int32)
    lib().fs_dist_host_bins(x.ctypes.data, len(x), lo, hi, B, out.ctypes.data)
    return out.astype(np.int64)


def host_keys(x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty(len(x), np.uint64)
    lib().fs_dist_host_keys(x.ctypes.data, len(x), out.ctypes.data)
    return out


def host_unkeys(k):
    k = np.ascontiguousarray(k, np.uint64)
    out = np.empty(len(k), np.float64)
    lib().fs_dist_host_unkeys(k.ctypes.data, len(k), out.ctypes.data)
    return out


def host_pick(table, rank):
    table = np.ascontiguousarray(table, np.int64)
    within = ctypes.c_longlong(-1)
    d = lib().fs_dist_host_pick(table.ctypes.data, len(table), rank, ctypes.byref(within))
    return d, within.value


def test_limits_and_digit_geometry_are_the_restatements():
    a, b, c, p = (ctypes.c_int() for _ in range(4))
    lib().fs_dist_host_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(p))
    assert (a.value, b.value, c.value, p.value) == (D.MAX_BINS, D.MAX_CHANNELS, D.MAX_RANKS, 6)
    total = 0
    for k in range(6):
        s, w = ctypes.c_int(), ctypes.c_int()
        lib().fs_dist_host_digit(k, ctypes.byref(s), ctypes.byref(w))
        assert (s.value, w.value) == D.digit_geometry(k)
        total += w.value
    assert total == 64 and D.digit_geometry(0) == (53, 11) and D.digit_geometry(5) == (0, 9)


RANGES = [(-1.0, 1.0, 4096), (0.1, 0.7, 63), (0.0, 1.0, 1), (-256.0, 256.0, 4096), (-3.5, 9.25, 64), (1.0e-300, 3.0e-300, 7), (-1.0e300, 1.0e300, 5)]


def _probe_values(lo, hi, B):
    edges = lo + (hi - lo) * (np.arange(B + 1) / B)
    edges[0], edges[-1] = lo, hi
    x = [edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), 0.5 * (edges[:-1] + edges[1:]),
         [lo, np.nextafter(lo, -np.inf), hi, np.nextafter(hi, 0.0) if hi > 0 else np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf)],
         [np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 1.7e308, -1.7e308],
         np.random.default_rng(B).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), 2000)]
    return np.concatenate([np.asarray(a, np.float64) for a in x])


@pytest.mark.parametrize("lo,hi,B", RANGES)
def test_bin_rule_of_the_host_object_equals_the_restatement(lo, hi, B):
    x = _probe_values(lo, hi, B)
    got, want = host_bins(x, lo, hi, B), D.bins_of(x, lo, hi, B)
    assert np.array_equal(got, want), (x[got != want][:5], got[got != want][:5], want[got != want][:5])
    assert got[np.isnan(x)].tolist() == [D.NAN] * int(np.isnan(x).sum())
    assert (got[x == np.inf] == D.ABOVE).all() and (got[x == -np.inf] == D.BELOW).all()
    assert (got[(x >= lo) & (x < hi)] >= 0).all() and got.max() <= B - 1
    # counts, tails and nan sum to the number of values
    h = D.histogram(x, lo, hi, B)
    assert h["counts"].sum() + h["below"] + h["above"] + h["nan"] == len(x)
    assert np.array_equal(h["counts"], np.bincount(got[got >= 0], minlength=B))


def test_the_largest_double_below_hi_needs_the_clamp():
    """(-1, 1, 4096): nextafter(1, 0) scales to exactly 4096.0 - without the clamp it would leave the table."""
    x = np.nextafter(1.0, 0.0)
    assert np.floor((x - -1.0) * (4096 / 2.0)) == 4096.0
    assert host_bins([x, -1.0, np.nextafter(-1.0, -np.inf), 1.0], -1.0, 1.0, 4096).tolist() == [4095, 0, D.BELOW, D.ABOVE]
    y = np.nextafter(0.7, 0.0)
    assert host_bins([y, 0.1, np.nextafter(0.1, -np.inf), 0.7], 0.1, 0.7, 63).tolist() == [62, 0, D.BELOW, D.ABOVE]
    assert D.bins_of([x], -1.0, 1.0, 4096).tolist() == [4095] and D.bins_of([y], 0.1, 0.7, 63).tolist() == [62]


SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1.0, -1.0, 1.0, np.inf, -np.inf, 1.7976931348623157e308,
                     -1.7976931348623157e308, 128.0, 128.0, 128.0, -128.0, -128.0, 0.1, np.nextafter(0.1, 1.0)])


def test_key_round_trip_and_order():
    x = np.concatenate([SPECIALS, np.random.default_rng(1).normal(0, 1e3, 500), np.random.default_rng(2).uniform(-1e-310, 1e-310, 100)])
    k = host_keys(x)
    assert np.array_equal(k, D.keys(x))
    back = host_unkeys(k)
    assert np.array_equal(back.view(np.uint64), x.view(np.uint64)), "the inverse key does not give the bits back"
    assert np.array_equal(D.unkeys(k).view(np.uint64), x.view(np.uint64))
    # the order of the keys is the order of the values; -0.0 sorts below +0.0 (distinct keys, equal values); ties share a key
    order = np.argsort(k, kind="stable")
    assert np.array_equal(x[order], np.sort(x))
    assert host_keys([-0.0])[0] + 1 == host_keys([0.0])[0]
    i, j = np.meshgrid(np.arange(len(x)), np.arange(len(x)), indexing="ij")
    assert np.array_equal(k[i] < k[j], (x[i] < x[j]) | ((x[i] == 0) & (x[j] == 0) & np.signbit(x[i]) & ~np.signbit(x[j])))
    assert np.array_equal(k[i] == k[j], x.view(np.uint64)[i] == x.view(np.uint64)[j])


def test_digit_pick():
    table = np.array([0, 3, 0, 2, 5, 0], np.int64)
    assert [host_pick(table, r) for r in range(10)] == [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)]
    assert host_pick(table, 10)[0] == -1 and host_pick(np.zeros(4, np.int64), 0)[0] == -1


def test_digits_of_the_host_object_match_the_restatement():
    x = np.concatenate([SPECIALS, np.random.default_rng(3).normal(0, 10, 300)])
    k = D.keys(x)
    prefix = int(k[7])
    for p in range(6):
        shift, width = D.digit_geometry(p)
        out = np.empty(len(k), np.int32)
        lib().fs_dist_host_digits(np.ascontiguousarray(k).ctypes.data, len(k), prefix, p, out.ctypes.data)
        hb = shift + width
        match = np.ones(len(k), bool) if hb >= 64 else (k >> np.uint64(hb)) == (np.uint64(prefix) >> np.uint64(hb))
        want = np.where(match, ((k >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64), -1)
        assert np.array_equal(out, want), p
        assert match[7]


def test_radix_select_through_the_host_pick_equals_the_sort():
    rng = np.random.default_rng(4)
    tie = np.full(700, 128.0)
    x = np.concatenate([rng.normal(0, 50, 1500), tie, -tie[:300], SPECIALS, rng.uniform(-1e-308, 1e-308, 50)])
    rng.shuffle(x)
    s = np.sort(x)
    n = len(x)
    lo, hi = int(np.searchsorted(s, 128.0, "left")), int(np.searchsorted(s, 128.0, "right")) - 1
    assert hi - lo + 1 >= 700
    for k in (0, 1, lo - 1, lo, (lo + hi) // 2, hi, hi + 1, n // 2, n - 2, n - 1):
        got = D.radix_select(x, k, host_pick)
        assert got == s[k], (k, got, s[k])
    z = np.zeros(64)
    z[:5] = -0.0
    for k in (0, 4, 5, 63):
        got = D.radix_select(z, k, host_pick)
        assert got == 0.0 and np.signbit(got) == (k < 5)


def test_binding_and_python_refusals():
    from fs import _lib as L
    from fs.runtime import DeviceBase
    for name in ("create", "launch", "read", "get", "set", "reset", "free", "select"):
        assert "fs_dist_" + name in L.EXPORTS
    assert L.ABI_VERSION >= 24

    class _Dev:
        nranks, capturing, nx, ny = 1, False, 40, 20
    ok = {"quantity": "u", "bins": 8, "range": (0.0, 1.0)}
    c = DeviceBase.dist_channel(_Dev(), ok)
    assert (c.quantity, c.bins, c.lo, c.hi, c.quantity_b, c.box, c.shape) == (0, 8, 0.0, 1.0, -1, (0, 0, 40, 20), (8,))
    j = DeviceBase.dist_channel(_Dev(), dict(ok, against={"quantity": "swirl", "bins": 512, "range": (-1, 1)}, box=(1, 2, 3, 4)))
    assert (j.quantity_b, j.bins_b, j.shape, j.box) == (6, 512, (8, 512), (1, 2, 3, 4))
    bad = [dict(ok, quantity="nope"), dict(ok, bins=0), dict(ok, bins=4097), dict(ok, range=(1.0, 1.0)), dict(ok, range=(2.0, 1.0)),
           dict(ok, range=(0.0, float("inf"))), dict(ok, range=(float("nan"), 1.0)), dict(ok, range=None), dict(ok, range=(-1e308, 1e308)),
           dict(ok, range=(0.0, 5e-324)), dict(ok, against={"quantity": "w", "bins": 513, "range": (0, 1)}), dict(ok, box=(0, 0, 41, 20)),
           dict(ok, box=(5, 0, 5, 20)), dict(ok, nonsense=1), "u"]
    for spec in bad:
        with pytest.raises(ValueError):
            DeviceBase.dist_channel(_Dev(), spec)
    with pytest.raises(ValueError, match="channels"):
        DeviceBase.dist_create(_Dev(), [ok] * 5)
    with pytest.raises(ValueError, match="channels"):
        DeviceBase.dist_create(_Dev(), [])
    with pytest.raises(ValueError, match="ranks"):
        DeviceBase.dist_select(_Dev(), "u", None, 1.0, None, None, list(range(9)))
    with pytest.raises(ValueError, match="ascending"):
        DeviceBase.dist_select(_Dev(), "u", None, 1.0, None, None, [3, 2])

    class _Slab(_Dev):
        nranks = 2
    for call in (lambda: DeviceBase.dist_create(_Slab(), ok), lambda: DeviceBase.dist_select(_Slab(), "u", None, 1.0, None, None, [0])):
        with pytest.raises(L.FsError, match="single-GPU"):
            call()

    class _Capturing(_Dev):
        capturing = True
    for call in (lambda: DeviceBase.dist_create(_Capturing(), ok), lambda: DeviceBase.dist_select(_Capturing(), "u", None, 1.0, None, None, [0])):
        with pytest.raises(L.FsError, match="capture"):
            call()


def test_quantile_arithmetic_and_helpers():
    from fs import dist
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 1000, 269860):
        x = np.sort(rng.normal(size=min(n, 5000)))
        for q in (0.0, 0.1, 0.5, 0.85, 0.9, 1.0, 1 / 3):
            a, b, g = dist.rank_pair(n, q)
            assert 0 <= a <= b <= n - 1 and b - a <= 1 and 0.0 <= g < 1.0
            if n <= 5000:
                assert dist.interpolate(x[a], x[b], g, "lower") == np.quantile(x, q, method="lower")
                assert dist.interpolate(x[a], x[b], g, "higher") == np.quantile(x, q, method="higher")
                assert dist.interpolate(x[a], x[b], g, "linear") == x[a] + (x[b] - x[a]) * g
                assert dist.interpolate(x[a], x[b], g, "nearest") in (x[a], x[b])
    with pytest.raises(ValueError):
        dist.rank_pair(10, 1.5)
    with pytest.raises(ValueError):
        dist.interpolate(0.0, 1.0, 0.5, "cubic")
    # the helpers on a hand-made table: 4 bins over [0, 4)
    d = {"counts": np.array([1, 3, 0, 4], np.int64), "edges": dist.edges(0.0, 4.0, 4), "below": 2, "above": 0, "nan": 1}
    assert np.array_equal(d["edges"], [0, 1, 2, 3, 4])
    assert np.array_equal(dist.density(d), np.array([1, 3, 0, 4]) / 8.0)
    assert np.array_equal(dist.cdf(d), np.array([3, 6, 6, 10]) / 10.0)
    m = dist.moments(d)
    assert m["mean"] == (0.5 + 3 * 1.5 + 4 * 3.5) / 8 and m["variance"] > 0
    assert dist.quantile_from_counts(d, 0.0) == 0.0 and dist.quantile_from_counts(d, 1.0) == 4.0 and dist.quantile_from_counts(d, 0.5) == 2.0
    assert np.array_equal(dist.quantile_from_counts(d, [0.125, 0.25]), [1.0, 1.0 + 1.0 / 3.0])
    e = dist.edges(-1.0, 1.0, 4096)
    assert e[0] == -1.0 and e[-1] == 1.0 and len(e) == 4097 and (np.diff(e) > 0).all()
