"""The cases of tests/vortex_cases.py under the NumPy restatement alone (tests/vortex_ref.py; no device): every property the GPU tests of
tests/test_gpu_vortices_large.py rely on to reach a branch of csrc/fs_vortex.h, so that a change of a seed, of the scene recipe or of the
restatement cannot take a case away from them silently.

Measured with the restatement (f32 and f64 agree in every figure below):
  random field, "vorticity", threshold at the 0.85 quantile of the criterion over the fluid cells: 28,458 components; min_area=1: all pass;
  min_area=2: 3,398 pass, 970 of the first 1,100 components are single cells (passing and failing ones interleave); max_components=1500
  with min_area=3: 27 pass, 30,591 cells dropped; omega_max=256: 19,598 of the 32,309 flagged cells clip; at the 0.5 quantile 65,327
  components - below the default max_components of 65,536.
  rotation field, "q", threshold 0: two components, labels 0 and 516, flags 1 and 2, areas 134,551 and 134,668; nothing clips; sum_q
  +72,063,377,211,392 and -72,126,191,108,096 (above 2^46); mx_hi 8,554,088 and 25,890,952, my_hi 4,329,487 and 4,332,930; 267,020 cells
  tie at |q| = 2^29; peak cells (1, 1) and (516, 1)."""
import functools

import numpy as np
import pytest

import vortex_cases as C
import vortex_ref as R

X, Y, _ = C.TALL
DX = 1.0 / Y
DTYPES = ("float32", "float64")


def test_geometry_of_the_grid():
    """The arithmetic the docstrings of the GPU tests quote (constants of csrc/fs_vortex.h and csrc/fs_pod.h restated here)."""
    from helpers import diag_floor
    n = X * Y
    assert n == 269860
    nb = -(-n // 1024)
    assert nb == 264 and -(-nb // 256) == 2 and -(-nb // 2) == 132          # k_vortex_scan: chunk 2, lanes 132 .. 255 empty
    assert -(-n // 256) == 1055 and 1055 // 256 == 4                        # k_vortex_reduce: the slot index wraps four times
    assert (-(-X // 32), -(-Y // 8)) == (33, 33) and X % 32 and Y % 8      # tiles, a partial last one each way
    nx = -(-X // 256)
    assert nx == 5
    # csrc/fs_launch.h diag_rows at the default floor of 2048 and at FS_DIAG_WGS = 85, from 4 rows up
    def rows(floor, rmax):
        r = 4
        while r < rmax and nx * -(-Y // (2 * r)) >= floor:
            r *= 2
        return r
    assert rows(2048, 32) == rows(2048, 64) == 4 and -(-Y // 4) == 66 and Y - 65 * 4 == 2 and nx * 66 == 330 > 256
    floor = diag_floor(nx, Y, 4, 16)
    assert floor == 85 and rows(floor, 32) == rows(floor, 64) == 16 and -(-Y // 16) == 17 and Y - 16 * 16 == 6


@functools.lru_cache(maxsize=None)
def _random(dtype):
    _, mask = C.tall_scene()
    v = C.random_field(dtype)
    c, _ = R.criterion("vorticity", v, mask, DX)
    return v, mask, c


def _quantile(dtype, q):
    _, mask, c = _random(dtype)
    return float(np.quantile(c[np.asarray(mask) == 0], q))


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_field_has_more_components_than_records_and_than_the_cap(dtype):
    v, mask, _ = _random(dtype)
    assert v.shape == (X, Y, 2) and v.dtype == np.dtype(dtype) and not v.flags.writeable
    thr = _quantile(dtype, 0.85)
    e = R.omega_exponent(2.0 * 10.0 / DX)
    ref = R.sample(v, mask, DX, "vorticity", thr, e, min_area=1, max_vortices=1024)
    assert ref["components"] > 1024 and ref["passed"] > 1024 and ref["count"] == 1024
    assert ref["components"] < 65536 and ref["dropped_cells"] == 0 and ref["clipped"] == 0
    # k_vortex_records: chunk = ceil(nc / 1024) > 1, and component 1024 is not the first of its lane: the cut falls inside a chunk
    chunk = -(-ref["components"] // 1024)
    assert chunk >= 2 and 1024 % chunk != 0
    # min_area=2: passing and failing components interleave in front of the cut
    two = R.sample(v, mask, DX, "vorticity", thr, e, min_area=2, max_vortices=1000)
    assert two["passed"] > 1000 and two["count"] == 1000
    full = R.sample(v, mask, DX, "vorticity", thr, e, min_area=1, max_vortices=1 << 20)["raw"]
    last = int(np.searchsorted(full["label"], two["raw"]["label"][-1]))
    head = full["area"][:last + 1]
    assert last + 1 > 2000 and (head == 1).sum() > 1000 and (head >= 2).sum() == 1000
    # max_components=1500 with min_area=3: found > maxc, chunk = 2, cells dropped by the hundred blocks
    cap = R.sample(v, mask, DX, "vorticity", thr, e, min_area=3, max_components=1500)
    assert cap["components"] > 1500 and cap["dropped_cells"] > 256 and 0 < cap["passed"] < 1024 and cap["count"] == min(cap["passed"], 64)
    # omega_max = 256: thousands of flagged cells clip, others do not
    clip = R.sample(v, mask, DX, "vorticity", thr, R.omega_exponent(256.0), min_area=1, max_vortices=1024)
    assert 256 < clip["clipped"] < int((clip["flags"] != 0).sum())
    if dtype == "float32":
        assert (ref["components"], cap["passed"], cap["dropped_cells"], two["passed"], clip["clipped"]) == (28458, 27, 30591, 3398, 19598)


def test_half_the_fluid_cells_stay_below_the_default_max_components():
    v, mask, _ = _random("float32")
    ref = R.sample(v, mask, DX, "vorticity", _quantile("float32", 0.5), R.omega_exponent(2.0 * 10.0 / DX), min_area=1)
    assert 1024 < ref["components"] < 65536 and ref["dropped_cells"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_rotation_field_is_two_large_components_with_tied_peaks(dtype):
    _, mask = C.rotation_scene()
    v = C.rotation_field(dtype)
    assert v.dtype == np.dtype(dtype) and (np.asarray(mask) == 1).sum() == 120 and not np.asarray(mask)[np.asarray(mask) != 1].any()
    e = C.rotation_exponent()
    assert e == 8
    ref = R.sample(v, mask, C.ROT_DX, "q", 0.0, e)
    raw = ref["raw"]
    assert (ref["components"], ref["passed"], ref["count"], ref["clipped"], ref["dropped_cells"]) == (2, 2, 2, 0, 0)
    assert raw["label"].tolist() == [0, 516] and raw["flag"].tolist() == [1, 2] and raw["area"].tolist() == [134551, 134668]
    assert (np.abs(raw["sum_q"]) > 1 << 46).all() and np.array_equal(np.abs(raw["sum_q"]), raw["sum_aq"])
    assert (raw["mx_hi"] > 0).all() and (raw["my_hi"] > 0).all() and (raw["mx_lo"] > 1 << 47).all()
    # the interior: |om| = 128 exactly, |q| = 2^29, by the hundred thousand - and nothing larger, so the peak is decided by the index alone
    _, om = R.criterion("q", v, mask, C.ROT_DX)
    q, clipped = R.quantise(om, e)
    on = ref["flags"] != 0
    assert not clipped[on].any() and int(np.abs(q[on]).max()) == 1 << 29
    assert (np.abs(om[on]) == C.ROT_OMEGA).sum() == (np.abs(q[on]) == 1 << 29).sum() > 100000
    conv = R.convert(raw, e, C.ROT_DX, X)
    assert conv["peak_cell"].tolist() == [[1, 1], [516, 1]] and np.array_equal(np.abs(conv["peak_omega"]), [C.ROT_OMEGA] * 2)
    for k, lab in enumerate(raw["label"].tolist()):
        ties = np.flatnonzero(((ref["labels"] == lab) & (np.abs(q) == 1 << 29)).T.ravel())          # ascending j * X + i
        assert len(ties) > 1000 and ties[0] == conv["peak_cell"][k][1] * X + conv["peak_cell"][k][0]
    # whole waves in one component: runs of 64 consecutive cells of one label, by the thousand
    lab = ref["labels"].T.ravel()
    lab = lab[:len(lab) // 64 * 64].reshape(-1, 64)
    assert ((lab == lab[:, :1]).all(axis=1) & (lab[:, 0] >= 0)).sum() > 2000


def test_label_patterns_of_the_grid():
    """serpentine and spiral are single components through every tile; the largest random_one_sign component spans the grid."""
    pats = R.patterns(X, Y)
    want = R.label_plane(pats["serpentine"])
    assert set(np.unique(want)) == {-1, 0}
    want = R.label_plane(pats["spiral"])
    assert set(np.unique(want)) == {-1, 0}
    want = R.label_plane(pats["random_one_sign"])
    ids, counts = np.unique(want[want >= 0], return_counts=True)
    big = want == ids[np.argmax(counts)]
    assert big[0].any() and big[-1].any() and big[:, 0].any() and big[:, -1].any()
