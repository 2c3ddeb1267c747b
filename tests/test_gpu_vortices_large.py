"""Vortex identification on the GPU at its large-grid forms (csrc/fs_vortex.h, host code in csrc/fs_diag.hip): the branches that the grids
of tests/test_gpu_vortices.py (at most 300 x 70 = 21,000 cells) never reach.  Everything is exact against the restatement
(tests/vortex_ref.py), through the helpers of tests/test_gpu_vortices.py; tests/test_vortex_cases_cpu.py guards the properties of the cases.

The grid is (1030, 262) with the random scene of tests/vortex_cases.py, 269,860 cells:
  k_vortex_scan      264 blocks of 1024 cells: chunk = ceil(264 / 256) = 2, lanes 0 .. 131 take two blocks, the clamp b0 = min(nb, 2 t) bites
                     from lane 132 on.
  k_vortex_records   random field, 28,458 components: chunk = 28, the cut pos < 1024 falls at offset 16 of lane 36's chunk, passed = 28,458
                     > max_vortices = 1024; with min_area=2 and max_vortices=1000, 970 of the first 1,100 components fail, so the kept
                     ones are spread over the chunks of 70 lanes and more; with max_components=1500: found > maxc, nc = 1500, chunk = 2.
  k_vortex_reduce    1055 workgroups: blockIdx % 256 wraps four times - the dropped counter with max_components=1500 (30,591 cells),
                     the clipped counter with omega_max=256 (19,598 cells).  Rotation field: two components of about 134,000 cells, more
                     than 2,000 waves wholly in one component (the combine), sum |q| = 7.2e13 > 2^46, the low words of |q|(2i+1) sum to
                     2.9e14 > 2^48, mx_hi and my_hi in the millions, 267,020 cells tied at |q| = 2^29: the peak is the smallest index.
  k_vortex_flags     4 rows per workgroup: 66 workgroups down the grid, the last of 2 rows; FS_DIAG_WGS=85: 16 rows, 17 workgroups, the
                     last of 6 rows (a full row group and a partial one of 2).
  k_vortex_local / seam / compress   33 x 33 tiles with a partial last one each way; serpentine and spiral are single components whose
                     chains of tile-local roots run through about a thousand tiles.
  the full ring      on the small (37, 12) grid through the device calls: launches that find the ring full do nothing and are counted."""
import time

import numpy as np
import pytest
from helpers import diag_floor
from test_gpu_vortices import CRITERIA, _assert_sample, _close, _exponent, _make

import vortex_cases as C
import vortex_ref as R

pytestmark = pytest.mark.gpu

X, Y, _ = C.TALL
DX = 1.0 / Y
NP_DTYPE = {"f32": "float32", "f64": "float64"}
# FS_DIAG_WGS at which the flag pass takes 16 rows per workgroup: the rule of csrc/fs_launch.h diag_rows with the inputs of vortex_flags_grid
# (csrc/fs_diag.hip) - nx = ceil(X / 256) workgroups across, ny = Y rows, from 4 rows up to 32.  Device.diag_rows()["flow_stats"] is the
# same rule with the same inputs (stats_rows: nx = ceil(X / 256), ny = Y on a single GPU, from 4 up to 32), which is what the tests assert.
WGS_16_ROWS = diag_floor(-(-X // 256), Y, 4, 16)


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _sim(scene, dx, dtype):
    """A simulator on (const, mask) as tests/test_gpu_vortices.py builds it; no step is taken."""
    import fs
    const, mask = scene
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask)


def _load(sim, v):
    """Upload v -> what the device holds (as test_clipped_counts_the_cells_beyond_omega_max does)."""
    sim._solver.v.current.from_numpy(np.array(v))
    return sim.field_to_numpy()["v"]


def _check(sim, v, mask, dx, which, thr, e, what, **kw):
    """find_vortices against the restatement: every integer, the converted floats and the planes -> the restatement's sample."""
    omega_max = kw.pop("omega_max", None)
    ref = R.sample(v, mask, dx, which, thr, e, **kw)
    out = sim.find_vortices(thr, which, omega_max=omega_max, **kw)
    assert out["exponent"] == e and len(out["step"]) == 1, what
    _assert_sample(out, 0, ref, e, dx, mask.shape[0], what)
    planes = sim.vortex_labels()
    assert np.array_equal(planes["flags"], ref["flags"]) and np.array_equal(planes["labels"], ref["labels"]), what
    return ref, out


def _threshold(v, mask):
    c, _ = R.criterion("vorticity", v, mask, DX)
    return float(np.quantile(c[mask == 0], 0.85))


# ---- the labelling primitive ----------------------------------------------------------------------------------------------------------------
LABEL_PATTERNS = ("ones", "serpentine", "spiral", "u_shape", "random_one_sign", "random_two_signs")


def test_labels_of_large_flag_planes_equal_the_search(hip_lib):
    from fs.runtime import Device
    _, mask = C.tall_scene()
    pats = R.patterns(X, Y)
    dev = Device(X, Y, "f32")
    try:
        dev.upload_scene(np.array(mask), np.zeros((X, Y, 2), np.float32))
        dev.vortex_label(pats["empty"])          # (the first call pays for loading the kernels: not part of a pattern's time)
        for name in LABEL_PATTERNS:
            flags = pats[name]
            want = R.label_plane(flags)
            t0 = time.perf_counter()
            got = dev.vortex_label(flags)
            print(f"vortex_label {name} ({X}, {Y}): {(time.perf_counter() - t0) * 1e3:.2f} ms with the copies")
            assert got.dtype == np.int32 and got.shape == (X, Y)
            assert np.array_equal(got, want), f"{name}: {(got != want).sum()} labels differ"
            if name in ("serpentine", "spiral"):
                assert set(np.unique(want)) == {-1, 0}
            if name == "random_one_sign":
                ids, counts = np.unique(want[want >= 0], return_counts=True)
                big = want == ids[np.argmax(counts)]
                assert big[0].any() and big[-1].any() and big[:, 0].any() and big[:, -1].any(), "no spanning component: the case degraded"
    finally:
        dev.close()


# ---- the pipeline on the random field ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_random_field_more_components_than_records_and_than_the_cap(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.tall_scene(), DX, dtype)
    try:
        assert sim._dev.diag_rows()["flow_stats"] == 4
        v = _load(sim, C.random_field(NP_DTYPE[dtype]))
        thr, e = _threshold(v, mask), _exponent(DX)
        # nc > 1024 components in k_vortex_records, every one passes: the cut falls inside a lane's chunk, passed > max_vortices
        ref, out = _check(sim, v, mask, DX, "vorticity", thr, e, f"{dtype} min_area=1", min_area=1, max_vortices=1024)
        assert ref["passed"] == ref["components"] > 1024 == ref["count"] == len(out["label"])
        # passing and failing components interleave in front of the cut
        ref, _ = _check(sim, v, mask, DX, "vorticity", thr, e, f"{dtype} min_area=2", min_area=2, max_vortices=1000)
        assert ref["components"] > ref["passed"] > 1000 == ref["count"]
        # found > max_components: chunk = 2 over the 1500 reduced ones, the dropped cells counted over the wrapped slots
        ref, _ = _check(sim, v, mask, DX, "vorticity", thr, e, f"{dtype} max_components=1500", min_area=3, max_components=1500)
        assert ref["components"] > 1500 and ref["dropped_cells"] > 256 and 0 < ref["passed"] == ref["count"] < 64
        # thousands of clipped cells, counted over the wrapped slots
        ref, out = _check(sim, v, mask, DX, "vorticity", thr, R.omega_exponent(256.0), f"{dtype} clipped", min_area=1, max_vortices=1024,
                          omega_max=256.0)
        assert ref["clipped"] > 256 and (np.abs(out["peak_omega"]) == 256.0).any()
    finally:
        _close(sim)


# ---- the pipeline on the rotation field -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rotation_field_sums_near_the_bounds_and_tied_peaks(dtype, hip_lib, monkeypatch):
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask = _sim(C.rotation_scene(), C.ROT_DX, dtype)
    try:
        v = _load(sim, C.rotation_field(NP_DTYPE[dtype]))
        e = C.rotation_exponent()
        ref, out = _check(sim, v, mask, C.ROT_DX, "q", 0.0, e, f"rotation {dtype}", omega_max=1.5 * C.ROT_OMEGA)
        raw = out["raw"]
        assert ref["count"] == 2 and ref["clipped"] == 0
        assert (raw["mx_hi"] > 0).all() and (raw["my_hi"] > 0).all() and (raw["sum_aq"] > 1 << 46).all(), "the sums are small: the case degraded"
        # the peak: thousands of cells tie at |q| = 2^29, the smallest j * X + i of them wins
        _, om = R.criterion("q", v, mask, C.ROT_DX)
        q, _ = R.quantise(om, e)
        for k in range(2):
            ties = np.flatnonzero(((ref["labels"] == raw["label"][k]) & (np.abs(q) == 1 << 29)).T.ravel())
            assert len(ties) > 1000 and int(np.abs(q[ref["labels"] == raw["label"][k]]).max()) == 1 << 29
            i, j = out["peak_cell"][k]
            assert j * X + i == ties[0], (k, (i, j), ties[0])
            assert abs(out["peak_omega"][k]) == C.ROT_OMEGA
    finally:
        _close(sim)


# ---- 16 rows per workgroup of the flag pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sixteen_rows_per_workgroup_of_the_flag_pass(dtype, hip_lib, monkeypatch):
    monkeypatch.setenv("FS_DIAG_WGS", str(WGS_16_ROWS))
    assert WGS_16_ROWS == 85
    sim, mask = _sim(C.tall_scene(), DX, dtype)
    try:
        # (the rule and the inputs of vortex_flags_grid: see WGS_16_ROWS) 17 workgroups down the grid, the last of 6 rows
        assert sim._dev.diag_rows()["flow_stats"] == 16, "the flag pass does not take 16 rows per workgroup: the test does not cover it"
        v = _load(sim, C.random_field(NP_DTYPE[dtype]))
        for which in CRITERIA:
            want, _ = R.criterion(which, v, mask, DX)
            got = sim.vortex_criterion(which)
            assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), f"{dtype} {which}: {(got != want).sum()} cells differ"
            assert np.abs(want).max() > 0 and np.all(got[mask != 0] == 0)
        ref, _ = _check(sim, v, mask, DX, "vorticity", _threshold(v, mask), _exponent(DX), f"{dtype} 16 rows", min_area=1, max_vortices=1024)
        assert ref["components"] > 1024
    finally:
        _close(sim)


# ---- the full ring -----------------------------------------------------------------------------------------------------------------------------
def test_launches_into_a_full_ring_do_nothing_and_are_counted(hip_lib, monkeypatch):
    """The device path of "a sampling launch that finds the ring full does nothing": FluidSimulator.step() and run() always drain first."""
    from fs.vortices import assemble
    monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    sim, mask, dx = _make("odd", "f32")
    dev = sim._dev
    try:
        nx = mask.shape[0]
        e = _exponent(dx)
        va, vb = (np.random.default_rng(seed).uniform(-1, 1, mask.shape + (2,)).astype(np.float32) for seed in (5, 6))
        vx = dev.vortex_create("vorticity", 1.0, e, min_area=1, capacity=2)

        def read():
            words, launches, lost = dev.vortex_read(vx)
            return words, assemble(words, vx.max_vortices, e, dx, nx, words[:, 0] + 1, sim._solver.dt), launches, lost
        va = _load(sim, va)
        for _ in range(2):
            dev.vortex_launch(vx, dx, sim._solver.get_fields()[0])
        vb = _load(sim, vb)
        for _ in range(3):
            dev.vortex_launch(vx, dx, sim._solver.get_fields()[0])          # the ring is full: nothing may be written, not even the planes
        ra, rb = (R.sample(v, mask, dx, "vorticity", 1.0, e, min_area=1) for v in (va, vb))
        assert ra["count"] > 0 and rb["count"] > 0 and not np.array_equal(ra["flags"], rb["flags"]) and not np.array_equal(ra["labels"], rb["labels"])
        planes = dev.vortex_labels(vx)
        assert np.array_equal(planes["flags"], ra["flags"]) and np.array_equal(planes["labels"], ra["labels"]), "a launch into the full ring wrote the planes"
        words, out, launches, lost = read()
        assert (len(words), launches, lost) == (2, 5, 3)
        assert words[:, 0].tolist() == [0, 1]
        for k in range(2):
            _assert_sample(out, k, ra, e, dx, nx, f"full ring, sample {k}")
        dev.vortex_launch(vx, dx, sim._solver.get_fields()[0])              # room again: B into slot 0, launch index 5 in its head
        planes = dev.vortex_labels(vx)
        assert np.array_equal(planes["flags"], rb["flags"]) and np.array_equal(planes["labels"], rb["labels"])
        words, out, launches, lost = read()
        assert (len(words), launches, lost) == (1, 6, 0) and words[0, 0] == 5
        _assert_sample(out, 0, rb, e, dx, nx, "after the read")
        dev.vortex_free(vx)
    finally:
        _close(sim)
