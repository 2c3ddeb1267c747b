"""Body surface loads on the GPU past one round of partials (csrc/fs_loads.h k_loads_faces / k_loads_record): the checkerboard body of
tests/surface_cases.py - 66,248 faces, 259 workgroups of 256 faces (the last of 200), so that lanes 0 .. 2 of k_loads_record fold two
partials each and lanes 3 .. 255 one.  The largest list of tests/test_gpu_loads.py has 4096 faces, 16 partials: a record launch that read
partial[threadIdx.x] alone passes there.

The simulator is never stepped - a flow on a checkerboard means nothing; the fields are uploaded and the device calls are driven directly
with dx = 2^-6 and inv_re = 2^-7.  On the integer fields every face term and every partial sum is exact in double
(tests/test_surface_cases_cpu.py proves it), so records and per-face sums compare with == whatever the order of the fold.  The float case
uses loads_ref.record_bound, the bound of tests/test_gpu_loads.py; no other tolerance occurs."""
import numpy as np
import pytest
from lcs_cases import make_sim
from loads_ref import record_bound, samples

import surface_cases as C

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
NP_DTYPE = {"f32": "float32", "f64": "float64"}


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _sim(dtype):
    import fs
    fs.runtime.init(gpu=0, dtype=dtype)
    return make_sim(C.mask(), dx=C.DX)


def _close(sim):
    sim._solver._bc.device.close()


def _upload(sim, v, p):
    s = sim._solver
    s.v.current.from_numpy(np.array(v))
    s.p.current.from_numpy(np.array(p))
    assert s.v.current.pending_limit is None          # (nothing is owed: the kernels read the values as uploaded)
    return s.get_fields()[:2]


_REF = {}


def _reference(dtype):
    """Three samples on the three exact field triples -> records (3, 6), the per-face sums after each sample; computed once per dtype."""
    if dtype not in _REF:
        fc = C.faces()
        sums, recs, after = np.zeros((4, len(fc))), [], []
        for seed in C.SEEDS:
            rec, _ = C.sample_vec(sums, *C.exact_fields(seed, NP_DTYPE[dtype]), fc, C.CENTRE, C.DX, C.INV_RE)
            recs.append(rec), after.append(sums.copy())
        recs = np.array(recs)
        assert np.all(recs != 0.0), "an entry of an expected record is zero: the comparison shows nothing"
        assert all(np.abs(after[-1][k]).max() > 0.0 for k in range(4)) and not np.array_equal(recs[0], recs[1])
        _REF[dtype] = recs, after
    return _REF[dtype]


def _six_launches(sim, lo, dtype, mid_sums=False):
    """every = 2, start = 0: launches 2, 4, 6 (from 1) sample; a new field triple goes up before launches 1, 3, 5.  -> the sums read after
    launch 2 and after launch 3 (without draining the ring) when asked."""
    dev = sim._dev
    peek = []
    for n in range(6):
        assert samples(n, 0, 2) == (n % 2 == 1)
        if n % 2 == 0:
            v, p = _upload(sim, *C.exact_fields(C.SEEDS[n // 2], NP_DTYPE[dtype]))
        dev.loads_record(lo, C.DX, C.INV_RE, v, p)
        if mid_sums and n in (1, 2):
            peek.append(dev.loads_sums(lo))
    return peek


# ---- 1. the second round of k_loads_record, launches that do not sample, the ring overflow -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_records_and_sums_equal_the_exact_restatement(dtype, hip_lib):
    recs, after = _reference(dtype)
    sim = _sim(dtype)
    dev = sim._dev
    try:
        fc = C.faces()
        assert C.partition(len(fc)) == (259, 200, 3)
        lo = dev.loads_create(fc, C.CENTRE, 8, every=2, start=0)
        after_2, after_3 = _six_launches(sim, lo, dtype, mid_sums=True)
        # launch 3 does not sample: k_loads_faces returns before it touches a sum, although the fields under it have changed
        assert np.array_equal(after_2, after[0]), "the per-face sums after the first sample differ from the restatement"
        assert np.array_equal(after_3, after_2), "a launch that does not sample changed the per-face sums"
        got, launches, nsamples, dropped = dev.loads_read(lo)
        assert (launches, nsamples, dropped) == (6, 3, 0) and got.shape == (3, 6)
        for k in range(3):
            assert got[k].tolist() == recs[k].tolist(), f"record {k}: {got[k].tolist()} != {recs[k].tolist()}"
        sums = dev.loads_sums(lo)
        for k, name in enumerate(("S_p", "S_pp", "S_t", "S_tt")):
            assert np.array_equal(sums[k], after[2][k]), f"{name} differs from the restatement after three samples"
        assert dev.loads_read(lo)[0].shape == (0, 6)          # (drained)
        dev.loads_free(lo)
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ring_of_two_drops_the_third_record_and_keeps_the_sums(dtype, hip_lib):
    recs, after = _reference(dtype)
    sim = _sim(dtype)
    dev = sim._dev
    try:
        lo = dev.loads_create(C.faces(), C.CENTRE, 2, every=2, start=0)
        _six_launches(sim, lo, dtype)
        got, launches, nsamples, dropped = dev.loads_read(lo)
        assert (launches, nsamples, dropped) == (6, 3, 1) and got.shape == (2, 6)
        assert got[0].tolist() == recs[0].tolist() and got[1].tolist() == recs[1].tolist()
        assert np.array_equal(dev.loads_sums(lo), after[2]), "the dropped record's sample is missing from the per-face sums"
        dev.loads_free(lo)
    finally:
        _close(sim)


# ---- 2. the launch form -------------------------------------------------------------------------------------------------------------------
def test_a_sampling_launch_is_the_split_pair(hip_lib):
    """66,248 faces > LOADS_SPLIT = 512 (csrc/fs_loads.h): k_loads_faces over 259 workgroups, then k_loads_record; never k_loads_one."""
    recs, _ = _reference("f32")
    sim = _sim("f32")
    dev = sim._dev
    try:
        lo = dev.loads_create(C.faces(), C.CENTRE, 1)
        v, p = _upload(sim, *C.exact_fields(C.SEEDS[0], "float32"))
        dev.profile(True)
        dev.loads_record(lo, C.DX, C.INV_RE, v, p)
        rep = dev.profile_report()
        kernels = dev.profile_kernels("loads_record")
        dev.profile(False)
        assert rep["loads_record"][0] == 1
        assert len(kernels) == 2 and any("k_loads_faces<" in k for k in kernels) and any(k.endswith("k_loads_record") for k in kernels), kernels
        got, launches, nsamples, dropped = dev.loads_read(lo)
        assert (launches, nsamples, dropped) == (1, 1, 0) and got[0].tolist() == recs[0].tolist()
        dev.loads_free(lo)
    finally:
        _close(sim)


# ---- 3. fields on which nothing is exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_fields_within_the_rounding_bound_and_repeatable(dtype, hip_lib):
    fc = C.faces()
    fields = C.float_fields(NP_DTYPE[dtype])
    sums = np.zeros((4, len(fc)))
    rec, scale = C.sample_vec(sums, *fields, fc, C.CENTRE, C.DX, C.INV_RE)
    tol = record_bound(len(fc), scale)
    assert np.all(np.abs(rec) > tol), "an expected entry lies inside its own bound: the comparison shows nothing"
    sim = _sim(dtype)
    dev = sim._dev
    try:
        v, p = _upload(sim, *fields)
        out = []
        for _ in range(2):          # two fresh objects
            lo = dev.loads_create(fc, C.CENTRE, 4)
            dev.loads_record(lo, C.DX, C.INV_RE, v, p)
            got, launches, nsamples, dropped = dev.loads_read(lo)
            assert (launches, nsamples, dropped) == (1, 1, 0) and got.shape == (1, 6)
            assert np.array_equal(dev.loads_sums(lo), sums), "per-face sums differ from the restatement"          # (one face, one lane: no fold)
            dev.loads_free(lo)
            out.append(got[0])
        err = np.abs(out[0] - rec)
        print(f"{dtype}: |record - restatement| = {err.tolist()}, bound = {tol.tolist()}")
        assert np.all(err <= tol), (err.tolist(), tol.tolist())
        assert out[0].tobytes() == out[1].tobytes(), "two trackers on the same fields differ"
    finally:
        _close(sim)


# ---- 4. body_snapshot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_snapshot_of_an_exact_pressure_field(dtype, hip_lib):
    """v = 0, so the solver's re (1e3, not dyadic) multiplies zeros only; the pressure entries are exact at the solver's dx = 2^-6."""
    fc = C.faces()
    _, p = C.exact_fields(C.SEEDS[2], NP_DTYPE[dtype])
    v = np.zeros(p.shape + (2,), p.dtype)
    sums = np.zeros((4, len(fc)))
    rec, _ = C.sample_vec(sums, v, p, fc, C.CENTRE, C.DX, 1.0e-3)
    assert rec[0] != 0.0 and rec[1] != 0.0 and rec[4] != 0.0 and not rec[[2, 3, 5]].any()
    sim = _sim(dtype)
    try:
        assert sim._solver.dx == C.DX
        _upload(sim, v, p)
        snap = sim.body_snapshot(C.BOX, center=C.CENTRE)
        assert np.array_equal(snap["faces"], fc)
        for key, c in (("pressure_x", 0), ("pressure_y", 1), ("moment_pressure", 4)):
            assert snap[key] == rec[c], (key, snap[key], rec[c])
        for key in ("viscous_x", "viscous_y", "moment_viscous"):
            assert snap[key] == 0.0, key
        assert snap["force_x"] == rec[0] and snap["force_y"] == rec[1] and snap["moment"] == rec[4]
        assert np.array_equal(snap["p"], sums[0]) and np.abs(snap["p"]).max() == 8.0 and not snap["tau"].any()
    finally:
        _close(sim)
