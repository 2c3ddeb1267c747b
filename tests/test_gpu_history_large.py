"""The per-step history on the GPU past the first round of its strided loops (csrc/fs_history.h k_history_faces / k_history_record, 256 lanes):
the checkerboard body of tests/surface_cases.py - 66,248 faces: 259 partials, lanes 0 .. 2 of the record launch fold two - and 600 probes:
three rounds of the probe loop, the last with 88 lanes.  tests/test_gpu_history.py stops at 9 probes and 16 partials, where a lane enters
neither loop twice; the ring-full path of the split form (k_history_faces returns on state[1] >= cap, the record launch counts a dropped
record) runs here for the first time.

The simulator is never stepped: the fields are uploaded and the device calls driven directly.  On the integer pressure fields every face
term p dx (dx = 2^-6) and every partial sum is exact in double (tests/test_surface_cases_cpu.py), so the forces compare with == against
NumPy, against flow_stats and between the two forms of the face sum.  No tolerance occurs in this file."""
import numpy as np
import pytest
from lcs_cases import make_sim

import surface_cases as C

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
NP_DTYPE = {"f32": "float32", "f64": "float64"}
NO_FACES = np.zeros((0, 3), np.int32)
NO_PROBES = np.zeros((0, 2), np.int32)


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
    assert s.v.current.pending_limit is None          # (nothing is owed: the probes read the values as uploaded)
    return s.get_fields()[:2]


def _forces(p, fc):
    fx, fy = C.exact_forces(p, fc, C.DX)
    assert fx != 0.0 and fy != 0.0, "an expected force is zero: the comparison shows nothing"
    return fx, fy


# ---- 1. three rounds of the probe loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_600_probes_equal_the_uploaded_fields(dtype, hip_lib):
    pts = C.probes()
    assert C.partition(len(pts)) == (3, 88, 0)
    sim = _sim(dtype)
    dev = sim._dev
    try:
        hist = dev.history_create(pts, NO_FACES, 4, 1)
        exp = []
        for seed in C.SEEDS[:2]:
            v, p = C.exact_fields(seed, NP_DTYPE[dtype])
            dev.history_record(hist, C.DX, *_upload(sim, v, p))
            exp.append(C.probe_values(v, p, pts))
        exp = np.array(exp)
        assert exp.shape == (2, 600, 3) and not np.array_equal(exp[0], exp[1]) and all(len(np.unique(exp[..., c])) == 17 for c in range(3))
        forces, values, launches, dropped = dev.history_read(hist)
        assert (launches, dropped) == (2, 0) and values.shape == (2, 600, 3)
        bad = np.argwhere(values != exp)
        assert len(bad) == 0, f"{len(bad)} of 3600 probe values differ; the first (record, probe, component): {bad[0].tolist()}"
        assert not forces.any()          # (no face: the force entries are the zeros of an empty sum)
        dev.history_free(hist)
    finally:
        _close(sim)


# ---- 2. the second round of the partial loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_forces_on_66248_faces_equal_numpy_and_flow_stats(dtype, hip_lib):
    fc = C.faces()
    assert C.partition(len(fc)) == (259, 200, 3)
    sim = _sim(dtype)
    dev = sim._dev
    try:
        assert sim._solver.dx == C.DX
        hist = dev.history_create(NO_PROBES, fc, 4, 1)
        exp = []
        for seed in C.SEEDS[:2]:
            v, p = C.exact_fields(seed, NP_DTYPE[dtype])
            dev.history_record(hist, C.DX, *_upload(sim, v, p))
            exp.append(_forces(p, fc))
        st = sim.flow_stats(C.BOX)          # (of the second upload: the same faces and terms, k_flow_stats' order of summation)
        forces, values, launches, dropped = dev.history_read(hist)
        assert (launches, dropped) == (2, 0) and forces.shape == (2, 2) and values.shape == (2, 0, 3)
        assert forces.tolist() == [list(e) for e in exp], (forces.tolist(), exp)
        assert (st["force_x"], st["force_y"]) == exp[1], (st["force_x"], st["force_y"], exp[1])
        dev.history_free(hist)
    finally:
        _close(sim)


# ---- 3. probes and faces together; a ring of one record: the ring-full path of the split form -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_full_ring_of_the_split_form_drops_and_resumes(dtype, hip_lib):
    fc, pts = C.faces(), C.probes()
    sim = _sim(dtype)
    dev = sim._dev
    try:
        hist = dev.history_create(pts, fc, 1, 2)          # capacity 1, every 2
        fields = [C.exact_fields(seed, NP_DTYPE[dtype]) for seed in C.SEEDS]
        for k in (0, 0, 1, 1):                            # launches 1 - 4: launch 2 records triple 0, launch 4 finds the ring full
            dev.history_record(hist, C.DX, *_upload(sim, *fields[k]))
        forces, values, launches, dropped = dev.history_read(hist)
        assert (launches, dropped) == (4, 1) and forces.shape == (1, 2) and values.shape == (1, 600, 3)
        # the record of launch 2, untouched by launches 3 and 4 (which ran on other fields)
        assert forces[0].tolist() == list(_forces(fields[0][1], fc))
        assert np.array_equal(values[0], C.probe_values(*fields[0], pts))
        assert _forces(fields[0][1], fc) != _forces(fields[1][1], fc)
        # after the read the ring has room again: two more launches write one more record
        for k in (2, 2):
            dev.history_record(hist, C.DX, *_upload(sim, *fields[k]))
        forces, values, launches, dropped = dev.history_read(hist)
        assert (launches, dropped) == (6, 0) and forces.shape == (1, 2)
        assert forces[0].tolist() == list(_forces(fields[2][1], fc)) and np.array_equal(values[0], C.probe_values(*fields[2], pts))
        dev.history_free(hist)
    finally:
        _close(sim)


# ---- 4. both forms of the face sum on one list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_split_and_one_workgroup_forms_agree_with_the_exact_sum(dtype, hip_lib):
    """700 faces > HIST_SPLIT = 512 (csrc/fs_history.h): three workgroups of k_history_faces, the last of 188 faces; 512 faces: the record
    launch sums them itself, two rounds per lane.  The first 512 faces are common to both."""
    fc = C.faces()
    assert C.partition(700) == (3, 188, 0)
    sim = _sim(dtype)
    dev = sim._dev
    try:
        v, p = C.exact_fields(C.SEEDS[1], NP_DTYPE[dtype])
        fv, fp = _upload(sim, v, p)
        got = {}
        for n in (700, 512, 513):
            hist = dev.history_create(NO_PROBES, fc[:n], 2, 1)
            dev.history_record(hist, C.DX, fv, fp)
            forces, _, launches, dropped = dev.history_read(hist)
            assert (launches, dropped) == (1, 0) and forces.shape == (1, 2)
            dev.history_free(hist)
            got[n] = forces[0].tolist()
            assert got[n] == list(_forces(p, fc[:n])), (n, got[n])
        # 513 = 512 and one face more, across the threshold between the forms: the difference is that face's term
        x, y, d = fc[512].tolist()
        from fs.history import SIGNS
        term = SIGNS[d] * float(p[x, y]) * C.DX
        assert got[513][d // 2] - got[512][d // 2] == term and got[513][1 - d // 2] == got[512][1 - d // 2]
    finally:
        _close(sim)
