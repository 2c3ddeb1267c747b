"""The cases of tests/surface_cases.py without a device: every property tests/test_gpu_loads_large.py and tests/test_gpu_history_large.py
rely on to reach the second round of a record launch's strided loops (csrc/fs_loads.h k_loads_record, csrc/fs_history.h k_history_record)
and to compare with ==, so that a change of the mask, of a seed or of the restatement cannot take a case away from them silently."""
import math
from fractions import Fraction

import numpy as np
import pytest
from loads_ref import MID, record_bound, sample_ref

import surface_cases as C

DTYPES = ("float32", "float64")


def test_face_count_and_the_partition_over_workgroups():
    m, fc = C.mask(), C.faces()
    assert m.shape == (192, 192) and m[0].all() and m[-1].all() and m[:, 0].all() and m[:, -1].all()
    x0, y0, x1, y1 = C.BOX
    assert int((m[x0:x1, y0:y1] == 1).sum()) == 182 * 182 // 2 == 16562
    assert not m[1:x0, 1:-1].any() and not m[x1:-1, 1:-1].any() and not m[1:-1, 1:y0].any() and not m[1:-1, y1:-1].any()
    assert len(fc) == C.NFACES == 66248 and [int((fc[:, 2] == d).sum()) for d in range(4)] == [16562] * 4
    assert (m[fc[:, 0], fc[:, 1]] == 0).all(), "a face's cell is not fluid"
    # constants of csrc/fs_loads.h and csrc/fs_history.h restated: 256 faces per workgroup, 256 lanes in the record launch, split above 512
    assert C.partition(len(fc)) == (259, 200, 3) and len(fc) > 512
    assert C.partition(700) == (3, 188, 0) and C.partition(4096) == (16, 256, 0)          # (the largest list of tests/test_gpu_loads.py)
    pts = C.probes()
    assert pts.shape == (600, 2) and len({tuple(q) for q in pts.tolist()}) == 600 and (m[pts[:, 0], pts[:, 1]] == 0).all()
    assert C.partition(600) == (3, 88, 0)          # three rounds of the 256-lane probe loop, the last with 88 lanes
    from fs.history import check_probes
    assert np.array_equal(check_probes(m, pts), pts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inputs_of_the_exact_fields_have_few_bits(dtype):
    fc = C.faces()
    for seed in C.SEEDS:
        v, p = C.exact_fields(seed, dtype)
        assert v.dtype == np.dtype(dtype) and not v.flags.writeable and not p.flags.writeable
        for a in (v, p):
            assert np.array_equal(a, np.rint(a)) and np.abs(a).max() == 8 and len(np.unique(a)) == 17
    assert not np.array_equal(C.exact_fields(C.SEEDS[0], dtype)[1], C.exact_fields(C.SEEDS[1], dtype)[1])
    assert math.frexp(C.DX)[0] == 0.5 and math.frexp(C.INV_RE)[0] == 0.5
    mid = np.asarray(MID)
    arms = np.stack([fc[:, 0] + mid[fc[:, 2], 0] - C.CENTRE[0], fc[:, 1] + mid[fc[:, 2], 1] - C.CENTRE[1]])
    assert np.array_equal(2 * arms, np.rint(2 * arms)) and np.abs(arms).max() < 2 ** 7
    # a sample of faces in rational arithmetic: the double terms are the exact values
    v, p = C.exact_fields(C.SEEDS[0], dtype)
    pick = np.arange(0, len(fc), 37)
    per_face, terms = C.face_terms(v, p, fc[pick], C.CENTRE, C.DX, C.INV_RE)
    dx, ir = Fraction(C.DX), Fraction(C.INV_RE)
    for n, (x, y, d) in enumerate(fc[pick].tolist()):
        pk, ut = Fraction(float(p[x, y])), Fraction(float(v[x, y, 1 if d < 2 else 0]))
        ax, ay = (Fraction(x) + Fraction(MID[d][0]) - Fraction(C.CENTRE[0])) * dx, (Fraction(y) + Fraction(MID[d][1]) - Fraction(C.CENTRE[1])) * dx
        tp, tv = pk * dx, ir * ut
        fpx, fpy = ((-tp, 0), (tp, 0), (0, -tp), (0, tp))[d]
        fvx, fvy = (0, tv) if d < 2 else (tv, 0)
        want = (fpx, fpy, fvx, fvy, ax * fpy - ay * fpx, ax * fvy - ay * fvx)
        assert [Fraction(float(t)) for t in terms[n]] == list(want), (x, y, d)
        assert [Fraction(float(t)) for t in per_face[:, n]] == [pk, pk * pk, tv / dx, (tv / dx) ** 2], (x, y, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_sums_do_not_depend_on_the_order(dtype):
    """The record in face order (sample_ref's loop), in a shuffled order, in reversed order and by math.fsum: identical; so are the per-face
    sums after three samples in both orders of the samples."""
    fc = C.faces()
    v, p = C.exact_fields(C.SEEDS[0], dtype)
    sums = np.zeros((4, len(fc)))
    rec, scale = sample_ref(sums, v, p, fc, C.CENTRE, C.DX, C.INV_RE)
    per_face, terms = C.face_terms(v, p, fc, C.CENTRE, C.DX, C.INV_RE)
    assert np.array_equal(sums, per_face)
    perm = np.random.default_rng(3).permutation(len(fc))
    for c in range(6):
        col = terms[:, c].tolist()
        shuffled, backwards = 0.0, 0.0
        for t in terms[perm, c].tolist():
            shuffled += t
        for t in reversed(col):
            backwards += t
        assert rec[c] == shuffled == backwards == math.fsum(col), c
        assert rec[c] == float(np.sum(terms[:, c])) and rec[c] == sum(float(np.sum(terms[b:b + 256, c])) for b in range(0, len(fc), 256)), c
    assert np.all(rec != 0.0) and np.all(scale > np.abs(rec)), "an entry of the record is zero: a test on it shows nothing"
    # three samples: any order of accumulation gives the same per-face sums
    fwd, bwd = np.zeros((4, len(fc))), np.zeros((4, len(fc)))
    for seed in C.SEEDS:
        C.sample_vec(fwd, *C.exact_fields(seed, dtype), fc, C.CENTRE, C.DX, C.INV_RE)
    for seed in C.SEEDS[::-1]:
        C.sample_vec(bwd, *C.exact_fields(seed, dtype), fc, C.CENTRE, C.DX, C.INV_RE)
    assert np.array_equal(fwd, bwd) and all(np.abs(fwd[k]).max() > 0.0 for k in range(4))
    # the history's forces are the pressure entries of the record
    assert C.exact_forces(p, fc, C.DX) == (rec[0], rec[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_vectorised_restatement_gives_the_bits_of_sample_ref(dtype):
    fc = C.faces()
    for fields in (C.exact_fields(C.SEEDS[1], dtype), C.float_fields(dtype)):
        a, b = np.zeros((4, len(fc))), np.zeros((4, len(fc)))
        rec_a, scale_a = sample_ref(a, *fields, fc, C.CENTRE, C.DX, C.INV_RE)
        rec_b, scale_b = C.sample_vec(b, *fields, fc, C.CENTRE, C.DX, C.INV_RE)
        assert np.array_equal(a, b) and rec_a.tobytes() == rec_b.tobytes() and scale_a.tobytes() == scale_b.tobytes()
    # the float case is not exact: the order matters, within the bound the GPU test uses
    per_face, terms = C.face_terms(*C.float_fields(dtype), fc, C.CENTRE, C.DX, C.INV_RE)
    other = np.sum(np.ascontiguousarray(terms.T), axis=1)          # (pairwise along the contiguous axis: another order than the loop's)
    assert np.all(np.abs(other - rec_b) <= record_bound(len(fc), scale_b))
    if dtype == "float64":          # (f32 values times powers of two: their sums happen to be exact far more often)
        assert np.any(other != rec_b)


def test_vectorised_restatement_on_a_scene_of_the_suite():
    """Scene 5 at res 64 (432 faces, tests/test_gpu_loads.py), non-dyadic dx and inv_re, two samples on top of each other."""
    from fs.boundary_condition import create_scene_arrays, default_body_box
    from fs.history import body_faces
    from fs.loads import body_centroid
    _, m, _ = create_scene_arrays(5, 64)
    box = default_body_box(5, 64)
    fc, centre = body_faces(m, box), body_centroid(m, box)
    assert len(fc) == 432
    rng = np.random.default_rng(9)
    a, b = np.zeros((4, len(fc))), np.zeros((4, len(fc)))
    for _ in range(2):
        v, p = rng.standard_normal(m.shape + (2,)).astype(np.float32), rng.standard_normal(m.shape).astype(np.float32)
        rec_a, scale_a = sample_ref(a, v, p, fc, centre, 1.0 / 64, 1.0 / 100)
        rec_b, scale_b = C.sample_vec(b, v, p, fc, centre, 1.0 / 64, 1.0 / 100)
        assert rec_a.tobytes() == rec_b.tobytes() and scale_a.tobytes() == scale_b.tobytes()
    assert a.tobytes() == b.tobytes()
