"""Get, reset, set and resume of every accumulator that rides the step, through the device primitives (fs/ride_ops.py over csrc/fs_host.h:
counted_read, counted_set, counted_reset): one table over the time averages, the harmonic modes, the snapshot POD, the distributions, the
spectra, the cross-spectra, the scale fluxes, the per-face sums of the body loads and the tracers' accumulated occupancy; bc3 res 64 of
tests/rider_cases.py with its boxes, f32 and f64, fields developed by 12 solver steps and then left alone.

Per kind, at every = 2: six launches, get -> A (three samples); reset leaves the payload as a fresh object's (all zero; the modes' phasors
(1, 0)), samples 0 and the launch count where it was; set(A) then get returns A bit for bit with A's counters; six more launches from there
equal, bit for bit, a fresh object taken through twelve launches on the same fields; a set with samples > launches is refused by the library
with the counters' message.  == everywhere: the same kernels produce both sides.

What this leaves to the kinds' own tests: the values (each against its NumPy restatement), the riders' checkpoints through the simulator
(the `see` column: a resumed run against an uninterrupted one) and the other refusals (tests/test_gpu_errors.py)."""
import numpy as np
import pytest

import rider_cases as RC

pytestmark = pytest.mark.gpu

EVERY, LAUNCHES = 2, 6
NFREQ, SLOTS, N_TRACERS = len(RC.MODE_CYCLES), RC.POD["snapshots"], 64


class Kind:
    """One row of the table.  create(s) -> object; launch(s, o): one launch behind a step; get(s, o) -> (payload arrays, launches, samples);
    put(s, o, payload, launches, samples): the checked set of the device; raw(s, o, payload, launches, samples): the `_p_*` primitive
    under it, which checks nothing on the host; reset, free; fresh(payload): the payload of a new or reset object (default: zeros)."""

    def __init__(self, see, create, launch, get, put, raw, reset, free, fresh=None):
        self.see, self.create, self.launch, self.get, self.put, self.raw, self.reset, self.free = see, create, launch, get, put, raw, reset, free
        self.fresh = fresh or (lambda payload: tuple(np.zeros_like(a) for a in payload))


def _phasors(payload):
    sums, scalars = payload
    sc = np.zeros_like(scalars)
    sc[0:2 * NFREQ:2] = 1.0
    return np.zeros_like(sums), sc


def _tables():
    from fs import spectra
    box = RC.SPEC_BOX
    return spectra.tables(box[2] - box[0], box[3] - box[1], "hann")


def _loads_get(s, lo):
    sums = s.dev.loads_sums(lo)
    _, launches, samples, _ = s.dev.loads_read(lo)      # (drains the ring, which is no part of the sums)
    return (sums,), launches, samples


def _tracer_create(s):
    from fs.tracers import seed_line
    tr = s.dev.tracer_create(seed_line((4.5, 2.5), (4.5, 61.5), N_TRACERS))
    s.dev.tracer_accum_create(tr, EVERY, 0)
    return tr


def _tracer_launch(s, tr):
    s.dev.tracer_advance(tr, RC.DT / RC.DX, s.v)
    s.dev.tracer_accum_add(tr)


def _tracer_get(s, tr):
    occ, age, launches, samples = s.dev.tracer_accum_read(tr)
    return (occ, age), launches, samples


KINDS = {
    "mean": Kind("test_gpu_mean.py::test_resume_equals_uninterrupted_run",
                 lambda s: s.dev.mean_create(EVERY, 0), lambda s, o: s.dev.mean_accumulate(o, s.v, s.p),
                 lambda s, o: (lambda sums, l, n: ((sums,), l, n))(*s.dev.mean_read(o)),
                 lambda s, o, a, l, n: s.dev.mean_write(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_mean_write(o._h, a[0], l, n),
                 lambda s, o: s.dev.mean_reset(o), lambda s, o: s.dev.mean_free(o)),
    "modes": Kind("test_gpu_modes.py::test_resume_equals_uninterrupted_run",
                  lambda s: s.dev.modes_create(s.cos_sin, EVERY, 0), lambda s, o: s.dev.modes_accumulate(o, s.v, s.p),
                  lambda s, o: (lambda sums, sc, l, n: ((sums, sc), l, n))(*s.dev.modes_read(o)),
                  lambda s, o, a, l, n: s.dev.modes_write(o, a[0], a[1], l, n), lambda s, o, a, l, n: s.dev._p_modes_write(o._h, a[0], a[1], l, n),
                  lambda s, o: s.dev.modes_reset(o), lambda s, o: s.dev.modes_free(o), fresh=_phasors),
    "pod": Kind("test_gpu_pod.py::test_get_set_round_trip_continues_the_ring",
                lambda s: s.dev.pod_create(SLOTS, EVERY, 0), lambda s, o: s.dev.pod_launch(o, s.v, s.p),
                lambda s, o: (lambda slots, l, n: ((slots,), l, n))(*s.dev.pod_get(o)),
                lambda s, o, a, l, n: s.dev.pod_set(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_pod_set(o._h, a[0], l, n),
                lambda s, o: s.dev.pod_reset(o), lambda s, o: s.dev.pod_free(o)),
    "dist": Kind("test_gpu_dist.py::test_rider_eager_graph_and_resumed_give_the_sum_of_one_shots",
                 lambda s: s.dev.dist_create(RC.CHANNELS, EVERY, 0), lambda s, o: s.dev.dist_launch(o, RC.DX, s.v, s.p),
                 lambda s, o: (lambda words, l, n: ((words,), l, n))(*s.dev.dist_get(o)),
                 lambda s, o, a, l, n: s.dev.dist_set(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_dist_set(o._h, a[0], l, n),
                 lambda s, o: s.dev.dist_reset(o), lambda s, o: s.dev.dist_free(o)),
    "spec": Kind("test_gpu_spec.py::test_rider_eager_graph_and_resumed_equal_the_numpy_loop",
                 lambda s: s.dev.spec_create(RC.SPEC_BOX, *_tables(), True, EVERY, 0), lambda s, o: s.dev.spec_launch(o, s.v),
                 lambda s, o: (lambda plane, l, n: ((plane,), l, n))(*s.dev.spec_get(o)),
                 lambda s, o, a, l, n: s.dev.spec_set(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_spec_set(o._h, a[0], l, n),
                 lambda s, o: s.dev.spec_reset(o), lambda s, o: s.dev.spec_free(o)),
    "xspec": Kind("test_gpu_xspec.py::test_rider_eager_graph_and_resumed_equal_the_numpy_loop",
                  lambda s: s.dev.xspec_create(RC.SPEC_BOX, RC.XSPEC_PAIR, RC.DX, *_tables(), True, EVERY, 0),
                  lambda s, o: s.dev.xspec_launch(o, s.v, s.p),
                  lambda s, o: (lambda planes, l, n: ((planes,), l, n))(*s.dev.xspec_get(o)),
                  lambda s, o, a, l, n: s.dev.xspec_set(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_xspec_set(o._h, a[0], l, n),
                  lambda s, o: s.dev.xspec_reset(o), lambda s, o: s.dev.xspec_free(o)),
    "flux": Kind("test_gpu_flux.py::test_rider_eager_graph_and_resumed_equal_the_numpy_loop",
                 lambda s: s.dev.flux_create(RC.FLUX_BOX, RC.FLUX_WIDTHS, RC.DX, EVERY, 0), lambda s, o: s.dev.flux_launch(o, s.v),
                 lambda s, o: (lambda sums, l, n: ((sums,), l, n))(*s.dev.flux_get(o)),
                 lambda s, o, a, l, n: s.dev.flux_set(o, a[0], l, n), lambda s, o, a, l, n: s.dev._p_flux_set(o._h, np.ascontiguousarray(a[0]).ravel(), l, n),
                 lambda s, o: s.dev.flux_reset(o), lambda s, o: s.dev.flux_free(o)),
    "loads": Kind("test_gpu_loads.py::test_reset_stop_and_refusals",
                  lambda s: s.dev.loads_create(s.faces, s.centre, 4 * LAUNCHES, EVERY, 0),
                  lambda s, o: s.dev.loads_record(o, RC.DX, 1.0 / RC.RE, s.v, s.p), _loads_get,
                  lambda s, o, a, l, n: s.dev.loads_sums(o, write=a[0], launches=l, samples=n),
                  lambda s, o, a, l, n: s.dev._p_loads_sums_write(o._h, a[0], l, n),
                  lambda s, o: s.dev.loads_reset(o), lambda s, o: s.dev.loads_free(o)),
    "tracer_accum": Kind("test_gpu_inertial.py::test_checkpoint_round_trip_continues_bit_for_bit",
                         _tracer_create, _tracer_launch, _tracer_get,
                         lambda s, o, a, l, n: s.dev.tracer_accum_write(o, a[0], a[1], l, n),
                         lambda s, o, a, l, n: s.dev._p_tracer_accum_write(o._h, a[0], a[1], l, n),
                         lambda s, o: s.dev.tracer_accum_reset(o), lambda s, o: s.dev.tracer_free(o)),
}


class Scene:
    """bc3 res 64 after 12 steps of the CIP solver, and what the creates need of it."""

    def __init__(self, dtype):
        from fs.boundary_condition import default_body_box
        from fs.history import body_faces
        from fs.loads import body_centroid
        from fs.modes import phasor_steps
        self.sim = RC.make(dtype)
        self.sim.run(12)
        self.dev = self.sim._dev
        self.v, self.p = self.sim._solver.get_fields()[:2]
        mask, box = self.sim._solver._bc.mask, default_body_box(3, RC.RES)
        self.faces, self.centre = body_faces(mask, box), body_centroid(mask, box)
        self.cos_sin = np.stack(phasor_steps(RC.frequencies(), EVERY, RC.DT), axis=1)


@pytest.fixture(scope="module", params=["f32", "f64"])
def scene(request, hip_lib):
    import fs
    s = Scene(request.param)
    yield s
    RC.close(s.sim)
    fs.runtime.init(gpu=0, dtype="f32")


def _same(a, b, what):
    assert len(a) == len(b), what
    for n, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{what}: array {n}"


@pytest.mark.parametrize("kind", list(KINDS))
def test_get_reset_set_and_resume(kind, scene):
    from fs import _lib
    k, s = KINDS[kind], scene
    obj, fresh = k.create(s), k.create(s)
    try:
        for _ in range(LAUNCHES):
            k.launch(s, obj)
        A, launches, samples = k.get(s, obj)
        assert (launches, samples) == (LAUNCHES, LAUNCHES // EVERY)
        assert all(a.any() for a in A), f"{kind}: an empty payload, the test covers nothing"
        k.reset(s, obj)
        Z, l, n = k.get(s, obj)
        assert (l, n) == (LAUNCHES, 0), f"{kind}: reset must zero the samples and leave the launch count"
        _same(Z, k.fresh(A), f"{kind}: the payload after reset")
        k.put(s, obj, A, launches, samples)
        B, l, n = k.get(s, obj)
        assert (l, n) == (launches, samples)
        _same(B, A, f"{kind}: set then get")
        for _ in range(LAUNCHES):
            k.launch(s, obj)
        for _ in range(2 * LAUNCHES):
            k.launch(s, fresh)
        got, want = k.get(s, obj), k.get(s, fresh)
        assert got[1:] == want[1:] == (2 * LAUNCHES, 2 * LAUNCHES // EVERY)
        _same(got[0], want[0], f"{kind}: resumed against uninterrupted")
        assert any((g != a).any() for g, a in zip(got[0], A)), f"{kind}: the second six launches added nothing"
        with pytest.raises(_lib.FsError, match="counters must satisfy 0 <= samples <= launches"):
            k.raw(s, obj, A, 1, 2)
        _same(k.get(s, obj)[0], got[0], f"{kind}: a refused set changed the payload")
    finally:
        k.free(s, obj)
        k.free(s, fresh)
