"""Flow maps and FTLE on the GPU (csrc/fs_lcs.h k_flowmap_seed / k_flowmap_advance / k_flowmap_cauchy_green, include/fs_hip.h fs_flowmap_*,
FluidSimulator.flow_map / ftle / ftle_fields): positions, statuses and lam bit for bit against the NumPy float64 restatement
(tests/lcs_ref.py) on a scene in which every fate occurs and on a real, wrapped ring; the time interpolation where it must be exact; the
stretching of a steady strain against its analytic value; the refusals and the life cycle.

The grids are the smallest at which the kernels can go wrong: (33, 16) - 528 nodes at refine 1, 2112 at refine 2: more than one workgroup of
256 and a partial last one, odd X; scene 1 at res 20 and a random mask at (37, 12) for the real ring; all-fluid (64, 16) and (64, 32) for the
analytic cases; and, for what only a larger lattice reaches (section 6), boxes with an offset at refine 4 and 8 on a (70, 40) grid - 45,120 and
36,960 nodes.  Rings are installed with pod_set wherever the case needs no time stepping.

Bounds (set by the issue that introduced the feature): equality everywhere but the strain case, whose lam = g^(2N) holds within 1e-10
relative - bilinear interpolation reproduces a linear field, what remains is N <= 64 steps of a few eps each, about 1e-13."""
import ctypes

import numpy as np
import pytest
from lcs_cases import (DT, DX, LATTICE_CASES, LATTICE_DT, LATTICE_DX, LATTICE_RINGS, LATTICE_SUBSTEPS, install_ring, lattice_geometry, lattice_rings,
                       make_sim, strain_expectation, strain_rings, uniform_rings)
from lcs_ref import ALIVE, LEFT, UNSEEDED, WALL_HIT, assert_state_equal, fate_rings, flow_map_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _close(sim):
    sim._solver._bc.device.close()


def _sim(mask, dtype, const=None, dt=DT, dx=DX):
    import fs
    fs.runtime.init(gpu=0, dtype=dtype)
    return make_sim(mask, const, dt, dx)


def _np(dtype):
    return np.float32 if dtype == "f32" else np.float64


# ---- 1. bit for bit against the restatement, every fate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fate_scene_equals_the_restatement(dtype, refine, hip_lib):
    mask, slots = fate_rings(dtype=_np(dtype))
    sim = _sim(mask, dtype, dt=0.5, dx=0.25)          # h = 2 / substeps cells per unit velocity
    try:
        install_ring(sim, slots)
        ring = sim._dev.pod_get(sim._podr.pod)[0]
        assert ring.dtype == _np(dtype) and np.array_equal(ring, slots, equal_nan=True)
        for direction in ("forward", "backward"):
            for substeps in (1, 3):
                exp = flow_map_ref(ring, 4, mask, 1, 0.5, 0.25, direction, refine, None, substeps)
                assert set(np.unique(exp["status"])) == {ALIVE, LEFT, WALL_HIT, UNSEEDED}, "the scene does not produce every fate: the test covers less than it says"
                m = sim.flow_map(direction, refine, None, substeps)
                assert m["x"].size == 528 * refine * refine
                assert_state_equal(m, exp, f"{dtype} r={refine} {direction} S={substeps}: ")
                assert set(np.unique(m["status"])) == {ALIVE, LEFT, WALL_HIT, UNSEEDED}
    finally:
        _close(sim)


# ---- 2. a real, wrapped ring -------------------------------------------------------------------------------------------------------------------
def _real_scene(grid):
    if grid == "scene1":
        from fs.boundary_condition import create_scene_arrays
        const, mask, _ = create_scene_arrays(1, 20)
        return const, mask, 1.0 / 20
    from multigrid_cases import scene
    const, mask = scene(37, 12, 0.3)
    return const, mask, 1.0 / 12


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["scene1", "odd"])
def test_real_wrapped_ring_equals_the_restatement_and_nothing_changes(grid, dtype, hip_lib):
    const, mask, dx = _real_scene(grid)
    mask = np.array(mask)
    dt = 0.05 * dx
    a, b = _sim(mask, dtype, const, dt, dx), None
    try:
        a.start_pod(4, every=2)
        for _ in range(14):          # 7 samples in 4 slots: samples 3 .. 6 sit in slots 3, 0, 1, 2
            a.step()
        ring, launches, samples = a._dev.pod_get(a._podr.pod)
        assert (launches, samples) == (14, 7) and np.isfinite(ring).all() and np.abs(ring[:, :2]).max() > 0
        before = a.field_to_numpy()
        for kw in (dict(direction="forward"), dict(direction="backward"), dict(direction="forward", first=1, last=-1, substeps=2),
                   dict(direction="backward", first=1, last=-1, refine=2)):
            m = a.flow_map(**kw)
            exp = flow_map_ref(ring, 7, mask, 2, dt, dx, **kw)
            assert_state_equal(m, exp, f"{grid} {dtype} {kw}: ")
            assert m["sample_steps"].tolist() == ([10, 12, 14] if "first" in kw else [8, 10, 12, 14])
            assert np.abs(m["x"] - m["x0"]).max() > 0, "nothing moved: the test covers nothing"
        again, launches, samples = a._dev.pod_get(a._podr.pod)
        assert np.array_equal(again, ring) and (launches, samples) == (14, 7), "the flow map changed the ring"
        after = a.field_to_numpy()
        assert all(np.array_equal(before[k], after[k]) for k in before), "the flow map changed a field"
        b = _sim(mask, dtype, const, dt, dx)
        for _ in range(16):
            b.step()
        a.step()
        a.step()
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        assert all(np.array_equal(fa[k], fb[k]) for k in fa), "the flow map changed the trajectory"
    finally:
        _close(a)
        if b is not None:
            _close(b)


# ---- 3. time interpolation is exact where it must be ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_time_linear_uniform_flow_is_integrated_exactly(dtype, hip_lib):
    mask, slots = uniform_rings()
    sim = _sim(mask, dtype)          # dt / dx = 0.5: h = 0.5 / substeps, a dyadic fraction
    try:
        install_ring(sim, slots)
        for substeps in (1, 2, 4):
            for direction, sign in (("forward", 1.0), ("backward", -1.0)):
                m = sim.flow_map(direction, substeps=substeps)
                stay = m["status"] == ALIVE
                # h_total c sum_m (m + (m + 1)) / 2 = 0.5 * 0.25 * 8 = 1 cell, forwards; minus that backwards
                assert stay.sum() == 63 * 16 and np.all(m["status"][~stay] == LEFT), (substeps, direction)
                assert np.all((m["x"] - m["x0"])[stay] == sign * 1.0) and np.all(m["y"] == m["y0"]), (substeps, direction)
            m = sim.flow_map("forward", substeps=substeps, first=2, last=-1)          # snapshots 2 .. 4: 0.5 * 0.25 * 6
            assert np.all((m["x"] - m["x0"])[m["status"] == ALIVE] == 0.75) and m["span"] == 2 * DT
    finally:
        _close(sim)


# ---- 4. stretching has the analytic value ------------------------------------------------------------------------------------------------------------
def test_steady_strain_stretches_by_the_analytic_factor(hip_lib):
    a = 0.1
    mask, slots = strain_rings(a=a)
    sim = _sim(mask, "f64")
    try:
        install_ring(sim, slots)
        for substeps, refine in ((1, 1), (4, 2), (16, 1)):
            for direction in ("forward", "backward"):
                m = sim.flow_map(direction, refine, None, substeps)
                N = substeps * 4
                inner, lam, g = strain_expectation(m, 64, 32, a, 0.5 / substeps, N)
                assert inner.sum() > 100 * refine * refine and np.all(m["status"][inner] == ALIVE)
                err = np.abs(m["lam"][inner] / lam - 1.0).max()
                want = N * np.log(g) / m["span"]
                ferr = np.abs(sim.ftle(direction, refine, None, substeps)[inner] / want - 1.0).max()
                print(f"{direction} S={substeps} r={refine}: {inner.sum()} nodes, max |lam / g^2N - 1| = {err:.3g}, max |ftle / (N log g / span) - 1| = {ferr:.3g}")
                assert err <= 1e-10 and ferr <= 1e-10 and m["span"] == 4 * DT
    finally:
        _close(sim)


# ---- 5. life cycle and refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_life_cycle_and_fields(hip_lib):
    from fs import _lib
    mask, slots = fate_rings()
    sim = _sim(mask, "f32", dt=0.5, dx=0.25)
    dev = sim._dev
    try:
        for call in (sim.flow_map, sim.ftle, sim.ftle_fields):
            with pytest.raises(RuntimeError):
                call()                                                   # no POD attached
        sim.start_pod(4)
        with pytest.raises(RuntimeError):
            sim.flow_map()                                               # no sample
        dev.pod_set(sim._podr.pod, slots, 1, 1)
        with pytest.raises(RuntimeError):
            sim.flow_map()                                               # one sample
        dev.pod_set(sim._podr.pod, slots, 4, 4)
        pod = sim._podr.pod
        ring = dev.pod_get(pod)
        for bad in (dict(refine=3), dict(refine=16), dict(substeps=0), dict(substeps=17), dict(box=(0, 0, 34, 16)), dict(box=(5, 5, 5, 9)),
                    dict(direction="up"), dict(first=2, last=1)):
            with pytest.raises(ValueError):
                sim.flow_map(**bad)
        with pytest.raises(IndexError):
            sim.flow_map(first=4)
        for call in (sim.flow_map, sim.ftle, sim.ftle_fields):
            with pytest.raises((_lib.FsError, RuntimeError)) as e:
                dev.capture(call)
            assert isinstance(e.value, _lib.FsError), call
        # the library checks on its own: FS_ERR_ARG = -1, FS_ERR_STATE = -3, FS_ERR_UNSUPPORTED = -5
        L, ctx = dev._lib, dev._ctx
        box = lambda *b: (ctypes.c_int * 4)(*b)
        hh = ctypes.c_void_p()
        for b, r in ((box(0, 0, 34, 16), 1), (box(0, 0, 33, 17), 1), (box(-1, 0, 4, 4), 1), (box(4, 4, 4, 8), 1), (box(4, 4, 8, 4), 1), (box(0, 0, 33, 16), 3),
                     (box(0, 0, 33, 16), 0), (box(0, 0, 33, 16), 16), (None, 1)):
            assert L.fs_flowmap_create(ctx, b, r, ctypes.byref(hh)) == -1 and not hh.value, (list(b) if b else b, r)
        assert L.fs_flowmap_create(ctx, box(0, 0, 33, 16), 1, None) == -1 and L.fs_flowmap_create(None, box(0, 0, 33, 16), 1, ctypes.byref(hh)) == -1
        fm = dev.flowmap_create((1, 2, 31, 14), 2)
        dev.flowmap_advance(fm, pod, 0, 1, 0.5, 2)
        state = dev.flowmap_get(fm)
        for args in ((0, 0, 0.5, 1), (0, 4, 0.5, 1), (-1, 0, 0.5, 1), (4, 0, 0.5, 1), (0, 1, 0.0, 1), (0, 1, float("inf"), 1), (0, 1, float("nan"), 1),
                     (0, 1, 0.5, 0), (0, 1, 0.5, 17)):
            assert L.fs_flowmap_advance(ctx, fm._h, pod._h, *args) == -1, args
        assert L.fs_flowmap_advance(ctx, None, pod._h, 0, 1, 0.5, 1) == -1 and L.fs_flowmap_advance(ctx, fm._h, None, 0, 1, 0.5, 1) == -1
        assert L.fs_flowmap_cauchy_green(ctx, None) == -1 and L.fs_flowmap_get(ctx, None, None, None, None, None) == -1 and L.fs_flowmap_reset(ctx, None) == -1
        n = fm.shape[0] * fm.shape[1]
        buf = (ctypes.c_double * n)()
        _lib.call("fs_graph_begin", ctx)
        try:
            st = [L.fs_flowmap_create(ctx, box(0, 0, 33, 16), 1, ctypes.byref(hh)), L.fs_flowmap_advance(ctx, fm._h, pod._h, 0, 1, 0.5, 1),
                  L.fs_flowmap_cauchy_green(ctx, fm._h), L.fs_flowmap_get(ctx, fm._h, buf, None, None, None), L.fs_flowmap_reset(ctx, fm._h),
                  L.fs_flowmap_free(ctx, fm._h)]
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", ctx, ctypes.byref(gid))
            _lib.call("fs_graph_free", ctx, gid.value)
        assert st == [-3] * 6 and not hh.value
        # more than 2^30 nodes: 8192 x 4096 cells at refine 8 (refused before anything is allocated or read)
        big = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(big), 0, 8192, 4096, 0, 0, 4096, 0)
        try:
            assert L.fs_flowmap_create(big, box(0, 0, 8192, 4096), 8, ctypes.byref(hh)) == -1 and not hh.value
            assert "2^30" in L.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", big)
        # a slab context (one of two ranks; no communicator is needed to ask)
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert L.fs_flowmap_create(slab, box(0, 0, 64, 32), 1, ctypes.byref(hh)) == -5 and not hh.value
            assert "slab" in L.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)

        class _Slab:
            nranks, capturing, nx, ny = 2, False, 33, 16
        from fs.runtime import DeviceBase
        with pytest.raises(_lib.FsError):
            DeviceBase.flowmap_create(_Slab(), None, 1)
        # nothing of the above moved a node or touched the ring
        for got, was in zip(dev.flowmap_get(fm), state):
            assert np.array_equal(got, was, equal_nan=True)
        again = dev.pod_get(pod)
        assert np.array_equal(again[0], ring[0], equal_nan=True) and again[1:] == ring[1:]
        # get with single outputs; reset seeds again; free releases the handle
        x_only = np.empty(fm.shape[::-1])
        _lib.call("fs_flowmap_get", ctx, fm._h, x_only.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None)
        assert np.array_equal(x_only.T, state[0])
        dev.flowmap_reset(fm)
        x, y, status, lam = dev.flowmap_get(fm)
        assert np.array_equal(x[:, 0], 1 + (np.arange(60) + 0.5) / 2) and np.array_equal(y[0], 2 + (np.arange(24) + 0.5) / 2)
        assert np.isnan(lam).all() and set(np.unique(status)) == {ALIVE, UNSEEDED} and not np.array_equal(x, state[0])
        assert np.array_equal(status == UNSEEDED, np.repeat(np.repeat(mask[1:31, 2:14] == 1, 2, 0), 2, 1))
        h = fm._h
        dev.flowmap_free(fm)
        assert fm._h is None
        with pytest.raises(_lib.FsError):                                # the handle is gone
            _lib.call("fs_flowmap_cauchy_green", ctx, h)
        # flow_map leaves no device object behind: a second call works, stop_pod after it too
        live = len(dev._handle_serial)
        m = sim.flow_map("forward", substeps=2)
        assert len(dev._handle_serial) == live
        assert_state_equal(sim.flow_map("forward", substeps=2), m)
        v, p = sim.ftle_fields("forward", substeps=2)
        assert np.array_equal(p.to_numpy(), np.where(np.isfinite(m["ftle"]), m["ftle"], 0.0).astype(np.float32)) and np.abs(p.to_numpy()).max() > 0
        assert np.array_equal(v.to_numpy(), np.stack([m["x"] - m["x0"], m["y"] - m["y0"]], -1).astype(np.float32))
        dev.profile(True)
        sim.flow_map("backward", substeps=2)
        rep = dev.profile_report()
        dev.profile(False)
        assert rep["flowmap_advance"][0] == 3 and rep["flowmap_cauchy_green"][0] == 1 and rep["flowmap_seed"][0] == 1      # one launch per interval
        sim.stop_pod()
        assert sim._podr is None
        with pytest.raises(RuntimeError):
            sim.flow_map()
    finally:
        _close(sim)


# ---- 6. boxed, refined lattices on a grid wider than one pitch unit -------------------------------------------------------------------------------------
# What the cases above leave out (tests/lcs_cases.py lattice_rings, guarded by tests/test_lcs_cpu.py): refine 4 and 8; a box with x0, y0 != 0
# that is advanced and differentiated - f.x0 + a / f.r and k % f.nx in the kernels, one-sided differences at lattice edges that are not domain
# edges; 16 sub-steps bit for bit; a smooth sheared flow whose bilinear weights and corner indices all matter; 45,120 and 36,960 nodes - 177
# and 145 workgroups, the last of 64 and 96 lanes; a (70, 40) grid whose rows span two 64-column pitch units.  Equality everywhere.
_LATTICE = {}


def _lattice_reference(dtype, box, refine, ring, direction, substeps):
    """flow_map_ref on the ring as the device stores it in `dtype`: computed once per case."""
    key = (dtype, box, refine, ring, direction, substeps)
    if key not in _LATTICE:
        mask, slots = lattice_rings(_np(dtype))
        state = LATTICE_RINGS[ring]
        _LATTICE[key] = flow_map_ref(slots, state["samples"], mask, 1, LATTICE_DT, LATTICE_DX, direction, refine, box, substeps, **state["window"])
    return _LATTICE[key]


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("ring", sorted(LATTICE_RINGS))
@pytest.mark.parametrize("box,refine", LATTICE_CASES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_boxed_refined_lattice_equals_the_restatement(dtype, box, refine, ring, direction, hip_lib):
    from fs.lcs import start_positions
    mask, slots = lattice_rings(_np(dtype))
    state = LATTICE_RINGS[ring]
    nx, ny, groups, last = lattice_geometry(box, refine)
    assert (nx * ny, groups, last) == {8: (45120, 177, 64), 4: (36960, 145, 96)}[refine]
    sim = _sim(mask, dtype, dt=LATTICE_DT, dx=LATTICE_DX)
    try:
        install_ring(sim, slots, samples=state["samples"])
        before = sim._dev.pod_get(sim._podr.pod)
        assert before[0].dtype == _np(dtype) and np.array_equal(before[0], slots) and before[1:] == (state["samples"], state["samples"])
        x0, y0 = start_positions(box, refine)
        for substeps in LATTICE_SUBSTEPS:
            what = f"{dtype} box={box} r={refine} {ring} {direction} S={substeps}: "
            exp = _lattice_reference(dtype, box, refine, ring, direction, substeps)
            fates = set(np.unique(exp["status"]).tolist())
            assert fates == {ALIVE, LEFT, WALL_HIT, UNSEEDED} if ring == "full" else {ALIVE, WALL_HIT, UNSEEDED} <= fates, what
            alive = exp["status"] == ALIVE
            assert alive.sum() > 25000 and np.abs(exp["x"] - x0)[alive].min() > 0 and np.isfinite(exp["lam"]).sum() > 30000, what + "nothing moved"
            m = sim.flow_map(direction, refine, box, substeps, **state["window"])
            assert m["x"].shape == (nx, ny) and m["box"] == box and m["refine"] == refine, what
            assert np.array_equal(m["x0"], x0) and np.array_equal(m["y0"], y0), what
            assert_state_equal(m, exp, what)
            assert m["sample_steps"].tolist() == ([1, 2, 3, 4] if ring == "full" else [4, 5, 6]), what
        after = sim._dev.pod_get(sim._podr.pod)
        assert np.array_equal(after[0], before[0]) and after[1:] == before[1:], "the flow map changed the ring"
    finally:
        _close(sim)


def test_substep_counts_give_different_maps():
    """S = 5 and S = 16 must not be interchangeable, nor the two directions: the cases above would otherwise check less than they say."""
    box, refine = LATTICE_CASES[0]
    a = _lattice_reference("f32", box, refine, "full", "forward", 5)
    b = _lattice_reference("f32", box, refine, "full", "forward", 16)
    c = _lattice_reference("f32", box, refine, "full", "backward", 16)
    both = (a["status"] == ALIVE) & (b["status"] == ALIVE)
    assert (a["x"][both] != b["x"][both]).mean() > 0.99 and not np.array_equal(a["status"], b["status"]) and not np.array_equal(b["status"], c["status"])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_reset_reseeds_a_boxed_refined_lattice(dtype, hip_lib):
    """create, two launches on different slot pairs, reset, the same two launches: the second state is the first, and both are the
    restatement's; the reset state is the seed - start positions, UNSEEDED over the wall block, lam NaN."""
    from fs.lcs import start_positions
    from lcs_ref import advance_ref, cauchy_green_ref, seed_ref
    box, refine = LATTICE_CASES[0]
    mask, slots = lattice_rings(_np(dtype))
    sim = _sim(mask, dtype, dt=LATTICE_DT, dx=LATTICE_DX)
    dev = sim._dev
    try:
        install_ring(sim, slots)
        pod = sim._podr.pod
        launches = ((0, 2, 2.5, 8), (3, 1, -0.625, 7))          # (from, to, h, substeps): forwards over 0 -> 2, then backwards over 3 -> 1
        exp = seed_ref(mask, box, refine)
        seed = {k: np.copy(v) for k, v in exp.items() if k in ("x", "y", "status", "lam")}
        for a, b, h, s in launches:
            advance_ref(exp, slots[a], slots[b], mask, h, s)
        cauchy_green_ref(exp)
        assert set(np.unique(exp["status"]).tolist()) == {ALIVE, LEFT, WALL_HIT, UNSEEDED}
        fm = dev.flowmap_create(box, refine)
        assert fm.shape == (376, 120)
        states = []
        for _ in range(2):
            for a, b, h, s in launches:
                dev.flowmap_advance(fm, pod, a, b, h, s)
            dev.flowmap_cauchy_green(fm)
            states.append(dict(zip(("x", "y", "status", "lam"), dev.flowmap_get(fm))))
            dev.flowmap_reset(fm)
            fresh = dict(zip(("x", "y", "status", "lam"), dev.flowmap_get(fm)))
            assert_state_equal(fresh, seed, "after reset: ")
        x0, y0 = start_positions(box, refine)
        assert np.array_equal(seed["x"], x0) and np.array_equal(seed["y"], y0) and (seed["status"] == UNSEEDED).sum() == 6 * 8 * 64
        assert_state_equal(states[0], exp, "first pass: ")
        assert_state_equal(states[1], states[0], "second pass, after reset: ")
        assert np.abs(states[0]["x"] - x0).max() > 1.0
        dev.flowmap_free(fm)
    finally:
        _close(sim)
