"""The energy spectra on the GPU (csrc/fs_spec.h, host code in csrc/fs_diag.hip, fs/spectra.py): every plane with == against the NumPy
restatement (tests/spec_ref.py) fed with downloads of the same fields and the same tables - no tolerance anywhere but against np.fft.fft2.

Part one, the transform: boxes on bc5 res 64 (grid 128 x 64) under a random velocity that is not zero inside the walls - the smallest box,
16 x 8 and 8 x 16 (a transposition error shows), 64 x 32 at an odd offset over the slotted wall (wall cells take 0), the whole grid - and on
grids made for them the rows of 1024, 2048 and 4096 points in both directions: a workgroup holds 4096 / N rows, the kernel has one form for
every N, and 4096 is the row that fills the LDS planes on its own (there is no longer one to put beside it); and the rows of 512 and 256
points (8 and 16 per workgroup) on grids of 512 x 256 and 256 x 512 - the whole grid, 32 workgroups and 16 x 8 transpose tiles, and a quarter
of it at an odd offset.  f32 and f64 fields at every row length, both windows, detrend on and off, a deferred limit_field.  Part two, the rider on bc1 res 32: eager steps against the NumPy loop over per-step
downloads, replayed graphs, a non-sampling launch, the checkpoint round trip, the unchanged trajectory, the refusals."""
import ctypes
import functools

import numpy as np
import pytest
from test_gpu_dist import _load, _sim
from test_gpu_vortices import _close

import spec_ref as S

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
COMBOS = (("hann", True), ("hann", False), ("boxcar", True), ("boxcar", False))
NP_DTYPE = {"f32": "float32", "f64": "float64"}


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


@functools.lru_cache(maxsize=None)
def _tabs(nx, ny, window):
    from fs import spectra
    return spectra.tables(nx, ny, window)


@functools.lru_cache(maxsize=None)
def _scene5():
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(5, 64)
    return const, mask


def _velocity(shape, dtype, seed=3):
    return np.random.default_rng(seed).normal(0.3, 1.0, tuple(shape) + (2,)).astype(dtype)


def _assert_box(sim, v, mask, box, combos=COMBOS):
    """box_fft and spectrum of `box` against the restatement on the downloaded velocity v."""
    nx, ny = box[2] - box[0], box[3] - box[1]
    for window, detrend in combos:
        re, im = S.plane(v, mask, box, _tabs(nx, ny, window), detrend)
        Z = sim.box_fft(box, window=window, detrend=detrend)
        assert Z.shape == (nx, ny) and Z.dtype == np.complex128
        bad = int((Z.real != re).sum() + (Z.imag != im).sum())
        assert bad == 0, (box, window, detrend, bad, float(np.abs(Z.real - re).max()))
        sp = sim.spectrum(box, window=window, detrend=detrend)
        assert np.array_equal(sp["sums"], S.power_of(re, im)), (box, window, detrend)
        assert sp["samples"] == 1 and sp["sample_steps"].tolist() == [0] and sp["box"] == tuple(box)
        assert np.abs(Z).max() > 0, "an empty plane: the test covers nothing"


BOXES_128x64 = {"8x8": (3, 5, 11, 13), "16x8": (1, 2, 17, 10), "8x16": (2, 1, 10, 17), "64x32 over the wall": (61, 17, 125, 49),
                "whole grid": (0, 0, 128, 64)}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(BOXES_128x64))
def test_boxes_on_bc5_res64_equal_the_restatement(name, dtype, hip_lib):
    const, mask = _scene5()
    box = BOXES_128x64[name]
    sim, mask = _sim((const, mask), 1.0 / 64, dtype)
    try:
        assert mask.shape == (128, 64)
        v, _ = _load(sim, _velocity(mask.shape, "float32" if dtype == "f32" else "float64"))
        if "wall" in name or "whole" in name:
            walls = mask[box[0]:box[2], box[1]:box[3]] == 1
            assert walls.any() and (v[box[0]:box[2], box[1]:box[3]][walls] != 0).any(), "no wall cell with a velocity in the box"
        _assert_box(sim, v, mask, box)
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid,boxes", [((4096, 8), ((0, 0, 4096, 8), (1001, 0, 3049, 8), (5, 0, 1029, 8))),
                                        ((8, 4096), ((0, 0, 8, 4096), (0, 1001, 8, 3049), (0, 5, 8, 1029)))], ids=["4096x8", "8x4096"])
def test_long_rows_in_both_directions(grid, boxes, dtype, hip_lib):
    """Rows of 4096 (one per workgroup: the full 64 KB of LDS), 2048 (two) and 1024 (four) points along x and along y."""
    from multigrid_cases import scene
    sim, mask = _sim(scene(grid[0], grid[1], 0.1), 1.0 / max(grid), dtype)
    try:
        v, _ = _load(sim, _velocity(mask.shape, NP_DTYPE[dtype], seed=4))
        assert (mask == 1).any()
        for box in boxes:
            _assert_box(sim, v, mask, box, combos=(("hann", True), ("boxcar", False)))
    finally:
        _close(sim)


# rows of 512 and 256 points: 8 and 16 rows per workgroup, planes of 32 workgroups and 16 x 8 transpose tiles; and a quarter of each at an
# odd offset (8 workgroups, rows of 256 and 128)
MID_GRIDS = {"512x256": (512, 256), "256x512": (256, 512)}
MID_BOXES = {("512x256", "whole grid"): (0, 0, 512, 256), ("512x256", "256x128 at an odd offset"): (129, 67, 385, 195),
             ("256x512", "whole grid"): (0, 0, 256, 512), ("256x512", "128x256 at an odd offset"): (67, 129, 195, 385)}


def _assert_walls_carry_values(mask, box, *fields):
    walls = mask[box[0]:box[2], box[1]:box[3]] == 1
    assert walls.any(), "no wall cell in the box"
    for f in fields:
        assert (f[box[0]:box[2], box[1]:box[3]][walls] != 0).any(), "no wall cell with a stored value in the box"


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid,name", list(MID_BOXES), ids=[f"{g} {n}" for g, n in MID_BOXES])
def test_rows_of_256_and_512(grid, name, dtype, hip_lib):
    from multigrid_cases import scene
    X, Y = MID_GRIDS[grid]
    box = MID_BOXES[grid, name]
    sim, mask = _sim(scene(X, Y, 0.1), 1.0 / max(X, Y), dtype)
    try:
        assert mask.shape == (X, Y) and 0 <= box[0] < box[2] <= X and 0 <= box[1] < box[3] <= Y
        v, _ = _load(sim, _velocity(mask.shape, NP_DTYPE[dtype], seed=4))
        _assert_walls_carry_values(mask, box, v)
        _assert_box(sim, v, mask, box, combos=(("hann", True), ("boxcar", False)))
    finally:
        _close(sim)


def _assert_fft2(sim, v, mask, box):
    nx, ny = box[2] - box[0], box[3] - box[1]
    wx, wy = _tabs(nx, ny, "hann")[:2]
    z = (v[box[0]:box[2], box[1]:box[3], 0] + 1j * v[box[0]:box[2], box[1]:box[3], 1]) * wx[:, None] * wy[None, :]
    z[mask[box[0]:box[2], box[1]:box[3]] == 1] = 0
    want = np.fft.fft2(z)
    got = sim.box_fft(box, window="hann", detrend=False)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(box, "relative L2 error in eps:", err / EPS)
    assert err <= 4 * EPS * np.log2(nx * ny), (box, err / EPS)


def test_box_fft_agrees_with_numpy_fft2(hip_lib):
    """Against np.fft.fft2 of the downloaded, windowed field within 4 eps log2(Nx Ny) in relative L2 norm: the worst-case bound of a
    radix-2 FFT with correctly rounded twiddles.  Boxes on bc5 res 64, and the whole of the 512 x 256 grid."""
    from multigrid_cases import scene
    const, mask = _scene5()
    sim, mask = _sim((const, mask), 1.0 / 64, "f64")
    try:
        v, _ = _load(sim, _velocity(mask.shape, "float64"))
        for box in ((0, 0, 128, 64), (3, 5, 11, 13)):
            _assert_fft2(sim, v, mask, box)
    finally:
        _close(sim)
    sim, mask = _sim(scene(512, 256, 0.1), 1.0 / 512, "f64")
    try:
        v, _ = _load(sim, _velocity(mask.shape, "float64", seed=4))
        _assert_fft2(sim, v, mask, (0, 0, 512, 256))
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_plane(hip_lib):
    """The case tests/test_gpu_dist.py uses: the MAC solver's end-of-step limit_field is deferred, and the flag is up."""
    import os
    import fs
    from fs.solver import VELOCITY_LIMIT
    from helpers import make_product, traj_config
    from test_gpu_vortices import GOLDEN
    g = np.load(os.path.join(GOLDEN, "traj_bc1_upwind_vc0.npz"))
    fs.runtime.init(gpu=0, dtype="f32")
    sim = make_product(g, traj_config(g))
    dev = sim._dev
    try:
        mask = g["bc_mask"]
        i = np.arange(mask.shape[0])[:, None] * np.ones(mask.shape[1])[None, :]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[..., 0] = 3.0 * VELOCITY_LIMIT * np.sin(i / 3.0)
        v[..., 1] = -2.0 * VELOCITY_LIMIT * np.cos(i / 5.0)
        v[mask != 0] = 0
        sim._solver.v.current.from_numpy(v)
        box = (2, 1, 2 + 32, 1 + 16)
        assert box[2] <= mask.shape[0] and box[3] <= mask.shape[1]
        sim.start_spectra(box, window="hann", detrend=True)
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        Z = sim.box_fft(box, window="hann", detrend=True)
        rider = sim.spectra()
        assert cur.pending_limit is not None, "reading the planes flushed the owed pass"
        down = sim.field_to_numpy()                           # (the download launches the owed pass first)
        sub = down["v"][box[0]:box[2], box[1]:box[3]]
        assert np.hypot(sub[..., 0], sub[..., 1]).max() > 0.99 * VELOCITY_LIMIT, "no cell of the box at the limit: the test does not cover it"
        re, im = S.plane(down["v"], mask, box, _tabs(32, 16, "hann"), True)
        assert np.array_equal(Z.real, re) and np.array_equal(Z.imag, im)
        assert rider["samples"] == 1 and np.array_equal(rider["sums"], S.power_of(re, im))
    finally:
        _close(sim)


# ---- the rider on bc1 res 32 ----------------------------------------------------------------------------------------------------------------
RES, BOX, EVERY, START, N = 32, (9, 8, 41, 24), 2, 3, 12


def _make(dtype="f32"):
    import fs
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(1, RES)
    dx = 1.0 / RES
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask)


def _sampled(first, last):
    return [k for k in range(first, last + 1) if k > START and (k - START) % EVERY == 0]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rider_eager_graph_and_resumed_equal_the_numpy_loop(dtype, hip_lib):
    a, mask = _make(dtype)
    b, _ = _make(dtype)
    c, _ = _make(dtype)
    try:
        assert (mask[BOX[0]:BOX[2], BOX[1]:BOX[3]] == 1).any(), "the box misses the cylinder"
        tabs = _tabs(BOX[2] - BOX[0], BOX[3] - BOX[1], "hann")
        ref = S.State(BOX, tabs, True, EVERY, START)
        a.start_spectra(BOX, every=EVERY, start_step=START)
        for n in range(1, N + 1):
            before = a.spectra()["sums"]
            a.step()
            ref.launch(a.field_to_numpy()["v"], mask)
            got = a.spectra()
            assert np.array_equal(got["sums"], ref.power), (dtype, n)
            assert got["samples"] == ref.samples and a._dev.spec_read(a._spectrar.spec, power=False)[1:] == (ref.launches, ref.samples)
            if n not in _sampled(1, N):
                assert np.array_equal(got["sums"], before), f"the non-sampling launch {n} touched the power plane"
        got = a.spectra()
        assert got["sample_steps"].tolist() == _sampled(1, N) and got["samples"] == 4 and got["sums"].max() > 0
        assert np.array_equal(a._dev.spec_plane(a._spectrar.spec).real, ref.re)
        # the same steps under run(graph=True)
        b.start_spectra(BOX, every=EVERY, start_step=START)
        b.run(N, graph=True)
        assert np.array_equal(b.spectra()["sums"], got["sums"]) and b.spectra()["samples"] == 4
        # twelve more: a through a checkpoint into a fresh object, eager; b under run(graph=True)
        z = {k: np.array(x) for k, x in a._spectrar.checkpoint().items()}
        assert (int(z["spec.launches"]), int(z["spec.samples"])) == (N, 4)
        a.stop_spectra()
        a.start_spectra(BOX, every=EVERY, start_step=START)
        assert a.spectra()["samples"] == 0 and a.spectra()["sums"].max() == 0
        assert a._spectrar.restore(z) == 4
        for _ in range(N):
            a.step()
            ref.launch(a.field_to_numpy()["v"], mask)
        b.run(N, graph=True)
        ga, gb = a.spectra(), b.spectra()
        assert np.array_equal(ga["sums"], ref.power) and np.array_equal(gb["sums"], ref.power)
        assert ga["samples"] == gb["samples"] == ref.samples == 10 and ga["sample_steps"].tolist() == gb["sample_steps"].tolist() == _sampled(1, 2 * N)
        # run() captures a period only in a chunk of 16 steps or more: 24 more, so that the launches are replayed from a graph
        for _ in range(2 * N):
            a.step()
            ref.launch(a.field_to_numpy()["v"], mask)
        b.run(2 * N, graph=True)
        assert b._graphs, "the run replayed no graph"
        ga, gb = a.spectra(), b.spectra()
        assert np.array_equal(ga["sums"], ref.power) and np.array_equal(gb["sums"], ref.power)
        assert ga["samples"] == gb["samples"] == ref.samples == 22 and gb["sample_steps"].tolist() == _sampled(1, 4 * N)
        for k in ("power", "energy", "E"):
            assert np.array_equal(ga[k], gb[k]), k
        # the trajectory: with the rider (eager, graphs) and without
        c.run(4 * N, graph=True)
        fa, fb, fc = a.field_to_numpy(), b.field_to_numpy(), c.field_to_numpy()
        for k in fc:
            assert np.array_equal(fa[k], fc[k]) and np.array_equal(fb[k], fc[k]), f"{k}: the rider changed the trajectory"
        b.reset_spectra()
        assert b.spectra()["samples"] == 0 and b.spectra()["sums"].max() == 0
        b.stop_spectra()
        with pytest.raises(RuntimeError):
            b.spectra()
    finally:
        for s in (a, b, c):
            _close(s)


def test_refusals(hip_lib):
    from fs import _lib
    sim, mask = _make()
    dev = sim._dev
    try:
        for bad in ((0, 0, 12, 8), (0, 0, 4, 8), (0, 0, 8, 64), (60, 0, 68, 8), (-8, 0, 0, 8), (0, 0, 8)):
            with pytest.raises(ValueError, match="box|sides"):
                sim.start_spectra(bad)
            with pytest.raises(ValueError, match="box|sides"):
                sim.spectrum(bad)
        with pytest.raises(ValueError, match="window"):
            sim.start_spectra(BOX, window="kaiser")
        assert sim._spectrar is None
        with pytest.raises(RuntimeError):
            sim.spectra()
        sim.start_spectra(BOX)
        with pytest.raises(RuntimeError, match="attached"):
            sim.start_spectra(BOX)
        for call in (sim.spectra, sim.reset_spectra, lambda: sim.spectrum(BOX), lambda: sim.box_fft(BOX), lambda: sim.start_spectra(BOX)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        h = sim._spectrar.spec._h
        out = np.zeros(2 * 32 * 16)
        dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ll = ctypes.c_longlong
        for call in (lambda: _lib.call("fs_spec_read", dev._ctx, h, None, None, None), lambda: _lib.call("fs_spec_reset", dev._ctx, h),
                     lambda: _lib.call("fs_spec_plane", dev._ctx, h, dp), lambda: _lib.call("fs_spec_set", dev._ctx, h, dp, ll(1), ll(0)),
                     lambda: _lib.call("fs_spec_get", dev._ctx, h, dp, ctypes.byref(ll()), ctypes.byref(ll()))):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        # the library's own argument checks
        from fs import spectra
        hh = ctypes.c_void_p()

        def create(ctx, box, every=1, start=0, c1=0.0):
            nx, ny = max(box[2] - box[0], 2), max(box[3] - box[1], 2)
            t = [np.ones(n) for n in (nx, ny, nx, ny)]
            p = [x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for x in t]
            return dev._lib.fs_spec_create(ctx, (ctypes.c_int * 4)(*box), *p, c1, c1, 1, every, start, ctypes.byref(hh))
        assert create(dev._ctx, (0, 0, 8, 8)) == 0 and hh.value
        _lib.call("fs_spec_free", dev._ctx, hh)
        with pytest.raises(_lib.FsError, match="freed"):
            _lib.call("fs_spec_reset", dev._ctx, hh)                      # a stale handle
        hh = ctypes.c_void_p()
        for kw in (dict(box=(0, 0, 12, 8)), dict(box=(0, 0, 4, 8)), dict(box=(0, 0, 8, 64)), dict(box=(-8, 0, 0, 8)), dict(box=(0, 0, 8, 8), every=0),
                   dict(box=(0, 0, 8, 8), start=-1), dict(box=(0, 0, 8, 8), c1=float("nan"))):
            assert create(dev._ctx, **kw) == -1 and not hh.value, kw      # FS_ERR_ARG
            assert dev._lib.fs_last_error()
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert create(slab, (0, 0, 8, 8)) == -5 and not hh.value      # FS_ERR_UNSUPPORTED
            assert "single-GPU" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)
        sim.stop_spectra()
        saved = dev.nranks
        dev.nranks = 2
        try:
            for call in (lambda: sim.start_spectra(BOX), lambda: sim.spectrum(BOX), lambda: sim.box_fft(BOX)):
                with pytest.raises(_lib.FsError, match="single-GPU"):
                    call()
        finally:
            dev.nranks = saved
        assert spectra.WINDOWS == ("hann", "boxcar")
    finally:
        _close(sim)
