"""The scale-to-scale fluxes on the GPU (csrc/fs_flux.h, host code in csrc/fs_diag.hip, fs/fluxes.py): every plane with == against the NumPy
restatement (tests/flux_ref.py) fed with downloads of the same fields - no tolerance anywhere.

Part one, the planes: bc5 res 64 (grid 128 x 64) under a random velocity that is not zero inside the walls, half-widths (1, 2, 5, 13), a box
with invalid cells on every side and the whole grid, f32 and f64 - the filtered planes of every half-width, then the fluxes; the grids
512 x 256 and 256 x 512 of tests/test_gpu_spec.py with half-widths (1, 31, 64) and a box at odd offsets that crosses the row kernel's strip
edge and the column kernel's block edges, and a grid of 640 x 136 on which a strip edge lies inside the valid cells of r = 64; a deferred
limit_field.  Part two, the rider on bc1 res 32: eager steps against the NumPy loop, replayed graphs, a non-sampling launch, the checkpoint
round trip, beside both spectra riders, the unchanged trajectory, stop inside a capture, the refusals."""
import ctypes
import os

import numpy as np
import pytest
from conftest import REPO
from test_flux_cpu import limits
from test_gpu_dist import _load, _sim
from test_gpu_spec import BOX as SBOX, MID_GRIDS, NP_DTYPE, _make, _scene5, _velocity
from test_gpu_vortices import _close

import flux_ref as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _tiles():
    """The tile sizes of the kernels, from the header's constants."""
    return limits(ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_flux_host.so")))


def _assert_planes(sim, v, mask, dx, box, hw):
    """filtered_fields of every half-width, then scale_flux, of `box` against the restatement on the downloaded velocity v."""
    x0, y0, x1, y1 = box
    Fs, fl = FR.sample(v, mask, dx, hw)
    for F, r in zip(Fs, hw):
        got = sim.filtered_fields(box, r)
        for k, name in enumerate(FR.NAMES):
            want = F[k, x0:x1, y0:y1]
            assert got[name].shape == want.shape and got[name].dtype == np.float64
            bad = int((got[name] != want).sum())
            assert bad == 0, (box, r, name, bad, float(np.abs(got[name] - want).max()))
        assert np.abs(got["om"]).max() > 0 and np.abs(got["wom"]).max() > 0, "an empty plane: the test covers nothing"
    out = sim.scale_flux(box, hw)
    want = fl[:, :, x0:x1, y0:y1]
    assert out["sums"].shape == want.shape == (len(hw), 3, x1 - x0, y1 - y0)
    for k, r in enumerate(hw):
        for n, name in enumerate(("PI", "ZF", "K")):
            bad = int((out["sums"][k, n] != want[k, n]).sum())
            assert bad == 0, (box, r, name, bad, float(np.abs(out["sums"][k, n] - want[k, n]).max()))
        pi = out["sums"][k, 0]
        assert (pi > 0).any() and (pi < 0).any(), (r, "PI of one sign: the test covers nothing")
        vx0, vy0, vx1, vy1 = FR.valid_rect(mask.shape, r, box)
        assert out["valid"][k] == (vx0, vy0, vx1, vy1) and vx0 < vx1 and vy0 < vy1
        outside = np.ones(pi.shape, bool)
        outside[vx0 - x0:vx1 - x0, vy0 - y0:vy1 - y0] = False
        for n in range(3):
            cells = out["sums"][k, n][outside]
            assert not cells.any() and not np.signbit(cells).any(), (r, n, "an invalid cell is not +0")
    assert out["samples"] == 1 and out["sample_steps"].tolist() == [0] and out["box"] == tuple(box) and out["half_widths"] == tuple(hw)
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_planes_on_bc5_res64_equal_the_restatement(dtype, hip_lib):
    const, mask = _scene5()
    dx, hw = 1.0 / 64, (1, 2, 5, 13)
    sim, mask = _sim((const, mask), dx, dtype)
    try:
        assert mask.shape == (128, 64)
        v, _ = _load(sim, _velocity(mask.shape, NP_DTYPE[dtype]))
        walls = mask == 1
        assert walls.any() and (v[walls] != 0).any() and (mask > 1).any(), "no wall cell with a velocity / no cell that is neither fluid nor wall"
        box = (3, 2, 120, 61)
        out = _assert_planes(sim, v, mask, dx, box, hw)
        assert out["valid"][3] == (14, 14, 114, 50)              # r = 13: only j in [14, 49] is valid
        assert all(lo > b for lo, b in zip(out["valid"][3][:2], box[:2])) and all(hi < b for hi, b in zip(out["valid"][3][2:], box[2:])), \
            "no invalid cells on some side of the box"
        _assert_planes(sim, v, mask, dx, (0, 0, 128, 64), hw)
    finally:
        _close(sim)


BIG = dict(MID_GRIDS, **{"640x136": (640, 136)})
BIG_BOXES = {"512x256": (37, 19, 501, 241), "256x512": (19, 37, 241, 501), "640x136": (31, 3, 633, 131)}
BIG_WIDTHS = {"512x256": (1, 31, 64), "256x512": (1, 31, 64), "640x136": (64,)}


@pytest.mark.parametrize("grid", list(BIG))
def test_past_one_workgroup_in_both_directions(grid, hip_lib):
    """r = 64: the halo is longer than a wave; 126 valid rows on the 256-high grid, 126 valid columns on the 256-wide one.  The boxes cross
    the strip edge of k_flux_rows (every FLUX_STRIP columns of the work region), its row blocks (FLUX_ROW_WAVES rows) and the blocks of
    k_flux_cols (FLUX_COL_LANES columns, FLUX_COL_V rows); on 640 x 136 the strip edge lies inside the valid cells of r = 64."""
    from multigrid_cases import scene
    T = _tiles()
    strip, waves, lanes, colv = T["strip"], T["row_waves"], T["col_lanes"], T["col_v"]
    X, Y = BIG[grid]
    box, hw = BIG_BOXES[grid], BIG_WIDTHS[grid]
    dx = 1.0 / max(X, Y)
    sim, mask = _sim(scene(X, Y, 0.1), dx, "f32")
    try:
        assert mask.shape == (X, Y) and 0 <= box[0] < box[2] <= X and 0 <= box[1] < box[3] <= Y and box[0] % 2 == 1 and box[1] % 2 == 1
        dx0, dy0 = max(0, box[0] - hw[-1] - 1), max(0, box[1] - hw[-1] - 1)      # the origin of the work region
        vx0, vy0, vx1, vy1 = FR.valid_rect(mask.shape, 64, box)
        if X > strip:
            assert box[0] < dx0 + strip < box[2], "the box does not cross a strip edge of the row kernel"
        if grid == "640x136":
            assert vx0 < dx0 + strip < vx1 - 1, "the strip edge is not inside the valid cells of r = 64"
        if X > lanes:
            assert box[0] < dx0 + lanes < box[2], "the box does not cross a block edge of the column kernel along x"
        assert (box[3] - box[1]) > 2 * max(waves, colv) and (box[1] - dy0) % colv and (box[1] - dy0) % waves
        if grid == "512x256":
            assert vy1 - vy0 == 126
        if grid == "256x512":
            assert vx1 - vx0 == 126
        v, _ = _load(sim, _velocity(mask.shape, "float32", seed=4))
        assert (mask[box[0]:box[2], box[1]:box[3]] == 1).any()
        _assert_planes(sim, v, mask, dx, box, hw)
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_planes(hip_lib):
    """The arrangement of tests/test_gpu_xspec.py: the centre values and the four neighbours of the gradient are limited."""
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
        box, hw = (2, 1, 2 + 32, 1 + 16), (1, 3)
        assert box[2] <= mask.shape[0] and box[3] <= mask.shape[1]
        sim.start_scale_fluxes(box, hw)
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        F = [sim.filtered_fields(box, r) for r in hw]
        once = sim.scale_flux(box, hw)
        rider = sim.scale_fluxes()
        kept = [dev.flux_filtered(sim._fluxr.flux, r) for r in hw]
        assert cur.pending_limit is not None, "reading the planes flushed the owed pass"
        down = sim.field_to_numpy()                           # (the download launches the owed pass first)
        sub = down["v"][box[0]:box[2], box[1]:box[3]]
        assert np.hypot(sub[..., 0], sub[..., 1]).max() > 0.99 * VELOCITY_LIMIT, "no cell of the box at the limit: the test does not cover it"
        Fs, fl = FR.sample(down["v"], mask, sim._solver.dx, hw)
        want = fl[:, :, box[0]:box[2], box[1]:box[3]]
        for k in range(len(hw)):
            for n, name in enumerate(FR.NAMES):
                wantF = Fs[k][n, box[0]:box[2], box[1]:box[3]]
                assert np.array_equal(F[k][name], wantF) and np.array_equal(kept[k][n], wantF), (hw[k], name)
        assert np.array_equal(once["sums"], want) and np.abs(want).max() > 0
        assert rider["samples"] == 1 and np.array_equal(rider["sums"], want)
    finally:
        _close(sim)


# ---- the rider on bc1 res 32 ----------------------------------------------------------------------------------------------------------------
BOX, HW, EVERY, START, N = (5, 3, 58, 30), (1, 3), 2, 3, 12
PAIR = ("vorticity", "p")


def _sampled(first, last):
    return [k for k in range(first, last + 1) if k > START and (k - START) % EVERY == 0]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rider_eager_graph_and_resumed_equal_the_numpy_loop(dtype, hip_lib):
    """a: eager, through a checkpoint; b: run(graph=True); c: no rider; d: the fluxes beside both spectra riders; e: those two alone."""
    made = [_make(dtype) for _ in range(5)]
    sims, mask = [m[0] for m in made], made[0][1]
    a, b, c, d, e = sims
    try:
        assert mask.shape == (64, 32) and (mask[BOX[0]:BOX[2], BOX[1]:BOX[3]] == 1).any(), "the box misses the cylinder"
        dx = a._solver.dx
        ref = FR.State(BOX, HW, dx, EVERY, START)

        def follow(steps):
            for _ in range(steps):
                a.step()
                ref.launch(a.field_to_numpy()["v"], mask)

        a.start_scale_fluxes(BOX, HW, every=EVERY, start_step=START)
        for n in range(1, N + 1):
            before = a.scale_fluxes()["sums"]
            follow(1)
            got = a.scale_fluxes()
            assert np.array_equal(got["sums"], ref.sums), (dtype, n)
            assert got["samples"] == ref.samples and a._dev.flux_read(a._fluxr.flux, sums=False)[1:] == (ref.launches, ref.samples)
            if n not in _sampled(1, N):
                assert np.array_equal(got["sums"], before), f"the non-sampling launch {n} touched the planes"
        got = a.scale_fluxes()
        assert got["sample_steps"].tolist() == _sampled(1, N) and got["samples"] == 4
        assert all(np.abs(got["sums"][k, n]).max() > 0 for k in range(len(HW)) for n in range(3))
        for k, r in enumerate(HW):                               # the filtered planes the object keeps: those of the last sample
            assert np.array_equal(a._dev.flux_filtered(a._fluxr.flux, r), ref.filtered[k]), r
        assert np.array_equal(a.scale_fluxes()["sums"], ref.sums), "reading the filtered planes touched the sums"
        # the same steps under run(graph=True)
        b.start_scale_fluxes(BOX, HW, every=EVERY, start_step=START)
        b.run(N, graph=True)
        assert np.array_equal(b.scale_fluxes()["sums"], got["sums"]) and b.scale_fluxes()["samples"] == 4
        # twelve more: a through a checkpoint into a fresh object, eager; b under run(graph=True)
        z = {k: np.array(x) for k, x in a._fluxr.checkpoint().items()}
        assert (int(z["flux.launches"]), int(z["flux.samples"])) == (N, 4)
        a.stop_scale_fluxes()
        a.start_scale_fluxes(BOX, HW, every=EVERY, start_step=START)
        assert a.scale_fluxes()["samples"] == 0 and not a.scale_fluxes()["sums"].any()
        assert a._fluxr.restore(z) == 4
        follow(N)
        b.run(N, graph=True)
        ga, gb = a.scale_fluxes(), b.scale_fluxes()
        assert np.array_equal(ga["sums"], ref.sums) and np.array_equal(gb["sums"], ref.sums)
        assert ga["samples"] == gb["samples"] == ref.samples == 10 and ga["sample_steps"].tolist() == gb["sample_steps"].tolist() == _sampled(1, 2 * N)
        # run() captures a period only in a chunk of 16 steps or more: 24 more, so that the launches are replayed from a graph
        follow(2 * N)
        b.run(2 * N, graph=True)
        assert b._graphs, "the run replayed no graph"
        ga, gb = a.scale_fluxes(), b.scale_fluxes()
        assert np.array_equal(ga["sums"], ref.sums) and np.array_equal(gb["sums"], ref.sums)
        assert ga["samples"] == gb["samples"] == ref.samples == 22 and gb["sample_steps"].tolist() == _sampled(1, 4 * N)
        for k in ("pi", "zf", "k", "mean_pi", "mean_zf", "mean_k"):
            assert np.array_equal(ga[k], gb[k]), k
        assert gb["valid"] == [FR.valid_rect(mask.shape, r, BOX) for r in HW]
        # beside both spectra riders: all three answer what they answer alone
        for s in (d, e):
            s.start_spectra(SBOX, every=EVERY, start_step=START)
            s.start_cross_spectra(SBOX, PAIR, every=EVERY, start_step=START)
        d.start_scale_fluxes(BOX, HW, every=EVERY, start_step=START)
        d.run(4 * N, graph=True)
        e.run(4 * N, graph=True)
        assert d._graphs and [type(r).__name__ for r in d._riders()] == ["Spectra", "CrossSpectra", "ScaleFluxes"]
        assert np.array_equal(d.scale_fluxes()["sums"], gb["sums"])
        assert np.array_equal(d.spectra()["sums"], e.spectra()["sums"]) and np.array_equal(d.cross_spectra()["sums"], e.cross_spectra()["sums"])
        assert d.spectra()["samples"] == 22 and d.spectra()["sums"].max() > 0
        # the trajectory: with the rider (eager, graphs, beside the others) and without
        c.run(4 * N, graph=True)
        fc = c.field_to_numpy()
        for s in (a, b, d):
            fs_ = s.field_to_numpy()
            for k in fc:
                assert np.array_equal(fs_[k], fc[k]), f"{k}: the rider changed the trajectory"
        b.reset_scale_fluxes()
        assert b.scale_fluxes()["samples"] == 0 and not b.scale_fluxes()["sums"].any()
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        fx, dev = b._fluxr.flux, b._dev
        h, v = fx._h, b._solver.get_fields()[0]
        gid = dev.capture(lambda: (dev.flux_launch(fx, v), b.stop_scale_fluxes()))
        dev.free_graph(gid)
        assert b._fluxr is None and fx._h is None
        from fs import _lib
        with pytest.raises(_lib.FsError):                        # the handle is gone
            _lib.call("fs_flux_read", dev._ctx, h, None, None, None)
        with pytest.raises(RuntimeError):
            b.scale_fluxes()
    finally:
        for s in sims:
            _close(s)


def test_refusals(hip_lib):
    from fs import _lib
    sim, mask = _make()
    dev = sim._dev
    try:
        for bad in ((0, 0, 0, 8), (60, 0, 68, 8), (-8, 0, 8, 8), (0, 0, 8)):
            for call in (sim.start_scale_fluxes, sim.scale_flux):
                with pytest.raises(ValueError, match="box"):
                    call(bad, (1,))
        for bad in ((0,), (65,), (2, 2), (3, 1), (), tuple(range(1, 10)), (15,)):
            for call in (sim.start_scale_fluxes, sim.scale_flux):
                with pytest.raises(ValueError, match="half"):
                    call(BOX, bad)
        assert sim._fluxr is None
        with pytest.raises(RuntimeError):
            sim.scale_fluxes()
        sim.start_scale_fluxes(BOX, HW)
        with pytest.raises(RuntimeError, match="attached"):
            sim.start_scale_fluxes(BOX, HW)
        for call in (sim.scale_fluxes, sim.reset_scale_fluxes, lambda: sim.scale_flux(BOX, HW), lambda: sim.filtered_fields(BOX, 1),
                     lambda: sim.start_scale_fluxes(BOX, HW)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        h = sim._fluxr.flux._h
        out = np.zeros(8 * 53 * 27)
        dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ll = ctypes.c_longlong
        for call in (lambda: _lib.call("fs_flux_read", dev._ctx, h, None, None, None), lambda: _lib.call("fs_flux_reset", dev._ctx, h),
                     lambda: _lib.call("fs_flux_filtered", dev._ctx, h, 0, dp), lambda: _lib.call("fs_flux_set", dev._ctx, h, dp, ll(1), ll(0)),
                     lambda: _lib.call("fs_flux_get", dev._ctx, h, dp, ctypes.byref(ll()), ctypes.byref(ll()))):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        with pytest.raises(_lib.FsError, match="width"):
            _lib.call("fs_flux_filtered", dev._ctx, h, 2, dp)              # an index past the object's half-widths
        # the library's own argument checks
        hh = ctypes.c_void_p()

        def create(ctx, box, hw=(1, 3), dx=0.5, every=1, start=0):
            return dev._lib.fs_flux_create(ctx, (ctypes.c_int * 4)(*box), len(hw), (ctypes.c_int * max(len(hw), 1))(*hw), dx, every, start,
                                           ctypes.byref(hh))
        assert create(dev._ctx, (0, 0, 8, 8)) == 0 and hh.value
        _lib.call("fs_flux_free", dev._ctx, hh)
        with pytest.raises(_lib.FsError, match="freed"):
            _lib.call("fs_flux_reset", dev._ctx, hh)                      # a stale handle
        hh = ctypes.c_void_p()
        with pytest.raises(_lib.FsError) as err:
            dev.capture(lambda: _lib.check(create(dev._ctx, (0, 0, 8, 8))))      # the library's create inside a capture
        assert "capture" in str(err.value) and not hh.value
        ok = dict(box=(0, 0, 64, 32))
        for kw in (dict(box=(0, 0, 0, 8)), dict(box=(60, 0, 68, 8)), dict(box=(-8, 0, 8, 8)), dict(ok, every=0), dict(ok, start=-1),
                   dict(ok, hw=()), dict(ok, hw=tuple(range(1, 10))), dict(ok, hw=(0,)), dict(ok, hw=(65,)), dict(ok, hw=(2, 2)), dict(ok, hw=(3, 1)),
                   dict(ok, hw=(15,)), dict(box=(0, 0, 2, 32), hw=(1,)), dict(ok, dx=0.0), dict(ok, dx=-1.0), dict(ok, dx=float("inf")),
                   dict(ok, dx=float("nan"))):
            assert create(dev._ctx, **kw) == -1 and not hh.value, kw      # FS_ERR_ARG
            assert dev._lib.fs_last_error()
        assert create(dev._ctx, hw=(14,), **ok) == 0 and hh.value         # the largest half-width with a valid cell on 64 x 32
        _lib.call("fs_flux_free", dev._ctx, hh)
        hh = ctypes.c_void_p()
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert create(slab, (0, 0, 64, 16)) == -5 and not hh.value    # FS_ERR_UNSUPPORTED
            assert "single-GPU" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)
        sim.stop_scale_fluxes()
        saved = dev.nranks
        dev.nranks = 2
        try:
            for call in (lambda: sim.start_scale_fluxes(BOX, HW), lambda: sim.scale_flux(BOX, HW), lambda: sim.filtered_fields(BOX, 1)):
                with pytest.raises(_lib.FsError, match="single-GPU"):
                    call()
        finally:
            dev.nranks = saved
    finally:
        _close(sim)
