"""The cross-spectra on the GPU (csrc/fs_xspec.h, host code in csrc/fs_diag.hip, fs/spectra.py): every plane with == against the NumPy
restatement (tests/xspec_ref.py) fed with downloads of the same fields and the same tables - no tolerance anywhere but the 16 eps relation
between Paa + Pbb and the power of the packed plane.

Part one, the planes: boxes on bc5 res 64 (grid 128 x 64) under a random velocity and pressure that are not zero inside the walls - the
smallest box, 16 x 8 and 8 x 16, 64 x 32 at an odd offset over the slotted wall, the whole grid (the gradients clamp at its edges) - f32 and
f64, five pairs that between them load every quantity, both windows; the mirror index at log2 N = 12 in each direction, f32 and f64; rows
of 512, 256 and 128 points on the grids 512 x 256 and 256 x 512 of tests/test_gpu_spec.py (32 and 8 workgroups), f32 and f64; a deferred
limit_field.  Part two, the rider on bc1 res 32: eager steps against the NumPy loop, replayed graphs, a non-sampling launch, the checkpoint
round trip, beside start_spectra, the unchanged trajectory, the refusals."""
import ctypes
import functools

import numpy as np
import pytest
from test_gpu_dist import _load, _sim
from test_gpu_spec import BOXES_128x64, MID_BOXES, MID_GRIDS, NP_DTYPE, _assert_walls_carry_values, _make, _scene5, _tabs, _velocity
from test_gpu_vortices import _close

import spec_ref as S
import xspec_ref as XR

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
COMBOS = (("hann", True), ("boxcar", False))
PAIRS = (("u", "w"), ("p", None), ("vorticity", "p"), ("speed", "q"), ("swirl", "w"))
Q = {name: k for k, name in enumerate(XR.QUANTITIES)}


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _q(pair):
    return Q[pair[0]], (-1 if pair[1] is None else Q[pair[1]])


@functools.lru_cache(maxsize=None)
def _pressure(shape, dtype):
    p = np.random.default_rng(11).normal(0.1, 2.0, shape).astype(dtype)
    p.setflags(write=False)
    return p


def _assert_symmetries(sums, re, im):
    """The relations of tests/test_xspec_cpu.py on the device's planes."""
    paa, pbb, cre, cim = sums
    assert np.array_equal(paa, XR.mirrored(paa)) and np.array_equal(pbb, XR.mirrored(pbb)) and np.array_equal(cre, XR.mirrored(cre))
    assert np.array_equal(cim, -XR.mirrored(cim))
    p = S.power_of(re, im)
    want = 0.5 * (p + XR.mirrored(p))
    assert np.all(np.abs((paa + pbb) - want) <= 16 * EPS * want)


def _assert_box(sim, v, p, mask, dx, box, pair, combos=COMBOS):
    """pair_fft and cross_spectrum of `box` against the restatement on the downloaded fields."""
    nx, ny = box[2] - box[0], box[3] - box[1]
    qa, qb = _q(pair)
    for window, detrend in combos:
        re, im = XR.plane(qa, qb, v, p, mask, dx, box, _tabs(nx, ny, window), detrend)
        Z = sim.pair_fft(box, pair, window=window, detrend=detrend)
        assert Z.shape == (nx, ny) and Z.dtype == np.complex128
        bad = int((Z.real != re).sum() + (Z.imag != im).sum())
        assert bad == 0, (box, pair, window, detrend, bad, float(np.abs(Z.real - re).max()), float(np.abs(Z.imag - im).max()))
        x = sim.cross_spectrum(box, pair, window=window, detrend=detrend)
        want = XR.accumulate(np.zeros((4 if qb >= 0 else 1, nx, ny)), re, im)
        assert x["sums"].shape == want.shape
        for n, name in enumerate(("Paa", "Pbb", "Cre", "Cim")[:len(want)]):
            assert np.array_equal(x["sums"][n], want[n]), (box, pair, window, detrend, name)
        assert x["samples"] == 1 and x["sample_steps"].tolist() == [0] and x["box"] == tuple(box) and x["quantities"] == pair
        assert np.abs(Z).max() > 0, "an empty plane: the test covers nothing"
        if qb >= 0:
            assert np.abs(Z.imag).max() > 0 and np.abs(x["sums"][3]).max() > 0
            _assert_symmetries(x["sums"], re, im)
        if pair == ("u", "w"):
            B = sim.box_fft(box, window=window, detrend=detrend)
            assert np.array_equal(Z.real, B.real) and np.array_equal(Z.imag, B.imag), "pair_fft(u, w) is not box_fft"


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(BOXES_128x64))
def test_boxes_on_bc5_res64_equal_the_restatement(name, dtype, hip_lib):
    const, mask = _scene5()
    box = BOXES_128x64[name]
    dx = 1.0 / 64
    sim, mask = _sim((const, mask), dx, dtype)
    try:
        assert mask.shape == (128, 64)
        np_dtype = "float32" if dtype == "f32" else "float64"
        v, p = _load(sim, _velocity(mask.shape, np_dtype), _pressure(mask.shape, np_dtype))
        if "wall" in name or "whole" in name:
            walls = mask[box[0]:box[2], box[1]:box[3]] == 1
            sub_v, sub_p = v[box[0]:box[2], box[1]:box[3]], p[box[0]:box[2], box[1]:box[3]]
            assert walls.any() and (sub_v[walls] != 0).any() and (sub_p[walls] != 0).any(), "no wall cell with stored values in the box"
            other = (mask[box[0]:box[2], box[1]:box[3]] > 1)
            assert other.any() or "wall" in name, "no cell that is neither fluid nor wall: the two selection rules are not told apart"
        for pair in PAIRS:
            _assert_box(sim, v, p, mask, dx, box, pair)
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", [(4096, 8), (8, 4096)], ids=["4096x8", "8x4096"])
def test_mirror_index_on_the_longest_rows(grid, dtype, hip_lib):
    """The whole grid as the box: the mirror (N - a) mod N at log2 N = 12 along x and along y, and the gradient's clamped neighbours."""
    from multigrid_cases import scene
    dx = 1.0 / max(grid)
    sim, mask = _sim(scene(grid[0], grid[1], 0.1), dx, dtype)
    try:
        v, p = _load(sim, _velocity(mask.shape, NP_DTYPE[dtype], seed=4), _pressure(mask.shape, NP_DTYPE[dtype]))
        assert (mask == 1).any()
        _assert_box(sim, v, p, mask, dx, (0, 0) + tuple(grid), ("vorticity", "u"), combos=(("hann", True),))
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid,name", list(MID_BOXES), ids=[f"{g} {n}" for g, n in MID_BOXES])
def test_rows_of_256_and_512(grid, name, dtype, hip_lib):
    """The grids and boxes of tests/test_gpu_spec.py: rows of 512, 256 and 128 points, planes of 32 and of 8 workgroups; a pair that reads
    the gradient and the pressure, and the pair that is box_fft."""
    from multigrid_cases import scene
    X, Y = MID_GRIDS[grid]
    box = MID_BOXES[grid, name]
    dx = 1.0 / max(X, Y)
    sim, mask = _sim(scene(X, Y, 0.1), dx, dtype)
    try:
        assert mask.shape == (X, Y) and 0 <= box[0] < box[2] <= X and 0 <= box[1] < box[3] <= Y
        v, p = _load(sim, _velocity(mask.shape, NP_DTYPE[dtype], seed=4), _pressure(mask.shape, NP_DTYPE[dtype]))
        _assert_walls_carry_values(mask, box, v, p)
        for pair in (("vorticity", "p"), ("u", "w")):
            _assert_box(sim, v, p, mask, dx, box, pair)
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_planes(hip_lib):
    """The case of tests/test_gpu_spec.py with (vorticity, u): the centre value and the four neighbours of the gradient are limited."""
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
        pair = ("vorticity", "u")
        assert box[2] <= mask.shape[0] and box[3] <= mask.shape[1]
        sim.start_cross_spectra(box, pair, window="hann", detrend=True)
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        Z = sim.pair_fft(box, pair, window="hann", detrend=True)
        rider = sim.cross_spectra()
        assert cur.pending_limit is not None, "reading the planes flushed the owed pass"
        down = sim.field_to_numpy()                           # (the download launches the owed pass first)
        sub = down["v"][box[0]:box[2], box[1]:box[3]]
        assert np.hypot(sub[..., 0], sub[..., 1]).max() > 0.99 * VELOCITY_LIMIT, "no cell of the box at the limit: the test does not cover it"
        re, im = XR.plane(Q["vorticity"], Q["u"], down["v"], down["p"], mask, sim._solver.dx, box, _tabs(32, 16, "hann"), True)
        assert np.array_equal(Z.real, re) and np.array_equal(Z.imag, im)
        assert rider["samples"] == 1 and np.array_equal(rider["sums"], XR.accumulate(np.zeros((4, 32, 16)), re, im))
    finally:
        _close(sim)


# ---- the rider on bc1 res 32 ----------------------------------------------------------------------------------------------------------------
RES, BOX, EVERY, START, N = 32, (9, 8, 41, 24), 2, 3, 12
PAIR = ("vorticity", "p")


def _sampled(first, last):
    return [k for k in range(first, last + 1) if k > START and (k - START) % EVERY == 0]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rider_eager_graph_and_resumed_equal_the_numpy_loop(dtype, hip_lib):
    """a: eager, through a checkpoint; b: run(graph=True); c: no rider; d: the cross-spectrum beside start_spectra; e: start_spectra alone."""
    made = [_make(dtype) for _ in range(5)]
    sims, mask = [m[0] for m in made], made[0][1]
    a, b, c, d, e = sims
    try:
        assert (mask[BOX[0]:BOX[2], BOX[1]:BOX[3]] == 1).any(), "the box misses the cylinder"
        dx = a._solver.dx
        tabs = _tabs(BOX[2] - BOX[0], BOX[3] - BOX[1], "hann")
        ref = XR.State(BOX, *_q(PAIR), dx, tabs, True, EVERY, START)

        def follow(steps):
            for _ in range(steps):
                a.step()
                f = a.field_to_numpy()
                ref.launch(f["v"], f["p"], mask)

        a.start_cross_spectra(BOX, PAIR, every=EVERY, start_step=START)
        for n in range(1, N + 1):
            before = a.cross_spectra()["sums"]
            follow(1)
            got = a.cross_spectra()
            assert np.array_equal(got["sums"], ref.sums), (dtype, n)
            assert got["samples"] == ref.samples and a._dev.xspec_read(a._xspectrar.xspec, sums=False)[1:] == (ref.launches, ref.samples)
            if n not in _sampled(1, N):
                assert np.array_equal(got["sums"], before), f"the non-sampling launch {n} touched the planes"
        got = a.cross_spectra()
        assert got["sample_steps"].tolist() == _sampled(1, N) and got["samples"] == 4
        assert all(np.abs(got["sums"][n]).max() > 0 for n in range(4))
        Zp = a._dev.xspec_plane(a._xspectrar.xspec)
        assert np.array_equal(Zp.real, ref.re) and np.array_equal(Zp.imag, ref.im)
        # the same steps under run(graph=True)
        b.start_cross_spectra(BOX, PAIR, every=EVERY, start_step=START)
        b.run(N, graph=True)
        assert np.array_equal(b.cross_spectra()["sums"], got["sums"]) and b.cross_spectra()["samples"] == 4
        # twelve more: a through a checkpoint into a fresh object, eager; b under run(graph=True)
        z = {k: np.array(x) for k, x in a._xspectrar.checkpoint().items()}
        assert (int(z["xspec.launches"]), int(z["xspec.samples"])) == (N, 4)
        a.stop_cross_spectra()
        a.start_cross_spectra(BOX, PAIR, every=EVERY, start_step=START)
        assert a.cross_spectra()["samples"] == 0 and not a.cross_spectra()["sums"].any()
        assert a._xspectrar.restore(z) == 4
        follow(N)
        b.run(N, graph=True)
        ga, gb = a.cross_spectra(), b.cross_spectra()
        assert np.array_equal(ga["sums"], ref.sums) and np.array_equal(gb["sums"], ref.sums)
        assert ga["samples"] == gb["samples"] == ref.samples == 10 and ga["sample_steps"].tolist() == gb["sample_steps"].tolist() == _sampled(1, 2 * N)
        # run() captures a period only in a chunk of 16 steps or more: 24 more, so that the launches are replayed from a graph
        follow(2 * N)
        b.run(2 * N, graph=True)
        assert b._graphs, "the run replayed no graph"
        ga, gb = a.cross_spectra(), b.cross_spectra()
        assert np.array_equal(ga["sums"], ref.sums) and np.array_equal(gb["sums"], ref.sums)
        assert ga["samples"] == gb["samples"] == ref.samples == 22 and gb["sample_steps"].tolist() == _sampled(1, 4 * N)
        for k in ("spectrum_a", "spectrum_b", "co", "quad", "Co", "Quad"):
            assert np.array_equal(ga[k], gb[k]), k
        paa, pbb, cre, cim = gb["sums"]                          # a bin and its mirror add the same terms in the same order, sample after sample
        assert np.array_equal(paa, XR.mirrored(paa)) and np.array_equal(pbb, XR.mirrored(pbb)) and np.array_equal(cre, XR.mirrored(cre))
        assert np.array_equal(cim, -XR.mirrored(cim))
        # beside start_spectra: both results are those of each alone
        d.start_spectra(BOX, every=EVERY, start_step=START)
        d.start_cross_spectra(BOX, PAIR, every=EVERY, start_step=START)
        e.start_spectra(BOX, every=EVERY, start_step=START)
        d.run(4 * N, graph=True)
        e.run(4 * N, graph=True)
        assert d._graphs and [type(r).__name__ for r in d._riders()] == ["Spectra", "CrossSpectra"]
        assert np.array_equal(d.cross_spectra()["sums"], gb["sums"]) and np.array_equal(d.spectra()["sums"], e.spectra()["sums"])
        assert d.spectra()["samples"] == 22 and d.spectra()["sums"].max() > 0
        # the trajectory: with the rider (eager, graphs, beside the other) and without
        c.run(4 * N, graph=True)
        fc = c.field_to_numpy()
        for s in (a, b, d):
            fs_ = s.field_to_numpy()
            for k in fc:
                assert np.array_equal(fs_[k], fc[k]), f"{k}: the rider changed the trajectory"
        b.reset_cross_spectra()
        assert b.cross_spectra()["samples"] == 0 and not b.cross_spectra()["sums"].any()
        b.stop_cross_spectra()
        with pytest.raises(RuntimeError):
            b.cross_spectra()
    finally:
        for s in sims:
            _close(s)


def test_refusals(hip_lib):
    from fs import _lib
    sim, mask = _make()
    dev = sim._dev
    try:
        for bad in ((0, 0, 12, 8), (0, 0, 4, 8), (0, 0, 8, 64), (60, 0, 68, 8), (-8, 0, 0, 8), (0, 0, 8)):
            for call in (sim.start_cross_spectra, sim.cross_spectrum, sim.pair_fft):
                with pytest.raises(ValueError, match="box|sides"):
                    call(bad)
        for bad in (("u", "dye"), ("vort", "p"), (None, "u"), ("u",), 3):
            for call in (sim.start_cross_spectra, sim.cross_spectrum, sim.pair_fft):
                with pytest.raises(ValueError, match="quantity|pair"):
                    call(BOX, bad)
        with pytest.raises(ValueError, match="window"):
            sim.start_cross_spectra(BOX, window="kaiser")
        assert sim._xspectrar is None
        with pytest.raises(RuntimeError):
            sim.cross_spectra()
        sim.start_cross_spectra(BOX, PAIR)
        with pytest.raises(RuntimeError, match="attached"):
            sim.start_cross_spectra(BOX, PAIR)
        for call in (sim.cross_spectra, sim.reset_cross_spectra, lambda: sim.cross_spectrum(BOX), lambda: sim.pair_fft(BOX),
                     lambda: sim.start_cross_spectra(BOX)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        h = sim._xspectrar.xspec._h
        out = np.zeros(4 * 32 * 16)
        dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ll = ctypes.c_longlong
        for call in (lambda: _lib.call("fs_xspec_read", dev._ctx, h, None, None, None), lambda: _lib.call("fs_xspec_reset", dev._ctx, h),
                     lambda: _lib.call("fs_xspec_plane", dev._ctx, h, dp), lambda: _lib.call("fs_xspec_set", dev._ctx, h, dp, ll(1), ll(0)),
                     lambda: _lib.call("fs_xspec_get", dev._ctx, h, dp, ctypes.byref(ll()), ctypes.byref(ll()))):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        # the library's own argument checks
        hh = ctypes.c_void_p()

        def create(ctx, box, qa=4, qb=2, dx=0.5, every=1, start=0, c1=0.0):
            nx, ny = max(box[2] - box[0], 2), max(box[3] - box[1], 2)
            t = [np.ones(n) for n in (nx, ny, nx, ny)]
            p = [x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for x in t]
            return dev._lib.fs_xspec_create(ctx, (ctypes.c_int * 4)(*box), qa, qb, dx, *p, c1, c1, 1, every, start, ctypes.byref(hh))
        assert create(dev._ctx, (0, 0, 8, 8)) == 0 and hh.value
        _lib.call("fs_xspec_free", dev._ctx, hh)
        with pytest.raises(_lib.FsError, match="freed"):
            _lib.call("fs_xspec_reset", dev._ctx, hh)                     # a stale handle
        hh = ctypes.c_void_p()
        with pytest.raises(_lib.FsError) as err:
            dev.capture(lambda: _lib.check(create(dev._ctx, (0, 0, 8, 8))))      # the library's create inside a capture
        assert "capture" in str(err.value) and not hh.value
        ok = dict(box=(0, 0, 8, 8))
        for kw in (dict(box=(0, 0, 12, 8)), dict(box=(0, 0, 4, 8)), dict(box=(0, 0, 8, 64)), dict(box=(-8, 0, 0, 8)), dict(ok, every=0),
                   dict(ok, start=-1), dict(ok, c1=float("nan")), dict(ok, qa=-1), dict(ok, qa=7), dict(ok, qb=-2), dict(ok, qb=7),
                   dict(ok, dx=0.0), dict(ok, dx=-1.0), dict(ok, dx=float("inf")), dict(ok, dx=float("nan"))):
            assert create(dev._ctx, **kw) == -1 and not hh.value, kw      # FS_ERR_ARG
            assert dev._lib.fs_last_error()
        assert create(dev._ctx, qb=-1, **ok) == 0 and hh.value           # one scalar
        _lib.call("fs_xspec_free", dev._ctx, hh)
        hh = ctypes.c_void_p()
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert create(slab, (0, 0, 8, 8)) == -5 and not hh.value      # FS_ERR_UNSUPPORTED
            assert "single-GPU" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)
        sim.stop_cross_spectra()
        saved = dev.nranks
        dev.nranks = 2
        try:
            for call in (lambda: sim.start_cross_spectra(BOX), lambda: sim.cross_spectrum(BOX), lambda: sim.pair_fft(BOX)):
                with pytest.raises(_lib.FsError, match="single-GPU"):
                    call()
        finally:
            dev.nranks = saved
    finally:
        _close(sim)
