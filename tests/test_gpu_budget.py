"""The kinetic-energy budget on the GPU (csrc/fs_budget.h, host code in csrc/fs_diag.hip, fs/budgets.py): every plane with == against the
NumPy restatement (tests/budget_ref.py) fed with downloads of the same fields - no tolerance anywhere.

The rider on bc3 res 32 (grid 64 x 32), 16 steps, every 2 from step 3, three boxes - (3, 2, 60, 29): odd origin and odd width 57, the scalar
kernel; the whole grid: the 16-byte kernel and clamped differences on all four edges; (7, 5, 8, 6): one cell -, f32 and f64: eager steps,
replayed graphs, a run resumed through a checkpoint, the averager's planes, the unchanged trajectory, beside three other riders, the
signatures.  Grids past one workgroup in x and in y for both widths of the kernel.  budget_sample, a deferred limit that bites, the round
trip of get / reset / set, and the refusals."""
import ctypes

import numpy as np
import pytest
from test_budget_cpu import limits
from test_gpu_dist import _load, _sim
from test_gpu_spec import NP_DTYPE, _velocity
from test_gpu_vortices import _close

import budget_ref as BR

pytestmark = pytest.mark.gpu

BOXES = {"odd origin, odd width": (3, 2, 60, 29), "whole grid": (0, 0, 64, 32), "one cell": (7, 5, 8, 6)}
EVERY, START, N = 2, 3, 16
HW = (1, 3)


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _make(dtype="f32"):
    import fs
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(3, 32)
    dx = 1.0 / 32
    fs.runtime.init(gpu=0, dtype=dtype)
    bc = fs.BoundaryCondition(np.array(const), np.array(mask))
    dt = 0.05 * dx
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None)), np.array(mask)


def _sampled(first, last):
    return [k for k in range(first, last + 1) if k > START and (k - START) % EVERY == 0]


def _same(got, want, what):
    bad = int((got != want).sum())
    assert got.shape == want.shape and bad == 0, (what, bad, float(np.abs(got - want).max()))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(BOXES))
def test_rider_eager_graph_and_resumed_equal_the_numpy_loop(name, dtype, hip_lib):
    """a: eager, through a checkpoint halfway, beside the averager; b: run(graph=True); c: no rider; d: the budget beside the averager, the
    distributions and the scale fluxes; e: those three alone."""
    box = BOXES[name]
    made = [_make(dtype) for _ in range(5)]
    sims, mask = [m[0] for m in made], made[0][1]
    a, b, c, d, e = sims
    try:
        assert mask.shape == (64, 32)
        fluid = mask[box[0]:box[2], box[1]:box[3]] == 0
        dx = a._solver.dx
        ref = BR.State(box, dx, EVERY, START)

        def follow(steps):
            for _ in range(steps):
                a.step()
                f = a.field_to_numpy()
                ref.launch(f["v"], f["p"], mask)

        a.start_budget(box, every=EVERY, start_step=START)
        a.start_averaging(every=EVERY, start_step=START)
        follow(N // 2)
        _same(a.budget()["sums"], ref.sums, (name, dtype, "eager, first half"))
        z = {k: np.array(x) for k, x in a._budgetr.checkpoint().items()}
        assert (int(z["budget.launches"]), int(z["budget.samples"])) == (N // 2, len(_sampled(1, N // 2)))
        a.stop_budget()
        a.start_budget(box, every=EVERY, start_step=START)
        assert a.budget()["samples"] == 0 and not a.budget()["sums"].any()
        assert a._budgetr.restore(z) == len(_sampled(1, N // 2))
        follow(N - N // 2)
        ga = a.budget()
        _same(ga["sums"], ref.sums, (name, dtype, "eager, resumed"))
        assert ga["samples"] == ref.samples == len(_sampled(1, N)) and ga["sample_steps"].tolist() == _sampled(1, N)
        assert np.array_equal(ga["fluid"], fluid) and not ga["sums"][:, ~fluid].any()
        if fluid.sum() > 1:
            assert all(np.abs(ga["sums"][k]).max() > 0 for k in range(BR.NPLANE)), "an empty plane: the test covers nothing"
        # planes 0 - 5 are the averager's on the fluid cells of the box, bit for bit
        avg = a._dev.mean_read(a._averager.mean)[0][:, box[0]:box[2], box[1]:box[3]]
        for k in range(6):
            assert np.array_equal(ga["sums"][k][fluid], avg[k][fluid]), (name, dtype, k)
        # the same steps under run(graph=True): a chunk of 16 steps is captured and replayed
        b.start_budget(box, every=EVERY, start_step=START)
        b.run(N, graph=True)
        assert b._graphs, "the run replayed no graph"
        gb = b.budget()
        _same(gb["sums"], ref.sums, (name, dtype, "graphs"))
        assert gb["samples"] == ref.samples and gb["sample_steps"].tolist() == _sampled(1, N)
        for k in ("production", "dissipation", "residual"):
            assert np.array_equal(ga[k], gb[k]), k
        for sig in b._graphs:
            kinds = [t[0] for t in sig if isinstance(t, tuple)]
            assert "budget" in kinds, sig
        # beside mean + distributions + scale fluxes: every reader returns what it returns alone
        for s in (d, e):
            s.start_averaging(every=EVERY, start_step=START)
            s.start_distributions([dict(quantity="u", bins=16, range=(-1.0, 1.0))], every=EVERY, start_step=START)
            s.start_scale_fluxes(BOXES["odd origin, odd width"], HW, every=EVERY, start_step=START)
        d.start_budget(box, every=EVERY, start_step=START)
        d.run(N, graph=True)
        e.run(N, graph=True)
        assert d._graphs and [type(r).__name__ for r in d._riders()] == ["Averager", "Distributions", "ScaleFluxes", "Budget"]
        _same(d.budget()["sums"], ref.sums, (name, dtype, "beside three riders"))
        assert np.array_equal(d._dev.mean_read(d._averager.mean)[0], e._dev.mean_read(e._averager.mean)[0])
        assert np.array_equal(d.scale_fluxes()["sums"], e.scale_fluxes()["sums"])
        dd, de = d.distributions(), e.distributions()
        assert np.array_equal(dd[0]["counts"], de[0]["counts"]) and dd[0]["samples"] == de[0]["samples"] == ref.samples and dd[0]["counts"].sum() > 0
        for sig in d._graphs:
            kinds = [t[0] for t in sig if isinstance(t, tuple)]
            assert kinds.index("budget") == kinds.index("flux") + 1, sig
        d.stop_budget()
        for sig in d._graphs:
            assert "budget" not in [t[0] for t in sig if isinstance(t, tuple)], sig
        assert "budget" not in [t[0] for t in d._signature() if isinstance(t, tuple)]
        # the trajectory: with the rider (eager, graphs, beside the others) and without
        c.run(N, graph=True)
        fc = c.field_to_numpy()
        for s in (a, b, d):
            fs_ = s.field_to_numpy()
            for k in fc:
                assert np.array_equal(fs_[k], fc[k]), f"{k}: the rider changed the trajectory"
    finally:
        for s in sims:
            _close(s)


# name: (grid, box, FS_DIAG_WGS or None, columns per lane)
WIDE = {"scalar kernel, 2 x 7 workgroups": ((320, 160), (3, 5, 304, 32), None, 1),
        "16-byte kernel, 2 x 7 workgroups": ((640, 136), (3, 5, 525, 32), None, 2),
        "scalar kernel, 32 rows per workgroup": ((320, 160), (3, 5, 304, 80), "1", 1)}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(WIDE))
def test_past_one_workgroup_in_both_directions(name, dtype, hip_lib, monkeypatch):
    """A workgroup of k_budget_accumulate takes 256 W columns - W = 2 when the box's width is even, else 1 - and BUDGET_ROWS0 = 4 rows on a
    grid this small (BUDGET_ROWS = 32 with FS_DIAG_WGS=1, the big grids' shape).  More than one workgroup in x therefore needs a box wider
    than 256 (W = 1; grid 320 x 160, res 160) or 512 (W = 2; grid 640 x 136, res 320) columns.  The boxes start at an odd x0, cross the
    workgroup edge in x, and their heights 27 and 75 are multiples of neither 4 nor 32, nor of the load group (2 rows at W = 1).  4 steps,
    every = 1."""
    from multigrid_cases import scene
    (X, Y), box, wgs, w = WIDE[name]
    L = limits()
    if wgs is None:
        monkeypatch.delenv("FS_DIAG_WGS", raising=False)
    else:
        monkeypatch.setenv("FS_DIAG_WGS", wgs)
    rows = L["rows0"] if wgs is None else L["rows"]
    nx, ny = box[2] - box[0], box[3] - box[1]
    group = L["cells"] // w                                # rows per load group
    assert box[0] % 2 == 1 and (2 if nx % 2 == 0 else 1) == w and nx > 256 * w and ny > rows and ny % rows and (group == 1 or ny % group)
    assert max(X, Y) <= 640
    dx = 1.0 / max(X, Y)
    sim, mask = _sim(scene(X, Y, 0.1), dx, dtype)
    try:
        rng = np.random.default_rng(8)
        _load(sim, _velocity(mask.shape, NP_DTYPE[dtype], seed=6), rng.normal(0, 2, mask.shape).astype(NP_DTYPE[dtype]))
        sub = mask[box[0]:box[2], box[1]:box[3]]
        assert (sub == 0).any() and (sub != 0).any()
        sim.start_budget(box)
        ref = BR.State(box, dx, 1, 0)
        for _ in range(4):
            sim.step()
            f = sim.field_to_numpy()
            ref.launch(f["v"], f["p"], mask)
        got = sim.budget()
        assert got["samples"] == 4
        for k, plane in enumerate(BR.NAMES):
            _same(got["sums"][k], ref.sums[k], (name, dtype, plane))
        assert all(np.abs(got["sums"][k]).max() > 0 for k in range(BR.NPLANE))
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_budget_sample_is_the_first_sample_of_a_fresh_rider(dtype, hip_lib):
    sim, mask = _make(dtype)
    try:
        sim.run(5)
        box = BOXES["odd origin, odd width"]
        graphs = len(sim._graphs)
        once, whole = sim.budget_sample(box), sim.budget_sample()
        assert len(sim._graphs) == graphs and sim._budgetr is None, "the one-shot call captured a graph or attached a rider"
        assert once["samples"] == 1 and once["sample_steps"].tolist() == [0] and once["box"] == box and whole["box"] == (0, 0, 64, 32)
        f = sim.field_to_numpy()
        ref = BR.State(box, sim._solver.dx, 1, 0)
        ref.launch(f["v"], f["p"], mask)
        _same(once["sums"], ref.sums, "budget_sample")
        _same(whole["sums"][:, box[0]:box[2], box[1]:box[3]], ref.sums, "budget_sample of the whole grid")
        # a fresh rider's first sample on the same fields: its launch alone, without a step
        sim.start_budget(box, every=1)
        v, p = sim._solver.get_fields()[:2]
        sim._dev.budget_launch(sim._budgetr.budget, v, p)
        first = sim.budget()
        assert first["samples"] == 1
        _same(first["sums"], once["sums"], "the first sample of start_budget(every=1)")
    finally:
        _close(sim)


def test_deferred_limit_reaches_the_planes(hip_lib):
    """The arrangement of tests/test_gpu_flux.py: speeds above the limit are uploaded, a step leaves the limit pass owed, and the launch of
    the rider - and the one-shot call - limit the cell's values and the four neighbours of its gradient."""
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
        assert VELOCITY_LIMIT == 10.0
        mask = g["bc_mask"]
        i = np.arange(mask.shape[0])[:, None] * np.ones(mask.shape[1])[None, :]
        v = np.zeros(mask.shape + (2,), np.float32)
        v[..., 0] = 3.0 * VELOCITY_LIMIT * np.sin(i / 3.0)
        v[..., 1] = -2.0 * VELOCITY_LIMIT * np.cos(i / 5.0)
        v[mask != 0] = 0
        sim._solver.v.current.from_numpy(v)
        box = (2, 1, 2 + 33, 1 + 16)
        assert box[2] <= mask.shape[0] and box[3] <= mask.shape[1]
        sim.start_budget(box)
        sim.step()
        cur = sim._solver.v.current
        assert cur.pending_limit is not None, "the limit pass was not deferred: the test does not cover it"
        assert dev.field_hot(cur), "the flag is down: the owed pass would change no cell and the test does not cover it"
        assert dev._limit_of(cur) == 10.0
        once = sim.budget_sample(box)
        rider = sim.budget()
        assert cur.pending_limit is not None, "reading the planes flushed the owed pass"
        # the same values without the limit: the stored speeds exceed it, so the planes must differ
        raw = BR.State(box, sim._solver.dx, 1, 0)
        h = sim._budgetr.budget._h
        p = sim._solver.p.current
        down = sim.field_to_numpy()                           # (the download launches the owed pass first)
        sub = down["v"][box[0]:box[2], box[1]:box[3]]
        assert np.hypot(sub[..., 0], sub[..., 1]).max() > 0.99 * VELOCITY_LIMIT, "no cell of the box at the limit: the test does not cover it"
        ref = BR.State(box, sim._solver.dx, 1, 0)
        ref.launch(down["v"], down["p"], mask)
        _same(once["sums"], ref.sums, "budget_sample with the limit owed")
        _same(rider["sums"], ref.sums, "the rider with the limit owed")
        assert rider["samples"] == 1 and np.abs(ref.sums[12]).max() > 0
        # the restatement's own limit = 10 on fields above it gives the same planes as the pass followed by no limit
        big = down["v"] * np.float32(1.0)
        over = np.hypot(big[..., 0], big[..., 1]) > 0.99 * VELOCITY_LIMIT
        big[over] *= np.float32(2.5)
        sim._solver.v.current.from_numpy(big)
        held = sim.field_to_numpy()["v"]
        assert np.array_equal(held, big)
        raw.launch(held, down["p"], mask, limit=10.0)
        from fs import _lib
        _lib.call("fs_budget_reset", dev._ctx, h)
        _lib.call("fs_budget_launch", dev._ctx, h, 10.0, sim._solver.v.current._h, p._h)
        got = sim.budget()
        assert got["samples"] == 1
        _same(got["sums"], raw.sums, "fs_budget_launch with limit = 10 on speeds above 10")
        free = BR.State(box, sim._solver.dx, 1, 0)
        free.launch(held, down["p"], mask)
        assert (free.sums[0] != raw.sums[0]).any() and (free.sums[12] != raw.sums[12]).any(), "the limit did not bite"
    finally:
        _close(sim)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_get_reset_set_and_resume_round_trip(dtype, hip_lib):
    sim, mask = _make(dtype)
    dev = sim._dev
    try:
        box = BOXES["odd origin, odd width"]
        sim.start_budget(box, every=2, start_step=1)
        sim.run(7)                                                   # steps 3, 5, 7 sampled
        bg = sim._budgetr.budget
        sums, launches, samples = dev.budget_get(bg)
        assert (launches, samples) == (7, 3) and sums.shape == (21, 57, 27) and np.abs(sums).max() > 0
        assert np.array_equal(sim.budget()["sums"], sums)
        sim.reset_budget()
        zero, l0, s0 = dev.budget_get(bg)
        assert not zero.any() and not np.signbit(zero).any() and (l0, s0) == (7, 0)
        dev.budget_set(bg, sums, launches, samples)
        back, l1, s1 = dev.budget_get(bg)
        assert np.array_equal(back, sums) and (l1, s1) == (7, 3)
        twin, _ = _make(dtype)
        try:
            twin.start_budget(box, every=2, start_step=1)
            twin.run(11)
            sim.run(4)                                               # steps 9 and 11 sample on both
            a, b = sim.budget(), twin.budget()
            assert a["samples"] == b["samples"] == 5 and np.array_equal(a["sums"], b["sums"])
        finally:
            _close(twin)
    finally:
        _close(sim)


def test_refusals(hip_lib):
    from fs import _lib
    sim, mask = _make()
    other, _ = _make()
    dev = sim._dev
    try:
        X, Y = mask.shape
        for bad in ((0, 0, 0, 8), (60, 0, 68, 8), (-8, 0, 8, 8), (0, 0, 8)):
            for call in (sim.start_budget, sim.budget_sample):
                with pytest.raises(ValueError, match="box"):
                    call(bad)
        solid = np.argwhere(mask != 0)
        i, j = (int(x) for x in solid[0])
        with pytest.raises(ValueError, match="no fluid cell"):
            sim.start_budget((i, j, i + 1, j + 1))
        assert sim._budgetr is None
        with pytest.raises(RuntimeError):
            sim.budget()
        box = BOXES["odd origin, odd width"]
        sim.start_budget(box)
        with pytest.raises(RuntimeError, match="attached"):
            sim.start_budget(box)
        for call in (sim.budget, sim.reset_budget, lambda: sim.budget_sample(box), lambda: sim.start_budget(box)):
            with pytest.raises((_lib.FsError, RuntimeError)):
                dev.capture(call)
        h = sim._budgetr.budget._h
        out = np.zeros(21 * 57 * 27)
        dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ll = ctypes.c_longlong
        for call in (lambda: _lib.call("fs_budget_read", dev._ctx, h, None, None, None), lambda: _lib.call("fs_budget_reset", dev._ctx, h),
                     lambda: _lib.call("fs_budget_set", dev._ctx, h, dp, ll(1), ll(0)),
                     lambda: _lib.call("fs_budget_get", dev._ctx, h, dp, ctypes.byref(ll()), ctypes.byref(ll()))):
            with pytest.raises(_lib.FsError) as err:
                dev.capture(call)                                        # the library refuses as well
            assert "capture" in str(err.value)
        with pytest.raises(_lib.FsError, match="counters"):
            _lib.call("fs_budget_set", dev._ctx, h, dp, ll(1), ll(2))
        # the library's own argument checks
        hh = ctypes.c_void_p()

        def create(ctx, box, dx=0.5, every=1, start=0):
            return dev._lib.fs_budget_create(ctx, *box, dx, every, start, ctypes.byref(hh))
        ok = dict(box=(0, 0, X, Y))
        for kw in (dict(box=(0, 0, 0, 8)), dict(box=(60, 0, 68, 8)), dict(box=(-8, 0, 8, 8)), dict(box=(i, j, i + 1, j + 1)), dict(ok, every=0),
                   dict(ok, start=-1), dict(ok, dx=0.0), dict(ok, dx=-1.0), dict(ok, dx=float("inf")), dict(ok, dx=float("nan"))):
            assert create(dev._ctx, **kw) == -1 and not hh.value, kw      # FS_ERR_ARG
            assert dev._lib.fs_last_error()
        assert "no fluid cell" in (create(dev._ctx, (i, j, i + 1, j + 1)), dev._lib.fs_last_error().decode())[1]
        with pytest.raises(_lib.FsError) as err:
            dev.capture(lambda: _lib.check(create(dev._ctx, (0, 0, 8, 8))))      # the library's create inside a capture
        assert "capture" in str(err.value) and not hh.value
        assert create(dev._ctx, (0, 0, 8, 8)) == 0 and hh.value
        v, p = sim._solver.get_fields()[:2]
        # another context's handle, a handle of another kind, a freed handle: the kind's text, and nothing is read through the handle
        sim.start_averaging()
        mean_h = sim._averager.mean._h
        for ctx, handle in ((other._dev._ctx, hh), (dev._ctx, mean_h)):
            for call in (lambda: _lib.call("fs_budget_read", ctx, handle, None, None, None), lambda: _lib.call("fs_budget_reset", ctx, handle),
                         lambda: _lib.call("fs_budget_launch", ctx, handle, 0.0, v._h, p._h), lambda: _lib.call("fs_budget_free", ctx, handle)):
                with pytest.raises(_lib.FsError, match="budget from another context or freed"):
                    call()
        with pytest.raises(_lib.FsError, match="mean from another context or freed"):
            _lib.call("fs_mean_reset", dev._ctx, hh)                      # the budget's handle is no mean
        _lib.call("fs_budget_free", dev._ctx, hh)
        for call in (lambda: _lib.call("fs_budget_reset", dev._ctx, hh), lambda: _lib.call("fs_budget_read", dev._ctx, hh, None, None, None),
                     lambda: _lib.call("fs_budget_launch", dev._ctx, hh, 0.0, v._h, p._h)):
            with pytest.raises(_lib.FsError, match="budget from another context or freed"):
                call()                                                   # use after free
        hh = ctypes.c_void_p()
        # stop inside a capture: the release waits for the end of the capture; the graph is never replayed
        bg = sim._budgetr.budget
        gid = dev.capture(lambda: (dev.budget_launch(bg, v, p), sim.stop_budget()))
        dev.free_graph(gid)
        assert sim._budgetr is None and bg._h is None
        with pytest.raises(_lib.FsError, match="freed"):
            _lib.call("fs_budget_read", dev._ctx, h, None, None, None)
        # a slab context (one of two ranks; no communicator is needed to ask): refused by the library with a message, and by the runtime
        slab = ctypes.c_void_p()
        _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
        try:
            assert create(slab, (0, 0, 64, 16)) == -5 and not hh.value    # FS_ERR_UNSUPPORTED
            assert "single-GPU" in dev._lib.fs_last_error().decode()
        finally:
            _lib.call("fs_destroy", slab)
        saved = dev.nranks
        dev.nranks = 2
        try:
            for call in (lambda: sim.start_budget(box), lambda: sim.budget_sample(box)):
                with pytest.raises(_lib.FsError, match="single-GPU"):
                    call()
        finally:
            dev.nranks = saved
    finally:
        _close(other)
        _close(sim)
