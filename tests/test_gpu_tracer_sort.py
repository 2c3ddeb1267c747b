"""The device sort of the tracer particles and the per-cell tracer fields on the GPU (csrc/fs_tracer.h k_tracer_sort_* / k_tracer_scan_* /
k_tracer_fields, include/fs_hip.h fs_tracer_sort / fs_tracer_order / fs_tracer_fields, FluidSimulator.seed_tracers(sort_every=K) /
sort_tracers / tracer_fields): the order contract, that sorting changes nothing any reader sees (against tests/tracers_ref.py, which knows
nothing of sorting, and against unsorted twin simulators on the golden trajectories), the graphs that stay valid, the fields against the
NumPy reference (tests/tracer_fields_ref.py), checkpoints across sorted and unsorted runs, the refusals.  Every comparison is
np.array_equal; nothing here looks at a time."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
from conftest import GOLDEN, REPO
from helpers import make_product, traj_config
from tracer_fields_ref import assert_order_contract, fields_ref
from tracers_ref import ALIVE, LEFT, WALL_HIT, advance_ref, assert_state_equal, new_state

pytestmark = pytest.mark.gpu

STATE = ("x", "y", "age", "status", "respawns", "seeds")


def _load(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    return g, traj_config(g)


def _close(sim):
    sim._solver._bc.device.close()


@pytest.fixture(autouse=True)
def _f32_default():
    import fs
    yield
    fs.runtime.init(gpu=0, dtype="f32")


def _same_state(a, b, what=""):
    for k in STATE:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}{k} differs"
    assert int(a["steps"]) == int(b["steps"]), what


def _random_scene(rng, X, Y):
    """The masks of tests/test_gpu_tracers.py test_random_fields_and_masks."""
    mask = (rng.random((X, Y)) < 0.12).astype(np.uint8)
    mask[rng.random((X, Y)) < 0.03] = 2
    mask[rng.random((X, Y)) < 0.03] = 3
    i, j = rng.integers(0, X - 6), rng.integers(0, Y - 6)
    mask[i:i + 6, j:j + 6] = 1
    return mask


# (X, Y, dtype, N, respawn, max_age): the grids of test_random_fields_and_masks; N no multiple of 256, N = 1, both respawn settings
DEVICE_CASES = [(101, 51, "f32", 1000, True, 0), (67, 33, "f64", 257, False, 9), (250, 125, "f32", 5000, False, 0), (1026, 37, "f64", 255, True, 7),
                (101, 51, "f32", 1, True, 0), (67, 33, "f64", 1, False, 0), (4, 4, "f32", 3, True, 0)]


def _device_case(X, Y, dtype, n):
    from fs.runtime import Device
    from fs.tracers import seed_random
    rng = np.random.default_rng(X * 1000 + Y)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = _random_scene(rng, X, Y) if X > 8 else np.zeros((X, Y), np.uint8)
    seeds = seed_random(mask, n, 5)
    dev = Device(X, Y, dtype)
    dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
    return dev, rng, dt_, mask, seeds


# ---- 1. the order contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X,Y,dtype,n,respawn,max_age", DEVICE_CASES)
def test_order_contract(X, Y, dtype, n, respawn, max_age, hip_lib):
    dev, rng, dt_, mask, seeds = _device_case(X, Y, dtype, n)
    try:
        vf = dev.alloc(2)
        v = (rng.standard_normal((X, Y, 2)) * 1.5).astype(dt_)
        vf.from_numpy(v)
        tr = dev.tracer_create(seeds, respawn=respawn, max_age=max_age)
        assert np.array_equal(dev.tracer_order(tr), np.arange(n, dtype=np.int32)), "id is not the identity at creation"
        for _ in range(6):
            dev.tracer_advance(tr, 0.4, vf)
        if respawn and n > 4:
            st = dev.tracer_read(tr)                          # a respawning set has no dead particles of its own: write some
            st["status"][::5] = LEFT
            st["status"][1::7] = WALL_HIT
            dev.tracer_write(tr, st)
        before = dev.tracer_read(tr)
        if n > 4:
            dead = before["status"] != ALIVE
            assert dead.any() and not dead.all(), "the case has no dead particles (or only dead ones)"
        for round_ in range(2):                               # the second sort starts from sorted slots
            dev.tracer_sort(tr)
            ids = dev.tracer_order(tr)
            assert ids.dtype == np.int32 and np.array_equal(np.sort(ids), np.arange(n)), "tracer_order is no permutation of arange(N)"
            raw = dev.tracer_read(tr, raw=True)
            assert np.array_equal(raw["id"], ids)
            assert_order_contract(raw, X, Y)
            for k in ("x", "y", "age", "status", "respawns"):
                assert np.array_equal(raw[k], before[k][ids], equal_nan=True), f"slot order: {k}"
            _same_state(dev.tracer_read(tr), before, f"after sort {round_}: ")
        if n >= 255:
            assert not np.array_equal(dev.tracer_order(tr), np.arange(n)), "the sort moved nothing: the case does not cover it"
        # a written state may hold anything: NaN and outside positions of alive particles go last as well
        if n > 4:
            st = dev.tracer_read(tr)
            st["status"][:] = ALIVE
            st["x"][0], st["y"][1], st["x"][2], st["y"][3] = np.nan, np.nan, -3.0, float(Y)
            dev.tracer_write(tr, st)
            assert np.array_equal(dev.tracer_order(tr), np.arange(n)), "tracer_write did not reset id to the identity"
            dev.tracer_sort(tr)
            raw = dev.tracer_read(tr, raw=True)
            assert_order_contract(raw, X, Y)
            assert sorted(raw["id"][-4:].tolist()) == [0, 1, 2, 3]
            _same_state(dev.tracer_read(tr), st, "NaN / outside: ")
        dev.tracer_free(tr)
    finally:
        dev.close()


# ---- 2. sorting changes nothing observable ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X,Y,dtype,n,respawn,max_age", DEVICE_CASES)
def test_advance_with_a_sort_after_every_launch_equals_the_reference(X, Y, dtype, n, respawn, max_age, hip_lib):
    dev, rng, dt_, mask, seeds = _device_case(X, Y, dtype, n)
    try:
        vf = dev.alloc(2)
        tr = dev.tracer_create(seeds, respawn=respawn, max_age=max_age)
        exp = new_state(seeds)
        for k in range(40):
            if k % 10 == 0:
                v = (rng.standard_normal((X, Y, 2)) * 1.5).astype(dt_)
                vf.from_numpy(v)
            dev.tracer_advance(tr, 0.4, vf)
            advance_ref(exp, v, mask, 0.4, respawn, max_age)
            dev.tracer_sort(tr)
            assert_state_equal(dev.tracer_read(tr), exp, f"launch {k}: ")
        if n >= 255:
            assert not np.array_equal(dev.tracer_order(tr), np.arange(n))
            if respawn:
                assert exp["respawns"].any(), "no particle respawned: the seed lookup through id is not covered"
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sorted_advance_under_a_deferred_limit(dtype, hip_lib):
    """The deferred-limit instantiations of the advance (tests/test_gpu_tracers.py test_deferred_limit_reaches_the_corners) with a sort
    after every launch."""
    from fs.runtime import Device
    from fs.tracers import seed_random
    X, Y = 130, 65
    rng = np.random.default_rng(17)
    dt_ = np.float32 if dtype == "f32" else np.float64
    mask = np.zeros((X, Y), np.uint8)
    mask[0, :] = mask[:, 0] = mask[:, -1] = 1
    mask[-1, :] = 3
    seeds = seed_random(mask, 700, 2)
    v = (rng.standard_normal((X, Y, 2)) * 9.0).astype(dt_)
    dev = Device(X, Y, dtype)
    try:
        dev.upload_scene(mask, np.zeros((X, Y, 2), dt_))
        vf = dev.alloc(2)
        vf.from_numpy(v)
        dev.limit_field(10.0, vf, defer=True)
        assert vf.pending_limit == 10.0, "the limit pass was not deferred: the test does not cover it"
        tr = dev.tracer_create(seeds, respawn=True)
        exp, unlimited = new_state(seeds), new_state(seeds)
        for k in range(40):
            dev.tracer_advance(tr, 0.05, vf)
            advance_ref(exp, v, mask, 0.05, limit=10.0)
            advance_ref(unlimited, v, mask, 0.05)
            dev.tracer_sort(tr)
            assert_state_equal(dev.tracer_read(tr), exp, f"launch {k}: ")
        assert vf.pending_limit == 10.0                       # (neither the advance nor the sort launches the owed pass)
        assert exp["respawns"].any() and not np.array_equal(exp["x"], unlimited["x"])
        assert not np.array_equal(dev.tracer_order(tr), np.arange(len(seeds)))
    finally:
        dev.close()


# ---- 3. twin simulators on the golden trajectories ----------------------------------------------------------------------------------------
CASES = ["traj_bc5_cip_vc5.npz", "traj_bc1_upwind_jacobi4_vc0.npz", "traj_dye_bc2_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"]      # (those of tests/test_gpu_tracers.py)


def _seeds(mask):
    from fs.tracers import fluid_only, seed_line, seed_random
    X, Y = mask.shape
    line, _ = fluid_only(mask, seed_line((1.5, 0.25), (1.5, Y - 0.25), 2 * Y))      # across the inflow side
    assert len(line) >= 8
    return np.concatenate([seed_random(mask, 500, 1), line])


def _drive(sims, compare):
    """A mix of step() and run(n, graph=True); compare() after every leg."""
    for leg in (("step", 3), ("run", 20), ("step", 2), ("run", 45), ("run", 5), ("step", 1), ("run", 33)):
        for sim in sims:
            if leg[0] == "step":
                for _ in range(leg[1]):
                    sim.step()
            else:
                sim.run(leg[1], graph=True)
        compare(leg)


@pytest.mark.parametrize("k_small,respawn", [(1, True), (7, False)])
@pytest.mark.parametrize("fname", CASES)
def test_twin_simulators_agree_whatever_the_sort_interval(fname, k_small, respawn, hip_lib):
    """Three simulators per case: sort_every = 0, 1 or 7, and 32."""
    import fs
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    sims = [make_product(g, cfg) for _ in range(3)]
    try:
        seeds = _seeds(g["bc_mask"])
        max_age = 25 if respawn else 60
        for sim, every in zip(sims, (0, k_small, 32)):
            sim.seed_tracers(seeds, respawn=respawn, max_age=max_age, sort_every=every)
        total = [0]

        def compare(leg):
            total[0] += leg[1]
            ref = sims[0].tracers()
            assert ref["steps"] == total[0]
            fields = [s.field_to_numpy() for s in sims]
            images = []
            for s in sims:
                s.get_norm_field()
                images.append(s.draw_tracers(color=(1.0, 0.25, 0.0)).to_numpy())
            for s, f, img in zip(sims[1:], fields[1:], images[1:]):
                what = f"{leg} at step {total[0]}, sort_every={s._tracers.sort_every}: "
                _same_state(s.tracers(), ref, what)
                for k in fields[0]:
                    assert np.array_equal(f[k], fields[0][k], equal_nan=True), what + k
                assert np.array_equal(img, images[0]), what + "draw_tracers image"
        _drive(sims, compare)
        assert total[0] == 109
        assert [s._tracers.sorts for s in sims] == [0, 109 // k_small, 109 // 32]
        assert not np.array_equal(sims[1]._dev.tracer_order(sims[1]._tracers.set), np.arange(len(seeds)))
        assert sims[2]._graphs, "the runs replayed no graph"
        got = sims[0].tracers()
        assert np.hypot(got["x"] - seeds[:, 0], got["y"] - seeds[:, 1]).max() > 0.25, "no particle moved"      # (max_age bounds the way)
        assert got["respawns"].any() if respawn else (got["status"] != ALIVE).any()
    finally:
        for s in sims:
            _close(s)


# ---- 4. graphs ----------------------------------------------------------------------------------------------------------------------------
def test_graphs_hold_the_launches_they_held_and_survive_a_sort(hip_lib):
    """sort_every=32 and run(200, graph=True).  The launch profile counts what is launched outside graphs, a replayed graph's launches are
    not in it: the number of advance launches is therefore taken from the counter the advance kernel itself keeps on the device (one per
    launch, replayed or not: "steps"), and from the profile in an eager run of the same 200 steps; the sorts are always launched outside
    graphs, so the profile counts all of them."""
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    a, b, c, d = (make_product(g, cfg) for _ in range(4))
    try:
        seeds = _seeds(g["bc_mask"])
        a.seed_tracers(seeds, sort_every=32)
        b.seed_tracers(seeds)
        c.seed_tracers(seeds, sort_every=32)
        a._dev.profile(True)
        a.run(200, graph=True)
        rep = a._dev.profile_report()
        a._dev.profile(False)
        assert a.tracers()["steps"] == 200, "not one advance launch per step"
        sort_names = sorted(k for k in rep if k.startswith("tracer_sort"))
        assert sort_names == ["tracer_sort_copy", "tracer_sort_count", "tracer_sort_scan", "tracer_sort_scatter"], sort_names
        assert all(rep[k][0] == 200 // 32 for k in sort_names), {k: rep[k][0] for k in sort_names}
        assert a._tracers.sorts == 200 // 32
        assert any("k_tracer_sort_scatter" in k for k in a._dev.profile_kernels("tracer_sort_scatter"))
        assert rep["tracer_advance"][0] < 200 and a._graphs, "nothing was replayed from a graph"
        # the unsorted twin in one uncut run(200): the chunks the sort schedule cuts find their way back to the cached graph's phase by
        # eager steps and pick up the long form once a chunk has room for it, so nothing more is cached
        b.run(200, graph=True)
        assert b._graphs and len(a._graphs) <= len(b._graphs), (len(a._graphs), len(b._graphs))
        assert sorted(e[1] for e in a._graphs.values()) == sorted(e[1] for e in b._graphs.values())
        assert [e[2] is not None and e[2][1] for e in a._graphs.values()] == [e[2] is not None and e[2][1] for e in b._graphs.values()]
        _same_state(a.tracers(), b.tracers(), "graph run: ")
        fa, fb = a.field_to_numpy(), b.field_to_numpy()
        assert all(np.array_equal(fa[k], fb[k]) for k in fa)
        # eagerly: the profile holds every launch
        c._dev.profile(True)
        c.run(200, graph=False)
        rep = c._dev.profile_report()
        c._dev.profile(False)
        assert rep["tracer_advance"][0] == 200 and rep["tracer_sort_count"][0] == 200 // 32, (rep["tracer_advance"], rep["tracer_sort_count"])
        _same_state(c.tracers(), a.tracers(), "eager run: ")
        # a graph captured before the first sort replays to the right state after one
        d.seed_tracers(seeds)
        d.run(40, graph=True)
        assert d._graphs and d._tracers.sorts == 0
        cached = dict(d._graphs)
        d.sort_tracers()
        assert not np.array_equal(d._dev.tracer_order(d._tracers.set), np.arange(len(seeds)))
        d.run(60, graph=True)
        assert all(d._graphs.get(k) == e for k, e in cached.items()), "a sort invalidated a cached graph"
        d.sort_tracers()
        d.run(100, graph=True)
        _same_state(d.tracers(), a.tracers(), "captured before the first sort: ")
    finally:
        for s in (a, b, c, d):
            _close(s)


# ---- 5. fields ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["traj_bc5_cip_vc5.npz", "traj_f64_bc1_cip_vc0.npz"])
def test_tracer_fields_equal_the_numpy_reference(fname, hip_lib):
    import fs
    from fs.tracers import residence_map
    g, cfg = _load(fname)
    fs.runtime.init(gpu=0, dtype="f64" if cfg["fp64"] else "f32")
    sim = make_product(g, cfg)
    try:
        mask = g["bc_mask"]
        X, Y = mask.shape
        sim.seed_tracers(np.concatenate([_seeds(mask)] * 3), respawn=False)      # (every seed three times: cells with several particles)
        sim.run(40, graph=True)
        st = sim.tracers()
        st["status"][::4] = LEFT                                  # a quarter of the particles dead, whatever the flow did
        sim._dev.tracer_write(sim._tracers.set, st)
        dead = st["status"] != ALIVE
        assert dead.any() and not dead.all(), "no dead particles: their exclusion is not covered"
        count, age_sum = fields_ref(st, X, Y)
        assert count.max() >= 2 and count.sum() == int((~dead).sum())
        for sort in (False, True, True):
            if sort:
                sim.sort_tracers()
            f = sim.tracer_fields()
            assert set(f) == {"count", "age_sum", "steps"} and f["steps"] == 40
            assert f["count"].dtype == np.int32 and f["age_sum"].dtype == np.int64 and f["count"].shape == f["age_sum"].shape == (X, Y)
            assert np.array_equal(f["count"], count) and np.array_equal(f["age_sum"], age_sum), f"sorted: {sort}"
            again = sim.tracer_fields()
            assert np.array_equal(again["count"], f["count"]) and np.array_equal(again["age_sum"], f["age_sum"])
        r = residence_map(f["count"], f["age_sum"], cfg["dt"])
        assert np.array_equal(np.isnan(r), count == 0) and np.nanmax(r) == 40 * cfg["dt"]
        # 64-bit sums: three particles of age 2^30 in one cell
        cell = np.argwhere(mask == 0)[0]
        st["x"][:3], st["y"][:3], st["age"][:3], st["status"][:3] = cell[0] + 0.5, cell[1] + 0.25, 2 ** 30, ALIVE
        st["x"][3], st["y"][3], st["status"][3] = cell[0] + 0.5, cell[1] + 0.25, LEFT           # a dead one in the same cell
        sim._dev.tracer_write(sim._tracers.set, st)
        count, age_sum = fields_ref(st, X, Y)
        for sort in (False, True):
            if sort:
                sim.sort_tracers()
            f = sim.tracer_fields()
            assert np.array_equal(f["count"], count) and np.array_equal(f["age_sum"], age_sum)
            assert f["age_sum"][cell[0], cell[1]] >= 3 * 2 ** 30 > np.iinfo(np.int32).max
        _same_state(sim.tracers(), st, "the fields moved something: ")
    finally:
        _close(sim)


# ---- 6. checkpoints -----------------------------------------------------------------------------------------------------------------------
def _copy_fields(src, dst):
    s, c = src._solver, dst._solver
    for name in ("v", "p", "vx", "vy"):
        getattr(c, name).current.from_numpy(getattr(s, name).current.to_numpy())
        getattr(c, name).next.from_numpy(getattr(s, name).next.to_numpy())
    c.vorticity_confinement.vorticity.from_numpy(s.vorticity_confinement.vorticity.to_numpy())
    c.vorticity_confinement.vorticity_abs.from_numpy(s.vorticity_confinement.vorticity_abs.to_numpy())


def test_checkpoint_from_a_sorted_run_continues_sorted_and_unsorted(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sims = []
    try:
        seeds = _seeds(g["bc_mask"])
        a = make_product(g, cfg)                                 # uninterrupted, unsorted
        sims.append(a)
        a.seed_tracers(seeds, respawn=True, max_age=35)
        a.run(50, graph=True)
        b = make_product(g, cfg)                                 # sorted, stopped at step 23
        sims.append(b)
        b.seed_tracers(seeds, respawn=True, max_age=35, sort_every=5)
        b.run(23, graph=True)
        assert b._tracers.sorts == 4
        state = b._dev.tracer_read(b._tracers.set)
        assert state["steps"] == 23 and np.array_equal(state["seeds"], seeds)
        ra = a.tracers()
        fa = a.field_to_numpy()
        for every in (7, 0):
            c = make_product(g, cfg)
            sims.append(c)
            _copy_fields(b, c)
            c.seed_tracers(seeds[::-1], respawn=True, max_age=35, sort_every=every)      # (other seeds: the write restores them too)
            c.sort_tracers()                                                            # ... onto slots that are permuted already
            c._dev.tracer_write(c._tracers.set, state)
            assert np.array_equal(c._dev.tracer_order(c._tracers.set), np.arange(len(seeds)))
            assert_state_equal(c.tracers(), state, "written ")
            c.run(27, graph=True)
            assert c._tracers.sorts == 1 + (27 // every if every else 0)
            rc = c.tracers()
            assert rc["steps"] == 50
            _same_state(rc, ra, f"resumed with sort_every={every}: ")
            fc = c.field_to_numpy()
            assert all(np.array_equal(fa[k], fc[k]) for k in fa)
        assert ra["respawns"].min() >= 1
    finally:
        for s in sims:
            _close(s)


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_tracer_sort_gpu", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("graph", [False, True])
def test_cli_round_trip_with_sorting_and_fields(graph, tmp_path, hip_lib):
    from fs.tracers import residence_map
    cli = _cli()
    res = 64
    X, Y = 2 * res, res                                          # (the scenes are two squares wide)
    dt = 0.05 / res                                              # (main.py's time step without -dt)
    common = ["-bc", "5", "-res", str(res), "--tracers", "900", "--tracer-seed", "9", "--tracer-max-age", "15"] + (["--graph"] if graph else [])
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    cli.main(common + ["--steps", "40", "--out", str(a), "--tracer-sort-every", "16", "--tracer-fields", "--tracer-dump-every", "20"])
    cli.main(common + ["--steps", "40", "--out", str(b)])                               # the same run, unsorted, without fields
    t, u = np.load(a / "tracers.npz"), np.load(b / "tracers.npz")
    for k in u.files:
        assert np.array_equal(t[k], u[k]), f"{k}: --tracer-sort-every changed the particles"
    assert not (b / "tracer_fields.npz").exists()
    for path, dump, step in ((a / "tracer_fields.npz", t, 40), (a / "tracer_fields_000020.npz", np.load(a / "tracers_000020.npz"), 20),
                             (a / "tracer_fields_000040.npz", t, 40)):
        f = np.load(path)
        assert sorted(f.files) == ["age_sum", "count", "residence", "step"] and int(f["step"]) == step
        assert f["count"].shape == (X, Y)
        count, age_sum = fields_ref({k: dump[k] for k in ("x", "y", "age", "status")}, X, Y)
        assert np.array_equal(f["count"], count) and np.array_equal(f["age_sum"], age_sum), path
        assert count.sum() == 900 and age_sum.max() > 0
        r = f["residence"]
        assert r.dtype == np.float64 and np.array_equal(np.isnan(r), count == 0)
        assert np.array_equal(r, residence_map(count, age_sum, dt), equal_nan=True)
    # over a restart: saved by the sorted run, continued unsorted, and the reverse; --tracer-fields-file moves the file
    c.mkdir()
    cli.main(common + ["--steps", "17", "--out", str(c), "--tracer-sort-every", "16", "--save-state", str(c / "ck.npz")])
    cli.main(common + ["--steps", "23", "--out", str(c), "--load-state", str(c / "ck.npz"), "--tracer-fields", "--tracer-fields-file", str(c / "f.npz")])
    r1 = np.load(c / "tracers.npz")
    assert (c / "f.npz").exists() and not (c / "tracer_fields.npz").exists()
    cli.main(common + ["--steps", "17", "--out", str(c), "--save-state", str(c / "ck2.npz")])
    cli.main(common + ["--steps", "23", "--out", str(c), "--load-state", str(c / "ck2.npz"), "--tracer-sort-every", "16"])
    r2 = np.load(c / "tracers.npz")
    for k in u.files:
        assert np.array_equal(r1[k], u[k]) and np.array_equal(r2[k], u[k]), f"{k}: the resumed particles differ from the uninterrupted run's"
    assert sorted(np.load(c / "ck.npz").files) == sorted(np.load(c / "ck2.npz").files)      # the checkpoint format does not know of sorting
    f = np.load(c / "f.npz")
    count, age_sum = fields_ref({k: r1[k] for k in ("x", "y", "age", "status")}, X, Y)
    assert np.array_equal(f["count"], count) and np.array_equal(f["age_sum"], age_sum) and int(f["step"]) == 40


# ---- 7. rules -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_capture_rules(hip_lib):
    import fs
    from fs import _lib
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    sim, other = make_product(g, cfg), make_product(g, cfg)
    dev = sim._dev
    mask = g["bc_mask"]
    X, Y = mask.shape
    try:
        for call in (sim.sort_tracers, sim.tracer_fields):
            with pytest.raises(RuntimeError):
                call()                                           # no set attached
        with pytest.raises(ValueError):
            sim.seed_tracers(_seeds(mask), sort_every=-1)
        assert sim._tracers is None
        sim.seed_tracers(_seeds(mask), sort_every=0)
        other.seed_tracers(_seeds(mask))
        sim.run(20, graph=True)
        before = sim.tracers()
        tr = sim._tracers.set
        h = tr._h
        n = tr.n
        for call in (sim.sort_tracers, sim.tracer_fields):
            with pytest.raises(RuntimeError):
                dev.capture(call)
        for call in (dev.tracer_sort, dev.tracer_order, dev.tracer_fields):
            with pytest.raises(_lib.FsError):
                dev.capture(lambda: call(tr))
        # the library refuses on its own as well (FS_ERR_STATE = -3) and leaves the capture usable
        ids = np.empty(n, np.int32)
        count, age = np.empty((Y, X), np.int32), np.empty((Y, X), np.int64)
        v = sim._solver.get_fields()[0]
        _lib.call("fs_graph_begin", dev._ctx)
        try:
            st = [dev._lib.fs_tracer_sort(dev._ctx, h),
                  dev._lib.fs_tracer_order(dev._ctx, h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
                  dev._lib.fs_tracer_fields(dev._ctx, h, count.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                            age.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))]
            _lib.call("fs_tracer_advance", dev._ctx, h, 0.0, 0.0, v._h)          # (h = 0: a launch that moves nothing but counts)
        finally:
            gid = ctypes.c_int(-1)
            _lib.call("fs_graph_end", dev._ctx, ctypes.byref(gid))
        assert st == [-3, -3, -3] and gid.value >= 0
        dev.replay(gid.value, 2)                                  # the capture held the advance launch and nothing else
        dev.free_graph(gid.value)
        after = sim.tracers()
        assert after["steps"] == 22 and np.array_equal(after["x"], before["x"]) and np.array_equal(after["age"], before["age"] + 2)
        assert np.array_equal(dev.tracer_order(tr), np.arange(n)), "a refused sort moved something"
        # handles of another context (FS_ERR_ARG = -1), null arguments
        oh = other._tracers.set._h
        st = [dev._lib.fs_tracer_sort(dev._ctx, oh),
              dev._lib.fs_tracer_order(dev._ctx, oh, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
              dev._lib.fs_tracer_fields(dev._ctx, oh, count.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), age.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))),
              dev._lib.fs_tracer_order(dev._ctx, h, None), dev._lib.fs_tracer_fields(dev._ctx, h, None, None), dev._lib.fs_tracer_sort(dev._ctx, None)]
        assert st == [-1] * 6, st
        for call in (dev.tracer_sort, dev.tracer_order, dev.tracer_fields):
            with pytest.raises(_lib.FsError):
                call(other._tracers.set)
        # the profile names: a sort is not an advance
        dev.profile(True)
        sim.step()
        sim.sort_tracers()
        sim.tracer_fields()
        rep = dev.profile_report()
        dev.profile(False)
        assert rep["tracer_advance"][0] == 1 and rep["tracer_sort_count"][0] == 1 and rep["tracer_fields"][0] == 1
        assert any("k_tracer_fields" in k for k in dev.profile_kernels("tracer_fields"))
        assert [k for k in dev.profile_kernels("tracer_sort_scan")] and all("k_tracer_scan" in k for k in dev.profile_kernels("tracer_sort_scan"))
    finally:
        _close(sim)
        _close(other)


def test_run_after_stop_equals_a_run_that_never_had_tracers(hip_lib):
    import fs
    g, cfg = _load("traj_bc5_cip_vc5.npz")
    fs.runtime.init(gpu=0, dtype="f32")
    reports, fields = {}, {}
    for traced in (False, True):
        sim = make_product(g, cfg)
        dev = sim._dev
        try:
            if traced:
                sim.seed_tracers(_seeds(g["bc_mask"]), sort_every=16)
            sim.run(40, graph=True)
            sim.step()
            if traced:
                assert sim._tracers.sorts == 2 and sim.tracer_fields()["count"].sum() > 0
                sim.stop_tracers()
                for call in (sim.sort_tracers, sim.tracer_fields):
                    with pytest.raises(RuntimeError):
                        call()
                assert not [k for k in sim._graphs if any(isinstance(t, tuple) and t and t[0] == "tracer" for t in k)]
            dev.profile(True)
            sim.run(12, graph=False)
            reports[traced] = {k: v[0] for k, v in dev.profile_report().items()}
            dev.profile(False)
            sim.run(25, graph=True)
            fields[traced] = sim.field_to_numpy()
        finally:
            _close(sim)
    assert reports[True] == reports[False], (reports[True], reports[False])
    assert not [k for k in reports[True] if "tracer" in k]
    for k in fields[False]:
        assert np.array_equal(fields[True][k], fields[False][k]), k


def test_slab_contexts_still_refuse(hip_lib):
    from fs import _lib
    from fs.runtime import Device, DeviceBase
    dev = Device(64, 32, "f32", gpu=0, rank=0, nranks=1)
    slab = ctypes.c_void_p()
    _lib.call("fs_create", ctypes.byref(slab), 0, 64, 32, 0, 0, 16, 4)
    try:
        one = (ctypes.c_double * 2)(3.5, 3.5)
        assert dev._lib.fs_tracer_create(slab, 1, one, 1, 0, ctypes.byref(ctypes.c_void_p())) == -5      # FS_ERR_UNSUPPORTED
        tr = dev.tracer_create(np.array([[3.5, 3.5]]))
        assert dev._lib.fs_tracer_sort(slab, tr._h) == -1        # (a set of the other context: no set can exist on a slab)
        dev.tracer_sort(tr)
        assert dev.tracer_order(tr).tolist() == [0]
    finally:
        _lib.call("fs_destroy", slab)
        dev.close()

    class _Slab:
        nranks, capturing = 2, False

    class _Set:
        _h, n = None, 1
    for call in (DeviceBase.tracer_sort, DeviceBase.tracer_order, DeviceBase.tracer_fields):
        with pytest.raises(_lib.FsError):
            call(_Slab(), _Set())

    import fs

    class _Sim:
        _tracers = None
    sim = _Sim()
    sim._dev = _Slab()
    sim._solver = None
    with pytest.raises(_lib.FsError):
        fs.FluidSimulator.seed_tracers(sim, np.array([[1.5, 1.5]]), sort_every=8)
