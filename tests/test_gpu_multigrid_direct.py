"""The multigrid updater with coarsest="direct" on the GPU (csrc/fs_mg.h k_mg_direct; include/fs_hip.h fs_mg_set_direct) against its NumPy
restatement (tests/multigrid_direct_ref.py), bit for bit.  The restatement is fed with the product's own upload
(MultigridPressureUpdater.direct_matrix()): the comparison is about the ordered product and the cycle around it, not about two LAPACK calls.

Cases (grid, wall density, direct_cells -> direct level, its shape, active cells), chosen for the kernel's edges - a row per wave, four rows per
workgroup, columns in blocks of 64:
    (8, 8)      0.5   default   1  4 x 4     11     n < 64: one partial column block, fewer rows than a workgroup holds
    (36, 20)    0     100       2  9 x 5     45     n < 64 under a global level
    (36, 20)    0     16        2  9 x 5     45     no level is that small: the last one
    (64, 8)     0     128       1  32 x 4    128    n a multiple of 64 and of the rows per workgroup
    (128, 16)   0.15  128       2  32 x 4    128    one global level above
    (36, 20)    0.3   180       1  18 x 10   160    three components without a Dirichlet coupling (pseudo-inverse); n no multiple of 64
    (96, 64)    0.3   100       3  12 x 8    96     two global levels above: four direct launches per cycle
    (96, 64)    0.3   default   1  48 x 32   1499   a single-level hierarchy, many workgroups
    (1024, 8)   0.3   default   1  512 x 4   1966   near the default cap, 82 inactive cells, 13 unanchored components
    (128, 128)  0.05  4096      1  64 x 64   4089   the size limit (f32)
    scenes 1, 5 res 100         2  50 x 25   1249 / 916     the resolutions the option is for (f32)"""
import ctypes

import numpy as np
import pytest

import multigrid_cases as C
import multigrid_direct_ref as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RE = 1000.0
CASES = [((8, 8), 0.5, None, 1, (4, 4), 11), ((36, 20), 0.0, 100, 2, (9, 5), 45), ((36, 20), 0.0, 16, 2, (9, 5), 45),
         ((64, 8), 0.0, 128, 1, (32, 4), 128), ((128, 16), 0.15, 128, 2, (32, 4), 128), ((36, 20), 0.3, 180, 1, (18, 10), 160),
         ((96, 64), 0.3, 100, 3, (12, 8), 96), ((96, 64), 0.3, None, 1, (48, 32), 1499), ((1024, 8), 0.3, None, 1, (512, 4), 1966)]


def launches(n):
    """Of one cycle on n levels: residual + correction; 3 x 2 sweeps = 12 half sweeps per visit of a global level (level k: 2^(k-1) visits);
    one direct launch per visit of the last; restriction + prolongation per coarse visit."""
    return 2 + 12 * (2 ** (n - 1) - 1) + 2 ** (n - 1) + 2 * (2 ** n - 2)


def check_update(const, mask, dtype, pc, pn, v, dt, dx, direct_cells, level, shape, cells):
    import fs
    from fs.multigrid import direct_solve
    dtype = np.dtype(dtype)
    kw = {} if direct_cells is None else dict(direct_cells=direct_cells)
    fs.runtime.init(gpu=0, dtype="f64" if dtype == np.float64 else "f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        pu = fs.MultigridPressureUpdater(bc, dt, dx, coarsest="direct", **kw)
        solver = fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, RE, None)
        solver.v.current.from_numpy(v)
        solver.p.current.from_numpy(pc)
        solver.p.next.from_numpy(pn)
        pu.update(solver.p, solver.v.current)
        got = (solver.p.current.to_numpy(), solver.p.next.to_numpy())
        info, levels = pu.info(), pu.levels
        cells_up, Minv = pu.direct_matrix()
    finally:
        bc.device.close()
    print(f"{mask.shape} {dtype.name} direct_cells={direct_cells}: {info}")
    assert info["tail_level"] == 0 and info["levels"] == len(levels) == level == info["direct_level"]
    assert levels[-1] == shape and info["direct_cells"] == cells == len(cells_up)
    assert info["launches"] == launches(level)
    assert cells_up.dtype == np.int32 and Minv.dtype == dtype and Minv.shape == (cells, cells)
    ref = D.MultigridDirectRef(O.OracleBC(const, mask, None, dtype), dt, dx, level, cells_up, Minv)      # (asserts the cells are the level's active ones)
    # the upload is the host inverse rounded to the field dtype: two float64 LAPACK runs differ by eps64 x condition (< 1e-11 of the largest
    # entry), the rounding by 2^-24 of an entry
    lv = ref.levels[-1]
    host = direct_solve(lv.cx, lv.cy, lv.diag)[1]
    assert float(np.abs(Minv - host).max()) <= 1e-6 * float(np.abs(host).max())
    p = O.Buf2(pc.shape, 1, dtype)
    p.current[...], p.next[...] = pc, pn
    ref.update(p, v.copy())
    assert np.isfinite(p.current).all() and np.isfinite(p.next).all() and not np.array_equal(p.current, pc)
    for name, a, e in zip(("p.current", "p.next"), got, (p.current, p.next)):
        assert a.dtype == e.dtype == dtype
        assert np.array_equal(a, e), f"{mask.shape} {dtype.name} direct_cells {direct_cells} {name}: {int((a != e).sum())} cells differ, max {np.abs(a - e).max():.3e}"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("grid,wall_p,direct_cells,level,shape,cells", CASES,
                         ids=[f"{g[0]}x{g[1]}-w{w}-cells{'default' if d is None else d}" for g, w, d, *_ in CASES])
def test_one_update_on_random_masks(grid, wall_p, direct_cells, level, shape, cells, dtype, hip_lib):
    const, mask = C.scene(*grid, wall_p)
    check_update(const, mask, dtype, *C.fields(*grid, wall_p, dtype), C.DT, C.DX, direct_cells, level, shape, cells)


def test_one_update_at_the_size_limit(hip_lib):
    const, mask = C.scene(128, 128, 0.05)
    check_update(const, mask, "float32", *C.fields(128, 128, 0.05, "float32"), C.DT, C.DX, 4096, 1, (64, 64), 4089)


@pytest.mark.parametrize("num,cells", [(1, 1249), (5, 916)])
def test_one_update_on_the_scenes_at_res_100(num, cells, hip_lib):
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(num, 100)
    check_update(const, mask, "float32", *C.fields(200, 100, 0.0, "float32"), 0.05 / 100, 1.0 / 100, None, 2, (50, 25), cells)


def test_the_default_has_no_direct_level_and_bad_options_are_refused(hip_lib):
    import fs
    const, mask = C.scene(36, 20, 0.0)
    fs.runtime.init(gpu=0, dtype="f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        pu = fs.MultigridPressureUpdater(bc, C.DT, C.DX)
        info = pu.info()
        assert info["direct_level"] == 0 and info["direct_cells"] == 0 and info["levels"] == 2
        with pytest.raises(ValueError, match="direct_matrix"):
            pu.direct_matrix()
        with pytest.raises(ValueError, match="coarsest"):
            fs.MultigridPressureUpdater(bc, C.DT, C.DX, coarsest="lu")
        with pytest.raises(ValueError, match="direct_cells"):
            fs.MultigridPressureUpdater(bc, C.DT, C.DX, coarsest="direct", direct_cells=0)
    finally:
        bc.device.close()
    # a last level beyond the size limit: (182, 98) ends on 91 x 49 with 4442 active cells
    const, mask = C.scene(182, 98, 0.0)
    fs.runtime.init(gpu=0, dtype="f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        with pytest.raises(ValueError, match=r"91 x 49.*4442"):
            fs.MultigridPressureUpdater(bc, C.DT, C.DX, coarsest="direct")
    finally:
        bc.device.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("grid,scheme,vc", [((72, 40), "upwind", None), ((260, 24), "kk", 10.0)])
def test_four_step_trajectories(grid, scheme, vc, dtype, hip_lib):
    """Four steps from a random v and p at Re 1000 on a random mask (wall density 0.15), the restatement as the oracle solver's pressure
    updater: every field after every step."""
    import fs
    wall_p = 0.15
    const, mask = C.scene(*grid, wall_p)
    pc, _, v = C.fields(*grid, wall_p, dtype)
    fs.runtime.init(gpu=0, dtype="f64" if dtype == "float64" else "f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        mg = fs.MultigridPressureUpdater(bc, C.DT, C.DX, coarsest="direct")
        fvc = fs.VorticityConfinement(bc, C.DT, C.DX, vc) if vc is not None else None
        solver = fs.MacSolver(bc, mg, fs.advect_upwind if scheme == "upwind" else fs.advect_kk_scheme, C.DT, C.DX, RE, fvc)
        obc = O.OracleBC(const, mask, None, np.dtype(dtype))
        pu = D.MultigridDirectRef(obc, C.DT, C.DX, mg.info()["direct_level"], *mg.direct_matrix())
        ovc = O.OracleVorticity(obc, C.DT, C.DX, vc) if vc is not None else None
        ref = O.OracleMacSolver(obc, pu, scheme, C.DT, C.DX, RE, ovc)
        solver.v.current.from_numpy(v)
        ref.v.current[...] = v
        solver.p.current.from_numpy(pc)
        ref.p.current[...] = pc
        for step in range(1, 5):
            solver.update()
            ref.update()
            got = [f.to_numpy() for f in solver.get_fields()]
            for a, (k, e) in zip(got, ref.fields().items()):
                assert np.isfinite(e).all(), f"the restatement's {k} is not finite at step {step}"
                assert a.dtype == e.dtype and np.array_equal(a, e), f"{grid} {scheme} {dtype} step {step} {k}: {int((a != e).sum())} cells differ"
        info = mg.info()
        assert info["direct_level"] == info["levels"] == 1 and info["launches"] == 3
    finally:
        bc.device.close()


def test_graph_replay_equals_eager_stepping(hip_lib):
    """30 steps of scene 5 at res 32 with the exact solve on level 2 (16 x 8): the captured period holds the direct launches."""
    from test_gpu_multigrid import make_sim
    n, kw = 30, dict(coarsest="direct", direct_cells=128)
    eager = make_sim(5, 32, "float32", vc=None, **kw)
    try:
        for _ in range(n):
            eager.step()
        exp = eager.field_to_numpy()
        info = eager._solver.pressure_updater.info()
    finally:
        eager._solver._bc.device.close()
    assert info["direct_level"] == 2 and info["tail_level"] == 0 and info["launches"] == launches(2)
    sim = make_sim(5, 32, "float32", vc=None, **kw)
    try:
        sim.run(n, graph=True)
        assert sim._graph is not None, "no period of the multigrid step was captured"
        out = sim.field_to_numpy()
    finally:
        sim._solver._bc.device.close()
    for k in exp:
        assert np.isfinite(exp[k]).all() and np.array_equal(out[k], exp[k]), k


def test_create_takes_the_updaters_keywords(hip_lib):
    import fs
    fs.runtime.init(gpu=0, dtype="f32")
    for spec, omega in ((("multigrid", 2, dict(coarsest="direct", direct_cells=128)), 1.3), (("multigrid", 1, 1.2, dict(coarsest="direct")), 1.2)):
        sim = fs.FluidSimulator.create(5, 32, 0.05 / 32, 1.0 / 32, RE, None, "upwind", pressure_updater=spec)
        try:
            pu = sim._solver.pressure_updater
            assert isinstance(pu, fs.MultigridPressureUpdater) and pu._n_cycles == spec[1] and pu._relaxation_factor == omega
            assert pu.info()["direct_level"] == (2 if "direct_cells" in spec[-1] else 1)
        finally:
            sim._solver._bc.device.close()


def test_set_direct_refusals(hip_lib):
    """Every refusal of fs_mg_set_direct returns its error and leaves the hierarchy as it was: still without a direct solve, still able to
    take a valid one and to run a cycle with it."""
    import fs
    from fs import _lib
    from fs._lib import FsError
    from fs.multigrid import build_hierarchy, direct_solve
    const, mask = C.scene(36, 20, 0.3)
    fs.runtime.init(gpu=0, dtype="f32")
    bc = fs.BoundaryCondition(const, mask)
    dev = bc.device
    try:
        levels = build_hierarchy(mask, np.float32)[:1]      # 18 x 10, 160 active cells
        cells, Minv = direct_solve(*levels[0])
        n = cells.size
        assert n == 160
        stride = 64 * ((n + 63) // 64)
        padded = np.zeros((n, stride), np.float32)
        padded[:, :n] = Minv
        h = dev.mg_create(levels, 0, 2, 64)
        tailed = dev.mg_create(levels, -1, 2, 64)
        assert dev.mg_info(tailed)["tail_level"] == 1

        def call(handle, n_, cells_, stride_, M=padded):
            c = np.ascontiguousarray(cells_, np.int32)
            _lib.call("fs_mg_set_direct", dev._ctx, handle, n_, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), M.ctypes.data_as(ctypes.c_void_p), stride_)

        big = np.arange(4097)
        beyond = cells.copy()
        beyond[-1] = 18 * 10
        swapped = cells.copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        for args, status, msg in (((h, 4097, big, 64 * 65), -1, "0 .. 4096"), ((h, -1, cells, 0), -1, "0 .. 4096"),
                                  ((h, n, cells[::-1], stride), -1, "strictly ascending"), ((h, n, swapped, stride), -1, "strictly ascending"),
                                  ((h, n, beyond, stride), -1, "of the last level"), ((h, n, cells, n), -1, "row_stride"),
                                  ((h, n, cells, stride + 64), -1, "row_stride"), ((tailed, n, cells, stride), -3, "without a tail kernel")):
            with pytest.raises(FsError, match=f"status {status}: .*{msg}"):
                call(*args)
            assert dev.mg_info(h)["direct_level"] == 0 and dev.mg_info(tailed)["direct_level"] == 0
        with pytest.raises(FsError, match="null argument"):
            _lib.call("fs_mg_set_direct", dev._ctx, h, n, None, padded.ctypes.data_as(ctypes.c_void_p), stride)
        p, q, v = dev.alloc(1), dev.alloc(1), dev.alloc(2)
        seen = []

        def body():
            dev.pressure_bc(p)
            with pytest.raises(FsError, match="status -3: multigrid set_direct during graph capture") as e:
                call(h, n, cells, stride)
            seen.append(e)
            dev.pressure_bc(p)

        gid = dev.capture(body)                                # the refusal left the capture intact
        assert seen
        dev.replay(gid)
        dev.free_graph(gid)
        assert dev.mg_info(h)["direct_level"] == 0
        call(h, n, cells, stride)                              # a valid call is accepted once ...
        assert dev.mg_info(h)["direct_level"] == 1 and dev.mg_info(h)["direct_cells"] == n
        with pytest.raises(FsError, match="status -3: .*already has a direct solve"):
            call(h, n, cells, stride)
        pc, pn, vv = C.fields(36, 20, 0.3, "float32")
        p.from_numpy(pc); q.from_numpy(pn); v.from_numpy(vv)
        dev.pressure_bc(p)
        dev.mg_cycle(h, C.DT, C.DX, p, q, v)                  # ... and the cycle runs on it
        out = p.to_numpy()
        assert np.isfinite(out).all() and not np.array_equal(out, pc) and dev.mg_info(h)["launches"] == 3
        dev.mg_free(h)
        dev.mg_free(tailed)
    finally:
        dev.close()
