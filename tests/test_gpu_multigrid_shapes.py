"""The multigrid kernels (csrc/fs_mg.h) where tests/test_gpu_multigrid.py does not take them: more than one block per row, the
launch-per-half-sweep form in both dtypes and on odd, one-row and coarsest levels, grids that are not 2:1 reference scenes, random masks with
inactive coarse cells, and degenerate sweep counts.  Product against the NumPy restatement (tests/multigrid_ref.py), bit for bit.

Grids (tests/multigrid_cases.py), each the smallest that reaches its form:
    (1088, 8)   544x4, 272x2, 136x1   FS_MG_TAIL=0: every kernel has blockIdx.x > 0 (fine_correct 5 blocks per row, fine_residual and prolong 3,
                                      restrict and halfsweep 2), the coarsest level has one row; default: one tail of 2856 cells (57 KB in f32,
                                      114 KB in f64: above the 48 KB from which fs_mg_create raises the kernel's LDS limit); 600: tail from level 2
    (1024, 8)   512x4, 256x2, 128x1   every width a whole number of blocks: no partial block hides a block that starts a lane early or late
    (2112, 4)   1056x2, 528x1         halfsweep on level 1: 528 lanes, 3 blocks; a launch-form coarsest level of 264 lanes in 2 blocks
    (260, 24)   130x12, 65x6          X no multiple of 64 (pitched fine fields, unpadded levels), odd-width coarsest level
    (96, 64)    48x32 ... 3x2         five levels; FS_MG_TAIL=100 splits at 12x8 (levels 1 - 2 as launches, 3 - 5 in the kernel)
    (36, 20)    18x10, 9x5            coarsest level odd in both extents
    (24, 96)    12x48, 6x24, 3x12     taller than wide, odd width 3
    (44, 6)     22x3                  one level: the tail kernel leaves at its first level; with tail 0 the coarsest sweeps run on level 1
    (8, 8)      4x4, 2x2, 1x1         a 1x1 level (half == 1)
FS_MG_TAIL is read by the updater's constructor, so setting it before construction is enough; info()["tail_level"] proves it took effect."""
import functools

import numpy as np
import pytest

import multigrid_cases as C
import multigrid_ref as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RE = 1000.0
GRIDS = [(1088, 8), (1024, 8), (2112, 4), (260, 24), (96, 64), (36, 20), (24, 96), (44, 6), (8, 8)]
SPLIT = {(1088, 8): 600, (96, 64): 100}      # an explicit FS_MG_TAIL that puts the tail's first level in the middle of the hierarchy
# the wall density that stands for "0.15" on a grid: at 0.15 the 16 level-1 cells of (8, 8) are all active (the CPU count), at 0.5 five are not
DENSITY = {(8, 8): 0.5}


def _kw(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def restatement(X, Y, wall_p, dtype, kw=()):
    """((p.current, p.next) after one MultigridRef.update, level 1's active map); computed once per case, read-only (every tail shares it)."""
    const, mask = C.scene(X, Y, wall_p)
    pc, pn, v = C.fields(X, Y, wall_p, dtype)
    ref = M.MultigridRef(O.OracleBC(const, mask, None, np.dtype(dtype)), C.DT, C.DX, **dict(kw))
    assert [lv.shape for lv in ref.levels] == C.SHAPES[(X, Y)]
    p = O.Buf2(pc.shape, 1, pc.dtype)
    p.current[...], p.next[...] = pc, pn
    ref.update(p, v.copy())
    out = (p.current, p.next, ref.levels[0].active)
    for a in out:
        a.setflags(write=False)
    return out[:2], out[2]


def set_tail(monkeypatch, tail):
    if tail is None:
        monkeypatch.delenv("FS_MG_TAIL", raising=False)
    else:
        monkeypatch.setenv("FS_MG_TAIL", str(tail))


def expected_tail_level(tail, levels):
    """FS_MG_TAIL = 0: no tail kernel; N > 0: the first level of at most N cells (0 when there is none)."""
    return next((k for k, (nx, ny) in enumerate(levels, start=1) if tail > 0 and nx * ny <= tail), 0)


def check_update(monkeypatch, const, mask, dtype, pc, pn, v, tail, exp=None, changes=True, **kw):
    """One update() of the product and of the restatement on the same arrays -> info().  exp: the restatement's (p.current, p.next) where the
    caller has them already.  changes=False: the restatement must hand the input back (and so must the product)."""
    import fs
    dtype = np.dtype(dtype)
    if exp is None:
        p = O.Buf2(pc.shape, 1, dtype)
        p.current[...], p.next[...] = pc, pn
        M.MultigridRef(O.OracleBC(const, mask, None, dtype), C.DT, C.DX, **kw).update(p, v.copy())
        exp = (p.current, p.next)
    assert all(np.isfinite(e).all() for e in exp), "the restatement's result is not finite"
    assert np.array_equal(exp[0], pc) != changes and (changes or np.array_equal(exp[1], pn))
    set_tail(monkeypatch, tail)
    fs.runtime.init(gpu=0, dtype="f64" if dtype == np.float64 else "f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        pu = fs.MultigridPressureUpdater(bc, C.DT, C.DX, **kw)
        solver = fs.MacSolver(bc, pu, fs.advect_upwind, C.DT, C.DX, RE, None)
        solver.v.current.from_numpy(v)
        solver.p.current.from_numpy(pc)
        solver.p.next.from_numpy(pn)
        pu.update(solver.p, solver.v.current)
        got = (solver.p.current.to_numpy(), solver.p.next.to_numpy())
        info = pu.info()
        levels = pu.levels
    finally:
        bc.device.close()
    print(f"{mask.shape} {dtype.name} FS_MG_TAIL={tail}: {info}")
    for name, a, e in zip(("p.current", "p.next"), got, exp):
        assert a.dtype == e.dtype == dtype
        assert np.array_equal(a, e), f"{mask.shape} {dtype.name} tail {tail} {kw} {name}: {int((a != e).sum())} cells differ, max {np.abs(a - e).max():.3e}"
    assert info["levels"] == len(levels)
    if tail is not None:
        assert info["tail_level"] == expected_tail_level(int(tail), levels), (tail, levels, info)
    return info


def _cases():
    out = []
    for grid in GRIDS:
        for wall_p in ((0.15, 0.3, 0.0) if grid in SPLIT else (0.15,)):
            for tail in (0, None) + ((SPLIT[grid],) if grid in SPLIT and wall_p == 0.15 else ()):
                out.append(pytest.param(grid, wall_p, tail, id=f"{grid[0]}x{grid[1]}-w{wall_p}-tail{'default' if tail is None else tail}"))
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("grid,wall_p,tail", _cases())
def test_one_update_on_random_masks(grid, wall_p, tail, dtype, hip_lib, monkeypatch):
    X, Y = grid
    density = DENSITY.get(grid, wall_p) if wall_p == 0.15 else wall_p
    exp, active = restatement(X, Y, density, dtype)
    if wall_p > 0:      # the case must exercise diag == 0, and not only that
        assert 0 < int((~active).sum()) < active.size, f"level 1 of {grid} at wall density {density}: {int((~active).sum())} of {active.size} cells inactive"
    const, mask = C.scene(X, Y, density)
    info = check_update(monkeypatch, const, mask, dtype, *C.fields(X, Y, density, dtype), tail, exp=exp)
    assert info["levels"] == len(C.SHAPES[grid])
    if tail == 0:       # residual + correction, 2 s half sweeps per visit of a level (level k: 2^(k-1) visits), restrict + prolong per coarse visit
        n = info["levels"]
        sweeps = sum(2 ** k * (64 if k == n - 1 else 3 * 2) * 2 for k in range(n))
        assert info["launches"] == 2 + sweeps + 2 * sum(2 ** k for k in range(1, n))
    elif info["tail_level"] == 1:
        assert info["launches"] == 3


DEGENERATE = [dict(coarse_sweeps=0), dict(coarsest_sweeps=0), dict(coarsest_sweeps=1), dict(pre=0, post=0),
              dict(coarse_sweeps=0, coarsest_sweeps=0), dict(n_cycles=0)]


@pytest.mark.parametrize("tail", [0, None], ids=["tail0", "taildefault"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kw", DEGENERATE, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_degenerate_counts(kw, dtype, tail, hip_lib, monkeypatch):
    """Counts of 0 and 1 that the constructor accepts, on (96, 64).  n_cycles=0: both buffers come back as they went in.  No sweeps on any
    level: the correction is exactly zero, so the result is also the oracle's red-black SOR alone - RB-SOR(pre), the boundary kernel on
    p.current and on p.next as the cycle applies it between its legs, RB-SOR(post).  (Not RB-SOR(pre + post) in one go: the boundary kernel on
    p.next rewrites wall cells that the first even half sweep of the second leg reads; on this mask the two differ in 135 cells of p.next.)"""
    X, Y, wall_p = 96, 64, 0.15
    const, mask = C.scene(X, Y, wall_p)
    pc, pn, v = C.fields(X, Y, wall_p, dtype)
    exp, _ = restatement(X, Y, wall_p, dtype, _kw(kw))
    if kw == dict(coarse_sweeps=0, coarsest_sweeps=0):
        bc = O.OracleBC(const, mask, None, np.dtype(dtype))
        p = O.Buf2(pc.shape, 1, pc.dtype)
        p.current[...], p.next[...] = pc, pn
        O.OracleRedBlackSor(bc, C.DT, C.DX, 1.3, 2).update(p, v.copy())
        bc.set_pressure_boundary_condition(p.current)
        bc.set_pressure_boundary_condition(p.next)
        O.OracleRedBlackSor(bc, C.DT, C.DX, 1.3, 2).update(p, v.copy())
        assert np.array_equal(exp[0], p.current) and np.array_equal(exp[1], p.next), "a zero correction must leave red-black SOR alone"
    check_update(monkeypatch, const, mask, dtype, pc, pn, v, tail, exp=exp, changes=kw != dict(n_cycles=0), **kw)


def _solvers(grid, wall_p, dtype, scheme, vc):
    import fs
    const, mask = C.scene(*grid, wall_p)
    obc = O.OracleBC(const, mask, None, np.dtype(dtype))
    pu = M.MultigridRef(obc, C.DT, C.DX)
    ovc = O.OracleVorticity(obc, C.DT, C.DX, vc) if vc is not None else None
    ref = O.OracleCipSolver(obc, pu, C.DT, C.DX, RE, ovc) if scheme == "cip" else O.OracleMacSolver(obc, pu, scheme, C.DT, C.DX, RE, ovc)
    fs.runtime.init(gpu=0, dtype="f64" if np.dtype(dtype) == np.float64 else "f32")
    bc = fs.BoundaryCondition(const, mask)
    try:
        mg = fs.MultigridPressureUpdater(bc, C.DT, C.DX)
        fvc = fs.VorticityConfinement(bc, C.DT, C.DX, vc) if vc is not None else None
        if scheme == "cip":
            solver = fs.CipMacSolver(bc, mg, C.DT, C.DX, RE, fvc)
        else:
            solver = fs.MacSolver(bc, mg, fs.advect_upwind if scheme == "upwind" else fs.advect_kk_scheme, C.DT, C.DX, RE, fvc)
    except BaseException:
        bc.device.close()
        raise
    return ref, solver, bc


@pytest.mark.parametrize("tail", [0, None], ids=["tail0", "taildefault"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("grid,scheme,vc", [((72, 40), "cip", 5.0), ((260, 24), "kk", 10.0), ((1088, 8), "upwind", None)])
def test_four_step_trajectories(grid, scheme, vc, dtype, tail, hip_lib, monkeypatch):
    """Four steps from a random v and p at Re 1000 on a random mask (wall density 0.15): every field after every step."""
    wall_p = 0.15
    set_tail(monkeypatch, tail)
    pc, _, v = C.fields(*grid, wall_p, dtype)
    ref, solver, bc = _solvers(grid, wall_p, dtype, scheme, vc)
    try:
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
                assert a.dtype == e.dtype and np.array_equal(a, e), f"{grid} {scheme} {dtype} tail {tail} step {step} {k}: {int((a != e).sum())} cells differ"
        info = solver.pressure_updater.info()
        print(f"{grid} {scheme} {dtype} FS_MG_TAIL={tail}: {info}")
        if tail == 0:
            assert info["tail_level"] == 0
    finally:
        bc.device.close()


@pytest.mark.parametrize("tail,kw", [(0, {}), (None, dict(n_cycles=2))], ids=["tail0", "two-cycles"])
def test_graph_replay_equals_eager_stepping(tail, kw, hip_lib, monkeypatch):
    """tests/test_gpu_multigrid.py's replay test with hundreds of captured launches per step (FS_MG_TAIL=0), and with two cycles per step."""
    from test_gpu_multigrid import make_sim
    set_tail(monkeypatch, tail)
    n = 30
    eager = make_sim(5, 32, "float32", vc=None, **kw)
    try:
        for _ in range(n):
            eager.step()
        exp = eager.field_to_numpy()
        info = eager._solver.pressure_updater.info()
    finally:
        eager._solver._bc.device.close()
    assert info["tail_level"] == (0 if tail == 0 else 1) and (info["launches"] > 100 if tail == 0 else info["launches"] == 3)
    sim = make_sim(5, 32, "float32", vc=None, **kw)
    try:
        sim.run(n, graph=True)
        assert sim._graph is not None, "no period of the multigrid step was captured"
        out = sim.field_to_numpy()
    finally:
        sim._solver._bc.device.close()
    for k in exp:
        assert np.isfinite(exp[k]).all() and np.array_equal(out[k], exp[k]), k
