"""CPU checks of the multigrid pressure updater's specification (tests/multigrid_ref.py) and of the product's host-side hierarchy
(fs/multigrid.py): the coefficient hierarchy, the convergence of W-cycles against literal red-black SOR on developed flows, and the
regression that guards the rule "wall cells K7 never writes are Dirichlet points".

Convergence criterion (the issue's): from a state whose v is frozen after 60 CIP steps of the oracle, 8 cycles of W(2, 2), omega 1.3, against
200 literal RB-SOR(1.3) iterations from the same state; the l2 Poisson residual over fluid cells must fall strictly from cycle 2 on and end
at <= 0.25 x the RB-SOR residual.  Measured ratios (float64): DESIGN.md section 4af."""
import functools

import numpy as np
import pytest

import multigrid_cases as C
import multigrid_ref as M
from oracle import oracle as O

CASES = [(1, 32), (2, 32), (4, 32), (5, 32), (1, 64), (2, 64), (4, 64), (5, 64), (3, 64)]


def _bc(scene, res, dtype=np.float64):
    from fs.boundary_condition import create_scene_arrays
    const, mask, _ = create_scene_arrays(scene, res)
    return O.OracleBC(const, mask, None, dtype), const, mask


@functools.lru_cache(maxsize=None)
def developed(scene, res):
    """(bc, dt, dx, p.current, p.next, v) after 60 oracle CIP + vorticity-confinement steps in float64 (computed once, never modified)."""
    bc, const, mask = _bc(scene, res)
    dt, dx = 0.05 / res, 1.0 / res
    sim = O.make_simulator(const, mask, None, scheme="cip", dt=dt, dx=dx, re=1.0e6, vor_eps=5.0, dtype=np.float64)
    for _ in range(60):
        sim.update()
    out = (bc, dt, dx, sim.p.current.copy(), sim.p.next.copy(), sim.v.current.copy())
    for a in out[3:]:
        a.setflags(write=False)
    return out


def _buf(pc, pn):
    p = O.Buf2(pc.shape, 1, pc.dtype)
    p.current[...], p.next[...] = pc, pn
    return p


def convergence(scene, res, wall_term=True, cycles=8, correct_next=True):
    """(residual at the start, [after each cycle], after 200 RB-SOR iterations)."""
    bc, dt, dx, pc, pn, v = developed(scene, res)
    start = M.poisson_l2(bc, dt, dx, pc, v)
    p = _buf(pc, pn)
    O.OracleRedBlackSor(bc, dt, dx, 1.3, 200).update(p, v)
    sor = M.poisson_l2(bc, dt, dx, p.current, v)
    p = _buf(pc, pn)
    mg = M.MultigridRef(bc, dt, dx, relaxation_factor=1.3, n_cycles=1, pre=2, post=2, wall_term=wall_term, correct_next=correct_next)
    hist = []
    for _ in range(cycles):
        mg.update(p, v)
        hist.append(M.poisson_l2(bc, dt, dx, p.current, v))
    return start, hist, sor


def meets(hist, sor):
    return all(b < a for a, b in zip(hist[1:], hist[2:])) and hist[-1] <= 0.25 * sor


@pytest.mark.parametrize("res,shapes", [(32, [(32, 16), (16, 8), (8, 4), (4, 2), (2, 1)]), (40, [(40, 20), (20, 10), (10, 5)]),
                                        (48, [(48, 24), (24, 12), (12, 6), (6, 3)]), (80, [(80, 40), (40, 20), (20, 10), (10, 5)])])
def test_level_shapes(res, shapes):
    bc, _, mask = _bc(1, res)
    levels, _ = M.hierarchy(bc)
    assert [lv.shape for lv in levels] == shapes
    from fs.multigrid import build_hierarchy
    assert [lv[0].shape for lv in build_hierarchy(mask)] == shapes


def test_odd_resolution_has_no_coarse_level():
    bc, _, mask = _bc(1, 33)
    with pytest.raises(ValueError):
        M.hierarchy(bc)
    from fs.multigrid import build_hierarchy
    with pytest.raises(ValueError):
        build_hierarchy(mask)


@pytest.mark.parametrize("scene", [1, 2, 3, 4, 5])
def test_coefficients_are_dyadic_and_the_product_builds_the_same(scene):
    """Every coefficient times 2^level is an integer, float32 holds it exactly, and fs.multigrid (mask rules) equals the restatement (K7 probe)."""
    from fs.multigrid import build_hierarchy, never_written
    for res in (32, 64):
        bc, _, mask = _bc(scene, res)
        assert np.array_equal(never_written(mask), M.probe_never_written(bc))
        levels, _ = M.hierarchy(bc)
        mine = build_hierarchy(mask, np.float32)
        assert len(mine) == len(levels)
        for k, (lv, (cx, cy, diag)) in enumerate(zip(levels, mine), start=1):
            for a, b in ((lv.cx, cx), (lv.cy, cy), (lv.diag, diag)):
                s = a * 2.0 ** k
                assert np.array_equal(s, np.round(s))
                assert b.dtype == np.float32 and np.array_equal(a, b.astype(np.float64))


@pytest.mark.parametrize("wall_p", C.DENSITIES)
@pytest.mark.parametrize("grid", list(C.SHAPES), ids=lambda g: f"{g[0]}x{g[1]}")
def test_random_masks_through_the_host_hierarchy(grid, wall_p):
    """What tests/test_gpu_multigrid_shapes.py rests on: on random masks (fluid on the domain edge, one-cell walls, inflow and outflow anywhere;
    wide, tall, one-level and 1 x 1-coarsest grids) the product's mask rules equal the K7 probe, its hierarchy equals the restatement's array
    for array in both dtypes, and one restatement update from uniform(-1, 1) fields is finite."""
    from fs.multigrid import build_hierarchy, never_written
    const, mask = C.scene(*grid, wall_p)
    for dtype in ("float32", "float64"):
        bc = O.OracleBC(const, mask, None, np.dtype(dtype))
        assert np.array_equal(never_written(mask), M.probe_never_written(bc))
        mg = M.MultigridRef(bc, C.DT, C.DX)
        mine = build_hierarchy(mask, np.dtype(dtype))
        assert [lv.shape for lv in mg.levels] == C.SHAPES[grid] == [lv[0].shape for lv in mine]
        for lv, (cx, cy, diag) in zip(mg.levels, mine):
            for a, b in ((lv.cx, cx), (lv.cy, cy), (lv.diag, diag)):
                assert a.dtype == b.dtype == np.dtype(dtype) and np.array_equal(a, b)
        pc, pn, v = C.fields(*grid, wall_p, dtype)
        p = _buf(pc, pn)
        mg.update(p, v.copy())
        assert np.isfinite(p.current).all() and np.isfinite(p.next).all()
        assert not np.array_equal(p.current, pc)


@pytest.mark.parametrize("scene,faces", [(1, 0), (2, 4), (4, 4), (5, 0)])
def test_d0_counts_the_never_written_faces(scene, faces):
    bc, _, mask = _bc(scene, 32)
    _, d0 = M.hierarchy(bc)
    _, d0_plain = M.hierarchy(bc, wall_term=False)
    assert int((d0 - d0_plain).sum()) == faces
    from fs.multigrid import level0
    assert np.array_equal(level0(mask)[2], d0)


@pytest.mark.parametrize("scene,res", CASES)
def test_w_cycles_converge_where_rbsor_stalls(scene, res):
    start, hist, sor = convergence(scene, res)
    print(f"scene {scene} res {res}: start {start:.4e}  rbsor200 {sor:.4e} ({sor / start:.3f})  cycles "
          + " ".join(f"{h / start:.3e}" for h in hist) + f"  ratio to rbsor {hist[-1] / sor:.3e}")
    assert all(b < a for a, b in zip(hist[1:], hist[2:])), f"residual not strictly decreasing from cycle 2 on: {hist}"
    assert hist[-1] <= 0.25 * sor, f"after 8 cycles {hist[-1]:.4e} > 0.25 x RB-SOR(200) {sor:.4e}"


def test_insulating_never_written_walls_break_scene_4():
    """Finding 2: with d0's wall term zeroed (never-written walls treated as insulating) scene 4 at res 32 must NOT meet the criterion."""
    _, hist, sor = convergence(4, 32, wall_term=False)
    print("scene 4 res 32 without the wall term:", hist, "rbsor", sor)
    assert not meets([h if np.isfinite(h) else np.inf for h in hist], sor)


def test_correcting_p_current_alone_does_not_converge():
    """The literal two-buffer smoother blends even cells with p.next: a correction that p.next does not receive comes back as an error of
    (1 - omega) x the correction, and scene 1 at res 32 must NOT meet the criterion (measured: the residual ends 87 x above its start)."""
    _, hist, sor = convergence(1, 32, correct_next=False)
    assert not meets(hist, sor)
