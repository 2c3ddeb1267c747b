"""Tracer particles without a device: the NumPy restatement of the advance (tests/tracers_ref.py) on flows with a known answer and with
every fate produced by construction, and the host helpers of fs/tracers.py (seed builders, the seed check, residence time)."""
import numpy as np
import pytest
from tracers_ref import ALIVE, EXPIRED, LEFT, WALL_HIT, advance_ref, fate_scene, new_state, velocity_ref


def test_solid_body_rotation_grows_the_radius_by_the_midpoint_factor():
    """u = -(y - c), w = x - c: bilinear interpolation is exact and the midpoint rule algebraic - every step turns the particle and
    multiplies its radius by sqrt(1 + h^4 / 4)."""
    X = Y = 64
    c = 32.0
    i, j = np.meshgrid(np.arange(X) + 0.5, np.arange(Y) + 0.5, indexing="ij")
    v = np.stack([-(j - c), i - c], axis=-1)
    mask = np.zeros((X, Y), np.uint8)
    rng = np.random.default_rng(3)
    r0 = rng.uniform(2.0, 25.0, 200)
    phi = rng.uniform(0.0, 2 * np.pi, 200)
    seeds = np.stack([c + r0 * np.cos(phi), c + r0 * np.sin(phi)], axis=1)
    u, w = velocity_ref(v, seeds[:, 0], seeds[:, 1])
    assert np.allclose(u, -(seeds[:, 1] - c), rtol=0, atol=1e-12) and np.allclose(w, seeds[:, 0] - c, rtol=0, atol=1e-12)
    st = new_state(seeds)
    h = 0.05
    growth = np.sqrt(1.0 + h ** 4 / 4.0)
    for n in range(1, 101):
        advance_ref(st, v, mask, h, respawn=False)
        r = np.hypot(st["x"] - c, st["y"] - c)
        assert np.all(np.abs(r / (r0 * growth ** n) - 1.0) < 1e-12), n
    assert st["steps"] == 100 and np.all(st["status"] == ALIVE) and np.all(st["age"] == 100) and not st["respawns"].any()
    # ... and turned by 100 atan(h / (1 - h^2 / 2))
    turned = np.unwrap(np.stack([phi, np.arctan2(st["y"] - c, st["x"] - c)]), axis=0)[1] - phi
    assert np.allclose(np.mod(turned, 2 * np.pi), np.mod(100 * np.arctan2(h, 1.0 - h * h / 2.0), 2 * np.pi), rtol=0, atol=1e-9)


def test_velocity_uses_constant_extrapolation_in_the_outer_half_cells():
    v = np.zeros((4, 3, 2), np.float32)
    v[..., 0] = np.arange(4, dtype=np.float32)[:, None]           # u = i
    v[..., 1] = np.arange(3, dtype=np.float32)[None, :] * 10      # w = 10 j
    x = np.array([0.0, 0.25, 0.5, 1.0, 3.5, 3.99])
    y = np.array([0.0, 2.9, 1.5, 1.0, 0.5, 2.75])
    u, w = velocity_ref(v, x, y)
    assert np.array_equal(u, [0.0, 0.0, 0.0, 0.5, 3.0, 3.0])
    assert np.array_equal(w, [0.0, 20.0, 10.0, 5.0, 0.0, 20.0])


def test_every_fate_by_construction():
    mask, v, seeds, expected = fate_scene()
    st = new_state(seeds)
    seen = set()
    for _ in range(25):
        seen |= set(advance_ref(st, v, mask, 0.5, respawn=False, max_age=20).tolist())
    assert seen == {ALIVE, LEFT, WALL_HIT, EXPIRED}, "a fate code did not occur"
    assert np.array_equal(st["status"], expected)
    assert st["x"][0] == 19.5 and st["y"][0] == 5.5 and st["age"][0] == 19          # WALL: the last valid position, 18 moves and the fatal step
    assert st["x"][1] == 31.5 and st["age"][1] == 13                                # LEFT at the outflow column: not entered
    assert st["y"][2] < 16.0 and st["x"][2] == 5.5                                  # LEFT through the top edge
    assert st["x"][3] == 3.5 and st["y"][3] == 1.5 and st["age"][3] == 1            # NaN velocity: LEFT on the first step, where it was
    assert st["x"][4] == 12.5 and st["age"][4] == 20                                # EXPIRED keeps the step it just took
    assert not st["respawns"].any() and st["steps"] == 25
    frozen = {k: st[k].copy() for k in ("x", "y", "age", "status")}
    advance_ref(st, v, mask, 0.5, respawn=False, max_age=20)
    assert all(np.array_equal(st[k], frozen[k]) for k in frozen), "a dead particle was touched"
    # with respawn every fate sends the particle back to its seed
    st = new_state(seeds)
    for _ in range(25):
        advance_ref(st, v, mask, 0.5, respawn=True, max_age=20)
    assert np.all(st["status"] == ALIVE) and np.array_equal(st["respawns"], [1, 1, 6, 25, 1])
    assert st["x"][3] == 3.5 and st["age"][3] == 0 and st["age"][0] == 25 - 19


def test_seed_builders_and_filter():
    from fs.tracers import fluid_only, seed_grid, seed_line, seed_random
    line = seed_line((1.5, 0.5), (1.5, 8.5), 5)
    assert line.dtype == np.float64 and np.array_equal(line, [[1.5, 0.5], [1.5, 2.5], [1.5, 4.5], [1.5, 6.5], [1.5, 8.5]])
    assert np.array_equal(seed_line((0, 0), (2, 4), 1), [[1.0, 2.0]])
    grid = seed_grid((0, 0, 4, 2), 2, 2)
    assert np.array_equal(grid, [[1.0, 0.5], [1.0, 1.5], [3.0, 0.5], [3.0, 1.5]])
    mask = np.zeros((6, 9), np.uint8)
    mask[1, 2:5] = 1
    mask[1, 6] = 3
    mask[1, 8] = 2
    kept, dropped = fluid_only(mask, np.concatenate([line, [[-1.0, 2.0], [np.nan, 1.0], [6.0, 1.0]]]))
    assert dropped == 6 and np.array_equal(kept, [[1.5, 0.5], [1.5, 8.5]])      # wall, wall, outflow and the three outside go; inflow stays
    a, b, c = seed_random(mask, 300, 7), seed_random(mask, 300, 7), seed_random(mask, 300, 8)
    assert a.shape == (300, 2) and a.dtype == np.float64 and np.array_equal(a, b) and not np.array_equal(a, c)
    cells = np.floor(a).astype(int)
    assert np.all(mask[cells[:, 0], cells[:, 1]] == 0) and len(np.unique(cells, axis=0)) > 40
    assert fluid_only(mask, a)[1] == 0
    for bad in (lambda: seed_line((0, 0), (1, 1), 0), lambda: seed_grid((0, 0, 1, 1), 0, 3), lambda: seed_random(mask, 0),
                lambda: seed_random(np.ones((3, 3), np.uint8), 4)):
        with pytest.raises(ValueError):
            bad()


def test_check_seeds_names_the_first_offender():
    from fs.tracers import check_seeds
    mask = np.zeros((6, 9), np.uint8)
    mask[1, 2:5] = 1
    mask[5, :] = 3
    mask[0, :] = 2
    ok = check_seeds(mask, [[0.5, 0.5], [2.25, 3.0], [4.999, 8.999]])
    assert ok.dtype == np.float64 and ok.flags["C_CONTIGUOUS"] and ok.shape == (3, 2)
    for seeds, words in (([[2.5, 2.5], [1.5, 3.5], [1.5, 2.5]], ("seed 1", "wall", "(1, 3)")),
                         ([[2.5, 2.5], [5.5, 1.0]], ("seed 1", "outflow")),
                         ([[6.0, 1.0]], ("seed 0", "outside")),
                         ([[2.0, 2.0], [2.0, -0.001]], ("seed 1", "outside")),
                         ([[2.0, 9.0]], ("seed 0", "outside")),
                         ([[np.nan, 1.0]], ("seed 0", "outside")),
                         (np.zeros((0, 2)), ("at least one",))):
        with pytest.raises(ValueError) as e:
            check_seeds(mask, seeds)
        assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ValueError):
        check_seeds(mask, [1.0, 2.0, 3.0])


def test_residence_time_token_and_constants():
    from fs import tracers
    assert np.array_equal(tracers.residence_time(np.array([0, 3, 40], np.int32), 0.25), [0.0, 0.75, 10.0])
    assert (tracers.FATE_ALIVE, tracers.FATE_LEFT, tracers.FATE_WALL, tracers.FATE_EXPIRED) == (ALIVE, LEFT, WALL_HIT, EXPIRED)

    class _Set:
        serial = 41
    t = tracers.Tracers(None, _Set(), np.zeros((1, 2)), True, 0)
    assert t.token == ("tracer", 41) and t.respawn is True and t.max_age == 0
    assert set(tracers.KEYS) == {"x", "y", "age", "status", "respawns", "seeds", "steps"}
