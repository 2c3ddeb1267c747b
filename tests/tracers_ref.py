"""NumPy float64 restatement of the tracer advance (csrc/fs_tracer.h, include/fs_hip.h fs_tracer_advance): one midpoint step of every alive
particle, every operation one correctly rounded double operation in the order of the specification, the corner values through limit_ref
(tests/mean_ref.py) when a deferred limit_field is owed.  The yardstick of tests/test_tracers_cpu.py and tests/test_gpu_tracers.py: states
compare with np.array_equal, in f32 and in f64 runs.

Positions are in cell units: cell (i, j) covers [i, i + 1) x [j, j + 1), its stored value sits at (i + 0.5, j + 0.5)."""
import numpy as np
from mean_ref import limit_ref

ALIVE, LEFT, WALL_HIT, EXPIRED = 0, 1, 2, 3
MASK_WALL, MASK_OUTFLOW = 1, 3


def new_state(seeds):
    seeds = np.array(seeds, np.float64).reshape(-1, 2)
    n = len(seeds)
    return {"x": seeds[:, 0].copy(), "y": seeds[:, 1].copy(), "age": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
            "respawns": np.zeros(n, np.int32), "seeds": seeds, "steps": 0}


def inside(x, y, X, Y):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x < X) & (y >= 0) & (y < Y)        # False for NaN


def velocity_ref(v, x, y, limit=None):
    """V(x, y) for points inside the domain: bilinear in the four stored values around (x - 0.5, y - 0.5) -> (u, w) in float64."""
    X, Y = v.shape[:2]
    fx, fy = x - 0.5, y - 0.5
    i0 = np.clip(np.floor(fx).astype(np.int64), 0, X - 2)
    j0 = np.clip(np.floor(fy).astype(np.int64), 0, Y - 2)
    tx = np.minimum(np.maximum(fx - i0.astype(np.float64), 0.0), 1.0)
    ty = np.minimum(np.maximum(fy - j0.astype(np.float64), 0.0), 1.0)
    corners = [v[i0, j0], v[i0 + 1, j0], v[i0, j0 + 1], v[i0 + 1, j0 + 1]]      # a00, a10, a01, a11: (n, 2) in the field's precision
    if limit is not None:
        corners = [limit_ref(c, limit) for c in corners]
    a00, a10, a01, a11 = (c.astype(np.float64) for c in corners)
    sx, sy = 1.0 - tx, 1.0 - ty
    out = []
    for c in (0, 1):
        out.append(sy * (sx * a00[:, c] + tx * a10[:, c]) + ty * (sx * a01[:, c] + tx * a11[:, c]))
    return out[0], out[1]


def advance_ref(state, v, mask, h, respawn=True, max_age=0, limit=None):
    """One launch of k_tracer_advance on `state` (in place): v (X, Y, 2) in the field's precision as stored, mask (X, Y) uint8,
    h = dt / dx; limit: v owes limit_field(limit)."""
    v, mask = np.asarray(v), np.asarray(mask)
    X, Y = mask.shape
    h = np.float64(h)
    alive = np.nonzero(state["status"] == ALIVE)[0]
    x, y = state["x"][alive], state["y"][alive]
    n = len(alive)
    fate = np.zeros(n, np.int32)
    px, py = x.copy(), y.copy()
    hh = np.float64(0.5) * h
    with np.errstate(invalid="ignore", over="ignore"):
        k1u, k1w = velocity_ref(v, x, y, limit)
        xm, ym = x + hh * k1u, y + hh * k1w
        ok1 = inside(xm, ym, X, Y)
        fate[~ok1] = LEFT
        a = np.nonzero(ok1)[0]
        k2u, k2w = velocity_ref(v, xm[a], ym[a], limit)
        xn, yn = x[a] + h * k2u, y[a] + h * k2w
        ok2 = inside(xn, yn, X, Y)
    fate[a[~ok2]] = LEFT
    b = a[ok2]
    xn, yn = xn[ok2], yn[ok2]
    m = mask[np.floor(xn).astype(np.int64), np.floor(yn).astype(np.int64)]
    fate[b[m == MASK_WALL]] = WALL_HIT
    fate[b[m == MASK_OUTFLOW]] = LEFT
    move = (m != MASK_WALL) & (m != MASK_OUTFLOW)
    px[b[move]], py[b[move]] = xn[move], yn[move]
    age = state["age"][alive] + 1
    if max_age > 0:
        fate[(fate == ALIVE) & (age >= max_age)] = EXPIRED
    done = fate != ALIVE
    if respawn:
        px[done], py[done] = state["seeds"][alive[done], 0], state["seeds"][alive[done], 1]
        age[done] = 0
        state["respawns"][alive[done]] += 1
    else:
        state["status"][alive[done]] = fate[done]
    state["x"][alive], state["y"][alive], state["age"][alive] = px, py, age
    state["steps"] += 1
    return fate


def run_reference(sim, steps, state, respawn=True, max_age=0):
    """Step `sim` (a twin without tracers) eagerly `steps` times and advance `state` from its downloaded velocity after every step."""
    mask = np.asarray(sim._solver._bc.mask)
    h = sim._solver.dt / sim._solver.dx
    for _ in range(steps):
        sim.step()
        advance_ref(state, sim.field_to_numpy()["v"], mask, h, respawn, max_age)
    return state


def assert_state_equal(got, exp, what=""):
    for k in ("x", "y", "age", "status", "respawns", "seeds"):
        assert np.array_equal(got[k], exp[k], equal_nan=True), f"{what}{k} differs from the NumPy float64 restatement"
    assert int(got["steps"]) == int(exp["steps"]), f"{what}steps {got['steps']} != {exp['steps']}"


def fate_scene(X=33, Y=16, dtype=np.float32):
    """A scene in which every fate occurs by construction within 25 steps of h = 0.5: uniform flow (1, 0) in rows j < 12, (0, 1) in the rows
    above; a wall block at i in [20, 24), j in [4, 8); the last column is outflow; one NaN cell.  -> (mask, v, seeds, expected fates without
    respawn and with max_age = 20)."""
    mask = np.zeros((X, Y), np.uint8)
    mask[20:24, 4:8] = MASK_WALL
    mask[X - 1, :] = MASK_OUTFLOW
    v = np.zeros((X, Y, 2), dtype)
    v[:, :12, 0] = 1.0
    v[:, 12:, 1] = 1.0
    v[3, 1, :] = np.nan
    seeds = np.array([[10.5, 5.5],         # runs into the wall block: WALL
                      [25.5, 10.5],        # reaches the outflow column: LEFT
                      [5.5, 14.25],        # leaves through the top edge, where no outflow cell is: LEFT
                      [3.5, 1.5],          # sits on the NaN cell: LEFT
                      [2.5, 9.5]])         # still on its way at age 20: EXPIRED
    return mask, v, seeds, np.array([WALL_HIT, LEFT, LEFT, LEFT, EXPIRED], np.int32)
