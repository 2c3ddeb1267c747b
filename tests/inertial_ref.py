"""NumPy float64 restatement of the inertial tracer advance and of the accumulated occupancy (csrc/fs_tracer.h k_tracer_advance_inertial /
k_tracer_accumulate, include/fs_hip.h fs_tracer_create_inertial ... fs_tracer_accum_*), built on tracers_ref.velocity_ref and
tracers_ref.inside: every operation one correctly rounded double operation in the order of the specification.  The yardstick of
tests/test_inertial_cpu.py and tests/test_gpu_inertial.py: states, deposit planes and accumulators compare with np.array_equal, in f32
and in f64 runs.

Positions are in cell units: cell (i, j) covers [i, i + 1) x [j, j + 1), its stored value sits at (i + 0.5, j + 0.5)."""
import numpy as np
import tracers_ref
from tracers_ref import ALIVE, EXPIRED, LEFT, MASK_OUTFLOW, MASK_WALL, WALL_HIT, inside, velocity_ref


def response_ref(tau, dt):
    """alpha = -expm1(-dt / tau), 1 for tau == 0 (what the host hands the device)."""
    tau = np.asarray(tau, np.float64)
    out = np.ones(tau.shape, np.float64)
    pos = tau > 0
    out[pos] = -np.expm1(-np.float64(dt) / tau[pos])
    return out


def new_state(seeds, alpha, tau):
    st = tracers_ref.new_state(seeds)
    n = len(st["x"])
    st["pu"], st["pw"] = np.zeros(n, np.float64), np.zeros(n, np.float64)
    st["alpha"] = np.broadcast_to(np.asarray(alpha, np.float64), (n,)).copy()
    st["tau"] = np.broadcast_to(np.asarray(tau, np.float64), (n,)).copy()
    return st


def advance_ref(state, v, mask, h, gravity=(0.0, 0.0), respawn=True, max_age=0, limit=None, deposits=None):
    """One launch of k_tracer_advance_inertial on `state` (in place): v (X, Y, 2) in the field's precision as stored, mask (X, Y) uint8,
    h = dt / dx, gravity (gx, gy); limit: v owes limit_field(limit); deposits: int32 (X, Y) plane that takes the wall hits, or None."""
    v, mask = np.asarray(v), np.asarray(mask)
    X, Y = mask.shape
    h, gx, gy = np.float64(h), np.float64(gravity[0]), np.float64(gravity[1])
    alive = np.nonzero(state["status"] == ALIVE)[0]
    x, y = state["x"][alive], state["y"][alive]
    age0 = state["age"][alive]
    pu, pw = state["pu"][alive].copy(), state["pw"][alive].copy()
    alpha, tau = state["alpha"][alive], state["tau"][alive]
    n = len(alive)
    fate = np.zeros(n, np.int32)
    px, py = x.copy(), y.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        U, W = velocity_ref(v, x, y, limit)
        fresh = age0 == 0
        pu[fresh], pw[fresh] = U[fresh], W[fresh]
        su, sw = tau * gx, tau * gy
        pu = pu + alpha * ((U + su) - pu)
        pw = pw + alpha * ((W + sw) - pw)
        xn, yn = x + h * pu, y + h * pw
        ok = inside(xn, yn, X, Y)
    fate[~ok] = LEFT
    b = np.nonzero(ok)[0]
    ci, cj = np.floor(xn[b]).astype(np.int64), np.floor(yn[b]).astype(np.int64)
    m = mask[ci, cj]
    hit = m == MASK_WALL
    fate[b[hit]] = WALL_HIT
    fate[b[m == MASK_OUTFLOW]] = LEFT
    if deposits is not None:
        np.add.at(deposits, (ci[hit], cj[hit]), 1)
    move = (m != MASK_WALL) & (m != MASK_OUTFLOW)
    px[b[move]], py[b[move]] = xn[b[move]], yn[b[move]]
    age = age0 + 1
    if max_age > 0:
        fate[(fate == ALIVE) & (age >= max_age)] = EXPIRED
    done = fate != ALIVE
    if respawn:
        px[done], py[done] = state["seeds"][alive[done], 0], state["seeds"][alive[done], 1]
        age[done] = 0
        pu[done] = pw[done] = 0.0
        state["respawns"][alive[done]] += 1
    else:
        state["status"][alive[done]] = fate[done]
    state["x"][alive], state["y"][alive], state["age"][alive] = px, py, age
    state["pu"][alive], state["pw"][alive] = pu, pw
    state["steps"] += 1
    return fate


def fields_ref(state, X, Y):
    """What k_tracer_fields bins: (count int64 (X, Y), age_sum int64 (X, Y)) of the alive particles inside the domain."""
    ok = (state["status"] == ALIVE) & inside(state["x"], state["y"], X, Y)
    i, j = np.floor(state["x"][ok]).astype(np.int64), np.floor(state["y"][ok]).astype(np.int64)
    count, age_sum = np.zeros((X, Y), np.int64), np.zeros((X, Y), np.int64)
    np.add.at(count, (i, j), 1)
    np.add.at(age_sum, (i, j), state["age"][ok].astype(np.int64))
    return count, age_sum


def samples_step(k, every, start):
    """Step k = 1, 2, ... since the accumulator was attached is a sampled one."""
    return k > start and (k - start) % every == 0


def new_accumulator(X, Y, every=1, start=0):
    return {"occupancy": np.zeros((X, Y), np.int64), "age_sum": np.zeros((X, Y), np.int64), "samples": 0, "steps": 0, "every": every, "start": start}


def accumulate_ref(acc, state):
    """One launch of k_tracer_accumulate behind an advance of `state`."""
    acc["steps"] += 1
    if samples_step(acc["steps"], acc["every"], acc["start"]):
        X, Y = acc["occupancy"].shape
        count, age_sum = fields_ref(state, X, Y)
        acc["occupancy"] += count
        acc["age_sum"] += age_sum
        acc["samples"] += 1


def run_reference(sim, steps, state, gravity=(0.0, 0.0), respawn=True, max_age=0, deposits=None, acc=None):
    """Step `sim` (a twin without tracers) eagerly `steps` times and advance `state` from its downloaded velocity after every step."""
    mask = np.asarray(sim._solver._bc.mask)
    h = sim._solver.dt / sim._solver.dx
    for _ in range(steps):
        sim.step()
        advance_ref(state, sim.field_to_numpy()["v"], mask, h, gravity, respawn, max_age, deposits=deposits)
        if acc is not None:
            accumulate_ref(acc, state)
    return state


def assert_state_equal(got, exp, what=""):
    """got: FluidSimulator.tracers() of an inertial set, or a dict with "pu" / "pw" keys; exp: a state of this module."""
    tracers_ref.assert_state_equal(got, exp, what)
    for a, b in (("u", "pu"), ("w", "pw")):
        g = got[a] if a in got else got[b]
        assert np.array_equal(g, exp[b], equal_nan=True), f"{what}{b} differs from the NumPy float64 restatement"


def band_scene(dtype=np.float32):
    """Grid 33 x 16: flow (1, 0) everywhere except columns 14 .. 19 where it is (0, 1); a wall block at i in [20, 24), j in [2, 10); the last
    column is outflow.  A light particle turns with the band and leaves through the top edge; a heavy one crosses it and hits the block."""
    X, Y = 33, 16
    mask = np.zeros((X, Y), np.uint8)
    mask[20:24, 2:10] = MASK_WALL
    mask[X - 1, :] = MASK_OUTFLOW
    v = np.zeros((X, Y, 2), dtype)
    v[..., 0] = 1.0
    v[14:20, :, 0] = 0.0
    v[14:20, :, 1] = 1.0
    seeds = np.array([[2.5, 4.5], [2.5, 5.25], [2.5, 6.5]])
    return mask, v, seeds
