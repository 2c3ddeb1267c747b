"""NumPy float64 restatement of the flow-map kernels (csrc/fs_lcs.h, include/fs_hip.h fs_flowmap_*): the seeding of the lattice, the advance
across one interval of the snapshot ring - every operation one correctly rounded double operation in the order of the header, the slot
velocities through tracers_ref.velocity_ref on the slot planes - and the Cauchy-Green pass.  The yardstick of tests/test_lcs_cpu.py and
tests/test_gpu_lcs.py: states compare with np.array_equal(..., equal_nan=True), in f32 and in f64 runs.

Arrays are (nx, ny), node (a, b) at [a, b]; slots are fs_pod_get's (M, 3, X, Y)."""
import numpy as np
from tracers_ref import inside, velocity_ref

ALIVE, LEFT, WALL_HIT, UNSEEDED = 0, 1, 2, 4
MASK_WALL, MASK_INFLOW, MASK_OUTFLOW = 1, 2, 3


def seed_ref(mask, box=None, refine=1):
    """k_flowmap_seed -> {"x", "y", "status", "lam", "box", "refine"}."""
    mask = np.asarray(mask)
    X, Y = mask.shape
    x0, y0, x1, y1 = (0, 0, X, Y) if box is None else box
    r = int(refine)
    a, b = np.arange(r * (x1 - x0)), np.arange(r * (y1 - y0))
    xs = np.float64(x0) + (a.astype(np.float64) + 0.5) / np.float64(r)
    ys = np.float64(y0) + (b.astype(np.float64) + 0.5) / np.float64(r)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    wall = mask[np.ix_(x0 + a // r, y0 + b // r)] == MASK_WALL
    return {"x": np.ascontiguousarray(x), "y": np.ascontiguousarray(y), "status": np.where(wall, UNSEEDED, ALIVE).astype(np.int32),
            "lam": np.full(x.shape, np.nan), "box": (x0, y0, x1, y1), "refine": r}


def _plane_pair(slot):
    """(3, X, Y) -> (X, Y, 2): the u and w planes as velocity_ref takes them."""
    return np.stack([slot[0], slot[1]], axis=-1)


def _velocity(va, vb, x, y, tau):
    ua, wa = velocity_ref(va, x, y)
    ub, wb = velocity_ref(vb, x, y)
    st = np.float64(1.0) - tau
    return st * ua + tau * ub, st * wa + tau * wb


def advance_ref(state, slot_from, slot_to, mask, h, substeps=1):
    """One launch of k_flowmap_advance on `state` (in place): the two slots (3, X, Y) in the fields' precision as the ring stores them."""
    mask = np.asarray(mask)
    X, Y = mask.shape
    va, vb = _plane_pair(np.asarray(slot_from)), _plane_pair(np.asarray(slot_to))
    h, S = np.float64(h), int(substeps)
    hh = np.float64(0.5) * h
    gone = MASK_OUTFLOW if h > 0 else MASK_INFLOW
    flat = {k: state[k].reshape(-1) for k in ("x", "y", "status")}          # (views: the arrays are contiguous)
    for s in range(S):
        tau0, tau1 = np.float64(s) / np.float64(S), (np.float64(s) + 0.5) / np.float64(S)
        alive = np.nonzero(flat["status"] == ALIVE)[0]
        x, y = flat["x"][alive], flat["y"][alive]
        fate = np.zeros(len(alive), np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            ku, kw = _velocity(va, vb, x, y, tau0)
            xm, ym = x + hh * ku, y + hh * kw
            ok1 = inside(xm, ym, X, Y)
            fate[~ok1] = LEFT
            a = np.nonzero(ok1)[0]
            ku, kw = _velocity(va, vb, xm[a], ym[a], tau1)
            xn, yn = x[a] + h * ku, y[a] + h * kw
            ok2 = inside(xn, yn, X, Y)
        fate[a[~ok2]] = LEFT
        b = a[ok2]
        xn, yn = xn[ok2], yn[ok2]
        m = mask[np.floor(xn).astype(np.int64), np.floor(yn).astype(np.int64)]
        fate[b[m == MASK_WALL]] = WALL_HIT
        fate[b[m == gone]] = LEFT
        move = (m != MASK_WALL) & (m != gone)
        flat["x"][alive[b[move]]], flat["y"][alive[b[move]]] = xn[move], yn[move]
        done = fate != ALIVE
        flat["status"][alive[done]] = fate[done]
    return state


def _diff(p, present, axis, r):
    """The difference of p along a lattice axis by the header's rule -> (values, whether any neighbour was present)."""
    n = p.shape[axis]
    pm, pp = np.roll(p, 1, axis), np.roll(p, -1, axis)
    idx = np.arange(n).reshape((-1, 1) if axis == 0 else (1, -1))
    lo = np.roll(present, 1, axis) & (idx > 0)
    hi = np.roll(present, -1, axis) & (idx < n - 1)
    r = np.float64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        central, fwd, bwd = (pp - pm) * (np.float64(0.5) * r), (pp - p) * r, (p - pm) * r
    return np.where(lo & hi, central, np.where(hi, fwd, bwd)), lo | hi


def cauchy_green_ref(state):
    """k_flowmap_cauchy_green on `state` (in place): lam from the positions of the lattice neighbours."""
    x, y, r = state["x"], state["y"], state["refine"]
    seeded = state["status"] != UNSEEDED
    dxx, okx = _diff(x, seeded, 0, r)
    dyx, _ = _diff(y, seeded, 0, r)
    dxy, oky = _diff(x, seeded, 1, r)
    dyy, _ = _diff(y, seeded, 1, r)
    with np.errstate(invalid="ignore", over="ignore"):
        c11, c12, c22 = dxx * dxx + dyx * dyx, dxx * dxy + dyx * dyy, dxy * dxy + dyy * dyy
        d = c11 - c22
        lam = np.float64(0.5) * (c11 + c22) + np.sqrt(np.float64(0.25) * (d * d) + c12 * c12)
    state["lam"] = np.where(seeded & okx & oky, lam, np.nan)
    return state


def chronological(samples, M):
    """The slot of every resident sample, oldest first (a plain loop over the samples the ring has seen)."""
    slot_of = {}
    for k in range(int(samples)):
        slot_of[k % M] = k
    return [s for s, _ in sorted(slot_of.items(), key=lambda kv: kv[1])]


def flow_map_ref(slots, samples, mask, every, dt, dx, direction="backward", refine=1, box=None, substeps=1, first=None, last=None):
    """What FluidSimulator.flow_map computes, from the downloaded ring: -> the state after the last interval and the Cauchy-Green pass."""
    order = chronological(samples, len(slots))
    n = len(order)
    i0 = 0 if first is None else first % n
    i1 = n - 1 if last is None else last % n
    walk = order[i0:i1 + 1]
    h = float(every) * float(dt) / (float(dx) * float(substeps))
    if direction == "backward":
        walk, h = walk[::-1], -h
    st = seed_ref(mask, box, refine)
    for a, b in zip(walk[:-1], walk[1:]):
        advance_ref(st, slots[a], slots[b], mask, h, substeps)
    return cauchy_green_ref(st)


def assert_state_equal(got, exp, what=""):
    for k in ("x", "y", "status", "lam"):
        assert np.asarray(got[k]).shape == exp[k].shape, f"{what}{k}: shape {np.asarray(got[k]).shape} != {exp[k].shape}"
        assert np.array_equal(got[k], exp[k], equal_nan=True), f"{what}{k} differs from the NumPy float64 restatement"


def fate_rings(X=33, Y=16, M=4, dtype=np.float32):
    """The scene of the bit-for-bit cases, modelled on tracers_ref.fate_scene: a wall block at i in [20, 24), j in [4, 8); the last column
    outflow, the first inflow; flow (1, 0) in rows j < 12 and (0, 1) above, scaled by 0.6 + 0.3 m in snapshot m; one NaN cell in snapshot 1.
    Wall cells hold 0, as the capture stores them.  -> (mask, slots (M, 3, X, Y))."""
    mask = np.zeros((X, Y), np.uint8)
    mask[20:24, 4:8] = MASK_WALL
    mask[X - 1, :] = MASK_OUTFLOW
    mask[0, :] = MASK_INFLOW
    slots = np.zeros((M, 3, X, Y), dtype)
    for m in range(M):
        scale = 0.6 + 0.3 * m
        slots[m, 0, :, :12] = scale
        slots[m, 1, :, 12:] = scale
        slots[m, 2] = 0.1 * m
    slots[1, :2, 3, 1] = np.nan
    slots[:, :, mask == MASK_WALL] = 0
    return mask, slots
