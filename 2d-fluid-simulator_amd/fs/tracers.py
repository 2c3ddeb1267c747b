"""Host side of the tracer particles (new; the reference has none): seed builders, the seed check, fate codes and the residence time.
Pure NumPy: testable without a device.

The advance itself is a device launch per step (csrc/fs_tracer.h, include/fs_hip.h fs_tracer_*), driven by FluidSimulator.seed_tracers /
tracers / draw_tracers / stop_tracers.  Positions are float64 in CELL units: cell (i, j) covers [i, i + 1) x [j, j + 1) and its stored value
sits at (i + 0.5, j + 0.5)."""
import numpy as np

from .riders import Rider

FLUID, WALL, INFLOW, OUTFLOW = 0, 1, 2, 3
# status of a particle (fs_tracer_read): alive, or the fate that ended it when the set does not respawn
FATE_ALIVE, FATE_LEFT, FATE_WALL, FATE_EXPIRED = 0, 1, 2, 3
KEYS = ("x", "y", "age", "status", "respawns", "seeds", "steps")      # what FluidSimulator.tracers() returns
INERTIAL_KEYS = ("u", "w", "tau")      # ... and on top of them for an inertial set (seed_tracers(tau=...)): particle velocity, response time
SORT_BIN_CELLS = 32      # cells per bin along x of the device sort (include/fs_hip.h FS_TRACER_SORT_BIN_CELLS): one 128-byte line of an f32 row


def _as_seeds(seeds):
    seeds = np.asarray(seeds, np.float64)
    if seeds.ndim != 2 or seeds.shape[1] != 2:
        raise ValueError(f"seeds must have shape (N, 2), got {seeds.shape}")
    return seeds


def _inside(mask, seeds):
    X, Y = mask.shape
    x, y = seeds[:, 0], seeds[:, 1]
    return (x >= 0) & (x < X) & (y >= 0) & (y < Y)        # (False for NaN)


def fluid_only(mask, seeds):
    """The seeds that lie inside the domain in a FLUID or INFLOW cell (the filter the seed builders share) -> (kept seeds, dropped count)."""
    mask, seeds = np.asarray(mask), _as_seeds(seeds)
    ok = _inside(mask, seeds)
    cells = np.floor(seeds[ok]).astype(np.int64)
    m = mask[cells[:, 0], cells[:, 1]]
    ok[np.nonzero(ok)[0][(m != FLUID) & (m != INFLOW)]] = False
    return np.ascontiguousarray(seeds[ok]), int(len(seeds) - ok.sum())


def check_seeds(mask, seeds):
    """Seeds as a contiguous float64 (N, 2) array, N >= 1, every one inside the domain and in a FLUID or INFLOW cell; ValueError naming
    the first offender otherwise."""
    mask, seeds = np.asarray(mask), _as_seeds(seeds)
    if len(seeds) < 1:
        raise ValueError("a tracer set needs at least one seed")
    X, Y = mask.shape
    inside = _inside(mask, seeds)
    if not inside.all():
        k = int(np.nonzero(~inside)[0][0])
        raise ValueError(f"seed {k} at ({seeds[k, 0]!r}, {seeds[k, 1]!r}) lies outside the domain [0, {X}) x [0, {Y})")
    cells = np.floor(seeds).astype(np.int64)
    m = mask[cells[:, 0], cells[:, 1]]
    bad = (m != FLUID) & (m != INFLOW)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        kind = {WALL: "a wall", OUTFLOW: "an outflow"}.get(int(m[k]), f"a mask-{int(m[k])}")
        raise ValueError(f"seed {k} at ({seeds[k, 0]!r}, {seeds[k, 1]!r}) lies in {kind} cell ({cells[k, 0]}, {cells[k, 1]})")
    return np.ascontiguousarray(seeds)


def seed_line(p0, p1, n):
    """n points from p0 to p1 (both included; n == 1: the midpoint), float64 (n, 2), cell units."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    if p0.shape != (2,) or p1.shape != (2,):
        raise ValueError("p0 and p1 must be (x, y)")
    t = np.array([0.5]) if n == 1 else np.arange(n, dtype=np.float64) / np.float64(n - 1)
    return p0[None, :] + t[:, None] * (p1 - p0)[None, :]


def seed_grid(box, nx, ny):
    """nx x ny points at the centres of an even partition of box = (x0, y0, x1, y1), float64 (nx * ny, 2), x varying slowest."""
    x0, y0, x1, y1 = (float(b) for b in box)
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1:
        raise ValueError("nx and ny must be >= 1")
    xs = x0 + (np.arange(nx, dtype=np.float64) + 0.5) * ((x1 - x0) / nx)
    ys = y0 + (np.arange(ny, dtype=np.float64) + 0.5) * ((y1 - y0) / ny)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1)


def seed_random(mask, n, rng_seed=0):
    """n points, each uniform inside a FLUID cell drawn uniformly from all FLUID cells (np.random.default_rng(rng_seed): the same seeds for
    the same arguments), float64 (n, 2)."""
    mask = np.asarray(mask)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    cells = np.argwhere(mask == FLUID)
    if len(cells) == 0:
        raise ValueError("the mask has no fluid cell")
    rng = np.random.default_rng(rng_seed)
    pick = cells[rng.integers(0, len(cells), n)]
    cell = pick.astype(np.float64)
    # (a cell index plus a float64 just below 1 can round up to the next integer: keep the point inside its cell)
    return np.minimum(cell + rng.random((n, 2)), np.nextafter(cell + 1.0, 0.0))


def residence_time(age, dt):
    """Simulated time since a particle was seeded or last respawned: age * dt."""
    return np.asarray(age, np.float64) * np.float64(dt)


def sort_key(x, y, status, X, Y):
    """The key the device sort (FluidSimulator.sort_tracers, include/fs_hip.h fs_tracer_sort) orders the particle slots by, int64 (N,):
    floor(y) * NB + floor(x) // SORT_BIN_CELLS with NB = ceil(X / SORT_BIN_CELLS) for an alive particle inside [0, X) x [0, Y); Y * NB for
    one that is not alive, or outside the domain, or at a NaN position - these go last."""
    x, y, status = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(status)
    X, Y = int(X), int(Y)
    nb = -(-X // SORT_BIN_CELLS)
    ok = (status == FATE_ALIVE) & (x >= 0) & (x < X) & (y >= 0) & (y < Y)        # (False for NaN)
    key = np.full(x.shape, Y * nb, np.int64)
    key[ok] = np.floor(y[ok]).astype(np.int64) * nb + np.floor(x[ok]).astype(np.int64) // SORT_BIN_CELLS
    return key


def residence_map(count, age_sum, dt):
    """Mean simulated time the particles now in each cell have spent since their seed or last respawn: age_sum / count * dt, float64 in
    the shape of `count` (FluidSimulator.tracer_fields gives (X, Y)), NaN where count == 0."""
    count, age_sum = np.asarray(count), np.asarray(age_sum)
    if count.shape != age_sum.shape:
        raise ValueError(f"count {count.shape} and age_sum {age_sum.shape} differ in shape")
    out = np.full(count.shape, np.nan, np.float64)
    has = count > 0
    out[has] = age_sum[has].astype(np.float64) / count[has].astype(np.float64) * np.float64(dt)
    return out


def response(tau, dt):
    """alpha = 1 - exp(-dt / tau), the fraction of the way to the fluid's velocity (plus tau g) an inertial particle of response time tau
    covers in one step dt - the exact integral of dv/dt = (U - v) / tau + g with U frozen.  -expm1(-dt / tau) in float64: no
    cancellation for tau >> dt; 1 for tau == 0 (the particle takes the fluid's velocity at once) and wherever exp(-dt / tau) rounds
    away; in (0, 1] for every finite tau >= 0 the format can tell from infinity.  Scalar or array -> the same shape."""
    dt = float(dt)
    if not (dt > 0.0 and np.isfinite(dt)):
        raise ValueError("dt must be finite and > 0")
    t = np.asarray(tau, np.float64)
    if not (np.isfinite(t) & (t >= 0.0)).all():
        raise ValueError("tau must be finite and >= 0")
    out = np.ones(t.shape, np.float64)
    pos = t > 0.0
    with np.errstate(over="ignore", under="ignore"):
        out[pos] = -np.expm1(-np.float64(dt) / t[pos])
    if not (out > 0.0).all():
        raise ValueError("tau is too large for this dt: the response of one step rounds to 0")
    return out if out.ndim else np.float64(out)


def stokes_number(tau, speed, length):
    """St = tau * speed / length: the response time over the flow's time scale (length / speed, e.g. body size / inflow speed, in the
    solver's units).  St << 1: the particle follows the fluid; St >> 1: it goes straight."""
    length = np.asarray(length, np.float64)
    if (length <= 0).any():
        raise ValueError("length must be > 0")
    return np.asarray(tau, np.float64) * np.asarray(speed, np.float64) / length


def concentration(occupancy, samples):
    """Mean particles per cell over the sampled steps: occupancy / samples (FluidSimulator.tracer_accumulation), float64."""
    samples = int(samples)
    if samples < 1:
        raise ValueError("no samples")
    return np.asarray(occupancy).astype(np.float64) / np.float64(samples)


class TracerAccumulation(Rider):
    """The accumulated occupancy of a FluidSimulator's tracer set (accumulate_tracers): the device accumulator and its parameters.  It
    rides inside its Tracers, which issues its launch behind the advance and writes its part of a checkpoint."""

    def __init__(self, accum, every, start_step, dev=None):
        self.accum, self.every, self.start_step, self.dev = accum, int(every), int(start_step), dev
        self.set = getattr(accum, "set", None)        # (the device set the planes are attached to)

    @property
    def token(self):
        return ("tracer_accum", self.accum.serial)

    def free(self):
        self.dev.tracer_accum_free(self.set)

    @staticmethod
    def held(z):
        """-> (every, start), or None."""
        return (int(z["tracer.accum.every"]), int(z["tracer.accum.start"])) if "tracer.accum.occupancy" in z else None

    def restore(self, z):
        """(After Tracers.restore, which sets the launch count the phase hangs on.)  A checkpoint without an accumulation: nothing."""
        if "tracer.accum.occupancy" not in z:
            return 0
        self.dev.tracer_accum_write(self.set, z["tracer.accum.occupancy"], z["tracer.accum.age_sum"], int(z["tracer.accum.steps"]),
                                    int(z["tracer.accum.samples"]))
        return int(z["tracer.accum.samples"])


class Tracers(Rider):
    """One tracer set of a FluidSimulator (seed_tracers): the device set and its parameters; `issued`: advances issued since seed_tracers
    (what sort_every counts), `sorts`: device sorts so far."""

    def __init__(self, dev, set_, seeds, respawn, max_age, sort_every=0, tau=None, gravity=(0.0, 0.0), deposits=False):
        self.dev, self.set, self.seeds, self.respawn, self.max_age = dev, set_, seeds, bool(respawn), int(max_age)
        self.sort_every, self.issued, self.sorts, self.sorted_at = int(sort_every), 0, 0, 0
        self.tau, self.gravity, self.deposits = tau, tuple(gravity), bool(deposits)      # tau: float64 (N,) - an inertial set - or None
        self.accumulation = None       # TracerAccumulation while accumulate_tracers() is on

    def to_next_sort(self):
        """Steps until the next scheduled sort (>= 1), or None without a schedule."""
        return self.sort_every - self.issued % self.sort_every if self.sort_every > 0 else None

    def due(self):
        """The schedule asks for a sort now: `issued` is a positive multiple of sort_every that has not been sorted at."""
        return self.sort_every > 0 and self.issued % self.sort_every == 0 and self.sorted_at != self.issued

    def sort(self):
        self.dev.tracer_sort(self.set)
        self.sorts += 1
        self.sorted_at = self.issued

    @property
    def token(self):
        return ("tracer", self.set.serial)

    def tokens(self):
        return (self.token,) if self.accumulation is None else (self.token, self.accumulation.token)

    def launch(self, sim):
        self.dev.tracer_advance(self.set, sim._solver.dt / sim._solver.dx, sim._solver.get_fields()[0])
        self.issued += 1
        if self.accumulation is not None:
            self.dev.tracer_accum_add(self.set)      # (behind the advance: gated on the device from the set's launch counter)

    def next_cut(self):
        return self.to_next_sort()

    def between_chunks(self):
        """The scheduled device sort (seed_tracers(sort_every=K)): after every K-th step."""
        if self.due():
            self.sort()

    def free(self):
        if self.accumulation is not None:
            self.accumulation.free()
            self.accumulation = None
        self.dev.tracer_free(self.set)

    def checkpoint(self):
        """A passive set: the keys of tracer_read and respawn, max_age - the format it always had; an inertial set adds u, w, tau, gravity
        and, when it has them, the deposit plane; an attached accumulation adds its planes, counters and parameters."""
        arrays = {f"tracer.{k}": np.asarray(a) for k, a in self.dev.tracer_read(self.set).items()}
        arrays.update({"tracer.respawn": np.array(self.respawn), "tracer.max_age": np.array(self.max_age)})
        if self.tau is not None:
            u, w = self.dev.tracer_read_vel(self.set)
            arrays.update({"tracer.u": u, "tracer.w": w, "tracer.tau": np.asarray(self.tau, np.float64),
                           "tracer.gravity": np.array(self.gravity, np.float64)})
            if self.deposits:
                arrays["tracer.deposits"] = self.dev.tracer_deposits(self.set)
        acc = self.accumulation
        if acc is not None:
            occ, age, launches, samples = self.dev.tracer_accum_read(self.set)
            arrays.update({"tracer.accum.occupancy": occ, "tracer.accum.age_sum": age, "tracer.accum.steps": np.array(launches),
                           "tracer.accum.samples": np.array(samples), "tracer.accum.every": np.array(acc.every),
                           "tracer.accum.start": np.array(acc.start_step)})
        return arrays

    @staticmethod
    def held(z):
        """-> (respawn, max_age, N) of the set, or None."""
        return (bool(z["tracer.respawn"]), int(z["tracer.max_age"]), len(z["tracer.x"])) if "tracer.x" in z else None

    @staticmethod
    def held_inertial(z):
        """What the set holds beyond a passive one's: {"tau": (N,) array or None, "gravity": (gx, gy), "deposits": bool, "accumulate":
        TracerAccumulation.held(z)}, or None without a set."""
        if "tracer.x" not in z:
            return None
        inertial = "tracer.tau" in z
        return {"tau": np.asarray(z["tracer.tau"], np.float64) if inertial else None,
                "gravity": tuple(float(g) for g in z["tracer.gravity"]) if inertial else (0.0, 0.0),
                "deposits": "tracer.deposits" in z, "accumulate": TracerAccumulation.held(z)}

    def restore(self, z):
        """The state of the set itself, in seed order -> its particles.  An accumulation is attached and restored after this
        (TracerAccumulation.restore)."""
        self.dev.tracer_write(self.set, {k: z[f"tracer.{k}"] for k in KEYS})
        if self.tau is not None:
            self.dev.tracer_write_vel(self.set, z["tracer.u"], z["tracer.w"])
            if self.deposits:
                self.dev.tracer_deposits_write(self.set, z["tracer.deposits"])
        return len(z["tracer.x"])
