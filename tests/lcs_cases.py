"""Scenes, analytic rings and the simulator factory shared by tests/test_lcs_cpu.py (NumPy stand-in) and tests/test_gpu_lcs.py: a simulator on
an arbitrary mask whose POD ring is installed with pod_set, so that most cases need no time stepping."""
import numpy as np

DX = 1.0 / 16          # dt / dx = 0.5 and every product with it exact in binary: the step size of the exactness cases is a dyadic fraction
DT = 1.0 / 32


def make_sim(mask, const=None, dt=DT, dx=DX):
    """A FluidSimulator (upwind MAC solver, two red-black iterations - any width) on `mask`, on the device class and dtype fs.runtime.init
    chose."""
    import fs
    mask = np.array(mask, np.uint8)
    const = np.zeros(mask.shape + (2,), np.float32) if const is None else np.array(const, np.float32)
    bc = fs.BoundaryCondition(const, mask)
    pu = fs.RedBlackSorPressureUpdater(bc, dt, dx, 1.3, 2)
    return fs.FluidSimulator(fs.MacSolver(bc, pu, fs.advect_upwind, dt, dx, 1.0e3, None))


def install_ring(sim, slots, every=1, samples=None):
    """start_pod(M, every) with `slots` (M, 3, X, Y) as its ring, `samples` samples taken so far (default M: a full ring in slot order)."""
    M = len(slots)
    samples = M if samples is None else samples
    sim.start_pod(M, every=every)
    sim._dev.pod_set(sim._podr.pod, np.asarray(slots).astype(sim._dev.dtype), samples * every, samples)


def uniform_rings(X=64, Y=16, M=5, c=0.25):
    """Snapshot m is the uniform flow (m c, 0): linear in time, so the midpoint rule integrates it exactly."""
    slots = np.zeros((M, 3, X, Y), np.float64)
    for m in range(M):
        slots[m, 0] = m * c
    return np.zeros((X, Y), np.uint8), slots


def strain_rings(X=64, Y=32, M=5, a=0.1):
    """Every snapshot the steady strain u = a (x - xc), w = -a (y - yc) about the centre of the grid, at the cell centres."""
    x, y = np.meshgrid(np.arange(X) + 0.5, np.arange(Y) + 0.5, indexing="ij")
    slots = np.zeros((M, 3, X, Y), np.float64)
    slots[:, 0] = a * (x - X / 2.0)
    slots[:, 1] = -a * (y - Y / 2.0)
    return np.zeros((X, Y), np.uint8), slots


# ---- boxed, refined lattices on a grid wider than one pitch unit ---------------------------------------------------------------------------
LATTICE_DT, LATTICE_DX = 0.5, 0.1          # every = 1: a sub-step is 5 / S cells per unit velocity
# (box, refine): 376 x 120 = 45,120 nodes, 177 workgroups of 256, the last of 64 lanes, the wall block inside the box;
#                264 x 140 = 36,960 nodes, 145 workgroups, the last of 96 lanes, the box one column short of the outflow
LATTICE_CASES = (((11, 5, 58, 20), 8), ((3, 2, 69, 37), 4))
LATTICE_SUBSTEPS = (16, 5)
LATTICE_RINGS = {"full": dict(samples=4, window={}), "wrapped": dict(samples=6, window=dict(first=1, last=-1))}


def lattice_rings(dtype=np.float32, X=70, Y=40, M=4):
    """A smooth, unsteady, sheared flow on a (70, 40) grid (row pitch 128: two 64-column units): walls in rows 0 and Y - 1 and a block at
    i in [30, 36), j in [12, 20); column 0 inflow and column X - 1 outflow between the walls.  Snapshot m at the cell centres x = i + 0.5,
    y = j + 0.5, a = 0.6 + 0.3 m:
        u = a (1 + 0.4 sin(2 pi y / 40 + 0.7 m)) + 0.5 cos(2 pi x / 23) sin(2 pi y / 17)
        w = 0.45 sin(2 pi x / 19 + 0.3 m) cos(2 pi y / 29)
    cast to `dtype`, 0 on wall cells, p = 0.  Unlike lcs_ref.fate_rings nothing is piecewise constant: every bilinear weight and every
    corner index matters.  -> (mask, slots (M, 3, X, Y))."""
    mask = np.zeros((X, Y), np.uint8)
    mask[0, 1:Y - 1] = 2
    mask[X - 1, 1:Y - 1] = 3
    mask[:, 0] = mask[:, Y - 1] = 1
    mask[30:36, 12:20] = 1
    x, y = np.meshgrid(np.arange(X) + 0.5, np.arange(Y) + 0.5, indexing="ij")
    slots = np.zeros((M, 3, X, Y), dtype)
    for m in range(M):
        a = 0.6 + 0.3 * m
        slots[m, 0] = a * (1.0 + 0.4 * np.sin(2.0 * np.pi * y / 40.0 + 0.7 * m)) + 0.5 * np.cos(2.0 * np.pi * x / 23.0) * np.sin(2.0 * np.pi * y / 17.0)
        slots[m, 1] = 0.45 * np.sin(2.0 * np.pi * x / 19.0 + 0.3 * m) * np.cos(2.0 * np.pi * y / 29.0)
    slots[:, :, mask == 1] = 0
    return mask, slots


def lattice_geometry(box, refine, wg=256):
    """-> (nodes across, nodes down, workgroups of `wg` lanes, lanes of the last one)."""
    nx, ny = refine * (box[2] - box[0]), refine * (box[3] - box[1])
    groups = -(-nx * ny // wg)
    return nx, ny, groups, nx * ny - (groups - 1) * wg


def missing_neighbours(status, unseeded=4):
    """Per side (lower a, upper a, lower b, upper b): the nodes whose lattice neighbour on that side is absent - outside the lattice or
    UNSEEDED - which is where k_flowmap_cauchy_green takes a one-sided difference."""
    there = np.asarray(status) != unseeded
    pad = np.pad(there, 1, constant_values=False)
    return ~pad[:-2, 1:-1], ~pad[2:, 1:-1], ~pad[1:-1, :-2], ~pad[1:-1, 2:]


def strain_expectation(m, X, Y, a, h, N):
    """-> (interior nodes of the flow map m whose path and whose neighbours' paths stay a cell from the edge, the analytic lam = g^(2N)).
    One midpoint step of size h multiplies x - xc by 1 + q + q^2 / 2 and y - yc by 1 - q + q^2 / 2, q = a h: the larger factor is
    g = 1 + |q| + q^2 / 2, and no coordinate grows by more than g^N."""
    q = a * abs(h)
    g = 1.0 + q + 0.5 * q * q
    grow = g ** N
    inner = ((np.abs(m["x0"] - X / 2.0) + 1.0) * grow <= X / 2.0 - 1.0) & ((np.abs(m["y0"] - Y / 2.0) + 1.0) * grow <= Y / 2.0 - 1.0)
    return inner, g ** (2 * N), g
