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


def strain_expectation(m, X, Y, a, h, N):
    """-> (interior nodes of the flow map m whose path and whose neighbours' paths stay a cell from the edge, the analytic lam = g^(2N)).
    One midpoint step of size h multiplies x - xc by 1 + q + q^2 / 2 and y - yc by 1 - q + q^2 / 2, q = a h: the larger factor is
    g = 1 + |q| + q^2 / 2, and no coordinate grows by more than g^N."""
    q = a * abs(h)
    g = 1.0 + q + 0.5 * q * q
    grow = g ** N
    inner = ((np.abs(m["x0"] - X / 2.0) + 1.0) * grow <= X / 2.0 - 1.0) & ((np.abs(m["y0"] - Y / 2.0) + 1.0) * grow <= Y / 2.0 - 1.0)
    return inner, g ** (2 * N), g
