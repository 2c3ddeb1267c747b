"""Harmonic flow modes without a GPU: the fit of fs/modes.py on synthetic signals with the phasors of the device's recurrence (one and two
frequencies, runs that hold no whole number of periods, 1e5 samples), the reconstruction weights against the host reconstruction, the
refusals, and the host logic of FluidSimulator.start_modes / modes / mode_fields / reset_modes / stop_modes on the NumPy stand-in device
(tests/modes_standin.py): launch and token order beside the other riders, checkpoint and restore, the capture rules.

Bounds of the recovery tests (set by the issue that introduced the feature): f64 samples 1e-11 absolute on coefficients of order 1; samples
rounded to f32 1e-6 max|x| - the normalised Gram matrix of these cases has a condition number <= 2.6 and f32 storage rounds each sample by
<= 6e-8 |x|."""
import numpy as np
import pytest
from modes_ref import State, accumulate_ref, rotate, run_reference, sampling_launches

F64_BOUND = 1e-11
F32_BOUND = 1e-6


def _phasor_series(n, cd, sd):
    """(n, K) c and s of samples 0 .. n - 1 by the device's recurrence."""
    c, s = np.ones(len(cd)), np.zeros(len(cd))
    cs, ss = np.empty((n, len(cd))), np.empty((n, len(cd)))
    for m in range(n):
        cs[m], ss[m] = c, s
        c, s = rotate(c, s, cd, sd)
    return cs, ss, c, s


def _accumulate_series(x, cd, sd):
    """Planes of ONE field and the scalars for the samples x (n, cells) -> (sums (B, cells), scalars).  Matrix products instead of the
    device's sample-by-sample sums: the same numbers up to the rounding of a different summation order, far inside the bounds."""
    n, K = len(x), len(cd)
    cs, ss, c, s = _phasor_series(n, cd, sd)
    basis = np.empty((n, 1 + 2 * K))
    basis[:, 0] = 1.0
    basis[:, 1::2], basis[:, 2::2] = cs, ss
    gram = basis.T @ basis
    ph = np.empty(2 * K)
    ph[0::2], ph[1::2] = c, s
    return basis.T @ x.astype(np.float64), np.concatenate([ph, gram[np.triu_indices(1 + 2 * K)]])


def _three(sums_one):
    """The planes of one field as the planes of (u, w, p): fit() takes all three."""
    return np.concatenate([sums_one, sums_one, sums_one])


def _signal(rng, n, deltas, cells=24):
    """x_m = m0 + sum_k A_k cos(m delta_k) + B_k sin(m delta_k), coefficients of order 1 per cell -> (x (n, cells), m0, A, B (K, cells))."""
    K = len(deltas)
    m0 = rng.uniform(-1.5, 1.5, cells)
    A, B = rng.uniform(-1.5, 1.5, (K, cells)), rng.uniform(-1.5, 1.5, (K, cells))
    m = np.arange(n)[:, None]
    x = np.broadcast_to(m0, (n, cells)).copy()
    for k, d in enumerate(deltas):
        x += A[k] * np.cos(m * d) + B[k] * np.sin(m * d)
    return x, m0, A, B


def _errors(fitted, m0, A, B):
    f = fitted["u"]
    return max(np.abs(f["mean"] - m0).max(), np.abs(f["cos"] - A).max(), np.abs(f["sin"] - B).max())


@pytest.mark.parametrize("n,per_period", [(20, 16.0), (37, 14.8), (100000, 333.3)])
def test_fit_recovers_a_synthetic_signal(n, per_period):
    from fs.modes import fit, gram_matrix
    rng = np.random.default_rng(n)
    delta = 2.0 * np.pi / per_period
    cd, sd = np.array([np.cos(delta)]), np.array([np.sin(delta)])
    x, m0, A, B = _signal(rng, n, [delta])
    sums, scalars = _accumulate_series(x, cd, sd)
    G = gram_matrix(scalars, 1)
    d = np.sqrt(np.diag(G))
    assert np.linalg.cond(G / np.outer(d, d)) <= 2.6
    out = fit(_three(sums), scalars, 1)
    e64 = _errors(out, m0, A, B)
    print(f"n {n}: f64 error {e64:.3g}")
    assert e64 <= F64_BOUND
    f = out["u"]
    assert np.allclose(f["amplitude"], np.hypot(A, B), atol=1e-10, rtol=0) and f["phase"].shape == (1, 24)
    # amplitude * cos(theta - phase) is the same signal
    assert np.allclose(f["amplitude"] * np.cos(0.7 - f["phase"]), A * np.cos(0.7) + B * np.sin(0.7), atol=1e-10, rtol=0)
    x32 = x.astype(np.float32)
    sums32, scalars32 = _accumulate_series(x32, cd, sd)
    e32 = _errors(fit(_three(sums32), scalars32, 1), m0, A, B)
    print(f"n {n}: f32 error {e32:.3g}, bound {F32_BOUND * np.abs(x).max():.3g}")
    assert e32 <= F32_BOUND * np.abs(x).max()


def test_two_frequencies_need_the_joint_fit():
    """f and 2 f over 2.3 periods of f: the two are far from orthogonal on such a window."""
    from fs.modes import fit
    rng = np.random.default_rng(5)
    per_period, n = 16.0, 37            # 37 / 16 = 2.3 periods
    d1 = 2.0 * np.pi / per_period
    deltas = np.array([d1, 2.0 * d1])
    x, m0, A, B = _signal(rng, n, deltas)
    for xs, bound in ((x, F64_BOUND), (x.astype(np.float32), F32_BOUND * np.abs(x).max())):
        sums, scalars = _accumulate_series(xs, np.cos(deltas), np.sin(deltas))
        assert _errors(fit(_three(sums), scalars, 2), m0, A, B) <= bound
    for k in (0, 1):      # each frequency fitted alone takes up part of the other
        sums, scalars = _accumulate_series(x, np.cos(deltas[k:k + 1]), np.sin(deltas[k:k + 1]))
        alone = fit(_three(sums), scalars, 1)
        assert _errors(alone, m0, A[k:k + 1], B[k:k + 1]) > 1e-3


def test_reconstruct_weights_equal_the_host_reconstruction():
    from fs.modes import fit, reconstruct, reconstruct_weights
    rng = np.random.default_rng(8)
    deltas = np.array([0.37, 0.91])
    x, m0, A, B = _signal(rng, 53, deltas)
    sums, scalars = _accumulate_series(x, np.cos(deltas), np.sin(deltas))
    planes = np.concatenate([sums, 2.0 * sums, -sums])
    out = fit(planes, scalars, 2)
    for phases in ([0.3, None], [None, 2.1], [1.0, -0.4], None):
        w = reconstruct_weights(scalars, 2, phases)
        assert w.shape == (5,)
        rec = reconstruct(out, phases)
        for a, name in enumerate(("u", "w", "p")):
            got = sum(w[j] * planes[a * 5 + j] for j in range(5))
            assert np.abs(got - rec[name]).max() <= 1e-12, (phases, name)
    assert np.abs(reconstruct(out, None)["u"] - m0).max() <= 1e-11
    assert np.abs(reconstruct(out, [0.3, None])["u"] - (m0 + A[0] * np.cos(0.3) + B[0] * np.sin(0.3))).max() <= 1e-11
    with pytest.raises(ValueError):
        reconstruct_weights(scalars, 2, [0.1])


def test_refusals():
    from fs.modes import MODES_MAX_FREQ, fit, gram_matrix, phasor_steps
    assert MODES_MAX_FREQ == 4
    dt = 0.01
    cd, sd = phasor_steps([2.0, 3.0], 4, dt)
    assert np.array_equal(cd, np.cos(2.0 * np.pi * np.array([2.0, 3.0]) * 4 * dt)) and np.array_equal(sd, np.sin(2.0 * np.pi * np.array([2.0, 3.0]) * 4 * dt))
    phasor_steps([12.4], 4, dt)                     # f every dt = 0.496
    for bad in ([12.5], [1.0, 30.0]):               # = 0.5; one of two beyond
        with pytest.raises(ValueError):
            phasor_steps(bad, 4, dt)
    for bad in ([1.0, 2.0, 3.0, 4.0, 5.0], [], [1.0, 1.0], [0.0], [-1.0], [np.nan]):
        with pytest.raises(ValueError):
            phasor_steps(bad, 1, dt)
    # fewer samples than unknowns
    deltas = np.array([0.4])
    x = np.random.default_rng(0).standard_normal((2, 5))
    sums, scalars = _accumulate_series(x, np.cos(deltas), np.sin(deltas))
    with pytest.raises(ValueError):
        fit(_three(sums), scalars, 1)
    with pytest.raises(ValueError):
        gram_matrix(scalars[:-1], 1)
    with pytest.raises(ValueError):
        fit(sums, scalars, 1)                       # planes of one field only


def test_reference_state_matches_the_series():
    """tests/modes_ref.py sample by sample against the matrix form above, within rounding; Gram[0][0] counts the samples."""
    from fs.modes import gram_matrix, samples_of
    rng = np.random.default_rng(2)
    deltas = np.array([0.5, 1.3, 2.9])
    n, shape = 25, (4, 3)
    st = State(shape, np.cos(deltas), np.sin(deltas))
    mask = np.zeros(shape, np.uint8)
    mask[1, 1] = 1
    xs = rng.standard_normal((n,) + shape).astype(np.float32)
    for m in range(n):
        accumulate_ref(st, np.stack([xs[m], -xs[m]], axis=-1), 2 * xs[m], mask)
    sums, scalars = _accumulate_series(xs.reshape(n, -1), np.cos(deltas), np.sin(deltas))
    assert np.array_equal(st.scalars()[:6], scalars[:6])
    assert np.allclose(st.scalars(), scalars, rtol=0, atol=1e-12)
    assert samples_of(st.scalars(), 3) == n == st.samples and gram_matrix(st.scalars(), 3)[0, 0] == n
    fluid = mask != 1
    assert np.allclose(st.sums[:7][:, fluid], sums.reshape(7, *shape)[:, fluid], rtol=0, atol=1e-12)
    assert np.array_equal(st.sums[7:14], -st.sums[:7]) and np.all(st.sums[:, 1, 1] == 0.0)


# ---- host logic on the NumPy stand-in ------------------------------------------------------------------------------------------------
FNAME = "traj_bc3_upwind_vc0.npz"
FREQS = [3.0, 7.5]


@pytest.fixture(scope="module")
def standin():
    import fs
    from modes_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from modes_standin import make_sim
    return make_sim(FNAME)


@pytest.mark.parametrize("every,start", [(1, 0), (3, 4)])
def test_modes_follow_the_steps(every, start, standin):
    from fs.modes import fit, gram_matrix
    (a, _), (b, _) = _sim(), _sim()
    a.start_modes(FREQS, every=every, start_step=start)
    a.run(17)
    a.run(12)
    st = run_reference(b, 29, FREQS, every, start)
    sums, scalars, launches, samples = a._dev.modes_read(a._moder.modes)
    assert (launches, samples) == (29, len(sampling_launches(29, every, start))) == (st.launches, st.samples)
    assert np.array_equal(sums, st.sums) and np.array_equal(scalars, st.scalars())
    mask = np.asarray(a._solver._bc.mask)
    assert np.all(sums[:, mask == 1] == 0.0) and np.abs(sums[4]).max() > 0.0
    out = a.modes()
    exp = fit(st.sums, st.scalars(), 2, mask)
    assert set(out) == {"frequencies", "samples", "steps", "sums", "gram", "mask", "u", "w", "p"}
    assert out["samples"] == samples and out["steps"] == 29 and out["frequencies"].tolist() == FREQS
    assert np.array_equal(out["gram"], gram_matrix(scalars, 2))
    for name in ("u", "w", "p"):
        for k, e in exp[name].items():
            assert np.array_equal(out[name][k], e), (name, k)
            assert np.all(out[name][k][..., mask == 1] == 0.0)
    fa, fb = a.field_to_numpy(), b.field_to_numpy()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa), "the modes changed the trajectory"


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    fluid = np.argwhere(np.asarray(sim._solver._bc.mask) == 0)
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_modes([3.0])
    sim.start_averaging(every=3)
    sim.record_history([tuple(fluid[len(fluid) // 2])], box, every=1, capacity=20)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["history_record", "mean_accumulate", "modes_accumulate", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4
    assert sig[-4:] == (("history", sim._recorder.hist.serial), ("mean", sim._averager.mean.serial), ("modes", sim._moder.modes.serial),
                        ("loads", sim._tracker.loads.serial))
    assert sim._moder.token == ("modes", sim._moder.modes.serial)
    assert not sim._moder.replaces_attached and sim._moder.stop_in_capture and not sim._moder.keeps_last
    assert sim._moder.room() is None and sim._moder.next_cut() is None          # (run() is not cut into chunks by it)


def test_start_reset_stop_and_refusals(standin):
    sim, _ = _sim()
    with pytest.raises(RuntimeError):
        sim.modes()
    with pytest.raises(RuntimeError):
        sim.mode_fields()
    dt = sim._solver.dt
    with pytest.raises(ValueError):
        sim.start_modes([0.5 / (2 * dt)], every=2)          # Nyquist: f every dt = 0.5
    with pytest.raises(ValueError):
        sim.start_modes([1.0, 2.0, 3.0, 4.0, 5.0])
    for bad in (dict(every=0), dict(start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_modes([1.0], **bad)
    assert sim._moder is None
    sim.start_modes([3.0], every=2, start_step=1)
    with pytest.raises(RuntimeError):
        sim.start_modes([3.0])                               # a second attach without stop_modes()
    sim.run(4)
    with pytest.raises(RuntimeError):
        sim.modes()                                          # 1 sample, 3 unknowns
    with pytest.raises(RuntimeError):
        sim.mode_fields()
    sim.run(5)
    assert (sim.modes()["samples"], sim.modes()["steps"]) == (4, 9)
    sim.reset_modes()
    sums, scalars, launches, samples = sim._dev.modes_read(sim._moder.modes)
    assert not sums.any() and (launches, samples) == (9, 0) and scalars.tolist() == [1.0, 0.0] + [0.0] * 6
    sim.run(2)                                               # steps 10, 11: the phase of every / start runs on - step 11 samples
    assert sim._dev.modes_read(sim._moder.modes)[2:] == (11, 1)
    tok = sim._moder.token
    sim.stop_modes()
    assert sim._moder is None and tok not in sim._signature()
    sim.stop_modes()                                         # (a second stop is a no-op)
    with pytest.raises(RuntimeError):
        sim.reset_modes()


def test_mode_fields_equal_the_host_reconstruction(standin):
    from fs.modes import reconstruct
    sim, _ = _sim()
    sim.start_modes(FREQS, every=2)
    sim.run(31)
    out = sim.modes()
    mask = out["mask"]
    for phase, frequency in ((None, 0), (0.8, 0), (-2.0, 1)):
        v, p = sim.mode_fields(phase, frequency)
        phases = None if phase is None else [phase if k == frequency else None for k in range(2)]
        rec = reconstruct(out, phases)
        scale = max(1.0, np.abs(out["sums"]).max())
        for got, name in ((v.to_numpy()[..., 0], "u"), (v.to_numpy()[..., 1], "w"), (p.to_numpy(), "p")):
            assert got.dtype == np.float32 and np.all(got[mask == 1] == 0.0)
            # the device sums weight * plane, the host solves per cell: equal up to the rounding of the B terms and of f32 storage
            assert np.abs(got - rec[name]).max() <= 1e-6 * max(1.0, np.abs(rec[name]).max()) + 1e-12 * scale, (phase, name)
    with pytest.raises(ValueError):
        sim.mode_fields(0.0, 2)


def test_checkpoint_and_restore(standin):
    (a, _), (b, _) = _sim(), _sim()
    a.start_modes(FREQS, every=3, start_step=2)
    a.run(20)
    z = a._moder.checkpoint()
    assert set(z) == {"modes.sums", "modes.scalars", "modes.launches", "modes.samples", "modes.frequencies", "modes.every", "modes.start"}
    assert (int(z["modes.launches"]), int(z["modes.samples"]), int(z["modes.every"]), int(z["modes.start"])) == (20, 6, 3, 2)
    assert z["modes.frequencies"].tolist() == FREQS
    b.run(20)
    b.start_modes(FREQS, every=3, start_step=2)
    assert b._moder.restore(z) == b._dev.modes_read_scalars(b._moder.modes)[3] == 6          # (-> the samples taken over: the CLI's "samples so far")
    a.run(11)
    b.run(11)
    ra, rb = a._dev.modes_read(a._moder.modes), b._dev.modes_read(b._moder.modes)
    assert ra[2:] == rb[2:] == (31, 9)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    with pytest.raises(ValueError):
        b._dev.modes_write(b._moder.modes, z["modes.sums"][:, :-1], z["modes.scalars"], 20, 6)
    with pytest.raises(ValueError):
        b._dev.modes_write(b._moder.modes, z["modes.sums"], z["modes.scalars"][:-1], 20, 6)
    with pytest.raises(ValueError):
        b._dev.modes_write(b._moder.modes, z["modes.sums"], z["modes.scalars"], 3, 4)


def test_stop_inside_and_outside_a_capture(standin):
    from fs import _lib
    sim, _ = _sim()
    sim.start_modes([3.0])
    sim.run(5)
    dev = sim._dev
    dev.capturing = True
    try:
        for call in (sim.modes, sim.reset_modes, sim.mode_fields):
            with pytest.raises(_lib.FsError):
                call()
        sim.stop_modes()                       # allowed: the device memory goes when the capture ends
        assert sim._moder is None
        with pytest.raises(RuntimeError):
            sim.start_modes([3.0])
    finally:
        dev.capturing = False
    sim.start_modes([3.0])
    sim.run(3)
    assert sim._dev.modes_read(sim._moder.modes)[2:] == (3, 3)
    sim.stop_modes()
    assert sim._moder is None
