"""Snapshot POD without a GPU: the host algebra of fs/pod.py (decompose) on synthetic float64 snapshots - a travelling wave, the same wave on
a constant mean, a spectrum that falls over four decades, a duplicated snapshot - and the host logic of FluidSimulator.start_pod / pod /
pod_fields / pod_snapshot / reset_pod / stop_pod on the NumPy stand-in device (tests/pod_standin.py): launch and token order beside the other
riders, the ring order after a wrap, checkpoint and restore, the capture rules.

Bounds (set by the issue that introduced the feature): the wave's two modes hold all the energy to 1e-12 and are equal to 1e-12 lambda_0;
modes with lambda_k / lambda_0 >= 1e-6 are orthonormal to 1e-10 (eps * cond: eps / 1e-6 is about 2e-10 at worst, the cases sit far below);
snapshots are reproduced to 1e-10 max|x|.  The falling spectrum spans lambda_k / lambda_0 down to 1e-4, where eps * cond is 2e-12: a case
at 1e-6 itself would sit AT the bound (measured there: 1.2e-10), not below it."""
import numpy as np
import pytest
from pod_ref import State, capture_ref, combine_ref, gram_ref


def _wave(n=16, cells=64, mean=(0.0, 0.0)):
    """u = cos(kx - wt), w = sin(kx - wt) over one spatial period, n samples over one full period in time -> (n, 2, cells)."""
    x = 2.0 * np.pi * np.arange(cells) / cells
    t = 2.0 * np.pi * np.arange(n) / n
    ph = x[None, :] - t[:, None]
    return np.stack([np.cos(ph) + mean[0], np.sin(ph) + mean[1]], axis=1)


def _modes(out, snaps):
    """(r, 2 cells): weights @ snapshots."""
    return out["weights"] @ snaps.reshape(len(snaps), -1)


def test_travelling_wave_gives_two_equal_modes_in_quadrature():
    from fs.pod import decompose
    snaps = _wave()
    for subtract_mean in (True, False):
        out = decompose(gram_ref(snaps), subtract_mean)
        lam = out["energies"]
        assert len(lam) == 2, lam          # (the rank rule drops the 14 others)
        assert out["fraction"][:2].sum() >= 1.0 - 1e-12
        assert abs(lam[0] - lam[1]) <= 1e-12 * lam[0]
        assert abs(lam[0] - 16 * 64 / 2.0) <= 1e-10 * lam[0]          # each carries half of sum |x|^2 = n cells
        a = out["coefficients"]
        assert a.shape == (16, 2) and out["weights"].shape == (2, 16)
        # quadrature: orthogonal, equal norms, and a_0^2 + a_1^2 the same at every sample (a circle in the phase plane)
        assert abs(a[:, 0] @ a[:, 1]) <= 1e-10 * lam[0]
        r2 = a[:, 0] ** 2 + a[:, 1] ** 2
        assert np.abs(r2 - lam[0] / 8.0).max() <= 1e-10 * lam[0]


def test_a_constant_mean_is_taken_out():
    from fs.pod import decompose
    base = decompose(gram_ref(_wave()), True)
    snaps = _wave(mean=(3.0, -1.5))
    out = decompose(gram_ref(snaps), True)
    # entries of G are sums of 128 terms of order 1 + |mean|^2 = 12.25: eigenvalues move by at most n * 128 eps * 12.25 * 64 = 4e-10 against
    # 512 - which is also what is left of the mean's direction, and may stand just above the rank rule's n eps lambda_0 = 1.8e-12
    assert np.abs(out["energies"][:2] - base["energies"]).max() <= 1e-11 * base["energies"][0]
    assert np.all(out["energies"][2:] <= 1e-11 * base["energies"][0]) and out["fraction"][:2].sum() >= 1.0 - 1e-12
    assert np.array_equal(out["mean_weights"], np.full(16, 1.0 / 16))
    raw = decompose(gram_ref(snaps), False)          # without the subtraction the mean is the most energetic "mode"
    assert len(raw["energies"]) == 3 and raw["energies"][0] > 10.0 * raw["energies"][1] and not raw["mean_weights"].any()


def _falling_spectrum(rng, n=12, cells=300, decades=2.0, mean=True):
    """n snapshots of 2 x cells values: n - 1 random orthogonal structures with amplitudes falling by `decades` decades (the eigenvalues by
    twice that), random temporal coefficients, plus a mean field of the norm of the first structure.  (The Gram matrix holds the RAW
    snapshots: what the subtraction leaves of a mean is of order eps n |mean|^2, so the eps * cond argument of the bound counts the mean's
    energy as well - a mean that outweighs lambda_0 by orders would take as many digits from the small modes.)"""
    q, _ = np.linalg.qr(rng.standard_normal((2 * cells, n - 1)))
    amp = 10.0 ** (-decades * np.arange(n - 1) / (n - 2))
    t, _ = np.linalg.qr(rng.standard_normal((n, n - 1)))
    x = (t * amp) @ q.T
    if mean:
        m = rng.standard_normal(2 * cells)
        x = x + m / np.linalg.norm(m)
    return x.reshape(n, 2, cells)


@pytest.mark.parametrize("case", ["wave", "wave_mean", "spectrum", "spectrum_raw"])
def test_modes_are_orthonormal_and_reproduce_the_snapshots(case):
    from fs.pod import decompose
    rng = np.random.default_rng(11)
    snaps = {"wave": lambda: _wave(), "wave_mean": lambda: _wave(mean=(3.0, -1.5)), "spectrum": lambda: _falling_spectrum(rng),
             "spectrum_raw": lambda: _falling_spectrum(rng, mean=False)}[case]()
    subtract = case != "spectrum_raw"
    out = decompose(gram_ref(snaps), subtract)
    lam = out["energies"]
    assert np.all(np.diff(lam) <= 0.0) and abs(out["fraction"].sum() - 1.0) <= 1e-12
    phi = _modes(out, snaps)
    big = lam / lam[0] >= 1e-6
    assert big.sum() >= 2
    gram_of_modes = phi[big] @ phi[big].T
    err = np.abs(gram_of_modes - np.eye(big.sum())).max()
    print(f"{case}: {len(lam)} modes, {big.sum()} with lambda / lambda_0 >= 1e-6, orthonormality error {err:.3g}")
    assert err <= 1e-10
    flat = snaps.reshape(len(snaps), -1)
    mean = out["mean_weights"] @ flat
    rec = mean + out["coefficients"] @ phi
    rerr = np.abs(rec - flat).max()
    print(f"{case}: reproduction error {rerr:.3g}, bound {1e-10 * np.abs(flat).max():.3g}")
    assert rerr <= 1e-10 * np.abs(flat).max()
    # the coefficient of mode k at sample m is the projection of the fluctuation on the mode
    assert np.abs((flat - mean) @ phi[big].T - out["coefficients"][:, big]).max() <= 1e-9 * np.sqrt(lam[0])


def test_the_rank_rule_drops_a_duplicated_snapshot():
    from fs.pod import decompose
    rng = np.random.default_rng(3)
    snaps = rng.standard_normal((6, 2, 50))
    assert len(decompose(gram_ref(snaps), False)["energies"]) == 6 and len(decompose(gram_ref(snaps), True)["energies"]) == 5
    snaps[5] = snaps[2]
    assert len(decompose(gram_ref(snaps), False)["energies"]) == 5 and len(decompose(gram_ref(snaps), True)["energies"]) == 4
    for bad in (np.zeros((1, 1)), np.zeros((3, 2)), np.full((2, 2), np.nan)):
        with pytest.raises(ValueError):
            decompose(bad)


def test_ring_order_and_sample_steps():
    from fs.pod import ring_slots, sample_steps
    st = State((3, 2), 4, np.float32)
    for samples in range(0, 12):
        assert ring_slots(samples, 4).tolist() == st.order(), samples
        st.samples += 1
    assert ring_slots(11, 4).tolist() == [3, 0, 1, 2]
    assert sample_steps(11, 4, 3, 2).tolist() == [2 + 3 * k for k in (8, 9, 10, 11)]
    assert sample_steps(3, 8, 1, 0).tolist() == [1, 2, 3] and sample_steps(2, 8, 2, 5, base=4).tolist() == [15, 17]


def test_reference_capture_and_combine():
    rng = np.random.default_rng(1)
    mask = np.zeros((5, 4), np.uint8)
    mask[2, 1] = 1
    st = State(mask.shape, 3, np.float32)
    fields = [(rng.standard_normal((5, 4, 2)).astype(np.float32), rng.standard_normal((5, 4)).astype(np.float32)) for _ in range(5)]
    for v, p in fields:
        capture_ref(st, v, p, mask)
    assert st.order() == [2, 0, 1] and st.resident == 3
    assert np.array_equal(st.slots[1, 0], np.where(mask == 1, 0, fields[4][0][..., 0])) and np.all(st.slots[:, :, 2, 1] == 0)
    v, p = combine_ref(st.slots, np.array([0.0, 1.0, 0.0]), mask, np.float32)
    assert np.array_equal(v[..., 1], st.slots[1, 1]) and np.array_equal(p, st.slots[1, 2])


# ---- host logic on the NumPy stand-in ------------------------------------------------------------------------------------------------
FNAME = "traj_bc3_upwind_vc0.npz"


@pytest.fixture(scope="module")
def standin():
    import fs
    from pod_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _sim():
    from pod_standin import make_sim
    return make_sim(FNAME)


def _snapshot_arrays(sim, m):
    v, p = sim.pod_snapshot(m)
    return v.to_numpy(), p.to_numpy()


@pytest.mark.parametrize("every,start,M,steps", [(1, 0, 8, 5), (3, 2, 4, 36)])
def test_pod_follows_the_steps(every, start, M, steps, standin):
    """A partly filled ring (5 of 8) and a wrapped one (11 samples in 4 slots): every resident sample equals the download after its step."""
    from pod_ref import sampling_launches
    (a, _), (b, _) = _sim(), _sim()
    a.start_pod(M, every=every, start_step=start)
    a.run(steps // 2)
    a.run(steps - steps // 2)
    want = sampling_launches(steps, every, start)
    downloads = {}
    for n in range(steps):
        b.step()
        if n in want:
            d = b.field_to_numpy()
            downloads[n + 1] = (d["v"].copy(), d["p"].copy())          # (the stand-in's downloads are views of its buffers)
    assert a._dev.pod_read(a._podr.pod) == (steps, len(want))
    out = a.pod()
    n_res = min(len(want), M)
    assert set(out) == {"gram", "energies", "fraction", "coefficients", "weights", "sample_steps", "samples", "steps"}
    assert (out["samples"], out["steps"]) == (len(want), steps) and out["gram"].shape == (n_res, n_res)
    assert out["sample_steps"].tolist() == [k + 1 for k in want][-n_res:]
    mask = np.asarray(a._solver._bc.mask)
    snaps = []
    for m, step in enumerate(out["sample_steps"]):
        v, p = _snapshot_arrays(a, m)
        ev, ep = downloads[int(step)]
        assert np.array_equal(v, np.where((mask == 1)[..., None], 0, ev)) and np.array_equal(p, np.where(mask == 1, 0, ep)), (m, step)
        snaps.append(np.stack([v[..., 0], v[..., 1]]))
    assert np.array_equal(_snapshot_arrays(a, -1)[0], snaps[-1].transpose(1, 2, 0))
    assert np.allclose(out["gram"], gram_ref(np.array(snaps)), rtol=1e-12, atol=0)          # chronological
    fa, fb = a.field_to_numpy(), b.field_to_numpy()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa), "the POD changed the trajectory"
    # the modes as fields: the restatement fed with the weights, in slot order
    slots = a._dev.pod_get(a._podr.pod)[0]
    assert out["weights"].shape == (len(out["energies"]), n_res)
    for k in (None, 0, len(out["energies"]) - 1):
        w = np.zeros(M)
        w[:n_res] = np.full(n_res, 1.0 / n_res) if k is None else out["weights"][k]
        v, p = a.pod_fields(k)
        ev, ep = combine_ref(slots, w, mask, np.float32)
        assert np.array_equal(v.to_numpy(), ev) and np.array_equal(p.to_numpy(), ep), k
    assert a.pod(n_modes=1)["coefficients"].shape == (n_res, 1) and a.pod(n_modes=1)["weights"].shape == (1, n_res)
    with pytest.raises(ValueError):
        a.pod_fields(len(out["energies"]))
    with pytest.raises(IndexError):
        a.pod_snapshot(n_res)


def test_launch_order_and_token_order(standin):
    from fs.boundary_condition import default_body_box
    sim, cfg = _sim()
    box = default_body_box(cfg["bc"], cfg["res"])
    base = sim._signature()
    # attached in another order than they ride
    sim.track_body(box, every=2, capacity=10)
    sim.start_pod(3)
    sim.start_modes([3.0])
    sim.start_averaging(every=3)
    dev = sim._dev
    dev._oplog = []
    try:
        sim.step()
        names = [op[1] for op in dev._oplog if op[0] == "k"]
    finally:
        dev._oplog = None
    riding = ["mean_accumulate", "modes_accumulate", "pod_launch", "loads_record"]
    assert names[-4:] == riding and not set(names[:-4]) & set(riding)
    sig = sim._signature()
    assert len(sig) == len(base) + 4
    assert sig[-4:] == (("mean", sim._averager.mean.serial), ("modes", sim._moder.modes.serial), ("pod", sim._podr.pod.serial),
                        ("loads", sim._tracker.loads.serial))
    po = sim._podr
    assert po.token == ("pod", po.pod.serial)
    assert not po.replaces_attached and po.stop_in_capture and not po.keeps_last
    assert po.room() is None and po.next_cut() is None          # (no ring to drain: run() is not cut into chunks by it)


def test_start_reset_stop_and_refusals(standin):
    from fs import _lib
    sim, _ = _sim()
    for call in (sim.pod, sim.pod_fields, sim.reset_pod, lambda: sim.pod_snapshot(0)):
        with pytest.raises(RuntimeError):
            call()
    for bad in (dict(snapshots=1), dict(snapshots=65), dict(snapshots=4, every=0), dict(snapshots=4, start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_pod(**bad)
    assert sim._podr is None
    sim.start_pod(4, every=2, start_step=1)
    with pytest.raises(RuntimeError):
        sim.start_pod(4)                                     # a second attach without stop_pod()
    sim.run(4)                                               # step 3 sampled
    with pytest.raises(RuntimeError):
        sim.pod()                                            # 1 sample
    with pytest.raises(RuntimeError):
        sim.pod_fields(0)
    sim.run(5)
    assert (sim.pod()["samples"], sim.pod()["steps"]) == (4, 9) and sim.pod()["sample_steps"].tolist() == [3, 5, 7, 9]
    sim.reset_pod()
    slots, launches, samples = sim._dev.pod_get(sim._podr.pod)
    assert not slots.any() and (launches, samples) == (9, 0)
    sim.run(4)                                               # steps 10 .. 13: the phase of every / start runs on - 11 and 13 sample
    assert sim._dev.pod_read(sim._podr.pod) == (13, 2) and sim.pod()["sample_steps"].tolist() == [11, 13]
    tok = sim._podr.token
    sim.stop_pod()
    assert sim._podr is None and tok not in sim._signature()
    sim.stop_pod()                                           # (a second stop is a no-op)
    with pytest.raises(RuntimeError):
        sim.reset_pod()
    # a slab context: refused with a message, as seed_tracers
    dev = sim._dev
    saved = dev.nranks
    dev.nranks = 2
    try:
        with pytest.raises(_lib.FsError, match="single-GPU"):
            sim.start_pod(4)
    finally:
        dev.nranks = saved
    assert sim._podr is None


def test_checkpoint_and_restore(standin):
    (a, _), (b, _) = _sim(), _sim()
    a.start_pod(4, every=3, start_step=2)
    a.run(10)
    a.reset_pod()                                            # (the samples before a reset stay in sample_steps' count)
    a.run(10)
    z = a._podr.checkpoint()
    assert set(z) == {"pod.slots", "pod.launches", "pod.samples", "pod.base", "pod.snapshots", "pod.every", "pod.start"}
    assert [int(z[k]) for k in ("pod.launches", "pod.samples", "pod.base", "pod.snapshots", "pod.every", "pod.start")] == [20, 4, 2, 4, 3, 2]
    assert z["pod.slots"].shape == (4, 3) + np.asarray(a._solver._bc.mask).shape and z["pod.slots"].dtype == np.float32
    b.run(20)
    b.start_pod(4, every=3, start_step=2)
    assert b._podr.restore(z) == b._dev.pod_read(b._podr.pod)[1] == 4          # (-> the samples taken over: the CLI's "samples so far")
    a.run(11)
    b.run(11)
    ra, rb = a._dev.pod_get(a._podr.pod), b._dev.pod_get(b._podr.pod)
    assert ra[1:] == rb[1:] == (31, 7)
    assert np.array_equal(ra[0], rb[0])
    pa, pb = a.pod(), b.pod()
    assert pa["sample_steps"].tolist() == pb["sample_steps"].tolist() == [20, 23, 26, 29]
    for k in ("gram", "energies", "coefficients", "weights"):
        assert np.array_equal(pa[k], pb[k]), k
    with pytest.raises(ValueError):
        b._dev.pod_set(b._podr.pod, z["pod.slots"][:, :, :-1], 20, 4)
    with pytest.raises(ValueError):
        b._dev.pod_set(b._podr.pod, z["pod.slots"], 3, 4)


def test_stop_inside_and_outside_a_capture(standin):
    from fs import _lib
    sim, _ = _sim()
    sim.start_pod(3)
    sim.run(5)
    dev = sim._dev
    dev.capturing = True
    try:
        for call in (sim.pod, sim.reset_pod, sim.pod_fields, lambda: sim.pod_snapshot(0)):
            with pytest.raises(_lib.FsError):
                call()
        sim.stop_pod()                         # allowed: the device memory goes when the capture ends
        assert sim._podr is None
        with pytest.raises(RuntimeError):
            sim.start_pod(3)
    finally:
        dev.capturing = False
    sim.start_pod(3)
    sim.run(3)
    assert sim._dev.pod_read(sim._podr.pod) == (3, 3)
    sim.stop_pod()
    assert sim._podr is None
