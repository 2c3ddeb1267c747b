"""Time averages without a GPU: the derivation of fs/averages.py against closed forms, the sampling rule against a plain loop,
recirculation_length on synthetic profiles, and the host logic of FluidSimulator.start_averaging / averages / reset_averages /
stop_averaging on the NumPy stand-in device (tests/mean_standin.py), including a gloo job of 2 - 4 slabs against one domain."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp
from mean_ref import accumulate_ref, new_sums, run_reference, sampling_launches


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- fs/averages.py ---------------------------------------------------------------------------------------------------------------
def test_derivation_against_closed_forms():
    """Per cell u = a + b sin(k t), w = c + d sin(k t), p = e + f cos(k t) sampled at N equidistant times over whole periods: means a, c, e;
    uu = b^2 / 2, ww = d^2 / 2, uw = b d / 2, p_rms = |f| / sqrt(2), tke = (b^2 + d^2) / 4.  Bound: every sum holds N terms of magnitude
    <= M^2 (M = the largest |a| + |b| of the cell) with a relative rounding error of 2^-53 each, the discrete orthogonality sums are exact
    in real arithmetic and sin / cos are good to an ulp: 8 N 2^-52 M^2 covers sums, divisions and the subtraction."""
    from fs.averages import derive_averages
    rng = np.random.default_rng(3)
    X, Y, N = 6, 5, 240
    a, b, c, d, e, f = (rng.uniform(-2.0, 2.0, (X, Y)) for _ in range(6))
    kper = rng.integers(1, 7, (X, Y))               # whole periods over the N samples, below N / 2
    mask = np.zeros((X, Y), np.uint8)
    mask[2, 3] = 1
    mask[0, 0] = 2
    sums = new_sums((X, Y))
    for j in range(N):
        ph = 2.0 * np.pi * kper * j / N
        v = np.stack([a + b * np.sin(ph), c + d * np.sin(ph)], axis=-1)
        accumulate_ref(sums, v, e + f * np.cos(ph), mask)
    out = derive_averages(sums, N, mask)
    M = np.abs(np.stack([a, b, c, d, e, f])).max(axis=0) * 2.0
    tol = 8 * N * 2.0 ** -52 * M * M
    fluid = mask != 1
    for key, exp in (("u", a), ("w", c), ("p", e), ("uu", b * b / 2), ("ww", d * d / 2), ("uw", b * d / 2), ("tke", (b * b + d * d) / 4)):
        assert np.all(np.abs(out[key] - exp)[fluid] <= tol[fluid]), key
    # p_rms: sqrt of a variance known to `tol` -> |sqrt(x + t) - sqrt(x)| <= t / sqrt(x) for x = f^2 / 2 (the cells have |f| well above 0)
    big = fluid & (np.abs(f) > 0.05)
    assert big.sum() > 10
    assert np.all(np.abs(out["p_rms"] - np.abs(f) / np.sqrt(2.0))[big] <= (tol / (np.abs(f) / np.sqrt(2.0)))[big])
    for key in ("u", "w", "p", "uu", "ww", "uw", "p_rms", "tke"):
        assert out[key].dtype == np.float64 and out[key].shape == (X, Y)
        assert out[key][2, 3] == 0.0, f"{key}: wall cell not 0"
    assert out["u"][0, 0] != 0.0        # (mask 2 is not a wall: averaged)


def test_derivation_order_and_clamp_under_cancellation():
    from fs.averages import derive_averages
    rng = np.random.default_rng(11)
    q = rng.uniform(0.05, 3.0, (64, 32))          # a constant (f64) pressure per cell: the true variance is 0, q * q is rounded
    v = np.stack([q, -q], axis=-1)
    sums = new_sums(q.shape)
    n = 7
    for _ in range(n):
        accumulate_ref(sums, v, q, np.zeros(q.shape, np.uint8))
    raw = sums[6] / np.float64(n) - (sums[2] / np.float64(n)) ** 2
    assert (raw < 0).any(), "no cell cancels below zero: the case is not covered"
    out = derive_averages(sums, n)
    assert np.all(np.isfinite(out["p_rms"])) and np.all(out["p_rms"] >= 0.0)
    assert np.all(out["p_rms"][raw < 0] == 0.0)
    # the stated order of evaluation, bit for bit
    nf = np.float64(n)
    u, w = sums[0] / nf, sums[1] / nf
    assert np.array_equal(out["uw"], sums[5] / nf - u * w)
    assert np.array_equal(out["uu"], sums[3] / nf - u * u)
    assert np.array_equal(out["tke"], 0.5 * (out["uu"] + out["ww"]))


def test_zero_samples_raises():
    from fs.averages import derive_averages
    with pytest.raises(ValueError):
        derive_averages(new_sums((4, 4)), 0)


@pytest.mark.parametrize("every,start", [(1, 0), (3, 0), (4, 10), (5, 3), (7, 50), (2, 1)])
def test_sampling_rule(every, start):
    from fs.averages import is_sampling_launch, samples_after
    launches = 61
    exp = sampling_launches(launches, every, start)
    assert [n for n in range(launches) if is_sampling_launch(n, every, start)] == exp
    for m in range(launches + 1):
        assert samples_after(m, every, start) == len([n for n in exp if n < m])


def test_recirculation_length():
    from fs.averages import recirculation_length
    X, Y = 40, 9
    mask = np.zeros((X, Y), np.uint8)
    box = (5, 3, 9, 6)
    mask[5:9, 3:6] = 1
    mask[X - 1, :] = 3
    u = np.ones((X, Y))
    dx = 0.25
    assert recirculation_length(u, mask, box, dx) == 0.0             # never reversed
    u[9:17, 4] = -0.2                                                 # bubble: cells 9 .. 16 of the middle row
    assert recirculation_length(u, mask, box, dx) == (17 - 9) * dx
    u[20, 4] = 0.0                                                    # a later cell that is not > 0: the run starts behind it
    assert recirculation_length(u, mask, box, dx) == (21 - 9) * dx
    u[9:17, 3] = 1.0                                                  # other rows do not matter
    assert recirculation_length(u, mask, box, dx) == (21 - 9) * dx
    u[9:, 4] = -1.0
    assert np.isnan(recirculation_length(u, mask, box, dx))          # reversed to the end of the row
    with pytest.raises(ValueError):
        recirculation_length(u, mask, (5, 3, X + 1, 6), dx)


# ---- host logic on the NumPy stand-in ------------------------------------------------------------------------------------------------
FNAME = "traj_bc1_upwind_vc0.npz"


@pytest.fixture
def standin():
    import fs
    from mean_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


@pytest.mark.parametrize("every,start", [(1, 0), (3, 0), (4, 10)])
def test_averages_follow_the_steps(every, start, standin):
    from fs.averages import derive_averages
    from mean_standin import make_sim
    a, b = make_sim(FNAME), make_sim(FNAME)
    a.start_averaging(every=every, start_step=start)
    a.run(17)
    a.run(12)
    sums, launches, samples = run_reference(b, 29, every, start)
    got = a._dev.mean_read(a._averager.mean)
    assert (got[1], got[2]) == (29, samples) and samples == len(sampling_launches(29, every, start))
    assert np.array_equal(got[0], sums)
    out = a.averages()
    assert out["samples"] == samples and out["steps"] == 29
    mask = np.asarray(a._solver._bc.mask)
    exp = derive_averages(sums, samples, mask)
    assert set(out) == {"samples", "steps", "mask"} | set(exp)
    for k, e in exp.items():
        assert np.array_equal(out[k], e), k
        assert np.all(out[k][mask == 1] == 0.0)
    assert np.array_equal(out["mask"], mask)
    fa, fb = a.field_to_numpy(), b.field_to_numpy()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa), "averaging changed the trajectory"


def test_start_reset_stop(standin):
    from mean_standin import make_sim
    sim = make_sim(FNAME)
    with pytest.raises(RuntimeError):
        sim.averages()
    base = sim._signature()
    sim.start_averaging(every=2, start_step=3)
    tok = sim._averager.token
    assert tok in sim._signature() and tok not in base
    with pytest.raises(RuntimeError):
        sim.start_averaging()
    sim.run(3)
    with pytest.raises(RuntimeError):
        sim.averages()                          # 3 steps, start 3: no sample yet
    sim.run(4)
    assert sim.averages()["samples"] == 2 and sim.averages()["steps"] == 7
    sim.reset_averages()
    with pytest.raises(RuntimeError):
        sim.averages()
    sim.run(2)                                  # steps 8, 9: the phase runs on - step 9 samples (9 - 3 = 6)
    out = sim.averages()
    assert (out["samples"], out["steps"]) == (1, 9)
    d = sim.field_to_numpy()
    fluid = np.asarray(sim._solver._bc.mask) != 1
    assert np.array_equal(out["u"][fluid], d["v"][..., 0].astype(np.float64)[fluid])
    sim.stop_averaging()
    assert tok not in sim._signature() and len(sim._signature()) == len(base)
    with pytest.raises(RuntimeError):
        sim.averages()
    with pytest.raises(RuntimeError):
        sim.reset_averages()
    sim.stop_averaging()                        # (a second stop is a no-op)
    for bad in (dict(every=0), dict(start_step=-1)):
        with pytest.raises(ValueError):
            sim.start_averaging(**bad)
    sim.start_averaging()                       # a fresh one after the stop
    sim.run(1)
    assert sim.averages()["samples"] == 1


def test_mean_fields_and_resume(standin):
    from mean_standin import make_sim
    a, b = make_sim(FNAME), make_sim(FNAME)
    a.start_averaging(every=2)
    a.run(10)
    sums, launches, samples = a._dev.mean_read(a._averager.mean)
    v, p = a.mean_fields()
    mask = np.asarray(a._solver._bc.mask)
    n = np.float64(samples)
    for got, k in ((v.to_numpy()[..., 0], 0), (v.to_numpy()[..., 1], 1), (p.to_numpy(), 2)):
        assert np.array_equal(got, np.where(mask == 1, np.float32(0), (sums[k] / n).astype(np.float32)))
    # resume: b takes a's state and sums after 10 steps, both go on
    b.run(10)
    b.start_averaging(every=2)
    b._dev.mean_write(b._averager.mean, sums, launches, samples)
    a.run(7)
    b.run(7)
    ra, rb = a._dev.mean_read(a._averager.mean), b._dev.mean_read(b._averager.mean)
    assert ra[1:] == rb[1:] == (17, 8) and np.array_equal(ra[0], rb[0])
    with pytest.raises(ValueError):
        b._dev.mean_write(b._averager.mean, sums[:, :-1], launches, samples)
    with pytest.raises(ValueError):
        b._dev.mean_write(b._averager.mean, sums, 3, 4)


@pytest.mark.parametrize("world,halo", [(2, 2), (3, 2), (4, 2)])
def test_slab_sums_match_single_domain(world, halo, tmp_path, standin):
    from mean_standin import make_sim, run
    every, start, chunks = 3, 4, [55, 6]
    mp.spawn(run, args=(world, _free_port(), FNAME, halo, every, start, chunks, str(tmp_path)), nprocs=world, join=True)
    got = dict(np.load(os.path.join(tmp_path, "slabs.npz")))
    sim = make_sim(FNAME)
    sim.start_averaging(every=every, start_step=start)
    for n in chunks:
        sim.run(n)
    sums, launches, samples = sim._dev.mean_read(sim._averager.mean)
    assert int(got["tapes"]) > 0, "the slab run never replayed a tape"
    assert (int(got["launches"]), int(got["samples"])) == (launches, samples) == (61, 19)
    assert np.array_equal(got["sums"], sums), "assembled slab sums differ from the single domain"
    avg = sim.averages()
    assert np.array_equal(got["u"], avg["u"]) and np.array_equal(got["uu"], avg["uu"])
    st = sim.mean_flow_stats()          # (the slabs' scratch fields start with stale ghost rows: the enstrophy needs them exchanged)
    for g, k in ((float(got["ke"]), "kinetic_energy"), (float(got["ens"]), "enstrophy")):       # (sums over ranks: the relative 1e-12 of
        assert st[k] > 0.0 and abs(g - st[k]) <= 1e-12 * st[k], k                                 #  tests/flow_stats_ref.py compare)
