"""The checkpoint format of the five riders that accumulate over counted samples (fs.riders.CountedRider), without a GPU: on the NumPy
stand-in devices (tests/budget_standin.py stacks those of the distributions, both spectra and the scale fluxes under its own) the keys of
checkpoint() are the ones written out here - those of the classes before they shared a base -, and held() of that checkpoint returns the
parameters the rider was attached with."""
import numpy as np
import pytest

FNAME = "traj_bc3_upwind_vc0.npz"            # a 64 x 32 grid
BOX = (8, 4, 40, 20)                         # 32 x 16: sides the spectra take
CHANNELS = [{"quantity": "speed", "bins": 16, "range": (0.0, 2.0)},
            {"quantity": "u", "bins": 8, "range": (-1.0, 2.0), "box": (3, 2, 30, 18), "against": {"quantity": "vorticity", "bins": 4, "range": (-20.0, 20.0)}}]
HW = (1, 3)
EVERY, START, STEPS = 2, 1, 6

KEYS = {
    "_distr": ["dist.base", "dist.channels", "dist.every", "dist.launches", "dist.samples", "dist.start", "dist.tables"],
    "_spectrar": ["spec.base", "spec.box", "spec.detrend", "spec.every", "spec.launches", "spec.power", "spec.samples", "spec.start",
                  "spec.window"],
    "_xspectrar": ["xspec.base", "xspec.box", "xspec.detrend", "xspec.every", "xspec.launches", "xspec.quantities", "xspec.samples",
                   "xspec.start", "xspec.sums", "xspec.window"],
    "_fluxr": ["flux.base", "flux.box", "flux.every", "flux.half_widths", "flux.launches", "flux.samples", "flux.start", "flux.sums"],
    "_budgetr": ["budget.base", "budget.box", "budget.every", "budget.launches", "budget.samples", "budget.start", "budget.sums"],
}


@pytest.fixture(scope="module")
def standin():
    import fs
    from budget_standin import device_cls
    saved = fs.runtime.config()
    fs.runtime.init(dtype="f32", device_cls=device_cls())
    yield
    fs.runtime.init(**{k: saved[k] for k in ("gpu", "rank", "nranks", "halo", "bcast", "allgather", "device_cls")},
                    dtype="f64" if saved["dtype"] == np.float64 else "f32")


def _held_equal(got, want):
    assert type(got) is tuple and len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w)
        else:
            assert type(g) is type(w) and g == w


def test_checkpoint_keys_and_held_parameters_of_the_counted_riders(standin):
    from budget_standin import make_sim
    from fs.dist import channels_array
    from fs.riders import CountedRider
    sim, _ = make_sim(FNAME)
    sim.start_distributions(CHANNELS, every=EVERY, start_step=START)
    sim.start_spectra(BOX, every=EVERY, start_step=START, window="boxcar", detrend=False)
    sim.start_cross_spectra(BOX, ("vorticity", None), every=EVERY, start_step=START, window="hann", detrend=True)
    sim.start_scale_fluxes(BOX, HW, every=EVERY, start_step=START)
    sim.start_budget(BOX, every=EVERY, start_step=START)
    sim.run(STEPS)
    attached = {
        "_distr": (channels_array(sim._distr.dist.channels), EVERY, START),
        "_spectrar": (BOX, "boxcar", False, EVERY, START),
        "_xspectrar": (BOX, ("vorticity", None), "hann", True, EVERY, START),
        "_fluxr": (BOX, HW, EVERY, START),
        "_budgetr": (BOX, EVERY, START),
    }
    assert attached["_distr"][0].shape == (2, 12) and attached["_distr"][0].dtype == np.float64
    for attr, keys in KEYS.items():
        rider = getattr(sim, attr)
        assert isinstance(rider, CountedRider), attr
        z = rider.checkpoint()
        assert sorted(z) == keys, attr
        kind = keys[0].split(".")[0]
        assert all(isinstance(a, np.ndarray) for a in z.values()), attr
        assert (int(z[kind + ".launches"]), int(z[kind + ".samples"]), int(z[kind + ".base"])) == (STEPS, 2, 0), attr
        _held_equal(rider.held(z), attached[attr])
        assert rider.held({}) is None and type(rider).held(z) is not None, attr
        assert rider.restore(z) == 2, attr
