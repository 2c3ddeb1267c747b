"""The scene, the cadences and the readers of the test that attaches every rider of the step at once (tests/test_gpu_riders.py): bc3 res
64 under the CIP solver - a body and a 6-step buffer rotation - with twelve kinds of rider whose cadences and starts are pairwise different,
so that no two of them sample on the same set of steps.  Shared so that the combined simulator, the eager one, the downloading one and the
twelve that carry one kind each are attached by the same code."""
import numpy as np

RES = 64
DT, DX, RE, VC = 0.05 / RES, 1.0 / RES, 1.0e6, 5.0
STEPS, MORE = 100, 20

# the documented order of FluidSimulator._riders(), and the kinds of the tokens they put into a signature, in that order
RIDER_ORDER = ["Recorder", "Averager", "Modes", "Pod", "Distributions", "Spectra", "CrossSpectra", "ScaleFluxes", "Budget", "Tracker", "Tracers", "Vortices"]
TOKEN_KINDS = ["history", "mean", "modes", "pod", "dist", "spec", "xspec", "flux", "budget", "loads", "tracer", "tracer_accum", "vortices"]
KINDS = ("history", "mean", "modes", "pod", "dist", "spec", "xspec", "flux", "budget", "loads", "tracers", "vortices")

PROBES = [(5, 30)]
HISTORY = dict(every=1, capacity=20)
MEAN = dict(every=3, start_step=0)
MODES = dict(every=2, start_step=5)
MODE_CYCLES = (0.06, 0.11)              # cycles per sample: below the Nyquist limit of 0.5
POD = dict(snapshots=4, every=5, start_step=0)
CHANNELS = [{"quantity": "speed", "bins": 100, "range": (0.0, 1.5)},       # CHANNELS of tests/test_gpu_dist.py
            {"quantity": "u", "bins": 32, "range": (-0.5, 1.5), "box": (3, 2, 30, 18), "against": {"quantity": "vorticity", "bins": 128, "range": (-20.0, 20.0)}}]
DIST = dict(every=2, start_step=3)
SPEC_BOX = (17, 23, 49, 39)             # 32 x 16 at an odd offset, over cylinders of the scene
SPEC = dict(every=4, start_step=1)
XSPEC_PAIR = ("vorticity", "p")
XSPEC = dict(every=3, start_step=2)
FLUX_BOX = (20, 24, 36, 40)             # 16 x 16 inside the box of the spectra
FLUX_WIDTHS = (1, 3)
FLUX = dict(every=5, start_step=2)
BUDGET = dict(every=7, start_step=1)    # over SPEC_BOX: wall cells and fluid cells; steps 8, 15, ..., 99
LOADS = dict(every=2, capacity=10)
N_TRACERS, SORT_EVERY = 256, 32
TRACER_ACCUM = dict(every=3)
VORTICES = dict(every=3, capacity=7)
RINGS = (HISTORY, LOADS, VORTICES)
# sim.quantile("q", 0.85) of a simulator of this scene without a rider, f32, after the STEPS steps of the run (f64: -0.09330): a constant,
# so that the tracker under test never chooses its own threshold
VORTEX_THRESHOLD = -0.09282344878504668


def frequencies():
    return [c / (MODES["every"] * DT) for c in MODE_CYCLES]


def tau():
    """Every third particle without inertia, the others with five response times of the order of the step."""
    n = np.arange(N_TRACERS)
    return np.where(n % 3 == 0, 0.0, 0.001 * (1 + n % 5))


def samples(every, start_step=0, steps=STEPS, **_):
    """The steps 1 .. steps at which a rider of this cadence samples, by the rule in a plain loop."""
    return [k for k in range(1, steps + 1) if k > start_step and (k - start_step) % every == 0]


def make(dtype):
    import fs
    fs.runtime.init(gpu=0, dtype=dtype)
    return fs.FluidSimulator.create(3, RES, DT, DX, RE, VC, "cip")


def close(sim):
    sim._solver._bc.device.close()


def attach(sim, kinds=KINDS, capacities=None):
    """Attach the riders of `kinds` (in the order of KINDS, whatever the order of the argument); capacities: other sizes for the history,
    loads and vortex rings."""
    from fs.boundary_condition import default_body_box
    from fs.tracers import seed_line
    box = default_body_box(3, RES)
    HISTORY, LOADS, VORTICES = (dict(d, capacity=c) for d, c in zip(RINGS, capacities or [d["capacity"] for d in RINGS]))
    if "history" in kinds:
        sim.record_history(PROBES, box, **HISTORY)
    if "mean" in kinds:
        sim.start_averaging(**MEAN)
    if "modes" in kinds:
        sim.start_modes(frequencies(), **MODES)
    if "pod" in kinds:
        sim.start_pod(**POD)
    if "dist" in kinds:
        sim.start_distributions(CHANNELS, **DIST)
    if "spec" in kinds:
        sim.start_spectra(SPEC_BOX, **SPEC)
    if "xspec" in kinds:
        sim.start_cross_spectra(SPEC_BOX, XSPEC_PAIR, **XSPEC)
    if "flux" in kinds:
        sim.start_scale_fluxes(FLUX_BOX, FLUX_WIDTHS, **FLUX)
    if "budget" in kinds:
        sim.start_budget(SPEC_BOX, **BUDGET)
    if "loads" in kinds:
        sim.track_body(box, **LOADS)
    if "tracers" in kinds:
        sim.seed_tracers(seed_line((4.5, 2.5), (4.5, 61.5), N_TRACERS), sort_every=SORT_EVERY, tau=tau(), deposits=True)
        sim.accumulate_tracers(**TRACER_ACCUM)
    if "vortices" in kinds:
        sim.track_vortices(VORTEX_THRESHOLD, "q", **VORTICES)
    return sim


def _fields(pair):
    v, p = pair
    return {"v": v.to_numpy(), "p": p.to_numpy()}


def read(sim, kind):
    """{reader: what it returns} for the readers of one kind of rider; device fields as downloads."""
    dev = sim._dev
    if kind == "history":
        return {"history": sim.history()}
    if kind == "mean":
        return {"averages": sim.averages()}
    if kind == "modes":
        return {"modes": sim.modes(), "mode_fields": _fields(sim.mode_fields()), "mode_fields(0.7, 1)": _fields(sim.mode_fields(0.7, 1))}
    if kind == "pod":
        out = {"pod": sim.pod(), "ftle": sim.ftle("backward")}
        out.update({f"pod_snapshot({m})": _fields(sim.pod_snapshot(m)) for m in range(POD["snapshots"])})
        return out
    if kind == "dist":
        return {"distributions": sim.distributions()}
    if kind == "spec":
        return {"spectra": sim.spectra(), "plane": dev.spec_plane(sim._spectrar.spec)}
    if kind == "xspec":
        return {"cross_spectra": sim.cross_spectra(), "plane": dev.xspec_plane(sim._xspectrar.xspec)}
    if kind == "flux":
        return {"scale_fluxes": sim.scale_fluxes(), "filtered": {r: dev.flux_filtered(sim._fluxr.flux, r) for r in FLUX_WIDTHS}}
    if kind == "budget":
        return {"budget": sim.budget()}
    if kind == "loads":
        return {"body_loads": sim.body_loads(), "body_surface.sums": sim.body_surface()["sums"]}
    if kind == "tracers":
        return {"tracers": sim.tracers(), "tracer_fields": sim.tracer_fields(), "tracer_deposits": sim.tracer_deposits(),
                "tracer_accumulation": sim.tracer_accumulation()}
    if kind == "vortices":
        return {"vortices": sim.vortices(), "vortex_labels": sim.vortex_labels()}
    raise ValueError(kind)


def same(a, b, what):
    """a == b through dicts, lists and tuples; arrays by dtype, shape and np.array_equal (NaN equal to NaN in float arrays)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), what
        for k in a:
            same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for n, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}[{n}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, what
        assert np.array_equal(a, b, equal_nan=a.dtype.kind in "fc"), what
    elif isinstance(a, float) and a != a:
        assert isinstance(b, float) and b != b, what
    else:
        assert a == b, what


def rider_tokens(sig):
    """The riders' tokens in a signature, in its order: (kind, serial) - the entries of the fields begin with a number."""
    return [t for t in sig if isinstance(t, tuple) and t and isinstance(t[0], str)]
