"""Every output of the CLI in one run (2d-fluid-simulator_amd/main.py with history, mean, modes, POD, distributions, FTLE, loads, vortices,
tracers and the stats on): the files it writes have the layout of tests/golden/cli_all_outputs.json - key sets, shapes, dtypes, recorded
from this command line - and the same 24 steps over a --save-state / --load-state restart give the same arrays."""
import importlib.util
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN, REPO

RES, STEPS = 64, 24
NPZ = ("history", "mean", "modes", "pod", "dist", "ftle", "loads", "vortices", "tracers", "tracer_fields")
# the recorders of the per-step series start at the resumed step (a history recorder resumes nothing; a body tracker numbers its records on,
# tests/test_cli_loads.py): these arrays of the resumed run hold the rows of the steps it covered, every other array the whole run
ROWS = {"history": ("step", "time", "u", "w", "p", "force_x", "force_y"),
        "loads": ("step", "time", "pressure_x", "pressure_y", "viscous_x", "viscous_y", "force_x", "force_y", "moment_pressure",
                  "moment_viscous", "moment", "cd", "cl", "cm")}


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_all_outputs", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def all_outputs_args(out):
    """The command line with everything on (without --steps); the probe: a fluid cell picked as in tests/test_cli_history.py, the vortex
    threshold and minimum area: those of tests/test_cli_vortices.py."""
    from fs.boundary_condition import create_scene_arrays
    fluid = np.argwhere(create_scene_arrays(5, RES)[1] == 0)
    x, y = (int(c) for c in fluid[len(fluid) // 2])
    return ["-bc", "5", "-res", str(RES), "--out", str(out), "--stats-every", "4", "--body", "auto",
            "--history-every", "1", "--probe", f"{x},{y}",
            "--mean-every", "2", "--mean-start", "4",
            "--modes-freq", "1.5,3", "--modes-every", "2",
            "--pod-snapshots", "4", "--pod-every", "2", "--pod-modes", "2",
            "--dist", "speed:64:0:1.5", "--dist", "u:16:-1:1,w:16:-1:1", "--dist-every", "2",
            "--ftle", "backward",
            "--loads-every", "2", "--loads-ref", "1,0.25",
            "--vortices-every", "3", "--vortex-threshold", "0.5", "--vortex-min-area", "2",
            "--tracers", "300", "--tracer-seed", "9", "--tracer-tau", "0,0.01", "--tracer-fields", "--tracer-accumulate-every", "2"]


def layout(out):
    """{file: {key: [shape, dtype]}} of the .npz files in `out`, and the column names of stats.csv."""
    got = {}
    for name in NPZ:
        path = os.path.join(str(out), name + ".npz")
        if os.path.exists(path):
            z = np.load(path)
            got[name + ".npz"] = {k: [list(z[k].shape), str(z[k].dtype)] for k in sorted(z.files)}
    stats = os.path.join(str(out), "stats.csv")
    if os.path.exists(stats):
        with open(stats) as fh:
            got["stats.csv"] = fh.readline().strip().split(",")
    return got


@pytest.fixture(scope="module")
def runs(tmp_path_factory, hip_lib):
    """(uninterrupted, resumed): the output folders of the 24 steps at once and of 12 steps, a checkpoint, 12 more.  Shared and left as
    they are."""
    cli = _cli()
    a, b = tmp_path_factory.mktemp("whole"), tmp_path_factory.mktemp("resumed")
    cli.main(all_outputs_args(a) + ["--steps", str(STEPS)])
    cli.main(all_outputs_args(b) + ["--steps", str(STEPS // 2), "--save-state", str(b / "ck.npz")])
    cli.main(all_outputs_args(b) + ["--steps", str(STEPS // 2), "--load-state", str(b / "ck.npz")])
    return a, b


@pytest.mark.gpu
def test_every_file_has_the_recorded_layout(runs):
    with open(os.path.join(GOLDEN, "cli_all_outputs.json")) as fh:
        exp = json.load(fh)
    assert set(exp) == {n + ".npz" for n in NPZ} | {"stats.csv"}
    got = layout(runs[0])
    assert set(got) == set(exp), "files written"
    for name in exp:
        assert got[name] == exp[name], name


@pytest.mark.gpu
def test_resumed_run_equals_the_uninterrupted_one(runs):
    a, b = runs
    for name in NPZ:
        whole, resumed = np.load(a / f"{name}.npz"), np.load(b / f"{name}.npz")
        assert set(whole.files) == set(resumed.files), name
        rows = ROWS.get(name, ())
        if rows:
            assert resumed["step"].tolist() == list(range(int(resumed["step"][0]), STEPS + 1, int(resumed["step"][1] - resumed["step"][0])))
            covered = np.isin(whole["step"], resumed["step"])
            assert covered.sum() == len(resumed["step"]) > 0
        for k in whole.files:
            x, y = (whole[k][covered] if k in rows else whole[k]), resumed[k]
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{name}.npz[{k}]"
