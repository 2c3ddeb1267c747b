"""CLI FTLE fields (2d-fluid-simulator_amd/main.py --ftle / --ftle-refine / --ftle-substeps / --ftle-file)."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

RES = 20


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_lcs", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.ftle, a.ftle_refine, a.ftle_substeps, a.ftle_file) == (None, None, None, None)
    a = cli.build_parser().parse_args(["--ftle", "both", "--ftle-refine", "4", "--ftle-substeps", "3", "--ftle-file", "f.npz"])
    assert (a.ftle, a.ftle_refine, a.ftle_substeps, a.ftle_file) == ("both", 4, 3, "f.npz")
    for argv in (["--ftle", "backward"],                                        # without --pod-snapshots
                 ["--ftle", "both", "--ftle-refine", "2"],
                 ["--ftle", "sideways", "--pod-snapshots", "4"],
                 ["--ftle-refine", "2", "--pod-snapshots", "4"],                # without --ftle
                 ["--ftle-substeps", "2", "--pod-snapshots", "4"],
                 ["--ftle-file", str(tmp_path / "f.npz"), "--pod-snapshots", "4"],
                 ["--ftle", "forward", "--pod-snapshots", "4", "--ftle-refine", "3"],
                 ["--ftle", "forward", "--pod-snapshots", "4", "--ftle-refine", "16"],
                 ["--ftle", "forward", "--pod-snapshots", "4", "--ftle-substeps", "0"],
                 ["--ftle", "forward", "--pod-snapshots", "4", "--ftle-substeps", "17"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["-res", str(RES), "--out", str(tmp_path)])
        assert e.value.code == 2, argv


@pytest.mark.gpu
def test_ftle_file(tmp_path, hip_lib):
    import fs
    cli = _cli()
    a = tmp_path / "a"
    cli.main(["-res", str(RES), "--pod-snapshots", "4", "--pod-every", "2", "--ftle", "both", "--ftle-refine", "2", "--ftle-substeps", "2",
              "--steps", "14", "--out", str(a), "--graph"])
    assert not list(a.glob("ftle_*.png"))                        # (no -vis given: the file alone)
    m = np.load(a / "ftle.npz")
    assert set(m.files) == {f"{k}_{d}" for k in ("ftle", "status", "x", "y") for d in ("forward", "backward")} | {"span", "sample_steps", "refine"}
    assert m["sample_steps"].tolist() == [8, 10, 12, 14] and int(m["refine"]) == 2 and float(m["span"]) == 3 * 2 * (0.05 / RES)
    assert m["ftle_forward"].shape == m["status_backward"].shape == m["x_forward"].shape == (4 * RES, 2 * RES)
    assert np.isfinite(m["ftle_backward"]).sum() > RES * RES and not np.array_equal(m["x_forward"], m["x_backward"])
    # the same run through the Python interface
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(1, RES, 0.05 / RES, 1.0 / RES, 1e6, 5.0, "cip")
    try:
        sim.start_pod(4, every=2)
        sim.run(14, graph=True)
        for d in ("forward", "backward"):
            exp = sim.flow_map(d, refine=2, substeps=2)
            for k in ("ftle", "status", "x", "y"):
                assert np.array_equal(m[f"{k}_{d}"], exp[k], equal_nan=True), (k, d)
    finally:
        sim._solver._bc.device.close()
    # with -vis: the image too; one sample only: a message and no file
    b = tmp_path / "b"
    cli.main(["-res", str(RES), "--pod-snapshots", "4", "--pod-every", "2", "--ftle", "backward", "--steps", "14", "--out", str(b), "-vis", "1",
              "--ftle-file", str(b / "lcs.npz")])
    assert sorted(f.name for f in b.glob("ftle_*.png")) == ["ftle_backward.png"] and (b / "lcs.npz").exists() and not (b / "ftle.npz").exists()
    assert set(np.load(b / "lcs.npz").files) == {"ftle_backward", "status_backward", "x_backward", "y_backward", "span", "sample_steps", "refine"}
    c = tmp_path / "c"
    cli.main(["-res", str(RES), "--pod-snapshots", "4", "--pod-every", "2", "--ftle", "backward", "--steps", "3", "--out", str(c)])
    assert not (c / "ftle.npz").exists()
