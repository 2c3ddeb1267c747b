"""CLI snapshot POD (2d-fluid-simulator_amd/main.py --pod-snapshots / --pod-every / --pod-start / --pod-modes / --pod-file, the snapshots in
--save-state / --load-state)."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

RES = 20
KEYS = {"energies", "fraction", "coefficients", "gram", "sample_steps", "samples", "steps", "u", "w", "p", "mean_u", "mean_w", "mean_p", "mask",
        "dt", "dx", "every", "start"}


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_pod", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.pod_snapshots, a.pod_every, a.pod_start, a.pod_modes, a.pod_file) == (0, None, None, None, None)
    a = cli.build_parser().parse_args(["--pod-snapshots", "16", "--pod-every", "5", "--pod-start", "100", "--pod-modes", "3", "--pod-file", "p.npz"])
    assert (a.pod_snapshots, a.pod_every, a.pod_start, a.pod_modes, a.pod_file) == (16, 5, 100, 3, "p.npz")
    for argv in (["--pod-every", "4"],                            # without --pod-snapshots
                 ["--pod-start", "4"],
                 ["--pod-modes", "2"],
                 ["--pod-file", str(tmp_path / "p.npz")],
                 ["--pod-snapshots", "1"],
                 ["--pod-snapshots", "65"],
                 ["--pod-snapshots", "-3"],
                 ["--pod-snapshots", "4", "--pod-every", "0"],
                 ["--pod-snapshots", "4", "--pod-start", "-1"],
                 ["--pod-snapshots", "4", "--pod-modes", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["-res", str(RES), "--out", str(tmp_path)])
        assert e.value.code == 2, argv


def test_checkpoint_with_other_parameters_is_refused(tmp_path, capsys):
    """--load-state of a checkpoint whose snapshots were taken with another M, every or start: message and exit status 2, before any device
    work."""
    from fs.pod import Pod
    cli = _cli()
    ck = tmp_path / "ck.npz"
    np.savez(str(ck), step=np.array(10), **{"pod.slots": np.zeros((4, 3, 4, 2), np.float32), "pod.launches": np.array(10), "pod.samples": np.array(3),
                                            "pod.base": np.array(0), "pod.snapshots": np.array(4), "pod.every": np.array(3), "pod.start": np.array(1)})
    assert Pod.held(np.load(str(ck))) == (4, 3, 1)
    for argv in (["--pod-snapshots", "4", "--pod-every", "2", "--pod-start", "1"], ["--pod-snapshots", "4", "--pod-every", "3"],
                 ["--pod-snapshots", "8", "--pod-every", "3", "--pod-start", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["-res", str(RES), "--load-state", str(ck), "--out", str(tmp_path)])
        assert e.value.code == 2
        assert "--pod-snapshots 4 --pod-every 3 --pod-start 1" in capsys.readouterr().err
    plain = tmp_path / "plain.npz"
    np.savez(str(plain), step=np.array(10))
    assert Pod.held(np.load(str(plain))) is None


@pytest.mark.gpu
def test_pod_file(tmp_path, hip_lib):
    import fs
    cli = _cli()
    a = tmp_path / "a"
    cli.main(["-res", str(RES), "--pod-snapshots", "8", "--pod-every", "2", "--steps", "21", "--out", str(a), "--graph"])
    assert not list(a.glob("pod_mode_*.png"))                    # (no -vis given: the file alone)
    m = np.load(a / "pod.npz")
    assert set(m.files) == KEYS
    assert int(m["samples"]) == 10 and int(m["steps"]) == 21 and (int(m["every"]), int(m["start"])) == (2, 0)
    assert m["sample_steps"].tolist() == [6, 8, 10, 12, 14, 16, 18, 20] and m["gram"].shape == (8, 8)
    lam = m["energies"]
    assert 1 <= len(lam) <= 7 and np.all(np.diff(lam) <= 0.0) and np.all(lam > 0.0)
    assert abs(m["fraction"].sum() - 1.0) <= 1e-12
    K = min(4, len(lam))
    X, Y = m["mask"].shape
    assert m["coefficients"].shape == (8, K) and m["u"].shape == m["w"].shape == m["p"].shape == (K, X, Y) and m["mean_u"].shape == (X, Y)
    assert np.all(m["u"][:, m["mask"] == 1] == 0.0) and np.abs(m["u"][0]).max() > 0.0
    # the same run through the Python interface
    assert float(m["dx"]) == 1 / RES and float(m["dt"]) == 0.05 / RES
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(1, RES, 0.05 / RES, 1.0 / RES, 1e6, 5.0, "cip")
    try:
        sim.start_pod(8, every=2)
        sim.run(21, graph=True)
        exp = sim.pod(4)
        for k in ("gram", "energies", "fraction", "coefficients", "sample_steps"):
            assert np.array_equal(m[k], exp[k]), k
        assert np.array_equal(m["u"][0], sim.pod_fields(0)[0].to_numpy()[..., 0]) and np.array_equal(m["mean_p"], sim.pod_fields(None)[1].to_numpy())
    finally:
        sim._solver._bc.device.close()
    # with -vis: the modes as images too
    b = tmp_path / "b"
    cli.main(["-res", str(RES), "--pod-snapshots", "8", "--pod-every", "2", "--pod-modes", "2", "--steps", "21", "--out", str(b), "-vis", "2"])
    assert sorted(f.name for f in b.glob("pod_mode_*.png")) == ["pod_mode_0.png", "pod_mode_1.png"]
    assert np.array_equal(np.load(b / "pod.npz")["gram"], m["gram"])          # (eager steps: the same bits as the graph's)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_resume_equals_the_uninterrupted_run(graph, tmp_path, hip_lib):
    cli = _cli()
    common = ["-res", str(RES), "--pod-snapshots", "4", "--pod-every", "2", "--pod-start", "3", "--pod-modes", "2"] + (["--graph"] if graph else [])
    a, b = tmp_path / "a", tmp_path / "b"
    cli.main(common + ["--steps", "27", "--out", str(a)])
    m = np.load(a / "pod.npz")
    assert int(m["samples"]) == 12 and m["sample_steps"].tolist() == [21, 23, 25, 27]
    b.mkdir()
    cli.main(common + ["--steps", "5", "--out", str(b), "--save-state", str(b / "ck.npz")])     # (1 sample: no file yet)
    assert not (b / "pod.npz").exists()
    ck = np.load(b / "ck.npz")
    assert int(ck["pod.samples"]) == 1 and ck["pod.slots"].shape[:2] == (4, 3)
    cli.main(common + ["--steps", "22", "--out", str(b), "--load-state", str(b / "ck.npz")])
    r = np.load(b / "pod.npz")
    assert set(r.files) == set(m.files)
    for k in r.files:
        assert np.array_equal(r[k], m[k]), f"{k}: the resumed POD differs from the uninterrupted one"
    # a checkpoint without snapshots starts fresh
    cli.main(["-res", str(RES), "--steps", "3", "--out", str(b), "--save-state", str(b / "plain.npz")])
    cli.main(common + ["--steps", "14", "--out", str(b), "--load-state", str(b / "plain.npz")])
    assert int(np.load(b / "pod.npz")["samples"]) == 5
