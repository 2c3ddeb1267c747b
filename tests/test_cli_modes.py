"""CLI harmonic modes (2d-fluid-simulator_amd/main.py --modes-freq / --modes-every / --modes-start / --modes-file / --modes-frames, the
sums in --save-state / --load-state)."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

RES = 64
DT = 0.05 / RES
FREQ = [repr(0.03 / DT), repr(0.07 / DT)]       # 0.06 and 0.14 cycles per sample at --modes-every 2


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_modes", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.modes_freq, a.modes_every, a.modes_start, a.modes_file, a.modes_frames) == (None, None, None, None, 0)
    a = cli.build_parser().parse_args(["--modes-freq", "1.5,3", "--modes-every", "5", "--modes-start", "100", "--modes-file", "m.npz", "--modes-frames", "8"])
    assert (a.modes_freq, a.modes_every, a.modes_start, a.modes_file, a.modes_frames) == ("1.5,3", 5, 100, "m.npz", 8)
    nyquist = repr(0.5 / (2 * DT))                                # f * every * dt = 0.5 at --modes-every 2
    for argv in (["--modes-every", "4"],                          # without --modes-freq
                 ["--modes-start", "4"],
                 ["--modes-file", str(tmp_path / "m.npz")],
                 ["--modes-frames", "4"],
                 ["--modes-freq", "x"],
                 ["--modes-freq", "1,2,3,4,5"],                   # more than MODES_MAX_FREQ
                 ["--modes-freq", "2,2"],
                 ["--modes-freq", "-1"],
                 ["--modes-freq", "0"],
                 ["--modes-freq", "1", "--modes-every", "0"],
                 ["--modes-freq", "1", "--modes-start", "-1"],
                 ["--modes-freq", "1", "--modes-frames", "-2"],
                 ["--modes-freq", "1", "--modes-frames", "4", "-vis", "3"],
                 ["--modes-freq", nyquist, "--modes-every", "2"],
                 ["--modes-freq", "1," + nyquist, "--modes-every", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["-res", str(RES), "--out", str(tmp_path)])
        assert e.value.code == 2, argv


def test_checkpoint_with_other_parameters_is_refused(tmp_path, capsys):
    """--load-state of a checkpoint whose modes were taken with other frequencies, every or start: message and exit status 2, before any
    device work."""
    from fs.modes import Modes
    cli = _cli()
    ck = tmp_path / "ck.npz"
    np.savez(str(ck), step=np.array(10), **{"modes.sums": np.zeros((9, 4, 2)), "modes.scalars": np.zeros(8), "modes.launches": np.array(10),
                                            "modes.samples": np.array(3), "modes.frequencies": np.array([1.5]), "modes.every": np.array(3),
                                            "modes.start": np.array(1)})
    assert Modes.held(np.load(str(ck))) == ((1.5,), 3, 1)
    for argv in (["--modes-freq", "1.5", "--modes-every", "2", "--modes-start", "1"], ["--modes-freq", "1.5", "--modes-every", "3"],
                 ["--modes-freq", "1.25", "--modes-every", "3", "--modes-start", "1"],
                 ["--modes-freq", "1.5,2.5", "--modes-every", "3", "--modes-start", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["-res", str(RES), "--load-state", str(ck), "--out", str(tmp_path)])
        assert e.value.code == 2
        assert "--modes-freq 1.5 --modes-every 3 --modes-start 1" in capsys.readouterr().err
    plain = tmp_path / "plain.npz"
    np.savez(str(plain), step=np.array(10))
    assert Modes.held(np.load(str(plain))) is None


ARRAYS = [f"{k}_{a}" for k in ("mean", "amplitude", "phase") for a in "uwp"]


@pytest.mark.gpu
def test_modes_file_and_phase_frames(tmp_path, hip_lib):
    import fs
    cli = _cli()
    a = tmp_path / "a"
    cli.main(["-bc", "5", "-res", str(RES), "--modes-freq", ",".join(FREQ), "--modes-every", "2", "--modes-start", "4", "--steps", "21",
              "--out", str(a), "-vis", "2", "--modes-frames", "3", "--graph"])
    m = np.load(a / "modes.npz")
    assert int(m["samples"]) == 8 and int(m["steps"]) == 21 and (int(m["every"]), int(m["start"])) == (2, 4)
    assert float(m["dx"]) == 1 / RES and float(m["dt"]) == DT and m["frequencies"].tolist() == [float(f) for f in FREQ]
    assert [(a / f"modes_phase_{i}.png").exists() for i in range(4)] == [True, True, True, False]
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(5, RES, DT, 1.0 / RES, 1e6, 5.0, "cip")
    try:
        sim.start_modes([float(f) for f in FREQ], every=2, start_step=4)
        sim.run(21, graph=True)
        exp = sim.modes()
    finally:
        sim._solver._bc.device.close()
    assert set(ARRAYS) | {"mask"} <= set(m.files)
    for name in "uwp":
        for k in ("mean", "amplitude", "phase"):
            assert np.array_equal(m[f"{k}_{name}"], exp[name][k]), (k, name)
    assert m["amplitude_u"].shape == (2, 2 * RES, RES) and np.abs(m["amplitude_u"]).max() > 0.0
    assert np.all(m["amplitude_p"][:, m["mask"] == 1] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_resume_equals_the_uninterrupted_run(graph, tmp_path, hip_lib):
    cli = _cli()
    common = ["-bc", "5", "-res", str(RES), "--modes-freq", ",".join(FREQ), "--modes-every", "2", "--modes-start", "2"] + (["--graph"] if graph else [])
    a, b = tmp_path / "a", tmp_path / "b"
    cli.main(common + ["--steps", "21", "--out", str(a)])
    m = np.load(a / "modes.npz")
    assert int(m["samples"]) == 9
    b.mkdir()
    cli.main(common + ["--steps", "9", "--out", str(b), "--save-state", str(b / "ck.npz")])     # (3 samples, 5 unknowns: no file yet)
    assert not (b / "modes.npz").exists()
    ck = np.load(b / "ck.npz")
    assert int(ck["modes.samples"]) == 3 and ck["modes.sums"].shape == (15, 2 * RES, RES)
    cli.main(common + ["--steps", "12", "--out", str(b), "--load-state", str(b / "ck.npz")])
    r = np.load(b / "modes.npz")
    assert set(r.files) == set(m.files)
    for k in r.files:
        assert np.array_equal(r[k], m[k]), f"{k}: the resumed modes differ from the uninterrupted ones"
    # a checkpoint without sums starts fresh
    cli.main(["-bc", "5", "-res", str(RES), "--steps", "3", "--out", str(b), "--save-state", str(b / "plain.npz")])
    cli.main(common + ["--steps", "14", "--out", str(b), "--load-state", str(b / "plain.npz")])
    assert int(np.load(b / "modes.npz")["samples"]) == 6
