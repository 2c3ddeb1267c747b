"""CLI time averages (2d-fluid-simulator_amd/main.py --mean-every / --mean-start / --mean-file, the sums in --save-state / --load-state)."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_mean", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.mean_every, a.mean_start, a.mean_file) == (0, 0, None)
    a = cli.build_parser().parse_args(["--mean-every", "5", "--mean-start", "1000", "--mean-file", "m.npz"])
    assert (a.mean_every, a.mean_start, a.mean_file) == (5, 1000, "m.npz")
    for argv in (["--mean-start", "4"],                          # without --mean-every
                 ["--mean-file", str(tmp_path / "m.npz")],
                 ["--mean-every", "-1"],
                 ["--mean-every", "2", "--mean-start", "-3"],
                 ["--mean-every", "x"],
                 ["--body", "auto", "--mean-every", "2"]):       # --body still needs --stats-every or --history-every
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2


def test_checkpoint_with_other_parameters_is_refused(tmp_path, capsys):
    """--load-state of a checkpoint whose average was taken with another every / start: message and exit status 2, before any device work."""
    from fs.averages import Averager
    cli = _cli()
    ck = tmp_path / "ck.npz"
    np.savez(str(ck), step=np.array(10), **{"mean.sums": np.zeros((7, 4, 2)), "mean.launches": np.array(10), "mean.samples": np.array(3),
                                            "mean.every": np.array(3), "mean.start": np.array(1)})
    assert Averager.held(np.load(str(ck))) == (3, 1)
    for argv in (["--mean-every", "2", "--mean-start", "1"], ["--mean-every", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--load-state", str(ck), "--out", str(tmp_path)])
        assert e.value.code == 2
        assert "--mean-every 3 --mean-start 1" in capsys.readouterr().err
    plain = tmp_path / "plain.npz"
    np.savez(str(plain), step=np.array(10))
    assert Averager.held(np.load(str(plain))) is None


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_mean_file_and_resume(graph, tmp_path, hip_lib):
    import fs
    cli = _cli()
    res = 64
    common = ["-bc", "5", "-res", str(res), "--mean-every", "2", "--mean-start", "4"] + (["--graph"] if graph else [])
    a, b = tmp_path / "a", tmp_path / "b"
    cli.main(common + ["--steps", "21", "--out", str(a), "-vis", "2", "--frame-every", "21"])
    m = np.load(a / "mean.npz")
    assert int(m["samples"]) == 8 and int(m["steps"]) == 21 and (int(m["every"]), int(m["start"])) == (2, 4)
    assert float(m["dx"]) == 1 / res and float(m["dt"]) == 0.05 / res
    assert (a / "mean_vis.png").exists()
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(5, res, 0.05 / res, 1.0 / res, 1e6, 5.0, "cip")
    try:
        sim.start_averaging(every=2, start_step=4)
        sim.run(21, graph=graph)
        exp = sim.averages()
    finally:
        sim._solver._bc.device.close()
    assert set(exp) <= set(m.files)
    for k in ("u", "w", "p", "uu", "ww", "uw", "p_rms", "tke", "mask"):
        assert np.array_equal(m[k], exp[k]), k
    assert np.abs(m["u"]).max() > 0.0
    # the same 21 steps over a restart: the sums travel with the checkpoint
    b.mkdir()
    cli.main(common + ["--steps", "9", "--out", str(b), "--save-state", str(b / "ck.npz")])
    assert int(np.load(b / "mean.npz")["samples"]) == 2
    cli.main(common + ["--steps", "12", "--out", str(b), "--load-state", str(b / "ck.npz")])
    r = np.load(b / "mean.npz")
    assert int(r["samples"]) == 8 and int(r["steps"]) == 21
    for k in ("u", "w", "p", "uu", "ww", "uw", "p_rms", "tke"):
        assert np.array_equal(r[k], m[k]), f"{k}: the resumed average differs from the uninterrupted one"
    # a checkpoint without sums starts a fresh average
    cli.main(["-bc", "5", "-res", str(res), "--steps", "3", "--out", str(b), "--save-state", str(b / "plain.npz")])
    cli.main(common + ["--steps", "6", "--out", str(b), "--load-state", str(b / "plain.npz")])
    assert int(np.load(b / "mean.npz")["samples"]) == 1
