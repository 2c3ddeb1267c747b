"""CLI tracer particles (2d-fluid-simulator_amd/main.py --tracers / --tracer-line / --tracer-once / --tracer-max-age / --tracer-file /
--tracer-dump-every, the particle state in --save-state / --load-state, the overlay in the -vis frames)."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

KEYS = ["age", "respawns", "seeds", "status", "steps", "x", "y"]


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_tracers", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.tracers, a.tracer_seed, a.tracer_line, a.tracer_once, a.tracer_max_age, a.tracer_file, a.tracer_dump_every) == (0, None, [], False, None, None, 0)
    a = cli.build_parser().parse_args(["--tracers", "500", "--tracer-seed", "3", "--tracer-line", "1.5,0.5,1.5,30.5,16", "--tracer-line", "4,4,9,9,2",
                                       "--tracer-once", "--tracer-max-age", "90", "--tracer-file", "t.npz", "--tracer-dump-every", "10"])
    assert (a.tracers, a.tracer_seed, a.tracer_once, a.tracer_max_age, a.tracer_file, a.tracer_dump_every) == (500, 3, True, 90, "t.npz", 10)
    assert a.tracer_line == ["1.5,0.5,1.5,30.5,16", "4,4,9,9,2"]
    for argv in (["--tracer-seed", "4"],                         # without --tracers / --tracer-line
                 ["--tracer-once"],
                 ["--tracer-max-age", "5"],
                 ["--tracer-file", str(tmp_path / "t.npz")],
                 ["--tracer-dump-every", "5"],
                 ["--tracers", "-1"],
                 ["--tracers", "x"],
                 ["--tracers", "10", "--tracer-max-age", "-2"],
                 ["--tracer-line", "1,2,3,4"],
                 ["--tracer-line", "1,2,3,4,0"],
                 ["--tracer-line", "1,2,3,4,5,6"],
                 ["--tracer-line", "a,2,3,4,5"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2, argv


def test_seeds_from_the_flags_and_dropped_wall_seeds():
    cli = _cli()
    mask = np.zeros((16, 8), np.uint8)
    mask[4:6, :4] = 1
    seeds, notes = cli.tracer_seeds(mask, 20, 3, [(0.5, 1.5, 15.5, 1.5, 16), (0.5, 6.5, 15.5, 6.5, 4)])
    assert seeds.shape == (20 + 14 + 4, 2) and seeds.dtype == np.float64
    assert len(notes) == 1 and "dropped 2 of 16 seeds" in notes[0] and "--tracer-line 0.5,1.5,15.5,1.5,16" in notes[0]
    again, _ = cli.tracer_seeds(mask, 20, 3, [])
    other, _ = cli.tracer_seeds(mask, 20, 4, [])
    assert np.array_equal(again, seeds[:20]) and not np.array_equal(other, again)
    none, notes = cli.tracer_seeds(mask, 0, 0, [(4.5, 0.5, 5.5, 3.5, 3)])
    assert none.shape == (0, 2) and "dropped 3 of 3" in notes[0]


def test_checkpoint_with_other_parameters_is_refused(tmp_path, capsys):
    """--load-state of a checkpoint whose tracers ran with another respawn / max_age: message and exit status 2, before any device work."""
    from fs.tracers import Tracers
    cli = _cli()
    ck = tmp_path / "ck.npz"
    n = 4
    np.savez(str(ck), step=np.array(10), **{"tracer.x": np.ones(n), "tracer.y": np.ones(n), "tracer.age": np.zeros(n, np.int32),
                                            "tracer.status": np.zeros(n, np.int32), "tracer.respawns": np.zeros(n, np.int32),
                                            "tracer.seeds": np.ones((n, 2)), "tracer.steps": np.array(10), "tracer.respawn": np.array(True),
                                            "tracer.max_age": np.array(50)})
    assert Tracers.held(np.load(str(ck))) == (True, 50, 4)
    for argv in (["--tracers", "4"], ["--tracers", "4", "--tracer-max-age", "50", "--tracer-once"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--load-state", str(ck), "--out", str(tmp_path)])
        assert e.value.code == 2
        assert "--tracer-max-age 50" in capsys.readouterr().err
    plain = tmp_path / "plain.npz"
    np.savez(str(plain), step=np.array(10))
    assert Tracers.held(np.load(str(plain))) is None


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_tracer_files_overlay_and_resume(graph, tmp_path, capsys, hip_lib):
    import fs
    from fs.tracers import fluid_only, seed_line, seed_random
    cli = _cli()
    res = 64
    line = "1.5,0.5,1.5,63.5,64"
    common = ["-bc", "5", "-res", str(res), "--tracers", "300", "--tracer-seed", "9", "--tracer-line", line] + (["--graph"] if graph else [])
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    cli.main(common + ["--steps", "21", "--out", str(a), "--tracer-dump-every", "7", "-vis", "2", "--frame-every", "21"])
    said = capsys.readouterr().out
    assert f"--tracer-line {line}: dropped" in said and "of 64 seeds" in said          # (the wall seeds of the line are reported)
    t = np.load(a / "tracers.npz")
    assert sorted(t.files) == KEYS and int(t["steps"]) == 21
    for k in (7, 14, 21):
        d = np.load(a / f"tracers_{k:06}.npz")
        assert sorted(d.files) == KEYS and int(d["steps"]) == k
    assert all(np.array_equal(np.load(a / "tracers_000021.npz")[k], t[k]) for k in KEYS)
    assert (a / "000000.png").exists()
    # the same run through the facade
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(5, res, 0.05 / res, 1.0 / res, 1e6, 5.0, "cip")
    try:
        mask = np.asarray(sim._solver._bc.mask)
        kept, dropped = fluid_only(mask, seed_line((1.5, 0.5), (1.5, 63.5), 64))
        assert dropped > 0
        seeds = np.concatenate([seed_random(mask, 300, 9), kept])
        sim.seed_tracers(seeds)
        sim.run(21, graph=graph)
        exp = sim.tracers()
        # the frame carries the overlay: white pixels where the particles are
        img = cli.frame(sim, 2)
        cells = np.floor(np.stack([exp["x"], exp["y"]], 1)).astype(int)
        assert np.all(img[cells[:, 0], cells[:, 1]] == 1.0)
    finally:
        sim._solver._bc.device.close()
    for k in KEYS:
        assert np.array_equal(t[k], exp[k]), k
    assert np.hypot(t["x"] - t["seeds"][:, 0], t["y"] - t["seeds"][:, 1]).max() > 0.5
    # the same 21 steps over a restart: the particles travel with the checkpoint
    b.mkdir()
    cli.main(common + ["--steps", "9", "--out", str(b), "--save-state", str(b / "ck.npz")])
    assert int(np.load(b / "tracers.npz")["steps"]) == 9
    cli.main(common + ["--steps", "12", "--out", str(b), "--load-state", str(b / "ck.npz")])
    r = np.load(b / "tracers.npz")
    for k in KEYS:
        assert np.array_equal(r[k], t[k]), f"{k}: the resumed particles differ from the uninterrupted run's"
    # --tracer-once with a maximum age: nothing respawns, everything still alive expires at that age
    cli.main(["-bc", "5", "-res", str(res), "--tracers", "100", "--tracer-once", "--tracer-max-age", "6", "--steps", "8", "--out", str(c),
              "--tracer-file", str(c / "once.npz")] + (["--graph"] if graph else []))
    o = np.load(c / "once.npz")
    assert not (c / "tracers.npz").exists() and not o["respawns"].any() and np.all(o["status"] != 0) and (o["status"] == 3).any()
    assert o["age"].max() == 6 and int(o["steps"]) == 8
    # a checkpoint without particles seeds fresh ones
    cli.main(["-bc", "5", "-res", str(res), "--steps", "3", "--out", str(c), "--save-state", str(c / "plain.npz")])
    cli.main(common + ["--steps", "4", "--out", str(c), "--load-state", str(c / "plain.npz")])
    assert int(np.load(c / "tracers.npz")["steps"]) == 4
