"""CLI flow diagnostics (2d-fluid-simulator_amd/main.py --stats-every / --body / --stop-on-nonfinite)."""
import csv
import importlib.util
import math
import os

import numpy as np
import pytest
from conftest import REPO


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_stats", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_flags_parse_and_need_stats_every(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.stats_every, a.stats_file, a.body, a.stop_on_nonfinite) == (0, None, None, False)
    with pytest.raises(SystemExit):
        cli.main(["--body", "auto", "--out", str(tmp_path)])
    with pytest.raises(SystemExit):
        cli.main(["--stats-every", "5", "--body", "1,2,3", "--out", str(tmp_path)])
    with pytest.raises(SystemExit):
        cli.main(["-bc", "2", "--stats-every", "5", "--body", "auto", "--out", str(tmp_path)])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_stats_csv_rows_and_last_row(graph, tmp_path, hip_lib):
    import fs
    cli = _cli()
    common = "-bc 5 -res 64 -vc 5".split()
    args = common + ["--steps", "20", "--stats-every", "5", "--out", str(tmp_path), "--save-state", str(tmp_path / "ck.npz"), "--body", "auto"]
    cli.main(args + (["--graph"] if graph else []))
    rows = _rows(tmp_path / "stats.csv")
    assert rows[0][:2] == ["step", "time"] and "kinetic_energy" in rows[0] and "force_x" in rows[0]
    assert [int(r[0]) for r in rows[1:]] == [0, 5, 10, 15, 20]
    last = dict(zip(rows[0], rows[-1]))
    # the saved state, loaded into a fresh simulator: its flow_stats() is the last row, value for value
    from fs.boundary_condition import default_body_box
    res = 64
    fs.runtime.init(gpu=0)
    sim = fs.DyeFluidSimulator.create(5, res, 0.05 / res, 1.0 / res, 1e6, 5.0, "cip")
    try:
        assert cli.load_state(sim, str(tmp_path / "ck.npz")) == 20
        d = sim.flow_stats(default_body_box(5, res))
    finally:
        sim._solver._bc.device.close()
    for k, x in d.items():
        assert float(last[k]) == x, k
    assert float(last["time"]) == 20 * (0.05 / res)


@pytest.mark.gpu
@pytest.mark.parametrize("bc", [1, 5])
def test_body_auto_gives_a_force(bc, tmp_path, hip_lib):
    cli = _cli()
    f = tmp_path / "s.csv"
    cli.main(["-bc", str(bc), "-res", "64", "--steps", "30", "--stats-every", "10", "--body", "auto", "--stats-file", str(f), "--out", str(tmp_path)])
    rows = _rows(f)
    last = dict(zip(rows[0], rows[-1]))
    fx = float(last["force_x"])
    assert math.isfinite(fx) and fx != 0.0
    assert int(last["nonfinite"]) == 0


@pytest.mark.gpu
def test_stop_on_nonfinite(tmp_path, capsys, hip_lib):
    cli = _cli()
    common = "-bc 2 -res 64 -vc 5".split()
    ck = tmp_path / "ck.npz"
    cli.main(common + ["--steps", "4", "--out", str(tmp_path), "--save-state", str(ck)])
    z = dict(np.load(ck))
    from fs.boundary_condition import create_scene_arrays
    mask = create_scene_arrays(2, 64)[1]
    i, j = np.argwhere(mask == 0)[len(np.argwhere(mask == 0)) // 2]
    z["p.current"] = z["p.current"].copy()
    z["p.current"][i, j] = np.nan                # a NaN prepared on the host in one fluid cell of the pressure
    bad = tmp_path / "bad.npz"
    np.savez(bad, **z)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(common + ["--steps", "10", "--out", str(tmp_path), "--load-state", str(bad), "--stats-every", "1", "--stop-on-nonfinite"])
    assert e.value.code == 3
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 1 and "step 4" in err[0] and "non-finite" in err[0]
    rows = _rows(tmp_path / "stats.csv")
    assert len(rows) == 2 and rows[1][0] == "4" and int(dict(zip(rows[0], rows[1]))["nonfinite"]) >= 1


@pytest.mark.gpu
def test_stdout_unchanged_without_the_flags(tmp_path, capsys, hip_lib):
    cli = _cli()
    cli.main("-bc 1 -res 64 --steps 6 --frame-every 3 --out".split() + [str(tmp_path)])
    out = capsys.readouterr().out.splitlines()
    assert out[:6] == ["Boundary Condition: 1", f"dt: {0.05 / 64}", "Re: 1000000.0", "Resolution: 64", "Scheme: cip",
                       "Vorticity confinement: 5.0"]
    assert len(out) == 7 and out[6].startswith("6 steps in ") and out[6].endswith(" steps/s")
    assert sorted(os.listdir(tmp_path)) == ["000000.png", "000003.png"]
