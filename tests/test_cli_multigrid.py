"""CLI of the multigrid pressure updater (2d-fluid-simulator_amd/main.py --pressure / --mg-cycles; the p_residual column of --stats-every)."""
import csv
import importlib.util
import math
import os

import pytest
from conftest import REPO

OLD_HEADER = ["step", "time", "kinetic_energy", "enstrophy", "max_speed", "cfl", "div_rms", "div_max", "nonfinite", "fluid_cells"]


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_multigrid", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.pressure, a.mg_cycles) == (None, None)
    a = cli.build_parser().parse_args(["--pressure", "multigrid", "--mg-cycles", "3"])
    assert (a.pressure, a.mg_cycles) == ("multigrid", 3)
    for argv in (["--mg-cycles", "2"], ["--pressure", "rbsor", "--mg-cycles", "2"], ["--pressure", "multigrid", "--mg-cycles", "0"],
                 ["--pressure", "vcycle"], ["--pressure", "multigrid", "-res", "33"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2, argv


@pytest.mark.gpu
def test_multigrid_runs_and_its_residual_falls_below_rbsor(tmp_path, hip_lib):
    """The same 40 steps of scene 5 (upwind, dye, no vorticity confinement) with either updater: both CSVs carry the p_residual column, and
    the multigrid run's last value lies below the red-black run's (CPU restatement: 6.0e-2 against 2.5e-1)."""
    cli = _cli()
    last = {}
    for kind, extra in (("rbsor", []), ("multigrid", ["--mg-cycles", "1"])):
        out = tmp_path / kind
        cli.main("-bc 5 -res 32 -vc 0 -scheme upwind".split() + ["--steps", "40", "--stats-every", "20", "--out", str(out), "--pressure", kind] + extra)
        rows = _rows(out / "stats.csv")
        assert rows[0] == OLD_HEADER + ["p_residual"]
        assert [int(r[0]) for r in rows[1:]] == [0, 20, 40]
        last[kind] = float(rows[-1][-1])
        assert math.isfinite(last[kind]) and int(dict(zip(rows[0], rows[-1]))["nonfinite"]) == 0
    print("p_residual after 40 steps:", last)
    assert 0.0 < last["multigrid"] < last["rbsor"]


@pytest.mark.gpu
def test_without_the_flag_the_header_is_the_old_one(tmp_path, hip_lib):
    cli = _cli()
    cli.main("-bc 5 -res 32 -vc 0".split() + ["--steps", "4", "--stats-every", "4", "--out", str(tmp_path)])
    assert _rows(tmp_path / "stats.csv")[0] == OLD_HEADER
