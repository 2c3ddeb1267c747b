"""CLI of the multigrid updater's exact last level (2d-fluid-simulator_amd/main.py --mg-coarsest / --mg-direct-cells)."""
import csv
import importlib.util
import math
import os

import pytest
from conftest import REPO


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_multigrid_direct", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_refusals(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.mg_coarsest, a.mg_direct_cells) == (None, None)
    a = cli.build_parser().parse_args(["--pressure", "multigrid", "--mg-coarsest", "direct", "--mg-direct-cells", "512"])
    assert (a.pressure, a.mg_coarsest, a.mg_direct_cells) == ("multigrid", "direct", 512)
    assert cli.build_parser().parse_args(["--pressure", "multigrid", "--mg-coarsest", "sweeps"]).mg_coarsest == "sweeps"
    for argv in (["--mg-coarsest", "direct"], ["--pressure", "rbsor", "--mg-coarsest", "direct"], ["--mg-direct-cells", "512"],
                 ["--pressure", "rbsor", "--mg-direct-cells", "512"], ["--pressure", "multigrid", "--mg-coarsest", "lu"],
                 ["--pressure", "multigrid", "--mg-coarsest", "direct", "--mg-direct-cells", "0"],
                 ["--pressure", "multigrid", "--mg-coarsest", "direct", "-res", "33"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2, argv


@pytest.mark.gpu
def test_at_res_100_the_direct_solve_ends_below_the_sweeps_below_rbsor(tmp_path, hip_lib):
    """The same 60 steps of scene 5 at res 100 (upwind, no vorticity confinement) three ways.  rms Poisson residual over the FLUID cells at
    step 60 in the CPU restatement (f32): direct 8.3e-5, 64 sweeps on the 50 x 25 last level 2.3e-3, RB-SOR(1.3, 2) 3.7e-2 - factors of 28
    and 16.  The CLI's column is the rms over the not-wall cells, inflow and outflow included, which no updater relaxes: measured on the GPU
    2.7e-3, 7.8e-2 and 1.3e-1."""
    cli = _cli()
    last = {}
    for kind, extra in (("rbsor", ["--pressure", "rbsor"]), ("sweeps", ["--pressure", "multigrid"]),
                        ("direct", ["--pressure", "multigrid", "--mg-coarsest", "direct"])):
        out = tmp_path / kind
        cli.main("-bc 5 -res 100 -vc 0 -scheme upwind".split() + ["--steps", "60", "--stats-every", "20", "--out", str(out)] + extra)
        with open(out / "stats.csv") as f:
            rows = list(csv.reader(f))
        assert rows[0][-1] == "p_residual" and [int(r[0]) for r in rows[1:]] == [0, 20, 40, 60]
        for r in rows[1:]:
            assert math.isfinite(float(r[-1])) and int(dict(zip(rows[0], r))["nonfinite"]) == 0, (kind, r)
        last[kind] = float(rows[-1][-1])
    print("p_residual after 60 steps:", last)
    assert 0.0 < last["direct"] < last["sweeps"] < last["rbsor"]
