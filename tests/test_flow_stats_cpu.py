"""Flow diagnostics without a GPU: the NumPy restatement (tests/flow_stats_ref.py) on closed forms, and the product's slab combination
(fs.runtime.DeviceBase.flow_stats: depth-1 exchange, sums over ranks, NaN-safe maxima) on 2 and 3 gloo ranks of the CPU stand-in device,
against the single-domain value.  Every rank's ghost rows of v and p are made stale (NaN, validity 0) before the call: the workers check that
the local sums read NaN without the exchange and that flow_stats exchanged them."""
import math
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp
from flow_stats_ref import flow_stats_ref


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rotation(X, Y, dx):
    i, j = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), indexing="ij")
    v = np.stack([-(j * dx), i * dx], axis=2)
    mask = np.ones((X, Y), np.uint8)
    mask[1:-1, 1:-1] = 0             # fluid only away from the domain edge: no clamped stencil
    return v, mask


def test_solid_body_rotation_is_exact():
    dx = 1.0 / 32
    v, mask = _rotation(64, 32, dx)
    d = flow_stats_ref(v, np.zeros((64, 32)), mask, dx)
    n = 62 * 30
    assert d["fluid_cells"] == n
    assert d["sum_om2"] == 4.0 * n and d["sum_dv2"] == 0.0 and d["max_abs_dv"] == 0.0
    F = mask == 0
    s2 = (v[..., 0] ** 2 + v[..., 1] ** 2)[F]
    assert d["max_s2"] == s2.max() and d["nonfinite"] == 0


@pytest.mark.parametrize("L", [1, 3, 4])
def test_square_body_in_linear_pressure(L):
    dx, c = 1.0 / 16, 0.25
    X, Y = 32, 16
    mask = np.zeros((X, Y), np.uint8)
    mask[10:10 + L, 5:5 + L] = 1
    p = c * np.arange(X, dtype=np.float64)[:, None] * np.ones((1, Y))
    d = flow_stats_ref(np.zeros((X, Y, 2)), p, mask, dx, box=(8, 3, 10 + L + 2, 5 + L + 2))
    assert d["force_x"] == -(L + 1) * L * c * dx
    assert d["force_y"] == 0.0
    d = flow_stats_ref(np.zeros((X, Y, 2)), np.full((X, Y), 3.5), mask, dx, box=(0, 0, X, Y))
    assert d["force_x"] == 0.0 and d["force_y"] == 0.0
    d = flow_stats_ref(np.zeros((X, Y, 2)), p, mask, dx)           # no box: no force
    assert d["force_x"] == 0.0 and d["force_y"] == 0.0


def test_nan_reaches_sums_maxima_and_count():
    dx = 1.0 / 32
    v, mask = _rotation(64, 32, dx)
    p = np.zeros((64, 32))
    p[20, 10] = np.nan                      # fluid cell: counted, but p enters no sum
    p[0, 0] = np.nan                        # wall cell: not counted
    d = flow_stats_ref(v, p, mask, dx)
    assert d["nonfinite"] == 1 and math.isfinite(d["sum_s2"])
    v[20, 10, 0] = np.inf
    d = flow_stats_ref(v, p, mask, dx)
    assert d["nonfinite"] == 1 and d["sum_s2"] == math.inf and d["max_s2"] == math.inf
    v[20, 10, 1] = np.nan
    d = flow_stats_ref(v, p, mask, dx)
    assert math.isnan(d["sum_s2"]) and math.isnan(d["max_s2"]) and math.isnan(d["max_a"]) and math.isnan(d["sum_om2"])


def test_derived_dict():
    from fs.fluid_simulator import derive_flow_stats
    raw = {"fluid_cells": 4.0, "sum_s2": 8.0, "sum_om2": 2.0, "sum_dv2": 16.0, "max_s2": 9.0, "max_a": 2.0, "max_abs_dv": 3.0,
           "nonfinite": 0.0, "force_x": 1.5, "force_y": -0.5}
    d = derive_flow_stats(raw, 0.5, 0.25, True)
    assert d == {"kinetic_energy": 1.0, "enstrophy": 0.25, "max_speed": 3.0, "cfl": 1.0, "div_rms": 2.0, "div_max": 3.0, "nonfinite": 0,
                 "fluid_cells": 4, "force_x": 1.5, "force_y": -0.5}
    assert "force_x" not in derive_flow_stats(raw, 0.5, 0.25, False)
    assert math.isnan(derive_flow_stats(dict(raw, max_s2=math.nan), 0.5, 0.25, False)["max_speed"])


def test_default_body_boxes():
    from fs.boundary_condition import WALL, create_scene_arrays, default_body_box
    for bc in (1, 3, 5):
        for res in (32, 48, 400):
            x0, y0, x1, y1 = default_body_box(bc, res)
            mask = create_scene_arrays(bc, res)[1]
            X, Y = mask.shape
            assert 0 <= x0 < x1 <= X and 2 <= y0 < y1 <= Y - 2          # off the floor and ceiling rows
            inside = mask[x0:x1, y0:y1] == WALL
            assert inside.any()
            if bc == 5:
                assert x0 >= X // 2 + X // 64                           # the post array, not the slotted mid wall
    with pytest.raises(ValueError):
        default_body_box(2, 32)


SLAB_CASES = [
    ("traj_bc5_cip_vc5.npz", 2, 2, 5),
    ("traj_bc1_upwind_vc0.npz", 3, 2, 5),
    ("traj_bc3_kk_vc5.npz", 2, 4, 3),
    ("traj_f64_bc1_cip_vc0.npz", 3, 3, 4),
    ("traj_bc2_cip_vc5.npz", 3, 8, 4),
]


@pytest.mark.parametrize("fname,world,halo,steps", SLAB_CASES)
def test_slab_flow_stats_match_single_domain(fname, world, halo, steps, tmp_path):
    from flow_stats_slab_worker import run
    mp.spawn(run, args=(world, _free_port(), fname, halo, steps, str(tmp_path)), nprocs=world, join=True)
    nbad, msg = open(os.path.join(tmp_path, "result.txt")).read().split(" ", 1)
    assert int(nbad) == 0, f"{fname} on {world} slabs: {msg}"


@pytest.mark.parametrize("poison_rank", [0, 2])
def test_slab_flow_stats_nan_on_one_rank(poison_rank, tmp_path):
    from flow_stats_slab_worker import run
    mp.spawn(run, args=(3, _free_port(), "traj_bc5_cip_vc5.npz", 2, 3, str(tmp_path), poison_rank), nprocs=3, join=True)
    nbad, msg = open(os.path.join(tmp_path, "result.txt")).read().split(" ", 1)
    assert int(nbad) == 0, msg
