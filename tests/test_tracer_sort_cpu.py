"""The host side of the tracer sort and the per-cell tracer fields, without a device: fs.tracers.sort_key / SORT_BIN_CELLS /
residence_map, the NumPy reference of the fields (tests/tracer_fields_ref.py), the command-line flags, and what the compiler made of the
kernels (csrc/fs_tracer.h): the advance must keep its 8 waves per SIMD with the slot -> seed index array in its arguments."""
import importlib.util
import os
import re

import numpy as np
import pytest
from conftest import REPO
from test_build_metadata import kernels  # noqa: F401  (the fixture that reads the code objects of the built library)
from tracer_fields_ref import assert_order_contract, fields_ref


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_main_tracer_sort", os.path.join(REPO, "2d-fluid-simulator_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- sort_key -----------------------------------------------------------------------------------------------------------------------------
def test_sort_bin_cells_is_the_headers_constant():
    from fs.tracers import SORT_BIN_CELLS
    assert isinstance(SORT_BIN_CELLS, int) and SORT_BIN_CELLS > 0
    text = open(os.path.join(REPO, "include", "fs_hip.h")).read()
    assert int(re.search(r"#define FS_TRACER_SORT_BIN_CELLS (\d+)", text).group(1)) == SORT_BIN_CELLS
    src = open(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "fs_tracer.h")).read()
    assert int(re.search(r"constexpr int TRACER_SORT_W = (\d+);", src).group(1)) == SORT_BIN_CELLS


def test_sort_key_on_bin_edges():
    from fs.tracers import SORT_BIN_CELLS as W, sort_key
    X, Y = 4 * W, 8
    nb = 4
    below = np.nextafter(np.float64(W), 0.0)
    x = np.array([0.0, below, W, W + 0.5, 2.0 * W, X - 0.25, 0.5, 0.5], np.float64)
    y = np.array([0.0, 0.0, 0.0, 0.999, 1.0, Y - 0.5, np.nextafter(3.0, 0.0), 3.0], np.float64)
    key = sort_key(x, y, np.zeros(8, np.int32), X, Y)
    assert key.dtype == np.int64
    assert key.tolist() == [0, 0, 1, 1, nb + 2, (Y - 1) * nb + 3, 2 * nb, 3 * nb]


def test_sort_key_odd_width_with_a_partial_last_bin():
    from fs.tracers import SORT_BIN_CELLS as W, sort_key
    X, Y = 2 * W + 5, 3               # NB = 3: the last bin holds 5 cells
    nb = 3
    x = np.array([0.5, W - 0.5, W + 0.5, 2 * W + 0.5, X - 0.5, X - 0.5], np.float64)
    y = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 2.5], np.float64)
    assert sort_key(x, y, np.zeros(6, np.int32), X, Y).tolist() == [0, 0, 1, 2, 2, 2 * nb + 2]
    assert sort_key([X - 0.5], [Y - 0.5], [0], X, Y)[0] == Y * nb - 1        # the largest key of a particle inside
    assert sort_key([0.5], [0.5], [0], W, 1).tolist() == [0] and sort_key([0.5], [0.5], [1], W, 1).tolist() == [1]


def test_sort_key_dead_outside_and_nan_go_last():
    from fs.tracers import SORT_BIN_CELLS as W, sort_key
    X, Y = 101, 51
    nb = -(-X // W)
    x = np.array([5.5, 5.5, 5.5, -0.5, 101.0, 5.5, 5.5, np.nan, 5.5, np.inf, 5.5], np.float64)
    y = np.array([5.5, 5.5, 5.5, 5.5, 5.5, -1e-9, 51.0, 5.5, np.nan, 5.5, 5.5], np.float64)
    status = np.array([1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)
    key = sort_key(x, y, status, X, Y)
    assert key[:10].tolist() == [Y * nb] * 10 and key[10] == 5 * nb


def test_order_contract_helper_rejects_what_it_should():
    from fs.tracers import SORT_BIN_CELLS as W
    X, Y = 2 * W, 4
    good = {"x": np.array([0.5, W + 0.5, 0.5, 0.5]), "y": np.array([0.5, 0.5, 1.5, 0.5]), "status": np.array([0, 0, 0, 2], np.int32),
            "id": np.array([3, 0, 1, 2], np.int32)}
    assert assert_order_contract(good, X, Y).tolist() == [0, 1, 2, 8]
    for bad in (dict(good, id=np.array([3, 0, 1, 1], np.int32)),                                  # no permutation
                dict(good, x=np.array([W + 0.5, 0.5, 0.5, 0.5])),                                  # keys 1, 0, 2
                dict(good, status=np.array([2, 0, 0, 0], np.int32))):                              # a dead particle in front
        with pytest.raises(AssertionError):
            assert_order_contract(bad, X, Y)


# ---- residence_map and the reference of the fields ----------------------------------------------------------------------------------------
def test_residence_map_by_hand():
    from fs.tracers import residence_map
    count = np.array([[0, 1], [2, 4]], np.int32)
    age_sum = np.array([[0, 7], [5, 2 ** 40]], np.int64)
    r = residence_map(count, age_sum, 0.25)
    assert r.dtype == np.float64 and r.shape == (2, 2)
    assert np.isnan(r[0, 0]) and r[0, 1] == 1.75 and r[1, 0] == 0.625 and r[1, 1] == 2.0 ** 36
    assert np.isnan(residence_map(np.zeros((3, 2), np.int32), np.zeros((3, 2), np.int64), 1.0)).all()
    with pytest.raises(ValueError):
        residence_map(count, age_sum[:1], 0.25)


def test_fields_reference_counts_alive_inside_particles_only():
    X, Y = 5, 4
    state = {"x": np.array([0.5, 0.75, 4.999, 2.0, 2.5, -0.5, 5.0, np.nan, 1.5]),
             "y": np.array([0.5, 0.25, 3.999, 1.0, 1.5, 1.0, 1.0, 1.0, 4.0]),
             "age": np.array([3, 4, 2 ** 30, 1, 2 ** 30, 9, 9, 9, 9], np.int32),
             "status": np.array([0, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)}
    count, age_sum = fields_ref(state, X, Y)
    assert count.dtype == np.int32 and age_sum.dtype == np.int64 and count.shape == age_sum.shape == (X, Y)
    exp_c = np.zeros((X, Y), np.int32)
    exp_c[0, 0], exp_c[4, 3], exp_c[2, 1] = 2, 1, 2
    exp_a = np.zeros((X, Y), np.int64)
    exp_a[0, 0], exp_a[4, 3], exp_a[2, 1] = 7, 2 ** 30, 2 ** 30 + 1
    assert np.array_equal(count, exp_c) and np.array_equal(age_sum, exp_a)
    state["status"][[1, 4]] = (2, 3)                     # dead particles leave the fields
    count, age_sum = fields_ref(state, X, Y)
    assert count[0, 0] == 1 and age_sum[0, 0] == 3 and count[2, 1] == 1 and age_sum[2, 1] == 1 and count.sum() == 3
    big = {"x": np.full(3, 1.5), "y": np.full(3, 1.5), "age": np.full(3, 2 ** 30, np.int32), "status": np.zeros(3, np.int32)}
    assert fields_ref(big, X, Y)[1][1, 1] == 3 * 2 ** 30 > np.iinfo(np.int32).max


def test_tracers_object_keeps_its_positional_signature_and_schedules():
    from fs.tracers import KEYS, Tracers

    class _Dev:
        sorted = 0

        def tracer_sort(self, set_):
            self.sorted += 1

    class _Set:
        serial = 7
    dev = _Dev()
    t = Tracers(dev, _Set(), np.zeros((2, 2)), True, 5)
    assert (t.respawn, t.max_age, t.sort_every, t.token) == (True, 5, 0, ("tracer", 7)) and t.to_next_sort() is None and not t.due()
    t = Tracers(dev, _Set(), np.zeros((2, 2)), False, 0, 8)
    assert t.sort_every == 8 and t.to_next_sort() == 8 and not t.due()      # (nothing issued yet: nothing to sort)
    t.issued = 5
    assert t.to_next_sort() == 3 and not t.due()
    t.issued = 16
    assert t.to_next_sort() == 8 and t.due()
    t.sort()
    assert dev.sorted == 1 and t.sorts == 1 and not t.due()
    assert KEYS == ("x", "y", "age", "status", "respawns", "seeds", "steps")


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_need_tracers(tmp_path):
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert (a.tracer_sort_every, a.tracer_fields, a.tracer_fields_file) == (0, False, None)
    a = cli.build_parser().parse_args(["--tracers", "100", "--tracer-sort-every", "32", "--tracer-fields", "--tracer-fields-file", "f.npz"])
    assert (a.tracers, a.tracer_sort_every, a.tracer_fields, a.tracer_fields_file) == (100, 32, True, "f.npz")
    for argv in (["--tracer-sort-every", "32"],                    # without --tracers / --tracer-line
                 ["--tracer-fields"],
                 ["--tracer-fields-file", str(tmp_path / "f.npz")],
                 ["--tracers", "10", "--tracer-sort-every", "-1"],
                 ["--tracers", "10", "--tracer-sort-every", "x"],
                 ["--tracers", "10", "--tracer-fields-file", str(tmp_path / "f.npz")]):      # the file without --tracer-fields
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--out", str(tmp_path)])
        assert e.value.code == 2, argv


def test_abi_table_holds_the_new_entries():
    from fs import _lib
    assert _lib.ABI_VERSION >= 14
    for name in ("fs_tracer_sort", "fs_tracer_order", "fs_tracer_fields"):
        assert name in _lib.EXPORTS, name


# ---- build metadata -----------------------------------------------------------------------------------------------------------------------
def _pick(kernels, pattern):
    got = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert got, pattern
    return got


def test_advance_keeps_eight_waves_per_simd_without_scratch(kernels):  # noqa: F811
    """512 VGPRs per SIMD lane: 8 waves need <= 64 each.  All four instantiations (f32 / f64, with and without the deferred limit)."""
    got = _pick(kernels, r"16k_tracer_advanceI[fd]Lb[01]E")
    assert len(got) == 4, sorted(got)
    for name, k in got.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)


@pytest.mark.parametrize("pattern", [r"19k_tracer_sort_countE", r"20k_tracer_scan_blocksE", r"18k_tracer_scan_sumsE", r"17k_tracer_scan_addE",
                                     r"21k_tracer_sort_scatterE", r"18k_tracer_sort_copyE", r"15k_tracer_fieldsE"])
def test_sort_and_field_kernels_have_no_scratch(kernels, pattern):  # noqa: F811
    for name, k in _pick(kernels, pattern).items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)
