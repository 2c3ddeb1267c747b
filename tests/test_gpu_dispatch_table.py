"""Which kernel runs for which input, against a recording (tests/golden/launch_kernels.json, written by tools/record_launch_kernels.py at the commit
before the launch sites' macro ladders became the typed dispatch of csrc/fs_pick.h): per configuration, 3 steps with profiling on must launch the same
__global__ symbols under the same launch names and leave bit-identical fields.  A launch site that picks another instantiation for some input - another
tile height, division mode, parity, plain / masked body - shows here by name; re-record only with a change that means to alter the selection."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, REPO

_spec = importlib.util.spec_from_file_location("record_launch_kernels", os.path.join(REPO, "tools", "record_launch_kernels.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(GOLDEN, "launch_kernels.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recording_holds_the_recorders_list():
    assert RECORDED["steps"] == recorder.STEPS
    keys = ("id", "dtype", "bc", "dye", "scheme", "res", "updater", "vc", "env", "dx")
    assert [{k: r[k] for k in keys} for r in RECORDED["configurations"]] == recorder.configurations()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", RECORDED["configurations"], ids=[r["id"] for r in RECORDED["configurations"]])
def test_same_kernels_and_fields_as_recorded(rec, hip_lib):
    got = recorder.run(rec)
    assert got["kernels"] == rec["kernels"]
    assert got["digests"] == rec["digests"]
