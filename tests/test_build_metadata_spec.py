"""What the compiler made of the spectrum kernels (csrc/fs_spec.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): the load pass exists for both field types, the untemplated kernels once each; none may
use scratch, and the row kernels hold exactly the LDS fs_spec.h derives for them - the re and the im plane of a chunk.  No VGPR bound is
asserted; DESIGN.md 4ak records the counts."""
import ctypes
import os
import re

from conftest import REPO
from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)

TILE = 32


def _lds_bytes():
    lib = ctypes.CDLL(os.path.join(REPO, "2d-fluid-simulator_amd", "csrc", "libfs_spec_host.so"))
    a, b, c, d = (ctypes.c_int() for _ in range(4))
    lib.fs_spec_host_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
    assert d.value == 2 * c.value * 8
    return d.value


def test_load_pass_is_built_for_both_field_types_without_scratch(kernels):      # noqa: F811
    load = {k: v for k, v in kernels.items() if re.search(r"\d+k_spec_load_rowsI", k)}
    assert len(load) == 2, sorted(load)
    for t in "fd":
        assert any(re.search(rf"k_spec_load_rowsI{t}E", n) for n in load), t
    for name, k in sorted(load.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == _lds_bytes(), (name, k)


def test_untemplated_kernels_are_built_once_without_scratch(kernels):      # noqa: F811
    for kern, lds in (("k_spec_rows", _lds_bytes()), ("k_spec_transpose", 2 * TILE * (TILE + 1) * 8), ("k_spec_power", 0), ("k_spec_tick", 0)):
        got = {n: k for n, k in kernels.items() if re.search(rf"\d+{kern}E", n)}
        assert len(got) == 1, (kern, sorted(got))
        for name, k in got.items():
            print(name, k)
            assert k["scratch"] == 0 and k["lds"] == lds, (name, k)
