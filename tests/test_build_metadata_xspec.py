"""What the compiler made of the cross-spectrum kernels (csrc/fs_xspec.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): the load pass exists for both field types, without scratch and with exactly the LDS of
fs_spec.h's row kernels - the re and the im plane of a chunk; the accumulate pass exists once, without scratch and without LDS.  Only the
metadata is read."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)
from test_build_metadata_spec import _lds_bytes


def test_load_pass_is_built_for_both_field_types_without_scratch(kernels):      # noqa: F811
    load = {k: v for k, v in kernels.items() if re.search(r"\d+k_xspec_load_rowsI", k)}
    assert len(load) == 2, sorted(load)
    for t in "fd":
        assert any(re.search(rf"k_xspec_load_rowsI{t}E", n) for n in load), t
    for name, k in sorted(load.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == _lds_bytes(), (name, k)


def test_accumulate_pass_is_built_once_without_scratch_or_lds(kernels):      # noqa: F811
    got = {n: k for n, k in kernels.items() if re.search(r"\d+k_xspec_accumulateE", n)}
    assert len(got) == 1, sorted(got)
    for name, k in got.items():
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
