"""What the compiler made of the harmonic-mode kernels (csrc/fs_modes.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): k_modes_accumulate carries 3 to 9 planes of double per field and row group in registers
- the split into one pass per field and the rows per group were chosen per frequency count so that no instantiation spills: scratch is paid
for by every workgroup of a launch that sits in every replayed step.  No VGPR bound is asserted; DESIGN.md 4ae records the counts."""
import re

import pytest
from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)


def _instantiations(kernels, name):      # noqa: F811
    return {k: v for k, v in kernels.items() if re.search(r"\d+" + name + "I", k)}


def test_every_accumulate_instantiation_is_built_without_scratch(kernels):      # noqa: F811
    got = _instantiations(kernels, "k_modes_accumulate")
    # T in (float, double) x W in (1, 2) x K in (1 .. 4)
    assert len(got) == 16, sorted(got)
    for t in "fd":
        for w in (1, 2):
            for k in (1, 2, 3, 4):
                assert any(re.search(rf"k_modes_accumulateI{t}Li{w}ELi{k}E", n) for n in got), (t, w, k)
    for name, k in sorted(got.items()):
        print(name, k)
        assert k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("name,count", [("k_modes_combine", 4)])
def test_combine_instantiations_exist(kernels, name, count):      # noqa: F811
    assert len(_instantiations(kernels, name)) == count
    assert any("k_modes_tick" in k for k in kernels)
