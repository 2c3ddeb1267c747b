"""What the compiler made of the flow-map kernels (csrc/fs_lcs.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): k_flowmap_advance holds the sixteen loads of a gather stage in flight, one node per lane -
it exists for both field types, and neither it nor the seed and Cauchy-Green kernels may use scratch.  No VGPR bound is asserted; DESIGN.md
4ah records the counts."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)


def test_both_advance_instantiations_are_built_without_scratch(kernels):      # noqa: F811
    got = {k: v for k, v in kernels.items() if re.search(r"\d+k_flowmap_advanceI", k)}
    assert len(got) == 2, sorted(got)
    for t in "fd":
        assert any(re.search(rf"k_flowmap_advanceI{t}E", n) for n in got), t
    for name, k in sorted(got.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)


def test_seed_and_cauchy_green_are_built_without_scratch(kernels):      # noqa: F811
    others = {n: k for n, k in kernels.items() if "k_flowmap_seed" in n or "k_flowmap_cauchy_green" in n}
    assert len(others) == 2, sorted(others)
    for name, k in sorted(others.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
