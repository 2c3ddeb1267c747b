"""What the compiler made of the distribution kernels (csrc/fs_dist.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): the accumulation exists for both field types in both forms (1-D, joint), the value pass
for both field types, the untemplated kernels once each; none may use scratch, and every one holds exactly the LDS its table needs.  No VGPR
bound is asserted; DESIGN.md 4aj records the counts."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)

MAX_BINS, TAILS, DIGITS = 4096, 4, 2048


def test_templated_kernels_are_built_for_both_field_types_without_scratch(kernels):      # noqa: F811
    acc = {k: v for k, v in kernels.items() if re.search(r"\d+k_dist_accumulateI", k)}
    assert len(acc) == 4, sorted(acc)
    for t in "fd":
        for joint in "01":
            assert any(re.search(rf"k_dist_accumulateI{t}Lb{joint}E", n) for n in acc), (t, joint)
    for name, k in sorted(acc.items()):
        print(name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] == 4 * (MAX_BINS + TAILS), (name, k)      # the private table of 32-bit counters and its tail words, nothing else
    values = {k: v for k, v in kernels.items() if re.search(r"\d+k_dist_valuesI", k)}
    assert len(values) == 2, sorted(values)
    for t in "fd":
        assert any(re.search(rf"k_dist_valuesI{t}E", n) for n in values), t
    for name, k in sorted(values.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 2 * 4, (name, k)      # the two counters of the workgroup


def test_untemplated_kernels_are_built_once_without_scratch(kernels):      # noqa: F811
    for kern, lds in (("k_dist_digits", 4 * DIGITS), ("k_dist_tick", 0)):
        got = {n: k for n, k in kernels.items() if re.search(rf"\d+{kern}E", n)}
        assert len(got) == 1, (kern, sorted(got))
        for name, k in got.items():
            print(name, k)
            assert k["scratch"] == 0 and k["lds"] == lds, (name, k)
