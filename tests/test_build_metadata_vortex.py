"""What the compiler made of the vortex kernels (csrc/fs_vortex.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): the flag pass exists for both field types in both forms (flag plane, criterion field), the
reduction for both field types, the untemplated kernels once each, and none of them may use scratch.  No VGPR bound is asserted; DESIGN.md 4ai
records the counts."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)


def test_templated_kernels_are_built_for_both_field_types_without_scratch(kernels):      # noqa: F811
    flags = {k: v for k, v in kernels.items() if re.search(r"\d+k_vortex_flagsI", k)}
    assert len(flags) == 4, sorted(flags)
    for t in "fd":
        for form in "01":
            assert any(re.search(rf"k_vortex_flagsI{t}Lb{form}E", n) for n in flags), (t, form)
    reduce = {k: v for k, v in kernels.items() if re.search(r"\d+k_vortex_reduceI", k)}
    assert len(reduce) == 2, sorted(reduce)
    for t in "fd":
        assert any(re.search(rf"k_vortex_reduceI{t}E", n) for n in reduce), t
    for name, k in sorted({**flags, **reduce}.items()):
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)


def test_labelling_and_record_kernels_are_built_without_scratch(kernels):      # noqa: F811
    for kern in ("k_vortex_local", "k_vortex_seam", "k_vortex_compress", "k_vortex_scan", "k_vortex_ids", "k_vortex_records", "k_vortex_tick"):
        got = {n: k for n, k in kernels.items() if re.search(rf"\d+{kern}E", n)}
        assert len(got) == 1, (kern, sorted(got))
        for name, k in got.items():
            print(name, k)
            assert k["scratch"] == 0, (name, k)
            assert k["lds"] == (32 * 8 * 5 if kern == "k_vortex_local" else k["lds"]), (name, k)      # the tile: an int and a flag byte per cell
