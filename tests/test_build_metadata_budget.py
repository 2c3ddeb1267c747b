"""What the compiler made of the budget kernels (csrc/fs_budget.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): k_budget_accumulate exists for both field types and both widths; every k_budget_* kernel
is built without scratch - the 84 VGPRs of accumulators a lane holds at once stay in registers - and holds exactly the LDS the header
declares (the figure libfs_budget_host.so exports: none).  Only the metadata is read; no register count is asserted."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)
from test_budget_cpu import limits


def test_the_accumulate_kernel_is_built_for_both_field_types(kernels):      # noqa: F811
    acc = {k: v for k, v in kernels.items() if re.search(r"\d+k_budget_accumulateI", k)}
    assert len(acc) == 4, sorted(acc)
    for t in "fd":
        for w in "12":
            assert any(re.search(rf"k_budget_accumulateI{t}Li{w}E", n) for n in acc), (t, w)


def test_every_budget_kernel_is_built_without_scratch_and_with_the_declared_lds(kernels):      # noqa: F811
    got = {n: k for n, k in kernels.items() if re.search(r"\d+k_budget_", n)}
    names = {re.search(r"\d+(k_budget_[a-z]+)", n).group(1) for n in got}
    assert names == {"k_budget_accumulate", "k_budget_tick"} and len(got) == 5, sorted(got)
    lds = limits()["lds_bytes"]
    for name, k in sorted(got.items()):
        print(name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] == lds, (name, k)
    assert lds == 0
