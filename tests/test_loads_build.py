"""What the compiler made of the body-load kernels (csrc/fs_loads.h), read from the code objects inside the built libfs_hip.so (no GPU
needed): they hold six running sums per lane and must keep them in registers - no scratch."""
import re

from test_build_metadata import kernels  # noqa: F401 - the module-scoped fixture that reads the code objects


def test_loads_kernels_use_no_scratch(kernels):  # noqa: F811
    got = {k: v for k, v in kernels.items() if re.search(r"k_loads_(one|faces|record)", k)}
    names = " ".join(got)
    for kernel in ("k_loads_oneIf", "k_loads_oneId", "k_loads_facesIf", "k_loads_facesId", "k_loads_record"):
        assert kernel in names, f"{kernel} is not in the library"
    for name, k in got.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)          # (small gathers: nothing here should need more than a quarter of the file)
        assert k["lds"] <= 6 * 4 * 8, (name, k)
