"""What the compiler made of the snapshot-POD kernels (csrc/fs_pod.h), read from the code objects inside the built libfs_hip.so as
tests/test_build_metadata.py does (no GPU needed): k_pod_gram holds a tile of 8 x 8 sums of double per lane - 128 registers of accumulators
beside the loaded row - and k_pod_capture sits in every replayed step; neither they nor k_pod_combine may use scratch.  No VGPR bound is
asserted; DESIGN.md 4ag records the counts."""
import re

from test_build_metadata import kernels  # noqa: F401 (the module-scoped fixture that unbundles the code objects)


def _instantiations(kernels, name):      # noqa: F811
    return {k: v for k, v in kernels.items() if re.search(r"\d+" + name + "I", k)}


def test_every_capture_and_combine_instantiation_is_built_without_scratch(kernels):      # noqa: F811
    for kname in ("k_pod_capture", "k_pod_combine"):
        got = _instantiations(kernels, kname)
        # T in (float, double) x W in (1, 2)
        assert len(got) == 4, sorted(got)
        for t in "fd":
            for w in (1, 2):
                assert any(re.search(rf"{kname}I{t}Li{w}E", n) for n in got), (kname, t, w)
        for name, k in sorted(got.items()):
            print(name, k)
            assert k["scratch"] == 0, (name, k)


def test_every_gram_instantiation_is_built_without_scratch(kernels):      # noqa: F811
    got = _instantiations(kernels, "k_pod_gram")
    # T in (float, double) x (diagonal tile, pair of tiles)
    assert len(got) == 4, sorted(got)
    for t in "fd":
        for diag in (0, 1):
            assert any(re.search(rf"k_pod_gramI{t}Lb{diag}E", n) for n in got), (t, diag)
    for name, k in sorted(got.items()):
        print(name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] == 4 * 64 * 8, (name, k)      # the four waves' 64 sums
    others = {n: k for n, k in kernels.items() if "k_pod_gram_final" in n or "k_pod_tick" in n}
    assert len(others) == 2, sorted(others)
    for name, k in others.items():
        print(name, k)
        assert k["scratch"] == 0, (name, k)
