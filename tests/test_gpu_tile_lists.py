"""The device path of the launch lists (fs_core.hip tile_list: build, upload, cache) tied to the restatement the CPU tests use
(tests/tiles_ref.py, tests/test_tile_lists_cpu.py) through what the ABI already reports: fs_cip_step_tiles' counts and fs_tile_list_stats."""
import numpy as np
import pytest

import tiles_ref as R

pytestmark = pytest.mark.gpu

RES = 256


@pytest.mark.parametrize("bc", [2, 5])
def test_cip_step_tile_counts_match_the_restatement(bc, hip_lib):
    import fs
    from fs.boundary_condition import BoundaryCondition, create_scene_arrays
    const, mask, _ = create_scene_arrays(bc, RES)
    fs.runtime.init(gpu=0, dtype="f32")
    dev = BoundaryCondition(const, mask).device
    try:
        assert dev.cip_step_fused
        plain, boundary, band, tile_rows, tile_cells = dev.cip_step_tiles()
        built, misses = dev.tile_list_stats()
        assert tile_cells == R.WIDTH[R.PAIR] and tile_rows in (2, 4) and band == 0

        m = np.ascontiguousarray(mask.astype(np.uint8))
        X, Y = m.shape
        act = R.activity(m, np.zeros_like(m), R.PAIR)      # (without the recipe bytes of the library's op lists: wall cells count as deep wall)
        nbx, nby, group = R.launch_geometry(X, R.PAIR, tile_rows, 1, False, 0, Y)
        counts = {cls: R.build(act, X, R.PAIR, tile_rows, 1, False, group, cls, 2, 0, 0, Y, nbx, nby)[2] for cls in (R.PLAIN, R.BOUNDARY)}
        print(f"bc{bc}: tiles of {tile_rows} rows - plain {plain} (restatement {counts[R.PLAIN]}), boundary {boundary} "
              f"(between {counts[R.BOUNDARY]} and {nbx * nby - counts[R.PLAIN]}); lists built {built}, misses {misses}")
        # the plain tiles depend on the mask alone; a boundary tile is any other tile with work: at least those with a cell that is not wall,
        # at most every other tile (which wall cells a boundary kernel writes is in the op lists)
        assert plain == counts[R.PLAIN] > 0
        assert counts[R.BOUNDARY] <= boundary <= nbx * nby - plain
        # a second identical call finds its lists
        assert dev.cip_step_tiles() == (plain, boundary, band, tile_rows, tile_cells)
        assert dev.tile_list_stats() == (built, misses) and misses == 0 and built >= 2
    finally:
        dev.close()
