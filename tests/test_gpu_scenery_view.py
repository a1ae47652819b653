"""The scenery draw lists (terra_tiles_scenery_view[_dev]) through HIP on the MI355X -- k_scenery_view, and the driver's simple form under "kernels.simple" -- against
tests/scenery_view_model.py, byte for byte on the tile records, the draw words, size_scale, dist, the lists and the group counts: the emulator's cases, and one
device-resident chain on a 3 x 3 batch at S = 128 from the zvals through the scenery placement and the terrain draw list, whose not_drawn bytes are the skip bytes
here."""
import contextlib

import pytest

import scenery_view_cases as sc_

pytestmark = pytest.mark.gpu
CASES = sc_.cases()
BY_NAME = {c.name: c for c in CASES}


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, gpu, orc, case):
    sc_.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["thresholds", "mixed_offsets", "big_tile_short_list", "tiles_skip_empty_over"])
def test_cases_host_form(pkg, gpu, orc, name):
    sc_.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["thresholds", "mixed", "big_tile", "big_tile_short_list", "water_camera_above", "shadow_pass", "frustum_planes"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        sc_.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_resident_chain(pkg, gpu, orc):
    sc_.run_resident_chain(pkg, gpu, orc)
