"""The pine and palm tree draw lists (terra_tiles_tree_view[_dev]) through HIP on the MI355X -- k_tree_view, and the driver's simple form under "kernels.simple" --
against tests/tree_view_model.py, byte for byte on the tile records, both instance lists, the leaf list, the counts and the trunk bytes, all_bcube by value: the
emulator's cases, and one device-resident chain on a 3 x 3 batch at S = 128 from the zvals through the placement, the tree AO pass and the terrain draw list, whose
not_drawn bytes are the skip bytes here."""
import contextlib

import pytest

import tree_view_cases as tc

pytestmark = pytest.mark.gpu
CASES = tc.cases()
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
    tc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["many_records", "instanced_many_ids", "camera_tile", "dropped_skip_empty"])
def test_cases_host_form(pkg, gpu, orc, name):
    tc.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["many_records", "instanced_many_ids", "instanced_big_table", "lod_ring", "camera_tile", "camera_tile_large_capacity", "frustum_planes"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        tc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_resident_chain(pkg, gpu, orc):
    tc.run_resident_chain(pkg, gpu, orc)
