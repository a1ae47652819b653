"""Sphere collisions and tree box tests against the containers of a tile batch (terra_tiles_sphere_collide[_dev], terra_tiles_cube_int_trees[_dev]) through HIP on the
MI355X -- k_sphere_collide and k_cube_int_trees, and the driver's simple form under "kernels.simple" -- against tests/collide_model.py, every output byte: the
emulator's cases, and one device-resident chain on a 3 x 3 batch at S = 128 from the zvals through the three placements to the queries."""
import contextlib

import pytest

import collide_cases as cc

pytestmark = pytest.mark.gpu
CASES = cc.cases()
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
    cc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["chain_across_containers", "row_of_stumps", "stages", "out_of_range_instanced", "three_hundred_queries", "cubes"])
def test_cases_host_form(pkg, gpu, orc, name):
    cc.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["chain_in_one_chunk", "scenery_kind_order", "lane_63_then_64", "round_trip_alone", "out_of_range", "tile_borders_offset", "three_hundred_queries",
                                  "cubes", "s128_offsets"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        cc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_resident_chain(pkg, gpu, orc):
    cc.run_resident_chain(pkg, gpu, orc)
