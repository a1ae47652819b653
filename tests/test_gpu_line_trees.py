"""Line queries with inc_trees = 1 on a tile batch (terra_tiles_line_intersect_trees[_dev]) through HIP on the MI355X -- k_line_tree_boxes and
k_line_intersect_trees, and the driver's simple form under "kernels.simple" -- against tests/line_trees_model.py, every byte of every hit record: the emulator's
cases, every row of tests/golden/line_trees_vectors.npz through the public entry point, and one device-resident chain on a 3 x 3 batch at S = 128 from the zvals
through the placement and a removing stroke of the tree brush to the lines."""
import contextlib
import os

import numpy as np
import pytest

import line_trees_cases as ltc

pytestmark = pytest.mark.gpu
CASES = ltc.cases()
BY_NAME = {c.name: c for c in CASES}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_trees_vectors.npz")


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, gpu, case):
    ltc.run_case(pkg, gpu, case, dev=True)


@pytest.mark.parametrize("name", ["parts_offset", "mesh_and_trees", "line_tile_out_of_range", "counts", "instanced", "trunk_override", "three_hundred_lines"])
def test_cases_host_form(pkg, gpu, name):
    ltc.run_case(pkg, gpu, BY_NAME[name])


@pytest.mark.parametrize("name", ["parts", "mesh_and_trees_offset", "same_tree_twice", "end_on_surface", "distant_and_line_tile", "line_tile_out_of_range", "counts", "dropped",
                                  "three_hundred_lines_offset", "s128_offsets"])
def test_cases_simple_form(pkg, gpu, name):
    with simple_form(gpu):
        ltc.run_case(pkg, gpu, BY_NAME[name], dev=True)


def test_fixture_rows_on_the_device(pkg, gpu):
    """every row of the fixture: the device's line_trunc_cone (its atan2f, cosf, double products and divisions) against the reference's compiled code"""
    fx = np.load(FIXTURE)
    assert ltc.run_fixture_rows(pkg, gpu, fx) >= len(fx["rows"]) // 2


def test_resident_chain(pkg, gpu):
    tally = ltc.run_resident_chain(pkg, gpu)
    assert tally["tree_hits"] >= 20


def test_resident_chain_simple_form(pkg, gpu):
    with simple_form(gpu):
        ltc.run_resident_chain(pkg, gpu)
