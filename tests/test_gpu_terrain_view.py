"""The terrain draw list (terra_tiles_terrain_view[_dev]) through HIP on the MI355X -- the k_terrain_view_* kernels, and the driver's simple form under
"kernels.simple" -- against tests/terrain_view_model.py, byte for byte on status, dist, lod, crack, both lists in order, counts and occl_state: the emulator's cases,
and one device-resident chain on a 5 x 5 batch at S = 128 from the zvals through the terrain view to the grass draw lists that its skip bytes gate."""
import contextlib

import numpy as np
import pytest

import terrain_view_cases as tc
import view_model
import test_grass_view_emul as tge

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


@pytest.mark.parametrize("name", ["ridge_low_camera", "state_in", "all_arrays"])
def test_cases_host_form(pkg, gpu, orc, name):
    tc.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["ridge_low_camera", "many_drawn_equal", "many_drawn_distinct", "lod_classes_s128", "cracks", "state_in", "all_arrays"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        tc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_behind_sphere_mult(pkg, gpu):
    for kw in tge.VIEWS:
        got = np.float32(gpu.view_behind_sphere_mult(kw["angle"], kw["aspect"]))
        assert got.tobytes() == view_model.behind_sphere_mult(kw["angle"], kw["aspect"]).tobytes(), kw


def test_resident_chain(pkg, gpu, orc):
    tc.run_resident_chain(pkg, gpu, orc)
