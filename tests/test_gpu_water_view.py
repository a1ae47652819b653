"""The reflection pass's terrain draw list (terra_tiles_reflection_view[_dev]) and the water quads and water caps (terra_tiles_water_view[_dev]) through HIP on the
MI355X -- the k_terrain_view_* kernels with pass 1's LOD, k_reflect_walk, k_reflect_finish and k_water_view, and the driver's simple form under "kernels.simple" --
against tests/water_view_model.py, byte for byte on every output: the emulator's cases, and one device-resident chain on a 5 x 5 batch at S = 128 from the zvals
through the reflection pass and the main pass to the water quads and caps."""
import contextlib

import pytest

import water_view_cases as wc

pytestmark = pytest.mark.gpu
RCASES, WCASES = wc.reflection_cases(), wc.water_cases()
R_BY_NAME, W_BY_NAME = {c.name: c for c in RCASES}, {c.name: c for c in WCASES}


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", RCASES, ids=[c.name for c in RCASES])
def test_reflection_cases(pkg, gpu, orc, case):
    wc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("case", WCASES, ids=[c.name for c in WCASES])
def test_water_cases(pkg, gpu, orc, case):
    wc.run_water_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["order_a_before_b", "state_in_unoccluded", "all_arrays"])
def test_reflection_cases_host_form(pkg, gpu, orc, name):
    wc.run_case(pkg, gpu, orc, R_BY_NAME[name])


@pytest.mark.parametrize("name", ["caps_masks", "water_all_arrays", "water_no_status"])
def test_water_cases_host_form(pkg, gpu, orc, name):
    wc.run_water_case(pkg, gpu, orc, W_BY_NAME[name])


@pytest.mark.parametrize("name", ["reflect_values", "order_shuffled", "order_chain", "lod_pass1_s128", "state_in_unoccluded", "all_arrays"])
def test_reflection_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        wc.run_case(pkg, gpu, orc, R_BY_NAME[name], dev=True)


@pytest.mark.parametrize("name", ["caps_masks", "caps_distance", "water_no_status"])
def test_water_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        wc.run_water_case(pkg, gpu, orc, W_BY_NAME[name], dev=True)


def test_resident_chain(pkg, gpu, orc):
    wc.run_resident_chain(pkg, gpu, orc)
