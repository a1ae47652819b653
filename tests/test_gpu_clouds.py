"""The clouds of a tile batch (terra_tiles_update_clouds[_dev], terra_tiles_cloud_view[_dev]) through HIP on the MI355X -- k_cloud_mark, k_cloud_tiles, k_cloud_tail,
k_cloud_view and k_cloud_rank, and the driver's simple form under "kernels.simple" -- against tests/cloud_model.py, byte for byte after every call: the emulator's
cases, and one device-resident chain on a 5 x 5 batch at S = 128 from the zvals through twenty updates to the draw list."""
import contextlib

import pytest

import cloud_cases as cc

pytestmark = pytest.mark.gpu
UCASES, VCASES = cc.update_cases(), cc.view_cases()
U_BY_NAME, V_BY_NAME = {c.name: c for c in UCASES}, {c.name: c for c in VCASES}


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", UCASES, ids=[c.name for c in UCASES])
def test_update_cases(pkg, gpu, orc, case):
    cc.run_update_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("case", VCASES, ids=[c.name for c in VCASES])
def test_view_cases(pkg, gpu, orc, case):
    cc.run_view_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["gen_default", "diagonal", "overflow", "density_zero"])
def test_update_cases_host_form(pkg, gpu, orc, name):
    cc.run_update_case(pkg, gpu, orc, U_BY_NAME[name])


@pytest.mark.parametrize("name", ["offset_low", "ties"])
def test_view_cases_host_form(pkg, gpu, orc, name):
    cc.run_view_case(pkg, gpu, orc, V_BY_NAME[name])


@pytest.mark.parametrize("name", ["row_crossed_in_one_frame", "diagonal_against_order", "drop_at_ungenerated", "fed_before_turn", "holes_shuffled_s128", "overflow", "density_zero"])
def test_update_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        cc.run_update_case(pkg, gpu, orc, U_BY_NAME[name], dev=True)


@pytest.mark.parametrize("name", ["offset_low", "beyond_max_dist", "ties"])
def test_view_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        cc.run_view_case(pkg, gpu, orc, V_BY_NAME[name], dev=True)


def test_resident_chain(pkg, gpu, orc):
    cc.run_resident_chain(pkg, gpu, orc)
