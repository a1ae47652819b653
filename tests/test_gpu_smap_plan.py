"""The shadow-map plan (terra_tiles_smap_plan[_dev]) and the caster lists (terra_tiles_smap_casters[_dev]) through HIP on the MI355X -- k_smap_plan,
k_smap_plan_lists, k_smap_plan_rank, k_smap_geom and k_smap_casters, and the driver's simple form under "kernels.simple" -- against tests/smap_plan_model.py, byte
for byte on every output: the emulator's cases in the device form, a handful in the host form and in the simple form, and one device-resident chain on a 5 x 5
batch at S = 128 from the zvals through the plan and the casters to a shadow-pass tree view."""
import contextlib

import pytest

import smap_plan_cases as sc_

pytestmark = pytest.mark.gpu
PCASES, CCASES = sc_.plan_cases(), sc_.caster_cases()
P_BY_NAME, C_BY_NAME = {c.name: c for c in PCASES}, {c.name: c for c in CCASES}


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", PCASES, ids=[c.name for c in PCASES])
def test_plan_cases(pkg, gpu, orc, case):
    sc_.run_plan_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("case", CCASES, ids=[c.name for c in CCASES])
def test_caster_cases(pkg, gpu, orc, case):
    sc_.run_cast_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["grid13_bands", "terrain_flags_ored", "recomp_order_ties", "n65"])
def test_plan_cases_host_form(pkg, gpu, orc, name):
    sc_.run_plan_case(pkg, gpu, orc, P_BY_NAME[name])


@pytest.mark.parametrize("name", ["r5_grid3", "receiver_absent_or_out_of_range", "all_arrays", "n65"])
def test_caster_cases_host_form(pkg, gpu, orc, name):
    sc_.run_cast_case(pkg, gpu, orc, C_BY_NAME[name])


@pytest.mark.parametrize("name", ["grid13_bands", "shadow_map_sz_8192", "recomp_order_absent", "s128", "large_batch"])
def test_plan_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        sc_.run_plan_case(pkg, gpu, orc, P_BY_NAME[name], dev=True)


@pytest.mark.parametrize("name", ["inc_adj_smap", "decid_only_some_counts", "all_water_tile", "n64", "large_batch_r7"])
def test_caster_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        sc_.run_cast_case(pkg, gpu, orc, C_BY_NAME[name], dev=True)


def test_make_light_view(pkg, gpu):
    """host only: the same bodies as in the emulator's library, compiled by hipcc for the host"""
    sc_.check_light_views(pkg, gpu)


def test_resident_chain(pkg, gpu, orc):
    sc_.run_resident_chain(pkg, gpu, orc)
