"""The grass draw lists (terra_tiles_grass_view[_dev]) through HIP on the MI355X -- k_grass_view, and the driver's simple form under "kernels.simple" -- against
tests/grass_view_model.py, byte for byte on insts, aux, group_counts, counts and pass, in order: the emulator's cases, and one device-resident chain on a 3 x 3
batch at S = 128 from the zvals to the draw lists before and after a grass stroke."""
import contextlib

import pytest

import grass_view_cases as gc
import view_model
import test_grass_view_emul as tge

pytestmark = pytest.mark.gpu
CASES = gc.cases()
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
    gc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["inside_along_ground", "mixed_nrnd3", "capacity_small"])
def test_cases_host_form(pkg, gpu, orc, name):
    gc.run_case(pkg, gpu, orc, BY_NAME[name])


def test_without_aux_and_pass(pkg, gpu, orc):
    gc.run_case(pkg, gpu, orc, BY_NAME["mixed_nrnd3"], dev=True, aux=False, want_pass=False)
    gc.run_case(pkg, gpu, orc, BY_NAME["ridge"], aux=False, want_pass=False)


@pytest.mark.parametrize("name", ["inside_along_ground", "ridge", "mixed_nrnd3", "full_s128"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        gc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_make_view(pkg, gpu):
    for kw in tge.VIEWS:
        got = gpu.make_view(kw["pos"], kw["dir"], kw["up"], kw["angle"], kw["aspect"], kw["near"], kw["far"])
        assert bytes(got) == view_model.make_view(**kw).words(), kw


def test_resident_chain(pkg, gpu, orc):
    gc.run_resident_chain(pkg, gpu, orc)
