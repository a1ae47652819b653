"""The flowers (terra_tiles_place_flowers[_dev], terra_tiles_edit_flowers[_dev]) through HIP on the MI355X -- k_flowers_place and k_flowers_remove, and the driver's
simple form under "kernels.simple" -- against tests/flower_model.py, byte for byte on records, aux words and counts, in order: the emulator's cases, and one
device-resident chain on a 4 x 4 batch at S = 128 from the zvals to the flowers after two grass strokes.

The colour of a flower whose index int is negative is compared like every other byte: the model follows the source's `int % unsigned` (see test_flowers_emul.py),
not the rule the issue proposed for what it took for an out-of-bounds read."""
import contextlib

import pytest

import flower_cases as fc

pytestmark = pytest.mark.gpu
CASES = fc.cases()
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
    fc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["pattern_s20", "skipped_tile", "capacity_small"])
def test_cases_host_form(pkg, gpu, orc, name):
    fc.run_case(pkg, gpu, orc, BY_NAME[name])


def test_without_aux(pkg, gpu, orc):
    fc.run_case(pkg, gpu, orc, BY_NAME["odd_density_s20"], dev=True, aux=False)
    fc.run_edit_case(pkg, gpu, orc, fc.edit_case(orc, "two_strokes"), dev=True, aux=False)


@pytest.mark.parametrize("name", ["pattern_s20", "fixed_color_s64", "negative_tiles_s20", "shore_s128"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        fc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


@pytest.mark.parametrize("name", fc.EDIT_NAMES)
def test_edit_cases(pkg, gpu, orc, name):
    fc.run_edit_case(pkg, gpu, orc, fc.edit_case(orc, name), dev=True)


@pytest.mark.parametrize("name", ["add_inside", "remove_round"])
def test_edit_cases_host_form(pkg, gpu, orc, name):
    fc.run_edit_case(pkg, gpu, orc, fc.edit_case(orc, name))


@pytest.mark.parametrize("name", ["two_strokes", "remove_square", "remove_dense"])
def test_edit_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        fc.run_edit_case(pkg, gpu, orc, fc.edit_case(orc, name), dev=True)


def test_resident_chain(pkg, gpu, orc):
    fc.run_resident_chain(pkg, gpu, orc)
