"""The tree brush on the record arrays of a tile batch (terra_tiles_edit_trees[_dev]) through HIP on the MI355X -- k_tree_edit, k_tree_edit_append and
k_tree_edit_finish, and the simple forms under "kernels.simple" -- against tests/tree_edit_model.py: records and counts byte for byte, decid_radius, trmax, status
and changed exactly, the update box by value; the emulator's cases, and the chain zvals -> both placements -> tree AO shadows -> a removing stroke -> an adding
stroke -> tree AO shadows -> shadow texture on a device-resident 4 x 4 batch at S = 128 with nothing read back in between."""
import contextlib

import pytest

import tree_edit_cases as tec
import tree_edit_chain as chain

pytestmark = pytest.mark.gpu
CASES = tec.cases()


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases(pkg, gpu, orc, case):
    tec.run_case(pkg, gpu, orc, case)


@pytest.mark.parametrize("name", tec.HOST_FORM)
def test_cases_host_form(pkg, gpu, orc, name):
    tec.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0], host=True)


@pytest.mark.parametrize("name", tec.SIMPLE_FORM)
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        tec.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0])


def test_refused(pkg, gpu, orc):
    tec.run_refused(pkg, gpu, orc, dev_form=False)


def test_refused_device_form(pkg, gpu, orc):
    tec.run_refused_dev(pkg, gpu, orc)


def test_resident_chain(pkg, gpu, orc):
    tallies = chain.run(pkg, gpu, orc, 128, 4)
    assert tallies[0]["removed_pine"] > 0 and tallies[1]["appended_decid"] > 0


def test_resident_chain_simple_form(pkg, gpu, orc):
    with simple_form(gpu):
        chain.run(pkg, gpu, orc, 128, 4)
