"""The tree AO shadows of a tile batch from the placement records (terra_tiles_tree_ao_shadows[_dev]) through HIP on the MI355X -- k_tree_ao_sources,
k_tree_ao_gather and k_tree_map, and the simple forms under "kernels.simple" -- against tests/tree_ao_model.py, byte for byte: every map, updated, trmax and
list_counts of the emulator's cases, and the chain zvals -> both placements -> tree AO shadows -> shadow texture and tree weights on a device-resident 4 x 4 batch at
S = 128 with nothing read back in between."""
import contextlib

import pytest

import tree_ao_cases as tac
import tree_ao_chain as chain

pytestmark = pytest.mark.gpu
CASES = tac.cases()


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases(pkg, gpu, orc, case):
    tac.run_case(pkg, gpu, orc, case)


@pytest.mark.parametrize("name", tac.HOST_FORM)
def test_cases_host_form(pkg, gpu, orc, name):
    tac.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0], host=True)


@pytest.mark.parametrize("name", tac.SIMPLE_FORM)
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        tac.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0])


def test_refused(pkg, gpu, orc):
    tac.run_refused(pkg, gpu, orc, dev_form=False)


def test_resident_chain(pkg, gpu, orc):
    tally = chain.run(pkg, gpu, orc, 128, 4)
    assert tally["pulled"] > 0 and tally["pushed"] > 0


def test_resident_chain_simple_form(pkg, gpu, orc):
    with simple_form(gpu):
        chain.run(pkg, gpu, orc, 128, 4)
