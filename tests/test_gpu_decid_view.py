"""The deciduous tree draw lists (terra_tiles_decid_view[_dev]) through HIP on the MI355X -- k_decid_view, and the driver's simple form under "kernels.simple" --
against tests/decid_view_model.py, byte for byte on the tile records, the words, scales, opacities and counts of both sweeps, the four lists and not_visible: the
emulator's cases, a leaves-only call followed by a branches-only call, and one device-resident chain on a 3 x 3 batch at S = 128 from the zvals through the deciduous
placement, the tree AO shadows and the terrain draw list, whose not_drawn bytes are the skip bytes here."""
import contextlib

import pytest

import decid_view_cases as dc

pytestmark = pytest.mark.gpu
CASES = dc.cases()
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
    dc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["stages_forms", "offsets", "big_tile", "tiles_skip_empty"])
def test_cases_host_form(pkg, gpu, orc, name):
    dc.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["stages_forms", "counts", "sorted_ties", "big_tile", "big_table", "shadow_pass", "frustum_planes"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        dc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_leaves_then_branches(pkg, gpu, orc):
    dc.run_split(pkg, gpu, orc, BY_NAME["all_ids"])


def test_resident_chain(pkg, gpu, orc):
    dc.run_resident_chain(pkg, gpu, orc)
