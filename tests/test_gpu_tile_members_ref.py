"""The device entry points terra_tiles_tree_map_dev, terra_tiles_shadow_texture_dev, terra_tiles_tree_weights_dev, terra_tiles_line_intersect_dev and
terra_tiles_edit_grass_dev through HIP on the MI355X -- the kernels, and the simple forms under "kernels.simple" -- against the compiled reference with no model
in between: the recording of tests/golden/tile_member_vectors.npz, and, where oracle/_ref travelled, the live reference on the full case sets of
tests/tile_member_cases.py.  One to four tiles at S = 128 a call, the line rows one batch of lines per tile, the grass strokes one a call; every byte, no
tolerance.  (The exhaustive kernel-against-model tests are tests/test_gpu_tree_map.py, test_gpu_line_intersect.py and test_gpu_grass_brush.py.)"""
import contextlib

import pytest

import tile_member_cases as tmc

pytestmark = pytest.mark.gpu
SETS = {}


@pytest.fixture(scope="module")
def fx_sets():
    return tmc.fixture_sets(tmc.load())


@pytest.fixture()
def ref_sets(ref):
    reason = tmc.stale_reference(ref)  # fails where the reference tree is present
    if reason:
        pytest.skip(reason)
    if "ref" not in SETS:
        SETS["ref"] = tmc.reference_sets(ref)
    return SETS["ref"]


@contextlib.contextmanager
def form(gpu, simple):
    gpu.set_option("kernels.simple", "1" if simple else "0")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("simple", [False, True], ids=["kernels", "simple form"])
@pytest.mark.parametrize("what", tmc.PASSES)
def test_device_entry_points_vs_fixture(pkg, gpu, fx_sets, what, simple):
    with form(gpu, simple):
        tmc.check_lib_against(pkg, gpu, True, only=(what,), **fx_sets)


def test_host_entry_points_vs_fixture(pkg, gpu, fx_sets):
    tmc.check_lib_against(pkg, gpu, False, **fx_sets)


@pytest.mark.parametrize("simple", [False, True], ids=["kernels", "simple form"])
@pytest.mark.parametrize("what", tmc.PASSES)
def test_device_entry_points_vs_live_reference(pkg, gpu, ref_sets, what, simple):
    with form(gpu, simple):
        tmc.check_lib_against(pkg, gpu, True, only=(what,), **ref_sets)
