"""Tree placement (terra_tiles_place_trees[_dev], terra_tiles_place_trees_brush[_dev]) through HIP on the MI355X -- k_tree_place, and the driver's simple form
under "kernels.simple" -- against tests/tree_place_model.py, byte for byte, order and counts included: the emulator's cases, and a device-resident 8 x 8 batch
at S = 128 whose z ranges come straight from terra_tiles_create_zvals_dev."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import orclib
import tree_place_cases as tpc
import tree_place_model as tpm

pytestmark = pytest.mark.gpu
CASES = tpc.cases()


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, gpu, orc, case):
    tpc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["defaults_s128", "skip_and_stats", "brush_round"])
def test_cases_host_form(pkg, gpu, orc, name):
    tpc.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0])


@pytest.mark.parametrize("name", ["defaults_s64", "palms_mode3", "capacity_small", "brush_four_tiles"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        tpc.run_case(pkg, gpu, orc, [c for c in CASES if c.name == name][0], dev=True)


def test_refused_on_device(pkg, gpu, orc):
    gpu.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=16))
    gpu.set_tree_params(pkg.make_tree_params(tree_mode=2))
    with pytest.raises(pkg.TerraError) as e:
        gpu.tiles_place_trees(tpc.TILES, 8)
    assert e.value.code == tpc.ERR_ARG and "XY_MULT_SIZE" in str(e.value)


def test_resident_batch(pkg, gpu, orc):
    """zvals and stats -> tree placement on an 8 x 8 batch at S = 128, nothing read back in between; the model's z ranges are the downloaded stats'"""
    S, side, cap = 128, 8, 192
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gpu.init_scene(cfg)
    gpu.set_landscape(pkg.make_landscape())
    tp = dict(tree_mode=3, sm_tree_density=0.5)
    gpu.set_tree_params(pkg.make_tree_params(**tp))
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(1, side + 1)]  # from the island's top out over its shore
    n, Z = len(tiles), S + 2
    skip = ((np.arange(n) % 13) == 5).astype(np.uint8)
    bufs = dict(z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), sk=gpu.alloc(n).upload(skip), tr=gpu.alloc(n * cap * 40), cn=gpu.alloc(n * 4))
    try:
        bufs["tr"].upload(np.zeros(n * cap * 40, np.uint8))
        gpu.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)
        gpu.tiles_place_trees_dev(tiles, cap, bufs["tr"].ptr, bufs["cn"].ptr, 0, 0, bufs["sk"].ptr, bufs["st"].ptr)
        trees = bufs["tr"].download(np.uint8, (n * cap * 40,)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap)
        counts = bufs["cn"].download(np.uint32, (n,))
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
    finally:
        for b in bufs.values():
            b.free()
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**tp))
    zranges = [(stats[i].mzmin, stats[i].mzmax) for i in range(n)]
    want = tpm.place(sc, tiles, 0, 0, skip, zranges)
    tpc.compare("resident", trees, counts, want, cap)
    culled = sum(not sc.can_have_pine_palm_trees_in_zrange(*zr) for zr in zranges)
    assert 0 < culled < n and sum(len(w) for w in want) > 20 * n // 4 and not counts[skip == 1].any()
