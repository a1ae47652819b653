"""Deciduous tree placement (terra_tiles_place_decid_trees[_dev], terra_tiles_place_decid_trees_brush[_dev]) through HIP on the MI355X -- k_decid_place, and the
driver's simple form under "kernels.simple" -- against tests/decid_place_model.py, byte for byte, order and counts included: the emulator's cases, and a
device-resident 8 x 8 batch at S = 128 whose zvals and stats come straight from terra_tiles_create_zvals_dev."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import decid_place_cases as dpc
import decid_place_model as dpm
import orclib
import tree_place_model as tpm

pytestmark = pytest.mark.gpu
CASES = dpc.cases()
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
    dpc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["defaults_s128", "skip_and_stats", "brush_round"])
def test_cases_host_form(pkg, gpu, orc, name):
    dpc.run_case(pkg, gpu, orc, BY_NAME[name])


@pytest.mark.parametrize("name", ["dwarp_s64", "mode3_shore", "slope_thresh", "brush_square_four_tiles"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        dpc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_resident_batch(pkg, gpu, orc):
    """zvals and stats -> deciduous placement on an 8 x 8 batch at S = 128, nothing read back in between; the model is fed the downloaded zvals and stats"""
    S, side, cap = 128, 8, 640
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gpu.init_scene(cfg)
    gpu.set_landscape(pkg.make_landscape())
    tp, dp = dict(tree_mode=3, tree_type_rand_zone=0.02), dict(num_trees=400, num_shared_trees=100, tree_slope_thresh=2.0)
    gpu.set_tree_params(pkg.make_tree_params(**tp))
    gpu.set_decid_params(pkg.make_decid_params(**dp))
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(1, side + 1)]  # from the island's top out over its shore
    n, Z = len(tiles), S + 2
    skip = ((np.arange(n) % 13) == 5).astype(np.uint8)
    bufs = dict(z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), sk=gpu.alloc(n).upload(skip), tr=gpu.alloc(n * cap * dpc.REC), cn=gpu.alloc(n * 4))
    try:
        bufs["tr"].upload(np.zeros(n * cap * dpc.REC, np.uint8))
        gpu.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)
        gpu.tiles_place_decid_trees_dev(tiles, cap, bufs["tr"].ptr, bufs["cn"].ptr, 0, 0, bufs["sk"].ptr, bufs["st"].ptr, bufs["z"].ptr)
        trees = bufs["tr"].download(np.uint8, (n * cap * dpc.REC,)).view(pkg.DECID_PLACE_DTYPE).reshape(n, cap)
        counts = bufs["cn"].download(np.uint32, (n,))
        zvals = bufs["z"].download(np.float32, (n, Z, Z))
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
    finally:
        for b in bufs.values():
            b.free()
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**tp))
    tally = dpm.new_tally()
    want = dpm.place(sc, dpm.DecidParams(**dp), tiles, 0, 0, skip, stats, zvals, None, tally)
    dpc.compare("resident", trees, counts, want, cap)
    culled = sum(not dpm.can_have_decid_trees_in_zrange(sc, s.mzmin, s.mzmax) for s in stats)
    steep = sum(bool(dpm.mesh_dz(s) > 1.0) for s in stats)
    assert 0 < culled < n and steep >= 1 and tally["slope_kept"] >= 10 and sum(len(w) for w in want) > 20 * n // 4 and not counts[skip == 1].any()
    assert max(len(w) for w in want) <= cap
