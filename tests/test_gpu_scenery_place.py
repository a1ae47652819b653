"""Scenery placement (terra_tiles_place_scenery[_dev]) through HIP on the MI355X -- k_scenery_place, and the driver's simple form under "kernels.simple" --
against tests/scenery_place_model.py, byte for byte, order, counts and kind counts included: the emulator's cases, and a device-resident 8 x 8 batch at S = 128
that goes through terra_tiles_create_zvals_dev first."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import orclib
import scenery_place_cases as spc
import scenery_place_model as spm
import tree_place_model as tpm

pytestmark = pytest.mark.gpu
CASES = spc.cases()
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
    spc.run_case(pkg, gpu, orc, case, dev=True)


@pytest.mark.parametrize("name", ["defaults_s128", "skipped_tile", "capacity_small"])
def test_cases_host_form(pkg, gpu, orc, name):
    spc.run_case(pkg, gpu, orc, BY_NAME[name])


def test_without_kind_counts(pkg, gpu, orc):
    spc.run_case(pkg, gpu, orc, BY_NAME["tree_scale_8_s64"], dev=True, kind_counts=False)


@pytest.mark.parametrize("name", ["dwarp_s64", "shore_mode3", "voxel_rocks_1", "tree_scale_8_s20"])
def test_cases_simple_form(pkg, gpu, orc, name):
    with simple_form(gpu):
        spc.run_case(pkg, gpu, orc, BY_NAME[name], dev=True)


def test_resident_batch(pkg, gpu, orc):
    """zvals and stats -> scenery placement on an 8 x 8 batch at S = 128 on one context, nothing read back in between, some tiles skipped"""
    S, side, cap = 128, 8, 192
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gpu.init_scene(cfg)
    gpu.set_landscape(pkg.make_landscape())
    tp = dict(tree_mode=3, tree_type_rand_zone=0.02)
    gpu.set_tree_params(pkg.make_tree_params(**tp))
    gpu.set_scenery_params(pkg.make_scenery_params(1))
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(1, side + 1)]  # from the island's top out over its shore
    n, Z = len(tiles), S + 2
    skip = ((np.arange(n) % 13) == 5).astype(np.uint8)
    bufs = dict(z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), sk=gpu.alloc(n).upload(skip), ob=gpu.alloc(n * cap * spc.REC), cn=gpu.alloc(n * 4),
                kc=gpu.alloc(n * spc.NK * 4))
    try:
        bufs["ob"].upload(np.zeros(n * cap * spc.REC, np.uint8))
        gpu.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)
        gpu.tiles_place_scenery_dev(tiles, cap, bufs["ob"].ptr, bufs["cn"].ptr, 0, 0, bufs["sk"].ptr, bufs["kc"].ptr)
        objs = bufs["ob"].download(np.uint8, (n * cap * spc.REC,)).view(pkg.SCENERY_PLACE_DTYPE).reshape(n, cap)
        counts = bufs["cn"].download(np.uint32, (n,))
        kinds = bufs["kc"].download(np.uint32, (n, spc.NK))
    finally:
        for b in bufs.values():
            b.free()
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**tp))
    tally = spm.new_tally()
    want = spm.place(sc, tiles, 0, 0, skip, 1, 0.0, tally)
    spc.compare("resident", objs, counts, kinds, want, cap)
    assert all(tally[k] >= 1 for k in spm.KINDS) and not counts[skip == 1].any() and counts[skip == 0].all()
    assert max(len(w) for w in want) <= cap
