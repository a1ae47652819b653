"""Tiles at tile sizes S = mesh_x other than 128 on the MI355X (k_tile_post_sized and the size-general passes of terra_simple_paths.hpp), bit for bit
against tests/tile_size_model.py (pinned to the oracle at S = 128 by tests/test_tile_size_model.py)."""
import os

import numpy as np
import pytest

import orclib
import tile_size_model as tsm
from orclib import assert_bit_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = [(x, y) for y in range(-2, 2) for x in range(-2, 2)]  # 4 x 4 tiles at mixed-sign coordinates
LIGHTS = ((1.0, 0.6, 0.3), (-0.4, -1.0, 0.15))


def scenes(pkg, t, orc, S, mode=0, **kw):
    t.init_scene(pkg.make_config(mesh_gen_mode=mode, mesh_xy=S, **kw))
    orc.init(orclib.make_config(mesh_gen_mode=mode, mesh_xy=S, **kw))


def check_tiles(orc, S, tiles, z, st, nm, mnz, iters, what, **kw):
    zs = []
    for i, (tx, ty) in enumerate(tiles):
        zm = tsm.tile_zvals(orc, S, tx, ty, iters, **kw)
        zs.append(zm)
        assert_bit_equal(zm, z[i], f"{what} zvals S={S} tile {tx},{ty}")
        assert bytes(st[i]) == tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, zm)), f"{what} stats S={S} tile {tx},{ty}"
        nmm, mm = tsm.tile_normals(orc, S, zm)
        assert (nm[i] == nmm).all(), f"{what} normals S={S} tile {tx},{ty}"
        assert np.float32(mnz[i]).view(np.uint32) == np.float32(mm).view(np.uint32), f"{what} min_normal_z S={S} tile {tx},{ty}"
    return zs


@pytest.mark.parametrize("S", [64, 192, 256])
@pytest.mark.parametrize("iters", [0, 1000])
def test_block_of_tiles(pkg, gpu, orc, S, iters):
    scenes(pkg, gpu, orc, S)
    assert gpu.tile_size == S
    z, st, nm, mnz = gpu.tiles_create_zvals(BLOCK, iters)
    check_tiles(orc, S, BLOCK, z, st, nm, mnz, iters, "block")
    ao = gpu.tiles_ao_lighting(BLOCK, z)
    for i, (tx, ty) in enumerate(BLOCK):
        assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i])).all(), f"ao S={S} tile {tx},{ty}"
    for lpos in LIGHTS:
        sm = gpu.tiles_mesh_shadows(BLOCK, z, lpos)
        assert (sm == tsm.tiles_shadows(orc, S, BLOCK, z, lpos)).all(), f"shadows S={S} light {lpos}"
        assert (sm != 0).any()


def test_ao_context_clip_256(pkg, gpu, orc):
    S = 256
    scenes(pkg, gpu, orc, S, mode=4)
    gpu.set_tiled_mesh_ao(1); orc.set_tiled_mesh_ao(1)
    try:
        tiles = [(0, 0), (-1, 1), (2, -1)]
        z, st, nm, mnz = gpu.tiles_create_zvals(tiles, 1000)
        check_tiles(orc, S, tiles, z, st, nm, mnz, 1000, "clip", ao_clip=True)
        ao = gpu.tiles_ao_lighting(tiles, z)
        for i, (tx, ty) in enumerate(tiles):
            assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i], ao_clip=True)).all(), f"clip ao tile {tx},{ty}"
    finally:
        gpu.set_tiled_mesh_ao(0); orc.set_tiled_mesh_ao(0)


def test_island_heightmap_tiles_256(pkg, gpu, orc):
    S = 256
    pix = pkg.terra.read_png(os.path.join(HERE, "golden", "heightmap_island_1k.png"), lib=gpu.lib)
    assert pix.shape == (1024, 1024)
    scenes(pkg, gpu, orc, S)
    buf = gpu.alloc(pix.nbytes).upload(np.ascontiguousarray(pix))
    gpu.hmap_set_dev(buf.ptr, 1024, 1024, 1, -0.2, 0.004)
    orc.hmap_set(np.ascontiguousarray(pix), -0.2, 0.004)
    try:
        tiles = [(x, y) for y in range(-2, 2) for x in range(-2, 2)] + [(2, 0)]  # the 16 tiles over the image, one past its edge
        z, st, nm, mnz = gpu.tiles_create_zvals(tiles, 1000)
        for i in (0, 5, 10, 16):  # (the model samples the texture cell by cell through the oracle: a few tiles)
            tx, ty = tiles[i]
            check_tiles(orc, S, [tiles[i]], z[i:i + 1], st[i:i + 1], nm[i:i + 1], mnz[i:i + 1], 0, "hmap", hmap=True)
        ao = gpu.tiles_ao_lighting(tiles, z)
        for i in (5, 16):
            tx, ty = tiles[i]
            assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i], hmap=True)).all(), f"hmap ao tile {tx},{ty}"
    finally:
        gpu.hmap_set_dev(None); orc.hmap_set(None)
        buf.free()


def test_one_tile_1024(pkg, gpu, orc):
    S = 1024
    scenes(pkg, gpu, orc, S)
    tiles = [(-1, 0)]
    z, st, nm, mnz = gpu.tiles_create_zvals(tiles, 1000)
    check_tiles(orc, S, tiles, z, st, nm, mnz, 1000, "S=1024")
    ao = gpu.tiles_ao_lighting(tiles, z)
    assert (ao[0] == tsm.tile_ao(orc, S, -1, 0, z[0])).all()
    for lpos in LIGHTS:
        sm = gpu.tiles_mesh_shadows(tiles, z, lpos)
        assert (sm == tsm.tiles_shadows(orc, S, tiles, z, lpos)).all(), f"shadows S=1024 light {lpos}"


def test_multi_tiles_create_zvals_256(pkg, orc):
    S = 256
    m = pkg.TerraMulti([0, 0])
    try:
        m.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
        orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S))
        tiles = BLOCK[:5]
        z, st, nm, mnz = m.tiles_create_zvals(tiles, 1000)
        check_tiles(orc, S, tiles, z, st, nm, mnz, 1000, "multi")
    finally:
        m.close()


def test_size_128_unchanged(pkg, gpu, orc):
    """at S = 128 the binding sizes its buffers from terra_tile_size and returns what the oracle's 128-cell tiles are"""
    scenes(pkg, gpu, orc, 128)
    assert gpu.tile_size == 128
    tiles = [(0, 0), (3, -2)]
    z, st, nm, mnz = gpu.tiles_create_zvals(tiles, 100)
    assert z.shape == (2, 130, 130) and nm.shape == (2, 129, 129, 4)
    for i, (tx, ty) in enumerate(tiles):
        zo, so = orc.tile_create_zvals(tx, ty, 100)
        assert_bit_equal(zo, z[i], "128 zvals")
        assert bytes(st[i]) == bytes(so)
        no, mo = orc.tile_normals(zo)
        assert (nm[i] == no).all()
    ao = gpu.tiles_ao_lighting(tiles, z)
    assert (ao[1] == orc.tile_ao_lighting(3, -2, z[1])).all()
