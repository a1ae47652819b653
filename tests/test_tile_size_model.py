"""tests/tile_size_model.py at S = 128 against the oracle's tile functions (which are pinned to the compiled reference): every piece bit for bit.  The model is
what the tests of other tile sizes (tests/test_tile_sizes_emul.py, tests/test_gpu_tile_sizes.py) compare against."""
import numpy as np
import pytest

import orclib
import tile_size_model as tsm
from orclib import assert_bit_equal

S = 128
TILES = [(0, 0), (-1, 0), (0, -1), (3, -2), (-2, 5)]


@pytest.mark.parametrize("iters", [0, 1000])
def test_zvals_stats_normals_ao_at_128(orc, iters):
    orc.init(orclib.make_config(mesh_gen_mode=0))
    for tx, ty in TILES[:3] if iters else TILES:
        zo, so = orc.tile_create_zvals(tx, ty, iters)
        z = tsm.tile_zvals(orc, S, tx, ty, iters)
        assert_bit_equal(zo, z, f"zvals {tx},{ty} iters {iters}")
        assert tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, z)) == bytes(so), f"stats {tx},{ty}"
        no, mo = orc.tile_normals(zo)
        nm, mnz = tsm.tile_normals(orc, S, z)
        assert (nm == no).all() and np.float32(mnz).view(np.uint32) == np.float32(mo).view(np.uint32), f"normals {tx},{ty}"
        assert (tsm.tile_ao(orc, S, tx, ty, z) == orc.tile_ao_lighting(tx, ty, zo)).all(), f"ao {tx},{ty}"


def test_ao_context_clip_at_128(orc):
    """enable_tiled_mesh_ao with a GL noise mode: zvals clipped from the AO context, the AO rays over that context everywhere"""
    orc.init(orclib.make_config(mesh_gen_mode=4))
    orc.set_tiled_mesh_ao(1)
    try:
        for tx, ty in TILES[:2]:
            zo, so = orc.tile_create_zvals(tx, ty, 0)
            z = tsm.tile_zvals(orc, S, tx, ty, 0, ao_clip=True)
            assert_bit_equal(zo, z, f"clip zvals {tx},{ty}")
            assert tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, z)) == bytes(so)
            assert (tsm.tile_ao(orc, S, tx, ty, z, ao_clip=True) == orc.tile_ao_lighting(tx, ty, zo)).all(), f"clip ao {tx},{ty}"
    finally:
        orc.set_tiled_mesh_ao(0)


@pytest.mark.parametrize("mesh_scale", [1.0, 0.5])
def test_heightmap_tiles_at_128(orc, mesh_scale):
    s0 = orc.init(orclib.make_config(mesh_gen_mode=0))
    n = 160
    g = orc.gen_grid(-n / 2, -n / 2, s0.DX_VAL, s0.DY_VAL, n, n, 1)
    q, mn, dz = orc.quantize16(g)
    pix = np.ascontiguousarray(q.reshape(n, n, 2))
    orc.init(orclib.make_config(mesh_gen_mode=0, mesh_scale=mesh_scale))
    orc.hmap_set(pix, float(mn), float(np.float32(np.float64(dz) / 255.0)))
    detail = 16.0 if mesh_scale < 0.75 else None
    try:
        for tx, ty in [(0, 0), (-1, 1), (2, -3)]:
            zo, so = orc.tile_create_zvals(tx, ty, 50)
            z = tsm.tile_zvals(orc, S, tx, ty, 50, hmap=True, detail_scale=detail)
            assert_bit_equal(zo, z, f"hmap zvals {tx},{ty}")
            assert tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, z)) == bytes(so)
            assert (tsm.tile_ao(orc, S, tx, ty, z, hmap=True, detail_scale=detail) == orc.tile_ao_lighting(tx, ty, zo)).all(), f"hmap ao {tx},{ty}"
    finally:
        orc.hmap_set(None)


@pytest.mark.parametrize("lpos", [(1.0, 0.6, 0.3), (-0.4, -1.0, 0.15)])
def test_mesh_shadows_at_128(orc, lpos):
    orc.init(orclib.make_config(mesh_gen_mode=0))
    tiles = [(x, y) for y in range(-1, 2) for x in range(-1, 2)]
    z = np.stack([orc.tile_create_zvals(tx, ty, 0)[0] for tx, ty in tiles])
    want = orc.tiles_mesh_shadows(tiles, z, lpos)
    got = tsm.tiles_shadows(orc, S, tiles, z, lpos)
    assert (got == want).all()
    assert (got != 0).any()  # the lights cast shadows here
