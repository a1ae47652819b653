"""Tiles at a tile size S = mesh_x other than 128 through the host emulator (tests/emul: the same driver, the size-general bodies of terra_simple_paths.hpp),
against tests/tile_size_model.py: every entry point that follows S, terra_tile_size, and the entry points that are refused at S != 128."""
import ctypes as C

import numpy as np
import pytest

import orclib
import tile_size_model as tsm
from orclib import assert_bit_equal

TILES = [(0, 0), (-1, 0), (0, -1), (-1, -1), (1, -2), (0, 0)]  # mixed signs, (0, 0) twice


def scenes(pkg, t, orc, S, mode=0, **kw):
    t.init_scene(pkg.make_config(mesh_gen_mode=mode, mesh_xy=S, **kw))
    orc.init(orclib.make_config(mesh_gen_mode=mode, mesh_xy=S, **kw))


def check_tiles(orc, S, tiles, z, st, nm, mnz, iters, what, **kw):
    for i, (tx, ty) in enumerate(tiles):
        zm = tsm.tile_zvals(orc, S, tx, ty, iters, **kw)
        assert_bit_equal(zm, z[i], f"{what} zvals S={S} tile {tx},{ty}")
        if st is not None:
            assert bytes(st[i]) == tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, zm)), f"{what} stats S={S} tile {tx},{ty}"
        if nm is not None:
            nmm, mm = tsm.tile_normals(orc, S, zm)
            assert (nm[i] == nmm).all(), f"{what} normals S={S} tile {tx},{ty}"
            assert np.float32(mnz[i]).view(np.uint32) == np.float32(mm).view(np.uint32)


@pytest.mark.parametrize("S", [64, 192])
@pytest.mark.parametrize("iters", [0, 200])
def test_zvals_post_ao_shadows(pkg, emul, orc, S, iters):
    scenes(pkg, emul, orc, S)
    assert emul.tile_size == S
    z, st, nm, mnz = emul.tiles_create_zvals(TILES, iters)
    assert z.shape == (len(TILES), S + 2, S + 2) and nm.shape == (len(TILES), S + 1, S + 1, 4)
    check_tiles(orc, S, TILES, z, st, nm, mnz, iters, "create")
    # the post pass alone over the caller's zvals
    n = len(TILES)
    zb = emul.alloc(z.nbytes).upload(z)
    sb, nb, mb = emul.alloc(n * C.sizeof(pkg.TileStats)), emul.alloc(nm.nbytes), emul.alloc(4 * n)
    emul.tiles_post_dev(TILES, zb.ptr, sb.ptr, nb.ptr, mb.ptr)
    st2 = (pkg.TileStats * n).from_buffer_copy(sb.download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
    assert all(bytes(st2[i]) == bytes(st[i]) for i in range(n))
    assert (nb.download(np.uint8, nm.shape) == nm).all() and (mb.download(np.float32, (n,)).view(np.uint32) == mnz.view(np.uint32)).all()
    for b in (zb, sb, nb, mb):
        b.free()
    ao = emul.tiles_ao_lighting(TILES, z)
    assert ao.shape == (n, S + 1, S + 1)
    for i, (tx, ty) in enumerate(TILES[:3]):
        assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i])).all(), f"ao S={S} tile {tx},{ty}"
    block = [(x, y) for y in range(-1, 1) for x in range(-1, 1)]
    zb_ = np.stack([z[TILES.index(t)] for t in block])
    for lpos in ((1.0, 0.6, 0.3), (-0.4, -1.0, 0.15)):
        sm = emul.tiles_mesh_shadows(block, zb_, lpos)
        want = tsm.tiles_shadows(orc, S, block, zb_, lpos)
        assert (sm == want).all(), f"shadows S={S} light {lpos}"
        assert (sm != 0).any()


@pytest.mark.parametrize("S", [64])
def test_ao_context_clip(pkg, emul, orc, S):
    scenes(pkg, emul, orc, S, mode=4)
    emul.set_tiled_mesh_ao(1); orc.set_tiled_mesh_ao(1)
    try:
        tiles = [(0, 0), (-1, 1)]
        z, st, nm, mnz = emul.tiles_create_zvals(tiles, 200)
        check_tiles(orc, S, tiles, z, st, nm, mnz, 200, "clip", ao_clip=True)
        ao = emul.tiles_ao_lighting(tiles, z)
        for i, (tx, ty) in enumerate(tiles):
            assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i], ao_clip=True)).all()
    finally:
        emul.set_tiled_mesh_ao(0); orc.set_tiled_mesh_ao(0)


@pytest.mark.parametrize("S", [64])
def test_heightmap_tiles(pkg, emul, orc, S):
    s0 = orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S))
    n = 96
    g = orc.gen_grid(-n / 2, -n / 2, s0.DX_VAL, s0.DY_VAL, n, n, 1)
    q, mn, dz = orc.quantize16(g)
    pix = np.ascontiguousarray(q.reshape(n, n, 2))
    dzs = float(np.float32(np.float64(dz) / 255.0))
    scenes(pkg, emul, orc, S)
    buf = emul.alloc(pix.nbytes).upload(pix)
    emul.hmap_set_dev(buf.ptr, n, n, 2, float(mn), dzs)
    orc.hmap_set(pix, float(mn), dzs)
    try:
        tiles = [(0, 0), (-1, 0), (1, 1), (-3, 2)]  # (1, 1) and (-3, 2) reach past the image: mirror wrap
        z, st, nm, mnz = emul.tiles_create_zvals(tiles, 200)
        check_tiles(orc, S, tiles, z, st, nm, mnz, 0, "hmap", hmap=True)
        ao = emul.tiles_ao_lighting(tiles, z)
        for i, (tx, ty) in enumerate(tiles[:2]):
            assert (ao[i] == tsm.tile_ao(orc, S, tx, ty, z[i], hmap=True)).all()
    finally:
        emul.hmap_set_dev(None); orc.hmap_set(None)
        buf.free()


def test_multi_tiles_create_zvals(pkg, emul_lib, orc):
    S = 64
    m = pkg.TerraMulti([0, 0], emul_lib)
    try:
        m.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
        orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S))
        tiles = TILES[:5]
        z, st, nm, mnz = m.tiles_create_zvals(tiles, 200)
        check_tiles(orc, S, tiles, z, st, nm, mnz, 200, "multi")
    finally:
        m.close()


def test_refused_entry_points(pkg, emul):
    ERR_ARG = -1
    emul.init_scene(pkg.make_config(mesh_xy=64))
    tiles = [(0, 0), (1, 0)]
    z = np.zeros((2, 66, 66), np.float32)
    zb = emul.alloc(z.nbytes).upload(z)
    sm = emul.alloc(2 * 66 * 66)
    lib, ctx = emul.lib, emul.ctx
    txy = np.array(tiles, np.int32)
    lp = (C.c_float * 3)(1.0, 0.5, 0.3)
    try:
        assert lib.terra_tiles_terrain_params(ctx, txy.ctypes.data, 2, np.zeros(24, np.float32).ctypes.data) == ERR_ARG
        assert lib.terra_tiles_create_weights_dev(ctx, txy.ctypes.data, 2, zb.ptr, sm.ptr, None, None) == ERR_ARG
        w = np.zeros(2 * 129 * 129 * 4, np.uint8)
        assert lib.terra_tiles_create_weights(ctx, txy.ctypes.data, 2, z.ctypes.data, w.ctypes.data, None, None) == ERR_ARG
        eo = np.zeros(2 * 2 * 130, np.float32)
        assert lib.terra_tiles_mesh_shadows_halo_dev(ctx, txy.ctypes.data, 2, zb.ptr, lp, sm.ptr, None, None, eo.ctypes.data) == ERR_ARG
        ep = np.ones(4, np.uint8)
        assert lib.terra_tiles_mesh_shadows_edges_dev(ctx, txy.ctypes.data, 2, zb.ptr, lp, sm.ptr, zb.ptr, ep.ctypes.data, None) == ERR_ARG
        assert "tile size 128" in lib.terra_last_error().decode()
    finally:
        zb.free(); sm.free()
    # a size outside the range, mesh_x != mesh_y, a size of the form 4k + 2: every tile call is refused
    for cfg in (pkg.make_config(mesh_xy=8), pkg.make_config(mesh_xy=2048), pkg.make_config(mesh_xy=130)):
        emul.init_scene(cfg)
        with pytest.raises(pkg.TerraError) as e:
            emul.tile_size
        assert e.value.code == ERR_ARG
        with pytest.raises(pkg.TerraError):
            emul.tiles_create_zvals([(0, 0)], 0)
    c = pkg.make_config(mesh_xy=64); c.mesh_y = 128
    emul.init_scene(c)
    with pytest.raises(pkg.TerraError) as e:
        emul.tiles_create_zvals([(0, 0)], 0)
    assert e.value.code == ERR_ARG and "mesh_y" in str(e.value)
    n = np.zeros(1, np.uint32)
    assert lib.terra_tile_size(ctx, n.ctypes.data_as(C.POINTER(C.c_uint32))) == ERR_ARG
    # at 128 mesh_y may differ, as before
    c = pkg.make_config(mesh_xy=128); c.mesh_y = 256
    emul.init_scene(c)
    assert emul.tile_size == 128


def test_multi_shadows_refused(pkg, emul_lib):
    m = pkg.TerraMulti([0, 0], emul_lib)
    try:
        m.init_scene(pkg.make_config(mesh_xy=64))
        txy = np.array([(0, 0), (1, 0)], np.int32)
        lp = (C.c_float * 3)(1.0, 0.5, 0.3)
        z = np.zeros(2 * 66 * 66, np.float32); sm = np.zeros(2 * 66 * 66, np.uint8)
        assert m.lib.terra_multi_tiles_mesh_shadows(m.m, txy.ctypes.data, 2, z.ctypes.data, lp, sm.ctypes.data) == -1
        own = np.zeros(2, np.uint32)
        assert m.lib.terra_multi_shadow_layout(m.m, txy.ctypes.data, 2, lp, own.ctypes.data, None, None) == -1
    finally:
        m.close()
