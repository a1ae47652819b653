"""The grass brush (terra_tiles_edit_grass[_dev]) through HIP on the MI355X (k_grass_brush_texels + k_grass_brush_tiles, and the simple form under
"kernels.simple") against tests/grass_brush_model.py, byte for byte: the emulator's cases, and 20 strokes in place on a device-resident 64 x 64 batch."""
import ctypes as C

import numpy as np
import pytest

import grass_brush_cases as gbc
import grass_brush_model as gbm
import orclib

pytestmark = pytest.mark.gpu


def test_cases(pkg, gpu, orc):
    gbc.run_cases(pkg, gpu, orc)


def test_cases_simple_form(pkg, gpu, orc):
    gpu.set_option("kernels.simple", "1")
    try:
        gbc.run_cases(pkg, gpu, orc)
    finally:
        gpu.set_option("kernels.simple", "0")


def test_resident_batch_strokes(pkg, gpu, orc):
    """the full 64 x 64 batch made on the device (terra_tiles_create_zvals_dev + terra_tiles_create_weights_dev, grass_density > 0), then 20 strokes in place:
    after each, the touched tiles equal the model and every other tile is unchanged, byte for byte"""
    cfg = pkg.make_config(mesh_gen_mode=0)
    gpu.init_scene(cfg)
    orc.init(orclib.make_config(mesh_gen_mode=0))
    ls = orclib.make_landscape(grass_density=1)
    gpu.set_landscape(pkg.make_landscape(grass_density=1))
    orc.set_landscape(ls)
    sc = gbm.Scene(orc, cfg, ls)
    tiles = [(x, y) for y in range(-32, 32) for x in range(-32, 32)]
    n = len(tiles)
    zb, sb = gpu.alloc(n * 130 * 130 * 4), gpu.alloc(n * C.sizeof(pkg.TileStats))
    wb, gb, ub, rb = gpu.alloc(n * 129 * 129 * 4), gpu.alloc(n * 32 * 32 * 12), gpu.alloc(n), gpu.alloc(n * 16)
    try:
        gpu.tiles_create_zvals_dev(tiles, 0, zb.ptr, sb.ptr)
        gpu.tiles_create_weights_dev(tiles, zb.ptr, wb.ptr, gb.ptr)
        z = zb.download(np.float32, (n, 130, 130))
        stats = (pkg.TileStats * n).from_buffer_copy(sb.download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        w = wb.download(np.uint8, (n, 129, 129, 4))
        blocks = gb.download(orclib.GRASS_BLOCK_DTYPE, (n, 32, 32))
        assert (blocks["ix"] != 0).any() and (w[..., gbm.GRASS] > 0).any()
        rs = np.random.RandomState(11)
        land = [i for i in range(n) if (w[i, ..., gbm.GRASS] > 0).sum() > 2000]
        touched_total = 0
        for k in range(20):
            i = land[rs.randint(len(land))] if k % 4 else rs.randint(n)
            tx_i, ty_i = (int(v) for v in rs.randint(0, 129, 2))
            x, y = gbc.texel_pos(sc, tiles[i], tx_i, ty_i)
            radius = float(sc.DX_VAL) * (float(rs.choice([2.0, 8.0, 32.0])) + 0.5)
            brush = pkg.make_grass_brush((x, y, float(z[i, ty_i, tx_i])), radius, k % 3 != 1, int(rs.randint(8)), float(rs.choice([0.004, 0.02, 0.05, 0.12])))
            gpu.tiles_edit_grass_dev(tiles, zb.ptr, sb.ptr, brush, wb.ptr, gb.ptr, ub.ptr, rb.ptr)
            upd = np.zeros(n, bool); rg = np.tile(np.array([128, 128, 0, 0], np.uint32), (n, 1))
            pos = tuple(gbm.f32(v) for v in brush.pos)
            for j, (tx, ty) in enumerate(tiles):
                if not gbm.mesh_sphere_intersect(sc, tx * 128, ty * 128, 0, 0, stats[j], pos, gbm.f32(brush.radius)):
                    continue
                upd[j], rg[j] = gbm.add_or_remove_grass_at(sc, tx, ty, z[j], stats[j], w[j], blocks[j], orc.tile_terrain_params(tx, ty), brush.pos, brush.radius,
                                                           bool(brush.add_grass), brush.shape, brush.brush_weight)
            gbc.compare(f"stroke {k}", (wb.download(np.uint8, w.shape), gb.download(orclib.GRASS_BLOCK_DTYPE, blocks.shape), ub.download(np.uint8, (n,)).astype(bool),
                                        rb.download(np.uint32, (n, 4))), (w, blocks, upd, rg))
            touched_total += int(upd.sum())
        assert touched_total >= 10
    finally:
        for b in (zb, sb, wb, gb, ub, rb):
            b.free()
