"""The grass brush (terra_tiles_edit_grass, tile_t::add_or_remove_grass_at) through the host emulator -- the driver's per-texel / per-block / per-tile form --
against tests/grass_brush_model.py, byte for byte; plus the argument checks."""
import ctypes as C

import numpy as np
import pytest

import grass_brush_cases as gbc


def test_cases(pkg, emul, orc):
    gbc.run_cases(pkg, emul, orc)


def test_stroke_chain(pkg, emul, orc):
    """20 strokes applied one after another: the state each leaves is the next one's input, on both sides"""
    sc, d = gbc.setup(pkg, emul, orc)
    lib_d, mod_d = gbc.copy(d), gbc.copy(d)
    touched = 0
    for k, brush in enumerate(gbc.strokes(sc, d)):
        u1, r1 = gbc.lib_stroke(emul, lib_d, brush)
        u2, r2 = gbc.model_stroke(sc, mod_d, brush)
        gbc.compare(f"stroke {k}", (lib_d["w"], lib_d["gb"], u1, r1), (mod_d["w"], mod_d["gb"], u2, r2))
        touched += int(u2.sum())
    assert touched >= 10
    assert (lib_d["w"] != d["w"]).any()


def test_dev_entry_point(pkg, emul, orc):
    """the device-pointer form on the emulator's "device" memory, ranges optional"""
    sc, d = gbc.setup(pkg, emul, orc)
    brush = gbc.cases(sc, d)[0][1]
    n = len(d["tiles"])
    zb, sb = emul.alloc(d["z"].nbytes).upload(d["z"]), emul.alloc(C.sizeof(d["stats"]))
    C.memmove(sb.ptr, C.addressof(d["stats"]), C.sizeof(d["stats"]))
    wb, gb, ub, rb = emul.alloc(d["w"].nbytes).upload(d["w"]), emul.alloc(d["gb"].nbytes).upload(d["gb"]), emul.alloc(n), emul.alloc(16 * n)
    try:
        emul.tiles_edit_grass_dev(d["tiles"], zb.ptr, sb.ptr, brush, wb.ptr, gb.ptr, ub.ptr, rb.ptr)
        mod_d = gbc.copy(d)
        u2, r2 = gbc.model_stroke(sc, mod_d, brush)
        gbc.compare("dev", (wb.download(np.uint8, d["w"].shape), gb.download(pkg.GRASS_BLOCK_DTYPE, d["gb"].shape), ub.download(np.uint8, (n,)).astype(bool),
                            rb.download(np.uint32, (n, 4))), (mod_d["w"], mod_d["gb"], u2, r2))
        emul.tiles_edit_grass_dev(d["tiles"], zb.ptr, sb.ptr, brush, wb.ptr, gb.ptr, ub.ptr, None)  # no ranges
    finally:
        for b in (zb, sb, wb, gb, ub, rb):
            b.free()


def test_refused(pkg, emul, orc):
    sc, d = gbc.setup(pkg, emul, orc, tiles=gbc.TILES[:2])
    lib, ctx = emul.lib, emul.ctx
    txy = np.array(d["tiles"], np.int32)
    z, w, gb = d["z"], d["w"], d["gb"]
    upd, rg = np.zeros(2, np.uint8), np.zeros((2, 4), np.uint32)
    brush = pkg.make_grass_brush((0.0, 0.0, 0.0), 0.5, 1, 1, 0.05)

    def call(b=None):
        return lib.terra_tiles_edit_grass(ctx, txy.ctypes.data, 2, 0, 0, z.ctypes.data, C.addressof(d["stats"]), None, C.byref(brush) if b is None else b,
                                          w.ctypes.data, gb.ctypes.data, upd.ctypes.data, rg.ctypes.data)
    assert call() == 0
    assert lib.terra_tiles_edit_grass(ctx, txy.ctypes.data, 2, 0, 0, z.ctypes.data, C.addressof(d["stats"]), None, None, w.ctypes.data, gb.ctypes.data,
                                      upd.ctypes.data, rg.ctypes.data) == gbc.ERR_ARG  # no brush
    assert lib.terra_tiles_edit_grass(ctx, txy.ctypes.data, 2, 0, 0, z.ctypes.data, None, None, C.byref(brush), w.ctypes.data, gb.ctypes.data,
                                      upd.ctypes.data, rg.ctypes.data) == gbc.ERR_ARG  # no stats
    for shape in (-1, 8):
        bad = pkg.make_grass_brush((0.0, 0.0, 0.0), 0.5, 1, shape, 0.05)
        assert call(C.byref(bad)) == gbc.ERR_ARG
        assert "shape" in lib.terra_last_error().decode()
    wb = emul.alloc(w.nbytes + 4)
    try:  # a d_weights that is not 4-byte aligned
        rc = lib.terra_tiles_edit_grass_dev(ctx, txy.ctypes.data, 2, 0, 0, z.ctypes.data, C.addressof(d["stats"]), None, C.byref(brush), wb.ptr + 1,
                                            gb.ctypes.data, upd.ctypes.data, rg.ctypes.data)
        assert rc == gbc.ERR_ARG and "aligned" in lib.terra_last_error().decode()
        for k in range(4):  # a null required pointer
            args = [z.ctypes.data, C.addressof(d["stats"]), wb.ptr, gb.ctypes.data, upd.ctypes.data]
            args[[0, 2, 3, 4][k]] = None
            assert lib.terra_tiles_edit_grass_dev(ctx, txy.ctypes.data, 2, 0, 0, args[0], args[1], None, C.byref(brush), args[2], args[3], args[4], None) == gbc.ERR_ARG
    finally:
        wb.free()
    # the weights family is 128-only: at S = 64 both entry points are refused with the family's message
    emul.init_scene(pkg.make_config(mesh_xy=64))
    assert call() == gbc.ERR_ARG
    assert "tile size 128" in lib.terra_last_error().decode()
    assert lib.terra_tiles_edit_grass_dev(ctx, txy.ctypes.data, 2, 0, 0, z.ctypes.data, C.addressof(d["stats"]), None, C.byref(brush), w.ctypes.data,
                                          gb.ctypes.data, upd.ctypes.data, None) == gbc.ERR_ARG
    assert "tile size 128" in lib.terra_last_error().decode()
