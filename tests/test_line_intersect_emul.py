"""Line-vs-terrain hits (terra_tiles_line_intersect[_dev], tile_draw_t::line_intersect_mesh) through the host emulator -- the driver's one-thread-per-line form --
against tests/line_intersect_model.py, byte for byte; hand-derived anchors for the model itself; the argument checks."""
import ctypes as C

import numpy as np

import line_intersect_cases as lic
import line_intersect_model as lim

f32 = np.float32


def anchor_batch(pkg, t, kind):
    """one synthetic tile (0, 0) at S = 128 (scene_x = scene_y = 4: DX_VAL = 1/16, the tile spans x, y in [-4, 4)) and its stats"""
    cfg = pkg.make_config(mesh_gen_mode=0)
    st = t.init_scene(cfg)
    sc = lim.Scene.of(cfg, st)
    assert float(sc.DX_VAL) == 0.0625 and float(sc.DX_VAL_INV) == 16.0
    z, zmin, zmax = lic.synthetic(sc, kind)
    stats = (pkg.TileStats * 1)()
    stats[0].mzmin, stats[0].mzmax = zmin, zmax
    return dict(sc=sc, tiles=[(0, 0)], z=z[None], stats=stats)


def both(t, d, lines):
    """the model's records, checked equal to the library's"""
    return lic.run(t, d, np.array(lines, f32), what="anchor")


def test_anchor_vertical_line_on_constant_tile(pkg, emul):
    """constant height 0.75; a vertical line at cell (10, 20) from z = 3 to z = -1.  The clip leaves v1c.z = 0.75 + 1e-6 and v2c.z = 0.75 - 1e-6 (both x and y
    stay), so xp = yp = (10, 20) at both ends: steps = 1, zinc = -2e-6, z = 0.7500008 (not below 0.75), then 0.7499988: a hit at the second step with
    cur_t = ((z - 0.5*zinc) - 3)/(-1 - 3) = (0.7499998 - 3)/(-4) = 0.5625 (within 2e-7)"""
    d = anchor_batch(pkg, emul, "const")
    x, y = -4.0 + 10 / 16, -4.0 + 20 / 16
    h = both(emul, d, [[[x, y, 3.0], [x, y, -1.0]]])[0]
    assert h["hit"] == 1 and h["tile"] == 0 and (h["xpos"], h["ypos"]) == (10, 20)
    assert abs(float(h["t"]) - 0.5625) < 2e-7
    assert np.allclose(h["p_int"], [x, y, 0.75], atol=1e-6)


def test_anchor_ramp(pkg, emul):
    """ramp z = ix/16 at column ix; the line from (-4, y, 2) to (4, y, -6) descends one unit per unit of x.  Its clip ends where it leaves the box's bottom
    (z = -1e-6, x = -2): xp 0 -> 32, steps = 32, xinc = 1, zinc = -2/32, z_k = 2 - 0.1/16 - k/16.  The first column whose height exceeds z_k:
    k/16 > 2 - 0.00625 - k/16  <=>  k > 15.95  ->  ix = 16, and cur_t = ((z_16 + 1/32) - 2)/(-8) = 0.121875 (within 1e-6)"""
    d = anchor_batch(pkg, emul, "ramp")
    y = -4.0 + 7 / 16
    h = both(emul, d, [[[-4.0, y, 2.0], [4.0, y, -6.0]]])[0]
    assert h["hit"] == 1 and (h["xpos"], h["ypos"]) == (16, 7)
    assert abs(float(h["t"]) - 0.121875) < 1e-6
    assert np.allclose(h["p_int"], [-4.0 + 8 * 0.121875, y, 2.0 - 8 * 0.121875], atol=1e-5)


def test_anchor_line_above_tile(pkg, emul):
    """both ends above mzmax + 1e-6: get_region gives both 0x20, the clip rejects the tile -> the miss record"""
    d = anchor_batch(pkg, emul, "ramp")
    h = both(emul, d, [[[-3.0, 0.5, 9.0], [3.0, 0.25, 8.2]]])[0]
    assert h.tobytes() == np.array([(2.0, -1, 0, 0, (0, 0, 0), 0)], lim.HIT_DTYPE).tobytes()


def test_cases(pkg, emul):
    lic.run_cases(pkg, emul)


def test_cases_tile_size_64(pkg, emul):
    lic.run_cases(pkg, emul, S=64)


def test_dev_entry_point(pkg, emul):
    """the device-pointer form on the emulator's "device" memory; a d_line_tile entry >= n is a miss there"""
    d = lic.setup(pkg, emul)
    n = len(d["tiles"])
    rs = np.random.RandomState(3)
    lines = lic.camera_rays(d["sc"], d["tiles"], d["z"], rs, 64)
    lt = np.full(64, -1, np.int32)
    lt[::4], lt[1::4] = 2, n + 3
    want = lic.model(d, lines, np.where(lt >= n, 2**30, lt))
    assert not want["hit"][1::4].any()
    zb, sb, lb, tb, hb = emul.alloc(d["z"].nbytes).upload(d["z"]), emul.alloc(C.sizeof(d["stats"])), emul.alloc(lines.nbytes).upload(lines), emul.alloc(lt.nbytes).upload(lt), emul.alloc(64 * 32)
    C.memmove(sb.ptr, C.addressof(d["stats"]), C.sizeof(d["stats"]))
    try:
        emul.tiles_line_intersect_dev(d["tiles"], zb.ptr, sb.ptr, lb.ptr, 64, hb.ptr, tb.ptr)
        lic.compare("dev", hb.download(pkg.LINE_HIT_DTYPE, (64,)), want)
        emul.tiles_line_intersect_dev(d["tiles"], zb.ptr, sb.ptr, lb.ptr, 64, hb.ptr)  # no restriction
        lic.compare("dev, whole batch", hb.download(pkg.LINE_HIT_DTYPE, (64,)), lic.model(d, lines))
    finally:
        for b in (zb, sb, lb, tb, hb):
            b.free()


def test_arguments(pkg, emul, emul_lib):
    lib, ctx = emul.lib, emul.ctx
    d = lic.setup(pkg, emul)
    n = len(d["tiles"])
    txy = np.array(d["tiles"], np.int32)
    z, st = d["z"], C.addressof(d["stats"])
    lines = lic.camera_rays(d["sc"], d["tiles"], d["z"], np.random.RandomState(5), 4)
    hits = np.zeros(4, pkg.LINE_HIT_DTYPE)

    def call(nn=n, zp=z.ctypes.data, sp=st, lp=lines.ctypes.data, lt=None, nl=4, hp=hits.ctypes.data, txp=txy.ctypes.data, dev=False):
        f = lib.terra_tiles_line_intersect_dev if dev else lib.terra_tiles_line_intersect
        return f(ctx, txp, nn, 0, 0, zp, sp, None, lp, lt, nl, hp)
    assert call() == 0 and hits["hit"].any()
    for dev in (False, True):  # a null required pointer
        assert call(zp=None, dev=dev) == lic.ERR_ARG and call(sp=None, dev=dev) == lic.ERR_ARG and call(txp=None, dev=dev) == lic.ERR_ARG
        assert call(lp=None, dev=dev) == lic.ERR_ARG and call(hp=None, dev=dev) == lic.ERR_ARG
        assert call(lp=None, hp=None, nl=0, dev=dev) == 0  # nlines == 0: nothing to read or write
    # nlines == 0 writes nothing; n == 0 writes misses (tile arrays may then be null)
    hits[:] = np.array([(0.5, 9, 1, 2, (1, 2, 3), 7)], pkg.LINE_HIT_DTYPE)
    keep = hits.tobytes()
    assert call(nl=0) == 0 and hits.tobytes() == keep
    assert call(nn=0, zp=None, sp=None, txp=None) == 0
    assert hits.tobytes() == np.tile(np.array([(2.0, -1, 0, 0, (0, 0, 0), 0)], pkg.LINE_HIT_DTYPE), 4).tobytes()
    # the host form refuses a line_tile entry >= n; negative entries mean the whole batch
    lt = np.array([-1, 0, n, -7], np.int32)
    assert call(lt=lt.ctypes.data) == lic.ERR_ARG and "line_tile" in lib.terra_last_error().decode()
    lt[2] = n - 1
    assert call(lt=lt.ctypes.data) == 0
    # an unsupported tile size (4k + 2) is TERRA_ERR_ARG; before terra_init_scene TERRA_ERR_STATE
    emul.init_scene(pkg.make_config(mesh_xy=66))
    assert call() == lic.ERR_ARG and call(dev=True) == lic.ERR_ARG
    fresh = pkg.Terra(0, emul_lib)
    try:
        for f in (fresh.lib.terra_tiles_line_intersect, fresh.lib.terra_tiles_line_intersect_dev):
            assert f(fresh.ctx, txy.ctypes.data, n, 0, 0, z.ctypes.data, st, None, lines.ctypes.data, None, 4, hits.ctypes.data) == lic.ERR_STATE
    finally:
        fresh.close()
