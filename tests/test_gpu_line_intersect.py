"""Line-vs-terrain hits (terra_tiles_line_intersect[_dev]) through HIP on the MI355X (k_line_boxes + k_line_intersect, and the one-thread-per-line form under
"kernels.simple") against tests/line_intersect_model.py, byte for byte: the emulator's cases, then 65536 rays against the full 64 x 64 batch made on the device
at S = 128 and 16384 rays against a 32 x 32 batch at S = 64."""
import ctypes as C

import numpy as np
import pytest

import line_intersect_cases as lic
import line_intersect_model as lim

pytestmark = pytest.mark.gpu


def test_cases(pkg, gpu):
    lic.run_cases(pkg, gpu)


def test_cases_tile_size_64(pkg, gpu):
    lic.run_cases(pkg, gpu, S=64)


def test_cases_simple_form(pkg, gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        lic.run_cases(pkg, gpu)
    finally:
        gpu.set_option("kernels.simple", "0")


def resident_batch_rays(pkg, gpu, S, side, nrays, seed):
    """side x side tiles made on the device (terra_tiles_create_zvals_dev), nrays lines through terra_tiles_line_intersect_dev -- camera rays of length FAR_CLIP
    over the whole batch, every 8th line restricted to one tile (every 64th to an index past the batch: a miss), every 7th tile distant -- vs the model"""
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    sc = lim.Scene.of(cfg, gpu.init_scene(cfg))
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(-side // 2, side // 2)]
    n = len(tiles)
    zb, sb = gpu.alloc(n * (S + 2) ** 2 * 4), gpu.alloc(n * C.sizeof(pkg.TileStats))
    bufs = [zb, sb]
    try:
        gpu.tiles_create_zvals_dev(tiles, 0, zb.ptr, sb.ptr)
        z = zb.download(np.float32, (n, S + 2, S + 2))
        stats = (pkg.TileStats * n).from_buffer_copy(sb.download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        mzmin, mzmax = np.array([s.mzmin for s in stats], np.float32), np.array([s.mzmax for s in stats], np.float32)
        rs = np.random.RandomState(seed)
        lines = lic.camera_rays(sc, tiles, z, rs, nrays)
        lt = np.full(nrays, -1, np.int32)
        lt[::8] = rs.randint(n, size=len(lt[::8]))
        lt[::64] = n + 5
        distant = (np.arange(n) % 7) == 3
        lb, tb, db, hb = gpu.alloc(lines.nbytes).upload(lines), gpu.alloc(lt.nbytes).upload(lt), gpu.alloc(n).upload(distant.astype(np.uint8)), gpu.alloc(nrays * 32)
        bufs += [lb, tb, db, hb]
        gpu.tiles_line_intersect_dev(tiles, zb.ptr, sb.ptr, lb.ptr, nrays, hb.ptr, tb.ptr, distant_ptr=db.ptr)
        got = hb.download(pkg.LINE_HIT_DTYPE, (nrays,))
        want = lim.batch_hits(sc, tiles, z, mzmin, mzmax, lines, lt, 0, 0, distant)
        lic.compare(f"S = {S}, {side} x {side} tiles", got, want)
        assert want["hit"].mean() > 0.5 and not want["hit"][::64].any()
    finally:
        for b in bufs:
            b.free()


def test_resident_batch_65536_rays(pkg, gpu):
    resident_batch_rays(pkg, gpu, 128, 64, 65536, 21)


def test_resident_batch_tile_size_64(pkg, gpu):
    resident_batch_rays(pkg, gpu, 64, 32, 16384, 22)
