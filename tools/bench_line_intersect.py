"""Line-vs-terrain hits (terra_tiles_line_intersect_dev) against a device-resident 64 x 64 tile batch at S = 128 (4096 tiles): microseconds per call for 1 line
(the fire-mode case, including the read-back of its 32-byte record), 1024 and 65536 lines, and lines per second at 65536.  The lines are camera rays of length
FAR_CLIP aimed at random terrain points.  Prints one JSON line."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import line_intersect_cases as lic
    import line_intersect_model as lim
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    cfg = pkg.make_config(mesh_gen_mode=0)
    sc = lim.Scene.of(cfg, t.init_scene(cfg))
    tiles = np.array([(x, y) for y in range(-32, 32) for x in range(-32, 32)], np.int32)  # (an int32 array: the binding passes it through without a conversion)
    n, S = len(tiles), 128
    zb, sb = t.alloc(n * (S + 2) ** 2 * 4), t.alloc(n * C.sizeof(pkg.TileStats))
    t.tiles_create_zvals_dev(tiles, 0, zb.ptr, sb.ptr)
    z = zb.download(np.float32, (n, S + 2, S + 2))
    lines = lic.camera_rays(sc, tiles, z, np.random.RandomState(1), 65536)
    lb, hb = t.alloc(lines.nbytes).upload(lines), t.alloc(65536 * 32)
    rec = np.zeros(1, pkg.LINE_HIT_DTYPE)
    out = {"tiles": n, "tile_size": S, "us_per_call": {}}

    def one():  # the fire-mode call: one line, then its record back on the host
        t.tiles_line_intersect_dev(tiles, zb.ptr, sb.ptr, lb.ptr, 1, hb.ptr)
        t._ck(t.lib.terra_memcpy_d2h(t.ctx, rec.ctypes.data, hb.ptr, 32))
    for _ in range(a.warmup):
        one()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        one()
    out["us_per_call"]["1"] = round(1e6 * (time.perf_counter() - t0) / a.calls, 2)
    for nl in (1024, 65536):
        calls = a.calls if nl <= 1024 else max(5, a.calls // 20)
        for _ in range(a.warmup):
            t.tiles_line_intersect_dev(tiles, zb.ptr, sb.ptr, lb.ptr, nl, hb.ptr)
        t.synchronize()
        t.timer_start()
        for _ in range(calls):
            t.tiles_line_intersect_dev(tiles, zb.ptr, sb.ptr, lb.ptr, nl, hb.ptr)
        ms = t.timer_stop()
        out["us_per_call"][str(nl)] = round(1000.0 * ms / calls, 2)
    out["lines_per_s"] = round(65536 / (out["us_per_call"]["65536"] * 1e-6))
    out["hits_of_65536"] = int(hb.download(pkg.LINE_HIT_DTYPE, (65536,))["hit"].sum())
    for b in (zb, sb, lb, hb):
        b.free()
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
