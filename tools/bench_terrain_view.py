"""The terrain draw list for a camera (terra_tiles_terrain_view_dev) on device-resident tile batches at S = 128, on the stats and min_normal_z the resident chain leaves
(terra_tiles_create_zvals_dev): a 19 x 19 batch around the camera -- about what a frame holds at TILE_RADIUS 6 and DRAW_DIST_TILES 1.5 -- and the 64 x 64 batch, each
on the default generated terrain with the camera 1.0 above the middle of the centre tile and on the same terrain with the camera 0.05 above it, which is where
occluders bite; a 60-degree, 16:9 view along the ground.  Per batch and camera: microseconds per call of the k_terrain_view_* kernels and, in the same run, of the
driver's one-thread-per-tile form ("kernels.simple": the literal loops), and of the same batch's terra_tiles_create_zvals_dev (zvals, stats and normals), the
yardstick of the other passes; the numbers of occluders, candidates (tiles that reach the occlusion test's place in the loop), occluded and drawn tiles.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls.  The two forms are timed
in --rounds alternating rounds; `spread` is the largest distance between two rounds' medians of the same form -- what a difference between the forms has to exceed.
Both forms' outputs are compared.  Prints one JSON line per batch and camera.
(The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`.)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(t, reps, warmup, fn):
    """median us per call over reps single calls"""
    for _ in range(warmup):
        fn()
    t.synchronize()
    us = []
    for _ in range(reps):
        t.timer_start()
        fn()
        us.append(1000.0 * t.timer_stop())
    return round(float(np.median(us)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[19, 64], help="a batch is side x side tiles")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S = 128
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    angle, aspect = 0.5236, 16.0 / 9.0
    zmin = float(t.state().zmin)
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        bufs = [t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4), t.alloc(n), t.alloc(n * 4), t.alloc(n), t.alloc(n * 4),
                t.alloc(n * 4), t.alloc(n * 4), t.alloc(8)]
        zb, st, nm, mnz, su, di, lod, cr, dr, oc, cn = bufs
        zvals_us = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(zb.download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        args = pkg.make_terrain_view_args(t.view_behind_sphere_mult(angle, aspect), zmin, 1, 1, 0)
        for camera, height in (("default", 1.0), ("low", 0.05)):
            view = t.make_view((0.0, 0.0, zc + height), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
            call = lambda: t.tiles_terrain_view_dev(tiles, view, args, st.ptr, su.ptr, di.ptr, lod.ptr, cr.ptr, dr.ptr, oc.ptr, cn.ptr, min_normal_z_ptr=mnz.ptr)  # noqa: E731
            out = {"tiles": n, "tile_size": S, "camera": camera, "camera_height": height, "reps": a.reps, "rounds": a.rounds, "create_zvals_us": zvals_us}
            rounds = {"default": [], "simple": []}
            result = {}
            for _ in range(a.rounds):
                for form in ("default", "simple"):
                    t.set_option("kernels.simple", "1" if form == "simple" else "0")
                    try:
                        rounds[form].append(timed(t, a.reps, a.warmup, call))
                    finally:
                        t.set_option("kernels.simple", "0")
                    if form not in result:
                        c = cn.download(np.uint32, (2,)).copy()
                        result[form] = (c, su.download(np.uint8, (n,)).copy(), di.download(np.float32, (n,)).copy(), lod.download(np.uint8, (n,)).copy(),
                                        cr.download(np.uint8, (n, 4)).copy(), dr.download(np.uint32, (n,))[:c[0]].copy(), oc.download(np.uint32, (n,))[:c[1]].copy())
            for x, y in zip(result["default"], result["simple"]):
                assert x.tobytes() == y.tobytes(), "the two forms disagree"
            c, status = result["default"][0], result["default"][1]
            low = status & 7
            out["occluders"], out["candidates"] = int((status & 0x80 != 0).sum()), int((low >= 4).sum())
            out["occluded"], out["drawn"], out["not_visible"], out["too_far"] = int(c[1]), int(c[0]), int((low == 2).sum()), int((low == 1).sum())
            for form in ("default", "simple"):
                out[f"terrain_view_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
            out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
            out["default_over_simple"] = round(out["terrain_view_default_us"]["median"] / out["terrain_view_simple_us"]["median"], 4)
            out["view_over_zvals"] = round(out["terrain_view_default_us"]["median"] / zvals_us, 3)
            print(json.dumps(out), flush=True)
        for b in bufs:
            b.free()
    t.close()


if __name__ == "__main__":
    main()
