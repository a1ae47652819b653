"""Scenery placement (terra_tiles_place_scenery_dev) on a device-resident tile batch at S = 128 (64 x 64 = 4096 tiles by default) at the reference's defaults, in
sine mode and under domain warp: microseconds per call and objects per second for k_scenery_place and, in the same run, for the driver's one-thread-per-tile form
("kernels.simple"), for terra_tiles_place_trees_dev (tree_mode 3) and for the same batch's terra_tiles_create_zvals_dev (zvals, stats and normals).  Every
repetition is timed on its own with device events on the context's stream, after a warm-up; the figure is the median.  Prints one JSON line per mode.
(The kernels' own time: run this under `rocprofv3 --kernel-trace --stats`.)"""
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
    """us per call: (median, min, max) over reps single calls"""
    for _ in range(warmup):
        fn()
    t.synchronize()
    us = []
    for _ in range(reps):
        t.timer_start()
        fn()
        us.append(1000.0 * t.timer_stop())
    return {"median": round(float(np.median(us)), 1), "min": round(float(min(us)), 1), "max": round(float(max(us)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--simple-reps", type=int, default=5, help="repetitions of the one-thread-per-tile form (0: skip it)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--side", type=int, default=64, help="the batch is side x side tiles")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 4], help="mesh_gen_mode values (0: sine, 4: domain warp)")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    tiles = np.array([(x, y) for y in range(-a.side // 2, a.side // 2) for x in range(-a.side // 2, a.side // 2)], np.int32)
    n, S, cap, nk = len(tiles), 128, a.capacity, len(pkg.SCENERY_KINDS)
    W, Z = S + 1, S + 2
    zb, st, nm, mnz = t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4)
    tr, ob, cn, kc = t.alloc(n * 1024 * 40), t.alloc(n * cap * 72), t.alloc(n * 4), t.alloc(n * nk * 4)
    for mode in a.modes:
        t.init_scene(pkg.make_config(mesh_gen_mode=mode))
        t.set_landscape(pkg.make_landscape())
        t.set_tree_params(pkg.make_tree_params(tree_mode=3))
        t.set_scenery_params(pkg.make_scenery_params())
        out = {"tiles": n, "tile_size": S, "mesh_gen_mode": mode, "capacity": cap, "reps": a.reps}
        out["create_zvals_us"] = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        out["place_trees_us"] = timed(t, a.reps, a.warmup, lambda: t.tiles_place_trees_dev(tiles, 1024, tr.ptr, cn.ptr, 0, 0, None, st.ptr))
        out["pine_palm_trees"] = int(cn.download(np.uint32, (n,)).sum())
        scenery = lambda: t.tiles_place_scenery_dev(tiles, cap, ob.ptr, cn.ptr, 0, 0, None, kc.ptr)  # noqa: E731
        out["place_scenery_us"] = timed(t, a.reps, a.warmup, scenery)
        counts, kinds = cn.download(np.uint32, (n,)), kc.download(np.uint32, (n, nk))
        out["objects"], out["max_objects_per_tile"] = int(counts.sum()), int(counts.max())
        out["objects_by_kind"] = dict(zip(pkg.SCENERY_KINDS, kinds.sum(axis=0).tolist()))
        out["objects_per_s"] = round(out["objects"] / out["place_scenery_us"]["median"] * 1e6)
        out["scenery_over_zvals"] = round(out["place_scenery_us"]["median"] / out["create_zvals_us"]["median"], 3)
        if a.simple_reps:
            t.set_option("kernels.simple", "1")
            try:
                out["place_scenery_simple_us"] = timed(t, a.simple_reps, 1, scenery)
            finally:
                t.set_option("kernels.simple", "0")
            assert (cn.download(np.uint32, (n,)) == counts).all() and (kc.download(np.uint32, (n, nk)) == kinds).all()
            out["kernel_over_simple"] = round(out["place_scenery_us"]["median"] / out["place_scenery_simple_us"]["median"], 4)
        print(json.dumps(out), flush=True)
    for b in (zb, st, nm, mnz, tr, ob, cn, kc):
        b.free()
    t.close()


if __name__ == "__main__":
    main()
