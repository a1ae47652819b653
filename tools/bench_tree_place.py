"""Tree placement (terra_tiles_place_trees_dev) on a device-resident tile batch at S = 128 (64 x 64 = 4096 tiles by default) at the reference's default tree
settings with tree_mode 2: microseconds per call and trees per second, and as the yardstick the same batch's terra_tiles_create_zvals_dev (zvals, stats and
normals) from the same run.  Every repetition is timed on its own with device events on the context's stream, after a warm-up; the figure is the median.
Prints one JSON line.  (The kernels' own time: run this under `rocprofv3 --kernel-trace --stats`.)"""
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
    return float(np.median(us)), float(min(us)), float(max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--side", type=int, default=64, help="the batch is side x side tiles")
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--mode", type=int, default=0, help="mesh_gen_mode")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    t.init_scene(pkg.make_config(mesh_gen_mode=a.mode))
    t.set_landscape(pkg.make_landscape())
    t.set_tree_params(pkg.make_tree_params(tree_mode=2))
    tiles = np.array([(x, y) for y in range(-a.side // 2, a.side // 2) for x in range(-a.side // 2, a.side // 2)], np.int32)
    n, S, cap = len(tiles), 128, a.capacity
    W, Z = S + 1, S + 2
    zb, st, nm, mnz = t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4)
    tr, cn = t.alloc(n * cap * 40), t.alloc(n * 4)
    out = {"tiles": n, "tile_size": S, "mesh_gen_mode": a.mode, "capacity": cap, "reps": a.reps}
    med, lo, hi = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
    out["create_zvals_us"] = {"median": round(med, 1), "min": round(lo, 1), "max": round(hi, 1)}
    med, lo, hi = timed(t, a.reps, a.warmup, lambda: t.tiles_place_trees_dev(tiles, cap, tr.ptr, cn.ptr, 0, 0, None, st.ptr))
    counts = cn.download(np.uint32, (n,))
    ntrees = int(counts.sum())
    out["place_trees_us"] = {"median": round(med, 1), "min": round(lo, 1), "max": round(hi, 1)}
    out["trees"] = ntrees
    out["max_trees_per_tile"] = int(counts.max())
    out["trees_per_s"] = round(ntrees / med * 1e6)
    out["place_over_zvals"] = round(med / out["create_zvals_us"]["median"], 3)
    for b in (zb, st, nm, mnz, tr, cn):
        b.free()
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
