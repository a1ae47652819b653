"""The flowers (terra_tiles_place_flowers_dev) on device-resident tile batches at S = 128 with flower_density 2.0 (scene_config/config.txt:43), on the weights the
resident chain leaves (zvals -> terra_tiles_create_weights_dev -> terra_tiles_tree_weights_dev without a tree map): a 3 x 3 batch -- the reference generates flowers
only near the camera, a handful of tiles a frame -- and a 64 x 64 batch.  Per batch: microseconds per call of k_flowers_place (one wave per tile, the speculative
walk) and, in the same run, of the driver's one-thread-per-tile form ("kernels.simple": the literal loop, which stands for the code before this pass existed), and
of the same batch's terra_tiles_create_zvals_dev (zvals, stats and normals), the yardstick of the other passes.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls.  The two forms are timed
in --rounds alternating rounds; `spread` is the largest distance between two rounds' medians of the same form -- what a difference between the forms has to exceed.
Both forms' counts and aux words (and, on the small batch, records) are compared.  Prints one JSON line per batch.
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
    ap.add_argument("--sides", type=int, nargs="+", default=[3, 64], help="a batch is side x side tiles")
    ap.add_argument("--capacity", type=int, default=24576)
    ap.add_argument("--density", type=float, default=2.0)
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, a.capacity
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_flower_params(pkg.make_flower_params(flower_density=a.density))
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        bufs = [t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4), t.alloc(n * W * W * 4), t.alloc(n * W * W * 4),
                t.alloc(n * cap * 48), t.alloc(n * cap * 4), t.alloc(n * 4)]
        zb, st, nm, mnz, mw, w, fl, ax, cn = bufs
        out = {"tiles": n, "tile_size": S, "flower_density": a.density, "capacity": cap, "reps": a.reps, "rounds": a.rounds}
        out["create_zvals_us"] = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        t.tiles_create_weights_dev(tiles, zb.ptr, mw.ptr)
        t.tiles_tree_weights_dev(n, mw.ptr, None, w.ptr)
        place = lambda: t.tiles_place_flowers_dev(tiles, w.ptr, cap, fl.ptr, cn.ptr, ax.ptr)  # noqa: E731
        rounds = {"default": [], "simple": []}
        result = {}
        for _ in range(a.rounds):
            for form in ("default", "simple"):
                t.set_option("kernels.simple", "1" if form == "simple" else "0")
                try:
                    rounds[form].append(timed(t, a.reps, a.warmup, place))
                finally:
                    t.set_option("kernels.simple", "0")
                if form not in result:
                    result[form] = (cn.download(np.uint32, (n,)), ax.download(np.uint32, (n, cap)), fl.download(np.uint8, (n * cap * 48,)) if n <= 16 else None)
        (c0, a0, f0), (c1, a1, f1) = result["default"], result["simple"]
        assert (c0 == c1).all() and c0.max() <= cap, "the two forms disagree on the counts"
        for i in range(n):
            assert (a0[i, :c0[i]] == a1[i, :c0[i]]).all(), f"the two forms disagree on tile {i}'s aux words"
            assert f0 is None or f0[i * cap * 48:(i * cap + int(c0[i])) * 48].tobytes() == f1[i * cap * 48:(i * cap + int(c0[i])) * 48].tobytes(), f"the two forms disagree on tile {i}'s records"
        out["flowers"], out["max_flowers_per_tile"] = int(c0.sum()), int(c0.max())
        for form in ("default", "simple"):
            out[f"place_flowers_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        out["default_over_simple"] = round(out["place_flowers_default_us"]["median"] / out["place_flowers_simple_us"]["median"], 4)
        out["flowers_over_zvals"] = round(out["place_flowers_default_us"]["median"] / out["create_zvals_us"], 3)
        out["flowers_per_s"] = round(out["flowers"] / out["place_flowers_default_us"]["median"] * 1e6)
        print(json.dumps(out), flush=True)
        for b in bufs:
            b.free()
    t.close()


if __name__ == "__main__":
    main()
