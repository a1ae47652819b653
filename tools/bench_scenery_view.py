"""The scenery draw lists for a camera (terra_tiles_scenery_view_dev) on device-resident tile batches at S = 128, on the records the real placement leaves
(terra_tiles_place_scenery_dev behind terra_tiles_create_zvals_dev, at the default settings): the 64 x 64 batch and a 3 x 3 batch around the camera; the camera 1.0
above the middle of the centre tile, a 60-degree, 16:9 view along the ground, every tile unskipped, both sweeps in one call.  Per batch: microseconds per call of
k_scenery_view and, in the same run, of the driver's one-thread-per-tile form ("kernels.simple": the literal loops), and of the same batch's
terra_tiles_create_zvals_dev (zvals, stats and normals), the yardstick of the other passes; the numbers of records, of drawn tiles and of list entries.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls.  The two forms are timed
in --rounds alternating rounds; `spread` is the largest distance between two rounds' medians of the same form -- what a difference between the forms has to exceed.
Both forms' outputs are compared.  Prints one JSON line per batch.
(The kernel's own time: run this under `rocprofv3 --kernel-trace --stats`.)"""
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
    ap.add_argument("--capacity", type=int, default=128)
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, a.capacity
    lcap = 3 * cap
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(vegetation=1.0))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3))
    t.set_scenery_params(pkg.make_scenery_params(2))
    angle, aspect = 0.5236, 16.0 / 9.0
    args = pkg.make_scenery_view_args(t.view_behind_sphere_mult(angle, aspect), 1.0, 0.0, 1920)
    names = pkg.Terra.SCENERY_VIEW_OUTPUTS
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        shapes = pkg.Terra._scenery_view_outputs(n, cap, lcap)
        outs = {k: t.alloc(max(x.nbytes, 4)) for k, x in shapes.items()}
        zb, st, nm, mnz, ob, pc = (t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4),
                                   t.alloc(n * cap * pkg.SCENERY_PLACE_DTYPE.itemsize), t.alloc(n * 4))
        zvals_us = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(zb.download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        view = t.make_view((0.0, 0.0, zc + 1.0), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
        t.tiles_place_scenery_dev(tiles, cap, ob.ptr, pc.ptr)
        counts = pc.download(np.uint32, (n,)).copy()
        o = [outs[k].ptr for k in names]
        call = lambda: t.tiles_scenery_view_dev(tiles, view, args, st.ptr, ob.ptr, pc.ptr, cap, *o[:5], lcap, o[5])  # noqa: E731
        out = {"tiles": n, "tile_size": S, "capacity": cap, "list_capacity": lcap, "reps": a.reps, "rounds": a.rounds, "create_zvals_us": zvals_us,
               "records": int(np.minimum(counts, cap).sum()), "max_records_per_tile": int(counts.max())}
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
                    result[form] = {k: outs[k].download(np.uint8, (shapes[k].nbytes,)).copy().view(shapes[k].dtype).reshape(shapes[k].shape) for k in names}
        d, s = result["default"], result["simple"]
        for k in ("tile", "group_counts"):
            assert d[k].tobytes() == s[k].tobytes(), f"the two forms disagree on {k}"
        for i in range(n):  # of every tile only what its record names
            m, lw = int(d["tile"][i]["num_records"]), int(d["tile"][i]["list_written"])
            ok = d["list"][i, :lw].tobytes() == s["list"][i, :lw].tobytes()
            for k in ("draw", "size_scale", "dist"):
                ok = ok and d[k][i, :m].tobytes() == s[k][i, :m].tobytes()
            assert ok, f"the two forms disagree on tile {i}"
        out["drawn_tiles"], out["records_in_drawn_tiles"] = int((d["tile"]["flags"] & 1).sum()), int(d["tile"]["num_records"].sum())
        out["list_entries"] = int(d["group_counts"].sum())
        out["group_counts"] = dict(zip(pkg.SCV_GROUPS, d["group_counts"].sum(axis=0).tolist()))
        for form in ("default", "simple"):
            out[f"scenery_view_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        out["default_over_simple"] = round(out["scenery_view_default_us"]["median"] / out["scenery_view_simple_us"]["median"], 4)
        out["view_over_zvals"] = round(out["scenery_view_default_us"]["median"] / zvals_us, 3)
        print(json.dumps(out), flush=True)
        for b in list(outs.values()) + [zb, st, nm, mnz, ob, pc]:
            b.free()
    t.close()


if __name__ == "__main__":
    main()
