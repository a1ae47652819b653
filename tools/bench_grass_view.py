"""The grass draw lists for a camera (terra_tiles_grass_view_dev) on device-resident tile batches at S = 128, on the zvals, stats and grass blocks the resident chain
leaves (terra_tiles_create_zvals_dev -> terra_tiles_create_weights_dev): the 3 x 3 batch around the camera and a 64 x 64 batch with the camera over its centre, at
the reference's tt_grass_scale_factor 1 and a 60-degree, 16:9 view along the ground from 0.3 above the centre tile's middle.  Per batch: microseconds per call of
k_grass_view (a workgroup per tile) and, in the same run, of the driver's one-thread-per-tile form ("kernels.simple": the literal loops), and of the same batch's
terra_tiles_create_zvals_dev (zvals, stats and normals), the yardstick of the other passes; the instances produced and the share of tiles that leave at the tile test.

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
    ap.add_argument("--scale", type=float, default=1.0, help="tt_grass_scale_factor")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, nrnd, cap = 128, 16, 1024
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1, num_rnd_grass_blocks=nrnd))
    t.set_grass_view_params(pkg.make_grass_view_params(a.scale))
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        bufs = [t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4), t.alloc(n * W * W * 4), t.alloc(n * 32 * 32 * 12),
                t.alloc(n * cap * 8), t.alloc(n * cap * 4), t.alloc(n * 6 * nrnd * 4), t.alloc(n * 4), t.alloc(n)]
        zb, st, nm, mnz, mw, gb, ins, ax, gc, cn, ps = bufs
        out = {"tiles": n, "tile_size": S, "tt_grass_scale_factor": a.scale, "capacity": cap, "reps": a.reps, "rounds": a.rounds}
        out["create_zvals_us"] = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        t.tiles_create_weights_dev(tiles, zb.ptr, mw.ptr, gb.ptr)
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(zb.download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        view = t.make_view((0.0, 0.0, zc + 0.3), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), 0.5236, 16.0 / 9.0, 0.01, 1000.0)
        call = lambda: t.tiles_grass_view_dev(tiles, zb.ptr, st.ptr, gb.ptr, view, cap, ins.ptr, gc.ptr, cn.ptr, ax.ptr, ps.ptr)  # noqa: E731
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
                    result[form] = (cn.download(np.uint32, (n,)).copy(), gc.download(np.uint32, (n, 6, nrnd)).copy(), ps.download(np.uint8, (n,)).copy(),
                                    ax.download(np.uint32, (n, cap)).copy(), ins.download(np.float32, (n, cap, 2)).copy())
        (c0, g0, p0, a0, i0), (c1, g1, p1, a1, i1) = result["default"], result["simple"]
        assert (c0 == c1).all() and (g0 == g1).all() and (p0 == p1).all() and c0.max() <= cap, "the two forms disagree on the counts"
        for i in range(n):
            assert (a0[i, :c0[i]] == a1[i, :c0[i]]).all() and i0[i, :c0[i]].tobytes() == i1[i, :c0[i]].tobytes(), f"the two forms disagree on tile {i}'s instances"
        out["instances"], out["max_instances_per_tile"], out["tiles_drawn"] = int(c0.sum()), int(c0.max()), int((p0 != 255).sum())
        out["tiles_leaving_at_tile_test"] = round(float((p0 == 255).mean()), 4)
        for form in ("default", "simple"):
            out[f"grass_view_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        out["default_over_simple"] = round(out["grass_view_default_us"]["median"] / out["grass_view_simple_us"]["median"], 4)
        out["view_over_zvals"] = round(out["grass_view_default_us"]["median"] / out["create_zvals_us"], 3)
        print(json.dumps(out), flush=True)
        for b in bufs:
            b.free()
    t.close()


if __name__ == "__main__":
    main()
