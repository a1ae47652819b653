"""The reflection pass's terrain draw list (terra_tiles_reflection_view_dev) and the water quads and caps (terra_tiles_water_view_dev) on device-resident tile
batches at S = 128, on the batches and cameras of tools/bench_terrain_view.py: a 19 x 19 batch around the camera and the 64 x 64 batch, on the default generated
terrain, the camera 1.0 and 0.05 above the middle of the centre tile; a 60-degree, 16:9 view along the ground.  The yardstick is measured in the same run: the
pass-0 terra_tiles_terrain_view_dev on the same batch and camera, whose work the reflection call repeats before it adds the walks of can_have_reflection.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls, in --rounds rounds that
alternate the three calls; `spread` is the largest distance between two rounds' medians of one call -- what a difference has to exceed.  The driver's simple form
("kernels.simple": the reference's loop on one thread) is timed in the same run with --simple-reps calls, and both forms' outputs are compared.  Per batch and
camera one JSON line: the times, the ratio to the yardstick, the tiles that :2869 asked, how it answered, the tiles that walked and the number of distinct
|dx| + |dy| distances to the camera's tile among them (the levels a wavefront over the walks would have had).
(The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`, with --rounds 1.)"""
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
    ap.add_argument("--simple-reps", type=int, default=3)
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
    zmin, zmax = float(t.state().zmin), float(t.state().zmax)
    bsm = t.view_behind_sphere_mult(angle, aspect)
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        names = ("zb", "st", "nm", "mnz", "su", "di", "lod", "cr", "dr", "oc", "cn", "rf", "su0", "wl", "cm", "cnw")
        sizes = (n * Z * Z * 4, n * C.sizeof(pkg.TileStats), n * W * W * 4, n * 4, n, n * 4, n, n * 4, n * 4, n * 4, 8, n, n, n * 4, n, 8)
        b = {k: t.alloc(s) for k, s in zip(names, sizes)}
        t.tiles_create_zvals_dev(tiles, 0, b["zb"].ptr, b["st"].ptr, b["nm"].ptr, b["mnz"].ptr)
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(b["zb"].download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        a0, a1, aw = pkg.make_terrain_view_args(bsm, zmin, 1, 1, 0), pkg.make_reflection_view_args(bsm, zmin, zmax, 1, 1), pkg.make_water_view_args(bsm, 1)
        for camera, height in (("default", 1.0), ("low", 0.05)):
            view = t.make_view((0.0, 0.0, zc + height), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
            calls = {
                "terrain_view_pass0": lambda: t.tiles_terrain_view_dev(tiles, view, a0, b["st"].ptr, b["su0"].ptr, b["di"].ptr, b["lod"].ptr, b["cr"].ptr, b["dr"].ptr, b["oc"].ptr,
                                                                         b["cn"].ptr, min_normal_z_ptr=b["mnz"].ptr),
                "reflection_view": lambda: t.tiles_reflection_view_dev(tiles, view, a1, b["st"].ptr, b["su"].ptr, b["di"].ptr, b["lod"].ptr, b["cr"].ptr, b["dr"].ptr, b["oc"].ptr,
                                                                       b["cn"].ptr, min_normal_z_ptr=b["mnz"].ptr, reflect_ptr=b["rf"].ptr),
                "water_view": lambda: t.tiles_water_view_dev(tiles, view, aw, b["st"].ptr, b["wl"].ptr, b["cnw"].ptr, status_ptr=b["su0"].ptr, cap_mask_ptr=b["cm"].ptr),
            }
            out = {"tiles": n, "tile_size": S, "camera": camera, "camera_height": height, "reps": a.reps, "rounds": a.rounds, "simple_reps": a.simple_reps}
            rounds = {k: [] for k in calls}
            for _ in range(a.rounds):
                for k, fn in calls.items():
                    rounds[k].append(timed(t, a.reps, a.warmup, fn))

            def outputs():
                c, cw = b["cn"].download(np.uint32, (2,)).copy(), b["cnw"].download(np.uint32, (2,)).copy()
                return (c, b["su"].download(np.uint8, (n,)).copy(), b["lod"].download(np.uint8, (n,)).copy(), b["cr"].download(np.uint8, (n, 4)).copy(),
                        b["dr"].download(np.uint32, (n,))[:c[0]].copy(), b["oc"].download(np.uint32, (n,))[:c[1]].copy(), b["rf"].download(np.uint8, (n,)).copy(), cw,
                        b["wl"].download(np.uint32, (n,))[:cw[0]].copy(), b["cm"].download(np.uint8, (n,)).copy())
            calls["terrain_view_pass0"]()
            calls["water_view"]()
            calls["reflection_view"]()
            fast = outputs()
            simple = {}
            t.set_option("kernels.simple", "1")
            try:
                calls["terrain_view_pass0"]()
                for k in ("water_view", "reflection_view"):
                    simple[k] = timed(t, a.simple_reps, 1, calls[k])
                slow = outputs()
            finally:
                t.set_option("kernels.simple", "0")
            for x, y in zip(fast, slow):
                assert x.tobytes() == y.tobytes(), "the two forms disagree"
            status, reflect = fast[1], fast[6]
            low = status & 7
            walked = np.isin(reflect, (2, 4))
            level = np.abs(tiles[:, 0]) + np.abs(tiles[:, 1])  # the camera stands in tile (0, 0)
            out.update(asked=int((reflect != 0).sum()), all_water_or_disabled=int((reflect == 1).sum()), has_water=int((reflect == 3).sum()), walk_found=int((reflect == 4).sum()),
                       walk_nothing=int((reflect == 2).sum()), walk_levels=int(len(set(level[walked].tolist()))), dropped=int((low == 6).sum()), drawn=int(fast[0][0]),
                       occluded=int(fast[0][1]), occluders=int((status & 0x80 != 0).sum()), water_quads=int(fast[7][0]), capped_tiles=int(fast[7][1]))
            for k in calls:
                out[f"{k}_us"] = {"median": round(float(np.median(rounds[k])), 1), "rounds": rounds[k]}
            out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
            out["reflection_over_pass0"] = round(out["reflection_view_us"]["median"] / out["terrain_view_pass0_us"]["median"], 3)
            out["simple_us"] = simple
            print(json.dumps(out), flush=True)
        for x in b.values():
            x.free()
    t.close()


if __name__ == "__main__":
    main()
