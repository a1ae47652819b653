"""The tree brush (terra_tiles_edit_trees_dev) on a device-resident tile batch at S = 128 (64 x 64 = 4096 tiles by default) at the reference's default tree settings
with tree_mode 3 and num_trees 400, both placements resident: microseconds per call for three strokes -- a one-tile-wide round brush removing, the same brush adding,
and a square brush over the whole batch removing (the worst case: every tile does the full work) -- and the same three under "kernels.simple".  A stroke edits the
records in place, so before every repetition both placements run again and trmax is uploaded again, outside the timed span; every repetition is timed on its own with
device events on the context's stream, after a warm-up; the figure is the median.  Prints one JSON line.
The passes of the call (k_tree_edit, the two brush placements, k_tree_edit_append, k_tree_edit_finish): run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=64, help="the batch is side x side tiles")
    ap.add_argument("--stroke", default=None, help="one stroke alone (for a kernel trace): one_tile_round_remove | one_tile_round_add | whole_batch_square_remove")
    ap.add_argument("--simple-reps", type=int, default=3, help="repetitions under kernels.simple (0: skip)")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape())
    t.set_tree_params(pkg.make_tree_params(tree_mode=3))
    nshared = 100
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=nshared))
    tiles = np.array([(x, y) for y in range(-a.side // 2, a.side // 2) for x in range(-a.side // 2, a.side // 2)], np.int32)
    n, S, cap_p, cap_d, cap_l = len(tiles), 128, 512, 512, 2048
    W, Z = S + 1, S + 2
    by_id = np.linspace(0.05, 0.4, nshared).astype(np.float32)  # tdata().sphere_radius of the shared trees
    bufs = dict(z=t.alloc(n * Z * Z * 4), st=t.alloc(n * C.sizeof(pkg.TileStats)), pt=t.alloc(n * cap_p * pkg.TREE_PLACE_DTYPE.itemsize), pc=t.alloc(n * 4), dt=t.alloc(n * cap_d * pkg.DECID_PLACE_DTYPE.itemsize), dc=t.alloc(n * 4),
                id=t.alloc(by_id.nbytes).upload(by_id), tm=t.alloc(n * W * W * 2), trm=t.alloc(n * 4), status=t.alloc(n), changed=t.alloc(n), box=t.alloc(24))
    t.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)

    def restore():
        t.tiles_place_trees_dev(tiles, cap_p, bufs["pt"].ptr, bufs["pc"].ptr, 0, 0, None, bufs["st"].ptr)
        t.tiles_place_decid_trees_dev(tiles, cap_d, bufs["dt"].ptr, bufs["dc"].ptr, 0, 0, None, bufs["st"].ptr, bufs["z"].ptr)

    restore()
    t.tiles_tree_ao_shadows_dev(tiles, cap_l, bufs["tm"].ptr, bufs["pt"].ptr, bufs["pc"].ptr, cap_p, bufs["dt"].ptr, bufs["dc"].ptr, cap_d, None, bufs["id"].ptr, nshared,
                                None, None, bufs["trm"].ptr, None)
    trmax = bufs["trm"].download(np.float32, (n,))
    pc0, dc0 = bufs["pc"].download(np.uint32, (n,)), bufs["dc"].download(np.uint32, (n,))
    dx = 8.0 / S  # DX_VAL of make_config's scene (X_SCENE_SIZE = 4)
    tile = (1, 0)  # on the island's slope: both kinds of tree
    one = ((np.float32(-4.0 + dx * S * (tile[0] + 0.5)), np.float32(-4.0 + dx * S * (tile[1] + 0.5)), np.float32(0.0)), np.float32(0.5 * S * dx))
    whole = ((np.float32(-4.0), np.float32(-4.0), np.float32(0.0)), np.float32(0.75 * a.side * S * dx))  # (the culls are spheres: beyond the batch's corners)
    strokes = {"one_tile_round_remove": one + (False, False), "one_tile_round_add": one + (True, False), "whole_batch_square_remove": whole + (False, True)}

    if a.stroke:
        strokes = {a.stroke: strokes[a.stroke]}

    def stroke(pos, radius, add, square):
        t.tiles_edit_trees_dev(tiles, bufs["st"].ptr, pos, radius, add, square, bufs["trm"].ptr, bufs["status"].ptr, bufs["changed"].ptr, bufs["pt"].ptr, bufs["pc"].ptr, cap_p,
                               bufs["dt"].ptr, bufs["dc"].ptr, cap_d, None, bufs["id"].ptr, nshared, None, bufs["z"].ptr, None, bufs["box"].ptr)

    def timed(reps, warmup, args, simple=False):
        us = []
        for k in range(warmup + reps):
            restore()
            bufs["trm"].upload(trmax)
            if simple:  # (the stroke alone: the restoring placements keep their kernels)
                t.set_option("kernels.simple", "1")
            t.synchronize()
            t.timer_start()
            stroke(*args)
            ms = t.timer_stop()
            if simple:
                t.set_option("kernels.simple", "0")
            if k >= warmup:
                us.append(1000.0 * ms)
        return {"median": round(float(np.median(us)), 1), "min": round(float(min(us)), 1), "max": round(float(max(us)), 1)}

    out = {"tiles": n, "tile_size": S, "reps": a.reps, "pine_palm_trees": int(pc0.sum()), "decid_trees": int(dc0.sum()), "strokes_us": {}, "strokes_simple_us": {}, "effect": {}}
    for name, args in strokes.items():
        out["strokes_us"][name] = timed(a.reps, a.warmup, args)
        st = bufs["status"].download(np.uint8, (n,))
        pc, dc = bufs["pc"].download(np.uint32, (n,)), bufs["dc"].download(np.uint32, (n,))
        out["effect"][name] = {"status": [int((st == k).sum()) for k in range(3)], "changed": int(bufs["changed"].download(np.uint8, (n,)).sum()),
                               "pine_palm_delta": int(pc.astype(np.int64).sum() - pc0.astype(np.int64).sum()), "decid_delta": int(dc.astype(np.int64).sum() - dc0.astype(np.int64).sum())}
    if a.simple_reps:
        for name, args in strokes.items():
            out["strokes_simple_us"][name] = timed(a.simple_reps, 1, args, True)["median"]
    for b in bufs.values():
        b.free()
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
