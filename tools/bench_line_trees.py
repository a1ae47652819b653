"""Line queries with inc_trees = 1 (terra_tiles_line_intersect_trees_dev) against a device-resident tile batch at S = 128 over the real pine / palm placement
(tree_mode 3 at the documented defaults): a 3 x 3 and the 64 x 64 batch, 1 line and 256 lines.  Half of the lines are aimed at placed pines (level shots of
--length through a point of the tree between its trunk's foot and its top), the other half are camera rays into the terrain.  Beside each load, in the same run:
the driver's simple form ("kernels.simple": a logical thread per tile for the boxes, then one per line, the reference's loops), terra_tiles_line_intersect_dev on
the same lines -- the difference is what the trees add -- and zvals + stats + normals of the batch.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls, in --rounds rounds that
alternate the forms; `spread` is the largest distance between two rounds' medians of one load and form -- what a difference has to exceed.  Both forms' records are
compared byte for byte.  Per batch one JSON line.  (The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`, with --rounds 1.)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
f32 = np.float32


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
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--length", type=float, default=12.0, help="the length of a shot at a tree")
    ap.add_argument("--no-simple", action="store_true")
    a = ap.parse_args()
    import line_intersect_cases as lic
    import line_intersect_model as lim
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, 320
    Z, W = S + 2, S + 1
    cfg = pkg.make_config(mesh_gen_mode=0)
    sc = lim.Scene.of(cfg, t.init_scene(cfg))
    t.set_landscape(pkg.make_landscape(grass_density=1, vegetation=1.0))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_tree_size_params(pkg.make_tree_size_params())
    rng = np.random.default_rng(7)
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), nm=n * W * W * 4, mz=n * 4, pt=n * cap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4)
        b = {k: t.alloc(s) for k, s in sizes.items()}
        p = {k: x.ptr for k, x in b.items()}
        b["pt"].upload(np.zeros(sizes["pt"], np.uint8))
        out = {"tiles": n, "tile_size": S, "reps": a.reps, "rounds": a.rounds}
        out["create_zvals_us"] = timed(t, max(3, a.reps // 8), 1, lambda: t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"], p["nm"], p["mz"]))
        t.tiles_place_trees_dev(tiles, cap, p["pt"], p["pc"], 0, 0, None, p["st"])
        pine = b["pt"].download(np.uint8, (sizes["pt"],)).copy().view(pkg.TREE_PLACE_DTYPE).reshape(n, cap)
        pc = np.minimum(b["pc"].download(np.uint32, (n,)).copy(), cap)
        z = b["z"].download(f32, (n, Z, Z)).copy()
        pines = [(i, j) for i in range(n) for j in range(int(pc[i])) if pine[i, j]["type"] in (0, 5) and pine[i, j]["inst"] < 0]
        out["records"], out["max_records_in_tile"], out["pines"] = int(pc.sum()), int(pc.max()), len(pines)
        shots = []
        for k in rng.choice(len(pines), a.lines // 2, replace=len(pines) < a.lines // 2):
            r = pine[pines[int(k)]]
            yaw, pitch = rng.uniform(0, 2 * np.pi), rng.uniform(-0.05, 0.05)
            d = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])
            tgt = np.array(r["pos"], np.float64) + [0.0, 0.0, float(r["height"]) * rng.uniform(0.1, 1.0)]
            shots.append([tgt - d * a.length * rng.uniform(0.2, 0.8), tgt + d * a.length * 0.2])
        rays = lic.camera_rays(sc, tiles, z, np.random.RandomState(1), a.lines - len(shots))
        lines = np.empty((a.lines, 2, 3), f32)
        lines[0::2], lines[1::2] = np.array(shots, f32), rays  # line 0 is a shot at a tree
        lb, hb, mb = t.alloc(lines.nbytes).upload(lines.view(np.uint8).reshape(-1)), t.alloc(a.lines * 40), t.alloc(a.lines * 32)
        lin = pkg.make_line_trees_in(zvals=p["z"], stats=p["st"], pine=p["pt"], pine_counts=p["pc"], pine_capacity=cap)
        forms = ("kernels",) if a.no_simple else ("kernels", "simple")
        rounds = {(nl, f): [] for nl in (1, a.lines) for f in forms + ("mesh_only",)}
        recs = {}
        for _ in range(a.rounds):
            for form in forms:
                t.set_option("kernels.simple", "1" if form == "simple" else "0")
                try:
                    for nl in (1, a.lines):
                        rounds[(nl, form)].append(timed(t, a.reps, a.warmup, lambda: t.tiles_line_intersect_trees_dev(tiles, lin, lb.ptr, nl, hb.ptr)))
                        recs[(nl, form)] = hb.download(np.uint8, (nl * 40,)).copy()
                finally:
                    t.set_option("kernels.simple", "0")
            for nl in (1, a.lines):
                rounds[(nl, "mesh_only")].append(timed(t, a.reps, a.warmup, lambda: t.tiles_line_intersect_dev(tiles, p["z"], p["st"], lb.ptr, nl, mb.ptr)))
        for nl in (1, a.lines):
            if "simple" in forms:
                assert recs[(nl, "kernels")].tobytes() == recs[(nl, "simple")].tobytes(), "the two forms disagree"
            h = recs[(nl, "kernels")].view(pkg.LINE_TREE_HIT_DTYPE)
            out[str(nl)] = {"tree_hits": int((h["hit"] == pkg.LINE_HIT_TREE).sum()), "mesh_hits": int((h["hit"] == pkg.LINE_HIT_MESH).sum())}
            for f in forms + ("mesh_only",):
                r = rounds[(nl, f)]
                out[str(nl)][f"{f}_us"] = {"median": round(float(np.median(r)), 1), "rounds": r}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        print(json.dumps(out), flush=True)
        for x in list(b.values()) + [lb, hb, mb]:
            x.free()
    t.close()


if __name__ == "__main__":
    main()
