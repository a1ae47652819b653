"""The pine and palm tree draw lists for a camera (terra_tiles_tree_view_dev) on device-resident tile batches at S = 128, on the records the real placement leaves
(terra_tiles_place_trees_dev behind terra_tiles_create_zvals_dev): the 64 x 64 batch and a 3 x 3 batch around the camera, at the default settings and in an
instanced setting (`instanced` with 50 + 50 instances); the camera 1.0 above the middle of the centre tile, a 60-degree, 16:9 view along the ground, every tile
unskipped, all three sweeps in one call.  Per batch and setting: microseconds per call of k_tree_view and, in the same run, of the driver's one-thread-per-tile form
("kernels.simple": the literal loops), and of the same batch's terra_tiles_create_zvals_dev (zvals, stats and normals), the yardstick of the other passes; the
numbers of records and of list entries.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls.  The two forms are timed
in --rounds alternating rounds; `spread` is the largest distance between two rounds' medians of the same form -- what a difference between the forms has to exceed.
Both forms' outputs are compared.  Prints one JSON line per batch and setting.
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


def instance_table(pkg, npine, npalm):
    """tree_instances as create_pine_tree_instances would leave it, with a plain generator: every tenth pine a short one"""
    rng = np.random.default_rng(1)
    v = np.zeros(npine + npalm, pkg.TREE_INST_DTYPE)
    for i in range(npine + npalm):
        h = float(rng.uniform(0.4, 1.0))
        v[i] = ((5 if i % 10 == 3 else 0) if i < npine else 4, h * (1.2 if i < npine else 2.0), h * float(rng.uniform(0.25, 0.35)))
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[3, 64], help="a batch is side x side tiles")
    ap.add_argument("--capacity", type=int, default=512)
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, a.capacity
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_size_params(pkg.make_tree_size_params())
    angle, aspect = 0.5236, 16.0 / 9.0
    args = pkg.make_tree_view_args(t.view_behind_sphere_mult(angle, aspect), 1.0, 1.0, 1920, 0, 1, 1, 1)
    names = pkg.Terra.TREE_VIEW_OUTPUTS
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        shapes = pkg.Terra._tree_view_outputs(n, cap)
        outs = {k: t.alloc(max(x.nbytes, 4)) for k, x in shapes.items()}
        zb, st, nm, mnz, pt, pc = (t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4),
                                   t.alloc(n * cap * pkg.TREE_PLACE_DTYPE.itemsize), t.alloc(n * 4))
        zvals_us = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(zb.download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        view = t.make_view((0.0, 0.0, zc + 1.0), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
        for setting, instanced in (("default", 0), ("instanced", 1)):
            t.set_tree_params(pkg.make_tree_params(tree_mode=3, instanced=instanced, num_pine_insts=50 * instanced, num_palm_insts=50 * instanced))
            t.set_tree_instances(instance_table(pkg, 50, 50) if instanced else np.zeros(0, pkg.TREE_INST_DTYPE))
            t.tiles_place_trees_dev(tiles, cap, pt.ptr, pc.ptr, 0, 0, None, st.ptr)
            counts = pc.download(np.uint32, (n,)).copy()
            call = lambda: t.tiles_tree_view_dev(tiles, view, args, st.ptr, pt.ptr, pc.ptr, cap, *[outs[k].ptr for k in names])  # noqa: E731
            out = {"tiles": n, "tile_size": S, "setting": setting, "capacity": cap, "reps": a.reps, "rounds": a.rounds, "create_zvals_us": zvals_us,
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
            for k in ("tile", "inst_counts", "leaf_counts"):
                assert d[k].tobytes() == s[k].tobytes(), f"the two forms disagree on {k}"
            assert (d["all_bcube"] == s["all_bcube"]).all(), "the two forms disagree on all_bcube"
            for i in range(n):  # of every tile only what the counts name
                m, lw = int(min(counts[i], cap)), int(d["tile"][i]["leaf_written"])
                ok = d["leaf_list"][i, :lw].tobytes() == s["leaf_list"][i, :lw].tobytes() and (d["tile"][i]["num_trees"] == 0 or d["trunk"][i, :m].tobytes() == s["trunk"][i, :m].tobytes())
                for j, k in enumerate(("pine_insts", "palm_insts")):
                    c = int(d["inst_counts"][i, j])
                    ok = ok and d[k][i, :c].tobytes() == s[k][i, :c].tobytes()
                assert ok, f"the two forms disagree on tile {i}"
            fl = d["tile"]["flags"]
            out["pine_insts"], out["palm_insts"] = int(d["inst_counts"][:, 0].sum()), int(d["inst_counts"][:, 1].sum())
            out["leaf_entries"], out["polygon_trunk_tiles"], out["near_leaf_tiles"] = int(d["tile"]["leaf_written"].sum()), int(((fl & 3) == 1).sum() + ((fl & 3) == 2).sum()), int((fl & 4 != 0).sum())
            for form in ("default", "simple"):
                out[f"tree_view_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
            out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
            out["default_over_simple"] = round(out["tree_view_default_us"]["median"] / out["tree_view_simple_us"]["median"], 4)
            out["view_over_zvals"] = round(out["tree_view_default_us"]["median"] / zvals_us, 3)
            print(json.dumps(out), flush=True)
        for b in list(outs.values()) + [zb, st, nm, mnz, pt, pc]:
            b.free()
    t.close()


if __name__ == "__main__":
    main()
