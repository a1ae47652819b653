"""The deciduous tree draw lists for a camera (terra_tiles_decid_view_dev) on device-resident tile batches at S = 128, on the records the real placement leaves
(terra_tiles_place_decid_trees_dev behind terra_tiles_create_zvals_dev, at num_trees 400 with 100 shared trees): the 64 x 64 batch and a 3 x 3 batch around the
camera; the camera 1.0 above the middle of the centre tile, a 60-degree, 16:9 view along the ground, every tile unskipped, leaves and branches in one call, billboards
on with tree_lod_scales 0.24 0.2 0.24 0.2, the not_visible array given.  Per batch: microseconds per call of k_decid_view and, in the same run, of the driver's
one-thread-per-tile form ("kernels.simple": the literal loops), and of the same batch's terra_tiles_create_zvals_dev (zvals, stats and normals), the yardstick of the
other passes; the numbers of records, of drawn and sorted tiles and of list entries.

The table is made here, since gen_tree is the engine's: entry i is a tree of TREE_SIZE's order scaled by s in [0.6, 1.4] from a fixed generator -- base_radius 0.005 s,
sphere_radius 0.06 s, its centre 0.08 s above the ground, boxes of +-0.06 s (leaves) and +-0.04 s (branches), 2000 to 6000 leaves, 300 to 900 branch quads, every
third entry with fourth-order branches, all generated with both billboard textures.

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


def tree_table(pkg, count):
    rng = np.random.default_rng(1)
    d = np.zeros(count, pkg.DECID_TREE_DATA_DTYPE)
    for i in range(count):
        s = float(rng.uniform(0.6, 1.4))
        d[i] = (0.005 * s, 0.06 * s, 0.08 * s, 0.09 * s, tuple(s * x for x in (-0.06, 0.06, -0.06, 0.06, 0.03, 0.16)), tuple(s * x for x in (-0.04, 0.04, -0.04, 0.04, 0.0, 0.14)),
                int(rng.integers(2000, 6000)), int(rng.integers(300, 900)), pkg.DCV_GENERATED | pkg.DCV_LEAF_TEX | pkg.DCV_BRANCH_TEX | (pkg.DCV_HAS_4TH if i % 3 == 0 else 0), 0)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[3, 64], help="a batch is side x side tiles")
    ap.add_argument("--capacity", type=int, default=512)
    ap.add_argument("--num-trees", type=int, default=400)
    ap.add_argument("--shared", type=int, default=100)
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, a.capacity
    W, Z = S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3))
    t.set_decid_params(pkg.make_decid_params(num_trees=a.num_trees, num_shared_trees=a.shared))
    angle, aspect = 0.5236, 16.0 / 9.0
    args = pkg.make_decid_view_args(t.view_behind_sphere_mult(angle, aspect), 1.0, (0.24, 0.2, 0.24, 0.2))
    names = pkg.Terra.DECID_VIEW_OUTPUTS
    table = tree_table(pkg, a.shared)
    td = t.alloc(table.nbytes).upload(table.view(np.uint8))
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        shapes = pkg.Terra._decid_view_outputs(n, cap)
        outs = {k: t.alloc(max(x.nbytes, 4)) for k, x in shapes.items()}
        zb, st, nm, mnz, de, pc, nv = (t.alloc(n * Z * Z * 4), t.alloc(n * C.sizeof(pkg.TileStats)), t.alloc(n * W * W * 4), t.alloc(n * 4),
                                       t.alloc(n * cap * pkg.DECID_PLACE_DTYPE.itemsize), t.alloc(n * 4), t.alloc(n * cap))
        zvals_us = timed(t, a.reps, a.warmup, lambda: t.tiles_create_zvals_dev(tiles, 0, zb.ptr, st.ptr, nm.ptr, mnz.ptr))
        centre = int(np.argwhere((tiles == (0, 0)).all(axis=1))[0, 0])
        zc = float(zb.download(np.float32, (n, Z, Z))[centre, S // 2, S // 2])
        view = t.make_view((0.0, 0.0, zc + 1.0), (1.0, 0.3, -0.05), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
        t.tiles_place_decid_trees_dev(tiles, cap, de.ptr, pc.ptr, 0, 0, None, st.ptr, zb.ptr)
        counts = pc.download(np.uint32, (n,)).copy()
        o = [outs[k].ptr for k in names]
        call = lambda: t.tiles_decid_view_dev(tiles, view, args, td.ptr, a.shared, de.ptr, pc.ptr, cap, o, not_visible_ptr=nv.ptr)  # noqa: E731
        out = {"tiles": n, "tile_size": S, "capacity": cap, "num_trees": a.num_trees, "shared_trees": a.shared, "reps": a.reps, "rounds": a.rounds, "create_zvals_us": zvals_us,
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
                    result[form]["nv"] = nv.download(np.uint8, (n * cap,)).copy().reshape(n, cap)
        d, s = result["default"], result["simple"]
        for k in ("tile", "list_counts"):
            assert d[k].tobytes() == s[k].tobytes(), f"the two forms disagree on {k}"
        assert (d["all_bcube"] == s["all_bcube"]).all(), "the two forms disagree on all_bcube"
        for i in np.nonzero(d["tile"]["flags"] & pkg.DCV_TILE_DRAWN)[0]:  # of every drawn tile only what the counts name
            m = int(min(counts[i], cap))
            ok = all(d[k][i, :m].tobytes() == s[k][i, :m].tobytes() for k in names[2:10] + ("nv",))
            for j, k in enumerate(names[10:14]):
                c = int(d["list_counts"][i, j])
                ok = ok and d[k][i, :c].tobytes() == s[k][i, :c].tobytes()
            assert ok, f"the two forms disagree on tile {i}"
        fl = d["tile"]["flags"]
        out["drawn_tiles"], out["sorted_tiles"] = int((fl & pkg.DCV_TILE_DRAWN != 0).sum()), int((fl & pkg.DCV_TILE_SORTED != 0).sum())
        out["trees_in_drawn_tiles"] = int(d["tile"]["num_trees"][fl & pkg.DCV_TILE_DRAWN != 0].sum())
        out["list_entries"] = dict(zip(names[10:14], d["list_counts"].sum(axis=0).tolist()))
        for form in ("default", "simple"):
            out[f"decid_view_{form}_us"] = {"median": round(float(np.median(rounds[form])), 1), "rounds": rounds[form]}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        out["default_over_simple"] = round(out["decid_view_default_us"]["median"] / out["decid_view_simple_us"]["median"], 4)
        out["view_over_zvals"] = round(out["decid_view_default_us"]["median"] / zvals_us, 3)
        print(json.dumps(out), flush=True)
        for b in list(outs.values()) + [zb, st, nm, mnz, de, pc, nv]:
            b.free()
    td.free()
    t.close()


if __name__ == "__main__":
    main()
