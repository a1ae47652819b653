"""Sphere queries against the resident containers of a device-resident tile batch at S = 128: one terra_tiles_sphere_collide_dev call on a 3 x 3 and on the 64 x 64
batch whose three containers are the real placements at the documented defaults (tree_mode 3, num_trees 400 over 16 shared trees, vegetation 1), with two query
loads: 1 query (the player, beside a placed tree of the middle tile) and 16 queries per tile (the animals and the physics objects), drawn around record positions --
a query stands --offset from a record of its tile with a radius of --radius, so that a stated share of them hits; and one terra_tiles_cube_int_trees_dev call with
16 small cubes per tile, half of them over a deciduous tree.  The kernel form (k_sphere_collide, a wave per
query) and the driver's simple form ("kernels.simple": a logical thread per query, the reference's loops) are measured in the same run.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls, in --rounds rounds that
alternate the two forms; `spread` is the largest distance between two rounds' medians of one load and form -- what a difference has to exceed.  Both forms' outputs
are compared.  Per batch one JSON line: the times, the records, the share of the queries that hit and the mean number of objects that moved a centre.
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
    ap.add_argument("--per-tile", type=int, default=16)
    ap.add_argument("--offset", type=float, default=0.03, help="how far a query stands from its record, in x and y")
    ap.add_argument("--radius", type=float, default=0.06)
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, pcap, dcap, scap, shared = 128, 320, 384, 160, 16
    Z = S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1, vegetation=1.0))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=shared))
    t.set_scenery_params(pkg.make_scenery_params(1))
    t.set_tree_size_params(pkg.make_tree_size_params())
    # a shared-tree table of TREE_SIZE's order (the engine's comes from its tree generator)
    rng = np.random.default_rng(5)
    data = np.zeros(shared, pkg.DECID_TREE_DATA_DTYPE)
    for i in range(shared):
        s = 0.2 * float(rng.uniform(0.7, 1.4))
        data[i] = (0.02 * s, 0.3 * s, 0.375 * s, 0.4 * s, tuple(s * x for x in (-0.3, 0.3, -0.3, 0.3, 0.125, 0.75)), tuple(s * x for x in (-0.2, 0.2, -0.2, 0.2, 0.0, 0.625)), 1000, 400,
                   pkg.DCV_GENERATED, 0)
    br_scale = np.ones(shared, f32)
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * pcap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4, de=n * dcap * pkg.DECID_PLACE_DTYPE.itemsize, dc=n * 4,
                     ob=n * scap * pkg.SCENERY_PLACE_DTYPE.itemsize, oc=n * 4)
        b = {k: t.alloc(s) for k, s in sizes.items()}
        b["td"], b["br"] = t.alloc(data.nbytes).upload(data.view(np.uint8)), t.alloc(br_scale.nbytes).upload(br_scale)
        p = {k: x.ptr for k, x in b.items()}
        for k in ("pt", "de", "ob"):
            b[k].upload(np.zeros(sizes[k], np.uint8))
        t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        t.tiles_place_trees_dev(tiles, pcap, p["pt"], p["pc"], 0, 0, None, p["st"])
        t.tiles_place_decid_trees_dev(tiles, dcap, p["de"], p["dc"], 0, 0, None, p["st"], p["z"])
        t.tiles_place_scenery_dev(tiles, scap, p["ob"], p["oc"])
        stats = (pkg.TileStats * n).from_buffer_copy(b["st"].download(np.uint8, (sizes["st"],)).tobytes())
        recs = [b[k].download(np.uint8, (sizes[k],)).copy().view(d).reshape(n, c) for k, d, c in (("pt", pkg.TREE_PLACE_DTYPE, pcap), ("de", pkg.DECID_PLACE_DTYPE, dcap),
                                                                                               ("ob", pkg.SCENERY_PLACE_DTYPE, scap))]
        counts = [np.minimum(b[k].download(np.uint32, (n,)).copy(), c) for k, c in (("pc", pcap), ("dc", dcap), ("oc", scap))]
        tile_zmax = np.array([float(stats[i].mzmax) + 1.0 for i in range(n)], f32)  # get_tile_zmax(): above every tree
        b["zm"] = t.alloc(tile_zmax.nbytes).upload(tile_zmax)
        cin = pkg.make_collide_in(stats=p["st"], tile_zmax=b["zm"].ptr, pine=p["pt"], pine_counts=p["pc"], decid=p["de"], decid_counts=p["dc"], scenery=p["ob"], scenery_counts=p["oc"],
                                  tree_data=b["td"].ptr, br_scale=b["br"].ptr, pine_capacity=pcap, decid_capacity=dcap, scenery_capacity=scap, num_tree_data=shared)

        def around(i, which, j):
            x, y, z = (float(v) for v in recs[which][i, j]["pos"])
            return ((x + float(rng.choice((-1.0, 1.0))) * a.offset, y + float(rng.uniform(-a.offset, a.offset)), z + float(rng.uniform(0.0, 0.05))), a.radius, -1, pkg.COLL_INC_ALL)
        many = []
        for i in range(n):
            total = [int(c[i]) for c in counts]
            for k in range(a.per_tile if sum(total) else 0):
                which = int(rng.choice(3, p=np.array(total) / sum(total)))
                many.append(around(i, which, int(rng.integers(total[which]))))
        # the player: the first of the middle tile's queries that meets something (asked once, outside the timing)
        mid = n // 2
        cand = np.zeros(a.per_tile, pkg.SPHERE_QUERY_DTYPE)
        first = sum(a.per_tile for i in range(mid) if sum(int(c[i]) for c in counts))
        for i in range(a.per_tile):
            cand[i] = many[first + i] if first + a.per_tile <= len(many) else ((0.0, 0.0, 0.0), a.radius, -1, pkg.COLL_INC_ALL)
        qb, hb = t.alloc(cand.nbytes).upload(cand.view(np.uint8).reshape(-1)), t.alloc(cand.nbytes)
        t.tiles_sphere_collide_dev(tiles, cin, qb.ptr, len(cand), hb.ptr)
        met = np.flatnonzero(hb.download(np.uint8, (cand.nbytes,)).copy().view(pkg.SPHERE_HIT_DTYPE)["nhits"])
        one = [tuple(cand[int(met[0]) if len(met) else 0].tolist())]
        qb.free()
        hb.free()
        loads, out_of = {}, {}
        for name, rows in (("player", one), ("per_tile", many)):
            q = np.zeros(len(rows), pkg.SPHERE_QUERY_DTYPE)
            for i, row in enumerate(rows):
                q[i] = row
            qb, hb = t.alloc(max(q.nbytes, 4)).upload(q.view(np.uint8).reshape(-1)), t.alloc(max(q.nbytes, 4))
            loads[name] = (len(q), qb, hb)
        rounds = {(k, form): [] for k in loads for form in ("kernels", "simple")}
        for _ in range(a.rounds):
            for form in ("kernels", "simple"):
                t.set_option("kernels.simple", "1" if form == "simple" else "0")
                try:
                    for k, (nq, qb, hb) in loads.items():
                        rounds[(k, form)].append(timed(t, a.reps, a.warmup, lambda: t.tiles_sphere_collide_dev(tiles, cin, qb.ptr, nq, hb.ptr)))
                        out_of[(k, form)] = hb.download(np.uint8, (nq * 24,)).copy()
                finally:
                    t.set_option("kernels.simple", "0")
        out = {"tiles": n, "tile_size": S, "reps": a.reps, "rounds": a.rounds, "records": [int(c.sum()) for c in counts], "max_records_in_tile": [int(c.max()) for c in counts],
               "offset": a.offset, "radius": a.radius}
        for k, (nq, qb, hb) in loads.items():
            assert out_of[(k, "kernels")].tobytes() == out_of[(k, "simple")].tobytes(), "the two forms disagree"
            h = out_of[(k, "kernels")].view(pkg.SPHERE_HIT_DTYPE)
            out[k] = {"queries": nq, "tested": int(((h["word"] & pkg.COLL_STAGE_MASK) == 0).sum()), "hit_share": round(float((h["nhits"] > 0).mean()), 3),
                      "mean_nhits": round(float(h["nhits"].mean()), 3), "max_nhits": int(h["nhits"].max())}
            for form in ("kernels", "simple"):
                r = rounds[(k, form)]
                out[k][f"{form}_us"] = {"median": round(float(np.median(r)), 1), "rounds": r}
            qb.free()
            hb.free()
        # the cube call: --per-tile cubes a tile (balconies), half of them over a deciduous tree, half a tree's width beside one
        cubes = []
        for i in range(n):
            for k in range(a.per_tile if counts[1][i] else 0):
                x, y, z = (float(v) for v in recs[1][i, int(rng.integers(counts[1][i]))]["pos"])
                x += 0.0 if k % 2 else 0.3
                cubes.append((x - 0.02, x + 0.02, y - 0.02, y + 0.02, z + 0.02, z + 0.06))
        cubes = np.array(cubes, f32).reshape(-1, 6)
        nc = len(cubes)
        cb, rb = t.alloc(max(cubes.nbytes, 4)).upload(cubes.view(np.uint8).reshape(-1)), t.alloc(max(nc, 4))
        crounds, cres = {"kernels": [], "simple": []}, {}
        for _ in range(a.rounds if nc else 0):
            for form in ("kernels", "simple"):
                t.set_option("kernels.simple", "1" if form == "simple" else "0")
                try:
                    crounds[form].append(timed(t, a.reps, a.warmup, lambda: t.tiles_cube_int_trees_dev(tiles, cin, cb.ptr, nc, rb.ptr)))
                    cres[form] = rb.download(np.uint8, (nc,)).copy()
                finally:
                    t.set_option("kernels.simple", "0")
        if nc:
            assert cres["kernels"].tobytes() == cres["simple"].tobytes(), "the two forms of the cube call disagree"
            out["cubes"] = {"queries": nc, "hit_share": round(float((cres["kernels"] & pkg.CUBE_INT_HIT).astype(bool).mean()), 3)}
            for form, r in crounds.items():
                out["cubes"][f"{form}_us"] = {"median": round(float(np.median(r)), 1), "rounds": r}
        cb.free()
        rb.free()
        out["spread_us"] = round(max(max(r) - min(r) for r in list(rounds.values()) + [r for r in crounds.values() if r]), 1)
        print(json.dumps(out), flush=True)
        for x in b.values():
            x.free()
    t.close()


if __name__ == "__main__":
    main()
