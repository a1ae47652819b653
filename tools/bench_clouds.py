"""The clouds of a device-resident tile batch at S = 128: one terra_tiles_update_clouds_dev call (a frame of the default wind (0.4, 0.2, 0) at fticks 1) and one
terra_tiles_cloud_view_dev call, on a 3 x 3 and on the 64 x 64 batch with the default parameters (clouds_per_tile 0.5), after 100 frames of that wind.  The kernel
form and the driver's simple form ("kernels.simple": the reference's loops on one thread) are measured in the same run.

Every repetition is timed on its own with device events on the context's stream, after a warm-up; a figure is the median of --reps calls, in --rounds rounds that
alternate the two forms; `spread` is the largest distance between two rounds' medians of one call and form -- what a difference has to exceed.  An update series starts
from the same state in both forms (the state after the 100 frames, put back before every series), so both run the same --reps frames; both forms' outputs are compared.
Per batch one JSON line: the times, the records, the clouds a frame moves and how many of them leave their tile (first hops, recomputed on the host from the state
before the frame), the hand-overs among them (the neighbour is in the batch), the listed entries and the exact-height evaluations of the view.
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


def timed(t, reps, warmup, fn, before=None):
    """median us per call over reps single calls"""
    if before:
        before()
    for _ in range(warmup):
        fn()
    t.synchronize()
    us = []
    for _ in range(reps):
        t.timer_start()
        fn()
        us.append(1000.0 * t.timer_stop())
    return round(float(np.median(us)), 1)


def first_hops(pkg, tiles, state, clouds, step):
    """(records moved, records that leave their tile, of them handed to a tile of the batch) in the next frame, first hops only"""
    d = 0.01 * float(step.fticks)
    mv = [f32(d * float(step.wind[0])), f32(d * float(step.wind[1]))]
    index = {(int(x), int(y)) for x, y in tiles}
    moved = left = handed = 0
    for t in np.flatnonzero((state["generated"] != 0) & (state["count"] > 0)):
        r, rec = state[t]["range"], clouds[t, :state[t]["count"]]
        ws = f32(0.5 / float(f32(r[5] - r[4])))
        wscale = f32(1.5) - ws * (rec["pos"][:, 2] - r[4])
        x, y = rec["pos"][:, 0] + wscale * mv[0], rec["pos"][:, 1] + wscale * mv[1]
        dx, dy = (x > r[1]).astype(int) - (x < r[0]).astype(int), (y > r[3]).astype(int) - (y < r[2]).astype(int)
        out = (dx != 0) | (dy != 0)
        moved += len(rec)
        left += int(out.sum())
        handed += sum((int(tiles[t][0] + a), int(tiles[t][1] + b)) in index for a, b in zip(dx[out], dy[out]))
    return moved, left, handed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--sides", type=int, nargs="+", default=[3, 64], help="a batch is side x side tiles")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    S, cap = 128, 32
    Z = S + 2
    st0 = t.init_scene(pkg.make_config(mesh_gen_mode=0))
    angle, aspect = 0.5236, 16.0 / 9.0
    bsm = t.view_behind_sphere_mult(angle, aspect)
    step = pkg.make_cloud_step((0.4, 0.2, 0.0), 1.0, 1)
    for side in a.sides:
        lo = -(side // 2)
        tiles = np.array([(x, y) for y in range(lo, lo + side) for x in range(lo, lo + side)], np.int32)
        n = len(tiles)
        names = ("zb", "ss", "st", "cl", "to", "sg", "li", "lc")
        sizes = (n * Z * Z * 4, n * C.sizeof(pkg.TileStats), n * 88, n * cap * 32, 4, n * cap, n * cap * 24, 4)
        b = {k: t.alloc(s) for k, s in zip(names, sizes)}
        t.tiles_create_zvals_dev(tiles, 0, b["zb"].ptr, b["ss"].ptr)
        b["st"].upload(np.zeros(n * 88, np.uint8))
        b["cl"].upload(np.zeros(n * cap * 32, np.uint8))
        for _ in range(a.frames):
            t.tiles_update_clouds_dev(tiles, step, b["st"].ptr, b["cl"].ptr, cap, b["to"].ptr)
        state0, clouds0 = b["st"].download(np.uint8, (n * 88,)).copy(), b["cl"].download(np.uint8, (n * cap * 32,)).copy()
        state, clouds = state0.view(pkg.CLOUD_TILE_DTYPE), clouds0.view(pkg.CLOUD_DTYPE).reshape(n, cap)
        view = t.make_view((0.0, 0.0, 0.5 * float(st0.zmax)), (1.0, 0.3, 0.1), (0.0, 0.0, 1.0), angle, aspect, 0.01, 1000.0)
        va = pkg.make_cloud_view_args(bsm, (0.0, 0.0, 0.0), 200.0)

        def restore():
            b["st"].upload(state0)
            b["cl"].upload(clouds0)
        calls = {"update": (lambda: t.tiles_update_clouds_dev(tiles, step, b["st"].ptr, b["cl"].ptr, cap, b["to"].ptr), restore),
                 "view": (lambda: t.tiles_cloud_view_dev(tiles, view, va, b["ss"].ptr, b["st"].ptr, b["cl"].ptr, cap, b["sg"].ptr, b["li"].ptr, b["lc"].ptr), restore)}

        def outputs():
            cnt = int(b["lc"].download(np.uint32, (1,))[0])
            s = b["st"].download(np.uint8, (n * 88,)).copy().view(pkg.CLOUD_TILE_DTYPE)
            c = b["cl"].download(np.uint8, (n * cap * 32,)).copy().view(pkg.CLOUD_DTYPE).reshape(n, cap)
            recs = b"".join(c[k, :s[k]["count"]].tobytes() for k in range(n))
            return (s.tobytes(), recs, b["to"].download(np.uint32, (1,)).tobytes(), b["sg"].download(np.uint8, (n * cap,)).tobytes(),
                    b["li"].download(np.uint8, (n * cap * 24,))[:cnt * 24].tobytes(), cnt)
        rounds = {(k, form): [] for k in calls for form in ("kernels", "simple")}
        results = {}
        for _ in range(a.rounds):
            for form in ("kernels", "simple"):
                t.set_option("kernels.simple", "1" if form == "simple" else "0")
                try:
                    for k, (fn, before) in calls.items():
                        rounds[(k, form)].append(timed(t, a.reps, a.warmup, fn, before))
                finally:
                    t.set_option("kernels.simple", "0")
        # both forms, one frame and one view from the same state
        for form in ("kernels", "simple"):
            t.set_option("kernels.simple", "1" if form == "simple" else "0")
            try:
                restore()
                calls["update"][0]()
                calls["view"][0]()
                results[form] = outputs()
            finally:
                t.set_option("kernels.simple", "0")
        assert results["kernels"] == results["simple"], "the two forms disagree"
        stage = np.frombuffer(results["kernels"][3], np.uint8).reshape(n, cap)
        s1 = np.frombuffer(results["kernels"][0], pkg.CLOUD_TILE_DTYPE)
        stats = (pkg.TileStats * n).from_buffer_copy(b["ss"].download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        mzmax = np.array([stats[k].mzmax for k in range(n)], f32)
        c1 = b["cl"].download(np.uint8, (n * cap * 32,)).copy().view(pkg.CLOUD_DTYPE).reshape(n, cap)
        reached = (stage == pkg.CLV_BELOW_MESH) | (stage == pkg.CLV_LISTED)
        zbot = c1["pos"][:, :, 2] - c1["size"][:, :, 2]
        exact = int((reached & (zbot < mzmax[:, None] + c1["size"][:, :, 2])).sum())
        moved, left, handed = first_hops(pkg, tiles, state, clouds, step)
        out = {"tiles": n, "tile_size": S, "capacity": cap, "frames_before": a.frames, "reps": a.reps, "rounds": a.rounds, "records": int(state["count"].sum()),
               "records_after": int(s1["count"].sum()), "clouds_moved": moved, "leaving": left, "hand_overs": handed, "listed": results["kernels"][5], "exact_height_evals": exact,
               "overflow_tiles": int((s1["flags"] & 1).sum())}
        for (k, form), r in rounds.items():
            out[f"{k}_{form}_us"] = {"median": round(float(np.median(r)), 1), "rounds": r}
        out["spread_us"] = round(max(max(r) - min(r) for r in rounds.values()), 1)
        print(json.dumps(out), flush=True)
        for x in b.values():
            x.free()
    t.close()


if __name__ == "__main__":
    main()
