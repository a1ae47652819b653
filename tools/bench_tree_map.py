"""The tree map (terra_tiles_tree_map_dev), the shadow texture (terra_tiles_shadow_texture_dev) and the tree weights (terra_tiles_tree_weights_dev) on a
device-resident tile batch at S = 128 (64 x 64 = 4096 tiles by default): microseconds per call of the tree map with 0, 256 and 2048 trees per tile (seeded, uniform over the
tile, radii of 1 .. 6 texels: rval 2 .. 6), microseconds per batch of the two streaming passes and the bytes they move per second.  Device events on the context's
stream, after a warm-up.  Prints one JSON line.  (The kernels' own time: run this under `rocprofv3 --kernel-trace --stats`.)"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(t, calls, warmup, fn):
    for _ in range(warmup):
        fn()
    t.synchronize()
    t.timer_start()
    for _ in range(calls):
        fn()
    return 1000.0 * t.timer_stop() / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-tile", type=int, nargs="*", default=[0, 256, 2048])
    ap.add_argument("--side", type=int, default=64, help="the batch is side x side tiles")
    a = ap.parse_args()
    pkg = importlib.import_module("3dworld_amd")
    t = pkg.Terra(0)
    st = t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    tiles = np.array([(x, y) for y in range(-a.side // 2, a.side // 2) for x in range(-a.side // 2, a.side // 2)], np.int32)
    n, S = len(tiles), 128
    W, Z = S + 1, S + 2
    zb, sun, moon, ao = t.alloc(n * Z * Z * 4), t.alloc(n * Z * Z), t.alloc(n * Z * Z), t.alloc(n * W * W)
    tm, upd, sh = t.alloc(n * W * W * 2), t.alloc(n), t.alloc(n * W * W * 4)
    mw, gb, wt = t.alloc(n * W * W * 4), t.alloc(n * 32 * 32 * 12), t.alloc(n * W * W * 4)
    bufs = [zb, sun, moon, ao, tm, upd, sh, mw, gb, wt]
    t.tiles_create_zvals_dev(tiles, 0, zb.ptr)
    t.tiles_mesh_shadows_dev(tiles, zb.ptr, (1.0, 0.6, 0.3), sun.ptr)
    t.tiles_mesh_shadows_dev(tiles, zb.ptr, (-0.4, -1.0, 0.15), moon.ptr)
    t.tiles_ao_lighting_dev(tiles, zb.ptr, ao.ptr)
    t.tiles_create_weights_dev(tiles, zb.ptr, mw.ptr, gb.ptr)
    out = {"tiles": n, "tile_size": S, "tree_map_us_per_call": {}}
    rs = np.random.RandomState(1)
    x0 = (-4.0 + st.DX_VAL * S * tiles[:, 0].astype(np.float64))[:, None]  # get_xval(x1) (scene_x = scene_y = 4)
    y0 = (-4.0 + st.DY_VAL * S * tiles[:, 1].astype(np.float64))[:, None]
    for per in a.per_tile:
        sp = np.zeros(n * per, pkg.TREE_SPLAT_DTYPE)
        if per:
            sp["x"] = (x0 + st.DX_VAL * rs.uniform(0.0, S, (n, per))).reshape(-1)
            sp["y"] = (y0 + st.DY_VAL * rs.uniform(0.0, S, (n, per))).reshape(-1)
            sp["radius"] = st.DX_VAL * rs.uniform(1.0, 5.99, n * per)
        first = (np.arange(n + 1, dtype=np.uint64) * per).astype(np.uint32)
        sb = t.alloc(max(sp.nbytes, 256)).upload(sp)
        calls = a.calls if per <= 256 else max(5, a.calls // 5)
        us = timed(t, calls, a.warmup, lambda: t.tiles_tree_map_dev(tiles, sb.ptr, first, tm.ptr, upd.ptr))
        out["tree_map_us_per_call"][str(per)] = round(us, 2)
        if per == a.per_tile[-1]:  # the two texture passes read the last tree map
            out["updated_tiles"] = int(upd.download(np.uint8, (n,)).sum())
            us = timed(t, a.calls, a.warmup, lambda: t.tiles_shadow_texture_dev(n, 0.5, sh.ptr, True, sun.ptr, moon.ptr, ao.ptr, tm.ptr))
            nbytes = n * (2 * Z * Z + W * W * (1 + 2 + 4))  # both masks, AO, the tree map, the texture (the masks' lines are read whole)
            out["shadow_texture"] = {"us_per_batch": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3)}
            us = timed(t, a.calls, a.warmup, lambda: t.tiles_tree_weights_dev(n, mw.ptr, tm.ptr, wt.ptr))
            nbytes = n * W * W * (4 + 2 + 4)  # mesh_weight_data, the tree map (its lines are read whole), weight_data
            out["tree_weights"] = {"us_per_batch": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3)}
        sb.free()
    for b in bufs:
        b.free()
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
