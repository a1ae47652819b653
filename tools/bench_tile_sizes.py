#!/usr/bin/env python3
"""Tile batches of equal area at three tile sizes: 64^2 tiles at S = 128, 32^2 at S = 256, 8^2 at S = 1024 (mesh_xy = S).  Per size and product: zvals + post
(stats + normals), eroded zvals + post (1000 droplets), AO lighting, mesh shadows -- ms per batch (median of the timed reps, device timer) and ns per cell.
One JSON line per size.  usage: bench_tile_sizes.py [reps=3] [sizes=128,256,1024]"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

pkg = importlib.import_module("3dworld_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [128, 256, 1024]
SIDE = {128: 64, 256: 32, 1024: 8}  # tiles a side: 8192^2 cells each


def timed(t, fn):
    fn()  # warm-up (scratch, first launches)
    ms = []
    for _ in range(reps):
        t.synchronize(); t.timer_start()
        fn()
        ms.append(t.timer_stop())
    return float(np.median(ms))


t = pkg.Terra(0)
for S in sizes:
    side = SIDE.get(S, max(1, 8192 // S))
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    assert t.tile_size == S
    tiles = np.array([(tx, ty) for ty in range(-side // 2, side - side // 2) for tx in range(-side // 2, side - side // 2)], np.int32)
    n, zv, st = len(tiles), S + 2, S + 1
    zt = t.alloc(n * zv * zv * 4); stt = t.alloc(n * 160); nm = t.alloc(n * st * st * 4); mz = t.alloc(n * 4); ao = t.alloc(n * st * st); sm = t.alloc(n * zv * zv)
    try:
        r = {"S": S, "tiles": n, "cells": n * S * S}
        r["zvals_post_ms"] = timed(t, lambda: t.tiles_create_zvals_dev(tiles, 0, zt.ptr, stt.ptr, nm.ptr, mz.ptr))
        r["eroded_1000_ms"] = timed(t, lambda: t.tiles_create_zvals_dev(tiles, 1000, zt.ptr, stt.ptr, nm.ptr, mz.ptr))
        t.tiles_create_zvals_dev(tiles, 0, zt.ptr, stt.ptr, nm.ptr, mz.ptr)
        r["ao_ms"] = timed(t, lambda: t.tiles_ao_lighting_dev(tiles, zt.ptr, ao.ptr))
        r["shadows_ms"] = timed(t, lambda: t.tiles_mesh_shadows_dev(tiles, zt.ptr, (0.6, 0.5, 0.4), sm.ptr))
        for k in ("zvals_post", "eroded_1000", "ao", "shadows"):
            r[k + "_ns_per_cell"] = round(1e6 * r[k + "_ms"] / r["cells"], 4)
        print(json.dumps(r), flush=True)
    finally:
        for b in (zt, stt, nm, mz, ao, sm):
            b.free()
t.close()
