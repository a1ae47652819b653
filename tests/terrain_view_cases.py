"""Cases of the terrain draw list (terra_tiles_terrain_view[_dev]) shared by test_terrain_view_emul.py (the host emulator) and test_gpu_terrain_view.py (HIP on the
MI355X).  status, dist, lod, crack, both lists in order, counts and the written occl_state are compared byte for byte with tests/terrain_view_model.py.

The call needs no zvals, so the cases feed synthetic terra_tile_stats on the synthetic 4 x 4 scene: a tile is 8 wide at every S, tile (0, 0) spans [-4, 4]^2,
get_scaled_tile_radius() is 48 (DRAW_DIST_TILES reaches 72 beyond a tile's radius, OCCLUDER_DIST 9.6), the water plane lies at about -5.9.  The model's result of a
case is computed once per process (MODEL) together with its tally, and every case carries a check on that tally: that it exercises what it is named for."""
import ctypes as C
import math

import numpy as np

import orclib
import terrain_view_model as tm
import view_model

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
ORDER_LDS_CAPACITY = 1024  # the drawn tiles that the kernels' fast ordering path holds (TV_ORDER_LDS, terra_kernels.hpp)
ALONG_X = dict(dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))


def grid(r):
    return [(x, y) for y in range(-r, r + 1) for x in range(-r, r + 1)]


GRID9 = grid(4)


class Case:
    def __init__(self, name, S=16, tiles=GRID9, terrain="ridge", view=None, valid=1, args=None, arrays=None, dxoff=0, dyoff=0, check=None):
        self.name, self.S, self.tiles, self.terrain, self.valid = name, S, list(tiles), terrain, valid
        self.view = dict(pos=(0.3, 0.2, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X) if view is None else dict(view)
        self.args = dict(args or {})
        self.arrays = arrays  # (case, n) -> dict of the optional per-tile arrays
        self.dxoff, self.dyoff, self.check = dxoff, dyoff, check


def _ridge_flags(case, n, ctx, bit):
    return dict(flags=np.array([bit if (tx == 1 and abs(ty) <= 1) else 0 for tx, ty in case.tiles], np.uint8))


def _state_in(case, n, ctx):
    # tiles that the ridge would occlude: (3, 0) and (4, 0) carry "occluded earlier this frame", (3, 1) and (4, -1) "unoccluded earlier this frame"
    st = np.zeros(n, np.uint8)
    for k, v in (((3, 0), 1), ((4, 0), 1), ((3, 1), 2), ((4, -1), 2)):
        st[case.tiles.index(k)] = v
    return dict(occl_state=st)


LOD_SPECIAL = 64  # the `lods` terrain and _lod_arrays: tiles 0 .. 63 are steep, the 17 behind them cover the other branches


def _lod_arrays(case, n, ctx):
    """min_normal_z in every branch of get_lod_level.  Tiles 0 .. 63: values in (0, 0.25) -- 32 spread geometrically over it, 32 chosen so that
    dist/-log2(2*min_normal_z) lands within a few float ulps of the loop's threshold or of a power-of-two multiple of it (where the tile is far enough for that; a
    random value otherwise).  Flag bit 2 on every third tile."""
    rng = np.random.default_rng(7)
    flags = np.array([4 if i % 3 == 0 else 0 for i in range(n)], np.uint8)
    mnz = np.zeros(n, f32)
    mnz[:32] = np.geomspace(1e-30, 0.2499, 32).astype(f32)
    thr = 1.8 if case.args.get("reflection_pass") else 2.0
    for i in range(32, LOD_SPECIAL):
        t = tm.Tile(ctx.sc, case.tiles[i], ctx.stats[i], 0.0, 0.0, None, 0, 0)
        d = float(tm.get_rel_dist_to_camera(ctx.sc, ctx.v, t, False)) * 6.0 / (2.0 if flags[i] else 1.0)
        target = thr * (1, 2, 4)[i % 3] * (1.0 + (i % 5 - 2) * 6e-8)
        m = 0.5 * 2.0 ** (-d / target) if d > 0 else 1.0
        mnz[i] = f32(m) if 0.0 < m < 0.2499 else f32(rng.uniform(1e-3, 0.2499))
    # 64, 65 flat tiles; 66, 67 normals not yet calculated; 68 .. 70: (0.9, 0.95] above / astride / below the water plane; 71 .. 73: above 0.95 likewise; the rest in [0.25, 0.9]
    mnz[LOD_SPECIAL:] = np.array([0.5, 0.5, 0.0, 0.0, 0.93, 0.93, 0.93, 0.97, 0.97, 0.97, 0.25, 0.9, 0.3, 0.6, 0.45, 0.8, 0.7], f32)[:n - LOD_SPECIAL]
    return dict(min_normal_z=mnz, flags=flags)


def _crack_arrays(case, n, ctx):
    a = _lod_arrays(case, n, ctx)
    for hole in ((-4, 0), (4, 4), (0, 1)):  # two at the batch edge, one inside
        a["flags"][case.tiles.index(hole)] |= 1
    return a


def _all_arrays(case, n, ctx):
    rng = np.random.default_rng(11)
    a = _lod_arrays(case, n, ctx)
    a["trmax"] = rng.uniform(0.0, 0.6, n).astype(f32)
    a["tile_zmax_add"] = rng.uniform(0.0, 0.5, n).astype(f32)  # tile_zmax = mzmax + this
    return a


def _unit(x, y, z):
    m = math.sqrt(x * x + y * y + z * z)
    return (x / m, y / m, z / m)


def cases():
    low = dict(pos=(0.3, 0.2, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
    high = dict(pos=(0.3, 0.2, 60.0), angle=0.9, aspect=1.5, near=0.05, far=300.0, dir=_unit(0.5, 0.0, -1.0), up=(0.0, 0.0, 1.0))
    away = dict(pos=(-17.0, -19.0, 1.0), angle=0.7, aspect=1.0, near=0.05, far=200.0, dir=_unit(-1.0, -0.9, 0.0), up=(0.0, 0.0, 1.0))
    centre = dict(pos=(0.0, 0.0, 30.0), angle=1.2, aspect=1.0, near=0.05, far=300.0, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
    lodv = dict(pos=(-30.0, -28.0, 3.0), angle=1.0, aspect=1.0, near=0.05, far=400.0, dir=_unit(1.0, 1.0, -0.1), up=(0.0, 0.0, 1.0))
    lod_check = lambda t, r, cap: (min(t["lod_flat"], t["lod_mnz0"], t["lod_mid"], t["lod_smap"]) >= 1 and t["lod_flat2"] >= 2 and t["lod_flat4"] >= 2  # noqa: E731
                                   and t["lod_water_blocked"] >= 2 and t["lod_steep"] >= 64 and t["max_lod_not_flat"] == cap)
    big = [(x, y) for y in range(-20, 20) for x in range(-20, 20)]
    return [
        Case("ridge_low_camera", view=low, check=lambda t, r: t["occluded"] >= 3 and t["one_sub_unoccluded"] >= 1 and t["occluders"] >= 2 and t["columns_zeroed"] >= 1
             and t["centre_rejected"] >= 1 and t["drawn"] >= 3),
        Case("high_camera", view=high, check=lambda t, r: t["occluders"] >= 1 and t["occluded"] == 0 and t["tested"] >= 10),
        Case("look_away", tiles=[(x, y) for y in range(-4, 5) for x in range(-4, 7)], terrain="rolling", view=away,  # (11 x 9: room for a tile beyond the draw distance)
             check=lambda t, r: min(t["too_far"], t["not_visible"], t["drawn"]) >= 1
             and min(t["sphere_all"], t["cube_accepted"], t["cube_rejected"], t["behind_true"], t["behind_false"]) >= 1),
        Case("view_invalid", view=low, valid=0, check=lambda t, r: t["not_visible"] == 0 and t["columns_zeroed"] == 0 and t["occluded"] >= 3),
        Case("water_over_tiles", terrain="lakes", view=low, args=dict(water_enabled=1), check=lambda t, r: t["water_radius"] >= 3 and t["water_z2"] >= 3),
        Case("water_over_tiles_disabled", terrain="lakes", view=low, args=dict(water_enabled=0), check=lambda t, r: t["water_radius"] == 0 and t["water_z2"] >= 3),
        Case("lod_classes_s16", terrain="lods", view=lodv, arrays=_lod_arrays, check=lambda t, r: lod_check(t, r, 2)),
        Case("lod_classes_s16_pass2", terrain="lods", view=lodv, arrays=_lod_arrays, args=dict(reflection_pass=2), check=lambda t, r: lod_check(t, r, 2)),
        Case("lod_classes_s32", S=32, terrain="lods", view=lodv, arrays=_lod_arrays, check=lambda t, r: lod_check(t, r, 3)),
        Case("lod_classes_s32_pass2", S=32, terrain="lods", view=lodv, arrays=_lod_arrays, args=dict(reflection_pass=2), check=lambda t, r: lod_check(t, r, 3)),
        Case("lod_classes_s128", S=128, terrain="lods", view=lodv, arrays=_lod_arrays, check=lambda t, r: lod_check(t, r, 4)),
        Case("lod_classes_s128_pass3", S=128, terrain="lods", view=lodv, arrays=_lod_arrays, args=dict(reflection_pass=3), check=lambda t, r: lod_check(t, r, 4)),
        Case("cracks", S=32, terrain="lods", view=lodv, arrays=_crack_arrays, dxoff=3, dyoff=-2, check=lambda t, r: t["absent"] == 3 and t["no_neighbour"] >= 4
             and min(t["adj_lower"], t["adj_equal"], t["adj_higher"]) >= 1),
        Case("state_in", view=low, arrays=_state_in, check=lambda t, r: t["occluded_before"] == 2 and t["test_skipped_state"] == 2 and t["occluded"] >= 1),
        Case("flags_no_occluder", view=low, arrays=lambda c, n, x: _ridge_flags(c, n, x, 2), check=lambda t, r: t["occluded"] == 0 and t["occluders"] >= 1),
        Case("ridge_absent", view=low, arrays=lambda c, n, x: _ridge_flags(c, n, x, 1), check=lambda t, r: t["occluded"] == 0 and t["absent"] == 3),
        Case("check_occlusion_off", view=low, args=dict(check_occlusion=0), check=lambda t, r: t["occluders"] == 0 and t["tested"] == 0 and t["occluded"] == 0),
        Case("ties", terrain="flat", view=centre, check=lambda t, r: t["ties"] >= 8),
        Case("all_arrays", terrain="rolling", view=low, arrays=_all_arrays, dxoff=-5, dyoff=7, check=lambda t, r: t["drawn"] >= 5),
        # more drawn tiles than the kernels' fast ordering path holds: all distances equal (the radii reach the camera from everywhere), then distinct ones
        Case("many_drawn_equal", tiles=big, terrain="huge_radius", view=centre, valid=0, args=dict(check_occlusion=0),
             check=lambda t, r: t["drawn"] > ORDER_LDS_CAPACITY and t["ties"] == t["drawn"] - 1),
        Case("many_drawn_distinct", tiles=big, terrain="big_radius", view=dict(centre, pos=(0.37, -0.21, 30.0)), valid=0, args=dict(check_occlusion=0),
             check=lambda t, r: t["drawn"] > ORDER_LDS_CAPACITY and t["ties"] < t["drawn"] // 2),
    ]


def stats_of(pkg_or_orclib, case, wpz):
    """synthetic terra_tile_stats: 16 sub-box ranges a tile, mzmin / mzmax over them, radius as tile_t::calc_radius does (half the diagonal of the mesh box)"""
    n = len(case.tiles)
    stats = (pkg_or_orclib.TileStats * n)()
    rng = np.random.default_rng(3)
    for t, (tx, ty) in enumerate(case.tiles):
        lo = 0.05 * rng.random(16) + 0.02 * (tx - ty)
        hi = lo + 0.1 + 0.2 * rng.random(16)
        radius = None
        if case.terrain == "ridge":  # a wall of high sub_zmin beside the camera's tile; behind it one tile with a single tall sub-box
            if tx == 1 and abs(ty) <= 1:  # (one low column keeps the mesh box, which the centre segments must cross, down at the camera's height)
                lo, hi = lo + 6.0, hi + 6.0
                lo[0], hi[0] = lo[0] - 6.0, hi[0] - 6.0
            if (tx, ty) == (3, 0):
                hi[5] = 40.0
        elif case.terrain == "rolling":
            lo = lo + 1.5 * math.sin(0.8 * tx) * math.cos(0.6 * ty)
            hi = hi + 1.5 * math.sin(0.8 * tx) * math.cos(0.6 * ty)
        elif case.terrain == "lakes":  # every other column of tiles lies below the water plane
            if tx % 2 == 0 and tx != 0:
                lo, hi = lo + wpz - 2.0, hi + wpz - 2.0
        elif case.terrain == "lods":  # flat tiles, tiles astride the water plane, tiles below it, the rest above (see _lod_arrays)
            if t in (LOD_SPECIAL, LOD_SPECIAL + 1):
                lo[:], hi[:] = 0.25, 0.25
            elif t in (LOD_SPECIAL + 5, LOD_SPECIAL + 8) or t % 16 == 3:
                lo, hi = lo + wpz - 0.3, hi + wpz + 0.3
            elif t in (LOD_SPECIAL + 6, LOD_SPECIAL + 9) or t % 16 == 7:
                lo, hi = lo + wpz - 3.0, hi + wpz - 3.0
        elif case.terrain == "flat":
            lo[:], hi[:] = 0.0, 0.5
        elif case.terrain == "huge_radius":
            lo[:], hi[:] = 0.0, 0.5
            radius = 400.0
        elif case.terrain == "big_radius":
            lo[:], hi[:] = 0.0, 0.5
            radius = 100.0 + 0.001 * t
        st = stats[t]
        for k in range(16):
            st.sub_zmin[k], st.sub_zmax[k] = float(f32(lo[k])), float(f32(hi[k]))
        st.mzmin, st.mzmax = min(st.sub_zmin), max(st.sub_zmax)
        st.radius = float(f32(radius if radius is not None else 0.5 * math.sqrt(8.0 ** 2 + 8.0 ** 2 + (st.mzmax - st.mzmin) ** 2)))
    return stats


def view_of(case):
    import grass_view_model as gm
    v = view_model.make_view(**case.view)
    v.valid = case.valid
    return v


def args_of(case):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]), occluder_zmin=-8.0, water_enabled=1, check_occlusion=1, reflection_pass=0)
    kw.update(case.args)
    return tm.Args(**kw)


class Ctx:
    def __init__(self, sc, stats, v):
        self.sc, self.stats, self.v = sc, stats, v


def arrays_of(case, sc, stats, v):
    n = len(case.tiles)
    a = dict(min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None)
    if case.arrays is not None:
        got = case.arrays(case, n, Ctx(sc, stats, v))
        add = got.pop("tile_zmax_add", None)
        a.update(got)
        if add is not None:
            a["tile_zmax"] = np.array([f32(stats[t].mzmax) + add[t] for t in range(n)], f32)
    return a


MODEL = {}


def model(orc, case):
    """(scene, stats, view, args, arrays, result, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
        orc.init(ocfg)
        sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
        stats, v, a = stats_of(orclib, case, float(sc.water_plane_z)), view_of(case), args_of(case)
        arr = arrays_of(case, sc, stats, v)
        tally = tm.new_tally()
        res = tm.draw(sc, v, a, case.tiles, stats, tally=tally, **arr)
        MODEL[case.name] = (sc, stats, v, a, arr, res, tally)
    return MODEL[case.name]


def lib_view(pkg, v):
    lv = pkg.View()
    C.memmove(C.addressof(lv), v.words(), C.sizeof(lv))
    return lv


def lib_args(pkg, a):
    return pkg.make_terrain_view_args(float(a.behind_sphere_mult), float(a.occluder_zmin), a.water_enabled, a.check_occlusion, a.reflection_pass)


def configure(pkg, t, case):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))


def compare(what, got, want, state_in):
    """(status, dist, lod, crack, draw_order, occluded, counts, occl_state) against the model's (status, dist, lod, crack, draw_order, occluded, occl_state)"""
    status, dist, lod, crack, order, occluded, counts, state = got
    w_status, w_dist, w_lod, w_crack, w_order, w_occluded, w_state = want
    assert counts.tolist() == [len(w_order), len(w_occluded)], f"{what}: counts {counts.tolist()} != {[len(w_order), len(w_occluded)]}"
    bad = np.argwhere(status != w_status)
    assert len(bad) == 0, f"{what}: status of tile {int(bad[0, 0])}: {int(status[bad[0, 0]]):#x} != {int(w_status[bad[0, 0]]):#x} ({len(bad)} differ)"
    bad = np.argwhere(dist.view(np.uint32) != w_dist.view(np.uint32))
    assert len(bad) == 0, f"{what}: dist of tile {int(bad[0, 0])}: {dist[bad[0, 0]]!r} != {w_dist[bad[0, 0]]!r}"
    bad = np.argwhere(lod != w_lod)
    assert len(bad) == 0, f"{what}: lod of tile {int(bad[0, 0])}: {int(lod[bad[0, 0]])} != {int(w_lod[bad[0, 0]])} ({len(bad)} differ)"
    assert crack.tobytes() == w_crack.tobytes(), f"{what}: cracks differ at {np.argwhere(crack != w_crack)[:4].tolist()}"
    assert order.tolist() == list(w_order), f"{what}: draw order differs, first at {next(k for k in range(len(w_order)) if order[k] != w_order[k])}"
    assert occluded.tolist() == list(w_occluded), f"{what}: occluded list {occluded.tolist()} != {list(w_occluded)}"
    if state_in is not None:
        assert state is not None and state.tolist() == w_state.tolist(), f"{what}: occl_state {state.tolist()} != {w_state.tolist()}"


def run_dev(pkg, t, tiles, stats, lv, la, arr, dxoff=0, dyoff=0):
    """the device-pointer form on freshly allocated buffers -> what Terra.tiles_terrain_view returns; the lists' tails must come back untouched"""
    n = len(tiles)
    bufs = dict(st=t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8)), su=t.alloc(n).upload(np.full(n, 0x77, np.uint8)), di=t.alloc(n * 4).upload(np.full(n, -1.0, f32)),
                lo=t.alloc(n).upload(np.full(n, 0x77, np.uint8)), cr=t.alloc(n * 4).upload(np.full(n * 4, 0x77, np.uint8)),
                dr=t.alloc(n * 4).upload(np.full(n, 0xABCDEF01, np.uint32)), oc=t.alloc(n * 4).upload(np.full(n, 0xABCDEF01, np.uint32)), cn=t.alloc(8).upload(np.full(2, 7, np.uint32)))
    bufs["nd"] = t.alloc(n).upload(np.full(n, 0x77, np.uint8))
    for k, key, dt in (("mn", "min_normal_z", f32), ("tr", "trmax", f32), ("tz", "tile_zmax", f32), ("fl", "flags", np.uint8), ("os", "occl_state", np.uint8)):
        if arr[key] is not None:
            a = np.ascontiguousarray(arr[key], dt)
            bufs[k] = t.alloc(a.nbytes).upload(a)
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_terrain_view_dev(tiles, lv, la, bufs["st"].ptr, bufs["su"].ptr, bufs["di"].ptr, bufs["lo"].ptr, bufs["cr"].ptr, bufs["dr"].ptr, bufs["oc"].ptr, bufs["cn"].ptr,
                                 ptr("mn"), ptr("tr"), ptr("tz"), ptr("fl"), ptr("os"), bufs["nd"].ptr, dxoff, dyoff)
        counts = bufs["cn"].download(np.uint32, (2,)).copy()
        assert (bufs["nd"].download(np.uint8, (n,)) == ((bufs["su"].download(np.uint8, (n,)) & 7) != tm.DRAWN)).all(), "not_drawn is not (status != drawn)"
        order, occluded = bufs["dr"].download(np.uint32, (n,)).copy(), bufs["oc"].download(np.uint32, (n,)).copy()
        assert (order[counts[0]:] == 0xABCDEF01).all() and (occluded[counts[1]:] == 0xABCDEF01).all(), "entries past the counts were written"
        return (bufs["su"].download(np.uint8, (n,)).copy(), bufs["di"].download(f32, (n,)).copy(), bufs["lo"].download(np.uint8, (n,)).copy(),
                bufs["cr"].download(np.uint8, (n, 4)).copy(), order[:counts[0]], occluded[:counts[1]], counts,
                bufs["os"].download(np.uint8, (n,)).copy() if "os" in bufs else None)
    finally:
        for b in bufs.values():
            b.free()


def run_case(pkg, t, orc, case, dev=False):
    sc, stats, v, a, arr, res, tally = model(orc, case)
    assert case.check(tally, res), (case.name, tally)
    configure(pkg, t, case)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv, la = lib_view(pkg, v), lib_args(pkg, a)
    if not dev:
        got = t.tiles_terrain_view(case.tiles, lstats, lv, la, dxoff=case.dxoff, dyoff=case.dyoff, **arr)
    else:
        got = run_dev(pkg, t, case.tiles, lstats, lv, la, arr, case.dxoff, case.dyoff)
    compare(case.name + (" (dev)" if dev else ""), got, res, arr["occl_state"])


def run_resident_chain(pkg, gpu, orc):
    """tiles_create_zvals_dev (zvals, stats, normals, min_normal_z) -> tiles_terrain_view_dev -> its not_drawn bytes as the skip bytes of tiles_grass_view_dev (behind
    tiles_create_weights_dev) on a 5 x 5 batch at S = 128 on one context with nothing read back in between, against the two models chained on the oracle's tiles"""
    import grass_brush_cases as gbc
    import grass_view_cases as gvc
    import grass_view_model as gm
    S, cap, nrnd = 128, 1024, 16
    tiles = grid(2)
    n, Z, T = len(tiles), S + 2, S + 1
    bsc, d = gbc.setup(pkg, gpu, orc, tiles)  # the scene and the landscape on both sides; the model's zvals, stats and grass blocks from the oracle
    gpu.set_grass_view_params(pkg.make_grass_view_params(0.25))
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gsc, sc = gm.Scene(orc, cfg, gm.Params(0.25, 0.02, nrnd)), tm.Scene(orc, cfg)
    mnz = np.array([orc.tile_normals(d["z"][i])[1] for i in range(n)], f32)
    zc = float(d["z"][tiles.index((0, 0))][64, 64])
    v = view_model.make_view((3.0, -0.3, zc + 0.5), _unit(1.0, 0.4, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 40.0)
    a = tm.Args(view_model.behind_sphere_mult(0.7, 1.6), float(orc.state().zmin), 1, 1, 0)
    lv, la = lib_view(pkg, v), lib_args(pkg, a)
    state = np.zeros(n, np.uint8)
    state[tiles.index((1, 0))] = 1  # the tile ahead of the camera, within the grass distance, was occluded in the shadow pass: only the skip byte keeps its grass out
    bufs = dict(os=gpu.alloc(n).upload(state), z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), nm=gpu.alloc(n * T * T * 4), mn=gpu.alloc(n * 4), w=gpu.alloc(n * T * T * 4),
                gb=gpu.alloc(n * 32 * 32 * 12), su=gpu.alloc(n), di=gpu.alloc(n * 4), lo=gpu.alloc(n), cr=gpu.alloc(n * 4), dr=gpu.alloc(n * 4), oc=gpu.alloc(n * 4), cn=gpu.alloc(8),
                sk=gpu.alloc(n), ins=gpu.alloc(n * cap * 8).upload(np.zeros(n * cap * 2, f32)), ax=gpu.alloc(n * cap * 4).upload(np.zeros(n * cap, np.uint32)),
                gc=gpu.alloc(n * 6 * nrnd * 4), gcn=gpu.alloc(n * 4), ps=gpu.alloc(n))
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        gpu.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"], p["nm"], p["mn"])
        gpu.tiles_terrain_view_dev(tiles, lv, la, p["st"], p["su"], p["di"], p["lo"], p["cr"], p["dr"], p["oc"], p["cn"], min_normal_z_ptr=p["mn"], occl_state_ptr=p["os"], not_drawn_ptr=p["sk"])
        gpu.tiles_create_weights_dev(tiles, p["z"], p["w"], p["gb"])
        gpu.tiles_grass_view_dev(tiles, p["z"], p["st"], p["gb"], lv, cap, p["ins"], p["gc"], p["gcn"], p["ax"], p["ps"], p["sk"])
        counts = bufs["cn"].download(np.uint32, (2,)).copy()
        got = (bufs["su"].download(np.uint8, (n,)).copy(), bufs["di"].download(f32, (n,)).copy(), bufs["lo"].download(np.uint8, (n,)).copy(), bufs["cr"].download(np.uint8, (n, 4)).copy(),
               bufs["dr"].download(np.uint32, (n,))[:counts[0]].copy(), bufs["oc"].download(np.uint32, (n,))[:counts[1]].copy(), counts, bufs["os"].download(np.uint8, (n,)).copy())
        skip = bufs["sk"].download(np.uint8, (n,)).copy()
        grass = (bufs["ins"].download(f32, (n, cap, 2)).copy(), bufs["ax"].download(np.uint32, (n, cap)).copy(), bufs["gc"].download(np.uint32, (n, 6, nrnd)).copy(),
                 bufs["gcn"].download(np.uint32, (n,)).copy(), bufs["ps"].download(np.uint8, (n,)).copy())
    finally:
        for b in bufs.values():
            b.free()
    tally = tm.new_tally()
    want = tm.draw(sc, v, a, tiles, d["stats"], min_normal_z=mnz, occl_state=state, tally=tally)
    compare("resident chain, terrain view", got, want, state)
    w_skip = ((want[0] & 7) != tm.DRAWN).astype(np.uint8)
    assert skip.tolist() == w_skip.tolist()
    assert tally["drawn"] >= 3 and tally["not_visible"] >= 3 and tally["lod_steep"] + tally["lod_mid"] + tally["lod_flat2"] + tally["lod_flat4"] >= n - tally["lod_flat"] - 1, tally
    lists, gcw, ps = gm.view_batch(gsc, v, tiles, d["z"], d["stats"], d["gb"], w_skip, gm.new_tally())
    gvc.compare("resident chain, grass view behind the terrain view", gsc, grass, lists, gcw, ps, cap)
    unskipped, _, _ = gm.view_batch(gsc, v, tiles, d["z"], d["stats"], d["gb"], None, gm.new_tally())
    assert sum(len(x) for x in lists) >= 50 and any(len(unskipped[t]) > 0 and w_skip[t] for t in range(n)), "the skip bytes decide nothing"
