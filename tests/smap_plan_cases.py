"""Cases of the shadow-map plan (terra_tiles_smap_plan[_dev]), of the caster lists (terra_tiles_smap_casters[_dev]) and of terra_make_light_view, shared by
test_smap_plan_emul.py (the host emulator) and test_gpu_smap_plan.py (HIP on the MI355X).  Every output is compared byte for byte with tests/smap_plan_model.py;
lists are compared in order up to their counts; entries past the counts and the outputs of tiles a call does not write must keep the fill pattern they went in with.

The cases live on the synthetic scene of terrain_view_cases.py: a tile is 8 wide at every S, tile (0, 0) spans [-4, 4]^2, get_scaled_tile_radius() is 48, so a
tile's distance in tiles is (its centre's xy distance - its radius)/8 and SMAP_NEW_THRESH lies at 9.6*smap_thresh_scale beyond the radius.  Synthetic stats by kind
as in water_view_cases.py.  The model's result of a case is computed once per process together with its tally, and every case carries a check on that tally: that
it exercises what it is named for."""
import ctypes as C

import numpy as np

import orclib
import smap_plan_model as sm
import terrain_view_cases as tc
import terrain_view_model as tm
import view_model
import water_view_cases as wc

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
grid, GRID9, ALONG_X, _unit = tc.grid, tc.GRID9, tc.ALONG_X, tc._unit
GRID3, GRID13 = grid(1), grid(6)
BIG = [(x, y) for y in range(-20, 20) for x in range(-20, 20)]
LOW = dict(pos=(0.3, 0.2, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
NARROW = dict(pos=(0.3, 0.2, 0.5), angle=0.25, aspect=1.0, near=0.05, far=200.0, **ALONG_X)
CORNER = dict(pos=(-41.0, -38.5, 0.5), angle=0.9, aspect=1.5, near=0.05, far=400.0, dir=_unit(1.0, 1.0, 0.0), up=(0.0, 0.0, 1.0))
FILL32, FILL8, FILLF = 0xABCDEF01, 0x77, -7.5
HIGH_SUN, LOW_SUN_X, MOON_NEG_Y = (30.0, 20.0, 200.0), (300.0, 0.0, 30.0), (10.0, -250.0, 60.0)


class Case:
    def __init__(self, name, S=16, tiles=GRID9, kind=None, view=LOW, valid=0, args=None, state=None, arrays=None, dxoff=0, dyoff=0, check=None, renders=None, light_valid=1, cargs=None,
                 recv_raw=None):
        self.name, self.S, self.tiles, self.kind, self.valid = name, S, list(tiles), kind, valid
        self.view, self.args, self.state, self.arrays, self.dxoff, self.dyoff, self.check = dict(view), args or {}, state, arrays, dxoff, dyoff, check
        self.terrain, self.wbox, self.radius, self.cam_z_water = None, {}, None, False  # (what water_view_cases.stats_of reads of a case)
        self.renders = renders        # casters: a list of (receiver tile or batch index, lpos)
        self.light_valid, self.cargs = light_valid, dict(cargs or {})
        self.recv_raw = recv_raw      # casters: batch indices instead of tiles, as they are (out of range included)


class Ctx:
    def __init__(self, sc, stats, v, case):
        self.sc, self.stats, self.v = sc, stats, v
        self.T = [tm.Tile(sc, case.tiles[i], stats[i], 0.0, 0.0, None, 0, 0) for i in range(len(case.tiles))]

    def in_tiles(self, i):
        return float(sm.get_dist_to_camera_in_tiles(self.sc, self.v, self.T[i]))


def _scale_for(tile, lod_f, **more):
    """smap_thresh_scale that puts `tile` at lod_level_f = lod_f"""
    def f(case, ctx):
        return dict(smap_thresh_scale=5.0 * ctx.in_tiles(case.tiles.index(tile)) / (1.2 * lod_f), **more)
    return f


def _state_all(v):
    return lambda case, n: np.full(n, v, np.uint8)


def _state_of(table, default=sm.NONE):
    def f(case, n):
        st = np.full(n, default, np.uint8)
        for k, v in table.items():
            st[case.tiles.index(k)] = v
        return st
    return f


def _absent(case, n):
    rng = np.random.default_rng(23)
    return dict(flags=(rng.random(n) < 0.3).astype(np.uint8))


def _trmax(val):
    return lambda case, n: dict(trmax=np.full(n, val, f32))


def _all_arrays(case, n):
    rng = np.random.default_rng(11)
    return dict(trmax=rng.uniform(0.0, 0.6, n).astype(f32), tile_zmax_add=rng.uniform(0.0, 0.5, n).astype(f32), flags=(rng.random(n) < 0.1).astype(np.uint8),
                terrain_flags=(rng.integers(0, 256, n) & 0xFB).astype(np.uint8) | ((rng.random(n) < 0.2) * 4).astype(np.uint8))


def _shuffle(tiles, seed):
    rng = np.random.default_rng(seed)
    return [tiles[i] for i in rng.permutation(len(tiles))]


def _word(r, case, tile):
    return int(r["plan"][case.tiles.index(tile)])


def plan_cases():
    flat = lambda tx, ty: "flat"  # noqa: E731
    X = (2, 0)  # the hysteresis tile: two tiles ahead of the camera
    cs = [
        Case("one_tile", tiles=[(0, 0)], check=lambda t, r, c: t["allocated"] == 1 and t["alloc_lod0"] == 1 and r["receivers"] == [0] and _word(r, c, (0, 0)) & sm.USABLE),
        Case("grid3_camera_in_centre", tiles=GRID3, args=dict(smap_thresh_scale=4.0), check=lambda t, r, c: t["alloc_lod0"] == 9 and r["receivers"] == list(range(9))),
        # 13 x 13 with the camera near a corner: every LOD, and tiles in each band beyond SMAP_NEW_THRESH
        Case("grid13_bands", tiles=GRID13, view=CORNER, args=dict(smap_thresh_scale=4.0),
             check=lambda t, r, c: min(t["alloc_lod0"], t["alloc_lod1"], t["alloc_lod2"], t["alloc_lod3"], t["band_new"], t["band_del"], t["band_fade"], t["band_beyond"], t["beyond_draw"]) >= 1
             and t["allocated"] == t["band_new"] == t["usable"]),
        Case("fade_band_usable", tiles=GRID13, view=CORNER, args=dict(smap_thresh_scale=4.0, shadow_map_sz=512), state=_state_all(0),
             check=lambda t, r, c: t["kept"] == t["band_new"] and t["cleared_far"] >= 10 and t["usable"] == t["band_new"] + t["band_del"] > t["band_new"] and t["not_usable_far"] == 0),
        # hysteresis: X holds LOD 0 and lod_level_f lies in (1, 1.1): no clear; above 1.1: cleared and allocated again at LOD 1
        Case("hysteresis_keeps", args=_scale_for(X, 1.05), state=_state_of({X: 0}),
             check=lambda t, r, c: t["hysteresis_kept"] >= 1 and not _word(r, c, X) & (sm.CLEARED_LOD_REDUCE | sm.ALLOCATED) and _word(r, c, X) & sm.RECEIVER and r["smap_state"][c.tiles.index(X)] == 0
             and (_word(r, c, X) >> 16) & 15 == 1 and (_word(r, c, X) >> 20) & 15 == 0),
        Case("hysteresis_clears", args=_scale_for(X, 1.15), state=_state_of({X: 0}),
             check=lambda t, r, c: _word(r, c, X) & sm.CLEARED_LOD_REDUCE and _word(r, c, X) & sm.ALLOCATED and r["smap_state"][c.tiles.index(X)] == 1),
        Case("lod_raise", args=dict(smap_thresh_scale=4.0), state=_state_all(3), check=lambda t, r, c: t["cleared_raise"] >= 5 and t["kept"] >= 1),
        Case("state_none", args=dict(smap_thresh_scale=2.0), state=_state_all(sm.NONE),
             check=lambda t, r, c: t["cleared_far"] + t["cleared_reduce"] + t["cleared_raise"] == 0 and t["allocated"] >= 5 and t["band_beyond"] >= 5),
        # a narrow frustum: the tiles beside and behind the camera are cleanup_only: they clear on reduce and never allocate
        Case("cleanup_only", view=NARROW, valid=1, args=dict(smap_thresh_scale=1.0), state=_state_all(0),
             check=lambda t, r, c: t["cleanup_cleared"] >= 3 and t["cleanup_only"] >= 20 and t["bounds_only"] == 0 and t["kept"] >= 1
             and all(not (w & sm.ALLOCATED) for w in r["plan"] if not (w & sm.UPDATE))),
        Case("bounds_by_trmax", view=NARROW, valid=1, arrays=_trmax(6.0), check=lambda t, r, c: t["bounds_only"] >= 1),
        Case("bounds_by_b_ext", view=NARROW, valid=1, args=dict(b_ext=(6.0, 5.0, 3.0)), check=lambda t, r, c: t["bounds_only"] >= 1),
        Case("bounds_by_road_len", view=NARROW, valid=1, args=dict(road_len=(12.0, 11.0)), check=lambda t, r, c: t["bounds_only"] >= 1),
        Case("models_valid", args=dict(models_valid=1, models_z2=30.0), check=lambda t, r, c: t["models"] >= 50 and all(b[5] == 30.0 for b in r["box"].values())),
        Case("shadow_map_sz_0", args=dict(shadow_map_sz=0), state=_state_of({(0, 0): 1}),
             check=lambda t, r, c: t["disabled"] >= 50 and t["allocated"] == 0 and t["usable"] == 0 and r["receivers"] == [] and len(r["box"]) >= 50),
        Case("shadow_map_sz_512", args=dict(shadow_map_sz=512, smap_thresh_scale=4.0), check=lambda t, r, c: t["allocated"] == t["alloc_lod0"] >= 9),
        Case("shadow_map_sz_8192", args=dict(shadow_map_sz=8192, smap_thresh_scale=4.0), state=_state_all(0),
             check=lambda t, r, c: t["large_inside"] == 1 and t["large_outside"] >= 8 and t["large_no_hysteresis"] >= 1 and t["cleared_reduce"] >= 1 and t["alloc_lod1"] >= 1
             and r["smap_state"][c.tiles.index((0, 0))] == 0),
        Case("have_buildings", args=dict(have_buildings=1, smap_thresh_scale=4.0), check=lambda t, r, c: t["alloc_lod2"] >= 1 and t["alloc_lod3"] == 0),
        Case("draw_model", args=dict(draw_model=1, smap_thresh_scale=4.0), state=_state_all(1),
             check=lambda t, r, c: t["cleared_wireframe"] >= 9 and t["allocated"] == 0 and not r["dist_scale"].any() and r["receivers"] == []),
        Case("absent_tiles", args=dict(smap_thresh_scale=4.0), arrays=_absent, state=_state_all(1), check=lambda t, r, c: t["absent"] >= 10 and t["present"] >= 40),
        Case("view_invalid", view=NARROW, valid=0, args=dict(smap_thresh_scale=4.0), check=lambda t, r, c: t["cleanup_only"] == 0 and t["invalid_view_tests"] >= 50),
        Case("shuffled_batch", tiles=_shuffle(GRID9, 5), args=dict(smap_thresh_scale=4.0), check=lambda t, r, c: len(r["receivers"]) >= 9 and r["receivers"] == sorted(r["receivers"])),
        # the recompute queue: flat tiles around a sun straight below tile (0, 0): ties in distance, broken by (y, x)
        Case("recomp_order_ties", kind=flat, args=dict(want_recomp=1, sun_pos=(0.0, 0.0, -50.0)), check=lambda t, r, c: t["recomp"] == 81 and t["recomp_dist_ties"] >= 40),
        Case("recomp_order_absent", tiles=_shuffle(GRID9, 9), args=dict(want_recomp=1, sun_pos=(-300.0, 120.0, 40.0)), arrays=_absent, check=lambda t, r, c: 40 <= t["recomp"] < 81),
        Case("terrain_flags_ored", args=dict(smap_thresh_scale=4.0), arrays=_all_arrays, dxoff=-5, dyoff=7, check=lambda t, r, c: t["flag_kept"] >= 5 and t["absent"] >= 1),
        Case("s128", S=128, args=dict(smap_thresh_scale=4.0, want_recomp=1, sun_pos=HIGH_SUN), arrays=_all_arrays, dxoff=3, dyoff=-2, check=lambda t, r, c: t["allocated"] >= 9),
        Case("n63", tiles=GRID9[:63], args=dict(smap_thresh_scale=6.0, want_recomp=1, sun_pos=LOW_SUN_X), check=lambda t, r, c: len(r["receivers"]) >= 50),
        Case("n64", tiles=GRID9[:64], args=dict(smap_thresh_scale=6.0, want_recomp=1, sun_pos=LOW_SUN_X), check=lambda t, r, c: len(r["receivers"]) >= 50),
        Case("n65", tiles=GRID9[:65], args=dict(smap_thresh_scale=6.0, want_recomp=1, sun_pos=LOW_SUN_X), check=lambda t, r, c: len(r["receivers"]) >= 50),
        Case("large_batch", tiles=BIG, args=dict(smap_thresh_scale=8.0, want_recomp=1, sun_pos=MOON_NEG_Y), state=_state_all(1),
             check=lambda t, r, c: len(r["receivers"]) > 256 and t["beyond_draw"] >= 100 and t["cleared_far"] >= 100 and t["recomp"] == 1600),
    ]
    return cs


def caster_cases():
    deep = lambda tx, ty: "deep" if (tx, ty) in ((1, 0), (-1, 1)) else "dry"  # noqa: E731
    sym = [((0, 1), LOW_SUN_X)]
    every = lambda tiles, lights: [(t, lights[i % len(lights)]) for i, t in enumerate(tiles)]  # noqa: E731
    cs = [
        Case("r1_grid3", tiles=GRID3, renders=[((0, 0), HIGH_SUN)], check=lambda t, r, c: t["in_to_draw"] >= 1 and t["terrain"] >= 1),
        # three lights; renders 0 and 3 share a receiver with different lights
        Case("r5_grid3", tiles=GRID3, renders=[((0, 0), HIGH_SUN), ((1, 0), LOW_SUN_X), ((-1, -1), MOON_NEG_Y), ((0, 0), MOON_NEG_Y), ((1, 1), HIGH_SUN)],
             check=lambda t, r, c: t["renders"] == 5 and r["terrain"][0] != r["terrain"][3] and min(len(x) for x in r["to_draw"]) >= 1),
        Case("fails_both", renders=[((0, 0), LOW_SUN_X), ((2, -1), MOON_NEG_Y), ((-1, 2), HIGH_SUN)], check=lambda t, r, c: t["fails_both"] >= 3 and t["not_visible"] >= 10 and t["nearer"] >= 3),
        Case("inc_adj_smap", renders=[((0, 0), LOW_SUN_X), ((2, -1), MOON_NEG_Y), ((-1, 2), HIGH_SUN)], cargs=dict(inc_adj_smap=1, b_ext=(6.0, 6.0, 2.0)),
             check=lambda t, r, c: t["overlap_only"] >= 2 and t["fails_both"] >= 1),
        # the light on the axis between (0, 1) and (0, -1): the two centres are equally far from it
        Case("at_recv_dist", renders=sym, light_valid=0, check=lambda t, r, c: t["at_recv_dist"] >= 1 and c.tiles.index((0, -1)) in r["terrain"][0] and t["invalid_view_tests"] >= 81),
        Case("invalid_light_view", tiles=GRID3, renders=every(GRID3[:4], [HIGH_SUN, MOON_NEG_Y]), light_valid=0,
             check=lambda t, r, c: all(len(x) == 9 for x in r["to_draw"]) and not r["not_drawn"].any()),
        Case("fully_in_city", tiles=GRID3, renders=[((0, 0), HIGH_SUN), ((1, 1), LOW_SUN_X)], light_valid=0,
             arrays=lambda case, n: dict(flags=np.array([8 if i % 3 == 1 else 0 for i in range(n)], np.uint8)), check=lambda t, r, c: t["in_city"] >= 2 and t["terrain"] >= 3),
        Case("decid_only_zero_counts", tiles=GRID3, renders=[((0, 0), HIGH_SUN), ((1, 0), MOON_NEG_Y)], cargs=dict(decid_trees_only=1), light_valid=0,
             arrays=lambda case, n: dict(decid_counts=np.zeros(n, np.uint32)), check=lambda t, r, c: t["no_decid"] == 18 and t["in_to_draw"] == 0 and r["not_drawn"].all()),
        Case("decid_only_some_counts", tiles=GRID3, renders=[((0, 0), HIGH_SUN), ((1, 0), MOON_NEG_Y)], cargs=dict(decid_trees_only=1), light_valid=0,
             arrays=lambda case, n: dict(decid_counts=np.array([0, 3, 0, 1, 0, 0, 7, 0, 2], np.uint32)), check=lambda t, r, c: t["no_decid"] == 10 and t["in_to_draw"] == 8 and t["terrain"] == 0),
        Case("receiver_absent_or_out_of_range", tiles=GRID3, renders=every([(0, 0)] * 5, [HIGH_SUN]), recv_raw=[4, 1, 9, 0xFFFFFFFF, 8],
             arrays=lambda case, n: dict(flags=np.array([0, 1, 0, 0, 0, 0, 0, 0, 0], np.uint8)), check=lambda t, r, c: t["no_tile"] == 3 and r["status"].tolist() == [0, 1, 1, 1, 0]),
        Case("all_water_tile", tiles=GRID3, kind=deep, renders=every([(0, 0), (1, 0), (-1, 1)], [LOW_SUN_X, HIGH_SUN]), check=lambda t, r, c: t["water_radius"] >= 3 and t["water_z2"] >= 3),
        Case("water_disabled", tiles=GRID3, kind=deep, renders=every([(0, 0), (1, 0), (-1, 1)], [LOW_SUN_X, HIGH_SUN]), cargs=dict(water_enabled=0), check=lambda t, r, c: t["water_radius"] == 0),
        Case("all_arrays", renders=every([(0, 0), (3, 1), (-2, -2)], [HIGH_SUN, LOW_SUN_X, MOON_NEG_Y]), arrays=_all_arrays, dxoff=-5, dyoff=7, cargs=dict(inc_adj_smap=1, road_len=(9.0, 3.0)),
             check=lambda t, r, c: t["in_to_draw"] >= 3),
        Case("s128", S=128, tiles=GRID3, renders=every(GRID3[:3], [HIGH_SUN, LOW_SUN_X, MOON_NEG_Y]), dxoff=3, dyoff=-2, check=lambda t, r, c: t["in_to_draw"] >= 3),
    ]
    for k in (63, 64, 65):  # an invalid and a valid view a render: survivors on both sides of the wave seam
        cs.append(Case("n%d" % k, tiles=GRID9[:k], renders=every([GRID9[0], GRID9[k - 1], GRID9[31]], [HIGH_SUN, MOON_NEG_Y]), light_valid=(1, 0, 0),
                       check=lambda t, r, c, k=k: len(r["to_draw"][1]) == k and 0 in r["to_draw"][2] and k - 1 in r["to_draw"][2] and any(0 < len(x) < k for x in r["terrain"])))
    cs.append(Case("large_batch_r7", tiles=BIG, renders=every([(0, 0), (-20, -20), (19, 19), (5, -7), (-13, 2), (0, 1), (10, 10)], [HIGH_SUN, LOW_SUN_X, MOON_NEG_Y]),
                   light_valid=(1, 1, 1, 0, 1, 0, 1), check=lambda t, r, c: len(r["to_draw"][3]) == 1600 and 0 < len(r["terrain"][3]) < 1600 and t["not_visible"] >= 1600 and t["in_to_draw"] >= 3200))
    return cs


MODEL = {}


def _setup(orc, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
    stats = wc.stats_of(orclib, case, float(sc.water_plane_z))
    v = view_model.make_view(**case.view)
    v.valid = case.valid
    n = len(case.tiles)
    arr = dict(trmax=None, tile_zmax=None, flags=None, terrain_flags=None, decid_counts=None)
    if case.arrays is not None:
        got = case.arrays(case, n)
        add = got.pop("tile_zmax_add", None)
        arr.update(got)
        if add is not None:
            arr["tile_zmax"] = np.array([f32(stats[t].mzmax) + add[t] for t in range(n)], f32)
    return sc, stats, v, arr


def plan_args_of(case, sc, stats, v):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]))
    kw.update(case.args(case, Ctx(sc, stats, v, case)) if callable(case.args) else case.args)
    return sm.PlanArgs(**kw)


def model(orc, case):
    """(scene, stats, view, args, arrays, state in, result, tally) of a plan case from the model, computed once"""
    key = "p:" + case.name
    if key not in MODEL:
        sc, stats, v, arr = _setup(orc, case)
        a = plan_args_of(case, sc, stats, v)
        n = len(case.tiles)
        state = case.state(case, n) if case.state else np.full(n, sm.NONE, np.uint8)
        tally = sm.new_tally()
        res = sm.plan(sc, v, a, case.tiles, stats, state, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"], terrain_flags=arr["terrain_flags"], tally=tally)
        MODEL[key] = (sc, stats, v, a, arr, state, res, tally)
    return MODEL[key]


def caster_model(orc, case):
    """(scene, stats, arrays, cast args, recv, views, bsm, lpos, result, tally) of a caster case: the light views are terra_make_light_view's model on the boxes of the
    model's plan of the same batch"""
    key = "c:" + case.name
    if key not in MODEL:
        sc, stats, v, arr = _setup(orc, case)
        a = sm.CastArgs(**case.cargs)
        pa = sm.PlanArgs(b_ext=a.b_ext, road_len=a.road_len)
        n = len(case.tiles)
        T = sm._tiles(sc, case.tiles, stats, arr["trmax"], arr["tile_zmax"], None)
        recv, views, bsm, lpos = [], [], [], []
        for r, (tile, lp) in enumerate(case.renders):
            i = case.tiles.index(tile)
            sb = sm.get_shadow_bcube(sc, pa, T[i])  # the box of the plan (without models)
            lv, m = sm.make_light_view(lp, [sb[0][0], sb[0][1], sb[1][0], sb[1][1], sb[2][0], sb[2][1]])
            lv.valid = case.light_valid[r] if isinstance(case.light_valid, tuple) else case.light_valid
            recv.append(i if case.recv_raw is None else case.recv_raw[r])
            views.append(lv)
            bsm.append(m)
            lpos.append(lp)
        tally = sm.new_tally()
        res = sm.casters(sc, a, case.tiles, stats, [x if x < 2 ** 31 else -1 for x in recv], views, bsm, lpos, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"],
                         decid_counts=arr["decid_counts"], tally=tally)
        MODEL[key] = (sc, stats, arr, a, np.array(recv, np.uint32), views, np.array(bsm, f32), np.array(lpos, f32).reshape(-1, 3), res, tally)
    return MODEL[key]


def lib_plan_args(pkg, a):
    return pkg.make_smap_plan_args(float(a.behind_sphere_mult), a.water_enabled, float(a.smap_thresh_scale), a.shadow_map_sz, a.have_buildings, a.draw_model, [float(x) for x in a.b_ext],
                                   [float(x) for x in a.road_len], float(a.models_z2), a.models_valid, [float(x) for x in a.sun_pos], a.want_recomp)


def lib_cast_args(pkg, a):
    return pkg.make_smap_cast_args(a.water_enabled, a.decid_trees_only, a.inc_adj_smap, [float(x) for x in a.b_ext], [float(x) for x in a.road_len])


def plan_fill(n, want_recomp_order=True):
    return dict(plan=np.full(n, FILL32, np.uint32), dist_scale=np.full(n, FILLF, f32), shadow_bcube=np.full((n, 6), FILLF, f32), receivers=np.full(n, FILL32, np.uint32),
                counts=np.full(2, 7, np.uint32), recomp_order=np.full(n, FILL32, np.uint32))


def cast_fill(n, R):
    return dict(to_draw=np.full((R, n), FILL32, np.uint32), terrain=np.full((R, n), FILL32, np.uint32), counts=np.full((R, 2), 7, np.uint32), not_drawn=np.full((R, n), FILL8, np.uint8),
                status=np.full(R, FILL8, np.uint8))


def compare_plan(what, got, want, state_in, terrain_flags_in, want_recomp):
    n = len(want["plan"])
    bad = np.argwhere(got["plan"] != want["plan"])
    assert len(bad) == 0, f"{what}: plan of tile {int(bad[0, 0])}: {int(got['plan'][bad[0, 0]]):#x} != {int(want['plan'][bad[0, 0]]):#x} ({len(bad)} differ)"
    bad = np.argwhere(got["dist_scale"].view(np.uint32) != want["dist_scale"].view(np.uint32))
    assert len(bad) == 0, f"{what}: dist_scale of tile {int(bad[0, 0])}: {got['dist_scale'][bad[0, 0]]!r} != {want['dist_scale'][bad[0, 0]]!r}"
    wb = np.full((n, 6), FILLF, f32)
    for t, b in want["box"].items():
        wb[t] = b
    bad = np.argwhere((got["shadow_bcube"].reshape(n, 6).view(np.uint32) != wb.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, f"{what}: shadow_bcube of tile {int(bad[0, 0])}: {got['shadow_bcube'].reshape(n, 6)[bad[0, 0]]} != {wb[bad[0, 0]]}"
    cn = got["counts"]
    nr = len(want["receivers"])
    assert int(cn[0]) == nr and got["receivers"][:nr].tolist() == want["receivers"], f"{what}: receivers {got['receivers'][:int(cn[0])].tolist()} != {want['receivers']}"
    assert (got["receivers"][nr:] == FILL32).all(), f"{what}: receivers past the count were written"
    assert got["smap_state"].tolist() == want["smap_state"].tolist(), f"{what}: smap_state {got['smap_state'].tolist()} != {want['smap_state'].tolist()}"
    assert (got["smap_state"][want["present"] == 0] == state_in[want["present"] == 0]).all()
    if terrain_flags_in is not None:
        assert got["terrain_flags"].tolist() == want["terrain_flags"].tolist(), f"{what}: terrain_flags differ"
    if want_recomp:
        no = len(want["recomp_order"])
        assert int(cn[1]) == no and got["recomp_order"][:no].tolist() == want["recomp_order"], f"{what}: recomp_order differs"
        assert (got["recomp_order"][no:] == FILL32).all(), f"{what}: recomp_order past the count was written"
    else:
        assert int(cn[1]) == 0 and (got["recomp_order"] == FILL32).all(), f"{what}: a recomp_order was written without want_recomp"


def compare_cast(what, got, want, n):
    R = len(want["to_draw"])
    assert got["status"].tolist() == want["status"].tolist(), f"{what}: status {got['status'].tolist()} != {want['status'].tolist()}"
    for r in range(R):
        for key, col in (("to_draw", 0), ("terrain", 1)):
            w = want[key][r]
            g = got[key].reshape(R, n)[r]
            assert int(got["counts"].reshape(R, 2)[r, col]) == len(w) and g[:len(w)].tolist() == w, f"{what}: {key} of render {r}: {g[:int(got['counts'].reshape(R, 2)[r, col])].tolist()} != {w}"
            assert (g[len(w):] == FILL32).all(), f"{what}: {key} of render {r} was written past its count"
    assert got["not_drawn"].reshape(R, n).tobytes() == want["not_drawn"].tobytes(), f"{what}: not_drawn differs at {np.argwhere(got['not_drawn'].reshape(R, n) != want['not_drawn'])[:4].tolist()}"


class DevBufs:
    """device arrays by name, freed together"""

    def __init__(self, t):
        self.t, self.b = t, {}

    def put(self, key, a):
        if a is not None:
            a = np.ascontiguousarray(a)
            self.b[key] = self.t.alloc(max(a.nbytes, 4)).upload(a.reshape(-1).view(np.uint8))
        return self

    def ptr(self, key):
        return self.b[key].ptr if key in self.b else None

    def get(self, key, dt, shape):
        return self.b[key].download(dt, shape).copy()

    def free(self):
        for x in self.b.values():
            x.free()


def run_plan_dev(pkg, t, case, stats, lv, la, arr, state):
    n = len(case.tiles)
    d = DevBufs(t)
    try:
        d.put("st", np.frombuffer(stats, np.uint8)).put("ss", state)
        for k, x in plan_fill(n).items():
            d.put(k, x)
        for k in ("trmax", "tile_zmax", "flags", "terrain_flags"):
            d.put(k, arr[k])
        t.tiles_smap_plan_dev(case.tiles, lv, la, d.ptr("st"), d.ptr("ss"), d.ptr("plan"), d.ptr("dist_scale"), d.ptr("shadow_bcube"), d.ptr("receivers"), d.ptr("counts"),
                              d.ptr("trmax"), d.ptr("tile_zmax"), d.ptr("flags"), d.ptr("terrain_flags"), d.ptr("recomp_order"), case.dxoff, case.dyoff)
        return dict(plan=d.get("plan", np.uint32, (n,)), dist_scale=d.get("dist_scale", f32, (n,)), shadow_bcube=d.get("shadow_bcube", f32, (n, 6)), receivers=d.get("receivers", np.uint32, (n,)),
                    counts=d.get("counts", np.uint32, (2,)), smap_state=d.get("ss", np.uint8, (n,)), recomp_order=d.get("recomp_order", np.uint32, (n,)),
                    terrain_flags=d.get("terrain_flags", np.uint8, (n,)) if arr["terrain_flags"] is not None else None)
    finally:
        d.free()


def run_plan_case(pkg, t, orc, case, dev=False):
    sc, stats, v, a, arr, state, res, tally = model(orc, case)
    assert case.check(tally, res, case), (case.name, {k: x for k, x in tally.items() if x})
    tc.configure(pkg, t, case)
    n = len(case.tiles)
    lstats = (pkg.TileStats * n).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), lib_plan_args(pkg, a)
    if dev:
        got = run_plan_dev(pkg, t, case, lstats, lv, la, arr, state)
    else:
        got = t.tiles_smap_plan(case.tiles, lstats, lv, la, state, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"], terrain_flags=arr["terrain_flags"],
                                want_recomp_order=True, dxoff=case.dxoff, dyoff=case.dyoff, fill=plan_fill(n))
    compare_plan(case.name + (" (dev)" if dev else ""), got, res, state, arr["terrain_flags"], a.want_recomp)


def run_cast_dev(pkg, t, case, stats, la, arr, recv, lviews, bsm, lpos):
    n, R = len(case.tiles), len(recv)
    d = DevBufs(t)
    try:
        d.put("st", np.frombuffer(stats, np.uint8)).put("recv", recv)
        for k, x in cast_fill(n, R).items():
            d.put(k, x)
        for k in ("trmax", "tile_zmax", "flags", "decid_counts"):
            d.put(k, arr[k])
        t.tiles_smap_casters_dev(case.tiles, d.ptr("recv"), lviews, bsm, lpos, la, d.ptr("st"), d.ptr("to_draw"), d.ptr("terrain"), d.ptr("counts"), d.ptr("not_drawn"), d.ptr("status"),
                                 d.ptr("trmax"), d.ptr("tile_zmax"), d.ptr("flags"), d.ptr("decid_counts"), case.dxoff, case.dyoff)
        return dict(to_draw=d.get("to_draw", np.uint32, (R, n)), terrain=d.get("terrain", np.uint32, (R, n)), counts=d.get("counts", np.uint32, (R, 2)),
                    not_drawn=d.get("not_drawn", np.uint8, (R, n)), status=d.get("status", np.uint8, (R,)))
    finally:
        d.free()


def run_cast_case(pkg, t, orc, case, dev=False):
    sc, stats, arr, a, recv, views, bsm, lpos, res, tally = caster_model(orc, case)
    assert case.check(tally, res, case), (case.name, {k: x for k, x in tally.items() if x})
    tc.configure(pkg, t, case)
    n, R = len(case.tiles), len(recv)
    lstats = (pkg.TileStats * n).from_buffer_copy(stats)
    la, lviews = lib_cast_args(pkg, a), [tc.lib_view(pkg, x) for x in views]
    if dev:
        got = run_cast_dev(pkg, t, case, lstats, la, arr, recv, lviews, bsm, lpos)
    else:
        got = t.tiles_smap_casters(case.tiles, lstats, recv, lviews, bsm, lpos, la, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"], decid_counts=arr["decid_counts"],
                                   dxoff=case.dxoff, dyoff=case.dyoff, fill=cast_fill(n, R))
    compare_cast(case.name + (" (dev)" if dev else ""), got, res, n)


# ---- terra_make_light_view: the lights of the cases on a tile's box, and degenerate ones
LIGHT_BOX = (-4.0, 4.0, -4.0, 4.0, 0.5, 1.1)
LIGHT_CASES = [
    ("high_sun", HIGH_SUN, LIGHT_BOX), ("low_sun_x", LOW_SUN_X, LIGHT_BOX), ("moon_neg_y", MOON_NEG_Y, LIGHT_BOX),
    ("offset_box", (-120.0, 33.0, 90.0), (36.0, 44.5, -20.0, -12.0, -3.0, 9.0)), ("straight_above", (0.0, 0.0, 150.0), (-4.0, 4.0, -4.0, 4.0, 0.0, 1.0)),
    ("flat_box_far_light", (2000.0, -900.0, 4000.0), (-4.0, 4.0, -4.0, 4.0, 0.25, 0.250002)), ("below_horizon", (40.0, 10.0, -60.0), LIGHT_BOX),
    ("along_y_axis", (0.0, 500.0, 0.08), (-4.0, 4.0, -4.0, 4.0, -0.2, 0.2)),
]
LIGHT_REFUSED = [("bounds_not_normalized", HIGH_SUN, (4.0, -4.0, -4.0, 4.0, 0.0, 1.0)), ("zero_height", HIGH_SUN, (-4.0, 4.0, -4.0, 4.0, 1.0, 1.0)),
                 ("light_in_centre", (0.0, 0.0, 0.05), (-4.0, 4.0, -4.0, 4.0, 0.0, 1.0))]


def check_light_views(pkg, t):
    for name, lp, box in LIGHT_CASES:
        want = sm.make_light_view(lp, box)
        assert want is not None, name
        lv, m = t.make_light_view(lp, box, 0.01)
        assert bytes(lv) == want[0].words(), f"{name}: the view differs: {np.frombuffer(bytes(lv), f32)} != {np.frombuffer(want[0].words(), f32)}"
        assert f32(m).tobytes() == f32(want[1]).tobytes(), f"{name}: behind_sphere_mult {m!r} != {want[1]!r}"
    for name, lp, box in LIGHT_REFUSED:
        assert sm.make_light_view(lp, box) is None, name
        v, m = pkg.View(), C.c_float(5.0)
        before = bytes(v)
        r = t.lib.terra_make_light_view((C.c_float * 3)(*lp), (C.c_float * 6)(*box), 0.01, C.byref(v), C.byref(m))
        assert r == ERR_ARG and bytes(v) == before and m.value == 5.0, name


# ---- the resident chain
CHAIN_TILES = [(x, y) for y in range(-1, 4) for x in range(1, 6)]  # of the default generated scene (water_view_cases.py)


def run_resident_chain(pkg, gpu, orc):
    """tiles_create_zvals_dev (zvals, stats) -> tiles_smap_plan_dev -> terra_make_light_view for each receiver on the host, from the plan's boxes -> tiles_smap_casters_dev
    (recv is the plan's receivers array, on the device) -> one shadow-pass tiles_tree_view_dev call with row 0 of not_drawn as its skip bytes, on a 5 x 5 batch at
    S = 128 on one context.  The boxes (with the receivers that name them) are the one read-back of the chain: the light views are made from them on the host.  Every
    stage is compared with the models, fed with the downloaded stats"""
    import tree_ao_model as tam
    import tree_view_cases as trc
    import tree_view_model as vm
    S, cap, cap_l = 128, 320, 2048
    tiles = CHAIN_TILES
    n, W, Z = len(tiles), S + 1, S + 2
    t = gpu
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_tree_size_params(pkg.make_tree_size_params())
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg)
    v = view_model.make_view((float(sc.g.get_xval(S + S // 2)), 0.3, 1.5), _unit(1.0, 0.3, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 60.0)
    pa = sm.PlanArgs(behind_sphere_mult=view_model.behind_sphere_mult(0.7, 1.6), smap_thresh_scale=2.0, want_recomp=1, sun_pos=HIGH_SUN)
    ca = sm.CastArgs()
    state_in = np.full(n, sm.NONE, np.uint8)
    state_in[:5] = 0
    out = pkg.Terra._tree_view_outputs(n, cap, trc.FILL)
    d = DevBufs(t)
    try:
        for k, b in dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * cap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4, tm=n * W * W * 2, trm=n * 4).items():
            d.put(k, np.zeros(b, np.uint8))
        d.put("ss", state_in).put("tf", np.zeros(n, np.uint8))
        for k, x in plan_fill(n).items():
            d.put(k, x)
        for k, x in cast_fill(n, n).items():
            d.put("c_" + k, x)
        for k, x in out.items():
            d.put("t_" + k, x)
        t.tiles_create_zvals_dev(tiles, 0, d.ptr("z"), d.ptr("st"))
        t.tiles_place_trees_dev(tiles, cap, d.ptr("pt"), d.ptr("pc"), 0, 0, None, d.ptr("st"))
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, d.ptr("tm"), d.ptr("pt"), d.ptr("pc"), cap, trmax_ptr=d.ptr("trm"))
        t.tiles_smap_plan_dev(tiles, tc.lib_view(pkg, v), lib_plan_args(pkg, pa), d.ptr("st"), d.ptr("ss"), d.ptr("plan"), d.ptr("dist_scale"), d.ptr("shadow_bcube"), d.ptr("receivers"),
                              d.ptr("counts"), trmax_ptr=d.ptr("trm"), terrain_flags_ptr=d.ptr("tf"), recomp_order_ptr=d.ptr("recomp_order"))
        # the one read-back of the chain: the boxes, and the receivers that say which of them get a light view
        boxes, recv, counts = d.get("shadow_bcube", f32, (n, 6)), d.get("receivers", np.uint32, (n,)), d.get("counts", np.uint32, (2,))
        R = int(counts[0])
        assert 2 <= R <= n
        lights = [t.make_light_view(HIGH_SUN, boxes[int(recv[r])]) for r in range(R)]
        lviews, bsm, lpos = [x[0] for x in lights], [x[1] for x in lights], [HIGH_SUN] * R
        t.tiles_smap_casters_dev(tiles, d.ptr("receivers"), lviews, bsm, lpos, lib_cast_args(pkg, ca), d.ptr("st"), d.ptr("c_to_draw"), d.ptr("c_terrain"), d.ptr("c_counts"),
                                 d.ptr("c_not_drawn"), d.ptr("c_status"), trmax_ptr=d.ptr("trm"))
        ta = vm.Args(bsm[0], 1.0, 1.0, 1920, shadow_pass=1)
        t.tiles_tree_view_dev(tiles, lviews[0], trc.lib_args(pkg, ta), d.ptr("st"), d.ptr("pt"), d.ptr("pc"), cap, *[d.ptr("t_" + k) for k in pkg.Terra.TREE_VIEW_OUTPUTS],
                              skip_ptr=d.ptr("c_not_drawn"), trmax_ptr=d.ptr("trm"))  # row 0 of not_drawn
        stats = (orclib.TileStats * n).from_buffer_copy(d.get("st", np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        pine = d.get("pt", np.uint8, (n * cap * pkg.TREE_PLACE_DTYPE.itemsize,)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap)
        pc, trm = d.get("pc", np.uint32, (n,)), d.get("trm", f32, (n,))
        got_plan = dict(plan=d.get("plan", np.uint32, (n,)), dist_scale=d.get("dist_scale", f32, (n,)), shadow_bcube=boxes, receivers=recv, counts=counts, smap_state=d.get("ss", np.uint8, (n,)),
                        recomp_order=d.get("recomp_order", np.uint32, (n,)), terrain_flags=d.get("tf", np.uint8, (n,)))
        got_cast = {k: d.get("c_" + k, x.dtype, x.shape)[:R] for k, x in cast_fill(n, n).items()}
        got_tree = {k: d.get("t_" + k, np.uint8, (x.nbytes,)).view(x.dtype).reshape(x.shape) for k, x in out.items()}
    finally:
        d.free()
    tally = sm.new_tally()
    want = sm.plan(sc, v, pa, tiles, stats, state_in, trmax=trm, terrain_flags=np.zeros(n, np.uint8), tally=tally)
    compare_plan("resident chain, plan", got_plan, want, state_in, np.zeros(n, np.uint8), 1)
    views = []
    for r in range(R):
        lv, m = sm.make_light_view(HIGH_SUN, want["box"][want["receivers"][r]])
        assert bytes(lviews[r]) == lv.words() and f32(bsm[r]).tobytes() == f32(m).tobytes(), f"resident chain, light view {r}"
        views.append(lv)
    wantc = sm.casters(sc, ca, tiles, stats, want["receivers"], views, bsm, lpos, trmax=trm, tally=tally)
    compare_cast("resident chain, casters", got_cast, wantc, n)
    wtally = vm.new_tally()
    wantt = vm.draw(sc, views[0], vm.Globals(tam.SizeParams(), ta), tiles, stats, pine, pc, wantc["not_drawn"][0], trm, None, 0, 0, wtally)
    trc.compare("resident chain, shadow-pass tree view", got_tree, wantt, pc, cap)
    assert tally["allocated"] >= 2 and tally["in_to_draw"] >= R and tally["not_visible"] >= 1 and int(pc.sum()) >= 100 and 1 <= wtally["skipped"] < n, (tally, wtally)
