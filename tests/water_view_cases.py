"""Cases of the reflection pass's terrain draw list (terra_tiles_reflection_view[_dev]) and of the water quads and water caps (terra_tiles_water_view[_dev]),
shared by test_water_view_emul.py (the host emulator) and test_gpu_water_view.py (HIP on the MI355X).  Every output is compared byte for byte with
tests/water_view_model.py; lists are compared in order up to their counts.

The cases live on the synthetic scene of terrain_view_cases.py: a tile is 8 wide at every S, tile (0, 0) spans [-4, 4]^2, the water plane lies at about -5.9.
A tile's kind gives its synthetic terra_tile_stats: "dry" (just above z = 0), "hill" (dry, up to z = 6), "lake" (down to two below the water plane, up to above
it: has_water), "pond" (one sub-box dips below the water plane: has_water), "deep" (all below the water plane: all_water), "wall" (the ridge of terrain_view_cases: an occluder), "flat" (mzmin == mzmax).  The water box of a
tile with water is the whole tile unless the case says otherwise.  The model's result of a case is computed once per process together with its tally, and every
case carries a check on that tally: that it exercises what it is named for."""
import ctypes as C
import math

import numpy as np

import orclib
import terrain_view_cases as tc
import terrain_view_model as tm
import view_model
import water_view_model as wm

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
grid, GRID9, ALONG_X, _unit = tc.grid, tc.GRID9, tc.ALONG_X, tc._unit
GRID11 = [(x, y) for y in range(-4, 5) for x in range(-4, 7)]
BIG = [(x, y) for y in range(-20, 20) for x in range(-20, 20)]
LOW = dict(pos=(0.3, 0.2, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
WIDE = dict(pos=(0.3, 0.2, 0.5), angle=1.2, aspect=1.5, near=0.05, far=400.0, **ALONG_X)
AWAY = dict(pos=(-17.0, -19.0, 1.0), angle=0.7, aspect=1.0, near=0.05, far=200.0, dir=_unit(-1.0, -0.9, 0.0), up=(0.0, 0.0, 1.0))
LODV = dict(pos=(-30.0, -28.0, 3.0), angle=1.0, aspect=1.0, near=0.05, far=400.0, dir=_unit(1.0, 1.0, -0.1), up=(0.0, 0.0, 1.0))


class Case:
    def __init__(self, name, S=16, tiles=GRID9, kind=None, terrain=None, view=LOW, valid=1, args=None, arrays=None, dxoff=0, dyoff=0, check=None, wbox=None, cam_z_water=False, radius=None):
        self.name, self.S, self.tiles, self.kind, self.terrain, self.valid = name, S, list(tiles), kind, terrain, valid
        self.view, self.args, self.arrays, self.dxoff, self.dyoff, self.check = dict(view), dict(args or {}), arrays, dxoff, dyoff, check
        self.wbox = wbox or {}           # (tx, ty) -> (wx1, wy1, wx2, wy2) in grid units from the tile's origin
        self.cam_z_water = cam_z_water   # the camera's z is water_plane_z
        self.radius = radius             # t -> the tile's radius instead of half the mesh box's diagonal


def stats_of(lib, case, wpz):
    """synthetic terra_tile_stats by kind; `terrain` names one of terrain_view_cases' fields instead (its tiles have no water box of their own: the whole tile)"""
    n, S = len(case.tiles), case.S
    if case.terrain is not None:
        stats = tc.stats_of(lib, tc.Case(case.name, S=S, tiles=case.tiles, terrain=case.terrain), wpz)
    else:
        stats = (lib.TileStats * n)()
        rng = np.random.default_rng(5)
        for t, (tx, ty) in enumerate(case.tiles):
            lo = 0.05 * rng.random(16) + 0.02 * (tx - ty) + 0.5
            hi = lo + 0.1 + 0.2 * rng.random(16)
            k = case.kind(tx, ty) if case.kind else "dry"
            if k == "hill":
                hi = hi + 5.0
            elif k == "lake":
                lo = lo * 0.0 + wpz - 2.0 + 0.05 * rng.random(16)
            elif k == "deep":
                lo, hi = lo * 0.0 + wpz - 2.0, hi * 0.0 + wpz - 1.0 - 0.2 * rng.random(16)
            elif k == "wall":
                lo, hi = lo + 6.0, hi + 6.0
                lo[0], hi[0] = -5.0, -4.8  # (one low column keeps the mesh box, which the centre segments must cross, down below the camera: still above the water plane)
            elif k == "pond":
                lo[5] = wpz - 0.5
            elif k == "flat":
                lo[:], hi[:] = 0.25, 0.25
            st = stats[t]
            for q in range(16):
                st.sub_zmin[q], st.sub_zmax[q] = float(f32(lo[q])), float(f32(hi[q]))
            st.mzmin, st.mzmax = min(st.sub_zmin), max(st.sub_zmax)
            st.radius = float(f32(case.radius(t) if case.radius else 0.5 * math.sqrt(8.0 ** 2 + 8.0 ** 2 + (st.mzmax - st.mzmin) ** 2)))
    for t, (tx, ty) in enumerate(case.tiles):
        st = stats[t]
        x1, y1 = tx * S, ty * S
        if (tx, ty) in case.wbox:
            b = case.wbox[(tx, ty)]
            st.wx1, st.wy1, st.wx2, st.wy2 = x1 + b[0], y1 + b[1], x1 + b[2], y1 + b[3]
        elif st.mzmin < wpz:
            st.wx1, st.wy1, st.wx2, st.wy2 = x1, y1, x1 + S, y1 + S
        else:
            st.wx1, st.wy1, st.wx2, st.wy2 = x1 + S, y1 + S, x1, y1  # denormalized (src/tiled_mesh.cpp:308)
    return stats


def _kinds(table, default="dry"):
    return lambda tx, ty: table.get((tx, ty), default)


def _wall(extra):
    d = {(1, -1): "wall", (1, 0): "wall", (1, 1): "wall"}
    d.update(extra)
    return _kinds(d)


def _reorder(tiles, first, then):
    """the same tiles with `first` moved to just before `then`"""
    out = [t for t in tiles if t != first]
    out.insert(out.index(then), first)
    return out


def _shuffled(tiles, seed, before, after):
    """a shuffle of the batch in which tile `before` precedes tile `after`"""
    rng = np.random.default_rng(seed)
    while True:
        out = [tiles[i] for i in rng.permutation(len(tiles))]
        if out.index(before) < out.index(after):
            return out


def _state(table):
    def f(case, n, ctx):
        st = np.zeros(n, np.uint8)
        for k, v in table.items():
            st[case.tiles.index(k)] = v
        return dict(occl_state=st)
    return f


def _flags(table):
    def f(case, n, ctx):
        fl = np.zeros(n, np.uint8)
        for k, v in table.items():
            fl[case.tiles.index(k)] = v
        return dict(flags=fl)
    return f


def _merge(*fs):
    def f(case, n, ctx):
        out = {}
        for g in fs:
            out.update(g(case, n, ctx))
        return out
    return f


def _lake_field(tx, ty):
    """lakes, deep water, hills and dry land in a pattern that gives every reflect value"""
    if (tx + 2 * ty) % 5 == 0:
        return "lake"
    if (tx - ty) % 7 == 3:
        return "deep"
    if (tx * ty) % 3 == 1:
        return "hill"
    return "dry"


def _rng_absent(case, n, ctx):
    rng = np.random.default_rng(23)
    return dict(flags=(rng.random(n) < 0.35).astype(np.uint8))


def _idx(case_tiles, xy):
    return case_tiles.index(xy)


A, B = (3, 1), (4, 1)  # the order-dependence pair: a lake tile behind the wall, the dry tile behind it


def reflection_cases():
    pair = _wall({A: "pond"})
    big_kind = lambda tx, ty: "dry" if (3 * tx + 7 * ty) % 5 == 0 else "lake"  # noqa: E731
    cs = [
        # every reflect value at least three times; value 1 from all_water here and from water disabled in the twin
        Case("reflect_values", kind=_lake_field, view=WIDE, valid=0, args=dict(check_occlusion=0),
             check=lambda t, r: min(t["refl_all_water"], t["refl_has_water"], t["refl_walk_found"], t["refl_walk_nothing"]) >= 3 and t["revisit"] == 0
             and min(t["found_x_only"], t["found_y_only"], t["found_turn3"]) >= 1 and min(t["cut_clip0"], t["cut_clip1"], t["cut_slope"]) >= 1
             and min(t["inside_one"], t["inside_both"]) >= 1 and t["no_reflection"] >= 3 and t["crack_to_dropped"] >= 1),
        Case("water_disabled", kind=_lake_field, view=WIDE, valid=0, args=dict(check_occlusion=0, water_enabled=0),
             check=lambda t, r: t["refl_disabled"] >= 3 and t["drawn"] == 0 and t["visits"] == 0),
        # the frustum: neighbours that fail is_visible(), water boxes that fail cube_visible
        Case("frustum_cuts", kind=_lake_field, view=WIDE, valid=1, args=dict(check_occlusion=0), wbox={xy: (0, 12, 3, 16) for xy in GRID9 if _lake_field(*xy) == "lake"},
             check=lambda t, r: min(t["cut_not_visible"], t["cut_cube"], t["refl_walk_found"]) >= 1 and t["revisit"] == 0),
        Case("absent_neighbours", kind=_lake_field, view=WIDE, valid=0, args=dict(check_occlusion=0), arrays=_rng_absent,
             check=lambda t, r: t["cut_absent"] >= 1 and t["absent"] >= 10 and t["revisit"] == 0),
        # the camera outside the batch: walks that end at the batch edge
        Case("camera_outside_batch", kind=_lake_field, view=dict(WIDE, pos=(-45.0, 3.0, 0.5)), valid=0, args=dict(check_occlusion=0),
             check=lambda t, r: t["cut_edge"] >= 1 and t["refl_walk_found"] >= 1 and t["revisit"] == 0),
        # order dependence: lake A = (3, 0) is found occluded by this call; dry B = (4, 0) has no other water on its walk
        Case("order_a_before_b", kind=pair, check=lambda t, r: r[0][_idx(GRID9, A)] & 7 == tm.OCCLUDED and r[7][_idx(GRID9, B)] == wm.WALK_NOTHING
             and r[0][_idx(GRID9, B)] & 7 == wm.NO_REFLECTION and t["written_on_walk"] >= 1 and t["cut_occluded"] >= 1),
        Case("order_b_before_a", kind=pair, tiles=_reorder(GRID9, B, A), check=lambda t, r: r[0][_idx(_reorder(GRID9, B, A), A)] & 7 == tm.OCCLUDED
             and r[7][_idx(_reorder(GRID9, B, A), B)] == wm.WALK_FOUND),
        Case("order_shuffled", kind=pair, tiles=_shuffled(GRID9, 3, B, A), check=lambda t, r: r[7][_idx(_shuffled(GRID9, 3, B, A), B)] == wm.WALK_FOUND
             and r[0][_idx(_shuffled(GRID9, 3, B, A), A)] & 7 == tm.OCCLUDED),
        Case("order_shuffled_a_first", kind=pair, tiles=_shuffled(GRID9, 4, A, B), check=lambda t, r: r[7][_idx(_shuffled(GRID9, 4, A, B), B)] == wm.WALK_NOTHING),
        # the chain: A is all_water, so its own answer at :2869 is no, so it is not tested, so it is not marked occluded, so B's walk finds its water
        Case("order_chain", kind=_wall({A: "deep"}), check=lambda t, r: r[0][_idx(GRID9, A)] & 7 == wm.NO_REFLECTION and r[7][_idx(GRID9, A)] == wm.NO_WATER
             and r[7][_idx(GRID9, B)] == wm.WALK_FOUND and r[6][_idx(GRID9, A)] == 0),
        # incoming state on lake tiles along a walk: 1 keeps the water test away, 2 keeps the occlusion test away
        Case("state_in_occluded", kind=pair, arrays=_state({A: 1}), check=lambda t, r: r[0][_idx(GRID9, A)] & 7 == tm.OCCLUDED_BEFORE
             and r[7][_idx(GRID9, B)] == wm.WALK_NOTHING and t["state1_on_walk"] >= 1),
        Case("state_in_unoccluded", kind=pair, arrays=_state({A: 2}), check=lambda t, r: r[0][_idx(GRID9, A)] & 7 == tm.DRAWN
             and r[7][_idx(GRID9, B)] == wm.WALK_FOUND and t["state2_on_walk"] >= 1 and t["test_skipped_state"] >= 1),
        Case("check_occlusion_off", kind=pair, args=dict(check_occlusion=0), check=lambda t, r: t["occluders"] == 0 and t["tested"] == 0 and r[7][_idx(GRID9, B)] == wm.WALK_FOUND),
        Case("no_occluder", kind=pair, arrays=lambda c, n, x: dict(flags=np.full(n, 2, np.uint8)), check=lambda t, r: t["occluders"] == 0 and t["refl_walk_found"] >= 1),
        # the division of :2643: the water box of the camera's tile ends right under the camera (inf), and the camera at the water plane's height on top of that (NaN)
        Case("closest_pt_under_camera", kind=_kinds({(0, 0): "lake"}), view=dict(WIDE, pos=(0.5, 0.2, 0.5)), valid=0, args=dict(check_occlusion=0), wbox={(0, 0): (2, 2, 9, 14)},
             check=lambda t, r: t["div_zero"] >= 1 and t["cut_slope"] >= 1),
        Case("camera_at_water_plane", kind=_kinds({(0, 0): "lake", (2, 1): "lake"}), view=dict(WIDE, pos=(0.5, 0.2, 0.5)), valid=0, args=dict(check_occlusion=0),
             wbox={(0, 0): (2, 2, 9, 14)}, cam_z_water=True, check=lambda t, r: t["div_zero"] >= 1 and t["cam_at_water"] >= 2 and t["refl_walk_found"] >= 1),
        # get_lod_level(1)
        Case("lod_pass1_s16", terrain="lods", view=LODV, arrays=tc._lod_arrays, check=lambda t, r: min(t["lod_low_detail"], t["lod_high_detail"]) >= 8 and t["lod_differs_pass2"] >= 1 and t["lod_flat"] >= 2),
        Case("lod_pass1_s32", S=32, terrain="lods", view=LODV, arrays=tc._lod_arrays, check=lambda t, r: min(t["lod_low_detail"], t["lod_high_detail"]) >= 8 and t["lod_differs_pass2"] >= 1 and t["lod_flat"] >= 2),
        Case("lod_pass1_s128", S=128, terrain="lods", view=LODV, arrays=tc._crack_arrays, dxoff=3, dyoff=-2,
             check=lambda t, r: min(t["lod_low_detail"], t["lod_high_detail"]) >= 8 and t["lod_differs_pass2"] >= 1 and t["lod_flat"] >= 2 and t["max_lod_not_flat"] == 4 and t["absent"] == 3),
        Case("all_arrays", kind=_lake_field, view=WIDE, valid=0, arrays=tc._all_arrays, dxoff=-5, dyoff=7, check=lambda t, r: t["drawn"] >= 5 and t["refl_walk_found"] >= 1),
        # 40 x 40: more than one workgroup of candidates, more drawn tiles than the ordering's first path holds, walks from 30 and more distances to the camera's tile
        Case("large_batch", tiles=BIG, kind=big_kind, view=dict(pos=(-55.3, 20.9, 30.0), angle=1.2, aspect=1.0, near=0.05, far=900.0, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)),
             valid=0, args=dict(check_occlusion=0), arrays=lambda c, n, x: dict(trmax=np.full(n, 0.25, f32)), radius=lambda t: 150.0 + 0.001 * t,
             check=lambda t, r: t["drawn"] > tc.ORDER_LDS_CAPACITY and len(t["walk_levels"]) >= 30 and t["drawn"] + t["no_reflection"] > 256 and t["revisit"] == 0),
    ]
    return cs


def water_cases():
    lakes = lambda tx, ty: "lake"  # noqa: E731
    return [
        Case("caps_masks", kind=lakes, view=WIDE, valid=0, args=dict(check_occlusion=0), arrays=_rng_absent,
             check=lambda t, r: len(set(r[1].tolist())) >= 10 and t["cap_adj_absent"] >= 1 and t["cap_adj_missing"] >= 1),
        Case("caps_occluded_dry", kind=_wall({A: "lake"}), check=lambda t, r: t["cap_occluded_dry"] >= 1 and t["cap_tiles"] >= 2),
        Case("caps_water_disabled", kind=_wall({A: "lake"}), args=dict(water_enabled=0), check=lambda t, r: t["cap_tiles"] == 0 and not r[1].any() and t["water_listed"] >= 1),
        Case("caps_distance", tiles=GRID11, kind=_lake_field, view=AWAY, valid=0, args=dict(check_occlusion=0),
             check=lambda t, r: min(t["cap_adj_near"], t["cap_adj_far"], t["water_far"], t["cap_tiles"]) >= 1),
        Case("water_frustum", tiles=GRID11, kind=_lake_field, view=AWAY, valid=1, check=lambda t, r: min(t["water_far"], t["water_not_visible"], t["water_listed"]) >= 1),
        Case("water_all_arrays", kind=_lake_field, view=WIDE, valid=0, arrays=tc._all_arrays, dxoff=-5, dyoff=7, check=lambda t, r: t["water_listed"] >= 5),
        Case("water_no_status", kind=_lake_field, view=WIDE, valid=1, args=dict(no_status=1), check=lambda t, r: r[1] is None and t["water_listed"] >= 1),
    ]


def view_of(case, wpz):
    kw = dict(case.view)
    if case.cam_z_water:
        kw["pos"] = (kw["pos"][0], kw["pos"][1], float(wpz))
    v = view_model.make_view(**kw)
    v.valid = case.valid
    return v


def args_of(case):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]), zmin=-8.0, zmax=45.0, water_enabled=1, check_occlusion=1, reflection_pass=1)
    kw.update({k: v for k, v in case.args.items() if k != "no_status"})
    return wm.Args(**kw)


def _arrays(case, sc, stats, v):
    n = len(case.tiles)
    a = dict(min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None)
    if case.arrays is not None:
        if "reflection_pass" not in case.args:
            case.args["reflection_pass"] = 1  # (tc._lod_arrays reads the threshold's pass from the case)
        got = case.arrays(case, n, tc.Ctx(sc, stats, v))
        add = got.pop("tile_zmax_add", None)
        a.update(got)
        if add is not None:
            a["tile_zmax"] = np.array([f32(stats[t].mzmax) + add[t] for t in range(n)], f32)
    return a


MODEL = {}


def _setup(orc, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
    stats = stats_of(orclib, case, float(sc.water_plane_z))
    v = view_of(case, sc.water_plane_z)
    return sc, stats, v, args_of(case), _arrays(case, sc, stats, v)


def model(orc, case):
    """(scene, stats, view, args, arrays, result, tally) of a reflection case from the model, computed once"""
    key = "r:" + case.name
    if key not in MODEL:
        sc, stats, v, a, arr = _setup(orc, case)
        tally = wm.new_tally()
        res = wm.draw(sc, v, a, case.tiles, stats, tally=tally, **arr)
        MODEL[key] = (sc, stats, v, a, arr, res, tally)
    return MODEL[key]


def water_model(orc, case):
    """(scene, stats, view, args, arrays, pass-0 status or None, (water_list, cap_mask), tally) of a water case from the models, computed once"""
    key = "w:" + case.name
    if key not in MODEL:
        sc, stats, v, a, arr = _setup(orc, case)
        status = None
        if not case.args.get("no_status"):
            a0 = tm.Args(a.behind_sphere_mult, a.occluder_zmin, a.water_enabled, a.check_occlusion, 0)
            status = tm.draw(sc, v, a0, case.tiles, stats, **arr)[0]
        tally = wm.new_tally()
        res = wm.water(sc, v, a, case.tiles, stats, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"], status=status, tally=tally)
        MODEL[key] = (sc, stats, v, a, arr, status, res, tally)
    return MODEL[key]


def lib_args(pkg, a):
    return pkg.make_reflection_view_args(float(a.behind_sphere_mult), float(a.zmin), float(a.zmax), a.water_enabled, a.check_occlusion, a.reflection_pass)


def lib_water_args(pkg, a):
    return pkg.make_water_view_args(float(a.behind_sphere_mult), a.water_enabled)


def compare(what, got, want, state_in):
    """(status, dist, lod, crack, order, occluded, counts, occl_state, reflect) against the model's (status, dist, lod, crack, order, occluded, occl_state, reflect)"""
    tc.compare(what, got[:8], want[:7], state_in)
    bad = np.argwhere(got[8] != want[7])
    assert len(bad) == 0, f"{what}: reflect of tile {int(bad[0, 0])}: {int(got[8][bad[0, 0]])} != {int(want[7][bad[0, 0]])} ({len(bad)} differ)"


def run_dev(pkg, t, tiles, stats, lv, la, arr, dxoff=0, dyoff=0):
    """the device-pointer form on freshly allocated buffers; the lists' tails must come back untouched"""
    n = len(tiles)
    bufs = dict(st=t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8)), su=t.alloc(n).upload(np.full(n, 0x77, np.uint8)), di=t.alloc(n * 4).upload(np.full(n, -1.0, f32)),
                lo=t.alloc(n).upload(np.full(n, 0x77, np.uint8)), cr=t.alloc(n * 4).upload(np.full(n * 4, 0x77, np.uint8)),
                dr=t.alloc(n * 4).upload(np.full(n, 0xABCDEF01, np.uint32)), oc=t.alloc(n * 4).upload(np.full(n, 0xABCDEF01, np.uint32)), cn=t.alloc(8).upload(np.full(2, 7, np.uint32)),
                nd=t.alloc(n).upload(np.full(n, 0x77, np.uint8)), rf=t.alloc(n).upload(np.full(n, 0x77, np.uint8)))
    for k, key, dt in (("mn", "min_normal_z", f32), ("tr", "trmax", f32), ("tz", "tile_zmax", f32), ("fl", "flags", np.uint8), ("os", "occl_state", np.uint8)):
        if arr[key] is not None:
            a = np.ascontiguousarray(arr[key], dt)
            bufs[k] = t.alloc(a.nbytes).upload(a)
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_reflection_view_dev(tiles, lv, la, bufs["st"].ptr, bufs["su"].ptr, bufs["di"].ptr, bufs["lo"].ptr, bufs["cr"].ptr, bufs["dr"].ptr, bufs["oc"].ptr, bufs["cn"].ptr,
                                    ptr("mn"), ptr("tr"), ptr("tz"), ptr("fl"), ptr("os"), bufs["nd"].ptr, bufs["rf"].ptr, dxoff, dyoff)
        counts = bufs["cn"].download(np.uint32, (2,)).copy()
        assert (bufs["nd"].download(np.uint8, (n,)) == ((bufs["su"].download(np.uint8, (n,)) & 7) != tm.DRAWN)).all(), "not_drawn is not (status != drawn)"
        order, occluded = bufs["dr"].download(np.uint32, (n,)).copy(), bufs["oc"].download(np.uint32, (n,)).copy()
        assert (order[counts[0]:] == 0xABCDEF01).all() and (occluded[counts[1]:] == 0xABCDEF01).all(), "entries past the counts were written"
        return (bufs["su"].download(np.uint8, (n,)).copy(), bufs["di"].download(f32, (n,)).copy(), bufs["lo"].download(np.uint8, (n,)).copy(),
                bufs["cr"].download(np.uint8, (n, 4)).copy(), order[:counts[0]], occluded[:counts[1]], counts,
                bufs["os"].download(np.uint8, (n,)).copy() if "os" in bufs else None, bufs["rf"].download(np.uint8, (n,)).copy())
    finally:
        for b in bufs.values():
            b.free()


def run_case(pkg, t, orc, case, dev=False):
    sc, stats, v, a, arr, res, tally = model(orc, case)
    assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})
    tc.configure(pkg, t, case)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), lib_args(pkg, a)
    if not dev:
        got = t.tiles_reflection_view(case.tiles, lstats, lv, la, dxoff=case.dxoff, dyoff=case.dyoff, **arr)
    else:
        got = run_dev(pkg, t, case.tiles, lstats, lv, la, arr, case.dxoff, case.dyoff)
    compare(case.name + (" (dev)" if dev else ""), got, res, arr["occl_state"])


def compare_water(what, got, want, n):
    wl, cm, counts = got
    w_wl, w_cm = want
    assert int(counts[0]) == len(w_wl) and wl.tolist() == list(w_wl), f"{what}: water list {wl.tolist()} ({int(counts[0])}) != {list(w_wl)}"
    if w_cm is None:
        assert cm is None
        return
    assert cm.tobytes() == w_cm.tobytes(), f"{what}: cap masks differ at {np.argwhere(cm != w_cm)[:4].tolist()}"
    assert int(counts[1]) == int((w_cm != 0).sum()), f"{what}: counts[1] {int(counts[1])} != {int((w_cm != 0).sum())}"


def run_water_dev(pkg, t, tiles, stats, lv, la, arr, status, dxoff=0, dyoff=0):
    n = len(tiles)
    bufs = dict(st=t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8)), wl=t.alloc(n * 4).upload(np.full(n, 0xABCDEF01, np.uint32)), cn=t.alloc(8).upload(np.full(2, 7, np.uint32)))
    if status is not None:
        bufs["su"], bufs["cm"] = t.alloc(n).upload(np.ascontiguousarray(status, np.uint8)), t.alloc(n).upload(np.full(n, 0x77, np.uint8))
    for k, key, dt in (("tr", "trmax", f32), ("tz", "tile_zmax", f32), ("fl", "flags", np.uint8)):
        if arr[key] is not None:
            a = np.ascontiguousarray(arr[key], dt)
            bufs[k] = t.alloc(a.nbytes).upload(a)
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_water_view_dev(tiles, lv, la, bufs["st"].ptr, bufs["wl"].ptr, bufs["cn"].ptr, ptr("su"), ptr("cm"), ptr("tr"), ptr("tz"), ptr("fl"), dxoff, dyoff)
        counts = bufs["cn"].download(np.uint32, (2,)).copy()
        wl = bufs["wl"].download(np.uint32, (n,)).copy()
        assert (wl[counts[0]:] == 0xABCDEF01).all(), "entries past the count were written"
        assert status is not None or counts[1] == 7, "counts[1] was written without a status"
        return wl[:counts[0]], (bufs["cm"].download(np.uint8, (n,)).copy() if status is not None else None), counts
    finally:
        for b in bufs.values():
            b.free()


def run_water_case(pkg, t, orc, case, dev=False):
    sc, stats, v, a, arr, status, res, tally = water_model(orc, case)
    assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})
    tc.configure(pkg, t, case)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), lib_water_args(pkg, a)
    if not dev:
        got = t.tiles_water_view(case.tiles, lstats, lv, la, trmax=arr["trmax"], tile_zmax=arr["tile_zmax"], flags=arr["flags"], status=status, dxoff=case.dxoff, dyoff=case.dyoff)
    else:
        got = run_water_dev(pkg, t, case.tiles, lstats, lv, la, arr, status, case.dxoff, case.dyoff)
    compare_water(case.name + (" (dev)" if dev else ""), got, res, len(case.tiles))


CHAIN_TILES = [(x, y) for y in range(-1, 4) for x in range(1, 6)]  # of the default generated scene: dry land in the south-west, the sea in the north-east


def run_resident_chain(pkg, gpu, orc):
    """tiles_create_zvals_dev (zvals, stats, normals, min_normal_z) -> tiles_reflection_view_dev -> tiles_terrain_view_dev (pass 0, on the occl_state the reflection
    pass left) -> tiles_water_view_dev (on the pass-0 status) on a 5 x 5 batch at S = 128 on one context with nothing read back in between, against the models fed
    with the downloaded stats.  The camera stands over the sea and looks back at the land: dry tiles see the water between them and the camera, or do not"""
    S = 128
    tiles = CHAIN_TILES
    n, Z, T = len(tiles), S + 2, S + 1
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gpu.init_scene(cfg)
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc, os_ = tm.Scene(orc, ocfg), orc.state()
    v = view_model.make_view((36.0, 20.0, 0.0), _unit(-1.0, -0.5, -0.1), (0.0, 0.0, 1.0), 0.9, 1.6, 0.05, 100.0)
    a = wm.Args(view_model.behind_sphere_mult(0.9, 1.6), float(os_.zmin), float(os_.zmax), 1, 1, 1)
    a0 = tm.Args(a.behind_sphere_mult, a.occluder_zmin, 1, 1, 0)
    lv = tc.lib_view(pkg, v)
    state = np.zeros(n, np.uint8)
    b = dict(os=gpu.alloc(n).upload(state), z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), nm=gpu.alloc(n * T * T * 4), mn=gpu.alloc(n * 4))
    for k in ("su", "lo", "nd", "rf", "su0", "lo0", "cm"):
        b[k] = gpu.alloc(n)
    for k in ("di", "cr", "dr", "oc", "di0", "cr0", "dr0", "oc0", "wl"):
        b[k] = gpu.alloc(n * 4)
    for k in ("cn", "cn0", "cnw"):
        b[k] = gpu.alloc(8)
    try:
        p = {k: x.ptr for k, x in b.items()}
        gpu.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"], p["nm"], p["mn"])
        gpu.tiles_reflection_view_dev(tiles, lv, lib_args(pkg, a), p["st"], p["su"], p["di"], p["lo"], p["cr"], p["dr"], p["oc"], p["cn"], min_normal_z_ptr=p["mn"], occl_state_ptr=p["os"],
                                      not_drawn_ptr=p["nd"], reflect_ptr=p["rf"])
        gpu.tiles_terrain_view_dev(tiles, lv, tc.lib_args(pkg, a0), p["st"], p["su0"], p["di0"], p["lo0"], p["cr0"], p["dr0"], p["oc0"], p["cn0"], min_normal_z_ptr=p["mn"],
                                   occl_state_ptr=p["os"])
        gpu.tiles_water_view_dev(tiles, lv, lib_water_args(pkg, a), p["st"], p["wl"], p["cnw"], status_ptr=p["su0"], cap_mask_ptr=p["cm"])
        dl = lambda k, dt, shape: b[k].download(dt, shape).copy()  # noqa: E731
        stats = (orclib.TileStats * n).from_buffer_copy(dl("st", np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        mnz = dl("mn", f32, (n,))
        cn, cn0, cnw = dl("cn", np.uint32, (2,)), dl("cn0", np.uint32, (2,)), dl("cnw", np.uint32, (2,))
        got = (dl("su", np.uint8, (n,)), dl("di", f32, (n,)), dl("lo", np.uint8, (n,)), dl("cr", np.uint8, (n, 4)), dl("dr", np.uint32, (n,))[:cn[0]], dl("oc", np.uint32, (n,))[:cn[1]], cn,
               None, dl("rf", np.uint8, (n,)))
        got0 = (dl("su0", np.uint8, (n,)), dl("di0", f32, (n,)), dl("lo0", np.uint8, (n,)), dl("cr0", np.uint8, (n, 4)), dl("dr0", np.uint32, (n,))[:cn0[0]],
                dl("oc0", np.uint32, (n,))[:cn0[1]], cn0, dl("os", np.uint8, (n,)))
        gotw = (dl("wl", np.uint32, (n,))[:cnw[0]], dl("cm", np.uint8, (n,)), cnw)
        nd = dl("nd", np.uint8, (n,))
    finally:
        for x in b.values():
            x.free()
    tally = wm.new_tally()
    want = wm.draw(sc, v, a, tiles, stats, min_normal_z=mnz, occl_state=state, tally=tally)
    compare("resident chain, reflection view", got, want, None)
    assert nd.tolist() == ((want[0] & 7) != tm.DRAWN).astype(np.uint8).tolist()
    want0 = tm.draw(sc, v, a0, tiles, stats, min_normal_z=mnz, occl_state=want[6])
    tc.compare("resident chain, terrain view behind the reflection view", got0, want0, want[6])
    wantw = wm.water(sc, v, a, tiles, stats, status=want0[0], tally=tally)
    compare_water("resident chain, water view", gotw, wantw, n)
    assert (want[7] == wm.WALK_FOUND).any() and ((want[0] & 7) == wm.NO_REFLECTION).any() and (wantw[1] != 0).any() and tally["revisit"] == 0, tally
