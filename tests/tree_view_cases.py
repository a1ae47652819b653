"""Cases of the pine and palm tree draw lists (terra_tiles_tree_view[_dev]) shared by test_tree_view_emul.py (the host emulator) and test_gpu_tree_view.py (HIP on
the MI355X).  Every output is compared byte for byte with tests/tree_view_model.py, all_bcube by value.

The view needs no placement, so the cases feed synthetic records on the synthetic scene of terrain_view_cases.py at S = 16: a tile is 8 wide, tile (0, 0) spans
[-4, 4]^2, get_scaled_tile_radius() is 48 and a flat tile's radius 5.66.  At tree_scale 1 get_tree_scale_denom() is 4.8, so get_tree_dist_scale() is
(d_xy - 5.66)/38.4 for a tile whose centre lies d_xy from the camera: polygon trunks and weight 1 below 44, the dithered band up to 50.5, trunk points up to 47.3.
The model's result of a case is computed once per process (MODEL) with its tally, and every case carries a check on that tally: that it reaches what it is named for."""
import ctypes as C

import numpy as np

import orclib
import terrain_view_cases as tvc
import terrain_view_model as tm
import tree_ao_model as tam
import tree_view_model as vm
import view_model

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
FILL = 0xA5
LDS_IDS = 1024  # the instance table that the kernel's histogram holds in LDS (TREE_VIEW_LDS_IDS, terra_treeview.hpp)
LDS_KEYS = 2048  # the capacity up to which the kernel ranks a tile's (key, record) pairs in LDS (TREE_VIEW_LDS_KEYS)
PINE, DECID, TDECID, BUSH, PALM, SH_PINE = range(6)
ALONG_X = dict(dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
LOW = dict(pos=(0.25, 0.25, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
RING = [(0, 0), (1, 0), (3, 0), (5, 0), (5, 3), (6, 0), (6, 1), (7, 0), (9, 0), (13, 0), (21, 0)]


class Case:
    def __init__(self, name, tiles, build, view=LOW, valid=1, args=None, instanced=False, ninst=(0, 0), tree_scale=1.0, dxoff=0, dyoff=0, xoff2=0, yoff2=0, cap=None, check=None):
        self.name, self.tiles, self.build, self.view, self.valid = name, list(tiles), build, dict(view), valid
        self.args, self.instanced, self.ninst, self.tree_scale = dict(args or {}), instanced, ninst, tree_scale
        self.dxoff, self.dyoff, self.xoff2, self.yoff2, self.check = dxoff, dyoff, xoff2, yoff2, check
        self.cap = cap  # the capacity, where it is not the builder's own
        self.S, self.terrain = 16, "flat"  # (what terrain_view_cases.stats_of reads)


class Records:
    """the inputs a case builds: records [n, cap], counts, and the optional skip, trmax and override arrays"""

    def __init__(self, n, cap):
        self.pine, self.counts = np.zeros((n, cap), tam_place_dtype()), np.zeros(n, np.uint32)
        self.skip = self.trmax = self.override = None
        self.cap = cap

    def add(self, t, pos, typ=PINE, inst=-1, height=0.5, width=0.15):
        j = int(self.counts[t])
        r = self.pine[t, j]
        r["pos"], r["type"], r["inst"], r["height"], r["width"] = pos, typ, inst, height, width
        self.counts[t] = j + 1
        return j


def tam_place_dtype():
    import importlib
    return importlib.import_module("3dworld_amd").TREE_PLACE_DTYPE


def tile_origin(case, t):
    tx, ty = case.tiles[t]
    return 8.0 * tx - 4.0 + 0.5 * (case.dxoff + 0), 8.0 * ty - 4.0 + 0.5 * case.dyoff  # DX_VAL = 0.5 at S = 16; positions are in the trees' own frame (before xlate)


def scatter(case, rec, t, m, rng, types=(PINE,), inst_of=None, z=0.1, hw=None):
    """m records spread over tile t, minus xlate so that they land in the tile once xlate is added"""
    ox, oy = tile_origin(case, t)
    xl = (0.5 * (case.dxoff + case.xoff2), 0.5 * (case.dyoff + case.yoff2))
    for k in range(m):
        typ = types[int(rng.integers(len(types)))]
        h = float(rng.uniform(0.32, 0.8)) if hw is None else hw[0]
        w = h * float(rng.uniform(0.25, 0.35)) if hw is None else hw[1]
        pos = (ox + float(rng.uniform(0.0, 8.0)) - xl[0], oy + float(rng.uniform(0.0, 8.0)) - xl[1], z + float(rng.uniform(0.0, 0.3)))
        rec.add(t, pos, typ, -1 if inst_of is None else inst_of(k, typ), h, w)


MIXED = (PINE, PINE, PINE, SH_PINE, PALM, BUSH)


def b_many(case, n):
    rec = Records(n, 300)
    rng = np.random.default_rng(1)
    for t, m in enumerate((300, 257, 300, 70)):
        scatter(case, rec, t, m, rng, MIXED)
    rec.counts[2] = 400  # above the capacity: the first 300 records
    return rec


def b_instanced(case, n):
    """300 and 257 records over more distinct ids than a wave has lanes; id 5 and id 140 shared by many records scattered through the tile"""
    rec = Records(n, case.cap or 300)
    rng = np.random.default_rng(2)
    npine, npalm = case.ninst

    def inst_of(k, typ):
        if typ == PALM:
            return npine + (k % 7 == 0) * 40 + (k * 13) % min(npalm, 90)
        return 5 if k % 6 == 0 else (k * 37) % min(npine, 97)
    for t, m in enumerate((300, 257, 120, 64)[:n]):
        scatter(case, rec, t, m, rng, (PINE, PINE, PINE, PALM), inst_of)
    return rec


def b_ring(case, n):
    rec = Records(n, 48)
    rng = np.random.default_rng(3)
    inst_of = None
    if case.instanced:
        npine, npalm = case.ninst
        inst_of = lambda k, typ: npine + k % npalm if typ == PALM else k % npine  # noqa: E731
    for t in range(n):
        scatter(case, rec, t, 40, rng, (PINE, PINE, PALM, SH_PINE) if t % 2 == 0 else (PINE, SH_PINE), inst_of)
    return rec


def b_camera_tile(case, n):
    """the camera's tile and a neighbour, pines that are not instanced: trunks of every class around the camera at (0.25, 0.25, 0.5), two pairs at equal distances"""
    rec = Records(n, case.cap or 160)
    rng = np.random.default_rng(4)
    for dx, dy in ((1.0, 0.5), (2.5, 1.0)):  # mirror images about the camera's axis, both ahead of it: equal p2p_dist_sq
        rec.add(0, (0.25 + dx, 0.25 + dy, 0.125), PINE)
        rec.add(0, (0.25 + dx, 0.25 - dy, 0.125), PINE)
    rec.add(0, (0.5, 0.25, 0.25), PINE, height=0.5, width=0.2)      # dist 0.35: nsides clamped at 32
    rec.add(0, (2.25, 0.75, 0.25), PINE, height=0.5, width=0.15)    # int(0.25*115.2/2.08) = 13
    rec.add(0, (3.75, -0.5, 0.25), PINE, height=0.5, width=0.03)    # size_scale 23, a thick cone: a cylinder with nsides clamped at 4
    rec.add(0, (3.0, 1.0, 0.25), PINE, height=0.4, width=0.002)     # size_scale 1.5 < dist: too small
    rec.add(0, (3.5, -1.5, 0.25), BUSH)
    rec.add(0, (3.5, 1.5, 0.25), PALM, height=0.4, width=0.12)
    scatter(case, rec, 0, 100, rng, (PINE, SH_PINE, PALM))
    scatter(case, rec, 1, 130, rng, (PINE, SH_PINE, PALM, BUSH))  # dist 4 .. 12: lines beyond 700*(r1 + r2)
    rec.override = np.zeros((n, rec.cap), override_dtype())
    for t in range(n):
        for j in range(int(rec.counts[t])):
            r = rec.pine[t, j]
            if r["type"] == PALM and j % 2 == 0:  # a tilted palm as setup_rotation would leave it; every fourth entry has rotated == 0 and is ignored
                o = rec.override[t, j]
                o["p1"] = (r["pos"][0], r["pos"][1], r["pos"][2] - 0.1)
                o["p2"] = (r["pos"][0] + 0.2, r["pos"][1] - 0.1, r["pos"][2] + 0.7)
                o["r1"], o["r2"], o["rotated"] = 0.02, 0.005, 0 if j % 4 == 0 else 7
    return rec


def override_dtype():
    import importlib
    return importlib.import_module("3dworld_amd").TRUNK_OVERRIDE_DTYPE


def b_frustum(case, n):
    """trees straddling every plane of a frustum with near 1 and far 30, and behind the camera inside and outside behind_sphere_mult's reach"""
    rec = Records(n, 200)
    rng = np.random.default_rng(5)
    cam = case.view["pos"]
    for t in range(n):
        scatter(case, rec, t, 60, rng, (PINE, PALM))
    t0, tfar = case.tiles.index((0, 0)), case.tiles.index((4, 0))
    for k in range(12):
        rec.add(t0, (cam[0] + 0.6 + 0.06 * k, cam[1] + 0.1, cam[2] - 0.25), PINE, height=0.5, width=0.15)   # the near plane at 1
        rec.add(t0, (cam[0] - 0.05 - 0.05 * k, cam[1], cam[2] - 0.25), PINE, height=0.5, width=0.15)          # behind the camera
        rec.add(tfar, (cam[0] + 29.4 + 0.1 * k, cam[1] - 0.2, cam[2] - 0.25), PINE, height=0.5, width=0.15)  # the far plane at 30
        rec.add(t0, (cam[0] + 3.0, cam[1] - 0.1, cam[2] + 1.35 + 0.09 * k), PINE, height=0.5, width=0.15)      # the upper plane: sin(0.6) of the distance above the axis
    return rec


def b_corner(case, n):
    """every tree of tile (2, 1) sits in its far corner, outside the frustum, while the tile's own sphere test passes"""
    rec = Records(n, 32)
    rng = np.random.default_rng(6)
    for t, (tx, ty) in enumerate(case.tiles):
        if (tx, ty) == (2, 1):
            for k in range(20):
                rec.add(t, (12.2 + 0.02 * k, 11.5 + 0.02 * k, 0.2), PINE if k % 3 else PALM)
        else:
            scatter(case, rec, t, 20, rng, (PINE, PALM))
    return rec


def b_dropped(case, n):
    """bad types, instances outside the table and instanced records while `instanced` is off amid good ones; a skipped tile, an empty one, one with only bad records"""
    rec = Records(n, 64)
    rng = np.random.default_rng(7)
    for t in range(n):
        scatter(case, rec, t, 40, rng, MIXED)
    for t in range(n):
        for j in range(0, 40, 5):
            rec.pine[t, j]["type"] = (9, -2, 6)[(j // 5) % 3]
        for j in range(2, 40, 7):
            rec.pine[t, j]["inst"] = 3 if not case.instanced else 5000
    rec.counts[2] = 0
    rec.pine[3, :int(rec.counts[3])]["type"] = 17
    rec.skip = np.zeros(n, np.uint8)
    rec.skip[1] = 1
    rec.trmax = np.linspace(0.0, 0.6, n).astype(f32)
    return rec


def inst_table(npine, npalm):
    rng = np.random.default_rng(9)
    t = np.zeros(npine + npalm, tam.INST_DTYPE)
    for i in range(npine + npalm):
        h = float(rng.uniform(0.4, 1.0))
        t[i] = ((SH_PINE if i % 10 == 3 else PINE) if i < npine else PALM, h * (1.2 if i < npine else 2.0), h * float(rng.uniform(0.25, 0.35)))
    return t


def cases():
    narrow = dict(LOW, angle=0.3)
    clipped = dict(LOW, pos=(0.25, 0.25, 0.5), near=1.0, far=30.0)
    outside = dict(LOW, pos=(-30.0, 0.25, 0.5))
    return [
        Case("many_records", [(0, 0), (1, 0), (2, 0), (3, 3)], b_many,
             check=lambda t, r: t["sorted_lists"] == 1 and len(r[0].leaf_pine) > 64 and t["pine_list"] >= 1 and t["palm_list_entries"] >= 10 and t["byte_bush"] >= 10),
        Case("instanced_many_ids", [(0, 0), (1, 0), (2, 0), (3, 3)], b_instanced, instanced=True, ninst=(100, 100),
             check=lambda t, r: t["max_ids_in_tile"] > 64 and t["max_share_of_id"] >= 30 and t["inst_sh_pine"] >= 5 and t["palm_insts"] >= 20 and t["near_not_all"] >= 1
             and t["draw_all_near"] >= 1),
        Case("instanced_big_table", [(0, 0), (1, 0)], b_instanced, instanced=True, ninst=(700, 700),
             check=lambda t, r: t["max_ids_in_tile"] > 64 and t["pine_insts"] >= 100 and t["palm_insts"] >= 20),
        Case("lod_ring", RING, b_ring, check=lambda t, r: min(t["trunk_poly_all"] + t["trunk_poly_skipped"], t["trunk_poly_skipped"], t["trunk_points"], t["trunk_none"], t["weight0"],
                                                               t["weight_mid"], t["weight1"], t["palms_yes"], t["palms_no"], t["render_all"]) >= 1 and t["contains_camera"] == 1),
        Case("lod_ring_instanced", RING, b_ring, instanced=True, ninst=(30, 20),
             check=lambda t, r: min(t["palms_inst_clause"], t["palms_inst_clause_fails"], t["weight0"], t["weight_mid"], t["weight1"]) >= 1),
        Case("lod_ring_shadow_pass", RING, b_ring, args=dict(shadow_pass=1), check=lambda t, r: t["nsides_shadow"] >= 50 and t["weight1"] == len(RING) and t["trunk_points"] == 0),
        Case("lod_ring_far_leaves_only", RING, b_ring, args=dict(draw_trunks=0, draw_near_leaves=0), check=lambda t, r: t["render_all"] >= 2 and t["palms_yes"] == 0 and t["pine_list"] == 0),
        Case("lod_ring_near_leaves_only", RING, b_ring, tree_scale=0.8, args=dict(draw_trunks=0, draw_far_leaves=0), check=lambda t, r: t["palms_yes"] >= 1 and t["trunk_none"] == 0),
        Case("camera_tile", [(0, 0), (1, 0)], b_camera_tile,
             check=lambda t, r: t["sorted_lists"] == 1 and t["sorted_ties"] >= 2 and min(t["byte_small"], t["byte_line"], t["nsides_4_clamped"], t["nsides_32_clamped"],
                                                                                      t["nsides_between"], t["byte_bush"], t["rotated"], t["rotated_ignored"]) >= 1),
        # a capacity beyond what the kernel ranks in LDS: the camera tile's pairs and the big table's pairs lie in global scratch
        Case("camera_tile_large_capacity", [(0, 0), (1, 0)], b_camera_tile, cap=LDS_KEYS + 52, check=lambda t, r: t["sorted_lists"] == 1 and t["sorted_ties"] >= 2 and len(r[0].leaf_pine) >= 30),
        Case("instanced_big_table_large_capacity", [(0, 0), (1, 0)], b_instanced, instanced=True, ninst=(700, 700), cap=LDS_KEYS + 52,
             check=lambda t, r: t["max_ids_in_tile"] > 64 and t["pine_insts"] >= 100 and t["palm_insts"] >= 20),
        Case("camera_outside", [(0, 0), (1, 0), (2, 0)], b_ring, view=outside, check=lambda t, r: t["contains_camera"] == 0 and t["sorted_lists"] == 0),
        Case("frustum_planes", [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (1, -1)], b_frustum, view=clipped,
             check=lambda t, r: min(t["up_straddle"], t["side_straddle"], t["near_straddle"], t["far_straddle"], t["behind_true"], t["behind_false"], t["up_reject"], t["side_reject"],
                                    t["near_reject"], t["far_reject"]) >= 1),
        Case("view_invalid", [(0, 0), (1, 0), (-2, 0)], b_ring, valid=0, check=lambda t, r: t["invalid_view_tests"] >= 3 and t["leaves_hidden"] == 0),
        Case("trees_in_corner", [(2, 1), (1, 0), (2, 0)], b_corner, view=narrow, check=lambda t, r: t["lists_culled_centre_visible"] >= 1 and t["trunks_culled"] >= 1),
        Case("dropped_skip_empty", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)], b_dropped, dxoff=3, dyoff=-2, xoff2=-5, yoff2=4,
             check=lambda t, r: t["dropped"] >= 40 and t["skipped"] == 1 and t["empty"] == 2),
        Case("dropped_instanced", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)], b_dropped, instanced=True, ninst=(8, 8), dxoff=-7, xoff2=2,
             check=lambda t, r: t["dropped"] >= 40 and t["skipped"] == 1 and t["empty"] == 2),
    ]


def view_of(case):
    return tvc.view_of(case)


def args_of(case):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]), zoom_f=1.0, tree_depth_scale=1.0, window_width=1920)
    kw.update(case.args)
    return vm.Args(**kw)


MODEL = {}


def model(orc, case):
    """(scene, stats, view, globals, records, results, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
        orc.init(ocfg)
        sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
        stats, v = tvc.stats_of(orclib, case, float(sc.water_plane_z)), view_of(case)
        insts = inst_table(*case.ninst) if case.instanced else None
        g = vm.Globals(tam.SizeParams(tree_scale=case.tree_scale), args_of(case), case.instanced, insts)
        rec = case.build(case, len(case.tiles))
        tally = vm.new_tally()
        res = vm.draw(sc, v, g, case.tiles, stats, rec.pine, rec.counts, rec.skip, rec.trmax, rec.override, case.xoff2, case.yoff2, tally)
        MODEL[case.name] = (sc, stats, v, g, rec, res, tally)
    return MODEL[case.name]


def lib_args(pkg, a):
    return pkg.make_tree_view_args(float(a.behind_sphere_mult), float(a.zoom_f), float(a.tree_depth_scale), a.window_width, a.shadow_pass, a.draw_trunks, a.draw_near_leaves,
                                   a.draw_far_leaves)


def configure(pkg, t, case, g):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_scale=case.tree_scale, instanced=case.instanced, num_pine_insts=case.ninst[0], num_palm_insts=case.ninst[1]))
    t.set_tree_size_params(pkg.make_tree_size_params())
    t.set_tree_instances(g.insts)


def compare(what, got, want, counts, cap):
    """the library's dict of arrays (allocated with the byte FILL) against the model's [TileResult]"""
    fill32 = np.frombuffer(bytes([FILL]) * 4, np.uint32)[0]
    for t, w in enumerate(want):
        tag = f"{what}, tile {t}"
        tile = got["tile"][t]
        assert (int(tile["flags"]), int(tile["num_pine"]), int(tile["num_palm"]), int(tile["num_trees"]), int(tile["pad"])) == (w.flags, w.num_pine, w.num_palm, w.num_trees, 0), \
            f"{tag}: flags {int(tile['flags']):#x} != {w.flags:#x} or counts {tile} != {(w.num_pine, w.num_palm, w.num_trees)}"
        assert f32(tile["dscale"]).tobytes() == f32(w.dscale).tobytes() and f32(tile["weight"]).tobytes() == f32(w.weight).tobytes(), f"{tag}: dscale / weight {tile} != {w.dscale!r}, {w.weight!r}"
        assert (got["all_bcube"][t] == np.array(w.bcube, f32)).all(), f"{tag}: all_bcube {got['all_bcube'][t].tolist()} != {[float(x) for x in w.bcube]}"
        for key, lst in (("pine_insts", w.pine_insts), ("palm_insts", w.palm_insts)):
            k = 0 if key == "pine_insts" else 1
            assert int(got["inst_counts"][t, k]) == len(lst), f"{tag}: {key} count {int(got['inst_counts'][t, k])} != {len(lst)}"
            arr = got[key][t]
            want_arr = np.zeros(len(lst), arr.dtype)
            for i, (iid, pos) in enumerate(lst):
                want_arr[i] = (iid, pos)
            assert arr[:len(lst)].tobytes() == want_arr.tobytes(), f"{tag}: {key} differ, first at {next(i for i in range(len(lst)) if arr[i].tobytes() != want_arr[i].tobytes())}"
            assert (arr[len(lst):].view(np.uint8) == FILL).all(), f"{tag}: {key} written past the count"
        written = (w.leaf_pine or []) + w.leaf_palm
        assert got["leaf_counts"][t].tolist() == [w.leaf_count_pine, len(w.leaf_palm)], f"{tag}: leaf_counts {got['leaf_counts'][t].tolist()} != {[w.leaf_count_pine, len(w.leaf_palm)]}"
        assert int(tile["leaf_written"]) == len(written) and got["leaf_list"][t, :len(written)].tolist() == written, f"{tag}: leaf_list differs ({int(tile['leaf_written'])} written, {len(written)} wanted)"
        assert (got["leaf_list"][t, len(written):] == fill32).all(), f"{tag}: leaf_list written past the count"
        m = min(int(counts[t]), cap) if w.written else 0
        assert got["trunk"][t, :m].tolist() == (w.trunk or []), f"{tag}: trunk bytes differ at {[i for i in range(m) if got['trunk'][t, i] != w.trunk[i]][:6]}"
        assert (got["trunk"][t, m:] == FILL).all(), f"{tag}: trunk bytes written past the count"


def run_dev(pkg, t, tiles, stats, lv, la, rec, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
    """the device-pointer form on freshly allocated buffers filled with FILL -> what Terra.tiles_tree_view returns"""
    n, cap = rec.pine.shape
    out = pkg.Terra._tree_view_outputs(n, cap, FILL)
    bufs = {k: t.alloc(max(a.nbytes, 4)).upload(a.view(np.uint8).reshape(-1)) for k, a in out.items() if a.nbytes}
    bufs["st"] = t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8))
    bufs["pt"] = t.alloc(max(rec.pine.nbytes, 4)).upload(rec.pine.view(np.uint8).reshape(-1))
    bufs["pc"] = t.alloc(n * 4).upload(rec.counts)
    for k, a in (("sk", rec.skip), ("tr", rec.trmax), ("ov", rec.override)):
        if a is not None:
            bufs[k] = t.alloc(a.nbytes).upload(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_tree_view_dev(tiles, lv, la, bufs["st"].ptr, bufs["pt"].ptr, bufs["pc"].ptr, cap, *[ptr(k) for k in pkg.Terra.TREE_VIEW_OUTPUTS], skip_ptr=ptr("sk"), trmax_ptr=ptr("tr"),
                              trunk_override_ptr=ptr("ov"), dxoff=dxoff, dyoff=dyoff, xoff2=xoff2, yoff2=yoff2)
        return {k: bufs[k].download(np.uint8, (a.nbytes,)).copy().view(a.dtype).reshape(a.shape) for k, a in out.items()}
    finally:
        for b in bufs.values():
            b.free()


def run_case(pkg, t, orc, case, dev=False):
    sc, stats, v, g, rec, res, tally = model(orc, case)
    assert case.check(tally, res), (case.name, tally)
    configure(pkg, t, case, g)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv, la = tvc.lib_view(pkg, v), lib_args(pkg, g.a)
    kw = dict(dxoff=case.dxoff, dyoff=case.dyoff, xoff2=case.xoff2, yoff2=case.yoff2)
    if not dev:
        got = t.tiles_tree_view(case.tiles, lstats, lv, la, rec.pine, rec.counts, rec.skip, rec.trmax, rec.override, fill=FILL, **kw)
    else:
        got = run_dev(pkg, t, case.tiles, lstats, lv, la, rec, **kw)
    compare(case.name + (" (dev)" if dev else ""), got, res, rec.counts, rec.cap)


def run_resident_chain(pkg, t, orc):
    """tiles_create_zvals_dev (zvals, stats) -> tiles_place_trees_dev -> tiles_tree_ao_shadows_dev (trmax) -> tiles_terrain_view_dev (not_drawn) -> tiles_tree_view_dev
    with not_drawn as its skip bytes, on a 3 x 3 batch at S = 128 on one context with nothing read back in between; the model is fed from the read-back records"""
    S, cap, cap_l = 128, 320, 2048
    tiles = [(x, y) for y in range(-1, 2) for x in range(1, 4)]  # over the island's shore: pines and palms
    n, W, Z = len(tiles), S + 1, S + 2
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_tree_size_params(pkg.make_tree_size_params())
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg)
    v = view_model.make_view((float(sc.g.get_xval(S + S // 2)), 0.3, 1.5), tvc._unit(1.0, 0.3, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 60.0)
    bsm = view_model.behind_sphere_mult(0.7, 1.6)
    ta, a = tm.Args(bsm, float(orc.state().zmin), 1, 0, 0), vm.Args(bsm, 1.0, 1.0, 1920)
    lv, lta, la = tvc.lib_view(pkg, v), tvc.lib_args(pkg, ta), lib_args(pkg, a)
    out = pkg.Terra._tree_view_outputs(n, cap, FILL)
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * cap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4, tm=n * W * W * 2, trm=n * 4, su=n, di=n * 4, lo=n, cr=n * 4,
                 dr=n * 4, oc=n * 4, cn=8, nd=n)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    bufs.update({k: t.alloc(x.nbytes).upload(x.view(np.uint8).reshape(-1)) for k, x in out.items()})
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        bufs["pt"].upload(np.zeros(sizes["pt"], np.uint8))
        t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        t.tiles_place_trees_dev(tiles, cap, p["pt"], p["pc"], 0, 0, None, p["st"])
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, p["tm"], p["pt"], p["pc"], cap, trmax_ptr=p["trm"])
        t.tiles_terrain_view_dev(tiles, lv, lta, p["st"], p["su"], p["di"], p["lo"], p["cr"], p["dr"], p["oc"], p["cn"], trmax_ptr=p["trm"], not_drawn_ptr=p["nd"])
        t.tiles_tree_view_dev(tiles, lv, la, p["st"], p["pt"], p["pc"], cap, *[p[k] for k in pkg.Terra.TREE_VIEW_OUTPUTS], skip_ptr=p["nd"], trmax_ptr=p["trm"])
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
        pine = bufs["pt"].download(np.uint8, (sizes["pt"],)).copy().view(pkg.TREE_PLACE_DTYPE).reshape(n, cap)
        pc, trm, nd = bufs["pc"].download(np.uint32, (n,)).copy(), bufs["trm"].download(f32, (n,)).copy(), bufs["nd"].download(np.uint8, (n,)).copy()
        got = {k: bufs[k].download(np.uint8, (x.nbytes,)).copy().view(x.dtype).reshape(x.shape) for k, x in out.items()}
    finally:
        for b in bufs.values():
            b.free()
    tally = vm.new_tally()
    want = vm.draw(sc, v, vm.Globals(tam.SizeParams(), a), tiles, stats, pine, pc, nd, trm, None, 0, 0, tally)
    compare("resident chain", got, want, pc, cap)
    assert int(pc.sum()) >= 100 and 1 <= tally["skipped"] < n and tally["trunk_poly_all"] + tally["trunk_poly_skipped"] >= 2 and tally["pine_list"] >= 1 and tally["render_all"] >= 2 and tally["byte_line"] >= 20, (tally, pc.tolist(), nd.tolist())
    return tally
