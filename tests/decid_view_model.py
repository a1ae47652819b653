"""NumPy / Python float32 restatement of the deciduous tree draw lists of a tile batch for a camera, written from the reference statements (not from the library's
bodies):

    tile_t::draw_decid_trees (without its GL and shader calls)                  src/tiled_mesh.cpp:1555-1563
    the two sweeps of tile_draw_t::draw_decid_trees, enable_billboards         src/tiled_mesh.cpp:3262-3292
    tree_cont_t::draw_branches_and_leaves                                      src/Tree.cpp:312-368
    tree::draw_leaves_top, tree::draw_branches_top                             src/Tree.cpp:993-1052, 948-990
    tree::is_visible_to_camera, add_bounds_to_bcube, calc_size_scale           src/Tree.cpp:858-865, 919-928
    tree_data_t::get_size_scale_mult, draw_branches, draw_leaves (the counts)  src/Tree.cpp:930, 1128-1140, 1182-1188
    tree_cont_t::calc_bcube                                                    src/Tree.cpp:2458-2461
    get_draw_tile_dist, get_scaled_tile_radius                                 src/tiled_mesh.cpp:117, src/tiled_mesh.h:93-94
    cube_t's helpers                                                           src/3DWorld.h:491-527, 602; src/csg.cpp:247

The view tests (cube_visible, cube_visible_likely, sphere_visible_test with its tally of the planes), closest_pt, InvSqrt and unsigned(double) are
tests/view_model.py's.  Types: np.float32 for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are double: 1.1*sphere_radius
(narrowed to the float parameter), 1.0*(X_SCENE_SIZE + Y_SCENE_SIZE) (narrowed likewise), 1.5*num_branch_quads*size_scale*mult and 4.0*nl*size_scale*mult,
(1.0 - geom_opacity) (narrowed), and the comparisons of size_scale and geom_opacity with 0.0, 0.05 and 2.0.  unsigned(double) converts like x86-64: cvttsd2si to 64
bits and the low word, 0 beyond the 64-bit range.  Tiled-terrain mode: sphere_in_camera_view is sphere_visible_test alone (src/visibility.cpp:338-339).

The billboard lists are sorted by tree_id and keep, within an id, the order in which the reference adds the entries: its own sort looks at the id alone.

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import numpy as np

import tree_ao_model as tam
import view_model

f32 = np.float32
ZERO, ONE, HALF = f32(0.0), f32(1.0), f32(0.5)
DIST_C_SCALE, LEAF_4TH_SCALE, DRAW_DIST_TILES = f32(0.01), f32(0.4), f32(1.5)
GENERATED, HAS_4TH, LEAF_TEX, BRANCH_TEX = 1, 2, 4, 8
TILE_DRAWN, TILE_LEAVES, TILE_BRANCHES, TILE_SORTED, TILE_BCUBE_ZERO_AREA = 1, 2, 4, 8, 16
FORM_NONE, FORM_GEOM, FORM_BOTH, FORM_BILLBOARD, NOT_VISIBLE, LOW_DETAIL, STAGE_SHIFT = 0, 1, 2, 3, 4, 8, 4
ST_NONE, ST_NOT_VISIBLE, ST_NO_LEAVES, ST_BOX, ST_SIZE, ST_SHADOW_DIST, ST_SHADOW_SPHERE = range(7)
cmax, cmin, d2u, inv_sqrt, cube_visible_likely = view_model.cmax, view_model.cmin, view_model.d2u, view_model.inv_sqrt, view_model.cube_visible_likely

TD_DTYPE = np.dtype([("base_radius", f32), ("sphere_radius", f32), ("sphere_center_zoff", f32), ("lr_z_cent", f32), ("leaves_bcube", f32, (6,)), ("branches_bcube", f32, (6,)),
                     ("num_leaves", np.uint32), ("num_branch_quads", np.uint32), ("flags", np.uint32), ("pad", np.uint32)])  # terra_decid_tree_data

TALLY = (("tiles", "skipped", "empty", "dropped", "dropped_negative", "dropped_outside", "dropped_not_generated", "tile_culled", "tile_zero_area", "tile_drawn", "sorted", "direct",
          "direct_all_visible_far", "sorted_ties", "sorted_culled", "bcube_zero_box", "conv_overflow", "at_dmax", "beyond_dmax", "lcc_drawn_not_visible", "low_detail",
          "low_detail_overridden", "reflection_low_detail", "nv_written", "nv_read_1", "max_ids_in_tile", "max_run", "max_records", "shadow_leaves_drawn", "shadow_branches_drawn",
          "cube_centre_visible", "cube_by_corners", "behind_true", "behind_false", "up_reject", "up_straddle", "side_reject", "side_straddle", "near_reject", "near_straddle",
          "far_reject", "far_straddle", "invalid_view_tests")
         + tuple(f"{s}_stage_{k}" for s in "lb" for k in range(1, 7)) + tuple(f"{s}_form_{k}" for s in "lb" for k in range(4))
         + tuple(f"{s}_{k}" for s in "lb" for k in ("at_start", "at_end", "between", "denom0", "above_start", "below_end"))
         + ("b_size_at_005", "b_size_below_005", "b_size_above_005")
         + tuple(f"{s}_{k}{q}" for s in ("nl", "num") for k in ("floor", "product", "full") for q in ("", "_4th")))


def new_tally():
    return {k: 0 for k in TALLY}


class Args:
    def __init__(self, behind_sphere_mult=1.0, zoom_f=1.0, lod_scales=(0.0, 0.0, 0.0, 0.0), shadow_pass=0, reflection_pass=0, billboards=1, leaf_color_changed=0, draw_leaves=1,
                 draw_branches=1):
        self.behind_sphere_mult, self.zoom_f, self.lod_scales = f32(behind_sphere_mult), f32(zoom_f), [f32(x) for x in lod_scales]
        self.shadow_pass, self.reflection_pass, self.billboards = int(bool(shadow_pass)), int(reflection_pass), int(bool(billboards))
        self.leaf_color_changed, self.draw_leaves, self.draw_branches = int(bool(leaf_color_changed)), int(bool(draw_leaves)), int(bool(draw_branches))


def add3(a, b):
    return [f32(a[0] + b[0]), f32(a[1] + b[1]), f32(a[2] + b[2])]


def cube_plus(box, p):  # cube_t + point: d[i][0] += p[i]; d[i][1] += p[i]
    return [[f32(box[2 * i] + p[i]), f32(box[2 * i + 1] + p[i])] for i in range(3)]


def is_all_zeros(d):
    return all(d[i][j] == 0 for i in range(3) for j in range(2))


def is_zero_area(d):
    return any(d[i][0] == d[i][1] for i in range(3))


class Scene:
    """what the pass reads of the globals: the scene's sizes and the offsets"""

    def __init__(self, tsc, xoff2=0, yoff2=0):
        g = tsc.g
        self.xlate = [f32(f32(tam.wrap32(tsc.dxoff + xoff2)) * g.DX_VAL), f32(f32(tam.wrap32(tsc.dyoff + yoff2)) * g.DY_VAL), ZERO]  # dtree_off.get_xlate()
        self.tile_width = g.tile_width
        self.dmax = f32(DRAW_DIST_TILES * g.scaled_tile_radius)            # get_draw_tile_dist()
        self.scene_sum = f32(1.0 * float(g.tile_width))                    # 1.0*(X_SCENE_SIZE + Y_SCENE_SIZE) narrowed to closest_dist_less_than's float


class Tree:
    def __init__(self, rec, td):
        self.center = [f32(rec["pos"][k]) for k in range(3)]
        self.td, self.tree_id = td, int(rec["tree_id"])
        self.not_visible = False

    def sphere_center(self):  # tree_center + point(0.0, 0.0, sphere_center_zoff)
        return add3(self.center, [ZERO, ZERO, f32(self.td["sphere_center_zoff"])])


def size_scale_mult(td):
    return float(LEAF_4TH_SCALE if int(td["flags"]) & HAS_4TH else ONE)


def calc_size_scale(sc, v, a, td, draw_pos, tally=None):
    dist_sq = view_model.p2p_dist_sq(v.pos, draw_pos)
    dd = f32(sc.dmax * sc.dmax)
    if tally is not None:
        tally["at_dmax"] += int(dist_sq == dd)
    if dist_sq > dd:
        if tally is not None:
            tally["beyond_dmax"] += 1
        return ZERO
    with np.errstate(all="ignore"):
        return f32(f32(f32(a.zoom_f * f32(td["base_radius"])) * inv_sqrt(dist_sq)) / DIST_C_SCALE)


def leaf_count(td, size_scale, tally):
    nl = int(td["num_leaves"])
    q = "_4th" if int(td["flags"]) & HAS_4TH else ""
    if float(size_scale) > 0.0:
        prod = 4.0 * float(nl) * float(size_scale) * size_scale_mult(td)
        if not (-9223372036854775808.0 < prod < 9223372036854775808.0):
            tally["conv_overflow"] += 1
        u = d2u(prod)
        m = max(nl // 8, u)
        tally["nl_full" + q if m >= nl else ("nl_product" + q if u > nl // 8 else "nl_floor" + q)] += 1
        nl = min(nl, m)
    return nl


def branch_count(td, size_scale, force_low_detail, shadow_pass, tally):
    nbq = int(td["num_branch_quads"])
    q = "_4th" if int(td["flags"]) & HAS_4TH else ""
    if float(size_scale) == 0.0:
        num = nbq
    else:
        prod = 1.5 * float(nbq) * float(size_scale) * size_scale_mult(td)
        if not (-9223372036854775808.0 < prod < 9223372036854775808.0):
            tally["conv_overflow"] += 1
        u = d2u(prod)
        m = max(nbq // 40, u)
        tally["num_full" + q if m >= nbq else ("num_product" + q if u > nbq // 40 else "num_floor" + q)] += 1
        num = min(nbq, m)
    low_detail = bool(force_low_detail or (float(size_scale) > 0.0 and float(size_scale) < 2.0))
    if not shadow_pass and int(td["flags"]) & HAS_4TH and num > nbq // 5:
        tally["low_detail_overridden"] += int(low_detail)
        low_detail = False
    tally["low_detail"] += int(low_detail)
    return num, low_detail


def opacity(a, billboards, tex_valid, size_scale, lod_start, lod_end, tally, s):
    """-> (geom_opacity, added)"""
    if not billboards:
        return ONE, False
    lod_denom = f32(lod_start - lod_end)
    tally[f"{s}_at_start"] += int(size_scale == lod_start)
    tally[f"{s}_above_start"] += int(size_scale > lod_start)
    if tex_valid and size_scale < lod_start:
        if float(lod_denom) == 0.0:
            tally[f"{s}_denom0"] += 1
            return ZERO, True
        tally[f"{s}_at_end"] += int(size_scale == lod_end)
        tally[f"{s}_below_end"] += int(size_scale < lod_end)
        tally[f"{s}_between"] += int(lod_end < size_scale)
        with np.errstate(all="ignore"):
            return cmax(ZERO, cmin(ONE, f32(f32(size_scale - lod_end) / lod_denom))), True
    return ONE, False


class Rec:
    """one sweep's answer for a record"""

    def __init__(self):
        self.word, self.num, self.scale, self.opacity, self.listed, self.bb = 0, 0, ZERO, ZERO, False, None

    def leave(self, stage, tally, s):
        self.word |= stage << STAGE_SHIFT
        tally[f"{s}_stage_{stage}"] += 1
        tally[f"{s}_form_0"] += 1
        return self


def form_of(geom_opacity, added):
    return FORM_BILLBOARD if float(geom_opacity) == 0.0 else (FORM_BOTH if added else FORM_GEOM)


def shadow_near(v, center):  # dist_less_than(center, camera_pdu.pos, camera_pdu.far_)
    return bool(view_model.p2p_dist_sq(center, v.pos) < f32(v.far_ * v.far_))


def draw_leaves_top(sc, v, a, t, index, billboards, tally):
    """tree::draw_leaves_top with, in the shadow pass, the two culls of :338-339 before it"""
    o, td = Rec(), t.td
    center = add3(t.sphere_center(), sc.xlate)
    r11 = f32(1.1 * float(f32(td["sphere_radius"])))
    if a.shadow_pass:
        if not shadow_near(v, center):
            return o.leave(ST_SHADOW_DIST, tally, "l")
        if not view_model.sphere_visible_test(v, a.behind_sphere_mult, center, r11, tally):
            return o.leave(ST_SHADOW_SPHERE, tally, "l")
        if int(td["num_leaves"]) == 0:  # draw_leaves_shadow_only: leaves.empty()
            return o.leave(ST_NO_LEAVES, tally, "l")
        o.scale, o.opacity, o.num, o.word, o.listed = HALF, ONE, leaf_count(td, HALF, tally), FORM_GEOM, True
        tally["l_form_1"] += 1
        tally["shadow_leaves_drawn"] += 1
        return o
    t.not_visible = not view_model.sphere_visible_test(v, a.behind_sphere_mult, center, r11, tally)  # !is_visible_to_camera(xlate)
    tally["nv_written"] += 1
    if t.not_visible:
        o.word |= NOT_VISIBLE
    if t.not_visible and not a.leaf_color_changed:
        return o.leave(ST_NOT_VISIBLE, tally, "l")
    if int(td["num_leaves"]) == 0:
        return o.leave(ST_NO_LEAVES, tally, "l")
    tree_xlate = add3(t.center, sc.xlate)
    if not a.leaf_color_changed and not cube_visible_likely(v, cube_plus(td["leaves_bcube"], tree_xlate), tally):
        return o.leave(ST_BOX, tally, "l")
    draw_pos = center
    size_scale = calc_size_scale(sc, v, a, td, draw_pos, tally)
    o.scale = size_scale
    if float(size_scale) == 0.0:
        return o.leave(ST_SIZE, tally, "l")
    geom_opacity, added = opacity(a, billboards, bool(int(td["flags"]) & LEAF_TEX), size_scale, a.lod_scales[2], a.lod_scales[3], tally, "l")
    o.opacity = geom_opacity
    o.word |= form_of(geom_opacity, added)
    tally[f"l_form_{o.word & 3}"] += 1
    if added:
        pos = add3(draw_pos, [ZERO, ZERO, f32(f32(td["lr_z_cent"]) - f32(td["sphere_center_zoff"]))])
        o.bb = (t.tree_id, index, pos, f32(1.0 - float(geom_opacity)))
    if float(geom_opacity) == 0.0:
        return o
    tally["lcc_drawn_not_visible"] += int(t.not_visible)
    o.num, o.listed = leaf_count(td, size_scale, tally), True
    return o


def draw_branches_top(sc, v, a, t, index, billboards, tally):
    """tree::draw_branches_top with, in the shadow pass, the cull of :325 before it"""
    o, td = Rec(), t.td
    center = add3(t.sphere_center(), sc.xlate)
    if a.shadow_pass and not shadow_near(v, center):
        return o.leave(ST_SHADOW_DIST, tally, "b")
    if not a.shadow_pass and t.not_visible:
        o.word |= NOT_VISIBLE
        tally["nv_read_1"] += 1
        return o.leave(ST_NOT_VISIBLE, tally, "b")
    tree_xlate = add3(t.center, sc.xlate)
    if not cube_visible_likely(v, cube_plus(td["branches_bcube"], tree_xlate), tally):
        return o.leave(ST_BOX, tally, "b")
    if a.shadow_pass:  # td.draw_branches(1.0, 1, 1)
        num, low = branch_count(td, ONE, True, True, tally)
        o.scale, o.opacity, o.num, o.word, o.listed = ONE, ONE, num, FORM_GEOM | (LOW_DETAIL if low else 0), True
        tally["b_form_1"] += 1
        tally["shadow_branches_drawn"] += 1
        return o
    size_scale = calc_size_scale(sc, v, a, td, center, tally)
    o.scale = size_scale
    tally["b_size_at_005"] += int(size_scale == f32(0.05))
    tally["b_size_below_005" if float(size_scale) < 0.05 else "b_size_above_005"] += 1
    if float(size_scale) < 0.05:
        return o.leave(ST_SIZE, tally, "b")
    geom_opacity, added = opacity(a, billboards, bool(int(td["flags"]) & BRANCH_TEX), size_scale, a.lod_scales[0], a.lod_scales[1], tally, "b")
    o.opacity = geom_opacity
    o.word |= form_of(geom_opacity, added)
    tally[f"b_form_{o.word & 3}"] += 1
    if added:
        o.bb = (t.tree_id, index, center, f32(1.0 - float(geom_opacity)))
    if float(geom_opacity) == 0.0:
        return o
    num, low = branch_count(td, size_scale, bool(a.reflection_pass), False, tally)
    tally["reflection_low_detail"] += int(bool(a.reflection_pass) and low)
    o.num, o.listed = num, True
    if low:
        o.word |= LOW_DETAIL
    return o


def calc_bcube(trees, tally):
    bc = [[ZERO, ZERO], [ZERO, ZERO], [ZERO, ZERO]]
    for t in trees:
        b, l = cube_plus(t.td["branches_bcube"], t.center), cube_plus(t.td["leaves_bcube"], t.center)
        if is_all_zeros(b):  # assign_or_union_with_cube
            tally["bcube_zero_box"] += 1
        elif is_all_zeros(bc):
            bc = b
        else:
            bc = [[cmin(bc[i][0], b[i][0]), cmax(bc[i][1], b[i][1])] for i in range(3)]
        bc = [[cmin(bc[i][0], l[i][0]), cmax(bc[i][1], l[i][1])] for i in range(3)]  # union_with_cube
    return bc


class TileResult:
    def __init__(self):
        self.flags = self.num_trees = 0
        self.bcube = [ZERO] * 6
        self.valid = []                      # the record indices that are not dropped
        self.leaf, self.branch = {}, {}      # record index -> Rec, of the sweeps that ran
        self.not_visible = {}                # record index -> 0 / 1, where :1017 assigns
        self.leaf_list, self.branch_list, self.leaf_bb, self.branch_bb = [], [], [], []


def draw_decid_trees(sc, v, a, recs, data, nv_in, tally):
    """one tile: recs the first min(count, capacity) records, nv_in its not_visible bytes or None"""
    res = TileResult()
    trees = []
    for j, r in enumerate(recs):
        tid = int(r["tree_id"])
        if tid < 0 or tid >= len(data) or not int(data[tid]["flags"]) & GENERATED:
            tally["dropped"] += 1
            tally["dropped_negative" if tid < 0 else ("dropped_outside" if tid >= len(data) else "dropped_not_generated")] += 1
            continue
        trees.append((j, Tree(r, data[tid])))
    tally["max_records"] = max(tally["max_records"], len(recs))
    if not trees:  # decid_trees.empty() (:1557)
        tally["empty"] += 1
        return res
    res.num_trees, res.valid = len(trees), [j for j, _ in trees]
    bc = calc_bcube([t for _, t in trees], tally)
    res.bcube = [bc[i][k] for i in range(3) for k in range(2)]
    zero_area = is_zero_area(bc)
    if zero_area:
        res.flags |= TILE_BCUBE_ZERO_AREA
        tally["tile_zero_area"] += 1
    if not zero_area and not view_model.cube_visible(v, [[f32(bc[i][0] + sc.xlate[i]), f32(bc[i][1] + sc.xlate[i])] for i in range(3)]):  # VFC (:316)
        tally["tile_culled"] += 1
        return res
    tally["tile_drawn"] += 1
    res.flags |= TILE_DRAWN | (TILE_LEAVES if a.draw_leaves else 0) | (TILE_BRANCHES if a.draw_branches else 0)
    billboards = bool(a.billboards and not a.shadow_pass)  # enable_billboards
    ids = [t.tree_id for _, t in trees]
    tally["max_ids_in_tile"] = max(tally["max_ids_in_tile"], len(set(ids)))
    tally["max_run"] = max(tally["max_run"], max(ids.count(i) for i in set(ids)))
    if a.draw_leaves:  # the leaves sweep comes first (src/tiled_mesh.cpp:3268-3292)
        order = trees
        if not a.shadow_pass:
            local_camera = view_model.sub(v.pos, sc.xlate)
            direct = not is_all_zeros(bc) and not bool(view_model.p2p_dist_sq(local_camera, view_model.closest_pt(bc, local_camera)) < f32(sc.scene_sum * sc.scene_sum))
            if direct:
                tally["direct"] += 1
            else:
                res.flags |= TILE_SORTED
                tally["sorted"] += 1
                keys = [(view_model.p2p_dist_sq(t.sphere_center(), local_camera), k) for k, (_, t) in enumerate(trees)]
                keys.sort(key=lambda e: (float(e[0]), e[1]))  # std::sort of pair<float, unsigned>
                tally["sorted_ties"] += sum(1 for x, y in zip(keys, keys[1:]) if x[0] == y[0])
                order = [trees[k] for _, k in keys]
        for j, t in order:
            o = draw_leaves_top(sc, v, a, t, j, billboards, tally)
            res.leaf[j] = o
            if not a.shadow_pass:
                res.not_visible[j] = int(t.not_visible)
            if o.bb is not None:
                res.leaf_bb.append(o.bb)
            if o.listed:
                res.leaf_list.append(j)
            elif res.flags & TILE_SORTED:
                tally["sorted_culled"] += 1
    elif not a.shadow_pass and nv_in is not None:
        for j, t in trees:
            t.not_visible = bool(nv_in[j])
    if a.draw_branches:
        for j, t in trees:
            o = draw_branches_top(sc, v, a, t, j, billboards, tally)
            res.branch[j] = o
            if o.bb is not None:
                res.branch_bb.append(o.bb)
            if o.listed:
                res.branch_list.append(j)
    res.leaf_bb.sort(key=lambda e: e[0])    # stable: within an id the order of addition
    res.branch_bb.sort(key=lambda e: e[0])
    return res


def draw(tsc, v, a, tiles, data, decid, counts, skip=None, not_visible=None, xoff2=0, yoff2=0, tally=None):
    """the batch -> [TileResult]; decid DECID_PLACE records [n, cap]; tsc terrain_view_model.Scene; not_visible uint8 [n, cap] or None (read only here: a result's
    not_visible says what the call writes)"""
    tally = new_tally() if tally is None else tally
    sc = Scene(tsc, xoff2, yoff2)
    n, cap = decid.shape
    out = []
    for i in range(n):
        tally["tiles"] += 1
        if skip is not None and skip[i]:
            tally["skipped"] += 1
            out.append(TileResult())
            continue
        m = min(int(counts[i]), cap)
        out.append(draw_decid_trees(sc, v, a, decid[i, :m], data, None if not_visible is None else not_visible[i], tally))
    return out
