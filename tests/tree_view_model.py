"""NumPy / Python float32 restatement of the pine and palm tree draw lists of a tile batch for a camera, written from the reference statements (not from the
library's bodies):

    tile_t::draw_pine_trees (without its GL and shader calls)                  src/tiled_mesh.cpp:1465-1526
    tile_t::draw_tree_leaves_lod                                               src/tiled_mesh.cpp:1459-1462
    the weights of tile_t::update_pine_tree_state                              src/tiled_mesh.cpp:1440-1448
    get_tree_scale_denom, get_dist_to_camera_in_tiles, get_tree_dist_scale,
      get_tree_far_weight, contains_camera                                     src/tiled_mesh.h:95, 264-265, 332-338
    small_tree_group::draw_trunks, get_back_to_front_ordering,
      draw_tree_insts (up to the GL loop), draw_pine_leaves,
      draw_non_pine_leaves, calc_bcube                                         src/sm_tree.cpp:176-179, 206-224, 233-323
    small_tree's constructors, get_trunk_cylin, add_bounds_to_bcube,
      are_leaves_visible, draw_trunk (down to nsides), stt[]                   src/sm_tree.cpp:46-53, 705-777, 832-838, 1007-1017, 1081-1102
    get_xy_radius, get_trunk_bsphere_radius                                    src/small_tree.h:77-78
    get_default_tree_depth, get_tree_z_bottom (the tiled-terrain branch)       src/Tree.cpp:209-214
    cube_t::assign_or_union_with_cube, cylinder_3dw::get_center                src/3DWorld.h:512-515, 748

The tile's centre, box and distance are tests/terrain_view_model.py's, the view tests (sphere_visible_test with its tally of the planes, cube_visible,
point_visible_test) tests/view_model.py's, the sizes of a record tests/tree_ao_model.py's (restatements of their own).  Types: np.float32 for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are
double: `(is_pine ? 1.05 : 0.8)*height`, `pos.z - 0.2*width`, the factor (0.5 + 0.5/tree_scale) of the tree depth, both arms of get_xy_radius's max, `0.2*width` and
`0.5*height` times a direction (operator*(S, pointT<T>) multiplies in S and narrows each component), `0.3*height + 0.2*width`, `r1 + 0.5*(..)` of the trunk's bounding
sphere, `-0.5*radius`, `0.25*size_scale/dist`, `1.0 - far_weight`, and the comparisons of dscale and weight with double literals.  sphere_in_camera_view(.., 2) is
sphere_visible_test alone in tiled-terrain mode (src/visibility.cpp:338-339).  The instance lists are sorted by (id, record index): the reference's sort looks at the
id alone.

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import numpy as np
import terrain_view_model as tm
import tree_ao_model as tam
import view_model

f32 = np.float32
T_PINE, T_DECID, T_TDECID, T_BUSH, T_PALM, T_SH_PINE = range(6)
N_CYL_SIDES = 32
TREE_LOD_THRESH, GEOMORPH_THRESH, PALM_DIST_SCALE = f32(6.0), f32(6.0), f32(0.75)
LINE_THRESH, TREE_DEPTH = f32(700.0), f32(0.1)
TOLERANCE = f32(1.0E-12)
W2 = [f32(x) for x in (0.00, 0.13, 0.13, 0.00, 0.03, 0.00)]  # stt[].w2: float members initialised from the double literals
WS = [f32(x) for x in (0.14, 0.15, 0.15, 0.15, 0.12, 0.08)]  # stt[].ws
SS = [f32(x) for x in (0.4, 0.8, 0.7, 0.8, 0.6, 0.4)]        # stt[].ss
ZERO, ONE = f32(0.0), f32(1.0)
TRUNK_NONE, TRUNK_POLY_ALL, TRUNK_POLY_SKIPPED, TRUNK_POINTS = range(4)
NEAR_LEAVES, FAR_LEAVES, DITHERED, PALMS, DRAW_ALL_NEAR, DRAW_ALL_FAR, ALL_VISIBLE, NEEDS_HIGH, NEEDS_LOW, CONTAINS_CAMERA = 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800
cmax, cmin, sub, sphere_visible_test = view_model.cmax, view_model.cmin, view_model.sub, view_model.sphere_visible_test

TALLY = ("tiles", "skipped", "empty", "dropped", "trunk_none", "trunk_poly_all", "trunk_poly_skipped", "trunk_points", "trunks_culled", "weight0", "weight_mid", "weight1",
         "palms_yes", "palms_no", "palms_inst_clause", "palms_inst_clause_fails", "contains_camera", "sorted_lists", "sorted_ties", "draw_all_near", "near_not_all",
         "lists_culled_centre_visible", "pine_list", "palm_list", "palm_list_entries", "pine_insts", "palm_insts", "inst_sh_pine", "render_all", "byte_bush", "byte_culled",
         "byte_small", "byte_line", "nsides_4_clamped", "nsides_32_clamped", "nsides_between", "nsides_shadow", "rotated", "rotated_ignored", "behind_true", "behind_false",
         "up_reject", "up_straddle", "side_reject", "side_straddle", "near_reject", "near_straddle", "far_reject", "far_straddle", "invalid_view_tests", "leaves_visible",
         "leaves_hidden", "bcube_zero_box", "max_ids_in_tile", "max_share_of_id")


def new_tally():
    return {k: 0 for k in TALLY}


class Args:
    def __init__(self, behind_sphere_mult=1.0, zoom_f=1.0, tree_depth_scale=1.0, window_width=1920, shadow_pass=0, draw_trunks=1, draw_near_leaves=1, draw_far_leaves=1):
        self.behind_sphere_mult, self.zoom_f, self.tree_depth_scale = f32(behind_sphere_mult), f32(zoom_f), f32(tree_depth_scale)
        self.window_width, self.shadow_pass = int(window_width), int(bool(shadow_pass))
        self.draw_trunks, self.draw_near_leaves, self.draw_far_leaves = int(bool(draw_trunks)), int(bool(draw_near_leaves)), int(bool(draw_far_leaves))


def add(a, b):
    return [f32(a[0] + b[0]), f32(a[1] + b[1]), f32(a[2] + b[2])]


def scale_d(d, vec):  # operator*(S const v, pointT<T> const &p) with S = double: pointT<T>(v*p.x, v*p.y, v*p.z)
    return [f32(d * float(vec[0])), f32(d * float(vec[1])), f32(d * float(vec[2]))]


def scale_f(vec, s):  # pointT::operator*(T const val)
    return [f32(vec[0] * s), f32(vec[1] * s), f32(vec[2] * s)]


class Globals:
    """what the trees read beside the scene: the size settings (tree_ao_model.SizeParams), `instanced` with the instance table, the args"""

    def __init__(self, p, a, instanced=False, insts=None):
        self.p, self.a, self.instanced = p, a, bool(instanced)
        self.insts = np.zeros(0, tam.INST_DTYPE) if insts is None else np.asarray(insts, tam.INST_DTYPE)
        self.tsize = tam.calc_tree_size(p)
        self.denom = cmax(ONE, f32(TREE_LOD_THRESH * self.tsize))  # get_tree_scale_denom()
        # get_default_tree_depth(): TREE_DEPTH*tree_depth_scale*(0.5 + 0.5/tree_scale)
        self.tree_depth = f32(float(f32(TREE_DEPTH * a.tree_depth_scale)) * (0.5 + 0.5 / float(p.tree_scale)))


class SmallTree:
    """a record after its constructor: None where the tree AO pass drops the record"""

    @staticmethod
    def make(g, rec, ov):
        inst = int(rec["inst"])
        if inst >= 0:
            if not g.instanced or inst >= len(g.insts):
                return None
            t, h, w = tam.instanced_size(g.p, g.insts[inst])  # small_tree(p, instance_id) (:705-715)
            if not 0 <= t < tam.NUM_ST_TYPES:
                return None
        else:
            t = int(rec["type"])
            if not 0 <= t < tam.NUM_ST_TYPES:
                return None
            h, w = tam.small_tree_size(g.p, rec["height"], rec["width"], t)
        s = SmallTree()
        s.type, s.height, s.width, s.inst_id = t, f32(h), f32(w), inst
        s.pos = [f32(x) for x in rec["pos"]]
        s.rotated = bool(ov is not None and int(ov["rotated"]) != 0)  # r_angle != 0.0
        if s.rotated:
            s.p1, s.p2, s.r1, s.r2 = [f32(x) for x in ov["p1"]], [f32(x) for x in ov["p2"]], f32(ov["r1"]), f32(ov["r2"])
        else:
            s.get_trunk_cylin(g)
        return s

    def is_pine_tree(self):
        return self.type in (T_PINE, T_SH_PINE)

    def get_trunk_cylin(self, g):
        if self.type == T_BUSH:  # cylinder_3dw()
            self.p1, self.p2, self.r1, self.r2 = [ZERO] * 3, [ZERO] * 3, ZERO, ZERO
            return
        dirv = [ZERO, ZERO, ONE]  # plus_z; r_angle == 0
        is_pine = self.is_pine_tree()
        trunk_height = f32((1.05 if is_pine else 0.8) * float(self.height))
        zb = f32(float(self.pos[2]) - 0.2 * float(self.width))
        zbot = f32(zb - g.tree_depth)  # get_tree_z_bottom(zb, pos): world_mode != WMODE_GROUND
        length = f32(trunk_height + f32(zb - zbot))
        base_rscale = f32(f32(f32(0.8) * length) / trunk_height) if (is_pine or self.type == T_PALM) else ONE
        self.p1 = add(self.pos, scale_f(dirv, f32(zbot - self.pos[2])))
        self.p2 = add(self.p1, scale_f(dirv, length))
        self.r1, self.r2 = f32(f32(WS[self.type] * self.width) * base_rscale), f32(W2[self.type] * self.width)

    def get_rot_dir(self):  # (r_angle == 0.0) ? plus_z : trunk_cylin.get_norm_dir_vect()
        if not self.rotated:
            return [ZERO, ZERO, ONE]
        d = sub(self.p2, self.p1)
        vmag = f32(np.sqrt(view_model.mag_sq(d)))
        return d if vmag < TOLERANCE else [f32(d[0] / vmag), f32(d[1] / vmag), f32(d[2] / vmag)]

    def get_xy_radius(self):  # max(1.5*branch_xy_scale*width, 0.5*height)
        return f32(max(1.5 * float(ONE) * float(self.width), 0.5 * float(self.height)))

    def cylin_center(self):  # 0.5f*(p1 + p2)
        s = add(self.p1, self.p2)
        return [f32(f32(0.5) * s[0]), f32(f32(0.5) * s[1]), f32(f32(0.5) * s[2])]

    def bounds(self):  # add_bounds_to_bcube's bc
        c, r = self.cylin_center(), self.get_xy_radius()
        return [[f32(c[0] - r), f32(c[0] + r)], [f32(c[1] - r), f32(c[1] + r)], [self.p1[2], self.p2[2]]]

    def get_trunk_bsphere_radius(self):
        if not self.rotated:
            ext = abs(f32(self.p1[2] - self.p2[2]))
        else:
            ext = f32(np.sqrt(view_model.mag_sq(sub(self.p1, self.p2))))
        return f32(float(self.r1) + 0.5 * float(ext))

    def are_leaves_visible(self, v, g, xlate, tally):
        if self.type == T_PALM:
            c = add(sub(self.p2, scale_d(0.2 * float(self.width), self.get_rot_dir())), xlate)
            r = sphere_visible_test(v, g.a.behind_sphere_mult, c, f32(0.3 * float(self.height) + 0.2 * float(self.width)), tally)
        elif not self.rotated:
            c = add(add(self.pos, [ZERO, ZERO, f32(0.5 * float(self.height))]), xlate)
            r = sphere_visible_test(v, g.a.behind_sphere_mult, c, self.get_xy_radius(), tally)
        else:
            c = add(add(self.pos, scale_d(0.5 * float(self.height), self.get_rot_dir())), xlate)
            r = sphere_visible_test(v, g.a.behind_sphere_mult, c, self.get_xy_radius(), tally)
        if tally is not None:
            tally["leaves_visible" if r else "leaves_hidden"] += 1
        return r

    def draw_trunk(self, v, g, all_visible, xlate, tally):
        """-> the trunk byte: 0 = returned 1 without drawing, 1 = the skipped line (the only case that returns 0), else nsides"""
        a = g.a
        if self.type == T_BUSH:
            tally["byte_bush"] += 1
            return 0
        if not all_visible:
            if not sphere_visible_test(v, a.behind_sphere_mult, add(self.cylin_center(), xlate), self.get_trunk_bsphere_radius(), tally):
                tally["byte_culled"] += 1
                return 0
        size_scale = f32(f32(f32(a.zoom_f * SS[self.type]) * self.width) * f32(a.window_width))
        dist = f32(np.sqrt(view_model.p2p_dist_sq(v.pos, add(self.pos, xlate))))  # distance_to_camera(pos + xlate)
        if not a.shadow_pass and size_scale < dist:
            tally["byte_small"] += 1
            return 0
        if not a.shadow_pass and f32(f32(LINE_THRESH * a.zoom_f) * f32(self.r1 + self.r2)) < dist:
            tally["byte_line"] += 1
            return 1
        if a.shadow_pass:
            tally["nsides_shadow"] += 1
            return 4
        with np.errstate(all="ignore"):
            q = np.float64(0.25 * float(size_scale)) / np.float64(dist)
        qi = int(q) if np.isfinite(q) and -2147483649.0 < q < 2147483648.0 else -2147483648  # cvttsd2si
        tally["nsides_4_clamped" if qi < 4 else ("nsides_32_clamped" if qi > N_CYL_SIDES else "nsides_between")] += 1
        return max(4, min(N_CYL_SIDES, qi))


def calc_bcube(trees, tally):
    bc = [[ZERO, ZERO], [ZERO, ZERO], [ZERO, ZERO]]
    zeros = lambda c: all(c[i][j] == 0 for i in range(3) for j in range(2))  # noqa: E731
    for s in trees:
        if s is None:
            continue
        c = s.bounds()
        if zeros(c):  # assign_or_union_with_cube: if (c.is_all_zeros()) return;
            tally["bcube_zero_box"] += 1
            continue
        if zeros(bc):
            bc = c
        else:
            bc = [[cmin(bc[i][0], c[i][0]), cmax(bc[i][1], c[i][1])] for i in range(3)]
    return bc


class TileResult:
    def __init__(self):
        self.written = False  # False: a skipped or empty tile -- zero tile record, box and counts, nothing else written
        self.dscale = self.weight = ZERO
        self.flags = self.num_pine = self.num_palm = self.num_trees = 0
        self.bcube = [ZERO] * 6
        self.pine_insts, self.palm_insts = [], []  # (id, pos)
        self.leaf_pine, self.leaf_palm = None, []  # None: no pine list written (leaf_count_pine says what render_all drew)
        self.leaf_count_pine = 0
        self.trunk = None


def draw_pine_trees(sc, v, g, txy, st, trmax, recs, ovs, xlate, tally):
    """one tile: recs the first min(count, capacity) records, ovs their override entries or None"""
    res = TileResult()
    trees = [SmallTree.make(g, recs[j], None if ovs is None else ovs[j]) for j in range(len(recs))]
    tally["dropped"] += sum(1 for s in trees if s is None)
    for j, s in enumerate(trees):
        if s is not None and ovs is not None:
            tally["rotated" if s.rotated else "rotated_ignored"] += 1
    valid = [s for s in trees if s is not None]
    if not valid:  # pine_trees.empty() (:1468)
        tally["empty"] += 1
        return res
    a = g.a
    res.written = True
    num_pine, num_palm = sum(1 for s in valid if s.is_pine_tree()), sum(1 for s in valid if s.type == T_PALM)
    res.num_pine, res.num_palm, res.num_trees = num_pine, num_palm, len(valid)
    bc = calc_bcube(trees, tally)
    res.bcube = [bc[0][0], bc[0][1], bc[1][0], bc[1][1], bc[2][0], bc[2][1]]
    t = tm.Tile(sc, txy, st, 0.0, trmax, None, 0, 0)
    center = tm.get_center(sc, t)
    in_tiles = f32(tm.get_rel_dist_to_camera(sc, v, t, True) * f32(tm.TILE_RADIUS))  # get_dist_to_camera_in_tiles()

    def dist_scale(has_palm=False):
        return f32(f32((PALM_DIST_SCALE if has_palm else ONE) * in_tiles) / g.denom)

    def far_weight(force_high_detail, has_palm=False):
        if force_high_detail:
            return ZERO
        return cmax(ZERO, cmin(ONE, f32(GEOMORPH_THRESH * f32(dist_scale(has_palm) - ONE))))  # CLIP_TO_01

    def cube_vis():
        return view_model.cube_visible(v, [[f32(bc[i][0] + xlate[i]), f32(bc[i][1] + xlate[i])] for i in range(3)])  # all_bcube + xlate

    force = bool(a.shadow_pass)
    has_palm = num_palm > 0
    flags = 0
    res.dscale = dist_scale()
    all_visible = sphere_visible_test(v, a.behind_sphere_mult, center, f32(-0.5 * float(t.radius)))
    bcube_t = tm.get_bcube(sc, t)
    contains_camera = bool(bcube_t[0][0] <= v.pos[0] <= bcube_t[0][1] and bcube_t[1][0] <= v.pos[1] <= bcube_t[1][1])
    flags |= ALL_VISIBLE if all_visible else 0
    flags |= CONTAINS_CAMERA if contains_camera else 0
    tally["contains_camera"] += int(contains_camera)
    # update_pine_tree_state: weights {high, low}
    w = far_weight(force, has_palm)
    if float(f32(ONE - w)) > 0.0:
        flags |= NEEDS_HIGH
    if float(w) > 0.0:
        flags |= NEEDS_LOW
    res.trunk = [0] * len(recs)
    if a.draw_trunks:
        dscale = ZERO if a.shadow_pass else dist_scale()
        if float(dscale) < 1.0:
            all_drawn = True
            if not all_visible and not cube_vis():  # draw_trunks' VFC: return 0
                all_drawn = False
                tally["trunks_culled"] += 1
            else:
                for j, s in enumerate(trees):
                    if s is None:
                        continue
                    res.trunk[j] = s.draw_trunk(v, g, all_visible, xlate, tally)
                    if res.trunk[j] == 1:
                        all_drawn = False
            flags |= TRUNK_POLY_ALL if all_drawn else TRUNK_POLY_SKIPPED
            tally["trunk_poly_all" if all_drawn else "trunk_poly_skipped"] += 1
        elif float(dscale) < 2.0 and float(far_weight(force)) < 0.5:
            flags |= TRUNK_POINTS
            tally["trunk_points"] += 1
        else:
            tally["trunk_none"] += 1
    weight = f32(1.0 - float(far_weight(force, has_palm)))
    res.weight = weight
    dith = 0.0 < float(weight) < 1.0
    flags |= DITHERED if dith else 0
    tally["weight0" if float(weight) == 0.0 else ("weight_mid" if dith else "weight1")] += 1
    sweeps = []  # low_detail of every draw_tree_leaves_lod call
    palms = False
    if a.draw_near_leaves or a.draw_far_leaves:
        if dith:
            if a.draw_near_leaves:
                sweeps.append(False)
            if a.draw_far_leaves:
                sweeps.append(True)
        elif (a.draw_far_leaves if float(weight) == 0.0 else a.draw_near_leaves):
            sweeps.append(float(weight) == 0.0)
        if a.draw_near_leaves and has_palm:
            inst_clause = g.instanced and float(dist_scale(has_palm)) < 3.0
            palms = bool(float(weight) > 0.0 or a.shadow_pass or inst_clause)
            if not (float(weight) > 0.0 or a.shadow_pass):
                tally["palms_inst_clause" if inst_clause else "palms_inst_clause_fails"] += 1
            tally["palms_yes" if palms else "palms_no"] += 1
    near, far = None, False  # near: what the high-detail sweep did when the group is not instanced: "all", "culled" or the list; far: the low-detail sweep drew the pines
    for low_detail in sweeps:  # draw_tree_leaves_lod -> draw_pine_leaves(s, 0, low_detail, draw_all, contains_camera(), xlate)
        draw_all = bool(low_detail or view_model.point_visible_test(v, center))
        flags |= (FAR_LEAVES if low_detail else NEAR_LEAVES) | ((DRAW_ALL_FAR if low_detail else DRAW_ALL_NEAR) if draw_all else 0)
        if not low_detail:
            tally["draw_all_near" if draw_all else "near_not_all"] += 1
        if g.instanced and not low_detail:  # draw_pine_insts
            res.pine_insts = draw_tree_insts(v, g, trees, num_pine, draw_all, cube_vis, xlate, True, tally)
            continue
        if num_pine == 0:
            continue
        if not draw_all and not cube_vis():
            near = "culled"
            continue
        if draw_all:  # render_all
            tally["render_all"] += 1
            if low_detail:
                far = True
            else:
                near = "all"
            continue
        tally["pine_list"] += 1
        if contains_camera:  # sort_front_to_back: get_back_to_front_ordering
            ref_pos = sub(v.pos, xlate)
            to_draw = sorted((view_model.p2p_dist_sq(s.pos, ref_pos), j) for j, s in enumerate(trees) if s is not None and s.are_leaves_visible(v, g, xlate, tally))
            tally["sorted_lists"] += 1
            order = [j for _, j in to_draw]
        else:
            to_draw = None
            order = [j for j, s in enumerate(trees) if s is not None]
        near = [j for j in order if trees[j].is_pine_tree() and trees[j].are_leaves_visible(v, g, xlate, None)]  # small_tree::draw_pine_leaves
        if to_draw is not None:
            keys = [d for d, j in to_draw if trees[j].is_pine_tree()]
            tally["sorted_ties"] += sum(1 for k in range(1, len(keys)) if keys[k] == keys[k - 1])
    # leaf_counts[0]: the high-detail sweep's draws when it ran on a group that is not instanced, else render_all's of the low-detail sweep
    if isinstance(near, list):
        res.leaf_pine, res.leaf_count_pine = near, len(near)
    elif near is not None:
        res.leaf_count_pine = num_pine if near == "all" else 0
    elif far:
        res.leaf_count_pine = num_pine
    if palms:
        flags |= PALMS
        if g.instanced:  # draw_palm_insts(s, sphere_visible_test(get_center(), -0.5*radius), ..)
            res.palm_insts = draw_tree_insts(v, g, trees, num_palm, all_visible, cube_vis, xlate, False, tally)
        elif cube_vis():  # draw_non_pine_leaves(0, 1, 0, ..)
            tally["palm_list"] += 1
            res.leaf_palm = [j for j, s in enumerate(trees) if s is not None and not s.is_pine_tree() and s.type == T_PALM and s.are_leaves_visible(v, g, xlate, tally)]
            tally["palm_list_entries"] += len(res.leaf_palm)
    if not cube_vis() and sphere_visible_test(v, a.behind_sphere_mult, center, t.radius):
        tally["lists_culled_centre_visible"] += 1
    res.flags = flags
    return res


def draw_tree_insts(v, g, trees, num_of_this_type, draw_all, cube_vis, xlate, is_pine, tally):
    if num_of_this_type == 0:
        return []
    if not draw_all and not cube_vis():
        return []
    insts = []
    for j, s in enumerate(trees):
        if s is None or (is_pine and not s.is_pine_tree()) or (not is_pine and s.type != T_PALM):
            continue
        if s.inst_id < 0:  # get_inst_id() asserts
            continue
        if draw_all or s.are_leaves_visible(v, g, xlate, tally):
            insts.append((s.inst_id, j, s.pos))
            if is_pine and s.type == T_SH_PINE:
                tally["inst_sh_pine"] += 1
    insts.sort(key=lambda e: (e[0], e[1]))
    tally["pine_insts" if is_pine else "palm_insts"] += len(insts)
    ids = [e[0] for e in insts]
    if ids:
        tally["max_ids_in_tile"] = max(tally["max_ids_in_tile"], len(set(ids)))
        tally["max_share_of_id"] = max(tally["max_share_of_id"], max(ids.count(i) for i in set(ids)))
    return [(e[0], e[2]) for e in insts]


def draw(sc, v, g, tiles, stats, pine, counts, skip=None, trmax=None, override=None, xoff2=0, yoff2=0, tally=None):
    """the batch -> [TileResult]; pine TREE_PLACE records [n, cap]"""
    tally = new_tally() if tally is None else tally
    n, cap = pine.shape
    xlate = [f32(f32(tam.wrap32(sc.dxoff + xoff2)) * sc.DX_VAL), f32(f32(tam.wrap32(sc.dyoff + yoff2)) * sc.DY_VAL), ZERO]  # ptree_off.get_xlate()
    out = []
    for i in range(n):
        tally["tiles"] += 1
        if skip is not None and skip[i]:
            tally["skipped"] += 1
            out.append(TileResult())
            continue
        m = min(int(counts[i]), cap)
        out.append(draw_pine_trees(sc, v, g, tiles[i], stats[i], ZERO if trmax is None else f32(trmax[i]), pine[i, :m], None if override is None else override[i, :m], xlate, tally))
    return out
