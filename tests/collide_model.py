"""NumPy / Python float32 restatement of the sphere collisions and tree box tests against the object containers of a tile batch, written from the reference
statements (not from the library's bodies), as the literal sequential loops:

    tile_draw_t::check_sphere_collision, check_cube_int_trees                  src/tiled_mesh.cpp:3566-3569, 3576-3579
    get_tile_pair_at_point, get_tile_containing_point                          src/tiled_mesh.cpp:3532-3537
    tile_t::check_sphere_collision, check_cube_int_trees                       src/tiled_mesh.cpp:2146-2173
    tile_t::get_tile_zmax, get_bcube, contains_point                           src/tiled_mesh.h:207, 232-236, 264
    small_tree_group::check_sphere_coll, small_tree::check_sphere_coll         src/sm_tree.cpp:181-186, 841-852
    tree::check_sphere_coll, tree_cont_t::check_sphere_coll,
      tree::check_cube_int, tree_cont_t::check_cube_int                        src/Tree.cpp:280-309
    scenery_group::check_sphere_coll, check_scenery_vector_sphere_coll         src/scenery.cpp:1100-1104, 1187-1199
    scenery_obj / s_stump / s_plant::check_sphere_coll                         src/scenery.cpp:80-86, 665-668, 772-775
    s_log::check_sphere_coll (returns 0), "no mushrooms"                       src/scenery.h:114; src/scenery.cpp:1197
    sphere_vert_cylin_intersect (without its asserts), sphere_cube_intersect   src/Math3d.cpp:427-437, 920-935
    dist_less_than, dist_xy_less_than, round_fp                                src/inlines.h:63, 176-195
    pointT::get_norm, cube_t::is_zero_area, intersects, contains_pt_xy,
      contains_pt_exp, get_cube_center, tile_offset_t::get_xlate               src/3DWorld.h:297-300, 524-527, 536-539, 579, 583, 602-604; src/animals.h:25

The tile's box is tests/terrain_view_model.py's, a small tree with its trunk_cylin and the group's calc_bcube tests/tree_view_model.py's, a deciduous tree and its
container's calc_bcube tests/decid_view_model.py's (restatements of their own).  Types: np.float32 for float, Python float for double, Python int for int.  Which
sub-expressions are double: 1.001*rsum (narrowed into operator*'s float parameter), 0.9*td.br_scale*td.base_radius (narrowed into trunk_radius), 0.2*height and
0.1*height (narrowed into point's float member), 0.1*radius of a rock_shape's pos.z.  int(float) is tests/view_model.py's x86 conversion: INT_MIN for what does not fit.

The tally counts what each query met, so that a case can show that it exercises what it is named for."""
import numpy as np

import decid_view_model as dm
import terrain_view_model as tm
import tree_ao_model as tam
import tree_view_model as vm
import view_model

f32 = np.float32
ZERO, HALF = f32(0.0), f32(0.5)
TOLERANCE = f32(1.0E-12)
cmax, cmin, sub, f2i, p2p_dist_sq = view_model.cmax, view_model.cmin, view_model.sub, view_model.f2i, view_model.p2p_dist_sq
LEAFY, PLANT, ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LOG, STUMP, MUSHROOM = range(9)
WALK = (ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LOG, STUMP, PLANT, LEAFY)  # scenery_group::check_sphere_coll's order; no mushrooms
INC_DTREES, INC_PTREES, INC_SCENERY = 1, 2, 4
TILE_DISTANT, TILE_NO_SCENERY = 1, 2
HIT_PINE, HIT_DECID, HIT_SCENERY, ROCK_SHAPE_UNDECIDED, STAGE_SHIFT = 1, 2, 4, 8, 8
TESTED, NO_TILE, DISTANT, OUTSIDE, ABOVE, BAD_QUERY = range(6)
STAGE_NAMES = ("tested", "no_tile", "distant", "outside", "above", "bad_query")
CUBE_HIT, CUBE_NO_TILE, CUBE_BAD_QUERY = 1, 2, 4
QUERY_DTYPE = np.dtype([("pos", f32, (3,)), ("radius", f32), ("tile", np.int32), ("flags", np.uint32)])
HIT_DTYPE = np.dtype([("pos", f32, (3,)), ("tile", np.int32), ("word", np.uint32), ("nhits", np.uint32)])

TALLY = ("queries", "tested", "no_tile", "distant", "outside", "above", "bad_query", "tile_out_of_range", "looked_up", "hits_pine", "hits_decid", "hits_scenery",
         "queries_hit", "multi_hit_queries", "max_hits", "chain_created", "chain_removed", "chain_created_across", "round_trip_only", "round_trips",
         "gate_exit_pine", "gate_pass_pine", "gate_zero_area_pine", "gate_exit_decid", "gate_pass_decid", "gate_zero_area_decid", "empty_pine", "empty_decid",
         "no_scenery", "short_tree_exit", "short_tree_extended", "bush", "zero_normal", "rock_shape_undecided", "rock_shape_override", "voxel_rock_override",
         "log_in_reach", "mushroom_in_reach", "dropped_pine", "dropped_decid", "rotated", "hits_by_kind", "cube_queries", "cube_hit", "cube_no_tile", "cube_bad",
         "cube_empty", "cube_culled", "cube_leaves_only", "cube_branches_only", "cube_boxes_missed", "cube_sphere_missed", "cube_zero_area")


def new_tally():
    t = {k: 0 for k in TALLY}
    t["hits_by_kind"] = [0] * 9
    return t


def round_fp(v):  # ((val > 0.0f) ? int(val + 0.5f) : int(val - 0.5f))
    v = f32(v)
    return f2i(f32(v + HALF)) if v > ZERO else f2i(f32(v - HALF))


def add(a, b):
    return [f32(a[0] + b[0]), f32(a[1] + b[1]), f32(a[2] + b[2])]


def p2p_dist_xy_sq(a, b):
    return f32(f32(f32(a[0] - b[0]) * f32(a[0] - b[0])) + f32(f32(a[1] - b[1]) * f32(a[1] - b[1])))


def dist_less_than(a, b, dval):
    dval = f32(dval)
    return bool(p2p_dist_sq(a, b) < f32(dval * dval))


def dist_xy_less_than(a, b, dval):
    dval = f32(dval)
    return bool(p2p_dist_xy_sq(a, b) < f32(dval * dval))


def get_norm(v, tally=None):
    vmag = f32(np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))))
    if vmag < TOLERANCE:
        if tally is not None:
            tally["zero_normal"] += 1
        return list(v)
    return [f32(v[0] / vmag), f32(v[1] / vmag), f32(v[2] / vmag)]


def pushed(base, normal, rsum):
    """base + normal*(1.001*rsum): the double product narrows into operator*(T const val)"""
    s = f32(1.001 * float(rsum))
    return [f32(base[0] + f32(normal[0] * s)), f32(base[1] + f32(normal[1] * s)), f32(base[2] + f32(normal[2] * s))]


def sphere_cube_intersect(pos, radius, d):
    dmin, r2 = ZERO, f32(f32(radius) * f32(radius))
    for i in range(3):
        if pos[i] < d[i][0]:
            dist = f32(pos[i] - d[i][0])
            dmin = f32(dmin + f32(dist * dist))
        elif pos[i] > d[i][1]:
            dist = f32(pos[i] - d[i][1])
            dmin = f32(dmin + f32(dist * dist))
        if dmin > r2:
            return False
    return True


def is_zero_area(d):
    return any(d[i][0] == d[i][1] for i in range(3))


def cubes_intersect(a, b):  # a.intersects(b)
    return not any(b[i][1] < a[i][0] or b[i][0] > a[i][1] for i in range(3))


def sphere_vert_cylin_intersect(center, radius, p1, p2, r1, r2, tally=None):
    """-> the moved centre, or None"""
    rsum = f32(radius + cmax(r1, r2))
    if center[2] < cmin(p1[2], p2[2]) or center[2] > cmax(p1[2], p2[2]):
        return None
    if not dist_xy_less_than(p1, center, rsum):
        return None
    normal = get_norm([f32(center[0] - p1[0]), f32(center[1] - p1[1]), ZERO], tally)
    return pushed([p1[0], p1[1], center[2]], normal, rsum)


# ---- the objects: each check_sphere_coll -> the moved centre, or None.  `tally` is None for the what-if evaluations of the chain events
def small_tree_coll(s, center, radius, tally=None):
    if s.type == vm.T_BUSH:
        if tally is not None:
            tally["bush"] += 1
        return None
    if not dist_xy_less_than(center, s.pos, f32(radius + s.r1)):
        return None
    if center[2] > s.p2[2] and f32(center[2] - radius) < s.p2[2]:  # short tree
        if f32(s.p2[2] - s.p1[2]) < radius:
            if tally is not None:
                tally["short_tree_exit"] += 1
            return None
        if tally is not None:
            tally["short_tree_extended"] += 1
        return sphere_vert_cylin_intersect(center, radius, s.p1, [s.p2[0], s.p2[1], f32(s.p2[2] + radius)], s.r1, s.r2, tally)
    return sphere_vert_cylin_intersect(center, radius, s.p1, s.p2, s.r1, s.r2, tally)


def decid_tree_coll(t, br_scale, center, radius, tally=None):
    td = t.td
    rel = sub(center, t.center)
    bb = [f32(x) for x in td["branches_bcube"]]
    if not all(rel[i] > f32(bb[2 * i] - radius) and rel[i] < f32(bb[2 * i + 1] + radius) for i in range(3)):  # contains_pt_exp
        return None
    trunk_radius = f32(0.9 * float(f32(br_scale)) * float(f32(td["base_radius"])))
    trunk_height = cmax(f32(td["sphere_radius"]), f32(td["sphere_center_zoff"]))
    p2 = add(t.center, [ZERO, ZERO, trunk_height])
    return sphere_vert_cylin_intersect(center, radius, t.center, p2, trunk_radius, trunk_radius, tally)


class SceneryObj:
    """a record as its class keeps it; the radius override as terra_tiles_scenery_view defines it"""

    def __init__(self, index, rec, ov):
        self.i, self.kind = index, int(rec["kind"])
        self.pos = [f32(x) for x in rec["pos"]]
        self.overridden = bool(ov is not None and f32(ov) > 0.0)
        self.radius = f32(ov) if self.overridden else f32(rec["radius"])
        self.p = [f32(x) for x in rec["p"]]
        if self.kind == ROCK_SHAPE and self.overridden:
            self.pos[2] = f32(float(self.pos[2]) + 0.1 * float(self.radius))  # pos.z += 0.1*radius (src/scenery.cpp:156)


def scenery_obj_coll(o, center, sphere_radius, tally=None):
    if o.kind in (ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LEAFY):  # scenery_obj::check_sphere_coll
        if o.kind == ROCK_SHAPE and not o.overridden:
            return None  # gen_rock's points give the radius: not decided here
        rsum = f32(o.radius + sphere_radius)
        if not dist_less_than(center, o.pos, rsum):
            return None
        return pushed(o.pos, get_norm(sub(center, o.pos), tally), rsum)
    if o.kind == STUMP:
        radius2, height = o.p[0], o.p[1]
        if not dist_less_than(center, o.pos, f32(cmax(height, cmax(o.radius, radius2)) + sphere_radius)):
            return None
        p1 = [f32(o.pos[0] - ZERO), f32(o.pos[1] - ZERO), f32(o.pos[2] - f32(0.2 * float(height)))]
        return sphere_vert_cylin_intersect(center, sphere_radius, p1, add(o.pos, [ZERO, ZERO, height]), o.radius, o.radius, tally)
    if o.kind == PLANT:
        height = o.p[0]
        if not dist_less_than(center, o.pos, f32(f32(HALF * f32(height + o.radius)) + sphere_radius)):
            return None
        p1 = [f32(o.pos[0] - ZERO), f32(o.pos[1] - ZERO), f32(o.pos[2] - f32(0.1 * float(height)))]
        return sphere_vert_cylin_intersect(center, sphere_radius, p1, add(o.pos, [ZERO, ZERO, height]), o.radius, o.radius, tally)
    return None  # s_log::check_sphere_coll returns 0; mushrooms are not walked


class TileObjects:
    """what a tile_t holds of the three containers, with both all_bcubes as calc_bcube leaves them"""

    def __init__(self, b, t, tally):
        g = b.g
        st = b.stats[t]
        self.tile = tm.Tile(b.sc, b.tiles[t], st, 0.0, 0.0 if b.trmax is None else b.trmax[t], None if b.tile_zmax is None else b.tile_zmax[t], 0, 0)
        fl = 0 if b.flags is None else int(b.flags[t])
        self.is_distant, self.scenery_generated = bool(fl & TILE_DISTANT), not fl & TILE_NO_SCENERY
        self.small, self.decid, self.scenery = [], [], [[] for _ in range(9)]
        vt, dt = vm.new_tally(), dm.new_tally()
        if b.pine is not None and b.pine_counts is not None and b.pine.shape[1]:
            m = min(int(b.pine_counts[t]), b.pine.shape[1])
            for j in range(m):
                s = vm.SmallTree.make(g, b.pine[t, j], None if b.override is None else b.override[t, j])
                if s is None:
                    tally["dropped_pine"] += 1
                else:
                    self.small.append(s)
                    tally["rotated"] += int(s.rotated)
        self.pine_bcube = vm.calc_bcube(self.small, vt)
        if b.decid is not None and b.decid_counts is not None and b.decid.shape[1]:
            m = min(int(b.decid_counts[t]), b.decid.shape[1])
            for j in range(m):
                r = b.decid[t, j]
                tid = int(r["tree_id"])
                if tid < 0 or tid >= len(b.data) or not int(b.data[tid]["flags"]) & dm.GENERATED:
                    tally["dropped_decid"] += 1
                else:
                    self.decid.append(dm.Tree(r, b.data[tid]))
        self.decid_bcube = dm.calc_bcube(self.decid, dt)
        self.undecided = False
        if b.scenery is not None and b.scenery_counts is not None and b.scenery.shape[1]:
            m = min(int(b.scenery_counts[t]), b.scenery.shape[1])
            for j in range(m):  # the stable split of the record list into the reference's vectors
                k = int(b.scenery[t, j]["kind"])
                if 0 <= k < 9:
                    o = SceneryObj(j, b.scenery[t, j], None if b.radius_override is None else b.radius_override[t, j])
                    self.scenery[k].append(o)
                    self.undecided |= k == ROCK_SHAPE and not o.overridden


class Batch:
    """the batch as tile_draw_t holds it.  g: tree_view_model.Globals (the size settings, `instanced` with the table, tree_depth_scale in its args); *_off2: the
    (xoff2, yoff2) each placement ran with"""

    def __init__(self, sc, g, tiles, stats, trmax=None, tile_zmax=None, flags=None, pine=None, pine_counts=None, override=None, decid=None, decid_counts=None, data=None,
                 br_scale=None, scenery=None, scenery_counts=None, radius_override=None, ptree_off2=(0, 0), dtree_off2=(0, 0), scenery_off2=(0, 0), tally=None,
                 scenery_in_record_order=False):
        self.sc, self.g, self.tiles, self.stats, self.trmax, self.tile_zmax, self.flags = sc, g, [tuple(int(x) for x in t) for t in tiles], stats, trmax, tile_zmax, flags
        self.pine, self.pine_counts, self.override, self.decid, self.decid_counts, self.data, self.br_scale = pine, pine_counts, override, decid, decid_counts, data, br_scale
        self.scenery, self.scenery_counts, self.radius_override = scenery, scenery_counts, radius_override
        self.tally = new_tally() if tally is None else tally
        self.scenery_in_record_order = scenery_in_record_order  # what the reference does NOT do: for a case to show that the order matters
        xl = lambda o: [f32(f32(tam.wrap32(sc.dxoff + o[0])) * sc.DX_VAL), f32(f32(tam.wrap32(sc.dyoff + o[1])) * sc.DY_VAL), ZERO]  # tile_offset_t::get_xlate()  # noqa: E731
        self.ptree_xlate, self.dtree_xlate, self.scenery_xlate = xl(ptree_off2), xl(dtree_off2), xl(scenery_off2)
        self.index = {t: i for i, t in enumerate(self.tiles)}
        assert len(self.index) == len(self.tiles), "a tile may appear once"
        with np.errstate(all="ignore"):
            self.objs = [TileObjects(self, t, self.tally) for t in range(len(self.tiles))]

    # ---- get_tile_containing_point
    def tile_pair_at_point(self, x, y):
        sc = self.sc
        ox, oy = f32(f32(sc.dxoff) * sc.DX_VAL), f32(f32(sc.dyoff) * sc.DY_VAL)  # (xoff - xoff2)*DX_VAL
        return (round_fp(f32(f32(HALF * f32(f32(x) - ox)) / sc.g.X_SCENE_SIZE)), round_fp(f32(f32(HALF * f32(f32(y) - oy)) / sc.g.Y_SCENE_SIZE)))

    def tile_for(self, tile, x, y):
        """a query's tile: -1 looks it up from the position, an index names it; -> batch index or -1"""
        tile = int(tile)
        if tile >= 0:
            if tile >= len(self.tiles):
                self.tally["tile_out_of_range"] += 1
                return -1
            return tile
        if tile != -1:
            self.tally["tile_out_of_range"] += 1
            return -1
        self.tally["looked_up"] += 1
        return self.index.get(self.tile_pair_at_point(x, y), -1)

    # ---- tile_t::check_sphere_collision, from `bool coll(0)` on
    def _chain(self, objs, test, center, orig, prior_hits):
        """for (i ..) coll |= i->check_sphere_coll(center, radius), with the chain events: orig is the query's own centre in this container's frame, prior_hits the
        hits of the containers before this one"""
        tally, hits = self.tally, 0
        for o in objs:
            moved = test(o, center, tally)
            if prior_hits + hits > 0:  # the centre has been pushed: what would the query's own centre have met?
                alone = test(o, orig, None) is not None
                if moved is not None and not alone:
                    tally["chain_created"] += 1
                    tally["chain_created_across"] += int(prior_hits > 0)
                elif moved is None and alone:
                    tally["chain_removed"] += 1
            if moved is not None:
                hits += 1
                center = moved
        return center, hits

    def tile_sphere_collision(self, t, pos, sradius, inc_dtrees, inc_ptrees, inc_scenery):
        """-> (pos, word, nhits)"""
        tally, ob = self.tally, self.objs[t]
        pos0 = list(pos)
        word = nhits = 0
        trips = 0
        if inc_ptrees and ob.small:
            pos = sub(pos, self.ptree_xlate)
            trips += 1
            bc = ob.pine_bcube
            if is_zero_area(bc):
                tally["gate_zero_area_pine"] += 1
            if not is_zero_area(bc) and not sphere_cube_intersect(pos, sradius, bc):
                tally["gate_exit_pine"] += 1
            else:
                tally["gate_pass_pine"] += 1
                pos, h = self._chain(ob.small, lambda s, c, ty: small_tree_coll(s, c, sradius, ty), pos, sub(pos0, self.ptree_xlate), 0)
                if h:
                    word |= HIT_PINE
                    nhits += h
                    tally["hits_pine"] += h
            pos = add(pos, self.ptree_xlate)
        elif inc_ptrees:
            tally["empty_pine"] += 1
        if inc_dtrees and ob.decid:
            pos = sub(pos, self.dtree_xlate)
            trips += 1
            bc = ob.decid_bcube
            if is_zero_area(bc):
                tally["gate_zero_area_decid"] += 1
            if not is_zero_area(bc) and not sphere_cube_intersect(pos, sradius, bc):
                tally["gate_exit_decid"] += 1
            else:
                tally["gate_pass_decid"] += 1
                br = lambda tr: f32(1.0) if self.br_scale is None else f32(self.br_scale[tr.tree_id])  # noqa: E731
                pos, h = self._chain(ob.decid, lambda tr, c, ty: decid_tree_coll(tr, br(tr), c, sradius, ty), pos, sub(pos0, self.dtree_xlate), nhits)
                if h:
                    word |= HIT_DECID
                    nhits += h
                    tally["hits_decid"] += h
            pos = add(pos, self.dtree_xlate)
        elif inc_dtrees:
            tally["empty_decid"] += 1
        if inc_scenery and ob.scenery_generated:
            pos = sub(pos, self.scenery_xlate)
            trips += 1
            if ob.undecided:
                word |= ROCK_SHAPE_UNDECIDED
                tally["rock_shape_undecided"] += 1
            orig = sub(pos0, self.scenery_xlate)
            walk = [(k, ob.scenery[k]) for k in WALK]
            if self.scenery_in_record_order:
                walk = [(-1, sorted((o for k in WALK if k != LOG for o in ob.scenery[k]), key=lambda o: o.i))]
            for kind, objs in walk:
                if kind == LOG:  # check_sphere_coll returns 0
                    tally["log_in_reach"] += sum(dist_less_than(pos, o.pos, f32(o.radius + sradius)) for o in objs)
                    continue

                def test(o, c, ty):
                    r = scenery_obj_coll(o, c, sradius, ty)
                    if r is not None and ty is not None:
                        ty["hits_by_kind"][o.kind] += 1
                        ty["rock_shape_override"] += int(o.kind == ROCK_SHAPE)
                        ty["voxel_rock_override"] += int(o.kind == VOXEL_ROCK and o.overridden)
                    return r
                pos, h = self._chain(objs, test, pos, orig, nhits)
                if h:
                    word |= HIT_SCENERY
                    nhits += h
                    tally["hits_scenery"] += h
            tally["mushroom_in_reach"] += sum(dist_less_than(pos, o.pos, f32(cmax(o.p[0], o.radius) + sradius)) for o in ob.scenery[MUSHROOM])
            pos = add(pos, self.scenery_xlate)
        elif inc_scenery:
            tally["no_scenery"] += 1
        tally["round_trips"] += trips
        if nhits == 0 and trips and [x.tobytes() for x in pos] != [f32(x).tobytes() for x in pos0]:
            tally["round_trip_only"] += 1
        return pos, word, nhits

    def sphere_query(self, q):
        """one terra_sphere_query -> (pos, tile, word, nhits)"""
        tally = self.tally
        tally["queries"] += 1
        pos, radius = [f32(x) for x in q["pos"]], f32(q["radius"])

        def leave(stage, tile=-1):
            tally[STAGE_NAMES[stage]] += 1
            return pos, tile, stage << STAGE_SHIFT, 0
        if not all(np.isfinite(x) for x in pos) or not np.isfinite(radius) or radius < 0.0:
            return leave(BAD_QUERY)
        t = self.tile_for(q["tile"], pos[0], pos[1])
        if t < 0:  # can return null for camera during tile generation frames
            return leave(NO_TILE)
        ob = self.objs[t]
        if ob.is_distant:
            return leave(DISTANT, t)
        bc = tm.get_bcube(self.sc, ob.tile)
        if not (pos[0] > bc[0][0] and pos[0] < bc[0][1] and pos[1] > bc[1][0] and pos[1] < bc[1][1]):  # contains_pt_xy
            return leave(OUTSIDE, t)
        if pos[2] > f32(ob.tile.tile_zmax + radius):  # sphere is completely above the tile
            return leave(ABOVE, t)
        tally["tested"] += 1
        fl = int(q["flags"])
        out, word, nhits = self.tile_sphere_collision(t, pos, radius, bool(fl & INC_DTREES), bool(fl & INC_PTREES), bool(fl & INC_SCENERY))
        tally["queries_hit"] += int(nhits > 0)
        tally["multi_hit_queries"] += int(nhits > 1)
        tally["max_hits"] = max(tally["max_hits"], nhits)
        return out, t, word, nhits

    def sphere_collide(self, queries):
        """terra_tiles_sphere_collide -> HIT_DTYPE [nq]"""
        hits = np.zeros(len(queries), HIT_DTYPE)
        with np.errstate(all="ignore"):
            for i, q in enumerate(queries):
                pos, tile, word, nhits = self.sphere_query(q)
                hits[i] = (pos, tile, word, nhits)
        return hits

    # ---- tile_draw_t::check_cube_int_trees
    def cube_query(self, cube, tile=-1):
        """cube: x1 x2 y1 y2 z1 z2 -> (result byte, tile)"""
        tally = self.tally
        tally["cube_queries"] += 1
        d = [[f32(cube[0]), f32(cube[1])], [f32(cube[2]), f32(cube[3])], [f32(cube[4]), f32(cube[5])]]
        if not all(np.isfinite(x) for r in d for x in r):
            tally["cube_bad"] += 1
            return CUBE_BAD_QUERY, -1
        centre = [f32(HALF * f32(d[i][0] + d[i][1])) for i in range(3)]  # get_cube_center()
        t = self.tile_for(tile, centre[0], centre[1])
        if t < 0:
            tally["cube_no_tile"] += 1
            return CUBE_NO_TILE, -1
        ob = self.objs[t]
        if not ob.decid:  # decid_trees.empty()
            tally["cube_empty"] += 1
            return 0, t
        c = [[f32(d[i][0] - self.dtree_xlate[i]), f32(d[i][1] - self.dtree_xlate[i])] for i in range(3)]  # c - dtree_off.get_xlate()
        bc = ob.decid_bcube
        if is_zero_area(bc):
            tally["cube_zero_area"] += 1
        if not is_zero_area(bc) and not cubes_intersect(bc, c):
            tally["cube_culled"] += 1
            return 0, t
        for tr in ob.decid:  # tree::check_cube_int
            rel = [[f32(c[i][0] - tr.center[i]), f32(c[i][1] - tr.center[i])] for i in range(3)]  # c - tree_center
            box = lambda b: [[f32(b[2 * i]), f32(b[2 * i + 1])] for i in range(3)]  # noqa: E731
            il, ib = cubes_intersect(box(tr.td["leaves_bcube"]), rel), cubes_intersect(box(tr.td["branches_bcube"]), rel)
            if not il and not ib:
                tally["cube_boxes_missed"] += 1
                continue
            tally["cube_leaves_only"] += int(il and not ib)
            tally["cube_branches_only"] += int(ib and not il)
            if sphere_cube_intersect([ZERO, ZERO, f32(tr.td["sphere_center_zoff"])], f32(tr.td["sphere_radius"]), rel):  # td.get_center(), td.sphere_radius
                tally["cube_hit"] += 1
                return CUBE_HIT, t
            tally["cube_sphere_missed"] += 1
        return 0, t

    def cube_int_trees(self, cubes, cube_tile=None):
        res, tile = np.zeros(len(cubes), np.uint8), np.zeros(len(cubes), np.int32)
        with np.errstate(all="ignore"):
            for i, c in enumerate(cubes):
                res[i], tile[i] = self.cube_query(c, -1 if cube_tile is None else cube_tile[i])
        return res, tile
