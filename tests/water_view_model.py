"""NumPy / Python float32 restatement of the reflection pass's terrain draw list and of the water quads and water caps of a tile batch, written from the
reference statements (not from the library's bodies):

    tile_draw_t::draw(1) up to its sort, with the filter of :2869              src/tiled_mesh.cpp:2844-2915
    tile_draw_t::can_have_reflection, can_have_reflection_recur               src/tiled_mesh.cpp:2630-2683
    tile_t::get_lod_level(1)                                                  src/tiled_mesh.cpp:1910-1932
    tile_t::is_water_visible, tile_draw_t::draw_water's loop                  src/tiled_mesh.cpp:2131-2133, 3075
    tile_t::draw_water_cap's edge tests and its two callers                   src/tiled_mesh.cpp:2093-2128, 2046, 2078, 2957-2959
    has_water, all_water, get_zmax, get_water_bcube                           src/tiled_mesh.h:206-210, 253-256
    cube_t::closest_pt / clamp_pt, get_cube_center                            src/3DWorld.h:591, 602-604, 636-640
    p2p_dist_xy                                                               src/inlines.h:183-188

The scene, the tiles, the boxes, is_visible, check_line_clip, the occluders and the tally are tests/terrain_view_model.py's; get_lod_level is extended here for
pass 1 (low_detail, :1913-1914).  Types: every statement of can_have_reflection[_recur] and of the water calls is float (np.float32) throughout -- water_plane_z,
the camera, the boxes and z_over_xy are floats and no literal promotes them; `min_normal_z > 0.1` compares in double.  The recursion is the reference's own, with
vis_ref_call; the loop runs in batch order, sequentially, and was_last_occluded() reads what the loop has written so far."""
import numpy as np
import terrain_view_model as tm
import view_model

f32 = np.float32
closest_pt = view_model.closest_pt
NO_REFLECTION = 6
NOT_ASKED, NO_WATER, WALK_NOTHING, HAS_WATER, WALK_FOUND = range(5)
TALLY = tm.TALLY + ("no_reflection", "refl_disabled", "refl_all_water", "refl_has_water", "refl_walk_found", "refl_walk_nothing", "found_x_only", "found_y_only",
                    "found_turn3", "cut_clip0", "cut_clip1", "cut_edge", "cut_absent", "cut_not_visible", "cut_cube", "cut_slope", "cut_occluded", "inside_one",
                    "inside_both", "revisit", "div_zero", "cam_at_water", "walk_levels", "lod_low_detail", "lod_high_detail", "lod_differs_pass2", "state1_on_walk", "state2_on_walk",
                    "written_on_walk", "visits", "crack_to_dropped", "water_listed", "water_far", "water_not_visible", "cap_tiles", "cap_occluded_dry",
                    "cap_adj_near", "cap_adj_far", "cap_adj_missing", "cap_adj_absent")


def new_tally():
    t = {k: 0 for k in TALLY}
    t["walk_levels"] = set()
    return t


class Args(tm.Args):
    def __init__(self, behind_sphere_mult=1.0, zmin=0.0, zmax=0.0, water_enabled=1, check_occlusion=1, reflection_pass=1):
        tm.Args.__init__(self, behind_sphere_mult, zmin, water_enabled, check_occlusion, reflection_pass)
        self.zmin, self.zmax = f32(zmin), f32(zmax)


def make_tiles(sc, tile_xy, stats, min_normal_z, trmax, tile_zmax, flags, occl_state):
    n = len(tile_xy)
    opt = lambda arr, i, d: d if arr is None else arr[i]  # noqa: E731
    tiles = [tm.Tile(sc, tile_xy[i], stats[i], opt(min_normal_z, i, 0.0), opt(trmax, i, 0.0), opt(tile_zmax, i, None), opt(flags, i, 0), opt(occl_state, i, 0)) for i in range(n)]
    for i, t in enumerate(tiles):
        t.wx1, t.wy1, t.wx2, t.wy2 = int(stats[i].wx1), int(stats[i].wy1), int(stats[i].wx2), int(stats[i].wy2)
    return tiles


def has_water(sc, t):
    return bool(t.mzmin < sc.water_plane_z)


def all_water(sc, t):
    return bool(t.mzmax < sc.water_plane_z)


def get_water_bcube(sc, t):
    xv1, yv1 = sc.g.get_xval(t.wx1 + sc.dxoff), sc.g.get_yval(t.wy1 + sc.dyoff)
    return [[xv1, f32(xv1 + f32(f32(t.wx2 - t.wx1) * sc.DX_VAL))], [yv1, f32(yv1 + f32(f32(t.wy2 - t.wy1) * sc.DY_VAL))], [sc.water_plane_z, sc.water_plane_z]]


def p2p_dist_xy(a, b):
    return f32(np.sqrt(tm.p2p_dist_xy_sq(a, b)))


def get_lod_level(sc, v, a, t, tally=None):
    """tile_t::get_lod_level(reflection_pass), pass 1 included"""
    if a.reflection_pass != 1:
        return tm.get_lod_level(sc, v, a, t, tally)
    if t.mzmax == t.mzmin:
        return tm.NUM_LODS - 1
    low_detail = float(t.min_normal_z) > 0.1
    if tally is not None and low_detail:
        tally["lod_low_detail"] += 1
    if tally is not None and not low_detail and float(t.min_normal_z) > 0.0:
        tally["lod_high_detail"] += 1  # min_normal_z on the other side of 0.1, and not the "not given" 0
    lod_level = min(tm.NUM_LODS - 1, 1) if low_detail else 0
    dist = f32(tm.get_rel_dist_to_camera(sc, v, t, False) * f32(tm.TILE_RADIUS))
    if t.flags & tm.FLAG_SHADOW_MAPS:
        dist = f32(dist / f32(2))
    mnz = t.min_normal_z
    if mnz > 0.0:
        if float(mnz) > 0.9:
            if not a.water_enabled or t.mzmax < sc.water_plane_z or t.mzmin > sc.water_plane_z:
                dist = f32(float(dist) * (4.0 if float(mnz) > 0.95 else 2.0))
        elif float(mnz) < 0.25:
            dist = tm.lod_steep_dist(dist, mnz)
    while float(dist) > 1.8 and lod_level + 1 < tm.NUM_LODS and (sc.S >> (lod_level + 1)) >= 4:
        dist = f32(dist / f32(2))
        lod_level += 1
    return lod_level


class Walk:
    """what can_have_reflection_recur reads beside its arguments: the tile map, is_visible(), last_occluded as the loop has left it"""

    def __init__(self, sc, v, a, tiles, index, visible, state, state_in, tally):
        self.sc, self.v, self.a, self.tiles, self.index, self.visible, self.state, self.state_in, self.tally = sc, v, a, tiles, index, visible, state, state_in, tally
        self.vis_ref_call = set()
        self.bcubes = {}

    def bcube(self, i):
        if i not in self.bcubes:
            self.bcubes[i] = tm.get_bcube(self.sc, self.tiles[i])
        return self.bcubes[i]

    def recur(self, i, corners, dim_ix, path):
        sc, tally, t, camera = self.sc, self.tally, self.tiles[i], self.v.pos
        tally["visits"] += 1
        b = self.bcube(i)
        bcube = [list(b[0]), list(b[1]), [view_model.cmin(b[2][0], self.a.zmin), view_model.cmax(b[2][1], self.a.zmax)]]  # make sure the line isn't clipped in z
        if dim_ix < 2 and not tm.check_line_clip(camera, corners[dim_ix], bcube):
            tally["cut_clip%d" % dim_ix] += 1
            return False
        if path:
            if self.state_in[i] in (1, 2):
                tally["state%d_on_walk" % self.state_in[i]] += 1
            if self.state[i] != self.state_in[i]:
                tally["written_on_walk"] += 1
        if has_water(sc, t) and self.state[i] == 1:
            tally["cut_occluded"] += 1
        if not self.state[i] == 1 and has_water(sc, t):  # !was_last_occluded() && has_water()
            water_bcube = get_water_bcube(sc, t)
            if view_model.cube_visible(self.v, water_bcube):
                cp = closest_pt(water_bcube, corners[2])
                with np.errstate(divide="ignore", invalid="ignore"):
                    den = p2p_dist_xy(camera, cp)
                    if den == 0:
                        tally["div_zero"] += 1
                    if camera[2] == sc.water_plane_z:
                        tally["cam_at_water"] += 1
                    z_over_xy = f32(f32(camera[2] - sc.water_plane_z) / den)  # slope
                    if f32(sc.water_plane_z + f32(z_over_xy * p2p_dist_xy(corners[2], cp))) < corners[2][2]:
                        if path and all(d == 0 for d in path):
                            tally["found_x_only"] += 1
                        elif path and all(d == 1 for d in path):
                            tally["found_y_only"] += 1
                        elif len(path) >= 3:
                            tally["found_turn3"] += 1
                        return True
                tally["cut_slope"] += 1
            else:
                tally["cut_cube"] += 1
        if i in self.vis_ref_call:
            tally["revisit"] += 1
            return False  # already seen
        self.vis_ref_call.add(i)
        ret, inside = False, 0
        for d in range(2):
            delta = [0, 0]
            if camera[d] < bcube[d][0]:
                delta[d] = -1
            elif camera[d] > bcube[d][1]:
                delta[d] = 1
            else:
                inside += 1
                continue
            key = (t.tx + delta[0], t.ty + delta[1])
            adj = self.index.get(key)
            if adj is None:
                tally["cut_edge"] += 1
                continue
            if self.tiles[adj].flags & tm.FLAG_ABSENT:
                tally["cut_absent"] += 1
                continue
            if not self.visible[adj]:
                tally["cut_not_visible"] += 1
                continue
            if self.recur(adj, corners, d, path + [d]):
                ret = True
                break
        if inside:
            tally["inside_one" if inside == 1 else "inside_both"] += 1
        self.vis_ref_call.discard(i)
        return ret

    def can_have_reflection(self, i):
        """-> the reflect byte"""
        sc, t, tally = self.sc, self.tiles[i], self.tally
        if not self.a.water_enabled:
            tally["refl_disabled"] += 1
            return NO_WATER
        if all_water(sc, t):
            tally["refl_all_water"] += 1
            return NO_WATER
        if has_water(sc, t):
            tally["refl_has_water"] += 1
            return HAS_WATER
        bcube = self.bcube(i)
        camera, center = self.v.pos, tm.get_cube_center(bcube)
        corners = [[None] * 3 for _ in range(3)]  # {x, y, closest}
        for d in range(2):
            corners[d][d] = bcube[d][1 if center[d] < camera[d] else 0]
            corners[1 - d][d] = bcube[d][1 if center[d] > camera[d] else 0]
            corners[d][2] = bcube[2][0]
        corners[2] = closest_pt(bcube, camera)
        corners[2][2] = t.mzmax  # get_zmax()
        found = self.recur(i, corners, 2, [])
        tally["refl_walk_found" if found else "refl_walk_nothing"] += 1
        return WALK_FOUND if found else WALK_NOTHING


def camera_tile(sc, v):
    """the tile position that holds the camera (only for the tally's count of distinct |dx| + |dy| among the walking tiles)"""
    w = float(f32(sc.S) * sc.DX_VAL)
    x0, y0 = float(sc.g.get_xval(sc.dxoff)), float(sc.g.get_yval(sc.dyoff))
    return int(np.floor((float(v.pos[0]) - x0) / w)), int(np.floor((float(v.pos[1]) - y0) / w))


def draw(sc, v, a, tile_xy, stats, min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None, tally=None):
    """tile_draw_t::draw(1) -> (status, dist, lod, crack, draw_order list, occluded list, occl_state after the call, reflect [n] uint8)"""
    assert a.reflection_pass == 1
    tally = new_tally() if tally is None else tally
    n = len(tile_xy)
    tiles = make_tiles(sc, tile_xy, stats, min_normal_z, trmax, tile_zmax, flags, occl_state)
    status, dist, lod, crack = np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, np.uint8), np.full((n, 4), tm.NO_CRACK, np.uint8)
    reflect = np.zeros(n, np.uint8)
    state = np.array([t.state for t in tiles], np.uint8)
    state_in = state.copy()
    present = [i for i in range(n) if not tiles[i].flags & tm.FLAG_ABSENT]
    tally["absent"] += n - len(present)
    camera = v.pos
    visible = {i: tm.is_visible(sc, v, a, tiles[i], tally) for i in present}
    index = {(tiles[i].tx, tiles[i].ty): i for i in range(n)}
    occluders = []
    if a.check_occlusion:
        for i in present:
            t = tiles[i]
            if not t.flags & tm.FLAG_NO_OCCLUDER and tm.rel_dist_to_camera_xy_lt(sc, v, t, tm.OCCLUDER_DIST) and visible[i]:  # use_as_occluder()
                occluders.append(tm.Occluder(sc, v, a, t, i, tally))
                status[i] |= tm.WAS_OCCLUDER
    tally["occluders"] += len(occluders)
    walk = Walk(sc, v, a, tiles, index, visible, state, state_in, tally)
    ctx, cty = camera_tile(sc, v)
    pass2 = tm.Args(a.behind_sphere_mult, a.occluder_zmin, a.water_enabled, a.check_occlusion, 2)
    to_draw, occluded_tiles = [], []
    for i in present:
        t = tiles[i]
        dist[i] = tm.get_rel_dist_to_camera(sc, v, t)
        lod[i] = get_lod_level(sc, v, a, t, tally)
        if lod[i] != tm.get_lod_level(sc, v, pass2, t):
            tally["lod_differs_pass2"] += 1
        if t.mzmax != t.mzmin:
            tally["max_lod_not_flat"] = max(tally["max_lod_not_flat"], int(lod[i]))
        else:
            tally["lod_flat"] += 1
        if dist[i] > tm.DRAW_DIST_TILES:
            status[i] |= tm.TOO_FAR
            continue
        if not visible[i]:
            status[i] |= tm.NOT_VISIBLE
            continue
        if state[i] == 1:  # was_last_occluded()
            status[i] |= tm.OCCLUDED_BEFORE
            continue
        reflect[i] = walk.can_have_reflection(i)  # :2869
        if reflect[i] in (WALK_FOUND, WALK_NOTHING):
            tally["walk_levels"].add(abs(t.tx - ctx) + abs(t.ty - cty))
        if reflect[i] < HAS_WATER:
            status[i] |= NO_REFLECTION
            continue
        if occluders and t.state == 2:
            tally["test_skipped_state"] += 1
        if occluders and t.state != 2:  # !was_last_unoccluded()
            tally["tested"] += 1
            tile_pts = tm.cube_top_points(tm.get_bcube(sc, t))
            occluder_ixs = [j for j, oc in enumerate(occluders) if oc.index != i and any(tm.check_line_clip(p, camera, oc.bcube) for p in tile_pts)]
            tile_occluded = True
            for q in range(16):
                sub_cube = tm.get_sub_bcube(sc, t, q >> 2, q & 3)
                pts, center = tm.cube_top_points(sub_cube), tm.get_cube_center(sub_cube)
                sub_tile_occluded = False
                for j in occluder_ixs:
                    if sub_tile_occluded:
                        break
                    oc = occluders[j]
                    if not tm.check_line_clip(center, camera, oc.bcube):
                        continue
                    for s in range(16):
                        if sub_tile_occluded:
                            break
                        occ = oc.sub_cubes[s]
                        if tm.is_all_zeros(occ):
                            continue
                        sub_tile_occluded = all(tm.check_line_clip(p, camera, occ) for p in pts)
                if not sub_tile_occluded:
                    tile_occluded = False
                    break
            state[i] = 1 if tile_occluded else 2  # set_last_occluded
            if tile_occluded:
                occluded_tiles.append(i)
                status[i] |= tm.OCCLUDED
                continue
        to_draw.append((float(dist[i]), i))
        status[i] |= tm.DRAWN
    to_draw.sort()
    ds = [d for d, _ in to_draw]
    tally["ties"] += sum(1 for k in range(1, len(ds)) if ds[k] == ds[k - 1])
    pindex = {(tiles[i].tx, tiles[i].ty): i for i in present}
    for _, i in to_draw:
        t = tiles[i]
        for dim in range(2):
            for dir in range(2):
                dx, dy = ((1 if dir else -1), 0) if dim == 0 else (0, (1 if dir else -1))
                adj = pindex.get((t.tx + dx, t.ty + dy))
                if adj is None:
                    tally["no_neighbour"] += 1
                    continue
                crack[i, 2 * dim + dir] = tm.crack_index(dim, dir, int(lod[i]), int(lod[adj]))
                if (status[adj] & 7) == NO_REFLECTION:
                    tally["crack_to_dropped"] += 1
                tally["adj_lower" if lod[adj] < lod[i] else "adj_equal" if lod[adj] == lod[i] else "adj_higher"] += 1
    for k, name in ((tm.TOO_FAR, "too_far"), (tm.NOT_VISIBLE, "not_visible"), (tm.OCCLUDED_BEFORE, "occluded_before"), (tm.OCCLUDED, "occluded"), (tm.DRAWN, "drawn"),
                    (NO_REFLECTION, "no_reflection")):
        tally[name] += int(((status & 7) == k).sum())
    return status, dist, lod, crack, [i for _, i in to_draw], occluded_tiles, state, reflect


def water(sc, v, a, tile_xy, stats, trmax=None, tile_zmax=None, flags=None, status=None, tally=None):
    """tile_draw_t::draw_water's loop and draw_water_cap's edge tests -> (water_list, cap_mask [n] uint8 or None)"""
    tally = new_tally() if tally is None else tally
    n = len(tile_xy)
    tiles = make_tiles(sc, tile_xy, stats, None, trmax, tile_zmax, flags, None)
    present = [i for i in range(n) if not tiles[i].flags & tm.FLAG_ABSENT]
    index = {(tiles[i].tx, tiles[i].ty): i for i in range(n)}
    water_list = []
    for i in present:  # draw_water: is_water_visible() (is_distant is 0)
        t = tiles[i]
        if not has_water(sc, t):
            continue
        if not tm.rel_dist_to_camera_xy_lt(sc, v, t, tm.DRAW_DIST_TILES):
            tally["water_far"] += 1
            continue
        if not tm.is_visible(sc, v, a, t):
            tally["water_not_visible"] += 1
            continue
        water_list.append(i)
    tally["water_listed"] += len(water_list)
    if status is None:
        return water_list, None
    cap_mask = np.zeros(n, np.uint8)
    for i in present:
        t, me = tiles[i], int(status[i]) & 7
        if not a.water_enabled:
            continue
        if not ((me == tm.DRAWN and has_water(sc, t)) or me == tm.OCCLUDED):  # draw_near_water (:2046, :2078); occluded_tiles (:2957-2959)
            continue
        for dim in range(2):
            for dir in range(2):
                dxy = [0, 0]
                dxy[dim] = 1 if dir else -1
                adj = index.get((t.tx + dxy[0], t.ty + dxy[1]))
                if adj is None:
                    tally["cap_adj_missing"] += 1
                elif tiles[adj].flags & tm.FLAG_ABSENT:
                    tally["cap_adj_absent"] += 1
                    adj = None
                if adj is not None:
                    at = tiles[adj]
                    if tm.rel_dist_to_camera_xy_lt(sc, v, at, tm.DRAW_DIST_TILES):
                        tally["cap_adj_near"] += 1
                        continue
                    tally["cap_adj_far"] += 1
                    if not has_water(sc, at):
                        continue
                    if not tm.is_visible(sc, v, a, at):
                        continue
                cap_mask[i] |= 1 << (2 * dim + dir)
        if cap_mask[i]:
            tally["cap_tiles"] += 1
            if me == tm.OCCLUDED and not has_water(sc, t):
                tally["cap_occluded_dry"] += 1
    return water_list, cap_mask
