"""NumPy / Python float32 restatement of the shadow-map plan of a tile batch, written from the reference statements (not from the library's bodies):

    tile_t::update_range's shadow-map deletion                               src/tiled_mesh.cpp:1409, 1416
    the loop of tile_draw_t::pre_draw (its shadow part)                      src/tiled_mesh.cpp:2781-2799
    tile_t::setup_shadow_maps, calc_max_smap_lod, tile_t::get_shadow_bcube   src/tiled_mesh.cpp:981-1016, 975-980, 959-965
    the gate of tile_t::try_bind_shadow_map                                  src/tiled_mesh.cpp:1958-1959
    the recompute queue and its consumption                                  src/tiled_mesh.cpp:2445-2448, 2459
    the head of tile_draw_t::draw_shadow_pass, draw_tiles_shadow_pass's
      filter, tile_t::draw_shadow_pass's inside_city return                  src/tiled_mesh.cpp:3025-3043, 3004-3018, 2083
    SMAP_NEW_THRESH, SMAP_DEL_THRESH, SMAP_FADE_THRESH, NUM_SMAP_LODS         src/tiled_mesh.cpp:30-32; src/tiled_mesh.h:26
    is_smap_bounds_visible, get_dist_to_camera_in_tiles, tile_xy_pair         src/tiled_mesh.h:331-332, 98-104
    cube_t::intersects_xy, contains_pt_xy, get_bsphere_radius                src/3DWorld.h:544-547, 579, 605-607
    get_pt_cube_frustum_pdu (the infinite-terrain form)                      src/shadow_map.cpp:423-457
    get_min_dim, get_cube_corners, pointT::get_norm, operator/               src/inlines.h:630-632; src/Math3d.cpp:1184-1193; src/3DWorld.h:297-300, 315-319

Every shared primitive is tests/view_model.py's (the view, the sphere and cube tests, the vectors), the tile's centre, boxes, distances and is_visible are
tests/terrain_view_model.py's: this module keeps no body of them.  Types: np.float32 for float, Python float for double, Python int for int / unsigned.  Which
sub-expressions are double: `smap_dist_scale < 1.0`, `1.0 + 0.5*bounds.dz()/dist` (narrowed into the float frustum_skew_val) and operator/'s `1.0/val` (narrowed
into the float val_inv).  floor() is the float overload; unsigned(float) is the x86-64 conversion.  atan2f is the C library's, called through ctypes.

The state of a tile is one byte: NONE for smap_data.empty(), else smap_lod_level.  The tally counts what each statement decided, so that a case can show that it
exercises what it is named for."""
import ctypes

import numpy as np

import terrain_view_model as tm
import view_model

f32 = np.float32
SMAP_NEW_THRESH, SMAP_DEL_THRESH, SMAP_FADE_THRESH = f32(1.2), f32(1.3), f32(1.5)
NUM_SMAP_LODS = 4
NONE = 0xFF
(IN_DRAW_DIST, VISIBLE, BOUNDS_VISIBLE, UPDATE, CLEARED_FAR, CLEARED_WIREFRAME, CLEARED_LOD_REDUCE, CLEARED_LOD_RAISE, ALLOCATED, RECEIVER, USABLE) = (1 << k for k in range(11))
LOD_SHIFT, REDUCE_SHIFT = 16, 20
FLAG_FULLY_IN_CITY = 8
CAST_NO_TILE = 1
ZERO, HALF = f32(0.0), f32(0.5)
cmax, cmin, sub, dot, cross, mag_sq = view_model.cmax, view_model.cmin, view_model.sub, view_model.dot, view_model.cross, view_model.mag_sq

_libm = view_model._libm
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]

TALLY = ("present", "absent", "beyond_draw", "visible", "bounds_only", "cleanup_only", "cleared_far", "cleared_wireframe", "cleared_reduce", "cleared_raise", "cleanup_cleared",
         "allocated", "alloc_lod0", "alloc_lod1", "alloc_lod2", "alloc_lod3", "receiver", "kept", "hysteresis_kept", "usable", "not_usable_far", "band_new", "band_del", "band_fade",
         "band_beyond", "large_outside", "large_inside", "large_no_hysteresis", "models", "disabled", "flag_set", "flag_kept", "recomp", "recomp_dist_ties", "water_radius", "water_z2",
         "invalid_view_tests", "sphere_rejected", "sphere_all", "cube_accepted", "cube_rejected", "behind_true", "behind_false", "renders", "no_tile", "in_to_draw", "not_visible", "nearer", "at_recv_dist", "overlap_only", "fails_both", "in_city", "no_decid", "terrain")


def new_tally():
    return {k: 0 for k in TALLY}


class PlanArgs:
    def __init__(self, behind_sphere_mult=1.0, water_enabled=1, smap_thresh_scale=1.0, shadow_map_sz=4096, have_buildings=0, draw_model=0, b_ext=(0.0, 0.0, 0.0), road_len=(0.0, 0.0),
                 models_z2=0.0, models_valid=0, sun_pos=(0.0, 0.0, 1.0), want_recomp=0):
        self.behind_sphere_mult, self.water_enabled, self.smap_thresh_scale = f32(behind_sphere_mult), int(water_enabled), f32(smap_thresh_scale)
        self.shadow_map_sz, self.have_buildings, self.draw_model = int(shadow_map_sz), int(have_buildings), int(draw_model)
        self.b_ext, self.road_len = [f32(x) for x in b_ext], [f32(x) for x in road_len]
        self.models_z2, self.models_valid, self.sun_pos, self.want_recomp = f32(models_z2), int(models_valid), [f32(x) for x in sun_pos], int(want_recomp)


class CastArgs:
    def __init__(self, water_enabled=1, decid_trees_only=0, inc_adj_smap=0, b_ext=(0.0, 0.0, 0.0), road_len=(0.0, 0.0)):
        self.water_enabled, self.decid_trees_only, self.inc_adj_smap = int(water_enabled), int(decid_trees_only), int(inc_adj_smap)
        self.b_ext, self.road_len = [f32(x) for x in b_ext], [f32(x) for x in road_len]


class _Vis:
    """what terrain_view_model.is_visible reads of its args"""

    def __init__(self, behind_sphere_mult, water_enabled):
        self.behind_sphere_mult, self.water_enabled = f32(behind_sphere_mult), int(water_enabled)


def get_shadow_bcube(sc, a, t):
    """:959-965"""
    xv1, yv1, xv2, yv2 = tm.corner(sc, t)
    x_ext = cmax(cmax(f32(HALF * a.road_len[0]), a.b_ext[0]), t.trmax)
    y_ext = cmax(cmax(f32(HALF * a.road_len[1]), a.b_ext[1]), t.trmax)
    return [[f32(xv1 - x_ext), f32(xv2 + x_ext)], [f32(yv1 - y_ext), f32(yv2 + y_ext)],
            [f32(t.mzmin - tm.BCUBE_ZTOLER), cmax(f32(t.tile_zmax + tm.BCUBE_ZTOLER), f32(t.mzmax + a.b_ext[2]))]]


def calc_max_smap_lod(a):
    """:975-980"""
    min_smap_sz = 1024 if a.have_buildings else 512
    lod_level, smap_sz = 0, a.shadow_map_sz
    while smap_sz > min_smap_sz and lod_level + 1 < NUM_SMAP_LODS:
        smap_sz >>= 1
        lod_level += 1
    return lod_level


def get_dist_to_camera_in_tiles(sc, v, t):
    return f32(tm.get_rel_dist_to_camera(sc, v, t, True) * f32(tm.TILE_RADIUS))


def _tiles(sc, tiles, stats, trmax, tile_zmax, flags):
    n = len(tiles)
    return [tm.Tile(sc, tiles[i], stats[i], 0.0, 0.0 if trmax is None else trmax[i], None if tile_zmax is None else tile_zmax[i], 0 if flags is None else flags[i], 0) for i in range(n)]


def plan(sc, v, a, tiles, stats, smap_state, trmax=None, tile_zmax=None, flags=None, terrain_flags=None, tally=None):
    """one frame.  -> dict(plan [n], dist_scale [n], box {t: 6 floats} (the tiles inside the draw distance), receivers (list), smap_state [n] after the call,
    terrain_flags [n] after the call or None, recomp_order (list) or None)"""
    tally = tally if tally is not None else new_tally()
    n = len(tiles)
    T = _tiles(sc, tiles, stats, trmax, tile_zmax, flags)
    vis = _Vis(a.behind_sphere_mult, a.water_enabled)
    enabled = a.shadow_map_sz != 0
    state = [int(x) for x in smap_state]
    words, scale, box, receivers = np.zeros(n, np.uint32), np.zeros(n, f32), {}, []
    tf = None if terrain_flags is None else np.array(terrain_flags, np.uint8)
    queue = []
    for i, t in enumerate(T):
        if t.flags & tm.FLAG_ABSENT:
            tally["absent"] += 1
            continue
        tally["present"] += 1
        w = 0
        # update_range (:1409, :1416)
        dist = tm.get_rel_dist_to_camera(sc, v, t, True)
        if f32(dist * f32(tm.TILE_RADIUS)) > f32(SMAP_DEL_THRESH * a.smap_thresh_scale):
            if state[i] != NONE:
                w |= CLEARED_FAR
                tally["cleared_far"] += 1
            state[i] = NONE
        in_tiles = get_dist_to_camera_in_tiles(sc, v, t)
        # pre_draw's loop (:2784-2791)
        if not tm.rel_dist_to_camera_xy_lt(sc, v, t, tm.DRAW_DIST_TILES):
            tally["beyond_draw"] += 1
        else:
            w |= IN_DRAW_DIST
            if in_tiles < f32(SMAP_NEW_THRESH * a.smap_thresh_scale):
                tally["band_new"] += 1
            elif not in_tiles > f32(SMAP_DEL_THRESH * a.smap_thresh_scale):
                tally["band_del"] += 1
            elif not in_tiles > f32(SMAP_FADE_THRESH * a.smap_thresh_scale):
                tally["band_fade"] += 1
            else:
                tally["band_beyond"] += 1
            is_visible = tm.is_visible(sc, v, vis, t, tally)
            sb = get_shadow_bcube(sc, a, t)
            bounds = view_model.cube_visible(v, sb)  # is_smap_bounds_visible()
            if is_visible:
                w |= VISIBLE
                tally["visible"] += 1
            if bounds:
                w |= BOUNDS_VISIBLE
                if not is_visible:
                    tally["bounds_only"] += 1
            if a.models_valid:  # :1013-1014
                sb[2][1] = cmax(sb[2][1], a.models_z2)
                tally["models"] += 1
            box[i] = [sb[0][0], sb[0][1], sb[1][0], sb[1][1], sb[2][0], sb[2][1]]
            if not enabled:
                tally["disabled"] += 1
            else:
                cleanup_only = not (is_visible or bounds)
                if cleanup_only:
                    tally["cleanup_only"] += 1
                else:
                    w |= UPDATE
                # setup_shadow_maps (:981-1016)
                if a.draw_model != 0:
                    if state[i] != NONE:
                        w |= CLEARED_WIREFRAME
                        tally["cleared_wireframe"] += 1
                    state[i] = NONE
                else:
                    smap_dist_scale = f32(in_tiles / f32(SMAP_NEW_THRESH * a.smap_thresh_scale))
                    scale[i] = smap_dist_scale
                    if float(smap_dist_scale) < 1.0:
                        max_lod_level = calc_max_smap_lod(a)
                        lod_level_f = cmin(f32(f32(5.0) * smap_dist_scale), f32(max_lod_level))
                        lod_level = view_model.f2u(np.floor(lod_level_f))
                        lod_level_reduce = view_model.f2u(np.floor(cmax(ZERO, f32(lod_level_f - f32(0.1)))))
                        if a.shadow_map_sz >= 8192:
                            mb = tm.get_mesh_bcube(sc, t)
                            inside = bool(v.pos[0] > mb[0][0] and v.pos[0] < mb[0][1] and v.pos[1] > mb[1][0] and v.pos[1] < mb[1][1])  # contains_pt_xy
                            tally["large_inside" if inside else "large_outside"] += 1
                            if not inside:
                                if lod_level == 0:
                                    lod_level_reduce = 1
                                    tally["large_no_hysteresis"] += 1
                                lod_level = min(lod_level + 1, max_lod_level)
                        w |= (lod_level << LOD_SHIFT) | (lod_level_reduce << REDUCE_SHIFT)
                        held = state[i] != NONE
                        if state[i] != NONE and lod_level_reduce > state[i]:
                            w |= CLEARED_LOD_REDUCE
                            tally["cleared_reduce"] += 1
                            if cleanup_only:
                                tally["cleanup_cleared"] += 1
                            state[i] = NONE
                        elif held and lod_level > state[i]:
                            tally["hysteresis_kept"] += 1  # lod_level_f lies within 0.1 above the next level: no clear
                        if not cleanup_only:
                            if state[i] != NONE and lod_level < state[i]:
                                w |= CLEARED_LOD_RAISE
                                tally["cleared_raise"] += 1
                                state[i] = NONE
                            if state[i] == NONE:
                                w |= ALLOCATED
                                state[i] = lod_level
                                tally["allocated"] += 1
                                tally["alloc_lod%d" % lod_level] += 1
                            elif held:
                                tally["kept"] += 1
                    if not cleanup_only and state[i] != NONE:
                        w |= RECEIVER
                        receivers.append(i)
                        tally["receiver"] += 1
        # try_bind_shadow_map's gate (:1958-1959)
        if enabled and state[i] != NONE:
            if in_tiles > f32(SMAP_FADE_THRESH * a.smap_thresh_scale):
                tally["not_usable_far"] += 1
            else:
                w |= USABLE
                tally["usable"] += 1
        words[i] = w
        if tf is not None and state[i] != NONE:
            tally["flag_kept" if int(tf[i]) & ~tm.FLAG_SHADOW_MAPS else "flag_set"] += 1
            tf[i] |= tm.FLAG_SHADOW_MAPS
        if a.want_recomp:  # :2446
            c = tm.get_center(sc, t)
            queue.append((f32(-f32(np.sqrt(view_model.p2p_dist_sq(a.sun_pos, c)))), (t.ty, t.tx), i))
    order = None
    if a.want_recomp:
        queue.sort(key=lambda q: (q[0], q[1]))  # std::pair's operator< over (float, tile_xy_pair); tile_xy_pair compares y, then x
        tally["recomp"] += len(queue)
        tally["recomp_dist_ties"] += sum(1 for k in range(1, len(queue)) if queue[k][0] == queue[k - 1][0])
        order = [q[2] for q in reversed(queue)]  # pop_back (:2459)
    return dict(plan=words, dist_scale=scale, box=box, receivers=receivers, smap_state=np.array(state, np.uint8), terrain_flags=tf, recomp_order=order,
                present=np.array([0 if t.flags & tm.FLAG_ABSENT else 1 for t in T], np.uint8))


def casters(sc, a, tiles, stats, recv, views, bsm, lpos, trmax=None, tile_zmax=None, flags=None, decid_counts=None, tally=None):
    """R renders.  -> dict(to_draw: R lists, terrain: R lists, not_drawn uint8 [R, n], status uint8 [R])"""
    tally = tally if tally is not None else new_tally()
    n, R = len(tiles), len(recv)
    T = _tiles(sc, tiles, stats, trmax, tile_zmax, flags)
    pa = PlanArgs(b_ext=a.b_ext, road_len=a.road_len)
    to_draw, terrain, not_drawn, status = [], [], np.ones((R, n), np.uint8), np.zeros(R, np.uint8)
    for r in range(R):
        tally["renders"] += 1
        td, te = [], []
        to_draw.append(td)
        terrain.append(te)
        ri = int(recv[r])
        if ri < 0 or ri >= n or (T[ri].flags & tm.FLAG_ABSENT):
            status[r] = CAST_NO_TILE
            tally["no_tile"] += 1
            continue
        v = views[r]
        light = view_model.View(v.pos, v.dir, v.upv_, v.cp, v.sterm, v.x_sterm, 0.0, v.far_, v.valid)  # camera_pdu.near_ = 0.0 (:3032)
        vis = _Vis(bsm[r], a.water_enabled)
        lp = [f32(x) for x in lpos[r]]
        tile = T[ri]
        recv_dist_sq = tm.p2p_dist_xy_sq(lp, tm.get_center(sc, tile))  # :3004
        shadow_bcube = get_shadow_bcube(sc, pa, tile)                  # :3005
        for i, t in enumerate(T):  # :3037-3043
            if t.flags & tm.FLAG_ABSENT:
                continue
            if a.decid_trees_only and int(decid_counts[i]) == 0:
                tally["no_decid"] += 1
                continue
            if not tm.is_visible(sc, light, vis, t, tally):
                tally["not_visible"] += 1
                continue
            td.append(i)
            not_drawn[r, i] = 0
            tally["in_to_draw"] += 1
            if a.decid_trees_only:  # :3046
                continue
            d = tm.p2p_dist_xy_sq(lp, tm.get_center(sc, t))
            nearer = bool(d <= recv_dist_sq)  # :3013
            bc = tm.get_bcube(sc, t)
            overlap = bool(a.inc_adj_smap) and not any(shadow_bcube[k][1] < bc[k][0] or shadow_bcube[k][0] > bc[k][1] for k in (0, 1))  # :3014: intersects_xy
            if nearer:
                tally["nearer"] += 1
                if d == recv_dist_sq and i != ri:
                    tally["at_recv_dist"] += 1
            elif overlap:
                tally["overlap_only"] += 1
            else:
                tally["fails_both"] += 1
                continue
            if t.flags & FLAG_FULLY_IN_CITY:  # :2083
                tally["in_city"] += 1
                continue
            te.append(i)
            tally["terrain"] += 1
    return dict(to_draw=to_draw, terrain=terrain, not_drawn=not_drawn, status=status)


def get_min_dim(v):
    """src/inlines.h:630-632"""
    a0, a1, a2 = abs(v[0]), abs(v[1]), abs(v[2])
    return ((0 if a0 < a2 else 2) if a0 < a1 else (1 if a1 < a2 else 2))


def make_light_view(lpos, bounds, near_clip=0.01):
    """get_pt_cube_frustum_pdu (src/shadow_map.cpp:423-457) with world_mode == WMODE_INF_TERRAIN -> (View, behind_sphere_mult), or None where it asserts"""
    b = [f32(x) for x in bounds]
    near_clip = f32(near_clip)
    if not (b[0] < b[1] and b[2] < b[3] and b[4] < b[5]):
        return None
    center = [f32(HALF * f32(b[0] + b[1])), f32(HALF * f32(b[2] + b[3])), f32(HALF * f32(b[4] + b[5]))]
    pos = [f32(f32(x) * f32(10.0)) for x in lpos]
    dist = f32(np.sqrt(view_model.p2p_dist_sq(pos, center)))
    if dist == 0.0:
        return None
    val_inv = f32(1.0 / float(dist))
    light_dir = [f32(x * val_inv) for x in sub(center, pos)]
    up_dir = [ZERO, ZERO, ZERO]
    up_dir[get_min_dim(light_dir)] = f32(1.0)
    size = [f32(b[1] - b[0]), f32(b[3] - b[2]), f32(b[5] - b[4])]
    radius = f32(HALF * f32(np.sqrt(mag_sq(size))))
    d1 = cross(light_dir, cross(up_dir, light_dir))  # orthogonalize_dir(up_dir, light_dir, dirs[1], 1)
    m = f32(np.sqrt(mag_sq(d1)))
    if m >= view_model.TOLERANCE:
        mi = f32(1.0 / float(m))
        d1 = [f32(x * mi) for x in d1]
    d0 = cross(light_dir, d1)
    rx = ry = ZERO
    with np.errstate(all="ignore"):
        for i in range(8):
            delta = sub([b[i >> 2], b[2 + ((i >> 1) & 1)], b[4 + (i & 1)]], pos)
            vmag = f32(np.sqrt(mag_sq(delta)))
            if not vmag < view_model.TOLERANCE:
                delta = [f32(x / vmag) for x in delta]
            rx, ry = cmax(rx, abs(dot(d0, delta))), cmax(ry, abs(dot(d1, delta)))
        frustum_skew_val = f32(1.0 + 0.5 * float(size[2]) / float(dist))
        angle = f32(_libm.atan2f(f32(frustum_skew_val * ry), f32(1.0)))
        aspect = f32(rx / ry)
    if not (np.isfinite(angle) and np.isfinite(aspect)) or aspect == 0.0:
        return None
    v = view_model.make_view(pos, light_dir, up_dir, angle, aspect, cmax(near_clip, f32(dist - radius)), f32(cmax(near_clip, dist) + radius))
    if v is None:
        return None
    return v, view_model.behind_sphere_mult(angle, aspect)
