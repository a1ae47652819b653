"""NumPy / Python float32 restatement of the scenery draw lists of a tile batch for a camera, written from the reference statements (not from the library's bodies):

    tile_t::draw_scenery (without its GL, shader and colour calls)             src/tiled_mesh.cpp:1580-1592
    get_scenery_thresh, get_scenery_dist_scale, get_dist_to_camera_in_tiles    src/tiled_mesh.h:332-334
    get_tile_width                                                             src/tiled_mesh.h:93
    scenery_group::draw_plant_leaves, draw_opaque_objects                      src/scenery.cpp:1413-1500
    rock_shape3d::draw, surface_rock::draw, s_rock::draw, voxel_rock::draw     src/scenery.cpp:300-305, 394-417, 442-461, 517-530
    s_log::draw, s_stump::draw                                                 src/scenery.cpp:606-632, 670-693
    s_plant::draw_stem, draw_leaves, draw_berries                              src/scenery.cpp:853-871, 898-934
    leafy_plant::draw_leaves, mushroom::draw                                   src/scenery.cpp:1030-1045, 1062-1081
    scenery_obj::check_visible, is_visible, get_size_scale                     src/scenery.cpp:122-135 (scale_exp = 8.0, src/shape_line3d.h:22)
    get_pt_line_thresh, skip_uw_draw, can_skip_small_shadow_objs' use          src/scenery.cpp:61-74, 1471
    the get_bsphere_radius() overrides                                         src/scenery.h:120, 132, 166, 199, 221
    approx_pixel_width's use, get_smap_ndiv, get_def_smap_ndiv                 src/shadow_map.cpp:57-64
    distance_to_camera, dot_product_ptv                                        src/inlines.h:227, 431

The tile's centre and distance are tests/terrain_view_model.py's, the sphere test (with its tally of the planes), int(double) and int(float)
tests/view_model.py's.  Types: np.float32 for float, np.float64 for double, Python int for int.  Which sub-expressions are double: PT_LINE_THRESH*(do_zoom ?
ZOOM_FACTOR : 1.0) (narrowed by the float return), (do_zoom ? ZOOM_FACTOR : 1.0)*window_width (then int, then the float parameter sscale), 1.3*radius (narrowed by
the float parameter), 2.0*sscale*radius/dist, 2.2*sscale*radius/dist, 1.0*sscale*radius/dist, 2.0*radius and 2.2*radius (narrowed by get_def_smap_ndiv's float
parameter), 0.5*radius/approx_pixel_width, 0.75*get_pt_line_thresh()*radius, 1000.0*radius, 0.5*height (narrowed by point's constructor), 0.1*(abs + abs),
2.0*size_scale, size_scale < 1.2, dist_scale > 1.0, pos.z += 0.1*radius.  Float: 2*get_pt_line_thresh()*radius, get_pt_line_thresh()*(radius + radius2),
sscale*radius/dist of s_rock, 0.5f*(..), cap_zscale*radius, (pos + pt2)*0.5 (pointT::operator*(T)).  pow(float, float) is libm's powf, taken from the C library.
In tiled-terrain mode check_visible is sphere_visible_test alone, and so is sphere_in_camera_view(.., 2) (src/visibility.cpp:338-339).

The reference keeps one vector per kind; a stable split of the record list by `kind` reproduces each.  The model walks those vectors in the order of
draw_opaque_objects and draw_plant_leaves and appends to the lists as the reference issues its draws, the two pt_line_drawer lists included.

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import collections
import ctypes

import numpy as np

import terrain_view_model as tm
import view_model

f32, f64 = np.float32, np.float64
LEAFY_PLANT, PLANT, ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LOG, STUMP, MUSHROOM = range(9)  # TERRA_SCENERY_*
KIND_NAMES = ("leafy_plant", "plant", "rock_shape", "surface_rock", "voxel_rock", "rock", "log", "stump", "mushroom")
NUM_LAND_PLANT_TYPES = 6
N_CYL_SIDES = N_SPHERE_DIV = 32
PT_LINE_THRESH, SCENERY_THRESH, SCENERY_THRESH_REF = f32(800.0), f32(5.0), f32(2.0)
NONE, POINT, LINE, POLY, ENGINE = 0, 1, 2, 3, 7
LOG_END, LOG_END2, STUMP_TOP, CAP_UNDERSIDE, LEAVES, UNDERWATER, BERRIES = 0x8, 0x10, 0x20, 0x40, 0x80, 0x4000, 0x8000
NDIV_SHIFT, BERRY_NDIV_SHIFT = 8, 16
TILE_DRAWN, TILE_OPAQUE, TILE_LEAVES = 1, 2, 4
G_ROCK_SHAPE, G_SURFACE_ROCK, G_ROCK, G_LOG, G_STUMP, G_MUSHROOM, G_STEM, G_BERRIES, G_VOXEL_ROCK, G_PLANT_LEAVES, G_LEAFY_LEAVES, G_PLD_POINTS, G_PLD_LINES = range(13)
GROUPS = 13
ZERO, HALF = f32(0.0), f32(0.5)
cmax, cmin, d2i, f2i = view_model.cmax, view_model.cmin, view_model.d2i, view_model.f2i

_libm = view_model._libm
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(a, b):
    return f32(_libm.powf(float(a), float(b)))


def new_tally():
    return collections.defaultdict(int)


class Args:
    def __init__(self, behind_sphere_mult=1.0, zoom_f=1.0, smap_pixel_width=0.0, window_width=1920, shadow_pass=0, reflection_pass=0, uw_skip=1, skip_small_shadow_objs=0,
                 draw_opaque=1, draw_leaves=1):
        self.behind_sphere_mult, self.zoom_f, self.smap_pixel_width = f32(behind_sphere_mult), f32(zoom_f), f32(smap_pixel_width)
        self.window_width, self.shadow_pass, self.reflection_pass = int(window_width), int(bool(shadow_pass)), int(reflection_pass)
        self.uw_skip, self.skip_small_shadow_objs = int(bool(uw_skip)), int(bool(skip_small_shadow_objs))
        self.draw_opaque, self.draw_leaves = int(bool(draw_opaque)), int(bool(draw_leaves))


class Globals:
    """what the objects read beside the scene and the view: the args, tree_scale, get_min_water_plane_z()"""

    def __init__(self, a, tree_scale=1.0, ocean_wave_height=0.0):
        self.a, self.tree_scale, self.ocean_wave_height = a, f32(tree_scale), f32(ocean_wave_height)


class Ctx:
    """the state of one tile's draw: the globals as the draw methods read them, and where their results go"""

    def __init__(self, sc, v, g, xlate, scale_val, nrec, tally):
        a = g.a
        self.v, self.a, self.tally = v, a, tally
        self.xlate = xlate
        self.scale_val = scale_val
        self.water_plane_z = sc.water_plane_z
        self.min_water_plane_z = f32(sc.water_plane_z - g.ocean_wave_height)  # get_water_z_height() - ocean_wave_height
        self.shadow_only, self.reflection_pass = bool(a.shadow_pass), bool(a.reflection_pass)
        self.pt_line_thresh = f32(f64(PT_LINE_THRESH) * f64(a.zoom_f))  # get_pt_line_thresh()
        self.sscale = f32(d2i(f64(a.zoom_f) * f64(a.window_width)))      # int sscale(int((do_zoom ? ZOOM_FACTOR : 1.0)*window_width)), passed as float
        self.word, self.size_scale, self.dist = [0] * nrec, [ZERO] * nrec, [ZERO] * nrec
        self.lists = [[] for _ in range(GROUPS)]

    def camera(self):
        return self.v.pos


def add_xlate(cx, p):
    return [f32(p[0] + cx.xlate[0]), f32(p[1] + cx.xlate[1]), f32(p[2] + cx.xlate[2])]


def add_z(p, dz):  # p + point(0.0, 0.0, dz)
    return [f32(p[0] + ZERO), f32(p[1] + ZERO), f32(p[2] + f32(dz))]


def distance_to_camera(cx, p):
    return f32(np.sqrt(view_model.p2p_dist_sq(cx.camera(), p)))


def check_visible(cx, radius, bradius, p):
    """scenery_obj::check_visible in tiled-terrain mode"""
    bradius = f32(bradius)
    return view_model.sphere_visible_test(cx.v, cx.a.behind_sphere_mult, p, radius if bradius == 0.0 else bradius, cx.tally)


def skip_uw_draw(cx, pos, radius):
    if not cx.a.uw_skip:
        cx.tally["uw_gate_off"] += 1
        return False
    r = bool(cx.camera()[2] > cx.water_plane_z and f32(pos[2] + radius) < cx.min_water_plane_z)
    cx.tally["uw_skipped" if r else ("uw_camera_below" if not cx.camera()[2] > cx.water_plane_z else "uw_top_above")] += 1
    return r


def is_visible(cx, o, bradius):
    p = add_xlate(cx, o.pos)
    if not check_visible(cx, o.radius, bradius, p):
        cx.tally[o.name + "_culled"] += 1
        return False
    return cx.shadow_only or not skip_uw_draw(cx, p, o.radius)


def get_size_scale(cx, o, dist_to_camera):
    if cx.scale_val == 0.0:
        return f32(1.0)
    s = cmin(f32(1.0), powf(f32(cx.scale_val / dist_to_camera), f32(8.0)))
    cx.tally["size_scale_1" if s == 1.0 else "size_scale_below_1"] += 1
    return s


def get_def_smap_ndiv(cx, radius):
    radius = f32(radius)
    n = min(N_SPHERE_DIV, max(4, d2i(f64(0.5) * f64(radius) / f64(cx.a.smap_pixel_width))))
    cx.tally["smap_ndiv"] += 1
    return n


def tally_ndiv(cx, o, n, lo, hi):
    cx.tally[o.name + ("_ndiv_lo" if n == lo else ("_ndiv_hi" if n == hi else "_ndiv_mid"))] += 1
    return n


def tally_thresh(cx, o, lhs, dist):
    cx.tally[o.name + ("_at_thresh" if lhs == dist else ("_small" if lhs < dist else "_large"))] += 1


class Obj:
    """a record as its class keeps it"""

    def __init__(self, index, rec, ov):
        self.i, self.kind = index, int(rec["kind"])
        self.name = KIND_NAMES[self.kind]
        self.pos = [f32(x) for x in rec["pos"]]
        self.radius = f32(ov) if ov is not None and f32(ov) > 0.0 else f32(rec["radius"])
        self.overridden = bool(ov is not None and f32(ov) > 0.0)
        self.iv, self.p = [int(x) for x in rec["iv"]], [f32(x) for x in rec["p"]]


def below_water(cx, z):
    r = bool(cx.reflection_pass and z < cx.water_plane_z)
    if r:
        cx.tally["reflection_below_water"] += 1
    return r


def draw_rock_shape(cx, o):
    if not o.overridden:  # gen_rock runs in the engine: not decided here
        cx.word[o.i] = ENGINE
        cx.tally["rock_shape_engine"] += 1
        return
    o.pos[2] = f32(f64(o.pos[2]) + f64(0.1) * f64(o.radius))  # pos.z += 0.1*radius (:156)
    if not is_visible(cx, o, 0.0):
        return
    if below_water(cx, o.pos[2]):
        return
    cx.word[o.i] = POLY
    cx.lists[G_ROCK_SHAPE].append(o.i)
    cx.tally["rock_shape_poly"] += 1


def draw_surface_rock(cx, o):
    if not is_visible(cx, o, 0.0):
        return
    if below_water(cx, o.pos[2]):
        return
    p = add_xlate(cx, o.pos)
    dist = distance_to_camera(cx, p)
    cx.dist[o.i] = dist
    lhs = f32(f32(f32(2) * cx.pt_line_thresh) * o.radius)
    if not cx.shadow_only:
        tally_thresh(cx, o, lhs, dist)
    if not cx.shadow_only and lhs < dist:  # draw as point
        cx.word[o.i] = POINT
        cx.lists[G_PLD_POINTS].append(o.i)
        return
    cx.size_scale[o.i] = get_size_scale(cx, o, dist)
    cx.word[o.i] = POLY
    cx.lists[G_SURFACE_ROCK].append(o.i)


def draw_rock(cx, o):
    if not is_visible(cx, o, f32(f64(1.3) * f64(o.radius))):
        return
    if below_water(cx, o.pos[2]):
        return
    p = add_xlate(cx, o.pos)
    dist = distance_to_camera(cx, p)
    cx.dist[o.i] = dist
    lhs = f32(f32(f32(2) * cx.pt_line_thresh) * o.radius)
    if not cx.shadow_only:
        tally_thresh(cx, o, lhs, dist)
    if not cx.shadow_only and lhs < dist:  # draw as point
        cx.word[o.i] = POINT
        cx.lists[G_PLD_POINTS].append(o.i)
        return
    ndiv = max(4, min(N_SPHERE_DIV, get_def_smap_ndiv(cx, o.radius) if cx.shadow_only else f2i(f32(f32(cx.sscale * o.radius) / dist))))
    tally_ndiv(cx, o, ndiv, 4, N_SPHERE_DIV)
    cx.size_scale[o.i] = get_size_scale(cx, o, dist)
    cx.word[o.i] = POLY | (ndiv << NDIV_SHIFT)
    cx.lists[G_ROCK].append(o.i)


def draw_voxel_rock(cx, o):
    if not is_visible(cx, o, o.radius):
        return
    if below_water(cx, o.pos[2]):
        return
    dist = distance_to_camera(cx, add_xlate(cx, o.pos))
    cx.dist[o.i] = dist
    cx.size_scale[o.i] = get_size_scale(cx, o, dist)
    cx.word[o.i] = POLY
    cx.lists[G_VOXEL_ROCK].append(o.i)
    cx.tally["voxel_rock_poly"] += 1


def draw_log(cx, o):
    typ, radius2, length, dirv, pt2 = o.iv[0], o.p[0], o.p[1], o.p[2:5], o.p[5:8]
    if typ < 0:
        return
    s = [f32(o.pos[k] + pt2[k]) for k in range(3)]
    center = add_xlate(cx, [f32(s[k] * HALF) for k in range(3)])  # (pos + pt2)*0.5 + xlate
    if not check_visible(cx, o.radius, cmax(length, cmax(o.radius, radius2)), center):
        cx.tally["log_culled"] += 1
        return
    if cx.reflection_pass and f32(HALF * f32(o.pos[2] + pt2[2])) < cx.water_plane_z:
        cx.tally["reflection_below_water"] += 1
        return
    dist = distance_to_camera(cx, center)
    cx.dist[o.i] = dist
    lhs = f32(cx.pt_line_thresh * f32(o.radius + radius2))
    if not cx.shadow_only:
        tally_thresh(cx, o, lhs, dist)
    if not cx.shadow_only and lhs < dist:  # draw as line
        cx.word[o.i] = LINE
        cx.lists[G_PLD_LINES].append(o.i)
        return
    ndiv = max(3, min(N_CYL_SIDES, get_def_smap_ndiv(cx, f32(f64(2.0) * f64(o.radius))) if cx.shadow_only else d2i(f64(2.0) * f64(cx.sscale) * f64(o.radius) / f64(dist))))
    tally_ndiv(cx, o, ndiv, 3, N_CYL_SIDES)
    w = POLY | (ndiv << NDIV_SHIFT)
    cx.lists[G_LOG].append(o.i)
    if not cx.shadow_only and f64(dist) > f64(0.75) * f64(cx.pt_line_thresh) * f64(o.radius):  # skip end drawing
        cx.tally["log_no_end"] += 1
    else:  # the end visible to the camera
        cam = cx.camera()
        dp = f32(f32(f32(dirv[0] * f32(cam[0] - center[0])) + f32(dirv[1] * f32(cam[1] - center[1]))) + f32(dirv[2] * f32(cam[2] - center[2])))  # dot_product_ptv
        if f64(dp) > 0.0:
            w |= LOG_END
            cx.tally["log_end_pos"] += 1
        else:
            w |= LOG_END | LOG_END2
            cx.tally["log_end_pt2"] += 1
    cx.word[o.i] = w


def draw_stump(cx, o):
    typ, radius2, height = o.iv[0], o.p[0], o.p[1]
    if typ < 0:
        return
    pos_cs = add_xlate(cx, o.pos)
    center = add_z(pos_cs, f64(0.5) * f64(height))
    if not check_visible(cx, o.radius, cmax(height, cmax(o.radius, radius2)), center):
        cx.tally["stump_culled"] += 1
        return
    if below_water(cx, o.pos[2]):
        return
    dist = distance_to_camera(cx, center)
    cx.dist[o.i] = dist
    lhs = f32(cx.pt_line_thresh * f32(o.radius + radius2))
    if not cx.shadow_only:
        tally_thresh(cx, o, lhs, dist)
    if not cx.shadow_only and lhs < dist:  # draw as line
        cx.word[o.i] = LINE
        cx.lists[G_PLD_LINES].append(o.i)
        return
    ndiv = max(3, min(N_CYL_SIDES, get_def_smap_ndiv(cx, f32(f64(2.2) * f64(o.radius))) if cx.shadow_only else d2i(f64(2.2) * f64(cx.sscale) * f64(o.radius) / f64(dist))))
    tally_ndiv(cx, o, ndiv, 3, N_CYL_SIDES)
    w = POLY | (ndiv << NDIV_SHIFT)
    delta = view_model.sub(cx.camera(), pos_cs)  # camera_delta
    above, steep = bool(delta[2] > height), bool(f64(delta[2]) > f64(0.1) * f64(f32(abs(delta[0]) + abs(delta[1]))))
    if above and steep:
        w |= STUMP_TOP
    cx.tally["stump_top" if above and steep else ("stump_top_shallow" if above else ("stump_top_below" if steep else "stump_top_neither"))] += 1
    cx.word[o.i] = w
    cx.lists[G_STUMP].append(o.i)


def draw_mushroom(cx, o):
    if below_water(cx, o.pos[2]):
        return
    height = o.p[0]
    cap_zscale = f32(0.5)
    cap_center = add_z(o.pos, f32(height - f32(cap_zscale * o.radius)))
    center_cs = add_xlate(cx, cap_center)
    dist = distance_to_camera(cx, center_cs)
    cx.dist[o.i] = dist
    if f64(dist) > f64(1000.0) * f64(o.radius):  # too far away
        cx.tally["mushroom_too_far"] += 1
        return
    if not check_visible(cx, o.radius, cmax(height, o.radius), center_cs):
        cx.tally["mushroom_culled"] += 1
        return
    ndiv = max(3, min(N_CYL_SIDES, d2i(f64(1.0) * f64(cx.sscale) * f64(o.radius) / f64(dist))))
    tally_ndiv(cx, o, ndiv, 3, N_CYL_SIDES)
    w = POLY | (ndiv << NDIV_SHIFT)
    if cx.camera()[2] < cap_center[2]:  # white underside of cap
        w |= CAP_UNDERSIDE
        cx.tally["mushroom_underside"] += 1
    cx.word[o.i] = w
    cx.lists[G_MUSHROOM].append(o.i)


def plant_underwater_skip(cx, o):
    """the first statement of s_plant::draw_stem and the second of draw_leaves (:855, :901)"""
    if not o.iv[0] >= NUM_LAND_PLANT_TYPES:  # is_water_plant()
        return False
    if cx.reflection_pass:
        cx.tally["water_plant_reflection"] += 1
        return True
    if not cx.shadow_only and o.pos[2] < cx.water_plane_z and cx.camera()[2] > cx.water_plane_z:
        cx.tally["water_plant_underwater"] += 1
        return True
    cx.tally["water_plant_drawn"] += 1
    return False


def draw_stem(cx, o):
    height = o.p[0]
    if plant_underwater_skip(cx, o):
        return
    pos_cs = add_xlate(cx, o.pos)
    pos2 = add_z(pos_cs, f64(0.5) * f64(height))
    if not check_visible(cx, o.radius, f32(height + o.radius), pos2):
        cx.tally["plant_culled"] += 1
        return
    dist = distance_to_camera(cx, pos2)
    cx.dist[o.i] = dist
    lhs = f32(f32(f32(2) * cx.pt_line_thresh) * o.radius)
    if not cx.shadow_only:
        tally_thresh(cx, o, lhs, dist)
    if not cx.shadow_only and lhs < dist:  # draw as line
        cx.word[o.i] |= LINE
        cx.lists[G_PLD_LINES].append(o.i)
    else:
        ndiv = max(3, min(N_CYL_SIDES, get_def_smap_ndiv(cx, f32(f64(2.0) * f64(o.radius))) if cx.shadow_only else d2i(f64(2.0) * f64(cx.sscale) * f64(o.radius) / f64(dist))))
        tally_ndiv(cx, o, ndiv, 3, N_CYL_SIDES)
        cx.word[o.i] |= POLY | (ndiv << NDIV_SHIFT)
        cx.lists[G_STEM].append(o.i)


def draw_berries(cx, o):
    """up to berries.empty() and burn_amt, which the engine knows"""
    height = o.p[0]
    pos2 = add_z(add_xlate(cx, o.pos), f64(0.5) * f64(height))
    if not view_model.sphere_visible_test(cx.v, cx.a.behind_sphere_mult, pos2, f32(HALF * f32(height + o.radius)), cx.tally):  # sphere_in_camera_view(.., 2)
        return
    dist = distance_to_camera(cx, pos2)
    cx.dist[o.i] = dist
    size_scale = f32(f32(cx.pt_line_thresh * o.radius) / dist)
    if f64(size_scale) < 1.2:  # too small/far away
        cx.tally["berries_too_small"] += 1
        return
    ndiv = max(4, min(16, d2i(f64(2.0) * f64(size_scale))))
    cx.tally["berries_ndiv_lo" if ndiv == 4 else ("berries_ndiv_hi" if ndiv == 16 else "berries_ndiv_mid")] += 1
    cx.word[o.i] |= BERRIES | (ndiv << BERRY_NDIV_SHIFT)
    cx.lists[G_BERRIES].append(o.i)


def draw_plant_leaves(cx, o):
    height = o.p[0]
    if plant_underwater_skip(cx, o):
        return
    pos2 = add_z(add_xlate(cx, o.pos), f64(0.5) * f64(height))
    if not check_visible(cx, o.radius, f32(HALF * f32(height + o.radius)), pos2):
        return
    cx.word[o.i] |= LEAVES
    cx.lists[G_PLANT_LEAVES].append(o.i)
    cx.tally["plant_leaves"] += 1


def draw_leafy_leaves(cx, o):
    if not is_visible(cx, o, o.radius):
        return
    if below_water(cx, o.pos[2]):
        return
    w = LEAVES
    if o.pos[2] < cx.water_plane_z:  # is_underwater
        w |= UNDERWATER
        cx.tally["leafy_underwater"] += 1
    cx.word[o.i] |= w
    cx.lists[G_LEAFY_LEAVES].append(o.i)
    cx.tally["leafy_leaves"] += 1


def draw_opaque_objects(cx, by_kind):
    for o in by_kind[ROCK_SHAPE]:
        draw_rock_shape(cx, o)
    for o in by_kind[SURFACE_ROCK]:
        draw_surface_rock(cx, o)
    for o in by_kind[ROCK]:
        draw_rock(cx, o)
    if not cx.shadow_only or not cx.a.skip_small_shadow_objs:  # can_skip_small_shadow_objs()
        for o in by_kind[LOG]:
            draw_log(cx, o)
        for o in by_kind[STUMP]:
            draw_stump(cx, o)
    elif by_kind[LOG] or by_kind[STUMP]:
        cx.tally["wood_skipped_in_shadow"] += 1
    if not cx.shadow_only:  # mushrooms are too small to cast shadows
        for o in by_kind[MUSHROOM]:
            draw_mushroom(cx, o)
    for o in by_kind[PLANT]:
        draw_stem(cx, o)
    if not cx.shadow_only:  # no berry shadows
        for o in by_kind[PLANT]:
            draw_berries(cx, o)
    for o in by_kind[VOXEL_ROCK]:
        draw_voxel_rock(cx, o)


def draw_plant_leaves_sweep(cx, by_kind):
    for o in by_kind[PLANT]:
        draw_plant_leaves(cx, o)
    for o in by_kind[LEAFY_PLANT]:
        draw_leafy_leaves(cx, o)


class TileResult:
    def __init__(self):
        self.written, self.dist_scale, self.scale_val, self.flags, self.num_records = False, ZERO, ZERO, 0, 0
        self.word, self.size_scale, self.dist, self.list, self.group_counts = [], [], [], [], [0] * GROUPS


def draw_tile(sc, v, g, txy, st, recs, ovs, xlate, tally):
    """tile_t::draw_scenery for one tile whose scenery is generated and that is in to_draw"""
    a = g.a
    res = TileResult()
    tally["tiles"] += 1
    if len(recs) == 0:
        tally["empty"] += 1
        return res
    t = tm.Tile(sc, txy, st, 0.0, 0.0, None, 0, 0)
    thresh = SCENERY_THRESH_REF if a.reflection_pass else SCENERY_THRESH
    in_tiles = f32(tm.get_rel_dist_to_camera(sc, v, t, False) * f32(tm.TILE_RADIUS))  # get_dist_to_camera_in_tiles(0)
    dist_scale = f32(f32(g.tree_scale * in_tiles) / thresh)
    if f64(dist_scale) > 1.0:
        tally["dropped"] += 1
        tally.setdefault("dropped_dist_scales", []).append(float(dist_scale))
        return res
    tally["drawn"] += 1
    res.written, res.dist_scale = True, dist_scale
    res.scale_val = f32(thresh * sc.g.tile_width)  # get_scenery_thresh(reflection_pass)*get_tile_width()
    res.flags = TILE_DRAWN | (TILE_OPAQUE if a.draw_opaque else 0) | (TILE_LEAVES if a.draw_leaves else 0)
    res.num_records = len(recs)
    cx = Ctx(sc, v, g, xlate, res.scale_val, len(recs), tally)
    by_kind = [[] for _ in range(9)]
    for j, r in enumerate(recs):
        k = int(r["kind"])
        if 0 <= k < 9:
            by_kind[k].append(Obj(j, r, None if ovs is None else ovs[j]))
        else:
            tally["bad_kind"] += 1
    if a.draw_opaque:
        draw_opaque_objects(cx, by_kind)
    if a.draw_leaves:
        draw_plant_leaves_sweep(cx, by_kind)
    res.word, res.size_scale, res.dist = cx.word, cx.size_scale, cx.dist
    res.group_counts = [len(x) for x in cx.lists]
    res.list = [i for x in cx.lists for i in x]
    # the pld lists hold the kinds in the order of the reference's loops
    kinds = [int(recs[i]["kind"]) for i in cx.lists[G_PLD_LINES]]
    assert kinds == sorted(kinds, key=(LOG, STUMP, PLANT).index)
    tally["max_records"] = max(tally["max_records"], len(recs))
    tally["max_entries"] = max(tally["max_entries"], len(res.list))
    return res


def draw(sc, v, g, tiles, stats, objs, counts, skip=None, radius_override=None, xoff2=0, yoff2=0, tally=None):
    """terra_tiles_scenery_view for a batch -> [TileResult]; xlate = scenery_off.get_xlate() = ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0)"""
    tally = new_tally() if tally is None else tally
    cap = objs.shape[1]
    xlate = [f32(f32(sc.dxoff + xoff2) * sc.DX_VAL), f32(f32(sc.dyoff + yoff2) * sc.DY_VAL), ZERO]
    out = []
    with np.errstate(all="ignore"):
        for t, txy in enumerate(tiles):
            if skip is not None and skip[t]:
                tally["skipped"] += 1
                out.append(TileResult())
                continue
            m = min(int(counts[t]), cap)
            out.append(draw_tile(sc, v, g, txy, stats[t], objs[t, :m], None if radius_override is None else radius_override[t, :m], xlate, tally))
    return out
