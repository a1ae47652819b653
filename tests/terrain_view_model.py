"""NumPy / Python float32 restatement of the terrain draw list of a tile batch for a camera, written from the reference statements (not from the library's bodies):

    tile_draw_t::draw up to its sort                                         src/tiled_mesh.cpp:2844-2915
    occluder_cubes_t's constructor, calc_cube_top_points                     src/tiled_mesh.cpp:2823-2842
    tile_t::get_lod_level                                                    src/tiled_mesh.cpp:1910-1932
    the crack look-ups of tile_t::draw, crack_ibuf_t::get_index              src/tiled_mesh.cpp:2059-2074, 2020-2023
    use_as_occluder, get_bsphere_radius_inc_water                            src/tiled_mesh.cpp:3801-3803, 366-368
    get_center, get_bcube, get_mesh_bcube, get_mesh_sub_bcube, get_sub_bcube src/tiled_mesh.h:229-252
    get_rel_dist_to_camera, rel_dist_to_camera_xy_lt, is_visible,
      get_dist_to_camera_in_tiles                                            src/tiled_mesh.h:320-332
    DRAW_DIST_TILES, OCCLUDER_DIST, TILE_RADIUS, NUM_LODS, BCUBE_ZTOLER      src/tiled_mesh.cpp:23, 33; src/tiled_mesh.h:24-25, 32
    pos_dir_up::sphere_and_cube_visible_test                                 src/visibility.cpp:215-219
    get_line_clip / check_line_clip, get_region                              src/Math3d.cpp:1029-1052; src/inlines.h:509-512, 522-528
    cube_t::get_cube_center, is_all_zeros                                    src/3DWorld.h:491, 602-604
    p2p_dist_xy, dist_xy_less_than                                           src/inlines.h:183-195

behind_sphere_mult, sphere_visible_test, cube_visible and the vector helpers are tests/view_model.py's.  Types: np.float32 for float, Python float for double, Python int
for int / unsigned.  Which sub-expressions are double: in get_lod_level the comparisons of min_normal_z with 0.9, 0.95 and
0.25, `dist *= 4.0 / 2.0`, `dist /= -log2(2.0*min_normal_z)` (each narrowed back into the float dist) and the loop's comparison with 1.8 / 2.0; log2 is the C
library's, called through ctypes.  Equal distances order by batch index (the reference's pointer order is not reproducible).

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import ctypes

import numpy as np

import grass_view_model as gm

import view_model

f32 = np.float32
NUM_LODS, TILE_RADIUS = 5, 6
DRAW_DIST_TILES, OCCLUDER_DIST = f32(1.5), f32(0.2)
BCUBE_ZTOLER = f32(1.0E-6)
ZERO, HALF, TWO = f32(0.0), f32(0.5), f32(2.0)
ABSENT, TOO_FAR, NOT_VISIBLE, OCCLUDED_BEFORE, OCCLUDED, DRAWN = range(6)
WAS_OCCLUDER = 0x80
FLAG_ABSENT, FLAG_NO_OCCLUDER, FLAG_SHADOW_MAPS = 1, 2, 4
NO_CRACK = 255
cmax, cmin, sub, sphere_visible_test = view_model.cmax, view_model.cmin, view_model.sub, view_model.sphere_visible_test

_libm = view_model._libm
_libm.log2.restype = ctypes.c_double
_libm.log2.argtypes = [ctypes.c_double]

TALLY = ("absent", "too_far", "not_visible", "occluded_before", "occluded", "drawn", "occluders", "columns_zeroed", "columns_kept", "tested", "test_skipped_state",
         "one_sub_unoccluded", "centre_rejected", "sphere_rejected", "sphere_all", "cube_accepted", "cube_rejected", "behind_true", "behind_false", "water_radius",
         "water_z2", "lod_flat", "lod_mnz0", "lod_steep", "lod_mid", "lod_flat2", "lod_flat4", "lod_water_blocked", "lod_smap", "ties", "no_neighbour", "adj_lower",
         "adj_equal", "adj_higher", "max_lod_not_flat")


def new_tally():
    return {k: 0 for k in TALLY}


class Args:
    def __init__(self, behind_sphere_mult=1.0, occluder_zmin=0.0, water_enabled=1, check_occlusion=1, reflection_pass=0):
        self.behind_sphere_mult, self.occluder_zmin = f32(behind_sphere_mult), f32(occluder_zmin)
        self.water_enabled, self.check_occlusion, self.reflection_pass = int(water_enabled), int(check_occlusion), int(reflection_pass)


class Scene:
    """the globals the pass reads: the oracle's state after orc.init(cfg), the config, the offsets"""

    def __init__(self, orc, cfg, dxoff=0, dyoff=0):
        self.g = gm.Scene(orc, cfg, gm.Params(), dxoff, dyoff)
        self.S, self.DX_VAL, self.DY_VAL, self.dxoff, self.dyoff = self.g.S, self.g.DX_VAL, self.g.DY_VAL, dxoff, dyoff
        self.scaled_tile_radius = self.g.scaled_tile_radius  # TILE_RADIUS*get_tile_width()
        self.water_plane_z = f32(orc.state().water_plane_z)


class Tile:
    def __init__(self, sc, txy, st, min_normal_z, trmax, tile_zmax, flags, state):
        self.tx, self.ty = int(txy[0]), int(txy[1])
        self.sub_zmin, self.sub_zmax = [f32(v) for v in st.sub_zmin], [f32(v) for v in st.sub_zmax]  # [y][x]
        self.mzmin, self.mzmax, self.radius = f32(st.mzmin), f32(st.mzmax), f32(st.radius)
        self.min_normal_z, self.trmax, self.flags, self.state = f32(min_normal_z), f32(trmax), int(flags), int(state)
        self.tile_zmax = self.mzmax if tile_zmax is None else f32(tile_zmax)
        S = sc.S
        self.x1, self.y1, self.x2, self.y2 = self.tx * S, self.ty * S, self.tx * S + S, self.ty * S + S


def get_center(sc, t):
    return [sc.g.get_xval(((t.x1 + t.x2) >> 1) + sc.dxoff), sc.g.get_yval(((t.y1 + t.y2) >> 1) + sc.dyoff), f32(HALF * f32(t.mzmin + t.mzmax))]


def corner(sc, t):
    xv1, yv1 = sc.g.get_xval(t.x1 + sc.dxoff), sc.g.get_yval(t.y1 + sc.dyoff)
    return xv1, yv1, f32(xv1 + f32(f32(t.x2 - t.x1) * sc.DX_VAL)), f32(yv1 + f32(f32(t.y2 - t.y1) * sc.DY_VAL))


def get_bcube(sc, t, tally=None):
    xv1, yv1, xv2, yv2 = corner(sc, t)
    top = f32(t.tile_zmax + BCUBE_ZTOLER)
    z2 = cmax(top, sc.water_plane_z)
    if tally is not None and top < sc.water_plane_z:
        tally["water_z2"] += 1
    return [[f32(xv1 - t.trmax), f32(xv2 + t.trmax)], [f32(yv1 - t.trmax), f32(yv2 + t.trmax)], [f32(t.mzmin - BCUBE_ZTOLER), z2]]


def get_mesh_bcube(sc, t):
    xv1, yv1, xv2, yv2 = corner(sc, t)
    return [[xv1, xv2], [yv1, yv2], [f32(t.mzmin - BCUBE_ZTOLER), f32(t.mzmax + BCUBE_ZTOLER)]]


def get_mesh_sub_bcube(sc, t, x, y):
    xv1, yv1, xv2, yv2 = corner(sc, t)
    dx, dy = f32(f32(xv2 - xv1) / f32(4)), f32(f32(yv2 - yv1) / f32(4))
    return [[f32(xv1 + f32(f32(x) * dx)), f32(xv1 + f32(f32(x + 1) * dx))], [f32(yv1 + f32(f32(y) * dy)), f32(yv1 + f32(f32(y + 1) * dy))],
            [t.sub_zmin[4 * y + x], t.sub_zmax[4 * y + x]]]


def get_sub_bcube(sc, t, x, y):
    b = get_mesh_sub_bcube(sc, t, x, y)
    b[2][1] = f32(b[2][1] + f32(t.tile_zmax - t.mzmax))
    return b


def p2p_dist_xy_sq(a, b):
    return f32(f32(f32(a[0] - b[0]) * f32(a[0] - b[0])) + f32(f32(a[1] - b[1]) * f32(a[1] - b[1])))


def get_rel_dist_to_camera(sc, v, t, xy_dist=True):
    c = get_center(sc, t)
    d = f32(np.sqrt(p2p_dist_xy_sq(v.pos, c))) if xy_dist else f32(np.sqrt(view_model.p2p_dist_sq(v.pos, c)))
    return f32(cmax(ZERO, f32(d - t.radius)) / sc.scaled_tile_radius)


def rel_dist_to_camera_xy_lt(sc, v, t, rel_dist):
    dval = f32(f32(rel_dist * sc.scaled_tile_radius) + t.radius)
    return bool(p2p_dist_xy_sq(v.pos, get_center(sc, t)) < f32(dval * dval))


def get_bsphere_radius_inc_water(sc, a, t, tally=None):
    if a.water_enabled and t.mzmax < sc.water_plane_z:
        if tally is not None:
            tally["water_radius"] += 1
        return cmax(t.radius, f32(sc.water_plane_z - f32(HALF * f32(t.mzmin + t.mzmax))))
    return t.radius


def is_visible(sc, v, a, t, tally=None):
    pos, radius, cube = get_center(sc, t), get_bsphere_radius_inc_water(sc, a, t, tally), get_bcube(sc, t, tally)
    if not sphere_visible_test(v, a.behind_sphere_mult, pos, radius, tally):
        if tally is not None:
            tally["sphere_rejected"] += 1
        return False
    if sphere_visible_test(v, a.behind_sphere_mult, pos, f32(-radius)):
        if tally is not None:
            tally["sphere_all"] += 1
        return True
    r = view_model.cube_visible(v, cube)
    if tally is not None:
        tally["cube_accepted" if r else "cube_rejected"] += 1
    return r


def get_region(p, d):
    region = 0
    if p[0] < d[0][0]:
        region |= 0x01
    elif p[0] >= d[0][1]:
        region |= 0x02
    if p[1] < d[1][0]:
        region |= 0x04
    elif p[1] >= d[1][1]:
        region |= 0x08
    if p[2] < d[2][0]:
        region |= 0x10
    elif p[2] >= d[2][1]:
        region |= 0x20
    return region


def check_line_clip(v1, v2, d):
    """get_line_clip's return value"""
    region1, region2 = get_region(v1, d), get_region(v2, d)
    if region1 & region2:
        return False
    region3 = region1 | region2
    tmax, tmin = f32(1.0), f32(0.0)
    if region3 == 0:
        return True
    dv = sub(v2, v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        for reg, va, vb, vd, vc in ((0x01, d[0][0], v1[0], dv[0], dv[0]), (0x02, d[0][1], v1[0], dv[0], f32(-dv[0])), (0x04, d[1][0], v1[1], dv[1], dv[1]),
                                    (0x08, d[1][1], v1[1], dv[1], f32(-dv[1])), (0x10, d[2][0], v1[2], dv[2], dv[2]), (0x20, d[2][1], v1[2], dv[2], f32(-dv[2]))):
            if region3 & reg:
                t = f32(f32(va - vb) / vd)
                if vc > 0.0:
                    if t > tmin:
                        tmin = t
                elif t < tmax:
                    tmax = t
                if tmin >= tmax:
                    return False
    return True


def cube_top_points(d):
    return [[d[0][i0], d[1][i1], d[2][1]] for i0 in (0, 1) for i1 in (0, 1)]


def get_cube_center(d):
    return [f32(HALF * f32(d[i][0] + d[i][1])) for i in range(3)]


def is_all_zeros(d):
    return all(d[i][j] == 0 for i in range(3) for j in range(2))


class Occluder:
    """occluder_cubes_t"""

    def __init__(self, sc, v, a, t, index, tally):
        self.index, self.bcube, self.sub_cubes = index, get_mesh_bcube(sc, t), []
        for s in range(16):
            c = get_mesh_sub_bcube(sc, t, s >> 2, s & 3)
            if not view_model.cube_visible(v, c):
                c = [[ZERO, ZERO], [ZERO, ZERO], [ZERO, ZERO]]
                tally["columns_zeroed"] += 1
            else:
                c[2][1] = c[2][0]
                c[2][0] = a.occluder_zmin
                tally["columns_kept"] += 1
            self.sub_cubes.append(c)


def lod_steep_dist(dist, mnz):
    """get_lod_level's statement for a steep tile: dist /= -log2(2.0*min_normal_z) (:1924), the quotient in double, narrowed into the float"""
    return f32(float(f32(dist)) / -_libm.log2(2.0 * float(f32(mnz))))


def get_lod_level(sc, v, a, t, tally=None):
    def count(k):
        if tally is not None:
            tally[k] += 1
    if t.mzmax == t.mzmin:
        count("lod_flat")
        return NUM_LODS - 1
    assert a.reflection_pass != 1
    lod_level = 0
    dist = f32(get_rel_dist_to_camera(sc, v, t, False) * f32(TILE_RADIUS))  # get_dist_to_camera_in_tiles(0)
    if t.flags & FLAG_SHADOW_MAPS:
        dist = f32(dist / f32(2))
        count("lod_smap")
    mnz = t.min_normal_z
    if mnz > 0.0:
        if float(mnz) > 0.9:
            if not a.water_enabled or t.mzmax < sc.water_plane_z or t.mzmin > sc.water_plane_z:
                dist = f32(float(dist) * (4.0 if float(mnz) > 0.95 else 2.0))
                count("lod_flat4" if float(mnz) > 0.95 else "lod_flat2")
            else:
                count("lod_water_blocked")
        elif float(mnz) < 0.25:
            dist = lod_steep_dist(dist, mnz)
            count("lod_steep")
        else:
            count("lod_mid")
    else:
        count("lod_mnz0")
    while float(dist) > (1.8 if a.reflection_pass else 2.0) and lod_level + 1 < NUM_LODS and (sc.S >> (lod_level + 1)) >= 4:
        dist = f32(dist / f32(2))
        lod_level += 1
    return lod_level


def crack_index(dim, dir, cur_lod, adj_lod):
    return NUM_LODS * (NUM_LODS * (2 * dim + dir) + cur_lod) + adj_lod


def draw(sc, v, a, tile_xy, stats, min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None, tally=None):
    """-> (status [n] uint8, dist [n] float32, lod [n] uint8, crack [n, 4] uint8, draw_order list, occluded list, occl_state [n] uint8 after the call)"""
    tally = new_tally() if tally is None else tally
    n = len(tile_xy)
    opt = lambda arr, i, d: d if arr is None else arr[i]  # noqa: E731
    tiles = [Tile(sc, tile_xy[i], stats[i], opt(min_normal_z, i, 0.0), opt(trmax, i, 0.0), opt(tile_zmax, i, None), opt(flags, i, 0), opt(occl_state, i, 0)) for i in range(n)]
    status, dist, lod, crack = np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, np.uint8), np.full((n, 4), NO_CRACK, np.uint8)
    state = np.array([t.state for t in tiles], np.uint8)
    present = [i for i in range(n) if not tiles[i].flags & FLAG_ABSENT]
    tally["absent"] += n - len(present)
    camera = v.pos
    visible = {i: is_visible(sc, v, a, tiles[i], tally) for i in present}
    occluders = []
    if a.check_occlusion:
        for i in present:
            t = tiles[i]
            if not t.flags & FLAG_NO_OCCLUDER and rel_dist_to_camera_xy_lt(sc, v, t, OCCLUDER_DIST) and visible[i]:  # use_as_occluder()
                occluders.append(Occluder(sc, v, a, t, i, tally))
                status[i] |= WAS_OCCLUDER
    tally["occluders"] += len(occluders)
    to_draw, occluded_tiles = [], []
    for i in present:
        t = tiles[i]
        dist[i] = get_rel_dist_to_camera(sc, v, t)
        lod[i] = get_lod_level(sc, v, a, t, tally)
        if t.mzmax != t.mzmin:
            tally["max_lod_not_flat"] = max(tally["max_lod_not_flat"], int(lod[i]))
        if dist[i] > DRAW_DIST_TILES:
            status[i] |= TOO_FAR
            continue
        if not visible[i]:
            status[i] |= NOT_VISIBLE
            continue
        if t.state == 1:  # was_last_occluded()
            status[i] |= OCCLUDED_BEFORE
            continue
        if occluders and t.state == 2:
            tally["test_skipped_state"] += 1
        if occluders and t.state != 2:  # !was_last_unoccluded()
            tally["tested"] += 1
            bcube = get_bcube(sc, t)
            tile_pts = cube_top_points(bcube)
            occluder_ixs = []
            for j, oc in enumerate(occluders):
                if oc.index == i:
                    continue  # no self-occlusion
                if any(check_line_clip(p, camera, oc.bcube) for p in tile_pts):
                    occluder_ixs.append(j)
            unoccluded = 0
            for q in range(16):  # (the reference breaks at the first unoccluded sub-tile; all are evaluated here for the tally)
                sub_cube = get_sub_bcube(sc, t, q >> 2, q & 3)
                pts, center = cube_top_points(sub_cube), get_cube_center(sub_cube)
                sub_tile_occluded = False
                for j in occluder_ixs:
                    if sub_tile_occluded:
                        break
                    oc = occluders[j]
                    if not check_line_clip(center, camera, oc.bcube):
                        tally["centre_rejected"] += 1
                        continue
                    for s in range(16):
                        if sub_tile_occluded:
                            break
                        occ = oc.sub_cubes[s]
                        if is_all_zeros(occ):
                            continue
                        sub_tile_occluded = all(check_line_clip(p, camera, occ) for p in pts)
                if not sub_tile_occluded:
                    unoccluded += 1
            tile_occluded = unoccluded == 0
            if unoccluded == 1:
                tally["one_sub_unoccluded"] += 1
            state[i] = 1 if tile_occluded else 2  # set_last_occluded
            if tile_occluded:
                occluded_tiles.append(i)
                status[i] |= OCCLUDED
                continue
        to_draw.append((float(dist[i]), i))
        status[i] |= DRAWN
    to_draw.sort()
    ds = [d for d, _ in to_draw]
    tally["ties"] += sum(1 for k in range(1, len(ds)) if ds[k] == ds[k - 1])
    index = {(tiles[i].tx, tiles[i].ty): i for i in present}
    for _, i in to_draw:
        t = tiles[i]
        for dim in range(2):
            for dir in range(2):
                dx, dy = ((1 if dir else -1), 0) if dim == 0 else (0, (1 if dir else -1))
                adj = index.get((t.tx + dx, t.ty + dy))
                if adj is None:
                    tally["no_neighbour"] += 1
                    continue
                crack[i, 2 * dim + dir] = crack_index(dim, dir, int(lod[i]), int(lod[adj]))
                tally["adj_lower" if lod[adj] < lod[i] else "adj_equal" if lod[adj] == lod[i] else "adj_higher"] += 1
    for k in (TOO_FAR, NOT_VISIBLE, OCCLUDED_BEFORE, OCCLUDED, DRAWN):
        tally[("", "too_far", "not_visible", "occluded_before", "occluded", "drawn")[k]] += int(((status & 7) == k).sum())
    return status, dist, lod, crack, [i for _, i in to_draw], occluded_tiles, state
