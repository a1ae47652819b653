"""Cases of the scenery draw lists (terra_tiles_scenery_view[_dev]) shared by test_scenery_view_emul.py (the host emulator) and test_gpu_scenery_view.py (HIP on the
MI355X).  Every output is compared byte for byte with tests/scenery_view_model.py.

The view needs no placement, so the cases feed synthetic records on the synthetic scene of terrain_view_cases.py at S = 16: a tile is 8 wide, tile (0, 0) spans
[-4, 4]^2, get_tile_width() is 8, get_scaled_tile_radius() 48 and a flat tile's radius 5.66, so get_dist_to_camera_in_tiles(0) is (d - 5.66)/8 for a tile whose centre
lies d from the camera.  At tree_scale 1 get_scenery_dist_scale() is (d - 5.66)/40 (a tile is dropped beyond d = 45.66) and scale_val 40; in the reflection pass
(d - 5.66)/16 and 16.  water_plane_z is -5.92.  get_pt_line_thresh() is 800 and sscale 1920: a rock of radius 2^-7 becomes a point beyond 12.5, a log or stump with
radii 2^-8 a line beyond 6.25 and a stem of radius 2^-9 a line beyond 3.125 -- distances that records on the camera's axis meet exactly.
The model's result of a case is computed once per process (MODEL) with its tally, and every case carries a check on that tally: that it reaches what it is named for."""
import ctypes as C
import importlib

import numpy as np

import orclib
import scenery_view_model as sm
import terrain_view_cases as tvc
import terrain_view_model as tm
import view_model

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
FILL = 0xA5
THREADS = 256  # the workgroup of k_scenery_view
LEAFY, PLANT, ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LOG, STUMP, MUSHROOM = range(9)
ALONG_X = dict(dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
CAM = (0.25, 0.25, 0.5)
LOW = dict(pos=CAM, angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
WPZ = -5.92  # water_plane_z of the scene, to two digits: the records keep well away from it


def place_dtype():
    return importlib.import_module("3dworld_amd").SCENERY_PLACE_DTYPE


class Case:
    def __init__(self, name, tiles, build, view=LOW, valid=1, args=None, tree_scale=1.0, dxoff=0, dyoff=0, xoff2=0, yoff2=0, list_cap=None, ocean_wave_height=0.0, check=None):
        self.name, self.tiles, self.build, self.view, self.valid = name, list(tiles), build, dict(view), valid
        self.args, self.tree_scale, self.list_cap, self.ocean_wave_height = dict(args or {}), tree_scale, list_cap, ocean_wave_height
        self.dxoff, self.dyoff, self.xoff2, self.yoff2, self.check = dxoff, dyoff, xoff2, yoff2, check
        self.S, self.terrain = 16, "flat"  # (what terrain_view_cases.stats_of reads)


class Records:
    """the inputs a case builds: records [n, cap], counts, and the optional skip and radius_override arrays"""

    def __init__(self, n, cap, override=False):
        self.objs, self.counts = np.zeros((n, cap), place_dtype()), np.zeros(n, np.uint32)
        self.skip = None
        self.override = np.zeros((n, cap), f32) if override else None
        self.cap = cap

    def add(self, t, kind, pos, radius, iv0=0, p=(), override=None):
        j = int(self.counts[t])
        r = self.objs[t, j]
        r["pos"], r["radius"], r["kind"], r["iv"] = pos, radius, kind, (iv0, 0)
        r["p"][:len(p)] = p
        r["cx"], r["cy"] = j % 16, j // 16 % 16
        if override is not None:
            self.override[t, j] = override
        self.counts[t] = j + 1
        return j

    # the kinds with their record layout (terra_scenery_place)
    def rock(self, t, pos, radius):
        return self.add(t, ROCK, pos, radius, 0, (1.0, 1.1, 0.9, radius, 0.0, 0.0, 1.0, 45.0))

    def surface_rock(self, t, pos, radius):
        return self.add(t, SURFACE_ROCK, pos, radius, 0, (0.0, 0.6, 0.8))

    def voxel_rock(self, t, pos, radius, override=None):
        return self.add(t, VOXEL_ROCK, pos, radius, 12345, (), override)

    def rock_shape(self, t, pos, override=None):
        return self.add(t, ROCK_SHAPE, pos, 0.0, 777, (), override)

    def log(self, t, pos, pt2, radius, radius2=None, typ=0):
        d = np.array(pt2, np.float64) - np.array(pos, np.float64)
        length = float(np.sqrt((d * d).sum()))
        dirv = -d / length
        return self.add(t, LOG, pos, radius, typ, (radius if radius2 is None else radius2, length, dirv[0], dirv[1], dirv[2], pt2[0], pt2[1], pt2[2]))

    def stump(self, t, pos, radius, height, radius2=None, typ=0):
        return self.add(t, STUMP, pos, radius, typ, (radius if radius2 is None else radius2, height))

    def mushroom(self, t, pos, radius, height=None):
        return self.add(t, MUSHROOM, pos, radius, 0, (4.5 * radius if height is None else height,))

    def plant(self, t, pos, radius, height, typ=0):
        return self.add(t, PLANT, pos, radius, typ, (height,))

    def leafy(self, t, pos, radius, typ=1):
        return self.add(t, LEAFY, pos, radius, typ)


def tile_of(case, x, y):
    return case.tiles.index((int(np.floor((x + 4.0) / 8.0)), int(np.floor((y + 4.0) / 8.0))))


def b_thresholds(case, n):
    """on the camera's axis: every kind with a point or line form at its threshold exactly and on both sides of it; ndiv at both clamps and between; berries and
    mushrooms at theirs"""
    rec = Records(n, 96)
    x0, y0, z0 = case.view["pos"]
    zf = float(case.args.get("zoom_f", 1.0))  # the thresholds scale with the zoom: the radii shrink by it (a power of two), the distances stay
    at = lambda d, dy=0.0, dz=0.0: (x0 + d, y0 + dy, z0 + dz)  # noqa: E731
    t = lambda d: tile_of(case, x0 + d, y0)  # noqa: E731
    for d in (12.5, 12.0, 13.0):  # 2*800*2^-7 = 12.5
        rec.surface_rock(t(d), at(d), 2.0 ** -7 / zf)
        rec.rock(t(d), at(d), 2.0 ** -7 / zf)  # int(1920*2^-7/12.5) = 1: ndiv clamped at 4
    for d in (6.25, 6.0, 6.5):  # 800*(2^-8 + 2^-8) = 6.25 to the centre
        rec.log(t(d), at(d - 0.25), at(d + 0.25), 2.0 ** -8 / zf)
        rec.stump(t(d), at(d, 0.0, -0.125), 2.0 ** -8 / zf, 0.25)  # centre = pos + 0.5*height
    for d in (3.125, 3.0, 3.25):  # 2*800*2^-9 = 3.125 to pos2 = pos + 0.5*height
        rec.plant(t(d), at(d, 0.0, -0.125), 2.0 ** -9 / zf, 0.25)
    # ndiv: rocks int(1920*r/d), logs int(2*1920*r/d), stumps 2.2, stems 2, mushrooms 1
    rec.rock(0, at(2.0, 0.3), 0.1)          # 96: clamped at 32
    rec.rock(t(10.0), at(10.0, 0.3), 0.1)   # 19
    rec.log(0, at(0.9, -0.3), at(1.1, -0.3), 0.01)                  # 38: clamped at 32
    rec.log(0, at(2.9, -0.3), at(3.1, -0.3), 0.01, 0.011)          # 12
    rec.stump(0, at(1.0, 0.5, -0.3), 0.01, 0.2)                     # 42: clamped at 32
    rec.stump(0, at(3.0, 0.5, -0.3), 0.01, 0.2, 0.008)              # 14
    rec.plant(0, at(0.4, -0.1, -0.05), 0.0045, 0.1)                 # 43: clamped at 32; berries 800*0.0045/0.4 = 9: ndiv 18 clamped at 16
    rec.plant(0, at(1.0, -0.1, -0.05), 0.004, 0.1)                  # 15; berries 3.2: ndiv 6
    rec.plant(0, at(2.0, -0.1, -0.05), 0.004, 0.1)                  # 7; berries 1.6: ndiv 3 clamped at 4
    rec.mushroom(0, at(0.5, 0.2, -0.2), 0.01)                       # 38: clamped at 32; the camera above the cap
    rec.mushroom(0, at(2.0, 0.2, 0.3), 0.01)                        # 9; the cap above the camera: its underside shows
    rec.mushroom(t(8.0), at(8.0, 0.2, -0.2), 0.01)                  # 2: clamped at 3
    rec.mushroom(t(11.0), at(11.0, 0.2, -0.2), 0.01)                # beyond 1000*radius = 10
    rec.voxel_rock(0, at(3.0, -0.6), 0.05)
    rec.leafy(0, at(2.0, 0.8), 0.1)
    return rec


def ck_thresholds(t, r):
    ok = all(t[f"{k}_at_thresh"] >= 1 and t[f"{k}_small"] >= 1 and t[f"{k}_large"] >= 1 for k in ("surface_rock", "rock", "log", "stump", "plant"))
    ok = ok and all(t[f"{k}_ndiv_lo"] >= 1 and t[f"{k}_ndiv_hi"] >= 1 and t[f"{k}_ndiv_mid"] >= 1 for k in ("rock", "log", "stump", "plant", "mushroom", "berries"))
    return ok and t["mushroom_too_far"] >= 1 and t["mushroom_underside"] >= 1 and t["berries_too_small"] >= 1


RADIUS = {LEAFY: (0.06, 0.12), PLANT: (0.0025, 0.0045), SURFACE_ROCK: (0.002, 0.04), VOXEL_ROCK: (0.01, 0.2), ROCK: (0.003, 0.1), LOG: (0.003, 0.008), STUMP: (0.005, 0.015),
          MUSHROOM: (0.005, 0.01)}


def rand_obj(rec, t, kind, pos, rng):
    """a record of `kind` at pos with radii in the placement's ranges"""
    u = lambda lo, hi: float(rng.uniform(lo, hi))  # noqa: E731
    if kind == ROCK_SHAPE:
        return rec.rock_shape(t, pos, u(0.02, 0.08) if rec.override is not None and rng.integers(2) else None)
    r = u(*RADIUS[kind])
    if kind == LEAFY:
        return rec.leafy(t, pos, r, int(rng.integers(4)))
    if kind == PLANT:
        return rec.plant(t, pos, r, u(0.2, 0.4) + 0.025, int(rng.integers(7)))
    if kind == SURFACE_ROCK:
        return rec.surface_rock(t, pos, r)
    if kind == VOXEL_ROCK:
        return rec.voxel_rock(t, pos, r, r / u(0.8, 1.6) if rec.override is not None and rng.integers(2) else None)
    if kind == ROCK:
        return rec.rock(t, pos, r)
    if kind == LOG:
        ang, ln = u(0.0, 6.28), u(0.03, 0.15)
        return rec.log(t, pos, (pos[0] + ln * np.cos(ang), pos[1] + ln * np.sin(ang), pos[2] + u(-0.02, 0.02)), r, r * u(0.9, 1.1), int(rng.integers(-1, 6)))
    if kind == STUMP:
        return rec.stump(t, pos, r, u(0.025, 0.2), r * u(0.8, 1.0), int(rng.integers(-1, 6)))
    return rec.mushroom(t, pos, r, r * u(4.0, 5.0))


def scatter(case, rec, t, m, rng, kinds=range(9), z=(0.0, 0.4)):
    """m records over tile t, the kinds interleaved, minus xlate so that they land in the tile once xlate is added"""
    tx, ty = case.tiles[t]
    ox, oy = 8.0 * tx - 4.0 + 0.5 * case.dxoff, 8.0 * ty - 4.0 + 0.5 * case.dyoff
    xl = (0.5 * (case.dxoff + case.xoff2), 0.5 * (case.dyoff + case.yoff2))
    kinds = list(kinds)
    for k in range(m):
        pos = (ox + float(rng.uniform(0.0, 8.0)) - xl[0], oy + float(rng.uniform(0.0, 8.0)) - xl[1], float(rng.uniform(*z)))
        rand_obj(rec, t, kinds[k % len(kinds)], pos, rng)


def b_mixed(case, n):
    rec = Records(n, 120, override=True)
    rng = np.random.default_rng(11)
    for t in range(n):
        scatter(case, rec, t, 100 + 3 * t, rng)
    x0, y0, z0 = case.view["pos"]
    xl = (0.5 * (case.dxoff + case.xoff2), 0.5 * (case.dyoff + case.yoff2))
    for k in range(4):  # plants near enough for their berries
        rec.plant(tile_of(case, x0 - 0.5 * case.dxoff, y0 - 0.5 * case.dyoff), (x0 + 0.8 + 0.4 * k - xl[0], y0 + 0.2 * k - 0.3 - xl[1], z0 - 0.2), 0.004, 0.3, k)
    return rec


def b_big(case, n):
    """tile 0 holds more records than twice the workgroup's width, all nine kinds interleaved; tile 1 one chunk and a bit; tile 2 reports more than the capacity"""
    rec = Records(n, 2 * THREADS + 130, override=True)
    rng = np.random.default_rng(12)
    for t, m in enumerate((2 * THREADS + 130, THREADS + 1, 300)[:n]):
        scatter(case, rec, t, m, rng)
    rec.counts[2] = 5000  # above the capacity: the first `capacity` records, of which 300 are set and the rest zero (leafy plants of radius 0 at the origin)
    return rec


def b_size_scale(case, n):
    """rocks of all three kinds around 40 from the camera, large enough to stay polygons: get_size_scale on both sides of 1"""
    rec = Records(n, 64)
    rng = np.random.default_rng(13)
    for t in range(n):
        scatter(case, rec, t, 60, rng, (SURFACE_ROCK, ROCK, VOXEL_ROCK))
        rec.objs[t, :60]["radius"] = 0.06
        rec.objs[t, :60]["p"][:, 3] = 0.06
    return rec


def b_ring(case, n):
    rec = Records(n, 40)
    rng = np.random.default_rng(14)
    for t in range(n):
        scatter(case, rec, t, 36, rng)
    return rec


def b_water(case, n):
    """objects below and above the water plane at -5.92, their tops below and above get_min_water_plane_z(); water plants and leafy plants on both sides"""
    rec = Records(n, 128, override=True)
    rng = np.random.default_rng(15)
    for t in range(n):
        tx, ty = case.tiles[t]
        for k in range(40):
            x, y = 8.0 * tx - 4.0 + float(rng.uniform(0, 8)), 8.0 * ty - 4.0 + float(rng.uniform(0, 8))
            kind = (ROCK_SHAPE, SURFACE_ROCK, ROCK, VOXEL_ROCK, LEAFY, LOG, STUMP, MUSHROOM)[k % 8]
            z = (WPZ - 1.0, WPZ - 0.06, WPZ + 0.5, 0.2)[(k // 8) % 4]  # well below; below, with a top above the minimum plane; above
            j = rand_obj(rec, t, kind, (x, y, z), rng)
            if (k // 8) % 4 == 1 and kind in (SURFACE_ROCK, ROCK, VOXEL_ROCK, LEAFY):
                rec.objs[t, j]["radius"] = 0.25
                rec.override[t, j] = 0.0
        for k in range(24):  # plants: land and water types, below and above the plane
            x, y = 8.0 * tx - 4.0 + float(rng.uniform(0, 8)), 8.0 * ty - 4.0 + float(rng.uniform(0, 8))
            rec.plant(t, (x, y, (WPZ - 0.5, WPZ + 0.3)[k % 2]), 0.004, 0.3, (2, 6)[(k // 2) % 2])
    return rec


def ck_water(t, r):
    return min(t["uw_skipped"], t["uw_top_above"], t["water_plant_underwater"], t["water_plant_drawn"], t["leafy_underwater"], t["rock_shape_poly"], t["rock_shape_engine"]) >= 1


def b_frustum(case, n):
    """one record of every kind beyond each plane of a frustum with near 1 and far 30, and behind the camera inside and outside behind_sphere_mult's reach"""
    rec = Records(n, 160, override=True)
    rng = np.random.default_rng(16)
    x0, y0, z0 = case.view["pos"]
    spots = [(0.9, 0.0, 0.0), (0.3, 0.0, 0.0),          # the near plane at 1: straddling, short of it
             (30.05, 0.0, 0.0), (31.5, 0.0, 0.0),      # the far plane at 30
             (6.0, 0.0, 4.15), (6.0, 0.0, 6.0),        # the upper plane: sin(0.6) of the distance above the axis
             (6.0, 7.9, 0.0), (6.0, 11.0, 0.0),        # the side plane
             (-0.02, 0.0, 0.0), (-3.0, 0.0, 0.0),      # behind the camera
             (5.0, 0.5, 0.1)]                          # inside
    for dx, dy, dz in spots:
        x, y = x0 + dx, y0 + dy
        t = tile_of(case, x, y)
        for kind in range(9):
            rand_obj(rec, t, kind, (x, y + 0.001 * kind, z0 + dz), rng)
    return rec


def ck_frustum(t, r):
    return min(t["up_reject"], t["side_reject"], t["near_reject"], t["far_reject"], t["behind_true"], t["behind_false"], t["up_straddle"], t["near_straddle"]) >= 1


def b_tiles(case, n):
    """a skipped tile, an empty one, one whose records all have a kind outside the enum, one with a count above the capacity"""
    rec = Records(n, 48, override=True)
    rng = np.random.default_rng(17)
    for t in range(n):
        scatter(case, rec, t, 48, rng)
    rec.skip = np.zeros(n, np.uint8)
    rec.skip[1] = 1
    rec.counts[2] = 0
    rec.objs[3, :48:3]["kind"] = 9
    rec.objs[3, 1:48:6]["kind"] = -1
    rec.counts[4] = 49 + 1000
    return rec


def b_rocks(case, n):
    """rock_shapes with and without an override; voxel rocks above the frustum's upper plane that only the override's radius brings into view"""
    rec = Records(n, 32, override=True)
    x0, y0, z0 = case.view["pos"]
    for k in range(4):
        rec.rock_shape(0, (x0 + 3.0 + k, y0 + 0.2, z0 - 0.3), 0.05 * (k + 1) if k % 2 else None)
    for k in range(4):
        pos = (x0 + 10.0, y0 + 0.1 * k, z0 + 7.2)  # 0.24 beyond the plane
        rec.voxel_rock(tile_of(case, *pos[:2]), pos, 0.05, (None, 0.5, 0.01, 0.3)[k])
    rec.rock_shape(0, (x0 - 2.0, y0, z0), 0.2)  # behind the camera
    return rec


def b_details(case, n):
    """the log's end on both sides and skipped; the stump's top with each of its two terms failing"""
    rec = Records(n, 32)
    x0, y0, z0 = case.view["pos"]
    rec.log(0, (x0 + 1.9, y0, z0 - 0.2), (x0 + 2.1, y0, z0 - 0.2), 0.01)          # dir = -x: towards the camera's side, the end at pos
    rec.log(0, (x0 + 2.1, y0 + 0.3, z0 - 0.2), (x0 + 1.9, y0 + 0.3, z0 - 0.2), 0.01)  # reversed: the end at pt2
    rec.log(0, (x0 + 7.0, y0, z0 - 0.2), (x0 + 7.2, y0, z0 - 0.2), 0.01)          # polygons (16 > 7.1), but beyond 0.75*800*radius = 6: no end
    rec.stump(0, (x0 + 2.0, y0, z0 - 0.5), 0.01, 0.2)   # camera_delta.z 0.5 > height and > 0.1*2: the top
    rec.stump(0, (x0 + 0.5, y0, z0 - 0.1), 0.01, 0.2)   # 0.1 < height, 0.1 > 0.05
    rec.stump(tile_of(case, x0 + 8.0, y0), (x0 + 8.0, y0, z0 - 0.5), 0.012, 0.2)   # 0.5 > height, 0.5 < 0.8: too shallow
    rec.stump(0, (x0 + 3.0, y0 - 0.5, z0 + 0.1), 0.01, 0.2)   # the camera below the stump's base
    rec.stump(0, (x0 + 2.0, y0 + 0.5, z0 - 0.5), 0.01, 0.2, typ=-1)  # type < 0: not drawn
    return rec


def ck_details(t, r):
    return min(t["log_end_pos"], t["log_end_pt2"], t["log_no_end"], t["stump_top"], t["stump_top_below"], t["stump_top_shallow"], t["stump_top_neither"]) >= 1


RING = [(0, 0), (1, 0), (2, 1), (2, 2), (3, 0), (4, 4), (5, 0), (5, 2), (5, 3), (3, 5), (6, 0), (9, 0)]
ROW = [(0, 0), (1, 0), (2, 0)]
PW = 0.5 * np.sqrt(32.0) / 4096  # approx_pixel_width(4096) on this scene


def cases():
    clipped = dict(LOW, near=1.0, far=30.0)
    submerged = dict(LOW, pos=(0.25, 0.25, WPZ - 0.6))
    down = dict(LOW, dir=tvc._unit(1.0, 0.0, -0.3))
    back = dict(LOW, pos=(-3.9, 0.25, 0.5))  # at the tile's edge: most of tile (0, 0) lies ahead
    gsum = lambda r: [sum(w.group_counts[k] for w in r) for k in range(sm.GROUPS)]  # noqa: E731
    sweeps = lambda t, r: (sum(w.group_counts[sm.G_PLANT_LEAVES] + w.group_counts[sm.G_LEAFY_LEAVES] for w in r), sum(sum(w.group_counts[:9]) for w in r))  # noqa: E731
    return [
        Case("thresholds", ROW, b_thresholds, check=ck_thresholds),
        Case("thresholds_zoom4", ROW, b_thresholds, args=dict(zoom_f=4.0),
             check=lambda t, r: all(t[f"{k}_at_thresh"] >= 1 and t[f"{k}_small"] >= 1 and t[f"{k}_large"] >= 1 for k in ("surface_rock", "rock", "log", "stump", "plant"))),
        Case("mixed", ROW + [(1, 1)], b_mixed, check=lambda t, r: min(gsum(r)) >= 1 and t["rock_shape_engine"] >= 1),
        Case("mixed_offsets", ROW + [(1, 1)], b_mixed, dxoff=3, dyoff=-2, xoff2=-5, yoff2=4, check=lambda t, r: min(gsum(r)) >= 1),
        Case("mixed_opaque_only", ROW, b_mixed, args=dict(draw_leaves=0), check=lambda t, r: sweeps(t, r)[0] == 0 and sweeps(t, r)[1] >= 50),
        Case("mixed_leaves_only", ROW, b_mixed, args=dict(draw_opaque=0), check=lambda t, r: sweeps(t, r)[0] >= 10 and sweeps(t, r)[1] == 0 and t["rock_shape_engine"] == 0),
        Case("mixed_tree_scale_2", ROW + [(3, 0), (4, 0)], b_mixed, tree_scale=2.0, check=lambda t, r: t["dropped"] >= 1 and t["drawn"] >= 3),
        Case("view_invalid", ROW, b_mixed, valid=0, check=lambda t, r: t["invalid_view_tests"] >= 100),
        Case("size_scale", [(4, 0), (5, 0), (4, 2)], b_size_scale, check=lambda t, r: min(t["size_scale_1"], t["size_scale_below_1"]) >= 20 and t["rock_ndiv_lo"] >= 1),
        Case("tile_ring", RING, b_ring, check=lambda t, r: t["dropped"] >= 3 and t["drawn"] >= 6 and 0.97 < t["max_drawn_dist_scale"] <= 1.0 < t["min_dropped_dist_scale"] < 1.03),
        Case("tile_ring_reflection", RING, b_ring, args=dict(reflection_pass=1),
             check=lambda t, r: t["dropped"] >= 7 and t["drawn"] >= 3 and float(r[0].scale_val) == 16.0 and t["max_drawn_dist_scale"] > 0.7 and t["min_dropped_dist_scale"] < 1.05),
        Case("water_camera_above", ROW, b_water, view=down, ocean_wave_height=0.1, check=ck_water),
        Case("water_camera_below", ROW, b_water, view=submerged, ocean_wave_height=0.1,
             check=lambda t, r: t["uw_camera_below"] >= 20 and t["uw_skipped"] == 0 and t["water_plant_underwater"] == 0 and t["water_plant_drawn"] >= 1),
        Case("water_uw_skip_off", ROW, b_water, view=down, args=dict(uw_skip=0), check=lambda t, r: t["uw_gate_off"] >= 20 and t["uw_skipped"] == 0 and t["leafy_underwater"] >= 1),
        Case("water_reflection", ROW, b_water, view=down, args=dict(reflection_pass=1), check=lambda t, r: t["reflection_below_water"] >= 10 and t["water_plant_reflection"] >= 2),
        Case("shadow_pass", ROW, b_mixed, args=dict(shadow_pass=1, smap_pixel_width=PW),
             check=lambda t, r: t["smap_ndiv"] >= 20 and sum(w.group_counts[sm.G_MUSHROOM] + w.group_counts[sm.G_BERRIES] + w.group_counts[sm.G_PLD_POINTS] + w.group_counts[sm.G_PLD_LINES] for w in r) == 0
             and sum(w.group_counts[sm.G_LOG] + w.group_counts[sm.G_STUMP] for w in r) >= 5 and min(t["rock_ndiv_lo"], t["rock_ndiv_mid"], t["rock_ndiv_hi"]) >= 1),
        Case("shadow_pass_skip_small", ROW, b_mixed, args=dict(shadow_pass=1, smap_pixel_width=PW, skip_small_shadow_objs=1),
             check=lambda t, r: t["wood_skipped_in_shadow"] >= 1 and sum(w.group_counts[sm.G_LOG] + w.group_counts[sm.G_STUMP] for w in r) == 0),
        Case("shadow_pass_thresholds", ROW, b_thresholds, args=dict(shadow_pass=1, smap_pixel_width=PW * 8), check=lambda t, r: t["smap_ndiv"] >= 10 and t["log_ndiv_mid"] >= 1),
        Case("frustum_planes", [(0, 0), (1, 0), (3, 0), (4, 0), (0, 1), (1, 1), (-1, 0)], b_frustum, view=clipped, check=ck_frustum),
        Case("tiles_skip_empty_over", ROW + [(1, 1), (0, 1)], b_tiles, check=lambda t, r: t["skipped"] == 1 and t["empty"] == 1 and t["bad_kind"] >= 20),
        Case("rock_overrides", ROW, b_rocks, check=lambda t, r: min(t["rock_shape_engine"], t["rock_shape_poly"], t["voxel_rock_culled"], t["voxel_rock_poly"]) >= 2 and t["rock_shape_culled"] >= 1),
        Case("log_stump_details", ROW, b_details, check=ck_details),
        Case("big_tile", ROW, b_big, view=back, check=lambda t, r: t["max_records"] > 2 * THREADS and min(r[0].group_counts) >= 1 and t["max_entries"] > THREADS),
        Case("big_tile_short_list", ROW, b_big, view=back, list_cap=200, check=lambda t, r: min(sum(w.group_counts) for w in r) > 200),
    ]


def view_of(case):
    return tvc.view_of(case)


def args_of(case):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]), zoom_f=1.0, smap_pixel_width=0.0, window_width=1920)
    kw.update(case.args)
    return sm.Args(**kw)


def oracle_config(case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    ocfg.ocean_wave_height = case.ocean_wave_height
    return ocfg


MODEL = {}


def model(orc, case):
    """(scene, stats, view, globals, records, list capacity, results, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = oracle_config(case)
        orc.init(ocfg)
        sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
        assert abs(float(sc.water_plane_z) - WPZ) < 0.005
        stats, v = tvc.stats_of(orclib, case, float(sc.water_plane_z)), view_of(case)
        g = sm.Globals(args_of(case), case.tree_scale, case.ocean_wave_height)
        rec = case.build(case, len(case.tiles))
        tally = sm.new_tally()
        res = sm.draw(sc, v, g, case.tiles, stats, rec.objs, rec.counts, rec.skip, rec.override, case.xoff2, case.yoff2, tally)
        drawn, dropped = [float(w.dist_scale) for w in res if w.written], tally.pop("dropped_dist_scales", [])
        tally["max_drawn_dist_scale"], tally["min_dropped_dist_scale"] = max(drawn, default=0.0), min(dropped, default=9.0)
        lcap = 3 * rec.cap if case.list_cap is None else case.list_cap
        MODEL[case.name] = (sc, stats, v, g, rec, lcap, res, tally)
    return MODEL[case.name]


def lib_args(pkg, a):
    return pkg.make_scenery_view_args(float(a.behind_sphere_mult), float(a.zoom_f), float(a.smap_pixel_width), a.window_width, a.shadow_pass, a.reflection_pass, a.uw_skip,
                                      a.skip_small_shadow_objs, a.draw_opaque, a.draw_leaves)


def configure(pkg, t, case):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    cfg.ocean_wave_height = case.ocean_wave_height
    t.init_scene(cfg)
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_scale=case.tree_scale))


def compare(what, got, want, lcap):
    """the library's dict of arrays (allocated with the byte FILL) against the model's [TileResult]"""
    fill = lambda a: (a.view(np.uint8) == FILL).all()  # noqa: E731
    for t, w in enumerate(want):
        tag = f"{what}, tile {t}"
        tile = got["tile"][t]
        nlist = min(len(w.list), lcap)
        assert (int(tile["flags"]), int(tile["num_records"]), int(tile["list_written"]), tile["pad"].tolist()) == (w.flags, w.num_records, nlist, [0, 0, 0]), \
            f"{tag}: tile record {tile} != flags {w.flags}, {w.num_records} records, {nlist} entries"
        assert f32(tile["dist_scale"]).tobytes() == f32(w.dist_scale).tobytes() and f32(tile["scale_val"]).tobytes() == f32(w.scale_val).tobytes(), \
            f"{tag}: dist_scale / scale_val {tile} != {w.dist_scale!r}, {w.scale_val!r}"
        assert got["group_counts"][t].tolist() == w.group_counts, f"{tag}: group_counts {got['group_counts'][t].tolist()} != {w.group_counts}"
        m = w.num_records
        words = got["draw"][t, :m].tolist()
        assert words == w.word, f"{tag}: draw words differ, first at {[(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(words, w.word)) if a != b][:4]}"
        for key, exp in (("size_scale", w.size_scale), ("dist", w.dist)):
            e = np.array(exp, f32)
            assert got[key][t, :m].tobytes() == e.tobytes(), f"{tag}: {key} differs, first at {[(i, a, b) for i, (a, b) in enumerate(zip(got[key][t, :m].tolist(), e.tolist())) if f32(a).tobytes() != f32(b).tobytes()][:4]}"
        for key in ("draw", "size_scale", "dist"):
            assert fill(got[key][t, m:]), f"{tag}: {key} written past the records"
        assert got["list"][t, :nlist].tolist() == w.list[:nlist], f"{tag}: list differs, first at {[(i, a, b) for i, (a, b) in enumerate(zip(got['list'][t, :nlist].tolist(), w.list)) if a != b][:4]}"
        assert fill(got["list"][t, nlist:]), f"{tag}: list written past the entries"


def run_dev(pkg, t, tiles, stats, lv, la, rec, lcap, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
    """the device-pointer form on freshly allocated buffers filled with FILL -> what Terra.tiles_scenery_view returns"""
    n, cap = rec.objs.shape
    out = pkg.Terra._scenery_view_outputs(n, cap, lcap, FILL)
    bufs = {k: t.alloc(max(a.nbytes, 4)).upload(a.view(np.uint8).reshape(-1)) for k, a in out.items() if a.nbytes}
    bufs["st"] = t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8))
    bufs["ob"] = t.alloc(max(rec.objs.nbytes, 4)).upload(rec.objs.view(np.uint8).reshape(-1))
    bufs["pc"] = t.alloc(n * 4).upload(rec.counts)
    for k, a in (("sk", rec.skip), ("ov", rec.override)):
        if a is not None and a.nbytes:
            bufs[k] = t.alloc(a.nbytes).upload(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        o = [ptr(k) for k in pkg.Terra.SCENERY_VIEW_OUTPUTS]
        t.tiles_scenery_view_dev(tiles, lv, la, bufs["st"].ptr, ptr("ob"), bufs["pc"].ptr, cap, *o[:5], lcap, o[5], skip_ptr=ptr("sk"), radius_override_ptr=ptr("ov"), dxoff=dxoff,
                                 dyoff=dyoff, xoff2=xoff2, yoff2=yoff2)
        return {k: (bufs[k].download(np.uint8, (a.nbytes,)).copy().view(a.dtype).reshape(a.shape) if a.nbytes else a) for k, a in out.items()}
    finally:
        for b in bufs.values():
            b.free()


def run_case(pkg, t, orc, case, dev=False):
    sc, stats, v, g, rec, lcap, res, tally = model(orc, case)
    assert case.check(tally, res), (case.name, dict(tally))
    configure(pkg, t, case)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv, la = tvc.lib_view(pkg, v), lib_args(pkg, g.a)
    kw = dict(dxoff=case.dxoff, dyoff=case.dyoff, xoff2=case.xoff2, yoff2=case.yoff2)
    if not dev:
        got = t.tiles_scenery_view(case.tiles, lstats, lv, la, rec.objs, rec.counts, lcap, rec.skip, rec.override, fill=FILL, **kw)
    else:
        got = run_dev(pkg, t, case.tiles, lstats, lv, la, rec, lcap, **kw)
    compare(case.name + (" (dev)" if dev else ""), got, res, lcap)


def run_resident_chain(pkg, t, orc):
    """tiles_create_zvals_dev (zvals, stats) -> tiles_place_scenery_dev -> tiles_terrain_view_dev (not_drawn) -> tiles_scenery_view_dev with not_drawn as its skip bytes,
    on a 3 x 3 batch at S = 128 on one context with nothing read back in between; the model is fed from the read-back records"""
    S, cap = 128, 160
    lcap = 3 * cap
    tiles = [(x, y) for y in range(-1, 2) for x in range(1, 4)]  # over the island's shore
    n, Z = len(tiles), S + 2
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(vegetation=1.0))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3))
    t.set_scenery_params(pkg.make_scenery_params(1))
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg)
    v = view_model.make_view((float(sc.g.get_xval(S + S // 2)), 0.3, 1.5), tvc._unit(1.0, 0.3, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 60.0)
    bsm = view_model.behind_sphere_mult(0.7, 1.6)
    ta, a = tm.Args(bsm, float(orc.state().zmin), 1, 0, 0), sm.Args(bsm, 1.0, 0.0, 1920)
    lv, lta, la = tvc.lib_view(pkg, v), tvc.lib_args(pkg, ta), lib_args(pkg, a)
    out = pkg.Terra._scenery_view_outputs(n, cap, lcap, FILL)
    rec_size = pkg.SCENERY_PLACE_DTYPE.itemsize
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), ob=n * cap * rec_size, pc=n * 4, su=n, di=n * 4, lo=n, cr=n * 4, dr=n * 4, oc=n * 4, cn=8, nd=n)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    bufs.update({k: t.alloc(x.nbytes).upload(x.view(np.uint8).reshape(-1)) for k, x in out.items()})
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        bufs["ob"].upload(np.zeros(sizes["ob"], np.uint8))
        t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        t.tiles_place_scenery_dev(tiles, cap, p["ob"], p["pc"])
        t.tiles_terrain_view_dev(tiles, lv, lta, p["st"], p["su"], p["di"], p["lo"], p["cr"], p["dr"], p["oc"], p["cn"], not_drawn_ptr=p["nd"])
        o = [p[k] for k in pkg.Terra.SCENERY_VIEW_OUTPUTS]
        t.tiles_scenery_view_dev(tiles, lv, la, p["st"], p["ob"], p["pc"], cap, *o[:5], lcap, o[5], skip_ptr=p["nd"])
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
        objs = bufs["ob"].download(np.uint8, (sizes["ob"],)).copy().view(pkg.SCENERY_PLACE_DTYPE).reshape(n, cap)
        pc, nd = bufs["pc"].download(np.uint32, (n,)).copy(), bufs["nd"].download(np.uint8, (n,)).copy()
        got = {k: bufs[k].download(np.uint8, (x.nbytes,)).copy().view(x.dtype).reshape(x.shape) for k, x in out.items()}
    finally:
        for b in bufs.values():
            b.free()
    tally = sm.new_tally()
    want = sm.draw(sc, v, sm.Globals(a), tiles, stats, objs, pc, nd, None, 0, 0, tally)
    compare("resident chain", got, want, lcap)
    entries = sum(sum(w.group_counts) for w in want)
    assert int(pc.sum()) >= 200 and int(pc.max()) <= cap and 1 <= tally["skipped"] < n and tally["drawn"] >= 2 and entries >= 50, (dict(tally), pc.tolist(), nd.tolist())
    return tally
