"""Cases of the deciduous tree draw lists (terra_tiles_decid_view[_dev]) shared by test_decid_view_emul.py (the host emulator) and test_gpu_decid_view.py (HIP on
the MI355X).  Every output is compared byte for byte with tests/decid_view_model.py (all_bcube by value).

The view needs no placement, so the cases feed synthetic records and a hand-made table on the synthetic scene of terrain_view_cases.py at S = 16: a tile is 8 wide,
tile (0, 0) spans [-4, 4]^2, X_SCENE_SIZE + Y_SCENE_SIZE is 8 (a tile whose all_bcube lies 8 or more from the camera is drawn directly, a nearer one sorted),
get_scaled_tile_radius() 48 and get_draw_tile_dist() 72.  The table's plain entries have base_radius 0.02, so size_scale is about 2/d for a tree d from the camera:
branches vanish beyond d = 40 (size_scale < 0.05), leaves beyond 72; num_leaves 1000 gives nl = min(nl, max(nl/8, 4000*size_scale*mult)).  The camera looks along +x from
(0.25, 0.25, 0.5); entry 0's sphere centre lies 0.375 above the tree's position, so a tree at z = 0.125 on the axis has its sphere centre on it, at an exact distance.
The model's result of a case is computed once per process (MODEL) with its tally, and every case carries a check on that tally: that it reaches what it is named for."""
import ctypes as C
import importlib

import numpy as np

import decid_view_model as dm
import orclib
import terrain_view_cases as tvc
import terrain_view_model as tm
import view_model

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
FILL = 0xA5
NV_FILL = 7      # the not_visible bytes a case starts with: whatever the call does not write must stay
THREADS = 256    # the workgroup of k_decid_view
LDS_IDS, LDS_KEYS, RANK_MAX = 1024, 2048, 512  # DECID_VIEW_LDS_IDS, DECID_VIEW_LDS_KEYS, DECID_VIEW_RANK_MAX (terra_decidview.hpp)
ALONG_X = dict(dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
CAM = (0.25, 0.25, 0.5)
LOW = dict(pos=CAM, angle=0.6, aspect=1.5, near=0.05, far=200.0, **ALONG_X)
LOD = (0.3, 0.15, 0.25, 0.1)  # branch start, branch end, leaf start, leaf end: billboards blend in between d = 6.7 and 13.3 (branches), 8 and 20 (leaves)
GEN, H4, LT, BT = dm.GENERATED, dm.HAS_4TH, dm.LEAF_TEX, dm.BRANCH_TEX
ALL = GEN | LT | BT
# the fixed head of every table
PLAIN, FOURTH, NO_TEX, NO_LEAVES, NOT_GEN, FEW_QUADS, BIG, FOURTH_FEW, WIDE_SPHERE, FLAT, TUNED = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10  # TUNED .. TUNED + 2: base_radius set by a case
HEAD = 13


def place_dtype():
    return importlib.import_module("3dworld_amd").DECID_PLACE_DTYPE


def make_table(n=16, seed=5):
    """a plausible shared-tree table: the head entries are what the cases name, the rest vary in size around them"""
    n = max(n, HEAD)
    d = np.zeros(n, dm.TD_DTYPE)
    rng = np.random.default_rng(seed)

    def entry(i, br=0.02, sr=0.3, zoff=0.375, lrz=0.4375, lb=(-0.3, 0.3, -0.3, 0.3, 0.125, 0.75), bb=(-0.2, 0.2, -0.2, 0.2, 0.0, 0.625), nl=1000, nbq=400, flags=ALL):
        d[i] = (br, sr, zoff, lrz, lb, bb, nl, nbq, flags, 0)
    for i in range(n):
        s = float(rng.uniform(0.7, 1.4))
        entry(i, 0.02 * s, 0.3 * s, 0.375 * s, 0.4 * s, tuple(s * x for x in (-0.3, 0.3, -0.3, 0.3, 0.125, 0.75)), tuple(s * x for x in (-0.2, 0.2, -0.2, 0.2, 0.0, 0.625)),
              int(rng.integers(200, 3000)), int(rng.integers(50, 900)), ALL | (H4 if rng.integers(3) == 0 else 0))
    entry(PLAIN)
    entry(FOURTH, nl=4000, nbq=900, flags=ALL | H4)
    entry(NO_TEX, flags=GEN)
    entry(NO_LEAVES, nl=0)
    entry(NOT_GEN, flags=LT | BT)
    entry(FEW_QUADS, nbq=13)
    entry(BIG, br=0.05, sr=0.6, zoff=0.75, lrz=0.875, lb=(-0.6, 0.6, -0.6, 0.6, 0.25, 1.5), bb=(-0.4, 0.4, -0.4, 0.4, 0.0, 1.25), nl=2500, nbq=800)
    entry(FOURTH_FEW, nbq=30, flags=ALL | H4)
    entry(WIDE_SPHERE, sr=2.0, lb=(-0.05, 0.05, -0.05, 0.05, 0.3, 0.4), bb=(-0.05, 0.05, -0.05, 0.05, 0.0, 0.4))  # its sphere reaches into the view where its boxes do not
    entry(FLAT, lb=(0.0, 0.0, -0.3, 0.3, 0.125, 0.75), bb=(0.0, 0.0, -0.2, 0.2, 0.0, 0.625))               # boxes of zero area
    for i in range(TUNED, HEAD):
        entry(i)
    return d


class Case:
    def __init__(self, name, tiles, build, view=LOW, valid=1, args=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, table=16, nv="fill", check=None):
        self.name, self.tiles, self.build, self.view, self.valid = name, list(tiles), build, dict(view), valid
        self.args, self.table, self.nv = dict(args or {}), table, nv  # nv: "fill" (an array of NV_FILL), "random" (0 / 1 bytes), None (no array)
        self.dxoff, self.dyoff, self.xoff2, self.yoff2, self.check = dxoff, dyoff, xoff2, yoff2, check
        self.S, self.terrain = 16, "flat"

    def xl(self):  # xlate
        return (0.5 * (self.dxoff + self.xoff2), 0.5 * (self.dyoff + self.yoff2))


class Records:
    """the inputs a case builds: records [n, cap], counts, the table, the optional skip bytes, and what it adds to the args"""

    def __init__(self, case, n, cap):
        self.decid, self.counts = np.zeros((n, cap), place_dtype()), np.zeros(n, np.uint32)
        self.skip, self.cap, self.args = None, cap, {}
        self.data = make_table(case.table)
        self.xl = case.xl()

    def add(self, t, pos, tree_id):
        """a tree whose position plus xlate is pos"""
        j = int(self.counts[t])
        r = self.decid[t, j]
        r["pos"] = (pos[0] - self.xl[0], pos[1] - self.xl[1], pos[2])
        r["zval"], r["type"], r["tree_id"], r["rseed1"], r["rseed2"], r["cx"], r["cy"] = pos[2], tree_id % 5, tree_id, 17 + j, 23 + j, j % 16, j // 16 % 16
        self.counts[t] = j + 1
        return j


def tile_of(case, x, y):
    """the batch index of the tile that holds (x, y); the first tile where the batch has none there (the call does not ask where a tile's records lie)"""
    key = (int(np.floor((x + 4.0) / 8.0)), int(np.floor((y + 4.0) / 8.0)))
    return case.tiles.index(key) if key in case.tiles else 0


def on_axis(case, rec, d, tree_id, dy=0.0, dz=0.0, t=None):
    """a tree whose sphere centre (for an entry with sphere_center_zoff 0.375) lies d ahead of the camera"""
    x0, y0, z0 = case.view["pos"]
    x, y = x0 + d, y0 + dy
    return rec.add(tile_of(case, min(x, 8.0 * max(tx for tx, _ in case.tiles) + 3.9), y) if t is None else t, (x, y, z0 - 0.375 + dz), tree_id)


def scatter(case, rec, t, m, rng, ids, z=(0.0, 0.3)):
    tx, ty = case.tiles[t]
    ids = list(ids)
    for k in range(m):
        rec.add(t, (8.0 * tx - 4.0 + float(rng.uniform(0.0, 8.0)), 8.0 * ty - 4.0 + float(rng.uniform(0.0, 8.0)), float(rng.uniform(*z))), ids[int(rng.integers(len(ids)))])


def size_scale_at(case, rec, d, tree_id=PLAIN):
    """the model's size_scale of a tree on the axis, d ahead"""
    tsc = _Flat()
    sc = dm.Scene(tsc)
    v, a = tvc.view_of(case), args_of(case, rec)
    x0, y0, z0 = case.view["pos"]
    return dm.calc_size_scale(sc, v, a, rec.data[tree_id], [f32(x0 + d), f32(y0), f32(z0)])


class _Flat:
    """terrain_view_model.Scene's members that decid_view_model.Scene reads, for the S = 16 scene, without an oracle (a builder has none)"""
    class g:
        DX_VAL = DY_VAL = f32(0.5)
        tile_width, scaled_tile_radius = f32(8.0), f32(48.0)
    dxoff = dyoff = 0


def b_stages(case, n):
    """every stage at which a record leaves either sweep, and every form"""
    rec = Records(case, n, 48)
    for d in (4.0, 10.0, 30.0):           # geometry; geometry and billboard; billboard only
        on_axis(case, rec, d, PLAIN)
        on_axis(case, rec, d, FOURTH, 0.5)
    on_axis(case, rec, 5.0, NO_TEX)       # no billboard texture: geometry at every distance
    on_axis(case, rec, 30.0, NO_TEX, 0.5)
    on_axis(case, rec, -3.0, PLAIN)       # behind the camera: not_visible
    on_axis(case, rec, 6.0, NO_LEAVES)    # leaves.empty()
    on_axis(case, rec, 6.0, WIDE_SPHERE, 5.8)   # 1.7 beyond the side plane: the sphere of radius 2.2 reaches in, the boxes do not
    on_axis(case, rec, 6.0, WIDE_SPHERE, 0.0, 4.9)
    on_axis(case, rec, 80.0, PLAIN, t=n - 1)    # beyond get_draw_tile_dist(): size_scale 0
    on_axis(case, rec, 50.0, PLAIN, t=n - 1)    # leaves drawn, branches below 0.05
    return rec


def ck_stages(t, r):
    return (all(t[f"l_stage_{k}"] >= 1 for k in (1, 2, 3, 4)) and all(t[f"b_stage_{k}"] >= 1 for k in (1, 3, 4)) and all(t[f"l_form_{k}"] >= 1 and t[f"b_form_{k}"] >= 1 for k in range(4))
            and t["beyond_dmax"] >= 1)


def b_lod_exact(case, n):
    """size_scale exactly at lod_start, at lod_end and between them, for both sweeps"""
    rec = Records(case, n, 16)
    for d in (5.0, 10.0, 20.0):
        on_axis(case, rec, d, PLAIN)
    a, c = size_scale_at(case, rec, 5.0), size_scale_at(case, rec, 20.0)
    rec.args = dict(lod_scales=(a, c, a, c))
    return rec


def b_lod_denom0(case, n):
    rec = Records(case, n, 16)
    for d in (5.0, 10.0, 20.0):
        on_axis(case, rec, d, PLAIN)
    b = size_scale_at(case, rec, 10.0)
    rec.args = dict(lod_scales=(b, b, b, b))
    return rec


def tune_base_radius(case, rec, d, tree_id, target):
    """base_radius of entry tree_id such that a tree d ahead has exactly size_scale == target"""
    target = f32(target)
    rec.data[tree_id]["base_radius"] = f32(0.02)
    br = f32(float(target) / float(size_scale_at(case, rec, d, tree_id)) * 0.02)
    for k in range(-64, 65):
        cand = br
        for _ in range(abs(k)):
            cand = np.nextafter(cand, f32(np.inf if k > 0 else -np.inf))
        rec.data[tree_id]["base_radius"] = cand
        if size_scale_at(case, rec, d, tree_id) == target:
            return True
    return False


def b_size_005(case, n):
    """size_scale on both sides of 0.05, as close as the statement allows.  size_scale is a float divided by DIST_C_SCALE = 0.01f, and around 0.0005 floats lie
    1.16e-7 apart (relatively) while around 0.05 they lie 7.5e-8 apart, so the division skips quotients: the float next to 0.05 (0.0500000007) is one of them -- no input
    gives it, which the builder verifies.  The cases are the two quotients that enclose 0.05: 0.049999997 (culled) and 0.050000004 (drawn)."""
    rec = Records(case, n, 16)
    x0 = f32(f32(0.05) * f32(0.01))
    xs = [x0]
    for _ in range(8):
        xs = [np.nextafter(xs[0], f32(0.0))] + xs + [np.nextafter(xs[-1], f32(1.0))]
    reach = sorted({f32(x / f32(0.01)) for x in xs})
    assert f32(0.05) not in reach and float(reach[0]) < 0.04999999 and float(reach[-1]) > 0.05000001
    targets = (max(q for q in reach if float(q) < 0.05), min(q for q in reach if float(q) >= 0.05))
    assert float(targets[1]) - float(targets[0]) < 8e-9
    for k, target in enumerate(targets):
        ok = False
        for d in np.arange(28.0, 36.0, 0.25):
            if tune_base_radius(case, rec, float(d), TUNED + k, target):
                on_axis(case, rec, float(d), TUNED + k)
                ok = True
                break
        assert ok, f"no base_radius gives size_scale {target!r}"
    on_axis(case, rec, 30.0, PLAIN)
    return rec


def b_dmax(case, n):
    """a tree exactly at get_draw_tile_dist() = 72 (dist_sq == dmax*dmax: drawn) and one float beyond"""
    rec = Records(case, n, 16)
    x0, y0, z0 = case.view["pos"]
    rec.add(n - 1, (x0 + 72.0, y0, z0 - 0.375), PLAIN)
    rec.add(n - 1, (float(np.nextafter(f32(x0 + 72.0), f32(100.0))), y0, z0 - 0.375), PLAIN)
    rec.add(n - 1, (x0 + 71.0, y0 + 1.0, z0 - 0.375), FOURTH)
    return rec


def b_counts(case, n):
    """nl and num on each of their three branches, with and without HAS_4TH; low_detail overridden by the fourth-order rule"""
    rec = Records(case, n, 64)
    for k, d in enumerate((1.0, 1.5, 3.0, 6.0, 12.0, 24.0, 38.0, 39.6, 60.0, 68.0)):
        for q, tid in enumerate((PLAIN, FOURTH, FEW_QUADS, FOURTH_FEW)):
            on_axis(case, rec, d, tid, 0.05 * q * d)
    return rec


def ck_counts(t, r):
    return all(t[f"{s}_{k}{q}"] >= 1 for s in ("nl", "num") for k in ("floor", "product", "full") for q in ("", "_4th")) and t["low_detail_overridden"] >= 1 and t["low_detail"] >= 1


def b_on_centre(case, n):
    """the camera on two trees' sphere centres: InvSqrt(0), and unsigned(double) of a product beyond 64 bits"""
    rec = Records(case, n, 16)
    x0, y0, z0 = case.view["pos"]
    rec.add(0, (x0, y0, z0 - 0.375), PLAIN)
    rec.add(0, (x0, y0, z0 - 0.375), FOURTH)
    on_axis(case, rec, 3.0, PLAIN)
    return rec


def b_sorted(case, n):
    """the camera's tile: two pairs of equal keys (mirror images about the axis), trees behind the camera that are culled, the rest scattered"""
    rec = Records(case, n, 64)
    rng = np.random.default_rng(21)
    scatter(case, rec, 0, 30, rng, range(case.table))
    for d, w in ((2.0, 1.0), (3.0, 0.5)):
        on_axis(case, rec, d, PLAIN, w, t=0)
        on_axis(case, rec, d, FOURTH, -w, t=0)
    on_axis(case, rec, -2.0, PLAIN, t=0)
    on_axis(case, rec, -3.5, BIG, 0.5, t=0)
    scatter(case, rec, 1, 20, rng, range(case.table))
    return rec


def b_mixed(case, n):
    """records over every tile from all ids of the table, some dropped"""
    rec = Records(case, n, 140)
    rng = np.random.default_rng(22)
    for t in range(n):
        scatter(case, rec, t, 100 + 10 * t, rng, range(case.table))
    return rec


def b_three_ids(case, n):
    """long runs: three ids, and more billboard entries in a tile than k_decid_view places by rank, so that its histogram runs"""
    rec = Records(case, n, RANK_MAX + 188)
    rng = np.random.default_rng(23)
    for t in range(n):
        scatter(case, rec, t, RANK_MAX + 138, rng, (PLAIN, FOURTH, BIG))
    return rec


def b_zero_area(case, n):
    """tile 1 lies behind the camera and would be culled, but its one tree's boxes have zero area: the cull is off; tile 2, beside it, is culled"""
    rec = Records(case, n, 16)
    rng = np.random.default_rng(24)
    scatter(case, rec, 0, 10, rng, (PLAIN, FOURTH))
    tx, ty = case.tiles[1]
    rec.add(1, (8.0 * tx, 8.0 * ty, 0.1), FLAT)
    scatter(case, rec, 2, 10, rng, (PLAIN, FOURTH))
    return rec


def b_big(case, n):
    """tile 0 holds more records than twice the workgroup's width; tile 1 one chunk and one; tile 2 reports more than the capacity"""
    rec = Records(case, n, 2 * THREADS + 130)
    rng = np.random.default_rng(25)
    for t, m in enumerate((2 * THREADS + 130, THREADS + 1, 300)[:n]):
        scatter(case, rec, t, m, rng, range(case.table))
    rec.counts[2] = 5000  # the first `capacity` records, of which 300 are set and the rest zero (entry 0 at the origin)
    return rec


def b_full_lists(case, n):
    """a count above a short capacity, and every record that is read in all four lists: they are full to the capacity"""
    rec = Records(case, n, 40)
    rng = np.random.default_rng(26)
    for t in range(n):
        for k in range(rec.cap):
            on_axis(case, rec, 10.0 + 0.05 * k, (PLAIN, BIG, FOURTH)[k % 3], float(rng.uniform(-1.5, 1.5)), t=t)
    rec.counts[0] = 100
    rec.args = dict(lod_scales=(5.0, 0.001, 5.0, 0.001))  # every tree blends
    return rec


def b_dropped(case, n):
    rec = Records(case, n, 64)
    rng = np.random.default_rng(27)
    for t in range(n):
        scatter(case, rec, t, 60, rng, range(case.table))
        rec.decid[t, 0:60:7]["tree_id"] = -1
        rec.decid[t, 3:60:7]["tree_id"] = case.table + t
        rec.decid[t, 5:60:7]["tree_id"] = NOT_GEN
    rec.decid[0, 1]["tree_id"] = 2 ** 31 - 1
    rec.decid[0, 2]["tree_id"] = -2 ** 31
    return rec


def b_big_capacity(case, n):
    """a capacity beyond the pairs k_decid_view keeps in LDS: the sorted tile and the billboard lists rank in the driver's scratch"""
    rec = Records(case, n, LDS_KEYS + 52)
    rng = np.random.default_rng(28)
    for t in range(n):
        scatter(case, rec, t, 300 + 40 * t, rng, range(case.table))
    return rec


def b_shadow(case, n):
    """the shadow pass with far = 30: trees beyond it (the distance cull), beside the frustum (the sphere cull), and drawn"""
    rec = Records(case, n, 96)
    rng = np.random.default_rng(29)
    for t in range(n):
        scatter(case, rec, t, 70, rng, range(case.table))
    for d in (29.0, 31.0, 45.0):
        on_axis(case, rec, d, PLAIN)
    on_axis(case, rec, 10.0, PLAIN, 12.0)
    return rec


def b_frustum(case, n):
    """a tree of every head entry beyond each plane of a frustum with near 1 and far 30, and behind the camera inside and outside behind_sphere_mult's reach"""
    rec = Records(case, n, 160)
    x0, y0, z0 = case.view["pos"]
    spots = [(1.2, 0.0, 0.0), (0.3, 0.0, 0.0), (30.2, 0.0, 0.0), (31.5, 0.0, 0.0), (6.0, 0.0, 4.15), (6.0, 0.0, 6.0), (6.0, 7.9, 0.0), (6.0, 11.0, 0.0),
             (-0.02, 0.0, 0.0), (-3.0, 0.0, 0.0), (5.0, 0.5, 0.1)]
    for dx, dy, dz in spots:
        x, y = x0 + dx, y0 + dy
        for tid in (PLAIN, FOURTH, NO_TEX, BIG, WIDE_SPHERE):
            rec.add(tile_of(case, x, y), (x, y + 0.001 * tid, z0 + dz - 0.375), tid)
    return rec


def ck_frustum(t, r):
    return min(t["up_reject"], t["side_reject"], t["near_reject"], t["far_reject"], t["behind_true"], t["behind_false"], t["up_straddle"], t["side_straddle"]) >= 1


def b_tiles(case, n):
    """a skipped tile, an empty one, one whose records are all dropped, one with a count above the capacity"""
    rec = Records(case, n, 48)
    rng = np.random.default_rng(30)
    for t in range(n):
        scatter(case, rec, t, 48, rng, range(case.table))
    rec.skip = np.zeros(n, np.uint8)
    rec.skip[1] = 1
    rec.counts[2] = 0
    rec.decid[3, :, ]["tree_id"] = NOT_GEN
    rec.decid[3, ::2]["tree_id"] = -1
    rec.counts[4] = 49 + 1000
    return rec


ROW = [(0, 0), (1, 0), (2, 0)]
FAR_ROW = ROW + [(4, 0), (9, 0)]


def cases():
    clipped = dict(LOW, near=1.0, far=30.0)
    back = dict(LOW, pos=(-3.9, 0.25, 0.5))  # at the tile's edge: most of tile (0, 0) lies ahead
    lod = dict(lod_scales=LOD)
    listed = lambda r: [sum(len(x) for x in (w.leaf_list, w.branch_list, w.leaf_bb, w.branch_bb)) for w in r]  # noqa: E731
    return [
        Case("stages_forms", FAR_ROW, b_stages, args=lod, check=ck_stages),
        Case("lod_exact", ROW, b_lod_exact, check=lambda t, r: min(t["l_at_start"], t["l_at_end"], t["l_between"], t["b_at_start"], t["b_at_end"], t["b_between"]) >= 1
             and min(t["l_form_1"], t["l_form_2"], t["l_form_3"], t["b_form_1"], t["b_form_2"], t["b_form_3"]) >= 1),
        Case("lod_denom0", ROW, b_lod_denom0, check=lambda t, r: min(t["l_denom0"], t["b_denom0"], t["l_at_start"], t["b_at_start"], t["l_above_start"], t["l_form_3"], t["b_form_3"]) >= 1),
        Case("size_005", FAR_ROW, b_size_005, args=lod, check=lambda t, r: t["b_size_below_005"] == 1 and t["b_size_above_005"] == 2 and t["b_stage_4"] == 1 and t["b_form_3"] == 2),
        Case("draw_tile_dist", FAR_ROW, b_dmax, args=lod, check=lambda t, r: t["at_dmax"] == 2 and t["beyond_dmax"] == 2 and t["l_stage_4"] == 1 and t["l_form_3"] >= 1),
        Case("counts", FAR_ROW, b_counts, args=dict(billboards=0), check=ck_counts),
        Case("camera_on_centre", ROW, b_on_centre, args=lod, check=lambda t, r: t["conv_overflow"] == 4 and t["nl_floor"] >= 1 and t["num_floor_4th"] >= 1),
        Case("sorted_ties", ROW, b_sorted, args=dict(lod_scales=(2.0, 0.2, 2.0, 0.2)), check=lambda t, r: t["sorted"] >= 1 and t["sorted_ties"] >= 2 and t["sorted_culled"] >= 2 and len(r[0].leaf_bb) >= 3),
        Case("direct_far_tile", [(3, 0), (4, 1), (0, 0)], b_mixed, args=lod, check=lambda t, r: t["direct"] == 2 and t["sorted"] == 1 and len(r[0].leaf_list) >= 10),
        Case("bcube_zero_area", [(0, 0), (-2, 0), (-2, 1)], b_zero_area, args=lod,
             check=lambda t, r: t["tile_zero_area"] == 1 and t["tile_culled"] == 1 and r[1].flags & dm.TILE_DRAWN and not r[2].flags & dm.TILE_DRAWN and r[2].num_trees == 10),
        Case("big_tile", ROW, b_big, view=back, args=lod, check=lambda t, r: t["max_records"] > 2 * THREADS and r[2].num_trees > 2 * THREADS and min(listed(r)) > THREADS),
        Case("full_lists", ROW[:2], b_full_lists, check=lambda t, r: all(len(x) == 40 for w in r for x in (w.leaf_list, w.branch_list, w.leaf_bb, w.branch_bb))),
        Case("dropped_records", ROW, b_dropped, args=lod, check=lambda t, r: min(t["dropped_negative"], t["dropped_outside"], t["dropped_not_generated"]) >= 9 and t["tile_drawn"] == 3),
        Case("big_table", ROW, b_mixed, args=lod, table=LDS_IDS + 476, check=lambda t, r: t["max_ids_in_tile"] > 90 and sum(len(w.leaf_bb) + len(w.branch_bb) for w in r) >= 30),
        Case("three_ids", ROW, b_three_ids, view=back, args=dict(lod_scales=(5.0, 0.001, 5.0, 0.001)),
             check=lambda t, r: t["max_ids_in_tile"] == 3 and t["max_run"] >= 150 and max(len(w.leaf_bb) for w in r) > RANK_MAX and max(len(w.branch_bb) for w in r) > RANK_MAX),
        Case("all_ids", ROW + [(1, 1)], b_mixed, args=lod, check=lambda t, r: t["max_ids_in_tile"] == 15 and t["dropped_not_generated"] >= 5 and min(listed(r)) >= 20),
        Case("big_capacity", ROW[:2], b_big_capacity, args=lod, check=lambda t, r: t["sorted"] == 2 and min(listed(r)) >= 100),
        Case("big_capacity_big_table", ROW[:2], b_big_capacity, args=lod, table=LDS_IDS + 476, check=lambda t, r: t["sorted"] == 2 and t["max_ids_in_tile"] > 200),
        Case("shadow_pass", ROW + [(4, 0), (5, 0)], b_shadow, view=dict(LOW, far=30.0), args=dict(lod, shadow_pass=1),
             check=lambda t, r: min(t["l_stage_5"], t["l_stage_6"], t["b_stage_5"], t["shadow_leaves_drawn"], t["shadow_branches_drawn"]) >= 3 and t["nv_written"] == 0
             and t["sorted"] == 0 and sum(len(w.leaf_bb) + len(w.branch_bb) for w in r) == 0),
        Case("reflection_pass", ROW, b_mixed, args=dict(lod, reflection_pass=1), check=lambda t, r: t["reflection_low_detail"] >= 20),
        Case("leaf_color_changed", ROW, b_mixed, args=dict(lod, leaf_color_changed=1), check=lambda t, r: t["lcc_drawn_not_visible"] >= 10 and t["l_stage_1"] == 0 and t["l_stage_3"] == 0),
        Case("leaves_only", ROW, b_mixed, args=dict(lod, draw_branches=0), check=lambda t, r: sum(len(w.branch) for w in r) == 0 and t["nv_written"] >= 300),
        Case("branches_only", ROW, b_mixed, args=dict(lod, draw_leaves=0), nv="random", check=lambda t, r: sum(len(w.leaf) for w in r) == 0 and t["nv_read_1"] >= 50 and t["nv_written"] == 0),
        Case("branches_only_no_array", ROW, b_mixed, args=dict(lod, draw_leaves=0), nv=None, check=lambda t, r: t["nv_read_1"] == 0 and t["b_stage_3"] >= 10),
        Case("no_not_visible_array", ROW, b_mixed, args=lod, nv=None, check=lambda t, r: t["nv_read_1"] >= 50),
        Case("no_billboards", ROW, b_mixed, args=dict(lod, billboards=0), check=lambda t, r: sum(len(w.leaf_bb) + len(w.branch_bb) for w in r) == 0 and t["l_form_1"] >= 50),
        Case("offsets", ROW + [(1, 1)], b_mixed, args=lod, dxoff=3, dyoff=-2, xoff2=-5, yoff2=4, check=lambda t, r: t["sorted"] >= 1 and min(listed(r)) >= 20),
        Case("frustum_planes", [(0, 0), (1, 0), (3, 0), (4, 0), (0, 1), (1, 1), (-1, 0)], b_frustum, view=clipped, args=lod, check=ck_frustum),
        Case("tiles_skip_empty", ROW + [(1, 1), (0, 1)], b_tiles, args=lod, check=lambda t, r: t["skipped"] == 1 and t["empty"] == 2 and r[4].num_trees >= 40),
        Case("view_invalid", ROW, b_mixed, valid=0, args=lod, check=lambda t, r: t["invalid_view_tests"] >= 100 and t["tile_culled"] == 0),
    ]


def args_of(case, rec):
    kw = dict(behind_sphere_mult=view_model.behind_sphere_mult(case.view["angle"], case.view["aspect"]), zoom_f=1.0)
    kw.update(case.args)
    kw.update(rec.args)
    return dm.Args(**kw)


def nv_of(case, rec):
    n, cap = rec.decid.shape
    if case.nv is None:
        return None
    if case.nv == "random":
        return np.random.default_rng(31).integers(0, 2, (n, cap)).astype(np.uint8)
    return np.full((n, cap), NV_FILL, np.uint8)


MODEL = {}


def model(orc, case):
    """(scene, view, args, records, not_visible in, results, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
        orc.init(ocfg)
        tsc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
        assert tsc.g.tile_width == _Flat.g.tile_width and tsc.g.scaled_tile_radius == _Flat.g.scaled_tile_radius and tsc.g.DX_VAL == _Flat.g.DX_VAL
        rec = case.build(case, len(case.tiles))
        v, a = tvc.view_of(case), args_of(case, rec)
        nv = nv_of(case, rec)
        tally = dm.new_tally()
        res = dm.draw(tsc, v, a, case.tiles, rec.data, rec.decid, rec.counts, rec.skip, nv, case.xoff2, case.yoff2, tally)
        MODEL[case.name] = (tsc, v, a, rec, nv, res, tally)
    return MODEL[case.name]


def lib_args(pkg, a):
    return pkg.make_decid_view_args(float(a.behind_sphere_mult), float(a.zoom_f), [float(x) for x in a.lod_scales], a.shadow_pass, a.reflection_pass, a.billboards,
                                    a.leaf_color_changed, a.draw_leaves, a.draw_branches)


def configure(pkg, t, case, num_shared=None):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    t.set_decid_params(pkg.make_decid_params(num_trees=100, num_shared_trees=max(case.table, HEAD) if num_shared is None else num_shared))


PER_RECORD = (("leaf", "leaf_word", "leaf_scale", "leaf_opacity", "leaf_num"), ("branch", "branch_word", "branch_scale", "branch_opacity", "branch_num"))


def compare(what, got, want, nv_got=None, nv_in=None):
    """the library's dict of arrays (allocated with the byte FILL) against the model's [TileResult]; nv_got / nv_in: the not_visible array after and before the call"""
    fill = lambda a: (np.ascontiguousarray(a).view(np.uint8) == FILL).all()  # noqa: E731
    cap = got["leaf_word"].shape[1]
    for t, w in enumerate(want):
        tag = f"{what}, tile {t}"
        tile = got["tile"][t]
        lists = (w.leaf_list, w.branch_list, w.leaf_bb, w.branch_bb)
        assert [int(x) for x in tile.tolist()[:6]] + tile["pad"].tolist() == [w.flags, w.num_trees] + [len(x) for x in lists] + [0, 0], f"{tag}: tile record {tile} != flags {w.flags}, " \
            f"{w.num_trees} trees, {[len(x) for x in lists]}"
        assert got["list_counts"][t].tolist() == [len(x) for x in lists], f"{tag}: list_counts {got['list_counts'][t].tolist()} != {[len(x) for x in lists]}"
        assert np.array_equal(got["all_bcube"][t], np.array(w.bcube, f32)), f"{tag}: all_bcube {got['all_bcube'][t].tolist()} != {[float(x) for x in w.bcube]}"
        for side, kw, ks, ko, kn in PER_RECORD:
            recs = getattr(w, side)
            for j in range(cap):
                if j in recs:
                    r = recs[j]
                    g = (int(got[kw][t, j]), got[ks][t, j].tobytes(), got[ko][t, j].tobytes(), int(got[kn][t, j]))
                    e = (r.word, f32(r.scale).tobytes(), f32(r.opacity).tobytes(), r.num)
                    assert g == e, f"{tag}: {side} record {j}: word {g[0]:#x} scale {got[ks][t, j]!r} opacity {got[ko][t, j]!r} num {g[3]} != {r.word:#x} {r.scale!r} {r.opacity!r} {r.num}"
                else:
                    assert all(fill(got[k][t, j]) for k in (kw, ks, ko, kn)), f"{tag}: {side} record {j} written"
        for key, exp in (("leaf_list", w.leaf_list), ("branch_list", w.branch_list)):
            m = len(exp)
            assert got[key][t, :m].tolist() == exp, f"{tag}: {key} differs, first at {[(i, a, b) for i, (a, b) in enumerate(zip(got[key][t, :m].tolist(), exp)) if a != b][:4]}"
            assert fill(got[key][t, m:]), f"{tag}: {key} written past the entries"
        for key, exp in (("leaf_bb", w.leaf_bb), ("branch_bb", w.branch_bb)):
            m = len(exp)
            e = np.zeros(m, got[key].dtype)
            for i, (tid, rj, pos, op) in enumerate(exp):
                e[i] = (tid, rj, pos, op)
            assert got[key][t, :m].tobytes() == e.tobytes(), f"{tag}: {key} differs, first at {[(i, a, b) for i, (a, b) in enumerate(zip(got[key][t, :m].tolist(), e.tolist())) if a != b][:3]}"
            assert fill(got[key][t, m:]), f"{tag}: {key} written past the entries"
        if nv_got is not None:
            e = nv_in[t].copy()
            for j, b in w.not_visible.items():
                e[j] = b
            assert nv_got[t].tolist() == e.tolist(), f"{tag}: not_visible differs at {[(j, a, b) for j, (a, b) in enumerate(zip(nv_got[t].tolist(), e.tolist())) if a != b][:6]}"


def run_dev(pkg, t, tiles, lv, la, rec, nv, dxoff=0, dyoff=0, xoff2=0, yoff2=0, out=None):
    """the device-pointer form on freshly allocated buffers filled with FILL (or holding `out`) -> (what Terra.tiles_decid_view returns, not_visible after the call)"""
    n, cap = rec.decid.shape
    out = pkg.Terra._decid_view_outputs(n, cap, FILL) if out is None else out
    up = lambda a: t.alloc(max(a.nbytes, 4)).upload(np.ascontiguousarray(a).view(np.uint8).reshape(-1))  # noqa: E731
    bufs = {k: up(a) for k, a in out.items()}
    bufs["td"], bufs["de"], bufs["pc"] = up(rec.data), up(rec.decid), up(rec.counts)
    if rec.skip is not None:
        bufs["sk"] = up(rec.skip)
    if nv is not None:
        bufs["nv"] = up(nv)
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_decid_view_dev(tiles, lv, la, bufs["td"].ptr, len(rec.data), bufs["de"].ptr, bufs["pc"].ptr, cap, [bufs[k].ptr for k in pkg.Terra.DECID_VIEW_OUTPUTS],
                               skip_ptr=ptr("sk"), not_visible_ptr=ptr("nv"), dxoff=dxoff, dyoff=dyoff, xoff2=xoff2, yoff2=yoff2)
        got = {k: (bufs[k].download(np.uint8, (a.nbytes,)).copy().view(a.dtype).reshape(a.shape) if a.nbytes else a) for k, a in out.items()}
        return got, (None if nv is None else bufs["nv"].download(np.uint8, (nv.size,)).copy().reshape(nv.shape))
    finally:
        for b in bufs.values():
            b.free()


def run_lib(pkg, t, case, rec, la, nv, dev, out=None):
    """one call of either form -> (outputs, not_visible after)"""
    lv = tvc.lib_view(pkg, tvc.view_of(case))
    kw = dict(dxoff=case.dxoff, dyoff=case.dyoff, xoff2=case.xoff2, yoff2=case.yoff2)
    if dev:
        return run_dev(pkg, t, case.tiles, lv, la, rec, nv, out=out, **kw)
    nv = None if nv is None else nv.copy()
    return t.tiles_decid_view(case.tiles, lv, la, rec.data, rec.decid, rec.counts, rec.skip, nv, fill=FILL, out=out, **kw), nv


def run_case(pkg, t, orc, case, dev=False):
    tsc, v, a, rec, nv, res, tally = model(orc, case)
    assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})
    configure(pkg, t, case)
    got, nv_got = run_lib(pkg, t, case, rec, lib_args(pkg, a), nv, dev)
    compare(case.name + (" (dev)" if dev else ""), got, res, nv_got, nv)


def run_split(pkg, t, orc, case, dev=True):
    """a leaves-only call followed by a branches-only call through the not_visible array gives what the combined call gives, byte for byte"""
    tsc, v, a, rec, nv, res, tally = model(orc, case)
    configure(pkg, t, case)
    both, nv_both = run_lib(pkg, t, case, rec, lib_args(pkg, a), nv, dev)
    compare(case.name + " (combined)", both, res, nv_both, nv)
    la = lib_args(pkg, a)
    la.draw_branches = 0
    first, nv1 = run_lib(pkg, t, case, rec, la, nv, dev)
    la.draw_branches, la.draw_leaves = 1, 0
    second, nv2 = run_lib(pkg, t, case, rec, la, nv1, dev, out={k: x.copy() for k, x in first.items()})
    assert nv2.tobytes() == nv1.tobytes() == nv_both.tobytes()
    both_flags = both["tile"]["flags"].copy()
    for k in pkg.Terra.DECID_VIEW_OUTPUTS:
        if k in ("tile", "list_counts"):
            continue
        assert second[k].tobytes() == both[k].tobytes(), k
    L, B = dm.TILE_LEAVES, dm.TILE_BRANCHES
    assert ((first["tile"]["flags"] | second["tile"]["flags"]) == both_flags).all() and not (first["tile"]["flags"] & B).any() and not (second["tile"]["flags"] & L).any()
    assert (first["list_counts"][:, (0, 2)] == both["list_counts"][:, (0, 2)]).all() and (second["list_counts"][:, (1, 3)] == both["list_counts"][:, (1, 3)]).all()
    assert not first["list_counts"][:, (1, 3)].any() and not second["list_counts"][:, (0, 2)].any()


def run_resident_chain(pkg, t, orc):
    """tiles_create_zvals_dev (zvals, stats) -> tiles_place_decid_trees_dev -> tiles_tree_ao_shadows_dev (the records' other reader) -> tiles_terrain_view_dev
    (not_drawn) -> tiles_decid_view_dev with not_drawn as its skip bytes, on a 3 x 3 batch at S = 128 on one context with nothing read back in between; the model is
    fed from the read-back records"""
    S, cap, cap_l, shared = 128, 384, 2048, 16
    tiles = [(x, y) for y in range(-1, 2) for x in range(1, 4)]  # from the island's top out over its shore
    n, W, Z = len(tiles), S + 1, S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=shared))
    t.set_tree_size_params(pkg.make_tree_size_params())
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    tsc = tm.Scene(orc, ocfg)
    data = make_table(shared)
    data["flags"][NOT_GEN] |= GEN  # (every shared tree of a running engine is generated; one of the 16 stays without textures)
    for k in ("base_radius", "sphere_radius", "sphere_center_zoff", "lr_z_cent", "leaves_bcube", "branches_bcube"):  # trees of TREE_SIZE's order: a fifth of the cases' size
        data[k] = (data[k] * f32(0.2)).astype(f32)
    by_id = data["sphere_radius"].copy()
    v = view_model.make_view((float(tsc.g.get_xval(S + S // 2)), 0.3, 1.5), tvc._unit(1.0, 0.3, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 60.0)
    bsm = view_model.behind_sphere_mult(0.7, 1.6)
    ta, a = tm.Args(bsm, float(orc.state().zmin), 1, 0, 0), dm.Args(bsm, 1.0, (0.06, 0.03, 0.05, 0.02))
    lv, lta, la = tvc.lib_view(pkg, v), tvc.lib_args(pkg, ta), lib_args(pkg, a)
    out = pkg.Terra._decid_view_outputs(n, cap, FILL)
    nv = np.full((n, cap), NV_FILL, np.uint8)
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), de=n * cap * pkg.DECID_PLACE_DTYPE.itemsize, pc=n * 4, tmap=n * W * W * 2, upd=n, trm=n * 4, lc=n * 4,
                 su=n, di=n * 4, lo=n, cr=n * 4, dr=n * 4, oc=n * 4, cn=8, nd=n)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    bufs.update({k: t.alloc(x.nbytes).upload(x.view(np.uint8).reshape(-1)) for k, x in out.items()})
    bufs["td"], bufs["id"], bufs["nv"] = t.alloc(data.nbytes).upload(data.view(np.uint8)), t.alloc(by_id.nbytes).upload(by_id), t.alloc(nv.size).upload(nv.reshape(-1))
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        bufs["de"].upload(np.zeros(sizes["de"], np.uint8))
        t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        t.tiles_place_decid_trees_dev(tiles, cap, p["de"], p["pc"], 0, 0, None, p["st"], p["z"])
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, p["tmap"], None, None, 0, p["de"], p["pc"], cap, None, p["id"], shared, None, p["upd"], p["trm"], p["lc"])
        t.tiles_terrain_view_dev(tiles, lv, lta, p["st"], p["su"], p["di"], p["lo"], p["cr"], p["dr"], p["oc"], p["cn"], not_drawn_ptr=p["nd"])
        t.tiles_decid_view_dev(tiles, lv, la, p["td"], shared, p["de"], p["pc"], cap, [p[k] for k in pkg.Terra.DECID_VIEW_OUTPUTS], skip_ptr=p["nd"], not_visible_ptr=p["nv"])
        decid = bufs["de"].download(np.uint8, (sizes["de"],)).copy().view(pkg.DECID_PLACE_DTYPE).reshape(n, cap)
        pc, nd = bufs["pc"].download(np.uint32, (n,)).copy(), bufs["nd"].download(np.uint8, (n,)).copy()
        nv_got = bufs["nv"].download(np.uint8, (nv.size,)).copy().reshape(nv.shape)
        got = {k: bufs[k].download(np.uint8, (x.nbytes,)).copy().view(x.dtype).reshape(x.shape) for k, x in out.items()}
    finally:
        for b in bufs.values():
            b.free()
    tally = dm.new_tally()
    want = dm.draw(tsc, v, a, tiles, data, decid, pc, nd, nv, 0, 0, tally)
    compare("resident chain", got, want, nv_got, nv)
    entries = [sum(len(w.leaf_list) for w in want), sum(len(w.branch_list) for w in want), sum(len(w.leaf_bb) for w in want), sum(len(w.branch_bb) for w in want)]
    assert int(pc.sum()) >= 200 and int(pc.max()) <= cap and 1 <= tally["skipped"] < n and tally["tile_drawn"] >= 2 and min(entries) >= 5, (dict(tally), pc.tolist(), nd.tolist(), entries)
    return tally
