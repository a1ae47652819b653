"""NumPy / Python restatement of pine and palm tree placement, written from the reference statements (not from the library's kernels):

    small_tree_group::gen_trees (from :439 on)      src/sm_tree.cpp:407-474
    small_tree_group::gen_trees_tt_within_radius    src/sm_tree.cpp:477-502
    get_ntrees_for_mesh_xy, maybe_add_tree          src/sm_tree.cpp:366-404
    val_signed_rand_bias_zone .. get_tree_type_from_height, can_have_pine_palm_trees_in_zrange   src/sm_tree.cpp:527-578
    calc_tree_scale / calc_tree_size / rand_tree_height / rand_tree_width / select_inst          src/sm_tree.cpp:325-338
    rand_gen_template_t                             src/rand_gen.h:19-34,60-93, src/gen_object.cpp:377-381
    get_median_height                               src/mesh_gen.cpp:487-491
    get_rel_height, get_pos_fract, extract_low_bits_pm1, dist_xy_less_than   src/inlines.h:660-663,68-73,183-195
    tile_t::update_terrain_params (veg), init_pine_tree_draw, add_new_trees   src/tiled_mesh.cpp:321-341,1430-1437,3805-3811

It is built on oracle primitives only: orc.gen_grid (the forced-sine density field and the glaciated height field of a tile), orc.eval_points(exact=1)
(get_exact_zval), orc.eval_mesh_sin_terms (the biome field; orc.tile_terrain_params is this at S = 128, which a test checks) and orc.state().  The histogram
is orc.gen_grid(0, 0, rm_scale, rm_scale, 128, 128, glaciate=0)[::4, ::4], sorted.

Types.  np.float32 for float, Python float for double, Python int for int and long; int arithmetic wraps at 32 bits where the reference's does (the seed
expressions of :371, val1 + rand() of rand_seed_mix, (int)rseed1 - (int)rseed2).  `/` and `%` of negative integers truncate toward zero.  pow(float, float) in
get_rel_height is the float overload, libm's powf (the reference includes <math.h>, which brings std::pow's overloads into the global namespace), and so are
sqrt(float), abs(float) and fabs(float).  x86-64 SSE2, no fused multiply-add.

The selection of get_ntrees_for_mesh_xy runs for every cell of a tile; it is done on int64 arrays (the same statements, array-wide).  Everything after it runs
per surviving cell with the scalar generator.  A test checks both generators against orc.rand_ints / rand_floats / rand_uniforms.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
TREE_CLASS_NONE, TREE_CLASS_PINE, TREE_CLASS_DECID, TREE_CLASS_PALM = 0, 1, 2, 3  # src/tree_3dw.h:20
TREE_NONE, T_PINE, T_DECID, T_PALM, T_SH_PINE = -1, 0, 1, 4, 5                     # src/small_tree.h:9
NUM_SMALL_TREES = 40000
TREE_DIST_RAND, SM_TREE_SIZE, TREE_DIST_SCALE = f32(0.125), f32(0.05), f32(100.0)
PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("type", np.int32), ("inst", np.int32), ("height", np.float32), ("width", np.float32),
                        ("rseed1", np.int32), ("rseed2", np.int32), ("cx", np.uint16), ("cy", np.uint16)])

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(a, b):
    return f32(_libm.powf(float(a), float(b)))


def wrap32(v):
    """an int (or int64 array) as the 32-bit int the reference's arithmetic leaves"""
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def cmod(a, b):
    return a - cdiv(a, b) * b


class RandGen:
    """rand_gen_t: long rseed1, rseed2"""

    def __init__(self, s1=1, s2=1):
        self.rseed1, self.rseed2 = int(s1), int(s2)

    def _advance(self):  # randome_int's two statements
        self.rseed1 = 40014 * cmod(self.rseed1, 53668) - 12211 * cdiv(self.rseed1, 53668)
        if self.rseed1 < 0:
            self.rseed1 += 2147483563
        self.rseed2 = 40692 * cmod(self.rseed2, 52774) - 3791 * cdiv(self.rseed2, 52774)
        if self.rseed2 < 0:
            self.rseed2 += 2147483399

    def rand(self):
        self._advance()
        v = wrap32(wrap32(self.rseed1) - wrap32(self.rseed2))
        return wrap32(v + 2147483562) if v < 1 else v

    def randd(self):
        self._advance()
        v = float(self.rseed1) - float(self.rseed2)
        if v < 1:
            v += 2147483562
        return v / 2147483563.

    def rand_seed_mix(self):
        v1 = self.rand()
        self.rseed1, self.rseed2 = self.rseed2, self.rseed1
        return wrap32(v1 + self.rand())

    def rand_mix(self):
        self.rand()
        self.rseed1, self.rseed2 = self.rseed2, self.rseed1

    def rand_float(self):
        return f32(0.000001 * cmod(self.rand(), 1000000))

    def signed_rand_float(self):
        return f32(2.0 * float(f32(self.randd())) - 1.0)

    def rand_uniform(self, a, b):
        a, b = f32(a), f32(b)
        return f32(a + f32(f32(b - a) * f32(self.randd())))


# ---- the same generator on int64 arrays (the selection runs for every cell)
def _cdiv_arr(a, b):
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) == (b < 0), q, -q)


def _cmod_arr(a, b):
    return a - _cdiv_arr(a, b) * b


def advance_arr(s1, s2):
    s1 = 40014 * _cmod_arr(s1, 53668) - 12211 * _cdiv_arr(s1, 53668)
    s1 = np.where(s1 < 0, s1 + 2147483563, s1)
    s2 = 40692 * _cmod_arr(s2, 52774) - 3791 * _cdiv_arr(s2, 52774)
    s2 = np.where(s2 < 0, s2 + 2147483399, s2)
    return s1, s2


def rand_arr(s1, s2):
    s1, s2 = advance_arr(s1, s2)
    v = wrap32(wrap32(s1) - wrap32(s2))
    return s1, s2, np.where(v < 1, wrap32(v + 2147483562), v)


class TreeParams:
    """the reference's globals of this path, with its defaults (tree_mode 1)"""

    def __init__(self, sm_tree_density=1.0, tree_scale=1.0, tree_density_thresh=0.55, tree_type_rand_zone=0.0, tree_mode=1, force_tree_class=-1,
                 only_pine_palm_trees=0, rand_gen_index=0, instanced=0, num_pine_insts=0, num_palm_insts=0):
        self.sm_tree_density, self.tree_scale, self.tree_density_thresh = f32(sm_tree_density), f32(tree_scale), f32(tree_density_thresh)
        self.tree_type_rand_zone = f32(tree_type_rand_zone)
        self.tree_mode, self.force_tree_class, self.only_pine_palm_trees, self.rand_gen_index = tree_mode, force_tree_class, only_pine_palm_trees, rand_gen_index
        self.instanced, self.num_pine_insts, self.num_palm_insts = instanced, num_pine_insts, num_palm_insts


def height_histogram(orc, state):
    """estimate_zminmax's histogram (src/mesh_gen.cpp:467-480) from the oracle's grid"""
    rm_scale = f32(1000.0 * float(f32(state.XY_SCENE_SIZE)) / float(f32(state.mesh_scale)))
    g = orc.gen_grid(0.0, 0.0, rm_scale, rm_scale, 128, 128, glaciate=0)
    return np.sort(g[::4, ::4].reshape(-1))


class Scene:
    """the globals tree placement reads: the oracle's state after orc.init(cfg) (and whatever the case changed since), the config, the tree and landscape settings"""

    def __init__(self, orc, cfg, tp, vegetation=1.0, biome_x_offset=0.0, enable_terrain_env=1, hist=None, water_plane_z=None):
        st = orc.state()
        self.orc, self.tp = orc, tp
        self.S, self.MX, self.MY = int(cfg.mesh_x), int(cfg.mesh_x), int(cfg.mesh_y)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE, self.Z_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y), f32(cfg.scene_z)
        self.DX_VAL, self.DY_VAL, self.mesh_scale = f32(st.DX_VAL), f32(st.DY_VAL), f32(st.mesh_scale)
        self.zmax_est, self.relh_adj_tex = f32(st.zmax_est), f32(st.relh_adj_tex)
        self.water_plane_z = f32(st.water_plane_z if water_plane_z is None else water_plane_z)
        self.glaciate_exp_inv = f32(1.0 / float(f32(st.glaciate_exp)))  # src/mesh_gen.cpp:393
        self.mesh_gen_mode = int(cfg.mesh_gen_mode)
        self.vegetation, self.biome_x_offset, self.enable_terrain_env = f32(vegetation), f32(biome_x_offset), enable_terrain_env
        self.hist = height_histogram(orc, st) if hist is None else np.asarray(hist, f32)
        self.XY_MULT_SIZE = self.MX * self.MY

    def get_xval(self, i):
        return f32(-self.X_SCENE_SIZE + f32(self.DX_VAL * f32(i)))

    def get_yval(self, i):
        return f32(-self.Y_SCENE_SIZE + f32(self.DY_VAL * f32(i)))

    # ---- src/tiled_mesh.cpp:321-341, veg only
    def veg_corners(self, tx, ty):
        """density[4] = {params[0][0].veg, [0][1], [1][0], [1][1]}"""
        if not self.enable_terrain_env:
            return [f32(1.0)] * 4
        S = self.S
        xv1, yv1 = self.get_xval(tx * S), self.get_yval(ty * S)
        xv2, yv2 = f32(xv1 + f32(f32(S) * self.DX_VAL)), f32(yv1 + f32(f32(S) * self.DY_VAL))
        out = []
        for yp in range(2):
            for xp in range(2):
                xv = f32(f32(self.mesh_scale * (xv2 if xp else xv1)) + self.biome_x_offset)
                yv = f32(self.mesh_scale * (yv2 if yp else yv1))
                veg_val = f32(self.orc.eval_mesh_sin_terms(f32(f32(5.0) * xv), f32(f32(5.0) * yv)))
                out.append(f32(max(f32(0.0), min(f32(1.0), f32(f32(5.0) * f32(veg_val + f32(1.5)))))))
        return out

    # ---- src/inlines.h:660-663
    def get_rel_height(self, zval):
        zmin0, zmax0 = f32(-self.zmax_est), self.zmax_est
        zv = f32(self.relh_adj_tex + f32(f32(f32(zval) - zmin0) / f32(zmax0 - zmin0)))
        return powf(zv, self.glaciate_exp_inv) if zv > 0.0 else f32(0.0)

    # ---- src/sm_tree.cpp:568-578 without a placer
    def can_have_pine_palm_trees_in_zrange(self, z_min, z_max):
        tp = self.tp
        z_min, z_max = f32(z_min), f32(z_max)
        if not (tp.tree_mode & 2):
            return False
        if z_max < self.water_plane_z:
            return False
        if tp.force_tree_class >= 0:
            return tp.force_tree_class != TREE_CLASS_NONE
        relh1, relh2 = self.get_rel_height(z_min), self.get_rel_height(z_max)
        if f32(relh1 - tp.tree_type_rand_zone) > f32(0.9):
            return False
        if f32(relh2 + tp.tree_type_rand_zone) > f32(0.6):
            return True
        if tp.tree_mode != 3:
            return True
        return float(z_min) < 0.85 * float(self.water_plane_z) and float(relh1) - 0.2 * float(tp.tree_type_rand_zone) < 0.435

    # ---- src/mesh_gen.cpp:487-491
    def get_median_height(self, pos):
        n = len(self.hist)
        if n == 0:
            return f32(pos)
        return self.hist[max(0, min(n - 1, int(f32(f32(n) * f32(pos)))))]

    # ---- src/sm_tree.cpp:527-566
    def val_signed_rand_bias_zone(self, v, ref_pt, zone_width):
        v, ref_pt, zone_width = f32(v), f32(ref_pt), f32(zone_width)
        if zone_width == 0.0:
            return v
        dist = f32(abs(f32(v - ref_pt)))
        rng = f32(zone_width - dist)
        if rng <= 0.0:
            return v
        m = f32(100.0 / float(zone_width))
        abs_v = f32(abs(f32(m * dist)))
        fract = f32(abs_v - f32(int(abs_v)))
        return f32(v + f32(rng * f32(2.0 * float(fract) - 1.0)))

    def rel_height_check(self, v, thresh, zw_scale=1.0):
        thresh = f32(thresh)
        return self.val_signed_rand_bias_zone(v, thresh, f32(f32(zw_scale) * self.tp.tree_type_rand_zone)) > thresh

    def get_tree_class_from_height(self, zpos, pine_trees_only):
        tp = self.tp
        if zpos < self.water_plane_z:
            return TREE_CLASS_NONE
        if tp.force_tree_class >= 0:
            return tp.force_tree_class
        relh = self.get_rel_height(zpos)
        if self.rel_height_check(relh, 0.9):
            return TREE_CLASS_NONE
        if self.rel_height_check(relh, 0.6):
            return TREE_CLASS_PINE
        allow_palm_trees = tp.tree_mode == 3
        if allow_palm_trees and float(zpos) < 0.85 * float(self.water_plane_z) and not self.rel_height_check(relh, 0.435, 0.2):
            return TREE_CLASS_PALM
        if pine_trees_only:
            return TREE_CLASS_NONE if tp.tree_mode == 3 else TREE_CLASS_PINE
        return TREE_CLASS_PINE if tp.only_pine_palm_trees else TREE_CLASS_DECID

    def get_tree_type_from_height(self, zpos, rgen):
        cls = self.get_tree_class_from_height(zpos, self.tp.tree_mode in (2, 3))  # world_mode == WMODE_INF_TERRAIN, for_scenery = 0
        if cls == TREE_CLASS_NONE:
            return TREE_NONE
        if cls == TREE_CLASS_PINE:
            return T_SH_PINE if cmod(rgen.rand(), 10) == 0 else T_PINE
        if cls == TREE_CLASS_PALM:
            return T_PALM
        assert cls == TREE_CLASS_DECID
        return T_DECID + cmod(rgen.rand(), 3)


def derived(sc, brush):
    """(:442-447, :455) / (:481-482)"""
    tp = sc.tp
    tscale = f32(f32(sc.Z_SCENE_SIZE * tp.tree_scale) / f32(16.0))
    tsize = f32(f32(f32(16.0) * SM_TREE_SIZE) / tp.tree_scale)
    if brush:
        ntrees_mult = f32(f32(f32(tp.sm_tree_density * tscale) * tscale) / f32(8.0))
    else:
        ntrees_mult = f32(f32(f32(f32(sc.vegetation * tp.sm_tree_density) * tscale) * tscale) / f32(8.0))
    skip_val = max(1, int(1.0 / float(np.sqrt(f32(tp.sm_tree_density * tp.tree_scale)))))
    return tscale, tsize, ntrees_mult, skip_val


def selection(sc, tx, ty, xoff2, yoff2, skip_val, nmd):
    """get_ntrees_for_mesh_xy for every visited cell of the tile at once: nmd = ntrees_mult_density per cell [rows, cols] (float32) ->
    (selected bool, rseed1, rseed2 as the selection leaves them, ntrees); asserts the case this library serves, XY_MULT_SIZE >= 2*ntrees everywhere"""
    S = sc.S
    cells = np.arange(0, S, skip_val, dtype=np.int64)
    gi, gj = np.meshgrid(ty * S + cells, tx * S + cells, indexing="ij")  # i + yoff2, j + xoff2
    ntrees = (np.minimum(f32(1.0), nmd).astype(f32) * f32(NUM_SMALL_TREES)).astype(f32).astype(np.int64)  # truncation toward zero
    assert (sc.XY_MULT_SIZE >= 2 * np.abs(ntrees)).all()
    rgi = sc.tp.rand_gen_index
    s1 = wrap32(657435 * gi + 243543 * gj + 734533 * rgi)
    s2 = wrap32(845631 * gj + 667239 * gi + 846357 * rgi)
    s1, s2, _ = rand_arr(s1, s2)       # rgen.rand()
    s1, s2, v1 = rand_arr(s1, s2)      # rand_seed_mix
    s1, s2 = s2, s1
    s1, s2, v2 = rand_arr(s1, s2)
    mix = wrap32(v1 + v2)
    div = _cdiv_arr(np.full_like(ntrees, sc.XY_MULT_SIZE), np.where(ntrees == 0, 1, ntrees))
    sel = (ntrees != 0) & (_cmod_arr(mix, div) == 0)
    return sel, s1, s2, ntrees


def maybe_add_tree(sc, rgen, tx, ty, cx, cy, xoff2, yoff2, zpos_in, tsize, skip_val):
    """:378-404 without check_hmap_normal, point_inside_voxel_terrain and check_valid_scenery_pos -> a record or None"""
    S, tp = sc.S, sc.tp
    j, i = tx * S - xoff2 + cx, ty * S - yoff2 + cy  # local indices
    rgen.rand_mix()
    xval = f32(float(sc.get_xval(j)) + 0.5 * skip_val * float(sc.DX_VAL) * float(rgen.signed_rand_float()))
    yval = f32(float(sc.get_yval(i)) + 0.5 * skip_val * float(sc.DY_VAL) * float(rgen.signed_rand_float()))
    if zpos_in != 0.0:
        zpos = f32(zpos_in)
    else:
        zpos = f32(sc.orc.eval_points([[xval, yval]], True, xoff2=xoff2, yoff2=yoff2)[0])  # interpolate_mesh_zval -> get_exact_zval(xval, yval)
    ttype = sc.get_tree_type_from_height(zpos, rgen)
    if ttype == TREE_NONE:
        return None
    rec = np.zeros((), PLACE_DTYPE)
    rec["pos"] = (xval, yval, zpos)
    rec["type"], rec["cx"], rec["cy"] = ttype, cx, cy
    if tp.instanced:
        assert ttype in (T_SH_PINE, T_PINE, T_PALM)
        start, end = (tp.num_pine_insts, tp.num_pine_insts + tp.num_palm_insts) if ttype == T_PALM else (0, tp.num_pine_insts)
        assert start < end
        rec["inst"] = start + cmod(rgen.rand(), end - start)
    else:
        height = f32(tsize * rgen.rand_uniform(0.4, 1.0))
        rec["inst"], rec["height"] = -1, height
        rec["width"] = f32(height * rgen.rand_uniform(0.25, 0.35))
    rec["rseed1"], rec["rseed2"] = wrap32(rgen.rseed1), wrap32(rgen.rseed2)
    return rec


def new_tally():
    return dict(unselected=0, density=0, none=0, pine=0, sh_pine=0, palm=0, decid=0)


def _count_type(tally, rec):
    if tally is None:
        return
    if rec is None:
        tally["none"] += 1
    else:
        t = int(rec["type"])
        tally["pine" if t == T_PINE else "sh_pine" if t == T_SH_PINE else "palm" if t == T_PALM else "decid"] += 1


def gen_trees(sc, tx, ty, xoff2=0, yoff2=0, tally=None):
    """small_tree_group::gen_trees(x1 - xoff2, y1 - yoff2, ...) from :439 on for tile (tx, ty) -> list of records, in loop order"""
    tp, S, orc = sc.tp, sc.S, sc.orc
    if tp.sm_tree_density == 0.0 or sc.vegetation == 0.0 or not (tp.tree_mode & 2):
        return []
    density = sc.veg_corners(tx, ty)
    if all(d == 0.0 for d in density):
        return []
    tscale, tsize, ntrees_mult, skip_val = derived(sc, False)
    approx_zval = sc.mesh_gen_mode == 0 or float(ntrees_mult) > 0.025
    tds = f32(float(TREE_DIST_SCALE) * (sc.XY_MULT_SIZE / 16384.0))
    xscale, yscale = f32(f32(tds * sc.DX_VAL) * sc.DX_VAL), f32(f32(tds * sc.DY_VAL) * sc.DY_VAL)
    gx1, gy1 = tx * S, ty * S  # x1 + xoff2, y1 + yoff2
    density_gen = orc.gen_grid(f32(gx1), f32(gy1), xscale, yscale, S, S, glaciate=0, force_sine=True)
    height_gen = None
    if approx_zval:
        height_gen = orc.gen_grid(f32(f32(gx1 - (sc.MX >> 1)) + f32(0.5)), f32(f32(gy1 - (sc.MY >> 1)) + f32(0.5)), sc.DX_VAL, sc.DY_VAL, S, S, glaciate=1)
    # the running sums: serial float sums, one step per visited column / row
    ncell = len(range(0, S, skip_val))
    dxv, dyv = f32(f32(skip_val) / f32(f32(S) - f32(1.0))), f32(f32(skip_val) / f32(f32(S) - f32(1.0)))
    xs, ys = np.zeros(ncell, f32), np.zeros(ncell, f32)
    xv = yv = f32(0.0)
    for k in range(ncell):
        xs[k], ys[k] = xv, yv
        xv, yv = f32(xv + dxv), f32(yv + dyv)
    XV, YV = xs[None, :], ys[:, None]
    one = f32(1.0)
    d0, d1, d2, d3 = density
    cur_density = (YV * (XV * d3 + (one - XV) * d2) + (one - YV) * (XV * d1 + (one - XV) * d0)).astype(f32)
    assert cur_density.dtype == f32
    sel, s1, s2, _ = selection(sc, tx, ty, xoff2, yoff2, skip_val, (cur_density * ntrees_mult).astype(f32))
    if tally is not None:
        tally["unselected"] += int((~sel).sum())
    out = []
    for iy, ix in np.argwhere(sel):  # rows, then columns
        cx, cy = int(ix) * skip_val, int(iy) * skip_val
        rgen = RandGen(int(s1[iy, ix]), int(s2[iy, ix]))
        hval = density_gen[cy, cx]
        if hval > sc.get_median_height(f32(tp.tree_density_thresh - f32(TREE_DIST_RAND * rgen.rand_float()))):
            if tally is not None:
                tally["density"] += 1
            continue
        rec = maybe_add_tree(sc, rgen, tx, ty, cx, cy, xoff2, yoff2, height_gen[cy, cx] if approx_zval else f32(0.0), tsize, skip_val)
        _count_type(tally, rec)
        if rec is not None:
            out.append(rec)
    return out


def gen_trees_tt_within_radius(sc, tx, ty, pos, radius, is_square, xoff2=0, yoff2=0, tally=None):
    """:477-502 as tile_t::add_new_trees calls it (xoff2 = -toff.dxoff) -> list of records"""
    tp, S = sc.tp, sc.S
    if tp.sm_tree_density == 0.0 or not (tp.tree_mode & 2):  # (the library's own early-out: the reference would divide by sqrt(0) / is not called)
        return []
    tscale, tsize, ntrees_mult, skip_val = derived(sc, True)
    px, py, radius = f32(pos[0]), f32(pos[1]), f32(radius)
    ncell = len(range(0, S, skip_val))
    sel, s1, s2, _ = selection(sc, tx, ty, xoff2, yoff2, skip_val, np.full((ncell, ncell), ntrees_mult, f32))
    out = []
    for iy in range(ncell):
        cy = iy * skip_val
        yval = sc.get_yval(ty * S - yoff2 + cy)
        if f32(abs(f32(yval - py))) > radius:
            continue
        for ix in range(ncell):
            cx = ix * skip_val
            xval = sc.get_xval(tx * S - xoff2 + cx)
            if f32(abs(f32(xval - px))) > radius:
                continue
            ddx, ddy = f32(px - xval), f32(py - yval)
            if not is_square and not (f32(f32(ddx * ddx) + f32(ddy * ddy)) < f32(radius * radius)):
                continue
            if not sel[iy, ix]:
                if tally is not None:
                    tally["unselected"] += 1
                continue
            rgen = RandGen(int(s1[iy, ix]), int(s2[iy, ix]))
            rgen.rand_float()  # to match the get_median_height() call in gen_trees()
            rec = maybe_add_tree(sc, rgen, tx, ty, cx, cy, xoff2, yoff2, f32(0.0), tsize, skip_val)
            _count_type(tally, rec)
            if rec is not None:
                out.append(rec)
    return out


def place(sc, tiles, xoff2=0, yoff2=0, skip=None, zranges=None, brush=None, tally=None):
    """the batch call: per tile the list of records.  skip[t]: can_have_trees() false; zranges[t] = (mzmin, mzmax) or None"""
    out = []
    for t, (tx, ty) in enumerate(tiles):
        if (skip is not None and skip[t]) or (zranges is not None and not sc.can_have_pine_palm_trees_in_zrange(*zranges[t])):
            out.append([])
        elif brush is None:
            out.append(gen_trees(sc, tx, ty, xoff2, yoff2, tally))
        else:
            out.append(gen_trees_tt_within_radius(sc, tx, ty, brush[0], brush[1], brush[2], xoff2, yoff2, tally))
    return out
