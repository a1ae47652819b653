"""NumPy / Python restatement of deciduous tree placement, written from the reference statements (not from the library's kernels):

    tree_cont_t::gen_trees_tt_within_radius (from :2240 on), gen_deterministic, add_new_tree   src/Tree.cpp:2209-2305, 2153-2155, 2157-2166
    adjust_tree_zval, get_tree_size_scale, TREE_SIZE                                           src/Tree.cpp:1465-1480, 20
    tile_t::get_z_minmax_for_area, mesh_dz, gen_decid_trees_if_needed, add_new_trees           src/tiled_mesh.cpp:548-564, 535, 1536-1547, 3805-3811
    tile_t::get_avg_veg                                                                        src/tiled_mesh.h:221
    can_have_decid_trees_in_zrange                                                             src/sm_tree.cpp:580-587
    get_xpos_round_down / get_ypos_round_down                                                  src/mesh.h:136-137
    get_pos_fract, extract_low_bits_01                                                         src/inlines.h:68-72

It is built on oracle primitives only: orc.gen_grid(force_sine=True, glaciate=0) (the six density fields of a tile), orc.eval_points(exact=1)
(interpolate_mesh_zval -> get_exact_zval), orc.eval_mesh_sin_terms (the veg corners, through tree_place_model.Scene) and orc.state().  The generator, its array
form, the Scene and the class from a height are tree_place_model's.  The slope test runs on NumPy arrays: the zvals and the stats a case hands to the library are
handed to the model as they are.

Types as in tree_place_model: np.float32 for float, Python float for double, Python int for int / unsigned / long with the wrap written out.  In
`num_trees/(NONUNIFORM_TREE_DEN ? sqrt(tree_density_thresh) : 1.0)` the ternary's operands are float and double, so its type is double: sqrt(float) is the float
overload, converted, and the int is divided by that double.  `0.5*DX_VAL*rgen.randd()`, `0.8*jitter*jitter`, `water_plane_z + 0.01*zmax_est`, `1.8*zmax_est`,
`size_est*(0.1*size_scale)`, `2.0*base_radius` and `0.5*radius` are double expressions stored to (or passed as) float; `TREE_SIZE*branch_size/tree_scale`,
`xoff2*DX_VAL`, `tree_slope_thresh*radius`, `100.0*den_val` inside extract_low_bits_01 (m is a float parameter) and `mzmax - pos.z` are float.
"""
import numpy as np

import tree_place_model as tpm
from tree_place_model import RandGen, f32, rand_arr, wrap32

NUM_TREE_TYPES = 5           # src/tree_leaf.h:8
TREE_SIZE = f32(0.005)       # src/Tree.cpp:20
TREE_CLASS_DECID = tpm.TREE_CLASS_DECID
PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("zval", np.float32), ("type", np.int32), ("tree_id", np.int32), ("rseed1", np.int32), ("rseed2", np.int32),
                        ("cx", np.uint16), ("cy", np.uint16)])
OUTCOMES = ("unselected", "veg", "range", "class", "coverage", "slope_dropped", "slope_kept", "type0", "type1", "type2", "type3", "type4")


class DecidParams:
    """num_trees, shared_tree_data.size(), tree_slope_thresh and tree_types[].branch_size, with the reference's defaults"""

    def __init__(self, num_trees=0, num_shared_trees=0, tree_slope_thresh=5.0, branch_size=(1.0, 1.0, 1.0, 1.0, 1.0)):
        self.num_trees, self.num_shared_trees, self.tree_slope_thresh = int(num_trees), int(num_shared_trees), f32(tree_slope_thresh)
        self.branch_size = [f32(b) for b in branch_size]


def new_tally():
    return {k: 0 for k in OUTCOMES}


def mesh_dz(stats):
    """tile_t::mesh_dz: max_eq(mesh_dz, szmax - szmin) over the 16 sub-blocks, from 0"""
    dz = f32(0.0)
    for k in range(16):
        dz = max(dz, f32(f32(stats.sub_zmax[k]) - f32(stats.sub_zmin[k])))
    return dz


def can_have_decid_trees_in_zrange(sc, z_min, z_max):
    if not (sc.tp.tree_mode & 1):  # are_trees_enabled()
        return False
    if f32(z_max) < sc.water_plane_z:
        return False
    relh1 = sc.get_rel_height(f32(z_min))
    return not f32(relh1 - sc.tp.tree_type_rand_zone) > f32(0.6)


def get_avg_veg(sc, tx, ty):
    p00, p01, p10, p11 = sc.veg_corners(tx, ty)  # params[0][0], [0][1], [1][0], [1][1]
    return f32(f32(0.25) * f32(f32(f32(p00 + p01) + p10) + p11))


def tree_radius(sc, dp, ttype):
    """adjust_tree_zval's radius for size = 0, create_bush = 0"""
    size_scale = f32(float(f32(f32(TREE_SIZE * dp.branch_size[ttype]) / sc.tp.tree_scale)) * 1.0)
    base_radius = f32(60 * (0.1 * float(size_scale)))
    return f32(2.0 * float(base_radius))


def get_z_minmax_for_area(sc, zvals, x1, y1, px, py, radius, zmin, zmax):
    st = sc.orc.state()
    S = sc.S
    zvsize = S + 2
    stride = zvsize - 1
    dxi, dyi = f32(st.DX_VAL_INV), f32(st.DY_VAL_INV)
    rx1, ry1, rx2, ry2 = f32(px - radius), f32(py - radius), f32(px + radius), f32(py + radius)
    rd_x = lambda v: int(f32(f32(v + sc.X_SCENE_SIZE) * dxi))  # noqa: E731  (int() truncates toward zero, as the cast does)
    rd_y = lambda v: int(f32(f32(v + sc.Y_SCENE_SIZE) * dyi))  # noqa: E731
    ix1, iy1 = max(0, rd_x(rx1) - x1), max(0, rd_y(ry1) - y1)
    ix2, iy2 = min(stride, (rd_x(rx2) - x1 + 1) % 2 ** 32), min(stride, (rd_y(ry2) - y1 + 1) % 2 ** 32)
    assert ix1 <= ix2 and iy1 <= iy2  # the reference's assert
    area = zvals[iy1:iy2 + 1, ix1:ix2 + 1]
    return min(zmin, f32(area.min())), max(zmax, f32(area.max()))


def gen_trees(sc, dp, tx, ty, xoff2=0, yoff2=0, zvals=None, stats=None, brush=None, tally=None):
    """gen_trees_tt_within_radius(x1, y1, x2, y2, center, radius, is_square, mesh_dz, cur_tile, vegetation_, use_density) from :2240 on for tile (tx, ty), x1 =
    tx*S - xoff2: brush None = gen_deterministic (vegetation*get_avg_veg(), use_density); else (pos, radius, is_square) as add_new_trees calls it (the defaults
    vegetation_ = 1, use_density = 0).  stats None: mesh_dz = 0 (no slope test).  -> list of records, in loop order"""
    tp, S, orc = sc.tp, sc.S, sc.orc
    tally = new_tally() if tally is None else tally
    mod_num_trees = int(dp.num_trees / float(np.sqrt(f32(tp.tree_density_thresh))))
    if mod_num_trees == 0 or not (tp.tree_mode & 1):
        return []
    min_tree_h, max_tree_h = f32(float(sc.water_plane_z) + 0.01 * float(sc.zmax_est)), f32(1.8 * float(sc.zmax_est))
    height_thresh = sc.get_median_height(tp.tree_density_thresh)
    smod = int(3.321 * sc.XY_MULT_SIZE + 1)
    tree_prob = max(1, sc.XY_MULT_SIZE // mod_num_trees)
    skip_val = max(1, int(1.0 / float(tp.tree_scale)))
    use_density = brush is None
    vegetation_ = f32(sc.vegetation * get_avg_veg(sc, tx, ty)) if brush is None else f32(1.0)
    dz = f32(0.0) if stats is None else mesh_dz(stats)
    gx1, gy1 = tx * S, ty * S  # x1 + xoff2, y1 + yoff2
    density_gen = [None] * (NUM_TREE_TYPES + 1)
    for i in range(0 if use_density else 1, NUM_TREE_TYPES + 1):
        tds = f32(float(tpm.TREE_DIST_SCALE) * (sc.XY_MULT_SIZE / 16384.0) * (1.0 if i == 0 else 0.1))
        xscale, yscale = f32(f32(tds * sc.DX_VAL) * sc.DX_VAL), f32(f32(tds * sc.DY_VAL) * sc.DY_VAL)
        density_gen[i] = orc.gen_grid(f32(gx1 + 1000 * i), f32(gy1 - 1500 * i), xscale, yscale, S, S, glaciate=0, force_sine=True)
    # the seeds and the selection for every visited cell at once (:2269-2275)
    cells = np.arange(0, S, skip_val, dtype=np.int64)
    gi, gj = np.meshgrid(gy1 + cells, gx1 + cells, indexing="ij")  # i + yoff2, j + xoff2
    rgi = tp.rand_gen_index
    s1 = wrap32(805306457 * gi + 12582917 * gj + 100663319 * rgi)
    s2 = wrap32(6291469 * gj + 3145739 * gi + 1572869 * rgi)
    s1, s2, _ = rand_arr(s1, s2)  # rand_mix
    s1, s2 = s2, s1
    s1, s2, v1 = rand_arr(s1, s2)  # rand_seed_mix
    s1, s2 = s2, s1
    s1, s2, v2 = rand_arr(s1, s2)
    val = (wrap32(v1 + v2) % 2 ** 32) % smod  # ((unsigned)rgen.rand_seed_mix()) % smod
    selected = (val > 100) & (val % tree_prob == 0)
    veg_ok = ~((s1 & 127) / 128.0 >= float(vegetation_))
    if brush is not None:
        px, py, radius = f32(brush[0][0]), f32(brush[0][1]), f32(brush[1])
    out = []
    for iy in range(len(cells)):
        cy = int(cells[iy])
        i = gy1 - yoff2 + cy  # the loop's local index
        yval = sc.get_yval(i)
        if brush is not None and radius > 0.0 and f32(abs(f32(yval - py))) > radius:
            continue
        for ix in range(len(cells)):
            cx = int(cells[ix])
            j = gx1 - xoff2 + cx
            if brush is not None and radius > 0.0:
                xval = sc.get_xval(j)
                if f32(abs(f32(xval - px))) > radius:
                    continue
                ddx, ddy = f32(px - xval), f32(py - yval)
                if not (f32(f32(ddx * ddx) + f32(ddy * ddy)) < f32(radius * radius)):  # dist_xy_less_than; is_square is not read
                    continue
            if not selected[iy, ix]:
                tally["unselected"] += 1
                continue
            if not veg_ok[iy, ix]:
                tally["veg"] += 1
                continue
            rgen = RandGen(int(s1[iy, ix]), int(s2[iy, ix]))
            posx = f32(float(sc.get_xval(j)) + 0.5 * float(sc.DX_VAL) * rgen.randd())
            posy = f32(float(yval) + 0.5 * float(sc.DY_VAL) * rgen.randd())
            zval = f32(orc.eval_points([[posx, posy]], True, xoff2=xoff2, yoff2=yoff2)[0])
            if zval > max_tree_h or zval < min_tree_h:
                tally["range"] += 1
                continue
            if tp.tree_mode == 3 and sc.get_tree_class_from_height(zval, 0) != TREE_CLASS_DECID:
                tally["class"] += 1
                continue
            if use_density and density_gen[0][cy, cx] > height_thresh:
                tally["coverage"] += 1
                continue
            ttype, max_val = -1, f32(0.0)
            for tt in range(NUM_TREE_TYPES):
                den_val = f32(density_gen[tt + 1][cy, cx])
                abs_v = f32(abs(f32(f32(100.0) * den_val)))
                jitter = f32(abs_v - f32(int(abs_v)))
                den_val = f32(float(den_val) + 0.8 * float(jitter) * float(jitter))
                if max_val == 0.0 or den_val > max_val:
                    max_val, ttype = den_val, tt
            posz = zval
            if dz < 0.0 or dz > 1.0:  # adjust_tree_zval(pos, 0, ttype, 0, cur_tile)
                radius_t = tree_radius(sc, dp, ttype)
                ax, ay = f32(posx + f32(f32(xoff2) * sc.DX_VAL)), f32(posy + f32(f32(yoff2) * sc.DY_VAL))
                posz, mzmax = get_z_minmax_for_area(sc, zvals, gx1, gy1, ax, ay, f32(0.5 * float(radius_t)), posz, posz)
                if not (f32(mzmax - posz) < f32(dp.tree_slope_thresh * radius_t)):
                    tally["slope_dropped"] += 1
                    continue
                tally["slope_kept"] += 1
            rec = np.zeros((), PLACE_DTYPE)
            rec["pos"], rec["zval"], rec["type"], rec["cx"], rec["cy"] = (posx, posy, posz), zval, ttype, cx, cy
            rec["tree_id"] = -1
            if dp.num_shared_trees:  # add_new_tree, ttype >= 0
                num_per_type = max(1, dp.num_shared_trees // NUM_TREE_TYPES)
                rec["tree_id"] = min((((rgen.rseed1 >> 7) + rgen.rseed2) % num_per_type + ttype * num_per_type) % 2 ** 32, dp.num_shared_trees - 1)
            rec["rseed1"], rec["rseed2"] = wrap32(rgen.rseed1), wrap32(rgen.rseed2)
            tally["type%d" % ttype] += 1
            out.append(rec)
    return out


def place(sc, dp, tiles, xoff2=0, yoff2=0, skip=None, stats=None, zvals=None, brush=None, tally=None):
    """the batch call: per tile the list of records.  skip[t]: can_have_trees() false; stats: the tiles' terra_tile_stats (or None), zvals [n, S+2, S+2]"""
    out = []
    for t, (tx, ty) in enumerate(tiles):
        if (skip is not None and skip[t]) or (stats is not None and not can_have_decid_trees_in_zrange(sc, stats[t].mzmin, stats[t].mzmax)):
            out.append([])
        else:
            out.append(gen_trees(sc, dp, tx, ty, xoff2, yoff2, None if zvals is None else zvals[t], None if stats is None else stats[t], brush, tally))
    return out
