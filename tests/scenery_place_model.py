"""NumPy / Python restatement of scenery placement, written from the reference statements (not from the library's kernels):

    scenery_group::gen, the cell loop                       src/scenery.cpp:1263-1353
    scenery_obj::gen_spos (use_xy = 1)                      src/scenery.cpp:94-99
    get_min_water_plane_z                                   src/scenery.cpp:62
    rock_shape3d::create (up to gen_rock)                   src/scenery.cpp:145-149
    surface_rock::create (up to the surface cache)          src/scenery.cpp:368-372
    s_rock::create                                          src/scenery.cpp:426-436
    voxel_rock::create (without gen_model_ix)               src/scenery.cpp:496-499
    wood_scenery_obj::calc_type, s_log::create, s_stump::create   src/scenery.cpp:547, 576-600, 642-658
    plant_base::create, s_plant::create, leafy_plant::create (up to gen_leaves)   src/scenery.cpp:697-709, 720-729, 943-959
    mushroom::create                                        src/scenery.cpp:1048-1055
    tile_t::update_scenery                                  src/tiled_mesh.cpp:1568-1578
    signed_rand_vector, signed_rand_vector_norm             src/gen_object.cpp:400-420
    pointT::operator/=, operator*(T), mag_sq, mag           src/3DWorld.h:268-272, 310, 324-325
    get_tree_type_from_height(zpos, rgen, for_scenery = 1)  src/sm_tree.cpp:555-566

It is built on oracle primitives only: orc.eval_points(exact=1) (interpolate_mesh_zval -> get_exact_zval), orc.eval_mesh_sin_terms (the veg corners, through
tree_place_model.Scene and decid_place_model.get_avg_veg) and orc.state().  The generator, its array form, the Scene and the class from a height are
tree_place_model's.

Types as in tree_place_model: np.float32 for float, Python float for double, Python int for int / unsigned / long with the wrap written out.  The literals are
double: `0.03/tree_scale`, `4.0*radius`, `0.9*radius`, `0.8*radius` are doubles (inside std::max / std::min too) and are narrowed to rand_uniform2's float
parameters; `0.02*rand_uniform2(..)/tree_scale`, `0.2*rand_uniform2(..)*rand_float2()/tree_scale`, `rand_uniform2(..)/tree_scale + 0.025`, `.. + 0.015`,
`pos.z -= 2.0*radius`, `radius *= 1.5`, `pos.z + (0.4/tree_scale + 0.025)` and the four minimum heights are double expressions stored to float;
`rand_uniform2(..)/tree_scale`, `rand_uniform2(..)*rand_float2()/tree_scale`, `size*(..)/3.0f`, `radius*rand_uniform2(..)`, `rand_uniform2(..)*radius` are float.
A float compared with a double literal (`relh < 0.46`, `> 0.62`) is compared as a double.  sqrt(float) is the float overload (<math.h> of libstdc++), so
`v*(1.0/sqrt(mag_sq))` multiplies by float(1.0/double(sqrtf(mag_sq))) -- operator*(T) narrows its argument -- and `dir /= -length` by float(1.0/double(-length)).
signed_rand_vector's `vector3d(scale*signed_rand_float(), .., ..)` has its three arguments evaluated right to left by g++: the first draw is z, the third x.  In
`rand_uniform2(a, b)*rand_float2()` the left operand draws first.
"""
import numpy as np

import decid_place_model as dpm
import tree_place_model as tpm
from tree_place_model import RandGen, cmod, f32, rand_arr, wrap32

KINDS = ("leafy_plant", "plant", "rock_shape", "surface_rock", "voxel_rock", "rock", "log", "stump", "mushroom")  # TERRA_SCENERY_*
LEAFY_PLANT, PLANT, ROCK_SHAPE, SURFACE_ROCK, VOXEL_ROCK, ROCK, LOG, STUMP, MUSHROOM = range(9)
LEAFY_PLANT_UW, LEAFY_PLANT_DIRT, LEAFY_PLANT_GRASS, LEAFY_PLANT_ROCK = 0, 1, 2, 3  # src/scenery.h:14
NUM_LAND_PLANT_TYPES, NUM_WATER_PLANT_TYPES = 6, 1                                   # src/scenery.h:13-16
TOLERANCE = f32(1.0E-12)                                                             # src/3DWorld.h:50
PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("radius", np.float32), ("kind", np.int32), ("iv", np.int32, (2,)), ("p", np.float32, (8,)),
                        ("rseed1", np.int32), ("rseed2", np.int32), ("cx", np.uint16), ("cy", np.uint16)])
DROPS = ("plant_too_high", "plant_between_water_tests", "log_below_minz", "log_no_type", "stump_too_low", "mushroom_too_low", "no_veg")
OTHER = ("unselected", "log_bad_z", "stump_no_type", "leafy_snow", "water_plant", "uw_leafy_plant", "palm_log", "pine_log", "max_selected")


def new_tally():
    t = {k: 0 for k in KINDS + DROPS + OTHER}
    return t


def signed_rand_vector_norm(rgen, scale=1.0):
    scale = f32(scale)
    while True:
        z = f32(scale * rgen.signed_rand_float())  # g++: the last argument first
        y = f32(scale * rgen.signed_rand_float())
        x = f32(scale * rgen.signed_rand_float())
        mag_sq = f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))
        if mag_sq > f32(scale * TOLERANCE):
            m = f32(1.0 / float(np.sqrt(mag_sq)))
            return [f32(x * m), f32(y * m), f32(z * m)]


class Ctx:
    """what the create functions read: the scene, tree_scale, the minimum heights, the cell's generator"""

    def __init__(self, sc, ocean_wave_height, use_voxel_rocks, xoff2, yoff2):
        self.sc, self.xoff2, self.yoff2 = sc, xoff2, yoff2
        self.ts = f32(sc.tp.tree_scale)
        wpz, zme = float(sc.water_plane_z), float(sc.zmax_est)
        self.min_stump_z, self.min_plant_z, self.min_log_z, self.min_mushroom_z = f32(wpz + 0.010 * zme), f32(wpz + 0.016 * zme), f32(wpz - 0.040 * zme), f32(wpz)
        self.min_water_plane_z = f32(sc.water_plane_z - f32(ocean_wave_height))  # get_water_z_height() - ocean_wave_height; water_plane_z is get_water_z_height()
        self.zmin = f32(sc.orc.state().zmin)
        self.voxel_rocks = use_voxel_rocks == 1 or (use_voxel_rocks >= 2 and sc.vegetation == 0.0)

    def zval(self, x, y):
        return f32(self.sc.orc.eval_points([[x, y]], True, xoff2=self.xoff2, yoff2=self.yoff2)[0])

    def gen_spos(self, rgen, j, i):
        sc = self.sc
        px = f32(float(sc.get_xval(j)) + 0.5 * float(sc.DX_VAL) * rgen.randd())
        py = f32(float(sc.get_yval(i)) + 0.5 * float(sc.DY_VAL) * rgen.randd())
        return [px, py, self.zval(px, py)]

    def calc_type(self, rgen, z):
        """(char)get_tree_type_from_height(pos.z, global_rand_gen, 1)"""
        sc = self.sc
        cls = sc.get_tree_class_from_height(z, sc.tp.tree_mode == 2)  # WMODE_INF_TERRAIN && (tree_mode == 2 || (!for_scenery && tree_mode == 3))
        if cls == tpm.TREE_CLASS_NONE:
            return tpm.TREE_NONE
        if cls == tpm.TREE_CLASS_PINE:
            return tpm.T_SH_PINE if cmod(rgen.rand(), 10) == 0 else tpm.T_PINE
        if cls == tpm.TREE_CLASS_PALM:
            return tpm.T_PALM
        return tpm.T_DECID + cmod(rgen.rand(), 3)


def _rec(kind, pos, radius, iv=(0, 0), p=()):
    rec = np.zeros((), PLACE_DTYPE)
    rec["pos"], rec["radius"], rec["kind"], rec["iv"] = pos, radius, kind, iv
    rec["p"] = list(p) + [0.0] * (8 - len(p))
    return rec


def plant_base_create(cx, rgen, j, i, tally):
    pos = cx.gen_spos(rgen, j, i)
    if pos[2] < cx.min_plant_z:
        if float(pos[2]) + (0.4 / float(cx.ts) + 0.025) > float(cx.min_water_plane_z):
            tally["plant_between_water_tests"] += 1
            return 0, pos
        return 2, pos
    if float(cx.sc.get_rel_height(pos[2])) > 0.62:
        tally["plant_too_high"] += 1
        return 0, pos
    return 1, pos


def leafy_plant_create(cx, rgen, j, i, tally):
    ret, pos = plant_base_create(cx, rgen, j, i, tally)
    if ret == 0:
        return None
    if ret == 2:
        ptype = LEAFY_PLANT_UW
        tally["uw_leafy_plant"] += 1
    else:
        relh = float(cx.sc.get_rel_height(pos[2]))
        if relh < 0.46:
            ptype = LEAFY_PLANT_DIRT
        elif relh < 0.60:
            ptype = LEAFY_PLANT_GRASS
        elif relh < 0.75:
            ptype = LEAFY_PLANT_ROCK
        else:
            tally["leafy_snow"] += 1
            return None
    radius = f32(rgen.rand_uniform(0.06, 0.12) / cx.ts)
    return _rec(LEAFY_PLANT, pos, radius, (ptype, 0))


def s_plant_create(cx, rgen, j, i, tally):
    ret, pos = plant_base_create(cx, rgen, j, i, tally)
    if ret == 0:
        return None
    if ret == 2:
        ptype = NUM_LAND_PLANT_TYPES + cmod(rgen.rand(), NUM_WATER_PLANT_TYPES)
        tally["water_plant"] += 1
    else:
        ptype = cmod(rgen.rand(), NUM_LAND_PLANT_TYPES)
    radius = f32(rgen.rand_uniform(0.0025, 0.0045) / cx.ts)
    height = f32(float(f32(rgen.rand_uniform(0.2, 0.4) / cx.ts)) + 0.025)
    return _rec(PLANT, pos, radius, (ptype, 0), [height])


def rock_shape_create(cx, rgen, j, i):
    rs_rock = rgen.rand()
    pos = cx.gen_spos(rgen, j, i)
    return _rec(ROCK_SHAPE, pos, 0.0, (rs_rock, rgen.rand() & 1))


def surface_rock_create(cx, rgen, j, i):
    pos = cx.gen_spos(rgen, j, i)
    u = rgen.rand_uniform(0.1, 0.2)
    radius = f32(f32(u * rgen.rand_float()) / cx.ts)
    return _rec(SURFACE_ROCK, pos, radius, p=signed_rand_vector_norm(rgen))


def voxel_rock_create(cx, rgen, j, i):
    pos = cx.gen_spos(rgen, j, i)
    u = 0.2 * float(rgen.rand_uniform(0.5, 1.0))
    radius = f32(u * float(rgen.rand_float()) / float(cx.ts))
    return _rec(VOXEL_ROCK, pos, radius, (rgen.rand(), 0))


def s_rock_create(cx, rgen, j, i):
    scale = [rgen.rand_uniform(0.8, 1.3) for _ in range(3)]
    pos = cx.gen_spos(rgen, j, i)
    size = f32(0.02 * float(rgen.rand_uniform(0.2, 0.8)) / float(cx.ts))
    if (rgen.rand() & 3) == 0:
        size = f32(size * rgen.rand_uniform(1.2, 8.0))
    dirv = signed_rand_vector_norm(rgen)
    angle = rgen.rand_uniform(0.0, 360.0)
    radius = f32(f32(size * f32(f32(scale[0] + scale[1]) + scale[2])) / f32(3.0))
    pos[2] = f32(pos[2] + f32(radius * rgen.rand_uniform(-0.1, 0.25)))
    return _rec(ROCK, pos, radius, p=scale + [size] + dirv + [angle])


def s_log_create(cx, rgen, j, i, tally):
    pos = cx.gen_spos(rgen, j, i)
    ts = float(cx.ts)
    radius = f32(rgen.rand_uniform(0.003, 0.008) / cx.ts)
    radius2 = rgen.rand_uniform(f32(0.9 * float(radius)), f32(1.1 * float(radius)))
    length = rgen.rand_uniform(f32(max(0.03 / ts, 4.0 * float(radius))), f32(min(0.15 / ts, 20.0 * float(radius))))
    dirv = signed_rand_vector_norm(rgen)
    dirv[0], dirv[1] = f32(dirv[0] * length), f32(dirv[1] * length)
    pt2 = [f32(pos[0] + dirv[0]), f32(pos[1] + dirv[1]), None]
    pos[2] = f32(cx.zval(pos[0], pos[1]) + f32(rgen.rand_uniform(0.7, 0.99) * radius))
    pt2[2] = f32(cx.zval(pt2[0], pt2[1]) + f32(rgen.rand_uniform(0.7, 0.99) * radius2))
    if max(pos[2], pt2[2]) < cx.min_log_z:
        tally["log_below_minz"] += 1
        return None
    if pos[2] <= cx.zmin or pt2[2] <= cx.zmin:
        tally["log_bad_z"] += 1
        return None
    dirv[2] = f32(pt2[2] - pos[2])
    length = f32(np.sqrt(f32(f32(f32(dirv[0] * dirv[0]) + f32(dirv[1] * dirv[1])) + f32(dirv[2] * dirv[2]))))  # dir.mag()
    m = f32(1.0 / float(f32(-length)))  # dir /= -length
    dirv = [f32(d * m) for d in dirv]
    ttype = cx.calc_type(rgen, pos[2])
    if ttype < 0:
        tally["log_no_type"] += 1
        return None
    if ttype == tpm.T_PALM:
        tally["palm_log"] += 1
    elif ttype in (tpm.T_PINE, tpm.T_SH_PINE):
        tally["pine_log"] += 1
    return _rec(LOG, pos, radius, (ttype, 0), [radius2, length] + dirv + pt2)


def s_stump_create(cx, rgen, j, i, tally):
    pos = cx.gen_spos(rgen, j, i)
    if pos[2] < cx.min_stump_z:
        tally["stump_too_low"] += 1
        return None
    ts = float(cx.ts)
    radius = f32(rgen.rand_uniform(0.005, 0.01) / cx.ts)
    radius2 = rgen.rand_uniform(f32(0.8 * float(radius)), radius)
    pos[2] = f32(float(pos[2]) - 2.0 * float(radius))
    height = f32(float(rgen.rand_uniform(f32(0.01 / ts), f32(min(0.05 / ts, 4.0 * float(radius))))) + 0.015)
    if (rgen.rand() & 3) == 0:
        height = f32(height * rgen.rand_uniform(1.0, 5.0))
        radius = f32(float(radius) * 1.5)
        radius2 = f32(float(radius2) * 1.3)
    ttype = cx.calc_type(rgen, pos[2])
    if ttype < 0:
        tally["stump_no_type"] += 1
        return None
    return _rec(STUMP, pos, radius, (ttype, 0), [radius2, height])


def mushroom_create(cx, rgen, j, i, tally):
    pos = cx.gen_spos(rgen, j, i)
    if pos[2] < cx.min_mushroom_z:
        tally["mushroom_too_low"] += 1
        return None
    radius = f32(rgen.rand_uniform(0.005, 0.01) / cx.ts)
    pos[2] = f32(pos[2] - radius)
    height = f32(rgen.rand_uniform(4.0, 5.0) * radius)
    return _rec(MUSHROOM, pos, radius, p=[height])


def selection(sc, tx, ty, smod):
    """:1276-1281 for every cell of the tile at once -> (val, rseed1, rseed2 after rand2_mix), int64 arrays [rows, cols]"""
    S = sc.S
    cells = np.arange(S, dtype=np.int64)
    gi, gj = np.meshgrid(ty * S + cells, tx * S + cells, indexing="ij")  # i + yoff2, j + xoff2
    rgi = sc.tp.rand_gen_index
    s1 = wrap32(786433 * gi + 196613 * rgi)
    s2 = wrap32(6291469 * gj + 1572869 * rgi)
    s1, s2, v1 = rand_arr(s1, s2)  # rand2_seed_mix
    s1, s2 = s2, s1
    s1, s2, v2 = rand_arr(s1, s2)
    val = (wrap32(v1 + v2) % 2 ** 32) % smod  # int % unsigned: the int converts to unsigned
    s1, s2, _ = rand_arr(s1, s2)  # rand2_mix
    s1, s2 = s2, s1
    return val, s1, s2


def gen(sc, tx, ty, xoff2=0, yoff2=0, use_voxel_rocks=2, ocean_wave_height=0.0, tally=None):
    """scenery_group::gen(x1, y1, x2, y2, vegetation*get_avg_veg(), ..)'s cell loop for tile (tx, ty), x1 = tx*S - xoff2 -> list of records, in loop order"""
    tally = new_tally() if tally is None else tally
    S, tp = sc.S, sc.tp
    smod = max(200, int(f32(f32(f32(3.321) * f32(sc.XY_MULT_SIZE)) / f32(tp.tree_scale + f32(1.0)))))
    vegetation_ = f32(sc.vegetation * dpm.get_avg_veg(sc, tx, ty))
    cx = Ctx(sc, ocean_wave_height, use_voxel_rocks, xoff2, yoff2)
    val_a, s1, s2 = selection(sc, tx, ty, smod)
    veg_a = (s1 & 127) / 128.0 < float(vegetation_)
    sel = val_a < 150
    tally["unselected"] += int((~sel).sum())
    nlive = 0
    out = []
    for iy, ix in np.argwhere(sel):  # rows, then columns
        iy, ix = int(iy), int(ix)
        i, j = ty * S - yoff2 + iy, tx * S - xoff2 + ix  # the loop's local indices
        val, veg = int(val_a[iy, ix]), bool(veg_a[iy, ix])
        rgen = RandGen(int(s1[iy, ix]), int(s2[iy, ix]))
        rec, add_mushroom = None, False
        if not veg and val >= 50:
            tally["no_veg"] += 1
        else:
            nlive += 1
        if val >= 100:
            if veg:
                rec = leafy_plant_create(cx, rgen, j, i, tally)
        elif veg and cmod(rgen.rand(), 100) < 35:
            rec = s_plant_create(cx, rgen, j, i, tally)
        elif val < 5:
            rec = rock_shape_create(cx, rgen, j, i)
        elif val < 15:
            rec = surface_rock_create(cx, rgen, j, i)
        elif cx.voxel_rocks and val < 35:
            rec = voxel_rock_create(cx, rgen, j, i)
        elif val < 50:
            if veg and val < 25:
                add_mushroom = True
            else:
                rec = s_rock_create(cx, rgen, j, i)
        elif veg and val < 85:
            if veg and val < 60:
                add_mushroom = True
            else:
                rec = s_log_create(cx, rgen, j, i, tally)
        elif veg:
            rec = s_stump_create(cx, rgen, j, i, tally)
        if add_mushroom:
            rec = mushroom_create(cx, rgen, j, i, tally)
        if rec is None:
            continue
        rec["rseed1"], rec["rseed2"], rec["cx"], rec["cy"] = wrap32(rgen.rseed1), wrap32(rgen.rseed2), ix, iy
        tally[KINDS[int(rec["kind"])]] += 1
        out.append(rec)
    tally["max_selected"] = max(tally["max_selected"], nlive)  # cells some branch can create an object from: what the kernel's ring holds
    return out


def place(sc, tiles, xoff2=0, yoff2=0, skip=None, use_voxel_rocks=2, ocean_wave_height=0.0, tally=None):
    """the batch call: per tile the list of records.  skip[t]: update_scenery does not generate"""
    return [[] if (skip is not None and skip[t]) else gen(sc, tx, ty, xoff2, yoff2, use_voxel_rocks, ocean_wave_height, tally) for t, (tx, ty) in enumerate(tiles)]


def kind_counts(want):
    return np.array([[sum(int(r["kind"]) == k for r in w) for k in range(len(KINDS))] for w in want], np.uint32).reshape(len(want), len(KINDS))
