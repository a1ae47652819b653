"""NumPy / Python float32 restatement of the grass draw lists of a tile for a camera, written from the reference statements (not from the library's kernel):

    tile_t::draw_grass (without the GL calls)                                src/tiled_mesh.cpp:1607-1664
    tile_draw_t::draw_grass' per-tile filters                                src/tiled_mesh.cpp:3420-3425
    tile_t::get_min_dist_to_pt (mesh_only)                                   src/tiled_mesh.cpp:354-364
    get_mesh_bcube, get_center, get_norm_not_normalized, get_grass_block_dim src/tiled_mesh.h:229-241, 281-283, 315
    get_rel_dist_to_camera, get_dist_to_camera_in_tiles                      src/tiled_mesh.h:320-332
    the thresholds                                                           src/tiled_mesh.cpp:27-29, 118-120; src/tiled_mesh.h:24, 93-94
    NUM_GRASS_LODS, GRASS_BLOCK_SZ                                           src/grass.h:9-10
    pos_dir_up: constructor, orthogonalize_up_dir, point_visible_test,
      check_clip_plane, pt_set_visible<8>, cube_visible,
      cube_completely_visible                                                src/visibility.cpp:67-103, 141-174, 186-196
    cube_t::closest_pt, closest_pt_dist_sq, dist_less_than, p2p_dist_sq      src/3DWorld.h:591, 636-641; src/csg.cpp:244-246; src/inlines.h:176-192
    orthogonalize_dir, cross_product, dot_product, pointT::normalize         src/inlines.h:153-157, 220-222, 265-268; src/3DWorld.h:273-279

Types: np.float32 for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are double: 0.56*bg_thresh_sq and the comparison
with it; 2.0*grass_length (narrowed by point's constructor); 0.5*tt_grass_scale_factor and the comparison with it; A*tterm (A is a double member; narrowed by
atanf's parameter); 1.0/d in normalize (narrowed to the float m).  Everything else is float: dot products are x*x + y*y + z*z left to right, SQRT2 is the float
sqrt(2.0), `unsigned*float` products convert the unsigned to float first.  tanf / sinf / atanf are the C library's, called through ctypes.

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
NUM_GRASS_LODS, GRASS_BLOCK_SZ, TILE_RADIUS = 6, 4, 6
GRASS_LOD_SCALE, GRASS_DIST_SLOPE, GRASS_THRESH = f32(15.0), f32(0.25), f32(1.6)
BCUBE_ZTOLER = f32(1.0E-6)
SQRT2 = f32(math.sqrt(2.0))
PI = f32(3.141592654)
TOLERANCE = f32(1.0E-12)
NO_PASS = 255
ZERO = f32(0.0)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("tanf", "sinf", "atanf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]

TALLY = ("tiles_skipped", "tiles_too_far", "tiles_no_grass", "tiles_all_visible", "tiles_frustum_tested", "too_far_tile_blocks_in_range", "empty", "beyond", "frustum_dropped",
         "frustum_kept", "far_dropped", "all_visible_kept", "backface_dropped", "backface_kept", "not_tested", "bad_ix", "kept", "lod_clamped", "wpass0", "wpass1",
         "beyond_capacity", "max_group", "max_lods_in_tile")


def new_tally():
    return {k: 0 for k in TALLY}


def cmax(a, b):  # std::max
    return b if a < b else a


def cmin(a, b):  # std::min
    return a if not (b < a) else b


def dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def cross(a, b):
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def sub(a, b):
    return [f32(a[0] - b[0]), f32(a[1] - b[1]), f32(a[2] - b[2])]


def mag_sq(a):
    return dot(a, a)


def f2u(v):
    """unsigned(float) as x86-64 converts it: cvttss2si to 64 bits, the low word"""
    v = float(v)
    if not (-9.2e18 < v < 9.2e18):
        return 0
    return int(v) & 0xFFFFFFFF


class View:
    """pos_dir_up: pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid"""

    def __init__(self, pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid=1):
        self.pos, self.dir, self.upv_, self.cp = [f32(v) for v in pos], [f32(v) for v in dir], [f32(v) for v in upv_], [f32(v) for v in cp]
        self.sterm, self.x_sterm, self.near_, self.far_, self.valid = f32(sterm), f32(x_sterm), f32(near_), f32(far_), int(valid)

    def words(self):
        return np.array(self.pos + self.dir + self.upv_ + self.cp + [self.sterm, self.x_sterm, self.near_, self.far_], f32).tobytes() + np.int32(self.valid).tobytes()


def make_view(pos, dir, up, angle, aspect, near, far):
    """the constructor (:67-85) and orthogonalize_up_dir (:87-92); None where it asserts"""
    pos, dir, up = [f32(v) for v in pos], [f32(v) for v in dir], [f32(v) for v in up]
    angle, near, far = f32(angle), f32(near), f32(far)
    if not (near >= 0.0 and far > 0.0 and far > near):
        return None
    if dir[0] == 0.0 and dir[1] == 0.0 and dir[2] == 0.0:
        return None
    A = float(f32(aspect))
    tterm, sterm = f32(_libm.tanf(angle)), f32(_libm.sinf(angle))
    if A == 1.0:
        x_sterm = sterm
    else:
        if not (tterm > 0.0):
            return None
        atan_val = f32(_libm.atanf(f32(A * float(tterm))))
        if atan_val < 0.0:
            atan_val = f32(atan_val + PI)
        x_sterm = f32(f32(atan_val / angle) * sterm)
    upv_ = cross(dir, cross(up, dir))  # orthogonalize_dir(upv, dir, upv_, 1)
    d = f32(np.sqrt(mag_sq(upv_)))
    if d >= TOLERANCE:
        m = f32(1.0 / float(d))
        upv_ = [f32(v * m) for v in upv_]
    return View(pos, dir, upv_, cross(dir, upv_), sterm, x_sterm, near, far, 1)


class Params:
    def __init__(self, tt=1.0, grass_length=0.02, nrnd=16):
        self.tt, self.grass_length, self.nrnd = f32(tt), f32(grass_length), int(nrnd)


class Scene:
    """the globals the pass reads: the oracle's state after orc.init(cfg), the config, the settings, the offsets"""

    def __init__(self, orc, cfg, params, dxoff=0, dyoff=0):
        st = orc.state()
        self.p = params
        self.S = int(cfg.mesh_x)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y)
        self.DX_VAL, self.DY_VAL = f32(st.DX_VAL), f32(st.DY_VAL)
        self.dxdy = f32(self.DX_VAL * self.DY_VAL)
        self.dxoff, self.dyoff = dxoff, dyoff
        self.dim = 1 + (self.S - 1) // GRASS_BLOCK_SZ
        self.tile_width = f32(self.X_SCENE_SIZE + self.Y_SCENE_SIZE)
        self.scaled_tile_radius = f32(f32(TILE_RADIUS) * self.tile_width)
        tt = params.tt
        self.grass_thresh = f32(f32(f32(GRASS_THRESH * tt) * self.tile_width) + f32(tt / GRASS_DIST_SLOPE))  # get_grass_thresh_pad()
        self.dx_step, self.dy_step = f32(f32(GRASS_BLOCK_SZ) * self.DX_VAL), f32(f32(GRASS_BLOCK_SZ) * self.DY_VAL)
        self.lod_scale = f32(GRASS_LOD_SCALE / f32(tt * self.scaled_tile_radius))

    def get_xval(self, x):
        return f32(-self.X_SCENE_SIZE + f32(self.DX_VAL * f32(x)))

    def get_yval(self, y):
        return f32(-self.Y_SCENE_SIZE + f32(self.DY_VAL * f32(y)))


def cube_pts(d):
    return [[d[0][i], d[1][j], d[2][k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]


def point_visible_test(v, p):
    if not v.valid:
        return True
    pv = sub(p, v.pos)
    if dot(v.dir, pv) < 0.0:
        return False
    dist = f32(np.sqrt(mag_sq(pv)))
    if abs(dot(v.upv_, pv)) > f32(dist * v.sterm):
        return False
    if abs(dot(v.cp, pv)) > f32(dist * v.x_sterm):
        return False
    return bool(dist > v.near_ and dist < v.far_)


def cube_completely_visible(v, d):
    if not v.valid:
        return True
    return all(point_visible_test(v, p) for p in cube_pts(d))


def check_clip_plane(pts, pos, n, aa, d):
    for p in pts:
        pv = sub(p, pos)
        dp = dot(n, pv)
        if (f32(-dp) if d else dp) <= 0.0 or f32(dp * dp) <= f32(aa * mag_sq(pv)):
            return True
    return False


def pt_set_visible(v, pts):
    su, sc = f32(v.sterm * v.sterm), f32(v.x_sterm * v.x_sterm)
    if not check_clip_plane(pts, v.pos, v.upv_, su, 0) or not check_clip_plane(pts, v.pos, v.upv_, su, 1):
        return False
    if not check_clip_plane(pts, v.pos, v.cp, sc, 0) or not check_clip_plane(pts, v.pos, v.cp, sc, 1):
        return False
    npass = fpass = False
    for p in pts:
        if npass and fpass:
            break
        dp = dot(v.dir, sub(p, v.pos))
        npass |= bool(dp > v.near_)
        fpass |= bool(dp < v.far_)
    return npass and fpass


def closest_pt(d, p):
    return [cmin(d[i][1], cmax(d[i][0], p[i])) for i in range(3)]


def p2p_dist_sq(a, b):
    return mag_sq(sub(a, b))


def cube_visible(v, d, tally=None):
    if not v.valid:
        return True
    if not pt_set_visible(v, cube_pts(d)):
        return False
    ok = bool(p2p_dist_sq(v.pos, closest_pt(d, v.pos)) < f32(v.far_ * v.far_))  # dist_less_than(pos, c.closest_pt(pos), far_)
    if tally is not None and not ok:
        tally["far_dropped"] += 1
    return ok


def mesh_bcube(sc, tx, ty, mzmin, mzmax):
    x1, y1 = tx * sc.S, ty * sc.S
    xv1, yv1 = sc.get_xval(x1 + sc.dxoff), sc.get_yval(y1 + sc.dyoff)
    return [[xv1, f32(xv1 + f32(f32(sc.S) * sc.DX_VAL))], [yv1, f32(yv1 + f32(f32(sc.S) * sc.DY_VAL))], [f32(f32(mzmin) - BCUBE_ZTOLER), f32(f32(mzmax) + BCUBE_ZTOLER)]]


def get_min_dist_to_pt(d, pt):
    dsq = ZERO
    for i in range(3):
        dist = cmax(ZERO, cmax(f32(d[i][0] - pt[i]), f32(pt[i] - d[i][1])))
        dsq = f32(dsq + f32(dist * dist))
    return f32(np.sqrt(dsq))


def dist_to_camera_in_tiles(sc, v, tx, ty, mzmin, mzmax, radius):
    x1, y1 = tx * sc.S, ty * sc.S
    center = [sc.get_xval(((x1 + x1 + sc.S) >> 1) + sc.dxoff), sc.get_yval(((y1 + y1 + sc.S) >> 1) + sc.dyoff), f32(f32(0.5) * f32(f32(mzmin) + f32(mzmax)))]
    dist = f32(np.sqrt(p2p_dist_sq(v.pos, center)))
    return f32(f32(cmax(ZERO, f32(dist - f32(radius))) / sc.scaled_tile_radius) * f32(TILE_RADIUS))


def back_facing(sc, v, llcx, llcy, adj_z, x, y, zt):
    """:1636-1643 over the block's 25 texels at once: elementwise float32, the dot product's sum in the reference's order"""
    x0, y0 = x * GRASS_BLOCK_SZ, y * GRASS_BLOCK_SZ
    z = zt[y0:y0 + 6, x0:x0 + 6]
    zc = z[:5, :5]
    nx, ny, nz = sc.DY_VAL * (zc - z[:5, 1:6]), sc.DX_VAL * (zc - z[1:6, :5]), sc.dxdy
    xs = (llcx + np.arange(x0, x0 + 5).astype(f32) * sc.DX_VAL).astype(f32)
    ys = (llcy + np.arange(y0, y0 + 5).astype(f32) * sc.DY_VAL).astype(f32)
    vx, vy, vz = (v.pos[0] - xs)[None, :], (v.pos[1] - ys)[:, None], adj_z - zc
    dp = (nx * vx + ny * vy) + nz * vz
    assert dp.dtype == np.float32
    return bool((dp < 0.0).all())


def draw_grass(sc, v, tx, ty, zt, stats, blocks, skip, tally):
    """one tile -> (list of (x, y, lod, bix) in draw order, group_counts [6][nrnd], pass byte)"""
    nrnd, dim = sc.p.nrnd, sc.dim
    gc = np.zeros((NUM_GRASS_LODS, nrnd), np.uint32)
    mzmin, mzmax, radius = f32(stats.mzmin), f32(stats.mzmax), f32(stats.radius)
    d = mesh_bcube(sc, tx, ty, mzmin, mzmax)
    camera = v.pos
    has_grass = bool((blocks["ix"] != 0).any())
    too_far = bool(get_min_dist_to_pt(d, camera) > sc.grass_thresh)
    llcx, llcy = d[0][0], d[1][0]
    block_grass_thresh = f32(sc.grass_thresh + f32(f32(SQRT2 * radius) / f32(dim)))
    bg_thresh_sq = f32(block_grass_thresh * block_grass_thresh)

    def bcube_of(x, y, gb):
        bcx1, bcy1 = f32(llcx + f32(f32(x) * sc.dx_step)), f32(llcy + f32(f32(y) * sc.dy_step))
        return [[bcx1, f32(bcx1 + sc.dx_step)], [bcy1, f32(bcy1 + sc.dy_step)], [f32(gb["zmin"]), f32(f32(gb["zmax"]) + sc.p.grass_length)]]

    if skip:
        tally["tiles_skipped"] += 1
        return [], gc, NO_PASS
    if not has_grass:
        tally["tiles_no_grass"] += 1
        return [], gc, NO_PASS
    if too_far:
        tally["tiles_too_far"] += 1
        for y in range(dim):  # (tally only) blocks that the block threshold alone would have let through: the tile-level return of :1612 decides
            for x in range(dim):
                gb = blocks[y, x]
                if gb["ix"] != 0 and not p2p_dist_sq(closest_pt(bcube_of(x, y, gb), camera), camera) > bg_thresh_sq:
                    tally["too_far_tile_blocks_in_range"] += 1
        return [], gc, NO_PASS
    wpass = int(float(dist_to_camera_in_tiles(sc, v, tx, ty, mzmin, mzmax, radius)) > 0.5 * float(sc.p.tt))
    tally["wpass1" if wpass else "wpass0"] += 1
    adj_z = f32(camera[2] + f32(2.0 * float(sc.p.grass_length)))
    all_visible = cube_completely_visible(v, d)
    tally["tiles_all_visible" if all_visible else "tiles_frustum_tested"] += 1
    insts = [[[] for _ in range(nrnd)] for _ in range(NUM_GRASS_LODS)]
    lods = set()
    for y in range(dim):
        for x in range(dim):
            gb = blocks[y, x]
            if gb["ix"] == 0:
                tally["empty"] += 1
                continue
            bcube = bcube_of(x, y, gb)
            dist_sq = p2p_dist_sq(closest_pt(bcube, camera), camera)
            if dist_sq > bg_thresh_sq:
                tally["beyond"] += 1
                continue
            if not all_visible:
                if not cube_visible(v, bcube, tally):
                    tally["frustum_dropped"] += 1
                    continue
                tally["frustum_kept"] += 1
            else:
                tally["all_visible_kept"] += 1
            if float(dist_sq) < 0.56 * float(bg_thresh_sq):
                if back_facing(sc, v, llcx, llcy, adj_z, x, y, zt):
                    tally["backface_dropped"] += 1
                    continue
                tally["backface_kept"] += 1
            else:
                tally["not_tested"] += 1
            raw = f2u(f32(sc.lod_scale * f32(np.sqrt(dist_sq))))
            lod_level = min(NUM_GRASS_LODS - 1, raw)
            bix = int(gb["ix"]) - 1
            if bix >= nrnd:  # the reference asserts: skipped
                tally["bad_ix"] += 1
                continue
            if raw > NUM_GRASS_LODS - 1:
                tally["lod_clamped"] += 1
            tally["kept"] += 1
            lods.add(lod_level)
            insts[lod_level][bix].append((x, y))
    out = []
    for lod in range(NUM_GRASS_LODS):
        for bix in range(nrnd):
            gc[lod, bix] = len(insts[lod][bix])
            tally["max_group"] = max(tally["max_group"], len(insts[lod][bix]))
            out += [(x, y, lod, bix) for (x, y) in insts[lod][bix]]
    tally["max_lods_in_tile"] = max(tally["max_lods_in_tile"], len(lods))
    return out, gc, wpass


def view_batch(sc, v, tiles, zvals, stats, blocks, skip=None, tally=None):
    """-> (per-tile lists, group_counts [n, 6, nrnd], pass [n])"""
    tally = new_tally() if tally is None else tally
    lists, gcs, ps = [], [], []
    for t, (tx, ty) in enumerate(tiles):
        lst, gc, p = draw_grass(sc, v, tx, ty, zvals[t], stats[t], blocks[t], bool(skip[t]) if skip is not None else False, tally)
        lists.append(lst); gcs.append(gc); ps.append(p)
    return lists, np.array(gcs, np.uint32).reshape(len(tiles), NUM_GRASS_LODS, sc.p.nrnd), np.array(ps, np.uint8)


def aux_word(sc, x, y, lod, bix):
    return (y * sc.dim + x) | (lod << 16) | (bix << 19)


def pack(sc, lists, capacity):
    """the model's lists as the library's arrays: (insts [n, capacity, 2], aux [n, capacity], counts [n]); what does not fit is dropped, counts keep all"""
    n = len(lists)
    insts, aux, counts = np.zeros((n, capacity, 2), f32), np.zeros((n, capacity), np.uint32), np.zeros(n, np.uint32)
    for t, lst in enumerate(lists):
        counts[t] = len(lst)
        for k, (x, y, lod, bix) in enumerate(lst[:capacity]):
            insts[t, k] = (f32(f32(x) * sc.dx_step), f32(f32(y) * sc.dy_step))
            aux[t, k] = aux_word(sc, x, y, lod, bix)
    return insts, aux, counts
