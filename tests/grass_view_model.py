"""NumPy / Python float32 restatement of the grass draw lists of a tile for a camera, written from the reference statements (not from the library's kernel):

    tile_t::draw_grass (without the GL calls)                                src/tiled_mesh.cpp:1607-1664
    tile_draw_t::draw_grass' per-tile filters                                src/tiled_mesh.cpp:3420-3425
    tile_t::get_min_dist_to_pt (mesh_only)                                   src/tiled_mesh.cpp:354-364
    get_mesh_bcube, get_center, get_norm_not_normalized, get_grass_block_dim src/tiled_mesh.h:229-241, 281-283, 315
    get_rel_dist_to_camera, get_dist_to_camera_in_tiles                      src/tiled_mesh.h:320-332
    the thresholds                                                           src/tiled_mesh.cpp:27-29, 118-120; src/tiled_mesh.h:24, 93-94
    NUM_GRASS_LODS, GRASS_BLOCK_SZ                                           src/grass.h:9-10

The view (pos_dir_up's constructor and its point and cube tests), closest_pt, unsigned(float) and the vector helpers are tests/view_model.py's.  Types: np.float32
for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are double: 0.56*bg_thresh_sq and the comparison with it;
2.0*grass_length (narrowed by point's constructor); 0.5*tt_grass_scale_factor and the comparison with it.  Everything else is float: SQRT2 is the float
sqrt(2.0), `unsigned*float` products convert the unsigned to float first.

The tally counts what each test decided, so that a case can show that it exercises what it is named for."""
import math

import numpy as np

from view_model import closest_pt, cmax, cube_completely_visible, cube_visible, f2u, p2p_dist_sq

f32 = np.float32
NUM_GRASS_LODS, GRASS_BLOCK_SZ, TILE_RADIUS = 6, 4, 6
GRASS_LOD_SCALE, GRASS_DIST_SLOPE, GRASS_THRESH = f32(15.0), f32(0.25), f32(1.6)
BCUBE_ZTOLER = f32(1.0E-6)
SQRT2 = f32(math.sqrt(2.0))
NO_PASS = 255
ZERO = f32(0.0)

TALLY = ("tiles_skipped", "tiles_too_far", "tiles_no_grass", "tiles_all_visible", "tiles_frustum_tested", "too_far_tile_blocks_in_range", "empty", "beyond", "frustum_dropped",
         "frustum_kept", "far_dropped", "all_visible_kept", "backface_dropped", "backface_kept", "not_tested", "bad_ix", "kept", "lod_clamped", "wpass0", "wpass1",
         "beyond_capacity", "max_group", "max_lods_in_tile")


def new_tally():
    return {k: 0 for k in TALLY}


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
