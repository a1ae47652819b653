"""NumPy / float32 restatement of the grass brush, written from the reference statements (not from the library's kernels):

    tile_t::add_or_remove_grass_at   src/tiled_mesh.cpp:3845-3948
    tile_t::add_grass_block_at       src/tiled_mesh.cpp:1354-1371
    tile_t::mesh_sphere_intersect    src/tiled_mesh.cpp:3796-3799, get_center / get_mesh_bcube src/tiled_mesh.h:229-241, sphere_cube_intersect src/Math3d.cpp:920-935
    adjust_brush_weight              src/heightmap.cpp:27-33
    get_tids / update_lttex_ix       src/Textures.cpp:1289-1313, h_dirt from init_terrain_mesh (src/mesh_gen.cpp:407-431) + gen_tex_height_tables (src/Textures.cpp:1757-1761)

Every float expression is evaluated in float32 in the reference's order (x86-64 SSE2, no fused multiply-add); where the C++ promotes to double the model uses a
Python float.  The oracle supplies the primitives it exports: the SINF / COSF table (orc.sin_table), the biome parameters (orc.tile_terrain_params) and the scene
state (orc.state).  powf is the C library's own, as in the reference.
This reading is confirmed against the compiler's output: tests/test_tile_members_ref.py compares the model, weights, blocks, return value and the arguments of the
two flower calls, with the compiled tile_t::add_or_remove_grass_at (oracle/ref_shim.cpp section 4).
"""
import ctypes as C

import numpy as np

import orclib

f32 = np.float32
SAND, DIRT, GRASS, ROCK, SNOW = range(5)  # get_texture_ixs (src/tiled_mesh.cpp:1049-1062) over mesh_tids_dirt (src/mesh_gen.cpp:42)
BSHAPE_CONST_SQ, BSHAPE_CNST_CIR, BSHAPE_LINEAR, BSHAPE_QUADRATIC, BSHAPE_COSINE, BSHAPE_SINE, BSHAPE_FLAT_SQ, BSHAPE_FLAT_CIR = range(8)  # src/heightmap.h:11
PI = f32(3.141592654)         # src/3DWorld.h:43
TSIZE = 1 << 15               # src/sinf.h:8
TEXTURE_SMOOTH = f32(0.01)    # src/Textures.cpp:12
BCUBE_ZTOLER = f32(1.0E-6)    # src/tiled_mesh.h:32
SIZE, TSIZE_TEX, ZVSIZE, GRASS_BLOCK_SZ, GRASS_BLOCK_DIM = 128, 129, 130, 4, 32

_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def uchar(v):
    """(unsigned char)<float or double>: x86 truncation to int (cvttss2si / cvttsd2si: INT_MIN when out of range), low byte"""
    v = float(v)
    if not (-2147483648.0 <= v < 2147483648.0):
        return 0
    return int(v) & 0xFF


def fmin(a, b):  # std::min
    return b if b < a else a


def fmax(a, b):  # std::max
    return b if a < b else a


class Scene:
    """the globals the brush reads, taken from the oracle after orc.init(cfg) (+ orc.set_landscape(ls))"""

    def __init__(self, orc, cfg, ls=None):
        st = orc.state()
        ls = ls or orclib.make_landscape()
        self.DX_VAL, self.DY_VAL = f32(st.DX_VAL), f32(st.DY_VAL)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y)
        self.zmin, self.zmax, self.relh_adj_tex = f32(st.zmin), f32(st.zmax), f32(st.relh_adj_tex)
        self.vegetation, self.temperature = f32(ls.vegetation), f32(ls.temperature)
        self.snow_to_rock = bool(ls.water_is_lava or ls.disable_water == 2)
        self.gen_grass_map = ls.grass_density > 0 and float(self.vegetation) > 0.0  # src/tiled_mesh.cpp:126 (GRASS_THRESH > 0)
        self.num_rnd_grass_blocks = int(ls.num_rnd_grass_blocks)
        # init_terrain_mesh (src/mesh_gen.cpp:407-431): lttex_dirt[i].zval from mesh_rh_dirt; W_PLANE_Z = 0.42, get_rel_wpz() = CLIP_TO_01(W_PLANE_Z + water_h_off_rel)
        W_PLANE_Z = f32(0.42)
        rel_wpz = fmax(f32(0.0), fmin(f32(1.0), f32(W_PLANE_Z + f32(cfg.water_h_off_rel))))
        zvals = []
        for i, def_h in enumerate(f32(v) for v in (0.40, 0.44, 0.60, 0.75, 1.0)):
            if def_h < W_PLANE_Z:
                h = f32(f32(def_h * rel_wpz) / W_PLANE_Z)
            else:
                rel_h = f32(f32(def_h - W_PLANE_Z) / f32(f32(1.0) - W_PLANE_Z))
                h = f32(float(rel_wpz) + float(rel_h) * (1.0 - float(rel_wpz)))
                if i == SNOW:
                    h = fmin(h, def_h)
                    if float(self.temperature) > 40.0:
                        h = f32(float(h) + 0.01 * (float(self.temperature) - 40.0))
            zvals.append(h)
        # gen_tex_height_tables (src/Textures.cpp:1757-1761): h_dirt[i] = pow(lttex_dirt[i].zval, glaciate_exp) with float arguments: powf
        self.h_dirt = [f32(_libm.powf(float(z), float(st.glaciate_exp))) for z in zvals]
        tab = orc.sin_table()
        self.sin_table = tab
        two_pi = f32(2.0 * float(PI))
        self.sscale = f32(f32(TSIZE) / two_pi)

    def get_xval(self, i):  # src/mesh.h:122
        return f32(-self.X_SCENE_SIZE + f32(self.DX_VAL * f32(i)))

    def get_yval(self, i):
        return f32(-self.Y_SCENE_SIZE + f32(self.DY_VAL * f32(i)))

    def st_scale(self, v):  # int(sscale*val) & (TSIZE-1), src/sinf.h
        p = float(f32(self.sscale * f32(v)))
        i = int(p) if -2147483648.0 <= p < 2147483648.0 else -2147483648
        return i & (TSIZE - 1)

    def SINF(self, v):
        v = f32(v)
        return f32(-self.sin_table[self.st_scale(-v)]) if v < 0 else f32(self.sin_table[self.st_scale(v)])

    def COSF(self, v):
        return f32(self.sin_table[TSIZE + self.st_scale(abs(f32(v)))])

    def update_lttex_ix(self, ix):  # src/Textures.cpp:1289-1292
        if self.snow_to_rock and ix == SNOW:
            ix -= 1
        if float(self.vegetation) == 0.0 and ix == GRASS:
            ix += 1
        return ix

    def get_tids(self, relh):  # src/Textures.cpp:1294-1313 -> (k1, k2, t or None when *t is not written)
        h = self.h_dirt
        k1 = 0 if relh < h[0] else 1 if relh < h[1] else 2 if relh < h[2] else 3 if relh < h[3] else 4
        if k1 < 4 and f32(h[k1] - relh) < TEXTURE_SMOOTH:
            t = f32(1.0 - float(f32(f32(h[k1] - relh) / TEXTURE_SMOOTH)))
            return self.update_lttex_ix(k1), self.update_lttex_ix(k1 + 1), t
        k1 = self.update_lttex_ix(k1)
        return k1, k1, None


def adjust_brush_weight(sc, delta, dval, shape):  # src/heightmap.cpp:27-33
    if shape == BSHAPE_LINEAR:
        delta = f32(delta * f32(f32(1.0) - dval))
    elif shape == BSHAPE_QUADRATIC:
        delta = f32(delta * f32(f32(1.0) - f32(dval * dval)))
    elif shape == BSHAPE_COSINE:
        delta = f32(delta * sc.COSF(f32(f32(f32(0.5) * PI) * dval)))
    elif shape == BSHAPE_SINE:
        delta = f32(delta * f32(f32(0.5) * f32(f32(1.0) + sc.SINF(f32(f32(PI * dval) + f32(f32(0.5) * PI))))))
    return delta


def mesh_sphere_intersect(sc, x1, y1, dxoff, dyoff, stats, pos, rradius):
    """src/tiled_mesh.cpp:3796-3799 with get_center / get_mesh_bcube (src/tiled_mesh.h:229-241); x2 = x1 + size"""
    x2, y2 = x1 + SIZE, y1 + SIZE
    mzmin, mzmax, radius = f32(stats.mzmin), f32(stats.mzmax), f32(stats.radius)
    center = (sc.get_xval(((x1 + x2) >> 1) + dxoff), sc.get_yval(((y1 + y2) >> 1) + dyoff), f32(f32(0.5) * f32(mzmin + mzmax)))
    d = [f32(pos[i] - center[i]) for i in range(3)]
    dist_sq = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))  # p2p_dist_sq (src/inlines.h:176-178)
    dval = f32(radius + rradius)
    if not dist_sq < f32(dval * dval):  # dist_less_than
        return False
    xv1, yv1 = sc.get_xval(x1 + dxoff), sc.get_yval(y1 + dyoff)
    cube = [(xv1, f32(xv1 + f32(f32(x2 - x1) * sc.DX_VAL))), (yv1, f32(yv1 + f32(f32(y2 - y1) * sc.DY_VAL))),
            (f32(mzmin - BCUBE_ZTOLER), f32(mzmax + BCUBE_ZTOLER))]
    dmin, r2 = f32(0.0), f32(rradius * rradius)
    for i in range(3):  # DMIN_CHECK (src/Math3d.cpp:920-922)
        if pos[i] < cube[i][0]:
            dd = f32(pos[i] - cube[i][0]); dmin = f32(dmin + f32(dd * dd))
        elif pos[i] > cube[i][1]:
            dd = f32(pos[i] - cube[i][1]); dmin = f32(dmin + f32(dd * dd))
        if dmin > r2:
            return False
    return True


def add_grass_block_at(sc, blocks, x1, y1, is_distant, x, y, mhmin, mhmax):  # src/tiled_mesh.cpp:1354-1371 (an all-zero array is the empty vector resized)
    if is_distant or x >= SIZE or y >= SIZE or not sc.gen_grass_map:
        return
    gb = blocks[y // GRASS_BLOCK_SZ, x // GRASS_BLOCK_SZ]
    if gb["ix"] == 0:
        u = lambda v: v & 0xFFFFFFFF  # int + unsigned: unsigned arithmetic
        gb["ix"] = (u(u(x1 + x) + u(1567 * u(y1 + y))) % sc.num_rnd_grass_blocks) + 1
        gb["zmin"], gb["zmax"] = mhmin, mhmax
    else:
        gb["zmin"] = fmin(f32(gb["zmin"]), mhmin)  # min_eq
        gb["zmax"] = fmax(f32(gb["zmax"]), mhmax)


def add_or_remove_grass_at(sc, tx, ty, zvals, stats, weights, blocks, params, pos, rradius, add_grass, brush_shape, brush_weight, dxoff=0, dyoff=0, is_distant=False):
    """tile_t::add_or_remove_grass_at from :3847 on for tile (tx, ty) (x1 = tx*128): weights [129,129,4] u8 and blocks [32,32] (orclib.GRASS_BLOCK_DTYPE) are edited
    in place; params = orc.tile_terrain_params(tx, ty).  -> (updated, (xl, yl, xh, yh))"""
    x1, y1 = tx * SIZE, ty * SIZE
    pos = tuple(f32(v) for v in pos)
    rradius, brush_weight = f32(rradius), f32(brush_weight)
    if rradius == 0.0:
        return False, (SIZE, SIZE, 0, 0)
    if not mesh_sphere_intersect(sc, x1, y1, dxoff, dyoff, stats, pos, rradius):
        return False, (SIZE, SIZE, 0, 0)
    updated = False
    is_square = brush_shape == BSHAPE_CONST_SQ
    r_inv = f32(1.0 / float(rradius))
    dz_inv = f32(f32(1.0) / f32(sc.zmax - sc.zmin))
    xy_mult = f32(1.0 / float(f32(SIZE)))
    bweight = f32(10.0 * float(brush_weight))
    llc_x, llcy = sc.get_xval(x1 + dxoff), sc.get_yval(y1 + dyoff)
    xl, yl, xh, yh = SIZE, SIZE, 0, 0
    z = np.asarray(zvals, np.float32).reshape(ZVSIZE, ZVSIZE)
    ptx, pty = [llc_x], [llcy]  # pt.x / pt.y: `+= DX_VAL` in the loop headers, skipped rows and columns included
    for _ in range(TSIZE_TEX - 1):
        ptx.append(f32(ptx[-1] + sc.DX_VAL)); pty.append(f32(pty[-1] + sc.DY_VAL))
    for y in range(TSIZE_TEX):
        pt_y = pty[y]
        if abs(f32(pt_y - pos[1])) > rradius:
            continue
        for x in range(TSIZE_TEX):
            pt_x = ptx[x]
            if abs(f32(pt_x - pos[0])) > rradius:
                continue
            ex, ey = f32(pt_x - pos[0]), f32(pt_y - pos[1])
            d2 = f32(f32(ex * ex) + f32(ey * ey))  # p2p_dist_xy_sq (src/inlines.h:183-185)
            if not is_square and not d2 < f32(rradius * rradius):
                continue
            w = weights[y, x]
            gw = int(w[GRASS])
            if gw == (255 if add_grass else 0):
                continue
            delta = adjust_brush_weight(sc, bweight, f32(np.sqrt(d2) * r_inv), brush_shape)
            mh = (z[y, x], z[y, x + 1], z[y + 1, x], z[y + 1, x + 1])
            mhmin, mhmax = fmin(fmin(mh[0], mh[1]), fmin(mh[2], mh[3])), fmax(fmax(mh[0], mh[1]), fmax(mh[2], mh[3]))
            if add_grass:
                if float(delta) >= 0.99:  # full addition
                    w[GRASS] = 255
                    for i in range(4):
                        if i != GRASS:
                            w[i] = 0
                elif float(delta) > 0.01:  # partial addition
                    prev_gw = gw
                    gw = uchar(fmin(f32(255.0), f32(f32(gw) + f32(f32(255.0) * delta))))
                    w[GRASS] = gw
                    grass_added = (gw - prev_gw) & 0xFF
                    for i in range(4):
                        if grass_added <= 0:
                            break
                        if i == GRASS or w[i] == 0:
                            continue
                        num_rem = fmin(int(w[i]), grass_added)
                        w[i] = (int(w[i]) - num_rem) & 0xFF
                        grass_added = (grass_added - num_rem) & 0xFF
                add_grass_block_at(sc, blocks, x1, y1, is_distant, x, y, mhmin, mhmax)
                xl = min(xl, x); xh = max(xh, min(x + 1, SIZE))
                yl = min(yl, y); yh = max(yh, min(y + 1, SIZE))
                updated = True
            else:
                prev_gw = gw
                gw = uchar(fmax(f32(0.0), f32(f32(gw) - f32(f32(255.0) * delta))))
                w[GRASS] = gw
                grass_rem = (prev_gw - gw) & 0xFF
                if grass_rem == 0:
                    continue
                k1, k2, t = sc.get_tids(f32(sc.relh_adj_tex + f32(f32(mhmax - sc.zmin) * dz_inv)))
                t = f32(0.0) if t is None else t
                grass_rem2 = uchar(f32(t * f32(grass_rem)))
                grass_rem1 = (grass_rem - grass_rem2) & 0xFF
                if k1 == GRASS:
                    k1 = DIRT  # replace grass with dirt
                if k2 == GRASS:
                    k2 = DIRT
                if k2 < 4:
                    w[k2] = (int(w[k2]) + grass_rem2) & 0xFF
                if k1 < 4:
                    w[k1] = (int(w[k1]) + grass_rem1) & 0xFF
                fx, fy = f32(f32(x) * xy_mult), f32(f32(y) * xy_mult)
                p = params[:, :, 2]  # BILINEAR_INTERP(params, dirt, x, y) (src/tiled_mesh.cpp:189): params[yp][xp]
                one = f32(1.0)
                dirt_scale = f32(f32(fy * f32(f32(fx * p[1, 1]) + f32(f32(one - fx) * p[1, 0]))) + f32(f32(one - fy) * f32(f32(fx * p[0, 1]) + f32(f32(one - fx) * p[0, 0]))))
                if float(dirt_scale) < 1.0:  # convert dirt to sand
                    dirt_w = int(w[DIRT])
                    w[SAND] = (int(w[SAND]) + uchar((1.0 - float(dirt_scale)) * dirt_w)) & 0xFF
                    w[DIRT] = uchar(f32(dirt_scale * f32(dirt_w)))
                updated = True
    if not updated:
        return False, (SIZE, SIZE, 0, 0)
    if not add_grass and (blocks["ix"] != 0).any():  # has_grass(): the has-grass scan (:3938-3945)
        if not (weights[:, :, GRASS] > 0).any():
            blocks[...] = np.zeros((), orclib.GRASS_BLOCK_DTYPE)
    return True, ((xl, yl, xh, yh) if add_grass else (SIZE, SIZE, 0, 0))
