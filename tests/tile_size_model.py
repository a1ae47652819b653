"""A size-general model of the tile path (tile_t at get_tile_size() = S = MESH_X_SIZE, src/tiled_mesh.cpp:142,300-314,447-546,586-692,865-880), built only from
the oracle's exported primitives (gen_grid, apply_erosion, get_clamped_height, calc_mesh_shadows) and numpy.  The oracle's own tile functions are fixed at
S = 128; tests/test_tile_size_model.py pins every piece of this model to them there, so at other sizes it stands for the reference.

orc: an orclib.Checker initialised with mesh_x = mesh_y = S (the scene of the tiles)."""
import numpy as np

F = np.float32
AO_RAY_LEN = 36
FAR_DISTANCE = F(100.0)


def _st(orc):
    return orc.state()


def field_origin(orc, S, tx, ty, shift=0):
    """(x0, y0) of build_arrays for a tile field: (x1 - shift) - MESH_X_SIZE/2 with MESH_X_SIZE = MESH_Y_SIZE = S"""
    return float((tx * S - shift) - S // 2), float((ty * S - shift) - S // 2)


def hmap_field(orc, S, tx, ty, size, shift, detail_scale=None):
    """get_clamped_height(x1 - shift + x, y1 - shift + y) (+ HMAP_DETAIL_MAG * the detail grid at xy_scale detail_scale)"""
    x1, y1 = tx * S - shift, ty * S - shift
    z = np.empty((size, size), F)
    for y in range(size):
        for x in range(size):
            z[y, x] = orc.get_clamped_height(x1 + x, y1 + y)
    if detail_scale:
        s = _st(orc)
        x0, y0 = field_origin(orc, S, tx, ty, shift)
        g = orc.gen_grid(x0, y0, F(detail_scale) * F(s.DX_VAL), F(detail_scale) * F(s.DY_VAL), size, size, 1)
        z = (z + F(0.01) * g).astype(F)
    return z


def ao_context(orc, S, tx, ty, hmap=False, detail_scale=None):
    """the (S + 73)^2 grid around the tile at (x1 - 36, y1 - 36): setup_height_gen_async / get_clamped_height (src/tiled_mesh.cpp:609-627)"""
    cs = S + 1 + 2 * AO_RAY_LEN
    if hmap:
        return hmap_field(orc, S, tx, ty, cs, AO_RAY_LEN, detail_scale)
    s = _st(orc)
    x0, y0 = field_origin(orc, S, tx, ty, AO_RAY_LEN)
    return orc.gen_grid(x0, y0, s.DX_VAL, s.DY_VAL, cs, cs, 1)


def tile_zvals(orc, S, tx, ty, iters_tt=0, ao_clip=False, hmap=False, detail_scale=None):
    """tile_t::create_zvals' heights: the (S + 2)^2 field at the tile's origin (or clipped out of the AO context, or sampled from the heightmap texture), eroded"""
    zv = S + 2
    if hmap:
        return hmap_field(orc, S, tx, ty, zv, 0, detail_scale)  # "heightmap is eroded during load" (:515)
    if ao_clip:
        z = np.ascontiguousarray(ao_context(orc, S, tx, ty)[AO_RAY_LEN:AO_RAY_LEN + zv, AO_RAY_LEN:AO_RAY_LEN + zv])
    else:
        s = _st(orc)
        x0, y0 = field_origin(orc, S, tx, ty)
        z = orc.gen_grid(x0, y0, s.DX_VAL, s.DY_VAL, zv, zv, 1)
    if iters_tt:
        orc.apply_erosion(z, _st(orc).zmin, iters_tt)
    return z


def _min_std(a, b): return b if b < a else a      # std::min
def _max_std(a, b): return b if a < b else a      # std::max


def tile_stats(orc, S, tx, ty, z):
    """the sub-block / water-bbox loop of create_zvals (src/tiled_mesh.cpp:517-541) -> dict with the terra_tile_stats fields"""
    s = _st(orc)
    zv = S + 2
    bs = zv // 4
    x1, y1 = tx * S, ty * S
    wpz_max = F(orc.get_max_sea_level())
    sub_zmin, sub_zmax = [], []
    mzmin, mzmax = FAR_DISTANCE, -FAR_DISTANCE
    for yy in range(4):
        for xx in range(4):
            blk = z[yy * bs:(yy + 1) * bs + 1, xx * bs:(xx + 1) * bs + 1]
            v = blk[blk == blk]
            szmin, szmax = FAR_DISTANCE, -FAR_DISTANCE
            if v.size:  # std::min / std::max over the block in row order: a NaN never wins; equal values keep the first (only +-0 can tell)
                szmin, szmax = _min_std(szmin, F(v.min())), _max_std(szmax, F(v.max()))
            sub_zmin.append(F(szmin)); sub_zmax.append(F(szmax))
            mzmin = F(_min_std(mzmin, szmin)); mzmax = F(_max_std(mzmax, szmax))
    lim = 4 * bs
    wet = z[:lim + 1, :lim + 1] < wpz_max
    wx1, wy1, wx2, wy2 = x1 + S, y1 + S, x1, y1
    if wet.any():
        ys, xs = np.nonzero(wet)
        wx1, wy1, wx2, wy2 = min(wx1, x1 + int(xs.min())), min(wy1, y1 + int(ys.min())), max(wx2, x1 + int(xs.max())), max(wy2, y1 + int(ys.max()))
    dx2 = F(F(s.DX_VAL) * F(s.DX_VAL) + F(s.DY_VAL) * F(s.DY_VAL))
    rad_c = F(F(dx2 * F(S)) * F(S))
    dz = F(mzmax - mzmin)
    radius = F(0.5 * np.sqrt(np.float64(F(rad_c + F(dz * dz)))))
    return dict(sub_zmin=sub_zmin, sub_zmax=sub_zmax, mzmin=F(mzmin), mzmax=F(mzmax), radius=radius, wx1=wx1, wy1=wy1, wx2=wx2, wy2=wy2)


def stats_bytes(st):
    """the terra_tile_stats / orc_tile_stats_t bytes of a tile_stats() dict"""
    return (np.array(st["sub_zmin"] + st["sub_zmax"] + [st["mzmin"], st["mzmax"], st["radius"]], F).tobytes()
            + np.array([st["wx1"], st["wy1"], st["wx2"], st["wy2"]], np.int32).tobytes())


def tile_normals(orc, S, z):
    """upload_normal_texture (src/tiled_mesh.cpp:865-880) with get_norm (src/tiled_mesh.h:281-284) -> (rgba [S+1][S+1][4], min_normal_z)"""
    s = _st(orc)
    st = S + 1
    with np.errstate(all="ignore"):
        zc, zr, zd = z[:st, :st], z[:st, 1:st + 1], z[1:st + 1, :st]
        n0 = (F(s.DY_VAL) * (zc - zr).astype(F)).astype(F)
        n1 = (F(s.DX_VAL) * (zc - zd).astype(F)).astype(F)
        n2 = np.full_like(n0, F(s.dxdy))
        mag = np.sqrt(((n0 * n0).astype(F) + (n1 * n1).astype(F)).astype(F) + (n2 * n2).astype(F)).astype(F)
        norm = ~(mag < F(1.0e-12))
        q = [np.where(norm, (c / mag).astype(F), c) for c in (n0, n1, n2)]
        rgba = np.zeros((st, st, 4), np.uint8)
        for i in range(3):
            rgba[:, :, i] = np.floor(127.0 * (q[i].astype(np.float64) + 1.0)).astype(np.int64).astype(np.uint8)
    mnz = F(1.0)
    v = q[2][q[2] == q[2]]
    if v.size and F(v.min()) < mnz:
        mnz = F(v.min())
    return rgba, mnz


def tile_ao(orc, S, tx, ty, z, hmap=False, ao_clip=False, detail_scale=None):
    """calc_mesh_ao_lighting (src/tiled_mesh.cpp:586-661): 8 directions x 8 steps over the (S + 73)^2 context -> [S+1][S+1] bytes.  Inside the tile the context is
    the tile's own zvals, except with the AO-context clip (ao_zvals: the context everywhere)."""
    st, zv, rl = S + 1, S + 2, AO_RAY_LEN
    ctx = np.array(ao_context(orc, S, tx, ty, hmap, detail_scale), F)
    if not ao_clip or hmap:
        ctx[rl:rl + zv, rl:rl + zv] = z
    dz = F(0.5 * np.float64(F(_st(orc).HALF_DXY)))
    ys, xs = np.mgrid[0:st, 0:st]
    atten = np.zeros((st, st), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            z0 = z[:st, :st].astype(F).copy()
            done = np.zeros((st, st), bool)
            for s in range(8):
                T = (s + 1) * (s + 2) // 2
                z0 = (z0 + dz).astype(F)
                hit = ~done & (ctx[ys + rl + T * dy, xs + rl + T * dx] > z0)
                atten[hit] += 8 - s
                done |= hit
    scale = (1.0 - (atten.astype(F) / F(64)).astype(np.float64)).astype(F)
    return np.floor(255.0 * scale.astype(np.float64)).astype(np.uint8)


def tiles_shadows(orc, S, tile_xy, zvals, lpos):
    """orc_tiles_mesh_shadows' order at any size: a tile after its batch neighbours toward the light, starting from their outgoing edges"""
    zv = S + 2
    n = len(tile_xy)
    idx = {}
    for i, t in enumerate(tile_xy):
        idx.setdefault((int(t[0]), int(t[1])), i)  # the first entry with those coordinates, as the oracle's linear search
    sx = -1 if lpos[0] < 0 else 1
    sy = -1 if lpos[1] < 0 else 1
    smask = np.zeros((n, zv, zv), np.uint8)
    out = [None] * n  # (sh_out_x, sh_out_y)
    done = [False] * n

    def rec(i):
        if done[i]:
            return
        done[i] = True
        tx, ty = int(tile_xy[i][0]), int(tile_xy[i][1])
        sh_in = [None, None]
        for d, (ax, ay) in enumerate(((tx + sx, ty), (tx, ty + sy))):
            j = idx.get((ax, ay))
            if j is not None:
                rec(j)
                sh_in[1 - d] = out[j][1 - d]
        sm, so_x, so_y = orc.calc_mesh_shadows(lpos, zvals[i], sh_in[0], sh_in[1])
        smask[i] = sm
        out[i] = (so_x, so_y)

    for i in range(n):
        rec(i)
    return smask
