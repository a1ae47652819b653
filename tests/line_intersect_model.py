"""NumPy restatement of the line-vs-terrain query, written from the reference statements (not from the library's kernels):

    tile_draw_t::line_intersect_mesh    src/tiled_mesh.cpp:3582-3605 (inc_trees = 0)
    tile_t::line_intersect_mesh         src/tiled_mesh.cpp:2176-2213
    get_mesh_bcube                      src/tiled_mesh.h:238-241, BCUBE_ZTOLER src/tiled_mesh.h:32
    do_line_clip, get_region            tests/view_model.py's
    get_xval / get_xpos                 src/mesh.h:122-123, 129-130
    line_intersect_tiled_mesh_get_tile  src/tiled_mesh.cpp:3643-3648

Every float statement is evaluated in float32 in the reference's order (x86-64 SSE2, no fused multiply-add); where the C++ promotes to double the model uses
float64.  Conversions to int are x86's cvttsd2si (INT_MIN when out of range or NaN) and int arithmetic wraps at 32 bits, as in the reference binary.  The model
works on arrays of (line, tile) pairs so that it can check tens of thousands of lines against a 64 x 64 batch; each array statement is the scalar statement it cites.
This reading is confirmed against the compiler's output: tests/test_tile_members_ref.py compares the model with the compiled tile_t::line_intersect_mesh
(oracle/ref_shim.cpp section 4) on lines built around the box's faces, get_xpos' ties and the zero denominator.
"""
import numpy as np

import view_model

f32, f64 = np.float32, np.float64
get_region, do_line_clip = view_model.line_region, view_model.do_line_clip
BCUBE_ZTOLER = f32(1.0E-6)   # src/tiled_mesh.h:32
INT_MIN = -2 ** 31
MAX_STEPS = 10000            # assert(steps < 10000) (src/tiled_mesh.cpp:2187)
HIT_DTYPE = np.dtype([("t", np.float32), ("tile", np.int32), ("xpos", np.int32), ("ypos", np.int32), ("p_int", np.float32, (3,)), ("hit", np.uint32)])


class Scene:
    """the globals the query reads: X/Y_SCENE_SIZE, DX/DY_VAL, DX/DY_VAL_INV and the tile size S"""

    def __init__(self, scene_x, scene_y, DX_VAL, DY_VAL, DX_VAL_INV, DY_VAL_INV, S):
        self.xss, self.yss = f32(scene_x), f32(scene_y)
        self.DX_VAL, self.DY_VAL, self.DX_VAL_INV, self.DY_VAL_INV = f32(DX_VAL), f32(DY_VAL), f32(DX_VAL_INV), f32(DY_VAL_INV)
        self.S = int(S)

    @classmethod
    def of(cls, cfg, st):
        """from a terra_config and the terra_state derived from it"""
        return cls(cfg.scene_x, cfg.scene_y, st.DX_VAL, st.DY_VAL, st.DX_VAL_INV, st.DY_VAL_INV, cfg.mesh_x)


def wrap(v):
    """int32 wrap-around of an int64 array"""
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)


def cvtt(v):
    """(int)<double>: truncation toward zero, INT_MIN when out of range or NaN (cvttsd2si)"""
    v = np.asarray(v, f64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), INT_MIN).astype(np.int64)


def mesh_bcube(sc, tx, ty, mzmin, mzmax, dxoff, dyoff):
    """get_mesh_bcube(): d[3][2] per tile as 6 float32 arrays, and x1, y1 = tx*size, ty*size (tile_t::tile_t, src/tiled_mesh.cpp:304-305)"""
    x1, y1 = wrap(np.asarray(tx, np.int64) * sc.S), wrap(np.asarray(ty, np.int64) * sc.S)
    xv1 = -sc.xss + sc.DX_VAL * wrap(x1 + dxoff).astype(f32)  # get_xval(x1 + xoff - xoff2)
    yv1 = -sc.yss + sc.DY_VAL * wrap(y1 + dyoff).astype(f32)
    d = [xv1, xv1 + f32(sc.S) * sc.DX_VAL, yv1, yv1 + f32(sc.S) * sc.DY_VAL,  # xv1 + (x2 - x1)*DX_VAL
         np.asarray(mzmin, f32) - BCUBE_ZTOLER, np.asarray(mzmax, f32) + BCUBE_ZTOLER]
    return [np.asarray(a, f32) for a in d], x1, y1


def get_pos(v, ss, inv):
    """get_xpos(x) = int((x + X_SCENE_SIZE)*DX_VAL_INV + 0.5): float sum and product, double add, x86 truncation"""
    return cvtt(((v + ss) * inv).astype(f64) + 0.5)


def tile_hits(sc, zvals, tile_of_pair, x1, y1, d, v1, v2, dxoff, dyoff):
    """tile_t::line_intersect_mesh (:2176-2213) for every (line, tile) pair: v1, v2 the pairs' unclipped ends, d / x1 / y1 the pairs' tiles' boxes.
    -> (hit bool, t float32, xpos, ypos) per pair.  Non-finite lines and distant tiles are the caller's (they never get here)."""
    npairs = len(v1[0])
    hit, t_out = np.zeros(npairs, bool), np.full(npairs, f32(1.0), f32)
    xpos, ypos = np.zeros(npairs, np.int64), np.zeros(npairs, np.int64)
    with np.errstate(all="ignore"):
        ok, v1c, v2c = do_line_clip(v1, v2, d)
        xp1 = wrap(get_pos(v1c[0], sc.xss, sc.DX_VAL_INV) - x1 - dxoff)  # get_xpos(v1c.x) - x1 - xoff + xoff2
        yp1 = wrap(get_pos(v1c[1], sc.yss, sc.DY_VAL_INV) - y1 - dyoff)
        xp2 = wrap(get_pos(v2c[0], sc.xss, sc.DX_VAL_INV) - x1 - dxoff)
        yp2 = wrap(get_pos(v2c[1], sc.yss, sc.DY_VAL_INV) - y1 - dyoff)
        dx, dy = wrap(xp2 - xp1), wrap(yp2 - yp1)
        iabs = lambda v: wrap(np.abs(v))  # noqa: E731  abs(INT_MIN) == INT_MIN
        steps = np.maximum(1, np.maximum(iabs(dx), iabs(dy)))
        ok &= steps < MAX_STEPS  # (the reference asserts)
        dz = v2c[2].astype(f64) - v1c[2].astype(f64)
        xinc, yinc, zinc = dx / steps.astype(f64), dy / steps.astype(f64), dz / steps.astype(f64)
        x, y = xp1.astype(f64), yp1.astype(f64)
        z = v1c[2].astype(f64) - 0.1 * np.abs(zinc)  # z offset below the clipped v1 (:2190)
        den = v2[2].astype(f64) - v1[2].astype(f64)
        live = np.nonzero(ok)[0]  # the pairs still walking
        x, y, z, xinc, yinc, zinc, steps, den = (a[live] for a in (x, y, z, xinc, yinc, zinc, steps, den))
        v1z, zt = v1[2][live].astype(f64), tile_of_pair[live]
        S, k = sc.S, 0
        while len(live):
            ix, iy = cvtt(x), cvtt(y)  # (int)x
            inb = (ix >= 0) & (iy >= 0) & (ix <= S) & (iy <= S)
            zv = zvals[zt, np.where(inb, iy, 0), np.where(inb, ix, 0)].astype(f64)
            test = inb & (zv > z)
            cur_t = (((z - 0.5 * zinc) - v1z) / den).astype(f32)  # t relative to the original v1, v2
            got = test & (cur_t >= 0.0) & (cur_t <= 1.0)
            g = live[got]
            hit[g], t_out[g], xpos[g], ypos[g] = True, cur_t[got], wrap(x1[g] + ix[got]), wrap(y1[g] + iy[got])
            x, y, z = x + xinc, y + yinc, z + zinc
            k += 1
            keep = ~got & (k <= steps)
            live, x, y, z, xinc, yinc, zinc, steps, den, v1z, zt = (a[keep] for a in (live, x, y, z, xinc, yinc, zinc, steps, den, v1z, zt))
    return hit, t_out, xpos, ypos


def batch_hits(sc, tile_xy, zvals, mzmin, mzmax, lines, line_tile=None, dxoff=0, dyoff=0, distant=None, chunk_pairs=1 << 21):
    """tile_draw_t::line_intersect_mesh (:3582-3605) + line_intersect_tiled_mesh_get_tile's p_int (:3643-3648) for every line -> HIT_DTYPE [nlines].
    tile_xy [n, 2], zvals [n, S+2, S+2], mzmin / mzmax [n], lines [nlines, 2, 3]; line_tile [nlines] (>= 0: that tile alone, >= n: none); distant [n] bool."""
    txy = np.asarray(tile_xy, np.int64).reshape(-1, 2)
    n = len(txy)
    lines = np.asarray(lines, f32).reshape(-1, 2, 3)
    nl = len(lines)
    out = np.zeros(nl, HIT_DTYPE)
    out["t"], out["tile"] = 2.0, -1
    if n == 0 or nl == 0:
        return out
    d_all, x1_all, y1_all = mesh_bcube(sc, txy[:, 0], txy[:, 1], mzmin, mzmax, dxoff, dyoff)
    live_tile = np.ones(n, bool) if distant is None else ~np.asarray(distant, bool)  # if (is_distant) return 0 (:2178)
    finite = np.isfinite(lines).all(axis=(1, 2))  # assert(!is_nan(v1) && !is_nan(v2)) (:2179): a miss here
    lt = np.full(nl, -1, np.int64) if line_tile is None else np.asarray(line_tile, np.int64)
    per = max(1, chunk_pairs // n)
    for l0 in range(0, nl, per):
        ls = np.arange(l0, min(nl, l0 + per))
        li, ti = np.repeat(ls, n), np.tile(np.arange(n), len(ls))
        sel = finite[li] & live_tile[ti] & ((lt[li] < 0) | (lt[li] == ti))
        li, ti = li[sel], ti[sel]
        v1 = [lines[li, 0, a] for a in range(3)]
        v2 = [lines[li, 1, a] for a in range(3)]
        d = [a[ti] for a in d_all]
        pre = (get_region(v1, d) & get_region(v2, d)) == 0  # do_line_clip's first test, only to keep the walk's arrays small
        li, ti, v1, v2, d = li[pre], ti[pre], [a[pre] for a in v1], [a[pre] for a in v2], [a[pre] for a in d]
        hit, t, xp, yp = tile_hits(sc, zvals, ti, x1_all[ti], y1_all[ti], d, v1, v2, dxoff, dyoff)
        # over the tiles in batch order: `tn < t` from t = 2.0 keeps the first of the smallest t (-0 == +0)
        li, ti, t, xp, yp = li[hit], ti[hit], t[hit], xp[hit], yp[hit]
        order = np.lexsort((ti, t + f32(0.0), li))
        li, ti, t, xp, yp = li[order], ti[order], t[order], xp[order], yp[order]
        first = np.ones(len(li), bool)
        first[1:] = li[1:] != li[:-1]
        for r, i, tv, xv, yv in zip(li[first], ti[first], t[first], xp[first], yp[first]):
            v1l, v2l = lines[r, 0], lines[r, 1]
            out[r] = (tv, i, xv, yv, v1l + tv * (v2l - v1l), 1)  # p_int = v1 + t*(v2 - v1), float32
    return out
