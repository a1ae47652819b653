"""NumPy / Python restatement of the tree map and of the two textures that read it, written from the reference statements (not from the library's kernels):

    tile_t::add_tree_ao_shadow (texel loop)   src/tiled_mesh.cpp:749-767
    tile_t::apply_tree_ao_shadows (the clear) src/tiled_mesh.cpp:820-828
    tile_t::push_tree_ao_shadow (distant)     src/tiled_mesh.cpp:740-746
    tile_t::upload_shadow_map_texture         src/tiled_mesh.cpp:885-911
    tile_t::create_texture (the tree pass)    src/tiled_mesh.cpp:1325-1348
    round_fp                                  src/inlines.h:63
    get_xval / get_yval                       src/mesh.h:122-123
    xstart / ystart                           src/tiled_mesh.cpp:309-310
    SHADOWED_ALL                              src/3DWorld.h:1404

Types.  Every operand carries the type the reference statement gives it: np.float32 for float, Python float for double, Python int for int, and a
conversion to unsigned char is the truncation toward zero of a value that is in range wherever the reference is defined.  x86-64 SSE2, no fused multiply-add.

mult (:761) is `float const mult(0.2 + 0.8*scale*sqrt(dist_sq))` with float scale and float dist_sq.  0.2 and 0.8 are double literals, so the two products and the
sum are double and the result is rounded to float once, by the initialisation.  sqrt is NOT the double function here: the reference includes <math.h>
(src/3DWorld.h:13, src/inlines.h:8), and g++'s <math.h> declares std::sqrt's overloads in the global namespace, so sqrt(float) is the float overload: the root is
rounded to float first and enters the double expression as that float.  scale (:754) is `float const scale(0.6/rval)`: a double division rounded to float.

This reading -- the overloads and promotions above, and those of the two textures -- is confirmed against the compiler's output: tests/test_tile_members_ref.py
compares this model, every byte, with tile_t's own compiled members (oracle/ref_shim.cpp section 4), on maps where a double sqrt or float products would change a byte.

The scene constants (DX_VAL, DY_VAL, X_SCENE_SIZE, Y_SCENE_SIZE) come from the oracle's state (orclib.Checker.state()), not from the library under test.
"""
import numpy as np

f32 = np.float32
SHADOWED_ALL = 0xCF  # src/3DWorld.h:1404
RVAL_MAX = 46340     # rval*rval fits an int up to here
SPLAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("radius", np.float32)])


class Scene:
    """the globals the tree map reads, from the oracle: Scene(orc.init(cfg), cfg) or Scene(orc.state(), cfg)"""

    def __init__(self, state, cfg):
        self.DX_VAL, self.DY_VAL = f32(state.DX_VAL), f32(state.DY_VAL)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y)
        self.S = int(cfg.mesh_x)  # get_tile_size() = MESH_X_SIZE (src/tiled_mesh.cpp:142)

    def get_xval(self, i):  # src/mesh.h:122: -X_SCENE_SIZE + DX_VAL*xpos, xpos converted to float
        return f32(-self.X_SCENE_SIZE + f32(self.DX_VAL * f32(i)))

    def get_yval(self, i):  # src/mesh.h:123
        return f32(-self.Y_SCENE_SIZE + f32(self.DY_VAL * f32(i)))


def round_fp(v):
    """src/inlines.h:63: (val > 0.0f) ? int(val + 0.5f) : int(val - 0.5f), the sums in float"""
    v = f32(v)
    return int(f32(v + f32(0.5))) if v > f32(0.0) else int(f32(v - f32(0.5)))


def splat_params(sc, tx, ty, dxoff, dyoff, x, y, tr):
    """:751-754 -> (xc, yc, rval, scale), or None where the reference is undefined and the library skips the splat: a non-finite member, tradius < 0,
    rval > 46340 (rval*rval overflows an int), |xc| or |yc| beyond 2^30 (a quotient beyond 2^30 in magnitude: floats there are integers, round_fp leaves them)"""
    x, y, tr = f32(x), f32(y), f32(tr)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(tr)) or tr < 0:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        xstart, ystart = sc.get_xval(tx * sc.S + dxoff), sc.get_yval(ty * sc.S + dyoff)  # src/tiled_mesh.cpp:309-310
        vx, vy = f32(f32(x - xstart) / sc.DX_VAL), f32(f32(y - ystart) / sc.DY_VAL)
        qx, qy = f32(tr / sc.DX_VAL), f32(tr / sc.DY_VAL)
    if not (abs(vx) <= 2.0 ** 30 and abs(vy) <= 2.0 ** 30):
        return None
    if not (qx < RVAL_MAX + 1 and qy < RVAL_MAX + 1):
        return None
    rval = max(int(qx), int(qy)) + 1  # int rval(max(int(tradius/DX_VAL), int(tradius/DY_VAL)) + 1)
    if rval > RVAL_MAX:
        return None
    return round_fp(vx), round_fp(vy), rval, f32(0.6 / rval)  # float const scale(0.6/rval): double division, rounded once


def mult_of(scale, dist_sq):
    """:761 for an array of float dist_sq: float(0.2 + 0.8*scale*sqrt(dist_sq)) -- double products and sum, float sqrt (see the module docstring)"""
    root = np.sqrt(np.asarray(dist_sq, f32)).astype(f32)  # sqrtf: correctly rounded float root
    return (0.2 + (0.8 * float(scale)) * root.astype(np.float64)).astype(f32)  # (0.8*scale)*sqrt: left to right


def add_tree_ao_shadow(sc, tree_map, p):
    """the texel loop :753-767 on one tile's map (u8 [S+1, S+1, 2] = {ao, sh}, in place) for p = splat_params(...) -> updated"""
    xc, yc, rval, scale = p
    S = sc.S
    rval_sq = rval * rval
    x1, y1, x2, y2 = max(0, xc - rval), max(0, yc - rval), min(S, xc + rval), min(S, yc + rval)
    if x2 < x1 or y2 < y1:
        return False
    ys, xs = np.mgrid[y1:y2 + 1, x1:x2 + 1]
    dx, dy = np.abs(xs - xc).astype(f32), np.abs(ys - yc).astype(f32)  # float const dx(abs(x - xc)): int abs, then float
    dist_sq = (dx * dx + dy * dy).astype(f32)
    hit = ~(dist_sq > f32(rval_sq))  # if (dist_sq > rval_sq) continue: the int converted to float
    if not hit.any():
        return False
    mult = mult_of(scale, dist_sq)
    win = tree_map[y1:y2 + 1, x1:x2 + 1]
    for ch in (0, 1):  # val.ao *= mult; val.sh *= mult: (unsigned char)((float)val*mult)
        v = (win[..., ch].astype(f32) * mult).astype(f32)
        win[..., ch] = np.where(hit, np.trunc(v).astype(np.uint8), win[..., ch])
    return True


def tiles_tree_map(sc, tiles, splats, first, reset, tree_map=None, dxoff=0, dyoff=0, distant=None):
    """every tile of a batch: the fill of apply_tree_ao_shadows under reset (an all-255 map reads as the reference's empty one), then the tile's splats
    splats[first[t]:first[t+1]] in list order; a distant tile is only filled (:743, :822) -> (tree_map u8 [n, S+1, S+1, 2], updated bool [n])"""
    n, W = len(tiles), sc.S + 1
    if tree_map is None:
        assert reset
        tree_map = np.empty((n, W, W, 2), np.uint8)
    upd = np.zeros(n, bool)
    for t, (tx, ty) in enumerate(tiles):
        if reset:
            tree_map[t] = 255
        if distant is not None and distant[t]:
            continue
        for k in range(int(first[t]), int(first[t + 1])):
            p = splat_params(sc, tx, ty, dxoff, dyoff, splats[k]["x"], splats[k]["y"], splats[k]["radius"])
            if p is not None:
                upd[t] |= add_tree_ao_shadow(sc, tree_map[t], p)
    return tree_map, upd


def shadow_flags(light_factor):
    """:885, :890: light_factor is the engine's float; 0.4, 0.6 and 5.0 are double literals -> (has_sun, has_moon, lfs)"""
    lf = float(f32(light_factor))
    with np.errstate(invalid="ignore", over="ignore"):
        return lf >= 0.4, lf <= 0.6, f32(5.0 * (lf - 0.4))


def shadow_texture(S, light_factor, mesh_shadows, smask_sun=None, smask_moon=None, ao=None, tree_map=None):
    """:885-911 for arrays of tiles: smask_* u8 [n, S+2, S+2], ao u8 [n, S+1, S+1] or None (170), tree_map u8 [n, S+1, S+1, 2] or None (empty)
    -> u8 [n, S+1, S+1, 4]; n from whichever input is given"""
    has_sun, has_moon, lfs = shadow_flags(light_factor)
    assert has_sun or has_moon  # (:844)
    n = next(len(a) for a in (smask_sun, smask_moon, ao, tree_map) if a is not None)
    W = S + 1
    out = np.zeros((n, W, W, 4), np.uint8)  # vector<unsigned char> shadow_data(4*stride*stride, 0)
    base_ao = np.full((n, W, W), 170, np.uint8) if ao is None else np.asarray(ao, np.uint8).reshape(n, W, W)  # :896
    if tree_map is None:
        out[..., 2] = base_ao
        out[..., 1] = 255
    else:
        tao, tsh = tree_map[..., 0], tree_map[..., 1]
        scaled = (base_ao.astype(f32) * (f32(0.3) + (f32(0.7) * tao.astype(f32)) / f32(255.0))).astype(f32)  # base_ao * (0.3f + 0.7f*tree_map[ix].ao/255.0f)
        out[..., 2] = np.where(tao == 255, base_ao, np.trunc(scaled).astype(np.uint8))                      # :897-898
        out[..., 1] = np.trunc(f32(63.75) + f32(0.75) * tsh.astype(f32)).astype(np.uint8)                  # :909
    shadow_val = np.full((n, W, W), 255, np.uint8)
    if mesh_shadows:
        if has_sun:
            assert smask_sun is not None  # :888
        if has_moon:
            assert smask_moon is not None  # :889
        crop = lambda m: np.asarray(m, np.uint8).reshape(n, S + 2, S + 2)[:, :W, :W]  # noqa: E731  ix2 = y*zvsize + x
        if has_sun and has_moon:
            sun_en = ((crop(smask_sun) & SHADOWED_ALL) == 0).astype(f32)
            moon_en = ((crop(smask_moon) & SHADOWED_ALL) == 0).astype(f32)
            f = (lfs * sun_en + (f32(1.0) - lfs) * moon_en).astype(f32)
            shadow_val = np.trunc(f32(255.0) * f).astype(np.uint8)  # shadow_val *= (...): (unsigned char)((float)255*f)
        else:
            cur = crop(smask_sun if has_sun else smask_moon)  # :887
            shadow_val = np.where((cur & SHADOWED_ALL) != 0, 0, 255).astype(np.uint8)
    out[..., 0] = shadow_val
    return out


SAND, DIRT, GRASS, ROCK = 0, 1, 2, 3  # get_texture_ixs maps the textures in the LT_* order (tests/grass_brush_model.py)


def tree_weights(mesh_weights, tree_map=None):
    """:1325-1348 with sz_factor == 1: u8 [..., 4] weights and u8 [..., 2] tree map of the same leading shape (or None: the plain copy) -> weight_data"""
    w = np.array(mesh_weights, np.uint8)  # weight_data = mesh_weight_data
    if tree_map is None:
        return w
    tree_ao = np.asarray(tree_map, np.uint8)[..., 0]
    act = (tree_ao != 255) & (w[..., ROCK] != 255)  # :1335, :1340
    v = (tree_ao.astype(np.float64) / 255.0).astype(f32)  # float const v(tree_ao/255.0)
    wsum = (w[..., DIRT].astype(np.float64) + (1.0 - v.astype(np.float64)) * w[..., GRASS].astype(np.float64)).astype(f32)  # w(dirt + (1.0 - v)*grass)
    dirt = np.trunc(np.maximum(f32(0.0), np.minimum(f32(255.0), wsum))).astype(np.uint8)
    grass = np.trunc((w[..., GRASS].astype(f32) * v).astype(f32)).astype(np.uint8)  # weight_data[off+grass_tex_ix] *= v
    w[..., DIRT] = np.where(act, dirt, w[..., DIRT])
    w[..., GRASS] = np.where(act, grass, w[..., GRASS])
    return w
