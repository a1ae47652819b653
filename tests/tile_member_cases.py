"""Inputs and comparisons for five tile_t members taken from the reference's own object file (oracle/ref_shim.cpp section 4: ref_tile_tree_map,
ref_tile_shadow_texture, ref_tile_tree_weights, ref_tile_line_intersect, ref_tile_grass_brush), shared by tests/test_tile_members_ref.py,
tests/test_gpu_tile_members_ref.py and tests/golden/make_tile_member_golden.py.

Every input is seeded or a formula, and is built where these bodies go wrong rather than drawn evenly: rounding ties, +-1 / +-2 ulp siblings of a threshold, every
byte value, borders.  `ref_*` runs the compiled reference (an orclib.Checker("ref")), `model_*` the Python models, `lib_*` the library (the emulator or HIP) through
its C ABI; every comparison is exact.  No generated row is one where the reference is undefined: the builders assert it, and the model runners count the rows they
would have had to skip (the count is asserted to be 0 by the callers)."""
import os

import numpy as np

import grass_brush_model as gbm
import line_intersect_model as lim
import orclib
import tree_map_model as tmm

f32 = np.float32
S, W, Z = 128, 129, 130
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_member_vectors.npz")
SCENES = [(4.0, 4.0, 4.0), (4.0, 6.0, 4.0)]  # the second: DX_VAL != DY_VAL
STEPS = (-2, -1, 0, 1, 2)


def step(x, k):
    """the float32 x moved by k units in the last place (through zero: -0.0 and 0.0 are one value)"""
    i = int(np.asarray(x, f32).reshape(1).view(np.int32)[0])
    key = (i if i >= 0 else -(i & 0x7FFFFFFF)) + k
    return np.array([key if key >= 0 else ((-key) | 0x80000000)], np.uint32).view(f32)[0]


def stale_reference(chk):
    """None when the reference library has the five exports.  A library without them fails the tests wherever the reference tree is present (make rebuilds the
    library from this tree's harness there, so an export is missing or the rebuild did not happen).  Only where there is no reference tree -- a prebuilt library
    nobody can rebuild, which is the same as having none -- the reason to skip is returned"""
    if chk.has_tile_members():
        return None
    assert not orclib.ref_source_available(), "oracle/_ref/liboracle_ref.so lacks ref_tile_tree_map although the reference tree is here to build it from"
    return "the prebuilt oracle/_ref/liboracle_ref.so is from another harness (no ref_tile_tree_map) and there is no reference tree to build this one from"


def tree_scene(chk, scene):
    """the checker put at a scene -> (tree_map_model.Scene from its state, its config)"""
    cfg = orclib.make_config(mesh_gen_mode=0, scene=scene)
    return tmm.Scene(chk.init(cfg), cfg), cfg


def first_diff(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tree map: tile_t::add_tree_ao_shadow
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
FIXTURE_TREE = ("bytes_mixed", "types_r25_v85", "types_r30_v125", "centres_s1_m2000_2000", "radii_s1", "order", "flags_touch_g0", "flags_corner_g1", "flags_touch_g1")
TYPE_CASES = [(25, 85), (25, 170), (31, 175), (37, 175), (30, 125), (30, 250), (33, 75)]
TREE_TILES = [(0, (0, 0)), (1, (40, -40)), (0, (-40, 40)), (1, (-2000, 2000)), (0, (2000, -2000))]  # (scene, tile): +-40 and +-2000 from the origin


def _at(sc, tile, fx, fy):
    return (f32(float(sc.get_xval(tile[0] * S)) + fx * float(sc.DX_VAL)), f32(float(sc.get_yval(tile[1] * S)) + fy * float(sc.DY_VAL)))


def _case(name, scene, tile, splats, prefill=None, hag=False):
    sp = np.ascontiguousarray(np.array(splats, f32).reshape(-1, 3))
    assert np.isfinite(sp).all() and (sp[:, 2] >= 0).all(), name
    pre = np.full((W, W, 2), 255, np.uint8) if prefill is None else np.ascontiguousarray(prefill, np.uint8)
    return dict(name=name, scene=scene, tile=tuple(tile), splats=sp, prefill=pre, hag=bool(hag))


def tree_cases(chk, names=None):
    """-> [dict(name, scene, tile, splats f32 [n, 3], prefill u8 [129, 129, 2], hag)].  names: only these (the fixture's)"""
    out = []
    scs = [tree_scene(chk, s)[0] for s in SCENES]
    sc = scs[0]
    yy, xx = np.mgrid[0:W, 0:W]
    # byte values: every value 0 .. 255 under every (rval, dist_sq) of a centred splat, rval 1 .. 12.  A map holds floor(129 / (2*rval + 1))^2 windows, each
    # prefilled with one value and hit by one splat at its centre; the windows do not overlap
    for r in range(1, 13):
        win = 2 * r + 1
        per = W // win
        nslot = per * per
        for m in range((256 + nslot - 1) // nslot):
            pre = np.full((W, W, 2), 255, np.uint8)
            sp = []
            for v in range(m * nslot, min(256, (m + 1) * nslot)):
                k = v - m * nslot
                ox, oy = (k % per) * win, (k // per) * win
                pre[oy:oy + win, ox:ox + win] = v
                sp.append(_at(sc, (0, 0), ox + r, oy + r) + (f32((r - 0.6) * float(sc.DX_VAL)),))
            out.append(dict(_case(f"bytes_r{r}_{m}", 0, (0, 0), sp, pre), rval=r, values=list(range(m * nslot, min(256, (m + 1) * nslot)))))
    # one map with every rval on a prefill that varies from texel to texel
    pre = np.stack([(xx * 7 + yy * 13) % 256, (xx * 11 + yy * 5 + 3) % 256], -1).astype(np.uint8)
    sp = [_at(sc, (0, 0), 25 * (k % 5) + 12, 25 * (k // 5) + 12) + (f32((1 + k % 12 - 0.6) * float(sc.DX_VAL)),) for k in range(25)]
    out.append(_case("bytes_mixed", 0, (0, 0), sp, pre))
    # the operand types of `float mult(0.2 + 0.8*scale*sqrt(dist_sq))`: up to rval 12 no byte tells the float sqrt from the double one; these (rval, value) tell it, and double
    # products from float ones, at dist_sq 514, 850, 545 (sqrt) and 81, 100, 121 (products).  One centred splat on a map of one value
    for r, v in TYPE_CASES:
        out.append(dict(_case(f"types_r{r}_v{v}", 0, (0, 0), [_at(sc, (0, 0), 64, 64) + (f32((r - 0.6) * float(sc.DX_VAL)),)], np.full((W, W, 2), v, np.uint8)), rval=-r))
    # centres on the round_fp ties (pos - xstart)/DX_VAL = k + 0.5 with their +-1, +-2 ulp siblings, along x, along y and along the diagonal, on and beyond all
    # four borders (rval = 3: the window reaches the tile from k = -4 to k = 131, and clamps to [0, size])
    ks = (-5, -4, -3, -2, -1, 0, 1, 63, 126, 127, 128, 129, 130, 131)
    for si, tile in TREE_TILES:
        s = scs[si]
        sp = []
        for k in ks:
            for j in STEPS:
                x, y = _at(s, tile, k + 0.5, k + 0.5)
                xm, ym = _at(s, tile, 40.25, 77.75)
                sp += [(step(x, j), ym, f32(2.3 * float(s.DX_VAL))), (xm, step(y, j), f32(2.3 * float(s.DX_VAL))), (step(x, j), step(y, -j), f32(2.3 * float(s.DX_VAL)))]
        out.append(_case(f"centres_s{si}_{tile[0]}_{tile[1]}".replace("-", "m"), si, tile, sp))
    # radii on the steps of int(tradius/DX_VAL) and int(tradius/DY_VAL): k*DX_VAL and k*DY_VAL with their +-1, +-2 ulp siblings
    for si in (0, 1):
        s = scs[si]
        sp = []
        for unit in ((s.DX_VAL,) if si == 0 else (s.DX_VAL, s.DY_VAL)):
            for k in range(1, 12):
                for j in STEPS:
                    i = len(sp)
                    sp.append(_at(s, (1, -1), 9.3 + 14 * (i % 9), 8.6 + 9 * (i // 9)) + (step(f32(k) * unit, j),))
        out.append(_case(f"radii_s{si}", si, (1, -1), sp))
    # order: 48 overlapping splats, and the same list backwards (the two results differ: test_tree_map_model_vs_reference asserts it)
    rs = np.random.RandomState(11)
    sp = [_at(sc, (0, 0), 60 + rs.uniform(-9, 9), 70 + rs.uniform(-9, 9)) + (f32(rs.uniform(1.2, 5.9) * float(sc.DX_VAL)),) for _ in range(48)]
    out.append(_case("order", 0, (0, 0), sp))
    out.append(_case("order_reversed", 0, (0, 0), sp[::-1]))
    # flags: a splat far outside (an empty window), one whose window holds texels of which none is within rval (centre (-3, -3), rval 4), one that touches
    for g in (0, 1):
        out.append(_case(f"flags_far_g{g}", 0, (0, 0), [_at(sc, (0, 0), -30.0, 50.0) + (f32(2.3 * float(sc.DX_VAL)),)], hag=g))
        out.append(_case(f"flags_corner_g{g}", 0, (0, 0), [_at(sc, (0, 0), -3.0, -3.0) + (f32(3.4 * float(sc.DX_VAL)),)], hag=g))
        out.append(_case(f"flags_touch_g{g}", 0, (0, 0), [_at(sc, (0, 0), 20.0, 20.0) + (f32(2.3 * float(sc.DX_VAL)),)], hag=g))
    if names is not None:
        out = [c for c in out if c["name"] in names]
        assert len(out) == len(names)
    return out


def ref_tree(chk, cases):
    """-> [(map, (sun_shadows_invalid, moon_shadows_invalid, recalc_tree_grass_weights))] from the reference"""
    out = [None] * len(cases)
    for si, scene in enumerate(SCENES):
        idx = [i for i, c in enumerate(cases) if c["scene"] == si]
        if idx:
            tree_scene(chk, scene)
        for i in idx:
            c = cases[i]
            out[i] = chk.tile_tree_map(c["tile"][0], c["tile"][1], c["splats"], c["prefill"], c["hag"])
    return out


def model_tree(chk, cases):
    """the model; chk supplies the scene constants only -> ([(map, flags)], number of splats the model would skip as undefined)"""
    out, skipped = [None] * len(cases), 0
    for si, scene in enumerate(SCENES):
        idx = [i for i, c in enumerate(cases) if c["scene"] == si]
        if not idx:
            continue
        sc = tree_scene(chk, scene)[0]
        for i in idx:
            c = cases[i]
            tm, upd = c["prefill"].copy(), False
            for x, y, r in c["splats"]:
                p = tmm.splat_params(sc, c["tile"][0], c["tile"][1], 0, 0, x, y, r)
                if p is None:
                    skipped += 1
                else:
                    upd |= bool(tmm.add_tree_ao_shadow(sc, tm, p))
            out[i] = (tm, (upd, upd, upd and c["hag"]))
    return out, skipped


def lib_tree(pkg, t, cases, per_call=4):
    """the library, one to four tiles a call -> [(map, updated)]"""
    out = [None] * len(cases)
    for si, scene in enumerate(SCENES):
        idx = [i for i, c in enumerate(cases) if c["scene"] == si]
        if not idx:
            continue
        t.init_scene(pkg.make_config(mesh_gen_mode=0, scene=scene))
        for k in range(0, len(idx), per_call):
            grp = idx[k:k + per_call]
            first = np.zeros(len(grp) + 1, np.uint32)
            first[1:] = np.cumsum([len(cases[i]["splats"]) for i in grp])
            sp = np.ascontiguousarray(np.concatenate([cases[i]["splats"] for i in grp])).view(tmm.SPLAT_DTYPE).reshape(-1)
            tm = np.ascontiguousarray(np.stack([cases[i]["prefill"] for i in grp]))
            tm, upd = t.tiles_tree_map([cases[i]["tile"] for i in grp], sp, first, reset=False, tree_map=tm)
            for a, i in enumerate(grp):
                out[i] = (tm[a].copy(), bool(upd[a]))
    return out


def compare_tree(what, cases, got, want, flags=True):
    """got / want: [(map, flags or updated)]; flags False: only the first flag of want against got's updated (what the library reports)"""
    for c, g, w in zip(cases, got, want):
        first_diff(f"{what}: tree map {c['name']}", g[0], w[0])
        if flags:
            assert tuple(g[1]) == tuple(w[1]), f"{what}: flags of {c['name']}: {g[1]} != {w[1]}"
        else:
            assert bool(g[1]) == bool(w[1][0]), f"{what}: updated of {c['name']}: {g[1]} != {w[1][0]}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# shadow texture: tile_t::upload_shadow_map_texture
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def light_factors():
    """0; the floats around 0.4 and 0.6 with their +-1, +-2 ulp siblings (the comparisons are against double literals); 33 evenly spaced in [0.4, 0.6]; 1"""
    lf = [f32(0.0)] + [step(f32(0.4), j) for j in STEPS] + [step(f32(0.6), j) for j in STEPS] + [f32(v) for v in np.linspace(0.4, 0.6, 33)] + [f32(1.0)]
    return np.array(lf, f32)


def shadow_inputs(rep):
    """tile `rep` of four: together they hold all 65536 (base_ao, tree ao) pairs; every tile holds all 256 sh values and all 256 mask bytes in either light, and
    all four (sun_en, moon_en) pairs"""
    idx = np.arange(W * W) + rep * W * W
    ao = (idx % 256).astype(np.uint8).reshape(W, W)
    tm = np.stack([(idx // 256) % 256, (idx * 7 + rep) % 256], 1).astype(np.uint8).reshape(W, W, 2)
    zi = np.arange(Z * Z)
    sun = ((zi + 3 * rep) % 256).astype(np.uint8).reshape(Z, Z)
    moon = ((zi // 7 + zi // 256 + rep) % 256).astype(np.uint8).reshape(Z, Z)
    return sun, moon, ao, tm


def shadow_calls():
    """(lf, ground_effects_level, rep, with_masks, with_ao, with_tree_map): every light factor on tile 0 with everything present, and at light factors 0, 0.5 and 1
    all four tiles x ground_effects_level 0 | 1 x AO present | empty x tree map present | empty (at level 0 the masks once present, once empty)"""
    calls = [(lf, 1, 0, True, True, True) for lf in light_factors()]
    for lf in (f32(0.0), f32(0.5), f32(1.0)):
        for rep in range(4):
            for gel in (0, 1):
                for with_ao in (True, False):
                    for with_tm in (True, False):
                        calls.append((lf, gel, rep, bool(gel) or (rep % 2 == 0), with_ao, with_tm))
    return calls


def _shadow_args(call):
    lf, gel, rep, masks, with_ao, with_tm = call
    sun, moon, ao, tm = shadow_inputs(rep)
    return float(lf), int(gel), (sun if masks else None), (moon if masks else None), (ao if with_ao else None), (tm if with_tm else None)


def ref_shadow(chk, call):
    return chk.tile_shadow_texture(*_shadow_args(call))


def model_shadow(call):
    lf, gel, sun, moon, ao, tm = _shadow_args(call)
    n1 = lambda a: None if a is None else a[None]  # noqa: E731
    if sun is None and ao is None and tm is None:  # the model takes the tile count from its inputs
        ao = np.full((W, W), 170, np.uint8)
    return tmm.shadow_texture(S, lf, gel, n1(sun), n1(moon), n1(ao), n1(tm))[0]


def lib_shadow(t, call):
    lf, gel, sun, moon, ao, tm = _shadow_args(call)
    return t.tiles_shadow_texture(1, lf, bool(gel >= 1), sun, moon, ao, tm)[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tree weights: tile_t::create_texture, existing-weights branch
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
PAIR_DIRT = (0, 1, 127, 128, 254, 255)
SAND, DIRT, GRASS, ROCK = tmm.SAND, tmm.DIRT, tmm.GRASS, tmm.ROCK


def weights_pairs():
    """every (tree_ao, grass) pair at every dirt of PAIR_DIRT: 6 * 65536 texels in 24 tiles -> (mesh_weights u8 [24, 129, 129, 4], tree_map u8 [24, 129, 129, 2]);
    the texels beyond the last pair have tree_ao 255 (no trees)"""
    n = len(PAIR_DIRT) * 65536
    nt = (n + W * W - 1) // (W * W)
    k = np.arange(nt * W * W)
    live = k < n
    w = np.zeros((nt * W * W, 4), np.uint8)
    w[:, SAND], w[:, ROCK] = k % 251, (k // 3) % 255  # (rock 255 is a case of its own)
    w[:, DIRT] = np.array(PAIR_DIRT, np.uint8)[np.minimum(k // 65536, len(PAIR_DIRT) - 1)]
    w[:, GRASS] = k % 256
    tm = np.zeros((nt * W * W, 2), np.uint8)
    tm[:, 0] = np.where(live, (k // 256) % 256, 255)
    tm[:, 1] = k % 253
    return w.reshape(nt, W, W, 4), tm.reshape(nt, W, W, 2)


def weights_stride(seed=17, tiles=8):
    """a seeded walk through the rest of the 256^3 (tree_ao, dirt, grass) combinations; every fifth row of the last tile has rock 255 (left alone)"""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 256, (tiles, W, W, 4)).astype(np.uint8)
    w[..., ROCK] = np.minimum(w[..., ROCK], 254)
    w[-1, ::5, :, ROCK] = 255
    tm = rs.randint(0, 256, (tiles, W, W, 2)).astype(np.uint8)
    tm[..., 0][rs.rand(tiles, W, W) < 0.1] = 255
    return w, tm


def ref_weights(chk, w, tm):
    return np.stack([chk.tile_tree_weights(w[i], None if tm is None else tm[i]) for i in range(len(w))])


def lib_weights(t, w, tm, per_call=4):
    return np.concatenate([t.tiles_tree_weights(w[i:i + per_call], None if tm is None else tm[i:i + per_call]) for i in range(0, len(w), per_call)])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# line query: tile_t::line_intersect_mesh, inc_trees = 0
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
LINE_KINDS = ("through", "inside", "face", "xpos tie", "vertical", "horizontal", "under mesh", "row / column size", "distant")
FLAT_TILE, FAR_TILE = (3, 3), (300, -200)
MAX_CELLS = 5000  # a line spans fewer cells than this: tile_t::line_intersect_mesh asserts steps < 10000


def line_scene(chk):
    cfg = orclib.make_config(mesh_gen_mode=0)
    st = chk.init(cfg)
    return lim.Scene(cfg.scene_x, cfg.scene_y, st.DX_VAL, st.DY_VAL, st.DX_VAL_INV, st.DY_VAL_INV, S)


def line_tiles(chk):
    """three generated tiles -- the one with the most water cells, the steepest, one far from the origin -- and a flat one
    -> (tiles int32 [4, 2], zvals f32 [4, 130, 130], mz f32 [4, 2] = mzmin, mzmax)"""
    cand = {}
    for ty in range(-3, 4):
        for tx in range(-3, 4):
            z, st = chk.tile_create_zvals(tx, ty, 0)
            water = max(0, st.wx2 - st.wx1) * max(0, st.wy2 - st.wy1)
            cand[(tx, ty)] = (z, st.mzmin, st.mzmax, water)
    wet = [k for k, v in cand.items() if 0 < v[3] < S * S]
    assert wet, "no candidate tile has both water and land"
    water_tile = max(wet, key=lambda k: (cand[k][3], k))
    steep_tile = max((k for k in cand if k != water_tile), key=lambda k: (cand[k][2] - cand[k][1], k))
    zf, stf = chk.tile_create_zvals(FAR_TILE[0], FAR_TILE[1], 0)
    tiles = [water_tile, steep_tile, FAR_TILE, FLAT_TILE]
    z = np.stack([cand[water_tile][0], cand[steep_tile][0], zf, np.full((Z, Z), 0.75, f32)]).astype(f32)
    mz = np.array([cand[water_tile][1:3], cand[steep_tile][1:3], (stf.mzmin, stf.mzmax), (0.75, 0.75)], f32)
    return np.array(tiles, np.int32), z, mz


class LineRows:
    def __init__(self):
        self.rows, self.kind, self.tile, self.groups = [], [], [], []

    def add(self, kind, tile, v1, v2):
        self.rows.append(np.concatenate([np.asarray(v1, np.float64), np.asarray(v2, np.float64)]).astype(f32))
        self.kind.append(kind); self.tile.append(tile)

    def group(self, kind, tile, v1, v2, cols):
        """the row and its +-1, +-2 ulp siblings: the columns `cols` of (v1, v2) move together"""
        self.groups.append((kind, len(self.rows), len(STEPS)))
        base = np.concatenate([np.asarray(v1, np.float64), np.asarray(v2, np.float64)]).astype(f32)
        for j in STEPS:
            q = base.copy()
            for c in cols:
                q[c] = step(base[c], j)
            self.add(kind, tile, q[:3], q[3:])


def line_rows(sc, tiles, z, mz, seed=23):
    """-> (rows f32 [n, 6], kind i32 [n], tile i32 [n], groups i32 [g, 3] = kind, first row, rows).  Kind 8 rows go to their tile as a distant one"""
    rs = np.random.RandomState(seed)
    r = LineRows()
    DX, DY = float(sc.DX_VAL), float(sc.DY_VAL)
    for i, (tx, ty) in enumerate(tiles):
        d, _, _ = lim.mesh_bcube(sc, np.array([tx]), np.array([ty]), mz[i:i + 1, 0], mz[i:i + 1, 1], 0, 0)
        d = [float(a[0]) for a in d]  # x1 x2 y1 y2 z1 z2
        zlo, zhi = float(mz[i, 0]), float(mz[i, 1])
        span = max(zhi - zlo, 0.5)

        def cell(ix, iy):
            return d[0] + ix * DX, d[2] + iy * DY, float(z[i, int(iy), int(ix)])

        def inside(zfrac=None):
            return np.array([rs.uniform(d[0], d[1]), rs.uniform(d[2], d[3]), zlo + (zhi - zlo) * (rs.uniform(0, 1) if zfrac is None else zfrac)])

        def downward():
            p, yaw = np.radians(rs.uniform(-85.0, -3.0)), rs.uniform(0.0, 2 * np.pi)
            return np.array([np.cos(p) * np.cos(yaw), np.cos(p) * np.sin(yaw), np.sin(p)])

        for k in range(70):  # through and past the tile: a ray toward a terrain point (or, every fourth, away from the ground), 60 units long
            x, y, zv = cell(rs.randint(0, W), rs.randint(0, W))
            dirv = downward()
            if k % 4 == 3:
                dirv[2] = -dirv[2]
            v1 = np.array([x, y, zv]) - dirv * rs.uniform(0.5, 40.0) * (1.0 if k % 4 != 3 else -0.02)
            r.add(0, i, v1, v1 + dirv * 60.0)
        for k in range(50):  # both ends inside the box
            r.add(1, i, inside(), inside())
        for a in range(3):  # an end on each face of get_mesh_bcube(), the other end inside
            for side in range(2):
                for k in range(6):
                    v1, v2 = inside(0.9 if a < 2 else None), inside(0.1 if a < 2 else None)
                    v1[a] = d[2 * a + side]
                    if a == 2:
                        v2[2] = d[4 + (1 - side)] + (0.5 * span if side == 0 else -0.5 * span)  # from the bottom face upward / from the top face downward
                    if k < 4:
                        r.group(2, i, v1, v2, [a])
                    else:
                        r.group(2, i, v2, v1, [3 + a])  # the line ends on the face
        for k in range(20):  # an end whose x (or y) is a get_xpos tie: (x + X_SCENE_SIZE)*DX_VAL_INV + 0.5 an integer
            ix, iy = rs.randint(1, S - 1), rs.randint(1, S - 1)
            x, y, zv = cell(ix, iy)
            v1 = np.array([x + 0.5 * DX if k % 2 == 0 else x + rs.uniform(0.1, 0.9) * DX, y + 0.5 * DY if k % 2 else y + rs.uniform(0.1, 0.9) * DY, min(zhi, zv + rs.uniform(0.02, 0.2) * span)])
            v2 = np.array([v1[0] + rs.uniform(-6, 6) * DX, v1[1] + rs.uniform(-6, 6) * DY, zlo - 0.5 * span])
            if k < 14:
                r.group(3, i, v1, v2, [k % 2])
            else:
                r.group(3, i, v2, v1, [3 + k % 2])
        for k in range(30):  # vertical: steps = 1
            x, y, zv = cell(rs.randint(0, W), rs.randint(0, W))
            x, y = x + (rs.uniform(0, 1) * DX if k % 3 else 0.0), y + (rs.uniform(0, 1) * DY if k % 3 else 0.0)
            a, b = zv + rs.uniform(0.1, 5.0), zv - rs.uniform(0.1, 5.0)
            r.add(4, i, [x, y, a if k % 2 == 0 else b], [x, y, b if k % 2 == 0 else a])
        for k in range(30):  # horizontal: v1.z == v2.z, the quotient's denominator is zero
            x, y, zv = cell(rs.randint(0, W), rs.randint(0, W))
            zz = zv - rs.uniform(0.0, 0.1) * span if k % 2 else zv + rs.uniform(0.0, 0.1) * span
            r.add(5, i, [x, y, zz], [x + rs.uniform(-30, 30), y + rs.uniform(-30, 30), zz])
        for k in range(30):  # the line starts under the mesh
            x, y, zv = cell(rs.randint(0, W), rs.randint(0, W))
            v1 = np.array([x, y, zv - rs.uniform(0.01, 0.3)])
            r.add(6, i, v1, v1 + rs.normal(size=3) * rs.uniform(1.0, 30.0))
        for k in range(24):  # along row and column `size`, on them and one ulp inside
            xe, ye = d[1], d[3]
            if k % 2:
                xe, ye = float(step(f32(xe), -1 if xe > 0 else 1)), float(step(f32(ye), -1 if ye > 0 else 1))
            t0 = rs.uniform(0, 100)
            if k % 4 < 2:
                r.add(7, i, [xe, d[2] + t0 * DY, zhi + 0.3 * span], [xe, d[2] + (t0 + rs.uniform(5, 28)) * DY, zlo - 0.3 * span])
            else:
                r.add(7, i, [d[0] + t0 * DX, ye, zhi + 0.3 * span], [d[0] + (t0 + rs.uniform(5, 28)) * DX, ye, zlo - 0.3 * span])
    n0 = len(r.rows)
    for k in range(0, n0, 29):  # a distant tile: the member returns 0 before it looks at the line
        r.rows.append(r.rows[k].copy()); r.kind.append(8); r.tile.append(r.tile[k])
    rows = np.stack(r.rows).astype(f32)
    assert np.isfinite(rows).all(), "a non-finite row would make the reference assert"
    assert (np.abs(rows[:, 3] - rows[:, 0]) < MAX_CELLS * DX).all() and (np.abs(rows[:, 4] - rows[:, 1]) < MAX_CELLS * DY).all(), "steps < 10000"
    return rows, np.array(r.kind, np.int32), np.array(r.tile, np.int32), np.array(r.groups, np.int32)


def line_rows_undefined(sc, rows):
    """the rows at which tile_t::line_intersect_mesh asserts (a non-finite end, or a walk of 10000 steps or more: here, conservatively, any line that spans
    MAX_CELLS cells) -> their number"""
    rows = np.asarray(rows, f32).reshape(-1, 6)
    bad = ~np.isfinite(rows).all(axis=1)
    with np.errstate(invalid="ignore"):
        bad |= ~(np.abs(rows[:, 3] - rows[:, 0]) < MAX_CELLS * float(sc.DX_VAL)) | ~(np.abs(rows[:, 4] - rows[:, 1]) < MAX_CELLS * float(sc.DY_VAL))
    return int(bad.sum())


def _line_sets(kind, tile, ntiles):
    for i in range(ntiles):
        for distant in (False, True):
            sel = np.nonzero((tile == i) & ((kind == 8) == distant))[0]
            if len(sel):
                yield i, distant, sel


def ref_lines(chk, tiles, z, mz, rows, kind, tile):
    """-> orclib.LINE_REF_DTYPE [n] (the checker's scene is line_scene's)"""
    out = np.zeros(len(rows), orclib.LINE_REF_DTYPE)
    for i, distant, sel in _line_sets(kind, tile, len(tiles)):
        out[sel] = chk.tile_line_intersect(int(tiles[i][0]), int(tiles[i][1]), z[i], float(mz[i, 0]), float(mz[i, 1]), rows[sel].reshape(-1, 2, 3), distant)
    return out


def model_lines(sc, tiles, z, mz, rows, kind, tile):
    out = np.zeros(len(rows), orclib.LINE_REF_DTYPE)
    out["t"] = 1.0
    for i, distant, sel in _line_sets(kind, tile, len(tiles)):
        h = lim.batch_hits(sc, [tuple(tiles[i])], z[i:i + 1], mz[i:i + 1, 0], mz[i:i + 1, 1], rows[sel].reshape(-1, 2, 3), distant=[distant])
        hit = h["hit"] == 1
        o = out[sel]
        o["hit"] = hit
        o["t"], o["xpos"], o["ypos"] = np.where(hit, h["t"], f32(1.0)), np.where(hit, h["xpos"], 0), np.where(hit, h["ypos"], 0)
        out[sel] = o
    return out


def lib_stats(pkg, mz, radius):
    st = (pkg.TileStats * len(mz))()
    for i in range(len(mz)):
        st[i].mzmin, st[i].mzmax, st[i].radius = float(mz[i, 0]), float(mz[i, 1]), float(radius)
    return st


def lib_lines(pkg, t, tiles, z, mz, rows, kind, tile, together=False):
    """the library: one batch of lines per tile, the tile alone in the call; together: all four tiles in one call, every line bound to its tile (the distant rows
    in a call of their own, their tiles flagged)"""
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    out = np.zeros(len(rows), orclib.LINE_REF_DTYPE)
    out["t"] = 1.0
    sets = []
    if together:
        for distant in (False, True):
            sel = np.nonzero((kind == 8) == distant)[0]
            sets.append((np.arange(len(tiles)), distant, sel, tile[sel]))
    else:
        sets = [(np.array([i]), distant, sel, None) for i, distant, sel in _line_sets(kind, tile, len(tiles))]
    for ti, distant, sel, lt in sets:
        st = lib_stats(pkg, mz[ti], 0.0)
        h = t.tiles_line_intersect(tiles[ti], z[ti], st, rows[sel].reshape(-1, 2, 3), lt, 0, 0, np.full(len(ti), int(distant), np.uint8))
        hit = h["hit"] == 1
        if lt is not None:
            assert (h["tile"][hit] == lt[hit]).all()
        o = out[sel]
        o["hit"] = hit
        o["t"], o["xpos"], o["ypos"] = np.where(hit, h["t"], f32(1.0)), np.where(hit, h["xpos"], 0), np.where(hit, h["ypos"], 0)
        out[sel] = o
    return out


def compare_lines(what, got, want, kind):
    bad = np.nonzero(got.view(np.uint8).reshape(len(got), -1).__ne__(want.view(np.uint8).reshape(len(want), -1)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rows differ, first row {bad[0]} ({LINE_KINDS[kind[bad[0]]]}): {got[bad[0]]} != {want[bad[0]]}"


def line_tallies(ref_out, kind, groups):
    """the tallies the generator prints and asserts -> (lines of text, {kind: (groups, groups inside which the reference's answer changes)})"""
    hit = ref_out["hit"] != 0
    text = [f"{len(kind)} line rows: " + ", ".join(f"{LINE_KINDS[k]} {int((kind == k).sum())}" for k in range(len(LINE_KINDS))),
            f"hits {int(hit.sum())} ({100 * hit.mean():.1f} %), misses {int((~hit).sum())} ({100 * (1 - hit.mean()):.1f} %)"]
    by_kind = {}
    key = ref_out.view(np.uint8).reshape(len(ref_out), -1)
    for k, first, n in groups:
        f = by_kind.setdefault(int(k), [0, 0])
        f[0] += 1
        f[1] += int((key[first:first + n] != key[first]).any())
    for k, (n, f) in sorted(by_kind.items()):
        text.append(f"  +-ulp groups, {LINE_KINDS[k]:9s} {n:4d} groups, the reference's answer changes inside {f:4d} ({100 * f / n:5.1f} %)")
    return text, by_kind


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# grass brush: tile_t::add_or_remove_grass_at
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
GRASS_TILE = (1, 0)  # beside it a second tile, found by grass_tiles: synthetic zvals, a ramp that rises through every texture layer, snow included
STROKE_DTYPE = np.dtype([("tile", np.int32), ("prep", np.int32), ("pos", np.float32, (3,)), ("radius", np.float32), ("add", np.int32), ("shape", np.int32),
                         ("weight", np.float32), ("flowers", np.int32), ("hag", np.int32)])
PREPS = ("as generated", "grassy", "balance", "random bytes", "no blocks", "last grass")


def grass_landscape():
    return dict(grass_density=1, enable_terrain_env=1)


def grass_scene(chk):
    """scene + landscape of the grass strokes on a checker -> grass_brush_model.Scene (callers put the landscape back: chk.set_landscape(orclib.make_landscape()))"""
    cfg = orclib.make_config(mesh_gen_mode=0)
    chk.init(cfg)
    ls = orclib.make_landscape(**grass_landscape())
    chk.set_landscape(ls)
    return gbm.Scene(chk, cfg, ls)


def grass_tiles(chk):
    """(call after grass_scene) -> dict(tiles, z [2, 130, 130], mz [2, 2], radius [2], w [2, 129, 129, 4], gb [2, 32, 32], params [2, 2, 2, 3]) from the reference's own
    create_zvals / create_texture / update_terrain_params; tile 1's zvals are a ramp from zmin to zmax along x with a ripple along y"""
    st0 = chk.state()
    # the ramp's tile: the first, going outward, with a corner whose dirt parameter lies strictly between 0 and 1 (dirt_scale < 1: dirt becomes sand)
    ring = sorted(((tx, ty) for ty in range(-12, 13) for tx in range(-12, 13)), key=lambda k: (max(abs(k[0]), abs(k[1])), k))
    ramp_tile = next(k for k in ring if k != GRASS_TILE and ((lambda p: ((p > 0) & (p < 1)).any())(chk.tile_terrain_params(k[0], k[1])[..., 2])))
    tiles = [GRASS_TILE, ramp_tile]
    z0, st = chk.tile_create_zvals(GRASS_TILE[0], GRASS_TILE[1], 0)
    yy, xx = np.mgrid[0:Z, 0:Z]
    ramp = (float(st0.zmin) + (float(st0.zmax) - float(st0.zmin)) * (xx + 0.4 * np.sin(yy * 0.7)) / float(Z)).astype(f32)
    z = np.stack([z0, ramp]).astype(f32)
    mz = np.array([(st.mzmin, st.mzmax), (ramp.min(), ramp.max())], f32)
    w, gb = np.zeros((2, W, W, 4), np.uint8), np.zeros((2, 32, 32), orclib.GRASS_BLOCK_DTYPE)
    params = np.zeros((2, 2, 2, 3), f32)
    for i, (tx, ty) in enumerate(tiles):
        w[i], gb[i], _ = chk.tile_create_weights(tx, ty, z[i])
        params[i] = chk.tile_terrain_params(tx, ty)
    # the radius create_zvals leaves (src/tiled_mesh.cpp:541); the ramp's from the same statement over its own z range (an input like the zvals)
    radius = np.array([st.radius, 0.5 * np.sqrt((float(st0.DX_VAL) ** 2 + float(st0.DY_VAL) ** 2) * S * S + float(mz[1, 1] - mz[1, 0]) ** 2)], f32)
    return dict(tiles=np.array(tiles, np.int32), z=z, mz=mz, radius=radius, w=w, gb=gb, params=params)


def prepared(d, i, prep):
    """the weights and blocks of tile i as stroke input -> (w u8 [129, 129, 4], gb [32, 32])"""
    w, gb = d["w"][i].copy(), d["gb"][i].copy()
    yy, xx = np.mgrid[0:W, 0:W]
    if prep == 1:  # grass of every amount, 0 and 255 included
        w[..., GRASS] = (37 * xx + 11 * yy) % 256
    elif prep == 2:  # small other layers under a partial addition: the balancing loop empties one, two and three of them
        w[..., SAND], w[..., DIRT], w[..., ROCK], w[..., GRASS] = xx % 8, yy % 8, (xx + yy) % 8, 100 + xx % 3
    elif prep == 3:  # bytes that wrap the unsigned char sums
        rs = np.random.RandomState(7)
        w[...] = rs.randint(0, 256, w.shape)
        w[::3, ::2, SAND] = 250; w[::2, ::3, DIRT] = 251
    elif prep == 4:  # a tile without a grass block: the stroke adds its first
        gb[...] = np.zeros((), orclib.GRASS_BLOCK_DTYPE)
        w[..., GRASS] = 0
    elif prep == 5:  # grass on a few texels only, blocks present: the stroke removes the last
        w[..., GRASS] = 0
        w[60:64, 60:64, GRASS] = 9
        gb[...] = np.zeros((), orclib.GRASS_BLOCK_DTYPE)
        gb[15, 15] = (3, -1.0, 1.0)
    return w, gb


def grass_strokes(sc, d):
    """-> STROKE_DTYPE [n]"""
    DX = float(sc.DX_VAL)
    rows = []

    def at(i, ix, iy, dz=0.0):
        tx, ty = (int(v) for v in d["tiles"][i])
        return (float(sc.get_xval(tx * S + ix)), float(sc.get_yval(ty * S + iy)), float(d["z"][i][iy, ix]) + dz)

    def add(i, prep, pos, radius, add_grass, shape, weight, flowers=None):
        rows.append((i, prep, pos, radius, add_grass, shape, weight, (not add_grass) if flowers is None else flowers, len(rows) % 2))

    for i, (cx, cy) in ((0, (40, 50)), (1, (70, 64))):
        for shape in range(8):  # all eight shapes, add and remove; weight 0.12: the decaying shapes cross delta = 0.99 and 0.01 between the centre and the rim
            add(i, 0, at(i, cx, cy), 9.5 * DX, 1, shape, 0.12)
            add(i, 1, at(i, cx, cy), 9.5 * DX, 0, shape, 0.12)
        for k in range(10):  # brush weights 0.001 .. 0.512
            wgt = 0.001 * 2 ** k
            add(i, 0, at(i, cx + 3, cy - 2), 6.5 * DX, 1, gbm.BSHAPE_CNST_CIR if k % 2 else gbm.BSHAPE_LINEAR, wgt)
            add(i, 1, at(i, cx + 3, cy - 2), 6.5 * DX, 0, gbm.BSHAPE_CNST_CIR if k % 2 else gbm.BSHAPE_LINEAR, wgt)
        for prep, add_grass, shape, wgt in ((2, 1, gbm.BSHAPE_CNST_CIR, 0.005), (2, 1, gbm.BSHAPE_COSINE, 0.008), (3, 0, gbm.BSHAPE_LINEAR, 0.06), (3, 0, gbm.BSHAPE_CNST_CIR, 0.3),
                                            (3, 1, gbm.BSHAPE_SINE, 0.05), (3, 1, gbm.BSHAPE_CONST_SQ, 0.2), (4, 1, gbm.BSHAPE_QUADRATIC, 0.03), (5, 0, gbm.BSHAPE_CONST_SQ, 1.0)):
            add(i, prep, at(i, 62, 62), 12.5 * DX, add_grass, shape, wgt)
        # centres on a texel, the radius a whole number of cells with its +-1, +-2 ulp siblings: fabs(pt.x - pos.x) > rradius and dist < rradius on their ties
        for j in STEPS:
            add(i, 0, at(i, 30, 90), float(step(f32(5.0 * DX), j)), 1, gbm.BSHAPE_CONST_SQ, 0.2)
            add(i, 1, at(i, 30, 90), float(step(f32(5.0 * DX), j)), 0, gbm.BSHAPE_CNST_CIR, 0.2)
        add(i, 0, at(i, 127, 127), 3.5 * DX, 1, gbm.BSHAPE_CONST_SQ, 0.06)  # row and column 128: edited, no grass block, the range clamped to size
        add(i, 1, at(i, 0, 0), 4.5 * DX, 0, gbm.BSHAPE_CNST_CIR, 0.06, flowers=False)  # a removal on a tile without flowers: no clear_within
        add(i, 1, at(i, 64, 64), 400.0 * DX, 0, gbm.BSHAPE_CONST_SQ, 1.0)  # everything removed: the blocks are cleared
        add(i, 0, at(i, cx, cy), 0.0, 1, gbm.BSHAPE_CNST_CIR, 0.05)  # radius 0
        add(i, 0, at(i, cx, cy, 50.0), 9.5 * DX, 1, gbm.BSHAPE_CNST_CIR, 0.05)  # a sphere that misses the tile
        # centres off the lattice (seeded fractions of a cell), every shape: dist, sqrt(dist)*r_inv and the shape functions away from the lattice distances; and the
        # half-cell siblings of a centre, where fabs(pt.x - pos.x) > rradius and dist < rradius*rradius meet their ties at a radius of k + 0.5 cells
        rs = np.random.RandomState(41 + i)
        for shape in range(8):
            for add_grass in (1, 0):
                x, y, zz = at(i, 20 + 11 * shape, 100)
                add(i, 1 - add_grass, (x + rs.uniform(0.05, 0.95) * DX, y + rs.uniform(0.05, 0.95) * float(sc.DY_VAL), zz), rs.uniform(3.0, 8.0) * DX, add_grass, shape,
                    float(rs.choice([0.03, 0.08, 0.12])))
        x, y, zz = at(i, 90, 30)
        for j in STEPS:
            add(i, 0, (float(step(f32(x + 0.5 * DX), j)), y, zz), 4.5 * DX, 1, gbm.BSHAPE_CONST_SQ, 0.2)
            add(i, 1, (float(step(f32(x + 0.5 * DX), j)), float(step(f32(y + 0.5 * float(sc.DY_VAL)), -j)), zz), 4.5 * DX, 0, gbm.BSHAPE_CNST_CIR, 0.2)
        # mesh_sphere_intersect on its ties: a sphere that just reaches the low corner of the tile's box along the diagonal from the tile's centre, where both
        # dist_less_than(pos, get_center(), radius + rradius) and sphere_cube_intersect decide; 0.1 % inside and outside, and +-1, +-2 ulp in z
        cx0, cy0, _ = at(i, 0, 0)
        cz0 = float(d["mz"][i, 0]) - 1.0e-6
        diag = np.array([-64.0 * DX, -64.0 * float(sc.DY_VAL), cz0 - 0.5 * float(d["mz"][i, 0] + d["mz"][i, 1])])
        diag /= np.sqrt((diag * diag).sum())
        rr = 2.5 * DX
        for scale, j in [(0.999, 0), (1.001, 0)] + [(1.0, j) for j in STEPS]:
            p = np.array([cx0, cy0, cz0]) + diag * rr * scale
            add(i, 0, (float(p[0]), float(p[1]), float(step(f32(p[2]), j))), rr, 1, gbm.BSHAPE_CONST_SQ, 0.2)
    # the ramp tile: a removal along the whole ramp, every layer (k1 / k2 on sand .. snow) under one stroke, and a wide band at each brush kind
    add(1, 1, at(1, 64, 64), 70.0 * DX, 0, gbm.BSHAPE_CONST_SQ, 0.02)
    add(1, 1, at(1, 64, 20), 66.0 * DX, 0, gbm.BSHAPE_QUADRATIC, 0.05)
    out = np.zeros(len(rows), STROKE_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["radius"]).all()
    return out


def ref_stroke(chk, d, s):
    """-> (returned, weights, blocks, has_any_grass, orclib.FlowerCalls)"""
    i = int(s["tile"])
    w, gb = prepared(d, i, int(s["prep"]))
    return chk.tile_grass_brush(int(d["tiles"][i][0]), int(d["tiles"][i][1]), d["z"][i], float(d["mz"][i, 0]), float(d["mz"][i, 1]), float(d["radius"][i]), w, gb, s["pos"], float(s["radius"]),
                                int(s["add"]), int(s["shape"]), float(s["weight"]), bool(s["hag"]), bool(s["flowers"]))


class _Stats:
    def __init__(self, mzmin, mzmax, radius):
        self.mzmin, self.mzmax, self.radius = mzmin, mzmax, radius


def expected_calls(sc, tile, s, updated, rng):
    """what add_or_remove_grass_at hands the flowers for a stroke that returned `updated` with the add range rng = (xl, yl, xh, yh) -> FlowerCalls.as_tuple()'s
    form.  update_subrange(weight_data, stride, x1 - xoff2, y1 - yoff2, xl, yl, xh, yh) (src/tiled_mesh.cpp:3932); clear_within(pos - flower_xlate, rradius,
    is_square) with flower_xlate = (get_xval(x1 + xoff - xoff2), get_yval(y1 + yoff - yoff2), 0) (:3935-3936), the subtraction in float as tests/flower_model.py's"""
    none = (0, 0, 0, 0, 0, 0, 0, 0, 0, (0.0, 0.0, 0.0), 0.0, 0)
    if not updated:
        return none
    tx, ty = int(tile[0]), int(tile[1])
    if s["add"]:
        return (1, 0, W, tx * S, ty * S) + tuple(int(v) for v in rng) + ((0.0, 0.0, 0.0), 0.0, 0)
    if not s["flowers"]:
        return none
    pos = tuple(float(f32(a) - b) for a, b in zip(s["pos"], (sc.get_xval(tx * S), sc.get_yval(ty * S), f32(0.0))))
    return (0, 1, 0, 0, 0, 0, 0, 0, 0, pos, float(f32(s["radius"])), int(s["shape"] == gbm.BSHAPE_CONST_SQ))


def model_stroke(sc, d, s):
    """-> (returned, weights, blocks, has_any_grass, expected flower calls as a tuple)"""
    i = int(s["tile"])
    w, gb = prepared(d, i, int(s["prep"]))
    tx, ty = (int(v) for v in d["tiles"][i])
    upd, rng = gbm.add_or_remove_grass_at(sc, tx, ty, d["z"][i], _Stats(d["mz"][i, 0], d["mz"][i, 1], d["radius"][i]), w, gb, d["params"][i], tuple(s["pos"]), s["radius"],
                                          bool(s["add"]), int(s["shape"]), s["weight"])
    return bool(upd), w, gb, bool(s["hag"]), expected_calls(sc, (tx, ty), s, upd, rng)


def lib_stroke(pkg, t, d, s):
    """one stroke, one tile, one call (the scene and landscape are the caller's: lib_grass_setup) -> (updated, weights, blocks, range)"""
    i = int(s["tile"])
    w, gb = prepared(d, i, int(s["prep"]))
    w, gb = np.ascontiguousarray(w[None]), np.ascontiguousarray(gb[None])
    st = lib_stats(pkg, d["mz"][i:i + 1], d["radius"][i])
    brush = pkg.make_grass_brush(tuple(float(v) for v in s["pos"]), float(s["radius"]), int(s["add"]), int(s["shape"]), float(s["weight"]))
    upd, rg = t.tiles_edit_grass(d["tiles"][i:i + 1], d["z"][i:i + 1], st, brush, w, gb)
    return bool(upd[0]), w[0], gb[0], tuple(int(v) for v in rg[0])


def lib_grass_setup(pkg, t):
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    t.set_landscape(pkg.make_landscape(**grass_landscape()))


def compare_stroke(what, got, want):
    """(returned, weights, blocks, ...) of two sides"""
    assert got[0] == want[0], f"{what}: returned {got[0]} != {want[0]}"
    first_diff(f"{what}: weights", got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes(), f"{what}: grass blocks differ at {np.argwhere(got[2].view(np.uint8) != want[2].view(np.uint8))[:4].tolist()}"


def texel_tids(sc, z):
    """get_tids of every texel of a tile as the removal branch calls it (src/tiled_mesh.cpp:3911: relh of the texel's mhmax) -> (snow, grass, blend) bool [129, 129]"""
    dz_inv = f32(f32(1.0) / f32(sc.zmax - sc.zmin))
    out = np.zeros((3, W, W), bool)
    for y in range(W):
        for x in range(W):
            k1, k2, t = sc.get_tids(f32(sc.relh_adj_tex + f32(f32(z[y:y + 2, x:x + 2].max() - sc.zmin) * dz_inv)))
            out[:, y, x] = (k1 >= 4 or k2 >= 4, gbm.GRASS in (k1, k2), t is not None)
    return out


def texel_dirt_scale(params):
    """BILINEAR_INTERP(params, dirt, x*xy_mult, y*xy_mult) of every texel (:3917), in float as tests/grass_brush_model.py evaluates it -> f32 [129, 129]"""
    xy_mult = f32(1.0 / float(f32(S)))
    fy, fx = np.meshgrid((np.arange(W).astype(f32) * xy_mult).astype(f32), (np.arange(W).astype(f32) * xy_mult).astype(f32), indexing="ij")
    p, one = np.asarray(params, f32)[:, :, 2], f32(1.0)
    return (fy * (fx * p[1, 1] + (one - fx) * p[1, 0]) + (one - fy) * (fx * p[0, 1] + (one - fx) * p[0, 0])).astype(f32)


def grass_tallies(sc, d, strokes, results):
    """what the strokes reach, from the reference's results [(returned, weights, blocks, ..)] -> dict: texels of a partial addition at which the balancing loop
    emptied 1 / 2 / 3 layers; strokes that gave a tile its first block / took its last; and, counted over the texels the removal strokes changed, those whose
    get_tids lands on snow, on grass and in a blend, and those with dirt_scale < 1 (dirt becomes sand); strokes
    that returned 1 from a centre off the texel lattice; and the spheres placed at the low corner of the box that mesh_sphere_intersect accepts and rejects"""
    tally = dict(emptied=[0, 0, 0, 0], first_block=0, last_block=0, grass0=0, grass255=0, partial_add=0, full_add=0, snow=0, grass_tid=0, blend=0, dirt_to_sand=0,
                 off_lattice=0, corner_hit=0, corner_miss=0)
    tids = [texel_tids(sc, d["z"][i]) for i in range(len(d["tiles"]))]
    dirt = [texel_dirt_scale(d["params"][i]) for i in range(len(d["tiles"]))]
    for s, r in zip(strokes, results):
        i = int(s["tile"])
        w0, gb0 = prepared(d, i, int(s["prep"]))
        changed = (w0 != r[1]).any(axis=-1)
        if s["add"] and r[0]:
            partial = changed & (r[1][..., GRASS] < 255)
            n = sum(((w0[..., c] > 0) & (r[1][..., c] == 0)).astype(int) for c in (SAND, DIRT, ROCK))
            for k in range(4):
                tally["emptied"][k] += int((n[partial] == k).sum())
            tally["partial_add"] += int(partial.sum()); tally["full_add"] += int((changed & (r[1][..., GRASS] == 255)).sum())
        if not s["add"]:
            tally["snow"] += int((changed & tids[i][0]).sum()); tally["grass_tid"] += int((changed & tids[i][1]).sum()); tally["blend"] += int((changed & tids[i][2]).sum())
            tally["dirt_to_sand"] += int((changed & (dirt[i] < f32(1.0))).sum())
        tally["grass0"] += int((changed & (w0[..., GRASS] == 0)).sum()); tally["grass255"] += int((changed & (w0[..., GRASS] == 255)).sum())
        tally["first_block"] += int(not gb0["ix"].any() and r[2]["ix"].any()); tally["last_block"] += int(gb0["ix"].any() and not r[2]["ix"].any())
        tx, ty = (int(v) for v in d["tiles"][i])
        fx = (float(s["pos"][0]) - float(sc.get_xval(tx * S))) / float(sc.DX_VAL)
        tally["off_lattice"] += int(r[0] and abs(fx - round(fx)) > 0.01)
        if fx < 0 and float(s["pos"][1]) < float(sc.get_yval(ty * S)) and float(s["pos"][2]) < float(d["mz"][i, 0]):  # the spheres beyond the low corner
            tally["corner_hit" if r[0] else "corner_miss"] += 1
    return tally


def check_grass_tallies(tally):
    assert min(tally["emptied"][1:]) > 0, tally  # the balancing loop empties one, two and three layers
    assert tally["first_block"] > 0 and tally["last_block"] > 0 and tally["grass0"] > 0 and tally["grass255"] > 0 and tally["partial_add"] > 0 and tally["full_add"] > 0, tally
    assert tally["snow"] > 0 and tally["grass_tid"] > 0 and tally["blend"] > 0 and tally["dirt_to_sand"] > 0 and tally["off_lattice"] >= 20, tally
    assert tally["corner_hit"] > 0 and tally["corner_miss"] > 0, tally  # mesh_sphere_intersect answers both ways around its tie


def calls_equal(calls, want):
    """orclib.FlowerCalls against expected_calls' tuple: integers equal, floats bit for bit"""
    g = calls.as_tuple() if hasattr(calls, "as_tuple") else tuple(calls)
    return g[:9] == tuple(want[:9]) and np.array(g[9] + (g[10],), f32).tobytes() == np.array(tuple(want[9]) + (want[10],), f32).tobytes() and g[11] == want[11]


def stroke_range(calls):
    """the range a stroke leaves for the flowers as the library reports it: update_subrange's (xl, yl, xh, yh), or the denormalized (size, size, 0, 0)"""
    c = calls.as_tuple() if hasattr(calls, "as_tuple") else tuple(calls)
    return tuple(c[5:9]) if c[0] else (S, S, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the device entry points (terra_tiles_*_dev) on buffers of the library's own allocator: the emulator's "device" memory or the GPU's
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class Bufs:
    """device buffers of one call, freed together"""

    def __init__(self, t):
        self.t, self.all = t, []

    def new(self, nbytes):
        self.all.append(self.t.alloc(max(int(nbytes), 4)))
        return self.all[-1]

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.new(arr.nbytes).upload(arr)

    def ptr(self, arr):
        return None if arr is None else self.up(arr).ptr

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.all:
            b.free()


def dev_tree(pkg, t, cases, per_call=4):
    """lib_tree through terra_tiles_tree_map_dev"""
    out = [None] * len(cases)
    for si, scene in enumerate(SCENES):
        idx = [i for i, c in enumerate(cases) if c["scene"] == si]
        if not idx:
            continue
        t.init_scene(pkg.make_config(mesh_gen_mode=0, scene=scene))
        for k in range(0, len(idx), per_call):
            grp = idx[k:k + per_call]
            first = np.zeros(len(grp) + 1, np.uint32)
            first[1:] = np.cumsum([len(cases[i]["splats"]) for i in grp])
            with Bufs(t) as b:
                sb = b.up(np.concatenate([cases[i]["splats"] for i in grp]))
                mb = b.up(np.stack([cases[i]["prefill"] for i in grp]))
                ub = b.up(np.full(len(grp), 7, np.uint8))
                t.tiles_tree_map_dev([cases[i]["tile"] for i in grp], sb.ptr, first, mb.ptr, ub.ptr, False)
                tm, upd = mb.download(np.uint8, (len(grp), W, W, 2)), ub.download(np.uint8, (len(grp),))
            assert ((upd == 0) | (upd == 1)).all()
            for a, i in enumerate(grp):
                out[i] = (tm[a].copy(), bool(upd[a]))
    return out


def dev_shadow(t, call):
    lf, gel, sun, moon, ao, tm = _shadow_args(call)
    with Bufs(t) as b:
        ob = b.new(W * W * 4)
        t.tiles_shadow_texture_dev(1, lf, ob.ptr, bool(gel >= 1), b.ptr(sun), b.ptr(moon), b.ptr(ao), b.ptr(tm))
        return ob.download(np.uint8, (W, W, 4))


def dev_weights(t, w, tm, per_call=4):
    out = []
    for i in range(0, len(w), per_call):
        with Bufs(t) as b:
            n = len(w[i:i + per_call])
            ob = b.new(n * W * W * 4)
            t.tiles_tree_weights_dev(n, b.up(w[i:i + per_call]).ptr, None if tm is None else b.up(tm[i:i + per_call]).ptr, ob.ptr)
            out.append(ob.download(np.uint8, (n, W, W, 4)))
    return np.concatenate(out)


def _stats_bytes(st):
    return np.frombuffer(bytes(memoryview(st).cast("B")), np.uint8)


def dev_lines(pkg, t, tiles, z, mz, rows, kind, tile):
    """lib_lines' one batch of lines per tile through terra_tiles_line_intersect_dev"""
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    out = np.zeros(len(rows), orclib.LINE_REF_DTYPE)
    out["t"] = 1.0
    for i, distant, sel in _line_sets(kind, tile, len(tiles)):
        with Bufs(t) as b:
            hb = b.new(len(sel) * pkg.LINE_HIT_DTYPE.itemsize)
            t.tiles_line_intersect_dev(tiles[i:i + 1], b.up(z[i:i + 1]).ptr, b.up(_stats_bytes(lib_stats(pkg, mz[i:i + 1], 0.0))).ptr, b.up(rows[sel]).ptr, len(sel), hb.ptr,
                                       None, 0, 0, b.up(np.array([int(distant)], np.uint8)).ptr)
            h = hb.download(pkg.LINE_HIT_DTYPE, (len(sel),))
        hit = h["hit"] == 1
        o = out[sel]
        o["hit"] = hit
        o["t"], o["xpos"], o["ypos"] = np.where(hit, h["t"], f32(1.0)), np.where(hit, h["xpos"], 0), np.where(hit, h["ypos"], 0)
        out[sel] = o
    return out


def dev_stroke(pkg, t, d, s):
    """lib_stroke through terra_tiles_edit_grass_dev"""
    i = int(s["tile"])
    w, gb = prepared(d, i, int(s["prep"]))
    brush = pkg.make_grass_brush(tuple(float(v) for v in s["pos"]), float(s["radius"]), int(s["add"]), int(s["shape"]), float(s["weight"]))
    with Bufs(t) as b:
        wb, gbb, ub, rb = b.up(w), b.up(gb), b.up(np.array([7], np.uint8)), b.up(np.full(4, 77, np.uint32))
        t.tiles_edit_grass_dev(d["tiles"][i:i + 1], b.up(d["z"][i:i + 1]).ptr, b.up(_stats_bytes(lib_stats(pkg, d["mz"][i:i + 1], d["radius"][i]))).ptr, brush, wb.ptr, gbb.ptr,
                               ub.ptr, rb.ptr)
        upd = ub.download(np.uint8, (1,))
        assert upd[0] in (0, 1)
        return bool(upd[0]), wb.download(np.uint8, (W, W, 4)), gbb.download(orclib.GRASS_BLOCK_DTYPE, (32, 32)), tuple(int(v) for v in rb.download(np.uint32, (4,)))


PASSES = ("tree", "shadow", "weights", "lines", "strokes")


def check_lib_against(pkg, t, dev, tree, shadow, weights, lines, strokes, only=PASSES):
    """the library (dev: its device entry points) against recorded or live reference results, every byte, for the passes named in `only`:
    tree = (cases, [(map, flags)]); shadow = [(call, texture)]; weights = [(mesh_weights, tree_map or None, weight_data)];
    lines = (tiles, z, mz, rows, kind, tile, hits); strokes = (d, [(stroke, (returned, weights, blocks, has_any_grass, flower calls))])"""
    assert set(only) <= set(PASSES)
    if "tree" in only:
        cases, want = tree
        compare_tree("library", cases, (dev_tree if dev else lib_tree)(pkg, t, cases), want, flags=False)
    t.init_scene(pkg.make_config(mesh_gen_mode=0))
    if "shadow" in only:
        for call, tex in shadow:
            first_diff(f"library: shadow texture {call}", dev_shadow(t, call) if dev else lib_shadow(t, call), tex)
    if "weights" in only:
        for w, tm, out in weights:
            first_diff("library: tree weights", (dev_weights if dev else lib_weights)(t, w, tm), out)
    if "lines" in only:
        tiles, z, mz, rows, kind, tile, hits = lines
        compare_lines("library, a tile a call", (dev_lines if dev else lib_lines)(pkg, t, tiles, z, mz, rows, kind, tile), hits, kind)
        if not dev:
            compare_lines("library, four tiles a call", lib_lines(pkg, t, tiles, z, mz, rows, kind, tile, together=True), hits, kind)
    if "strokes" in only:
        lib_grass_setup(pkg, t)
        d, recorded = strokes
        for k, (s, want) in enumerate(recorded):
            got = (dev_stroke if dev else lib_stroke)(pkg, t, d, s)
            compare_stroke(f"library: stroke {k}", got, want)
            assert got[3] == stroke_range(want[4]), f"stroke {k}: range {got[3]} != the reference's update_subrange {stroke_range(want[4])}"


def fixture_sets(fx):
    """the fixture in check_lib_against's form"""
    w, tm, out = fixture_weights(fx)
    return dict(tree=fixture_tree(fx), shadow=[fixture_shadow(fx, k) for k in range(len(fx["shadow_lf"]))], weights=[(w, tm, out)],
                lines=(fx["line_tiles"], fx["line_z"], fx["line_mz"], fx["line_rows"], fx["line_kind"], fx["line_tile"], fx["line_hits"]),
                strokes=(fx["grass_d"], [fixture_stroke(fx, k) for k in range(len(fx["grass_strokes"]))]))


def reference_sets(chk):
    """the full case sets with the live reference's results, in check_lib_against's form (the reference's landscape is put back)"""
    try:
        cases = tree_cases(chk)
        tree = (cases, ref_tree(chk, cases))
        shadow = [(c, ref_shadow(chk, c)) for c in shadow_calls()]
        w, tm = weights_pairs()
        ws, tms = weights_stride()
        weights = [(w, tm, ref_weights(chk, w, tm)), (ws, tms, ref_weights(chk, ws, tms)), (ws[:1], None, ref_weights(chk, ws[:1], None))]
        sc = line_scene(chk)
        tiles, z, mz = line_tiles(chk)
        rows, kind, tile, groups = line_rows(sc, tiles, z, mz)
        lines = (tiles, z, mz, rows, kind, tile, ref_lines(chk, tiles, z, mz, rows, kind, tile))
        gsc = grass_scene(chk)
        d = grass_tiles(chk)
        recorded = []
        for s in grass_strokes(gsc, d):
            r = ref_stroke(chk, d, s)
            c = r[4].as_tuple()
            recorded.append((s, r[:4] + (c,)))
        return dict(tree=tree, shadow=shadow, weights=weights, lines=lines, strokes=(d, recorded))
    finally:
        chk.set_landscape(orclib.make_landscape())


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the fixture: a compact recording (inputs with the reference's outputs) for checkouts without the reference tree
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def sparse(out, base):
    """the bytes of `out` that differ from `base` -> (positions uint32, values uint8)"""
    a, b = np.ascontiguousarray(out).view(np.uint8).reshape(-1), np.ascontiguousarray(base).view(np.uint8).reshape(-1)
    pos = np.nonzero(a != b)[0].astype(np.uint32)
    return pos, a[pos]


def unsparse(base, pos, val):
    out = np.ascontiguousarray(base).copy()
    out.view(np.uint8).reshape(-1)[pos] = val
    return out


def record(chk):
    """everything the fixture holds, from the live reference -> (dict of arrays for np.savez_compressed, tallies as lines of text, the +-ulp group counts of
    line_tallies, grass_tallies' dict)"""
    fx, text = {}, []
    try:
        # tree map: one splat list per kind
        cases = tree_cases(chk, FIXTURE_TREE)
        got = ref_tree(chk, cases)
        fx["tree_name"] = np.array([c["name"] for c in cases])
        fx["tree_scene"] = np.array([c["scene"] for c in cases], np.int32)
        fx["tree_tile"] = np.array([c["tile"] for c in cases], np.int32)
        fx["tree_hag"] = np.array([c["hag"] for c in cases], np.uint8)
        fx["tree_first"] = np.concatenate([[0], np.cumsum([len(c["splats"]) for c in cases])]).astype(np.uint32)
        fx["tree_splats"] = np.concatenate([c["splats"] for c in cases])
        fx["tree_in"] = np.stack([c["prefill"] for c in cases])
        fx["tree_out"] = np.stack([g[0] for g in got])
        fx["tree_flags"] = np.array([g[1] for g in got], np.uint8)
        text.append(f"tree map: {len(cases)} splat lists, {len(fx['tree_splats'])} splats, {int((fx['tree_out'] != fx['tree_in']).sum())} bytes changed")
        # shadow texture: the light-factor set on tile 0.  Bytes 1 .. 3 of a texel do not depend on the light factor (asserted here): they are kept once
        lfs = light_factors()
        sh = np.stack([ref_shadow(chk, (lf, 1, 0, True, True, True)) for lf in lfs])
        assert (sh[:, :, :, 1:] == sh[0, :, :, 1:]).all()
        fx["shadow_lf"], fx["shadow_mesh"], fx["shadow_rest"] = lfs, np.ascontiguousarray(sh[..., 0]), np.ascontiguousarray(sh[0, :, :, 1:])
        text.append(f"shadow texture: {len(lfs)} light factors, {len(np.unique(sh[..., 0]))} distinct mesh shadow bytes")
        # tree weights: the pair set.  The inputs are weights_pairs()'s formula; kept: the dirt and grass bytes the reference leaves
        w, tm = weights_pairs()
        out = ref_weights(chk, w, tm)
        assert (out[..., SAND] == w[..., SAND]).all() and (out[..., ROCK] == w[..., ROCK]).all()
        fx["weights_dirt"], fx["weights_grass"] = np.ascontiguousarray(out[..., DIRT]), np.ascontiguousarray(out[..., GRASS])
        text.append(f"tree weights: {len(PAIR_DIRT) * 65536} (tree_ao, grass, dirt) texels, {int((out != w).sum())} bytes changed")
        # lines
        sc = line_scene(chk)
        tiles, z, mz = line_tiles(chk)
        rows, kind, tile, groups = line_rows(sc, tiles, z, mz)
        hits = ref_lines(chk, tiles, z, mz, rows, kind, tile)
        fx.update(line_tiles=tiles, line_z=z, line_mz=mz, line_rows=rows, line_kind=kind, line_tile=tile, line_groups=groups, line_hits=hits)
        fx["line_scene"] = np.array([sc.xss, sc.yss, sc.DX_VAL, sc.DY_VAL, sc.DX_VAL_INV, sc.DY_VAL_INV], f32)
        t2, by_kind = line_tallies(hits, kind, groups)
        text += [f"line tiles: water {tiles[0].tolist()}, steep {tiles[1].tolist()}, far {tiles[2].tolist()}, flat {tiles[3].tolist()}"] + t2
        # grass strokes: outputs kept as the bytes that differ from the stroke's input
        gsc = grass_scene(chk)
        d = grass_tiles(chk)
        strokes = grass_strokes(gsc, d)
        fx.update(grass_tiles=d["tiles"], grass_z=d["z"], grass_mz=d["mz"], grass_radius=d["radius"], grass_w=d["w"], grass_gb=d["gb"],
                  grass_params=d["params"], grass_strokes=strokes)
        ret, hag, calls, wpos, wval, gpos, gval, wfirst, gfirst, results = [], [], [], [], [], [], [], [0], [0], []
        for s in strokes:
            r, w1, gb1, h1, c1 = ref_stroke(chk, d, s)
            results.append((r, w1, gb1))
            w0, gb0 = prepared(d, int(s["tile"]), int(s["prep"]))
            p, v = sparse(w1, w0); wpos.append(p); wval.append(v); wfirst.append(wfirst[-1] + len(p))
            p, v = sparse(gb1, gb0); gpos.append(p); gval.append(v); gfirst.append(gfirst[-1] + len(p))
            ret.append(r); hag.append(h1)
            c = c1.as_tuple()
            calls.append(c[:9] + c[9] + (c[10], c[11]))
        fx["grass_ret"], fx["grass_hag"] = np.array(ret, np.uint8), np.array(hag, np.uint8)
        fx["grass_calls_i"] = np.array([c[:9] + (c[13],) for c in calls], np.int64)
        fx["grass_calls_f"] = np.array([c[9:13] for c in calls], f32)
        fx["grass_wpos"], fx["grass_wval"], fx["grass_wfirst"] = np.concatenate(wpos), np.concatenate(wval), np.array(wfirst, np.uint32)
        fx["grass_gpos"], fx["grass_gval"], fx["grass_gfirst"] = np.concatenate(gpos), np.concatenate(gval), np.array(gfirst, np.uint32)
        text.append(f"grass strokes: {len(strokes)}, returned 1: {int(sum(ret))}, weight bytes changed {len(fx['grass_wpos'])}, update_subrange calls "
                    f"{int(fx['grass_calls_i'][:, 0].sum())}, clear_within calls {int(fx['grass_calls_i'][:, 1].sum())}")
        reach = grass_tallies(gsc, d, strokes, results)
        text.append("grass strokes reach: " + ", ".join(f"{k} {v}" for k, v in reach.items()))
    finally:
        chk.set_landscape(orclib.make_landscape())
    return fx, text, by_kind, reach


def load():
    fx = dict(np.load(FIXTURE))
    d = dict(tiles=fx["grass_tiles"], z=fx["grass_z"], mz=fx["grass_mz"], radius=fx["grass_radius"], w=fx["grass_w"], gb=fx["grass_gb"], params=fx["grass_params"])
    fx["grass_d"] = d
    return fx


def fixture_tree(fx):
    """-> (cases, [(map, flags)]) as recorded"""
    cases = [dict(name=str(fx["tree_name"][k]), scene=int(fx["tree_scene"][k]), tile=tuple(int(v) for v in fx["tree_tile"][k]), hag=bool(fx["tree_hag"][k]),
                  splats=np.ascontiguousarray(fx["tree_splats"][fx["tree_first"][k]:fx["tree_first"][k + 1]]), prefill=fx["tree_in"][k]) for k in range(len(fx["tree_name"]))]
    return cases, [(fx["tree_out"][k], tuple(bool(v) for v in fx["tree_flags"][k])) for k in range(len(cases))]


def fixture_shadow(fx, k):
    """-> (call, recorded texture) of light factor k"""
    return (fx["shadow_lf"][k], 1, 0, True, True, True), np.concatenate([fx["shadow_mesh"][k][..., None], fx["shadow_rest"]], -1)


def fixture_weights(fx):
    """-> (mesh_weights, tree_map, recorded weight_data)"""
    w, tm = weights_pairs()
    out = w.copy()
    out[..., DIRT], out[..., GRASS] = fx["weights_dirt"], fx["weights_grass"]
    return w, tm, out


def fixture_line_scene(fx):
    s = fx["line_scene"]
    return lim.Scene(s[0], s[1], s[2], s[3], s[4], s[5], S)


def fixture_stroke(fx, k):
    """-> (stroke, (returned, weights, blocks, has_any_grass, flower calls as expected_calls' tuple)) as recorded"""
    s, d = fx["grass_strokes"][k], fx["grass_d"]
    w0, gb0 = prepared(d, int(s["tile"]), int(s["prep"]))
    a, b = fx["grass_wfirst"][k:k + 2]
    w1 = unsparse(w0, fx["grass_wpos"][a:b], fx["grass_wval"][a:b])
    a, b = fx["grass_gfirst"][k:k + 2]
    gb1 = unsparse(gb0, fx["grass_gpos"][a:b], fx["grass_gval"][a:b])
    ci, cf = fx["grass_calls_i"][k], fx["grass_calls_f"][k]
    calls = tuple(int(v) for v in ci[:9]) + (tuple(float(v) for v in cf[:3]), float(cf[3]), int(ci[9]))
    return s, (bool(fx["grass_ret"][k]), w1, gb1, bool(fx["grass_hag"][k]), calls)
