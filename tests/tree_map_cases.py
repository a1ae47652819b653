"""Cases of the tree map (terra_tiles_tree_map[_dev]), the shadow texture (terra_tiles_shadow_texture[_dev]) and the tree weights (terra_tiles_tree_weights[_dev])
shared by the emulator and GPU tests: every case runs the library and tests/tree_map_model.py on the same inputs and compares every byte of every tile."""
import numpy as np

import orclib
import tree_map_model as tmm

TILES = [(0, 0), (1, 0), (0, 1), (1, 1), (-1, 0), (2, -1)]
ERR_ARG, ERR_STATE = -1, -3
LIGHT_FACTORS = [0.0, 0.39, float(np.float32(0.4)), 0.45, 0.5, 0.55, float(np.float32(0.6)), 0.61, 1.0]


def setup(pkg, t, orc, S=128, scene=(4.0, 4.0, 4.0)):
    """the scene on both sides; the model's constants are the oracle's"""
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S, scene=scene)
    t.init_scene(cfg)
    return tmm.Scene(orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S, scene=scene)), cfg)


def at(sc, tile, fx, fy, dxoff=0, dyoff=0):
    """camera-space (x, y) of the (fractional) texel (fx, fy) of a tile, as floats"""
    tx, ty = tile
    return (np.float32(float(sc.get_xval(tx * sc.S + dxoff)) + fx * float(sc.DX_VAL)), np.float32(float(sc.get_yval(ty * sc.S + dyoff)) + fy * float(sc.DY_VAL)))


def radius(sc, r):
    """a tradius of r texels along x"""
    return np.float32(r * float(sc.DX_VAL))


def lists(per_tile):
    """[[(x, y, radius), ...] per tile] -> (splats SPLAT_DTYPE, first uint32 [n+1])"""
    first = np.zeros(len(per_tile) + 1, np.uint32)
    first[1:] = np.cumsum([len(li) for li in per_tile])
    sp = np.zeros(int(first[-1]), tmm.SPLAT_DTYPE)
    k = 0
    for li in per_tile:
        for x, y, r in li:
            sp[k] = (x, y, r)
            k += 1
    return sp, first


def cluster(sc, tile, rs, count, cx, cy, spread, dxoff=0, dyoff=0, rmin=1.2, rmax=5.9):
    """count trees around texel (cx, cy): dense, overlapping, rval 2 .. 6 by default"""
    out = []
    for _ in range(count):
        x, y = at(sc, tile, cx + rs.uniform(-spread, spread), cy + rs.uniform(-spread, spread), dxoff, dyoff)
        out.append((x, y, radius(sc, rs.uniform(rmin, rmax))))
    return out


def cases(sc, tiles=TILES):
    """(name, per-tile lists, dxoff, dyoff, distant or None)"""
    S, n = sc.S, len(tiles)
    rs = np.random.RandomState(5)
    empty = lambda: [[] for _ in range(n)]  # noqa: E731
    out = []
    # rval 1 .. 13 inside a tile (radius k + 0.4 texels: rval = k + 1), each tile its own positions
    li = empty()
    for i, tile in enumerate(tiles):
        for k in range(13):
            x, y = at(sc, tile, 6.3 + (S - 12) * ((k * 5 + i) % 13) / 13.0, 5.7 + (S - 12) * ((k * 3 + 2 * i) % 13) / 13.0)
            li[i].append((x, y, radius(sc, k + 0.4)))
    out.append(("rvals", li, 0, 0, None))
    # across each border and corner, inside, and wholly outside (the caller's cull lets such splats through: the window is empty)
    li = empty()
    edge = [-20.0, -3.2, 0.0, 0.4 * S, S - 0.3, S + 0.0, S + 3.4, S + 25.0]
    for i, tile in enumerate(tiles):
        for a, fx in enumerate(edge):
            for b, fy in enumerate(edge):
                if (a + 2 * b + i) % 3 == 0:
                    x, y = at(sc, tile, fx, fy)
                    li[i].append((x, y, radius(sc, 4.4 + 0.5 * ((a + b) % 3))))
    out.append(("borders", li, 0, 0, None))
    # centres on half-texel ties and at negative offsets: round_fp adds 0.5 to a positive quotient and subtracts it from the others
    li = empty()
    for i, tile in enumerate(tiles):
        for k in (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 40.5, S - 0.5, S + 0.5, S + 1.5, -2.49, -0.51, 0.49, -0.0):
            for fx, fy, r in ((k, 20.5, 2.3), (37.5, k, 1.0), (k, k, 3.7), (k, S - 1.5, 5.2)):
                x, y = at(sc, tile, fx, fy)
                li[i].append((x, y, radius(sc, r)))
    out.append(("ties", li, 0, 0, None))
    # tradius/DX_VAL exactly integral: int() of an integer, rval = that + 1
    li = empty()
    for i, tile in enumerate(tiles):
        for k, r in enumerate((0.0, 1.0, 2.0, 3.0, 7.0, 12.0)):
            x, y = at(sc, tile, 10.0 + 0.17 * S * k, 0.5 * S + 3 * i)
            li[i].append((x, y, np.float32(r) * sc.DX_VAL))
    out.append(("integral_radius", li, 0, 0, None))
    # dense overlapping clusters, some on a corner so that they reach four tiles' frames; tiles 2 and 5 have no trees
    li = empty()
    li[0] = cluster(sc, tiles[0], rs, 300, 0.3 * S, 0.4 * S, 9.0)
    li[1] = cluster(sc, tiles[1], rs, 150, 1.5, 0.6 * S, 6.0)
    li[3] = cluster(sc, tiles[3], rs, 200, 0.0, 0.0, 8.0) + cluster(sc, tiles[3], rs, 50, 0.9 * S, 0.9 * S, 20.0, rmin=6.0, rmax=14.0)
    li[4] = cluster(sc, tiles[4], rs, 80, S - 1.0, S - 2.0, 5.0)
    out.append(("clusters", li, 0, 0, None))
    out.append(("all_empty", empty(), 0, 0, None))
    # distant tiles: filled under reset, otherwise left alone, never updated
    dist = np.array([(i % 2) for i in range(n)], np.uint8)
    out.append(("distant", out[4][1], 0, 0, dist))
    # where the reference is undefined the splat is skipped; the others of the list are applied
    li = empty()
    x0, y0 = at(sc, tiles[0], 30.2, 40.1)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    good = [(x0, y0, radius(sc, 3.3)), (at(sc, tiles[0], 33.0, 41.5) + (radius(sc, 4.6),))]
    bad = [(nan, y0, radius(sc, 3.0)), (x0, nan, radius(sc, 3.0)), (x0, y0, nan), (inf, y0, radius(sc, 3.0)), (x0, -inf, radius(sc, 3.0)), (x0, y0, inf),
           (x0, y0, radius(sc, -0.5)), (x0, y0, np.float32(-0.0) - np.float32(1e-30)), (x0, y0, radius(sc, 46340.0)), (x0, y0, radius(sc, 1.0e6)),
           (np.float32(1.0e9), y0, radius(sc, 3.0)), (x0, np.float32(-1.0e9), radius(sc, 3.0)), (np.float32(3.0e38), y0, radius(sc, 3.0)),
           (np.float32(-3.0e38), np.float32(3.0e38), np.float32(3.0e38))]
    edge_ok = [(x0, y0, radius(sc, 46339.5)),                 # rval = 46340, the largest whose square fits: every texel of the tile
               (np.float32(6.0e7 * float(sc.DX_VAL) / 0.0625), y0, radius(sc, 3.0)),  # a quotient just inside 2^30: an empty window
               (x0, y0, np.float32(-0.0))]                      # -0 is not < 0: rval = 1
    for i in range(n):
        li[i] = [good[0]] + bad[:7] + [good[1]] + bad[7:] + edge_ok + [good[0]]
    out.append(("skipped", li, 0, 0, None))
    # non-zero offsets: the tile's frame moves by dxoff / dyoff cells
    li = empty()
    for i, tile in enumerate(tiles):
        li[i] = cluster(sc, tile, rs, 40, 0.5 * S, 0.5 * S, 0.6 * S, 5, -3)
    out.append(("offsets", li, 5, -3, None))
    return out


def run_one(t, sc, tiles, per_tile, dxoff=0, dyoff=0, distant=None, what="", pad=0):
    """one reset call through the host entry point vs the model; pad: unused records in front of the list (h_first[0] != 0)"""
    sp, first = lists(per_tile)
    if pad:
        sp = np.concatenate([np.full(pad, np.nan, np.float32).repeat(3).view(tmm.SPLAT_DTYPE), sp])
        first = first + np.uint32(pad)
    got, gupd = t.tiles_tree_map(tiles, sp, first, True, None, dxoff, dyoff, distant)
    want, wupd = tmm.tiles_tree_map(sc, tiles, sp, first, True, None, dxoff, dyoff, distant)
    compare(what, got, gupd, want, wupd)
    return want, wupd


def compare(what, got, gupd, want, wupd):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} tree map bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert (np.asarray(gupd, bool) == np.asarray(wupd, bool)).all(), f"{what}: updated {np.asarray(gupd, bool)} != {np.asarray(wupd, bool)}"


def order_sensitive(sc, tiles=TILES):
    """on the model alone: the clusters case gives another map when every list is reversed (so a library that reorders splats cannot pass it)"""
    per_tile = [c for c in cases(sc, tiles) if c[0] == "clusters"][0][1]
    sp, first = lists(per_tile)
    a, _ = tmm.tiles_tree_map(sc, tiles, sp, first, True)
    sp2, first2 = lists([li[::-1] for li in per_tile])
    b, _ = tmm.tiles_tree_map(sc, tiles, sp2, first2, True)
    return int((a != b).sum())


def run_cases(pkg, t, orc, S=128, scene=(4.0, 4.0, 4.0), only=None):
    sc = setup(pkg, t, orc, S, scene)
    for k, (name, per_tile, dxoff, dyoff, distant) in enumerate(cases(sc)):
        if only and name not in only:
            continue
        want, upd = run_one(t, sc, TILES, per_tile, dxoff, dyoff, distant, f"S={S} {name}", pad=3 if k % 2 else 0)
        if name in ("all_empty",):
            assert not upd.any() and (want == 255).all()
        elif name == "distant":
            assert not upd[1::2].any() and upd[0] and (want[1::2] == 255).all()
        else:
            assert upd.any() and (want != 255).any(), name
    return sc


def run_continue(pkg, t, orc, S=128):
    """reset = 0 continues a map: two calls (the second with reset = 0) equal one call with the concatenated lists, and both equal the model; a distant tile is
    left alone by the second call whatever it holds"""
    sc = setup(pkg, t, orc, S)
    cs = {c[0]: c[1] for c in cases(sc)}
    first_half, second_half = cs["clusters"], cs["borders"]
    sp1, f1 = lists(first_half)
    sp2, f2 = lists(second_half)
    spc, fc = lists([a + b for a, b in zip(first_half, second_half)])
    m, u1 = t.tiles_tree_map(TILES, sp1, f1, True)
    m, u2 = t.tiles_tree_map(TILES, sp2, f2, False, m)
    one, uo = t.tiles_tree_map(TILES, spc, fc, True)
    want, wu = tmm.tiles_tree_map(sc, TILES, spc, fc, True)
    compare("two calls", m, u1 | u2, want, wu)
    compare("one call", one, uo, want, wu)
    _, wu2 = tmm.tiles_tree_map(sc, TILES, sp2, f2, False, want.copy())
    assert (u2 == wu2).all()  # `updated` is this call's alone
    # reset = 0 with a distant tile and with empty lists: nothing is touched
    rs = np.random.RandomState(9)
    held = rs.randint(0, 256, want.shape).astype(np.uint8)
    dist = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    got, gu = t.tiles_tree_map(TILES, sp2, f2, False, held.copy(), 0, 0, dist)
    wm, wu3 = tmm.tiles_tree_map(sc, TILES, sp2, f2, False, held.copy(), 0, 0, dist)
    compare("continue on held bytes, distant tiles", got, gu, wm, wu3)
    assert (got[dist == 1] == held[dist == 1]).all() and not gu[dist == 1].any()
    got, gu = t.tiles_tree_map(TILES, np.zeros(0, tmm.SPLAT_DTYPE), np.zeros(len(TILES) + 1, np.uint32), False, held.copy())
    assert (got == held).all() and not gu.any()


# ---- shadow texture: exhaustive over the byte inputs
def shadow_inputs(S, seed=3):
    """enough tiles at S for 65536 texels: texel q has base_ao = q & 255 and tree ao = q >> 8 (every pair), sun smask = q & 255 and moon smask = q >> 8 (every
    pair, the bytes with only bits outside 0xCF among them), sh = every byte; the smask cells outside the texture hold random bytes"""
    W, Z = S + 1, S + 2
    n = -(-65536 // (W * W))
    q = np.arange(n * W * W, dtype=np.uint32).reshape(n, W, W)
    rs = np.random.RandomState(seed)
    ao = (q & 255).astype(np.uint8)
    tree = np.stack([((q >> 8) & 255).astype(np.uint8), ((q * 7 + 3) & 255).astype(np.uint8)], axis=-1)
    sun, moon = rs.randint(0, 256, (n, Z, Z)).astype(np.uint8), rs.randint(0, 256, (n, Z, Z)).astype(np.uint8)
    sun[:, :W, :W] = (q & 255).astype(np.uint8)
    moon[:, :W, :W] = ((q >> 8) & 255).astype(np.uint8)
    assert n * W * W >= 65536 and set(np.unique(tree[..., 1])) == set(range(256))
    return n, sun, moon, ao, tree


def run_shadow_texture(pkg, t, orc, S):
    setup(pkg, t, orc, S)
    n, sun, moon, ao, tree = shadow_inputs(S)
    seen = set()
    for lf in LIGHT_FACTORS:
        has_sun, has_moon, _ = tmm.shadow_flags(lf)
        for ms in (1, 0):
            for use_ao in (True, False):
                for use_tree in (True, False):
                    for masks in ("both", "needed"):  # every mask given, or only what the lights that are up need (none without mesh shadows)
                        s_in = sun if (masks == "both" or (ms and has_sun)) else None
                        m_in = moon if (masks == "both" or (ms and has_moon)) else None
                        got = t.tiles_shadow_texture(n, lf, ms, s_in, m_in, ao if use_ao else None, tree if use_tree else None)
                        want = tmm.shadow_texture(S, lf, ms, sun, moon, ao if use_ao else None, tree if use_tree else None)
                        bad = np.argwhere(got != want)
                        assert len(bad) == 0, (f"S={S} lf={lf} mesh_shadows={ms} ao={use_ao} tree={use_tree} masks={masks}: {len(bad)} bytes differ, first at "
                                               f"{bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
                        seen.update(np.unique(want[..., 0]).tolist())
    assert {0, 255} <= seen and len(seen) > 2  # both lights up blends the two masks


# ---- tree weights: exhaustive over tree_ao x dirt x grass
def weights_inputs(stride=1, rock255=False):
    """texel c*stride has tree_ao = c & 255, dirt = (c >> 8) & 255, grass = c >> 16; sand and rock vary with c (rock is 255 on a few texels: the city skip)"""
    c = np.arange(0, 256 ** 3, stride, dtype=np.uint32)
    n = -(-len(c) // (129 * 129))
    c = np.resize(c, n * 129 * 129)
    w = np.stack([(c * 13 + 5) & 255, (c >> 8) & 255, (c >> 16) & 255, np.where(c % 97 == 0, 255, (c * 5) & 255)], axis=-1).astype(np.uint8).reshape(n, 129, 129, 4)
    if rock255:
        w[..., tmm.ROCK] = 255
    tree = np.stack([c & 255, (c >> 3) & 255], axis=-1).astype(np.uint8).reshape(n, 129, 129, 2)
    return w, tree


def model_weights_chunked(w, tree, chunk=64):
    return np.concatenate([tmm.tree_weights(w[i:i + chunk], None if tree is None else tree[i:i + chunk]) for i in range(0, len(w), chunk)])
