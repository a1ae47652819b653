"""Cases of the line-vs-terrain query (terra_tiles_line_intersect[_dev]) shared by the emulator and GPU tests: every case runs the same lines through the
library and through tests/line_intersect_model.py and compares the records byte for byte.  Zvals and stats come from the library's own tiles_create_zvals
(which the existing tile tests pin to the oracle), plus two synthetic tiles: a constant height and a ramp along x."""
import ctypes as C

import numpy as np

import line_intersect_model as lim

TILES = [(0, 0), (1, 0), (0, 1), (1, 1), (-1, 0), (-1, -1), (2, -1)]
CONST_TILE, RAMP_TILE = (3, 3), (4, 3)
ERR_ARG, ERR_STATE = -1, -3
FAR_CLIP = 100.0  # DEF_FAR_CLIP (src/3DWorld.h:115): the length of a fire-mode ray
f32 = np.float32


def synthetic(sc, kind):
    """[S+2, S+2] zvals and (mzmin, mzmax) of a constant-height tile (0.75) or a ramp rising DX_VAL per column from 0"""
    n = sc.S + 2
    if kind == "const":
        z = np.full((n, n), 0.75, f32)
    else:
        z = np.tile((np.arange(n) * float(sc.DX_VAL)).astype(f32), (n, 1))
    return z, f32(z.min()), f32(z.max())


def setup(pkg, t, S=128, tiles=TILES):
    """scene at tile size S; the batch = the library's tiles + the constant and ramp tiles, stats' mzmin / mzmax set to match the synthetic zvals"""
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    st = t.init_scene(cfg)
    sc = lim.Scene.of(cfg, st)
    z, stats, _, _ = t.tiles_create_zvals(tiles, 0, normals=False)
    txy = list(tiles) + [CONST_TILE, RAMP_TILE]
    n = len(txy)
    zall = np.empty((n, S + 2, S + 2), f32)
    zall[:len(tiles)] = z
    sall = (pkg.TileStats * n)()
    C.memmove(C.addressof(sall), C.addressof(stats), C.sizeof(stats))
    for i, kind in ((len(tiles), "const"), (len(tiles) + 1, "ramp")):
        zall[i], sall[i].mzmin, sall[i].mzmax = synthetic(sc, kind)
    return dict(sc=sc, tiles=txy, z=zall, stats=sall)


def mz(d):
    n = len(d["tiles"])
    return np.array([d["stats"][i].mzmin for i in range(n)], f32), np.array([d["stats"][i].mzmax for i in range(n)], f32)


def cell_xy(sc, tile, ix, iy, dxoff=0, dyoff=0):
    """camera-space x, y of mesh cell (ix, iy) of a tile: get_xval(x1 + ix + xoff - xoff2)"""
    return (f32(-sc.xss + sc.DX_VAL * f32(tile[0] * sc.S + ix + dxoff)), f32(-sc.yss + sc.DY_VAL * f32(tile[1] * sc.S + iy + dyoff)))


def camera_rays(sc, tiles, z, rs, count, dxoff=0, dyoff=0, length=FAR_CLIP):
    """rays of length FAR_CLIP from a camera 0.5 .. 40 units before a random terrain point, pitched 3 .. 85 degrees down at every heading"""
    out = np.empty((count, 2, 3), f32)
    for k in range(count):
        i = rs.randint(len(tiles))
        ix, iy = rs.randint(0, sc.S + 1, 2)
        x, y = cell_xy(sc, tiles[i], ix, iy, dxoff, dyoff)
        tgt = np.array([x, y, z[i, iy, ix]], f32)
        p, yaw = np.radians(rs.uniform(-85.0, -3.0)), rs.uniform(0.0, 2 * np.pi)
        dirv = np.array([np.cos(p) * np.cos(yaw), np.cos(p) * np.sin(yaw), np.sin(p)], f32)
        out[k, 0] = tgt - dirv * f32(rs.uniform(0.5, 40.0))
        out[k, 1] = out[k, 0] + dirv * f32(length)
    return out


def special_lines(sc, d, rs):
    """the named cases -> {name: [nlines, 2, 3]}"""
    tiles, z = d["tiles"], d["z"]
    mzmin, mzmax = mz(d)
    S, n = sc.S, len(tiles)
    cases = {}
    pts = []  # random terrain points: (tile, x, y, zval)
    for _ in range(64):
        i = rs.randint(n)
        ix, iy = rs.randint(0, S + 1, 2)
        x, y = cell_xy(sc, tiles[i], ix, iy)
        pts.append((i, x, y, z[i, iy, ix]))
    rand_dir = lambda: rs.normal(size=3).astype(f32)  # noqa: E731
    cases["under_mesh"] = np.array([[[x, y, zv - f32(0.3)], [x, y, zv - f32(0.3)] + f32(30.0) * rand_dir()] for i, x, y, zv in pts], f32)
    cases["inside_bcube"] = np.array([[[x, y, f32(rs.uniform(mzmin[i], mzmax[i]))], [x, y, f32(0.0)] + f32(20.0) * rand_dir()] for i, x, y, zv in pts], f32)
    cases["vertical"] = np.array([[[x, y, zv + f32(5.0)], [x, y, zv - f32(5.0)]] for i, x, y, zv in pts[:32]]
                                 + [[[x, y, zv - f32(5.0)], [x, y, zv + f32(5.0)]] for i, x, y, zv in pts[32:]], f32)
    cases["horizontal"] = np.array([[[x, y, zv - f32(0.05)], [x + f32(30.0), y - f32(7.0), zv - f32(0.05)]] for i, x, y, zv in pts], f32)
    # along the shared edges x = x of column S of tile (0, 0) = column 0 of tile (1, 0), and just inside tile (0, 0); y likewise
    xe, ye = cell_xy(sc, (0, 0), S, S)
    eps = f32(1e-6)
    edge = []
    for k in range(16):
        y0, x0 = cell_xy(sc, (0, 0), 0, 4 * k)[1], cell_xy(sc, (0, 0), 4 * k, 0)[0]
        edge += [[[xe, y0, f32(3.0)], [xe, y0 + f32(10.0), f32(-3.0)]], [[xe - eps, y0, f32(3.0)], [xe - eps, y0 + f32(10.0), f32(-3.0)]],
                 [[x0, ye, f32(3.0)], [x0 + f32(10.0), ye, f32(-3.0)]], [[xe, ye, f32(2.0 + 0.1 * k)], [xe, ye, f32(-2.0)]]]
    cases["shared_edge"] = np.array(edge, f32)
    # v1 just inside the bottom of a tile's box, v2 a million units below: tmax <= TOLERANCE leaves v2 unclipped, the walk runs to x in (-1, 0) (ix = 0) and
    # the first cell that passes has cur_t < 0; with a far x offset (11200 cells) the walk would take >= 10000 steps (the reference's assert: a miss)
    neg = []
    for i in range(n):
        zlo = f32(mzmin[i] - lim.BCUBE_ZTOLER)
        x, y = cell_xy(sc, tiles[i], 0, S // 3)
        v1 = np.array([x + f32(0.3) * sc.DX_VAL, y + f32(0.3) * sc.DY_VAL, np.nextafter(zlo, f32(np.inf))], f32)
        for cx, cy in ((-2.4, 8.0), (-1.2, 5.0), (11200.0, 0.0)):  # v2's offset in cells
            neg.append([v1, v1 + np.array([f32(cx) * sc.DX_VAL, f32(cy) * sc.DY_VAL, f32(-1e6)], f32)])
    cases["unclipped_v2"] = np.array(neg, f32)
    cases["misses"] = np.array([[[x, y, f32(60.0)], [x + f32(5.0), y, f32(59.0)]] for i, x, y, zv in pts[:16]]
                               + [[[f32(900.0), f32(-900.0), f32(1.0)], [f32(950.0), f32(-900.0), f32(-1.0)]], [[f32(0.1), f32(0.2), f32(-50.0)], [f32(0.3), f32(0.2), f32(-60.0)]]], f32)
    nf = []
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(6):
            v = np.array([[0.1, 0.2, 5.0], [0.15, 0.25, -5.0]], f32)
            v.reshape(-1)[a] = bad
            nf.append(v)
    cases["non_finite"] = np.array(nf, f32)
    return cases


def compare(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.view(np.uint8).reshape(len(got), -1).__ne__(want.view(np.uint8).reshape(len(want), -1)).any(axis=1))[0]
        r = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first line {r}: got {got[r]} want {want[r]}")


def model(d, lines, line_tile=None, dxoff=0, dyoff=0, distant=None):
    mzmin, mzmax = mz(d)
    return lim.batch_hits(d["sc"], d["tiles"], d["z"], mzmin, mzmax, lines, line_tile, dxoff, dyoff, distant)


def run(t, d, lines, line_tile=None, dxoff=0, dyoff=0, distant=None, what=""):
    """one call of the host entry point and the model on the same lines: identical records.  -> the records"""
    got = t.tiles_line_intersect(d["tiles"], d["z"], d["stats"], lines, line_tile, dxoff, dyoff, distant)
    want = model(d, lines, line_tile, dxoff, dyoff, distant)
    compare(what, got, want)
    return want


def reorder(d, perm):
    perm = list(perm)
    st = (d["stats"]._type_ * len(perm))()
    for k, i in enumerate(perm):
        C.memmove(C.addressof(st[k]), C.addressof(d["stats"][i]), C.sizeof(st[k]))
    return dict(d, tiles=[d["tiles"][i] for i in perm], z=d["z"][perm].copy(), stats=st)


def run_cases(pkg, t, S=128):
    d = setup(pkg, t, S)
    sc, n = d["sc"], len(d["tiles"])
    rs = np.random.RandomState(7 + S)
    cam = camera_rays(sc, d["tiles"], d["z"], rs, 1500)
    h = run(t, d, cam, what="camera rays")
    assert h["hit"].mean() > 0.5 and len(set(h["tile"][h["hit"] == 1])) >= n - 2
    off = camera_rays(sc, d["tiles"], d["z"], rs, 400, 5, -3)
    assert run(t, d, off, dxoff=5, dyoff=-3, what="offsets")["hit"].mean() > 0.5
    sp = special_lines(sc, d, rs)
    for name, lines in sp.items():
        h = run(t, d, lines, what=name)
        if name in ("horizontal", "misses", "non_finite"):
            assert not h["hit"].any(), name
        if name == "unclipped_v2":
            assert h["hit"][0::3].all() and h["hit"][1::3].all() and not h["hit"][2::3].any()
        if name in ("vertical", "under_mesh"):
            assert h["hit"].any(), name
    distant = (np.arange(n) % 3) == 1
    hd = run(t, d, cam, distant=distant, what="distant")
    assert not np.isin(hd["tile"], np.nonzero(distant)[0]).any()
    lt = np.full(len(cam), -1, np.int32)
    lt[0::3] = rs.randint(n, size=len(lt[0::3]))
    hr = run(t, d, cam, line_tile=lt, what="one tile per line")
    assert (hr["tile"][lt >= 0] == lt[lt >= 0])[hr["hit"][lt >= 0] == 1].all()
    # ties: tile (1, 0) twice in the batch; then the batch reversed -- the same t / xpos / ypos / p_int, the tile the first of the equal-t tiles in the new order
    dd = reorder(d, list(range(n)) + [1])
    aim = camera_rays(sc, [d["tiles"][1]], d["z"][1:2], rs, 200)
    both = np.concatenate([aim, cam[:300]])
    hf = run(t, dd, both, what="duplicate tile")
    on_dup = hf["tile"][:200] == 1
    assert on_dup.sum() > 100 and not (hf["tile"] == n).any()
    rev = reorder(dd, range(n, -1, -1))
    hb = run(t, rev, both, what="reversed batch")
    for f in ("t", "xpos", "ypos", "p_int", "hit"):
        assert hf[f].tobytes() == hb[f].tobytes(), f
    assert (hb["tile"][:200][on_dup] == 0).all()  # (the duplicate is batch index 0 of the reversed batch)
    return d
