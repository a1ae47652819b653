"""Cases of the grass draw lists (terra_tiles_grass_view[_dev]) shared by test_grass_view_emul.py (the host emulator) and test_gpu_grass_view.py (HIP on the
MI355X).  insts, aux, group_counts, counts and pass are compared byte for byte and in order with tests/grass_view_model.py.

Zvals and grass blocks are inputs of the pass, so most cases use synthetic ones on the smallest tiles (S = 16: 16 blocks a tile; S = 20: dim 5).  The model's result
of a case is computed once per process (MODEL) together with its tally, and every case carries a check on that tally: that it exercises what it is named for.

The scene is the synthetic 4 x 4 one: a tile is 8 wide, get_grass_thresh_pad() is 16.8*tt_grass_scale_factor, lod_scale 0.3125/tt_grass_scale_factor."""
import ctypes as C
import math

import numpy as np

import grass_brush_cases as gbc
import grass_brush_model as gbm
import grass_view_model as gm
import view_model
import orclib

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
GRID3 = [(x, y) for y in (-1, 0, 1) for x in (-1, 0, 1)]
DOWN = dict(dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
ALONG_X = dict(dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))


class Case:
    def __init__(self, name, S=16, tiles=GRID3, terrain="slope", blocks="all", view=None, valid=1, tt=0.25, grass_length=0.02, nrnd=16, skip=None, dxoff=0, dyoff=0,
                 capacity=None, check=None):
        self.name, self.S, self.tiles, self.terrain, self.blocks, self.valid = name, S, list(tiles), terrain, blocks, valid
        self.view = dict(pos=(0.0, 0.0, 3.0), angle=1.2, aspect=1.0, near=0.01, far=100.0, **DOWN) if view is None else dict(view)
        self.tt, self.grass_length, self.nrnd, self.skip, self.dxoff, self.dyoff = tt, grass_length, nrnd, skip, dxoff, dyoff
        dim = 1 + (S - 1) // 4
        self.capacity = dim * dim if capacity is None else capacity
        self.check = check  # (tally, per-tile lists, pass bytes) -> bool


def cases():
    low = dict(pos=(-2.7, 0.2, 0.4), angle=0.6, aspect=1.5, near=0.05, far=7.0, **ALONG_X)
    return [
        # the camera above the batch looking down: the middle tile is completely visible, and nothing in range is dropped by a view test
        Case("above_looking_down", check=lambda t, w, p: t["tiles_all_visible"] >= 1 and t["all_visible_kept"] >= 16 and t["backface_dropped"] == 0
             and t["kept"] == t["all_visible_kept"] + t["frustum_kept"] and t["frustum_dropped"] == 0),
        # the camera inside the batch looking along the ground with a short far_: the frustum drops and keeps blocks, the final dist_less_than(.., far_) drops some
        Case("inside_along_ground", S=20, view=low, tt=0.5, check=lambda t, w, p: t["tiles_all_visible"] == 0 and t["frustum_dropped"] >= 20 and t["frustum_kept"] >= 20
             and t["far_dropped"] >= 1),
        # a ridge with a low camera on one side: the far slope faces away
        Case("ridge", S=20, terrain="ridge", valid=0, tt=0.5, view=dict(pos=(-9.0, 0.5, 0.6), angle=1.0, aspect=1.0, near=0.01, far=100.0, **ALONG_X),
             check=lambda t, w, p: min(t["backface_dropped"], t["backface_kept"], t["not_tested"]) >= 10),
        # every LOD in one tile, the clamp to 5 included: lod_scale*sqrt(dist_sq) reaches 1.25*6.2 at this scale factor
        Case("lods", tiles=[(0, 0), (1, 0)], valid=0, view=dict(pos=(-3.9, -3.9, 0.3), angle=1.0, aspect=1.0, near=0.01, far=100.0, **ALONG_X),
             check=lambda t, w, p: t["max_lods_in_tile"] >= 4 and t["lod_clamped"] >= 1),
        # tiles beyond grass_thresh some of whose blocks would pass the block threshold: the tile-level return decides
        Case("tile_beyond_thresh", tiles=[(x, 0) for x in range(-2, 3)], valid=0, view=dict(pos=(-0.5, 0.0, 0.5), angle=1.0, aspect=1.0, near=0.01, far=100.0, **ALONG_X),
             check=lambda t, w, p: t["tiles_too_far"] >= 1 and t["too_far_tile_blocks_in_range"] >= 1 and t["kept"] >= 16),
        # the wind-pass flag on both sides of 0.5*tt_grass_scale_factor, at two values of the factor
        Case("wind_pass_tt1", tiles=[(x, 0) for x in range(-2, 3)], valid=0, tt=1.0, check=lambda t, w, p: t["wpass0"] >= 1 and t["wpass1"] >= 1),
        Case("wind_pass_tt025", tiles=[(x, 0) for x in range(-2, 3)], valid=0, tt=0.25, view=dict(pos=(0.0, 0.0, 0.5), angle=1.0, aspect=1.0, near=0.01, far=100.0, **ALONG_X),
             check=lambda t, w, p: t["wpass0"] >= 1 and t["wpass1"] >= 1),
        # mixed inputs: empty blocks, a tile with no grass, an ix above num_rnd_grass_blocks, three bins a LOD, skipped tiles, negative tiles, offsets
        Case("mixed_nrnd3", S=20, tiles=[(-3, -2), (-2, -2), (-3, -1), (-2, -1), (-1, -2)], blocks="mixed", nrnd=3, skip=[0, 0, 1, 0, 0], dxoff=5, dyoff=-3, tt=0.5,
             view=dict(pos=(-16.0, -12.0, 2.5), angle=1.1, aspect=1.3, near=0.01, far=60.0, dir=(-0.4, -0.6, -0.5), up=(0.0, 0.0, 1.0)),
             check=lambda t, w, p: t["empty"] >= 5 and t["tiles_no_grass"] == 1 and t["bad_ix"] >= 1 and t["tiles_skipped"] == 1 and t["kept"] >= 20 and t["max_group"] >= 3),
        Case("invalid_view", S=20, valid=0, view=low, tt=0.5, check=lambda t, w, p: t["frustum_dropped"] == 0 and t["tiles_all_visible"] >= 2 and t["kept"] >= 50),
        Case("capacity_small", capacity=5, check=lambda t, w, p: t["beyond_capacity"] >= 10 and max(len(x) for x in w) > 5),
        # 1024 kept blocks in one tile, nearly all at one LOD, two bins: a group holds more than 256 instances, and a bin's running sum spans all 16 chunks of 64 keys
        Case("full_s128", S=128, tiles=[(0, 0)], nrnd=2, tt=1.0, view=dict(pos=(0.0, 0.0, 7.0), angle=1.2, aspect=1.0, near=0.01, far=100.0, **DOWN),
             check=lambda t, w, p: t["kept"] == 1024 and t["max_group"] > 256),
        # 4225 blocks in one tile, more than the 4096 keys the kernel holds in LDS: kept blocks on both sides of that index, in one draw order
        Case("blocks_beyond_lds_s260", S=260, tiles=[(0, 0)], valid=0, view=dict(pos=(0.0, 3.0, 2.5), angle=1.0, aspect=1.0, near=0.01, far=100.0, **ALONG_X),
             check=lambda t, w, p: sum(1 for (x, y, lod, bix) in w[0] if y * 65 + x >= 4096) >= 50 and sum(1 for (x, y, lod, bix) in w[0] if y * 65 + x < 4096) >= 500
             and t["beyond"] >= 500),
    ]


def terrain_of(case):
    """zvals [n, S+2, S+2]: `slope` a gentle plane with a ripple (different in every tile), `ridge` a tent along y whose crest runs through each tile's middle"""
    n, Z = len(case.tiles), case.S + 2
    z = np.zeros((n, Z, Z), f32)
    ii = np.arange(Z, dtype=np.float64)
    for t, (tx, ty) in enumerate(case.tiles):
        if case.terrain == "slope":
            z[t] = (0.01 * ii[None, :] + 0.005 * ii[:, None] + 0.02 * np.sin(0.9 * ii[None, :] + t) * np.cos(0.7 * ii[:, None])).astype(f32)
        else:
            z[t] = (1.5 - 3.0 * np.abs(ii[None, :] / case.S - 0.5) + 0.01 * np.sin(1.3 * ii[:, None] + t)).astype(f32)
    return z


def stats_of(pkg_or_orclib, case, z):
    """mzmin / mzmax over the tile's zvals, radius as tile_t::calc_radius does (half the diagonal of the mesh box)"""
    n = len(case.tiles)
    stats = (pkg_or_orclib.TileStats * n)()
    for t in range(n):
        stats[t].mzmin, stats[t].mzmax = float(z[t].min()), float(z[t].max())
        stats[t].radius = float(f32(0.5 * math.sqrt(8.0 ** 2 + 8.0 ** 2 + float(z[t].max() - z[t].min()) ** 2)))
    return stats


def blocks_of(case, z):
    """[n, dim, dim] grass blocks: ix as add_grass_block_at sets it, the z range of the block's texels.  mixed: every third block empty, the last tile but one without
    grass, one ix beyond num_rnd_grass_blocks"""
    n, S = len(case.tiles), case.S
    dim = 1 + (S - 1) // 4
    gb = np.zeros((n, dim, dim), orclib.GRASS_BLOCK_DTYPE)
    for t, (tx, ty) in enumerate(case.tiles):
        for y in range(dim):
            for x in range(dim):
                zz = z[t, 4 * y:4 * y + 5, 4 * x:4 * x + 5]
                gb[t, y, x] = (((tx * S + x) + 1567 * (ty * S + y)) % 2 ** 32 % case.nrnd + 1, zz.min(), zz.max())
    if case.blocks == "mixed":
        flat = gb.reshape(n, -1)
        flat["ix"][:, ::3] = 0
        flat["ix"][n - 2, :] = 0
        flat["ix"][0, 4] = case.nrnd + 5
    return gb


def scene_of(orc, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    orc.init(ocfg)
    return gm.Scene(orc, ocfg, gm.Params(case.tt, case.grass_length, case.nrnd), case.dxoff, case.dyoff)


def view_of(case):
    v = view_model.make_view(**case.view)
    v.valid = case.valid
    return v


MODEL = {}


def model(orc, case):
    """(scene, zvals, stats, blocks, view, per-tile lists, group_counts, pass, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        z = terrain_of(case)
        stats, gb, sc, v = stats_of(orclib, case, z), blocks_of(case, z), scene_of(orc, case), view_of(case)
        tally = gm.new_tally()
        lists, gc, ps = gm.view_batch(sc, v, case.tiles, z, stats, gb, case.skip, tally)
        tally["beyond_capacity"] = sum(max(0, len(x) - case.capacity) for x in lists)
        MODEL[case.name] = (sc, z, stats, gb, v, lists, gc, ps, tally)
    return MODEL[case.name]


def lib_view(pkg, v):
    lv = pkg.View()
    C.memmove(C.addressof(lv), v.words(), C.sizeof(lv))
    return lv


def configure(pkg, t, case):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    t.set_landscape(pkg.make_landscape(grass_density=1, num_rnd_grass_blocks=case.nrnd))
    t.set_flower_params(pkg.make_flower_params(grass_length=case.grass_length))
    t.set_grass_view_params(pkg.make_grass_view_params(case.tt))


def compare(what, sc, got, lists, want_gc, want_pass, capacity, tail_zero=True):
    """(insts, aux or None, group_counts, counts, pass or None) against the model: every byte, in order; the slots past a tile's count still hold their zeros"""
    insts, aux, gc, counts, ps = got
    ei, ea, ec = gm.pack(sc, lists, capacity)
    assert counts.tolist() == ec.tolist(), f"{what}: counts {counts.tolist()} != {ec.tolist()}"
    assert gc.tobytes() == want_gc.tobytes(), f"{what}: group counts differ at {np.argwhere(gc != want_gc)[:4].tolist()}"
    if ps is not None:
        assert ps.tolist() == want_pass.tolist(), f"{what}: pass {ps.tolist()} != {want_pass.tolist()}"
    for t in range(len(lists)):
        m = capacity if tail_zero else min(len(lists[t]), capacity)
        if insts[t, :m].tobytes() != ei[t, :m].tobytes():
            k = int(np.argwhere((insts[t, :m].view(np.uint32) != ei[t, :m].view(np.uint32)).any(axis=1))[0, 0])
            raise AssertionError(f"{what}: tile {t} instance {k} of {int(ec[t])}: got {insts[t, k]} != {ei[t, k]}")
        if aux is not None:
            bad = np.argwhere(aux[t, :m] != ea[t, :m])
            assert len(bad) == 0, f"{what}: tile {t} aux {int(bad[0, 0])}: {int(aux[t][bad[0, 0]]):#x} != {int(ea[t][bad[0, 0]]):#x}"


def run_dev(pkg, t, tiles, z, stats, gb, lv, cap, nrnd, skip=None, aux=True, want_pass=True, dxoff=0, dyoff=0):
    """the device-pointer form on freshly allocated buffers -> (insts, aux, group_counts, counts, pass)"""
    n = len(tiles)
    bufs = dict(z=t.alloc(z.nbytes).upload(z), st=t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8)), gb=t.alloc(gb.nbytes).upload(gb),
                ins=t.alloc(max(n * cap * 8, 8)).upload(np.zeros(max(n * cap * 2, 2), f32)), gc=t.alloc(n * 6 * nrnd * 4).upload(np.full(n * 6 * nrnd, 7, np.uint32)),
                cn=t.alloc(n * 4).upload(np.full(n, 7, np.uint32)))
    if aux:
        bufs["ax"] = t.alloc(max(n * cap * 4, 4)).upload(np.zeros(max(n * cap, 1), np.uint32))
    if want_pass:
        bufs["ps"] = t.alloc(n).upload(np.full(n, 9, np.uint8))
    if skip is not None:
        bufs["sk"] = t.alloc(n).upload(np.asarray(skip, np.uint8))
    try:
        ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        t.tiles_grass_view_dev(tiles, bufs["z"].ptr, bufs["st"].ptr, bufs["gb"].ptr, lv, cap, bufs["ins"].ptr, bufs["gc"].ptr, bufs["cn"].ptr, ptr("ax"), ptr("ps"), ptr("sk"),
                               dxoff, dyoff)
        insts = bufs["ins"].download(f32, (max(n * cap * 2, 2),))[:n * cap * 2].reshape(n, cap, 2).copy()
        ax = bufs["ax"].download(np.uint32, (max(n * cap, 1),))[:n * cap].reshape(n, cap).copy() if aux else None
        return (insts, ax, bufs["gc"].download(np.uint32, (n, 6, nrnd)).copy(), bufs["cn"].download(np.uint32, (n,)).copy(),
                bufs["ps"].download(np.uint8, (n,)).copy() if want_pass else None)
    finally:
        for b in bufs.values():
            b.free()


def run_case(pkg, t, orc, case, dev=False, aux=True, want_pass=True):
    sc, z, stats, gb, v, lists, gc, ps, tally = model(orc, case)
    assert case.check(tally, lists, ps), (case.name, tally, [len(x) for x in lists])
    configure(pkg, t, case)
    lstats = (pkg.TileStats * len(case.tiles)).from_buffer_copy(stats)
    lv = lib_view(pkg, v)
    if not dev:
        got = t.tiles_grass_view(case.tiles, z, lstats, gb, lv, case.capacity, case.skip, aux, want_pass, case.dxoff, case.dyoff)
    else:
        got = run_dev(pkg, t, case.tiles, z, lstats, gb, lv, case.capacity, case.nrnd, case.skip, aux, want_pass, case.dxoff, case.dyoff)
    compare(case.name + (" (dev)" if dev else ""), sc, got, lists, gc, ps, case.capacity)


def run_resident_chain(pkg, gpu, orc):
    """tiles_create_zvals_dev -> tiles_create_weights_dev -> tiles_grass_view_dev on a 3 x 3 batch at S = 128 on one context with nothing read back in between,
    against the model fed with the oracle's zvals and grass blocks; then one removing tiles_edit_grass_dev stroke and the view again"""
    S, cap, nrnd = 128, 1024, 16
    tiles = GRID3
    n, Z, T = len(tiles), S + 2, S + 1
    bsc, d = gbc.setup(pkg, gpu, orc, tiles)  # the scene and the landscape on both sides; the model's zvals, stats, mesh weights and grass blocks from the oracle
    gpu.set_grass_view_params(pkg.make_grass_view_params(0.25))
    sc = gm.Scene(orc, pkg.make_config(mesh_gen_mode=0, mesh_xy=S), gm.Params(0.25, 0.02, nrnd))
    zc = float(d["z"][tiles.index((0, 0))][64, 64])
    v = view_model.make_view((0.4, -0.3, zc + 0.5), (1.0, 0.4, -0.1), (0.0, 0.0, 1.0), 0.7, 1.6, 0.05, 40.0)
    lv = lib_view(pkg, v)
    x, y = gbc.texel_pos(bsc, (0, 0), 80, 70)
    b_rem = pkg.make_grass_brush((x, y, float(d["z"][tiles.index((0, 0))][70, 80])), 14.5 * float(bsc.DX_VAL), 0, gbm.BSHAPE_CONST_SQ, 1.0)
    bufs = dict(z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), w=gpu.alloc(n * T * T * 4), gb=gpu.alloc(n * 32 * 32 * 12), up=gpu.alloc(n), rg=gpu.alloc(n * 16))
    for k in (1, 2):
        bufs.update({f"ins{k}": gpu.alloc(n * cap * 8).upload(np.zeros(n * cap * 2, f32)), f"ax{k}": gpu.alloc(n * cap * 4).upload(np.zeros(n * cap, np.uint32)),
                     f"gc{k}": gpu.alloc(n * 6 * nrnd * 4), f"cn{k}": gpu.alloc(n * 4), f"ps{k}": gpu.alloc(n)})
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        gpu.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        gpu.tiles_create_weights_dev(tiles, p["z"], p["w"], p["gb"])
        gpu.tiles_grass_view_dev(tiles, p["z"], p["st"], p["gb"], lv, cap, p["ins1"], p["gc1"], p["cn1"], p["ax1"], p["ps1"])
        gpu.tiles_edit_grass_dev(tiles, p["z"], p["st"], b_rem, p["w"], p["gb"], p["up"], p["rg"])
        gpu.tiles_grass_view_dev(tiles, p["z"], p["st"], p["gb"], lv, cap, p["ins2"], p["gc2"], p["cn2"], p["ax2"], p["ps2"])
        got = [(bufs[f"ins{k}"].download(f32, (n, cap, 2)).copy(), bufs[f"ax{k}"].download(np.uint32, (n, cap)).copy(), bufs[f"gc{k}"].download(np.uint32, (n, 6, nrnd)).copy(),
                bufs[f"cn{k}"].download(np.uint32, (n,)).copy(), bufs[f"ps{k}"].download(np.uint8, (n,)).copy()) for k in (1, 2)]
    finally:
        for b in bufs.values():
            b.free()
    t1 = gm.new_tally()
    lists, gc, ps = gm.view_batch(sc, v, tiles, d["z"], d["stats"], d["gb"], None, t1)
    compare("resident chain", sc, got[0], lists, gc, ps, cap)
    assert t1["kept"] >= 100 and t1["frustum_dropped"] >= 100 and t1["tiles_too_far"] >= 1, t1
    upd, _ = gbc.model_stroke(bsc, d, b_rem)
    assert upd.any()
    t2 = gm.new_tally()
    lists2, gc2, ps2 = gm.view_batch(sc, v, tiles, d["z"], d["stats"], d["gb"], None, t2)
    compare("resident chain after the stroke", sc, got[1], lists2, gc2, ps2, cap)
    assert t2["kept"] <= t1["kept"], (t1, t2)
