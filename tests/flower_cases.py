"""Cases of the flowers (terra_tiles_place_flowers[_dev], terra_tiles_edit_flowers[_dev]) shared by test_flowers_emul.py (the host emulator) and
test_gpu_flowers.py (HIP on the MI355X).  Records, aux words and counts are compared byte for byte and in order with tests/flower_model.py.

The weights are an input of the pass, so most cases use synthetic weights on tiny tiles.  The model's result of a case is computed once per process (MODEL)
together with its tally, and every case carries a check on that tally: that it exercises what it is named for."""
import ctypes as C
import importlib

import numpy as np

import flower_model as fm
import grass_brush_cases as gbc
import grass_brush_model as gbm
import orclib
import tree_map_model as tmm
import tree_place_cases as tpc

ERR_ARG, ERR_STATE = -1, -3
REC = 48  # bytes of a record
PATTERN = (0, 1, 127, 128, 191, 192, 255)  # at flower_density 2.0: 127 | 128 is grass_den 0.5, 191 | 192 is num_per_bin 1 | 2
NEG_TILES = [(-1, -1), (-7, -23), (-9, 2), (3, -30)]  # at S = 20 the seeds are tx*20 + 123 and ty*20 + 456: (-7, -23) has both <= 0, (-9, 2) the first, (3, -30) the second


SHORE_TILE = (5, 0)  # beside (6, 0) of tree_place_cases.SHORE, on the island's shore: sand and water (weight 0), thin and full grass in one tile


class Case:
    def __init__(self, name, S=20, tiles=tpc.TILES[:3], weights="full", params=None, capacity=800, skip=None, hist=None, check=None):
        self.name, self.S, self.tiles, self.weights, self.capacity, self.skip, self.hist = name, S, list(tiles), weights, capacity, skip, hist
        self.params = dict(flower_density=2.0) if params is None else dict(params)
        self.check = check  # (tally, per-tile lists) -> bool


def _both(t, w):
    return t["accepted"] >= 20 and t["rejected"] >= 20


def cases():
    return [
        Case("full_s16", S=16, capacity=512, check=lambda t, w: _both(t, w) and t["bin2_cells"] == 3 * 256 and t["bin1_cells"] == 0),
        Case("full_s20", check=lambda t, w: _both(t, w) and t["bin2_cells"] == 3 * 400),
        # every threshold of num_per_bin on a cell boundary; accepted and rejected candidates, both bin counts, colours on both sides of the int -> unsigned conversion
        Case("pattern_s20", weights="pattern", check=lambda t, w: _both(t, w) and min(t["weight0_cells"], t["low_density_cells"], t["bin1_cells"], t["bin2_cells"]) >= 100
             and t["negative_ix"] >= 10 and t["nonnegative_ix"] >= 10),
        Case("fixed_color_s64", S=64, tiles=tpc.TILES[:3], params=dict(flower_density=0.8, flower_color=(0.9, 0.25, 0.5, 1.0)), capacity=4096,
             check=lambda t, w: _both(t, w) and t["bin1_cells"] == 3 * 4096 and t["negative_ix"] == t["nonnegative_ix"] == 0),
        Case("negative_tiles_s20", tiles=NEG_TILES, weights="pattern", check=lambda t, w: _both(t, w) and all(len(x) > 0 for x in w)),
        Case("capacity_small", capacity=50, check=lambda t, w: t["beyond_capacity"] >= 100 and max(len(x) for x in w) > 50),
        Case("skipped_tile", skip=[0, 1, 0], check=lambda t, w: [len(x) > 0 for x in w] == [True, False, True]),
        Case("density_0", params=dict(flower_density=0.0), check=lambda t, w: not any(len(x) for x in w)),
        Case("no_grass", params=dict(flower_density=2.0, no_grass=1), check=lambda t, w: not any(len(x) for x in w)),
        Case("empty_histogram", hist=(), check=_both),  # hthresh = 0.5
        Case("odd_density_s20", weights="pattern", params=dict(flower_density=5.3, grass_length=0.05, grass_width=0.004), capacity=2400,
             check=lambda t, w: _both(t, w) and t["bin_more_cells"] >= 100),  # up to 5 candidates a cell: a chunk of 64 cells holds more than 64 candidates
        # 5 candidates in every cell: 320 in a chunk of 64 cells, more than the 256 the kernel lays out in LDS -- its searching form
        Case("dense_full_s16", S=16, params=dict(flower_density=5.3), capacity=1280, check=lambda t, w: _both(t, w) and t["bin_more_cells"] == 3 * 256),
        Case("shore_s128", S=128, tiles=[SHORE_TILE], weights="oracle", capacity=16384,
             check=lambda t, w: _both(t, w) and min(t["weight0_cells"], t["low_density_cells"], t["bin1_cells"], t["bin2_cells"]) >= 50),
    ]


def weights_of(orc, case):
    """[n, S+1, S+1, 4] bytes.  full: every weight 255; pattern: the grass byte cycles through PATTERN along the texels; oracle: orc.tile_create_weights"""
    n, T = len(case.tiles), case.S + 1
    w = np.zeros((n, T, T, 4), np.uint8)
    if case.weights == "full":
        w[...] = 255
    elif case.weights == "pattern":
        idx = np.arange(T * T).reshape(T, T)
        for t in range(n):
            w[t, :, :, 2] = np.array(PATTERN, np.uint8)[(idx + 3 * t) % len(PATTERN)]
            w[t, :, :, 1] = 255 - w[t, :, :, 2]
    else:
        assert case.weights == "oracle" and case.S == 128
        orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=128))
        orc.set_landscape(orclib.make_landscape(grass_density=1))
        for t, (tx, ty) in enumerate(case.tiles):
            z, _ = orc.tile_create_zvals(tx, ty, 0)
            w[t] = orc.tile_create_weights(tx, ty, z)[0]
    return w


def scene_of(orc, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    orc.init(ocfg)
    return fm.Scene(orc, ocfg, fm.Params(**case.params), hist=case.hist)


MODEL = {}


def model(orc, case):
    """(weights, per-tile lists of (record, cx, cy, ix), tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        w = weights_of(orc, case)
        sc = scene_of(orc, case)
        tally = fm.new_tally()
        want = fm.place(sc, case.tiles, w, case.skip, tally)
        tally["beyond_capacity"] = sum(max(0, len(x) - case.capacity) for x in want)
        MODEL[case.name] = (w, want, tally)
    return MODEL[case.name]


def configure(pkg, t, case):
    """the scene and the settings of a case on the library's side"""
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    t.set_flower_params(pkg.make_flower_params(**case.params))
    if case.hist is not None:
        t.set_height_histogram(np.asarray(case.hist, np.float32))


def pack(want, capacity):
    """the model's lists as the library's arrays: (flowers [n, capacity], aux [n, capacity], counts [n]); what does not fit is dropped, counts keep all"""
    n = len(want)
    flowers, aux, counts = np.zeros((n, capacity), fm.FLOWER_DTYPE), np.zeros((n, capacity), np.uint32), np.zeros(n, np.uint32)
    for t, lst in enumerate(want):
        counts[t] = len(lst)
        for k, (rec, cx, cy, ix) in enumerate(lst[:capacity]):
            flowers[t, k], aux[t, k] = rec, fm.aux_word(cx, cy, ix)
    return flowers, aux, counts


def compare(what, flowers, aux, counts, want, capacity, tail_zero=False):
    """flowers [n, capacity] + aux [n, capacity] (or None) + counts [n] against the model's per-tile lists: every byte of the records the counts name, in order.
    tail_zero: the slots behind them still hold the zeros they were filled with (generation writes nothing past the count)"""
    ef, ea, ec = pack(want, capacity)
    assert counts.tolist() == ec.tolist(), f"{what}: counts {counts.tolist()} != {ec.tolist()}"
    for t in range(len(want)):
        m = capacity if tail_zero else min(len(want[t]), capacity)
        got = np.ascontiguousarray(flowers[t, :m])
        if got.tobytes() != ef[t, :m].tobytes():
            for k in range(m):
                if got[k].tobytes() != ef[t, k].tobytes():
                    raise AssertionError(f"{what}: tile {t} record {k} of {int(ec[t])}: got {got[k]} != {ef[t, k]}")
        if aux is not None:
            bad = np.argwhere(aux[t, :m] != ea[t, :m])
            assert len(bad) == 0, f"{what}: tile {t} aux {int(bad[0, 0])}: {int(aux[t][bad[0, 0]]):#x} != {int(ea[t][bad[0, 0]]):#x}"


def run_case(pkg, t, orc, case, dev=False, aux=True):
    w, want, tally = model(orc, case)
    assert case.check(tally, want), (case.name, tally, [len(x) for x in want])
    configure(pkg, t, case)
    n, cap = len(case.tiles), case.capacity
    if not dev:
        flowers, ax, counts = t.tiles_place_flowers(case.tiles, w, cap, case.skip, aux)
    else:
        bufs = dict(w=t.alloc(w.nbytes).upload(w), fl=t.alloc(n * cap * REC).upload(np.zeros(n * cap * REC, np.uint8)), cn=t.alloc(n * 4))
        if aux:
            bufs["ax"] = t.alloc(n * cap * 4).upload(np.zeros(n * cap, np.uint32))
        if case.skip is not None:
            bufs["sk"] = t.alloc(n).upload(np.asarray(case.skip, np.uint8))
        try:
            ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
            t.tiles_place_flowers_dev(case.tiles, bufs["w"].ptr, cap, bufs["fl"].ptr, bufs["cn"].ptr, ptr("ax"), ptr("sk"))
            flowers = bufs["fl"].download(np.uint8, (n * cap * REC,)).view(pkg.FLOWER_DTYPE).reshape(n, cap)
            ax = bufs["ax"].download(np.uint32, (n, cap)) if aux else None
            counts = bufs["cn"].download(np.uint32, (n,))
        finally:
            for b in bufs.values():
                b.free()
    compare(case.name + (" (dev)" if dev else ""), flowers, ax, counts, want, cap, tail_zero=True)
    return want


# ---- the edit: every case starts from the model's records of BASE (S = 20, the pattern weights) and applies one or two strokes.
# A stroke is (brush, updated [n], ranges [n, 4] or None, weights after the grass brush); the grass brush itself is not part of these cases: an adding stroke sets the
# grass byte of its range to 255 as a full addition does, a removing one leaves the weights alone (clear_within does not read them).
BASE = Case("edit_base_s20", weights="pattern", capacity=800)
# (BASE's tiles hold 152 to 186 records.)  The same tiles with every weight 255 and five candidates a cell: more than 512 records a tile, so that a removal takes
# k_flowers_remove's sweeps of 256 records more than once
DENSE = Case("edit_dense_s20", params=dict(flower_density=5.3), capacity=1100)


class EditCase:
    def __init__(self, name, strokes, generated=None, dxoff=0, dyoff=0, capacity=800, want_status=None, check=None, base=BASE):
        self.name, self.strokes, self.generated, self.dxoff, self.dyoff, self.capacity, self.want_status, self.check = name, strokes, generated, dxoff, dyoff, capacity, want_status, check
        self.base = base  # the case whose records the strokes start from


def _brush(sc, tile, cx, cy, cells, add, shape, dxoff=0, dyoff=0):
    """a brush centred on cell (cx, cy) of `tile`, `cells` cells in radius, in camera space"""
    pkg = importlib.import_module("3dworld_amd")
    S = sc.S
    x = float(np.float32(-sc.X_SCENE_SIZE) + np.float32(sc.DX_VAL) * np.float32(tile[0] * S + cx + dxoff))
    y = float(np.float32(-sc.Y_SCENE_SIZE) + np.float32(sc.DY_VAL) * np.float32(tile[1] * S + cy + dyoff))
    return pkg.make_grass_brush((x, y, 0.0), cells * float(sc.DX_VAL), add, shape, 0.5)


EDIT_NAMES = ("add_inside", "add_reaches_column_S", "add_empty_ranges", "remove_round", "remove_square", "remove_offsets", "not_generated", "two_strokes", "add_small_capacity", "remove_dense")


def edit_case(orc, name):
    by_name = {ec.name: ec for ec in edit_cases(scene_of(orc, BASE))}
    assert tuple(by_name) == EDIT_NAMES
    return by_name[name]


def edit_cases(sc):
    S, tiles = BASE.S, BASE.tiles
    D = [S, S, 0, 0]  # a tile the stroke did not update: the denormalised range of tile_t::add_or_remove_grass_at
    some = lambda key, k=5: (lambda t, st: t[key] >= k)  # noqa: E731
    add = lambda rgs: (_brush(sc, tiles[0], 8, 8, 4.5, 1, 0), [int(r is not D) for r in rgs], rgs)  # noqa: E731
    rem = lambda tile, cx, cy, cells, shape, upd, **kw: (_brush(sc, tile, cx, cy, cells, 0, shape, **kw), upd, None)  # noqa: E731
    return [
        EditCase("add_inside", [add([[3, 4, 12, 13], D, [0, 0, S, S]])], want_status=[1, 0, 1], check=lambda t, st: t["removed"] >= 5 and t["refilled"] >= 5),
        EditCase("add_reaches_column_S", [add([[5, 5, S + 1, 9], [2, 2, 6, S + 1], [1, 1, S, S]])], want_status=[2, 2, 1], check=some("refilled")),
        EditCase("add_empty_ranges", [add([[7, 3, 7, 9], [9, 9, 4, 4], D])], want_status=[0, 0, 0], check=lambda t, st: t["removed"] == t["refilled"] == 0),
        EditCase("remove_round", [rem(tiles[1], 10, 9, 6.5, 1, [0, 1, 0])], want_status=[0, 1, 0], check=some("removed")),
        EditCase("remove_square", [rem(tiles[2], 4, 15, 5.5, 0, [1, 1, 1])], want_status=[1, 1, 1], check=some("removed")),
        EditCase("remove_offsets", [rem(tiles[0], 12, 6, 5.5, 1, [1, 0, 0], dxoff=3, dyoff=-2)], dxoff=3, dyoff=-2, want_status=[1, 0, 0], check=some("removed")),
        EditCase("not_generated", [add([[3, 4, 12, 13], [2, 2, 9, 9], D]), rem(tiles[0], 8, 8, 30.0, 0, [1, 1, 1])], generated=[0, 1, 1], want_status=[0, 1, 1],
                 check=lambda t, st: t["removed"] >= 5),
        EditCase("two_strokes", [add([[3, 4, 12, 13], D, D]), rem(tiles[0], 9, 9, 4.5, 1, [1, 0, 0]), add([[6, 6, 15, 10], D, D])], want_status=[1, 0, 0],
                 check=lambda t, st: t["removed"] >= 10 and t["refilled"] >= 10),
        EditCase("add_small_capacity", [add([[0, 0, S, S], D, D])], capacity=260, want_status=[1, 0, 0], check=some("refilled", 261)),  # the refill does not fit: counts say so
        # a disc in the middle of a tile of DENSE: removed records on either side of M, the survivors' count (test_flowers_emul.py::test_cases_are_not_vacuous)
        EditCase("remove_dense", [rem(tiles[0], 10, 9, 6.5, 1, [1, 1, 1])], base=DENSE, capacity=DENSE.capacity, want_status=[1, 1, 1], check=some("removed", 100)),
    ]


def edit_weights(w, ranges):
    """the weights as a full addition of the grass brush leaves them inside every range: grass 255, the other layers 0 (src/tiled_mesh.cpp:3882-3885)"""
    w = w.copy()
    for t, (xl, yl, xh, yh) in enumerate(ranges):
        if xh > xl and yh > yl:
            w[t, yl:yh, xl:xh, :] = 0
            w[t, yl:yh, xl:xh, 2] = 255
    return w


def run_edit_case(pkg, t, orc, ec, dev=False, aux=True):
    """the strokes of ec through the library and through the model, from the model's records of ec.base; compared after every stroke"""
    BASE = ec.base
    w, base, _ = model(orc, BASE)
    sc = scene_of(orc, BASE)
    configure(pkg, t, BASE)
    n, cap = len(BASE.tiles), ec.capacity
    lists = [list(x) for x in base]
    assert ec.capacity >= max(len(x) for x in base)
    flowers, ax, counts = pack(lists, cap)
    if not aux:
        ax = None
    tally = fm.new_tally()
    status = None
    for k, (brush, updated, ranges) in enumerate(ec.strokes):
        what = f"{ec.name} stroke {k}" + (" (dev)" if dev else "")
        add = bool(brush.add_grass)
        if add:
            w = edit_weights(w, [[min(v, BASE.S) for v in r] for r in ranges])
        before = (flowers.copy(), None if ax is None else ax.copy(), counts.copy())
        upd = np.asarray(updated, np.uint8)
        rg = None if ranges is None else np.asarray(ranges, np.uint32)
        if not dev:
            status = t.tiles_edit_flowers(BASE.tiles, brush, upd, rg, w if add else None, flowers, ax, counts, ec.generated, ec.dxoff, ec.dyoff)
        else:
            bufs = dict(fl=t.alloc(flowers.nbytes).upload(flowers), cn=t.alloc(n * 4).upload(counts), up=t.alloc(n).upload(upd), st=t.alloc(n).upload(np.full(n, 9, np.uint8)))
            if ax is not None:
                bufs["ax"] = t.alloc(ax.nbytes).upload(ax)
            if rg is not None:
                bufs["rg"] = t.alloc(rg.nbytes).upload(rg)
            if add:
                bufs["w"] = t.alloc(w.nbytes).upload(w)
            if ec.generated is not None:
                bufs["ge"] = t.alloc(n).upload(np.asarray(ec.generated, np.uint8))
            try:
                ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
                t.tiles_edit_flowers_dev(BASE.tiles, brush, bufs["up"].ptr, ptr("rg"), ptr("w"), cap, bufs["fl"].ptr, bufs["cn"].ptr, bufs["st"].ptr, ptr("ax"), ptr("ge"),
                                         ec.dxoff, ec.dyoff)
                flowers = bufs["fl"].download(np.uint8, (n * cap * REC,)).view(pkg.FLOWER_DTYPE).reshape(n, cap).copy()
                counts = bufs["cn"].download(np.uint32, (n,)).copy()
                status = bufs["st"].download(np.uint8, (n,)).copy()
                if ax is not None:
                    ax = bufs["ax"].download(np.uint32, (n, cap)).copy()
            finally:
                for b in bufs.values():
                    b.free()
        brush_t = (tuple(brush.pos), brush.radius, add, brush.shape == 0)
        want_status = fm.edit(sc, BASE.tiles, w, lists, brush_t, upd, ranges, ec.generated, ec.dxoff, ec.dyoff, tally)
        assert status.tolist() == want_status, f"{what}: status {status.tolist()} != {want_status}"
        compare(what, flowers, ax, counts, lists, cap)  # (where a refill does not fit: the first `capacity` records, and counts report all)
        for i in range(n):  # a tile the stroke does not touch, or refuses, keeps every byte
            if status[i] != 1:
                assert flowers[i].tobytes() == before[0][i].tobytes() and counts[i] == before[2][i] and (ax is None or ax[i].tobytes() == before[1][i].tobytes()), (what, i)
    if ec.want_status is not None:
        assert status.tolist() == ec.want_status, (ec.name, status.tolist())
    assert ec.check(tally, status), (ec.name, tally)
    return lists


def run_resident_chain(pkg, gpu, orc):
    """zvals -> weights -> tree weights with an all-zero tree map -> flowers -> grass brush adding -> flowers' upkeep -> grass brush removing -> flowers' upkeep on a
    4 x 4 batch at S = 128 on one context, nothing read back in between.  An all-zero tree map is full tree AO: it takes all grass away, so generation finds no
    flowers and every flower at the end comes from the adding stroke's update_subrange on the four tiles that meet under the brush, less what the removal clears."""
    S, cap = 128, 512
    tiles = [(x, y) for y in range(-1, 3) for x in range(-1, 3)]
    n, Z, T = len(tiles), S + 2, S + 1
    sc, d = gbc.setup(pkg, gpu, orc, tiles)  # the scene and the landscape on both sides; the model's zvals, stats, mesh weights and grass blocks from the oracle
    params = dict(flower_density=2.0)
    gpu.set_flower_params(pkg.make_flower_params(**params))
    i11 = tiles.index((1, 1))
    x, y = gbc.texel_pos(sc, (1, 1), 0, 0)  # the corner where (0, 0), (1, 0), (0, 1) and (1, 1) meet
    zc = float(d["z"][i11][0, 0])
    DX = float(sc.DX_VAL)
    b_add = pkg.make_grass_brush((x, y, zc), 9.5 * DX, 1, gbm.BSHAPE_CNST_CIR, 0.12)
    b_rem = pkg.make_grass_brush((x + 3.0 * DX, y - 2.0 * DX, zc), 5.5 * DX, 0, gbm.BSHAPE_CONST_SQ, 0.5)
    bufs = dict(z=gpu.alloc(n * Z * Z * 4), st=gpu.alloc(n * C.sizeof(pkg.TileStats)), mw=gpu.alloc(n * T * T * 4), gb=gpu.alloc(n * 32 * 32 * 12),
                tm=gpu.alloc(n * T * T * 2).upload(np.zeros(n * T * T * 2, np.uint8)), w=gpu.alloc(n * T * T * 4), fl=gpu.alloc(n * cap * REC), ax=gpu.alloc(n * cap * 4),
                cn=gpu.alloc(n * 4), up=gpu.alloc(n), rg=gpu.alloc(n * 16), s1=gpu.alloc(n), s2=gpu.alloc(n))
    try:
        bufs["fl"].upload(np.zeros(n * cap * REC, np.uint8))
        bufs["ax"].upload(np.zeros(n * cap, np.uint32))
        p = {k: b.ptr for k, b in bufs.items()}
        gpu.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        gpu.tiles_create_weights_dev(tiles, p["z"], p["mw"], p["gb"])
        gpu.tiles_tree_weights_dev(n, p["mw"], p["tm"], p["w"])
        gpu.tiles_place_flowers_dev(tiles, p["w"], cap, p["fl"], p["cn"], p["ax"])
        gpu.tiles_edit_grass_dev(tiles, p["z"], p["st"], b_add, p["w"], p["gb"], p["up"], p["rg"])
        gpu.tiles_edit_flowers_dev(tiles, b_add, p["up"], p["rg"], p["w"], cap, p["fl"], p["cn"], p["s1"], p["ax"])
        gpu.tiles_edit_grass_dev(tiles, p["z"], p["st"], b_rem, p["w"], p["gb"], p["up"], p["rg"])
        gpu.tiles_edit_flowers_dev(tiles, b_rem, p["up"], p["rg"], p["w"], cap, p["fl"], p["cn"], p["s2"], p["ax"])
        flowers = bufs["fl"].download(np.uint8, (n * cap * REC,)).view(pkg.FLOWER_DTYPE).reshape(n, cap)
        aux, counts = bufs["ax"].download(np.uint32, (n, cap)), bufs["cn"].download(np.uint32, (n,))
        st1, st2 = bufs["s1"].download(np.uint8, (n,)), bufs["s2"].download(np.uint8, (n,))
        weights = bufs["w"].download(np.uint8, (n, T, T, 4))
    finally:
        for b in bufs.values():
            b.free()
    # the model: the same chain on the oracle's tiles
    fsc = fm.Scene(orc, pkg.make_config(mesh_gen_mode=0, mesh_xy=S), fm.Params(**params))
    d["w"] = tmm.tree_weights(d["w"], np.zeros((n, T, T, 2), np.uint8))
    tally = fm.new_tally()
    lists = fm.place(fsc, tiles, d["w"], None, tally)
    assert not any(len(x) for x in lists)
    upd, rg = gbc.model_stroke(sc, d, b_add)
    want1 = fm.edit(fsc, tiles, d["w"], lists, (tuple(b_add.pos), b_add.radius, True, False), upd, rg, tally=tally)
    after_add = [len(x) for x in lists]
    upd, rg = gbc.model_stroke(sc, d, b_rem)
    want2 = fm.edit(fsc, tiles, d["w"], lists, (tuple(b_rem.pos), b_rem.radius, False, True), upd, rg, tally=tally)
    assert (weights == d["w"]).all()
    assert st1.tolist() == want1 and st2.tolist() == want2 and sum(want1) == 4 and sum(want2) >= 2
    compare("resident chain", flowers, aux, counts, lists, cap)
    assert tally["refilled"] >= 100 and tally["removed"] >= 10 and max(after_add) <= cap and sum(len(x) for x in lists) < sum(after_add)
