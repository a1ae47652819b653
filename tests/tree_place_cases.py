"""Cases of tree placement (terra_tiles_place_trees / terra_tiles_place_trees_brush) shared by test_tree_place_emul.py (the host emulator) and
test_gpu_tree_place.py (HIP on the MI355X).  Every record is compared byte for byte with tests/tree_place_model.py, order and counts included.

The model's result of a case is computed once per process (MODEL) and shared by the tests that need it; the tally of outcomes it keeps is what
test_tree_place_emul.py::test_cases_are_not_vacuous checks."""
import ctypes as C

import numpy as np

import orclib
import tree_place_model as tpm

ERR_ARG, ERR_STATE = -1, -3
TILES = [(-2, -1), (0, 0), (1, -2), (-1, 2)]              # mixed-sign coordinates
SHORE = [(0, 0), (6, 0), (0, -6), (-4, 4), (5, -3), (-6, -1)]  # from an island's top to its shore (the island term's period is 2*pi*1000 cells)
ZERO_CORNERS = (-30, -40)  # all four veg corners of this tile are 0 in the default scene at S = 128 (:440)
TILES9 = [(x, y) for y in (-2, -1, 0) for x in (-1, 0, 1)]  # a 3 x 3 block around the origin


class Case:
    def __init__(self, name, S=128, mode=0, tiles=TILES, tp=None, xoff2=0, yoff2=0, capacity=400, skip=None, zranges=None, brush=None, vegetation=1.0,
                 water_h_off=0.0, hist="scene", positive=True, islands=True, relh_adj_tex=0.0, min_trees=20):
        self.name, self.S, self.mode, self.tiles, self.xoff2, self.yoff2, self.capacity = name, S, mode, tiles, xoff2, yoff2, capacity
        self.tp = dict(tree_mode=2)
        self.tp.update(tp or {})
        self.skip, self.zranges, self.brush, self.vegetation, self.water_h_off, self.hist, self.positive = skip, zranges, brush, vegetation, water_h_off, hist, positive
        self.relh_adj_tex, self.min_trees = relh_adj_tex, min_trees  # min_trees: what a positive case places at the least
        self.hmap = None if islands else list(orclib.HMAP_DEFAULT)  # islands: the synthetic scene's sine_mag / sine_bias term (make_config's default)


def brush_at(S, tile, fx, fy, r_cells, is_square, xoff2=0, yoff2=0):
    """a brush centred on the (fractional) cell (fx, fy) of a tile with a radius of r_cells cells, in the scene of make_config (X_SCENE_SIZE = 4) and in the
    frame of the local indices (x1 - xoff2)"""
    dx = 8.0 / S
    return ((np.float32(-4.0 + dx * (tile[0] * S - xoff2 + fx)), np.float32(-4.0 + dx * (tile[1] * S - yoff2 + fy)), np.float32(0.0)), np.float32(r_cells * dx), is_square)


def cases():
    cs = [
        Case("defaults_s128"),
        Case("defaults_s64", S=64),
        Case("defaults_s256", S=256),
        Case("odd_s20", S=20, tp=dict(sm_tree_density=0.3), tiles=TILES9),               # 400 cells: not a multiple of the kernel's 256
        Case("dwarp_exact_s64", S=64, mode=4, tp=dict(sm_tree_density=2.0)),           # ntrees_mult = 0.0156 <= 0.025: get_exact_zval per tree
        Case("dwarp_approx_s64", S=64, mode=4, tp=dict(sm_tree_density=4.0)),          # 0.031 > 0.025: the glaciated height field
        Case("skip_val_2", tp=dict(sm_tree_density=0.2), tiles=TILES9),                # int(1/sqrt(0.2)) = 2: every other cell, the running sums
        # skip_val = int(1/sqrt(2.66e-5*124)) = 17 > S = 16: cell (0, 0) alone, so at most one tree per tile (eight of these nine have one, (5, -19) has none),
        # and maybe_add_tree's offsets are 0.5*17*DX_VAL wide; ntrees <= 127, 2*127 <= 256
        Case("skip_val_above_s", S=16, tp=dict(sm_tree_density=2.66e-5, tree_scale=124.0), min_trees=8,
             tiles=[(-17, -19), (7, -19), (5, -19), (6, -18), (7, -18), (-19, -17), (6, -17), (9, -17), (-4, -17)]),
        Case("zero_corners", tiles=TILES[:3] + [ZERO_CORNERS]),
        Case("palms_mode3", tp=dict(tree_mode=3, sm_tree_density=3.0), tiles=SHORE, water_h_off=0.1, relh_adj_tex=-0.03),
        Case("rand_zone_mode3", tp=dict(tree_mode=3, tree_type_rand_zone=0.05, sm_tree_density=3.0), tiles=SHORE, water_h_off=0.1, relh_adj_tex=-0.03),
        Case("force_class_palm", tp=dict(force_tree_class=tpm.TREE_CLASS_PALM)),
        Case("force_class_decid", tp=dict(force_tree_class=tpm.TREE_CLASS_DECID)),
        Case("instanced", tp=dict(tree_mode=3, sm_tree_density=3.0, instanced=1, num_pine_insts=3, num_palm_insts=2), tiles=SHORE, water_h_off=0.1, relh_adj_tex=-0.03),
        Case("offsets_rgi", xoff2=37, yoff2=-21, tp=dict(rand_gen_index=5)),
        Case("skip_and_stats", skip=[0, 1, 0, 0], zranges=[(-0.5, 0.4), (-0.5, 0.4), (-8.0, -6.5), (-0.5, 0.4)]),  # tile 1 skipped, tile 2 under water (water_plane_z = -5.89)
        Case("capacity_small", capacity=25),
        Case("vegetation_0", vegetation=0.0, positive=False),
        Case("hist_empty", hist=np.zeros(0, np.float32)),
        Case("hist_2048", hist="double"),
        Case("brush_round", brush=brush_at(128, (0, 0), 64.3, 70.1, 40.0, False), tiles=[(0, 0), (1, 0), (-1, 0), (0, 1)]),
        Case("brush_square", brush=brush_at(128, (0, 0), 30.0, 30.0, 25.0, True), tiles=[(0, 0), (1, 0), (-1, 0), (0, 1)]),
        Case("brush_four_tiles", brush=brush_at(128, (0, 0), 0.4, -0.3, 48.0, False, -128, 64), tiles=[(0, 0), (-1, 0), (0, -1), (-1, -1), (1, 1)], xoff2=-128, yoff2=64),
        Case("brush_radius_0", brush=brush_at(128, (0, 0), 64.0, 64.0, 0.0, False), positive=False),
    ]
    return cs


def configure(pkg, t, orc, case):
    """the scene and the settings of a case on both sides -> the model's Scene"""
    cfg = pkg.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S, hmap=case.hmap)
    ocfg = orclib.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S, hmap=case.hmap)
    cfg.water_h_off = ocfg.water_h_off = case.water_h_off
    cfg.relh_adj_tex = ocfg.relh_adj_tex = case.relh_adj_tex
    t.init_scene(cfg)
    orc.init(ocfg)
    t.set_landscape(pkg.make_landscape(vegetation=case.vegetation))
    t.set_tree_params(pkg.make_tree_params(**case.tp))
    hist = None
    if isinstance(case.hist, np.ndarray):
        hist = case.hist
    elif case.hist == "double":  # an engine that estimated twice: the reference appends and sorts again
        h = tpm.height_histogram(orc, orc.state())
        hist = np.sort(np.concatenate([h, h]))
    if hist is not None:
        t.set_height_histogram(hist)
    return tpm.Scene(orc, cfg, tpm.TreeParams(**case.tp), vegetation=case.vegetation, hist=hist)


MODEL = {}


def model(orc, pkg, case):
    """(records per tile, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = orclib.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S, hmap=case.hmap)
        ocfg.water_h_off, ocfg.relh_adj_tex = case.water_h_off, case.relh_adj_tex
        orc.init(ocfg)
        hist = case.hist if isinstance(case.hist, np.ndarray) else None
        if isinstance(case.hist, str) and case.hist == "double":
            h = tpm.height_histogram(orc, orc.state())
            hist = np.sort(np.concatenate([h, h]))
        sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**case.tp), vegetation=case.vegetation, hist=hist)
        tally = tpm.new_tally()
        MODEL[case.name] = (tpm.place(sc, case.tiles, case.xoff2, case.yoff2, case.skip, case.zranges, case.brush, tally), tally)
    return MODEL[case.name]


def make_stats(pkg, zranges):
    if zranges is None:
        return None
    st = (pkg.TileStats * len(zranges))()
    for i, (lo, hi) in enumerate(zranges):
        st[i].mzmin, st[i].mzmax = lo, hi
    return st


def compare(what, trees, counts, want, capacity):
    """trees [n, capacity] + counts [n] against the model's per-tile lists"""
    assert [int(c) for c in counts] == [len(w) for w in want], f"{what}: counts {counts.tolist()} != {[len(w) for w in want]}"
    for t, w in enumerate(want):
        m = min(len(w), capacity)
        if m == 0:
            continue
        exp = np.array(w[:m], tpm.PLACE_DTYPE)
        got = np.ascontiguousarray(trees[t, :m])
        if got.tobytes() != exp.tobytes():
            for k in range(m):
                if got[k].tobytes() != exp[k].tobytes():
                    raise AssertionError(f"{what}: tile {t} tree {k} of {len(w)}: got {got[k]} != {exp[k]}")


def run_case(pkg, t, orc, case, dev=False):
    want, _ = model(orc, pkg, case)
    configure(pkg, t, orc, case)
    n, cap = len(case.tiles), case.capacity
    stats = make_stats(pkg, case.zranges)
    if not dev:
        trees, counts = t.tiles_place_trees(case.tiles, cap, case.xoff2, case.yoff2, case.skip, stats, case.brush)
    else:
        bufs = dict(tr=t.alloc(n * cap * 40), cn=t.alloc(n * 4))
        if case.skip is not None:
            bufs["sk"] = t.alloc(n).upload(np.asarray(case.skip, np.uint8))
        if stats is not None:
            bufs["st"] = t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8))
        try:
            bufs["tr"].upload(np.zeros(n * cap * 40, np.uint8))
            t.tiles_place_trees_dev(case.tiles, cap, bufs["tr"].ptr, bufs["cn"].ptr, case.xoff2, case.yoff2, bufs["sk"].ptr if "sk" in bufs else None,
                                    bufs["st"].ptr if "st" in bufs else None, case.brush)
            trees = bufs["tr"].download(np.uint8, (n * cap * 40,)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap)
            counts = bufs["cn"].download(np.uint32, (n,))
        finally:
            for b in bufs.values():
                b.free()
    compare(case.name + (" (dev)" if dev else ""), trees, counts, want, cap)
    # records past the count are not written
    for i in range(n):
        assert not trees[i, min(int(counts[i]), cap):].tobytes().strip(b"\0"), f"{case.name}: tile {i}: records past the count were written"
    if case.positive:
        assert sum(len(w) for w in want) >= case.min_trees
    return want
