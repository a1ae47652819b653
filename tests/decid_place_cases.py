"""Cases of deciduous tree placement (terra_tiles_place_decid_trees / terra_tiles_place_decid_trees_brush) shared by test_decid_place_emul.py (the host emulator) and
test_gpu_decid_place.py (HIP on the MI355X).  Every record is compared byte for byte with tests/decid_place_model.py, order and counts included.

A case's zvals are the oracle's grid of the tile (orc.gen_grid at the tile's origin, S + 2 cells a side, glaciated: what tile_t::create_zvals evaluates), with seeded
waves added where the case wants slopes the scene does not offer; its stats are the sub-block loop of src/tiled_mesh.cpp:517-541 on those zvals, in NumPy.  Both
are inputs: the library and the model get the same arrays.  The model's result of a case is computed once per process (MODEL) together with its tally of outcomes,
which test_decid_place_emul.py::test_cases_are_not_vacuous checks."""
import ctypes as C

import numpy as np

import decid_place_model as dpm
import orclib
import tree_place_cases as tpc
import tree_place_model as tpm

ERR_ARG, ERR_STATE = -1, -3
TILES = tpc.TILES
REC = 36  # bytes of a record


class Case:
    def __init__(self, name, S=128, mode=0, tiles=TILES, tp=None, dp=None, xoff2=0, yoff2=0, capacity=600, skip=None, zranges=None, brush=None, vegetation=1.0,
                 water_h_off=0.0, hist="scene", positive=True, relh_adj_tex=0.0, stats=True, synth=None):
        self.name, self.S, self.mode, self.tiles, self.xoff2, self.yoff2, self.capacity = name, S, mode, tiles, xoff2, yoff2, capacity
        self.tp = dict(tp or {})           # tree_mode 1, the reference's default, has deciduous trees
        self.dp = dict(num_trees=400)
        self.dp.update(dp or {})
        self.skip, self.zranges, self.brush, self.vegetation, self.water_h_off, self.hist, self.positive = skip, zranges, brush, vegetation, water_h_off, hist, positive
        self.relh_adj_tex = relh_adj_tex
        self.stats = stats                 # False: the call gets neither stats nor zvals
        self.synth = synth                 # (seed, amplitude): seeded waves added to the scene's heights
        self.zranges = zranges             # {tile index: (mzmin, mzmax) in units of zmax_est}: the z range of that tile's stats is replaced


def cases():
    b = tpc.brush_at
    four = [(0, 0), (1, 0), (-1, 0), (0, 1)]
    return [
        Case("defaults_s128"),
        Case("mode3_shore", tp=dict(tree_mode=3), tiles=tpc.SHORE, water_h_off=0.1, relh_adj_tex=-0.03),
        Case("dwarp_s64", S=64, mode=4, dp=dict(num_trees=200)),
        Case("odd_s20", S=20, dp=dict(num_trees=60), tiles=tpc.TILES9, synth=(13, 0.25)),                     # 400 cells: not a multiple of the kernel's 256
        Case("defaults_s256", S=256, capacity=1500),
        Case("tree_scale_half", tp=dict(tree_scale=0.5), dp=dict(num_trees=1200), tiles=tpc.TILES9),  # skip_val 2
        Case("offsets_rgi", xoff2=37, yoff2=-21, tp=dict(rand_gen_index=5)),
        Case("slope_thresh", dp=dict(num_trees=400, tree_slope_thresh=1.0), synth=(11, 0.2)),
        Case("branch_size", dp=dict(num_trees=400, tree_slope_thresh=2.0, branch_size=(0.6, 1.0, 1.7, 2.5, 3.2)), synth=(12, 0.5)),
        Case("shared_100", dp=dict(num_trees=400, num_shared_trees=100)),
        Case("shared_3", dp=dict(num_trees=400, num_shared_trees=3)),                         # num_per_type = max(1, 0), min(.., size - 1)
        Case("skip_and_stats", skip=[0, 1, 0, 0], zranges={2: (-1.3, -1.1), 3: (0.5, 0.9)}),  # tile 1 skipped, tile 2 under water, tile 3 above the 0.6 line
        Case("no_stats", stats=False),
        Case("capacity_small", capacity=25),
        Case("num_trees_0", dp=dict(num_trees=0), positive=False),
        Case("tree_mode_2", tp=dict(tree_mode=2), positive=False),
        Case("vegetation_0", vegetation=0.0, positive=False),
        Case("hist_empty", hist=np.zeros(0, np.float32)),
        Case("hist_2048", hist="double"),
        Case("brush_round", brush=b(128, (0, 0), 64.3, 70.1, 40.0, False), tiles=four),
        Case("brush_square_four_tiles", brush=b(128, (0, 0), 0.4, -0.3, 48.0, True, -128, 64), tiles=[(0, 0), (-1, 0), (0, -1), (-1, -1), (1, 1)], xoff2=-128, yoff2=64),
        Case("brush_radius_0", brush=b(128, (0, 0), 64.0, 64.0, 0.0, False), tiles=four),     # the whole tile, no coverage test
    ]


def tile_zvals(orc, state, case):
    """[n, S+2, S+2]: the heights of the case's tiles"""
    S, Z = case.S, case.S + 2
    out = np.zeros((len(case.tiles), Z, Z), np.float32)
    for t, (tx, ty) in enumerate(case.tiles):
        out[t] = orc.gen_grid(np.float32(tx * S - S // 2), np.float32(ty * S - S // 2), state.DX_VAL, state.DY_VAL, Z, Z, glaciate=1)
        if case.synth is not None:  # the scene's heights under three seeded waves about two thirds of a tile long: slopes on both sides of the slope threshold
            seed, amp = case.synth
            rs = np.random.RandomState(seed + 17 * t)
            y, x = np.mgrid[0:Z, 0:Z].astype(np.float64)
            z = np.zeros((Z, Z))
            for _ in range(3):
                ang, ph = rs.uniform(0, 6.28), rs.uniform(0, 6.28)
                k = 2 * np.pi * 1.5 / Z
                z += np.sin(k * (np.cos(ang) * x + np.sin(ang) * y) + ph)
            out[t] = (out[t].astype(np.float64) + amp * z).astype(np.float32)
    return out


def tile_stats(pkg, zvals, S, zranges=None, zmax_est=1.0):
    """the sub-block loop of tile_t::create_zvals (src/tiled_mesh.cpp:517-541) on zvals [n, S+2, S+2]: sub_zmin / sub_zmax / mzmin / mzmax (the rest stays zero)"""
    n, zvsize = len(zvals), S + 2
    bs = zvsize // 4
    st = (pkg.TileStats * n)()
    for t in range(n):
        for yy in range(4):
            for xx in range(4):
                blk = zvals[t, yy * bs:(yy + 1) * bs + 1, xx * bs:(xx + 1) * bs + 1]  # x_end, y_end inclusive
                st[t].sub_zmin[4 * yy + xx], st[t].sub_zmax[4 * yy + xx] = blk.min(), blk.max()
        st[t].mzmin, st[t].mzmax = min(st[t].sub_zmin), max(st[t].sub_zmax)
        if zranges and t in zranges:
            st[t].mzmin, st[t].mzmax = np.float32(zranges[t][0] * zmax_est), np.float32(zranges[t][1] * zmax_est)
    return st


def _oracle_config(case):
    ocfg = orclib.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S)
    ocfg.water_h_off, ocfg.relh_adj_tex = case.water_h_off, case.relh_adj_tex
    return ocfg


def _hist(orc, case):
    if isinstance(case.hist, np.ndarray):
        return case.hist
    if case.hist == "double":  # an engine that estimated twice: the reference appends and sorts again
        h = tpm.height_histogram(orc, orc.state())
        return np.sort(np.concatenate([h, h]))
    return None


MODEL = {}


def model(orc, pkg, case):
    """(records per tile, tally, zvals, stats) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = _oracle_config(case)
        state = orc.init(ocfg)
        sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**case.tp), vegetation=case.vegetation, hist=_hist(orc, case))
        zvals = stats = None
        if case.stats:
            zvals = tile_zvals(orc, state, case)
            stats = tile_stats(pkg, zvals, case.S, case.zranges, float(state.zmax_est))
        tally = dpm.new_tally()
        want = dpm.place(sc, dpm.DecidParams(**case.dp), case.tiles, case.xoff2, case.yoff2, case.skip, stats, zvals, case.brush, tally)
        MODEL[case.name] = (want, tally, zvals, stats)
    return MODEL[case.name]


def configure(pkg, t, orc, case):
    """the scene and the settings of a case on the library's side"""
    cfg = pkg.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S)
    cfg.water_h_off, cfg.relh_adj_tex = case.water_h_off, case.relh_adj_tex
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(vegetation=case.vegetation))
    t.set_tree_params(pkg.make_tree_params(**case.tp))
    t.set_decid_params(pkg.make_decid_params(**case.dp))
    if not isinstance(case.hist, str) or case.hist == "double":
        orc.init(_oracle_config(case))
        t.set_height_histogram(_hist(orc, case))


def compare(what, trees, counts, want, capacity):
    """trees [n, capacity] + counts [n] against the model's per-tile lists"""
    assert [int(c) for c in counts] == [len(w) for w in want], f"{what}: counts {counts.tolist()} != {[len(w) for w in want]}"
    for t, w in enumerate(want):
        m = min(len(w), capacity)
        if m == 0:
            continue
        exp = np.array(w[:m], dpm.PLACE_DTYPE)
        got = np.ascontiguousarray(trees[t, :m])
        if got.tobytes() != exp.tobytes():
            for k in range(m):
                if got[k].tobytes() != exp[k].tobytes():
                    raise AssertionError(f"{what}: tile {t} tree {k} of {len(w)}: got {got[k]} != {exp[k]}")


def run_case(pkg, t, orc, case, dev=False):
    want, _, zvals, stats = model(orc, pkg, case)
    configure(pkg, t, orc, case)
    n, cap = len(case.tiles), case.capacity
    if not dev:
        trees, counts = t.tiles_place_decid_trees(case.tiles, cap, case.xoff2, case.yoff2, case.skip, stats, zvals, case.brush)
    else:
        bufs = dict(tr=t.alloc(n * cap * REC), cn=t.alloc(n * 4))
        if case.skip is not None:
            bufs["sk"] = t.alloc(n).upload(np.asarray(case.skip, np.uint8))
        if stats is not None:
            bufs["st"] = t.alloc(C.sizeof(stats)).upload(np.frombuffer(stats, np.uint8))
            bufs["z"] = t.alloc(zvals.nbytes).upload(zvals)
        try:
            bufs["tr"].upload(np.zeros(n * cap * REC, np.uint8))
            ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
            t.tiles_place_decid_trees_dev(case.tiles, cap, bufs["tr"].ptr, bufs["cn"].ptr, case.xoff2, case.yoff2, ptr("sk"), ptr("st"), ptr("z"), case.brush)
            trees = bufs["tr"].download(np.uint8, (n * cap * REC,)).view(pkg.DECID_PLACE_DTYPE).reshape(n, cap)
            counts = bufs["cn"].download(np.uint32, (n,))
        finally:
            for b in bufs.values():
                b.free()
    compare(case.name + (" (dev)" if dev else ""), trees, counts, want, cap)
    # records past the count are not written
    for i in range(n):
        assert not trees[i, min(int(counts[i]), cap):].tobytes().strip(b"\0"), f"{case.name}: tile {i}: records past the count were written"
    ntrees = sum(len(w) for w in want)
    assert (ntrees >= 20) if case.positive else (ntrees == 0), (case.name, ntrees)
    return want
