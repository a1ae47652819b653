"""Tree placement (terra_tiles_place_trees, terra_tiles_place_trees_brush, terra_set_tree_params, terra_set_height_histogram) through the host emulator -- the
driver's one-thread-per-tile form -- against tests/tree_place_model.py, byte for byte, order and counts included; plus the settings, the histogram and the refusals.

test_model_on_oracle_primitives checks the model alone and passes without the feature; every other test needs the new symbols."""
import numpy as np
import pytest

import orclib
import tree_place_cases as tpc
import tree_place_model as tpm

CASES = tpc.cases()


def test_model_on_oracle_primitives(orc):
    """the model's two generators against the oracle's rand_gen_t, negative and out-of-range seeds included, and its veg corners against
    orc.tile_terrain_params at S = 128"""
    for s1, s2 in [(1, 1), (12345, 678), (-2071690107, 1973594324), (2147483647, -2147483648), (657435 * 300 + 243543 * -77, 845631 * -77 + 667239 * 300)]:
        r = tpm.RandGen(s1, s2)
        assert [r.rand() for _ in range(50)] == orc.rand_ints(s1, s2, 50).tolist()
        r = tpm.RandGen(s1, s2)
        assert np.array([r.rand_float() for _ in range(50)], np.float32).tobytes() == orc.rand_floats(s1, s2, 50).tobytes()
        r = tpm.RandGen(s1, s2)
        assert np.array([r.rand_uniform(0.4, 1.0) for _ in range(50)], np.float32).tobytes() == orc.rand_uniforms(s1, s2, np.float32(0.4), np.float32(1.0), 50).tobytes()
    rs = np.random.RandomState(5)
    a1, a2 = rs.randint(-2 ** 31, 2 ** 31, 64).astype(np.int64), rs.randint(-2 ** 31, 2 ** 31, 64).astype(np.int64)
    got = []
    b1, b2 = a1, a2
    for _ in range(6):
        b1, b2, v = tpm.rand_arr(b1, b2)
        got.append(v)
    got = np.array(got).T
    for k in range(64):
        assert got[k].tolist() == orc.rand_ints(int(a1[k]), int(a2[k]), 6).tolist()
    cfg = orclib.make_config(mesh_gen_mode=0)
    orc.init(cfg)
    orc.set_landscape(orclib.make_landscape())
    sc = tpm.Scene(orc, cfg, tpm.TreeParams())
    for tx, ty in tpc.TILES:
        assert np.array(sc.veg_corners(tx, ty), np.float32).tobytes() == orc.tile_terrain_params(tx, ty)[:, :, 0].tobytes()


def test_cases_are_not_vacuous(pkg, orc):
    """on the model alone: every positive case places at least 20 trees, and across the file every outcome occurs at least 10 times"""
    assert pkg.TREE_PLACE_DTYPE == tpm.PLACE_DTYPE
    total = tpm.new_tally()
    for case in CASES:
        want, tally = tpc.model(orc, pkg, case)
        ntrees = sum(len(w) for w in want)
        assert (ntrees >= case.min_trees) if case.positive else (ntrees == 0), (case.name, ntrees)
        assert case.min_trees == 20 or case.name == "skip_val_above_s"  # (one cell per tile there: nine tiles cannot hold twenty trees)
        assert 4 <= len(case.tiles) <= 9
        for k in total:
            total[k] += tally[k]
    for k in ("unselected", "density", "none", "pine", "sh_pine", "palm"):
        assert total[k] >= 10, total
    # the capacity case does cut a tile short, and a brush case reaches four tiles
    by_name = {c.name: c for c in CASES}
    assert max(len(w) for w in tpc.MODEL["capacity_small"][0]) > by_name["capacity_small"].capacity
    assert sum(len(w) > 0 for w in tpc.MODEL["brush_four_tiles"][0]) == 4
    # the kernel's ring of 512 cell numbers wraps: the selected cells of a case are what its tally counts besides "unselected", and some tile has their mean at least
    for name in ("dwarp_exact_s64", "dwarp_approx_s64", "palms_mode3"):
        selected = sum(v for k, v in tpc.MODEL[name][1].items() if k != "unselected")
        assert selected > 512 * len(by_name[name].tiles), (name, selected)
    # the tile with four zero corners is one (on the oracle's own biome field) and gets no tree, its neighbours in the batch do
    cfg = orclib.make_config(mesh_gen_mode=0)
    orc.init(cfg)
    sc = tpm.Scene(orc, cfg, tpm.TreeParams(tree_mode=2))
    assert all(d == 0.0 for d in sc.veg_corners(*tpc.ZERO_CORNERS)) and any(d > 0.0 for d in sc.veg_corners(0, 0))
    assert [len(w) > 0 for w in tpc.MODEL["zero_corners"][0]] == [True, True, True, False]
    # skip_val above S: 17 against 16, and exactly the tile chosen for it stays empty
    cfg16 = orclib.make_config(mesh_gen_mode=0, mesh_xy=16)
    orc.init(cfg16)
    assert tpm.derived(tpm.Scene(orc, cfg16, tpm.TreeParams(**by_name["skip_val_above_s"].tp)), False)[3] == 17
    assert [len(w) for w in tpc.MODEL["skip_val_above_s"][0]] == [1, 1, 0, 1, 1, 1, 1, 1, 1]
    assert len(tpc.MODEL["skip_and_stats"][0][1]) == 0 and len(tpc.MODEL["skip_and_stats"][0][2]) == 0


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    tpc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("name", ["defaults_s64", "skip_and_stats", "capacity_small", "brush_four_tiles"])
def test_cases_dev_entry_point(pkg, emul, orc, name):
    """the device-pointer forms on the emulator's "device" memory"""
    tpc.run_case(pkg, emul, orc, [c for c in CASES if c.name == name][0], dev=True)


def test_histogram(pkg, emul, orc):
    """terra_init_scene keeps estimate_zminmax's 1024 sorted values; the setter takes any length"""
    lib, ctx = emul.lib, emul.ctx
    assert len(emul.get_height_histogram()) == 0
    for mode in (0, 4):
        emul.init_scene(pkg.make_config(mesh_gen_mode=mode))
        st = orc.init(orclib.make_config(mesh_gen_mode=mode))
        want = tpm.height_histogram(orc, st)
        got = emul.get_height_histogram()
        assert len(want) == 1024 and got.tobytes() == want.tobytes()
    two = np.sort(np.concatenate([want, want]))
    emul.set_height_histogram(two)
    assert emul.get_height_histogram().tobytes() == two.tobytes()
    emul.set_height_histogram(np.zeros(0, np.float32))
    assert len(emul.get_height_histogram()) == 0
    assert lib.terra_set_height_histogram(ctx, None, 4) == tpc.ERR_ARG and lib.terra_get_height_histogram(ctx, None, 0, None) == tpc.ERR_ARG
    emul.init_scene(pkg.make_config(mesh_gen_mode=0))  # a new scene estimates again
    assert len(emul.get_height_histogram()) == 1024


def test_tree_params(pkg, emul):
    tp = emul.get_tree_params()  # the reference's defaults
    assert (tp.sm_tree_density, tp.tree_scale, tp.tree_mode, tp.force_tree_class, tp.instanced) == (1.0, 1.0, 1, -1, 0)
    assert abs(tp.tree_density_thresh - 0.55) < 1e-7 and tp.tree_type_rand_zone == 0.0
    emul.set_tree_params(pkg.make_tree_params(sm_tree_density=2.5, tree_mode=3, instanced=1, num_pine_insts=7, num_palm_insts=4, rand_gen_index=9))
    tp = emul.get_tree_params()
    assert (tp.sm_tree_density, tp.tree_mode, tp.instanced, tp.num_pine_insts, tp.num_palm_insts, tp.rand_gen_index) == (2.5, 3, 1, 7, 4, 9)
    bad = [dict(sm_tree_density=-1.0), dict(sm_tree_density=float("nan")), dict(tree_scale=0.0), dict(tree_mode=4), dict(tree_mode=-1), dict(force_tree_class=4),
           dict(force_tree_class=-2), dict(instanced=1), dict(instanced=1, num_pine_insts=3), dict(instanced=1, num_pine_insts=3, num_palm_insts=2, force_tree_class=2)]
    for kw in bad:
        with pytest.raises(pkg.TerraError) as e:
            emul.set_tree_params(pkg.make_tree_params(**kw))
        assert e.value.code == tpc.ERR_ARG, kw
    assert emul.get_tree_params().sm_tree_density == 2.5  # a refused setting changes nothing
    assert emul.lib.terra_set_tree_params(emul.ctx, None) == tpc.ERR_ARG and emul.lib.terra_get_tree_params(emul.ctx, None) == tpc.ERR_ARG


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    tiles = tpc.TILES

    def code(**kw):
        try:
            emul.tiles_place_trees(tiles, 8, **kw)
            return 0
        except pkg.TerraError as e:
            return e.code

    brush = tpc.brush_at(128, (0, 0), 64.0, 64.0, 30.0, False)
    # before terra_init_scene
    assert code() == tpc.ERR_STATE and code(brush=brush) == tpc.ERR_STATE
    emul.init_scene(pkg.make_config(mesh_gen_mode=0))
    # the defaults have tree_mode 1: zero trees, nothing written
    trees, counts = emul.tiles_place_trees(tiles, 8)
    assert not counts.any() and not trees.tobytes().strip(b"\0")
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2, sm_tree_density=0.0))
    assert not emul.tiles_place_trees(tiles, 8)[1].any() and not emul.tiles_place_trees(tiles, 8, brush=brush)[1].any()
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2))
    assert emul.tiles_place_trees(tiles, 8)[1].all() and emul.tiles_place_trees(tiles, 0)[1].all()  # capacity 0: counts only
    # null pointers, n == 0
    txy = np.array(tiles, np.int32)
    cn, tr = np.zeros(4, np.uint32), np.zeros((4, 8), pkg.TREE_PLACE_DTYPE)
    assert lib.terra_tiles_place_trees(ctx, None, 4, 0, 0, None, None, 8, tr.ctypes.data, cn.ctypes.data) == tpc.ERR_ARG
    assert lib.terra_tiles_place_trees(ctx, txy.ctypes.data, 4, 0, 0, None, None, 8, None, cn.ctypes.data) == tpc.ERR_ARG
    assert lib.terra_tiles_place_trees(ctx, txy.ctypes.data, 4, 0, 0, None, None, 8, tr.ctypes.data, None) == tpc.ERR_ARG
    assert lib.terra_tiles_place_trees_brush(ctx, txy.ctypes.data, 4, 0, 0, None, None, None, 1.0, 0, 8, tr.ctypes.data, cn.ctypes.data) == tpc.ERR_ARG
    assert lib.terra_tiles_place_trees(ctx, None, 0, 0, 0, None, None, 8, None, None) == 0
    assert lib.terra_tiles_place_trees_dev(ctx, txy.ctypes.data, 4, 0, 0, None, None, 8, tr.ctypes.data + 2, cn.ctypes.data) == tpc.ERR_ARG
    assert "aligned" in lib.terra_last_error().decode()
    # negative vegetation
    emul.set_landscape(pkg.make_landscape(vegetation=-1.0))
    assert code() == tpc.ERR_ARG
    emul.set_landscape(pkg.make_landscape())
    # a heightmap texture
    pix = emul.alloc(64 * 64 * 2).upload(np.zeros(64 * 64 * 2, np.uint8))
    try:
        emul.hmap_set_dev(pix.ptr, 64, 64, 2)
        assert code() == tpc.ERR_STATE and "heightmap" in lib.terra_last_error().decode()
        assert code(brush=brush) == tpc.ERR_STATE
        emul.hmap_set_dev(None)
        assert code() == 0
    finally:
        emul.hmap_set_dev(None)
        pix.free()
    # XY_MULT_SIZE < 2*ntrees: S = 16 at the defaults (624 > 256), S = 64 at sm_tree_density 8 (5004 > 4096) but not at 6 (3752)
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=16))
    assert code() == tpc.ERR_ARG and "XY_MULT_SIZE = 256 < 2*ntrees = 624" in lib.terra_last_error().decode()
    assert code(brush=tpc.brush_at(16, (0, 0), 8.0, 8.0, 4.0, False)) == tpc.ERR_ARG
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=64))
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2, sm_tree_density=8.0))
    assert code() == tpc.ERR_ARG
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2, sm_tree_density=6.0))
    assert code() == 0
    # int(1/sqrt(sm_tree_density*tree_scale)) beyond an int
    emul.init_scene(pkg.make_config(mesh_gen_mode=0))
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2, sm_tree_density=1e-20, tree_scale=1e-3))
    assert code() == tpc.ERR_ARG and "skip_val" in lib.terra_last_error().decode()
    # n == 0 does nothing, whatever the settings
    assert lib.terra_tiles_place_trees(ctx, None, 0, 0, 0, None, None, 8, None, None) == 0
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert code() == tpc.ERR_ARG
