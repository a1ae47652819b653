"""Deciduous tree placement (terra_tiles_place_decid_trees, terra_tiles_place_decid_trees_brush, terra_set_decid_params) through the host emulator -- the driver's
one-thread-per-tile form -- against tests/decid_place_model.py, byte for byte, order and counts included; plus the settings and the refusals.

test_model_on_oracle_primitives checks the model alone and passes without the feature; every other test needs the new symbols."""
import ctypes as C

import numpy as np
import pytest

import decid_place_cases as dpc
import decid_place_model as dpm
import orclib
import tree_place_model as tpm

CASES = dpc.cases()
BY_NAME = {c.name: c for c in CASES}


def test_model_on_oracle_primitives(orc):
    """the model's pieces against the oracle: the array form of the seeding and selection against orc.rand_ints on the wrapped seeds, get_avg_veg against
    orc.tile_terrain_params, the tile heights the cases use against orc.tile_create_zvals and the NumPy sub-block loop against its stats, at S = 128"""
    cfg = orclib.make_config(mesh_gen_mode=0)
    state = orc.init(cfg)
    orc.set_landscape(orclib.make_landscape())
    sc = tpm.Scene(orc, cfg, tpm.TreeParams())
    for (i, j, rgi) in [(0, 0, 0), (300, -77, 0), (-255, 129, 5), (123456, -654321, -3)]:
        s1, s2 = tpm.wrap32(805306457 * i + 12582917 * j + 100663319 * rgi), tpm.wrap32(6291469 * j + 3145739 * i + 1572869 * rgi)
        r = tpm.RandGen(s1, s2)
        r.rand_mix()
        v = r.rand_seed_mix()
        a = orc.rand_ints(s1, s2, 1).tolist()                      # rand_mix: one value, then the swap
        r2 = tpm.RandGen(s1, s2)
        assert r2.rand() == a[0]
        b1, b2, _ = tpm.rand_arr(np.array([s1], np.int64), np.array([s2], np.int64))
        b1, b2 = b2, b1
        b1, b2, v1 = tpm.rand_arr(b1, b2)
        b1, b2 = b2, b1
        b1, b2, v2 = tpm.rand_arr(b1, b2)
        assert int(tpm.wrap32(v1 + v2)[0]) == v and (int(b1[0]), int(b2[0])) == (r.rseed1, r.rseed2)
        # the swapped generator's values are the oracle's for the swapped seeds
        assert int(v1[0]) == orc.rand_ints(int(r2.rseed2), int(r2.rseed1), 1)[0]
    for tx, ty in dpc.TILES:
        p = orc.tile_terrain_params(tx, ty)[:, :, 0]
        want = np.float32(np.float32(0.25) * np.float32(np.float32(np.float32(p[0, 0] + p[0, 1]) + p[1, 0]) + p[1, 1]))
        assert dpm.get_avg_veg(sc, tx, ty) == want
    case = BY_NAME["defaults_s128"]
    zvals = dpc.tile_zvals(orc, state, case)

    class P:
        TileStats = orclib.TileStats
    stats = dpc.tile_stats(P, zvals, 128)
    for t, (tx, ty) in enumerate(case.tiles):
        z, st = orc.tile_create_zvals(tx, ty)
        assert z.tobytes() == zvals[t].tobytes()
        assert list(st.sub_zmin) == list(stats[t].sub_zmin) and list(st.sub_zmax) == list(stats[t].sub_zmax) and (st.mzmin, st.mzmax) == (stats[t].mzmin, stats[t].mzmax)
    # get_tree_class_from_height's second argument: without pine_trees_only the lowlands are deciduous at tree_mode 3
    sc3 = tpm.Scene(orc, cfg, tpm.TreeParams(tree_mode=3))
    zs = np.linspace(float(sc3.water_plane_z), float(sc3.zmax_est), 200).astype(np.float32)
    low = [z for z in zs if sc3.get_tree_class_from_height(z, 0) == tpm.TREE_CLASS_DECID]
    assert len(low) >= 10 and all(sc3.get_tree_class_from_height(z, 1) == tpm.TREE_CLASS_NONE for z in low)


def test_cases_are_not_vacuous(pkg, orc):
    """on the model alone: every positive case places at least 20 trees, every other none, and across the file every outcome occurs at least 10 times"""
    assert pkg.DECID_PLACE_DTYPE == dpm.PLACE_DTYPE
    total = dpm.new_tally()
    for case in CASES:
        want, tally, _, stats = dpc.model(orc, pkg, case)
        ntrees = sum(len(w) for w in want)
        assert (ntrees >= 20) if case.positive else (ntrees == 0), (case.name, ntrees)
        assert 4 <= len(case.tiles) <= 9
        for k in total:
            total[k] += tally[k]
    for k in dpm.OUTCOMES:
        assert total[k] >= 10, total
    M = dpc.MODEL
    # the slope cases run the test on every tile, keep and drop; the defaults run it on (1, -2) alone
    for name in ("slope_thresh", "branch_size", "odd_s20"):
        assert all(dpm.mesh_dz(s) > 1.0 for s in M[name][3]) and M[name][1]["slope_kept"] >= 10 and M[name][1]["slope_dropped"] >= 10, name
    assert [bool(dpm.mesh_dz(s) > 1.0) for s in M["defaults_s128"][3]] == [False, False, True, False]
    assert M["no_stats"][1]["slope_kept"] == 0 and M["defaults_s128"][1]["slope_kept"] == len(M["defaults_s128"][0][2])
    # a lowered position: some kept tree stands below its get_exact_zval height
    assert any(r["pos"][2] < r["zval"] for w in M["slope_thresh"][0] for r in w)
    # the capacity case does cut a tile short; the square brush reaches four tiles; radius 0 takes whole tiles without the coverage test
    assert max(len(w) for w in M["capacity_small"][0]) > BY_NAME["capacity_small"].capacity
    assert [len(w) > 0 for w in M["brush_square_four_tiles"][0]] == [True, True, True, True, False]
    assert M["brush_radius_0"][1]["coverage"] == 0 and all(len(w) > 300 for w in M["brush_radius_0"][0])
    # both of the kernel's rings of 512 wrap: a record has been through both, and four tiles there hold more than 512; at the defaults the first ring does on the mean tile
    # (the selected cells that pass the vegetation test: every outcome but "unselected" and "veg"; slope_kept counts records a second time)
    assert all(len(w) > 512 for w in M["brush_radius_0"][0][:4])
    ta = M["defaults_s128"][1]
    first = sum(v for k, v in ta.items() if k not in ("unselected", "veg", "slope_kept"))
    assert first > 512 * len(BY_NAME["defaults_s128"].tiles), (first, ta)
    # mode 3: two empty tiles, rejections by class
    assert sum(len(w) == 0 for w in M["mode3_shore"][0]) == 2 and M["mode3_shore"][1]["class"] >= 10
    # skip and the two stats culls
    assert [len(w) > 0 for w in M["skip_and_stats"][0]] == [True, False, False, False]
    ocfg = orclib.make_config(mesh_gen_mode=0)
    orc.init(ocfg)
    sc = tpm.Scene(orc, ocfg, tpm.TreeParams())
    st = M["skip_and_stats"][3]
    assert st[2].mzmax < sc.water_plane_z and sc.get_rel_height(st[3].mzmin) > 0.6 and st[3].mzmax > sc.water_plane_z
    assert [dpm.can_have_decid_trees_in_zrange(sc, s.mzmin, s.mzmax) for s in st] == [True, True, False, False]
    # shared trees: ids within the type's share at 100, clamped to the last at 3
    ids100 = np.array([(r["tree_id"], r["type"]) for w in M["shared_100"][0] for r in w])
    assert ((ids100[:, 0] >= 20 * ids100[:, 1]) & (ids100[:, 0] < 20 * (ids100[:, 1] + 1))).all() and len(set(ids100[:, 0])) > 40
    ids3 = np.array([(r["tree_id"], r["type"]) for w in M["shared_3"][0] for r in w])
    assert (ids3[:, 0] == np.minimum(ids3[:, 1], 2)).all() and (ids3[:, 1] > 2).any()
    assert all(r["tree_id"] == -1 for w in M["defaults_s128"][0] for r in w)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    dpc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer forms on the emulator's "device" memory"""
    dpc.run_case(pkg, emul, orc, case, dev=True)


def test_decid_params(pkg, emul):
    dp = emul.get_decid_params()  # the reference's defaults
    assert (dp.num_trees, dp.num_shared_trees, dp.tree_slope_thresh, list(dp.branch_size)) == (0, 0, 5.0, [1.0] * 5)
    emul.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=100, tree_slope_thresh=2.5, branch_size=(0.5, 1.0, 1.5, 2.0, 2.5)))
    dp = emul.get_decid_params()
    assert (dp.num_trees, dp.num_shared_trees, dp.tree_slope_thresh, list(dp.branch_size)) == (400, 100, 2.5, [0.5, 1.0, 1.5, 2.0, 2.5])
    bad = [(dict(num_trees=-1), "num_trees"), (dict(tree_slope_thresh=0.0), "tree_slope_thresh"), (dict(tree_slope_thresh=-1.0), "tree_slope_thresh"),
           (dict(tree_slope_thresh=float("nan")), "tree_slope_thresh"), (dict(tree_slope_thresh=float("inf")), "tree_slope_thresh"),
           (dict(branch_size=(1.0, 1.0, 0.0, 1.0, 1.0)), "branch_size"), (dict(branch_size=(1.0, 1.0, 1.0, 1.0, float("nan"))), "branch_size"),
           (dict(branch_size=(float("inf"), 1.0, 1.0, 1.0, 1.0)), "branch_size"), (dict(branch_size=(1.0, -2.0, 1.0, 1.0, 1.0)), "branch_size")]
    for kw, word in bad:
        with pytest.raises(pkg.TerraError) as e:
            emul.set_decid_params(pkg.make_decid_params(**kw))
        assert e.value.code == dpc.ERR_ARG and word in str(e.value), kw
    dp = emul.get_decid_params()  # a refused setting changes nothing
    assert (dp.num_trees, dp.num_shared_trees, dp.tree_slope_thresh, list(dp.branch_size)) == (400, 100, 2.5, [0.5, 1.0, 1.5, 2.0, 2.5])
    assert emul.lib.terra_set_decid_params(emul.ctx, None) == dpc.ERR_ARG and emul.lib.terra_get_decid_params(emul.ctx, None) == dpc.ERR_ARG


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    tiles = dpc.TILES
    last = lambda: lib.terra_last_error().decode()  # noqa: E731

    def code(**kw):
        try:
            emul.tiles_place_decid_trees(tiles, 8, **kw)
            return 0
        except pkg.TerraError as e:
            return e.code

    brush = dpc.tpc.brush_at(128, (0, 0), 64.0, 64.0, 30.0, False)
    # before terra_init_scene
    assert code() == dpc.ERR_STATE and code(brush=brush) == dpc.ERR_STATE
    emul.init_scene(pkg.make_config(mesh_gen_mode=0))
    # the defaults have num_trees 0: zero trees, nothing written
    trees, counts = emul.tiles_place_decid_trees(tiles, 8)
    assert not counts.any() and not trees.tobytes().strip(b"\0")
    emul.set_decid_params(pkg.make_decid_params(num_trees=400))
    assert emul.tiles_place_decid_trees(tiles, 8)[1].all() and emul.tiles_place_decid_trees(tiles, 0)[1].all()  # capacity 0: counts only
    emul.set_tree_params(pkg.make_tree_params(tree_mode=2))  # bit 1 clear
    assert not emul.tiles_place_decid_trees(tiles, 8)[1].any() and not emul.tiles_place_decid_trees(tiles, 8, brush=brush)[1].any()
    emul.set_tree_params(pkg.make_tree_params(tree_mode=0))
    assert not emul.tiles_place_decid_trees(tiles, 8)[1].any()
    emul.set_tree_params(pkg.make_tree_params())
    # null pointers, n == 0, alignment, stats without zvals
    txy = np.array(tiles, np.int32)
    cn, tr = np.zeros(4, np.uint32), np.zeros((4, 8), pkg.DECID_PLACE_DTYPE)
    z, st = np.zeros((4, 130, 130), np.float32), (pkg.TileStats * 4)()
    f = lib.terra_tiles_place_decid_trees
    assert f(ctx, None, 4, 0, 0, None, None, None, 8, tr.ctypes.data, cn.ctypes.data) == dpc.ERR_ARG and "null" in last()
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, None, None, 8, None, cn.ctypes.data) == dpc.ERR_ARG and "null" in last()
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, None, None, 8, tr.ctypes.data, None) == dpc.ERR_ARG and "null" in last()
    assert lib.terra_tiles_place_decid_trees_brush(ctx, txy.ctypes.data, 4, 0, 0, None, None, None, None, 1.0, 0, 8, tr.ctypes.data, cn.ctypes.data) == dpc.ERR_ARG and "null" in last()
    assert f(ctx, None, 0, 0, 0, None, None, None, 8, None, None) == 0
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, C.addressof(st), None, 8, tr.ctypes.data, cn.ctypes.data) == dpc.ERR_ARG and "stats without zvals" in last()
    g = lib.terra_tiles_place_decid_trees_dev
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, C.addressof(st), None, 8, tr.ctypes.data, cn.ctypes.data) == dpc.ERR_ARG and "stats without zvals" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, None, None, 8, tr.ctypes.data + 2, cn.ctypes.data) == dpc.ERR_ARG and "aligned" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, C.addressof(st), z.ctypes.data + 1, 8, tr.ctypes.data, cn.ctypes.data) == dpc.ERR_ARG and "aligned" in last()
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, C.addressof(st), z.ctypes.data, 8, tr.ctypes.data, cn.ctypes.data) == 0
    # a heightmap texture
    pix = emul.alloc(64 * 64 * 2).upload(np.zeros(64 * 64 * 2, np.uint8))
    try:
        emul.hmap_set_dev(pix.ptr, 64, 64, 2)
        assert code() == dpc.ERR_STATE and "heightmap" in last()
        assert code(brush=brush) == dpc.ERR_STATE
        emul.hmap_set_dev(None)
        assert code() == 0
    finally:
        emul.hmap_set_dev(None)
        pix.free()
    # 1.0/tree_scale beyond an int
    emul.set_tree_params(pkg.make_tree_params(tree_scale=1e-10))
    assert code() == dpc.ERR_ARG and "skip_val" in last()
    # num_trees/sqrt(tree_density_thresh) beyond an unsigned
    emul.set_tree_params(pkg.make_tree_params(tree_density_thresh=0.0))
    assert code() == dpc.ERR_ARG and "mod_num_trees" in last()
    emul.set_tree_params(pkg.make_tree_params())
    # n == 0 does nothing, whatever the settings
    assert f(ctx, None, 0, 0, 0, None, None, None, 8, None, None) == 0
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert code() == dpc.ERR_ARG
