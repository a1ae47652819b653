"""Scenery placement (terra_tiles_place_scenery, terra_set_scenery_params) through the host emulator -- the driver's one-thread-per-tile form -- against
tests/scenery_place_model.py, byte for byte, order, counts and kind counts included; plus the settings and the refusals.

test_model_on_oracle_primitives checks the model alone and passes without the feature; every other test needs the new symbols."""
import numpy as np
import pytest

import orclib
import scenery_place_cases as spc
import scenery_place_model as spm
import tree_place_model as tpm

CASES = spc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_on_oracle_primitives(orc):
    """the model's generator helpers against the oracle's generator: the array form of the seeding and selection against orc.rand_ints on the wrapped seeds, and
    signed_rand_vector_norm, rand_uniform and rand_float -- the draws every create() is made of -- against orc.rand_floats / rand_uniforms, with
    signed_rand_vector's arguments evaluated right to left (the first draw is z)"""
    cfg = orclib.make_config(mesh_gen_mode=0)
    orc.init(cfg)
    sc = tpm.Scene(orc, cfg, tpm.TreeParams(rand_gen_index=5))
    val, a1, a2 = spm.selection(sc, -2, 1, 6043)
    for (iy, ix) in [(0, 0), (17, 101), (127, 127), (64, 3)]:
        gi, gj = 1 * 128 + iy, -2 * 128 + ix
        s1, s2 = tpm.wrap32(786433 * gi + 196613 * 5), tpm.wrap32(6291469 * gj + 1572869 * 5)
        v1 = int(orc.rand_ints(s1, s2, 1)[0])  # rand2_seed_mix: one value, the swap, one more
        r = tpm.RandGen(s1, s2)
        assert r.rand() == v1
        v2 = int(orc.rand_ints(r.rseed2, r.rseed1, 1)[0])
        assert int(val[iy, ix]) == (tpm.wrap32(v1 + v2) % 2 ** 32) % 6043
        r = tpm.RandGen(s1, s2)
        assert (tpm.wrap32(r.rand_seed_mix()) % 2 ** 32) % 6043 == int(val[iy, ix])
        r.rand_mix()
        assert (int(a1[iy, ix]), int(a2[iy, ix])) == (r.rseed1, r.rseed2)
    for (s1, s2) in [(1, 1), (12345, 678910), (2147483000, 77), (40014, 40692)]:
        # signed_rand_float is 2.0*float(randd()) - 1.0 and rand_uniform(-1, 1) is -1 + 2*float(randd()): the same float for the same draw wherever 2*d is exact,
        # which it always is; so the oracle's rand_uniforms(-1, 1) are the draws of signed_rand_vector, in draw order
        draws = orc.rand_uniforms(s1, s2, -1.0, 1.0, 30)
        r = tpm.RandGen(s1, s2)
        k = 0
        for _ in range(3):
            v = spm.signed_rand_vector_norm(r)
            while True:  # the reference's rejection loop on the oracle's draws
                z, y, x = draws[k], draws[k + 1], draws[k + 2]  # the first draw lands in z, the third in x
                k += 3
                mag_sq = f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))
                if mag_sq > f32(1.0E-12):
                    break
            m = f32(1.0 / float(np.sqrt(mag_sq)))
            assert [float(c) for c in v] == [float(f32(x * m)), float(f32(y * m)), float(f32(z * m))]
            assert abs(float(v[0]) ** 2 + float(v[1]) ** 2 + float(v[2]) ** 2 - 1.0) < 1e-6
        # the generator stands where the oracle's stands after k draws
        assert r.rand() == int(orc.rand_ints(s1, s2, k + 1)[k])
        for (a, b) in [(0.8, 1.3), (0.003, 0.008), (-0.1, 0.25), (0.0, 360.0)]:
            r = tpm.RandGen(s1, s2)
            assert [float(r.rand_uniform(a, b)) for _ in range(5)] == [float(v) for v in orc.rand_uniforms(s1, s2, a, b, 5)]
        r = tpm.RandGen(s1, s2)
        assert [float(r.rand_float()) for _ in range(5)] == [float(v) for v in orc.rand_floats(s1, s2, 5)]


def test_cases_are_not_vacuous(pkg, orc):
    """on the model alone: every kind occurs, every drop reason occurs, some tile has more than 256 selected cells and one more than the 512 the kernel's ring holds"""
    assert pkg.SCENERY_PLACE_DTYPE == spm.PLACE_DTYPE and tuple(pkg.SCENERY_KINDS) == spm.KINDS
    total = spm.new_tally()
    for case in CASES:
        want, tally = spc.model(orc, case)
        assert sum(len(w) for w in want) >= case.min_objs, (case.name, sum(len(w) for w in want))
        assert 3 <= len(case.tiles) <= 9
        for k in total:
            total[k] = max(total[k], tally[k]) if k == "max_selected" else total[k] + tally[k]
    for k in spm.KINDS + spm.DROPS:
        assert total[k] >= 1, (k, total)
    assert total["max_selected"] > 256, total
    M = spc.MODEL
    # the shore: water plants, underwater leafy plants, stumps and mushrooms below their minima, palm and pine log types
    sh = M["shore_mode3"][1]
    assert min(sh["water_plant"], sh["uw_leafy_plant"], sh["stump_too_low"], sh["mushroom_too_low"], sh["palm_log"], sh["pine_log"]) >= 1, sh
    # the defaults at S = 128: every kind except voxel rocks, 77 to 101 selected cells a tile would fit a single flush of the ring
    d = M["defaults_s128"][1]
    assert d["voxel_rock"] == 0 and all(d[k] >= 1 for k in spm.KINDS if k != "voxel_rock"), d
    assert d["max_selected"] <= 256
    # voxel rocks: always at 1; at 2 only without vegetation, and then no plant, log or stump; never at 0
    assert M["voxel_rocks_1"][1]["voxel_rock"] >= 5 and M["voxel_rocks_0"][1]["voxel_rock"] == 0
    v2 = M["voxel_rocks_2_no_vegetation"][1]
    assert v2["voxel_rock"] >= 5 and v2["plant"] == v2["leafy_plant"] == v2["log"] == v2["stump"] == v2["mushroom"] == 0 and v2["no_veg"] >= 20
    # the skipped tile is empty and the others are not; the capacity case does cut a tile short; the ring fills more than once at tree_scale 8
    assert [len(w) > 0 for w in M["skipped_tile"][0]] == [True, False, True, True]
    assert max(len(w) for w in M["capacity_small"][0]) > BY_NAME["capacity_small"].capacity
    assert M["tree_scale_8_s64"][1]["max_selected"] > 256 and M["tree_scale_8_s20"][1]["max_selected"] > 256
    assert M["tree_scale_16_s64"][1]["max_selected"] > 512  # the ring index wraps
    for case in CASES:
        if case.name != "capacity_small":
            assert max(len(w) for w in M[case.name][0]) <= case.capacity, case.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    spc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    spc.run_case(pkg, emul, orc, case, dev=True)


def test_without_kind_counts(pkg, emul, orc):
    spc.run_case(pkg, emul, orc, BY_NAME["defaults_s128"], kind_counts=False)
    spc.run_case(pkg, emul, orc, BY_NAME["skipped_tile"], dev=True, kind_counts=False)


def test_scenery_params(pkg, emul):
    assert emul.get_scenery_params().use_voxel_rocks == 2  # the reference's default
    for v in (0, 1, 3):
        emul.set_scenery_params(pkg.make_scenery_params(v))
        assert emul.get_scenery_params().use_voxel_rocks == v
    with pytest.raises(pkg.TerraError) as e:
        emul.set_scenery_params(pkg.make_scenery_params(-1))
    assert e.value.code == spc.ERR_ARG and "use_voxel_rocks" in str(e.value)
    assert emul.get_scenery_params().use_voxel_rocks == 3  # a refused setting changes nothing
    assert emul.lib.terra_set_scenery_params(emul.ctx, None) == spc.ERR_ARG and emul.lib.terra_get_scenery_params(emul.ctx, None) == spc.ERR_ARG


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    tiles = spc.TILES
    last = lambda: lib.terra_last_error().decode()  # noqa: E731

    def code(**kw):
        try:
            emul.tiles_place_scenery(tiles, 8, **kw)
            return 0
        except pkg.TerraError as e:
            return e.code

    # before terra_init_scene
    assert code() == spc.ERR_STATE
    txy = np.array(tiles, np.int32)
    cn, ob, kc = np.zeros(4, np.uint32), np.zeros((4, 8), pkg.SCENERY_PLACE_DTYPE), np.zeros((4, spc.NK), np.uint32)
    f, g = lib.terra_tiles_place_scenery, lib.terra_tiles_place_scenery_dev
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, cn.ctypes.data, None) == spc.ERR_STATE
    emul.init_scene(pkg.make_config(mesh_gen_mode=0))
    objs, counts, kinds = emul.tiles_place_scenery(tiles, 8)
    assert counts.all() and (kinds.sum(axis=1) == counts).all()
    assert emul.tiles_place_scenery(tiles, 0)[1].tolist() == counts.tolist()  # capacity 0: counts only
    # null pointers, n == 0, alignment
    assert f(ctx, None, 4, 0, 0, None, 8, ob.ctypes.data, cn.ctypes.data, None) == spc.ERR_ARG and "null" in last()
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, 8, None, cn.ctypes.data, None) == spc.ERR_ARG and "null" in last()
    assert f(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, None, None) == spc.ERR_ARG and "null" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, None, None) == spc.ERR_ARG and "null" in last()
    assert f(ctx, None, 0, 0, 0, None, 8, None, None, None) == 0 and g(ctx, None, 0, 0, 0, None, 8, None, None, None) == 0
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data + 2, cn.ctypes.data, None) == spc.ERR_ARG and "aligned" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, cn.ctypes.data + 1, None) == spc.ERR_ARG and "aligned" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, cn.ctypes.data, kc.ctypes.data + 2) == spc.ERR_ARG and "aligned" in last()
    assert g(ctx, txy.ctypes.data, 4, 0, 0, None, 8, ob.ctypes.data, cn.ctypes.data, kc.ctypes.data) == 0
    # a heightmap texture
    pix = emul.alloc(64 * 64 * 2).upload(np.zeros(64 * 64 * 2, np.uint8))
    try:
        emul.hmap_set_dev(pix.ptr, 64, 64, 2)
        assert code() == spc.ERR_STATE and "heightmap" in last()
        emul.hmap_set_dev(None)
        assert code() == 0
    finally:
        emul.hmap_set_dev(None)
        pix.free()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert code() == spc.ERR_ARG
    assert f(ctx, None, 0, 0, 0, None, 8, None, None, None) == spc.ERR_ARG  # n == 0 does nothing only once the scene and the tile size have passed
