"""Five tile_t members pinned to the reference's own compiled code (oracle/_ref/tiled_mesh.o through oracle/ref_shim.cpp section 4), every byte, no tolerance:

    tile_t::add_tree_ao_shadow                    tests/tree_map_model.py        terra_tiles_tree_map[_dev]
    tile_t::upload_shadow_map_texture             tests/tree_map_model.py        terra_tiles_shadow_texture[_dev]
    tile_t::create_texture, existing weights      tests/tree_map_model.py        terra_tiles_tree_weights[_dev]
    tile_t::line_intersect_mesh, inc_trees = 0    tests/line_intersect_model.py  terra_tiles_line_intersect[_dev]
    tile_t::add_or_remove_grass_at                tests/grass_brush_model.py     terra_tiles_edit_grass[_dev]

The `ref` tests compare the models with the live reference on tests/tile_member_cases.py's inputs (they skip where oracle/_ref is absent).  The fixture tests
need no reference tree: tests/golden/tile_member_vectors.npz holds a recording of the reference's outputs, which the models and the host emulator (through the C
ABI, host and device entry points) must reproduce; under `ref` the live reference must still reproduce the recording.

The flower calls add_or_remove_grass_at ends with are recorded by the harness.  update_subrange's range is compared with the range terra_tiles_edit_grass reports
for the same stroke (what terra_tiles_edit_flowers takes); the library derives clear_within's arguments inside terra_tiles_edit_flowers and exposes nothing
comparable, so those are compared with tests/flower_model.py's statement of them (tile_member_cases.expected_calls)."""
import numpy as np
import pytest

import orclib
import tile_member_cases as tmc
import tree_map_model as tmm


LIVE = {}  # the live reference's results on the full case sets, computed once


@pytest.fixture(scope="module")
def fx():
    return tmc.load()


@pytest.fixture()
def ref(ref):
    """the reference checker with the five tile_t members; see tile_member_cases.stale_reference for the one case that skips (it fails where the tree is present)"""
    reason = tmc.stale_reference(ref)
    if reason:
        pytest.skip(reason)
    return ref


# ---- the models against the live reference
def test_tree_map_model_vs_reference(ref):
    cases = tmc.tree_cases(ref)
    by_name = {c["name"]: i for i, c in enumerate(cases)}
    # every byte value under every rval 1 .. 12
    for r in range(1, 13):
        mine = [c for c in cases if c.get("rval") == r]
        assert sorted(v for c in mine for v in c["values"]) == list(range(256)) and all(set(c["values"]) <= set(np.unique(c["prefill"]).tolist()) for c in mine)
        assert all(tmm.splat_params(tmc.tree_scene(ref, tmc.SCENES[0])[0], 0, 0, 0, 0, *sp)[2] == r for sp in mine[0]["splats"][:2])
    assert {tuple(c["tile"]) for c in cases if c["name"].startswith("centres")} == {t for _, t in tmc.TREE_TILES}
    assert min(len(c["splats"]) for c in cases if c["name"].startswith("order")) >= 40
    want = tmc.ref_tree(ref, cases)
    got, skipped = tmc.model_tree(ref, cases)
    assert skipped == 0
    tmc.compare_tree("model", cases, got, want)
    # the inputs do what they are named for
    assert (want[by_name["order"]][0] != want[by_name["order_reversed"]][0]).any()
    for g in (0, 1):
        assert want[by_name[f"flags_far_g{g}"]][1] == (False, False, False) and want[by_name[f"flags_corner_g{g}"]][1] == (False, False, False)
        assert want[by_name[f"flags_touch_g{g}"]][1] == (True, True, bool(g))
        assert (want[by_name[f"flags_corner_g{g}"]][0] == 255).all()
    for c, w in zip(cases, want):
        if c["name"].startswith(("centres", "radii")):
            assert (w[0] != 255).any() and w[1][0], c["name"]
    # the round_fp ties and the int(tradius/DX_VAL) steps are reached: within a +-ulp family the reference's window moves
    sc = tmc.tree_scene(ref, tmc.SCENES[1])[0]
    c = cases[by_name["radii_s1"]]
    rv = [tmm.splat_params(sc, c["tile"][0], c["tile"][1], 0, 0, x, y, r)[2] for x, y, r in c["splats"]]
    assert sum(len(set(rv[k:k + 5])) > 1 for k in range(0, len(rv), 5)) >= 10


def test_tree_map_operand_types_vs_reference(ref, monkeypatch):
    """tests/tree_map_model.py argues that sqrt(float) is the float overload in `float mult(0.2 + 0.8*scale*sqrt(dist_sq))` and that the products are double: a model
    with the double sqrt, or with float products, disagrees with the compiled reference on the maps made for it"""
    cases = [c for c in tmc.tree_cases(ref) if c["name"].startswith("types_")]
    want = tmc.ref_tree(ref, cases)
    tmc.compare_tree("model", cases, tmc.model_tree(ref, cases)[0], want)
    f32 = np.float32
    variants = dict(double_sqrt=lambda scale, d2: (0.2 + (0.8 * float(scale)) * np.sqrt(np.asarray(d2, np.float64))).astype(f32),
                    float_products=lambda scale, d2: (f32(0.2) + (f32(0.8) * f32(scale)) * np.sqrt(np.asarray(d2, f32))).astype(f32))
    for name, fn in variants.items():
        monkeypatch.setattr(tmm, "mult_of", fn)
        got = tmc.model_tree(ref, cases)[0]
        differ = {c["name"] for c, g, w in zip(cases, got, want) if (g[0] != w[0]).any()}
        assert differ >= {f"types_r{r}_v{v}" for r, v in (tmc.TYPE_CASES[:4] if name == "double_sqrt" else tmc.TYPE_CASES[4:])}, (name, differ)


def test_shadow_texture_model_vs_reference(ref):
    pairs, sh, masks = set(), set(), [set(), set()]
    for rep in range(4):
        sun, moon, ao, tm = tmc.shadow_inputs(rep)
        pairs |= set((ao.astype(np.int32).reshape(-1) * 256 + tm[..., 0].reshape(-1)).tolist())
        sh |= set(tm[..., 1].reshape(-1).tolist())
        masks[0] |= set(sun[:129, :129].reshape(-1).tolist()); masks[1] |= set(moon[:129, :129].reshape(-1).tolist())
        en = ((sun[:129, :129] & tmm.SHADOWED_ALL) == 0) * 2 + ((moon[:129, :129] & tmm.SHADOWED_ALL) == 0)
        assert len(np.unique(en)) == 4
    assert len(pairs) == 65536 and len(sh) == 256 and len(masks[0]) == 256 and len(masks[1]) == 256
    lfs = tmc.light_factors()
    assert len(lfs) == 45 and len({tmm.shadow_flags(lf)[:2] for lf in lfs}) == 3  # sun only, moon only, both
    flags = [tmm.shadow_flags(tmc.step(np.float32(v), j))[:2] for v in (0.4, 0.6) for j in tmc.STEPS]
    assert len(set(flags[:5])) == 2 and len(set(flags[5:])) == 2  # the double comparisons flip inside both +-ulp families
    calls = tmc.shadow_calls()
    assert {(c[1], c[4], c[5]) for c in calls} == {(g, a, m) for g in (0, 1) for a in (True, False) for m in (True, False)}
    for call in calls:
        tmc.first_diff(f"model: shadow texture {call}", tmc.model_shadow(call), tmc.ref_shadow(ref, call))


def test_tree_weights_model_vs_reference(ref):
    w, tm = tmc.weights_pairs()
    live = tm[..., 0] != 255
    keys = (tm[..., 0].astype(np.int64) * 256 + w[..., tmc.GRASS]) * 256 + w[..., tmc.DIRT]
    assert len(np.unique(keys.reshape(-1))) >= len(tmc.PAIR_DIRT) * 65536 - 256 * len(tmc.PAIR_DIRT)  # (tree_ao 255 is "no trees": those pairs are left alone)
    for dirt in tmc.PAIR_DIRT:
        sel = w[..., tmc.DIRT] == dirt
        assert len(np.unique(keys[sel & live])) == 255 * 256 and len(np.unique(keys[sel])) == 65536, dirt
    want = tmc.ref_weights(ref, w, tm)
    tmc.first_diff("model: pairs", tmm.tree_weights(w, tm), want)
    assert (want != w).any()
    ws, tms = tmc.weights_stride()
    want = tmc.ref_weights(ref, ws, tms)
    tmc.first_diff("model: stride", tmm.tree_weights(ws, tms), want)
    rock = ws[..., tmc.ROCK] == 255
    assert rock.any() and (want[rock] == ws[rock]).all() and (want[~rock] != ws[~rock]).any()
    tmc.first_diff("model: no tree map", tmm.tree_weights(ws[:2], None), tmc.ref_weights(ref, ws[:2], None))
    assert (tmc.ref_weights(ref, ws[:2], None) == ws[:2]).all()


def test_line_query_model_vs_reference(ref):
    sc = tmc.line_scene(ref)
    tiles, z, mz = tmc.line_tiles(ref)
    rows, kind, tile, groups = tmc.line_rows(sc, tiles, z, mz)
    assert set(kind.tolist()) == set(range(len(tmc.LINE_KINDS))) and set(tile.tolist()) == {0, 1, 2, 3}
    assert tmc.line_rows_undefined(sc, rows) == 0  # no row is skipped
    want = tmc.ref_lines(ref, tiles, z, mz, rows, kind, tile)
    tmc.compare_lines("model", tmc.model_lines(sc, tiles, z, mz, rows, kind, tile), want, kind)
    hit = want["hit"] != 0
    assert 0.25 <= hit.mean() <= 0.75
    assert not hit[kind == 8].any() and not hit[kind == 5].any() and hit[kind == 4].any() and hit[kind == 6].any() and hit[kind == 7].any()
    for k, (n, f) in tmc.line_tallies(want, kind, groups)[1].items():
        assert f >= 0.25 * n, (tmc.LINE_KINDS[k], f, n)


def test_grass_brush_model_vs_reference(ref):
    try:
        sc = tmc.grass_scene(ref)
        d = tmc.grass_tiles(ref)
        strokes = tmc.grass_strokes(sc, d)
        assert {(int(s["shape"]), int(s["add"])) for s in strokes} >= {(sh, a) for sh in range(8) for a in (0, 1)}
        assert {round(float(s["weight"]), 6) for s in strokes} >= {round(0.001 * 2 ** k, 6) for k in range(10)}
        results = []
        for k, s in enumerate(strokes):
            want = tmc.ref_stroke(ref, d, s)
            got = tmc.model_stroke(sc, d, s)
            tmc.compare_stroke(f"model: stroke {k}", got, want)
            assert got[3] == want[3] == bool(s["hag"]), k
            assert tmc.calls_equal(want[4], got[4]), f"stroke {k}: flower calls {want[4].as_tuple()} != {got[4]}"
            if s["radius"] == 0 or s["pos"][2] > d["mz"][int(s["tile"]), 1] + 10:
                assert not want[0], k
            results.append(want)
        tmc.check_grass_tallies(tmc.grass_tallies(sc, d, strokes, results))
        n_upd, n_clr = sum(r[4].n_update for r in results), sum(r[4].n_clear for r in results)
        assert n_upd >= 40 and n_clr >= 40 and any(r[0] and not s["add"] and not r[4].n_clear for s, r in zip(strokes, results))
    finally:
        ref.set_landscape(orclib.make_landscape())


def test_reference_reproduces_fixture(ref, fx):
    got = tmc.record(ref)[0]
    assert set(got) == set(fx) - {"grass_d"}
    for k, v in got.items():
        assert np.asarray(v).dtype == fx[k].dtype and np.asarray(v).tobytes() == fx[k].tobytes(), k


# ---- the recording, where there is no reference tree
def test_fixture_size():
    import os
    assert os.path.getsize(tmc.FIXTURE) < 1000000


def test_models_vs_fixture(orc, fx):
    """the models with the scene constants of the C restatement (pinned to the reference by tests/test_oracle.py) reproduce every recorded byte"""
    try:
        cases, want = tmc.fixture_tree(fx)
        assert [c["name"] for c in cases] == list(tmc.FIXTURE_TREE)
        got, skipped = tmc.model_tree(orc, cases)
        assert skipped == 0
        tmc.compare_tree("model", cases, got, want)
        assert (fx["shadow_lf"].view(np.uint32) == tmc.light_factors().view(np.uint32)).all()
        for k in range(len(fx["shadow_lf"])):
            call, tex = tmc.fixture_shadow(fx, k)
            tmc.first_diff(f"model: shadow texture at light factor {call[0]!r}", tmc.model_shadow(call), tex)
        w, tm, out = tmc.fixture_weights(fx)
        tmc.first_diff("model: tree weights", tmm.tree_weights(w, tm), out)
        sc = tmc.line_scene(orc)
        assert np.array([sc.xss, sc.yss, sc.DX_VAL, sc.DY_VAL, sc.DX_VAL_INV, sc.DY_VAL_INV], np.float32).tobytes() == fx["line_scene"].tobytes()
        assert tmc.line_rows_undefined(sc, fx["line_rows"]) == 0
        tmc.compare_lines("model", tmc.model_lines(sc, fx["line_tiles"], fx["line_z"], fx["line_mz"], fx["line_rows"], fx["line_kind"], fx["line_tile"]), fx["line_hits"], fx["line_kind"])
        gsc = tmc.grass_scene(orc)
        for k in range(len(fx["grass_strokes"])):
            s, want = tmc.fixture_stroke(fx, k)
            got = tmc.model_stroke(gsc, fx["grass_d"], s)
            tmc.compare_stroke(f"model: stroke {k}", got, want)
            assert got[3] == want[3] and tmc.calls_equal(want[4], got[4]), f"stroke {k}: flag / flower calls {want[3:]} != {got[3:]}"
    finally:
        orc.set_landscape(orclib.make_landscape())


@pytest.mark.parametrize("dev", [False, True], ids=["host entry points", "device entry points"])
def test_emulator_vs_fixture(pkg, emul, fx, dev):
    """the emulator through the C ABI against the recording, with no model in between"""
    tmc.check_lib_against(pkg, emul, dev, **tmc.fixture_sets(fx))


@pytest.mark.parametrize("dev", [False, True], ids=["host entry points", "device entry points"])
def test_emulator_vs_live_reference(pkg, emul, ref, dev):
    """the emulator against the live reference on the full case sets (what tests/test_gpu_tile_members_ref.py runs through HIP)"""
    if "sets" not in LIVE:
        LIVE["sets"] = tmc.reference_sets(ref)
    tmc.check_lib_against(pkg, emul, dev, **LIVE["sets"])
