"""The deciduous tree draw lists (terra_tiles_decid_view[_dev]) through the host emulator -- the driver's one-thread-per-tile form -- against
tests/decid_view_model.py: the tile records, all_bcube, the words, scales, opacities and counts of both sweeps, the four lists and not_visible byte for byte; the
refusals with every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without it."""
import ctypes

import numpy as np
import pytest

import decid_view_cases as dc
import decid_view_model as dm
import terrain_view_cases as tvc

CASES = dc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_alone(orc):
    """every case reaches what it is named for, on the model alone; the lists are consistent with the words; the orders are what the header states"""
    for case in CASES:
        tsc, v, a, rec, nv, res, tally = dc.model(orc, case)
        assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})
        for t, w in enumerate(res):
            if not w.flags & dm.TILE_DRAWN:
                assert not w.leaf and not w.branch and not w.not_visible and not (w.leaf_list or w.branch_list or w.leaf_bb or w.branch_bb), case.name
                continue
            for side, lst, bb in ((w.leaf, w.leaf_list, w.leaf_bb), (w.branch, w.branch_list, w.branch_bb)):
                assert sorted(lst) == [j for j in w.valid if j in side and side[j].word & 3 in (dm.FORM_GEOM, dm.FORM_BOTH)], case.name
                assert sorted(e[1] for e in bb) == [j for j in w.valid if j in side and side[j].word & 3 >= dm.FORM_BOTH], case.name
                assert [e[0] for e in bb] == sorted(e[0] for e in bb) and all(e[0] == int(rec.decid[t, e[1]]["tree_id"]) for e in bb), case.name
                assert all((o.num > 0) <= o.listed and (o.word >> dm.STAGE_SHIFT != 0) <= (o.word & 3 == 0) for o in side.values()), case.name
                assert len(lst) <= rec.cap and len(bb) <= rec.cap
            assert w.branch_list == sorted(w.branch_list) and (w.flags & dm.TILE_SORTED or w.leaf_list == sorted(w.leaf_list)), case.name
            for lst in (w.leaf_bb, w.branch_bb):  # within an id: the order of the sweep
                pos = {j: k for k, j in enumerate(w.leaf_list)} if lst is w.leaf_bb and w.flags & dm.TILE_SORTED else None
                for x, y in zip(lst, lst[1:]):
                    if x[0] == y[0] and (pos is None or (x[1] in pos and y[1] in pos)):
                        assert (x[1] < y[1]) if pos is None else (pos[x[1]] < pos[y[1]]), case.name
    # a sorted tile's list is not in record order, and its billboard runs follow it
    res = dc.MODEL["sorted_ties"][5]
    assert res[0].leaf_list != sorted(res[0].leaf_list)
    # the camera on a sphere centre: the product is beyond 64 bits and the count falls to the floor
    res = dc.MODEL["camera_on_centre"][5]
    assert res[0].leaf[0].num == 1000 // 8 and res[0].branch[0].num == 400 // 40 and float(res[0].leaf[0].scale) > 1e19
    # exactly at get_draw_tile_dist() the leaves are drawn, one float beyond they are not
    res = dc.MODEL["draw_tile_dist"][5]
    assert res[-1].leaf[0].word & 3 and res[-1].leaf[1].word >> dm.STAGE_SHIFT == dm.ST_SIZE


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    dc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    dc.run_case(pkg, emul, orc, case, dev=True)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_leaves_then_branches(pkg, emul, orc, dev):
    dc.run_split(pkg, emul, orc, BY_NAME["all_ids"], dev)


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["all_ids"]
    tsc, v, a, rec, nv, res, tally = dc.model(orc, case)
    n, cap = rec.decid.shape
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    lv, la = tvc.lib_view(pkg, v), dc.lib_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    out = pkg.Terra._decid_view_outputs(n, cap, 3)
    nvb = np.full((n, cap), 3, np.uint8)
    names = pkg.Terra.DECID_VIEW_OUTPUTS
    untouched = lambda: all((x.view(np.uint8) == 3).all() for x in out.values()) and (nvb == 3).all()  # noqa: E731
    f, d = lib.terra_tiles_decid_view, lib.terra_tiles_decid_view_dev

    def call(fn, **kw):
        o = [kw.get(k, p(out[k])) for k in names]
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("td", p(rec.data)), kw.get("ntd", len(rec.data)), None,
                  kw.get("de", p(rec.decid)), kw.get("pc", p(rec.counts)), kw.get("cap", cap), kw.get("nv", p(nvb)), *o)
    # before terra_init_scene
    assert call(f) == dc.ERR_STATE and call(d) == dc.ERR_STATE and untouched()
    dc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == dc.ERR_ARG and "null" in last() and call(fn, args=None) == dc.ERR_ARG and "null" in last()
        for k in ("txy", "td", "de", "pc") + names:
            assert call(fn, **{k: None}) == dc.ERR_ARG and "null" in last(), k
        # n == 0 does nothing once the checks have passed; the table is required all the same
        assert call(fn, n=0, txy=None, de=None, pc=None, nv=None, **{k: None for k in names}) == 0
        assert call(fn, n=0, view=None) == dc.ERR_ARG and call(fn, n=0, td=None) == dc.ERR_ARG
        # a view or args with a non-finite member
        for field in ("pos", "cp"):
            bad = tvc.lib_view(pkg, v)
            getattr(bad, field)[1] = float("nan")
            assert call(fn, view=ctypes.byref(bad)) == dc.ERR_ARG and "finite" in last(), field
        for field in ("behind_sphere_mult", "zoom_f", 0, 1, 2, 3):
            for val in (float("nan"), float("inf")):
                bad = dc.lib_args(pkg, a)
                if isinstance(field, int):
                    bad.lod_scales[field] = val
                else:
                    setattr(bad, field, val)
                assert call(fn, args=ctypes.byref(bad)) == dc.ERR_ARG and "finite" in last(), field
                assert call(fn, n=0, args=ctypes.byref(bad)) == dc.ERR_ARG
        for val in (0.0, -1.0):
            bad = dc.lib_args(pkg, a)
            bad.zoom_f = val
            assert call(fn, args=ctypes.byref(bad)) == dc.ERR_ARG and "> 0" in last(), val
        for val in (2, -1):
            bad = dc.lib_args(pkg, a)
            bad.reflection_pass = val
            assert call(fn, args=ctypes.byref(bad)) == dc.ERR_ARG and "reflection_pass" in last(), val
        # a table that is empty or not num_shared_trees long
        for val in (0, len(rec.data) - 1, len(rec.data) + 1):
            assert call(fn, ntd=val) == dc.ERR_ARG and "num_shared_trees" in last(), val
        # n*capacity beyond 32 bits
        assert call(fn, n=1 << 20, cap=1 << 13) == dc.ERR_ARG and "32 bits" in last()
    assert untouched()
    # misaligned device pointers
    for k in names:
        assert call(d, **{k: p(out[k]) + 2}) == dc.ERR_ARG and "aligned" in last(), k
    assert call(d, td=p(rec.data) + 2) == dc.ERR_ARG and "aligned" in last() and call(d, de=p(rec.decid) + 2) == dc.ERR_ARG and call(d, pc=p(rec.counts) + 1) == dc.ERR_ARG
    assert untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == dc.ERR_ARG and call(d) == dc.ERR_ARG and call(d, n=0) == dc.ERR_ARG and call(f, n=0) == dc.ERR_ARG
    assert untouched()


def test_capacity_zero(pkg, emul, orc):
    """no room for a record: every tile is empty, and the [n][capacity] arrays may be NULL"""
    case = BY_NAME["all_ids"]
    tsc, v, a, rec, nv, res, tally = dc.model(orc, case)
    dc.configure(pkg, emul, case)
    n = len(case.tiles)
    got = emul.tiles_decid_view(case.tiles, tvc.lib_view(pkg, v), dc.lib_args(pkg, a), rec.data, np.zeros((n, 0), pkg.DECID_PLACE_DTYPE), rec.counts, fill=dc.FILL)
    assert not got["tile"].view(np.uint8).any() and not got["list_counts"].any() and not got["all_bcube"].any() and got["leaf_list"].size == 0
    lib, names = emul.lib, pkg.Terra.DECID_VIEW_OUTPUTS
    out = pkg.Terra._decid_view_outputs(n, 0, dc.FILL)
    txy = np.array(case.tiles, np.int32)
    lv, la = tvc.lib_view(pkg, v), dc.lib_args(pkg, a)
    o = [out[k].ctypes.data if out[k].size else None for k in names]
    for fn in (lib.terra_tiles_decid_view, lib.terra_tiles_decid_view_dev):
        assert fn(emul.ctx, txy.ctypes.data, n, 0, 0, 0, 0, ctypes.byref(lv), ctypes.byref(la), rec.data.ctypes.data, len(rec.data), None, None, rec.counts.ctypes.data, 0, None, *o) == 0


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_decid_view.py::test_resident_chain on the emulator's "device" memory"""
    dc.run_resident_chain(pkg, emul, orc)
