"""The reflection pass's terrain draw list (terra_tiles_reflection_view[_dev]) and the water quads and water caps (terra_tiles_water_view[_dev]) through the host
emulator -- the driver's simple form: the reference's loop, sequential over the batch -- against tests/water_view_model.py: every output byte for byte, lists in
order up to their counts; the refusals with every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without them."""
import ctypes

import numpy as np
import pytest

import terrain_view_cases as tc
import terrain_view_model as tm
import water_view_cases as wc
import water_view_model as wm

RCASES, WCASES = wc.reflection_cases(), wc.water_cases()
R_BY_NAME, W_BY_NAME = {c.name: c for c in RCASES}, {c.name: c for c in WCASES}
f32 = np.float32


def test_model_alone(orc):
    """every case exercises what it is named for, on the model alone; the lists are consistent with the status bytes; vis_ref_call never fires"""
    for case in RCASES:
        sc, stats, v, a, arr, res, tally = wc.model(orc, case)
        assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})
        assert tally["revisit"] == 0, case.name
        status, dist, lod, crack, order, occluded, state, reflect = res
        low = status & 7
        assert sorted(order) == np.flatnonzero(low == tm.DRAWN).tolist() and occluded == np.flatnonzero(low == tm.OCCLUDED).tolist(), case.name
        assert (crack[low != tm.DRAWN] == tm.NO_CRACK).all() and (lod < tm.NUM_LODS).all(), case.name
        # a dropped tile: reflect 1 or 2, its state as it came in; a tile that passed :2869: reflect 3 or 4; everything else was not asked
        sin = arr["occl_state"] if arr["occl_state"] is not None else np.zeros(len(low), np.uint8)
        assert (np.isin(reflect[low == wm.NO_REFLECTION], (wm.NO_WATER, wm.WALK_NOTHING))).all() and (state[low == wm.NO_REFLECTION] == sin[low == wm.NO_REFLECTION]).all(), case.name
        assert (np.isin(reflect[(low == tm.DRAWN) | (low == tm.OCCLUDED)], (wm.HAS_WATER, wm.WALK_FOUND))).all() and (reflect[low < tm.OCCLUDED] == 0).all(), case.name
    # the two answers of the order-dependence pair differ with the batch order alone, and the shuffled batches follow batch order, not (y, x) order
    ab, ba = wc.MODEL["r:order_a_before_b"], wc.MODEL["r:order_b_before_a"]
    assert ab[5][7][R_BY_NAME["order_a_before_b"].tiles.index(wc.B)] == wm.WALK_NOTHING and ba[5][7][R_BY_NAME["order_b_before_a"].tiles.index(wc.B)] == wm.WALK_FOUND
    sh = R_BY_NAME["order_shuffled"].tiles
    assert sh.index(wc.B) < sh.index(wc.A) and sorted(sh, key=lambda k: (k[1], k[0])).index(wc.A) < sorted(sh, key=lambda k: (k[1], k[0])).index(wc.B)
    # reflect value 1 from all_water and from water disabled
    assert wc.MODEL["r:reflect_values"][6]["refl_all_water"] >= 3 and wc.MODEL["r:water_disabled"][6]["refl_disabled"] >= 3
    for case in WCASES:
        sc, stats, v, a, arr, status, res, tally = wc.water_model(orc, case)
        assert case.check(tally, res), (case.name, {k: x for k, x in tally.items() if x})


@pytest.mark.parametrize("case", RCASES, ids=[c.name for c in RCASES])
def test_reflection_cases(pkg, emul, orc, case):
    wc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", RCASES, ids=[c.name for c in RCASES])
def test_reflection_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    wc.run_case(pkg, emul, orc, case, dev=True)


@pytest.mark.parametrize("case", WCASES, ids=[c.name for c in WCASES])
def test_water_cases(pkg, emul, orc, case):
    wc.run_water_case(pkg, emul, orc, case)
    wc.run_water_case(pkg, emul, orc, case, dev=True)


def test_reflection_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = R_BY_NAME["order_a_before_b"]
    sc, stats, v, a, arr, res, tally = wc.model(orc, case)
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tc.lib_view(pkg, v), wc.lib_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    mn, os_ = np.full(n, 0.5, f32), np.zeros(n, np.uint8)
    out = dict(su=np.full(n, 3, np.uint8), di=np.full(n, 3.0, f32), lo=np.full(n, 3, np.uint8), cr=np.full((n, 4), 3, np.uint8), dr=np.full(n, 3, np.uint32),
               oc=np.full(n, 3, np.uint32), cn=np.full(2, 3, np.uint32), nd=np.full(n, 3, np.uint8), rf=np.full(n, 3, np.uint8))
    untouched = lambda: all((x == 3).all() for x in out.values()) and (os_ == 0).all()  # noqa: E731
    f, d = lib.terra_tiles_reflection_view, lib.terra_tiles_reflection_view_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), kw.get("mn", p(mn)), None, None, None,
                  kw.get("os", p(os_)), o["su"], o["di"], o["lo"], o["cr"], o["dr"], o["oc"], o["cn"], o["nd"], o["rf"])
    # before terra_init_scene
    assert call(f) == wc.ERR_STATE and call(d) == wc.ERR_STATE and untouched()
    tc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == wc.ERR_ARG and "null" in last() and call(fn, args=None) == wc.ERR_ARG and "null" in last()
        for k in ("txy", "st", "su", "di", "lo", "cr", "dr", "oc", "cn"):
            assert call(fn, **{k: None}) == wc.ERR_ARG and "null" in last(), k
        # n == 0 does nothing once the checks have passed
        assert call(fn, n=0, txy=None, st=None, su=None, di=None, lo=None, cr=None, dr=None, oc=None, cn=None, mn=None, os=None, nd=None, rf=None) == 0
        assert call(fn, n=0, view=None) == wc.ERR_ARG
        # a reflection_pass other than 1
        for rp in (0, 2, 3, -1, 100):
            bad = wc.lib_args(pkg, a)
            bad.tv.reflection_pass = rp
            assert call(fn, args=ctypes.byref(bad)) == wc.ERR_ARG and "reflection_pass" in last(), rp
            assert call(fn, n=0, args=ctypes.byref(bad)) == wc.ERR_ARG
        # a non-finite zmax, zmin, behind_sphere_mult; a non-finite member of the view
        for val in (float("nan"), float("inf"), float("-inf")):
            bad = wc.lib_args(pkg, a)
            bad.zmax = val
            assert call(fn, args=ctypes.byref(bad)) == wc.ERR_ARG and "finite" in last()
            bad = wc.lib_args(pkg, a)
            bad.tv.occluder_zmin = val
            assert call(fn, args=ctypes.byref(bad)) == wc.ERR_ARG and "finite" in last()
        bad = tc.lib_view(pkg, v)
        bad.pos[2] = float("nan")
        assert call(fn, view=ctypes.byref(bad)) == wc.ERR_ARG and "finite" in last()
        # a tile that appears twice
        twice = txy.copy()
        twice[5] = twice[17]
        assert call(fn, txy=p(twice)) == wc.ERR_ARG and "twice" in last()
        # tile positions that span more than 2^18 positions
        wide = txy.copy()
        wide[0] = (1 << 20, 0)
        assert call(fn, txy=p(wide)) == wc.ERR_ARG and "bounding box" in last()
    assert untouched()
    # misaligned device pointers
    for k in ("di", "dr", "oc", "cn"):
        assert call(d, **{k: p(out[k]) + 2}) == wc.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == wc.ERR_ARG and "aligned" in last() and call(d, mn=p(mn) + 1) == wc.ERR_ARG and "aligned" in last()
    assert untouched()


def test_water_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = W_BY_NAME["caps_occluded_dry"]
    sc, stats, v, a, arr, status, res, tally = wc.water_model(orc, case)
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tc.lib_view(pkg, v), wc.lib_water_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    su = np.ascontiguousarray(status, np.uint8)
    out = dict(wl=np.full(n, 3, np.uint32), cm=np.full(n, 3, np.uint8), cn=np.full(2, 3, np.uint32))
    untouched = lambda: all((x == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_water_view, lib.terra_tiles_water_view_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), None, None, None, kw.get("su", p(su)), o["wl"], o["cm"], o["cn"])
    assert call(f) == wc.ERR_STATE and call(d) == wc.ERR_STATE and untouched()
    tc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == wc.ERR_ARG and "null" in last() and call(fn, args=None) == wc.ERR_ARG and "null" in last()
        for k in ("txy", "st", "wl", "cn"):
            assert call(fn, **{k: None}) == wc.ERR_ARG and "null" in last(), k
        # status without cap_mask, cap_mask without status
        assert call(fn, cm=None) == wc.ERR_ARG and "both" in last() and call(fn, su=None) == wc.ERR_ARG and "both" in last()
        assert call(fn, n=0, txy=None, st=None, wl=None, cn=None, su=None, cm=None) == 0 and call(fn, n=0, view=None) == wc.ERR_ARG
        bad = wc.lib_water_args(pkg, a)
        bad.behind_sphere_mult = float("nan")
        assert call(fn, args=ctypes.byref(bad)) == wc.ERR_ARG and "finite" in last()
        bad = tc.lib_view(pkg, v)
        bad.far_ = float("inf")
        assert call(fn, view=ctypes.byref(bad)) == wc.ERR_ARG and "finite" in last()
        twice = txy.copy()
        twice[5] = twice[17]
        assert call(fn, txy=p(twice)) == wc.ERR_ARG and "twice" in last()
    assert untouched()
    for k in ("wl", "cn"):
        assert call(d, **{k: p(out[k]) + 2}) == wc.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == wc.ERR_ARG and "aligned" in last()
    assert untouched()


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_water_view.py::test_resident_chain on the emulator's "device" memory"""
    wc.run_resident_chain(pkg, emul, orc)
