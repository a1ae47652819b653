"""The terrain draw list (terra_tiles_terrain_view[_dev], terra_view_behind_sphere_mult) through the host emulator -- the driver's one-thread-per-tile form -- against
tests/terrain_view_model.py: status, dist, lod, crack, both lists in order, counts and the written occl_state byte for byte; the refusals with every output
untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without it."""
import ctypes

import numpy as np
import pytest

import terrain_view_cases as tc
import terrain_view_model as tm
import view_model
import test_grass_view_emul as tge

CASES = tc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_alone(orc):
    """every case exercises what it is named for, on the model alone; the lists are consistent with the status bytes; the draw order is sorted by (dist, index)"""
    for case in CASES:
        sc, stats, v, a, arr, res, tally = tc.model(orc, case)
        assert case.check(tally, res), (case.name, tally)
        status, dist, lod, crack, order, occluded, state = res
        low = status & 7
        assert sorted(order) == np.flatnonzero(low == tm.DRAWN).tolist() and occluded == np.flatnonzero(low == tm.OCCLUDED).tolist(), case.name
        keys = [(float(dist[i]), i) for i in order]
        assert keys == sorted(keys), case.name
        assert (crack[low != tm.DRAWN] == tm.NO_CRACK).all() and (lod < tm.NUM_LODS).all(), case.name
    # at least one tile's LOD differs between reflection_pass 0 and 2 (the 1.8 against the 2.0 of :1926)
    for a, b in (("lod_classes_s16", "lod_classes_s16_pass2"), ("lod_classes_s32", "lod_classes_s32_pass2")):
        assert (tc.MODEL[a][5][2] != tc.MODEL[b][5][2]).any(), (a, b)
    # both many_drawn cases exceed what the kernels' fast ordering path holds
    for name in ("many_drawn_equal", "many_drawn_distinct"):
        assert len(tc.MODEL[name][5][4]) > tc.ORDER_LDS_CAPACITY == 1024, name
    # the state written: 1 exactly on the tiles occluded now, 2 on the tested ones that were not, the rest as it came in
    sc, stats, v, a, arr, res, tally = tc.MODEL["state_in"]
    low, sin, sout = res[0] & 7, arr["occl_state"], res[6]
    assert ((sout == 1) == ((low == tm.OCCLUDED) | (sin == 1))).all() and (sout[sin == 2] == 2).all() and (low[sin == 1] == tm.OCCLUDED_BEFORE).all()


def test_behind_sphere_mult(pkg, emul):
    """terra_view_behind_sphere_mult against the model (the C library's tanf through ctypes), bit for bit, for the views of test_grass_view_emul.VIEWS"""
    for kw in tge.VIEWS:
        want = view_model.behind_sphere_mult(kw["angle"], kw["aspect"])
        got = f32(emul.view_behind_sphere_mult(kw["angle"], kw["aspect"]))
        assert got.tobytes() == want.tobytes(), (kw, got, want)
    assert emul.lib.terra_view_behind_sphere_mult(0.5, 1.0, None) == tc.ERR_ARG


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    tc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    tc.run_case(pkg, emul, orc, case, dev=True)


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["ridge_low_camera"]
    sc, stats, v, a, arr, res, tally = tc.model(orc, case)
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tc.lib_view(pkg, v), tc.lib_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    mn, os_ = np.full(n, 0.5, f32), np.zeros(n, np.uint8)
    out = dict(su=np.full(n, 3, np.uint8), di=np.full(n, 3.0, f32), lo=np.full(n, 3, np.uint8), cr=np.full((n, 4), 3, np.uint8), dr=np.full(n, 3, np.uint32),
               oc=np.full(n, 3, np.uint32), cn=np.full(2, 3, np.uint32))
    untouched = lambda: all((x == 3).all() for x in out.values()) and (os_ == 0).all()  # noqa: E731
    f, d = lib.terra_tiles_terrain_view, lib.terra_tiles_terrain_view_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), kw.get("mn", p(mn)), None, None, None,
                  kw.get("os", p(os_)), o["su"], o["di"], o["lo"], o["cr"], o["dr"], o["oc"], o["cn"], None)
    # before terra_init_scene
    assert call(f) == tc.ERR_STATE and call(d) == tc.ERR_STATE and untouched()
    tc.configure(pkg, emul, case)
    for fn in (f, d):
        # null pointers
        assert call(fn, view=None) == tc.ERR_ARG and "null" in last() and call(fn, args=None) == tc.ERR_ARG and "null" in last()
        for k in ("txy", "st", "su", "di", "lo", "cr", "dr", "oc", "cn"):
            assert call(fn, **{k: None}) == tc.ERR_ARG and "null" in last(), k
        # n == 0 does nothing once the checks have passed
        assert call(fn, n=0, txy=None, st=None, su=None, di=None, lo=None, cr=None, dr=None, oc=None, cn=None, mn=None, os=None) == 0
        assert call(fn, n=0, view=None) == tc.ERR_ARG
        # a view or args with a non-finite member
        for field in ("pos", "upv"):
            bad = tc.lib_view(pkg, v)
            getattr(bad, field)[2] = float("nan")
            assert call(fn, view=ctypes.byref(bad)) == tc.ERR_ARG and "finite" in last(), field
        bad = tc.lib_view(pkg, v)
        bad.near_ = float("-inf")
        assert call(fn, view=ctypes.byref(bad)) == tc.ERR_ARG and "finite" in last()
        for field in ("behind_sphere_mult", "occluder_zmin"):
            for val in (float("nan"), float("inf")):
                bad = tc.lib_args(pkg, a)
                setattr(bad, field, val)
                assert call(fn, args=ctypes.byref(bad)) == tc.ERR_ARG and "finite" in last(), field
                assert call(fn, n=0, args=ctypes.byref(bad)) == tc.ERR_ARG
        # reflection_pass 1 (needs can_have_reflection), above 3, negative
        for rp in (1, 4, -1, 100):
            bad = tc.lib_args(pkg, a)
            bad.reflection_pass = rp
            assert call(fn, args=ctypes.byref(bad)) == tc.ERR_ARG and "reflection_pass" in last(), rp
        # a tile that appears twice
        twice = txy.copy()
        twice[5] = twice[17]
        assert call(fn, txy=p(twice)) == tc.ERR_ARG and "twice" in last()
    assert untouched()
    # misaligned device pointers
    for k in ("di", "dr", "oc", "cn"):
        assert call(d, **{k: p(out[k]) + 2}) == tc.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == tc.ERR_ARG and "aligned" in last() and call(d, mn=p(mn) + 1) == tc.ERR_ARG and "aligned" in last()
    assert untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == tc.ERR_ARG and call(d) == tc.ERR_ARG and call(d, n=0) == tc.ERR_ARG and call(f, n=0) == tc.ERR_ARG
    assert untouched()


def test_odd_tile_size(pkg, emul, orc):
    """S = 17 (refused by the grass view) is accepted here: the tile size enters only through `size`, the boxes and radius"""
    case = tc.Case("ridge_s17", S=17, view=BY_NAME["ridge_low_camera"].view, check=lambda t, r: t["occluded"] >= 3)
    tc.run_case(pkg, emul, orc, case)
    tc.run_case(pkg, emul, orc, case, dev=True)


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_terrain_view.py::test_resident_chain on the emulator's "device" memory"""
    tc.run_resident_chain(pkg, emul, orc)


def test_log2_check_program(tmp_path):
    """tools/terrain_view_log2_check.cpp builds as a stand-alone host program and walks a sub-range: 2^20 floats of one binade.  (Its counts over every float in
    (0, 0.25) are in DESIGN.md; here only that it runs, sees every float of the range once, and that its second count is part of its first.)"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "terrain_view_log2_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-o", exe, os.path.join(root, "tools", "terrain_view_log2_check.cpp")], check=True)
    out = json.loads(subprocess.run([exe, "2", "0x3E000000", "0x3E0FFFFF"], check=True, capture_output=True, text=True).stdout)
    assert out["floats"] == 1 << 20 and out["could_change_float_quotient"] <= out["doubles_differ"] <= out["floats"], out
    assert subprocess.run([exe, "2", "0", "5"], capture_output=True).returncode == 2  # 0.0 is outside (0, 0.25)
