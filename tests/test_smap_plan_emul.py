"""The shadow-map plan (terra_tiles_smap_plan[_dev]), the caster lists (terra_tiles_smap_casters[_dev]) and terra_make_light_view through the host emulator -- the
driver's simple form: the reference's loops, sequential over the batch -- against tests/smap_plan_model.py: every output byte for byte, lists in order up to their
counts, the fill pattern intact wherever a call does not write; the refusals with every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import smap_plan_cases as sc_
import smap_plan_model as sm
import terrain_view_cases as tc

PCASES, CCASES = sc_.plan_cases(), sc_.caster_cases()
P_BY_NAME, C_BY_NAME = {c.name: c for c in PCASES}, {c.name: c for c in CCASES}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_model_alone(orc):
    """every case exercises what it is named for, on the model alone; the lists are consistent with the plan words and the bytes"""
    for case in PCASES:
        sc, stats, v, a, arr, state, res, tally = sc_.model(orc, case)
        assert case.check(tally, res, case), (case.name, {k: x for k, x in tally.items() if x})
        w = res["plan"]
        assert res["receivers"] == np.flatnonzero(w & sm.RECEIVER).tolist(), case.name
        assert sorted(res["box"]) == np.flatnonzero(w & sm.IN_DRAW_DIST).tolist(), case.name
        held = res["smap_state"] != sm.NONE
        assert not (w[~held] & (sm.RECEIVER | sm.USABLE)).any() and (res["smap_state"][held] < sm.NUM_SMAP_LODS).all(), case.name
        assert not (w[(w & sm.UPDATE) == 0] & (sm.ALLOCATED | sm.CLEARED_LOD_RAISE | sm.RECEIVER)).any(), case.name  # cleanup_only never allocates
        if a.want_recomp:
            assert sorted(res["recomp_order"]) == np.flatnonzero(res["present"]).tolist(), case.name
    # the four bands beyond SMAP_NEW_THRESH and every LOD on the 13 x 13 grid
    t = sc_.MODEL["p:grid13_bands"][7]
    assert min(t["band_new"], t["band_del"], t["band_fade"], t["band_beyond"], t["beyond_draw"]) >= 1, t
    # ties in distance come out by (y, x) descending: the queue is consumed from the back
    case = P_BY_NAME["recomp_order_ties"]
    order = sc_.MODEL["p:recomp_order_ties"][6]["recomp_order"]
    assert case.tiles[order[0]] == (0, 0) and [case.tiles[i] for i in order[1:5]] == [(0, 1), (1, 0), (-1, 0), (0, -1)]
    for case in CCASES:
        sc, stats, arr, a, recv, views, bsm, lpos, res, tally = sc_.caster_model(orc, case)
        assert case.check(tally, res, case), (case.name, {k: x for k, x in tally.items() if x})
        for r in range(len(recv)):
            assert res["to_draw"][r] == np.flatnonzero(res["not_drawn"][r] == 0).tolist() and set(res["terrain"][r]) <= set(res["to_draw"][r]), case.name


@pytest.mark.parametrize("case", PCASES, ids=[c.name for c in PCASES])
def test_plan_cases(pkg, emul, orc, case):
    sc_.run_plan_case(pkg, emul, orc, case)
    sc_.run_plan_case(pkg, emul, orc, case, dev=True)


@pytest.mark.parametrize("case", CCASES, ids=[c.name for c in CCASES])
def test_caster_cases(pkg, emul, orc, case):
    sc_.run_cast_case(pkg, emul, orc, case)
    sc_.run_cast_case(pkg, emul, orc, case, dev=True)


def test_make_light_view(pkg, emul):
    sc_.check_light_views(pkg, emul)


def test_plan_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = P_BY_NAME["terrain_flags_ored"]
    sc, stats, v, a, arr, state, res, tally = sc_.model(orc, case)
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tc.lib_view(pkg, v), sc_.lib_plan_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    out = dict(ss=np.full(n, 3, np.uint8), pl=np.full(n, 3, np.uint32), ds=np.full(n, 3.0, f32), sb=np.full((n, 6), 3.0, f32), rc=np.full(n, 3, np.uint32), cn=np.full(2, 3, np.uint32),
               tf=np.full(n, 3, np.uint8), ro=np.full(n, 3, np.uint32))
    untouched = lambda: all((x == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_smap_plan, lib.terra_tiles_smap_plan_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), None, None, None, o["ss"], o["pl"], o["ds"], o["sb"], o["rc"],
                  o["cn"], o["tf"], o["ro"])
    assert call(f) == sc_.ERR_STATE and call(d) == sc_.ERR_STATE and untouched()
    tc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == sc_.ERR_ARG and "null" in last() and call(fn, args=None) == sc_.ERR_ARG and "null" in last()
        for k in ("txy", "st", "ss", "pl", "ds", "sb", "rc", "cn"):
            assert call(fn, **{k: None}) == sc_.ERR_ARG and "null" in last(), k
        assert call(fn, n=0, txy=None, st=None, ss=None, pl=None, ds=None, sb=None, rc=None, cn=None, tf=None, ro=None) == 0 and call(fn, n=0, view=None) == sc_.ERR_ARG
        for field in ("behind_sphere_mult", "smap_thresh_scale", "models_z2"):
            for val in (float("nan"), float("inf")):
                bad = sc_.lib_plan_args(pkg, a)
                setattr(bad, field, val)
                assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last(), field
        for field, k in (("b_ext", 2), ("road_len", 1), ("sun_pos", 0)):
            bad = sc_.lib_plan_args(pkg, a)
            getattr(bad, field)[k] = float("-inf")
            assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last(), field
        for val in (0.0, -1.0):
            bad = sc_.lib_plan_args(pkg, a)
            bad.smap_thresh_scale = val
            assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "smap_thresh_scale" in last()
            assert call(fn, n=0, args=ctypes.byref(bad)) == sc_.ERR_ARG
        bad = tc.lib_view(pkg, v)
        bad.pos[2] = float("nan")
        assert call(fn, view=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last()
    assert untouched()
    for k in ("pl", "ds", "sb", "rc", "cn", "ro"):
        assert call(d, **{k: p(out[k]) + 2}) == sc_.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == sc_.ERR_ARG and "aligned" in last()
    opt = np.zeros(n + 1, f32)  # trmax, tile_zmax
    for slot in (8, 9):
        a_ = [ctx, p(txy), n, 0, 0, vp, ap, sp, None, None, None] + [p(out[k]) for k in ("ss", "pl", "ds", "sb", "rc", "cn", "tf", "ro")]
        a_[slot] = p(opt) + 2
        assert d(*a_) == sc_.ERR_ARG and "aligned" in last(), slot
    assert untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == sc_.ERR_ARG and call(d) == sc_.ERR_ARG and untouched()


def test_casters_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = C_BY_NAME["r5_grid3"]
    sc, stats, arr, a, recv, views, bsm, lpos, res, tally = sc_.caster_model(orc, case)
    n, R = len(case.tiles), len(recv)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    la = sc_.lib_cast_args(pkg, a)
    va = (pkg.View * R)(*[tc.lib_view(pkg, x) for x in views])
    dc = np.ones(n, np.uint32)
    out = dict(td=np.full((R, n), 3, np.uint32), te=np.full((R, n), 3, np.uint32), cn=np.full((R, 2), 3, np.uint32), nd=np.full((R, n), 3, np.uint8), su=np.full(R, 3, np.uint8))
    untouched = lambda: all((x == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_smap_casters, lib.terra_tiles_smap_casters_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("R", R), kw.get("recv", p(recv)), kw.get("views", ctypes.addressof(va)), kw.get("bsm", p(bsm)),
                  kw.get("lpos", p(lpos)), kw.get("args", ctypes.byref(la)), kw.get("st", sp), None, None, None, kw.get("dc", p(dc)), o["td"], o["te"], o["cn"], o["nd"], o["su"])
    assert call(f) == sc_.ERR_STATE and call(d) == sc_.ERR_STATE and untouched()
    tc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, args=None) == sc_.ERR_ARG and "null" in last()
        for k in ("txy", "st", "recv", "views", "bsm", "lpos", "td", "te", "cn", "nd", "su"):
            assert call(fn, **{k: None}) == sc_.ERR_ARG and "null" in last(), k
        assert call(fn, dc=None) == 0  # decid_counts is optional without decid_trees_only
        for x in out.values():
            x[...] = 3
        only = sc_.lib_cast_args(pkg, a)
        only.decid_trees_only = 1
        assert call(fn, dc=None, args=ctypes.byref(only)) == sc_.ERR_ARG and "null" in last()
        none = dict(txy=None, st=None, recv=None, views=None, bsm=None, lpos=None, td=None, te=None, cn=None, nd=None, su=None, dc=None)
        assert call(fn, n=0, **none) == 0 and call(fn, R=0, **none) == 0 and call(fn, n=0, args=None) == sc_.ERR_ARG
        assert call(fn, n=1 << 20, R=1 << 13) == sc_.ERR_ARG and "32 bits" in last()
        bad = sc_.lib_cast_args(pkg, a)
        bad.b_ext[1] = float("nan")
        assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last()
        vb = (pkg.View * R)(*[tc.lib_view(pkg, x) for x in views])
        vb[R - 1].far_ = float("inf")
        assert call(fn, views=ctypes.addressof(vb)) == sc_.ERR_ARG and "finite" in last()
        for name, arr_ in (("bsm", bsm), ("lpos", lpos)):
            nb = arr_.copy()
            nb.reshape(-1)[-1] = float("nan")
            assert call(fn, **{name: p(nb)}) == sc_.ERR_ARG and "finite" in last(), name
    assert untouched()
    for k in ("td", "te", "cn"):
        assert call(d, **{k: p(out[k]) + 2}) == sc_.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == sc_.ERR_ARG and "aligned" in last() and call(d, recv=p(recv) + 1) == sc_.ERR_ARG and "aligned" in last()
    assert call(d, dc=p(dc) + 2) == sc_.ERR_ARG and "aligned" in last()
    opt = np.zeros(n + 1, f32)  # trmax, tile_zmax
    for slot in (12, 13):
        a_ = [ctx, p(txy), n, 0, 0, R, p(recv), ctypes.addressof(va), p(bsm), p(lpos), ctypes.byref(la), sp, None, None, None, p(dc)] + [p(out[k]) for k in ("td", "te", "cn", "nd", "su")]
        a_[slot] = p(opt) + 2
        assert d(*a_) == sc_.ERR_ARG and "aligned" in last(), slot
    assert untouched()
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == sc_.ERR_ARG and call(d) == sc_.ERR_ARG and untouched()


def test_workgroup_scheme_host_program(tmp_path):
    """tests/smap_casters_check.cpp: k_smap_casters' scheme -- a lane per tile, a ballot per list and wave, one prefix over the waves' packed counts -- written for the
    host over the bodies of terra_smapview.hpp, compiled under -fsanitize=address,undefined, against the literal loop on random dense and sparse batches, n not a multiple
    of 64 and out-of-range receivers"""
    exe = str(tmp_path / "smap_casters_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "smap_casters_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)"), r.stdout + r.stderr


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_smap_plan.py::test_resident_chain on the emulator's "device" memory"""
    sc_.run_resident_chain(pkg, emul, orc)
