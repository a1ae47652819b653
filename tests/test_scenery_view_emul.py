"""The scenery draw lists (terra_tiles_scenery_view[_dev]) through the host emulator -- the driver's one-thread-per-tile form -- against
tests/scenery_view_model.py: the tile records, the draw words, size_scale, dist, the lists and the group counts byte for byte; the refusals with every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without it."""
import ctypes

import numpy as np
import pytest

import scenery_view_cases as sc_
import scenery_view_model as sm
import terrain_view_cases as tvc

CASES = sc_.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_alone(orc):
    """every case reaches what it is named for, on the model alone; the lists are consistent with the draw words; the orders are what the header states"""
    for case in CASES:
        sc, stats, v, g, rec, lcap, res, tally = sc_.model(orc, case)
        assert case.check(tally, res), (case.name, dict(tally))
        for t, w in enumerate(res):
            if not w.written:
                assert w.flags == 0 and w.num_records == 0 and not w.list and not any(w.group_counts), case.name
                continue
            assert len(w.word) == len(w.size_scale) == len(w.dist) == w.num_records == min(int(rec.counts[t]), rec.cap) and len(w.list) == sum(w.group_counts), case.name
            assert len(w.list) <= 3 * w.num_records, case.name
            at = 0
            for gidx, m in enumerate(w.group_counts):
                part, at = w.list[at:at + m], at + m
                kinds = [int(rec.objs[t, i]["kind"]) for i in part]
                if gidx < sm.G_PLD_POINTS:
                    assert part == sorted(part) and len(set(kinds)) <= 1, (case.name, gidx)  # record order, one kind
                else:  # the kinds in the reference's loop order, record order inside a kind
                    order = (sm.SURFACE_ROCK, sm.ROCK) if gidx == sm.G_PLD_POINTS else (sm.LOG, sm.STUMP, sm.PLANT)
                    assert [(order.index(k), i) for k, i in zip(kinds, part)] == sorted((order.index(k), i) for k, i in zip(kinds, part)), (case.name, gidx)
                form = {sm.G_PLD_POINTS: sm.POINT, sm.G_PLD_LINES: sm.LINE}.get(gidx, sm.POLY)
                if gidx not in (sm.G_BERRIES, sm.G_PLANT_LEAVES, sm.G_LEAFY_LEAVES):
                    assert all(w.word[i] & 7 == form for i in part), (case.name, gidx)
            for i, word in enumerate(w.word):
                assert (w.size_scale[i] != 0.0) <= (word & 7 == sm.POLY and int(rec.objs[t, i]["kind"]) in (sm.SURFACE_ROCK, sm.ROCK, sm.VOXEL_ROCK)), (case.name, i)
    # the big tile spans more than two chunks of the kernel's workgroup, and the short list cuts every tile's entries
    sc, stats, v, g, rec, lcap, res, tally = sc_.MODEL["big_tile"]
    assert res[0].num_records > 2 * sc_.THREADS and rec.counts[2] > rec.cap and res[2].num_records == rec.cap
    assert all(len(w.list) > sc_.MODEL["big_tile_short_list"][5] for w in sc_.MODEL["big_tile_short_list"][6])
    # exactly at a threshold the polygon form is kept
    sc, stats, v, g, rec, lcap, res, tally = sc_.MODEL["thresholds"]
    for t, w in enumerate(res):
        for i, word in enumerate(w.word):
            r = rec.objs[t, i]
            if int(r["kind"]) == sm.SURFACE_ROCK and float(w.dist[i]) == 12.5:
                assert word & 7 == sm.POLY


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    sc_.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    sc_.run_case(pkg, emul, orc, case, dev=True)


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["mixed"]
    sc, stats, v, g, rec, lcap, res, tally = sc_.model(orc, case)
    n, cap = rec.objs.shape
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tvc.lib_view(pkg, v), sc_.lib_args(pkg, g.a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    out = pkg.Terra._scenery_view_outputs(n, cap, lcap, 3)
    names = pkg.Terra.SCENERY_VIEW_OUTPUTS
    untouched = lambda: all((x.view(np.uint8) == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_scenery_view, lib.terra_tiles_scenery_view_dev

    def call(fn, **kw):
        o = [kw.get(k, p(out[k])) for k in names]
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), None, kw.get("objs", p(rec.objs)),
                  kw.get("pc", p(rec.counts)), kw.get("cap", cap), kw.get("ov", p(rec.override)), *o[:5], kw.get("lcap", lcap), o[5])
    # before terra_init_scene
    assert call(f) == sc_.ERR_STATE and call(d) == sc_.ERR_STATE and untouched()
    sc_.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == sc_.ERR_ARG and "null" in last() and call(fn, args=None) == sc_.ERR_ARG and "null" in last()
        for k in ("txy", "st", "objs", "pc") + names:
            assert call(fn, **{k: None}) == sc_.ERR_ARG and "null" in last(), k
        # n == 0 does nothing once the checks have passed
        assert call(fn, n=0, txy=None, st=None, objs=None, pc=None, ov=None, **{k: None for k in names}) == 0
        assert call(fn, n=0, view=None) == sc_.ERR_ARG
        # a view or args with a non-finite member
        for field in ("pos", "cp"):
            bad = tvc.lib_view(pkg, v)
            getattr(bad, field)[1] = float("nan")
            assert call(fn, view=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last(), field
        for field in ("behind_sphere_mult", "zoom_f", "smap_pixel_width"):
            for val in (float("nan"), float("inf")):
                bad = sc_.lib_args(pkg, g.a)
                setattr(bad, field, val)
                assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "finite" in last(), field
                assert call(fn, n=0, args=ctypes.byref(bad)) == sc_.ERR_ARG
        # window_width or zoom_f not > 0; smap_pixel_width not > 0 under shadow_pass (and unread without it)
        for field, val in (("window_width", 0), ("window_width", -5), ("zoom_f", 0.0), ("zoom_f", -1.0)):
            bad = sc_.lib_args(pkg, g.a)
            setattr(bad, field, val)
            assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "> 0" in last(), (field, val)
        for val in (0.0, -1.0):
            bad = sc_.lib_args(pkg, g.a)
            bad.shadow_pass, bad.smap_pixel_width = 1, val
            assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "> 0" in last(), val
        # reflection_pass other than 0 or 1
        for val in (2, -1):
            bad = sc_.lib_args(pkg, g.a)
            bad.reflection_pass = val
            assert call(fn, args=ctypes.byref(bad)) == sc_.ERR_ARG and "reflection_pass" in last(), val
        # n*capacity or n*list_capacity beyond 32 bits
        assert call(fn, n=1 << 20, cap=1 << 13) == sc_.ERR_ARG and "32 bits" in last()
        assert call(fn, n=1 << 20, lcap=1 << 13) == sc_.ERR_ARG and "32 bits" in last()
    assert untouched()
    # misaligned device pointers
    for k in names:
        assert call(d, **{k: p(out[k]) + 2}) == sc_.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == sc_.ERR_ARG and "aligned" in last() and call(d, objs=p(rec.objs) + 2) == sc_.ERR_ARG and call(d, pc=p(rec.counts) + 1) == sc_.ERR_ARG
    assert call(d, ov=p(rec.override) + 2) == sc_.ERR_ARG and "aligned" in last()
    assert untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == sc_.ERR_ARG and call(d) == sc_.ERR_ARG and call(d, n=0) == sc_.ERR_ARG and call(f, n=0) == sc_.ERR_ARG
    assert untouched()


def test_capacity_zero(pkg, emul, orc):
    """no room for a record: every tile is empty, and the [n][capacity] and [n][list_capacity] arrays may be NULL"""
    case = BY_NAME["mixed"]
    sc, stats, v, g, rec, lcap, res, tally = sc_.model(orc, case)
    sc_.configure(pkg, emul, case)
    n = len(case.tiles)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    got = emul.tiles_scenery_view(case.tiles, st, tvc.lib_view(pkg, v), sc_.lib_args(pkg, g.a), np.zeros((n, 0), pkg.SCENERY_PLACE_DTYPE), rec.counts, fill=sc_.FILL)
    assert not got["tile"].view(np.uint8).any() and not got["group_counts"].any() and got["list"].size == 0
    # room for the records, none for the lists: the words and the counts come out, list may be NULL
    got = emul.tiles_scenery_view(case.tiles, st, tvc.lib_view(pkg, v), sc_.lib_args(pkg, g.a), rec.objs, rec.counts, 0, rec.skip, rec.override, fill=sc_.FILL)
    sc_.compare("list_capacity 0", got, res, 0)


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_scenery_view.py::test_resident_chain on the emulator's "device" memory"""
    sc_.run_resident_chain(pkg, emul, orc)
