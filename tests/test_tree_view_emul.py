"""The pine and palm tree draw lists (terra_tiles_tree_view[_dev]) through the host emulator -- the driver's one-thread-per-tile form -- against
tests/tree_view_model.py: the tile records, both instance lists, the leaf list, the counts and the trunk bytes byte for byte, all_bcube by value; the refusals with
every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without it."""
import ctypes

import numpy as np
import pytest

import terrain_view_cases as tvc
import tree_view_cases as tc
import tree_view_model as vm

CASES = tc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_alone(orc):
    """every case reaches what it is named for, on the model alone; the lists are consistent with the flags; the orders are what the header states"""
    for case in CASES:
        sc, stats, v, g, rec, res, tally = tc.model(orc, case)
        assert case.check(tally, res), (case.name, tally)
        for t, w in enumerate(res):
            ids = [i for i, _ in w.pine_insts]
            assert ids == sorted(ids) and [i for i, _ in w.palm_insts] == sorted(i for i, _ in w.palm_insts), case.name
            if not w.written:
                assert w.flags == 0 and w.trunk is None and not w.pine_insts and w.leaf_pine is None, case.name
                continue
            mode = w.flags & 3
            assert all(b == 0 for b in w.trunk) or mode in (vm.TRUNK_POLY_ALL, vm.TRUNK_POLY_SKIPPED), case.name
            assert (1 in w.trunk) <= (mode == vm.TRUNK_POLY_SKIPPED) and all(b in (0, 1) or 4 <= b <= 32 for b in w.trunk), case.name
            assert not w.pine_insts or (g.instanced and w.flags & vm.NEAR_LEAVES), case.name
            assert not (w.palm_insts or w.leaf_palm) or w.flags & vm.PALMS, case.name
            if w.leaf_pine is not None:
                assert w.flags & vm.NEAR_LEAVES and not w.flags & vm.DRAW_ALL_NEAR and not g.instanced, case.name
                if not w.flags & vm.CONTAINS_CAMERA:
                    assert w.leaf_pine == sorted(w.leaf_pine), case.name
    # the big table exceeds what the kernel's histogram holds, the other stays within it
    assert sum(BY_NAME["instanced_big_table"].ninst) > tc.LDS_IDS >= sum(BY_NAME["instanced_many_ids"].ninst)
    # two cases exceed the capacity whose pairs the kernel ranks in LDS
    for name in ("camera_tile_large_capacity", "instanced_big_table_large_capacity"):
        assert tc.MODEL[name][4].cap > tc.LDS_KEYS == 2048, name
    # the camera tile's list is not in record order, and its equal keys come in index order
    w = tc.MODEL["camera_tile"][5][0]
    assert w.leaf_pine != sorted(w.leaf_pine) and w.leaf_pine.index(0) + 1 == w.leaf_pine.index(1)
    # a count above the capacity means the first `capacity` records
    sc, stats, v, g, rec, res, tally = tc.MODEL["many_records"]
    assert rec.counts[2] > rec.cap and res[2].num_trees == rec.cap


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    tc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    tc.run_case(pkg, emul, orc, case, dev=True)


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["instanced_many_ids"]
    sc, stats, v, g, rec, res, tally = tc.model(orc, case)
    n, cap = rec.pine.shape
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv, la = tvc.lib_view(pkg, v), tc.lib_args(pkg, g.a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    out = pkg.Terra._tree_view_outputs(n, cap, 3)
    names = pkg.Terra.TREE_VIEW_OUTPUTS
    untouched = lambda: all((x.view(np.uint8) == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_tree_view, lib.terra_tiles_tree_view_dev

    def call(fn, **kw):
        o = [kw.get(k, p(out[k])) for k in names]
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, 0, 0, kw.get("view", vp), kw.get("args", ap), kw.get("st", sp), None, None, kw.get("pine", p(rec.pine)),
                  kw.get("pc", p(rec.counts)), kw.get("cap", cap), None, *o)
    # before terra_init_scene
    assert call(f) == tc.ERR_STATE and call(d) == tc.ERR_STATE and untouched()
    tc.configure(pkg, emul, case, g)
    for fn in (f, d):
        assert call(fn, view=None) == tc.ERR_ARG and "null" in last() and call(fn, args=None) == tc.ERR_ARG and "null" in last()
        for k in ("txy", "st", "pine", "pc") + names:
            assert call(fn, **{k: None}) == tc.ERR_ARG and "null" in last(), k
        # n == 0 does nothing once the checks have passed
        assert call(fn, n=0, txy=None, st=None, pine=None, pc=None, **{k: None for k in names}) == 0
        assert call(fn, n=0, view=None) == tc.ERR_ARG
        # a view or args with a non-finite member
        for field in ("pos", "cp"):
            bad = tvc.lib_view(pkg, v)
            getattr(bad, field)[1] = float("nan")
            assert call(fn, view=ctypes.byref(bad)) == tc.ERR_ARG and "finite" in last(), field
        for field in ("behind_sphere_mult", "zoom_f", "tree_depth_scale"):
            for val in (float("nan"), float("inf")):
                bad = tc.lib_args(pkg, g.a)
                setattr(bad, field, val)
                assert call(fn, args=ctypes.byref(bad)) == tc.ERR_ARG and "finite" in last(), field
                assert call(fn, n=0, args=ctypes.byref(bad)) == tc.ERR_ARG
        # window_width, zoom_f, tree_depth_scale not > 0
        for field, val in (("window_width", 0), ("window_width", -5), ("zoom_f", 0.0), ("zoom_f", -1.0), ("tree_depth_scale", 0.0), ("tree_depth_scale", -2.0)):
            bad = tc.lib_args(pkg, g.a)
            setattr(bad, field, val)
            assert call(fn, args=ctypes.byref(bad)) == tc.ERR_ARG and "> 0" in last(), (field, val)
        # n*capacity beyond 32 bits
        assert call(fn, n=1 << 20, cap=1 << 13) == tc.ERR_ARG and "32 bits" in last()
    assert untouched()
    # misaligned device pointers
    for k in ("tile", "all_bcube", "pine_insts", "palm_insts", "inst_counts", "leaf_list", "leaf_counts"):
        assert call(d, **{k: p(out[k]) + 2}) == tc.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == tc.ERR_ARG and "aligned" in last() and call(d, pine=p(rec.pine) + 2) == tc.ERR_ARG and call(d, pc=p(rec.counts) + 1) == tc.ERR_ARG
    assert untouched()
    # `instanced` with an instance table of the wrong length
    emul.set_tree_instances(g.insts[:-1])
    assert call(f) == tc.ERR_ARG and "instances" in last() and call(d) == tc.ERR_ARG and call(d, n=0) == tc.ERR_ARG
    emul.set_tree_instances(g.insts)
    assert untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == tc.ERR_ARG and call(d) == tc.ERR_ARG and call(d, n=0) == tc.ERR_ARG and call(f, n=0) == tc.ERR_ARG
    assert untouched()


def test_capacity_zero(pkg, emul, orc):
    """no room for a record: every tile is empty, and the [n][capacity] arrays may be NULL"""
    case = BY_NAME["lod_ring"]
    sc, stats, v, g, rec, res, tally = tc.model(orc, case)
    tc.configure(pkg, emul, case, g)
    n = len(case.tiles)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    got = emul.tiles_tree_view(case.tiles, st, tvc.lib_view(pkg, v), tc.lib_args(pkg, g.a), np.zeros((n, 0), pkg.TREE_PLACE_DTYPE), rec.counts, fill=tc.FILL)
    assert not got["tile"].view(np.uint8).any() and not got["inst_counts"].any() and not got["leaf_counts"].any() and not got["all_bcube"].any()


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_tree_view.py::test_resident_chain on the emulator's "device" memory"""
    tc.run_resident_chain(pkg, emul, orc)
