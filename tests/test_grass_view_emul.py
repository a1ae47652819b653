"""The grass draw lists (terra_tiles_grass_view[_dev], terra_make_view, terra_set_grass_view_params) through the host emulator -- the driver's one-thread-per-tile
form -- against tests/grass_view_model.py: insts, aux, group_counts, counts and pass byte for byte and in order; the view constructor bit for bit; the settings and
the refusals.

test_model_alone passes without the feature; every other test needs its entry points and fails without it."""
import ctypes

import numpy as np
import pytest

import grass_view_cases as gc
import grass_view_model as gm
import view_model
import orclib

CASES = gc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32

VIEWS = [dict(pos=(0.3, 0.2, 0.4), dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), angle=0.5, aspect=1.5, near=0.05, far=5.0),
         dict(pos=(-15.0, 7.0, 2.5), dir=(0.6, 0.5, -0.4), up=(0.1, 0.0, 1.0), angle=0.9, aspect=1.0, near=0.0, far=60.0),
         dict(pos=(1.0, 2.0, 3.0), dir=(0.0, 0.0, -2.0), up=(0.0, 1.0, 0.0), angle=1.2, aspect=0.7, near=0.01, far=100.0),
         dict(pos=(0.0, 0.0, 0.0), dir=(0.3, -0.8, 0.1), up=(0.0, 0.0, 1.0), angle=2.0, aspect=1.0, near=1.0, far=2.0),   # angle > 90 degrees: fine while aspect == 1
         dict(pos=(0.0, 0.0, 0.0), dir=(0.0, 0.0, 1.0), up=(0.0, 0.0, 1.0), angle=0.4, aspect=2.0, near=0.1, far=9.0)]    # up along dir: upv_ stays unnormalized (zero)
BAD_VIEWS = [dict(near=-0.1), dict(far=0.05), dict(near=2.0, far=1.0), dict(dir=(0.0, 0.0, 0.0)), dict(angle=2.0, aspect=1.5), dict(angle=0.0, aspect=1.5)]


def test_model_alone(orc):
    """the model's own invariants on every case: group counts sum to the counts, the lists are grouped by (lod, bix) in draw order, and within a group the instances
    are in (y, x) scan order"""
    for case in CASES:
        sc, z, stats, gb, v, lists, g, ps, tally = gc.model(orc, case)
        assert case.check(tally, lists, ps), (case.name, tally)
        for t, lst in enumerate(lists):
            assert int(g[t].sum()) == len(lst)
            keys = [(lod, bix) for (x, y, lod, bix) in lst]
            assert keys == sorted(keys), (case.name, t)
            for lod in range(gm.NUM_GRASS_LODS):
                for bix in range(case.nrnd):
                    grp = [(y, x) for (x, y, l, b) in lst if (l, b) == (lod, bix)]
                    assert len(grp) == int(g[t, lod, bix]) and grp == sorted(grp) and len(set(grp)) == len(grp), (case.name, t, lod, bix)
            if ps[t] == gm.NO_PASS:
                assert not lst
    # 1024 kept blocks at S = 128: one group holds more than 256 instances and the scatter's running sums span all 16 chunks of 64 keys
    t128 = gc.MODEL["full_s128"][8]
    assert t128["kept"] == 1024 and t128["max_group"] > 256, t128


def test_make_view(pkg, emul):
    """terra_make_view against the model's constructor (the C library's tanf / sinf / atanf through ctypes), bit for bit; refused where the constructor asserts"""
    for kw in VIEWS:
        want = view_model.make_view(**kw)
        got = emul.make_view(kw["pos"], kw["dir"], kw["up"], kw["angle"], kw["aspect"], kw["near"], kw["far"])
        assert bytes(got) == want.words(), (kw, [float(x) for x in got.upv], [float(x) for x in want.upv_])
    for bad in BAD_VIEWS:
        kw = dict(VIEWS[0], **bad)
        assert view_model.make_view(**kw) is None, bad
        out = pkg.View()
        ctypes.memset(ctypes.addressof(out), 0x5A, ctypes.sizeof(out))
        f3 = lambda a: (ctypes.c_float * 3)(*a)  # noqa: E731
        rc = emul.lib.terra_make_view(f3(kw["pos"]), f3(kw["dir"]), f3(kw["up"]), kw["angle"], kw["aspect"], kw["near"], kw["far"], ctypes.byref(out))
        assert rc == gc.ERR_ARG and bytes(out) == b"\x5a" * ctypes.sizeof(out), bad
    assert emul.lib.terra_make_view(None, None, None, 0.5, 1.0, 0.1, 1.0, None) == gc.ERR_ARG


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    gc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    gc.run_case(pkg, emul, orc, case, dev=True)


def test_without_aux_and_pass(pkg, emul, orc):
    gc.run_case(pkg, emul, orc, BY_NAME["mixed_nrnd3"], aux=False, want_pass=False)
    gc.run_case(pkg, emul, orc, BY_NAME["lods"], dev=True, aux=False, want_pass=False)


def test_grass_view_params(pkg, emul):
    assert emul.get_grass_view_params().tt_grass_scale_factor == 1.0  # the reference's default
    emul.set_grass_view_params(pkg.make_grass_view_params(0.25))
    assert emul.get_grass_view_params().tt_grass_scale_factor == 0.25
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.TerraError) as e:
            emul.set_grass_view_params(pkg.make_grass_view_params(bad))
        assert e.value.code == gc.ERR_ARG, bad
    assert emul.get_grass_view_params().tt_grass_scale_factor == 0.25  # a refused setting changes nothing
    assert emul.lib.terra_set_grass_view_params(emul.ctx, None) == gc.ERR_ARG and emul.lib.terra_get_grass_view_params(emul.ctx, None) == gc.ERR_ARG


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["lods"]
    sc, z, stats, gb, v, lists, g, ps, tally = gc.model(orc, case)
    S, n, cap, nrnd = case.S, len(case.tiles), case.capacity, case.nrnd
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda a: a.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(st)
    lv = gc.lib_view(pkg, v)
    vp = ctypes.byref(lv)
    ins, ax, cn, gcn, pb = np.full((n, cap, 2), 3.0, f32), np.full((n, cap), 3, np.uint32), np.full(n, 3, np.uint32), np.full((n, 6, nrnd), 3, np.uint32), np.full(n, 3, np.uint8)
    untouched = lambda: (ins == 3.0).all() and (ax == 3).all() and (cn == 3).all() and (gcn == 3).all() and (pb == 3).all()  # noqa: E731
    f, d = lib.terra_tiles_grass_view, lib.terra_tiles_grass_view_dev
    call = lambda fn, **kw: fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, kw.get("z", p(z)), kw.get("st", sp), kw.get("gb", p(gb)), None, kw.get("view", vp), kw.get("cap", cap),  # noqa: E731
                               kw.get("ins", p(ins)), kw.get("ax", p(ax)), kw.get("gc", p(gcn)), kw.get("cn", p(cn)), p(pb))
    # before terra_init_scene
    assert call(f) == gc.ERR_STATE and call(d) == gc.ERR_STATE and untouched()
    gc.configure(pkg, emul, case)
    # null pointers
    for fn in (f, d):
        assert call(fn, view=None) == gc.ERR_ARG and "null" in last()
        for k in ("txy", "z", "st", "gb", "gc", "cn", "ins"):
            assert call(fn, **{k: None}) == gc.ERR_ARG and "null" in last(), k
        assert call(fn, n=0, txy=None, z=None, st=None, gb=None, gc=None, cn=None, ins=None, ax=None) == 0
        assert call(fn, n=0, view=None) == gc.ERR_ARG
    assert untouched()
    # misaligned device pointers
    for k, a in (("z", z), ("gb", gb), ("ins", ins), ("ax", ax), ("gc", gcn), ("cn", cn)):
        assert call(d, **{k: p(a) + 2}) == gc.ERR_ARG and "aligned" in last(), k
    assert call(d, st=sp + 1) == gc.ERR_ARG and "aligned" in last()
    # a view with a non-finite member
    for field in ("pos", "cp"):
        bad = gc.lib_view(pkg, v)
        getattr(bad, field)[1] = float("nan")
        assert call(f, view=ctypes.byref(bad)) == gc.ERR_ARG and "finite" in last() and call(d, view=ctypes.byref(bad)) == gc.ERR_ARG
    bad = gc.lib_view(pkg, v)
    bad.far_ = float("inf")
    assert call(f, view=ctypes.byref(bad)) == gc.ERR_ARG and "finite" in last()
    assert untouched()
    # num_rnd_grass_blocks above 4096 (0 is refused by terra_set_landscape itself)
    emul.set_landscape(pkg.make_landscape(grass_density=1, num_rnd_grass_blocks=4097))
    assert call(f) == gc.ERR_ARG and "num_rnd_grass_blocks" in last() and call(d) == gc.ERR_ARG and untouched()
    with pytest.raises(pkg.TerraError):
        emul.set_landscape(pkg.make_landscape(grass_density=1, num_rnd_grass_blocks=0))
    emul.set_landscape(pkg.make_landscape(grass_density=1, num_rnd_grass_blocks=nrnd))
    # capacity 0: counts only
    assert call(f, cap=0, ins=None, ax=None) == 0 and cn.tolist() == [len(x) for x in lists] and gcn.tobytes() == g.tobytes() and pb.tolist() == ps.tolist()
    assert (ins == 3.0).all() and (ax == 3).all()
    cn[:], gcn[...], pb[:] = 3, 3, 3
    # a tile size that is not a multiple of 4, and an unsupported one
    z17, gb17 = np.zeros((n, 19, 19), f32), np.ones((n, 5, 5), orclib.GRASS_BLOCK_DTYPE)
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=17))
    assert call(f, z=p(z17), gb=p(gb17)) == gc.ERR_ARG and "multiple of 4" in last() and call(d, z=p(z17), gb=p(gb17)) == gc.ERR_ARG
    assert call(f, n=0) == gc.ERR_ARG  # n == 0 does nothing only once the scene and the tile size have passed
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert call(f) == gc.ERR_ARG and call(d) == gc.ERR_ARG and call(d, n=0) == gc.ERR_ARG
    assert untouched()


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_grass_view.py::test_resident_chain on the emulator's "device" memory"""
    gc.run_resident_chain(pkg, emul, orc)
