"""The clouds of a tile batch (terra_tiles_update_clouds[_dev], terra_tiles_cloud_view[_dev], terra_set_cloud_params) through the host emulator -- the driver's simple
form: the reference's loops, sequential over the batch -- against tests/cloud_model.py: after every call the state, the records up to count and the total, for the view
the stage bytes and the list up to list_count, byte for byte; the refusals with every output untouched.

test_model_alone passes without the feature; every other test needs its entry points and fails without them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cloud_cases as cc
import cloud_model as cm
import terrain_view_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UCASES, VCASES = cc.update_cases(), cc.view_cases()
U_BY_NAME, V_BY_NAME = {c.name: c for c in UCASES}, {c.name: c for c in VCASES}
f32 = np.float32


def test_model_alone(orc):
    """every case exercises what it is named for, on the model alone; the generator is the reference's; the order pair differs in its answers"""
    # the model's generator against the reference's compiled one, from seeds as gen() makes them (x1 + 123, y1 + 321), negative ones included
    for s1, s2 in [(123, 321), (1, 123), (-2048 + 123, -16 + 321), (123 - 16, 321 + 128), (-53668, -52774)]:
        r = cm.RandGen(s1, s2)
        assert [r.rand() for _ in range(64)] == orc.rand_ints(s1, s2, 64).tolist(), (s1, s2)
        for a, b in [(0.6, 1.0), (2.0, 4.0), (-36.0, -28.0)]:
            r = cm.RandGen(s1, s2)
            got = np.array([r.rand_uniform(a, b) for _ in range(64)], f32)
            assert got.tobytes() == orc.rand_uniforms(s1, s2, a, b, 64).tobytes(), (s1, s2, a, b)
    for seed in (1, 7):
        g = cm.gauss_table(orc, seed)
        assert len(g) == 10002 and abs(float(g.mean())) < 0.05 and 0.9 < float(g.std()) < 1.1 and float(np.abs(g).max()) < 5.5, seed  # (|g| < 5.5: num_clouds <= clouds_per_tile + 22)
    for case in UCASES:
        sc, step, frames, tally = cc.model(orc, case)
        assert case.check(tally), (case.name, {k: x for k, x in tally.items() if x})
        assert 0.099 <= max(abs(w) for w in case.wind[:2]) <= 0.5 or case.name in ("zero_wind", "wind_z_alone", "stay_only"), case.name
        for s_in, c_in, state, clouds, total in frames:
            assert (state["count"] <= case.capacity).all() and total <= int(state["count"].sum()), case.name  # (num: the sizes at the tiles' turns)
    # density 0 makes no draw: the seeds are gen's
    sc, step, frames, tally = cc.model(orc, U_BY_NAME["density_zero"])
    for (tx, ty), s in zip(U_BY_NAME["density_zero"].tiles, frames[-1][2]):
        assert (int(s["rseed1"]), int(s["rseed2"])) == (tx * 16 + 123, ty * 16 + 321)
    # two batches that differ in order alone: the model's answers differ
    ab, ba = cc.model(orc, U_BY_NAME["to_later_moved_twice"])[2][1], cc.model(orc, U_BY_NAME["to_earlier_moved_once"])[2][1]
    assert ab[0].tobytes() == ba[0][::-1].tobytes() and ab[1].tobytes() == ba[1][::-1].tobytes(), "the two batches start frame 1 from the same tiles"
    assert ab[2].tobytes() != ba[2][::-1].tobytes()
    # num is the sum of the sizes at the tiles' turns: a cloud handed to an earlier tile is not in it
    fr = cc.model(orc, U_BY_NAME["to_earlier_moved_once"])[2]
    assert any(total < int(state["count"].sum()) for _, _, state, _, total in fr)
    # overflow: the sticky bit, and count at the capacity
    st = cc.model(orc, U_BY_NAME["overflow"])[2][-1][2]
    assert (st["flags"] & cm.OVERFLOW).any() and (st["count"] <= 4).all()
    union = cm.new_tally()
    for case in VCASES:
        res = cc.view_model(orc, case)
        assert case.check(res[7]), (case.name, {k: x for k, x in res[7].items() if x})
        stage, lst = res[6]
        assert len(lst) == int((stage == cm.LISTED).sum()) and (np.diff(lst["dist_sq"]) >= 0).all(), case.name
        for k, x in res[7].items():
            union[k] += x
    assert all(union[k] > 0 for k in ("vfc", "below_zmin", "below_water", "below_mesh", "listed", "alpha_one_high", "alpha_one_near", "alpha_frac", "too_distant", "drawn", "ties")), union
    # the tie rule: equal keys in (tile, slot) order
    lst = cc.view_model(orc, V_BY_NAME["ties"])[6][1]
    eq = [i for i in range(len(lst) - 1) if lst["dist_sq"][i] == lst["dist_sq"][i + 1]]
    assert len(eq) >= 6 and all((lst["tile"][i], lst["slot"][i]) < (lst["tile"][i + 1], lst["slot"][i + 1]) for i in eq)
    assert len({int(lst["tile"][i]) for i in eq}) >= 3


@pytest.mark.parametrize("case", UCASES, ids=[c.name for c in UCASES])
def test_update_cases(pkg, emul, orc, case):
    cc.run_update_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", UCASES, ids=[c.name for c in UCASES])
def test_update_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    cc.run_update_case(pkg, emul, orc, case, dev=True)


@pytest.mark.parametrize("case", VCASES, ids=[c.name for c in VCASES])
def test_view_cases(pkg, emul, orc, case):
    cc.run_view_case(pkg, emul, orc, case)
    cc.run_view_case(pkg, emul, orc, case, dev=True)


def test_params(pkg, emul):
    lib, ctx = emul.lib, emul.ctx
    p = emul.get_cloud_params()
    assert (p.clouds_per_tile, p.cloud_height_offset, p.rgen_seed) == (0.5, 0.0, 1)
    emul.set_cloud_params(pkg.make_cloud_params(3.0, -0.25, 9))
    p = emul.get_cloud_params()
    assert (p.clouds_per_tile, p.cloud_height_offset, p.rgen_seed) == (3.0, -0.25, 9)
    for bad in (pkg.make_cloud_params(-1.0), pkg.make_cloud_params(float("nan")), pkg.make_cloud_params(float("inf")), pkg.make_cloud_params(1000.5),
                pkg.make_cloud_params(1.0, float("nan")), pkg.make_cloud_params(1.0, float("-inf"))):
        assert lib.terra_set_cloud_params(ctx, ctypes.byref(bad)) == cc.ERR_ARG
    assert lib.terra_set_cloud_params(ctx, None) == cc.ERR_ARG and lib.terra_get_cloud_params(ctx, None) == cc.ERR_ARG
    p = emul.get_cloud_params()
    assert (p.clouds_per_tile, p.cloud_height_offset, p.rgen_seed) == (3.0, -0.25, 9)
    emul.set_cloud_params(pkg.make_cloud_params(1000.0, 0.0, 1))


def test_gauss_seed(pkg, emul, orc):
    """another rgen_seed: another table, another num_clouds"""
    case = cc.Case("gauss_seed_7", params=dict(clouds_per_tile=2.0, rgen_seed=7), frames=2)
    other = cc.Case("gauss_seed_1", params=dict(clouds_per_tile=2.0), frames=2)
    assert cc.model(orc, case)[2][0][2]["num_clouds"].tolist() != cc.model(orc, other)[2][0][2]["num_clouds"].tolist()
    cc.run_update_case(pkg, emul, orc, case)
    cc.run_update_case(pkg, emul, orc, other)  # (and back: the table follows the seed)


def test_update_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = U_BY_NAME["diagonal"]
    sc, step, frames, tally = cc.model(orc, case)
    n, cap = len(case.tiles), case.capacity
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    s0, c0 = frames[0][2].copy(), frames[0][3].copy()
    st, cl, to = s0.copy(), c0.copy(), np.full(1, 3, np.uint32)
    untouched = lambda: st.tobytes() == s0.tobytes() and cl.tobytes() == c0.tobytes() and to[0] == 3  # noqa: E731
    ls = cc.lib_step(pkg, step)
    f, d = lib.terra_tiles_update_clouds, lib.terra_tiles_update_clouds_dev

    def call(fn, **kw):
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), kw.get("step", ctypes.byref(ls)), kw.get("st", p(st)), kw.get("cl", p(cl)), kw.get("cap", cap), kw.get("to", p(to)))
    assert call(f) == cc.ERR_STATE and call(d) == cc.ERR_STATE and untouched()
    cc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, step=None) == cc.ERR_ARG and "null" in last()
        for k in ("txy", "st", "cl"):
            assert call(fn, **{k: None}) == cc.ERR_ARG and "null" in last(), k
        assert call(fn, cap=0, cl=None) == cc.ERR_ARG and "capacity" in last()
        for k in range(4):
            for val in (float("nan"), float("inf"), float("-inf")):
                bad = cc.lib_step(pkg, step)
                if k < 3:
                    bad.wind[k] = val
                else:
                    bad.fticks = val
                assert call(fn, step=ctypes.byref(bad)) == cc.ERR_ARG and "finite" in last(), (k, val)
                assert call(fn, n=0, step=ctypes.byref(bad)) == cc.ERR_ARG
        twice = txy.copy()
        twice[5] = twice[2]
        assert call(fn, txy=p(twice)) == cc.ERR_ARG and "twice" in last()
        assert untouched()
        # n == 0 writes total = 0 and nothing else
        assert call(fn, n=0, txy=None, st=None, cl=None) == 0 and to[0] == 0 and st.tobytes() == s0.tobytes() and cl.tobytes() == c0.tobytes()
        assert call(fn, n=0, txy=None, st=None, cl=None, to=None) == 0
        to[0] = 3
    assert call(d, st=p(st) + 4) == cc.ERR_ARG and "aligned" in last() and call(d, cl=p(cl) + 2) == cc.ERR_ARG and "aligned" in last()
    assert call(d, to=p(to) + 2) == cc.ERR_ARG and "aligned" in last() and untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=66))
    assert call(f) == cc.ERR_ARG and call(d) == cc.ERR_ARG and untouched()
    # total is optional
    cc.configure(pkg, emul, case)
    assert call(f, to=None) == 0 and st.tobytes() == frames[1][2].tobytes()


def test_view_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = V_BY_NAME["xlate"]
    sc, v, a, stats, state, clouds, res, tally = cc.view_model(orc, case)
    n, cap = len(case.tiles), case.capacity
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    lst_ = (pkg.TileStats * n).from_buffer_copy(stats)
    sp = ctypes.addressof(lst_)
    lv, la = tc.lib_view(pkg, v), cc.lib_view_args(pkg, a)
    vp, ap = ctypes.byref(lv), ctypes.byref(la)
    out = dict(sg=np.full(n * cap, 3, np.uint8), li=np.full(n * cap * 6, 3, np.uint32), lc=np.full(1, 3, np.uint32))
    untouched = lambda: all((x == 3).all() for x in out.values())  # noqa: E731
    f, d = lib.terra_tiles_cloud_view, lib.terra_tiles_cloud_view_dev

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), kw.get("view", vp), kw.get("args", ap), kw.get("ss", sp), kw.get("st", p(state)), kw.get("cl", p(clouds)), cap,
                  o["sg"], o["li"], o["lc"])
    assert call(f) == cc.ERR_STATE and call(d) == cc.ERR_STATE and untouched()
    cc.configure(pkg, emul, case)
    for fn in (f, d):
        assert call(fn, view=None) == cc.ERR_ARG and "null" in last() and call(fn, args=None) == cc.ERR_ARG and "null" in last()
        for k in ("txy", "ss", "st", "cl", "sg", "li", "lc"):
            assert call(fn, **{k: None}) == cc.ERR_ARG and "null" in last(), k
        for k in range(5):
            for val in (float("nan"), float("inf")):
                bad = cc.lib_view_args(pkg, a)
                if k == 0:
                    bad.behind_sphere_mult = val
                elif k < 4:
                    bad.xlate[k - 1] = val
                else:
                    bad.max_dist = val
                assert call(fn, args=ctypes.byref(bad)) == cc.ERR_ARG and "finite" in last(), (k, val)
        for val in (0.0, -1.0):
            bad = cc.lib_view_args(pkg, a)
            bad.max_dist = val
            assert call(fn, args=ctypes.byref(bad)) == cc.ERR_ARG and "max_dist" in last()
            assert call(fn, n=0, args=ctypes.byref(bad)) == cc.ERR_ARG
        bad = tc.lib_view(pkg, v)
        bad.pos[1] = float("nan")
        assert call(fn, view=ctypes.byref(bad)) == cc.ERR_ARG and "finite" in last()
        assert untouched()
        assert call(fn, n=0, txy=None, ss=None, st=None, cl=None, sg=None, li=None) == 0 and out["lc"][0] == 0 and (out["sg"] == 3).all() and (out["li"] == 3).all()
        out["lc"][0] = 3
    assert call(d, st=p(state) + 4) == cc.ERR_ARG and "aligned" in last() and call(d, li=p(out["li"]) + 2) == cc.ERR_ARG and "aligned" in last()
    assert call(d, ss=sp + 1) == cc.ERR_ARG and "aligned" in last() and call(d, lc=p(out["lc"]) + 2) == cc.ERR_ARG and "aligned" in last() and untouched()
    # a heightmap texture: the exact height is not this call's
    buf = emul.alloc(64 * 64 * 2).upload(np.zeros(64 * 64 * 2, np.uint8))
    try:
        emul.hmap_set_dev(buf.ptr, 64, 64, 2)
        assert call(f) == cc.ERR_STATE and call(d) == cc.ERR_STATE and "heightmap" in last() and untouched()
    finally:
        emul.hmap_set_dev(None)
        buf.free()


def test_replay_host_program(tmp_path):
    """tests/clouds_replay_check.cpp: the kernels' split of the update (marks, tiles without traffic, ordered replay), compiled for the host under
    -fsanitize=address,undefined, against the literal loop on randomised traffic"""
    exe = str(tmp_path / "clouds_replay_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "clouds_replay_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)"), r.stdout + r.stderr


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_clouds.py::test_resident_chain on the emulator's "device" memory"""
    cc.run_resident_chain(pkg, emul, orc)
