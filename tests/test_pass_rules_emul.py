"""The argument rules of the terrain view, the reflection view, the water view, the clouds' update and the cloud view exist once per pass (terrain_view_io_check,
water_view_io_check, cloud_update_io_check, cloud_view_io_check in the pass headers), and the host form and the device form of an entry point both call them:
for every required array in turn a null pointer is refused by both forms with the same error code and the same terra_last_error() text, which names the pass;
n == 0 with otherwise valid arguments is OK in both forms and writes nothing but the cloud passes' count word.  Through the host emulator, on the batches of the
passes' own *_refused_and_zero tests."""
import ctypes

import numpy as np
import pytest

import cloud_cases as cc
import terrain_view_cases as tc
import water_view_cases as wc
from test_clouds_emul import U_BY_NAME, V_BY_NAME
from test_terrain_view_emul import BY_NAME
from test_water_view_emul import R_BY_NAME, W_BY_NAME

f32 = np.float32
p = lambda x: x.ctypes.data  # noqa: E731


class Pass:
    """name: what the refusals call the pass; f, d: the host and the device entry point; call(fn, **kw): a call with the named arguments replaced; required: the
    arrays that must not be null; outputs: every array a call may write, filled with 3; count: the key of the count word that n == 0 zeroes, or None"""
    def __init__(self, name, f, d, call, required, outputs, count=None):
        self.name, self.f, self.d, self.call, self.required, self.outputs, self.count = name, f, d, call, required, outputs, count
        self.untouched = lambda: all((x == 3).all() for x in outputs.values())


def terrain_pass(pkg, emul, orc, reflection):
    lib, ctx = emul.lib, emul.ctx
    case = R_BY_NAME["order_a_before_b"] if reflection else BY_NAME["ridge_low_camera"]
    sc, stats, v, a = (wc.model(orc, case) if reflection else tc.model(orc, case))[:4]
    n = len(case.tiles)
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), (wc.lib_args(pkg, a) if reflection else tc.lib_args(pkg, a))
    mn = np.full(n, 0.5, f32)
    out = dict(os=np.full(n, 3, np.uint8), su=np.full(n, 3, np.uint8), di=np.full(n, 3.0, f32), lo=np.full(n, 3, np.uint8), cr=np.full((n, 4), 3, np.uint8),
               dr=np.full(n, 3, np.uint32), oc=np.full(n, 3, np.uint32), cn=np.full(2, 3, np.uint32), nd=np.full(n, 3, np.uint8), rf=np.full(n, 3, np.uint8))
    tc.configure(pkg, emul, case)

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        args = [ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, ctypes.byref(lv), ctypes.byref(la), kw.get("st", ctypes.addressof(st)), p(mn), None, None, None,
                o["os"], o["su"], o["di"], o["lo"], o["cr"], o["dr"], o["oc"], o["cn"], o["nd"]]
        return fn(*(args + [o["rf"]] if reflection else args))
    name = "tiles_reflection_view" if reflection else "tiles_terrain_view"
    return Pass(name, getattr(lib, "terra_" + name), getattr(lib, "terra_" + name + "_dev"), call, ("txy", "st", "su", "di", "lo", "cr", "dr", "oc", "cn"), out)


def water_pass(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = W_BY_NAME["caps_occluded_dry"]
    sc, stats, v, a, arr, status = wc.water_model(orc, case)[:6]
    n = len(case.tiles)
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), wc.lib_water_args(pkg, a)
    su = np.ascontiguousarray(status, np.uint8)
    out = dict(wl=np.full(n, 3, np.uint32), cm=np.full(n, 3, np.uint8), cn=np.full(2, 3, np.uint32))
    tc.configure(pkg, emul, case)

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), 0, 0, ctypes.byref(lv), ctypes.byref(la), kw.get("st", ctypes.addressof(st)), None, None, None, kw.get("su", p(su)),
                  o["wl"], o["cm"], o["cn"])
    return Pass("tiles_water_view", lib.terra_tiles_water_view, lib.terra_tiles_water_view_dev, call, ("txy", "st", "wl", "cn"), out)


def cloud_update_pass(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = U_BY_NAME["diagonal"]
    sc, step, frames, tally = cc.model(orc, case)
    n, cap = len(case.tiles), case.capacity
    txy = np.array(case.tiles, np.int32)
    s0, c0 = frames[0][2].copy(), frames[0][3].copy()
    st, cl = s0.copy(), c0.copy()
    out = dict(to=np.full(1, 3, np.uint32))
    ls = cc.lib_step(pkg, step)
    cc.configure(pkg, emul, case)

    def call(fn, **kw):
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), ctypes.byref(ls), kw.get("st", p(st)), kw.get("cl", p(cl)), cap, kw.get("to", p(out["to"])))
    ps = Pass("tiles_update_clouds", lib.terra_tiles_update_clouds, lib.terra_tiles_update_clouds_dev, call, ("txy", "st", "cl"), out, count="to")
    base = ps.untouched
    ps.untouched = lambda: base() and st.tobytes() == s0.tobytes() and cl.tobytes() == c0.tobytes()
    return ps


def cloud_view_pass(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case = V_BY_NAME["xlate"]
    sc, v, a, stats, state, clouds = cc.view_model(orc, case)[:6]
    n, cap = len(case.tiles), case.capacity
    txy = np.array(case.tiles, np.int32)
    st = (pkg.TileStats * n).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), cc.lib_view_args(pkg, a)
    out = dict(sg=np.full(n * cap, 3, np.uint8), li=np.full(n * cap * 6, 3, np.uint32), lc=np.full(1, 3, np.uint32))
    cc.configure(pkg, emul, case)

    def call(fn, **kw):
        o = {k: kw.get(k, p(x)) for k, x in out.items()}
        return fn(ctx, kw.get("txy", p(txy)), kw.get("n", n), ctypes.byref(lv), ctypes.byref(la), kw.get("ss", ctypes.addressof(st)), kw.get("st", p(state)), kw.get("cl", p(clouds)), cap,
                  o["sg"], o["li"], o["lc"])
    return Pass("tiles_cloud_view", lib.terra_tiles_cloud_view, lib.terra_tiles_cloud_view_dev, call, ("txy", "ss", "st", "cl", "sg", "li", "lc"), out, count="lc")


PASSES = {"terrain_view": lambda *a: terrain_pass(*a, False), "reflection_view": lambda *a: terrain_pass(*a, True), "water_view": water_pass,
          "update_clouds": cloud_update_pass, "cloud_view": cloud_view_pass}


@pytest.mark.parametrize("which", list(PASSES))
def test_host_and_device_form_share_the_rules(pkg, emul, orc, which):
    ps = PASSES[which](pkg, emul, orc)
    last = lambda: emul.lib.terra_last_error().decode()  # noqa: E731
    # a null pointer for each required array in turn: the same code and the same text, which names the pass, from both forms
    for k in ps.required:
        got = []
        for fn in (ps.f, ps.d):
            got.append((ps.call(fn, **{k: None}), last()))
        assert got[0][0] == got[1][0] == tc.ERR_ARG, (k, got)
        assert got[0][1] == got[1][1] and ps.name in got[0][1] and "null" in got[0][1], (k, got)
    assert ps.untouched()
    # the water view's both-or-neither rule comes before n == 0
    if which == "water_view":
        for kw in (dict(cm=None), dict(su=None)):
            got = [(ps.call(fn, n=0, **kw), last()) for fn in (ps.f, ps.d)]
            assert got[0][0] == got[1][0] == tc.ERR_ARG and got[0][1] == got[1][1] and ps.name in got[0][1] and "both" in got[0][1], (kw, got)
        assert ps.untouched()
    # n == 0 with otherwise valid arguments: OK from both forms, the cloud passes' count word is 0, nothing else is written
    for fn in (ps.f, ps.d):
        assert ps.call(fn, n=0) == 0
        if ps.count:
            assert ps.outputs[ps.count][0] == 0
            ps.outputs[ps.count][0] = 3
        assert ps.untouched()
