"""The tree map, the shadow texture and the tree weights (terra_tiles_tree_map, terra_tiles_shadow_texture, terra_tiles_tree_weights) through the host emulator --
the driver's per-row / per-texel forms -- against tests/tree_map_model.py, byte for byte, every tile and every texel of every case; plus the argument checks."""
import ctypes as C

import numpy as np
import pytest

import tree_map_cases as tmc
import tree_map_model as tmm


def test_model_mult_types():
    """the two points of the model's docstring: with a double sqrt, or with float products, mult would differ for some (rval, dist_sq)"""
    diff_sqrt = diff_float = 0
    for rval in range(1, 13):
        scale = np.float32(0.6 / rval)
        d2 = np.array(sorted({dx * dx + dy * dy for dx in range(rval + 1) for dy in range(rval + 1) if dx * dx + dy * dy <= rval * rval}), np.float32)
        m = tmm.mult_of(scale, d2)
        m_dsqrt = (0.2 + (0.8 * float(scale)) * np.sqrt(d2.astype(np.float64))).astype(np.float32)
        m_float = (np.float32(0.2) + (np.float32(0.8) * scale) * np.sqrt(d2)).astype(np.float32)
        diff_sqrt += int((m != m_dsqrt).sum()); diff_float += int((m != m_float).sum())
        assert m[0] == np.float32(0.2) and (m <= np.float32(0.8)).all()
    assert diff_sqrt > 0 and diff_float > 0


def test_order_matters_in_the_model(pkg, emul, orc):
    sc = tmc.setup(pkg, emul, orc)
    assert tmc.order_sensitive(sc) > 0


def test_cases(pkg, emul, orc):
    tmc.run_cases(pkg, emul, orc)


@pytest.mark.parametrize("S", [64, 192])
def test_cases_other_sizes(pkg, emul, orc, S):
    tmc.run_cases(pkg, emul, orc, S)


def test_cases_dx_differs_from_dy(pkg, emul, orc):
    """X_SCENE_SIZE != Y_SCENE_SIZE at S = 128: rval takes the larger of the two quotients, the window's texels are not square"""
    sc = tmc.run_cases(pkg, emul, orc, 128, (4.0, 6.0, 4.0), only=("rvals", "borders", "clusters", "skipped"))
    assert sc.DX_VAL != sc.DY_VAL


def test_continue(pkg, emul, orc):
    tmc.run_continue(pkg, emul, orc)


def test_dev_entry_point(pkg, emul, orc):
    """the device-pointer form on the emulator's "device" memory, updated optional"""
    sc = tmc.setup(pkg, emul, orc)
    per_tile = [c for c in tmc.cases(sc) if c[0] == "clusters"][0][1]
    sp, first = tmc.lists(per_tile)
    n = len(tmc.TILES)
    sb, mb, ub = emul.alloc(sp.nbytes).upload(sp), emul.alloc(n * 129 * 129 * 2), emul.alloc(n)
    try:
        emul.tiles_tree_map_dev(tmc.TILES, sb.ptr, first, mb.ptr, ub.ptr)
        want, wupd = tmm.tiles_tree_map(sc, tmc.TILES, sp, first, True)
        tmc.compare("dev", mb.download(np.uint8, want.shape), ub.download(np.uint8, (n,)), want, wupd)
        emul.tiles_tree_map_dev(tmc.TILES, sb.ptr, first, mb.ptr, None)  # no updated
        tmc.compare("dev, no updated", mb.download(np.uint8, want.shape), wupd, want, wupd)
    finally:
        for b in (sb, mb, ub):
            b.free()


@pytest.mark.parametrize("S", [64, 128, 192])
def test_shadow_texture_exhaustive(pkg, emul, orc, S):
    tmc.run_shadow_texture(pkg, emul, orc, S)


def test_tree_weights(pkg, emul, orc):
    """a fixed stride of the 256^3 (tree_ao, dirt, grass) combinations (all of them run on the GPU), the rock-255 skip, no tree map, and in place"""
    tmc.setup(pkg, emul, orc)
    w, tree = tmc.weights_inputs(stride=61)
    assert len(np.unique(tree[..., 0])) == 256 and len(np.unique(w[..., 1])) == 256 and len(np.unique(w[..., 2])) == 256
    want = tmm.tree_weights(w, tree)
    got = emul.tiles_tree_weights(w, tree)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[0].tolist()}: {w[tuple(bad[0][:3])]} tree {tree[tuple(bad[0][:3])]} -> {got[tuple(bad[0][:3])]} != {want[tuple(bad[0][:3])]}"
    assert (want != w).any() and (want[..., 0] == w[..., 0]).all() and (want[..., 3] == w[..., 3]).all()
    w255, _ = tmc.weights_inputs(stride=61, rock255=True)
    assert (emul.tiles_tree_weights(w255, tree) == w255).all() and (tmm.tree_weights(w255, tree) == w255).all()
    assert (emul.tiles_tree_weights(w, None) == w).all()
    n = len(w)
    wb, tb = emul.alloc(w.nbytes).upload(w), emul.alloc(tree.nbytes).upload(tree)
    try:
        emul.tiles_tree_weights_dev(n, wb.ptr, tb.ptr, wb.ptr)  # in place
        assert (wb.download(np.uint8, w.shape) == want).all()
    finally:
        wb.free(); tb.free()


def test_refused(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    n = 2
    txy = np.array(tmc.TILES[:n], np.int32)
    first = np.array([0, 1, 2], np.uint32)
    sp = np.zeros(2, tmm.SPLAT_DTYPE)
    tm, upd = np.zeros((n, 129, 129, 2), np.uint8), np.zeros(n, np.uint8)
    sm, ao, sh = np.zeros((n, 130, 130), np.uint8), np.zeros((n, 129, 129), np.uint8), np.zeros((n, 129, 129, 4), np.uint8)
    w = np.zeros((n, 129, 129, 4), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def tree_map(txy_=txy, first_=first, sp_=sp, tm_=tm, nn=n):
        return lib.terra_tiles_tree_map(ctx, p(txy_), nn, 0, 0, None, p(sp_), p(first_), 1, p(tm_), p(upd))

    def shadow(lf=0.5, ms=1, sun=sm, moon=sm, out=sh, nn=n):
        return lib.terra_tiles_shadow_texture(ctx, nn, p(sun), p(moon), p(ao), p(tm), lf, ms, p(out))

    # before terra_init_scene
    assert tree_map() == tmc.ERR_STATE and shadow() == tmc.ERR_STATE and lib.terra_tiles_tree_weights(ctx, n, p(w), p(tm), p(w)) == tmc.ERR_STATE
    tmc.setup(pkg, emul, orc)
    assert tree_map() == 0 and shadow() == 0 and lib.terra_tiles_tree_weights(ctx, n, p(w), p(tm), p(w)) == 0
    # tree map: a null required pointer, a decreasing h_first, n == 0
    assert tree_map(txy_=None) == tmc.ERR_ARG and tree_map(first_=None) == tmc.ERR_ARG and tree_map(tm_=None) == tmc.ERR_ARG and tree_map(sp_=None) == tmc.ERR_ARG
    assert tree_map(first_=np.array([0, 2, 1], np.uint32)) == tmc.ERR_ARG
    assert "h_first" in lib.terra_last_error().decode()
    assert tree_map(txy_=None, first_=None, sp_=None, tm_=None, nn=0) == 0
    assert tree_map(first_=np.zeros(3, np.uint32), sp_=None) == 0  # empty lists need no splat array
    assert lib.terra_tiles_tree_map_dev(ctx, p(txy), n, 0, 0, None, p(sp), p(first), 1, tm.ctypes.data + 1, p(upd)) == tmc.ERR_ARG  # not 2-byte aligned
    assert "aligned" in lib.terra_last_error().decode()
    assert lib.terra_tiles_tree_map_dev(ctx, p(txy), n, 0, 0, None, p(sp), p(np.array([0, 2, 1], np.uint32)), 1, p(tm), p(upd)) == tmc.ERR_ARG
    assert lib.terra_tiles_tree_map_dev(ctx, p(txy), n, 0, 0, None, None, p(first), 1, p(tm), p(upd)) == tmc.ERR_ARG
    # shadow texture: where the reference asserts
    assert shadow(sun=None) == tmc.ERR_ARG and shadow(moon=None) == tmc.ERR_ARG  # both lights up at 0.5
    assert shadow(lf=0.7, moon=None) == 0 and shadow(lf=0.7, sun=None) == tmc.ERR_ARG
    assert shadow(lf=0.3, sun=None) == 0 and shadow(lf=0.3, moon=None) == tmc.ERR_ARG
    assert shadow(ms=0, sun=None, moon=None) == 0
    assert shadow(lf=float("nan")) == tmc.ERR_ARG and "neither light" in lib.terra_last_error().decode()
    assert shadow(out=None) == tmc.ERR_ARG and shadow(out=None, nn=0) == 0
    assert lib.terra_tiles_shadow_texture_dev(ctx, n, p(sm), p(sm), p(ao), p(tm), 0.5, 1, sh.ctypes.data + 2) == tmc.ERR_ARG
    assert "aligned" in lib.terra_last_error().decode()
    # tree weights: null pointers, and the weights family's refusal at another tile size
    assert lib.terra_tiles_tree_weights(ctx, n, None, p(tm), p(w)) == tmc.ERR_ARG and lib.terra_tiles_tree_weights(ctx, n, p(w), p(tm), None) == tmc.ERR_ARG
    assert lib.terra_tiles_tree_weights_dev(ctx, n, w.ctypes.data + 2, p(tm), p(w)) == tmc.ERR_ARG
    emul.init_scene(pkg.make_config(mesh_xy=64))
    for fn in (lib.terra_tiles_tree_weights, lib.terra_tiles_tree_weights_dev):
        assert fn(ctx, n, p(w), p(tm), p(w)) == tmc.ERR_ARG
        assert "tile size 128" in lib.terra_last_error().decode()
    # an unsupported tile size refuses the other two
    emul.init_scene(pkg.make_config(mesh_xy=130))
    assert tree_map() == tmc.ERR_ARG and shadow() == tmc.ERR_ARG
