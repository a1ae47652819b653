"""The tree AO shadows of a tile batch from the placement records (terra_tiles_tree_ao_shadows[_dev]) through the host emulator -- the driver's one-thread-per-tile
forms and the tree map's per-row form -- against tests/tree_ao_model.py, byte for byte: every map, updated, trmax and list_counts of every case, the resident chain
zvals -> both placements -> tree AO shadows -> shadow texture and tree weights, and the argument checks."""
import numpy as np
import pytest

import tree_ao_cases as tac
import tree_ao_chain as chain
import tree_ao_model as tam
import tree_map_model as tmm

CASES = tac.cases()


def test_model_alone(pkg, orc):
    """the model against hand-computed radii (one record of each type) and, on a two-tile batch, against tree_map_model fed hand-built lists"""
    f32 = np.float32
    p = tam.SizeParams()
    # T_PINE: height 0.5 -> *1.2 = 0.6; height0 = 0.75*0.6 = 0.45; radius = 0.35*(0.45 + 0.03) = 0.168; ao = 1.8*0.168
    h, w = tam.small_tree_size(p, 0.5, 0.1, tam.T_PINE)
    assert h == f32(f32(0.5) * f32(1.2)) and w == f32(0.1)
    r = tam.get_radius(p, tam.T_PINE, h, w)
    assert abs(float(r) - 0.168) < 1e-6 and tam.small_tree_ao_radius(tam.T_PINE, r) == f32(1.8 * float(r))
    # T_SH_PINE: height 0.5 -> *0.8 = 0.4; radius = 0.35*(0.4 + 0.03) = 0.1505; width *= 1.2 and does not count
    h, w = tam.small_tree_size(p, 0.5, 0.1, tam.T_SH_PINE)
    assert w == f32(f32(0.1) * f32(1.2)) and abs(float(tam.get_radius(p, tam.T_SH_PINE, h, w)) - 0.1505) < 1e-6
    # T_PALM: radius = width*1.4, ao = 0.4*radius; the three others: radius = width, ao = 0.5*radius
    h, w = tam.small_tree_size(p, 0.5, 0.1, tam.T_PALM)
    assert h == f32(1.0) and w == f32(f32(0.1) * f32(1.4)) and tam.get_radius(p, tam.T_PALM, h, w) == w and tam.small_tree_ao_radius(tam.T_PALM, w) == f32(0.4 * float(w))
    for typ in (tam.T_DECID, tam.T_TDECID, tam.T_BUSH):
        h, w = tam.small_tree_size(p, 0.5, 0.1, typ)
        assert (h, w) == (f32(0.5), f32(0.1)) and tam.get_radius(p, typ, h, w) == f32(0.1) and tam.small_tree_ao_radius(typ, w) == f32(0.5 * float(w))
    # the scales: height *= 2*3 and back out again in height0, pine_tree_radius_scale and tree_scale in the last product
    q = tam.SizeParams(2.0, 3.0, 1.5, 2.0)
    h, w = tam.small_tree_size(q, 0.5, 0.1, tam.T_PINE)
    assert abs(float(tam.get_radius(q, tam.T_PINE, h, w)) - 0.35 * 1.5 * (0.45 + 0.015)) < 1e-6
    assert tam.calc_tree_size(q) == f32(0.4) and tam.instanced_size(q, tac.INSTS[1]) == (tam.T_SH_PINE, f32(f32(0.7) * f32(0.4)), f32(f32(0.25) * f32(0.4)))
    assert tam.decid_ao_radius(0.3) == f32(0.5 * float(f32(0.3)))
    # two tiles side by side, one deciduous tree each, 5 texels from the shared border with an ao radius of 6.4 texels (rval 7): tile 0 gets its own tree; tile 1
    # its own, then pulls tile 0's (the box cull passes), and pushes its own into tile 0 (xc = 5 <= rval)
    S = 32
    sc = tac.model_scene(orc, pkg, S)
    tiles = [(0, 0), (1, 0)]
    dx = float(sc.DX_VAL)
    decid = np.zeros((2, 1), pkg.DECID_PLACE_DTYPE)
    x0, y0 = f32(float(sc.get_xval(0)) + (S - 5) * dx), f32(float(sc.get_yval(0)) + 10.0 * dx)
    x1, y1 = f32(float(sc.get_xval(S)) + 5 * dx), f32(float(sc.get_yval(0)) + 20.0 * dx)
    decid[0, 0]["pos"], decid[1, 0]["pos"] = (x0, y0, 0), (x1, y1, 0)
    rad = np.full((2, 1), 2 * 6.4 * dx, np.float32)
    ao = tam.decid_ao_radius(rad[0, 0])
    tally = tam.new_tally()
    got = tam.Batch(sc, p, tiles, 16, decid=decid, decid_counts=np.ones(2, np.uint32), decid_radius=rad, tally=tally).run()
    sp = np.array([(x0, y0, ao), (x1, y1, ao), (x1, y1, ao), (x0, y0, ao)], tmm.SPLAT_DTYPE)  # tile 0: own, pushed; tile 1: own, pulled
    want_map, want_upd = tmm.tiles_tree_map(sc, tiles, sp, [0, 2, 4], True)
    assert (got[0] == want_map).all() and (got[1] == want_upd).all() and got[3].tolist() == [2, 2] and (got[2] == rad[:, 0]).all()
    assert (tally["own"], tally["pulled"], tally["pushed"], tally["no_adj_false"]) == (2, 1, 1, 2)


def test_cases_cover_every_branch(pkg, emul, orc):
    """on the model alone: the tally over the case list shows every branch taken; then one case through the library, so that the test needs the feature"""
    total = tac.check_tally(orc, pkg)
    assert total["pushed"] > 20 and total["pulled"] > 20 and total["culled_pull"] > 20
    tac.run_case(pkg, emul, orc, CASES[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases(pkg, emul, orc, case):
    tac.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("name", tac.HOST_FORM)
def test_cases_host_form(pkg, emul, orc, name):
    tac.run_case(pkg, emul, orc, [c for c in CASES if c.name == name][0], host=True)


def test_optional_outputs(pkg, emul, orc):
    """updated, trmax and list_counts may be NULL"""
    case = CASES[1]
    d, want, _ = tac.reference(orc, pkg, case)
    tac.scene(pkg, emul, orc, case.S)
    tac.configure(pkg, emul, case, d["p"])
    n, W = len(d["tiles"]), case.S + 1
    tm = np.zeros((n, W, W, 2), np.uint8)
    rc = emul.lib.terra_tiles_tree_ao_shadows(emul.ctx, np.array(d["tiles"], np.int32).ctypes.data, n, 0, 0, 0, 0, d["pine"].ctypes.data, d["pine_counts"].ctypes.data,
                                              d["pine"].shape[1], d["decid"].ctypes.data, d["decid_counts"].ctypes.data, d["decid"].shape[1], d["decid_radius"].ctypes.data,
                                              None, 0, None, case.list_capacity, tm.ctypes.data, None, None, None)
    assert rc == 0 and (tm == want[0]).all()


def test_refused(pkg, emul, orc):
    tac.run_refused(pkg, emul, orc)


def test_resident_chain(pkg, emul, orc):
    chain.run(pkg, emul, orc, 128, 4)
