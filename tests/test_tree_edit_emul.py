"""The tree brush on the record arrays of a tile batch (terra_tiles_edit_trees[_dev]) through the host emulator -- the driver's one-thread-per-tile forms, the removal
as the literal remove_element loop -- against tests/tree_edit_model.py: records and counts byte for byte, decid_radius, trmax, status and changed exactly, the update
box by value; every case, the host form, the resident chain and the argument checks."""
import numpy as np
import pytest

import tree_edit_cases as tec
import tree_edit_chain as chain
import tree_edit_model as tem

CASES = tec.cases()


def test_model_alone():
    """the model's literal remove_element loop against the closed form the kernel uses (the proof obligation of its ordering), and the model's serially accumulated
    box against a plain min / max, by value"""
    rs = np.random.RandomState(7)
    seen_chain = 0
    for trial in range(4000):
        n = int(rs.randint(0, 71))
        pr = rs.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        keep = [bool(rs.uniform() < pr) for _ in range(n)]
        v = list(range(n))
        changed = tem.remove_loop(v, lambda e: not keep[e])
        assert v == tem.closed_form(keep), (keep, v)
        assert changed == (not all(keep)) and len(v) == sum(keep)
        seen_chain += n >= 3 and not keep[0] and not keep[n - 1] and not keep[n - 2]
    assert seen_chain > 100
    # hand cases: a back element that is itself removed, twice in a row; the last element; everything
    assert tem.closed_form([False, True, True, False, False]) == [2, 1] and tem.closed_form([True, True, False]) == [0, 1] and tem.closed_form([False] * 4) == []
    assert tem.closed_form([False, False, True, True, True, True]) == [5, 4, 2, 3]
    f32 = np.float32
    for trial in range(200):
        k = int(rs.randint(1, 12))
        pts = rs.uniform(-5, 5, (k, 3)).astype(np.float32)
        rad = rs.uniform(0, 2, k).astype(np.float32)
        if trial % 4 == 0:
            pts[0], rad[0] = 0.0, 0.0  # the box is all zeros after the first sphere: the next one restarts it (:3777)
        cube = tem.Cube()
        for p, r in zip(pts, rad):
            tem.update_trees_bcube([f32(c) for c in p], f32(r), cube)
        if trial % 4 == 0:
            pts, rad = pts[1:], rad[1:]
            if k == 1:
                assert cube.is_all_zeros()
                continue
        lo, hi = (pts - rad[:, None]).min(0), (pts + rad[:, None]).max(0)
        assert (cube.values() == np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], np.float32)).all()


def test_cases_cover_every_mechanism(pkg, emul, orc):
    """on the model alone: the tally over the case list shows every mechanism at work; then one case through the library, so that the test needs the feature"""
    total = tec.check_tally(orc, pkg)
    assert total["removed_pine"] > 20 and total["removed_decid"] > 20 and total["appended_pine"] > 5 and total["appended_decid"] > 5, total
    tec.run_case(pkg, emul, orc, CASES[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases(pkg, emul, orc, case):
    tec.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("name", tec.HOST_FORM)
def test_cases_host_form(pkg, emul, orc, name):
    tec.run_case(pkg, emul, orc, [c for c in CASES if c.name == name][0], host=True)


def test_optional_outputs(pkg, emul, orc):
    """update_bcube may be NULL"""
    case = CASES[0]
    d, want, _ = tec.reference(orc, pkg, case)
    tec.configure(pkg, emul, case)
    n = len(d["tiles"])
    pine, pc, decid, dc, rad, trmax = (d[k].copy() for k in ("pine", "pine_counts", "decid", "decid_counts", "decid_radius", "trmax"))
    st, ch = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    import ctypes as C
    rc = emul.lib.terra_tiles_edit_trees(emul.ctx, np.array(d["tiles"], np.int32).ctypes.data, n, 0, 0, 0, 0, (C.c_float * 3)(*d["pos"]), float(d["radius"]), 0, 0, None,
                                         C.addressof(d["stats"]), None, None, pine.ctypes.data, pc.ctypes.data, pine.shape[1], decid.ctypes.data, dc.ctypes.data, decid.shape[1],
                                         rad.ctypes.data, None, 0, trmax.ctypes.data, st.ctypes.data, ch.ctypes.data, None)
    assert rc == 0 and (st == want["status"]).all() and (pc == want["pine_counts"]).all() and (dc == want["decid_counts"]).all()


def test_refused(pkg, emul, orc):
    tec.run_refused(pkg, emul, orc)


def test_refused_device_form(pkg, emul, orc):
    tec.run_refused_dev(pkg, emul, orc)


def test_resident_chain(pkg, emul, orc):
    chain.run(pkg, emul, orc, 128, 4)
