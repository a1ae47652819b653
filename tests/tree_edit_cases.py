"""Cases of the tree brush (terra_tiles_edit_trees[_dev]) shared by the emulator and GPU tests: every case runs the library and tests/tree_edit_model.py on the same
hand-built record arrays and compares records and counts byte for byte, decid_radius, trmax, status and changed exactly, and the update box by value.  The batches
are 3 x 3 and L-shaped at S = 20 and 32, the sizes tree_ao_cases uses; the heights and the tile statistics come from the oracle's height field."""
import ctypes as C
import types

import numpy as np

import decid_place_cases as dpc
import decid_place_model as dpm
import orclib
import tree_ao_cases as tac
import tree_ao_model as tam
import tree_edit_model as tem
import tree_map_model as tmm
import tree_place_model as tpm

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
GRID = [(x, y) for y in (-1, 0, 1) for x in (1, 2, 3)]  # from the island's top out over its shore, as tree_ao_chain: both placements make trees here
LSHAPE = [(1, -1), (2, -1), (3, -1), (1, 0), (1, 1)]
TP = dict(tree_mode=3, tree_type_rand_zone=0.02)
INSTS, NUM_PINE_INSTS, NUM_PALM_INSTS = tac.INSTS, tac.NUM_PINE_INSTS, tac.NUM_PALM_INSTS


class Case:
    def __init__(self, name, S=32, tiles=GRID, seed=1, at=(0, 0.8, 0.8), r_cells=0.3, is_square=False, add=False, offs=(0, 0, 0, 0), per_record=True, by_id=True,
                 num_shared=7, instanced=False, bad_records=False, over_capacity=False, cap_slack=(40, 40), gen_flags=None, skip=None, per_tile=24, pine=True, decid=True,
                 exact=False, empty_near=False, rscale=1.0, inside_frac=0.0):
        """at = (tile index, fx, fy): the brush centre as a fraction of that tile; r_cells: the radius as a fraction of a tile"""
        self.__dict__.update(locals())
        del self.self


def cases():
    return [
        Case("remove_round_S32"), Case("remove_square_S32", is_square=True),               # the same records: the corners of the square differ
        Case("remove_round_S20", S=20, seed=2), Case("remove_lshape_S20", S=20, tiles=LSHAPE, seed=3, at=(0, 0.5, 0.5), r_cells=0.45),
        Case("boundary_round", seed=4, exact=True, at=(4, 0.5, 0.5), r_cells=0.125), Case("boundary_square", seed=4, exact=True, at=(4, 0.5, 0.5), r_cells=0.125, is_square=True),
        Case("whole_tile_square", seed=5, at=(4, 0.5, 0.5), r_cells=0.55, is_square=True),  # the centre tile emptied completely
        Case("nothing_there", seed=6, at=(8, 0.5, 0.5), r_cells=0.1, empty_near=True),      # a stroke that changes nothing
        Case("over_capacity", S=20, seed=7, over_capacity=True),
        Case("instanced", seed=8, instanced=True), Case("bad_records", S=20, seed=9, bad_records=True),
        Case("by_id", seed=10, per_record=False), Case("per_record_only", S=20, seed=10, by_id=False),
        Case("offsets", seed=11, offs=(5, -3, -7, 11)), Case("offsets_S20", S=20, seed=12, offs=(-20, 40, 9, -2), is_square=True),
        Case("pine_only", S=20, seed=13, decid=False), Case("decid_only", seed=14, pine=False), Case("no_groups", S=20, seed=15, pine=False, decid=False),
        # groups of 700 records, nearly half of them removed: the kernel's sweeps of 256 records carry M, the tail list and the holes' ranks across 256 and 512
        Case("many_records_round", seed=25, per_tile=700, cap_slack=(8, 40), inside_frac=0.3, at=(4, 0.5, 0.5), r_cells=0.25),
        Case("many_records_square_by_id", seed=26, per_tile=700, cap_slack=(40, 8), inside_frac=0.3, at=(4, 0.3, 0.6), r_cells=0.4, is_square=True, per_record=False),
        Case("many_records_add", seed=27, per_tile=700, cap_slack=(300, 300), inside_frac=0.4, at=(4, 0.5, 0.5), r_cells=0.3, add=True),
        Case("radius_0", seed=16, r_cells=0.0, is_square=True, exact=True, at=(4, 0.5, 0.5)),
        Case("add_round", seed=17, add=True, at=(4, 0.4, 0.6), r_cells=0.4), Case("add_square", seed=18, add=True, at=(4, 0.9, 0.9), r_cells=0.35, is_square=True),
        Case("add_overflow", seed=19, add=True, at=(4, 0.5, 0.5), r_cells=0.6, cap_slack=(3, 2)),
        Case("add_gated", seed=20, add=True, at=(4, 0.95, 0.5), r_cells=0.5, gen_flags=[0, 0, 0, 0, 1, 2, 0, 0, 0], skip=[0, 0, 0, 0, 0, 0, 0, 1, 1]),
        Case("add_by_id_only", seed=21, add=True, at=(4, 0.1, 0.1), r_cells=0.4, per_record=False),
        Case("add_small_radii", seed=24, add=True, at=(4, 0.6, 0.3), r_cells=0.4, rscale=0.02),  # the new records raise trmax
        Case("add_offsets_instanced", seed=22, add=True, at=(4, 0.5, 0.1), r_cells=0.4, offs=(64, -32, -64, 32), instanced=True),
        Case("add_lshape", tiles=LSHAPE, seed=23, add=True, at=(0, 0.9, 0.9), r_cells=0.5),
    ]


HOST_FORM = ("remove_round_S32", "over_capacity", "add_round", "add_gated")
SIMPLE_FORM = ("many_records_round", "remove_square_S32", "remove_lshape_S20", "bad_records", "add_square", "add_overflow")


def configure(pkg, t, case):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape())
    t.set_tree_params(pkg.make_tree_params(instanced=int(case.instanced), num_pine_insts=NUM_PINE_INSTS if case.instanced else 0,
                                           num_palm_insts=NUM_PALM_INSTS if case.instanced else 0, **TP))
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=case.num_shared))
    t.set_tree_size_params(pkg.make_tree_size_params())
    t.set_tree_instances(INSTS if case.instanced else np.zeros(0, pkg.TREE_INST_DTYPE))
    return cfg


def model_scenes(orc, pkg, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    state = orc.init(ocfg)
    tp = dict(TP, instanced=int(case.instanced), num_pine_insts=NUM_PINE_INSTS if case.instanced else 0, num_palm_insts=NUM_PALM_INSTS if case.instanced else 0)
    return tmm.Scene(state, pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S)), tpm.Scene(orc, ocfg, tpm.TreeParams(**tp)), state


def build(orc, pkg, case):
    """the case's inputs: dict(tiles, stats, zvals, trmax, pine, pine_counts, decid, decid_counts, decid_radius, by_id, gen_flags, skip, pos, radius) + the scenes"""
    sc, psc, state = model_scenes(orc, pkg, case)
    S, rs = case.S, np.random.RandomState(case.seed)
    tiles = list(case.tiles)
    n = len(tiles)
    p = tam.SizeParams()
    dx = float(sc.DX_VAL)
    dxoff, dyoff, xoff2, yoff2 = case.offs
    xlate = (float(f32(f32(dxoff + xoff2) * sc.DX_VAL)), float(f32(f32(dyoff + yoff2) * sc.DY_VAL)))
    zvals = dpc.tile_zvals(orc, state, types.SimpleNamespace(S=S, tiles=tiles, synth=None))
    stats = dpc.tile_stats(pkg, zvals, S)
    calc_radius = 0.5 * np.sqrt(2.0) * dx * S
    for i in range(n):
        stats[i].radius = calc_radius * (0.9 if i % 2 else 1.4)  # max(stats.radius, calc_radius() + trmax) takes either side

    def world(tile, fx, fy):  # camera-space position of the (fractional) cell (fx, fy) of a tile
        return float(sc.get_xval(tile[0] * S + dxoff)) + fx * dx, float(sc.get_yval(tile[1] * S + dyoff)) + fy * float(sc.DY_VAL)

    bt, bfx, bfy = case.at
    if case.exact:  # a centre on a cell corner and a radius of whole cells: at S = 32 every sum below is exact
        bfx, bfy = round(bfx * S) / S, round(bfy * S) / S
    wx, wy = world(tiles[bt], bfx * S, bfy * S)
    radius = f32(case.r_cells * S * dx)
    mid_z = [0.5 * (stats[i].mzmin + stats[i].mzmax) for i in range(n)]
    pos = (f32(wx), f32(wy), f32(mid_z[bt]))
    ptx, pty = f32(pos[0] - f32(xlate[0])), f32(pos[1] - f32(xlate[1]))  # pt_pos

    cap_p, cap_d = case.per_tile + case.cap_slack[0], case.per_tile + case.cap_slack[1]
    pine, decid = np.zeros((n, cap_p), pkg.TREE_PLACE_DTYPE), np.zeros((n, cap_d), pkg.DECID_PLACE_DTYPE)
    pc, dc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rad = np.zeros((n, cap_d), np.float32)
    by_id = (rs.uniform(0.3, 2.5, case.num_shared) * dx).astype(np.float32)
    R = float(radius)

    def spots(i, count):
        """record positions (the placement's frame) of tile i: the first and the last four inside the brush where the brush reaches the tile (a chain of pulled-in
        back elements that are removed themselves), the rest anywhere on the tile"""
        out = []
        for j in range(count):
            fx, fy = rs.uniform(0.0, S, 2)
            x, y = world(tiles[i], fx, fy)
            inside = j == 0 or j >= count - 4 or j % 5 == 2 or (case.inside_frac > 0.0 and rs.uniform() < case.inside_frac)
            if inside and not case.empty_near:
                a, rr = rs.uniform(0, 6.283), R * rs.uniform(0.0, 0.95 if j % 2 else 1.35)  # beyond 1: the square's corners, or outside
                x, y = float(pos[0]) + rr * np.cos(a), float(pos[1]) + rr * np.sin(a)
            if case.empty_near and abs(x - float(pos[0])) < 2.5 * R and abs(y - float(pos[1])) < 2.5 * R:
                x += 5.0 * R
            out.append((f32(x - xlate[0]), f32(y - xlate[1]), f32(mid_z[i] + rs.uniform(-0.05, 0.05))))
        if case.exact and i == bt and count >= 8:  # exactly on the edge of the fabs test, in x and in y; and exactly at pt_pos
            out[1] = (f32(ptx + radius), f32(pty), out[1][2])
            out[3] = (f32(ptx), f32(pty - radius), out[3][2])
            out[5] = (f32(ptx), f32(pty), out[5][2])
            out[6] = (f32(ptx + radius), f32(pty + radius), out[6][2])
        return out

    for i in range(n):
        npine = 0 if not case.pine else (5 if i == n - 1 else case.per_tile)
        for j, ps in enumerate(spots(i, npine)):
            typ = (j + i) % 6
            r = rs.uniform(0.3, 2.2) * dx * case.rscale
            rec = pine[i, j]
            rec["pos"], rec["type"], rec["inst"] = ps, typ, -1
            if tam.is_pine(typ):
                kk = 0.75 if typ == tam.T_PINE else 1.0
                rec["height"], rec["width"] = max(r / 0.35 - 0.03, 0.004) / (kk * float(tam.HEIGHT_SCALE[typ])), 0.3 * r
            else:
                rec["height"], rec["width"] = 4.0 * r, r / float(tam.WIDTH_SCALE[typ])
            if (case.instanced or case.bad_records) and j % 2:
                rec["inst"], rec["type"] = (j // 2) % len(INSTS), (tam.T_PALM if (j // 2) % len(INSTS) >= NUM_PINE_INSTS else tam.T_PINE)
                rec["height"] = rec["width"] = 0.0
            if case.bad_records and j % 5 == 0:
                rec["inst"], rec["type"] = -1, 6 + j
            rec["rseed1"], rec["rseed2"], rec["cx"], rec["cy"] = 1000 * i + j, -j, j, i  # every record distinct: a wrong move shows
        pc[i] = npine
        ndec = 0 if not case.decid else (4 if i == n - 1 else case.per_tile)
        for j, ps in enumerate(spots(i, ndec)):
            rec = decid[i, j]
            rec["pos"], rec["zval"], rec["type"] = ps, ps[2], j % 5
            rec["tree_id"] = (j % (case.num_shared + 1) - 1) if (case.bad_records or j % 7 == 6) else j % case.num_shared
            rec["rseed1"], rec["rseed2"], rec["cx"], rec["cy"] = 2000 * i + j, j, j, i
            rad[i, j] = rs.uniform(0.4, 3.0) * dx * case.rscale
            if case.bad_records and j % 6 == 1:
                rad[i, j] = -1.0
        dc[i] = ndec
    if case.over_capacity:  # a count above its capacity: the first `capacity` records, all of them real
        for i in range(n):
            k = int(pc[i])
            if case.pine and k:
                pine[i, k:] = pine[i, :cap_p - k]
                pc[i] = cap_p + 3 + i
            k = int(dc[i])
            if case.decid and k and i % 2 == 0:
                decid[i, k:], rad[i, k:] = decid[i, :cap_d - k], rad[i, :cap_d - k]
                dc[i] = cap_d + 1
    d = dict(tiles=tiles, stats=stats, zvals=zvals, pos=pos, radius=radius, pine=pine if case.pine else None, pine_counts=pc if case.pine else None,
             decid=decid if case.decid else None, decid_counts=dc if case.decid else None, decid_radius=rad if (case.decid and case.per_record) else None,
             by_id=by_id if (case.decid and case.by_id) else None, gen_flags=None if case.gen_flags is None else np.array(case.gen_flags[:n], np.uint8),
             skip=None if case.skip is None else np.array(case.skip[:n], np.uint8), p=p, sc=sc, psc=psc)
    # trmax as terra_tiles_tree_ao_shadows returns it: the largest get_radius() of the tile's records (the precondition of the call)
    trmax = np.zeros(n, np.float32)
    for i in range(n):
        rr = [f32(0.0)]
        if case.pine:
            rr += [tem.pine_tree_radius(p, r, case.instanced, INSTS) for r in pine[i, :min(int(pc[i]), cap_p)]]
        if case.decid:
            rr += [tem.decid_tree_radius(r, rad[i, j] if case.per_record else None, d["by_id"]) for j, r in enumerate(decid[i, :min(int(dc[i]), cap_d)])]
        trmax[i] = max(v for v in rr if v is not None)
    d["trmax"] = trmax
    return d


def model(case, d, tally=None):
    dxoff, dyoff, xoff2, yoff2 = case.offs
    b = tem.Batch(d["sc"], d["psc"], d["p"], dpm.DecidParams(num_trees=400, num_shared_trees=case.num_shared), d["tiles"], d["stats"], d["trmax"], d["pine"],
                  d["pine_counts"], d["decid"], d["decid_counts"], d["decid_radius"], d["by_id"], d["gen_flags"], d["skip"], d["zvals"], case.instanced, INSTS,
                  dxoff, dyoff, xoff2, yoff2, tally)
    return b.run(d["pos"], d["radius"], case.add, case.is_square)


_WANT = {}  # (case name) -> (inputs, the model's result, tally): computed once, shared by the tests of a session, never changed


def reference(orc, pkg, case):
    if case.name not in _WANT:
        d = build(orc, pkg, case)
        tally = tem.new_tally()
        _WANT[case.name] = (d, model(case, d, tally), tally)
    return _WANT[case.name]


def compare(what, case, got, want):
    assert (got["status"] == want["status"]).all(), f"{what}: status {got['status'].tolist()} != {want['status'].tolist()}"
    for key in ("pine", "decid"):
        if want[key].shape[1] == 0 or got.get(key) is None:
            continue
        gc, wc = got[key + "_counts"], want[key + "_counts"]
        assert (gc == wc).all(), f"{what}: {key}_counts {gc.tolist()} != {wc.tolist()}"
        cap = want[key].shape[1]
        for t in range(len(wc)):
            m = min(int(wc[t]), cap)
            g, w = np.ascontiguousarray(got[key][t, :m]), np.ascontiguousarray(want[key][t, :m])
            if want["hit"][t]:
                for k in range(m):
                    assert g[k].tobytes() == w[k].tobytes(), f"{what}: tile {t} {key} record {k} of {m}: got {g[k]} != {w[k]}"
                if key == "decid" and got.get("decid_radius") is not None:
                    gr, wr = got["decid_radius"][t, :m], want["decid_radius"][t, :m]
                    assert (gr.view(np.uint32) == wr.view(np.uint32)).all(), f"{what}: tile {t} decid_radius {gr.tolist()} != {wr.tolist()}"
            else:  # a tile that did not pass both culls is not touched at all
                assert got[key][t].tobytes() == got["in_" + key][t].tobytes(), f"{what}: tile {t} {key} records were touched"
    assert (got["trmax"].view(np.uint32) == want["trmax"].view(np.uint32)).all(), f"{what}: trmax {got['trmax'].tolist()} != {want['trmax'].tolist()}"
    assert (got["changed"].astype(bool) == want["changed"]).all(), f"{what}: changed {got['changed'].astype(int).tolist()} != {want['changed'].astype(int).tolist()}"
    assert (got["box"] == want["box"]).all(), f"{what}: box {got['box'].tolist()} != {want['box'].tolist()}"  # by value: -0 == +0


def run_dev(t, pkg, case, d):
    """the device form on uploaded arrays; nothing but the outputs is read back"""
    n = len(d["tiles"])
    dxoff, dyoff, xoff2, yoff2 = case.offs
    bufs = {}

    def dev(key, a):
        if a is None:
            return None
        a = np.frombuffer(a, np.uint8) if isinstance(a, C.Array) else np.ascontiguousarray(a)
        bufs[key] = t.alloc(max(a.nbytes, 4)).upload(a) if a.nbytes else t.alloc(4)
        return bufs[key].ptr

    try:
        ptrs = {k: dev(k, d[k]) for k in ("pine", "pine_counts", "decid", "decid_counts", "decid_radius", "by_id", "gen_flags", "skip", "stats", "zvals", "trmax")}
        out = dict(st=t.alloc(n), ch=t.alloc(n), box=t.alloc(24))
        bufs.update(out)
        cap_p, cap_d = (0 if d["pine"] is None else d["pine"].shape[1]), (0 if d["decid"] is None else d["decid"].shape[1])
        t.tiles_edit_trees_dev(d["tiles"], ptrs["stats"], d["pos"], d["radius"], case.add, case.is_square, ptrs["trmax"], out["st"].ptr, out["ch"].ptr, ptrs["pine"],
                               ptrs["pine_counts"], cap_p, ptrs["decid"], ptrs["decid_counts"], cap_d, ptrs["decid_radius"], ptrs["by_id"],
                               0 if d["by_id"] is None else len(d["by_id"]), ptrs["skip"], ptrs["zvals"], ptrs["gen_flags"], out["box"].ptr, dxoff, dyoff, xoff2, yoff2)
        got = dict(status=out["st"].download(np.uint8, (n,)), changed=out["ch"].download(np.uint8, (n,)), box=out["box"].download(np.float32, (6,)),
                   trmax=bufs["trmax"].download(np.float32, (n,)))
        if d["pine"] is not None:
            got["pine"] = bufs["pine"].download(np.uint8, (d["pine"].nbytes,)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap_p)
            got["pine_counts"] = bufs["pine_counts"].download(np.uint32, (n,))
        if d["decid"] is not None:
            got["decid"] = bufs["decid"].download(np.uint8, (d["decid"].nbytes,)).view(pkg.DECID_PLACE_DTYPE).reshape(n, cap_d)
            got["decid_counts"] = bufs["decid_counts"].download(np.uint32, (n,))
        if d["decid_radius"] is not None:
            got["decid_radius"] = bufs["decid_radius"].download(np.float32, (n, cap_d))
        return got
    finally:
        for b in bufs.values():
            b.free()


def run_host(t, pkg, case, d):
    dxoff, dyoff, xoff2, yoff2 = case.offs
    cp = lambda a: None if a is None else a.copy()  # noqa: E731
    got = dict(pine=cp(d["pine"]), pine_counts=cp(d["pine_counts"]), decid=cp(d["decid"]), decid_counts=cp(d["decid_counts"]), decid_radius=cp(d["decid_radius"]),
               trmax=d["trmax"].copy())
    got["status"], got["changed"], got["box"] = t.tiles_edit_trees(d["tiles"], d["stats"], d["pos"], d["radius"], case.add, case.is_square, got["trmax"], got["pine"],
                                                                   got["pine_counts"], got["decid"], got["decid_counts"], got["decid_radius"], d["by_id"], d["skip"],
                                                                   d["zvals"], d["gen_flags"], dxoff, dyoff, xoff2, yoff2)
    return got


def run_case(pkg, t, orc, case, host=False):
    d, want, _ = reference(orc, pkg, case)
    configure(pkg, t, case)
    got = run_host(t, pkg, case, d) if host else run_dev(t, pkg, case, d)
    got["in_pine"], got["in_decid"] = d["pine"], d["decid"]
    compare(f"{case.name} ({'host' if host else 'device'} form)", case, got, want)
    return got


MECHANISMS = ("status0", "status1", "status2", "near_only", "hit_unchanged", "removed_pine", "removed_decid", "removed_last", "chain3", "emptied", "boundary_kept",
              "square_only", "over_capacity_in", "append_overflow", "appended_pine", "appended_decid", "instanced", "per_record", "by_id", "dropped_removed", "multi_sweep", "gated_gen",
              "gated_skip", "removed_while_gated", "changed_by_box", "box_zero", "trmax_raised", "radius_by_stats", "radius_by_trmax")


def check_tally(orc, pkg):
    """every mechanism the cases are there for occurs at least once over the case list -- on the model alone"""
    total = tem.new_tally()
    res = {}
    for case in cases():
        _, want, ta = reference(orc, pkg, case)
        res[case.name] = want
        for k, v in ta.items():
            total[k] += v
    for k in MECHANISMS:
        assert total[k] > 0, f"no case shows the mechanism {k!r}: {total}"
    for case in cases():  # each of the many-record cases carries the kernel's running sums across its sweeps
        if case.name.startswith("many_records"):
            assert reference(orc, pkg, case)[2]["multi_sweep"] > 0, case.name
    # a round brush against a square one on the same records: they differ
    a, b = res["remove_round_S32"], res["remove_square_S32"]
    assert (a["pine_counts"] != b["pine_counts"]).any() or (a["decid_counts"] != b["decid_counts"]).any()
    a, b = res["boundary_round"], res["boundary_square"]
    assert (a["pine_counts"] > b["pine_counts"]).any()
    # status 0 next to status 2 in one batch; offsets that are not zero; a stroke that changes nothing
    assert any(0 in r["status"] and 2 in r["status"] for r in res.values())
    z = res["nothing_there"]
    assert not z["box"].any() and not z["changed"].any() and (z["status"] <= 1).all() and (z["status"] == 1).any()
    return total


def run_refused(pkg, t, orc, dev_form=True):
    """dev_form: also through the device form, on the arrays as they are (the emulator's "device" memory is the host's; on a GPU only the host form runs)"""
    lib, ctx = t.lib, t.ctx
    case = [c for c in cases() if c.name == "add_round"][0]
    d, _, _ = reference(orc, pkg, case)
    n = len(d["tiles"])
    txy = np.array(d["tiles"], np.int32)
    ptr = lambda a: None if a is None else (C.addressof(a) if isinstance(a, C.Array) else a.ctypes.data)  # noqa: E731
    st, ch, box = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(6, np.float32)
    base = dict(txy=txy, nn=n, pos=(C.c_float * 3)(*d["pos"]), radius=float(d["radius"]), add=1, stats=d["stats"], zvals=d["zvals"], pc=None, dc=None, rad=None,
                by_id=d["by_id"], st=st, ch=ch, trmax=None, fn=None, pine=None, decid=None)
    live = {}

    def call(**kw):
        a = dict(base, **kw)
        live.clear()
        for k, src in (("pine", "pine"), ("pc", "pine_counts"), ("decid", "decid"), ("dc", "decid_counts"), ("rad", "decid_radius"), ("trmax", "trmax")):
            if k not in kw:  # fresh copies: a call that goes through edits them
                live[k] = d[src].copy()
                a[k] = live[k]
        fn = a["fn"] or lib.terra_tiles_edit_trees
        nid = 0 if a["by_id"] is None else len(a["by_id"])
        pos = a["pos"]
        return fn(ctx, ptr(a["txy"]), a["nn"], 0, 0, 0, 0, pos, a["radius"], a["add"], 0, None, ptr(a["stats"]), ptr(a["zvals"]), None, ptr(a["pine"]), ptr(a["pc"]),
                  d["pine"].shape[1], ptr(a["decid"]), ptr(a["dc"]), d["decid"].shape[1], ptr(a["rad"]), ptr(a["by_id"]), a.get("nid", nid), ptr(a["trmax"]),
                  ptr(a["st"]), ptr(a["ch"]), ptr(box))

    def untouched():
        return all(live[k].tobytes() == d[s].tobytes() for k, s in (("pine", "pine"), ("pc", "pine_counts"), ("decid", "decid"), ("dc", "decid_counts"),
                                                                    ("rad", "decid_radius"), ("trmax", "trmax")) if k in live)

    err = lambda: lib.terra_last_error().decode()  # noqa: E731
    dev = lib.terra_tiles_edit_trees_dev if dev_form else lib.terra_tiles_edit_trees
    assert call() == ERR_STATE and call(fn=dev) == ERR_STATE  # before terra_init_scene
    configure(pkg, t, case)
    assert call() == 0, err()
    assert not untouched()
    assert call(fn=dev) == 0, err()
    for fn in (None, dev):
        for kw in (dict(txy=None), dict(stats=None), dict(st=None), dict(ch=None), dict(trmax=None), dict(pos=None), dict(pine=None), dict(decid=None)):
            assert call(fn=fn, **kw) == ERR_ARG and untouched(), kw
        assert call(fn=fn, txy=None, stats=None, st=None, ch=None, trmax=None, nn=0) == 0
        for r in (-1.0, float("nan"), float("inf")):
            assert call(fn=fn, radius=r) == ERR_ARG and "radius" in err() and untouched()
        # a new deciduous record's radius is known only through the table; the slope test needs the heights
        assert call(fn=fn, by_id=None) == ERR_ARG and "decid_radius_by_id" in err() and untouched()
        assert call(fn=fn, nid=3) == ERR_ARG and "num_shared_trees" in err() and untouched()
        assert call(fn=fn, zvals=None) == ERR_ARG and "zvals" in err() and untouched()
        assert call(fn=fn, add=0, by_id=None, zvals=None) == 0             # removal alone: the per-record radii do
        assert call(fn=fn, add=0, by_id=None, rad=None) == ERR_ARG and "radius" in err() and untouched()
        assert call(fn=fn, add=0, rad=None) == 0
        assert call(fn=fn, pc=None, dc=None, rad=None, by_id=None, zvals=None) == 0  # both groups absent
    if dev_form:
        assert call(fn=dev, trmax=np.zeros(n + 1, np.float32).view(np.uint8)[1:4 * n + 1]) == ERR_ARG and "aligned" in err() and untouched()
    # what the brush placements refuse: XY_MULT_SIZE < 2*ntrees (a density the tile size cannot take)
    t.set_tree_params(pkg.make_tree_params(sm_tree_density=40.0, **TP))
    assert call() == ERR_ARG and "XY_MULT_SIZE" in err() and untouched()
    assert call(add=0) == 0
    t.set_tree_params(pkg.make_tree_params(**TP))
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=0))
    assert call() == ERR_ARG and "num_shared_trees == 0" in err() and untouched()
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=case.num_shared))
    t.set_tree_params(pkg.make_tree_params(instanced=1, num_pine_insts=NUM_PINE_INSTS, num_palm_insts=NUM_PALM_INSTS, **TP))
    assert call() == ERR_ARG and "instances" in err() and untouched()
    # an unsupported tile size
    t.init_scene(pkg.make_config(mesh_xy=130))
    assert call() == ERR_ARG and call(fn=dev) == ERR_ARG and untouched()


def run_refused_dev(pkg, t, orc):
    """the device entry's own refusals on device allocations (what a GPU context can run): nothing a refused call was given is changed"""
    lib, ctx = t.lib, t.ctx
    case = [c for c in cases() if c.name == "add_round"][0]
    d, _, _ = reference(orc, pkg, case)
    n = len(d["tiles"])
    txy = np.array(d["tiles"], np.int32)
    src = dict(pine=d["pine"], pc=d["pine_counts"], decid=d["decid"], dc=d["decid_counts"], rad=d["decid_radius"], trmax=d["trmax"], by_id=d["by_id"], zvals=d["zvals"],
               stats=np.frombuffer(d["stats"], np.uint8))
    bufs = {k: t.alloc(a.nbytes).upload(a) for k, a in src.items()}
    bufs.update(st=t.alloc(n), ch=t.alloc(n), box=t.alloc(24))
    base = dict({k: b.ptr for k, b in bufs.items()}, txy=txy.ctypes.data, nn=n, pos=(C.c_float * 3)(*d["pos"]), radius=float(d["radius"]), add=1, nid=len(d["by_id"]))

    def call(**kw):
        a = dict(base, **kw)
        return lib.terra_tiles_edit_trees_dev(ctx, a["txy"], a["nn"], 0, 0, 0, 0, a["pos"], a["radius"], a["add"], 0, None, a["stats"], a["zvals"], None, a["pine"], a["pc"],
                                              d["pine"].shape[1], a["decid"], a["dc"], d["decid"].shape[1], a["rad"], a["by_id"], a["nid"], a["trmax"], a["st"], a["ch"], a["box"])

    def untouched():
        return all(bufs[k].download(np.uint8, (src[k].nbytes,)).tobytes() == src[k].tobytes() for k in ("pine", "pc", "decid", "dc", "rad", "trmax"))

    err = lambda: lib.terra_last_error().decode()  # noqa: E731
    try:
        assert call() == ERR_STATE  # before terra_init_scene
        configure(pkg, t, case)
        for k in ("txy", "stats", "st", "ch", "trmax", "pos", "pine", "decid"):
            assert call(**{k: None}) == ERR_ARG, k
        assert call(txy=None, stats=None, st=None, ch=None, trmax=None, nn=0) == 0
        assert call(trmax=bufs["trmax"].ptr + 1) == ERR_ARG and "aligned" in err()
        assert call(pine=bufs["pine"].ptr + 2) == ERR_ARG and "aligned" in err()
        for r in (-1.0, float("nan"), float("inf")):
            assert call(radius=r) == ERR_ARG and "radius" in err()
        assert call(by_id=None) == ERR_ARG and "decid_radius_by_id" in err()
        assert call(nid=3) == ERR_ARG and "num_shared_trees" in err()
        assert call(zvals=None) == ERR_ARG and "zvals" in err()
        assert call(add=0, by_id=None, rad=None) == ERR_ARG and "radius" in err()
        t.synchronize()
        assert untouched()
        assert call() == 0, err()
        t.synchronize()
        assert not untouched()
    finally:
        for b in bufs.values():
            b.free()
