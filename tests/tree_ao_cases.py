"""Cases of the tree AO shadows (terra_tiles_tree_ao_shadows[_dev]) shared by the emulator and GPU tests: every case runs the library and tests/tree_ao_model.py on the
same synthetic placement records and compares every byte of every map plus updated, trmax and list_counts.  The call takes records of any origin, so the cases
build terra_tree_place / terra_decid_place arrays by hand at S = 20, 32 and 64 on 3 x 3 batches (one with a hole, one L-shaped)."""
import ctypes as C

import numpy as np

import orclib
import tree_ao_model as tam
import tree_map_model as tmm

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
GRID = [(x, y) for y in (-4, -3, -2) for x in (2, 3, 4)]          # 3 x 3
HOLE = [xy for xy in GRID if xy != (3, -3)]                       # the centre missing
LSHAPE = [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2)]
INSTS = np.array([(tam.T_PINE, 0.9, 0.2), (tam.T_SH_PINE, 0.7, 0.25), (tam.T_PINE, 1.6, 0.3), (tam.T_PALM, 1.1, 0.45), (tam.T_PALM, 0.8, 1.3)], tam.INST_DTYPE)
NUM_PINE_INSTS, NUM_PALM_INSTS = 3, 2  # the T_SH_PINE instance sits in the pine range


class Case:
    def __init__(self, name, S=32, tiles=GRID, seed=1, flags=None, list_capacity=4096, instanced=False, size=None, by_id=False, per_record=True, num_shared=7,
                 offs=(0, 0, 0, 0), over_capacity=False, small=lambda i: i % 3 == 1, pine=True, decid=True, per_tile=14, order=None, bad_records=False):
        self.__dict__.update(locals())
        del self.self
        self.size = size or {}


def cases():
    out = [
        Case("edges_S20", S=20), Case("edges_S32", S=32, seed=2), Case("edges_S64", S=64, seed=3),
        Case("hole", S=32, tiles=HOLE, seed=4), Case("lshape", S=20, tiles=LSHAPE, seed=5),
        Case("small_next_to_big", S=64, seed=6, small=lambda i: i % 2 == 0),
        Case("all_small", S=32, seed=7, small=lambda i: True),
        Case("flags_each", S=32, seed=8, flags=[0, 1, 2, 3, 4, 5, 6, 7, 0]),
        Case("flags_rotated", S=20, seed=9, flags=[2, 0, 1, 4, 0, 3, 1, 2, 4], small=lambda i: False),
        Case("distant_centre", S=32, seed=10, flags=[0, 0, 0, 0, 4, 0, 0, 0, 0], small=lambda i: False),
        Case("distant_first_last", S=20, seed=11, flags=[4, 0, 1, 0, 2, 0, 0, 0, 4]),
        Case("order_a", S=32, seed=12), Case("order_b", S=32, seed=12, order=[8, 7, 6, 5, 4, 3, 2, 1, 0]), Case("order_c", S=32, seed=12, order=[4, 0, 8, 2, 6, 1, 3, 5, 7]),
        Case("over_capacity", S=20, seed=13, over_capacity=True),
        Case("list_overflow", S=32, seed=14, list_capacity=9, small=lambda i: False),
        Case("list_capacity_0", S=20, seed=14, list_capacity=0),
        Case("instanced", S=32, seed=15, instanced=True),
        Case("instanced_off", S=20, seed=15, instanced=False, bad_records=True),
        Case("scales", S=64, seed=16, size=dict(tree_height_scale=1.3, sm_tree_scale=0.7, pine_tree_radius_scale=1.6, tree_scale=1.5), instanced=True),
        Case("by_id", S=32, seed=17, by_id=True, per_record=False),
        Case("by_id_and_per_record", S=20, seed=17, by_id=True, per_record=True),
        Case("offsets", S=32, seed=18, offs=(5, -3, -7, 11)),
        Case("pine_only", S=20, seed=19, decid=False), Case("decid_only", S=32, seed=20, pine=False),
        Case("no_trees", S=20, seed=21, pine=False, decid=False),
    ]
    return out


HOST_FORM = ("edges_S20", "flags_each", "scales")
SIMPLE_FORM = ("edges_S32", "flags_rotated", "instanced")


def scene(pkg, t, orc, S):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    t.init_scene(cfg)
    return tmm.Scene(orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S)), cfg)


def model_scene(orc, pkg, S):
    return tmm.Scene(orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S)), pkg.make_config(mesh_gen_mode=0, mesh_xy=S))


def build(sc, case, pkg):
    """the case's arrays: dict(tiles, pine, pine_counts, decid, decid_counts, decid_radius, by_id, flags, p)"""
    S, rs = sc.S, np.random.RandomState(case.seed)
    tiles = list(case.tiles)
    n = len(tiles)
    p = tam.SizeParams(**case.size)
    dx = float(sc.DX_VAL)
    dxoff, dyoff, xoff2, yoff2 = case.offs
    pt_off = (float(f32(f32(dxoff + xoff2) * sc.DX_VAL)), float(f32(f32(dyoff + yoff2) * sc.DY_VAL)))

    def pos(tile, fx, fy):  # the record's pos whose pt = pos + pt_off lands on (fractional) texel (fx, fy) of the tile
        x = float(sc.get_xval(tile[0] * S + dxoff)) + fx * dx - pt_off[0]
        y = float(sc.get_yval(tile[1] * S + dyoff)) + fy * float(sc.DY_VAL) - pt_off[1]
        return (f32(x), f32(y), f32(0.1))

    tsize = float(tam.calc_tree_size(p))
    hs = float(p.tree_height_scale) * float(p.sm_tree_scale)
    cap_p, cap_d = case.per_tile + 8, case.per_tile + 40
    pine, decid = np.zeros((n, cap_p), pkg.TREE_PLACE_DTYPE), np.zeros((n, cap_d), pkg.DECID_PLACE_DTYPE)
    pc, dc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    radius = np.zeros((n, cap_d), np.float32)
    by_id = (rs.uniform(0.6, 5.0, case.num_shared) * dx).astype(np.float32)
    for i, tile in enumerate(tiles):
        small = case.small(i)
        rho = (lambda: rs.uniform(0.2, 0.95)) if small else (lambda: rs.uniform(0.4, 3.5))  # get_radius() in texels
        k = 0
        for j in range(case.per_tile if case.pine else 0):
            typ = (j + i) % 6
            fx, fy = rs.uniform(-1.0, S + 1.0, 2) if j % 3 else rs.choice([0.2, 1.0, 2.5, S - 2.5, S - 1.0, S - 0.2], 2)
            r = rho() * dx
            rec = pine[i, k]
            rec["pos"], rec["type"], rec["inst"] = pos(tile, fx, fy), typ, -1
            if tam.is_pine(typ):  # radius = 0.35*prs*(k*height/hs + 0.03/tree_scale)
                kk = 0.75 if typ == tam.T_PINE else 1.0
                h0 = max(r / (0.35 * float(p.pine_tree_radius_scale)) - 0.03 / float(p.tree_scale), 0.004)
                rec["height"], rec["width"] = h0 / (kk * float(tam.HEIGHT_SCALE[typ])), 0.3 * r
            else:
                rec["height"], rec["width"] = 4.0 * r, r / float(tam.WIDTH_SCALE[typ])
            if (case.instanced or case.bad_records) and j % 2:
                rec["inst"], rec["type"] = (j // 2) % len(INSTS), (tam.T_PALM if (j // 2) % len(INSTS) >= NUM_PINE_INSTS else tam.T_PINE)
                rec["height"] = rec["width"] = 0.0
            if case.bad_records and j % 5 == 0:
                rec["inst"], rec["type"] = -1, 6 + j  # no such type
            k += 1
        pc[i] = k
        k = 0
        # the border tests of :769-770 at rval = 3: xc == rval, rval + 1, S - rval, S - rval - 1, the same in y, and the four corners
        edge = []
        if case.decid and not small:
            rv, lo, hi = 3, [3, 4], [S - 3, S - 4]
            mid = 0.5 * S + 0.3
            edge = [(a, mid) for a in lo + hi] + [(mid, a) for a in lo + hi] + [(a, b) for a in (3, S - 3) for b in (3, S - 3)] + [(4, 4), (S - 4, S - 4), (4, S - 3), (S - 3, 4)]
            for fx, fy in edge:
                decid[i, k]["pos"] = pos(tile, fx, fy)
                radius[i, k] = 2.0 * (rv - 1 + 0.4) * dx  # ao radius 2.4 texels: rval 3
                decid[i, k]["tree_id"] = -1
                k += 1
        for j in range(case.per_tile if case.decid else 0):
            fx, fy = rs.uniform(-0.4, S + 0.4, 2)
            decid[i, k]["pos"] = pos(tile, fx, fy)
            decid[i, k]["type"] = j % 5
            radius[i, k] = (rs.uniform(0.3, 1.8) if small else rs.uniform(0.8, 9.0)) * dx
            decid[i, k]["tree_id"] = j % (case.num_shared + 1) - 1 if case.bad_records or j % 7 == 6 else j % case.num_shared
            k += 1
        dc[i] = k
        if small and case.by_id and not case.per_record:
            dc[i] = 0  # (the shared radii are too large for a tile that is to stay below min(DX_VAL, DY_VAL))
    if case.over_capacity:  # a count above its capacity: the first `capacity` records (all of them hold a tree here)
        for i in range(n):
            if i % 2 == 0:
                cap_used = int(pc[i])
                pine[i, cap_used:] = pine[i, :cap_p - cap_used]
                pc[i] = cap_p + 5 + i
            else:
                decid[i, int(dc[i]):] = decid[i, :cap_d - int(dc[i])]
                radius[i, int(dc[i]):] = radius[i, :cap_d - int(dc[i])]
                dc[i] = cap_d + 3
    flags = None if case.flags is None else np.array(case.flags[:n], np.uint8)
    d = dict(tiles=tiles, pine=pine if case.pine else None, pine_counts=pc if case.pine else None, decid=decid if case.decid else None,
             decid_counts=dc if case.decid else None, decid_radius=radius if (case.decid and case.per_record) else None,
             by_id=by_id if (case.decid and case.by_id) else None, flags=flags, p=p)
    if case.order is not None:
        o = list(case.order)
        d["tiles"] = [tiles[i] for i in o]
        for key in ("pine", "pine_counts", "decid", "decid_counts", "decid_radius", "flags"):
            if d[key] is not None:
                d[key] = np.ascontiguousarray(d[key][o])
    return d


def model(sc, case, d, tally=None):
    dxoff, dyoff, xoff2, yoff2 = case.offs
    b = tam.Batch(sc, d["p"], d["tiles"], case.list_capacity, d["pine"], d["pine_counts"], d["decid"], d["decid_counts"], d["decid_radius"], d["by_id"], d["flags"],
                  case.instanced, INSTS, dxoff, dyoff, xoff2, yoff2, tally)
    return b.run()


def configure(pkg, t, case, p):
    t.set_tree_params(pkg.make_tree_params(tree_scale=float(p.tree_scale), instanced=int(case.instanced), num_pine_insts=NUM_PINE_INSTS if case.instanced else 0,
                                           num_palm_insts=NUM_PALM_INSTS if case.instanced else 0))
    t.set_decid_params(pkg.make_decid_params(num_shared_trees=case.num_shared))
    t.set_tree_size_params(pkg.make_tree_size_params(float(p.tree_height_scale), float(p.sm_tree_scale), float(p.pine_tree_radius_scale)))
    t.set_tree_instances(INSTS if case.instanced else np.zeros(0, pkg.TREE_INST_DTYPE))


def compare(what, got, want):
    (gm, gu, gt, gc), (wm, wu, wt, wc) = got, want
    assert (np.asarray(gc, np.uint32) == wc).all(), f"{what}: list_counts {np.asarray(gc).tolist()} != {wc.tolist()}"
    assert (np.asarray(gt, np.float32).view(np.uint32) == wt.view(np.uint32)).all(), f"{what}: trmax {np.asarray(gt).tolist()} != {wt.tolist()}"
    bad = np.argwhere(gm != wm)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ in tiles {sorted(set(bad[:, 0].tolist()))}, first at {bad[0].tolist()}: {gm[tuple(bad[0])]} != {wm[tuple(bad[0])]}"
    assert (np.asarray(gu).astype(bool) == wu).all(), f"{what}: updated {np.asarray(gu).astype(int).tolist()} != {wu.astype(int).tolist()}"


def run_dev(t, case, d):
    """the device form on uploaded arrays"""
    n, S = len(d["tiles"]), t.tile_size
    W = S + 1
    dxoff, dyoff, xoff2, yoff2 = case.offs
    bufs = {}

    def dev(key, a):
        if a is None:
            return None
        bufs[key] = t.alloc(max(a.nbytes, 4)).upload(np.ascontiguousarray(a)) if a.nbytes else t.alloc(4)
        return bufs[key].ptr

    try:
        ptrs = {k: dev(k, d[k]) for k in ("pine", "pine_counts", "decid", "decid_counts", "decid_radius", "by_id", "flags")}
        out = dict(tm=t.alloc(n * W * W * 2), upd=t.alloc(n), trmax=t.alloc(4 * n), lc=t.alloc(4 * n))
        bufs.update(out)
        t.tiles_tree_ao_shadows_dev(d["tiles"], case.list_capacity, out["tm"].ptr, ptrs["pine"], ptrs["pine_counts"], 0 if d["pine"] is None else d["pine"].shape[1],
                                    ptrs["decid"], ptrs["decid_counts"], 0 if d["decid"] is None else d["decid"].shape[1], ptrs["decid_radius"], ptrs["by_id"],
                                    0 if d["by_id"] is None else len(d["by_id"]), ptrs["flags"], out["upd"].ptr, out["trmax"].ptr, out["lc"].ptr, dxoff, dyoff, xoff2, yoff2)
        return (out["tm"].download(np.uint8, (n, W, W, 2)), out["upd"].download(np.uint8, (n,)), out["trmax"].download(np.float32, (n,)),
                out["lc"].download(np.uint32, (n,)))
    finally:
        for b in bufs.values():
            b.free()


def run_host(t, case, d):
    dxoff, dyoff, xoff2, yoff2 = case.offs
    return t.tiles_tree_ao_shadows(d["tiles"], case.list_capacity, d["pine"], d["pine_counts"], d["decid"], d["decid_counts"], d["decid_radius"], d["by_id"], d["flags"],
                                   dxoff, dyoff, xoff2, yoff2)


_WANT = {}  # (case name) -> the model's result: computed once, shared by the tests of a session, never changed


def reference(orc, pkg, case):
    if case.name not in _WANT:
        sc = model_scene(orc, pkg, case.S)
        d = build(sc, case, pkg)
        tally = tam.new_tally()
        _WANT[case.name] = (d, model(sc, case, d, tally), tally)
    return _WANT[case.name]


def run_case(pkg, t, orc, case, host=False):
    d, want, _ = reference(orc, pkg, case)
    scene(pkg, t, orc, case.S)
    configure(pkg, t, case, d["p"])
    got = run_host(t, case, d) if host else run_dev(t, case, d)
    compare(f"{case.name} ({'host' if host else 'device'} form)", got, want)


def check_tally(orc, pkg):
    """every branch the cases are there for is taken at least once over the case list -- on the model alone"""
    total = tam.new_tally()
    maps = {}
    for case in cases():
        _, want, ta = reference(orc, pkg, case)
        maps[case.name] = want[0]
        for k, v in ta.items():
            total[k] = (total[k] | v) if isinstance(v, set) else total[k] + v
    for k in ("own", "pulled", "pushed", "culled_own", "culled_pull", "no_adj_true", "no_adj_false", "instanced", "by_id", "per_record", "dropped", "overflow"):
        assert total[k] > 0, f"no case takes the branch {k!r}: {total}"
    assert total["types"] == set(range(6)) and tam.T_SH_PINE in total["inst_types"] and tam.T_PALM in total["inst_types"], total
    # the same tile set in three batch orders gives three different sets of maps
    a, b, c = (maps[k] for k in ("order_a", "order_b", "order_c"))
    cs = {c_.name: c_ for c_ in cases()}
    ob, oc = cs["order_b"].order, cs["order_c"].order
    assert (a[ob] != b).any() and (a[oc] != c).any()
    return total


def run_refused(pkg, t, orc, dev_form=True):
    """dev_form: also through the device form, on the arrays as they are (the emulator's "device" memory is the host's; on a GPU only the host form runs)"""
    lib, ctx = t.lib, t.ctx
    case = [c for c in cases() if c.name == "by_id_and_per_record"][0]
    d, _, _ = reference(orc, pkg, case)
    n, S = len(d["tiles"]), case.S
    txy = np.array(d["tiles"], np.int32)
    tm, upd, trm, lc = np.zeros((n, S + 1, S + 1, 2), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    base = dict(txy=txy, nn=n, pine=d["pine"], pc=d["pine_counts"], decid=d["decid"], dc=d["decid_counts"], rad=d["decid_radius"], by_id=d["by_id"], tm=tm, fn=None)

    def call(**kw):
        a = dict(base, **kw)
        fn = a["fn"] or lib.terra_tiles_tree_ao_shadows
        nid = 0 if a["by_id"] is None else len(a["by_id"])
        tmp = a["tm"] if isinstance(a["tm"], (int, type(None))) else ptr(a["tm"])
        return fn(ctx, ptr(a["txy"]), a["nn"], 0, 0, 0, 0, ptr(a["pine"]), ptr(a["pc"]), d["pine"].shape[1], ptr(a["decid"]), ptr(a["dc"]), d["decid"].shape[1], ptr(a["rad"]), ptr(a["by_id"]), a.get("nid", nid), None, 64, tmp, ptr(upd), ptr(trm), ptr(lc))

    err = lambda: lib.terra_last_error().decode()  # noqa: E731
    dev = lib.terra_tiles_tree_ao_shadows_dev if dev_form else lib.terra_tiles_tree_ao_shadows
    assert call() == ERR_STATE and call(fn=dev) == ERR_STATE  # before terra_init_scene
    scene(pkg, t, orc, S)
    configure(pkg, t, case, d["p"])
    assert call() == 0, err()
    assert call(fn=dev) == 0, err()
    assert call(txy=None) == ERR_ARG and call(tm=None) == ERR_ARG and call(fn=dev, txy=None) == ERR_ARG and call(fn=dev, tm=None) == ERR_ARG
    assert call(txy=None, tm=None, nn=0) == 0 and call(fn=dev, txy=None, tm=None, nn=0) == 0
    for fn in (None, dev):
        assert call(fn=fn, txy=np.ascontiguousarray(txy[[0, 1, 2, 1, 4, 5, 6, 7, 8]])) == ERR_ARG and "twice" in err()
        # a deciduous group needs radii; the by-id form needs num_shared_trees values
        assert call(fn=fn, rad=None, by_id=None) == ERR_ARG and "radius" in err()
        assert call(fn=fn, rad=None, nid=3) == ERR_ARG and "num_shared_trees" in err()
        assert call(fn=fn, rad=None) == 0
    if dev_form:
        assert call(fn=dev, tm=tm.ctypes.data + 1) == ERR_ARG and "aligned" in err()
    assert call(fn=dev, pine=None) == ERR_ARG and call(fn=dev, decid=None) == ERR_ARG and call(pine=None) == ERR_ARG  # counts without records
    assert call(pc=None, dc=None, rad=None, by_id=None) == 0  # both groups absent
    t.set_decid_params(pkg.make_decid_params(num_shared_trees=0))
    assert call(rad=None, by_id=d["by_id"][:0], nid=0) == ERR_ARG and "num_shared_trees == 0" in err()
    assert call() == 0  # the per-record form does not look at the shared trees
    # instanced: the instance table must hold num_pine_insts + num_palm_insts entries
    t.set_tree_params(pkg.make_tree_params(instanced=1, num_pine_insts=NUM_PINE_INSTS, num_palm_insts=NUM_PALM_INSTS))
    assert call() == ERR_ARG and "instances" in err()
    t.set_tree_instances(INSTS[:4])
    assert call() == ERR_ARG
    t.set_tree_instances(INSTS)
    assert call() == 0 and (t.get_tree_instances() == INSTS).all()
    assert call(pc=None) == 0  # no pine group: the table is not looked at
    # terra_tree_size_params: finite and > 0, or nothing changes
    good = pkg.make_tree_size_params(1.25, 0.5, 2.0)
    t.set_tree_size_params(good)
    for bad in (dict(tree_height_scale=0.0), dict(sm_tree_scale=-1.0), dict(pine_tree_radius_scale=float("nan")), dict(tree_height_scale=float("inf"))):
        assert lib.terra_set_tree_size_params(ctx, C.byref(pkg.make_tree_size_params(**bad))) == ERR_ARG
        g = t.get_tree_size_params()
        assert (g.tree_height_scale, g.sm_tree_scale, g.pine_tree_radius_scale) == (1.25, 0.5, 2.0)
    assert lib.terra_set_tree_size_params(ctx, None) == ERR_ARG and lib.terra_set_tree_instances(ctx, None, 3) == ERR_ARG
    # an unsupported tile size
    t.init_scene(pkg.make_config(mesh_xy=130))
    assert call() == ERR_ARG and call(fn=dev) == ERR_ARG
