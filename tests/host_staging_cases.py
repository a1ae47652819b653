"""Cases of the host entry points' staging (terra_stage.hpp) shared by test_host_staging_emul.py (the host emulator) and test_gpu_host_staging.py (HIP on the
MI355X): every host-pointer entry point that has a `_dev` twin is called through the C ABI itself, so that an optional array can really be absent and an output
array can be pre-filled with a byte pattern.

A case is a list of C arguments in which every array is an Arr: the host form gets the arrays as they are, the device form gets device copies the test uploads
itself (pattern-filled outputs included) and downloads again.  What the two forms leave in every output must be the same bytes; what a call has no business
writing keeps the pattern.  The inputs come from the library's own host calls (tiles_create_zvals, tiles_create_weights, the placements), once per tile size and
batch, and are never changed."""
import ctypes as C

import numpy as np

PATTERN = 0xA5
TILES16 = [(0, 0), (-1, 2), (-2, -1), (1, -2)]  # at S = 16 the first two have pine / palm trees (sm_tree_density 0.1, tree_mode 2), three have deciduous trees, all have scenery
TILES128 = [(0, 0), (1, 0), (0, 1), (1, 1)]
OPTS = ("all", "none", "mixed")
ENTRIES = ("grass_brush", "line_intersect", "tree_map", "shadow_texture", "tree_weights", "place_trees", "place_decid_trees", "place_scenery", "tree_ao", "tree_brush")
PLACEMENTS = ("place_trees", "place_decid_trees", "place_scenery")
NUM_SHARED = 7
PINE_CAP, DECID_CAP = 4, 6  # of the record arrays the tree AO and the tree brush read


class Arr:
    """one array argument: kind "in" (read), "out" (written: starts as the pattern), "inout" (starts as data, handed back), "host" (a host pointer in both forms)"""

    def __init__(self, name, kind, data):
        self.name, self.kind = name, kind
        self.data = None if data is None else np.ascontiguousarray(data)


class Count:
    """a tile or line count: what the empty batch sets to 0"""

    def __init__(self, v):
        self.v = int(v)


def tile_size(entry):
    return 128 if entry in ("grass_brush", "tree_weights") else 16  # (the grass brush and the tree weights are still require_tile_128)


def configure(pkg, t, S, pine=False):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    t.set_landscape(pkg.make_landscape())
    t.set_tree_params(pkg.make_tree_params(tree_mode=2 if pine else 3, sm_tree_density=0.1))
    t.set_decid_params(pkg.make_decid_params(num_trees=60, num_shared_trees=NUM_SHARED))
    t.set_scenery_params(pkg.make_scenery_params(2))
    t.set_tree_size_params(pkg.make_tree_size_params())


_INPUTS = {}  # (S, n) -> dict of input arrays: computed once, shared, never changed


def inputs(pkg, t, S, n):
    key = (S, n)
    if key in _INPUTS:
        return _INPUTS[key]
    tiles = (TILES128 if S == 128 else TILES16)[:n]
    rs = np.random.RandomState(100 * S + n)
    configure(pkg, t, S)
    z, stats, _, _ = t.tiles_create_zvals(tiles, 0, normals=False)
    d = dict(tiles=tiles, txy=np.array(tiles, np.int32), z=z, stats=np.frombuffer(stats, np.uint8).copy(), dx=8.0 / S)
    W, Z = S + 1, S + 2
    d["tree_map"] = rs.randint(0, 256, (n, W, W, 2)).astype(np.uint8)
    if S == 128:
        d["w"], d["gb"], _ = t.tiles_create_weights(tiles, z)
    else:
        d["sun"], d["moon"] = rs.randint(0, 256, (n, Z, Z)).astype(np.uint8), rs.randint(0, 256, (n, Z, Z)).astype(np.uint8)
        d["ao"] = rs.randint(0, 256, (n, W, W)).astype(np.uint8)
        # vertical lines through terrain points, four a tile
        ln = []
        for i, (tx, ty) in enumerate(tiles):
            for ix, iy in ((2, 3), (9, 5), (13, 12), (5, 14)):
                x, y, zz = -4.0 + d["dx"] * (tx * S + ix), -4.0 + d["dx"] * (ty * S + iy), float(z[i, iy, ix])
                ln.append([[x, y, zz + 5.0], [x, y, zz - 5.0]])
        d["lines"] = np.array(ln, np.float32)
        d["line_tile"] = np.array([(k // 4) if k % 3 else -1 for k in range(len(ln))], np.int32)
        # splats of a few texels' radius around every tile, behind three unused records (h_first[0] != 0: the host form uploads a slice)
        sp = np.zeros(3 + 5 * n, pkg.TREE_SPLAT_DTYPE)
        sp.view(np.float32)[:9] = np.nan
        for i, (tx, ty) in enumerate(tiles):
            for k in range(5):
                sp[3 + 5 * i + k] = (-4.0 + d["dx"] * (tx * S + rs.uniform(0, S)), -4.0 + d["dx"] * (ty * S + rs.uniform(0, S)), d["dx"] * rs.uniform(1.2, 4.0))
        d["splats"], d["first"] = sp, (3 + 5 * np.arange(n + 1)).astype(np.uint32)
        # the record arrays of the tree AO and the tree brush: the placements' own output
        configure(pkg, t, S, pine=True)
        d["pine"], d["pine_counts"] = t.tiles_place_trees(tiles, PINE_CAP)
        configure(pkg, t, S)
        st = (pkg.TileStats * n).from_buffer_copy(d["stats"].tobytes())
        d["decid"], d["decid_counts"] = t.tiles_place_decid_trees(tiles, DECID_CAP, stats=st, zvals=z)
        d["decid_radius"] = (rs.uniform(0.4, 3.0, (n, DECID_CAP)) * d["dx"]).astype(np.float32)
        d["by_id"] = (rs.uniform(0.3, 2.5, NUM_SHARED) * d["dx"]).astype(np.float32)
        _, _, d["trmax"], _ = t.tiles_tree_ao_shadows(tiles, 64, d["pine"], d["pine_counts"], d["decid"], d["decid_counts"], d["decid_radius"])
    d["distant"] = np.array([0, 0, 1, 0][:n], np.uint8)  # (tile 2 of a batch of four: the two-tile batches keep both tiles live)
    d["skip"] = np.array([0, 0, 1, 0][:n], np.uint8)
    _INPUTS[key] = d
    return d


def case(pkg, t, entry, n, opt):
    """-> (host function, device function, the arguments behind ctx, pine: the scene wants the pine / palm settings)"""
    S = tile_size(entry)
    d = inputs(pkg, t, S, n)
    has = lambda k: opt == "all" or (opt == "mixed" and k % 2 == 0)  # noqa: E731  (mixed: every other optional array of the layout, the first present)
    A, N = Arr, Count(n)
    txy = A("txy", "host", d["txy"])
    lib = t.lib
    W = S + 1
    u8 = lambda name, *shape: A(name, "out", np.zeros(shape, np.uint8))  # noqa: E731
    opt_in = lambda k, name: A(name, "in", d[name]) if has(k) else None  # noqa: E731
    if entry == "grass_brush":  # a stroke across the edge of the first two tiles: both are updated
        brush = pkg.make_grass_brush((-4.0 + d["dx"] * 128, -4.0 + d["dx"] * 60, float(d["z"][1][60, 0])), 7.5 * d["dx"], 1, 1, 0.08)
        args = [txy, N, 0, 0, A("z", "in", d["z"]), A("stats", "in", d["stats"]), opt_in(0, "distant"), C.byref(brush), A("w", "inout", d["w"]), A("gb", "inout", d["gb"]),
                u8("updated", n), A("ranges", "out", np.zeros((n, 4), np.uint32)) if has(1) else None]
        return lib.terra_tiles_edit_grass, lib.terra_tiles_edit_grass_dev, args, False
    if entry == "line_intersect":
        nl = len(d["lines"])
        args = [txy, N, 0, 0, A("z", "in", d["z"]), A("stats", "in", d["stats"]), opt_in(0, "distant"), A("lines", "in", d["lines"]), opt_in(1, "line_tile"), Count(nl),
                u8("hits", nl, 32)]
        return lib.terra_tiles_line_intersect, lib.terra_tiles_line_intersect_dev, args, False
    if entry == "tree_map":  # all: continues a held map (the map is uploaded); else: reset
        reset = 0 if opt == "all" else 1
        args = [txy, N, 0, 0, opt_in(0, "distant"), A("splats", "in", d["splats"]), A("first", "host", d["first"]), reset,
                A("tree_map", "inout", d["tree_map"]) if not reset else u8("tree_map", n, W, W, 2), u8("updated", n) if has(1) else None]
        return lib.terra_tiles_tree_map, lib.terra_tiles_tree_map_dev, args, False
    if entry == "shadow_texture":
        # all: both lights up; mixed: the sun alone (light_factor 1), its mask and the ao; none: no mesh shadows, so no mask is read
        args = [N, opt_in(0, "sun"), opt_in(1, "moon"), opt_in(2, "ao"), opt_in(3, "tree_map"), C.c_float(0.5 if opt == "all" else 1.0), int(opt != "none"), u8("shadow", n, W, W, 4)]
        return lib.terra_tiles_shadow_texture, lib.terra_tiles_shadow_texture_dev, args, False
    if entry == "tree_weights":
        args = [N, A("w", "in", d["w"]), opt_in(0, "tree_map"), u8("weights", n, 129, 129, 4)]
        return lib.terra_tiles_tree_weights, lib.terra_tiles_tree_weights_dev, args, False
    cnt = lambda name: A(name, "out", np.zeros(n, np.uint32))  # noqa: E731
    if entry == "place_trees":
        args = [txy, N, 0, 0, opt_in(0, "skip"), opt_in(1, "stats"), 1, u8("trees", n, 1, 40), cnt("counts")]
        return lib.terra_tiles_place_trees, lib.terra_tiles_place_trees_dev, args, True
    if entry == "place_decid_trees":  # (stats need zvals: the mixed pick is skip and zvals)
        args = [txy, N, 0, 0, opt_in(0, "skip"), opt_in(1, "stats"), A("z", "in", d["z"]) if opt != "none" else None, 1, u8("trees", n, 1, 36), cnt("counts")]
        return lib.terra_tiles_place_decid_trees, lib.terra_tiles_place_decid_trees_dev, args, False
    if entry == "place_scenery":
        args = [txy, N, 0, 0, opt_in(0, "skip"), 1, u8("objs", n, 1, 72), cnt("counts"), A("kinds", "out", np.zeros((n, 9), np.uint32)) if has(1) else None]
        return lib.terra_tiles_place_scenery, lib.terra_tiles_place_scenery_dev, args, False
    decid = opt != "none"  # none: the pine / palm group alone, nothing else that is optional
    rad, by_id = decid and opt == "all", decid  # mixed: per-record radii absent, by-id radii present
    if entry == "tree_ao":
        args = [txy, N, 0, 0, 0, 0, A("pine", "in", d["pine"]), A("pine_counts", "in", d["pine_counts"]), PINE_CAP,
                A("decid", "in", d["decid"]) if decid else None, A("decid_counts", "in", d["decid_counts"]) if decid else None, DECID_CAP if decid else 0,
                A("decid_radius", "in", d["decid_radius"]) if rad else None, A("by_id", "in", d["by_id"]) if by_id else None, NUM_SHARED if by_id else 0,
                A("flags", "in", np.zeros(n, np.uint8)) if has(0) else None, 64, u8("tree_map", n, W, W, 2), u8("updated", n) if has(1) else None,
                A("trmax", "out", np.zeros(n, np.float32)) if has(2) else None, cnt("list_counts") if has(3) else None]
        return lib.terra_tiles_tree_ao_shadows, lib.terra_tiles_tree_ao_shadows_dev, args, False
    assert entry == "tree_brush"  # all, mixed: a stroke that adds trees over the first two tiles; none: one that removes pines (mixed: skip present, gen_flags absent)
    tx, ty = d["tiles"][0]
    pos = (C.c_float * 3)(-4.0 + d["dx"] * (tx * S + 0.9 * S), -4.0 + d["dx"] * (ty * S + 0.5 * S), float(d["z"][0][S // 2, S // 2]))
    args = [txy, N, 0, 0, 0, 0, pos, C.c_float(1.5 * S * d["dx"]), 1 if decid else 0, 0, opt_in(0, "skip"), A("stats", "in", d["stats"]), A("z", "in", d["z"]) if decid else None,
            A("gen_flags", "in", np.zeros(n, np.uint8)) if has(1) else None, A("pine", "inout", d["pine"]), A("pine_counts", "inout", d["pine_counts"]), PINE_CAP,
            A("decid", "inout", d["decid"]) if decid else None, A("decid_counts", "inout", d["decid_counts"]) if decid else None, DECID_CAP if decid else 0,
            A("decid_radius", "inout", d["decid_radius"]) if rad else None, A("by_id", "in", d["by_id"]) if by_id else None, NUM_SHARED if by_id else 0,
            A("trmax", "inout", d["trmax"]), u8("status", n), u8("changed", n), A("box", "out", np.zeros(6, np.float32)) if has(2) else None]
    return lib.terra_tiles_edit_trees, lib.terra_tiles_edit_trees_dev, args, False


def _start(a):
    """the bytes an array holds before the call"""
    return np.full(a.data.nbytes, PATTERN, np.uint8) if a.kind == "out" else a.data.view(np.uint8).reshape(-1).copy()


def run(pkg, t, entry, n, opt, form, empty=False):
    """one call -> {name: the bytes of every out / inout array afterwards}; empty: the same arrays with every count 0"""
    fn_host, fn_dev, args, pine = case(pkg, t, entry, n, opt)
    configure(pkg, t, tile_size(entry), pine)
    keep, bufs, out, cargs = [], {}, {}, []
    try:
        for a in args:
            if isinstance(a, Count):
                cargs.append(0 if empty else a.v)
            elif not isinstance(a, Arr):
                cargs.append(a)
            elif a.kind == "host":
                keep.append(a.data)
                cargs.append(a.data.ctypes.data)
            elif form == "host":
                h = _start(a) if a.kind != "in" else a.data
                keep.append(h)
                if a.kind != "in":
                    out[a.name] = h
                cargs.append(h.ctypes.data if h.nbytes else None)
            else:
                bufs[a.name] = t.alloc(max(a.data.nbytes, 4)).upload(_start(a))
                cargs.append(bufs[a.name].ptr)
        rc = (fn_host if form == "host" else fn_dev)(t.ctx, *cargs)
        assert rc == 0, f"{entry} n={n} {opt} ({form} form): {t.lib.terra_last_error().decode()}"
        for a in args:
            if isinstance(a, Arr) and a.kind in ("out", "inout") and form != "host":
                out[a.name] = bufs[a.name].download(np.uint8, (a.data.nbytes,))
    finally:
        for b in bufs.values():
            b.free()
    return out


def counted(entry, out):
    """of a placement: (records [n, 1, record bytes], counts [n])"""
    rec = {"place_trees": ("trees", 40), "place_decid_trees": ("trees", 36), "place_scenery": ("objs", 72)}[entry]
    counts = out["counts"].view(np.uint32)
    return out[rec[0]].reshape(len(counts), 1, rec[1]), counts


def check_not_trivial(entry, n, opt, out):
    """the call did something: the comparison of the two forms is not one of untouched buffers"""
    what = f"{entry} n={n} {opt}"
    if entry in PLACEMENTS:  # records in two tiles at the least, and a tile with more than the capacity of 1 (asserted on the emulator: the models' tiles and settings)
        _, counts = counted(entry, out)
        assert (counts >= 1).sum() >= 2 and (counts > 1).any(), f"{what}: counts {counts.tolist()}"
    elif entry == "grass_brush":
        assert out["updated"][:2].all(), what
    elif entry == "line_intersect":
        assert (out["hits"] != PATTERN).any(), what
    elif entry in ("tree_map", "tree_ao"):
        assert (out["tree_map"] != 255).any() and (out["tree_map"] != PATTERN).any(), what
    elif entry == "tree_brush":
        assert out["changed"].any() and (out["status"] == 2).any(), f"{what}: status {out['status'].tolist()} changed {out['changed'].tolist()}"
    else:
        assert (out[{"shadow_texture": "shadow", "tree_weights": "weights"}[entry]] != PATTERN).any(), what


def check_padding(entry, opt, out):
    """host form: records past min(count, capacity) keep the pattern"""
    if entry not in PLACEMENTS:
        return
    recs, counts = counted(entry, out)
    for i, c in enumerate(counts):
        assert (recs[i, min(int(c), 1):] == PATTERN).all(), f"{entry}: tile {i}: records past the count were written"
    if entry != "place_scenery" or opt != "none":  # (every tile has scenery: only a skipped one has none)
        assert (counts == 0).any(), f"{entry}: no tile without a record: counts {counts.tolist()}"  # (its whole slot keeps the pattern)


def run_forms(pkg, t, entry, opt):
    n = 2 if tile_size(entry) == 128 else 4
    host, dev = run(pkg, t, entry, n, opt, "host"), run(pkg, t, entry, n, opt, "dev")
    assert sorted(host) == sorted(dev)
    for k in host:
        bad = np.flatnonzero(host[k] != dev[k])
        assert len(bad) == 0, f"{entry} {opt}: {k}: {len(bad)} bytes differ between the host and the device form, first at {bad[0]}: {host[k][bad[0]]} != {dev[k][bad[0]]}"
    check_not_trivial(entry, n, opt, host)
    check_padding(entry, opt, host)


def run_regrowth(pkg, t, entry):
    """n = 2, then 4, then 2 on one context: the scratch is released and regrown in between, the first and the third result are the same"""
    res = []
    for n in (2, 4, 2):
        res.append(run(pkg, t, entry, n, "all", "host"))
        t.release_scratch()
    for k in res[0]:
        assert res[0][k].tobytes() == res[2][k].tobytes(), f"{entry}: {k} differs between the first and the third call"
    assert any(len(res[1][k]) > len(res[0][k]) for k in res[0])


def run_empty(pkg, t, entry):
    out = run(pkg, t, entry, 2, "all", "host", empty=True)
    _, _, args, _ = case(pkg, t, entry, 2, "all")
    for a in args:
        if isinstance(a, Arr) and a.kind in ("out", "inout"):
            assert out[a.name].tobytes() == _start(a).tobytes(), f"{entry}: an empty batch wrote {a.name}"
