"""The resident chain of the tree brush, shared by the emulator and GPU tests: tiles_create_zvals_dev -> both placements -> terra_tiles_tree_ao_shadows_dev (its trmax
feeds the brush) -> one removing stroke -> one adding stroke at another place -> terra_tiles_tree_ao_shadows_dev again -> terra_tiles_shadow_texture_dev, on one
context with nothing read back in between, against the model chain (tree_place_model, decid_place_model, tree_ao_model, tree_edit_model, tree_map_model) run on the
downloaded zvals and stats (which have parity tests of their own)."""
import ctypes as C
import types

import numpy as np

import decid_place_model as dpm
import decid_place_cases as dpc
import orclib
import tree_ao_cases as tac
import tree_ao_chain as tac_chain
import tree_ao_model as tam
import tree_edit_model as tem
import tree_map_model as tmm
import tree_place_model as tpm

TP, DP, LIGHT_FACTOR = tac_chain.TP, tac_chain.DP, tac_chain.LIGHT_FACTOR
_MODEL = {}  # the model chain, computed once per process


def strokes(sc, tiles, S, stats):
    """(pos, radius, add, is_square) of the two strokes: a round removal on the second row, a square addition on the third"""
    def at(i, fx, fy, r):
        x, y = float(sc.get_xval(tiles[i][0] * S)) + fx * S * float(sc.DX_VAL), float(sc.get_yval(tiles[i][1] * S)) + fy * S * float(sc.DY_VAL)
        return (np.float32(x), np.float32(y), np.float32(0.5 * (stats[i].mzmin + stats[i].mzmax))), np.float32(r * S * float(sc.DX_VAL))
    return [at(5, 0.95, 0.5, 0.4) + (False, False), at(9, 0.3, 0.9, 0.3) + (True, True)]


def run(pkg, t, orc, S, side):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(**TP))
    t.set_decid_params(pkg.make_decid_params(**DP))
    t.set_tree_size_params(pkg.make_tree_size_params())
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(1, side + 1)]
    n, W, Z = len(tiles), S + 1, S + 2
    cap_p, cap_d, cap_l = 400, 448, 2048
    by_id = (np.float32(0.06) + np.float32(0.02) * np.arange(DP["num_shared_trees"], dtype=np.float32)).astype(np.float32)
    prec, drec = pkg.TREE_PLACE_DTYPE.itemsize, pkg.DECID_PLACE_DTYPE.itemsize
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * cap_p * prec, pc=n * 4, dt=n * cap_d * drec, dc=n * 4, id=by_id.nbytes, tm=n * W * W * 2,
                 upd=n, trm=n * 4, lc=n * 4, sh=n * W * W * 4, s1=n, c1=n, b1=24, s2=n, c2=n, b2=24)
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    sc = tmm.Scene(orc.init(ocfg), cfg)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    try:
        bufs["id"].upload(by_id)
        bufs["pt"].upload(np.zeros(sizes["pt"], np.uint8)); bufs["dt"].upload(np.zeros(sizes["dt"], np.uint8))
        groups = (bufs["pt"].ptr, bufs["pc"].ptr, cap_p, bufs["dt"].ptr, bufs["dc"].ptr, cap_d, None, bufs["id"].ptr, len(by_id))
        # the chain: nothing is read back between its steps (the strokes' positions need the tiles' height range: taken from the model's side below)
        t.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)
        t.tiles_place_trees_dev(tiles, cap_p, bufs["pt"].ptr, bufs["pc"].ptr, 0, 0, None, bufs["st"].ptr)
        t.tiles_place_decid_trees_dev(tiles, cap_d, bufs["dt"].ptr, bufs["dc"].ptr, 0, 0, None, bufs["st"].ptr, bufs["z"].ptr)
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, bufs["tm"].ptr, *groups, None, bufs["upd"].ptr, bufs["trm"].ptr, bufs["lc"].ptr)
        zr = _zranges(orc, sc, tiles, S)
        st_list = strokes(sc, tiles, S, zr)
        for (pos, radius, add, sq), (s, c, b) in zip(st_list, (("s1", "c1", "b1"), ("s2", "c2", "b2"))):
            t.tiles_edit_trees_dev(tiles, bufs["st"].ptr, pos, radius, add, sq, bufs["trm"].ptr, bufs[s].ptr, bufs[c].ptr, *groups, None, bufs["z"].ptr, None, bufs[b].ptr)
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, bufs["tm"].ptr, *groups, None, bufs["upd"].ptr, bufs["trm"].ptr, bufs["lc"].ptr)
        t.tiles_shadow_texture_dev(n, LIGHT_FACTOR, bufs["sh"].ptr, False, None, None, None, bufs["tm"].ptr)
        zvals = bufs["z"].download(np.float32, (n, Z, Z))
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
        pine = bufs["pt"].download(np.uint8, (sizes["pt"],)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap_p)
        pc = bufs["pc"].download(np.uint32, (n,))
        decid = bufs["dt"].download(np.uint8, (sizes["dt"],)).view(pkg.DECID_PLACE_DTYPE).reshape(n, cap_d)
        dc = bufs["dc"].download(np.uint32, (n,))
        got_ao = (bufs["tm"].download(np.uint8, (n, W, W, 2)), bufs["upd"].download(np.uint8, (n,)), bufs["trm"].download(np.float32, (n,)), bufs["lc"].download(np.uint32, (n,)))
        got_sh = bufs["sh"].download(np.uint8, (n, W, W, 4))
        got_strokes = [dict(status=bufs[s].download(np.uint8, (n,)), changed=bufs[c].download(np.uint8, (n,)), box=bufs[b].download(np.float32, (6,)))
                       for s, c, b in (("s1", "c1", "b1"), ("s2", "c2", "b2"))]
    finally:
        for b in bufs.values():
            b.free()
    key = (S, side)
    if key not in _MODEL:
        orc.init(ocfg)
        psc = tpm.Scene(orc, ocfg, tpm.TreeParams(**TP))
        want_p = tpm.place(psc, tiles, 0, 0, None, [(stats[i].mzmin, stats[i].mzmax) for i in range(n)])
        want_d = dpm.place(psc, dpm.DecidParams(**DP), tiles, 0, 0, None, stats, zvals)
        assert max(len(w) for w in want_p) <= cap_p and max(len(w) for w in want_d) <= cap_d
        mp, md = np.zeros((n, cap_p), tpm.PLACE_DTYPE), np.zeros((n, cap_d), dpm.PLACE_DTYPE)
        for i in range(n):
            if want_p[i]:
                mp[i, :len(want_p[i])] = np.array(want_p[i], tpm.PLACE_DTYPE)
            if want_d[i]:
                md[i, :len(want_d[i])] = np.array(want_d[i], dpm.PLACE_DTYPE)
        mpc, mdc = np.array([len(w) for w in want_p], np.uint32), np.array([len(w) for w in want_d], np.uint32)
        trmax = tam.Batch(sc, tam.SizeParams(), tiles, cap_l, mp, mpc, md, mdc, None, by_id).run()[2]
        res, tallies = [], []
        for pos, radius, add, sq in st_list:
            tally = tem.new_tally()
            r = tem.Batch(sc, psc, tam.SizeParams(), dpm.DecidParams(**DP), tiles, stats, trmax, mp, mpc, md, mdc, None, by_id, zvals=zvals, tally=tally).run(pos, radius, add, sq)
            mp, mpc, md, mdc, trmax = r["pine"], r["pine_counts"], r["decid"], r["decid_counts"], r["trmax"]
            res.append(r); tallies.append(tally)
        want_ao = tam.Batch(sc, tam.SizeParams(), tiles, cap_l, mp, mpc, md, mdc, None, by_id).run()
        _MODEL[key] = (res, tallies, want_ao, tmm.shadow_texture(S, LIGHT_FACTOR, 0, None, None, None, want_ao[0]))
    res, tallies, want_ao, want_sh = _MODEL[key]
    # both strokes changed records of both groups
    assert tallies[0]["removed_pine"] > 0 and tallies[0]["removed_decid"] > 0 and tallies[1]["appended_pine"] > 0 and tallies[1]["appended_decid"] > 0, tallies
    assert tallies[0]["status0"] > 0 and tallies[0]["status2"] > 1
    for k, (g, w) in enumerate(zip(got_strokes, res)):
        assert (g["status"] == w["status"]).all() and (g["changed"].astype(bool) == w["changed"]).all() and (g["box"] == w["box"]).all(), (k, g, w["status"], w["changed"], w["box"])
    final = res[-1]
    hit = [a or b for a, b in zip(res[0]["hit"], res[1]["hit"])]
    for key2, g, gc in (("pine", pine, pc), ("decid", decid, dc)):
        assert (gc == final[key2 + "_counts"]).all(), (key2, gc.tolist(), final[key2 + "_counts"].tolist())
        for i in range(n):
            m = int(gc[i])
            assert np.ascontiguousarray(g[i, :m]).tobytes() == np.ascontiguousarray(final[key2][i, :m]).tobytes(), f"chain: tile {i} {key2} records differ (hit: {hit[i]})"
    tac.compare(f"chain S={S}, after the strokes", got_ao, want_ao)
    bad = np.argwhere(got_sh != want_sh)
    assert len(bad) == 0, f"shadow texture: {len(bad)} bytes differ, first at {bad[0].tolist()}"
    assert (want_sh[..., 1] != 255).any()
    return tallies


def _zranges(orc, sc, tiles, S):
    """(mzmin, mzmax) per tile from the oracle's height field, for the strokes' z alone (any z inside the range does)"""
    zv = dpc.tile_zvals(orc, orc.state(), types.SimpleNamespace(S=S, tiles=tiles, synth=None))
    return [types.SimpleNamespace(mzmin=float(z.min()), mzmax=float(z.max())) for z in zv]
