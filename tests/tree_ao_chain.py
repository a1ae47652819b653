"""The resident chain of the tree AO shadows, shared by the emulator and GPU tests: tiles_create_zvals_dev -> both placements -> terra_tiles_tree_ao_shadows_dev ->
terra_tiles_shadow_texture_dev and terra_tiles_tree_weights_dev on one context with nothing read back in between, against the model chain (tree_place_model,
decid_place_model, tree_ao_model, tree_map_model) run on the downloaded zvals, stats and mesh weights (which have parity tests of their own)."""
import ctypes as C

import numpy as np

import decid_place_cases as dpc
import decid_place_model as dpm
import orclib
import tree_ao_cases as tac
import tree_ao_model as tam
import tree_map_model as tmm
import tree_place_cases as tpc
import tree_place_model as tpm

TP = dict(tree_mode=3, tree_type_rand_zone=0.02)
DP = dict(num_trees=400, num_shared_trees=16)
LIGHT_FACTOR = 0.7


def run(pkg, t, orc, S, side):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(**TP))
    t.set_decid_params(pkg.make_decid_params(**DP))
    t.set_tree_size_params(pkg.make_tree_size_params())
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(1, side + 1)]  # from the island's top out over its shore: both kinds of tree
    n, W, Z = len(tiles), S + 1, S + 2
    cap_p, cap_d, cap_l = 320, 384, 2048
    by_id = (np.float32(0.06) + np.float32(0.02) * np.arange(DP["num_shared_trees"], dtype=np.float32)).astype(np.float32)  # sphere_radius of the shared trees
    flags = np.zeros(n, np.uint8)
    flags[n - 2] = tam.DISTANT
    prec, drec = pkg.TREE_PLACE_DTYPE.itemsize, pkg.DECID_PLACE_DTYPE.itemsize
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * cap_p * prec, pc=n * 4, dt=n * cap_d * drec, dc=n * 4, id=by_id.nbytes, fl=n, tm=n * W * W * 2,
                 upd=n, trm=n * 4, lc=n * 4, sh=n * W * W * 4, mw=n * W * W * 4, gb=n * 32 * 32 * 12, w=n * W * W * 4)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    try:
        bufs["id"].upload(by_id); bufs["fl"].upload(flags)
        bufs["pt"].upload(np.zeros(sizes["pt"], np.uint8)); bufs["dt"].upload(np.zeros(sizes["dt"], np.uint8))
        # the chain: nothing is read back between its steps
        t.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr, bufs["st"].ptr)
        t.tiles_place_trees_dev(tiles, cap_p, bufs["pt"].ptr, bufs["pc"].ptr, 0, 0, None, bufs["st"].ptr)
        t.tiles_place_decid_trees_dev(tiles, cap_d, bufs["dt"].ptr, bufs["dc"].ptr, 0, 0, None, bufs["st"].ptr, bufs["z"].ptr)
        t.tiles_tree_ao_shadows_dev(tiles, cap_l, bufs["tm"].ptr, bufs["pt"].ptr, bufs["pc"].ptr, cap_p, bufs["dt"].ptr, bufs["dc"].ptr, cap_d, None, bufs["id"].ptr, len(by_id),
                                    bufs["fl"].ptr, bufs["upd"].ptr, bufs["trm"].ptr, bufs["lc"].ptr)
        t.tiles_shadow_texture_dev(n, LIGHT_FACTOR, bufs["sh"].ptr, False, None, None, None, bufs["tm"].ptr)
        t.tiles_create_weights_dev(tiles, bufs["z"].ptr, bufs["mw"].ptr, bufs["gb"].ptr)
        t.tiles_tree_weights_dev(n, bufs["mw"].ptr, bufs["tm"].ptr, bufs["w"].ptr)
        zvals = bufs["z"].download(np.float32, (n, Z, Z))
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
        pine = bufs["pt"].download(np.uint8, (sizes["pt"],)).view(pkg.TREE_PLACE_DTYPE).reshape(n, cap_p)
        pc = bufs["pc"].download(np.uint32, (n,))
        decid = bufs["dt"].download(np.uint8, (sizes["dt"],)).view(pkg.DECID_PLACE_DTYPE).reshape(n, cap_d)
        dc = bufs["dc"].download(np.uint32, (n,))
        got = (bufs["tm"].download(np.uint8, (n, W, W, 2)), bufs["upd"].download(np.uint8, (n,)), bufs["trm"].download(np.float32, (n,)), bufs["lc"].download(np.uint32, (n,)))
        got_sh, mw, got_w = bufs["sh"].download(np.uint8, (n, W, W, 4)), bufs["mw"].download(np.uint8, (n, W, W, 4)), bufs["w"].download(np.uint8, (n, W, W, 4))
    finally:
        for b in bufs.values():
            b.free()
    # the model chain
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    psc = tpm.Scene(orc, ocfg, tpm.TreeParams(**TP))
    want_p = tpm.place(psc, tiles, 0, 0, None, [(stats[i].mzmin, stats[i].mzmax) for i in range(n)])
    want_d = dpm.place(psc, dpm.DecidParams(**DP), tiles, 0, 0, None, stats, zvals)
    tpc.compare("chain, pine / palm", pine, pc, want_p, cap_p)
    dpc.compare("chain, deciduous", decid, dc, want_d, cap_d)
    assert max(len(w) for w in want_p) <= cap_p and max(len(w) for w in want_d) <= cap_d
    mp, md = np.zeros((n, cap_p), tpm.PLACE_DTYPE), np.zeros((n, cap_d), dpm.PLACE_DTYPE)
    for i in range(n):
        if want_p[i]:
            mp[i, :len(want_p[i])] = np.array(want_p[i], tpm.PLACE_DTYPE)
        if want_d[i]:
            md[i, :len(want_d[i])] = np.array(want_d[i], dpm.PLACE_DTYPE)
    sc = tmm.Scene(orc.state(), cfg)
    tally = tam.new_tally()
    want = tam.Batch(sc, tam.SizeParams(), tiles, cap_l, mp, np.array([len(w) for w in want_p], np.uint32), md, np.array([len(w) for w in want_d], np.uint32), None, by_id,
                     flags, tally=tally).run()
    tac.compare(f"chain S={S}", got, want)
    # the tiles were chosen so that every mechanism is at work
    assert tally["pulled"] > 0 and tally["pushed"] > 0 and tally["own"] > 0 and tally["by_id"] > 0 and len(tally["types"]) >= 2, tally
    assert sum(len(w) for w in want_p) > 0 and sum(len(w) for w in want_d) > 0 and want[1].any() and not want[1][n - 2]
    want_sh = tmm.shadow_texture(S, LIGHT_FACTOR, 0, None, None, None, want[0])
    bad = np.argwhere(got_sh != want_sh)
    assert len(bad) == 0, f"shadow texture: {len(bad)} bytes differ, first at {bad[0].tolist()}"
    assert (want_sh[..., 1] != 255).any()
    want_w = tmm.tree_weights(mw, want[0])
    bad = np.argwhere(got_w != want_w)
    assert len(bad) == 0, f"tree weights: {len(bad)} bytes differ, first at {bad[0].tolist()}"
    return tally
