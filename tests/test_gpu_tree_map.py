"""The tree map, the shadow texture and the tree weights (terra_tiles_tree_map[_dev], terra_tiles_shadow_texture[_dev], terra_tiles_tree_weights[_dev]) through HIP on
the MI355X -- k_tree_splats + k_tree_map, k_shadow_texture, k_tree_weights, and the simple forms under "kernels.simple" -- against tests/tree_map_model.py, byte
for byte, every tile and every texel: the emulator's cases, all 256^3 (tree_ao, dirt, grass) weights texels, and the chain zvals -> shadows -> AO -> tree map ->
shadow texture -> weights -> tree weights on a device-resident 64 x 64 batch with nothing read back in between."""
import contextlib

import numpy as np
import pytest

import orclib
import tree_map_cases as tmc
import tree_map_model as tmm

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def simple_form(gpu):
    gpu.set_option("kernels.simple", "1")
    try:
        yield
    finally:
        gpu.set_option("kernels.simple", "0")


@pytest.mark.parametrize("S", [128, 64, 192, 256])
def test_cases(pkg, gpu, orc, S):
    tmc.run_cases(pkg, gpu, orc, S)


def test_cases_dx_differs_from_dy(pkg, gpu, orc):
    tmc.run_cases(pkg, gpu, orc, 128, (4.0, 6.0, 4.0))


@pytest.mark.parametrize("S", [128, 256])
def test_cases_simple_form(pkg, gpu, orc, S):
    with simple_form(gpu):
        tmc.run_cases(pkg, gpu, orc, S)


def test_order_matters_in_the_model(pkg, gpu, orc):
    assert tmc.order_sensitive(tmc.setup(pkg, gpu, orc)) > 0


def test_continue(pkg, gpu, orc):
    tmc.run_continue(pkg, gpu, orc)
    tmc.run_continue(pkg, gpu, orc, 256)
    with simple_form(gpu):
        tmc.run_continue(pkg, gpu, orc)


@pytest.mark.parametrize("S", [64, 128, 192, 256])
def test_shadow_texture_exhaustive(pkg, gpu, orc, S):
    tmc.run_shadow_texture(pkg, gpu, orc, S)


def test_shadow_texture_exhaustive_simple_form(pkg, gpu, orc):
    with simple_form(gpu):
        tmc.run_shadow_texture(pkg, gpu, orc, 128)


def weights_on_device(gpu, w, tree, in_place):
    n = len(w)
    wb, tb = gpu.alloc(w.nbytes).upload(w), gpu.alloc(tree.nbytes).upload(tree)
    ob = wb if in_place else gpu.alloc(w.nbytes)
    try:
        gpu.tiles_tree_weights_dev(n, wb.ptr, tb.ptr, ob.ptr)
        out = ob.download(np.uint8, w.shape)
        if not in_place:
            assert (wb.download(np.uint8, w.shape) == w).all()  # mesh_weight_data is left as it was
        return out
    finally:
        for b in {wb, tb, ob}:
            b.free()


def test_tree_weights_exhaustive(pkg, gpu, orc):
    """every (tree_ao, dirt, grass): 256^3 texels in 1009 tiles, out of place and in place; the rock-255 skip; no tree map"""
    tmc.setup(pkg, gpu, orc)
    w, tree = tmc.weights_inputs()
    assert len(w) * 129 * 129 >= 256 ** 3
    want = tmc.model_weights_chunked(w, tree)
    assert (want != w).any()
    for in_place in (False, True):
        got = weights_on_device(gpu, w, tree, in_place)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (f"in_place={in_place}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {w[tuple(bad[0][:3])]} tree {tree[tuple(bad[0][:3])]} -> "
                               f"{got[tuple(bad[0][:3])]} != {want[tuple(bad[0][:3])]}")
    w255 = w[:64].copy()
    w255[..., tmm.ROCK] = 255
    assert (weights_on_device(gpu, w255, tree[:64], False) == w255).all()
    assert (gpu.tiles_tree_weights(w[:64], None) == w[:64]).all()
    with simple_form(gpu):
        assert (weights_on_device(gpu, w[:128], tree[:128], True) == want[:128]).all()
    gpu.init_scene(pkg.make_config(mesh_xy=64))
    try:
        with pytest.raises(pkg.TerraError) as e:
            gpu.tiles_tree_weights(w[:1], tree[:1])
        assert e.value.code == tmc.ERR_ARG and "tile size 128" in str(e.value)
    finally:
        tmc.setup(pkg, gpu, orc)  # the context goes on at the default scene


def seeded_lists(sc, tiles, rs, per_tile):
    """per_tile trees in every tile's frame, a third of them within a few texels of a border or beyond it (what a neighbour's push leaves in the list)"""
    S = sc.S
    n = len(tiles)
    fx, fy = rs.uniform(-4.0, S + 4.0, (2, n, per_tile))
    edge = rs.randint(0, 3, (n, per_tile)) == 0
    fx = np.where(edge, rs.choice([-2.5, -0.5, 0.0, 1.5, S - 1.0, S + 0.5, S + 3.0], (n, per_tile)), fx)
    r = rs.uniform(0.3, 6.9, (n, per_tile))
    txy = np.asarray(tiles, np.int64)
    xs = np.array([float(sc.get_xval(int(tx) * S)) for tx in txy[:, 0]])[:, None] + fx * float(sc.DX_VAL)
    ys = np.array([float(sc.get_yval(int(ty) * S)) for ty in txy[:, 1]])[:, None] + fy * float(sc.DY_VAL)
    sp = np.zeros(n * per_tile, tmm.SPLAT_DTYPE)
    sp["x"], sp["y"], sp["radius"] = xs.reshape(-1), ys.reshape(-1), (r * float(sc.DX_VAL)).reshape(-1)
    # uneven lists: tile t owns per_tile records less t % 5 (the records left over belong to nobody), every 17th tile has none
    first = np.zeros(n + 1, np.uint32)
    cnt = np.array([0 if t % 17 == 5 else per_tile - t % 5 for t in range(n)], np.uint32)
    first[1:] = np.cumsum(cnt)
    keep = np.concatenate([np.arange(t * per_tile, t * per_tile + int(cnt[t])) for t in range(n)])
    return np.ascontiguousarray(sp[keep]), first


def resident_chain(pkg, gpu, orc, S, side, per_tile, with_weights):
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    gpu.init_scene(cfg)
    sc = tmm.Scene(orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S)), cfg)
    if with_weights:
        gpu.set_landscape(pkg.make_landscape(grass_density=1))
    tiles = [(x, y) for y in range(-side // 2, side // 2) for x in range(-side // 2, side // 2)]
    n, W, Z = len(tiles), S + 1, S + 2
    rs = np.random.RandomState(31)
    sp, first = seeded_lists(sc, tiles, rs, per_tile)
    distant = ((np.arange(n) % 11) == 7).astype(np.uint8)
    light_factor = 0.47  # both lights up
    bufs = {k: gpu.alloc(b) for k, b in dict(z=n * Z * Z * 4, sun=n * Z * Z, moon=n * Z * Z, ao=n * W * W, tm=n * W * W * 2, upd=n, sh=n * W * W * 4, sp=sp.nbytes, dist=n).items()}
    if with_weights:
        bufs.update(mw=gpu.alloc(n * W * W * 4), gb=gpu.alloc(n * 32 * 32 * 12), w=gpu.alloc(n * W * W * 4))
    try:
        bufs["sp"].upload(sp); bufs["dist"].upload(distant)
        # the chain: nothing is read back between its steps
        gpu.tiles_create_zvals_dev(tiles, 0, bufs["z"].ptr)
        gpu.tiles_mesh_shadows_dev(tiles, bufs["z"].ptr, (1.0, 0.6, 0.3), bufs["sun"].ptr)
        gpu.tiles_mesh_shadows_dev(tiles, bufs["z"].ptr, (-0.4, -1.0, 0.15), bufs["moon"].ptr)
        gpu.tiles_ao_lighting_dev(tiles, bufs["z"].ptr, bufs["ao"].ptr)
        gpu.tiles_tree_map_dev(tiles, bufs["sp"].ptr, first, bufs["tm"].ptr, bufs["upd"].ptr, True, 0, 0, bufs["dist"].ptr)
        gpu.tiles_shadow_texture_dev(n, light_factor, bufs["sh"].ptr, True, bufs["sun"].ptr, bufs["moon"].ptr, bufs["ao"].ptr, bufs["tm"].ptr)
        if with_weights:
            gpu.tiles_create_weights_dev(tiles, bufs["z"].ptr, bufs["mw"].ptr, bufs["gb"].ptr)
            gpu.tiles_tree_weights_dev(n, bufs["mw"].ptr, bufs["tm"].ptr, bufs["w"].ptr)
        # the model on the downloaded intermediates (smask, AO and mesh_weight_data have parity tests of their own)
        sun, moon = bufs["sun"].download(np.uint8, (n, Z, Z)), bufs["moon"].download(np.uint8, (n, Z, Z))
        ao = bufs["ao"].download(np.uint8, (n, W, W))
        want_tm, want_upd = tmm.tiles_tree_map(sc, tiles, sp, first, True, None, 0, 0, distant)
        tmc.compare(f"resident S={S}", bufs["tm"].download(np.uint8, (n, W, W, 2)), bufs["upd"].download(np.uint8, (n,)), want_tm, want_upd)
        assert want_upd.sum() > n // 2 and not want_upd[distant == 1].any() and (sun != 0).any() and (moon != 0).any()
        want_sh = np.concatenate([tmm.shadow_texture(S, light_factor, 1, sun[i:i + 256], moon[i:i + 256], ao[i:i + 256], want_tm[i:i + 256]) for i in range(0, n, 256)])
        got_sh = bufs["sh"].download(np.uint8, (n, W, W, 4))
        bad = np.argwhere(got_sh != want_sh)
        assert len(bad) == 0, f"shadow texture S={S}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got_sh[tuple(bad[0])]} != {want_sh[tuple(bad[0])]}"
        assert len(np.unique(want_sh[..., 0])) > 2 and (want_sh[..., 1] != 255).any() and (want_sh[..., 3] == 0).all()
        if with_weights:
            mw = bufs["mw"].download(np.uint8, (n, W, W, 4))
            want_w = tmc.model_weights_chunked(mw, want_tm)
            got_w = bufs["w"].download(np.uint8, (n, W, W, 4))
            bad = np.argwhere(got_w != want_w)
            assert len(bad) == 0, f"weights: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got_w[tuple(bad[0])]} != {want_w[tuple(bad[0])]}"
            assert (want_w != mw).any()
    finally:
        for b in bufs.values():
            b.free()


def test_resident_chain(pkg, gpu, orc):
    """the full 64 x 64 batch at S = 128: 4096 tiles, every tile a seeded list"""
    resident_chain(pkg, gpu, orc, 128, 64, 14, True)


def test_resident_chain_tile_size_256(pkg, gpu, orc):
    """a 16 x 16 batch at S = 256: the tree map and the shadow texture (the weights family runs at 128 only)"""
    resident_chain(pkg, gpu, orc, 256, 16, 40, False)

