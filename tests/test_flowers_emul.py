"""The flowers (terra_tiles_place_flowers, terra_tiles_edit_flowers, terra_set_flower_params) through the host emulator -- the driver's one-thread-per-tile form --
against tests/flower_model.py, byte for byte on records, aux words and counts, in order; the generator's jump-ahead against literal stepping; the closed form of the
remove_element loop that k_flowers_remove uses; the settings and the refusals.

The colour.  The issue this feature answers took colors[int(0.5*NUM_COLORS*color_val)%NUM_COLORS] for an out-of-bounds read where the int is negative and proposed
colors[ix + 3] there.  The source says otherwise: NUM_COLORS is `unsigned`, so the int converts to unsigned before the remainder and the index is 0 .. 2 for every
value (test_colour_index_is_the_unsigned_remainder).  The model and the library follow the source, and every comparison here -- the flowers with a negative int
included -- is byte for byte against that.

test_model_draw_order, test_colour_index_is_the_unsigned_remainder, test_jump_ahead_identity_model and test_remove_closed_form pass without the feature; the two host
programs need its header and every other test its entry points: they fail without it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flower_cases as fc
import flower_model as fm
import orclib
import tree_place_model as tpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_draw_order(orc):
    """the model's draws for one accepted candidate against the oracle's generator: test draw, height, y's rand_float, x's rand_float, the normal's z, y, x, the radius,
    the colour -- nine draws, in that order; a rejected candidate takes one"""
    cfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=16)
    orc.init(cfg)
    sc = fm.Scene(orc, cfg, fm.Params(flower_density=1.0), hist=())
    fields = [np.full((16, 16), -5.0, f32), np.full((16, 16), 0.1, f32)]  # dval far below hthresh 0.5: accepted
    for (s1, s2) in [(1, 1), (123, 456), (40014, 7)]:
        out, tally = [], fm.new_tally()
        rgen = tpm.RandGen(s1, s2)
        fm.add_flowers(sc, rgen, fields, 255, sc.get_median_height(0.5), 3, 5, out, tally)
        assert len(out) == 1 and tally["accepted"] == 1
        rec = out[0][0]
        u = orc.rand_uniforms(s1, s2, 0.0, 1.0, 9)       # float(randd()) of every draw
        ri = orc.rand_floats(s1, s2, 4)                   # rand_float of draws 0 .. 3
        sr = orc.rand_uniforms(s1, s2, -1.0, 1.0, 9)      # signed_rand_float (2*float(randd()) - 1 is exact)
        height = f32(f32(0.02) * f32(f32(0.85) + f32(f32(f32(1.0) - f32(0.85)) * u[1])))
        assert float(rec["height"]) == float(height) == float(rec["pos"][2])
        assert float(rec["pos"][1]) == float(f32(float(sc.DY_VAL) * (float(f32(f32(5) + ri[2])) - 0.5)))  # the third draw is y's
        assert float(rec["pos"][0]) == float(f32(float(sc.DX_VAL) * (float(f32(f32(3) + ri[3])) - 0.5)))  # the fourth x's
        n = [f32(f32(0.2) * sr[6]), f32(f32(0.2) * sr[5]), f32(f32(1.0) + f32(f32(0.2) * sr[4]))]        # z drew first
        mag = f32(np.sqrt(f32(f32(f32(n[0] * n[0]) + f32(n[1] * n[1])) + f32(n[2] * n[2]))))
        assert [float(v) for v in rec["normal"]] == [float(f32(c / mag)) for c in n]
        assert float(rec["radius"]) == float(f32(f32(0.002) * f32(f32(1.5) + f32(f32(f32(2.5) - f32(1.5)) * u[7]))))
        color_val = f32(0.1 + 0.25 * float(sr[8]))
        assert [float(v) for v in rec["color"]] == [float(f32(v)) for v in fm.COLORS[int(1.5 * float(color_val)) % 3]]  # (color_val >= -0.15: the int is 0)
        assert rgen.rand() == int(orc.rand_ints(s1, s2, 10)[9])  # nine draws
        # rejected: one draw
        out2, rgen2 = [], tpm.RandGen(s1, s2)
        fm.add_flowers(sc, rgen2, [np.full((16, 16), 5.0, f32), fields[1]], 255, sc.get_median_height(0.5), 3, 5, out2, fm.new_tally())
        assert not out2 and rgen2.rand() == int(orc.rand_ints(s1, s2, 2)[1])


def test_colour_index_is_the_unsigned_remainder(tmp_path):
    """`int % unsigned` as a C++ compiler evaluates it, against the model's rule and against the signed remainder the aux word reports"""
    src = tmp_path / "rem.cpp"
    src.write_text('#include <cstdio>\nint main() {unsigned const NUM_COLORS(3); for (int v = -7; v <= 7; ++v) {float const color_val = v/1.5f + (v < 0 ? -0.01f : 0.01f);'
                   ' printf("%d %u %d\\n", int(0.5*NUM_COLORS*color_val), unsigned(int(0.5*NUM_COLORS*color_val)%NUM_COLORS), int(0.5*NUM_COLORS*color_val)%3);} return 0;}\n')
    exe = str(tmp_path / "rem")
    subprocess.run(["g++", "-std=c++17", "-o", exe, str(src)], check=True)
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(-7, 8))
    for iq, index, signed_rem in rows:
        assert index == (iq % 2 ** 32) % 3 and 0 <= index <= 2       # what the model (and the library) index colors[] with
        assert signed_rem == tpm.cmod(iq, 3)                         # what aux reports (+ 2)
    assert dict((r[0], r[1]) for r in rows)[-1] == 0 and tpm.cmod(-1, 3) + 3 == 2  # not "the signed remainder plus 3"


def test_jump_ahead_identity_host_program(tmp_path):
    """tests/flowers_jump_check.cpp exercises terra_flowers.hpp's lcg_mulmod / lcg_powmod / lcg_jump against literal stepping, seeds <= 0 included"""
    exe = str(tmp_path / "flowers_jump_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "flowers_jump_check.cpp"), "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)"), r.stdout + r.stderr


def test_speculative_walk_host_program(tmp_path):
    """tests/flowers_wave_check.cpp: k_flowers_place's walk restated for 64 lanes in lockstep on the host against the literal loop, on random tiles and rectangles"""
    exe = str(tmp_path / "flowers_wave_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "flowers_wave_check.cpp"), "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)"), r.stdout + r.stderr


def test_jump_ahead_identity_model():
    """the same identity on the model's generator (the reference's `long` statements): after one literal step the state is in [0, m) and k steps on it is a^k*s mod m"""
    M1, A1, M2, A2 = 2147483563, 40014, 2147483399, 40692
    for (s1, s2) in [(1, 1), (0, 0), (-17, -4), (123 - 7 * 20, 456 - 23 * 20), (-2 ** 31, 2 ** 31 - 1), (-53668, -52774), (2 ** 31 - 1, -2 ** 31)]:
        r = tpm.RandGen(s1, s2)
        r._advance()
        b1, b2 = r.rseed1, r.rseed2
        assert 0 <= b1 < M1 and 0 <= b2 < M2
        for k in range(1, 400):
            r._advance()
            assert (r.rseed1, r.rseed2) == (pow(A1, k, M1) * b1 % M1, pow(A2, k, M2) * b2 % M2), (s1, s2, k)


def test_remove_closed_form():
    """the remove_element loop's result in closed form, as k_flowers_remove computes it: with M survivors a survivor below M stays, and the holes below M, ascending,
    receive the survivors at M and above, descending -- against the literal loop"""
    rs = np.random.RandomState(11)
    for trial in range(300):
        n = int(rs.randint(0, 40))
        dead = rs.rand(n) < rs.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        lst = [(i, None, None, None) for i in range(n)]
        fm.remove_elements(lst, lambda rec: dead[rec])
        keep = [i for i in range(n) if not dead[i]]
        m = len(keep)
        closed = list(range(m))
        tail = [i for i in keep if i >= m]
        holes = [i for i in range(m) if dead[i]]
        assert len(holes) == len(tail)
        for k, h in enumerate(holes):
            closed[h] = tail[len(tail) - 1 - k]
        assert [x[0] for x in lst] == closed, (trial, dead.tolist())


def test_cases_are_not_vacuous(pkg, orc):
    """on the model alone: every case exercises what it is named for"""
    assert pkg.FLOWER_DTYPE == fm.FLOWER_DTYPE and pkg.FLOWER_AUX_FIXED == fm.AUX_FIXED
    for case in CASES:
        w, want, tally = fc.model(orc, case)
        assert case.check(tally, want), (case.name, tally, [len(x) for x in want])
        if case.name != "capacity_small":
            assert max(len(x) for x in want) <= case.capacity, case.name
    # the shore tile: hundreds of flowers on either side of the int -> unsigned conversion of the colour index
    t = fc.MODEL["shore_s128"][2]
    assert min(t["negative_ix"], t["nonnegative_ix"]) >= 100, t
    # the tiles with negative coordinates: the seeds the model used
    sc = fc.scene_of(orc, BY_NAME["negative_tiles_s20"])
    seeds = [(fm.seed(sc, tx, ty).rseed1, fm.seed(sc, tx, ty).rseed2) for tx, ty in fc.NEG_TILES]
    assert seeds[1][0] <= 0 and seeds[1][1] <= 0 and seeds[2][0] <= 0 < seeds[2][1] and seeds[3][1] <= 0 < seeds[3][0], seeds
    # remove_dense: a tile with more than 512 records before the stroke and M survivors, records removed below M and at M and above: every sweep of the kernel's
    # removal runs more than once and the moves happen; the tiles the brush misses have more than 256 records and lose none
    ec = fc.edit_case(orc, "remove_dense")
    w, base, _ = fc.model(orc, ec.base)
    lists = [list(x) for x in base]
    brush, upd, rg = ec.strokes[0]
    fm.edit(fc.scene_of(orc, ec.base), ec.base.tiles, w, lists, (tuple(brush.pos), brush.radius, False, brush.shape == 0), upd, rg)
    m, kept = len(lists[0]), {id(x) for x in lists[0]}
    gone = [i for i, x in enumerate(base[0]) if id(x) not in kept]
    assert len(base[0]) > 512 and m > 256 and len(base[0]) - m > 256, (len(base[0]), m)
    assert sum(i < m for i in gone) >= 10 and sum(i >= m for i in gone) >= 10, (m, gone)
    assert all(len(a) == len(b) > 256 for a, b in zip(lists[1:], base[1:]))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    fc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    fc.run_case(pkg, emul, orc, case, dev=True)


def test_without_aux(pkg, emul, orc):
    fc.run_case(pkg, emul, orc, BY_NAME["pattern_s20"], aux=False)
    fc.run_case(pkg, emul, orc, BY_NAME["skipped_tile"], dev=True, aux=False)
    fc.run_edit_case(pkg, emul, orc, fc.edit_case(orc, "two_strokes"), aux=False)


@pytest.mark.parametrize("name", fc.EDIT_NAMES)
def test_edit_cases(pkg, emul, orc, name):
    fc.run_edit_case(pkg, emul, orc, fc.edit_case(orc, name))


@pytest.mark.parametrize("name", fc.EDIT_NAMES)
def test_edit_cases_dev_entry_point(pkg, emul, orc, name):
    fc.run_edit_case(pkg, emul, orc, fc.edit_case(orc, name), dev=True)


def test_flower_params(pkg, emul):
    fp = emul.get_flower_params()  # the reference's defaults
    assert (fp.flower_density, fp.no_grass, list(fp.flower_color)) == (0.0, 0, [0.0] * 4) and f32(fp.grass_length) == f32(0.02) and f32(fp.grass_width) == f32(0.002)
    emul.set_flower_params(pkg.make_flower_params(2.0, 0.03, 0.004, (0.1, 0.2, 0.3, 1.0), 1))
    fp = emul.get_flower_params()
    assert (fp.flower_density, fp.no_grass) == (2.0, 1) and [f32(v) for v in fp.flower_color] == [f32(0.1), f32(0.2), f32(0.3), f32(1.0)]
    for bad in (dict(flower_density=-1.0), dict(flower_density=float("nan")), dict(flower_density=float("inf")), dict(flower_density=1025.0), dict(grass_length=-0.1),
                dict(grass_length=float("nan")), dict(grass_width=-1.0), dict(grass_width=float("inf"))):
        with pytest.raises(pkg.TerraError) as e:
            emul.set_flower_params(pkg.make_flower_params(**bad))
        assert e.value.code == fc.ERR_ARG, bad
    assert emul.get_flower_params().flower_density == 2.0  # a refused setting changes nothing
    assert emul.lib.terra_set_flower_params(emul.ctx, None) == fc.ERR_ARG and emul.lib.terra_get_flower_params(emul.ctx, None) == fc.ERR_ARG


def test_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    S, n, cap = 20, 3, 16
    tiles = fc.BASE.tiles
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    txy = np.array(tiles, np.int32)
    w = np.full((n, S + 1, S + 1, 4), 255, np.uint8)
    fl, ax, cn, st = np.zeros((n, cap), pkg.FLOWER_DTYPE), np.zeros((n, cap), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    up, rg = np.ones(n, np.uint8), np.array([[1, 1, 5, 5]] * n, np.uint32)
    f, g, ef, eg = lib.terra_tiles_place_flowers, lib.terra_tiles_place_flowers_dev, lib.terra_tiles_edit_flowers, lib.terra_tiles_edit_flowers_dev
    p = lambda a: a.ctypes.data  # noqa: E731
    br = pkg.make_grass_brush((0.0, 0.0, 0.0), 0.3, 1, 0, 0.1)
    bp = ctypes.byref(br)
    # before terra_init_scene
    assert f(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), p(cn)) == fc.ERR_STATE and g(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), p(cn)) == fc.ERR_STATE
    assert ef(ctx, p(txy), n, 0, 0, None, bp, p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_STATE
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    # skip_generate: zero counts, the weights are not touched (they may be null)
    cn[:] = 7
    assert f(ctx, p(txy), n, None, None, cap, p(fl), p(ax), p(cn)) == 0 and not cn.any()
    cn[:] = 7
    assert g(ctx, p(txy), n, None, None, cap, p(fl), p(ax), p(cn)) == 0 and not cn.any()
    emul.set_flower_params(pkg.make_flower_params(flower_density=2.0))
    assert f(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), p(cn)) == 0 and cn.all() and (cn > cap).all()
    counts = cn.copy()
    assert f(ctx, p(txy), n, None, p(w), 0, None, None, p(cn)) == 0 and cn.tolist() == counts.tolist()  # capacity 0: counts only
    # null pointers, n == 0, alignment
    assert f(ctx, None, n, None, p(w), cap, p(fl), p(ax), p(cn)) == fc.ERR_ARG and "null" in last()
    assert f(ctx, p(txy), n, None, None, cap, p(fl), p(ax), p(cn)) == fc.ERR_ARG and "null" in last()
    assert f(ctx, p(txy), n, None, p(w), cap, None, p(ax), p(cn)) == fc.ERR_ARG and "null" in last()
    assert f(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), None) == fc.ERR_ARG and "null" in last()
    assert g(ctx, p(txy), n, None, None, cap, p(fl), p(ax), p(cn)) == fc.ERR_ARG and "null" in last()
    assert f(ctx, None, 0, None, None, cap, None, None, None) == 0 and g(ctx, None, 0, None, None, cap, None, None, None) == 0
    assert g(ctx, p(txy), n, None, p(w), cap, p(fl) + 2, p(ax), p(cn)) == fc.ERR_ARG and "aligned" in last()
    assert g(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax) + 1, p(cn)) == fc.ERR_ARG and "aligned" in last()
    assert g(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), p(cn) + 2) == fc.ERR_ARG and "aligned" in last()
    # the edit
    cn[:] = np.minimum(counts, cap)
    assert ef(ctx, p(txy), n, 0, 0, None, bp, p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn), p(st)) == 0 and st.tolist() == [1, 1, 1]
    assert ef(ctx, p(txy), n, 0, 0, None, None, p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_ARG and "null" in last()
    assert ef(ctx, p(txy), n, 0, 0, None, bp, None, p(rg), p(w), cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_ARG and "null" in last()
    assert ef(ctx, p(txy), n, 0, 0, None, bp, p(up), None, p(w), cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_ARG and "ranges" in last()
    assert ef(ctx, p(txy), n, 0, 0, None, bp, p(up), p(rg), None, cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_ARG and "weights" in last()
    assert ef(ctx, p(txy), n, 0, 0, None, bp, p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn), None) == fc.ERR_ARG and "null" in last()
    assert eg(ctx, p(txy), n, 0, 0, None, bp, p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn) + 2, p(st)) == fc.ERR_ARG and "aligned" in last()
    bad = pkg.make_grass_brush((0.0, 0.0, 0.0), 0.3, 1, 8, 0.1)
    assert ef(ctx, p(txy), n, 0, 0, None, ctypes.byref(bad), p(up), p(rg), p(w), cap, p(fl), p(ax), p(cn), p(st)) == fc.ERR_ARG and "shape" in last()
    rem = pkg.make_grass_brush((0.0, 0.0, 0.0), 0.3, 0, 1, 0.1)
    assert ef(ctx, p(txy), n, 0, 0, None, ctypes.byref(rem), p(up), None, None, cap, p(fl), p(ax), p(cn), p(st)) == 0  # a removal reads neither ranges nor weights
    assert ef(ctx, None, 0, 0, 0, None, bp, None, None, None, cap, None, None, None, None) == 0
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=130))
    assert f(ctx, p(txy), n, None, p(w), cap, p(fl), p(ax), p(cn)) == fc.ERR_ARG
    assert f(ctx, None, 0, None, None, cap, None, None, None) == fc.ERR_ARG  # n == 0 does nothing only once the scene and the tile size have passed
    assert ef(ctx, None, 0, 0, 0, None, bp, None, None, None, cap, None, None, None, None) == fc.ERR_ARG


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_flowers.py::test_resident_chain on the emulator's "device" memory"""
    fc.run_resident_chain(pkg, emul, orc)
