"""Sphere collisions and tree box tests against the containers of a tile batch (terra_tiles_sphere_collide[_dev], terra_tiles_cube_int_trees[_dev]) through the host
emulator -- the driver's simple form: a logical thread per query, the reference's loops -- against tests/collide_model.py, every output byte; the refusals with every
output untouched; the kernel's 64-wide ballot-and-resume scheme as a stand-alone host program against the literal loop.

test_model_alone passes without the feature; every other test needs its entry points and fails without them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import collide_cases as cc
import collide_model as cm
import decid_view_model as dm
import scenery_view_cases as svc
import tree_view_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32


def test_model_alone(orc):
    """every case exercises what it is named for, on the model alone; the model's geometry is the view models' on the shared records"""
    union = cm.new_tally()
    for case in CASES:
        sc, g, stats, inp, hits, (cres, ctile), tally = cc.model(orc, case)
        assert case.check(tally, hits), (case.name, {k: x for k, x in tally.items() if x}, hits.tolist())
        assert len(inp.queries) + len(inp.cubes) > 0 and len(case.tiles) <= 4
        for k, x in tally.items():
            if k == "hits_by_kind":
                union[k] = [a + b for a, b in zip(union[k], x)]
            elif k == "max_hits":
                union[k] = max(union[k], x)
            else:
                union[k] += x
        # a query that never reaches the containers keeps its pos; one that is answered names its tile
        for q, h in zip(inp.query_array(), hits):
            stage = (int(h["word"]) & 0xF00) >> cm.STAGE_SHIFT
            if stage != cm.TESTED:
                assert h["pos"].tobytes() == q["pos"].tobytes() and h["nhits"] == 0 and not int(h["word"]) & 0xFF, (case.name, q, h)
            assert (h["tile"] == -1) == (stage in (cm.NO_TILE, cm.BAD_QUERY)), (case.name, q, h)
    for k in ("tested", "no_tile", "distant", "outside", "above", "bad_query", "tile_out_of_range", "hits_pine", "hits_decid", "hits_scenery", "chain_created", "chain_removed",
              "chain_created_across", "round_trip_only", "gate_exit_pine", "gate_pass_pine", "gate_zero_area_pine", "gate_exit_decid", "gate_pass_decid", "gate_zero_area_decid",
              "empty_pine", "empty_decid", "no_scenery", "short_tree_exit", "short_tree_extended", "bush", "zero_normal", "rock_shape_undecided", "rock_shape_override",
              "voxel_rock_override", "log_in_reach", "mushroom_in_reach", "dropped_pine", "dropped_decid", "rotated", "cube_hit", "cube_no_tile", "cube_bad", "cube_empty",
              "cube_culled", "cube_leaves_only", "cube_branches_only", "cube_boxes_missed", "cube_sphere_missed", "cube_zero_area"):
        assert union[k] > 0, k
    assert all(union["hits_by_kind"][k] > 0 for k in (svc.LEAFY, svc.PLANT, svc.ROCK_SHAPE, svc.SURFACE_ROCK, svc.VOXEL_ROCK, svc.ROCK, svc.STUMP)), union["hits_by_kind"]
    assert union["hits_by_kind"][svc.LOG] == 0 and union["hits_by_kind"][svc.MUSHROOM] == 0 and union["max_hits"] == 70
    # the scenery is walked by kind: in record order the same records leave another pos
    case = BY_NAME["scenery_kind_order"]
    sc, g, stats, inp, hits, _, tally = cc.model(orc, case)
    other = cc.batch_of(sc, g, case, stats, inp, scenery_in_record_order=True).sphere_collide(inp.query_array())
    assert all(other[i]["pos"].tobytes() != hits[i]["pos"].tobytes() for i in range(2)), (other, hits)
    # the round trip alone: pos differs from the query's in the last bits, and by no more
    case = BY_NAME["round_trip_alone"]
    hits, q = cc.model(orc, case)[4], cc.model(orc, case)[3].query_array()
    d = np.abs(hits["pos"].astype(np.float64) - q["pos"].astype(np.float64))
    assert 0.0 < d.max() < 4.0e-6 and (hits["word"] == 0).all()
    # the model's geometry against the view models on the shared records: both all_bcubes and the numbers of valid records of the dense case (the trunk cylinders are
    # tree_view_model.SmallTree's own: the model holds the very objects the view model makes)
    case = BY_NAME["three_hundred_queries"]
    sc, g, stats, inp, hits, _, tally = cc.model(orc, case)
    b = cc.batch_of(sc, g, case, stats, inp)
    a = vm.Args()
    want_p = vm.draw(sc, cc.tvc.view_of(_ViewCase()), vm.Globals(g.p, a, g.instanced, g.insts), case.tiles, stats, inp.pine.pine, inp.pine.counts, None, None, inp.pine.override,
                     case.poff2[0], case.poff2[1], vm.new_tally())
    want_d = dm.draw(sc, cc.tvc.view_of(_ViewCase()), dm.Args(1.0, 1.0, (0.3, 0.15, 0.25, 0.1)), case.tiles, inp.data, inp.decid, inp.decid_counts, None, None, case.doff2[0],
                     case.doff2[1], dm.new_tally())
    for t in range(len(case.tiles)):
        assert [x for r in b.objs[t].pine_bcube for x in r] == list(want_p[t].bcube) and [x for r in b.objs[t].decid_bcube for x in r] == list(want_d[t].bcube), t
        assert len(b.objs[t].small) == want_p[t].num_trees and len(b.objs[t].decid) == want_d[t].num_trees


class _ViewCase:
    view = dict(pos=(0.25, 0.25, 0.5), angle=0.6, aspect=1.5, near=0.05, far=200.0, dir=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    valid = 1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, orc, case):
    cc.run_case(pkg, emul, orc, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, orc, case):
    """the device-pointer form on the emulator's "device" memory"""
    cc.run_case(pkg, emul, orc, case, dev=True)


def _setup(pkg, orc, name):
    case = BY_NAME[name]
    sc, g, stats, inp, hits, cubes, tally = cc.model(orc, case)
    return case, g, stats, inp, hits, cubes


def test_sphere_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case, g, stats, inp, hits, _ = _setup(pkg, orc, "three_translations")
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    q = inp.query_array()
    out = np.full(len(q) * 6, 3, np.uint32)
    untouched = lambda: (out == 3).all()  # noqa: E731
    kw, sc = cc.host_arrays(pkg, case, stats, inp), cc.scalars(case)
    f, d = lib.terra_tiles_sphere_collide, lib.terra_tiles_sphere_collide_dev

    def call(fn, cin=None, **k):
        cin = pkg.make_collide_in(**kw, **sc) if cin is None else cin
        return fn(ctx, k.get("txy", p(txy)), k.get("n", n), ctypes.byref(cin) if cin != "null" else None, k.get("q", p(q)), k.get("nq", len(q)), k.get("out", p(out)))
    assert call(f) == cc.ERR_STATE and call(d) == cc.ERR_STATE and untouched()
    cc.configure(pkg, emul, case, g)
    for fn in (f, d):
        assert call(fn, "null") == cc.ERR_ARG and "null" in last()
        for k in ("txy", "q", "out"):
            assert call(fn, **{k: None}) == cc.ERR_ARG and "null" in last(), k
        assert call(fn, pkg.make_collide_in(**dict(kw, stats=None), **sc)) == cc.ERR_ARG and "null" in last()
        assert call(fn, pkg.make_collide_in(**dict(kw, tree_data=None), num_tree_data=cc.TABLE, **sc)) == cc.ERR_ARG and "null" in last()
        assert call(fn, pkg.make_collide_in(**dict(kw, br_scale=None), **sc)) == cc.ERR_ARG and "null" in last()
        assert call(fn, pkg.make_collide_in(**kw, **dict(sc, tree_depth_scale=0.0))) == cc.ERR_ARG and "tree_depth_scale" in last()
        assert call(fn, pkg.make_collide_in(**kw, **dict(sc, tree_depth_scale=float("nan")))) == cc.ERR_ARG and "tree_depth_scale" in last()
        assert call(fn, pkg.make_collide_in(**kw, num_tree_data=cc.TABLE - 1, **sc)) == cc.ERR_ARG and "num_shared_trees" in last()
        assert call(fn, pkg.make_collide_in(**kw, pine_capacity=2**31, **sc), n=2) == cc.ERR_ARG and "32 bits" in last()
        twice = txy.copy()
        twice[2] = twice[0]
        assert call(fn, txy=p(twice)) == cc.ERR_ARG and "twice" in last()
        assert untouched()
        # nq == 0 and n == 0 do nothing once the checks have passed; with n == 0 every query is answered "no tile"
        assert call(fn, nq=0, q=None, out=None) == 0 and untouched()
        assert call(fn, pkg.make_collide_in(**kw, **dict(sc, tree_depth_scale=-1.0)), nq=0) == cc.ERR_ARG
        assert call(fn, txy=p(twice), nq=0) == cc.ERR_ARG and "twice" in last()
        got = np.full(len(q), 3, cm.HIT_DTYPE)
        assert call(fn, pkg.make_collide_in(**sc), n=0, txy=None, out=p(got)) == 0
        assert got["pos"].tobytes() == q["pos"].tobytes() and (got["tile"] == -1).all() and (got["word"] == cm.NO_TILE << cm.STAGE_SHIFT).all() and not got["nhits"].any()
    # a misaligned pointer (the device form; the host form stages its arrays)
    assert call(d, q=p(q) + 2) == cc.ERR_ARG and "aligned" in last() and call(d, out=p(out) + 1) == cc.ERR_ARG and "aligned" in last()
    assert call(d, pkg.make_collide_in(**dict(kw, pine_counts=p(inp.pine.counts) + 2), pine_capacity=8, **sc)) == cc.ERR_ARG and "aligned" in last() and untouched()
    # instanced with a table of another length
    emul.set_tree_params(pkg.make_tree_params(tree_mode=3, instanced=1, num_pine_insts=5, num_palm_insts=5))
    assert call(f) == cc.ERR_ARG and "instances" in last() and call(d) == cc.ERR_ARG and untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=66))
    assert call(f) == cc.ERR_ARG and call(d) == cc.ERR_ARG and untouched()
    # a container that is not given is absent: the other two answer
    cc.configure(pkg, emul, case, g)
    only = pkg.make_collide_in(**{k: v for k, v in kw.items() if k not in ("decid", "decid_counts", "tree_data", "br_scale")}, **sc)
    got = emul.tiles_sphere_collide(case.tiles, only, q)
    assert (got["word"] == cm.HIT_PINE | cm.HIT_SCENERY).all()


def test_cubes_refused_and_zero(pkg, emul, orc):
    lib, ctx = emul.lib, emul.ctx
    case, g, stats, inp, _, (cres, ctile) = _setup(pkg, orc, "cubes")
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    cubes, ct = np.array(inp.cubes, f32), np.array(inp.cube_tile, np.int32)
    res, tile = np.full(len(cubes), 3, np.uint8), np.full(len(cubes), 3, np.int32)
    untouched = lambda: (res == 3).all() and (tile == 3).all()  # noqa: E731
    kw, sc = cc.host_arrays(pkg, case, stats, inp), cc.scalars(case)
    f, d = lib.terra_tiles_cube_int_trees, lib.terra_tiles_cube_int_trees_dev

    def call(fn, cin=None, **k):
        cin = pkg.make_collide_in(**kw, **sc) if cin is None else cin
        return fn(ctx, k.get("txy", p(txy)), k.get("n", n), ctypes.byref(cin) if cin != "null" else None, k.get("cu", p(cubes)), k.get("ct", p(ct)), k.get("nq", len(cubes)),
                  k.get("res", p(res)), k.get("tile", p(tile)))
    assert call(f) == cc.ERR_STATE and call(d) == cc.ERR_STATE and untouched()
    cc.configure(pkg, emul, case, g)
    for fn in (f, d):
        assert call(fn, "null") == cc.ERR_ARG and "null" in last()
        for k in ("txy", "cu", "res"):
            assert call(fn, **{k: None}) == cc.ERR_ARG and "null" in last(), k
        assert call(fn, pkg.make_collide_in(**dict(kw, tree_data=None), num_tree_data=cc.TABLE, **sc)) == cc.ERR_ARG and "null" in last()
        assert call(fn, pkg.make_collide_in(**kw, num_tree_data=cc.TABLE + 1, **sc)) == cc.ERR_ARG and "num_shared_trees" in last()
        twice = txy.copy()
        twice[1] = twice[0]
        assert call(fn, txy=p(twice)) == cc.ERR_ARG and "twice" in last()
        assert untouched()
        assert call(fn, nq=0, cu=None, res=None) == 0 and untouched()
        # the tile output is optional; the stats and a tree_depth_scale are not read
        r2 = np.full(len(cubes), 3, np.uint8)
        assert call(fn, pkg.make_collide_in(**dict(kw, stats=None), **dict(sc, tree_depth_scale=0.0)), res=p(r2), tile=None) == 0 and r2.tolist() == cres.tolist() and untouched()
    assert call(d, cu=p(cubes) + 2) == cc.ERR_ARG and "aligned" in last() and call(d, tile=p(tile) + 2) == cc.ERR_ARG and "aligned" in last() and untouched()


def test_wave_form_host_program(tmp_path):
    """tests/collide_wave_check.cpp: the kernel's scheme -- 64 records a round, the lowest hit of the ballot, resume behind it -- written for the host over the bodies
    of terra_collide.hpp, compiled under -fsanitize=address,undefined, against the literal loop on random tiles with dense overlaps and on out-of-range inputs"""
    exe = str(tmp_path / "collide_wave_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "collide_wave_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)"), r.stdout + r.stderr


def test_resident_chain(pkg, emul, orc):
    """the chain of test_gpu_collide.py::test_resident_chain on the emulator's "device" memory"""
    cc.run_resident_chain(pkg, emul, orc)
