"""Line queries with inc_trees = 1 on a tile batch (terra_tiles_line_intersect_trees[_dev]) through the host emulator -- the driver's simple form: a logical thread
per line, the reference's loops -- against tests/line_trees_model.py, every byte of every hit record; the model against the reference's own compiled
line_intersect_trunc_cone (tests/golden/line_trees_vectors.npz); terra_atan2f.hpp against this machine's libm; the refusals with every output untouched; the shared
bodies as a stand-alone host program under -fsanitize=address,undefined.

test_model_against_fixture passes without the feature; every other test needs the feature's headers or entry points and fails without them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import line_intersect_cases as lic
import line_trees_cases as ltc
import line_trees_model as ltm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "line_trees_vectors.npz")
CASES = ltc.cases()
BY_NAME = {c.name: c for c in CASES}
f32 = np.float32
THREADS = 8


def test_model_against_fixture():
    """every row: t_set and the bits of t as the reference's compiled code returned them; a second pass of -num instead of the source's 2^32*num would not"""
    fx = np.load(FIXTURE)
    rows, t_set, t = fx["rows"], fx["t_set"], fx["t"]
    assert len(rows) >= 4000 and 0.25 <= (t_set != 0).mean() <= 0.75
    other = 0
    for i, r in enumerate(rows):
        m = ltm.trunc_cone(r[0:3], r[3:6], r[6:9], r[9:12], r[12], r[13])
        assert m[0] == t_set[i] and (not m[0] or m[1].tobytes() == t[i].tobytes()), (i, r.tolist(), m, t_set[i], t[i])
        a = ltm.trunc_cone(r[0:3], r[3:6], r[6:9], r[9:12], r[12], r[13], second=-1.0)
        other += int(a[0] != m[0] or (m[0] and a[1].tobytes() != m[1].tobytes()))
    assert other >= 100


def test_model_alone():
    """every case exercises what it is named for, on the model alone"""
    union = ltm.new_tally()
    for case in CASES:
        g, inp, hits, tally = ltc.model(case)
        assert case.check(tally, hits), (case.name, {k: x for k, x in tally.items() if x}, hits.tolist())
        for k, x in tally.items():
            union[k] += x
        for h in hits:  # a tree hit leaves xpos / ypos at 0 and names its record; everything else has tree = -1
            assert (h["hit"] == ltm.HIT_TREE) == (h["tree"] >= 0) and (h["hit"] != ltm.HIT_TREE or (h["xpos"] == 0 and h["ypos"] == 0 and h["t"] < 1.0)), (case.name, h)
            assert h["hit"] != 0 or (h["t"] == 2.0 and h["tile"] == -1 and not h["p_int"].any() and h["part"] == 0 and h["xpos"] == 0 and h["ypos"] == 0), (case.name, h)
    for k in ltm.TALLY:
        if k != "second_root":  # (the source's second pass multiplies num by 2^32: it sets t nowhere)
            assert union[k] > 0, k
    assert sum(c.dxoff != 0 for c in CASES) >= len(CASES) // 2 - 1


@pytest.fixture(scope="module")
def atan_lib(tmp_path_factory):
    """terra_atan2f.hpp for the host: tests/line_trees_atan_lib.cpp (-fno-builtin: the atanf / atan2f it compares with are libm's)"""
    so = str(tmp_path_factory.mktemp("lt_atan") / "liblt_atan.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-builtin", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "line_trees_atan_lib.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.lt_atanf_sweep.restype = lib.lt_atan2f_pairs.restype = ctypes.c_uint64
    lib.lt_atanf_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.lt_atan2f_pairs.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.lt_atan2f_eval.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    return lib


def test_atanf_every_7th_pattern(atan_lib):
    """atanf on every 7th bit pattern of all floats, both signs (6.1e8 arguments, the infinities and NaNs among them): zero mismatches (a few seconds on 8 threads)"""
    bad = ctypes.c_uint32(0)
    n = atan_lib.lt_atanf_sweep(0, 7, THREADS, ctypes.addressof(bad))
    assert n == 0, f"{n} mismatches, the first at bit pattern {bad.value:#010x}"


def test_atan2f_four_quadrants(atan_lib):
    """atan2f on 4e7 seeded pairs over the four quadrants with exponents spread so that |k| > 60 occurs: zero mismatches"""
    tally, bad = np.zeros(7, np.uint64), np.zeros(2, f32)
    n = atan_lib.lt_atan2f_pairs(20241021, 40000000, THREADS, tally.ctypes.data, bad.ctypes.data)
    assert n == 0, f"{n} mismatches, the first at y = {bad[0]!r}, x = {bad[1]!r}"
    assert tally[:4].sum() >= 39000000 and tally[:4].min() >= 9000000 and tally[4] >= 1000000 and tally[5] >= 500000 and tally[6] >= 25000000, tally.tolist()


def test_atan2f_special_cases(atan_lib):
    """+-0, +-inf, NaN, x == 1, denormals, the breakpoints of atanf and the two thresholds on k, every pairing"""
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1e-40, 1.1754944e-38, 3.4028235e38, -3.4028235e38, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25,
                   2.0 ** -29, 2.0 ** 60, 2.0 ** 61, 2.0 ** 62, 2.0 ** -60, 2.0 ** -61, 2.0 ** -62, 0.5, 1.5, 3.0, -0.3, 7.0e-10], f32)
    with np.errstate(over="ignore"):
        sp = np.concatenate([sp, np.nextafter(sp, f32(np.inf)), np.nextafter(sp, f32(-np.inf))]).astype(f32)
    y, x = (a.ravel().copy() for a in np.meshgrid(sp, sp, indexing="ij"))
    out = [np.zeros(len(y), f32) for _ in range(4)]
    atan_lib.lt_atan2f_eval(y.ctypes.data, x.ctypes.data, len(y), *[o.ctypes.data for o in out])
    for ours, libm, what in ((out[0], out[1], "atan2f"), (out[2], out[3], "atanf")):
        same = (ours.view(np.uint32) == libm.view(np.uint32)) | (np.isnan(ours) & np.isnan(libm))
        assert same.all(), (what, y[~same][:4], x[~same][:4], ours[~same][:4], libm[~same][:4])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases(pkg, emul, case):
    ltc.run_case(pkg, emul, case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_dev_entry_point(pkg, emul, case):
    """the device-pointer form on the emulator's "device" memory"""
    ltc.run_case(pkg, emul, case, dev=True)


def test_fixture_rows_through_the_entry_point(pkg, emul):
    """every 5th row of the fixture as the trunk cylinder of a pine of its own tile (the GPU test runs every row)"""
    ltc.run_fixture_rows(pkg, emul, np.load(FIXTURE), step=5)


def test_without_records_equals_the_mesh_query(pkg, emul):
    """pine == NULL, pine_counts == NULL or pine_capacity == 0: the first 32 bytes of every record are terra_tiles_line_intersect's, on the existing line cases"""
    d = lic.setup(pkg, emul, 128)
    sc, n = d["sc"], len(d["tiles"])
    rs = np.random.RandomState(5)
    lines = np.concatenate([lic.camera_rays(sc, d["tiles"], d["z"], rs, 400)] + list(lic.special_lines(sc, d, rs).values()))
    lt = np.full(len(lines), -1, np.int32)
    lt[0::3] = rs.randint(n, size=len(lt[0::3]))
    distant = ((np.arange(n) % 4) == 1).astype(np.uint8)
    rec = ltc.trc.Records(n, 4)
    for kw in (dict(), dict(pine=rec.pine), dict(pine_counts=rec.counts), dict(pine=rec.pine, pine_counts=rec.counts, pine_capacity=0)):
        for line_tile, dist in ((None, None), (lt, distant)):
            want = emul.tiles_line_intersect(d["tiles"], d["z"], d["stats"], lines, line_tile, 0, 0, dist)
            got = emul.tiles_line_intersect_trees(d["tiles"], pkg.make_line_trees_in(zvals=d["z"], stats=d["stats"], is_distant=dist, **kw), lines, line_tile)
            assert got.view(np.uint8).reshape(len(lines), 40)[:, :32].tobytes() == want.tobytes()
            assert (got["tree"] == -1).all() and (got["part"] == 0).all() and want["hit"].sum() > 300


def test_refused_and_zero(pkg, emul):
    lib, ctx = emul.lib, emul.ctx
    case = BY_NAME["parts_offset"]
    g, inp, hits, _ = ltc.model(case)
    n = len(case.tiles)
    last = lambda: lib.terra_last_error().decode()  # noqa: E731
    p = lambda x: x.ctypes.data  # noqa: E731
    txy = np.array(case.tiles, np.int32)
    lines = inp.line_array()
    out = np.full(len(lines) * 10, 3, np.uint32)
    untouched = lambda: (out == 3).all()  # noqa: E731
    kw, sc = ltc.host_arrays(pkg, case, inp), ltc.scalars(case)
    f, d = lib.terra_tiles_line_intersect_trees, lib.terra_tiles_line_intersect_trees_dev

    def call(fn, lin=None, **k):
        lin = pkg.make_line_trees_in(**kw, **sc) if lin is None else lin
        return fn(ctx, k.get("txy", p(txy)), k.get("n", n), ctypes.byref(lin) if lin != "null" else None, k.get("ln", p(lines)), k.get("lt", None), k.get("nl", len(lines)),
                  k.get("out", p(out)))
    assert call(f) == ltc.ERR_STATE and call(d) == ltc.ERR_STATE and untouched()
    ltc.configure(pkg, emul, case, g)
    for fn in (f, d):
        assert call(fn, "null") == ltc.ERR_ARG and "null" in last()
        for k in ("txy", "ln", "out"):
            assert call(fn, **{k: None}) == ltc.ERR_ARG and "null" in last(), k
        for k in ("zvals", "stats"):
            assert call(fn, pkg.make_line_trees_in(**dict(kw, **{k: None}), **sc)) == ltc.ERR_ARG and "null" in last(), k
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(fn, pkg.make_line_trees_in(**kw, **dict(sc, tree_depth_scale=bad))) == ltc.ERR_ARG and "tree_depth_scale" in last()
        assert call(fn, pkg.make_line_trees_in(**kw, pine_capacity=2 ** 31, **sc), n=2) == ltc.ERR_ARG and "32 bits" in last()
        assert untouched()
        # nlines == 0 does nothing once the checks have passed; n == 0 writes misses
        assert call(fn, nl=0, ln=None, out=None) == 0 and untouched()
        assert call(fn, pkg.make_line_trees_in(**kw, **dict(sc, tree_depth_scale=-1.0)), nl=0) == ltc.ERR_ARG
        got = np.full(len(lines), 3, pkg.LINE_TREE_HIT_DTYPE)
        assert call(fn, pkg.make_line_trees_in(**sc), n=0, txy=None, out=p(got)) == 0
        assert (got["t"] == 2.0).all() and (got["tile"] == -1).all() and (got["tree"] == -1).all() and not got["hit"].any() and not got["part"].any() and not got["p_int"].any()
    # the host form reads line_tile up front
    lt = np.full(len(lines), -1, np.int32)
    lt[1] = n
    assert call(f, lt=p(lt)) == ltc.ERR_ARG and "line_tile" in last() and untouched()
    # a misaligned pointer (the device form; the host form stages its arrays)
    assert call(d, ln=p(lines) + 2) == ltc.ERR_ARG and "aligned" in last() and call(d, out=p(out) + 1) == ltc.ERR_ARG and "aligned" in last()
    assert call(d, pkg.make_line_trees_in(**dict(kw, pine_counts=p(inp.rec.counts) + 2), pine_capacity=8, **sc)) == ltc.ERR_ARG and "aligned" in last() and untouched()
    # instanced with a table of another length
    emul.set_tree_params(pkg.make_tree_params(tree_mode=3, instanced=1, num_pine_insts=5, num_palm_insts=5))
    assert call(f) == ltc.ERR_ARG and "instances" in last() and call(d) == ltc.ERR_ARG and untouched()
    # an unsupported tile size
    emul.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=66))
    assert call(f) == ltc.ERR_ARG and call(d) == ltc.ERR_ARG and untouched()


def test_shared_bodies_host_program(tmp_path):
    """tests/line_trees_check.cpp: line_trunc_cone over the fixture's rows and the kernel's order-free reduction against the literal loop, under
    -fsanitize=address,undefined"""
    fx = np.load(FIXTURE)
    raw = str(tmp_path / "rows.bin")
    with open(raw, "wb") as fh:
        fh.write(np.int32(len(fx["rows"])).tobytes() + fx["rows"].astype(f32).tobytes() + fx["t_set"].astype(np.int32).tobytes() + fx["t"].astype(f32).tobytes())
    exe = str(tmp_path / "line_trees_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "line_trees_check.cpp")], check=True)
    r = subprocess.run([exe, raw], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 problems)") and f"{len(fx['rows'])} fixture rows, 0 differ" in r.stdout, r.stdout + r.stderr


def test_resident_chain(pkg, emul):
    """the chain of test_gpu_line_trees.py::test_resident_chain on the emulator's "device" memory"""
    ltc.run_resident_chain(pkg, emul)
