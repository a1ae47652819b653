"""The shared host/device primitives against the reference's own code: what tests/test_primitives_host.py, tests/test_gpu_primitives.py and the generator
tests/golden/make_primitive_golden.py have in common (TEST INFRASTRUCTURE ONLY).

tests/golden/primitive_vectors.npz holds inputs and what the reference's compiled code (oracle/_ref, oracle/ref_shim.cpp section 5) and this machine's C library
answered for them; nothing else.  Everything is compared exactly: floats bit for bit (NaN equals NaN), decisions and integers value for value.

    family            inputs                                   recorded outputs
    powf              powf_x, powf_y                           powf_out                        (libm)
    sincosf           sc_x                                     sin_out, cos_out                (libm)
    sincosf_droplet   sc_x[:sc_droplets]                       the same rows                   the form of sinf / cosf the droplets call (|x| < 120)
    camera            cam_in [C][13], cam_valid [C]            cam_out [C][19]                 pos_dir_up's constructor
    points            pt_xyz [n][3], pt_off [C+1]              pt_out                          point_visible_test
    spheres           sp_xyzr [n][4], sp_off                   sp_out                          sphere_visible_test
    cubes             cb_box [n][6], cb_sph, cb_q [n][4]       cb_out [n][5]                   cube_visible, cube_completely_visible, cube_visible_likely,
                                                                                               sphere_and_cube_visible_test, closest_dist_less_than
    inv_sqrt          isq_x                                    isq_out                         InvSqrt
    line_clip         lc_v [n][6], lc_d [n][6]                 lc_ok, lc_out [n][6]            do_line_clip
    lod               lod_dist, lod_mnz                        lod_out                         dist /= -log2(2.0*min_normal_z)
    convert_floats    cvf_x                                    cvf_u, cvf_i                    unsigned(float), int(float)
    convert_doubles   cvd_x                                    cvd_u, cvd_i                    unsigned(double), int(double)

cam_in: pos, dir, up, angle, aspect, near, far; cam_out: pos, dir, upv_, cp, sterm, x_sterm, near_, far_, behind_sphere_mult, angle, tterm.
The rows of points / spheres / cubes are grouped by camera: camera c owns rows off[c] .. off[c + 1].

One camera is built the way the engine builds camera_pdu: with an angle of 0, for which the constructor takes 0.5*TO_RADIANS*PERSP_ANGLE itself.  The reference's
build evaluates tanf of that constant at compile time, correctly rounded, where the C library's tanf is one unit off; x_sterm and behind_sphere_mult inherit it.
terra_make_view leaves that default to the engine (include/terra.h), so the constructor comparisons run on the cameras with an angle of their own (one of them the
same default half-angle, passed explicitly), and the view tests run on all of them: an engine's views are copies of camera_pdu's members.
"""
import collections
import ctypes as C
import os

import numpy as np

import view_model

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "primitive_vectors.npz")
f32 = np.float32

FAMILIES = ("powf", "sincosf", "sincosf_droplet", "points", "spheres", "cubes", "inv_sqrt", "line_clip", "lod", "convert_floats", "convert_doubles")
# the recorded outputs of each family (camera: the constructor; the libm rows are recorded by the generator, not by the reference library)
OUTPUTS = {"powf": ("powf_out",), "sincosf": ("sin_out", "cos_out"), "sincosf_droplet": ("sin_out", "cos_out"), "camera": ("cam_out",), "points": ("pt_out",), "spheres": ("sp_out",), "cubes": ("cb_out",),
           "inv_sqrt": ("isq_out",), "line_clip": ("lc_ok", "lc_out"), "lod": ("lod_out",), "convert_floats": ("cvf_u", "cvf_i"), "convert_doubles": ("cvd_u", "cvd_i")}
CUBE_COLUMNS = ("cube_visible", "cube_completely_visible", "cube_visible_likely", "sphere_and_cube_visible_test", "closest_dist_less_than")

_fixture = None


def load():
    """the fixture as a dict of arrays, read once and shared (nobody writes to them)"""
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def num_cameras(fx):
    return len(fx["cam_in"])


def rows(fx, key, c):
    """the rows of camera c in the family whose offsets are fx[key + "_off"]"""
    off = fx[key + "_off"]
    return slice(int(off[c]), int(off[c + 1]))


def assert_same(what, exp, got):
    exp, got = np.asarray(exp), np.asarray(got)
    assert exp.shape == got.shape and exp.dtype == got.dtype, (what, exp.shape, got.shape, exp.dtype, got.dtype)
    if exp.dtype.kind == "f":
        u = np.uint32 if exp.dtype == np.float32 else np.uint64
        same = (np.ascontiguousarray(exp).view(u) == np.ascontiguousarray(got).view(u)) | (np.isnan(exp) & np.isnan(got))
    else:
        same = exp == got
    if not same.all():
        idx = np.argwhere(~same)
        i = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} of {exp.size} values differ; first at {i}: expected {exp[i]!r}, got {got[i]!r}")


def count_different(exp, got):
    """rows (first axis) on which got differs from exp: what the mutation report counts"""
    exp, got = np.asarray(exp), np.asarray(got)
    if exp.dtype.kind == "f":
        u = np.uint32 if exp.dtype == np.float32 else np.uint64
        same = (np.ascontiguousarray(exp).view(u) == np.ascontiguousarray(got).view(u)) | (np.isnan(exp) & np.isnan(got))
    else:
        same = exp == got
    return int((~same.reshape(len(exp), -1).all(axis=1)).sum())


def lod_level(dist_out):
    """the level get_lod_level's loop reaches from the statement's float for a tile of 128 cells outside a reflection pass (src/tiled_mesh.cpp:1926-1929): halvings are
    exact, so this is arithmetic on the recorded float, not a second opinion on it"""
    d = np.asarray(dist_out, f32).astype(np.float64)
    lod = np.zeros(len(d), np.uint8)
    for _ in range(4):  # lod_level + 1 < NUM_LODS (5) and (128 >> (lod_level + 1)) >= 4
        more = (d > 2.0) & (lod == _)
        lod[more] += 1
        d = np.where(more, d / 2.0, d)
    return lod


# ---- the live reference (oracle/_ref): what the generator records and what the fixture is re-checked against
def eval_reference(ref, fx):
    out = {}
    ncam = num_cameras(fx)
    cam_out = np.zeros((ncam, 19), f32)
    pt, sp, cb = np.zeros(len(fx["pt_xyz"]), np.uint8), np.zeros(len(fx["sp_xyzr"]), np.uint8), np.zeros((len(fx["cb_box"]), 5), np.uint8)
    for c in range(ncam):
        ci = fx["cam_in"][c]
        r = ref.pdu_make(ci[0:3], ci[3:6], ci[6:9], float(ci[9]), float(ci[10]), float(ci[11]), float(ci[12]))
        assert r is not None, f"camera {c}: the reference's constructor would assert"
        cam_out[c] = r
        ref.pdu_set_valid(int(fx["cam_valid"][c]))
        s = rows(fx, "pt", c); pt[s] = ref.pdu_points(fx["pt_xyz"][s])
        s = rows(fx, "sp", c); sp[s] = ref.pdu_spheres(fx["sp_xyzr"][s])
        s = rows(fx, "cb", c); cb[s] = ref.pdu_cubes(fx["cb_box"][s], fx["cb_sph"][s], fx["cb_q"][s])
    out["cam_out"], out["pt_out"], out["sp_out"], out["cb_out"] = cam_out, pt, sp, cb
    out["isq_out"] = ref.inv_sqrt(fx["isq_x"])
    out["lc_ok"], out["lc_out"] = ref.do_line_clip(fx["lc_v"], fx["lc_d"])
    out["lod_out"] = ref.lod_steep_dist(fx["lod_dist"], fx["lod_mnz"])
    out["cvf_u"], out["cvf_i"] = ref.convert_floats(fx["cvf_x"])
    out["cvd_u"], out["cvd_i"] = ref.convert_doubles(fx["cvd_x"])
    return out


def eval_libm(fx):
    """powf / sinf / cosf of this machine's C library (the one the reference binary links)"""
    import ctypes.util
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.powf.restype = m.sinf.restype = m.cosf.restype = C.c_float
    m.powf.argtypes = [C.c_float, C.c_float]
    m.sinf.argtypes = m.cosf.argtypes = [C.c_float]
    return {"powf_out": np.array([m.powf(float(x), float(y)) for x, y in zip(fx["powf_x"], fx["powf_y"])], f32),
            "sin_out": np.array([m.sinf(float(x)) for x in fx["sc_x"]], f32), "cos_out": np.array([m.cosf(float(x)) for x in fx["sc_x"]], f32)}


# ---- the probe (tests/devprobe): either build behind the same entry points
class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        vp, u32, i32, fl = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
        for name, args in (("powf", [vp, vp, u32, vp]), ("sincosf", [vp, u32, vp, vp]), ("sincosf_droplet", [vp, u32, vp, vp]), ("points", [vp, i32, vp, u32, vp]), ("spheres", [vp, i32, fl, vp, u32, vp]),
                           ("cubes", [vp, i32, fl, vp, vp, vp, u32, vp]), ("inv_sqrt", [vp, u32, vp]), ("line_clip", [vp, vp, u32, vp, vp]), ("lod", [vp, vp, u32, vp, vp]),
                           ("convert_floats", [vp, u32, vp, vp]), ("convert_doubles", [vp, u32, vp, vp])):
            fn = getattr(self.lib, "probe_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        self.lib.probe_is_device.restype = C.c_int
        self.is_device = bool(self.lib.probe_is_device())

    def call(self, name, *args):
        keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
        err = getattr(self.lib, "probe_" + name)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep])
        assert err == 0, f"probe_{name}: error {err}"


def _cam(fx, c):
    return np.ascontiguousarray(fx["cam_out"][c][:16]), int(fx["cam_valid"][c]), float(fx["cam_out"][c][16])


def eval_probe(probe, fx, family, limit=None):
    """the family's outputs from the probe, keyed like the fixture; limit: only the first `limit` rows of the family (of each camera, for the view families)"""
    cut = (lambda n: n) if limit is None else (lambda n: min(n, limit))
    if family == "powf":
        n = cut(len(fx["powf_x"])); o = np.zeros(n, f32)
        probe.call("powf", fx["powf_x"][:n], fx["powf_y"][:n], n, o)
        return {"powf_out": o}
    if family in ("sincosf", "sincosf_droplet"):
        n = cut(len(fx["sc_x"]) if family == "sincosf" else int(fx["sc_droplets"])); s, c = np.zeros(n, f32), np.zeros(n, f32)
        probe.call(family, fx["sc_x"][:n], n, s, c)
        return {"sin_out": s, "cos_out": c}
    if family in ("points", "spheres", "cubes"):
        key = {"points": "pt", "spheres": "sp", "cubes": "cb"}[family]
        parts = []
        for c in range(num_cameras(fx)):
            view, valid, bsm = _cam(fx, c)
            r = rows(fx, key, c)
            r = slice(r.start, r.start + cut(r.stop - r.start))
            n = r.stop - r.start
            if family == "points":
                o = np.zeros(n, np.uint8); probe.call("points", view, valid, fx["pt_xyz"][r], n, o)
            elif family == "spheres":
                o = np.zeros(n, np.uint8); probe.call("spheres", view, valid, bsm, fx["sp_xyzr"][r], n, o)
            else:
                o = np.zeros((n, 5), np.uint8); probe.call("cubes", view, valid, bsm, fx["cb_box"][r], fx["cb_sph"][r], fx["cb_q"][r], n, o)
            parts.append(o)
        return {key + "_out": np.concatenate(parts)}
    if family == "inv_sqrt":
        n = cut(len(fx["isq_x"])); o = np.zeros(n, f32)
        probe.call("inv_sqrt", fx["isq_x"][:n], n, o)
        return {"isq_out": o}
    if family == "line_clip":
        n = cut(len(fx["lc_v"])); ok, o = np.zeros(n, np.uint8), np.zeros((n, 6), f32)
        probe.call("line_clip", fx["lc_v"][:n], fx["lc_d"][:n], n, ok, o)
        return {"lc_ok": ok, "lc_out": o}
    if family == "lod":
        n = cut(len(fx["lod_dist"])); o, lv = np.zeros(n, f32), np.zeros(n, np.uint8)
        probe.call("lod", fx["lod_dist"][:n], fx["lod_mnz"][:n], n, o, lv)
        return {"lod_out": o, "lod_level": lv}
    if family == "convert_floats":
        n = cut(len(fx["cvf_x"])); u, s = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        probe.call("convert_floats", fx["cvf_x"][:n], n, u, s)
        return {"cvf_u": u, "cvf_i": s}
    if family == "convert_doubles":
        n = cut(len(fx["cvd_x"])); u, s = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        probe.call("convert_doubles", fx["cvd_x"][:n], n, u, s)
        return {"cvd_u": u, "cvd_i": s}
    raise KeyError(family)


def expected(fx, family, limit=None):
    """the fixture's rows that eval_probe(..., family, limit) answers for, under the same keys (lod_level: derived from lod_out, see lod_level())"""
    cut = (lambda a: a) if limit is None else (lambda a: a[:limit])
    if family in ("points", "spheres", "cubes"):
        key = {"points": "pt", "spheres": "sp", "cubes": "cb"}[family]
        return {key + "_out": np.concatenate([cut(fx[key + "_out"][rows(fx, key, c)]) for c in range(num_cameras(fx))])}
    e = {k: cut(fx[k] if family != "sincosf_droplet" else fx[k][:int(fx["sc_droplets"])]) for k in OUTPUTS[family]}
    if family == "lod":
        e["lod_level"] = lod_level(e["lod_out"])
    return e


def check_probe(probe, fx, family, limit=None):
    got, exp = eval_probe(probe, fx, family, limit), expected(fx, family, limit)
    assert set(got) == set(exp)
    for k in exp:
        assert_same(f"{family}/{k}" + ("" if limit is None else f" (first {limit})"), exp[k], got[k])
    return sum(len(v) for v in exp.values())


def constructed_cameras(fx):
    """the cameras whose angle is the caller's (see the module's header)"""
    return [c for c in range(num_cameras(fx)) if fx["cam_in"][c][9] != 0.0]


def check_abi_cameras(t, fx):
    """terra_make_view and terra_view_behind_sphere_mult of a loaded library (t: a Terra of either backend) on the fixture's cameras"""
    for c in constructed_cameras(fx):
        ci, co = fx["cam_in"][c], fx["cam_out"][c]
        angle = float(ci[9])
        assert co[17] == ci[9]
        v = t.make_view([float(x) for x in ci[0:3]], [float(x) for x in ci[3:6]], [float(x) for x in ci[6:9]], angle, float(ci[10]), float(ci[11]), float(ci[12]))
        got = np.array(list(v.pos) + list(v.dir) + list(v.upv) + list(v.cp) + [v.sterm, v.x_sterm, v.near_, v.far_], f32)
        assert_same(f"terra_make_view, camera {c}", co[:16], got)
        assert v.valid == 1
        assert_same(f"terra_view_behind_sphere_mult, camera {c}", co[16:17], np.array([t.view_behind_sphere_mult(angle, float(ci[10]))], f32))


# ---- the Python models' primitives (tests/view_model.py, and the LOD statement of tests/terrain_view_model.py) on the fixture's inputs
def model_views(fx):
    return [view_model.View(o[0:3], o[3:6], o[6:9], o[9:12], o[12], o[13], o[14], o[15], int(valid)) for o, valid in zip(fx["cam_out"], fx["cam_valid"])]


def box3(b):
    return [[f32(b[0]), f32(b[1])], [f32(b[2]), f32(b[3])], [f32(b[4]), f32(b[5])]]


def eval_models(fx):
    """-> {label: (expected, got)} for every primitive of the models that the fixture has rows for"""
    import terrain_view_model as tm
    res = {}
    views = model_views(fx)
    ncam = num_cameras(fx)
    # the constructor and behind_sphere_mult
    cams, bsm = [], []
    made = constructed_cameras(fx)
    for c in made:
        ci, co = fx["cam_in"][c], fx["cam_out"][c]
        v = view_model.make_view(ci[0:3], ci[3:6], ci[6:9], ci[9], ci[10], ci[11], ci[12])
        assert v is not None, f"camera {c}: the model refuses what the reference constructs"
        cams.append(np.array(v.pos + v.dir + v.upv_ + v.cp + [v.sterm, v.x_sterm, v.near_, v.far_], f32))
        bsm.append(view_model.behind_sphere_mult(ci[9], ci[10]))
    res["view_model.make_view"] = (fx["cam_out"][made, :16], np.array(cams, f32))
    res["view_model.behind_sphere_mult"] = (fx["cam_out"][made, 16], np.array(bsm, f32))
    pt, sp = [], []
    cv, ccv, cvl = [], [], []
    for c in range(ncam):
        v, b = views[c], f32(fx["cam_out"][c][16])
        with np.errstate(all="ignore"):
            pt += [view_model.point_visible_test(v, [f32(x) for x in p]) for p in fx["pt_xyz"][rows(fx, "pt", c)]]
        for s in fx["sp_xyzr"][rows(fx, "sp", c)]:
            pos = [f32(s[0]), f32(s[1]), f32(s[2])]
            with np.errstate(all="ignore"):
                sp.append(view_model.sphere_visible_test(v, b, pos, f32(s[3])))
        for bx in fx["cb_box"][rows(fx, "cb", c)]:
            d = box3(bx)
            with np.errstate(all="ignore"):
                cv.append(view_model.cube_visible(v, d))
                ccv.append(view_model.cube_completely_visible(v, d))
                cvl.append(view_model.cube_visible_likely(v, d, collections.defaultdict(int)))
    u8 = lambda a: np.array(a, bool).astype(np.uint8)  # noqa: E731
    res["view_model.point_visible_test"] = (fx["pt_out"], u8(pt))
    res["view_model.sphere_visible_test"] = (fx["sp_out"], u8(sp))
    res["view_model.cube_visible"] = (fx["cb_out"][:, 0], u8(cv))
    res["view_model.cube_completely_visible"] = (fx["cb_out"][:, 1], u8(ccv))
    res["view_model.cube_visible_likely"] = (fx["cb_out"][:, 2], u8(cvl))
    with np.errstate(all="ignore"):
        res["view_model.inv_sqrt"] = (fx["isq_out"], np.array([view_model.inv_sqrt(x) for x in fx["isq_x"]], f32))
        res["terrain_view_model.lod_steep_dist"] = (fx["lod_out"], np.array([tm.lod_steep_dist(d, z) for d, z in zip(fx["lod_dist"], fx["lod_mnz"])], f32))
    res["view_model.f2u"] = (fx["cvf_u"], np.array([view_model.f2u(x) for x in fx["cvf_x"]], np.uint32))
    res["view_model.f2i"] = (fx["cvf_i"], np.array([view_model.f2i(x) for x in fx["cvf_x"]], np.int32))
    res["view_model.d2u"] = (fx["cvd_u"], np.array([view_model.d2u(x) for x in fx["cvd_x"]], np.uint32))
    res["view_model.d2i"] = (fx["cvd_i"], np.array([view_model.d2i(x) for x in fx["cvd_x"]], np.int32))
    with np.errstate(all="ignore"):
        v, d = fx["lc_v"], fx["lc_d"]
        ok, v1c, v2c = view_model.do_line_clip([v[:, 0], v[:, 1], v[:, 2]], [v[:, 3], v[:, 4], v[:, 5]], [d[:, k] for k in range(6)])
    res["view_model.do_line_clip (ok)"] = (fx["lc_ok"], np.asarray(ok).astype(np.uint8))
    res["view_model.do_line_clip (ends)"] = (fx["lc_out"], np.stack([np.asarray(a, f32) for a in list(v1c) + list(v2c)], axis=1))
    return res
