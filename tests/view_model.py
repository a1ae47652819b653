"""The one NumPy / Python restatement of the primitives every pass model shares, written from the reference statements (not from the library's bodies):

    pos_dir_up: constructor, orthogonalize_up_dir, behind_sphere_mult,
      point_visible_test, sphere_visible_test, check_clip_plane,
      pt_set_visible<8>, cube_visible, cube_completely_visible               src/visibility.cpp:67-103, 119-128, 141-174, 186-196
    cube_visible_likely                                                      src/3DWorld.h:724
    cube_t::closest_pt, closest_pt_dist_sq, dist_less_than, p2p_dist_sq      src/3DWorld.h:591, 636-641; src/csg.cpp:244-246; src/inlines.h:176-192
    orthogonalize_dir, cross_product, dot_product, pointT::normalize         src/inlines.h:153-157, 220-222, 265-268; src/3DWorld.h:273-279
    InvSqrt                                                                  src/inlines.h:39-50
    do_line_clip / TEST_CLIP_T, get_region                                   src/Math3d.cpp:1029-1034, 1070-1086; src/inlines.h:522-528
    int(float), unsigned(float), int(double), unsigned(double)               as the reference's x86-64 build converts them (cvttss2si / cvttsd2si)

These are what tests/test_primitives_host.py pins to the reference's compiled code (tests/golden/primitive_vectors.npz).  The pass models import them from here
and keep no body of their own: a module-level alias at the most, and test_no_model_keeps_a_copy checks that such a name is this module's object.

Types: np.float32 for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are double: A*tterm (A is a double member; narrowed
by atanf's parameter), 1.0/d in normalize (narrowed to the float m), the whole of behind_sphere_mult but tterm, and do_line_clip's comparison of tmin with
1.0 - TOLERANCE.  Everything else is float: dot products are x*x + y*y + z*z left to right.  tanf / sinf / atanf are the C library's, called through ctypes.

A tally counts what a test decided.  The passes' tallies differ in what they keep: a test here counts a key only in a tally that has it (a defaultdict has all)."""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
PI = f32(3.141592654)
TOLERANCE = f32(1.0E-12)  # src/3DWorld.h:50
HALF = f32(0.5)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("tanf", "sinf", "atanf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def _count(tally, key):
    if tally is not None:
        try:
            tally[key] += 1
        except KeyError:  # this pass's tally does not keep the key
            pass


# ---- vectors
def cmax(a, b):  # std::max
    return b if a < b else a


def cmin(a, b):  # std::min
    return a if not (b < a) else b


def dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def cross(a, b):
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def sub(a, b):
    return [f32(a[0] - b[0]), f32(a[1] - b[1]), f32(a[2] - b[2])]


def mag_sq(a):
    return dot(a, a)


def p2p_dist_sq(a, b):
    return mag_sq(sub(a, b))


# ---- the conversions of the reference's x86-64 build: NaN and what does not fit give INT_MIN (to int) or 0 (to unsigned, through 64 bits)
def f2i(x):
    x = float(f32(x))
    return int(x) if -2147483648.0 <= x < 2147483648.0 else -2 ** 31


def d2i(x):
    x = float(x)
    return int(x) if -2147483649.0 < x < 2147483648.0 else -2 ** 31


def f2u(v):
    """cvttss2si to 64 bits, the low word"""
    v = float(v)
    if not (-9.2e18 < v < 9.2e18):
        return 0
    return int(v) & 0xFFFFFFFF


def d2u(d):
    """cvttsd2si to 64 bits, the low word"""
    d = float(d)
    if not (-9223372036854775808.0 < d < 9223372036854775808.0):
        return 0
    return int(d) & 0xFFFFFFFF


def inv_sqrt(x):
    """InvSqrt: tmp.i = 0x5f3759df - (tmp.i >> 1); y*(1.5f - 0.5f*x*y*y)"""
    x = f32(x)
    i = int(np.array([x], f32).view(np.int32)[0])
    y = np.array([(0x5f3759df - (i >> 1)) & 0xFFFFFFFF], np.uint32).view(f32)[0]
    with np.errstate(all="ignore"):
        return f32(y * f32(f32(1.5) - f32(f32(f32(HALF * x) * y) * y)))


# ---- pos_dir_up
class View:
    """pos_dir_up: pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid"""

    def __init__(self, pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid=1):
        self.pos, self.dir, self.upv_, self.cp = [f32(v) for v in pos], [f32(v) for v in dir], [f32(v) for v in upv_], [f32(v) for v in cp]
        self.sterm, self.x_sterm, self.near_, self.far_, self.valid = f32(sterm), f32(x_sterm), f32(near_), f32(far_), int(valid)

    def words(self):
        return np.array(self.pos + self.dir + self.upv_ + self.cp + [self.sterm, self.x_sterm, self.near_, self.far_], f32).tobytes() + np.int32(self.valid).tobytes()


def make_view(pos, dir, up, angle, aspect, near, far):
    """the constructor (:67-85) and orthogonalize_up_dir (:87-92); None where it asserts"""
    pos, dir, up = [f32(v) for v in pos], [f32(v) for v in dir], [f32(v) for v in up]
    angle, near, far = f32(angle), f32(near), f32(far)
    if not (near >= 0.0 and far > 0.0 and far > near):
        return None
    if dir[0] == 0.0 and dir[1] == 0.0 and dir[2] == 0.0:
        return None
    A = float(f32(aspect))
    tterm, sterm = f32(_libm.tanf(angle)), f32(_libm.sinf(angle))
    if A == 1.0:
        x_sterm = sterm
    else:
        if not (tterm > 0.0):
            return None
        atan_val = f32(_libm.atanf(f32(A * float(tterm))))
        if atan_val < 0.0:
            atan_val = f32(atan_val + PI)
        x_sterm = f32(f32(atan_val / angle) * sterm)
    upv_ = cross(dir, cross(up, dir))  # orthogonalize_dir(upv, dir, upv_, 1)
    d = f32(np.sqrt(mag_sq(upv_)))
    if d >= TOLERANCE:
        m = f32(1.0 / float(d))
        upv_ = [f32(v * m) for v in upv_]
    return View(pos, dir, upv_, cross(dir, upv_), sterm, x_sterm, near, far, 1)


def behind_sphere_mult(angle, aspect):
    """max(1.0, A*A)*max(1.0, 2.0f/((double)tterm*tterm*(1.0 + A*A))) narrowed into the float member (src/visibility.cpp:83)"""
    A = np.float64(f32(aspect))
    tterm = np.float64(f32(_libm.tanf(f32(angle))))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.float64(2.0) / (tterm * tterm * (1.0 + A * A))
        a = A * A if 1.0 < A * A else np.float64(1.0)
        b = q if 1.0 < q else np.float64(1.0)
        return f32(a * b)


def point_visible_test(v, p):
    if not v.valid:
        return True
    pv = sub(p, v.pos)
    if dot(v.dir, pv) < 0.0:
        return False
    dist = f32(np.sqrt(mag_sq(pv)))
    if abs(dot(v.upv_, pv)) > f32(dist * v.sterm):
        return False
    if abs(dot(v.cp, pv)) > f32(dist * v.x_sterm):
        return False
    return bool(dist > v.near_ and dist < v.far_)


def sphere_visible_test(v, bsm, pos, radius, tally=None):
    """with a tally of which plane decided for a sphere whose centre lies beyond it"""
    radius = f32(radius)
    if not v.valid:
        _count(tally, "invalid_view_tests")
        return bool(radius >= 0.0)
    pv = sub(pos, v.pos)
    if dot(v.dir, pv) < 0.0:
        r = bool(radius > 0.0 and mag_sq(pv) < f32(f32(radius * radius) * bsm))
        if radius > 0.0:
            _count(tally, "behind_true" if r else "behind_false")
        return r
    dist = f32(np.sqrt(mag_sq(pv)))
    du, dc = abs(dot(v.upv_, pv)), abs(dot(v.cp, pv))
    if du > f32(f32(dist * v.sterm) + radius):
        _count(tally, "up_reject")
        return False
    if radius > 0.0 and du > f32(dist * v.sterm):
        _count(tally, "up_straddle")
    if dc > f32(f32(dist * v.x_sterm) + radius):
        _count(tally, "side_reject")
        return False
    if radius > 0.0 and dc > f32(dist * v.x_sterm):
        _count(tally, "side_straddle")
    near_ok, far_ok = bool(f32(dist + radius) > v.near_), bool(f32(dist - radius) < v.far_)
    if radius > 0.0:
        if not near_ok:
            _count(tally, "near_reject")
        elif dist <= v.near_:
            _count(tally, "near_straddle")
        if near_ok and not far_ok:
            _count(tally, "far_reject")
        elif near_ok and dist >= v.far_:
            _count(tally, "far_straddle")
    return near_ok and far_ok


def cube_pts(d):
    return [[d[0][i], d[1][j], d[2][k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]


def cube_completely_visible(v, d):
    if not v.valid:
        return True
    return all(point_visible_test(v, p) for p in cube_pts(d))


def check_clip_plane(pts, pos, n, aa, d):
    for p in pts:
        pv = sub(p, pos)
        dp = dot(n, pv)
        if (f32(-dp) if d else dp) <= 0.0 or f32(dp * dp) <= f32(aa * mag_sq(pv)):
            return True
    return False


def pt_set_visible(v, pts):
    su, sc = f32(v.sterm * v.sterm), f32(v.x_sterm * v.x_sterm)
    if not check_clip_plane(pts, v.pos, v.upv_, su, 0) or not check_clip_plane(pts, v.pos, v.upv_, su, 1):
        return False
    if not check_clip_plane(pts, v.pos, v.cp, sc, 0) or not check_clip_plane(pts, v.pos, v.cp, sc, 1):
        return False
    npass = fpass = False
    for p in pts:
        if npass and fpass:
            break
        dp = dot(v.dir, sub(p, v.pos))
        npass |= bool(dp > v.near_)
        fpass |= bool(dp < v.far_)
    return npass and fpass


def closest_pt(d, p):  # clamp_pt: min(d[i][1], max(d[i][0], pt[i]))
    return [cmin(d[i][1], cmax(d[i][0], p[i])) for i in range(3)]


def cube_visible(v, d, tally=None):
    if not v.valid:
        return True
    if not pt_set_visible(v, cube_pts(d)):
        return False
    ok = bool(p2p_dist_sq(v.pos, closest_pt(d, v.pos)) < f32(v.far_ * v.far_))  # dist_less_than(pos, c.closest_pt(pos), far_)
    if not ok:
        _count(tally, "far_dropped")
    return ok


def cube_visible_likely(v, d, tally=None):
    if not v.valid:
        return True
    if point_visible_test(v, [f32(HALF * f32(d[i][0] + d[i][1])) for i in range(3)]):  # get_cube_center()
        _count(tally, "cube_centre_visible")
        return True
    r = cube_visible(v, d)
    if r:
        _count(tally, "cube_by_corners")
    return r


# ---- the line clip, on arrays of lines: each array statement is the scalar statement it cites
def line_region(v, d):
    """get_region (src/inlines.h:522-528): low bounds with <, high bounds with >=; v: 3 arrays, d: 6 arrays"""
    r = np.zeros(len(v[0]), np.int64)
    for a in range(3):
        lo, hi = d[2 * a], d[2 * a + 1]
        r |= np.where(v[a] < lo, 1 << (2 * a), np.where(v[a] >= hi, 2 << (2 * a), 0))
    return r


def do_line_clip(v1, v2, d):
    """do_line_clip (src/Math3d.cpp:1070-1086) -> (ok, v1c, v2c); v1, v2: 3 float32 arrays, d: 6 float32 arrays"""
    r1, r2 = line_region(v1, d), line_region(v2, d)
    ok = (r1 & r2) == 0
    r3 = r1 | r2
    tmin, tmax = np.zeros(len(r1), f32), np.ones(len(r1), f32)
    dv = [v2[a] - v1[a] for a in range(3)]  # vector3d const dv(v2, v1)
    for a in range(3):
        for side in range(2):  # TEST_CLIP_T(reg, d[a][side], v1[a], dv[a], side ? -dv[a] : dv[a]) (:1029-1034)
            reg = (1 << side) << (2 * a)
            act = ok & ((r3 & reg) != 0)
            t = (d[2 * a + side] - v1[a]) / dv[a]  # float quotient
            vc = -dv[a] if side else dv[a]
            tmin = np.where(act & (vc > 0.0) & (t > tmin), t, tmin)
            tmax = np.where(act & ~(vc > 0.0) & (t < tmax), t, tmax)
            ok &= ~(act & (tmin >= tmax))
    clip = ok & (r3 != 0)
    mv2 = clip & (tmax > TOLERANCE)                          # float compare
    mv1 = clip & (tmin.astype(f64) < (1.0 - f64(TOLERANCE)))  # double compare
    v2c = [np.where(mv2, v1[a] + dv[a] * tmax, v2[a]) for a in range(3)]  # v2 first, from the original v1
    v1c = [np.where(mv1, v1[a] + dv[a] * tmin, v1[a]) for a in range(3)]
    return ok, v1c, v2c
