"""Generate tests/golden/primitive_vectors.npz: inputs at which the shared host/device primitives can go wrong, and what the REFERENCE'S OWN compiled code
(oracle/_ref: visibility.cpp, Math3d.cpp, inlines.h through oracle/ref_shim.cpp section 5) and this machine's C library answer for them.  Run where the
reference tree is (it is not needed to run the tests):

    python tests/golden/make_primitive_golden.py

Every input is seeded.  The layout is described in tests/primitive_cases.py.  The generator asserts the coverage conditions -- every decision is true on at least
10 % and false on at least 10 % of its rows; in each kind of +-ulp group (side planes, near, far, behind-sphere, cube corner) the reference's answer changes inside
at least 25 % of the groups; no input makes the reference assert -- and prints the tally.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orclib  # noqa: E402
import primitive_cases as pc  # noqa: E402

f32, f64 = np.float32, np.float64
FLT_MIN, FLT_MAX = f32(1.17549435e-38), f32(3.4028234663852886e38)
DENORMALS = np.array([1.0e-45, 3.0e-45, 1.0e-42, 1.0e-40, 5.0e-39, 1.1754942e-38], f32)
STEPS = (-2, -1, 0, 1, 2)


def step(x, k):
    """x moved by k units in the last place (through zero: -0.0 and 0.0 are one value)"""
    i = np.atleast_1d(np.asarray(x, f32)).view(np.int32).astype(np.int64)
    key = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + k
    return np.where(key >= 0, key, (-key) | 0x80000000).astype(np.uint32).view(f32)


def with_neighbours(vals, k=2):
    vals = np.asarray(vals, f32)
    return np.concatenate([step(vals, j) for j in range(-k, k + 1)])


def unit(v):
    v = np.asarray(v, f64)
    return (v / np.sqrt((v * v).sum())).astype(f32)


# ---------------------------------------------------------------- libm rows
def powf_inputs(rng):
    ys = np.array([0.3, 0.5, 1.0, 1.5, 2.0, 3.0, 7.25], f32)
    xr = rng.random(4096).astype(f32)
    x = [xr, xr]
    y = [ys[np.arange(4096) % 7], (8.0 * (1.0 - rng.random(4096))).astype(f32)]  # (0, 8]
    xs = np.concatenate([[f32(0)], DENORMALS, [FLT_MIN], step(f32(1), -1), [f32(1)], step(f32(1), 1), np.array([1.25, 1.5, 2.0, 2.5, 3.0, 3.999, 4.0], f32)]).astype(f32)
    yy = np.concatenate([ys, (8.0 * (1.0 - rng.random(8))).astype(f32)])
    gx, gy = np.meshgrid(xs, yy, indexing="ij")
    x.append(gx.ravel()); y.append(gy.ravel())
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 1e-40, 3e38], f32)
    gx, gy = np.meshgrid(sp, sp, indexing="ij")
    x.append(gx.ravel()); y.append(gy.ravel())
    # denormal results: x^y = target in [2e-45, 1e-38]
    xd = (10.0 ** rng.uniform(-8.0, -5.7, 96)).astype(f32)
    target = 10.0 ** rng.uniform(np.log10(2e-45), np.log10(1e-38), 96)
    yd = (np.log(target) / np.log(xd.astype(f64))).astype(f32)
    keep = yd <= 8.0
    x.append(xd[keep]); y.append(yd[keep])
    return np.concatenate(x).astype(f32), np.concatenate(y).astype(f32)


def sincos_inputs(ref):
    TWO_PI = f32(2.0 * float(f32(3.141592654)))  # float const TWO_PI = 2.0*PI (src/3DWorld.h:43,129)
    droplets = (ref.rand_floats(11, 121, 4096) * TWO_PI).astype(f32)  # float a = rgen.rand_float()*TWO_PI (src/erosion.cpp:80-83), rgen of droplet 0 (:69)
    halfpi = np.array([k * (np.pi / 2) for k in range(1, int(120 / (np.pi / 2)) + 1)] + [np.pi / 4], f64).astype(f32)
    edge = with_neighbours(halfpi)
    parts = [droplets, np.array([0.0, -0.0], f32), DENORMALS, -DENORMALS, with_neighbours([f32(2.0 ** -12)]), -with_neighbours([f32(2.0 ** -12)]), edge, -edge,
             with_neighbours([f32(120)], 1), -with_neighbours([f32(120)], 1), np.array([10.0 ** k for k in range(3, 31)], f32), -np.array([10.0 ** k for k in range(3, 31)], f32),
             np.array([FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], f32)]
    return np.concatenate(parts).astype(f32)


# ---------------------------------------------------------------- the view family
S2, S3 = 4.0 / 3.0, 16.0 / 9.0
DEF = float(f32(0.5 * float(f32(np.pi / 180.0)) * 60.0))  # 0.5*TO_RADIANS*PERSP_ANGLE narrowed into the float member (src/visibility.cpp:72, src/3DWorld.h:117,137)
CAMERAS = [  # pos, dir, up, angle, aspect, near, far, valid
    ((0, 0, 0), (1, 0, 0), (0, 0, 1), DEF, S3, 0.0125, 100.0, 1),
    ((0, 0, 0), (0, 1, 0), (0, 0, 1), 0.2, 1.0, 0.0, 50.0, 1),
    ((3.7, -12.4, 1.3), (0, 0, -1), (0, 1, 0), 0.5, S2, 0.1, 20.0, 1),
    ((100.5, -250.25, 12.0), unit((1, 2, -0.5)), (0, 0, 1), 0.7, S3, 0.05, 200.0, 1),                 # oblique, up not orthogonal to dir
    ((-1234.5, 987.6, 55.5), unit((-3, 1, 2)), (0.3, 0.1, 1.0), 1.2, 0.5, 0.0, 1000.0, 1),           # oblique, up neither orthogonal nor of unit length
    ((5, 5, 5), (-1, 0, 0), (0, 0, 1), 1.0, 1.0, 1.0, 10.0, 1),
    ((0.5, 0.25, 2.0), unit((1, 1, 0)), (0, 0, 1), DEF, S2, 0.01, 64.0, 1),
    ((0, 0, 0), (0, 0, 1), (1, 0, 0), 0.35, 0.5, 0.0, 5.0, 1),
    ((4096, -4096, 100), unit((2, -1, -1)), unit((1, 1, 1)), 0.9, S3, 0.5, 5000.0, 1),
    ((-2, -3, -4), unit((1, -2, 3)), (0, 0, 1), 1.2, 1.0, 0.2, 30.0, 1),
    ((1.0e4, 2.0e4, 300.0), (0, -1, 0), (0, 0, 1), 0.6, S2, 0.0, 1.0e5, 1),
    ((2.03, -1.57, 0.9), unit((0.6, 0.7, -0.39)), (0, 0, 1), DEF, S3, 0.0125, 80.0, 1),               # a camera a metre above the default scene
    ((2.03, -1.57, 0.9), unit((0.6, 0.7, -0.39)), (0, 0, 1), 0.0, S3, 0.0125, 80.0, 1),               # the same as the engine builds camera_pdu: angle 0 = its default
    ((3.25, 0.5, 1.75), unit((0.2, -0.9, 0.1)), (0, 0, 1), 0.45, 1.0, 0.3, 40.0, 1),
    ((1, 2, 3), (1, 0, 0), (0, 0, 1), DEF, S3, 0.0125, 100.0, 0),                                     # valid = 0: every test answers for safety
]


class Cam:
    def __init__(self, out):
        o = out.astype(f64)
        self.pos, self.dir, self.upv, self.cp = o[0:3], o[3:6], o[6:9], o[9:12]
        self.sterm, self.x_sterm, self.near, self.far, self.bsm = o[12], o[13], o[14], o[15], o[16]
        self.f = out

    def at(self, a, b, c):
        """pos + a*dir + b*upv_ + c*cp in double, rounded"""
        return (self.pos + a * self.dir + b * self.upv + c * self.cp).astype(f32)

    def radius(self, rng, lo=0.02, hi=0.9):
        return self.near + (self.far - self.near) * rng.uniform(lo, hi)

    def plane_point(self, rng, which, sign):
        """a point of the side surface |dot(n, pv)| = |pv|*sin -- n = upv_ ('u') or cp ('c') -- built in double; -> (point, the coordinate the normal is largest in,
        the outward gradient), or None where the surface does not exist (x_sterm >= 1)"""
        for _ in range(8):
            R, t = self.radius(rng), rng.uniform(-0.8, 0.8)
            if which == "u":
                b, c, n, s = sign * R * self.sterm, t * R * min(self.x_sterm, 0.99), self.upv, self.sterm
            else:
                b, c, n, s = t * R * self.sterm, sign * R * self.x_sterm, self.cp, self.x_sterm
            a2 = R * R - b * b - c * c
            if a2 > (0.05 * R) ** 2:
                a = np.sqrt(a2)
                pv = a * self.dir + b * self.upv + c * self.cp
                return (self.pos + pv).astype(f32), int(np.argmax(np.abs(n))), sign * n - s * pv / R
        return None

    def in_cone(self, rng, spread=0.6, lo=0.02, hi=0.9):
        R = self.radius(rng, min(lo, 0.25 * hi), hi)
        b, c = rng.uniform(-spread, spread) * R * self.sterm, rng.uniform(-spread, spread) * R * min(self.x_sterm, 0.9)
        return self.at(np.sqrt(max(R * R - b * b - c * c, 0.0)), b, c)

    def around(self, rng, scale=None):
        scale = min(self.far, 300.0) if scale is None else scale
        return (self.pos + rng.uniform(-1.0, 1.0, 3) * scale).astype(f32)


class Rows:
    """the rows of one family for one camera, with the +-ulp groups among them: (kind, first row, rows)"""

    def __init__(self):
        self.rows, self.groups = [], []

    def add(self, *cols):
        self.rows.append(tuple(np.asarray(c, f32) for c in cols))

    def group(self, kind, variants):
        self.groups.append((kind, len(self.rows), len(variants)))
        for v in variants:
            self.add(*v)


def siblings(p, k):
    out = []
    for j in STEPS:
        q = p.copy(); q[k] = step(p[k], j)[0]
        out.append(q)
    return out


def dominant(v):
    return int(np.argmax(np.abs(v)))


def camera_points(cam, rng):
    r = Rows()
    for which in "uc":
        for sign in (1.0, -1.0):
            for _ in range(6):
                pp = cam.plane_point(rng, which, sign)
                if pp is not None:
                    r.group("side planes", [(q,) for q in siblings(pp[0], pp[1])])
    kd = dominant(cam.dir)
    for _ in range(2):  # exactly near_ / far_ from the camera, along dir and off it
        b = 0.0 if _ == 0 else 0.3 * cam.sterm
        for kind, R in (("near", cam.near), ("far", cam.far)):
            r.group(kind, [(q,) for q in siblings(cam.at(R * np.sqrt(1.0 - b * b), R * b, 0.0), kd)])
    for b, c in ((0.0, 0.4), (0.3, -0.2)):  # dot(dir, pv) of zero and of either sign next to it
        R = cam.radius(rng)
        r.group("dir zero", [(q,) for q in siblings(cam.at(0.0, b * R, c * R), kd)])
    r.add(cam.f[0:3])  # the camera position itself
    for big in ((1.0e18, 0.0, 0.0), (1.0e18, 1.0e18, -1.0e18), (-3.0e19, 2.0e18, 1.0e18), (0.0, 0.0, 2.0e19)):  # the squared length overflows
        r.add(np.array(big, f32)); r.add((cam.pos + 1.0e18 * cam.dir + np.array(big) * 0.1).astype(f32))
    for _ in range(36):
        r.add(cam.in_cone(rng, spread=1.1))
    for _ in range(24):
        r.add(cam.around(rng))
    return r


def msq32(p, pos):
    x, y, z = (f32(p[i]) - f32(pos[i]) for i in range(3))
    return f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))


def camera_spheres(cam, rng):
    r = Rows()
    radii = [0.0, 1.0e-6, 0.37, 2.5, 1.0e4, 3.0e19, -1.0e-6, -0.37, -2.5, -1.0e4]
    n = 0
    for _ in range(20):
        for p in (cam.in_cone(rng, spread=1.2), cam.around(rng)):
            r.add(p, radii[n % len(radii)]); n += 1
    for which in "uc":  # centres on the side surfaces: the radius decides, or nothing does
        for sign in (1.0, -1.0):
            for _ in range(2):
                pp = cam.plane_point(rng, which, sign)
                if pp is not None:
                    R = np.sqrt(((pp[0].astype(f64) - cam.pos) ** 2).sum())
                    for rad in (0.0, 1.0e-7 * R, -1.0e-7 * R, 0.01 * R):
                        r.add(pp[0], rad)
    # behind the camera with the squared distance at radius^2*behind_sphere_mult: the radius is found that the float test changes its answer at
    bsm = f32(cam.bsm)
    for _ in range(6):
        R = rng.uniform(0.5, 40.0)
        p = cam.at(-R * rng.uniform(0.3, 1.0), R * rng.uniform(-0.5, 0.5), R * rng.uniform(-0.5, 0.5))
        m = msq32(p, cam.f[0:3])
        rad = f32(np.sqrt(float(m) / float(bsm)))
        T = lambda q: f32(f32(q * q) * bsm)  # noqa: E731
        with np.errstate(over="ignore"):
            while m < T(rad):
                rad = step(rad, -1)[0]
            while not (m < T(step(rad, 1)[0])):
                rad = step(rad, 1)[0]
        r.group("behind-sphere", [(p, step(rad, j)[0]) for j in (-1, 0, 1, 2)])  # rad: the last radius the test is false at
    r.add(cam.f[0:3], 0.0); r.add(cam.f[0:3], 1.0); r.add(cam.f[0:3], -1.0)
    r.add(np.array((1.0e18, 1.0e18, 1.0e18), f32), 1.0e18); r.add((cam.pos - 1.0e18 * cam.dir).astype(f32), 3.0e19); r.add((cam.pos - 1.0e18 * cam.dir).astype(f32), 1.0e30)
    for rad in (0.25, 3.0):  # touching the near and the far shell from outside
        for j in (-1, 0, 1):
            if cam.near > 0.0:
                r.add(cam.at(max(cam.near - rad, -cam.near), 0.0, 0.0), step(f32(rad), j)[0])
            r.add(cam.at(cam.far + rad, 0.0, 0.0), step(f32(rad), j)[0])
    return r


def box_from(p, ext):
    """the box from corner p to p + ext (ext of either sign per axis) as x1 x2 y1 y2 z1 z2"""
    p = np.asarray(p, f32); q = (p.astype(f64) + ext).astype(f32)
    return np.array([min(p[0], q[0]), max(p[0], q[0]), min(p[1], q[1]), max(p[1], q[1]), min(p[2], q[2]), max(p[2], q[2])], f32)


def centred(c, h):
    c = np.asarray(c, f64); h = np.asarray(h, f64) * np.ones(3)
    return np.array([c[0] - h[0], c[0] + h[0], c[1] - h[1], c[1] + h[1], c[2] - h[2], c[2] + h[2]], f32)


def camera_cubes(cam, rng):
    r = Rows()
    boxes = Rows()
    for h in (0.1, 10.0, 1.0e6):  # around the camera; huge and straddling
        boxes.add(centred(cam.pos, h))
    boxes.add(centred(cam.pos + 3.0 * cam.dir, (1.0e6, 0.5, 0.5))); boxes.add(np.array([-1e18, 1e18, -1e18, 1e18, -1e18, 1e18], f32))
    boxes.add(np.array([-3e19, 3e19, -1.0, 1.0, -3e19, 3e19], f32))
    for which in "uc":  # one corner on a side surface, the other seven beyond it
        for sign in (1.0, -1.0):
            for _ in range(4):
                pp = cam.plane_point(rng, which, sign)
                if pp is None:
                    continue
                R = np.sqrt(((pp[0].astype(f64) - cam.pos) ** 2).sum())
                ext = np.where(pp[2] >= 0.0, 1.0, -1.0) * 0.01 * R
                boxes.group("cube corner", [(box_from(q, ext),) for q in siblings(pp[0], pp[1])])
    for phi in (0.0, 0.3, 0.6):  # the closest point at far_ from the camera while a corner is in front of the far plane
        ang = phi * min(np.arcsin(min(cam.x_sterm, 1.0)), 1.0)
        L = cam.at(cam.far * np.cos(ang), 0.0, cam.far * np.sin(ang))
        d = L.astype(f64) - cam.pos
        ext = np.where(d >= 0.0, 1.0, -1.0) * 0.05 * cam.far
        boxes.group("far", [(box_from(q, ext),) for q in siblings(L, dominant(d))])
    for _ in range(3):  # zero thickness, inside the frustum and across a side surface
        c = cam.in_cone(rng, spread=0.9); h = np.array([0.5, 0.5, 0.5]) * 0.05 * cam.far; h[_] = 0.0
        boxes.add(centred(c, h))
    for s in (0.5, 5.0, 50.0):  # all eight corners behind
        boxes.add(centred(cam.pos - (2.5 * s) * cam.dir, s))
    # the default scene (S = 128, X_SCENE_SIZE = 4): DX_VAL = 1/16, grass blocks of 4 cells, tiles of 128
    DX = 0.0625
    for _ in range(28):
        c = cam.in_cone(rng, spread=1.15, hi=min(0.9, 12.0 / cam.far)) if _ % 4 else cam.around(rng, 6.0)
        x1, y1 = np.floor(c[0] / (4 * DX)) * 4 * DX, np.floor(c[1] / (4 * DX)) * 4 * DX
        z = float(c[2]) + rng.uniform(-0.05, 0.05)
        boxes.add(np.array([x1, x1 + 4 * DX, y1, y1 + 4 * DX, z, z + rng.uniform(0.0, 0.1) + 0.02], f32))
    for _ in range(14):
        c = cam.in_cone(rng, spread=1.3, hi=min(0.9, 60.0 / cam.far)) if _ % 3 else cam.around(rng, 20.0)
        x1, y1 = np.floor(c[0] / 8.0) * 8.0, np.floor(c[1] / 8.0) * 8.0
        z = float(c[2]) + rng.uniform(-1.0, 0.5)
        boxes.add(np.array([x1, x1 + 8.0, y1, y1 + 8.0, z, z + rng.uniform(0.2, 1.5)], f32))
    for _ in range(24):  # small boxes well inside: completely visible
        c = cam.in_cone(rng, spread=0.5, lo=0.1, hi=0.8)
        R = np.sqrt(((c.astype(f64) - cam.pos) ** 2).sum())
        boxes.add(centred(c, rng.uniform(0.002, 0.03, 3) * R))
    # the sphere of sphere_and_cube_visible_test and the point / distance of closest_dist_less_than for every box
    for i, (b,) in enumerate(boxes.rows):
        bd = b.astype(f64)
        with np.errstate(over="ignore", invalid="ignore"):
            ctr = (0.5 * (b[0::2] + b[1::2])).astype(f32)
            half_diag = 0.5 * np.sqrt(((bd[1::2] - bd[0::2]) ** 2).sum())
            sph = np.concatenate([ctr, [f32(min(half_diag * rng.uniform(0.3, 1.2), 3.0e38))]]).astype(f32)
            q = cam.f[0:3] if i % 3 else cam.around(rng, 10.0)
            cl = np.minimum(b[1::2], np.maximum(b[0::2], q))
            dsq = msq32(cl, q)
            d0 = f32(np.sqrt(float(dsq))) if np.isfinite(dsq) else f32(1.0e18)
        dist = step(d0, (i % 5) - 2)[0] if d0 > 0 else f32((i % 5) * 0.25)
        r.add(b, sph, np.concatenate([q, [dist]]).astype(f32))
    r.groups = boxes.groups
    return r


def stack(rows_list, col):
    return np.stack([row[col] for rows in rows_list for row in rows.rows]).astype(f32)


def offsets(rows_list):
    return np.concatenate([[0], np.cumsum([len(r.rows) for r in rows_list])]).astype(np.int32)


# ---------------------------------------------------------------- the rest
def conversion_inputs():
    p = np.array([2.0 ** k for k in range(-2, 66)], f64)
    pf = p.astype(f32)
    xf = np.concatenate([step(pf, -1), pf, step(pf, 1)])
    xf = np.concatenate([xf, -xf, np.array([0.0, -0.0, 0.5, -0.5, 0.99999994, 255.5, -255.5, np.nan, np.inf, -np.inf], f32)]).astype(f32)
    xd = np.concatenate([np.nextafter(p, 0.0), p, np.nextafter(p, np.inf)])
    extra = [2.0 ** 31 - 1, 2.0 ** 31 + 1, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5, 2.0 ** 32 - 1, 2.0 ** 32 + 1, 4294967295.5, 0.5, 2.0 ** 63 - 1024, 1.0e300, 1.0e-300, 0.0]
    xd = np.concatenate([xd, -xd, np.array(extra, f64), -np.array(extra, f64), np.array([np.nan, np.inf, -np.inf], f64)])
    return xf, xd


def inv_sqrt_inputs(rng):
    return np.concatenate([(10.0 ** rng.uniform(-30.0, 30.0, 4096)).astype(f32), [FLT_MIN], DENORMALS, np.array([4.0 ** k for k in range(-60, 61)], f32)]).astype(f32)


def lod_inputs(rng):
    special = np.concatenate([np.array([2.0 ** -k for k in range(3, 21)], f32), step(f32(0.25), -1), [FLT_MIN]]).astype(f32)
    rand = (0.25 * (1.0 - rng.random(2048))).astype(f32)
    rand = rand[(rand > 0) & (rand < 0.25)]
    dist, mnz = [], []
    for i, z in enumerate(np.concatenate([special, rand])):
        L = -np.log2(2.0 * float(z))
        ts = (2.0, 4.0, 8.0, 16.0) if i < len(special) else ((2.0, 4.0, 8.0, 16.0)[i % 4],)
        ds = [f32(10.0 ** rng.uniform(-2.0, np.log10(50.0)))] + ([f32(0.01), f32(50.0)] if i < len(special) else [])
        for t in ts:  # where the loop's threshold falls: the level changes with the last bit of the statement's result
            d = f32(t * L)
            if 0.01 <= d <= 50.0:
                ds += [step(d, -1)[0], d, step(d, 1)[0]]
        dist += ds; mnz += [z] * len(ds)
    return np.array(dist, f32), np.array(mnz, f32)


def line_clip_inputs(rng):
    v, d = [], []
    boxes = [np.array([-1, 1, -1, 1, -1, 1], f32), np.array([0.0, 8.0, -8.0, 0.0, -0.25, 1.5], f32), np.array([100.125, 100.375, -3.5, -3.25, 0.1, 0.12], f32)]
    boxes += [np.sort(rng.uniform(-50, 50, (3, 2)), axis=1).ravel().astype(f32) for _ in range(5)]

    def at(b, u):  # u in box units: 0 .. 1 inside
        return np.array([b[2 * k] + (b[2 * k + 1] - b[2 * k]) * u[k] for k in range(3)], f32)

    for b in boxes:
        add = lambda p, q: (v.append(np.concatenate([p, q]).astype(f32)), d.append(b))  # noqa: E731
        for _ in range(12):  # inside
            add(at(b, rng.uniform(0.05, 0.95, 3)), at(b, rng.uniform(0.05, 0.95, 3)))
        for k in range(3):
            for side in (0, 1):
                for _ in range(4):
                    u1 = rng.uniform(0.1, 0.9, 3); u1[k] = -0.5 - rng.random() if side == 0 else 1.5 + rng.random()
                    add(at(b, u1), at(b, rng.uniform(0.1, 0.9, 3)))                       # from one region to the inside, and back
                    add(at(b, rng.uniform(0.1, 0.9, 3)), at(b, u1))
                    u2 = rng.uniform(-0.5, 1.5, 3); u2[k] = 2.0 - u1[k]
                    add(at(b, u1), at(b, u2))                                             # through, to the opposite region
                    u3 = u1.copy(); u3[(k + 1) % 3] = rng.uniform(-1, 2)
                    add(at(b, u1), at(b, u3))                                             # both ends in the same region
                e = at(b, rng.uniform(0.1, 0.9, 3)); e[k] = b[2 * k + side]               # ending exactly on a face, from inside and from outside
                add(at(b, rng.uniform(0.1, 0.9, 3)), e)
                u1 = rng.uniform(0.1, 0.9, 3); u1[k] = -1.0 if side == 0 else 2.0
                add(at(b, u1), e); add(e, at(b, u1))
                o = at(b, u1)                                                             # parallel to the face pair (a delta of zero), outside and inside the slab
                p2 = o.copy(); p2[(k + 1) % 3] = at(b, [2.0, 2.0, 2.0])[(k + 1) % 3]
                add(o, p2)
                i1 = at(b, [0.5, 0.5, 0.5]); i1[(k + 1) % 3] = at(b, [-1.0] * 3)[(k + 1) % 3]
                i2 = i1.copy(); i2[(k + 1) % 3] = at(b, [2.0] * 3)[(k + 1) % 3]
                add(i1, i2)
        for u in (rng.uniform(0.1, 0.9, 3), np.array([-0.5, 0.5, 0.5]), np.array([0.5, 2.0, 0.5]), np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0])):  # zero length
            add(at(b, u), at(b, u))
        for _ in range(40):  # anywhere around
            add(at(b, rng.uniform(-1.5, 2.5, 3)), at(b, rng.uniform(-1.5, 2.5, 3)))
    return np.stack(v).astype(f32), np.stack(d).astype(f32)


# ---------------------------------------------------------------- the tally and the conditions
def share(name, a, tally):
    a = np.asarray(a).astype(bool)
    t = a.mean()
    tally.append(f"  {name:32s} {len(a):6d} rows, true {100 * t:5.1f} %, false {100 * (1 - t):5.1f} %")
    assert 0.1 <= t <= 0.9, f"{name}: true on {100 * t:.1f} % of its rows"


def flips(name, rows_list, offs, out, tally, column_name=""):
    by_kind = {}
    for c, rows in enumerate(rows_list):
        for kind, first, n in rows.groups:
            o = out[offs[c] + first: offs[c] + first + n]
            f = by_kind.setdefault(kind, [0, 0])
            f[0] += 1; f[1] += int(o.min() != o.max())
    for kind, (n, f) in by_kind.items():
        tally.append(f"  {name + ' ' + column_name:32s} {kind:14s} {n:4d} groups, the answer changes inside {f:4d} ({100 * f / n:5.1f} %)")
        if kind != "dir zero":  # (the plane through the camera is not a boundary of point_visible_test on its own: reported only)
            assert f >= 0.25 * n, f"{name} {kind}: the answer changes inside {f} of {n} groups"


def main():
    orclib.build_oracle()
    assert orclib.ref_available(), "needs the reference tree (oracle/_ref)"
    R = orclib.Checker("ref")
    rng = np.random.default_rng(20240607)
    fx = {}
    fx["powf_x"], fx["powf_y"] = powf_inputs(rng)
    fx["sc_x"], fx["sc_droplets"] = sincos_inputs(R), np.int32(4096)  # the droplet angles come first
    cam_in = np.array([list(p) + list(d) + list(u) + [a, asp, n, f] for p, d, u, a, asp, n, f, _ in CAMERAS], f32)
    fx["cam_in"], fx["cam_valid"] = cam_in, np.array([c[7] for c in CAMERAS], np.int32)
    pts, sps, cbs = [], [], []
    for c, ci in enumerate(cam_in):
        out = R.pdu_make(ci[0:3], ci[3:6], ci[6:9], float(ci[9]), float(ci[10]), float(ci[11]), float(ci[12]))
        assert out is not None, f"camera {c}: the reference's constructor would assert"
        cam = Cam(out)
        pts.append(camera_points(cam, rng)); sps.append(camera_spheres(cam, rng)); cbs.append(camera_cubes(cam, rng))
    fx["pt_xyz"], fx["pt_off"] = stack(pts, 0), offsets(pts)
    fx["sp_xyzr"], fx["sp_off"] = np.concatenate([stack(sps, 0), stack(sps, 1)[:, None]], axis=1).astype(f32), offsets(sps)
    fx["cb_box"], fx["cb_sph"], fx["cb_q"], fx["cb_off"] = stack(cbs, 0), stack(cbs, 1), stack(cbs, 2), offsets(cbs)
    fx["isq_x"] = inv_sqrt_inputs(rng)
    fx["lc_v"], fx["lc_d"] = line_clip_inputs(rng)
    fx["lod_dist"], fx["lod_mnz"] = lod_inputs(rng)
    fx["cvf_x"], fx["cvd_x"] = conversion_inputs()
    for k, a in fx.items():
        if a.dtype.kind == "f" and a.ndim and k not in ("powf_x", "powf_y", "sc_x", "cvf_x", "cvd_x", "pt_xyz", "sp_xyzr", "cb_box", "cb_sph", "cb_q"):
            assert np.isfinite(a).all(), k
    fx.update(pc.eval_reference(R, fx))
    fx.update(pc.eval_libm(fx))

    # ---- the conditions
    nrows = lambda fam: int(fx["sc_droplets"]) if fam == "sincosf_droplet" else len(fx[pc.OUTPUTS[fam][0]])  # noqa: E731
    tally = ["rows per family:"]
    for fam in ("camera",) + pc.FAMILIES:
        tally.append(f"  {fam:18s} {nrows(fam):6d}")
    tally.append("decisions:")
    valid = np.repeat(fx["cam_valid"], np.diff(fx["pt_off"])).astype(bool)
    share("point_visible_test", fx["pt_out"], tally)
    share("sphere_visible_test", fx["sp_out"], tally)
    for j, name in enumerate(pc.CUBE_COLUMNS):
        share(name, fx["cb_out"][:, j], tally)
    share("do_line_clip", fx["lc_ok"], tally)
    tally.append(f"  lod level reached from the statement: {np.bincount(pc.lod_level(fx['lod_out']), minlength=5).tolist()} rows at levels 0..4")
    tally.append("+-ulp groups:")
    flips("point_visible_test", pts, fx["pt_off"], fx["pt_out"], tally)
    flips("sphere_visible_test", sps, fx["sp_off"], fx["sp_out"], tally)
    flips("cube_visible", cbs, fx["cb_off"], fx["cb_out"][:, 0], tally)
    po = fx["powf_out"]
    den = int(((po != 0) & (np.abs(po) < FLT_MIN)).sum())
    x, y = fx["powf_x"], fx["powf_y"]
    with np.errstate(invalid="ignore"):
        odd, even = np.abs(y) % 2 == 1, (y != 0) & (np.abs(y) % 2 == 0)
    kinds = {"denormal results": den, "overflow to inf": int((np.isinf(po) & np.isfinite(x) & np.isfinite(y) & (x != 0)).sum()),
             "underflow to 0": int(((po == 0) & (x != 0) & np.isfinite(x) & np.isfinite(y)).sum()), "NaN": int(np.isnan(po).sum()),
             "negative base, odd exponent": int(((x < 0) & np.isfinite(x) & odd).sum()),
             "negative base, even exponent": int(((x < 0) & np.isfinite(x) & even).sum())}
    tally.append("powf: " + ", ".join(f"{k} {v}" for k, v in kinds.items()))
    assert den >= 32 and all(v >= 1 for v in kinds.values()), kinds
    auto = [c for c in range(len(CAMERAS)) if cam_in[c][9] == 0.0]
    assert len(auto) == 1 and fx["cam_out"][auto[0]][17] == f32(DEF), "the default half-angle"
    tally.append(f"the engine's own camera (angle 0): tterm {fx['cam_out'][auto[0]][18]!r}, x_sterm {fx['cam_out'][auto[0]][13]!r}, behind_sphere_mult {fx['cam_out'][auto[0]][16]!r}; "
                 f"the same angle passed explicitly: {fx['cam_out'][auto[0] - 1][18]!r}, {fx['cam_out'][auto[0] - 1][13]!r}, {fx['cam_out'][auto[0] - 1][16]!r}")
    assert len(CAMERAS) >= 12 and (fx["cam_valid"] == 0).sum() == 1 and valid.any()
    total = sum(nrows(f) for f in pc.FAMILIES)
    tally.append(f"total rows of the probe families: {total}")
    assert total <= 200000
    np.savez_compressed(pc.FIXTURE, **fx)
    size = os.path.getsize(pc.FIXTURE)
    tally.append(f"{os.path.relpath(pc.FIXTURE, os.path.dirname(os.path.dirname(HERE)))}: {size} bytes")
    assert size < 1000000
    print("\n".join(tally))


if __name__ == "__main__":
    main()
