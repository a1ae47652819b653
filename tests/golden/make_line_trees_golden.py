"""Generate tests/golden/line_trees_vectors.npz: rows of (p1, p2, cp1, cp2, r1, r2) with the t_set and t that the REFERENCE'S OWN compiled
line_intersect_trunc_cone(.., check_ends = 0, ..) (oracle/_ref/Math3d.o) returns for them.  Run where the reference tree is (it is not needed to run the tests):

    python tests/golden/make_line_trees_golden.py

The harness -- a dozen lines that declare the function through the reference's header and loop over the rows -- is written and compiled in a temporary directory
outside the repository and linked with the objects `make -C oracle ref` leaves in oracle/_ref/; only the .npz is kept.  Every input is seeded.

Rows (kind): 0 lines through and past pine leaf cones (r1 = 0, vertical axis, the radii and heights of small_tree_size / get_pine_tree_radius at tree_scale 1 and 4),
from the side and steeply from above; 1 lines that graze the side (num near 0); 2 lines that end on the surface (ti near 1); 3 lines through the apex (dp near 0);
4 lines through the base rim (dp near len); 5 frusta with r1 > 0 on any axis (the apex extension); 6 trunk-shaped cones.  Kinds 1 - 4 come in groups of five: the
row and its +-1, +-2 ulp neighbours in one coordinate of the line's ends.  No row makes the reference assert (r2 > 0 && r2 > r1 everywhere).

The generator asserts and prints: hits and misses are each >= 25 % of the rows; within the +-ulp groups of each kind the reference's answer changes inside >= 25 % of
the groups; tests/line_trees_model.py reproduces every row bit for bit.  It prints how often each pass of the root loop set t.  The source's second pass multiplies
num by float(1 - 2*i) with an unsigned i, that is by 2^32 and not by -1, so it can set t only where num is almost zero: the second pass does not reach 10 % of the
rows and cannot; the tally of rows at which a multiplier of -1 would have answered differently shows that the fixture pins this."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import line_trees_model as ltm  # noqa: E402
from make_primitive_golden import step  # noqa: E402

FIXTURE = os.path.join(HERE, "line_trees_vectors.npz")
f32, f64 = np.float32, np.float64
STEPS = (-2, -1, 0, 1, 2)
KINDS = ("through", "graze", "end on surface", "apex", "base rim", "frustum", "trunk")
HARNESS = r"""
#include "3DWorld.h" // (first: it renames the C library's timer_t before its own system includes)
int line_intersect_trunc_cone(point const &p1, point const &p2, point const &cp1, point const &cp2, float r1, float r2, bool check_ends, float &t, bool swap_ends);
extern "C" __attribute__((visibility("default"))) void lt_cone_rows(float const *rows, int n, int *t_set, float *t) {
	for (int i = 0; i < n; ++i) {
		float const *r = rows + 14*i;
		float tv = 0.0f;
		t_set[i] = line_intersect_trunc_cone(point(r[0], r[1], r[2]), point(r[3], r[4], r[5]), point(r[6], r[7], r[8]), point(r[9], r[10], r[11]), r[12], r[13], 0, tv, 0);
		t[i] = tv;
	}
}
"""


def build_harness(td):
    ref = os.environ.get("REF", "/root/reference")
    oref = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
    src, obj, lib = (os.path.join(td, n) for n in ("lt_harness.cpp", "lt_harness.o", "liblt_harness.so"))
    open(src, "w").write(HARNESS)
    inc = ["-I" + os.path.join(oref, "stub"), "-I" + os.path.join(ref, "src"), "-I" + os.path.join(ref, "Targa"), "-I" + os.path.join(ref, "dependencies", "glm"),
           "-I" + os.path.join(ref, "dependencies", "gli"), "-I" + os.path.join(ref, "dependencies", "glew-2.0.0", "include"),
           "-I" + os.path.join(ref, "dependencies", "freeglut-3.3.2", "include")]
    flags = ["-std=c++17", "-O3", "-fopenmp", "-fPIC", "-w", "-DGLEW_NO_GLU", "-fvisibility=hidden", "-ffunction-sections", "-fdata-sections"]  # oracle/Makefile: REFFLAGS
    subprocess.run(["g++"] + flags + inc + ["-c", src, "-o", obj], check=True)
    objs = sorted(os.path.join(oref, f) for f in os.listdir(oref) if f.endswith(".o"))
    subprocess.run(["g++", "-shared", "-fopenmp", "-Wl,--gc-sections", "-o", lib, obj] + objs, check=True)
    return ctypes.CDLL(lib)


def reference(lib, rows):
    rows = np.ascontiguousarray(rows, f32)
    t_set, t = np.zeros(len(rows), np.int32), np.zeros(len(rows), f32)
    lib.lt_cone_rows(ctypes.c_void_p(rows.ctypes.data), len(rows), ctypes.c_void_p(t_set.ctypes.data), ctypes.c_void_p(t.ctypes.data))
    return t_set, t


class Rows:
    def __init__(self):
        self.rows, self.kind, self.groups = [], [], []

    def add(self, kind, p1, p2, cp1, cp2, r1, r2):
        self.rows.append(np.concatenate([np.asarray(p1, f64), np.asarray(p2, f64), np.asarray(cp1, f64), np.asarray(cp2, f64), [r1, r2]]).astype(f32))
        self.kind.append(kind)

    def group(self, kind, p1, p2, cp1, cp2, r1, r2, cols):
        """the row and its +-ulp neighbours: the columns `cols` of the row (0 .. 5: the line's ends) move together"""
        self.groups.append((kind, len(self.rows), len(STEPS)))
        base = np.concatenate([np.asarray(p1, f64), np.asarray(p2, f64)]).astype(f32)
        for j in STEPS:
            q = base.copy()
            for c in cols:
                q[c] = step(base[c], j)[0]
            self.add(kind, q[0:3], q[3:6], cp1, cp2, r1, r2)


def pine_cone(rng):
    """apex (top), base centre, base radius of a pine's leaf cone: pos + dirh, pos + 0.35*dirh, get_pine_tree_radius"""
    ts = (1.0, 4.0)[rng.integers(2)]
    h = rng.uniform(0.06, 0.7) / ts  # height after the constructor's scales
    pos = np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(-1.0, 4.0)]) * (5.0 if rng.random() < 0.15 else 1.0)
    sh = rng.random() < 0.25  # T_SH_PINE: from pos, height0 = height
    R = 0.35 * ((1.0 if sh else 0.75) * h + 0.03 / ts)
    a, b = pos + [0, 0, h], pos + [0, 0, 0.0 if sh else 0.35 * h]
    a, b = a.astype(f32).astype(f64), b.astype(f32).astype(f64)  # the cone the reference sees
    return a, b, float(f32(R))


def trunk_cone(rng):
    ts = (1.0, 4.0)[rng.integers(2)]
    h = rng.uniform(0.06, 0.7) / ts
    w = h * rng.uniform(0.15, 0.5)
    pos = np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(-1.0, 4.0)])
    zb = pos[2] - 0.2 * w
    zbot = zb - 0.1 * (0.5 + 0.5 / ts)
    ln = 1.05 * h + (zb - zbot)
    a, b = np.array([pos[0], pos[1], zbot + ln]), np.array([pos[0], pos[1], zbot])
    return a.astype(f32).astype(f64), b.astype(f32).astype(f64), float(f32(0.14 * w * 0.8 * ln / (1.05 * h)))


def surface(a, b, R, u, phi):
    """the point of the cone at the fraction u from the apex and the angle phi; its outward normal; the unit generatrix; the horizontal tangent"""
    axis = b - a
    L = np.sqrt((axis * axis).sum())
    ez = axis / L
    ex = np.cross(ez, [1.0, 0.0, 0.0] if abs(ez[0]) < 0.9 else [0.0, 1.0, 0.0]); ex /= np.sqrt((ex * ex).sum())
    ey = np.cross(ez, ex)
    rad = np.cos(phi) * ex + np.sin(phi) * ey
    S = a + u * axis + u * R * rad
    gen = (S - a) / np.sqrt(((S - a) ** 2).sum())
    tang = np.cross(ez, rad)
    normal = np.cross(tang, gen); normal /= np.sqrt((normal * normal).sum())
    if (normal * rad).sum() < 0:
        normal = -normal
    return S, normal, gen, tang, rad


def unit(v):
    return v / np.sqrt((v * v).sum())


def dominant(v):
    return int(np.argmax(np.abs(v)))


def build(rng):
    r = Rows()
    for k in range(1400):  # through and past, from the side and steeply from above
        a, b, R = pine_cone(rng) if k % 4 else trunk_cone(rng)
        kind = 0 if k % 4 else 6
        u, phi = rng.uniform(0.05, 1.3), rng.uniform(0, 2 * np.pi)
        S, normal, gen, tang, rad = surface(a, b, R, min(u, 1.0), phi)
        target = a + u * (b - a) + rad * R * u * rng.uniform(0.0, 2.2)
        if k % 3 == 0:
            d = unit(np.array([rng.normal() * 0.3, rng.normal() * 0.3, -1.0]))  # steeply from above: inside the half angle of a wide cone
        else:
            d = unit(np.array([rng.normal(), rng.normal(), rng.normal() * 0.35]))
        L1, L2 = rng.uniform(0.3, 30.0), rng.uniform(-0.5, 30.0) if k % 5 else rng.uniform(0.001, 0.2)
        r.add(kind, target - d * L1, target + d * L2, a, b, 0.0, R)
    for k in range(160):  # grazing the side
        a, b, R = pine_cone(rng)
        S, normal, gen, tang, rad = surface(a, b, R, rng.uniform(0.15, 0.95), rng.uniform(0, 2 * np.pi))
        al = rng.uniform(-1.2, 1.2)
        d = np.cos(al) * tang + np.sin(al) * gen
        L1, L2 = rng.uniform(0.5, 20.0), rng.uniform(0.5, 20.0)
        r.group(1, S - d * L1, S + d * L2, a, b, 0.0, R, [dominant(normal)])
    for k in range(160):  # ending on the surface
        a, b, R = pine_cone(rng)
        S, normal, gen, tang, rad = surface(a, b, R, rng.uniform(0.15, 0.95), rng.uniform(0, 2 * np.pi))
        d = unit(normal + 0.5 * rng.normal() * tang + 0.3 * rng.normal() * gen)
        r.group(2, S + d * rng.uniform(0.5, 25.0), S, a, b, 0.0, R, [3 + dominant(normal)])
    for k in range(160):  # through the apex
        a, b, R = pine_cone(rng)
        d = unit(np.array([rng.normal(), rng.normal(), rng.normal() * 0.2]))
        L1, L2 = rng.uniform(0.3, 20.0), rng.uniform(0.3, 20.0)
        r.group(3, a + d * L1, a - d * L2, a, b, 0.0, R, [2, 5])
    for k in range(160):  # through the base rim
        a, b, R = pine_cone(rng)
        S, normal, gen, tang, rad = surface(a, b, R, 1.0, rng.uniform(0, 2 * np.pi))
        d = unit(rad + 0.4 * rng.normal() * tang + np.array([0.0, 0.0, rng.normal() * 0.02]))
        L1, L2 = rng.uniform(0.5, 20.0), rng.uniform(0.5, 20.0)
        r.group(4, S + d * L1, S - d * L2, a, b, 0.0, R, [2, 5])
    for k in range(500):  # frusta with r1 > 0, any axis
        cp1 = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-2, 6)])
        axis = unit(rng.normal(size=3)) * rng.uniform(0.1, 3.0)
        cp2 = cp1 + axis
        r2 = rng.uniform(0.02, 1.0)
        r1 = r2 * rng.uniform(0.05, 0.95)
        rad = unit(np.cross(axis, rng.normal(size=3)))
        u = rng.uniform(-0.3, 1.3)
        target = cp1 + u * axis + rad * (r1 + (r2 - r1) * min(max(u, 0.0), 1.0)) * rng.uniform(0.0, 2.0)
        d = unit(rng.normal(size=3))
        L1, L2 = rng.uniform(0.3, 30.0), rng.uniform(-0.5, 30.0)
        r.add(5, target - d * L1, target + d * L2, cp1, cp2, r1, r2)
    return r


def main():
    rng = np.random.default_rng(20241021)
    r = build(rng)
    rows, kind = np.stack(r.rows).astype(f32), np.array(r.kind, np.int32)
    groups = np.array(r.groups, np.int32)
    assert np.isfinite(rows).all() and (rows[:, 13] > 0).all() and (rows[:, 13] > rows[:, 12]).all(), "a row would make the reference assert"
    with tempfile.TemporaryDirectory() as td:
        assert not os.path.abspath(td).startswith(ROOT)
        t_set, t = reference(build_harness(td), rows)
    tally = [f"{len(rows)} rows: " + ", ".join(f"{KINDS[k]} {int((kind == k).sum())}" for k in range(len(KINDS)))]
    hit = t_set != 0
    tally.append(f"hits {100 * hit.mean():.1f} %, misses {100 * (1 - hit.mean()):.1f} %")
    assert 0.25 <= hit.mean() <= 0.75
    by_kind = {}
    for k, first, n in r.groups:
        o = t_set[first:first + n].astype(np.int64) * 2 ** 32 + t[first:first + n].view(np.uint32)
        f = by_kind.setdefault(k, [0, 0, 0])
        f[0] += 1; f[1] += int(o.min() != o.max()); f[2] += int(t_set[first:first + n].min() != t_set[first:first + n].max())
    for k, (n, f, fs) in sorted(by_kind.items()):
        tally.append(f"  +-ulp groups, {KINDS[k]:15s} {n:4d} groups, the answer changes inside {f:4d} ({100 * f / n:5.1f} %), t_set changes inside {fs:4d} ({100 * fs / n:5.1f} %)")
        assert fs >= 0.25 * n, f"{KINDS[k]}: t_set changes inside {fs} of {n} groups"
    # the model on every row; which pass set t; what a second pass of -num would have answered
    passes, other = [0, 0], 0
    for i, row in enumerate(rows):
        m = ltm.trunc_cone(row[0:3], row[3:6], row[6:9], row[9:12], row[12], row[13])
        assert m[0] == t_set[i] and (not m[0] or m[1].tobytes() == t[i].tobytes()), f"row {i} (kind {KINDS[kind[i]]}): reference {t_set[i]} {t[i]!r}, model {m}"
        if m[0]:
            passes[m[2]] += 1
        alt = ltm.trunc_cone(row[0:3], row[3:6], row[6:9], row[9:12], row[12], row[13], second=-1.0)
        other += int(alt[0] != m[0] or (m[0] and alt[1].tobytes() != m[1].tobytes()))
    tally.append(f"the model agrees on every row; t set by the first pass {passes[0]} times ({100 * passes[0] / hit.sum():.1f} % of the hits), by the second pass {passes[1]} times")
    tally.append(f"rows at which a second pass of -num (not 2^32*num) would answer differently: {other} ({100 * other / len(rows):.1f} %)")
    assert other >= 100, "too few rows tell the two multipliers apart"
    np.savez_compressed(FIXTURE, rows=rows, kind=kind, groups=groups, t_set=t_set, t=t)
    size = os.path.getsize(FIXTURE)
    tally.append(f"{os.path.relpath(FIXTURE, ROOT)}: {size} bytes")
    assert size < 1000000
    print("\n".join(tally))


if __name__ == "__main__":
    main()
