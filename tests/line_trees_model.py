"""NumPy / Python float32 restatement of the line query with inc_trees != 0, written from the reference statements (not from the library's bodies):

    tile_draw_t::line_intersect_mesh            src/tiled_mesh.cpp:3582-3604
    tile_t::line_intersect_mesh (inc_trees)     src/tiled_mesh.cpp:2176-2216
    small_tree_group::line_intersect (t != 0)   src/sm_tree.cpp:189-200
    small_tree::line_intersect                  src/sm_tree.cpp:854-876
    line_intersect_trunc_cone (check_ends = 0)  src/Math3d.cpp:543-593
    pointT::normalize, operator*(S, pointT<T>)  src/3DWorld.h:273-278, 343
    matrix_mult, dot_product_ptv                src/inlines.h:227-240

The mesh walk of a (line, tile) is tests/line_intersect_model.py's, a record's constructor, trunk_cylin and calc_bcube tests/tree_view_model.py's, get_radius()
tests/tree_ao_model.py's, check_line_clip tests/view_model.py's do_line_clip (its answer; the moved ends are not used).  atan2f and cosf are the C library's,
called through ctypes.  Types: np.float32 for float, Python float for double.  What is double in the cone test: m = 1.0/d of normalize(), the matrix M
(double(A[i])*A[i_], M[i][i] -= double(g)*g), the three-term sums of matrix_mult (narrowed to float), 0.35*dirh per component.  Everything else is float, sums
left to right.  `(1-2*i)*num` of the root loop has an unsigned i: its second pass multiplies by float(4294967295u) = 2^32 (trunc_cone's `second` stands for it so
that a caller can ask what -1 would have given)."""
import ctypes
import ctypes.util

import numpy as np

import line_intersect_model as lim
import tree_ao_model as tam
import tree_view_model as vm
import view_model

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)
TOLERANCE = f32(1.0E-12)
HIT_NONE, HIT_MESH, HIT_TREE = 0, 1, 2
HIT_DTYPE = np.dtype([("t", np.float32), ("tile", np.int32), ("xpos", np.int32), ("ypos", np.int32), ("p_int", np.float32, (3,)), ("hit", np.uint32), ("tree", np.int32),
                      ("part", np.uint32)])
SECOND_PASS = f32(4294967295.0)  # float(1u - 2u*1u)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = _libm.cosf.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.cosf.argtypes = [ctypes.c_float]
TALLY = ("pairs", "distant", "mesh_hits", "mesh_hides_nearer_tree", "tiles_without_trees", "gate_exit", "gate_pass", "gate_zero_area", "records", "dropped", "not_pine",
         "asserting_cylinders", "trunk_lowers", "cone_lowers", "both_lower", "t_new_not_below", "tree_hits", "tree_wins", "mesh_wins", "ties", "mesh_box_missed_tree_hit",
         "second_root", "rotated")


def new_tally():
    return {k: 0 for k in TALLY}


def atan2f(y, x):
    return f32(_libm.atan2f(ctypes.c_float(float(y)), ctypes.c_float(float(x))))


def cosf(x):
    return f32(_libm.cosf(ctypes.c_float(float(x))))


sub = view_model.sub


def mag(a):  # sqrt(x*x + y*y + z*z)
    return f32(np.sqrt(view_model.mag_sq(a)))


def trunc_cone(p1, p2, cp1, cp2, r1, r2, second=SECOND_PASS):
    """line_intersect_trunc_cone(p1, p2, cp1, cp2, r1, r2, 0, t) -> (t_set, t, the pass that set t or -1); None where the source asserts"""
    p1, p2, cp1, cp2 = ([f32(x) for x in v] for v in (p1, p2, cp1, cp2))
    r1, r2 = f32(r1), f32(r2)
    if not (r2 > 0.0 and r2 > r1):
        return None
    with np.errstate(all="ignore"):
        V = list(cp1)
        dirv = sub(cp2, cp1)  # vector3d dir(cp2, cp1)
        if r1 > 0.0:
            s = f32(r1 / f32(r2 - r1))
            V = [f32(V[k] - f32(dirv[k] * s)) for k in range(3)]  # V -= dir*(r1/(r2 - r1))
        A, D, d = sub(cp2, V), sub(p2, p1), sub(p1, V)
        amag = mag(A)
        g = cosf(atan2f(r2, amag))
        if amag >= TOLERANCE:  # normalize(): T const m(1.0/d)
            m = f32(1.0 / float(amag))
            A = [f32(a * m) for a in A]
        M = [[float(A[i]) * float(A[j]) for j in range(3)] for i in range(3)]
        for i in range(3):
            M[i][i] -= float(g) * float(g)
        mult = lambda v, i: f32(float(v[0]) * M[i][0] + float(v[1]) * M[i][1] + float(v[2]) * M[i][2])  # noqa: E731  matrix_mult
        Md, MD = [mult(d, i) for i in range(3)], [mult(D, i) for i in range(3)]
        c0 = c1 = c2 = ZERO
        for i in range(3):
            c0 = f32(c0 + f32(D[i] * MD[i]))
            c1 = f32(c1 + f32(D[i] * Md[i]))
            c2 = f32(c2 + f32(d[i] * Md[i]))
        num = f32(f32(c1 * c1) - f32(c2 * c0))
        t_set, t, which = 0, ZERO, -1
        if num >= 0.0:
            length = mag(dirv)
            num = f32(np.sqrt(num))
            for i, factor in enumerate((ONE, f32(second))):
                ti = f32(f32(f32(-c1) + f32(factor * num)) / c0)
                if ti >= 0.0 and ti <= 1.0 and (not t_set or ti < t):
                    q = [f32(f32(p1[k] + f32(D[k] * ti)) - cp1[k]) for k in range(3)]  # (p1 + D*ti) - cp1
                    dp = f32(f32(f32(A[0] * q[0]) + f32(A[1] * q[1])) + f32(A[2] * q[2]))
                    if dp >= 0.0 and dp <= length:
                        t, t_set, which = ti, 1, i
        return t_set, t, which


def tree_cylinders(g, s):
    """cylins[2] of small_tree::line_intersect as (p1, p2, r1, r2)"""
    rot = s.get_rot_dir()
    dirh = vm.scale_f(rot, s.height)  # get_rot_dir()*height
    lo = vm.add(s.pos, vm.scale_d(0.35, dirh) if s.type == vm.T_PINE else [ZERO] * 3)
    return [(s.p1, s.p2, s.r1, s.r2), (lo, vm.add(s.pos, dirh), tam.get_radius(g.p, s.type, s.height, s.width), ZERO)]


def tree_line(g, s, p1, p2, t, tally):
    """small_tree::line_intersect(p1, p2, &t) -> (coll, t, the cylinder that lowered t last)"""
    if not s.is_pine_tree():
        tally["not_pine"] += 1
        return False, t, 0
    coll, part, lowered = False, 0, 0
    for i, (c1, c2, r1, r2) in enumerate(tree_cylinders(g, s)):
        r = trunc_cone(p1, p2, c2, c1, r2, r1)  # (.., cylins[i].p2, cylins[i].p1, cylins[i].r2, cylins[i].r1, 0, t_new)
        if r is None:
            tally["asserting_cylinders"] += 1
            continue
        if r[0]:
            if r[1] < t:
                t, coll, part = r[1], True, i
                lowered += 1
                tally["trunk_lowers" if i == 0 else "cone_lowers"] += 1
                tally["second_root"] += r[2] == 1
            else:
                tally["t_new_not_below"] += 1
    tally["both_lower"] += lowered == 2
    return coll, t, part


class Tile:
    """a tile's pine container as the query sees it: the valid records, calc_bcube() over them"""

    def __init__(self, g, recs, count, ovs, tally):
        cap = len(recs)
        self.trees = [vm.SmallTree.make(g, recs[j], None if ovs is None else ovs[j]) for j in range(min(int(count), cap))]
        tally["records"] += len(self.trees)
        tally["dropped"] += sum(s is None for s in self.trees)
        tally["rotated"] += sum(s is not None and s.rotated and s.is_pine_tree() for s in self.trees)
        self.nvalid = sum(s is not None for s in self.trees)
        self.bcube = vm.calc_bcube(self.trees, vm.new_tally())

    def line_intersect(self, g, p1, p2, t, tally):
        """small_tree_group::line_intersect(p1, p2, &t) -> (coll, t, record, part)"""
        bc = self.bcube
        if any(bc[i][0] == bc[i][1] for i in range(3)):
            tally["gate_zero_area"] += 1
        else:
            d = [np.array([bc[i][j]], f32) for i in range(3) for j in range(2)]
            with np.errstate(all="ignore"):
                ok = view_model.do_line_clip([np.array([x], f32) for x in p1], [np.array([x], f32) for x in p2], d)[0][0]
            tally["gate_pass" if ok else "gate_exit"] += 1
            if not ok:
                return False, t, -1, 0
        coll, rec, part = False, -1, 0
        for j, s in enumerate(self.trees):
            if s is None:
                continue
            c, t, pt = tree_line(g, s, p1, p2, t, tally)
            if c:
                coll, rec, part = True, j, pt
        return coll, t, rec, part


def xlate_of(sc, dxoff, dyoff, poff2):
    """ptree_off.get_xlate(): ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0)"""
    w = lambda v: int(tam.wrap32(v))  # noqa: E731
    return [f32(f32(w(dxoff + poff2[0])) * sc.DX_VAL), f32(f32(w(dyoff + poff2[1])) * sc.DY_VAL), ZERO]


def batch_hits(sc, g, tile_xy, zvals, mzmin, mzmax, pine, counts, override, lines, line_tile=None, dxoff=0, dyoff=0, poff2=(0, 0), distant=None, tally=None):
    """every line against the batch -> HIT_DTYPE [nlines].  sc: line_intersect_model.Scene; g: tree_view_model.Globals; pine [n, cap] / counts [n] / override (or None:
    no records: the mesh query)"""
    tally = new_tally() if tally is None else tally
    txy = np.asarray(tile_xy, np.int64).reshape(-1, 2)
    n = len(txy)
    lines = np.asarray(lines, f32).reshape(-1, 2, 3)
    nl = len(lines)
    out = np.zeros(nl, HIT_DTYPE)
    out["t"], out["tile"], out["tree"] = 2.0, -1, -1
    if n == 0 or nl == 0:
        return out
    has_pine = pine is not None and counts is not None and pine.shape[1] > 0
    tiles = [Tile(g, pine[i], counts[i], None if override is None else override[i], tally) for i in range(n)] if has_pine else None
    xl = xlate_of(sc, dxoff, dyoff, poff2)
    lt = np.full(nl, -1, np.int64) if line_tile is None else np.asarray(line_tile, np.int64)
    # the mesh walk of every (line, tile): the mesh model with the line restricted to that tile
    mesh = [lim.batch_hits(sc, txy, zvals, mzmin, mzmax, lines, np.full(nl, i, np.int64), dxoff, dyoff, distant) for i in range(n)]
    finite = np.isfinite(lines).all(axis=(1, 2))
    for r in range(nl):
        if not finite[r]:
            continue
        v1, v2 = lines[r, 0], lines[r, 1]
        best = None  # (t, tile, record of the hit)
        for i in (range(n) if lt[r] < 0 else ([int(lt[r])] if lt[r] < n else [])):
            tally["pairs"] += 1
            if distant is not None and distant[i]:
                tally["distant"] += 1
                continue
            tn, rec = ONE, None
            m = mesh[i][r]
            p1, p2 = sub(v1, xl), sub(v2, xl)
            if m["hit"]:
                tally["mesh_hits"] += 1
                tn, rec = f32(m["t"]), (HIT_MESH, int(m["xpos"]), int(m["ypos"]), -1, 0)
                if tiles is not None and tiles[i].nvalid:  # (for the tally only: what the trees would have said)
                    c, tt, _, _ = tiles[i].line_intersect(g, p1, p2, ONE, new_tally())
                    tally["mesh_hides_nearer_tree"] += bool(c and tt < tn)
            elif tiles is None or tiles[i].nvalid == 0:
                tally["tiles_without_trees"] += 1
            else:
                c, tt, j, part = tiles[i].line_intersect(g, p1, p2, tn, tally)
                if c:
                    tally["tree_hits"] += 1
                    tn, rec = tt, (HIT_TREE, 0, 0, j, part)
                    d = lim.mesh_bcube(sc, txy[i:i + 1, 0], txy[i:i + 1, 1], mzmin[i:i + 1], mzmax[i:i + 1], dxoff, dyoff)[0]
                    with np.errstate(all="ignore"):
                        inbox = view_model.do_line_clip([np.array([x], f32) for x in v1], [np.array([x], f32) for x in v2], d)[0][0]
                    tally["mesh_box_missed_tree_hit"] += not inbox
            if rec is None:
                continue
            if best is not None and tn == best[0]:
                tally["ties"] += 1
            if tn < (f32(2.0) if best is None else best[0]):
                best = (tn, i, rec)
        if best is not None:
            tn, i, (kind, xp, yp, j, part) = best
            tally["tree_wins" if kind == HIT_TREE else "mesh_wins"] += 1
            out[r] = (tn, i, xp, yp, v1 + tn * (v2 - v1), kind, j, part)
    return out
