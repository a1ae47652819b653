"""Cases of the line query with inc_trees = 1 (terra_tiles_line_intersect_trees[_dev]) shared by test_line_trees_emul.py (the host emulator) and
test_gpu_line_trees.py (HIP on the MI355X).  Every byte of every hit record is compared with tests/line_trees_model.py.

The cases author their zvals and records: S = 16 on a 3 x 3 batch unless said otherwise (a tile is 8 wide, tile (0, 0) spans [-4, 4]^2, DX_VAL is 0.5), the ground
flat at z = 0 (the mesh box of a tile is 2e-6 high: a line above the ground misses it).  A pine of height 0.5 and width 0.15 at z = 0 becomes 0.6 high: its trunk
runs from z = -0.13 up to 0.5 with radius 0.017 at the bottom, its leaf cone from z = 0.21 (radius 0.168) up to the apex at 0.6.  Positions are given in camera
space; the container's xlate is taken off.  The model's result of a case is computed once per process (MODEL) with its tally, and every case carries a check on that
tally: that it reaches what it is named for."""
import ctypes as C

import numpy as np

import line_intersect_model as lim
import line_trees_model as ltm
import tree_ao_model as tam
import tree_view_cases as trc
import tree_view_model as vm

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
FILL = 0xA5
PINE, DECID_T, TDECID, BUSH, PALM, SH_PINE = range(6)
TILES3 = [(x, y) for y in (-1, 0, 1) for x in (-1, 0, 1)]  # tile (0, 0) is batch index 4
MESH, TREE = ltm.HIT_MESH, ltm.HIT_TREE


class Case:
    def __init__(self, name, build, tiles=TILES3, S=16, dxoff=0, dyoff=0, poff2=(0, 0), instanced=False, ninst=(0, 0), tree_scale=1.0, tree_depth_scale=1.0, dev_only=False,
                 check=None):
        self.name, self.build, self.tiles, self.S, self.dxoff, self.dyoff, self.poff2 = name, build, list(tiles), S, dxoff, dyoff, poff2
        self.instanced, self.ninst, self.tree_scale, self.tree_depth_scale, self.dev_only, self.check = instanced, ninst, tree_scale, tree_depth_scale, dev_only, check

    def dx(self):
        return 8.0 / self.S

    def xlate(self):
        return (self.dx() * (self.dxoff + self.poff2[0]), self.dx() * (self.dyoff + self.poff2[1]))

    def origin(self, t):
        """the low corner of tile t in camera space"""
        tx, ty = self.tiles[t]
        return 8.0 * tx - 4.0 + self.dx() * self.dxoff, 8.0 * ty - 4.0 + self.dx() * self.dyoff

    def centre(self, t):
        ox, oy = self.origin(t)
        return ox + 4.0, oy + 4.0


class Inputs:
    def __init__(self, case, cap=8):
        n, Z = len(case.tiles), case.S + 2
        self.case, self.n = case, n
        self.z = np.zeros((n, Z, Z), f32)
        self.rec = trc.Records(n, cap) if cap else None
        self.lines, self.line_tile, self.distant = [], None, None

    def tree(self, t, pos, typ=PINE, inst=-1, height=0.5, width=0.15):
        xl = self.case.xlate()
        return self.rec.add(t, (pos[0] - xl[0], pos[1] - xl[1], pos[2]), typ, inst, height, width)

    def override(self, t, j, p1, p2, r1, r2, rotated=1):
        if self.rec.override is None:
            self.rec.override = np.zeros(self.rec.pine.shape, trc.override_dtype())
        xl = self.case.xlate()
        self.rec.override[t, j] = ((p1[0] - xl[0], p1[1] - xl[1], p1[2]), (p2[0] - xl[0], p2[1] - xl[1], p2[2]), r1, r2, rotated)

    def line(self, v1, v2, tile=None):
        self.lines.append((v1, v2))
        if tile is not None:
            if self.line_tile is None:
                self.line_tile = [-1] * (len(self.lines) - 1)
            self.line_tile.append(tile)
        elif self.line_tile is not None:
            self.line_tile.append(-1)

    def across(self, pos, z=0.1, dy=0.0, half=2.0, dz=0.0, tile=None):
        """a line along x through (pos.x, pos.y + dy) at height pos.z + z (+- dz at its ends)"""
        self.line((pos[0] - half, pos[1] + dy, pos[2] + z + dz), (pos[0] + half, pos[1] + dy, pos[2] + z - dz), tile)

    def line_array(self):
        return np.array(self.lines, f32).reshape(-1, 2, 3)

    def tile_array(self):
        return None if self.line_tile is None else np.array(self.line_tile, np.int32)

    def mz(self):
        return self.z.reshape(self.n, -1).min(axis=1).astype(f32), self.z.reshape(self.n, -1).max(axis=1).astype(f32)


def at(case, t, x, y, z=0.0):
    cx, cy = case.centre(t)
    return (cx + x, cy + y, z)


# ---- the builders
def b_parts(case):
    """trunk only (below the cone), cone only (beside the trunk), both (the cone nearer: the second cylinder lowers t again), a T_SH_PINE's cone from pos"""
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    inp.tree(4, p)
    inp.across(p, 0.1)
    inp.across(p, 0.4, dy=0.05)
    inp.across(p, 0.3)
    q = at(case, 5, 0.5, 1.0)
    inp.tree(5, q, SH_PINE)
    inp.across(q, 0.1, dy=0.05)
    inp.tree(5, at(case, 5, 0.5, 2.0), PINE)
    inp.across(at(case, 5, 0.5, 2.0), 0.1, dy=0.05)   # the same line beside a T_PINE: its cone starts at 0.35*height
    return inp


def b_two_trees(case):
    """two trees on one line: the nearer one is record 0, then record 1"""
    inp = Inputs(case)
    a, b = at(case, 4, -1.0, 0.0), at(case, 4, 1.0, 0.0)
    inp.tree(4, a); inp.tree(4, b)
    inp.line((a[0] - 1.0, a[1], 0.3), (b[0] + 1.0, b[1], 0.28))
    inp.line((b[0] + 1.0, b[1], 0.3), (a[0] - 1.0, a[1], 0.28))
    return inp


def b_other_types(case):
    """palms, bushes and deciduous types beside a pine on one line: only the pine is hit"""
    inp = Inputs(case)
    for k, typ in enumerate((PALM, BUSH, DECID_T, TDECID, PINE, PALM)):
        inp.tree(4, at(case, 4, -2.0 + 0.6 * k, 0.0), typ)
    inp.line(at(case, 4, -3.5, 0.0, 0.15), at(case, 4, 3.5, 0.0, 0.14))
    inp.line(at(case, 4, -3.5, 0.0, 0.15), at(case, 4, 0.0, 0.0, 0.14))   # ends before the pine
    inp.tree(3, at(case, 3, 0.0, 0.0), BUSH)                              # a lone bush: a container that is not empty with an all_bcube of zero area (no cull)
    inp.across(at(case, 3, 0.0, 0.0), 0.1, tile=3)
    return inp


def b_mesh_and_trees(case):
    """the mesh of a tree's own tile wins although the tree stands nearer; a tree in one tile against the mesh of another, either way round"""
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    inp.tree(4, p)
    inp.line((p[0] - 1.0, p[1], 0.4), (p[0] + 2.0, p[1], -0.2))           # through the tree, then into the ground of the same tile
    q = at(case, 5, -3.0, 1.0)                                           # 1 from tile 5's low edge
    inp.tree(5, q)
    inp.line((q[0] + 1.0, q[1], 0.35), (q[0] - 3.0, q[1], -0.05))         # the tree of tile 5 at t = 0.25, the ground of tile 4 behind it
    inp.line((q[0] - 3.0, q[1], 0.05), (q[0] + 1.0, q[1], -0.15))         # the ground of tile 4 first, then (under the ground) the trunk of tile 5
    return inp


def b_same_tree_twice(case):
    """one tree recorded in two tiles: equal t, the lowest batch index"""
    inp = Inputs(case)
    p = at(case, 4, 0.3, 0.3)
    inp.tree(7, p); inp.tree(2, p); inp.tree(6, p)
    inp.across(p, 0.3)
    inp.across(p, 0.3, tile=6)
    return inp


def b_horizontal(case):
    """a horizontal line through a trunk (the mesh can never hit), at the ground's own height too"""
    inp = Inputs(case)
    p = at(case, 4, 1.0, -1.0)
    inp.tree(4, p)
    inp.across(p, 0.1)
    inp.across(p, 0.0)
    inp.across(p, -0.05)
    inp.line((p[0], p[1] - 2.0, 0.2), (p[0], p[1] + 2.0, 0.2))
    return inp


def b_end_on_surface(case):
    """lines that end on the trunk's surface: the one whose t_new is exactly 1 is no hit (t_new < *t with *t = 1.0), its neighbours an ulp on are"""
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    inp.tree(4, p)
    g = globals_of(case)
    s = vm.SmallTree.make(g, inp.rec.pine[4, 0], None)
    xl = [f32(v) for v in case.xlate()] + [f32(0.0)]
    found = 0
    for k in range(400):
        z = 0.02 + 0.0004 * k  # (below the leaf cone, which starts at 0.21)
        v1 = np.array([p[0] - 1.0 - 0.01 * (k % 7), p[1], z], f32)
        r_at = float(s.r1) * (float(s.p2[2]) - z) / (float(s.p2[2]) - float(s.p1[2]))
        v2 = np.array([p[0] - r_at, p[1], z], f32)
        for _ in range(40):
            r = ltm.trunc_cone(ltm.sub(v1, xl), ltm.sub(v2, xl), s.p2, s.p1, s.r2, s.r1)
            if r[0] and r[1] == f32(1.0):
                break
            v2[0] = np.nextafter(v2[0], f32(-np.inf) if r[0] else f32(np.inf))  # a hit below 1: pull the end back; no hit: push it on
        else:
            continue
        inp.line(v1, v2.copy())
        longer = v2.copy(); longer[0] = p[0] - 0.5 * r_at
        inp.line(v1, longer)
        found += 1
        if found == 3:
            break
    assert found == 3, "no line with t_new == 1 found"
    return inp


def b_distant_and_tiles(case):
    """a distant tile (its tree is not hit), line_tile >= 0 in range"""
    inp = Inputs(case)
    inp.distant = np.zeros(inp.n, np.uint8)
    inp.distant[5] = 1
    for t in (3, 4, 5):
        inp.tree(t, at(case, t, 0.0, 0.0))
    a, b = at(case, 3, -2.0, 0.0, 0.3), at(case, 5, 2.0, 0.0, 0.29)
    inp.line(a, b)           # the tree of tile 3
    inp.line(b, a)           # tile 5 is distant: the tree of tile 4
    inp.line(b, a, tile=5)   # the distant tile alone
    inp.line(b, a, tile=3)
    inp.line(a, b, tile=4)
    inp.line(a, b, tile=0)   # a tile without trees
    return inp


def b_out_of_range(case):
    """line_tile out of range (the device form: a miss), negative values other than -1"""
    inp = Inputs(case)
    inp.tree(4, at(case, 4, 0.0, 0.0))
    a, b = at(case, 4, -2.0, 0.0, 0.3), at(case, 4, 2.0, 0.0, 0.29)
    for tile in (9, 10, 2 ** 31 - 1, -2, -2 ** 31, 4):
        inp.line(a, b, tile=tile)
    return inp


def b_non_finite(case):
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    inp.tree(4, p)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            v = np.array([[p[0] - 2.0, p[1], 0.3], [p[0] + 2.0, p[1], 0.29]], f32)
            v.reshape(-1)[k] = bad
            inp.line(v[0], v[1])
    inp.across(p, 0.3)
    return inp


COUNTS = [0, 1, 63, 64, 65, 75, 2, 129, 4000000000]


def b_counts(case):
    """counts 0, 1, 63, 64, 65 and above the capacity (70): a tile's last live record stands on the line, the others far off it; where the count exceeds the capacity
    a line also runs where record `capacity` would stand"""
    cap = 70
    inp = Inputs(case, cap)
    for t, cnt in enumerate(COUNTS):
        m = min(cnt, cap)
        for j in range(m):
            last = j == m - 1
            inp.tree(t, at(case, t, 0.0 if last else -3.0 + 0.08 * j, 0.0 if last else 2.0 + 0.02 * (j % 9)), PINE if j % 5 else BUSH if not last else PINE)
        inp.rec.counts[t] = cnt
        inp.across(at(case, t, 0.0, 0.0), 0.3, tile=t)
        inp.across(at(case, t, 0.0, 2.05), 0.3, half=3.5, tile=t)   # along the row of the others
    inp.line(at(case, 0, -3.0, 0.0, 0.3), at(case, 2, 3.0, 0.0, 0.29))  # across three tiles
    return inp


def b_dropped(case):
    """a tile of dropped records only (all_bcube stays zero, the container is empty); a dropped record between two valid ones; an instanced record while `instanced`
    is off; a width <= 0 (the trunk's cylinder asserts in the reference: it does not hit, the cone does)"""
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    inp.tree(4, p, 9); inp.tree(4, p, -1); inp.tree(4, p, PINE, inst=2)
    inp.across(p, 0.3)
    q = at(case, 5, 0.0, 0.0)
    inp.tree(5, at(case, 5, -1.0, 1.0)); inp.tree(5, q, 6); inp.tree(5, q)
    inp.across(q, 0.3)
    w = at(case, 3, 0.0, 0.0)
    inp.tree(3, w, PINE, width=-0.1); inp.tree(3, at(case, 3, 1.0, 1.0), PINE, width=0.0)
    inp.across(w, 0.1)
    inp.across(w, 0.3)
    inp.across(at(case, 3, 1.0, 1.0), 0.1)
    return inp


def b_instanced(case):
    """instanced records: the instance's type and size; an instance outside the table is dropped"""
    inp = Inputs(case, 12)
    for k in range(10):
        inp.tree(4, at(case, 4, -3.0 + 0.6 * k, 0.0), PALM, inst=k - 1 if k else 40)  # (the record's own type is not read)
    inp.line(at(case, 4, -3.9, 0.0, 0.12), at(case, 4, 3.9, 0.0, 0.11))
    inp.line(at(case, 4, 3.9, 0.0, 0.12), at(case, 4, -3.9, 0.0, 0.11))
    for k in range(10):
        inp.across(at(case, 4, -3.0 + 0.6 * k, 0.0), 0.2, dy=0.01, half=0.25)
    return inp


def b_override(case):
    """a rotated pine: the caller's cylinder is trunk_cylin and its direction get_rot_dir(); rotated = 0: the entry is not read"""
    inp = Inputs(case)
    p = at(case, 4, 0.0, 0.0)
    j = inp.tree(4, p)
    inp.override(4, j, (p[0], p[1], -0.1), (p[0] + 0.4, p[1], 0.5), 0.03, 0.0)
    q = at(case, 4, 0.0, 2.0)
    j = inp.tree(4, q)
    inp.override(4, j, (q[0] + 1.0, q[1], -0.1), (q[0] + 1.0, q[1], 0.5), 0.2, 0.0, rotated=0)
    inp.line((p[0] + 0.4 / 6.0, p[1] - 1.0, 0.0), (p[0] + 0.4 / 6.0, p[1] + 1.0, 0.0))   # the leaning trunk where it crosses z = 0, away from pos and below the cone
    inp.line((p[0] - 1.0, p[1] + 0.01, 0.45), (p[0] + 1.0, p[1] + 0.01, 0.44))  # the leaning cone
    inp.across(q, 0.1)
    inp.line((q[0] + 1.0, q[1] - 1.0, 0.1), (q[0] + 1.0, q[1] + 1.0, 0.1))   # where the unread entry stands
    return inp


def forest(case, inp, rng, per_tile, h=(0.3, 0.7)):
    for t in range(inp.n):
        for k in range(per_tile):
            typ = (PINE, PINE, SH_PINE, PALM, PINE, BUSH)[k % 6]
            inp.tree(t, at(case, t, float(rng.uniform(-3.9, 3.9)), float(rng.uniform(-3.9, 3.9))), typ, height=float(rng.uniform(*h)), width=float(rng.uniform(0.1, 0.2)))


def b_many_lines(case):
    """300 lines in one call over 40 trees a tile: level shots at the trees, shots into the ground, shots from above, a third of them restricted to a tile"""
    inp = Inputs(case, 40)
    rng = np.random.default_rng(31)
    forest(case, inp, rng, 40)
    xl = case.xlate()
    for k in range(300):
        t = int(rng.integers(inp.n))
        r = inp.rec.pine[t, int(rng.integers(40))]
        off = 0.0 if k % 4 == 0 else 0.1  # every fourth line at the trunk's axis, low and level
        tgt = np.array([r["pos"][0] + xl[0] + rng.uniform(-off, off), r["pos"][1] + xl[1] + rng.uniform(-off, off), rng.uniform(0.02, 0.15) if k % 4 == 0 else rng.uniform(0.0, 0.6)])
        yaw, pitch = rng.uniform(0, 2 * np.pi), (rng.uniform(-0.1, 0.1), rng.uniform(-1.2, -0.2), rng.uniform(-0.5, 0.0))[0 if k % 4 == 0 else k % 3]
        d = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])
        inp.line(tgt - d * rng.uniform(0.5, 9.0), tgt + d * rng.uniform(0.1, 9.0), tile=(t if k % 3 == 0 else -1))
    return inp


def b_s128(case):
    """S = 128 with offsets, rolling ground: 30 trees a tile on the ground, lines as b_many_lines"""
    inp = Inputs(case, 32)
    rng = np.random.default_rng(37)
    Z = case.S + 2
    for t in range(inp.n):
        ox, oy = case.origin(t)
        xs, ys = ox + case.dx() * np.arange(Z), oy + case.dx() * np.arange(Z)
        inp.z[t] = (0.3 * np.sin(0.7 * xs)[None, :] * np.cos(0.5 * ys)[:, None]).astype(f32)
    xl = case.xlate()
    for t in range(inp.n):
        for k in range(30):
            x, y = float(rng.uniform(-3.9, 3.9)), float(rng.uniform(-3.9, 3.9))
            cx, cy = case.centre(t)
            zg = 0.3 * np.sin(0.7 * (cx + x)) * np.cos(0.5 * (cy + y))
            inp.tree(t, (cx + x, cy + y, float(zg)), (PINE, SH_PINE, PALM)[k % 3], height=float(rng.uniform(0.3, 0.7)), width=float(rng.uniform(0.1, 0.2)))
    for k in range(120):
        t = int(rng.integers(inp.n))
        r = inp.rec.pine[t, int(rng.integers(30))]
        tgt = np.array([r["pos"][0] + xl[0] + rng.uniform(-0.05, 0.05), r["pos"][1] + xl[1] + rng.uniform(-0.05, 0.05), r["pos"][2] + rng.uniform(0.05, 0.5)])
        yaw, pitch = rng.uniform(0, 2 * np.pi), (rng.uniform(-0.05, 0.05), rng.uniform(-1.0, -0.2))[k % 2]
        d = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])
        inp.line(tgt - d * rng.uniform(0.3, 6.0), tgt + d * rng.uniform(0.1, 6.0))
    return inp


OFF = dict(dxoff=-37, dyoff=22, poff2=(5, -3))


def cases():
    kinds = lambda h: h["hit"].tolist()  # noqa: E731
    return [
        Case("parts", b_parts, check=lambda t, h: kinds(h) == [TREE] * 4 + [0] and h["part"].tolist()[:4] == [0, 1, 1, 1] and t["both_lower"] == 1 and t["trunk_lowers"] == 2),
        Case("parts_offset", b_parts, **OFF, check=lambda t, h: kinds(h) == [TREE] * 4 + [0] and h["part"].tolist()[:4] == [0, 1, 1, 1]),
        Case("two_trees", b_two_trees, check=lambda t, h: h["tree"].tolist() == [0, 1] and t["t_new_not_below"] >= 1),
        Case("other_types", b_other_types, **OFF, check=lambda t, h: kinds(h) == [TREE, 0, 0] and h["tree"][0] == 4 and t["not_pine"] >= 8 and t["gate_zero_area"] >= 1),
        Case("mesh_and_trees", b_mesh_and_trees, check=lambda t, h: kinds(h) == [MESH, TREE, MESH] and h["tile"].tolist() == [4, 5, 4] and t["mesh_hides_nearer_tree"] == 1
             and t["tree_hits"] >= 2),
        Case("mesh_and_trees_offset", b_mesh_and_trees, **OFF, check=lambda t, h: kinds(h) == [MESH, TREE, MESH] and h["tile"].tolist() == [4, 5, 4]),
        Case("same_tree_twice", b_same_tree_twice, check=lambda t, h: h["tile"].tolist() == [2, 6] and t["ties"] >= 2),
        Case("horizontal", b_horizontal, **OFF, check=lambda t, h: kinds(h) == [TREE] * 4 and t["mesh_hits"] == 0),
        Case("end_on_surface", b_end_on_surface, check=lambda t, h: kinds(h) == [0, TREE] * 3 and t["t_new_not_below"] >= 3),
        Case("end_on_surface_offset", b_end_on_surface, **OFF, check=lambda t, h: kinds(h) == [0, TREE] * 3),
        Case("distant_and_line_tile", b_distant_and_tiles, check=lambda t, h: h["tile"].tolist() == [3, 4, -1, 3, 4, -1] and t["distant"] >= 2 and t["mesh_box_missed_tree_hit"] >= 4),
        Case("line_tile_out_of_range", b_out_of_range, dev_only=True, check=lambda t, h: kinds(h) == [0] * 3 + [TREE] * 3),
        Case("non_finite", b_non_finite, **OFF, check=lambda t, h: kinds(h) == [0] * 18 + [TREE]),
        Case("counts", b_counts, check=lambda t, h: [int(x) for x in h["tree"][0:18:2]] == [-1, 0, 62, 63, 64, 69, 1, 69, 69] and h["hit"][18] == TREE and t["tiles_without_trees"] >= 1),
        Case("dropped", b_dropped, **OFF, check=lambda t, h: kinds(h) == [0, TREE, 0, TREE, 0] and h["tree"][1] == 2 and t["dropped"] == 4 and t["tiles_without_trees"] >= 1
             and t["asserting_cylinders"] >= 2 and t["gate_zero_area"] == 0),
        Case("instanced", b_instanced, instanced=True, ninst=(4, 4), check=lambda t, h: t["dropped"] == 2 and (h["hit"][:2] == TREE).all() and (h["hit"] == TREE).sum() >= 4 and t["not_pine"] >= 4),
        Case("trunk_override", b_override, **OFF, check=lambda t, h: kinds(h) == [TREE] * 3 + [0] and h["part"].tolist()[:3] == [0, 1, 0] and t["rotated"] == 1),
        Case("three_hundred_lines", b_many_lines, check=lambda t, h: len(h) == 300 and (h["hit"] == TREE).sum() >= 60 and (h["hit"] == MESH).sum() >= 60 and (h["hit"] == 0).sum() >= 10
             and t["mesh_hides_nearer_tree"] >= 3 and t["gate_exit"] >= 100 and t["cone_lowers"] >= 30 and t["trunk_lowers"] >= 10),
        Case("three_hundred_lines_offset", b_many_lines, **OFF, tree_scale=2.0, tree_depth_scale=1.5, check=lambda t, h: (h["hit"] == TREE).sum() >= 40 and (h["hit"] == MESH).sum() >= 60),
        Case("s128_offsets", b_s128, S=128, dxoff=-70, dyoff=33, poff2=(3, 8), check=lambda t, h: (h["hit"] == TREE).sum() >= 25 and (h["hit"] == MESH).sum() >= 25),
    ]


# ---- the model and the library on a case
MODEL = {}


def globals_of(case):
    insts = trc.inst_table(*case.ninst) if case.instanced else None
    return vm.Globals(tam.SizeParams(tree_scale=case.tree_scale), vm.Args(tree_depth_scale=case.tree_depth_scale), case.instanced, insts)


def scene_of(case):
    return lim.Scene(4.0, 4.0, case.dx(), case.dx(), 1.0 / case.dx(), 1.0 / case.dx(), case.S)


def model(case):
    """(globals, inputs, hits, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        g = globals_of(case)
        inp = case.build(case)
        tally = ltm.new_tally()
        mzmin, mzmax = inp.mz()
        hits = ltm.batch_hits(scene_of(case), g, case.tiles, inp.z, mzmin, mzmax, inp.rec.pine, inp.rec.counts, inp.rec.override, inp.line_array(), inp.tile_array(), case.dxoff,
                              case.dyoff, case.poff2, inp.distant, tally)
        MODEL[case.name] = (g, inp, hits, tally)
    return MODEL[case.name]


def configure(pkg, t, case, g):
    st = t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    sc = scene_of(case)
    assert (f32(st.DX_VAL), f32(st.DY_VAL), f32(st.DX_VAL_INV), f32(st.DY_VAL_INV)) == (sc.DX_VAL, sc.DY_VAL, sc.DX_VAL_INV, sc.DY_VAL_INV)
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_scale=case.tree_scale, instanced=case.instanced, num_pine_insts=case.ninst[0], num_palm_insts=case.ninst[1]))
    t.set_tree_size_params(pkg.make_tree_size_params())
    t.set_tree_instances(g.insts)


def stats_of(pkg, inp):
    st = (pkg.TileStats * inp.n)()
    mzmin, mzmax = inp.mz()
    for i in range(inp.n):
        st[i].mzmin, st[i].mzmax = float(mzmin[i]), float(mzmax[i])
        st[i].radius = 6.0
    return st


def host_arrays(pkg, case, inp):
    return dict(zvals=inp.z, stats=stats_of(pkg, inp), is_distant=inp.distant, pine=inp.rec.pine, pine_counts=inp.rec.counts, trunk_override=inp.rec.override)


def scalars(case):
    return dict(dxoff=case.dxoff, dyoff=case.dyoff, ptree_xoff2=case.poff2[0], ptree_yoff2=case.poff2[1], tree_depth_scale=case.tree_depth_scale)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1) if isinstance(a, np.ndarray) else np.frombuffer(bytes(memoryview(a).cast("B")), np.uint8)


class DeviceInputs:
    """the arrays of a make_line_trees_in uploaded: .lin holds device addresses"""

    def __init__(self, pkg, t, kw, sc):
        self.bufs, dev = {}, {}
        for k, a in kw.items():
            if a is None:
                continue
            b = as_bytes(a)
            self.bufs[k] = t.alloc(max(b.nbytes, 4))
            if b.nbytes:
                self.bufs[k].upload(b)
            dev[k] = self.bufs[k].ptr
        self.lin = pkg.make_line_trees_in(pine_capacity=kw["pine"].shape[1] if kw.get("pine") is not None else 0, **dev, **sc)

    def free(self):
        for b in self.bufs.values():
            b.free()


def run_dev(pkg, t, tiles, kw, sc, lines, line_tile):
    """the device-pointer form on freshly allocated buffers, the records filled with FILL -> LINE_TREE_HIT_DTYPE [nlines]"""
    d = DeviceInputs(pkg, t, kw, sc)
    nl = len(lines)
    nb = max(nl * 40, 4)
    lb, hb = t.alloc(max(lines.nbytes, 4)), t.alloc(nb + 8).upload(np.full(nb + 8, FILL, np.uint8))
    tb = None if line_tile is None else t.alloc(max(line_tile.nbytes, 4))
    try:
        if nl:
            lb.upload(as_bytes(lines))
            if tb is not None:
                tb.upload(as_bytes(line_tile))
        t.tiles_line_intersect_trees_dev(tiles, d.lin, lb.ptr, nl, hb.ptr, None if tb is None else tb.ptr)
        raw = hb.download(np.uint8, (nb + 8,)).copy()
        assert (raw[nl * 40:nl * 40 + 8] == FILL).all(), "written past the last record"
        return raw[:nl * 40].view(pkg.LINE_TREE_HIT_DTYPE)
    finally:
        d.free()
        for b in (lb, hb, tb):
            if b is not None:
                b.free()


def compare(what, got, want, lines):
    assert len(got) == len(want), what
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), f"{what}: line {i} {np.asarray(lines[i]).tolist()}: {got[i]} != {want[i]}"


def run_case(pkg, t, case, dev=False):
    g, inp, hits, tally = model(case)
    assert case.check(tally, hits), (case.name, {k: x for k, x in tally.items() if x}, hits.tolist())
    configure(pkg, t, case, g)
    kw, sc = host_arrays(pkg, case, inp), scalars(case)
    lines, lt = inp.line_array(), inp.tile_array()
    what = case.name + (" (dev)" if dev else "")
    if dev:
        got = run_dev(pkg, t, case.tiles, kw, sc, lines, lt)
    elif case.dev_only:  # the host form reads line_tile up front and refuses the call
        out = np.full(len(lines) * 40, 3, np.uint8)
        lin = pkg.make_line_trees_in(**kw, **sc)
        txy = np.array(case.tiles, np.int32)
        assert t.lib.terra_tiles_line_intersect_trees(t.ctx, txy.ctypes.data, len(txy), C.byref(lin), lines.ctypes.data, lt.ctypes.data, len(lines), out.ctypes.data) == ERR_ARG
        assert (out == 3).all()
        return
    else:
        got = t.tiles_line_intersect_trees(case.tiles, pkg.make_line_trees_in(**kw, **sc), lines, lt)
    compare(what, got, hits, lines)


# ---- the fixture's rows through the public entry point: a row's cone is the trunk_override of a pine that stands alone in a tile of its own
def run_fixture_rows(pkg, t, fixture, step=1):
    """row r -> tile r: a rotated pine whose override is (p1 = cp2, p2 = cp1, r1 = r2, r2 = r1) and whose own pos (and leaf cone) is far away; line r against tile r
    alone; the ground lies at z = -1000, out of every line's reach.  The expected record is the model's (the container's gate included); where the gate passes it
    must say what the fixture says: a hit exactly where t_set and t < 1, with the fixture's t"""
    rows, t_set, tf = fixture["rows"][::step], fixture["t_set"][::step], fixture["t"][::step]
    n, S = len(rows), 16
    case = Case("fixture_rows", None, tiles=[(i % 64, i // 64) for i in range(n)])
    g = globals_of(case)
    configure(pkg, t, case, g)
    z = np.full((n, S + 2, S + 2), -1000.0, f32)
    rec = trc.Records(n, 1)
    rec.override = np.zeros(rec.pine.shape, trc.override_dtype())
    for i, r in enumerate(rows):
        rec.add(i, (1.0e4, 1.0e4, 1.0e4), PINE, -1, 100.0, 1.0)
        rec.override[i, 0] = (r[9:12], r[6:9], r[13], r[12], 1)
    lines = rows[:, 0:6].reshape(n, 2, 3).copy()
    assert lines[:, :, 2].min() > -900.0
    lt = np.arange(n, dtype=np.int32)
    st = (pkg.TileStats * n)()
    for i in range(n):
        st[i].mzmin = st[i].mzmax = -1000.0
    want = np.zeros(n, ltm.HIT_DTYPE)
    want["t"], want["tile"], want["tree"] = 2.0, -1, -1
    tally = ltm.new_tally()
    direct = 0
    for i in range(n):
        tile = ltm.Tile(g, rec.pine[i], 1, rec.override[i], tally)
        before = tally["gate_exit"]
        c, tt, j, part = tile.line_intersect(g, list(lines[i, 0]), list(lines[i, 1]), f32(1.0), tally)
        if c:
            want[i] = (tt, i, 0, 0, lines[i, 0] + tt * (lines[i, 1] - lines[i, 0]), TREE, j, part)
        if tally["gate_exit"] == before:
            direct += 1
            assert bool(c) == bool(t_set[i] and tf[i] < 1.0) and (not c or (tt.tobytes() == tf[i].tobytes() and part == 0)), (i, rows[i], c, tt, t_set[i], tf[i])
    assert direct >= 0.5 * n and tally["trunk_lowers"] >= 0.2 * n, (direct, n, tally)
    kw = dict(zvals=z, stats=st, is_distant=None, pine=rec.pine, pine_counts=rec.counts, trunk_override=rec.override)
    got = run_dev(pkg, t, case.tiles, kw, scalars(case), lines, lt)
    compare("fixture rows", got, want, lines)
    return direct


# ---- the resident chain: zvals -> placement -> a removing stroke -> lines
def run_resident_chain(pkg, t):
    """tiles_create_zvals_dev -> tiles_place_trees_dev -> tiles_tree_ao_shadows_dev (trmax) -> one removing stroke of tiles_edit_trees_dev ->
    tiles_line_intersect_trees_dev on a 3 x 3 batch at S = 128 on one context with nothing read back in between.  The lines are aimed at pines the stroke removes and
    at pines it leaves, so the placement (it is deterministic) is run and read once beforehand to choose them; the model is fed from the records read back at the end"""
    S, cap, cap_l = 128, 320, 2048
    tiles = [(x, y) for y in range(-1, 2) for x in range(1, 4)]  # over the island's shore: pines and palms
    n, W, Z = len(tiles), S + 1, S + 2
    cfg = pkg.make_config(mesh_gen_mode=0, mesh_xy=S)
    st0 = t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(grass_density=1))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_tree_size_params(pkg.make_tree_size_params())
    sc = lim.Scene.of(cfg, st0)
    sizes = dict(z=n * Z * Z * 4, st=n * C.sizeof(pkg.TileStats), pt=n * cap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4, tm=n * W * W * 2, trm=n * 4, es=n, ec=n)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    p = {k: b.ptr for k, b in bufs.items()}
    read = lambda: (bufs["pt"].download(np.uint8, (sizes["pt"],)).copy().view(pkg.TREE_PLACE_DTYPE).reshape(n, cap), bufs["pc"].download(np.uint32, (n,)).copy())  # noqa: E731
    try:
        def place():
            bufs["pt"].upload(np.zeros(sizes["pt"], np.uint8))
            t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
            t.tiles_place_trees_dev(tiles, cap, p["pt"], p["pc"], 0, 0, None, p["st"])
            t.tiles_tree_ao_shadows_dev(tiles, cap_l, p["tm"], p["pt"], p["pc"], cap, trmax_ptr=p["trm"])
        place()
        pine0, pc0 = read()
        pines = [(i, j) for i in range(n) for j in range(min(int(pc0[i]), cap)) if pine0[i, j]["type"] in (PINE, SH_PINE) and pine0[i, j]["inst"] < 0]
        assert len(pines) >= 60, pc0.tolist()
        rng = np.random.default_rng(41)
        xy = np.array([pine0[ij]["pos"][:2] for ij in pines], np.float64)
        radius = 1.5
        near = (np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]) < 0.6 * radius).sum(axis=1)
        centre = [float(v) for v in pine0[pines[int(np.argmax(near))]]["pos"]]  # the pine with the most pines around it
        dist = lambda ij: float(np.hypot(pine0[ij]["pos"][0] - centre[0], pine0[ij]["pos"][1] - centre[1]))  # noqa: E731
        inside, outside = [ij for ij in pines if dist(ij) < 0.6 * radius], [ij for ij in pines if dist(ij) > 1.5 * radius]
        assert len(inside) >= 3 and len(outside) >= 20, (len(inside), len(outside))
        aimed = inside[:12] + [outside[k] for k in rng.choice(len(outside), 40, replace=False)]
        lines = []
        for ij in aimed:
            x, y, zz = (float(v) for v in pine0[ij]["pos"])
            h = float(pine0[ij]["height"])
            yaw = rng.uniform(0, 2 * np.pi)
            d = np.array([np.cos(yaw), np.sin(yaw), -0.02])
            tgt = np.array([x, y, zz + 0.3 * h])
            lines.append([tgt - 0.4 * d, tgt + 0.2 * d])
        lines = np.array(lines, f32)
        bufs["ln"], bufs["h"] = t.alloc(lines.nbytes).upload(as_bytes(lines)), t.alloc(len(lines) * 40).upload(np.full(len(lines) * 40, FILL, np.uint8))
        # the chain, nothing read back between its steps
        place()
        t.tiles_edit_trees_dev(tiles, p["st"], centre, radius, False, False, p["trm"], p["es"], p["ec"], p["pt"], p["pc"], cap)
        lin = pkg.make_line_trees_in(zvals=p["z"], stats=p["st"], pine=p["pt"], pine_counts=p["pc"], pine_capacity=cap)
        t.tiles_line_intersect_trees_dev(tiles, lin, bufs["ln"].ptr, len(lines), bufs["h"].ptr)
        got = bufs["h"].download(np.uint8, (len(lines) * 40,)).copy().view(pkg.LINE_TREE_HIT_DTYPE)
        pine, pc = read()
        zv = bufs["z"].download(f32, (n, Z, Z)).copy()
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
    finally:
        for b in bufs.values():
            b.free()
    assert int(pc.sum()) < int(pc0.sum()), "the stroke removed nothing"
    mzmin, mzmax = np.array([s.mzmin for s in stats], f32), np.array([s.mzmax for s in stats], f32)
    tally = ltm.new_tally()
    want = ltm.batch_hits(sc, vm.Globals(tam.SizeParams(), vm.Args()), tiles, zv, mzmin, mzmax, pine, pc, None, lines, None, 0, 0, (0, 0), None, tally)
    compare("resident chain", got, want, lines)
    live = {(i, tuple(pine[i, j]["pos"].tolist())) for i in range(n) for j in range(min(int(pc[i]), cap))}
    removed = [k for k, ij in enumerate(aimed) if (ij[0], tuple(pine0[ij]["pos"].tolist())) not in live]
    survivors = [k for k, ij in enumerate(aimed) if k >= 12 and (ij[0], tuple(pine0[ij]["pos"].tolist())) in live]
    assert len(removed) >= 3 and len(survivors) >= 30, (len(removed), len(survivors))
    hit_pos = lambda k: tuple(pine[got[k]["tile"], got[k]["tree"]]["pos"].tolist()) if got[k]["hit"] == TREE else None  # noqa: E731
    for k in removed:  # a removed tree no longer hits
        assert hit_pos(k) != tuple(pine0[aimed[k]]["pos"].tolist()), k
    own = sum(hit_pos(k) == tuple(pine0[aimed[k]]["pos"].tolist()) for k in survivors)
    assert own >= 0.6 * len(survivors), (own, len(survivors), tally)  # a survivor does (but for the ones the ground or another tree hides)
    return tally
