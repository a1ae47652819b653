"""Cases of the sphere collisions and tree box tests (terra_tiles_sphere_collide[_dev], terra_tiles_cube_int_trees[_dev]) shared by test_collide_emul.py (the host
emulator) and test_gpu_collide.py (HIP on the MI355X).  Every output byte is compared with tests/collide_model.py.

The calls need no placement, so the cases author their records on the synthetic scene of terrain_view_cases.py at S = 16 ("flat": every tile spans z 0 .. 0.5, a
tile is 8 wide, tile (0, 0) spans [-4, 4]^2, DX_VAL is 0.5): a pine of height 0.5 and width 0.15 has a trunk of radius 0.0235 from z = pos.z - 0.13 up to
pos.z + 0.6; the table's entry 0 is a deciduous tree with a trunk of radius 0.9*br_scale*0.02 and height 0.375 inside a branch box of +-0.2; a query is a
sphere of radius 0.1 at z = 0.3 unless the case says otherwise.  The model's result of a case is computed once per process (MODEL) with its tally, and every case
carries a check on that tally: that it reaches what it is named for."""
import ctypes as C

import numpy as np

import collide_model as cm
import decid_view_cases as dvc
import orclib
import scenery_view_cases as svc
import terrain_view_cases as tvc
import terrain_view_model as tm
import tree_ao_model as tam
import tree_view_cases as trc
import tree_view_model as vm

ERR_ARG, ERR_STATE = -1, -3
f32 = np.float32
FILL = 0xA5
PINE, DECID_T, TDECID, BUSH, PALM, SH_PINE = range(6)
ALL = cm.INC_DTREES | cm.INC_PTREES | cm.INC_SCENERY
TABLE = 16
R, Z = 0.1, 0.3  # the usual query


class Case:
    def __init__(self, name, tiles, build, S=16, instanced=False, ninst=(0, 0), tree_scale=1.0, tree_depth_scale=1.0, dxoff=0, dyoff=0, poff2=(0, 0), doff2=(0, 0), soff2=(0, 0),
                 check=None):
        self.name, self.tiles, self.build, self.S, self.instanced, self.ninst, self.tree_scale = name, list(tiles), build, S, instanced, ninst, tree_scale
        self.tree_depth_scale, self.dxoff, self.dyoff, self.poff2, self.doff2, self.soff2, self.check = tree_depth_scale, dxoff, dyoff, poff2, doff2, soff2, check
        self.terrain = "flat"  # (what terrain_view_cases.stats_of reads)

    def dx(self):
        return 8.0 / self.S  # DX_VAL = DY_VAL

    def xlate(self, off2):
        return (self.dx() * (self.dxoff + off2[0]), self.dx() * (self.dyoff + off2[1]))

    def origin(self, t):
        """the low corner of tile t in camera space"""
        tx, ty = self.tiles[t]
        return 8.0 * tx - 4.0 + self.dx() * self.dxoff, 8.0 * ty - 4.0 + self.dx() * self.dyoff


class Inputs:
    """what a case builds: the three containers (positions are given in camera space; the container's xlate is taken off), the optional per-tile arrays, the
    queries and the cubes"""

    def __init__(self, case, pcap=8, dcap=8, scap=8):
        n = len(case.tiles)
        self.case, self.n = case, n
        self.pine = trc.Records(n, pcap) if pcap else None
        self.decid, self.decid_counts = (np.zeros((n, dcap), dvc.place_dtype()), np.zeros(n, np.uint32)) if dcap else (None, None)
        self.scen = svc.Records(n, scap, override=True) if scap else None
        self.data = dvc.make_table(TABLE)
        self.br_scale = np.array([1.0 + 0.05 * (k % 5) for k in range(TABLE)], f32)
        self.trmax = self.tile_zmax = self.flags = None
        self.queries, self.cubes, self.cube_tile = [], [], None

    def _loc(self, pos, off2):
        xl = self.case.xlate(off2)
        return (pos[0] - xl[0], pos[1] - xl[1], pos[2])

    def tree(self, t, pos, typ=PINE, inst=-1, height=0.5, width=0.15):
        return self.pine.add(t, self._loc(pos, self.case.poff2), typ, inst, height, width)

    def override(self, t, j, p1, p2, r1, r2, rotated=1):
        if self.pine.override is None:
            self.pine.override = np.zeros(self.pine.pine.shape, trc.override_dtype())
        a, b = self._loc(p1, self.case.poff2), self._loc(p2, self.case.poff2)
        self.pine.override[t, j] = (a, b, r1, r2, rotated)

    def dtree(self, t, pos, tree_id=dvc.PLAIN):
        j = int(self.decid_counts[t])
        r = self.decid[t, j]
        r["pos"] = self._loc(pos, self.case.doff2)
        r["zval"], r["type"], r["tree_id"], r["rseed1"], r["rseed2"], r["cx"], r["cy"] = pos[2], tree_id % 5, tree_id, 17 + j, 23 + j, j % 16, j // 16 % 16
        self.decid_counts[t] = j + 1
        return j

    def sloc(self, pos):
        return self._loc(pos, self.case.soff2)

    def query(self, pos, radius=R, tile=-1, flags=ALL):
        self.queries.append((pos, radius, tile, flags))

    def cube(self, centre, half=(0.05, 0.05, 0.05), tile=None):
        self.cubes.append([centre[0] - half[0], centre[0] + half[0], centre[1] - half[1], centre[1] + half[1], centre[2] - half[2], centre[2] + half[2]])
        if tile is not None:
            self.cube_tile.append(tile)

    def query_array(self):
        q = np.zeros(len(self.queries), cm.QUERY_DTYPE)
        for i, (pos, radius, tile, flags) in enumerate(self.queries):
            q[i] = (pos, radius, tile, flags)
        return q


def fill_far(inp, t, m, which="pine"):
    """m records of a container far from every query of the case: in the tile's far corner"""
    ox, oy = inp.case.origin(t)
    for k in range(m):
        pos = (ox + 7.0 + 0.01 * (k % 50), oy + 7.0 + 0.01 * (k // 50), 0.1)
        if which == "pine":
            inp.tree(t, pos)
        else:
            inp.dtree(t, pos)


# ---- the builders
def b_chain_pine(case, n):
    """query 0: A's push lands the centre in B, which the query's own centre misses; query 1: the centre starts in A' and in C, and A's push takes it out of C.
    Far records lie between them, all in one 64-record chunk"""
    inp = Inputs(case, pcap=40)
    inp.tree(0, (0.0, 0.0, 0.1))          # A
    fill_far(inp, 0, 10)
    inp.tree(0, (0.23, 0.0, 0.1))         # B
    fill_far(inp, 0, 10)
    inp.tree(0, (1.0, 1.0, 0.1))          # A'
    fill_far(inp, 0, 5)
    inp.tree(0, (1.05, 1.0, 0.1))         # C, behind A' as the centre sees it
    inp.query((0.05, 0.0, Z))
    inp.query((0.94, 1.0, Z))
    return inp


def b_chain_across(case, n):
    """a pine's push creates a deciduous hit; a deciduous push creates a scenery hit"""
    inp = Inputs(case)
    inp.tree(0, (0.0, 0.0, 0.1))
    inp.dtree(0, (0.23, 0.0, 0.0))
    inp.dtree(0, (2.0, 2.0, 0.0))
    inp.scen.stump(0, inp.sloc((2.235, 2.0, 0.0)), 0.03, 0.3)
    inp.query((0.05, 0.0, Z))
    inp.query((2.05, 2.0, 0.2))
    return inp


def b_kind_order(case, n):
    """a stump recorded before a rock that the reference walks first: the rock's push takes the centre out of the stump's reach, the stump's would not have; a
    leafy plant recorded before a plant and a surface rock that are walked before it"""
    inp = Inputs(case)
    inp.scen.stump(0, inp.sloc((0.1, 0.0, 0.0)), 0.03, 0.3)
    inp.scen.rock(0, inp.sloc((0.1, 0.3, 0.2)), 0.3)
    inp.scen.leafy(0, inp.sloc((1.0, 0.0, 0.2)), 0.1)
    inp.scen.plant(0, inp.sloc((1.1, 0.05, 0.1)), 0.02, 0.3)
    inp.scen.surface_rock(0, inp.sloc((1.0, 0.2, 0.2)), 0.08)
    inp.query((0.0, 0.0, 0.2))
    inp.query((1.04, 0.08, 0.2))
    return inp


def b_lane63(case, n):
    """130 pines: records 63 and 64 both move the centre (the second only after the first), record 129 moves another query's; 64 deciduous trees whose last is hit"""
    inp = Inputs(case, pcap=130, dcap=64)
    fill_far(inp, 0, 63)
    inp.tree(0, (0.0, 0.0, 0.1))
    inp.tree(0, (0.23, 0.0, 0.1))
    fill_far(inp, 0, 64)
    inp.tree(0, (-2.0, -2.0, 0.1))
    fill_far(inp, 0, 63, "decid")
    inp.dtree(0, (2.0, -2.0, 0.0))
    inp.query((0.05, 0.0, Z))
    inp.query((-2.05, -2.0, Z))
    inp.query((2.05, -2.0, Z))
    return inp


def b_over_capacity(case, n):
    """counts above the capacity: the first `capacity` records, no more (the last query stands where a fifth record would)"""
    inp = Inputs(case, pcap=4, dcap=4, scap=4)
    for k in range(4):
        inp.tree(0, (0.5 * k, 0.0, 0.1))
        inp.dtree(0, (0.5 * k, 1.0, 0.0))
        inp.scen.rock(0, inp.sloc((0.5 * k, 2.0, 0.2)), 0.05)
    inp.pine.counts[0], inp.decid_counts[0], inp.scen.counts[0] = 9, 4000000000, 5
    for k in range(4):
        inp.query((0.5 * k + 0.05, 0.0, Z))
        inp.query((0.5 * k + 0.05, 1.0, Z))
        inp.query((0.5 * k + 0.05, 2.0, 0.2))
    inp.query((2.05, 0.0, Z))
    return inp


def b_stump_row(case, n):
    """70 stumps, each placed so that the push of the one before lands the centre in it: every record is a hit, the replay runs one record per round"""
    inp = Inputs(case, pcap=0, dcap=0, scap=70)
    c = [f32(-3.9), f32(0.0), f32(0.2)]
    start = [float(x) for x in c]
    for k in range(70):
        inp.scen.stump(0, inp.sloc((float(c[0]) - 0.02, float(c[1]), 0.0)), 0.03, 0.3)
        c = cm.scenery_obj_coll(cm.SceneryObj(k, inp.scen.objs[0, k], None), c, f32(R))
        assert c is not None
    inp.query(start)
    return inp


def b_round_trip(case, n):
    """no object near: pos changes by `pos -= xlate; pos += xlate` alone"""
    inp = Inputs(case)
    ox, oy = case.origin(0)
    inp.tree(0, (ox + 7.0, oy + 7.0, 0.1))
    inp.dtree(0, (ox + 7.0, oy + 1.0, 0.0))
    inp.scen.rock(0, inp.sloc((ox + 1.0, oy + 7.0, 0.2)), 0.05)
    rng = np.random.default_rng(11)
    for k in range(24):
        inp.query((ox + float(rng.uniform(0.5, 5.0)), oy + float(rng.uniform(1.5, 5.0)), Z))
    return inp


def b_gates(case, n):
    """both all_bcube gates taken and not taken; tile 1: a lone bush and trees of the flat table entry give boxes of zero area, which never gate"""
    inp = Inputs(case)
    for k in range(3):
        inp.tree(0, (0.4 * k, 0.0, 0.1))
        inp.dtree(0, (0.4 * k, 2.0, 0.0))
    inp.query((0.05, 0.0, Z))      # in the pines' box, out of the deciduous trees' reach
    inp.query((0.05, 2.0, Z))      # the other way round
    inp.query((-3.0, -3.0, Z))     # outside both
    ox, oy = case.origin(1)
    inp.tree(1, (ox + 1.0, oy + 1.0, 0.1), BUSH)
    inp.dtree(1, (ox + 2.0, oy + 2.0, 0.0), dvc.FLAT)
    inp.dtree(1, (ox + 2.0, oy + 3.0, 0.0), dvc.FLAT)
    inp.query((ox + 5.0, oy + 5.0, Z))
    inp.query((ox + 1.0, oy + 1.0, Z))  # the bush: no trunk
    return inp


def b_short_tree(case, n):
    """the short-tree branch: the centre above the trunk's top with the sphere reaching below it -- a trunk shorter than the radius is stepped over, a longer one is
    extended upward by the radius; the same two trees met from the side"""
    inp = Inputs(case)
    inp.tile_zmax = np.full(n, 2.0, f32)
    inp.tree(0, (0.0, 0.0, 0.0), PINE, height=0.05, width=0.15)    # trunk z -0.13 .. 0.033
    inp.tree(0, (1.0, 0.0, 0.0), PINE, height=0.5, width=0.15)     # trunk z -0.13 .. 0.6
    inp.query((0.02, 0.0, 0.2), 0.25)
    inp.query((1.02, 0.0, 0.7), 0.25)
    inp.query((0.02, 0.0, 0.02), 0.25)
    inp.query((1.02, 0.0, 0.3), 0.25)
    inp.query((1.02, 0.0, 1.0), 0.25)   # wholly above the long trunk
    return inp


def b_palm(case, n):
    """a rotated palm: the caller's cylinder replaces get_trunk_cylin's -- the first test is still against pos, the push comes from the cylinder's p1"""
    inp = Inputs(case)
    j = inp.tree(0, (0.0, 0.0, 0.0), PALM, height=0.5, width=0.15)
    inp.override(0, j, (0.05, 0.0, -0.1), (0.45, 0.0, 0.8), 0.03, 0.01)
    j = inp.tree(0, (2.0, 0.0, 0.0), PALM, height=0.5, width=0.15)
    inp.override(0, j, (2.5, 0.0, 0.0), (2.5, 0.0, 1.0), 0.5, 0.5, rotated=0)  # not rotated: the entry is not read
    inp.query((0.02, 0.0, Z))
    inp.query((2.02, 0.0, Z))
    inp.query((0.1, 0.0, Z))
    inp.query((0.3, 0.0, Z))    # beside the leaning trunk, away from pos: not met
    return inp


def b_rocks(case, n):
    """a rock_shape with and without an override, a voxel_rock with one (and one without), a log and a mushroom at the centre"""
    inp = Inputs(case, scap=12)
    inp.scen.rock_shape(0, inp.sloc((0.0, 0.0, 0.2)), override=0.12)
    inp.scen.rock_shape(0, inp.sloc((1.0, 0.0, 0.2)))
    inp.scen.voxel_rock(0, inp.sloc((2.0, 0.0, 0.2)), 0.5, override=0.08)
    inp.scen.voxel_rock(0, inp.sloc((3.0, 0.0, 0.2)), 0.08)
    inp.scen.log(0, inp.sloc((0.0, 2.0, 0.2)), inp.sloc((0.3, 2.0, 0.2)), 0.05)
    inp.scen.mushroom(0, inp.sloc((1.0, 2.0, 0.2)), 0.05)
    for x in (0.0, 1.0, 2.0, 3.0):
        inp.query((x + 0.05, 0.0, 0.22))
    inp.query((2.3, 0.0, 0.22))    # inside the voxel_rock's own radius, outside the override
    inp.query((0.01, 2.0, 0.2))
    inp.query((1.0, 2.01, 0.2))
    ox, oy = case.origin(1)
    inp.scen.rock(1, inp.sloc((ox + 1.0, oy + 1.0, 0.2)), 0.05)
    inp.query((ox + 1.02, oy + 1.0, 0.2))   # a tile without a rock_shape: the bit stays clear
    return inp


def b_on_axis(case, n):
    """a sphere exactly on a stump's axis, on a pine's, on a deciduous trunk's and exactly on a rock's centre: get_norm() of a zero vector"""
    inp = Inputs(case)
    inp.scen.stump(0, inp.sloc((0.0, 0.0, 0.0)), 0.03, 0.3)
    inp.scen.rock(0, inp.sloc((1.0, 0.0, 0.25)), 0.05)
    inp.tree(0, (2.0, 0.0, 0.1))
    inp.dtree(0, (3.0, 0.0, 0.0))
    inp.query((0.0, 0.0, 0.2))
    inp.query((1.0, 0.0, 0.25))
    inp.query((2.0, 0.0, Z))
    inp.query((3.0, 0.0, Z))
    return inp


def b_stages(case, n):
    """every stage at which a query leaves, in both forms"""
    inp = Inputs(case)
    inp.flags = np.zeros(n, np.uint8)
    inp.flags[2] = cm.TILE_DISTANT
    for t in range(n):
        ox, oy = case.origin(t)
        inp.tree(t, (ox + 4.0, oy + 4.0, 0.1))
    nan, inf = float("nan"), float("inf")
    o1, o2 = case.origin(1), case.origin(2)
    inp.query((o1[0] + 4.03, o1[1] + 4.0, Z))            # tile 1: tested, a hit
    inp.query((20.0, 0.0, Z))                            # no tile there
    inp.query((o2[0] + 4.03, o2[1] + 4.0, Z))            # the distant tile
    inp.query((o2[0] + 4.03, o2[1] + 4.0, Z), tile=2)
    inp.query((0.03, 0.0, Z), tile=1)                    # tile_t's form with a position outside that tile
    inp.query((0.03, 0.0, 0.5 + R + 0.01))               # above get_tile_zmax() + radius
    inp.query((0.03, 0.0, float(f32(0.5) + f32(R))))     # at it: not above
    for bad in ((nan, 0.0, Z), (0.0, inf, Z), (0.0, 0.0, -inf)):
        inp.query(bad)
        inp.query(bad, tile=0)
    inp.query((0.03, 0.0, Z), nan)
    inp.query((0.03, 0.0, Z), inf)
    inp.query((0.03, 0.0, Z), -0.5)
    inp.query((0.03, 0.0, Z), 0.0)                       # radius 0 is a query
    inp.query((1.0e30, 0.0, Z))                          # round_fp beyond the int range
    inp.query((0.0, -3.0e38, Z))
    return inp


def b_out_of_range(case, n):
    """a query's tile outside [-1, n); records whose tree_id / inst lie outside their tables, at the centre of queries: answered, nothing out of range is read"""
    inp = Inputs(case)
    inp.tree(0, (0.0, 0.0, 0.1), PINE, inst=5000)
    inp.tree(0, (1.0, 0.0, 0.1), PINE, inst=2 if not case.instanced else -1)
    inp.tree(0, (2.0, 0.0, 0.1), 9)
    inp.tree(0, (3.0, 0.0, 0.1), -2)
    inp.tree(0, (-1.0, 0.0, 0.1), PINE, inst=0 if case.instanced else -1)
    for k, tid in enumerate((99, -3, TABLE, 2**31 - 1, dvc.NOT_GEN, dvc.PLAIN)):
        inp.dtree(0, (float(k) - 2.0, 1.0, 0.0), tid)
    for x in (0.0, 1.0, 2.0, 3.0, -1.0):
        inp.query((x + 0.03, 0.0, Z))
    for k in range(6):
        inp.query((float(k) - 2.0 + 0.03, 1.0, Z))
    for tile in (n, n + 5, -2, -2**31, 2**31 - 1):
        inp.query((0.03, 0.0, Z), tile=tile)
    inp.scen.add(0, 17, inp.sloc((0.0, 2.0, 0.2)), 0.2)   # no such kind
    inp.scen.add(0, -1, inp.sloc((0.0, 2.0, 0.2)), 0.2)
    inp.query((0.03, 2.0, 0.2))
    return inp


def b_borders(case, n):
    """the lookup on all four sides of a tile border, at negative tile coordinates: the four tiles around the corner (-4, -4) of tile (0, 0), each with a pine a
    step from the corner"""
    inp = Inputs(case)
    inp.trmax = np.full(n, 0.05, f32)
    cx, cy = -4.0 + case.dx() * case.dxoff, -4.0 + case.dx() * case.dyoff
    for sx in (-1, 1):
        for sy in (-1, 1):
            t = case.tiles.index(((0 if sx > 0 else -1), (0 if sy > 0 else -1)))
            inp.tree(t, (cx + 0.03 * sx, cy + 0.03 * sy, 0.1))
            for e in (1.0e-6, 0.001, 0.03):
                inp.query((cx + e * sx, cy + e * sy, Z))
            inp.query((cx + 0.03 * sx, cy + 0.03 * sy, Z), tile=(t + 1) % n)  # the neighbour's box reaches over by trmax
    inp.query((cx, cy, Z))
    inp.query((cx, cy + 1.0, Z))
    inp.query((cx - 8.0 + 0.001, cy - 8.0 + 0.001, Z))
    inp.query((cx - 8.0 - 0.001, cy, Z))
    return inp


def b_inc(case, n):
    """all eight inc_* combinations on one position that meets all three containers in turn; tile 1: !scenery.generated"""
    inp = Inputs(case)
    inp.flags = np.zeros(n, np.uint8)
    inp.flags[1] = cm.TILE_NO_SCENERY
    for t in range(2):
        ox, oy = case.origin(t)
        inp.tree(t, (ox + 2.0, oy + 2.0, 0.1))
        inp.dtree(t, (ox + 2.23, oy + 2.0, 0.0))
        inp.scen.stump(t, inp.sloc((ox + 2.08, oy + 2.1, 0.0)), 0.03, 0.4)
        for fl in range(8):
            inp.query((ox + 2.05, oy + 2.0, 0.25), flags=fl)
    inp.query((case.origin(0)[0] + 2.05, case.origin(0)[1] + 2.0, 0.25), flags=0xFFFFFFF8)  # no known bit
    return inp


def scatter_all(inp, t, m, rng, spread=2.0):
    """m records of each container over a spread x spread patch of tile t: dense enough that a sphere meets several"""
    ox, oy = inp.case.origin(t)
    u = lambda: (ox + 3.0 + float(rng.uniform(0.0, spread)), oy + 3.0 + float(rng.uniform(0.0, spread)))  # noqa: E731
    for k in range(m):
        x, y = u()
        inp.tree(t, (x, y, 0.1), (PINE, PINE, PALM, SH_PINE, BUSH)[k % 5], height=float(rng.uniform(0.3, 0.6)), width=float(rng.uniform(0.1, 0.2)))
        x, y = u()
        inp.dtree(t, (x, y, 0.0), int(rng.integers(0, TABLE)))
        x, y = u()
        kind = k % 9
        pos = inp.sloc((x, y, 0.15))
        if kind == svc.ROCK_SHAPE:
            inp.scen.rock_shape(t, pos, override=0.08 if k % 2 else None)
        elif kind == svc.STUMP:
            inp.scen.stump(t, pos, 0.04, 0.3)
        elif kind == svc.PLANT:
            inp.scen.plant(t, pos, 0.02, 0.3)
        elif kind == svc.LOG:
            inp.scen.log(t, pos, (pos[0] + 0.2, pos[1], pos[2]), 0.04)
        elif kind == svc.MUSHROOM:
            inp.scen.mushroom(t, pos, 0.04)
        else:
            inp.scen.add(t, kind, pos, 0.08)


def b_many_queries(case, n):
    """70 queries in one tile (more than a wave, more than a workgroup's four) / 300 over 4 tiles, in both forms, over dense records"""
    m = 60
    inp = Inputs(case, pcap=m, dcap=m, scap=m)
    rng = np.random.default_rng(17 + n)
    for t in range(n):
        scatter_all(inp, t, m, rng)
    nq = 70 if n == 1 else 300
    for k in range(nq):
        t = k % n
        ox, oy = case.origin(t)
        pos = (ox + 3.0 + float(rng.uniform(-0.2, 2.2)), oy + 3.0 + float(rng.uniform(-0.2, 2.2)), float(rng.uniform(0.1, 0.45)))
        inp.query(pos, float(rng.uniform(0.05, 0.2)), (t + (k % 7 == 0)) % n if k % 3 == 0 else -1, ALL if k % 4 else int(rng.integers(0, 8)))
    return inp


def b_offsets(case, n):
    """three different translations: the three objects of inc_combinations, met through dxoff / dyoff and three xoff2 / yoff2 pairs"""
    inp = Inputs(case)
    inp.cube_tile = []
    for t in range(n):
        ox, oy = case.origin(t)
        inp.tree(t, (ox + 2.0, oy + 2.0, 0.1))
        inp.dtree(t, (ox + 2.23, oy + 2.0, 0.0))
        inp.scen.stump(t, inp.sloc((ox + 2.08, oy + 2.1, 0.0)), 0.03, 0.4)
        inp.query((ox + 2.05, oy + 2.0, 0.25))
        inp.query((ox + 2.05, oy + 2.0, 0.25), tile=t)
        inp.cube((ox + 2.23, oy + 2.0, 0.3), tile=-1)
    return inp


def b_cubes(case, n):
    """the cube call: the all_bcube cull, leaves box only, branches box only, boxes hit but the sphere missed, a hit, no tile, an empty container (tile 1), an
    explicit tile, a bad cube.  Entry 0's leaves box is +-0.3 x +-0.3 x 0.125 .. 0.75, its branches box +-0.2 x +-0.2 x 0 .. 0.625, its sphere 0.3 about z 0.375"""
    inp = Inputs(case)
    inp.cube_tile = []
    inp.dtree(0, (0.0, 0.0, 0.0))
    inp.dtree(0, (2.0, 0.0, 0.0), dvc.BIG)
    inp.dtree(0, (0.0, 2.0, 0.0), 99)              # dropped
    inp.cube((-3.0, -3.0, 0.3), tile=-1)                        # outside all_bcube
    inp.cube((0.28, 0.0, 0.7), (0.01, 0.01, 0.01), tile=-1)     # the leaves box alone, outside the sphere
    inp.cube((0.0, 0.0, 0.05), (0.15, 0.15, 0.04), tile=-1)     # the branches box alone (below the leaves box), inside the sphere: a hit
    inp.cube((0.28, 0.28, 0.72), (0.015, 0.015, 0.02), tile=-1)  # a corner of the leaves box: a box hit, the sphere missed
    inp.cube((0.0, 0.0, 0.4), tile=-1)                          # a hit
    inp.cube((1.0, 0.0, 0.4), tile=-1)                          # inside all_bcube, between the trees: no box
    inp.cube((0.0, 2.0, 0.3), tile=-1)                          # at the dropped record
    inp.cube((30.0, 0.0, 0.3), tile=-1)                         # no tile
    ox, oy = case.origin(1)
    inp.cube((ox + 1.0, oy + 1.0, 0.3), tile=-1)                # tile 1 holds no tree
    inp.cube((float("nan"), 0.0, 0.3), tile=-1)
    inp.cube((ox + 1.0, oy + 1.0, 0.3), tile=0)    # tile 0 asked about a cube that lies over tile 1
    inp.cube((0.0, 0.0, 0.4), tile=1)              # and the other way round
    inp.cube((0.0, 0.0, 0.4), tile=7)              # no such tile
    inp.cube((0.0, 0.0, 0.4), tile=-9)
    return inp


def b_cubes_flat(case, n):
    """an all_bcube of zero area never culls; no cube_tile array: every tile from the cube's centre"""
    inp = Inputs(case)
    inp.dtree(0, (0.0, 0.0, 0.0), dvc.FLAT)
    inp.cube((3.0, 3.0, 0.3))
    inp.cube((0.0, 0.0, 0.4), (0.01, 0.01, 0.01))
    return inp


def b_s128(case, n):
    """the tile size of the product: the same objects at S = 128 with offsets"""
    inp = b_offsets(case, n)
    rng = np.random.default_rng(23)
    for t in range(n):
        ox, oy = case.origin(t)
        for k in range(20):
            inp.query((ox + 2.0 + float(rng.uniform(-0.2, 0.4)), oy + 2.0 + float(rng.uniform(-0.2, 0.3)), float(rng.uniform(0.1, 0.4))), float(rng.uniform(0.05, 0.2)))
    return inp


QUAD = [(0, 0), (-1, 0), (0, -1), (-1, -1)]
HIT_ALL3 = cm.HIT_PINE | cm.HIT_DECID | cm.HIT_SCENERY
HIT_OF_INC = [(cm.HIT_DECID if f & cm.INC_DTREES else 0) | (cm.HIT_PINE if f & cm.INC_PTREES else 0) | (cm.HIT_SCENERY if f & cm.INC_SCENERY else 0) for f in range(8)]


def cases():
    return [
        Case("chain_in_one_chunk", [(0, 0)], b_chain_pine, check=lambda t, h: t["chain_created"] == 1 and t["chain_removed"] == 1 and h["nhits"].tolist() == [2, 1]),
        Case("chain_across_containers", [(0, 0)], b_chain_across,
             check=lambda t, h: t["chain_created_across"] == 2 and h["word"].tolist() == [cm.HIT_PINE | cm.HIT_DECID, cm.HIT_DECID | cm.HIT_SCENERY]),
        Case("scenery_kind_order", [(0, 0)], b_kind_order, check=lambda t, h: t["chain_removed"] >= 1 and t["hits_by_kind"][svc.ROCK] == 1 and t["hits_scenery"] >= 3),
        Case("lane_63_then_64", [(0, 0)], b_lane63, check=lambda t, h: h["nhits"].tolist() == [2, 1, 1] and t["chain_created"] == 1),
        Case("count_above_capacity", [(0, 0)], b_over_capacity, check=lambda t, h: t["queries_hit"] == 12 and h["nhits"][-1] == 0),
        Case("row_of_stumps", [(0, 0)], b_stump_row, check=lambda t, h: h["nhits"].tolist() == [70]),
        Case("round_trip_alone", [(0, 0)], b_round_trip, dxoff=3, dyoff=-5, poff2=(7, 2), doff2=(-4, 9), soff2=(1, -6),
             check=lambda t, h: t["round_trip_only"] >= 5 and t["queries_hit"] == 0 and t["gate_exit_pine"] >= 10 and t["gate_exit_decid"] >= 10),
        Case("bcube_gates", [(0, 0), (1, 0)], b_gates,
             check=lambda t, h: min(t["gate_exit_pine"], t["gate_pass_pine"], t["gate_exit_decid"], t["gate_pass_decid"], t["gate_zero_area_pine"], t["gate_zero_area_decid"], t["bush"]) >= 1),
        Case("short_tree", [(0, 0)], b_short_tree, check=lambda t, h: t["short_tree_exit"] == 1 and t["short_tree_extended"] == 1 and h["nhits"].tolist() == [0, 1, 1, 1, 0]),
        Case("rotated_palm", [(0, 0)], b_palm, check=lambda t, h: t["rotated"] == 1 and h["nhits"].tolist() == [1, 1, 1, 0] and float(h["pos"][0][0]) < 0.0),
        Case("rocks_logs_mushrooms", [(0, 0), (1, 0)], b_rocks,
             check=lambda t, h: t["rock_shape_override"] == 1 and t["voxel_rock_override"] == 1 and t["log_in_reach"] >= 1 and t["mushroom_in_reach"] >= 1
             and h["nhits"].tolist() == [1, 0, 1, 1, 0, 0, 0, 1] and [int(w) & cm.ROCK_SHAPE_UNDECIDED for w in h["word"]] == [8] * 7 + [0]),
        Case("zero_normals", [(0, 0)], b_on_axis, check=lambda t, h: t["zero_normal"] == 4 and h["nhits"].tolist() == [1, 1, 1, 1]),
        Case("stages", [(0, 0), (1, 0), (0, 1)], b_stages,
             check=lambda t, h: min(t["tested"], t["outside"], t["above"]) >= 1 and t["distant"] == 2 and t["bad_query"] == 9 and t["no_tile"] >= 3),
        Case("out_of_range", [(0, 0), (1, 0)], b_out_of_range, check=lambda t, h: t["tile_out_of_range"] == 5 and t["dropped_pine"] == 4 and t["dropped_decid"] == 5 and t["queries_hit"] == 2),
        Case("out_of_range_instanced", [(0, 0), (1, 0)], b_out_of_range, instanced=True, ninst=(4, 4),
             check=lambda t, h: t["tile_out_of_range"] == 5 and t["dropped_pine"] == 3 and t["queries_hit"] == 3),
        Case("tile_borders", QUAD, b_borders, check=lambda t, h: t["looked_up"] >= 12 and t["queries_hit"] >= 8 and sorted(set(h["tile"].tolist())) == [-1, 0, 1, 2, 3]),
        Case("tile_borders_offset", QUAD, b_borders, dxoff=-37, dyoff=22, poff2=(5, -3), check=lambda t, h: t["queries_hit"] >= 8 and sorted(set(h["tile"].tolist())) == [-1, 0, 1, 2, 3]),
        Case("inc_combinations", [(0, 0), (5, -7)], b_inc, check=lambda t, h: len(set(h["word"][:8].tolist())) >= 6 and h["word"][7] == HIT_ALL3 and all(not int(h["word"][k]) & ~HIT_OF_INC[k % 8] for k in range(16))
             and t["no_scenery"] == 4 and t["chain_created_across"] >= 2),
        Case("seventy_queries", [(0, 0)], b_many_queries, check=lambda t, h: t["queries"] == 70 and t["multi_hit_queries"] >= 10 and t["chain_created"] + t["chain_removed"] >= 5),
        Case("three_hundred_queries", QUAD, b_many_queries,
             check=lambda t, h: t["queries"] == 300 and t["multi_hit_queries"] >= 40 and min(t["hits_pine"], t["hits_decid"], t["hits_scenery"]) >= 20 and t["outside"] >= 1),
        Case("three_translations", [(0, 0), (1, 0), (-3, 2)], b_offsets, dxoff=11, dyoff=-4, poff2=(3, 8), doff2=(-6, 1), soff2=(2, -9),
             check=lambda t, h: (h["word"] == HIT_ALL3).all() and t["cube_hit"] == 3),
        Case("cubes", [(0, 0), (1, 0)], b_cubes,
             check=lambda t, h: min(t["cube_culled"], t["cube_leaves_only"], t["cube_branches_only"], t["cube_sphere_missed"], t["cube_hit"], t["cube_empty"], t["cube_bad"],
                                    t["cube_boxes_missed"]) >= 1 and t["cube_no_tile"] >= 3),
        Case("cubes_zero_area", [(0, 0)], b_cubes_flat, check=lambda t, h: t["cube_zero_area"] == 2 and t["cube_culled"] == 0),
        Case("s128_offsets", [(0, 0), (1, 0), (-3, 2)], b_s128, S=128, dxoff=-70, dyoff=33, poff2=(3, 8), doff2=(-6, 1), soff2=(2, -9),
             check=lambda t, h: t["queries_hit"] >= 20 and min(t["hits_pine"], t["hits_decid"], t["hits_scenery"]) >= 5 and t["cube_hit"] == 3),
    ]


# ---- the model and the library on a case
MODEL = {}


def globals_of(case):
    insts = trc.inst_table(*case.ninst) if case.instanced else None
    return vm.Globals(tam.SizeParams(tree_scale=case.tree_scale), vm.Args(tree_depth_scale=case.tree_depth_scale), case.instanced, insts)


def batch_of(sc, g, case, stats, inp, tally=None, **kw):
    return cm.Batch(sc, g, case.tiles, stats, inp.trmax, inp.tile_zmax, inp.flags, None if inp.pine is None else inp.pine.pine, None if inp.pine is None else inp.pine.counts,
                    None if inp.pine is None else inp.pine.override, inp.decid, inp.decid_counts, inp.data, inp.br_scale, None if inp.scen is None else inp.scen.objs,
                    None if inp.scen is None else inp.scen.counts, None if inp.scen is None else inp.scen.override, case.poff2, case.doff2, case.soff2, tally, **kw)


def model(orc, case):
    """(scene, globals, stats, inputs, hits, (cube result, cube tile), tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
        orc.init(ocfg)
        sc = tm.Scene(orc, ocfg, case.dxoff, case.dyoff)
        assert float(sc.DX_VAL) == case.dx() and float(sc.g.X_SCENE_SIZE) == 4.0
        stats = tvc.stats_of(orclib, case, float(sc.water_plane_z))
        g = globals_of(case)
        inp = case.build(case, len(case.tiles))
        b = batch_of(sc, g, case, stats, inp)
        hits = b.sphere_collide(inp.query_array())
        cubes = b.cube_int_trees(np.array(inp.cubes, f32).reshape(-1, 6), inp.cube_tile)
        MODEL[case.name] = (sc, g, stats, inp, hits, cubes, b.tally)
    return MODEL[case.name]


def configure(pkg, t, case, g):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_scale=case.tree_scale, instanced=case.instanced, num_pine_insts=case.ninst[0], num_palm_insts=case.ninst[1]))
    t.set_tree_size_params(pkg.make_tree_size_params())
    t.set_tree_instances(g.insts)
    t.set_decid_params(pkg.make_decid_params(num_trees=100, num_shared_trees=TABLE))


def host_arrays(pkg, case, stats, inp):
    """the array arguments of make_collide_in, as host arrays"""
    n = len(case.tiles)
    kw = dict(stats=(pkg.TileStats * n).from_buffer_copy(stats), trmax=inp.trmax, tile_zmax=inp.tile_zmax, flags=inp.flags, tree_data=inp.data, br_scale=inp.br_scale)
    if inp.pine is not None:
        kw.update(pine=inp.pine.pine, pine_counts=inp.pine.counts, trunk_override=inp.pine.override)
    if inp.decid is not None:
        kw.update(decid=inp.decid, decid_counts=inp.decid_counts)
    if inp.scen is not None:
        kw.update(scenery=inp.scen.objs, scenery_counts=inp.scen.counts, radius_override=inp.scen.override)
    return kw


def scalars(case):
    return dict(dxoff=case.dxoff, dyoff=case.dyoff, ptree_xoff2=case.poff2[0], ptree_yoff2=case.poff2[1], dtree_xoff2=case.doff2[0], dtree_yoff2=case.doff2[1],
                scenery_xoff2=case.soff2[0], scenery_yoff2=case.soff2[1], tree_depth_scale=case.tree_depth_scale)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1) if isinstance(a, np.ndarray) else np.frombuffer(bytes(memoryview(a).cast("B")), np.uint8)


class DeviceInputs:
    """the arrays of a make_collide_in uploaded: .cin holds device addresses"""

    def __init__(self, pkg, t, kw, sc):
        self.bufs, dev = {}, {}
        caps = {k + "_capacity": (kw[k].shape[1] if kw.get(k) is not None else 0) for k in ("pine", "decid", "scenery")}
        for k, a in kw.items():
            if a is None:
                continue
            b = as_bytes(a)
            self.bufs[k] = t.alloc(max(b.nbytes, 4))
            if b.nbytes:
                self.bufs[k].upload(b)
            dev[k] = self.bufs[k].ptr
        self.cin = pkg.make_collide_in(num_tree_data=len(kw["tree_data"]), **caps, **dev, **sc)

    def free(self):
        for b in self.bufs.values():
            b.free()


def run_sphere(pkg, t, case, stats, inp, dev):
    q = inp.query_array()
    kw, sc = host_arrays(pkg, case, stats, inp), scalars(case)
    if not dev:
        return t.tiles_sphere_collide(case.tiles, pkg.make_collide_in(**kw, **sc), q)
    d = DeviceInputs(pkg, t, kw, sc)
    nb = max(q.nbytes, 4)
    qb, hb = t.alloc(nb), t.alloc(nb).upload(np.full(nb, FILL, np.uint8))
    try:
        if q.nbytes:
            qb.upload(as_bytes(q))
        t.tiles_sphere_collide_dev(case.tiles, d.cin, qb.ptr, len(q), hb.ptr)
        return hb.download(np.uint8, (nb,)).copy()[:q.nbytes].view(cm.HIT_DTYPE)
    finally:
        d.free()
        qb.free()
        hb.free()


def run_cubes(pkg, t, case, stats, inp, dev):
    cubes = np.array(inp.cubes, f32).reshape(-1, 6)
    ct = None if inp.cube_tile is None else np.array(inp.cube_tile, np.int32)
    kw, sc = host_arrays(pkg, case, stats, inp), scalars(case)
    if not dev:
        return t.tiles_cube_int_trees(case.tiles, pkg.make_collide_in(**kw, **sc), cubes, ct)
    d = DeviceInputs(pkg, t, kw, sc)
    nq = len(cubes)
    cb, rb, tb = t.alloc(cubes.nbytes).upload(as_bytes(cubes)), t.alloc(nq + 4).upload(np.full(nq + 4, FILL, np.uint8)), t.alloc(nq * 4).upload(np.full(nq * 4, FILL, np.uint8))
    ctb = None if ct is None else t.alloc(ct.nbytes).upload(as_bytes(ct))
    try:
        t.tiles_cube_int_trees_dev(case.tiles, d.cin, cb.ptr, nq, rb.ptr, None if ctb is None else ctb.ptr, tb.ptr)
        res = rb.download(np.uint8, (nq + 4,)).copy()
        assert (res[nq:] == FILL).all(), "result bytes written past nq"
        return res[:nq], tb.download(np.int32, (nq,)).copy()
    finally:
        d.free()
        for b in (cb, rb, tb, ctb):
            if b is not None:
                b.free()


def compare_hits(what, got, want, queries):
    assert got.dtype == cm.HIT_DTYPE and len(got) == len(want)
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), f"{what}: query {i} {queries[i]}: {got[i]} != {want[i]}"


def run_case(pkg, t, orc, case, dev=False):
    sc, g, stats, inp, hits, (cres, ctile), tally = model(orc, case)
    assert case.check(tally, hits), (case.name, {k: x for k, x in tally.items() if x}, hits.tolist())
    configure(pkg, t, case, g)
    what = case.name + (" (dev)" if dev else "")
    if len(inp.queries):
        compare_hits(what, run_sphere(pkg, t, case, stats, inp, dev), hits, inp.queries)
    if len(inp.cubes):
        res, tile = run_cubes(pkg, t, case, stats, inp, dev)
        assert res.tolist() == cres.tolist() and tile.tolist() == ctile.tolist(), f"{what}: cubes {res.tolist()} {tile.tolist()} != {cres.tolist()} {ctile.tolist()}"


# ---- the resident chain: zvals -> the three placements -> collide
def run_resident_chain(pkg, t, orc):
    """tiles_create_zvals_dev (zvals, stats) -> tiles_place_trees_dev, tiles_place_decid_trees_dev, tiles_place_scenery_dev -> tiles_sphere_collide_dev and
    tiles_cube_int_trees_dev on a 3 x 3 batch at S = 128 on one context, the containers staying where the placements left them.  The queries are drawn around the
    placed records (an engine draws its queries from its own objects), so the records are read back once before the collide calls; the model is fed from the same
    read-back records"""
    S, pcap, dcap, scap, shared = 128, 320, 384, 160, 16
    tiles = [(x, y) for y in range(-1, 2) for x in range(1, 4)]  # over the island's shore
    n, Zs = len(tiles), S + 2
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S))
    t.set_landscape(pkg.make_landscape(grass_density=1, vegetation=1.0))
    t.set_tree_params(pkg.make_tree_params(tree_mode=3, tree_type_rand_zone=0.02))
    t.set_decid_params(pkg.make_decid_params(num_trees=400, num_shared_trees=shared))
    t.set_scenery_params(pkg.make_scenery_params(1))
    t.set_tree_size_params(pkg.make_tree_size_params())
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=S)
    orc.init(ocfg)
    sc = tm.Scene(orc, ocfg)
    data = dvc.make_table(shared)
    data["flags"][dvc.NOT_GEN] |= dvc.GEN
    for k in ("base_radius", "sphere_radius", "sphere_center_zoff", "lr_z_cent", "leaves_bcube", "branches_bcube"):  # trees of TREE_SIZE's order
        data[k] = (data[k] * f32(0.2)).astype(f32)
    br_scale = np.array([1.0 + 0.05 * (k % 5) for k in range(shared)], f32)
    sizes = dict(z=n * Zs * Zs * 4, st=n * C.sizeof(pkg.TileStats), pt=n * pcap * pkg.TREE_PLACE_DTYPE.itemsize, pc=n * 4, de=n * dcap * pkg.DECID_PLACE_DTYPE.itemsize, dc=n * 4,
                 ob=n * scap * pkg.SCENERY_PLACE_DTYPE.itemsize, oc=n * 4)
    bufs = {k: t.alloc(b) for k, b in sizes.items()}
    bufs["td"], bufs["br"] = t.alloc(data.nbytes).upload(data.view(np.uint8)), t.alloc(br_scale.nbytes).upload(br_scale)
    try:
        p = {k: b.ptr for k, b in bufs.items()}
        for k in ("pt", "de", "ob"):
            bufs[k].upload(np.zeros(sizes[k], np.uint8))
        t.tiles_create_zvals_dev(tiles, 0, p["z"], p["st"])
        t.tiles_place_trees_dev(tiles, pcap, p["pt"], p["pc"], 0, 0, None, p["st"])
        t.tiles_place_decid_trees_dev(tiles, dcap, p["de"], p["dc"], 0, 0, None, p["st"], p["z"])
        t.tiles_place_scenery_dev(tiles, scap, p["ob"], p["oc"])
        stats = (pkg.TileStats * n).from_buffer_copy(bufs["st"].download(np.uint8, (sizes["st"],)).tobytes())
        pine = bufs["pt"].download(np.uint8, (sizes["pt"],)).copy().view(pkg.TREE_PLACE_DTYPE).reshape(n, pcap)
        decid = bufs["de"].download(np.uint8, (sizes["de"],)).copy().view(pkg.DECID_PLACE_DTYPE).reshape(n, dcap)
        objs = bufs["ob"].download(np.uint8, (sizes["ob"],)).copy().view(pkg.SCENERY_PLACE_DTYPE).reshape(n, scap)
        pc, dc, oc = (bufs[k].download(np.uint32, (n,)).copy() for k in ("pc", "dc", "oc"))
        # the queries: around the placed records, a step off their axes; a third name their tile.  get_tile_zmax(): above every tree (ptzmax / dtzmax are the engine's)
        rng = np.random.default_rng(29)
        queries, cubes = [], []
        tile_zmax = np.array([float(stats[i].mzmax) + 1.0 for i in range(n)], f32)
        for i in range(n):
            for recs, cnt in ((pine[i], pc[i]), (decid[i], dc[i]), (objs[i], oc[i])):
                m = min(int(cnt), len(recs))
                for j in (rng.choice(m, min(m, 14), replace=False) if m else []):
                    x, y, z = (float(v) for v in recs[j]["pos"])
                    queries.append(((x + float(rng.uniform(-0.04, 0.04)), y + float(rng.uniform(-0.04, 0.04)), z + float(rng.uniform(0.0, 0.06))), float(rng.uniform(0.03, 0.09)),
                                    i if len(queries) % 3 == 0 else -1, ALL))
            for j in range(min(int(dc[i]), dcap, 6)):
                x, y, z = (float(v) for v in decid[i, j]["pos"])
                cubes.append([x - 0.02, x + 0.05, y - 0.03, y + 0.03, z + 0.02, z + 0.09])
                cubes.append([x + 0.5, x + 0.55, y - 0.03, y + 0.03, z + 0.02, z + 0.09])
        q = np.zeros(len(queries), cm.QUERY_DTYPE)
        for i, row in enumerate(queries):
            q[i] = row
        cubes = np.array(cubes, f32).reshape(-1, 6)
        bufs["zm"] = t.alloc(tile_zmax.nbytes).upload(tile_zmax)
        bufs["q"], bufs["h"] = t.alloc(q.nbytes).upload(as_bytes(q)), t.alloc(q.nbytes).upload(np.full(q.nbytes, FILL, np.uint8))
        bufs["cu"], bufs["cr"], bufs["ct"] = t.alloc(cubes.nbytes).upload(as_bytes(cubes)), t.alloc(len(cubes)), t.alloc(len(cubes) * 4)
        cin = pkg.make_collide_in(stats=p["st"], tile_zmax=bufs["zm"].ptr, pine=p["pt"], pine_counts=p["pc"], decid=p["de"], decid_counts=p["dc"], scenery=p["ob"],
                                  scenery_counts=p["oc"], tree_data=bufs["td"].ptr, br_scale=bufs["br"].ptr, pine_capacity=pcap, decid_capacity=dcap, scenery_capacity=scap,
                                  num_tree_data=shared)
        t.tiles_sphere_collide_dev(tiles, cin, bufs["q"].ptr, len(q), bufs["h"].ptr)
        t.tiles_cube_int_trees_dev(tiles, cin, bufs["cu"].ptr, len(cubes), bufs["cr"].ptr, None, bufs["ct"].ptr)
        got = bufs["h"].download(np.uint8, (q.nbytes,)).copy().view(cm.HIT_DTYPE)
        cres, ctile = bufs["cr"].download(np.uint8, (len(cubes),)).copy(), bufs["ct"].download(np.int32, (len(cubes),)).copy()
    finally:
        for b in bufs.values():
            b.free()
    b = cm.Batch(sc, vm.Globals(tam.SizeParams(), vm.Args()), tiles, stats, None, tile_zmax, None, pine, pc, None, decid, dc, data, br_scale, objs, oc, None)
    want = b.sphere_collide(q)
    compare_hits("resident chain", got, want, queries)
    wres, wtile = b.cube_int_trees(cubes)
    assert cres.tolist() == wres.tolist() and ctile.tolist() == wtile.tolist()
    tally = b.tally
    assert len(q) >= 200 and min(tally["hits_pine"], tally["hits_decid"], tally["hits_scenery"]) >= 5 and tally["chain_created"] + tally["chain_removed"] >= 1 and tally["cube_hit"] >= 5, \
        ({k: x for k, x in tally.items() if x}, pc.tolist(), dc.tolist(), oc.tolist())
    return tally
