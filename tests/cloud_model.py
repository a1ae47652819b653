"""NumPy / Python float32 restatement of the tile clouds, written from the reference statements (not from the library's bodies):

    tile_cloud_t::draw (the decision and alpha)                        src/tiled_mesh.cpp:1691-1697
    tile_cloud_manager_t::gen_new_cloud, gen, choose_num_clouds,
      populate_clouds, try_add_cloud, update_bcube, move_by_wind,
      get_draw_list                                                    src/tiled_mesh.cpp:1710-1820
    tile_t::update_tile_clouds                                         src/tiled_mesh.cpp:1822-1827
    tile_draw_t::draw_tile_clouds (the two loops and the sort)         src/tiled_mesh.cpp:3484-3493
    tile_cloud_t, cloud_inst_t, tile_cloud_manager_t                   src/tiled_mesh.h:116-153
    gen_gauss_rand_arr                                                 src/gen_object.cpp:363-374
    rand_gen_t: rand, randd, rand_uniform, rgauss, rand_gaussian,
      gen_rand_cube_point                                              src/rand_gen.h:20-35, 63-95; src/gen_object.cpp:464-468
    cube_t: set_to_zeros, is_all_zeros, union_with_cube, expand_by     src/3DWorld.h:436, 491, 506, 621
    get_tile_width, get_xval / get_yval, p2p_dist_sq                   src/tiled_mesh.h:93; src/mesh.h:122-123; src/inlines.h:176-178

Leaves from the reference's compiled code (the oracle): the draws of the Gaussian table are ref_rand_ints(rgen_seed, 123); the exact height is ref_eval_points with
no_xyoff = 1; the generator below is pinned to ref_rand_ints / ref_rand_uniforms by test_model_alone.  sphere_visible_test is tests/view_model.py's restatement (the
reference's own, ref_pdu_spheres, is exported by the reference build alone; tests/primitive_cases.py pins the library's sphere test to it).  Types: np.float32 for float, Python float for double, Python int for int / unsigned / long.

Which sub-expressions are double: `+ 2.0`, `0.0*z_range` and `0.9*z_range` of :1727-1728; `(0.01*fticks)*wind.x` (:1761); `2.0*get_tile_width()` (:1765);
`0.5/range.dz()` (:1782); `0.15*move_amt_mag` (:1788); `0.2*i->size.z` (:1809); `1.0*i->size.z` (:1810); `1.0 - (...)` of :1696; RG_NORM, mconst of gen_gauss_rand_arr.
g++ evaluates the arguments of vector3d(a, b, c) from the right: the draw for size.z comes first (:1715).

The batch order stands for the reference's map order.  capacity: a push_back onto a list of `capacity` records stores nothing and sets OVERFLOW; update_bcube still runs.
Equal dist_sq order by (tile, slot).  The tally counts what happened, so that a case can show that it exercises what it is named for."""
import numpy as np

import view_model

f32 = np.float32
N_RAND_DIST, N_RAND_GAUSS = 10000, 10
OVERFLOW = 1
NONE, VFC, BELOW_ZMIN, BELOW_WATER, BELOW_MESH, LISTED = range(6)
cmax, cmin = view_model.cmax, view_model.cmin

CLOUD_DTYPE = np.dtype([("pos_hash", f32), ("pos", f32, 3), ("size", f32, 3), ("pad", np.uint32)])
TILE_DTYPE = np.dtype([("generated", np.uint32), ("flags", np.uint32), ("count", np.uint32), ("num_clouds", np.uint32), ("cur_move_dist", f32), ("pad", np.uint32),
                       ("rseed1", np.int64), ("rseed2", np.int64), ("bcube", f32, 6), ("range", f32, 6)])
INST_DTYPE = np.dtype([("tile", np.uint32), ("slot", np.uint32), ("dist_sq", f32), ("alpha", f32), ("draw_alpha", f32), ("drawn", np.uint32)])

TALLY = ("gen", "gen_no_draw", "gen_clouds", "gen_already", "not_animated", "early_not_generated", "early_zero_wind", "steps", "zero_move_steps", "redraw", "repop_edge",
         "repop_edge_zero_component", "no_repop_inner", "empty_nothing", "moved", "stay", "stay_only_tiles", "to_later", "to_earlier", "diagonal", "drop_hole", "drop_ungenerated",
         "drop_then_generated", "moved_twice", "left_again", "first_left", "swapped_in_left", "fed_before_turn", "fed_after_repop", "overflow_gen", "overflow_imm", "overflow_sticky",
         "vfc", "below_zmin", "below_water", "below_mesh", "listed", "alpha_one_high", "alpha_one_near", "alpha_frac", "exact_evals", "too_distant", "drawn", "ties")


def new_tally():
    return {k: 0 for k in TALLY}


def _cdiv(a, b):  # C's / and % on long
    q = abs(a) // b
    q = -q if a < 0 else q
    return q, a - q * b


class RandGen:
    """rand_gen_t (src/rand_gen.h:20-35, 63-79)"""

    def __init__(self, s1=0, s2=0):
        self.rseed1, self.rseed2 = int(s1), int(s2)

    def advance(self):
        q, r = _cdiv(self.rseed1, 53668)
        self.rseed1 = 40014 * r - 12211 * q
        if self.rseed1 < 0:
            self.rseed1 += 2147483563
        q, r = _cdiv(self.rseed2, 52774)
        self.rseed2 = 40692 * r - 3791 * q
        if self.rseed2 < 0:
            self.rseed2 += 2147483399

    def rand(self):
        self.advance()
        v = self.rseed1 - self.rseed2
        return v + 2147483562 if v < 1 else v

    def randd(self):
        self.advance()
        v = float(self.rseed1) - float(self.rseed2)
        if v < 1:
            v += 2147483562
        return v / 2147483563.

    def rand_uniform(self, a, b):
        a, b = f32(a), f32(b)
        return f32(a + f32(f32(b - a) * f32(self.randd())))


def gauss_table(orc, rgen_seed):
    """gen_gauss_rand_arr: N_RAND_DIST + 2 entries, each ten rand() % 10000 of the generator (rgen_seed, 123) summed in float"""
    RG_NORM = f32(np.sqrt(3.0 / N_RAND_GAUSS))
    mconst, aconst = f32(2.0E-4 * float(RG_NORM)), f32(f32(N_RAND_GAUSS) * RG_NORM)
    draws = orc.rand_ints(rgen_seed, 123, (N_RAND_DIST + 2) * N_RAND_GAUSS).astype(np.int64) % 10000
    out = np.zeros(N_RAND_DIST + 2, f32)
    for i in range(N_RAND_DIST + 2):
        val = f32(0.0)
        for j in range(N_RAND_GAUSS):
            val = f32(val + f32(draws[i * N_RAND_GAUSS + j]))
        out[i] = f32(f32(mconst * val) - aconst)
    return out


class Params:
    def __init__(self, clouds_per_tile=0.5, cloud_height_offset=0.0, rgen_seed=1):
        self.clouds_per_tile, self.cloud_height_offset, self.rgen_seed = f32(clouds_per_tile), f32(cloud_height_offset), int(rgen_seed)


class Step:
    def __init__(self, wind=(0.4, 0.2, 0.0), fticks=1.0, animate=1):
        self.wind, self.fticks, self.animate = [f32(w) for w in wind], f32(fticks), int(animate)


class Scene:
    """the globals the clouds read: the oracle's state after orc.init(cfg)"""

    def __init__(self, orc, cfg, params, capacity):
        st = orc.state()
        self.orc, self.p, self.capacity = orc, params, int(capacity)
        self.S = int(cfg.mesh_x)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y)
        self.DX_VAL, self.DY_VAL = f32(st.DX_VAL), f32(st.DY_VAL)
        self.zmin, self.zmax, self.water_plane_z = f32(st.zmin), f32(st.zmax), f32(st.water_plane_z)
        self.tile_width = f32(self.X_SCENE_SIZE + self.Y_SCENE_SIZE)
        self.gauss = gauss_table(orc, params.rgen_seed)

    def get_xval(self, x):
        return f32(-self.X_SCENE_SIZE + f32(self.DX_VAL * f32(x)))

    def get_yval(self, y):
        return f32(-self.Y_SCENE_SIZE + f32(self.DY_VAL * f32(y)))


class Cloud:
    def __init__(self, pos_hash, pos, size):
        self.pos_hash, self.pos, self.size = f32(pos_hash), [f32(v) for v in pos], [f32(v) for v in size]
        self.moves = 0  # (the tally's: how often this frame)

    def copy(self):
        c = Cloud(self.pos_hash, self.pos, self.size)
        c.moves = self.moves
        return c

    def get_bcube(self):
        return [[f32(self.pos[i] - self.size[i]), f32(self.pos[i] + self.size[i])] for i in range(3)]


class Manager:
    """tile_cloud_manager_t; a fresh one is the all-zero terra_cloud_tile"""

    def __init__(self):
        self.generated, self.flags, self.num_clouds, self.cur_move_dist = 0, 0, 0, f32(0.0)
        self.rgen = RandGen(0, 0)
        self.bcube, self.range = [[f32(0.0)] * 2 for _ in range(3)], [[f32(0.0)] * 2 for _ in range(3)]
        self.clouds = []
        self.fed, self.repopulated, self.empty_at_start = 0, 0, 0  # (the tally's, per frame)

    def update_bcube(self, c):  # :1753-1756
        b = c.get_bcube()
        if all(v == 0.0 for d in self.bcube for v in d):
            self.bcube = b
        else:
            self.bcube = [[cmin(self.bcube[i][0], b[i][0]), cmax(self.bcube[i][1], b[i][1])] for i in range(3)]

    def push_back(self, sc, c, tally, how):
        if len(self.clouds) < sc.capacity:
            self.clouds.append(c)
        else:
            tally[how] += 1
            if self.flags & OVERFLOW:
                tally["overflow_sticky"] += 1  # the bit was set before
            self.flags |= OVERFLOW
        self.update_bcube(c)

    def choose_num_clouds(self, sc):  # :1733-1735
        if sc.p.clouds_per_tile == 0.0:
            self.num_clouds = 0
            return
        g = sc.gauss[self.rgen.rand() % N_RAND_DIST]
        self.num_clouds = int(cmax(f32(0.0), f32(sc.p.clouds_per_tile + f32(f32(4.0) * g))))

    def gen_new_cloud(self, sc, tally):  # :1710-1720
        r = self.rgen
        pos = [r.rand_uniform(self.range[i][0], self.range[i][1]) for i in range(3)]
        sz = r.rand_uniform(0.6, 1.0)
        sy = r.rand_uniform(1.0, 2.0)
        sx = r.rand_uniform(1.0, 2.0)
        m = r.rand_uniform(2.0, 4.0)
        self.push_back(sc, Cloud(pos[0], pos, [f32(sx * m), f32(sy * m), f32(sz * m)]), tally, "overflow_gen")
        tally["gen_clouds"] += 1

    def populate_clouds(self, sc, tally):  # :1737-1743
        assert not self.clouds
        self.bcube = [[f32(0.0)] * 2 for _ in range(3)]
        for _ in range(self.num_clouds):
            self.gen_new_cloud(sc, tally)

    def gen(self, sc, x1, y1, x2, y2, tally):  # :1722-1731
        if self.generated:
            tally["gen_already"] += 1
            return
        self.generated = 1
        self.rgen = RandGen(x1 + 123, y1 + 321)
        z_range = f32(sc.zmax - sc.zmin)
        z_cloud_bot = f32(float(f32(sc.zmax + f32(sc.p.cloud_height_offset * z_range))) + 2.0)
        self.range = [[sc.get_xval(x1), sc.get_xval(x2)], [sc.get_yval(y1), sc.get_yval(y2)],
                      [f32(float(z_cloud_bot) + 0.0 * float(z_range)), f32(float(z_cloud_bot) + 0.9 * float(z_range))]]
        before = (self.rgen.rseed1, self.rgen.rseed2)
        self.choose_num_clouds(sc)
        self.populate_clouds(sc, tally)
        tally["gen"] += 1
        if before == (self.rgen.rseed1, self.rgen.rseed2):
            tally["gen_no_draw"] += 1
        if self.fed < 0:  # it dropped a guest earlier in this frame
            tally["drop_then_generated"] += 1


def move_by_wind(sc, step, tiles, index, mgrs, t, tally):
    """:1758-1797 for tile t of the batch; get_adj_tile(dx, dy) is the batch's tile at (x + dx, y + dy) or None"""
    m = mgrs[t]
    zero = f32(0.0)
    if not m.generated or (step.wind[0] == zero and step.wind[1] == zero and step.wind[2] == zero):
        tally["early_not_generated" if not m.generated else "early_zero_wind"] += 1
        return
    d = 0.01 * float(step.fticks)
    move_amt = [f32(d * float(step.wind[0])), f32(d * float(step.wind[1])), f32(d * 0.0)]
    move_amt_mag = f32(np.sqrt(f32(f32(f32(move_amt[0] * move_amt[0]) + f32(move_amt[1] * move_amt[1])) + f32(move_amt[2] * move_amt[2]))))
    m.cur_move_dist = f32(m.cur_move_dist + move_amt_mag)
    tally["steps"] += 1
    if move_amt_mag == 0.0:
        tally["zero_move_steps"] += 1
    if float(m.cur_move_dist) > 2.0 * float(sc.tile_width):
        m.choose_num_clouds(sc)
        m.cur_move_dist = f32(0.0)
        tally["redraw"] += 1
    adj = lambda dx, dy: index.get((tiles[t][0] + dx, tiles[t][1] + dy))  # noqa: E731
    if not m.clouds and m.num_clouds > 0:
        on_edge, zc = False, False
        for dd in range(2):
            dxy = [0, 0]
            if step.wind[dd] < 0.0:
                dxy[dd] = 1
            elif step.wind[dd] > 0.0:
                dxy[dd] = -1
            else:
                zc = True
            if adj(dxy[0], dxy[1]) is None:
                on_edge = True
                break
        if on_edge:
            m.populate_clouds(sc, tally)
            m.repopulated = 1
            tally["repop_edge"] += 1
            if zc:
                tally["repop_edge_zero_component"] += 1
        else:
            tally["no_repop_inner"] += 1
        return
    if not m.clouds:
        tally["empty_nothing"] += 1
        return
    if m.empty_at_start and m.num_clouds > 0:
        tally["fed_before_turn"] += 1
    ws_mult = f32(0.5 / float(f32(m.range[2][1] - m.range[2][0])))
    m.bcube = [[f32(0.0)] * 2 for _ in range(3)]
    i, left, last_hole = 0, 0, -1
    while i < len(m.clouds):
        c = m.clouds[i]
        wscale = f32(f32(1.5) - f32(ws_mult * f32(c.pos[2] - m.range[2][0])))
        c.pos = [f32(c.pos[k] + f32(wscale * move_amt[k])) for k in range(3)]
        c.pos_hash = f32(float(c.pos_hash) + 0.15 * float(move_amt_mag))
        c.moves += 1
        tally["moved"] += 1
        if c.moves == 2:
            tally["moved_twice"] += 1
        dx = -1 if c.pos[0] < m.range[0][0] else (1 if c.pos[0] > m.range[0][1] else 0)
        dy = -1 if c.pos[1] < m.range[1][0] else (1 if c.pos[1] > m.range[1][1] else 0)
        if dx == 0 and dy == 0:
            m.update_bcube(c)
            tally["stay"] += 1
            i += 1
            continue
        left += 1
        if c.moves >= 2:
            tally["left_again"] += 1
        if i == 0 and last_hole != 0:
            tally["first_left"] += 1
        if last_hole == i and i < len(m.clouds) - 1:
            tally["swapped_in_left"] += 1  # a non-last element left, and the back that took its place leaves too
        last_hole = i if i < len(m.clouds) - 1 else -1
        if dx and dy:
            tally["diagonal"] += 1
        u = adj(dx, dy)
        if u is None:
            tally["drop_hole"] += 1
        elif not mgrs[u].generated:
            tally["drop_ungenerated"] += 1
            mgrs[u].fed = -1
        else:
            tally["to_later" if u > t else "to_earlier"] += 1
            if mgrs[u].repopulated:
                tally["fed_after_repop"] += 1
            mgrs[u].fed = 1
            mgrs[u].push_back(sc, c.copy(), tally, "overflow_imm")  # try_add_cloud (:1745-1751)
        m.clouds[i] = m.clouds[-1]  # std::swap(*i, back()); pop_back(); --i
        m.clouds.pop()
    if left == 0:
        tally["stay_only_tiles"] += 1


def update(sc, step, tiles, mgrs, tally):
    """the first loop of draw_tile_clouds (:3490) in batch order -> num"""
    index = {tuple(xy): t for t, xy in enumerate(tiles)}
    for m in mgrs:
        m.fed, m.repopulated, m.empty_at_start = 0, 0, int(not m.clouds)
        for c in m.clouds:
            c.moves = 0
    num = 0
    for t, (tx, ty) in enumerate(tiles):
        if step.animate:
            move_by_wind(sc, step, tiles, index, mgrs, t, tally)
        else:
            tally["not_animated"] += 1
        x1, y1 = tx * sc.S, ty * sc.S
        mgrs[t].gen(sc, x1, y1, x1 + sc.S, y1 + sc.S, tally)
        num += len(mgrs[t].clouds)
    return num


def pack(sc, mgrs):
    """-> (state TILE_DTYPE [n], clouds CLOUD_DTYPE [n, capacity] with the records up to count; the rest zero)"""
    n = len(mgrs)
    state, clouds = np.zeros(n, TILE_DTYPE), np.zeros((n, sc.capacity), CLOUD_DTYPE)
    for t, m in enumerate(mgrs):
        s = state[t]
        s["generated"], s["flags"], s["count"], s["num_clouds"], s["cur_move_dist"] = m.generated, m.flags, len(m.clouds), m.num_clouds, m.cur_move_dist
        s["rseed1"], s["rseed2"] = m.rgen.rseed1, m.rgen.rseed2
        s["bcube"], s["range"] = [v for d in m.bcube for v in d], [v for d in m.range for v in d]
        for k, c in enumerate(m.clouds):
            clouds[t, k]["pos_hash"], clouds[t, k]["pos"], clouds[t, k]["size"] = c.pos_hash, c.pos, c.size
    return state, clouds


def unpack(state, clouds):
    """managers from arrays (hand-written records)"""
    mgrs = []
    for t in range(len(state)):
        m, s = Manager(), state[t]
        m.generated, m.flags, m.num_clouds, m.cur_move_dist = int(s["generated"]), int(s["flags"]), int(s["num_clouds"]), f32(s["cur_move_dist"])
        m.rgen = RandGen(int(s["rseed1"]), int(s["rseed2"]))
        m.bcube, m.range = [[f32(s["bcube"][2 * i]), f32(s["bcube"][2 * i + 1])] for i in range(3)], [[f32(s["range"][2 * i]), f32(s["range"][2 * i + 1])] for i in range(3)]
        m.clouds = [Cloud(c["pos_hash"], c["pos"], c["size"]) for c in clouds[t, :int(s["count"])]]
        mgrs.append(m)
    return mgrs


class ViewArgs:
    def __init__(self, behind_sphere_mult=1.0, xlate=(0.0, 0.0, 0.0), max_dist=100.0):
        self.behind_sphere_mult, self.xlate, self.max_dist = f32(behind_sphere_mult), [f32(v) for v in xlate], f32(max_dist)


def view(sc, v, a, tiles, stats, mgrs, tally):
    """get_draw_list for every tile in batch order (:3491, :1799-1820), the sort (:3493), tile_cloud_t::draw's decision (:1693-1696)
    -> (stage uint8 [n, capacity], list INST_DTYPE [count])"""
    n = len(tiles)
    stage = np.zeros((n, sc.capacity), np.uint8)
    found = []
    for t, m in enumerate(mgrs):
        mesh_zmin, mesh_zmax = f32(stats[t].mzmin), f32(stats[t].mzmax)
        for k, c in enumerate(m.clouds):
            pt = [f32(c.pos[i] + a.xlate[i]) for i in range(3)]
            rmax = cmax(c.size[0], cmax(c.size[1], c.size[2]))
            if not view_model.sphere_visible_test(v, a.behind_sphere_mult, pt, rmax):
                stage[t, k] = VFC
                tally["vfc"] += 1
                continue
            zbot = f32(c.pos[2] - c.size[2])
            if zbot < mesh_zmin:
                stage[t, k] = BELOW_ZMIN
                tally["below_zmin"] += 1
                continue
            if float(zbot) + 0.2 * float(c.size[2]) < float(sc.water_plane_z):
                stage[t, k] = BELOW_WATER
                tally["below_water"] += 1
                continue
            start_dist = f32(1.0 * float(c.size[2]))
            alpha = f32(1.0)
            if zbot < f32(mesh_zmax + start_dist):
                tally["exact_evals"] += 1
                dist = f32(zbot - sc.orc.eval_points([[c.pos[0], c.pos[1]]], True, no_xyoff=True)[0])
                if dist < 0.0:
                    stage[t, k] = BELOW_MESH
                    tally["below_mesh"] += 1
                    continue
                if dist < start_dist:
                    alpha = f32(dist / start_dist)
                    tally["alpha_frac"] += 1
                else:
                    tally["alpha_one_near"] += 1
            else:
                tally["alpha_one_high"] += 1
            stage[t, k] = LISTED
            tally["listed"] += 1
            d = [f32(v.pos[i] - pt[i]) for i in range(3)]
            dsq = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
            view_dist = f32(np.sqrt(dsq))
            if view_dist >= a.max_dist:
                drawn, draw_alpha = 0, f32(0.0)
                tally["too_distant"] += 1
            else:
                val = f32(1.0 - float(f32(f32(a.max_dist - view_dist) / a.max_dist)))
                drawn, draw_alpha = 1, f32(alpha * f32(f32(1.0) - f32(val * val)))
                tally["drawn"] += 1
            found.append((f32(-dsq), t, k, alpha, draw_alpha, drawn))
    keys = [e[0] for e in found]
    tally["ties"] += len(keys) - len(set(float(x) for x in keys))
    found.sort(key=lambda e: (float(e[0]), e[1], e[2]))
    lst = np.zeros(len(found), INST_DTYPE)
    for i, e in enumerate(found):
        lst[i] = (e[1], e[2], e[0], e[3], e[4], e[5])
    return stage, lst
