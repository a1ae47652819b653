"""NumPy / Python restatement of the flowers of a tile, written from the reference statements (not from the library's kernels):

    flower_tile_manager_t::gen_flowers, update_subrange, clear_within        src/grass.cpp:859-926
    flower_manager_t::add_flowers, gen_density_cache, skip_generate          src/grass.cpp:752-754, 813-845
    flower_t                                                                 src/grass.h:80-88
    get_median_height(0.5)                                                   src/mesh_gen.cpp:487-491
    rand_float, signed_rand_float, rand_uniform                              src/rand_gen.h:86-90
    signed_rand_vector                                                       src/gen_object.cpp:400-403
    pointT::get_norm, mag                                                    src/3DWorld.h:297-300, 324-325
    remove_element                                                           src/inlines.h:743-747
    p2p_dist_xy_sq, dist_xy_less_than                                        src/inlines.h:183-195
    the callers: tile_t::draw_flowers, tile_t::add_or_remove_grass_at        src/tiled_mesh.cpp:1666-1677, 3930-3937

It is built on oracle primitives only: orc.gen_grid(.., glaciate=0, min_start_sin=50, force_sine=True) for the two density fields and orc.state(); the
generator, f32 and the way the height histogram is read are tree_place_model's.

Types as in tree_place_model: np.float32 for float, Python float for double, Python int for int / unsigned.  Which sub-expressions are double:
  weight/255.0 (narrowed to the float parameter grass_den), grass_den < 0.5, flower_density*grass_den + 0.5 (a float product plus a double),
  dval + 0.2*zmax_est*signed_rand_float() > hthresh (all double), 0.000001*(rand()%1000000) (narrowed by rand_float's return),
  dx + DX_VAL*(xpos + rand_float() - 0.5): xpos + rand_float() is a float sum, the - 0.5 and everything outside it double, narrowed by point's constructor,
  cval + 0.25*signed_rand_float() (narrowed to color_val), 0.5*NUM_COLORS*color_val (1.5*double(color_val)).
float: grass_length*rand_uniform(..), scale*signed_rand_float(), plus_z + v, mag() = sqrt(x*x + y*y + z*z) (the float overload), x/vmag, grass_width*rand_uniform(..).

Order of draws.  `point pos(a, b, height)` and `vector3d(scale*srf(), scale*srf(), scale*srf())` are function-style calls: g++ evaluates their arguments right to
left (as scenery_place_model documents for signed_rand_vector).  So of the position's two rand_float() the first is y's, and of the normal's three
signed_rand_float() the first is z's.  `height` is a named variable drawn before.  The order is pinned here and in test_flowers_emul.py::test_model_draw_order.

The colour index.  `colors[int(0.5*NUM_COLORS*color_val)%NUM_COLORS]` with `unsigned const NUM_COLORS(3)`: the usual arithmetic conversions turn the int into an
unsigned before the remainder, so the index is (int(..) mod 2^32) % 3 -- 0 .. 2 for every color_val, defined behaviour, and NOT the signed remainder plus 3 for a
negative int (-1 -> 4294967295 % 3 = 0).  `ix` below is the signed C remainder (-2 .. 2); the library reports ix + 2 in its aux word so that the flowers whose
colour hangs on that conversion can be told apart; the tally counts them."""
import numpy as np

import tree_place_model as tpm
from tree_place_model import RandGen, cmod, f32

FLOWER_DTYPE = np.dtype([("pos", np.float32, (3,)), ("normal", np.float32, (3,)), ("radius", np.float32), ("height", np.float32), ("color", np.float32, (4,))])
NUM_COLORS, START_EVAL_SINE = 3, 50
COLORS = [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 0.0, 1.0], [0.58, 0.58, 1.0, 1.0]]  # WHITE, YELLOW, LT_BLUE (src/3DWorld.h:1264-1281)
AUX_FIXED = 7
FLOWER_DIST_THRESH = 0.5
TOLERANCE = f32(1.0E-12)
TALLY = ("weight0_cells", "low_density_cells", "bin1_cells", "bin2_cells", "bin_more_cells", "rejected", "accepted", "negative_ix", "nonnegative_ix", "beyond_capacity",
         "removed", "refilled")


def new_tally():
    return {k: 0 for k in TALLY}


class Params:
    """flower_density, grass_length, grass_width (src/grass.cpp:15), flower_color (src/3DWorld.cpp:124: ALPHA0), no_grass()"""

    def __init__(self, flower_density=0.0, grass_length=0.02, grass_width=0.002, flower_color=(0.0, 0.0, 0.0, 0.0), no_grass=0):
        self.flower_density, self.grass_length, self.grass_width = f32(flower_density), f32(grass_length), f32(grass_width)
        self.flower_color, self.no_grass = [f32(v) for v in flower_color], bool(no_grass)


class Scene:
    """the globals the flowers read: the oracle's state after orc.init(cfg), the config, the settings, the height histogram (hist=() is the empty one)"""

    def __init__(self, orc, cfg, params, hist=None):
        st = orc.state()
        self.orc, self.p = orc, params
        self.S = int(cfg.mesh_x)
        self.X_SCENE_SIZE, self.Y_SCENE_SIZE = f32(cfg.scene_x), f32(cfg.scene_y)
        self.DX_VAL, self.DY_VAL, self.DX_VAL_INV, self.DY_VAL_INV = f32(st.DX_VAL), f32(st.DY_VAL), f32(st.DX_VAL_INV), f32(st.DY_VAL_INV)
        self.zmax_est = f32(st.zmax_est)
        self.hist = tpm.height_histogram(orc, st) if hist is None else np.asarray(hist, f32)
        self._fields = {}

    def skip_generate(self):
        return self.p.no_grass or self.p.flower_density == 0.0

    def get_median_height(self, pos):  # as tree_place_model.Scene reads it
        n = len(self.hist)
        if n == 0:
            return f32(pos)
        return self.hist[max(0, min(n - 1, int(f32(f32(n) * f32(pos)))))]

    def density_fields(self, tx, ty):
        """gen_density_cache: build_arrays(tile x1, tile y1, fds*DX_VAL*DX_VAL, fds*DY_VAL*DY_VAL, S, S, 0, 1), read with eval_index(x, y, 50) -> two [S, S] arrays"""
        if (tx, ty) not in self._fields:
            S, out = self.S, []
            for i in range(2):
                fds = f32(500.0 * (1.0 + 0.3 * i))
                dx, dy = f32(f32(fds * self.DX_VAL) * self.DX_VAL), f32(f32(fds * self.DY_VAL) * self.DY_VAL)
                out.append(self.orc.gen_grid(float(tx * S), float(ty * S), float(dx), float(dy), S, S, glaciate=0, min_start_sin=START_EVAL_SINE, force_sine=True))
            self._fields[(tx, ty)] = out
        return self._fields[(tx, ty)]


def num_per_bin(sc, weight, tally=None):
    grass_den = f32(int(weight) / 255.0)
    if float(grass_den) < 0.5:
        if tally is not None:
            tally["weight0_cells" if int(weight) == 0 else "low_density_cells"] += 1
        return 0
    n = int(float(f32(sc.p.flower_density * grass_den)) + 0.5)
    if tally is not None and n:
        tally["bin1_cells" if n == 1 else ("bin2_cells" if n == 2 else "bin_more_cells")] += 1
    return n


def add_flowers(sc, rgen, fields, weight, hthresh, xpos, ypos, out, tally):
    """flower_manager_t::add_flowers(density_gen, weight/255.0, hthresh, 0.0, 0.0, xpos, ypos, 0); out: list of (record, cx, cy, ix or None)"""
    p = sc.p
    n = num_per_bin(sc, weight, tally)
    if n == 0:
        return
    dval, cval = f32(fields[0][ypos, xpos]), f32(fields[1][ypos, xpos])
    for _ in range(n):
        if float(dval) + 0.2 * float(sc.zmax_est) * float(rgen.signed_rand_float()) > float(hthresh):
            tally["rejected"] += 1
            continue
        tally["accepted"] += 1
        height = f32(p.grass_length * rgen.rand_uniform(0.85, 1.0))
        ry = rgen.rand_float()  # the constructor's arguments right to left: y's draw first
        rx = rgen.rand_float()
        px = f32(0.0 + float(sc.DX_VAL) * (float(f32(f32(xpos) + rx)) - 0.5))
        py = f32(0.0 + float(sc.DY_VAL) * (float(f32(f32(ypos) + ry)) - 0.5))
        vz = f32(f32(0.2) * rgen.signed_rand_float())  # signed_rand_vector(0.2): z's draw first
        vy = f32(f32(0.2) * rgen.signed_rand_float())
        vx = f32(f32(0.2) * rgen.signed_rand_float())
        nx, ny, nz = f32(f32(0.0) + vx), f32(f32(0.0) + vy), f32(f32(1.0) + vz)
        vmag = f32(np.sqrt(f32(f32(f32(nx * nx) + f32(ny * ny)) + f32(nz * nz))))
        normal = [nx, ny, nz] if vmag < TOLERANCE else [f32(nx / vmag), f32(ny / vmag), f32(nz / vmag)]
        radius = f32(p.grass_width * rgen.rand_uniform(1.5, 2.5))
        if p.flower_color[3] > 0.0:
            color, ix = p.flower_color, None
        else:
            color_val = f32(float(cval) + 0.25 * float(rgen.signed_rand_float()))
            iq = int(0.5 * NUM_COLORS * float(color_val))  # truncation
            ix = cmod(iq, NUM_COLORS)                      # the signed remainder: what the aux word reports
            color = COLORS[(iq % 2 ** 32) % NUM_COLORS]    # int % unsigned: the int converts to unsigned first
            tally["negative_ix" if ix < 0 else "nonnegative_ix"] += 1
        rec = np.zeros((), FLOWER_DTYPE)
        rec["pos"], rec["normal"], rec["radius"], rec["height"], rec["color"] = [px, py, height], normal, radius, height, color
        out.append((rec, xpos, ypos, ix))


def seed(sc, tx, ty, xl=0, yl=0):
    """rgen.set_state(x1 + xl + xoff2 + 123, y1 + yl + yoff2 + 456) with the caller's x1 - xoff2: the tile's own x1 (int sums, held in long)"""
    return RandGen(tpm.wrap32(tx * sc.S + xl + 123), tpm.wrap32(ty * sc.S + yl + 456))


def gen_flowers(sc, tx, ty, weights, tally=None):
    """flower_tile_manager_t::gen_flowers(weight_data, S + 1, x1 - xoff2, y1 - yoff2, 0) -> list of (record, cx, cy, ix); weights: [S+1, S+1, 4] bytes"""
    tally = new_tally() if tally is None else tally
    out = []
    if sc.skip_generate():
        return out
    rgen = seed(sc, tx, ty)
    fields = sc.density_fields(tx, ty)
    hthresh = sc.get_median_height(FLOWER_DIST_THRESH)
    for y in range(sc.S):
        for x in range(sc.S):
            weight = int(weights[y, x, 2])
            if weight == 0:
                tally["weight0_cells"] += 1
                continue
            add_flowers(sc, rgen, fields, weight, hthresh, x, y, out, tally)
    return out


def remove_elements(flowers, removed, tally=None):
    """for (i = 0; i < size; ++i) if (removed(v[i])) remove_element(v, i): swap with the back, pop, --i"""
    i = 0
    while i < len(flowers):
        if removed(flowers[i][0]):
            flowers[i] = flowers[-1]
            flowers.pop()
            if tally is not None:
                tally["removed"] += 1
            continue  # (--i, ++i)
        i += 1


def update_subrange(sc, tx, ty, weights, flowers, xl, yl, xh, yh, tally=None):
    """flower_tile_manager_t::update_subrange on a generated tile, in place.  eval_index asserts x < S: a range with xh > S or yh > S is the caller's to refuse"""
    tally = new_tally() if tally is None else tally
    if xh <= xl or yh <= yl:
        return
    assert xh <= sc.S and yh <= sc.S

    def in_range(rec):
        fx, fy = int(f32(rec["pos"][0] * sc.DX_VAL_INV)), int(f32(rec["pos"][1] * sc.DY_VAL_INV))
        return xl <= fx < xh and yl <= fy < yh

    remove_elements(flowers, in_range, tally)
    rgen = seed(sc, tx, ty, xl, yl)
    fields = sc.density_fields(tx, ty)
    hthresh = sc.get_median_height(FLOWER_DIST_THRESH)
    before = len(flowers)
    for y in range(yl, yh):
        for x in range(xl, xh):
            add_flowers(sc, rgen, fields, int(weights[y, x, 2]), hthresh, x, y, flowers, tally)
    tally["refilled"] += len(flowers) - before


def clear_within(sc, tx, ty, flowers, pos, radius, is_square, dxoff=0, dyoff=0, tally=None):
    """flowers.clear_within(pos - flower_xlate, rradius, is_square) with flower_xlate = (get_xval(x1 + xoff - xoff2), get_yval(y1 + yoff - yoff2), 0)"""
    radius = f32(radius)
    xl8 = f32(-sc.X_SCENE_SIZE + f32(sc.DX_VAL * f32(tx * sc.S + dxoff)))
    yl8 = f32(-sc.Y_SCENE_SIZE + f32(sc.DY_VAL * f32(ty * sc.S + dyoff)))
    px, py = f32(f32(pos[0]) - xl8), f32(f32(pos[1]) - yl8)

    def in_brush(rec):
        fx, fy = f32(rec["pos"][0]), f32(rec["pos"][1])
        if abs(f32(fx - px)) > radius or abs(f32(fy - py)) > radius:
            return False
        if not is_square:
            dx, dy = f32(fx - px), f32(fy - py)
            if not f32(f32(dx * dx) + f32(dy * dy)) < f32(radius * radius):
                return False
        return True

    remove_elements(flowers, in_brush, tally)


def aux_word(cx, cy, ix):
    return cx | (cy << 10) | ((AUX_FIXED if ix is None else ix + 2) << 20)


def place(sc, tiles, weights, skip=None, tally=None):
    """the batch call: per tile the list of (record, cx, cy, ix)"""
    return [[] if (skip is not None and skip[t]) else gen_flowers(sc, tx, ty, weights[t], tally) for t, (tx, ty) in enumerate(tiles)]


def edit(sc, tiles, weights, lists, brush, updated, ranges, generated=None, dxoff=0, dyoff=0, tally=None):
    """the flowers' half of tile_t::add_or_remove_grass_at on every tile, in place on `lists` -> status per tile.  brush: (pos[3], radius, add_grass, is_square)"""
    pos, radius, add, is_square = brush
    status = []
    for t, (tx, ty) in enumerate(tiles):
        if not updated[t] or (generated is not None and not generated[t]):
            status.append(0)
            continue
        if add:
            xl, yl, xh, yh = (int(v) for v in ranges[t])
            if xh <= xl or yh <= yl:
                status.append(0)
            elif xh > sc.S or yh > sc.S:
                status.append(2)
            else:
                update_subrange(sc, tx, ty, weights[t], lists[t], xl, yl, xh, yh, tally)
                status.append(1)
        else:
            clear_within(sc, tx, ty, lists[t], pos, radius, is_square, dxoff, dyoff, tally)
            status.append(1)
    return status
