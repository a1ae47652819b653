"""NumPy / Python restatement of the tree AO shadows of a tile batch, written from the reference statements (not from the library's segment formulation):

    tile_t::push_tree_ao_shadow                src/tiled_mesh.cpp:740-746
    tile_t::add_tree_ao_shadow                 src/tiled_mesh.cpp:749-783 (the texel loop is tree_map_model's)
    tile_t::apply_ao_shadows_for_tree_group    src/tiled_mesh.cpp:785-796
    tile_t::apply_ao_shadows_for_trees         src/tiled_mesh.cpp:798-817
    tile_t::apply_tree_ao_shadows              src/tiled_mesh.cpp:820-828
    tile_t::get_adj_tile_smap, get_mesh_bcube  src/tiled_mesh.h:295-298, :238-241
    tile_offset_t::subtract_from               src/animals.h:26
    small_tree's two constructors, stt[]       src/sm_tree.cpp:705-753, :46-53
    small_tree::get_pine_tree_radius           src/sm_tree.cpp:911-914
    small_tree::get_radius / get_ao_radius     src/small_tree.h:74-75
    tree::get_ao_radius                        src/tree_3dw.h:313
    calc_tree_size                             src/sm_tree.cpp:326

The tiles are objects with a tree_map that is empty until apply_tree_ao_shadows has run on them; they are processed one after another in batch order, and pushes and
pulls really happen between them, as in the reference.  Types as in tree_map_model: np.float32 for float, Python float for double, Python int for int.
A record the reference could not have made (see include/terra.h) is dropped before anything else looks at it.
"""
import numpy as np

import tree_map_model as tmm

f32 = np.float32
T_PINE, T_DECID, T_TDECID, T_BUSH, T_PALM, T_SH_PINE = range(6)  # src/small_tree.h:9
NUM_ST_TYPES = 6
WIDTH_SCALE = [f32(v) for v in (1.0, 1.0, 1.0, 1.0, 1.4, 1.2)]   # stt[].width_scale: a float member initialised from the double literal
HEIGHT_SCALE = [f32(v) for v in (1.2, 1.0, 1.0, 1.0, 2.0, 0.8)]  # stt[].height_scale
SM_TREE_SIZE = f32(0.05)  # src/sm_tree.cpp:12
NO_PINE, NO_DECID, DISTANT = 1, 2, 4  # the flag byte: !can_have_pine_palm_trees(), !can_have_decid_trees(), is_distant
INST_DTYPE = np.dtype([("type", np.int32), ("height", np.float32), ("width", np.float32)])


class SizeParams:
    """the globals the radii read: config keys tree_height_scale, sm_tree_scale, pine_tree_radius_scale, tree_scale (all float, default 1)"""

    def __init__(self, tree_height_scale=1.0, sm_tree_scale=1.0, pine_tree_radius_scale=1.0, tree_scale=1.0):
        self.tree_height_scale, self.sm_tree_scale = f32(tree_height_scale), f32(sm_tree_scale)
        self.pine_tree_radius_scale, self.tree_scale = f32(pine_tree_radius_scale), f32(tree_scale)


def calc_tree_size(p):  # 16.0f*SM_TREE_SIZE/tree_scale
    return f32(f32(f32(16.0) * SM_TREE_SIZE) / p.tree_scale)


def is_pine(t):
    return t in (T_PINE, T_SH_PINE)


def small_tree_size(p, h, w, t):
    """the constructor of :717-753 as far as it touches the size -> (height, width)"""
    h, w = f32(h), f32(w)
    h = f32(h * f32(p.tree_height_scale * p.sm_tree_scale))  # height *= tree_height_scale*sm_tree_scale
    w = f32(w * WIDTH_SCALE[t])                              # width  *= stt[type].width_scale
    h = f32(h * HEIGHT_SCALE[t])                             # height *= stt[type].height_scale
    return h, w


def instanced_size(p, inst):
    """small_tree(p, instance_id) (:705-715): the instance, its width and height times calc_tree_size() -> (type, height, width)"""
    tsize = calc_tree_size(p)
    return int(inst["type"]), f32(f32(inst["height"]) * tsize), f32(f32(inst["width"]) * tsize)


def get_pine_tree_radius(p, t, height):
    hs = f32(p.tree_height_scale * p.sm_tree_scale)
    with np.errstate(all="ignore"):
        height0 = f32(((0.75 if t == T_PINE else 1.0) * float(height)) / float(hs))      # float const height0(((type == T_PINE) ? 0.75 : 1.0)*height/(...))
        return f32((0.35 * float(p.pine_tree_radius_scale)) * (float(height0) + 0.03 / float(p.tree_scale)))


def get_radius(p, t, height, width):  # branch_xy_scale = 1.0, the constructor's default
    return f32(f32(1.0) * get_pine_tree_radius(p, t, height)) if is_pine(t) else f32(width)


def small_tree_ao_radius(t, radius):  # (is_pine_tree() ? 1.8 : ((type == T_PALM) ? 0.4 : 0.5))*get_radius()
    with np.errstate(all="ignore"):
        return f32((1.8 if is_pine(t) else (0.4 if t == T_PALM else 0.5)) * float(radius))


def decid_ao_radius(radius):  # 0.5*get_radius()
    with np.errstate(all="ignore"):
        return f32(0.5 * float(f32(radius)))


def radius_ok(r):
    return bool(np.isfinite(r)) and r >= 0


def new_tally():
    return dict(own=0, pulled=0, pushed=0, culled_own=0, culled_pull=0, no_adj_true=0, no_adj_false=0, instanced=0, by_id=0, per_record=0, dropped=0,
                overflow=0, types=set(), inst_types=set())


class Tile:
    def __init__(self, ix, tx, ty, flags):
        self.ix, self.tx, self.ty, self.flags = ix, tx, ty, int(flags)
        self.pine, self.decid = [], []  # (pos.x, pos.y, get_radius(), get_ao_radius()) of every tree, in record order
        self.tree_map = None            # tree_map.empty()
        self.updated = False
        self.nsplat = 0                 # add_tree_ao_shadow calls so far
        self.trmax = f32(0.0)

    is_distant = property(lambda self: bool(self.flags & DISTANT))
    can_have_pine_palm_trees = property(lambda self: not self.flags & NO_PINE)
    can_have_decid_trees = property(lambda self: not self.flags & NO_DECID)


class Batch:
    """the tiles of one call and everything apply_tree_ao_shadows reads; run() processes them in batch order"""

    def __init__(self, sc, p, tiles, list_capacity, pine=None, pine_counts=None, decid=None, decid_counts=None, decid_radius=None, decid_radius_by_id=None, flags=None,
                 instanced=False, insts=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, tally=None):
        self.sc, self.p, self.cap, self.dxoff, self.dyoff = sc, p, list_capacity, dxoff, dyoff
        self.tally = new_tally() if tally is None else tally
        self.tiles = [Tile(i, int(tx), int(ty), 0 if flags is None else flags[i]) for i, (tx, ty) in enumerate(tiles)]
        self.by_xy = {(t.tx, t.ty): t for t in self.tiles}
        assert len(self.by_xy) == len(self.tiles)
        # pt_off = toff.subtract_from(mesh_off) with toff.dxoff = -xoff2: an int sum times a float
        self.pt_off = (f32(f32(wrap32(dxoff + xoff2)) * sc.DX_VAL), f32(f32(wrap32(dyoff + yoff2)) * sc.DY_VAL))
        for t in self.tiles:
            if pine is not None and pine_counts is not None:
                for r in pine[t.ix][:min(int(pine_counts[t.ix]), pine.shape[1])]:
                    self._add_small_tree(t, r, instanced, insts)
            if decid is not None and decid_counts is not None:
                for k, r in enumerate(decid[t.ix][:min(int(decid_counts[t.ix]), decid.shape[1])]):
                    self._add_decid_tree(t, r, None if decid_radius is None else decid_radius[t.ix][k], decid_radius_by_id)
            t.trmax = f32(max([f32(0.0)] + [tr[2] for tr in t.pine + t.decid]))  # postproc_trees / add_tree / get_rmax

    def _add_small_tree(self, t, r, instanced, insts):
        ta = self.tally
        if int(r["inst"]) >= 0:
            if not instanced or insts is None or int(r["inst"]) >= len(insts):
                ta["dropped"] += 1
                return
            typ, h, w = instanced_size(self.p, insts[int(r["inst"])])
            if not 0 <= typ < NUM_ST_TYPES:
                ta["dropped"] += 1
                return
            ta["instanced"] += 1
            ta["inst_types"].add(typ)
        else:
            typ = int(r["type"])
            if not 0 <= typ < NUM_ST_TYPES:
                ta["dropped"] += 1
                return
            h, w = small_tree_size(self.p, r["height"], r["width"], typ)
        rad = get_radius(self.p, typ, h, w)
        ao = small_tree_ao_radius(typ, rad)
        if not (radius_ok(rad) and radius_ok(ao)):
            ta["dropped"] += 1
            return
        ta["types"].add(typ)
        t.pine.append((f32(r["pos"][0]), f32(r["pos"][1]), rad, ao))

    def _add_decid_tree(self, t, r, rec_radius, by_id):
        ta = self.tally
        if rec_radius is not None:
            rad = f32(rec_radius)
            kind = "per_record"
        elif by_id is not None and 0 <= int(r["tree_id"]) < len(by_id):
            rad = f32(by_id[int(r["tree_id"])])
            kind = "by_id"
        else:
            ta["dropped"] += 1
            return
        ao = decid_ao_radius(rad)
        if not (radius_ok(rad) and radius_ok(ao)):
            ta["dropped"] += 1
            return
        ta[kind] += 1
        t.decid.append((f32(r["pos"][0]), f32(r["pos"][1]), rad, ao))

    # ---- the reference's functions, `this` = tile
    def get_adj_tile_smap(self, tile, dx, dy):
        adj = self.by_xy.get((tile.tx + dx, tile.ty + dy))
        return adj if adj is not None and adj.tree_map is not None else None

    def push_tree_ao_shadow(self, tile, dx, dy, pos, tradius):
        adj = self.get_adj_tile_smap(tile, dx, dy)
        if adj is None or adj.is_distant:
            return
        self.tally["pushed"] += 1
        self.add_tree_ao_shadow(adj, pos, tradius, True)  # pos2 = pos: both tiles have the batch's mesh_off

    def add_tree_ao_shadow(self, tile, pos, tradius, no_adj_test):
        sc, S = self.sc, self.sc.S
        k = tile.nsplat
        tile.nsplat += 1
        par = tmm.splat_params(sc, tile.tx, tile.ty, self.dxoff, self.dyoff, pos[0], pos[1], tradius)
        if par is None:  # undefined in the reference: the library skips the splat, and it pushes nothing
            return
        if k < self.cap:
            tile.updated |= tmm.add_tree_ao_shadow(sc, tile.tree_map, par)
        else:
            self.tally["overflow"] += 1
        if not no_adj_test:
            xc, yc, rval, _ = par
            x_test = [xc <= rval, True, xc >= S - rval]
            y_test = [yc <= rval, True, yc >= S - rval]
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    if x_test[dx + 1] and y_test[dy + 1]:
                        self.push_tree_ao_shadow(tile, dx, dy, pos, tradius)

    def apply_ao_shadows_for_tree_group(self, this, trees, no_adj_test, own):
        sc = self.sc
        x1, y1 = sc.get_xval(this.tx * sc.S + self.dxoff), sc.get_yval(this.ty * sc.S + self.dyoff)   # get_mesh_bcube()
        x2, y2 = f32(x1 + f32(f32(sc.S) * sc.DX_VAL)), f32(y1 + f32(f32(sc.S) * sc.DY_VAL))
        for (px, py, _, tr) in trees:
            pt = (f32(px + self.pt_off[0]), f32(py + self.pt_off[1]))
            if no_adj_test and (f32(pt[0] + tr) < x1 or f32(pt[0] - tr) > x2 or f32(pt[1] + tr) < y1 or f32(pt[1] - tr) > y2):
                self.tally["culled_own" if own else "culled_pull"] += 1
                continue
            self.tally["own" if own else "pulled"] += 1
            self.add_tree_ao_shadow(this, pt, tr, no_adj_test)

    def apply_ao_shadows_for_trees(self, this, tile, no_adj_test):
        own = tile is this
        if this.can_have_pine_palm_trees:
            self.apply_ao_shadows_for_tree_group(this, tile.pine, no_adj_test, own)
        if this.can_have_decid_trees:
            self.apply_ao_shadows_for_tree_group(this, tile.decid, no_adj_test, own)
        if not no_adj_test and not this.is_distant:  # pull mode
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    adj = self.get_adj_tile_smap(this, dx, dy)
                    if adj is not None and not adj.is_distant:
                        self.apply_ao_shadows_for_trees(this, adj, True)

    def apply_tree_ao_shadows(self, this):
        if this.is_distant:
            return
        W = self.sc.S + 1
        this.tree_map = np.full((W, W, 2), 255, np.uint8)  # tree_map.clear(); tree_map.resize(stride*stride)
        no_adj_test = bool(this.trmax < min(self.sc.DX_VAL, self.sc.DY_VAL))
        self.tally["no_adj_true" if no_adj_test else "no_adj_false"] += 1
        self.apply_ao_shadows_for_trees(this, this, no_adj_test)

    def run(self):
        """-> (tree_map u8 [n, S+1, S+1, 2], updated bool [n], trmax float32 [n], list_counts uint32 [n])"""
        for t in self.tiles:
            self.apply_tree_ao_shadows(t)
        n, W = len(self.tiles), self.sc.S + 1
        maps = np.full((n, W, W, 2), 255, np.uint8)  # an all-255 map reads as the reference's empty one
        for t in self.tiles:
            if t.tree_map is not None:
                maps[t.ix] = t.tree_map
        return (maps, np.array([t.updated for t in self.tiles], bool), np.array([t.trmax for t in self.tiles], np.float32),
                np.array([t.nsplat for t in self.tiles], np.uint32))


def wrap32(v):
    """an int sum that wraps"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v
