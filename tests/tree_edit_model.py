"""NumPy / Python restatement of one stroke of the tree brush on the two tree containers of a tile batch, written from the reference statements:

    tile_draw_t::add_or_remove_trees_at        src/tiled_mesh.cpp:3746-3769 (from :3756 on: the static same-position early-out stays with the caller)
    update_trees_bcube                         src/tiled_mesh.cpp:3776-3778
    remove_tree                                src/tiled_mesh.cpp:3779-3787
    remove_element                             src/inlines.h:743-747
    tile_t::mesh_sphere_intersect              src/tiled_mesh.cpp:3796-3799
    tile_t::add_new_trees                      src/tiled_mesh.cpp:3805-3819
    tile_t::add_or_remove_trees_at             src/tiled_mesh.cpp:3822-3843
    tile_t::calc_radius, get_center, get_mesh_bcube, postproc_trees   src/tiled_mesh.h:204, :229-241, :342-347
    sphere_cube_intersect (DMIN_CHECK)         src/Math3d.cpp:920-935
    cube_t::set_from_sphere, is_all_zeros, union_with_sphere, intersects   src/3DWorld.h:441-443, :491, :502-504, :536-539
    tile_offset_t::get_xlate                   src/animals.h:25

The two containers are Python lists; removal is the literal remove_element loop (swap with the back, pop, test the same index again), never a closed form, and the
box is the literal serial accumulation with its is_all_zeros() restart.  The radii come from tree_ao_model, the appended records from tree_place_model /
decid_place_model.  Types: np.float32 for float, Python float for double, Python int for int.
What the library adds to the reference (include/terra.h): arrays with a capacity (a container is the first min(count, capacity) records; an append stores what
fits, and only stored records count for the box and trmax), and records the reference could not have made, which have no radius: they are removed by position
like any other and add nothing to the box.
"""
import numpy as np

import decid_place_model as dpm
import tree_ao_model as tam
import tree_place_model as tpm

f32 = np.float32
BCUBE_ZTOLER = f32(1.0e-6)  # src/tiled_mesh.h:32
NO_PINE_GEN, NO_DECID_GEN = 1, 2  # gen_flags: !pine_trees_generated(), !decid_trees.was_generated()


def std_min(a, b):  # std::min(a, b): (b < a) ? b : a
    return b if b < a else a


def std_max(a, b):  # std::max(a, b): (a < b) ? b : a
    return b if a < b else a


class Cube:
    """cube_t: d[3][2], all zeros after its default constructor"""

    def __init__(self):
        self.d = [[f32(0.0), f32(0.0)] for _ in range(3)]

    def is_all_zeros(self):
        return all(v == 0 for ax in self.d for v in ax)

    def set_from_sphere(self, pt, radius):
        for i in range(3):
            self.d[i][0], self.d[i][1] = f32(pt[i] - radius), f32(pt[i] + radius)

    def union_with_sphere(self, pt, radius):  # min_eq(d[i][0], pt[i]-radius); max_eq(d[i][1], pt[i]+radius)
        for i in range(3):
            self.d[i][0], self.d[i][1] = std_min(self.d[i][0], f32(pt[i] - radius)), std_max(self.d[i][1], f32(pt[i] + radius))

    def intersects(self, lo, hi):  # this.intersects(cube) with cube = (lo, hi): includes adjacency
        return not any(hi[i] < self.d[i][0] or lo[i] > self.d[i][1] for i in range(3))

    def values(self):
        return np.array([v for ax in self.d for v in ax], np.float32)  # x1 x2 y1 y2 z1 z2


def update_trees_bcube(tpos, tradius, bcube):
    if bcube.is_all_zeros():
        bcube.set_from_sphere(tpos, tradius)
    else:
        bcube.union_with_sphere(tpos, tradius)


def remove_element(v, i):  # swap(v[i], v.back()); v.pop_back(); --i
    v[i], v[-1] = v[-1], v[i]
    v.pop()
    return i - 1


def remove_loop(v, is_removed, on_remove=lambda e: None):
    """for (unsigned i = 0; i < v.size(); ++i) {remove_tree(v, i, ..);} -> whether anything was removed"""
    changed, i = False, 0
    while i < len(v):
        if is_removed(v[i]):
            on_remove(v[i])
            i = remove_element(v, i)
            changed = True
        i += 1
    return changed


def closed_form(keep):
    """the order remove_loop leaves, as the kernel forms it: keep[i] -> the list of source indices.  With M survivors, a survivor below M stays; the holes below M,
    ascending, receive the survivors at M and above, descending"""
    m = sum(keep)
    out = [i if keep[i] else None for i in range(m)]
    tail = [i for i in range(len(keep) - 1, m - 1, -1) if keep[i]]
    holes = [i for i in range(m) if not keep[i]]
    assert len(tail) == len(holes)
    for h, s in zip(holes, tail):
        out[h] = s
    return out


class Tree:
    """one element of a container: the record, its get_radius() (None: a record without a tree) and the caller's per-record radius that travels with it"""

    def __init__(self, rec, radius, rec_radius=None):
        self.rec, self.radius, self.rec_radius = rec, radius, rec_radius

    def get_center(self):
        return (f32(self.rec["pos"][0]), f32(self.rec["pos"][1]), f32(self.rec["pos"][2]))


def pine_tree_radius(p, r, instanced, insts, tally=None):
    """get_radius() of a pine / palm record as tree_ao_model forms it; None when tree_ao_model drops the record"""
    if int(r["inst"]) >= 0:
        if not instanced or insts is None or int(r["inst"]) >= len(insts):
            return None
        typ, h, w = tam.instanced_size(p, insts[int(r["inst"])])
        if not 0 <= typ < tam.NUM_ST_TYPES:
            return None
        if tally is not None:
            tally["instanced"] += 1
    else:
        typ = int(r["type"])
        if not 0 <= typ < tam.NUM_ST_TYPES:
            return None
        h, w = tam.small_tree_size(p, r["height"], r["width"], typ)
    rad = tam.get_radius(p, typ, h, w)
    return rad if tam.radius_ok(rad) and tam.radius_ok(tam.small_tree_ao_radius(typ, rad)) else None


def decid_tree_radius(r, rec_radius, by_id, tally=None):
    if rec_radius is not None:
        rad, kind = f32(rec_radius), "per_record"
    elif by_id is not None and 0 <= int(r["tree_id"]) < len(by_id):
        rad, kind = f32(by_id[int(r["tree_id"])]), "by_id"
    else:
        return None
    if not (tam.radius_ok(rad) and tam.radius_ok(tam.decid_ao_radius(rad))):
        return None
    if tally is not None:
        tally[kind] += 1
    return rad


def new_tally():
    return dict(status0=0, status1=0, status2=0, near_only=0, hit_unchanged=0, removed_pine=0, removed_decid=0, removed_last=0, chain3=0, emptied=0, boundary_kept=0,
                square_only=0, over_capacity_in=0, append_overflow=0, appended_pine=0, appended_decid=0, instanced=0, per_record=0, by_id=0, dropped_removed=0,
                multi_sweep=0, gated_gen=0, gated_skip=0, removed_while_gated=0, changed_by_box=0, box_zero=0, trmax_raised=0, radius_by_stats=0, radius_by_trmax=0)


class Tile:
    def __init__(self, ix, tx, ty, stats, trmax, gen_flags, skip):
        self.ix, self.tx, self.ty, self.gen_flags, self.skip = ix, tx, ty, int(gen_flags), bool(skip)
        self.mzmin, self.mzmax, self.stats_radius = f32(stats.mzmin), f32(stats.mzmax), f32(stats.radius)
        self.trmax = f32(trmax)
        self.pine_trees, self.decid_trees = None, None  # lists of Tree, None: the group is absent
        self.pine_count = self.decid_count = 0          # counts[t]: may exceed the array


class Batch:
    def __init__(self, sc, psc, p, dp, tiles, stats, trmax, pine=None, pine_counts=None, decid=None, decid_counts=None, decid_radius=None, decid_radius_by_id=None,
                 gen_flags=None, skip=None, zvals=None, instanced=False, insts=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, tally=None):
        """sc: tree_map_model.Scene; psc: tree_place_model.Scene (the placements); p: tree_ao_model.SizeParams; dp: decid_place_model.DecidParams"""
        self.sc, self.psc, self.p, self.dp, self.dxoff, self.dyoff, self.xoff2, self.yoff2 = sc, psc, p, dp, dxoff, dyoff, xoff2, yoff2
        self.stats, self.zvals, self.instanced, self.insts, self.by_id = stats, zvals, instanced, insts, decid_radius_by_id
        self.per_record = decid_radius is not None
        self.tally = new_tally() if tally is None else tally
        self.pine_cap = 0 if pine is None else pine.shape[1]
        self.decid_cap = 0 if decid is None else decid.shape[1]
        self.tiles = []
        for i, (tx, ty) in enumerate(tiles):
            t = Tile(i, int(tx), int(ty), stats[i], trmax[i], 0 if gen_flags is None else gen_flags[i], False if skip is None else skip[i])
            if pine is not None and pine_counts is not None:
                k = min(int(pine_counts[i]), self.pine_cap)
                self.tally["over_capacity_in"] += int(pine_counts[i]) > self.pine_cap
                t.pine_count = int(pine_counts[i])
                t.pine_trees = [Tree(r.copy(), pine_tree_radius(p, r, instanced, insts, self.tally)) for r in pine[i][:k]]
            if decid is not None and decid_counts is not None:
                k = min(int(decid_counts[i]), self.decid_cap)
                self.tally["over_capacity_in"] += int(decid_counts[i]) > self.decid_cap
                t.decid_count = int(decid_counts[i])
                t.decid_trees = [Tree(r.copy(), decid_tree_radius(r, decid_radius[i][j] if self.per_record else None, decid_radius_by_id, self.tally),
                                      f32(decid_radius[i][j]) if self.per_record else None) for j, r in enumerate(decid[i][:k])]
            self.tiles.append(t)
        # get_xlate(): (get_delta_xoff()*DX_VAL, get_delta_yoff()*DY_VAL, 0.0) with get_delta_xoff() = (xoff - xoff2) - toff.dxoff = dxoff + xoff2 of the placement
        self.xlate = (f32(f32(tam.wrap32(dxoff + xoff2)) * sc.DX_VAL), f32(f32(tam.wrap32(dyoff + yoff2)) * sc.DY_VAL), f32(0.0))

    # ---- src/tiled_mesh.h
    def calc_radius(self):  # 0.5*sqrt(DX_VAL*DX_VAL + DY_VAL*DY_VAL)*size
        sc = self.sc
        return f32(0.5 * float(np.sqrt(f32(f32(sc.DX_VAL * sc.DX_VAL) + f32(sc.DY_VAL * sc.DY_VAL)))) * sc.S)

    def tile_radius(self, t):  # what postproc_trees leaves: radius = max(radius, calc_radius() + trmax), and trmax only grows
        a, b = t.stats_radius, f32(self.calc_radius() + t.trmax)
        self.tally["radius_by_trmax" if a < b else "radius_by_stats"] += 1
        return std_max(a, b)

    def get_center(self, t):
        sc, S = self.sc, self.sc.S
        x1, y1 = t.tx * S, t.ty * S
        return (sc.get_xval(((x1 + x1 + S) >> 1) + self.dxoff), sc.get_yval(((y1 + y1 + S) >> 1) + self.dyoff), f32(f32(0.5) * f32(t.mzmin + t.mzmax)))

    def get_mesh_bcube(self, t):
        sc, S = self.sc, self.sc.S
        xv1, yv1 = sc.get_xval(t.tx * S + self.dxoff), sc.get_yval(t.ty * S + self.dyoff)
        return ([xv1, yv1, f32(t.mzmin - BCUBE_ZTOLER)], [f32(xv1 + f32(f32(S) * sc.DX_VAL)), f32(yv1 + f32(f32(S) * sc.DY_VAL)), f32(t.mzmax + BCUBE_ZTOLER)])

    def mesh_sphere_intersect(self, t, pos, rradius):
        rradius = f32(rradius)
        center = self.get_center(t)
        d = [f32(pos[i] - center[i]) for i in range(3)]
        dist_sq = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
        dval = f32(self.tile_radius(t) + rradius)
        if not dist_sq < f32(dval * dval):  # dist_less_than
            return False
        lo, hi = self.get_mesh_bcube(t)
        dmin, r2 = f32(0.0), f32(rradius * rradius)
        for i in range(3):  # DMIN_CHECK
            if pos[i] < lo[i]:
                dd = f32(pos[i] - lo[i]); dmin = f32(dmin + f32(dd * dd))
            elif pos[i] > hi[i]:
                dd = f32(pos[i] - hi[i]); dmin = f32(dmin + f32(dd * dd))
            if dmin > r2:
                return False
        return True

    # ---- src/tiled_mesh.cpp
    def is_removed(self, tree, pos, rradius, is_square):  # remove_tree's two tests
        tpos = tree.get_center()
        ex, ey = f32(tpos[0] - pos[0]), f32(tpos[1] - pos[1])
        if abs(ex) > rradius or abs(ey) > rradius:
            return False
        in_circle = bool(f32(f32(ex * ex) + f32(ey * ey)) < f32(rradius * rradius))  # dist_xy_less_than
        if not is_square and not in_circle:
            self.tally["boundary_kept"] += int(abs(ex) == rradius or abs(ey) == rradius)  # exactly on the edge of the fabs test: passes it, fails the circle
            return False
        self.tally["square_only"] += int(is_square and not in_circle)
        return True

    def tree_sphere(self, tree, update_bcube):
        if tree.radius is None:
            self.tally["dropped_removed"] += 1
            return
        tpos = tree.get_center()
        update_trees_bcube([f32(tpos[i] + self.xlate[i]) for i in range(3)], f32(2.0 * float(tree.radius)), update_bcube)

    def remove_group(self, v, pos, rradius, is_square, update_bcube, key):
        n0, last = len(v), [False]
        orig, gone = {id(e): k for k, e in enumerate(v)}, set()  # the removed records by their place on input

        def on_remove(e):
            last[0] = v[-1] is e
            gone.add(orig[id(e)])
            self.tree_sphere(e, update_bcube)

        # chains: consecutive removals at one index are a pulled-in back element that is itself removed
        run, prev_i, best = 0, None, 0
        changed, i = False, 0
        while i < len(v):  # for (unsigned i = 0; i < v.size(); ++i) {changed |= remove_tree(v, i, ..);}
            if self.is_removed(v[i], pos, rradius, is_square):
                on_remove(v[i])
                run = run + 1 if prev_i == i else 1
                best, prev_i = max(best, run), i
                i = remove_element(v, i)
                changed = True
            i += 1
        self.tally[key] += n0 - len(v)
        self.tally["removed_last"] += int(last[0])
        self.tally["chain3"] += int(best >= 3)
        self.tally["emptied"] += int(n0 > 0 and not v)
        # a group that takes the kernel through several sweeps of 256 records: more than 512 records, M beyond the first sweep and off its boundary, holes below M
        # in both of their sweeps, and survivors and removed records at M and above on both sides of 512, more than 256 places from M to the end
        m = len(v)
        both = lambda pred, lo, mid, hi: any(pred(k) for k in range(lo, mid)) and any(pred(k) for k in range(mid, hi))  # noqa: E731
        self.tally["multi_sweep"] += int(n0 > 512 and 256 < m < 512 and n0 - m > 256 and both(lambda k: k in gone, 0, 256, m) and both(lambda k: k in gone, m, 512, n0) and
                                         both(lambda k: k not in gone, m, 512, n0))
        return changed

    def add_new_trees(self, t, pine, tpos, rradius, is_square, update_bcube):
        v, cap = (t.pine_trees, self.pine_cap) if pine else (t.decid_trees, self.decid_cap)
        start_sz = len(v)
        brush = ((tpos[0], tpos[1], f32(0.0)), rradius, is_square)
        if pine:
            zr = [(t.mzmin, t.mzmax)]
            new = tpm.place(self.psc, [(t.tx, t.ty)], self.xoff2, self.yoff2, [t.skip], zr, brush)[0]
            new = [Tree(r, pine_tree_radius(self.p, r, self.instanced, self.insts)) for r in (np.array(new, tpm.PLACE_DTYPE) if new else [])]
        else:
            new = dpm.place(self.psc, self.dp, [(t.tx, t.ty)], self.xoff2, self.yoff2, [t.skip], [self.stats[t.ix]], self.zvals[t.ix:t.ix + 1], brush)[0]
            new = [Tree(r, decid_tree_radius(r, None, self.by_id), None) for r in (np.array(new, dpm.PLACE_DTYPE) if new else [])]
            for e in new:  # the per-record radius of a new record is the table's
                e.rec_radius = f32(-1.0) if e.radius is None else e.radius
        stored = new[:max(0, cap - start_sz)]
        self.tally["append_overflow"] += int(len(stored) < len(new))
        self.tally["appended_pine" if pine else "appended_decid"] += len(stored)
        v.extend(stored)
        if pine:  # counts[t] = M + all new records
            t.pine_count = start_sz + len(new)
        else:
            t.decid_count = start_sz + len(new)
        # postproc_trees: trmax = max(trmax, trees.get_rmax()) -- exact while trmax is at least the radius of every record present
        old = t.trmax
        for e in stored:
            if e.radius is not None:
                t.trmax = std_max(t.trmax, e.radius)
        self.tally["trmax_raised"] += int(t.trmax > old)
        for e in stored:  # for (i = start_sz; i < trees.size(); ++i) update_trees_bcube(trees[i].get_center()+xlate, 2.0*trees[i].get_radius(), update_bcube)
            if e.radius is not None:
                tp_ = e.get_center()
                update_trees_bcube([f32(tp_[i] + self.xlate[i]) for i in range(3)], f32(2.0 * float(e.radius)), update_bcube)
        return len(new) > 0  # trees.size() > start_sz

    def add_or_remove_trees_at(self, t, pos, rradius, add_trees, is_square, update_bcube):
        rradius = f32(rradius)
        if not self.mesh_sphere_intersect(t, pos, f32(1.1 * float(rradius) + 2.0 * float(t.trmax))):
            return 0
        if not self.mesh_sphere_intersect(t, pos, rradius):
            self.tally["near_only"] += 1
            return 1
        pt_pos = tuple(f32(pos[i] - self.xlate[i]) for i in range(3))
        pine_changed = decid_changed = False
        if t.pine_trees is not None:
            pine_changed |= self.remove_group(t.pine_trees, pt_pos, rradius, is_square, update_bcube, "removed_pine")
        if t.decid_trees is not None:
            decid_changed |= self.remove_group(t.decid_trees, pt_pos, rradius, is_square, update_bcube, "removed_decid")
        t.pine_count, t.decid_count = len(t.pine_trees or []), len(t.decid_trees or [])  # counts[t] = M
        if add_trees:
            for pine, v, bit in ((True, t.pine_trees, NO_PINE_GEN), (False, t.decid_trees, NO_DECID_GEN)):
                if v is None:
                    continue
                if t.gen_flags & bit or t.skip:
                    self.tally["gated_gen" if t.gen_flags & bit else "gated_skip"] += 1
                    self.tally["removed_while_gated"] += int(pine_changed if pine else decid_changed)
                if t.gen_flags & bit:
                    continue
                ch = self.add_new_trees(t, pine, pt_pos, rradius, is_square, update_bcube)  # (can_have_*_trees(): skip and the zrange test, inside the placement)
                if pine:
                    pine_changed |= ch
                else:
                    decid_changed |= ch
        t.hit = True
        if not pine_changed and not decid_changed:
            self.tally["hit_unchanged"] += 1
            return 1
        return 2

    def run(self, pos, rradius, add_trees, is_square):
        """tile_draw_t::add_or_remove_trees_at from :3756 on -> dict(pine, pine_counts, decid, decid_counts, decid_radius, trmax, status, changed, box); the record
        arrays hold the containers' elements, zero beyond them"""
        pos = tuple(f32(v) for v in pos)
        update_bcube = Cube()
        n = len(self.tiles)
        status = np.zeros(n, np.uint8)
        for t in self.tiles:
            t.hit = False
            status[t.ix] = self.add_or_remove_trees_at(t, pos, rradius, add_trees, is_square, update_bcube)
            self.tally["status%d" % status[t.ix]] += 1
        changed = status == 2  # register_tree_change at :3841
        if update_bcube.is_all_zeros():
            self.tally["box_zero"] += 1
        else:
            for t in self.tiles:
                if status[t.ix] >= 1:  # near_tiles
                    lo, hi = self.get_mesh_bcube(t)
                    if Cube.intersects(_as_cube(lo, hi), *_lo_hi(update_bcube)):  # get_mesh_bcube().intersects(update_bcube)
                        self.tally["changed_by_box"] += int(not changed[t.ix])
                        changed[t.ix] = True
        out = dict(status=status, changed=changed, box=update_bcube.values(), trmax=np.array([t.trmax for t in self.tiles], np.float32), hit=[t.hit for t in self.tiles])
        for key, cap, dt in (("pine", self.pine_cap, tpm.PLACE_DTYPE), ("decid", self.decid_cap, dpm.PLACE_DTYPE)):
            arr, cnt, rad = np.zeros((n, cap), dt), np.zeros(n, np.uint32), np.zeros((n, cap), np.float32)
            for t in self.tiles:
                v = t.pine_trees if key == "pine" else t.decid_trees
                if v is None:
                    continue
                for k, e in enumerate(v):
                    arr[t.ix, k] = e.rec
                    if e.rec_radius is not None:
                        rad[t.ix, k] = e.rec_radius
                cnt[t.ix] = t.pine_count if key == "pine" else t.decid_count
            out[key], out[key + "_counts"] = arr, cnt
            if key == "decid":
                out["decid_radius"] = rad
        return out


def _as_cube(lo, hi):
    c = Cube()
    for i in range(3):
        c.d[i][0], c.d[i][1] = lo[i], hi[i]
    return c


def _lo_hi(cube):
    return [cube.d[i][0] for i in range(3)], [cube.d[i][1] for i in range(3)]
