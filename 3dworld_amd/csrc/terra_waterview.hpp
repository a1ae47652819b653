// terra_waterview.hpp -- what tile_draw_t::draw(1) and the water calls decide about the tiles of a batch: tile_draw_t::can_have_reflection and
// can_have_reflection_recur (src/tiled_mesh.cpp:2630-2683) behind the filter of :2869, tile_t::is_water_visible (:2131-2133) and the edge tests of
// tile_t::draw_water_cap (:2093-2128) as tile_t::draw (:2046, :2078) and tile_draw_t::draw (:2957-2959) call it, with has_water / all_water / get_zmax
// (src/tiled_mesh.h:206-210), get_water_bcube (:253-256), rel_dist_to_camera_xy_lt (:323-325), cube_t::closest_pt / clamp_pt (src/3DWorld.h:591,636-640),
// get_cube_center (:602-604) and p2p_dist_xy (src/inlines.h:183-188).
//
// The bodies are shared by the driver's simple form (the reference's loop, sequential over the batch) and by the k_reflect_* / k_water_view kernels
// (terra_kernels.hpp).  The geometry, is_visible and the line clip are terra_terrainview.hpp's, cube_visible terra_view.hpp's.  Every operand carries the
// type the reference statement gives it (all of them are float here); sums run in the reference's order.
//
// can_have_reflection_recur is pure reachability: its result for a start tile is 1 exactly when some tile that is reachable by its steps -- every tile but the
// start entered through the line clip of the step's dimension -- passes the water test.  What a visit does (the water test, the two steps) does not depend on the
// dimension it was entered through, so a tile that was entered once and found nothing need not be entered again: reflect_walk keeps a visited set (the caller's)
// and a work list instead of the call stack.  vis_ref_call never fires: every step moves one tile nearer to the camera in x or in y.
#pragma once
#include "terra_view.hpp"
#include "terra_terrainview.hpp"

namespace terra {

enum {TV_NO_REFLECTION = 6};                                                                                   // status: dropped at :2869
enum {RF_NOT_ASKED = 0, RF_NO_WATER = 1, RF_WALK_NOTHING = 2, RF_HAS_WATER = 3, RF_WALK_FOUND = 4};            // the reflect byte
enum {WV_PRESENT = 1, WV_HAS_WATER = 2, WV_NEAR = 4, WV_VISIBLE = 8};                                          // what the water view keeps of a tile

struct reflection_view_args_pod_t {terrain_view_args_pod_t tv; float zmax;}; // terra_reflection_view_args
struct water_view_args_pod_t {float behind_sphere_mult; int32_t water_enabled;}; // terra_water_view_args

struct reflect_consts_t {terrain_view_consts_t tv; float zmin, zmax;}; // the global zmin / zmax of :2634-2635
struct reflect_box_t {int32_t x0, y0; uint32_t w, nwords, cap;}; // the bounding box of the batch's tile positions: origin, width, the words of its bits, the work list's room

TERRA_HD bool tile_has_water(terrain_view_consts_t const &c, terra_tile_stats const &st) {return st.mzmin < c.water_plane_z;} // has_water()
TERRA_HD bool tile_all_water(terrain_view_consts_t const &c, terra_tile_stats const &st) {return st.mzmax < c.water_plane_z;} // all_water()

// rel_dist_to_camera_xy_lt(rel_dist): dist_xy_less_than(get_camera_pos(), get_center(), rel_dist*get_scaled_tile_radius() + radius)
TERRA_HD bool terrain_view_dist_xy_lt(terrain_view_consts_t const &c, terrain_view_geom_t const &g, float radius, float rel_dist) {
	float const *cam = c.v.pos;
	float const dval = rel_dist*c.scaled_tile_radius + radius;
	return (cam[0] - g.cx)*(cam[0] - g.cx) + (cam[1] - g.cy)*(cam[1] - g.cy) < dval*dval;
}
// get_water_bcube(): the int water box of the stats, zero height
TERRA_HD void tile_water_box(terrain_view_consts_t const &c, terra_tile_stats const &st, float d[3][2]) {
	float const xv1 = -c.xss + c.DX_VAL*(float)(int)((uint32_t)st.wx1 + (uint32_t)c.dxoff), yv1 = -c.yss + c.DY_VAL*(float)(int)((uint32_t)st.wy1 + (uint32_t)c.dyoff);
	d[0][0] = xv1; d[0][1] = xv1 + (float)(int)((uint32_t)st.wx2 - (uint32_t)st.wx1)*c.DX_VAL;
	d[1][0] = yv1; d[1][1] = yv1 + (float)(int)((uint32_t)st.wy2 - (uint32_t)st.wy1)*c.DY_VAL;
	d[2][0] = c.water_plane_z; d[2][1] = c.water_plane_z;
}
TERRA_HD float reflect_dist_xy(float ax, float ay, float bx, float by) {return sqrtf((ax - bx)*(ax - bx) + (ay - by)*(ay - by));} // p2p_dist_xy

// what the walk reads of a tile, left by the pass's first step: get_bcube() and four facts
enum {RT_ENTERABLE = 1, RT_HAS_WATER = 2, RT_ALL_WATER = 4, RT_OCCLUDED_IN = 8}; // present and is_visible(); has_water(); all_water(); the incoming occl_state is 1
struct alignas(16) reflect_tile_t {float bc[3][2]; uint32_t flags, pad;};
static_assert(sizeof(reflect_tile_t) == 32, "reflect_tile_t: two 16-byte loads");
TERRA_HD reflect_tile_t reflect_tile(terrain_view_consts_t const &c, terrain_view_in_t const &in, int32_t const *tile_xy, size_t t, bool visible) {
	reflect_tile_t r;
	r.pad = 0u;
	if ((in.flags ? in.flags[t] : 0u) & TV_FLAG_ABSENT) {
		for (int i = 0; i < 3; ++i) {r.bc[i][0] = 0.0f; r.bc[i][1] = 0.0f;}
		r.flags = 0u;
		return r;
	}
	terrain_view_geom_t const g = terrain_view_geom_of(c, in, tile_xy, t);
	for (int i = 0; i < 3; ++i) {r.bc[i][0] = g.bc[i][0]; r.bc[i][1] = g.bc[i][1];}
	r.flags = (visible ? RT_ENTERABLE : 0u) | (tile_has_water(c, in.stats[t]) ? RT_HAS_WATER : 0u) | (tile_all_water(c, in.stats[t]) ? RT_ALL_WATER : 0u) |
	          ((in.occl_state && in.occl_state[t] == TV_STATE_OCCLUDED) ? RT_OCCLUDED_IN : 0u);
	return r;
}
// corners[3] of can_have_reflection (:2671-2681): {x, y, closest}
struct reflect_corners_t {float p[3][3];};
TERRA_HD reflect_corners_t reflect_corners(terrain_view_consts_t const &c, float const bc[3][2], float mzmax) {
	reflect_corners_t k;
	float const *cam = c.v.pos;
	for (int d = 0; d < 2; ++d) {
		float const center = 0.5f*(bc[d][0] + bc[d][1]); // get_cube_center()
		k.p[d][d]     = (center < cam[d]) ? bc[d][1] : bc[d][0]; // bcube.d[d][center[d] < camera[d]]
		k.p[1 - d][d] = (center > cam[d]) ? bc[d][1] : bc[d][0]; // bcube.d[d][center[d] > camera[d]]
		k.p[d][2]     = bc[2][0];
	}
	for (int d = 0; d < 3; ++d) {k.p[2][d] = min_std(bc[d][1], max_std(bc[d][0], cam[d]));} // bcube.closest_pt(camera)
	k.p[2][2] = mzmax; // get_zmax()
	return k;
}
// the box of :2633-2635 and the test of :2636 for dim_ix < 2: check_line_clip(camera, corners[dim_ix], bcube.d)
TERRA_HD bool reflect_enter(reflect_consts_t const &c, float const bc[3][2], reflect_corners_t const &k, uint32_t dim_ix) {
	float d[3][2];
	for (int i = 0; i < 2; ++i) {d[i][0] = bc[i][0]; d[i][1] = bc[i][1];}
	d[2][0] = min_std(bc[2][0], c.zmin); d[2][1] = max_std(bc[2][1], c.zmax); // make sure the line isn't clipped in z
	shadow_pt_t v1 = {c.tv.v.pos[0], c.tv.v.pos[1], c.tv.v.pos[2]}, v2 = {k.p[dim_ix][0], k.p[dim_ix][1], k.p[dim_ix][2]};
	return shadow_line_clip(v1, v2, d);
}
// the water test of :2638-2646 behind `!was_last_occluded() && has_water()`.  The division can give inf, or NaN where closest_pt lies under the camera; the
// comparison then does what IEEE says
TERRA_HD bool reflect_water_test(terrain_view_consts_t const &c, terra_tile_stats const &st, reflect_corners_t const &k) {
	float w[3][2];
	tile_water_box(c, st, w);
	if (!view_cube_visible(c.v, w)) return false;
	float const px = min_std(w[0][1], max_std(w[0][0], k.p[2][0])), py = min_std(w[1][1], max_std(w[1][0], k.p[2][1])); // water_bcube.closest_pt(corners[2])
	float const z_over_xy = (c.v.pos[2] - c.water_plane_z)/reflect_dist_xy(c.v.pos[0], c.v.pos[1], px, py); // slope
	return c.water_plane_z + z_over_xy*reflect_dist_xy(k.p[2][0], k.p[2][1], px, py) < k.p[2][2];
}
// the step of :2652-2655 in dimension d: -1, 1, or 0 for the `continue`
TERRA_HD int reflect_step(terrain_view_consts_t const &c, float const bc[3][2], uint32_t d) {
	float const cam = c.v.pos[d];
	return (cam < bc[d][0]) ? -1 : ((cam > bc[d][1]) ? 1 : 0);
}
// can_have_reflection_recur(start, corners, 2) as a work list.  rt: the tiles' records; work: room for `cap` >= 1 batch indices; seen(u): marks tile u, true if it was
// marked before; occluded(u): was_last_occluded() of tile u as the start tile's turn of the loop of :2863 sees it.  A work list that would outgrow `cap` (no walk
// that only nears the camera can) loses an entry.  pin(k): a kernel's hook on the visit's copy of the corners (see k_reflect_walk); it changes no value
template<class SEEN, class OCCLUDED, class PIN> TERRA_HD bool reflect_walk(reflect_consts_t const &c, terra_tile_stats const *stats, int32_t const *nbr, reflect_tile_t const *rt,
	uint32_t start, reflect_corners_t const &k0, int32_t *work, uint32_t cap, SEEN seen, OCCLUDED occluded, PIN pin)
{
	uint32_t sp = 0;
	seen(start);
	work[sp++] = (int32_t)start;
	while (sp) {
		uint32_t const t = (uint32_t)work[--sp];
		reflect_corners_t k = k0;
		pin(k);
		reflect_tile_t const r = rt[t];
		if ((r.flags & RT_HAS_WATER) && !occluded(t)) {
			if (reflect_water_test(c.tv, stats[t], k)) return true;
		}
		_Pragma("unroll") for (uint32_t d = 0; d < 2; ++d) {
			int const s = reflect_step(c.tv, r.bc, d);
			if (s == 0) continue;
			int32_t const u = nbr[(size_t)t*9u + (d ? (s > 0 ? 7u : 1u) : (s > 0 ? 5u : 3u))]; // get_tile_xy_pair(delta[0], delta[1])
			if (u < 0) continue;                          // !adj
			reflect_tile_t const a = rt[u];
			if (!(a.flags & RT_ENTERABLE)) continue;      // absent, or !adj->is_visible()
			if (!reflect_enter(c, a.bc, k, d)) continue;  // not within the shadow of the original tile
			if (seen((uint32_t)u)) continue;
			work[(sp < cap) ? sp : cap - 1u] = u; // (a full list loses an entry)
			sp = (sp < cap) ? sp + 1u : sp;
		}
	}
	return false;
}
// can_have_reflection (:2665-2683) up to the walk: the reflect byte where no walk is needed, else RF_NOT_ASKED
TERRA_HD uint32_t reflect_without_walk(terrain_view_consts_t const &c, uint32_t flags) {
	if (!c.water_enabled) return RF_NO_WATER;
	if (flags & RT_ALL_WATER) return RF_NO_WATER;
	if (flags & RT_HAS_WATER) return RF_HAS_WATER;
	return RF_NOT_ASKED;
}

// ---- the water view: what is_water_visible() and draw_water_cap read of a tile
TERRA_HD uint32_t water_view_tile(terrain_view_consts_t const &c, terrain_view_in_t const &in, int32_t const *tile_xy, size_t t) {
	if ((in.flags ? in.flags[t] : 0u) & TV_FLAG_ABSENT) return 0u;
	terra_tile_stats const &st = in.stats[t];
	terrain_view_geom_t const g = terrain_view_geom_of(c, in, tile_xy, t);
	float const DRAW_DIST_TILES = 1.5f;
	return WV_PRESENT | (tile_has_water(c, st) ? WV_HAS_WATER : 0u) | (terrain_view_dist_xy_lt(c, g, st.radius, DRAW_DIST_TILES) ? WV_NEAR : 0u) |
	       (terrain_view_visible(c, g, st.mzmin, st.mzmax, st.radius) ? WV_VISIBLE : 0u);
}
TERRA_HD bool water_view_listed(uint32_t w) {return (w & (WV_PRESENT | WV_HAS_WATER | WV_NEAR | WV_VISIBLE)) == (WV_PRESENT | WV_HAS_WATER | WV_NEAR | WV_VISIBLE);} // is_water_visible()
// draw_water_cap for tile t (its water-view byte w, its terrain status): bit 2*dim + dir where the edge's quad is emitted (:2102-2119)
TERRA_HD uint32_t water_view_caps(terrain_view_consts_t const &c, uint32_t w, uint32_t status, int32_t const *nbr, uint8_t const *wv, size_t t) {
	uint32_t const me = status & TV_STATUS_MASK;
	if (!c.water_enabled || !(w & WV_PRESENT)) return 0u;
	if (!((me == TV_DRAWN && (w & WV_HAS_WATER)) || me == TV_OCCLUDED)) return 0u; // draw_near_water (:2046, :2078); occluded_tiles (:2957-2959)
	uint32_t mask = 0;
	for (uint32_t k = 0; k < 4u; ++k) {
		int32_t const u = nbr[t*9u + terrain_view_nbr_slot(k >> 1, k & 1u)];
		uint32_t const a = (u >= 0) ? (uint32_t)wv[u] : 0u;
		if ((a & WV_PRESENT) && ((a & WV_NEAR) || !(a & WV_HAS_WATER) || !(a & WV_VISIBLE))) continue; // :2108-2112
		mask |= 1u << k;
	}
	return mask;
}

TERRA_HD bool reflection_view_args_finite(reflection_view_args_pod_t const &a) {return terrain_view_args_finite(a.tv) && isfinite(a.zmax);}

// ---- the reflection view: the terrain view's records (terrain_view_io_t, terrain_view_io_check, terrain_view_scratch_t), all of the scratch
inline void reflection_view_scratch_add(stage_layout_t &lay, terrain_view_scratch_t &s, uint32_t n) {
	lay.add(s.rc, 1); lay.add(s.rt, n); lay.add(s.occ, n); lay.add(s.txy, (size_t)n*2); lay.add(s.nbr, (size_t)n*9); lay.add(s.nocc, 4); lay.add(s.keys, n); lay.add(s.key_tile, n); lay.add(s.mark, n);
	lay.add(s.work, n); lay.add(s.test, n); lay.add(s.prov, n); lay.add(s.refl, n); lay.add(s.state, n);
}
// the literal bodies of its simple form.  (1) a logical thread per tile: the terrain view's first step, and what the loop of :2863 reads of the tile
TERRA_HD void reflection_view_tile_literal(terrain_view_consts_t const &c, terrain_view_io_t const &io, terrain_view_scratch_t const &s, size_t t) {
	terrain_view_tile_t const o = terrain_view_tile_literal(c, io, s, t);
	s.rt[t] = reflect_tile(c, io.in, s.txy, t, o.visible != 0);
	s.state[t] = io.in.occl_state ? io.in.occl_state[t] : (uint8_t)TV_STATE_NONE; s.mark[t] = 0u;
	if (io.reflect) {io.reflect[t] = RF_NOT_ASKED;}
}
// (2) one thread: the occluders in batch order, then the loop of :2863 as written, in batch order: a tile's walk sees what the turns before it left of last_occluded.  c: the
// launch's own copy of rc.tv (as an alias of rc.tv the kernel reloaded n from its arguments in every skipped turn of the occluder loop: 3% at 4096 tiles)
TERRA_HD void reflection_view_loop_literal(terrain_view_consts_t const &c, reflect_consts_t const &rc, terrain_view_io_t const &io, terrain_view_scratch_t const &s, uint32_t n) {
	terrain_view_in_t const &in = io.in;
	uint32_t const nocc = terrain_view_occluders_literal(c, io, s, n);
	for (uint32_t t = 0; t < n; ++t) {
		if ((io.status[t] & TV_STATUS_MASK) != TV_DRAWN) continue;
		terrain_view_geom_t const g = terrain_view_geom_of(c, in, s.txy, t);
		uint32_t r = reflect_without_walk(c, s.rt[t].flags);
		if (r == RF_NOT_ASKED) {
			reflect_corners_t const k = reflect_corners(c, g.bc, in.stats[t].mzmax);
			auto seen = [&](uint32_t u) {bool const was = s.mark[u] == t + 1u; s.mark[u] = t + 1u; return was;};
			auto occluded = [&](uint32_t u) {return s.state[u] == TV_STATE_OCCLUDED;};
			r = reflect_walk(rc, in.stats, s.nbr, s.rt, t, k, s.work, n, seen, occluded, [](reflect_corners_t &) {}) ? RF_WALK_FOUND : RF_WALK_NOTHING;
		}
		if (io.reflect) {io.reflect[t] = (uint8_t)r;}
		if (r < RF_HAS_WATER) {io.status[t] = (uint8_t)((io.status[t] & ~TV_STATUS_MASK) | TV_NO_REFLECTION); continue;} // :2869
		if (!s.test[t] || nocc == 0) continue;
		bool const occluded_now = terrain_view_occluded(c, g, in.stats[t], s.occ, nocc, (int32_t)t);
		if (occluded_now) {io.status[t] = (uint8_t)((io.status[t] & ~TV_STATUS_MASK) | TV_OCCLUDED);}
		s.state[t] = occluded_now ? TV_STATE_OCCLUDED : TV_STATE_UNOCCLUDED; // set_last_occluded (:2906)
		if (in.occl_state) {in.occl_state[t] = s.state[t];}
	}
}

// ---- the arrays of a water view call, in the order of terra_tiles_water_view[_dev] (in.min_normal_z and in.occl_state are not the pass's: null)
struct water_view_io_t {terrain_view_in_t in; uint8_t const *status; uint32_t *water_list; uint8_t *cap_mask; uint32_t *counts;};
// the argument rules of a call, behind water_view_check: throws what the call refuses; false: nothing to do (n == 0).  dev: the arrays are the device's
inline bool water_view_io_check(int32_t const *tile_xy, uint32_t n, water_view_io_t const &io, bool dev) {
	if ((io.status != nullptr) != (io.cap_mask != nullptr)) throw std::invalid_argument("tiles_water_view: status and cap_mask are both null or both given");
	if (n == 0) return false;
	if (!tile_xy || !io.in.stats || !io.water_list || !io.counts) throw std::invalid_argument("tiles_water_view: null argument");
	if (dev && (((uintptr_t)io.in.stats | (uintptr_t)io.in.trmax | (uintptr_t)io.in.tile_zmax | (uintptr_t)io.water_list | (uintptr_t)io.counts) & 3u) != 0) throw std::invalid_argument(
		"tiles_water_view: d_stats, d_trmax, d_tile_zmax, d_water_list and d_counts must be 4-byte aligned");
	return true;
}
// scratch: the coordinates, the neighbour table, and what the pass keeps of a tile (WV_*)
struct water_view_scratch_t {int32_t *txy, *nbr; uint8_t *wv;};
inline void water_view_scratch_add(stage_layout_t &lay, water_view_scratch_t &s, uint32_t n) {lay.add(s.txy, (size_t)n*2); lay.add(s.nbr, (size_t)n*9); lay.add(s.wv, n);}
// the literal body of the simple form's second step, one thread (the first is water_view_tile, a thread per tile): tile_draw_t::draw_water's loop in batch order, then the caps
TERRA_HD void water_view_lists_literal(terrain_view_consts_t const &c, water_view_io_t const &io, water_view_scratch_t const &s, uint32_t n) {
	uint32_t nw = 0, nc = 0;
	for (uint32_t t = 0; t < n; ++t) {if (water_view_listed(s.wv[t])) {io.water_list[nw++] = t;}}
	io.counts[0] = nw;
	if (!io.status) return;
	for (uint32_t t = 0; t < n; ++t) {
		uint32_t const m = water_view_caps(c, s.wv[t], io.status[t], s.nbr, s.wv, t);
		io.cap_mask[t] = (uint8_t)m;
		nc += m ? 1u : 0u;
	}
	io.counts[1] = nc;
}

} // namespace terra
