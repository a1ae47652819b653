// terra_smapview.hpp -- the shadow-map plan of a tile batch: which tiles hold a shadow map and at which LOD, and which tiles are drawn into a receiver's shadow map.
// The plan: tile_t::update_range's shadow-map deletion (src/tiled_mesh.cpp:1416 with :1409), the loop of tile_draw_t::pre_draw (:2781-2799, its shadow part: the
// draw-distance gate of :2784, is_visible, is_smap_bounds_visible and the split into to_update_shadows against cleanup_only), tile_t::setup_shadow_maps (:981-1016)
// with calc_max_smap_lod (:975-980) and tile_t::get_shadow_bcube (:959-965), the gate of tile_t::try_bind_shadow_map (:1958-1959), the queue of :2445-2448 as
// :2459 consumes it, and the constants (:30-32; NUM_SMAP_LODS, src/tiled_mesh.h:26).  The casters: the head of tile_draw_t::draw_shadow_pass (:3025-3043), the
// filter of draw_tiles_shadow_pass (:3004-3018) with the `inside_city == 2` return of tile_t::draw_shadow_pass (:2083), cube_t::intersects_xy / contains_pt_xy
// (src/3DWorld.h:544-547,579) and p2p_dist_xy_sq (src/inlines.h:183-185).  The light's frustum: get_pt_cube_frustum_pdu (src/shadow_map.cpp:423-457) in its
// infinite-terrain form with get_min_dim (src/inlines.h:630-632), get_cube_corners (src/Math3d.cpp:1184-1193), cube_t::get_bsphere_radius (src/3DWorld.h:605-607)
// and pointT::get_norm / operator/ (:297-300,315-319).
//
// The bodies are shared by the driver's simple form (the reference's loop, sequential over the batch) and by the k_smap_* kernels (terra_kernels.hpp).  A tile's
// centre, get_bcube(), get_mesh_bcube(), is_visible, the radius with water and the camera distances are terra_terrainview.hpp's and terra_waterview.hpp's, the
// sphere and cube tests terra_view.hpp's: nothing of them is restated here.  Every operand carries the type the reference statement gives it; where the C++ source
// promotes to double the promotion is written out; sums run in the reference's order.  The tile size enters only through the boxes and the radius.
//
// The state of a tile is one byte: SMAP_NONE for smap_data.empty(), else smap_lod_level.  The reference keeps a stale smap_lod_level in a tile whose shadow maps
// were cleared; it is not observable: its uses (:998, :1000) only guard a clear_shadow_map that is a no-op on a tile without shadow maps, and :1006 overwrites it
// before anything else reads it.
//
// The order of the recompute queue: the reference sorts (-p2p_dist(sun_pos, get_center()), tile_xy_pair) ascending -- std::pair's operator< over a float and
// tile_xy_pair::operator<, which compares y, then x: a total order on distinct tiles -- and pops from the back.  The place of a tile in recomp_order is the number
// of present tiles that come after it in that order (the batch index breaks the tie of a tile that the batch names twice).
#pragma once
#include "terra_view.hpp"
#include "terra_terrainview.hpp"
#include "terra_waterview.hpp"
#include <math.h>
#include <stdexcept>

namespace terra {

constexpr uint8_t  SMAP_NONE = 0xFF;  // the state byte of a tile without shadow maps
constexpr uint32_t SMAP_LODS = 4;     // NUM_SMAP_LODS (src/tiled_mesh.h:26)
enum {SMP_IN_DRAW_DIST = 0x1, SMP_VISIBLE = 0x2, SMP_BOUNDS_VISIBLE = 0x4, SMP_UPDATE = 0x8, SMP_CLEARED_FAR = 0x10, SMP_CLEARED_WIREFRAME = 0x20, SMP_CLEARED_LOD_REDUCE = 0x40,
      SMP_CLEARED_LOD_RAISE = 0x80, SMP_ALLOCATED = 0x100, SMP_RECEIVER = 0x200, SMP_USABLE = 0x400, SMP_LOD_SHIFT = 16, SMP_REDUCE_SHIFT = 20}; // the plan word
enum {SMC_NO_TILE = 1};                                // the status byte of a render whose receiver is out of range or absent
enum {TV_FLAG_FULLY_IN_CITY = 8};                      // flags: inside_city == 2 (:2083)
enum {SG_PRESENT = 1, SG_IN_CITY = 2, SG_NO_DECID = 4}; // what the casters keep of a tile

struct smap_plan_args_pod_t { // terra_smap_plan_args
	float behind_sphere_mult; int32_t water_enabled; float smap_thresh_scale; uint32_t shadow_map_sz; int32_t have_buildings, draw_model;
	float b_ext[3], road_len[2], models_z2; int32_t models_valid; float sun_pos[3]; int32_t want_recomp;
};
struct smap_cast_args_pod_t {int32_t water_enabled, decid_trees_only, inc_adj_smap; float b_ext[3], road_len[2];}; // terra_smap_cast_args

// calc_max_smap_lod (:975-980)
TERRA_HD uint32_t smap_max_lod(uint32_t shadow_map_sz, bool have_buildings) {
	uint32_t const min_smap_sz = have_buildings ? 1024u : 512u;
	uint32_t lod_level = 0;
	for (uint32_t smap_sz = shadow_map_sz; smap_sz > min_smap_sz && lod_level + 1u < SMAP_LODS; ++lod_level) {smap_sz >>= 1;}
	return lod_level;
}

struct smap_consts_t {
	terrain_view_consts_t tv;   // the view, behind_sphere_mult, the scene, the offsets, water_enabled
	float thresh_scale;         // smap_thresh_scale
	uint32_t sz, max_lod;       // shadow_map_sz (0: shadow_map_enabled() is false), calc_max_smap_lod()
	int draw_model;
	float x_ext0, y_ext0, bz;   // max(0.5f*road_len.x, b_ext.x), the same in y, b_ext.z (get_shadow_bcube, :963-964)
	float models_z2; int models_valid;
	float sun[3]; int want_recomp;
};
inline smap_consts_t smap_consts(view_pod_t const &v, float behind_sphere_mult, int water_enabled, float const b_ext[3], float const road_len[2], float xss, float yss, float DX_VAL,
	float DY_VAL, int S, int dxoff, int dyoff, float water_plane_z)
{
	smap_consts_t c;
	terrain_view_args_pod_t const ta = {behind_sphere_mult, 0.0f, water_enabled, 0, 0};
	c.tv = terrain_view_consts(v, ta, xss, yss, DX_VAL, DY_VAL, S, dxoff, dyoff, water_plane_z);
	c.thresh_scale = 1.0f; c.sz = 0u; c.max_lod = 0u; c.draw_model = 0;
	c.x_ext0 = max_std(0.5f*road_len[0], b_ext[0]); c.y_ext0 = max_std(0.5f*road_len[1], b_ext[1]); c.bz = b_ext[2];
	c.models_z2 = 0.0f; c.models_valid = 0; c.sun[0] = c.sun[1] = c.sun[2] = 0.0f; c.want_recomp = 0;
	return c;
}
inline smap_consts_t smap_plan_consts(view_pod_t const &v, smap_plan_args_pod_t const &a, float xss, float yss, float DX_VAL, float DY_VAL, int S, int dxoff, int dyoff, float water_plane_z) {
	smap_consts_t c = smap_consts(v, a.behind_sphere_mult, a.water_enabled, a.b_ext, a.road_len, xss, yss, DX_VAL, DY_VAL, S, dxoff, dyoff, water_plane_z);
	c.thresh_scale = a.smap_thresh_scale; c.sz = a.shadow_map_sz; c.max_lod = smap_max_lod(a.shadow_map_sz, a.have_buildings != 0); c.draw_model = a.draw_model;
	c.models_z2 = a.models_z2; c.models_valid = a.models_valid ? 1 : 0;
	for (int k = 0; k < 3; ++k) {c.sun[k] = a.sun_pos[k];}
	c.want_recomp = a.want_recomp ? 1 : 0;
	return c;
}
inline bool smap_plan_args_ok(smap_plan_args_pod_t const &a, char const *&why) {
	bool fin = isfinite(a.behind_sphere_mult) && isfinite(a.smap_thresh_scale) && isfinite(a.models_z2);
	for (int k = 0; k < 3; ++k) {fin = fin && isfinite(a.b_ext[k]) && isfinite(a.sun_pos[k]);}
	fin = fin && isfinite(a.road_len[0]) && isfinite(a.road_len[1]);
	if (!fin) {why = "tiles_smap_plan: a member of the args is not finite"; return false;}
	if (!(a.smap_thresh_scale > 0.0f)) {why = "tiles_smap_plan: smap_thresh_scale must be > 0"; return false;}
	return true;
}
inline bool smap_cast_args_finite(smap_cast_args_pod_t const &a) {
	bool fin = isfinite(a.road_len[0]) && isfinite(a.road_len[1]);
	for (int k = 0; k < 3; ++k) {fin = fin && isfinite(a.b_ext[k]);}
	return fin;
}

// tile_t::get_shadow_bcube (:959-965)
TERRA_HD void smap_shadow_box(smap_consts_t const &c, terrain_view_geom_t const &g, float mzmin, float mzmax, float trmax, float tile_zmax, float d[3][2]) {
	float const BCUBE_ZTOLER = 1.0E-6f;
	float const x_ext = max_std(c.x_ext0, trmax), y_ext = max_std(c.y_ext0, trmax);
	d[0][0] = g.xv1 - x_ext; d[0][1] = g.xv2 + x_ext; d[1][0] = g.yv1 - y_ext; d[1][1] = g.yv2 + y_ext;
	d[2][0] = mzmin - BCUBE_ZTOLER; d[2][1] = max_std(tile_zmax + BCUBE_ZTOLER, mzmax + c.bz);
}

// ---- the plan of one tile: update_range's deletion, the tile's turn of pre_draw's loop and its setup_shadow_maps call
struct smap_plan_tile_t {uint32_t plan; float dist_scale; float box[3][2]; float key; uint8_t state, present;}; // key: -p2p_dist(sun_pos, get_center()) (:2446)
TERRA_HD smap_plan_tile_t smap_plan_tile(smap_consts_t const &c, terrain_view_in_t const &in, int32_t const *tile_xy, uint8_t state_in, size_t t) {
	smap_plan_tile_t o;
	o.plan = 0u; o.dist_scale = 0.0f; o.key = 0.0f; o.state = state_in; o.present = 0;
	for (int k = 0; k < 3; ++k) {o.box[k][0] = 0.0f; o.box[k][1] = 0.0f;}
	if ((in.flags ? in.flags[t] : 0u) & TV_FLAG_ABSENT) return o;
	o.present = 1;
	terra_tile_stats const &st = in.stats[t];
	terrain_view_geom_t const g = terrain_view_geom_of(c.tv, in, tile_xy, t);
	float const SMAP_NEW_THRESH = 1.2f, SMAP_DEL_THRESH = 1.3f, SMAP_FADE_THRESH = 1.5f, DRAW_DIST_TILES = 1.5f;
	int const TILE_RADIUS = 6;
	bool const enabled = c.sz != 0u; // shadow_map_enabled()
	uint32_t state = state_in;       // SMAP_NONE, or smap_lod_level
	uint32_t plan = 0u;
	{float const dx = c.sun[0] - g.cx, dy = c.sun[1] - g.cy, dz = c.sun[2] - g.cz; o.key = -sqrtf(dx*dx + dy*dy + dz*dz);}
	// update_range (:1409, :1416)
	float const dist = terrain_view_rel_dist_xy(c.tv, g, st.radius); // get_rel_dist_to_camera()
	if (dist*(float)TILE_RADIUS > SMAP_DEL_THRESH*c.thresh_scale) {
		if (state != SMAP_NONE) {plan |= SMP_CLEARED_FAR;}
		state = SMAP_NONE;
	}
	float const in_tiles = dist*(float)TILE_RADIUS; // get_dist_to_camera_in_tiles(1)
	// pre_draw's loop (:2784-2791)
	if (terrain_view_dist_xy_lt(c.tv, g, st.radius, DRAW_DIST_TILES)) {
		plan |= SMP_IN_DRAW_DIST;
		bool const visible = terrain_view_visible(c.tv, g, st.mzmin, st.mzmax, st.radius);
		smap_shadow_box(c, g, st.mzmin, st.mzmax, in.trmax ? in.trmax[t] : 0.0f, in.tile_zmax ? in.tile_zmax[t] : st.mzmax, o.box);
		bool const bounds = view_cube_visible(c.tv.v, o.box); // is_smap_bounds_visible()
		if (visible) {plan |= SMP_VISIBLE;}
		if (bounds) {plan |= SMP_BOUNDS_VISIBLE;}
		if (c.models_valid) {o.box[2][1] = max_std(o.box[2][1], c.models_z2);} // :1013-1014 (behind is_smap_bounds_visible, which reads get_shadow_bcube() itself)
		if (enabled) {
			bool const cleanup_only = !(visible || bounds);
			if (!cleanup_only) {plan |= SMP_UPDATE;}
			// setup_shadow_maps(smap_manager, cleanup_only) (:981-1016)
			if (c.draw_model != 0) {
				if (state != SMAP_NONE) {plan |= SMP_CLEARED_WIREFRAME;}
				state = SMAP_NONE;
			}
			else {
				float const smap_dist_scale = in_tiles/(SMAP_NEW_THRESH*c.thresh_scale);
				o.dist_scale = smap_dist_scale;
				if ((double)smap_dist_scale < 1.0) {
					float const lod_level_f = min_std(5.0f*smap_dist_scale, (float)c.max_lod);
					uint32_t lod_level = f2u_x86(floorf(lod_level_f)), lod_level_reduce = f2u_x86(floorf(max_std(0.0f, lod_level_f - 0.1f)));
					if (c.sz >= 8192u) { // :994: !get_mesh_bcube().contains_pt_xy(get_camera_pos())
						float const *cam = c.tv.v.pos;
						bool const inside = cam[0] > g.xv1 && cam[0] < g.xv2 && cam[1] > g.yv1 && cam[1] < g.yv2;
						if (!inside) {
							if (lod_level == 0u) {lod_level_reduce = 1u;}
							lod_level = (c.max_lod < lod_level + 1u) ? c.max_lod : lod_level + 1u; // min(lod_level+1, max_lod_level)
						}
					}
					plan |= (lod_level << SMP_LOD_SHIFT) | (lod_level_reduce << SMP_REDUCE_SHIFT);
					if (state != SMAP_NONE && lod_level_reduce > state) {plan |= SMP_CLEARED_LOD_REDUCE; state = SMAP_NONE;}
					if (!cleanup_only) {
						if (state != SMAP_NONE && lod_level < state) {plan |= SMP_CLEARED_LOD_RAISE; state = SMAP_NONE;}
						if (state == SMAP_NONE) {plan |= SMP_ALLOCATED; state = lod_level;}
					}
				}
				if (!cleanup_only && state != SMAP_NONE) {plan |= SMP_RECEIVER;} // :1015: create_if_needed on a tile that holds shadow maps
			}
		}
	}
	// try_bind_shadow_map's gate (:1958-1959) on the new state
	if (enabled && state != SMAP_NONE && !(in_tiles > SMAP_FADE_THRESH*c.thresh_scale)) {plan |= SMP_USABLE;}
	o.plan = plan; o.state = (uint8_t)state;
	return o;
}

// ---- the recompute queue: what the rank reads of a tile, and a tile's place
struct alignas(16) smap_rank_key_t {float key; int32_t y, x; uint32_t present;};
// does (a, ia) come after (b, ib) in the sorted queue?  std::pair<float, tile_xy_pair>'s operator<, b < a
TERRA_HD bool smap_queue_after(smap_rank_key_t const &a, uint32_t ia, smap_rank_key_t const &b, uint32_t ib) {
	if (b.key < a.key) return true;
	if (a.key < b.key) return false;
	if (b.y != a.y) return b.y < a.y;
	if (b.x != a.x) return b.x < a.x;
	return ib < ia;
}
// how many of the m records keys[0 .. m) -- the tiles base .. base + m - 1 -- are present and come after tile t (record me) in the sorted queue
TERRA_HD uint32_t smap_recomp_count(smap_rank_key_t const *keys, uint32_t m, uint32_t base, smap_rank_key_t const &me, uint32_t t) {
	uint32_t place = 0;
	for (uint32_t j = 0; j < m; ++j) {smap_rank_key_t const k = keys[j]; place += (k.present && smap_queue_after(k, base + j, me, t)) ? 1u : 0u;}
	return place;
}
// the place of present tile t in the order in which pop_back (:2459) yields the queue
TERRA_HD uint32_t smap_recomp_place(smap_rank_key_t const *keys, uint32_t n, uint32_t t) {return smap_recomp_count(keys, n, 0u, keys[t], t);}

// ---- the arrays of a plan call, in the order of terra_tiles_smap_plan[_dev]
struct smap_plan_io_t {
	terra_tile_stats const *stats; float const *trmax, *tile_zmax; uint8_t const *flags; uint8_t *smap_state;
	uint32_t *plan; float *dist_scale, *shadow_bcube; uint32_t *receivers, *counts; uint8_t *terrain_flags; uint32_t *recomp_order;
};
// the argument rules of a plan call, behind the checks that need no array: throws what the call refuses; false: nothing to do (n == 0).  dev: the arrays are the device's
inline bool smap_plan_io_check(int32_t const *tile_xy, uint32_t n, smap_plan_io_t const &io, bool dev) {
	if (n == 0) return false;
	if (!tile_xy || !io.stats || !io.smap_state || !io.plan || !io.dist_scale || !io.shadow_bcube || !io.receivers || !io.counts) throw std::invalid_argument("tiles_smap_plan: null argument");
	if (dev && (((uintptr_t)io.stats | (uintptr_t)io.trmax | (uintptr_t)io.tile_zmax | (uintptr_t)io.plan | (uintptr_t)io.dist_scale | (uintptr_t)io.shadow_bcube | (uintptr_t)io.receivers |
	             (uintptr_t)io.counts | (uintptr_t)io.recomp_order) & 3u) != 0) throw std::invalid_argument("tiles_smap_plan: every array but flags, smap_state and terrain_flags must be 4-byte aligned");
	return true;
}
// what a tile's plan leaves in the per-tile arrays (the lists aside)
TERRA_HD void smap_plan_store(smap_plan_io_t const &io, smap_plan_tile_t const &o, size_t t) {
	io.plan[t] = o.plan; io.dist_scale[t] = o.dist_scale;
	if (!o.present) return;
	io.smap_state[t] = o.state;
	if (o.plan & SMP_IN_DRAW_DIST) {for (int k = 0; k < 6; ++k) {io.shadow_bcube[t*6 + k] = o.box[k >> 1][k & 1];}}
	if (io.terrain_flags && o.state != SMAP_NONE) {io.terrain_flags[t] = (uint8_t)(io.terrain_flags[t] | TV_FLAG_SHADOW_MAPS);}
}
// the literal body: the reference's loops, sequential over the batch.  keys: n records of scratch
TERRA_HD void smap_plan_literal_tiles(smap_consts_t const &c, terrain_view_in_t const &in, smap_plan_io_t const &io, int32_t const *tile_xy, uint32_t n, smap_rank_key_t *keys) {
	uint32_t nr = 0, np = 0;
	for (uint32_t t = 0; t < n; ++t) {
		smap_plan_tile_t const o = smap_plan_tile(c, in, tile_xy, io.smap_state[t], t);
		smap_plan_store(io, o, t);
		smap_rank_key_t k; k.key = o.key; k.y = tile_xy[2*t + 1]; k.x = tile_xy[2*t]; k.present = o.present;
		keys[t] = k;
		np += o.present ? 1u : 0u;
		if (o.plan & SMP_RECEIVER) {io.receivers[nr++] = t;}
	}
	io.counts[0] = nr; io.counts[1] = (c.want_recomp && io.recomp_order) ? np : 0u;
}
TERRA_HD void smap_plan_literal(smap_consts_t const &c, terrain_view_in_t const &in, smap_plan_io_t const &io, int32_t const *tile_xy, uint32_t n, smap_rank_key_t *keys) {
	smap_plan_literal_tiles(c, in, io, tile_xy, n, keys);
	if (!c.want_recomp || !io.recomp_order) return;
	for (uint32_t t = 0; t < n; ++t) {if (keys[t].present) {io.recomp_order[smap_recomp_place(keys, n, t)] = t;}}
}

// ---- the casters.  What every render reads of a tile, made once per call: get_center(), get_bsphere_radius_inc_water(), get_bcube(), the xy of get_shadow_bcube()
struct alignas(16) smap_geom_t {float cx, cy, cz, r; float bc[3][2]; float sb[2][2]; uint32_t flags, pad;};
static_assert(sizeof(smap_geom_t) == 64, "smap_geom_t: four 16-byte loads");
TERRA_HD smap_geom_t smap_geom(smap_consts_t const &c, terrain_view_in_t const &in, uint32_t const *decid_counts, int decid_trees_only, int32_t const *tile_xy, size_t t) {
	smap_geom_t o;
	uint32_t const fl = in.flags ? in.flags[t] : 0u;
	o.pad = 0u;
	if (fl & TV_FLAG_ABSENT) {
		o.cx = o.cy = o.cz = o.r = 0.0f; o.flags = 0u;
		for (int k = 0; k < 3; ++k) {o.bc[k][0] = 0.0f; o.bc[k][1] = 0.0f;}
		for (int k = 0; k < 2; ++k) {o.sb[k][0] = 0.0f; o.sb[k][1] = 0.0f;}
		return o;
	}
	terra_tile_stats const &st = in.stats[t];
	terrain_view_geom_t const g = terrain_view_geom_of(c.tv, in, tile_xy, t);
	o.cx = g.cx; o.cy = g.cy; o.cz = g.cz; o.r = terrain_view_radius_inc_water(c.tv, st.mzmin, st.mzmax, st.radius);
	for (int k = 0; k < 3; ++k) {o.bc[k][0] = g.bc[k][0]; o.bc[k][1] = g.bc[k][1];}
	float d[3][2];
	smap_shadow_box(c, g, st.mzmin, st.mzmax, in.trmax ? in.trmax[t] : 0.0f, in.tile_zmax ? in.tile_zmax[t] : st.mzmax, d);
	for (int k = 0; k < 2; ++k) {o.sb[k][0] = d[k][0]; o.sb[k][1] = d[k][1];}
	o.flags = SG_PRESENT | ((fl & TV_FLAG_FULLY_IN_CITY) ? SG_IN_CITY : 0u) | ((decid_trees_only && decid_counts[t] == 0u) ? SG_NO_DECID : 0u);
	return o;
}
// what a render keeps of its receiver: recv_dist_sq (:3004), the xy of shadow_bcube (:3005)
struct smap_recv_t {float lx, ly, dist_sq, sb[2][2]; int ok;};
TERRA_HD smap_recv_t smap_recv(smap_geom_t const *geom, uint32_t n, uint32_t recv, float const lpos[3]) {
	smap_recv_t o;
	o.lx = lpos[0]; o.ly = lpos[1]; o.dist_sq = 0.0f; o.ok = 0;
	for (int k = 0; k < 2; ++k) {o.sb[k][0] = 0.0f; o.sb[k][1] = 0.0f;}
	if (recv >= n) return o;
	smap_geom_t const g = geom[recv];
	if (!(g.flags & SG_PRESENT)) return o;
	o.ok = 1;
	o.dist_sq = (lpos[0] - g.cx)*(lpos[0] - g.cx) + (lpos[1] - g.cy)*(lpos[1] - g.cy); // p2p_dist_xy_sq(lpos, tile->get_center())
	for (int k = 0; k < 2; ++k) {o.sb[k][0] = g.sb[k][0]; o.sb[k][1] = g.sb[k][1];}
	return o;
}
// a tile's turn of the loops of :3037-3043 and :3010-3018: bit 0 it joins to_draw, bit 1 it reaches draw_mesh_vbo
TERRA_HD uint32_t smap_cast_tile(view_pod_t const &v, float behind_sphere_mult, smap_geom_t const &g, smap_recv_t const &rc, int decid_trees_only, int inc_adj_smap) {
	if (!rc.ok || !(g.flags & SG_PRESENT)) return 0u;
	if (g.flags & SG_NO_DECID) return 0u; // :3038
	if (!view_sphere_and_cube_visible(v, behind_sphere_mult, g.cx, g.cy, g.cz, g.r, g.bc)) return 0u; // :3039
	if (decid_trees_only) return 1u; // :3046
	bool const nearer = (rc.lx - g.cx)*(rc.lx - g.cx) + (rc.ly - g.cy)*(rc.ly - g.cy) <= rc.dist_sq; // :3013
	bool const overlap = inc_adj_smap && !(rc.sb[0][1] < g.bc[0][0] || rc.sb[0][0] > g.bc[0][1]) && !(rc.sb[1][1] < g.bc[1][0] || rc.sb[1][0] > g.bc[1][1]); // :3014: intersects_xy
	return ((nearer || overlap) && !(g.flags & SG_IN_CITY)) ? 3u : 1u; // :2083
}
// ---- the arithmetic of the two-list compaction of a workgroup (k_smap_casters' tp_block_rank2): m0 / m1 are a wave's ballots of the two flags.  A wave leaves
// its two counts as the halves of one word; a lane's rank in a list is the counts of the waves before its own plus the flagged lanes below it in its wave
TERRA_HD uint32_t smap_rank2_word(unsigned long long m0, unsigned long long m1) {return (uint32_t)__builtin_popcountll(m0) | ((uint32_t)__builtin_popcountll(m1) << 16);}
struct smap_rank2_t {uint32_t r0, r1, n0, n1;};
TERRA_HD smap_rank2_t smap_rank2(uint32_t const *s_wave, uint32_t waves, uint32_t w, uint32_t lane, unsigned long long m0, unsigned long long m1) {
	uint32_t before = 0, all = 0;
	for (uint32_t k = 0; k < waves; ++k) {uint32_t const v = s_wave[k]; all += v; if (k < w) {before += v;}}
	unsigned long long const below = (1ull << lane) - 1ull;
	smap_rank2_t q;
	q.n0 = all & 0xFFFFu; q.n1 = all >> 16;
	q.r0 = (before & 0xFFFFu) + (uint32_t)__builtin_popcountll(m0 & below); q.r1 = (before >> 16) + (uint32_t)__builtin_popcountll(m1 & below);
	return q;
}
// the light's view as the call uses it: near_ = 0 (:3032)
TERRA_HD view_pod_t smap_cast_view(view_pod_t const &in) {view_pod_t v = in; v.near_ = 0.0f; return v;}

// ---- the arrays of a casters call, in the order of terra_tiles_smap_casters[_dev].  recv is the device's in the device form; views, bsm and lpos are host arrays in both
struct smap_cast_io_t {
	terra_tile_stats const *stats; float const *trmax, *tile_zmax; uint8_t const *flags; uint32_t const *decid_counts; uint32_t const *recv;
	uint32_t *to_draw, *terrain, *counts; uint8_t *not_drawn, *status;
};
inline bool smap_cast_io_check(int32_t const *tile_xy, uint32_t n, uint32_t R, view_pod_t const *views, float const *bsm, float const *lpos, smap_cast_args_pod_t const &a,
	smap_cast_io_t const &io, bool dev)
{
	if ((uint64_t)R*n > 0xFFFFFFFFull) throw std::invalid_argument("tiles_smap_casters: R*n must fit 32 bits");
	if (n == 0 || R == 0) return false;
	if (!tile_xy || !io.stats || !io.recv || !views || !bsm || !lpos || !io.to_draw || !io.terrain || !io.counts || !io.not_drawn || !io.status || (a.decid_trees_only && !io.decid_counts)) {
		throw std::invalid_argument("tiles_smap_casters: null argument");
	}
	for (uint32_t r = 0; r < R; ++r) {
		if (!view_finite(views[r])) throw std::invalid_argument("tiles_smap_casters: a member of a view is not finite");
		if (!isfinite(bsm[r])) throw std::invalid_argument("tiles_smap_casters: a behind_sphere_mult is not finite");
		if (!isfinite(lpos[3*r]) || !isfinite(lpos[3*r + 1]) || !isfinite(lpos[3*r + 2])) throw std::invalid_argument("tiles_smap_casters: a member of lpos is not finite");
	}
	if (dev && (((uintptr_t)io.stats | (uintptr_t)io.trmax | (uintptr_t)io.tile_zmax | (uintptr_t)io.decid_counts | (uintptr_t)io.recv | (uintptr_t)io.to_draw | (uintptr_t)io.terrain |
	             (uintptr_t)io.counts) & 3u) != 0) throw std::invalid_argument("tiles_smap_casters: every array but flags, not_drawn and status must be 4-byte aligned");
	return true;
}
// the literal body: render r, the reference's loops over the batch
TERRA_HD void smap_casters_literal(smap_geom_t const *geom, smap_cast_io_t const &io, view_pod_t const *views, float const *bsm, float const *lpos, uint32_t n, int decid_trees_only,
	int inc_adj_smap, size_t r)
{
	view_pod_t const v = smap_cast_view(views[r]);
	smap_recv_t const rc = smap_recv(geom, n, io.recv[r], lpos + 3*r);
	uint32_t nd = 0, nt = 0;
	for (uint32_t t = 0; t < n; ++t) {
		uint32_t const w = smap_cast_tile(v, bsm[r], geom[t], rc, decid_trees_only, inc_adj_smap);
		io.not_drawn[r*n + t] = (w & 1u) ? 0 : 1;
		if (w & 1u) {io.to_draw[r*n + nd++] = t;}
		if (w & 2u) {io.terrain[r*n + nt++] = t;}
	}
	io.counts[2*r] = nd; io.counts[2*r + 1] = nt;
	io.status[r] = rc.ok ? 0 : (uint8_t)SMC_NO_TILE;
}

// ---- get_pt_cube_frustum_pdu (src/shadow_map.cpp:423-457) in its infinite-terrain form, into pos_dir_up's constructor (view_make) with the C library's atan2f.
// bounds: x1 x2 y1 y2 z1 z2, strictly normalized (:425).  false where the reference asserts or the constructor does
inline bool smap_light_view(float const lpos[3], float const bounds[6], float near_clip, view_pod_t &o, float &behind_sphere_mult) {
	if (!(bounds[0] < bounds[1] && bounds[2] < bounds[3] && bounds[4] < bounds[5])) return false;
	float const center[3] = {0.5f*(bounds[0] + bounds[1]), 0.5f*(bounds[2] + bounds[3]), 0.5f*(bounds[4] + bounds[5])}; // get_cube_center()
	float const ten = (float)10.0;
	float const pos[3] = {lpos[0]*ten, lpos[1]*ten, lpos[2]*ten}; // pos *= 10.0
	float const dist = sqrtf((pos[0] - center[0])*(pos[0] - center[0]) + (pos[1] - center[1])*(pos[1] - center[1]) + (pos[2] - center[2])*(pos[2] - center[2]));
	if (dist == 0.0f) return false; // operator/'s assert
	float const inv = (float)(1.0/(double)dist);
	float const light_dir[3] = {(center[0] - pos[0])*inv, (center[1] - pos[1])*inv, (center[2] - pos[2])*inv};
	float up_dir[3] = {0.0f, 0.0f, 0.0f};
	float const a0 = fabsf(light_dir[0]), a1 = fabsf(light_dir[1]), a2 = fabsf(light_dir[2]);
	up_dir[(a0 < a1) ? ((a0 < a2) ? 0 : 2) : ((a1 < a2) ? 1 : 2)] = 1.0f; // get_min_dim
	float const sx = bounds[1] - bounds[0], sy = bounds[3] - bounds[2], sz = bounds[5] - bounds[4];
	float const radius = 0.5f*sqrtf(sx*sx + sy*sy + sz*sz); // get_bsphere_radius()
	// orthogonalize_dir(up_dir, light_dir, dirs[1], 1); cross_product(light_dir, dirs[1], dirs[0])
	float const tx = up_dir[1]*light_dir[2] - up_dir[2]*light_dir[1], ty = up_dir[2]*light_dir[0] - up_dir[0]*light_dir[2], tz = up_dir[0]*light_dir[1] - up_dir[1]*light_dir[0];
	float d1[3] = {light_dir[1]*tz - light_dir[2]*ty, light_dir[2]*tx - light_dir[0]*tz, light_dir[0]*ty - light_dir[1]*tx};
	float const mag = sqrtf(d1[0]*d1[0] + d1[1]*d1[1] + d1[2]*d1[2]);
	if (mag >= 1.0E-12f) {float const m = (float)(1.0/(double)mag); d1[0] *= m; d1[1] *= m; d1[2] *= m;}
	float const d0[3] = {light_dir[1]*d1[2] - light_dir[2]*d1[1], light_dir[2]*d1[0] - light_dir[0]*d1[2], light_dir[0]*d1[1] - light_dir[1]*d1[0]};
	float rx = 0.0f, ry = 0.0f;
	for (unsigned i = 0; i < 8; ++i) { // get_cube_corners: ix = (((i<<1)+j)<<1)+k over x, y, z
		float dx = bounds[i >> 2] - pos[0], dy = bounds[2 + ((i >> 1) & 1)] - pos[1], dz = bounds[4 + (i & 1)] - pos[2];
		float const vmag = sqrtf(dx*dx + dy*dy + dz*dz);
		if (!(vmag < 1.0E-12f)) {dx = dx/vmag; dy = dy/vmag; dz = dz/vmag;} // get_norm()
		rx = max_std(rx, fabsf(view_dot(d0, dx, dy, dz))); ry = max_std(ry, fabsf(view_dot(d1, dx, dy, dz)));
	}
	float const frustum_skew_val = (float)(1.0 + 0.5*(double)sz/(double)dist);
	float const angle = atan2f(frustum_skew_val*ry, 1.0f), aspect = rx/ry;
	if (!isfinite(angle) || !isfinite(aspect) || aspect == 0.0f) return false; // (aspect 0 would take the window's in the constructor)
	if (!view_make(pos, light_dir, up_dir, angle, aspect, max_std(near_clip, dist - radius), max_std(near_clip, dist) + radius, o)) return false;
	behind_sphere_mult = view_behind_sphere_mult(angle, aspect);
	return view_finite(o) && isfinite(behind_sphere_mult);
}

} // namespace terra
