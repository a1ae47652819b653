// terra_terrainview.hpp -- the terrain draw list of a tile batch for a camera: the head of tile_draw_t::draw (src/tiled_mesh.cpp:2844-2915) with
// occluder_cubes_t's constructor (:2834-2842) and calc_cube_top_points (:2823-2832), tile_t::get_lod_level (:1910-1932), the crack look-ups of tile_t::draw
// (:2059-2074) with crack_ibuf_t::get_index (:2020-2023), tile_t::use_as_occluder (:3801-3803), get_bsphere_radius_inc_water (:366-368), get_center / get_bcube /
// get_mesh_sub_bcube / get_sub_bcube / get_rel_dist_to_camera / rel_dist_to_camera_xy_lt / is_visible (src/tiled_mesh.h:229-252,320-332), the constants
// (src/tiled_mesh.cpp:23,33; src/tiled_mesh.h:24-25,32,93-94), cube_t::get_cube_center (src/3DWorld.h:602-604), dist_xy_less_than / p2p_dist_xy
// (src/inlines.h:183-195) and check_line_clip (src/inlines.h:509-512) = get_line_clip (src/Math3d.cpp:1037-1052).
//
// The bodies are shared by the driver's simple form (one logical thread per tile, the reference's loops) and by the k_terrain_view_* kernels
// (terra_kernels.hpp).  The sphere and cube tests and behind_sphere_mult are terra_view.hpp's, the line clip terra_common.hpp's shadow_line_clip.  Every operand
// carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out; sums run in the reference's order (the library is built
// without contraction).
//
// The occlusion loops' early exits (`&& !intersected`, `&& !sub_tile_occluded`, `&& sub_tile_occluded`, the `break` of :2904) only shortcut booleans: the result of
// a tile is "for every sub-box t there is an occluder o, not the tile itself, with any of the tile's four top points clipped by o's mesh box, the sub-box's centre
// clipped by it, and a column s of o that is not zeroed and clips all four top points of the sub-box".  It does not depend on the order of the occluders.
#pragma once
#include "terra_view.hpp"
#include "terra_stage.hpp"
#include "../../include/terra.h"
#include <stdexcept>
#include <string>

namespace terra {

constexpr uint32_t TERRAIN_VIEW_LODS = 5;          // NUM_LODS (src/tiled_mesh.h:25)
constexpr uint8_t  TERRAIN_VIEW_NO_CRACK = 255;    // no present neighbour, or the tile is not drawn
enum {TV_ABSENT = 0, TV_TOO_FAR = 1, TV_NOT_VISIBLE = 2, TV_OCCLUDED_BEFORE = 3, TV_OCCLUDED = 4, TV_DRAWN = 5, TV_STATUS_MASK = 7, TV_WAS_OCCLUDER = 0x80}; // status
enum {TV_FLAG_ABSENT = 1, TV_FLAG_NO_OCCLUDER = 2, TV_FLAG_SHADOW_MAPS = 4};                                                                                 // flags
enum {TV_STATE_NONE = 0, TV_STATE_OCCLUDED = 1, TV_STATE_UNOCCLUDED = 2};                                                                                    // occl_state

struct terrain_view_args_pod_t {float behind_sphere_mult, occluder_zmin; int32_t water_enabled, check_occlusion, reflection_pass;}; // terra_terrain_view_args

struct terrain_view_consts_t {
	view_pod_t v;
	float behind_sphere_mult;
	float xss, yss, DX_VAL, DY_VAL;
	int S, dxoff, dyoff;
	float scaled_tile_radius;            // get_scaled_tile_radius() (src/tiled_mesh.h:94)
	float water_plane_z, occluder_zmin;
	int water_enabled, check_occlusion, reflection_pass;
};
inline terrain_view_consts_t terrain_view_consts(view_pod_t const &v, terrain_view_args_pod_t const &a, float xss, float yss, float DX_VAL, float DY_VAL, int S, int dxoff,
	int dyoff, float water_plane_z)
{
	terrain_view_consts_t c;
	c.v = v; c.behind_sphere_mult = a.behind_sphere_mult; c.xss = xss; c.yss = yss; c.DX_VAL = DX_VAL; c.DY_VAL = DY_VAL; c.S = S; c.dxoff = dxoff; c.dyoff = dyoff;
	int const TILE_RADIUS = 6;                           // src/tiled_mesh.h:24
	c.scaled_tile_radius = (float)TILE_RADIUS*(xss + yss); // TILE_RADIUS*get_tile_width()
	c.water_plane_z = water_plane_z; c.occluder_zmin = a.occluder_zmin;
	c.water_enabled = a.water_enabled ? 1 : 0; c.check_occlusion = a.check_occlusion ? 1 : 0; c.reflection_pass = a.reflection_pass;
	return c;
}
// ---- log2 of a positive normal double in plain double arithmetic, the same on the host and on the device (get_lod_level divides by -log2(2.0*min_normal_z),
// :1924, and the device library's log2 is not the C library's).  x = 2^e*m with m in (sqrt(1/2), sqrt(2)]; f = m - 1, s = f/(2 + f), z = s*s;
// log(m) = 2*atanh(s) = f - hfsq + s*(hfsq + R), hfsq = f*f/2, R = z*(2/3 + z*(2/5 + ...)) (z <= 0.0295: twelve terms reach below 2^-60); the head f - hfsq is
// split so that its product with the head of 1/ln 2 is exact, and e is added last with its rounding error carried.
TERRA_HD double terrain_view_log2(double x) {
	uint64_t u; memcpy(&u, &x, 8);
	int e = (int)(u >> 52) - 1023;
	u = (u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
	double m; memcpy(&m, &u, 8);
	if (m > 1.4142135623730951) {m *= 0.5; ++e;}
	double const f = m - 1.0, s = f/(2.0 + f), z = s*s, hfsq = 0.5*f*f;
	double r = 2.0/25.0;
	r = 2.0/23.0 + z*r; r = 2.0/21.0 + z*r; r = 2.0/19.0 + z*r; r = 2.0/17.0 + z*r; r = 2.0/15.0 + z*r; r = 2.0/13.0 + z*r; r = 2.0/11.0 + z*r;
	r = 2.0/9.0 + z*r; r = 2.0/7.0 + z*r; r = 2.0/5.0 + z*r; r = 2.0/3.0 + z*r;
	double const R = z*r;
	double hi = f - hfsq;
	uint64_t h; memcpy(&h, &hi, 8); h &= 0xFFFFFFFFF8000000ull; memcpy(&hi, &h, 8);
	double const lo = ((f - hi) - hfsq) + s*(hfsq + R);
	double const ivln2hi = 0x1.715476p+0, ivln2lo = 0x1.4ae0bf85ddf44p-26; // 1/ln 2 = ivln2hi + ivln2lo, ivln2hi of 26 bits
	double const val_hi = hi*ivln2hi;
	double val_lo = (lo + hi)*ivln2lo + lo*ivln2hi;
	double const y = (double)e, w = y + val_hi;
	val_lo += (y - w) + val_hi;
	return val_lo + w;
}
// the steep-slope statement of get_lod_level (:1924): dist /= -log2(2.0*min_normal_z)
TERRA_HD float terrain_view_steep_dist(float dist, float min_normal_z) {return (float)((double)dist/-terrain_view_log2(2.0*(double)min_normal_z));}

// ---- a tile's boxes and centre
struct terrain_view_geom_t {
	float cx, cy, cz;          // get_center()
	float xv1, yv1, xv2, yv2;  // the mesh box's corners: get_xval(x1 + xoff - xoff2), xv1 + (x2 - x1)*DX_VAL
	float bc[3][2];            // get_bcube()
	float zadd;                // get_tile_zmax() - mzmax (get_sub_bcube)
};
TERRA_HD terrain_view_geom_t terrain_view_geom(terrain_view_consts_t const &c, int tx, int ty, float mzmin, float mzmax, float trmax, float tile_zmax) {
	terrain_view_geom_t g;
	float const BCUBE_ZTOLER = 1.0E-6f;
	int const x1 = (int)((uint32_t)tx*(uint32_t)c.S), y1 = (int)((uint32_t)ty*(uint32_t)c.S); // integer steps wrap as in the reference binary
	int const mx = (int)((uint32_t)x1 + (uint32_t)x1 + (uint32_t)c.S) >> 1, my = (int)((uint32_t)y1 + (uint32_t)y1 + (uint32_t)c.S) >> 1;
	g.cx = -c.xss + c.DX_VAL*(float)(int)((uint32_t)mx + (uint32_t)c.dxoff); g.cy = -c.yss + c.DY_VAL*(float)(int)((uint32_t)my + (uint32_t)c.dyoff);
	g.cz = 0.5f*(mzmin + mzmax);
	g.xv1 = -c.xss + c.DX_VAL*(float)(int)((uint32_t)x1 + (uint32_t)c.dxoff); g.yv1 = -c.yss + c.DY_VAL*(float)(int)((uint32_t)y1 + (uint32_t)c.dyoff);
	g.xv2 = g.xv1 + (float)c.S*c.DX_VAL; g.yv2 = g.yv1 + (float)c.S*c.DY_VAL;
	g.bc[0][0] = g.xv1 - trmax; g.bc[0][1] = g.xv2 + trmax; g.bc[1][0] = g.yv1 - trmax; g.bc[1][1] = g.yv2 + trmax;
	g.bc[2][0] = mzmin - BCUBE_ZTOLER; g.bc[2][1] = max_std(tile_zmax + BCUBE_ZTOLER, c.water_plane_z);
	g.zadd = tile_zmax - mzmax;
	return g;
}
// get_mesh_bcube()
TERRA_HD void terrain_view_mesh_box(terrain_view_geom_t const &g, float mzmin, float mzmax, float d[3][2]) {
	d[0][0] = g.xv1; d[0][1] = g.xv2; d[1][0] = g.yv1; d[1][1] = g.yv2; d[2][0] = mzmin - 1.0E-6f; d[2][1] = mzmax + 1.0E-6f;
}
// get_mesh_sub_bcube(x, y): sub_zmin[y][x]
TERRA_HD void terrain_view_mesh_sub_box(terrain_view_geom_t const &g, terra_tile_stats const &st, uint32_t x, uint32_t y, float d[3][2]) {
	float const dx = (g.xv2 - g.xv1)/(float)4, dy = (g.yv2 - g.yv1)/(float)4;
	d[0][0] = g.xv1 + (float)x*dx; d[0][1] = g.xv1 + (float)(x + 1u)*dx; d[1][0] = g.yv1 + (float)y*dy; d[1][1] = g.yv1 + (float)(y + 1u)*dy;
	d[2][0] = st.sub_zmin[4u*y + x]; d[2][1] = st.sub_zmax[4u*y + x];
}
// get_rel_dist_to_camera(xy_dist = 1)
TERRA_HD float terrain_view_rel_dist_xy(terrain_view_consts_t const &c, terrain_view_geom_t const &g, float radius) {
	float const *cam = c.v.pos;
	float const d = sqrtf((cam[0] - g.cx)*(cam[0] - g.cx) + (cam[1] - g.cy)*(cam[1] - g.cy));
	return max_std(0.0f, d - radius)/c.scaled_tile_radius;
}
// get_dist_to_camera_in_tiles(xy_dist = 0)
TERRA_HD float terrain_view_dist_in_tiles(terrain_view_consts_t const &c, terrain_view_geom_t const &g, float radius) {
	float const *cam = c.v.pos;
	float const d = sqrtf((cam[0] - g.cx)*(cam[0] - g.cx) + (cam[1] - g.cy)*(cam[1] - g.cy) + (cam[2] - g.cz)*(cam[2] - g.cz));
	return (max_std(0.0f, d - radius)/c.scaled_tile_radius)*(float)6;
}
// get_bsphere_radius_inc_water() (src/tiled_mesh.cpp:366-368)
TERRA_HD float terrain_view_radius_inc_water(terrain_view_consts_t const &c, float mzmin, float mzmax, float radius) {
	return (c.water_enabled && mzmax < c.water_plane_z) ? max_std(radius, c.water_plane_z - 0.5f*(mzmin + mzmax)) : radius;
}
// tile_t::is_visible(): sphere_and_cube_visible_test(get_center(), get_bsphere_radius_inc_water(), get_bcube())
TERRA_HD bool terrain_view_visible(terrain_view_consts_t const &c, terrain_view_geom_t const &g, float mzmin, float mzmax, float radius) {
	float const r = terrain_view_radius_inc_water(c, mzmin, mzmax, radius);
	return view_sphere_and_cube_visible(c.v, c.behind_sphere_mult, g.cx, g.cy, g.cz, r, g.bc);
}
// rel_dist_to_camera_xy_lt(OCCLUDER_DIST): the distance half of use_as_occluder()
TERRA_HD bool terrain_view_occluder_dist(terrain_view_consts_t const &c, terrain_view_geom_t const &g, float radius) {
	float const *cam = c.v.pos;
	float const OCCLUDER_DIST = 0.2f, dval = OCCLUDER_DIST*c.scaled_tile_radius + radius;
	return (cam[0] - g.cx)*(cam[0] - g.cx) + (cam[1] - g.cy)*(cam[1] - g.cy) < dval*dval;
}
// tile_t::get_lod_level(reflection_pass): in_tiles = get_dist_to_camera_in_tiles(0); low_detail (:1913) holds in pass 1 only
TERRA_HD uint32_t terrain_view_lod(terrain_view_consts_t const &c, float mzmin, float mzmax, float min_normal_z, float in_tiles, bool shadow_maps) {
	if (mzmax == mzmin) return TERRAIN_VIEW_LODS - 1u; // flat, use lowest LOD
	bool const low_detail = c.reflection_pass == 1 && (double)min_normal_z > 0.1;
	uint32_t lod_level = low_detail ? 1u : 0u; // min(NUM_LODS-1, 1U)
	float dist = in_tiles;
	if (shadow_maps) {dist /= (float)2;}
	if (min_normal_z > 0.0f) {
		if ((double)min_normal_z > 0.9) {
			if (!c.water_enabled || mzmax < c.water_plane_z || mzmin > c.water_plane_z) {dist = (float)((double)dist*(((double)min_normal_z > 0.95) ? 4.0 : 2.0));}
		}
		else if ((double)min_normal_z < 0.25) {dist = terrain_view_steep_dist(dist, min_normal_z);}
	}
	double const thresh = c.reflection_pass ? 1.8 : 2.0;
	while ((double)dist > thresh && lod_level + 1u < TERRAIN_VIEW_LODS && ((uint32_t)c.S >> (lod_level + 1u)) >= 4u) {
		dist /= (float)2;
		++lod_level;
	}
	return lod_level;
}
// crack_ibuf_t::get_index
TERRA_HD uint32_t terrain_view_crack_index(uint32_t dim, uint32_t dir, uint32_t cur_lod, uint32_t adj_lod) {
	return TERRAIN_VIEW_LODS*(TERRAIN_VIEW_LODS*(2u*dim + dir) + cur_lod) + adj_lod;
}
// the slot of get_adj_tile(dx, dy) in the [n][9] neighbour table ((dy + 1)*3 + dx + 1) for the crack loop's (dim, dir) (:2063-2067)
TERRA_HD uint32_t terrain_view_nbr_slot(uint32_t dim, uint32_t dir) {return dim ? (dir ? 7u : 1u) : (dir ? 5u : 3u);}

// ---- what the first pass leaves of a tile: everything but the occlusion test, the cracks and the lists
struct terrain_view_tile_t {float dist; uint8_t status, lod, occluder, test, visible;}; // status: TV_ABSENT .. TV_OCCLUDED_BEFORE, or TV_DRAWN for a candidate; test: the loop of :2872 runs (if there are occluders)
struct terrain_view_in_t { // the per-tile arrays
	terra_tile_stats const *stats; float const *min_normal_z, *trmax, *tile_zmax; uint8_t const *flags; uint8_t *occl_state;
};
TERRA_HD terrain_view_geom_t terrain_view_geom_of(terrain_view_consts_t const &c, terrain_view_in_t const &in, int32_t const *tile_xy, size_t t) {
	terra_tile_stats const &st = in.stats[t];
	return terrain_view_geom(c, tile_xy[2*t], tile_xy[2*t + 1], st.mzmin, st.mzmax, in.trmax ? in.trmax[t] : 0.0f, in.tile_zmax ? in.tile_zmax[t] : st.mzmax);
}
TERRA_HD terrain_view_tile_t terrain_view_tile(terrain_view_consts_t const &c, terrain_view_in_t const &in, int32_t const *tile_xy, size_t t) {
	terrain_view_tile_t o;
	o.dist = 0.0f; o.status = TV_ABSENT; o.lod = 0; o.occluder = 0; o.test = 0; o.visible = 0;
	uint32_t const fl = in.flags ? in.flags[t] : 0u;
	if (fl & TV_FLAG_ABSENT) return o;
	terra_tile_stats const &st = in.stats[t];
	terrain_view_geom_t const g = terrain_view_geom_of(c, in, tile_xy, t);
	float const DRAW_DIST_TILES = 1.5f;
	o.dist = terrain_view_rel_dist_xy(c, g, st.radius);
	o.lod = (uint8_t)terrain_view_lod(c, st.mzmin, st.mzmax, in.min_normal_z ? in.min_normal_z[t] : 0.0f, terrain_view_dist_in_tiles(c, g, st.radius), (fl & TV_FLAG_SHADOW_MAPS) != 0);
	bool const visible = terrain_view_visible(c, g, st.mzmin, st.mzmax, st.radius);
	o.visible = visible ? 1 : 0;
	o.occluder = (c.check_occlusion && !(fl & TV_FLAG_NO_OCCLUDER) && terrain_view_occluder_dist(c, g, st.radius) && visible) ? 1 : 0; // use_as_occluder() (:2857-2860)
	uint32_t const state = in.occl_state ? in.occl_state[t] : (uint32_t)TV_STATE_NONE;
	if (o.dist > DRAW_DIST_TILES) {o.status = TV_TOO_FAR;}
	else if (!visible) {o.status = TV_NOT_VISIBLE;}
	else if (state == TV_STATE_OCCLUDED) {o.status = TV_OCCLUDED_BEFORE;} // was_last_occluded() (:2868)
	else {o.status = TV_DRAWN; o.test = (state != TV_STATE_UNOCCLUDED) ? 1 : 0;} // !was_last_unoccluded() (:2872)
	return o;
}

// ---- an occluder: occluder_cubes_t
struct alignas(16) terrain_view_occluder_t {float bc[3][2]; float sub[16][3][2]; int32_t tile, pad;};
static_assert(sizeof(terrain_view_occluder_t) == 416, "terrain_view_occluder_t: 26 16-byte loads");
// column s of the occluder: get_mesh_sub_bcube(s >> 2, s & 3), zeroed where cube_visible fails, else the column from occluder_zmin up to sub_zmin (:2837-2840)
TERRA_HD void terrain_view_occluder_column(terrain_view_consts_t const &c, terrain_view_geom_t const &g, terra_tile_stats const &st, uint32_t s, float d[3][2]) {
	terrain_view_mesh_sub_box(g, st, s >> 2, s & 3u, d);
	if (!view_cube_visible(c.v, d)) {for (int i = 0; i < 3; ++i) {d[i][0] = 0.0f; d[i][1] = 0.0f;} return;}
	d[2][1] = d[2][0]; // cube below the bcube
	d[2][0] = c.occluder_zmin;
}
TERRA_HD bool terrain_view_all_zeros(float const d[3][2]) {return d[0][0] == 0.0f && d[0][1] == 0.0f && d[1][0] == 0.0f && d[1][1] == 0.0f && d[2][0] == 0.0f && d[2][1] == 0.0f;}
// check_line_clip(p, camera, d)
TERRA_HD bool terrain_view_clip(terrain_view_consts_t const &c, float px, float py, float pz, float const d[3][2]) {
	shadow_pt_t v1 = {px, py, pz}, v2 = {c.v.pos[0], c.v.pos[1], c.v.pos[2]};
	return shadow_line_clip(v1, v2, d);
}
// calc_cube_top_points: cube_pts[(i0 << 1) + i1] = (d[0][i0], d[1][i1], d[2][1]); any / all of the four against a box
TERRA_HD bool terrain_view_top_any(terrain_view_consts_t const &c, float const b[3][2], float const d[3][2]) {
	bool r = false;
	for (int k = 0; k < 4; ++k) {r = r || terrain_view_clip(c, b[0][k >> 1], b[1][k & 1], b[2][1], d);}
	return r;
}
TERRA_HD bool terrain_view_top_all(terrain_view_consts_t const &c, float const b[3][2], float const d[3][2]) {
	bool r = true;
	for (int k = 0; k < 4; ++k) {r = r && terrain_view_clip(c, b[0][k >> 1], b[1][k & 1], b[2][1], d);}
	return r;
}
// get_sub_bcube(t >> 2, t & 3)
TERRA_HD void terrain_view_sub_box(terrain_view_geom_t const &g, terra_tile_stats const &st, uint32_t t, float d[3][2]) {
	terrain_view_mesh_sub_box(g, st, t >> 2, t & 3u, d);
	d[2][1] += g.zadd;
}
// does occluder o's column s hide sub-box b (centre cx, cy, cz) of a tile that o's mesh box intersects?  (:2892-2901 for one s)
TERRA_HD bool terrain_view_column_hides(terrain_view_consts_t const &c, terrain_view_occluder_t const &o, uint32_t s, float const b[3][2], float cx, float cy, float cz) {
	if (!terrain_view_clip(c, cx, cy, cz, o.bc)) return false; // if not occluded by the full tile, then won't be occluded by a sub-cube of it
	if (terrain_view_all_zeros(o.sub[s])) return false;          // invalid cube, skip
	return terrain_view_top_all(c, b, o.sub[s]);
}
// the loop of :2873-2905 for tile t: true = occluded
TERRA_HD bool terrain_view_occluded(terrain_view_consts_t const &c, terrain_view_geom_t const &g, terra_tile_stats const &st, terrain_view_occluder_t const *occ, uint32_t nocc,
	int32_t t)
{
	for (uint32_t q = 0; q < 16; ++q) {
		float b[3][2];
		terrain_view_sub_box(g, st, q, b);
		float const cx = 0.5f*(b[0][0] + b[0][1]), cy = 0.5f*(b[1][0] + b[1][1]), cz = 0.5f*(b[2][0] + b[2][1]); // get_cube_center()
		bool hidden = false;
		for (uint32_t j = 0; j < nocc && !hidden; ++j) {
			terrain_view_occluder_t const &o = occ[j];
			if (o.tile == t) continue;                      // no self-occlusion
			if (!terrain_view_top_any(c, g.bc, o.bc)) continue; // not in occluder_ixs
			for (uint32_t s = 0; s < 16 && !hidden; ++s) {hidden = terrain_view_column_hides(c, o, s, b, cx, cy, cz);}
		}
		if (!hidden) return false;
	}
	return true;
}
// std::pair<float, tile_t *>'s operator< with the batch index in the pointer's place
TERRA_HD bool terrain_view_before(float da, uint32_t ia, float db, uint32_t ib) {return da < db || (!(db < da) && ia < ib);}

TERRA_HD bool terrain_view_args_finite(terrain_view_args_pod_t const &a) {return isfinite(a.behind_sphere_mult) && isfinite(a.occluder_zmin);}

// ---- the arrays of a call, in the order of terra_tiles_terrain_view[_dev] and terra_tiles_reflection_view[_dev] (reflect: the reflection view's, null in the terrain view)
struct terrain_view_io_t {terrain_view_in_t in; uint8_t *status; float *dist; uint8_t *lod, *crack; uint32_t *draw_order, *occluded, *counts; uint8_t *not_drawn, *reflect;};
// the argument rules of both views, behind their checks that need no array: throws what the call refuses; false: nothing to do (n == 0).  what: the pass's name; dev: the arrays are the device's
inline bool terrain_view_io_check(char const *what, int32_t const *tile_xy, uint32_t n, terrain_view_io_t const &io, bool dev) {
	if (n == 0) return false;
	if (!tile_xy || !io.in.stats || !io.status || !io.dist || !io.lod || !io.crack || !io.draw_order || !io.occluded || !io.counts) throw std::invalid_argument(std::string(what) + ": null argument");
	if (dev && (((uintptr_t)io.in.stats | (uintptr_t)io.in.min_normal_z | (uintptr_t)io.in.trmax | (uintptr_t)io.in.tile_zmax | (uintptr_t)io.dist | (uintptr_t)io.draw_order | (uintptr_t)io.occluded |
	             (uintptr_t)io.counts) & 3u) != 0) throw std::invalid_argument(std::string(what) + ": d_stats, d_min_normal_z, d_trmax, d_tile_zmax, d_dist, d_draw_order, d_occluded and d_counts must be 4-byte aligned");
	return true;
}
// ---- the scratch of both views: the coordinates and the neighbour table, the occluders of the batch in batch order with their count, the candidates that run the occlusion
// test, and the (dist, batch index) keys of the drawn tiles in batch order for the order's second path.  The reflection view's alone, null in the terrain view: the constants for
// k_reflect_walk, per tile what the walk reads of it, the marks of the walk (the start tile's index + 1), its work list, the provisional result of the occlusion test, the answer of :2869, last_occluded as the loop goes
struct reflect_consts_t; struct reflect_tile_t;
struct terrain_view_scratch_t {
	int32_t *txy, *nbr; terrain_view_occluder_t *occ; uint32_t *nocc, *key_tile; uint8_t *test; float *keys;
	reflect_consts_t *rc; reflect_tile_t *rt; uint32_t *mark; int32_t *work; uint8_t *prov, *refl, *state;
};
inline void terrain_view_scratch_add(stage_layout_t &lay, terrain_view_scratch_t &s, uint32_t n) {lay.add(s.occ, n); lay.add(s.txy, (size_t)n*2); lay.add(s.nbr, (size_t)n*9); lay.add(s.nocc, 4); lay.add(s.keys, n); lay.add(s.key_tile, n); lay.add(s.test, n);}
// ---- the literal bodies of the simple form.  (1) a logical thread per tile: everything but the occlusion test, the cracks and the lists
TERRA_HD terrain_view_tile_t terrain_view_tile_literal(terrain_view_consts_t const &c, terrain_view_io_t const &io, terrain_view_scratch_t const &s, size_t t) {
	terrain_view_tile_t const o = terrain_view_tile(c, io.in, s.txy, t);
	io.status[t] = (uint8_t)(o.status | (o.occluder ? TV_WAS_OCCLUDER : 0)); io.dist[t] = o.dist; io.lod[t] = o.lod; s.test[t] = o.test;
	return o;
}
// (2) one thread: the occluders in batch order, as the loop of :2858-2861 leaves them; -> their number
TERRA_HD uint32_t terrain_view_occluders_literal(terrain_view_consts_t const &c, terrain_view_io_t const &io, terrain_view_scratch_t const &s, uint32_t n) {
	uint32_t m = 0;
	for (uint32_t t = 0; t < n; ++t) {
		if (!(io.status[t] & TV_WAS_OCCLUDER)) continue;
		terrain_view_geom_t const g = terrain_view_geom_of(c, io.in, s.txy, t);
		terrain_view_occluder_t &o = s.occ[m++];
		terrain_view_mesh_box(g, io.in.stats[t].mzmin, io.in.stats[t].mzmax, o.bc);
		for (uint32_t q = 0; q < 16; ++q) {terrain_view_occluder_column(c, g, io.in.stats[t], q, o.sub[q]);}
		o.tile = (int32_t)t; o.pad = 0;
	}
	return *s.nocc = m;
}
// (3) a thread per tile: the loop of :2872-2908
TERRA_HD void terrain_view_occlusion_literal(terrain_view_consts_t const &c, terrain_view_io_t const &io, terrain_view_scratch_t const &s, size_t t) {
	uint32_t const nocc = *s.nocc;
	if ((io.status[t] & TV_STATUS_MASK) != TV_DRAWN || !s.test[t] || nocc == 0) return;
	bool const occluded = terrain_view_occluded(c, terrain_view_geom_of(c, io.in, s.txy, t), io.in.stats[t], s.occ, nocc, (int32_t)t);
	if (occluded) {io.status[t] = (uint8_t)((io.status[t] & ~TV_STATUS_MASK) | TV_OCCLUDED);}
	if (io.in.occl_state) {io.in.occl_state[t] = occluded ? TV_STATE_OCCLUDED : TV_STATE_UNOCCLUDED;} // set_last_occluded (:2906)
}
// the last step of both views, a thread per tile: its cracks, and its place in its list -- the rank of (dist, batch index) among the drawn tiles is where the sort of :2915 puts it
TERRA_HD void terrain_view_lists_literal(terrain_view_io_t const &io, terrain_view_scratch_t const &s, uint32_t n, size_t t) {
	uint32_t const me = io.status[t] & TV_STATUS_MASK;
	for (uint32_t k = 0; k < 4; ++k) {
		int32_t const u = s.nbr[t*9 + terrain_view_nbr_slot(k >> 1, k & 1u)];
		bool const adj = me == TV_DRAWN && u >= 0 && (io.status[u] & TV_STATUS_MASK) != TV_ABSENT;
		io.crack[t*4 + k] = adj ? (uint8_t)terrain_view_crack_index(k >> 1, k & 1u, io.lod[t], io.lod[u]) : TERRAIN_VIEW_NO_CRACK;
	}
	if (io.not_drawn) {io.not_drawn[t] = (me != TV_DRAWN) ? 1 : 0;}
	if (me == TV_DRAWN) {
		uint32_t rank = 0;
		for (uint32_t u = 0; u < n; ++u) {rank += ((io.status[u] & TV_STATUS_MASK) == TV_DRAWN && terrain_view_before(io.dist[u], u, io.dist[t], (uint32_t)t)) ? 1u : 0u;}
		io.draw_order[rank] = (uint32_t)t;
	}
	else if (me == TV_OCCLUDED) {
		uint32_t rank = 0;
		for (uint32_t u = 0; u < t; ++u) {rank += ((io.status[u] & TV_STATUS_MASK) == TV_OCCLUDED) ? 1u : 0u;}
		io.occluded[rank] = (uint32_t)t;
	}
	if (t == 0) {
		uint32_t nd = 0, no = 0;
		for (uint32_t u = 0; u < n; ++u) {uint32_t const su = io.status[u] & TV_STATUS_MASK; nd += (su == TV_DRAWN) ? 1u : 0u; no += (su == TV_OCCLUDED) ? 1u : 0u;}
		io.counts[0] = nd; io.counts[1] = no;
	}
}

} // namespace terra
