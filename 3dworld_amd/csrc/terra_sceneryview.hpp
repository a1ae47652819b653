// terra_sceneryview.hpp -- the scenery draw lists of a tile batch for a camera: tile_t::draw_scenery (src/tiled_mesh.cpp:1580-1592) without its GL, shader and colour
// calls, scenery_group::draw_opaque_objects and draw_plant_leaves (src/scenery.cpp:1413-1500), the per-object rock_shape3d::draw (:300-305), surface_rock::draw
// (:394-417), s_rock::draw (:442-461), voxel_rock::draw (:517-530), s_log::draw (:606-632), s_stump::draw (:670-693), s_plant::draw_stem / draw_leaves / draw_berries
// (:853-871, 898-934), leafy_plant::draw_leaves (:1030-1045) and mushroom::draw (:1062-1081), scenery_obj::check_visible / is_visible / get_size_scale (:122-135,
// scale_exp = 8.0, src/shape_line3d.h:22), skip_uw_draw and get_pt_line_thresh (:61-74), the get_bsphere_radius() overrides (src/scenery.h:120,132,166,199,221),
// get_scenery_thresh / get_scenery_dist_scale (src/tiled_mesh.h:333-334), get_tile_width (:93), get_smap_ndiv (src/shadow_map.cpp:60-64), distance_to_camera
// (src/inlines.h:431) and dot_product_ptv (:227).  The records are terra_sceneryplace.hpp's, the tile's centre and get_dist_to_camera_in_tiles(0)
// terra_terrainview.hpp's (terrain_view_geom, terrain_view_dist_in_tiles), the sphere test terra_view.hpp's, int(double) and int(float) terra_common.hpp's.
//
// In tiled-terrain mode check_visible is camera_pdu.sphere_visible_test alone, in the shadow pass too, and sphere_in_camera_view(.., 2) (draw_berries) is the same
// test (src/visibility.cpp:338-339).  next_frame, burn_amt, is_shadowed and the colours stay with the engine.
//
// The bodies are shared by the driver's simple form (one logical thread per tile) and by k_scenery_view (terra_kernels.hpp).  Every operand carries the type the
// reference statement gives it; where the C++ source promotes to double the promotion is written out; sums run in the reference's order.
#pragma once
#include "terra_view.hpp"
#include "terra_terrainview.hpp"
#include "terra_sceneryplace.hpp"
#include "terra_powf.hpp"
#include "terra_landscape.hpp" // min_u32
#include <stdexcept>

namespace terra {

constexpr uint32_t SCV_GROUPS = 13;   // the lists of a tile, in the order in which the reference issues them (TERRA_SCV_GROUPS)
constexpr uint32_t SCV_STREAMS = 16;  // the same with the pld groups split by kind: points = surface rocks, rocks; lines = logs, stumps, stems
enum {SCV_NONE = 0, SCV_POINT = 1, SCV_LINE = 2, SCV_POLY = 3, SCV_ENGINE = 7, SCV_FORM_MASK = 7,                 // bits 0-2 of a draw word
      SCV_LOG_END = 0x8, SCV_LOG_END2 = 0x10, SCV_STUMP_TOP = 0x20, SCV_CAP_UNDERSIDE = 0x40, SCV_LEAVES = 0x80, // :623-630, :687, :1077, draw_leaves
      SCV_NDIV_SHIFT = 8, SCV_UNDERWATER = 0x4000, SCV_BERRIES = 0x8000, SCV_BERRY_NDIV_SHIFT = 16};             // ndiv: 6 bits each
enum {SCV_TILE_DRAWN = 1, SCV_TILE_OPAQUE = 2, SCV_TILE_LEAVES = 4};                                            // the flags word of a tile record
enum {SCV_G_ROCK_SHAPE = 0, SCV_G_SURFACE_ROCK, SCV_G_ROCK, SCV_G_LOG, SCV_G_STUMP, SCV_G_MUSHROOM, SCV_G_STEM, SCV_G_BERRIES, SCV_G_VOXEL_ROCK, SCV_G_PLANT_LEAVES,
      SCV_G_LEAFY_LEAVES, SCV_G_PLD_POINTS, SCV_G_PLD_LINES};                                                   // TERRA_SCV_G_*

struct scenery_view_args_pod_t {float behind_sphere_mult, zoom_f, smap_pixel_width; int32_t window_width, shadow_pass, reflection_pass, uw_skip, skip_small_shadow_objs,
	draw_opaque, draw_leaves;};                                                                                  // terra_scenery_view_args
struct scenery_view_tile_pod_t {float dist_scale, scale_val; uint32_t flags, num_records, list_written, pad[3];}; // terra_scenery_view_tile

struct scenery_view_consts_t {
	terrain_view_consts_t tv;      // the view, behind_sphere_mult, the scene, the offsets and water_plane_z: what the tile's centre reads
	float offx, offy;              // xlate = scenery_off.get_xlate()
	float tree_scale, min_water_plane_z;
	float thresh;                  // get_scenery_thresh(reflection_pass)
	float scale_val;               // thresh*get_tile_width() (src/tiled_mesh.cpp:1587)
	float pt_thresh;               // get_pt_line_thresh()
	float sscale;                  // int((do_zoom ? ZOOM_FACTOR : 1.0)*window_width) as the float parameter of every draw()
	float smap_pw;                 // approx_pixel_width(shadow_map_sz)
	int shadow, reflection, uw_skip, wood, opaque, leaves; // wood: the gate of :1471
	uint32_t cap, list_cap;
};
inline scenery_view_consts_t scenery_view_consts(view_pod_t const &v, scenery_view_args_pod_t const &a, float xss, float yss, float dxv, float dyv, int S, int dxoff, int dyoff,
	float offx, float offy, float water_plane_z, float min_water_plane_z, float tree_scale, uint32_t cap, uint32_t list_cap)
{
	scenery_view_consts_t c;
	terrain_view_args_pod_t const ta = {a.behind_sphere_mult, 0.0f, 0, 0, 0};
	c.tv = terrain_view_consts(v, ta, xss, yss, dxv, dyv, S, dxoff, dyoff, water_plane_z);
	c.offx = offx; c.offy = offy; c.tree_scale = tree_scale; c.min_water_plane_z = min_water_plane_z;
	float const SCENERY_THRESH_REF = 2.0f, SCENERY_THRESH = 5.0f, PT_LINE_THRESH = 800.0f; // src/tiled_mesh.h:30-31; src/scenery.cpp:22
	c.thresh = a.reflection_pass ? SCENERY_THRESH_REF : SCENERY_THRESH;
	c.scale_val = c.thresh*(xss + yss);
	c.pt_thresh = (float)((double)PT_LINE_THRESH*(double)a.zoom_f);                         // PT_LINE_THRESH*(do_zoom ? ZOOM_FACTOR : 1.0)
	c.sscale = (float)d2i_x86((double)a.zoom_f*(double)a.window_width);
	c.smap_pw = a.smap_pixel_width;
	c.shadow = a.shadow_pass ? 1 : 0; c.reflection = a.reflection_pass; c.uw_skip = a.uw_skip ? 1 : 0;
	c.wood = (!c.shadow || !a.skip_small_shadow_objs) ? 1 : 0;
	c.opaque = a.draw_opaque ? 1 : 0; c.leaves = a.draw_leaves ? 1 : 0;
	c.cap = cap; c.list_cap = list_cap;
	return c;
}
TERRA_HD bool scenery_view_args_finite(scenery_view_args_pod_t const &a) {return isfinite(a.behind_sphere_mult) && isfinite(a.zoom_f) && isfinite(a.smap_pixel_width);}
TERRA_HD bool scenery_view_args_ok(scenery_view_args_pod_t const &a) {return a.zoom_f > 0.0f && a.window_width > 0 && (!a.shadow_pass || a.smap_pixel_width > 0.0f);}

// ---- the tile: get_scenery_dist_scale(reflection_pass) and whether the tile draws (:1582)
TERRA_HD bool scenery_view_tile(scenery_view_consts_t const &c, int tx, int ty, float mzmin, float mzmax, float radius, float &dist_scale) {
	terrain_view_geom_t const g = terrain_view_geom(c.tv, tx, ty, mzmin, mzmax, 0.0f, mzmax);
	dist_scale = c.tree_scale*terrain_view_dist_in_tiles(c.tv, g, radius)/c.thresh;
	return !((double)dist_scale > 1.0);
}
TERRA_HD uint32_t scenery_view_tile_flags(scenery_view_consts_t const &c) {return SCV_TILE_DRAWN | (c.opaque ? SCV_TILE_OPAQUE : 0u) | (c.leaves ? SCV_TILE_LEAVES : 0u);}

// ---- what the per-object methods share
TERRA_HD float scv_max(float a, float b) {return (a < b) ? b : a;} // std::max
TERRA_HD int scv_clamp(int lo, int hi, int v) {int const m = (v < hi) ? v : hi; return (lo < m) ? m : lo;} // max(lo, min(hi, v))
// check_visible(shadow_only, bradius, p)
TERRA_HD bool scv_check_visible(scenery_view_consts_t const &c, float bradius, float radius, float x, float y, float z) {
	return view_sphere_visible(c.tv.v, c.tv.behind_sphere_mult, x, y, z, (bradius == 0.0f) ? radius : bradius);
}
// skip_uw_draw(pos, radius)
TERRA_HD bool scv_skip_uw(scenery_view_consts_t const &c, float z, float radius) {return c.uw_skip && c.tv.v.pos[2] > c.tv.water_plane_z && (z + radius) < c.min_water_plane_z;}
// is_visible(shadow_only, bradius, xlate) at pos + xlate = (x, y, z)
TERRA_HD bool scv_is_visible(scenery_view_consts_t const &c, float bradius, float radius, float x, float y, float z) {
	if (!scv_check_visible(c, bradius, radius, x, y, z)) return false;
	return c.shadow || !scv_skip_uw(c, z, radius);
}
TERRA_HD float scv_dist(scenery_view_consts_t const &c, float x, float y, float z) { // distance_to_camera
	float const *cam = c.tv.v.pos;
	return sqrtf((cam[0] - x)*(cam[0] - x) + (cam[1] - y)*(cam[1] - y) + (cam[2] - z)*(cam[2] - z));
}
// get_size_scale(dist, scale_val): (scale_val == 0.0) ? 1.0 : min(1.0f, pow(scale_val/dist_to_camera, scale_exp)), the float pow
TERRA_HD float scv_size_scale(scenery_view_consts_t const &c, float dist) {
	if (c.scale_val == 0.0f) return 1.0f;
	float const p = glibc_powf(c.scale_val/dist, 8.0f);
	return (p < 1.0f) ? p : 1.0f;
}
// get_def_smap_ndiv(radius): min(N_SPHERE_DIV, max(4, int(0.5*radius/approx_pixel_width(smap_sz))))
TERRA_HD int scv_smap_ndiv(scenery_view_consts_t const &c, float radius) {
	int const q = d2i_x86(0.5*(double)radius/(double)c.smap_pw), m = (4 < q) ? q : 4;
	return (m < 32) ? m : 32;
}
// the `2*get_pt_line_thresh()*radius < dist` of the rocks and the stems
TERRA_HD bool scv_small(scenery_view_consts_t const &c, float radius, float dist) {return !c.shadow && (2.0f*c.pt_thresh)*radius < dist;}

// ---- a record -> its draw word, size_scale, dist and the streams it enters (bit s: stream s)
struct scenery_view_rec_t {uint32_t word; float size_scale, dist; uint32_t streams;};
enum {SCV_S_ROCK_SHAPE = 0, SCV_S_SURFACE_ROCK, SCV_S_ROCK, SCV_S_LOG, SCV_S_STUMP, SCV_S_MUSHROOM, SCV_S_STEM, SCV_S_BERRIES, SCV_S_VOXEL_ROCK, SCV_S_PLANT_LEAVES,
      SCV_S_LEAFY_LEAVES, SCV_S_PT_SURFACE_ROCK, SCV_S_PT_ROCK, SCV_S_LN_LOG, SCV_S_LN_STUMP, SCV_S_LN_STEM};
// the group of a stream
TERRA_HD uint32_t scenery_view_group(uint32_t s) {return (s <= SCV_S_LEAFY_LEAVES) ? s : ((s <= SCV_S_PT_ROCK) ? (uint32_t)SCV_G_PLD_POINTS : (uint32_t)SCV_G_PLD_LINES);}

TERRA_HD scenery_view_rec_t scenery_view_record(scenery_view_consts_t const &c, scenery_place_pod_t const &r, float ov) {
	scenery_view_rec_t o; o.word = SCV_NONE; o.size_scale = 0.0f; o.dist = 0.0f; o.streams = 0u;
	float const *cam = c.tv.v.pos;
	float const wpz = c.tv.water_plane_z;
	float const radius = (ov > 0.0f) ? ov : r.radius;
	float const x = r.pos[0] + c.offx, y = r.pos[1] + c.offy; // pos + xlate
	switch (r.kind) {
	case SCENERY_ROCK_SHAPE: { // rock_shape3d::draw
		if (!c.opaque) break;
		if (!(ov > 0.0f)) {o.word = SCV_ENGINE; break;} // gen_rock's points give the radius: the engine's
		float const pz = (float)((double)r.pos[2] + 0.1*(double)radius); // pos.z += 0.1*radius (:156)
		if (!scv_is_visible(c, 0.0f, radius, x, y, pz + 0.0f)) break;
		if (c.reflection && pz < wpz) break;
		o.word = SCV_POLY; o.streams = 1u << SCV_S_ROCK_SHAPE;
		break;
	}
	case SCENERY_SURFACE_ROCK: case SCENERY_ROCK: case SCENERY_VOXEL_ROCK: { // surface_rock::draw, s_rock::draw, voxel_rock::draw
		if (!c.opaque) break;
		float const z = r.pos[2] + 0.0f;
		float const bradius = (r.kind == SCENERY_ROCK) ? (float)(1.3*(double)radius) : ((r.kind == SCENERY_VOXEL_ROCK) ? radius : 0.0f);
		if (!scv_is_visible(c, bradius, radius, x, y, z)) break;
		if (c.reflection && r.pos[2] < wpz) break;
		float const dist = scv_dist(c, x, y, z);
		o.dist = dist;
		if (r.kind != SCENERY_VOXEL_ROCK && scv_small(c, radius, dist)) { // draw as point
			o.word = SCV_POINT; o.streams = 1u << ((r.kind == SCENERY_ROCK) ? SCV_S_PT_ROCK : SCV_S_PT_SURFACE_ROCK);
			break;
		}
		uint32_t ndiv = 0;
		if (r.kind == SCENERY_ROCK) {ndiv = (uint32_t)scv_clamp(4, 32, c.shadow ? scv_smap_ndiv(c, radius) : f2i_x86(c.sscale*radius/dist));}
		o.word = SCV_POLY | (ndiv << SCV_NDIV_SHIFT); o.size_scale = scv_size_scale(c, dist);
		o.streams = 1u << ((r.kind == SCENERY_ROCK) ? SCV_S_ROCK : ((r.kind == SCENERY_VOXEL_ROCK) ? SCV_S_VOXEL_ROCK : SCV_S_SURFACE_ROCK));
		break;
	}
	case SCENERY_LOG: case SCENERY_STUMP: { // s_log::draw, s_stump::draw
		if (!c.opaque || !c.wood || r.iv[0] < 0) break;
		bool const log = r.kind == SCENERY_LOG;
		float const radius2 = r.p[0];
		float cx, cy, cz, bsr, zref;
		if (log) { // center = (pos + pt2)*0.5 + xlate; get_bsphere_radius() = max(length, max(radius, radius2))
			cx = (r.pos[0] + r.p[5])*0.5f + c.offx; cy = (r.pos[1] + r.p[6])*0.5f + c.offy; cz = (r.pos[2] + r.p[7])*0.5f + 0.0f;
			bsr = scv_max(r.p[1], scv_max(radius, radius2)); zref = 0.5f*(r.pos[2] + r.p[7]);
		}
		else {     // center = pos_cs + point(0.0, 0.0, 0.5*height); max(height, max(radius, radius2))
			cx = x + 0.0f; cy = y + 0.0f; cz = (r.pos[2] + 0.0f) + (float)(0.5*(double)r.p[1]);
			bsr = scv_max(r.p[1], scv_max(radius, radius2)); zref = r.pos[2];
		}
		if (!scv_check_visible(c, bsr, radius, cx, cy, cz)) break;
		if (c.reflection && zref < wpz) break;
		float const dist = scv_dist(c, cx, cy, cz);
		o.dist = dist;
		if (!c.shadow && c.pt_thresh*(radius + radius2) < dist) {o.word = SCV_LINE; o.streams = 1u << (log ? SCV_S_LN_LOG : SCV_S_LN_STUMP); break;} // draw as line
		double const k = log ? 2.0 : 2.2;
		int const ndiv = scv_clamp(3, 32, c.shadow ? scv_smap_ndiv(c, (float)(k*(double)radius)) : d2i_x86(k*(double)c.sscale*(double)radius/(double)dist));
		uint32_t w = SCV_POLY | ((uint32_t)ndiv << SCV_NDIV_SHIFT);
		if (log) {
			if (c.shadow || !((double)dist > 0.75*(double)c.pt_thresh*(double)radius)) { // the end visible to the camera
				float const dp = r.p[2]*(cam[0] - cx) + r.p[3]*(cam[1] - cy) + r.p[4]*(cam[2] - cz); // dot_product_ptv(dir, get_camera_pos(), center)
				w |= SCV_LOG_END | (((double)dp > 0.0) ? 0u : (uint32_t)SCV_LOG_END2);
			}
		}
		else {
			float const dx = cam[0] - x, dy = cam[1] - y, dz = cam[2] - (r.pos[2] + 0.0f); // camera_delta
			if (dz > r.p[1] && (double)dz > 0.1*(double)(fabsf(dx) + fabsf(dy))) {w |= SCV_STUMP_TOP;}
		}
		o.word = w; o.streams = 1u << (log ? SCV_S_LOG : SCV_S_STUMP);
		break;
	}
	case SCENERY_MUSHROOM: { // mushroom::draw; not drawn in the shadow pass (:1475)
		if (!c.opaque || c.shadow) break;
		if (c.reflection && r.pos[2] < wpz) break;
		float const height = r.p[0], capz = r.pos[2] + (height - 0.5f*radius); // cap_center
		float const cx = (r.pos[0] + 0.0f) + c.offx, cy = (r.pos[1] + 0.0f) + c.offy, cz = capz + 0.0f;
		float const dist = scv_dist(c, cx, cy, cz);
		o.dist = dist;
		if ((double)dist > 1000.0*(double)radius) break; // too far away
		if (!scv_check_visible(c, scv_max(height, radius), radius, cx, cy, cz)) break;
		int const ndiv = scv_clamp(3, 32, d2i_x86(1.0*(double)c.sscale*(double)radius/(double)dist));
		o.word = SCV_POLY | ((uint32_t)ndiv << SCV_NDIV_SHIFT) | ((cam[2] < capz) ? (uint32_t)SCV_CAP_UNDERSIDE : 0u);
		o.streams = 1u << SCV_S_MUSHROOM;
		break;
	}
	case SCENERY_PLANT: { // s_plant::draw_stem, draw_berries, draw_leaves
		float const height = r.p[0];
		bool const water_plant = r.iv[0] >= NUM_LAND_PLANT_TYPES;
		bool const uw = water_plant && (c.reflection || (!c.shadow && r.pos[2] < wpz && cam[2] > wpz)); // underwater, skip (:855, :901)
		float const z2 = (r.pos[2] + 0.0f) + (float)(0.5*(double)height), x2 = x + 0.0f, y2 = y + 0.0f; // pos2
		uint32_t w = SCV_NONE;
		if (c.opaque && !uw && scv_check_visible(c, height + radius, radius, x2, y2, z2)) {
			float const dist = scv_dist(c, x2, y2, z2);
			o.dist = dist;
			if (scv_small(c, radius, dist)) {w = SCV_LINE; o.streams |= 1u << SCV_S_LN_STEM;} // draw as line
			else {
				int const ndiv = scv_clamp(3, 32, c.shadow ? scv_smap_ndiv(c, (float)(2.0*(double)radius)) : d2i_x86(2.0*(double)c.sscale*(double)radius/(double)dist));
				w = SCV_POLY | ((uint32_t)ndiv << SCV_NDIV_SHIFT); o.streams |= 1u << SCV_S_STEM;
			}
		}
		float const lr = 0.5f*(height + radius);
		if (c.opaque && !c.shadow && view_sphere_visible(c.tv.v, c.tv.behind_sphere_mult, x2, y2, z2, lr)) { // draw_berries up to berries.empty()
			float const dist = scv_dist(c, x2, y2, z2);
			o.dist = dist;
			float const size_scale = c.pt_thresh*radius/dist;
			if (!((double)size_scale < 1.2)) {
				int const ndiv = scv_clamp(4, 16, d2i_x86(2.0*(double)size_scale));
				w |= SCV_BERRIES | ((uint32_t)ndiv << SCV_BERRY_NDIV_SHIFT); o.streams |= 1u << SCV_S_BERRIES;
			}
		}
		if (c.leaves && !uw && scv_check_visible(c, lr, radius, x2, y2, z2)) {w |= SCV_LEAVES; o.streams |= 1u << SCV_S_PLANT_LEAVES;}
		o.word = w;
		break;
	}
	case SCENERY_LEAFY_PLANT: { // leafy_plant::draw_leaves
		if (!c.leaves) break;
		if (!scv_is_visible(c, radius, radius, x, y, r.pos[2] + 0.0f)) break;
		if (c.reflection && r.pos[2] < wpz) break;
		o.word = SCV_LEAVES | ((r.pos[2] < wpz) ? (uint32_t)SCV_UNDERWATER : 0u); o.streams = 1u << SCV_S_LEAFY_LEAVES;
		break;
	}
	default: break; // no such kind: not drawn
	}
	return o;
}
// the streams of a record from what the call wrote of it: its kind and its draw word
TERRA_HD uint32_t scenery_view_streams(int kind, uint32_t w) {
	uint32_t const form = w & SCV_FORM_MASK;
	uint32_t s = 0;
	switch (kind) {
	case SCENERY_ROCK_SHAPE:   if (form == SCV_POLY) {s = 1u << SCV_S_ROCK_SHAPE;} break;
	case SCENERY_SURFACE_ROCK: s = (form == SCV_POLY) ? 1u << SCV_S_SURFACE_ROCK : ((form == SCV_POINT) ? 1u << SCV_S_PT_SURFACE_ROCK : 0u); break;
	case SCENERY_ROCK:         s = (form == SCV_POLY) ? 1u << SCV_S_ROCK : ((form == SCV_POINT) ? 1u << SCV_S_PT_ROCK : 0u); break;
	case SCENERY_VOXEL_ROCK:   if (form == SCV_POLY) {s = 1u << SCV_S_VOXEL_ROCK;} break;
	case SCENERY_LOG:          s = (form == SCV_POLY) ? 1u << SCV_S_LOG : ((form == SCV_LINE) ? 1u << SCV_S_LN_LOG : 0u); break;
	case SCENERY_STUMP:        s = (form == SCV_POLY) ? 1u << SCV_S_STUMP : ((form == SCV_LINE) ? 1u << SCV_S_LN_STUMP : 0u); break;
	case SCENERY_MUSHROOM:     if (form == SCV_POLY) {s = 1u << SCV_S_MUSHROOM;} break;
	case SCENERY_PLANT:
		s = (form == SCV_POLY) ? 1u << SCV_S_STEM : ((form == SCV_LINE) ? 1u << SCV_S_LN_STEM : 0u);
		if (w & SCV_BERRIES) {s |= 1u << SCV_S_BERRIES;}
		if (w & SCV_LEAVES) {s |= 1u << SCV_S_PLANT_LEAVES;}
		break;
	case SCENERY_LEAFY_PLANT:  if (w & SCV_LEAVES) {s = 1u << SCV_S_LEAFY_LEAVES;} break;
	default: break;
	}
	return s;
}

// ---- the arrays of a call, in the order of terra_tiles_scenery_view[_dev]: host pointers in the host form's first record, device pointers everywhere else
struct scenery_view_io_t {
	terra_tile_stats const *stats; uint8_t const *skip; scenery_place_pod_t const *objs; uint32_t const *counts; float const *rov;
	scenery_view_tile_pod_t *tile_out; uint32_t *draw; float *size_scale, *dist; uint32_t *list, *group_counts;
};
// the argument rules of a call, behind scenery_view_check: throws what the call refuses; false: nothing to do (n == 0).  dev: the arrays are the device's
inline bool scenery_view_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, uint32_t list_capacity, scenery_view_io_t const &io, bool dev) {
	if ((uint64_t)n*capacity > 0xFFFFFFFFull || (uint64_t)n*list_capacity > 0xFFFFFFFFull) throw std::invalid_argument("tiles_scenery_view: n*capacity and n*list_capacity must fit 32 bits");
	if (n == 0) return false;
	if (!tile_xy || !io.stats || !io.counts || !io.tile_out || !io.group_counts || (capacity && (!io.objs || !io.draw || !io.size_scale || !io.dist)) || (list_capacity && !io.list)) {
		throw std::invalid_argument("tiles_scenery_view: null argument");
	}
	if (dev && (((uintptr_t)io.stats | (uintptr_t)io.objs | (uintptr_t)io.counts | (uintptr_t)io.rov | (uintptr_t)io.tile_out | (uintptr_t)io.draw | (uintptr_t)io.size_scale |
	             (uintptr_t)io.dist | (uintptr_t)io.list | (uintptr_t)io.group_counts) & 3u) != 0) {
		throw std::invalid_argument("tiles_scenery_view: every array but skip must be 4-byte aligned");
	}
	return true;
}

// ---- the literal body: tile t of the batch, its records walked once, then once per stream for the lists
TERRA_HD void scenery_view_tile_literal(scenery_view_consts_t const &c, scenery_view_io_t const &io, int32_t const *tile_xy, size_t t) {
	uint32_t const cnt = (io.skip && io.skip[t]) ? 0u : min_u32(io.counts[t], c.cap);
	scenery_view_tile_pod_t o; o.dist_scale = 0.0f; o.scale_val = 0.0f; o.flags = o.num_records = o.list_written = 0u; o.pad[0] = o.pad[1] = o.pad[2] = 0u;
	uint32_t groups[SCV_GROUPS];
	for (uint32_t g = 0; g < SCV_GROUPS; ++g) {groups[g] = 0u;}
	float ds = 0.0f;
	if (cnt != 0u && scenery_view_tile(c, tile_xy[2*t], tile_xy[2*t + 1], io.stats[t].mzmin, io.stats[t].mzmax, io.stats[t].radius, ds)) {
		scenery_place_pod_t const *const recs = io.objs + t*c.cap;
		for (uint32_t j = 0; j < cnt; ++j) {
			scenery_view_rec_t const r = scenery_view_record(c, recs[j], io.rov ? io.rov[t*c.cap + j] : 0.0f);
			io.draw[t*c.cap + j] = r.word; io.size_scale[t*c.cap + j] = r.size_scale; io.dist[t*c.cap + j] = r.dist;
		}
		uint32_t at = 0;
		#pragma unroll // (a walk per stream with its bit and its group as constants, the groups in registers: what the device build made of the loop in the driver)
		for (uint32_t s = 0; s < SCV_STREAMS; ++s) { // a stable split of the record list
			for (uint32_t j = 0; j < cnt; ++j) {
				if (!((scenery_view_streams(recs[j].kind, io.draw[t*c.cap + j]) >> s) & 1u)) continue;
				if (at < c.list_cap) {io.list[t*c.list_cap + at] = j;}
				++at; ++groups[scenery_view_group(s)];
			}
		}
		o.dist_scale = ds; o.scale_val = c.scale_val; o.flags = scenery_view_tile_flags(c); o.num_records = cnt; o.list_written = min_u32(at, c.list_cap);
	}
	io.tile_out[t] = o;
	for (uint32_t g = 0; g < SCV_GROUPS; ++g) {io.group_counts[t*SCV_GROUPS + g] = groups[g];}
}

} // namespace terra
