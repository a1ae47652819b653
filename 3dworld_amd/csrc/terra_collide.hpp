// terra_collide.hpp -- sphere collisions and tree box tests against the three object containers of a tile batch: tile_t::check_sphere_collision
// (src/tiled_mesh.cpp:2146-2168) and tile_draw_t::check_sphere_collision (:3566-3569) with get_tile_containing_point / get_tile_pair_at_point (:3532-3537),
// small_tree_group::check_sphere_coll and small_tree::check_sphere_coll (src/sm_tree.cpp:181-186, 841-852), tree_cont_t::check_sphere_coll and tree::check_sphere_coll
// (src/Tree.cpp:280-294), scenery_group::check_sphere_coll (src/scenery.cpp:1187-1199) over scenery_obj::check_sphere_coll (:80-86), s_stump::check_sphere_coll
// (:665-668) and s_plant::check_sphere_coll (:772-775), sphere_vert_cylin_intersect (src/Math3d.cpp:427-437), sphere_cube_intersect (:930-935), dist_less_than /
// dist_xy_less_than (src/inlines.h:176-195), round_fp (:63), pointT::get_norm (src/3DWorld.h:297-300), cube_t::contains_pt_exp, is_zero_area, contains_pt_xy,
// intersects (:524-583), tile_t::get_bcube / get_tile_zmax / contains_point (src/tiled_mesh.h:207,232-236,264); tile_t::check_cube_int_trees and
// tile_draw_t::check_cube_int_trees (src/tiled_mesh.cpp:2170-2173, 3576-3579) over tree_cont_t::check_cube_int and tree::check_cube_int (src/Tree.cpp:296-309).
//
// A small tree's trunk_cylin is terra_treeview.hpp's tree_view_record (the rotated-palm override included), both all_bcubes are calc_bcube as the tree view and the
// deciduous view form them (tree_view_bounds; decid_view_union_t), the tile's box is terra_terrainview.hpp's terrain_view_geom.  Logs and mushrooms never collide
// (src/scenery.h:114; the "no mushrooms" line of :1197).  The asserts of sphere_vert_cylin_intersect are not restated.
//
// The bodies are shared by k_sphere_collide / k_cube_int_trees (terra_kernels.hpp), by the driver's simple form (one logical thread per query, the reference's loops)
// and by a stand-alone host check.  Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is
// written out.
#pragma once
#include "terra_treeview.hpp"
#include "terra_decidview.hpp"
#include "terra_sceneryplace.hpp"

namespace terra {

enum {COLL_INC_DTREES = 1, COLL_INC_PTREES = 2, COLL_INC_SCENERY = 4};                               // terra_sphere_query.flags
enum {COLL_TILE_DISTANT = 1, COLL_TILE_NO_SCENERY = 2};                                              // the per-tile flag byte: is_distant, !scenery.generated
enum {COLL_HIT_PINE = 1, COLL_HIT_DECID = 2, COLL_HIT_SCENERY = 4, COLL_ROCK_SHAPE_UNDECIDED = 8,    // terra_sphere_hit.word
      COLL_STAGE_SHIFT = 8, COLL_STAGE_MASK = 0xF00,
      COLL_STAGE_TESTED = 0, COLL_STAGE_NO_TILE = 1, COLL_STAGE_DISTANT = 2, COLL_STAGE_OUTSIDE = 3, COLL_STAGE_ABOVE = 4, COLL_STAGE_BAD_QUERY = 5};
enum {CUBE_INT_HIT = 1, CUBE_INT_NO_TILE = 2, CUBE_INT_BAD_QUERY = 4};                               // the result byte of the cube call
constexpr int COLL_SCENERY_PASSES = 7; // rock_shapes, surface_rocks, voxel_rocks, rocks, (logs: nothing), stumps, plants, leafy_plants

struct sphere_query_pod_t {float pos[3], radius; int32_t tile; uint32_t flags;}; // terra_sphere_query
struct sphere_hit_pod_t {float pos[3]; int32_t tile; uint32_t word, nhits;};     // terra_sphere_hit
struct coll_pt_t {float x, y, z;};

// the arrays of a call, all on the device; a container without records or counts is absent in every tile
struct collide_in_t {
	terra_tile_stats const *stats; float const *trmax, *tile_zmax; uint8_t const *flags;
	tree_place_pod_t const *pine; uint32_t const *pine_counts; trunk_override_pod_t const *ov;
	decid_place_pod_t const *decid; uint32_t const *decid_counts;
	scenery_place_pod_t const *scen; uint32_t const *scen_counts; float const *rov;
	tree_inst_pod_t const *insts; decid_tree_data_pod_t const *data; float const *br_scale;
	int32_t const *tile_xy; int32_t const *slots; // the key table of the batch: slots[hash] -> batch index or -1
};
struct collide_consts_t {
	tree_view_consts_t pv;           // what tree_view_record reads (pv.a.offx / offy: ptree_off.get_xlate()); pv.tv: what the tile's box reads
	float doffx, doffy, soffx, soffy; // dtree_off.get_xlate(), scenery_off.get_xlate()
	float lookup_ox, lookup_oy;      // (xoff - xoff2)*DX_VAL, (yoff - yoff2)*DY_VAL of get_tile_pair_at_point
	uint32_t n, hbits, num_data, pine_cap, decid_cap, scen_cap;
};

// ---- the key table: open addressing over (tx, ty), at most half full, so a search ends at an empty slot
TERRA_HD uint64_t batch_key(int32_t tx, int32_t ty) {return ((uint64_t)(uint32_t)tx << 32) | (uint32_t)ty;}
TERRA_HD uint32_t batch_key_hash(uint64_t k, uint32_t hbits) {return (uint32_t)((k*0x9E3779B97F4A7C15ull) >> (64 - hbits));}
TERRA_HD int32_t batch_key_find(int32_t const *tile_xy, int32_t const *slots, uint32_t hbits, uint32_t n, int32_t tx, int32_t ty) {
	uint32_t const hmask = (uint32_t)((1ull << hbits) - 1);
	uint64_t const k = batch_key(tx, ty);
	uint32_t h = batch_key_hash(k, hbits);
	for (uint32_t step = 0; step <= hmask; ++step, h = (h + 1) & hmask) {
		int32_t const v = slots[h];
		if (v < 0 || (uint32_t)v >= n) return -1;
		if (tile_xy[2*v] == tx && tile_xy[2*v + 1] == ty) return v;
	}
	return -1;
}

// ---- the primitives
TERRA_HD int coll_round_fp(float v) {return (v > 0.0f) ? f2i_x86(v + 0.5f) : f2i_x86(v - 0.5f);} // round_fp(float) as the reference binary converts
// get_tile_pair_at_point
TERRA_HD void coll_tile_pair(collide_consts_t const &c, float x, float y, int &tx, int &ty) {
	tx = coll_round_fp(0.5f*(x - c.lookup_ox)/c.pv.tv.xss); ty = coll_round_fp(0.5f*(y - c.lookup_oy)/c.pv.tv.yss);
}
// sphere_cube_intersect: DMIN_CHECK per dimension, with its early return
TERRA_HD bool coll_sphere_cube(float px, float py, float pz, float radius, float const d[6]) {
	float dmin = 0.0f;
	float const r2 = radius*radius;
	if      (px < d[0]) {float const dist = px - d[0]; dmin += dist*dist;}
	else if (px > d[1]) {float const dist = px - d[1]; dmin += dist*dist;}
	if (dmin > r2) return false;
	if      (py < d[2]) {float const dist = py - d[2]; dmin += dist*dist;}
	else if (py > d[3]) {float const dist = py - d[3]; dmin += dist*dist;}
	if (dmin > r2) return false;
	if      (pz < d[4]) {float const dist = pz - d[4]; dmin += dist*dist;}
	else if (pz > d[5]) {float const dist = pz - d[5]; dmin += dist*dist;}
	if (dmin > r2) return false;
	return true;
}
TERRA_HD bool coll_zero_area(float const d[6]) {return d[0] == d[1] || d[2] == d[3] || d[4] == d[5];}
// the gate of both tree containers: !all_bcube.is_zero_area() && !sphere_cube_intersect(center, radius, all_bcube) -> return 0
TERRA_HD bool coll_gate_exits(coll_pt_t const &c, float radius, float const bc[6]) {return !coll_zero_area(bc) && !coll_sphere_cube(c.x, c.y, c.z, radius, bc);}
// center = base + normal*(1.001*rsum) with normal = v.get_norm(): a vector shorter than TOLERANCE stays as it is
TERRA_HD void coll_push(coll_pt_t &c, float bx, float by, float bz, float vx, float vy, float vz, float rsum) {
	float const vmag = sqrtf(vx*vx + vy*vy + vz*vz);
	float nx = vx, ny = vy, nz = vz;
	if (!(vmag < 1.0E-12f)) {nx = vx/vmag; ny = vy/vmag; nz = vz/vmag;}
	float const s = (float)(1.001*(double)rsum); // operator*(T const val): the double narrows at the call
	c.x = bx + nx*s; c.y = by + ny*s; c.z = bz + nz*s;
}
// sphere_vert_cylin_intersect(center, radius, cylinder_3dw(p1, p2, r1, r2)): of p2 only z is read
TERRA_HD bool coll_vert_cylin(coll_pt_t &c, float radius, float p1x, float p1y, float p1z, float p2z, float r1, float r2) {
	float const rsum = radius + max_std(r1, r2);
	if (c.z < min_std(p1z, p2z) || c.z > max_std(p1z, p2z)) return false;
	if (!((p1x - c.x)*(p1x - c.x) + (p1y - c.y)*(p1y - c.y) < rsum*rsum)) return false; // dist_xy_less_than(c.p1, center, rsum)
	coll_push(c, p1x, p1y, c.z, c.x - p1x, c.y - p1y, 0.0f, rsum);
	return true;
}
// small_tree::check_sphere_coll
TERRA_HD bool coll_small_tree(tree_view_rec_t const &r, coll_pt_t &c, float radius) {
	if (r.type == T_BUSH) return false;
	float const dv = radius + r.r1;
	if (!((c.x - r.pos[0])*(c.x - r.pos[0]) + (c.y - r.pos[1])*(c.y - r.pos[1]) < dv*dv)) return false;
	if (c.z > r.p2[2] && c.z - radius < r.p2[2]) { // short tree
		if (r.p2[2] - r.p1[2] < radius) return false; // too short, can step over
		return coll_vert_cylin(c, radius, r.p1[0], r.p1[1], r.p1[2], r.p2[2] + radius, r.r1, r.r2);
	}
	return coll_vert_cylin(c, radius, r.p1[0], r.p1[1], r.p1[2], r.p2[2], r.r1, r.r2);
}
// tree::check_sphere_coll; br_scale: tree_data_t::br_scale of the record's table entry
TERRA_HD bool coll_decid_tree(decid_tree_data_pod_t const &td, float br_scale, float const pos[3], coll_pt_t &c, float radius) {
	float const x = c.x - pos[0], y = c.y - pos[1], z = c.z - pos[2]; // center - tree_center
	float const *b = td.branches_bcube;
	if (!(x > b[0] - radius && x < b[1] + radius && y > b[2] - radius && y < b[3] + radius && z > b[4] - radius && z < b[5] + radius)) return false; // contains_pt_exp
	float const trunk_radius = (float)(0.9*(double)br_scale*(double)td.base_radius);
	float const trunk_height = max_std(td.sphere_radius, td.sphere_center_zoff);
	return coll_vert_cylin(c, radius, pos[0], pos[1], pos[2], pos[2] + trunk_height, trunk_radius, trunk_radius);
}
// the kind of pass k of scenery_group::check_sphere_coll
TERRA_HD int coll_scenery_pass_kind(int k) {
	return (k == 0) ? (int)SCENERY_ROCK_SHAPE : (k == 1) ? (int)SCENERY_SURFACE_ROCK : (k == 2) ? (int)SCENERY_VOXEL_ROCK : (k == 3) ? (int)SCENERY_ROCK :
	       (k == 4) ? (int)SCENERY_STUMP : (k == 5) ? (int)SCENERY_PLANT : (int)SCENERY_LEAFY_PLANT;
}
// one scenery record's check_sphere_coll.  ov: its radius_override entry (0: none).  undecided: a rock_shape without an override (gen_rock's points give its radius)
TERRA_HD bool coll_scenery(scenery_place_pod_t const &r, float ov, coll_pt_t &c, float sphere_radius, bool &undecided) {
	float const radius = (ov > 0.0f) ? ov : r.radius;
	switch (r.kind) {
	case SCENERY_ROCK_SHAPE: case SCENERY_SURFACE_ROCK: case SCENERY_VOXEL_ROCK: case SCENERY_ROCK: case SCENERY_LEAFY_PLANT: { // scenery_obj::check_sphere_coll
		float pz = r.pos[2];
		if (r.kind == SCENERY_ROCK_SHAPE) {
			if (!(ov > 0.0f)) {undecided = true; return false;}
			pz = (float)((double)r.pos[2] + 0.1*(double)radius); // pos.z += 0.1*radius (src/scenery.cpp:156)
		}
		float const rsum = radius + sphere_radius;
		float const x = c.x - r.pos[0], y = c.y - r.pos[1], z = c.z - pz;
		if (!(x*x + y*y + z*z < rsum*rsum)) return false;
		coll_push(c, r.pos[0], r.pos[1], pz, x, y, z, rsum);
		return true;
	}
	case SCENERY_STUMP: {
		float const radius2 = r.p[0], height = r.p[1];
		float const dv = max_std(height, max_std(radius, radius2)) + sphere_radius;
		float const x = c.x - r.pos[0], y = c.y - r.pos[1], z = c.z - r.pos[2];
		if (!(x*x + y*y + z*z < dv*dv)) return false;
		return coll_vert_cylin(c, sphere_radius, r.pos[0] - 0.0f, r.pos[1] - 0.0f, r.pos[2] - (float)(0.2*(double)height), r.pos[2] + height, radius, radius);
	}
	case SCENERY_PLANT: {
		float const height = r.p[0];
		float const dv = 0.5f*(height + radius) + sphere_radius;
		float const x = c.x - r.pos[0], y = c.y - r.pos[1], z = c.z - r.pos[2];
		if (!(x*x + y*y + z*z < dv*dv)) return false;
		return coll_vert_cylin(c, sphere_radius, r.pos[0] - 0.0f, r.pos[1] - 0.0f, r.pos[2] - (float)(0.1*(double)height), r.pos[2] + height, radius, radius);
	}
	default: return false; // logs, mushrooms, no such kind
	}
}

// ---- a query and its tile
TERRA_HD bool coll_query_ok(sphere_query_pod_t const &q) {return isfinite(q.pos[0]) && isfinite(q.pos[1]) && isfinite(q.pos[2]) && isfinite(q.radius) && q.radius >= 0.0f;}
// the batch index a position or an explicit index leads to, -1: none.  Nothing is indexed before its range is known
TERRA_HD int32_t coll_tile_of(collide_consts_t const &c, collide_in_t const &in, int32_t tile, float x, float y) {
	if (tile >= 0) return ((uint32_t)tile < c.n) ? tile : -1;
	if (tile != -1 || c.n == 0) return -1;
	int tx, ty;
	coll_tile_pair(c, x, y, tx, ty);
	return batch_key_find(in.tile_xy, in.slots, c.hbits, c.n, tx, ty);
}
// tile_t::check_sphere_collision down to `bool coll(0)`: the stage at which the query leaves, COLL_STAGE_TESTED: it goes on
TERRA_HD uint32_t coll_tile_stage(collide_consts_t const &c, collide_in_t const &in, uint32_t t, float const pos[3], float sradius) {
	if (in.flags && (in.flags[t] & COLL_TILE_DISTANT)) return COLL_STAGE_DISTANT;
	terra_tile_stats const &st = in.stats[t];
	float const tile_zmax = in.tile_zmax ? in.tile_zmax[t] : st.mzmax; // get_tile_zmax()
	terrain_view_geom_t const g = terrain_view_geom(c.pv.tv, in.tile_xy[2*t], in.tile_xy[2*t + 1], st.mzmin, st.mzmax, in.trmax ? in.trmax[t] : 0.0f, tile_zmax);
	if (!(pos[0] > g.bc[0][0] && pos[0] < g.bc[0][1] && pos[1] > g.bc[1][0] && pos[1] < g.bc[1][1])) return COLL_STAGE_OUTSIDE; // contains_pt_xy
	if (pos[2] > tile_zmax + sradius) return COLL_STAGE_ABOVE;
	return COLL_STAGE_TESTED;
}
TERRA_HD uint32_t coll_pine_count(collide_consts_t const &c, collide_in_t const &in, uint32_t t)  {return (in.pine && in.pine_counts) ? min_u32(in.pine_counts[t], c.pine_cap) : 0u;}
TERRA_HD uint32_t coll_decid_count(collide_consts_t const &c, collide_in_t const &in, uint32_t t) {return (in.decid && in.decid_counts && in.data) ? min_u32(in.decid_counts[t], c.decid_cap) : 0u;}
TERRA_HD uint32_t coll_scen_count(collide_consts_t const &c, collide_in_t const &in, uint32_t t)  {return (in.scen && in.scen_counts) ? min_u32(in.scen_counts[t], c.scen_cap) : 0u;}
TERRA_HD bool coll_scenery_generated(collide_in_t const &in, uint32_t t) {return !(in.flags && (in.flags[t] & COLL_TILE_NO_SCENERY));}
// record j of tile t as the containers hold it; false: the views drop it
TERRA_HD bool coll_pine_rec(collide_consts_t const &c, collide_in_t const &in, uint32_t t, uint32_t j, tree_view_rec_t &rec) {
	size_t const i = (size_t)t*c.pine_cap + j;
	return tree_view_record(c.pv, in.insts, in.pine[i], in.ov ? in.ov + i : nullptr, rec);
}
TERRA_HD bool coll_decid_rec(collide_consts_t const &c, collide_in_t const &in, uint32_t t, uint32_t j, decid_place_pod_t &r) {
	r = in.decid[(size_t)t*c.decid_cap + j];
	return decid_view_valid(c.num_data, in.data, r);
}

// ---- the literal loops: one query from its tile's stage on.  What the simple form runs, and what the wave form must equal
struct coll_result_t {coll_pt_t c; uint32_t word, nhits;};
// calc_bcube of the two tree containers over the valid records; -> their number
TERRA_HD uint32_t coll_pine_bcube(collide_consts_t const &c, collide_in_t const &in, uint32_t t, uint32_t cnt, float bc[6]) {
	for (int k = 0; k < 6; ++k) {bc[k] = 0.0f;}
	bool any = false;
	uint32_t nvalid = 0;
	tree_view_rec_t rec;
	for (uint32_t j = 0; j < cnt; ++j) {
		if (!coll_pine_rec(c, in, t, j, rec)) continue;
		++nvalid;
		float d[6];
		if (!tree_view_bounds(rec, d)) continue;
		if (!any) {for (int k = 0; k < 6; ++k) {bc[k] = d[k];} any = true;}
		else {box_union(bc, d);}
	}
	return nvalid;
}
TERRA_HD uint32_t coll_decid_bcube(collide_consts_t const &c, collide_in_t const &in, uint32_t t, uint32_t cnt, float bc[6]) {
	decid_view_union_t un;
	decid_view_union_init(un);
	uint32_t nvalid = 0;
	decid_place_pod_t r;
	for (uint32_t j = 0; j < cnt; ++j) {
		if (!coll_decid_rec(c, in, t, j, r)) continue;
		++nvalid;
		float b[6], l[6];
		decid_view_bounds(in.data[r.tree_id], r.pos, b, l);
		decid_view_union_add(un, j, b, l);
	}
	decid_view_union_result(un, bc);
	return nvalid;
}
TERRA_HD coll_result_t coll_query_literal(collide_consts_t const &c, collide_in_t const &in, uint32_t t, float const pos[3], float radius, uint32_t flags) {
	coll_result_t o; o.c.x = pos[0]; o.c.y = pos[1]; o.c.z = pos[2]; o.word = 0u; o.nhits = 0u;
	float bc[6];
	uint32_t const np = (flags & COLL_INC_PTREES) ? coll_pine_count(c, in, t) : 0u;
	if (np != 0u && coll_pine_bcube(c, in, t, np, bc) != 0u) { // inc_ptrees && !pine_trees.empty()
		o.c.x -= c.pv.a.offx; o.c.y -= c.pv.a.offy; o.c.z -= 0.0f;
		if (!coll_gate_exits(o.c, radius, bc)) {
			tree_view_rec_t rec;
			for (uint32_t j = 0; j < np; ++j) {
				if (coll_pine_rec(c, in, t, j, rec) && coll_small_tree(rec, o.c, radius)) {o.word |= COLL_HIT_PINE; ++o.nhits;}
			}
		}
		o.c.x += c.pv.a.offx; o.c.y += c.pv.a.offy; o.c.z += 0.0f;
	}
	uint32_t const nd = (flags & COLL_INC_DTREES) ? coll_decid_count(c, in, t) : 0u;
	if (nd != 0u && coll_decid_bcube(c, in, t, nd, bc) != 0u) {
		o.c.x -= c.doffx; o.c.y -= c.doffy; o.c.z -= 0.0f;
		if (!coll_gate_exits(o.c, radius, bc)) {
			decid_place_pod_t r;
			for (uint32_t j = 0; j < nd; ++j) {
				if (coll_decid_rec(c, in, t, j, r) && coll_decid_tree(in.data[r.tree_id], in.br_scale ? in.br_scale[r.tree_id] : 1.0f, r.pos, o.c, radius)) {o.word |= COLL_HIT_DECID; ++o.nhits;}
			}
		}
		o.c.x += c.doffx; o.c.y += c.doffy; o.c.z += 0.0f;
	}
	if ((flags & COLL_INC_SCENERY) && coll_scenery_generated(in, t)) {
		uint32_t const ns = coll_scen_count(c, in, t);
		o.c.x -= c.soffx; o.c.y -= c.soffy; o.c.z -= 0.0f;
		for (int k = 0; k < COLL_SCENERY_PASSES; ++k) {
			int const kind = coll_scenery_pass_kind(k);
			for (uint32_t j = 0; j < ns; ++j) {
				size_t const i = (size_t)t*c.scen_cap + j;
				if (in.scen[i].kind != kind) continue;
				bool und = false;
				if (coll_scenery(in.scen[i], in.rov ? in.rov[i] : 0.0f, o.c, radius, und)) {o.word |= COLL_HIT_SCENERY; ++o.nhits;}
				if (und) {o.word |= COLL_ROCK_SHAPE_UNDECIDED;}
			}
		}
		o.c.x += c.soffx; o.c.y += c.soffy; o.c.z += 0.0f;
	}
	return o;
}
// one query from the start: what both forms write for it.  run: (t) -> coll_result_t
template<class RUN> TERRA_HD sphere_hit_pod_t coll_query(collide_consts_t const &c, collide_in_t const &in, sphere_query_pod_t const &q, RUN run) {
	sphere_hit_pod_t h; h.pos[0] = q.pos[0]; h.pos[1] = q.pos[1]; h.pos[2] = q.pos[2]; h.tile = -1; h.nhits = 0u;
	if (!coll_query_ok(q)) {h.word = (uint32_t)COLL_STAGE_BAD_QUERY << COLL_STAGE_SHIFT; return h;}
	int32_t const t = coll_tile_of(c, in, q.tile, q.pos[0], q.pos[1]);
	if (t < 0) {h.word = (uint32_t)COLL_STAGE_NO_TILE << COLL_STAGE_SHIFT; return h;}
	h.tile = t;
	uint32_t const stage = coll_tile_stage(c, in, (uint32_t)t, q.pos, q.radius);
	if (stage != COLL_STAGE_TESTED) {h.word = stage << COLL_STAGE_SHIFT; return h;}
	coll_result_t const r = run((uint32_t)t);
	h.pos[0] = r.c.x; h.pos[1] = r.c.y; h.pos[2] = r.c.z; h.word = r.word; h.nhits = r.nhits;
	return h;
}

// ---- the cube call: tile_draw_t::check_cube_int_trees.  cube: x1 x2 y1 y2 z1 z2
TERRA_HD bool coll_cube_ok(float const d[6]) {return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && isfinite(d[3]) && isfinite(d[4]) && isfinite(d[5]);}
TERRA_HD bool coll_cubes_intersect(float const a[6], float const b[6]) { // a.intersects(b): includes adjacency
	return !(b[1] < a[0] || b[0] > a[1] || b[3] < a[2] || b[2] > a[3] || b[5] < a[4] || b[4] > a[5]);
}
// c - dtree_off.get_xlate()
TERRA_HD void coll_cube_local(collide_consts_t const &c, float const d[6], float o[6]) {
	o[0] = d[0] - c.doffx; o[1] = d[1] - c.doffx; o[2] = d[2] - c.doffy; o[3] = d[3] - c.doffy; o[4] = d[4] - 0.0f; o[5] = d[5] - 0.0f;
}
// tree::check_cube_int(c) with c in the container's frame
TERRA_HD bool coll_decid_cube(decid_tree_data_pod_t const &td, float const pos[3], float const cube[6]) {
	float rel[6];
	for (int k = 0; k < 6; ++k) {rel[k] = cube[k] - pos[k >> 1];} // c - tree_center
	if (!coll_cubes_intersect(td.leaves_bcube, rel) && !coll_cubes_intersect(td.branches_bcube, rel)) return false;
	return coll_sphere_cube(0.0f, 0.0f, td.sphere_center_zoff, td.sphere_radius, rel); // td.get_center(), td.sphere_radius
}
// the tile of a cube: get_tile_containing_point(c.get_cube_center()), or the explicit index
TERRA_HD int32_t coll_cube_tile(collide_consts_t const &c, collide_in_t const &in, int32_t tile, float const d[6]) {
	return coll_tile_of(c, in, tile, 0.5f*(d[0] + d[1]), 0.5f*(d[2] + d[3]));
}
TERRA_HD uint8_t coll_cube_literal(collide_consts_t const &c, collide_in_t const &in, uint32_t t, float const d[6]) {
	uint32_t const nd = coll_decid_count(c, in, t);
	float bc[6], loc[6];
	if (nd == 0u || coll_decid_bcube(c, in, t, nd, bc) == 0u) return 0; // decid_trees.empty()
	coll_cube_local(c, d, loc);
	if (!coll_zero_area(bc) && !coll_cubes_intersect(bc, loc)) return 0;
	decid_place_pod_t r;
	for (uint32_t j = 0; j < nd; ++j) {
		if (coll_decid_rec(c, in, t, j, r) && coll_decid_cube(in.data[r.tree_id], r.pos, loc)) return CUBE_INT_HIT;
	}
	return 0;
}

} // namespace terra
