// terra_linetrees.hpp -- line queries with inc_trees != 0: the pine part of tile_t::line_intersect_mesh (src/tiled_mesh.cpp:2208-2215) under
// tile_draw_t::line_intersect_mesh (:3582-3604): small_tree_group::line_intersect with t != NULL (src/sm_tree.cpp:189-200), small_tree::line_intersect (:854-876) and
// line_intersect_trunc_cone with check_ends = 0 (src/Math3d.cpp:543-593), over pointT::normalize (src/3DWorld.h:273-278), matrix_mult and dot_product_ptv
// (src/inlines.h:227-240).  The mesh walk is terra_lineintersect.hpp's, a record's trunk_cylin terra_treeview.hpp's tree_view_record, get_radius()
// terra_treeao.hpp's small_tree_radius, check_line_clip terra_common.hpp's shadow_line_clip, cosf terra_sincosf.hpp's, atan2f terra_atan2f.hpp's.
//
// The bodies are shared by k_line_tree_boxes / k_line_intersect_trees (terra_kernels.hpp), by the driver's simple form (one logical thread per line, the reference's
// loops) and by a stand-alone host check.  Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion
// is written out; sums run in the reference's order.
//
// Two things are the source's and look odd: `(1-2*i)*num` of the root loop has an unsigned i, so the second pass multiplies num by float(4294967295u) = 2^32,
// not by -1; and where the source asserts (r2 > 0 && r2 > r1) the cylinder does not hit.
#pragma once
#include "terra_lineintersect.hpp"
#include "terra_treeview.hpp"
#include "terra_sincosf.hpp"
#include "terra_atan2f.hpp"

namespace terra {

enum {LINE_HIT_NONE = 0, LINE_HIT_MESH = 1, LINE_HIT_TREE = 2};
struct line_tree_hit_pod_t {float t; int32_t tile, xpos, ypos; float p[3]; uint32_t hit; int32_t tree; uint32_t part;}; // terra_line_tree_hit
static_assert(sizeof(line_tree_hit_pod_t) == 40, "terra_line_tree_hit");
// a tile's pine container for the query: calc_bcube() over the valid records and their number (0: pine_trees.empty())
struct alignas(16) line_tree_box_t {float bc[6]; uint32_t nvalid, pad;};
static_assert(sizeof(line_tree_box_t) == 32, "line_tree_box_t: two 16-byte loads");
struct line_trees_consts_t {
	line_query_consts_t q;
	tree_view_consts_t pv; // what tree_view_record reads; pv.a.offx / offy: ptree_off.get_xlate()
	uint32_t cap;          // records per tile, 0: no records (the query is the mesh query)
};
struct line_trees_in_t {tree_place_pod_t const *pine; uint32_t const *counts; trunk_override_pod_t const *ov; tree_inst_pod_t const *insts;};

// line_intersect_trunc_cone(p1, p2, cp1, cp2, r1, r2, check_ends = 0, t): radius r1 at cp1, r2 at cp2.  -> t_set
TERRA_HD int line_trunc_cone(float const p1[3], float const p2[3], float const cp1[3], float const cp2[3], float r1, float r2, float &t) {
	if (!(r2 > 0.0f && r2 > r1)) return 0; // the source's assert
	float V[3] = {cp1[0], cp1[1], cp1[2]};
	float const dir[3] = {cp2[0] - cp1[0], cp2[1] - cp1[1], cp2[2] - cp1[2]};
	if (r1 > 0.0f) {float const s = r1/(r2 - r1); V[0] -= dir[0]*s; V[1] -= dir[1]*s; V[2] -= dir[2]*s;} // extend to the cone's apex
	float A[3] = {cp2[0] - V[0], cp2[1] - V[1], cp2[2] - V[2]};
	float const D[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]}, d[3] = {p1[0] - V[0], p1[1] - V[1], p1[2] - V[2]};
	float const amag = sqrtf(A[0]*A[0] + A[1]*A[1] + A[2]*A[2]);
	float const g = glibc_cosf(glibc_atan2f(r2, amag));
	if (amag >= 1.0E-12f) {float const m = (float)(1.0/(double)amag); A[0] *= m; A[1] *= m; A[2] *= m;} // normalize()
	double M[3][3];
	for (int i = 0; i < 3; ++i) {
		for (int j = 0; j < 3; ++j) {M[i][j] = (double)A[i]*(double)A[j];}
		M[i][i] -= (double)g*(double)g;
	}
	float Md[3], MD[3];
	for (int i = 0; i < 3; ++i) { // matrix_mult: float x double sums narrowed to float
		Md[i] = (float)(((double)d[0]*M[i][0] + (double)d[1]*M[i][1]) + (double)d[2]*M[i][2]);
		MD[i] = (float)(((double)D[0]*M[i][0] + (double)D[1]*M[i][1]) + (double)D[2]*M[i][2]);
	}
	float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
	for (int i = 0; i < 3; ++i) {
		c0 += D[i]*MD[i];
		c1 += D[i]*Md[i];
		c2 += d[i]*Md[i];
	}
	float num = c1*c1 - c2*c0;
	int t_set = 0;
	if (num >= 0.0f) {
		float const len = sqrtf(dir[0]*dir[0] + dir[1]*dir[1] + dir[2]*dir[2]);
		num = sqrtf(num);
		for (unsigned i = 0; i < 2; ++i) {
			float const ti = (-c1 + (float)(1u - 2u*i)*num)/c0; // (1-2*i) is unsigned in the source
			if (ti >= 0.0f && ti <= 1.0f && (!t_set || ti < t)) { // between p1 and p2
				float const dp = A[0]*((p1[0] + D[0]*ti) - cp1[0]) + A[1]*((p1[1] + D[1]*ti) - cp1[1]) + A[2]*((p1[2] + D[2]*ti) - cp1[2]); // dot_product_ptv(A, p1 + D*ti, cp1)
				if (dp >= 0.0f && dp <= len) {t = ti; t_set = 1;}
			}
		}
	}
	return t_set;
}

// small_tree::line_intersect(p1, p2, t) with t != NULL: *t is lowered by a nearer cylinder; part: the cylinder that lowered it last (0 trunk_cylin, 1 the leaf cone)
TERRA_HD bool line_small_tree(tree_ao_consts_t const &a, tree_view_rec_t const &r, float const p1[3], float const p2[3], float &t, uint32_t &part) {
	if (!is_pine_tree_type(r.type)) return false;
	float const dirh[3] = {r.dir[0]*r.height, r.dir[1]*r.height, r.dir[2]*r.height}; // get_rot_dir()*height
	float lo[3], hi[3];
	for (int k = 0; k < 3; ++k) {
		lo[k] = r.pos[k] + ((r.type == T_PINE) ? (float)(0.35*(double)dirh[k]) : 0.0f); // operator*(S, pointT<T>): the double product narrows per component
		hi[k] = r.pos[k] + dirh[k];
	}
	float const radius = small_tree_radius(a, r.type, r.height, r.width);
	bool coll = false;
	float t_new = 0.0f;
	if (line_trunc_cone(p1, p2, r.p2, r.p1, r.r2, r.r1, t_new) && t_new < t) {t = t_new; coll = true; part = 0u;}
	t_new = 0.0f;
	if (line_trunc_cone(p1, p2, hi, lo, 0.0f, radius, t_new) && t_new < t) {t = t_new; coll = true; part = 1u;}
	return coll;
}

TERRA_HD uint32_t line_trees_count(line_trees_consts_t const &c, line_trees_in_t const &in, uint32_t tile) {return (c.cap && in.pine && in.counts) ? min_u32(in.counts[tile], c.cap) : 0u;}
// record j of a tile as the container holds it; false: the tree view drops it
TERRA_HD bool line_trees_rec(line_trees_consts_t const &c, line_trees_in_t const &in, uint32_t tile, uint32_t j, tree_view_rec_t &rec) {
	size_t const i = (size_t)tile*c.cap + j;
	return tree_view_record(c.pv, in.insts, in.pine[i], in.ov ? in.ov + i : nullptr, rec);
}
// calc_bcube of a tile's container and the number of its valid records, in record order
TERRA_HD line_tree_box_t line_trees_box(line_trees_consts_t const &c, line_trees_in_t const &in, uint32_t tile) {
	line_tree_box_t b;
	for (int k = 0; k < 6; ++k) {b.bc[k] = 0.0f;}
	b.nvalid = 0u; b.pad = 0u;
	uint32_t const cnt = line_trees_count(c, in, tile);
	bool any = false;
	tree_view_rec_t rec;
	for (uint32_t j = 0; j < cnt; ++j) {
		if (!line_trees_rec(c, in, tile, j, rec)) continue;
		++b.nvalid;
		float d[6];
		if (!tree_view_bounds(rec, d)) continue;
		if (!any) {for (int k = 0; k < 6; ++k) {b.bc[k] = d[k];} any = true;}
		else {box_union(b.bc, d);}
	}
	return b;
}
// v - xlate, per component
TERRA_HD void line_trees_local(line_trees_consts_t const &c, shadow_pt_t v, float o[3]) {o[0] = v.x - c.pv.a.offx; o[1] = v.y - c.pv.a.offy; o[2] = v.z - 0.0f;}
// the gate of small_tree_group::line_intersect: false -> return 0
TERRA_HD bool line_trees_gate(line_tree_box_t const &b, float const p1[3], float const p2[3]) {
	if (b.bc[0] == b.bc[1] || b.bc[2] == b.bc[3] || b.bc[4] == b.bc[5]) return true; // is_zero_area(): no cull
	float const d[3][2] = {{b.bc[0], b.bc[1]}, {b.bc[2], b.bc[3]}, {b.bc[4], b.bc[5]}};
	shadow_pt_t a = {p1[0], p1[1], p1[2]}, e = {p2[0], p2[1], p2[2]};
	return shadow_line_clip(a, e, d); // check_line_clip
}
// one record against the line: its t below 1.0 and the part, or false
TERRA_HD bool line_trees_test(line_trees_consts_t const &c, line_trees_in_t const &in, uint32_t tile, uint32_t j, float const p1[3], float const p2[3], float &t, uint32_t &part) {
	tree_view_rec_t rec;
	if (!line_trees_rec(c, in, tile, j, rec)) return false;
	t = 1.0f; part = 0u;
	return line_small_tree(c.pv.a, rec, p1, p2, t, part);
}
// small_tree_group::line_intersect over a tile's records in order, *t starting at the caller's tn
TERRA_HD bool line_trees_tile_literal(line_trees_consts_t const &c, line_trees_in_t const &in, uint32_t tile, line_tree_box_t const &b, shadow_pt_t v1, shadow_pt_t v2,
	float &t, int32_t &tree, uint32_t &part)
{
	float p1[3], p2[3];
	line_trees_local(c, v1, p1); line_trees_local(c, v2, p2);
	if (!line_trees_gate(b, p1, p2)) return false;
	uint32_t const cnt = line_trees_count(c, in, tile);
	bool coll = false;
	tree_view_rec_t rec;
	for (uint32_t j = 0; j < cnt; ++j) {
		uint32_t pt = 0u;
		if (line_trees_rec(c, in, tile, j, rec) && line_small_tree(c.pv.a, rec, p1, p2, t, pt)) {coll = true; tree = (int32_t)j; part = pt;}
	}
	return coll;
}

TERRA_HD line_tree_hit_pod_t line_tree_miss() {
	line_tree_hit_pod_t h; h.t = 2.0f; h.tile = -1; h.xpos = h.ypos = 0; h.p[0] = h.p[1] = h.p[2] = 0.0f; h.hit = LINE_HIT_NONE; h.tree = -1; h.part = 0u;
	return h;
}
TERRA_HD line_tree_hit_pod_t line_tree_hit_mesh(shadow_pt_t v1, shadow_pt_t v2, float t, uint32_t i, line_box_t const &b, int ix, int iy) {
	line_hit_pod_t const m = line_hit_make(v1, v2, t, i, b, ix, iy);
	line_tree_hit_pod_t h; h.t = m.t; h.tile = m.tile; h.xpos = m.xpos; h.ypos = m.ypos; h.p[0] = m.p[0]; h.p[1] = m.p[1]; h.p[2] = m.p[2]; h.hit = LINE_HIT_MESH; h.tree = -1; h.part = 0u;
	return h;
}
// a tree hit: new_xpos / new_ypos stay 0 in the reference; p_int from the untranslated ends
TERRA_HD line_tree_hit_pod_t line_tree_hit_tree(shadow_pt_t v1, shadow_pt_t v2, float t, uint32_t i, int32_t tree, uint32_t part) {
	line_tree_hit_pod_t h; h.t = t; h.tile = (int32_t)i; h.xpos = h.ypos = 0;
	h.p[0] = v1.x + t*(v2.x - v1.x); h.p[1] = v1.y + t*(v2.y - v1.y); h.p[2] = v1.z + t*(v2.z - v1.z);
	h.hit = LINE_HIT_TREE; h.tree = tree; h.part = part;
	return h;
}
// one line against the batch, the reference's loops: tile_draw_t::line_intersect_mesh over tile_t::line_intersect_mesh with inc_trees != 0
TERRA_HD line_tree_hit_pod_t line_trees_query_literal(line_trees_consts_t const &c, line_trees_in_t const &in, float const *zvals, line_box_t const *boxes, line_tree_box_t const *tboxes,
	uint32_t n, shadow_pt_t v1, shadow_pt_t v2, int32_t only)
{
	uint32_t i0, i1;
	line_tile_range(only, n, line_finite(v1, v2), i0, i1);
	size_t const zn = (size_t)(c.q.S + 2)*(c.q.S + 2);
	line_tree_hit_pod_t h = line_tree_miss();
	for (uint32_t i = i0; i < i1; ++i) {
		line_box_t const b = boxes[i];
		if (b.d[2][0] > b.d[2][1]) continue; // a distant tile (k_line_boxes' mark): returns 0 before the trees (:2178)
		float tn = 1.0f; int ix = 0, iy = 0;
		if (line_tile_hit(c.q, b, v1, v2, zvals + i*zn, tn, ix, iy)) {
			if (tn < h.t) {h = line_tree_hit_mesh(v1, v2, tn, i, b, ix, iy);}
			continue;
		}
		if (!tboxes || tboxes[i].nvalid == 0u) continue; // pine_trees.empty()
		int32_t tree = -1; uint32_t part = 0u;
		if (line_trees_tile_literal(c, in, i, tboxes[i], v1, v2, tn, tree, part) && tn < h.t) {h = line_tree_hit_tree(v1, v2, tn, i, tree, part);}
	}
	return h;
}

} // namespace terra
