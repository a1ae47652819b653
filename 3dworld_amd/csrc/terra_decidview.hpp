// terra_decidview.hpp -- the deciduous tree draw lists of a tile batch for a camera: tile_t::draw_decid_trees (src/tiled_mesh.cpp:1555-1563) without its GL and
// shader calls, tree_cont_t::draw_branches_and_leaves (src/Tree.cpp:312-368), tree::draw_leaves_top (:993-1052), tree::draw_branches_top (:948-990),
// tree::is_visible_to_camera (:858-861), tree::calc_size_scale (:919-928), tree_data_t::get_size_scale_mult (:930), the counts of tree_data_t::draw_leaves
// (:1182-1188) and draw_branches (:1128-1140), tree_cont_t::calc_bcube (:2458-2461) with tree::add_bounds_to_bcube (:862-865), get_draw_tile_dist
// (src/tiled_mesh.cpp:117) and cube_t::is_zero_area (src/3DWorld.h:491-527).  The sphere and cube tests (cube_visible_likely, closest_dist_less_than), InvSqrt
// and the box unions are terra_view.hpp's, unsigned(double) terra_common.hpp's d2u_x86.
//
// Tiled-terrain mode throughout: sphere_in_camera_view(.., 0 or 2) is sphere_visible_test alone (src/visibility.cpp:338-339), so ztop / czmax are not read;
// wind_enabled and leaf_dynamic_en are 0; rot_angle, the world_space_offset uniform, bcolor, gen_leaf_color and update_leaf_cobj_color stay with the engine.
//
// The bodies are shared by the driver's simple form (one logical thread per tile, the reference's loops) and by k_decid_view (terra_kernels.hpp).  Every operand
// carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out; sums run in the reference's order.
//
// One deviation: the billboard lists are ordered by tree_id and, within an id, by the order in which the reference adds the entries.  tree_lod_render_t::finalize
// sorts all tiles' entries with a comparison that looks at the tree_data_t pointer alone, so its order inside one tree's run is whatever introsort leaves.
#pragma once
#include "terra_view.hpp"
#include "terra_decidplace.hpp"
#include "terra_landscape.hpp" // min_u32
#include <stdexcept>

namespace terra {

constexpr uint32_t DECID_VIEW_LDS_KEYS = 2048; // the pairs of a tile that k_decid_view ranks in LDS; a larger capacity ranks in the tile's part of the driver's scratch
constexpr uint32_t DECID_VIEW_LDS_IDS  = 1024; // the table that k_decid_view's histogram holds in LDS; a larger table takes the ranking path
constexpr uint32_t DECID_VIEW_RANK_MAX = 512;  // the billboard entries of a tile that k_decid_view places by rank; more take the histogram
enum {DCV_GENERATED = 1, DCV_HAS_4TH = 2, DCV_LEAF_TEX = 4, DCV_BRANCH_TEX = 8};                                       // terra_decid_tree_data.flags
enum {DCV_TILE_DRAWN = 1, DCV_TILE_LEAVES = 2, DCV_TILE_BRANCHES = 4, DCV_TILE_SORTED = 8, DCV_TILE_BCUBE_ZERO_AREA = 16}; // terra_decid_view_tile.flags
enum {DCV_FORM_NONE = 0, DCV_FORM_GEOM = 1, DCV_FORM_BOTH = 2, DCV_FORM_BILLBOARD = 3, DCV_FORM_MASK = 3, DCV_NOT_VISIBLE = 4, DCV_LOW_DETAIL = 8, DCV_STAGE_SHIFT = 4,
      DCV_STAGE_NONE = 0, DCV_STAGE_NOT_VISIBLE = 1, DCV_STAGE_NO_LEAVES = 2, DCV_STAGE_BOX = 3, DCV_STAGE_SIZE = 4, DCV_STAGE_SHADOW_DIST = 5, DCV_STAGE_SHADOW_SPHERE = 6};

struct decid_view_args_pod_t {float behind_sphere_mult, zoom_f, lod_scales[4]; int32_t shadow_pass, reflection_pass, billboards, leaf_color_changed, draw_leaves, draw_branches;}; // terra_decid_view_args
struct decid_tree_data_pod_t {float base_radius, sphere_radius, sphere_center_zoff, lr_z_cent, leaves_bcube[6], branches_bcube[6]; uint32_t num_leaves, num_branch_quads, flags, pad;}; // terra_decid_tree_data
struct decid_view_tile_pod_t {uint32_t flags, num_trees, leaf_written, branch_written, leaf_bb_written, branch_bb_written, pad[2];}; // terra_decid_view_tile
struct decid_view_bb_pod_t {uint32_t tree_id, rec; float pos[3], opacity;};                                                        // terra_decid_view_bb

struct decid_view_consts_t {
	view_pod_t v;
	float behind_sphere_mult;
	float offx, offy;             // xlate = dtree_off.get_xlate()
	float lcx, lcy, lcz;          // local_camera = get_camera_pos() - xlate (:346)
	float scene_sum;              // the float that 1.0*(X_SCENE_SIZE + Y_SCENE_SIZE) narrows to (:349)
	float dmax;                   // get_draw_tile_dist() = DRAW_DIST_TILES*(TILE_RADIUS*get_tile_width())
	float zoom_f, lod[4];
	int shadow, reflection, billboards, lcc, leaves, branches;
	uint32_t num_data, cap;
};
inline decid_view_consts_t decid_view_consts(view_pod_t const &v, decid_view_args_pod_t const &a, float xss, float yss, float offx, float offy, uint32_t num_data, uint32_t cap) {
	decid_view_consts_t c;
	c.v = v; c.behind_sphere_mult = a.behind_sphere_mult; c.offx = offx; c.offy = offy;
	c.lcx = v.pos[0] - offx; c.lcy = v.pos[1] - offy; c.lcz = v.pos[2] - 0.0f;
	float const tile_width = xss + yss, DRAW_DIST_TILES = 1.5f; // src/tiled_mesh.h:93, src/tiled_mesh.cpp:23
	c.scene_sum = (float)(1.0*(double)tile_width);
	c.dmax = DRAW_DIST_TILES*((float)6*tile_width);              // TILE_RADIUS = 6 (src/tiled_mesh.h:24)
	c.zoom_f = a.zoom_f;
	for (int k = 0; k < 4; ++k) {c.lod[k] = a.lod_scales[k];}
	c.shadow = a.shadow_pass ? 1 : 0; c.reflection = a.reflection_pass; c.billboards = (a.billboards && !a.shadow_pass) ? 1 : 0; // enable_billboards (src/tiled_mesh.cpp:3262)
	c.lcc = a.leaf_color_changed ? 1 : 0; c.leaves = a.draw_leaves ? 1 : 0; c.branches = a.draw_branches ? 1 : 0;
	c.num_data = num_data; c.cap = cap;
	return c;
}
TERRA_HD bool decid_view_args_finite(decid_view_args_pod_t const &a) {
	return isfinite(a.behind_sphere_mult) && isfinite(a.zoom_f) && isfinite(a.lod_scales[0]) && isfinite(a.lod_scales[1]) && isfinite(a.lod_scales[2]) && isfinite(a.lod_scales[3]);
}

// ---- a record with its table entry.  false: dropped (tree_id outside the table, or the entry is not GENERATED): not drawn, not in all_bcube
TERRA_HD bool decid_view_valid(uint32_t num_data, decid_tree_data_pod_t const *data, decid_place_pod_t const &r) {
	return r.tree_id >= 0 && (uint32_t)r.tree_id < num_data && (data[r.tree_id].flags & DCV_GENERATED) != 0;
}
TERRA_HD bool decid_view_valid(decid_view_consts_t const &c, decid_tree_data_pod_t const *data, decid_place_pod_t const &r) {return decid_view_valid(c.num_data, data, r);}
// add_bounds_to_bcube's two boxes: branches_bcube + tree_center and leaves_bcube + tree_center (cube_t::operator+ adds the point to both bounds)
TERRA_HD void decid_view_bounds(decid_tree_data_pod_t const &td, float const pos[3], float b[6], float l[6]) {
	for (int k = 0; k < 6; ++k) {b[k] = td.branches_bcube[k] + pos[k >> 1]; l[k] = td.leaves_bcube[k] + pos[k >> 1];}
}
// calc_bcube as a union.  Tree after tree the reference runs assign_or_union_with_cube(B) -- a B of all zeros is ignored, an all_bcube of all zeros is replaced --
// and then union_with_cube(L).  With k the first tree whose B or L is not all zeros: all_bcube is the min / max union of every B that is not all zeros and of every
// L from tree k on, and of the zero cube when B_k is all zeros (L_k met a zero all_bcube) or some L from tree k on is all zeros.  The sweep reduces, beside the two
// unions, first = min over those trees of 2*i + (B_i all zeros), and last_zero = max i + 1 over the trees whose L is all zeros.
struct decid_view_union_t {float b[6], l[6]; uint32_t first, last_zero;}; // b: the B's that count; l: the L's that are not all zeros
TERRA_HD void decid_view_union_init(decid_view_union_t &u) {
	float const INF = __builtin_inff();
	for (int k = 0; k < 6; k += 2) {u.b[k] = u.l[k] = INF; u.b[k + 1] = u.l[k + 1] = -INF;}
	u.first = 0xFFFFFFFFu; u.last_zero = 0u;
}
TERRA_HD void decid_view_union_add(decid_view_union_t &u, uint32_t i, float const b[6], float const l[6]) {
	bool const bz = box_all_zeros(b), lz = box_all_zeros(l);
	if (!bz) {for (int k = 0; k < 6; k += 2) {u.b[k] = min_std(u.b[k], b[k]); u.b[k + 1] = max_std(u.b[k + 1], b[k + 1]);}}
	if (!lz) {for (int k = 0; k < 6; k += 2) {u.l[k] = min_std(u.l[k], l[k]); u.l[k + 1] = max_std(u.l[k + 1], l[k + 1]);}}
	else {u.last_zero = (u.last_zero < i + 1u) ? i + 1u : u.last_zero;}
	if (!bz || !lz) {uint32_t const f = 2u*i + (bz ? 1u : 0u); u.first = (f < u.first) ? f : u.first;}
}
TERRA_HD void decid_view_union_merge(decid_view_union_t &u, decid_view_union_t const &o) {
	for (int k = 0; k < 6; k += 2) {
		u.b[k] = min_std(u.b[k], o.b[k]); u.b[k + 1] = max_std(u.b[k + 1], o.b[k + 1]);
		u.l[k] = min_std(u.l[k], o.l[k]); u.l[k + 1] = max_std(u.l[k + 1], o.l[k + 1]);
	}
	u.first = (o.first < u.first) ? o.first : u.first; u.last_zero = (u.last_zero < o.last_zero) ? o.last_zero : u.last_zero;
}
TERRA_HD void decid_view_union_result(decid_view_union_t const &u, float bc[6]) {
	if (u.first == 0xFFFFFFFFu) {for (int k = 0; k < 6; ++k) {bc[k] = 0.0f;} return;} // every box is all zeros
	bool const zero = (u.first & 1u) != 0 || u.last_zero > (u.first >> 1);
	for (int k = 0; k < 6; k += 2) {
		float lo = min_std(u.b[k], u.l[k]), hi = max_std(u.b[k + 1], u.l[k + 1]);
		if (zero) {lo = min_std(lo, 0.0f); hi = max_std(hi, 0.0f);}
		bc[k] = lo; bc[k + 1] = hi;
	}
}

// ---- the tile-level decisions: the cull of :316 and the choice of :347-348
struct decid_view_tile_t {uint32_t flags; int drawn, sorted;};
TERRA_HD decid_view_tile_t decid_view_tile(decid_view_consts_t const &c, float const bc[6]) {
	decid_view_tile_t o;
	bool const zero_area = bc[0] == bc[1] || bc[2] == bc[3] || bc[4] == bc[5];
	float const xb[3][2] = {{bc[0] + c.offx, bc[1] + c.offx}, {bc[2] + c.offy, bc[3] + c.offy}, {bc[4] + 0.0f, bc[5] + 0.0f}}; // all_bcube + xlate
	o.drawn = (zero_area || view_cube_visible(c.v, xb)) ? 1 : 0;
	o.flags = zero_area ? (uint32_t)DCV_TILE_BCUBE_ZERO_AREA : 0u;
	o.sorted = 0;
	if (!o.drawn) return o;
	o.flags |= DCV_TILE_DRAWN | (c.leaves ? (uint32_t)DCV_TILE_LEAVES : 0u) | (c.branches ? (uint32_t)DCV_TILE_BRANCHES : 0u);
	if (c.leaves && !c.shadow) { // direct draw: !all_bcube.is_all_zeros() && !all_bcube.closest_dist_less_than(local_camera, 1.0*(X_SCENE_SIZE + Y_SCENE_SIZE))
		float const d[3][2] = {{bc[0], bc[1]}, {bc[2], bc[3]}, {bc[4], bc[5]}};
		bool const direct = !box_all_zeros(bc) && !view_closest_dist_less_than(d, c.lcx, c.lcy, c.lcz, c.scene_sum);
		o.sorted = direct ? 0 : 1;
	}
	if (o.sorted) {o.flags |= DCV_TILE_SORTED;}
	return o;
}

// ---- what both sweeps read of a tree: sphere_center(), draw_pos = sphere_center() + xlate, tree_xlate = tree_center + xlate
struct decid_view_tree_t {float scx, scy, scz, dx, dy, dz, tx, ty, tz;};
TERRA_HD decid_view_tree_t decid_view_tree(decid_view_consts_t const &c, decid_tree_data_pod_t const &td, float const pos[3]) {
	decid_view_tree_t o;
	o.scx = pos[0] + 0.0f; o.scy = pos[1] + 0.0f; o.scz = pos[2] + td.sphere_center_zoff; // tree_center + point(0.0, 0.0, sphere_center_zoff)
	o.dx = o.scx + c.offx; o.dy = o.scy + c.offy; o.dz = o.scz + 0.0f;
	o.tx = pos[0] + c.offx; o.ty = pos[1] + c.offy; o.tz = pos[2] + 0.0f;
	return o;
}
// !is_visible_to_camera(xlate) (:858-861)
TERRA_HD bool decid_view_not_visible(decid_view_consts_t const &c, decid_tree_data_pod_t const &td, decid_view_tree_t const &g) {
	return !view_sphere_visible(c.v, c.behind_sphere_mult, g.dx, g.dy, g.dz, (float)(1.1*(double)td.sphere_radius));
}
// camera_pdu.cube_visible_likely(box + tree_xlate)
TERRA_HD bool decid_view_cube_likely(decid_view_consts_t const &c, float const box[6], decid_view_tree_t const &g) {
	if (!c.v.valid) return true; // an invalid view reads no box
	float const d[3][2] = {{box[0] + g.tx, box[1] + g.tx}, {box[2] + g.ty, box[3] + g.ty}, {box[4] + g.tz, box[5] + g.tz}};
	return view_cube_visible_likely(c.v, d);
}
// calc_size_scale(draw_pos) (:919-928)
TERRA_HD float decid_view_size_scale(decid_view_consts_t const &c, decid_tree_data_pod_t const &td, decid_view_tree_t const &g) {
	float const *cam = c.v.pos;
	float const dist_sq = (cam[0] - g.dx)*(cam[0] - g.dx) + (cam[1] - g.dy)*(cam[1] - g.dy) + (cam[2] - g.dz)*(cam[2] - g.dz); // distance_to_camera_sq
	if (dist_sq > c.dmax*c.dmax) return 0.0f; // too far away to draw
	return c.zoom_f*td.base_radius*inv_sqrt_ref(dist_sq)/0.01f; // DIST_C_SCALE (src/Tree.cpp:23)
}
// the tt_shadow_mode test of :325 and :338: dist_less_than(sphere_center() + xlate, camera_pdu.pos, camera_pdu.far_)
TERRA_HD bool decid_view_shadow_near(decid_view_consts_t const &c, decid_view_tree_t const &g) {
	float const *cam = c.v.pos;
	return (g.dx - cam[0])*(g.dx - cam[0]) + (g.dy - cam[1])*(g.dy - cam[1]) + (g.dz - cam[2])*(g.dz - cam[2]) < c.v.far_*c.v.far_;
}
TERRA_HD double decid_view_scale_mult(decid_tree_data_pod_t const &td) {return (double)((td.flags & DCV_HAS_4TH) ? 0.4f : 1.0f);} // get_size_scale_mult(): LEAF_4TH_SCALE
// nl of tree_data_t::draw_leaves(size_scale) (:1182-1188), ENABLE_CLIP_LEAVES = 1
TERRA_HD uint32_t decid_view_leaf_num(decid_tree_data_pod_t const &td, float size_scale) {
	uint32_t nl = td.num_leaves;
	if ((double)size_scale > 0.0) {
		uint32_t const q = d2u_x86(4.0*(double)nl*(double)size_scale*decid_view_scale_mult(td)), lo = nl/8u, m = (lo < q) ? q : lo;
		nl = (m < nl) ? m : nl;
	}
	return nl;
}
// num and low_detail of tree_data_t::draw_branches(size_scale, force_low_detail, shadow_pass) (:1128-1140)
TERRA_HD uint32_t decid_view_branch_num(decid_tree_data_pod_t const &td, float size_scale, bool force_low_detail, bool shadow_pass, bool &low_detail) {
	uint32_t const nbq = td.num_branch_quads;
	uint32_t num = nbq;
	if (!((double)size_scale == 0.0)) {
		uint32_t const q = d2u_x86(1.5*(double)nbq*(double)size_scale*decid_view_scale_mult(td)), lo = nbq/40u, m = (lo < q) ? q : lo;
		num = (m < nbq) ? m : nbq;
	}
	low_detail = force_low_detail || ((double)size_scale > 0.0 && (double)size_scale < 2.0);
	if (!shadow_pass && (td.flags & DCV_HAS_4TH) && num > nbq/5u) {low_detail = false;}
	return num;
}
// the billboard blend of :972-981 and :1026-1036: geom_opacity, and whether add_branches / add_leaves is called
TERRA_HD float decid_view_opacity(decid_view_consts_t const &c, bool tex_valid, float size_scale, float lod_start, float lod_end, bool &added) {
	added = false;
	float geom_opacity = 1.0f;
	if (!c.billboards) return geom_opacity;
	float const lod_denom = lod_start - lod_end;
	if (tex_valid && size_scale < lod_start) {
		geom_opacity = ((double)lod_denom == 0.0) ? 0.0f : clip01((size_scale - lod_end)/lod_denom);
		added = true;
	}
	return geom_opacity;
}
// one sweep's result for a record
struct decid_view_rec_t {uint32_t word, num; float scale, opacity; int listed, added;};
TERRA_HD uint32_t decid_view_form(float geom_opacity, bool added) {return ((double)geom_opacity == 0.0) ? DCV_FORM_BILLBOARD : (added ? DCV_FORM_BOTH : DCV_FORM_GEOM);}
// tree::draw_leaves_top behind the loops of :335-361.  not_visible: in: unused; out: tree::not_visible where :1017 assigns it (wrote_nv)
TERRA_HD decid_view_rec_t decid_view_leaves(decid_view_consts_t const &c, decid_tree_data_pod_t const &td, decid_view_tree_t const &g, bool &not_visible, bool &wrote_nv) {
	decid_view_rec_t o; o.word = 0u; o.num = 0u; o.scale = 0.0f; o.opacity = 0.0f; o.listed = 0; o.added = 0;
	wrote_nv = false;
	auto leave = [&](uint32_t stage) {o.word |= stage << DCV_STAGE_SHIFT; return o;};
	if (c.shadow) {
		if (!decid_view_shadow_near(c, g)) return leave(DCV_STAGE_SHADOW_DIST);
		if (!view_sphere_visible(c.v, c.behind_sphere_mult, g.dx, g.dy, g.dz, (float)(1.1*(double)td.sphere_radius))) return leave(DCV_STAGE_SHADOW_SPHERE);
		if (td.num_leaves == 0u) return leave(DCV_STAGE_NO_LEAVES); // draw_leaves_shadow_only: leaves.empty()
		o.scale = 0.5f; o.opacity = 1.0f; o.num = decid_view_leaf_num(td, 0.5f); o.word = DCV_FORM_GEOM; o.listed = 1;
		return o;
	}
	not_visible = decid_view_not_visible(c, td, g); wrote_nv = true;
	if (not_visible) {o.word |= DCV_NOT_VISIBLE;}
	if (not_visible && !c.lcc) return leave(DCV_STAGE_NOT_VISIBLE);
	if (td.num_leaves == 0u) return leave(DCV_STAGE_NO_LEAVES);
	if (!c.lcc && !decid_view_cube_likely(c, td.leaves_bcube, g)) return leave(DCV_STAGE_BOX);
	float const size_scale = decid_view_size_scale(c, td, g);
	o.scale = size_scale;
	if ((double)size_scale == 0.0) return leave(DCV_STAGE_SIZE);
	bool added;
	float const geom_opacity = decid_view_opacity(c, (td.flags & DCV_LEAF_TEX) != 0, size_scale, c.lod[2], c.lod[3], added);
	o.opacity = geom_opacity; o.added = added ? 1 : 0; o.word |= decid_view_form(geom_opacity, added);
	if ((double)geom_opacity == 0.0) return o;
	o.num = decid_view_leaf_num(td, size_scale); o.listed = 1;
	return o;
}
// tree::draw_branches_top behind the loop of :324-327
TERRA_HD decid_view_rec_t decid_view_branches(decid_view_consts_t const &c, decid_tree_data_pod_t const &td, decid_view_tree_t const &g, bool not_visible) {
	decid_view_rec_t o; o.word = 0u; o.num = 0u; o.scale = 0.0f; o.opacity = 0.0f; o.listed = 0; o.added = 0;
	auto leave = [&](uint32_t stage) {o.word |= stage << DCV_STAGE_SHIFT; return o;};
	if (c.shadow && !decid_view_shadow_near(c, g)) return leave(DCV_STAGE_SHADOW_DIST);
	if (!c.shadow && not_visible) {o.word |= DCV_NOT_VISIBLE; return leave(DCV_STAGE_NOT_VISIBLE);}
	if (!decid_view_cube_likely(c, td.branches_bcube, g)) return leave(DCV_STAGE_BOX);
	bool low_detail;
	if (c.shadow) { // td.draw_branches(1.0, 1, 1)
		o.scale = 1.0f; o.opacity = 1.0f; o.num = decid_view_branch_num(td, 1.0f, true, true, low_detail);
		o.word = DCV_FORM_GEOM | (low_detail ? (uint32_t)DCV_LOW_DETAIL : 0u); o.listed = 1;
		return o;
	}
	float const size_scale = decid_view_size_scale(c, td, g);
	o.scale = size_scale;
	if ((double)size_scale < 0.05) return leave(DCV_STAGE_SIZE);
	bool added;
	float const geom_opacity = decid_view_opacity(c, (td.flags & DCV_BRANCH_TEX) != 0, size_scale, c.lod[0], c.lod[1], added);
	o.opacity = geom_opacity; o.added = added ? 1 : 0; o.word |= decid_view_form(geom_opacity, added);
	if ((double)geom_opacity == 0.0) return o;
	o.num = decid_view_branch_num(td, size_scale, c.reflection != 0, false, low_detail); o.listed = 1;
	if (low_detail) {o.word |= DCV_LOW_DETAIL;}
	return o;
}
// the entry add_leaves (LEAVES) / add_branches receives: (1.0 - geom_opacity) narrows to the float parameter
template<bool LEAVES> TERRA_HD decid_view_bb_pod_t decid_view_bb(decid_tree_data_pod_t const &td, decid_view_tree_t const &g, uint32_t tree_id, uint32_t rec, float geom_opacity) {
	decid_view_bb_pod_t e;
	e.tree_id = tree_id; e.rec = rec;
	e.pos[0] = LEAVES ? g.dx + 0.0f : g.dx; e.pos[1] = LEAVES ? g.dy + 0.0f : g.dy; e.pos[2] = LEAVES ? g.dz + (td.lr_z_cent - td.sphere_center_zoff) : g.dz;
	e.opacity = (float)(1.0 - (double)geom_opacity);
	return e;
}
// p2p_dist_sq(sphere_center(), local_camera) (:356)
TERRA_HD float decid_view_sort_key(decid_view_consts_t const &c, decid_view_tree_t const &g) {
	return (g.scx - c.lcx)*(g.scx - c.lcx) + (g.scy - c.lcy)*(g.scy - c.lcy) + (g.scz - c.lcz)*(g.scz - c.lcz);
}
// std::pair<float, unsigned>'s operator<
TERRA_HD bool decid_view_before(float da, uint32_t ia, float db, uint32_t ib) {return da < db || (!(db < da) && ia < ib);}

// ---- the arrays of a call, in the order of terra_tiles_decid_view[_dev]: host pointers in the host form's first record, device pointers everywhere else
struct decid_view_io_t {
	decid_tree_data_pod_t const *data; uint8_t const *skip; decid_place_pod_t const *decid; uint32_t const *counts;
	uint8_t *not_visible; decid_view_tile_pod_t *tile_out; float *bcube;
	uint32_t *leaf_word; float *leaf_scale, *leaf_opacity; uint32_t *leaf_num, *branch_word; float *branch_scale, *branch_opacity; uint32_t *branch_num;
	uint32_t *leaf_list, *branch_list; decid_view_bb_pod_t *leaf_bb, *branch_bb; uint32_t *list_counts;
};
// the argument rules of a call, behind decid_view_check: throws what the call refuses; false: nothing to do (n == 0).  The table is required and the alignment
// is looked at for an empty batch too.  dev: the arrays are the device's
inline bool decid_view_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, decid_view_io_t const &io, bool dev) {
	if (!io.data) throw std::invalid_argument("tiles_decid_view: null argument");
	if ((uint64_t)n*capacity > 0xFFFFFFFFull) throw std::invalid_argument("tiles_decid_view: n*capacity must fit 32 bits");
	if (n && (!tile_xy || !io.counts || !io.tile_out || !io.bcube || !io.list_counts)) throw std::invalid_argument("tiles_decid_view: null argument");
	if (n && capacity && (!io.decid || !io.leaf_word || !io.leaf_scale || !io.leaf_opacity || !io.leaf_num || !io.branch_word || !io.branch_scale || !io.branch_opacity ||
	                      !io.branch_num || !io.leaf_list || !io.branch_list || !io.leaf_bb || !io.branch_bb)) throw std::invalid_argument("tiles_decid_view: null argument");
	if (dev && (((uintptr_t)io.data | (uintptr_t)io.decid | (uintptr_t)io.counts | (uintptr_t)io.tile_out | (uintptr_t)io.bcube | (uintptr_t)io.leaf_word | (uintptr_t)io.leaf_scale |
	             (uintptr_t)io.leaf_opacity | (uintptr_t)io.leaf_num | (uintptr_t)io.branch_word | (uintptr_t)io.branch_scale | (uintptr_t)io.branch_opacity | (uintptr_t)io.branch_num |
	             (uintptr_t)io.leaf_list | (uintptr_t)io.branch_list | (uintptr_t)io.leaf_bb | (uintptr_t)io.branch_bb | (uintptr_t)io.list_counts) & 3u) != 0) {
		throw std::invalid_argument("tiles_decid_view: every array but skip and not_visible must be 4-byte aligned");
	}
	return n != 0;
}

// ---- the literal body: tile t of the batch, its records walked in the reference's order, the leaves sweep before the branches sweep
TERRA_HD void decid_view_tile_literal(decid_view_consts_t const &c, decid_view_io_t const &io, size_t t) {
	decid_tree_data_pod_t const *const data = io.data;
	uint32_t const cnt = (io.skip && io.skip[t]) ? 0u : min_u32(io.counts[t], c.cap);
	size_t const o = t*c.cap;
	decid_place_pod_t const *const recs = io.decid + o;
	// calc_bcube, literally
	float bc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	uint32_t nvalid = 0;
	for (uint32_t j = 0; j < cnt; ++j) {
		if (!decid_view_valid(c, data, recs[j])) continue;
		++nvalid;
		float b[6], l[6];
		decid_view_bounds(data[recs[j].tree_id], recs[j].pos, b, l);
		box_assign_or_union(bc, b);
		box_union(bc, l);
	}
	for (int k = 0; k < 6; ++k) {io.bcube[t*6 + k] = bc[k];}
	decid_view_tile_pod_t out; out.flags = 0u; out.num_trees = nvalid; out.leaf_written = out.branch_written = out.leaf_bb_written = out.branch_bb_written = out.pad[0] = out.pad[1] = 0u;
	uint32_t nl = 0, nb = 0, nlb = 0, nbb = 0;
	decid_view_tile_t tl; tl.flags = 0u; tl.drawn = 0; tl.sorted = 0;
	if (nvalid != 0u) {tl = decid_view_tile(c, bc);} // else: skipped, or decid_trees.empty() (:1557)
	out.flags = tl.flags;
	if (tl.drawn) {
		uint32_t *const ll = io.leaf_list + o, *const bl = io.branch_list + o;
		decid_view_bb_pod_t *const lb = io.leaf_bb + o, *const bb = io.branch_bb + o;
		auto insert = [&](decid_view_bb_pod_t *list, uint32_t &m, decid_view_bb_pod_t const &e) { // behind every entry with an id that is not larger
			uint32_t k = m++;
			for (; k > 0 && list[k - 1].tree_id > e.tree_id; --k) {list[k] = list[k - 1];}
			list[k] = e;
		};
		if (c.leaves) {
			// the sequence of the sweep: the valid records in record order, or ascending (p2p_dist_sq, index) (:355-357).  No array holds it (the outputs keep
			// their bytes where the call writes no entry): the sorted walk selects, step after step, the smallest pair behind the one before
			auto key_of = [&](uint32_t q) {return decid_view_sort_key(c, decid_view_tree(c, data[recs[q].tree_id], recs[q].pos));};
			float prev_key = 0.0f; uint32_t prev = 0; bool first = true;
			for (uint32_t p = 0, rj = 0; p < nvalid; ++p) {
				uint32_t j = 0;
				if (!tl.sorted) {
					while (!decid_view_valid(c, data, recs[rj])) {++rj;}
					j = rj++;
				}
				else {
					bool have = false; float best = 0.0f;
					for (uint32_t q = 0; q < cnt; ++q) {
						if (!decid_view_valid(c, data, recs[q])) continue;
						float const k = key_of(q);
						if (!first && !tree_view_before_f(prev_key, prev, k, q)) continue;
						if (!have || tree_view_before_f(k, q, best, j)) {have = true; best = k; j = q;}
					}
					prev_key = best; prev = j; first = false;
				}
				decid_tree_data_pod_t const td = data[recs[j].tree_id];
				decid_view_tree_t const g = decid_view_tree(c, td, recs[j].pos);
				bool nvis = false, wrote = false;
				decid_view_rec_t const r = decid_view_leaves(c, td, g, nvis, wrote);
				io.leaf_word[o + j] = r.word; io.leaf_scale[o + j] = r.scale; io.leaf_opacity[o + j] = r.opacity; io.leaf_num[o + j] = r.num;
				if (wrote && io.not_visible) {io.not_visible[o + j] = nvis ? 1 : 0;}
				if (r.added) {insert(lb, nlb, decid_view_bb<true>(td, g, (uint32_t)recs[j].tree_id, j, r.opacity));}
				if (r.listed) {ll[nl++] = j;}
			}
		}
		if (c.branches) {
			for (uint32_t j = 0; j < cnt; ++j) {
				if (!decid_view_valid(c, data, recs[j])) continue;
				decid_tree_data_pod_t const td = data[recs[j].tree_id];
				decid_view_tree_t const g = decid_view_tree(c, td, recs[j].pos);
				bool nvis = false;
				if (!c.shadow) {nvis = c.leaves ? (io.leaf_word[o + j] & DCV_NOT_VISIBLE) != 0 : (io.not_visible && io.not_visible[o + j] != 0);}
				decid_view_rec_t const r = decid_view_branches(c, td, g, nvis);
				io.branch_word[o + j] = r.word; io.branch_scale[o + j] = r.scale; io.branch_opacity[o + j] = r.opacity; io.branch_num[o + j] = r.num;
				if (r.added) {insert(bb, nbb, decid_view_bb<false>(td, g, (uint32_t)recs[j].tree_id, j, r.opacity));}
				if (r.listed) {bl[nb++] = j;}
			}
		}
		out.leaf_written = nl; out.branch_written = nb; out.leaf_bb_written = nlb; out.branch_bb_written = nbb; // (a list holds a record once: never more than the capacity)
	}
	io.tile_out[t] = out;
	io.list_counts[4*t] = nl; io.list_counts[4*t + 1] = nb; io.list_counts[4*t + 2] = nlb; io.list_counts[4*t + 3] = nbb;
}

} // namespace terra
