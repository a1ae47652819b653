// terra_treeview.hpp -- the pine and palm tree draw lists of a tile batch for a camera: tile_t::draw_pine_trees (src/tiled_mesh.cpp:1465-1526) without its GL and
// shader calls, draw_tree_leaves_lod (:1459-1462), the weights of update_pine_tree_state (:1440-1448), get_tree_dist_scale / get_tree_far_weight /
// get_tree_scale_denom / get_dist_to_camera_in_tiles (src/tiled_mesh.h:95,332-338), contains_camera (:264-265), small_tree_group::draw_tree_insts
// (src/sm_tree.cpp:242-279, up to the GL loop), draw_pine_leaves (:281-310), get_back_to_front_ordering (:233-240), draw_non_pine_leaves as called with (0, 1, 0, ..)
// (:312-323), draw_trunks (:206-224), calc_bcube / add_bounds_to_bcube (:176-179,832-838), small_tree::are_leaves_visible (:1007-1017), the decisions of
// small_tree::draw_trunk (:1081-1102, down to nsides), get_trunk_cylin (:767-777) with get_tree_z_bottom / get_default_tree_depth (src/Tree.cpp:209-214, the
// tiled-terrain branch), get_xy_radius / get_trunk_bsphere_radius (src/small_tree.h:77-78), stt[] (src/sm_tree.cpp:46-53) and the constants (src/tiled_mesh.h:
// 27-29; src/sm_tree.cpp:14; src/3DWorld.h:104; src/tree_3dw.h:10).  The size of a record is terra_treeao.hpp's small_tree_size, the tile's centre and box
// terra_terrainview.hpp's, the sphere, cube and point tests terra_view.hpp's, int(double) terra_common.hpp's d2i_x86.
//
// sphere_in_camera_view(.., 2) (are_leaves_visible's palm branch) is sphere_visible_test alone in tiled-terrain mode (src/visibility.cpp:338-339).
//
// The bodies are shared by the driver's simple form (one logical thread per tile, the reference's loops) and by k_tree_view (terra_kernels.hpp).  Every operand
// carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out; sums run in the reference's order.
//
// One deviation: the instance lists are ordered by (id, record index).  The reference calls std::sort on a comparison that looks at the id alone
// (tree_inst_t::operator<), so its order inside an id is whatever the library's introsort leaves; the instanced draw per id does not depend on it.  The
// front-to-back list of the tile that holds the camera is ordered by std::pair's operator< on (p2p_dist_sq, index), a total order: no deviation there.
#pragma once
#include "terra_view.hpp"
#include "terra_terrainview.hpp"
#include "terra_treeao.hpp"
#include <stdexcept>

namespace terra {

constexpr int T_BUSH = 3;                  // src/small_tree.h:9
constexpr int TREE_VIEW_CYL_SIDES = 32;    // N_CYL_SIDES (src/3DWorld.h:104)
constexpr uint32_t TREE_VIEW_LDS_KEYS = 2048; // the (key, record) pairs of a tile that k_tree_view ranks in LDS; a larger capacity ranks in global scratch
constexpr uint32_t TREE_VIEW_LDS_IDS = 1024;  // the instance table that k_tree_view's histogram holds in LDS; a larger table takes the ranking path
constexpr uint32_t TREE_VIEW_RANK_MAX = 512;  // the entries of an instance list that k_tree_view places by rank; more take the histogram
enum {TRV_TRUNK_NONE = 0, TRV_TRUNK_POLY_ALL = 1, TRV_TRUNK_POLY_SKIPPED = 2, TRV_TRUNK_POINTS = 3, TRV_TRUNK_MASK = 3, // :1477-1489
      TRV_NEAR_LEAVES = 0x4, TRV_FAR_LEAVES = 0x8, TRV_DITHERED = 0x10, TRV_PALMS = 0x20, TRV_DRAW_ALL_NEAR = 0x40, TRV_DRAW_ALL_FAR = 0x80, TRV_ALL_VISIBLE = 0x100,
      TRV_NEEDS_HIGH = 0x200, TRV_NEEDS_LOW = 0x400, TRV_CONTAINS_CAMERA = 0x800};

struct tree_view_args_pod_t {float behind_sphere_mult, zoom_f, tree_depth_scale; int32_t window_width, shadow_pass, draw_trunks, draw_near_leaves, draw_far_leaves;}; // terra_tree_view_args
struct tree_view_tile_pod_t {float dscale, weight; uint32_t flags, num_pine, num_palm, num_trees, leaf_written, pad;};  // terra_tree_view_tile
struct tree_view_inst_pod_t {uint32_t id; float pt[3];};                                          // terra_tree_view_inst: tree_inst_t
struct trunk_override_pod_t {float p1[3], p2[3], r1, r2; int32_t rotated;};                       // terra_trunk_override

struct tree_view_consts_t {
	terrain_view_consts_t tv;     // the view, behind_sphere_mult, the scene and the offsets: what the tile's centre and box read
	tree_ao_consts_t a;           // what small_tree_size reads; offx / offy are xlate = ptree_off.get_xlate()
	float denom;                  // get_tree_scale_denom() (src/tiled_mesh.h:95)
	float tree_depth;             // get_default_tree_depth() (src/Tree.cpp:209)
	float zoom_f, window_width;   // window_width: the int as the float that `float*int` makes of it
	int shadow_pass, draw_trunks, draw_near, draw_far;
	uint32_t cap;
};
inline tree_view_consts_t tree_view_consts(view_pod_t const &v, tree_view_args_pod_t const &a, tree_ao_consts_t const &ao, float xss, float yss, int dxoff, int dyoff, uint32_t cap)
{
	tree_view_consts_t c;
	terrain_view_args_pod_t const ta = {a.behind_sphere_mult, 0.0f, 0, 0, 0};
	c.tv = terrain_view_consts(v, ta, xss, yss, ao.dxv, ao.dyv, ao.S, dxoff, dyoff, 0.0f);
	c.a = ao;
	float const TREE_LOD_THRESH = 6.0f, TREE_DEPTH = 0.1f;
	c.denom = max_std(1.0f, TREE_LOD_THRESH*ao.tsize);
	c.tree_depth = (float)((double)(TREE_DEPTH*a.tree_depth_scale)*(0.5 + 0.5/(double)ao.tree_scale)); // TREE_DEPTH*tree_depth_scale*(0.5 + 0.5/tree_scale)
	c.zoom_f = a.zoom_f; c.window_width = (float)a.window_width;
	c.shadow_pass = a.shadow_pass ? 1 : 0; c.draw_trunks = a.draw_trunks ? 1 : 0; c.draw_near = a.draw_near_leaves ? 1 : 0; c.draw_far = a.draw_far_leaves ? 1 : 0;
	c.cap = cap;
	return c;
}
TERRA_HD bool tree_view_args_ok(tree_view_args_pod_t const &a) {
	return isfinite(a.behind_sphere_mult) && isfinite(a.zoom_f) && a.zoom_f > 0.0f && isfinite(a.tree_depth_scale) && a.tree_depth_scale > 0.0f && a.window_width > 0;
}

// stt[type].w2 / ws / ss (src/sm_tree.cpp:46-53): floats initialised from the double literals
TERRA_HD float stt_w2(int type) {return (type == 1 || type == 2) ? 0.13f : ((type == T_PALM) ? 0.03f : 0.0f);}
TERRA_HD float stt_ws(int type) {return (type == T_PINE) ? 0.14f : ((type == T_PALM) ? 0.12f : ((type == T_SH_PINE) ? 0.08f : 0.15f));}
TERRA_HD float stt_ss(int type) {return (type == T_PINE || type == T_SH_PINE) ? 0.4f : ((type == 2) ? 0.7f : ((type == T_PALM) ? 0.6f : 0.8f));}

// ---- a record as the small_tree constructors leave it: type, size, pos and trunk_cylin; rotated: r_angle != 0 (only through the caller's override)
struct tree_view_rec_t {int type; float height, width; float pos[3], p1[3], p2[3], r1, r2, dir[3]; int rotated;};
// false: no such tree (what the tree AO pass drops: a bad type, an instance outside the table, an instanced record while `instanced` is off)
TERRA_HD bool tree_view_record(tree_view_consts_t const &c, tree_inst_pod_t const *insts, tree_place_pod_t const &r, trunk_override_pod_t const *ov, tree_view_rec_t &o) {
	if (!small_tree_size(c.a, insts, r, o.type, o.height, o.width)) return false;
	for (int k = 0; k < 3; ++k) {o.pos[k] = r.pos[k];}
	o.rotated = 0; o.dir[0] = 0.0f; o.dir[1] = 0.0f; o.dir[2] = 1.0f; // get_rot_dir(): plus_z
	if (ov && ov->rotated) { // the constructor's setup_rotation stays with the engine: its cylinder, and get_rot_dir() = trunk_cylin.get_norm_dir_vect()
		for (int k = 0; k < 3; ++k) {o.p1[k] = ov->p1[k]; o.p2[k] = ov->p2[k];}
		o.r1 = ov->r1; o.r2 = ov->r2; o.rotated = 1;
		float const x = o.p2[0] - o.p1[0], y = o.p2[1] - o.p1[1], z = o.p2[2] - o.p1[2], vmag = sqrtf(x*x + y*y + z*z);
		if (vmag < 1.0E-12f) {o.dir[0] = x; o.dir[1] = y; o.dir[2] = z;} else {o.dir[0] = x/vmag; o.dir[1] = y/vmag; o.dir[2] = z/vmag;} // get_norm()
		return true;
	}
	if (o.type == T_BUSH) {for (int k = 0; k < 3; ++k) {o.p1[k] = 0.0f; o.p2[k] = 0.0f;} o.r1 = 0.0f; o.r2 = 0.0f; return true;} // cylinder_3dw()
	// get_trunk_cylin (:767-777) with dir = plus_z
	bool const is_pine = is_pine_tree_type(o.type);
	float const trunk_height = (float)((is_pine ? 1.05 : 0.8)*(double)o.height), zb = (float)((double)o.pos[2] - 0.2*(double)o.width);
	float const zbot = zb - c.tree_depth;                       // get_tree_z_bottom: world_mode != WMODE_GROUND
	float const len = trunk_height + (zb - zbot);
	float const base_rscale = (is_pine || o.type == T_PALM) ? 0.8f*len/trunk_height : 1.0f;
	float const s = zbot - o.pos[2];
	o.p1[0] = o.pos[0] + 0.0f*s; o.p1[1] = o.pos[1] + 0.0f*s; o.p1[2] = o.pos[2] + 1.0f*s;       // pos + dir*(zbot - pos.z)
	o.p2[0] = o.p1[0] + 0.0f*len; o.p2[1] = o.p1[1] + 0.0f*len; o.p2[2] = o.p1[2] + 1.0f*len;   // p1 + dir*len
	o.r1 = stt_ws(o.type)*o.width*base_rscale; o.r2 = stt_w2(o.type)*o.width;
	return true;
}
// get_xy_radius(): max(1.5*branch_xy_scale*width, 0.5*height), branch_xy_scale = 1.0f
TERRA_HD float tree_view_xy_radius(tree_view_rec_t const &r) {
	double const a = 1.5*(double)1.0f*(double)r.width, b = 0.5*(double)r.height;
	return (float)((a < b) ? b : a);
}
// add_bounds_to_bcube's bc (:833-836); false: all zeros (assign_or_union_with_cube ignores such a box)
TERRA_HD bool tree_view_bounds(tree_view_rec_t const &r, float d[6]) {
	float const cx = 0.5f*(r.p1[0] + r.p2[0]), cy = 0.5f*(r.p1[1] + r.p2[1]), xyr = tree_view_xy_radius(r);
	d[0] = cx - xyr; d[1] = cx + xyr; d[2] = cy - xyr; d[3] = cy + xyr; d[4] = r.p1[2]; d[5] = r.p2[2];
	return !box_all_zeros(d);
}
// are_leaves_visible(xlate); xlate = (offx, offy, 0).  (Written out per component: indexed locals would live in scratch memory on the device.)
TERRA_HD bool tree_view_leaves_visible(tree_view_consts_t const &c, tree_view_rec_t const &r) {
	float px, py, pz, radius;
	if (r.type == T_PALM) { // trunk_cylin.p2 - 0.2*width*get_rot_dir() + xlate, 0.3*height + 0.2*width
		double const q = 0.2*(double)r.width;
		px = (r.p2[0] - (float)(q*(double)r.dir[0])) + c.a.offx; py = (r.p2[1] - (float)(q*(double)r.dir[1])) + c.a.offy; pz = (r.p2[2] - (float)(q*(double)r.dir[2])) + 0.0f;
		radius = (float)(0.3*(double)r.height + 0.2*(double)r.width);
	}
	else if (!r.rotated) { // pos + vector3d(0.0, 0.0, 0.5*height) + xlate
		px = (r.pos[0] + 0.0f) + c.a.offx; py = (r.pos[1] + 0.0f) + c.a.offy; pz = (r.pos[2] + (float)(0.5*(double)r.height)) + 0.0f;
		radius = tree_view_xy_radius(r);
	}
	else { // pos + 0.5*height*get_rot_dir() + xlate
		double const h = 0.5*(double)r.height;
		px = (r.pos[0] + (float)(h*(double)r.dir[0])) + c.a.offx; py = (r.pos[1] + (float)(h*(double)r.dir[1])) + c.a.offy; pz = (r.pos[2] + (float)(h*(double)r.dir[2])) + 0.0f;
		radius = tree_view_xy_radius(r);
	}
	return view_sphere_visible(c.tv.v, c.tv.behind_sphere_mult, px, py, pz, radius);
}
// p2p_dist_sq(i->get_pos(), ref_pos), ref_pos = get_camera_pos() - xlate (:234-237)
TERRA_HD float tree_view_sort_key(tree_view_consts_t const &c, float const pos[3]) {
	float const *cam = c.tv.v.pos;
	float const rx = cam[0] - c.a.offx, ry = cam[1] - c.a.offy, rz = cam[2] - 0.0f;
	return (pos[0] - rx)*(pos[0] - rx) + (pos[1] - ry)*(pos[1] - ry) + (pos[2] - rz)*(pos[2] - rz);
}
// the trunk byte: small_tree::draw_trunk(shadow_pass, all_visible, skip_lines = 1, xlate) down to nsides.  0: returns 1 without drawing; 1: the skipped line; else nsides
TERRA_HD uint8_t tree_view_trunk(tree_view_consts_t const &c, tree_view_rec_t const &r, bool all_visible) {
	if (r.type == T_BUSH) return 0;
	if (!all_visible) {
		float const x = 0.5f*(r.p1[0] + r.p2[0]) + c.a.offx, y = 0.5f*(r.p1[1] + r.p2[1]) + c.a.offy, z = 0.5f*(r.p1[2] + r.p2[2]) + 0.0f; // trunk_cylin.get_center() + xlate
		float ext;
		if (!r.rotated) {ext = fabsf(r.p1[2] - r.p2[2]);}
		else {float const dx = r.p1[0] - r.p2[0], dy = r.p1[1] - r.p2[1], dz = r.p1[2] - r.p2[2]; ext = sqrtf(dx*dx + dy*dy + dz*dz);} // get_length()
		float const bsr = (float)((double)r.r1 + 0.5*(double)ext); // get_trunk_bsphere_radius()
		if (!view_sphere_visible(c.tv.v, c.tv.behind_sphere_mult, x, y, z, bsr)) return 0;
	}
	float const size_scale = c.zoom_f*stt_ss(r.type)*r.width*c.window_width;
	float const *cam = c.tv.v.pos;
	float const px = r.pos[0] + c.a.offx, py = r.pos[1] + c.a.offy, pz = r.pos[2] + 0.0f;
	float const dist = sqrtf((cam[0] - px)*(cam[0] - px) + (cam[1] - py)*(cam[1] - py) + (cam[2] - pz)*(cam[2] - pz)); // distance_to_camera(pos + xlate)
	if (!c.shadow_pass && size_scale < dist) return 0; // too small/far
	float const LINE_THRESH = 700.0f;
	if (!c.shadow_pass && LINE_THRESH*c.zoom_f*(r.r1 + r.r2) < dist) return 1;
	if (c.shadow_pass) return 4;
	int const q = d2i_x86(0.25*(double)size_scale/(double)dist), lo = (TREE_VIEW_CYL_SIDES < q) ? TREE_VIEW_CYL_SIDES : ((q < TREE_VIEW_CYL_SIDES) ? q : TREE_VIEW_CYL_SIDES);
	return (uint8_t)((4 < lo) ? lo : 4); // max(4, min(N_CYL_SIDES, int(0.25*size_scale/dist)))
}

// ---- the tile-level decisions: what draw_pine_trees decides before it walks a tree, from the counts and all_bcube of the group
struct tree_view_tile_t {
	tree_view_tile_pod_t out;
	int all_visible;           // camera_pdu.sphere_visible_test(get_center(), -0.5*radius) (:1483, :1520)
	int trunks;                // the trunk bytes are made (polygon mode and draw_trunks() passed its cull)
	int near_sweep, far_sweep; // draw_tree_leaves_lod(.., 0 / 1, ..) runs
	int draw_all_near;         // its draw_all
	int cube;                  // camera_pdu.cube_visible(all_bcube + xlate)
	int pine_insts, palm_insts, pine_list, pine_sorted, palm_list; // which lists the sweeps write
};
// get_tree_dist_scale(has_palm) from get_dist_to_camera_in_tiles() (xy_dist = 1)
TERRA_HD float tree_view_dist_scale(tree_view_consts_t const &c, float in_tiles, bool has_palm) {float const PALM_DIST_SCALE = 0.75f; return (has_palm ? PALM_DIST_SCALE : 1.0f)*in_tiles/c.denom;}
// get_tree_far_weight(force_high_detail, has_palm): ENABLE_TREE_LOD is 1
TERRA_HD float tree_view_far_weight(tree_view_consts_t const &c, float in_tiles, bool force_high_detail, bool has_palm) {
	float const GEOMORPH_THRESH = 6.0f;
	if (force_high_detail) return 0.0f;
	return max_std(0.0f, min_std(1.0f, GEOMORPH_THRESH*(tree_view_dist_scale(c, in_tiles, has_palm) - 1.0f))); // CLIP_TO_01
}
TERRA_HD tree_view_tile_t tree_view_tile(tree_view_consts_t const &c, int tx, int ty, terra_tile_stats const &st, float trmax, uint32_t num_trees, uint32_t num_pine, uint32_t num_palm, float const bc[6]) {
	tree_view_tile_t o;
	terrain_view_geom_t const g = terrain_view_geom(c.tv, tx, ty, st.mzmin, st.mzmax, trmax, st.mzmax);
	float const *cam = c.tv.v.pos;
	float const in_tiles = terrain_view_rel_dist_xy(c.tv, g, st.radius)*(float)6; // get_dist_to_camera_in_tiles(): get_rel_dist_to_camera(1)*TILE_RADIUS
	bool const has_palm = num_palm > 0, force = c.shadow_pass != 0;
	uint32_t fl = 0;
	o.out.dscale = tree_view_dist_scale(c, in_tiles, false);
	o.out.num_pine = num_pine; o.out.num_palm = num_palm; o.out.num_trees = num_trees; o.out.leaf_written = 0u; o.out.pad = 0u;
	o.all_visible = view_sphere_visible(c.tv.v, c.tv.behind_sphere_mult, g.cx, g.cy, g.cz, (float)(-0.5*(double)st.radius)) ? 1 : 0;
	float const xb[3][2] = {{bc[0] + c.a.offx, bc[1] + c.a.offx}, {bc[2] + c.a.offy, bc[3] + c.a.offy}, {bc[4] + 0.0f, bc[5] + 0.0f}}; // all_bcube + xlate
	o.cube = view_cube_visible(c.tv.v, xb) ? 1 : 0;
	bool const contains_camera = cam[0] >= g.bc[0][0] && cam[0] <= g.bc[0][1] && cam[1] >= g.bc[1][0] && cam[1] <= g.bc[1][1]; // get_bcube().contains_pt_xy(camera)
	if (o.all_visible) {fl |= TRV_ALL_VISIBLE;}
	if (contains_camera) {fl |= TRV_CONTAINS_CAMERA;}
	// update_pine_tree_state's weights (:1443-1448)
	float const fw = tree_view_far_weight(c, in_tiles, force, has_palm), w_high = 1.0f - fw;
	if ((double)w_high > 0.0) {fl |= TRV_NEEDS_HIGH;}
	if ((double)fw > 0.0) {fl |= TRV_NEEDS_LOW;}
	// the trunks (:1477-1489)
	o.trunks = 0;
	if (c.draw_trunks) {
		float const dscale = force ? (float)0.0 : o.out.dscale;
		if ((double)dscale < 1.0) {
			bool const culled = !o.all_visible && !o.cube; // draw_trunks' VFC (:208): returns 0, so the tile joins to_draw_trunk_pts
			o.trunks = culled ? 0 : 1;
			fl |= TRV_TRUNK_POLY_ALL; // k_tree_view / the simple form raise it to TRV_TRUNK_POLY_SKIPPED once a line was skipped
			if (culled) {fl = (fl & ~(uint32_t)TRV_TRUNK_MASK) | TRV_TRUNK_POLY_SKIPPED;}
		}
		else if ((double)dscale < 2.0 && (double)tree_view_far_weight(c, in_tiles, force, false) < 0.5) {fl |= TRV_TRUNK_POINTS;}
	}
	// the leaves (:1490-1524)
	float const weight = (float)(1.0 - (double)fw);
	o.out.weight = weight;
	o.near_sweep = o.far_sweep = 0;
	bool const dith = (double)weight > 0.0 && (double)weight < 1.0;
	if (dith) {fl |= TRV_DITHERED;}
	bool palms = false;
	if (c.draw_near || c.draw_far) {
		if (dith) {o.near_sweep = c.draw_near; o.far_sweep = c.draw_far;}
		else if (((double)weight == 0.0) ? c.draw_far : c.draw_near) {if ((double)weight == 0.0) {o.far_sweep = 1;} else {o.near_sweep = 1;}}
		palms = c.draw_near && has_palm && ((double)weight > 0.0 || force || (c.a.instanced && (double)tree_view_dist_scale(c, in_tiles, has_palm) < 3.0));
	}
	o.draw_all_near = (o.near_sweep && view_point_visible(c.tv.v, g.cx, g.cy, g.cz)) ? 1 : 0; // draw_all of :1460 for low_detail = 0
	if (o.near_sweep) {fl |= TRV_NEAR_LEAVES; if (o.draw_all_near) {fl |= TRV_DRAW_ALL_NEAR;}}
	if (o.far_sweep) {fl |= TRV_FAR_LEAVES | TRV_DRAW_ALL_FAR;}
	if (palms) {fl |= TRV_PALMS;}
	// which lists: draw_pine_leaves (:281-310), draw_tree_insts (:242-258), draw_non_pine_leaves (:312-323)
	bool const near_ok = o.near_sweep && num_pine > 0 && (o.draw_all_near || o.cube);
	o.pine_insts = (near_ok && c.a.instanced) ? 1 : 0;
	o.pine_list = (near_ok && !c.a.instanced && !o.draw_all_near) ? 1 : 0;
	o.pine_sorted = (o.pine_list && contains_camera) ? 1 : 0;
	o.palm_insts = (palms && c.a.instanced && (o.all_visible || o.cube)) ? 1 : 0;
	o.palm_list = (palms && !c.a.instanced && o.cube) ? 1 : 0;
	o.out.flags = fl;
	return o;
}
// leaf_counts[0] where no pine list is written: render_all's num_pine_trees when a non-instanced sweep draws everything, else 0
TERRA_HD uint32_t tree_view_render_all(tree_view_consts_t const &c, tree_view_tile_t const &tl) {
	if (tl.out.num_pine == 0) return 0u;
	if (tl.near_sweep && !c.a.instanced) return tl.draw_all_near ? tl.out.num_pine : 0u; // (a culled sweep draws nothing)
	return tl.far_sweep ? tl.out.num_pine : 0u;
}

// ---- the arrays of a call, in the order of terra_tiles_tree_view[_dev]: host pointers in the host form's first record, device pointers everywhere else
struct tree_view_io_t {
	terra_tile_stats const *stats; uint8_t const *skip; float const *trmax; tree_place_pod_t const *pine; uint32_t const *counts; trunk_override_pod_t const *ov;
	tree_view_tile_pod_t *tile_out; float *bcube; tree_view_inst_pod_t *pine_insts, *palm_insts; uint32_t *inst_counts, *leaf_list, *leaf_counts; uint8_t *trunk;
};
// the argument rules of a call, behind tree_view_check: throws what the call refuses; false: nothing to do (n == 0).  dev: the arrays are the device's
inline bool tree_view_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, tree_view_io_t const &io, bool dev) {
	if ((uint64_t)n*capacity > 0xFFFFFFFFull) throw std::invalid_argument("tiles_tree_view: n*capacity must fit 32 bits");
	if (n == 0) return false;
	if (!tile_xy || !io.stats || !io.counts || !io.tile_out || !io.bcube || !io.inst_counts || !io.leaf_counts ||
	    (capacity && (!io.pine || !io.pine_insts || !io.palm_insts || !io.leaf_list || !io.trunk))) throw std::invalid_argument("tiles_tree_view: null argument");
	if (dev && (((uintptr_t)io.stats | (uintptr_t)io.trmax | (uintptr_t)io.pine | (uintptr_t)io.counts | (uintptr_t)io.ov | (uintptr_t)io.tile_out | (uintptr_t)io.bcube |
	             (uintptr_t)io.pine_insts | (uintptr_t)io.palm_insts | (uintptr_t)io.inst_counts | (uintptr_t)io.leaf_list | (uintptr_t)io.leaf_counts) & 3u) != 0) {
		throw std::invalid_argument("tiles_tree_view: every array but skip and trunk must be 4-byte aligned");
	}
	return true;
}

// ---- the literal body: tile t of the batch, its records walked in the reference's order.  insts: the instance table (null unless instanced)
TERRA_HD void tree_view_tile_literal(tree_view_consts_t const &c, tree_view_io_t const &io, int32_t const *tile_xy, tree_inst_pod_t const *insts, size_t t) {
	uint32_t const cnt = (io.skip && io.skip[t]) ? 0u : min_u32(io.counts[t], c.cap);
	tree_place_pod_t const *const recs = io.pine + t*c.cap;
	trunk_override_pod_t const *const ovs = io.ov ? io.ov + t*c.cap : nullptr;
	// calc_bcube, num_pine_trees, num_palm_trees
	float bc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	bool any = false;
	uint32_t nvalid = 0, np = 0, npalm = 0;
	tree_view_rec_t rec;
	for (uint32_t j = 0; j < cnt; ++j) {
		if (!tree_view_record(c, insts, recs[j], ovs ? ovs + j : nullptr, rec)) continue;
		++nvalid; np += is_pine_tree_type(rec.type) ? 1u : 0u; npalm += (rec.type == T_PALM) ? 1u : 0u;
		float d[6];
		if (!tree_view_bounds(rec, d)) continue;
		if (!any) {for (int k = 0; k < 6; ++k) {bc[k] = d[k];} any = true;}
		else {box_union(bc, d);}
	}
	for (int k = 0; k < 6; ++k) {io.bcube[t*6 + k] = bc[k];}
	if (nvalid == 0) { // skipped, or pine_trees.empty() (:1468)
		tree_view_tile_pod_t z; z.dscale = 0.0f; z.weight = 0.0f; z.flags = 0u; z.num_pine = z.num_palm = z.num_trees = z.leaf_written = z.pad = 0u;
		io.tile_out[t] = z; io.inst_counts[2*t] = io.inst_counts[2*t + 1] = 0u; io.leaf_counts[2*t] = io.leaf_counts[2*t + 1] = 0u;
		return;
	}
	tree_view_tile_t tl = tree_view_tile(c, tile_xy[2*t], tile_xy[2*t + 1], io.stats[t], io.trmax ? io.trmax[t] : 0.0f, nvalid, np, npalm, bc);
	tree_view_inst_pod_t *const pi = io.pine_insts + t*c.cap, *const mi = io.palm_insts + t*c.cap;
	uint32_t *const ll = io.leaf_list + t*c.cap;
	uint32_t npi = 0, nmi = 0, nl = 0, nm = 0;
	bool skipped = false;
	bool const need_vis = (tl.pine_insts && !tl.draw_all_near) || (tl.palm_insts && !tl.all_visible) || tl.pine_list;
	for (uint32_t j = 0; j < cnt; ++j) {
		bool const valid = tree_view_record(c, insts, recs[j], ovs ? ovs + j : nullptr, rec);
		uint8_t const b = (valid && tl.trunks) ? tree_view_trunk(c, rec, tl.all_visible != 0) : (uint8_t)0;
		io.trunk[t*c.cap + j] = b; skipped = skipped || b == 1;
		if (!valid) continue;
		bool const pine = is_pine_tree_type(rec.type), palm = rec.type == T_PALM;
		bool const vis = need_vis && tree_view_leaves_visible(c, rec);
		int32_t const id = recs[j].inst;
		auto insert = [&](tree_view_inst_pod_t *out, uint32_t &m) { // where sort(insts) puts it: behind every entry with an id that is not larger
			uint32_t k = m++;
			for (; k > 0 && out[k - 1].id > (uint32_t)id; --k) {out[k] = out[k - 1];}
			out[k].id = (uint32_t)id; for (int q = 0; q < 3; ++q) {out[k].pt[q] = rec.pos[q];}
		};
		if (tl.pine_insts && pine && id >= 0 && (tl.draw_all_near || vis)) {insert(pi, npi);}
		if (tl.palm_insts && palm && id >= 0 && (tl.all_visible || vis)) {insert(mi, nmi);}
		if (tl.pine_list && pine && vis) {
			uint32_t k = nl++;
			if (tl.pine_sorted) { // get_back_to_front_ordering: ascending (p2p_dist_sq, index)
				float const key = tree_view_sort_key(c, rec.pos);
				for (; k > 0 && tree_view_before_f(key, j, tree_view_sort_key(c, recs[ll[k - 1]].pos), ll[k - 1]); --k) {ll[k] = ll[k - 1];}
			}
			ll[k] = j;
		}
	}
	if (tl.palm_list) { // draw_non_pine_leaves(0, 1, 0, ..): behind the pine entries
		for (uint32_t j = 0; j < cnt; ++j) {
			if (!tree_view_record(c, insts, recs[j], ovs ? ovs + j : nullptr, rec) || rec.type != T_PALM || !tree_view_leaves_visible(c, rec)) continue;
			ll[nl + nm++] = j;
		}
	}
	if (skipped) {tl.out.flags = (tl.out.flags & ~(uint32_t)TRV_TRUNK_MASK) | TRV_TRUNK_POLY_SKIPPED;}
	tl.out.leaf_written = nl + nm;
	io.tile_out[t] = tl.out;
	io.inst_counts[2*t] = npi; io.inst_counts[2*t + 1] = nmi;
	io.leaf_counts[2*t] = tl.pine_list ? nl : tree_view_render_all(c, tl); io.leaf_counts[2*t + 1] = nm;
}

} // namespace terra
