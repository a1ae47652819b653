// terra_treeedit.hpp -- one stroke of the tree brush on the two record arrays of a tile batch, tile_draw_t::add_or_remove_trees_at (src/tiled_mesh.cpp:3746-3769) and
// what it calls, as per-tile and per-record bodies shared by the driver's one-thread-per-tile form and the HIP kernels (k_tree_edit, k_tree_edit_append,
// k_tree_edit_finish):
//   tile_t::mesh_sphere_intersect              (src/tiled_mesh.cpp:3796-3799)   -> tree_edit_sphere_hit
//   the two culls of add_or_remove_trees_at    (src/tiled_mesh.cpp:3824-3825)   -> tree_edit_cull
//   remove_tree's two tests                    (src/tiled_mesh.cpp:3782-3783)   -> tree_edit_removed
//   update_trees_bcube of a record             (src/tiled_mesh.cpp:3776-3778, :3784, :3816) -> tree_edit_box_pine / tree_edit_box_decid
//   remove_element                             (src/inlines.h:743-747)          -> remove_elements_serial (terra_common.hpp: the literal loop, the simple form's)
//   the near_tiles loop                        (src/tiled_mesh.cpp:3764-3768)   -> tree_edit_finish
// Every operand has the type the reference statement gives it; where the statement promotes to double the doubles are written out.
#pragma once
#include "terra_erosion.hpp"
#include "terra_treeao.hpp"

namespace terra {

// a tile's get_mesh_bcube() corner (xv1, yv1) and the x, y of its get_center() (src/tiled_mesh.h:229-241), built on the host like tree_frame_t
struct tree_edit_frame_t {float x, y, cx, cy;};
enum {TREE_EDIT_NEAR = 1, TREE_EDIT_HIT = 2, TREE_EDIT_CHANGED = 4}; // the per-tile state byte between the launches (kept in `status`)
enum {TREE_EDIT_NO_PINE_GEN = 1, TREE_EDIT_NO_DECID_GEN = 2};        // gen_flags: pine_trees_generated() / decid_trees.was_generated() is false
struct tree_edit_consts_t {
	tree_ao_consts_t a;    // the radii; a.offx / a.offy = pine_xlate = decid_xlate (:3827)
	float px, py, pz;      // pos, camera space
	float ptx, pty;        // pt_pos = dt_pos = pos - xlate (:3828)
	float rr;              // rradius
	float calc_radius;     // calc_radius() (src/tiled_mesh.h:204)
	int32_t is_square, add;
};
// the update box as the launches accumulate it: lo and hi of the three axes; empty: lo > hi
struct tree_box_t {float lo[3], hi[3];};
TERRA_HD void tree_box_clear(tree_box_t &b) {for (int i = 0; i < 3; ++i) {b.lo[i] = 3.0e38f; b.hi[i] = -3.0e38f;}}
TERRA_HD bool tree_box_empty(tree_box_t const &b) {return b.lo[0] > b.hi[0];}
// set_from_sphere / union_with_sphere (src/3DWorld.h:441-443, :502-504): pt[i] - radius, pt[i] + radius in float
TERRA_HD void tree_box_add_sphere(tree_box_t &b, float x, float y, float z, float r) {
	float const p[3] = {x, y, z};
	for (int i = 0; i < 3; ++i) {b.lo[i] = min_std(b.lo[i], p[i] - r); b.hi[i] = max_std(b.hi[i], p[i] + r);}
}
// tile_t::mesh_sphere_intersect(pos, r) with the tile's radius given: dist_less_than(pos, get_center(), radius + r) (src/inlines.h:176-192), then
// sphere_cube_intersect(pos, r, get_mesh_bcube()) (src/Math3d.cpp:920-935: DMIN_CHECK with its early return per axis; BCUBE_ZTOLER = 1e-6)
TERRA_HD bool tree_edit_sphere_hit(tree_edit_consts_t const &c, tree_edit_frame_t const &f, float mzmin, float mzmax, float radius, float r) {
	float const cz = 0.5f*(mzmin + mzmax);
	float const ex = c.px - f.cx, ey = c.py - f.cy, ez = c.pz - cz, dv = radius + r;
	if (!(ex*ex + ey*ey + ez*ez < dv*dv)) return false;
	float const lo[3] = {f.x, f.y, mzmin - 1.0E-6f}, hi[3] = {f.x + (float)c.a.S*c.a.dxv, f.y + (float)c.a.S*c.a.dyv, mzmax + 1.0E-6f}, p[3] = {c.px, c.py, c.pz};
	float const r2 = r*r;
	float dmin = 0.0f;
	for (int i = 0; i < 3; ++i) {
		if      (p[i] < lo[i]) {float const d = p[i] - lo[i]; dmin += d*d;}
		else if (p[i] > hi[i]) {float const d = p[i] - hi[i]; dmin += d*d;}
		if (dmin > r2) return false;
	}
	return true;
}
// the culls of :3824-3825 -> 0: not near, TREE_EDIT_NEAR: near and not overlapping, TREE_EDIT_NEAR | TREE_EDIT_HIT: the loops run.  `radius` of the tile is what
// postproc_trees (src/tiled_mesh.h:342-347) leaves: max(stats.radius, calc_radius() + trmax), because trmax only grows
TERRA_HD uint32_t tree_edit_cull(tree_edit_consts_t const &c, tree_edit_frame_t const &f, float mzmin, float mzmax, float stats_radius, float trmax) {
	float const radius = max_std(stats_radius, c.calc_radius + trmax);
	float const r1 = (float)(1.1*(double)c.rr + 2.0*(double)trmax); // (1.1*rradius + 2.0*trmax): a double expression narrowed at the call
	if (!tree_edit_sphere_hit(c, f, mzmin, mzmax, radius, r1)) return 0u;
	if (!tree_edit_sphere_hit(c, f, mzmin, mzmax, radius, c.rr)) return TREE_EDIT_NEAR;
	return TREE_EDIT_NEAR | TREE_EDIT_HIT;
}
// the skip byte the brush placements of a stroke run with: the caller's (can_have_trees() is false), or a tile the culls left out, or a group its gen_flags bit gates: new records nobody would append.  One byte per group: [2][n], pine / palm first
TERRA_HD uint8_t tree_edit_place_skip(uint32_t state, uint32_t skip, uint32_t not_generated) {return (skip != 0u || not_generated != 0u || !(state & TREE_EDIT_HIT)) ? 1u : 0u;}
// remove_tree's tests (:3782-3783) on a record's get_center() against pt_pos
TERRA_HD bool tree_edit_removed(tree_edit_consts_t const &c, float tx, float ty) {
	float const ex = tx - c.ptx, ey = ty - c.pty;
	if (fabsf(ex) > c.rr || fabsf(ey) > c.rr) return false;
	if (!c.is_square && !(ex*ex + ey*ey < c.rr*c.rr)) return false; // dist_xy_less_than
	return true;
}
// update_trees_bcube(tpos + xlate, 2.0*get_radius(), box) of a record; a record terra_treeao.hpp drops adds nothing.  Returns get_radius() (0 when dropped)
TERRA_HD float tree_edit_box_pine(tree_edit_consts_t const &c, tree_inst_pod_t const *insts, tree_place_pod_t const &r, tree_box_t &b) {
	float radius;
	tree_splat_in_t const s = tree_ao_source_pine(c.a, insts, r, radius);
	if (s.radius < 0.0f) return 0.0f;
	tree_box_add_sphere(b, s.x, s.y, r.pos[2] + 0.0f, (float)(2.0*(double)radius));
	return radius;
}
TERRA_HD float tree_edit_box_decid(tree_edit_consts_t const &c, decid_place_pod_t const &r, float const *by_record, float const *by_id, tree_box_t &b) {
	float radius;
	tree_splat_in_t const s = tree_ao_source_decid(c.a, r, by_record, by_id, radius);
	if (s.radius < 0.0f) return 0.0f;
	tree_box_add_sphere(b, s.x, s.y, r.pos[2] + 0.0f, (float)(2.0*(double)radius));
	return radius;
}
// a new deciduous record's get_radius(): by_id[tree_id]; -1 (dropped by tree_radius_ok) when the id is outside the table
TERRA_HD float tree_edit_new_decid_radius(tree_edit_consts_t const &c, decid_place_pod_t const &r, float const *by_id) {
	return (by_id && r.tree_id >= 0 && (uint32_t)r.tree_id < c.a.num_shared) ? by_id[r.tree_id] : -1.0f;
}
// the box into its six words: [0..2] min of f2ord(lo), [3..5] min of ~f2ord(hi), all 0xFFFFFFFF while empty.  Look first: thousands of waves fold into six words
// and only a few can lower one (a word only falls, so a value that does not beat what the look saw cannot beat what is there now)
TERRA_HD void tree_box_commit(tree_box_t const &b, uint32_t *ord) {
	if (tree_box_empty(b)) return;
	for (int i = 0; i < 3; ++i) {
		uint32_t const lo = f2ord(b.lo[i]), hi = ~f2ord(b.hi[i]);
		if (lo < TERRA_L2_LOAD(&ord[i])) {TERRA_ATOMIC_MIN(&ord[i], lo);}
		if (hi < TERRA_L2_LOAD(&ord[3 + i])) {TERRA_ATOMIC_MIN(&ord[3 + i], hi);}
	}
}
// after all tiles (:3764-3768): status (0, 1, 2) and changed of tile t from its state byte and the batch's box.  A box that is all zeros by value ends the
// reference's function at :3764.  out6 (tile 0 alone writes it): x1 x2 y1 y2 z1 z2, zeros when nothing was added to the box
TERRA_HD void tree_edit_finish(tree_edit_consts_t const &c, tree_edit_frame_t const &f, float mzmin, float mzmax, uint32_t state, uint32_t const *ord, uint8_t &status,
	uint8_t &changed, float *out6)
{
	bool const empty = ord[0] == 0xFFFFFFFFu;
	float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
	if (!empty) {for (int i = 0; i < 3; ++i) {lo[i] = ord2f(ord[i]); hi[i] = ord2f(~ord[3 + i]);}}
	if (out6) {for (int i = 0; i < 3; ++i) {out6[2*i] = lo[i]; out6[2*i + 1] = hi[i];}}
	bool const zeros = lo[0] == 0.0f && hi[0] == 0.0f && lo[1] == 0.0f && hi[1] == 0.0f && lo[2] == 0.0f && hi[2] == 0.0f; // is_all_zeros() (src/3DWorld.h:491)
	status = (state & TREE_EDIT_CHANGED) ? 2u : ((state & TREE_EDIT_NEAR) ? 1u : 0u);
	bool ch = status == 2u; // register_tree_change at :3841
	if (!ch && status >= 1u && !zeros) { // get_mesh_bcube().intersects(update_bcube) (src/3DWorld.h:536-539, adjacency included)
		float const mlo[3] = {f.x, f.y, mzmin - 1.0E-6f}, mhi[3] = {f.x + (float)c.a.S*c.a.dxv, f.y + (float)c.a.S*c.a.dyv, mzmax + 1.0E-6f};
		ch = true;
		for (int i = 0; i < 3; ++i) {if (hi[i] < mlo[i] || lo[i] > mhi[i]) {ch = false;}}
	}
	changed = ch ? 1u : 0u;
}

} // namespace terra
