// terra_treeao.hpp -- tile_t::apply_tree_ao_shadows (src/tiled_mesh.cpp:740-828) from the placement records to the splat lists of a batch, as per-record bodies
// shared by the driver's simple form and the HIP kernels (k_tree_ao_sources, k_tree_ao_gather):
//   small_tree's constructors                  (src/sm_tree.cpp:705-753)   -> small_tree_size
//   small_tree::get_pine_tree_radius           (src/sm_tree.cpp:911-914)   -> small_tree_radius
//   small_tree::get_radius / get_ao_radius     (src/small_tree.h:74-75)    -> small_tree_radius, small_tree_ao_radius
//   tree::get_ao_radius                        (src/tree_3dw.h:313)        -> decid_tree_ao_radius
//   apply_ao_shadows_for_tree_group's cull     (src/tiled_mesh.cpp:793)    -> tree_ao_culled
//   add_tree_ao_shadow's x_test / y_test       (src/tiled_mesh.cpp:769-775) -> tree_ao_pushed
// Every operand has the type the reference statement gives it; where the statement promotes to double the doubles are written out.
#pragma once
#include "terra_treemap.hpp"
#include "terra_treeplace.hpp"
#include "terra_decidplace.hpp"

namespace terra {

struct tree_inst_pod_t {int32_t type; float height, width;}; // terra_tree_inst: tree_instances' small_tree after its constructor
struct tree_frame_t {float x, y;};                            // xstart, ystart of a tile (src/tiled_mesh.cpp:309-310)
constexpr int NUM_ST_TYPES = 6;                              // src/small_tree.h:9
enum {TREE_AO_NO_PINE = 1, TREE_AO_NO_DECID = 2, TREE_AO_DISTANT = 4}; // the per-tile flag byte
// what the radii read of the globals: hs = tree_height_scale*sm_tree_scale (a float product, :721 and :912)
struct tree_ao_consts_t {
	float hs, pine_radius_scale, tree_scale, tsize; // tsize = calc_tree_size() (:326)
	float dxv, dyv, offx, offy;                     // DX_VAL, DY_VAL and pt_off = ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL) (src/animals.h:26)
	int32_t S, instanced;
	uint32_t num_insts, num_shared;
	uint32_t pine_cap, decid_cap, list_cap;
	uint32_t src_cap;                               // pine_cap + decid_cap: a tile's part of the source array, pine first
};
TERRA_HD bool is_pine_tree_type(int type) {return type == T_PINE || type == T_SH_PINE;}
// stt[type].width_scale / height_scale (src/sm_tree.cpp:46-53): floats initialised from the double literals
TERRA_HD float stt_width_scale(int type)  {return (type == T_PALM) ? 1.4f : ((type == T_SH_PINE) ? 1.2f : 1.0f);}
TERRA_HD float stt_height_scale(int type) {return (type == T_PINE) ? 1.2f : ((type == T_PALM) ? 2.0f : ((type == T_SH_PINE) ? 0.8f : 1.0f));}
// height and width as the constructor leaves them: (:717-726) for a record that is not instanced, (:705-713) for an instance.  false: no such tree
// (a type outside stt[], an instance outside the table, an instanced record while `instanced` is off)
TERRA_HD bool small_tree_size(tree_ao_consts_t const &c, tree_inst_pod_t const *insts, tree_place_pod_t const &r, int &type, float &height, float &width) {
	if (r.inst >= 0) {
		if (!c.instanced || (uint32_t)r.inst >= c.num_insts) return false;
		tree_inst_pod_t const in = insts[r.inst]; // *this = tree_instances.get_tree(instance_id): the instance's type, not the record's
		type = in.type; width = in.width*c.tsize; height = in.height*c.tsize;
	}
	else {
		type = r.type; height = r.height; width = r.width;
		if (type < 0 || type >= NUM_ST_TYPES) return false;
		height *= c.hs;                     // height *= tree_height_scale*sm_tree_scale
		width  *= stt_width_scale(type);
		height *= stt_height_scale(type);
	}
	return type >= 0 && type < NUM_ST_TYPES;
}
// get_radius() with branch_xy_scale = 1.0 (the constructor's default): get_pine_tree_radius for the two pines, width for the others
TERRA_HD float small_tree_radius(tree_ao_consts_t const &c, int type, float height, float width) {
	if (!is_pine_tree_type(type)) return width;
	float const height0 = (float)(((type == T_PINE) ? 0.75 : 1.0)*(double)height/(double)c.hs);
	float const r = (float)(0.35*(double)c.pine_radius_scale*((double)height0 + 0.03/(double)c.tree_scale));
	return 1.0f*r;
}
TERRA_HD float small_tree_ao_radius(int type, float radius) {return (float)((is_pine_tree_type(type) ? 1.8 : ((type == T_PALM) ? 0.4 : 0.5))*(double)radius);}
TERRA_HD float decid_tree_ao_radius(float radius) {return (float)(0.5*(double)radius);}
// a radius the reference can work with; anything else drops the record (it adds nothing to trmax and makes no splat)
TERRA_HD bool tree_radius_ok(float r) {return isfinite(r) && r >= 0.0f;}

// one record -> its source entry {pt.x, pt.y, get_ao_radius()} (radius -1: dropped) and its get_radius() (0 when dropped)
TERRA_HD tree_splat_in_t tree_ao_source_pine(tree_ao_consts_t const &c, tree_inst_pod_t const *insts, tree_place_pod_t const &r, float &radius) {
	tree_splat_in_t o = {r.pos[0] + c.offx, r.pos[1] + c.offy, -1.0f};
	int type; float h, w;
	radius = 0.0f;
	if (!small_tree_size(c, insts, r, type, h, w)) return o;
	float const rad = small_tree_radius(c, type, h, w), ao = small_tree_ao_radius(type, rad);
	if (!tree_radius_ok(rad) || !tree_radius_ok(ao)) return o;
	radius = rad; o.radius = ao;
	return o;
}
// by_record: the caller's radius of this record; else by_id[tree_id]
TERRA_HD tree_splat_in_t tree_ao_source_decid(tree_ao_consts_t const &c, decid_place_pod_t const &r, float const *by_record, float const *by_id, float &radius) {
	tree_splat_in_t o = {r.pos[0] + c.offx, r.pos[1] + c.offy, -1.0f};
	radius = 0.0f;
	float rad;
	if (by_record) {rad = *by_record;}
	else if (by_id && r.tree_id >= 0 && (uint32_t)r.tree_id < c.num_shared) {rad = by_id[r.tree_id];}
	else return o;
	float const ao = decid_tree_ao_radius(rad);
	if (!tree_radius_ok(rad) || !tree_radius_ok(ao)) return o;
	radius = rad; o.radius = ao;
	return o;
}
// the cull of :793 against get_mesh_bcube() of the tile whose frame starts at (xstart, ystart) (src/tiled_mesh.h:238-241)
TERRA_HD bool tree_ao_culled(tree_ao_consts_t const &c, tree_splat_in_t const &s, float xstart, float ystart) {
	float const bx2 = xstart + (float)c.S*c.dxv, by2 = ystart + (float)c.S*c.dyv;
	return s.x + s.radius < xstart || s.x - s.radius > bx2 || s.y + s.radius < ystart || s.y - s.radius > by2;
}
// x_test[dx+1] && y_test[dy+1] of :769-775 for a tree of the tile whose frame starts at (xstart, ystart); a splat skipped there (rval == 0) pushes nothing
TERRA_HD bool tree_ao_pushed(tree_ao_consts_t const &c, tree_splat_in_t const &s, float xstart, float ystart, int dx, int dy) {
	tree_splat_pod_t const p = tree_splat_params(s, xstart, ystart, c.dxv, c.dyv);
	if (p.rval == 0) return false;
	bool const xt = (dx < 0) ? (p.xc <= p.rval) : ((dx > 0) ? (p.xc >= c.S - p.rval) : true);
	bool const yt = (dy < 0) ? (p.yc <= p.rval) : ((dy > 0) ? (p.yc >= c.S - p.rval) : true);
	return xt && yt;
}
// no_adj_test (:826)
TERRA_HD bool tree_ao_no_adj(tree_ao_consts_t const &c, float trmax) {return trmax < min_std(c.dxv, c.dyv);}

// ---- the (up to) 17 segments of tile t's list: own, 8 pulls in dy, dx order, 8 pushes in batch order.  A segment is a filtered subsequence of one source tile's
// array; tree_ao_segment sets it up, tree_ao_keep is the filter of one entry.
enum {TREE_AO_OWN = 0, TREE_AO_PULL = 1, TREE_AO_PUSH = 2};
struct tree_ao_seg_t {
	uint32_t u;          // the source tile
	int mode, dx, dy;    // push: (dx, dy) points from u to t
	uint32_t gate;       // the flag bits that gate the two groups: t's for own and pull (the reference tests `this`), u's for push
	bool cull;           // the cull of :793 against t's box
	uint32_t np, nd;     // u's pine and deciduous entries
};
// one segment of tile t's list, from source tile u (own: u == t); false: the segment is empty.  slot: where u sits in t's row of the [n][9] neighbour table
// ((dy+1)*3 + dx+1 -> batch index, -1: none), which gives a push its direction
TERRA_HD bool tree_ao_segment(tree_ao_consts_t const &c, uint32_t t, int mode, uint32_t u, int slot, uint8_t const *flags, float const *trmax,
	uint32_t const *pine_counts, uint32_t const *decid_counts, tree_ao_seg_t &sg)
{
	uint32_t const ft = flags ? flags[t] : 0u, fu = flags ? flags[u] : 0u;
	if ((ft | fu) & TREE_AO_DISTANT) return false; // a distant tile is neither processed nor a source nor a target (:743, :813, :822)
	bool const no_adj_t = tree_ao_no_adj(c, trmax[t]);
	sg.u = u; sg.mode = mode; sg.dx = sg.dy = 0;
	if (mode == TREE_AO_OWN) {sg.gate = ft; sg.cull = no_adj_t;}
	else if (mode == TREE_AO_PULL) {if (no_adj_t) return false; sg.gate = ft; sg.cull = true;}
	else {
		if (tree_ao_no_adj(c, trmax[u])) return false; // u ran with no_adj_test: no push
		sg.gate = fu; sg.cull = false;
		sg.dx = -(slot%3 - 1); sg.dy = -(slot/3 - 1); // u sits at (slot%3 - 1, slot/3 - 1) from t
	}
	sg.np = (pine_counts && !(sg.gate & TREE_AO_NO_PINE)) ? min_u32(pine_counts[u], c.pine_cap) : 0u;
	sg.nd = (decid_counts && !(sg.gate & TREE_AO_NO_DECID)) ? min_u32(decid_counts[u], c.decid_cap) : 0u;
	return sg.np + sg.nd != 0;
}
// entry j = 0 .. np + nd - 1 of the segment -> its place in the source array
TERRA_HD size_t tree_ao_entry(tree_ao_consts_t const &c, tree_ao_seg_t const &sg, uint32_t j) {
	return (size_t)sg.u*c.src_cap + ((j < sg.np) ? j : c.pine_cap + (j - sg.np));
}
// does source entry s of the segment reach tile t's list?  (xs_t, ys_t): t's frame, (xs_u, ys_u): u's
TERRA_HD bool tree_ao_keep(tree_ao_consts_t const &c, tree_ao_seg_t const &sg, tree_splat_in_t const &s, float xs_t, float ys_t, float xs_u, float ys_u) {
	if (s.radius < 0.0f) return false; // dropped by the sources pass
	if (sg.cull && tree_ao_culled(c, s, xs_t, ys_t)) return false;
	if (sg.mode == TREE_AO_PUSH && !tree_ao_pushed(c, s, xs_u, ys_u, sg.dx, sg.dy)) return false;
	return true;
}
// the push sources of tile t in batch order: the smallest neighbour index above `last` (start with last = t), its slot in `slot`; false: no more
TERRA_HD bool tree_ao_next_push(int32_t const *nb, uint32_t &last, int &slot) {
	uint32_t best = 0xFFFFFFFFu; int bs = -1;
	for (int k = 0; k < 9; ++k) {
		int32_t const v = nb[k];
		if (k != 4 && v >= 0 && (uint32_t)v > last && (uint32_t)v < best) {best = (uint32_t)v; bs = k;}
	}
	if (bs < 0) return false;
	last = best; slot = bs;
	return true;
}

} // namespace terra
