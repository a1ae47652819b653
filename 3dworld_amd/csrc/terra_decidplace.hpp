// terra_decidplace.hpp -- deciduous tree placement of a tile: tree_cont_t::gen_trees_tt_within_radius (src/Tree.cpp:2209-2305) from :2240 on, as
// tile_t::gen_decid_trees_if_needed (src/tiled_mesh.cpp:1536-1547, through gen_deterministic, src/Tree.cpp:2153-2155) and tile_t::add_new_trees (:3805-3811) call it,
// with add_new_tree's tree_id (src/Tree.cpp:2157-2166), adjust_tree_zval / get_tree_size_scale (:1465-1480), tile_t::get_z_minmax_for_area (src/tiled_mesh.cpp:548-564),
// get_xpos_round_down (src/mesh.h:136), extract_low_bits_01 (src/inlines.h:68-72) and can_have_decid_trees_in_zrange (src/sm_tree.cpp:580-587).
//
// The per-cell bodies are shared by the driver's simple form (one logical thread per tile, the reference's loop) and by k_decid_place (terra_kernels.hpp); they
// stand on those of terra_treeplace.hpp (the generator, get_xval, the forced-sine cell, get_exact_zval, the class from a height, get_median_height).
// Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out.
// A cell is independent of every other: the generator is re-seeded from the cell's global coordinates (:2269-2270).  Both seed expressions are int products that
// wrap, so the `long` state starts in int range and tree_rgen_t's 32-bit form holds (see there).
#pragma once
#include "terra_treeplace.hpp"
#include "../../include/terra.h" // terra_tile_stats

namespace terra {

constexpr int   NUM_TREE_TYPES = 5;      // src/tree_leaf.h:8
constexpr float TREE_SIZE      = 0.005f; // src/Tree.cpp:20

struct decid_place_pod_t {float pos[3]; float zval; int32_t type, tree_id, rseed1, rseed2; uint16_t cx, cy;}; // terra_decid_place

struct decid_place_consts_t {
	tree_place_consts_t b;  // the scene: tables, get_xval, get_exact_zval, the class from a height, the histogram, the brush (ntrees_mult, sums, tsize ... are not read)
	uint32_t smod, tree_prob, num_shared; // (:2242), shared_tree_data.size()
	int use_density, slope;               // the coverage field (:2285); the caller gave stats and zvals: the slope test can run
	float vegetation;                     // `vegetation` of :1545; times get_avg_veg() per tile
	float min_tree_h, max_tree_h, height_thresh, slope_thresh; // (:2215, :2241), tree_slope_thresh
	float xscale[2], yscale[2];           // [0]: the coverage field, [1]: the type fields (:2250)
	float radius[NUM_TREE_TYPES];         // adjust_tree_zval's radius per type (:1474)
};

// can_have_decid_trees_in_zrange(mzmin, mzmax) without a tree placer; are_trees_enabled() is tree_mode & 1, tested by the caller
TERRA_HD bool decid_zrange_ok(tree_place_consts_t const &c, float z_min, float z_max) {
	if (z_max < c.water_plane_z) return false; // underwater
	return !(tree_rel_height(c, z_min) - c.rand_zone > 0.6f); // must have pine trees, or too high
}
// tile_t::mesh_dz (src/tiled_mesh.cpp:535): max_eq from 0 over the 16 sub-blocks
TERRA_HD float decid_mesh_dz(terra_tile_stats const &s) {
	float dz = 0.0f;
	for (int k = 0; k < 16; ++k) {dz = max_std(dz, s.sub_zmax[k] - s.sub_zmin[k]);}
	return dz;
}
// vegetation*get_avg_veg() (src/tiled_mesh.cpp:1545, src/tiled_mesh.h:221); dens = {params[0][0].veg, [0][1], [1][0], [1][1]}.  The brush passes the default 1.0
TERRA_HD float decid_avg_veg(float const dens[4]) {return 0.25f*(dens[0] + dens[1] + dens[2] + dens[3]);}
TERRA_HD float decid_tile_veg(decid_place_consts_t const &c, float const dens[4]) {
	return c.b.brush ? 1.0f : c.vegetation*decid_avg_veg(dens);
}

// density_gen[f].eval_index(x, y): build_arrays((x1 + xoff2 + 1000*f), (y1 + yoff2 - 1500*f), xscale, yscale, S, S, 0, force_sine_mode = 1), no glaciate
TERRA_HD float decid_field(decid_place_consts_t const &c, int gx1, int gy1, int f, unsigned x, unsigned y) {
	float const xs = c.xscale[f != 0], ys = c.yscale[f != 0];
	float const mx0 = xs*(float)(gx1 + 1000*f), my0 = ys*(float)(gy1 - 1500*f);
	return apply_noise_shape_final(tree_sine_cell(c.b, mx0, my0, xs, ys, x, y), 0, c.b.nc.hp);
}
// density_gen[1 .. 5].eval_index(x, y) in one pass over k: the five fields share sinTable's row and every per-k constant up to x_mult*mx0 / y_mult*my0, and each
// sum still adds its terms in k order, so the bits are those of five decid_field calls
TERRA_HD void decid_type_fields(decid_place_consts_t const &c, int gx1, int gy1, unsigned x, unsigned y, float den[NUM_TREE_TYPES]) {
	tree_place_consts_t const &b = c.b;
	float const xs = c.xscale[1], ys = c.yscale[1];
	float const msx = b.msc*b.nc.DX_VAL_INV, msy = b.msc*b.nc.DY_VAL_INV, ms2 = (float)(0.5*(double)b.msc);
	float mx0[NUM_TREE_TYPES], my0[NUM_TREE_TYPES];
	for (int f = 0; f < NUM_TREE_TYPES; ++f) {mx0[f] = xs*(float)(gx1 + 1000*(f + 1)); my0[f] = ys*(float)(gy1 - 1500*(f + 1)); den[f] = 0.0f;}
	float const fx = (float)x, fy = (float)y;
#pragma unroll 2
	for (int k = b.k0; k < F_TABLE_SIZE; ++k) {
		float const *stk = b.st + 5*k;
		float const x_mult = msx*stk[4], y_mult = msy*stk[3], y_scale = b.mszi*stk[0];
		float const xc0 = ms2*stk[4] + stk[2], yc0 = ms2*stk[3] + stk[1];
		float const xa = (x_mult*xs)*fx, ya = (y_mult*ys)*fy;
#pragma unroll
		for (int f = 0; f < NUM_TREE_TYPES; ++f) {
			float const x_const = xc0 + x_mult*mx0[f], y_const = yc0 + y_mult*my0[f];
			den[f] += b.L.SINF(xa + x_const)*(y_scale*b.L.SINF(ya + y_const));
		}
	}
	for (int f = 0; f < NUM_TREE_TYPES; ++f) {den[f] = apply_noise_shape_final(den[f], 0, b.nc.hp);}
}

// ---- the cell (ix, iy) of the loop (cell ix*skip_val, iy*skip_val of the tile), :2255-2275: the brush test, the seeds and the selection.  veg: vegetation_.
// Returns whether the cell has a tree to try; r is then the generator as the selection leaves it.
TERRA_HD bool decid_cell_selected(decid_place_consts_t const &c, float veg, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r) {
	tree_place_consts_t const &b = c.b;
	int const cx = (int)ix*b.skip_val, cy = (int)iy*b.skip_val;
	int const gj = tx*b.S + cx, gi = ty*b.S + cy; // j + xoff2, i + yoff2
	if (b.brush && b.brad > 0.0f) { // (:2256-2264) on the cell's corner, local indices
		float const yval = tree_get_yval(b, gi - b.yoff2), xval = tree_get_xval(b, gj - b.xoff2);
		if (fabsf(yval - b.by) > b.brad) return false;
		if (fabsf(xval - b.bx) > b.brad) return false;
		if (!((b.bx - xval)*(b.bx - xval) + (b.by - yval)*(b.by - yval) < b.brad*b.brad)) return false; // dist_xy_less_than; is_square is not read by this function
	}
	uint32_t const ui = (uint32_t)gi, uj = (uint32_t)gj, ug = (uint32_t)b.rand_gen_index; // the int seed expressions wrap
	r.set_state((int32_t)(805306457u*ui + 12582917u*uj + 100663319u*ug), (int32_t)(6291469u*uj + 3145739u*ui + 1572869u*ug));
	r.rand_mix();
	uint32_t const val = (uint32_t)r.rand_seed_mix() % c.smod;
	if (val <= 100u) return false;            // scenery
	if (val % c.tree_prob != 0u) return false; // not selected
	return !((double)(r.rseed1 & 127)/128.0 >= (double)veg);
}
// :2276-2285: the position, its height, the range, the class and the coverage field.  Returns whether the cell goes on; pos[2] is get_exact_zval's height.
TERRA_HD bool decid_cell_site(decid_place_consts_t const &c, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r, float pos[3]) {
	tree_place_consts_t const &b = c.b;
	int const cx = (int)ix*b.skip_val, cy = (int)iy*b.skip_val, gx1 = tx*b.S, gy1 = ty*b.S;
	pos[0] = (float)((double)tree_get_xval(b, gx1 - b.xoff2 + cx) + 0.5*(double)b.DX_VAL*r.randd());
	pos[1] = (float)((double)tree_get_yval(b, gy1 - b.yoff2 + cy) + 0.5*(double)b.DY_VAL*r.randd());
	pos[2] = tree_exact_zval(b, pos[0], pos[1]); // interpolate_mesh_zval(pos.x, pos.y, 0.0, 1, 1)
	if (pos[2] > c.max_tree_h || pos[2] < c.min_tree_h) return false;
	if (b.tree_mode == 3 && tree_class_from_height(b, pos[2], false) != TREE_CLASS_DECID) return false; // a pine tree here (or no tree)
	if (c.use_density && decid_field(c, gx1, gy1, 0, (unsigned)cx, (unsigned)cy) > c.height_thresh) return false;
	return true;
}
// tile_t::get_z_minmax_for_area(pos, radius, zmin, zmax) on the tile's zvals [S+2][S+2]; x1 / y1: the tile's global origin.  An empty index range (the reference
// asserts there is none) reads nothing; no index leaves the array whatever the position is.
TERRA_HD void decid_z_minmax_for_area(tree_place_consts_t const &b, float const *zvals, int x1, int y1, float px, float py, float radius, float &zmin, float &zmax) {
	unsigned const zvsize = (unsigned)b.S + 2u, stride = zvsize - 1u;
	float const rx1 = px - radius, ry1 = py - radius, rx2 = px + radius, ry2 = py + radius;
	auto rel = [](float v, int o) {return (int)((uint32_t)f2i_x86(v) - (uint32_t)o);}; // get_xpos_round_down(v) - x1 (wrapping where the reference's int would overflow)
	auto lo = [](int v) {return (unsigned)imax(0, v);};
	auto hi = [stride](int v) {unsigned const u = (unsigned)v + 1u; return (u < stride) ? u : stride;}; // min(stride, (unsigned)(v + 1)): a negative v + 1 is a large unsigned
	unsigned const ix1 = lo(rel((rx1 + b.xss)*b.nc.DX_VAL_INV, x1)), iy1 = lo(rel((ry1 + b.yss)*b.nc.DY_VAL_INV, y1));
	unsigned const ix2 = hi(rel((rx2 + b.xss)*b.nc.DX_VAL_INV, x1)), iy2 = hi(rel((ry2 + b.yss)*b.nc.DY_VAL_INV, y1));
	for (unsigned y = iy1; y <= iy2; ++y) {
		for (unsigned x = ix1; x <= ix2; ++x) {
			float const z = zvals[(size_t)y*zvsize + x];
			zmin = min_std(zmin, z);
			zmax = max_std(zmax, z);
		}
	}
}
// :2286-2301: the type, the slope test and add_new_tree's tree_id.  zvals: the tile's own (read only when slope_test).  Returns whether o is a tree.
TERRA_HD bool decid_cell_finish(decid_place_consts_t const &c, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t const &r, float const pos[3], bool slope_test,
	float const *zvals, decid_place_pod_t &o)
{
	tree_place_consts_t const &b = c.b;
	int const cx = (int)ix*b.skip_val, cy = (int)iy*b.skip_val, gx1 = tx*b.S, gy1 = ty*b.S;
	float den[NUM_TREE_TYPES];
	decid_type_fields(c, gx1, gy1, (unsigned)cx, (unsigned)cy, den);
	int ttype = -1;
	float max_val = 0.0f;
	for (int tt = 0; tt < NUM_TREE_TYPES; ++tt) {
		float den_val = den[tt];
		float const mv = fabsf(100.0f*den_val), jitter = mv - (float)f2i_x86(mv); // extract_low_bits_01(den_val, 100.0)
		den_val = (float)((double)den_val + 0.8*(double)jitter*(double)jitter);
		if (max_val == 0.0f || den_val > max_val) {max_val = den_val; ttype = tt;}
	}
	float zpos = pos[2];
	if (slope_test) { // adjust_tree_zval(pos, 0, ttype, 0, cur_tile)
		float const radius = c.radius[ttype];
		float mzmax = zpos;
		decid_z_minmax_for_area(b, zvals, gx1, gy1, pos[0] + (float)b.xoff2*b.DX_VAL, pos[1] + (float)b.yoff2*b.DY_VAL, (float)(0.5*(double)radius), zpos, mzmax);
		if (!((mzmax - zpos) < c.slope_thresh*radius)) return false; // drop trees on steep slopes
	}
	o.pos[0] = pos[0]; o.pos[1] = pos[1]; o.pos[2] = zpos; o.zval = pos[2]; o.type = ttype; o.cx = (uint16_t)cx; o.cy = (uint16_t)cy;
	o.tree_id = -1;
	if (c.num_shared) { // add_new_tree, ttype >= 0: both seeds are in [0, 2^31) after randd, so the long sum fits 32 unsigned bits
		uint32_t const q = c.num_shared/(uint32_t)NUM_TREE_TYPES, num_per_type = q ? q : 1u;
		uint32_t const id = (((uint32_t)(r.rseed1 >> 7) + (uint32_t)r.rseed2) % num_per_type) + (uint32_t)ttype*num_per_type;
		o.tree_id = (int32_t)((id < c.num_shared - 1u) ? id : c.num_shared - 1u);
	}
	o.rseed1 = r.rseed1; o.rseed2 = r.rseed2;
	return true;
}

} // namespace terra
