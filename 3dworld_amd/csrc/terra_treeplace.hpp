// terra_treeplace.hpp -- pine / palm tree placement of a tile: small_tree_group::gen_trees from src/sm_tree.cpp:439 on and gen_trees_tt_within_radius (:477-502),
// with get_ntrees_for_mesh_xy (:366-376), maybe_add_tree (:378-404), get_tree_type_from_height / get_tree_class_from_height / rel_height_check /
// val_signed_rand_bias_zone (:527-566), can_have_pine_palm_trees_in_zrange (:568-578), get_median_height (src/mesh_gen.cpp:487-491), get_rel_height
// (src/inlines.h:660-663), extract_low_bits_pm1 (src/inlines.h:68-73) and get_exact_zval (src/mesh_gen.cpp:816-847, the procedural branch).
//
// The per-cell bodies are shared by the driver's simple form (one logical thread per tile, the reference's loop) and by k_tree_place (terra_kernels.hpp).
// Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out.
// A cell is independent of every other: get_ntrees_for_mesh_xy re-seeds the generator from the cell's global coordinates whenever XY_MULT_SIZE >= 2*ntrees, which
// the driver proves for every cell before it launches anything (terra_engine::tree_place_consts).
#pragma once
#include "terra_common.hpp"
#include "terra_powf.hpp"
#include "terra_noise.hpp"

namespace terra {

enum {TREE_CLASS_NONE = 0, TREE_CLASS_PINE, TREE_CLASS_DECID, TREE_CLASS_PALM, TREE_CLASS_DETAILED}; // src/tree_3dw.h:20
enum {TREE_NONE = -1, T_PINE = 0, T_DECID = 1, T_PALM = 4, T_SH_PINE = 5};                             // src/small_tree.h:9
constexpr int   NUM_SMALL_TREES = 40000;   // src/sm_tree.cpp:18
constexpr float TREE_DIST_RAND  = 0.125f;  // src/sm_tree.cpp:13
constexpr float SM_TREE_SIZE    = 0.05f;   // src/sm_tree.cpp:12
constexpr float TREE_DIST_SCALE = 100.0f;  // src/tree_3dw.h:9

struct tree_place_pod_t {float pos[3]; int32_t type, inst; float height, width; int32_t rseed1, rseed2; uint16_t cx, cy;}; // terra_tree_place

struct tree_place_consts_t {
	noise_consts_t nc; sin_lut_t L;
	float const *st;   // sinTable [F_TABLE_SIZE][5]
	float const *hist; // height_histogram, sorted
	float const *sums; // the running xv / yv sums of :455-470, one per visited column / row: the same serial float sum on both axes of every tile
	uint32_t nhist;
	int mode, shape, k0; // mesh_gen_mode, mesh_gen_shape, start_eval_sin
	int S, ncell, skip_val, xoff2, yoff2, xy_mult, half_x, half_y; // ncell: cells visited per axis; half_*: MESH_*_SIZE >> 1
	float xss, yss, DX_VAL, DY_VAL, msc, mszi, bxo; // bxo: biome_x_offset
	float ntrees_mult, tsize, thresh, rand_zone, water_plane_z, relh_adj_tex, glaciate_exp_inv, xscale, yscale;
	int tree_mode, force_class, only_pine_palm, rand_gen_index, instanced, num_pine, num_palm, approx_zval, terrain_env;
	int brush, is_square; float bx, by, brad; // gen_trees_tt_within_radius
};

// ---- rand_gen_t (src/rand_gen.h:19-93, src/gen_object.cpp:377-381) for a generator that was seeded with two `int` values, as get_ntrees_for_mesh_xy seeds it:
// the reference holds the state in `long`, but from such seeds every value it ever takes fits an int, and so does every intermediate:
//   |40014*(s % 53668)| <= 40014*53667 = 2147431338 and |12211*(s / 53668)| <= 12211*40014 = 488610954 for any int s, and the two terms have the sign of s, so
//   their difference lies in [-2147431338, 2147431338]; a negative one gets 2147483563 added and lands in [52225, 2147483563).  The same holds for the second
//   seed (40692*52773 = 2147438916, 3791*40692 = 154263372) and survives rand_mix's swap: either recurrence takes any int.
// So 32-bit division by a constant serves where the 64-bit state of terra_common.hpp's rand_gen_t would cost a 64-bit one (six per cell, for every cell).
struct tree_rgen_t {
	int32_t rseed1, rseed2;
	TERRA_HD void set_state(int32_t s1, int32_t s2) {rseed1 = s1; rseed2 = s2;}
	TERRA_HD void advance() {
		if ((rseed1 = 40014*(rseed1%53668) - 12211*(rseed1/53668)) < 0) rseed1 += 2147483563;
		if ((rseed2 = 40692*(rseed2%52774) - 3791 *(rseed2/52774)) < 0) rseed2 += 2147483399;
	}
	TERRA_HD int rand() { // (after a step both seeds are in [0, 2^31): the difference fits)
		advance();
		int v = rseed1 - rseed2;
		if (v < 1) v += 2147483562;
		return v;
	}
	TERRA_HD double randd() {
		advance();
		double v = (double)rseed1 - (double)rseed2;
		if (v < 1) v += 2147483562;
		return v/2147483563.;
	}
	TERRA_HD void swap() {int32_t const s = rseed1; rseed1 = rseed2; rseed2 = s;}
	TERRA_HD int rand_seed_mix() { // int val1(rand()); swap; return val1 + rand(): the int sum wraps
		uint32_t const v1 = (uint32_t)rand();
		swap();
		return (int)(v1 + (uint32_t)rand());
	}
	TERRA_HD void rand_mix() {rand(); swap();}
	TERRA_HD float rand_float() {return (float)(0.000001*(rand()%1000000));}
	TERRA_HD float signed_rand_float() {return (float)(2.0*(double)(float)randd() - 1.0);}
	TERRA_HD float rand_uniform(float a, float b) {return a + (b - a)*(float)randd();}
};

TERRA_HD float tree_get_xval(tree_place_consts_t const &c, int j) {return -c.xss + c.DX_VAL*(float)j;} // get_xval (src/mesh.h:122)
TERRA_HD float tree_get_yval(tree_place_consts_t const &c, int i) {return -c.yss + c.DY_VAL*(float)i;}

// params[yp][xp].veg of tile_t::update_terrain_params (src/tiled_mesh.cpp:321-343) at the tile size S
TERRA_HD float tree_veg_corner(tree_place_consts_t const &c, int tx, int ty, unsigned xp, unsigned yp) {
	if (!c.terrain_env) return 1.0f; // terrain_params_t's default (src/tiled_mesh.h:193)
	int const x1 = tx*c.S, y1 = ty*c.S;
	float const xv1 = tree_get_xval(c, x1), xv2 = xv1 + (float)c.S*c.DX_VAL, yv1 = tree_get_yval(c, y1), yv2 = yv1 + (float)c.S*c.DY_VAL;
	float const xv = c.msc*(xp ? xv2 : xv1) + c.bxo, yv = c.msc*(yp ? yv2 : yv1);
	float const ax = 5.0f*xv, ay = 5.0f*yv; // veg_mult
	float zval = 0.0f; // eval_mesh_sin_terms (src/mesh_gen.cpp:797-805)
#pragma unroll 8
	for (int k = c.k0; k < F_TABLE_SIZE; ++k) {
		float const *stk = c.st + 5*k;
		zval += stk[0]*c.L.SINF(stk[3]*ay + stk[1])*c.L.SINF(stk[4]*ax + stk[2]);
	}
	return clip01(5.000f*(zval + 1.5f));
}

// can_have_pine_palm_trees_in_zrange(mzmin, mzmax) without a tree placer (:568-578); small_trees_enabled() is tree_mode & 2, tested by the caller
TERRA_HD float tree_rel_height(tree_place_consts_t const &c, float zval) { // get_rel_height(zval, -zmax_est, zmax_est)
	float const zmin0 = -c.nc.zmax_est, zmax0 = c.nc.zmax_est;
	float const zv = c.relh_adj_tex + (zval - zmin0)/(zmax0 - zmin0);
	return (zv > 0.0f) ? glibc_powf(zv, c.glaciate_exp_inv) : 0.0f;
}
TERRA_HD bool tree_zrange_ok(tree_place_consts_t const &c, float z_min, float z_max) {
	if (z_max < c.water_plane_z) return false; // underwater
	if (c.force_class >= 0) return c.force_class != TREE_CLASS_NONE;
	float const relh1 = tree_rel_height(c, z_min), relh2 = tree_rel_height(c, z_max);
	if (relh1 - c.rand_zone > 0.9f) return false; // too high
	if (relh2 + c.rand_zone > 0.6f) return true;  // can have pine trees
	if (c.tree_mode != 3) return true;
	return (double)z_min < 0.85*(double)c.water_plane_z && (double)relh1 - 0.2*(double)c.rand_zone < 0.435; // can have palm trees
}

// ---- one cell of a mesh_xy_grid_cache_t: build_arrays' per-k constants (src/mesh_gen.cpp:607-613) and eval_index's sum (:766-780) at (x, y) alone, the same
// fp32 expressions in the same order as the table form (terra_engine::gen_grid_dev), so the same bits
TERRA_HD float tree_sine_cell(tree_place_consts_t const &c, float mx0, float my0, float mdx, float mdy, unsigned x, unsigned y) {
	float const msx = c.msc*c.nc.DX_VAL_INV, msy = c.msc*c.nc.DY_VAL_INV, ms2 = (float)(0.5*(double)c.msc);
	float z = 0.0f;
#pragma unroll 4
	for (int k = c.k0; k < F_TABLE_SIZE; ++k) {
		float const *stk = c.st + 5*k;
		float const x_mult = msx*stk[4], y_mult = msy*stk[3], y_scale = c.mszi*stk[0];
		float const x_const = ms2*stk[4] + stk[2] + x_mult*mx0, y_const = ms2*stk[3] + stk[1] + y_mult*my0;
		float const xmdx = x_mult*mdx, ymdy = y_mult*mdy;
		z += c.L.SINF(xmdx*(float)x + x_const)*(y_scale*c.L.SINF(ymdy*(float)y + y_const));
	}
	return z;
}
TERRA_HD float tree_noise_zval(tree_place_consts_t const &c, float xval, float yval) { // get_noise_zval in the scene's mode
	switch (c.mode) {
	case MGEN_PERLIN:      return noise_zval<MGEN_PERLIN>(xval, yval, c.shape, c.nc);
	case MGEN_DWARP_GPU:   return noise_zval<MGEN_DWARP_GPU>(xval, yval, c.shape, c.nc);
	case MGEN_SIMPLEX_GPU: return noise_zval<MGEN_SIMPLEX_GPU>(xval, yval, c.shape, c.nc);
	default:               return noise_zval<MGEN_SIMPLEX>(xval, yval, c.shape, c.nc);
	}
}
// density_gen.eval_index(j - x1, i - y1): build_arrays((x1 + xoff2), (y1 + yoff2), xscale, yscale, S, S, 0, force_sine_mode = 1), no glaciate (:449, :463)
TERRA_HD float tree_density_field(tree_place_consts_t const &c, int gx1, int gy1, unsigned x, unsigned y) {
	float const mx0 = c.xscale*(float)gx1, my0 = c.yscale*(float)gy1;
	return apply_noise_shape_final(tree_sine_cell(c, mx0, my0, c.xscale, c.yscale, x, y), 0, c.nc.hp);
}
// height_gen.eval_index(j - x1, i - y1): build_arrays((x1 + xoff2 - (MESH_X_SIZE >> 1) + 0.5f), ..., DX_VAL, DY_VAL, S, S) + enable_glaciate() (:452-453, :467)
TERRA_HD float tree_height_field(tree_place_consts_t const &c, int gx1, int gy1, unsigned x, unsigned y) {
	float const mx0 = c.DX_VAL*((float)(gx1 - c.half_x) + 0.5f), my0 = c.DY_VAL*((float)(gy1 - c.half_y) + 0.5f);
	float const xg = ((float)x*c.DX_VAL + mx0)*c.nc.DX_VAL_INV, yg = ((float)y*c.DY_VAL + my0)*c.nc.DY_VAL_INV;
	float z;
	if (c.mode == MGEN_SINE) {z = apply_noise_shape_final(tree_sine_cell(c, mx0, my0, c.DX_VAL, c.DY_VAL, x, y), c.shape, c.nc.hp);}
	else {z = tree_noise_zval(c, xg, yg);}
	float smx = 0.0f, smy = 0.0f;
	if (c.nc.hp.sine_mag > 0.0f) { // enable_glaciate (src/mesh_gen.cpp:640-650)
		float const sm_scale = c.nc.hp.sine_mag*c.mszi, freq = c.msc*c.nc.hp.sine_freq;
		smx = sm_scale*c.L.COSF(xg*freq); smy = c.L.COSF(yg*freq);
	}
	return glaciate_epilogue(z, smx, smy, c.nc.hp.sine_bias*c.mszi, xg, yg, c.nc, c.L);
}
// get_exact_zval(xval, yval) in the tiled-terrain world without a heightmap texture (src/mesh_gen.cpp:816-847); terra_engine::eval_points_dev's kind 1
TERRA_HD float tree_exact_zval(tree_place_consts_t const &c, float xin, float yin) {
	float xval = (float)((double)((xin + c.xss)*c.nc.DX_VAL_INV) + 0.5), yval = (float)((double)((yin + c.yss)*c.nc.DY_VAL_INV) + 0.5);
	xval += (float)c.xoff2; yval += (float)c.yoff2;
	float const fx = xval - (float)c.half_x, fy = yval - (float)c.half_y; // eval_mesh_sin_terms_scaled(xval, yval, 1.0)
	float zval;
	if (c.mode != MGEN_SINE) {zval = tree_noise_zval(c, fx, fy);}
	else {
		float const ax = c.msc*fx, ay = c.msc*fy;
		float s = 0.0f;
#pragma unroll 4
		for (int k = c.k0; k < F_TABLE_SIZE; ++k) {float const *stk = c.st + 5*k; s += stk[0]*c.L.SINF(stk[3]*ay + stk[1])*c.L.SINF(stk[4]*ax + stk[2]);}
		zval = apply_noise_shape_final(s*c.mszi, c.shape, c.nc.hp);
	}
	if (c.nc.glaciate) {float const relh = (zval + c.nc.zmax_est)*c.nc.zmax_est2_inv; zval = glaciate_exp_fn(relh, c.nc.custom_glaciate_exp)*c.nc.zmax_est2 - c.nc.zmax_est;}
	if (c.nc.hp.sine_mag > 0.0f) { // apply_mesh_sine (src/mesh_gen.cpp:373-379)
		float const freq = c.nc.mesh_scale*c.nc.hp.sine_freq;
		zval += (c.nc.hp.sine_mag*c.L.COSF(fx*freq)*c.L.COSF(fy*freq) + c.nc.hp.sine_bias)*c.nc.mesh_scale_z_inv;
		if (c.nc.hp.volcano_width > 0.0f && c.nc.hp.volcano_height > 0.0f) {zval += volcano_height(fx, fy, c.nc, c.L);}
	}
	return zval;
}

// ---- tree types (:527-566)
TERRA_HD float tree_bias_zone(float v, float ref_pt, float zone_width) { // val_signed_rand_bias_zone
	if (zone_width == 0.0f) return v;
	float const dist = fabsf(v - ref_pt), range = zone_width - dist;
	if (range <= 0.0f) return v; // outside the zone
	float const m = (float)(100.0/(double)zone_width), abs_v = fabsf(m*dist); // extract_low_bits_pm1(dist, 100.0/zone_width)
	float const fract = abs_v - (float)f2i_x86(abs_v);                         // get_pos_fract
	return v + range*(float)(2.0*(double)fract - 1.0);
}
TERRA_HD bool tree_rel_height_check(tree_place_consts_t const &c, float v, float thresh, float zw_scale) {return tree_bias_zone(v, thresh, zw_scale*c.rand_zone) > thresh;}
TERRA_HD int tree_class_from_height(tree_place_consts_t const &c, float zpos, bool pine_trees_only) {
	if (zpos < c.water_plane_z) return TREE_CLASS_NONE;
	if (c.force_class >= 0) return c.force_class;
	float const relh = tree_rel_height(c, zpos);
	if (tree_rel_height_check(c, relh, 0.9f, 1.0f)) return TREE_CLASS_NONE; // too high
	if (tree_rel_height_check(c, relh, 0.6f, 1.0f)) return TREE_CLASS_PINE;
	bool const allow_palm_trees = (c.tree_mode == 3);
	if (allow_palm_trees && (double)zpos < 0.85*(double)c.water_plane_z && !tree_rel_height_check(c, relh, 0.435f, 0.2f)) return TREE_CLASS_PALM;
	if (pine_trees_only) return (c.tree_mode == 3) ? TREE_CLASS_NONE : TREE_CLASS_PINE;
	return c.only_pine_palm ? TREE_CLASS_PINE : TREE_CLASS_DECID;
}
TERRA_HD int tree_type_from_height(tree_place_consts_t const &c, float zpos, tree_rgen_t &r, bool for_scenery = false) {
	bool const pine_trees_only = (c.tree_mode == 2 || (!for_scenery && c.tree_mode == 3)); // world_mode == WMODE_INF_TERRAIN (:556)
	switch (tree_class_from_height(c, zpos, pine_trees_only)) {
	case TREE_CLASS_PINE:  return (r.rand()%10 == 0) ? T_SH_PINE : T_PINE;
	case TREE_CLASS_PALM:  return T_PALM;
	case TREE_CLASS_DECID: return T_DECID + r.rand()%3;
	default:               return TREE_NONE;
	}
}

TERRA_HD float tree_median_height(tree_place_consts_t const &c, float pos) { // get_median_height
	if (c.nhist == 0) return pos;
	return c.hist[imax(0, imin((int)c.nhist - 1, f2i_x86((float)c.nhist*pos)))];
}

// can_have_trees() as the caller reports it, can_have_pine_palm_trees_in_zrange when the caller gave the tile's z range, and :440
TERRA_HD bool tree_tile_live(tree_place_consts_t const &c, float const dens[4], bool skipped, bool have_range, float mzmin, float mzmax) {
	if (skipped || (have_range && !tree_zrange_ok(c, mzmin, mzmax))) return false;
	return c.brush || !(dens[0] == 0.0f && dens[1] == 0.0f && dens[2] == 0.0f && dens[3] == 0.0f);
}

// ---- the cell (ix, iy) of the loop (cell ix*skip_val, iy*skip_val of the tile): everything up to and including get_ntrees_for_mesh_xy's selection.
// dens: density[4].  Returns whether the cell has a tree to try; r is then the generator as the selection leaves it.
TERRA_HD bool tree_cell_selected(tree_place_consts_t const &c, float const dens[4], int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r) {
	int const cx = (int)ix*c.skip_val, cy = (int)iy*c.skip_val;
	int const gj = tx*c.S + cx, gi = ty*c.S + cy; // j + xoff2, i + yoff2
	float nmd;
	if (c.brush) { // (:484-493) on the cell's centre, local indices
		float const yval = tree_get_yval(c, gi - c.yoff2), xval = tree_get_xval(c, gj - c.xoff2);
		if (fabsf(yval - c.by) > c.brad) return false;
		if (fabsf(xval - c.bx) > c.brad) return false;
		if (!c.is_square && !((c.bx - xval)*(c.bx - xval) + (c.by - yval)*(c.by - yval) < c.brad*c.brad)) return false; // dist_xy_less_than
		nmd = c.ntrees_mult;
	}
	else {
		float const xv = c.sums[ix], yv = c.sums[iy];
		float const cur_density = yv*(xv*dens[3] + (1.0f - xv)*dens[2]) + (1.0f - yv)*(xv*dens[1] + (1.0f - xv)*dens[0]);
		nmd = cur_density*c.ntrees_mult;
	}
	int const ntrees = (int)(min_std(1.0f, nmd)*(float)NUM_SMALL_TREES); // get_ntrees_for_mesh_xy
	if (ntrees == 0) return false; // (a running sum a few ulps above 1 can leave ntrees a small negative number: the reference goes on, and so does this)
	// XY_MULT_SIZE >= 2*|ntrees| here (the driver's bound): the generator is re-seeded; the int seed expressions wrap
	uint32_t const ui = (uint32_t)gi, uj = (uint32_t)gj, ug = (uint32_t)c.rand_gen_index;
	r.set_state((int32_t)(657435u*ui + 243543u*uj + 734533u*ug), (int32_t)(845631u*uj + 667239u*ui + 846357u*ug));
	r.rand();
	return (r.rand_seed_mix() % (c.xy_mult/ntrees)) == 0; // then max(1, ntrees/XY_MULT_SIZE) = 1 tree
}
// the rest of the cell: the density test (:463-466) or its discarded rand_float (:496), then maybe_add_tree.  Returns whether o is a tree.
TERRA_HD bool tree_cell_finish(tree_place_consts_t const &c, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r, tree_place_pod_t &o) {
	int const cx = (int)ix*c.skip_val, cy = (int)iy*c.skip_val, gx1 = tx*c.S, gy1 = ty*c.S;
	if (c.brush) {r.rand_float();}
	else {
		float const hval = tree_density_field(c, gx1, gy1, (unsigned)cx, (unsigned)cy);
		if (hval > tree_median_height(c, c.thresh - TREE_DIST_RAND*r.rand_float())) return false;
	}
	float const zpos_in = (c.approx_zval && !c.brush) ? tree_height_field(c, gx1, gy1, (unsigned)cx, (unsigned)cy) : 0.0f;
	r.rand_mix(); // maybe_add_tree
	double const half_skip = 0.5*(double)c.skip_val;
	float const xval = (float)((double)tree_get_xval(c, gx1 - c.xoff2 + cx) + half_skip*(double)c.DX_VAL*(double)r.signed_rand_float());
	float const yval = (float)((double)tree_get_yval(c, gy1 - c.yoff2 + cy) + half_skip*(double)c.DY_VAL*(double)r.signed_rand_float());
	float const zpos = (zpos_in != 0.0f) ? zpos_in : tree_exact_zval(c, xval, yval);
	int const ttype = tree_type_from_height(c, zpos, r);
	if (ttype == TREE_NONE) return false;
	o.pos[0] = xval; o.pos[1] = yval; o.pos[2] = zpos; o.type = ttype; o.cx = (uint16_t)cx; o.cy = (uint16_t)cy;
	if (c.instanced) { // num_insts_per_type[ttype].select_inst(rgen): pines share [0, num_pine), palms own [num_pine, num_pine + num_palm)
		bool const palm = (ttype == T_PALM);
		o.inst = (palm ? c.num_pine : 0) + r.rand()%(palm ? c.num_palm : c.num_pine);
		o.height = 0.0f; o.width = 0.0f;
	}
	else {
		o.inst = -1;
		o.height = c.tsize*r.rand_uniform(0.4f, 1.0f);     // tsize*rand_tree_height(rgen)
		o.width  = o.height*r.rand_uniform(0.25f, 0.35f);  // height*rand_tree_width(rgen)
	}
	o.rseed1 = (int32_t)r.rseed1; o.rseed2 = (int32_t)r.rseed2;
	return true;
}

} // namespace terra
