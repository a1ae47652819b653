// terra_sceneryplace.hpp -- scenery placement of a tile: the cell loop of scenery_group::gen (src/scenery.cpp:1263-1353) as tile_t::update_scenery
// (src/tiled_mesh.cpp:1568-1578) calls it, with scenery_obj::gen_spos (:94-99, use_xy = 1) and the create functions of the nine object classes: plant_base (:697-709),
// s_plant (:720-729), leafy_plant (:943-959, up to gen_leaves), rock_shape3d (:145-149, up to gen_rock), surface_rock (:368-372, up to the surface cache), voxel_rock
// (:496-499, without gen_model_ix), s_rock (:426-436), s_log (:576-600), s_stump (:642-658), mushroom (:1048-1055); wood_scenery_obj::calc_type (:547),
// signed_rand_vector_norm (src/gen_object.cpp:400-420) and pointT's operator/= and mag() (src/3DWorld.h:268-272, :325).
//
// The per-cell bodies are shared by the driver's simple form (one logical thread per tile, the reference's loop) and by k_scenery_place (terra_kernels.hpp); they
// stand on those of terra_treeplace.hpp (the generator, get_xval, get_exact_zval, get_rel_height, the tree type from a height) and terra_decidplace.hpp (get_avg_veg).
// Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out.
// A cell is independent of every other: the generator is re-seeded from the cell's global coordinates (:1276-1277).  Both seed expressions are int products that
// wrap, so the `long` state starts in int range and tree_rgen_t's 32-bit form holds (see there).
#pragma once
#include "terra_decidplace.hpp"

namespace terra {

enum {SCENERY_LEAFY_PLANT = 0, SCENERY_PLANT, SCENERY_ROCK_SHAPE, SCENERY_SURFACE_ROCK, SCENERY_VOXEL_ROCK, SCENERY_ROCK, SCENERY_LOG, SCENERY_STUMP, SCENERY_MUSHROOM,
      SCENERY_KINDS, SCENERY_NONE = -1}; // TERRA_SCENERY_*
enum {LEAFY_PLANT_UW = 0, LEAFY_PLANT_DIRT, LEAFY_PLANT_GRASS, LEAFY_PLANT_ROCK}; // src/scenery.h:14
constexpr int NUM_LAND_PLANT_TYPES = 6, NUM_WATER_PLANT_TYPES = 1;                // src/scenery.h:13-16

struct scenery_place_pod_t {float pos[3]; float radius; int32_t kind; int32_t iv[2]; float p[8]; int32_t rseed1, rseed2; uint16_t cx, cy;}; // terra_scenery_place

struct scenery_place_consts_t {
	tree_place_consts_t b;  // the scene: tables, get_xval, get_exact_zval, get_rel_height, the tree type from a height (skip_val 1, ncell S; no brush)
	uint32_t smod;          // (:1266)
	int voxel_rocks;        // use_voxel_rocks == 1 || (use_voxel_rocks >= 2 && vegetation == 0.0) (:1311)
	float vegetation;       // `vegetation` of src/tiled_mesh.cpp:1575; times get_avg_veg() per tile
	float tree_scale;
	float min_stump_z, min_plant_z, min_log_z, min_mushroom_z; // (:1267-1270)
	float min_water_plane_z;                                   // get_water_z_height() - ocean_wave_height (:62)
	float zmin;                                                // the global s_log::create tests (:594)
};

// vegetation*get_avg_veg() (src/tiled_mesh.cpp:1575)
TERRA_HD float scenery_tile_veg(scenery_place_consts_t const &c, float const dens[4]) {return c.vegetation*decid_avg_veg(dens);}

// signed_rand_vector_norm(1.0): signed_rand_vector builds vector3d(scale*signed_rand_float(), .., ..) and g++ evaluates the three arguments right to left, so the
// first draw is z and the third x; scale = 1 leaves every product as it is
TERRA_HD void scenery_rand_vector_norm(tree_rgen_t &r, float v[3]) {
	for (;;) {
		float const z = r.signed_rand_float(), y = r.signed_rand_float(), x = r.signed_rand_float();
		float const mag_sq = x*x + y*y + z*z;
		if (mag_sq > 1.0f*1.0E-12f) { // scale*TOLERANCE
			float const m = (float)(1.0/(double)sqrtf(mag_sq)); // v*(1.0/sqrt(mag_sq)): operator*(T val)
			v[0] = x*m; v[1] = y*m; v[2] = z*m;
			return;
		}
	}
}

// ---- the cell (ix, iy) of the loop, :1276-1281: the seeds, val, rand2_mix and veg.  veg_: vegetation_.  Returns whether any branch of :1284-1351 can create an
// object: val < 150, and val < 50 (the rocks) or veg; r is then the generator as :1281 leaves it.
TERRA_HD bool scenery_cell_selected(scenery_place_consts_t const &c, float veg_, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r, int &val, bool &veg) {
	tree_place_consts_t const &b = c.b;
	int const gj = tx*b.S + (int)ix, gi = ty*b.S + (int)iy; // j + xoff2, i + yoff2
	uint32_t const ui = (uint32_t)gi, uj = (uint32_t)gj, ug = (uint32_t)b.rand_gen_index; // the int seed expressions wrap
	r.set_state((int32_t)(786433u*ui + 196613u*ug), (int32_t)(6291469u*uj + 1572869u*ug));
	uint32_t const v = (uint32_t)r.rand_seed_mix() % c.smod; // int % unsigned
	val = (int)v;
	if (v >= 150u) return false;
	r.rand_mix();
	veg = (double)(r.rseed1 & 127)/128.0 < (double)veg_;
	return veg || v < 50u;
}

// plant_base::create after gen_spos: 0 no plant, 1 land plant, 2 water plant
TERRA_HD int scenery_plant_base(scenery_place_consts_t const &c, float z) {
	if (z < c.min_plant_z) {
		if ((double)z + (0.4/(double)c.tree_scale + 0.025) > (double)c.min_water_plane_z) return 0; // max plant height above min water plane zval
		return 2;
	}
	if ((double)tree_rel_height(c.b, z) > 0.62) return 0; // altitude too high for plants
	return 1;
}
// wood_scenery_obj::calc_type: (char)get_tree_type_from_height(pos.z, global_rand_gen, 1); the types are -1 .. 5, so the char holds them
TERRA_HD int scenery_wood_type(scenery_place_consts_t const &c, float z, tree_rgen_t &r) {return tree_type_from_height(c.b, z, r, true);}

// ---- the chain of :1284-1351 in three stages, so that the kernel keeps the one thing all kinds share -- gen_spos with its get_exact_zval -- out of the divergent code.
// Stage 1: the kind (SCENERY_NONE: no branch creates anything) and what the kind draws before gen_spos: rock_shape3d's rs_rock (pre_i), s_rock's scale (pre_f).
TERRA_HD int scenery_cell_kind(scenery_place_consts_t const &c, int val, bool veg, tree_rgen_t &r, int32_t &pre_i, float pre_f[3]) {
	int kind;
	if (val >= 100) {kind = veg ? SCENERY_LEAFY_PLANT : SCENERY_NONE;}
	else if (veg && r.rand()%100 < 35) {kind = SCENERY_PLANT;}
	else if (val < 5) {kind = SCENERY_ROCK_SHAPE;}
	else if (val < 15) {kind = SCENERY_SURFACE_ROCK;}
	else if (c.voxel_rocks && val < 35) {kind = SCENERY_VOXEL_ROCK;}
	else if (val < 50) {kind = (veg && val < 25) ? SCENERY_MUSHROOM : SCENERY_ROCK;}
	else if (veg && val < 85) {kind = (val < 60) ? SCENERY_MUSHROOM : SCENERY_LOG;}
	else if (veg) {kind = SCENERY_STUMP;}
	else {kind = SCENERY_NONE;}
	if (kind == SCENERY_ROCK_SHAPE) {pre_i = r.rand();} // rs_rock (:147)
	if (kind == SCENERY_ROCK) {for (int i = 0; i < 3; ++i) {pre_f[i] = r.rand_uniform(0.8f, 1.3f);}} // UNROLL_3X(scale[i_] = ..) (:428)
	return kind;
}
// Stage 2: gen_spos(j, i, 1) with the loop's local indices
TERRA_HD void scenery_gen_spos(scenery_place_consts_t const &c, int tx, int ty, unsigned ix, unsigned iy, tree_rgen_t &r, float pos[3]) {
	tree_place_consts_t const &b = c.b;
	pos[0] = (float)((double)tree_get_xval(b, tx*b.S - b.xoff2 + (int)ix) + 0.5*(double)b.DX_VAL*r.randd());
	pos[1] = (float)((double)tree_get_yval(b, ty*b.S - b.yoff2 + (int)iy) + 0.5*(double)b.DY_VAL*r.randd());
	pos[2] = tree_exact_zval(b, pos[0], pos[1]); // interpolate_mesh_zval(px, py, 0.0, 1, 1)
}
// Stage 3: the rest of the kind's create().  Returns whether o is an object -- for a log: whether it goes on to scenery_log_finish, with pt2.xy in o.p[5..6], the
// direction before its z in o.p[2..3] and both radii in place.
TERRA_HD bool scenery_cell_create(scenery_place_consts_t const &c, int kind, int32_t pre_i, float const pre_f[3], tree_rgen_t &r, float const pos[3], scenery_place_pod_t &o) {
	float const ts = c.tree_scale;
	o.pos[0] = pos[0]; o.pos[1] = pos[1]; o.pos[2] = pos[2]; o.radius = 0.0f; o.kind = kind; o.iv[0] = 0; o.iv[1] = 0;
	for (int k = 0; k < 8; ++k) {o.p[k] = 0.0f;}
	switch (kind) {
	case SCENERY_LEAFY_PLANT: {
		int const ret = scenery_plant_base(c, pos[2]);
		if (ret == 0) return false;
		if (ret == 2) {o.iv[0] = LEAFY_PLANT_UW;}
		else {
			float const relh = tree_rel_height(c.b, pos[2]);
			if      ((double)relh < 0.46) {o.iv[0] = LEAFY_PLANT_DIRT;}
			else if ((double)relh < 0.60) {o.iv[0] = LEAFY_PLANT_GRASS;}
			else if ((double)relh < 0.75) {o.iv[0] = LEAFY_PLANT_ROCK;}
			else return false; // snow
		}
		o.radius = r.rand_uniform(0.06f, 0.12f)/ts;
		return true;
	}
	case SCENERY_PLANT: {
		int const ret = scenery_plant_base(c, pos[2]);
		if (ret == 0) return false;
		if (ret == 2) {o.iv[0] = NUM_LAND_PLANT_TYPES + r.rand()%NUM_WATER_PLANT_TYPES;}
		else          {o.iv[0] = r.rand()%NUM_LAND_PLANT_TYPES;}
		o.radius = r.rand_uniform(0.0025f, 0.0045f)/ts;
		o.p[0]   = (float)((double)(r.rand_uniform(0.2f, 0.4f)/ts) + 0.025);
		return true;
	}
	case SCENERY_ROCK_SHAPE:
		o.iv[0] = pre_i; o.iv[1] = r.rand() & 1; // gen_rock(48, 0.05/tree_scale, rs_rock, (rand2()&1))
		return true;
	case SCENERY_SURFACE_ROCK: {
		float const u = r.rand_uniform(0.1f, 0.2f); // the left operand of the product draws first
		o.radius = u*r.rand_float()/ts;
		scenery_rand_vector_norm(r, o.p);
		return true;
	}
	case SCENERY_VOXEL_ROCK: {
		double const u = 0.2*(double)r.rand_uniform(0.5f, 1.0f);
		o.radius = (float)(u*(double)r.rand_float()/(double)ts);
		o.iv[0]  = r.rand(); // rseed
		return true;
	}
	case SCENERY_ROCK: {
		float size = (float)(0.02*(double)r.rand_uniform(0.2f, 0.8f)/(double)ts);
		if ((r.rand() & 3) == 0) {size *= r.rand_uniform(1.2f, 8.0f);}
		o.p[0] = pre_f[0]; o.p[1] = pre_f[1]; o.p[2] = pre_f[2]; o.p[3] = size;
		scenery_rand_vector_norm(r, o.p + 4);
		o.p[7]   = r.rand_uniform(0.0f, 360.0f);
		o.radius = size*(pre_f[0] + pre_f[1] + pre_f[2])/3.0f;
		o.pos[2] = pos[2] + o.radius*r.rand_uniform(-0.1f, 0.25f);
		return true;
	}
	case SCENERY_LOG: {
		float const radius = r.rand_uniform(0.003f, 0.008f)/ts;
		o.radius = radius;
		o.p[0]   = r.rand_uniform((float)(0.9*(double)radius), (float)(1.1*(double)radius)); // radius2
		float const length = r.rand_uniform((float)fmax(0.03/(double)ts, 4.0*(double)radius), (float)fmin(0.15/(double)ts, 20.0*(double)radius));
		float dir[3];
		scenery_rand_vector_norm(r, dir);
		dir[0] *= length; dir[1] *= length;
		o.p[2] = dir[0]; o.p[3] = dir[1]; o.p[4] = dir[2];
		o.p[5] = pos[0] + dir[0]; o.p[6] = pos[1] + dir[1]; // pt2.xy
		o.pos[2] = pos[2] + r.rand_uniform(0.7f, 0.99f)*radius; // interpolate_mesh_zval(pos.x, pos.y, ..) is gen_spos's height again
		return true;
	}
	case SCENERY_STUMP: {
		if (pos[2] < c.min_stump_z) return false;
		float radius = r.rand_uniform(0.005f, 0.01f)/ts;
		float radius2 = r.rand_uniform((float)(0.8*(double)radius), radius);
		o.pos[2] = (float)((double)pos[2] - 2.0*(double)radius);
		float height = (float)((double)r.rand_uniform((float)(0.01/(double)ts), (float)fmin(0.05/(double)ts, 4.0*(double)radius)) + 0.015);
		if ((r.rand() & 3) == 0) { // larger stump = upright dead tree
			height *= r.rand_uniform(1.0f, 5.0f);
			radius  = (float)((double)radius*1.5);
			radius2 = (float)((double)radius2*1.3);
		}
		o.radius = radius; o.p[0] = radius2; o.p[1] = height;
		o.iv[0] = scenery_wood_type(c, o.pos[2], r);
		return o.iv[0] >= 0;
	}
	case SCENERY_MUSHROOM: {
		if (pos[2] < c.min_mushroom_z) return false;
		o.radius = r.rand_uniform(0.005f, 0.01f)/ts;
		o.pos[2] = pos[2] - o.radius; // sink a bit into the ground
		o.p[0]   = r.rand_uniform(4.0f, 5.0f)*o.radius;
		return true;
	}
	default: return false;
	}
}
// s_log::create from :592 on: z2 = get_exact_zval(pt2.x, pt2.y).  Returns whether the log stays.
TERRA_HD bool scenery_log_finish(scenery_place_consts_t const &c, float z2, tree_rgen_t &r, scenery_place_pod_t &o) {
	float const pt2z = z2 + r.rand_uniform(0.7f, 0.99f)*o.p[0];
	if (max_std(o.pos[2], pt2z) < c.min_log_z) return false;
	if (o.pos[2] <= c.zmin || pt2z <= c.zmin) return false; // bad z value
	float const dx = o.p[2], dy = o.p[3], dz = pt2z - o.pos[2];
	float const length = sqrtf(dx*dx + dy*dy + dz*dz); // dir.mag()
	float const m = (float)(1.0/(double)(-length));    // dir /= -length: T const m(1.0/d)
	o.p[1] = length; o.p[2] = dx*m; o.p[3] = dy*m; o.p[4] = dz*m; o.p[7] = pt2z;
	o.iv[0] = scenery_wood_type(c, o.pos[2], r);
	return o.iv[0] >= 0;
}
TERRA_HD void scenery_set_tail(tree_rgen_t const &r, unsigned ix, unsigned iy, scenery_place_pod_t &o) {o.rseed1 = r.rseed1; o.rseed2 = r.rseed2; o.cx = (uint16_t)ix; o.cy = (uint16_t)iy;}

// everything after the selection, in one piece (the simple form).  Returns whether o is an object.
TERRA_HD bool scenery_cell_finish(scenery_place_consts_t const &c, int tx, int ty, unsigned ix, unsigned iy, int val, bool veg, tree_rgen_t &r, scenery_place_pod_t &o) {
	int32_t pre_i = 0; float pre_f[3] = {0.0f, 0.0f, 0.0f}, pos[3];
	int const kind = scenery_cell_kind(c, val, veg, r, pre_i, pre_f);
	if (kind == SCENERY_NONE) return false;
	scenery_gen_spos(c, tx, ty, ix, iy, r, pos);
	if (!scenery_cell_create(c, kind, pre_i, pre_f, r, pos, o)) return false;
	if (kind == SCENERY_LOG && !scenery_log_finish(c, tree_exact_zval(c.b, o.p[5], o.p[6]), r, o)) return false;
	scenery_set_tail(r, ix, iy, o);
	return true;
}

} // namespace terra
