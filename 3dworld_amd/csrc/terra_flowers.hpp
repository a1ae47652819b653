// terra_flowers.hpp -- the flowers of a tile: flower_tile_manager_t::gen_flowers, update_subrange and clear_within (src/grass.cpp:859-926) with
// flower_manager_t::add_flowers (:813-838), as tile_t::draw_flowers (src/tiled_mesh.cpp:1666-1677) and tile_t::add_or_remove_grass_at (:3930-3937) call them;
// rand_float / signed_rand_float / rand_uniform (src/rand_gen.h:86-90), signed_rand_vector (src/gen_object.cpp:400-403), pointT::get_norm (src/3DWorld.h:297-300),
// remove_element (src/inlines.h:743-747), dist_xy_less_than (src/inlines.h:183-195).
//
// The bodies are shared by the driver's simple form (one logical thread per tile, the reference's loops) and by k_flowers_place / k_flowers_remove
// (terra_kernels.hpp).  Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out.
//
// Unlike tree and scenery placement the generator is seeded ONCE per tile (or once per update_subrange) and runs through all its cells: a rejected candidate takes
// one draw, an accepted one nine (eight with a fixed flower_color), so where a candidate's draws lie in the stream depends on every acceptance before it.  The
// second half of this file is what lets a wave leave the serial walk: both recurrences of the generator are multiplications modulo a prime, so the state k steps
// on is a^k * s mod m and any stream position is one modular multiplication away (lcg_jump).
#pragma once
#include "terra_treeplace.hpp"

namespace terra {

struct flower_pod_t {float pos[3]; float normal[3]; float radius, height; float color[4];}; // terra_flower = flower_t (src/grass.h:80-88)

constexpr uint32_t FLOWER_NUM_COLORS = 3;     // NUM_COLORS (:817)
constexpr int      FLOWER_START_EVAL_SIN = 50; // start_eval_sine (:817)
constexpr uint32_t FLOWER_AUX_FIXED = 7;      // the aux word's colour field under a fixed flower_color
constexpr float    FLOWER_DENSITY_MAX = 1024.0f;

struct flower_consts_t {
	int S;
	float DX_VAL, DY_VAL, DX_VAL_INV, DY_VAL_INV;
	float flower_density, grass_length, grass_width;
	float color[4]; int fixed_color; // flower_color and flower_color.alpha > 0.0
	float hthresh;                   // get_median_height(FLOWER_DIST_THRESH)
	double zs;                       // 0.2*zmax_est
};

// add_flowers' head (:816, :821): the candidates of a cell from its grass weight; 0 where grass_den < 0.5
TERRA_HD uint32_t flower_num_per_bin(flower_consts_t const &c, uint8_t weight) {
	float const grass_den = (float)((double)weight/255.0); // weight/255.0 narrowed to the float parameter
	if ((double)grass_den < 0.5) return 0;
	return (uint32_t)((double)(c.flower_density*grass_den) + 0.5); // (flower_density <= FLOWER_DENSITY_MAX: the conversion is in range)
}
// the density function test of :824, one draw: true = the candidate becomes a flower
TERRA_HD bool flower_candidate_accepted(flower_consts_t const &c, float dval, tree_rgen_t &r) {
	return !((double)dval + c.zs*(double)r.signed_rand_float() > (double)c.hthresh);
}
// :825-836 for an accepted candidate of cell (xpos, ypos), dx = dy = 0.0, gen_zval = 0: seven draws and, without a fixed colour, an eighth.
// -> the aux word's colour field: 2 + the C remainder int(0.5*NUM_COLORS*color_val) % 3 taken as signed (-2 .. 2), or FLOWER_AUX_FIXED.
// The colour itself is what the reference computes: NUM_COLORS is `unsigned`, so in `int(..)%NUM_COLORS` the int converts to unsigned before the remainder
// (the usual arithmetic conversions) and the index is unsigned(int(..)) % 3u, 0 .. 2 for every color_val -- for a negative int NOT the signed remainder plus 3.
TERRA_HD uint32_t flower_record(flower_consts_t const &c, int xpos, int ypos, float cval, tree_rgen_t &r, flower_pod_t &o) {
	float const height = c.grass_length*r.rand_uniform(0.85f, 1.0f);
	// point pos(dx + DX_VAL*(xpos + rand_float() - 0.5), dy + DY_VAL*(ypos + rand_float() - 0.5), height): g++ evaluates the constructor's arguments right to left,
	// so the first rand_float() is y's; xpos + rand_float() is a float sum, the - 0.5 and everything outside it double
	float const ry = r.rand_float(), rx = r.rand_float();
	o.pos[0] = (float)(0.0 + (double)c.DX_VAL*((double)((float)xpos + rx) - 0.5));
	o.pos[1] = (float)(0.0 + (double)c.DY_VAL*((double)((float)ypos + ry) - 0.5));
	o.pos[2] = height;
	// (plus_z + signed_rand_vector(0.2)).get_norm(): the vector's arguments right to left too (the first draw is z)
	float const vz = 0.2f*r.signed_rand_float(), vy = 0.2f*r.signed_rand_float(), vx = 0.2f*r.signed_rand_float();
	float const nx = 0.0f + vx, ny = 0.0f + vy, nz = 1.0f + vz;
	float const vmag = sqrtf(nx*nx + ny*ny + nz*nz);
	if (vmag < 1.0E-12f) {o.normal[0] = nx; o.normal[1] = ny; o.normal[2] = nz;} // TOLERANCE (never: nz >= 0.8)
	else {o.normal[0] = nx/vmag; o.normal[1] = ny/vmag; o.normal[2] = nz/vmag;}
	o.radius = c.grass_width*r.rand_uniform(1.5f, 2.5f);
	o.height = height;
	if (c.fixed_color) {
		for (int k = 0; k < 4; ++k) {o.color[k] = c.color[k];}
		return FLOWER_AUX_FIXED;
	}
	float const color_val = (float)((double)cval + 0.25*(double)r.signed_rand_float());
	double const q = 0.5*(double)FLOWER_NUM_COLORS*(double)color_val; // |q| < 2^31: cval is a sum of at most 50 sine terms
	int const iq = (int)q;
	uint32_t const ci = (uint32_t)iq % FLOWER_NUM_COLORS;
	// colors[] = {WHITE, YELLOW, LT_BLUE} (:818; src/3DWorld.h:1264-1281)
	o.color[0] = (ci == 2u) ? 0.58f : 1.0f; o.color[1] = (ci == 2u) ? 0.58f : 1.0f; o.color[2] = (ci == 1u) ? 0.0f : 1.0f; o.color[3] = 1.0f;
	return (uint32_t)(iq % (int)FLOWER_NUM_COLORS + 2);
}
TERRA_HD uint32_t flower_aux(uint32_t cx, uint32_t cy, uint32_t color_field) {return cx | (cy << 10) | (color_field << 20);}

// ---- the two removal tests
// update_subrange (:895-896): the flower's cell by truncation, inside [xl, xh) x [yl, yh)
TERRA_HD bool flower_in_range(flower_consts_t const &c, flower_pod_t const &f, int xl, int yl, int xh, int yh) {
	int const fx = f2i_x86(f.pos[0]*c.DX_VAL_INV), fy = f2i_x86(f.pos[1]*c.DY_VAL_INV);
	return fx >= xl && fx < xh && fy >= yl && fy < yh;
}
// clear_within (:919-922); px / py = pos - flower_xlate
TERRA_HD bool flower_in_brush(flower_pod_t const &f, float px, float py, float radius, bool is_square) {
	if (fabsf(f.pos[0] - px) > radius || fabsf(f.pos[1] - py) > radius) return false;
	if (!is_square) {
		float const dx = f.pos[0] - px, dy = f.pos[1] - py;
		if (!(dx*dx + dy*dy < radius*radius)) return false; // dist_xy_less_than
	}
	return true;
}
// what an edit does to tile t: 0 nothing, 1 update_subrange, 2 clear_within, 3 nothing because the range reaches texel row or column S (FLOWER_EDIT_*)
enum {FLOWER_EDIT_NONE = 0, FLOWER_EDIT_ADD, FLOWER_EDIT_REMOVE, FLOWER_EDIT_REFUSED};
struct flower_edit_consts_t {
	flower_consts_t f;
	int add, is_square, dxoff, dyoff;
	float px, py, radius; // the brush in camera space
	float xss, yss;       // X_SCENE_SIZE, Y_SCENE_SIZE (get_xval, get_yval)
};
TERRA_HD int flower_edit_kind(flower_edit_consts_t const &c, uint8_t updated, uint8_t generated, uint32_t const *rg) {
	if (!updated || !generated) return FLOWER_EDIT_NONE;
	if (!c.add) return FLOWER_EDIT_REMOVE;
	if ((int)rg[2] <= (int)rg[0] || (int)rg[3] <= (int)rg[1]) return FLOWER_EDIT_NONE; // xh <= xl || yh <= yl (:892)
	if (rg[2] > (uint32_t)c.f.S || rg[3] > (uint32_t)c.f.S) return FLOWER_EDIT_REFUSED;
	return FLOWER_EDIT_ADD;
}

// the tile's corner in camera space for clear_within: flower_xlate = (get_xval(x1 + xoff - xoff2), get_yval(y1 + yoff - yoff2)) (src/tiled_mesh.cpp:3935)
TERRA_HD void flower_brush_local(flower_edit_consts_t const &c, int tx, int ty, float &px, float &py) {
	px = c.px - (-c.xss + c.f.DX_VAL*(float)(tx*c.f.S + c.dxoff));
	py = c.py - (-c.yss + c.f.DY_VAL*(float)(ty*c.f.S + c.dyoff));
}
// the seeds of gen_flowers (:864; xl = yl = 0) and update_subrange (:898): x1 + xoff2 with the caller's x1 - xoff2 is the tile's own x1.  int sums, as in the reference
TERRA_HD void flower_seed(int S, int tx, int ty, int xl, int yl, tree_rgen_t &r) {
	r.set_state((int32_t)((uint32_t)tx*(uint32_t)S + (uint32_t)xl + 123u), (int32_t)((uint32_t)ty*(uint32_t)S + (uint32_t)yl + 456u));
}
// the cell loops of gen_flowers (:871-885) and update_subrange (:904-910) over [xl, xh) x [yl, yh), literally: rows, then columns, one generator through all of it.
// w: the tile's [S+1][S+1][4] weights, den / col: its two S x S density fields.  Records go to out[count ..] while they fit; returns the new count.
// (gen_flowers' `weight == 0` skip needs no statement of its own: add_flowers returns at grass_den < 0.5)
TERRA_HD uint32_t flower_gen_serial(flower_consts_t const &c, int tx, int ty, uint32_t xl, uint32_t yl, uint32_t xh, uint32_t yh, uint8_t const *w, float const *den, float const *col,
	uint32_t capacity, flower_pod_t *out, uint32_t *aux, uint32_t count)
{
	uint32_t const S = (uint32_t)c.S;
	tree_rgen_t r;
	flower_seed(c.S, tx, ty, (int)xl, (int)yl, r);
	for (uint32_t y = yl; y < yh; ++y) {
		for (uint32_t x = xl; x < xh; ++x) {
			uint32_t const npb = flower_num_per_bin(c, w[4*((size_t)y*(S + 1) + x) + 2]);
			if (npb == 0) continue;
			float const dval = den[(size_t)y*S + x], cval = col[(size_t)y*S + x];
			for (uint32_t k = 0; k < npb; ++k) {
				if (!flower_candidate_accepted(c, dval, r)) continue;
				flower_pod_t o;
				uint32_t const cf = flower_record(c, (int)x, (int)y, cval, r, o);
				if (count < capacity) {out[count] = o; if (aux) {aux[count] = flower_aux(x, y, cf);}}
				++count;
			}
		}
	}
	return count;
}

// ---- the generator k steps on.  randome_int's two statements (src/rand_gen.h:23-24) are Schrage's form of s = 40014*s mod 2147483563 and s = 40692*s mod 2147483399
// for 0 <= s < m; both moduli are prime.  A state from set_state may lie outside [0, m) (a tile with negative coordinates seeds with values <= 0): the FIRST step
// is therefore always taken literally (tree_rgen_t::advance), after it both states are in [0, m) (see tree_rgen_t) and k further steps are a^k * s mod m.
constexpr uint32_t LCG_M1 = 2147483563u, LCG_A1 = 40014u, LCG_M2 = 2147483399u, LCG_A2 = 40692u;
// a*b mod m for m = 2^31 - C, a, b < m: 2^31 = C (mod m), so the high part folds down twice (a*b < 2^62 -> < 2^39 + 2^31 -> < 2^31 + 2^16 < 2m)
template<uint32_t M> TERRA_HD uint32_t lcg_mulmod(uint32_t a, uint32_t b) {
	constexpr uint32_t C = 0x80000000u - M;
	static_assert(C < 256u, "the fold below needs a small C");
	uint64_t const x = (uint64_t)a*b;
	uint64_t const y = (x >> 31)*C + (x & 0x7FFFFFFFull);
	uint32_t z = (uint32_t)(y >> 31)*C + (uint32_t)(y & 0x7FFFFFFFull);
	if (z >= M) {z -= M;}
	return z;
}
template<uint32_t M> TERRA_HD uint32_t lcg_powmod(uint32_t a, uint32_t k) {
	uint32_t r = 1u;
	for (; k; k >>= 1) {if (k & 1u) {r = lcg_mulmod<M>(r, a);} a = lcg_mulmod<M>(a, a);}
	return r;
}
// the state k steps behind s (both seeds in [0, m)), given p1 = A1^k mod M1 and p2 = A2^k mod M2
TERRA_HD tree_rgen_t lcg_jump(tree_rgen_t s, uint32_t p1, uint32_t p2) {
	s.rseed1 = (int32_t)lcg_mulmod<LCG_M1>((uint32_t)s.rseed1, p1);
	s.rseed2 = (int32_t)lcg_mulmod<LCG_M2>((uint32_t)s.rseed2, p2);
	return s;
}
// the draw a state stands for: what randd() / rand() return right after the step that produced it
TERRA_HD double lcg_state_randd(tree_rgen_t const &s) {
	double v = (double)s.rseed1 - (double)s.rseed2;
	if (v < 1) v += 2147483562;
	return v/2147483563.;
}
TERRA_HD float lcg_state_signed_rand_float(tree_rgen_t const &s) {return (float)(2.0*(double)(float)lcg_state_randd(s) - 1.0);}

} // namespace terra
