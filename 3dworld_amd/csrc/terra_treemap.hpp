// terra_treemap.hpp -- the tree map of a tile and its two consumers, as per-element bodies shared by the driver's simple forms and the HIP kernels:
//   tile_t::add_tree_ao_shadow's texel loop   (src/tiled_mesh.cpp:749-767)   -> tree_splat_params, tree_mult, tree_texel
//   tile_t::upload_shadow_map_texture         (src/tiled_mesh.cpp:885-911)   -> shadow_tex_consts, shadow_texel
//   the tail of tile_t::create_texture        (src/tiled_mesh.cpp:1325-1348) -> tree_weights_texel
// Every operand has the type the reference statement gives it; where the statement promotes to double the doubles are written out.
#pragma once
#include "terra_common.hpp"
#include "terra_erosion.hpp"
#include "terra_landscape.hpp"

namespace terra {

struct tree_splat_in_t {float x, y, radius;};                // terra_tree_splat
struct tree_splat_pod_t {int32_t xc, yc, rval; float scale;}; // what the texel loop reads of one tree; rval == 0: the splat is skipped
struct tree_tile_pod_t {float xstart, ystart; uint32_t first, count;}; // get_xval(x1 + dxoff), get_yval(y1 + dyoff) and the tile's part of the splat list
constexpr int TREE_RVAL_MAX = 46340;                         // rval*rval fits an int up to here

TERRA_HD int tree_round_fp(float v) {return (v > 0.0f) ? (int)(v + 0.5f) : (int)(v - 0.5f);} // round_fp (src/inlines.h:63)
// :751-754.  Skipped (rval = 0) where the reference is undefined: a non-finite member, tradius < 0, rval > 46340, |xc| or |yc| beyond 2^30
TERRA_HD tree_splat_pod_t tree_splat_params(tree_splat_in_t const &s, float xstart, float ystart, float DX_VAL, float DY_VAL) {
	tree_splat_pod_t o = {0, 0, 0, 0.0f};
	if (!(isfinite(s.x) && isfinite(s.y) && isfinite(s.radius)) || s.radius < 0.0f) return o;
	float const vx = (s.x - xstart)/DX_VAL, vy = (s.y - ystart)/DY_VAL; // (a NaN or an infinity fails the next test)
	if (!(fabsf(vx) <= 0x1p30f && fabsf(vy) <= 0x1p30f)) return o;
	float const qx = s.radius/DX_VAL, qy = s.radius/DY_VAL;
	if (!(qx < (float)(TREE_RVAL_MAX + 1) && qy < (float)(TREE_RVAL_MAX + 1))) return o;
	int const rval = imax((int)qx, (int)qy) + 1;
	if (rval > TREE_RVAL_MAX) return o;
	o.xc = tree_round_fp(vx); o.yc = tree_round_fp(vy); o.rval = rval;
	o.scale = (float)(0.6/(double)rval); // float const scale(0.6/rval)
	return o;
}
// the tile that owns splat i: the last one whose first <= i among those with a non-empty list
TERRA_HD uint32_t tree_tile_of(tree_tile_pod_t const *tiles, uint32_t n, uint32_t i) {
	uint32_t lo = 0, hi = n; // tiles[lo].first <= i < tiles[hi].first (hi == n: the end of the list)
	while (hi - lo > 1) {uint32_t const mid = lo + (hi - lo)/2; if (tiles[mid].first <= i) {lo = mid;} else {hi = mid;}}
	return lo;
}
// float const mult(0.2 + 0.8*scale*sqrt(dist_sq)) (:761): the sum and both products are double.  The reference includes <math.h> (src/3DWorld.h:13,
// src/inlines.h:8), and g++'s <math.h> brings std::sqrt's overloads into the global namespace: sqrt of a float is the float overload, so the root is rounded to
// float before it enters the double expression; one rounding to float at the end.
// s8 = 0.8*(double)scale, the statement's first product
TERRA_HD float tree_mult(double s8, float dist_sq) {return (float)(0.2 + s8*(double)sqrt_rn(dist_sq));}
// the loop body (:759-765) for texel (x, y) of the window: v = {ao, sh} as the low and high byte.  Returns whether the texel was multiplied
TERRA_HD bool tree_texel(tree_splat_pod_t const &s, double s8, float rval_sq, int x, int y, uint16_t &v) {
	int const ix = x - s.xc, iy = y - s.yc;
	float const dx = (float)((ix < 0) ? -ix : ix), dy = (float)((iy < 0) ? -iy : iy), dist_sq = dx*dx + dy*dy;
	if (dist_sq > rval_sq) return false;
	float const mult = tree_mult(s8, dist_sq);
	uint32_t const ao = (uint32_t)(int)((float)(v & 0xFFu)*mult) & 0xFFu, sh = (uint32_t)(int)((float)(v >> 8)*mult) & 0xFFu; // val.ao *= mult; val.sh *= mult
	v = (uint16_t)(ao | (sh << 8));
	return true;
}
// the clipped window of a splat (:753): x1 .. x2 and y1 .. y2, both inclusive; empty when x2 < x1 or y2 < y1
TERRA_HD void tree_window(tree_splat_pod_t const &s, int S, int &x1, int &y1, int &x2, int &y2) {
	x1 = imax(0, s.xc - s.rval); y1 = imax(0, s.yc - s.rval); x2 = imin(S, s.xc + s.rval); y2 = imin(S, s.yc + s.rval);
}

// ---- upload_shadow_map_texture (:885-911): one RGBA8 texel {mesh shadow, tree shadow, ambient occlusion, 0}
constexpr uint32_t SHADOWED_ALL = 0xCF; // src/3DWorld.h:1404
struct shadow_tex_consts_t {
	float lfs;                         // float const lfs(5.0*(light_factor - 0.4)): a double expression rounded once
	int has_sun, has_moon, mesh_shadows; // light_factor >= 0.4, light_factor <= 0.6 (the float against the double constants), mesh_shadows_enabled()
};
TERRA_HD shadow_tex_consts_t shadow_tex_consts(float light_factor, int mesh_shadows) {
	shadow_tex_consts_t c;
	c.has_sun = ((double)light_factor >= 0.4) ? 1 : 0; c.has_moon = ((double)light_factor <= 0.6) ? 1 : 0; c.mesh_shadows = mesh_shadows ? 1 : 0;
	c.lfs = (float)(5.0*((double)light_factor - 0.4));
	return c;
}
// sun / moon: the smask bytes at the texel's cell (read only where the flags need them); has_tree: a tree map exists, tv = its {ao, sh} pair
TERRA_HD uint32_t shadow_texel(shadow_tex_consts_t const &c, uint32_t sun, uint32_t moon, uint32_t base_ao, bool has_tree, uint32_t tv) {
	uint32_t const tao = tv & 0xFFu, tsh = (tv >> 8) & 0xFFu;
	uint32_t ch2 = base_ao; // no tree AO
	if (has_tree && tao != 255u) {ch2 = (uint32_t)f2i_x86((float)base_ao*(0.3f + 0.7f*(float)tao/255.0f)) & 0xFFu;}
	uint32_t ch0 = 255u;
	if (!c.mesh_shadows) {} // do nothing
	else if (c.has_sun && c.has_moon) {
		float const sun_en = ((sun & SHADOWED_ALL) == 0) ? 1.0f : 0.0f, moon_en = ((moon & SHADOWED_ALL) == 0) ? 1.0f : 0.0f;
		ch0 = (uint32_t)f2i_x86(255.0f*(c.lfs*sun_en + (1.0f - c.lfs)*moon_en)) & 0xFFu; // shadow_val *= (...)
	}
	else if ((c.has_sun ? sun : moon) & SHADOWED_ALL) {ch0 = 0u;} // fully in shadow
	uint32_t const ch1 = has_tree ? ((uint32_t)f2i_x86(63.75f + 0.75f*(float)tsh) & 0xFFu) : 255u;
	return ch0 | (ch1 << 8) | (ch2 << 16);
}

// ---- create_texture's tree pass (:1329-1347) with sz_factor == 1: w = the texel of mesh_weight_data ({sand, dirt, grass, rock}: the LT_* order), tree_ao = tree_map[ix].ao
TERRA_HD uint32_t tree_weights_texel(uint32_t w, uint32_t tree_ao) {
	if (tree_ao == 255u) return w;                        // no trees
	if (((w >> (8*LT_ROCK)) & 0xFFu) == 255u) return w;   // skip city texels with both rock and dirt textures set
	uint32_t const dirt = (w >> (8*LT_DIRT)) & 0xFFu, grass = (w >> (8*LT_GROUND)) & 0xFFu;
	float const v = (float)((double)(int)tree_ao/255.0), wsum = (float)((double)(int)dirt + (1.0 - (double)v)*(double)(int)grass);
	uint32_t const nd = (uint32_t)f2i_x86(max_std(0.0f, min_std(255.0f, wsum))) & 0xFFu, ng = (uint32_t)f2i_x86((float)grass*v) & 0xFFu;
	return (w & ~((0xFFu << (8*LT_DIRT)) | (0xFFu << (8*LT_GROUND)))) | (nd << (8*LT_DIRT)) | (ng << (8*LT_GROUND));
}

} // namespace terra
