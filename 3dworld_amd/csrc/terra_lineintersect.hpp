// terra_lineintersect.hpp -- line-vs-terrain hits: tile_t::line_intersect_mesh (src/tiled_mesh.cpp:2176-2213) with inc_trees = 0, shared by the driver's simple form,
// the HIP kernels and the grass view (a tile's get_mesh_bcube()).
// terra_common.hpp's shadow_line_clip is do_line_clip: its `(double)tmax > 1e-12` and `(double)tmin < 1 - 1e-12` decide every float as the reference's
// `tmax > TOLERANCE` (the float 1e-12f) and `tmin < 1.0 - TOLERANCE` do.  Integer steps wrap and float -> int conversions follow x86 (cvttsd2si: INT_MIN when out
// of range), as the reference binary does for lines whose ends are far outside the scene.
#pragma once
#include "terra_common.hpp"

namespace terra {

struct line_hit_pod_t {float t; int32_t tile, xpos, ypos; float p[3]; uint32_t hit;}; // terra_line_hit
struct line_query_consts_t {float xss, yss, DX_VAL, DY_VAL, DX_VAL_INV, DY_VAL_INV; int S, dxoff, dyoff;};
struct alignas(16) line_box_t {float d[3][2]; int32_t x1, y1;}; // a tile's get_mesh_bcube() and its first mesh cell
static_assert(sizeof(line_box_t) == 32, "line_box_t: two 16-byte loads");
TERRA_HD bool line_finite(shadow_pt_t a, shadow_pt_t b) {return isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z);}
// get_mesh_bcube (src/tiled_mesh.h:238-241) of tile (tx, ty): get_xval(x1 + xoff - xoff2) = -X_SCENE_SIZE + DX_VAL*i (src/mesh.h:122), x2 - x1 = S, BCUBE_ZTOLER = 1e-6
TERRA_HD line_box_t line_tile_box(line_query_consts_t const &c, int tx, int ty, float mzmin, float mzmax) {
	line_box_t b;
	b.x1 = (int)((uint32_t)tx*(uint32_t)c.S); b.y1 = (int)((uint32_t)ty*(uint32_t)c.S);
	float const xv1 = -c.xss + c.DX_VAL*(float)add_wrap(b.x1, c.dxoff), yv1 = -c.yss + c.DY_VAL*(float)add_wrap(b.y1, c.dyoff);
	b.d[0][0] = xv1; b.d[0][1] = xv1 + (float)c.S*c.DX_VAL;
	b.d[1][0] = yv1; b.d[1][1] = yv1 + (float)c.S*c.DY_VAL;
	b.d[2][0] = mzmin - 1.0E-6f; b.d[2][1] = mzmax + 1.0E-6f;
	return b;
}
TERRA_HD bool line_box_clip(line_box_t const &b, shadow_pt_t v1, shadow_pt_t v2) {return shadow_line_clip(v1, v2, b.d);}
// the walk of one (line, tile): false = no hit; else t = cur_t and (ix, iy) = the cell in the tile.  zt: the tile's (S+2)^2 zvals.  Non-finite lines and distant tiles
// are the caller's (they never hit).  Steps are taken LINE_CHUNK at a time: the x / y / z sums advance serially as in the reference, the chunk's zvals are loaded
// before any of its height tests, then the tests run in step order.  Every step loads, a step off the tile from cell 0 (it always exists; its value is not
// tested): the loads carry no condition, so the chunk's LINE_CHUNK loads are all in flight before the first test waits.
constexpr int LINE_CHUNK = 8;
TERRA_HD bool line_tile_hit(line_query_consts_t const &c, line_box_t const &b, shadow_pt_t const v1, shadow_pt_t const v2, float const *zt, float &t, int &ix, int &iy) {
	shadow_pt_t v1c = v1, v2c = v2; // clipped verts
	if (!shadow_line_clip(v1c, v2c, b.d)) return false;
	// get_xpos(x) = int((x + X_SCENE_SIZE)*DX_VAL_INV + 0.5) (src/mesh.h:129-130); xp = get_xpos(x) - x1 - xoff + xoff2
	auto xpos = [&](float x) {return d2i_x86((double)((x + c.xss)*c.DX_VAL_INV) + 0.5);};
	auto ypos = [&](float y) {return d2i_x86((double)((y + c.yss)*c.DY_VAL_INV) + 0.5);};
	int const xp1 = sub_wrap(sub_wrap(xpos(v1c.x), b.x1), c.dxoff), yp1 = sub_wrap(sub_wrap(ypos(v1c.y), b.y1), c.dyoff);
	int const xp2 = sub_wrap(sub_wrap(xpos(v2c.x), b.x1), c.dxoff), yp2 = sub_wrap(sub_wrap(ypos(v2c.y), b.y1), c.dyoff);
	int const dx = sub_wrap(xp2, xp1), dy = sub_wrap(yp2, yp1), steps = imax(1, imax(abs_x86(dx), abs_x86(dy)));
	if (steps >= 10000) return false; // the reference asserts (:2187)
	double const dz = (double)v2c.z - (double)v1c.z, xinc = dx/(double)steps, yinc = dy/(double)steps, zinc = dz/(double)steps;
	double x = xp1, y = yp1, z = (double)v1c.z - 0.1*fabs(zinc);
	double const zden = (double)v2.z - (double)v1.z;
	int const S = c.S, zs = S + 2;
	for (int k0 = 0; k0 <= steps; k0 += LINE_CHUNK) {
		float zv[LINE_CHUNK]; double zc[LINE_CHUNK]; int cell[LINE_CHUNK];
		for (int j = 0; j < LINE_CHUNK; ++j) {
			int const cx = d2i_x86(x), cy = d2i_x86(y); // (int)x: truncation toward zero
			bool const in = k0 + j <= steps && cx >= 0 && cy >= 0 && cx <= S && cy <= S;
			cell[j] = in ? ((cy << 16) | cx) : -1;
			zv[j] = zt[in ? cy*zs + cx : 0];
			zc[j] = z;
			x += xinc; y += yinc; z += zinc;
		}
		for (int j = 0; j < LINE_CHUNK; ++j) {
			bool const above = (double)zv[j] > zc[j]; // (evaluated for every step: no load waits behind a branch)
			if (!(above && cell[j] >= 0)) continue;
			float const cur_t = (float)(((zc[j] - 0.5*zinc) - (double)v1.z)/zden); // t relative to the unclipped v1, v2
			if (cur_t >= 0.0f && cur_t <= 1.0f) {t = cur_t; ix = cell[j] & 0xFFFF; iy = cell[j] >> 16; return true;}
		}
	}
	return false;
}
// the record of a hit on batch tile i: p_int = v1 + t*(v2 - v1) (line_intersect_tiled_mesh_get_tile, :3643-3648)
TERRA_HD line_hit_pod_t line_hit_make(shadow_pt_t v1, shadow_pt_t v2, float t, uint32_t i, line_box_t const &b, int ix, int iy) {
	line_hit_pod_t h;
	h.t = t; h.tile = (int32_t)i; h.xpos = add_wrap(b.x1, ix); h.ypos = add_wrap(b.y1, iy);
	h.p[0] = v1.x + t*(v2.x - v1.x); h.p[1] = v1.y + t*(v2.y - v1.y); h.p[2] = v1.z + t*(v2.z - v1.z);
	h.hit = 1;
	return h;
}
TERRA_HD line_hit_pod_t line_miss() {line_hit_pod_t h; h.t = 2.0f; h.tile = -1; h.xpos = h.ypos = 0; h.p[0] = h.p[1] = h.p[2] = 0.0f; h.hit = 0; return h;}
// the tiles line r may hit: [i0, i1) -- all of them, the one tile line_tile names (none when it is out of range), none for a non-finite line
TERRA_HD void line_tile_range(int32_t only, uint32_t n, bool finite, uint32_t &i0, uint32_t &i1) {
	i0 = 0; i1 = n;
	if (only >= 0) {i0 = (uint32_t)only; i1 = ((uint32_t)only < n) ? i0 + 1 : i0;}
	if (!finite) {i1 = i0;}
}

} // namespace terra
