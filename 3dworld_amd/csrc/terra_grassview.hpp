// terra_grassview.hpp -- the grass draw lists of a tile for a camera: tile_t::draw_grass (src/tiled_mesh.cpp:1607-1664) without its GL calls, the per-tile filters of
// its caller tile_draw_t::draw_grass (:3420-3425), tile_t::get_min_dist_to_pt (:354-364, mesh_only), get_rel_dist_to_camera / get_dist_to_camera_in_tiles
// (src/tiled_mesh.h:320-332), get_norm_not_normalized (:281-283) and the thresholds (src/tiled_mesh.cpp:27-29,118-120; src/tiled_mesh.h:24,93-94).  The view
// frustum (view_pod_t, the point and cube tests, closest_pt_dist_sq) is terra_view.hpp's, unsigned(float) terra_common.hpp's f2u_x86.
//
// The bodies are shared by the driver's simple form (one logical thread per tile, the reference's loops) and by k_grass_view (terra_kernels.hpp).  Every operand
// carries the type the reference statement gives it; where the C++ source promotes to double the promotion is written out; dot products are summed in the
// reference's order (the library is built without contraction).
//
// The tests of a block are pure: where the reference leaves a loop early (the `&& back_facing` of the back-face loops) the bodies here evaluate every term and
// combine them -- the same booleans, no branch per term.
#pragma once
#include "terra_view.hpp"
#include "terra_lineintersect.hpp"
#include "terra_landscape.hpp" // grass_block_pod_t
#include "../../include/terra.h" // terra_tile_stats
#include <stdexcept>

namespace terra {

constexpr uint32_t GRASS_VIEW_LODS    = 6;       // NUM_GRASS_LODS (src/grass.h:9)
constexpr uint32_t GRASS_VIEW_BLOCK   = 4;       // GRASS_BLOCK_SZ (src/grass.h:10)
constexpr uint32_t GRASS_VIEW_DROPPED = 0xFFFFu; // the key of a block that is not drawn; a kept block's key is lod*num_rnd_grass_blocks + bix
constexpr uint32_t GRASS_VIEW_MAX_RND = 4096;    // 6*4096 keys fit 16 bits beside GRASS_VIEW_DROPPED; bix fits the aux word's 13 bits
constexpr uint8_t  GRASS_VIEW_NO_PASS = 255;     // the pass byte of a tile that draws nothing

// ---- the constants block: what draw_grass computes before its loops from globals alone
struct grass_view_consts_t {
	view_pod_t v;
	float xss, yss, DX_VAL, DY_VAL, dxdy;
	int S, dxoff, dyoff;
	uint32_t dim, nrnd;                 // get_grass_block_dim() (src/tiled_mesh.h:315), num_rnd_grass_blocks
	float tt;                           // tt_grass_scale_factor
	float grass_thresh;                 // get_grass_thresh_pad() (src/tiled_mesh.cpp:118-120)
	float scaled_tile_radius;           // get_scaled_tile_radius() (src/tiled_mesh.h:94)
	float dx_step, dy_step, lod_scale;  // :1619-1620
	float grass_length, adj_z;          // adj_camera.z (:1622)
};
inline grass_view_consts_t grass_view_consts(view_pod_t const &v, float xss, float yss, float DX_VAL, float DY_VAL, float dxdy, int S, int dxoff, int dyoff, uint32_t nrnd,
	float tt, float grass_length)
{
	grass_view_consts_t c;
	c.v = v; c.xss = xss; c.yss = yss; c.DX_VAL = DX_VAL; c.DY_VAL = DY_VAL; c.dxdy = dxdy; c.S = S; c.dxoff = dxoff; c.dyoff = dyoff;
	c.dim = 1u + ((uint32_t)S - 1u)/GRASS_VIEW_BLOCK; c.nrnd = nrnd; c.tt = tt; c.grass_length = grass_length;
	float const GRASS_LOD_SCALE = 15.0f, GRASS_DIST_SLOPE = 0.25f, GRASS_THRESH = 1.6f; // src/tiled_mesh.cpp:27-29
	int const TILE_RADIUS = 6;                                                             // src/tiled_mesh.h:24
	float const tile_width = xss + yss;                                                    // get_tile_width() (src/tiled_mesh.h:93)
	c.scaled_tile_radius = (float)TILE_RADIUS*tile_width;
	c.grass_thresh = GRASS_THRESH*tt*tile_width + tt/GRASS_DIST_SLOPE;                     // get_grass_thresh() + get_grass_blend_dist()
	c.dx_step = (float)GRASS_VIEW_BLOCK*DX_VAL; c.dy_step = (float)GRASS_VIEW_BLOCK*DY_VAL; // unsigned*float
	c.lod_scale = GRASS_LOD_SCALE/(tt*c.scaled_tile_radius);
	c.adj_z = v.pos[2] + (float)(2.0*(double)grass_length);                                // camera + point(0.0, 0.0, 2.0*grass_length): the double narrows in point()
	return c;
}
// terra_lineintersect.hpp's box of a tile from these constants: tile_t::draw_grass reads get_mesh_bcube() for all_visible and the minimum distance
TERRA_HD line_box_t grass_view_box(grass_view_consts_t const &c, int tx, int ty, float mzmin, float mzmax) {
	line_query_consts_t q;
	q.xss = c.xss; q.yss = c.yss; q.DX_VAL = c.DX_VAL; q.DY_VAL = c.DY_VAL; q.DX_VAL_INV = 0.0f; q.DY_VAL_INV = 0.0f; q.S = c.S; q.dxoff = c.dxoff; q.dyoff = c.dyoff;
	return line_tile_box(q, tx, ty, mzmin, mzmax);
}

// ---- the arrays of a call, in the order of terra_tiles_grass_view[_dev]: host pointers in the host form's first record, device pointers everywhere else
struct grass_view_io_t {
	float const *zvals; terra_tile_stats const *stats; grass_block_pod_t const *blocks; uint8_t const *skip;
	float *insts; uint32_t *aux, *group_counts, *counts; uint8_t *pass;
};
// the argument rules of a call, behind grass_view_check: throws what the call refuses; false: nothing to do (n == 0).  dev: the arrays are the device's
inline bool grass_view_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, grass_view_io_t const &io, bool dev) {
	if (n == 0) return false;
	if (!tile_xy || !io.zvals || !io.stats || !io.blocks || !io.group_counts || !io.counts || (capacity && !io.insts)) throw std::invalid_argument("tiles_grass_view: null argument");
	if (dev && (((uintptr_t)io.zvals | (uintptr_t)io.stats | (uintptr_t)io.blocks | (uintptr_t)io.insts | (uintptr_t)io.aux | (uintptr_t)io.group_counts | (uintptr_t)io.counts) & 3u) != 0) {
		throw std::invalid_argument("tiles_grass_view: d_zvals, d_stats, d_grass_blocks, d_insts, d_aux, d_group_counts and d_counts must be 4-byte aligned");
	}
	return true;
}

// ---- the tile test: what decides for a whole tile (has_grass() is the caller's: it reads the blocks)
struct grass_view_tile_t {
	float llcx, llcy;      // get_xval(x1 + xoff - xoff2), get_yval(y1 + yoff - yoff2) (:1618)
	float bg_thresh_sq;    // :1621
	int in_range;          // !(get_min_dist_to_pt(camera) > grass_thresh) (:1612)
	int all_visible;       // :1623
	int wpass;             // get_dist_to_camera_in_tiles(0) > 0.5*tt_grass_scale_factor (:3424)
};
// d: get_mesh_bcube() of the tile (line_tile_box), x1 / y1: its first mesh cell
TERRA_HD grass_view_tile_t grass_view_tile(grass_view_consts_t const &c, float const d[3][2], int x1, int y1, float mzmin, float mzmax, float radius) {
	grass_view_tile_t o;
	float const *cam = c.v.pos;
	o.llcx = d[0][0]; o.llcy = d[1][0];
	float dsq = 0.0f; // get_min_dist_to_pt(camera, xy_only=0, mesh_only=1)
	for (int i = 0; i < 3; ++i) {
		float const dist = max_std(0.0f, max_std(d[i][0] - cam[i], cam[i] - d[i][1]));
		dsq += dist*dist;
	}
	o.in_range = !(sqrtf(dsq) > c.grass_thresh);
	o.bg_thresh_sq = 0.0f; o.all_visible = 0; o.wpass = 0;
	if (!o.in_range) return o; // too far away to draw (:1612): nothing below is read, and most tiles of a large batch end here
	float const SQRT2 = 1.41421356237309515f; // float const SQRT2 = sqrt(2.0) (src/3DWorld.h:132)
	float const block_grass_thresh = c.grass_thresh + (SQRT2*radius)/(float)c.dim;
	o.bg_thresh_sq = block_grass_thresh*block_grass_thresh;
	o.all_visible = view_cube_completely_visible(c.v, d);
	// get_center() (src/tiled_mesh.h:229-231): get_xval(((x1 + x2) >> 1) + (xoff - xoff2)), x2 = x1 + S; integer steps wrap as in the reference binary
	int const mx = (int)((uint32_t)x1 + (uint32_t)x1 + (uint32_t)c.S) >> 1, my = (int)((uint32_t)y1 + (uint32_t)y1 + (uint32_t)c.S) >> 1;
	float const ccx = -c.xss + c.DX_VAL*(float)(int)((uint32_t)mx + (uint32_t)c.dxoff), ccy = -c.yss + c.DY_VAL*(float)(int)((uint32_t)my + (uint32_t)c.dyoff);
	float const ccz = 0.5f*(mzmin + mzmax);
	float const dist = sqrtf((cam[0] - ccx)*(cam[0] - ccx) + (cam[1] - ccy)*(cam[1] - ccy) + (cam[2] - ccz)*(cam[2] - ccz)); // p2p_dist(get_camera_pos(), get_center())
	float const in_tiles = (max_std(0.0f, dist - radius)/c.scaled_tile_radius)*(float)6; // get_rel_dist_to_camera(0)*TILE_RADIUS
	o.wpass = ((double)in_tiles > 0.5*(double)c.tt) ? 1 : 0;
	return o;
}

// ---- the back-face test of a near block (:1636-1643): true = every one of its 25 texels faces away from adj_camera.  zt: the tile's (S + 2)^2 zvals.
// The block's 6 x 6 zvals are loaded before the first product is formed: a texel reads its own, its +x and its +y neighbour, neighbours share them.
// S is a multiple of 4 here (the caller refuses others): rows and columns up to (dim*4 + 1) = S + 1 exist.
TERRA_HD bool grass_view_back_facing(grass_view_consts_t const &c, grass_view_tile_t const &t, uint32_t x, uint32_t y, float const *zt) {
	uint32_t const zvsize = (uint32_t)c.S + 2u, x0 = x*GRASS_VIEW_BLOCK, y0 = y*GRASS_VIEW_BLOCK;
	float z[6][6];
	for (uint32_t r = 0; r < 6; ++r) {for (uint32_t q = 0; q < 6; ++q) {z[r][q] = zt[(y0 + r)*zvsize + x0 + q];}}
	bool back_facing = true;
	for (uint32_t r = 0; r < 5; ++r) {
		for (uint32_t q = 0; q < 5; ++q) {
			uint32_t const xx = x0 + q, yy = y0 + r;
			float const nx = c.DY_VAL*(z[r][q] - z[r][q + 1]), ny = c.DX_VAL*(z[r][q] - z[r + 1][q]), nz = c.dxdy; // get_norm_not_normalized(ix)
			float const vx = c.v.pos[0] - (t.llcx + (float)xx*c.DX_VAL), vy = c.v.pos[1] - (t.llcy + (float)yy*c.DY_VAL), vz = c.adj_z - z[r][q];
			back_facing = back_facing && (nx*vx + ny*vy + nz*vz < 0.0f);
		}
	}
	return back_facing;
}

// ---- the block test (:1628-1650): GRASS_VIEW_DROPPED or lod*nrnd + bix
TERRA_HD uint32_t grass_view_block(grass_view_consts_t const &c, grass_view_tile_t const &t, uint32_t x, uint32_t y, uint32_t ix, float zmin, float zmax, float const *zt) {
	if (ix == 0) return GRASS_VIEW_DROPPED; // empty block
	float const bcx1 = t.llcx + (float)x*c.dx_step, bcy1 = t.llcy + (float)y*c.dy_step;
	float const d[3][2] = {{bcx1, bcx1 + c.dx_step}, {bcy1, bcy1 + c.dy_step}, {zmin, zmax + c.grass_length}};
	float const dist_sq = view_closest_dist_sq(d, c.v.pos[0], c.v.pos[1], c.v.pos[2]);
	if (dist_sq > t.bg_thresh_sq || (!t.all_visible && !view_cube_visible(c.v, d))) return GRASS_VIEW_DROPPED;
	if ((double)dist_sq < 0.56*(double)t.bg_thresh_sq) { // only do back face culling on nearby blocks
		if (grass_view_back_facing(c, t, x, y, zt)) return GRASS_VIEW_DROPPED;
	}
	uint32_t const lod = f2u_x86(c.lod_scale*sqrtf(dist_sq)), lod_level = (lod < GRASS_VIEW_LODS - 1u) ? lod : GRASS_VIEW_LODS - 1u;
	uint32_t const bix = ix - 1u;
	if (bix >= c.nrnd) return GRASS_VIEW_DROPPED; // assert(bix < num_rnd_grass_blocks): skipped
	return lod_level*c.nrnd + bix;
}
// the aux word of a kept block: bits 0-15 y*dim + x, 16-18 the LOD, 19-31 bix
TERRA_HD uint32_t grass_view_aux(grass_view_consts_t const &c, uint32_t block, uint32_t key) {return block | ((key / c.nrnd) << 16) | ((key % c.nrnd) << 19);}

// ---- the literal body: tile t of the batch runs the reference's loops; its per-LOD, per-bix lists are the groups' counts, then their offsets, then a second walk
// in the same scan order that appends every kept block to its group.  keys: a key per block (16 bits: dropped, or lod*nrnd + bix); offs: a running offset per group;
// nb = dim^2 blocks, nbins = GRASS_VIEW_LODS*nrnd groups and zn = (S + 2)^2 zvals of a tile, as the caller sized the arrays (arguments: computed here they cost the
// device build registers it spills)
TERRA_HD void grass_view_tile_literal(grass_view_consts_t const &c, grass_view_io_t const &io, int32_t const *tile_xy, uint32_t capacity, uint16_t *keys, uint32_t *offs,
	size_t nb, size_t nbins, size_t zn, size_t t)
{
	terra_tile_stats const &st = io.stats[t];
	line_box_t const box = grass_view_box(c, tile_xy[2*t], tile_xy[2*t + 1], st.mzmin, st.mzmax);
	grass_view_tile_t const tl = grass_view_tile(c, box.d, box.x1, box.y1, st.mzmin, st.mzmax, st.radius);
	uint32_t *const gc = io.group_counts + t*nbins, *const of = offs + t*nbins;
	uint16_t *const ky = keys + t*nb;
	for (size_t b = 0; b < nbins; ++b) {gc[b] = 0u;}
	bool has_grass = false;
	if (!(io.skip && io.skip[t]) && tl.in_range) {
		grass_block_pod_t const *const bl = io.blocks + t*nb;
		for (uint32_t y = 0; y < c.dim; ++y) {
			for (uint32_t x = 0; x < c.dim; ++x) {
				grass_block_pod_t const gb = bl[y*c.dim + x];
				has_grass = has_grass || gb.ix != 0u;
				uint32_t const key = grass_view_block(c, tl, x, y, gb.ix, gb.zmin, gb.zmax, io.zvals + t*zn);
				ky[y*c.dim + x] = (uint16_t)key;
				if (key != GRASS_VIEW_DROPPED) {++gc[key];}
			}
		}
	}
	if (!has_grass) { // skipped, too far away (:1612) or !has_grass() (:1609, :3422)
		io.counts[t] = 0u;
		if (io.pass) {io.pass[t] = GRASS_VIEW_NO_PASS;}
		return;
	}
	uint32_t total = 0;
	for (size_t b = 0; b < nbins; ++b) {of[b] = total; total += gc[b];}
	for (uint32_t i = 0; i < (uint32_t)nb; ++i) {
		uint32_t const key = ky[i];
		if (key == GRASS_VIEW_DROPPED) continue;
		uint32_t const rank = of[key]++;
		if (rank >= capacity) continue;
		float *const o = io.insts + (t*capacity + rank)*2;
		o[0] = (float)(i % c.dim)*c.dx_step; o[1] = (float)(i / c.dim)*c.dy_step; // emplace_back(x*dx_step, y*dy_step) (:1651)
		if (io.aux) {io.aux[t*capacity + rank] = grass_view_aux(c, i, key);}
	}
	io.counts[t] = total;
	if (io.pass) {io.pass[t] = (uint8_t)tl.wpass;}
}

} // namespace terra
