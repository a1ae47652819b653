// terra_cxx.hpp -- engine-side C++ mirror of the reference's call surface over the C ABI (include/terra.h).
//
// Same names, argument meaning and blocking behaviour as the 3DWorld interfaces they stand in for, so the callers
// (tile_t::create_zvals, heightmap_t::proc_gen, gen_mesh, voxel_manager) stay untouched:
//   mesh_xy_grid_cache_t  src/mesh.h:22-45        (build_arrays / enable_glaciate / eval_index / clear_context / free_cshader)
//   apply_erosion         src/function_registry.h:354, src/erosion.cpp:14
//   create_procedural     src/voxels.cpp:278      (fill part)
// Header only; link with -lterra_hip.  The reference asserts on misuse; so does this header (terra_status < 0 -> assert + message).
#pragma once
#include "terra.h"
#include <vector>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstddef>

namespace terra_cxx {

inline void check(int rc, char const *what) {
	if (rc < 0) {std::fprintf(stderr, "terra: %s failed (%d): %s\n", what, rc, terra_last_error()); assert(!"terra call failed"); std::abort();}
}

// process-wide context, like the engine's process-wide globals; created on first use on GPU 0 (TERRA_DEVICE overrides)
inline terra_ctx *default_ctx() {
	static terra_ctx *ctx = [] {
		terra_ctx *c = nullptr;
		char const *dev = std::getenv("TERRA_DEVICE");
		check(terra_create(&c, dev ? std::atoi(dev) : 0), "terra_create");
		return c;
	}();
	return ctx;
}

// Call once after the engine has loaded its config and derived its globals (after gen_scene()/estimate_zminmax()):
// copies the config-file values and the derived globals across the boundary.  Alternatively terra_init_scene() derives them itself.
inline void set_engine_state(terra_config const &cfg, terra_state const &st) {
	check(terra_set_config(default_ctx(), &cfg), "terra_set_config");
	check(terra_set_state(default_ctx(), &st), "terra_set_state");
}

class mesh_xy_grid_cache_t { // src/mesh.h:22-45
	terra_gen *gen = nullptr;
	unsigned cur_nx = 0, cur_ny = 0;
	terra_gen *handle() {if (!gen) {check(terra_gen_create(default_ctx(), &gen), "terra_gen_create");} return gen;}
public:
	mesh_xy_grid_cache_t() = default;
	mesh_xy_grid_cache_t(mesh_xy_grid_cache_t const &) = delete;
	mesh_xy_grid_cache_t &operator=(mesh_xy_grid_cache_t const &) = delete;
	~mesh_xy_grid_cache_t() {clear_context();}
	// returns 1 when values are available, 0 when no_wait and the job was only launched (call again with the same arguments)
	bool build_arrays(float x0, float y0, float dx, float dy, unsigned nx, unsigned ny, bool cache_values=0, bool force_sine_mode=0, bool no_wait=0) {
		assert(nx > 0 && ny > 0);
		unsigned const flags = (cache_values ? TERRA_GEN_CACHE_VALUES : 0u) | (force_sine_mode ? TERRA_GEN_FORCE_SINE : 0u) | (no_wait ? TERRA_GEN_NO_WAIT : 0u);
		int const rc = terra_gen_build_arrays(handle(), x0, y0, dx, dy, nx, ny, flags, 0);
		check(rc, "build_arrays");
		cur_nx = nx; cur_ny = ny;
		return rc != 0;
	}
	void enable_glaciate() {check(terra_gen_enable_glaciate(handle()), "enable_glaciate");}
	// min_start_sin > start_eval_sin (tile_t::create_texture passes 50, src/tiled_mesh.cpp:1114; grass.cpp:819-820): the library evaluates the grid once more from
	// that term on the first such call and serves the following ones from it
	float eval_index(unsigned x, unsigned y, int min_start_sin=0, bool use_cache=1) const {
		assert(x < cur_nx && y < cur_ny);
		return terra_gen_eval_index(gen, x, y, min_start_sin, use_cache ? 1 : 0);
	}
	float const *device_values() const {return terra_gen_device_values(gen);} // extension: the grid stays in HBM for erosion / normals
	void clear_context() {if (gen) {terra_gen_destroy(gen); gen = nullptr;}}
	void free_cshader() {} // nothing GL-side to release
};

// src/erosion.cpp:14 -- in place on a host buffer, blocking, silent no-op when disabled
inline void apply_erosion(float *heightmap, int xsize, int ysize, float min_zval, unsigned num_iters) {
	check(terra_apply_erosion(default_ctx(), heightmap, xsize, ysize, min_zval, num_iters), "apply_erosion");
}

// heightmap_t::proc_gen (src/heightmap.cpp:130-151) as one call: the texture's 16-bit pixels + {min_z, dz} for set_mesh_height_scales_for_zval_range(min_z, dz/255)
inline void heightmap_proc_gen(unsigned width, unsigned height, unsigned erosion_iters, unsigned char *pixels16, float &min_z, float &dz) {
	float range[2] = {0.0f, 0.0f};
	check(terra_heightmap_proc_gen(default_ctx(), width, height, erosion_iters, pixels16, range), "heightmap_proc_gen");
	min_z = range[0]; dz = range[1];
}

// tile_t::create_zvals for a batch of tiles (src/tiled_mesh.cpp:467-546) at the tile size S = MESH_X_SIZE (terra_tile_size): zvals n*(S+2)*(S+2), stats n,
// normals n*(S+1)*(S+1)*4 (optional) -- 130 / 129 at S = 128
// ---- eval_mesh_sin_terms (src/mesh_gen.cpp:797-805): point query, evaluated on the host
inline float eval_mesh_sin_terms(float xv, float yv) {
	float z = 0.0f;
	check(terra_eval_mesh_sin_terms(default_ctx(), xv, yv, &z), "eval_mesh_sin_terms");
	return z;
}
// ---- eval_mesh_sin_terms_scaled (src/mesh_gen.cpp:807-813) and get_exact_zval (:816-847): the all-modes point queries; a batch at a time where the caller has one
// (biome parameters of a tile's corners src/tiled_mesh.cpp:332-338, voxel terrain src/voxels.cpp:434), else one point
inline void eval_mesh_sin_terms_scaled(float const *xy, unsigned n, float xy_scale, float *out) {
	check(terra_eval_points(default_ctx(), xy, n, TERRA_POINTS_SCALED, xy_scale, 0, 0, 0, out), "eval_mesh_sin_terms_scaled");
}
inline float eval_mesh_sin_terms_scaled(float xval, float yval, float xy_scale) {
	float const xy[2] = {xval, yval}; float z = 0.0f;
	eval_mesh_sin_terms_scaled(xy, 1, xy_scale, &z);
	return z;
}
inline void get_exact_zval(float const *xy, unsigned n, float *out, bool no_xyoff = false, int xoff2 = 0, int yoff2 = 0) { // xoff2 / yoff2: the reference's scroll-offset globals
	check(terra_eval_points(default_ctx(), xy, n, TERRA_POINTS_EXACT, 1.0f, no_xyoff ? 1 : 0, xoff2, yoff2, out), "get_exact_zval");
}
inline float get_exact_zval(float xval, float yval, bool no_xyoff = false, int xoff2 = 0, int yoff2 = 0) {
	float const xy[2] = {xval, yval}; float z = 0.0f;
	get_exact_zval(xy, 1, &z, no_xyoff, xoff2, yoff2);
	return z;
}
// ---- glaciate() over the ground mesh (src/mesh_gen.cpp:388-404): in place on a device buffer, returns zbottom / ztop
inline void glaciate_mesh_dev(float *d_mesh, unsigned nx, unsigned ny, int xoff2, int yoff2, float &zbottom, float &ztop) {
	float zz[2] = {0.0f, 0.0f};
	check(terra_glaciate_mesh_dev(default_ctx(), d_mesh, nx, ny, xoff2, yoff2, zz), "glaciate");
	zbottom = zz[0]; ztop = zz[1];
}

inline void tiles_create_zvals(int const *tile_xy, unsigned n, unsigned erosion_iters_tt, float *zvals, terra_tile_stats *stats, unsigned char *normals=nullptr, float *min_normal_z=nullptr) {
	check(terra_tiles_create_zvals(default_ctx(), tile_xy, n, erosion_iters_tt, zvals, stats, normals, min_normal_z), "tiles_create_zvals");
}

// ---- tile_t::upload_normal_texture (src/tiled_mesh.cpp:865-880) and the sub-block / water-bbox loop of create_zvals (:517-541) over zvals the engine already has
inline void tiles_upload_normal_texture(int const *tile_xy, unsigned n, float const *zvals, terra_tile_stats *stats, unsigned char *normals, float *min_normal_z=nullptr) {
	check(terra_tiles_post(default_ctx(), tile_xy, n, zvals, stats, normals, min_normal_z), "upload_normal_texture");
}

// ---- tile_t::calc_shadows_for_light (src/tiled_mesh.cpp:664-692) for a batch and one light: smask [n][130][130] gets the MESH_SHADOW bits
inline void tiles_mesh_shadows(int const *tile_xy, unsigned n, float const *zvals, float const lpos[3], unsigned char *smask) {
	check(terra_tiles_mesh_shadows(default_ctx(), tile_xy, n, zvals, lpos, smask), "calc_mesh_shadows");
}
// ---- terrain_hmap_manager: serve tiles from a heightmap texture that is already on the device (src/heightmap.cpp:385-407, src/mesh_gen.cpp:125-131)
inline void use_heightmap_texture(unsigned char const *d_pixels, int width, int height, int ncolors, float min_z, float dz) {
	check(terra_hmap_set_dev(default_ctx(), d_pixels, width, height, ncolors), "terrain_hmap_manager");
	if (d_pixels) {check(terra_set_mesh_height_scales_for_zval_range(default_ctx(), min_z, dz), "set_mesh_height_scales_for_zval_range");}
}
// ---- heightmap_t::postprocess_height (src/heightmap.cpp:117-128) on the loaded image: `data` = texture_t::data (width*height*ncolors bytes, host), eroded in place with
// erosion_iters_tt droplets; mesh_file_scale / mesh_file_tz as the config line `mh_filename <png> <scale> <tz>` set them.  Asserts like the reference when a value leaves [0, 256)
inline void heightmap_postprocess_height(unsigned char *data, unsigned width, unsigned height, int ncolors, unsigned erosion_iters_tt, float mesh_file_scale, float mesh_file_tz) {
	if (erosion_iters_tt == 0) return; // no erosion or cities => no need to update height values
	terra_ctx *ctx = default_ctx();
	size_t const bytes = (size_t)width*height*(size_t)ncolors;
	void *d_pixels = nullptr;
	check(terra_set_mesh_file_scale(ctx, mesh_file_scale, mesh_file_tz), "mh_filename scale");
	check(terra_malloc(ctx, &d_pixels, bytes), "postprocess_height");
	int rc = terra_memcpy_h2d(ctx, d_pixels, data, bytes);
	unsigned bad = 0;
	if (rc == 0) {rc = terra_heightmap_postprocess_dev(ctx, (unsigned char *)d_pixels, width, height, ncolors, erosion_iters_tt, nullptr, &bad);}
	if (rc == 0) {rc = terra_memcpy_d2h(ctx, data, d_pixels, bytes);}
	terra_free(ctx, d_pixels);
	check(rc, "postprocess_height");
	assert(bad == 0); // assert(v >= 0.0 && v < 256.0), src/heightmap.cpp:210
	(void)bad;
}
// ---- heightmap_t::write_png / texture_t::load_png for grayscale heightmaps (src/image_io.cpp:493-605)
inline void write_heightmap_png(char const *fn, unsigned char const *pixels, unsigned width, unsigned height, int ncolors) {
	check(terra_heightmap_write_png(fn, pixels, width, height, ncolors), "write_png");
}

// ---- read_mesh / write_mesh (src/mesh_gen.cpp:895-965): the ground mesh's text file.  Same return value as the reference (0: the file is missing, short or of another size);
// mesh_height is the engine's float ** matrix of MESH_Y_SIZE rows.  After read_mesh copy zmin / zmax / zmax_est / water_plane_z back from terra_get_state().
inline bool read_mesh(char const *filename, float zmm, float **mesh_height, unsigned mesh_x_size, unsigned mesh_y_size, float &zbottom, float &ztop) {
	if (filename == nullptr) return 0;
	std::vector<float> m((size_t)mesh_x_size*mesh_y_size);
	float zz[2];
	if (terra_read_mesh(default_ctx(), filename, zmm, m.data(), mesh_x_size, mesh_y_size, zz) != TERRA_OK) {std::fprintf(stderr, "read_mesh: %s\n", terra_last_error()); return 0;}
	for (unsigned i = 0; i < mesh_y_size; ++i) {for (unsigned j = 0; j < mesh_x_size; ++j) {mesh_height[i][j] = m[(size_t)i*mesh_x_size + j];}}
	zbottom = zz[0]; ztop = zz[1];
	return 1;
}
inline bool write_mesh(char const *filename, float const *const *mesh_height, unsigned mesh_x_size, unsigned mesh_y_size) {
	if (filename == nullptr || mesh_height == nullptr) return 0;
	std::vector<float> m((size_t)mesh_x_size*mesh_y_size);
	for (unsigned i = 0; i < mesh_y_size; ++i) {for (unsigned j = 0; j < mesh_x_size; ++j) {m[(size_t)i*mesh_x_size + j] = mesh_height[i][j];}}
	return terra_write_mesh(filename, m.data(), mesh_x_size, mesh_y_size) == TERRA_OK;
}

// ---- tile_t::calc_mesh_ao_lighting (src/tiled_mesh.cpp:586-661) for a batch: zvals [n][130][130] -> ao_lighting [n][129][129]
inline void tiles_ao_lighting(int const *tile_xy, unsigned n, float const *zvals, unsigned char *ao) {
	check(terra_tiles_ao_lighting(default_ctx(), tile_xy, n, zvals, ao), "calc_mesh_ao_lighting");
}
// ---- tile_t::create_texture's weights (src/tiled_mesh.cpp:1071-1240, terrain-only branch) for a batch: zvals [n][130][130] -> mesh_weight_data
// [n][129][129][4], grass_blocks [n][32][32] (may be null), has_any_grass [n] (may be null); set_landscape = the globals it reads (vegetation, ...)
inline void set_landscape(terra_landscape const &params) {check(terra_set_landscape(default_ctx(), &params), "set_landscape");}
inline void tiles_create_weights(int const *tile_xy, unsigned n, float const *zvals, unsigned char *mesh_weight_data, terra_grass_block *grass_blocks, unsigned char *has_any_grass) {
	check(terra_tiles_create_weights(default_ctx(), tile_xy, n, zvals, mesh_weight_data, grass_blocks, has_any_grass), "create_texture");
}
// tile_draw_t::add_or_remove_grass_at (src/tiled_mesh.cpp:3771-3774): tile_t::add_or_remove_grass_at on every tile of a batch whose weights / grass blocks the
// caller holds (tiles_create_weights' layouts), in place; dxoff / dyoff = xoff - xoff2 / yoff - yoff2; is_distant and ranges may be null.  updated[t] / ranges[t]
// = {xl, yl, xh, yh} drive the caller's flowers.update_subrange and create_or_update_weight_tex
inline void tiles_add_or_remove_grass_at(int const *tile_xy, unsigned n, int dxoff, int dyoff, float const *zvals, terra_tile_stats const *stats, unsigned char const *is_distant,
	float const pos[3], float rradius, bool add_grass, int brush_shape, float brush_weight, unsigned char *mesh_weight_data, terra_grass_block *grass_blocks,
	unsigned char *updated, unsigned *ranges = nullptr)
{
	terra_grass_brush const b = {{pos[0], pos[1], pos[2]}, rradius, add_grass ? 1 : 0, brush_shape, brush_weight};
	check(terra_tiles_edit_grass(default_ctx(), tile_xy, n, dxoff, dyoff, zvals, stats, is_distant, &b, mesh_weight_data, grass_blocks, updated, ranges), "add_or_remove_grass_at");
}
// The engine's tile batch as the line queries read it: tile_xy on the host, zvals / stats (terra_tiles_create_zvals_dev's) and is_distant (or null) on the device
struct tile_batch_dev_t {int const *tile_xy; unsigned n; int dxoff, dyoff; float const *d_zvals; terra_tile_stats const *d_stats; unsigned char const *d_is_distant;};
// one line against the batch (only_tile >= 0: against that batch tile alone, tile_t::line_intersect_mesh); the line goes up and the 32-byte record comes back.
// The staging buffer d_io is one per process, allocated on first use and never freed, like default_ctx(): the wrappers serve the engine's single-threaded
// frame loop; threads that query concurrently call terra_tiles_line_intersect_dev with buffers of their own
inline terra_line_hit tiles_line_intersect(tile_batch_dev_t const &b, float const v1[3], float const v2[3], int only_tile = -1) {
	struct io_t {float line[6]; int32_t only; int32_t pad; terra_line_hit hit;};
	static void *d_io = [] {void *p = nullptr; check(terra_malloc(default_ctx(), &p, sizeof(io_t)), "terra_malloc"); return p;}();
	io_t const in = {{v1[0], v1[1], v1[2], v2[0], v2[1], v2[2]}, only_tile, 0, {}};
	io_t *d = (io_t *)d_io;
	check(terra_memcpy_h2d(default_ctx(), d, &in, offsetof(io_t, hit)), "line_intersect_mesh");
	check(terra_tiles_line_intersect_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, b.d_zvals, b.d_stats, b.d_is_distant, d->line, &d->only, 1, &d->hit), "line_intersect_mesh");
	terra_line_hit h;
	check(terra_memcpy_d2h(default_ctx(), &h, &d->hit, sizeof(h)), "line_intersect_mesh");
	return h;
}
// tile_draw_t::line_intersect_mesh (src/tiled_mesh.cpp:3582-3605) with inc_trees = 0: t, the batch index of the tile (for intersected_tile; -1 on a miss, as the
// reference's nullptr) and the cell's xpos / ypos (left as they were on a miss, as the reference leaves them)
inline bool tile_draw_line_intersect_mesh(tile_batch_dev_t const &b, float const v1[3], float const v2[3], float &t, int &tile, int &xpos, int &ypos) {
	terra_line_hit const h = tiles_line_intersect(b, v1, v2);
	t = h.t;
	tile = h.tile;
	if (h.hit) {xpos = h.xpos; ypos = h.ypos;}
	return h.hit != 0;
}
// line_intersect_tiled_mesh (src/tiled_mesh.cpp:3954-3957 -> :3643-3648) with inc_trees = 0: p_int = v1 + t*(v2 - v1) on a hit
inline bool line_intersect_tiled_mesh(tile_batch_dev_t const &b, float const v1[3], float const v2[3], float p_int[3]) {
	terra_line_hit const h = tiles_line_intersect(b, v1, v2);
	if (h.hit) {p_int[0] = h.p_int[0]; p_int[1] = h.p_int[1]; p_int[2] = h.p_int[2];}
	return h.hit != 0;
}
// The same with the reference's inc_trees argument: inc_trees != 0 adds the pine records of `trees` (terra_tiles_line_intersect_trees_dev).  Of `trees` the device
// arrays pine / pine_counts / trunk_override, pine_capacity, ptree_xoff2 / ptree_yoff2 and tree_depth_scale are the caller's; zvals, stats, is_distant, dxoff and
// dyoff are taken from the batch.  With inc_trees == 0 the record's first 32 bytes are tiles_line_intersect's and no tree is looked at
inline terra_line_tree_hit tiles_line_intersect(tile_batch_dev_t const &b, terra_line_trees_in const &trees, float const v1[3], float const v2[3], float inc_trees, int only_tile = -1) {
	struct io_t {float line[6]; int32_t only; int32_t pad; terra_line_tree_hit hit;};
	static void *d_io = [] {void *p = nullptr; check(terra_malloc(default_ctx(), &p, sizeof(io_t)), "terra_malloc"); return p;}();
	io_t const in = {{v1[0], v1[1], v1[2], v2[0], v2[1], v2[2]}, only_tile, 0, {}};
	io_t *d = (io_t *)d_io;
	terra_line_trees_in a = trees;
	a.zvals = b.d_zvals; a.stats = b.d_stats; a.is_distant = b.d_is_distant; a.dxoff = b.dxoff; a.dyoff = b.dyoff;
	if (inc_trees == 0.0f) {a.pine = nullptr; a.pine_counts = nullptr; a.trunk_override = nullptr; a.pine_capacity = 0;}
	check(terra_memcpy_h2d(default_ctx(), d, &in, offsetof(io_t, hit)), "line_intersect_mesh");
	check(terra_tiles_line_intersect_trees_dev(default_ctx(), b.tile_xy, b.n, &a, d->line, &d->only, 1, &d->hit), "line_intersect_mesh");
	terra_line_tree_hit h;
	check(terra_memcpy_d2h(default_ctx(), &h, &d->hit, sizeof(h)), "line_intersect_mesh");
	return h;
}
// tile_draw_t::line_intersect_mesh(v1, v2, t, intersected_tile, xpos, ypos, inc_trees): a tree hit leaves xpos / ypos at 0, as the reference's new_xpos / new_ypos
inline bool tile_draw_line_intersect_mesh(tile_batch_dev_t const &b, terra_line_trees_in const &trees, float const v1[3], float const v2[3], float &t, int &tile, int &xpos, int &ypos,
	float inc_trees, terra_line_tree_hit *hit_out = nullptr)
{
	terra_line_tree_hit const h = tiles_line_intersect(b, trees, v1, v2, inc_trees);
	t = h.t;
	tile = h.tile;
	if (h.hit) {xpos = h.xpos; ypos = h.ypos;}
	if (hit_out) {*hit_out = h;}
	return h.hit != 0;
}
// line_intersect_tiled_mesh(v1, v2, p_int, inc_trees) (src/tiled_mesh.cpp:3954-3957): what the hit-scan weapon path calls with inc_trees = 1 (src/Gameplay.cpp:2143)
inline bool line_intersect_tiled_mesh(tile_batch_dev_t const &b, terra_line_trees_in const &trees, float const v1[3], float const v2[3], float p_int[3], float inc_trees) {
	terra_line_tree_hit const h = tiles_line_intersect(b, trees, v1, v2, inc_trees);
	if (h.hit) {p_int[0] = h.p_int[0]; p_int[1] = h.p_int[1]; p_int[2] = h.p_int[2];}
	return h.hit != 0;
}
// ---- sphere collisions and tree box tests against the resident containers (terra_tiles_sphere_collide_dev / terra_tiles_cube_int_trees_dev): `in` holds the device
// arrays of the three containers as the placements left them.  The one-query forms below go through a staging buffer of the process, like tiles_line_intersect; a
// frame's queries (the player, the physics objects, the animals) are better collected and asked in one terra_tiles_sphere_collide_dev call.
// tile_draw_t::check_sphere_collision (src/tiled_mesh.cpp:3566-3569): pos is modified; only_tile >= 0: tile_t::check_sphere_collision of that batch tile
inline bool tile_draw_check_sphere_collision(tile_batch_dev_t const &b, terra_collide_in const &in, float pos[3], float radius, int only_tile = -1,
	bool inc_dtrees = 1, bool inc_ptrees = 1, bool inc_scenery = 1, terra_sphere_hit *hit_out = nullptr)
{
	struct io_t {terra_sphere_query q; terra_sphere_hit hit;};
	static void *d_io = [] {void *p = nullptr; check(terra_malloc(default_ctx(), &p, sizeof(io_t)), "terra_malloc"); return p;}();
	io_t io = {{{pos[0], pos[1], pos[2]}, radius, only_tile, (inc_dtrees ? (unsigned)TERRA_COLL_INC_DTREES : 0u) | (inc_ptrees ? (unsigned)TERRA_COLL_INC_PTREES : 0u) |
		(inc_scenery ? (unsigned)TERRA_COLL_INC_SCENERY : 0u)}, {}};
	io_t *d = (io_t *)d_io;
	check(terra_memcpy_h2d(default_ctx(), &d->q, &io.q, sizeof(io.q)), "terra_memcpy_h2d");
	check(terra_tiles_sphere_collide_dev(default_ctx(), b.tile_xy, b.n, &in, &d->q, 1, &d->hit), "tile_draw_t::check_sphere_collision");
	check(terra_memcpy_d2h(default_ctx(), &io.hit, &d->hit, sizeof(io.hit)), "terra_memcpy_d2h");
	pos[0] = io.hit.pos[0]; pos[1] = io.hit.pos[1]; pos[2] = io.hit.pos[2];
	if (hit_out) {*hit_out = io.hit;}
	return (io.hit.word & (TERRA_COLL_HIT_PINE | TERRA_COLL_HIT_DECID | TERRA_COLL_HIT_SCENERY)) != 0;
}
// sphere_int_tiled_terrain (src/tiled_mesh.cpp: the call Physics.cpp:858 makes): check_sphere_collision on a copy that is written back
inline bool sphere_int_tiled_terrain(tile_batch_dev_t const &b, terra_collide_in const &in, float pos[3], float radius) {return tile_draw_check_sphere_collision(b, in, pos, radius);}
// cube_int_tiled_terrain_trees = tile_draw_t::check_cube_int_trees (:3576-3579): cube = x1 x2 y1 y2 z1 z2 in camera space
inline bool cube_int_tiled_terrain_trees(tile_batch_dev_t const &b, terra_collide_in const &in, float const cube[6]) {
	struct io_t {float cube[6]; int32_t tile; uint8_t res; uint8_t pad[3];};
	static void *d_io = [] {void *p = nullptr; check(terra_malloc(default_ctx(), &p, sizeof(io_t)), "terra_malloc"); return p;}();
	io_t io = {{cube[0], cube[1], cube[2], cube[3], cube[4], cube[5]}, -1, 0, {0, 0, 0}};
	io_t *d = (io_t *)d_io;
	check(terra_memcpy_h2d(default_ctx(), d->cube, io.cube, sizeof(io.cube)), "terra_memcpy_h2d");
	check(terra_tiles_cube_int_trees_dev(default_ctx(), b.tile_xy, b.n, &in, d->cube, nullptr, 1, &d->res, nullptr), "tile_draw_t::check_cube_int_trees");
	check(terra_memcpy_d2h(default_ctx(), &io.res, &d->res, 1), "terra_memcpy_d2h");
	return (io.res & TERRA_CUBE_INT_HIT) != 0;
}
// ---- the tree map of a batch and the two textures that read it (what tile_t::pre_draw runs after register_tree_change, src/tiled_mesh.cpp:1900-1907), on device
// arrays.  tile_t::apply_tree_ao_shadows (:820-828) for every tile: the engine's add_tree_ao_shadow (:749) appends terra_tree_splat{pos.x, pos.y, tradius} to the
// tile's list instead of looping over texels, and this runs the lists (tile t: d_splats[first[t] .. first[t+1]), first on the host).  reset = false is a later
// push_tree_ao_shadow round on the resident map.  d_updated[t] (may be null) sets the tile's sun / moon_shadows_invalid and recalc_tree_grass_weights
inline void tiles_apply_tree_ao_shadows(tile_batch_dev_t const &b, terra_tree_splat const *d_splats, unsigned const *first, bool reset, unsigned char *d_tree_map, unsigned char *d_updated = nullptr) {
	check(terra_tiles_tree_map_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, b.d_is_distant, d_splats, first, reset ? 1 : 0, d_tree_map, d_updated), "apply_tree_ao_shadows");
}
// tile_t::upload_shadow_map_texture (:882-913) up to the texture upload: d_shadow_data [n][S+1][S+1][4]; d_ao_lighting / d_tree_map may be null (ao_lighting.empty() /
// tree_map.empty()), a smask may be null when its light is down or mesh_shadows_enabled() is false
inline void tiles_upload_shadow_map_texture(unsigned n, unsigned char const *d_smask_sun, unsigned char const *d_smask_moon, unsigned char const *d_ao_lighting,
	unsigned char const *d_tree_map, float light_factor, bool mesh_shadows, unsigned char *d_shadow_data)
{
	check(terra_tiles_shadow_texture_dev(default_ctx(), n, d_smask_sun, d_smask_moon, d_ao_lighting, d_tree_map, light_factor, mesh_shadows ? 1 : 0, d_shadow_data), "upload_shadow_map_texture");
}
// the tail of tile_t::create_texture (:1325-1348): weight_data from mesh_weight_data and tree_map (null: the plain copy); d_weight_data may be d_mesh_weight_data
inline void tiles_create_texture_tree_weights(unsigned n, unsigned char const *d_mesh_weight_data, unsigned char const *d_tree_map, unsigned char *d_weight_data) {
	check(terra_tiles_tree_weights_dev(default_ctx(), n, d_mesh_weight_data, d_tree_map, d_weight_data), "create_texture");
}
// ---- pine / palm tree placement of a batch on device arrays.  The globals of src/sm_tree.cpp:29-33 go in once (set_tree_globals: sm_tree_density, tree_scale,
// tree_density_thresh, tree_type_rand_zone, tree_mode, force_tree_class, only_pine_palm_trees, rand_gen_index, enable_instanced_pine_trees() and the two ranges of
// num_insts_per_type); an engine that owns height_histogram passes it with terra_set_height_histogram.
inline void set_tree_globals(terra_tree_params const &p) {check(terra_set_tree_params(default_ctx(), &p), "set_tree_params");}
// small_tree_group::gen_trees (src/sm_tree.cpp:407-474, from :439 on) for every tile as tile_t::init_pine_tree_draw (src/tiled_mesh.cpp:1430-1437) calls it: xoff2 /
// yoff2 are the globals at that time (ptree_off.set_from_xyoff2()).  d_can_have_trees_false[t] != 0: can_have_trees() is false; b.d_stats (may be null):
// can_have_pine_palm_trees_in_zrange(mzmin, mzmax).  d_trees [n][capacity], d_counts [n]: the engine filters each record with check_valid_scenery_pos /
// point_inside_voxel_terrain and constructs the small_tree (instanced: from inst; else from height, width, type and the generator state rseed1 / rseed2)
inline void tiles_gen_trees(tile_batch_dev_t const &b, int xoff2, int yoff2, unsigned char const *d_can_have_trees_false, unsigned capacity, terra_tree_place *d_trees, unsigned *d_counts) {
	check(terra_tiles_place_trees_dev(default_ctx(), b.tile_xy, b.n, xoff2, yoff2, d_can_have_trees_false, b.d_stats, capacity, d_trees, d_counts), "gen_trees");
}
// small_tree_group::gen_trees_tt_within_radius (:477-502) as tile_t::add_new_trees (src/tiled_mesh.cpp:3805-3811) calls it: toff_dxoff / toff_dyoff = ptree_off's
// members (the call runs with xoff2 = -toff.dxoff), pos = pt_pos, is_square = (brush_shape == BSHAPE_CONST_SQ)
inline void tiles_gen_trees_tt_within_radius(tile_batch_dev_t const &b, int toff_dxoff, int toff_dyoff, unsigned char const *d_can_have_trees_false, float const pos[3], float radius,
	bool is_square, unsigned capacity, terra_tree_place *d_trees, unsigned *d_counts)
{
	check(terra_tiles_place_trees_brush_dev(default_ctx(), b.tile_xy, b.n, -toff_dxoff, -toff_dyoff, d_can_have_trees_false, b.d_stats, pos, radius, is_square ? 1 : 0, capacity, d_trees, d_counts),
		"gen_trees_tt_within_radius");
}
// ---- deciduous tree placement of a batch on device arrays.  The globals beyond set_tree_globals go in once (set_decid_globals: num_trees, shared_tree_data.size(),
// tree_slope_thresh and tree_types[].branch_size).
inline void set_decid_globals(terra_decid_params const &p) {check(terra_set_decid_params(default_ctx(), &p), "set_decid_params");}
// tree_cont_t::gen_deterministic (src/Tree.cpp:2153-2155) for every tile as tile_t::gen_decid_trees_if_needed (src/tiled_mesh.cpp:1536-1547) calls it: xoff2 / yoff2 are
// the globals at that time (dtree_off.set_from_xyoff2()); vegetation*get_avg_veg() and mesh_dz are taken from the landscape, the biome field and b.d_stats.
// d_can_have_trees_false[t] != 0: can_have_trees() is false; b.d_stats (may be null, then without cull and slope test): can_have_decid_trees_in_zrange(mzmin, mzmax) and
// mesh_dz; b.d_zvals: the tile heights adjust_tree_zval scans.  d_trees [n][capacity], d_counts [n]: the engine filters each record with check_valid_scenery_pos (on
// zval, the height before adjust_tree_zval) / point_inside_voxel_terrain, calls add_new_tree with tree_id and type, then rgen.set_state(rseed1, rseed2) and gen_tree
inline void tiles_gen_decid_trees(tile_batch_dev_t const &b, int xoff2, int yoff2, unsigned char const *d_can_have_trees_false, unsigned capacity, terra_decid_place *d_trees, unsigned *d_counts) {
	check(terra_tiles_place_decid_trees_dev(default_ctx(), b.tile_xy, b.n, xoff2, yoff2, d_can_have_trees_false, b.d_stats, b.d_stats ? b.d_zvals : nullptr, capacity, d_trees, d_counts), "gen_decid_trees");
}
// tree_cont_t::gen_trees_tt_within_radius (src/Tree.cpp:2209-2305) as tile_t::add_new_trees (src/tiled_mesh.cpp:3805-3811) calls it for decid_trees: toff_dxoff /
// toff_dyoff = dtree_off's members, pos = dt_pos, is_square = (brush_shape == BSHAPE_CONST_SQ) (passed on; the reference's function never reads it)
inline void tiles_gen_decid_trees_tt_within_radius(tile_batch_dev_t const &b, int toff_dxoff, int toff_dyoff, unsigned char const *d_can_have_trees_false, float const pos[3], float radius,
	bool is_square, unsigned capacity, terra_decid_place *d_trees, unsigned *d_counts)
{
	check(terra_tiles_place_decid_trees_brush_dev(default_ctx(), b.tile_xy, b.n, -toff_dxoff, -toff_dyoff, d_can_have_trees_false, b.d_stats, b.d_stats ? b.d_zvals : nullptr, pos, radius,
		is_square ? 1 : 0, capacity, d_trees, d_counts), "gen_decid_trees_tt_within_radius");
}
// ---- scenery placement of a batch on device arrays.  use_voxel_rocks goes in once (set_scenery_globals); tree_scale, tree_mode .. come from set_tree_globals.
inline void set_scenery_globals(terra_scenery_params const &p) {check(terra_set_scenery_params(default_ctx(), &p), "set_scenery_params");}
// scenery_group::gen (src/scenery.cpp:1263-1353, the cell loop) for every tile as tile_t::update_scenery (src/tiled_mesh.cpp:1568-1578) calls it: xoff2 / yoff2 are the
// globals at that time (scenery_off.set_from_xyoff2()); vegetation*get_avg_veg() is taken from the landscape and the biome field.  d_no_scenery[t] != 0: update_scenery
// returns before gen() (scenery_enabled, is_distant, dist_scale, is_visible).  d_objs [n][capacity], d_counts [n], d_kind_counts [n][TERRA_SCENERY_KINDS] (or null):
// the engine reserve()s from the kind counts, then for each record in order: builds the object of `kind` from the fields (for a rock_shape: set_state is not needed,
// gen_rock(48, 0.05/tree_scale, iv[0], iv[1]) re-seeds; for a leafy plant and a surface rock: global_rand_gen.set_state(rseed1, rseed2) before gen_leaves() / the
// surface cache), filters it with check_valid_scenery_pos and pushes it; then the city ponds and post_gen_setup as before
inline void tiles_gen_scenery(tile_batch_dev_t const &b, int xoff2, int yoff2, unsigned char const *d_no_scenery, unsigned capacity, terra_scenery_place *d_objs, unsigned *d_counts,
	unsigned *d_kind_counts)
{
	check(terra_tiles_place_scenery_dev(default_ctx(), b.tile_xy, b.n, xoff2, yoff2, d_no_scenery, capacity, d_objs, d_counts, d_kind_counts), "scenery_group::gen");
}
// ---- the flowers of a batch on device arrays.  flower_density, grass_length, grass_width, flower_color and no_grass() go in once (set_flower_globals).
inline void set_flower_globals(terra_flower_params const &p) {check(terra_set_flower_params(default_ctx(), &p), "set_flower_params");}
// flower_tile_manager_t::gen_flowers(weight_data, weights_tsize, x1 - xoff2, y1 - yoff2, 0) (src/grass.cpp:859-888) for every tile as tile_t::draw_flowers
// (src/tiled_mesh.cpp:1666-1677) calls it: d_weight_data is what tiles_create_texture_tree_weights left.  d_no_flowers[t] != 0 (or null): the tile is not generated
// (already generated, too far, a city tile with tsize_bitshift > 0).  d_flowers [n][capacity] records with flower_t's layout, d_aux (or null), d_counts [n]: the
// engine copies flowers[t][0 .. counts[t]) into the tile's vector and sets generated; check_vbo, create_verts_range and the drawing stay where they are
inline void tiles_gen_flowers(tile_batch_dev_t const &b, unsigned char const *d_no_flowers, unsigned char const *d_weight_data, unsigned capacity, terra_flower *d_flowers,
	unsigned *d_aux, unsigned *d_counts)
{
	check(terra_tiles_place_flowers_dev(default_ctx(), b.tile_xy, b.n, d_no_flowers, d_weight_data, capacity, d_flowers, d_aux, d_counts), "gen_flowers");
}
// the flowers' half of tile_t::add_or_remove_grass_at (src/tiled_mesh.cpp:3930-3937) on the resident records, after tiles_add_or_remove_grass_at's device form left
// d_updated / d_ranges: flowers.update_subrange when adding, flowers.clear_within(pos - flower_xlate, rradius, is_square) when removing.  d_generated[t] (or null: all):
// the tile's `generated`.  d_status[t]: 0 untouched, 1 edited (the engine clears the tile's VBO), 2 refused (a range that reaches texel row or column S)
inline void tiles_update_flowers_at(tile_batch_dev_t const &b, unsigned char const *d_generated, float const pos[3], float rradius, bool add_grass, int brush_shape,
	unsigned char const *d_updated, unsigned const *d_ranges, unsigned char const *d_weight_data, unsigned capacity, terra_flower *d_flowers, unsigned *d_aux, unsigned *d_counts,
	unsigned char *d_status)
{
	terra_grass_brush const br = {{pos[0], pos[1], pos[2]}, rradius, add_grass ? 1 : 0, brush_shape, 0.0f};
	check(terra_tiles_edit_flowers_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, d_generated, &br, d_updated, d_ranges, d_weight_data, capacity, d_flowers, d_aux, d_counts,
		d_status), "flowers.update_subrange / clear_within");
}
// ---- the grass draw lists of a batch for the camera.  tt_grass_scale_factor goes in once (set_grass_view_globals); grass_length is set_flower_globals'.
inline void set_grass_view_globals(float tt_grass_scale_factor) {
	terra_grass_view_params const p = {tt_grass_scale_factor};
	check(terra_set_grass_view_params(default_ctx(), &p), "set_grass_view_params");
}
// camera_pdu as the library reads it: pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid
inline terra_view view_of(float const pos[3], float const dir[3], float const upv_[3], float const cp[3], float sterm, float x_sterm, float near_, float far_, bool valid) {
	terra_view v;
	for (int k = 0; k < 3; ++k) {v.pos[k] = pos[k]; v.dir[k] = dir[k]; v.upv[k] = upv_[k]; v.cp[k] = cp[k];}
	v.sterm = sterm; v.x_sterm = x_sterm; v.near_ = near_; v.far_ = far_; v.valid = valid ? 1 : 0;
	return v;
}
// tile_t::draw_grass (src/tiled_mesh.cpp:1607-1664) for every tile of the batch as tile_draw_t::draw_grass (:3420-3425) calls it, up to the GL calls: d_insts[t] is
// the tile's instance buffer in draw order, d_group_counts[t][lod][bix] the v.size() of each render_block call, d_pass[t] the wpass the tile is drawn in (255: not at
// all).  d_not_drawn[t] != 0 (or null): the tile is not in to_draw.  The using_shadow_maps() split, the shaders, the texture binds and render_block stay with the engine
inline void tile_draw_grass_lists(tile_batch_dev_t const &b, terra_grass_block const *d_grass_blocks, unsigned char const *d_not_drawn, terra_view const &camera_pdu, unsigned capacity, float *d_insts, unsigned *d_aux, unsigned *d_group_counts, unsigned *d_counts,
	unsigned char *d_pass)
{
	check(terra_tiles_grass_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, b.d_zvals, b.d_stats, d_grass_blocks, d_not_drawn, &camera_pdu, capacity, d_insts, d_aux,
		d_group_counts, d_counts, d_pass), "tile_t::draw_grass");
}
// ---- the terrain draw list of a batch for the camera: the head of tile_draw_t::draw (src/tiled_mesh.cpp:2844-2915) up to its sort, get_lod_level for every present
// tile and the crack indices of tile_t::draw (:2059-2074).  The per-tile state that the library does not hold comes in as arrays (any of them may be null):
// d_min_normal_z (tiles_create_zvals' output), d_trmax (tiles_apply_tree_ao_shadows' output), d_tile_zmax (get_tile_zmax()), d_flags (TERRA_TVIEW_FLAG_*),
// d_last_occluded (in and out: 0 nothing recorded this frame, 1 was_last_occluded(), 2 was_last_unoccluded()).  d_status[t]: TERRA_TVIEW_* with bit 7 on the
// occluders; d_draw_order's first d_counts[0] entries are to_draw after its sort, d_occluded's first d_counts[1] entries occluded_tiles; d_crack[t][2*dim + dir] is
// crack_ibuf.get_index(dim, dir, lod, adj_lod) or 255; d_not_drawn (or null) is what tile_draw_grass_lists takes.  Equal distances order by batch index
struct tile_draw_state_dev_t {
	float const *d_min_normal_z, *d_trmax, *d_tile_zmax; unsigned char const *d_flags; unsigned char *d_last_occluded;
};
inline terra_terrain_view_args terrain_view_args_of(float behind_sphere_mult, float zmin, bool water_enabled, bool check_occlusion, int reflection_pass) {
	terra_terrain_view_args const a = {behind_sphere_mult, zmin, water_enabled ? 1 : 0, check_occlusion ? 1 : 0, reflection_pass};
	return a;
}
inline void tile_draw_lists(tile_batch_dev_t const &b, terra_view const &camera_pdu, terra_terrain_view_args const &args, tile_draw_state_dev_t const &st, unsigned char *d_status,
	float *d_dist, unsigned char *d_lod, unsigned char *d_crack, unsigned *d_draw_order, unsigned *d_occluded, unsigned *d_counts, unsigned char *d_not_drawn = nullptr)
{
	check(terra_tiles_terrain_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, &camera_pdu, &args, b.d_stats, st.d_min_normal_z, st.d_trmax, st.d_tile_zmax, st.d_flags,
		st.d_last_occluded, d_status, d_dist, d_lod, d_crack, d_draw_order, d_occluded, d_counts, d_not_drawn), "tile_draw_t::draw");
}
// tile_draw_t::draw(1): the same lists for the water plane's reflection pass, with can_have_reflection (src/tiled_mesh.cpp:2630-2683, :2869) and get_lod_level(1).
// A tile dropped at :2869 has status TERRA_TVIEW_NO_REFLECTION; d_reflect (or null) says how :2869 was decided.  zmin / zmax: the globals of :2634-2635
inline terra_reflection_view_args reflection_view_args_of(float behind_sphere_mult, float zmin, float zmax, bool water_enabled, bool check_occlusion) {
	terra_reflection_view_args const a = {terrain_view_args_of(behind_sphere_mult, zmin, water_enabled, check_occlusion, 1), zmax};
	return a;
}
inline void tile_draw_lists_reflection(tile_batch_dev_t const &b, terra_view const &camera_pdu, terra_reflection_view_args const &args, tile_draw_state_dev_t const &st,
	unsigned char *d_status, float *d_dist, unsigned char *d_lod, unsigned char *d_crack, unsigned *d_draw_order, unsigned *d_occluded, unsigned *d_counts,
	unsigned char *d_not_drawn = nullptr, unsigned char *d_reflect = nullptr)
{
	check(terra_tiles_reflection_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, &camera_pdu, &args, b.d_stats, st.d_min_normal_z, st.d_trmax, st.d_tile_zmax, st.d_flags,
		st.d_last_occluded, d_status, d_dist, d_lod, d_crack, d_draw_order, d_occluded, d_counts, d_not_drawn, d_reflect), "tile_draw_t::draw(1)");
}
// tile_draw_t::draw_water's per-tile test (tile_t::is_water_visible, :2131-2133) and tile_t::draw_water_cap's edge tests (:2102-2119): d_water_list's first
// d_counts[0] entries are the tiles whose quad is drawn, in batch order; with d_status (a pass-0 tile_draw_lists' on the same batch and camera) d_cap_mask[t] has bit
// 2*dim + dir set where the cap's quad of that edge is emitted, and d_counts[1] counts the tiles with any.  ztop, the vertices and the GL calls stay with the engine
inline void tile_water_lists(tile_batch_dev_t const &b, terra_view const &camera_pdu, float behind_sphere_mult, bool water_enabled, tile_draw_state_dev_t const &st,
	unsigned char const *d_status, unsigned *d_water_list, unsigned char *d_cap_mask, unsigned *d_counts)
{
	terra_water_view_args const a = {behind_sphere_mult, water_enabled ? 1 : 0};
	check(terra_tiles_water_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, &camera_pdu, &a, b.d_stats, st.d_trmax, st.d_tile_zmax, st.d_flags, d_status, d_water_list,
		d_cap_mask, d_counts), "tile_t::draw_water / draw_water_cap");
}
// tile_draw_t::pre_draw's shadow part with tile_t::update_range's deletion and tile_t::setup_shadow_maps (src/tiled_mesh.cpp:1416, :2781-2799, :981-1016): one frame's
// decisions for camera_pdu.  d_smap_state [n] bytes (TERRA_SMAP_NONE or smap_lod_level) is the engine's between frames; d_plan [n] TERRA_SMAP_* words, d_dist_scale [n],
// d_shadow_bcube [n][6], d_receivers' first d_counts[0] entries the tiles to call create_if_needed for; d_terrain_flags (or null) gains TERRA_TVIEW_FLAG_SHADOW_MAPS;
// d_recomp_order (or null, with args.want_recomp) is shadow_recomp_queue in pop_back order, d_counts[1] entries
inline void tile_smap_plan(tile_batch_dev_t const &b, terra_view const &camera_pdu, terra_smap_plan_args const &args, tile_draw_state_dev_t const &st, unsigned char *d_smap_state,
	unsigned *d_plan, float *d_dist_scale, float *d_shadow_bcube, unsigned *d_receivers, unsigned *d_counts, unsigned char *d_terrain_flags = nullptr, unsigned *d_recomp_order = nullptr)
{
	check(terra_tiles_smap_plan_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, &camera_pdu, &args, b.d_stats, st.d_trmax, st.d_tile_zmax, st.d_flags, d_smap_state, d_plan,
		d_dist_scale, d_shadow_bcube, d_receivers, d_counts, d_terrain_flags, d_recomp_order), "tile_t::setup_shadow_maps");
}
// get_pt_cube_frustum_pdu (src/shadow_map.cpp:423-457, the infinite-terrain form) for a receiver's shadow_bcube: the view of one render and its behind_sphere_mult
inline terra_view light_view_of(float const lpos[3], float const shadow_bcube[6], float near_clip, float &behind_sphere_mult) {
	terra_view v;
	check(terra_make_light_view(lpos, shadow_bcube, near_clip, &v, &behind_sphere_mult), "get_pt_cube_frustum_pdu");
	return v;
}
// the head of tile_draw_t::draw_shadow_pass and the filter of draw_tiles_shadow_pass (src/tiled_mesh.cpp:3025-3043, :3004-3018) for R renders: d_recv [R] receivers (on the
// device), views / bsm / lpos [R] on the host.  Row r of d_to_draw / d_terrain [R][n] with d_counts [R][2]; row r of d_not_drawn [R][n] is the skip array of that render's
// shadow-pass tile_draw_pine_trees / scenery / deciduous lists
inline void tile_smap_casters(tile_batch_dev_t const &b, unsigned R, unsigned const *d_recv, terra_view const *views, float const *bsm, float const *lpos, terra_smap_cast_args const &args,
	tile_draw_state_dev_t const &st, unsigned const *d_decid_counts, unsigned *d_to_draw, unsigned *d_terrain, unsigned *d_counts, unsigned char *d_not_drawn, unsigned char *d_status)
{
	check(terra_tiles_smap_casters_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, R, d_recv, views, bsm, lpos, &args, b.d_stats, st.d_trmax, st.d_tile_zmax, st.d_flags,
		d_decid_counts, d_to_draw, d_terrain, d_counts, d_not_drawn, d_status), "tile_draw_t::draw_shadow_pass");
}
// tile_draw_t::draw_tile_clouds (src/tiled_mesh.cpp:3484-3508), first loop: tile_t::update_tile_clouds for every tile in batch order (b.tile_xy, b.n alone are read).
// d_state [n] terra_cloud_tile -- zeroed for a tile that enters the batch -- and d_clouds [n][capacity] terra_cloud travel with their tile between batches.
// clouds_per_tile, cloud_height_offset and rgen_seed: set_cloud_params.  d_total (or null): the `num` of :3489
inline void set_cloud_params(float clouds_per_tile, float cloud_height_offset, int rgen_seed = 1) {
	terra_cloud_params const p = {clouds_per_tile, cloud_height_offset, rgen_seed};
	check(terra_set_cloud_params(default_ctx(), &p), "clouds_per_tile / cloud_height_offset");
}
inline void tile_clouds_update(tile_batch_dev_t const &b, float const wind[3], float fticks, bool animate2, terra_cloud_tile *d_state, terra_cloud *d_clouds, unsigned capacity,
	unsigned *d_total = nullptr)
{
	terra_cloud_step const s = {{wind[0], wind[1], wind[2]}, fticks, animate2 ? 1 : 0};
	check(terra_tiles_update_clouds_dev(default_ctx(), b.tile_xy, b.n, &s, d_state, d_clouds, capacity, d_total), "tile_t::update_tile_clouds");
}
// the rest of draw_tile_clouds: get_draw_list, the sort (back to front; equal keys by (tile, slot)) and tile_cloud_t::draw's decision and alpha per instance.
// xlate: get_tiled_terrain_model_xlate(); max_dist: max(get_draw_tile_dist(), get_inf_terrain_fog_dist()).  The gates clouds_enabled() && atmosphere >= 0.5, the
// points (gen_pts(size)), get_cloud_color(), tfticks, the shader and the GL state stay with the engine
inline void tile_clouds_draw_list(tile_batch_dev_t const &b, terra_view const &camera_pdu, float behind_sphere_mult, float const xlate[3], float max_dist,
	terra_cloud_tile const *d_state, terra_cloud const *d_clouds, unsigned capacity, unsigned char *d_stage, terra_cloud_inst *d_list, unsigned *d_list_count)
{
	terra_cloud_view_args const a = {behind_sphere_mult, {xlate[0], xlate[1], xlate[2]}, max_dist};
	check(terra_tiles_cloud_view_dev(default_ctx(), b.tile_xy, b.n, &camera_pdu, &a, b.d_stats, d_state, d_clouds, capacity, d_stage, d_list, d_list_count), "tile_draw_t::draw_tile_clouds");
}
// tile_t::apply_tree_ao_shadows (src/tiled_mesh.cpp:820-828) for every tile of the batch in batch order, from the records tiles_gen_trees / tiles_gen_decid_trees left
// on the device: small_tree::get_radius / get_ao_radius and tree::get_ao_radius per record, apply_ao_shadows_for_trees' own loop, pulls and pushes, add_tree_ao_shadow's
// texel loop.  xoff2 / yoff2: what the placements ran with (ptree_off / dtree_off).  d_sphere_radius [n][decid_capacity] (tdata().sphere_radius per record) or
// d_sphere_radius_by_id [num_shared_trees]; d_flags[t]: TERRA_TREE_AO_* (or null).  d_trmax feeds get_bcube; d_updated sets sun / moon_shadows_invalid and
// recalc_tree_grass_weights.  Globals: set_tree_size_params once, set_tree_instances after create_pine_tree_instances
struct tile_trees_dev_t {
	terra_tree_place const *d_pine_trees; unsigned const *d_pine_counts; unsigned pine_capacity;
	terra_decid_place const *d_decid_trees; unsigned const *d_decid_counts; unsigned decid_capacity;
	float const *d_sphere_radius, *d_sphere_radius_by_id; unsigned num_shared_trees;
};
inline void tiles_apply_tree_ao_shadows(tile_batch_dev_t const &b, int xoff2, int yoff2, tile_trees_dev_t const &tr, unsigned char const *d_flags, unsigned list_capacity,
	unsigned char *d_tree_map, unsigned char *d_updated = nullptr, float *d_trmax = nullptr, unsigned *d_list_counts = nullptr)
{
	check(terra_tiles_tree_ao_shadows_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, xoff2, yoff2, tr.d_pine_trees, tr.d_pine_counts, tr.pine_capacity, tr.d_decid_trees,
		tr.d_decid_counts, tr.decid_capacity, tr.d_sphere_radius, tr.d_sphere_radius_by_id, tr.num_shared_trees, d_flags, list_capacity, d_tree_map, d_updated, d_trmax,
		d_list_counts), "apply_tree_ao_shadows");
}
// tile_draw_t::add_or_remove_trees_at (src/tiled_mesh.cpp:3746-3769) from :3756 on, for the tiles of the batch, on the records tiles_gen_trees / tiles_gen_decid_trees
// left on the device, in place: the culls, the removal loops, add_new_trees and the near_tiles decision.  xoff2 / yoff2: what the placements ran with.  The caller keeps
// the same-position early-out (:3748-3754), then calls register_tree_change on every tile with d_changed[t] != 0 and tiles_apply_tree_ao_shadows on the batch.
// d_trmax: tiles_apply_tree_ao_shadows' output, in and out
inline void tiles_add_or_remove_trees_at(tile_batch_dev_t const &b, int xoff2, int yoff2, float const pos[3], float radius, bool add_trees, bool is_square,
	unsigned char const *d_no_trees, unsigned char const *d_gen_flags, terra_tree_place *d_pine_trees,
	unsigned *d_pine_counts, unsigned pine_capacity, terra_decid_place *d_decid_trees, unsigned *d_decid_counts, unsigned decid_capacity, float *d_sphere_radius,
	float const *d_sphere_radius_by_id, unsigned num_shared_trees, float *d_trmax, unsigned char *d_status, unsigned char *d_changed, float *d_update_bcube = nullptr)
{
	check(terra_tiles_edit_trees_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, xoff2, yoff2, pos, radius, add_trees, is_square, d_no_trees, b.d_stats, b.d_zvals, d_gen_flags,
		d_pine_trees, d_pine_counts, pine_capacity, d_decid_trees, d_decid_counts, decid_capacity, d_sphere_radius, d_sphere_radius_by_id, num_shared_trees, d_trmax, d_status,
		d_changed, d_update_bcube), "add_or_remove_trees_at");
}
inline void set_tree_size_params(float tree_height_scale, float sm_tree_scale, float pine_tree_radius_scale) {
	terra_tree_size_params const p = {tree_height_scale, sm_tree_scale, pine_tree_radius_scale};
	check(terra_set_tree_size_params(default_ctx(), &p), "set_tree_size_params");
}
// tree_instances after create_pine_tree_instances (src/sm_tree.cpp:342-364): {get_type(), get_height(), get_width()} of every instance, in order
inline void set_tree_instances(terra_tree_inst const *insts, unsigned count) {check(terra_set_tree_instances(default_ctx(), insts, count), "create_pine_tree_instances");}
// ---- the pine and palm tree draw lists of a batch for the camera: tile_t::draw_pine_trees (src/tiled_mesh.cpp:1465-1526) for every tile, without its GL and shader
// calls, from the records tiles_gen_trees left on the device.  One call answers the three draw_pine_tree_bl sweeps of a frame (args.draw_trunks / draw_near_leaves /
// draw_far_leaves).  d_not_drawn: tile_draw_lists' output (or null); d_trmax: tiles_apply_tree_ao_shadows' output (or null); d_trunk_override: the cylinders of the
// rotated palms that are not instanced (or null).  d_tile_out[t].flags: TERRA_TRV_*; the instance lists are tree_inst_t records in ascending (id, record index);
// d_leaf_list holds record indices, the pine entries first; d_trunk one byte per record (0, 1 = a skipped line, else nsides)
inline terra_tree_view_args tree_view_args_of(float behind_sphere_mult, bool shadow_pass, int window_width, float zoom_f, float tree_depth_scale, bool draw_trunks,
	bool draw_near_leaves, bool draw_far_leaves)
{
	terra_tree_view_args const a = {behind_sphere_mult, zoom_f, tree_depth_scale, window_width, shadow_pass ? 1 : 0, draw_trunks ? 1 : 0, draw_near_leaves ? 1 : 0, draw_far_leaves ? 1 : 0};
	return a;
}
inline void tile_draw_pine_tree_lists(tile_batch_dev_t const &b, int xoff2, int yoff2, terra_view const &camera_pdu, terra_tree_view_args const &args, unsigned char const *d_not_drawn,
	float const *d_trmax, terra_tree_place const *d_pine_trees, unsigned const *d_pine_counts, unsigned capacity, terra_trunk_override const *d_trunk_override,
	terra_tree_view_tile *d_tile_out, float *d_all_bcube, terra_tree_view_inst *d_pine_insts, terra_tree_view_inst *d_palm_insts, unsigned *d_inst_counts, unsigned *d_leaf_list,
	unsigned *d_leaf_counts, unsigned char *d_trunk)
{
	check(terra_tiles_tree_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, xoff2, yoff2, &camera_pdu, &args, b.d_stats, d_not_drawn, d_trmax, d_pine_trees, d_pine_counts,
		capacity, d_trunk_override, d_tile_out, d_all_bcube, d_pine_insts, d_palm_insts, d_inst_counts, d_leaf_list, d_leaf_counts, d_trunk), "tile_t::draw_pine_trees");
}
// ---- the scenery draw lists of a batch for the camera: tile_t::draw_scenery (src/tiled_mesh.cpp:1580-1592) for every tile, without its GL, shader and colour calls,
// from the records tiles_gen_scenery left on the device.  One call answers both sweeps of tile_draw_t::draw_scenery (args.draw_opaque / draw_leaves).  d_not_drawn:
// tile_draw_lists' output (or null); d_radius_override: voxel_rock::build_model's and gen_rock's radii (or null).  d_draw holds one TERRA_SCV_* word per record,
// d_list record indices in TERRA_SCV_GROUPS groups per tile in the order draw_opaque_objects and draw_plant_leaves issue them
inline terra_scenery_view_args scenery_view_args_of(float behind_sphere_mult, bool shadow_only, bool reflection_pass, int window_width, float zoom_f, float smap_pixel_width,
	bool uw_skip, bool can_skip_small_shadow_objs, bool draw_opaque, bool draw_leaves)
{
	terra_scenery_view_args const a = {behind_sphere_mult, zoom_f, smap_pixel_width, window_width, shadow_only ? 1 : 0, reflection_pass ? 1 : 0, uw_skip ? 1 : 0,
		can_skip_small_shadow_objs ? 1 : 0, draw_opaque ? 1 : 0, draw_leaves ? 1 : 0};
	return a;
}
inline void tile_draw_scenery_lists(tile_batch_dev_t const &b, int xoff2, int yoff2, terra_view const &camera_pdu, terra_scenery_view_args const &args, unsigned char const *d_not_drawn,
	terra_scenery_place const *d_scenery, unsigned const *d_counts, unsigned capacity, float const *d_radius_override, terra_scenery_view_tile *d_tile_out, unsigned *d_draw,
	float *d_size_scale, float *d_dist, unsigned *d_list, unsigned list_capacity, unsigned *d_group_counts)
{
	check(terra_tiles_scenery_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, xoff2, yoff2, &camera_pdu, &args, b.d_stats, d_not_drawn, d_scenery, d_counts, capacity,
		d_radius_override, d_tile_out, d_draw, d_size_scale, d_dist, d_list, list_capacity, d_group_counts), "tile_t::draw_scenery");
}
// ---- the deciduous tree draw lists of a batch for the camera: tile_t::draw_decid_trees (src/tiled_mesh.cpp:1555-1563) for every tile, without its GL, shader and
// colour calls, from the records tiles_gen_decid_trees left on the device.  One call answers both sweeps of tile_draw_t::draw_decid_trees (args.draw_leaves /
// draw_branches), the leaves first.  d_not_drawn: tile_draw_lists' output (or null); d_tree_data: what the decisions read of the shared tree_data_t's, on the device;
// d_not_visible: tree::not_visible per record (or null).  out.leaf_word / branch_word hold one TERRA_DCV_* word per record, leaf_list / branch_list record indices in
// the reference's order, leaf_bb / branch_bb the entries of add_leaves / add_branches in runs of one tree_id
struct decid_view_out_t {
	terra_decid_view_tile *d_tile_out; float *d_all_bcube;
	unsigned *d_leaf_word; float *d_leaf_scale, *d_leaf_opacity; unsigned *d_leaf_num, *d_branch_word; float *d_branch_scale, *d_branch_opacity; unsigned *d_branch_num;
	unsigned *d_leaf_list, *d_branch_list; terra_decid_view_bb *d_leaf_bb, *d_branch_bb; unsigned *d_list_counts;
};
inline terra_decid_view_args decid_view_args_of(float behind_sphere_mult, float zoom_f, float const tree_lod_scales[4], bool shadow_pass, bool reflection_pass, bool use_tree_billboards,
	bool leaf_color_changed, bool draw_leaves, bool draw_branches)
{
	terra_decid_view_args const a = {behind_sphere_mult, zoom_f, {tree_lod_scales[0], tree_lod_scales[1], tree_lod_scales[2], tree_lod_scales[3]}, shadow_pass ? 1 : 0,
		reflection_pass ? 1 : 0, use_tree_billboards ? 1 : 0, leaf_color_changed ? 1 : 0, draw_leaves ? 1 : 0, draw_branches ? 1 : 0};
	return a;
}
inline void tile_draw_decid_tree_lists(tile_batch_dev_t const &b, int xoff2, int yoff2, terra_view const &camera_pdu, terra_decid_view_args const &args,
	terra_decid_tree_data const *d_tree_data, unsigned num_tree_data, unsigned char const *d_not_drawn, terra_decid_place const *d_decid_trees, unsigned const *d_counts,
	unsigned capacity, unsigned char *d_not_visible, decid_view_out_t const &out)
{
	check(terra_tiles_decid_view_dev(default_ctx(), b.tile_xy, b.n, b.dxoff, b.dyoff, xoff2, yoff2, &camera_pdu, &args, d_tree_data, num_tree_data, d_not_drawn, d_decid_trees,
		d_counts, capacity, d_not_visible, out.d_tile_out, out.d_all_bcube, out.d_leaf_word, out.d_leaf_scale, out.d_leaf_opacity, out.d_leaf_num, out.d_branch_word,
		out.d_branch_scale, out.d_branch_opacity, out.d_branch_num, out.d_leaf_list, out.d_branch_list, out.d_leaf_bb, out.d_branch_bb, out.d_list_counts),
		"tile_t::draw_decid_trees");
}
// tile_t::update_terrain_params (src/tiled_mesh.cpp:321-343): params [n][2][2]{veg, grass, dirt}
inline void tiles_terrain_params(int const *tile_xy, unsigned n, float *params) {check(terra_tiles_terrain_params(default_ctx(), tile_xy, n, params), "update_terrain_params");}
// voxel_manager::create_procedural fill (src/voxels.cpp:278-346): `vals` is the voxel_grid<float> storage, z fastest
inline void voxel_create_procedural(std::vector<float> &vals, unsigned nx, unsigned ny, unsigned nz, float const lo_pos[3], float const vsz[3], float const offset[3],
	float mag, float freq, bool normalize_to_1, int rseed1, int rseed2, int gen_mode, float zscale)
{
	vals.resize((size_t)nx*ny*nz);
	check(terra_voxel_fill(default_ctx(), vals.data(), nx, ny, nz, lo_pos, vsz, offset, mag, freq, rseed1, rseed2, gen_mode, zscale, normalize_to_1 ? 1 : 0), "voxel_create_procedural");
}

} // namespace terra_cxx
