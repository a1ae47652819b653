// tests/emul/stage_san_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program over the emulator (terra_emul.cpp, the same driver and host entry points as libterra_hip.so with a host-loop backend): every host-pointer
// entry point that stages through the host-grid scratch (terra_stage.hpp) is called once, with a mixed pick of optional arrays, at S = 16, n = 3, capacity 1 --
// and the two passes that still need S = 128 at n = 2.  tests/test_host_staging_emul.py builds it with -fsanitize=address,undefined and runs it as a child
// process: the emulator's device memory is malloc'd and every host array here is a vector of its exact size, so a staged array that runs past the scratch, or a
// download that runs past the caller's array, ends the program.  Exit status 0: every call returned TERRA_OK.
#include "terra_emul.cpp"
#include <vector>
#include <cstdio>

#define CK(call) do {if ((call) != TERRA_OK) {fprintf(stderr, "%s:%d: %s\n  -> %s\n", __FILE__, __LINE__, #call, terra_last_error()); return 1;}} while (0)

static terra_config scene(int S) { // the synthetic scene the tests use
	terra_config c; memset(&c, 0, sizeof(c));
	c.mesh_x = c.mesh_y = S; c.scene_x = c.scene_y = c.scene_z = 4.0f; c.mesh_height = 0.7f; c.mesh_scale = 1.0f;
	c.mesh_seed = 1; c.mesh_freq_filter = 0; c.mesh_gen_mode = TERRA_MGEN_SINE; c.mesh_gen_shape = 0; c.glaciate = 1;
	c.hmap[0] = 1000.0f; c.hmap[4] = 1000.0f; c.hmap[9] = 5.0f; c.hmap[10] = 0.001f; c.hmap[11] = -4.0f;
	c.erode_amount = 1.0f; c.start_mag = 0.02f; c.start_freq = 240.0f; c.mag_mult = 2.0f; c.freq_mult = 0.5f;
	return c;
}

static int run16(terra_ctx *ctx) {
	uint32_t const S = 16, n = 3, W = S + 1, Z = S + 2, cap = 1, nshared = 7;
	float const dx = 8.0f/S;
	std::vector<int32_t> txy = {0, 0, -1, 2, -2, -1};
	terra_config const cfg = scene((int)S);
	CK(terra_init_scene(ctx, &cfg));
	terra_tree_params tp; CK(terra_get_tree_params(ctx, &tp));
	tp.tree_mode = 2; tp.sm_tree_density = 0.1f; CK(terra_set_tree_params(ctx, &tp));
	terra_decid_params dp; CK(terra_get_decid_params(ctx, &dp));
	dp.num_trees = 60; dp.num_shared_trees = nshared; CK(terra_set_decid_params(ctx, &dp));

	// grids: a generated grid, an eroded one, the 16-bit heightmap
	std::vector<float> grid(40*24);
	CK(terra_gen_grid(ctx, -20.0f, -12.0f, 1.0f, 1.0f, 40, 24, TERRA_GEN_GLACIATE, 0, grid.data()));
	CK(terra_apply_erosion(ctx, grid.data(), 40, 24, -10.0f, 20));
	std::vector<uint8_t> pix(48*32*2); float range[2];
	CK(terra_heightmap_proc_gen(ctx, 48, 32, 10, pix.data(), range));

	std::vector<float> z((size_t)n*Z*Z);
	std::vector<terra_tile_stats> stats(n);
	CK(terra_tiles_create_zvals(ctx, txy.data(), n, 0, z.data(), stats.data(), nullptr, nullptr));
	std::vector<uint8_t> skip = {0, 0, 1}, distant = {0, 0, 1};

	// line queries: distant present, line_tile absent
	std::vector<float> lines;
	for (uint32_t i = 0; i < n; ++i) {
		for (uint32_t k = 0; k < 3; ++k) {
			float const x = -4.0f + dx*((float)txy[2*i]*S + 2 + 5*k), y = -4.0f + dx*((float)txy[2*i+1]*S + 3 + 4*k), zz = z[(size_t)i*Z*Z + (3 + 4*k)*Z + 2 + 5*k];
			float const l[6] = {x, y, zz + 5.0f, x, y, zz - 5.0f};
			lines.insert(lines.end(), l, l + 6);
		}
	}
	uint32_t const nlines = (uint32_t)lines.size()/6;
	std::vector<terra_line_hit> hits(nlines);
	CK(terra_tiles_line_intersect(ctx, txy.data(), n, 0, 0, z.data(), stats.data(), distant.data(), lines.data(), nullptr, nlines, hits.data()));

	// tree map: a slice of the splat array (h_first[0] = 2), distant present, updated absent; then continued (reset = 0: the map is uploaded) with updated
	std::vector<terra_tree_splat> splats(2 + 4*n);
	for (uint32_t i = 0; i < n; ++i) {
		for (uint32_t k = 0; k < 4; ++k) {splats[2 + 4*i + k] = terra_tree_splat{-4.0f + dx*((float)txy[2*i]*S + 3.5f*k + 1), -4.0f + dx*((float)txy[2*i+1]*S + 2.5f*k + 4), dx*(1.3f + k)};}
	}
	std::vector<uint32_t> first(n + 1);
	for (uint32_t i = 0; i <= n; ++i) {first[i] = 2 + 4*i;}
	std::vector<uint8_t> tree_map((size_t)n*W*W*2), updated(n);
	CK(terra_tiles_tree_map(ctx, txy.data(), n, 0, 0, distant.data(), splats.data(), first.data(), 1, tree_map.data(), nullptr));
	CK(terra_tiles_tree_map(ctx, txy.data(), n, 0, 0, nullptr, splats.data(), first.data(), 0, tree_map.data(), updated.data()));

	// shadow texture: sun and ao present, moon and the tree map absent (light_factor 1: the sun alone is up)
	std::vector<uint8_t> sun((size_t)n*Z*Z, 0x5A), ao((size_t)n*W*W, 0x77), shadow((size_t)n*W*W*4);
	CK(terra_tiles_shadow_texture(ctx, n, sun.data(), nullptr, ao.data(), nullptr, 1.0f, 1, shadow.data()));

	// the placements at capacity 1: skip present, stats absent (deciduous: zvals present), kind counts absent; and their brush forms with stats
	std::vector<terra_tree_place> pine((size_t)n*cap); std::vector<uint32_t> pine_counts(n);
	CK(terra_tiles_place_trees(ctx, txy.data(), n, 0, 0, skip.data(), nullptr, cap, pine.data(), pine_counts.data()));
	tp.tree_mode = 3; CK(terra_set_tree_params(ctx, &tp));
	std::vector<terra_decid_place> decid((size_t)n*cap); std::vector<uint32_t> decid_counts(n);
	CK(terra_tiles_place_decid_trees(ctx, txy.data(), n, 0, 0, skip.data(), nullptr, z.data(), cap, decid.data(), decid_counts.data()));
	std::vector<terra_scenery_place> objs((size_t)n*cap); std::vector<uint32_t> obj_counts(n), kinds((size_t)n*TERRA_SCENERY_KINDS);
	CK(terra_tiles_place_scenery(ctx, txy.data(), n, 0, 0, skip.data(), cap, objs.data(), obj_counts.data(), nullptr));
	CK(terra_tiles_place_scenery(ctx, txy.data(), n, 0, 0, nullptr, cap, objs.data(), obj_counts.data(), kinds.data()));
	float const pos[3] = {-4.0f + dx*0.9f*S, -4.0f + dx*0.5f*S, z[(S/2)*Z + S/2]}, radius = 1.5f*S*dx;
	{
		std::vector<terra_tree_place> bp((size_t)n*cap); std::vector<terra_decid_place> bd((size_t)n*cap); std::vector<uint32_t> bc(n);
		CK(terra_tiles_place_trees_brush(ctx, txy.data(), n, 0, 0, nullptr, stats.data(), pos, radius, 0, cap, bp.data(), bc.data()));
		CK(terra_tiles_place_decid_trees_brush(ctx, txy.data(), n, 0, 0, nullptr, stats.data(), z.data(), pos, radius, 1, cap, bd.data(), bc.data()));
	}
	if (pine_counts[0] == 0 || pine_counts[1] == 0 || decid_counts[0] <= cap) {fprintf(stderr, "the placements place too little: the calls below would be trivial\n"); return 1;}

	// tree AO: both groups, per-record radii absent, by-id radii present, flags present, updated absent, trmax present, list counts absent
	std::vector<float> by_id(nshared), trmax(n);
	for (uint32_t k = 0; k < nshared; ++k) {by_id[k] = dx*(0.4f + 0.3f*k);}
	std::vector<uint8_t> flags(n, 0);
	CK(terra_tiles_tree_ao_shadows(ctx, txy.data(), n, 0, 0, 0, 0, pine.data(), pine_counts.data(), cap, decid.data(), decid_counts.data(), cap, nullptr, by_id.data(), nshared,
		flags.data(), 64, tree_map.data(), nullptr, trmax.data(), nullptr));

	// tree brush, adding: skip present, gen_flags absent, per-record radii absent, by-id radii present, the box present; then removing, with per-record radii and no box
	std::vector<uint8_t> status(n), changed(n); float box[6];
	CK(terra_tiles_edit_trees(ctx, txy.data(), n, 0, 0, 0, 0, pos, radius, 1, 0, skip.data(), stats.data(), z.data(), nullptr, pine.data(), pine_counts.data(), cap,
		decid.data(), decid_counts.data(), cap, nullptr, by_id.data(), nshared, trmax.data(), status.data(), changed.data(), box));
	std::vector<float> rad((size_t)n*cap, dx);
	CK(terra_tiles_edit_trees(ctx, txy.data(), n, 0, 0, 0, 0, pos, radius, 0, 1, nullptr, stats.data(), nullptr, flags.data(), pine.data(), pine_counts.data(), cap,
		decid.data(), decid_counts.data(), cap, rad.data(), nullptr, 0, trmax.data(), status.data(), changed.data(), nullptr));
	return 0;
}

static int run128(terra_ctx *ctx) { // the grass brush and the tree weights
	uint32_t const n = 2;
	std::vector<int32_t> txy = {0, 0, 1, 0};
	terra_config const cfg = scene(128);
	CK(terra_init_scene(ctx, &cfg));
	std::vector<float> z((size_t)n*130*130);
	std::vector<terra_tile_stats> stats(n);
	CK(terra_tiles_create_zvals(ctx, txy.data(), n, 0, z.data(), stats.data(), nullptr, nullptr));
	std::vector<uint8_t> w((size_t)n*129*129*4), updated(n), distant = {0, 0};
	std::vector<terra_grass_block> gb((size_t)n*32*32);
	CK(terra_tiles_create_weights(ctx, txy.data(), n, z.data(), w.data(), gb.data(), nullptr));
	terra_grass_brush brush = {{-4.0f + 0.0625f*128, -4.0f + 0.0625f*60, z[(size_t)130*130 + 60*130]}, 7.5f*0.0625f, 1, 1, 0.08f};
	CK(terra_tiles_edit_grass(ctx, txy.data(), n, 0, 0, z.data(), stats.data(), distant.data(), &brush, w.data(), gb.data(), updated.data(), nullptr)); // distant present, ranges absent
	std::vector<uint8_t> tree_map((size_t)n*129*129*2, 0x40), out((size_t)n*129*129*4);
	CK(terra_tiles_tree_weights(ctx, n, w.data(), nullptr, out.data()));
	CK(terra_tiles_tree_weights(ctx, n, w.data(), tree_map.data(), out.data()));
	return 0;
}

int main() {
	terra_ctx *ctx = nullptr;
	CK(terra_create(&ctx, 0));
	int rc = run16(ctx);
	if (rc == 0) {rc = run128(ctx);}
	terra_destroy(ctx);
	if (rc == 0) {printf("stage_san: every host entry point returned TERRA_OK\n");}
	return rc;
}
