/* terra.h -- C ABI of libterra_hip.so: MI355X (gfx950) procedural-terrain hot path of 3DWorld.
 *
 * Drop-in boundary.  3DWorld has no plugin/FFI layer; the seam is the three C++ call surfaces
 * below plus the voxel fill.  Every entry point names the reference interface it replaces (paths relative to the
 * 3DWorld tree).  All pointers are plain host or device pointers, all sizes plain integers; nothing here depends on
 * torch, OpenGL or the engine's headers.  The engine keeps its process globals; they cross the boundary explicitly
 * as terra_config (what the config file sets) or terra_state (already-derived globals).
 *
 *   reference interface                                                     replaced by
 *   ----------------------------------------------------------------------  -------------------------------------------
 *   create_sin_table / gen_rand_sine_table_entries / compute_scale /        terra_init_scene
 *     estimate_zminmax / set_zvals / init_terrain_mesh / gen_tex_height_tables
 *     (src/mesh_gen.cpp:72-81,213-254,407-431,447-512,544-548; src/Textures.cpp:1757-1761)
 *   mesh_xy_grid_cache_t::build_arrays / enable_glaciate / eval_index       terra_gen_* handle, terra_gen_grid[_dev]
 *     (src/mesh.h:22-45, src/mesh_gen.cpp:588-650,754-792)
 *   apply_erosion(float*,int,int,float,unsigned)                            terra_apply_erosion[_dev]
 *     (src/function_registry.h:354, src/erosion.cpp:14-164)
 *   tile_t::create_zvals + get_norm/upload_normal_texture CPU part          terra_tiles_create_zvals[_dev]
 *     (src/tiled_mesh.h:277,281-284; src/tiled_mesh.cpp:467-546,865-880)
 *   heightmap_t::proc_gen / run_erosion / from_floats                       terra_heightmap_proc_gen[_dev], terra_quantize16_dev
 *     (src/heightmap.cpp:130-215, src/Textures.cpp:1889-1893)
 *   heightmap_t::to_floats / postprocess_height (loaded heightmaps)         terra_heightmap_to_floats_dev, terra_heightmap_from_floats_dev,
 *     (src/heightmap.cpp:117-128,191-203,351)                                 terra_heightmap_postprocess_dev, terra_set_mesh_file_scale
 *   voxel_manager::create_procedural                                        terra_voxel_fill[_dev]
 *     (src/voxels.cpp:278-346, src/upsurface.cpp:16-70)
 *
 * Error behaviour: the reference asserts; this library returns TERRA_OK (0) or a negative terra_status and keeps a
 * thread-local message (terra_last_error).  There is NO CPU fall-back: without a usable HIP device terra_create fails.
 *
 * Threading: one terra_ctx per host thread / GPU (one process per GPU in multi-GPU runs).  All *_dev work is enqueued
 * on the context's HIP stream (its own, or the caller's via terra_set_stream) and is asynchronous unless noted.
 * The terra_gen_* handles are the one exception (the reference calls eval_index from its OpenMP workers): handles of one context may be
 * used from several threads at once, terra_gen_eval_index on a collected grid takes no lock at all; what may NOT overlap is (a) any other
 * terra_* call on the same context with a terra_gen_* call that launches work (build_arrays, enable_glaciate, collect, an eval_index that
 * needs another first sine term), and (b) terra_gen_build_arrays with terra_gen_eval_index on the SAME handle (build_arrays is main-thread
 * only in the reference too, src/mesh.h:40).
 */
#ifndef TERRA_H
#define TERRA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TERRA_F_TABLE_SIZE 90 /* F_TABLE_SIZE, src/mesh_gen.cpp:30 */

typedef enum {TERRA_OK = 0, TERRA_ERR_ARG = -1, TERRA_ERR_HIP = -2, TERRA_ERR_STATE = -3, TERRA_ERR_NODEVICE = -4, TERRA_ERR_LIMIT = -5} terra_status;

/* mesh_gen_mode values (src/3DWorld.h:1399) */
enum {TERRA_MGEN_SINE = 0, TERRA_MGEN_SIMPLEX = 1, TERRA_MGEN_PERLIN = 2, TERRA_MGEN_SIMPLEX_GPU = 3, TERRA_MGEN_DWARP_GPU = 4};

/* What the engine's config file sets for this path (keyword -> global binding in src/3DWorld.cpp:1763-2110). */
typedef struct terra_config {
	int32_t mesh_x, mesh_y;                  /* mesh_size            -> MESH_X_SIZE, MESH_Y_SIZE */
	float scene_x, scene_y, scene_z;         /* scene_size           -> X/Y/Z_SCENE_SIZE */
	float mesh_height, mesh_scale;           /* mesh_height (-> mesh_height_scale), mesh_scale */
	int32_t mesh_seed, mesh_freq_filter, mesh_gen_mode, mesh_gen_shape, glaciate; /* mesh_seed, mesh_freq_filter, mesh_gen_mode, mesh_gen_shape, GLACIATE */
	float custom_glaciate_exp;               /* custom_glaciate_exp (0 = cubic) */
	float hmap[14];                          /* hmap_params_t in declaration order, src/mesh.h:84-88 */
	float erode_amount, water_h_off, water_h_off_rel, relh_adj_tex, ocean_wave_height;
	float start_mag, start_freq, mag_mult, freq_mult; /* mesh_start_mag/freq, mesh_mag/freq_mult */
} terra_config;

/* The derived globals of the reference; terra_get_state exports them, terra_set_state injects an engine's own values. */
typedef struct terra_state {
	float sinTable[TERRA_F_TABLE_SIZE][5];   /* {mag, y-phase, x-phase, y-freq, x-freq}, src/mesh_gen.cpp:247-251 */
	int32_t start_eval_sin;
	float MESH_HEIGHT, DX_VAL, DY_VAL, DX_VAL_INV, DY_VAL_INV, HALF_DXY, dxdy, XY_SCENE_SIZE;
	float mesh_scale, mesh_scale_z_inv, mesh_height_scale;
	float zmax_est, zmin, zmax, water_plane_z, glaciate_exp, clip_hd1, relh_adj_tex;
	float rx, ry;                            /* gen_rx_ry(), src/mesh_gen.cpp:581-586 */
} terra_state;

/* tile_t outputs of create_zvals (src/tiled_mesh.cpp:517-541): 4x4 sub-block z range, tile z range, radius, water bbox (ints, bit-exact) */
typedef struct terra_tile_stats {
	float sub_zmin[16], sub_zmax[16], mzmin, mzmax, radius;
	int32_t wx1, wy1, wx2, wy2;
} terra_tile_stats;

/* counters of the last terra_apply_erosion*_dev call (diagnostics / bench) */
typedef struct terra_erosion_report {
	uint32_t droplets, windows /* ring generations = ceil(droplets / slots) */, rounds, traces, serial_fallbacks, nan_droplets;
	uint64_t steps;          /* droplet steps of the final (committed) traces */
	uint64_t traced_steps;   /* droplet steps actually simulated, re-traces included */
	uint64_t retraces_same;  /* re-traces that reproduced the published version bit for bit (the conflict that caused them was one of blocks, not of cells read) */
	uint64_t checkpoint_resumes;     /* re-traces that started from a checkpoint of the droplet's previous trace instead of from its spawn */
	uint64_t checkpoint_steps_saved; /* steps those re-traces did not have to repeat */
	/* where the time goes (speculative scheduler only).  Everything from here down to the end is collected only with TERRA_ERO_DIAG=1 in the environment
	 * (0 otherwise): the counters live in one cache line that every trace of the chip would have to update */
	uint64_t window_shifts;  /* times the 32 x 32 LDS window was moved */
	uint64_t critical_steps; /* sum over the rounds of the most steps any one trace made in the round: the scheduler's serial chain, in droplet steps */
	uint64_t critical_shifts;/* the same for window moves */
	/* device time in 10 ns ticks, summed over all traces: a trace's whole wave body / before its first step / inside window moves / after its last step;
	 * clk_critical: the longest wave body of each round, summed over the rounds */
	uint64_t clk_wave, clk_init, clk_shift, clk_tail, clk_critical;
	uint64_t clk_shift_flush, clk_shift_prep, clk_shift_load; /* parts of clk_shift: write-back of the cells that leave / block flags (candidate versions per block); clk_shift_load is 0 since the grid loads are in flight during the look-ups and are not timed apart: the rest of clk_shift is loads + look-ups + filling the window */
	uint64_t crit_clk_flush, crit_clk_load, crit_clk_prep; /* the parts of crit_clk_shift */
	uint64_t crit_clk_shift, crit_clk_edge, crit_steps_own; /* of each round's longest wave body: ticks in window moves, ticks before + after its steps, its steps (multiple of 4) */
	/* the sparse scheduler (few droplets on a big map: lean traces on the grid itself, one round per conflicting droplet): droplets it committed (0: not tried; `droplets`: the
	 * whole run -- anything less: the multi-version scheduler did the rest) and the re-traces that took */
	uint64_t sparse_droplets, sparse_retraces;
	uint64_t sparse_probe_only; /* droplets of such a run that ended at their first step without writing (ocean): settled by one thread each, no trace wave */
} terra_erosion_report;

/* The globals tile_t::create_texture and tile_t::update_terrain_params read beyond terra_config; the defaults are the reference's. */
typedef struct terra_landscape {
	float vegetation;            /* config "vegetation" (src/3DWorld.cpp:109): 0 turns ground/grass into rock and disables the sand conversions */
	float temperature;           /* DEF_TEMPERATURE = 20 (src/3DWorld.h:87): above 40 the snow line rises (src/mesh_gen.cpp:423-426) */
	float biome_x_offset;        /* config "biome_x_offset" */
	float mesh_scale_z;          /* src/mesh_gen.cpp:37,873: 1 until the terrain zoom changes it */
	int32_t water_is_lava;       /* config "water_is_lava": snow -> rock */
	int32_t disable_water;       /* DISABLE_WATER: 2 also turns snow into rock (src/Textures.cpp:1290) */
	int32_t enable_terrain_env;  /* ENABLE_TERRAIN_ENV = 1 (src/tiled_mesh.h:21): biome parameters from eval_mesh_sin_terms at the tile corners; 0 = {veg 1, grass 1, dirt 0} */
	uint32_t grass_density;      /* config "grass_density": 0 = gen_grass_map() false, no grass blocks (src/tiled_mesh.cpp:126) */
	uint32_t num_rnd_grass_blocks; /* 16 (src/grass.cpp:14) */
} terra_landscape;
/* tile_t::grass_block_t (src/tiled_mesh.h:186): ix 0 = no grass in this 4x4-texel block, else 1 + index of the random grass block; z range of its texels */
typedef struct terra_grass_block {uint32_t ix; float zmin, zmax;} terra_grass_block;

typedef struct terra_ctx terra_ctx;
typedef struct terra_gen terra_gen;

/* flags of terra_gen_grid* / terra_gen_build_arrays (bool arguments of build_arrays, src/mesh.h:40) */
#define TERRA_GEN_GLACIATE     1u  /* enable_glaciate() after build_arrays() */
#define TERRA_GEN_FORCE_SINE   2u  /* force_sine_mode */
#define TERRA_GEN_NO_WAIT      4u  /* no_wait: return 0 right after launch */
#define TERRA_GEN_CACHE_VALUES 8u  /* cache_values: every cell is always evaluated on the device; the flag only decides what eval_index(.., use_cache=1) returns */
/* TOLERANCE mode (opt-in; everything else in this library is bit-identical to the reference's CPU path).  The reference binary has no fused multiply-add, so the exact
 * kernels pay a multiply AND an add per term of eval_index's sum (src/mesh_gen.cpp:777-779) and can never pass half of the chip's fp32 rate.  With this flag every a*b + c of
 * the sum and of eval_index's tail (glaciate's last step, the island term; src/mesh_gen.cpp:380-385,781-790) rounds ONCE: the value is the reference's expression tree
 * evaluated with fmaf, exactly (pinned against that restatement in the tests' checker: orc_set_fused), and within 1e-5 * zmax_est of the reference (BASELINE's bar; measured
 * max 3e-7 * zmax_est on the 16384^2 grid).  The sine tables are the exact mode's (SINF indices pinned).  The sum runs on the f32 matrix pipe (csrc/terra_fused.hpp).  It is a
 * permission, not a command: a configuration without a fused kernel (fBm modes, shapes / plateau / crater / volcano set-ups whose cells can leave the short tail) is
 * evaluated by the exact kernel.  Do not feed fused heights to apply_erosion when the droplet paths must be the reference's: erosion amplifies a last-bit difference.
 * The calls without a flags argument (tiles, voxels) take it from terra_set_option(ctx, "gen.fused", "1"). */
#define TERRA_GEN_FUSED        16u
/* The cheapest form within the same tolerance (implies TERRA_GEN_FUSED where it has no kernel of its own): the sine sum's tables are split into scaled half-precision pairs and
 * the contraction runs on the half-precision matrix pipe, 16 times the f32 pipe's rate (csrc/terra_fused.hpp: k_sine_grid_h3) -- the kernel is then bound by writing its result.
 * Within 1e-5 * zmax_est of the reference like TERRA_GEN_FUSED (measured ~1e-6), but not the value of any restatement: tested against the tolerance only.  Option "gen.fused" = "2". */
#define TERRA_GEN_FAST         32u
/* flags of terra_apply_erosion*_dev */
#define TERRA_ERODE_SERIAL        1u /* walk droplets one by one on one lane (reference order, no speculation): debugging / tiny grids */
#define TERRA_ERODE_SERIAL_WAVE   4u /* droplets one after another, each simulated by a whole wave through the LDS window (no speculation) */
#define TERRA_ERODE_MINZ_IS_MIN   2u /* caller guarantees min_zval <= every grid value (heightmap_t::run_erosion passes min(vals)): clamp only written cells */

const char *terra_last_error(void);
int  terra_device_count(void);

/* ---- context */
int  terra_create(terra_ctx **out, int device_index);
void terra_destroy(terra_ctx *ctx);
int  terra_set_stream(terra_ctx *ctx, void *hip_stream);   /* use the caller's hipStream_t (e.g. torch's current stream); NULL = own stream */
int  terra_synchronize(terra_ctx *ctx);
/* ---- options: every behaviour switch of the library (nothing in it reads the process environment).  Values are strings; an unknown key or a value outside the key's
 * range is TERRA_ERR_ARG and changes nothing.  The call drains the context's stream first.  Only "gen.fused" changes a result.
 *   "gen.fused"            "0" | "1" | "2"   every generator call of this context behaves as if TERRA_GEN_FUSED ("1") / TERRA_GEN_FAST ("2") were given (tile batches and voxel fields have no flags argument)
 *   "kernels.simple"       "0" | "1"      one-thread-per-cell cross-check kernels instead of the tiled ones (tests)
 *   "graphs"               "0" | "1"      replay the erosion rounds as hipGraphs (default 1)
 *   "sg.kc" "20"|"27"|"45", "sg.kc_tiles" "27"|"45", "sg.rowgroup" "1".."1024"      LDS chunking / tile walk of the exact sine kernel
 *   "sg.turn_rows"         n | "default"  rows of a heightmap still to be evaluated when terra_gen_grid_minmax_turn_dev hands the noise turn on, rounded up to whole 128-row tile rows; "0": no split.
 *                                          "default": 2048 on grids of at least 8 x as many rows, 0 on smaller ones; a value that was set applies to every grid (results never depend on it)
 *   "tile_erosion"         "lds" | "window"   the whole padded tile in LDS (default) or a 32 x 32 window over a copy in HBM
 *   "weights.simple"       "0" | "1"      per-texel form of the weights-texture pass;   "shadows.levels" "0" | "1"   one launch per dependency level of the mesh shadows
 *   "ao.bands"             "1" | "0"      the AO context of a tile batch evaluated as four bands around each tile (its centre is the tile's own heights) / as whole squares
 *   "ao.whole"             "1" | "0"      the AO rays of a tile from one workgroup that holds the tile's whole 201 x 201 context in LDS / from four 33-row band workgroups
 *   "voxels.cols"          "1" | "0"      the lane-per-column form of the voxel sine field (no array of x*y products) wherever the depth is a multiple of 4 / the z-lane form everywhere
 *   "ero.sparse"           "0" | "1" | "auto"   never / always / by droplet density try the sparse erosion scheduler;   "ero.sparse_retraces" n
 *   "ero.lead" "0".."2", "ero.batch" n, "ero.fuse" 0..7, "ero.live" "0"|"1", "ero.diag" "0"|"1", "ero.ck" "steps:max"|"default", "ero.near" n|"default", "ero.mem_budget" bytes|"-1"
 *                                          scheduling knobs of the multi-version erosion scheduler (terra_set_erosion_tuning has the documented ones) */
int  terra_set_option(terra_ctx *ctx, const char *key, const char *value);
/* ---- whole grids between host and device.  The reference's callers own HOST arrays (cached_vals of build_arrays, src/mesh_gen.cpp:597-603; apply_erosion's float*,
 * src/erosion.cpp:14; heightmap_t's pixels, src/heightmap.cpp:130-151), 1 GiB at 16384^2.  Every host-pointer entry point moves arrays of >= 16 MiB in 8 MiB bands on four
 * streams at once through pinned staging (csrc/terra_xfer.hpp); an array allocated with terra_host_alloc (pinned) is the DMA target itself, no staging copy.
 * terra_download_async: d_src -> h_dst behind everything enqueued on ctx so far, without blocking the host or the context's later kernels (the next map's noise runs
 * beside the copy); h_dst is complete when terra_download_wait returns.  One context = one thread at a time, as everywhere. */
void *terra_host_alloc(size_t bytes);   /* NULL + terra_last_error() when pinned memory is exhausted */
void terra_host_free(void *p);
int  terra_download_async(terra_ctx *ctx, const void *d_src, void *h_dst, size_t bytes);
int  terra_download_wait(terra_ctx *ctx);
/* give every grow-only work buffer of the context back to the device (synchronises first; they grow again on demand).  The one that matters is the speculation ring of
 * terra_apply_erosion_dev: ~266 KiB per droplet in flight, 8.5 GiB for a 16384^2 map -- its size is also capped by the memory that is free when it has to grow. */
int  terra_release_scratch(terra_ctx *ctx);

/* ---- events: stream-level ordering between contexts (hipEventRecord / hipStreamWaitEvent; the host never blocks).  The engine keeps several generator objects in
 * flight (height_gens[8], src/tiled_mesh.h:418); here one context can produce (noise of map i, recorded) what another consumes (erosion of map i, its stream waits):
 * terra_event_record marks everything enqueued so far on ctx's stream, terra_event_wait makes everything enqueued on ctx's stream from now on wait for the last
 * record of ev.  Record before you wait (host order is the caller's business).  An event may be recorded again once its waits have been enqueued. */
typedef struct terra_event terra_event;
int  terra_event_create(terra_ctx *ctx, terra_event **out);
int  terra_event_record(terra_ctx *ctx, terra_event *ev);
int  terra_event_wait(terra_ctx *ctx, terra_event *ev);
/* the HOST waits until everything before the last record of ev has completed (hipEventSynchronize; returns at once for an event that was never recorded).  A thread that
 * drives the next heightmap can wait for the previous map's noise kernel itself -- not for the thread that launched it to wake up, notice and tell it */
int  terra_event_synchronize(terra_event *ev);
void terra_event_destroy(terra_event *ev);

/* ---- scene / globals.  terra_init_scene = main()'s start-up sequence for this path (src/3DWorld.cpp:2393-2460 -> gen_mesh). */
int  terra_init_scene(terra_ctx *ctx, const terra_config *cfg);
int  terra_set_config(terra_ctx *ctx, const terra_config *cfg);   /* store the config-file values only (engine integration: follow with terra_set_state) */
int  terra_get_state(terra_ctx *ctx, terra_state *out);
int  terra_set_state(terra_ctx *ctx, const terra_state *in);
int  terra_set_mode(terra_ctx *ctx, int mesh_gen_mode, int mesh_gen_shape);
int  terra_set_zmax_est(terra_ctx *ctx, float zmax_est);          /* set_zmax_est + zmin/zmax/water_plane_z, src/mesh_gen.cpp:162-167,494-512 */
int  terra_set_water_plane_z(terra_ctx *ctx, float water_plane_z);
int  terra_set_start_eval_sin(terra_ctx *ctx, int start_eval_sin);
int  terra_set_erode_amount(terra_ctx *ctx, float erode_amount);
float terra_get_max_sea_level(terra_ctx *ctx);                    /* src/tiled_mesh.cpp:141 */

/* ---- generator: mesh_xy_grid_cache_t (src/mesh.h:22-45).  One handle per in-flight grid, like height_gens[8] (src/tiled_mesh.h:418). */
int  terra_gen_create(terra_ctx *ctx, terra_gen **out);
void terra_gen_destroy(terra_gen *g);                              /* ~mesh_xy_grid_cache_t / clear_context */
/* build_arrays: returns 1 = results available, 0 = launched and not ready (only with TERRA_GEN_NO_WAIT), <0 = error.
 * Same async protocol as the GL path (src/mesh_gen.cpp:597-603): call again with the same arguments to collect.
 * min_start_sin: the first sine term the caller's eval_index() calls will ask for (0 when unknown): the device grid is evaluated from
 * max(start_eval_sin, min_start_sin), e.g. 50 for tile_t::create_texture's noise field (src/tiled_mesh.cpp:1099,1114). */
int  terra_gen_build_arrays(terra_gen *g, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin);
int  terra_gen_enable_glaciate(terra_gen *g);                      /* must follow build_arrays, as in the reference */
int  terra_gen_is_running(terra_gen *g);                           /* compute_shader_t::get_is_running (src/shaders.h:233) */
int  terra_gen_collect(terra_gen *g, float *host_out);            /* blocks; copies nx*ny floats (cached_vals) */
/* eval_index(x, y, min_start_sin, use_cache) (src/mesh.h:42, src/mesh_gen.cpp:754-792) on collected values.  Sine mode: the sum starts at
 * max(start_eval_sin, min_start_sin) unless use_cache && TERRA_GEN_CACHE_VALUES was given (cached values are built with min_start_sin = 0); when that is not
 * the first term the device grid was evaluated with, the grid is evaluated once more for it (kept until the next build).  fBm modes ignore both arguments. */
float terra_gen_eval_index(terra_gen *g, uint32_t x, uint32_t y, int min_start_sin, int use_cache);
const float *terra_gen_device_values(terra_gen *g);                /* device pointer to the nx*ny grid (valid until the next build) */

/* one-shot: build_arrays + [enable_glaciate] + the caller's eval_index double loop (src/heightmap.cpp:135-143, src/tiled_mesh.cpp:495-514) */
int  terra_gen_grid_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out);
/* same, plus min(vals)/max(vals) folded into the grid kernel (what heightmap_t::run_erosion / get_heightmap_z_range compute next); synchronous */
int  terra_gen_grid_minmax_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *h_min, float *h_max);
/* the same with min / max left in DEVICE memory (d_minmax: 2 floats) and nothing read back: asynchronous.  With terra_apply_erosion_devmin_dev the whole
 * heightmap_t::proc_gen step (src/heightmap.cpp:135-169: eval loop, min(vals), apply_erosion) is enqueued without a host round trip in between */
int  terra_gen_grid_minmax_async_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *d_minmax);
/* terra_gen_grid_minmax_async_dev for one of several heightmaps in flight that take turns in their noise phase (3dworld_amd/pipeline.py), the turn in one call:
 *   argument checks -> tables (and the reset of the min / max words: they read nothing of the map before, so they are enqueued at once) -> the HOST waits for the last
 *   record of wait_for (may be NULL: no wait) -> the grid kernel over all but the last T rows -> turn is recorded (may be NULL) -> the grid kernel over the last T rows
 *   -> {min, max} into d_minmax.  A call that fails its argument checks enqueues nothing and waits for nothing.
 * T is option "sg.turn_rows".  The thread of the next map, waiting for `turn` through its own call's wait_for, has its tables built by then: it wakes and enqueues its
 * first grid launch while this map's last rows drain from the chip, instead of after them.  Values are those of terra_gen_grid_minmax_async_dev, bit for bit.
 * CONTRACT: when `turn` fires this map is NOT complete -- neither d_out nor d_minmax.  `turn` says only that the next noise phase may be enqueued; that the map is complete
 * is said by this context's stream order (terra_apply_erosion_devmin_dev on the same context, a terra_event_record after this call) or by terra_synchronize, by nothing else.
 * No split (turn recorded right behind the grid kernel, in front of the min / max conversion): T = 0, T covers the grid, the fBm modes, TERRA_GEN_FUSED / TERRA_GEN_FAST. */
int  terra_gen_grid_minmax_turn_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *d_minmax,
                                    terra_event *wait_for, terra_event *turn);
int  terra_gen_grid(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *h_out);
/* rows [row0, row0 + nrows) of the nx x ny grid only, d_out = nrows*nx floats; bit-identical to the same rows of the full-grid call (heightmap_t::proc_gen's
 * row loop is independent per row, src/heightmap.cpp:139-143): one heightmap as row strips on several GPUs.  h_min / h_max (optional, synchronous when given):
 * min / max of the strip -- min(vals) of the whole map is the minimum over the strips (one float through ncclAllReduce(min), see bench.py --workload strips). */
int  terra_gen_grid_rows_minmax_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin,
                                    uint32_t row0, uint32_t nrows, float *d_out, float *h_min, float *h_max);
/* the same with the strip's {min, max} left in DEVICE memory (d_minmax: 2 floats), nothing read back: the call only enqueues.  One rank's part of a step of the one-grid
 * pipeline with no host round trip: the strip's noise, ncclAllReduce(min) of d_minmax[0] on the same stream, terra_apply_erosion_devmin_dev on the eroding rank
 * (tools/bench_native_onegrid.c) */
int  terra_gen_grid_rows_minmax_async_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin,
                                          uint32_t row0, uint32_t nrows, float *d_out, float *d_minmax);

/* ---- point query and ground-mode post-pass
 * eval_mesh_sin_terms (src/mesh_gen.cpp:797-805): non-separable point query used for biome parameters / collision height; evaluated on the host.
 * glaciate() (src/mesh_gen.cpp:388-404): in-place apply_glaciate + apply_mesh_sine over the MESH_X x MESH_Y ground mesh (xoff2/yoff2 = scroll offsets);
 * h_zbottom_ztop (optional) receives {zbottom, ztop}. */
int  terra_eval_mesh_sin_terms(terra_ctx *ctx, float xv, float yv, float *out);
/* The all-modes point queries, batched (n points, xy[2 i] = x, xy[2 i + 1] = y), evaluated on the device:
 *   TERRA_POINTS_SCALED  out[i] = eval_mesh_sin_terms_scaled(x, y, xy_scale) (src/mesh_gen.cpp:807-813): index-space coordinates; sine mode = the sine sum scaled and shaped,
 *                        the fBm modes go to get_noise_zval (the detail noise of heightmap tiles src/tiled_mesh.cpp:499-503, density fields)
 *   TERRA_POINTS_EXACT   out[i] = get_exact_zval(x, y, no_xyoff) (src/mesh_gen.cpp:816-847): world-space point -> index space (+ xoff2 / yoff2, the reference's scroll-offset
 *                        globals, unless no_xyoff) -> the heightmap texture (+ detail noise) when terra_hmap_set_dev gave one, else noise + apply_glaciate +
 *                        apply_mesh_sine (islands, volcano).  What collision / building placement / biome code calls (src/tiled_mesh.cpp:332-338, src/voxels.cpp:434).
 * Not covered: get_exact_zval's two branches that only read the caller's state -- the ground-mode mesh_height[][] look-up (:821-825) and the constant returned while a named
 * texture is not loaded yet (:839-843).  xy_scale is ignored by TERRA_POINTS_EXACT; no_xyoff / xoff2 / yoff2 by TERRA_POINTS_SCALED. */
#define TERRA_POINTS_SCALED 0u
#define TERRA_POINTS_EXACT  1u
int  terra_eval_points(terra_ctx *ctx, const float *xy, uint32_t n, uint32_t kind, float xy_scale, int no_xyoff, int xoff2, int yoff2, float *out);
int  terra_eval_points_dev(terra_ctx *ctx, const float *d_xy, uint32_t n, uint32_t kind, float xy_scale, int no_xyoff, int xoff2, int yoff2, float *d_out);
int  terra_glaciate_mesh_dev(terra_ctx *ctx, float *d_mesh, uint32_t nx, uint32_t ny, int xoff2, int yoff2, float *h_zbottom_ztop);

/* ---- erosion: apply_erosion (src/erosion.cpp:14).  In place; silently returns TERRA_OK when num_iters == 0 or erode_amount <= 0.
 * num_iters (and erosion_iters_tt of the tile calls) above 27 183 336 is TERRA_ERR_ARG: the reference's `int` seed 79*iter+121 of droplet iter = 27 183 336 overflows (undefined). */
int  terra_apply_erosion_dev(terra_ctx *ctx, float *d_heightmap, int xsize, int ysize, float min_zval, uint32_t num_iters, uint32_t flags);
/* min_zval read from device memory (one float, e.g. d_minmax of terra_gen_grid_minmax_async_dev -- possibly written by ANOTHER context's stream that this context's
 * stream was made to wait for) when the final clamp runs, the only use apply_erosion makes of it (src/erosion.cpp:158-162) */
int  terra_apply_erosion_devmin_dev(terra_ctx *ctx, float *d_heightmap, int xsize, int ysize, const float *d_min_zval, uint32_t num_iters, uint32_t flags);
int  terra_apply_erosion(terra_ctx *ctx, float *h_heightmap, int xsize, int ysize, float min_zval, uint32_t num_iters);
/* ---- the erosion of ONE grid whose row strips live on several GPUs (terra_dgrid below), with the sparse scheduler's read-only phases run where the
 * rows live.  apply_erosion (src/erosion.cpp:14) is one serial droplet order over the whole map, so it is the eroding rank that checks and commits -- but the first step of
 * every droplet and the trace of the ones that move read the ORIGINAL grid only, and a droplet spends its life near where it starts: rank r probes / traces the droplets
 * that start in its rows into its own HBM, the eroding rank fetches the (small) traces over xGMI instead of walking remote rows window by window.
 *   every rank r (the eroding one too), once the whole grid is written:
 *       terra_erosion_shard_trace_dev(ctx, d_grid, xsize, ysize, num_iters, row0_r, nrows_r, d_arena_r)
 *   the eroding rank, once every rank's trace call has completed (the caller's collective / event):
 *       terra_erosion_shard_finish_dev(ctx, d_grid, xsize, ysize, d_min_zval, num_iters, flags, world, self, row_end, d_arena_self, arena_stride)
 *         = terra_apply_erosion_devmin_dev on the same grid, bit for bit (the traces are the ones it would have made itself).
 * d_arena_r: terra_erosion_shard_arena_bytes() bytes of rank r's memory, all of them mapped on the eroding rank arena_stride bytes apart in rank order (one more
 * terra_dgrid whose strips are the arenas); row_end[r] = first row after rank r's strip (row_end[world - 1] = ysize); world <= 16.  Runs the sparse scheduler would not
 * take (many droplets on a small map) make the trace call a no-op and the finish call the ordinary erosion.  Not with TERRA_ERODE_SERIAL*. */
size_t terra_erosion_shard_arena_bytes(terra_ctx *ctx, uint32_t num_iters);
int  terra_erosion_shard_trace_dev(terra_ctx *ctx, float *d_heightmap, int xsize, int ysize, uint32_t num_iters, uint32_t row0, uint32_t nrows, void *d_arena);
int  terra_erosion_shard_finish_dev(terra_ctx *ctx, float *d_heightmap, int xsize, int ysize, const float *d_min_zval, uint32_t num_iters, uint32_t flags,
                                    uint32_t world, uint32_t self, const uint32_t *row_end, void *d_arena_self, size_t arena_stride);
int  terra_get_erosion_report(terra_ctx *ctx, terra_erosion_report *out);
/* tuning of the speculative scheduler (0 keeps a value): droplets in flight (ring slots; default automatic from the grid size, 0xFFFFFFFF restores that; at most
 * 2^20 is accepted, and a run uses at most (2^25 - 1)/block_list_capacity slots: version pages are addressed with 31-bit float indices),
 * log_capacity_log2: ignored (range-checked only) -- a droplet's writes are kept as one 64-cell page per 8x8 block of its footprint, there is no hashed log to size,
 * per-droplet block-list capacity = pages per droplet (16 .. 256, larger values mean 256).  A droplet whose footprint overflows it runs alone, in order, directly on
 * the grid (still exact).
 * slice_steps: while droplets wait for a slot a trace advances at most this many steps per round (default 96), except the 128 droplets next in line for the
 * commit, which trace to the end; a droplet's first trace is visible to the droplets after it from its first slice on (what it has written back so far).
 * Results never depend on any of these. */
int  terra_set_erosion_tuning(terra_ctx *ctx, uint32_t window, uint32_t log_capacity_log2, uint32_t block_list_capacity);
int  terra_set_erosion_slice_steps(terra_ctx *ctx, uint32_t slice_steps);

/* ---- whole heightmap: heightmap_t::proc_gen (src/heightmap.cpp:130-151) minus run_city_gen.
 * d_vals: width*height floats (final z); d_pixels16: optional 2 bytes per pixel {lo, hi} (from_floats/write_pixel_16_bits);
 * h_range: optional {min_z, dz} used for the 16-bit scale. */
int  terra_heightmap_proc_gen_dev(terra_ctx *ctx, uint32_t width, uint32_t height, uint32_t erosion_iters, float *d_vals, uint8_t *d_pixels16, float *h_range);
/* the same with the 16-bit pixels delivered to HOST memory (h_pixels16: 2*width*height bytes, what proc_gen leaves in the texture): the drop-in for the whole body of
 * heightmap_t::proc_gen when there are no cities -- 2 bytes per cell cross the host link instead of three float grids */
int  terra_heightmap_proc_gen(terra_ctx *ctx, uint32_t width, uint32_t height, uint32_t erosion_iters, uint8_t *h_pixels16, float *h_range);
int  terra_minmax_dev(terra_ctx *ctx, const float *d_vals, size_t n, float *h_min, float *h_max); /* synchronous */
int  terra_quantize16_dev(terra_ctx *ctx, const float *d_vals, size_t n, float min_z, float dz, uint8_t *d_pixels16);

/* ---- the loaded-heightmap path: heightmap_t::to_floats / from_floats / postprocess_height (src/heightmap.cpp:117-128,191-215), what
 * terrain_hmap_manager_t::load runs right after reading the PNG (src/heightmap.cpp:351), e.g. scene_config/config_heightmap.txt:78-87.
 * terra_set_mesh_file_scale = the two numbers of the config line `mh_filename <png> <mesh_file_scale> <mesh_file_tz>` (src/3DWorld.cpp:2205): a pixel value
 * v in [0, 256) is the height get_mh_texture_mult()*v + get_mh_texture_add() (src/mesh_gen.cpp:122-123); terra_set_mesh_height_scales_for_zval_range sets the same pair.
 * d_pixels: width*height pixels in device memory, 1 byte each or 2 = {fraction, integer}.
 * to_floats: pixels -> heights.  from_floats: heights -> pixels with the scale in force (8-bit: truncation; 16-bit: write_pixel_16_bits).
 * postprocess: to_floats -> run_erosion (apply_erosion over the whole image, min_zval = min(vals), erosion_iters_tt droplets) -> from_floats, in place;
 *   nothing happens when erosion_iters_tt == 0 (run_city_gen is another subsystem).  d_vals: width*height floats of device scratch that is left holding the
 *   eroded heights, or NULL (allocated internally).
 * h_out_of_range (optional): number of values that map outside [0, 256) -- the reference asserts on those (src/heightmap.cpp:210); with NULL such an image is
 * TERRA_ERR_STATE (the pixels are still written, with the x86 conversion's wrap-around). */
int  terra_set_mesh_file_scale(terra_ctx *ctx, float mesh_file_scale, float mesh_file_tz);
int  terra_get_mesh_file_scale(terra_ctx *ctx, float *mesh_file_scale, float *mesh_file_tz);
int  terra_heightmap_to_floats_dev(terra_ctx *ctx, const uint8_t *d_pixels, uint32_t width, uint32_t height, int ncolors, float *d_vals);
int  terra_heightmap_from_floats_dev(terra_ctx *ctx, const float *d_vals, uint32_t width, uint32_t height, int ncolors, uint8_t *d_pixels, uint32_t *h_out_of_range);
int  terra_heightmap_postprocess_dev(terra_ctx *ctx, uint8_t *d_pixels, uint32_t width, uint32_t height, int ncolors, uint32_t erosion_iters_tt, float *d_vals, uint32_t *h_out_of_range);

/* ---- the ground mesh's text file: read_mesh / write_mesh (src/mesh_gen.cpp:895-965), e.g. BASELINE config 1's `mesh_file mapx/mesh128.txt` (src/3DWorld.cpp:2206).
 * Format: "nx ny" then ny rows of nx heights (written with "%f ").  Host functions, like the PNG ones: the file is a few hundred KB and is parsed with the C library's
 * own fscanf, so every height has the bits the reference reads.
 * terra_read_mesh: the header must equal (nx, ny) = the scene's MESH_X_SIZE x MESH_Y_SIZE (the reference refuses other sizes); h_mesh[i*nx + j] = mesh_file_scale*height +
 *   mesh_file_tz (terra_set_mesh_file_scale); then calc_zminmax, set_zmax_est(zmm != 0 ? zmm : max(-zmin, zmax)) and set_zvals: the context's zmin / zmax / zmax_est /
 *   water_plane_z are what the engine's globals are after read_mesh (terra_get_state).  h_zbottom_ztop (optional) receives the mesh's own {min, max} (set_zvals' zbottom / ztop).
 *   Returns TERRA_ERR_ARG for a missing file, a short file or a size mismatch (the reference prints an error and returns 0); h_mesh may then be partly written, the state is untouched.
 * terra_write_mesh: the inverse (no scale is applied, as in the reference). */
int  terra_read_mesh(terra_ctx *ctx, const char *filename, float zmm, float *h_mesh, uint32_t nx, uint32_t ny, float *h_zbottom_ztop);
int  terra_write_mesh(const char *filename, const float *h_mesh, uint32_t nx, uint32_t ny);

/* ---- tiles: tile_t::create_zvals batch.  The tile size S is get_tile_size() = MESH_X_SIZE = the scene's mesh_x (src/tiled_mesh.cpp:142); every tile buffer is
 * sized from it (the numbers in brackets are S = 128, the size every call supports):
 *   zvals  [n][S+2][S+2] floats         ([n][130][130])    tile (tx, ty) covers cells x1 = tx*S .. x1 + S + 1, y1 = ty*S .., field origin x1 - mesh_x/2, y1 - mesh_y/2
 *   normals [n][S+1][S+1][4] bytes      ([n][129][129][4]) RGBA8, A = 0
 *   AO     [n][S+1][S+1] bytes          ([n][129][129])    from an (S+73)^2 context at (x1 - 36, y1 - 36) (201^2)
 *   smask  [n][S+2][S+2] bytes          ([n][130][130])
 *   stats: 4 x 4 sub-blocks of block_size = (S+2)/4 cells (32), radius from (DX^2 + DY^2)*S*S.
 * Supported: 16 <= S <= 1024; S other than 128 also needs mesh_x == mesh_y (the reference asserts it in tiled mode) and S != 4k + 2 (the reference's sub-block
 * loop would read past the zvals there); otherwise every tile call is TERRA_ERR_ARG.  At S != 128 these entry points follow S: terra_tiles_create_zvals[_dev]
 * (all three field sources: procedural, the AO-context clip, the heightmap texture), terra_tiles_post[_dev], terra_tiles_ao_lighting[_dev],
 * terra_tiles_mesh_shadows[_dev], terra_tiles_line_intersect[_dev] and terra_multi_tiles_create_zvals[_dev].  These are TERRA_ERR_ARG at S != 128 for now: terra_tiles_terrain_params,
 * terra_tiles_create_weights[_dev], terra_tiles_edit_grass[_dev], terra_tiles_tree_weights[_dev], terra_tiles_mesh_shadows_halo_dev / _edges_dev, terra_multi_tiles_mesh_shadows[_dev] and terra_multi_shadow_layout.
 * terra_tile_size: *size = S of the scene in force (TERRA_ERR_ARG when the scene's S is not supported, TERRA_ERR_STATE before terra_init_scene).
 * tile_xy: n pairs (tile x, tile y) on the HOST.  d_zvals: n zvals.  d_stats: n terra_tile_stats (optional).
 * d_normals: n normals (optional); d_min_normal_z: n floats (optional). */
int  terra_tile_size(terra_ctx *ctx, uint32_t *size);
int  terra_tiles_create_zvals_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, uint32_t erosion_iters_tt,
                                  float *d_zvals, terra_tile_stats *d_stats, uint8_t *d_normals, float *d_min_normal_z);
int  terra_tiles_create_zvals(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, uint32_t erosion_iters_tt,
                              float *h_zvals, terra_tile_stats *h_stats, uint8_t *h_normals, float *h_min_normal_z);
/* the stats + normals pass alone, over zvals the caller HAS (edited with the brushes, eroded elsewhere, read from a file): the sub-block / water-bbox loop of
 * tile_t::create_zvals (src/tiled_mesh.cpp:517-541) and tile_t::upload_normal_texture (src/tiled_mesh.cpp:865-880), which the engine also runs on its own whenever a
 * tile's heights changed.  d_zvals is not written.  Outputs as above (each optional). */
int  terra_tiles_post_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, terra_tile_stats *d_stats, uint8_t *d_normals, float *d_min_normal_z);
int  terra_tiles_post(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, terra_tile_stats *h_stats, uint8_t *h_normals, float *h_min_normal_z); /* host arrays */
/* self test: the droplet step takes its two square roots per step with a shortened instruction sequence (csrc/terra_erosion.hpp: sqrt_rn); this runs it over every
 * stride-th fp32 bit pattern (stride 1: all 2^32, a few ms on the GPU) against sqrtf and against the correctly rounded double-precision route; the tile normals' byte test
 * (csrc/terra_kernels.hpp: k_tile_post) relies on the hardware's reciprocal square root being within 2^-23 of the real one, checked over the same inputs.  *mismatches must be 0. */
int  terra_selftest_hot_sqrt(terra_ctx *ctx, uint32_t stride, uint64_t *mismatches);

/* ---- heightmap files, host side: 8- / 16-bit grayscale PNG exactly as the reference reads / writes them through libpng (src/image_io.cpp:493-605):
 * write: rows in memory order, 16-bit pixels {fraction, integer} -> big-endian samples (heightmap_t::write_png, src/heightmap.cpp:375-378);
 * read: file row i -> memory row height-1-i (texture_t::load_png flips), allow_two_byte_grayscale keeps 16 bits as 2 bytes per pixel, otherwise the
 * high byte only.  h_pixels may be NULL to query the size (width*height*ncolors bytes).  Non-grayscale / interlaced files are refused. */
int  terra_heightmap_write_png(const char *path, const uint8_t *h_pixels, uint32_t width, uint32_t height, int ncolors);
int  terra_heightmap_read_png(const char *path, int allow_two_byte_grayscale, uint32_t *width, uint32_t *height, int *ncolors, uint8_t *h_pixels, size_t capacity);

/* ---- tiles from a heightmap texture instead of the procedural generator: terrain_hmap_manager_t (src/heightmap.h:110-142).
 * d_pixels: width*height pixels in DEVICE memory, 1 byte each or 2 = {fraction, integer} as written by terra_quantize16_dev / write_pixel_16_bits;
 * the library keeps the pointer (no copy), NULL switches back to procedural tiles.  While set, terra_tiles_create_zvals samples
 * get_clamped_height(x1 + x, y1 + y) (nearest for mesh_scale >= 1, bilinear below, mirror-wrapped outside the image; src/heightmap.cpp:310-402), adds
 * HMAP_DETAIL_MAG * the detail noise grid when mesh_scale < 0.75, skips erosion (src/tiled_mesh.cpp:499-503,515) and the AO context does the same (:623-627).
 * terra_set_mesh_height_scales_for_zval_range = src/mesh_gen.cpp:125-131 (pixel value -> height, e.g. range[0], range[1]/255 of terra_heightmap_proc_gen_dev). */
int  terra_hmap_set_dev(terra_ctx *ctx, const uint8_t *d_pixels, int width, int height, int ncolors);
int  terra_set_mesh_height_scales_for_zval_range(terra_ctx *ctx, float min_z, float dz);

/* ---- height edits of the heightmap texture (tex_mod_map_manager_t / terrain_hmap_manager_t, src/heightmap.h:38-142, src/heightmap.cpp:27-58,99-115,216-308,
 * 414-440): brushes, the per-texel mod map and the .mod file that stores both.  The records have the reference's in-memory = on-disk layouts.
 * The *_dev calls edit the image registered with terra_hmap_set_dev in place (it must be writable device memory, at most 65536 texels per side, 16-bit
 * images 2-byte aligned; a texel is updated by a compare-and-swap on the aligned 32-bit word around it, so when the image does not start / end on a
 * 4-byte boundary the up to 3 neighbouring bytes are re-written with their own values: nothing else may modify them during an edit call); a brush
 * point (xp, yp, sub-step) lands on texel clamp_xy(xp + dx, yp + dy) (mesh_scale, mirror wrap) and adds round_fp(delta * weight(shape, dist / radius)) with
 * clamping to the pixel range, flatten brushes store delta.  Brushes are applied in list order (apply_cur_brushes); within one brush the reference's
 * OpenMP loop order is immaterial (same-signed saturating adds commute) and so is the thread order here. */
enum {TERRA_BSHAPE_CONST_SQ = 0, TERRA_BSHAPE_CNST_CIR, TERRA_BSHAPE_LINEAR, TERRA_BSHAPE_QUADRATIC, TERRA_BSHAPE_COSINE, TERRA_BSHAPE_SINE, TERRA_BSHAPE_FLAT_SQ, TERRA_BSHAPE_FLAT_CIR, TERRA_NUM_BSHAPES};
typedef struct terra_hmap_brush {int32_t x, y; uint32_t radius; int32_t delta; int16_t shape;} terra_hmap_brush; /* hmap_brush_t, src/heightmap.h:71-76 (20 bytes) */
typedef struct terra_hmap_mod {uint16_t x, y; int32_t delta;} terra_hmap_mod;                                    /* mod_elem_t, src/heightmap.h:59-64 (8 bytes) */
int  terra_hmap_apply_brushes_dev(terra_ctx *ctx, const terra_hmap_brush *brushes, uint32_t n, int step_sz, uint32_t num_steps); /* apply_brush(brush, step_sz, num_steps) for each */
int  terra_hmap_apply_mods_dev(terra_ctx *ctx, const terra_hmap_mod *mods, uint32_t n);      /* add_mod for each (deltas of one texel are summed) + apply_cur_mod_map */
int  terra_hmap_read_and_apply_mod_dev(terra_ctx *ctx, const char *path);                   /* read_and_apply_mod: mods, then brushes with step_sz = num_steps = 1 */
int  terra_hmap_write_mod(const char *path, const terra_hmap_mod *mods, uint32_t n, const terra_hmap_brush *brushes, uint32_t n_brushes); /* write_mod */
/* read_mod: counts always; records when the buffers are non-NULL and large enough (capacities in records).  Mods come back combined, in map order. */
int  terra_hmap_read_mod(const char *path, terra_hmap_mod *mods, uint32_t mods_capacity, uint32_t *n_mods, terra_hmap_brush *brushes, uint32_t brushes_capacity, uint32_t *n_brushes);
/* ---- the map-view heightmap exporter write_map_mode_heightmap_image (src/map_view.cpp:409-442) from the image origin on: width x height cells starting at
 * scene position (xstart, ystart) with the mesh spacing, rows inverted, 16-bit pixels = (h - min_z) * (255 / dz).  d_vals: width*height floats (the
 * reference's `heights`), d_pixels16: 2 bytes per pixel or NULL, h_min_z_dz: {min_z, dz} or NULL.  With a heightmap texture set the heights are sampled
 * from it (get_mesh_height, src/map_view.cpp:97-105).  terra_write_map_mode_heightmap_image = the same + the PNG file. */
int  terra_export_heightmap_dev(terra_ctx *ctx, float xstart, float ystart, uint32_t width, uint32_t height, float *d_vals, uint8_t *d_pixels16, float *h_min_z_dz);
int  terra_write_map_mode_heightmap_image(terra_ctx *ctx, const char *path, float xstart, float ystart, uint32_t width, uint32_t height);

/* ---- tile ambient-occlusion lighting: tile_t::calc_mesh_ao_lighting (src/tiled_mesh.cpp:586-661).  zvals: [n][S+2][S+2] exactly as
 * terra_tiles_create_zvals left them (eroded or not); ao: [n][S+1][S+1] bytes = (unsigned char)(255*(1 - atten/64)).  The (S+73)^2 context
 * around each tile is generated internally (setup_height_gen_async(x1 - 36, y1 - 36, S+73, S+73); 201 at S = 128).
 * terra_set_tiled_mesh_ao = the config key enable_tiled_mesh_ao (src/3DWorld.cpp:1778; scene_config/config.txt turns it on): with mesh_gen_mode >= 3 the
 * reference clips a tile's zvals out of that context grid instead of a 130 x 130 grid of its own (src/tiled_mesh.cpp:478-488,505), which changes
 * their low bits; terra_tiles_create_zvals follows the flag. */
int  terra_set_tiled_mesh_ao(terra_ctx *ctx, int enable);
int  terra_tiles_ao_lighting_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, uint8_t *d_ao);
int  terra_tiles_ao_lighting(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, uint8_t *h_ao);

/* ---- landscape weights texture of a tile (tile size 128 only): tile_t::create_texture (src/tiled_mesh.cpp:1071-1240) with update_terrain_params (:321-343), get_tids /
 * update_lttex_ix (src/Textures.cpp:1289-1316) and add_grass_block_at (src/tiled_mesh.cpp:1354-1371).  Terrain-only branch: the city, tunnel and building
 * queries come from subsystems outside this library (their texels are the caller's to overwrite afterwards, as the reference does); the tree map's texels are
 * terra_tiles_tree_weights[_dev]'s, below: mesh_weight_data is what this call writes, weight_data what that one makes of it.
 * zvals: [n][130][130]; weights: [n][129][129][4] bytes RGBA = {sand, dirt, grass, rock}, snow = remainder; grass_blocks: [n][32][32] or NULL;
 * has_any_grass: [n] bytes or NULL.  The second noise field (build_arrays(..., 80*DX_VAL, 80*DY_VAL, 129, 129, 0, force_sine_mode=1) + eval_index(x, y, 50))
 * and the biome parameters are generated internally.  terra_tiles_terrain_params returns those parameters: [n][2][2][3] = [yp][xp]{veg, grass, dirt}. */
int  terra_set_landscape(terra_ctx *ctx, const terra_landscape *params);
int  terra_get_landscape(terra_ctx *ctx, terra_landscape *out);
int  terra_tiles_terrain_params(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, float *h_params);
int  terra_tiles_create_weights_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, uint8_t *d_weights, terra_grass_block *d_grass_blocks, uint8_t *d_has_any_grass);
int  terra_tiles_create_weights(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, uint8_t *h_weights, terra_grass_block *h_grass_blocks, uint8_t *h_has_any_grass);
/* ---- grass brush on those weights (tile size 128 only): the fire modes "Add Grass" / "Remove Grass" (inf_terrain_fire_weapon, src/tiled_mesh.cpp:4004-4011) ->
 * tile_draw_t::add_or_remove_grass_at (:3771-3774) -> tile_t::add_or_remove_grass_at (:3845-3948) on every tile of the batch, in place.  Per tile the call does
 * everything from :3847 on: the rradius == 0 test, mesh_sphere_intersect (:3796-3799), the texel loop, add_grass_block_at (:1354-1371, with its is_distant /
 * x >= size / gen_grass_map() early-outs) and, after a removal, the has-grass scan that clears every grass block (:3938-3945).  The caller keeps the early
 * returns for "texture not generated" and weights_tsize != stride (city tiles) and the follow-ups flowers.update_subrange / create_or_update_weight_tex, for
 * which updated[t] (0 / 1) and ranges[t] = {xl, yl, xh, yh} are returned (add only; they start denormalised at {128, 128, 0, 0}, as at :3863).
 * dxoff / dyoff = xoff - xoff2 / yoff - yoff2.  stats: what terra_tiles_create_zvals returned (mzmin, mzmax and radius are read; the engine may have enlarged radius
 * for trees).  is_distant: [n] bytes or NULL (none distant).  Layouts of terra_tiles_create_weights: weights [n][129][129][4] (4-byte aligned), grass blocks
 * [n][32][32]: a tile whose blocks all have ix == 0 has an empty grass_blocks vector, cleared blocks become {0, 0, 0}.  has_any_grass is not touched (the
 * reference does not touch it either).  The biome parameters of the dirt scale (:3917) are generated internally.  ranges may be NULL. */
typedef struct terra_grass_brush {
	float pos[3];       /* p_int, camera space */
	float radius;       /* rradius = (bradius + 0.5)*HALF_DXY, computed by the caller */
	int32_t add_grass;  /* FM_ADD_GRASS (1) vs FM_REM_GRASS (0) */
	int32_t shape;      /* TERRA_BSHAPE_* */
	float brush_weight; /* cur_brush_param.get_delta_mag() */
} terra_grass_brush;
int  terra_tiles_edit_grass_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff,
                                const float *d_zvals, const terra_tile_stats *d_stats, const uint8_t *d_is_distant, const terra_grass_brush *brush,
                                uint8_t *d_weights, terra_grass_block *d_grass_blocks, uint8_t *d_updated, uint32_t *d_ranges);
int  terra_tiles_edit_grass(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff,
                            const float *h_zvals, const terra_tile_stats *h_stats, const uint8_t *h_is_distant, const terra_grass_brush *brush,
                            uint8_t *h_weights, terra_grass_block *h_grass_blocks, uint8_t *h_updated, uint32_t *h_ranges);

/* ---- line-vs-terrain hits on a tile batch (every supported tile size S): what aims the terrain fire modes (inf_terrain_fire_weapon, src/tiled_mesh.cpp:3983-4020)
 * and serves projectiles, animals' sight lines and cars.  Per line: tile_draw_t::line_intersect_mesh (:3582-3605) with inc_trees = 0 -> tile_t::line_intersect_mesh
 * (:2176-2213) on every tile, bit for bit; p_int = v1 + t*(v2 - v1) as line_intersect_tiled_mesh_get_tile (:3643-3648) computes it.
 * tile_xy: n pairs on the HOST.  dxoff / dyoff = xoff - xoff2 / yoff - yoff2.  zvals [n][S+2][S+2] and stats (mzmin / mzmax are read) as terra_tiles_create_zvals
 * returned them.  is_distant: [n] bytes or NULL (none distant); a distant tile never hits (:2178).  lines: [nlines][2][3] = v1, v2 in camera space.
 * line_tile: [nlines] or NULL; line_tile[r] >= 0 tests line r against that batch tile alone (tile_t::line_intersect_mesh, as animals.cpp calls it), a negative entry
 * against the whole batch.  The host form refuses an entry >= n (TERRA_ERR_ARG); the device form cannot read it up front, there such a line is a miss.
 * hits: one record per line.  A hit: t = the winning tn, tile = its batch index, (xpos, ypos) = (x1 + ix, y1 + iy), global mesh indices without the scroll offset as
 * the reference's, and hit = 1.  A miss: {t = 2, tile = -1, xpos = ypos = 0, p_int = {0, 0, 0}, hit = 0}.
 * Ties: over the tiles the reference keeps the first strictly smaller tn of its unordered_map's iteration order; here equal t go to the lowest batch index, so an
 * engine that passes its tiles in that iteration order gets the identical tile (tiles share their edge row and column: ties do happen).
 * Where the reference asserts, a line misses: a non-finite coordinate (:2179), and steps >= 10000 in a tile (:2187), which only a line longer than 10000 cells can
 * reach, when its clip leaves v2 where it was (tmax <= TOLERANCE).  A horizontal line never hits (its cur_t divides by v2.z - v1.z = 0), as in the reference.
 * TERRA_ERR_STATE before terra_init_scene; TERRA_ERR_ARG for an unsupported S or a NULL required pointer (tile_xy, zvals, stats when n > 0; lines, hits when
 * nlines > 0).  n == 0 writes misses; nlines == 0 does nothing.  The device form only enqueues. */
typedef struct terra_line_hit {
	float t;            /* cur_t of the winning tile, 2 on a miss */
	int32_t tile;       /* batch index, -1 on a miss */
	int32_t xpos, ypos; /* mesh indices of the hit cell */
	float p_int[3];     /* v1 + t*(v2 - v1) */
	uint32_t hit;       /* 0 / 1 */
} terra_line_hit;       /* 32 bytes */
int  terra_tiles_line_intersect_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff,
                                    const float *d_zvals, const terra_tile_stats *d_stats, const uint8_t *d_is_distant,
                                    const float *d_lines, const int32_t *d_line_tile, uint32_t nlines, terra_line_hit *d_hits);
int  terra_tiles_line_intersect(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff,
                                const float *h_zvals, const terra_tile_stats *h_stats, const uint8_t *h_is_distant,
                                const float *h_lines, const int32_t *h_line_tile, uint32_t nlines, terra_line_hit *h_hits);

/* ---- line queries with inc_trees = 1 on a tile batch (every supported tile size S): the hit-scan weapon path, line_intersect_tiled_mesh(pos, pos2, coll_pos, 1)
 * (src/Gameplay.cpp:2143).  Per line: tile_draw_t::line_intersect_mesh (src/tiled_mesh.cpp:3582-3604) over tile_t::line_intersect_mesh (:2176-2216) with
 * inc_trees != 0, bit for bit: small_tree_group::line_intersect with t != NULL (src/sm_tree.cpp:189-200), small_tree::line_intersect (:854-876) and
 * line_intersect_trunc_cone with check_ends = 0 (src/Math3d.cpp:543-593) with the source's operand types -- the double matrix M, matrix_mult's float x double sums,
 * m = 1.0/d of normalize(), 0.35*dirh narrowed per component, g = cosf(atan2f(r2, |A|)) with the C library's results (glibc 2.35), and `(1-2*i)*num` with its
 * unsigned i.  Where line_intersect_trunc_cone asserts (!(r2 > 0 && r2 > r1)) that cylinder does not hit; nothing else is special-cased.
 * Per (line, tile), in the reference's order: a distant tile returns 0 before the trees; a mesh hit returns cur_t and the tile's trees are not looked at, even when
 * one stands nearer; otherwise, when the tile holds a valid record, the trees run on (v1 - xlate, v2 - xlate) with xlate = ((dxoff + ptree_xoff2)*DX_VAL,
 * (dyoff + ptree_yoff2)*DY_VAL, 0), *t starting at 1.0: only a t_new < 1 hits, and within a tile the first record and cylinder that reaches the minimum wins.  The
 * gate is !all_bcube.is_zero_area() && !check_line_clip(p1, p2, all_bcube.d); a tile whose mesh box the line misses still tests its trees.  Only T_PINE and
 * T_SH_PINE records hit (two cylinders: trunk_cylin and the leaf cone from pos + 0.35*dirh, or pos for T_SH_PINE, to pos + dirh with get_radius()).
 * Records, validity and geometry are terra_tiles_tree_view's: the context's instance table and terra_tree_size_params, tree_depth_scale, trunk_override with
 * rotated != 0 as documented there.  Records that the tree view drops are skipped and do not enter all_bcube, which is calc_bcube() over the valid records,
 * computed by this call.  A count above the capacity means the first `capacity` records.
 * Over the tiles the strictly smaller tn wins, ties go to the lowest batch index (as terra_tiles_line_intersect).
 * zvals, stats, is_distant, lines, line_tile, misses, non-finite lines and n == 0 / nlines == 0: as terra_tiles_line_intersect.  hits, one record per line:
 * a mesh hit has hit = TERRA_LINE_HIT_MESH, tree = -1, part = 0 and the fields of terra_line_hit; a tree hit has hit = TERRA_LINE_HIT_TREE, xpos = ypos = 0 (the
 * reference leaves new_xpos / new_ypos at 0), tree = the record index in its tile, part = 0 (trunk_cylin) or 1 (the leaf cone) and p_int = v1 + t*(v2 - v1) from
 * the untranslated ends; a miss has hit = 0, tree = -1, part = 0.  With pine == NULL, pine_counts == NULL or pine_capacity == 0 the first 32 bytes of every
 * record equal terra_tiles_line_intersect's, byte for byte.  terra_tiles_line_intersect[_dev] itself does not change.
 * TERRA_ERR_ARG, with nothing written: a NULL required pointer (in; tile_xy, zvals, stats when n > 0; lines, hits when nlines > 0); a pointer other than
 * is_distant that is not 4-byte aligned; tree_depth_scale not finite and > 0; `instanced` with an instance table of another length; an unsupported S;
 * n*pine_capacity beyond 32 bits; in the host form a line_tile entry >= n.  TERRA_ERR_STATE before terra_init_scene.  The device form only enqueues and reads
 * nothing back; tile_xy is a host array in both forms.  Scratch comes from the context's arena.  The kernels index nothing with a record's inst, a line_tile or a
 * count before its range is known. */
struct terra_tree_place;
struct terra_trunk_override;
typedef struct terra_line_trees_in {
	const float *zvals;                  /* [n][S+2][S+2] */
	const terra_tile_stats *stats;       /* [n] */
	const uint8_t *is_distant;           /* [n] or NULL */
	const struct terra_tree_place *pine; /* [n][pine_capacity] or NULL */
	const uint32_t *pine_counts;         /* [n] or NULL */
	const struct terra_trunk_override *trunk_override; /* [n][pine_capacity] or NULL */
	uint32_t pine_capacity;
	int32_t dxoff, dyoff;                /* xoff - xoff2, yoff - yoff2 */
	int32_t ptree_xoff2, ptree_yoff2;    /* what the placement ran with */
	float tree_depth_scale;
} terra_line_trees_in;      /* 72 bytes */
typedef struct terra_line_tree_hit {
	float t;            /* the winning tn, 2 on a miss */
	int32_t tile;       /* batch index, -1 on a miss */
	int32_t xpos, ypos; /* mesh indices of the hit cell; 0 for a tree */
	float p_int[3];     /* v1 + t*(v2 - v1) */
	uint32_t hit;       /* TERRA_LINE_HIT_* */
	int32_t tree;       /* record index in the tile, -1 unless a tree was hit */
	uint32_t part;      /* 0 trunk_cylin, 1 the leaf cone */
} terra_line_tree_hit;      /* 40 bytes */
enum {TERRA_LINE_HIT_NONE = 0, TERRA_LINE_HIT_MESH = 1, TERRA_LINE_HIT_TREE = 2};
int  terra_tiles_line_intersect_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_line_trees_in *in,
                                          const float *d_lines, const int32_t *d_line_tile, uint32_t nlines, terra_line_tree_hit *d_hits);
int  terra_tiles_line_intersect_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_line_trees_in *in,
                                      const float *h_lines, const int32_t *h_line_tile, uint32_t nlines, terra_line_tree_hit *h_hits);

/* ---- tree map of a tile batch (every supported tile size S): what the fire modes "Add Trees" / "Remove Trees" (src/tiled_mesh.cpp:3998-4002) leave for the terrain
 * to do.  tile_t::register_tree_change (:3789-3794) clears tree_map and forces the textures to be re-made; tile_t::pre_draw (:1900-1907) then runs apply_tree_ao_shadows,
 * create_texture and check_shadow_map_and_normal_texture.  The three calls below are the terrain side of those steps; trees themselves (generation, drawing,
 * collision) stay with the engine, which passes each tree as (pos.x, pos.y, tradius).
 * terra_tiles_tree_map: tile t owns splats[h_first[t] .. h_first[t+1]-1]; h_first ([n+1], non-decreasing) is on the HOST in both forms.  Per tile: reset != 0 fills
 * the map with 255 (tree_map.clear() + resize, :824-825), reset == 0 continues on the map as it is (a neighbour's push_tree_ao_shadow, :740-746); then every splat of
 * its list is the texel loop of tile_t::add_tree_ao_shadow (:751-767), in list order, bit for bit: the order matters, (uchar)((uchar)(255*a)*b) is not
 * (uchar)((uchar)(255*b)*a).  x, y: pos in the tile's camera-space frame (get_center() + pt_off, :791, or pos2 of :744); radius: get_ao_radius().
 * Here the caller builds the lists -- the own-tree loop, the eight neighbours in dy, dx order with the bounding-box cull of :793, the x_test / y_test border push of
 * :768-778 and the trmax < min(DX_VAL, DY_VAL) shortcut -- and add_tree_ao_shadow's body becomes "append to the tile's list": the call for engines that keep their
 * own trees.  terra_tiles_tree_ao_shadows, below, builds the lists on the device from the placement records.
 * tree_map: [n][S+1][S+1][2] bytes {ao, sh}, 2-byte aligned.  updated: [n] bytes or NULL; updated[t] = 1 when any texel of tile t was multiplied in this call
 * (:765, :779).  is_distant: [n] bytes or NULL; a distant tile is filled with 255 under reset and left alone otherwise, updated = 0 (:743, :822): an all-255 map reads
 * as the reference's empty tree_map in both consumers.  dxoff / dyoff = xoff - xoff2 / yoff - yoff2.
 * A splat is skipped where the reference is undefined: a non-finite member, radius < 0, rval = max(int(radius/DX_VAL), int(radius/DY_VAL)) + 1 > 46340 (rval*rval
 * overflows), |xc| or |yc| beyond 2^30.
 * TERRA_ERR_ARG: a NULL required pointer (tile_xy, h_first, tree_map when n > 0; splats when the lists are not empty), a decreasing h_first, an unsupported S.
 * TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing.  The device form only enqueues. */
typedef struct terra_tree_splat {float x, y, radius;} terra_tree_splat;
int  terra_tiles_tree_map_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *d_is_distant,
                              const terra_tree_splat *d_splats, const uint32_t *h_first, int32_t reset, uint8_t *d_tree_map, uint8_t *d_updated);
int  terra_tiles_tree_map(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *h_is_distant,
                          const terra_tree_splat *h_splats, const uint32_t *h_first, int32_t reset, uint8_t *h_tree_map, uint8_t *h_updated);
/* terra_tiles_shadow_texture: tile_t::upload_shadow_map_texture (:885-911), the RGBA8 texel {mesh shadow, tree shadow, ambient occlusion, 0} the engine uploads.
 * smask_sun / smask_moon: [n][S+2][S+2] as terra_tiles_mesh_shadows wrote them for get_light_pos(LIGHT_SUN / LIGHT_MOON); ao: [n][S+1][S+1] or NULL (170, the
 * reference's value without AO lighting); tree_map: as above or NULL (tree_map.empty()); shadow: [n][S+1][S+1][4], 4-byte aligned.  has_sun = light_factor >= 0.4,
 * has_moon = light_factor <= 0.6; mesh_shadows = mesh_shadows_enabled(): 0 leaves channel 0 at 255 and reads no mask.
 * TERRA_ERR_ARG where the reference asserts: mesh_shadows with the smask of a light that is up NULL (:888-889), neither light up (a NaN light_factor, :844);
 * also a NULL shadow with n > 0, a misaligned pointer, an unsupported S. */
int  terra_tiles_shadow_texture_dev(terra_ctx *ctx, uint32_t n, const uint8_t *d_smask_sun, const uint8_t *d_smask_moon, const uint8_t *d_ao, const uint8_t *d_tree_map,
                                    float light_factor, int32_t mesh_shadows, uint8_t *d_shadow);
int  terra_tiles_shadow_texture(terra_ctx *ctx, uint32_t n, const uint8_t *h_smask_sun, const uint8_t *h_smask_moon, const uint8_t *h_ao, const uint8_t *h_tree_map,
                                float light_factor, int32_t mesh_shadows, uint8_t *h_shadow);
/* terra_tiles_tree_weights (tile size 128 only): the tail of tile_t::create_texture (:1325-1348) with sz_factor == 1.  weights = mesh_weights; then, where the tree
 * map's ao != 255 and the texel's rock byte is not 255 (a city texel), grass under trees becomes dirt.  mesh_weights / weights: [n][129][129][4] as
 * terra_tiles_create_weights wrote them, 4-byte aligned; weights may be mesh_weights (in place), any other overlap is undefined.  tree_map: [n][129][129][2] or
 * NULL (the plain copy). */
int  terra_tiles_tree_weights_dev(terra_ctx *ctx, uint32_t n, const uint8_t *d_mesh_weights, const uint8_t *d_tree_map, uint8_t *d_weights);
int  terra_tiles_tree_weights(terra_ctx *ctx, uint32_t n, const uint8_t *h_mesh_weights, const uint8_t *h_tree_map, uint8_t *h_weights);

/* ---- pine / palm tree placement of a tile batch (every supported tile size S): the generating half of "Add Trees" and of tile_t::init_pine_tree_draw
 * (src/tiled_mesh.cpp:1430-1437).  The chain zvals -> tree placement -> terra_tiles_tree_ao_shadows (radii, splat lists and tree map) -> shadow texture and weights
 * runs without the host in between.
 * terra_tree_params: the globals this path reads beyond the scene (water_plane_z, zmax_est, glaciate_exp, relh_adj_tex: terra_state) and the landscape (vegetation,
 * biome_x_offset, enable_terrain_env: terra_landscape).  The defaults are the reference's; with tree_mode 1 no call places a tree.
 * TERRA_ERR_ARG: sm_tree_density < 0, tree_scale <= 0, tree_mode outside 0 .. 3, force_tree_class outside -1 .. 3 (TREE_CLASS_DETAILED has no small tree type:
 * get_tree_type_from_height asserts), instanced with an empty or oversized (> 2^30) instance range (select_inst asserts start < end), instanced with
 * force_tree_class 2 (maybe_add_tree asserts pine or palm). */
typedef struct terra_tree_params {
	float sm_tree_density;       /* config "sm_tree_density", 1 */
	float tree_scale;            /* config "tree_scale" (src/mesh_gen.cpp:37), 1 */
	float tree_density_thresh;   /* config "tree_density_thresh", 0.55 */
	float tree_type_rand_zone;   /* config "tree_type_rand_zone", 0 */
	int32_t tree_mode;           /* 0 .. 3; bit 2 = small trees (small_trees_enabled), 3 = palms too; 1 */
	int32_t force_tree_class;    /* -1 = by height, else TREE_CLASS_{NONE 0, PINE 1, DECID 2, PALM 3} (src/tree_3dw.h:20) */
	int32_t only_pine_palm_trees;
	int32_t rand_gen_index;
	int32_t instanced;           /* what enable_instanced_pine_trees() returned (src/tiled_mesh.cpp:154-159) */
	uint32_t num_pine_insts;     /* num_insts_per_type[T_PINE] = [0, num_pine_insts) (shared by T_SH_PINE), [T_PALM] = [num_pine_insts, num_pine_insts + num_palm_insts) */
	uint32_t num_palm_insts;     /* (create_pine_tree_instances, src/sm_tree.cpp:342-364) */
} terra_tree_params;
int  terra_set_tree_params(terra_ctx *ctx, const terra_tree_params *params);
int  terra_get_tree_params(terra_ctx *ctx, terra_tree_params *out);
/* height_histogram (src/mesh_gen.cpp:467-480), what get_median_height (:487-491) reads: terra_init_scene keeps the 1024 sorted values of its own estimate grid
 * (every fourth value in both directions); an engine that owns its globals (terra_set_state) passes its vector, of any length (the reference never clears it: two
 * estimates leave 2048 values).  Every terra_init_scene REPLACES the values with those of its own estimate (none when zmax == zmin: the reference returns before
 * the grid then) instead of appending to them: an engine that mirrors a vector grown over several estimates calls the setter after terra_init_scene.
 * count == 0 is the empty vector: get_median_height then returns its argument.  get: *count = the length; up to `capacity` values
 * are written when h_vals is not NULL. */
int  terra_set_height_histogram(terra_ctx *ctx, const float *h_vals, uint32_t count);
int  terra_get_height_histogram(terra_ctx *ctx, float *h_vals, uint32_t capacity, uint32_t *count);
/* terra_tiles_place_trees: small_tree_group::gen_trees (src/sm_tree.cpp:407-474) from :439 on for every tile, as tile_t::init_pine_tree_draw calls it, bit for bit:
 * the running xv / yv sums (:455-470), the bilinear cur_density over density[4] = params[..].veg (generated internally, as for terra_tiles_create_weights),
 * get_ntrees_for_mesh_xy (:366-376), density_gen.eval_index, the get_median_height test (:466), and maybe_add_tree (:378-404) with zpos from the glaciated
 * height_gen.eval_index when approx_zval (:446) and from get_exact_zval otherwise, get_tree_type_from_height (:527-566) and select_inst or rand_tree_height /
 * rand_tree_width.  xoff2 / yoff2: the loop runs over the local indices x1 - xoff2 .. (ptree_off.set_from_xyoff2()), seeds and field origins use j + xoff2,
 * get_xval(j) the local j.
 * skip (optional): [n] bytes, non-zero = can_have_trees() is false.  stats (optional): a tile failing can_have_pine_palm_trees_in_zrange(mzmin, mzmax) (:568-578,
 * no tree placer) gets no trees.  trees: [n][capacity] records; counts: [n].  The trees of a tile appear in the reference's loop order (rows, then columns); a tile
 * with more than `capacity` trees gets the first `capacity` and counts[t] still reports all of them.  Records past counts[t] are not written.
 * With the engine stay check_valid_scenery_pos and point_inside_voxel_terrain (:399, :402; they draw no random numbers, so filtering the records afterwards is
 * identical), the tree placer block (:412-438), the small_tree constructor (for a tree that is not instanced, from the generator state in the record),
 * and postproc_trees.  Deciduous trees have a call of their own: terra_tiles_place_decid_trees, below.
 * Zero trees everywhere (:439-440): vegetation == 0, sm_tree_density == 0, bit 2 of tree_mode clear; per tile: all four density corners 0.
 * TERRA_ERR_ARG when some cell could have XY_MULT_SIZE < 2*ntrees: the reference then does not re-seed its generator per cell (:370), the sequence runs serially
 * through the tile and trees_this_xy can exceed 1.  The test, on the host: ntrees = int(min(1, cur_density*ntrees_mult)*40000) with cur_density = 1.001, which
 * covers every cell (corners are CLIP_TO_01 values, a running sum stays within [0, 1 + 1e-4], six float roundings).  At the defaults ntrees <= 312 against
 * XY_MULT_SIZE = 16384; S = 16 is refused (624 > 256).  skip_val = int(1/sqrt(sm_tree_density*tree_scale)) may exceed S: cell (0, 0) alone is visited then and
 * the position offsets still scale with skip_val; a quotient that does not fit an int (undefined in the reference) is TERRA_ERR_ARG.
 * Also TERRA_ERR_ARG: vegetation*sm_tree_density < 0, an unsupported S, a NULL required pointer (tile_xy,
 * counts when n > 0; trees when capacity > 0), a misaligned pointer.
 * TERRA_ERR_STATE before terra_init_scene, and while a heightmap texture is set (check_hmap_normal and the texture heights of get_exact_zval are not part of this
 * call).  n == 0 does nothing once the scene and the tile size have passed: the settings are not looked at.  The device form only enqueues. */
typedef struct terra_tree_place {
	float pos[3];            /* xval, yval, zpos */
	int32_t type;            /* T_PINE 0, T_DECID 1 .. 3 (force_tree_class 2 only), T_PALM 4, T_SH_PINE 5 (src/small_tree.h:9) */
	int32_t inst;            /* select_inst's result, -1 when not instanced */
	float height, width;     /* tsize*rand_tree_height, height*rand_tree_width; 0 when instanced */
	int32_t rseed1, rseed2;  /* the generator where the reference constructs the small_tree */
	uint16_t cx, cy;         /* the cell inside the tile */
} terra_tree_place;          /* 40 bytes */
int  terra_tiles_place_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                 uint32_t capacity, terra_tree_place *d_trees, uint32_t *d_counts);
int  terra_tiles_place_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                             uint32_t capacity, terra_tree_place *h_trees, uint32_t *h_counts);
/* terra_tiles_place_trees_brush: gen_trees_tt_within_radius (:477-502) as tile_t::add_new_trees (src/tiled_mesh.cpp:3805-3811) calls it, xoff2 / yoff2 = -toff.dxoff /
 * -toff.dyoff: the same cell with ntrees_mult without vegetation, no density field, one discarded rand_float, zpos always from get_exact_zval, and the fabs /
 * dist_xy_less_than test of the cell's centre against pos (x and y are read) and radius; is_square = (brush_shape == BSHAPE_CONST_SQ).  The caller keeps the
 * mesh_sphere_intersect culls and the removal loop (:3822-3838); terra_tiles_edit_trees, below, runs both and this call on resident records.  skip / stats: can_have_pine_palm_trees() as above.  Zero trees: sm_tree_density == 0 or bit 2
 * of tree_mode clear.  Refusals as above, the bound on ntrees taken at ntrees_mult itself. */
int  terra_tiles_place_trees_brush_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                       const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_tree_place *d_trees, uint32_t *d_counts);
int  terra_tiles_place_trees_brush(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                   const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_tree_place *h_trees, uint32_t *h_counts);

/* ---- deciduous tree placement of a tile batch (every supported tile size S): tree_cont_t::gen_trees_tt_within_radius (src/Tree.cpp:2209-2305) from :2240 on, the
 * generating half of tile_t::gen_decid_trees_if_needed (src/tiled_mesh.cpp:1536-1547) and of the decid_trees half of "Add Trees" (tile_t::add_new_trees, :3805-3811,
 * :3837).  With terra_tiles_place_trees both tree containers of a tile now come from the device; the scenery container: terra_tiles_place_scenery, below.
 * terra_decid_params: what this path reads beyond terra_tree_params (tree_scale, tree_density_thresh, tree_type_rand_zone, tree_mode, force_tree_class,
 * only_pine_palm_trees, rand_gen_index), terra_landscape and the scene.  TERRA_ERR_ARG (and nothing changes): num_trees < 0, a tree_slope_thresh or a branch_size
 * that is not finite and > 0. */
typedef struct terra_decid_params {
	int32_t  num_trees;          /* config "num_trees", 0: no generated trees */
	uint32_t num_shared_trees;   /* shared_tree_data.size() (max_unique_trees); 0: tree_id = -1 */
	float    tree_slope_thresh;  /* config "tree_slope_thresh", 5 */
	float    branch_size[5];     /* tree_types[].branch_size (src/Tree.cpp:38), 1 */
} terra_decid_params;
int  terra_set_decid_params(terra_ctx *ctx, const terra_decid_params *params);
int  terra_get_decid_params(terra_ctx *ctx, terra_decid_params *out);
/* terra_tiles_place_decid_trees: gen_deterministic (src/Tree.cpp:2153-2155) for every tile, bit for bit, trees in the reference's loop order (rows, then columns): the
 * loop visits every skip_val = max(1, int(1.0/tree_scale))-th cell; the seeds of :2269-2270 from i + yoff2, j + xoff2 and rand_gen_index (int products that wrap),
 * rand_mix, val = unsigned(rand_seed_mix()) % smod; the cell is dropped when val <= 100, when val % tree_prob != 0 or when (rseed1 & 127)/128.0 >= vegetation_
 * (smod = unsigned(3.321*XY_MULT_SIZE + 1), tree_prob = max(1U, XY_MULT_SIZE/mod_num_trees), mod_num_trees = unsigned(num_trees/sqrt(tree_density_thresh)), an int
 * divided by the double of a float sqrt); pos.xy = get_xval(j) / get_yval(i) + 0.5*DX_VAL*randd(); pos.z = get_exact_zval; the range [water_plane_z + 0.01*zmax_est,
 * 1.8*zmax_est]; at tree_mode 3 get_tree_class_from_height(pos.z, 0) must be TREE_CLASS_DECID; the coverage test density_gen[0].eval_index(j - x1, i - y1) >
 * get_median_height(tree_density_thresh); the type as the arg-max over the five jittered type fields density_gen[1 .. 5] (:2286-2293); the slope test (below);
 * add_new_tree's tree_id (:2163-2166) from the generator as it stands.  vegetation_ = vegetation*get_avg_veg(), the four veg corners generated internally as for
 * terra_tiles_place_trees and averaged as src/tiled_mesh.h:221 does.  xoff2 / yoff2: as for terra_tiles_place_trees (dtree_off.set_from_xyoff2()).
 * skip (optional): [n] bytes, non-zero = can_have_trees() is false.  stats (optional): a tile failing can_have_decid_trees_in_zrange(mzmin, mzmax)
 * (src/sm_tree.cpp:580-587, no tree placer) gets no trees, and a tile whose mesh_dz = max(sub_zmax[k] - sub_zmin[k]), taken from 0 (src/tiled_mesh.cpp:535), is above
 * 1.0 runs the slope test adjust_tree_zval(pos, 0, ttype, 0, cur_tile) (src/Tree.cpp:1471-1480): radius = 2*(60*(0.1*(TREE_SIZE*branch_size[ttype]/tree_scale))), the
 * tile's zvals scanned over get_z_minmax_for_area(pos + (xoff2*DX_VAL, yoff2*DY_VAL), 0.5*radius) (src/tiled_mesh.cpp:548-564: round-down indices against the tile's
 * x1 = tx*S, unsigned max(0, ..) / min(stride, ..), rows and columns inclusive), pos.z lowered to the area's minimum, and the tree dropped unless
 * mzmax - pos.z < tree_slope_thresh*radius.  zvals: [n][S+2][S+2], required with stats; without stats no tile is culled and no slope test runs.
 * get_z_minmax_for_area asserts that its index range is not empty.  It never is: pos lies within half a cell of a cell of its own tile, so the column of
 * pos.x + radius is at least the tile's first (ix2 >= 0 after the + 1) and that of pos.x - radius at most its last (ix1 <= S < stride), and ix1 <= ix2 because
 * rx1 <= rx2 and both indices round the same way; the same holds in y.  (The kernel's loops do not rely on it: an empty range reads nothing.)
 * trees: [n][capacity] records; counts: [n].  A tile with more than `capacity` trees gets the first `capacity` and counts[t] still reports all of them.  Records
 * past counts[t] are not written.
 * With the engine stay check_valid_scenery_pos (:2295; it sees the height before adjust_tree_zval, which is why the record carries both), point_inside_voxel_terrain
 * (:2281), the pre-placed city trees of tree_placer (:2219-2239), the is_created() type override of add_new_tree (:2171), tree::gen_tree (fed from the generator
 * state in the record) and postproc_trees.  None of them draws a random number and cells are independent, so filtering the records afterwards is identical.
 * Zero trees everywhere (:2240): mod_num_trees == 0 (num_trees 0, or fewer than sqrt(tree_density_thresh)), bit 1 of tree_mode clear.
 * TERRA_ERR_ARG: a 1.0/tree_scale that does not fit an int, a num_trees/sqrt(tree_density_thresh) that does not fit an unsigned (undefined in the reference), an
 * unsupported S, a NULL required pointer (tile_xy, counts when n > 0; trees when capacity > 0), a misaligned pointer, stats without zvals.
 * TERRA_ERR_STATE before terra_init_scene, and while a heightmap texture is set (the texture heights of get_exact_zval are not part of this call).  n == 0 does
 * nothing once the scene and the tile size have passed.  The device form only enqueues. */
typedef struct terra_decid_place {
	float pos[3];            /* pos.z after adjust_tree_zval */
	float zval;              /* get_exact_zval(pos.x, pos.y): what check_valid_scenery_pos sees */
	int32_t type;            /* 0 .. 4 (src/tree_leaf.h:8) */
	int32_t tree_id;         /* add_new_tree's, -1 without shared trees */
	int32_t rseed1, rseed2;  /* the generator where the reference calls gen_tree */
	uint16_t cx, cy;         /* the cell inside the tile */
} terra_decid_place;         /* 36 bytes */
int  terra_tiles_place_decid_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                       const float *d_zvals, uint32_t capacity, terra_decid_place *d_trees, uint32_t *d_counts);
int  terra_tiles_place_decid_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                   const float *h_zvals, uint32_t capacity, terra_decid_place *h_trees, uint32_t *h_counts);
/* terra_tiles_place_decid_trees_brush: the same function as tile_t::add_new_trees calls it (xoff2 / yoff2 = -toff.dxoff / -toff.dyoff): vegetation_ = 1, no coverage
 * field, and the fabs / dist_xy_less_than test of the cell's get_xval / get_yval against pos (x and y are read) and radius (:2256-2264).  A radius of 0 or less means
 * the whole tile.  is_square is accepted as the reference accepts it: this function never reads it (a square brush places deciduous trees within the circle).
 * The caller keeps the mesh_sphere_intersect culls and the removal loop (:3822-3838); terra_tiles_edit_trees, below, runs both and this call on resident records. */
int  terra_tiles_place_decid_trees_brush_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                             const float *d_zvals, const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_decid_place *d_trees, uint32_t *d_counts);
int  terra_tiles_place_decid_trees_brush(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                         const float *h_zvals, const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_decid_place *h_trees, uint32_t *h_counts);

/* ---- scenery placement of a tile batch (every supported tile size S): the cell loop of scenery_group::gen (src/scenery.cpp:1263-1353), the generating half of
 * tile_t::update_scenery (src/tiled_mesh.cpp:1568-1578), which fills the third container of a tile -- rocks, plants, logs, stumps and mushrooms.  The reference
 * "assumes trees are generated before scenery"; nothing here reads the trees.
 * terra_scenery_params: what this path reads beyond terra_tree_params (tree_scale, tree_type_rand_zone, tree_mode, force_tree_class, only_pine_palm_trees,
 * rand_gen_index), terra_landscape (vegetation, the biome field) and the scene.  TERRA_ERR_ARG (and nothing changes): use_voxel_rocks < 0. */
typedef struct terra_scenery_params {
	int32_t use_voxel_rocks;     /* config "use_voxel_rocks", 2 (src/3DWorld.cpp:93): 0 never, 1 always, 2 only when the landscape's vegetation is 0 */
} terra_scenery_params;
int  terra_set_scenery_params(terra_ctx *ctx, const terra_scenery_params *params);
int  terra_get_scenery_params(terra_ctx *ctx, terra_scenery_params *out);
/* terra_tiles_place_scenery: scenery_group::gen(x1 - xoff2, y1 - yoff2, .., vegetation*get_avg_veg(), ..) for every tile, bit for bit.  All objects of a tile go into
 * one list in the reference's loop order (rows, then columns); the reference pushes into nine vectors, and a stable split of the list by `kind` reproduces each.
 * Per cell: the seeds of :1276-1277 from i + yoff2, j + xoff2 and rand_gen_index (int products that wrap); val = int(unsigned(rand2_seed_mix()) % smod) with
 * smod = max(200U, unsigned(3.321f*XY_MULT_SIZE/(tree_scale+1))) in float arithmetic; the cell is dropped when val >= 150; rand2_mix(); veg = (rseed1&127)/128.0 <
 * vegetation_, with vegetation_ = vegetation*get_avg_veg() from the four veg corners generated internally as for terra_tiles_place_decid_trees; then the chain of
 * :1284-1351 in the reference's order (rand2()%100 < 35 draws only when veg holds, and the later branches see the advanced generator); voxel rocks when
 * use_voxel_rocks == 1 or (use_voxel_rocks >= 2 and the landscape's vegetation == 0.0: the global, not vegetation_).  The minimum heights of :1267-1270 are formed in
 * double.  Every create() runs with use_xy = 1: gen_spos (:94-99: get_xval / get_yval of the local index + 0.5*DX_VAL*rand2d(), then get_exact_zval) and the class's
 * own statements with the operand types the source gives them (the double literals, pointT's operator/= and mag(), signed_rand_vector_norm whose first draw is z and
 * third x, the left operand of rand_uniform2(..)*rand_float2() drawing first).  get_min_water_plane_z() is get_water_z_height() - ocean_wave_height of the scene; a
 * log's `zmin` is the scene's.  Logs and stumps take calc_type() = get_tree_type_from_height(pos.z, rgen, 1) and are dropped when it is negative.
 * The record stops where the object's random draws for its placement end: leafy_plant before gen_leaves(), rock_shape3d before gen_rock (the record carries rs_rock and
 * the type bit; gen_rock re-seeds itself from rs_rock), surface_rock before the surface cache, voxel_rock without gen_model_ix.  rseed1 / rseed2 are global_rand_gen
 * at that point, which is what gen_leaves() and the surface cache continue from.
 * xoff2 / yoff2: as for terra_tiles_place_trees (scenery_off.set_from_xyoff2()): the loop runs over the local indices, the seeds use i + yoff2 and j + xoff2,
 * get_xval takes the local index.  skip (optional): [n] bytes, non-zero = update_scenery does not generate (scenery_enabled, is_distant, dist_scale, is_visible).
 * objs: [n][capacity] records; counts: [n].  A tile with more than `capacity` objects gets the first `capacity` and counts[t] still reports all of them.  Records
 * past counts[t] are not written.  kind_counts (optional): [n][TERRA_SCENERY_KINDS], every object of the tile per kind, those beyond `capacity` included (what the
 * engine reserve()s).
 * With the engine stay check_valid_scenery_pos (on pos and radius of the record; for a rock_shape after its gen_rock), the city ponds (:1354-1375), post_gen_setup
 * (geometry, VBOs, cache_closest_tree_type) and leafy_plants.size() as plant_ix.  None of them draws from a cell's generator before the next cell re-seeds it, so
 * filtering the records afterwards is identical.
 * TERRA_ERR_ARG: a 3.321*XY_MULT_SIZE/(tree_scale+1) that does not fit an unsigned, an unsupported S, a NULL required pointer (tile_xy, counts when n > 0; objs when
 * capacity > 0), a misaligned pointer.  TERRA_ERR_STATE before terra_init_scene, and while a heightmap texture is set (the texture heights of get_exact_zval are not
 * part of this call).  n == 0 does nothing once the scene and the tile size have passed.  The device form only enqueues. */
enum {TERRA_SCENERY_LEAFY_PLANT, TERRA_SCENERY_PLANT, TERRA_SCENERY_ROCK_SHAPE, TERRA_SCENERY_SURFACE_ROCK, TERRA_SCENERY_VOXEL_ROCK,
      TERRA_SCENERY_ROCK, TERRA_SCENERY_LOG, TERRA_SCENERY_STUMP, TERRA_SCENERY_MUSHROOM, TERRA_SCENERY_KINDS};
typedef struct terra_scenery_place {
	float pos[3];            /* the object's pos as its create() leaves it (rock_shape: before the += 0.1*radius of :156, radius comes from gen_rock) */
	float radius;            /* 0 for rock_shape */
	int32_t kind;            /* TERRA_SCENERY_* */
	int32_t iv[2];           /* plant / leafy plant: {type, 0}; log / stump: {calc_type()'s type, 0}; rock_shape: {rs_rock, gen_rock's type bit}; voxel_rock: {rseed, 0}; else 0 */
	float p[8];              /* plant {height}; mushroom {height}; stump {radius2, height}; surface_rock {dir xyz}; rock {scale xyz, size, dir xyz, angle};
	                            log {radius2, length, dir xyz, pt2 xyz}; unused entries 0 */
	int32_t rseed1, rseed2;  /* global_rand_gen where the device stops */
	uint16_t cx, cy;         /* the cell inside the tile */
} terra_scenery_place;       /* 72 bytes */
int  terra_tiles_place_scenery_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, uint32_t capacity,
                                   terra_scenery_place *d_objs, uint32_t *d_counts, uint32_t *d_kind_counts);
int  terra_tiles_place_scenery(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, uint32_t capacity,
                               terra_scenery_place *h_objs, uint32_t *h_counts, uint32_t *h_kind_counts);

/* ---- flowers of a tile batch (every supported tile size S): flower_tile_manager_t::gen_flowers (src/grass.cpp:859-888) with flower_manager_t::add_flowers
 * (:813-838), as tile_t::draw_flowers (src/tiled_mesh.cpp:1666-1677) calls it -- the fourth generated container of a tile -- and its upkeep after a grass
 * stroke, update_subrange / clear_within (src/grass.cpp:890-926) as tile_t::add_or_remove_grass_at (src/tiled_mesh.cpp:3930-3937) calls them.  The input is
 * "mesh weight + tree dirt": the weights terra_tiles_create_weights followed by terra_tiles_tree_weights leaves.  Only tsize_bitshift == 0: a city tile with a
 * finer weight texture stays with the caller, as for the grass brush.
 * terra_flower_params: flower_density (config "flower_density", 0: no flowers), grass_length / grass_width (config "grass_size", 0.02 / 0.002), flower_color
 * (config "flower_color" sets alpha 1; alpha > 0 = every flower has this colour), no_grass (no_grass()).  TERRA_ERR_ARG (and nothing changes): a density,
 * length or width that is negative or not finite; a flower_density above 1024 (a tile's count is 32 bits).
 * Generation, bit for bit.  The generator is seeded ONCE per tile with (tile x1 + 123, tile y1 + 456) -- set_state(x1 + xoff2 + 123, ..) with the caller's
 * x1 - xoff2: the offsets cancel -- and runs through all cells, rows then columns.  The two density fields are generated internally: build_arrays(tile x1, tile y1,
 * fds*DX_VAL*DX_VAL, fds*DY_VAL*DY_VAL, S, S, 0, force_sine_mode=1) for fds = 500 and 650, read with eval_index(x, y, 50).  Per cell: the weight is byte 2 (grass)
 * of texel (x, y); grass_den = weight/255.0 as a float; below 0.5 (weight 0 .. 127) no flowers; num_per_bin = unsigned(flower_density*grass_den + 0.5).  Per
 * candidate: dval + 0.2*zmax_est*signed_rand_float() > get_median_height(0.5) in double rejects it after that one draw (the histogram is
 * terra_set_height_histogram's; empty: 0.5); an accepted one draws rand_uniform(0.85, 1.0) for the height, the position's two rand_float() -- y's first: g++
 * evaluates the constructor's arguments right to left --, signed_rand_vector(0.2)'s three (z's first), rand_uniform(1.5, 2.5) for the radius and, unless
 * flower_color.alpha > 0, signed_rand_float() for the colour.  pos is tile-local (dx = dy = 0, gen_zval = 0: pos.z = height).
 * The colour index.  The source reads colors[int(0.5*NUM_COLORS*color_val)%NUM_COLORS] with `unsigned const NUM_COLORS(3)`: the usual arithmetic conversions turn
 * the int into an unsigned BEFORE the remainder, so the index is unsigned(int(1.5*color_val)) % 3u -- 0 .. 2 for every color_val, defined behaviour -- and that
 * is the colour of the record.  For a negative int this is NOT the signed remainder plus 3 (-1 -> 4294967295 % 3 = 0, -2 -> 2, -3 -> 1, -4 -> 0).  About four
 * flowers in ten have a negative int (the colour field is a zero-mean sine sum); aux reports the signed remainder so that a caller or a test can tell them apart.
 * weights: [n][S+1][S+1][4] bytes.  flowers: [n][capacity] records of terra_flower, whose layout is flower_t's (src/grass.h:80-88): an engine copies a tile's
 * records straight into its vector.  aux (optional): [n][capacity] words, bits 0-9 the cell's x, 10-19 its y, 20-22 the colour field: 2 + (int(1.5*color_val) % 3
 * as a signed remainder, -2 .. 2), or 7 under a fixed flower_color.  counts: [n].  The reference's order is kept; only the first `capacity` records of a tile are
 * written and counts[t] still reports all; records past counts[t] are not written.  skip (optional): [n] bytes, non-zero = the tile is not generated (counts[t] = 0).
 * skip_generate(): with flower_density == 0 or no_grass every count is 0 and the weights are not touched (they may be NULL).
 * With the engine stay `generated`, check_vbo, create_verts_range, the drawing and scale_flowers.
 * TERRA_ERR_ARG: an unsupported S, a NULL required pointer (tile_xy, counts, weights when n > 0; flowers when capacity > 0), a misaligned pointer.
 * TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the scene and the tile size have passed.  The device form only enqueues. */
typedef struct terra_flower_params {
	float flower_density;    /* 0 */
	float grass_length;      /* 0.02 */
	float grass_width;       /* 0.002 */
	float flower_color[4];   /* RGBA, alpha 0: the three colours of add_flowers */
	int32_t no_grass;        /* 0 */
} terra_flower_params;
typedef struct terra_flower {
	float pos[3];
	float normal[3];
	float radius, height;
	float color[4];
} terra_flower;              /* 48 bytes, flower_t */
int  terra_set_flower_params(terra_ctx *ctx, const terra_flower_params *params);
int  terra_get_flower_params(terra_ctx *ctx, terra_flower_params *out);
int  terra_tiles_place_flowers_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const uint8_t *d_skip, const uint8_t *d_weights, uint32_t capacity,
                                   terra_flower *d_flowers, uint32_t *d_aux, uint32_t *d_counts);
int  terra_tiles_place_flowers(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const uint8_t *h_skip, const uint8_t *h_weights, uint32_t capacity,
                               terra_flower *h_flowers, uint32_t *h_aux, uint32_t *h_counts);
/* terra_tiles_edit_flowers: the flowers' half of a grass stroke, in place on the records (and aux, where given) of a batch.  brush, updated and ranges are what
 * terra_tiles_edit_grass[_dev] took and left; generated (optional, [n] bytes; NULL = all) is the engine's flag.  Only tiles with updated[t] && generated[t] are
 * touched.  A tile's container is its first min(counts[t], capacity) records.
 * Adding: update_subrange(.., xl, yl, xh, yh); nothing when xh <= xl or yh <= yl.  The remove_element loop (swap with the back, pop, test the index again) runs
 * over the cell test int(pos.x*DX_VAL_INV), int(pos.y*DY_VAL_INV) inside the range, which truncates; the generator is re-seeded with (tile x1 + xl + 123,
 * tile y1 + yl + 456); add_flowers runs over the rectangle's cells (no minimum over texels); the new records go behind the survivors while they fit, counts[t]
 * reports all.  Removing: clear_within(pos - flower_xlate, radius, shape == TERRA_BSHAPE_CONST_SQ) with the same loop; flower_xlate = (get_xval(x1 + dxoff),
 * get_yval(y1 + dyoff)), dxoff / dyoff = xoff - xoff2 / yoff - yoff2 as for the grass brush.  ranges and weights are read only when adding.
 * status: [n] bytes.  0: untouched.  1: edited (the loops ran, whether or not a record changed).  2: left unchanged because the range reaches texel row or column
 * S (xh > S or yh > S): update_subrange would call eval_index(S, ..) there, which the reference asserts against (the density fields have S x S cells).
 * terra_tiles_edit_grass never leaves such a range -- it clamps xh and yh to S as src/tiled_mesh.cpp:3900-3901 does, so a stroke at a tile's far edge updates
 * columns up to S - 1 -- the value guards ranges that come from elsewhere.
 * TERRA_ERR_ARG: a bad brush shape, an unsupported S, a NULL required pointer (brush; tile_xy, updated, counts, status when n > 0; ranges and weights when adding;
 * flowers when capacity > 0), a misaligned pointer.  TERRA_ERR_STATE before terra_init_scene.  The device form only enqueues. */
int  terra_tiles_edit_flowers_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *d_generated,
                                  const terra_grass_brush *brush, const uint8_t *d_updated, const uint32_t *d_ranges, const uint8_t *d_weights, uint32_t capacity,
                                  terra_flower *d_flowers, uint32_t *d_aux, uint32_t *d_counts, uint8_t *d_status);
int  terra_tiles_edit_flowers(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *h_generated,
                              const terra_grass_brush *brush, const uint8_t *h_updated, const uint32_t *h_ranges, const uint8_t *h_weights, uint32_t capacity,
                              terra_flower *h_flowers, uint32_t *h_aux, uint32_t *h_counts, uint8_t *h_status);

/* ---- the grass draw lists of a tile batch for a camera (every supported tile size S that is a multiple of 4): tile_t::draw_grass (src/tiled_mesh.cpp:1607-1664)
 * without its GL calls, behind the per-tile filters of its caller tile_draw_t::draw_grass (:3420-3425) -- the library's first view-dependent call.  It answers for
 * every tile of a batch which of its grass blocks are drawn from this camera, at what LOD, and in what order the instanced draws take them, bit for bit.
 * terra_view: the members of pos_dir_up (src/3DWorld.h:705-711) that the view tests read.  An engine copies camera_pdu's pos, dir, upv_ (the orthogonalized up
 * vector, NOT upv), cp, sterm, x_sterm, near_, far_ and valid into it; valid == 0 makes every frustum test pass, as in the reference.
 * terra_make_view: pos_dir_up's constructor (src/visibility.cpp:67-92) with the C library's tanf / sinf / atanf, for callers without a camera_pdu.  angle (radians,
 * half the vertical field of view) and aspect are the caller's: the window_width / PERSP_ANGLE defaults that the constructor takes for 0 stay with the engine.
 * (They are not the same numbers: for its default angle the reference's build folds tanf at compile time, correctly rounded, and camera_pdu's x_sterm and
 * behind_sphere_mult differ in the last place from what the C library's tanf gives for the same angle passed explicitly.  Copy camera_pdu's members.)
 * TERRA_ERR_ARG where the constructor asserts (near < 0, far <= near, a zero dir, tanf(angle) <= 0 with aspect != 1) and for a NULL pointer; *out is untouched then.
 * terra_grass_view_params: tt_grass_scale_factor (1).  TERRA_ERR_ARG for a value that is not finite and > 0 (src/grass.cpp:1126 resets such a value to 1; here it is
 * refused and nothing changes).  grass_length is terra_flower_params.grass_length, num_rnd_grass_blocks the landscape's.
 * Per tile: skipped (skip[t] != 0: the tile is not in the engine's to_draw), or get_min_dist_to_pt(camera) > get_grass_thresh_pad() (:1612), or every block's
 * ix == 0 (the reference's empty grass_blocks: !has_grass(), :1609 and :3422) -> nothing is drawn: counts[t] = 0, its group counts are 0, pass[t] = 255.  Otherwise
 * pass[t] is the wpass of :3424 in which the tile is drawn -- 1 where get_dist_to_camera_in_tiles(0) > 0.5*tt_grass_scale_factor (no wind), else 0 (wind) -- and every
 * block runs :1628-1651: empty; closest_pt_dist_sq(camera) against bg_thresh_sq; cube_visible unless the tile's mesh box is completely visible; for blocks nearer
 * than 0.56*bg_thresh_sq the back-face test over its 25 texels' zvals and slopes against the camera raised by 2*grass_length; the LOD
 * min(5, unsigned(lod_scale*sqrt(dist_sq))); bix = ix - 1.  Where the reference asserts (bix >= num_rnd_grass_blocks, :1650) the block is skipped.
 * Inputs.  tile_xy is on the host.  dxoff / dyoff = xoff - xoff2 / yoff - yoff2 as for the line queries.  zvals: [n][S+2][S+2].  stats: [n], of which mzmin, mzmax
 * and radius are read (the engine may have enlarged radius).  grass_blocks: [n][dim][dim] with dim = 1 + (S-1)/4, the layout terra_tiles_create_weights writes at
 * S = 128 and terra_tiles_edit_grass keeps.  skip (optional): [n] bytes.  view is a host struct read at the call, like the brushes.
 * Outputs.  insts: [n][capacity] pairs of floats {x*dx_step, y*dy_step}, the layout of the reference's vector2d, in the reference's DRAW ORDER: LOD 0 .. 5, within a
 * LOD block index 0 .. num_rnd_grass_blocks - 1, within such a group the (y, x) scan order of :1626-1627.  An engine uploads a tile's row as its instance buffer
 * and walks group_counts: [n][6][num_rnd_grass_blocks], the v.size() of :1659.  counts: [n] totals.  Only the first `capacity` instances of a tile are written;
 * counts and group_counts still report all; records past the count are not written.  aux (optional): [n][capacity] words, bits 0-15 the block's y*dim + x, bits
 * 16-18 the LOD, bits 19-31 bix.  pass (optional): [n] bytes, see above.
 * With the engine stay the shaders, the texture binds, render_block and the using_shadow_maps() split of :3423.
 * TERRA_ERR_ARG: an unsupported S; an S that is not a multiple of 4 (dim = 1 + (S-1)/4 rounds up, and the back-face loop of :1638-1641 runs to texel (y+1)*4 of
 * the last block row, whose slopes would read past the (S+2)^2 zvals: the reference reads out of bounds there); a view with a non-finite member;
 * num_rnd_grass_blocks equal to 0 or above 4096; a NULL required pointer (view; tile_xy, zvals, stats, grass_blocks, counts, group_counts when n > 0; insts when capacity > 0); a
 * misaligned pointer (4 bytes).  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the scene, the tile size and the view have passed.  The device
 * form only enqueues; the host form refuses bad arguments before it stages anything. */
typedef struct terra_view {
	float pos[3], dir[3], upv[3] /* upv_ */, cp[3];
	float sterm, x_sterm, near_, far_;
	int32_t valid;
} terra_view;
typedef struct terra_grass_view_params {
	float tt_grass_scale_factor; /* 1 */
} terra_grass_view_params;
int  terra_make_view(const float pos[3], const float dir[3], const float up[3], float angle, float aspect, float near_clip, float far_clip, terra_view *out);
int  terra_set_grass_view_params(terra_ctx *ctx, const terra_grass_view_params *params);
int  terra_get_grass_view_params(terra_ctx *ctx, terra_grass_view_params *out);
int  terra_tiles_grass_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *d_zvals, const terra_tile_stats *d_stats,
                                const terra_grass_block *d_grass_blocks, const uint8_t *d_skip, const terra_view *view, uint32_t capacity, float *d_insts, uint32_t *d_aux,
                                uint32_t *d_group_counts, uint32_t *d_counts, uint8_t *d_pass);
int  terra_tiles_grass_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *h_zvals, const terra_tile_stats *h_stats,
                            const terra_grass_block *h_grass_blocks, const uint8_t *h_skip, const terra_view *view, uint32_t capacity, float *h_insts, uint32_t *h_aux,
                            uint32_t *h_group_counts, uint32_t *h_counts, uint8_t *h_pass);

/* ---- the terrain draw list of a tile batch for a camera (every supported tile size S): the head of tile_draw_t::draw (src/tiled_mesh.cpp:2844-2915) up to and
 * including its sort, tile_t::get_lod_level (:1910-1932) and the crack look-ups of tile_t::draw (:2059-2074) -- the per-frame decision about the tiles themselves:
 * which are drawn, in what order, at which mesh LOD, with which crack strips towards each neighbour, bit for bit.  Its status is also what an engine turns into the
 * skip bytes of terra_tiles_grass_view.  The tile size enters only through `size` (:1926), the boxes and radius.
 * terra_terrain_view_args: a host struct read at the call, like the brushes.  behind_sphere_mult: pos_dir_up's member that terra_view lacks;
 * terra_view_behind_sphere_mult restates src/visibility.cpp:83 with the C library's tanf and the statement's own float / double mix (angle and aspect as for
 * terra_make_view; TERRA_ERR_ARG for a NULL out).  water_enabled: is_water_enabled(); water_plane_z is the scene's.  occluder_zmin: the global zmin that
 * occluder_cubes_t reads (:2840) -- an engine passes its zmin (terra_get_state's zmin for a generated scene).  check_occlusion: the condition of :2857,
 * (display_mode & 0x08) && (display_mode & 0x01) && check_tt_mesh_occlusion.  reflection_pass: 0, 2 or 3; pass 1 needs can_have_reflection (:2869): it is
 * terra_tiles_reflection_view's, and is refused here.
 * Inputs.  tile_xy is on the host; a tile may appear once (the neighbour look-up is the [n][9] table of terra_tiles_tree_ao_shadows).  dxoff / dyoff = xoff - xoff2 /
 * yoff - yoff2 as for the grass view.  Per-tile arrays: stats [n] (sub_zmin, sub_zmax, mzmin, mzmax and radius are read); min_normal_z [n] (optional; NULL = 0,
 * "normals not yet calculated"); trmax [n] (optional; NULL = 0; terra_tiles_tree_ao_shadows writes it); tile_zmax [n] (optional; the engine's get_tile_zmax(),
 * src/tiled_mesh.h:207; NULL = mzmax); flags [n] bytes (optional): bit 0 = the tile is absent for this frame -- not drawn, no occluder, no neighbour: where an
 * engine puts its building-occluder and city filters --, bit 1 = has_tunnel || has_city (never an occluder), bit 2 = shadow_maps_allocated() (the dist /= 2 of
 * :1916); occl_state [n] bytes (optional, in and out): last_occluded as of this frame, 0 = nothing recorded this frame, 1 = was_last_occluded(), 2 =
 * was_last_unoccluded(); the call writes 1 or 2 wherever the reference calls set_last_occluded (:2906).
 * Per tile that is present: get_center(), get_rel_dist_to_camera() (xy), get_bcube() (trmax, tile_zmax + BCUBE_ZTOLER, the water plane), is_visible()
 * (sphere_and_cube_visible_test with get_bsphere_radius_inc_water()), use_as_occluder() (:3801) under check_occlusion, the filters of :2867-2868, and
 * get_lod_level(reflection_pass) -- for every present tile, since neighbours' LODs feed the crack index.  A candidate whose occl_state is not 2 runs, when the batch
 * has any occluder, the test of :2872-2908: the occluders' boxes are get_mesh_bcube() and the 16 get_mesh_sub_bcube columns, each zeroed where cube_visible fails and
 * else turned into the column from occluder_zmin up to sub_zmin; check_line_clip is get_line_clip (src/Math3d.cpp:1037-1052).  The loop's early exits only shortcut
 * booleans, so the result does not depend on the order of the occluders.
 * Outputs.  status [n] bytes, low bits: 0 absent, 1 beyond DRAW_DIST_TILES, 2 not visible, 3 occluded earlier this frame (occl_state was 1), 4 occluded now, 5 drawn;
 * bit 7 is set where the tile served as an occluder.  dist [n] floats, get_rel_dist_to_camera() (0 for an absent tile).  lod [n] bytes (0 for an absent tile).
 * crack [n][4] bytes indexed 2*dim + dir: crack_ibuf_t::get_index(dim, dir, lod, adj_lod) (:2020-2023), or 255 where there is no present neighbour in the batch or
 * the tile is not drawn.  draw_order [n] words: its first counts[0] entries are the batch indices of to_draw after the sort of :2915, front to back.  occluded [n]
 * words: its first counts[1] entries are occluded_tiles, in batch order.  counts [2].  Entries past the counts are not written.  not_drawn [n] bytes (optional): 1
 * where the status is not 5, else 0 -- the skip bytes of terra_tiles_grass_view, so that a frame's two view calls chain on the device.
 * One deviation: the reference sorts pair<float, tile_t *>, so equal distances fall back on pointer values; here equal distances order by batch index (a camera
 * over a tile centre makes such ties common).
 * With the engine stay the shaders, the binds, inside_city == 2, the texture-ready test and the building occluders (:2855, :2870).  Reflection pass 1 with
 * can_have_reflection is terra_tiles_reflection_view, the water quads and the water caps are terra_tiles_water_view (below).
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or of the args; reflection_pass 1, negative or above 3; an unsupported S; a NULL required
 * pointer (view, args; tile_xy, stats and every output when n > 0); a misaligned pointer (4 bytes: stats, min_normal_z, trmax, tile_zmax, dist, draw_order,
 * occluded, counts); a tile that appears twice.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.  The device form only
 * enqueues; tile_xy is a host array in both forms.  Scratch comes from the context's arena. */
typedef struct terra_terrain_view_args {
	float behind_sphere_mult;  /* pos_dir_up::behind_sphere_mult */
	float occluder_zmin;       /* the global zmin */
	int32_t water_enabled;     /* is_water_enabled() */
	int32_t check_occlusion;   /* (display_mode & 0x08) && (display_mode & 0x01) && check_tt_mesh_occlusion */
	int32_t reflection_pass;   /* 0, 2 or 3 */
} terra_terrain_view_args;
enum {TERRA_TVIEW_ABSENT = 0, TERRA_TVIEW_TOO_FAR = 1, TERRA_TVIEW_NOT_VISIBLE = 2, TERRA_TVIEW_OCCLUDED_BEFORE = 3, TERRA_TVIEW_OCCLUDED = 4, TERRA_TVIEW_DRAWN = 5,
      TERRA_TVIEW_STATUS_MASK = 7, TERRA_TVIEW_WAS_OCCLUDER = 0x80};
enum {TERRA_TVIEW_FLAG_ABSENT = 1, TERRA_TVIEW_FLAG_NO_OCCLUDER = 2, TERRA_TVIEW_FLAG_SHADOW_MAPS = 4};
int  terra_view_behind_sphere_mult(float angle, float aspect, float *out);
int  terra_tiles_terrain_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_terrain_view_args *args,
                                  const terra_tile_stats *d_stats, const float *d_min_normal_z, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags,
                                  uint8_t *d_occl_state, uint8_t *d_status, float *d_dist, uint8_t *d_lod, uint8_t *d_crack, uint32_t *d_draw_order, uint32_t *d_occluded,
                                  uint32_t *d_counts, uint8_t *d_not_drawn);
int  terra_tiles_terrain_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_terrain_view_args *args,
                              const terra_tile_stats *h_stats, const float *h_min_normal_z, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags,
                              uint8_t *h_occl_state, uint8_t *h_status, float *h_dist, uint8_t *h_lod, uint8_t *h_crack, uint32_t *h_draw_order, uint32_t *h_occluded,
                              uint32_t *h_counts, uint8_t *h_not_drawn);

/* ---- the terrain draw list of reflection pass 1 (every supported tile size S): tile_draw_t::draw(1) (src/tiled_mesh.cpp:2844-2915) -- the loop of
 * terra_tiles_terrain_view with the filter of :2869, tile_draw_t::can_have_reflection and can_have_reflection_recur (:2630-2683), and get_lod_level(1) (:1910-1932:
 * min_normal_z > 0.1 starts at LOD 1, the threshold is 1.8), bit for bit.  It is the pass that every frame with water draws first; the tree, scenery and deciduous
 * views take its not_drawn bytes as they take the main pass's.
 * Inputs: those of terra_tiles_terrain_view with the same meaning; of stats, wx1 .. wy2 (get_water_bcube(), src/tiled_mesh.h:253-256) are read as well.  trmax must
 * not be negative.  terra_reflection_view_args: a terra_terrain_view_args whose reflection_pass is 1 and whose occluder_zmin doubles as the global zmin of :2634, and
 * zmax, the global zmax of :2635.
 * A candidate -- within DRAW_DIST_TILES, visible, not occluded earlier this frame -- is dropped at :2869 unless can_have_reflection holds: 0 with water disabled and
 * for an all_water() tile, 1 for a has_water() tile, else the walk of can_have_reflection_recur from the tile towards the camera through its neighbours in the batch:
 * a neighbour must be present (not absent by flag) and is_visible(), is entered through check_line_clip(camera, corners[dim], its box widened to zmin .. zmax), and
 * ends the walk with 1 where it has water, was not last occluded, its water box is cube_visible and the slope comparison of :2643-2644 holds (the float division may
 * give inf or NaN; the comparison does what IEEE says).  The walk is pure reachability, and vis_ref_call never fires.  last_occluded of a tile met on the walk is
 * what this same loop wrote where the tile came earlier in the batch and was tested, else the incoming occl_state: batch order stands for the loop's map order.
 * Outputs: those of terra_tiles_terrain_view, and: status gains TERRA_TVIEW_NO_REFLECTION = 6 for a tile dropped at :2869 -- it is in neither list, its crack bytes
 * are 255, its not_drawn byte is 1 and its occl_state is left alone (no set_last_occluded).  lod and crack follow get_lod_level(1).  reflect [n] bytes (optional): how
 * :2869 was decided, 0 not asked (the tile left earlier or is absent), 1 all_water or water disabled, 2 the walk found nothing, 3 has_water, 4 the walk found water.
 * Deviations: equal distances order by batch index, as documented above; an absent tile is no neighbour for the walk, as it is none for the cracks.
 * TERRA_ERR_ARG, with nothing written: as for terra_tiles_terrain_view, and a reflection_pass other than 1, a non-finite zmax, a batch whose tile positions span a
 * bounding box more than 2048 wide or of more than 2^18 positions (the walk's visited bits and work list are in LDS).  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.
 * The device form only enqueues; tile_xy is a host array in both forms.  Scratch comes from the context's arena. */
typedef struct terra_reflection_view_args {
	terra_terrain_view_args tv; /* reflection_pass must be 1; occluder_zmin is also the global zmin of :2634 */
	float zmax;                 /* the global zmax of :2635 */
} terra_reflection_view_args;
enum {TERRA_TVIEW_NO_REFLECTION = 6};
enum {TERRA_REFLECT_NOT_ASKED = 0, TERRA_REFLECT_NO_WATER = 1, TERRA_REFLECT_WALK_NOTHING = 2, TERRA_REFLECT_HAS_WATER = 3, TERRA_REFLECT_WALK_FOUND = 4};
int  terra_tiles_reflection_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view,
                                     const terra_reflection_view_args *args, const terra_tile_stats *d_stats, const float *d_min_normal_z, const float *d_trmax,
                                     const float *d_tile_zmax, const uint8_t *d_flags, uint8_t *d_occl_state, uint8_t *d_status, float *d_dist, uint8_t *d_lod, uint8_t *d_crack,
                                     uint32_t *d_draw_order, uint32_t *d_occluded, uint32_t *d_counts, uint8_t *d_not_drawn, uint8_t *d_reflect);
int  terra_tiles_reflection_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view,
                                 const terra_reflection_view_args *args, const terra_tile_stats *h_stats, const float *h_min_normal_z, const float *h_trmax,
                                 const float *h_tile_zmax, const uint8_t *h_flags, uint8_t *h_occl_state, uint8_t *h_status, float *h_dist, uint8_t *h_lod, uint8_t *h_crack,
                                 uint32_t *h_draw_order, uint32_t *h_occluded, uint32_t *h_counts, uint8_t *h_not_drawn, uint8_t *h_reflect);

/* ---- water quads and water caps of a tile batch (every supported tile size S): which tiles tile_draw_t::draw_water (src/tiled_mesh.cpp:3075) draws a quad of the
 * water plane for -- tile_t::is_water_visible (:2131-2133): has_water() && rel_dist_to_camera_xy_lt(DRAW_DIST_TILES) && is_visible(); is_distant is never set --
 * and which of a tile's four edges tile_t::draw_water_cap (:2093-2128) closes the water volume at.
 * Inputs: tile_xy, dxoff / dyoff, view, stats, trmax, tile_zmax and flags (bit 0, absent) as for terra_tiles_terrain_view; terra_water_view_args with
 * behind_sphere_mult and water_enabled (is_water_enabled(): it widens is_visible()'s sphere and gates the caps).  status [n] bytes (optional, on the device in the
 * device form): the status output of a pass-0 terra_tiles_terrain_view on the same batch and camera.
 * Outputs: water_list [n] words, its first counts[0] entries the batch indices of the present tiles with is_water_visible(), in batch order; entries past the count
 * are not written.  cap_mask [n] bytes and counts[1], produced only with status: bit 2*dim + dir of a tile's byte is set where draw_water_cap emits that edge's quad
 * -- unless the neighbour exists (in the batch, not absent) and rel_dist_to_camera_xy_lt(DRAW_DIST_TILES), !has_water() or !is_visible() holds for it (:2108-2112).
 * The byte is 0 unless water is enabled and the status is DRAWN and the tile has_water() (draw_near_water, :2046, :2078), or the status is OCCLUDED (occluded_tiles,
 * :2957-2959; not OCCLUDED_BEFORE).  counts[1] is the number of non-zero bytes.  status and cap_mask are both NULL or both given.
 * With the engine stay ztop (water_plane_z - (draw_distant_water() ? 0.1 : 0.0), one value per call), the quads' vertices and the GL calls.
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or of the args; an unsupported S; a NULL required pointer (view, args; tile_xy, stats,
 * water_list, counts when n > 0); status without cap_mask or the reverse; a misaligned pointer (4 bytes: stats, trmax, tile_zmax, water_list, counts); a tile that
 * appears twice.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.  The device form only enqueues. */
typedef struct terra_water_view_args {
	float behind_sphere_mult;  /* pos_dir_up::behind_sphere_mult */
	int32_t water_enabled;     /* is_water_enabled() */
} terra_water_view_args;
int  terra_tiles_water_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_water_view_args *args,
                                const terra_tile_stats *d_stats, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags, const uint8_t *d_status,
                                uint32_t *d_water_list, uint8_t *d_cap_mask, uint32_t *d_counts);
int  terra_tiles_water_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_water_view_args *args,
                            const terra_tile_stats *h_stats, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags, const uint8_t *h_status,
                            uint32_t *h_water_list, uint8_t *h_cap_mask, uint32_t *h_counts);

/* ---- the shadow-map plan of a tile batch (every supported tile size S; S enters only through the boxes and the radius): which tiles hold a shadow map, at which
 * LOD, and which tiles are drawn into a receiver's shadow map.  All line numbers are src/tiled_mesh.cpp's.
 *
 * terra_tiles_smap_plan[_dev]: one call is one frame's decisions for the camera `view`: tile_t::update_range's shadow-map deletion (:1416 with :1409), the loop of
 * tile_draw_t::pre_draw (:2781-2799, its shadow part: the draw-distance gate of :2784, is_visible, is_smap_bounds_visible, to_update_shadows against cleanup_only),
 * tile_t::setup_shadow_maps (:981-1016) with calc_max_smap_lod (:975-980) and tile_t::get_shadow_bcube (:959-965), the large-map branch of :994-997, and the gate of
 * tile_t::try_bind_shadow_map (:1958-1959).
 * Inputs: tile_xy, dxoff / dyoff, view, stats, trmax, tile_zmax and flags (bit 0, absent) as for terra_tiles_terrain_view; terra_smap_plan_args, read at the call.
 * State, read and written: smap_state [n] bytes, TERRA_SMAP_NONE for smap_data.empty(), else smap_lod_level (0..3).  It is the engine's to keep between frames; a
 * tile's stale smap_lod_level while it holds no shadow maps is not observable in the reference (its uses at :998 and :1000 only guard a clear_shadow_map that is
 * then a no-op, and :1006 overwrites it), so the byte is the whole state.  An absent tile's byte is not touched.
 * Outputs: plan [n] words (TERRA_SMAP_* bits; bits 16-19 lod_level and bits 20-23 lod_level_reduce where :988 was entered; 0 for an absent tile).  A CLEARED bit is
 * set only when the tile held shadow maps at that point, so the engine releases exactly what the reference releases.  RECEIVER: :1015 was reached and the tile holds
 * shadow maps -- the engine calls create_if_needed for it; USABLE: try_bind_shadow_map's gate with the new state.  dist_scale [n]: smap_dist_scale (:986), 0 where it
 * was not formed.  shadow_bcube [n][6] (x1 x2 y1 y2 z1 z2): what :1010-1014 hand to create_if_needed, written for every tile inside the draw distance and for no
 * other.  receivers [n]: its first counts[0] entries are the batch indices with RECEIVER in batch order; entries past the count are not written.  terrain_flags [n]
 * bytes (optional): TERRA_TVIEW_FLAG_SHADOW_MAPS is or'ed into the byte of every present tile whose new state is not NONE -- the flags of the next
 * terra_tiles_terrain_view, taken from the device (it may be the flags array itself).  recomp_order [n] (optional, written when want_recomp): every present tile in
 * the order in which pop_back at :2459 yields the queue of :2445-2448 -- ascending (-p2p_dist(sun_pos, get_center()), tile_xy_pair) consumed from the back;
 * tile_xy_pair::operator< compares y, then x, so the order is total; counts[1] is their number (0 when nothing was asked).  The 12-per-frame budget and
 * clear_shadows stay with the engine.
 *
 * terra_tiles_smap_casters[_dev]: for R independent (receiver tile, light) renders the head of tile_draw_t::draw_shadow_pass (:3025-3043) and the filter of
 * draw_tiles_shadow_pass (:3004-3018) with the inside_city == 2 return of tile_t::draw_shadow_pass (:2083).
 * Inputs: the batch as above (flags bit 3, TERRA_SMAP_TILE_FULLY_IN_CITY); recv [R] batch indices (on the device in the device form: the plan's receivers can feed
 * it; an index that is out of range or names an absent tile gets empty lists, a row of ones in not_drawn and status TERRA_SMAP_CAST_NO_TILE); views [R], the light
 * frustum each render uses (the call applies near_ = 0, :3032, to its copy), bsm [R] their behind_sphere_mult and lpos [R][3] -- host arrays in both forms, read at
 * the call like `view`; decid_counts [n] (needed only with decid_trees_only, :3038); terra_smap_cast_args.
 * Outputs per render r: to_draw [R][n] with counts [R][2]: row r's first counts[r][0] entries are the tiles of :3042 in batch order; terrain [R][n]: the
 * counts[r][1] of them that reach draw_mesh_vbo (:3013 or :3014 holds and the tile is not fully in a city); entries past the counts are not written.  not_drawn
 * [R][n] bytes: 1 for a tile that is not in to_draw.  Row r is the `skip` argument (d_skip / h_skip) of the shadow-pass calls of terra_tiles_tree_view,
 * terra_tiles_scenery_view and terra_tiles_decid_view for that render, the same contract as terra_tiles_terrain_view's not_drawn.  status [R] bytes.  Under
 * decid_trees_only the terrain lists are empty and to_draw follows :3038.
 *
 * terra_make_light_view (host only): get_pt_cube_frustum_pdu (src/shadow_map.cpp:423-457) in its infinite-terrain form (pos *= 10.0) into pos_dir_up's constructor,
 * with the C library's atan2f: the view of a render from lpos and a receiver's shadow_bcube, and its behind_sphere_mult.  near_clip is the engine's NEAR_CLIP.
 * TERRA_ERR_ARG where the reference asserts (bounds not strictly normalized, the light in the box's centre) or the result is not finite.
 *
 * TERRA_ERR_ARG, with nothing written: a non-finite member of a view, the args, lpos, bsm or sun_pos; smap_thresh_scale not > 0; an unsupported S; a NULL required
 * pointer; a pointer other than the byte arrays that is not 4-byte aligned (device forms); R*n beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene.  n == 0 or
 * R == 0 does nothing once the checks have passed.  The device forms only enqueue and read nothing back; tile_xy is a host array in both forms.  The host forms
 * upload the caller's arrays and copy them back, so entries a call does not write keep the caller's bytes. */
#define TERRA_SMAP_NONE 0xFF
enum {TERRA_SMAP_IN_DRAW_DIST = 0x1, TERRA_SMAP_VISIBLE = 0x2, TERRA_SMAP_BOUNDS_VISIBLE = 0x4, TERRA_SMAP_UPDATE = 0x8, TERRA_SMAP_CLEARED_FAR = 0x10,
      TERRA_SMAP_CLEARED_WIREFRAME = 0x20, TERRA_SMAP_CLEARED_LOD_REDUCE = 0x40, TERRA_SMAP_CLEARED_LOD_RAISE = 0x80, TERRA_SMAP_ALLOCATED = 0x100,
      TERRA_SMAP_RECEIVER = 0x200, TERRA_SMAP_USABLE = 0x400, TERRA_SMAP_LOD_SHIFT = 16, TERRA_SMAP_LOD_REDUCE_SHIFT = 20};
enum {TERRA_SMAP_TILE_FULLY_IN_CITY = 8};  /* a bit of the per-tile flags byte, beside TERRA_TVIEW_FLAG_* */
enum {TERRA_SMAP_CAST_NO_TILE = 1};        /* the status byte of a render without a receiver */
typedef struct terra_smap_plan_args {      /* 68 bytes */
	float behind_sphere_mult;              /* pos_dir_up::behind_sphere_mult of `view` */
	int32_t water_enabled;                 /* is_water_enabled() */
	float smap_thresh_scale;               /* > 0 */
	uint32_t shadow_map_sz;                /* 0: shadow_map_enabled() is false */
	int32_t have_buildings;                /* have_buildings(): 1024 instead of 512 in calc_max_smap_lod */
	int32_t draw_model;                    /* non-zero: the wireframe branch of :984 */
	float b_ext[3];                        /* get_buildings_max_extent() */
	float road_len[2];                     /* get_road_max_len() */
	float models_z2; int32_t models_valid; /* calc_and_return_all_models_bcube().z2() and !is_all_zeros() (:1013-1014) */
	float sun_pos[3]; int32_t want_recomp; /* the queue of :2445-2448 */
} terra_smap_plan_args;
typedef struct terra_smap_cast_args {      /* 32 bytes */
	int32_t water_enabled, decid_trees_only;
	int32_t inc_adj_smap;                  /* :3006, the engine's: get_buildings_max_extent() != zero_vector || get_road_max_len().x > 0.0 */
	float b_ext[3], road_len[2];           /* for the receiver's get_shadow_bcube() */
} terra_smap_cast_args;
int  terra_tiles_smap_plan_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_smap_plan_args *args,
                               const terra_tile_stats *d_stats, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags, uint8_t *d_smap_state, uint32_t *d_plan,
                               float *d_dist_scale, float *d_shadow_bcube, uint32_t *d_receivers, uint32_t *d_counts, uint8_t *d_terrain_flags, uint32_t *d_recomp_order);
int  terra_tiles_smap_plan(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_smap_plan_args *args,
                           const terra_tile_stats *h_stats, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags, uint8_t *h_smap_state, uint32_t *h_plan,
                           float *h_dist_scale, float *h_shadow_bcube, uint32_t *h_receivers, uint32_t *h_counts, uint8_t *h_terrain_flags, uint32_t *h_recomp_order);
int  terra_tiles_smap_casters_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, uint32_t R, const uint32_t *d_recv, const terra_view *views,
                                  const float *bsm, const float *lpos, const terra_smap_cast_args *args, const terra_tile_stats *d_stats, const float *d_trmax,
                                  const float *d_tile_zmax, const uint8_t *d_flags, const uint32_t *d_decid_counts, uint32_t *d_to_draw, uint32_t *d_terrain, uint32_t *d_counts,
                                  uint8_t *d_not_drawn, uint8_t *d_status);
int  terra_tiles_smap_casters(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, uint32_t R, const uint32_t *h_recv, const terra_view *views,
                              const float *bsm, const float *lpos, const terra_smap_cast_args *args, const terra_tile_stats *h_stats, const float *h_trmax,
                              const float *h_tile_zmax, const uint8_t *h_flags, const uint32_t *h_decid_counts, uint32_t *h_to_draw, uint32_t *h_terrain, uint32_t *h_counts,
                              uint8_t *h_not_drawn, uint8_t *h_status);
int  terra_make_light_view(const float lpos[3], const float bounds[6], float near_clip, terra_view *out, float *behind_sphere_mult);

/* ---- the clouds of a tile batch (every supported tile size S): tile_cloud_manager_t (src/tiled_mesh.cpp:1689-1827) as tile_draw_t::draw_tile_clouds (:3484-3508)
 * drives it.  No call reads a zval: a tile is its tile_xy, S (x1 = x*S, x2 = x1 + S) and, for the view, its stats.
 *
 * terra_cloud_params: clouds_per_tile (config "clouds_per_tile", 0.5), cloud_height_offset (config "cloud_height_offset", 0) and rgen_seed (1), the seed of
 * gen_gauss_rand_arr's table of 10002 floats (src/gen_object.cpp:363-374) that rand_gaussian reads; the table is built on the host when the seed changes and kept on
 * the device.  zmin, zmax and water_plane_z are the context's own (terra_set_zmax_est, terra_set_water_plane_z).  TERRA_ERR_ARG: clouds_per_tile negative, not finite
 * or above 1000; a cloud_height_offset that is not finite.
 *
 * terra_tiles_update_clouds: the first loop of draw_tile_clouds (:3490) -- for every tile in batch order update_tile_clouds() (:1822-1827): move_by_wind when
 * step->animate, then gen.  (The reference walks an unordered_map; here its order is the caller's batch order.)
 *   state [n] terra_cloud_tile, in/out: everything a tile_cloud_manager_t holds.  An all-zero struct is a freshly constructed manager: the caller zeroes the state
 *     of a tile that enters the batch.  State and records hold no batch index: a tile's state and records may move to another batch slot between calls.
 *   clouds [n][capacity] terra_cloud, in/out: a tile's records are its first state.count entries; what lies behind them means nothing.  The points of volume_part_cloud are
 *     gen_pts(size), a function of size alone: they stay with the engine.
 *   total: optional, one word: the `num` of :3489, the sum of every tile's count right after its own turn (a cloud handed to an earlier tile is not in it).
 * Bit for bit the reference's: gen (once; seed (x1 + 123, y1 + 321); range; choose_num_clouds, which draws nothing when clouds_per_tile == 0; populate_clouds with
 * the draws of gen_new_cloud in g++'s order: pos x, y, z, size z, y, x, the common factor), and move_by_wind in full: the early return, cur_move_dist and the re-draw
 * of num_clouds past 2*get_tile_width(), repopulation of an empty tile on a windward edge of the batch (its clouds are not moved in that call), the per-cloud step,
 * the removal loop (swap with the back, pop, look at the same index again) and the rebuild of bcube.  A cloud that leaves its tile's range is appended to the
 * neighbour (dx, dy) of the batch; it is dropped when the batch has no such tile or that tile is not generated at that moment.  The batch is walked in order: a
 * cloud handed to a later tile is moved again at that tile's turn, one handed to an earlier tile is not; an empty tile repopulates only if no earlier tile has
 * handed it a cloud; a later tile that is not yet generated drops what it is handed and then generates.
 * capacity: a push_back onto a list that holds `capacity` records makes all its draws and stores nothing (generation and immigration alike), sets the sticky bit
 * TERRA_CLD_OVERFLOW in the tile's flags and still unites bcube with the cloud; count never exceeds capacity.  32 holds what generation alone makes at the default
 * density (num_clouds <= clouds_per_tile + 4*max|table|, about clouds_per_tile + 16 at seed 1).
 * TERRA_ERR_STATE before terra_init_scene.  TERRA_ERR_ARG, with nothing written: an unsupported S; a NULL step; NULL tile_xy or state when n > 0; NULL clouds when
 * capacity > 0; capacity == 0 with clouds_per_tile > 0; a non-finite member of the step; a misaligned pointer (8 bytes: state; 4 bytes: clouds, total); a tile that
 * appears twice.  n == 0 writes total = 0 and nothing else.  The device form only enqueues.
 *
 * terra_tiles_cloud_view: the rest of draw_tile_clouds -- get_draw_list for every tile (:1799-1820), the sort of :3493 and the per-instance decision and alpha of
 * tile_cloud_t::draw (:1691-1697).  terra_cloud_view_args: behind_sphere_mult as for the terrain view, xlate = get_tiled_terrain_model_xlate(), max_dist =
 * max(get_draw_tile_dist(), get_inf_terrain_fog_dist()).  stats: mzmin / mzmax are read.
 *   stage [n][capacity] bytes: where a record left get_draw_list: TERRA_CLV_NONE (slot >= count), _VFC, _BELOW_ZMIN, _BELOW_WATER, _BELOW_MESH, _LISTED.
 *   list: up to n*capacity terra_cloud_inst, list_count of them written: tile, slot, dist_sq = -p2p_dist_sq(camera, pos + xlate), alpha (1, or dist/start_dist under
 *     zbot < mzmax + start_dist with dist = zbot - get_exact_zval(pos.x, pos.y, 1)), draw_alpha = alpha*(1 - val*val) with the val of :1696, and drawn = view_dist <
 *     max_dist: an entry that is too distant stays in the list, as it stays in to_draw_clouds, with drawn = 0 and draw_alpha = 0.
 * The exact height is get_exact_zval with no_xyoff = 1 (the scroll offsets taken as 0), evaluated only for the records that reach :1813; as for the placements the
 * call returns TERRA_ERR_STATE while a heightmap texture is set.
 * Order: ascending in dist_sq, that is back to front.  std::sort leaves equal keys in unspecified order; here equal keys go by (tile, slot) ascending.
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or of the args; max_dist not > 0; an unsupported S; a NULL required pointer (view, args;
 * tile_xy, stats, state, stage, list_count when n > 0; clouds, list when n*capacity > 0); a misaligned pointer (8 bytes: state; 4 bytes: stats, clouds, list,
 * list_count).  n == 0 writes list_count = 0 and nothing else.
 * With the engine stay the gates clouds_enabled() && atmosphere >= 0.5 and animate2, the points, get_cloud_color(), tfticks (pos_hash + 0.002*tfticks), the shader and
 * the GL state. */
typedef struct terra_cloud_params {
	float clouds_per_tile;      /* 0.5 */
	float cloud_height_offset;  /* 0 */
	int32_t rgen_seed;          /* 1 */
} terra_cloud_params;
typedef struct terra_cloud_step {
	float wind[3];              /* wind == zero_vector tests all three; z does not move a cloud */
	float fticks;
	int32_t animate;            /* animate2 */
} terra_cloud_step;
typedef struct terra_cloud {
	float pos_hash;
	float pos[3];
	float size[3];
	uint32_t pad;               /* written as 0 */
} terra_cloud;
enum {TERRA_CLD_OVERFLOW = 1};
typedef struct terra_cloud_tile {
	uint32_t generated;
	uint32_t flags;             /* TERRA_CLD_* */
	uint32_t count;             /* size() */
	uint32_t num_clouds;
	float cur_move_dist;
	uint32_t pad;
	int64_t rseed1, rseed2;     /* rgen */
	float bcube[6];             /* x1, x2, y1, y2, z1, z2 */
	float range[6];
} terra_cloud_tile;
typedef struct terra_cloud_view_args {
	float behind_sphere_mult;
	float xlate[3];
	float max_dist;
} terra_cloud_view_args;
enum {TERRA_CLV_NONE = 0, TERRA_CLV_VFC = 1, TERRA_CLV_BELOW_ZMIN = 2, TERRA_CLV_BELOW_WATER = 3, TERRA_CLV_BELOW_MESH = 4, TERRA_CLV_LISTED = 5};
typedef struct terra_cloud_inst {
	uint32_t tile, slot;
	float dist_sq, alpha, draw_alpha;
	uint32_t drawn;
} terra_cloud_inst;
int  terra_set_cloud_params(terra_ctx *ctx, const terra_cloud_params *params);
int  terra_get_cloud_params(terra_ctx *ctx, terra_cloud_params *out);
int  terra_tiles_update_clouds_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_cloud_step *step, terra_cloud_tile *d_state, terra_cloud *d_clouds,
                                   uint32_t capacity, uint32_t *d_total);
int  terra_tiles_update_clouds(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_cloud_step *step, terra_cloud_tile *h_state, terra_cloud *h_clouds,
                               uint32_t capacity, uint32_t *h_total);
int  terra_tiles_cloud_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_view *view, const terra_cloud_view_args *args, const terra_tile_stats *d_stats,
                                const terra_cloud_tile *d_state, const terra_cloud *d_clouds, uint32_t capacity, uint8_t *d_stage, terra_cloud_inst *d_list, uint32_t *d_list_count);
int  terra_tiles_cloud_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_view *view, const terra_cloud_view_args *args, const terra_tile_stats *h_stats,
                            const terra_cloud_tile *h_state, const terra_cloud *h_clouds, uint32_t capacity, uint8_t *h_stage, terra_cloud_inst *h_list, uint32_t *h_list_count);

/* ---- tree AO shadows of a tile batch from the placement records (every supported tile size S): tile_t::apply_tree_ao_shadows (src/tiled_mesh.cpp:740-828), the step
 * between the two placements above and terra_tiles_shadow_texture / terra_tiles_tree_weights.  One call goes from the records as they lie in device memory to the
 * tree maps of the batch, bit for bit; with it zvals -> stats -> both placements -> tree map -> shadow texture / tree weights is one stream of launches.
 * terra_tree_size_params: the globals the radii read beyond terra_tree_params.tree_scale (config keys, src/3DWorld.cpp:1968-1999).  A value that is not finite and
 * > 0 is TERRA_ERR_ARG and changes nothing.
 * terra_set_tree_instances: tree_instances (create_pine_tree_instances, src/sm_tree.cpp:342-364) as far as the radii read it: type, height and width of every
 * instance after its constructor.  The library keeps a copy on the host and one on the device.  get: *count = the length; up to `capacity` values are written when
 * h_insts is not NULL.
 * Radii.  A pine / palm record that is not instanced (inst < 0) is the constructor of src/sm_tree.cpp:717-753 as far as it touches the size -- height *=
 * tree_height_scale*sm_tree_scale, width *= stt[type].width_scale, height *= stt[type].height_scale (stt[], :46-53), none of its random draws -- then
 * get_pine_tree_radius (:911-914), get_radius and get_ao_radius (src/small_tree.h:74-75, branch_xy_scale 1) with the source's operand types.  An instanced record
 * (inst >= 0) is small_tree(p, instance_id) (:705-715): the instance's type (not the record's: T_SH_PINE shares the pine range), its width and height times
 * calc_tree_size() (:326).  Instanced records are applied only while terra_tree_params.instanced is set.  A deciduous record's get_radius() is
 * tdata().sphere_radius, which comes from gen_tree's geometry and stays with the engine: decid_radius [n][decid_capacity] holds one value per record, or
 * decid_radius_by_id [num_radius_by_id] one per shared tree, indexed by the record's tree_id; the per-record form wins when both are given.  get_ao_radius() is
 * 0.5*radius (src/tree_3dw.h:313).  A record the reference could not have made is dropped (no splat, nothing added to trmax): a type outside 0 .. 5, an inst outside
 * the table or while `instanced` is off, a tree_id outside the table, a radius that is negative or not finite.
 * Inputs.  dxoff / dyoff: the map's mesh_off, as for terra_tiles_tree_map.  xoff2 / yoff2: what the placement ran with (ptree_off / dtree_off.set_from_xyoff2()):
 * pt = get_center() + pt_off with pt_off = ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL), an int sum times a float (src/animals.h:26).  pine / pine_counts /
 * pine_capacity and decid / decid_counts / decid_capacity: as the placement calls wrote them; a count above its capacity means the first `capacity` records.  A
 * group is absent when its counts are NULL or its capacity 0.  flags (optional): [n] bytes, bit 0 = can_have_pine_palm_trees() is false, bit 1 =
 * can_have_decid_trees() is false, bit 2 = is_distant.
 * Semantics.  The result is what the reference leaves after apply_tree_ao_shadows() has run on the tiles of the batch in batch order, every tree_map empty at the
 * start; tiles outside the batch do not exist.  get_adj_tile_smap (src/tiled_mesh.h:295-298) returns a neighbour only when its tree_map is not empty, that is when
 * it was processed earlier and is not distant.  trmax(t) = the maximum of 0 and get_radius() over both groups of tile t as passed, whatever the flags say
 * (postproc_trees, small_tree_group::add_tree, tree_cont_t::get_rmax); no_adj_test(t) = trmax(t) < min(DX_VAL, DY_VAL) (:826).  Tile t's ordered list:
 *  1. its own pine trees, then its own deciduous trees, each group gated by t's flag (:800-807); under no_adj_test(t) the bounding-box cull of :793 against
 *     get_mesh_bcube() (src/tiled_mesh.h:238-241) applies;
 *  2. unless no_adj_test(t): for dy = -1 .. 1, dx = -1 .. 1 (:809-815) the trees of the neighbour u that is in the batch, earlier than t and not distant, pine then
 *     deciduous, gated by t's flags (the reference tests `this`, not `tile`), the cull of :793 always on;
 *  3. for every neighbour u later than t, in batch order, not distant and with no_adj_test(u) false: those of u's own trees, gated by u's flags, for which
 *     x_test[dx+1] && y_test[dy+1] of :769-775 holds with xc, yc, rval taken in u's frame and (dx, dy) pointing from u to t (push_tree_ao_shadow, :740-746;
 *     pos2 = pos: all tiles of a batch share mesh_off).
 * The list then runs through the texel loop of terra_tiles_tree_map in list order, with its tie-breaking and its skipped splats.  A distant tile's map is filled
 * with 255, its updated is 0, and it is neither a pull source nor a push target.
 * The same tile set in another batch order gives other maps: step 2 culls by the float box, step 3 by the integer test on rounded texel coordinates, so a tree near
 * a border can reach the neighbour in one order and not in the other, and the order of the list decides the roundings of the texels' products.
 * Outputs.  tree_map: [n][S+1][S+1][2], 2-byte aligned.  updated (optional): [n] bytes.  trmax (optional): [n] floats, what get_bcube needs.  list_counts
 * (optional): [n], the full length of each tile's list; a tile whose list exceeds list_capacity gets its first list_capacity splats applied.
 * TERRA_ERR_ARG: a NULL required pointer (tile_xy, tree_map when n > 0; the records of a group that is present; a radius array for a deciduous group), a misaligned
 * pointer, an unsupported S, a tile that appears twice in tile_xy, `instanced` with an instance table whose length is not num_pine_insts + num_palm_insts,
 * decid_radius_by_id alone with num_radius_by_id != terra_decid_params.num_shared_trees or with 0 shared trees, n*list_capacity or n*(pine_capacity +
 * decid_capacity) beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing.  The device form only enqueues; tile_xy is a host array in both
 * forms (the [n][9] neighbour table is built from it and uploaded).  Scratch comes from the context's arena (terra_release_scratch frees it). */
typedef struct terra_tree_size_params {
	float tree_height_scale;       /* config "tree_height_scale", 1 */
	float sm_tree_scale;           /* config "sm_tree_scale", 1 */
	float pine_tree_radius_scale;  /* config "pine_tree_radius_scale", 1 */
} terra_tree_size_params;
int  terra_set_tree_size_params(terra_ctx *ctx, const terra_tree_size_params *params);
int  terra_get_tree_size_params(terra_ctx *ctx, terra_tree_size_params *out);
typedef struct terra_tree_inst {int32_t type; float height, width;} terra_tree_inst;
int  terra_set_tree_instances(terra_ctx *ctx, const terra_tree_inst *h_insts, uint32_t count);
int  terra_get_tree_instances(terra_ctx *ctx, terra_tree_inst *h_insts, uint32_t capacity, uint32_t *count);
enum {TERRA_TREE_AO_NO_PINE_PALM = 1, TERRA_TREE_AO_NO_DECID = 2, TERRA_TREE_AO_DISTANT = 4};
int  terra_tiles_tree_ao_shadows_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                                     const terra_tree_place *d_pine, const uint32_t *d_pine_counts, uint32_t pine_capacity,
                                     const terra_decid_place *d_decid, const uint32_t *d_decid_counts, uint32_t decid_capacity,
                                     const float *d_decid_radius, const float *d_decid_radius_by_id, uint32_t num_radius_by_id, const uint8_t *d_flags,
                                     uint32_t list_capacity, uint8_t *d_tree_map, uint8_t *d_updated, float *d_trmax, uint32_t *d_list_counts);
int  terra_tiles_tree_ao_shadows(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                                 const terra_tree_place *h_pine, const uint32_t *h_pine_counts, uint32_t pine_capacity,
                                 const terra_decid_place *h_decid, const uint32_t *h_decid_counts, uint32_t decid_capacity,
                                 const float *h_decid_radius, const float *h_decid_radius_by_id, uint32_t num_radius_by_id, const uint8_t *h_flags,
                                 uint32_t list_capacity, uint8_t *h_tree_map, uint8_t *h_updated, float *h_trmax, uint32_t *h_list_counts);

/* ---- tree brush on the resident records of a tile batch (every supported tile size S): the fire modes "Add Trees" / "Remove Trees" -> tile_draw_t::add_or_remove_trees_at
 * (src/tiled_mesh.cpp:3746-3769) from :3756 on -> tile_t::add_or_remove_trees_at (:3822-3843) on every tile of the batch, with remove_tree (:3779-3787), remove_element
 * (src/inlines.h:743-747), update_trees_bcube (:3776-3778), tile_t::add_new_trees (:3805-3819), tile_t::mesh_sphere_intersect (:3796-3799) and the register_tree_change
 * decision of :3766-3768.  One call edits the pine / palm and the deciduous record arrays of the batch in place, bit for bit as the reference leaves its two vectors; with
 * terra_tiles_tree_ao_shadows before and after it a stroke is one stream of launches on resident data.
 * Inputs.  dxoff / dyoff: the tiles' mesh_off (xoff - xoff2), as for terra_tiles_tree_map.  xoff2 / yoff2: what the placements ran with; pine_xlate = decid_xlate =
 * ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0), an int sum times a float (tile_offset_t::get_xlate, src/animals.h:25), the same value as the tree AO call's
 * pt_off.  pos: camera space, as the reference receives it; pt_pos = dt_pos = pos - xlate.  radius: rradius.  is_square = (brush_shape == BSHAPE_CONST_SQ).
 * stats (required): mzmin, mzmax and radius are read.  skip, zvals: what they mean for the two brush placement calls; read only when add_trees is set (zvals is then
 * required for a deciduous group).  gen_flags (optional): [n] bytes, bit 0 = pine_trees_generated() is false, bit 1 = decid_trees.was_generated() is false.
 * pine / pine_counts / pine_capacity, decid / decid_counts / decid_capacity, decid_radius, decid_radius_by_id: as for terra_tiles_tree_ao_shadows, but written: a group
 * is absent when its counts are NULL or its capacity 0; a count above its capacity means the first `capacity` records.  trmax: [n], in and out.
 * Per tile, in the reference's order:
 *  1. The culls (:3824-3825).  mesh_sphere_intersect(pos, r) = dist_less_than(pos, get_center(), radius_t + r) && sphere_cube_intersect(pos, r, get_mesh_bcube())
 *     (src/tiled_mesh.h:229-241, BCUBE_ZTOLER 1e-6; DMIN_CHECK of src/Math3d.cpp:920-935 with its early return per axis) with radius_t = max(stats.radius,
 *     calc_radius() + trmax[t]): what postproc_trees (src/tiled_mesh.h:342-347) leaves, because trmax only grows; calc_radius() = 0.5*sqrt(DX_VAL*DX_VAL +
 *     DY_VAL*DY_VAL)*size, a float sqrt and double products (:204).  r = 1.1*rradius + 2.0*trmax[t] (a double expression narrowed at the call) fails: status 0.
 *     r = rradius fails: status 1.
 *  2. The removal loops (:3832-3833), pine / palm first.  A record stays when fabs(tpos.x - pos.x) > rradius || fabs(tpos.y - pos.y) > rradius, or when the brush is
 *     not square and dist_xy_less_than(tpos, pos, rradius) fails.  Removal is remove_element: the back is swapped in and the same index is tested again, so the
 *     survivors do NOT keep their order.  The resulting order: with M survivors among the first min(count, capacity) records, a survivor at an index below M stays
 *     where it is, and the holes below M, in ascending order, receive the survivors at indices >= M in descending order.  decid_radius, when given, moves with its
 *     records.  Every removed record adds the sphere (tpos + xlate, 2.0*get_radius()) to the update box, get_radius() as terra_tiles_tree_ao_shadows forms it (the
 *     per-record radius wins over decid_radius_by_id[tree_id]); a record that call would drop (bad type, instance, tree_id or radius) is removed by its position
 *     like any other and adds nothing to the box.  Records past the new count keep whatever the moves left there.
 *  3. The addition (:3835-3838), only when add_trees.  A group is extended when it is present, its gen_flags bit is clear and can_have_pine_palm_trees() /
 *     can_have_decid_trees() holds (skip and the zrange test of the brush placement calls).  The records terra_tiles_place_trees_brush makes for (pt_pos, rradius,
 *     is_square), in that call's order, are appended behind the M survivors; the same for terra_tiles_place_decid_trees_brush (which, like the reference, places over
 *     the whole tile at rradius == 0 and never reads is_square).  counts[t] = M + all new records; the array receives those that fit, and a count above the capacity
 *     keeps its meaning.  The appended records that are stored add their spheres to the update box (:3815-3817) and raise trmax[t] = max(trmax[t], get_radius())
 *     (postproc_trees).  This is exact as long as trmax[t] on input is at least the radius of every record present: PRECONDITION, met by the trmax output of
 *     terra_tiles_tree_ao_shadows on the same records.  A new deciduous record's radius is decid_radius_by_id[tree_id]; decid_radius, when given, receives it.
 *  4. status[t] = 2 when either group changed (a record removed, or new records made: trees.size() > start_sz), else 1.  On a tile that passed both
 *     culls counts[t] is rewritten (M + new) even when nothing changed; on every other tile nothing is written but status and changed.
 * After all tiles (:3764-3768): update_bcube = {x1, x2, y1, y2, z1, z2}, the union of all spheres over the batch, or six zeros when no sphere was added.  changed[t] = 1
 * when status[t] == 2 (register_tree_change, :3841), and when status[t] >= 1 and get_mesh_bcube().intersects(update_bcube) (src/3DWorld.h:536-539, adjacency
 * included); for each such tile the caller runs register_tree_change.  The box is specified BY VALUE (== on floats): it is a min / max union reduced on the device with
 * atomics, so it does not depend on the order of tiles and records, but a bound that is zero may come out as -0 where the reference has +0 (std::min keeps its first
 * argument on a tie).  Not reproduced: the is_all_zeros() restart of update_trees_bcube (:3777), which fires only while the box is exactly zero in all six values --
 * a tree of radius 0 at the origin; a box that is all zeros by value ends the call like the reference's :3764 (no changed beyond status 2).
 * With the caller stay: the static same-position early-out of :3748-3754, clear_pine_tree_vbos and the shadow-map clears of register_tree_change, the small_tree /
 * tree constructors of the new records, and the re-shadowing.  The reference re-shadows incrementally (only the changed tiles, against neighbours whose maps
 * exist); terra_tiles_tree_ao_shadows recomputes a batch from empty maps, and that is what a caller runs after this call.
 * radius == 0 is not special-cased: a round brush then removes nothing, a square one removes a record exactly at pt_pos, and the additions follow the two placement
 * calls.  TERRA_ERR_ARG (and nothing is changed): a NULL required pointer (pos; tile_xy, stats, trmax, status, changed when n > 0; the records of a group that is
 * present), a misaligned pointer, an unsupported S, a radius that is negative or not finite, a deciduous group without decid_radius and without
 * decid_radius_by_id, add_trees with a deciduous group and no decid_radius_by_id or no zvals, decid_radius_by_id (where it is needed) with num_radius_by_id !=
 * terra_decid_params.num_shared_trees or with 0 shared trees, `instanced` with an instance table of the wrong length, everything the two brush placement calls refuse
 * when add_trees, n*pine_capacity or n*decid_capacity beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene (and, when add_trees, while a heightmap texture is
 * set).  n == 0 does nothing.  The device form only enqueues and reads nothing back; tile_xy and pos are host arrays in both forms.  update_bcube may be NULL.  Scratch
 * comes from the context's arena. */
enum {TERRA_TREE_EDIT_PINE_NOT_GENERATED = 1, TERRA_TREE_EDIT_DECID_NOT_GENERATED = 2}; /* gen_flags */
int  terra_tiles_edit_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                                const float pos[3], float radius, int32_t add_trees, int32_t is_square,
                                const uint8_t *d_skip, const terra_tile_stats *d_stats, const float *d_zvals, const uint8_t *d_gen_flags,
                                terra_tree_place *d_pine, uint32_t *d_pine_counts, uint32_t pine_capacity,
                                terra_decid_place *d_decid, uint32_t *d_decid_counts, uint32_t decid_capacity,
                                float *d_decid_radius, const float *d_decid_radius_by_id, uint32_t num_radius_by_id,
                                float *d_trmax, uint8_t *d_status, uint8_t *d_changed, float *d_update_bcube);
int  terra_tiles_edit_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                            const float pos[3], float radius, int32_t add_trees, int32_t is_square,
                            const uint8_t *h_skip, const terra_tile_stats *h_stats, const float *h_zvals, const uint8_t *h_gen_flags,
                            terra_tree_place *h_pine, uint32_t *h_pine_counts, uint32_t pine_capacity,
                            terra_decid_place *h_decid, uint32_t *h_decid_counts, uint32_t decid_capacity,
                            float *h_decid_radius, const float *h_decid_radius_by_id, uint32_t num_radius_by_id,
                            float *h_trmax, uint8_t *h_status, uint8_t *h_changed, float *h_update_bcube);

/* ---- tile mesh shadows of one directional light: tile_t::calc_shadows_for_light + calc_mesh_shadows / mesh_shadow_gen (src/tiled_mesh.cpp:664-692,
 * src/visibility.cpp:411-520).  zvals: [n][S+2][S+2]; light_pos: the light's position vector (get_light_pos(l)); smask: [n][S+2][S+2] bytes, 0 or
 * MESH_SHADOW (0x02).  Shadows cross tile borders: a tile starts its sweeps from the edge heights left by its neighbours toward the light when those are
 * part of the batch (sh_out -> sh_in), otherwise from nothing, exactly like a tile whose neighbour does not exist.  Order of evaluation = the
 * reference's single-threaded order (its two OpenMP sections race). */
int  terra_tiles_mesh_shadows_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask);
int  terra_tiles_mesh_shadows(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, const float light_pos[3], uint8_t *h_smask);
/* The same for a batch that is only PART of the terrain (the rest lives on another GPU / rank): h_edge_in[i][0] = sh_in_x, h_edge_in[i][1] = sh_in_y of
 * tile i (130 floats each, host memory), used where h_edge_in_present[i][d] != 0 and the neighbour toward the light is not in the batch; h_edge_out[i][0..1]
 * receives every tile's sh_out_x / sh_out_y (MESH_MIN_Z = -1e6 where nothing was written) -- what the owner of the next tile away from the light needs.
 * All three are optional (NULL).  3dworld_amd/dist.py: tile strips over torch.distributed ranks, the border edges travel by send/recv. */
int  terra_tiles_mesh_shadows_halo_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask,
                                       const float *h_edge_in, const uint8_t *h_edge_in_present, float *h_edge_out);

/* ---- voxels: voxel_manager::create_procedural fill (src/voxels.cpp:278-346).  out is z-fastest: ix = z + (x + y*nx)*nz (src/voxels.h:141-144). */
int  terra_voxel_fill_dev(terra_ctx *ctx, float *d_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo_pos[3], const float vsz[3], const float offset[3],
                          float mag, float freq, int rseed1, int rseed2, int gen_mode, float zscale, int normalize_to_1);
/* the y slab [y0, y0 + nys) of the same field: d_out = nys*nx*nz floats, bit-identical to those rows of the full-grid call (voxels are independent; the axis
 * positions are the full grid's running sums, src/upsurface.cpp:41-57): one field as y slabs on several GPUs, no collective (3dworld_amd/dist.py, bench.py) */
int  terra_voxel_fill_slab_dev(terra_ctx *ctx, float *d_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo_pos[3], const float vsz[3], const float offset[3],
                               float mag, float freq, int rseed1, int rseed2, int gen_mode, float zscale, int normalize_to_1, uint32_t y0, uint32_t nys);
int  terra_voxel_fill(terra_ctx *ctx, float *h_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo_pos[3], const float vsz[3], const float offset[3],
                      float mag, float freq, int rseed1, int rseed2, int gen_mode, float zscale, int normalize_to_1);

/* ---- several GPUs from ONE host process.  3DWorld is a single C++ process that keeps eight generator objects in flight and collects them as they finish
 * (height_gens[8], src/tiled_mesh.h:418; src/tiled_mesh.cpp:2317,2367-2416).  terra_multi = N contexts, one per entry of device_indices (an index may repeat:
 * several contexts on one GPU), each driven by its own host thread for the duration of a call.  Units are dealt out in contiguous blocks -- context i gets
 * terra_multi_partition(n_units, size, i) -- of independent work: tiles (no neighbour data, src/tiled_mesh.cpp:515), rows of one heightmap
 * (src/heightmap.cpp:139-143), y slabs of a voxel field; nothing there is collective.  In the *_dev forms the outputs are arrays of per-context device
 * pointers (entry i lives on context i's device and holds its block).  terra_multi_foreach runs fn(ctx, index, user) on every context's thread at once for
 * everything else (e.g. one heightmap region per GPU: terra_gen_grid_minmax_dev + terra_apply_erosion_dev); a negative return is the call's error.
 * terra_multi_tiles_mesh_shadows: the one pass of the tile path with a cross-tile dependency (tile_t::calc_shadows_for_light, src/tiled_mesh.cpp:664-692) --
 * tile columns in strips, one per context, rows pipelined through the strips, the border tiles' outgoing edges handed from device to device
 * (hipMemcpyPeerAsync); host zvals in ([n][130][130]), host shadow masks out ([n][130][130]), same result as terra_tiles_mesh_shadows on one context. */
typedef struct terra_multi terra_multi;
int  terra_multi_create(terra_multi **out, const int *device_indices, uint32_t n);
void terra_multi_destroy(terra_multi *m);
uint32_t terra_multi_size(const terra_multi *m);
terra_ctx *terra_multi_ctx(terra_multi *m, uint32_t i);
void terra_multi_partition(uint32_t n_units, uint32_t n_parts, uint32_t part, uint32_t *first, uint32_t *count);
int  terra_multi_foreach(terra_multi *m, int (*fn)(terra_ctx *ctx, uint32_t index, void *user), void *user);
int  terra_multi_synchronize(terra_multi *m);
int  terra_multi_init_scene(terra_multi *m, const terra_config *cfg);
int  terra_multi_tiles_create_zvals_dev(terra_multi *m, const int32_t *tile_xy, uint32_t n, uint32_t erosion_iters_tt,
                                        float *const *d_zvals, terra_tile_stats *const *d_stats, uint8_t *const *d_normals, float *const *d_min_normal_z);
int  terra_multi_tiles_create_zvals(terra_multi *m, const int32_t *tile_xy, uint32_t n, uint32_t erosion_iters_tt,
                                    float *h_zvals, terra_tile_stats *h_stats, uint8_t *h_normals, float *h_min_normal_z);
int  terra_multi_gen_grid_rows_dev(terra_multi *m, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin,
                                   float *const *d_out, float *h_min, float *h_max);
int  terra_multi_voxel_fill_dev(terra_multi *m, float *const *d_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo_pos[3], const float vsz[3], const float offset[3],
                                float mag, float freq, int rseed1, int rseed2, int gen_mode, float zscale, int normalize_to_1);
int  terra_multi_tiles_mesh_shadows(terra_multi *m, const int32_t *tile_xy, uint32_t n, const float *h_zvals, const float light_pos[3], uint8_t *h_smask);
/* the device-resident form: the terrain already lies on the GPUs as strips of tile columns.  terra_multi_shadow_layout tells where: tile i belongs to context
 * ctx_of_tile[i] and is the pos_in_ctx[i]-th tile of that context's arrays (tiles_per_ctx[s] tiles on context s: rows toward the light first); d_zvals[s] / d_smask[s] are
 * [tiles_per_ctx[s]][130][130] on context s's device.  Between strips only the border tiles' 130-float edges move, device to device: an event behind a chunk's kernels, the
 * next strip's stream waits for it and gathers the edges out of the peer's buffer in one launch (xGMI; staged copies when the devices cannot map each other). */
int  terra_multi_shadow_layout(terra_multi *m, const int32_t *tile_xy, uint32_t n, const float light_pos[3], uint32_t *ctx_of_tile, uint32_t *pos_in_ctx, uint32_t *tiles_per_ctx);
int  terra_multi_tiles_mesh_shadows_dev(terra_multi *m, const int32_t *tile_xy, uint32_t n, float *const *d_zvals, const float light_pos[3], uint8_t *const *d_smask);
/* the device-resident form of the halo arrays of terra_tiles_mesh_shadows_halo_dev: d_edge_in / d_edge_out are [n][2][130] floats in device memory
 * (d_edge_in is read where h_edge_in_present says so); what terra_multi_tiles_mesh_shadows hands from GPU to GPU */
int  terra_tiles_mesh_shadows_edges_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask,
                                        const float *d_edge_in, const uint8_t *h_edge_in_present, float *d_edge_out);

/* ---- ONE grid whose row strips live on several GPUs ("erosion on one big grid").  apply_erosion works on one shared array in serial droplet order
 * (src/erosion.cpp:66-155): the droplets cannot be dealt out, the MEMORY can.  Strip i is a physical allocation on its owner's device; every rank maps all strips back
 * to back into one address range (HIP virtual memory management; a strip crosses a process boundary as a POSIX file descriptor, e.g. over a unix socket with
 * SCM_RIGHTS -- 3dworld_amd/dist.py).  Each rank then fills its own rows with terra_gen_grid_rows_minmax_dev at HBM speed, and ONE rank runs terra_apply_erosion_dev on the
 * mapped pointer: rows that live on another GPU are read and written over xGMI by the same kernels -- bit for bit the single-GPU result.
 *   rank r:  terra_dgrid_create(ctx, W, strip_bytes, r, &g); terra_dgrid_export_fd(g, &fd) -> send fd to the peers; terra_dgrid_import_fd(g, j, fd_j) for j != r;
 *            terra_dgrid_map(g, &d_grid)                 strip sizes must be multiples of terra_dgrid_granularity(ctx) (2 MiB on MI355X)
 * terra_multi_dgrid_create: the same inside one process -- strip i on context i's device, one pointer that every context's device may use. */
typedef struct terra_dgrid terra_dgrid;
size_t terra_dgrid_granularity(terra_ctx *ctx);
int  terra_dgrid_create(terra_ctx *ctx, uint32_t n_strips, const size_t *strip_bytes, uint32_t local_strip, terra_dgrid **out);
int  terra_dgrid_export_fd(terra_dgrid *g, int *fd);                    /* a new descriptor of the local strip (the caller closes it after sending) */
int  terra_dgrid_import_fd(terra_dgrid *g, uint32_t strip, int fd);     /* a peer's strip (the descriptor may be closed afterwards) */
int  terra_dgrid_map(terra_dgrid *g, void **d_base);
void terra_dgrid_destroy(terra_dgrid *g);
int  terra_multi_dgrid_create(terra_multi *m, const size_t *strip_bytes, terra_dgrid **out, void **d_base);

/* ---- the pine and palm tree draw lists of a tile batch for a camera (every supported tile size S): tile_t::draw_pine_trees (src/tiled_mesh.cpp:1465-1526) without
 * its GL and shader calls, with small_tree_group::draw_tree_insts, draw_pine_leaves, draw_non_pine_leaves and draw_trunks under it (src/sm_tree.cpp:206-323) -- the
 * per-frame decision about the trees of every drawn tile: which are drawn, in which form, in what order, bit for bit, from the records that
 * terra_tiles_place_trees_dev and terra_tiles_edit_trees_dev keep on the device.  A frame is then one stream of launches: zvals -> placements -> tree AO -> terrain
 * draw list -> grass draw lists -> tree draw lists, and only the lists are read back.
 * Restated with the source's operand types: draw_tree_leaves_lod (:1459-1462), the weights of update_pine_tree_state (:1440-1448), get_tree_dist_scale,
 * get_tree_far_weight, get_tree_scale_denom, get_dist_to_camera_in_tiles (src/tiled_mesh.h:95,332-338), contains_camera, get_back_to_front_ordering, calc_bcube /
 * add_bounds_to_bcube, small_tree::are_leaves_visible (:1007-1017), the decisions of small_tree::draw_trunk (:1081-1102, down to nsides), get_trunk_cylin (:767-777)
 * with get_tree_z_bottom / get_default_tree_depth (src/Tree.cpp:209-214, the tiled-terrain branch), get_xy_radius, get_trunk_bsphere_radius (src/small_tree.h:
 * 77-78), the two small_tree constructors as terra_tiles_tree_ao_shadows forms them, and pos_dir_up::sphere_visible_test (src/visibility.cpp:119-128).
 * sphere_in_camera_view(.., 2) is sphere_visible_test alone in tiled-terrain mode (src/visibility.cpp:338-339).
 * Inputs.  tile_xy on the host; dxoff / dyoff = xoff - xoff2 / yoff - yoff2 and xoff2 / yoff2 as for terra_tiles_tree_ao_shadows: xlate = ptree_off.get_xlate() =
 * ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0).  stats [n] (mzmin, mzmax, radius).  skip [n] bytes (optional): !can_have_trees(), or the tile is not in
 * to_draw -- the not_drawn bytes of terra_tiles_terrain_view plug in here.  trmax [n] (optional; NULL = 0; terra_tiles_tree_ao_shadows writes it): contains_camera()
 * tests get_bcube(), which is wider than the mesh by trmax.  pine [n][capacity] with counts [n] as the placement wrote them; a count above the capacity means the
 * first `capacity` records.  view; terra_tree_view_args, a host struct read at the call: behind_sphere_mult as for terra_tiles_terrain_view; shadow_pass;
 * window_width; zoom_f = (do_zoom ? ZOOM_FACTOR : 1); tree_depth_scale; draw_trunks / draw_near_leaves / draw_far_leaves: the three booleans of one
 * draw_pine_tree_bl sweep, in any combination, so that one call can answer a whole frame.  Everything else comes from terra_tree_params (tree_scale, instanced),
 * terra_tree_size_params and the instance table.
 * trunk_override [n][capacity] (optional).  A record's geometry is derived with a vertical trunk (r_angle == 0): exact for every pine, for every instanced record
 * (instances are never rotated, src/sm_tree.cpp:351,358) and for three in four generated palms.  setup_rotation's random draws belong to the small_tree
 * constructor, which stays with the engine: for a record whose entry has rotated != 0 the call uses the entry's cylinder as trunk_cylin and get_rot_dir() =
 * (p2 - p1).get_norm().  Entries with rotated == 0 are ignored.  This is the one thing an engine with rotated palms that are not instanced passes in.
 * Records that terra_tiles_tree_ao_shadows would drop -- a type outside stt[], an instance index outside the table, an instanced record while `instanced` is off --
 * are skipped everywhere and do not enter all_bcube.  `instanced` is the group's flag (enable_instanced()); a record with inst < 0 in an instanced group enters no
 * instance list (get_inst_id() asserts).  A skipped tile, or one without a valid record (pine_trees.empty()), gets a zero tile_out, zero all_bcube and zero counts,
 * and nothing else of it is written.
 * Outputs.  tile_out [n]: dscale = get_tree_dist_scale(); weight = the weight of :1492; num_pine / num_palm = num_pine_trees / num_palm_trees over the valid
 * records, num_trees = all valid records (bushes too), leaf_written = the entries of leaf_list that were written; flags: bits 0-1 the trunk mode (the branches of :1477-1489: 0 none, 1 polygons and all drawn, 2 polygons and draw_trunks() returned 0, so the tile also
 * joins to_draw_trunk_pts, 3 trunk points only), TERRA_TRV_NEAR_LEAVES / TERRA_TRV_FAR_LEAVES: draw_tree_leaves_lod ran with low_detail 0 / 1, TERRA_TRV_DITHERED: 0 <
 * weight < 1, TERRA_TRV_PALMS: the condition of :1517, TERRA_TRV_DRAW_ALL_NEAR / _FAR: draw_all of :1460 in the sweep that ran, TERRA_TRV_ALL_VISIBLE: the
 * sphere test of :1483 and :1520, TERRA_TRV_NEEDS_HIGH / _LOW: weights[0] > 0 / weights[1] > 0 in update_pine_tree_state (with force_high_detail = shadow_pass),
 * TERRA_TRV_CONTAINS_CAMERA.  all_bcube [n][6] = x1 x2 y1 y2 z1 z2 after calc_bcube(), by value: it is a min / max union, so a zero bound may come out with the
 * other sign.
 * pine_insts / palm_insts [n][capacity] with inst_counts [n][2]: the reference's tree_inst_t {id, pt} of draw_pine_insts / draw_palm_insts, written when the group is
 * instanced and the sweep draws it, after the cull of :250, in ascending id and within an id in ascending record index.  That order is the one deviation: the
 * reference calls std::sort on a comparison that looks at the id alone, so its order inside an id is whatever the library's introsort leaves; the instanced draw
 * per id does not depend on it.
 * leaf_list [n][capacity] with leaf_counts [n][2] (pine, palm): record indices of the forms that are not instanced.  The pine entries are what the high-detail
 * sweep draws when the group is not instanced and draw_all does not hold: in record order, but in the tile that contains the camera in the order of
 * get_back_to_front_ordering, ascending (p2p_dist_sq, index) -- a total order.  Under draw_all the list is not written and leaf_counts[0] is num_pine
 * (render_all); so it is when only the low-detail sweep draws pines.  The palm entries (draw_non_pine_leaves(0, 1, 0, ..), the group not instanced) follow the
 * written pine entries, in record order.
 * trunk [n][capacity] bytes, one per record in record order, written for every tile that is not skipped or empty, nonzero only in the polygon trunk modes: 0 not
 * drawn (a bush, culled, size_scale < dist, a dropped record), 1 a line that skip_lines skipped, otherwise nsides (4 .. N_CYL_SIDES = 32).  Vertex generation stays
 * with the engine.  Entries past the counts are never written.
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or the args; window_width, zoom_f or tree_depth_scale not > 0; a NULL required pointer
 * (view, args; tile_xy, stats, counts, tile_out, all_bcube, inst_counts, leaf_counts when n > 0; the records and the four [n][capacity] outputs when capacity > 0
 * as well); a pointer other than skip and trunk that is not 4-byte aligned; an unsupported S; `instanced` with an instance table whose length is not
 * num_pine_insts + num_palm_insts; n*capacity beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.  The
 * device form only enqueues and reads nothing back; tile_xy is a host array in both forms.  Scratch comes from the context's arena. */
typedef struct terra_tree_view_args {
	float behind_sphere_mult;  /* pos_dir_up::behind_sphere_mult */
	float zoom_f;              /* do_zoom ? ZOOM_FACTOR : 1 */
	float tree_depth_scale;
	int32_t window_width;
	int32_t shadow_pass;
	int32_t draw_trunks, draw_near_leaves, draw_far_leaves;
} terra_tree_view_args;      /* 32 bytes */
typedef struct terra_tree_view_tile {float dscale, weight; uint32_t flags, num_pine, num_palm, num_trees, leaf_written, pad;} terra_tree_view_tile; /* 32 bytes */
typedef struct terra_tree_view_inst {uint32_t id; float pt[3];} terra_tree_view_inst;                                        /* tree_inst_t, 16 bytes */
typedef struct terra_trunk_override {float p1[3], p2[3], r1, r2; int32_t rotated;} terra_trunk_override;                     /* 36 bytes */
enum {TERRA_TRV_TRUNK_NONE = 0, TERRA_TRV_TRUNK_POLY_ALL = 1, TERRA_TRV_TRUNK_POLY_SKIPPED = 2, TERRA_TRV_TRUNK_POINTS = 3, TERRA_TRV_TRUNK_MASK = 3,
      TERRA_TRV_NEAR_LEAVES = 0x4, TERRA_TRV_FAR_LEAVES = 0x8, TERRA_TRV_DITHERED = 0x10, TERRA_TRV_PALMS = 0x20, TERRA_TRV_DRAW_ALL_NEAR = 0x40,
      TERRA_TRV_DRAW_ALL_FAR = 0x80, TERRA_TRV_ALL_VISIBLE = 0x100, TERRA_TRV_NEEDS_HIGH = 0x200, TERRA_TRV_NEEDS_LOW = 0x400, TERRA_TRV_CONTAINS_CAMERA = 0x800};
int  terra_tiles_tree_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                               const terra_tree_view_args *args, const terra_tile_stats *d_stats, const uint8_t *d_skip, const float *d_trmax, const terra_tree_place *d_pine,
                               const uint32_t *d_pine_counts, uint32_t capacity, const terra_trunk_override *d_trunk_override, terra_tree_view_tile *d_tile_out,
                               float *d_all_bcube, terra_tree_view_inst *d_pine_insts, terra_tree_view_inst *d_palm_insts, uint32_t *d_inst_counts, uint32_t *d_leaf_list,
                               uint32_t *d_leaf_counts, uint8_t *d_trunk);
int  terra_tiles_tree_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                           const terra_tree_view_args *args, const terra_tile_stats *h_stats, const uint8_t *h_skip, const float *h_trmax, const terra_tree_place *h_pine,
                           const uint32_t *h_pine_counts, uint32_t capacity, const terra_trunk_override *h_trunk_override, terra_tree_view_tile *h_tile_out,
                           float *h_all_bcube, terra_tree_view_inst *h_pine_insts, terra_tree_view_inst *h_palm_insts, uint32_t *h_inst_counts, uint32_t *h_leaf_list,
                           uint32_t *h_leaf_counts, uint8_t *h_trunk);

/* ---- the scenery draw lists of a tile batch for a camera (every supported tile size S): tile_t::draw_scenery (src/tiled_mesh.cpp:1580-1592) for every tile, without
 * its GL, shader and colour calls, over the records terra_tiles_place_scenery[_dev] leaves -- so that a frame's stream is zvals -> placements -> ... -> tree draw
 * lists -> scenery draw lists, with nothing read back but the lists.  One call answers both sweeps of tile_draw_t::draw_scenery (args.draw_opaque / draw_leaves).
 * Restated with the source's operand types: scenery_group::draw_opaque_objects and draw_plant_leaves (src/scenery.cpp:1413-1500), rock_shape3d::draw (:300-305),
 * surface_rock::draw (:394-417), s_rock::draw (:442-461), voxel_rock::draw (:517-530), s_log::draw (:606-632), s_stump::draw (:670-693), s_plant::draw_stem,
 * draw_leaves and draw_berries (:853-871, 898-934), leafy_plant::draw_leaves (:1030-1045), mushroom::draw (:1062-1081), scenery_obj::check_visible / is_visible /
 * get_size_scale (:122-135; the float pow with scale_exp 8.0), skip_uw_draw and get_pt_line_thresh (:61-74), the get_bsphere_radius() overrides, get_scenery_thresh /
 * get_scenery_dist_scale (src/tiled_mesh.h:333-334) over get_dist_to_camera_in_tiles(0), get_tile_width, get_def_smap_ndiv (src/shadow_map.cpp:57-64) and
 * distance_to_camera.  sscale is the int of :1456 taken as the float parameter of every draw(); 2.0*sscale*radius/dist, 0.5*radius/approx_pixel_width,
 * 0.75*get_pt_line_thresh()*radius, 1000.0*radius and the 0.5*height / 0.1*(..) terms are formed in double, 2*get_pt_line_thresh()*radius in float.  In tiled-terrain
 * mode check_visible is camera_pdu.sphere_visible_test alone, in the shadow pass too, and sphere_in_camera_view(.., 2) is the same test.  next_frame, burn_amt,
 * is_shadowed and the colours stay with the engine.
 * Inputs.  tile_xy on the host; dxoff / dyoff and xoff2 / yoff2 as for terra_tiles_tree_view: xlate = scenery_off.get_xlate() = ((dxoff + xoff2)*DX_VAL,
 * (dyoff + yoff2)*DY_VAL, 0).  stats [n] (mzmin, mzmax, radius).  skip [n] bytes (optional): !scenery.generated, or the tile is not in to_draw -- the not_drawn
 * bytes of terra_tiles_terrain_view plug in.  objs [n][capacity] with counts [n] as the placement wrote them; a count above the capacity means the first `capacity`
 * records.  radius_override [n][capacity] floats (optional): an entry > 0 replaces the record's radius -- voxel_rock::build_model divides the radius by the model's
 * bounding radius, and a rock_shape3d record carries radius 0 because gen_rock runs in the engine; a rock_shape with an override also gets pos.z += 0.1*radius (:156).
 * A rock_shape without an override is not decided: its draw word is TERRA_SCV_ENGINE and it enters no list.  water_plane_z and get_min_water_plane_z() are the
 * scene's, tree_scale comes from terra_tree_params.
 * Per tile: get_scenery_dist_scale(reflection_pass) > 1.0 drops the tile; scale_val = get_scenery_thresh(reflection_pass)*get_tile_width().  tile_out [n]:
 * dist_scale, scale_val, flags (TERRA_SCV_TILE_DRAWN, _OPAQUE / _LEAVES: which sweeps ran), num_records = min(counts, capacity), list_written = the entries of `list`
 * that were written.  A skipped, dropped or empty tile gets a zero record and zero group_counts, and nothing else of it is written.
 * Per record of every other tile, in record order: draw [n][capacity] words.  Bits 0-2 the opaque form: 0 not drawn, TERRA_SCV_POINT a point in tree_scenery_pld
 * (surface rocks and rocks beyond 2*get_pt_line_thresh()*radius), TERRA_SCV_LINE a line in it (logs, stumps, plant stems), TERRA_SCV_POLY polygons, TERRA_SCV_ENGINE.
 * Bits 8-13 ndiv of the polygon form (0 for rock_shape, surface_rock and voxel_rock, which have none).  TERRA_SCV_LOG_END: the log's end cap is drawn (:623), with
 * TERRA_SCV_LOG_END2 the end at pt2 (radius2), else the end at pos; TERRA_SCV_STUMP_TOP (:687); TERRA_SCV_CAP_UNDERSIDE (:1077); TERRA_SCV_LEAVES: the leaves of a
 * plant or a leafy plant are drawn; TERRA_SCV_UNDERWATER: the leafy plant's is_underwater (:1035); TERRA_SCV_BERRIES: the plant passes draw_berries up to
 * berries.empty(), which the engine knows, with the berries' ndiv in bits 16-21.  A record whose kind is none of TERRA_SCENERY_* gets 0.
 * size_scale [n][capacity] floats: get_size_scale(dist, scale_val) of a surface rock, rock or voxel rock drawn as polygons (the engine multiplies by scale,
 * size*scale or radius), 0 elsewhere.  dist [n][capacity] floats: the distance_to_camera the kind computes (a plant: of the stem or the berries, the same point), 0
 * where the record was culled before it or the kind computes none (rock_shape, leafy plants, a plant in a leaves-only call).
 * Logs and stumps are not drawn when shadow_pass && skip_small_shadow_objs (:1471); mushrooms and berries are not drawn in the shadow pass; the water-plant
 * conditions of :855 and :901 read the record's iv[0] against NUM_LAND_PLANT_TYPES.
 * Lists.  list [n][list_capacity] record indices with group_counts [n][TERRA_SCV_GROUPS], the groups in the order in which the reference issues them: rock_shape,
 * surface_rock, rock, log, stump, mushroom, plant stem (polygon forms only), berries, voxel_rock, plant leaves, leafy-plant leaves, pld points (surface rocks, then
 * rocks), pld lines (logs, stumps, stems).  Within a group, and within each kind inside the two pld groups, the order is record order: the order of the reference's
 * per-kind vectors.  A group's entries start at the sum of the counts before it; only the first list_capacity entries of a tile are written, group_counts still
 * reports all, entries past the counts are never written.  A plant can appear in three groups: 3*capacity always suffices.
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or the args; window_width or zoom_f not > 0; smap_pixel_width not > 0 under shadow_pass;
 * reflection_pass other than 0 or 1; a NULL required pointer (view, args; tile_xy, stats, counts, tile_out, group_counts when n > 0; objs, draw, size_scale, dist
 * when capacity > 0 as well; list when list_capacity > 0); a pointer other than skip that is not 4-byte aligned; an unsupported S; n*capacity or n*list_capacity
 * beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.  The device form only enqueues and reads nothing
 * back; tile_xy is a host array in both forms.  Scratch comes from the context's arena. */
typedef struct terra_scenery_view_args {
	float behind_sphere_mult;   /* as for terra_tiles_terrain_view */
	float zoom_f;               /* do_zoom ? ZOOM_FACTOR : 1 */
	float smap_pixel_width;     /* approx_pixel_width(shadow_map_sz); read only when shadow_pass */
	int32_t window_width;
	int32_t shadow_pass;        /* shadow_only */
	int32_t reflection_pass;    /* 0 or 1: the bool of tile_t::draw_scenery */
	int32_t uw_skip;            /* !DISABLE_WATER && (display_mode & 0x04): skip_uw_draw's gate */
	int32_t skip_small_shadow_objs; /* can_skip_small_shadow_objs() */
	int32_t draw_opaque, draw_leaves; /* the two sweeps of tile_draw_t::draw_scenery, in any combination */
} terra_scenery_view_args;      /* 40 bytes */
typedef struct terra_scenery_view_tile {float dist_scale, scale_val; uint32_t flags, num_records, list_written, pad[3];} terra_scenery_view_tile; /* 32 bytes */
enum {TERRA_SCV_NONE = 0, TERRA_SCV_POINT = 1, TERRA_SCV_LINE = 2, TERRA_SCV_POLY = 3, TERRA_SCV_ENGINE = 7, TERRA_SCV_FORM_MASK = 7,
      TERRA_SCV_LOG_END = 0x8, TERRA_SCV_LOG_END2 = 0x10, TERRA_SCV_STUMP_TOP = 0x20, TERRA_SCV_CAP_UNDERSIDE = 0x40, TERRA_SCV_LEAVES = 0x80,
      TERRA_SCV_NDIV_SHIFT = 8, TERRA_SCV_NDIV_MASK = 0x3F, TERRA_SCV_UNDERWATER = 0x4000, TERRA_SCV_BERRIES = 0x8000, TERRA_SCV_BERRY_NDIV_SHIFT = 16};
enum {TERRA_SCV_TILE_DRAWN = 1, TERRA_SCV_TILE_OPAQUE = 2, TERRA_SCV_TILE_LEAVES = 4};
enum {TERRA_SCV_G_ROCK_SHAPE, TERRA_SCV_G_SURFACE_ROCK, TERRA_SCV_G_ROCK, TERRA_SCV_G_LOG, TERRA_SCV_G_STUMP, TERRA_SCV_G_MUSHROOM, TERRA_SCV_G_STEM, TERRA_SCV_G_BERRIES,
      TERRA_SCV_G_VOXEL_ROCK, TERRA_SCV_G_PLANT_LEAVES, TERRA_SCV_G_LEAFY_LEAVES, TERRA_SCV_G_PLD_POINTS, TERRA_SCV_G_PLD_LINES, TERRA_SCV_GROUPS};
int  terra_tiles_scenery_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                                  const terra_scenery_view_args *args, const terra_tile_stats *d_stats, const uint8_t *d_skip, const terra_scenery_place *d_objs,
                                  const uint32_t *d_counts, uint32_t capacity, const float *d_radius_override, terra_scenery_view_tile *d_tile_out, uint32_t *d_draw,
                                  float *d_size_scale, float *d_dist, uint32_t *d_list, uint32_t list_capacity, uint32_t *d_group_counts);
int  terra_tiles_scenery_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                              const terra_scenery_view_args *args, const terra_tile_stats *h_stats, const uint8_t *h_skip, const terra_scenery_place *h_objs,
                              const uint32_t *h_counts, uint32_t capacity, const float *h_radius_override, terra_scenery_view_tile *h_tile_out, uint32_t *h_draw,
                              float *h_size_scale, float *h_dist, uint32_t *h_list, uint32_t list_capacity, uint32_t *h_group_counts);

/* ---- the deciduous tree draw lists of a tile batch for a camera (every supported tile size S): tile_t::draw_decid_trees (src/tiled_mesh.cpp:1555-1563) without its
 * GL, shader and colour calls, with tree_cont_t::draw_branches_and_leaves (src/Tree.cpp:312-368), tree::draw_leaves_top (:993-1052) and tree::draw_branches_top
 * (:948-990) under it -- the per-frame decision about the deciduous trees of every drawn tile: which are drawn, in which form, with how many leaves and branch
 * quads, in what order, bit for bit in fp32 and integers, from the records that terra_tiles_place_decid_trees_dev and terra_tiles_edit_trees_dev keep on the device.
 * A frame is then one stream of launches: zvals -> placements -> tree AO -> terrain draw list -> grass -> tree -> scenery -> deciduous draw lists, and only the lists
 * are read back.  One call answers both sweeps of tile_draw_t::draw_decid_trees (args.draw_leaves / args.draw_branches); when both run the leaves come first, as at
 * src/tiled_mesh.cpp:3268-3292.
 * Restated with the source's operand types: tree::is_visible_to_camera (:858-861), tree::calc_size_scale (:919-928), tree_data_t::get_size_scale_mult (:930), the
 * counts of tree_data_t::draw_leaves (:1182-1188) and draw_branches (:1128-1140), tree_cont_t::calc_bcube (:2458-2461) with tree::add_bounds_to_bcube (:862-865),
 * get_draw_tile_dist (src/tiled_mesh.cpp:117), InvSqrt (src/inlines.h:39-50: the bit trick with one iteration, not 1/sqrtf), pos_dir_up::cube_visible_likely
 * (src/3DWorld.h:724: !valid || point_visible_test(c.get_cube_center()) || cube_visible(c)), cube_t::get_cube_center (0.5f*(d0 + d1)), is_zero_area (some d0 == d1),
 * is_all_zeros, closest_dist_less_than (dist_less_than(pos, closest_pt(pos), dist), src/csg.cpp:247) and sphere_visible_test.
 * Tiled-terrain mode throughout: sphere_in_camera_view(.., 0 or 2) is sphere_visible_test alone (src/visibility.cpp:338-339), so ztop / czmax are not read;
 * wind_enabled and leaf_dynamic_en are 0; rot_angle, the world_space_offset uniform, bcolor, gen_leaf_color and update_leaf_cobj_color stay with the engine.
 * Mixed arithmetic: 1.1*sphere_radius is a double product narrowed to the float parameter; 1.0*(X_SCENE_SIZE + Y_SCENE_SIZE), 1.5*num_branch_quads*size_scale*mult
 * and 4.0*nl*size_scale*mult are formed in double; (1.0 - geom_opacity) is a double narrowed to the float parameter of add_leaves / add_branches; size_scale < 0.05
 * and the tests against 0.0 and 2.0 compare in double.  unsigned(double) converts as the reference binary does (cvttsd2si to 64 bits, the low word; a value beyond
 * the 64-bit range gives 0): with the camera on a tree's sphere centre InvSqrt(0) is about 2e19 and the product overflows, so the count falls to nl/8 or num/40.
 * Billboard opacity: CLIP_TO_01((size_scale - lod_end)/lod_denom), 0 when lod_denom == 0; lod_start / lod_end are args.lod_scales (tree_lod_scales[4]: branch start,
 * branch end, leaf start, leaf end).
 * Inputs.  tile_xy on the host (checked, not read: no decision depends on a tile's place).  dxoff / dyoff and xoff2 / yoff2 as for terra_tiles_tree_view: xlate =
 * dtree_off.get_xlate() = ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0).  skip [n] bytes (optional): !can_have_trees(), or the tile is not in to_draw -- the
 * not_drawn bytes of terra_tiles_terrain_view plug in here.  decid [n][capacity] with counts [n] as the placement and the brush leave them; a count above the
 * capacity means the first `capacity` records.  view; terra_decid_view_args, a host struct read at the call: behind_sphere_mult as for terra_tiles_terrain_view;
 * zoom_f = (do_zoom ? ZOOM_FACTOR : 1); lod_scales; shadow_pass; reflection_pass (0 or 1); billboards = USE_TREE_BILLBOARDS (the call itself applies && !shadow_pass,
 * src/tiled_mesh.cpp:3262); leaf_color_changed; draw_leaves, draw_branches.
 * tree_data [num_tree_data] of terra_decid_tree_data: what the decisions read of a shared tree_data_t, which gen_tree makes and the engine owns -- base_radius,
 * sphere_radius, sphere_center_zoff, lr_z_cent; leaves_bcube / branches_bcube (x1 x2 y1 y2 z1 z2, relative to tree_center); num_leaves = leaves.size(),
 * num_branch_quads; flags: TERRA_DCV_GENERATED (is_created(): the trees that use it are `created`), TERRA_DCV_HAS_4TH (has_4th_branches), TERRA_DCV_LEAF_TEX /
 * TERRA_DCV_BRANCH_TEX (get_render_leaf_texture().is_valid() / get_render_branch_texture().is_valid()).  A device array in the device form.  num_tree_data must equal
 * terra_decid_params.num_shared_trees and be > 0: tiled terrain always runs with shared trees (max_unique_trees, src/tiled_mesh.cpp:1540).
 * A record is dropped if its tree_id is outside the table or its entry is not GENERATED: it is not drawn and not in all_bcube, as in terra_tiles_tree_ao_shadows.
 * Every order below is taken over the remaining (valid) records.
 * not_visible [n][capacity] bytes (optional, read and written): tree::not_visible, the one piece of state the leaves sweep hands to the branches sweep.  The leaves
 * sweep outside the shadow pass writes it exactly where :1017 assigns it -- every valid record of a tile that passes the all_bcube test -- and no other byte.  A
 * branches sweep in the same call reads what that sweep computed, whether the array is given or not; a branches-only call reads the array (NULL = all zero).  The
 * shadow pass neither reads nor writes it.
 * Outputs.  tile_out [n]: flags -- TERRA_DCV_TILE_DRAWN (passed :1557 and the cull of :316: !all_bcube.is_zero_area() && !cube_visible(all_bcube + xlate) culls),
 * TERRA_DCV_TILE_LEAVES / _BRANCHES (which sweeps ran), TERRA_DCV_TILE_SORTED (the sorted branch of :352: not the shadow pass, and all_bcube is all zeros or
 * closer to camera - xlate than X_SCENE_SIZE + Y_SCENE_SIZE), TERRA_DCV_TILE_BCUBE_ZERO_AREA; num_trees = the valid records; leaf_written, branch_written,
 * leaf_bb_written, branch_bb_written = the entries written to the four lists.  all_bcube [n][6] = x1 x2 y1 y2 z1 z2 after calc_bcube(), by value: it is a min / max
 * union, so a zero bound may come out with either sign.  (assign_or_union_with_cube ignores a branches box of all zeros and replaces an all_bcube of all zeros;
 * union_with_cube takes every leaves box, so the zero cube stays in the union when the first tree's branches box is all zeros or a leaves box is.)  A tile that is
 * skipped, or empty after the drops, gets a zero record, a zero all_bcube and zero counts, and nothing else of it is written; a tile culled by all_bcube gets its
 * flags, num_trees, all_bcube and zero counts.
 * Per record, in record order, for every valid record of a drawn tile, the four arrays of a sweep only when that sweep ran; entries of dropped records and past the
 * counts are never written.  leaf_word [n][capacity]: bits 0-1 the leaves' form -- 0 not drawn, 1 geometry, 2 geometry and a billboard entry (0 < geom_opacity < 1
 * in every usual setting of lod_scales), 3 billboard only (geom_opacity == 0); TERRA_DCV_NOT_VISIBLE: not_visible as computed; bits 4-7 the stage at which a record
 * that is not drawn left: TERRA_DCV_STAGE_NOT_VISIBLE, _NO_LEAVES, _BOX (the leaves' box), _SIZE (size_scale == 0), and in the shadow pass _SHADOW_DIST /
 * _SHADOW_SPHERE (the culls of :338-339), 0 otherwise.  leaf_scale, leaf_opacity [n][capacity] floats: size_scale as last_size_scale would hold it (0 where the
 * record left before it was formed) and geom_opacity (0 where not formed); in the shadow pass 0.5 (the value passed to draw_leaves_shadow_only) and 1.  leaf_num
 * [n][capacity]: nl of draw_leaves (0 where not drawn as geometry).  branch_word, branch_scale, branch_opacity, branch_num: the same for draw_branches_top, the
 * stages TERRA_DCV_STAGE_NOT_VISIBLE, _BOX (the branches' box), _SIZE (size_scale < 0.05) and _SHADOW_DIST (:325); TERRA_DCV_NOT_VISIBLE as read; branch_num = num
 * of draw_branches, TERRA_DCV_LOW_DETAIL its low_detail (:1131-1133; force_low_detail = reflection_pass); the shadow pass is draw_branches(1.0, 1, 1).
 * Lists per tile, with list_counts [n][4] (leaf_list, branch_list, leaf_bb, branch_bb).  A list holds a record at most once, so it never outgrows the capacity.
 * leaf_list [n][capacity]: record indices of the trees that reach td.draw_leaves, in the reference's order: under TERRA_DCV_TILE_SORTED ascending
 * (p2p_dist_sq(sphere_center(), camera - xlate), index) -- std::sort of a pair<float, unsigned> is a total order, so no deviation; the key takes sphere_center()
 * without xlate --, otherwise record order.  branch_list [n][capacity]: the trees that reach td.draw_branches, in record order.  leaf_bb / branch_bb [n][capacity]
 * of terra_decid_view_bb: the entries add_leaves / add_branches receive from this tile; pos for leaves is draw_pos + (0, 0, lr_z_cent - sphere_center_zoff), for
 * branches draw_pos = sphere_center() + xlate; opacity = 1 - geom_opacity; rec the record's index.  Order: ascending tree_id, and within an id the order in which
 * the reference adds them (leaf_list's order for leaves -- the sorted sequence under TERRA_DCV_TILE_SORTED --, record order for branches).  This is the one stated
 * deviation, the one the tree view's instance lists carry: tree_lod_render_t::finalize sorts all tiles' entries with a comparison that looks at the tree_data_t
 * pointer alone, so the order inside one tree's run is whatever introsort leaves; render_billboards only needs the runs.  Merging the tiles' runs stays with the
 * engine.
 * TERRA_ERR_ARG, with nothing written: a non-finite member of the view or the args (lod_scales included); zoom_f not > 0; reflection_pass other than 0 or 1; a NULL
 * required pointer (view, args, tree_data; tile_xy, counts, tile_out, all_bcube, list_counts when n > 0; the records, the eight per-record arrays and the four lists
 * when capacity > 0 as well); a pointer other than skip and not_visible that is not 4-byte aligned; an unsupported S; num_tree_data that is 0 or differs from
 * num_shared_trees; n*capacity beyond 32 bits.  TERRA_ERR_STATE before terra_init_scene.  n == 0 does nothing once the checks have passed.  The device form only
 * enqueues and reads nothing back; tile_xy is a host array in both forms.  Scratch comes from the context's arena.  The host form uploads the per-record arrays and
 * the lists as the caller has them and copies them back, so the entries the call does not write keep the caller's bytes. */
typedef struct terra_decid_view_args {
	float behind_sphere_mult;  /* pos_dir_up::behind_sphere_mult */
	float zoom_f;              /* do_zoom ? ZOOM_FACTOR : 1 */
	float lod_scales[4];       /* tree_lod_scales: branch start, branch end, leaf start, leaf end */
	int32_t shadow_pass, reflection_pass, billboards, leaf_color_changed;
	int32_t draw_leaves, draw_branches;
} terra_decid_view_args;     /* 48 bytes */
typedef struct terra_decid_tree_data {
	float base_radius, sphere_radius, sphere_center_zoff, lr_z_cent;
	float leaves_bcube[6], branches_bcube[6];
	uint32_t num_leaves, num_branch_quads, flags, pad;
} terra_decid_tree_data;     /* 80 bytes */
typedef struct terra_decid_view_tile {uint32_t flags, num_trees, leaf_written, branch_written, leaf_bb_written, branch_bb_written, pad[2];} terra_decid_view_tile; /* 32 bytes */
typedef struct terra_decid_view_bb {uint32_t tree_id, rec; float pos[3], opacity;} terra_decid_view_bb;                                                        /* 24 bytes */
enum {TERRA_DCV_GENERATED = 1, TERRA_DCV_HAS_4TH = 2, TERRA_DCV_LEAF_TEX = 4, TERRA_DCV_BRANCH_TEX = 8};
enum {TERRA_DCV_TILE_DRAWN = 1, TERRA_DCV_TILE_LEAVES = 2, TERRA_DCV_TILE_BRANCHES = 4, TERRA_DCV_TILE_SORTED = 8, TERRA_DCV_TILE_BCUBE_ZERO_AREA = 16};
enum {TERRA_DCV_FORM_NONE = 0, TERRA_DCV_FORM_GEOM = 1, TERRA_DCV_FORM_BOTH = 2, TERRA_DCV_FORM_BILLBOARD = 3, TERRA_DCV_FORM_MASK = 3, TERRA_DCV_NOT_VISIBLE = 4,
      TERRA_DCV_LOW_DETAIL = 8, TERRA_DCV_STAGE_SHIFT = 4, TERRA_DCV_STAGE_NONE = 0, TERRA_DCV_STAGE_NOT_VISIBLE = 1, TERRA_DCV_STAGE_NO_LEAVES = 2, TERRA_DCV_STAGE_BOX = 3,
      TERRA_DCV_STAGE_SIZE = 4, TERRA_DCV_STAGE_SHADOW_DIST = 5, TERRA_DCV_STAGE_SHADOW_SPHERE = 6};
int  terra_tiles_decid_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                                const terra_decid_view_args *args, const terra_decid_tree_data *d_tree_data, uint32_t num_tree_data, const uint8_t *d_skip,
                                const terra_decid_place *d_decid, const uint32_t *d_counts, uint32_t capacity, uint8_t *d_not_visible, terra_decid_view_tile *d_tile_out,
                                float *d_all_bcube, uint32_t *d_leaf_word, float *d_leaf_scale, float *d_leaf_opacity, uint32_t *d_leaf_num, uint32_t *d_branch_word,
                                float *d_branch_scale, float *d_branch_opacity, uint32_t *d_branch_num, uint32_t *d_leaf_list, uint32_t *d_branch_list,
                                terra_decid_view_bb *d_leaf_bb, terra_decid_view_bb *d_branch_bb, uint32_t *d_list_counts);
int  terra_tiles_decid_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                            const terra_decid_view_args *args, const terra_decid_tree_data *h_tree_data, uint32_t num_tree_data, const uint8_t *h_skip,
                            const terra_decid_place *h_decid, const uint32_t *h_counts, uint32_t capacity, uint8_t *h_not_visible, terra_decid_view_tile *h_tile_out,
                            float *h_all_bcube, uint32_t *h_leaf_word, float *h_leaf_scale, float *h_leaf_opacity, uint32_t *h_leaf_num, uint32_t *h_branch_word,
                            float *h_branch_scale, float *h_branch_opacity, uint32_t *h_branch_num, uint32_t *h_leaf_list, uint32_t *h_branch_list,
                            terra_decid_view_bb *h_leaf_bb, terra_decid_view_bb *h_branch_bb, uint32_t *h_list_counts);

/* ---- sphere collisions and tree box tests against the resident containers of a tile batch (every supported tile size S): what lets an engine drop its host copy
 * of the pine / palm, deciduous and scenery containers.  terra_tiles_sphere_collide answers nq independent calls of tile_draw_t::check_sphere_collision
 * (src/tiled_mesh.cpp:3566-3569: the player, :3570-3575, and every large physics object, src/Physics.cpp:858) or of tile_t::check_sphere_collision (:2146-2168: every
 * butterfly every frame, src/animals.cpp:422); terra_tiles_cube_int_trees answers nq calls of tile_draw_t::check_cube_int_trees (:3576-3579: balcony placement,
 * src/building_rooms.cpp:1655).  Restated bit for bit with the source's operand types: get_tile_pair_at_point (:3532-3534; round_fp of a float expression, converted
 * as x86 converts it), tile_t::get_bcube / contains_point / get_tile_zmax (src/tiled_mesh.h:207,232-236,264), small_tree_group::check_sphere_coll and
 * small_tree::check_sphere_coll (src/sm_tree.cpp:181-186, 841-852), tree_cont_t::check_sphere_coll and tree::check_sphere_coll (src/Tree.cpp:280-294),
 * scenery_group::check_sphere_coll (src/scenery.cpp:1187-1199) over scenery_obj::check_sphere_coll (:80-86), s_stump::check_sphere_coll (:665-668) and
 * s_plant::check_sphere_coll (:772-775), sphere_vert_cylin_intersect (src/Math3d.cpp:427-437, without its asserts), sphere_cube_intersect (:930-935), dist_less_than,
 * dist_xy_less_than, contains_pt_exp, is_zero_area, contains_pt_xy, get_norm(); tree_cont_t::check_cube_int and tree::check_cube_int (src/Tree.cpp:296-309).
 * 1.001*rsum, 0.9*br_scale*base_radius, 0.2*height, 0.1*height and 0.1*radius are formed in double and narrowed where the source narrows them.
 * Line queries with inc_trees = 1 (line_intersect_trunc_cone against the pine cylinders) are terra_tiles_line_intersect_trees[_dev], beside the line queries above.
 *
 * What a query sees, as in the reference.  Every hit moves the centre and every later object sees the moved centre, within a container and across containers:
 * pine / palm, then deciduous, then scenery; nothing ends early.  The scenery is walked by kind -- rock_shapes, surface_rocks, voxel_rocks, rocks, (logs: no
 * collision), stumps, plants, leafy_plants (mushrooms: none) -- and within a kind in record order; the record list is the stable interleave of those vectors.
 * `pos -= xlate; ..; pos += xlate` runs for a container whenever it is included and present (a tree container: it holds a valid record; the scenery: generated), hit
 * or no hit, also when its all_bcube gate returns early: in floats that round trip is not the identity, and pos comes back as the reference leaves it.  The three
 * translations are ((dxoff + xoff2)*DX_VAL, (dyoff + yoff2)*DY_VAL, 0) with the container's own xoff2 / yoff2.  Both tree containers gate on
 * !all_bcube.is_zero_area() && !sphere_cube_intersect(center, radius, all_bcube) with the centre as it stands at the container's turn; all_bcube is calc_bcube()
 * over the valid records exactly as terra_tiles_tree_view and terra_tiles_decid_view form it, computed by this call.  Records that those views drop are skipped
 * and do not enter all_bcube: a bad type, an instance outside the table, an instanced record while `instanced` is off, a tree_id outside the table or not
 * TERRA_DCV_GENERATED.  A rock_shape or voxel_rock takes radius_override as terra_tiles_scenery_view defines it (pos.z += 0.1*radius for a rock_shape with one); a
 * rock_shape without an override is not tested, and TERRA_COLL_ROCK_SHAPE_UNDECIDED says that the tile held one.
 *
 * terra_collide_in is read at the call; its pointers are device pointers for the _dev forms and host pointers otherwise.  Per tile: stats [n] (mzmin, mzmax),
 * trmax [n] and tile_zmax [n] (optional) as for terra_tiles_terrain_view (no tile_zmax: get_tile_zmax() is mzmax), flags [n] bytes (optional): TERRA_COLL_TILE_DISTANT
 * (is_distant), TERRA_COLL_TILE_NO_SCENERY (!scenery.generated).  The three record arrays [n][capacity] with counts [n] as the placements and the brush keep them; a
 * count above the capacity means the first `capacity` records; a container with NULL records or counts or capacity 0 is absent everywhere.  trunk_override
 * [n][pine_capacity] and radius_override [n][scenery_capacity] (optional).  The instance table and terra_tree_size_params are the context's, as for
 * terra_tiles_tree_view; tree_depth_scale as in terra_tree_view_args.  tree_data [num_tree_data] with br_scale [num_tree_data] (tree_data_t::br_scale; the struct
 * keeps its layout), required with the deciduous records; num_tree_data must be terra_decid_params.num_shared_trees.
 * A query: pos, radius, tile, flags (TERRA_COLL_INC_*).  tile = -1: the tile is looked up from pos (tile_draw_t's form); tile >= 0: that batch index
 * (tile_t's form, the analogue of line_tile).  A tile outside [-1, n) is answered as no tile.  A query with a non-finite member or a negative radius is a bad
 * query: its pos comes back unchanged and nothing is read for it.  The kernels index nothing with a query's tile, a looked-up tile or a record's tree_id / inst
 * before its range is known.
 * A hit record: pos as the reference leaves it; tile: the batch index used or -1; word: TERRA_COLL_HIT_PINE / _DECID / _SCENERY (the container reported a
 * collision), TERRA_COLL_ROCK_SHAPE_UNDECIDED, and in TERRA_COLL_STAGE_MASK where the query left: _TESTED (it reached the containers), _NO_TILE, _DISTANT,
 * _OUTSIDE (contains_point failed), _ABOVE (pos.z > get_tile_zmax() + radius), _BAD_QUERY; nhits: the number of objects that moved the centre.
 * The cube call: cubes [nq][6] = x1 x2 y1 y2 z1 z2 in camera space, cube_tile [nq] or NULL (as a query's tile; NULL: every tile from the cube's centre),
 * result [nq] bytes: TERRA_CUBE_INT_HIT, TERRA_CUBE_INT_NO_TILE, TERRA_CUBE_INT_BAD_QUERY (a non-finite bound); tile_out [nq] (optional): the batch index or -1.
 * It reads the deciduous members of terra_collide_in alone (with dxoff / dyoff and dtree_xoff2 / dtree_yoff2).
 *
 * TERRA_ERR_ARG, with nothing written: a NULL required pointer (in; tile_xy and stats when n > 0; queries / cubes and hits / result when nq > 0; tree_data and
 * br_scale with deciduous records); a pointer other than flags and result that is not 4-byte aligned; tree_depth_scale not finite and > 0; num_tree_data other than
 * num_shared_trees when there are deciduous records; `instanced` with an instance table of another length; an unsupported S; n*capacity beyond 32 bits; a tile
 * that appears twice.  TERRA_ERR_STATE before terra_init_scene.  n == 0 or nq == 0 does nothing once the checks have passed.  The device forms only enqueue and read
 * nothing back; tile_xy is a host array in both forms (the key table of the batch is built from it and searched on the device).  Scratch comes from the context's arena. */
typedef struct terra_collide_in {
	const terra_tile_stats *stats;
	const float *trmax, *tile_zmax;
	const uint8_t *flags;
	const terra_tree_place *pine;       const uint32_t *pine_counts;    const terra_trunk_override *trunk_override;
	const terra_decid_place *decid;     const uint32_t *decid_counts;
	const terra_scenery_place *scenery; const uint32_t *scenery_counts; const float *radius_override;
	const terra_decid_tree_data *tree_data; const float *br_scale;
	uint32_t pine_capacity, decid_capacity, scenery_capacity, num_tree_data;
	int32_t dxoff, dyoff;               /* xoff - xoff2, yoff - yoff2 */
	int32_t ptree_xoff2, ptree_yoff2, dtree_xoff2, dtree_yoff2, scenery_xoff2, scenery_yoff2; /* what the three placements ran with */
	float tree_depth_scale;
	uint32_t pad;
} terra_collide_in;          /* 168 bytes */
typedef struct terra_sphere_query {float pos[3], radius; int32_t tile; uint32_t flags;} terra_sphere_query;    /* 24 bytes */
typedef struct terra_sphere_hit {float pos[3]; int32_t tile; uint32_t word, nhits;} terra_sphere_hit;          /* 24 bytes */
enum {TERRA_COLL_INC_DTREES = 1, TERRA_COLL_INC_PTREES = 2, TERRA_COLL_INC_SCENERY = 4, TERRA_COLL_INC_ALL = 7};
enum {TERRA_COLL_TILE_DISTANT = 1, TERRA_COLL_TILE_NO_SCENERY = 2};
enum {TERRA_COLL_HIT_PINE = 1, TERRA_COLL_HIT_DECID = 2, TERRA_COLL_HIT_SCENERY = 4, TERRA_COLL_ROCK_SHAPE_UNDECIDED = 8, TERRA_COLL_STAGE_SHIFT = 8,
      TERRA_COLL_STAGE_MASK = 0xF00, TERRA_COLL_STAGE_TESTED = 0, TERRA_COLL_STAGE_NO_TILE = 1, TERRA_COLL_STAGE_DISTANT = 2, TERRA_COLL_STAGE_OUTSIDE = 3,
      TERRA_COLL_STAGE_ABOVE = 4, TERRA_COLL_STAGE_BAD_QUERY = 5};
enum {TERRA_CUBE_INT_HIT = 1, TERRA_CUBE_INT_NO_TILE = 2, TERRA_CUBE_INT_BAD_QUERY = 4};
int  terra_tiles_sphere_collide_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const terra_sphere_query *d_queries, uint32_t nq,
                                    terra_sphere_hit *d_hits);
int  terra_tiles_sphere_collide(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const terra_sphere_query *h_queries, uint32_t nq,
                                terra_sphere_hit *h_hits);
int  terra_tiles_cube_int_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const float *d_cubes, const int32_t *d_cube_tile,
                                    uint32_t nq, uint8_t *d_result, int32_t *d_tile_out);
int  terra_tiles_cube_int_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const float *h_cubes, const int32_t *h_cube_tile,
                                uint32_t nq, uint8_t *h_result, int32_t *h_tile_out);


/* ---- plumbing for callers without a HIP runtime of their own (tests, ctypes) */
int  terra_malloc(terra_ctx *ctx, void **d_ptr, size_t bytes);
int  terra_free(terra_ctx *ctx, void *d_ptr);
int  terra_memcpy_h2d(terra_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);   /* synchronous */
int  terra_memcpy_d2h(terra_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);   /* synchronous */
/* timing on the context's stream (HIP events): t0 = terra_timer_start; ... ; ms = terra_timer_stop (synchronises) */
int  terra_timer_start(terra_ctx *ctx);
int  terra_timer_stop(terra_ctx *ctx, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* TERRA_H */
