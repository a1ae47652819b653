// terra_api_impl.hpp -- the extern "C" entry points of include/terra.h, written once over terra_engine<BACKEND>.
// Included by exactly one translation unit per library after it has defined `terra_backend_t`:
//   3dworld_amd/csrc/terra_hip.hip  -> libterra_hip.so  (product, HIP/gfx950)
//   tests/emul/terra_emul.cpp       -> tests/emul/libterra_emul.so (test-only host emulation of the kernel bodies)
#pragma once
#include "terra_driver.hpp"
#include "terra_png.hpp"
#include <new>
#include <mutex>
#include <atomic>

namespace terra {
static thread_local std::string g_last_error;
inline int fail(int code, char const *what) {g_last_error = what ? what : "unknown error"; return code;}
} // namespace terra

struct terra_ctx {
	terra::terra_engine<terra_backend_t> eng;
	// A context is driven by one host thread at a time (include/terra.h).  The exception is the generator handle: eval_index is const in the reference and is called
	// from its OpenMP workers (src/tiled_mesh.cpp:495, src/heightmap.cpp:139), and several handles share the context's engine (grow-only scratch, stream, the sine-table
	// upload): every terra_gen_* call that touches the engine takes this lock, so handles of one context may be used from several threads
	std::recursive_mutex eng_mtx;
};

struct terra_gen { // mesh_xy_grid_cache_t (src/mesh.h:22-45)
	terra_ctx *ctx = nullptr;
	float x0 = 0, y0 = 0, dx = 0, dy = 0;
	uint32_t nx = 0, ny = 0, flags = 0;
	bool built = false, running = false, glaciated = false;
	std::atomic<bool> collected{false}; // release-stored after cached_vals is filled: eval_index's fast path reads the grid without the lock once this is set
	float *d_vals = nullptr; size_t d_count = 0;
	std::vector<float> cached_vals;
	// eval_index(x, y, min_start_sin): the sine sum starts at max(start_eval_sin, min_start_sin) (src/mesh_gen.cpp:770); the device grid was evaluated with
	// kstart; a caller that asks for another first term gets a grid evaluated with that one (one more launch, kept per first term)
	int kstart = 0, sev = 0, gen_mode = 0;
	std::map<int, std::vector<float>> alt_vals;
	std::mutex mtx; // eval_index is const in the reference and called from its OpenMP workers (src/tiled_mesh.cpp:495, src/heightmap.cpp:139): the handle's own state (lazy read-back, alternative
	                // first terms) is serialised by this lock, the shared engine of the context by terra_ctx::eng_mtx
};

#define TERRA_TRY   try {
#define TERRA_CATCH } catch (std::invalid_argument const &e) {return terra::fail(TERRA_ERR_ARG, e.what());} \
                      catch (std::logic_error const &e) {return terra::fail(TERRA_ERR_STATE, e.what());} \
                      catch (std::bad_alloc const &) {return terra::fail(TERRA_ERR_LIMIT, "out of memory");} \
                      catch (std::exception const &e) {return terra::fail(TERRA_ERR_HIP, e.what());} \
                      return TERRA_OK;
#define TERRA_CHECK_CTX if (!ctx) return terra::fail(TERRA_ERR_ARG, "null terra_ctx");
typedef terra::host_stage_t<terra::terra_engine<terra_backend_t>> terra_stage; // the device copies of a host-pointer entry point's arrays (terra_stage.hpp)

extern "C" {

const char *terra_last_error(void) {return terra::g_last_error.c_str();}
int terra_device_count(void) {return terra_backend_t::device_count();}

int terra_create(terra_ctx **out, int device_index) {
	if (!out) return terra::fail(TERRA_ERR_ARG, "terra_create: null out pointer");
	*out = nullptr;
	int const ndev = terra_backend_t::device_count();
	if (ndev <= 0) return terra::fail(TERRA_ERR_NODEVICE, "terra_create: no usable HIP device (libterra_hip has no CPU fall-back)");
	if (device_index < 0 || device_index >= ndev) return terra::fail(TERRA_ERR_ARG, "terra_create: device index out of range");
	TERRA_TRY
		terra_ctx *c = new terra_ctx();
		try {c->eng.be.init(device_index);} catch (...) {delete c; throw;}
		*out = c;
	TERRA_CATCH
}
void terra_destroy(terra_ctx *ctx) {if (ctx) {try {ctx->eng.be.download_wait();} catch (...) {} try {ctx->eng.be.sync();} catch (...) {} delete ctx;}} // (a pending terra_download_async still reads device scratch)
int terra_set_stream(terra_ctx *ctx, void *s) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.set_stream(s); TERRA_CATCH}
int terra_release_scratch(terra_ctx *ctx) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.download_wait(); ctx->eng.release_scratch(); TERRA_CATCH}
int terra_synchronize(terra_ctx *ctx) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.sync(); TERRA_CATCH}
int terra_set_option(terra_ctx *ctx, const char *key, const char *value) {
	TERRA_CHECK_CTX if (!key || !value) return terra::fail(TERRA_ERR_ARG, "terra_set_option: null key / value");
	TERRA_TRY std::lock_guard<std::recursive_mutex> lk(ctx->eng_mtx); ctx->eng.set_option(key, value); TERRA_CATCH
}
void *terra_host_alloc(size_t bytes) {void *p = terra_backend_t::host_alloc(bytes); if (!p) {terra::fail(TERRA_ERR_HIP, "terra_host_alloc: out of pinned host memory");} return p;}
void terra_host_free(void *p) {terra_backend_t::host_free(p);}
int terra_download_async(terra_ctx *ctx, const void *d_src, void *h_dst, size_t bytes) {
	TERRA_CHECK_CTX if (!d_src || !h_dst) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.be.download_async(d_src, h_dst, bytes); TERRA_CATCH
}
int terra_download_wait(terra_ctx *ctx) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.download_wait(); TERRA_CATCH}

// ---- events: stream-level ordering between contexts
struct terra_event {void *ev = nullptr;};
int terra_event_create(terra_ctx *ctx, terra_event **out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null out");
	*out = nullptr;
	TERRA_TRY terra_event *e = new terra_event(); try {e->ev = ctx->eng.be.event_create();} catch (...) {delete e; throw;} *out = e; TERRA_CATCH
}
int terra_event_record(terra_ctx *ctx, terra_event *ev) {TERRA_CHECK_CTX if (!ev) return terra::fail(TERRA_ERR_ARG, "null event"); TERRA_TRY ctx->eng.be.event_record(ev->ev); TERRA_CATCH}
int terra_event_synchronize(terra_event *ev) {if (!ev) return terra::fail(TERRA_ERR_ARG, "null event"); TERRA_TRY terra_backend_t::event_synchronize(ev->ev); TERRA_CATCH}
int terra_event_wait(terra_ctx *ctx, terra_event *ev) {TERRA_CHECK_CTX if (!ev) return terra::fail(TERRA_ERR_ARG, "null event"); TERRA_TRY ctx->eng.be.event_wait(ev->ev); TERRA_CATCH}
void terra_event_destroy(terra_event *ev) {if (ev) {terra_backend_t::event_destroy(ev->ev); delete ev;}}

int terra_init_scene(terra_ctx *ctx, const terra_config *cfg) {
	TERRA_CHECK_CTX
	if (!cfg) return terra::fail(TERRA_ERR_ARG, "terra_init_scene: null config");
	TERRA_TRY ctx->eng.init_scene(*cfg); TERRA_CATCH
}
int terra_set_config(terra_ctx *ctx, const terra_config *cfg) {
	TERRA_CHECK_CTX
	if (!cfg) return terra::fail(TERRA_ERR_ARG, "terra_set_config: null config");
	TERRA_TRY ctx->eng.set_config(*cfg); TERRA_CATCH
}
int terra_get_state(terra_ctx *ctx, terra_state *out) {TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null out"); TERRA_TRY ctx->eng.require_scene(); ctx->eng.get_state(*out); TERRA_CATCH}
int terra_set_state(terra_ctx *ctx, const terra_state *in) {TERRA_CHECK_CTX if (!in) return terra::fail(TERRA_ERR_ARG, "null state"); TERRA_TRY ctx->eng.set_state(*in); TERRA_CATCH}
int terra_set_mode(terra_ctx *ctx, int mode, int shape) {
	TERRA_CHECK_CTX
	if (mode < 0 || mode > TERRA_MGEN_DWARP_GPU || shape < 0 || shape > 2) return terra::fail(TERRA_ERR_ARG, "terra_set_mode: bad mode/shape");
	ctx->eng.mode = mode; ctx->eng.shape = shape; return TERRA_OK;
}
int terra_set_zmax_est(terra_ctx *ctx, float v) {TERRA_CHECK_CTX ctx->eng.set_zmax_est(v); ctx->eng.set_zvals(); return TERRA_OK;}
int terra_set_water_plane_z(terra_ctx *ctx, float v) {TERRA_CHECK_CTX ctx->eng.water_plane_z = v; return TERRA_OK;}
int terra_set_start_eval_sin(terra_ctx *ctx, int v) {
	TERRA_CHECK_CTX
	if (v < 0 || v > TERRA_F_TABLE_SIZE) return terra::fail(TERRA_ERR_ARG, "start_eval_sin out of range"); // assert(start_eval_sin <= F_TABLE_SIZE), src/mesh_gen.cpp:590
	ctx->eng.start_eval_sin = v; return TERRA_OK;
}
int terra_set_erode_amount(terra_ctx *ctx, float v) {TERRA_CHECK_CTX ctx->eng.erode_amount = v; return TERRA_OK;}
float terra_get_max_sea_level(terra_ctx *ctx) {return ctx ? ctx->eng.get_max_sea_level() : 0.0f;}

// ---- generator handle
int terra_gen_create(terra_ctx *ctx, terra_gen **out) {
	TERRA_CHECK_CTX
	if (!out) return terra::fail(TERRA_ERR_ARG, "null out");
	TERRA_TRY *out = new terra_gen(); (*out)->ctx = ctx; TERRA_CATCH
}
void terra_gen_destroy(terra_gen *g) {
	if (!g) return;
	try {if (g->d_vals) {std::lock_guard<std::recursive_mutex> eng_lock(g->ctx->eng_mtx); g->ctx->eng.be.sync(); g->ctx->eng.be.free(g->d_vals);}} catch (...) {}
	delete g;
}
static void terra_gen_do_collect(terra_gen *g) { // caller holds g->mtx
	if (g->collected.load(std::memory_order_acquire)) return;
	std::lock_guard<std::recursive_mutex> eng_lock(g->ctx->eng_mtx);
	g->cached_vals.resize((size_t)g->nx*g->ny);
	g->ctx->eng.be.d2h(g->cached_vals.data(), g->d_vals, g->cached_vals.size()*sizeof(float)); // blocks on the stream, like read_float_vals (src/shaders.cpp:1196-1235)
	g->running = false; g->collected.store(true, std::memory_order_release);
}
int terra_gen_build_arrays(terra_gen *g, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin) {
	if (!g) return terra::fail(TERRA_ERR_ARG, "null terra_gen");
	try {
		std::lock_guard<std::mutex> lock(g->mtx);
		std::lock_guard<std::recursive_mutex> eng_lock(g->ctx->eng_mtx);
		bool const no_wait = (flags & TERRA_GEN_NO_WAIT) != 0;
		uint32_t const key = flags & (TERRA_GEN_GLACIATE | TERRA_GEN_FORCE_SINE | TERRA_GEN_FUSED | TERRA_GEN_FAST);
		int const sev = g->ctx->eng.start_eval_sin, kstart = terra::imax(sev, min_start_sin);
		bool const same = g->built && g->x0 == x0 && g->y0 == y0 && g->dx == dx && g->dy == dy && g->nx == nx && g->ny == ny && (g->flags & (TERRA_GEN_GLACIATE | TERRA_GEN_FORCE_SINE | TERRA_GEN_FUSED | TERRA_GEN_FAST)) == key && g->kstart == kstart;
		bool const was_running = g->running && same;
		if (!was_running) { // launch the job (run_gpu_simplex, src/mesh_gen.cpp:652-681)
			size_t const count = (size_t)nx*ny;
			if (count == 0) return terra::fail(TERRA_ERR_ARG, "build_arrays: nx, ny must be > 0");
			g->collected.store(false, std::memory_order_release); // before the geometry changes: eval_index's lock-free path is only valid while this is set
			if (count > g->d_count) {if (g->d_vals) {g->ctx->eng.be.sync(); g->ctx->eng.be.free(g->d_vals);} g->d_vals = (float *)g->ctx->eng.be.alloc(count*sizeof(float)); g->d_count = count;}
			g->x0 = x0; g->y0 = y0; g->dx = dx; g->dy = dy; g->nx = nx; g->ny = ny; g->flags = flags;
			g->ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, g->d_vals);
			g->built = true; g->running = true; g->collected.store(false, std::memory_order_release); g->glaciated = (flags & TERRA_GEN_GLACIATE) != 0;
			g->kstart = kstart; g->sev = sev; g->gen_mode = (flags & TERRA_GEN_FORCE_SINE) ? (int)terra::MGEN_SINE : g->ctx->eng.mode;
			g->cached_vals.clear(); g->alt_vals.clear();
		}
		if (no_wait && !was_running) return 0; // just started, results not yet available
		terra_gen_do_collect(g);
		return 1;
	}
	catch (std::invalid_argument const &e) {return terra::fail(TERRA_ERR_ARG, e.what());}
	catch (std::logic_error const &e) {return terra::fail(TERRA_ERR_STATE, e.what());}
	catch (std::exception const &e) {return terra::fail(TERRA_ERR_HIP, e.what());}
}
int terra_gen_enable_glaciate(terra_gen *g) {
	if (!g) return terra::fail(TERRA_ERR_ARG, "null terra_gen");
	TERRA_TRY
		std::lock_guard<std::mutex> lock(g->mtx); // the handle's state is read under its lock: a build_arrays on another thread may be rewriting it
		if (!g->built) throw std::logic_error("enable_glaciate: build_arrays() must have been called first"); // assert(cur_nx > 0 && cur_ny > 0), src/mesh_gen.cpp:644
		if (g->glaciated) return TERRA_OK;
		std::lock_guard<std::recursive_mutex> eng_lock(g->ctx->eng_mtx);
		// not fused at build time: re-evaluate with the glaciate epilogue (pure per-cell function, identical values)
		g->ctx->eng.gen_grid_dev(g->x0, g->y0, g->dx, g->dy, g->nx, g->ny, g->flags | TERRA_GEN_GLACIATE, g->kstart, g->d_vals);
		g->flags |= TERRA_GEN_GLACIATE; g->glaciated = true; g->running = true; g->collected.store(false, std::memory_order_release); g->alt_vals.clear();
	TERRA_CATCH
}
int terra_gen_is_running(terra_gen *g) {return (g && g->running) ? 1 : 0;}
int terra_gen_collect(terra_gen *g, float *host_out) {
	if (!g || !host_out) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		std::lock_guard<std::mutex> lock(g->mtx);
		if (!g->built) throw std::logic_error("collect: nothing was built");
		terra_gen_do_collect(g); memcpy(host_out, g->cached_vals.data(), g->cached_vals.size()*sizeof(float));
	TERRA_CATCH
}
float terra_gen_eval_index(terra_gen *g, uint32_t x, uint32_t y, int min_start_sin, int use_cache) {
	if (!g) {terra::fail(TERRA_ERR_ARG, "eval_index: null terra_gen"); return 0.0f;}
	try {
		// fast path, lock-free: the reference's OpenMP workers all call eval_index on one collected grid (src/tiled_mesh.cpp:495, src/heightmap.cpp:139).  Once `collected`
		// is set (release) the handle's geometry and cached_vals do not change until the next build_arrays, which the caller must not overlap with eval_index on the
		// same handle (the reference's build_arrays is main-thread only, src/mesh.h:40) -- concurrent builds of OTHER handles are fine
		if (g->collected.load(std::memory_order_acquire)) {
			int const want0 = (g->gen_mode == (int)terra::MGEN_SINE) ? ((use_cache && (g->flags & TERRA_GEN_CACHE_VALUES)) ? g->sev : terra::imax(g->sev, min_start_sin)) : g->kstart;
			if (want0 == g->kstart) {
				if (x >= g->nx || y >= g->ny) {terra::fail(TERRA_ERR_ARG, "eval_index: out of range"); return 0.0f;}
				return g->cached_vals[(size_t)y*g->nx + x];
			}
		}
		std::lock_guard<std::mutex> lock(g->mtx);
		if (!g->built || x >= g->nx || y >= g->ny) {terra::fail(TERRA_ERR_ARG, "eval_index: out of range"); return 0.0f;} // assert(x < cur_nx && y < cur_ny), src/mesh_gen.cpp:756
		// which first sine term the reference would use (src/mesh_gen.cpp:759-770): cached values (cache_values at build time, filled with min_start_sin = 0)
		// win when use_cache is set; the fBm modes have no sine terms
		int want = g->kstart;
		if (g->gen_mode == (int)terra::MGEN_SINE) {want = (use_cache && (g->flags & TERRA_GEN_CACHE_VALUES)) ? g->sev : terra::imax(g->sev, min_start_sin);}
		if (want == g->kstart) {terra_gen_do_collect(g); return g->cached_vals[(size_t)y*g->nx + x];}
		std::vector<float> &alt = g->alt_vals[want];
		if (alt.empty()) { // same grid from another first term: one more launch, kept for the following calls
			std::lock_guard<std::recursive_mutex> eng_lock(g->ctx->eng_mtx);
			terra_backend_t &be = g->ctx->eng.be;
			size_t const count = (size_t)g->nx*g->ny;
			float *d = (float *)be.alloc(count*sizeof(float));
			std::vector<float> tmp(count);
			try {
				g->ctx->eng.gen_grid_dev(g->x0, g->y0, g->dx, g->dy, g->nx, g->ny, g->flags & (TERRA_GEN_GLACIATE | TERRA_GEN_FORCE_SINE | TERRA_GEN_FUSED | TERRA_GEN_FAST), want, d); // first term = max(start_eval_sin, want)
				be.d2h(tmp.data(), d, count*sizeof(float));
			} catch (...) {be.free(d); g->alt_vals.erase(want); throw;}
			be.free(d);
			alt.swap(tmp);
		}
		return alt[(size_t)y*g->nx + x];
	}
	catch (std::exception const &e) {terra::fail(TERRA_ERR_HIP, e.what()); return 0.0f;}
}
const float *terra_gen_device_values(terra_gen *g) {return (g && g->built) ? g->d_vals : nullptr;}

int terra_gen_grid_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out) {
	TERRA_CHECK_CTX if (!d_out) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out); TERRA_CATCH
}
int terra_gen_grid_minmax_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *h_min, float *h_max) {
	TERRA_CHECK_CTX if (!d_out) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY float mm[2]; ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out, mm); if (h_min) *h_min = mm[0]; if (h_max) *h_max = mm[1]; TERRA_CATCH
}
int terra_gen_grid_minmax_async_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *d_minmax) {
	TERRA_CHECK_CTX if (!d_out || !d_minmax) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out, nullptr, 0, 0xFFFFFFFFu, d_minmax); TERRA_CATCH
}
int terra_gen_grid_minmax_turn_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *d_out, float *d_minmax, terra_event *wait_for, terra_event *turn) {
	TERRA_CHECK_CTX if (!d_out || !d_minmax) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY
		terra::noise_turn_t nt;
		nt.wait_for = wait_for ? wait_for->ev : nullptr; nt.record = turn ? turn->ev : nullptr; nt.rows = ctx->eng.turn_rows(ny);
		ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out, nullptr, 0, 0xFFFFFFFFu, d_minmax, &nt);
	TERRA_CATCH
}
int terra_gen_grid_rows_minmax_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, uint32_t row0, uint32_t nrows, float *d_out, float *h_min, float *h_max) {
	TERRA_CHECK_CTX if (!d_out) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY
		float mm[2];
		ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out, (h_min || h_max) ? mm : nullptr, row0, nrows);
		if (h_min) *h_min = mm[0];
		if (h_max) *h_max = mm[1];
	TERRA_CATCH
}
int terra_gen_grid_rows_minmax_async_dev(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, uint32_t row0, uint32_t nrows, float *d_out, float *d_minmax) {
	TERRA_CHECK_CTX if (!d_out || !d_minmax) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, d_out, nullptr, row0, nrows, d_minmax); TERRA_CATCH
}
int terra_gen_grid(terra_ctx *ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, uint32_t flags, int min_start_sin, float *h_out) {
	TERRA_CHECK_CTX if (!h_out) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY
		size_t const bytes = (size_t)nx*ny*sizeof(float);
		if (bytes == 0) throw std::invalid_argument("build_arrays: nx, ny must be > 0");
		terra_stage st(ctx->eng);
		int const o = st.out(h_out, bytes);
		st.begin();
		ctx->eng.gen_grid_dev(x0, y0, dx, dy, nx, ny, flags, min_start_sin, st.dev<float>(o));
		st.end();
	TERRA_CATCH
}

int terra_eval_points(terra_ctx *ctx, const float *xy, uint32_t n, uint32_t kind, float xy_scale, int no_xyoff, int xoff2, int yoff2, float *out) {
	TERRA_CHECK_CTX if (n && (!xy || !out)) return terra::fail(TERRA_ERR_ARG, "terra_eval_points: null pointer");
	TERRA_TRY std::lock_guard<std::recursive_mutex> lk(ctx->eng_mtx); ctx->eng.eval_points(xy, n, kind, xy_scale, no_xyoff, xoff2, yoff2, out); TERRA_CATCH
}
int terra_eval_points_dev(terra_ctx *ctx, const float *d_xy, uint32_t n, uint32_t kind, float xy_scale, int no_xyoff, int xoff2, int yoff2, float *d_out) {
	TERRA_CHECK_CTX if (n && (!d_xy || !d_out)) return terra::fail(TERRA_ERR_ARG, "terra_eval_points_dev: null pointer");
	TERRA_TRY std::lock_guard<std::recursive_mutex> lk(ctx->eng_mtx); ctx->eng.eval_points_dev(d_xy, n, kind, xy_scale, no_xyoff, xoff2, yoff2, d_out); TERRA_CATCH
}
int terra_eval_mesh_sin_terms(terra_ctx *ctx, float xv, float yv, float *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null out");
	TERRA_TRY *out = ctx->eng.eval_mesh_sin_terms(xv, yv); TERRA_CATCH
}
int terra_glaciate_mesh_dev(terra_ctx *ctx, float *d_mesh, uint32_t nx, uint32_t ny, int xoff2, int yoff2, float *h_zbottom_ztop) {
	TERRA_CHECK_CTX if (!d_mesh) return terra::fail(TERRA_ERR_ARG, "null mesh");
	TERRA_TRY ctx->eng.glaciate_mesh_dev(d_mesh, nx, ny, xoff2, yoff2, h_zbottom_ztop); TERRA_CATCH
}

// ---- erosion
int terra_apply_erosion_dev(terra_ctx *ctx, float *d, int xs, int ys, float min_zval, uint32_t iters, uint32_t flags) {
	TERRA_CHECK_CTX if (!d) return terra::fail(TERRA_ERR_ARG, "null heightmap");
	TERRA_TRY ctx->eng.apply_erosion_dev(d, xs, ys, min_zval, iters, flags); TERRA_CATCH
}
int terra_apply_erosion_devmin_dev(terra_ctx *ctx, float *d, int xs, int ys, const float *d_min_zval, uint32_t iters, uint32_t flags) {
	TERRA_CHECK_CTX if (!d || !d_min_zval) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.apply_erosion_dev(d, xs, ys, 0.0f, iters, flags, d_min_zval); TERRA_CATCH
}
size_t terra_erosion_shard_arena_bytes(terra_ctx *ctx, uint32_t iters) {
	if (!ctx) return 0;
	return ctx->eng.sparse_arena_bytes(iters);
}
int terra_erosion_shard_trace_dev(terra_ctx *ctx, float *d, int xs, int ys, uint32_t iters, uint32_t row0, uint32_t nrows, void *d_arena) {
	TERRA_CHECK_CTX if (!d || !d_arena) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (ys <= 0 || row0 > (uint32_t)ys || nrows > (uint32_t)ys - row0) return terra::fail(TERRA_ERR_ARG, "terra_erosion_shard_trace_dev: rows outside the grid");
	TERRA_TRY
		terra::sparse_shard_t sh{};
		sh.phase = 1; sh.row0 = row0; sh.row1 = row0 + nrows; sh.arena = (uint8_t *)d_arena;
		ctx->eng.apply_erosion_dev(d, xs, ys, 0.0f, iters, 0, nullptr, &sh);
	TERRA_CATCH
}
int terra_erosion_shard_finish_dev(terra_ctx *ctx, float *d, int xs, int ys, const float *d_min_zval, uint32_t iters, uint32_t flags, uint32_t world, uint32_t self, const uint32_t *row_end, void *d_arena_self, size_t arena_stride) {
	TERRA_CHECK_CTX if (!d || !d_min_zval || !row_end || !d_arena_self) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (world == 0 || world > terra::SPARSE_SHARD_MAX_WORLD || self >= world) return terra::fail(TERRA_ERR_ARG, "terra_erosion_shard_finish_dev: world must be 1 .. 16 and self below it");
	if (world > 1 && arena_stride < ctx->eng.sparse_arena_bytes(iters)) return terra::fail(TERRA_ERR_ARG, "terra_erosion_shard_finish_dev: arena_stride is smaller than an arena (terra_erosion_shard_arena_bytes)");
	for (uint32_t r = 0; r < world; ++r) {
		if ((r && row_end[r] < row_end[r - 1]) || (r + 1 == world && (ys <= 0 || row_end[r] != (uint32_t)ys))) return terra::fail(TERRA_ERR_ARG, "terra_erosion_shard_finish_dev: row_end must be non-decreasing and end at ysize");
	}
	TERRA_TRY
		terra::sparse_shard_t sh{};
		sh.phase = 2; sh.arena = (uint8_t *)d_arena_self; sh.world = world; sh.self = self; sh.stride = (long long)arena_stride;
		for (uint32_t r = 0; r < world; ++r) {sh.rows.end[r] = row_end[r];}
		ctx->eng.apply_erosion_dev(d, xs, ys, 0.0f, iters, flags, d_min_zval, &sh);
	TERRA_CATCH
}
int terra_apply_erosion(terra_ctx *ctx, float *h, int xs, int ys, float min_zval, uint32_t iters) {
	TERRA_CHECK_CTX if (!h) return terra::fail(TERRA_ERR_ARG, "null heightmap");
	TERRA_TRY
		if (iters == 0 || ctx->eng.erode_amount <= 0.0f) return TERRA_OK;
		if (xs <= 0 || ys <= 0) throw std::invalid_argument("apply_erosion: bad grid size");
		size_t const bytes = (size_t)xs*ys*sizeof(float);
		terra_stage st(ctx->eng); // grow-only (a 1 GiB hipMalloc + hipFree per call cost more than the erosion)
		int const g = st.inout(h, bytes);
		st.begin();
		ctx->eng.apply_erosion_dev(st.dev<float>(g), xs, ys, min_zval, iters, 0);
		st.end();
	TERRA_CATCH
}
int terra_set_erosion_tuning(terra_ctx *ctx, uint32_t window, uint32_t cap_log2, uint32_t maxb) {
	TERRA_CHECK_CTX
	if ((cap_log2 && (cap_log2 < 12 || cap_log2 > 20)) || (maxb && (maxb < 8 || maxb > 65536)) || (window > (1u << 20) && window != 0xFFFFFFFFu)) return terra::fail(TERRA_ERR_ARG, "terra_set_erosion_tuning: value out of range");
	if (window) ctx->eng.spec_cfg.window = (window == 0xFFFFFFFFu) ? 0 : window; // 0xFFFFFFFF: back to the automatic choice
	(void)cap_log2; // versions are stored as one 64-float page per footprint block since round 2: there is no hashed log to size any more (accepted for compatibility)
	if (maxb) ctx->eng.spec_cfg.maxb = maxb;
	return TERRA_OK;
}
int terra_set_erosion_slice_steps(terra_ctx *ctx, uint32_t steps) {
	TERRA_CHECK_CTX
	if (steps == 0) return terra::fail(TERRA_ERR_ARG, "terra_set_erosion_slice_steps: steps must be > 0");
	ctx->eng.spec_cfg.slice_steps = steps;
	return TERRA_OK;
}
int terra_get_erosion_report(terra_ctx *ctx, terra_erosion_report *out) {TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null out"); *out = ctx->eng.report; return TERRA_OK;}

// ---- whole heightmap (heightmap_t::proc_gen, src/heightmap.cpp:130-151)
int terra_minmax_dev(terra_ctx *ctx, const float *d, size_t n, float *h_min, float *h_max) {
	TERRA_CHECK_CTX if (!d || n == 0) return terra::fail(TERRA_ERR_ARG, "empty input");
	TERRA_TRY float mn, mx; ctx->eng.minmax_dev(d, n, mn, mx); if (h_min) *h_min = mn; if (h_max) *h_max = mx; TERRA_CATCH
}
int terra_quantize16_dev(terra_ctx *ctx, const float *d, size_t n, float min_z, float dz, uint8_t *d_pix) {
	TERRA_CHECK_CTX if (!d || !d_pix) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (!(dz > 0.0f)) return terra::fail(TERRA_ERR_ARG, "quantize16: dz must be > 0"); // assert(dz > 0.0), src/mesh_gen.cpp:126
	TERRA_TRY ctx->eng.quantize16_dev(d, n, min_z, dz, d_pix); TERRA_CATCH
}
int terra_heightmap_proc_gen_dev(terra_ctx *ctx, uint32_t width, uint32_t height, uint32_t erosion_iters, float *d_vals, uint8_t *d_pix, float *h_range) {
	TERRA_CHECK_CTX if (!d_vals) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY
		auto &e = ctx->eng;
		size_t const n = (size_t)width*height;
		float mm[2];
		bool const erode = erosion_iters > 0 && e.erode_amount > 0.0f;
		e.gen_grid_dev((float)(-0.5*(double)width), (float)(-0.5*(double)height), e.DX_VAL, e.DY_VAL, width, height, TERRA_GEN_GLACIATE, 0, d_vals, erode ? mm : nullptr); // src/heightmap.cpp:135-143
		if (erode) {e.apply_erosion_dev(d_vals, (int)width, (int)height, mm[0], erosion_iters, TERRA_ERODE_MINZ_IS_MIN);} // run_erosion (src/heightmap.cpp:153-187): min_zval = min(vals)
		if (d_pix || h_range) {
			float mn, mx; e.minmax_dev(d_vals, n, mn, mx); // get_heightmap_z_range
			float const dz = terra::max_std(1.0E-12f, (mx - mn)); // max(TOLERANCE, ...), src/heightmap.cpp:148
			if (h_range) {h_range[0] = mn; h_range[1] = dz;}
			if (d_pix) {e.quantize16_dev(d_vals, n, mn, dz, d_pix);}
		}
	TERRA_CATCH
}

// host form: what heightmap_t::proc_gen leaves in the texture's pixel buffer (src/heightmap.cpp:130-151) -- 2 bytes per cell cross the host link, nothing else
int terra_heightmap_proc_gen(terra_ctx *ctx, uint32_t width, uint32_t height, uint32_t erosion_iters, uint8_t *h_pix, float *h_range) {
	TERRA_CHECK_CTX if (!h_pix) return terra::fail(TERRA_ERR_ARG, "null output");
	if (width == 0 || height == 0) return terra::fail(TERRA_ERR_ARG, "terra_heightmap_proc_gen: empty map");
	TERRA_TRY
		size_t const n = (size_t)width*height;
		terra_stage st(ctx->eng);
		int const v = st.temp(n*4), p = st.out(h_pix, n*2); // floats, then the 16-bit pixels
		st.begin();
		int const rc = terra_heightmap_proc_gen_dev(ctx, width, height, erosion_iters, st.dev<float>(v), st.dev<uint8_t>(p), h_range);
		if (rc != TERRA_OK) return rc;
		st.end();
	TERRA_CATCH
}

// ---- the loaded-heightmap path (rest of row a12): heightmap_t::to_floats / from_floats / postprocess_height (src/heightmap.cpp:117-128,191-215)
int terra_set_mesh_file_scale(terra_ctx *ctx, float mesh_file_scale, float mesh_file_tz) {
	TERRA_CHECK_CTX
	if (!(mesh_file_scale != 0.0f) || mesh_file_scale != mesh_file_scale || mesh_file_tz != mesh_file_tz) return terra::fail(TERRA_ERR_ARG, "terra_set_mesh_file_scale: scale must be a non-zero number");
	ctx->eng.mesh_file_scale = mesh_file_scale; ctx->eng.mesh_file_tz = mesh_file_tz;
	return TERRA_OK;
}
int terra_get_mesh_file_scale(terra_ctx *ctx, float *mesh_file_scale, float *mesh_file_tz) {
	TERRA_CHECK_CTX
	if (mesh_file_scale) *mesh_file_scale = ctx->eng.mesh_file_scale;
	if (mesh_file_tz) *mesh_file_tz = ctx->eng.mesh_file_tz;
	return TERRA_OK;
}
static int terra_check_image(uint32_t width, uint32_t height, int ncolors) {
	if (width == 0 || height == 0 || (uint64_t)width*height >= (1ull << 31)) return terra::fail(TERRA_ERR_ARG, "heightmap image: bad size");
	if (ncolors != 1 && ncolors != 2) return terra::fail(TERRA_ERR_ARG, "heightmap image: one or two byte grayscale only");
	return TERRA_OK;
}
int terra_heightmap_to_floats_dev(terra_ctx *ctx, const uint8_t *d_pixels, uint32_t width, uint32_t height, int ncolors, float *d_vals) {
	TERRA_CHECK_CTX if (!d_pixels || !d_vals) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (int const rc = terra_check_image(width, height, ncolors)) return rc;
	TERRA_TRY ctx->eng.heightmap_to_floats_dev(d_pixels, (size_t)width*height, ncolors, d_vals); TERRA_CATCH
}
int terra_heightmap_from_floats_dev(terra_ctx *ctx, const float *d_vals, uint32_t width, uint32_t height, int ncolors, uint8_t *d_pixels, uint32_t *h_out_of_range) {
	TERRA_CHECK_CTX if (!d_pixels || !d_vals) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (int const rc = terra_check_image(width, height, ncolors)) return rc;
	TERRA_TRY
		uint32_t const bad = ctx->eng.heightmap_from_floats_dev(d_vals, (size_t)width*height, ncolors, d_pixels);
		if (h_out_of_range) {*h_out_of_range = bad;}
		else if (bad) throw std::logic_error("heightmap from_floats: values outside [0, 256) pixel units (the reference asserts, src/heightmap.cpp:210)");
	TERRA_CATCH
}
int terra_heightmap_postprocess_dev(terra_ctx *ctx, uint8_t *d_pixels, uint32_t width, uint32_t height, int ncolors, uint32_t erosion_iters_tt, float *d_vals, uint32_t *h_out_of_range) {
	TERRA_CHECK_CTX if (!d_pixels) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (int const rc = terra_check_image(width, height, ncolors)) return rc;
	TERRA_TRY
		auto &be = ctx->eng.be;
		float *vals = d_vals;
		if (!vals && erosion_iters_tt) {vals = (float *)be.alloc((size_t)width*height*sizeof(float));}
		uint32_t bad = 0;
		try {bad = ctx->eng.heightmap_postprocess_dev(d_pixels, width, height, ncolors, erosion_iters_tt, vals); if (!d_vals) {be.sync();}} catch (...) {if (!d_vals && vals) be.free(vals); throw;}
		if (!d_vals && vals) {be.free(vals);}
		if (h_out_of_range) {*h_out_of_range = bad;}
		else if (bad) throw std::logic_error("heightmap postprocess_height: eroded values outside [0, 256) pixel units (the reference asserts, src/heightmap.cpp:210)");
	TERRA_CATCH
}

// ---- heightmap files (host): 8- / 16-bit grayscale PNG with the reference's row order and byte order (terra_png.hpp)
int terra_heightmap_write_png(const char *path, const uint8_t *h_pixels, uint32_t width, uint32_t height, int ncolors) {
	if (!path || !h_pixels) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY terra::png_write_gray(path, h_pixels, width, height, ncolors); TERRA_CATCH
}
int terra_heightmap_read_png(const char *path, int allow_two_byte_grayscale, uint32_t *width, uint32_t *height, int *ncolors, uint8_t *h_pixels, size_t capacity) {
	if (!path || !width || !height || !ncolors) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		std::vector<uint8_t> const px = terra::png_read_gray(path, *width, *height, *ncolors, allow_two_byte_grayscale != 0);
		if (h_pixels) {
			if (capacity < px.size()) return terra::fail(TERRA_ERR_ARG, "terra_heightmap_read_png: buffer too small");
			memcpy(h_pixels, px.data(), px.size());
		}
	TERRA_CATCH
}

// ---- the ground mesh's text file (host): read_mesh / write_mesh, src/mesh_gen.cpp:895-965
int terra_read_mesh(terra_ctx *ctx, const char *filename, float zmm, float *h_mesh, uint32_t nx, uint32_t ny, float *h_zbottom_ztop) {
	TERRA_CHECK_CTX
	if (!filename || !h_mesh || nx == 0 || ny == 0) return terra::fail(TERRA_ERR_ARG, "terra_read_mesh: null or empty argument");
	FILE *fp = fopen(filename, "r");
	if (!fp) return terra::fail(TERRA_ERR_ARG, (std::string("terra_read_mesh: cannot open ") + filename).c_str());
	int xsize = 0, ysize = 0;
	if (fscanf(fp, "%i%i", &xsize, &ysize) != 2) {fclose(fp); return terra::fail(TERRA_ERR_ARG, "terra_read_mesh: error reading the size header");}
	if (xsize != (int)nx || ysize != (int)ny) {fclose(fp); return terra::fail(TERRA_ERR_ARG, "terra_read_mesh: the mesh size in the file is not the scene's");}
	float const fscale = ctx->eng.mesh_file_scale, ftz = ctx->eng.mesh_file_tz;
	for (size_t i = 0; i < (size_t)nx*ny; ++i) {
		float height;
		if (fscanf(fp, "%f", &height) != 1) {fclose(fp); return terra::fail(TERRA_ERR_ARG, "terra_read_mesh: error reading mesh heights");}
		h_mesh[i] = fscale*height + ftz;
	}
	fclose(fp);
	float mn = h_mesh[0], mx = h_mesh[0]; // matrix_min_max (src/mesh_gen.cpp:84-94): std::min / std::max, so a NaN never replaces a number
	for (size_t i = 0; i < (size_t)nx*ny; ++i) {float const v = h_mesh[i]; mn = (v < mn) ? v : mn; mx = (mx < v) ? v : mx;}
	if (h_zbottom_ztop) {h_zbottom_ztop[0] = mn; h_zbottom_ztop[1] = mx;}
	float const neg = -mn;
	ctx->eng.set_zmax_est((zmm != 0.0f) ? zmm : ((neg < mx) ? mx : neg)); // max(-zmin, zmax)
	ctx->eng.set_zvals();
	return TERRA_OK;
}
int terra_write_mesh(const char *filename, const float *h_mesh, uint32_t nx, uint32_t ny) {
	if (!filename || !h_mesh) return terra::fail(TERRA_ERR_ARG, "terra_write_mesh: null argument");
	FILE *fp = fopen(filename, "w");
	if (!fp) return terra::fail(TERRA_ERR_ARG, (std::string("terra_write_mesh: cannot open ") + filename).c_str());
	bool ok = fprintf(fp, "%i %i\n", (int)nx, (int)ny) > 0;
	for (uint32_t i = 0; i < ny && ok; ++i) {
		for (uint32_t j = 0; j < nx && ok; ++j) {ok = fprintf(fp, "%f ", (double)h_mesh[(size_t)i*nx + j]) > 0;}
		ok = ok && fprintf(fp, "\n") > 0;
	}
	ok = (fclose(fp) == 0) && ok;
	return ok ? TERRA_OK : terra::fail(TERRA_ERR_ARG, "terra_write_mesh: write error");
}

// ---- tiles
int terra_hmap_set_dev(terra_ctx *ctx, const uint8_t *d_pixels, int width, int height, int ncolors) {
	TERRA_CHECK_CTX
	if (d_pixels && (width <= 0 || height <= 0 || (ncolors != 1 && ncolors != 2) || (int64_t)width*height >= (1ll << 31))) return terra::fail(TERRA_ERR_ARG, "terra_hmap_set_dev: bad image shape");
	if (d_pixels && ncolors == 2 && ((uintptr_t)d_pixels & 1u)) return terra::fail(TERRA_ERR_ARG, "terra_hmap_set_dev: a 16-bit image must be 2-byte aligned"); // the edit kernels update a texel inside its aligned 32-bit word
	ctx->eng.hmap_pix = d_pixels; ctx->eng.hmap_w = d_pixels ? width : 0; ctx->eng.hmap_h = d_pixels ? height : 0; ctx->eng.hmap_nc = d_pixels ? ncolors : 0;
	return TERRA_OK;
}
int terra_set_mesh_height_scales_for_zval_range(terra_ctx *ctx, float min_z, float dz) {
	TERRA_CHECK_CTX
	TERRA_TRY ctx->eng.set_mesh_height_scales_for_zval_range(min_z, dz); TERRA_CATCH
}
int terra_set_tiled_mesh_ao(terra_ctx *ctx, int enable) {TERRA_CHECK_CTX ctx->eng.tiled_mesh_ao = (enable != 0); return TERRA_OK;}
// ---- height edits, the .mod file and the map exporter (rest of row f4)
static_assert(sizeof(terra_hmap_brush) == sizeof(terra::hmap_brush_pod_t) && sizeof(terra_hmap_mod) == sizeof(terra::hmap_mod_pod_t), "mod record layouts");
int terra_hmap_apply_brushes_dev(terra_ctx *ctx, const terra_hmap_brush *brushes, uint32_t n, int step_sz, uint32_t num_steps) {
	TERRA_CHECK_CTX if (n && !brushes) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.hmap_apply_brushes_dev((terra::hmap_brush_pod_t const *)brushes, n, step_sz, num_steps); ctx->eng.be.sync(); TERRA_CATCH
}
int terra_hmap_apply_mods_dev(terra_ctx *ctx, const terra_hmap_mod *mods, uint32_t n) {
	TERRA_CHECK_CTX if (n && !mods) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.hmap_apply_mods_dev((terra::hmap_mod_pod_t const *)mods, n); TERRA_CATCH
}
int terra_hmap_read_and_apply_mod_dev(terra_ctx *ctx, const char *path) {
	TERRA_CHECK_CTX if (!path) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.hmap_read_and_apply_mod_dev(path); ctx->eng.be.sync(); TERRA_CATCH
}
int terra_hmap_write_mod(const char *path, const terra_hmap_mod *mods, uint32_t n, const terra_hmap_brush *brushes, uint32_t n_brushes) {
	if (!path || (n && !mods) || (n_brushes && !brushes)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY terra::write_mod_file(path, (terra::hmap_mod_pod_t const *)mods, n, (terra::hmap_brush_pod_t const *)brushes, n_brushes); TERRA_CATCH
}
int terra_hmap_read_mod(const char *path, terra_hmap_mod *mods, uint32_t mods_capacity, uint32_t *n_mods, terra_hmap_brush *brushes, uint32_t brushes_capacity, uint32_t *n_brushes) {
	if (!path || !n_mods || !n_brushes) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		std::vector<terra::hmap_mod_pod_t> m; std::vector<terra::hmap_brush_pod_t> b;
		terra::read_mod_file(path, m, b);
		*n_mods = (uint32_t)m.size(); *n_brushes = (uint32_t)b.size();
		if (mods) {if (mods_capacity < m.size()) return terra::fail(TERRA_ERR_ARG, "terra_hmap_read_mod: mods buffer too small"); if (!m.empty()) memcpy(mods, m.data(), m.size()*sizeof(terra_hmap_mod));}
		if (brushes) {if (brushes_capacity < b.size()) return terra::fail(TERRA_ERR_ARG, "terra_hmap_read_mod: brushes buffer too small"); if (!b.empty()) memcpy(brushes, b.data(), b.size()*sizeof(terra_hmap_brush));}
	TERRA_CATCH
}
int terra_export_heightmap_dev(terra_ctx *ctx, float xstart, float ystart, uint32_t width, uint32_t height, float *d_vals, uint8_t *d_pixels16, float *h_min_z_dz) {
	TERRA_CHECK_CTX if (!d_vals) return terra::fail(TERRA_ERR_ARG, "null output");
	TERRA_TRY ctx->eng.export_heightmap_dev(xstart, ystart, width, height, d_vals, d_pixels16, h_min_z_dz); ctx->eng.be.sync(); TERRA_CATCH
}
int terra_write_map_mode_heightmap_image(terra_ctx *ctx, const char *path, float xstart, float ystart, uint32_t width, uint32_t height) {
	TERRA_CHECK_CTX if (!path) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		size_t const n = (size_t)width*height;
		if (n == 0) return terra::fail(TERRA_ERR_ARG, "empty image");
		std::vector<uint8_t> px(n*2);
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const v = st.temp(n*4), p = st.out(px.data(), n*2);
		st.begin();
		ctx->eng.export_heightmap_dev(xstart, ystart, width, height, st.dev<float>(v), st.dev<uint8_t>(p), nullptr);
		st.end();
		terra::png_write_gray(path, px.data(), width, height, 2);
	TERRA_CATCH
}
int terra_set_landscape(terra_ctx *ctx, const terra_landscape *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_landscape(*params); TERRA_CATCH
}
int terra_get_landscape(terra_ctx *ctx, terra_landscape *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.ls; return TERRA_OK;
}
int terra_tiles_terrain_params(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, float *h_params) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_params)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_terrain_params(tile_xy, n, h_params); TERRA_CATCH
}
int terra_tiles_create_weights_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, uint8_t *d_weights, terra_grass_block *d_grass_blocks, uint8_t *d_has_any_grass) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals || !d_weights)) return terra::fail(TERRA_ERR_ARG, "null argument");
	static_assert(sizeof(terra_grass_block) == sizeof(terra::grass_block_pod_t), "grass block layout");
	TERRA_TRY ctx->eng.tiles_create_weights_dev(tile_xy, n, d_zvals, d_weights, (terra::grass_block_pod_t *)d_grass_blocks, d_has_any_grass); TERRA_CATCH
}
int terra_tiles_create_weights(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, uint8_t *h_weights, terra_grass_block *h_grass_blocks, uint8_t *h_has_any_grass) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_zvals || !h_weights)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (n == 0) return TERRA_OK;
	TERRA_TRY
		ctx->eng.require_tile_128("tiles_create_weights"); // (before the zvals are read: they are 130^2 floats a tile)
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const z = st.in(h_zvals, (size_t)n*130*130*4), w = st.out(h_weights, (size_t)n*129*129*4), g = st.opt_out(h_grass_blocks, (size_t)n*32*32*sizeof(terra_grass_block)),
			a = st.opt_out(h_has_any_grass, n);
		st.begin();
		ctx->eng.tiles_create_weights_dev(tile_xy, n, st.dev<float>(z), st.dev<uint8_t>(w), st.dev<terra::grass_block_pod_t>(g), st.dev<uint8_t>(a));
		st.end();
	TERRA_CATCH
}
int terra_tiles_edit_grass_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *d_zvals, const terra_tile_stats *d_stats,
                               const uint8_t *d_is_distant, const terra_grass_brush *brush, uint8_t *d_weights, terra_grass_block *d_grass_blocks, uint8_t *d_updated, uint32_t *d_ranges) {
	TERRA_CHECK_CTX if (!brush || (n && (!tile_xy || !d_zvals || !d_stats || !d_weights || !d_grass_blocks || !d_updated))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_edit_grass_dev(tile_xy, n, dxoff, dyoff, d_zvals, d_stats, d_is_distant, brush->pos, brush->radius, brush->add_grass != 0, brush->shape, brush->brush_weight,
		d_weights, (terra::grass_block_pod_t *)d_grass_blocks, d_updated, d_ranges); TERRA_CATCH
}
int terra_tiles_edit_grass(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *h_zvals, const terra_tile_stats *h_stats,
                           const uint8_t *h_is_distant, const terra_grass_brush *brush, uint8_t *h_weights, terra_grass_block *h_grass_blocks, uint8_t *h_updated, uint32_t *h_ranges) {
	TERRA_CHECK_CTX if (!brush || (n && (!tile_xy || !h_zvals || !h_stats || !h_weights || !h_grass_blocks || !h_updated))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_128("tiles_edit_grass"); // (before the arrays are read: they are sized for 128)
		if (n == 0) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const z = st.in(h_zvals, (size_t)n*130*130*4), s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), w = st.inout(h_weights, (size_t)n*129*129*4),
			g = st.inout(h_grass_blocks, (size_t)n*32*32*sizeof(terra_grass_block)), k = st.opt_in(h_is_distant, n), u = st.out(h_updated, n), r = st.out(h_ranges, (size_t)n*16);
		st.begin();
		ctx->eng.tiles_edit_grass_dev(tile_xy, n, dxoff, dyoff, st.dev<float>(z), st.dev<terra_tile_stats>(s), st.dev<uint8_t>(k), brush->pos, brush->radius,
			brush->add_grass != 0, brush->shape, brush->brush_weight, st.dev<uint8_t>(w), st.dev<terra::grass_block_pod_t>(g), st.dev<uint8_t>(u), st.dev<uint32_t>(r));
		st.end();
	TERRA_CATCH
}
static_assert(sizeof(terra_line_hit) == 32 && sizeof(terra::line_hit_pod_t) == 32, "terra_line_hit layout");
int terra_tiles_line_intersect_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *d_zvals, const terra_tile_stats *d_stats,
                                   const uint8_t *d_is_distant, const float *d_lines, const int32_t *d_line_tile, uint32_t nlines, terra_line_hit *d_hits) {
	TERRA_CHECK_CTX if ((n && (!tile_xy || !d_zvals || !d_stats)) || (nlines && (!d_lines || !d_hits))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_line_intersect_dev(tile_xy, n, dxoff, dyoff, d_zvals, d_stats, d_is_distant, d_lines, d_line_tile, nlines, (terra::line_hit_pod_t *)d_hits); TERRA_CATCH
}
int terra_tiles_line_intersect(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *h_zvals, const terra_tile_stats *h_stats,
                               const uint8_t *h_is_distant, const float *h_lines, const int32_t *h_line_tile, uint32_t nlines, terra_line_hit *h_hits) {
	TERRA_CHECK_CTX if ((n && (!tile_xy || !h_zvals || !h_stats)) || (nlines && (!h_lines || !h_hits))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (h_line_tile) {
			for (uint32_t r = 0; r < nlines; ++r) {if (h_line_tile[r] >= 0 && (uint32_t)h_line_tile[r] >= n) {return terra::fail(TERRA_ERR_ARG, "tiles_line_intersect: line_tile entry out of range");}}
		}
		if (nlines == 0) return TERRA_OK;
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng); // (with n == 0 the tile arrays are empty: nothing of them is uploaded)
		int const z = st.in(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), k = st.opt_in(h_is_distant, n),
			l = st.in(h_lines, (size_t)nlines*24), lt = st.opt_in(h_line_tile, (size_t)nlines*4), h = st.out(h_hits, (size_t)nlines*32);
		st.begin();
		ctx->eng.tiles_line_intersect_dev(tile_xy, n, dxoff, dyoff, st.dev<float>(z), st.dev<terra_tile_stats>(s), st.dev<uint8_t>(k), st.dev<float>(l), st.dev<int32_t>(lt), nlines,
			st.dev<terra::line_hit_pod_t>(h));
		st.end();
	TERRA_CATCH
}
static_assert(sizeof(terra_line_tree_hit) == 40 && sizeof(terra::line_tree_hit_pod_t) == 40 && sizeof(terra_line_trees_in) == 72, "terra_line_tree_hit / terra_line_trees_in layout");
int terra_tiles_line_intersect_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_line_trees_in *in, const float *d_lines, const int32_t *d_line_tile,
                                         uint32_t nlines, terra_line_tree_hit *d_hits) {
	TERRA_CHECK_CTX
	TERRA_TRY ctx->eng.tiles_line_intersect_trees_dev(tile_xy, n, in, d_lines, d_line_tile, nlines, (terra::line_tree_hit_pod_t *)d_hits); TERRA_CATCH
}
int terra_tiles_line_intersect_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_line_trees_in *in, const float *h_lines, const int32_t *h_line_tile,
                                     uint32_t nlines, terra_line_tree_hit *h_hits) {
	TERRA_CHECK_CTX
	TERRA_TRY
		ctx->eng.line_trees_check(in, "tiles_line_intersect_trees"); // the scene, the tile size and the members that are no arrays: before anything is staged
		if ((n && (!tile_xy || !in->zvals || !in->stats)) || (nlines && (!h_lines || !h_hits))) return terra::fail(TERRA_ERR_ARG, "null argument");
		if ((uint64_t)n*in->pine_capacity > 0xFFFFFFFFull) return terra::fail(TERRA_ERR_ARG, "tiles_line_intersect_trees: n*pine_capacity must fit 32 bits");
		if ((((uintptr_t)in->zvals | (uintptr_t)in->stats | (uintptr_t)in->pine | (uintptr_t)in->pine_counts | (uintptr_t)in->trunk_override | (uintptr_t)h_lines | (uintptr_t)h_line_tile |
		      (uintptr_t)h_hits) & 3u) != 0) return terra::fail(TERRA_ERR_ARG, "tiles_line_intersect_trees: every array but is_distant must be 4-byte aligned");
		if (h_line_tile) {
			for (uint32_t r = 0; r < nlines; ++r) {if (h_line_tile[r] >= 0 && (uint32_t)h_line_tile[r] >= n) {return terra::fail(TERRA_ERR_ARG, "tiles_line_intersect_trees: line_tile entry out of range");}}
		}
		if (nlines == 0) return TERRA_OK;
		size_t const S = ctx->eng.tile_size(), np = (size_t)n*in->pine_capacity;
		bool const hp = in->pine && in->pine_counts && np;
		terra_stage st(ctx->eng); // (with n == 0 the tile arrays are empty: nothing of them is uploaded)
		int const z = st.in(in->zvals, (size_t)n*(S + 2)*(S + 2)*4), s = st.in(in->stats, (size_t)n*sizeof(terra_tile_stats)), k = st.opt_in(in->is_distant, n),
			p = st.add(in->pine, nullptr, np*sizeof(terra_tree_place), hp), pc = st.add(in->pine_counts, nullptr, (size_t)n*4, hp),
			ov = st.add(in->trunk_override, nullptr, np*sizeof(terra_trunk_override), hp && in->trunk_override),
			l = st.in(h_lines, (size_t)nlines*24), lt = st.opt_in(h_line_tile, (size_t)nlines*4), h = st.out(h_hits, (size_t)nlines*sizeof(terra_line_tree_hit));
		st.begin();
		terra_line_trees_in d = *in;
		d.zvals = st.dev<float>(z); d.stats = st.dev<terra_tile_stats>(s); d.is_distant = st.dev<uint8_t>(k);
		d.pine = st.dev<terra_tree_place>(p); d.pine_counts = st.dev<uint32_t>(pc); d.trunk_override = st.dev<terra_trunk_override>(ov);
		ctx->eng.tiles_line_intersect_trees_dev(tile_xy, n, &d, st.dev<float>(l), st.dev<int32_t>(lt), nlines, st.dev<terra::line_tree_hit_pod_t>(h));
		st.end();
	TERRA_CATCH
}
static_assert(sizeof(terra_tree_splat) == 12 && sizeof(terra::tree_splat_in_t) == 12, "terra_tree_splat layout");
int terra_tiles_tree_map_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *d_is_distant, const terra_tree_splat *d_splats,
                             const uint32_t *h_first, int32_t reset, uint8_t *d_tree_map, uint8_t *d_updated) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_first || !d_tree_map)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_tree_map_dev(tile_xy, n, dxoff, dyoff, d_is_distant, (terra::tree_splat_in_t const *)d_splats, h_first, reset != 0, d_tree_map, d_updated); TERRA_CATCH
}
int terra_tiles_tree_map(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *h_is_distant, const terra_tree_splat *h_splats,
                         const uint32_t *h_first, int32_t reset, uint8_t *h_tree_map, uint8_t *h_updated) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_first || !h_tree_map)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (n == 0) return TERRA_OK;
		for (uint32_t t = 0; t < n; ++t) {if (h_first[t+1] < h_first[t]) {return terra::fail(TERRA_ERR_ARG, "tiles_tree_map: h_first must not decrease");}}
		uint32_t const s0 = h_first[0], ns = h_first[n] - s0;
		if (ns && !h_splats) return terra::fail(TERRA_ERR_ARG, "tiles_tree_map: null splat list");
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng);
		int const m = st.add(reset ? nullptr : h_tree_map, h_tree_map, (size_t)n*(S + 1)*(S + 1)*2), s = st.in(ns ? h_splats + s0 : nullptr, (size_t)ns*sizeof(terra_tree_splat)),
			k = st.opt_in(h_is_distant, n), u = st.out(h_updated, n);
		st.begin();
		std::vector<uint32_t> first(h_first, h_first + n + 1);
		for (uint32_t &f : first) {f -= s0;} // (the device copy holds only the splats the lists name)
		ctx->eng.tiles_tree_map_dev(tile_xy, n, dxoff, dyoff, st.dev<uint8_t>(k), st.dev<terra::tree_splat_in_t>(s), first.data(), reset != 0, st.dev<uint8_t>(m), st.dev<uint8_t>(u));
		st.end();
	TERRA_CATCH
}
int terra_tiles_shadow_texture_dev(terra_ctx *ctx, uint32_t n, const uint8_t *d_smask_sun, const uint8_t *d_smask_moon, const uint8_t *d_ao, const uint8_t *d_tree_map,
                                   float light_factor, int32_t mesh_shadows, uint8_t *d_shadow) {
	TERRA_CHECK_CTX if (n && !d_shadow) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_shadow_texture_dev(n, d_smask_sun, d_smask_moon, d_ao, d_tree_map, light_factor, mesh_shadows, d_shadow); TERRA_CATCH
}
int terra_tiles_shadow_texture(terra_ctx *ctx, uint32_t n, const uint8_t *h_smask_sun, const uint8_t *h_smask_moon, const uint8_t *h_ao, const uint8_t *h_tree_map,
                               float light_factor, int32_t mesh_shadows, uint8_t *h_shadow) {
	TERRA_CHECK_CTX if (n && !h_shadow) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size();
		size_t const S = ctx->eng.tile_size();
		size_t const zb = (size_t)n*(S + 2)*(S + 2), ab = (size_t)n*(S + 1)*(S + 1);
		terra_stage st(ctx->eng); // (with n == 0 every array is empty: nothing is copied)
		int const s1 = st.opt_in(h_smask_sun, zb), s2 = st.opt_in(h_smask_moon, zb), a = st.opt_in(h_ao, ab), t = st.opt_in(h_tree_map, 2*ab), o = st.out(h_shadow, 4*ab);
		st.begin();
		ctx->eng.tiles_shadow_texture_dev(n, st.dev<uint8_t>(s1), st.dev<uint8_t>(s2), st.dev<uint8_t>(a), st.dev<uint8_t>(t), light_factor, mesh_shadows, st.dev<uint8_t>(o));
		st.end();
	TERRA_CATCH
}
int terra_tiles_tree_weights_dev(terra_ctx *ctx, uint32_t n, const uint8_t *d_mesh_weights, const uint8_t *d_tree_map, uint8_t *d_weights) {
	TERRA_CHECK_CTX if (n && (!d_mesh_weights || !d_weights)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_tree_weights_dev(n, d_mesh_weights, d_tree_map, d_weights); TERRA_CATCH
}
int terra_tiles_tree_weights(terra_ctx *ctx, uint32_t n, const uint8_t *h_mesh_weights, const uint8_t *h_tree_map, uint8_t *h_weights) {
	TERRA_CHECK_CTX if (n && (!h_mesh_weights || !h_weights)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_128("tiles_tree_weights"); // (before the arrays are read: they are sized for 128)
		if (n == 0) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const w = st.add(h_mesh_weights, h_weights, (size_t)n*129*129*4), t = st.opt_in(h_tree_map, (size_t)n*129*129*2); // (the output is written over the input)
		st.begin();
		ctx->eng.tiles_tree_weights_dev(n, st.dev<uint8_t>(w), st.dev<uint8_t>(t), st.dev<uint8_t>(w));
		st.end();
	TERRA_CATCH
}
int terra_set_tree_params(terra_ctx *ctx, const terra_tree_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_tree_params(*params); TERRA_CATCH
}
int terra_get_tree_params(terra_ctx *ctx, terra_tree_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.tp; return TERRA_OK;
}
int terra_set_height_histogram(terra_ctx *ctx, const float *h_vals, uint32_t count) {
	TERRA_CHECK_CTX if (count && !h_vals) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_height_histogram(h_vals, count); TERRA_CATCH
}
int terra_get_height_histogram(terra_ctx *ctx, float *h_vals, uint32_t capacity, uint32_t *count) {
	TERRA_CHECK_CTX if (!count) return terra::fail(TERRA_ERR_ARG, "null argument");
	std::vector<float> const &h = ctx->eng.height_histogram;
	*count = (uint32_t)h.size();
	if (h_vals) {memcpy(h_vals, h.data(), std::min<size_t>(capacity, h.size())*sizeof(float));}
	return TERRA_OK;
}
static_assert(sizeof(terra_tree_place) == 40 && sizeof(terra::tree_place_pod_t) == 40, "terra_tree_place layout");
static int tiles_place_trees_impl(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *skip, const terra_tile_stats *stats,
	const float *brush, uint32_t capacity, terra_tree_place *trees, uint32_t *counts, bool host)
{
	TERRA_CHECK_CTX if (n && (!tile_xy || !counts || (capacity && !trees))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		if (!host) {ctx->eng.tiles_place_trees_dev(tile_xy, n, xoff2, yoff2, skip, stats, brush, capacity, (terra::tree_place_pod_t *)trees, counts); return TERRA_OK;}
		ctx->eng.require_scene();
		ctx->eng.require_tile_size();
		if (n == 0) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const r = st.temp((size_t)n*capacity*sizeof(terra_tree_place)), c = st.temp((size_t)n*4), k = st.opt_in(skip, n), s = st.opt_in(stats, (size_t)n*sizeof(terra_tile_stats));
		st.begin();
		ctx->eng.tiles_place_trees_dev(tile_xy, n, xoff2, yoff2, st.dev<uint8_t>(k), st.dev<terra_tile_stats>(s), brush, capacity, st.dev<terra::tree_place_pod_t>(r), st.dev<uint32_t>(c));
		st.end_counted(r, c, trees, counts, n, capacity);
	TERRA_CATCH
}
int terra_tiles_place_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                uint32_t capacity, terra_tree_place *d_trees, uint32_t *d_counts) {
	return tiles_place_trees_impl(ctx, tile_xy, n, xoff2, yoff2, d_skip, d_stats, nullptr, capacity, d_trees, d_counts, false);
}
int terra_tiles_place_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                            uint32_t capacity, terra_tree_place *h_trees, uint32_t *h_counts) {
	return tiles_place_trees_impl(ctx, tile_xy, n, xoff2, yoff2, h_skip, h_stats, nullptr, capacity, h_trees, h_counts, true);
}
int terra_tiles_place_trees_brush_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                      const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_tree_place *d_trees, uint32_t *d_counts) {
	if (!pos) return terra::fail(TERRA_ERR_ARG, "null argument");
	float const brush[4] = {pos[0], pos[1], radius, is_square ? 1.0f : 0.0f};
	return tiles_place_trees_impl(ctx, tile_xy, n, xoff2, yoff2, d_skip, d_stats, brush, capacity, d_trees, d_counts, false);
}
int terra_tiles_place_trees_brush(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                  const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_tree_place *h_trees, uint32_t *h_counts) {
	if (!pos) return terra::fail(TERRA_ERR_ARG, "null argument");
	float const brush[4] = {pos[0], pos[1], radius, is_square ? 1.0f : 0.0f};
	return tiles_place_trees_impl(ctx, tile_xy, n, xoff2, yoff2, h_skip, h_stats, brush, capacity, h_trees, h_counts, true);
}
int terra_set_decid_params(terra_ctx *ctx, const terra_decid_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_decid_params(*params); TERRA_CATCH
}
int terra_get_decid_params(terra_ctx *ctx, terra_decid_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.dp; return TERRA_OK;
}
static_assert(sizeof(terra_decid_place) == 36 && sizeof(terra::decid_place_pod_t) == 36, "terra_decid_place layout");
static int tiles_place_decid_trees_impl(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *skip, const terra_tile_stats *stats,
	const float *zvals, const float *brush, uint32_t capacity, terra_decid_place *trees, uint32_t *counts, bool host)
{
	TERRA_CHECK_CTX if (n && (!tile_xy || !counts || (capacity && !trees))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		if (!host) {ctx->eng.tiles_place_decid_trees_dev(tile_xy, n, xoff2, yoff2, skip, stats, zvals, brush, capacity, (terra::decid_place_pod_t *)trees, counts); return TERRA_OK;}
		ctx->eng.require_scene();
		ctx->eng.require_tile_size();
		if (n && stats && !zvals) throw std::invalid_argument("tiles_place_decid_trees: stats without zvals (the slope test reads the tile's heights)");
		if (n == 0) return TERRA_OK;
		size_t const Z = (size_t)ctx->eng.tile_size() + 2;
		terra_stage st(ctx->eng);
		int const r = st.temp((size_t)n*capacity*sizeof(terra_decid_place)), c = st.temp((size_t)n*4), k = st.opt_in(skip, n), s = st.opt_in(stats, (size_t)n*sizeof(terra_tile_stats)),
			z = st.opt_in(zvals, (size_t)n*Z*Z*sizeof(float));
		st.begin();
		ctx->eng.tiles_place_decid_trees_dev(tile_xy, n, xoff2, yoff2, st.dev<uint8_t>(k), st.dev<terra_tile_stats>(s), st.dev<float>(z), brush, capacity,
			st.dev<terra::decid_place_pod_t>(r), st.dev<uint32_t>(c));
		st.end_counted(r, c, trees, counts, n, capacity);
	TERRA_CATCH
}
int terra_tiles_place_decid_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                      const float *d_zvals, uint32_t capacity, terra_decid_place *d_trees, uint32_t *d_counts) {
	return tiles_place_decid_trees_impl(ctx, tile_xy, n, xoff2, yoff2, d_skip, d_stats, d_zvals, nullptr, capacity, d_trees, d_counts, false);
}
int terra_tiles_place_decid_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                  const float *h_zvals, uint32_t capacity, terra_decid_place *h_trees, uint32_t *h_counts) {
	return tiles_place_decid_trees_impl(ctx, tile_xy, n, xoff2, yoff2, h_skip, h_stats, h_zvals, nullptr, capacity, h_trees, h_counts, true);
}
int terra_tiles_place_decid_trees_brush_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, const terra_tile_stats *d_stats,
                                            const float *d_zvals, const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_decid_place *d_trees, uint32_t *d_counts) {
	if (!pos) return terra::fail(TERRA_ERR_ARG, "null argument");
	float const brush[4] = {pos[0], pos[1], radius, is_square ? 1.0f : 0.0f};
	return tiles_place_decid_trees_impl(ctx, tile_xy, n, xoff2, yoff2, d_skip, d_stats, d_zvals, brush, capacity, d_trees, d_counts, false);
}
int terra_tiles_place_decid_trees_brush(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, const terra_tile_stats *h_stats,
                                        const float *h_zvals, const float pos[3], float radius, int32_t is_square, uint32_t capacity, terra_decid_place *h_trees, uint32_t *h_counts) {
	if (!pos) return terra::fail(TERRA_ERR_ARG, "null argument");
	float const brush[4] = {pos[0], pos[1], radius, is_square ? 1.0f : 0.0f};
	return tiles_place_decid_trees_impl(ctx, tile_xy, n, xoff2, yoff2, h_skip, h_stats, h_zvals, brush, capacity, h_trees, h_counts, true);
}
int terra_set_scenery_params(terra_ctx *ctx, const terra_scenery_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_scenery_params(*params); TERRA_CATCH
}
int terra_get_scenery_params(terra_ctx *ctx, terra_scenery_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.sp; return TERRA_OK;
}
static_assert(sizeof(terra_scenery_place) == 72 && sizeof(terra::scenery_place_pod_t) == 72 && (int)TERRA_SCENERY_KINDS == (int)terra::SCENERY_KINDS, "terra_scenery_place layout");
int terra_tiles_place_scenery_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *d_skip, uint32_t capacity,
                                  terra_scenery_place *d_objs, uint32_t *d_counts, uint32_t *d_kind_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_counts || (capacity && !d_objs))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_place_scenery_dev(tile_xy, n, xoff2, yoff2, d_skip, capacity, (terra::scenery_place_pod_t *)d_objs, d_counts, d_kind_counts); TERRA_CATCH
}
int terra_tiles_place_scenery(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t xoff2, int32_t yoff2, const uint8_t *h_skip, uint32_t capacity,
                              terra_scenery_place *h_objs, uint32_t *h_counts, uint32_t *h_kind_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_counts || (capacity && !h_objs))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size();
		if (n == 0) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const r = st.temp((size_t)n*capacity*sizeof(terra_scenery_place)), c = st.temp((size_t)n*4), k = st.opt_in(h_skip, n), q = st.opt_out(h_kind_counts, (size_t)n*TERRA_SCENERY_KINDS*4);
		st.begin();
		ctx->eng.tiles_place_scenery_dev(tile_xy, n, xoff2, yoff2, st.dev<uint8_t>(k), capacity, st.dev<terra::scenery_place_pod_t>(r), st.dev<uint32_t>(c), st.dev<uint32_t>(q));
		st.end_counted(r, c, h_objs, h_counts, n, capacity);
		st.end();
	TERRA_CATCH
}
int terra_set_flower_params(terra_ctx *ctx, const terra_flower_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_flower_params(*params); TERRA_CATCH
}
int terra_get_flower_params(terra_ctx *ctx, terra_flower_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.fp; return TERRA_OK;
}
static_assert(sizeof(terra_flower) == 48 && sizeof(terra::flower_pod_t) == 48, "terra_flower layout: flower_t (src/grass.h:80-88)");
int terra_tiles_place_flowers_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const uint8_t *d_skip, const uint8_t *d_weights, uint32_t capacity,
                                  terra_flower *d_flowers, uint32_t *d_aux, uint32_t *d_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_counts || (capacity && !d_flowers))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_place_flowers_dev(tile_xy, n, d_skip, d_weights, capacity, (terra::flower_pod_t *)d_flowers, d_aux, d_counts); TERRA_CATCH
}
int terra_tiles_place_flowers(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const uint8_t *h_skip, const uint8_t *h_weights, uint32_t capacity,
                              terra_flower *h_flowers, uint32_t *h_aux, uint32_t *h_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_counts || (capacity && !h_flowers))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (n == 0) return TERRA_OK;
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng);
		int const r = st.temp((size_t)n*capacity*sizeof(terra_flower)), a = st.add(nullptr, nullptr, (size_t)n*capacity*4, h_aux != nullptr), c = st.temp((size_t)n*4),
			k = st.opt_in(h_skip, n), w = st.opt_in(ctx->eng.flowers_skip_generate() ? nullptr : h_weights, (size_t)n*(S + 1)*(S + 1)*4); // (skip_generate: the weights are not read)
		st.begin();
		ctx->eng.tiles_place_flowers_dev(tile_xy, n, st.dev<uint8_t>(k), st.dev<uint8_t>(w), capacity, st.dev<terra::flower_pod_t>(r), st.dev<uint32_t>(a), st.dev<uint32_t>(c));
		st.end_counted(r, c, h_flowers, h_counts, n, capacity);
		if (h_aux) {st.end_counted(a, c, h_aux, h_counts, n, capacity);}
	TERRA_CATCH
}
int terra_tiles_edit_flowers_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *d_generated,
                                 const terra_grass_brush *brush, const uint8_t *d_updated, const uint32_t *d_ranges, const uint8_t *d_weights, uint32_t capacity,
                                 terra_flower *d_flowers, uint32_t *d_aux, uint32_t *d_counts, uint8_t *d_status) {
	TERRA_CHECK_CTX if (!brush || (n && (!tile_xy || !d_updated || !d_counts || !d_status || (capacity && !d_flowers)))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_edit_flowers_dev(tile_xy, n, dxoff, dyoff, d_generated, brush->pos, brush->radius, brush->add_grass != 0, brush->shape, d_updated, d_ranges,
		d_weights, capacity, (terra::flower_pod_t *)d_flowers, d_aux, d_counts, d_status); TERRA_CATCH
}
int terra_tiles_edit_flowers(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const uint8_t *h_generated,
                             const terra_grass_brush *brush, const uint8_t *h_updated, const uint32_t *h_ranges, const uint8_t *h_weights, uint32_t capacity,
                             terra_flower *h_flowers, uint32_t *h_aux, uint32_t *h_counts, uint8_t *h_status) {
	TERRA_CHECK_CTX if (!brush || (n && (!tile_xy || !h_updated || !h_counts || !h_status || (capacity && !h_flowers)))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (n == 0) return TERRA_OK;
		size_t const S = ctx->eng.tile_size();
		bool const add = brush->add_grass != 0;
		terra_stage st(ctx->eng);
		int const r = st.inout(h_flowers, (size_t)n*capacity*sizeof(terra_flower)), a = st.inout(h_aux, (size_t)n*capacity*4, h_aux != nullptr), c = st.inout(h_counts, (size_t)n*4),
			g = st.opt_in(h_generated, n), u = st.in(h_updated, n), q = st.opt_in(h_ranges, (size_t)n*16), w = st.opt_in(add ? h_weights : nullptr, (size_t)n*(S + 1)*(S + 1)*4),
			s = st.out(h_status, n);
		st.begin();
		ctx->eng.tiles_edit_flowers_dev(tile_xy, n, dxoff, dyoff, st.dev<uint8_t>(g), brush->pos, brush->radius, add, brush->shape, st.dev<uint8_t>(u), st.dev<uint32_t>(q),
			st.dev<uint8_t>(w), capacity, st.dev<terra::flower_pod_t>(r), st.dev<uint32_t>(a), st.dev<uint32_t>(c), st.dev<uint8_t>(s));
		st.end();
	TERRA_CATCH
}
static_assert(sizeof(terra_view) == sizeof(terra::view_pod_t) && sizeof(terra_view) == 68, "terra_view layout");
int terra_make_view(const float pos[3], const float dir[3], const float up[3], float angle, float aspect, float near_clip, float far_clip, terra_view *out) {
	if (!pos || !dir || !up || !out) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v;
	if (!terra::view_make(pos, dir, up, angle, aspect, near_clip, far_clip, v)) {
		return terra::fail(TERRA_ERR_ARG, "terra_make_view: needs near >= 0, far > near, a non-zero dir, and tanf(angle) > 0 unless aspect == 1");
	}
	memcpy(out, &v, sizeof(v));
	return TERRA_OK;
}
int terra_set_grass_view_params(terra_ctx *ctx, const terra_grass_view_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_grass_view_params(*params); TERRA_CATCH
}
int terra_get_grass_view_params(terra_ctx *ctx, terra_grass_view_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.gvp; return TERRA_OK;
}
int terra_tiles_grass_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *d_zvals, const terra_tile_stats *d_stats,
                               const terra_grass_block *d_grass_blocks, const uint8_t *d_skip, const terra_view *view, uint32_t capacity, float *d_insts, uint32_t *d_aux,
                               uint32_t *d_group_counts, uint32_t *d_counts, uint8_t *d_pass) {
	TERRA_CHECK_CTX if (!view) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::grass_view_io_t const io = {d_zvals, d_stats, (terra::grass_block_pod_t const *)d_grass_blocks, d_skip, d_insts, d_aux, d_group_counts, d_counts, d_pass};
	TERRA_TRY ctx->eng.tiles_grass_view_dev(tile_xy, n, dxoff, dyoff, v, capacity, io); TERRA_CATCH
}
int terra_tiles_grass_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const float *h_zvals, const terra_tile_stats *h_stats,
                           const terra_grass_block *h_grass_blocks, const uint8_t *h_skip, const terra_view *view, uint32_t capacity, float *h_insts, uint32_t *h_aux,
                           uint32_t *h_group_counts, uint32_t *h_counts, uint8_t *h_pass) {
	TERRA_CHECK_CTX if (!view) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	TERRA_TRY
		ctx->eng.grass_view_check(v); // the scene, the tile size (the arrays are sized by S), the view, num_rnd_grass_blocks: before anything is staged
		terra::grass_view_io_t const h = {h_zvals, h_stats, (terra::grass_block_pod_t const *)h_grass_blocks, h_skip, h_insts, h_aux, h_group_counts, h_counts, h_pass};
		if (!terra::grass_view_io_check(tile_xy, n, capacity, h, false)) return TERRA_OK;
		size_t const S = ctx->eng.tile_size(), dim = 1 + (S - 1)/4, nbins = (size_t)terra::GRASS_VIEW_LODS*ctx->eng.ls.num_rnd_grass_blocks;
		struct inst_t {float v[2];};
		terra_stage st(ctx->eng);
		int const z = st.in(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), g = st.in(h_grass_blocks, (size_t)n*dim*dim*sizeof(terra_grass_block)),
			k = st.opt_in(h_skip, n), r = st.temp((size_t)n*capacity*sizeof(inst_t)), a = st.add(nullptr, nullptr, (size_t)n*capacity*4, h_aux != nullptr),
			gc = st.out(h_group_counts, (size_t)n*nbins*4), c = st.temp((size_t)n*4), p = st.opt_out(h_pass, n);
		st.begin();
		ctx->eng.tiles_grass_view_dev(tile_xy, n, dxoff, dyoff, v, capacity, terra::grass_view_io_t{st.dev<float>(z), st.dev<terra_tile_stats>(s), st.dev<terra::grass_block_pod_t>(g),
			st.dev<uint8_t>(k), st.dev<float>(r), st.dev<uint32_t>(a), st.dev<uint32_t>(gc), st.dev<uint32_t>(c), st.dev<uint8_t>(p)});
		st.end();
		st.end_counted(r, c, (inst_t *)h_insts, h_counts, n, capacity);
		if (h_aux) {st.end_counted(a, c, h_aux, h_counts, n, capacity);}
	TERRA_CATCH
}
static_assert(sizeof(terra_terrain_view_args) == sizeof(terra::terrain_view_args_pod_t) && sizeof(terra_terrain_view_args) == 20, "terra_terrain_view_args layout");
int terra_view_behind_sphere_mult(float angle, float aspect, float *out) {
	if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = terra::view_behind_sphere_mult(angle, aspect);
	return TERRA_OK;
}
// the host form of the terrain view (ra null) and of the reflection view (ta null): `h` holds the caller's arrays
static int terra_terrain_lists_host(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, terra::view_pod_t const &v, terra::terrain_view_args_pod_t const *ta,
                                    terra::reflection_view_args_pod_t const *ra, terra::terrain_view_io_t const &h) {
	TERRA_TRY
		if (ra) {ctx->eng.reflection_view_check(v, *ra);} else {ctx->eng.terrain_view_check(v, *ta);} // the scene, the tile size, the view and the args: before anything is staged
		if (!terra::terrain_view_io_check(ra ? "tiles_reflection_view" : "tiles_terrain_view", tile_xy, n, h, false)) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const s = st.in(h.in.stats, (size_t)n*sizeof(terra_tile_stats)), mn = st.opt_in(h.in.min_normal_z, (size_t)n*4), tr = st.opt_in(h.in.trmax, (size_t)n*4),
			tz = st.opt_in(h.in.tile_zmax, (size_t)n*4), fl = st.opt_in(h.in.flags, n), os = st.inout(h.in.occl_state, n, h.in.occl_state != nullptr), su = st.out(h.status, n),
			di = st.out(h.dist, (size_t)n*4), lo = st.out(h.lod, n), cr = st.out(h.crack, (size_t)n*4), dr = st.temp((size_t)n*4), oc = st.temp((size_t)n*4), cn = st.temp(8),
			nd = st.opt_out(h.not_drawn, n), rf = st.opt_out(h.reflect, n);
		st.begin();
		terra::terrain_view_io_t const io = {{st.dev<terra_tile_stats>(s), st.dev<float>(mn), st.dev<float>(tr), st.dev<float>(tz), st.dev<uint8_t>(fl), st.dev<uint8_t>(os)}, st.dev<uint8_t>(su),
			st.dev<float>(di), st.dev<uint8_t>(lo), st.dev<uint8_t>(cr), st.dev<uint32_t>(dr), st.dev<uint32_t>(oc), st.dev<uint32_t>(cn), st.dev<uint8_t>(nd), st.dev<uint8_t>(rf)};
		if (ra) {ctx->eng.tiles_reflection_view_dev(tile_xy, n, dxoff, dyoff, v, *ra, io);} else {ctx->eng.tiles_terrain_view_dev(tile_xy, n, dxoff, dyoff, v, *ta, io);}
		st.end();
		st.end_counted(dr, cn, h.draw_order, h.counts, 1, n); // the lists' entries past their counts stay as the caller had them
		ctx->eng.be.d2h(h.counts + 1, st.dev<uint32_t>(cn) + 1, 4);
		if (h.counts[1]) {ctx->eng.be.d2h(h.occluded, st.dev<uint32_t>(oc), (size_t)std::min(h.counts[1], n)*4);}
	TERRA_CATCH
}
int terra_tiles_terrain_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_terrain_view_args *args,
                                 const terra_tile_stats *d_stats, const float *d_min_normal_z, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags,
                                 uint8_t *d_occl_state, uint8_t *d_status, float *d_dist, uint8_t *d_lod, uint8_t *d_crack, uint32_t *d_draw_order, uint32_t *d_occluded,
                                 uint32_t *d_counts, uint8_t *d_not_drawn) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::terrain_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY ctx->eng.tiles_terrain_view_dev(tile_xy, n, dxoff, dyoff, v, a, terra::terrain_view_io_t{{d_stats, d_min_normal_z, d_trmax, d_tile_zmax, d_flags, d_occl_state}, d_status, d_dist, d_lod,
		d_crack, d_draw_order, d_occluded, d_counts, d_not_drawn, nullptr}); TERRA_CATCH
}
int terra_tiles_terrain_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_terrain_view_args *args,
                             const terra_tile_stats *h_stats, const float *h_min_normal_z, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags,
                             uint8_t *h_occl_state, uint8_t *h_status, float *h_dist, uint8_t *h_lod, uint8_t *h_crack, uint32_t *h_draw_order, uint32_t *h_occluded,
                             uint32_t *h_counts, uint8_t *h_not_drawn) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::terrain_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	return terra_terrain_lists_host(ctx, tile_xy, n, dxoff, dyoff, v, &a, nullptr, {{h_stats, h_min_normal_z, h_trmax, h_tile_zmax, h_flags, h_occl_state}, h_status, h_dist, h_lod, h_crack,
		h_draw_order, h_occluded, h_counts, h_not_drawn, nullptr});
}
static_assert(sizeof(terra_reflection_view_args) == sizeof(terra::reflection_view_args_pod_t) && sizeof(terra_reflection_view_args) == 24, "terra_reflection_view_args layout");
static_assert(sizeof(terra_water_view_args) == sizeof(terra::water_view_args_pod_t) && sizeof(terra_water_view_args) == 8, "terra_water_view_args layout");
int terra_tiles_reflection_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view,
                                    const terra_reflection_view_args *args, const terra_tile_stats *d_stats, const float *d_min_normal_z, const float *d_trmax,
                                    const float *d_tile_zmax, const uint8_t *d_flags, uint8_t *d_occl_state, uint8_t *d_status, float *d_dist, uint8_t *d_lod, uint8_t *d_crack,
                                    uint32_t *d_draw_order, uint32_t *d_occluded, uint32_t *d_counts, uint8_t *d_not_drawn, uint8_t *d_reflect) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::reflection_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY ctx->eng.tiles_reflection_view_dev(tile_xy, n, dxoff, dyoff, v, a, terra::terrain_view_io_t{{d_stats, d_min_normal_z, d_trmax, d_tile_zmax, d_flags, d_occl_state}, d_status, d_dist, d_lod,
		d_crack, d_draw_order, d_occluded, d_counts, d_not_drawn, d_reflect}); TERRA_CATCH
}
int terra_tiles_reflection_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view,
                                const terra_reflection_view_args *args, const terra_tile_stats *h_stats, const float *h_min_normal_z, const float *h_trmax,
                                const float *h_tile_zmax, const uint8_t *h_flags, uint8_t *h_occl_state, uint8_t *h_status, float *h_dist, uint8_t *h_lod, uint8_t *h_crack,
                                uint32_t *h_draw_order, uint32_t *h_occluded, uint32_t *h_counts, uint8_t *h_not_drawn, uint8_t *h_reflect) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::reflection_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	return terra_terrain_lists_host(ctx, tile_xy, n, dxoff, dyoff, v, nullptr, &a, {{h_stats, h_min_normal_z, h_trmax, h_tile_zmax, h_flags, h_occl_state}, h_status, h_dist, h_lod, h_crack,
		h_draw_order, h_occluded, h_counts, h_not_drawn, h_reflect});
}
int terra_tiles_water_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_water_view_args *args,
                               const terra_tile_stats *d_stats, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags, const uint8_t *d_status,
                               uint32_t *d_water_list, uint8_t *d_cap_mask, uint32_t *d_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::water_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::water_view_io_t const io = {{d_stats, nullptr, d_trmax, d_tile_zmax, d_flags, nullptr}, d_status, d_water_list, d_cap_mask, d_counts};
	TERRA_TRY ctx->eng.tiles_water_view_dev(tile_xy, n, dxoff, dyoff, v, a, io); TERRA_CATCH
}
int terra_tiles_water_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_water_view_args *args,
                           const terra_tile_stats *h_stats, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags, const uint8_t *h_status,
                           uint32_t *h_water_list, uint8_t *h_cap_mask, uint32_t *h_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::water_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.water_view_check(v, a); // the scene, the tile size, the view and the args: before anything is staged
		if (!terra::water_view_io_check(tile_xy, n, {{h_stats, nullptr, h_trmax, h_tile_zmax, h_flags, nullptr}, h_status, h_water_list, h_cap_mask, h_counts}, false)) return TERRA_OK;
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), tr = st.opt_in(h_trmax, (size_t)n*4), tz = st.opt_in(h_tile_zmax, (size_t)n*4), fl = st.opt_in(h_flags, n),
			su = st.opt_in(h_status, n), wl = st.temp((size_t)n*4), cm = st.opt_out(h_cap_mask, n), cn = st.temp(8);
		st.begin();
		ctx->eng.tiles_water_view_dev(tile_xy, n, dxoff, dyoff, v, a, terra::water_view_io_t{{st.dev<terra_tile_stats>(s), nullptr, st.dev<float>(tr), st.dev<float>(tz), st.dev<uint8_t>(fl), nullptr},
			st.dev<uint8_t>(su), st.dev<uint32_t>(wl), st.dev<uint8_t>(cm), st.dev<uint32_t>(cn)});
		st.end();
		st.end_counted(wl, cn, h_water_list, h_counts, 1, n); // the list's entries past its count stay as the caller had them
		if (h_status) {ctx->eng.be.d2h(h_counts + 1, st.dev<uint32_t>(cn) + 1, 4);}
	TERRA_CATCH
}
static_assert(sizeof(terra_smap_plan_args) == sizeof(terra::smap_plan_args_pod_t) && sizeof(terra_smap_plan_args) == 68, "terra_smap_plan_args layout");
static_assert(sizeof(terra_smap_cast_args) == sizeof(terra::smap_cast_args_pod_t) && sizeof(terra_smap_cast_args) == 32, "terra_smap_cast_args layout");
static_assert(TERRA_SMAP_NONE == terra::SMAP_NONE && (int)TERRA_SMAP_USABLE == (int)terra::SMP_USABLE && (int)TERRA_SMAP_TILE_FULLY_IN_CITY == (int)terra::TV_FLAG_FULLY_IN_CITY, "smap enums");
int terra_tiles_smap_plan_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_smap_plan_args *args,
                              const terra_tile_stats *d_stats, const float *d_trmax, const float *d_tile_zmax, const uint8_t *d_flags, uint8_t *d_smap_state, uint32_t *d_plan,
                              float *d_dist_scale, float *d_shadow_bcube, uint32_t *d_receivers, uint32_t *d_counts, uint8_t *d_terrain_flags, uint32_t *d_recomp_order) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::smap_plan_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::smap_plan_io_t const io = {d_stats, d_trmax, d_tile_zmax, d_flags, d_smap_state, d_plan, d_dist_scale, d_shadow_bcube, d_receivers, d_counts, d_terrain_flags, d_recomp_order};
	TERRA_TRY ctx->eng.tiles_smap_plan_dev(tile_xy, n, dxoff, dyoff, v, a, io); TERRA_CATCH
}
int terra_tiles_smap_plan(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, const terra_view *view, const terra_smap_plan_args *args,
                          const terra_tile_stats *h_stats, const float *h_trmax, const float *h_tile_zmax, const uint8_t *h_flags, uint8_t *h_smap_state, uint32_t *h_plan,
                          float *h_dist_scale, float *h_shadow_bcube, uint32_t *h_receivers, uint32_t *h_counts, uint8_t *h_terrain_flags, uint32_t *h_recomp_order) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::smap_plan_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.smap_plan_check(v, a); // the scene, the tile size, the view and the args: before anything is staged
		terra::smap_plan_io_t const h = {h_stats, h_trmax, h_tile_zmax, h_flags, h_smap_state, h_plan, h_dist_scale, h_shadow_bcube, h_receivers, h_counts, h_terrain_flags, h_recomp_order};
		if (!terra::smap_plan_io_check(tile_xy, n, h, false)) return TERRA_OK;
		// every output goes up and comes back: what the call does not write keeps the caller's bytes
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), tr = st.opt_in(h_trmax, (size_t)n*4), tz = st.opt_in(h_tile_zmax, (size_t)n*4), fl = st.opt_in(h_flags, n),
			ss = st.inout(h_smap_state, n), pl = st.inout(h_plan, (size_t)n*4), ds = st.inout(h_dist_scale, (size_t)n*4), sb = st.inout(h_shadow_bcube, (size_t)n*24),
			rc = st.inout(h_receivers, (size_t)n*4), cn = st.inout(h_counts, 8), tf = st.inout(h_terrain_flags, n, h_terrain_flags != nullptr),
			ro = st.inout(h_recomp_order, (size_t)n*4, h_recomp_order != nullptr);
		st.begin();
		ctx->eng.tiles_smap_plan_dev(tile_xy, n, dxoff, dyoff, v, a, terra::smap_plan_io_t{st.dev<terra_tile_stats>(s), st.dev<float>(tr), st.dev<float>(tz), st.dev<uint8_t>(fl),
			st.dev<uint8_t>(ss), st.dev<uint32_t>(pl), st.dev<float>(ds), st.dev<float>(sb), st.dev<uint32_t>(rc), st.dev<uint32_t>(cn), st.dev<uint8_t>(tf), st.dev<uint32_t>(ro)});
		st.end();
	TERRA_CATCH
}
int terra_tiles_smap_casters_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, uint32_t R, const uint32_t *d_recv, const terra_view *views,
                                 const float *bsm, const float *lpos, const terra_smap_cast_args *args, const terra_tile_stats *d_stats, const float *d_trmax,
                                 const float *d_tile_zmax, const uint8_t *d_flags, const uint32_t *d_decid_counts, uint32_t *d_to_draw, uint32_t *d_terrain, uint32_t *d_counts,
                                 uint8_t *d_not_drawn, uint8_t *d_status) {
	TERRA_CHECK_CTX if (!args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::smap_cast_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::smap_cast_io_t const io = {d_stats, d_trmax, d_tile_zmax, d_flags, d_decid_counts, d_recv, d_to_draw, d_terrain, d_counts, d_not_drawn, d_status};
	TERRA_TRY ctx->eng.tiles_smap_casters_dev(tile_xy, n, dxoff, dyoff, R, (terra::view_pod_t const *)views, bsm, lpos, a, io); TERRA_CATCH
}
int terra_tiles_smap_casters(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, uint32_t R, const uint32_t *h_recv, const terra_view *views,
                             const float *bsm, const float *lpos, const terra_smap_cast_args *args, const terra_tile_stats *h_stats, const float *h_trmax,
                             const float *h_tile_zmax, const uint8_t *h_flags, const uint32_t *h_decid_counts, uint32_t *h_to_draw, uint32_t *h_terrain, uint32_t *h_counts,
                             uint8_t *h_not_drawn, uint8_t *h_status) {
	TERRA_CHECK_CTX if (!args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::smap_cast_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.smap_cast_check(a); // the scene, the tile size and the args: before anything is staged
		terra::smap_cast_io_t const h = {h_stats, h_trmax, h_tile_zmax, h_flags, h_decid_counts, h_recv, h_to_draw, h_terrain, h_counts, h_not_drawn, h_status};
		if (!terra::smap_cast_io_check(tile_xy, n, R, (terra::view_pod_t const *)views, bsm, lpos, a, h, false)) return TERRA_OK;
		size_t const rn = (size_t)R*n;
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), tr = st.opt_in(h_trmax, (size_t)n*4), tz = st.opt_in(h_tile_zmax, (size_t)n*4), fl = st.opt_in(h_flags, n),
			dc = st.opt_in(h_decid_counts, (size_t)n*4), rv = st.in(h_recv, (size_t)R*4), td = st.inout(h_to_draw, rn*4), te = st.inout(h_terrain, rn*4), cn = st.inout(h_counts, (size_t)R*8),
			nd = st.inout(h_not_drawn, rn), su = st.inout(h_status, R);
		st.begin();
		ctx->eng.tiles_smap_casters_dev(tile_xy, n, dxoff, dyoff, R, (terra::view_pod_t const *)views, bsm, lpos, a, terra::smap_cast_io_t{st.dev<terra_tile_stats>(s), st.dev<float>(tr),
			st.dev<float>(tz), st.dev<uint8_t>(fl), st.dev<uint32_t>(dc), st.dev<uint32_t>(rv), st.dev<uint32_t>(td), st.dev<uint32_t>(te), st.dev<uint32_t>(cn), st.dev<uint8_t>(nd),
			st.dev<uint8_t>(su)});
		st.end();
	TERRA_CATCH
}
int terra_make_light_view(const float lpos[3], const float bounds[6], float near_clip, terra_view *out, float *behind_sphere_mult) {
	if (!lpos || !bounds || !out || !behind_sphere_mult) return terra::fail(TERRA_ERR_ARG, "null argument");
	bool fin = isfinite(near_clip);
	for (int k = 0; k < 3; ++k) {fin = fin && isfinite(lpos[k]);}
	for (int k = 0; k < 6; ++k) {fin = fin && isfinite(bounds[k]);}
	terra::view_pod_t v; float m = 0.0f;
	if (!fin || !terra::smap_light_view(lpos, bounds, near_clip, v, m)) {
		return terra::fail(TERRA_ERR_ARG, "terra_make_light_view: needs finite arguments, strictly normalized bounds, a light outside the box's centre and a finite view");
	}
	memcpy(out, &v, sizeof(v));
	*behind_sphere_mult = m;
	return TERRA_OK;
}
static_assert(sizeof(terra_cloud_params) == sizeof(terra::cloud_params_pod_t) && sizeof(terra_cloud_params) == 12, "terra_cloud_params layout");
static_assert(sizeof(terra_cloud_step) == sizeof(terra::cloud_step_pod_t) && sizeof(terra_cloud_step) == 20, "terra_cloud_step layout");
static_assert(sizeof(terra_cloud) == sizeof(terra::cloud_pod_t) && sizeof(terra_cloud) == 32, "terra_cloud layout");
static_assert(sizeof(terra_cloud_tile) == sizeof(terra::cloud_tile_pod_t) && sizeof(terra_cloud_tile) == 88, "terra_cloud_tile layout");
static_assert(sizeof(terra_cloud_view_args) == sizeof(terra::cloud_view_args_pod_t) && sizeof(terra_cloud_view_args) == 20, "terra_cloud_view_args layout");
static_assert(sizeof(terra_cloud_inst) == sizeof(terra::cloud_inst_pod_t) && sizeof(terra_cloud_inst) == 24, "terra_cloud_inst layout");
int terra_set_cloud_params(terra_ctx *ctx, const terra_cloud_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::cloud_params_pod_t p; memcpy(&p, params, sizeof(p));
	TERRA_TRY ctx->eng.set_cloud_params(p); TERRA_CATCH
}
int terra_get_cloud_params(terra_ctx *ctx, terra_cloud_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	memcpy(out, &ctx->eng.cp, sizeof(*out)); return TERRA_OK;
}
int terra_tiles_update_clouds_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_cloud_step *step, terra_cloud_tile *d_state, terra_cloud *d_clouds,
                                  uint32_t capacity, uint32_t *d_total) {
	TERRA_CHECK_CTX if (!step) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::cloud_step_pod_t s; memcpy(&s, step, sizeof(s));
	TERRA_TRY ctx->eng.tiles_update_clouds_dev(tile_xy, n, s, capacity, terra::cloud_update_io_t{(terra::cloud_tile_pod_t *)d_state, (terra::cloud_pod_t *)d_clouds, d_total}); TERRA_CATCH
}
int terra_tiles_update_clouds(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_cloud_step *step, terra_cloud_tile *h_state, terra_cloud *h_clouds,
                              uint32_t capacity, uint32_t *h_total) {
	TERRA_CHECK_CTX if (!step) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::cloud_step_pod_t s; memcpy(&s, step, sizeof(s));
	TERRA_TRY
		ctx->eng.cloud_update_check(s, capacity); // the scene, the tile size, the step and the capacity: before anything is staged
		if (!terra::cloud_update_io_check(tile_xy, n, capacity, {(terra::cloud_tile_pod_t *)h_state, (terra::cloud_pod_t *)h_clouds, h_total}, false)) {if (h_total) {*h_total = 0u;} return TERRA_OK;}
		terra_stage st(ctx->eng);
		int const ss = st.inout(h_state, (size_t)n*sizeof(terra_cloud_tile)), cl = st.inout(h_clouds, (size_t)n*capacity*sizeof(terra_cloud), capacity != 0), to = st.opt_out(h_total, 4);
		st.begin();
		ctx->eng.tiles_update_clouds_dev(tile_xy, n, s, capacity, terra::cloud_update_io_t{st.dev<terra::cloud_tile_pod_t>(ss), st.dev<terra::cloud_pod_t>(cl), st.dev<uint32_t>(to)});
		st.end();
	TERRA_CATCH
}
int terra_tiles_cloud_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_view *view, const terra_cloud_view_args *args, const terra_tile_stats *d_stats,
                               const terra_cloud_tile *d_state, const terra_cloud *d_clouds, uint32_t capacity, uint8_t *d_stage, terra_cloud_inst *d_list, uint32_t *d_list_count) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::cloud_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::cloud_view_io_t const io = {d_stats, (terra::cloud_tile_pod_t const *)d_state, (terra::cloud_pod_t const *)d_clouds, d_stage, (terra::cloud_inst_pod_t *)d_list, d_list_count};
	TERRA_TRY ctx->eng.tiles_cloud_view_dev(tile_xy, n, v, a, capacity, io); TERRA_CATCH
}
int terra_tiles_cloud_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_view *view, const terra_cloud_view_args *args, const terra_tile_stats *h_stats,
                           const terra_cloud_tile *h_state, const terra_cloud *h_clouds, uint32_t capacity, uint8_t *h_stage, terra_cloud_inst *h_list, uint32_t *h_list_count) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::cloud_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.cloud_view_check(v, a); // the scene, the tile size, the view and the args: before anything is staged
		terra::cloud_view_io_t const h = {h_stats, (terra::cloud_tile_pod_t const *)h_state, (terra::cloud_pod_t const *)h_clouds, h_stage, (terra::cloud_inst_pod_t *)h_list, h_list_count};
		if (!terra::cloud_view_io_check(tile_xy, n, capacity, h, false)) {if (h_list_count) {*h_list_count = 0u;} return TERRA_OK;}
		size_t const nrec = (size_t)n*capacity;
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), ss = st.in(h_state, (size_t)n*sizeof(terra_cloud_tile)), cl = st.add(h_clouds, nullptr, nrec*sizeof(terra_cloud), nrec != 0),
			sg = st.add(nullptr, h_stage, nrec, nrec != 0), li = st.add(nullptr, nullptr, nrec*sizeof(terra_cloud_inst), nrec != 0), lc = st.out(h_list_count, 4);
		st.begin();
		ctx->eng.tiles_cloud_view_dev(tile_xy, n, v, a, capacity, terra::cloud_view_io_t{st.dev<terra_tile_stats>(s), st.dev<terra::cloud_tile_pod_t>(ss), st.dev<terra::cloud_pod_t>(cl),
			st.dev<uint8_t>(sg), st.dev<terra::cloud_inst_pod_t>(li), st.dev<uint32_t>(lc)});
		st.end();
		if (*h_list_count) {ctx->eng.be.d2h(h_list, st.dev<terra_cloud_inst>(li), (size_t)*h_list_count*sizeof(terra_cloud_inst));} // the entries past the count stay as the caller had them
	TERRA_CATCH
}
static_assert(sizeof(terra_sphere_query) == sizeof(terra::sphere_query_pod_t) && sizeof(terra_sphere_query) == 24, "terra_sphere_query layout");
static_assert(sizeof(terra_sphere_hit) == sizeof(terra::sphere_hit_pod_t) && sizeof(terra_sphere_hit) == 24, "terra_sphere_hit layout");
static_assert(sizeof(terra_collide_in) == 168, "terra_collide_in layout");
int terra_tiles_sphere_collide_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const terra_sphere_query *d_queries, uint32_t nq,
                                   terra_sphere_hit *d_hits) {
	TERRA_CHECK_CTX
	TERRA_TRY ctx->eng.tiles_sphere_collide_dev(tile_xy, n, in, (terra::sphere_query_pod_t const *)d_queries, nq, (terra::sphere_hit_pod_t *)d_hits); TERRA_CATCH
}
// the device copies of a terra_collide_in of host pointers: declared on `st`, bound into `dev` after st.begin()
struct terra_collide_stage {
	int s[14];
	terra_collide_stage(terra_stage &st, terra_collide_in const &a, uint32_t n, bool cube) {
		size_t const np = (size_t)n*a.pine_capacity, nd = (size_t)n*a.decid_capacity, ns = (size_t)n*a.scenery_capacity;
		bool const hp = !cube && a.pine && a.pine_counts && np, hd = a.decid && a.decid_counts && nd, hs = !cube && a.scenery && a.scenery_counts && ns;
		s[0] = st.add(a.stats, nullptr, (size_t)n*sizeof(terra_tile_stats), !cube && a.stats && n);
		s[1] = st.add(a.trmax, nullptr, (size_t)n*4, !cube && a.trmax && n); s[2] = st.add(a.tile_zmax, nullptr, (size_t)n*4, !cube && a.tile_zmax && n);
		s[3] = st.add(a.flags, nullptr, n, !cube && a.flags && n);
		s[4] = st.add(a.pine, nullptr, np*sizeof(terra_tree_place), hp); s[5] = st.add(a.pine_counts, nullptr, (size_t)n*4, hp);
		s[6] = st.add(a.trunk_override, nullptr, np*sizeof(terra_trunk_override), hp && a.trunk_override);
		s[7] = st.add(a.decid, nullptr, nd*sizeof(terra_decid_place), hd); s[8] = st.add(a.decid_counts, nullptr, (size_t)n*4, hd);
		s[9] = st.add(a.scenery, nullptr, ns*sizeof(terra_scenery_place), hs); s[10] = st.add(a.scenery_counts, nullptr, (size_t)n*4, hs);
		s[11] = st.add(a.radius_override, nullptr, ns*4, hs && a.radius_override);
		s[12] = st.add(a.tree_data, nullptr, (size_t)a.num_tree_data*sizeof(terra_decid_tree_data), hd && a.tree_data);
		s[13] = st.add(a.br_scale, nullptr, (size_t)a.num_tree_data*4, hd && a.br_scale);
	}
	terra_collide_in bind(terra_stage const &st, terra_collide_in const &a) const {
		terra_collide_in d = a;
		d.stats = st.dev<terra_tile_stats>(s[0]); d.trmax = st.dev<float>(s[1]); d.tile_zmax = st.dev<float>(s[2]); d.flags = st.dev<uint8_t>(s[3]);
		d.pine = st.dev<terra_tree_place>(s[4]); d.pine_counts = st.dev<uint32_t>(s[5]); d.trunk_override = st.dev<terra_trunk_override>(s[6]);
		d.decid = st.dev<terra_decid_place>(s[7]); d.decid_counts = st.dev<uint32_t>(s[8]);
		d.scenery = st.dev<terra_scenery_place>(s[9]); d.scenery_counts = st.dev<uint32_t>(s[10]); d.radius_override = st.dev<float>(s[11]);
		d.tree_data = st.dev<terra_decid_tree_data>(s[12]); d.br_scale = st.dev<float>(s[13]);
		return d;
	}
};
int terra_tiles_sphere_collide(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const terra_sphere_query *h_queries, uint32_t nq,
                               terra_sphere_hit *h_hits) {
	TERRA_CHECK_CTX
	TERRA_TRY
		ctx->eng.collide_check(in, false, "tiles_sphere_collide"); // the scene, the tile size and the members that are no arrays: before anything is staged
		if (n && (!tile_xy || !in->stats)) return terra::fail(TERRA_ERR_ARG, "null argument");
		if (nq && (!h_queries || !h_hits)) return terra::fail(TERRA_ERR_ARG, "null argument");
		if ((uint64_t)n*in->pine_capacity > 0xFFFFFFFFull || (uint64_t)n*in->decid_capacity > 0xFFFFFFFFull || (uint64_t)n*in->scenery_capacity > 0xFFFFFFFFull) {
			return terra::fail(TERRA_ERR_ARG, "tiles_sphere_collide: n*capacity must fit 32 bits");
		}
		terra_stage st(ctx->eng);
		terra_collide_stage const cs(st, *in, n, false);
		int const q = st.add(h_queries, nullptr, (size_t)nq*sizeof(terra_sphere_query), nq != 0), h = st.add(nullptr, h_hits, (size_t)nq*sizeof(terra_sphere_hit), nq != 0);
		st.begin();
		terra_collide_in const d = cs.bind(st, *in);
		ctx->eng.tiles_sphere_collide_dev(tile_xy, n, &d, st.dev<terra::sphere_query_pod_t>(q), nq, st.dev<terra::sphere_hit_pod_t>(h));
		st.end();
	TERRA_CATCH
}
int terra_tiles_cube_int_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const float *d_cubes, const int32_t *d_cube_tile,
                                   uint32_t nq, uint8_t *d_result, int32_t *d_tile_out) {
	TERRA_CHECK_CTX
	TERRA_TRY ctx->eng.tiles_cube_int_trees_dev(tile_xy, n, in, d_cubes, d_cube_tile, nq, d_result, d_tile_out); TERRA_CATCH
}
int terra_tiles_cube_int_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const terra_collide_in *in, const float *h_cubes, const int32_t *h_cube_tile,
                               uint32_t nq, uint8_t *h_result, int32_t *h_tile_out) {
	TERRA_CHECK_CTX
	TERRA_TRY
		ctx->eng.collide_check(in, true, "tiles_cube_int_trees");
		if (n && !tile_xy) return terra::fail(TERRA_ERR_ARG, "null argument");
		if (nq && (!h_cubes || !h_result)) return terra::fail(TERRA_ERR_ARG, "null argument");
		if ((uint64_t)n*in->decid_capacity > 0xFFFFFFFFull) return terra::fail(TERRA_ERR_ARG, "tiles_cube_int_trees: n*capacity must fit 32 bits");
		terra_stage st(ctx->eng);
		terra_collide_stage const cs(st, *in, n, true);
		int const q = st.add(h_cubes, nullptr, (size_t)nq*24, nq != 0), qt = st.add(h_cube_tile, nullptr, (size_t)nq*4, nq != 0 && h_cube_tile),
			r = st.add(nullptr, h_result, nq, nq != 0), to = st.add(nullptr, h_tile_out, (size_t)nq*4, nq != 0 && h_tile_out);
		st.begin();
		terra_collide_in const d = cs.bind(st, *in);
		ctx->eng.tiles_cube_int_trees_dev(tile_xy, n, &d, st.dev<float>(q), st.dev<int32_t>(qt), nq, st.dev<uint8_t>(r), st.dev<int32_t>(to));
		st.end();
	TERRA_CATCH
}
static_assert(sizeof(terra_tree_view_args) == sizeof(terra::tree_view_args_pod_t) && sizeof(terra_tree_view_args) == 32, "terra_tree_view_args layout");
static_assert(sizeof(terra_tree_view_tile) == sizeof(terra::tree_view_tile_pod_t) && sizeof(terra_tree_view_tile) == 32, "terra_tree_view_tile layout");
static_assert(sizeof(terra_tree_view_inst) == sizeof(terra::tree_view_inst_pod_t) && sizeof(terra_tree_view_inst) == 16, "terra_tree_view_inst layout");
static_assert(sizeof(terra_trunk_override) == sizeof(terra::trunk_override_pod_t) && sizeof(terra_trunk_override) == 36, "terra_trunk_override layout");
int terra_tiles_tree_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                              const terra_tree_view_args *args, const terra_tile_stats *d_stats, const uint8_t *d_skip, const float *d_trmax, const terra_tree_place *d_pine,
                              const uint32_t *d_pine_counts, uint32_t capacity, const terra_trunk_override *d_trunk_override, terra_tree_view_tile *d_tile_out,
                              float *d_all_bcube, terra_tree_view_inst *d_pine_insts, terra_tree_view_inst *d_palm_insts, uint32_t *d_inst_counts, uint32_t *d_leaf_list,
                              uint32_t *d_leaf_counts, uint8_t *d_trunk) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::tree_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::tree_view_io_t const io = {d_stats, d_skip, d_trmax, (terra::tree_place_pod_t const *)d_pine, d_pine_counts, (terra::trunk_override_pod_t const *)d_trunk_override,
		(terra::tree_view_tile_pod_t *)d_tile_out, d_all_bcube, (terra::tree_view_inst_pod_t *)d_pine_insts, (terra::tree_view_inst_pod_t *)d_palm_insts, d_inst_counts, d_leaf_list,
		d_leaf_counts, d_trunk};
	TERRA_TRY ctx->eng.tiles_tree_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, capacity, io); TERRA_CATCH
}
int terra_tiles_tree_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                          const terra_tree_view_args *args, const terra_tile_stats *h_stats, const uint8_t *h_skip, const float *h_trmax, const terra_tree_place *h_pine,
                          const uint32_t *h_pine_counts, uint32_t capacity, const terra_trunk_override *h_trunk_override, terra_tree_view_tile *h_tile_out,
                          float *h_all_bcube, terra_tree_view_inst *h_pine_insts, terra_tree_view_inst *h_palm_insts, uint32_t *h_inst_counts, uint32_t *h_leaf_list,
                          uint32_t *h_leaf_counts, uint8_t *h_trunk) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::tree_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.tree_view_check(v, a); // the scene, the tile size, the view, the args and the instance table: before anything is staged
		typedef terra::tree_view_inst_pod_t inst_t;
		terra::tree_view_io_t const h = {h_stats, h_skip, h_trmax, (terra::tree_place_pod_t const *)h_pine, h_pine_counts, (terra::trunk_override_pod_t const *)h_trunk_override,
			(terra::tree_view_tile_pod_t *)h_tile_out, h_all_bcube, (inst_t *)h_pine_insts, (inst_t *)h_palm_insts, h_inst_counts, h_leaf_list, h_leaf_counts, h_trunk};
		if (!terra::tree_view_io_check(tile_xy, n, capacity, h, false)) return TERRA_OK;
		size_t const nc = (size_t)n*capacity;
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), sk = st.opt_in(h_skip, n), tr = st.opt_in(h_trmax, (size_t)n*4), p = st.in(h_pine, nc*sizeof(terra_tree_place)),
			pc = st.in(h_pine_counts, (size_t)n*4), ov = st.opt_in(h_trunk_override, nc*sizeof(terra_trunk_override)), to = st.out(h_tile_out, (size_t)n*sizeof(terra_tree_view_tile)),
			bc = st.out(h_all_bcube, (size_t)n*24), pi = st.temp(nc*sizeof(inst_t)), mi = st.temp(nc*sizeof(inst_t)), ic = st.out(h_inst_counts, (size_t)n*8), ll = st.temp(nc*4),
			lc = st.out(h_leaf_counts, (size_t)n*8), tk = st.temp(nc);
		st.begin();
		ctx->eng.tiles_tree_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, capacity, terra::tree_view_io_t{st.dev<terra_tile_stats>(s), st.dev<uint8_t>(sk), st.dev<float>(tr),
			st.dev<terra::tree_place_pod_t>(p), st.dev<uint32_t>(pc), st.dev<terra::trunk_override_pod_t>(ov), st.dev<terra::tree_view_tile_pod_t>(to), st.dev<float>(bc), st.dev<inst_t>(pi),
			st.dev<inst_t>(mi), st.dev<uint32_t>(ic), st.dev<uint32_t>(ll), st.dev<uint32_t>(lc), st.dev<uint8_t>(tk)});
		st.end();
		for (uint32_t t = 0; t < n; ++t) { // of every tile only what the counts name: the rest of the caller's arrays stays as it was
			size_t const o = (size_t)t*capacity;
			uint32_t const np = std::min(h_inst_counts[2*t], capacity), nm = std::min(h_inst_counts[2*t + 1], capacity), nl = std::min(h_tile_out[t].leaf_written, capacity);
			if (np) {ctx->eng.be.d2h(h_pine_insts + o, st.dev<inst_t>(pi) + o, (size_t)np*sizeof(inst_t));}
			if (nm) {ctx->eng.be.d2h(h_palm_insts + o, st.dev<inst_t>(mi) + o, (size_t)nm*sizeof(inst_t));}
			if (nl) {ctx->eng.be.d2h(h_leaf_list + o, st.dev<uint32_t>(ll) + o, (size_t)nl*4);}
			if (h_tile_out[t].num_trees) {ctx->eng.be.d2h(h_trunk + o, st.dev<uint8_t>(tk) + o, std::min(h_pine_counts[t], capacity));}
		}
	TERRA_CATCH
}
static_assert(sizeof(terra_scenery_view_args) == sizeof(terra::scenery_view_args_pod_t) && sizeof(terra_scenery_view_args) == 40, "terra_scenery_view_args layout");
static_assert(sizeof(terra_scenery_view_tile) == sizeof(terra::scenery_view_tile_pod_t) && sizeof(terra_scenery_view_tile) == 32, "terra_scenery_view_tile layout");
static_assert((uint32_t)TERRA_SCV_GROUPS == terra::SCV_GROUPS && (int)TERRA_SCV_ENGINE == (int)terra::SCV_ENGINE && (int)TERRA_SCV_BERRIES == (int)terra::SCV_BERRIES &&
              (int)TERRA_SCV_G_PLD_LINES == (int)terra::SCV_G_PLD_LINES, "TERRA_SCV_* mirror terra_sceneryview.hpp");
int terra_tiles_scenery_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                                 const terra_scenery_view_args *args, const terra_tile_stats *d_stats, const uint8_t *d_skip, const terra_scenery_place *d_objs,
                                 const uint32_t *d_counts, uint32_t capacity, const float *d_radius_override, terra_scenery_view_tile *d_tile_out, uint32_t *d_draw,
                                 float *d_size_scale, float *d_dist, uint32_t *d_list, uint32_t list_capacity, uint32_t *d_group_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::scenery_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::scenery_view_io_t const io = {d_stats, d_skip, (terra::scenery_place_pod_t const *)d_objs, d_counts, d_radius_override, (terra::scenery_view_tile_pod_t *)d_tile_out, d_draw,
		d_size_scale, d_dist, d_list, d_group_counts};
	TERRA_TRY ctx->eng.tiles_scenery_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, capacity, list_capacity, io); TERRA_CATCH
}
int terra_tiles_scenery_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                             const terra_scenery_view_args *args, const terra_tile_stats *h_stats, const uint8_t *h_skip, const terra_scenery_place *h_objs,
                             const uint32_t *h_counts, uint32_t capacity, const float *h_radius_override, terra_scenery_view_tile *h_tile_out, uint32_t *h_draw,
                             float *h_size_scale, float *h_dist, uint32_t *h_list, uint32_t list_capacity, uint32_t *h_group_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::scenery_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.scenery_view_check(v, a); // the scene, the tile size, the view and the args: before anything is staged
		terra::scenery_view_io_t const h = {h_stats, h_skip, (terra::scenery_place_pod_t const *)h_objs, h_counts, h_radius_override, (terra::scenery_view_tile_pod_t *)h_tile_out, h_draw,
			h_size_scale, h_dist, h_list, h_group_counts};
		if (!terra::scenery_view_io_check(tile_xy, n, capacity, list_capacity, h, false)) return TERRA_OK;
		size_t const nc = (size_t)n*capacity, nl = (size_t)n*list_capacity;
		terra_stage st(ctx->eng);
		int const s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), sk = st.opt_in(h_skip, n), ob = st.in(h_objs, nc*sizeof(terra_scenery_place)), pc = st.in(h_counts, (size_t)n*4),
			ov = st.opt_in(h_radius_override, nc*4), to = st.out(h_tile_out, (size_t)n*sizeof(terra_scenery_view_tile)), dr = st.temp(nc*4), sz = st.temp(nc*4), di = st.temp(nc*4),
			ll = st.temp(nl*4), gc = st.out(h_group_counts, (size_t)n*TERRA_SCV_GROUPS*4);
		st.begin();
		ctx->eng.tiles_scenery_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, capacity, list_capacity, terra::scenery_view_io_t{st.dev<terra_tile_stats>(s), st.dev<uint8_t>(sk),
			st.dev<terra::scenery_place_pod_t>(ob), st.dev<uint32_t>(pc), st.dev<float>(ov), st.dev<terra::scenery_view_tile_pod_t>(to), st.dev<uint32_t>(dr), st.dev<float>(sz),
			st.dev<float>(di), st.dev<uint32_t>(ll), st.dev<uint32_t>(gc)});
		st.end();
		for (uint32_t t = 0; t < n; ++t) { // of every tile only what its record names: the rest of the caller's arrays stays as it was
			size_t const o = (size_t)t*capacity, lo = (size_t)t*list_capacity;
			uint32_t const nr = std::min(h_tile_out[t].num_records, capacity), nw = std::min(h_tile_out[t].list_written, list_capacity);
			if (nr) {
				ctx->eng.be.d2h(h_draw + o, st.dev<uint32_t>(dr) + o, (size_t)nr*4);
				ctx->eng.be.d2h(h_size_scale + o, st.dev<float>(sz) + o, (size_t)nr*4);
				ctx->eng.be.d2h(h_dist + o, st.dev<float>(di) + o, (size_t)nr*4);
			}
			if (nw) {ctx->eng.be.d2h(h_list + lo, st.dev<uint32_t>(ll) + lo, (size_t)nw*4);}
		}
	TERRA_CATCH
}
static_assert(sizeof(terra_decid_view_args) == sizeof(terra::decid_view_args_pod_t) && sizeof(terra_decid_view_args) == 48, "terra_decid_view_args layout");
static_assert(sizeof(terra_decid_tree_data) == sizeof(terra::decid_tree_data_pod_t) && sizeof(terra_decid_tree_data) == 80, "terra_decid_tree_data layout");
static_assert(sizeof(terra_decid_view_tile) == sizeof(terra::decid_view_tile_pod_t) && sizeof(terra_decid_view_tile) == 32, "terra_decid_view_tile layout");
static_assert(sizeof(terra_decid_view_bb) == sizeof(terra::decid_view_bb_pod_t) && sizeof(terra_decid_view_bb) == 24, "terra_decid_view_bb layout");
static_assert((int)TERRA_DCV_BRANCH_TEX == (int)terra::DCV_BRANCH_TEX && (int)TERRA_DCV_TILE_BCUBE_ZERO_AREA == (int)terra::DCV_TILE_BCUBE_ZERO_AREA &&
              (int)TERRA_DCV_LOW_DETAIL == (int)terra::DCV_LOW_DETAIL && (int)TERRA_DCV_STAGE_SHADOW_SPHERE == (int)terra::DCV_STAGE_SHADOW_SPHERE &&
              (int)TERRA_DCV_STAGE_SHIFT == (int)terra::DCV_STAGE_SHIFT, "TERRA_DCV_* mirror terra_decidview.hpp");
int terra_tiles_decid_view_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                               const terra_decid_view_args *args, const terra_decid_tree_data *d_tree_data, uint32_t num_tree_data, const uint8_t *d_skip,
                               const terra_decid_place *d_decid, const uint32_t *d_counts, uint32_t capacity, uint8_t *d_not_visible, terra_decid_view_tile *d_tile_out,
                               float *d_all_bcube, uint32_t *d_leaf_word, float *d_leaf_scale, float *d_leaf_opacity, uint32_t *d_leaf_num, uint32_t *d_branch_word,
                               float *d_branch_scale, float *d_branch_opacity, uint32_t *d_branch_num, uint32_t *d_leaf_list, uint32_t *d_branch_list,
                               terra_decid_view_bb *d_leaf_bb, terra_decid_view_bb *d_branch_bb, uint32_t *d_list_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::decid_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	terra::decid_view_io_t const io = {(terra::decid_tree_data_pod_t const *)d_tree_data, d_skip, (terra::decid_place_pod_t const *)d_decid, d_counts, d_not_visible,
		(terra::decid_view_tile_pod_t *)d_tile_out, d_all_bcube, d_leaf_word, d_leaf_scale, d_leaf_opacity, d_leaf_num, d_branch_word, d_branch_scale, d_branch_opacity, d_branch_num,
		d_leaf_list, d_branch_list, (terra::decid_view_bb_pod_t *)d_leaf_bb, (terra::decid_view_bb_pod_t *)d_branch_bb, d_list_counts};
	TERRA_TRY ctx->eng.tiles_decid_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, num_tree_data, capacity, io); TERRA_CATCH
}
int terra_tiles_decid_view(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2, const terra_view *view,
                           const terra_decid_view_args *args, const terra_decid_tree_data *h_tree_data, uint32_t num_tree_data, const uint8_t *h_skip,
                           const terra_decid_place *h_decid, const uint32_t *h_counts, uint32_t capacity, uint8_t *h_not_visible, terra_decid_view_tile *h_tile_out,
                           float *h_all_bcube, uint32_t *h_leaf_word, float *h_leaf_scale, float *h_leaf_opacity, uint32_t *h_leaf_num, uint32_t *h_branch_word,
                           float *h_branch_scale, float *h_branch_opacity, uint32_t *h_branch_num, uint32_t *h_leaf_list, uint32_t *h_branch_list,
                           terra_decid_view_bb *h_leaf_bb, terra_decid_view_bb *h_branch_bb, uint32_t *h_list_counts) {
	TERRA_CHECK_CTX if (!view || !args) return terra::fail(TERRA_ERR_ARG, "null argument");
	terra::view_pod_t v; memcpy(&v, view, sizeof(v));
	terra::decid_view_args_pod_t a; memcpy(&a, args, sizeof(a));
	TERRA_TRY
		ctx->eng.decid_view_check(v, a, num_tree_data); // the scene, the tile size, the view, the args and the table's length: before anything is staged
		typedef terra::decid_view_bb_pod_t bb_t;
		terra::decid_view_io_t const h = {(terra::decid_tree_data_pod_t const *)h_tree_data, h_skip, (terra::decid_place_pod_t const *)h_decid, h_counts, h_not_visible,
			(terra::decid_view_tile_pod_t *)h_tile_out, h_all_bcube, h_leaf_word, h_leaf_scale, h_leaf_opacity, h_leaf_num, h_branch_word, h_branch_scale, h_branch_opacity, h_branch_num,
			h_leaf_list, h_branch_list, (bb_t *)h_leaf_bb, (bb_t *)h_branch_bb, h_list_counts};
		if (!terra::decid_view_io_check(tile_xy, n, capacity, h, false)) return TERRA_OK;
		size_t const nc = (size_t)n*capacity;
		terra_stage st(ctx->eng);
		// the per-record arrays and the lists go up as the caller has them and come back: the call writes only some of their entries
		int const td = st.in(h_tree_data, (size_t)num_tree_data*sizeof(terra_decid_tree_data)), sk = st.opt_in(h_skip, n), de = st.in(h_decid, nc*sizeof(terra_decid_place)),
			pc = st.in(h_counts, (size_t)n*4), nv = st.inout(h_not_visible, nc, h_not_visible != nullptr), to = st.out(h_tile_out, (size_t)n*sizeof(terra_decid_view_tile)),
			bc = st.out(h_all_bcube, (size_t)n*24), lw = st.inout(h_leaf_word, nc*4), ls = st.inout(h_leaf_scale, nc*4), lo = st.inout(h_leaf_opacity, nc*4),
			ln = st.inout(h_leaf_num, nc*4), bw = st.inout(h_branch_word, nc*4), bs = st.inout(h_branch_scale, nc*4), bo = st.inout(h_branch_opacity, nc*4),
			bn = st.inout(h_branch_num, nc*4), ll = st.inout(h_leaf_list, nc*4), bl = st.inout(h_branch_list, nc*4), lb = st.inout(h_leaf_bb, nc*sizeof(bb_t)),
			bb = st.inout(h_branch_bb, nc*sizeof(bb_t)), lc = st.out(h_list_counts, (size_t)n*16);
		st.begin();
		ctx->eng.tiles_decid_view_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, v, a, num_tree_data, capacity, terra::decid_view_io_t{st.dev<terra::decid_tree_data_pod_t>(td),
			st.dev<uint8_t>(sk), st.dev<terra::decid_place_pod_t>(de), st.dev<uint32_t>(pc), st.dev<uint8_t>(nv), st.dev<terra::decid_view_tile_pod_t>(to), st.dev<float>(bc),
			st.dev<uint32_t>(lw), st.dev<float>(ls), st.dev<float>(lo), st.dev<uint32_t>(ln), st.dev<uint32_t>(bw), st.dev<float>(bs), st.dev<float>(bo), st.dev<uint32_t>(bn),
			st.dev<uint32_t>(ll), st.dev<uint32_t>(bl), st.dev<bb_t>(lb), st.dev<bb_t>(bb), st.dev<uint32_t>(lc)});
		st.end();
	TERRA_CATCH
}
int terra_set_tree_size_params(terra_ctx *ctx, const terra_tree_size_params *params) {
	TERRA_CHECK_CTX if (!params) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_tree_size_params(*params); TERRA_CATCH
}
int terra_get_tree_size_params(terra_ctx *ctx, terra_tree_size_params *out) {
	TERRA_CHECK_CTX if (!out) return terra::fail(TERRA_ERR_ARG, "null argument");
	*out = ctx->eng.tsp; return TERRA_OK;
}
static_assert(sizeof(terra_tree_inst) == 12 && sizeof(terra::tree_inst_pod_t) == 12, "terra_tree_inst layout");
int terra_set_tree_instances(terra_ctx *ctx, const terra_tree_inst *h_insts, uint32_t count) {
	TERRA_CHECK_CTX if (count && !h_insts) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.set_tree_instances((terra::tree_inst_pod_t const *)h_insts, count); TERRA_CATCH
}
int terra_get_tree_instances(terra_ctx *ctx, terra_tree_inst *h_insts, uint32_t capacity, uint32_t *count) {
	TERRA_CHECK_CTX if (!count) return terra::fail(TERRA_ERR_ARG, "null argument");
	std::vector<terra::tree_inst_pod_t> const &v = ctx->eng.tree_insts;
	*count = (uint32_t)v.size();
	if (h_insts) {memcpy(h_insts, v.data(), std::min<size_t>(capacity, v.size())*sizeof(terra_tree_inst));}
	return TERRA_OK;
}
int terra_tiles_tree_ao_shadows_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                                    const terra_tree_place *d_pine, const uint32_t *d_pine_counts, uint32_t pine_capacity,
                                    const terra_decid_place *d_decid, const uint32_t *d_decid_counts, uint32_t decid_capacity,
                                    const float *d_decid_radius, const float *d_decid_radius_by_id, uint32_t num_radius_by_id, const uint8_t *d_flags,
                                    uint32_t list_capacity, uint8_t *d_tree_map, uint8_t *d_updated, float *d_trmax, uint32_t *d_list_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_tree_map)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_tree_ao_shadows_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, (terra::tree_place_pod_t const *)d_pine, d_pine_counts, pine_capacity,
		(terra::decid_place_pod_t const *)d_decid, d_decid_counts, decid_capacity, d_decid_radius, d_decid_radius_by_id, num_radius_by_id, d_flags, list_capacity,
		d_tree_map, d_updated, d_trmax, d_list_counts); TERRA_CATCH
}
int terra_tiles_tree_ao_shadows(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                                const terra_tree_place *h_pine, const uint32_t *h_pine_counts, uint32_t pine_capacity,
                                const terra_decid_place *h_decid, const uint32_t *h_decid_counts, uint32_t decid_capacity,
                                const float *h_decid_radius, const float *h_decid_radius_by_id, uint32_t num_radius_by_id, const uint8_t *h_flags,
                                uint32_t list_capacity, uint8_t *h_tree_map, uint8_t *h_updated, float *h_trmax, uint32_t *h_list_counts) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_tree_map)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (n == 0) return TERRA_OK;
		bool const has_pine = h_pine_counts && pine_capacity, has_decid = h_decid_counts && decid_capacity;
		if ((has_pine && !h_pine) || (has_decid && !h_decid)) return terra::fail(TERRA_ERR_ARG, "tiles_tree_ao_shadows: counts without records");
		size_t const S = ctx->eng.tile_size(), cb = (size_t)n*4;
		terra_stage st(ctx->eng);
		int const m = st.out(h_tree_map, (size_t)n*(S + 1)*(S + 1)*2),
			p = st.add(h_pine, nullptr, (size_t)n*pine_capacity*sizeof(terra_tree_place), has_pine), pc = st.add(h_pine_counts, nullptr, cb, has_pine),
			e = st.add(h_decid, nullptr, (size_t)n*decid_capacity*sizeof(terra_decid_place), has_decid), ec = st.add(h_decid_counts, nullptr, cb, has_decid),
			r = st.add(h_decid_radius, nullptr, (size_t)n*decid_capacity*4, has_decid && h_decid_radius),
			ri = st.add(h_decid_radius_by_id, nullptr, (size_t)num_radius_by_id*4, has_decid && h_decid_radius_by_id),
			f = st.opt_in(h_flags, n), u = st.out(h_updated, n), t = st.out(h_trmax, cb), l = st.out(h_list_counts, cb);
		st.begin();
		ctx->eng.tiles_tree_ao_shadows_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, st.dev<terra::tree_place_pod_t>(p), st.dev<uint32_t>(pc), pine_capacity,
			st.dev<terra::decid_place_pod_t>(e), st.dev<uint32_t>(ec), decid_capacity, st.dev<float>(r), st.dev<float>(ri), num_radius_by_id,
			st.dev<uint8_t>(f), list_capacity, st.dev<uint8_t>(m), st.dev<uint8_t>(u), st.dev<float>(t), st.dev<uint32_t>(l));
		st.end();
	TERRA_CATCH
}
int terra_tiles_edit_trees_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                               const float pos[3], float radius, int32_t add_trees, int32_t is_square,
                               const uint8_t *d_skip, const terra_tile_stats *d_stats, const float *d_zvals, const uint8_t *d_gen_flags,
                               terra_tree_place *d_pine, uint32_t *d_pine_counts, uint32_t pine_capacity,
                               terra_decid_place *d_decid, uint32_t *d_decid_counts, uint32_t decid_capacity,
                               float *d_decid_radius, const float *d_decid_radius_by_id, uint32_t num_radius_by_id,
                               float *d_trmax, uint8_t *d_status, uint8_t *d_changed, float *d_update_bcube) {
	TERRA_CHECK_CTX if (!pos || (n && (!tile_xy || !d_stats || !d_trmax || !d_status || !d_changed))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_edit_trees_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, pos, radius, add_trees != 0, is_square != 0, d_skip, d_stats, d_zvals, d_gen_flags,
		(terra::tree_place_pod_t *)d_pine, d_pine_counts, pine_capacity, (terra::decid_place_pod_t *)d_decid, d_decid_counts, decid_capacity, d_decid_radius,
		d_decid_radius_by_id, num_radius_by_id, d_trmax, d_status, d_changed, d_update_bcube); TERRA_CATCH
}
int terra_tiles_edit_trees(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, int32_t dxoff, int32_t dyoff, int32_t xoff2, int32_t yoff2,
                           const float pos[3], float radius, int32_t add_trees, int32_t is_square,
                           const uint8_t *h_skip, const terra_tile_stats *h_stats, const float *h_zvals, const uint8_t *h_gen_flags,
                           terra_tree_place *h_pine, uint32_t *h_pine_counts, uint32_t pine_capacity,
                           terra_decid_place *h_decid, uint32_t *h_decid_counts, uint32_t decid_capacity,
                           float *h_decid_radius, const float *h_decid_radius_by_id, uint32_t num_radius_by_id,
                           float *h_trmax, uint8_t *h_status, uint8_t *h_changed, float *h_update_bcube) {
	TERRA_CHECK_CTX if (!pos || (n && (!tile_xy || !h_stats || !h_trmax || !h_status || !h_changed))) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY
		ctx->eng.require_scene();
		ctx->eng.require_tile_size(); // (before the arrays are read: they are sized by S)
		if (n == 0) return TERRA_OK;
		bool const has_pine = h_pine_counts && pine_capacity, has_decid = h_decid_counts && decid_capacity;
		if ((has_pine && !h_pine) || (has_decid && !h_decid)) return terra::fail(TERRA_ERR_ARG, "tiles_edit_trees: counts without records");
		// the cheap refusals before anything is staged (the driver repeats them)
		if (!std::isfinite(radius) || radius < 0.0f) return terra::fail(TERRA_ERR_ARG, "tiles_edit_trees: the radius must be finite and not negative");
		if ((has_pine && (uint64_t)n*pine_capacity > 0xFFFFFFFFull) || (has_decid && (uint64_t)n*decid_capacity > 0xFFFFFFFFull)) return terra::fail(TERRA_ERR_ARG, "tiles_edit_trees: n*capacity must fit 32 bits");
		size_t const Z = (size_t)ctx->eng.tile_size() + 2, cb = (size_t)n*4;
		terra_stage st(ctx->eng);
		int const p = st.inout(h_pine, (size_t)n*pine_capacity*sizeof(terra_tree_place), has_pine), pc = st.inout(h_pine_counts, cb, has_pine),
			e = st.inout(h_decid, (size_t)n*decid_capacity*sizeof(terra_decid_place), has_decid), ec = st.inout(h_decid_counts, cb, has_decid),
			r = st.inout(h_decid_radius, (size_t)n*decid_capacity*4, has_decid && h_decid_radius),
			ri = st.add(h_decid_radius_by_id, nullptr, (size_t)num_radius_by_id*4, has_decid && h_decid_radius_by_id && num_radius_by_id),
			s = st.in(h_stats, (size_t)n*sizeof(terra_tile_stats)), t = st.inout(h_trmax, cb), z = st.opt_in(h_zvals, (size_t)n*Z*Z*sizeof(float)), k = st.opt_in(h_skip, n),
			g = st.opt_in(h_gen_flags, n), u = st.out(h_status, n), c = st.out(h_changed, n), b = st.out(h_update_bcube, 24);
		st.begin();
		ctx->eng.tiles_edit_trees_dev(tile_xy, n, dxoff, dyoff, xoff2, yoff2, pos, radius, add_trees != 0, is_square != 0, st.dev<uint8_t>(k), st.dev<terra_tile_stats>(s),
			st.dev<float>(z), st.dev<uint8_t>(g), st.dev<terra::tree_place_pod_t>(p), st.dev<uint32_t>(pc), pine_capacity, st.dev<terra::decid_place_pod_t>(e), st.dev<uint32_t>(ec),
			decid_capacity, st.dev<float>(r), st.dev<float>(ri), num_radius_by_id, st.dev<float>(t), st.dev<uint8_t>(u), st.dev<uint8_t>(c), st.dev<float>(b));
		st.end();
	TERRA_CATCH
}
int terra_tiles_ao_lighting_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, uint8_t *d_ao) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals || !d_ao)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_ao_lighting_dev(tile_xy, n, d_zvals, d_ao); TERRA_CATCH
}
int terra_tiles_ao_lighting(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, uint8_t *h_ao) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_zvals || !h_ao)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (n == 0) return TERRA_OK;
	TERRA_TRY
		ctx->eng.require_scene(); ctx->eng.require_tile_size();
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const z = st.in(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), a = st.out(h_ao, (size_t)n*(S + 1)*(S + 1));
		st.begin();
		ctx->eng.tiles_ao_lighting_dev(tile_xy, n, st.dev<float>(z), st.dev<uint8_t>(a));
		st.end();
	TERRA_CATCH
}
int terra_tiles_mesh_shadows_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals || !d_smask || !light_pos)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_mesh_shadows_dev(tile_xy, n, d_zvals, light_pos, d_smask); TERRA_CATCH
}
int terra_tiles_mesh_shadows_halo_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask,
	const float *h_edge_in, const uint8_t *h_edge_in_present, float *h_edge_out)
{
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals || !d_smask || !light_pos)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if ((h_edge_in == nullptr) != (h_edge_in_present == nullptr)) return terra::fail(TERRA_ERR_ARG, "edge_in and edge_in_present go together");
	TERRA_TRY ctx->eng.tiles_mesh_shadows_dev(tile_xy, n, d_zvals, light_pos, d_smask, h_edge_in, h_edge_in_present, h_edge_out); TERRA_CATCH
}
int terra_tiles_mesh_shadows_edges_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, const float light_pos[3], uint8_t *d_smask,
	const float *d_edge_in, const uint8_t *h_edge_in_present, float *d_edge_out)
{
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals || !d_smask || !light_pos)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if ((d_edge_in == nullptr) != (h_edge_in_present == nullptr)) return terra::fail(TERRA_ERR_ARG, "edge_in and edge_in_present go together");
	TERRA_TRY ctx->eng.tiles_mesh_shadows_dev(tile_xy, n, d_zvals, light_pos, d_smask, nullptr, h_edge_in_present, nullptr, d_edge_in, d_edge_out); TERRA_CATCH
}
int terra_tiles_mesh_shadows(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, const float light_pos[3], uint8_t *h_smask) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_zvals || !h_smask || !light_pos)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (n == 0) return TERRA_OK;
	TERRA_TRY
		ctx->eng.require_scene(); ctx->eng.require_tile_size();
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const z = st.in(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), m = st.out(h_smask, (size_t)n*(S + 2)*(S + 2));
		st.begin();
		ctx->eng.tiles_mesh_shadows_dev(tile_xy, n, st.dev<float>(z), light_pos, st.dev<uint8_t>(m));
		st.end();
	TERRA_CATCH
}
int terra_tiles_create_zvals_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, uint32_t iters_tt, float *d_zvals, terra_tile_stats *d_stats, uint8_t *d_normals, float *d_min_nz) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_create_zvals_dev(tile_xy, n, iters_tt, d_zvals, d_stats, d_normals, d_min_nz); TERRA_CATCH
}
int terra_tiles_post_dev(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *d_zvals, terra_tile_stats *d_stats, uint8_t *d_normals, float *d_min_nz) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !d_zvals)) return terra::fail(TERRA_ERR_ARG, "null argument");
	TERRA_TRY ctx->eng.tiles_post_dev(tile_xy, n, d_zvals, d_stats, d_normals, d_min_nz); TERRA_CATCH
}
int terra_tiles_post(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, const float *h_zvals, terra_tile_stats *h_stats, uint8_t *h_normals, float *h_min_nz) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_zvals)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (n == 0) return TERRA_OK;
	TERRA_TRY
		ctx->eng.require_scene(); ctx->eng.require_tile_size();
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const z = st.in(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), s = st.opt_out(h_stats, (size_t)n*sizeof(terra_tile_stats)), m = st.opt_out(h_normals, (size_t)n*(S + 1)*(S + 1)*4),
			mn = st.add(nullptr, h_min_nz, (size_t)n*4, h_normals && h_min_nz);
		st.begin();
		ctx->eng.tiles_post_dev(tile_xy, n, st.dev<float>(z), st.dev<terra_tile_stats>(s), st.dev<uint8_t>(m), st.dev<float>(mn));
		st.end();
	TERRA_CATCH
}
int terra_tiles_create_zvals(terra_ctx *ctx, const int32_t *tile_xy, uint32_t n, uint32_t iters_tt, float *h_zvals, terra_tile_stats *h_stats, uint8_t *h_normals, float *h_min_nz) {
	TERRA_CHECK_CTX if (n && (!tile_xy || !h_zvals)) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (n == 0) return TERRA_OK;
	TERRA_TRY
		ctx->eng.require_scene(); ctx->eng.require_tile_size();
		size_t const S = ctx->eng.tile_size();
		terra_stage st(ctx->eng, terra_stage::OWN_ALLOC);
		int const z = st.out(h_zvals, (size_t)n*(S + 2)*(S + 2)*4), s = st.opt_out(h_stats, (size_t)n*sizeof(terra_tile_stats)), m = st.opt_out(h_normals, (size_t)n*(S + 1)*(S + 1)*4),
			mn = st.add(nullptr, h_min_nz, (size_t)n*4, h_normals && h_min_nz);
		st.begin();
		ctx->eng.tiles_create_zvals_dev(tile_xy, n, iters_tt, st.dev<float>(z), st.dev<terra_tile_stats>(s), st.dev<uint8_t>(m), st.dev<float>(mn));
		st.end();
	TERRA_CATCH
}

int terra_tile_size(terra_ctx *ctx, uint32_t *size) {
	TERRA_CHECK_CTX if (!size) return terra::fail(TERRA_ERR_ARG, "null out");
	TERRA_TRY ctx->eng.require_scene(); ctx->eng.require_tile_size(); *size = ctx->eng.tile_size(); TERRA_CATCH
}

int terra_selftest_hot_sqrt(terra_ctx *ctx, uint32_t stride, uint64_t *mismatches) {
	TERRA_CHECK_CTX
	TERRA_TRY
	if (!mismatches) throw std::invalid_argument("terra_selftest_hot_sqrt: null result pointer");
	std::lock_guard<std::recursive_mutex> lk(ctx->eng_mtx);
	*mismatches = ctx->eng.selftest_hot_sqrt(stride);
	return TERRA_OK;
	TERRA_CATCH
}

// ---- voxels
int terra_voxel_fill_dev(terra_ctx *ctx, float *d_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo[3], const float vsz[3], const float off[3],
	float mag, float freq, int rs1, int rs2, int gen_mode, float zscale, int normalize)
{
	TERRA_CHECK_CTX if (!d_out || !lo || !vsz || !off) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (gen_mode < 0 || gen_mode > TERRA_MGEN_DWARP_GPU) return terra::fail(TERRA_ERR_ARG, "bad gen_mode");
	if (!(mag > 0.0f) || !(freq > 0.0f)) return terra::fail(TERRA_ERR_ARG, "voxel_fill: mag and freq must be > 0"); // assert(mag > 0.0 && freq > 0.0), src/upsurface.cpp:19
	TERRA_TRY ctx->eng.voxel_fill_dev(d_out, nx, ny, nz, lo, vsz, off, mag, freq, rs1, rs2, gen_mode, zscale, normalize); TERRA_CATCH
}
int terra_voxel_fill_slab_dev(terra_ctx *ctx, float *d_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo[3], const float vsz[3], const float off[3],
	float mag, float freq, int rs1, int rs2, int gen_mode, float zscale, int normalize, uint32_t y0, uint32_t nys)
{
	TERRA_CHECK_CTX if (!d_out || !lo || !vsz || !off) return terra::fail(TERRA_ERR_ARG, "null argument");
	if (gen_mode < 0 || gen_mode > TERRA_MGEN_DWARP_GPU) return terra::fail(TERRA_ERR_ARG, "bad gen_mode");
	if (!(mag > 0.0f) || !(freq > 0.0f)) return terra::fail(TERRA_ERR_ARG, "voxel_fill: mag and freq must be > 0");
	TERRA_TRY ctx->eng.voxel_fill_dev(d_out, nx, ny, nz, lo, vsz, off, mag, freq, rs1, rs2, gen_mode, zscale, normalize, y0, nys); TERRA_CATCH
}
int terra_voxel_fill(terra_ctx *ctx, float *h_out, uint32_t nx, uint32_t ny, uint32_t nz, const float lo[3], const float vsz[3], const float off[3],
	float mag, float freq, int rs1, int rs2, int gen_mode, float zscale, int normalize)
{
	TERRA_CHECK_CTX if (!h_out) return terra::fail(TERRA_ERR_ARG, "null output");
	size_t const bytes = (size_t)nx*ny*nz*sizeof(float);
	if (bytes == 0) return terra::fail(TERRA_ERR_ARG, "voxel_fill: empty grid");
	float *d = nullptr;
	try {d = (float *)ctx->eng.be.alloc(bytes);} catch (std::exception const &e) {return terra::fail(TERRA_ERR_LIMIT, e.what());}
	int const rc = terra_voxel_fill_dev(ctx, d, nx, ny, nz, lo, vsz, off, mag, freq, rs1, rs2, gen_mode, zscale, normalize);
	if (rc == TERRA_OK) {try {ctx->eng.be.d2h(h_out, d, bytes);} catch (std::exception const &e) {ctx->eng.be.free(d); return terra::fail(TERRA_ERR_HIP, e.what());}}
	ctx->eng.be.free(d);
	return rc;
}

// ---- plumbing
int terra_malloc(terra_ctx *ctx, void **p, size_t bytes) {TERRA_CHECK_CTX if (!p) return terra::fail(TERRA_ERR_ARG, "null out"); TERRA_TRY *p = ctx->eng.be.alloc(bytes ? bytes : 1); TERRA_CATCH}
int terra_free(terra_ctx *ctx, void *p) {TERRA_CHECK_CTX TERRA_TRY if (p) {ctx->eng.be.sync(); ctx->eng.be.free(p);} TERRA_CATCH}
int terra_memcpy_h2d(terra_ctx *ctx, void *d, const void *h, size_t bytes) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.h2d(d, h, bytes); ctx->eng.be.sync(); TERRA_CATCH}
int terra_memcpy_d2h(terra_ctx *ctx, void *h, const void *d, size_t bytes) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.d2h(h, d, bytes); TERRA_CATCH}
int terra_timer_start(terra_ctx *ctx) {TERRA_CHECK_CTX TERRA_TRY ctx->eng.be.timer_start(); TERRA_CATCH}
int terra_timer_stop(terra_ctx *ctx, float *ms) {TERRA_CHECK_CTX TERRA_TRY float const t = ctx->eng.be.timer_stop(); if (ms) *ms = t; TERRA_CATCH}

} // extern "C"
#include "terra_multi.hpp"
#include "terra_dgrid.hpp"
