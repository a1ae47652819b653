// tests/emul/terra_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Builds tests/emul/libterra_emul.so: the SAME host driver (terra_driver.hpp) and the SAME kernel bodies as
// libterra_hip.so, with a backend that runs every "logical thread" in a host loop.  It exists so that the scene start-up,
// the speculative erosion round logic, the tile batching and the argument checking of the C ABI can be tested against
// the oracle on machines without a GPU (`pytest -m "not gpu"`).  It is NOT a fall-back: the 3dworld_amd package never
// loads it, libterra_hip.so contains no host execution path, and terra_create() there fails without a HIP device.
// LDS-tiled fast kernels have no emulation; only their one-thread-per-cell equivalents run here.
#include "../../3dworld_amd/csrc/terra_simple_paths.hpp"
#include <chrono>
#include <stdlib.h>
#include <omp.h>
#include <sys/mman.h>
#include <unistd.h>

struct cpu_backend_t : terra::simple_paths<cpu_backend_t> {
	std::chrono::steady_clock::time_point t0;
	terra::options_t const *opt = nullptr; // the engine's options (terra_set_option)
	void options_changed() {}
	static int device_count() {return 1;}
	void init(int) {}
	void set_stream(void *) {}
	size_t mem_free() {return ~(size_t)0 >> 1;}
	void release_scratch() {}
	void sync() {}
	void *alloc(size_t bytes) {void *p = malloc(bytes ? bytes : 1); if (!p) throw std::bad_alloc(); return p;}
	void free(void *p) {::free(p);}
	void fill32(void *p, uint32_t v, size_t count) {uint32_t *q = (uint32_t *)p; for (size_t i = 0; i < count; ++i) q[i] = v;}
	void h2d(void *d, void const *h, size_t bytes) {memcpy(d, h, bytes);}
	void h2d_async(void *d, void const *h, size_t bytes) {memcpy(d, h, bytes);}
	void d2h(void *h, void const *d, size_t bytes) {memcpy(h, d, bytes);}
	void d2d(void *dst, void const *src, size_t bytes) {memcpy(dst, src, bytes);}
	void download_async(void const *d, void *h, size_t bytes) {memcpy(h, d, bytes);} // every "launch" has finished when it returns
	void download_wait() {}
	static void *host_alloc(size_t bytes) {return malloc(bytes ? bytes : 1);}
	static void host_free(void *p) {::free(p);}
	void copy_from_peer(void *dst, cpu_backend_t &, void const *src, size_t bytes) {memcpy(dst, src, bytes);}
	void enable_peer(cpu_backend_t &) {}
	bool can_map(cpu_backend_t const &) const {return map_peers;} // TERRA_EMUL_NO_PEER_MAP=1: take the staged-copy path of the multi-context mesh shadows
	bool map_peers = !(getenv("TERRA_EMUL_NO_PEER_MAP") && getenv("TERRA_EMUL_NO_PEER_MAP")[0] == '1');
	// the host analog of the device's virtual memory management (terra_dgrid): a strip is a memfd, a grid a PROT_NONE reservation that the strips are mapped into
	// (MAP_SHARED | MAP_FIXED), the shareable handle the file descriptor itself -- so two emulator PROCESSES really share a grid, like two ranks share HBM
	int device = 0;
	struct vm_handle_t {int fd;};
	size_t vm_granularity() {return (size_t)sysconf(_SC_PAGESIZE);}
	void *vm_create(size_t bytes) {
		int const fd = memfd_create("terra_dgrid_strip", 0);
		if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) {if (fd >= 0) close(fd); throw std::runtime_error("memfd_create / ftruncate failed");}
		return new vm_handle_t{fd};
	}
	int vm_export_fd(void *h) {int const fd = dup(((vm_handle_t *)h)->fd); if (fd < 0) throw std::runtime_error("dup failed"); return fd;}
	void *vm_import_fd(int fd) {int const d = dup(fd); if (d < 0) throw std::runtime_error("dup failed"); return new vm_handle_t{d};}
	void *vm_reserve(size_t total, size_t) {void *p = mmap(nullptr, total, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0); if (p == MAP_FAILED) throw std::bad_alloc(); return p;}
	void vm_map(void *base, size_t off, void *h, size_t bytes) {
		if (mmap((uint8_t *)base + off, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, ((vm_handle_t *)h)->fd, 0) == MAP_FAILED) throw std::runtime_error("mmap of a strip failed");
	}
	static void vm_set_access(void *, size_t, int const *, size_t) {}
	static void vm_unmap(void *base, size_t off, size_t bytes) {(void)mmap((uint8_t *)base + off, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED | MAP_NORESERVE, -1, 0);}
	static void vm_release(void *h) {if (h) {close(((vm_handle_t *)h)->fd); delete (vm_handle_t *)h;}}
	static void vm_free(void *base, size_t total) {if (base) munmap(base, total);}
	void *event_create() {return malloc(1);} // every "launch" has finished when it returns: events order nothing here
	void event_record(void *) {}
	void event_wait(void *) {}
	static void event_destroy(void *e) {::free(e);}
	static void event_synchronize(void *) {}
	void timer_start() {t0 = std::chrono::steady_clock::now();}
	float timer_stop() {return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();}
	template<class F> void launch_waves_nolds(size_t n, F f) {for (size_t i = 0; i < n; ++i) f(i);}
	void tile_shadows(terra::shadow_consts_t const &c, uint32_t cnt, uint32_t const *ord, int32_t const *adj, uint32_t n, float const *z, unsigned long long *out, uint8_t *sm, uint32_t np) {tile_shadows_simple(c, cnt, ord, adj, n, z, out, sm, np);}
	void fill8(void *p, uint8_t v, size_t count) {memset(p, v, count);}
	bool graph_replay(void const *, size_t) {return false;} // no graphs here: every launch runs at once
	bool graph_begin() {return false;}
	void graph_end(void const *, size_t) {}
	void graph_abort() {}
	// sequential on purpose: bodies use non-atomic stand-ins for atomics (terra_erosion.hpp)
	template<class F> void launch(size_t n, F f, int = 256) {for (size_t i = 0; i < n; ++i) f(i);}
	// a "wave" is one call; its LDS scratch is a few stack arrays
	template<class F> void launch_waves(size_t n, F f) {
		std::vector<float> win(terra::EW*terra::EW); std::vector<uint8_t> dirty(terra::EW*terra::EW); terra::wave_shared_t sh;
		terra::wave_scratch_t const ws{win.data(), dirty.data(), &sh};
		for (size_t i = 0; i < n; ++i) f(i, ws);
	}

	template<class F> void launch_waves_lean(size_t n, F f) {
		std::vector<float> win(terra::EW*terra::EW); std::vector<uint8_t> dirty(terra::EW*terra::EW); terra::lean_shared_t sh;
		terra::lean_scratch_t const ws{win.data(), dirty.data(), &sh};
		for (size_t i = 0; i < n; ++i) f(i, ws);
	}

	bool sine_grid(terra::grid_job_t const &job, terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float const *xt, float const *yt, float const *smx, float const *smy, float *out, uint32_t *) {sine_grid_simple(job, nc, L, xt, yt, smx, smy, out); return false;}
	bool noise_grid(terra::grid_job_t const &job, terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float const *smx, float const *smy, float *out, uint32_t *, uint32_t const *) {noise_grid_simple(job, nc, L, smx, smy, out); return false;}
	void tile_grid(uint32_t n, terra::tile_ref_pod_t const *refs, uint32_t nux, uint32_t nuy, float const *xt, float const *yt, uint32_t nxpv, uint32_t nypv, float const *d_sm, float const *d_m0, int md, int shp, int kstart, bool use_sm, float so,
		terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float dxv, float dyv, float *zvals, bool /*plain_only*/, uint32_t tw, bool /*unique_tiles*/, bool glaciate = true, uint32_t const * = nullptr, int fused = 0, float = 0.0f, terra::tile_band_t const * = nullptr) {tile_grid_simple(n, refs, nux, nuy, xt, yt, nxpv, nypv, d_sm, d_m0, md, shp, kstart, use_sm, so, nc, L, dxv, dyv, zvals, tw, glaciate, fused);}
	void tile_erosion(uint32_t n, float *zvals, terra::erosion_consts_t const &ec, uint32_t iters) {
		// tiles cycle through the three implementations: wave-cooperative whole-tile-in-LDS (k_tile_erosion's body; lanes run sequentially here), scalar, wave + window
		std::vector<float> padded((size_t)ec.NX*ec.NY);
		for (uint32_t t = 0; t < n; ++t) {
			float *z = zvals + (size_t)t*ec.xsize*ec.ysize;
			if ((t % 3) == 1) {tile_erosion_simple(1, z, ec, iters, padded.data()); continue;}   // scalar cross-check path
			if ((t % 3) == 2) {tile_erosion_windowed(1, z, ec, iters, padded.data()); continue;} // wave + LDS window over the padded copy
			for (int Z = 0; Z < ec.NY; ++Z) for (int X = 0; X < ec.NX; ++X) {
				padded[(size_t)Z*ec.NX + X] = z[(size_t)terra::imax(terra::imin(Z - terra::EROSION_PAD, ec.ysize-1), 0)*ec.xsize + terra::imax(terra::imin(X - terra::EROSION_PAD, ec.xsize-1), 0)];
			}
			terra::wave_lds_mem_t m; m.pad = padded.data(); m.NX = ec.NX; m.NY = ec.NY;
			for (uint32_t it = 0; it < iters; ++it) {terra::simulate_droplet((int)it, m, ec);}
			for (int y = 0; y < ec.ysize; ++y) for (int x = 0; x < ec.xsize; ++x) {
				z[(size_t)y*ec.xsize + x] = terra::max_std(ec.min_zval, padded[(size_t)(y + terra::EROSION_PAD)*ec.NX + x + terra::EROSION_PAD]);
			}
		}
	}
	void minmax(float const *vals, size_t n, uint32_t *d) {minmax_simple(vals, n, d);}
	void quantize16(float const *vals, size_t n, float val_add, float val_div, uint8_t *pix) {quantize16_simple(vals, n, val_add, val_div, pix);}
	// the pair evaluation of the HIP kernel (k_voxel_noise) over the same table, serially: columns x (z, z + 1) pairs
	void voxel_noise(float *out, size_t nvox, terra::vox_noise_job_t const &J, bool perlin, bool /*fused: the exact values are within every tolerance*/, uint32_t const *lut3) {
		size_t const ncol = nvox / J.nz;
		for (size_t col = 0; col < ncol; ++col) {
			unsigned const x = (unsigned)(col % J.nx), y = (unsigned)(col / J.nx) + J.y0;
			for (unsigned z = 0; z < J.nz; z += 2) {
				terra::nv2 const v = perlin ? terra::voxel_noise_pair<true>(x, y, z, J, (char const *)lut3) : terra::voxel_noise_pair<false>(x, y, z, J, (char const *)lut3);
				out[col*J.nz + z] = v[0];
				if (z + 1 < J.nz) {out[col*J.nz + z + 1] = v[1];}
			}
		}
	}
	void voxel_sines(float *out, uint32_t nx, uint32_t ny, uint32_t nz, float const *d_tab, float zscale, int normalize, int fused = 0, float = 0.0f, float const * = nullptr, uint32_t = 0) {voxel_sines_simple(out, nx, ny, nz, d_tab, zscale, normalize, fused);}
};
typedef cpu_backend_t terra_backend_t;
#include "../../3dworld_amd/csrc/terra_api_impl.hpp"


// glibc_powf (terra_powf.hpp) against the build host's libm over n pseudo-random arguments: [0,2) ^ {typical exponents}, then raw bit patterns
extern "C" unsigned long long terra_emul_powf_mismatches(unsigned long long n, uint32_t seed) {
	unsigned long long bad = 0;
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	float const exps[] = {2.5f, 0.5f, 1.7f, 3.3f, 0.01f, 7.9f, -1.5f, 2.0f, 3.0f, 1.0f};
	for (unsigned long long i = 0; i < n; ++i) {
		float x, y;
		if (i & 1) {x = (float)(rnd() >> 8)*(1.0f/16777216.0f)*2.0f; y = exps[(i >> 1) % 10];}
		else {uint32_t const ux = rnd(), uy = rnd(); memcpy(&x, &ux, 4); memcpy(&y, &uy, 4); if (i & 2) {y = (float)((int)(rnd() % 41) - 20)*0.5f;}}
		float const a = powf(x, y), b = terra::glibc_powf(x, y);
		if (memcmp(&a, &b, 4) != 0 && !(a != a && b != b)) {++bad;}
	}
	return bad;
}

// the division-free lattice helpers of terra_noise.hpp against the divisions they replace
extern "C" unsigned long long terra_emul_noise_helper_mismatches() {
	unsigned long long bad = 0;
	uint32_t seed = 99;
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	for (int i = -400; i <= 700; ++i) {float const h = (float)i, a = h/41.0f, b = terra::gl_div41(h); if (memcmp(&a, &b, 4) != 0) ++bad;}
	for (int i = -600000; i <= 600000; ++i) {float const v = (float)i, a = terra::gl_mod(v, 289.0f), b = terra::gl_mod289_int(v); if (memcmp(&a, &b, 4) != 0) ++bad;}
	for (int i = 0; i < 4000000; ++i) {
		float const v = (float)((int)(rnd() >> 7) - (1 << 24)); // integers in [-2^24, 2^24): both sides of the 2^23 switch to the division
		float const a = terra::gl_mod(v, 289.0f), b = terra::gl_mod289_int(v);
		if (memcmp(&a, &b, 4) != 0) ++bad;
	}
	// the table look-ups' residue (terra_noise.hpp: gl_mod289_raw / gl_mod289_small): every integer below 2^22 in magnitude
	for (int i = -4194304; i <= 4194304; ++i) {
		float const v = (float)i, a = terra::gl_mod(v, 289.0f), r = terra::gl_mod289_raw(v), sm = terra::gl_mod289_small(v);
		if (memcmp(&a, &sm, 4) != 0) ++bad;
		if (!(r == a || (r == 289.0f && a == 0.0f))) ++bad;
	}
	float const special[] = {INFINITY, -INFINITY, NAN, 1e30f, -1e30f, 8388608.0f, -8388608.0f, 8388607.0f};
	for (float v : special) {float const a = terra::gl_mod(v, 289.0f), b = terra::gl_mod289_int(v); if (memcmp(&a, &b, 4) != 0 && !(a != a && b != b)) ++bad;}
	return bad;
}

// the table-driven lattice noise of the grid kernels (simplex2_lut / perlin2_lut over noise_lut_fill) against the direct evaluation: bit-identical
// on random positions at every octave scale, on positions that straddle the lattice columns / rows where mod 289 wraps (cx = 288 -> 289 vs 0),
// beyond the 2^22 switch to the direct code, and through the whole fBm / domain-warp evaluation
extern "C" unsigned long long terra_emul_noise_lut_mismatches(unsigned n, uint32_t seed) {
	unsigned long long bad = 0;
	std::vector<uint32_t> tab(terra::NOISE_LUT_DWORDS + 4);
	uint32_t *t = (uint32_t *)(((uintptr_t)tab.data() + 15) & ~(uintptr_t)15);
	for (unsigned i = 0; i < terra::NOISE_LUT_DWORDS; ++i) {t[i] = terra::noise_lut_fill(i);}
	terra::noise_tab_t const ns{(char const *)t, (char const *)(t + terra::NOISE_LUT_S_DWORDS)};
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	auto rf = [&](float lo, float hi) {return lo + (hi - lo)*(float)(rnd() >> 8)*(1.0f/16777216.0f);};
	auto same = [&](float a, float b) {return memcmp(&a, &b, 4) == 0 || (a != a && b != b);};
	terra::noise_consts_t nc{};
	nc.mesh_scale = 1.0f; nc.start_eval_sin = 10; nc.rx = 1.3f; nc.ry = 1.7f; nc.MESH_HEIGHT = 0.1f; nc.mesh_height_scale = 0.7f; nc.mesh_scale_z_inv = 1.0f;
	nc.hp.plat_bot = 1000.0f; nc.hp.crat_h = 1000.0f;
	for (unsigned i = 0; i < n; ++i) {
		float x0, y0, x1, y1;
		unsigned const kind = i % 6;
		if (kind == 0) {float const s = 3e6f; x0 = rf(-s, s); x1 = rf(-s, s); y0 = rf(-s, s); y1 = rf(-s, s);}            // around the 2^22 switch
		else if (kind == 1) {float const s = 1e8f; x0 = rf(-s, s); x1 = rf(-s, s); y0 = rf(-s, s); y1 = rf(-s, s);}       // far beyond it
		else if (kind == 2) {                                                                                             // next to the wrap columns / rows: lattice coordinate 289*k - 1 .. 289*k + 1
			float const kx = (float)((int)(rnd() % 41) - 20)*289.0f, ky = (float)((int)(rnd() % 41) - 20)*289.0f;
			x0 = kx + rf(-1.5f, 1.5f); x1 = kx + rf(-1.5f, 1.5f); y0 = ky + rf(-1.5f, 1.5f); y1 = ky + rf(-1.5f, 1.5f);
			if (i & 8) {y0 = rf(-400.0f, 400.0f);} if (i & 16) {x1 = rf(-400.0f, 400.0f);}
		}
		else {float const s = (kind == 3) ? 300.0f : ((kind == 4) ? 3.0f : 30000.0f); x0 = rf(-s, s); x1 = rf(-s, s); y0 = rf(-s, s); y1 = rf(-s, s);}
		terra::nv2 const xs = {x0, x1}, ys = {y0, y1};
		terra::nv2 const s2 = ns.simplex(xs, ys), p2 = ns.perlin(xs, ys);
		if (!same(s2[0], terra::simplex2(x0, y0)) || !same(s2[1], terra::simplex2(x1, y1))) ++bad;
		if (!same(p2[0], terra::perlin2(x0, y0)) || !same(p2[1], terra::perlin2(x1, y1))) ++bad;
		if ((i & 31) == 0) {
			int const shape = (int)(i >> 5) % 3;
			float const sc = 1.0f/0.0007f; // grid coordinates whose noise-space image is x0, y0
			terra::nv2 const gx = {x0*sc, x1*sc}, gy = {y0*sc, y1*sc};
			terra::noise_oct_t const oc = terra::make_noise_oct(nc);
			terra::nv2 const a = terra::noise_zval_tab<terra::MGEN_DWARP_GPU>(gx, gy, shape, nc, oc, ns), b = terra::noise_zval_tab<terra::MGEN_PERLIN>(gx, gy, shape, nc, oc, ns);
			if (!same(a[0], terra::noise_zval<terra::MGEN_DWARP_GPU>(gx[0], gy[0], shape, nc)) || !same(a[1], terra::noise_zval<terra::MGEN_DWARP_GPU>(gx[1], gy[1], shape, nc))) ++bad;
			if (!same(b[0], terra::noise_zval<terra::MGEN_PERLIN>(gx[0], gy[0], shape, nc)) || !same(b[1], terra::noise_zval<terra::MGEN_PERLIN>(gx[1], gy[1], shape, nc))) ++bad;
		}
	}
	// every hashed lattice point once, simplex and Perlin, incl. the 288 | 289 column: positions at the cell centres of a 300 x 300 lattice patch
	for (int cy = -5; cy < 295; ++cy) {
		for (int cx = -5; cx < 295; cx += 2) {
			terra::nv2 const xs = {(float)cx + 0.37f, (float)(cx + 1) + 0.81f}, ys = {(float)cy + 0.29f, (float)cy + 0.63f};
			terra::nv2 const p2 = ns.perlin(xs, ys), s2 = ns.simplex(xs, ys);
			if (!same(p2[0], terra::perlin2(xs[0], ys[0])) || !same(p2[1], terra::perlin2(xs[1], ys[1]))) ++bad;
			if (!same(s2[0], terra::simplex2(xs[0], ys[0])) || !same(s2[1], terra::simplex2(xs[1], ys[1]))) ++bad;
		}
	}
	return bad;
}

// the 3-D table-driven lattice noise of the voxel-field kernel (perlin3_lut_z2 / simplex3_lut over noise3_lut_fill) against the direct evaluation: bit-identical on random
// positions at several scales, next to the lattice planes where mod 289 wraps, beyond the 2^22 switch to the direct code, and on every hash value (a 300^2 x 4 lattice patch)
extern "C" unsigned long long terra_emul_noise3_lut_mismatches(unsigned n, uint32_t seed) {
	unsigned long long bad = 0;
	std::vector<uint32_t> tab(2*terra::NOISE3_LUT_DWORDS + 4);
	uint32_t *t = (uint32_t *)(((uintptr_t)tab.data() + 15) & ~(uintptr_t)15);
	for (unsigned i = 0; i < 2*terra::NOISE3_LUT_DWORDS; ++i) {t[i] = terra::noise3_lut_fill(i % terra::NOISE3_LUT_DWORDS, i >= terra::NOISE3_LUT_DWORDS);}
	char const *ts = (char const *)t, *tp = (char const *)(t + terra::NOISE3_LUT_DWORDS);
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	auto rf = [&](float lo, float hi) {return lo + (hi - lo)*(float)(rnd() >> 8)*(1.0f/16777216.0f);};
	auto same = [&](float a, float b) {return memcmp(&a, &b, 4) == 0 || (a != a && b != b);};
	auto check = [&](float x0, float y0, float z0, float x1, float y1, float z1) {
		terra::nv2 const p = terra::perlin3_lut_z2<true>(x0, y0, terra::nv2{z0, z1}, tp);
		if (!same(p[0], terra::perlin3(x0, y0, z0)) || !same(p[1], terra::perlin3(x0, y0, z1))) ++bad;
		terra::nv2 const s = terra::simplex3_lut<true>(terra::nv2{x0, x1}, terra::nv2{y0, y1}, terra::nv2{z0, z1}, ts);
		if (!same(s[0], terra::simplex3(x0, y0, z0)) || !same(s[1], terra::simplex3(x1, y1, z1))) ++bad;
	};
	for (unsigned i = 0; i < n; ++i) {
		unsigned const kind = i % 6;
		float v[6];
		if (kind == 0) {for (float &f : v) {f = rf(-3e6f, 3e6f);}}       // around the 2^22 switch
		else if (kind == 1) {for (float &f : v) {f = rf(-1e8f, 1e8f);}}  // far beyond it
		else if (kind == 2) {                                            // next to the wrap planes: lattice coordinate 289*k - 1 .. 289*k + 1
			for (float &f : v) {f = (float)((int)(rnd() % 41) - 20)*289.0f + rf(-1.5f, 1.5f);}
			if (i & 8) {v[1] = rf(-400.0f, 400.0f);} if (i & 16) {v[5] = rf(-400.0f, 400.0f);}
		}
		else {float const s = (kind == 3) ? 300.0f : ((kind == 4) ? 3.0f : 30000.0f); for (float &f : v) {f = rf(-s, s);}}
		check(v[0], v[1], v[2], v[3], v[4], v[5]);
	}
	for (int cz = -2; cz < 2; ++cz) { // every (x, y) lattice column incl. the 288 | 289 planes, a few z planes around 0 and around the wrap
		for (int cy = -5; cy < 295; ++cy) {
			for (int cx = -5; cx < 295; ++cx) {
				float const zb = (float)(cz + ((cy & 1) ? 289 : 0));
				check((float)cx + 0.37f, (float)cy + 0.29f, zb + 0.41f, (float)cx + 0.81f, (float)cy + 0.63f, zb + 1.17f);
			}
		}
	}
	return bad;
}

// the block records of the regular fBm sums (noise_blocktab_build / fbm2_bt) against the direct evaluation: a "block" = a rows x cols patch of a regular grid with
// random origin, cell spacing and octave count; every cell of the patch must give the bits of fbm2_t.  Also counts how often the records did not fit (the caller's fall-back).
extern "C" unsigned long long terra_emul_noise_blocktab_mismatches(unsigned nblocks, uint32_t seed, unsigned *fallbacks) {
	unsigned long long bad = 0;
	std::vector<uint32_t> tab(terra::NOISE_LUT_DWORDS + 4);
	uint32_t *t = (uint32_t *)(((uintptr_t)tab.data() + 15) & ~(uintptr_t)15);
	for (unsigned i = 0; i < terra::NOISE_LUT_DWORDS; ++i) {t[i] = terra::noise_lut_fill(i);}
	char const *stab = (char const *)t, *ptab = (char const *)(t + terra::NOISE_LUT_S_DWORDS);
	std::vector<float> rec(terra::NOISE_BT_FLOATS);
	terra::noise_bt_meta_t meta[terra::NUM_FREQ_COMP];
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	auto rf = [&](float lo, float hi) {return lo + (hi - lo)*(float)(rnd() >> 8)*(1.0f/16777216.0f);};
	auto same = [&](float a, float b) {return memcmp(&a, &b, 4) == 0 || (a != a && b != b);};
	unsigned nfall = 0;
	for (unsigned b = 0; b < nblocks; ++b) {
		terra::noise_consts_t nc{};
		nc.mesh_scale = 1.0f; nc.start_eval_sin = 10*(int)(rnd() % 4); nc.rx = rf(1.0f, 2.0f); nc.ry = rf(1.0f, 2.0f);
		terra::noise_oct_t const oc = terra::make_noise_oct(nc);
		unsigned const cols = 128, rows = 16;
		float const step = (b % 5 == 4) ? rf(0.0005f, 0.01f) : 0.0007f*rf(0.5f, 2.0f); // noise-space distance between cells (mesh_scale 0.5 .. 2; sometimes far coarser: the records may not fit)
		float const ox = (b % 7 == 6) ? (float)((int)(rnd() % 41) - 20)*289.0f/oc.freq[oc.end_octave - 1] : rf(-3000.0f, 3000.0f)*step, oy = rf(-3000.0f, 3000.0f)*step; // some origins next to a mod-289 wrap column
		auto vx = [&](unsigned x) {return ox + (float)x*step;};
		auto vy = [&](unsigned y) {return oy + (float)y*step;};
		int const shape = (int)(b % 3);
		for (int simplex = 0; simplex < 2; ++simplex) {
			bool const ok = simplex ? terra::noise_blocktab_build<true>(vx(0), vy(0), vx(cols - 1), vy(rows - 1), oc, stab, rec.data(), meta, 0, 1)
			                        : terra::noise_blocktab_build<false>(vx(0), vy(0), vx(cols - 1), vy(rows - 1), oc, ptab, rec.data(), meta, 0, 1);
			if (!ok) {++nfall; continue;}
			terra::noise_btab_t const bt{rec.data(), meta};
			for (unsigned y = 0; y < rows; ++y) {
				for (unsigned x = 0; x < cols; x += 2) {
					terra::nv2 const xs = {vx(x), vx(x + 1)}, ys = {vy(y), vy(y)};
					terra::nv2 const a = simplex ? terra::fbm2_bt<true>(xs, ys, shape, oc, bt) : terra::fbm2_bt<false>(xs, ys, shape, oc, bt);
					for (int e = 0; e < 2; ++e) {
						float const d = simplex ? terra::fbm2<true>(xs[e], ys[e], shape, oc.end_octave, nc.rx, nc.ry) : terra::fbm2<false>(xs[e], ys[e], shape, oc.end_octave, nc.rx, nc.ry);
						if (!same(a[e], d)) ++bad;
					}
				}
			}
		}
	}
	if (fallbacks) *fallbacks = nfall;
	return bad;
}

// the two-cells-per-lane instantiation of the 2-D lattice noise against the one-cell instantiation (must be bit-identical)
extern "C" unsigned long long terra_emul_noise_x2_mismatches(unsigned n, uint32_t seed) {
	unsigned long long bad = 0;
	auto rnd = [&]() {seed = seed*1664525u + 1013904223u; return seed;};
	auto rf = [&](float lo, float hi) {return lo + (hi - lo)*(float)(rnd() >> 8)*(1.0f/16777216.0f);};
	auto same = [&](float a, float b) {return memcmp(&a, &b, 4) == 0 || (a != a && b != b);};
	terra::noise_consts_t nc{};
	nc.mesh_scale = 1.0f; nc.start_eval_sin = 10; nc.rx = 1.3f; nc.ry = 1.7f; nc.MESH_HEIGHT = 0.1f; nc.mesh_height_scale = 0.7f; nc.mesh_scale_z_inv = 1.0f;
	nc.hp.plat_bot = 1000.0f; nc.hp.crat_h = 1000.0f;
	for (unsigned i = 0; i < n; ++i) {
		float const scale = (i & 3) == 0 ? 1e7f : ((i & 3) == 1 ? 3e4f : 300.0f); // incl. coordinates beyond the 2^23 switch of mod 289
		float const x0 = rf(-scale, scale), x1 = rf(-scale, scale), y0 = rf(-scale, scale), y1 = rf(-scale, scale);
		terra::nv2 const xs = {x0, x1}, ys = {y0, y1};
		terra::nv2 const s2 = terra::simplex2_t<terra::nv2>(xs, ys), p2 = terra::perlin2_t<terra::nv2>(xs, ys);
		if (!same(s2[0], terra::simplex2(x0, y0)) || !same(s2[1], terra::simplex2(x1, y1))) ++bad;
		if (!same(p2[0], terra::perlin2(x0, y0)) || !same(p2[1], terra::perlin2(x1, y1))) ++bad;
		if ((i & 15) == 0) {
			int const shape = (int)(i >> 4) % 3;
			terra::nv2 const a = terra::noise_zval_t<terra::MGEN_DWARP_GPU, terra::nv2>(xs, ys, shape, nc), b = terra::noise_zval_t<terra::MGEN_PERLIN, terra::nv2>(xs, ys, shape, nc);
			if (!same(a[0], terra::noise_zval<terra::MGEN_DWARP_GPU>(x0, y0, shape, nc)) || !same(a[1], terra::noise_zval<terra::MGEN_DWARP_GPU>(x1, y1, shape, nc))) ++bad;
			if (!same(b[0], terra::noise_zval<terra::MGEN_PERLIN>(x0, y0, shape, nc)) || !same(b[1], terra::noise_zval<terra::MGEN_PERLIN>(x1, y1, shape, nc))) ++bad;
		}
	}
	return bad;
}
