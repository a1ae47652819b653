// terra_hip.hip -- libterra_hip.so: HIP backend (gfx950 / MI355X) + the C ABI of include/terra.h.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off terra_hip.hip -o libterra_hip.so
// (see 3dworld_amd/build.py).  There is no host execution path in this library: every entry point needs a HIP device.
#include "terra_kernels.hpp"
#include "terra_fused.hpp"
#include "terra_fz_api.hpp"
#include "terra_simple_paths.hpp"
#include "terra_xfer.hpp"
#include <stdlib.h>

#define TERRA_HIP_CHECK(expr) do {hipError_t const e_ = (expr); if (e_ != hipSuccess) {throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));}} while (0)

struct hip_backend_t : terra::simple_paths<hip_backend_t> {
	int device = -1;
	hipStream_t stream = nullptr, own_stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	static constexpr bool has_kernels = true; // the driver tries the bool tile_*() hooks below before its own one-thread-per-tile forms
	terra::options_t const *opt = nullptr; // the engine's options (terra_set_option), set by terra_engine() before init(): read where they are used, never copied
	int num_cus = 256;
	// the grow-only device buffers (terra_stage.hpp: dev_buf_t): tile erosion's padded copies, its land counts + launch order, k_tile_post's per-tile accumulators,
	// tile_grid's (column, row) -> tile map, the voxel sine field's P array, the split tables of TERRA_GEN_FAST
	terra::dev_buf_t tile_pad, tile_order, tile_acc, tile_map, vox_p, h3_tab;
	template<class F> void for_each_buf(F f) {for (terra::dev_buf_t *b : {&tile_pad, &tile_order, &tile_acc, &tile_map, &vox_p, &h3_tab}) {f(*b);}} // the one list of them: what release_scratch() and the destructor walk

	static int device_count() {int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n;}
	void init(int dev) {
		device = dev;
		TERRA_HIP_CHECK(hipSetDevice(dev));
		TERRA_HIP_CHECK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
		stream = own_stream;
		TERRA_HIP_CHECK(hipEventCreate(&ev0)); TERRA_HIP_CHECK(hipEventCreate(&ev1));
		{int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) {num_cus = n;} else {(void)hipGetLastError();}}
		options_changed();
		// LDS-tiled kernels use > 64 KiB of dynamic LDS (160 KiB per CU on gfx950)
		TERRA_HIP_CHECK(hipFuncSetAttribute((void const *)terra::k_tile_erosion, hipFuncAttributeMaxDynamicSharedMemorySize, 96*1024));
		TERRA_HIP_CHECK(hipFuncSetAttribute((void const *)terra::k_tile_shadows_level, hipFuncAttributeMaxDynamicSharedMemorySize, 96*1024));
		TERRA_HIP_CHECK(hipFuncSetAttribute((void const *)terra::k_tile_shadows_flow, hipFuncAttributeMaxDynamicSharedMemorySize, 96*1024));
		TERRA_HIP_CHECK(hipFuncSetAttribute((void const *)terra::k_tile_ao<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64*1024));
		TERRA_HIP_CHECK(hipFuncSetAttribute((void const *)terra::k_tile_ao<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64*1024));
		// the whole context of a tile in one workgroup's LDS (162 408 of the CU's 163 840 bytes); a runtime that refuses the size leaves the band kernel in charge
		ao_tile_ok = hipFuncSetAttribute((void const *)terra::k_tile_ao_tile<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)terra::AOT_LDS) == hipSuccess
			&& hipFuncSetAttribute((void const *)terra::k_tile_ao_tile<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)terra::AOT_LDS) == hipSuccess;
		if (!ao_tile_ok) {(void)hipGetLastError();}
	}
	void options_changed() { // (the engine has drained the stream)
		if (graphs_enabled != (opt->graphs != 0)) {for (graph_slot_t &g : graphs) {graph_drop(g);} graphs_enabled = opt->graphs != 0;}
	}
	~hip_backend_t() {
		if (pin) (void)hipHostFree(pin);
		for_each_buf([&](terra::dev_buf_t &b) {b.drop(*this);});
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
		for (graph_slot_t &g : graphs) {graph_drop(g);}
		if (relay_ev) (void)hipEventDestroy(relay_ev);
		if (side_stream) (void)hipStreamDestroy(side_stream);
		if (own_stream) (void)hipStreamDestroy(own_stream);
	}
	size_t mem_free() {use(); size_t f = 0, t = 0; if (hipMemGetInfo(&f, &t) != hipSuccess) {(void)hipGetLastError(); return ~(size_t)0 >> 1;} return f;}
	void release_scratch() {for_each_buf([&](terra::dev_buf_t &b) {b.drop(*this);});} // the backend's own grow-only buffers (the caller has drained the stream)
	void use() {TERRA_HIP_CHECK(hipSetDevice(device));}
	void set_stream(void *s) {sync(); pin_off = 0; stream = s ? (hipStream_t)s : own_stream;} // cached graphs are stream-agnostic (the stream is given at launch)
	void sync() {use(); TERRA_HIP_CHECK(hipStreamSynchronize(stream));}
	void *alloc(size_t bytes) {use(); void *p = nullptr; TERRA_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1)); return p;}
	void free(void *p) {use(); (void)hipFree(p);}
	void fill8(void *p, uint8_t v, size_t count) {use(); if (count) TERRA_HIP_CHECK(hipMemsetAsync(p, v, count, stream));}
	void fill32(void *p, uint32_t v, size_t count) {use(); if (count) TERRA_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)p, (int)v, count, stream));}
	// host buffers are ordinary pageable memory (often stack variables): copies are stream-ordered and then waited for
	void h2d(void *d, void const *h, size_t bytes) {
		use();
		if (bytes >= BIG_XFER) {xfer.submit(device, stream, const_cast<void *>(h), d, bytes, true, [this](hipEvent_t e) {return record_via_side(e);}); xfer.wait_all(); return;} // (the host waits: later kernels of any stream see the data)
		TERRA_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream)); TERRA_HIP_CHECK(hipStreamSynchronize(stream));
	}
	// small parameter blocks (tile references, per-column constants, dependency orders): staged through a pinned ring and copied asynchronously, stream-ordered -- the
	// host does not wait (a pageable hipMemcpyAsync + hipStreamSynchronize per upload was ~10 % of a 0.68 ms tile batch).  The ring drains the stream when it wraps.
	uint8_t *pin = nullptr; size_t pin_bytes = 0, pin_off = 0; bool pin_failed = false; // pin_failed: the pinned allocation was refused once -- not retried on every upload
	void h2d_async(void *d, void const *h, size_t bytes) {
		if (bytes == 0) return;
		use();
		if (!pin && !pin_failed) {pin_bytes = (size_t)8 << 20; if (hipHostMalloc((void **)&pin, pin_bytes, hipHostMallocDefault) != hipSuccess) {pin = nullptr; pin_bytes = 0; pin_failed = true; (void)hipGetLastError();}}
		size_t const need = terra::stage_up(bytes);
		if (!pin || need > pin_bytes/2) {h2d(d, h, bytes); return;}
		if (pin_off + need > pin_bytes) {TERRA_HIP_CHECK(hipStreamSynchronize(stream)); pin_off = 0;}
		memcpy(pin + pin_off, h, bytes);
		TERRA_HIP_CHECK(hipMemcpyAsync(d, pin + pin_off, bytes, hipMemcpyHostToDevice, stream));
		pin_off += need;
	}
	void d2h(void *h, void const *d, size_t bytes) {
		use();
		if (bytes >= BIG_XFER) {download_async(d, h, bytes); download_wait(); return;} // whole grids: banded, K streams, pinned staging (terra_xfer.hpp)
		TERRA_HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream)); TERRA_HIP_CHECK(hipStreamSynchronize(stream));
	}
	// ---- big host <-> device transfers (terra_xfer.hpp): stream-ordered behind the work enqueued so far, asynchronous to the host and to the context's later kernels
	static constexpr size_t BIG_XFER = (size_t)16 << 20;
	terra::xfer_engine_t xfer;
	void download_async(void const *d, void *h, size_t bytes) {use(); xfer.submit(device, stream, h, const_cast<void *>(d), bytes, false, [this](hipEvent_t e) {return record_via_side(e);});}
	void download_wait() {xfer.wait_all();}
	static void *host_alloc(size_t bytes) {void *p = nullptr; if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {(void)hipGetLastError(); return nullptr;} return p;}
	static void host_free(void *p) {if (p) (void)hipHostFree(p);}
	// device-to-device copies on this context's stream: inside the device, and from another context's device (several GPUs in one process, terra_multi.hpp)
	void d2d(void *dst, void const *src, size_t bytes) {use(); TERRA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));}
	void copy_from_peer(void *dst, hip_backend_t &src_be, void const *src, size_t bytes) {
		use();
		if (src_be.device == device) {TERRA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));}
		else {TERRA_HIP_CHECK(hipMemcpyPeerAsync(dst, device, src, src_be.device, bytes, stream));} // xGMI when peer access is on, staged through the host otherwise
	}
	std::vector<int> peers_mapped; // devices whose memory this device's kernels may address (hipDeviceEnablePeerAccess succeeded)
	void enable_peer(hip_backend_t &other) { // best effort
		if (other.device == device) return;
		int can = 0;
		if (hipDeviceCanAccessPeer(&can, device, other.device) != hipSuccess || !can) return;
		if (hipSetDevice(device) != hipSuccess) return;
		hipError_t const e = hipDeviceEnablePeerAccess(other.device, 0);
		if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {(void)hipGetLastError(); return;}
		if (std::find(peers_mapped.begin(), peers_mapped.end(), other.device) == peers_mapped.end()) {peers_mapped.push_back(other.device);}
	}
	bool can_map(hip_backend_t const &other) const {return other.device == device || std::find(peers_mapped.begin(), peers_mapped.end(), other.device) != peers_mapped.end();}
	// ---- virtual memory management (terra_dgrid: ONE grid whose row strips live on several GPUs, mapped back to back in one address range).
	// A strip is a physical allocation on its device (hipMemCreate) that can leave the process as a POSIX file descriptor; every process (or every device of one
	// process) reserves a range, maps all strips into it in order and enables access for its own device: kernels then address the whole grid through one plain pointer and
	// rows that live on another GPU are reached over xGMI by ordinary loads and stores.
	hipMemAllocationProp vm_prop() const {
		hipMemAllocationProp p; memset(&p, 0, sizeof(p));
		p.type = hipMemAllocationTypePinned; p.requestedHandleTypes = hipMemHandleTypePosixFileDescriptor;
		p.location.type = hipMemLocationTypeDevice; p.location.id = device;
		return p;
	}
	size_t vm_granularity() {use(); hipMemAllocationProp const p = vm_prop(); size_t g = 0; TERRA_HIP_CHECK(hipMemGetAllocationGranularity(&g, &p, hipMemAllocationGranularityRecommended)); return g ? g : ((size_t)2 << 20);}
	void *vm_create(size_t bytes) {use(); hipMemAllocationProp const p = vm_prop(); hipMemGenericAllocationHandle_t h = nullptr; TERRA_HIP_CHECK(hipMemCreate(&h, bytes, &p, 0)); return (void *)h;}
	int vm_export_fd(void *h) {use(); int fd = -1; TERRA_HIP_CHECK(hipMemExportToShareableHandle((void *)&fd, (hipMemGenericAllocationHandle_t)h, hipMemHandleTypePosixFileDescriptor, 0)); return fd;}
	// The runtime that PyTorch 2.10 brings along (HIP 7.0: what a process that imported torch runs on) takes a POINTER to the descriptor; the system runtime of ROCm 7.2 (what a
	// plain C / C++ process such as 3DWorld links) takes the descriptor itself, as CUDA does, and reports the pointer form as "invalid argument" -- found with
	// tools/bench_native_onegrid.c.  The pointer form is tried first (the value form would make an older runtime dereference a small integer).
	void *vm_import_fd(int fd) {
		use();
		hipMemGenericAllocationHandle_t h = nullptr;
		hipError_t e = hipMemImportFromShareableHandle(&h, (void *)&fd, hipMemHandleTypePosixFileDescriptor);
		int ver = 0;
		if (e == hipErrorInvalidValue && hipRuntimeGetVersion(&ver) == hipSuccess && ver >= 70200000) {
			(void)hipGetLastError();
			h = nullptr;
			e = hipMemImportFromShareableHandle(&h, (void *)(uintptr_t)fd, hipMemHandleTypePosixFileDescriptor);
		}
		if (e != hipSuccess) {throw std::runtime_error(std::string("hipMemImportFromShareableHandle (descriptor by pointer and by value): ") + hipGetErrorString(e));}
		return (void *)h;
	}
	void *vm_reserve(size_t total, size_t align) {use(); void *p = nullptr; TERRA_HIP_CHECK(hipMemAddressReserve(&p, total, align, nullptr, 0)); return p;}
	void vm_map(void *base, size_t off, void *h, size_t bytes) {use(); TERRA_HIP_CHECK(hipMemMap((uint8_t *)base + off, bytes, 0, (hipMemGenericAllocationHandle_t)h, 0));}
	static void vm_set_access(void *base, size_t total, int const *devices, size_t n) {
		std::vector<hipMemAccessDesc> d(n);
		for (size_t i = 0; i < n; ++i) {memset(&d[i], 0, sizeof(d[i])); d[i].location.type = hipMemLocationTypeDevice; d[i].location.id = devices[i]; d[i].flags = hipMemAccessFlagsProtReadWrite;}
		TERRA_HIP_CHECK(hipMemSetAccess(base, total, d.data(), n));
	}
	static void vm_unmap(void *base, size_t off, size_t bytes) {(void)hipMemUnmap((uint8_t *)base + off, bytes);}
	static void vm_release(void *h) {if (h) (void)hipMemRelease((hipMemGenericAllocationHandle_t)h);}
	static void vm_free(void *base, size_t total) {if (base) (void)hipMemAddressFree(base, total);}
	// stream-level ordering between contexts (terra_event_*): an event recorded on one context's stream, waited for by another's -- the host never blocks
	void *event_create() {use(); hipEvent_t e = nullptr; TERRA_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return (void *)e;}
	// An event that another THREAD may wait for on the host (terra_event_synchronize) must not be "last recorded" in a stream that later enters graph capture -- the runtime
	// then refuses the wait and poisons the capture (hipErrorStreamCaptureUnsupported; the erosion schedulers capture their rounds on first use) -- so the record goes through
	// a side stream of the context that never captures: [stream: relay event] -> [side stream: wait relay, record e]
	hipStream_t side_stream = nullptr; hipEvent_t relay_ev = nullptr;
	hipError_t record_via_side(hipEvent_t e) {
		hipError_t r = hipSuccess;
		if (!side_stream) {
			if ((r = hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking)) != hipSuccess) return r;
			if ((r = hipEventCreateWithFlags(&relay_ev, hipEventDisableTiming)) != hipSuccess) return r;
		}
		if ((r = hipEventRecord(relay_ev, stream)) != hipSuccess) return r;
		if ((r = hipStreamWaitEvent(side_stream, relay_ev, 0)) != hipSuccess) return r;
		return hipEventRecord(e, side_stream);
	}
	void event_record(void *e) {use(); TERRA_HIP_CHECK(record_via_side((hipEvent_t)e));}
	void event_wait(void *e) {use(); TERRA_HIP_CHECK(hipStreamWaitEvent(stream, (hipEvent_t)e, 0));}
	static void event_destroy(void *e) {if (e) (void)hipEventDestroy((hipEvent_t)e);}
	static void event_synchronize(void *e) {TERRA_HIP_CHECK(hipEventSynchronize((hipEvent_t)e));}
	void timer_start() {use(); TERRA_HIP_CHECK(hipEventRecord(ev0, stream));}
	float timer_stop() {use(); TERRA_HIP_CHECK(hipEventRecord(ev1, stream)); TERRA_HIP_CHECK(hipEventSynchronize(ev1)); float ms = 0; TERRA_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1)); return ms;}

	// ---- hipGraph cache: a fixed sequence of small dependent launches (one speculative-erosion round) is captured once and replayed with a
	// single hipGraphLaunch.  `key` = every byte the captured closures depend on; the caller re-captures when it changes.
	struct graph_slot_t {std::vector<uint8_t> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; uint64_t last_use = 0;};
	std::vector<graph_slot_t> graphs; uint64_t graph_clock = 0; bool capturing = false; bool graphs_enabled = true;
	void graph_drop(graph_slot_t &g) {if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); g.exec = nullptr; g.graph = nullptr; g.key.clear();}
	bool graph_replay(void const *key, size_t n) {
		if (!graphs_enabled) return false;
		for (graph_slot_t &g : graphs) {
			if (g.exec && g.key.size() == n && memcmp(g.key.data(), key, n) == 0) {use(); g.last_use = ++graph_clock; TERRA_HIP_CHECK(hipGraphLaunch(g.exec, stream)); return true;}
		}
		return false;
	}
	bool graph_begin() { // false: graphs are off, the caller's launches simply run
		if (!graphs_enabled) return false;
		use();
		TERRA_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
		capturing = true;
		return true;
	}
	void graph_abort() {if (capturing) {hipGraph_t g = nullptr; (void)hipStreamEndCapture(stream, &g); if (g) (void)hipGraphDestroy(g); capturing = false;}}
	void graph_end(void const *key, size_t n) { // instantiate, remember (16 slots -- a tracer context of the one-grid pipeline holds one per grid in flight --, least recently used goes), launch
		hipGraph_t g = nullptr;
		capturing = false;
		TERRA_HIP_CHECK(hipStreamEndCapture(stream, &g));
		hipGraphExec_t ex = nullptr;
		hipError_t const e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
		if (e != hipSuccess) {(void)hipGraphDestroy(g); throw std::runtime_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));}
		graph_slot_t *slot = nullptr;
		if (graphs.size() < 16) {graphs.emplace_back(); slot = &graphs.back();}
		else {slot = &graphs[0]; for (graph_slot_t &c : graphs) {if (c.last_use < slot->last_use) slot = &c;} graph_drop(*slot);}
		slot->key.assign((uint8_t const *)key, (uint8_t const *)key + n); slot->graph = g; slot->exec = ex; slot->last_use = ++graph_clock;
		TERRA_HIP_CHECK(hipGraphLaunch(ex, stream));
	}

	// every kernel launch of this file: on the context's stream and checked at once, so a refused launch stops a pass before the launches that depend on it.
	// No use(): a method calls it once at entry
	template<class K, class... A> void run(K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
		hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
		TERRA_HIP_CHECK(hipGetLastError());
	}
	template<class F> static void with_noise_mode(int md, F f) { // f(the fBm mode as a compile-time constant): the kernels are templates over it
		switch (md) {
		case terra::MGEN_PERLIN:      f(std::integral_constant<int, terra::MGEN_PERLIN>()); break;
		case terra::MGEN_DWARP_GPU:   f(std::integral_constant<int, terra::MGEN_DWARP_GPU>()); break;
		case terra::MGEN_SIMPLEX_GPU: f(std::integral_constant<int, terra::MGEN_SIMPLEX_GPU>()); break;
		default:                      f(std::integral_constant<int, terra::MGEN_SIMPLEX>()); break;
		}
	}

	template<class F> void launch(size_t n, F f, int block = 256) {
		if (n == 0) return;
		use();
		size_t const nblocks = (n + block - 1)/block;
		if (nblocks > 0x7FFFFFFFull) throw std::invalid_argument("launch: grid too large");
		run(terra::k_generic<F>, dim3((unsigned)nblocks), dim3(block), 0, n, f);
	}

	template<class F> void launch_waves(size_t n, F f) {
		if (n == 0) return;
		use();
		if (n > 0x7FFFFFFFull) throw std::invalid_argument("launch_waves: grid too large");
		run(terra::k_waves<F>, dim3((unsigned)n), dim3(64), 0, f, 0u);
	}

	template<class F> void launch_waves_lean(size_t n, F f) { // one 64-lane workgroup per item with the lean droplet scratch (terra_kernels.hpp: k_waves_lean)
		if (n == 0) return;
		use();
		if (n > 0x7FFFFFFFull) throw std::invalid_argument("launch_waves: grid too large");
		run(terra::k_waves_lean<F>, dim3((unsigned)n), dim3(64), 0, f);
	}

	template<class F> void launch_waves_nolds(size_t n, F f) { // one 64-lane workgroup per item, no LDS scratch (does not compete with LDS-heavy kernels for a CU)
		if (n == 0) return;
		use();
		if (n > 0x7FFFFFFFull) throw std::invalid_argument("launch_waves: grid too large");
		run(terra::k_waves_nolds<F>, dim3((unsigned)n), dim3(64), 0, f);
	}

	// TERRA_GEN_FAST (terra_fused.hpp: k_sine_grid_h3): split the f32 tables of J (k-major, rows padded to nxp / nyp) into scaled half-precision pairs and run the contraction on
	// the half-precision matrix pipe.  amax_y / amax_x: the largest magnitude the row / column table can hold.  Returns false when the tables are too large for its 32-bit offsets.
	static float h3_scale(float amax) {int e = 0; if (amax > 0.0f && amax < 3.0e38f) {(void)frexpf(amax, &e);} return ldexpf(1.0f, 14 - e);} // amax < 2^e: scaled magnitudes stay below 2^14
	// vox_tab: (voxels) noise_gen_3d's [entry][nsines] sine table with the field's nx, ny -- the split tables are then made straight from it (J.xt / J.yt unused)
	template<int KIND> bool sine_grid_h3(terra::sgf_job_t J, float amax_x, float amax_y, float const *vox_tab = nullptr, uint32_t vnx = 0, uint32_t vny = 0) {
		int const nk = (J.kstart < J.kend) ? J.kend - J.kstart : 0;
		uint32_t const nchunks = (uint32_t)((3*nk + 15)/16);
		if ((uint64_t)std::max(J.nxp, J.nyp)*32u*(nchunks + 1) >= 0xFFFFFFFFull) return false;
		size_t const bx = (size_t)nchunks*J.nxp*32u, by = (size_t)nchunks*J.nyp*32u;
		float const sx = h3_scale(amax_x), sy = h3_scale(amax_y);
		J.xh = h3_tab.grow(*this, bx + by + 64); J.yh = (char const *)J.xh + bx; J.nchunks = nchunks; J.unscale = 1.0f/(sx*sy);
		if (nchunks && vox_tab) {
			run(terra::k_split_voxel_table<false, terra::VOX_SINES>, dim3((J.nxp + 255)/256), dim3(256), 0, vox_tab, vnx, vny, J.nx, J.nxp, sx, (terra::sgh_u4 *)J.xh);
			run(terra::k_split_voxel_table<true, terra::VOX_SINES>, dim3((J.nyp + 255)/256), dim3(256), 0, vox_tab, vnx, vny, J.nx, J.nyp, sy, (terra::sgh_u4 *)J.yh);
		}
		else if (nchunks) {
			run(terra::k_split_table<false>, dim3((unsigned)(((size_t)nchunks*J.nxp + 255)/256)), dim3(256), 0, J.xt, J.nxp, J.kstart, J.kend, nchunks, sx, (terra::sgh_u4 *)J.xh);
			run(terra::k_split_table<true>, dim3((unsigned)(((size_t)nchunks*J.nyp + 255)/256)), dim3(256), 0, J.yt, J.nyp, J.kstart, J.kend, nchunks, sy, (terra::sgh_u4 *)J.yh);
		}
		if (KIND == terra::SGF_VOXELS && J.nx <= 64 && (J.nyp % 256u) == 0) {J.narrow = 1; J.ntx = 1; J.nty = J.nyp/256u;} // (rows beyond ny: zero table rows, nothing stored)
		unsigned const nb = J.ntx*J.nty, grid = ((nb + 7)/8)*8;
		run(terra::k_sine_grid_h3<KIND>, dim3(grid), dim3(256), 0, J);
		return true;
	}
	// the job of the matrix-pipe sum (k_sine_grid_mx / k_sine_grid_h3) over a grid job's tables; a tile batch adds its map
	terra::sgf_job_t make_sgf_job(terra::grid_job_t const &job, terra::noise_consts_t const &nc, float const *xt, float const *yt, float const *smx, float const *smy, float *out, uint32_t *mm, unsigned ntx, unsigned nty) const {
		terra::sgf_job_t J; memset(&J, 0, sizeof(J));
		J.xt = xt; J.yt = yt; J.smx = smx; J.smy = smy; J.out = out; J.mm = mm; J.nx = job.nx; J.ny = job.ny; J.nxp = job.nxp; J.nyp = job.nyp; J.ntx = ntx; J.nty = nty; J.rowgroup = (unsigned)opt->sg_rowgroup;
		J.kstart = job.kstart; J.kend = terra::F_TABLE_SIZE; J.glaciate = (job.glaciate && nc.glaciate) ? 1 : 0; J.sine_mag = (job.glaciate && job.use_sine_mag) ? 1 : 0;
		J.zmax_est = nc.zmax_est; J.zmax_est2 = nc.zmax_est2; J.zmax_est2_inv = nc.zmax_est2_inv; J.sine_offset = job.sine_offset;
		return J;
	}
	// mm (optional): device uint32[2] pre-set to 0xFFFFFFFF receiving min f2ord(z) / min ~f2ord(z); returns false when the caller must run minmax() itself
	bool sine_grid(terra::grid_job_t const &job, terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float const *xt, float const *yt, float const *smx, float const *smy, float *out, uint32_t *mm) {
		if (opt->simple_kernels) {sine_grid_simple(job, nc, L, xt, yt, smx, smy, out); return false;}
		use();
		unsigned const ntx = job.nxp/terra::SG_BX, nty_all = (job.ny + terra::SG_BY - 1)/terra::SG_BY;
		if ((job.tyn || job.ty0) && (job.fused || job.tyn == 0 || job.ty0 >= nty_all || job.tyn > nty_all - job.ty0)) throw std::invalid_argument("sine_grid: a tile-row window must lie inside the grid (the fused kernels take whole grids only)");
		unsigned const nty = job.tyn ? job.tyn : nty_all; // the launch's tile rows: the kernel adds job.ty0 (grid_job_t: a window of the grid, the whole of it by default)
		unsigned const nb = ntx*nty, grid = ((nb + 7)/8)*8;
		if (job.fused) { // TERRA_GEN_FUSED: the sum on the f32 matrix pipe, persistent blocks (two per CU: 225 registers per lane)
			terra::sgf_job_t const J = make_sgf_job(job, nc, xt, yt, smx, smy, out, mm, ntx, nty);
			if (job.fused == 2 && sine_grid_h3<terra::SGF_GRID>(J, 1.0f, job.fast_amax)) return true; // TERRA_GEN_FAST (|SINF| <= 1 bounds the x table)
			run(terra::k_sine_grid_mx<terra::SGF_GRID>, dim3(std::min(grid, (unsigned)(2*num_cus + 7)/8*8)), dim3(256), 0, J);
			return true;
		}
		terra::sg_tiles_t const tl{nullptr, nullptr, 0, (unsigned)opt->sg_rowgroup, 0, 0, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0};
		if (job.plain_only) {
			auto const go = [&](auto kern) {run(kern, dim3(grid), dim3(terra::SG_THREADS), 0, job, nc, L, xt, yt, smx, smy, out, ntx, nty, mm, tl);};
			if ((job.nx & 3u) == 0) { // rows of whole 16-byte groups: the packed epilogue, and nothing else in the kernel
				if (opt->sg_kc == 27) {
					// the row-scalar form (terra_kernels.hpp: k_sine_grid_rs): blocks of 256 columns x 64 rows, the window's 128-row tile rows as two block rows each, "sg.rowgroup"
					// tile rows walked together as twice as many block rows.  The other chunk lengths ("sg.kc" 20 / 45) stay on k_sine_grid: the same bits either way
					unsigned const first = terra::job_window_first(job), end = terra::job_window_end(job);
					unsigned const ntx2 = (job.nxp + terra::SGR_BX - 1)/terra::SGR_BX, nty2 = (end - first + terra::SGR_BY - 1)/terra::SGR_BY, nb2 = ntx2*nty2;
					run(terra::k_sine_grid_rs<27>, dim3(((nb2 + 7)/8)*8), dim3(terra::SG_THREADS), 0, job, nc, xt, yt, smx, smy, out, ntx2, nty2, 2u*(unsigned)opt->sg_rowgroup, mm);
				}
				else if (opt->sg_kc == 20) go(terra::k_sine_grid<false, false, 20>); else go(terra::k_sine_grid<false, false, 45>);
			}
			else { // any other row length: the same sum with the per-cell epilogue, instantiations of their own
				if (opt->sg_kc == 27) go(terra::k_sine_grid<false, false, 27, false>); else if (opt->sg_kc == 20) go(terra::k_sine_grid<false, false, 20, false>); else go(terra::k_sine_grid<false, false, 45, false>);
			}
		}
		else                {run(terra::k_sine_grid<false, true>, dim3(grid), dim3(terra::SG_THREADS), 0, job, nc, L, xt, yt, smx, smy, out, ntx, nty, mm, tl);}
		return true;
	}
	bool noise_grid(terra::grid_job_t const &job, terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float const *smx, float const *smy, float *out, uint32_t *mm, uint32_t const *nlut) {
		if (opt->simple_kernels) {noise_grid_simple(job, nc, L, smx, smy, out); return false;}
		use();
		if (job.fused) {TERRA_HIP_CHECK((hipError_t)terra_fz_noise_grid(job.mode, &job, &nc, &L, smx, smy, out, mm, nlut, (void *)stream)); return true;} // TERRA_GEN_FUSED: the contraction-allowed build (terra_fz.hip)
		dim3 const grid((job.nx + 127)/128, (job.ny + terra::NG_ROWS - 1)/terra::NG_ROWS), block(256); // 64 lanes x 2 cells per row segment, 4 rows at a time, NG_ROWS rows per block
		terra::noise_oct_t const oc = terra::make_noise_oct(nc);
		with_noise_mode(job.mode, [&](auto m) {run(terra::k_noise_grid<decltype(m)::value>, grid, block, 0, job, nc, L, smx, smy, out, mm, nlut, oc);});
		return true;
	}
	// may a band of the tiles' fields be evaluated instead of whole squares?  Only where tile_grid takes the packed epilogue of the plain sine kernel (the one that knows bands)
	bool tile_band_ok(uint32_t n, uint32_t nux, uint32_t nuy, uint32_t twx, bool unique_tiles, bool plain_only, int md) const {
		return !opt->simple_kernels && md == terra::MGEN_SINE && unique_tiles && plain_only && (uint64_t)n*2 >= (uint64_t)nux*nuy && ((nux*twx) & 3u) == 0 && opt->sg_kc_tiles == 27 && opt->ao_bands != 0;
	}
	void tile_grid(uint32_t n, terra::tile_ref_pod_t const *refs, uint32_t nux, uint32_t nuy, float const *xt, float const *yt, uint32_t nxpv, uint32_t nypv, float const *d_sm, float const *d_m0,
		int md, int shp, int kstart, bool use_sm, float so, terra::noise_consts_t const &nc, terra::sin_lut_t const &L, float dxv, float dyv, float *zvals, bool plain_only, uint32_t tw, bool unique_tiles, bool glaciate = true, uint32_t const *nlut = nullptr, int fused = 0, float fast_amax = 0.0f,
		terra::tile_band_t const *band = nullptr) // band (tile_band_ok() said yes): tw = the band's cells per tile in x
	{
		// sine mode and a batch that fills at least half of (distinct tile columns) x (distinct tile rows): ONE LDS-tiled k_sine_grid launch over the
		// virtual grid, scattered into the per-tile layout.  Sparse batches and the fBm modes are per-cell anyway.
		if (!opt->simple_kernels && md != terra::MGEN_SINE) { // fBm modes: per-cell work, two cells per lane
			use();
			terra::grid_job_t job;
			job.mx0 = 0; job.my0 = 0; job.mdx = dxv; job.mdy = dyv; job.nx = job.ny = tw; job.nxp = nxpv; job.nyp = nypv;
			job.mode = md; job.shape = shp; job.kstart = kstart; job.glaciate = glaciate ? 1 : 0; job.use_sine_mag = use_sm ? 1 : 0; job.sine_offset = so; job.plain_only = 0;
			if (fused) {TERRA_HIP_CHECK((hipError_t)terra_fz_noise_tiles(refs, n, nux, d_sm, d_m0, &job, &nc, &L, zvals, tw, nlut, (void *)stream)); return;} // "gen.fused"
			terra::noise_oct_t const oc = terra::make_noise_oct(nc);
			size_t const threads = (size_t)n*tw*((tw + 1)/2);
			dim3 const grid((unsigned)((threads + 255)/256)), block(256);
			with_noise_mode(md, [&](auto m) {run(terra::k_noise_tiles<decltype(m)::value>, grid, block, 0, refs, n, nux, d_sm, d_m0, job, nc, L, zvals, tw, nlut, oc);});
			return;
		}
		if (opt->simple_kernels || md != terra::MGEN_SINE || !unique_tiles || (uint64_t)n*2 < (uint64_t)nux*nuy || ((uintptr_t)zvals & 7)) {tile_grid_simple(n, refs, nux, nuy, xt, yt, nxpv, nypv, d_sm, d_m0, md, shp, kstart, use_sm, so, nc, L, dxv, dyv, zvals, tw, glaciate, fused); return;}
		use();
		size_t const cnt = (size_t)nux*nuy;
		int32_t *tm = (int32_t *)tile_map.grow(*this, cnt*sizeof(int32_t));
		fill32(tm, 0xFFFFFFFFu, cnt);
		launch(n, [=] TERRA_LAMBDA (size_t i) {terra::tile_ref_pod_t const r = refs[i]; tm[(size_t)r.yi*nux + r.xi] = (int32_t)i;});
		terra::grid_job_t job;
		job.mx0 = 0; job.my0 = 0; job.mdx = dxv; job.mdy = dyv; job.nx = nux*tw; job.ny = nuy*(band ? band->twy : tw); job.nxp = nxpv; job.nyp = nypv;
		job.mode = terra::MGEN_SINE; job.shape = shp; job.kstart = kstart; job.glaciate = glaciate ? 1 : 0; job.use_sine_mag = use_sm ? 1 : 0; job.sine_offset = so;
		unsigned const ntx = job.nxp/terra::SG_BX, nty = (job.ny + terra::SG_BY - 1)/terra::SG_BY, nb = ntx*nty, grid = ((nb + 7)/8)*8;
		terra::sg_tiles_t tl{tm, d_m0, nux, (unsigned)opt->sg_rowgroup, tw, tw, tw, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0};
		if (band) {tl.twy = band->twy; tl.ostride = band->ostride; tl.xsplit = band->xsplit; tl.xgap = band->xgap; tl.ysplit = band->ysplit; tl.ygap = band->ygap; fused = 0;}
		job.plain_only = plain_only ? 1 : 0;
		if (fused && plain_only) { // "gen.fused": the batch's virtual grid on the matrix pipe, scattered into the per-tile layout
			terra::sgf_job_t J = make_sgf_job(job, nc, xt, yt, d_sm, d_sm + (size_t)nux*tw, zvals, nullptr, ntx, nty);
			J.tile_map = tm; J.nux = nux; J.tw = tw;
			if (fused == 2 && sine_grid_h3<terra::SGF_TILES>(J, 1.0f, fast_amax)) return;
			run(terra::k_sine_grid_mx<terra::SGF_TILES>, dim3(std::min(grid, (unsigned)(2*num_cus + 7)/8*8)), dim3(256), 0, J);
			return;
		}
		int const kc_tiles = opt->sg_kc_tiles; // 27: three chunks, 29.7 KB per block (measured on the 64 x 64 batch: 291.8 -> 283.9 us, the 201-wide AO context 735 -> 706 us); "sg.kc_tiles" 45: two chunks, 48 KB.  The same sum either way
		if (plain_only && kc_tiles == 27) {run(terra::k_sine_grid<true, false, 27>, dim3(grid), dim3(terra::SG_THREADS), 0, job, nc, L, xt, yt, d_sm, d_sm + (size_t)nux*tw, zvals, ntx, nty, (uint32_t *)nullptr, tl);}
		else if (plain_only) {run(terra::k_sine_grid<true, false>, dim3(grid), dim3(terra::SG_THREADS), 0, job, nc, L, xt, yt, d_sm, d_sm + (size_t)nux*tw, zvals, ntx, nty, (uint32_t *)nullptr, tl);}
		else            {run(terra::k_sine_grid<true, true>, dim3(grid), dim3(terra::SG_THREADS), 0, job, nc, L, xt, yt, d_sm, d_sm + (size_t)nux*tw, zvals, ntx, nty, (uint32_t *)nullptr, tl);}
	}
	// the whole batch in one dataflow launch (k_tile_shadows_flow); sync_words: the ticket counter, zeroed here.  false: use the per-level launches.  Leaves SHADOW_EDGE_PUB set in `out`
	// the lane order of the shadow kernels (terra::shadow_lane_order) for the last light / tile geometry seen: the per-level launches of a batch ask for it once per level
	terra::shadow_consts_t lanes_key; uint32_t lanes_np = 0; bool lanes_ok = false; terra::shadow_lanes_t lanes_cached;
	bool shadow_lanes(terra::shadow_consts_t const &c, uint32_t np, terra::shadow_lanes_t &lanes) {
		if (lanes_np != np || memcmp(&lanes_key, &c, sizeof(c)) != 0) {
			memset(&lanes_key, 0, sizeof(lanes_key)); memcpy(&lanes_key, &c, sizeof(c)); lanes_np = np;
			lanes_ok = terra::shadow_lane_order(c, np, terra::SH_LEVEL_THREADS, lanes_cached.path);
		}
		lanes = lanes_cached;
		return lanes_ok;
	}
	// The LDS kernels: their layout is for tiles of 130 cells a side (S = 128), the block ORs its mask out a word at a time.  Every level of a batch must take the same
	// path (the LDS kernels order a sweep's edge writes with stride 1024, tile_shadows_simple with 4096): the choice depends only on the batch's constants
	bool shadow_kernels_ok(terra::shadow_consts_t const &c, uint8_t const *sm, uint32_t np, terra::shadow_lanes_t &lanes) {
		return !opt->simple_kernels && c.xsize == 130 && !((uintptr_t)sm & 3) && shadow_lanes(c, np, lanes);
	}
	bool tile_shadows_flow(terra::shadow_consts_t const &c, uint32_t ntiles, uint32_t nslots, uint32_t const *ord, int32_t const *adj, float const *z, unsigned long long *out, uint8_t *sm, uint32_t np, uint32_t *sync_words) {
		terra::shadow_lanes_t lanes;
		if (opt->shadows_levels || !shadow_kernels_ok(c, sm, np, lanes)) return false;
		use();
		fill32(sync_words, 0u, 1); // the ticket (the edge arrays were zeroed by the caller: no stale `published` bit)
		unsigned const grid = std::min<unsigned>(ntiles, (unsigned)(2*num_cus));
		run(terra::k_tile_shadows_flow, dim3(grid), dim3(terra::SH_LEVEL_THREADS), terra::SH_LEVEL_LDS, c, nslots, ntiles, ord, adj, z, out, sm, np, sync_words, lanes);
		return true;
	}
	void tile_shadows(terra::shadow_consts_t const &c, uint32_t cnt, uint32_t const *ord, int32_t const *adj, uint32_t n, float const *z, unsigned long long *out, uint8_t *sm, uint32_t np) {
		terra::shadow_lanes_t lanes;
		if (!shadow_kernels_ok(c, sm, np, lanes)) {tile_shadows_simple(c, cnt, ord, adj, n, z, out, sm, np); return;}
		use();
		run(terra::k_tile_shadows_level, dim3(cnt), dim3(terra::SH_LEVEL_THREADS), terra::SH_LEVEL_LDS, c, n, ord, adj, z, out, sm, np, lanes);
	}
	bool ao_tile_ok = false;
	void tile_ao_pass(uint32_t n, float const *z, float const *ctx, uint8_t *ao, float dz, bool own, uint32_t S) {
		if (opt->simple_kernels || S != 128) {tile_ao_simple(n, z, ctx, ao, dz, own, S); return;} // (the kernels' LDS layout is for 130-cell tiles)
		use();
		if (ao_tile_ok && opt->ao_whole) { // one workgroup per tile, the context staged once
			unsigned const grid = std::min<unsigned>(n, (unsigned)num_cus); // persistent: a CU holds one of these workgroups
			if (own) {run(terra::k_tile_ao_tile<true>, dim3(grid), dim3(terra::AOT_THREADS), terra::AOT_LDS, z, ctx, ao, dz, n);}
			else {run(terra::k_tile_ao_tile<false>, dim3(grid), dim3(terra::AOT_THREADS), terra::AOT_LDS, z, ctx, ao, dz, n);}
			return;
		}
		unsigned const nbands = (terra::AO_TEX + terra::AO_BAND - 1)/terra::AO_BAND;
		size_t const lds = (size_t)(terra::AO_BAND + terra::AO_RL)*terra::AO_CS*sizeof(float);
		if (own) {run(terra::k_tile_ao<true>, dim3(n*nbands), dim3(terra::AO_THREADS), lds, z, ctx, ao, dz);}
		else {run(terra::k_tile_ao<false>, dim3(n*nbands), dim3(terra::AO_THREADS), lds, z, ctx, ao, dz);}
	}
	// k_tile_post (S = 128, LDS-staged: the zvals 16-byte aligned), else k_tile_post_sized, else tile_post_simple; both kernels store texels as words
	void tile_post_pass(uint32_t n, terra::tile_ref_pod_t const *refs, float const *z, terra_tile_stats *st, uint8_t *nm, float *mnz, float wpz, float rad_c, float dxv, float dyv, float dxy, uint32_t S) {
		float const c2 = dxy*dxy;
		// the kernels take min_normal_z from the largest |n|^2 and never look at get_norm's "mag < TOLERANCE" branch: a texel's mag is >= sqrtf(dxdy*dxdy) (a sum that only grows, monotone roundings)
		bool const normalized = !(sqrtf(c2) < 1.0E-12f) && dxy > 0.0f;
		bool const kernels = !opt->simple_kernels && !((uintptr_t)nm & 3) && normalized;
		bool const tuned = kernels && S == 128 && !((uintptr_t)z & 15), sized = kernels && (uint64_t)n*4 <= 0x7FFFFFFFull;
		if (!tuned && !sized) {tile_post_simple(n, refs, z, st, nm, mnz, wpz, rad_c, dxv, dyv, dxy, S); return;}
		use();
		uint32_t flat_word; // the texel of a flat cell (n = (+-0, +-0, dxdy): the ocean floor), by the reference's statements
		{
			float nv[3]; terra::tile_normal_v(0.0f, 0.0f, 0.0f, dxv, dyv, dxy, nv);
			flat_word = (uint32_t)(uint8_t)(127.0*((double)nv[0] + 1.0)) | ((uint32_t)(uint8_t)(127.0*((double)nv[1] + 1.0)) << 8) | ((uint32_t)(uint8_t)(127.0*((double)nv[2] + 1.0)) << 16);
		}
		uint32_t *const acc = (uint32_t *)tile_acc.grow(*this, (size_t)n*terra::TP_ACC*sizeof(uint32_t));
		run(terra::k_tile_post_init, dim3((n*terra::TP_ACC + 255)/256), dim3(256), 0, acc, n);
		if (tuned) {run(terra::k_tile_post, dim3(n*4), dim3(terra::TP_THREADS), 0, refs, z, st, nm, acc, wpz, dxv, dyv, dxy, c2, flat_word);}
		else {run(terra::k_tile_post_sized, dim3(n*4), dim3(terra::TPS_THREADS), 0, refs, z, st, nm, acc, wpz, dxv, dyv, dxy, c2, flat_word, S);}
		run(terra::k_tile_post_final, dim3((n + 255)/256), dim3(256), 0, refs, n, st, mnz, acc, rad_c, dxy, nm ? 1 : 0, S);
	}
	void tile_erosion(uint32_t n, float *zvals, terra::erosion_consts_t const &ec, uint32_t iters) {
		use();
		size_t const lds = (size_t)ec.NX*ec.NY*sizeof(float);
		// default: the whole clamp-padded tile resident in LDS (76 KB, 2 tiles per CU; measured 126 ms for 4096 tiles x 1000 droplets);
		// option "tile_erosion" = "window": a 32x32 LDS window over an HBM/L2-resident copy (10 KB, ~15 tiles per CU; 141 ms: the batch is bound by its
		// heaviest land tiles, ~50k dependent droplet steps each, not by occupancy).  Grids too large for LDS always use the window.
		bool const use_lds = !opt->tile_erosion_window && lds <= 96*1024;
		if (!use_lds) {
			float *const pad = (float *)tile_pad.grow(*this, (size_t)n*lds);
			if (opt->simple_kernels) {tile_erosion_simple(n, zvals, ec, iters, pad);} // cross-check path: one scalar lane per tile
			else {tile_erosion_windowed(n, zvals, ec, iters, pad);}
			return;
		}
		uint32_t const *d_order = nullptr, *d_landc = nullptr;
		if (n > 512 && (uint64_t)n*iters >= (1u << 16)) { // more tiles than the chip holds at once (2 per CU): longest predicted chains first
			uint32_t *d_land = (uint32_t *)tile_order.grow(*this, (size_t)n*2*sizeof(uint32_t)), *d_ord = d_land + n;
			fill32(d_land, 0, n);
			run(terra::k_tile_land_cells, dim3(n), dim3(256), 0, zvals, (uint32_t)(ec.xsize*ec.ysize), ec.water_thresh, d_land);
			if (n <= 65536) { // the order is made on the device (rank by counting: n^2 / 2^12 block-steps, 16 M comparisons for the 64 x 64 batch): the call never waits for the stream
				run(terra::k_tile_order_by_land, dim3((n + 255)/256), dim3(256), 0, d_land, n, d_ord);
			}
			else {
				std::vector<uint32_t> land(n), ord(n);
				d2h(land.data(), d_land, (size_t)n*4);
				for (uint32_t i = 0; i < n; ++i) {ord[i] = i;}
				std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {return land[a] > land[b];});
				h2d(d_ord, ord.data(), (size_t)n*4);
			}
			d_order = d_ord; d_landc = d_land;
		}
		run(terra::k_tile_erosion, dim3(n), dim3(64), lds, zvals, ec, iters, d_order, d_landc);
	}
	void minmax(float const *vals, size_t n, uint32_t *d) {
		if (opt->simple_kernels || ((uintptr_t)vals & 15)) {minmax_simple(vals, n, d); return;}
		use();
		unsigned const blocks = (unsigned)std::min<size_t>((n/4 + 255)/256 + 1, 256*8);
		run(terra::k_minmax, dim3(blocks), dim3(256), 0, vals, n, d);
	}
	void quantize16(float const *vals, size_t n, float val_add, float val_div, uint8_t *pix) {
		size_t const n8 = ((opt->simple_kernels || ((uintptr_t)vals & 15) || ((uintptr_t)pix & 15)) ? 0 : n/8);
		if (n8) {
			use();
			if ((n8 + 255)/256 > 0x7FFFFFFFull) throw std::invalid_argument("quantize16: grid too large");
			run(terra::k_quantize16, dim3((unsigned)((n8 + 255)/256)), dim3(256), 0, vals, n8, val_add, val_div, (terra::st_u4 *)pix);
		}
		quantize16_simple(vals + n8*8, n - n8*8, val_add, val_div, pix + n8*16); // the tail (or everything, unaligned / cross-check)
	}
	// a hook that is one launch: false (and no launch) where the driver's simple form is to run -- "kernels.simple", or a grid that does not fit (`fits`)
	template<class K, class... A> bool launch_if(bool fits, K kernel, dim3 grid, dim3 block, A... args) {
		if (opt->simple_kernels || !fits) return false;
		use();
		run(kernel, grid, block, 0, args...);
		return true;
	}
	// one workgroup of T threads per tile of a batch of n
	template<unsigned T, class K, class... A> bool launch_per_tile(K kernel, uint32_t n, A... args) {return launch_if(n <= 0x7FFFFFFFu, kernel, dim3(n), dim3(T), args...);}
	bool tile_weights(terra::landscape_consts_t const &c, terra::tile_ref_pod_t const *refs, uint32_t n, float const *zvals, float const *noise, float const *params, uint32_t *w32, terra::grass_block_pod_t *blocks, uint8_t *any_grass) {
		return launch_if((uint64_t)n*terra::WK_BANDS <= 0x7FFFFFFFull, terra::k_tile_weights, dim3(n*terra::WK_BANDS), dim3(256), c, refs, zvals, noise, params, w32, blocks, any_grass);
	}
	// the grass brush: k_grass_brush_texels over (tile, window chunk) -- only when the brush has a radius -- then k_grass_brush_tiles once per tile
	bool tile_edit_grass(terra::grass_brush_consts_t const &g, terra::landscape_consts_t const &c, terra::tile_ref_pod_t const *refs, uint32_t n, float const *zvals, terra_tile_stats const *stats,
		uint8_t const *distant, float const *params, uint32_t *w32, terra::grass_block_pod_t *blocks, uint8_t *flags, uint8_t *updated, uint32_t *ranges)
	{
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		uint32_t const chunks = (g.wx*g.wy + terra::GB_CHUNK - 1)/terra::GB_CHUNK;
		if (g.rr > 0.0f && chunks) {run(terra::k_grass_brush_texels, dim3(n, chunks), dim3(terra::GB_THREADS), 0, g, c, refs, zvals, stats, params, w32, flags);}
		run(terra::k_grass_brush_tiles, dim3(n), dim3(terra::GB_THREADS), 0, g, c, refs, zvals, stats, distant, w32, blocks, flags, updated, ranges);
		return true;
	}
	// the line queries: k_line_boxes once per tile, then k_line_intersect once per line, in launches of fewer than 2^32 / LI_THREADS lines (HIP's limit on the
	// work-items of one grid dimension)
	bool tile_line_intersect(terra::line_query_consts_t const &c, terra::tile_ref_pod_t const *refs, uint32_t n, float const *zvals, terra_tile_stats const *stats,
		uint8_t const *distant, terra::line_box_t *boxes, float const *lines, int32_t const *line_tile, uint32_t nlines, terra::line_hit_pod_t *hits)
	{
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		if (n) {run(terra::k_line_boxes, dim3((n + 255)/256), dim3(256), 0, c, refs, stats, distant, n, boxes);}
		uint32_t const per = (0xFFFFFFFFu/terra::LI_THREADS) & ~255u;
		for (uint32_t r0 = 0; r0 < nlines;) {
			uint32_t const m = terra::min_u32(per, nlines - r0);
			run(terra::k_line_intersect, dim3(m), dim3(terra::LI_THREADS), 0, c, zvals, boxes, n, lines + (size_t)6*r0, line_tile ? line_tile + r0 : nullptr, hits + r0);
			r0 += m;
		}
		return true;
	}
	// the line queries with inc_trees != 0: k_line_tree_boxes once per tile (a wave a tile), then k_line_intersect_trees once per line, in launches as above.
	// record*2 + part must fit 32 bits: a capacity beyond 2^31 goes to the simple form
	bool tile_line_intersect_trees(terra::line_trees_consts_t const &c, terra::line_trees_in_t const &in, terra::tile_ref_pod_t const *refs, uint32_t n, float const *zvals,
		terra_tile_stats const *stats, uint8_t const *distant, terra::line_box_t *boxes, terra::line_tree_box_t *tboxes, float const *lines, int32_t const *line_tile, uint32_t nlines,
		terra::line_tree_hit_pod_t *hits)
	{
		if (opt->simple_kernels || n > 0x7FFFFFFFu || c.cap > 0x7FFFFFFFu) return false;
		use();
		if (n) {run(terra::k_line_tree_boxes, dim3((n + 3)/4), dim3(256), 0, c, in, refs, stats, distant, n, boxes, tboxes);}
		uint32_t const per = (0xFFFFFFFFu/terra::LT_THREADS) & ~255u;
		for (uint32_t r0 = 0; r0 < nlines;) {
			uint32_t const m = terra::min_u32(per, nlines - r0);
			run(terra::k_line_intersect_trees, dim3(m), dim3(terra::LT_THREADS), 0, c, in, zvals, boxes, tboxes, n, lines + (size_t)6*r0, line_tile ? line_tile + r0 : nullptr, hits + r0);
			r0 += m;
		}
		return true;
	}
	// the tree map: k_tree_splats once per splat, then k_tree_map once per (tile, band of rows): bands of equal height that fit the kernel's LDS
	bool tile_tree_map(terra::tree_tile_pod_t const *tiles, uint32_t n, uint32_t S, uint8_t const *distant, terra::tree_splat_in_t const *splats, uint32_t ns,
		terra::tree_splat_pod_t *par, float dxv, float dyv, bool reset, uint16_t *map, uint8_t *updated)
	{
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		uint32_t const W = S + 1, rmax = terra::TM_CELLS/W, bands = (W + rmax - 1)/rmax, R = (W + bands - 1)/bands;
		uint32_t const m = (ns > n) ? ns : n;
		run(terra::k_tree_splats, dim3((m + 255)/256), dim3(256), 0, tiles, n, splats, ns, dxv, dyv, par, updated);
		run(terra::k_tree_map, dim3(n, (W + R - 1)/R), dim3(64), 0, tiles, distant, par, (int)S, (int)R, reset ? 1 : 0, map, updated);
		return true;
	}
	bool tile_shadow_texture(terra::shadow_tex_consts_t const &c, uint32_t n, uint32_t S, uint8_t const *sun, uint8_t const *moon, uint8_t const *ao, uint16_t const *tree, uint32_t *out) {
		return launch_if(n <= 0x7FFFFFFFu, terra::k_shadow_texture, dim3(n, ((S + 1)*(S + 1) + 255)/256), dim3(256), c, S, sun, moon, ao, tree, out);
	}
	bool tile_tree_weights(size_t ntex, uint32_t const *in, uint8_t const *tree, uint32_t *out) {
		return launch_if((ntex + 255)/256 <= 0x7FFFFFFFull, terra::k_tree_weights, dim3((unsigned)((ntex + 255)/256)), dim3(256), ntex, in, tree, out);
	}
	// tree AO shadows from the placement records: k_tree_ao_sources once per record slot, k_tree_ao_gather once per tile, then k_tree_map on the device-built lists
	// (trmax is zero on entry)
	bool tile_tree_ao(terra::tree_ao_consts_t const &c, uint32_t n, terra::tree_inst_pod_t const *insts, terra::tree_place_pod_t const *pine, uint32_t const *pine_counts,
		terra::decid_place_pod_t const *decid, uint32_t const *decid_counts, float const *decid_radius, float const *decid_radius_by_id, uint8_t const *flags,
		terra::tree_frame_t const *frames, int32_t const *nbr, terra::tree_splat_in_t *src, float *trmax, terra::tree_tile_pod_t *tiles, terra::tree_splat_pod_t *par,
		uint32_t *list_counts, uint16_t *map, uint8_t *updated)
	{
		uint32_t const chunks = (c.src_cap + 255)/256;
		if (opt->simple_kernels || n > 0x7FFFFFFFu || chunks > 65535u) return false;
		use();
		uint32_t const S = (uint32_t)c.S, W = S + 1, rmax = terra::TM_CELLS/W, bands = (W + rmax - 1)/rmax, R = (W + bands - 1)/bands;
		run(terra::k_tree_ao_sources, dim3(n, chunks ? chunks : 1), dim3(256), 0, c, insts, pine, pine_counts, decid, decid_counts, decid_radius,
			decid_radius_by_id, src, trmax, updated);
		run(terra::k_tree_ao_gather, dim3(n), dim3(terra::TREEP_THREADS), 0, c, frames, nbr, flags, trmax, pine_counts, decid_counts, src, tiles, par, list_counts);
		run(terra::k_tree_map, dim3(n, (W + R - 1)/R), dim3(64), 0, tiles, (uint8_t const *)nullptr, par, (int)S, (int)R, 1, map, updated);
		return true;
	}
	// the tree brush on the record arrays: k_tree_edit once per tile (culls and removal), k_tree_edit_append once per tile after the brush placements, k_tree_edit_finish
	// once per tile for status and changed
	bool tile_edit_trees(terra::tree_edit_consts_t const &c, uint32_t n, terra::tree_edit_frame_t const *frames, terra_tile_stats const *stats, terra::tree_inst_pod_t const *insts,
		terra::tree_place_pod_t *pine, uint32_t *pine_counts, terra::decid_place_pod_t *decid, uint32_t *decid_counts, float *decid_radius, float const *by_id, float const *trmax,
		uint32_t *idx, uint32_t *box, uint8_t *status, uint8_t const *skip, uint8_t const *gen_flags, uint8_t *place_skip)
	{
		return launch_per_tile<terra::TREEP_THREADS>(terra::k_tree_edit, n, c, frames, stats, insts, pine, pine_counts, decid, decid_counts, decid_radius, by_id, trmax, idx, box, status,
			skip, gen_flags, place_skip);
	}
	bool tile_edit_trees_append(terra::tree_edit_consts_t const &c, uint32_t n, uint8_t const *gen_flags, terra::tree_inst_pod_t const *insts, terra::tree_place_pod_t const *new_pine,
		uint32_t const *new_pine_counts, terra::tree_place_pod_t *pine, uint32_t *pine_counts, terra::decid_place_pod_t const *new_decid, uint32_t const *new_decid_counts,
		terra::decid_place_pod_t *decid, uint32_t *decid_counts, float *decid_radius, float const *by_id, float *trmax, uint32_t *box, uint8_t *status)
	{
		return launch_if(true, terra::k_tree_edit_append, dim3(n), dim3(terra::TREEP_THREADS), c, gen_flags, insts, new_pine, new_pine_counts, pine, pine_counts, new_decid,
			new_decid_counts, decid, decid_counts, decid_radius, by_id, trmax, box, status);
	}
	bool tile_edit_trees_finish(terra::tree_edit_consts_t const &c, uint32_t n, terra::tree_edit_frame_t const *frames, terra_tile_stats const *stats, uint32_t const *box,
		uint8_t *status, uint8_t *changed, float *update_bcube)
	{
		return launch_if(true, terra::k_tree_edit_finish, dim3((n + 255)/256), dim3(256), c, n, frames, stats, box, status, changed, update_bcube);
	}
	// tree placement: one workgroup per tile (k_tree_place)
	bool tile_place_trees(terra::tree_place_consts_t const *c, terra::tile_ref_pod_t const *tiles, uint32_t n, float const *dens, uint8_t const *skip, terra_tile_stats const *stats,
		uint32_t capacity, terra::tree_place_pod_t *trees, uint32_t *counts)
	{
		return launch_per_tile<terra::TREEP_THREADS>(terra::k_tree_place, n, c, tiles, dens, skip, stats, capacity, trees, counts);
	}
	// deciduous tree placement: one workgroup per tile (k_decid_place)
	bool tile_place_decid_trees(terra::decid_place_consts_t const *c, terra::tile_ref_pod_t const *tiles, uint32_t n, float const *dens, uint8_t const *skip, terra_tile_stats const *stats,
		float const *zvals, uint32_t capacity, terra::decid_place_pod_t *trees, uint32_t *counts)
	{
		return launch_per_tile<terra::TREEP_THREADS>(terra::k_decid_place, n, c, tiles, dens, skip, stats, zvals, capacity, trees, counts);
	}
	// scenery placement: one workgroup per tile (k_scenery_place)
	bool tile_place_scenery(terra::scenery_place_consts_t const *c, terra::tile_ref_pod_t const *tiles, uint32_t n, float const *dens, uint8_t const *skip, uint32_t capacity,
		terra::scenery_place_pod_t *objs, uint32_t *counts, uint32_t *kind_counts)
	{
		return launch_per_tile<terra::TREEP_THREADS>(terra::k_scenery_place, n, c, tiles, dens, skip, capacity, objs, counts, kind_counts);
	}
	// flowers: one wave per tile (k_flowers_place)
	bool tile_place_flowers(terra::flower_consts_t const &c, terra::tile_ref_pod_t const *tiles, uint32_t n, uint8_t const *skip, uint8_t const *weights, float const *den,
		float const *col, uint32_t capacity, terra::flower_pod_t *flowers, uint32_t *aux, uint32_t *counts)
	{
		return launch_per_tile<64>(terra::k_flowers_place<false>, n, c, tiles, skip, (uint8_t const *)nullptr, (uint32_t const *)nullptr, weights, den, col, capacity, flowers, aux, counts);
	}
	// the flowers' upkeep after a grass stroke: k_flowers_remove once per tile, then, when adding, k_flowers_place over the strokes' rectangles
	bool tile_edit_flowers(terra::flower_edit_consts_t const &c, terra::tile_ref_pod_t const *tiles, uint32_t n, uint8_t const *generated, uint8_t const *updated,
		uint32_t const *ranges, uint8_t const *weights, float const *den, float const *col, uint32_t capacity, terra::flower_pod_t *flowers, uint32_t *aux, uint32_t *counts,
		uint8_t *status, uint32_t *idx, uint8_t *kind)
	{
		if (!launch_per_tile<terra::TREEP_THREADS>(terra::k_flowers_remove, n, c, tiles, generated, updated, ranges, capacity, flowers, aux, counts, status, idx, kind)) return false;
		if (c.add) {launch_per_tile<64>(terra::k_flowers_place<true>, n, c.f, tiles, (uint8_t const *)nullptr, (uint8_t const *)kind, ranges, weights, den, col, capacity, flowers, aux, counts);}
		return true;
	}
	// the grass draw lists for a camera: one workgroup per tile (k_grass_view)
	bool tile_grass_view(terra::grass_view_consts_t const &c, terra::grass_view_io_t const &io, int32_t const *tile_xy, uint32_t n, uint32_t capacity, uint16_t *keys) {
		return launch_per_tile<terra::GV_THREADS>(terra::k_grass_view, n, c, tile_xy, io.zvals, io.stats, io.blocks, io.skip, capacity, io.insts, io.aux, io.group_counts, io.counts,
			io.pass, keys);
	}
	// the terrain draw list for a camera: the five launches of k_terrain_view_* (terra_kernels.hpp); with a box, reflection pass 1: k_reflect_walk and k_reflect_finish between
	// the occlusion test and the lists (s.rt and s.prov are null in the terrain view)
	bool terrain_view_launches(terra::terrain_view_consts_t const &c, terra::reflect_box_t const *box, terra::terrain_view_io_t const &io, terra::terrain_view_scratch_t const &s, uint32_t n) {
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		uint32_t const T = terra::TV_THREADS, nb = (n + T - 1)/T;
		run(terra::k_terrain_view_tiles, dim3(nb), dim3(T), 0, c, io.in, s.txy, n, io.status, io.dist, io.lod, s.test, s.rt);
		run(terra::k_terrain_view_occluders, dim3(1), dim3(T), 0, c, io.in, s.txy, n, io.status, s.occ, s.nocc);
		run(terra::k_terrain_view_occlusion, dim3(n), dim3(T), 0, c, io.in, s.txy, s.occ, s.nocc, s.test, io.status, s.prov);
		if (box) {
			run(terra::k_reflect_walk, dim3(n), dim3(terra::RF_THREADS), ((size_t)box->nwords + box->cap)*4, s.rc, io.in.stats, s.txy, s.nbr, s.rt, io.status, s.prov, *box, s.refl, io.reflect ? io.reflect : s.refl);
			run(terra::k_reflect_finish, dim3(nb), dim3(T), 0, n, s.prov, s.refl, io.status, io.in.occl_state);
		}
		run(terra::k_terrain_view_lists, dim3(1), dim3(T), 0, s.nbr, n, io.status, io.dist, io.lod, io.crack, io.draw_order, io.occluded, io.counts, io.not_drawn, s.keys, s.key_tile);
		run(terra::k_terrain_view_rank, dim3(nb), dim3(T), 0, s.keys, s.key_tile, io.counts, io.draw_order);
		return true;
	}
	bool tile_terrain_view(terra::terrain_view_consts_t const &c, terra::terrain_view_io_t const &io, terra::terrain_view_scratch_t const &s, uint32_t n) {return terrain_view_launches(c, nullptr, io, s, n);}
	bool tile_reflection_view(terra::reflect_consts_t const &c, terra::reflect_box_t const &box, terra::terrain_view_io_t const &io, terra::terrain_view_scratch_t const &s, uint32_t n) {return terrain_view_launches(c.tv, &box, io, s, n);}
	// water quads and water caps: one workgroup (k_water_view)
	bool tile_water_view(terra::terrain_view_consts_t const &c, terra::water_view_io_t const &io, terra::water_view_scratch_t const &s, uint32_t n) {
		return launch_if(true, terra::k_water_view, dim3(1), dim3(terra::TV_THREADS), c, io.in, s.txy, s.nbr, n, io.status, s.wv, io.water_list, io.cap_mask, io.counts);
	}
	// the shadow-map plan: a lane per tile, the receivers by one workgroup, the recompute queue by rank (k_smap_plan*)
	bool tile_smap_plan(terra::smap_consts_t const &c, terra::terrain_view_in_t const &in, terra::smap_plan_io_t const &io, int32_t const *tile_xy, uint32_t n, terra::smap_rank_key_t *keys) {
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		uint32_t const T = terra::TV_THREADS, nb = (n + T - 1)/T;
		bool const recomp = c.want_recomp && io.recomp_order;
		run(terra::k_smap_plan, dim3(nb), dim3(T), 0, c, in, io, tile_xy, n, keys);
		run(terra::k_smap_plan_lists, dim3(1), dim3(T), 0, n, (uint32_t const *)io.plan, (terra::smap_rank_key_t const *)keys, io.receivers, io.counts, recomp ? 1 : 0);
		if (recomp) {run(terra::k_smap_plan_rank, dim3(nb), dim3(T), 0, (terra::smap_rank_key_t const *)keys, n, io.recomp_order);}
		return true;
	}
	// the casters of R renders: the geometry of the batch once, then a workgroup per render (k_smap_geom, k_smap_casters)
	bool tile_smap_casters(terra::smap_consts_t const &c, terra::terrain_view_in_t const &in, terra::smap_cast_io_t const &io, int32_t const *tile_xy, uint32_t n, uint32_t R,
		terra::smap_geom_t *geom, terra::view_pod_t const *views, float const *bsm, float const *lpos, int decid_trees_only, int inc_adj_smap)
	{
		if (opt->simple_kernels || n > 0x7FFFFFFFu || R > 0x7FFFFFFFu) return false;
		use();
		uint32_t const T = terra::TV_THREADS, nb = (n + T - 1)/T;
		run(terra::k_smap_geom, dim3(nb), dim3(T), 0, c, in, io.decid_counts, decid_trees_only, tile_xy, n, geom);
		run(terra::k_smap_casters, dim3(R), dim3(terra::SMC_THREADS), 0, (terra::smap_geom_t const *)geom, n, io.recv, views, bsm, lpos, decid_trees_only, inc_adj_smap, io.to_draw,
			io.terrain, io.counts, io.not_drawn, io.status);
		return true;
	}
	// the clouds' update: the marks of every record's path, the unmarked tiles in parallel, the marked tiles replayed in batch order by one workgroup
	bool tile_update_clouds(terra::cloud_consts_t const &c, terra::cloud_update_io_t const &io, terra::cloud_update_scratch_t const &s, uint32_t n) {
		if (opt->simple_kernels || n > 0x7FFFFFFFu) return false;
		use();
		uint32_t const T = terra::CLD_THREADS, nb = (n + T - 1)/T;
		uint8_t *const touched = (uint8_t *)s.marks;
		run(terra::k_cloud_mark, dim3(nb), dim3(T), 0, c, s.nbr, n, io.state, io.clouds, touched);
		run(terra::k_cloud_tiles, dim3(nb), dim3(T), 0, c, s.txy, s.nbr, n, touched, io.state, io.clouds);
		run(terra::k_cloud_tail, dim3(1), dim3(T), 0, c, s.txy, s.nbr, n, touched, s.order, io.state, io.clouds, io.total);
		return true;
	}
	// the clouds' draw list: a lane per record slot, then every listed instance to its rank
	bool tile_cloud_view(terra::cloud_view_consts_t const &c, terra::cloud_view_io_t const &io, terra::cloud_view_scratch_t const &s, uint32_t n) {
		if (opt->simple_kernels) return false;
		use();
		uint32_t const T = terra::CLD_THREADS, nrec = n*c.capacity, nb = (nrec + T - 1)/T;
		run(terra::k_cloud_view, dim3(nb), dim3(T), 0, c, s.tc, nrec, io.stats, io.state, io.clouds, io.stage, s.found, s.cnt);
		run(terra::k_cloud_rank, dim3(nb), dim3(T), 0, s.found, s.cnt, io.list, io.list_count);
		return true;
	}
	// sphere collisions and tree box tests: one wave per query, four to a workgroup (k_sphere_collide, k_cube_int_trees)
	bool tile_sphere_collide(terra::collide_consts_t const &c, terra::collide_in_t const &in, terra::sphere_query_pod_t const *queries, uint32_t nq, terra::sphere_hit_pod_t *hits) {
		uint32_t const per = terra::COLL_THREADS/64u;
		return launch_if(true, terra::k_sphere_collide, dim3(nq/per + ((nq%per) ? 1u : 0u)), dim3(terra::COLL_THREADS), c, in, queries, nq, hits);
	}
	bool tile_cube_int_trees(terra::collide_consts_t const &c, terra::collide_in_t const &in, float const *cubes, int32_t const *cube_tile, uint32_t nq, uint8_t *result, int32_t *tile_out) {
		uint32_t const per = terra::COLL_THREADS/64u;
		return launch_if(true, terra::k_cube_int_trees, dim3(nq/per + ((nq%per) ? 1u : 0u)), dim3(terra::COLL_THREADS), c, in, cubes, cube_tile, nq, result, tile_out);
	}
	// the pine and palm tree draw lists for a camera: one workgroup per tile (k_tree_view)
	bool tile_tree_view(terra::tree_view_consts_t const &c, terra::tree_view_io_t const &io, int32_t const *tile_xy, uint32_t n, terra::tree_inst_pod_t const *insts, uint32_t *keys) {
		return launch_per_tile<terra::TRV_THREADS>(terra::k_tree_view, n, c, tile_xy, insts, io.stats, io.skip, io.trmax, io.pine, io.counts, io.ov, io.tile_out, io.bcube, io.pine_insts,
			io.palm_insts, io.inst_counts, io.leaf_list, io.leaf_counts, io.trunk, keys);
	}
	// the scenery draw lists for a camera: one workgroup per tile (k_scenery_view)
	bool tile_scenery_view(terra::scenery_view_consts_t const &c, terra::scenery_view_io_t const &io, int32_t const *tile_xy, uint32_t n) {
		return launch_per_tile<terra::SCVW_THREADS>(terra::k_scenery_view, n, c, tile_xy, io.stats, io.skip, io.objs, io.counts, io.rov, io.tile_out, io.draw, io.size_scale, io.dist, io.list,
			io.group_counts);
	}
	// the deciduous tree draw lists for a camera: one workgroup per tile (k_decid_view)
	bool tile_decid_view(terra::decid_view_consts_t const &c, terra::decid_view_io_t const &io, uint32_t n, uint32_t *keys) {
		return launch_per_tile<terra::DCV_THREADS>(terra::k_decid_view, n, c, io.data, io.skip, io.decid, io.counts, io.not_visible, io.tile_out, io.bcube, io.leaf_word, io.leaf_scale,
			io.leaf_opacity, io.leaf_num, io.branch_word, io.branch_scale, io.branch_opacity, io.branch_num, io.leaf_list, io.branch_list, io.leaf_bb, io.branch_bb, io.list_counts, keys);
	}
	void voxel_noise(float *out, size_t nvox, terra::vox_noise_job_t const &J, bool perlin, bool fused, uint32_t const *lut3) {
		if (opt->simple_kernels) {voxel_noise_simple(out, nvox, J, perlin); return;}
		if (nvox == 0) return;
		use();
		// "gen.fused" has no kernel here: glm's 3-D lattice noise picks its gradients by the SIGN of expressions that are exactly zero at some of the hash's 49 / 289 values
		// (h = 1 - |x| - |y| in simplex(vec3), gz = 0.5 - |gx| - |gy| in perlin(vec3); noise.inl:149-157,690-700), so one contracted rounding flips a gradient: measured 0.146
		// on a 40 x 24 x 64 Perlin field for 1.2x.  The exact kernel answers (its gradients come from the table the exact code builds).
		(void)fused;
		uint32_t const nzp = (J.nz + 1)/2; // pairs (z, z + 1) per column
		size_t const npairs = (nvox / J.nz)*nzp, per_block = (size_t)256*terra::VN_CHUNKS;
		if ((npairs + per_block - 1)/per_block > 0x7FFFFFFFull) throw std::invalid_argument("voxel_fill: grid too large");
		dim3 const grid((unsigned)((npairs + per_block - 1)/per_block)), block(256);
		if (perlin) {run(terra::k_voxel_noise<true>, grid, block, 0, out, npairs, nzp, J, lut3);}
		else        {run(terra::k_voxel_noise<false>, grid, block, 0, out, npairs, nzp, J, lut3);}
	}
	void voxel_sines(float *out, uint32_t nx, uint32_t ny, uint32_t nz, float const *d_tab, float zscale, int normalize, int fused = 0, float fast_amax = 0.0f, float const *d_zt = nullptr, uint32_t nzp = 0) {
		if (opt->simple_kernels) {voxel_sines_simple(out, nx, ny, nz, d_tab, zscale, normalize, fused); return;}
		use();
		if (fused && (uint64_t)nx*ny <= 0x7FFFFF00ull) { // "gen.fused": the field as a (columns x 60) x (60 x nz) product on the f32 matrix pipe (terra_fused.hpp)
			size_t const ncol = (size_t)nx*ny;
			uint32_t const nyp = (uint32_t)((ncol + 255)/256*256), nxp = (nz + 127)/128*128; // (256: the narrow form of k_sine_grid_h3 walks 256-row tiles)
			terra::sgf_job_t J; memset(&J, 0, sizeof(J));
			J.out = out; J.nx = nz; J.ny = (uint32_t)ncol; J.nxp = nxp; J.nyp = nyp; J.ntx = nxp/128; J.nty = nyp/128; J.rowgroup = (unsigned)opt->sg_rowgroup;
			J.kstart = 0; J.kend = terra::VOX_SINES; J.zscale = zscale; J.normalize = normalize;
			if (fused == 2 && sine_grid_h3<terra::SGF_VOXELS>(J, 1.0f, fast_amax, d_tab, nx, ny)) return; // TERRA_GEN_FAST (|zv| <= 1; |xv*yv| <= the largest magnitude)
			size_t const np = (size_t)terra::VOX_SINES*((size_t)nyp + nxp);
			float *const pt = (float *)vox_p.grow(*this, np*4), *const zt = pt + (size_t)terra::VOX_SINES*nyp;
			// PT[k][column] = xv[x][k]*yv[y][k] (the product rounds as in the reference, src/upsurface.cpp:66; only the multiply-add with zv is fused), ZT[k][z]: both k-major, zero padded
			launch(np, [=] TERRA_LAMBDA (size_t i) {
				if (i < (size_t)terra::VOX_SINES*nyp) {
					uint32_t const k = (uint32_t)(i / nyp); size_t const c = i % nyp;
					float v = 0.0f;
					if (c < ncol) {uint32_t const x = (uint32_t)(c % nx), y = (uint32_t)(c / nx); v = __fmul_rn(d_tab[(size_t)x*terra::VOX_SINES + k], d_tab[((size_t)nx + y)*terra::VOX_SINES + k]);}
					pt[i] = v;
				}
				else {
					size_t const j = i - (size_t)terra::VOX_SINES*nyp;
					uint32_t const k = (uint32_t)(j / nxp), z = (uint32_t)(j % nxp);
					zt[j] = (z < nz) ? d_tab[((size_t)nx + ny + z)*terra::VOX_SINES + k] : 0.0f;
				}
			});
			J.xt = zt; J.yt = pt;
			unsigned const nb = J.ntx*J.nty, grid = ((nb + 7)/8)*8;
			run(terra::k_sine_grid_mx<terra::SGF_VOXELS>, dim3(std::min(grid, (unsigned)(2*num_cus + 7)/8*8)), dim3(256), 0, J);
			return;
		}
		if ((nz & 3u) == 0 && opt->voxels_cols && d_zt) { // a lane per column, the products in registers, the z table as scalar operands (k_voxel_sines_cols): no P array
			size_t const ncolc = (size_t)nx*ny;
			run(terra::k_voxel_sines_cols, dim3((unsigned)((ncolc + terra::VC_COLS - 1)/terra::VC_COLS), (nz + terra::VC_Z - 1)/terra::VC_Z), dim3(256), 0, out, nx, ny, nz, nzp, d_tab, d_zt, zscale, normalize);
			return;
		}
		size_t const ncol2 = ((size_t)nx*ny + 1) & ~(size_t)1, np = (ncol2/2)*terra::VX_PSTRIDE + (size_t)nz*terra::VOX_SINES, nprod = (ncol2 + nz)*terra::VOX_SINES; // column pairs + transposed z table
		float *const vp = (float *)vox_p.grow(*this, np*4), *const vz = vp + (ncol2/2)*terra::VX_PSTRIDE; // the products, the transposed z table behind them
		run(terra::k_voxel_P, dim3((unsigned)((nprod + 255)/256)), dim3(256), 0, vp, vz, nx, ny, nz, d_tab);
		unsigned const block = (nz >= 256) ? 256 : ((nz + 63)/64)*64;
		size_t const ncol = (size_t)nx*ny;
		run(terra::k_voxel_sines, dim3((unsigned)((ncol + terra::VX_PER_BLOCK - 1)/terra::VX_PER_BLOCK), (nz + block - 1)/block), dim3(block), 0, out, nx, ny, nz, vz, vp, zscale, normalize);
	}
};
typedef hip_backend_t terra_backend_t;
#include "terra_api_impl.hpp"
