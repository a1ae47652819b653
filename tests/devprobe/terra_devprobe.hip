// tests/devprobe/terra_devprobe.hip -- TEST INFRASTRUCTURE ONLY (never linked into libterra_hip.so, nothing of include/terra.h).
//
// The small host/device functions every pass shares (TERRA_HD bodies of 3dworld_amd/csrc/*.hpp), evaluated alone on arrays of arguments: one C entry point per
// family, one source, two builds (tests/devprobe/build_probe.py):
//   libterra_devprobe_hip.so    hipcc with the product's flags for gfx950: every entry point copies its arrays to device 0, launches ONE kernel (256 threads per
//                               block, `i < n` guard) whose thread i evaluates element i, and copies the results back
//   libterra_devprobe_host.so   g++ -x c++ with the host emulation's flags: the same bodies in a loop
// Each body calls the product's own function: the view and box primitives of terra_view.hpp, the line clip and the conversions of terra_common.hpp, the libm
// restatements, and terra_terrainview.hpp's two LOD functions.  Every entry point returns 0, or the first HIP error's code (-1: no device); nothing aborts.
#include "terra_view.hpp"
#include "terra_common.hpp"
#include "terra_sincosf.hpp"
#include "terra_powf.hpp"
#include "terra_terrainview.hpp" // terrain_view_steep_dist, terrain_view_lod
#include <vector>

using namespace terra;

namespace {

#if defined(__HIPCC__)
template<class F> __global__ void __launch_bounds__(256) k_probe(F f, uint32_t n) {
	uint32_t const i = blockIdx.x*256u + threadIdx.x;
	if (i < n) {f(i);}
}
// the arrays of one call: inputs are copied up at once, outputs are copied down by finish(); the first error is kept and turns every later step into a no-op
struct probe_run_t {
	struct out_t {void *d, *h; size_t bytes;};
	int err;
	std::vector<void *> bufs;
	std::vector<out_t> outs;
	probe_run_t() : err(0) {
		int count = 0;
		if (check(hipGetDeviceCount(&count)) && count < 1) {err = -1;}
		if (!err) {check(hipSetDevice(0));}
	}
	~probe_run_t() {for (void *p : bufs) {(void)hipFree(p);}}
	bool check(hipError_t e) {if (e != hipSuccess && !err) {err = (int)e;} return !err;}
	void *alloc(size_t bytes) {
		void *d = nullptr;
		if (err || !check(hipMalloc(&d, bytes ? bytes : 1))) return nullptr;
		bufs.push_back(d);
		return d;
	}
	template<class T> T const *in(T const *h, size_t count) {
		void *d = alloc(count*sizeof(T));
		if (d && count) {check(hipMemcpy(d, h, count*sizeof(T), hipMemcpyHostToDevice));}
		return (T const *)d;
	}
	template<class T> T *out(T *h, size_t count) {
		void *d = alloc(count*sizeof(T));
		if (d && count) {check(hipMemset(d, 0xA5, count*sizeof(T)));} // an element no thread wrote cannot pass for a result
		if (d) {outs.push_back({d, h, count*sizeof(T)});}
		return (T *)d;
	}
	template<class F> void run(F f, uint32_t n) {
		if (err || n == 0) return;
		k_probe<<<dim3((n + 255u)/256u), dim3(256)>>>(f, n);
		check(hipGetLastError());
		check(hipDeviceSynchronize());
	}
	int finish() {
		for (out_t const &o : outs) {if (!err && o.bytes) {check(hipMemcpy(o.h, o.d, o.bytes, hipMemcpyDeviceToHost));}}
		return err;
	}
};
#define PROBE_FN __device__
#else
struct probe_run_t {
	template<class T> T const *in(T const *h, size_t) {return h;}
	template<class T> T *out(T *h, size_t) {return h;}
	template<class F> void run(F f, uint32_t n) {for (uint32_t i = 0; i < n; ++i) {f(i);}}
	int finish() {return 0;}
};
#define PROBE_FN
#endif

struct f_powf {
	float const *x, *y; float *o;
	PROBE_FN void operator()(uint32_t i) const {o[i] = glibc_powf(x[i], y[i]);}
};
struct f_sincosf {
	float const *x; float *s, *c;
	PROBE_FN void operator()(uint32_t i) const {s[i] = glibc_sinf(x[i]); c[i] = glibc_cosf(x[i]);}
};
struct f_sincosf_droplet { // the form the droplets call: the same bodies without the branches for |x| >= 120
	float const *x; float *s, *c;
	PROBE_FN void operator()(uint32_t i) const {s[i] = glibc_sinf_below_120(x[i]); c[i] = glibc_cosf_below_120(x[i]);}
};
struct f_points {
	view_pod_t v; float const *p; uint8_t *o;
	PROBE_FN void operator()(uint32_t i) const {o[i] = view_point_visible(v, p[3*i], p[3*i + 1], p[3*i + 2]) ? 1 : 0;}
};
struct f_spheres {
	view_pod_t v; float bsm; float const *s; uint8_t *o;
	PROBE_FN void operator()(uint32_t i) const {o[i] = view_sphere_visible(v, bsm, s[4*i], s[4*i + 1], s[4*i + 2], s[4*i + 3]) ? 1 : 0;}
};
// o[5]: cube_visible, cube_completely_visible, cube_visible_likely, sphere_and_cube_visible_test, closest_dist_less_than
struct f_cubes {
	view_pod_t v; float bsm; float const *c, *s, *q; uint8_t *o;
	PROBE_FN void operator()(uint32_t i) const {
		float const d[3][2] = {{c[6*i], c[6*i + 1]}, {c[6*i + 2], c[6*i + 3]}, {c[6*i + 4], c[6*i + 5]}};
		o[5*i]     = view_cube_visible(v, d) ? 1 : 0;
		o[5*i + 1] = view_cube_completely_visible(v, d) ? 1 : 0;
		o[5*i + 2] = view_cube_visible_likely(v, d) ? 1 : 0;
		o[5*i + 3] = view_sphere_and_cube_visible(v, bsm, s[4*i], s[4*i + 1], s[4*i + 2], s[4*i + 3], d) ? 1 : 0;
		o[5*i + 4] = view_closest_dist_less_than(d, q[4*i], q[4*i + 1], q[4*i + 2], q[4*i + 3]) ? 1 : 0;
	}
};
struct f_inv_sqrt {
	float const *x; float *o;
	PROBE_FN void operator()(uint32_t i) const {o[i] = inv_sqrt_ref(x[i]);}
};
struct f_line_clip {
	float const *v, *d; uint8_t *ok; float *o;
	PROBE_FN void operator()(uint32_t i) const {
		shadow_pt_t v1 = {v[6*i], v[6*i + 1], v[6*i + 2]}, v2 = {v[6*i + 3], v[6*i + 4], v[6*i + 5]};
		float const dd[3][2] = {{d[6*i], d[6*i + 1]}, {d[6*i + 2], d[6*i + 3]}, {d[6*i + 4], d[6*i + 5]}};
		ok[i] = shadow_line_clip(v1, v2, dd) ? 1 : 0;
		o[6*i] = v1.x; o[6*i + 1] = v1.y; o[6*i + 2] = v1.z; o[6*i + 3] = v2.x; o[6*i + 4] = v2.y; o[6*i + 5] = v2.z;
	}
};
// od: the steep-slope statement of terrain_view_lod (terrain_view_steep_dist);
// ol: terrain_view_lod itself for a tile of S = 128 that is not flat, no shadow maps, no water, no reflection: the level that float gives
struct f_lod {
	float const *dist, *mnz; float *od; uint8_t *ol;
	PROBE_FN void operator()(uint32_t i) const {
		od[i] = terrain_view_steep_dist(dist[i], mnz[i]);
		terrain_view_consts_t tc = {}; tc.S = 128; tc.water_enabled = 0; tc.reflection_pass = 0;
		ol[i] = (uint8_t)terrain_view_lod(tc, 0.0f, 1.0f, mnz[i], dist[i], false);
	}
};
struct f_conv_f {
	float const *x; uint32_t *u; int32_t *s;
	PROBE_FN void operator()(uint32_t i) const {u[i] = f2u_x86(x[i]); s[i] = f2i_x86(x[i]);}
};
struct f_conv_d {
	double const *x; uint32_t *u; int32_t *s;
	PROBE_FN void operator()(uint32_t i) const {u[i] = d2u_x86(x[i]); s[i] = d2i_x86(x[i]);}
};

view_pod_t load_view(float const *w, int32_t valid) { // w[16]: pos, dir, upv_, cp, sterm, x_sterm, near_, far_
	view_pod_t v;
	for (int k = 0; k < 3; ++k) {v.pos[k] = w[k]; v.dir[k] = w[3 + k]; v.upv[k] = w[6 + k]; v.cp[k] = w[9 + k];}
	v.sterm = w[12]; v.x_sterm = w[13]; v.near_ = w[14]; v.far_ = w[15]; v.valid = valid;
	return v;
}

} // namespace

#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int probe_is_device() {
#if defined(__HIPCC__)
	return 1;
#else
	return 0;
#endif
}
PROBE_API int probe_powf(float const *x, float const *y, uint32_t n, float *out) {
	probe_run_t r;
	f_powf f = {r.in(x, n), r.in(y, n), r.out(out, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_sincosf(float const *x, uint32_t n, float *s, float *c) {
	probe_run_t r;
	f_sincosf f = {r.in(x, n), r.out(s, n), r.out(c, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_sincosf_droplet(float const *x, uint32_t n, float *s, float *c) {
	probe_run_t r;
	f_sincosf_droplet f = {r.in(x, n), r.out(s, n), r.out(c, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_points(float const *view, int32_t valid, float const *p, uint32_t n, uint8_t *out) {
	probe_run_t r;
	f_points f = {load_view(view, valid), r.in(p, 3*(size_t)n), r.out(out, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_spheres(float const *view, int32_t valid, float bsm, float const *s, uint32_t n, uint8_t *out) {
	probe_run_t r;
	f_spheres f = {load_view(view, valid), bsm, r.in(s, 4*(size_t)n), r.out(out, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_cubes(float const *view, int32_t valid, float bsm, float const *c, float const *s, float const *q, uint32_t n, uint8_t *out) {
	probe_run_t r;
	f_cubes f = {load_view(view, valid), bsm, r.in(c, 6*(size_t)n), r.in(s, 4*(size_t)n), r.in(q, 4*(size_t)n), r.out(out, 5*(size_t)n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_inv_sqrt(float const *x, uint32_t n, float *out) {
	probe_run_t r;
	f_inv_sqrt f = {r.in(x, n), r.out(out, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_line_clip(float const *v, float const *d, uint32_t n, uint8_t *ok, float *out) {
	probe_run_t r;
	f_line_clip f = {r.in(v, 6*(size_t)n), r.in(d, 6*(size_t)n), r.out(ok, n), r.out(out, 6*(size_t)n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_lod(float const *dist, float const *mnz, uint32_t n, float *out_dist, uint8_t *out_lod) {
	probe_run_t r;
	f_lod f = {r.in(dist, n), r.in(mnz, n), r.out(out_dist, n), r.out(out_lod, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_convert_floats(float const *x, uint32_t n, uint32_t *u, int32_t *s) {
	probe_run_t r;
	f_conv_f f = {r.in(x, n), r.out(u, n), r.out(s, n)};
	r.run(f, n);
	return r.finish();
}
PROBE_API int probe_convert_doubles(double const *x, uint32_t n, uint32_t *u, int32_t *s) {
	probe_run_t r;
	f_conv_d f = {r.in(x, n), r.out(u, n), r.out(s, n)};
	r.run(f, n);
	return r.finish();
}
