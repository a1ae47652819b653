// terra_common.hpp -- shared host/device helpers for libterra_hip (MI355X / gfx950).
//
// Everything here is arithmetic that must agree bit-for-bit with the reference CPU path
// (g++ -O3, x86-64 SSE2 scalar float, NO fused multiply-add): the whole library is compiled with
// -ffp-contract=off and the few places where the C++ source promotes to double are written out explicitly.
// Citations are relative to the 3DWorld reference tree.
#pragma once
#include <stdint.h>
#include <math.h>
#include <float.h>
#include <limits.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TERRA_HD __host__ __device__ __forceinline__
#define TERRA_D  __device__ __forceinline__
#define TERRA_HD_COLD __host__ __device__ __attribute__((noinline)) // rarely executed and large: a real call keeps its registers out of the caller's hot loop
#define TERRA_LAMBDA __host__ __device__
#else
#define TERRA_HD inline
#define TERRA_HD_COLD inline
#define TERRA_D  inline
#define TERRA_LAMBDA
#endif

// branch-probability hints: they only steer basic-block placement, so that the step loop of a droplet trace stays one compact run of
// instructions (the rarely taken window shifts, multi-version look-ups and libm restatements are laid out behind it)
#define TERRA_LIKELY(x)   __builtin_expect(!!(x), 1)
#define TERRA_UNLIKELY(x) __builtin_expect(!!(x), 0)

namespace terra {

constexpr int   F_TABLE_SIZE   = 90;     // NUM_FREQ_COMP(9)*N_RAND_SIN2(10), src/mesh_gen.cpp:14,16,30
constexpr int   NUM_FREQ_COMP  = 9;
constexpr int   N_RAND_SIN2    = 10;
constexpr int   TSIZE          = 1 << 15; // src/sinf.h:8
constexpr float PI_F           = 3.141592654f; // src/3DWorld.h:43
constexpr int   EROSION_PAD    = 4;      // src/erosion.cpp:25

// The sine tables of k_sine_grid (terra_kernels.hpp) and what its staging reads of them.  The kernel sums the terms kstart..89 in ceil(nk / KC) chunks of equal length (the
// last may be shorter) and copies a chunk into LDS in whole row PAIRS without a test per row: a chunk of kn rows from row k0 reads the rows k0 .. k0 + kn - 1 and, when kn is
// odd, row k0 + kn as well -- the next chunk's first row or, behind the last term, row 90.  So every table has SG_TABLE_ROWS rows, and the launch that builds the tables
// writes zeros into the rows behind row 89 (they never reach a sum).  Nothing depends on how large the scratch buffer under a table is: row k begins at k*(padded row length)
// of the CURRENT grid, so a buffer that grew for a larger grid holds the smaller grid's table in its first SG_TABLE_ROWS*(row length) floats, all written by that grid's launch.
TERRA_HD constexpr int sg_chunk_len(int kstart, int KC) {int const nk = F_TABLE_SIZE - kstart, n = (nk + KC - 1)/KC; return (nk > 0 && n > 0) ? (nk + n - 1)/n : 0;}
TERRA_HD constexpr int sg_chunk_last_row(int k0, int kn) {return k0 + kn - 1 + (kn & 1);}
TERRA_HD constexpr int sg_last_row_read(int kstart, int KC) { // the last table row the staging of any chunk reads (-1: no term, nothing is read)
	int const per = sg_chunk_len(kstart, KC);
	int last = -1;
	for (int k0 = kstart; per > 0 && k0 < F_TABLE_SIZE; k0 += per) {
		int const kn = (k0 + per > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per, l = sg_chunk_last_row(k0, kn);
		if (l > last) {last = l;}
	}
	return last;
}
constexpr int SG_TABLE_ROWS = F_TABLE_SIZE + 1;
constexpr bool sg_table_rows_suffice() {
	constexpr int kcs[3] = {20, 27, 45}; // "sg.kc" / "sg.kc_tiles"
	for (int i = 0; i < 3; ++i) {for (int kstart = 0; kstart <= F_TABLE_SIZE; ++kstart) {if (sg_last_row_read(kstart, kcs[i]) >= SG_TABLE_ROWS) return false;}}
	return true;
}
static_assert(sg_table_rows_suffice(), "k_sine_grid's staging would read behind the sine tables");
// k_sine_grid_rs (the heightmap's row-scalar form, KC = 27) stages X one table row per load -- rows k0 .. k0 + kn - 1 -- and prefetches the row operands one term ahead: the
// last stage of a chunk asks for table row k0 + kn, the next chunk's first row or row 90
TERRA_HD constexpr int sg_rs_last_row_read(int kstart, int KC) { // the last table row the row-scalar kernel reads (X staging: k0 + kn - 1; Y prefetch: k0 + kn)
	int const per = sg_chunk_len(kstart, KC);
	int last = -1;
	for (int k0 = kstart; per > 0 && k0 < F_TABLE_SIZE; k0 += per) {int const kn = (k0 + per > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per; if (k0 + kn > last) {last = k0 + kn;}}
	return last;
}
constexpr bool sg_rs_table_rows_suffice() {for (int kstart = 0; kstart <= F_TABLE_SIZE; ++kstart) {if (sg_rs_last_row_read(kstart, 27) >= SG_TABLE_ROWS) return false;} return true;}
static_assert(sg_rs_table_rows_suffice(), "k_sine_grid_rs's row prefetch would read behind the sine tables");

enum {MGEN_SINE = 0, MGEN_SIMPLEX, MGEN_PERLIN, MGEN_SIMPLEX_GPU, MGEN_DWARP_GPU}; // src/3DWorld.h:1399

// std::min / std::max semantics (NaN-propagation exactly as "(b<a)?b:a" / "(a<b)?b:a"), NOT fminf/fmaxf
TERRA_HD float min_std(float a, float b) {return (b < a) ? b : a;}
TERRA_HD float max_std(float a, float b) {return (a < b) ? b : a;}
// float <-> order-preserving uint (for atomic min/max of floats)
TERRA_HD uint32_t f2ord(float f) {uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u);}
TERRA_HD float ord2f(uint32_t o) {uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; float f; memcpy(&f, &u, 4); return f;}
TERRA_HD int   imin(int a, int b) {return (b < a) ? b : a;}
TERRA_HD int   imax(int a, int b) {return (a < b) ? b : a;}
TERRA_HD float clip01(float x)  {return max_std(0.0f, min_std(1.0f, x));}    // CLIP_TO_01  src/3DWorld.h:148
TERRA_HD float clip_pm1(float x) {return max_std(-1.0f, min_std(1.0f, x));}  // CLIP_TO_pm1 src/3DWorld.h:149
// float -> int with x86 cvttss2si semantics (NaN / out of range -> INT_MIN): what the reference binary does
TERRA_HD int f2i_x86(float f) {return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN;}
// double -> int with x86 cvttsd2si semantics: every double that truncates into the int range converts, NaN and the others give INT_MIN
TERRA_HD int d2i_x86(double v) {return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;}
// float / double -> unsigned as the reference binary converts them (cvttss2si / cvttsd2si to 64 bits, the low word): NaN and values beyond the 64-bit range give 0
TERRA_HD uint32_t f2u_x86(float f) {return (f > -9223372036854775808.0f && f < 9223372036854775808.0f) ? (uint32_t)(uint64_t)(int64_t)f : 0u;}
TERRA_HD uint32_t d2u_x86(double d) {return (d > -9223372036854775808.0 && d < 9223372036854775808.0) ? (uint32_t)(uint64_t)(int64_t)d : 0u;}
// int steps as the reference binary takes them: sums and differences wrap, abs(INT_MIN) == INT_MIN
TERRA_HD int add_wrap(int a, int b) {return (int)((uint32_t)a + (uint32_t)b);}
TERRA_HD int sub_wrap(int a, int b) {return (int)((uint32_t)a - (uint32_t)b);}
TERRA_HD int abs_x86(int v) {return (v < 0) ? (int)(0u - (uint32_t)v) : v;}

// do_line_clip (src/Math3d.cpp:1029-1086) with get_region (src/inlines.h:522-528): shared by the mesh shadows, the line queries and the terrain view, whose
// check_line_clip (get_line_clip, src/Math3d.cpp:1037-1052) is the same function without the two updates of the end points
struct shadow_pt_t {float x, y, z;};
TERRA_HD int shadow_region(shadow_pt_t v, float const d[3][2]) {
	int region = 0;
	if (v.x < d[0][0]) {region |= 0x01;} else if (v.x >= d[0][1]) {region |= 0x02;}
	if (v.y < d[1][0]) {region |= 0x04;} else if (v.y >= d[1][1]) {region |= 0x08;}
	if (v.z < d[2][0]) {region |= 0x10;} else if (v.z >= d[2][1]) {region |= 0x20;}
	return region;
}
TERRA_HD bool shadow_line_clip(shadow_pt_t &v1, shadow_pt_t &v2, float const d[3][2]) {
	int const region1 = shadow_region(v1, d), region2 = shadow_region(v2, d);
	if (region1 & region2) return false;
	int const region3 = region1 | region2;
	if (region3 == 0) return true;
	float tmin = 0.0f, tmax = 1.0f;
	shadow_pt_t const dv = {v2.x - v1.x, v2.y - v1.y, v2.z - v1.z};
#define TERRA_SH_CLIP(reg, va, vb, vd, vc) if (region3 & (reg)) {float const t = ((va) - (vb))/(vd); if ((vc) > 0.0f) {if (t > tmin) tmin = t;} else {if (t < tmax) tmax = t;} if (tmin >= tmax) return false;}
	TERRA_SH_CLIP(0x01, d[0][0], v1.x, dv.x,  dv.x)
	TERRA_SH_CLIP(0x02, d[0][1], v1.x, dv.x, -dv.x)
	TERRA_SH_CLIP(0x04, d[1][0], v1.y, dv.y,  dv.y)
	TERRA_SH_CLIP(0x08, d[1][1], v1.y, dv.y, -dv.y)
	TERRA_SH_CLIP(0x10, d[2][0], v1.z, dv.z,  dv.z)
	TERRA_SH_CLIP(0x20, d[2][1], v1.z, dv.z, -dv.z)
#undef TERRA_SH_CLIP
	if ((double)tmax > 1.0E-12) {v2.x = v1.x + dv.x*tmax; v2.y = v1.y + dv.y*tmax; v2.z = v1.z + dv.z*tmax;}
	if ((double)tmin < (1.0 - 1.0E-12)) {v1.x += dv.x*tmin; v1.y += dv.y*tmin; v1.z += dv.z*tmin;}
	return true;
}
// the reference's removal loops, literally: `for (i = 0; i < size; ++i) if (removed(i)) remove_element(v, i)` with remove_element (src/inlines.h:743-747) = swap with
// the back, pop, --i.  removed(i) tests record i and returning true is its removal, once; move(dst, src) copies the back and whatever travels with it into the hole
// (what the back receives is gone).  Returns the new size
template<class REMOVED, class MOVE> TERRA_HD uint32_t remove_elements_serial(uint32_t size, REMOVED removed, MOVE move) {
	for (uint32_t i = 0; i < size; ++i) {
		if (!removed(i)) continue;
		move(i, size - 1);
		--size;
		--i; // (wraps at 0 and comes back with the ++i, as the reference's unsigned does)
	}
	return size;
}

// ------------------------------------------------------------------ RNG (src/rand_gen.h:20-35,63-79; src/gen_object.cpp:377-381)
// L'Ecuyer combined LCG; the reference holds the state in `long`, values always fit in int32 after the first step.
struct rand_gen_t {
	int64_t rseed1, rseed2;
	TERRA_HD void set_state(int64_t s1, int64_t s2) {rseed1 = s1; rseed2 = s2;}
	TERRA_HD void advance() {
		if ((rseed1 = 40014*(rseed1%53668) - 12211*(rseed1/53668)) < 0) rseed1 += 2147483563;
		if ((rseed2 = 40692*(rseed2%52774) - 3791 *(rseed2/52774)) < 0) rseed2 += 2147483399;
	}
	TERRA_HD int rand() {
		advance();
		int v = (int)rseed1 - (int)rseed2;
		if (v < 1) v += 2147483562;
		return v;
	}
	TERRA_HD double randd() {
		advance();
		double v = (double)rseed1 - (double)rseed2;
		if (v < 1) v += 2147483562;
		return v/2147483563.;
	}
	TERRA_HD float rand_float() {return (float)(0.000001*(rand()%1000000));}                  // src/rand_gen.h:87
	TERRA_HD float rand_uniform(float a, float b) {return a + (b - a)*(float)randd();}        // src/rand_gen.h:91
};

// ------------------------------------------------------------------ SINF/COSF table lookup (src/sinf.h:8-21)
// The 2*TSIZE table itself is filled on the host with libm sinf/cosf exactly as create_sin_table() does
// (src/mesh_gen.cpp:72-81) and uploaded once per context.
struct sin_lut_t {
	float const *tab; // [2*TSIZE]: sin then cos
	float sscale;     // float(TSIZE)/TWO_PI
	// int(sscale*val) overflows for |val| > ~4e5 (estimate_zminmax samples at a 4000-cell spacing): the reference binary then gets
	// cvttss2si's 0x80000000 -> table index 0, so the x86 conversion is part of the function's definition
	TERRA_HD int st_scale(float v) const {return f2i_x86(sscale*v) & (TSIZE-1);}
	TERRA_HD float SINF(float v) const {return (v < 0) ? -tab[st_scale(-v)] : tab[st_scale(v)];}
	TERRA_HD float COSF(float v) const {return tab[TSIZE + st_scale(fabsf(v))];}
};

// hmap_params_t (src/mesh.h:84-88)
struct hmap_params_t {
	float plat_bot, plat_h, plat_s, plat_max, crat_h, crat_s, crack_lo, crack_hi, crack_d, sine_mag, sine_freq, sine_bias, volcano_width, volcano_height;
};

// Everything the per-cell evaluators read; mirrors the reference's process globals (SURVEY section 5 "Config / flags").
struct noise_consts_t {
	hmap_params_t hp;
	float mesh_scale, mesh_scale_z_inv, DX_VAL_INV, DY_VAL_INV, MESH_HEIGHT, mesh_height_scale;
	float zmax_est, zmax_est2, zmax_est2_inv, custom_glaciate_exp;
	float rx, ry;           // gen_rx_ry()
	int   start_eval_sin;   // compute_scale()
	int   glaciate;         // GLACIATE
};

} // namespace terra
