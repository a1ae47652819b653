// terra_sincosf.hpp -- device/host sinf/cosf with the EXACT results of glibc's libm (2.28+: sysdeps/ieee754/flt-32/
// s_sinf.c, s_cosf.c, sincosf.h, sincosf_data.c = ARM optimized-routines' sincosf, fp64 polynomial, result rounded to float).
//
// Why: the droplet's "pick a random direction" branch calls libm cosf(a)/sinf(a) (src/erosion.cpp:80-83).  glibc's
// sinf/cosf are NOT correctly rounded: on the 10^6 possible arguments a = rand_float()*TWO_PI they differ from
// (float)cos((double)a) in 2.6% of the cases, so neither the device's ocml sinf/cosf nor a correctly-rounded evaluation
// reproduces the reference there.
//
// Which glibc: on x86-64 the library picks, on every CPU that has FMA, its build of these files WITH fused multiply-adds
// (sysdeps/x86_64/fpu/multiarch/s_sinf.c: __sinf_fma), and that is the function a reference binary calls.  Every `a + b*c`
// of the source is one rounding there.  In the polynomials this moves a result by at most one double ulp; in the reduction
// x - n*(pi/2) next to a multiple of pi/2 it decides bits a float keeps (sinf(74*pi/2) differs in the last place).  The
// fused operations are written out with fma() -- the library is built without contraction, so nothing else fuses.
// The whole domain is covered: |y| < pi/4, the fast reduction below 120, the 4/pi table reduction up to infinity, and
// NaN for an infinity or a NaN (tests/test_primitives_host.py and tests/test_gpu_primitives.py against the C library).
#pragma once
#include "terra_common.hpp"

namespace terra {

struct sincosf_tab_t {double hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3;};

TERRA_HD float sincosf_poly(double x, double x2, bool neg_tab, int n) {
	// __sincosf_table[0] / [1]: the second table is the first with c0..c4 negated
	double const sg = neg_tab ? -1.0 : 1.0;
	double const c0 = sg*0x1p0, c1 = sg*-0x1.ffffffd0c621cp-2, c2 = sg*0x1.55553e1068f19p-5, c3 = sg*-0x1.6c087e89a359dp-10, c4 = sg*0x1.99343027bf8c3p-16;
	double const s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
	if ((n & 1) == 0) {
		double const x3 = x*x2, t1 = fma(x2, s3, s2), x5 = x3*x2, s = fma(x3, s1, x);
		return (float)fma(x5, t1, s);
	}
	double const x4 = x2*x2, t2 = fma(x2, c4, c3), t1 = fma(x2, c1, c0), x6 = x4*x2, c = fma(x4, c2, t1);
	return (float)fma(x6, t2, c);
}
TERRA_HD uint32_t sincosf_abstop12(float x) {uint32_t u; memcpy(&u, &x, 4); return (u >> 20) & 0x7ff;}

// reduce_large: |y| >= 120.  The 24 + shift bits of the mantissa times 96 bits of 4/pi picked by the exponent; the top two bits of the product are the quadrant,
// the rest, as a signed 62-bit fraction of pi/4, the reduced argument.  Rare (never on the droplet path) and out of line
struct sincosf_reduced_t {double x; int n;};
TERRA_HD_COLD sincosf_reduced_t sincosf_reduce_large(uint32_t xi) {
	uint32_t const inv_pio4[24] = {0xa2u, 0xa2f9u, 0xa2f983u, 0xa2f9836eu, 0xf9836e4eu, 0x836e4e44u, 0x6e4e4415u, 0x4e441529u, 0x441529fcu, 0x1529fc27u, 0x29fc2757u, 0xfc2757d1u,
		0x2757d1f5u, 0x57d1f534u, 0xd1f534ddu, 0xf534ddc0u, 0x34ddc0dbu, 0xddc0db62u, 0xc0db6295u, 0xdb629599u, 0x6295993cu, 0x95993c43u, 0x993c4390u, 0x3c439041u};
	uint32_t const *arr = &inv_pio4[(xi >> 26) & 15];
	int const shift = (int)((xi >> 23) & 7);
	xi = (xi & 0xffffffu) | 0x800000u;
	xi <<= shift;
	uint64_t res0 = (uint64_t)(uint32_t)(xi*arr[0]); // the low word of the product, as the 32-bit multiply of the source leaves it
	uint64_t const res1 = (uint64_t)xi*arr[4], res2 = (uint64_t)xi*arr[8];
	res0 = (res2 >> 32) | (res0 << 32);
	res0 += res1;
	uint64_t const n = (res0 + (1ull << 61)) >> 62;
	res0 -= n << 62;
	sincosf_reduced_t const r = {(double)(int64_t)res0*0x1.921FB54442D18p-62, (int)n};
	return r;
}

// is_cos = false: sinf(y), true: cosf(y), for |y| < 120 ONLY: the two branches every caller on a hot path needs.  The droplets' a = rand_float()*TWO_PI lies in
// [0, 2*pi), and a kernel that carried the large-argument branch as well would pay for it in registers on every thread
TERRA_HD float glibc_sincosf_below_120(float y, bool is_cos) {
	double x = (double)y;
	if (sincosf_abstop12(y) < sincosf_abstop12(0x1.921FB6p-1f)) { // |y| < pi/4
		double const x2 = x*x;
		if (sincosf_abstop12(y) < sincosf_abstop12(0x1p-12f)) {return is_cos ? 1.0f : y;}
		return sincosf_poly(x, x2, false, is_cos ? 1 : 0);
	}
	// reduce_fast: n = round(x * 2/pi), x -= n*pi/2
	double const r = x*0x1.45F306DC9C883p+23;
	int const n = ((int32_t)r + 0x800000) >> 24;
	x = fma(-(double)n, 0x1.921FB54442D18p0, x);
	double const sign = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0; // sign[] = {1,-1,-1,1}
	return sincosf_poly(x*sign, x*x, (n & 2) != 0, is_cos ? (n ^ 1) : n);
}
// the whole function
TERRA_HD float glibc_sincosf(float y, bool is_cos) {
	if (TERRA_LIKELY(sincosf_abstop12(y) < sincosf_abstop12(120.0f))) return glibc_sincosf_below_120(y, is_cos);
	if (sincosf_abstop12(y) < sincosf_abstop12(__builtin_inff())) {
		uint32_t xi; memcpy(&xi, &y, 4);
		sincosf_reduced_t const rl = sincosf_reduce_large(xi);
		int const n = rl.n, q = is_cos ? n : n + (int)(xi >> 31); // sinf folds the argument's sign into the quadrant, cosf is even
		double const sign = ((q & 3) == 1 || (q & 3) == 2) ? -1.0 : 1.0;
		return sincosf_poly(rl.x*sign, rl.x*rl.x, (q & 2) != 0, is_cos ? (n ^ 1) : n);
	}
	return (y - y)/(y - y); // __math_invalidf: NaN for an infinity or a NaN
}
TERRA_HD float glibc_sinf(float y) {return glibc_sincosf(y, false);}
TERRA_HD float glibc_cosf(float y) {return glibc_sincosf(y, true);}
TERRA_HD float glibc_sinf_below_120(float y) {return glibc_sincosf_below_120(y, false);}
TERRA_HD float glibc_cosf_below_120(float y) {return glibc_sincosf_below_120(y, true);}

} // namespace terra
