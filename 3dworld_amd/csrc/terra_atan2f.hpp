// terra_atan2f.hpp -- device/host atanf and atan2f with the EXACT results of glibc's libm (2.35: sysdeps/ieee754/flt-32/e_atan2f.c over s_atanf.c, the
// fdlibm-derived all-float routines: four breakpoints with hi / lo parts of their arctangents and an 11-term odd polynomial split into two chains).
//
// Why: line_intersect_trunc_cone (src/Math3d.cpp:556) takes the cone's half angle as cosf(atan2f(r2, |A|)) through libm, which is not correctly rounded; the
// device's ocml atan2f differs from it.  The restatement is evaluated with separate float multiplies, adds and divisions (the library is built with
// -ffp-contract=off) and is checked against libm over every 7th bit pattern (atanf) and 4*10^7 pairs over the four quadrants (atan2f) on the build host
// (tests/test_line_trees_emul.py).  The large-argument threshold is 0x4c000000 (|x| >= 2^25), as glibc has it, not fdlibm's 0x50800000.
#pragma once
#include "terra_common.hpp"

namespace terra {

TERRA_HD uint32_t atanf_asuint(float f) {uint32_t u; memcpy(&u, &f, 4); return u;}
TERRA_HD float atanf_asfloat(uint32_t u) {float f; memcpy(&f, &u, 4); return f;}

TERRA_HD float glibc_atanf(float x) {
	float const hi0 = 4.6364760399e-01f, hi1 = 7.8539812565e-01f, hi2 = 9.8279368877e-01f, hi3 = 1.5707962513e+00f; // atan(0.5), atan(1), atan(1.5), atan(inf)
	float const lo0 = 5.0121582440e-09f, lo1 = 3.7748947079e-08f, lo2 = 3.4473217170e-08f, lo3 = 7.5497894159e-08f;
	float const aT0 = 3.3333334327e-01f, aT1 = -2.0000000298e-01f, aT2 = 1.4285714924e-01f, aT3 = -1.1111110449e-01f, aT4 = 9.0908870101e-02f, aT5 = -7.6918758452e-02f,
		aT6 = 6.6610731184e-02f, aT7 = -5.8335702866e-02f, aT8 = 4.9768779427e-02f, aT9 = -3.6531571299e-02f, aT10 = 1.6285819933e-02f;
	uint32_t const hx = atanf_asuint(x), ix = hx & 0x7fffffffu;
	bool const neg = (hx >> 31) != 0;
	if (ix >= 0x4c000000u) { // |x| >= 2^25
		if (ix > 0x7f800000u) return x + x; // NaN
		float const r = hi3 + lo3;
		return neg ? -r : r;
	}
	int id;
	float hi = 0.0f, lo = 0.0f;
	if (ix < 0x3ee00000u) { // |x| < 0.4375
		if (ix < 0x31000000u) return x; // |x| < 2^-29
		id = -1;
	}
	else {
		x = atanf_asfloat(ix); // fabsf
		if (ix < 0x3f980000u) { // |x| < 1.1875
			if (ix < 0x3f300000u) {id = 0; hi = hi0; lo = lo0; x = (2.0f*x - 1.0f)/(2.0f + x);} // 7/16 <= |x| < 11/16
			else                  {id = 1; hi = hi1; lo = lo1; x = (x - 1.0f)/(x + 1.0f);}       // 11/16 <= |x| < 19/16
		}
		else {
			if (ix < 0x401c0000u) {id = 2; hi = hi2; lo = lo2; x = (x - 1.5f)/(1.0f + 1.5f*x);}  // |x| < 2.4375
			else                  {id = 3; hi = hi3; lo = lo3; x = -1.0f/x;}
		}
	}
	float z = x*x;
	float const w = z*z;
	float const s1 = z*(aT0 + w*(aT2 + w*(aT4 + w*(aT6 + w*(aT8 + w*aT10)))));
	float const s2 = w*(aT1 + w*(aT3 + w*(aT5 + w*(aT7 + w*aT9))));
	if (id < 0) return x - x*(s1 + s2);
	z = hi - ((x*(s1 + s2) - lo) - x);
	return neg ? -z : z;
}

TERRA_HD float glibc_atan2f(float y, float x) {
	float const tiny = 1.0e-30f, pi_o_4 = atanf_asfloat(0x3f490fdbu), pi_o_2 = atanf_asfloat(0x3fc90fdbu), pi = atanf_asfloat(0x40490fdbu), pi_lo = atanf_asfloat(0xb3bbbd2eu);
	uint32_t const hx = atanf_asuint(x), hy = atanf_asuint(y), ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
	if (ix > 0x7f800000u || iy > 0x7f800000u) return x + y; // NaN
	if (hx == 0x3f800000u) return glibc_atanf(y);            // x == 1.0
	uint32_t const m = ((hy >> 31) & 1u) | ((hx >> 30) & 2u); // 2*sign(x) + sign(y)
	bool const yneg = (hy >> 31) != 0;
	if (iy == 0u) { // y == 0
		if (m < 2u) return y;                   // atan(+-0, +anything) = +-0
		return (m == 2u) ? pi + tiny : -pi - tiny;
	}
	if (ix == 0u) return yneg ? -pi_o_2 - tiny : pi_o_2 + tiny; // x == 0
	if (ix == 0x7f800000u) { // x is inf
		if (iy == 0x7f800000u) {
			switch (m) {
			case 0: return pi_o_4 + tiny;
			case 1: return -pi_o_4 - tiny;
			case 2: return 3.0f*pi_o_4 + tiny;
			default: return -3.0f*pi_o_4 - tiny;
			}
		}
		switch (m) {
		case 0: return 0.0f;
		case 1: return -0.0f;
		case 2: return pi + tiny;
		default: return -pi - tiny;
		}
	}
	if (iy == 0x7f800000u) return yneg ? -pi_o_2 - tiny : pi_o_2 + tiny; // y is inf
	int32_t const k = ((int32_t)iy - (int32_t)ix) >> 23;
	float z;
	if (k > 60) {z = pi_o_2 + 0.5f*pi_lo;}                    // |y/x| > 2^60
	else if ((hx >> 31) != 0 && k < -60) {z = 0.0f;}          // |y|/x < -2^60
	else {z = glibc_atanf(atanf_asfloat(atanf_asuint(y/x) & 0x7fffffffu));}
	switch (m) {
	case 0: return z;
	case 1: return atanf_asfloat(atanf_asuint(z) ^ 0x80000000u);
	case 2: return pi - (z - pi_lo);
	default: return (z - pi_lo) - pi;
	}
}

} // namespace terra
