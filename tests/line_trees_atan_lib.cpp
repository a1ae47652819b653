// line_trees_atan_lib.cpp -- terra_atan2f.hpp built for the host into a small shared library by tests/test_line_trees_emul.py and held against this machine's libm
// (atanf / atan2f called from here, with -fno-builtin so that they are libm's):
//   lt_atanf_sweep   every `stride`-th bit pattern of all floats from `first` on, both signs and the NaNs included -> the number of mismatches
//   lt_atan2f_pairs  n seeded pairs over the four quadrants: exponents of y and x drawn over the whole range in a third of the pairs (|k| > 60 in most of those),
//                    within +-30 of each other in the rest, zeros, denormals and infinities among them -> the number of mismatches; tally[0..3]: pairs per
//                    quadrant m, tally[4]: k > 60, tally[5]: k < -60 with x < 0, tally[6]: pairs that reached atanf(|y/x|)
//   lt_atan2f_eval   the restatement and libm on given arrays, for the special cases
// A NaN result matches a NaN result.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#include "../3dworld_amd/csrc/terra_atan2f.hpp"

static bool same(float a, float b) {
	uint32_t x, y; memcpy(&x, &a, 4); memcpy(&y, &b, 4);
	return x == y || (a != a && b != b);
}
static uint64_t splitmix(uint64_t &s) {uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30))*0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27))*0x94D049BB133111EBull; return z ^ (z >> 31);}

extern "C" {
uint64_t lt_atanf_sweep(uint32_t first, uint32_t stride, uint32_t threads, uint32_t *first_bad) {
	std::vector<uint64_t> bad(threads, 0);
	std::vector<uint32_t> where(threads, 0);
	uint64_t const total = ((uint64_t)0x100000000ull - first + stride - 1)/stride;
	std::vector<std::thread> pool;
	for (uint32_t w = 0; w < threads; ++w) {
		pool.emplace_back([&, w]() {
			for (uint64_t k = total*w/threads; k < total*(w + 1)/threads; ++k) {
				uint32_t const u = (uint32_t)(first + k*stride);
				float x; memcpy(&x, &u, 4);
				if (!same(terra::glibc_atanf(x), atanf(x))) {if (!bad[w]++) {where[w] = u;}}
			}
		});
	}
	for (auto &t : pool) {t.join();}
	uint64_t n = 0;
	for (uint32_t w = 0; w < threads; ++w) {if (bad[w] && !n && first_bad) {*first_bad = where[w];} n += bad[w];}
	return n;
}
uint64_t lt_atan2f_pairs(uint64_t seed, uint64_t n, uint32_t threads, uint64_t *tally, float *first_bad) {
	std::vector<uint64_t> bad(threads, 0);
	std::vector<std::vector<uint64_t>> tl(threads, std::vector<uint64_t>(7, 0));
	std::vector<float> where(2*threads, 0.0f);
	std::vector<std::thread> pool;
	for (uint32_t w = 0; w < threads; ++w) {
		pool.emplace_back([&, w]() {
			uint64_t s = seed + 0x1234567ull*w;
			for (uint64_t k = n*w/threads; k < n*(w + 1)/threads; ++k) {
				uint64_t const a = splitmix(s), b = splitmix(s);
				uint32_t ex = (uint32_t)(a >> 32) % 256u, ey;
				if (b % 3u == 0u) {ey = (uint32_t)(b >> 40) % 256u;}
				else {int const e = (int)ex + (int)((b >> 40) % 61u) - 30; ey = (uint32_t)(e < 0 ? 0 : (e > 255 ? 255 : e));}
				uint32_t ux = ((uint32_t)(a & 1u) << 31) | (ex << 23) | ((uint32_t)(a >> 8) & 0x7FFFFFu), uy = ((uint32_t)(b & 1u) << 31) | (ey << 23) | ((uint32_t)(b >> 8) & 0x7FFFFFu);
				if (((a >> 4) & 15u) == 0u) {ux &= 0xFF800000u;} // powers of two, zeros and infinities
				if (((b >> 4) & 15u) == 0u) {uy &= 0xFF800000u;}
				float x, y; memcpy(&x, &ux, 4); memcpy(&y, &uy, 4);
				if (x != x || y != y) continue; // (the NaNs are among the special cases)
				uint32_t const ix = ux & 0x7FFFFFFFu, iy = uy & 0x7FFFFFFFu;
				int const kk = ((int)iy - (int)ix) >> 23;
				++tl[w][((uy >> 31) & 1u) | ((ux >> 30) & 2u)];
				bool const plain = ix != 0 && iy != 0 && ix != 0x7F800000u && iy != 0x7F800000u && ux != 0x3F800000u;
				if (plain && kk > 60) {++tl[w][4];} else if (plain && (ux >> 31) && kk < -60) {++tl[w][5];} else if (plain) {++tl[w][6];}
				if (!same(terra::glibc_atan2f(y, x), atan2f(y, x))) {if (!bad[w]++) {where[2*w] = y; where[2*w + 1] = x;}}
			}
		});
	}
	for (auto &t : pool) {t.join();}
	uint64_t nb = 0;
	for (uint32_t w = 0; w < threads; ++w) {
		if (bad[w] && !nb && first_bad) {first_bad[0] = where[2*w]; first_bad[1] = where[2*w + 1];}
		nb += bad[w];
		for (int q = 0; q < 7; ++q) {tally[q] += tl[w][q];}
	}
	return nb;
}
void lt_atan2f_eval(float const *y, float const *x, uint32_t n, float *ours, float *libm, float *ours1, float *libm1) {
	for (uint32_t i = 0; i < n; ++i) {ours[i] = terra::glibc_atan2f(y[i], x[i]); libm[i] = atan2f(y[i], x[i]); ours1[i] = terra::glibc_atanf(y[i]); libm1[i] = atanf(y[i]);}
}
}
