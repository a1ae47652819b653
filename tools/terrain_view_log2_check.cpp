// tools/terrain_view_log2_check.cpp -- stand-alone host program (no GPU): terrain_view_log2 (3dworld_amd/csrc/terra_terrainview.hpp), the plain-double log2 that
// get_lod_level's `dist /= -log2(2.0*min_normal_z)` (src/tiled_mesh.cpp:1924) uses on the host and on the device alike, against the C library's log2 for EVERY float
// min_normal_z in (0, 0.25) -- the only values that reach the statement.
//
// It reports (1) how many of the doubles -log2(2.0*min_normal_z) differ between the two, with the largest difference in units of the last place, and (2) for how
// many of those some float dist exists whose narrowed quotient float(double(dist)/L) differs between the two divisors.  (2) is searched, not enumerated (2^23
// mantissas a value would be 10^16 divisions): two quotients of D (a 24-bit integer; the power of two of dist does not matter away from the subnormals) round to
// different floats only if a rounding boundary (M + 1/2)*2^-e lies between them, that is if some L* between the two divisors has L*/2^(e+1) = D/(2M + 1) exactly.
// The divisors are a few ulps apart, so |L/2^(e+1) - D/Q| < 2^-51 <= 1/(2 Q^2) for the odd Q = 2M + 1 < 2^25: D/Q is a multiple of a continued-fraction convergent of
// L/2^(e+1) (Legendre).  The program walks the convergents p/q with odd q < 2^25 of both divisors for the two e that can occur, and tries every odd multiple c with
// c*p in [2^23, 2^24) of a convergent that lies between the divisors (give or take 8 times their distance) by doing the two divisions as the statement does them.  What it finds is a witness; what it does not find does not exist while the divisors
// are within 2 ulps (double rounding of the quotient aside).
//
// build: g++ -std=c++17 -O2 -ffp-contract=off -pthread [-fsanitize=address,undefined] -o terrain_view_log2_check tools/terrain_view_log2_check.cpp
// usage: terrain_view_log2_check [threads = 8] [first float bits = 1] [last float bits = 0x3E7FFFFF]
#include "../3dworld_amd/csrc/terra_terrainview.hpp"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static bool quotient_differs(uint32_t D, double la, double lb) {
	float const d = (float)D;
	return (float)((double)d/la) != (float)((double)d/lb);
}
// the convergents of x = l/2^(e+1), l > 0: x = mant*2^ex exactly
static bool witness_for(double l, int e, double la, double lb, uint32_t &D_out) {
	int ex;
	double const fr = frexp(l, &ex); // l = fr*2^ex, fr in [0.5, 1)
	unsigned __int128 num = (unsigned __int128)(uint64_t)ldexp(fr, 53), den = 1; // l = num*2^(ex - 53)
	int const sh = ex - 53 - (e + 1); // x = num*2^sh
	if (sh >= 0) {if (sh > 60) return false; num <<= sh;} else {if (-sh > 120) return false; den <<= -sh;}
	uint64_t p0 = 0, q0 = 1, p1 = 1, q1 = 0; // p(-2)/q(-2), p(-1)/q(-1)
	for (int it = 0; it < 64 && den != 0; ++it) {
		unsigned __int128 const a = num/den, r = num - a*den;
		if (a > (unsigned __int128)1 << 40) break;
		uint64_t const p = (uint64_t)a*p1 + p0, q = (uint64_t)a*q1 + q0;
		if (q >= (1ull << 25) || p >= (1ull << 24)) break;
		// (only a convergent that lies between the two divisors, give or take a few ulps, can be the D/Q of a boundary: its multiples are not worth their divisions otherwise)
		long double const at = ldexpl((long double)p/(long double)q, e + 1), lmin = (la < lb) ? la : lb, lmax = (la < lb) ? lb : la, slack = 8.0L*(lmax - lmin);
		if ((q & 1ull) && p > 0 && at >= lmin - slack && at <= lmax + slack) {
			for (uint64_t c = 1; c*q < (1ull << 25) && c*p < (1ull << 24); c += 2) {
				if (c*p >= (1ull << 23) && quotient_differs((uint32_t)(c*p), la, lb)) {D_out = (uint32_t)(c*p); return true;}
			}
		}
		p0 = p1; q0 = q1; p1 = p; q1 = q;
		num = den; den = r;
	}
	return false;
}
static bool could_change(double la, double lb, uint32_t &D_out) {
	int ex;
	frexp(la, &ex); // la in [2^(ex-1), 2^ex): D/la*2^e in [2^23, 2^24) for D in [2^23, 2^24) needs e = ex - 1 or ex
	for (int e = ex - 2; e <= ex + 1; ++e) {
		if (witness_for(la, e, la, lb, D_out) || witness_for(lb, e, la, lb, D_out)) return true;
	}
	return false;
}

struct tally_t {uint64_t values = 0, differ = 0, could = 0, max_ulps = 0; uint32_t first_bits = 0, first_D = 0;};

int main(int argc, char **argv) {
	unsigned const nthreads = (argc > 1) ? (unsigned)atoi(argv[1]) : 8u;
	uint32_t const lo = (argc > 2) ? (uint32_t)strtoul(argv[2], nullptr, 0) : 1u, hi = (argc > 3) ? (uint32_t)strtoul(argv[3], nullptr, 0) : 0x3E7FFFFFu; // 0x3E800000 is 0.25f
	if (nthreads == 0 || lo == 0 || hi > 0x3E7FFFFFu || lo > hi) {fprintf(stderr, "usage: %s [threads] [first bits >= 1] [last bits <= 0x3E7FFFFF]\n", argv[0]); return 2;}
	std::vector<tally_t> tallies(nthreads);
	std::vector<std::thread> pool;
	for (unsigned w = 0; w < nthreads; ++w) {
		pool.emplace_back([&, w] {
			tally_t &T = tallies[w];
			for (uint64_t u = (uint64_t)lo + w; u <= hi; u += nthreads) { // interleaved: every thread sees every exponent
				uint32_t const bits = (uint32_t)u;
				float f; memcpy(&f, &bits, 4);
				double const x = 2.0*(double)f, la = -log2(x), lb = -terra::terrain_view_log2(x);
				++T.values;
				if (la == lb) continue;
				++T.differ;
				int64_t ia, ib; memcpy(&ia, &la, 8); memcpy(&ib, &lb, 8);
				uint64_t const ulps = (uint64_t)((ia > ib) ? ia - ib : ib - ia);
				if (ulps > T.max_ulps) {T.max_ulps = ulps;}
				uint32_t D;
				if (could_change(la, lb, D)) {if (!T.could) {T.first_bits = bits; T.first_D = D;} ++T.could;}
			}
		});
	}
	for (auto &t : pool) {t.join();}
	tally_t S;
	for (tally_t const &T : tallies) {
		S.values += T.values; S.differ += T.differ; S.could += T.could; if (T.max_ulps > S.max_ulps) {S.max_ulps = T.max_ulps;}
		if (T.could && !S.first_D) {S.first_bits = T.first_bits; S.first_D = T.first_D;}
	}
	// the rest of the shared header's host side, once: the LOD of a steep tile near the loop's threshold, and behind_sphere_mult
	terra::terrain_view_consts_t c; memset(&c, 0, sizeof(c)); c.S = 128; c.water_enabled = 1;
	uint32_t const lod = terra::terrain_view_lod(c, 0.0f, 1.0f, 0.01f, 11.3f, false);
	float const bsm = terra::view_behind_sphere_mult(0.5236f, 16.0f/9.0f);
	printf("{\"floats\": %llu, \"doubles_differ\": %llu, \"max_ulps\": %llu, \"could_change_float_quotient\": %llu, \"first_witness_bits\": \"0x%08X\", \"first_witness_dist\": %u, "
	       "\"lod_sample\": %u, \"behind_sphere_mult_sample\": %.9g}\n", (unsigned long long)S.values, (unsigned long long)S.differ, (unsigned long long)S.max_ulps,
	       (unsigned long long)S.could, S.first_bits, S.first_D, lod, (double)bsm);
	return 0;
}
