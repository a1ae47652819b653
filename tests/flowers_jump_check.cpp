// tests/flowers_jump_check.cpp -- TEST INFRASTRUCTURE (built and run by tests/test_flowers_emul.py, no GPU): the generator's jump-ahead of
// 3dworld_amd/csrc/terra_flowers.hpp, which k_flowers_place rests on, against literal stepping.
//   * lcg_mulmod against the 64-bit remainder, lcg_powmod against repeated multiplication;
//   * for seeds of every sign (a tile with negative coordinates seeds with values <= 0; the reference holds them in `long`): after ONE literal step the state lies in
//     [0, m) and the state k further steps on equals lcg_jump by the k-th powers, for the 32-bit generator the kernels use and for the `long` form of the reference;
//   * lcg_state_randd / lcg_state_signed_rand_float of a state equal what randd() / signed_rand_float() returned on the step that produced it;
//   * the kernel's (candidate, acceptances before it) pairs: every pair's stream offset lies inside the kernel's power table.
#include "../3dworld_amd/csrc/terra_flowers.hpp"
#include <cstdio>
using namespace terra;

static int problems = 0;
#define CHECK(c, ...) do {if (!(c)) {if (++problems <= 10) {printf(__VA_ARGS__); printf("\n");}}} while (0)

int main() {
	uint32_t const edge1[] = {0u, 1u, 2u, 84u, 85u, 86u, 40014u, 53668u, 0x3FFFFFFFu, 0x40000000u, LCG_M1 - 2u, LCG_M1 - 1u};
	uint32_t const edge2[] = {0u, 1u, 2u, 248u, 249u, 250u, 40692u, 52774u, 0x3FFFFFFFu, 0x40000000u, LCG_M2 - 2u, LCG_M2 - 1u};
	for (uint32_t a : edge1) {for (uint32_t b : edge1) {CHECK(lcg_mulmod<LCG_M1>(a, b) == (uint32_t)(((uint64_t)a*b) % LCG_M1), "mulmod M1 %u %u", a, b);}}
	for (uint32_t a : edge2) {for (uint32_t b : edge2) {CHECK(lcg_mulmod<LCG_M2>(a, b) == (uint32_t)(((uint64_t)a*b) % LCG_M2), "mulmod M2 %u %u", a, b);}}
	uint64_t x = 88172645463325252ull; // xorshift64: reproducible operands
	for (int i = 0; i < 2000000; ++i) {
		x ^= x << 13; x ^= x >> 7; x ^= x << 17;
		uint32_t const a = (uint32_t)(x % LCG_M1), b = (uint32_t)((x >> 32) % LCG_M1), c = (uint32_t)(x % LCG_M2), d = (uint32_t)((x >> 32) % LCG_M2);
		CHECK(lcg_mulmod<LCG_M1>(a, b) == (uint32_t)(((uint64_t)a*b) % LCG_M1), "mulmod M1 %u %u", a, b);
		CHECK(lcg_mulmod<LCG_M2>(c, d) == (uint32_t)(((uint64_t)c*d) % LCG_M2), "mulmod M2 %u %u", c, d);
	}
	uint32_t p1 = 1u, p2 = 1u;
	for (uint32_t k = 0; k < 300u; ++k) {
		CHECK(lcg_powmod<LCG_M1>(LCG_A1, k) == p1 && lcg_powmod<LCG_M2>(LCG_A2, k) == p2, "powmod %u", k);
		p1 = (uint32_t)(((uint64_t)p1*LCG_A1) % LCG_M1); p2 = (uint32_t)(((uint64_t)p2*LCG_A2) % LCG_M2);
	}
	// seeds as flower_seed forms them (tile*S + 123, tile*S + 456) and the corners of the int range
	int32_t const seeds[][2] = {{1, 1}, {123, 456}, {0, 0}, {0, 456}, {123, 0}, {-17, -4}, {-1, -1}, {-53668, -52774}, {-53669, -52775}, {53668, 52774}, {-140 + 123, -460 + 456},
		{-1000000, 999999}, {2147483647, 2147483647}, {-2147483647 - 1, -2147483647 - 1}, {2147483563, 2147483399}, {-2147483563, -2147483399}, {-128*5000 + 123, 128*7000 + 456}};
	uint32_t const K = 5000u;
	for (auto const &sd : seeds) {
		tree_rgen_t s; s.set_state(sd[0], sd[1]);
		rand_gen_t l; l.set_state(sd[0], sd[1]);
		s.advance(); l.advance(); // the first step literally
		CHECK(s.rseed1 >= 0 && (uint32_t)s.rseed1 < LCG_M1 && s.rseed2 >= 0 && (uint32_t)s.rseed2 < LCG_M2, "seeds %d %d: the first step leaves [0, m)", sd[0], sd[1]);
		CHECK(l.rseed1 == s.rseed1 && l.rseed2 == s.rseed2, "seeds %d %d: the long form differs after the first step", sd[0], sd[1]);
		tree_rgen_t const base = s;
		tree_rgen_t draw; draw.set_state(sd[0], sd[1]);
		uint32_t q1 = 1u, q2 = 1u;
		for (uint32_t k = 0; k < K; ++k) {
			tree_rgen_t const j = lcg_jump(base, q1, q2);
			CHECK(j.rseed1 == s.rseed1 && j.rseed2 == s.rseed2 && l.rseed1 == s.rseed1 && l.rseed2 == s.rseed2, "seeds %d %d: %u steps on", sd[0], sd[1], k);
			// `draw` is one step behind: the draw it makes now is the one state s stands for
			tree_rgen_t d2 = draw;
			CHECK(draw.randd() == lcg_state_randd(j), "seeds %d %d: randd of step %u", sd[0], sd[1], k);
			CHECK(d2.signed_rand_float() == lcg_state_signed_rand_float(j), "seeds %d %d: signed_rand_float of step %u", sd[0], sd[1], k);
			s.advance(); l.advance();
			q1 = lcg_mulmod<LCG_M1>(q1, LCG_A1); q2 = lcg_mulmod<LCG_M2>(q2, LCG_A2);
		}
		// a far jump by binary powers, as a candidate late in a tile's stream would need
		tree_rgen_t const far = lcg_jump(base, lcg_powmod<LCG_M1>(LCG_A1, K), lcg_powmod<LCG_M2>(LCG_A2, K));
		CHECK(far.rseed1 == s.rseed1 && far.rseed2 == s.rseed2, "seeds %d %d: the jump by %u", sd[0], sd[1], K);
	}
	// the speculative block: candidate l with a acceptances before it draws at offset l + E*a; after nb candidates with a acceptances the stream stands nb + E*a on
	uint32_t const B = 10u, POW = 91u; // FLW_B, FLW_POW of terra_kernels.hpp
	for (uint32_t E = 7u; E <= 8u; ++E) {
		for (uint32_t l = 0; l < B; ++l) {for (uint32_t a = 0; a <= l; ++a) {CHECK(l + E*a < POW && l*(l + 1)/2 + a < 64u, "pair %u %u", l, a);}}
		CHECK(B + E*B < POW, "block advance");
	}
	printf("flowers_jump_check: %s (%d problems)\n", problems ? "FAILED" : "ok", problems);
	return problems ? 1 : 0;
}
