// tests/flowers_wave_check.cpp -- TEST INFRASTRUCTURE (built and run by tests/test_flowers_emul.py, no GPU): the speculative walk of k_flowers_place
// (3dworld_amd/csrc/terra_kernels.hpp) restated for 64 lanes in lockstep on the host, statement for statement -- the chunks of 64 cells and their prefix sums, the
// candidate table and the searching form behind it, the blocks of ten candidates with their 55 (candidate, acceptances before it) pairs, the outcome mask and the
// walk over it, the queue of accepted states and when it is flushed, the base state's jump -- against flower_gen_serial, the reference's literal loop
// (3dworld_amd/csrc/terra_flowers.hpp), on random weights and fields: whole tiles and rectangles, both colour modes, densities with up to five candidates a cell,
// tiles whose seeds are <= 0, capacities below the count.  What it cannot show is the HIP code's own lane mechanics; the GPU tests do.
#include "../3dworld_amd/csrc/terra_flowers.hpp"
#include <cstdio>
#include <vector>
using namespace terra;

static int problems = 0;
#define CHECK(c, ...) do {if (!(c)) {if (++problems <= 10) {printf(__VA_ARGS__); printf("\n");}}} while (0)
constexpr uint32_t FLW_B = 10, FLW_PAIRS = FLW_B*(FLW_B + 1)/2, FLW_POW = FLW_B*9 + 1, FLW_Q = 64, FLW_MAP = 256, LANES = 64;

static uint32_t wave_place(flower_consts_t const &c, int tx, int ty, uint32_t xl, uint32_t yl, uint32_t xh, uint32_t yh, uint8_t const *w, float const *dn, float const *cl,
	uint32_t capacity, flower_pod_t *out, uint32_t *out_aux, uint32_t count, uint32_t &searched)
{
	uint32_t s_p1[FLW_POW], s_p2[FLW_POW], s_pre[65], s_cc[FLW_MAP], s_q[3*FLW_Q]; float s_cd[FLW_MAP];
	uint32_t const S = (uint32_t)c.S;
	for (uint32_t k = 0; k < FLW_POW; ++k) {s_p1[k] = lcg_powmod<LCG_M1>(LCG_A1, k); s_p2[k] = lcg_powmod<LCG_M2>(LCG_A2, k);}
	uint32_t const nx = xh - xl, ncells = nx*(yh - yl);
	uint32_t const E = c.fixed_color ? 7u : 8u;
	uint32_t pl[LANES], pa[LANES];
	for (uint32_t lane = 0; lane < LANES; ++lane) {pl[lane] = 0; while ((pl[lane] + 1)*(pl[lane] + 2)/2 <= lane) {++pl[lane];} pa[lane] = lane - pl[lane]*(pl[lane] + 1)/2;}
	tree_rgen_t cur;
	flower_seed(c.S, tx, ty, (int)xl, (int)yl, cur);
	cur.advance();
	uint32_t qn = 0;
	auto flush = [&]() {
		for (uint32_t lane = 0; lane < qn; ++lane) {
			tree_rgen_t rg; rg.rseed1 = (int32_t)s_q[lane]; rg.rseed2 = (int32_t)s_q[FLW_Q + lane];
			uint32_t const cell = s_q[2*FLW_Q + lane], x = cell & 1023u, y = cell >> 10;
			flower_pod_t o;
			uint32_t const cf = flower_record(c, (int)x, (int)y, cl[(size_t)y*S + x], rg, o);
			if (count + lane < capacity) {out[count + lane] = o; if (out_aux) {out_aux[count + lane] = flower_aux(x, y, cf);}}
		}
		count += qn; qn = 0;
	};
	for (uint32_t base = 0; base < ncells; base += 64) {
		uint32_t npb[LANES], cell[LANES], incl[LANES]; float dval[LANES];
		uint32_t run = 0;
		for (uint32_t lane = 0; lane < LANES; ++lane) {
			uint32_t const k = base + lane;
			npb[lane] = 0; cell[lane] = 0; dval[lane] = 0.0f;
			if (k < ncells) {
				uint32_t const y = yl + k/nx, x = xl + k%nx;
				npb[lane] = flower_num_per_bin(c, w[4*((size_t)y*(S + 1) + x) + 2]);
				if (npb[lane]) {dval[lane] = dn[(size_t)y*S + x];}
				cell[lane] = x | (y << 10);
			}
			run += npb[lane]; incl[lane] = run;
		}
		uint32_t const total = incl[63];
		if (total == 0) continue;
		bool const mapped = total <= FLW_MAP;
		if (!mapped) {++searched;}
		for (uint32_t lane = 0; lane < LANES; ++lane) {
			if (mapped) {for (uint32_t i = 0; i < npb[lane]; ++i) {s_cd[incl[lane] - npb[lane] + i] = dval[lane]; s_cc[incl[lane] - npb[lane] + i] = cell[lane];}}
			else {s_pre[lane] = incl[lane] - npb[lane]; if (lane == 63) {s_pre[64] = incl[lane];}}
		}
		for (uint32_t kb = 0; kb < total; kb += FLW_B) {
			uint32_t const nb = (total - kb < FLW_B) ? total - kb : FLW_B;
			uint32_t owner[LANES]; bool acc[LANES];
			unsigned long long mask = 0;
			for (uint32_t lane = 0; lane < LANES; ++lane) {
				bool const live = lane < FLW_PAIRS && pl[lane] < nb;
				owner[lane] = 0;
				float dv = 0.0f;
				if (mapped) {if (live) {dv = s_cd[kb + pl[lane]];}}
				else {
					if (live) {
						uint32_t const ci = kb + pl[lane];
						uint32_t lo = 0, hi = 64;
						while (hi - lo > 1) {uint32_t const mid = (lo + hi) >> 1; if (s_pre[mid] <= ci) {lo = mid;} else {hi = mid;}}
						owner[lane] = lo;
					}
					dv = dval[owner[lane]];
				}
				acc[lane] = false;
				if (live) {
					uint32_t const off = pl[lane] + E*pa[lane];
					CHECK(off < FLW_POW, "pair offset");
					acc[lane] = !((double)dv + c.zs*(double)lcg_state_signed_rand_float(lcg_jump(cur, s_p1[off], s_p2[off])) > (double)c.hthresh);
				}
				if (acc[lane]) {mask |= 1ull << lane;}
			}
			uint32_t a = 0, my_a[LANES] = {0}; bool my_acc[LANES] = {false};
			for (uint32_t l = 0; l < FLW_B; ++l) {
				uint32_t const bit = (l < nb) ? (uint32_t)((mask >> (l*(l + 1)/2 + a)) & 1ull) : 0u;
				my_a[l] = a; my_acc[l] = bit != 0;
				a += bit;
			}
			for (uint32_t lane = 0; lane < LANES; ++lane) {
				uint32_t my_cell;
				if (mapped) {my_cell = (lane < nb) ? s_cc[kb + lane] : 0u;}
				else {uint32_t const lc = (lane < FLW_B) ? lane : 0u; my_cell = cell[owner[lc*(lc + 1)/2]];}
				if (lane < FLW_B && my_acc[lane]) {
					uint32_t const off = lane + E*my_a[lane];
					tree_rgen_t const st = lcg_jump(cur, s_p1[off], s_p2[off]);
					CHECK(qn + my_a[lane] < FLW_Q, "queue overflow");
					s_q[qn + my_a[lane]] = (uint32_t)st.rseed1; s_q[FLW_Q + qn + my_a[lane]] = (uint32_t)st.rseed2; s_q[2*FLW_Q + qn + my_a[lane]] = my_cell;
				}
			}
			qn += a;
			CHECK(nb + E*a < FLW_POW, "block advance");
			cur = lcg_jump(cur, s_p1[nb + E*a], s_p2[nb + E*a]);
			if (qn + FLW_B > FLW_Q) {flush();}
		}
	}
	if (qn) {flush();}
	return count;
}

int main() {
	uint64_t x = 0x9E3779B97F4A7C15ull;
	auto rnd = [&]() {x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 32);};
	uint32_t total_flowers = 0, searched = 0, cut = 0, trials = 0;
	uint8_t const pattern[7] = {0, 1, 127, 128, 191, 192, 255};
	for (int trial = 0; trial < 120; ++trial) {
		flower_consts_t c;
		c.S = (trial % 3 == 0) ? 16 : ((trial % 3 == 1) ? 20 : 37);
		c.DX_VAL = c.DY_VAL = 8.0f/(float)c.S; c.DX_VAL_INV = c.DY_VAL_INV = 1.0f/c.DX_VAL;
		float const dens[5] = {2.0f, 0.8f, 5.3f, 1.0f, 9.7f};
		c.flower_density = dens[trial % 5]; c.grass_length = 0.02f; c.grass_width = 0.002f;
		c.fixed_color = (trial % 4 == 1) ? 1 : 0;
		c.color[0] = 0.9f; c.color[1] = 0.25f; c.color[2] = 0.5f; c.color[3] = c.fixed_color ? 1.0f : 0.0f;
		c.hthresh = 0.1f*(float)((int)(rnd() % 11u) - 5); c.zs = 0.2*1.3;
		uint32_t const S = (uint32_t)c.S;
		std::vector<uint8_t> w((size_t)(S + 1)*(S + 1)*4);
		std::vector<float> dn((size_t)S*S), cl((size_t)S*S);
		int const wkind = trial % 6; // all 255, the thresholds, random bytes, mostly nothing
		for (size_t i = 0; i < w.size(); ++i) {w[i] = (wkind == 0) ? 255 : ((wkind <= 2) ? pattern[(i/4 + (size_t)trial) % 7] : ((wkind <= 4) ? (uint8_t)rnd() : ((rnd() % 9u) ? 0 : 255)));}
		for (size_t i = 0; i < dn.size(); ++i) {dn[i] = (float)((int)(rnd() % 2001u) - 1000)*0.001f; cl[i] = (float)((int)(rnd() % 12001u) - 6000)*0.001f;}
		int const tx = (trial % 7 == 2) ? -(int)(rnd() % 40u) - 7 : (int)(rnd() % 9u) - 4, ty = (trial % 7 == 3) ? -(int)(rnd() % 40u) - 30 : (int)(rnd() % 9u) - 4;
		uint32_t xl = 0, yl = 0, xh = S, yh = S;
		if (trial % 2) {xl = rnd() % S; xh = xl + 1 + rnd() % (S - xl); yl = rnd() % S; yh = yl + 1 + rnd() % (S - yl);} // an update_subrange rectangle
		uint32_t const count0 = (trial % 2) ? rnd() % 50u : 0u;
		uint32_t const full = flower_gen_serial(c, tx, ty, xl, yl, xh, yh, w.data(), dn.data(), cl.data(), 0u, nullptr, nullptr, count0);
		uint32_t const capacity = (trial % 5 == 4 && full > 3) ? full - 3 : full + 2;
		std::vector<flower_pod_t> a((size_t)capacity + 1), b((size_t)capacity + 1);
		std::vector<uint32_t> ax((size_t)capacity + 1, 0xDEADBEEFu), bx((size_t)capacity + 1, 0xDEADBEEFu);
		memset(a.data(), 0xA5, a.size()*sizeof(flower_pod_t)); memset(b.data(), 0xA5, b.size()*sizeof(flower_pod_t));
		uint32_t const n1 = flower_gen_serial(c, tx, ty, xl, yl, xh, yh, w.data(), dn.data(), cl.data(), capacity, a.data(), ax.data(), count0);
		uint32_t const n2 = wave_place(c, tx, ty, xl, yl, xh, yh, w.data(), dn.data(), cl.data(), capacity, b.data(), bx.data(), count0, searched);
		CHECK(n1 == full && n2 == full, "trial %d: counts %u %u %u", trial, full, n1, n2);
		CHECK(memcmp(a.data(), b.data(), a.size()*sizeof(flower_pod_t)) == 0, "trial %d: the records differ (count %u, capacity %u)", trial, full, capacity);
		CHECK(ax == bx, "trial %d: the aux words differ", trial);
		total_flowers += full - count0; cut += full > capacity; ++trials;
	}
	CHECK(total_flowers > 20000u && searched > 20u && cut > 5u, "the trials are too thin: %u flowers, %u searched chunks, %u cut", total_flowers, searched, cut);
	printf("flowers_wave_check: %u trials, %u flowers, %u searched chunks, %u cut short: %s (%d problems)\n", trials, total_flowers, searched, cut, problems ? "FAILED" : "ok", problems);
	return problems ? 1 : 0;
}
