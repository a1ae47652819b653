// smap_casters_check.cpp -- the caster lists as k_smap_casters makes them (terra_kernels.hpp): one workgroup of 1024 lanes per render, a lane per tile, 1024 tiles a
// turn; per turn a ballot per list and wave, the two counts of a wave packed into one word, one prefix over the waves' words, and every lane with a flag stores its
// tile at (entries so far) + (its rank) -- written for the host over the same bodies (terra_smapview.hpp), against the literal loop (smap_casters_literal), on seeded
// random batches: dense and sparse lists, n not a multiple of 64 or of 1024, absent tiles, tiles fully in a city, tiles without deciduous trees, and receivers that
// are absent or out of range.  The plan's literal body (smap_plan_literal) runs on every batch, and the recompute queue's rank is held against std::sort on the
// reference's pair.  The arrays are sized exactly, so
// a read or a store outside them is an AddressSanitizer report.  A stand-alone program: built with -fsanitize=address,undefined and run by
// tests/test_smap_plan_emul.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>
#include "../3dworld_amd/csrc/terra_smapview.hpp"

using namespace terra;

static unsigned const THREADS = 1024, WAVES = THREADS/64;

// tp_block_rank2 for every lane of the workgroup at once: the ballots and the barriers are the host's loops, the packed word and the ranks are the kernel's own
// arithmetic (smap_rank2_word, smap_rank2 of terra_smapview.hpp)
static void block_rank2(std::vector<uint8_t> const &f0, std::vector<uint8_t> const &f1, std::vector<uint32_t> &r0, std::vector<uint32_t> &r1, uint32_t &n0, uint32_t &n1) {
	uint32_t s_wave[WAVES];
	unsigned long long m0[WAVES], m1[WAVES];
	for (unsigned w = 0; w < WAVES; ++w) { // __ballot
		m0[w] = m1[w] = 0ull;
		for (unsigned lane = 0; lane < 64; ++lane) {
			if (f0[w*64 + lane]) {m0[w] |= 1ull << lane;}
			if (f1[w*64 + lane]) {m1[w] |= 1ull << lane;}
		}
		s_wave[w] = smap_rank2_word(m0[w], m1[w]);
	}
	for (unsigned tid = 0; tid < THREADS; ++tid) {
		unsigned const lane = tid & 63u, w = tid >> 6;
		smap_rank2_t const q = smap_rank2(s_wave, WAVES, w, lane, m0[w], m1[w]);
		n0 = q.n0; n1 = q.n1; r0[tid] = q.r0; r1[tid] = q.r1;
	}
}

struct outputs_t {
	std::vector<uint32_t> to_draw, terrain, counts; std::vector<uint8_t> not_drawn, status;
	outputs_t(uint32_t n, uint32_t R) : to_draw((size_t)R*n, 0xABCDEF01u), terrain((size_t)R*n, 0xABCDEF01u), counts((size_t)R*2, 7u), not_drawn((size_t)R*n, 0x77), status(R, 0x77) {}
	bool operator==(outputs_t const &o) const {return to_draw == o.to_draw && terrain == o.terrain && counts == o.counts && not_drawn == o.not_drawn && status == o.status;}
};

// k_smap_casters for render r
static void render_workgroup(std::vector<smap_geom_t> const &geom, uint32_t n, uint32_t const *recv, view_pod_t const *views, float const *bsm, float const *lpos, int decid, int adj,
	outputs_t &o, uint32_t r)
{
	size_t const row = (size_t)r*n;
	view_pod_t const v = smap_cast_view(views[r]);
	smap_recv_t const rc = smap_recv(geom.data(), n, recv[r], lpos + 3u*r);
	uint32_t nd = 0, nt = 0;
	std::vector<uint8_t> f0(THREADS), f1(THREADS);
	std::vector<uint32_t> r0(THREADS), r1(THREADS);
	for (uint32_t base = 0; base < n; base += THREADS) {
		for (uint32_t tid = 0; tid < THREADS; ++tid) {
			uint32_t const t = base + tid;
			uint32_t const w = (t < n) ? smap_cast_tile(v, bsm[r], geom[t], rc, decid, adj) : 0u;
			if (t < n) {o.not_drawn[row + t] = (w & 1u) ? 0 : 1;}
			f0[tid] = (w & 1u) != 0u; f1[tid] = (w & 2u) != 0u;
		}
		uint32_t n0 = 0, n1 = 0;
		block_rank2(f0, f1, r0, r1, n0, n1);
		for (uint32_t tid = 0; tid < THREADS; ++tid) {
			if (f0[tid]) {o.to_draw.at(row + nd + r0[tid]) = base + tid;}
			if (f1[tid]) {o.terrain.at(row + nt + r1[tid]) = base + tid;}
		}
		nd += n0; nt += n1;
	}
	o.counts[2u*r] = nd; o.counts[2u*r + 1u] = nt; o.status[r] = rc.ok ? 0 : (uint8_t)SMC_NO_TILE;
}

int main() {
	int problems = 0;
	std::mt19937 rng(20240611u);
	auto uni = [&](float a, float b) {return std::uniform_real_distribution<float>(a, b)(rng);};
	uint32_t const sizes[] = {1, 63, 64, 65, 200, 1023, 1024, 1025, 1600, 2500};
	unsigned long renders = 0, listed = 0;
	for (uint32_t n : sizes) {
		for (int density = 0; density < 3; ++density) { // 0: sparse lists (narrow frusta), 1: mixed, 2: dense (invalid views: every tile is visible)
			uint32_t const side = (uint32_t)std::ceil(std::sqrt((double)n)), R = 9;
			std::vector<int32_t> txy((size_t)n*2);
			std::vector<terra_tile_stats> stats(n);
			std::vector<uint8_t> flags(n);
			std::vector<uint32_t> decid(n);
			std::vector<float> trmax(n);
			for (uint32_t t = 0; t < n; ++t) {
				txy[2*t] = (int32_t)(t % side) - (int32_t)side/2; txy[2*t + 1] = (int32_t)(t/side) - (int32_t)side/2;
				memset(&stats[t], 0, sizeof(stats[t]));
				stats[t].mzmin = uni(-7.0f, 0.0f); stats[t].mzmax = stats[t].mzmin + uni(0.0f, 3.0f); stats[t].radius = uni(5.0f, 7.0f);
				uint32_t const k = rng() % 16u;
				flags[t] = (uint8_t)((k == 0 ? TV_FLAG_ABSENT : 0) | (k == 1 || k == 2 ? TV_FLAG_FULLY_IN_CITY : 0));
				decid[t] = (rng() % 3u) ? rng() % 5u : 0u;
				trmax[t] = uni(0.0f, 0.5f);
			}
			view_pod_t none; memset(&none, 0, sizeof(none));
			float const b_ext[3] = {2.0f, 1.0f, 0.5f}, road_len[2] = {3.0f, 7.0f};
			smap_consts_t const c = smap_consts(none, 1.0f, 1, b_ext, road_len, 4.0f, 4.0f, 0.5f, 0.5f, 16, 1, -2, -5.9f);
			terrain_view_in_t const in = {stats.data(), nullptr, trmax.data(), nullptr, flags.data(), nullptr};
			for (int decid_only = 0; decid_only < 2; ++decid_only) {
				std::vector<smap_geom_t> geom(n);
				for (uint32_t t = 0; t < n; ++t) {geom[t] = smap_geom(c, in, decid.data(), decid_only, txy.data(), t);}
				std::vector<uint32_t> recv(R);
				std::vector<view_pod_t> views(R);
				std::vector<float> bsm(R), lpos((size_t)R*3);
				for (uint32_t r = 0; r < R; ++r) {
					recv[r] = (r == 3) ? n : ((r == 5) ? 0xFFFFFFFFu : rng() % n); // out of range twice
					float const lp[3] = {uni(-300.0f, 300.0f), uni(-300.0f, 300.0f), uni(20.0f, 300.0f)};
					for (int k = 0; k < 3; ++k) {lpos[3*r + k] = lp[k];}
					uint32_t const bt = rng() % n;
					float box[6] = {geom[bt].sb[0][0], geom[bt].sb[0][1], geom[bt].sb[1][0], geom[bt].sb[1][1], -1.0f, 2.0f};
					if (!(box[0] < box[1])) {box[0] = -4.0f; box[1] = 4.0f; box[2] = -4.0f; box[3] = 4.0f;} // (an absent tile's record is all zeros)
					if (!smap_light_view(lp, box, 0.01f, views[r], bsm[r])) {printf("no light view for render %u\n", r); ++problems; memset(&views[r], 0, sizeof(view_pod_t)); bsm[r] = 1.0f;}
					if (density == 2 || (density == 1 && (r & 1u))) {views[r].valid = 0;}
				}
				outputs_t lit(n, R), wg(n, R);
				smap_cast_io_t const io = {stats.data(), trmax.data(), nullptr, flags.data(), decid.data(), recv.data(), lit.to_draw.data(), lit.terrain.data(), lit.counts.data(),
				                           lit.not_drawn.data(), lit.status.data()};
				for (uint32_t r = 0; r < R; ++r) {
					smap_casters_literal(geom.data(), io, views.data(), bsm.data(), lpos.data(), n, decid_only, 1, r);
					render_workgroup(geom, n, recv.data(), views.data(), bsm.data(), lpos.data(), decid_only, 1, wg, r);
					++renders; listed += lit.counts[2*r];
				}
				if (!(lit == wg)) {printf("n %u density %d decid_only %d: the workgroup's lists differ from the literal loop's\n", n, density, decid_only); ++problems;}
				if (lit.status[3] != SMC_NO_TILE || lit.status[5] != SMC_NO_TILE || lit.counts[6] != 0u) {printf("n %u: an out-of-range receiver got a list\n", n); ++problems;}
			}
			// the plan's literal body on the same batch (smap_plan_literal: the loops in batch order, then every tile's place in the queue): its recomp_order against
			// std::sort on the reference's pair of the keys it left, consumed from the back; its receivers against its plan words
			{
				view_pod_t cam; float cbsm = 1.0f;
				float const cpos[3] = {0.3f, 0.2f, 0.5f}, cdir[3] = {1.0f, 0.0f, 0.0f}, cup[3] = {0.0f, 0.0f, 1.0f};
				if (!view_make(cpos, cdir, cup, 0.6f, 1.5f, 0.05f, 400.0f, cam)) {printf("no camera\n"); ++problems;}
				cam.valid = density ? 1 : 0;
				smap_plan_args_pod_t pa; memset(&pa, 0, sizeof(pa));
				pa.behind_sphere_mult = cbsm; pa.water_enabled = 1; pa.smap_thresh_scale = 3.0f; pa.shadow_map_sz = 4096u; pa.want_recomp = 1;
				pa.sun_pos[0] = 0.0f; pa.sun_pos[1] = 0.0f; pa.sun_pos[2] = 90.0f; // (over the batch's middle: ties between mirrored tiles of equal height)
				smap_consts_t const pc = smap_plan_consts(cam, pa, 4.0f, 4.0f, 0.5f, 0.5f, 16, 1, -2, -5.9f);
				std::vector<uint8_t> state(n, SMAP_NONE), tf(n, 0);
				std::vector<uint32_t> plan(n, 0xABCDEF01u), recvs(n, 0xABCDEF01u), cnt(2, 7u), ro(n, 0xABCDEF01u);
				std::vector<float> ds(n, -7.5f), sb((size_t)n*6, -7.5f);
				std::vector<smap_rank_key_t> pk(n);
				smap_plan_io_t const pio = {stats.data(), trmax.data(), nullptr, flags.data(), state.data(), plan.data(), ds.data(), sb.data(), recvs.data(), cnt.data(), tf.data(), ro.data()};
				smap_plan_literal(pc, in, pio, txy.data(), n, pk.data());
				typedef std::pair<float, std::pair<int32_t, int32_t> > pentry_t;
				std::vector<std::pair<pentry_t, uint32_t> > pq;
				uint32_t nrecv = 0;
				for (uint32_t t = 0; t < n; ++t) {
					if (pk[t].present) {pq.push_back(std::make_pair(pentry_t(pk[t].key, std::make_pair(txy[2*t + 1], txy[2*t])), t));}
					if (plan[t] & SMP_RECEIVER) {if (recvs.at(nrecv) != t) {printf("n %u: receivers differ at %u\n", n, nrecv); ++problems;} ++nrecv;}
				}
				std::sort(pq.begin(), pq.end());
				if (cnt[0] != nrecv || cnt[1] != pq.size()) {printf("n %u: the plan's counts %u %u != %u %zu\n", n, cnt[0], cnt[1], nrecv, pq.size()); ++problems;}
				for (size_t k = 0; k < pq.size(); ++k) {
					if (ro[k] != pq[pq.size() - 1 - k].second) {printf("n %u: the plan's recomp_order differs at %zu\n", n, k); ++problems; break;}
				}
				for (size_t k = pq.size(); k < n; ++k) {if (ro[k] != 0xABCDEF01u) {printf("n %u: recomp_order written past its count\n", n); ++problems; break;}}
			}
			// the recompute queue: the place by rank against std::sort on the reference's pair, consumed from the back
			std::vector<smap_rank_key_t> keys(n);
			typedef std::pair<float, std::pair<int32_t, int32_t> > entry_t; // (-dist, (y, x)): tile_xy_pair::operator< compares y, then x
			std::vector<std::pair<entry_t, uint32_t> > queue;
			for (uint32_t t = 0; t < n; ++t) {
				keys[t].key = -(float)(rng() % 7u); keys[t].y = txy[2*t + 1]; keys[t].x = txy[2*t]; keys[t].present = (flags[t] & TV_FLAG_ABSENT) ? 0u : 1u; // (many ties)
				if (keys[t].present) {queue.push_back(std::make_pair(entry_t(keys[t].key, std::make_pair(keys[t].y, keys[t].x)), t));}
			}
			std::sort(queue.begin(), queue.end());
			std::vector<uint32_t> order(queue.size(), 0xFFFFFFFFu);
			for (uint32_t t = 0; t < n; ++t) {if (keys[t].present) {order.at(smap_recomp_place(keys.data(), n, t)) = t;}}
			for (size_t k = 0; k < queue.size(); ++k) {
				if (order[k] != queue[queue.size() - 1 - k].second) {printf("n %u: recomp_order differs at %zu\n", n, k); ++problems; break;}
			}
		}
	}
	if (listed < renders) {printf("the batches list too little: %lu entries in %lu renders\n", listed, renders); ++problems;}
	printf("%lu renders, %lu listed tiles: %s (%d problems)\n", renders, listed, problems ? "FAILED" : "ok", problems);
	return problems ? 1 : 0;
}
