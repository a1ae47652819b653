// clouds_replay_check.cpp -- the clouds' update as the kernels split it (k_cloud_mark, k_cloud_tiles, k_cloud_tail; terra_kernels.hpp), compiled for the host from the
// same bodies (terra_clouds.hpp), against the literal loop over the batch in order, on randomised traffic: batches with holes in shuffled order, tiles that are not
// generated, emptied lists, clouds on both sides of every edge, winds with zero components, small capacities.  A stand-alone program: built with
// -fsanitize=address,undefined and run by tests/test_clouds_emul.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>
#include "../3dworld_amd/csrc/terra_clouds.hpp"

using namespace terra;

struct batch_t {
	std::vector<int32_t> txy, nbr;
	std::vector<cloud_tile_pod_t> state;
	std::vector<cloud_pod_t> clouds;
	uint32_t n = 0, cap = 0;
};

static void literal(cloud_consts_t const &c, batch_t &b) {
	for (uint32_t t = 0; t < b.n; ++t) {cloud_update_tile(c, b.txy.data(), b.nbr.data(), b.state.data(), b.clouds.data(), t);}
}
// what the three launches do, in an order of the tiles within a launch that a GPU may pick: descending
static uint32_t split(cloud_consts_t const &c, batch_t &b) {
	std::vector<uint8_t> touched(b.n + 4, 0);
	for (uint32_t t = b.n; t-- > 0;) {cloud_mark_tile(c, b.nbr.data(), b.state.data(), b.clouds.data(), t, b.n, touched.data());}
	for (uint32_t t = b.n; t-- > 0;) {if (!touched[t]) {cloud_update_tile_alone(c, b.txy.data(), b.nbr.data(), b.state.data(), b.clouds.data(), t);}}
	uint32_t nt = 0;
	for (uint32_t t = 0; t < b.n; ++t) {if (touched[t]) {cloud_update_tile(c, b.txy.data(), b.nbr.data(), b.state.data(), b.clouds.data(), t); ++nt;}}
	return nt;
}

int main() {
	std::mt19937 rng(12345);
	auto uni = [&](float a, float b) {return std::uniform_real_distribution<float>(a, b)(rng);};
	auto pick = [&](uint32_t k) {return (uint32_t)(rng()%k);};
	std::vector<float> gauss(CLOUD_GAUSS_SIZE);
	cloud_gauss_table(1, gauss.data());
	int problems = 0;
	unsigned long replayed = 0, tiles = 0, handed = 0;
	for (int trial = 0; trial < 400 && problems < 5; ++trial) {
		int const S = (trial & 1) ? 128 : 16, w = 1 + (int)pick(5), h = 1 + (int)pick(5), ox = (int)pick(9) - 4, oy = (int)pick(9) - 4;
		batch_t b;
		b.cap = (trial % 5 == 0) ? 3u : 32u;
		std::vector<std::pair<int, int>> xy;
		for (int y = 0; y < h; ++y) {for (int x = 0; x < w; ++x) {if (w*h < 4 || pick(6) != 0) {xy.push_back({ox + x, oy + y});}}}
		if (xy.empty()) {xy.push_back({ox, oy});}
		if (trial % 3 != 0) {std::shuffle(xy.begin(), xy.end(), rng);}
		b.n = (uint32_t)xy.size();
		std::map<std::pair<int, int>, int> index;
		for (uint32_t t = 0; t < b.n; ++t) {b.txy.push_back(xy[t].first); b.txy.push_back(xy[t].second); index[xy[t]] = (int)t;}
		b.nbr.assign((size_t)b.n*9, -1);
		for (uint32_t t = 0; t < b.n; ++t) {
			for (int k = 0; k < 9; ++k) {auto it = index.find({xy[t].first + k%3 - 1, xy[t].second + k/3 - 1}); if (it != index.end()) {b.nbr[(size_t)t*9 + k] = it->second;}}
		}
		b.state.assign(b.n, cloud_tile_pod_t());
		for (auto &s : b.state) {memset(&s, 0, sizeof(s));}
		b.clouds.assign((size_t)b.n*b.cap, cloud_pod_t());
		for (auto &r : b.clouds) {memset(&r, 0, sizeof(r));}
		cloud_params_pod_t const p = {(trial % 7 == 0) ? 0.0f : uni(0.5f, 6.0f), 0.0f, 1};
		float const width = 2.0f*4.0f; // a tile's width at scene size 4
		for (int frame = 0; frame < 5; ++frame) {
			cloud_step_pod_t s;
			float const mx = (pick(5) == 0) ? 0.0f : uni(-0.6f, 0.6f), my = (pick(5) == 0) ? 0.0f : uni(-0.6f, 0.6f);
			s.wind[0] = mx*width*100.0f; s.wind[1] = my*width*100.0f; s.wind[2] = (pick(4) == 0) ? 0.5f : 0.0f; s.fticks = 1.0f; s.animate = (pick(10) != 0) ? 1 : 0;
			cloud_consts_t const c = cloud_consts(p, s, gauss.data(), 4.0f, 4.0f, 2.0f*4.0f/(float)S, 2.0f*4.0f/(float)S, S, -7.0f, 7.0f, b.cap);
			// what an engine may do between frames: a tile enters anew; a list is empty; clouds stand at an edge
			for (uint32_t t = 0; t < b.n && frame > 0; ++t) {
				cloud_tile_pod_t &st = b.state[t];
				uint32_t const what = pick(8);
				if (what == 0) {memset(&st, 0, sizeof(st));}
				else if (what == 1 && st.generated) {st.count = 0; st.num_clouds = pick(4);}
				else if (what == 2 && st.generated) {
					for (uint32_t i = 0; i < st.count; ++i) {
						cloud_pod_t &r = b.clouds[(size_t)t*b.cap + i];
						if (pick(2)) {r.pos[0] = pick(2) ? st.range[0] + 0.01f*width : st.range[1] - 0.01f*width;}
						if (pick(2)) {r.pos[1] = pick(2) ? st.range[2] + 0.01f*width : st.range[3] - 0.01f*width;}
					}
				}
			}
			batch_t a = b;
			literal(c, a);
			replayed += split(c, b); tiles += b.n;
			for (uint32_t t = 0; t < b.n; ++t) {
				bool bad = memcmp(&a.state[t], &b.state[t], sizeof(cloud_tile_pod_t)) != 0;
				for (uint32_t i = 0; !bad && i < a.state[t].count; ++i) {bad = memcmp(&a.clouds[(size_t)t*b.cap + i], &b.clouds[(size_t)t*b.cap + i], sizeof(cloud_pod_t)) != 0;}
				if (a.state[t].count > b.cap) {bad = true;}
				if (bad) {printf("trial %d frame %d tile %u (%d, %d): the split form differs from the literal loop\n", trial, frame, t, xy[t].first, xy[t].second); ++problems;}
			}
			uint32_t sum = 0;
			for (auto const &st : a.state) {sum += st.count;}
			handed += sum;
			b = a; // (the records behind the counts may differ: go on from the literal loop's)
		}
	}
	printf("%lu of %lu tile steps replayed in order, %lu records carried\n", replayed, tiles, handed);
	if (replayed == 0 || replayed == tiles) {printf("the traffic is not mixed\n"); ++problems;}
	printf("ok (%d problems)\n", problems);
	return problems ? 1 : 0;
}
