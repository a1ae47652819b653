// line_trees_check.cpp -- the shared bodies of terra_linetrees.hpp on the host, as a stand-alone program built with -fsanitize=address,undefined and run by
// tests/test_line_trees_emul.py:
//  1. line_trunc_cone over the rows of tests/golden/line_trees_vectors.npz (the test hands them over as a raw file: int32 n, n x 14 floats, n int32 t_set, n floats
//     t): t_set and the bits of t as the reference's own compiled line_intersect_trunc_cone returned them;
//  2. the order-free form k_line_intersect_trees takes -- every record against the line on its own with *t = 1.0, then the minimum of (t, record*2 + part) -- against
//     the literal loop of small_tree_group::line_intersect (line_trees_tile_literal) on seeded random tiles: dense rows of pines that one line crosses, ties between
//     identical records, palms and bushes between them, dropped records, counts above the capacity.  The arrays are sized exactly, so a read outside them is an
//     AddressSanitizer report.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../3dworld_amd/csrc/terra_linetrees.hpp"

using namespace terra;

static int problems = 0;

static void fixture_rows(char const *path) {
	FILE *f = fopen(path, "rb");
	if (!f) {printf("cannot open %s\n", path); ++problems; return;}
	int32_t n = 0;
	if (fread(&n, 4, 1, f) != 1 || n <= 0) {printf("bad row file\n"); ++problems; fclose(f); return;}
	std::vector<float> rows((size_t)n*14), t((size_t)n);
	std::vector<int32_t> t_set((size_t)n);
	bool const ok = fread(rows.data(), 4, rows.size(), f) == rows.size() && fread(t_set.data(), 4, t_set.size(), f) == t_set.size() && fread(t.data(), 4, t.size(), f) == t.size();
	fclose(f);
	if (!ok) {printf("short row file\n"); ++problems; return;}
	int bad = 0;
	for (int32_t i = 0; i < n; ++i) {
		float const *r = rows.data() + (size_t)14*i;
		float tv = 0.0f;
		int const s = line_trunc_cone(r, r + 3, r + 6, r + 9, r[12], r[13], tv);
		if (s != t_set[i] || (s && memcmp(&tv, &t[i], 4) != 0)) {
			if (bad++ < 5) {printf("row %d: t_set %d t %.9g, the reference %d %.9g\n", i, s, tv, t_set[i], t[i]);}
		}
	}
	printf("%d fixture rows, %d differ\n", n, bad);
	problems += bad;
}

static void wave_form(unsigned seed, uint32_t cap, uint32_t count, bool instanced) {
	std::mt19937 rng(seed);
	auto uni = [&](float a, float b) {return std::uniform_real_distribution<float>(a, b)(rng);};
	line_trees_consts_t c;
	memset(&c, 0, sizeof(c));
	c.cap = cap;
	c.pv.a.hs = 1.0f; c.pv.a.pine_radius_scale = 1.0f; c.pv.a.tree_scale = 1.0f; c.pv.a.tsize = 0.8f; c.pv.a.offx = 1.5f; c.pv.a.offy = -2.5f;
	c.pv.a.instanced = instanced ? 1 : 0; c.pv.a.num_insts = instanced ? 4u : 0u;
	c.pv.tree_depth = 0.1f; c.pv.cap = cap;
	std::vector<tree_inst_pod_t> insts = {{T_PINE, 0.6f, 0.2f}, {T_PALM, 0.8f, 0.2f}, {T_SH_PINE, 0.5f, 0.25f}, {7, 0.5f, 0.2f}};
	std::vector<tree_place_pod_t> recs(cap);
	uint32_t const live = count < cap ? count : cap;
	for (uint32_t j = 0; j < cap; ++j) {
		tree_place_pod_t r;
		memset(&r, 0, sizeof(r));
		bool const row = (j % 3) != 2; // two of three stand in a row along x, some of them twice at one place
		r.pos[0] = row ? 0.25f*(float)((j/2) % 40) : uni(-5.0f, 5.0f); r.pos[1] = row ? 0.0f : uni(-0.3f, 0.3f); r.pos[2] = 0.0f;
		int const types[8] = {T_PINE, T_PINE, T_SH_PINE, T_PINE, T_PALM, T_BUSH, 9, T_PINE};
		r.type = types[rng() % 8]; r.inst = instanced ? (int32_t)(rng() % 6) - 1 : ((rng() % 16 == 0) ? 3 : -1);
		r.height = uni(0.3f, 0.7f); r.width = (rng() % 12 == 0) ? -0.1f : uni(0.1f, 0.25f);
		recs[j] = r;
	}
	std::vector<uint32_t> counts = {count};
	line_trees_in_t in;
	in.pine = recs.data(); in.counts = counts.data(); in.ov = nullptr; in.insts = insts.data();
	line_tree_box_t const box = line_trees_box(c, in, 0);
	int hits = 0;
	for (int k = 0; k < 200; ++k) {
		shadow_pt_t v1, v2;
		if (k % 2) {v1 = {-3.0f + c.pv.a.offx, uni(-0.02f, 0.02f) + c.pv.a.offy, uni(0.05f, 0.5f)}; v2 = {13.0f + c.pv.a.offx, uni(-0.02f, 0.02f) + c.pv.a.offy, uni(0.05f, 0.5f)};}
		else {v1 = {uni(-6.0f, 6.0f), uni(-6.0f, 2.0f), uni(0.0f, 1.0f)}; v2 = {uni(-6.0f, 12.0f), uni(-6.0f, 2.0f), uni(-0.2f, 0.8f)};}
		if (k % 7 == 0) {shadow_pt_t const s = v1; v1 = v2; v2 = s;}
		float t = 1.0f; int32_t tree = -1; uint32_t part = 0;
		bool const want = line_trees_tile_literal(c, in, 0, box, v1, v2, t, tree, part);
		// the kernel's form
		float p1[3], p2[3];
		line_trees_local(c, v1, p1); line_trees_local(c, v2, p2);
		unsigned long long best = ~0ull;
		float bt = 0.0f;
		if (box.nvalid && line_trees_gate(box, p1, p2)) {
			for (uint32_t j0 = 0; j0 < live; j0 += 64) {
				for (uint32_t lane = 0; lane < 64; ++lane) {
					uint32_t const jj = j0 + lane;
					float tl; uint32_t pl;
					if (!(jj < live && line_trees_test(c, in, 0, jj, p1, p2, tl, pl))) continue;
					uint32_t tb; memcpy(&tb, &tl, 4);
					if (tb == 0x80000000u) {tb = 0u;}
					unsigned long long const key = ((unsigned long long)tb << 32) | (jj*2u + pl);
					if (key < best) {best = key; bt = tl;}
				}
			}
		}
		bool const got = best != ~0ull;
		if (got != want || (got && (memcmp(&bt, &t, 4) != 0 || (int32_t)((uint32_t)best >> 1) != tree || ((uint32_t)best & 1u) != part))) {
			if (problems++ < 5) {printf("seed %u line %d: wave form %d t %.9g rec %u, literal %d t %.9g rec %d part %u\n", seed, k, (int)got, bt, (uint32_t)best, (int)want, t, tree, part);}
		}
		hits += want ? 1 : 0;
	}
	printf("seed %u cap %u count %u: %u valid records, %d of 200 lines hit\n", seed, cap, count, box.nvalid, hits);
	if (box.nvalid >= 30 && hits < 20) {printf("too few hits to mean anything\n"); ++problems;}
}

int main(int argc, char **argv) {
	if (argc > 1) {fixture_rows(argv[1]);}
	uint32_t const counts[] = {0, 1, 63, 64, 65, 130, 200};
	unsigned seed = 1;
	for (uint32_t cnt : counts) {
		wave_form(seed++, cnt > 130 ? 130u : (cnt ? cnt : 1u), cnt, false);
		wave_form(seed++, cnt > 130 ? 130u : (cnt ? cnt : 1u), cnt, true);
	}
	printf("ok (%d problems)\n", problems);
	return problems ? 1 : 0;
}
