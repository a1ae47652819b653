// collide_wave_check.cpp -- the sphere queries as k_sphere_collide runs them (terra_kernels.hpp): a wave of 64 lanes per query, per container a prologue sweep
// reduced over the lanes, then rounds of 64 records against the current centre, the lowest hit of the ballot applied and the walk resumed behind it -- written for the
// host over the same bodies (terra_collide.hpp), against the literal loops (coll_query_literal), on seeded random tiles with dense overlaps (most queries have
// several hits) and on inputs out of range: query tiles outside [-1, n), tree_id / inst / kind outside their tables, counts above the capacity, bad queries.  The
// arrays are sized exactly, so a read outside them is an AddressSanitizer report.  A stand-alone program: built with -fsanitize=address,undefined and run by
// tests/test_collide_emul.py.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../3dworld_amd/csrc/terra_collide.hpp"

using namespace terra;

struct lanes_pt {coll_pt_t m[64]; bool hit[64];};

// coll_wave_chain: test(j, m) -> whether record j moves the centre m
template<class TEST> static uint32_t wave_chain(uint32_t cnt, coll_pt_t &c, unsigned long &rounds, TEST test) {
	uint32_t nhits = 0;
	for (uint32_t start = 0; start < cnt;) {
		lanes_pt L;
		unsigned long long mask = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) { // every lane sees the same centre
			uint32_t const j = start + lane;
			L.m[lane] = c;
			L.hit[lane] = j < cnt && test(j, L.m[lane]);
			if (L.hit[lane]) {mask |= 1ull << lane;}
		}
		++rounds;
		if (mask == 0ull) {start += 64u; continue;}
		int const l = __builtin_ctzll(mask);
		c = L.m[l];
		++nhits; start += (uint32_t)l + 1u;
	}
	return nhits;
}
// the xor butterfly of the kernel's reductions over 64 per-lane values
template<class T, class MERGE> static T butterfly(std::vector<T> v, MERGE merge) {
	for (int off = 32; off; off >>= 1) {
		std::vector<T> const o = v;
		for (int lane = 0; lane < 64; ++lane) {merge(v[lane], o[lane ^ off]);}
	}
	return v[0];
}
struct pine_box_t {float box[6]; uint32_t nv, nb;};

static coll_result_t query_wave(collide_consts_t const &c, collide_in_t const &in, uint32_t t, float const pos[3], float radius, uint32_t flags, unsigned long &rounds) {
	coll_result_t o; o.c.x = pos[0]; o.c.y = pos[1]; o.c.z = pos[2]; o.word = 0u; o.nhits = 0u;
	float const INF = __builtin_inff();
	uint32_t const np = (flags & COLL_INC_PTREES) ? coll_pine_count(c, in, t) : 0u;
	if (np != 0u) {
		std::vector<pine_box_t> per(64);
		for (uint32_t lane = 0; lane < 64; ++lane) {
			pine_box_t &p = per[lane];
			for (int k = 0; k < 6; k += 2) {p.box[k] = INF; p.box[k + 1] = -INF;}
			p.nv = p.nb = 0;
			for (uint32_t j = lane; j < np; j += 64u) {
				tree_view_rec_t rec;
				if (!coll_pine_rec(c, in, t, j, rec)) continue;
				++p.nv;
				float d[6];
				if (!tree_view_bounds(rec, d)) continue;
				++p.nb;
				for (int k = 0; k < 6; k += 2) {p.box[k] = min_std(p.box[k], d[k]); p.box[k + 1] = max_std(p.box[k + 1], d[k + 1]);}
			}
		}
		pine_box_t all = butterfly(per, [](pine_box_t &a, pine_box_t const &b) {
			a.nv += b.nv; a.nb += b.nb;
			for (int k = 0; k < 6; k += 2) {a.box[k] = min_std(a.box[k], b.box[k]); a.box[k + 1] = max_std(a.box[k + 1], b.box[k + 1]);}
		});
		if (all.nv != 0u) {
			if (all.nb == 0u) {for (int k = 0; k < 6; ++k) {all.box[k] = 0.0f;}}
			o.c.x -= c.pv.a.offx; o.c.y -= c.pv.a.offy; o.c.z -= 0.0f;
			if (!coll_gate_exits(o.c, radius, all.box)) {
				uint32_t const nh = wave_chain(np, o.c, rounds, [&](uint32_t j, coll_pt_t &m) {
					tree_view_rec_t rec;
					return coll_pine_rec(c, in, t, j, rec) && coll_small_tree(rec, m, radius);
				});
				if (nh) {o.word |= COLL_HIT_PINE; o.nhits += nh;}
			}
			o.c.x += c.pv.a.offx; o.c.y += c.pv.a.offy; o.c.z += 0.0f;
		}
	}
	uint32_t const nd = (flags & COLL_INC_DTREES) ? coll_decid_count(c, in, t) : 0u;
	if (nd != 0u) {
		struct du_t {decid_view_union_t un; uint32_t nv;};
		std::vector<du_t> per(64);
		for (uint32_t lane = 0; lane < 64; ++lane) {
			decid_view_union_init(per[lane].un); per[lane].nv = 0;
			for (uint32_t j = lane; j < nd; j += 64u) {
				decid_place_pod_t r;
				if (!coll_decid_rec(c, in, t, j, r)) continue;
				++per[lane].nv;
				float b[6], l[6];
				decid_view_bounds(in.data[r.tree_id], r.pos, b, l);
				decid_view_union_add(per[lane].un, j, b, l);
			}
		}
		du_t const all = butterfly(per, [](du_t &a, du_t const &b) {decid_view_union_merge(a.un, b.un); a.nv += b.nv;});
		if (all.nv != 0u) {
			float bc[6];
			decid_view_union_result(all.un, bc);
			o.c.x -= c.doffx; o.c.y -= c.doffy; o.c.z -= 0.0f;
			if (!coll_gate_exits(o.c, radius, bc)) {
				uint32_t const nh = wave_chain(nd, o.c, rounds, [&](uint32_t j, coll_pt_t &m) {
					decid_place_pod_t r;
					return coll_decid_rec(c, in, t, j, r) && coll_decid_tree(in.data[r.tree_id], in.br_scale ? in.br_scale[r.tree_id] : 1.0f, r.pos, m, radius);
				});
				if (nh) {o.word |= COLL_HIT_DECID; o.nhits += nh;}
			}
			o.c.x += c.doffx; o.c.y += c.doffy; o.c.z += 0.0f;
		}
	}
	if ((flags & COLL_INC_SCENERY) && coll_scenery_generated(in, t)) {
		uint32_t const ns = coll_scen_count(c, in, t);
		size_t const base = (size_t)t*c.scen_cap;
		uint32_t present = 0;
		for (uint32_t j = 0; j < ns; ++j) {
			int const kind = in.scen[base + j].kind;
			if (kind >= 0 && kind < SCENERY_KINDS) {present |= 1u << kind;}
			if (kind == SCENERY_ROCK_SHAPE && !((in.rov ? in.rov[base + j] : 0.0f) > 0.0f)) {present |= 0x80000000u;}
		}
		if (present & 0x80000000u) {o.word |= COLL_ROCK_SHAPE_UNDECIDED;}
		o.c.x -= c.soffx; o.c.y -= c.soffy; o.c.z -= 0.0f;
		for (int k = 0; k < COLL_SCENERY_PASSES; ++k) {
			int const kind = coll_scenery_pass_kind(k);
			if (!((present >> kind) & 1u)) continue;
			uint32_t const nh = wave_chain(ns, o.c, rounds, [&](uint32_t j, coll_pt_t &m) {
				if (in.scen[base + j].kind != kind) return false;
				bool und = false;
				return coll_scenery(in.scen[base + j], in.rov ? in.rov[base + j] : 0.0f, m, radius, und);
			});
			if (nh) {o.word |= COLL_HIT_SCENERY; o.nhits += nh;}
		}
		o.c.x += c.soffx; o.c.y += c.soffy; o.c.z += 0.0f;
	}
	return o;
}

int main() {
	std::mt19937 rng(4711);
	auto uni = [&](float a, float b) {return std::uniform_real_distribution<float>(a, b)(rng);};
	auto pick = [&](uint32_t k) {return (uint32_t)(rng()%k);};
	int problems = 0;
	unsigned long queries = 0, tested = 0, multi = 0, hits = 0, rounds = 0, bad = 0, no_tile = 0;
	for (int trial = 0; trial < 120 && problems < 5; ++trial) {
		int const S = 16;
		uint32_t const n = 1 + pick(4), pcap = (trial % 4 == 0) ? 7u : 60u + pick(90), dcap = (trial % 5 == 0) ? 64u : 30u + pick(100), scap = 20u + pick(120), ndata = 8, ninst = 6;
		std::vector<int32_t> txy;
		for (uint32_t t = 0; t < n; ++t) {txy.push_back((int)t%2 - 1); txy.push_back((int)t/2 - 1);}
		// the key table, as the driver builds it
		uint32_t hbits = 4;
		while ((1ull << hbits) < 2ull*n) {++hbits;}
		std::vector<int32_t> slots((size_t)1 << hbits, -1);
		for (uint32_t t = 0; t < n; ++t) {
			uint32_t h = batch_key_hash(batch_key(txy[2*t], txy[2*t + 1]), hbits);
			while (slots[h] >= 0) {h = (h + 1) & (((uint32_t)1 << hbits) - 1);}
			slots[h] = (int32_t)t;
		}
		std::vector<terra_tile_stats> stats(n);
		for (auto &s : stats) {memset(&s, 0, sizeof(s)); s.mzmin = 0.0f; s.mzmax = 0.5f; s.radius = 5.7f;}
		std::vector<uint8_t> flags(n, 0);
		if (n > 2) {flags[2] = (uint8_t)(1u + pick(2));}
		std::vector<tree_place_pod_t> pine((size_t)n*pcap);
		std::vector<trunk_override_pod_t> ov((size_t)n*pcap);
		std::vector<decid_place_pod_t> decid((size_t)n*dcap);
		std::vector<scenery_place_pod_t> scen((size_t)n*scap);
		std::vector<float> rov((size_t)n*scap, 0.0f), br(ndata);
		std::vector<uint32_t> pc(n), dc(n), sc(n);
		std::vector<tree_inst_pod_t> insts(ninst);
		std::vector<decid_tree_data_pod_t> data(ndata);
		for (uint32_t i = 0; i < ninst; ++i) {insts[i].type = (i % 3 == 2) ? T_PALM : T_PINE; insts[i].height = uni(8.0f, 14.0f); insts[i].width = uni(2.0f, 4.0f);}
		for (uint32_t i = 0; i < ndata; ++i) {
			decid_tree_data_pod_t &d = data[i];
			memset(&d, 0, sizeof(d));
			float const s = uni(0.7f, 1.4f);
			d.base_radius = 0.03f*s; d.sphere_radius = 0.3f*s; d.sphere_center_zoff = 0.375f*s; d.lr_z_cent = 0.4f*s;
			float const lb[6] = {-0.3f, 0.3f, -0.3f, 0.3f, 0.125f, 0.75f}, bb[6] = {-0.2f, 0.2f, -0.2f, 0.2f, 0.0f, 0.625f};
			for (int k = 0; k < 6; ++k) {d.leaves_bcube[k] = s*lb[k]; d.branches_bcube[k] = s*bb[k];}
			d.flags = (i == 5) ? 0u : (uint32_t)DCV_GENERATED;
			if (i == 6) {for (int k = 0; k < 6; ++k) {d.leaves_bcube[k] = d.branches_bcube[k] = 0.0f;}} // boxes of all zeros
			br[i] = uni(0.8f, 1.3f);
		}
		int const dxoff = (int)pick(41) - 20, dyoff = (int)pick(41) - 20;
		float const dxv = 0.5f;
		for (uint32_t t = 0; t < n; ++t) {
			float const ox = 8.0f*(float)txy[2*t] - 4.0f + dxv*(float)dxoff + 3.0f, oy = 8.0f*(float)txy[2*t + 1] - 4.0f + dxv*(float)dyoff + 3.0f; // a 1.5 x 1.5 patch: dense
			pc[t] = (trial % 6 == 1) ? pcap + 9u : pick(pcap + 1); dc[t] = (trial % 6 == 2) ? 0xFFFFFFF0u : pick(dcap + 1); sc[t] = (trial % 6 == 3) ? scap + 1u : pick(scap + 1);
			for (uint32_t j = 0; j < pcap; ++j) {
				tree_place_pod_t &r = pine[(size_t)t*pcap + j];
				memset(&r, 0, sizeof(r));
				r.pos[0] = ox + uni(0.0f, 1.5f); r.pos[1] = oy + uni(0.0f, 1.5f); r.pos[2] = uni(0.0f, 0.2f);
				uint32_t const w = pick(20);
				r.type = (w == 0) ? 9 : (w == 1) ? -3 : (int)(pick(6)); r.inst = (w == 2) ? 5000 : (w == 3) ? (int)pick(ninst) : (w == 4) ? (int)0x7FFFFFFF : -1;
				r.height = uni(0.03f, 0.6f); r.width = uni(0.1f, 0.25f);
				trunk_override_pod_t &o = ov[(size_t)t*pcap + j];
				memset(&o, 0, sizeof(o));
				if (pick(10) == 0) {o.rotated = 1; o.p1[0] = r.pos[0] + uni(-0.05f, 0.05f); o.p1[1] = r.pos[1]; o.p1[2] = -0.1f; o.p2[0] = o.p1[0] + 0.3f; o.p2[1] = o.p1[1]; o.p2[2] = 0.7f; o.r1 = 0.03f; o.r2 = 0.01f;}
			}
			for (uint32_t j = 0; j < dcap; ++j) {
				decid_place_pod_t &r = decid[(size_t)t*dcap + j];
				memset(&r, 0, sizeof(r));
				r.pos[0] = ox + uni(0.0f, 1.5f); r.pos[1] = oy + uni(0.0f, 1.5f); r.pos[2] = uni(0.0f, 0.1f);
				uint32_t const w = pick(16);
				r.tree_id = (w == 0) ? 99 : (w == 1) ? -4 : (w == 2) ? (int)ndata : (w == 3) ? (int)0x7FFFFFFF : (w == 4) ? (int)0x80000000u : (int)pick(ndata);
			}
			for (uint32_t j = 0; j < scap; ++j) {
				scenery_place_pod_t &r = scen[(size_t)t*scap + j];
				memset(&r, 0, sizeof(r));
				r.pos[0] = ox + uni(0.0f, 1.5f); r.pos[1] = oy + uni(0.0f, 1.5f); r.pos[2] = uni(0.0f, 0.3f);
				uint32_t const w = pick(24);
				r.kind = (w == 0) ? 17 : (w == 1) ? -1 : (w == 2) ? (int)0x7FFFFFFF : (int)pick(9);
				r.radius = (r.kind == SCENERY_STUMP || r.kind == SCENERY_PLANT) ? uni(0.02f, 0.05f) : uni(0.04f, 0.12f);
				r.p[0] = (r.kind == SCENERY_PLANT) ? uni(0.2f, 0.4f) : r.radius; r.p[1] = uni(0.1f, 0.4f);
				if (r.kind == SCENERY_ROCK_SHAPE) {r.radius = 0.0f; if (pick(2)) {rov[(size_t)t*scap + j] = uni(0.05f, 0.12f);}}
				if (r.kind == SCENERY_VOXEL_ROCK && pick(2)) {rov[(size_t)t*scap + j] = uni(0.05f, 0.12f);}
			}
		}
		tree_ao_consts_t ac;
		memset(&ac, 0, sizeof(ac));
		ac.hs = 1.0f; ac.pine_radius_scale = 1.0f; ac.tree_scale = 1.0f; ac.tsize = 16.0f*0.05f/1.0f; ac.dxv = dxv; ac.dyv = dxv;
		int const px2 = (int)pick(21) - 10, dx2 = (int)pick(21) - 10, sx2 = (int)pick(21) - 10;
		ac.offx = (float)(dxoff + px2)*dxv; ac.offy = (float)(dyoff - px2)*dxv; ac.S = S; ac.instanced = trial & 1; ac.num_insts = ninst; ac.pine_cap = pcap; ac.src_cap = pcap;
		view_pod_t v; memset(&v, 0, sizeof(v));
		tree_view_args_pod_t const ta = {0.0f, 1.0f, 1.0f, 1, 0, 0, 0, 0};
		collide_consts_t c;
		memset(&c, 0, sizeof(c));
		c.pv = tree_view_consts(v, ta, ac, 4.0f, 4.0f, dxoff, dyoff, pcap);
		c.doffx = (float)(dxoff + dx2)*dxv; c.doffy = (float)(dyoff - dx2)*dxv; c.soffx = (float)(dxoff + sx2)*dxv; c.soffy = (float)(dyoff - sx2)*dxv;
		c.lookup_ox = (float)dxoff*dxv; c.lookup_oy = (float)dyoff*dxv;
		c.n = n; c.hbits = hbits; c.num_data = ndata; c.pine_cap = pcap; c.decid_cap = dcap; c.scen_cap = scap;
		// the records are authored in camera space: take each container's translation off
		for (auto &r : pine) {r.pos[0] -= c.pv.a.offx; r.pos[1] -= c.pv.a.offy;}
		for (auto &o : ov) {o.p1[0] -= c.pv.a.offx; o.p1[1] -= c.pv.a.offy; o.p2[0] -= c.pv.a.offx; o.p2[1] -= c.pv.a.offy;}
		for (auto &r : decid) {r.pos[0] -= c.doffx; r.pos[1] -= c.doffy;}
		for (auto &r : scen) {r.pos[0] -= c.soffx; r.pos[1] -= c.soffy;}
		collide_in_t in;
		memset(&in, 0, sizeof(in));
		in.stats = stats.data(); in.flags = (trial % 3 == 0) ? nullptr : flags.data();
		in.pine = pine.data(); in.pine_counts = pc.data(); in.ov = (trial % 2) ? ov.data() : nullptr;
		in.decid = decid.data(); in.decid_counts = dc.data(); in.scen = scen.data(); in.scen_counts = sc.data(); in.rov = (trial % 7 == 0) ? nullptr : rov.data();
		in.insts = ac.instanced ? insts.data() : nullptr; in.data = data.data(); in.br_scale = br.data(); in.tile_xy = txy.data(); in.slots = slots.data();
		for (int qi = 0; qi < 60; ++qi) {
			uint32_t const t = pick(n);
			sphere_query_pod_t q;
			q.pos[0] = 8.0f*(float)txy[2*t] - 4.0f + dxv*(float)dxoff + 3.0f + uni(-0.1f, 1.6f); q.pos[1] = 8.0f*(float)txy[2*t + 1] - 4.0f + dxv*(float)dyoff + 3.0f + uni(-0.1f, 1.6f);
			q.pos[2] = uni(0.05f, 0.45f); q.radius = uni(0.05f, 0.3f);
			uint32_t const w = pick(30);
			q.tile = (w < 10) ? (int32_t)t : (w == 10) ? (int32_t)n : (w == 11) ? -2 : (w == 12) ? (int32_t)0x7FFFFFFF : (w == 13) ? (int32_t)0x80000000u : -1;
			q.flags = (w % 5 == 4) ? pick(8) : 7u;
			if (w == 14) {q.pos[pick(3)] = __builtin_nanf("");}
			if (w == 15) {q.radius = (pick(2)) ? -1.0f : __builtin_inff();}
			if (w == 16) {q.pos[0] = 3.0e38f;}
			sphere_hit_pod_t const a = coll_query(c, in, q, [&](uint32_t tt) {return coll_query_literal(c, in, tt, q.pos, q.radius, q.flags);});
			sphere_hit_pod_t const b = coll_query(c, in, q, [&](uint32_t tt) {return query_wave(c, in, tt, q.pos, q.radius, q.flags, rounds);});
			++queries;
			uint32_t const stage = (a.word & COLL_STAGE_MASK) >> COLL_STAGE_SHIFT;
			tested += stage == COLL_STAGE_TESTED; bad += stage == COLL_STAGE_BAD_QUERY; no_tile += stage == COLL_STAGE_NO_TILE;
			multi += a.nhits > 1; hits += a.nhits;
			if (memcmp(&a, &b, sizeof(a)) != 0) {
				printf("trial %d query %d: the wave form differs from the literal loop: (%g %g %g) word %x nhits %u  vs  (%g %g %g) word %x nhits %u\n", trial, qi, a.pos[0], a.pos[1], a.pos[2],
					a.word, a.nhits, b.pos[0], b.pos[1], b.pos[2], b.word, b.nhits);
				++problems;
			}
			if (stage != COLL_STAGE_TESTED && (memcmp(a.pos, q.pos, 12) != 0 || a.nhits != 0)) {printf("trial %d query %d: a query that left early was changed\n", trial, qi); ++problems;}
			// the cube call's bodies on the same data: the literal form reads nothing out of range either
			float const cube[6] = {q.pos[0] - 0.05f, q.pos[0] + 0.05f, q.pos[1] - 0.05f, q.pos[1] + 0.05f, q.pos[2], q.pos[2] + 0.1f};
			if (coll_cube_ok(cube)) {
				int32_t const ct = coll_cube_tile(c, in, q.tile, cube);
				if (ct >= 0) {(void)coll_cube_literal(c, in, (uint32_t)ct, cube);}
			}
		}
	}
	printf("%lu queries: %lu tested, %lu bad, %lu without a tile; %lu hits, %lu queries with several; %lu rounds\n", queries, tested, bad, no_tile, hits, multi, rounds);
	if (multi*2 < tested || bad == 0 || no_tile == 0) {printf("the queries are not what the check is for\n"); ++problems;}
	printf("ok (%d problems)\n", problems);
	return problems ? 1 : 0;
}
