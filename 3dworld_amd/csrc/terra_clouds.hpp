// terra_clouds.hpp -- the clouds of a tile batch: tile_cloud_manager_t (src/tiled_mesh.cpp:1710-1820, src/tiled_mesh.h:116-153) as tile_t::update_tile_clouds
// (:1822-1827) and tile_draw_t::draw_tile_clouds (:3484-3508) drive it, with tile_cloud_t::draw's decision and alpha (:1691-1697), gen_gauss_rand_arr
// (src/gen_object.cpp:363-374), rand_gaussian / rand_uniform / gen_rand_cube_point (src/rand_gen.h:91-95, src/gen_object.cpp:464-468), cube_t's set_to_zeros /
// is_all_zeros / union_with_cube / expand_by (src/3DWorld.h:436,491,506,621), p2p_dist_sq (src/inlines.h:176-178) and get_tile_width (src/tiled_mesh.h:93).
//
// The bodies are shared by the driver's simple form (the reference's loops, literal, over the batch in order), by the k_cloud_* kernels (terra_kernels.hpp) and
// by tests/clouds_replay_check.cpp.  Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is
// written out; the library is built without contraction.
//
// The generator: a manager's rand_gen_t is seeded with two ints (x1 + 123, y1 + 321), so every value it takes fits 32 bits (tree_rgen_t, terra_treeplace.hpp); the
// state keeps it in 64 bits each, as the reference does.
//
// The wind step of a batch, and where its order dependence lies (cloud_path, cloud_update_tile, cloud_update_batch_split):
//   A record that exists when the call begins is moved by the tile that holds it, handed to a neighbour when it leaves that tile's range, moved again by that
//   neighbour if its turn is still to come, and so on.  Which tiles it visits depends on the record, on those tiles' ranges, on their `generated` bits before the
//   call and on the batch order -- not on any other record.  Records made in the call (generation, repopulation) are not moved in it.  So cloud_path follows every
//   record on its own and marks the tile it leaves and the tile it is handed to: the marked tiles are all that can send or receive in this call (a record that a full
//   list drops would have gone on: the marks are a superset; a later tile that drops a record because it has not generated yet is marked too, so that it does not
//   generate before the sender's turn).  An unmarked tile's step reads and writes nothing but the tile itself: those run in parallel.  The
//   marked tiles are replayed in batch order by the literal loop, which hands records only to marked tiles.
#pragma once
#include "terra_view.hpp"
#include "terra_treeplace.hpp"
#include "terra_stage.hpp"
#include "../../include/terra.h" // terra_tile_stats
#include <stdexcept>

namespace terra {

constexpr int      CLOUD_GAUSS_DIST = 10000, CLOUD_GAUSS_N = 10; // N_RAND_DIST (src/rand_gen.h:10), N_RAND_GAUSS (src/3DWorld.h:102)
constexpr int      CLOUD_GAUSS_SIZE = CLOUD_GAUSS_DIST + 2;
constexpr uint32_t CLD_OVERFLOW = 1u; // terra_cloud_tile.flags: a push_back met a full list
enum {CLV_NONE = 0, CLV_VFC = 1, CLV_BELOW_ZMIN = 2, CLV_BELOW_WATER = 3, CLV_BELOW_MESH = 4, CLV_LISTED = 5}; // the stage byte of the view

struct cloud_params_pod_t {float clouds_per_tile, cloud_height_offset; int32_t rgen_seed;};                           // terra_cloud_params
struct cloud_step_pod_t {float wind[3], fticks; int32_t animate;};                                                    // terra_cloud_step
struct cloud_pod_t {float pos_hash, pos[3], size[3]; uint32_t pad;};                                                   // terra_cloud
struct cloud_tile_pod_t {uint32_t generated, flags, count, num_clouds; float cur_move_dist; uint32_t pad; int64_t rseed1, rseed2; float bcube[6], range[6];}; // terra_cloud_tile
struct cloud_view_args_pod_t {float behind_sphere_mult, xlate[3], max_dist;};                                          // terra_cloud_view_args
struct cloud_inst_pod_t {uint32_t tile, slot; float dist_sq, alpha, draw_alpha; uint32_t drawn;};                      // terra_cloud_inst

// gen_gauss_rand_arr()
inline void cloud_gauss_table(int32_t rgen_seed, float *out) {
	float const RG_NORM = (float)sqrt(3.0/(double)CLOUD_GAUSS_N), mconst = (float)(2.0E-4*(double)RG_NORM), aconst = ((float)CLOUD_GAUSS_N)*RG_NORM;
	rand_gen_t rgen;
	rgen.set_state(rgen_seed, 123);
	for (int i = 0; i < CLOUD_GAUSS_SIZE; ++i) {
		float val = 0.0f;
		for (int j = 0; j < CLOUD_GAUSS_N; ++j) {val += (float)(rgen.rand()%10000);}
		out[i] = mconst*val - aconst;
	}
}

struct cloud_consts_t {
	float const *gauss;         // gauss_rand_arr
	float clouds_per_tile;
	float xss, yss, DX_VAL, DY_VAL;
	float z1, z2;               // the z interval of a range made in this call (:1727-1728)
	int S;
	uint32_t capacity;
	int animate, moving;        // animate2; wind != zero_vector
	int edge[2];                // the dxy[d] of :1775
	float move[3], move_mag;    // move_amt, move_amt.mag() (:1761-1762)
	double two_widths;          // 2.0*get_tile_width()
};
inline cloud_consts_t cloud_consts(cloud_params_pod_t const &p, cloud_step_pod_t const &s, float const *gauss, float xss, float yss, float DX_VAL, float DY_VAL, int S,
	float zmin, float zmax, uint32_t capacity)
{
	cloud_consts_t c;
	c.gauss = gauss; c.clouds_per_tile = p.clouds_per_tile; c.xss = xss; c.yss = yss; c.DX_VAL = DX_VAL; c.DY_VAL = DY_VAL; c.S = S; c.capacity = capacity;
	float const z_range = zmax - zmin, z_cloud_bot = (float)((double)(zmax + p.cloud_height_offset*z_range) + 2.0);
	c.z1 = (float)((double)z_cloud_bot + 0.0*(double)z_range); c.z2 = (float)((double)z_cloud_bot + 0.9*(double)z_range);
	c.animate = s.animate ? 1 : 0;
	c.moving = (s.wind[0] == 0.0f && s.wind[1] == 0.0f && s.wind[2] == 0.0f) ? 0 : 1;
	for (int d = 0; d < 2; ++d) {c.edge[d] = ((double)s.wind[d] < 0.0) ? 1 : (((double)s.wind[d] > 0.0) ? -1 : 0);}
	double const m = 0.01*(double)s.fticks;
	c.move[0] = (float)(m*(double)s.wind[0]); c.move[1] = (float)(m*(double)s.wind[1]); c.move[2] = (float)(m*(double)0.0f);
	c.move_mag = sqrtf(c.move[0]*c.move[0] + c.move[1]*c.move[1] + c.move[2]*c.move[2]);
	c.two_widths = 2.0*(double)(xss + yss);
	return c;
}

TERRA_HD tree_rgen_t cloud_rgen(cloud_tile_pod_t const &st) {tree_rgen_t r; r.set_state((int32_t)st.rseed1, (int32_t)st.rseed2); return r;}
TERRA_HD void cloud_rgen_store(cloud_tile_pod_t &st, tree_rgen_t const &r) {st.rseed1 = r.rseed1; st.rseed2 = r.rseed2;}

// update_bcube (:1753-1756) with tile_cloud_t::get_bcube
TERRA_HD void cloud_update_bcube(cloud_tile_pod_t &st, cloud_pod_t const &c) {
	float *b = st.bcube;
	bool const zeros = box_all_zeros(b);
	for (int i = 0; i < 3; ++i) {
		float const lo = c.pos[i] - c.size[i], hi = c.pos[i] + c.size[i];
		if (zeros) {b[2*i] = lo; b[2*i+1] = hi;} else {b[2*i] = min_std(b[2*i], lo); b[2*i+1] = max_std(b[2*i+1], hi);}
	}
}
// push_back + update_bcube: a list that holds `capacity` records takes no more, and says so
TERRA_HD void cloud_push(cloud_consts_t const &c, cloud_tile_pod_t &st, cloud_pod_t *recs, cloud_pod_t const &r) {
	if (st.count < c.capacity) {recs[st.count++] = r;} else {st.flags |= CLD_OVERFLOW;}
	cloud_update_bcube(st, r);
}
// choose_num_clouds (:1733-1735)
TERRA_HD uint32_t cloud_choose_num(cloud_consts_t const &c, tree_rgen_t &rg) {
	if (c.clouds_per_tile == 0.0f) return 0u;
	float const g = c.gauss[rg.rand()%CLOUD_GAUSS_DIST];
	return (uint32_t)max_std(0.0f, c.clouds_per_tile + 4.0f*g);
}
// gen_new_cloud (:1710-1720): the generator chain of one cloud.  g++ evaluates the three arguments of vector3d(...) from the right: size.z is drawn first
TERRA_HD cloud_pod_t cloud_gen_one(float const range[6], tree_rgen_t &rg) {
	cloud_pod_t r;
	for (int i = 0; i < 3; ++i) {r.pos[i] = rg.rand_uniform(range[2*i], range[2*i+1]);}
	r.size[2] = rg.rand_uniform(0.6f, 1.0f); r.size[1] = rg.rand_uniform(1.0f, 2.0f); r.size[0] = rg.rand_uniform(1.0f, 2.0f);
	float const m = rg.rand_uniform(2.0f, 4.0f);
	for (int i = 0; i < 3; ++i) {r.size[i] *= m;}
	r.pos_hash = r.pos[0]; r.pad = 0u;
	return r;
}
// populate_clouds (:1737-1743)
TERRA_HD void cloud_populate(cloud_consts_t const &c, cloud_tile_pod_t &st, cloud_pod_t *recs, tree_rgen_t &rg) {
	for (int i = 0; i < 6; ++i) {st.bcube[i] = 0.0f;}
	for (uint32_t k = 0; k < st.num_clouds; ++k) {cloud_push(c, st, recs, cloud_gen_one(st.range, rg));}
}
// gen (:1722-1731)
TERRA_HD void cloud_gen(cloud_consts_t const &c, cloud_tile_pod_t &st, cloud_pod_t *recs, int tx, int ty) {
	if (st.generated) return;
	st.generated = 1u;
	int const x1 = (int)((uint32_t)tx*(uint32_t)c.S), y1 = (int)((uint32_t)ty*(uint32_t)c.S), x2 = (int)((uint32_t)x1 + (uint32_t)c.S), y2 = (int)((uint32_t)y1 + (uint32_t)c.S);
	tree_rgen_t rg;
	rg.set_state((int32_t)((uint32_t)x1 + 123u), (int32_t)((uint32_t)y1 + 321u));
	st.range[0] = -c.xss + c.DX_VAL*(float)x1; st.range[1] = -c.xss + c.DX_VAL*(float)x2; st.range[2] = -c.yss + c.DY_VAL*(float)y1; st.range[3] = -c.yss + c.DY_VAL*(float)y2;
	st.range[4] = c.z1; st.range[5] = c.z2;
	st.num_clouds = cloud_choose_num(c, rg);
	cloud_populate(c, st, recs, rg);
	cloud_rgen_store(st, rg);
}
// one cloud's wind step and classification (:1786-1791): bit 0..1 of the result: dx + 1, bit 2..3: dy + 1 (5: it stays)
TERRA_HD uint32_t cloud_step(cloud_consts_t const &c, float const range[6], float ws_mult, cloud_pod_t &r) {
	float const wscale = 1.5f - ws_mult*(r.pos[2] - range[4]);
	for (int i = 0; i < 3; ++i) {r.pos[i] += wscale*c.move[i];}
	r.pos_hash = (float)((double)r.pos_hash + 0.15*(double)c.move_mag);
	uint32_t const dx = (r.pos[0] < range[0]) ? 0u : ((r.pos[0] > range[1]) ? 2u : 1u), dy = (r.pos[1] < range[2]) ? 0u : ((r.pos[1] > range[3]) ? 2u : 1u);
	return dx | (dy << 2);
}
TERRA_HD float cloud_ws_mult(float const range[6]) {return (float)(0.5/(double)(range[5] - range[4]));}
TERRA_HD uint32_t cloud_nbr_slot(uint32_t code) {return (code >> 2)*3u + (code & 3u);} // -> the [n][9] neighbour table's (dy + 1)*3 + dx + 1

// does the tile run the loop of :1785 in this call, given the list it has at its turn
TERRA_HD bool cloud_tile_active(cloud_consts_t const &c, cloud_tile_pod_t const &st) {return c.animate && c.moving && st.generated;}

// move_by_wind (:1758-1797) of one tile, literal; hand(u, record) is adj->add_cloud for the tile u of the batch
template<class HAND> TERRA_HD void cloud_move_tile(cloud_consts_t const &c, cloud_tile_pod_t &st, cloud_pod_t *recs, int32_t const *nbr9, HAND hand) {
	if (!st.generated || !c.moving) return;
	st.cur_move_dist += c.move_mag;
	tree_rgen_t rg = cloud_rgen(st);
	if ((double)st.cur_move_dist > c.two_widths) {
		st.num_clouds = cloud_choose_num(c, rg);
		st.cur_move_dist = 0.0f;
		cloud_rgen_store(st, rg);
	}
	if (st.count == 0u && st.num_clouds > 0u) {
		bool on_edge = false;
		for (uint32_t d = 0; d < 2 && !on_edge; ++d) {
			int const dx = (d == 0) ? c.edge[0] : 0, dy = (d == 1) ? c.edge[1] : 0;
			if (nbr9[(dy + 1)*3 + dx + 1] < 0) {on_edge = true;}
		}
		if (on_edge) {cloud_populate(c, st, recs, rg); cloud_rgen_store(st, rg);}
		return;
	}
	if (st.count == 0u) return;
	float const ws_mult = cloud_ws_mult(st.range);
	for (int i = 0; i < 6; ++i) {st.bcube[i] = 0.0f;}
	st.count = remove_elements_serial(st.count, [&](uint32_t i) {
		uint32_t const code = cloud_step(c, st.range, ws_mult, recs[i]);
		if (code == 5u) {cloud_update_bcube(st, recs[i]); return false;}
		int32_t const u = nbr9[cloud_nbr_slot(code)];
		if (u >= 0) {hand((uint32_t)u, recs[i]);}
		return true;
	}, [&](uint32_t dst, uint32_t src) {recs[dst] = recs[src];});
}
// update_tile_clouds (:1822-1827) of tile t of the batch
TERRA_HD void cloud_update_tile(cloud_consts_t const &c, int32_t const *tile_xy, int32_t const *nbr, cloud_tile_pod_t *state, cloud_pod_t *clouds, uint32_t t) {
	cloud_pod_t *recs = clouds + (size_t)t*c.capacity;
	if (c.animate) {
		cloud_move_tile(c, state[t], recs, nbr + (size_t)t*9, [&](uint32_t u, cloud_pod_t const &r) {
			if (state[u].generated) {cloud_push(c, state[u], clouds + (size_t)u*c.capacity, r);} // try_add_cloud (:1745-1751)
		});
	}
	cloud_gen(c, state[t], recs, tile_xy[2*t], tile_xy[2*t+1]);
}
// ---- the arrays of an update call, in the order of terra_tiles_update_clouds[_dev]: host pointers in the host form's first record, device pointers everywhere else
struct cloud_update_io_t {cloud_tile_pod_t *state; cloud_pod_t *clouds; uint32_t *total;};
// the argument rules of a call, behind cloud_update_check: throws what the call refuses; false: n == 0, nothing to do but total = 0 (the caller's).  dev: the arrays are the device's
inline bool cloud_update_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, cloud_update_io_t const &io, bool dev) {
	if (dev && (((uintptr_t)io.state & 7u) != 0 || ((((uintptr_t)io.clouds | (uintptr_t)io.total)) & 3u) != 0)) throw std::invalid_argument(
		"tiles_update_clouds: d_state must be 8-byte aligned, d_clouds and d_total 4-byte aligned");
	if (n == 0) return false;
	if (!tile_xy || !io.state || (capacity && !io.clouds)) throw std::invalid_argument("tiles_update_clouds: null argument");
	return true;
}
// scratch: the coordinates, the neighbour table; for the kernels the marks of cloud_path and the marked tiles in batch order
struct cloud_update_scratch_t {int32_t *txy, *nbr; uint32_t *marks, *order;};
inline void cloud_update_scratch_add(stage_layout_t &lay, cloud_update_scratch_t &s, uint32_t n) {lay.add(s.txy, (size_t)n*2); lay.add(s.nbr, (size_t)n*9); lay.add(s.marks, ((size_t)n + 3)/4); lay.add(s.order, n);}
// the literal body of the simple form: one thread, the reference's loop over the batch in order
TERRA_HD void cloud_update_literal(cloud_consts_t const &c, cloud_update_io_t const &io, cloud_update_scratch_t const &s, uint32_t n) {
	uint32_t num = 0;
	for (uint32_t t = 0; t < n; ++t) {cloud_update_tile(c, s.txy, s.nbr, io.state, io.clouds, t); num += io.state[t].count;}
	if (io.total) {*io.total = num;}
}
// the path of record i of tile t through this call: mark(u) for the tile it leaves and the tile that takes it.  Every hop but the last goes to a later tile
TERRA_HD void cloud_path(cloud_consts_t const &c, int32_t const *nbr, cloud_tile_pod_t const *state, cloud_pod_t r, uint32_t t, uint32_t n, uint8_t *touched) {
	uint32_t cur = t;
	for (uint32_t hop = 0; hop < n; ++hop) {
		float const *range = state[cur].range;
		uint32_t const code = cloud_step(c, range, cloud_ws_mult(range), r);
		if (code == 5u) return;
		touched[cur] = 1;
		int32_t const u = nbr[(size_t)cur*9 + cloud_nbr_slot(code)];
		if (u < 0) return;                       // no such tile: dropped
		if ((uint32_t)u < cur) {touched[u] = 1; return;} // an earlier tile has generated by now and takes it; its turn is over
		touched[u] = 1;
		if (!state[u].generated) return;         // a later tile that has not generated drops it (marked: it must not generate before the sender's turn)
		cur = (uint32_t)u;
	}
}
// all paths of tile t's records
TERRA_HD void cloud_mark_tile(cloud_consts_t const &c, int32_t const *nbr, cloud_tile_pod_t const *state, cloud_pod_t const *clouds, uint32_t t, uint32_t n, uint8_t *touched) {
	if (!cloud_tile_active(c, state[t])) return;
	uint32_t const cnt = (state[t].count < c.capacity) ? state[t].count : c.capacity;
	for (uint32_t i = 0; i < cnt; ++i) {cloud_path(c, nbr, state, clouds[(size_t)t*c.capacity + i], t, n, touched);}
}
// the step of a tile without traffic: nothing leaves it and nothing reaches it
TERRA_HD void cloud_update_tile_alone(cloud_consts_t const &c, int32_t const *tile_xy, int32_t const *nbr, cloud_tile_pod_t *state, cloud_pod_t *clouds, uint32_t t) {
	cloud_tile_pod_t st = state[t];
	cloud_pod_t *recs = clouds + (size_t)t*c.capacity;
	if (c.animate) {cloud_move_tile(c, st, recs, nbr + (size_t)t*9, [](uint32_t, cloud_pod_t const &) {});}
	cloud_gen(c, st, recs, tile_xy[2*t], tile_xy[2*t+1]);
	state[t] = st;
}

// ---- the view: get_draw_list (:1799-1820) of one record and tile_cloud_t::draw's decision (:1693-1696)
struct cloud_view_consts_t {
	view_pod_t v;
	float behind_sphere_mult, xlate[3], max_dist, water_plane_z;
	uint32_t capacity;
};
// -> the stage byte; `o` is written where it is CLV_LISTED.  exact(x, y) is get_exact_zval(x, y, 1), called only for the records that reach :1813
template<class EXACT> TERRA_HD uint32_t cloud_view_record(cloud_view_consts_t const &c, cloud_pod_t const &r, float mzmin, float mzmax, EXACT exact, cloud_inst_pod_t &o) {
	float const px = r.pos[0] + c.xlate[0], py = r.pos[1] + c.xlate[1], pz = r.pos[2] + c.xlate[2];
	float const rmax = max_std(r.size[0], max_std(r.size[1], r.size[2]));
	if (!view_sphere_visible(c.v, c.behind_sphere_mult, px, py, pz, rmax)) return CLV_VFC;
	float const zbot = r.pos[2] - r.size[2];
	if (zbot < mzmin) return CLV_BELOW_ZMIN;
	if ((double)zbot + 0.2*(double)r.size[2] < (double)c.water_plane_z) return CLV_BELOW_WATER;
	float const start_dist = (float)(1.0*(double)r.size[2]);
	float alpha = 1.0f;
	if (zbot < mzmax + start_dist) {
		float const dist = zbot - exact(r.pos[0], r.pos[1]);
		if (dist < 0.0f) return CLV_BELOW_MESH;
		if (dist < start_dist) {alpha = dist/start_dist;}
	}
	float const dx = c.v.pos[0] - px, dy = c.v.pos[1] - py, dz = c.v.pos[2] - pz;
	float const dsq = dx*dx + dy*dy + dz*dz; // p2p_dist_sq(get_camera_pos(), pt); view_dir.mag() of :1694 is the root of the same sum
	float const view_dist = sqrtf(dsq);
	o.dist_sq = -dsq; o.alpha = alpha;
	o.drawn = (view_dist >= c.max_dist) ? 0u : 1u;
	if (o.drawn) {
		float const val = (float)(1.0 - (double)((c.max_dist - view_dist)/c.max_dist));
		o.draw_alpha = alpha*(1.0f - val*val);
	}
	else {o.draw_alpha = 0.0f;}
	return CLV_LISTED;
}
// the order of the list: ascending in (dist_sq, tile, slot), dist_sq compared as floats compare
TERRA_HD bool cloud_inst_before(cloud_inst_pod_t const &a, cloud_inst_pod_t const &b) {
	if (a.dist_sq < b.dist_sq) return true;
	if (b.dist_sq < a.dist_sq) return false;
	return a.tile < b.tile || (a.tile == b.tile && a.slot < b.slot);
}

// ---- the arrays of a view call, in the order of terra_tiles_cloud_view[_dev]
struct cloud_view_io_t {terra_tile_stats const *stats; cloud_tile_pod_t const *state; cloud_pod_t const *clouds; uint8_t *stage; cloud_inst_pod_t *list; uint32_t *list_count;};
// the argument rules of a call, behind cloud_view_check: throws what the call refuses; false: n == 0, nothing to do but list_count = 0 (the caller's).  dev: the arrays are the device's
inline bool cloud_view_io_check(int32_t const *tile_xy, uint32_t n, uint32_t capacity, cloud_view_io_t const &io, bool dev) {
	if (dev && (((uintptr_t)io.state & 7u) != 0 || ((((uintptr_t)io.stats | (uintptr_t)io.clouds | (uintptr_t)io.list | (uintptr_t)io.list_count)) & 3u) != 0)) throw std::invalid_argument(
		"tiles_cloud_view: d_state must be 8-byte aligned, d_stats, d_clouds, d_list and d_list_count 4-byte aligned");
	if (n == 0) return false;
	size_t const nrec = (size_t)n*capacity;
	if (!tile_xy || !io.stats || !io.state || !io.list_count || (nrec && (!io.clouds || !io.stage || !io.list))) throw std::invalid_argument("tiles_cloud_view: null argument");
	if (nrec > 0x7FFFFFFFu) throw std::invalid_argument("tiles_cloud_view: n*capacity must be below 2^31");
	return true;
}
// scratch: get_exact_zval's constants (read from memory), the instances by slot and then in the order they were listed, their number
struct cloud_view_scratch_t {tree_place_consts_t *tc; cloud_inst_pod_t *by_slot, *found; uint32_t *cnt;};
inline void cloud_view_scratch_add(stage_layout_t &lay, cloud_view_scratch_t &s, size_t nrec) {lay.add(s.tc, 1); lay.add(s.by_slot, nrec); lay.add(s.found, nrec); lay.add(s.cnt, 4);}
// the literal bodies of the simple form.  (1) a logical thread per record slot: get_draw_list's decision
TERRA_HD void cloud_view_slot_literal(cloud_view_consts_t const &c, cloud_view_io_t const &io, cloud_view_scratch_t const &s, size_t i) {
	uint32_t const t = (uint32_t)(i/c.capacity), k = (uint32_t)(i%c.capacity);
	uint32_t stg = CLV_NONE;
	if (k < io.state[t].count) {
		cloud_inst_pod_t o; o.tile = t; o.slot = k;
		stg = cloud_view_record(c, io.clouds[i], io.stats[t].mzmin, io.stats[t].mzmax, [&](float x, float y) {return tree_exact_zval(*s.tc, x, y);}, o);
		if (stg == CLV_LISTED) {s.by_slot[i] = o;}
	}
	io.stage[i] = (uint8_t)stg;
}
// (2) one thread: to_draw_clouds as the loop of :3491 fills it, in batch order
TERRA_HD void cloud_view_found_literal(cloud_view_io_t const &io, cloud_view_scratch_t const &s, size_t nrec) {
	uint32_t cnt = 0;
	for (size_t i = 0; i < nrec; ++i) {if (io.stage[i] == CLV_LISTED) {s.found[cnt++] = s.by_slot[i];}}
	*s.cnt = cnt; *io.list_count = cnt;
}
// (3) a logical thread per record slot: the sort of :3493 -- an entry's place is its rank
TERRA_HD void cloud_view_rank_literal(cloud_view_io_t const &io, cloud_view_scratch_t const &s, size_t i) {
	uint32_t const cnt = *s.cnt;
	if (i >= cnt) return;
	cloud_inst_pod_t const me = s.found[i];
	uint32_t rank = 0;
	for (uint32_t j = 0; j < cnt; ++j) {rank += cloud_inst_before(s.found[j], me) ? 1u : 0u;}
	io.list[rank] = me;
}

} // namespace terra
