// terra_kernels.hpp -- hand-written gfx950 kernels for the hot loops (device only; included by terra_hip.hip).
//
//   k_sine_grid     K1+K4: z = sum_k X[x][k]*Y[y][k] as an LDS-tiled rank-90 outer-product contraction + fused
//                   shape/glaciate/island epilogue (mesh_xy_grid_cache_t::eval_index, src/mesh_gen.cpp:766-790)
//   k_sine_grid_rs  the same for the heightmap's hot case (plain-only, rows of whole 16-byte groups): row operands from scalar loads, only the columns in LDS
//   k_noise_grid    K2/K3: per-cell simplex/Perlin fBm and domain warp (get_noise_zval, src/mesh_gen.cpp:734-751)
//   k_tile_erosion  K5 (tile mode): one wave per tile, the clamp-padded 138x138 grid resident in LDS, droplets in serial order
//   k_voxel_sines   K8: rank-60 3-D sine field, z-fastest output (noise_gen_3d::get_val, src/upsurface.cpp:60-70)
//
// No MFMA: the sums must round exactly like the CPU's mul-then-add chain (an MFMA/fma chain rounds once per term).
// Wave = 64 lanes; block sizes are multiples of 64; LDS tiles are read with 16-byte ds_read_b128 and broadcast.
#pragma once
#include "terra_driver.hpp"
#include "terra_noise_kernels.hpp"

namespace terra {

typedef float    st_f4 __attribute__((ext_vector_type(4))); // native vector types: what the nontemporal load / store builtins take
typedef uint32_t st_u4 __attribute__((ext_vector_type(4)));

template<class F> __global__ void k_generic(size_t n, F f) {
	size_t const i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i < n) {f(i);}
}

// one 64-lane workgroup (= one wave) per item, with the per-wave LDS scratch of the droplet window (terra_erosion.hpp)
template<class F> __global__ __launch_bounds__(64) void k_waves(F f, unsigned first) {
	__builtin_amdgcn_s_setprio(3); // (see k_waves_lean)
	__shared__ __attribute__((aligned(16))) float win[EW*EW];
	__shared__ uint8_t dirty[EW*EW];
	__shared__ wave_shared_t sh;
	wave_scratch_t const ws{win, dirty, &sh};
	f((size_t)blockIdx.x + first, ws);
}

template<class F> __global__ __launch_bounds__(64) void k_waves_nolds(F f) {f((size_t)blockIdx.x);}

// the same for the lean traces of the sparse erosion scheduler (terra_erosion.hpp: lean_back_t): window + dirty bytes + 4.6 KB of footprint bookkeeping = 9.8 KB of LDS, and
// at most 128 registers (four waves per SIMD requested) -- beside a k_sine_grid_rs block of another heightmap (29.7 KB, 84 registers per wave, allocated as 88) a SIMD has room for four of
// that kernel's waves and one of these (beside the 8 x 8 form's 106 registers: three and one), and a CU for four of its blocks and four of these; the general trace wave (22.7 KB, 260
// registers) leaves room for two and two
template<class F> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_waves_lean(F f) {
	__builtin_amdgcn_s_setprio(3); // a droplet is a chain of dependent instructions: beside three waves of another kernel on its SIMD it should never wait for an issue slot (it asks for one every ~5 cycles)
	__shared__ __attribute__((aligned(16))) float win[EW*EW];
	__shared__ uint8_t dirty[EW*EW];
	__shared__ lean_shared_t sh;
	lean_scratch_t const ws{win, dirty, &sh};
	f((size_t)blockIdx.x, ws);
}


// ------------------------------------------------------------------ K1: sine-sum grid
// z[y][x] = sum_k X[k][x]*Y[k][y] is a rank-(90-kstart) outer-product contraction.  It is fp32-VALU bound: every term costs one
// v_mul and one v_add (no FMA: the CPU reference rounds the product before adding), i.e. 2*terms VALU ops for 4 B written.
// (The heightmap's hot case -- plain-only, row length a multiple of 4, KC = 27 -- runs on k_sine_grid_rs below since profiles/r11_sine_rowscalar_ab.txt; this kernel keeps the
// tile batches, the general epilogue, the other row lengths and the chunk lengths 20 / 45.)
// Tiling: 128 x 128 cells per 256-thread block, 8 x 8 cells per thread (64 independent accumulator chains), the K range staged
// through LDS in chunks of <= KC terms (template parameter; at 27: three chunks for 8 octaves, 29.7 KB per block,
// 106 VGPRs -> 4 blocks = 16 waves per CU alone, and two waves per SIMD beside a 264-register droplet wave of another map's erosion;
// the plain tile variant -- 118 VGPRs -- uses 27 as well, the general one keeps SG_KC = 45: two chunks, 48 KB), operands of the next step prefetched from LDS while this one is multiplied.
// What is not the sum is kept short (profiles/r09_sine_overhead_ab.txt: 5976 -> 5718 vector instructions per wave, 5120 of them the sum; 4 % fewer cycles, which the
// power-limited clock turns into time on some machines only): a chunk goes from the tables to LDS by direct-to-LDS loads of whole row pairs (no register, no test per row: the tables have a zero row behind the last
// term, terra_common.hpp), a block inside the grid runs its 16 groups of four cells in a straight line with the island terms waiting in LDS, and row lengths that are no
// multiple of 4 have an instantiation of their own.
// Per k a thread issues four ds_read_b128 (conflict-free / broadcast) for 64 mul + 64 add.  The f32 matrix instructions cannot take the
// products: exact with K = 1, C = 0, but they share the packed-f32 datapath (profiles/r04_sine_matrix_pipe.txt).
constexpr int SG_BX = 128, SG_BY = 128, SG_TX = 8, SG_TY = 8, SG_THREADS = 256, SG_KC = 45; // 16 x 16 threads
// XCD-aware tile order: the dispatcher places block b on XCD b % 8 (observed, speed only); give every XCD one contiguous
// band of tile rows so its private L2 keeps that band's Y tiles, and walk the band in groups of `rowgroup` tile rows
// (an X slice is reused by `rowgroup` consecutive blocks before the walk moves to the next tile column).
__device__ __forceinline__ bool sg_tile_of_block(unsigned b, unsigned ntx, unsigned nty, unsigned rowgroup, unsigned &bx, unsigned &by) {
	unsigned const nb = ntx*nty, per_xcd = (nb + 7)/8;
	unsigned const lin = (b & 7)*per_xcd + (b >> 3); // position in the global tile order
	if (lin >= nb) return false;
	unsigned const group = lin/(rowgroup*ntx), r = lin % (rowgroup*ntx);
	unsigned const rows_here = (nty - group*rowgroup < rowgroup) ? nty - group*rowgroup : rowgroup;
	bx = r/rows_here; by = group*rowgroup + r % rows_here;
	return bx < ntx;
}

struct sg_tiles_t {int32_t const *tile_map; float const *m0; uint32_t nux; uint32_t rowgroup; uint32_t tw; // tw: cells per tile edge of the virtual grid (130 zvals, 201 AO context)
	// a BAND of the tiles' fields (round 6: the AO context without the centre nobody reads): tw x twy virtual cells per tile, written into the tile's ostride x ostride field at
	// (c + (c >= split ? gap : 0)) -- the square case: twy = ostride = tw, splits at 0xFFFFFFFF.  Only the packed epilogue of the plain kernel knows about it (the launcher checks).
	uint32_t twy, ostride, xsplit, xgap, ysplit, ygap;};

typedef float sg_v2f __attribute__((ext_vector_type(2)));
// Two rows x eight columns per call: r0[jp] += {x0*y0, x1*y0}, r1[jp] += {x0*y1, x1*y1} with (y0,y1) = one register pair straight from ds_read_b128.
// v_pk_mul_f32 broadcasts the row's y from either half of the pair through op_sel, so no operand is ever copied (the compiler's own selection
// moves half of the broadcast operands into fresh registers every step), and the mul/mul/add/add order keeps one independent instruction
// between each product and the add that consumes it (no hazard nops).  Product rounded by v_pk_mul, then added by v_pk_add: never fused.
__device__ __forceinline__ void sg_mul_add_2x8(sg_v2f (&r0)[SG_TX/2], sg_v2f (&r1)[SG_TX/2], sg_v2f const (&xp)[4], sg_v2f yp) {
	sg_v2f t0, t1;
#define TERRA_SG_2X2(A0, A1, X) \
	"v_pk_mul_f32 %8, " X ", %13 op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %9, " X ", %13 op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " A0 ", " A0 ", %8\n\t" \
	"v_pk_add_f32 " A1 ", " A1 ", %9\n\t"
	asm(TERRA_SG_2X2("%0", "%4", "%10") TERRA_SG_2X2("%1", "%5", "%11") TERRA_SG_2X2("%2", "%6", "%12") TERRA_SG_2X2("%3", "%7", "%14")
	    : "+v"(r0[0]), "+v"(r0[1]), "+v"(r0[2]), "+v"(r0[3]), "+v"(r1[0]), "+v"(r1[1]), "+v"(r1[2]), "+v"(r1[3]), "=&v"(t0), "=&v"(t1)
	    : "v"(xp[0]), "v"(xp[1]), "v"(xp[2]), "v"(yp), "v"(xp[3]));
#undef TERRA_SG_2X2
}
// {a.x*y, a.y*y} with y the low (SEL = 0) or high (SEL = 1) half of the register pair yp, broadcast by op_sel: the products of a*{y, y} without the copy that builds {y, y}
template<int SEL> __device__ __forceinline__ sg_v2f sg_pk_mul_bcast(sg_v2f a, sg_v2f yp) {
	sg_v2f r;
	if (SEL) {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(yp));}
	else     {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(yp));}
	return r;
}
// acc[i][jp] holds cells (row i, columns 2*jp, 2*jp+1) of the thread's 8 x 8 patch; one call = the four rows that one 16-byte Y read feeds (rows 4 h .. 4 h + 3)
struct sg_xop_t {float4 a, b;};
__device__ __forceinline__ sg_xop_t sg_load_x(float const *px, int k) {return sg_xop_t{*(float4 const *)(px + k*SG_BX), *(float4 const *)(px + k*SG_BX + 64)};}
__device__ __forceinline__ void sg_accumulate_half(sg_v2f (&acc)[SG_TY][SG_TX/2], sg_xop_t const &x, float4 const &y, int h) {
	sg_v2f const xp[4] = {{x.a.x, x.a.y}, {x.a.z, x.a.w}, {x.b.x, x.b.y}, {x.b.z, x.b.w}};
	sg_mul_add_2x8(acc[4*h], acc[4*h + 1], xp, sg_v2f{y.x, y.y});
	sg_mul_add_2x8(acc[4*h + 2], acc[4*h + 3], xp, sg_v2f{y.z, y.w});
}

// a value the compiler cannot see to be the same in all lanes of a wave (the wave's number in its block), as the scalar it is
__device__ __forceinline__ unsigned sg_wave_uniform(unsigned v) {return (unsigned)__builtin_amdgcn_readfirstlane((int)v);}
__device__ __forceinline__ char const *sg_wave_uniform_ptr(void const *p) {uint64_t const v = (uint64_t)(uintptr_t)p; return (char const *)(uintptr_t)(((uint64_t)sg_wave_uniform((unsigned)(v >> 32)) << 32) | sg_wave_uniform((unsigned)v));}
// one direct-to-LDS load: every lane's BYTES (4 or 16) from its own global address to lds + BYTES*lane, lds being the same in all lanes.  Counted by vmcnt like any load; the
// data is in LDS for the other waves after the next __syncthreads()
template<int BYTES> __device__ __forceinline__ void sg_load_to_lds(void const *g, float *lds) {
	static_assert(BYTES == 4 || BYTES == 16, "sg_load_to_lds: 4 or 16 bytes per lane");
	auto const src = (__attribute__((address_space(1))) void *)(uintptr_t)g; auto const dst = (__attribute__((address_space(3))) void *)lds;
	if (BYTES == 16) {__builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);} else {__builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);} // (the size is an immediate of the instruction)
}

// GENERAL = false: the host proved that every cell takes the short epilogue (terra_engine::sine_plain_only), so finish_cell() -- 64 inlined
// copies of the plateau / crater / crack / volcano / powf code, ~340 KB of instructions the hot path would otherwise be threaded through -- is left out
// PACKED (heightmap, GENERAL = false): the row length is a multiple of 4 (the host's promise, terra_hip.hip), the kernel is the packed epilogue and nothing else; PACKED = false
// is the same sum with the per-cell epilogue for the other row lengths, an instantiation of its own so that the hot one does not carry it
template<bool TILES, bool GENERAL, int KC = SG_KC, bool PACKED = true> __global__ __launch_bounds__(SG_THREADS) void k_sine_grid(grid_job_t job, noise_consts_t nc, sin_lut_t L,
	float const *__restrict__ xt, float const *__restrict__ yt, float const *__restrict__ smx, float const *__restrict__ smy, float *__restrict__ out, unsigned ntx, unsigned nty, uint32_t *__restrict__ mm, sg_tiles_t tiles)
{
	__shared__ __attribute__((aligned(16))) float sX[(KC + 2)*SG_BX];
	__shared__ __attribute__((aligned(16))) float sY[(KC + 2)*SG_BY];
	unsigned bxi, byi;
	if (!sg_tile_of_block(blockIdx.x, ntx, nty, tiles.rowgroup, bxi, byi)) return; // (nty: the tile rows of this launch, walked in XCD band order)
	if (!TILES) {byi += job.ty0;} // a heightmap launch may cover a window of the grid's tile rows (grid_job_t::ty0, tyn): everything below is in whole-grid terms
	uint32_t mm_lo = 0xFFFFFFFFu, mm_hi = 0xFFFFFFFFu; // fused min(vals)/max(vals) (heightmap_t::run_erosion, get_heightmap_z_range): saves a 4 B/cell read pass
	unsigned const tid = threadIdx.x, bx0 = bxi*SG_BX, by0 = byi*SG_BY;
	unsigned const tx = tid & 15, ty = tid >> 4;
	// thread (tx,ty) owns columns {tx*4..+3} u {64+tx*4..+3} and rows {ty*4..+3} u {64+ty*4..+3}: every LDS read is one aligned ds_read_b128,
	// 16 distinct 16-byte slots per 16-lane group for X (conflict-free) and a broadcast for Y
	float const *px = sX + tx*4, *py = sY + ty*4;
	sg_v2f acc[SG_TY][SG_TX/2];
#pragma unroll
	for (int i = 0; i < SG_TY; ++i) {
#pragma unroll
		for (int jp = 0; jp < SG_TX/2; ++jp) {acc[i][jp] = sg_v2f{0.0f, 0.0f};}
	}
	int const nk = F_TABLE_SIZE - job.kstart, nchunks = (nk + KC - 1)/KC, per_chunk = sg_chunk_len(job.kstart, KC);
	// the packed heightmap epilogue takes its island terms from LDS: the block's 128 of each axis go into the spare row KC + 1 (no chunk is staged there and no product reads it)
	// by direct-to-LDS loads, 4 bytes per lane -- waves 0, 1 the columns', waves 2, 3 the rows' -- which the first chunk's barrier waits for, so the epilogue never
	// waits for memory (the island tables are zero-padded to the tile grid like the sine tables)
	constexpr bool ISLANDS_IN_LDS = !TILES && !GENERAL && PACKED;
	if (ISLANDS_IN_LDS && job.glaciate && job.use_sine_mag) {
		unsigned const w = sg_wave_uniform(tid >> 6), h = w & 1u, lane = tid & 63u;
		if (w < 2u) {sg_load_to_lds<4>(smx + bx0 + h*64u + lane, sX + (KC + 1)*SG_BX + h*64u);}
		else        {sg_load_to_lds<4>(smy + by0 + h*64u + lane, sY + (KC + 1)*SG_BY + h*64u);}
		if (nchunks <= 0) {__syncthreads();} // (no term to sum: no chunk barrier either)
	}
	for (int c = 0; c < nchunks; ++c) { // terms are summed in k order across chunks, exactly like the CPU loop
		int const k0 = job.kstart + c*per_chunk, kn = ((k0 + per_chunk > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per_chunk);
		if (c > 0) {__syncthreads();} // everyone is done reading the previous chunk
		{	// stage the chunk straight into LDS, no register in between: one 16-byte direct-to-LDS load per wave moves 64 x 16 B = two whole 128-float rows (lanes 0..31 row r, lanes
			// 32..63 row r + 1; the LDS side of such a load is wave-uniform base + 16*lane, which is exactly the rows' layout).  Wave w takes the row pairs r = 2 w, 2 w + 8, ...
			// below kn: the only test is the scalar loop condition, and the addresses are a scalar base that advances by eight table rows plus one per-lane offset.  An odd kn
			// copies table row k0 + kn as well: the next chunk's first row or, behind row 89, the zero row the tables are padded with (sg_last_row_read(), terra_common.hpp)
			// into LDS row kn <= KC, which exists and is never used.
			unsigned const w2 = sg_wave_uniform(tid >> 6)*2u, lane = tid & 63u;
			unsigned const vx = ((lane >> 5)*job.nxp + (lane & 31u)*4u)*4u, vy = ((lane >> 5)*job.nyp + (lane & 31u)*4u)*4u; // bytes from the row pair's first cell (nxp, nyp < 2^29)
			char const *gx = sg_wave_uniform_ptr(xt + (size_t)(k0 + (int)w2)*job.nxp + bx0), *gy = sg_wave_uniform_ptr(yt + (size_t)(k0 + (int)w2)*job.nyp + by0);
			for (int r = (int)w2; r < kn; r += 8) {
				sg_load_to_lds<16>(gx + vx, sX + r*SG_BX); sg_load_to_lds<16>(gy + vy, sY + r*SG_BY);
				gx += (size_t)job.nxp*32u; gy += (size_t)job.nyp*32u;
			}
		}
		__syncthreads(); // (waits for the wave's direct-to-LDS loads -- vmcnt(0) -- before the barrier)
		// Operand registers: X (the eight columns, used by all eight rows of a step) in two sets that alternate between steps; Y (four rows per 16-byte read) in ONE set --
		// a Y read is reloaded with the next step's values right after the four rows that use it, half a step (64 packed instructions, ~256 cycles) before it is needed
		// again, an X set right after its step, a whole step ahead.  24 operand registers instead of 32: the kernel stays under 120 VGPRs, so that two of its waves fit on a
		// SIMD beside a droplet wave of another heightmap's erosion (264 registers), where one did before.  The scheduling barriers keep the loads where they are written
		// (the compiler would hoist them above the multiplies whose operands they replace, and copy).  Rows kn, kn + 1 may be read but are never used (KC + 2 rows are allocated).
		sg_xop_t XA = sg_load_x(px, 0), XB = sg_load_x(px, 1);
		float4 ya = *(float4 const *)py, yb = *(float4 const *)(py + 64);
		int k = 0;
		for (; k + 1 < kn; k += 2) {
			sg_accumulate_half(acc, XA, ya, 0); __builtin_amdgcn_sched_barrier(0); ya = *(float4 const *)(py + (k + 1)*SG_BY);
			sg_accumulate_half(acc, XA, yb, 1); __builtin_amdgcn_sched_barrier(0); yb = *(float4 const *)(py + (k + 1)*SG_BY + 64); XA = sg_load_x(px, k + 2);
			sg_accumulate_half(acc, XB, ya, 0); __builtin_amdgcn_sched_barrier(0); ya = *(float4 const *)(py + (k + 2)*SG_BY);
			sg_accumulate_half(acc, XB, yb, 1); __builtin_amdgcn_sched_barrier(0); yb = *(float4 const *)(py + (k + 2)*SG_BY + 64); XB = sg_load_x(px, k + 3);
		}
		if (k < kn) {sg_accumulate_half(acc, XA, ya, 0); sg_accumulate_half(acc, XA, yb, 1);}
	}
	// ---- epilogue (eval_index's tail, src/mesh_gen.cpp:781-790): shape / post-process, glaciate, sine-mag islands, volcano.
	// The common configuration (linear shape, no plateau/crater/crack, no volcano) takes a short path with the island terms of the
	// thread's 8 columns / 8 rows loaded once; anything else goes through the general finish_cell().  Same arithmetic either way.
	bool const vec_ok = ((job.nx & 3u) == 0) && !TILES;
	if (!GENERAL && TILES && (job.nx & 3u) == 0) {
		// the tile batch's common case: the packed epilogue of the grid (below), then the scatter into the per-tile layout -- a 4-cell group that lies in one tile goes out as ONE
		// 16-byte store (tile rows are 4-byte aligned only: tw = 130, 201, 129), a group across a tile boundary cell by cell.  (The per-cell epilogue with 8-byte stores made this
		// variant run at 0.7 of the grid kernel's rate: profiles/r06_tiles_kernel_stats.txt.)
		typedef sg_v2f v2f;
		typedef float st_f4u __attribute__((ext_vector_type(4), aligned(4)));
		bool const gl = job.glaciate && nc.glaciate, sm = job.glaciate && job.use_sine_mag;
		float4 sx[2], sy[2];
		sx[0] = sx[1] = sy[0] = sy[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (sm) { // (the batch's island tables end with the virtual grid: nothing is read behind nx / ny; nx is a multiple of 4 here, ny need not be)
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				unsigned const x = bx0 + h*64 + tx*4, y = by0 + h*64 + ty*4;
				if (x < job.nx) {sx[h] = *(float4 const *)(smx + x);}
				sy[h] = make_float4((y < job.ny) ? smy[y] : 0.0f, (y + 1 < job.ny) ? smy[y + 1] : 0.0f, (y + 2 < job.ny) ? smy[y + 2] : 0.0f, (y + 3 < job.ny) ? smy[y + 3] : 0.0f);
			}
		}
		v2f const zme = {nc.zmax_est, nc.zmax_est}, inv = {nc.zmax_est2_inv, nc.zmax_est2_inv}, z2 = {nc.zmax_est2, nc.zmax_est2}, off = {job.sine_offset, job.sine_offset};
		unsigned const tw = tiles.tw, twy = tiles.twy, os = tiles.ostride, nuy = job.ny/twy; // (the virtual grid is nux x nuy tiles of tw x twy cells)
		unsigned ux0[2], cx0[2], uy0[2], cy0[2];
#pragma unroll
		for (int half = 0; half < 2; ++half) {unsigned const x = bx0 + half*64 + tx*4; ux0[half] = x/tw; cx0[half] = x - ux0[half]*tw;}
#pragma unroll
		for (int g = 0; g < 2; ++g) {unsigned const y = by0 + g*64 + ty*4; uy0[g] = y/twy; cy0[g] = y - uy0[g]*twy;}
		// the tiles under the thread's cells: two tile columns per half at most (a group may cross into the next), two tile rows per 4-row group
		int tmap[2][2][2][2];
#pragma unroll
		for (int g = 0; g < 2; ++g) {
#pragma unroll
			for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
				for (int half = 0; half < 2; ++half) {
#pragma unroll
					for (int dx = 0; dx < 2; ++dx) {
						unsigned const uy = uy0[g] + dy, ux = ux0[half] + dx;
						tmap[g][dy][half][dx] = (uy < nuy && ux < tiles.nux) ? tiles.tile_map[uy*tiles.nux + ux] : -1;
					}
				}
			}
		}
#pragma unroll
		for (int i = 0; i < SG_TY; ++i) {
			unsigned const y = by0 + (i >> 2)*64 + ty*4 + (i & 3);
			if (y >= job.ny) continue;
			float const syq[4] = {sy[i >> 2].x, sy[i >> 2].y, sy[i >> 2].z, sy[i >> 2].w};
			v2f const syi = {syq[i & 3], syq[i & 3]};
			unsigned cy = cy0[i >> 2] + (unsigned)(i & 3); int dy = 0;
			if (cy >= twy) {cy -= twy; dy = 1;}
			unsigned const oy = cy + ((cy >= tiles.ysplit) ? tiles.ygap : 0u); // row of the tile's field
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				unsigned const x = bx0 + half*64 + tx*4;
				if (x >= job.nx) continue;
				v2f z01 = acc[i][half*2], z23 = acc[i][half*2 + 1];
				if (gl) {
					v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
					z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
				}
				if (sm) {
					v2f const s01 = {sx[half].x, sx[half].y}, s23 = {sx[half].z, sx[half].w};
					z01 = z01 + (s01*syi + off); z23 = z23 + (s23*syi + off);
				}
				unsigned const cx = cx0[half];
				int const ta = dy ? tmap[i >> 2][1][half][0] : tmap[i >> 2][0][half][0], tb = dy ? tmap[i >> 2][1][half][1] : tmap[i >> 2][0][half][1];
				if (cx + 3 < tw && (cx + 3 < tiles.xsplit || cx >= tiles.xsplit)) { // the whole group in one tile row (and on one side of a band's gap)
					unsigned const ox = cx + ((cx >= tiles.xsplit) ? tiles.xgap : 0u);
					if (ta >= 0) {*(st_f4u *)(out + (size_t)ta*os*os + oy*os + ox) = st_f4u{z01.x, z01.y, z23.x, z23.y};}
				}
				else {
					float const v[4] = {z01.x, z01.y, z23.x, z23.y};
#pragma unroll
					for (int j = 0; j < 4; ++j) {
						bool const next = cx + (unsigned)j >= tw;
						int const t = next ? tb : ta;
						unsigned const cxx = next ? cx + (unsigned)j - tw : cx + (unsigned)j, ox = cxx + ((cxx >= tiles.xsplit) ? tiles.xgap : 0u);
						if (t >= 0) {out[(size_t)t*os*os + oy*os + ox] = v[j];}
					}
				}
			}
		}
		return; // (a tile batch has no fused min / max)
	}
	if constexpr (!GENERAL && !TILES && PACKED) {
		// the common case, two cells per instruction (v_pk_mul_f32 / v_pk_add_f32): the island tables are zero-padded to the tile grid, rows of 4 cells
		// are either wholly inside the grid or wholly outside
		typedef sg_v2f v2f;
		bool const gl = job.glaciate && nc.glaciate, sm = job.glaciate && job.use_sine_mag;
		float4 sx[2], sy[2];
		auto const islands = [&]() { // (staged in front of the first chunk, see above)
			sx[0] = *(float4 const *)(px + (KC + 1)*SG_BX); sx[1] = *(float4 const *)(px + (KC + 1)*SG_BX + 64);
			sy[0] = *(float4 const *)(py + (KC + 1)*SG_BY); sy[1] = *(float4 const *)(py + (KC + 1)*SG_BY + 64);
		};
		v2f const zme = {nc.zmax_est, nc.zmax_est}, inv = {nc.zmax_est2_inv, nc.zmax_est2_inv}, z2 = {nc.zmax_est2, nc.zmax_est2}, off = {job.sine_offset, job.sine_offset};
		float fmn = INFINITY, fmx = -INFINITY;
		if (bx0 + SG_BX <= job.nx && by0 + SG_BY <= job.ny && job.nx < (1u << 24)) {
			// a block wholly inside the grid (all but the last tile column / row of a map): the 16 groups of 4 cells in a straight line -- no lane is masked, gl / sm are
			// tested once per block, a row's island term is broadcast from its register pair by op_sel, and the stores share one per-lane offset (< 2^32 bytes: nx < 2^24) on a
			// scalar row address.  The same operations on the same values in the same order as the guarded loop below.
			unsigned const voff = (ty*4u*job.nx + tx*4u)*4u;
			char *const ob = (char *)(out + (size_t)by0*job.nx + bx0);
			size_t const rowb = (size_t)job.nx*4u;
			auto const groups = [&](auto GL, auto SM) {
				if (decltype(SM)::value) {islands();}
#pragma unroll
				for (int i = 0; i < SG_TY; ++i) {
					char *const orow = ob + (size_t)((i >> 2)*64 + (i & 3))*rowb;
					v2f const syp = (i & 2) ? v2f{sy[i >> 2].z, sy[i >> 2].w} : v2f{sy[i >> 2].x, sy[i >> 2].y};
#pragma unroll
					for (int half = 0; half < 2; ++half) {
						v2f z01 = acc[i][half*2], z23 = acc[i][half*2 + 1];
						if (decltype(GL)::value) {
							v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
							z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
						}
						if (decltype(SM)::value) {
							v2f const s01 = {sx[half].x, sx[half].y}, s23 = {sx[half].z, sx[half].w};
							z01 = z01 + (((i & 1) ? sg_pk_mul_bcast<1>(s01, syp) : sg_pk_mul_bcast<0>(s01, syp)) + off); z23 = z23 + (((i & 1) ? sg_pk_mul_bcast<1>(s23, syp) : sg_pk_mul_bcast<0>(s23, syp)) + off);
						}
						fmn = sg_min3(sg_min3(fmn, z01.x, z01.y), z23.x, z23.y);
						fmx = sg_max3(sg_max3(fmx, z01.x, z01.y), z23.x, z23.y);
						*(float4 *)(orow + half*256 + voff) = make_float4(z01.x, z01.y, z23.x, z23.y);
					}
				}
			};
			typedef std::true_type yes; typedef std::false_type no;
			if (gl) {if (sm) {groups(yes(), yes());} else {groups(yes(), no());}}
			else    {if (sm) {groups(no(), yes());} else {groups(no(), no());}}
		}
		else { // a block on the grid's right or lower edge
		sx[0] = sx[1] = sy[0] = sy[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (sm) {islands();}
#pragma unroll
		for (int i = 0; i < SG_TY; ++i) {
			unsigned const y = by0 + (i >> 2)*64 + ty*4 + (i & 3);
			if (y >= job.ny) continue;
			float const syq[4] = {sy[i >> 2].x, sy[i >> 2].y, sy[i >> 2].z, sy[i >> 2].w};
			v2f const syi = {syq[i & 3], syq[i & 3]};
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				unsigned const x = bx0 + half*64 + tx*4;
				if (x >= job.nx) continue;
				v2f z01 = acc[i][half*2], z23 = acc[i][half*2 + 1];
				if (gl) {
					v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
					z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
				}
				if (sm) {
					v2f const s01 = {sx[half].x, sx[half].y}, s23 = {sx[half].z, sx[half].w};
					z01 = z01 + (s01*syi + off); z23 = z23 + (s23*syi + off);
				}
				fmn = sg_min3(sg_min3(fmn, z01.x, z01.y), z23.x, z23.y); // (v_min3 / v_max3 by hand: fminf / fmaxf on values that come out of the inline-asm sum cost a canonicalising
				fmx = sg_max3(sg_max3(fmx, z01.x, z01.y), z23.x, z23.y); //  v_max x, x per operand -- 12 instructions per 4 cells instead of 4; NaNs are skipped either way)
				*(float4 *)(out + (size_t)y*job.nx + x) = make_float4(z01.x, z01.y, z23.x, z23.y);
			}
		}
		}
		if (mm) {
			if (fmn <= fmx) {mm_lo = f2ord(fmn); mm_hi = ~f2ord(fmx);}
			wave_minmax_publish_full(mm_lo, mm_hi, mm); // (all 64 lanes are here: a block leaves the kernel as a whole or not at all)
		}
		return;
	}
	hmap_params_t const &hp = nc.hp;
	bool const plain = !GENERAL || ((job.shape == 0) && !(hp.crack_lo < hp.crack_hi) && !(hp.volcano_width > 0.0f && hp.volcano_height > 0.0f));
	float const pp_limit = min_std(hp.plat_bot, hp.crat_h); // below this the post-process is the identity
	float smxv[SG_TX], smyv[SG_TY];
#pragma unroll
	for (int j = 0; j < SG_TX; ++j) {unsigned const x = bx0 + (j >> 2)*64 + tx*4 + (j & 3); smxv[j] = (job.use_sine_mag && x < job.nx) ? smx[x] : 0.0f;}
#pragma unroll
	for (int i = 0; i < SG_TY; ++i) {unsigned const y = by0 + (i >> 2)*64 + ty*4 + (i & 3); smyv[i] = (job.use_sine_mag && y < job.ny) ? smy[y] : 0.0f;}
	float fmn = INFINITY, fmx = -INFINITY;
	unsigned t_ux[2] = {0, 0}, t_cx[2] = {0, 0}, t_uy[4] = {0, 0, 0, 0}, t_cy[4] = {0, 0, 0, 0}; // TILES: tile column / row and offset of the thread's two 4-cell groups and four 4-row groups
	if (TILES) {
#pragma unroll
		for (int half = 0; half < 2; ++half) {unsigned const x = bx0 + half*64 + tx*4; t_ux[half] = x/tiles.tw; t_cx[half] = x - t_ux[half]*tiles.tw;}
#pragma unroll
		for (int g = 0; g < 4; ++g) {unsigned const y = by0 + g*64 + ty*4; t_uy[g] = y/tiles.tw; t_cy[g] = y - t_uy[g]*tiles.tw;}
	}
#pragma unroll
	for (int i = 0; i < SG_TY; ++i) {
		unsigned const y = by0 + (i >> 2)*64 + ty*4 + (i & 3);
		if (y >= job.ny) continue;
#pragma unroll
		for (int half = 0; half < 2; ++half) {
			unsigned const x = bx0 + half*64 + tx*4;
			if (x >= job.nx) continue;
			float v[4];
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				float z = acc[i][half*2 + (j >> 1)][j & 1];
				if (!GENERAL || (plain && !(z > pp_limit))) {
					if (job.glaciate) {
						if (nc.glaciate) {float const relh = (z + nc.zmax_est)*nc.zmax_est2_inv; z = (GENERAL ? glaciate_exp_fn(relh, nc.custom_glaciate_exp) : relh*relh*relh)*nc.zmax_est2 - nc.zmax_est;} // !GENERAL: custom_glaciate_exp == 0
						if (job.use_sine_mag) {z += smxv[half*4 + j]*smyv[i] + job.sine_offset;}
					}
				}
				else if (GENERAL && x + j < job.nx) {
					if (TILES) { // general epilogue in tile-local coordinates (volcano term needs the tile's own origin)
						unsigned const tw = tiles.tw, ux = (x + j)/tw, uy = y/tw;
						grid_job_t jt = job; jt.mx0 = tiles.m0[ux]; jt.my0 = tiles.m0[tiles.nux + uy];
						z = finish_cell(z, jt, nc, L, smx + ux*tw, smy + uy*tw, (x + j) - ux*tw, y - uy*tw);
					}
					else {z = finish_cell(z, job, nc, L, smx, smy, x + j, y);}
				}
				else {z = 0.0f;}
				v[j] = z;
				if (x + j < job.nx) {fmn = fminf(fmn, z); fmx = fmaxf(fmx, z);} // fminf/fmaxf skip NaNs, like min_eq/max_eq never let a NaN win
			}
			if (TILES) { // scatter into the per-tile layout: tile column / row and the offsets inside come from the thread's precomputed bases (no division per cell)
				unsigned const tw = tiles.tw;
				unsigned uy = t_uy[i >> 2], cy = t_cy[i >> 2] + (unsigned)(i & 3);
				if (cy >= tw) {cy -= tw; ++uy;}
				if ((tw & 1u) == 0) { // even tile width (130): x is a multiple of 4, so cell pairs (j, j+1) share a tile row and are 8-byte aligned there
#pragma unroll
					for (int j = 0; j < 4; j += 2) {
						if (x + j >= job.nx) continue; // nx = nux*tw is even as well: the pair is inside or outside together
						unsigned ux = t_ux[half], cx = t_cx[half] + (unsigned)j;
						if (cx >= tw) {cx -= tw; ++ux;}
						int const t = tiles.tile_map[uy*tiles.nux + ux];
						if (t >= 0) {*(float2 *)(out + (size_t)t*tw*tw + cy*tw + cx) = make_float2(v[j], v[j + 1]);}
					}
					continue;
				}
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					if (x + j >= job.nx) continue;
					unsigned ux = t_ux[half], cx = t_cx[half] + (unsigned)j;
					if (cx >= tw) {cx -= tw; ++ux;}
					int const t = tiles.tile_map[uy*tiles.nux + ux];
					if (t >= 0) {out[(size_t)t*tw*tw + cy*tw + cx] = v[j];}
				}
				continue;
			}
			float *o = out + (size_t)y*job.nx + x;
			if (vec_ok) {*(float4 *)o = make_float4(v[0], v[1], v[2], v[3]);}
			else {
#pragma unroll
				for (int j = 0; j < 4; ++j) {if (x + j < job.nx) o[j] = v[j];}
			}
		}
	}
	if (mm) {
		if (fmn <= fmx) {mm_lo = f2ord(fmn); mm_hi = ~f2ord(fmx);}
		wave_minmax_publish(mm_lo, mm_hi, mm);
	}
}

// ---- K1, the heightmap's hot form (plain-only, row length a multiple of 4, KC = 27): the ROW operands are scalars.
// A wave is 64 lanes along x and a lane owns 4 columns x 16 rows -- the same 32 packed accumulators as above -- so a row's value is the same in all 64 lanes: it belongs in
// scalar registers, not in LDS plus VGPRs.  A block is four waves stacked in y: 256 columns x 64 rows, the same 16384 cells as a 128 x 128 block.  Only X is staged in LDS
// (one direct-to-LDS load per wave = one whole 256-float row; KC + 2 rows = 29.7 KB as before); per term a lane reads its four columns with ONE ds_read_b128 and the wave
// its 16 row values yt[k][y0 .. y0 + 15] with ONE 64-byte scalar load, and the 32 + 32 packed instructions take the row value from an SGPR pair through op_sel -- a quarter
// of the LDS read bytes of the 8 x 8 form, no VGPR read for the row operand, 8 operand VGPRs instead of 24.  Same multiplies and adds on the same values in the same k
// order: same bits.  What it buys is CLOCK, not cycles (profiles/r11_sine_rowscalar_probe.txt: the two loops take the same shader cycles per block, the chip holds
// ~2.24 GHz under this one against ~2.12 GHz under the 8 x 8 loop).
// LDS reads and scalar loads share one counter and scalar loads return out of order, so the only wait is lgkmcnt(0): a stage is one term -- wait, put the next term's
// ds_read_b128 and scalar load in flight, run this term's 64 packed instructions.  A buffer whose load is in flight must never meet a register copy: the buffers are asm
// operands from issue to use, vector and scalar outputs never share an asm statement (mixed, the compiler takes the scalar ones for divergent values and cannot carry them
// around the loop), and no scalar buffer is live from one chunk to the next (the compiler puts copies where two paths join).
// Columns behind the padded row length (the last block of a grid whose nxp is an odd multiple of 128) are staged from the row's last four columns instead: whatever they
// sum to is never stored.  Rows: nyp = round_up(ny, 128) covers every 64-row block's scalar loads, and the last prefetch of a chunk reads table row k0 + kn <= 90
// (sg_rs_last_row_read(), terra_common.hpp) and LDS row kn <= KC.
constexpr int SGR_BX = 256, SGR_BY = 64, SGR_ROWS = 16;
typedef unsigned sgr_u2 __attribute__((ext_vector_type(2)));   // scalar operands live in integer types: uniform integers stay in SGPRs
typedef unsigned sgr_u16 __attribute__((ext_vector_type(16)));
typedef float sgr_v4f __attribute__((ext_vector_type(4)));
typedef sgr_u16 const __attribute__((address_space(4))) *sgr_row16_ptr;
// Eight rows x four columns per asm statement.  Per row pair, r0 += {x0*y0, x1*y0}, {x2*y0, x3*y0} and r1 the same with y1: (y0, y1) is an SGPR pair, the row's value
// broadcast from either half by op_sel.  mul / mul / add / add as in sg_mul_add_2x8; product rounded by v_pk_mul_f32, then added by v_pk_add_f32: never fused.
__device__ __forceinline__ void sgr_mul_add_8x4(sg_v2f (&acc)[SGR_ROWS][2], int r, sg_v2f x01, sg_v2f x23, sgr_u2 y01, sgr_u2 y23, sgr_u2 y45, sgr_u2 y67) { // rows r .. r + 7
	sg_v2f t0, t1;
#define TERRA_SGR_2X4(R00, R01, R10, R11, Y) \
	"v_pk_mul_f32 %16, %18, " Y " op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %17, %18, " Y " op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " R00 ", " R00 ", %16\n\t" \
	"v_pk_add_f32 " R10 ", " R10 ", %17\n\t" \
	"v_pk_mul_f32 %16, %19, " Y " op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %17, %19, " Y " op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " R01 ", " R01 ", %16\n\t" \
	"v_pk_add_f32 " R11 ", " R11 ", %17\n\t"
	asm(TERRA_SGR_2X4("%0", "%1", "%2", "%3", "%20") TERRA_SGR_2X4("%4", "%5", "%6", "%7", "%21") TERRA_SGR_2X4("%8", "%9", "%10", "%11", "%22") TERRA_SGR_2X4("%12", "%13", "%14", "%15", "%23")
	    : "+v"(acc[r][0]), "+v"(acc[r][1]), "+v"(acc[r + 1][0]), "+v"(acc[r + 1][1]), "+v"(acc[r + 2][0]), "+v"(acc[r + 2][1]), "+v"(acc[r + 3][0]), "+v"(acc[r + 3][1]),
	      "+v"(acc[r + 4][0]), "+v"(acc[r + 4][1]), "+v"(acc[r + 5][0]), "+v"(acc[r + 5][1]), "+v"(acc[r + 6][0]), "+v"(acc[r + 6][1]), "+v"(acc[r + 7][0]), "+v"(acc[r + 7][1]),
	      "=&v"(t0), "=&v"(t1)
	    : "v"(x01), "v"(x23), "s"(y01), "s"(y23), "s"(y45), "s"(y67));
#undef TERRA_SGR_2X4
}
__device__ __forceinline__ void sgr_accumulate_term(sg_v2f (&acc)[SGR_ROWS][2], sgr_v4f const &x, sgr_u16 const &y) {
	sg_v2f const x01 = {x.x, x.y}, x23 = {x.z, x.w};
	sgr_mul_add_8x4(acc, 0, x01, x23, sgr_u2{y.s0, y.s1}, sgr_u2{y.s2, y.s3}, sgr_u2{y.s4, y.s5}, sgr_u2{y.s6, y.s7});
	sgr_mul_add_8x4(acc, 8, x01, x23, sgr_u2{y.s8, y.s9}, sgr_u2{y.sa, y.sb}, sgr_u2{y.sc, y.sd}, sgr_u2{y.se, y.sf});
}
// {a.x*y, a.y*y} with y the low (SEL = 0) or high (SEL = 1) half of the SGPR pair yp
template<int SEL> __device__ __forceinline__ sg_v2f sgr_pk_mul_bcast(sg_v2f a, sgr_u2 yp) {
	sg_v2f r;
	if (SEL) {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "s"(yp));}
	else     {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "s"(yp));}
	return r;
}
// ntx: 256-column blocks of the padded row; nty: 64-row blocks of this launch, the first of them block row 2 job.ty0 of the grid (grid_job_t::ty0 / tyn stay in 128-row units)
template<int KC> __global__ __launch_bounds__(SG_THREADS) void k_sine_grid_rs(grid_job_t job, noise_consts_t nc, float const *__restrict__ xt, float const *__restrict__ yt,
	float const *__restrict__ smx, float const *__restrict__ smy, float *__restrict__ out, unsigned ntx, unsigned nty, unsigned rowgroup, uint32_t *__restrict__ mm)
{
	__shared__ __attribute__((aligned(16))) float sX[(KC + 2)*SGR_BX];
	unsigned bxi, byi;
	if (!sg_tile_of_block(blockIdx.x, ntx, nty, rowgroup, bxi, byi)) return;
	byi += job.ty0*2u;
	uint32_t mm_lo = 0xFFFFFFFFu, mm_hi = 0xFFFFFFFFu;
	unsigned const tid = threadIdx.x, bx0 = bxi*SGR_BX, by0 = byi*SGR_BY;
	unsigned const w = sg_wave_uniform(tid >> 6), lane = tid & 63u;
	sg_v2f acc[SGR_ROWS][2];
#pragma unroll
	for (int i = 0; i < SGR_ROWS; ++i) {acc[i][0] = sg_v2f{0.0f, 0.0f}; acc[i][1] = sg_v2f{0.0f, 0.0f};}
	int const nk = F_TABLE_SIZE - job.kstart, nchunks = (nk + KC - 1)/KC, per_chunk = sg_chunk_len(job.kstart, KC);
	// the island terms of the block's 256 columns go into the spare LDS row KC + 1, 64 per wave (the row terms are scalars: loaded in the epilogue)
	if (job.glaciate && job.use_sine_mag) {
		if (bx0 + w*64u < job.nxp) {sg_load_to_lds<4>(smx + bx0 + w*64u + lane, sX + (KC + 1)*SGR_BX + w*64u);}
		if (nchunks <= 0) {__syncthreads();}
	}
	unsigned const xcol = bx0 + lane*4u, vx = (((xcol < job.nxp) ? xcol : job.nxp - 4u) - bx0)*4u; // bytes from the block's first column; behind the padded row: its last four columns
	size_t const rowb = (size_t)job.nyp*4u;
	char const *const ybase = sg_wave_uniform_ptr(yt + by0 + w*(unsigned)SGR_ROWS); // the wave's 16 rows of table row 0: 64 bytes, 64-byte aligned
	unsigned const la = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)sX + lane*16u; // the lane's four columns of LDS row 0
	sgr_v4f xa, xb; sgr_u16 ya, yb;
#define TERRA_SGR_NEXT(CX, CY, NX, NY, LADDR, OFF, YP) \
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %1, %2, 0x0" : "+s"(CY), "=&s"(NY) : "s"(YP)); \
	asm volatile("ds_read_b128 %1, %2 offset:" #OFF : "+v"(CX), "=&v"(NX) : "v"(LADDR))
	for (int c = 0; c < nchunks; ++c) { // terms are summed in k order across chunks, exactly like the CPU loop
		int const k0 = job.kstart + c*per_chunk, kn = ((k0 + per_chunk > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per_chunk);
		if (c > 0) {__syncthreads();} // everyone is done reading the previous chunk
		char const *yp = ybase + (size_t)k0*rowb;
		asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(ya) : "s"(yp)); // the chunk's first row operands, asked for in front of the staging, land under it
		{	// wave w takes the table rows w, w + 4, ... below kn: the only test is the scalar loop condition
			char const *gx = sg_wave_uniform_ptr(xt + (size_t)(k0 + (int)w)*job.nxp + bx0);
			for (int r = (int)w; r < kn; r += 4) {sg_load_to_lds<16>(gx + vx, sX + r*SGR_BX); gx += (size_t)job.nxp*16u;}
		}
		__syncthreads(); // (waits for the wave's direct-to-LDS loads -- vmcnt(0) -- before the barrier)
		asm volatile("ds_read_b128 %0, %1" : "=&v"(xa) : "v"(la));
		unsigned a = la;
		int k = 0;
		for (; k + 1 < kn; k += 2) { // (the last pair's second stage asks for LDS row kn and table row k0 + kn: both exist, neither is used)
			TERRA_SGR_NEXT(xa, ya, xb, yb, a, 1024, yp + rowb);   sgr_accumulate_term(acc, xa, ya); __builtin_amdgcn_sched_barrier(0);
			TERRA_SGR_NEXT(xb, yb, xa, ya, a, 2048, yp + 2*rowb); sgr_accumulate_term(acc, xb, yb); __builtin_amdgcn_sched_barrier(0);
			a += 2048u; yp += 2*rowb;
		}
		asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ya)); asm volatile("" : "+v"(xa)); // nothing is in flight when the block meets at the next barrier
		if (k < kn) {sgr_accumulate_term(acc, xa, ya); __builtin_amdgcn_sched_barrier(0);}
	}
#undef TERRA_SGR_NEXT
	// ---- the packed epilogue of k_sine_grid (glaciate, island term, off; fused min / max): a lane's island column terms are its 4 floats of LDS row KC + 1, the 16 row terms
	// of the wave are scalars (one 64-byte scalar load; the island tables are zero-padded like the sine tables)
	typedef sg_v2f v2f;
	bool const gl = job.glaciate && nc.glaciate, sm = job.glaciate && job.use_sine_mag;
	float4 sx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	sgr_u16 sy = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
	auto const islands = [&]() {sx = *(float4 const *)(sX + (KC + 1)*SGR_BX + lane*4u); sy = *(sgr_row16_ptr)(uintptr_t)(smy + by0 + w*(unsigned)SGR_ROWS);};
	v2f const zme = {nc.zmax_est, nc.zmax_est}, inv = {nc.zmax_est2_inv, nc.zmax_est2_inv}, z2 = {nc.zmax_est2, nc.zmax_est2}, off = {job.sine_offset, job.sine_offset};
	float fmn = INFINITY, fmx = -INFINITY;
	if (bx0 + SGR_BX <= job.nx && by0 + SGR_BY <= job.ny && job.nx < (1u << 24)) {
		// a block wholly inside the grid: 16 rows in a straight line -- no lane is masked, gl / sm are tested once per block, and a wave's store is 64 lanes x 16 bytes = 1 KB
		// of one row, one per-lane offset on a scalar row address.  The same operations on the same values in the same order as the guarded loop below.
		unsigned const voff = lane*16u;
		char *const ob = (char *)(out + (size_t)(by0 + w*(unsigned)SGR_ROWS)*job.nx + bx0);
		size_t const rowbytes = (size_t)job.nx*4u;
		auto const rows = [&](auto GL, auto SM) {
			if (decltype(SM)::value) {islands();}
#pragma unroll
			for (int i = 0; i < SGR_ROWS; ++i) {
				v2f z01 = acc[i][0], z23 = acc[i][1];
				if (decltype(GL)::value) {
					v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
					z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
				}
				if (decltype(SM)::value) {
					v2f const s01 = {sx.x, sx.y}, s23 = {sx.z, sx.w};
					sgr_u2 const syp = {sy[i & ~1], sy[i | 1]};
					z01 = z01 + (((i & 1) ? sgr_pk_mul_bcast<1>(s01, syp) : sgr_pk_mul_bcast<0>(s01, syp)) + off); z23 = z23 + (((i & 1) ? sgr_pk_mul_bcast<1>(s23, syp) : sgr_pk_mul_bcast<0>(s23, syp)) + off);
				}
				fmn = sg_min3(sg_min3(fmn, z01.x, z01.y), z23.x, z23.y);
				fmx = sg_max3(sg_max3(fmx, z01.x, z01.y), z23.x, z23.y);
				// a streaming store: this kernel never reads a row again and a map is far larger than the L2.  profiles/r12_sine_epilogue_probe.txt: 757 -> 744 us per map at the
				// same clock and the same cycles per block, SQ_WAIT_ANY 0.13 -> 0.10 of the wave cycles (the tables' fetch traffic is the same: every XCD reads them once either way)
				__builtin_nontemporal_store(st_f4{z01.x, z01.y, z23.x, z23.y}, (st_f4 *)(ob + (size_t)i*rowbytes + voff));
			}
		};
		typedef std::true_type yes; typedef std::false_type no;
		if (gl) {if (sm) {rows(yes(), yes());} else {rows(yes(), no());}}
		else    {if (sm) {rows(no(), yes());} else {rows(no(), no());}}
	}
	else { // a block on the grid's right or lower edge: rows of 4 cells are either wholly inside the grid or wholly outside
		if (sm) {islands();}
		unsigned const x = bx0 + lane*4u;
#pragma unroll
		for (int i = 0; i < SGR_ROWS; ++i) {
			unsigned const y = by0 + w*(unsigned)SGR_ROWS + (unsigned)i;
			if (y >= job.ny || x >= job.nx) continue;
			float const syf = __uint_as_float(sy[i]);
			v2f const syi = {syf, syf};
			v2f z01 = acc[i][0], z23 = acc[i][1];
			if (gl) {
				v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
				z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
			}
			if (sm) {
				v2f const s01 = {sx.x, sx.y}, s23 = {sx.z, sx.w};
				z01 = z01 + (s01*syi + off); z23 = z23 + (s23*syi + off);
			}
			fmn = sg_min3(sg_min3(fmn, z01.x, z01.y), z23.x, z23.y);
			fmx = sg_max3(sg_max3(fmx, z01.x, z01.y), z23.x, z23.y);
			*(float4 *)(out + (size_t)y*job.nx + x) = make_float4(z01.x, z01.y, z23.x, z23.y);
		}
	}
	if (mm) {
		if (fmn <= fmx) {mm_lo = f2ord(fmn); mm_hi = ~f2ord(fmx);}
		wave_minmax_publish_full(mm_lo, mm_hi, mm); // (all 64 lanes are here: a block leaves the kernel as a whole or not at all)
	}
}

// ------------------------------------------------------------------ K5 tile mode: LDS-resident padded grid, serial droplets
// how much of a tile is land: droplets that start under water stop at once, the others walk ~50 steps, so this predicts a tile's serial chain length
__global__ __launch_bounds__(256) void k_tile_land_cells(float const *__restrict__ zvals, uint32_t cells, float water_thresh, uint32_t *__restrict__ land) {
	float const *z = zvals + (size_t)blockIdx.x*cells;
	uint32_t cnt = 0;
	for (uint32_t i = threadIdx.x; i < cells; i += 256) {cnt += !(z[i] < water_thresh) ? 1u : 0u;} // a NaN counts as land: it does not pass the ocean test either
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {cnt += __shfl_down(cnt, off, 64);}
	if ((threadIdx.x & 63) == 0 && cnt) {atomicAdd(&land[blockIdx.x], cnt);}
}
// the stable descending order of the tiles by land count, without a sort: tile i goes to position #{j : land[j] > land[i]} + #{j < i : land[j] == land[i]}
__global__ __launch_bounds__(256) void k_tile_order_by_land(uint32_t const *__restrict__ land, uint32_t n, uint32_t *__restrict__ order) {
	__shared__ uint32_t s_land[256];
	uint32_t const i = blockIdx.x*256 + threadIdx.x;
	uint32_t const mine = (i < n) ? land[i] : 0u;
	uint32_t pos = 0;
	for (uint32_t j0 = 0; j0 < n; j0 += 256) {
		__syncthreads();
		s_land[threadIdx.x] = (j0 + threadIdx.x < n) ? land[j0 + threadIdx.x] : 0u;
		__syncthreads();
		uint32_t const cnt = (n - j0 < 256u) ? n - j0 : 256u;
		for (uint32_t e = 0; e < cnt; ++e) {uint32_t const l = s_land[e]; pos += (l > mine || (l == mine && j0 + e < i)) ? 1u : 0u;}
	}
	if (i < n) {order[pos] = i;}
}
// `order` (or null): the tile each block takes.  Blocks are dispatched in index order and only two tiles fit a CU, so the batch is a list-scheduling
// problem: handing out the longest chains first keeps the heavy land tiles from forming the tail of the launch.
__global__ __launch_bounds__(64) void k_tile_erosion(float *__restrict__ zvals, erosion_consts_t ec, uint32_t iters, uint32_t const *__restrict__ order, uint32_t const *__restrict__ land) {
	extern __shared__ __attribute__((aligned(16))) float te_pad[];
	int const NX = ec.NX, NY = ec.NY, xs = ec.xsize, ys = ec.ysize;
	uint32_t const tile = order ? order[blockIdx.x] : blockIdx.x;
	float *z = zvals + (size_t)tile*xs*ys;
	if (land && land[tile] == 0) { // every cell (and so every clamp-padded copy) is below the ocean threshold: each droplet stops at its first step without a write
		// (src/erosion.cpp:98), so apply_erosion reduces to its final clamp -- no need to hold one of the chip's 512 LDS tile slots for a thousand such droplets
		for (int i = threadIdx.x; i < xs*ys; i += 64) {z[i] = max_std(ec.min_zval, z[i]);}
		return;
	}
	for (int i = threadIdx.x; i < NX*NY; i += 64) { // clamp-padded copy (src/erosion.cpp:31-37), coalesced rows
		int const X = i % NX, Z = i / NX;
		te_pad[i] = z[(size_t)imax(imin(Z - EROSION_PAD, ys-1), 0)*xs + imax(imin(X - EROSION_PAD, xs-1), 0)];
	}
	__syncthreads();
	{ // droplet order is the semantics: droplets run one after another; within a droplet the wave's lanes share the brush / corner accesses (LDS latency, not HBM, bounds a step)
		wave_lds_mem_t m; m.pad = te_pad; m.NX = NX; m.NY = NY;
		for (uint32_t it = 0; it < iters; ++it) {simulate_droplet((int)it, m, ec);}
	}
	__syncthreads();
	for (int i = threadIdx.x; i < xs*ys; i += 64) { // unpad + clamp (src/erosion.cpp:158-162)
		int const x = i % xs, y = i / xs;
		z[i] = max_std(ec.min_zval, te_pad[(y + EROSION_PAD)*NX + (x + EROSION_PAD)]);
	}
}

// ------------------------------------------------------------------ K6+K7: tile post-pass, one 256-thread block per tile
// sub-block z ranges, water bbox (ints), mzmin/mzmax/radius (src/tiled_mesh.cpp:517-541) and RGBA8 normals + min_normal_z (src/tiled_mesh.cpp:865-880).
// HBM-bound: 4 B read + 4 B written per cell; reductions go through LDS atomics on order-preserving uints.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {uint32_t const o = __shfl_down(v, off, 64); v = (o < v) ? o : v;}
	return v; // valid in lane 0
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {int const o = __shfl_down(v, off, 64); v = (o < v) ? o : v;}
	return v;
}
// One block per (tile, band of 32 texel rows): 4 x more blocks than tiles and 17.7 KB of LDS each.  Band yy owns sub-block row yy completely (rows 32*yy .. 32*yy + 32), so the
// 4 x 4 sub-block ranges are written by exactly one block each; what spans the tile (the water bbox, min_normal_z) is folded through 8 words of global scratch per tile with
// atomics and written by a one-thread-per-tile kernel afterwards.
//
// Round 5: the kernel was instruction-bound (127 per texel: three IEEE divisions, a square root, three double-precision byte conversions, an index division).  Now a WAVE walks
// rows -- lane = column, both halves of a row per step, column 128 in one extra pass -- so the row / water bookkeeping is scalar, and a texel's three bytes come from ~40 instructions:
//   * the bytes are floor(127*(n_i/|n| + 1)).  t_i = fma(127, n_i*rsq(s), 127) is within 4.6e-5 of the double-precision value the reference truncates (rsq <= 2^-23 relative:
//     terra_selftest_hot_sqrt checks every fp32 input; RN(n/RN(sqrt(s))) is within 2^-23 relative of n/sqrt(s); the fma rounds once, <= 2^-17), so when every t_i of a wave's step
//     is further than TP_EPS = 2^-14 from an integer, floor(t_i) IS the reference's byte.  Otherwise (a few percent of the steps, and every NaN / Inf) the whole step is redone
//     with the reference's own statements (tile_normal_v + the double conversion).  Exactly flat texels (n_x = n_y = 0: ocean floor) would always land on an integer: their word
//     is a launch constant, computed by the host with the same statements.
//   * min_normal_z = min over texels of RN(dxdy/RN(sqrt(s))) is monotone in s: the wave keeps max(s) (NaN never wins, as in std::min) and k_tile_post_final takes the one square
//     root and division.  The reference's "mag < TOLERANCE: leave unnormalized" branch cannot be taken when sqrtf(dxdy*dxdy) >= TOLERANCE, which the host checks (else: simple path).
constexpr unsigned TP_THREADS = 256, TP_BAND_ROWS = 34, TP_ACC = 8; // acc: {-, -, bbox x1, y1, x2, y2, max |n|^2 bits, -}
constexpr float TP_EPS = 0x1p-14f;
__global__ __launch_bounds__(256) void k_tile_post_init(uint32_t *__restrict__ acc, uint32_t n) {
	uint32_t const i = blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n*TP_ACC) return;
	uint32_t const f = i % TP_ACC;
	acc[i] = (f < 2) ? 0xFFFFFFFFu : ((f < 4) ? 0x7FFFFFFFu : ((f < 6) ? 0x80000000u : 0u));
}
// the reference's texel, statement by statement (src/tiled_mesh.cpp:865-880)
__device__ __forceinline__ uint32_t tp_word_exact(float zc, float zr, float zd, float dxv, float dyv, float dxy) {
	float nv[3];
	tile_normal_v(zc, zr, zd, dxv, dyv, dxy, nv);
	uint32_t const b0 = (uint8_t)(127.0*((double)nv[0] + 1.0)), b1 = (uint8_t)(127.0*((double)nv[1] + 1.0)), b2 = (uint8_t)(127.0*((double)nv[2] + 1.0));
	return b0 | (b1 << 8) | (b2 << 16); // A = 0
}
// the short form: word and |n|^2; returns false when a byte is not certain
__device__ __forceinline__ bool tp_word_fast(float zc, float zr, float zd, float dxv, float dyv, float dxy, float c2, uint32_t flat_word, uint32_t &word, float &s) {
	float const n0 = dyv*(zc - zr), n1 = dxv*(zc - zd);
	s = n0*n0 + n1*n1 + c2; // the reference's sum, in its order; c2 = dxdy*dxdy
	float const r = rsq_approx(s);
	float const t0 = __builtin_fmaf(127.0f, n0*r, 127.0f), t1 = __builtin_fmaf(127.0f, n1*r, 127.0f), t2 = __builtin_fmaf(127.0f, dxy*r, 127.0f);
	float const lim = 0.5f - TP_EPS;
	bool const sure = (__builtin_fabsf(__builtin_amdgcn_fractf(t0) - 0.5f) < lim) & (__builtin_fabsf(__builtin_amdgcn_fractf(t1) - 0.5f) < lim) & (__builtin_fabsf(__builtin_amdgcn_fractf(t2) - 0.5f) < lim); // false for NaN
	bool const flat = (n0 == 0.0f) & (n1 == 0.0f);
	uint32_t const w = (uint32_t)t0 | ((uint32_t)t1 << 8) | ((uint32_t)t2 << 16);
	word = flat ? flat_word : w;
	return sure | flat;
}
__global__ __launch_bounds__(TP_THREADS) void k_tile_post(tile_ref_pod_t const *__restrict__ refs, float const *__restrict__ zvals, terra_tile_stats *__restrict__ stats,
	uint8_t *__restrict__ normals, uint32_t *__restrict__ acc, float wpz_max, float dxv, float dyv, float dxy, float c2, uint32_t flat_word)
{
	__shared__ __attribute__((aligned(16))) float tp_z[TP_BAND_ROWS*130];
	__shared__ uint32_t s_lo[4], s_hi[4], s_smax;
	__shared__ int s_bb[4];
	unsigned const t = blockIdx.x >> 2, yy = blockIdx.x & 3u, tid = threadIdx.x, zv = 130, stride = 129, bs = 32, row0 = yy*bs;
	tile_ref_pod_t const r = refs[t];
	int const x1 = r.tx*128, y1 = r.ty*128;
	{
		st_f4 const *src = (st_f4 const *)(zvals + (size_t)t*zv*zv + (size_t)row0*zv); // 67600 bytes per tile, 16640 per band: 16-byte aligned
		for (unsigned i = tid; i < TP_BAND_ROWS*zv/4; i += TP_THREADS) {((st_f4 *)tp_z)[i] = __builtin_nontemporal_load(src + i);} // read once (measured: 127.2 -> 125.5 us with the stores below)
	}
	if (tid < 4) {s_lo[tid] = f2ord(100.0f); s_hi[tid] = ~f2ord(-100.0f);} // folds start at szmin = FAR_DISTANCE, szmax = -FAR_DISTANCE
	if (tid == 0) {s_smax = 0u; s_bb[0] = x1 + 128; s_bb[1] = y1 + 128; s_bb[2] = x1; s_bb[3] = y1;} // water bbox starts denormalized
	__syncthreads();
	unsigned const w = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63; // the wave index as a scalar: rows, row tests and the water rows stay on the scalar unit
	unsigned const nrows = (yy == 3) ? bs + 1 : bs; // texel rows of this band: 32, the last band also row 128
	uint32_t *nout = normals ? (uint32_t *)(normals + (size_t)t*stride*stride*4) + (size_t)row0*stride : nullptr;
	bool const want_stats = stats != nullptr;
	// rows [ya, yb) of the band's 33 cell rows belong to this wave; lane = cell column x (first half) and 64 + x (second half)
	unsigned const ya = w*8, yb = (w == 3) ? bs + 1 : ya + 8;
	float loA = 100.0f, hiA = -100.0f, loB = 100.0f, hiB = -100.0f, smax = 0.0f;
	unsigned long long wetA = 0, wetB = 0; // columns with a cell under wpz_max
	int wy0 = 0x7FFFFFFF, wy1 = -1; // first / last such row (band coordinates)
	float const *zl = tp_z + lane;
	float cA = zl[ya*zv], cB = zl[ya*zv + 64];
	for (unsigned y = ya; y < yb; ++y) {
		float const *row = zl + y*zv;
		float const rA = row[1], rB = row[65], dA = row[zv], dB = row[zv + 64];
		if (want_stats) {
			loA = (cA < loA) ? cA : loA; hiA = (cA > hiA) ? cA : hiA; loB = (cB < loB) ? cB : loB; hiB = (cB > hiB) ? cB : hiB; // std::min / std::max: a NaN never wins
			unsigned long long const mA = __builtin_amdgcn_ballot_w64(cA < wpz_max), mB = __builtin_amdgcn_ballot_w64(cB < wpz_max);
			wetA |= mA; wetB |= mB;
			if (mA | mB) {wy0 = (wy0 < (int)y) ? wy0 : (int)y; wy1 = (int)y;}
		}
		if (nout && y < nrows) {
			uint32_t wA, wB; float sA, sB;
			bool const okA = tp_word_fast(cA, rA, dA, dxv, dyv, dxy, c2, flat_word, wA, sA), okB = tp_word_fast(cB, rB, dB, dxv, dyv, dxy, c2, flat_word, wB, sB);
			if (__builtin_amdgcn_ballot_w64(!(okA & okB)) != 0) {wA = tp_word_exact(cA, rA, dA, dxv, dyv, dxy); wB = tp_word_exact(cB, rB, dB, dxv, dyv, dxy);}
			__builtin_nontemporal_store(wA, &nout[y*stride + lane]); __builtin_nontemporal_store(wB, &nout[y*stride + lane + 64]); // written once, read by nobody here
			smax = __builtin_fmaxf(smax, __builtin_fmaxf(sA, sB));
		}
		cA = dA; cB = dB;
	}
	if (want_stats) { // sub-block xx covers columns [32*xx, 32*xx + 32]: the shared columns 32, 64, 96 count on both sides
		uint32_t la = f2ord(loA), ha = ~f2ord(hiA), lb = f2ord(loB), hb = ~f2ord(hiB);
		uint32_t const la0 = la, ha0 = ha, lb0 = lb, hb0 = hb;
#pragma unroll
		for (int off = 16; off > 0; off >>= 1) { // minima over each half of the wave
			uint32_t o;
			o = __shfl_xor(la, off, 64); la = (o < la) ? o : la; o = __shfl_xor(ha, off, 64); ha = (o < ha) ? o : ha;
			o = __shfl_xor(lb, off, 64); lb = (o < lb) ? o : lb; o = __shfl_xor(hb, off, 64); hb = (o < hb) ? o : hb;
		}
		if (lane == 0)  {atomicMin(&s_lo[0], la); atomicMin(&s_hi[0], ha); atomicMin(&s_lo[2], lb); atomicMin(&s_hi[2], hb); atomicMin(&s_lo[1], lb0); atomicMin(&s_hi[1], hb0);} // column 64 also closes sub-block 1
		if (lane == 32) {atomicMin(&s_lo[1], la); atomicMin(&s_hi[1], ha); atomicMin(&s_lo[3], lb); atomicMin(&s_hi[3], hb); atomicMin(&s_lo[0], la0); atomicMin(&s_hi[0], ha0); atomicMin(&s_lo[2], lb0); atomicMin(&s_hi[2], hb0);} // columns 32 and 96 close sub-blocks 0 and 2
	}
	int wx0 = 0x7FFFFFFF, wx1 = -1;
	if (wetA) {wx0 = __builtin_ctzll(wetA); wx1 = 63 - __builtin_clzll(wetA);}
	if (wetB) {int const f = 64 + __builtin_ctzll(wetB); wx0 = (wx0 < f) ? wx0 : f; wx1 = 127 - __builtin_clzll(wetB);}
	if (w == 1) { // column 128: a lane per row
		unsigned const y = lane;
		bool const in = y <= bs;
		float const *c = tp_z + (in ? y : 0u)*zv + 128;
		float const zc = c[0], zr = c[1], zd = c[zv];
		if (want_stats) {
			if (in && zc == zc) {uint32_t const o = f2ord(zc); atomicMin(&s_lo[3], o); atomicMin(&s_hi[3], ~o);}
			unsigned long long const m = __builtin_amdgcn_ballot_w64(in && zc < wpz_max);
			if (m) {
				int const f = __builtin_ctzll(m), l = 63 - __builtin_clzll(m);
				wx1 = 128; wx0 = (wx0 < 128) ? wx0 : 128; wy0 = (wy0 < f) ? wy0 : f; wy1 = (wy1 > l) ? wy1 : l;
			}
		}
		if (nout) {
			uint32_t wd; float s;
			bool const ok = tp_word_fast(zc, zr, zd, dxv, dyv, dxy, c2, flat_word, wd, s);
			if (__builtin_amdgcn_ballot_w64(!ok) != 0) {wd = tp_word_exact(zc, zr, zd, dxv, dyv, dxy);}
			if (y < nrows) {nout[y*stride + 128] = wd; smax = __builtin_fmaxf(smax, s);}
		}
	}
	if (want_stats && lane == 0 && wx1 >= 0) {atomicMin(&s_bb[0], x1 + wx0); atomicMin(&s_bb[1], y1 + (int)row0 + wy0); atomicMax(&s_bb[2], x1 + wx1); atomicMax(&s_bb[3], y1 + (int)row0 + wy1);}
	if (nout) { // s >= 0: positive floats order like their bit patterns
		uint32_t u; memcpy(&u, &smax, 4);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) {uint32_t const o = __shfl_xor(u, off, 64); u = (o > u) ? o : u;}
		if (lane == 0) {atomicMax(&s_smax, u);}
	}
	__syncthreads();
	if (tid == 0) { // the band's results; the tile's totals are folded by k_tile_post_final after this kernel (a device-wide fence per block, the
		// alternative, writes back the XCD's L2 every time on this chip: measured 3 x slower than the whole pass)
		uint32_t *a = acc + (size_t)t*TP_ACC;
		if (want_stats) {
			for (int k = 0; k < 4; ++k) {stats[t].sub_zmin[yy*4 + k] = ord2f(s_lo[k]); stats[t].sub_zmax[yy*4 + k] = ord2f(~s_hi[k]);}
			atomicMin((int *)&a[2], s_bb[0]); atomicMin((int *)&a[3], s_bb[1]); atomicMax((int *)&a[4], s_bb[2]); atomicMax((int *)&a[5], s_bb[3]);
		}
		if (nout) {atomicMax(&a[6], s_smax);}
	}
}
// one thread per tile: mzmin / mzmax fold the 16 sub-block ranges in the reference's order with its std::min / std::max (src/tiled_mesh.cpp:536-538), radius, water bbox, min_normal_z,
// after k_tile_post or k_tile_post_sized at the tile size S
__global__ __launch_bounds__(256) void k_tile_post_final(tile_ref_pod_t const *__restrict__ refs, uint32_t n, terra_tile_stats *__restrict__ stats, float *__restrict__ min_nz, uint32_t const *__restrict__ acc,
	float rad_c, float dxy, int have_normals, unsigned S)
{
	uint32_t const t = blockIdx.x*blockDim.x + threadIdx.x;
	if (t >= n) return;
	uint32_t const *a = acc + (size_t)t*TP_ACC;
	if (stats) {
		tile_ref_pod_t const r = refs[t];
		int const x1 = r.tx*(int)S, y1 = r.ty*(int)S;
		float mzmin = 100.0f, mzmax = -100.0f;
		for (int k = 0; k < 16; ++k) {mzmin = min_std(mzmin, stats[t].sub_zmin[k]); mzmax = max_std(mzmax, stats[t].sub_zmax[k]);}
		stats[t].mzmin = mzmin; stats[t].mzmax = mzmax;
		stats[t].radius = (float)(0.5*sqrt((double)(rad_c + (mzmax - mzmin)*(mzmax - mzmin))));
		stats[t].wx1 = imin((int)a[2], x1 + (int)S); stats[t].wy1 = imin((int)a[3], y1 + (int)S); stats[t].wx2 = imax((int)a[4], x1); stats[t].wy2 = imax((int)a[5], y1);
	}
	if (min_nz && have_normals) { // min_normal_z = min(1.0, min over texels of dxdy/mag) = dxdy / (the largest mag), both roundings monotone; a NaN never wins (src/tiled_mesh.cpp:874)
		float smax; uint32_t const u = a[6]; memcpy(&smax, &u, 4);
		float const nz = dxy/sqrtf(smax);
		min_nz[t] = (nz < 1.0f) ? nz : 1.0f;
	}
}

// ---- the post pass at any tile size S (zv = S + 2, stride = S + 1, block_size bs = zv/4): one block per (tile, sub-block row yy).  The block owns the
// stats rows [yy*bs, (yy + 1)*bs] (the shared row (yy + 1)*bs counts in both bands, as in the reference) and the texel rows [yy*bs, (yy + 1)*bs) -- the last band
// through row S.  A wave walks every TPS_WAVES-th row, a lane every 64th column; the rows are read through the caches (no LDS staging: a band of a 1024-cell tile
// is 1 MB).  The texel words are tp_word_fast / tp_word_exact's, by the same wave-uniform decision as k_tile_post; the tile's totals go through the same per-tile
// accumulators to k_tile_post_final.  It runs at S != 128 and at S = 128 where k_tile_post's 16-byte staging does not apply.
constexpr unsigned TPS_THREADS = 512, TPS_WAVES = TPS_THREADS/64;
__global__ __launch_bounds__(TPS_THREADS) void k_tile_post_sized(tile_ref_pod_t const *__restrict__ refs, float const *__restrict__ zvals, terra_tile_stats *__restrict__ stats,
	uint8_t *__restrict__ normals, uint32_t *__restrict__ acc, float wpz_max, float dxv, float dyv, float dxy, float c2, uint32_t flat_word, unsigned S)
{
	__shared__ uint32_t s_lo[4], s_hi[4], s_smax;
	__shared__ int s_bb[4];
	unsigned const t = blockIdx.x >> 2, yy = blockIdx.x & 3u, tid = threadIdx.x, zv = S + 2, stride = S + 1, bs = zv/4, lim = 4*bs;
	unsigned const srow0 = yy*bs, srow1 = (yy + 1)*bs;              // stats rows [srow0, srow1]
	unsigned const nrow0 = yy*bs, nrow1 = (yy == 3) ? stride : srow1; // texel rows [nrow0, nrow1)
	unsigned const rowN = (srow1 + 1 > nrow1) ? srow1 + 1 : nrow1;    // rows this band visits: [srow0, rowN)
	tile_ref_pod_t const r = refs[t];
	int const x1 = r.tx*(int)S, y1 = r.ty*(int)S;
	if (tid < 4) {s_lo[tid] = f2ord(100.0f); s_hi[tid] = ~f2ord(-100.0f);} // folds start at szmin = FAR_DISTANCE, szmax = -FAR_DISTANCE
	if (tid == 0) {s_smax = 0u; s_bb[0] = x1 + (int)S; s_bb[1] = y1 + (int)S; s_bb[2] = x1; s_bb[3] = y1;} // water bbox starts denormalized
	__syncthreads();
	unsigned const w = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
	float const *z = zvals + (size_t)t*zv*zv;
	uint32_t *nout = normals ? (uint32_t *)(normals + (size_t)t*stride*stride*4) : nullptr;
	bool const want_stats = stats != nullptr;
	uint32_t lo[4] = {f2ord(100.0f), f2ord(100.0f), f2ord(100.0f), f2ord(100.0f)}, hi[4] = {~f2ord(-100.0f), ~f2ord(-100.0f), ~f2ord(-100.0f), ~f2ord(-100.0f)};
	int wx0 = 0x7FFFFFFF, wx1 = -1, wy0 = 0x7FFFFFFF, wy1 = -1;
	float smax = 0.0f;
	for (unsigned y = srow0 + w; y < rowN; y += TPS_WAVES) { // (wave-uniform)
		float const *row = z + (size_t)y*zv;
		bool const srow = y <= srow1, nrow = nout && y >= nrow0 && y < nrow1;
		for (unsigned x0 = 0; x0 < zv; x0 += 64) {
			unsigned const x = x0 + lane;
			bool const in = x < zv;
			float const zc = row[in ? x : 0u];
			if (want_stats && srow) {
				if (in && x <= lim && zc == zc) { // sub-block xx covers columns [xx*bs, (xx + 1)*bs]: a column on a block border counts on both sides; a NaN never wins
					uint32_t const o = f2ord(zc);
#pragma unroll
					for (unsigned k = 0; k < 4; ++k) {
						if (x >= k*bs && x <= k*bs + bs) {lo[k] = (o < lo[k]) ? o : lo[k]; hi[k] = (~o < hi[k]) ? ~o : hi[k];}
					}
				}
				if (in && x <= lim && zc < wpz_max) {wx0 = (wx0 < (int)x) ? wx0 : (int)x; wx1 = (wx1 > (int)x) ? wx1 : (int)x; wy0 = (wy0 < (int)y) ? wy0 : (int)y; wy1 = (int)y;}
			}
			if (nrow && x0 < stride) { // (wave-uniform)
				bool const tx = x < stride;
				float const zr = row[tx ? x + 1 : 0u], zd = row[(tx ? x : 0u) + zv];
				uint32_t wd; float sv;
				bool const ok = tp_word_fast(zc, zr, zd, dxv, dyv, dxy, c2, flat_word, wd, sv);
				if (__builtin_amdgcn_ballot_w64(tx && !ok) != 0) {wd = tp_word_exact(zc, zr, zd, dxv, dyv, dxy);}
				if (tx) {__builtin_nontemporal_store(wd, &nout[(size_t)y*stride + x]); smax = __builtin_fmaxf(smax, sv);}
			}
		}
	}
	if (want_stats) {
#pragma unroll
		for (unsigned k = 0; k < 4; ++k) {uint32_t const a = wave_min_u32(lo[k]), b = wave_min_u32(hi[k]); if (lane == 0) {atomicMin(&s_lo[k], a); atomicMin(&s_hi[k], b);}}
		int const ax0 = wave_min_i32(wx0), ay0 = wave_min_i32(wy0), ax1 = -wave_min_i32(-wx1), ay1 = -wave_min_i32(-wy1);
		if (lane == 0 && ax1 >= 0) {atomicMin(&s_bb[0], x1 + ax0); atomicMin(&s_bb[1], y1 + ay0); atomicMax(&s_bb[2], x1 + ax1); atomicMax(&s_bb[3], y1 + ay1);}
	}
	if (nout) { // s >= 0: positive floats order like their bit patterns
		uint32_t u; memcpy(&u, &smax, 4);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) {uint32_t const o = __shfl_xor(u, off, 64); u = (o > u) ? o : u;}
		if (lane == 0) {atomicMax(&s_smax, u);}
	}
	__syncthreads();
	if (tid == 0) {
		uint32_t *a = acc + (size_t)t*TP_ACC;
		if (want_stats) {
			for (int k = 0; k < 4; ++k) {stats[t].sub_zmin[yy*4 + k] = ord2f(s_lo[k]); stats[t].sub_zmax[yy*4 + k] = ord2f(~s_hi[k]);}
			atomicMin((int *)&a[2], s_bb[0]); atomicMin((int *)&a[3], s_bb[1]); atomicMax((int *)&a[4], s_bb[2]); atomicMax((int *)&a[5], s_bb[3]);
		}
		if (nout) {atomicMax(&a[6], s_smax);}
	}
}

// ------------------------------------------------------------------ row f1: tile AO lighting (tile_t::calc_mesh_ao_lighting, src/tiled_mesh.cpp:634-659)
// One block = one band of AO_BAND texel rows of one tile (33: four bands cover the 129 rows; with 32 a fifth block staged 74 context rows for one texel row).  The context rows the rays of the band can reach are staged in LDS in two passes:
// rays going up or sideways need context rows [y0, y0 + band + 35], rays going down rows [y0 + 36, y0 + band + 71] (context coordinates =
// texel + 36) -- 68 rows x 201 floats = 54.7 KB each time, so two blocks share a CU.  A thread owns up to 17 texels and keeps their
// attenuation sums in registers across the passes.  Same integer sums as the one-thread-per-texel version (tile_ao_simple).
constexpr unsigned AO_BAND = 33, AO_CS = 201, AO_RL = 36, AO_TEX = 129, AO_THREADS = 256, AO_ROWS_W = (AO_BAND + 3)/4, AO_HALF = (AO_BAND + AO_RL + 1)/2;
// one ray, branch-free: the eight samples sit at fixed offsets 1,3,6,...,36 steps from the texel (immediate ds_read offsets after unrolling),
// are all requested before the first compare, and the first hit is selected backwards (hit at step s attenuates by 8 - s)
template<int DX, int DY> __device__ __forceinline__ unsigned ao_march(float const *s_base, float const (&zr)[8]) {
	float smp[8];
#pragma unroll
	for (int s = 0; s < 8; ++s) {int const off = (s + 1)*(s + 2)/2; smp[s] = s_base[off*(DY*(int)AO_CS + DX)];}
	unsigned att = 0;
#pragma unroll
	for (int s = 7; s >= 0; --s) {att = (smp[s] > zr[s]) ? (unsigned)(8 - s) : att;}
	return att;
}
// the rays of one pass from the texel at sb (pass 0: up and sideways, pass 1: down)
template<int PASS> __device__ __forceinline__ unsigned ao_rays(float const *sb, float z0, float dz) {
	float zr[8];
#pragma unroll
	for (int s = 0; s < 8; ++s) {z0 += dz; zr[s] = z0;} // every ray rises by dz per step: sequential float adds, as in the reference
	if (PASS == 0) {return ao_march<-1, -1>(sb, zr) + ao_march<0, -1>(sb, zr) + ao_march<1, -1>(sb, zr) + ao_march<-1, 0>(sb, zr) + ao_march<1, 0>(sb, zr);}
	return ao_march<-1, 1>(sb, zr) + ao_march<0, 1>(sb, zr) + ao_march<1, 1>(sb, zr);
}
__device__ __forceinline__ uint8_t ao_byte(unsigned atten) {float const ao_scale = (float)(1.0 - (double)((float)atten/(float)64)); return (uint8_t)(255.0*(double)ao_scale);}
// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2: xcd_ordered() renumbers the blocks so that an XCD walks a CONTIGUOUS range of logical blocks (a tile's
// four bands, whose staging passes overlap each other's rows, run on one XCD one after another).  (Measured equal for this kernel: its context rows come out of the
// infinity cache either way; kept because it is free.)
__device__ __forceinline__ unsigned xcd_ordered(unsigned b, unsigned nb) {
	unsigned const xcd = b & 7u, j = b >> 3, per = nb >> 3, rem = nb & 7u; // XCD k owns blocks k, k + 8, ...: per + (k < rem) of them
	return ((xcd < rem) ? xcd*(per + 1u) : rem*(per + 1u) + (xcd - rem)*per) + j;
}
// (Taking the tile's own zvals from `zvals` while staging, instead of the caller's copy pass into the context, was measured: the extra index work in the staging loop costs more
// than the 170 us copy kernel saves -- 1.95 vs 1.87 ms for the row.)
// The kernel is bound by its LDS reads (64 per texel).  A WAVE owns texel rows (every fourth row of the band); a lane is a column: x = lane and 64 + lane, column 128 is one
// extra pass with a lane per row (row stride 201 = 9 mod 32: distinct banks).  With texels dealt out linearly (p = tid + 256 k) a wave's 64 texels crossed a row end and
// the part behind the wrap met the part before it in the banks: half of the LDS cycles were bank conflicts (SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_LDS = 0.53).
// OWN: the context cells inside the tile are taken from zvals (the tile's own, possibly eroded / edited heights) instead of ctx while the context is staged.
template<bool OWN> __global__ __launch_bounds__(AO_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_tile_ao(float const *__restrict__ zvals, float const *__restrict__ ctx, uint8_t *__restrict__ ao, float dz) {
	extern __shared__ __attribute__((aligned(16))) float s_ao_ctx[];
	unsigned const lb = xcd_ordered(blockIdx.x, gridDim.x);
	unsigned const nbands = (AO_TEX + AO_BAND - 1)/AO_BAND, t = lb/nbands, band = lb % nbands, tid = threadIdx.x;
	unsigned const w = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
	unsigned const y0 = band*AO_BAND, rows = (AO_TEX - y0 < AO_BAND) ? AO_TEX - y0 : AO_BAND;
	float const *c = ctx + (size_t)t*AO_CS*AO_CS, *z = zvals + (size_t)t*130*130;
	uint8_t *out = ao + (size_t)t*AO_TEX*AO_TEX;
	unsigned attA[AO_ROWS_W], attB[AO_ROWS_W], attC = 0; // rows w, w + 4, ...: columns lane and 64 + lane; column 128 of row `lane` (wave 3, which has a row less than wave 0)
	float zA[AO_ROWS_W], zB[AO_ROWS_W], zC = 0.0f;
#pragma unroll
	for (unsigned i = 0; i < AO_ROWS_W; ++i) {
		unsigned const yl = w + 4*i;
		attA[i] = attB[i] = 0;
		float const *zr = z + (size_t)(y0 + ((yl < rows) ? yl : 0u))*130;
		zA[i] = zr[lane]; zB[i] = zr[64 + lane];
	}
	if (w == 3) {zC = z[(size_t)(y0 + ((lane < rows) ? lane : 0u))*130 + 128];}
	// Staging: a pass's rows (<= 69 x 201 floats), thread = context column (threads 201 .. 255 idle), the rows in two halves of <= 35 loads per thread, each half ALL in
	// flight before its first LDS store (as a plain copy loop, a few loads at a time between LDS stores, two blocks per CU kept ~8 KB in flight per CU: 775 -> 740 us).
	// By rows, which source a cell has (OWN) is one compare per row and one per thread.  Measured for 4096 tiles: linear staging (thread = element i, i + 256, ...) without OWN
	// 663 us + the 168 us copy pass it needs = 831; this form 763; linear staging with an index division per element for OWN: 2813 (its 55 unrolled divisions spill).
	unsigned const nrow = rows + AO_RL;
	bool const col_ok = tid < AO_CS, col_own = OWN && (tid - AO_RL) < 130u;
	for (int pass = 0; pass < 2; ++pass) {
		unsigned const row0 = pass ? y0 + AO_RL : y0;
#pragma unroll
		for (unsigned h = 0; h < 2; ++h) {
			float stg[AO_HALF];
#pragma unroll
			for (unsigned k = 0; k < AO_HALF; ++k) {
				unsigned const r = h*AO_HALF + k, gr = row0 + r;
				bool const ok = col_ok && r < nrow;
				float const *p = c + (size_t)(ok ? gr : 0u)*AO_CS + (col_ok ? tid : 0u);
				if (OWN) {bool const in = col_own && (gr - AO_RL) < 130u && ok; p = in ? z + (size_t)(gr - AO_RL)*130 + (tid - AO_RL) : p;}
				stg[k] = *p;
			}
			if (h == 0) {__syncthreads();} // everybody is done with the previous pass's rows
#pragma unroll
			for (unsigned k = 0; k < AO_HALF; ++k) {unsigned const r = h*AO_HALF + k; if (col_ok && r < nrow) {s_ao_ctx[r*AO_CS + tid] = stg[k];}}
		}
		__syncthreads();
		unsigned const lrow = pass ? 0u : AO_RL; // LDS row of the band's first texel row
#pragma unroll
		for (unsigned i = 0; i < AO_ROWS_W; ++i) {
			unsigned const yl = w + 4*i;
			if (yl >= rows) break; // (wave-uniform)
			float const *sb = s_ao_ctx + (yl + lrow)*AO_CS + AO_RL + lane; // the texel itself in the staged context
			if (pass == 0) {attA[i] += ao_rays<0>(sb, zA[i], dz); attB[i] += ao_rays<0>(sb + 64, zB[i], dz);}
			else           {attA[i] += ao_rays<1>(sb, zA[i], dz); attB[i] += ao_rays<1>(sb + 64, zB[i], dz);}
		}
		if (w == 3) {
			float const *sb = s_ao_ctx + (((lane < rows) ? lane : 0u) + lrow)*AO_CS + AO_RL + 128;
			attC += (pass == 0) ? ao_rays<0>(sb, zC, dz) : ao_rays<1>(sb, zC, dz);
		}
	}
#pragma unroll
	for (unsigned i = 0; i < AO_ROWS_W; ++i) {
		unsigned const yl = w + 4*i;
		if (yl >= rows) break;
		uint8_t *o = out + (size_t)(y0 + yl)*AO_TEX;
		o[lane] = ao_byte(attA[i]); o[64 + lane] = ao_byte(attB[i]);
	}
	if (w == 3 && lane < rows) {out[(size_t)(y0 + lane)*AO_TEX + 128] = ao_byte(attC);}
}

// ---- the whole tile's context in LDS (k_tile_ao_tile): one block of 16 waves per tile, the 201 x 201 context staged ONCE -- 201 rows x 202 floats = 162 408 of the CU's
// 163 840 bytes -- instead of 68 rows twice per 33-row band (2.7 x 201 rows per tile, and the staging of a band was as long as its rays).  A lane owns the texel PAIR
// (2 lane, 2 lane + 1) of a row, a wave a row: the two texels' samples of a ray step are neighbours in LDS, one 8-byte read (256 B per clock against the 4-byte read's 128)
// where the step's x offset is even; where it is odd the pair straddles two aligned 8-byte words and takes both (the 4-byte reads of a lane pair would be 2-way bank
// conflicts at a stride of two dwords).  Per texel pair 40 + 2 x 24 eight-byte reads = 176 LDS cycles instead of 256, four waves per SIMD instead of two to hide them;
// the compares (2 instructions per sample) are what is left.  Column 128 is a lane per row.  Same integer sums as k_tile_ao / tile_ao_simple at S = 128.
constexpr unsigned AOT_THREADS = 1024, AOT_S = 202, AOT_LDS = AO_CS*AOT_S*4;
typedef float ao_f2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) float ao_lds_f;   // (the volatile reads below must know they are LDS reads: a generic volatile pointer becomes a flat load)
typedef __attribute__((address_space(3))) ao_f2 ao_lds_f2;
// Half a ray of a texel pair (steps 4 H .. 4 H + 3): the unit the row loop keeps two of in flight.  sb: the sample 36 steps up and left of the pair's first texel -- an even
// dword: every offset below is non-negative and known at compile time.  volatile LDS reads: each stays ONE ds_read_b64 -- the compiler otherwise pairs them into ds_read2_b64,
// half the rate per byte, and narrows the odd case to 4-byte reads -- and they keep their place between the `pins` of ao_pair_hits4 (an empty asm volatile on the ray's sums):
// all eight rays' reads moved to the front spill at 128 registers.  (One whole ray in flight and two half rays in flight measure the same, 382 / 380 us: with four waves per
// SIMD the LDS latency is hidden either way.)
template<int DX, int DY, int H> __device__ __forceinline__ void ao_pair_load4(ao_lds_f const *sb, float (&a)[4], float (&b)[4]) {
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		int const s = 4*H + i, T = (s + 1)*(s + 2)/2, off = ((int)AO_RL + T*DY)*(int)AOT_S + (int)AO_RL + T*DX;
		if ((off & 1) == 0) {ao_f2 const v = *(ao_lds_f2 const volatile *)(sb + off); a[i] = v.x; b[i] = v.y;}
		else {ao_f2 const u = *(ao_lds_f2 const volatile *)(sb + off - 1), v = *(ao_lds_f2 const volatile *)(sb + off + 1); a[i] = u.y; b[i] = v.x;}
	}
}
template<int H> __device__ __forceinline__ void ao_pair_hits4(float const (&a)[4], float const (&b)[4], float const (&zr0)[8], float const (&zr1)[8], unsigned &r0, unsigned &r1) {
#pragma unroll
	for (int i = 3; i >= 0; --i) {int const s = 4*H + i; r0 = (a[i] > zr0[s]) ? (unsigned)(8 - s) : r0; r1 = (b[i] > zr1[s]) ? (unsigned)(8 - s) : r1;}
	asm volatile("" : "+v"(r0), "+v"(r1)); // the pin
}
template<int DX, int DY> __device__ __forceinline__ unsigned ao_march_one(float const *sb, float const (&zr)[8]) { // one texel, context rows AOT_S apart
	float smp[8];
#pragma unroll
	for (int s = 0; s < 8; ++s) {int const T = (s + 1)*(s + 2)/2; smp[s] = sb[((int)AO_RL + T*DY)*(int)AOT_S + (int)AO_RL + T*DX];}
	unsigned att = 0;
#pragma unroll
	for (int s = 7; s >= 0; --s) {att = (smp[s] > zr[s]) ? (unsigned)(8 - s) : att;}
	return att;
}
// Staging: thread = context column, the block's four 256-thread quarters take every fourth row: 51 values per thread.  They are LOADED into registers while the tile before is
// still being computed (the block is persistent: tiles blockIdx.x, + gridDim.x, ...) and stored to LDS when its rays are done: a CU holds one workgroup (the LDS is full), so
// nobody else would hide the loads.  Which source a cell has (OWN: the tile's own heights inside the tile) is a scalar test per row and a per-thread base + stride.
constexpr unsigned AOT_STG = 51;
template<bool OWN> __device__ __forceinline__ void aot_stage_load(float const *__restrict__ zvals, float const *__restrict__ ctx, unsigned t, unsigned col, unsigned rq, float (&stg)[AOT_STG]) {
	float const *c = ctx + (size_t)t*AO_CS*AO_CS, *z = zvals + (size_t)t*130*130;
	bool const col_ok = col < AO_CS, col_own = OWN && (col - AO_RL) < 130u;
	float const *base_out = c + (col_ok ? col : 0u);
	float const *base_in = col_own ? z + (col - AO_RL) - (size_t)AO_RL*130 : base_out; // centre rows: r*130 from here is row r - 36 of the tile
	unsigned const stride_in = col_own ? 130u : AO_CS;
	// rows rq + 4k: for k = 9 .. 40 they lie inside the tile whatever rq is (36 .. 163 + rq), for k = 41 (164 .. 167) it depends on rq, the others never do -- no
	// per-element choice between two pointers but for that one
#pragma unroll
	for (unsigned k = 0; k < AOT_STG; ++k) {
		unsigned const r = rq + 4u*k, rr = (r < AO_CS) ? r : 0u; // (scalar: rq is wave-uniform)
		float const *p;
		if (OWN && k >= 9 && k <= 40) {p = base_in + __umul24(rr, stride_in);}
		else if (OWN && k == 41) {p = ((rr - AO_RL) < 130u) ? base_in + __umul24(rr, stride_in) : base_out + rr*AO_CS;}
		else {p = base_out + rr*AO_CS;}
		stg[k] = *p;
	}
}
__device__ __forceinline__ void aot_stage_store(float *s, unsigned col, unsigned rq, float const (&stg)[AOT_STG]) {
	if (col >= AO_CS) return;
#pragma unroll
	for (unsigned k = 0; k < AOT_STG; ++k) {unsigned const r = rq + 4u*k; if (r < AO_CS) {s[r*AOT_S + col] = stg[k];}}
}
template<bool OWN> __global__ __launch_bounds__(AOT_THREADS) void k_tile_ao_tile(float const *__restrict__ zvals, float const *__restrict__ ctx, uint8_t *__restrict__ ao, float dz, unsigned n) {
	extern __shared__ __attribute__((aligned(16))) float s_aot[];
	__shared__ unsigned s_item;
	unsigned const tid = threadIdx.x, lane = tid & 63u, col = tid & 255u;
	unsigned const w = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), rq = w >> 2;
	float stg[AOT_STG];
	if (blockIdx.x < n) {aot_stage_load<OWN>(zvals, ctx, blockIdx.x, col, rq, stg);}
	for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
	float const *z = zvals + (size_t)t*130*130;
	uint8_t *out = ao + (size_t)t*AO_TEX*AO_TEX;
	aot_stage_store(s_aot, col, rq, stg);
	if (tid == 0) {s_item = 0u;}
	__syncthreads();
	// in flight behind this tile's rays -- which then must not wait for a global load of their own (a wave's loads return in order): with OWN the texels' heights are the
	// centre of the staged context; without, they are the caller's zvals (not the context's centre) and the next tile is loaded after the rays instead
	if (OWN && t + gridDim.x < n) {aot_stage_load<OWN>(zvals, ctx, t + gridDim.x, col, rq, stg);}
	for (;;) { // work items of the tile, dealt out by a counter in LDS (a fixed deal leaves one wave with a ninth row while the others wait at the barrier): 129 rows of 64 texel pairs, then column 128 in three pieces
		unsigned item = 0;
		if (lane == 0) {item = atomicAdd(&s_item, 1u);}
		item = (unsigned)__builtin_amdgcn_readfirstlane((int)item);
		if (item >= AO_TEX) {
			if (item >= AO_TEX + 3u) break;
			unsigned const y = (item - AO_TEX)*64u + lane; // column 128: a lane per row
			if (y < AO_TEX) {
				float z0 = OWN ? s_aot[(y + AO_RL)*AOT_S + AO_RL + 128] : z[(size_t)y*130 + 128];
				float zr[8];
#pragma unroll
				for (int s = 0; s < 8; ++s) {z0 += dz; zr[s] = z0;}
				float const *sb = s_aot + y*AOT_S + 128;
				unsigned const att = ao_march_one<-1, -1>(sb, zr) + ao_march_one<0, -1>(sb, zr) + ao_march_one<1, -1>(sb, zr) + ao_march_one<-1, 0>(sb, zr) + ao_march_one<1, 0>(sb, zr)
					+ ao_march_one<-1, 1>(sb, zr) + ao_march_one<0, 1>(sb, zr) + ao_march_one<1, 1>(sb, zr);
				out[(size_t)y*AO_TEX + 128] = ao_byte(att);
			}
			continue;
		}
		unsigned const y = item, x0 = 2u*lane;
		float z0, z1;
		if (OWN) {ao_f2 const v = *(ao_f2 const *)(s_aot + (y + AO_RL)*AOT_S + AO_RL + x0); z0 = v.x; z1 = v.y;}
		else {z0 = z[(size_t)y*130 + x0]; z1 = z[(size_t)y*130 + x0 + 1];}
		float zr0[8], zr1[8];
#pragma unroll
		for (int s = 0; s < 8; ++s) {z0 += dz; z1 += dz; zr0[s] = z0; zr1[s] = z1;} // every ray rises by dz per step: sequential float adds, as in the reference
		ao_lds_f const *sb = (ao_lds_f const *)s_aot + y*AOT_S + x0;
		unsigned a0 = 0, a1 = 0;
		// two HALF rays in flight: the far half (steps 4 .. 7, scanned first: the nearest hit wins) of a ray is loaded behind the near half of the ray before it
		float pa[4], pb[4], qa[4], qb[4];
		unsigned r0 = 0, r1 = 0;
#define TERRA_AO_RAY(DX, DY, NEXT) ao_pair_load4<DX, DY, 0>(sb, qa, qb); ao_pair_hits4<1>(pa, pb, zr0, zr1, r0, r1); NEXT; ao_pair_hits4<0>(qa, qb, zr0, zr1, r0, r1); a0 += r0; a1 += r1; r0 = r1 = 0;
		ao_pair_load4<-1, -1, 1>(sb, pa, pb);
		TERRA_AO_RAY(-1, -1, (ao_pair_load4< 0, -1, 1>(sb, pa, pb)))
		TERRA_AO_RAY( 0, -1, (ao_pair_load4< 1, -1, 1>(sb, pa, pb)))
		TERRA_AO_RAY( 1, -1, (ao_pair_load4<-1,  0, 1>(sb, pa, pb)))
		TERRA_AO_RAY(-1,  0, (ao_pair_load4< 1,  0, 1>(sb, pa, pb)))
		TERRA_AO_RAY( 1,  0, (ao_pair_load4<-1,  1, 1>(sb, pa, pb)))
		TERRA_AO_RAY(-1,  1, (ao_pair_load4< 0,  1, 1>(sb, pa, pb)))
		TERRA_AO_RAY( 0,  1, (ao_pair_load4< 1,  1, 1>(sb, pa, pb)))
		TERRA_AO_RAY( 1,  1, (void)0)
#undef TERRA_AO_RAY
		uint8_t *o = out + (size_t)y*AO_TEX + x0;
		o[0] = ao_byte(a0); o[1] = ao_byte(a1);
	}
	if (!OWN && t + gridDim.x < n) {aot_stage_load<OWN>(zvals, ctx, t + gridDim.x, col, rq, stg);}
	__syncthreads(); // (the next tile's staging overwrites the context)
	}
}

// ------------------------------------------------------------------ row f2: mesh shadows, one launch per dependency level
// An outgoing edge height travels between tiles as (dependency order << 32 | float bits) under a 64-bit max; 0 = nothing arrived (MESH_MIN_Z).
constexpr unsigned long long SHADOW_EDGE_PUB = 1ull << 63; // (k_tile_shadows_flow) this word of a finished tile's edge array has been published
struct shadow_edge_t {
	__device__ static float decode(unsigned long long v) {if (v == 0) return -1.0E6f; uint32_t const b = (uint32_t)(v & 0xFFFFFFFFull); float f; memcpy(&f, &b, 4); return f;}
	__device__ static unsigned long long pack(uint32_t order, float v) {uint32_t b; memcpy(&b, &v, 4); return ((unsigned long long)order << 32) | b;}
};
constexpr unsigned SH_LEVEL_THREADS = 576; // 9 waves: all 520 sweeps of a tile in one round

// One dependency level of the tile mesh shadows: one block per tile of the level, one thread per sweep.  A sweep is a chain of ~260 dependent steps, so
// what a step costs is latency: everything it reads AND writes lives in LDS -- the tile's heights, the two incoming edge arrays (decoded), the tile's
// shadow bytes and its two outgoing edge arrays (ordered 64-bit max, as in the other variants).  The walk touches no global memory at all; with the
// per-step shadow atomics going to L2 a step took ~270 ns (a wave's atomics drain one after another), with global reads in the loop it also stalled on
// `s_waitcnt vmcnt(0)` every step.  The block copies its results out at the end: it is the only writer of its tile's mask and edges.
struct shadow_lds_in_t {
	float const *ix, *iy; // LDS: decoded incoming edge heights (MESH_MIN_Z where there is none)
	__device__ float x(int i) const {return ix[i];}
	__device__ float y(int i) const {return iy[i];}
};
struct shadow_lds_out_t {
	uint8_t *sm; unsigned long long *ox, *oy; int xsize; // all LDS
	int spare_b; unsigned long long *spare_q; // this lane's spare byte (an index into sm) and spare 8-byte slot: where the branch-free steps write when they have nothing to write
	__device__ void shadow(int x, int y) {sm[y*xsize + x] = 0x02;} // MESH_SHADOW: every writer stores the same byte
	__device__ void shadow_at(int idx) {sm[idx] = 0x02;}            // (the mask and the heights have the same row length)
	__device__ void shadow_if(bool sh, int idx) {sm[sh ? idx : spare_b] = 0x02;} // branch-free: a selected address instead of a skipped store
	__device__ void out_x_if(bool on, int i, unsigned long long v) {atomicMax(on ? &ox[i] : spare_q, v);}
	__device__ void out_y_if(bool on, int i, unsigned long long v) {atomicMax(on ? &oy[i] : spare_q, v);}
	__device__ void out_x(int i, uint32_t order, float v) {atomicMax(&ox[i], shadow_edge_t::pack(order, v));}
	__device__ void out_y(int i, uint32_t order, float v) {atomicMax(&oy[i], shadow_edge_t::pack(order, v));}
};
// The sweep of the LDS kernels (same arithmetic as shadow_trace_path, which the per-thread cross-check kernels and the emulator keep): a tile is a chain of <= 131 dependent
// steps per sweep and the batch a chain of tiles, so what a step costs is what the row costs.  Cut out of the step: the incoming edge heights are looked at only while a sweep
// is still on its first column / row (x and y move away from xa / ya monotonically: a wave-uniform branch that is not taken after the first steps), the outgoing ones only
// where a shadowed step sits on the last column / row; the cell index and the coordinate along the light's dominant axis are carried instead of multiplied out; the last
// unshadowed height is carried as the double it is used as; the rest of the step is selects, not branches.
__device__ __forceinline__ int shadow_wave_max(int v) {for (int off = 32; off; off >>= 1) {v = max(v, __shfl_xor(v, off));} return __builtin_amdgcn_readfirstlane(v);} // (all 64 lanes active; the result in a scalar register: loop bounds)
// A lane's sweep and its wave's phases: the same for every tile of a batch (the light and the tile geometry are), so a persistent block makes it once, not per tile (the line
// clip with its divisions and three wave reductions were ~10 % of a tile's time).  Called by every lane of a wave, sweep or not (p >= npaths: none): the phases are the wave's.
struct shadow_plan_t {shadow_path_t w; unsigned p; bool has; int n1, e, lmax;};
__device__ __forceinline__ shadow_plan_t shadow_sweep_plan(shadow_consts_t const &c, unsigned p, unsigned npaths) {
	shadow_plan_t pl;
	pl.w = shadow_path_t{0, 0, 0, 0, -1, 0, 0, 0, 0, 0}; pl.p = p;
	pl.has = p < npaths && shadow_path_setup(c, p, pl.w);
	if (!pl.has) {pl.w.longest = -1;}
	// x and y move away from xa / ya and toward xb / yb monotonically, and where a walk leaves its first column / row and reaches its last is known in closed form
	// (shadow_path_zones): three phases with wave-uniform trip counts -- until the last lane has left its first zone; the middle, which no lane's edge words can touch and whose
	// cells lie strictly inside the tile; from where the first lane reaches its last zone
	int first_end = 0, last_begin = 0x7FFFFFFF;
	if (pl.has) {shadow_path_zones(pl.w.longest, pl.w.shortest, first_end, last_begin);}
	pl.n1 = shadow_wave_max(first_end); pl.e = -shadow_wave_max(-last_begin); pl.lmax = shadow_wave_max(pl.w.longest);
	return pl;
}
template<class IN, class OUT> __device__ __forceinline__ void shadow_trace_path_lean(shadow_consts_t const &c, float const *mh, IN const &in, shadow_plan_t const &pl, OUT &out) {
	if (!pl.has) return;
	shadow_path_t const &w = pl.w; unsigned const p = pl.p;
	int const xa = w.xa, ya = w.ya, xb = w.xb, yb = w.yb, longest = w.longest, shortest = w.shortest, dx1 = w.dx1, dy1 = w.dy1, dx2 = w.dx2, dy2 = w.dy2;
	bool const dim = (fabsf(c.dirx) < fabsf(c.diry));
	double const dir_ratio = (double)(c.dirz/(dim ? c.diry : c.dirx));
	float const org_d = dim ? -c.Y_SCENE_SIZE : -c.X_SCENE_SIZE, step_d = dim ? c.DY_VAL : c.DX_VAL;
	int x = xa, y = ya, numerator = longest >> 1;
	int const xs = c.xsize, di1 = dy1*xs + dx1, di2 = dy2*xs + dx2, dc1 = dim ? dy1 : dx1, dc2 = dim ? dy2 : dx2, last_cell = xs*c.ysize - 1;
	int idx = y*xs + x, cc = dim ? y : x, i = 0; // the cell, its coordinate along the dominant light axis, the step
	float cur_d; double cur_zd; // the caster (the last unshadowed point: its coordinate along the light's axis, its height)
	float nxt_z = mh[min(max(idx, 0), last_cell)]; // the height of the cell a step works on is read one step ahead: its address does not depend on the shadow state
	// One step of the first or the last phase (on the first / last column or row of the walk: edge heights come in / go out, the cell may lie just outside the tile), straight-line:
	// lanes whose sweep has ended and cells outside the tile are folded into `valid`, `not yet inited` into the caster (a caster at -inf shadows nothing: the step then takes the
	// cell as the new caster, which is what the reference's `inited` does), the incoming edge heights are read whether needed or not and selected, the outgoing ones go through LDS
	// atomics on selected addresses (the lane's spare slot when the step has nothing to hand on).  EDGE_IN: some lane may still be on its first column / row.
	cur_d = 0.0f; cur_zd = -(double)INFINITY;
	auto zone_step = [&](auto in_tag) {
		constexpr bool EDGE_IN = decltype(in_tag)::value;
		int const x0 = x, y0 = y, idx0 = idx, cc0 = cc, i0 = i;
		float const pt_z = nxt_z;
		double const pt_zd = (double)pt_z;
		numerator += shortest;
		bool const both = numerator >= longest;
		numerator -= both ? longest : 0;
		x += both ? dx1 : dx2; y += both ? dy1 : dy2; idx += both ? di1 : di2; cc += both ? dc1 : dc2; ++i;
		nxt_z = mh[min(max(idx, 0), last_cell)];
		bool const valid = i0 <= longest && (unsigned)x0 < (unsigned)c.xsize && (unsigned)y0 < (unsigned)c.ysize;
		float const pt_d = org_d + step_d*(float)cc0;
		if (EDGE_IN) {
			float const siy = in.y(min(max(y0, 0), c.ysize - 1)), six = in.x(min(max(x0, 0), c.xsize - 1));
			bool const take_y = valid && x0 == xa && siy > -1.0E6f, take_x = valid && !take_y && y0 == ya && six > -1.0E6f;
			float const siv = take_y ? siy : six;
			cur_d = (take_y || take_x) ? pt_d : cur_d; cur_zd = (take_y || take_x) ? (double)siv : cur_zd;
		}
		float const shadow_z = (float)((double)(pt_d - cur_d)*dir_ratio + cur_zd);
		bool const sh = valid && shadow_z > pt_z;
		out.shadow_if(sh, idx0);
		unsigned long long const word = shadow_edge_t::pack(p*1024u + (uint32_t)i0 + 1u, shadow_z);
		out.out_y_if(sh && x0 == xb, y0, word);
		out.out_x_if(sh && y0 == yb, x0, word);
		bool const upd = valid && !sh;
		cur_d = upd ? pt_d : cur_d; cur_zd = upd ? pt_zd : cur_zd;
	};
	int const n1 = pl.n1, e = pl.e, lmax = pl.lmax; // the wave's phases (shadow_sweep_plan): the middle has no loop test, no zone test, no bounds test per step -- the wave's lanes all have a step to make
	int k = 0;
	for (; k < n1; ++k) {zone_step(std::true_type());}
	if (k < e) { // the middle: straight-line steps -- no x / y (recomputed behind it), no bounds, `not yet inited` folded into the caster (a caster at -inf shadows nothing), the
		// shadow byte stored with a selected address instead of a branch
		int const k0 = k;
		for (; k < e; ++k) {
			int const idx0 = idx, cc0 = cc;
			float const pt_z = nxt_z;
			double const pt_zd = (double)pt_z;
			numerator += shortest;
			bool const both = numerator >= longest;
			numerator -= both ? longest : 0;
			idx += both ? di1 : di2; cc += both ? dc1 : dc2;
			nxt_z = mh[idx]; // (a walk's cell: at worst one column / row past the tile, still this block's LDS)
			float const pt_d = org_d + step_d*(float)cc0;
			float const shadow_z = (float)((double)(pt_d - cur_d)*dir_ratio + cur_zd);
			bool const sh = shadow_z > pt_z;
			out.shadow_if(sh, idx0);
			cur_d = sh ? cur_d : pt_d; cur_zd = sh ? cur_zd : pt_zd;
		}
		i += k - k0;
		int const m = (longest > 0) ? ((longest >> 1) + i*shortest)/longest : 0; // how often the minor coordinate has moved in i steps
		x = xa + dx2*i + (dx1 - dx2)*m; y = ya + dy2*i + (dy1 - dy2)*m;
	}
	for (; k <= lmax; ++k) {zone_step(std::false_type());}
}
struct shadow_lanes_t {uint16_t path[SH_LEVEL_THREADS];}; // which sweep a lane takes (shadow_lane_order), 0xFFFF = none; travels as a kernel argument
// LDS of the shadow kernels: the shadow bytes FIRST (the sweep's byte stores and height reads then carry their array's offset as the instruction's 16-bit immediate: behind
// 70 KB of heights the mask's offset did not fit and cost an addition per step: 1.71 -> 1.65 ms), a spare byte per lane behind them, the heights (16-byte aligned), the
// decoded incoming edges, the outgoing edge words, a spare 8-byte slot per lane.  (The cell's coordinate along the light's axis from a 132-entry table in LDS instead of a
// conversion, a multiplication and an addition per step was measured and LOST, 1.65 -> 1.72 ms: a second LDS read per step to wait for.)
constexpr unsigned SH_SPARE_B = 130*130, SH_OFF_MH = (130*130 + SH_LEVEL_THREADS + 15)/16*16; // byte offsets: the lanes' spare bytes, the heights
constexpr unsigned SH_LEVEL_LDS = SH_OFF_MH + 130*130*4 + 2*130*4 + 2*130*8 + SH_LEVEL_THREADS*8; // = 17 488 + 67 600 + 1 040 + 2 080 + 4 608 = 92 816 bytes
__global__ __launch_bounds__(SH_LEVEL_THREADS) void k_tile_shadows_level(shadow_consts_t c, uint32_t n, uint32_t const *__restrict__ order, int32_t const *__restrict__ adj,
	float const *__restrict__ zvals, unsigned long long *out, uint8_t *smask, uint32_t npaths, shadow_lanes_t lanes)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t s_sh_raw[];
	unsigned const zv = 130, tid = threadIdx.x;
	uint32_t const t = order[blockIdx.x];
	int32_t const ax = adj[2*t], ay = adj[2*t + 1];
	float const *z = zvals + (size_t)t*zv*zv;
	uint32_t *s_mask = (uint32_t *)s_sh_raw;
	float *s_sh_mh = (float *)(s_sh_raw + SH_OFF_MH), *s_in = s_sh_mh + zv*zv;
	unsigned long long *s_out = (unsigned long long *)(s_in + 2*zv); // (8-byte aligned: 17 488 + 67 600 + 1 040)
	if (((uintptr_t)z & 15) == 0) {for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {((float4 *)s_sh_mh)[i] = ((float4 const *)z)[i];}} // 67 600 bytes per tile
	else {for (unsigned i = tid; i < zv*zv; i += SH_LEVEL_THREADS) {s_sh_mh[i] = z[i];}}
	for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {s_mask[i] = 0u;}
	if (tid < 2*zv) { // in.x(i) = the y-neighbour's out_x, in.y(i) = the x-neighbour's out_y (src/tiled_mesh.cpp:676-687); earlier levels have finished
		bool const isx = tid < zv; unsigned const i = isx ? tid : tid - zv; int32_t const a = isx ? ay : ax;
		s_in[tid] = (a >= 0) ? shadow_edge_t::decode(out[((size_t)(isx ? 0 : 1)*n + a)*zv + i]) : -1.0E6f;
		s_out[tid] = 0ull; // 0 = never written
	}
	__syncthreads();
	shadow_lds_in_t const in{s_in, s_in + zv};
	shadow_lds_out_t o{(uint8_t *)s_mask, s_out, s_out + zv, (int)zv, (int)(SH_SPARE_B + tid), s_out + 2*zv + tid};
	shadow_trace_path_lean(c, s_sh_mh, in, shadow_sweep_plan(c, lanes.path[tid], npaths), o);
	__syncthreads();
	uint32_t *gm = (uint32_t *)(smask + (size_t)t*zv*zv); // 16 900 bytes per tile: word-aligned
	for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {gm[i] = s_mask[i] | c.mask_fill;} // plain stores: nobody else writes this tile's mask
	if (tid < 2*zv) {
		unsigned long long const v = s_out[tid];
		if (v) {out[((size_t)((tid < zv) ? 0 : 1)*n + t)*zv + ((tid < zv) ? tid : tid - zv)] = v;}
	}
}

// The whole batch as ONE dataflow launch.  A tile needs the edge arrays of its two neighbours toward the light (src/tiled_mesh.cpp:664-692) and nothing else: a launch per
// dependency LEVEL (127 of them for a 64 x 64 batch) makes every tile wait for the slowest tile of the level before -- and for two launch gaps.  Here blocks take tiles from
// a queue in level order (an atomic ticket; `order` lists a tile's dependencies before it), stage the tile's heights, and only then wait for the upstream tiles' `done`
// words.  Progress: a waiting block holds a ticket, the tile it waits for has a LOWER ticket and was therefore taken by a block that is running -- whatever the grid size and
// however many blocks are resident; the lowest ticket in flight never waits.
// Hand-off between workgroups (they sit on other CUs, maybe other XCDs: neither their L1 nor their L2 is ours): the edge words ARE the flags.  A finished tile stores ALL
// 260 words of its two edge arrays as 8-byte agent-scope (write-through) stores with SHADOW_EDGE_PUB set -- `nothing arrived at this cell` is published as 0 | PUB -- and a
// consumer lane polls exactly the word it needs with relaxed agent-scope loads until the bit is there: no flag word, no fence, no second round trip (a `done` word per tile
// with a release / acquire pair was measured first: ~5 us more per tile of a 127-tile chain).  While a tile is far from its turn only ONE lane per upstream tile polls,
// sleeping in between; the 260 lanes join when that lane has seen the first word.  `ticket` is zeroed by the caller per call, the edge arrays too (no stale PUB bit);
// the virtual halo slots (index >= ntiles) were written before the launch and are read without polling.
__global__ __launch_bounds__(SH_LEVEL_THREADS) void k_tile_shadows_flow(shadow_consts_t c, uint32_t n, uint32_t ntiles, uint32_t const *__restrict__ order, int32_t const *__restrict__ adj,
	float const *__restrict__ zvals, unsigned long long *out, uint8_t *smask, uint32_t npaths, uint32_t *ticket, shadow_lanes_t lanes)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t s_sh_raw[];
	__shared__ uint32_t s_ticket;
	unsigned const zv = 130, tid = threadIdx.x;
	uint32_t *s_mask = (uint32_t *)s_sh_raw;
	float *s_sh_mh = (float *)(s_sh_raw + SH_OFF_MH), *s_in = s_sh_mh + zv*zv;
	unsigned long long *s_out = (unsigned long long *)(s_in + 2*zv);
	shadow_plan_t const plan = shadow_sweep_plan(c, lanes.path[tid], npaths); // (the same for every tile)
	for (;;) {
		if (tid == 0) {s_ticket = atomicAdd(ticket, 1u);}
		__syncthreads();
		uint32_t const k = s_ticket;
		if (k >= ntiles) return; // (block-uniform)
		uint32_t const t = order[k];
		int32_t const ax = adj[2*t], ay = adj[2*t + 1];
		float const *z = zvals + (size_t)t*zv*zv;
		// everything that does not depend on the neighbours first
		if (((uintptr_t)z & 15) == 0) {for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {((float4 *)s_sh_mh)[i] = ((float4 const *)z)[i];}}
		else {for (unsigned i = tid; i < zv*zv; i += SH_LEVEL_THREADS) {s_sh_mh[i] = z[i];}}
		for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {s_mask[i] = 0u;}
		if (tid < 64) { // far from this tile's turn: lane 0 watches the x neighbour's first word, lane 1 the y neighbour's
			int32_t const a = (tid == 0) ? ax : ((tid == 1) ? ay : -1);
			unsigned long long const *w = (a >= 0 && (uint32_t)a < ntiles) ? &out[((size_t)((tid == 0) ? 1 : 0)*n + a)*zv] : nullptr;
			for (;;) {
				bool const ready = !w || (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & SHADOW_EDGE_PUB) != 0ull;
				if (__all(ready)) break;
				__builtin_amdgcn_s_sleep(8);
			}
		}
		__syncthreads();
		if (tid < 2*zv) { // in.x(i) = the y-neighbour's out_x, in.y(i) = the x-neighbour's out_y (src/tiled_mesh.cpp:676-687): every lane waits for its own word
			bool const isx = tid < zv; unsigned const i = isx ? tid : tid - zv; int32_t const a = isx ? ay : ax;
			float v = -1.0E6f;
			if (a >= 0) {
				unsigned long long const *w = &out[((size_t)(isx ? 0 : 1)*n + a)*zv + i];
				unsigned long long e = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if ((uint32_t)a < ntiles) {while (!(e & SHADOW_EDGE_PUB)) {__builtin_amdgcn_s_sleep(1); e = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);}}
				v = shadow_edge_t::decode(e & ~SHADOW_EDGE_PUB);
			}
			s_in[tid] = v;
			s_out[tid] = 0ull; // 0 = never written
		}
		__syncthreads();
		shadow_lds_in_t const in{s_in, s_in + zv};
		shadow_lds_out_t o{(uint8_t *)s_mask, s_out, s_out + zv, (int)zv, (int)(SH_SPARE_B + tid), s_out + 2*zv + tid};
		shadow_trace_path_lean(c, s_sh_mh, in, plan, o);
		__syncthreads();
		if (tid < 2*zv) { // the edges first, every word: somebody may be polling it
			__hip_atomic_store(&out[((size_t)((tid < zv) ? 0 : 1)*n + t)*zv + ((tid < zv) ? tid : tid - zv)], s_out[tid] | SHADOW_EDGE_PUB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		uint32_t *gm = (uint32_t *)(smask + (size_t)t*zv*zv); // 16 900 bytes per tile: word-aligned; read by later launches only
		for (unsigned i = tid; i < zv*zv/4; i += SH_LEVEL_THREADS) {gm[i] = s_mask[i] | c.mask_fill;}
		__syncthreads(); // (the next tile's staging overwrites the mask words being copied out)
	}
}

// ------------------------------------------------------------------ min / max reduction (run_erosion's min(vals), get_heightmap_z_range): HBM-bound, 4 B read per cell
// Every thread keeps MM_UNROLL independent 16-byte loads in flight per trip (the loop-carried state is only the running min / max), the grid is sized
// to the chip (256 CUs x 8 blocks of 256 threads) so a 16384^2 grid is ~8 trips of 64 bytes per thread; wave shuffle reduction, then look-before-atomic
// like the fused variant.  d[0] = min f2ord(v), d[1] = min ~f2ord(v); NaNs are skipped.
constexpr int MM_UNROLL = 4;
__device__ __forceinline__ void minmax_acc4(st_f4 const v, float &lo, float &hi) {
	// fminf / fmaxf drop NaNs (v_min_f32 / v_max_f32 with IEEE mode return the non-NaN operand): the same set of values as the `v == v` filter
	lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
	hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
}
__global__ __launch_bounds__(256) void k_minmax(float const *__restrict__ vals, size_t n, uint32_t *__restrict__ d) {
	float lo = INFINITY, hi = -INFINITY;
	bool any = false; // +-inf are legitimate values: remember whether anything but NaNs was seen
	size_t const n4 = n/4, stride = (size_t)gridDim.x*blockDim.x;
	st_f4 const *v4 = (st_f4 const *)vals;
	size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	for (; i + (MM_UNROLL - 1)*stride < n4; i += MM_UNROLL*stride) {
		st_f4 r[MM_UNROLL];
#pragma unroll
		for (int u = 0; u < MM_UNROLL; ++u) {r[u] = __builtin_nontemporal_load(&v4[i + u*stride]);}
#pragma unroll
		for (int u = 0; u < MM_UNROLL; ++u) {minmax_acc4(r[u], lo, hi);}
	}
	for (; i < n4; i += stride) {minmax_acc4(v4[i], lo, hi);}
	if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {float const t = vals[n4*4 + threadIdx.x]; lo = fminf(lo, t); hi = fmaxf(hi, t);}
	any = (lo <= hi); // false only when every value this thread saw was a NaN (or it saw none)
	uint32_t mlo = any ? f2ord(lo) : 0xFFFFFFFFu, mhi = any ? ~f2ord(hi) : 0xFFFFFFFFu;
	wave_minmax_publish(mlo, mhi, d);
}

// ------------------------------------------------------------------ f3: landscape weights texture (tile_t::create_texture, src/tiled_mesh.cpp:1071-1240) + grass blocks
// One block per 32-row band of a tile (the fourth band takes row 128 as well): the band's 33 / 34 height rows are staged in LDS once -- a texel reads its cell's four corners
// from there -- the texels are walked in linear order (consecutive lanes = consecutive texels: the noise field is read and the RGBA words are written in full lines), and the
// band's 8 x 32 grass blocks (add_grass_block_at, src/tiled_mesh.cpp:1354-1371) are folded from the flags the texels left in LDS: no flag array in HBM, no second launch.
constexpr uint32_t WK_BAND = 32, WK_BANDS = 4;
__global__ __launch_bounds__(256) void k_tile_weights(landscape_consts_t c, tile_ref_pod_t const *__restrict__ refs, float const *__restrict__ zvals, float const *__restrict__ noise,
	float const *__restrict__ params, uint32_t *__restrict__ w32, grass_block_pod_t *__restrict__ blocks, uint8_t *__restrict__ any_grass)
{
	__shared__ float s_z[(WK_BAND + 2)*WT_ZV];
	__shared__ uint8_t s_flag[(WK_BAND + 1)*WT_TEX + 3];
	uint32_t const t = blockIdx.x/WK_BANDS, band = blockIdx.x % WK_BANDS, y0 = band*WK_BAND, rows = (band == WK_BANDS - 1) ? WK_BAND + 1 : WK_BAND;
	float const *zt = zvals + (size_t)t*WT_ZV*WT_ZV + (size_t)y0*WT_ZV;
	for (uint32_t i = threadIdx.x; i < (rows + 1)*WT_ZV; i += 256) {s_z[i] = zt[i];}
	biome_corners_t bio;
#pragma unroll
	for (int k = 0; k < 12; ++k) {bio.v[k] = params[(size_t)t*12 + k];} // (block-uniform: scalar loads)
	__syncthreads();
	size_t const tex0 = (size_t)t*WT_TEX*WT_TEX + (size_t)y0*WT_TEX;
	bool grass_here = false;
	for (uint32_t p = threadIdx.x; p < rows*WT_TEX; p += 256) {
		uint32_t const yy = p/WT_TEX, x = p - yy*WT_TEX;
		float const *zc = s_z + yy*WT_ZV + x;
		unsigned flags;
		w32[tex0 + p] = weights_texel_v(c, corner_heights_t{zc[0], zc[1], zc[WT_ZV], zc[WT_ZV + 1]}, bio, noise[tex0 + p], x, y0 + yy, flags);
		s_flag[p] = (uint8_t)flags;
		grass_here |= (flags & 1u) != 0;
	}
	if (grass_here) {any_grass[t] = 1;} // has_any_grass: every writer stores the same value
	if (!blocks) return;
	__syncthreads();
	// the band's grass blocks: 8 rows of 32 blocks of 4 x 4 texels = one per thread, texels in the reference's row-major order (the first contributor picks the block's ix)
	uint32_t const bx = threadIdx.x & 31u, byl = threadIdx.x >> 5;
	tile_ref_pod_t const r = refs[t];
	grass_block_pod_t gb = {0u, 0.0f, 0.0f};
	for (uint32_t yy = byl*GRASS_BLOCK_SZ; yy < (byl + 1)*GRASS_BLOCK_SZ; ++yy) {
		for (uint32_t x = bx*GRASS_BLOCK_SZ; x < (bx + 1)*GRASS_BLOCK_SZ; ++x) {
			if (!(s_flag[yy*WT_TEX + x] & 2u)) continue;
			float const *zc = s_z + yy*WT_ZV + x;
			corner_heights_t const h{zc[0], zc[1], zc[WT_ZV], zc[WT_ZV + 1]};
			float const lowest = min4_std(h), highest = max4_std(h);
			if (gb.ix == 0) {
				gb.ix = ((((uint32_t)(r.tx*128) + x) + 1567u*((uint32_t)(r.ty*128) + y0 + yy)) % c.num_rnd_grass_blocks) + 1; // int + unsigned: unsigned arithmetic
				gb.zmin = lowest; gb.zmax = highest;
			}
			else {gb.zmin = min_std(gb.zmin, lowest); gb.zmax = max_std(gb.zmax, highest);}
		}
	}
	blocks[(size_t)t*GRASS_BLOCK_DIM*GRASS_BLOCK_DIM + (size_t)(band*(WK_BAND/GRASS_BLOCK_SZ) + byl)*GRASS_BLOCK_DIM + bx] = gb;
}

// ------------------------------------------------------------------ grass brush (tile_t::add_or_remove_grass_at, src/tiled_mesh.cpp:3845-3948) on the resident weights, two launches
// k_grass_brush_texels: one block per (tile, GB_CHUNK texels of the tile's window).  The sphere test is the whole block's (a tile outside it leaves at once); two lanes
// build the tile's serial x / y position sums in LDS; every window texel is edited and leaves its `updated` byte in flags[tile][window texel].
constexpr uint32_t GB_THREADS = 256, GB_CHUNK = 1024;
__global__ __launch_bounds__(GB_THREADS) void k_grass_brush_texels(grass_brush_consts_t g, landscape_consts_t c, tile_ref_pod_t const *__restrict__ refs, float const *__restrict__ zvals,
	terra_tile_stats const *__restrict__ stats, float const *__restrict__ params, uint32_t *__restrict__ w32, uint8_t *__restrict__ flags)
{
	__shared__ float s_pos[2*WT_TEX];
	uint32_t const t = blockIdx.x;
	tile_ref_pod_t const r = refs[t];
	if (!grass_tile_hit(g, r.tx, r.ty, stats[t].mzmin, stats[t].mzmax, stats[t].radius)) return;
	if (threadIdx.x < 2) { // pt.x += DX_VAL / pt.y += DY_VAL from the tile's corner on (:3865-3869)
		uint32_t const ax = threadIdx.x;
		float v = ax ? grass_yval(g, r.ty*(int)WT_SIZE + g.dyoff) : grass_xval(g, r.tx*(int)WT_SIZE + g.dxoff);
		float const step = ax ? g.DY_VAL : g.DX_VAL;
		for (uint32_t k = 0; k < WT_TEX; ++k) {s_pos[ax*WT_TEX + k] = v; v += step;}
	}
	__syncthreads();
	uint32_t const x0 = (uint32_t)grass_win0(g.px, s_pos[0], g.DX_VAL, g.hx, g.wx), y0 = (uint32_t)grass_win0(g.py, s_pos[WT_TEX], g.DY_VAL, g.hy, g.wy);
	uint32_t const nwin = g.wx*g.wy;
	float const *zt = zvals + (size_t)t*WT_ZV*WT_ZV, *prm = params + (size_t)t*12;
	for (uint32_t k = 0; k < GB_CHUNK/GB_THREADS; ++k) {
		uint32_t const p = blockIdx.y*GB_CHUNK + k*GB_THREADS + threadIdx.x;
		if (p >= nwin) break;
		uint32_t const yy = p/g.wx, x = x0 + (p - yy*g.wx), y = y0 + yy;
		uint32_t *wp = w32 + ((size_t)t*WT_TEX + y)*WT_TEX + x;
		uint32_t w = *wp;
		unsigned const f = grass_texel(g, c, s_pos[x], s_pos[WT_TEX + y], w, zt, prm, x, y);
		if (f) {*wp = w;}
		flags[(size_t)t*nwin + p] = (uint8_t)f;
	}
}
// k_grass_brush_tiles: one block per tile.  updated / ranges as reductions over the window's flags; on the add path the grass blocks under the window, each
// scanning its 16 texels in row-major order; after a removal the has-grass scan of the whole tile, for a tile that was updated and had grass blocks.
__global__ __launch_bounds__(GB_THREADS) void k_grass_brush_tiles(grass_brush_consts_t g, landscape_consts_t c, tile_ref_pod_t const *__restrict__ refs, float const *__restrict__ zvals,
	terra_tile_stats const *__restrict__ stats, uint8_t const *__restrict__ distant, uint32_t const *__restrict__ w32, grass_block_pod_t *__restrict__ blocks,
	uint8_t const *__restrict__ flags, uint8_t *__restrict__ updated, uint32_t *__restrict__ ranges)
{
	__shared__ uint32_t s_red[6]; // xl, yl, xh, yh, any updated texel, any grass / block
	uint32_t const t = blockIdx.x;
	tile_ref_pod_t const r = refs[t];
	bool const hit = g.rr > 0.0f && grass_tile_hit(g, r.tx, r.ty, stats[t].mzmin, stats[t].mzmax, stats[t].radius);
	if (!hit) {
		if (threadIdx.x < 4) {ranges[4*t + threadIdx.x] = (threadIdx.x < 2) ? WT_SIZE : 0u;}
		if (threadIdx.x == 0) {updated[t] = 0;}
		return;
	}
	if (threadIdx.x < 6) {s_red[threadIdx.x] = (threadIdx.x < 2) ? WT_SIZE : 0u;}
	__syncthreads();
	uint32_t const x0 = (uint32_t)grass_win0(g.px, grass_xval(g, r.tx*(int)WT_SIZE + g.dxoff), g.DX_VAL, g.hx, g.wx);
	uint32_t const y0 = (uint32_t)grass_win0(g.py, grass_yval(g, r.ty*(int)WT_SIZE + g.dyoff), g.DY_VAL, g.hy, g.wy);
	uint32_t const wx = g.wx, wy = g.wy, nwin = wx*wy;
	uint8_t const *fl = flags + (size_t)t*nwin;
	uint32_t xl = WT_SIZE, yl = WT_SIZE, xh = 0, yh = 0, any = 0;
	for (uint32_t p = threadIdx.x; p < nwin; p += GB_THREADS) {
		if (!(fl[p] & 1u)) continue;
		uint32_t const yy = p/wx, x = x0 + (p - yy*wx), y = y0 + yy;
		any = 1;
		xl = min_u32(xl, x); xh = max_u32(xh, min_u32(x + 1, WT_SIZE));
		yl = min_u32(yl, y); yh = max_u32(yh, min_u32(y + 1, WT_SIZE));
	}
	if (any) {atomicMin(&s_red[0], xl); atomicMin(&s_red[1], yl); atomicMax(&s_red[2], xh); atomicMax(&s_red[3], yh); atomicOr(&s_red[4], 1u);}
	__syncthreads();
	bool const upd = s_red[4] != 0;
	if (threadIdx.x < 4) {ranges[4*t + threadIdx.x] = (g.add && upd) ? s_red[threadIdx.x] : ((threadIdx.x < 2) ? WT_SIZE : 0u);}
	if (threadIdx.x == 0) {updated[t] = upd ? 1 : 0;}
	if (!upd) return;
	grass_block_pod_t *bl = blocks + (size_t)t*GRASS_BLOCK_DIM*GRASS_BLOCK_DIM;
	float const *zt = zvals + (size_t)t*WT_ZV*WT_ZV;
	if (g.add) {
		if ((distant && distant[t]) || !c.gen_grass_map) return;
		uint32_t const xe = min_u32(x0 + wx, WT_SIZE), ye = min_u32(y0 + wy, WT_SIZE); // blocks cover texels 0 .. 127 (x >= size: no block)
		if (x0 >= xe || y0 >= ye) return;
		uint32_t const bx0 = x0/GRASS_BLOCK_SZ, by0 = y0/GRASS_BLOCK_SZ, nbx = (xe - 1)/GRASS_BLOCK_SZ - bx0 + 1, nby = (ye - 1)/GRASS_BLOCK_SZ - by0 + 1;
		for (uint32_t b = threadIdx.x; b < nbx*nby; b += GB_THREADS) {
			uint32_t const by = by0 + b/nbx, bx = bx0 + (b - (b/nbx)*nbx);
			grass_block_pod_t gb = bl[by*GRASS_BLOCK_DIM + bx];
			if (grass_block_merge(c, gb, zt, r.tx*(int)WT_SIZE, r.ty*(int)WT_SIZE, bx, by, [=] (unsigned x, unsigned y) {return x - x0 < wx && y - y0 < wy && (fl[(y - y0)*wx + (x - x0)] & 1u);})) {
				bl[by*GRASS_BLOCK_DIM + bx] = gb;
			}
		}
		return;
	}
	// removal: clear every block when no texel has grass left (:3938-3945), for a tile with a non-empty block array
	uint32_t nonempty = 0;
	for (uint32_t b = threadIdx.x; b < GRASS_BLOCK_DIM*GRASS_BLOCK_DIM; b += GB_THREADS) {nonempty |= (bl[b].ix != 0) ? 1u : 0u;}
	if (__syncthreads_or((int)nonempty) == 0) return;
	uint32_t const *wt = w32 + (size_t)t*WT_TEX*WT_TEX;
	uint32_t grass = 0;
	for (uint32_t k = threadIdx.x; k < WT_TEX*WT_TEX; k += GB_THREADS) {grass |= ((wt[k] >> (8*LT_GROUND)) & 0xFFu) ? 1u : 0u;}
	if (__syncthreads_or((int)grass) != 0) return;
	for (uint32_t b = threadIdx.x; b < GRASS_BLOCK_DIM*GRASS_BLOCK_DIM; b += GB_THREADS) {bl[b] = grass_block_pod_t{0u, 0.0f, 0.0f};}
}

// ------------------------------------------------------------------ line-vs-terrain hits (tile_draw_t::line_intersect_mesh, src/tiled_mesh.cpp:3582-3605), two launches
// k_line_boxes: every tile's get_mesh_bcube() and first cell, 32 bytes, once per call.  A distant tile gets the z range [+inf, -inf]: both ends of every finite line
// are below it, so the clip rejects the tile (:2178).
__global__ __launch_bounds__(256) void k_line_boxes(line_query_consts_t c, tile_ref_pod_t const *__restrict__ refs, terra_tile_stats const *__restrict__ stats,
	uint8_t const *__restrict__ distant, uint32_t n, line_box_t *__restrict__ boxes)
{
	uint32_t const i = blockIdx.x*256u + threadIdx.x;
	if (i >= n) return;
	line_box_t b = line_tile_box(c, refs[i].tx, refs[i].ty, stats[i].mzmin, stats[i].mzmax);
	if (distant && distant[i]) {b.d[2][0] = INFINITY; b.d[2][1] = -INFINITY;}
	boxes[i] = b;
}
// k_line_intersect: one workgroup per line.  The batch is culled in rounds of LI_ROUND tiles, LI_PER exact clips per thread; the tiles that pass go to an LDS list and
// are walked one per thread, in parallel.  (A parallel cull rather than a walk of the batch's tile grid: a batch is any list of tiles -- gaps, any order, the same
// tile twice -- and the tie rule follows the batch index, so a grid walk would first need a per-call map from tile coordinates to batch indices.)  Each thread keeps its best (t, batch index); the workgroup takes their lexicographic minimum as one 64-bit key (hits have
// 0 <= t <= 1, whose float bits order as the values do once -0 is read as +0), and the thread that holds it writes the record.
constexpr uint32_t LI_THREADS = 256, LI_PER = 4, LI_ROUND = LI_THREADS*LI_PER;
// a tile's box into registers with two 16-byte loads, before the clip's branches (which would otherwise fetch its fields one at a time)
TERRA_D line_box_t line_box_load(line_box_t const *p) {
	uint4 const a = ((uint4 const *)p)[0], b = ((uint4 const *)p)[1];
	uint32_t const w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
	line_box_t r;
	memcpy(&r, w, sizeof(r));
	return r;
}
__global__ __launch_bounds__(LI_THREADS) void k_line_intersect(line_query_consts_t c, float const *__restrict__ zvals, line_box_t const *__restrict__ boxes, uint32_t n,
	float const *__restrict__ lines, int32_t const *__restrict__ line_tile, line_hit_pod_t *__restrict__ hits)
{
	__shared__ uint32_t s_list[LI_ROUND];
	__shared__ uint32_t s_cnt;
	__shared__ unsigned long long s_best;
	uint32_t const r = blockIdx.x;
	float const *L = lines + (size_t)6*r;
	shadow_pt_t const v1 = {L[0], L[1], L[2]}, v2 = {L[3], L[4], L[5]};
	uint32_t i0, i1;
	line_tile_range(line_tile ? line_tile[r] : -1, n, line_finite(v1, v2), i0, i1);
	size_t const zn = (size_t)(c.S + 2)*(c.S + 2);
	unsigned long long best = ~0ull;
	float bt = 0.0f; int bx = 0, by = 0;
	if (threadIdx.x == 0) {s_best = ~0ull;}
	for (uint32_t base = i0; base < i1; base += LI_ROUND) {
		if (threadIdx.x == 0) {s_cnt = 0;}
		__syncthreads();
		for (uint32_t k = 0; k < LI_PER; ++k) {
			uint32_t const i = base + k*LI_THREADS + threadIdx.x;
			if (i < i1 && line_box_clip(line_box_load(boxes + i), v1, v2)) {s_list[atomicAdd(&s_cnt, 1u)] = i;}
		}
		__syncthreads();
		uint32_t const cnt = s_cnt;
		for (uint32_t j = threadIdx.x; j < cnt; j += LI_THREADS) {
			uint32_t const i = s_list[j];
			float t = 1.0f; int ix = 0, iy = 0;
			if (!line_tile_hit(c, line_box_load(boxes + i), v1, v2, zvals + i*zn, t, ix, iy)) continue;
			uint32_t tb = __float_as_uint(t);
			if (tb == 0x80000000u) {tb = 0u;}
			unsigned long long const key = ((unsigned long long)tb << 32) | i;
			if (key < best) {best = key; bt = t; bx = ix; by = iy;}
		}
		__syncthreads(); // (the next round rewrites s_cnt / s_list)
	}
	if (best != ~0ull) {atomicMin(&s_best, best);}
	__syncthreads();
	unsigned long long const win = s_best;
	if (win == ~0ull) {
		if (threadIdx.x == 0) {hits[r] = line_miss();}
	}
	else if (best == win) {
		uint32_t const i = (uint32_t)win;
		hits[r] = line_hit_make(v1, v2, bt, i, boxes[i], bx, by);
	}
}

// ------------------------------------------------------------------ line queries with inc_trees != 0 (tile_t::line_intersect_mesh, src/tiled_mesh.cpp:2176-2216;
// terra_linetrees.hpp), two launches
// k_line_tree_boxes: one 64-lane wave per tile, four tiles per workgroup.  Lane 0 writes the tile's mesh box as k_line_boxes does; the wave sweeps the tile's pine
// records, a lane a record, for calc_bcube() and the number of valid records, reduced with shuffles (the union starts from an empty box instead of the first
// record's: the same bounds but for the sign of a zero, which neither is_zero_area() nor the clip's comparisons see).
__global__ __launch_bounds__(256) void k_line_tree_boxes(line_trees_consts_t c, line_trees_in_t in, tile_ref_pod_t const *__restrict__ refs, terra_tile_stats const *__restrict__ stats,
	uint8_t const *__restrict__ distant, uint32_t n, line_box_t *__restrict__ boxes, line_tree_box_t *__restrict__ tboxes)
{
	uint32_t const lane = threadIdx.x & 63u;
	uint32_t const i = blockIdx.x*4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (i >= n) return; // (the whole wave)
	if (lane == 0u) {
		line_box_t b = line_tile_box(c.q, refs[i].tx, refs[i].ty, stats[i].mzmin, stats[i].mzmax);
		if (distant && distant[i]) {b.d[2][0] = INFINITY; b.d[2][1] = -INFINITY;}
		boxes[i] = b;
	}
	if (!tboxes) return;
	float const INF = __builtin_inff();
	float box[6] = {INF, -INF, INF, -INF, INF, -INF};
	uint32_t nv = 0, nb = 0;
	uint32_t const cnt = line_trees_count(c, in, i);
	for (uint32_t j = lane; j < cnt; j += 64u) {
		tree_view_rec_t rec;
		if (!line_trees_rec(c, in, i, j, rec)) continue;
		++nv;
		float d[6];
		if (!tree_view_bounds(rec, d)) continue;
		++nb;
		box_union(box, d);
	}
	for (int off = 32; off; off >>= 1) {
		nv += __shfl_xor(nv, off); nb += __shfl_xor(nb, off);
#pragma unroll
		for (int k = 0; k < 6; k += 2) {box[k] = min_std(box[k], __shfl_xor(box[k], off)); box[k + 1] = max_std(box[k + 1], __shfl_xor(box[k + 1], off));}
	}
	if (lane == 0u) {
		line_tree_box_t b;
#pragma unroll
		for (int k = 0; k < 6; ++k) {b.bc[k] = nb ? box[k] : 0.0f;}
		b.nvalid = nv; b.pad = 0u;
		tboxes[i] = b;
	}
}
// k_line_intersect_trees: one workgroup per line, k_line_intersect's rounds.  A tile is kept when its mesh box or the gate of its pine container passes (a distant
// tile never); the kept tiles' mesh walks run first, a tile per thread; a tile whose walk hit drops out (the reference returns cur_t and does not look at its
// trees); then the waves take the remaining gated tiles, a tile per wave, its records 64 at a time, a record per lane, each lane the literal
// small_tree::line_intersect with *t = 1.0.  Every thread keeps its best (t, batch index) as k_line_intersect's 64-bit key and beside it record*2 + part (0 for a
// mesh hit; a tile gives mesh hits or tree hits, never both).  The workgroup takes the minimum key, then among its holders the minimum record*2 + part: over the tiles
// the strictly smaller tn and then the lowest batch index, within a tile the first record and cylinder that reaches the minimum -- what the sequential `t_new < *t`
// leaves.  No per-record pre-test stands in front of the cone test: a record's add_bounds_to_bcube box does not bound its leaf cone.
// Nothing is indexed with a line_tile, a count or a record's inst before its range is known (line_tile_range, line_trees_count, small_tree_size).
constexpr uint32_t LT_THREADS = 256, LT_PER = 4, LT_ROUND = LT_THREADS*LT_PER, LT_TREES = 0x80000000u;
TERRA_D line_tree_box_t line_tree_box_load(line_tree_box_t const *p) {
	uint4 const a = ((uint4 const *)p)[0], b = ((uint4 const *)p)[1];
	uint32_t const w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
	line_tree_box_t r;
	memcpy(&r, w, sizeof(r));
	return r;
}
__global__ __launch_bounds__(LT_THREADS) void k_line_intersect_trees(line_trees_consts_t c, line_trees_in_t in, float const *__restrict__ zvals, line_box_t const *__restrict__ boxes,
	line_tree_box_t const *__restrict__ tboxes, uint32_t n, float const *__restrict__ lines, int32_t const *__restrict__ line_tile, line_tree_hit_pod_t *__restrict__ hits)
{
	__shared__ uint32_t s_list[LT_ROUND]; // the round's kept tiles; LT_TREES: the container's gate passed and the mesh walk has not hit
	__shared__ uint32_t s_cnt, s_sub;
	__shared__ unsigned long long s_best;
	uint32_t const r = blockIdx.x, lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	float const *L = lines + (size_t)6*r;
	shadow_pt_t const v1 = {L[0], L[1], L[2]}, v2 = {L[3], L[4], L[5]};
	uint32_t i0, i1;
	line_tile_range(line_tile ? line_tile[r] : -1, n, line_finite(v1, v2), i0, i1);
	float p1[3], p2[3];
	line_trees_local(c, v1, p1); line_trees_local(c, v2, p2);
	size_t const zn = (size_t)(c.q.S + 2)*(c.q.S + 2);
	unsigned long long best = ~0ull;
	uint32_t bsub = 0u;
	bool bmesh = false;
	float bt = 0.0f; int bx = 0, by = 0;
	if (threadIdx.x == 0) {s_best = ~0ull; s_sub = 0xFFFFFFFFu;}
	for (uint32_t base = i0; base < i1; base += LT_ROUND) {
		if (threadIdx.x == 0) {s_cnt = 0;}
		__syncthreads();
		for (uint32_t k = 0; k < LT_PER; ++k) {
			uint32_t const i = base + k*LT_THREADS + threadIdx.x;
			if (i >= i1) continue;
			line_box_t const b = line_box_load(boxes + i);
			if (b.d[2][0] > b.d[2][1]) continue; // distant (:2178)
			bool const mesh = line_box_clip(b, v1, v2);
			bool trees = false;
			if (tboxes) {
				line_tree_box_t const tb = line_tree_box_load(tboxes + i);
				trees = tb.nvalid != 0u && line_trees_gate(tb, p1, p2);
			}
			if (mesh || trees) {s_list[atomicAdd(&s_cnt, 1u)] = i | (trees ? LT_TREES : 0u);}
		}
		__syncthreads();
		uint32_t const cnt = s_cnt;
		for (uint32_t j = threadIdx.x; j < cnt; j += LT_THREADS) {
			uint32_t const i = s_list[j] & ~LT_TREES;
			float t = 1.0f; int ix = 0, iy = 0;
			if (!line_tile_hit(c.q, line_box_load(boxes + i), v1, v2, zvals + i*zn, t, ix, iy)) continue;
			s_list[j] = i; // the mesh hit: the tile's trees are not looked at
			uint32_t tb = __float_as_uint(t);
			if (tb == 0x80000000u) {tb = 0u;}
			unsigned long long const key = ((unsigned long long)tb << 32) | i;
			if (key < best) {best = key; bsub = 0u; bmesh = true; bt = t; bx = ix; by = iy;}
		}
		__syncthreads();
		for (uint32_t j = wave; j < cnt; j += LT_THREADS/64u) {
			uint32_t const e = s_list[j];
			if (!(e & LT_TREES)) continue; // (the whole wave)
			uint32_t const i = e & ~LT_TREES, nrec = line_trees_count(c, in, i);
			for (uint32_t j0 = 0; j0 < nrec; j0 += 64u) {
				uint32_t const jj = j0 + lane;
				float t; uint32_t part;
				if (!(jj < nrec && line_trees_test(c, in, i, jj, p1, p2, t, part))) continue;
				uint32_t tb = __float_as_uint(t);
				if (tb == 0x80000000u) {tb = 0u;}
				unsigned long long const key = ((unsigned long long)tb << 32) | i;
				uint32_t const sub = jj*2u + part;
				if (key < best || (key == best && !bmesh && sub < bsub)) {best = key; bsub = sub; bmesh = false; bt = t;}
			}
		}
		__syncthreads(); // (the next round rewrites s_cnt / s_list)
	}
	if (best != ~0ull) {atomicMin(&s_best, best);}
	__syncthreads();
	unsigned long long const win = s_best;
	if (win == ~0ull) { // (the whole workgroup)
		if (threadIdx.x == 0) {hits[r] = line_tree_miss();}
		return;
	}
	if (best == win) {atomicMin(&s_sub, bsub);}
	__syncthreads();
	if (best == win && bsub == s_sub) {
		uint32_t const i = (uint32_t)win;
		hits[r] = bmesh ? line_tree_hit_mesh(v1, v2, bt, i, boxes[i], bx, by) : line_tree_hit_tree(v1, v2, bt, i, (int32_t)(bsub >> 1), bsub & 1u);
	}
}

// ------------------------------------------------------------------ tree map (tile_t::add_tree_ao_shadow, src/tiled_mesh.cpp:749-767), two launches
// k_tree_splats: xc, yc, rval and scale of every splat, once per call (a float division per axis and a double one per splat); it also clears `updated`.
__global__ __launch_bounds__(256) void k_tree_splats(tree_tile_pod_t const *__restrict__ tiles, uint32_t n, tree_splat_in_t const *__restrict__ splats, uint32_t ns,
	float dxv, float dyv, tree_splat_pod_t *__restrict__ par, uint8_t *__restrict__ updated)
{
	uint32_t const i = blockIdx.x*256u + threadIdx.x;
	if (i < n) {updated[i] = 0;}
	if (i >= ns) return;
	tree_tile_pod_t const tt = tiles[tree_tile_of(tiles, n, i)];
	par[i] = tree_splat_params(splats[i], tt.xstart, tt.ystart, dxv, dyv);
}
// k_tree_map: one wave per (tile, band of R texel rows); the band lives in LDS for the length of the tile's list.  An ordered scatter with overlap and no atomics:
// a texel belongs to one wave, and that wave applies the tile's splats one after another, in list order.  The list is read 64 splats at a time, one per lane; a
// ballot finds those whose clipped window reaches the band and the wave takes them in lane (= list) order.  A window up to 64 texels wide is covered 64/w rows at
// a time, a wider one row by row.  The barrier between two splats orders the LDS read-modify-writes of different lanes on one texel.
// Cost: every band of a tile reads the tile's whole parameter list (16 bytes a splat, 64 splats per load): 5 bands at S = 128, 342 at S = 1024.  Measured at
// S = 128 only; a long list at a large S would want the splats binned by band first.
constexpr uint32_t TM_CELLS = 4096; // 8 KB of LDS per wave
__global__ __launch_bounds__(64) void k_tree_map(tree_tile_pod_t const *__restrict__ tiles, uint8_t const *__restrict__ distant, tree_splat_pod_t const *__restrict__ par,
	int S, int R, int reset, uint16_t *__restrict__ map, uint8_t *__restrict__ updated)
{
	__shared__ uint16_t s_map[TM_CELLS];
	uint32_t const t = blockIdx.x, lane = threadIdx.x;
	int const W = S + 1, r0 = (int)blockIdx.y*R, r1 = imin(r0 + R, W) - 1; // rows r0 .. r1
	uint32_t const cells = (uint32_t)((r1 - r0 + 1)*W);
	uint16_t *g = map + ((size_t)t*W + r0)*W;
	tree_tile_pod_t const tt = tiles[t];
	if ((distant && distant[t]) || tt.count == 0) { // nothing to apply: the fill of a reset, or nothing at all
		if (reset) {for (uint32_t k = lane; k < cells; k += 64) {g[k] = 0xFFFFu;}}
		return;
	}
	for (uint32_t k = lane; k < cells; k += 64) {s_map[k] = reset ? (uint16_t)0xFFFFu : g[k];}
	__syncthreads();
	bool any = false;
	for (uint32_t base = 0; base < tt.count; base += 64) {
		tree_splat_pod_t s = {0, 0, 0, 0.0f};
		if (base + lane < tt.count) {s = par[tt.first + base + lane];}
		int x1, y1, x2, y2;
		tree_window(s, S, x1, y1, x2, y2);
		unsigned long long m = __ballot(s.rval != 0 && x1 <= x2 && imax(y1, r0) <= imin(y2, r1));
		while (m) {
			int const j = __ffsll((long long)m) - 1;
			m &= m - 1;
			tree_splat_pod_t u;
			u.xc = __shfl(s.xc, j); u.yc = __shfl(s.yc, j); u.rval = __shfl(s.rval, j); u.scale = __shfl(s.scale, j);
			tree_window(u, S, x1, y1, x2, y2);
			int const ya = imax(y1, r0), yb = imin(y2, r1), w = x2 - x1 + 1;
			double const s8 = 0.8*(double)u.scale; float const rval_sq = (float)(u.rval*u.rval);
			if (w <= 64) {
				// lane -> (row ly, column lx) of a block of rp = 64/w rows: (lane + 0.5)/w is at least 1/128 away from an integer, far more than the float error
				float const rcp = 1.0f/(float)w;
				int const rp = (int)(64.5f*rcp), ly = (int)(((float)lane + 0.5f)*rcp), x = x1 + ((int)lane - ly*w);
				if (ly < rp) {
					for (int y = ya + ly; y <= yb; y += rp) {
						uint16_t &c = s_map[(y - r0)*W + x];
						uint16_t v = c;
						if (tree_texel(u, s8, rval_sq, x, y, v)) {c = v; any = true;}
					}
				}
			}
			else {
				for (int y = ya; y <= yb; ++y) {
					for (int x = x1 + (int)lane; x <= x2; x += 64) {
						uint16_t &c = s_map[(y - r0)*W + x];
						uint16_t v = c;
						if (tree_texel(u, s8, rval_sq, x, y, v)) {c = v; any = true;}
					}
				}
			}
			__syncthreads();
		}
	}
	bool const upd = __syncthreads_or((int)any) != 0;
	if (reset || upd) {for (uint32_t k = lane; k < cells; k += 64) {g[k] = s_map[k];}}
	if (upd && lane == 0) {updated[t] = 1;} // (every band that multiplied a texel stores the same 1)
}

// ------------------------------------------------------------------ shadow texture (tile_t::upload_shadow_map_texture, src/tiled_mesh.cpp:885-911) and the tree pass of
// the weights texture (tile_t::create_texture, :1325-1348): streaming, one texel and one 32-bit store per thread; a wave reads 64 consecutive bytes of each byte input
__global__ __launch_bounds__(256) void k_shadow_texture(shadow_tex_consts_t c, uint32_t S, uint8_t const *__restrict__ sun, uint8_t const *__restrict__ moon,
	uint8_t const *__restrict__ ao, uint16_t const *__restrict__ tree, uint32_t *__restrict__ out)
{
	uint32_t const t = blockIdx.x, p = blockIdx.y*256u + threadIdx.x, W = S + 1, Z = S + 2;
	if (p >= W*W) return;
	uint32_t const y = p/W, x = p - y*W;
	size_t const i = (size_t)t*W*W + p, iz = (size_t)t*Z*Z + (size_t)y*Z + x;
	out[i] = shadow_texel(c, sun ? sun[iz] : 0u, moon ? moon[iz] : 0u, ao ? ao[i] : 170u, tree != nullptr, tree ? tree[i] : 0xFFFFu);
}
// (in and out may be the same array: no __restrict__)
__global__ __launch_bounds__(256) void k_tree_weights(size_t ntex, uint32_t const *in, uint8_t const *__restrict__ tree, uint32_t *out) {
	size_t const i = (size_t)blockIdx.x*256u + threadIdx.x;
	if (i >= ntex) return;
	out[i] = tree_weights_texel(in[i], tree[2*i]);
}

// ------------------------------------------------------------------ tree placement (small_tree_group::gen_trees, src/sm_tree.cpp:439-474; terra_treeplace.hpp)
// One workgroup per tile, so that the tile's trees come out in the reference's loop order without atomics.  The loop's cells are taken 256 at a time, row-major:
// every thread runs the selection of get_ntrees_for_mesh_xy for its cell (three generator steps and a modulo; about one cell in fifty passes at the defaults) and
// the survivors' cell numbers go, in order, into a ring in LDS.  Whenever the ring holds 256 of them (and once more at the end) every thread takes one and runs the
// expensive rest -- the 80-term density field, the histogram test, maybe_add_tree with its zval -- so the lanes stay busy; the trees that come out of a batch
// are written behind those of the batches before.  Both compactions are a ballot per wave plus a prefix over the four waves.
// Where the time goes (kernel trace, 4096 tiles at S = 128, sine mode): the survivors, not the selection.  A survivor's two fields are 2 x 80 terms of two SINF
// look-ups each, and a look-up is a gather from the 128 KB table that no two lanes share; four cells per thread in the selection made the kernel slower (443 us
// against 353: one wave less per SIMD to hide those gathers behind).
constexpr uint32_t TREEP_THREADS = 256, TREEP_RING = 512;
// ---- the block-stream helpers of the per-tile record kernels: a workgroup of TREEP_THREADS threads, everything "uniform" the same in every thread of it
// rank of the calling thread among the block's threads with `flag`, in thread order, and their number; two barriers
__device__ __forceinline__ uint32_t tp_block_rank(bool flag, uint32_t *s_wave, uint32_t &total) {
	uint32_t const lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	unsigned long long const m = __ballot(flag);
	if (lane == 0) {s_wave[w] = (uint32_t)__popcll(m);}
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t k = 0; k < TREEP_THREADS/64; ++k) {uint32_t const v = s_wave[k]; all += v; if (k < w) {before += v;}}
	__syncthreads();
	total = all;
	return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
// A ring of RING slots in LDS that holds entries [head, tail) in the order they were pushed (head, tail: uniform); the slots themselves belong to the kernel.
// A round of the kernel is: push what the round's threads selected; if due(), take() up to TREEP_THREADS entries, one per thread, and hand what becomes of them
// to tp_emit or to the push of a next ring.  Why RING >= 2*TREEP_THREADS is enough: due() leaves at most `at` - 1 <= TREEP_THREADS - 1 entries behind, a push adds
// at most TREEP_THREADS, and a take that is due follows before the next push, so no more than RING - 1 entries are ever pending.
// The barriers: push ends with one, after its stores, so a take that follows reads complete slots.  Every take is followed by a tp_emit or a push before the next
// push to its ring, and the next push ranks before it stores: the barriers of those tp_block_ranks lie between a take's reads and the stores that reuse its slots.
template<uint32_t RING> struct tp_ring_t {
	static_assert((RING & (RING - 1)) == 0 && RING >= 2*TREEP_THREADS, "a power of two that holds a not-yet-due remainder and one push");
	uint32_t head = 0, tail = 0;
	// the threads with `flag` append, in thread order: store(slot) writes one's entry
	template<class STORE> __device__ __forceinline__ void push(bool flag, uint32_t *s_wave, STORE store) {
		uint32_t n;
		uint32_t const rank = tp_block_rank(flag, s_wave, n);
		if (flag) {store((tail + rank) & (RING - 1));}
		tail += n;
		__syncthreads();
	}
	// the flush rule: `at` (<= TREEP_THREADS) entries pending, or anything pending when no push will follow
	__device__ __forceinline__ bool due(bool nothing_more_comes, uint32_t at = TREEP_THREADS) const {return tail - head >= at || (nothing_more_comes && head < tail);}
	// the oldest min(pending, TREEP_THREADS) entries leave, thread i with the i-th: whether this thread has one, and its slot
	__device__ __forceinline__ bool take(uint32_t &slot) {
		uint32_t const nb = (tail - head < TREEP_THREADS) ? tail - head : TREEP_THREADS;
		slot = (head + threadIdx.x) & (RING - 1);
		head += nb;
		return threadIdx.x < nb;
	}
};
// the records of the threads with `ok` go behind the `count` records so far, in thread order, as far as the array has room; count (uniform) counts them all.
// record() gives a thread's record and is called only where it is stored
template<class REC, class RECORD> __device__ __forceinline__ void tp_emit(bool ok, RECORD record, REC *out, uint32_t capacity, uint32_t &count, uint32_t *s_wave) {
	uint32_t n;
	uint32_t const rank = tp_block_rank(ok, s_wave, n);
	if (ok && count + rank < capacity) {out[count + rank] = record();}
	count += n;
}
// remove_elements_serial's result (terra_common.hpp) on records [0, cnt) by the workgroup, in place; returns the new size M (uniform).  remove_element swaps the
// back into the hole and tests the same index again, so the result is not in input order; its closed form: with M survivors among the cnt records, a survivor below M
// stays, and the holes below M, ascending, receive the survivors at M and above, descending (tests/test_tree_edit_emul.py checks this against the literal loop).
// Three sweeps of TREEP_THREADS records: (1) M, (2) the survivors at M and above into idx[] (cnt words of global scratch) in ascending order, (3) the k-th hole below M
// takes record idx[H - 1 - k].  Sources lie at M and above, destinations below: in place after a barrier.  removed(i) is a pure test of record i that the sweeps
// repeat.  move(dst, src) copies a record and whatever travels with it.
template<class REMOVED, class MOVE> __device__ __forceinline__ uint32_t tp_block_remove(uint32_t cnt, uint32_t *idx, uint32_t *s_wave, REMOVED removed, MOVE move) {
	uint32_t const tid = threadIdx.x;
	uint32_t m = 0, nk;
	for (uint32_t base = 0; base < cnt; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		tp_block_rank(i < cnt && !removed(i), s_wave, nk);
		m += nk;
	}
	if (m == cnt) return m;
	uint32_t h = 0;
	for (uint32_t base = m; base < cnt; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool const keep = i < cnt && !removed(i);
		uint32_t const rank = tp_block_rank(keep, s_wave, nk);
		if (keep) {idx[h + rank] = i;}
		h += nk;
	}
	__syncthreads(); // idx[] is complete
	uint32_t k0 = 0;
	for (uint32_t base = 0; base < m; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool const hole = i < m && removed(i);
		uint32_t const rank = tp_block_rank(hole, s_wave, nk);
		if (hole) {move(i, idx[h - 1u - (k0 + rank)]);}
		k0 += nk;
	}
	return m;
}
__global__ __launch_bounds__(TREEP_THREADS) void k_tree_place(tree_place_consts_t const *__restrict__ consts, tile_ref_pod_t const *__restrict__ tiles, float const *__restrict__ d_dens,
	uint8_t const *__restrict__ skip, terra_tile_stats const *__restrict__ stats, uint32_t capacity, tree_place_pod_t *__restrict__ trees, uint32_t *__restrict__ counts)
{
	__shared__ uint32_t s_ring[TREEP_RING], s_wave[TREEP_THREADS/64];
	tree_place_consts_t const &c = *consts;
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	tile_ref_pod_t const r = tiles[t];
	float dens[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	if (!c.brush) {for (int k = 0; k < 4; ++k) {dens[k] = d_dens[4*(size_t)t + k];}}
	// (uniform over the block)
	if (!tree_tile_live(c, dens, skip && skip[t], stats != nullptr, stats ? stats[t].mzmin : 0.0f, stats ? stats[t].mzmax : 0.0f)) {
		if (tid == 0) {counts[t] = 0;}
		return;
	}
	uint32_t const ncell = (uint32_t)c.ncell, ncells = ncell*ncell;
	tree_place_pod_t *const out = trees + (size_t)t*capacity;
	tp_ring_t<TREEP_RING> q;
	uint32_t count = 0; // the tile's trees so far (uniform)
	for (uint32_t base = 0; base < ncells || q.head < q.tail; base += TREEP_THREADS) {
		if (base < ncells) {
			uint32_t const cell = base + tid;
			bool sel = false;
			if (cell < ncells) {
				uint32_t const iy = cell/ncell, ix = cell - iy*ncell;
				tree_rgen_t rg;
				sel = tree_cell_selected(c, dens, r.tx, r.ty, ix, iy, rg);
			}
			q.push(sel, s_wave, [&](uint32_t k) {s_ring[k] = cell;});
		}
		if (!q.due(base + TREEP_THREADS >= ncells)) continue; // (fewer than 256 pending and more cells to come)
		bool ok = false;
		tree_place_pod_t o;
		uint32_t k;
		if (q.take(k)) {
			uint32_t const cell = s_ring[k], iy = cell/ncell, ix = cell - iy*ncell;
			tree_rgen_t rg;
			tree_cell_selected(c, dens, r.tx, r.ty, ix, iy, rg); // (the generator as the selection left it: cheaper to redo than to keep)
			ok = tree_cell_finish(c, r.tx, r.ty, ix, iy, rg, o);
		}
		tp_emit(ok, [&] {return o;}, out, capacity, count, s_wave);
	}
	if (tid == 0) {counts[t] = count;}
}

// ------------------------------------------------------------------ deciduous tree placement (tree_cont_t::gen_trees_tt_within_radius, src/Tree.cpp:2240-2303; terra_decidplace.hpp)
// One workgroup per tile and the loop's cells 256 at a time, row-major, as in k_tree_place: every thread runs the selection of :2269-2275 for its cell and the
// survivors' cell numbers go, in order, into a first ring in LDS.  Whenever that ring holds 256 of them (and at the end) every thread takes one and finds its
// site -- the position, get_exact_zval, the range, the class, the 80-term coverage field -- and what is left goes, in order, with its height and its generator,
// into a second ring.  Whenever that one holds 256 (and at the end) every thread takes one and runs the five type fields, the slope test over the tile's zvals
// and add_new_tree's index; the trees of a batch are written behind those of the batches before.  Three ballot-and-prefix compactions, no atomics.
// Why two rings: at num_trees 400 about one cell in thirty is selected and a third to a half of those fail the range, the class or the coverage field, so without
// the second compaction the five type fields (5 x 80 terms of two SINF gathers, the bulk of a tree's work) would run with that share of the lanes idle.  The type
// fields take one pass over k (decid_type_fields).  87 VGPRs, 106 SGPRs with 20 spilled to vector lanes, 14352 B LDS, no scratch: five waves per SIMD.
// The variants without the second ring and with five separate field passes, and the timings (tools/bench_decid_place.py): DESIGN.md, section 4.
constexpr uint32_t DECIDP_RING = 512;
__global__ __launch_bounds__(TREEP_THREADS) void k_decid_place(decid_place_consts_t const *__restrict__ consts, tile_ref_pod_t const *__restrict__ tiles, float const *__restrict__ d_dens,
	uint8_t const *__restrict__ skip, terra_tile_stats const *__restrict__ stats, float const *__restrict__ zvals, uint32_t capacity, decid_place_pod_t *__restrict__ trees,
	uint32_t *__restrict__ counts)
{
	__shared__ uint32_t s_ring[DECIDP_RING], s_wave[TREEP_THREADS/64];
	__shared__ uint32_t s_cell[DECIDP_RING]; __shared__ float s_pos[DECIDP_RING][3]; __shared__ int32_t s_seed[DECIDP_RING][2]; // the second ring
	decid_place_consts_t const &c = *consts;
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	tile_ref_pod_t const r = tiles[t];
	float dens[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	if (!c.b.brush) {for (int k = 0; k < 4; ++k) {dens[k] = d_dens[4*(size_t)t + k];}}
	// (uniform over the block)
	if ((skip && skip[t]) || (stats && !decid_zrange_ok(c.b, stats[t].mzmin, stats[t].mzmax))) {
		if (tid == 0) {counts[t] = 0;}
		return;
	}
	float const veg = decid_tile_veg(c, dens);
	bool const slope_test = stats && decid_mesh_dz(stats[t]) > 1.0f;
	float const *const tz = zvals ? zvals + (size_t)t*(size_t)(c.b.S + 2)*(size_t)(c.b.S + 2) : nullptr;
	uint32_t const ncell = (uint32_t)c.b.ncell, ncells = ncell*ncell;
	decid_place_pod_t *const out = trees + (size_t)t*capacity;
	tp_ring_t<DECIDP_RING> q1, q2;
	uint32_t count = 0; // the tile's trees so far (uniform)
	for (uint32_t base = 0; ; base += TREEP_THREADS) {
		if (base < ncells) {
			uint32_t const cell = base + tid;
			bool sel = false;
			if (cell < ncells) {
				uint32_t const iy = cell/ncell, ix = cell - iy*ncell;
				tree_rgen_t rg;
				sel = decid_cell_selected(c, veg, r.tx, r.ty, ix, iy, rg);
			}
			q1.push(sel, s_wave, [&](uint32_t k) {s_ring[k] = cell;});
		}
		bool const last = base + TREEP_THREADS >= ncells; // no cell comes after this round
		if (q1.due(last)) { // the sites of up to 256 selected cells
			bool ok = false;
			uint32_t cell = 0, k1;
			float pos[3] = {0.0f, 0.0f, 0.0f};
			tree_rgen_t rg; rg.set_state(0, 0);
			if (q1.take(k1)) {
				cell = s_ring[k1];
				uint32_t const iy = cell/ncell, ix = cell - iy*ncell;
				decid_cell_selected(c, veg, r.tx, r.ty, ix, iy, rg); // (the generator as the selection left it: cheaper to redo than to keep)
				ok = decid_cell_site(c, r.tx, r.ty, ix, iy, rg, pos);
			}
			q2.push(ok, s_wave, [&](uint32_t k) {
				s_cell[k] = cell; s_pos[k][0] = pos[0]; s_pos[k][1] = pos[1]; s_pos[k][2] = pos[2]; s_seed[k][0] = rg.rseed1; s_seed[k][1] = rg.rseed2;
			});
		}
		bool const drained = last && q1.head == q1.tail; // nothing comes after what the second ring holds
		if (q2.due(drained)) { // the types, the slope test and the records of up to 256 sites
			bool ok = false;
			decid_place_pod_t o;
			uint32_t k;
			if (q2.take(k)) {
				uint32_t const cell = s_cell[k], iy = cell/ncell, ix = cell - iy*ncell;
				float const pos[3] = {s_pos[k][0], s_pos[k][1], s_pos[k][2]};
				tree_rgen_t rg; rg.set_state(s_seed[k][0], s_seed[k][1]);
				ok = decid_cell_finish(c, r.tx, r.ty, ix, iy, rg, pos, slope_test, tz, o);
			}
			tp_emit(ok, [&] {return o;}, out, capacity, count, s_wave);
		}
		if (drained && q2.head == q2.tail) break;
	}
	if (tid == 0) {counts[t] = count;}
}

// ------------------------------------------------------------------ scenery placement (scenery_group::gen, src/scenery.cpp:1274-1353; terra_sceneryplace.hpp)
// One workgroup per tile and the tile's S*S cells 256 at a time, row-major, as in k_tree_place: every thread runs the selection of :1276-1281 for its cell (three
// generator steps and a modulo, then one more step for veg) and the survivors' cell numbers go, in order, into a ring in LDS.  When the ring is flushed every
// thread takes one survivor and creates its object; the objects of a batch are written behind those of the batches before.  Two ballot-and-prefix compactions, no
// atomics.  The per-kind counts are ballots too: lane k of every wave adds up the wave's objects of kind k, and the four waves' sums meet in LDS at the end.
// The finish stage diverges by kind, so it is cut in three: the kind and what it draws before its position (a few generator steps), then gen_spos with its
// get_exact_zval -- 80 terms of two SINF gathers, the bulk of a survivor's time -- for all lanes together, then the kind's create().  A log's second get_exact_zval
// (pt2) runs after that in a region of its own in which only the log lanes are live, so no other kind's code waits inside it.
// When to flush: at 256 pending (and at the end), not at one wave's 64.  The barriers make a flush a block-wide event whatever its size, and its time is the latency
// of one survivor's gather loop, which is the same for 64 survivors in one wave as for 256 in four waves on four SIMDs.  At the defaults a tile has about 90
// survivors among 16384 cells: at 256 they are finished in one flush at the end, at 64 in two, the first of them with three waves idle at the barrier.  A higher
// threshold never adds a flush; only above 256 survivors per tile (tree_scale 8) do both forms flush equally full waves.  The other workgroups of the CU hide a
// flush's latency in either form.  Measured, 4096 tiles at S = 128: 0.59 ms with 256 against 0.86 ms with 64 in sine mode, 1.22 against 2.43 ms at tree_scale 8.
// 86 VGPRs, 106 SGPRs with 111 spilled to vector lanes, 2208 B LDS, no scratch: five waves per SIMD.  The timings (tools/bench_scenery_place.py): DESIGN.md, section 4.
constexpr uint32_t SCENP_FLUSH = TREEP_THREADS;
static_assert(SCENP_FLUSH <= TREEP_THREADS, "tp_ring_t's bound on what is pending");
__global__ __launch_bounds__(TREEP_THREADS) void k_scenery_place(scenery_place_consts_t const *__restrict__ consts, tile_ref_pod_t const *__restrict__ tiles, float const *__restrict__ d_dens,
	uint8_t const *__restrict__ skip, uint32_t capacity, scenery_place_pod_t *__restrict__ objs, uint32_t *__restrict__ counts, uint32_t *__restrict__ kind_counts)
{
	__shared__ uint32_t s_ring[TREEP_RING], s_wave[TREEP_THREADS/64], s_kind[TREEP_THREADS/64][SCENERY_KINDS];
	scenery_place_consts_t const &c = *consts;
	uint32_t const t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
	tile_ref_pod_t const r = tiles[t];
	// (uniform over the block)
	if (skip && skip[t]) {
		if (tid == 0) {counts[t] = 0;}
		if (kind_counts && tid < (uint32_t)SCENERY_KINDS) {kind_counts[(size_t)t*SCENERY_KINDS + tid] = 0;}
		return;
	}
	float dens[4];
	for (int k = 0; k < 4; ++k) {dens[k] = d_dens[4*(size_t)t + k];}
	float const veg_ = scenery_tile_veg(c, dens);
	uint32_t const S = (uint32_t)c.b.S, ncells = S*S;
	scenery_place_pod_t *const out = objs + (size_t)t*capacity;
	tp_ring_t<TREEP_RING> q;
	uint32_t count = 0; // the tile's objects so far (uniform)
	uint32_t kc = 0;    // lane k < SCENERY_KINDS: this wave's objects of kind k so far
	for (uint32_t base = 0; base < ncells || q.head < q.tail; base += TREEP_THREADS) {
		if (base < ncells) {
			uint32_t const cell = base + tid;
			bool sel = false;
			if (cell < ncells) {
				uint32_t const iy = cell/S, ix = cell - iy*S;
				tree_rgen_t rg; int val; bool veg;
				sel = scenery_cell_selected(c, veg_, r.tx, r.ty, ix, iy, rg, val, veg);
			}
			q.push(sel, s_wave, [&](uint32_t k) {s_ring[k] = cell;});
		}
		if (!q.due(base + TREEP_THREADS >= ncells, SCENP_FLUSH)) continue; // (too few pending and more cells to come)
		bool ok = false;
		int kind = SCENERY_NONE, val = 0; bool veg = false;
		int32_t pre_i = 0; float pre_f[3] = {0.0f, 0.0f, 0.0f}, pos[3] = {0.0f, 0.0f, 0.0f};
		uint32_t ix = 0, iy = 0, k;
		tree_rgen_t rg; rg.set_state(1, 1);
		scenery_place_pod_t o;
		if (q.take(k)) {
			uint32_t const cell = s_ring[k];
			iy = cell/S; ix = cell - iy*S;
			scenery_cell_selected(c, veg_, r.tx, r.ty, ix, iy, rg, val, veg); // (the generator as the selection left it: cheaper to redo than to keep)
			kind = scenery_cell_kind(c, val, veg, rg, pre_i, pre_f);
		}
		if (kind != SCENERY_NONE) {scenery_gen_spos(c, r.tx, r.ty, ix, iy, rg, pos);} // all kinds together
		if (kind != SCENERY_NONE) {ok = scenery_cell_create(c, kind, pre_i, pre_f, rg, pos, o);}
		if (ok && kind == SCENERY_LOG) {ok = scenery_log_finish(c, tree_exact_zval(c.b, o.p[5], o.p[6]), rg, o);} // the log lanes alone
		if (ok) {scenery_set_tail(rg, ix, iy, o);}
		tp_emit(ok, [&] {return o;}, out, capacity, count, s_wave);
#pragma unroll
		for (int k = 0; k < SCENERY_KINDS; ++k) {
			uint32_t const nk = (uint32_t)__popcll(__ballot(ok && kind == k));
			if (lane == (uint32_t)k) {kc += nk;}
		}
	}
	if (tid == 0) {counts[t] = count;}
	if (kind_counts) { // (uniform)
		if (lane < (uint32_t)SCENERY_KINDS) {s_kind[tid >> 6][lane] = kc;}
		__syncthreads();
		if (tid < (uint32_t)SCENERY_KINDS) {
			uint32_t sum = 0;
			for (uint32_t w = 0; w < TREEP_THREADS/64; ++w) {sum += s_kind[w][tid];}
			kind_counts[(size_t)t*SCENERY_KINDS + tid] = sum;
		}
	}
}

// ------------------------------------------------------------------ flowers (flower_tile_manager_t::gen_flowers / update_subrange / clear_within, src/grass.cpp:859-926; terra_flowers.hpp)
// k_flowers_place: ONE WAVE per tile.  The reference seeds its generator once per tile and draws once for a rejected candidate and nine times (eight with a fixed
// colour) for an accepted one, so where candidate i's test draw lies in the stream depends on every acceptance before it: a literal walk is a chain of generator
// steps as long as the tile's stream.  Both recurrences are multiplications modulo a prime, so the state k draws on is one modular multiplication away (lcg_jump),
// and the wave speculates:
//   - the cells of the rectangle 64 at a time, row-major; a prefix sum over the lanes numbers their candidates in loop order, and the chunk's candidates are laid out
//     in LDS in that order with their cell and its dval;
//   - the candidates FLW_B = 10 at a time.  Candidate l of a block can have 0 .. l acceptances before it, so its test draw lies at one of l + 1 stream offsets
//     l + E*a (E = the further draws of an acceptance): 55 (l, a) pairs, one per lane.  Every lane jumps to its pair's state, runs the density test there and the
//     ballot is the block's whole outcome table in two scalar registers;
//   - the true path is then ten scalar steps over that mask (bit l(l+1)/2 + a, a += bit), not ten dependent generator steps and double compares;
//   - the accepted candidates' test states go into a queue in LDS; whenever it cannot take another block (and at the end) every lane takes one entry, draws the
//     rest of its record and writes it at queue order behind the records so far.
// No window of states in LDS: a lane reaches its state with one multiplication each of the two seeds by a power from a 91-entry table that the wave computes once.
// The update_subrange generation is the same kernel over the stroke's rectangle with that call's seed, behind the survivors k_flowers_remove left.
constexpr uint32_t FLW_B = 10, FLW_PAIRS = FLW_B*(FLW_B + 1)/2, FLW_POW = FLW_B*9 + 1, FLW_Q = 64, FLW_MAP = 256;
template<bool EDIT> __global__ __launch_bounds__(64) void k_flowers_place(flower_consts_t c, tile_ref_pod_t const *__restrict__ tiles, uint8_t const *__restrict__ skip,
	uint8_t const *__restrict__ kind, uint32_t const *__restrict__ ranges, uint8_t const *__restrict__ weights, float const *__restrict__ den, float const *__restrict__ col,
	uint32_t capacity, flower_pod_t *flowers, uint32_t *aux, uint32_t *counts)
{
	__shared__ uint32_t s_p1[FLW_POW], s_p2[FLW_POW]; // A1^k mod M1, A2^k mod M2
	__shared__ uint32_t s_pre[65];                    // candidates before cell `lane` of the chunk; [64]: all of them (read only by a chunk with more than FLW_MAP)
	__shared__ float s_cd[FLW_MAP];                   // the chunk's candidates in loop order: dval of the cell ..
	__shared__ uint32_t s_cc[FLW_MAP];                // .. and the cell
	__shared__ uint32_t s_q[3*FLW_Q];                 // accepted candidates: the two seeds at the test draw, the cell
	uint32_t const t = blockIdx.x, lane = threadIdx.x;
	uint32_t const S = (uint32_t)c.S;
	uint32_t xl = 0, yl = 0, xh = S, yh = S, count = 0;
	if (EDIT) {
		if (kind[t] != FLOWER_EDIT_ADD) return; // (uniform)
		xl = ranges[4*t]; yl = ranges[4*t + 1]; xh = ranges[4*t + 2]; yh = ranges[4*t + 3]; // inside the tile: flower_edit_kind
		count = counts[t];                                                                 // the survivors
	}
	else if (skip && skip[t]) {
		if (lane == 0) {counts[t] = 0;}
		return;
	}
	for (uint32_t k = lane; k < FLW_POW; k += 64) {s_p1[k] = lcg_powmod<LCG_M1>(LCG_A1, k); s_p2[k] = lcg_powmod<LCG_M2>(LCG_A2, k);}
	tile_ref_pod_t const r = tiles[t];
	uint32_t const nx = xh - xl, ncells = nx*(yh - yl);
	uint8_t const *const w = weights + (size_t)t*(S + 1)*(S + 1)*4;
	float const *const dn = den + (size_t)t*S*S, *const cl = col + (size_t)t*S*S;
	flower_pod_t *const out = flowers + (size_t)t*capacity;
	uint32_t *const out_aux = aux ? aux + (size_t)t*capacity : nullptr;
	uint32_t const E = c.fixed_color ? 7u : 8u; // the draws of an accepted candidate after its test
	// lane p < 55 owns the pair (l, a): candidate l of a block with a acceptances before it
	uint32_t pl = 0;
	while ((pl + 1)*(pl + 2)/2 <= lane) {++pl;}
	uint32_t const pa = lane - pl*(pl + 1)/2;
	bool const is_pair = lane < FLW_PAIRS;
	tree_rgen_t cur; // the state that stands for the next draw of the stream
	flower_seed(c.S, r.tx, r.ty, (int)xl, (int)yl, cur);
	cur.advance(); // the first step literally: the seeds may lie outside [0, m)
	uint32_t qn = 0; // (uniform)
	auto flush = [&]() {
		__syncthreads();
		if (lane < qn) {
			tree_rgen_t rg; rg.rseed1 = (int32_t)s_q[lane]; rg.rseed2 = (int32_t)s_q[FLW_Q + lane];
			uint32_t const cell = s_q[2*FLW_Q + lane], x = cell & 1023u, y = cell >> 10;
			flower_pod_t o;
			uint32_t const cf = flower_record(c, (int)x, (int)y, cl[(size_t)y*S + x], rg, o);
			if (count + lane < capacity) {out[count + lane] = o; if (out_aux) {out_aux[count + lane] = flower_aux(x, y, cf);}}
		}
		count += qn; qn = 0;
		__syncthreads();
	};
	__syncthreads(); // the power tables
	for (uint32_t base = 0; base < ncells; base += 64) {
		uint32_t const k = base + lane;
		uint32_t npb = 0, cell = 0; float dval = 0.0f;
		if (k < ncells) {
			uint32_t const y = yl + k/nx, x = xl + k%nx;
			npb = flower_num_per_bin(c, w[4*((size_t)y*(S + 1) + x) + 2]);
			if (npb) {dval = dn[(size_t)y*S + x];}
			cell = x | (y << 10);
		}
		uint32_t incl = npb; // inclusive prefix over the lanes
		for (uint32_t d = 1; d < 64; d <<= 1) {uint32_t const v = __shfl_up(incl, d); if (lane >= d) {incl += v;}}
		uint32_t const total = __builtin_amdgcn_readfirstlane(__shfl(incl, 63));
		if (total == 0) continue;
		// a chunk's candidates are laid out in LDS, so that a lane finds its candidate's cell with one read; a chunk with more of them than the table holds (five and
		// more candidates a cell) searches the prefix sums instead
		bool const mapped = total <= FLW_MAP; // (uniform)
		if (mapped) {for (uint32_t i = 0; i < npb; ++i) {s_cd[incl - npb + i] = dval; s_cc[incl - npb + i] = cell;}}
		else {
			s_pre[lane] = incl - npb;
			if (lane == 63) {s_pre[64] = incl;}
		}
		__syncthreads();
		for (uint32_t kb = 0; kb < total; kb += FLW_B) {
			uint32_t const nb = (total - kb < FLW_B) ? total - kb : FLW_B;
			bool const live = is_pair && pl < nb;
			uint32_t owner = 0; // (searching form) the lane that holds the cell of candidate kb + l: the last one whose prefix is <= kb + l
			float dv = 0.0f;
			if (mapped) {if (live) {dv = s_cd[kb + pl];}}
			else {
				if (live) {
					uint32_t const ci = kb + pl;
					uint32_t lo = 0, hi = 64; // s_pre[lo] <= ci < s_pre[hi]
					while (hi - lo > 1) {uint32_t const mid = (lo + hi) >> 1; if (s_pre[mid] <= ci) {lo = mid;} else {hi = mid;}}
					owner = lo;
				}
				dv = __shfl(dval, owner);
			}
			bool acc = false;
			if (live) {
				uint32_t const off = pl + E*pa;
				acc = !((double)dv + c.zs*(double)lcg_state_signed_rand_float(lcg_jump(cur, s_p1[off], s_p2[off])) > (double)c.hthresh); // flower_candidate_accepted on that state
			}
			unsigned long long const mask = __ballot(acc);
			uint32_t a = 0, my_a = 0; bool my_acc = false;
#pragma unroll
			for (uint32_t l = 0; l < FLW_B; ++l) {
				uint32_t const bit = (l < nb) ? (uint32_t)((mask >> (l*(l + 1)/2 + a)) & 1ull) : 0u;
				if (lane == l) {my_a = a; my_acc = bit != 0;}
				a += bit;
			}
			a = __builtin_amdgcn_readfirstlane(a);
			// lane l < nb holds candidate l's outcome; (searching form) its cell is the one pair (l, 0) found, lane l(l+1)/2
			uint32_t my_cell;
			if (mapped) {my_cell = (lane < nb) ? s_cc[kb + lane] : 0u;}
			else {
				uint32_t const lc = (lane < FLW_B) ? lane : 0u;
				my_cell = __shfl(cell, __shfl(owner, lc*(lc + 1)/2));
			}
			if (my_acc) {
				uint32_t const off = lane + E*my_a;
				tree_rgen_t const st = lcg_jump(cur, s_p1[off], s_p2[off]);
				s_q[qn + my_a] = (uint32_t)st.rseed1; s_q[FLW_Q + qn + my_a] = (uint32_t)st.rseed2; s_q[2*FLW_Q + qn + my_a] = my_cell;
			}
			qn += a;
			cur = lcg_jump(cur, s_p1[nb + E*a], s_p2[nb + E*a]);
			if (qn + FLW_B > FLW_Q) {flush();}
		}
		__syncthreads(); // the next chunk rewrites the candidate table
	}
	if (qn) {flush();}
	if (lane == 0) {counts[t] = count;}
}
// k_flowers_remove: a workgroup per tile decides what the stroke does to the tile (flower_edit_kind), writes its status and runs the removal loop of update_subrange
// or clear_within with tp_block_remove.  aux moves with its records.  counts[t] = M; an adding stroke's k_flowers_place continues from there.
__global__ __launch_bounds__(TREEP_THREADS) void k_flowers_remove(flower_edit_consts_t c, tile_ref_pod_t const *__restrict__ tiles, uint8_t const *__restrict__ generated,
	uint8_t const *__restrict__ updated, uint32_t const *__restrict__ ranges, uint32_t capacity, flower_pod_t *flowers, uint32_t *aux, uint32_t *counts, uint8_t *status,
	uint32_t *idx, uint8_t *kind_out)
{
	__shared__ uint32_t s_wave[TREEP_THREADS/64];
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	uint32_t rg[4] = {0u, 0u, 0u, 0u};
	if (ranges) {for (int k = 0; k < 4; ++k) {rg[k] = ranges[4*t + k];}}
	int const kind = flower_edit_kind(c, updated[t], generated ? generated[t] : (uint8_t)1, rg); // (uniform)
	if (tid == 0) {kind_out[t] = (uint8_t)kind; status[t] = (kind == FLOWER_EDIT_NONE) ? 0 : ((kind == FLOWER_EDIT_REFUSED) ? 2 : 1);}
	if (kind != FLOWER_EDIT_ADD && kind != FLOWER_EDIT_REMOVE) return;
	tile_ref_pod_t const r = tiles[t];
	float px, py;
	flower_brush_local(c, r.tx, r.ty, px, py);
	auto removed = [&](flower_pod_t const &f) {
		return (kind == FLOWER_EDIT_ADD) ? flower_in_range(c.f, f, (int)rg[0], (int)rg[1], (int)rg[2], (int)rg[3]) : flower_in_brush(f, px, py, c.radius, c.is_square != 0);
	};
	flower_pod_t *const v = flowers + (size_t)t*capacity;
	uint32_t *const ax = aux ? aux + (size_t)t*capacity : nullptr, *const my_idx = idx + (size_t)t*capacity;
	uint32_t const cnt = min_u32(counts[t], capacity);
	uint32_t const m = tp_block_remove(cnt, my_idx, s_wave, [&](uint32_t i) {return removed(v[i]);}, [&](uint32_t dst, uint32_t src) {v[dst] = v[src]; if (ax) {ax[dst] = ax[src];}});
	__syncthreads(); // every thread has read the count
	if (tid == 0) {counts[t] = m;}
}

// ------------------------------------------------------------------ the grass draw lists of a tile batch for a camera (tile_t::draw_grass, src/tiled_mesh.cpp:1607-1664;
// terra_grassview.hpp).  k_grass_view: a workgroup of 16 waves per tile.
//  1. Every thread runs the tile test (uniform: a few dozen flops on scalars); a skipped tile and one beyond grass_thresh -- most tiles of a large batch -- read no
//     block and leave after zeroing their group counts.
//  2. Sweeps of 1024 blocks in scan order (one sweep at S = 128, whose latency 16 waves share): a thread runs the block test of its block (grass_view_block; the
//     back-face test loads the block's 6 x 6 zvals before it forms the first product) and leaves the block's key -- dropped, or lod*nrnd + bix -- as 16 bits.  The
//     first GV_LDS_KEYS keys of a tile lie in LDS (8 KB: every key up to S = 256), the rest in the tile's row of `keys` in global scratch (65 536 blocks at
//     S = 1024 would be 128 KB, more than a workgroup should ask for): one kernel and one walk for every tile size, a chunk of 64 keys comes from one or the other.
//     has_grass() is the OR of `ix != 0` over the sweeps, taken at the barrier that ends them.
//  3. The stable grouping, 1024 bins at a time (one pass at the reference's 6 x 16 bins): lane l of wave w owns bin 16*l + w and keeps its running sum in a register.
//     A wave walks the keys 64 at a time, one load a chunk, and for each of its bins takes the ballot of `key == bin`: the population count goes to the owner lane.
//     The counts go through LDS into bin order, are scanned there (wave scans and the waves' totals), and come back to the owners as the bins' offsets;
//     group_counts is written on the way.  A second walk of the same shape writes the instances: a matching lane's rank is its bin's running sum (read from the
//     owner lane) plus the matches below it in the ballot.  No atomics anywhere, so the order inside a group is the scan order by construction.
constexpr uint32_t GV_THREADS = 1024, GV_WAVES = GV_THREADS/64, GV_LDS_KEYS = 4096;
__global__ __launch_bounds__(GV_THREADS) void k_grass_view(grass_view_consts_t c, int32_t const *__restrict__ tile_xy, float const *__restrict__ zvals,
	terra_tile_stats const *__restrict__ stats, grass_block_pod_t const *__restrict__ blocks, uint8_t const *__restrict__ skip, uint32_t capacity, float *__restrict__ insts,
	uint32_t *__restrict__ aux, uint32_t *__restrict__ group_counts, uint32_t *__restrict__ counts, uint8_t *__restrict__ pass, uint16_t *keys)
{
	__shared__ uint32_t s_cnt[GV_THREADS], s_wave[GV_WAVES];
	__shared__ uint16_t s_keys[GV_LDS_KEYS];
	uint32_t const t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t const dim = c.dim, nb = dim*dim, nbins = GRASS_VIEW_LODS*c.nrnd;
	uint32_t *const gc = group_counts + (size_t)t*nbins;
	uint16_t *const ky = keys + (size_t)t*nb;
	float const mzmin = stats[t].mzmin, mzmax = stats[t].mzmax, radius = stats[t].radius;
	line_box_t const box = grass_view_box(c, tile_xy[2u*t], tile_xy[2u*t + 1u], mzmin, mzmax);
	grass_view_tile_t const tl = grass_view_tile(c, box.d, box.x1, box.y1, mzmin, mzmax, radius);
	int has = 0;
	if (!(skip && skip[t]) && tl.in_range) { // (uniform)
		size_t const zn = (size_t)(c.S + 2)*(size_t)(c.S + 2);
		float const *const zt = zvals + (size_t)t*zn;
		grass_block_pod_t const *const bl = blocks + (size_t)t*nb;
		for (uint32_t base = 0; base < nb; base += GV_THREADS) {
			uint32_t const i = base + tid;
			if (i < nb) {
				grass_block_pod_t const gb = bl[i];
				has |= (gb.ix != 0u);
				uint16_t const key = (uint16_t)grass_view_block(c, tl, i % dim, i / dim, gb.ix, gb.zmin, gb.zmax, zt);
				if (i < GV_LDS_KEYS) {s_keys[i] = key;} else {ky[i] = key;}
			}
		}
	}
	if (!__syncthreads_or(has)) { // skipped, too far away or no grass: nothing is drawn (the keys were not all written: they are not read)
		for (uint32_t b = tid; b < nbins; b += GV_THREADS) {gc[b] = 0u;}
		if (tid == 0) {counts[t] = 0u; if (pass) {pass[t] = GRASS_VIEW_NO_PASS;}}
		return;
	}
	if (tid == 0 && pass) {pass[t] = (uint8_t)tl.wpass;}
	auto key_at = [&](uint32_t j) -> uint32_t {return (j < nb) ? (uint32_t)((j < GV_LDS_KEYS) ? s_keys[j] : ky[j]) : GRASS_VIEW_DROPPED;}; // (one source per chunk of 64)
	float *const my_insts = insts + (size_t)t*capacity*2u;
	uint32_t *const my_aux = aux ? aux + (size_t)t*capacity : nullptr;
	uint64_t const below = (1ull << lane) - 1ull;
	uint32_t carry = 0; // the instances of the bins before b0
	for (uint32_t b0 = 0; b0 < nbins; b0 += GV_THREADS) {
		uint32_t const rem = nbins - b0, nl = (rem > wave) ? min_u32(64u, (rem - wave + GV_WAVES - 1u)/GV_WAVES) : 0u; // this wave's bins: b0 + 16*l + wave for l < nl
		uint32_t cnt = 0;
		for (uint32_t j0 = 0; j0 < nb && nl; j0 += 64u) {
			uint32_t const k = key_at(j0 + lane);
			if (__ballot(k != GRASS_VIEW_DROPPED) == 0ull) continue;
			for (uint32_t l = 0; l < nl; ++l) {
				uint64_t const m = __ballot(k == b0 + GV_WAVES*l + wave);
				if (lane == l) {cnt += (uint32_t)__popcll(m);}
			}
		}
		s_cnt[GV_WAVES*lane + wave] = cnt; // into bin order
		__syncthreads();
		uint32_t const v = s_cnt[tid];
		uint32_t incl = v;
		for (uint32_t d = 1; d < 64u; d <<= 1) {uint32_t const u = __shfl_up(incl, d); if (lane >= d) {incl += u;}}
		if (lane == 63u) {s_wave[wave] = incl;}
		if (b0 + tid < nbins) {gc[b0 + tid] = v;}
		__syncthreads();
		uint32_t before = 0, total = 0;
		for (uint32_t w = 0; w < GV_WAVES; ++w) {uint32_t const sw = s_wave[w]; if (w < wave) {before += sw;} total += sw;}
		s_cnt[tid] = carry + before + incl - v; // the bin's offset (each thread overwrites the count it alone has read)
		carry += total;
		__syncthreads();
		uint32_t pos = s_cnt[GV_WAVES*lane + wave];
		for (uint32_t j0 = 0; j0 < nb && nl; j0 += 64u) {
			uint32_t const j = j0 + lane, k = key_at(j);
			if (__ballot(k != GRASS_VIEW_DROPPED) == 0ull) continue;
			uint32_t const x = j % dim, y = j / dim;
			for (uint32_t l = 0; l < nl; ++l) {
				uint32_t const bin = b0 + GV_WAVES*l + wave;
				uint64_t const m = __ballot(k == bin);
				if (m == 0ull) continue;
				uint32_t const at = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)l);
				if (k == bin) {
					uint32_t const rank = at + (uint32_t)__popcll(m & below);
					if (rank < capacity) {
						my_insts[2u*rank] = (float)x*c.dx_step; my_insts[2u*rank + 1u] = (float)y*c.dy_step; // emplace_back(x*dx_step, y*dy_step) (:1651)
						if (my_aux) {my_aux[rank] = grass_view_aux(c, j, bin);}
					}
				}
				if (lane == l) {pos += (uint32_t)__popcll(m);}
			}
		}
		__syncthreads(); // the next pass rewrites s_cnt and s_wave
	}
	if (tid == 0) {counts[t] = carry;}
}

// ------------------------------------------------------------------ the terrain draw list of a tile batch for a camera (the head of tile_draw_t::draw,
// src/tiled_mesh.cpp:2844-2915; terra_terrainview.hpp), five launches on one stream:
//  1. k_terrain_view_tiles: a lane per tile runs terrain_view_tile -- centre, boxes, is_visible, use_as_occluder, the filters of :2867-2868, get_lod_level -- and
//     leaves status (a candidate as TV_DRAWN), dist, lod and whether the tile runs the occlusion test.
//  2. k_terrain_view_occluders: one workgroup compacts the occluders in batch order (tp_block_rank, the record kernels' ranking) and builds their 17 boxes, a lane a box.
//  3. k_terrain_view_occlusion: a workgroup of 256 lanes per tile; every tile but a candidate that is to be tested leaves at once.  Lane (q, s) = (sub-box of the
//     tile, column of the occluder).  The occluders are walked in order; an occluder's record is read at a uniform address (scalar loads), and the `intersected`
//     test of :2881 -- the tile's four top points against the occluder's mesh box -- is a uniform branch around everything else.  A lane then clips its sub-box's
//     centre against the mesh box and its four top points against its column.  "Any over s" is a 16-bit segment of the wave's ballot, "all over q" the four
//     segments of a wave and the four waves through LDS.  No atomics; the result does not depend on the order of the occluders.
//  4. k_terrain_view_lists: one workgroup walks the batch 256 tiles at a time: a lane writes its tile's four crack bytes (the neighbours' lod and presence through
//     the [n][9] table), the optional skip byte, the occluded tiles are appended in batch order (tp_emit), and the drawn tiles' (dist, batch index) keys are compacted in batch order, into
//     global scratch and, the first TV_ORDER_LDS of them, into LDS.  With at most TV_ORDER_LDS drawn tiles the order is made here: an entry's place after the sort
//     of :2915 is its rank by (dist, batch index) -- std::pair's operator< with the index in the pointer's place --, counted against the keys in LDS, which every
//     lane reads at the same address.
//  5. k_terrain_view_rank: the second path, for more drawn tiles than that: the same rank, a lane an entry over as many workgroups as it takes, against the keys in
//     global scratch (uniform addresses again).  It leaves at once when step 4 has made the order.
constexpr uint32_t TV_THREADS = 256, TV_ORDER_LDS = 1024;
static_assert(TV_THREADS == TREEP_THREADS, "tp_block_rank and tp_emit rank TREEP_THREADS threads");
__global__ __launch_bounds__(TV_THREADS) void k_terrain_view_tiles(terrain_view_consts_t c, terrain_view_in_t in, int32_t const *__restrict__ tile_xy, uint32_t n,
	uint8_t *__restrict__ status, float *__restrict__ dist, uint8_t *__restrict__ lod, uint8_t *__restrict__ test, reflect_tile_t *__restrict__ rt)
{
	uint32_t const t = blockIdx.x*TV_THREADS + threadIdx.x;
	if (t >= n) return;
	terrain_view_tile_t const o = terrain_view_tile(c, in, tile_xy, t);
	status[t] = (uint8_t)(o.status | (o.occluder ? TV_WAS_OCCLUDER : 0)); dist[t] = o.dist; lod[t] = o.lod; test[t] = o.test;
	if (rt) {rt[t] = reflect_tile(c, in, tile_xy, t, o.visible != 0);} // (the reflection pass: what the walk of :2630-2662 reads of a tile)
}
__global__ __launch_bounds__(TV_THREADS) void k_terrain_view_occluders(terrain_view_consts_t c, terrain_view_in_t in, int32_t const *__restrict__ tile_xy, uint32_t n,
	uint8_t const *__restrict__ status, terrain_view_occluder_t *occ, uint32_t *__restrict__ nocc)
{
	__shared__ uint32_t s_wave[TV_THREADS/64];
	uint32_t const tid = threadIdx.x;
	uint32_t count = 0;
	for (uint32_t base = 0; base < n; base += TV_THREADS) {
		uint32_t const t = base + tid;
		bool const ok = t < n && (status[t] & TV_WAS_OCCLUDER) != 0;
		uint32_t total;
		uint32_t const rank = tp_block_rank(ok, s_wave, total);
		if (ok) {occ[count + rank].tile = (int32_t)t; occ[count + rank].pad = 0;}
		count += total;
	}
	if (tid == 0) {*nocc = count;}
	__syncthreads(); // the tiles of the records, written by other lanes
	for (uint32_t i = tid; i < count*17u; i += TV_THREADS) {
		uint32_t const j = i/17u, s = i - j*17u;
		uint32_t const t = (uint32_t)occ[j].tile;
		terrain_view_geom_t const g = terrain_view_geom_of(c, in, tile_xy, t);
		float d[3][2];
		if (s == 16u) {terrain_view_mesh_box(g, in.stats[t].mzmin, in.stats[t].mzmax, d);}
		else {terrain_view_occluder_column(c, g, in.stats[t], s, d);}
		float *const o = (s == 16u) ? &occ[j].bc[0][0] : &occ[j].sub[s][0][0];
		for (int k = 0; k < 6; ++k) {o[k] = d[k >> 1][k & 1];}
	}
}
__global__ __launch_bounds__(TV_THREADS) void k_terrain_view_occlusion(terrain_view_consts_t c, terrain_view_in_t in, int32_t const *__restrict__ tile_xy,
	terrain_view_occluder_t const *__restrict__ occ, uint32_t const *__restrict__ nocc_p, uint8_t const *__restrict__ test, uint8_t *status, uint8_t *__restrict__ prov)
{
	__shared__ uint32_t s_all[TV_THREADS/64];
	uint32_t const t = blockIdx.x, tid = threadIdx.x, nocc = *nocc_p;
	if ((status[t] & TV_STATUS_MASK) != TV_DRAWN || !test[t] || nocc == 0u) { // (uniform)
		if (prov && tid == 0) {prov[t] = TV_STATE_NONE;}
		return;
	}
	terrain_view_geom_t const g = terrain_view_geom_of(c, in, tile_xy, t);
	uint32_t const q = tid >> 4, s = tid & 15u;
	float b[3][2];
	terrain_view_sub_box(g, in.stats[t], q, b);
	float const cx = 0.5f*(b[0][0] + b[0][1]), cy = 0.5f*(b[1][0] + b[1][1]), cz = 0.5f*(b[2][0] + b[2][1]); // get_cube_center()
	bool hidden = false;
	for (uint32_t j = 0; j < nocc; ++j) {
		terrain_view_occluder_t const &o = occ[j];
		if (o.tile == (int32_t)t) continue;                 // no self-occlusion (uniform)
		if (!terrain_view_top_any(c, g.bc, o.bc)) continue; // not in occluder_ixs (uniform)
		hidden = hidden || terrain_view_column_hides(c, o, s, b, cx, cy, cz);
	}
	unsigned long long const m = __ballot(hidden);
	bool all4 = true; // this wave's four sub-boxes: each hidden by some column
	for (uint32_t k = 0; k < 4u; ++k) {all4 = all4 && ((m >> (16u*k)) & 0xFFFFull) != 0ull;}
	if ((tid & 63u) == 0u) {s_all[tid >> 6] = all4 ? 1u : 0u;}
	__syncthreads();
	if (tid == 0) {
		bool const occluded = s_all[0] && s_all[1] && s_all[2] && s_all[3];
		if (prov) {prov[t] = occluded ? TV_STATE_OCCLUDED : TV_STATE_UNOCCLUDED; return;} // (the reflection pass: k_reflect_finish decides whether the test took place)
		if (occluded) {status[t] = (uint8_t)((status[t] & ~TV_STATUS_MASK) | TV_OCCLUDED);}
		if (in.occl_state) {in.occl_state[t] = occluded ? TV_STATE_OCCLUDED : TV_STATE_UNOCCLUDED;} // set_last_occluded (:2906)
	}
}
// rank of entry i (key di) among the m keys k[0 .. m): the entries before it by (dist, position); positions are in batch order
__device__ __forceinline__ uint32_t tv_rank(float const *k, uint32_t m, float di, uint32_t i) {
	uint32_t rank = 0;
	for (uint32_t j = 0; j < m; ++j) {rank += terrain_view_before(k[j], j, di, i) ? 1u : 0u;}
	return rank;
}
__global__ __launch_bounds__(TV_THREADS) void k_terrain_view_lists(int32_t const *__restrict__ nbr, uint32_t n, uint8_t const *__restrict__ status, float const *__restrict__ dist,
	uint8_t const *__restrict__ lod, uint8_t *__restrict__ crack, uint32_t *__restrict__ draw_order, uint32_t *__restrict__ occluded, uint32_t *__restrict__ counts,
	uint8_t *__restrict__ not_drawn, float *__restrict__ keys, uint32_t *__restrict__ key_tile)
{
	__shared__ uint32_t s_wave[TV_THREADS/64], s_tile[TV_ORDER_LDS];
	__shared__ float s_key[TV_ORDER_LDS];
	uint32_t const tid = threadIdx.x;
	uint32_t nd = 0, no = 0;
	for (uint32_t base = 0; base < n; base += TV_THREADS) {
		uint32_t const t = base + tid;
		uint32_t const me = (t < n) ? (uint32_t)(status[t] & TV_STATUS_MASK) : (uint32_t)TV_ABSENT;
		if (t < n) {
			uint32_t cr = 0;
			for (uint32_t k = 0; k < 4u; ++k) {
				int32_t const u = nbr[(size_t)t*9u + terrain_view_nbr_slot(k >> 1, k & 1u)];
				bool const adj = me == TV_DRAWN && u >= 0 && (status[u] & TV_STATUS_MASK) != TV_ABSENT;
				cr |= (adj ? terrain_view_crack_index(k >> 1, k & 1u, lod[t], lod[u]) : (uint32_t)TERRAIN_VIEW_NO_CRACK) << (8u*k);
			}
			for (uint32_t k = 0; k < 4u; ++k) {crack[(size_t)t*4u + k] = (uint8_t)(cr >> (8u*k));}
			if (not_drawn) {not_drawn[t] = (me != TV_DRAWN) ? 1 : 0;}
		}
		tp_emit(me == TV_OCCLUDED, [&] {return t;}, occluded, n, no, s_wave);
		uint32_t total;
		uint32_t const rank = tp_block_rank(me == TV_DRAWN, s_wave, total);
		if (me == TV_DRAWN) {
			float const d = dist[t];
			keys[nd + rank] = d; key_tile[nd + rank] = t;
			if (nd + rank < TV_ORDER_LDS) {s_key[nd + rank] = d; s_tile[nd + rank] = t;}
		}
		nd += total;
	}
	if (tid == 0) {counts[0] = nd; counts[1] = no;}
	if (nd > TV_ORDER_LDS) return; // k_terrain_view_rank makes the order
	__syncthreads();
	for (uint32_t i = tid; i < nd; i += TV_THREADS) {draw_order[tv_rank(s_key, nd, s_key[i], i)] = s_tile[i];}
}
__global__ __launch_bounds__(TV_THREADS) void k_terrain_view_rank(float const *__restrict__ keys, uint32_t const *__restrict__ key_tile, uint32_t const *__restrict__ counts,
	uint32_t *__restrict__ draw_order)
{
	uint32_t const nd = counts[0], i = blockIdx.x*TV_THREADS + threadIdx.x;
	if (nd <= TV_ORDER_LDS || i >= nd) return;
	draw_order[tv_rank(keys, nd, keys[i], i)] = key_tile[i];
}

// ------------------------------------------------------------------ the terrain draw list of reflection pass 1 (tile_draw_t::draw(1) with can_have_reflection, :2869 and
// :2630-2683; terra_waterview.hpp): the launches above with pass 1's LOD, and between the occlusion test and the lists the two kernels of :2869.
//  - k_terrain_view_tiles also leaves what the walk reads of a tile (reflect_tile_t: get_bcube(), is_visible() for :2657, has_water, all_water, the incoming state); k_terrain_view_occlusion leaves its result as a provisional byte (0 not
//    tested, 1 occluded, 2 not) instead of writing status and occl_state: a candidate's test does not depend on :2869, only whether it takes place.
//  - k_reflect_walk: one wave per tile; the lanes clear the visited bits in LDS -- one for every tile position of the batch's bounding box -- and lane 0 goes on: every
//    tile but a candidate is done at once, and so is a candidate that :2667-2669 decide; for the others it runs reflect_walk with the work list in LDS too.  was_last_occluded()
//    of a tile A met on the walk of tile T matters only where A has water, and there A's own answer at :2869 needs no walk (yes unless all_water): A was occluded
//    by this loop exactly when it precedes T in the batch, its provisional byte is 1 and it is not all_water -- else its incoming state counts.  So no walk waits for
//    another, and all of them are one launch.
//  - k_reflect_finish: a lane per tile turns the provisional bytes into status and occl_state: a candidate that :2869 drops gets status 6 and keeps its state.
constexpr uint32_t RF_THREADS = 64;
__global__ __launch_bounds__(RF_THREADS) void k_reflect_walk(reflect_consts_t const *cp, terra_tile_stats const *__restrict__ stats, int32_t const *__restrict__ tile_xy,
	int32_t const *__restrict__ nbr, reflect_tile_t const *__restrict__ rt, uint8_t const *__restrict__ status, uint8_t const *__restrict__ prov, reflect_box_t B,
	uint8_t *refl, uint8_t *reflect)
{
	extern __shared__ uint32_t s_rf[]; // [B.nwords] visited bits, [B.cap] work list
	for (uint32_t i = threadIdx.x; i < B.nwords; i += RF_THREADS) {s_rf[i] = 0u;}
	__syncthreads();
	if (threadIdx.x != 0) return;
	// Everything a walk reads sits at addresses that are uniform over the wave, so the compiler would keep all of it in scalar registers, run out of them and park
	// them in vector lanes.  One lane works: its values belong in vector registers.  Hiding the tile's index and the address of the constants (in device memory
	// for this) in vector registers puts them there.
	uint32_t t = blockIdx.x;
	asm volatile("" : "+v"(t), "+v"(cp));
	reflect_consts_t const c = *cp;
	uint32_t r = RF_NOT_ASKED;
	if ((status[t] & TV_STATUS_MASK) == TV_DRAWN) {
		reflect_tile_t const me = rt[t];
		r = reflect_without_walk(c.tv, me.flags);
		if (r == RF_NOT_ASKED) {
			reflect_corners_t const k = reflect_corners(c.tv, me.bc, stats[t].mzmax);
			uint32_t *const bits = s_rf;
			auto seen = [=](uint32_t u) {
				uint32_t const bit = ((uint32_t)tile_xy[2u*u] - (uint32_t)B.x0) + ((uint32_t)tile_xy[2u*u + 1u] - (uint32_t)B.y0)*B.w;
				if ((bit >> 5) >= B.nwords) return true; // (no tile of the batch lies outside its bounding box)
				uint32_t const w = bits[bit >> 5], m = 1u << (bit & 31u);
				bits[bit >> 5] = w | m;
				return (w & m) != 0u;
			};
			auto occluded = [=](uint32_t u) {
				uint32_t const f = rt[u].flags;
				return (u < t && prov[u] == TV_STATE_OCCLUDED && !(f & RT_ALL_WATER)) || (f & RT_OCCLUDED_IN) != 0u;
			};
			// (opaque per visit: the corners do not change along a walk, so the tests of the line clip that depend on them alone -- a dozen lane masks, two scalar
			// registers each -- would be hoisted out of the walk's loop, kept through it and spilled)
			auto pin = [](reflect_corners_t &q) {asm volatile("" : "+v"(q.p[0][0]), "+v"(q.p[0][1]), "+v"(q.p[0][2]), "+v"(q.p[1][0]), "+v"(q.p[1][1]), "+v"(q.p[1][2]));};
			r = reflect_walk(c, stats, nbr, rt, t, k, (int32_t *)(s_rf + B.nwords), B.cap, seen, occluded, pin) ? RF_WALK_FOUND : RF_WALK_NOTHING;
		}
	}
	refl[t] = (uint8_t)r;
	reflect[t] = (uint8_t)r; // (the caller's array, or `refl` again)
}
__global__ __launch_bounds__(TV_THREADS) void k_reflect_finish(uint32_t n, uint8_t const *__restrict__ prov, uint8_t const *__restrict__ refl, uint8_t *__restrict__ status,
	uint8_t *__restrict__ occl_state)
{
	uint32_t const t = blockIdx.x*TV_THREADS + threadIdx.x;
	if (t >= n || (status[t] & TV_STATUS_MASK) != TV_DRAWN) return;
	if (refl[t] < RF_HAS_WATER) {status[t] = (uint8_t)((status[t] & ~TV_STATUS_MASK) | TV_NO_REFLECTION); return;} // :2869: no set_last_occluded
	if (prov[t] == TV_STATE_NONE) return;
	if (prov[t] == TV_STATE_OCCLUDED) {status[t] = (uint8_t)((status[t] & ~TV_STATUS_MASK) | TV_OCCLUDED);}
	if (occl_state) {occl_state[t] = prov[t];} // set_last_occluded (:2906)
}

// ------------------------------------------------------------------ water quads and water caps of a tile batch (tile_t::is_water_visible, :2131-2133; the edge tests of
// tile_t::draw_water_cap, :2102-2119; terra_waterview.hpp).  k_water_view: one workgroup walks the batch 256 tiles at a time, twice.  First a lane takes a tile's
// four facts (present, has_water, within DRAW_DIST_TILES, is_visible) into a byte of global scratch, and the tiles with is_water_visible() are appended in batch
// order (tp_emit).  Then, with a status array, a lane reads its four neighbours' bytes through the [n][9] table and writes its cap mask.
__global__ __launch_bounds__(TV_THREADS) void k_water_view(terrain_view_consts_t c, terrain_view_in_t in, int32_t const *__restrict__ tile_xy, int32_t const *__restrict__ nbr, uint32_t n,
	uint8_t const *__restrict__ status, uint8_t *wv, uint32_t *__restrict__ water_list, uint8_t *__restrict__ cap_mask, uint32_t *__restrict__ counts)
{
	__shared__ uint32_t s_wave[TV_THREADS/64];
	uint32_t const tid = threadIdx.x;
	uint32_t nw = 0, nc = 0;
	for (uint32_t base = 0; base < n; base += TV_THREADS) {
		uint32_t const t = base + tid;
		uint32_t const w = (t < n) ? water_view_tile(c, in, tile_xy, t) : 0u;
		if (t < n) {wv[t] = (uint8_t)w;}
		tp_emit(t < n && water_view_listed(w), [&] {return t;}, water_list, n, nw, s_wave);
	}
	if (tid == 0) {counts[0] = nw;}
	if (!status) return;
	__syncthreads(); // the bytes of the neighbours, written by other lanes
	for (uint32_t base = 0; base < n; base += TV_THREADS) {
		uint32_t const t = base + tid;
		uint32_t const m = (t < n) ? water_view_caps(c, wv[t], status[t], nbr, wv, t) : 0u;
		if (t < n) {cap_mask[t] = (uint8_t)m;}
		uint32_t total;
		tp_block_rank(m != 0u, s_wave, total);
		nc += total;
	}
	if (tid == 0) {counts[1] = nc;}
}

// ------------------------------------------------------------------ the shadow-map plan of a tile batch (tile_t::setup_shadow_maps, src/tiled_mesh.cpp:981-1016, with
// update_range's deletion, :1416, pre_draw's loop, :2781-2799, and the queue of :2445-2448; terra_smapview.hpp), three launches on one stream:
//  1. k_smap_plan: a lane per tile runs smap_plan_tile and leaves the plan word, dist_scale, the box, the new state byte, the terrain flag and what the queue's rank
//     reads of the tile (its key, its position, whether it is present) as one 16-byte record.
//  2. k_smap_plan_lists: one workgroup walks the batch 256 tiles at a time and appends the receivers in batch order (tp_emit); the present tiles are counted on the way.
//  3. k_smap_plan_rank: k_terrain_view_rank's scheme on the queue: a lane per tile counts the present tiles that come after it in the sorted queue -- its place in
//     the order of pop_back.  The records pass through LDS 256 at a time, where every lane reads them at the same address (as k_terrain_view_lists' keys): read
//     from global memory at uniform addresses, a record a turn, the loop waited out one scalar load's latency per record (625 us for 4096 tiles, most of the call).
//     Launched only where a recomp_order is wanted.
// The casters (the head of tile_draw_t::draw_shadow_pass, :3025-3043, the filter of draw_tiles_shadow_pass, :3004-3018), two launches:
//  4. k_smap_geom: a lane per tile leaves the 64 bytes every render reads of it (centre, radius with water, get_bcube(), the xy of get_shadow_bcube(), three flags).
//  5. k_smap_casters: one workgroup per render, a lane per tile, SMC_THREADS tiles a turn.  The view, the light and the receiver's record sit at addresses that are
//     uniform over the workgroup.  Both lists are compacted in batch order by one ballot per list and wave and one prefix over the waves' counts (tp_block_rank2:
//     the two counts travel as the halves of one word, so the pair costs the two barriers of one).
// Why 1024 lanes a workgroup: a call has R workgroups, a few dozen against 256 compute units, so its time is one workgroup's walk through the batch, not the
// device's throughput; a turn costs two barriers and the latency of four 16-byte loads whatever the width, and 1024 lanes take a quarter of the turns of 256.  The
// test needs few registers (see tools/check_kernel_resources.py), so sixteen waves of it fit a compute unit.
constexpr uint32_t SMC_THREADS = 1024;
__global__ __launch_bounds__(TV_THREADS) void k_smap_plan(smap_consts_t c, terrain_view_in_t in, smap_plan_io_t io, int32_t const *__restrict__ tile_xy, uint32_t n,
	smap_rank_key_t *__restrict__ keys)
{
	uint32_t const t = blockIdx.x*TV_THREADS + threadIdx.x;
	if (t >= n) return;
	smap_plan_tile_t const o = smap_plan_tile(c, in, tile_xy, io.smap_state[t], t);
	smap_plan_store(io, o, t);
	smap_rank_key_t k; k.key = o.key; k.y = tile_xy[2u*t + 1u]; k.x = tile_xy[2u*t]; k.present = o.present;
	keys[t] = k;
}
__global__ __launch_bounds__(TV_THREADS) void k_smap_plan_lists(uint32_t n, uint32_t const *__restrict__ plan, smap_rank_key_t const *__restrict__ keys, uint32_t *__restrict__ receivers,
	uint32_t *__restrict__ counts, int recomp)
{
	__shared__ uint32_t s_wave[TV_THREADS/64];
	uint32_t const tid = threadIdx.x;
	uint32_t nr = 0, np = 0;
	for (uint32_t base = 0; base < n; base += TV_THREADS) {
		uint32_t const t = base + tid;
		tp_emit(t < n && (plan[t] & SMP_RECEIVER) != 0u, [&] {return t;}, receivers, n, nr, s_wave);
		uint32_t total;
		tp_block_rank(t < n && keys[t].present != 0u, s_wave, total);
		np += total;
	}
	if (tid == 0) {counts[0] = nr; counts[1] = recomp ? np : 0u;}
}
__global__ __launch_bounds__(TV_THREADS) void k_smap_plan_rank(smap_rank_key_t const *__restrict__ keys, uint32_t n, uint32_t *__restrict__ recomp_order) {
	__shared__ smap_rank_key_t s_keys[TV_THREADS];
	uint32_t const tid = threadIdx.x, t = blockIdx.x*TV_THREADS + tid;
	smap_rank_key_t me; me.key = 0.0f; me.y = 0; me.x = 0; me.present = 0u;
	if (t < n) {me = keys[t];}
	uint32_t place = 0;
	for (uint32_t base = 0; base < n; base += TV_THREADS) { // (every thread of the workgroup takes every turn: the barriers)
		uint32_t const u = base + tid, m = (n - base < TV_THREADS) ? n - base : TV_THREADS;
		__syncthreads(); // the turn before has read its records
		if (u < n) {s_keys[tid] = keys[u];}
		__syncthreads();
		place += smap_recomp_count(s_keys, m, base, me, t);
	}
	if (t < n && me.present) {recomp_order[place] = t;}
}
__global__ __launch_bounds__(TV_THREADS) void k_smap_geom(smap_consts_t c, terrain_view_in_t in, uint32_t const *__restrict__ decid_counts, int decid_trees_only,
	int32_t const *__restrict__ tile_xy, uint32_t n, smap_geom_t *__restrict__ geom)
{
	uint32_t const t = blockIdx.x*TV_THREADS + threadIdx.x;
	if (t >= n) return;
	geom[t] = smap_geom(c, in, decid_counts, decid_trees_only, tile_xy, t);
}
// tp_block_rank for two flags at once in a workgroup of THREADS threads: the ranks of the calling thread among the threads with f0 and among those with f1, in thread
// order, and their numbers (uniform); two barriers
template<uint32_t THREADS> __device__ __forceinline__ void tp_block_rank2(bool f0, bool f1, uint32_t *s_wave, uint32_t &r0, uint32_t &r1, uint32_t &n0, uint32_t &n1) {
	static_assert(THREADS % 64 == 0 && THREADS <= 1024, "whole waves; a count fits half a word");
	uint32_t const lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	unsigned long long const m0 = __ballot(f0), m1 = __ballot(f1);
	if (lane == 0) {s_wave[w] = smap_rank2_word(m0, m1);}
	__syncthreads();
	smap_rank2_t const q = smap_rank2(s_wave, THREADS/64, w, lane, m0, m1); // (terra_smapview.hpp: the arithmetic the host check runs too)
	__syncthreads();
	r0 = q.r0; r1 = q.r1; n0 = q.n0; n1 = q.n1;
}
__global__ __launch_bounds__(SMC_THREADS) void k_smap_casters(smap_geom_t const *__restrict__ geom, uint32_t n, uint32_t const *__restrict__ recv, view_pod_t const *__restrict__ views,
	float const *__restrict__ bsm, float const *__restrict__ lpos, int decid_trees_only, int inc_adj_smap, uint32_t *__restrict__ to_draw, uint32_t *__restrict__ terrain,
	uint32_t *__restrict__ counts, uint8_t *__restrict__ not_drawn, uint8_t *__restrict__ status)
{
	__shared__ uint32_t s_wave[SMC_THREADS/64];
	uint32_t const r = blockIdx.x, tid = threadIdx.x;
	size_t const row = (size_t)r*n;
	view_pod_t const &v = views[r]; // (the driver's copy: near_ is 0 already, :3032)
	float const mult = bsm[r];
	smap_recv_t const rc = smap_recv(geom, n, recv[r], lpos + 3u*(size_t)r);
	uint32_t nd = 0, nt = 0;
	for (uint32_t base = 0; base < n; base += SMC_THREADS) {
		uint32_t const t = base + tid;
		uint32_t w = 0u;
		if (t < n) { // (the lane's own copy of its record, four 16-byte loads: with the test reading the record through a reference the kernel kept an 8-byte frame that nothing used)
			smap_geom_t const g = geom[t];
			w = smap_cast_tile(v, mult, g, rc, decid_trees_only, inc_adj_smap);
			not_drawn[row + t] = (w & 1u) ? 0 : 1;
		}
		uint32_t r0, r1, n0, n1;
		tp_block_rank2<SMC_THREADS>((w & 1u) != 0u, (w & 2u) != 0u, s_wave, r0, r1, n0, n1);
		if (w & 1u) {to_draw[row + nd + r0] = t;} // (nd + r0 < n: the ranks count tiles of the batch)
		if (w & 2u) {terrain[row + nt + r1] = t;}
		nd += n0; nt += n1;
	}
	if (tid == 0) {counts[2u*r] = nd; counts[2u*r + 1u] = nt; status[r] = rc.ok ? 0 : (uint8_t)SMC_NO_TILE;}
}

// ------------------------------------------------------------------ the clouds of a tile batch (tile_cloud_manager_t, src/tiled_mesh.cpp:1710-1827; terra_clouds.hpp).
// The wind step is order dependent only where a cloud crosses from one tile to another, and a cloud's way through a call depends on nothing but the cloud:
//  - k_cloud_mark: a lane per tile follows each of its records through the call (cloud_path) and marks every tile that sends or receives (a byte store of 1).
//  - k_cloud_tiles: a lane per unmarked tile runs that tile's update_tile_clouds; it reads and writes the tile alone.
//  - k_cloud_tail: one workgroup.  Its lanes list the marked tiles in batch order; after the barrier lane 0 replays them with the literal loop, which hands clouds
//    only to marked tiles; after a second barrier the lanes add the other tiles' counts to the replayed tiles' counts at their turns.  Nothing waits for another workgroup: the three steps are three launches.
// The draw list: k_cloud_view, a lane per record slot, leaves the stage byte and appends a listed instance to scratch in any order; k_cloud_rank puts an instance at
// its rank by (dist_sq, tile, slot), a total order, so the list does not depend on the order of the appends.
constexpr uint32_t CLD_THREADS = 256;
static_assert(CLD_THREADS == TREEP_THREADS, "tp_emit and tp_block_rank rank TREEP_THREADS threads");
__global__ __launch_bounds__(CLD_THREADS) void k_cloud_mark(cloud_consts_t c, int32_t const *__restrict__ nbr, uint32_t n, cloud_tile_pod_t const *__restrict__ state,
	cloud_pod_t const *__restrict__ clouds, uint8_t *touched)
{
	uint32_t const t = blockIdx.x*CLD_THREADS + threadIdx.x;
	if (t < n) {cloud_mark_tile(c, nbr, state, clouds, t, n, touched);}
}
__global__ __launch_bounds__(CLD_THREADS) void k_cloud_tiles(cloud_consts_t c, int32_t const *__restrict__ tile_xy, int32_t const *__restrict__ nbr, uint32_t n,
	uint8_t const *__restrict__ touched, cloud_tile_pod_t *state, cloud_pod_t *clouds)
{
	uint32_t const t = blockIdx.x*CLD_THREADS + threadIdx.x;
	if (t < n && !touched[t]) {cloud_update_tile_alone(c, tile_xy, nbr, state, clouds, t);}
}
__global__ __launch_bounds__(CLD_THREADS) void k_cloud_tail(cloud_consts_t c, int32_t const *__restrict__ tile_xy, int32_t const *__restrict__ nbr, uint32_t n,
	uint8_t const *__restrict__ touched, uint32_t *order, cloud_tile_pod_t *state, cloud_pod_t *clouds, uint32_t *__restrict__ total)
{
	__shared__ uint32_t s_wave[CLD_THREADS/64], s_sum;
	uint32_t const tid = threadIdx.x;
	uint32_t nm = 0;
	for (uint32_t base = 0; base < n; base += CLD_THREADS) {
		uint32_t const t = base + tid;
		tp_emit(t < n && touched[t] != 0, [&] {return t;}, order, n, nm, s_wave);
	}
	__syncthreads(); // order[] is complete
	if (tid == 0) { // (a replayed tile's part of `num` is its count right after its turn: an earlier tile's list may still grow)
		uint32_t num = 0;
		for (uint32_t k = 0; k < nm; ++k) {uint32_t const t = order[k]; cloud_update_tile(c, tile_xy, nbr, state, clouds, t); num += state[t].count;}
		s_sum = num;
	}
	__syncthreads();
	if (!total) return;
	uint32_t sum = 0;
	for (uint32_t t = tid; t < n; t += CLD_THREADS) {sum += touched[t] ? 0u : state[t].count;}
	atomicAdd(&s_sum, sum);
	__syncthreads();
	if (tid == 0) {*total = s_sum;}
}
__global__ __launch_bounds__(CLD_THREADS) void k_cloud_view(cloud_view_consts_t c, tree_place_consts_t const *__restrict__ consts, uint32_t nrec, terra_tile_stats const *__restrict__ stats,
	cloud_tile_pod_t const *__restrict__ state, cloud_pod_t const *__restrict__ clouds, uint8_t *__restrict__ stage, cloud_inst_pod_t *__restrict__ found, uint32_t *cnt)
{
	uint32_t const i = blockIdx.x*CLD_THREADS + threadIdx.x;
	if (i >= nrec) return;
	uint32_t const t = i/c.capacity, k = i%c.capacity;
	uint32_t stg = CLV_NONE;
	if (k < state[t].count) {
		cloud_inst_pod_t o; o.tile = t; o.slot = k;
		stg = cloud_view_record(c, clouds[i], stats[t].mzmin, stats[t].mzmax, [&](float x, float y) {return tree_exact_zval(*consts, x, y);}, o);
		if (stg == CLV_LISTED) {found[atomicAdd(cnt, 1u)] = o;} // (at most one per slot: below nrec)
	}
	stage[i] = (uint8_t)stg;
}
__global__ __launch_bounds__(CLD_THREADS) void k_cloud_rank(cloud_inst_pod_t const *__restrict__ found, uint32_t const *__restrict__ cnt_p, cloud_inst_pod_t *__restrict__ list,
	uint32_t *__restrict__ list_count)
{
	__shared__ cloud_inst_pod_t s_in[CLD_THREADS];
	uint32_t const cnt = *cnt_p, i = blockIdx.x*CLD_THREADS + threadIdx.x;
	if (i == 0) {*list_count = cnt;}
	if (blockIdx.x*CLD_THREADS >= cnt) return; // (uniform)
	cloud_inst_pod_t me = found[(i < cnt) ? i : 0u];
	uint32_t rank = 0;
	for (uint32_t base = 0; base < cnt; base += CLD_THREADS) {
		uint32_t const m = (cnt - base < CLD_THREADS) ? cnt - base : CLD_THREADS;
		__syncthreads(); // the reads of the last round
		if (threadIdx.x < m) {s_in[threadIdx.x] = found[base + threadIdx.x];}
		__syncthreads();
		for (uint32_t j = 0; j < m; ++j) {rank += cloud_inst_before(s_in[j], me) ? 1u : 0u;}
	}
	if (i < cnt) {list[rank] = me;}
}

// ------------------------------------------------------------------ the pine and palm tree draw lists of a tile batch for a camera (tile_t::draw_pine_trees,
// src/tiled_mesh.cpp:1465-1526; terra_treeview.hpp).  k_tree_view: a workgroup of 256 lanes per tile; a skipped tile and one without records leave at once.
//  1. A sweep over the tile's records, a lane a record: the record's size and trunk cylinder (tree_view_record), the counts of the valid, pine and palm records and
//     the min / max union of the boxes (calc_bcube), reduced over the wave with shuffles and over the four waves through LDS.
//  2. One lane takes the tile-level decisions (tree_view_tile) and broadcasts them through LDS.
//  3. A second sweep in record order: the trunk byte of every record, and the pine entries of leaf_list -- appended in record order (tp_emit), or, in the tile that
//     holds the camera, compacted as (p2p_dist_sq, index) pairs and placed by their rank among the pairs (as k_terrain_view_rank places a tile).  A third sweep
//     appends the palm entries where draw_non_pine_leaves draws them.
//  4. The instance lists, pine then palm: a stable counting sort by id (tp_sort_by_id).  The entries are compacted as (id, index) pairs in record order; up to
//     TREE_VIEW_RANK_MAX of them, or with an instance table beyond TREE_VIEW_LDS_IDS entries, every pair is placed by its rank like the camera tile's list.  More
//     take a histogram of the ids in LDS (atomic adds: only counts), an exclusive scan of it, then emission in record order: the waves take turns, and in a wave
//     the lanes that share an id are ranked by a ballot, so the order inside an id is the record index and no atomic decides an order.
// The pairs lie in LDS for capacities up to TREE_VIEW_LDS_KEYS, else in the tile's part of the driver's scratch.  The sweeps recompute a record's geometry instead
// of keeping it: a few dozen flops against a round trip through memory, and the records come from L2 after the first sweep.
constexpr uint32_t TRV_THREADS = 256;
static_assert(TRV_THREADS == TREEP_THREADS, "tp_block_rank and tp_emit rank TREEP_THREADS threads");
template<bool FLOATKEY> __device__ __forceinline__ uint32_t trv_rank(uint32_t const *key, uint32_t const *idx, uint32_t m, uint32_t ki, uint32_t ii) {
	uint32_t rank = 0;
	for (uint32_t j = 0; j < m; ++j) {
		bool const b = FLOATKEY ? tree_view_before_f(__uint_as_float(key[j]), idx[j], __uint_as_float(ki), ii) : tree_view_before_u(key[j], idx[j], ki, ii);
		rank += b ? 1u : 0u;
	}
	return rank;
}
// ---- a stable counting sort by id of the entries of a sequence, for the workgroup (the instance lists of k_tree_view, the billboard lists of k_decid_view):
// positions [0, m) of a sequence; entry(p, id): does position p enter the list, and with which id (< nid); store(at, id, p) -> the number of entries (uniform).
// The entries are compacted first, as (id, position) pairs in sequence order.  Up to RANK_MAX of them, or with a table beyond the LDS bins, every pair is
// placed by its rank among the pairs: n/256 rounds of n comparisons, which for the few hundred entries of a real tile is far less than the turns below.  More
// entries take the histogram: its emission costs a turn per wave and chunk and in it a step per distinct id, whatever the number of entries.
template<uint32_t BINS, uint32_t RANK_MAX, class ENTRY, class STORE> __device__ __forceinline__ uint32_t tp_sort_by_id(uint32_t nid, uint32_t m, ENTRY entry, STORE store, uint32_t *s_hist, uint32_t *s_wave,
	uint32_t *kbuf, uint32_t *ibuf)
{
	uint32_t const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t n = 0;
	for (uint32_t base = 0; base < m; base += TREEP_THREADS) {
		uint32_t id = 0, tot;
		bool const e = base + tid < m && entry(base + tid, id);
		uint32_t const rank = tp_block_rank(e, s_wave, tot);
		if (e) {kbuf[n + rank] = id; ibuf[n + rank] = base + tid;}
		n += tot;
	}
	__syncthreads();
	if (n == 0u) return 0u; // (uniform)
	if (nid > BINS || n <= RANK_MAX) {
		for (uint32_t i = tid; i < n; i += TREEP_THREADS) {store(trv_rank<false>(kbuf, ibuf, n, kbuf[i], ibuf[i]), kbuf[i], ibuf[i]);}
		__syncthreads(); // the pairs are reused
		return n;
	}
	for (uint32_t b = tid; b < nid; b += TREEP_THREADS) {s_hist[b] = 0u;}
	__syncthreads();
	for (uint32_t i = tid; i < n; i += TREEP_THREADS) {atomicAdd(&s_hist[kbuf[i]], 1u);}
	__syncthreads();
	// exclusive scan of the nid counts: lane q owns bins PER*q .. PER*q + PER - 1
	static_assert(BINS % TREEP_THREADS == 0, "the scan gives every lane the same number of bins");
	constexpr uint32_t PER = BINS/TREEP_THREADS;
	uint32_t v[PER], sum = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {uint32_t const b = PER*tid + k; v[k] = (b < nid) ? s_hist[b] : 0u; sum += v[k];}
	uint32_t incl = sum;
	for (uint32_t d = 1; d < 64u; d <<= 1) {uint32_t const u = __shfl_up(incl, d); if (lane >= d) {incl += u;}}
	if (lane == 63u) {s_wave[wave] = incl;}
	__syncthreads();
	uint32_t before = 0;
	for (uint32_t w = 0; w < wave; ++w) {before += s_wave[w];}
	uint32_t at = before + incl - sum;
#pragma unroll
	for (uint32_t k = 0; k < PER; ++k) {uint32_t const b = PER*tid + k; if (b < nid) {s_hist[b] = at;} at += v[k];}
	__syncthreads();
	uint64_t const below = (1ull << lane) - 1ull;
	for (uint32_t base = 0; base < n; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool const e = i < n;
		uint32_t const id = e ? kbuf[i] : 0u;
		for (uint32_t w = 0; w < TREEP_THREADS/64; ++w) { // the waves in sequence order
			if (wave == w) {
				uint64_t rem = __ballot(e);
				while (rem) {
					int const leader = __ffsll((unsigned long long)rem) - 1;
					uint32_t const lid = (uint32_t)__shfl((int)id, leader);
					uint64_t const mm = __ballot(e && id == lid);
					uint32_t const start = s_hist[lid]; // (every lane reads before the leader writes)
					if (e && id == lid) {store(start + (uint32_t)__popcll(mm & below), id, ibuf[i]);}
					if ((int)lane == leader) {s_hist[lid] = start + (uint32_t)__popcll(mm);}
					rem &= ~mm;
				}
			}
			__syncthreads();
		}
	}
	return n;
}
// one instance list of the tile (PINE: draw_pine_insts, else draw_palm_insts) -> its count (uniform)
template<bool PINE> __device__ __forceinline__ uint32_t trv_insts(tree_view_consts_t const &c, tree_view_tile_t const &tl, tree_inst_pod_t const *__restrict__ insts,
	tree_place_pod_t const *__restrict__ recs, trunk_override_pod_t const *__restrict__ ovs, uint32_t cnt, tree_view_inst_pod_t *__restrict__ out, uint32_t *s_hist, uint32_t *s_wave,
	uint32_t *kbuf, uint32_t *ibuf)
{
	bool const all = PINE ? tl.draw_all_near != 0 : tl.all_visible != 0;
	auto entry = [&](uint32_t i, uint32_t &id) -> bool { // does record i enter the list, and with which id
		tree_view_rec_t rec;
		if (recs[i].inst < 0 || !tree_view_record(c, insts, recs[i], ovs ? ovs + i : nullptr, rec)) return false;
		if (PINE ? !is_pine_tree_type(rec.type) : rec.type != T_PALM) return false;
		id = (uint32_t)recs[i].inst;
		return all || tree_view_leaves_visible(c, rec);
	};
	auto store = [&](uint32_t at, uint32_t id, uint32_t i) {out[at].id = id; for (int q = 0; q < 3; ++q) {out[at].pt[q] = recs[i].pos[q];}};
	return tp_sort_by_id<TREE_VIEW_LDS_IDS, TREE_VIEW_RANK_MAX>(c.a.num_insts, cnt, entry, store, s_hist, s_wave, kbuf, ibuf);
}
__global__ __launch_bounds__(TRV_THREADS) void k_tree_view(tree_view_consts_t c, int32_t const *__restrict__ tile_xy, tree_inst_pod_t const *__restrict__ insts,
	terra_tile_stats const *__restrict__ stats, uint8_t const *__restrict__ skip, float const *__restrict__ trmax, tree_place_pod_t const *__restrict__ pine,
	uint32_t const *__restrict__ counts, trunk_override_pod_t const *__restrict__ ov, tree_view_tile_pod_t *__restrict__ tile_out, float *__restrict__ bcube,
	tree_view_inst_pod_t *__restrict__ pine_insts, tree_view_inst_pod_t *__restrict__ palm_insts, uint32_t *__restrict__ inst_counts, uint32_t *__restrict__ leaf_list,
	uint32_t *__restrict__ leaf_counts, uint8_t *__restrict__ trunk, uint32_t *keys)
{
	__shared__ uint32_t s_wave[TRV_THREADS/64], s_cnt[TRV_THREADS/64][4], s_key[TREE_VIEW_LDS_KEYS], s_idx[TREE_VIEW_LDS_KEYS], s_hist[TREE_VIEW_LDS_IDS];
	__shared__ float s_box[TRV_THREADS/64][6];
	__shared__ tree_view_tile_t s_tile;
	uint32_t const t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t const cnt = (skip && skip[t]) ? 0u : min_u32(counts[t], c.cap); // (uniform)
	auto leave_empty = [&] {
		if (tid < 6u) {bcube[(size_t)t*6u + tid] = 0.0f;}
		if (tid == 0) {
			tree_view_tile_pod_t z; z.dscale = 0.0f; z.weight = 0.0f; z.flags = 0u; z.num_pine = z.num_palm = z.num_trees = z.leaf_written = z.pad = 0u;
			tile_out[t] = z; inst_counts[2u*t] = inst_counts[2u*t + 1u] = 0u; leaf_counts[2u*t] = leaf_counts[2u*t + 1u] = 0u;
		}
	};
	if (cnt == 0u) {leave_empty(); return;}
	tree_place_pod_t const *const recs = pine + (size_t)t*c.cap;
	trunk_override_pod_t const *const ovs = ov ? ov + (size_t)t*c.cap : nullptr;
	// 1. calc_bcube and the counts
	float const INF = __builtin_inff();
	float box[6] = {INF, -INF, INF, -INF, INF, -INF};
	uint32_t nv = 0, np = 0, nm = 0, nb = 0;
	for (uint32_t i = tid; i < cnt; i += TRV_THREADS) {
		tree_view_rec_t rec;
		if (!tree_view_record(c, insts, recs[i], ovs ? ovs + i : nullptr, rec)) continue;
		++nv; np += is_pine_tree_type(rec.type) ? 1u : 0u; nm += (rec.type == T_PALM) ? 1u : 0u;
		float d[6];
		if (!tree_view_bounds(rec, d)) continue;
		++nb;
		box_union(box, d);
	}
	for (int off = 32; off; off >>= 1) {
		nv += __shfl_xor(nv, off); np += __shfl_xor(np, off); nm += __shfl_xor(nm, off); nb += __shfl_xor(nb, off);
#pragma unroll
		for (int k = 0; k < 6; k += 2) {box[k] = min_std(box[k], __shfl_xor(box[k], off)); box[k + 1] = max_std(box[k + 1], __shfl_xor(box[k + 1], off));}
	}
	if (lane == 0) {
		s_cnt[wave][0] = nv; s_cnt[wave][1] = np; s_cnt[wave][2] = nm; s_cnt[wave][3] = nb;
#pragma unroll
		for (int k = 0; k < 6; ++k) {s_box[wave][k] = box[k];}
	}
	__syncthreads();
	nv = np = nm = nb = 0;
	for (uint32_t w = 0; w < TRV_THREADS/64; ++w) {nv += s_cnt[w][0]; np += s_cnt[w][1]; nm += s_cnt[w][2]; nb += s_cnt[w][3];}
	if (nv == 0u) {leave_empty(); return;} // pine_trees.empty() (:1468) (uniform)
	// 2. the tile's decisions
	if (tid == 0) {
		float bc[6];
#pragma unroll
		for (int k = 0; k < 6; k += 2) {
			float lo = s_box[0][k], hi = s_box[0][k + 1];
			for (uint32_t w = 1; w < TRV_THREADS/64; ++w) {lo = min_std(lo, s_box[w][k]); hi = max_std(hi, s_box[w][k + 1]);}
			bc[k] = nb ? lo : 0.0f; bc[k + 1] = nb ? hi : 0.0f;
		}
#pragma unroll
		for (int k = 0; k < 6; ++k) {bcube[(size_t)t*6u + k] = bc[k];}
		s_tile = tree_view_tile(c, tile_xy[2u*t], tile_xy[2u*t + 1u], stats[t], trmax ? trmax[t] : 0.0f, nv, np, nm, bc);
	}
	__syncthreads();
	tree_view_tile_t const tl = s_tile;
	uint32_t *const kbuf = (c.cap > TREE_VIEW_LDS_KEYS) ? keys + (size_t)t*c.cap*2u : s_key, *const ibuf = (c.cap > TREE_VIEW_LDS_KEYS) ? kbuf + c.cap : s_idx;
	uint32_t *const ll = leaf_list + (size_t)t*c.cap;
	// 3. the trunk bytes and the pine entries of leaf_list
	uint32_t nl = 0;
	int skipped = 0;
	for (uint32_t base = 0; base < cnt; base += TRV_THREADS) {
		uint32_t const i = base + tid;
		tree_view_rec_t rec;
		bool const valid = i < cnt && tree_view_record(c, insts, recs[i], ovs ? ovs + i : nullptr, rec);
		if (i < cnt) {
			uint8_t const b = (valid && tl.trunks) ? tree_view_trunk(c, rec, tl.all_visible != 0) : (uint8_t)0;
			trunk[(size_t)t*c.cap + i] = b; skipped |= (b == 1) ? 1 : 0;
		}
		if (tl.pine_list) { // (uniform)
			bool const e = valid && is_pine_tree_type(rec.type) && tree_view_leaves_visible(c, rec);
			if (!tl.pine_sorted) {tp_emit(e, [&] {return i;}, ll, c.cap, nl, s_wave);}
			else {
				uint32_t tot;
				uint32_t const rank = tp_block_rank(e, s_wave, tot);
				if (e) {kbuf[nl + rank] = __float_as_uint(tree_view_sort_key(c, rec.pos)); ibuf[nl + rank] = i;}
				nl += tot;
			}
		}
	}
	skipped = __syncthreads_or(skipped); // (also: the pairs are complete)
	if (tl.pine_sorted) {
		for (uint32_t i = tid; i < nl; i += TRV_THREADS) {ll[trv_rank<true>(kbuf, ibuf, nl, kbuf[i], ibuf[i])] = ibuf[i];}
		__syncthreads(); // the pairs are reused
	}
	uint32_t npl = 0;
	if (tl.palm_list) { // draw_non_pine_leaves(0, 1, 0, ..): behind the pine entries
		for (uint32_t base = 0; base < cnt; base += TRV_THREADS) {
			uint32_t const i = base + tid;
			tree_view_rec_t rec;
			bool const e = i < cnt && tree_view_record(c, insts, recs[i], ovs ? ovs + i : nullptr, rec) && rec.type == T_PALM && tree_view_leaves_visible(c, rec);
			tp_emit(e, [&] {return i;}, ll + nl, c.cap - nl, npl, s_wave);
		}
	}
	// 4. the instance lists
	uint32_t npi = 0, nmi = 0;
	if (tl.pine_insts) {npi = trv_insts<true>(c, tl, insts, recs, ovs, cnt, pine_insts + (size_t)t*c.cap, s_hist, s_wave, kbuf, ibuf);}
	if (tl.palm_insts) {nmi = trv_insts<false>(c, tl, insts, recs, ovs, cnt, palm_insts + (size_t)t*c.cap, s_hist, s_wave, kbuf, ibuf);}
	if (tid == 0) {
		tree_view_tile_pod_t o = tl.out;
		if (skipped) {o.flags = (o.flags & ~(uint32_t)TRV_TRUNK_MASK) | TRV_TRUNK_POLY_SKIPPED;}
		o.leaf_written = nl + npl;
		tile_out[t] = o;
		inst_counts[2u*t] = npi; inst_counts[2u*t + 1u] = nmi;
		leaf_counts[2u*t] = tl.pine_list ? nl : tree_view_render_all(c, tl); leaf_counts[2u*t + 1u] = npl;
	}
}

// ------------------------------------------------------------------ the scenery draw lists of a tile batch for a camera (tile_t::draw_scenery, src/tiled_mesh.cpp:1580-1592;
// terra_sceneryview.hpp).  k_scenery_view: a workgroup of 256 lanes per tile.
//  1. One lane reads the tile's centre and radius, forms get_scenery_dist_scale() and broadcasts the decision through LDS: a dropped tile -- most tiles of a large
//     batch -- leaves here, like a skipped or an empty one, with a zero record and zero counts.
//  2. A sweep over the tile's records, a lane a record: the draw word, size_scale and dist of every record (scenery_view_record), and the number of records in each of
//     the 16 streams (the 13 groups with the pld groups split by kind) -- a ballot per stream, lane s of a wave keeps the wave's count of stream s.  The counts of
//     the waves meet in LDS; one lane turns them into the streams' starts and writes group_counts and the tile record.
//  3. A second sweep in chunks of 256 records: a record's streams follow from its kind and its own draw word; per chunk and stream a ballot ranks the lanes of a wave,
//     the waves' counts of the chunk give the start of a wave, and the running starts advance by the chunk's totals.  So every list comes out in record order for any
//     number of records, and no atomic decides a position.  tp_block_rank would rank one stream with two barriers; the 16 streams share three barriers per chunk here.
constexpr uint32_t SCVW_THREADS = 256, SCVW_WAVES = SCVW_THREADS/64;
static_assert(SCV_STREAMS <= 64, "lane s of a wave counts stream s");
__global__ __launch_bounds__(SCVW_THREADS) void k_scenery_view(scenery_view_consts_t c, int32_t const *__restrict__ tile_xy, terra_tile_stats const *__restrict__ stats,
	uint8_t const *__restrict__ skip, scenery_place_pod_t const *__restrict__ objs, uint32_t const *__restrict__ counts, float const *__restrict__ rov,
	scenery_view_tile_pod_t *__restrict__ tile_out, uint32_t *draw, float *__restrict__ size_scale, float *__restrict__ dist, uint32_t *__restrict__ list,
	uint32_t *__restrict__ group_counts)
{
	__shared__ uint32_t s_w[SCVW_WAVES][SCV_STREAMS], s_base[SCV_STREAMS], s_total;
	__shared__ float s_dist_scale;
	__shared__ int s_go;
	uint32_t const t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t const cnt = (skip && skip[t]) ? 0u : min_u32(counts[t], c.cap); // (uniform)
	auto leave_empty = [&] {
		if (tid < SCV_GROUPS) {group_counts[(size_t)t*SCV_GROUPS + tid] = 0u;}
		if (tid == 0) {scenery_view_tile_pod_t z; z.dist_scale = 0.0f; z.scale_val = 0.0f; z.flags = z.num_records = z.list_written = 0u; z.pad[0] = z.pad[1] = z.pad[2] = 0u; tile_out[t] = z;}
	};
	if (cnt == 0u) {leave_empty(); return;}
	// 1. the tile
	if (tid == 0) {
		terra_tile_stats const &st = stats[t];
		float ds;
		s_go = scenery_view_tile(c, tile_xy[2u*t], tile_xy[2u*t + 1u], st.mzmin, st.mzmax, st.radius, ds) ? 1 : 0;
		s_dist_scale = ds;
	}
	__syncthreads();
	if (!s_go) {leave_empty(); return;} // (uniform)
	scenery_place_pod_t const *const recs = objs + (size_t)t*c.cap;
	size_t const o0 = (size_t)t*c.cap;
	// 2. the records
	uint32_t mine = 0;
	for (uint32_t base = 0; base < cnt; base += SCVW_THREADS) {
		uint32_t const i = base + tid;
		uint32_t streams = 0;
		if (i < cnt) {
			scenery_view_rec_t const r = scenery_view_record(c, recs[i], rov ? rov[o0 + i] : 0.0f);
			draw[o0 + i] = r.word; size_scale[o0 + i] = r.size_scale; dist[o0 + i] = r.dist;
			streams = r.streams;
		}
#pragma unroll
		for (uint32_t s = 0; s < SCV_STREAMS; ++s) {
			uint32_t const m = (uint32_t)__popcll(__ballot((streams >> s) & 1u));
			if (lane == s) {mine += m;}
		}
	}
	if (lane < SCV_STREAMS) {s_w[wave][lane] = mine;}
	__syncthreads();
	if (tid == 0) {
		uint32_t at = 0, groups[SCV_GROUPS];
#pragma unroll
		for (uint32_t g = 0; g < SCV_GROUPS; ++g) {groups[g] = 0u;}
#pragma unroll
		for (uint32_t s = 0; s < SCV_STREAMS; ++s) {
			uint32_t m = 0;
			for (uint32_t w = 0; w < SCVW_WAVES; ++w) {m += s_w[w][s];}
			s_base[s] = at; at += m;
			groups[scenery_view_group(s)] += m;
		}
#pragma unroll
		for (uint32_t g = 0; g < SCV_GROUPS; ++g) {group_counts[(size_t)t*SCV_GROUPS + g] = groups[g];}
		s_total = at;
		scenery_view_tile_pod_t o;
		o.dist_scale = s_dist_scale; o.scale_val = c.scale_val; o.flags = scenery_view_tile_flags(c); o.num_records = cnt; o.list_written = min_u32(at, c.list_cap);
		o.pad[0] = o.pad[1] = o.pad[2] = 0u;
		tile_out[t] = o;
	}
	__syncthreads();
	if (s_total == 0u || c.list_cap == 0u) return; // (uniform)
	// 3. the lists
	uint32_t *const ll = list + (size_t)t*c.list_cap;
	uint64_t const below = (1ull << lane) - 1ull;
	for (uint32_t base = 0; base < cnt; base += SCVW_THREADS) {
		uint32_t const i = base + tid;
		uint32_t const streams = (i < cnt) ? scenery_view_streams(recs[i].kind, draw[o0 + i]) : 0u; // (the lane reads the word it wrote)
#pragma unroll
		for (uint32_t s = 0; s < SCV_STREAMS; ++s) {
			uint32_t const m = (uint32_t)__popcll(__ballot((streams >> s) & 1u));
			if (lane == s) {s_w[wave][s] = m;}
		}
		__syncthreads();
#pragma unroll
		for (uint32_t s = 0; s < SCV_STREAMS; ++s) {
			uint64_t const m = __ballot((streams >> s) & 1u);
			if ((streams >> s) & 1u) {
				uint32_t at = s_base[s] + (uint32_t)__popcll(m & below);
				for (uint32_t w = 0; w < wave; ++w) {at += s_w[w][s];}
				if (at < c.list_cap) {ll[at] = i;}
			}
		}
		__syncthreads(); // every start is read
		if (tid < SCV_STREAMS) {
			uint32_t m = 0;
			for (uint32_t w = 0; w < SCVW_WAVES; ++w) {m += s_w[w][tid];}
			s_base[tid] += m;
		}
		__syncthreads(); // before the next chunk's counts
	}
}

// ------------------------------------------------------------------ the deciduous tree draw lists of a tile batch for a camera (tile_t::draw_decid_trees,
// src/tiled_mesh.cpp:1555-1563, tree_cont_t::draw_branches_and_leaves, src/Tree.cpp:312-368; terra_decidview.hpp).  k_decid_view: a workgroup of 256 lanes per
// tile; a skipped tile and one without records leave at once.
//  1. A sweep over the tile's records, a lane a record: the table entry (80 bytes, from L2), the number of valid records and the unions of calc_bcube
//     (decid_view_union_t), reduced over the wave with shuffles and over the four waves through LDS.
//  2. One lane takes the tile-level decisions (decid_view_tile: the cull of :316, the choice of :347-348) and broadcasts them through LDS.
//  3. One sweep in chunks of 256 answers both of the reference's sweeps for a record: the leaves' word, scale, opacity and count, not_visible, then the branches'.
//     tree::not_visible goes from the one to the other in a register, and into the caller's array when there is one: no second array.  leaf_list and branch_list
//     are appended in record order (tp_emit); in a sorted tile the records that reach draw_leaves or add a billboard are compacted as (key, index) pairs instead
//     and placed by their rank (trv_rank, as k_tree_view places the camera tile), which gives the sequence the reference walks; leaf_list is its filtered copy.
//  4. The two billboard lists: a stable counting sort by tree_id over a sequence (record order, or the sorted sequence for the leaves of a sorted tile), so the order
//     inside an id is the sequence's.  tp_sort_by_id (above, shared with k_tree_view) compacts the entries as (id, position) pairs in sequence order (tp_block_rank).  A few hundred pairs, or a table
//     of more than DECID_VIEW_LDS_IDS entries, are placed by rank (trv_rank); more take a histogram in LDS (atomic adds: only counts), an
//     exclusive scan, then emission in sequence order, the waves taking turns and a ballot ranking the lanes that share an id, so no atomic decides an order.
// The pairs lie in LDS for capacities up to DECID_VIEW_LDS_KEYS, else in the tile's part of the driver's scratch.  Steps 3 and 4 read words and opacities that other
// lanes of the workgroup stored: the barriers of tp_block_rank lie between.
constexpr uint32_t DCV_THREADS = 256;
static_assert(DCV_THREADS == TREEP_THREADS, "tp_block_rank and tp_emit rank TREEP_THREADS threads");
__global__ __launch_bounds__(DCV_THREADS) void k_decid_view(decid_view_consts_t c, decid_tree_data_pod_t const *__restrict__ data, uint8_t const *__restrict__ skip,
	decid_place_pod_t const *__restrict__ decid, uint32_t const *__restrict__ counts, uint8_t *not_visible, decid_view_tile_pod_t *__restrict__ tile_out, float *__restrict__ bcube,
	uint32_t *leaf_word, float *__restrict__ leaf_scale, float *leaf_opacity, uint32_t *__restrict__ leaf_num, uint32_t *branch_word, float *__restrict__ branch_scale,
	float *branch_opacity, uint32_t *__restrict__ branch_num, uint32_t *__restrict__ leaf_list, uint32_t *__restrict__ branch_list, decid_view_bb_pod_t *__restrict__ leaf_bb,
	decid_view_bb_pod_t *__restrict__ branch_bb, uint32_t *__restrict__ list_counts, uint32_t *keys)
{
	__shared__ uint32_t s_wave[DCV_THREADS/64], s_nv[DCV_THREADS/64], s_key[DECID_VIEW_LDS_KEYS], s_idx[DECID_VIEW_LDS_KEYS], s_seq[DECID_VIEW_LDS_KEYS], s_hist[DECID_VIEW_LDS_IDS];
	__shared__ decid_view_union_t s_un[DCV_THREADS/64];
	__shared__ decid_view_tile_t s_tile;
	uint32_t const t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t const cnt = (skip && skip[t]) ? 0u : min_u32(counts[t], c.cap); // (uniform)
	auto leave = [&](uint32_t flags, uint32_t num_trees) {
		if (tid == 0) {
			decid_view_tile_pod_t z; z.flags = flags; z.num_trees = num_trees; z.leaf_written = z.branch_written = z.leaf_bb_written = z.branch_bb_written = z.pad[0] = z.pad[1] = 0u;
			tile_out[t] = z;
		}
		if (tid < 4u) {list_counts[4u*t + tid] = 0u;}
	};
	if (cnt == 0u) {if (tid < 6u) {bcube[(size_t)t*6u + tid] = 0.0f;} leave(0u, 0u); return;}
	size_t const o = (size_t)t*c.cap;
	decid_place_pod_t const *const recs = decid + o;
	// 1. the valid records and calc_bcube
	decid_view_union_t un;
	decid_view_union_init(un);
	uint32_t nv = 0;
	for (uint32_t i = tid; i < cnt; i += DCV_THREADS) {
		decid_place_pod_t const r = recs[i];
		if (!decid_view_valid(c, data, r)) continue;
		++nv;
		float b[6], l[6];
		decid_view_bounds(data[r.tree_id], r.pos, b, l);
		decid_view_union_add(un, i, b, l);
	}
	for (int off = 32; off; off >>= 1) {
		decid_view_union_t ot;
#pragma unroll
		for (int k = 0; k < 6; ++k) {ot.b[k] = __shfl_xor(un.b[k], off); ot.l[k] = __shfl_xor(un.l[k], off);}
		ot.first = __shfl_xor(un.first, off); ot.last_zero = __shfl_xor(un.last_zero, off);
		decid_view_union_merge(un, ot);
		nv += __shfl_xor(nv, off);
	}
	if (lane == 0) {s_un[wave] = un; s_nv[wave] = nv;}
	__syncthreads();
	nv = 0;
	for (uint32_t w = 0; w < DCV_THREADS/64; ++w) {nv += s_nv[w];}
	if (nv == 0u) {if (tid < 6u) {bcube[(size_t)t*6u + tid] = 0.0f;} leave(0u, 0u); return;} // decid_trees.empty() (:1557) (uniform)
	// 2. the tile's decisions
	if (tid == 0) {
		decid_view_union_t all = s_un[0];
		for (uint32_t w = 1; w < DCV_THREADS/64; ++w) {decid_view_union_merge(all, s_un[w]);}
		float bc[6];
		decid_view_union_result(all, bc);
#pragma unroll
		for (int k = 0; k < 6; ++k) {bcube[(size_t)t*6u + k] = bc[k];}
		s_tile = decid_view_tile(c, bc);
	}
	__syncthreads();
	decid_view_tile_t const tl = s_tile;
	if (!tl.drawn) {leave(tl.flags, nv); return;} // (uniform)
	bool const big = c.cap > DECID_VIEW_LDS_KEYS;
	uint32_t *const kbuf = big ? keys + o*3u : s_key, *const ibuf = big ? kbuf + c.cap : s_idx, *const sbuf = big ? ibuf + c.cap : s_seq;
	uint32_t *const ll = leaf_list + o, *const bl = branch_list + o;
	// 3. both sweeps of a record
	uint32_t nll = 0, nbl = 0, ms = 0;
	for (uint32_t base = 0; base < cnt; base += DCV_THREADS) {
		uint32_t const i = base + tid;
		bool const valid = i < cnt && decid_view_valid(c, data, recs[i]);
		bool l_listed = false, l_seq = false, b_listed = false;
		float key = 0.0f;
		if (valid) {
			decid_tree_data_pod_t const td = data[recs[i].tree_id];
			decid_view_tree_t const g = decid_view_tree(c, td, recs[i].pos);
			bool nvis = false, wrote = false;
			if (c.leaves) {
				decid_view_rec_t const r = decid_view_leaves(c, td, g, nvis, wrote);
				leaf_word[o + i] = r.word; leaf_scale[o + i] = r.scale; leaf_opacity[o + i] = r.opacity; leaf_num[o + i] = r.num;
				if (wrote && not_visible) {not_visible[o + i] = nvis ? 1 : 0;}
				l_listed = r.listed != 0; l_seq = r.listed != 0 || r.added != 0;
				if (tl.sorted) {key = decid_view_sort_key(c, g);}
			}
			else if (!c.shadow && not_visible) {nvis = not_visible[o + i] != 0;}
			if (c.branches) {
				decid_view_rec_t const r = decid_view_branches(c, td, g, nvis);
				branch_word[o + i] = r.word; branch_scale[o + i] = r.scale; branch_opacity[o + i] = r.opacity; branch_num[o + i] = r.num;
				b_listed = r.listed != 0;
			}
		}
		if (c.leaves) { // (uniform)
			if (!tl.sorted) {tp_emit(l_listed, [&] {return i;}, ll, c.cap, nll, s_wave);}
			else {
				uint32_t tot;
				uint32_t const rank = tp_block_rank(l_seq, s_wave, tot);
				if (l_seq) {kbuf[ms + rank] = __float_as_uint(key); ibuf[ms + rank] = i;}
				ms += tot;
			}
		}
		if (c.branches) {tp_emit(b_listed, [&] {return i;}, bl, c.cap, nbl, s_wave);}
	}
	__syncthreads(); // the words, the opacities and the pairs are complete
	if (tl.sorted) { // the sequence the reference walks, then leaf_list out of it
		for (uint32_t i = tid; i < ms; i += DCV_THREADS) {sbuf[trv_rank<true>(kbuf, ibuf, ms, kbuf[i], ibuf[i])] = ibuf[i];}
		__syncthreads(); // the pairs are reused
		for (uint32_t base = 0; base < ms; base += DCV_THREADS) {
			uint32_t const p = base + tid, idx = (p < ms) ? sbuf[p] : 0u;
			uint32_t const form = (p < ms) ? (leaf_word[o + idx] & (uint32_t)DCV_FORM_MASK) : 0u;
			tp_emit(form == DCV_FORM_GEOM || form == DCV_FORM_BOTH, [&] {return idx;}, ll, c.cap, nll, s_wave);
		}
	}
	// 4. the billboard lists
	uint32_t nlb = 0, nbb = 0;
	if (c.billboards) { // (uniform)
		if (c.leaves) {
			decid_view_bb_pod_t *const out = leaf_bb + o;
			auto rec_of = [&](uint32_t p) {return tl.sorted ? sbuf[p] : p;};
			nlb = tp_sort_by_id<DECID_VIEW_LDS_IDS, DECID_VIEW_RANK_MAX>(c.num_data, tl.sorted ? ms : cnt,
				[&](uint32_t p, uint32_t &id) {
					uint32_t const idx = rec_of(p);
					if (!decid_view_valid(c, data, recs[idx]) || (leaf_word[o + idx] & (uint32_t)DCV_FORM_MASK) < (uint32_t)DCV_FORM_BOTH) return false;
					id = (uint32_t)recs[idx].tree_id;
					return true;
				},
				[&](uint32_t at, uint32_t id, uint32_t p) {
					uint32_t const idx = rec_of(p);
					decid_tree_data_pod_t const td = data[id];
					if (at < c.cap) {out[at] = decid_view_bb<true>(td, decid_view_tree(c, td, recs[idx].pos), id, idx, leaf_opacity[o + idx]);}
				}, s_hist, s_wave, kbuf, ibuf);
		}
		if (c.branches) {
			decid_view_bb_pod_t *const out = branch_bb + o;
			nbb = tp_sort_by_id<DECID_VIEW_LDS_IDS, DECID_VIEW_RANK_MAX>(c.num_data, cnt,
				[&](uint32_t idx, uint32_t &id) {
					if (!decid_view_valid(c, data, recs[idx]) || (branch_word[o + idx] & (uint32_t)DCV_FORM_MASK) < (uint32_t)DCV_FORM_BOTH) return false;
					id = (uint32_t)recs[idx].tree_id;
					return true;
				},
				[&](uint32_t at, uint32_t id, uint32_t idx) {
					decid_tree_data_pod_t const td = data[id];
					if (at < c.cap) {out[at] = decid_view_bb<false>(td, decid_view_tree(c, td, recs[idx].pos), id, idx, branch_opacity[o + idx]);}
				}, s_hist, s_wave, kbuf, ibuf);
		}
	}
	if (tid == 0) {
		decid_view_tile_pod_t z; z.flags = tl.flags; z.num_trees = nv; z.pad[0] = z.pad[1] = 0u;
		z.leaf_written = min_u32(nll, c.cap); z.branch_written = min_u32(nbl, c.cap); z.leaf_bb_written = min_u32(nlb, c.cap); z.branch_bb_written = min_u32(nbb, c.cap);
		tile_out[t] = z;
		list_counts[4u*t] = nll; list_counts[4u*t + 1u] = nbl; list_counts[4u*t + 2u] = nlb; list_counts[4u*t + 3u] = nbb;
	}
}

// ------------------------------------------------------------------ sphere collisions and tree box tests against the containers of a tile batch
// (tile_t::check_sphere_collision, src/tiled_mesh.cpp:2146-2168; tile_t::check_cube_int_trees, :2170-2173; terra_collide.hpp).
// k_sphere_collide: one 64-lane wave per query, four queries per workgroup; no LDS, no barrier, nothing waits for another wave.  Every lane holds the query and the
// centre; what decides where the wave goes (the stage, the counts, the gates, the ballots) is the same in all 64 lanes.  Per container, in the reference's order:
//  - the prologue: a sweep over the tile's records, a lane a record, for the number of valid records (the container's empty()) and calc_bcube, reduced with shuffles;
//    for the scenery, which kinds the tile holds and whether a rock_shape has no override.
//  - the chain: the wave tests the next 64 records against the current centre, a lane a record, with the exact test.  The lowest lane of the ballot is the first hit
//    in the reference's order -- every record before it has seen the centre it would have seen sequentially -- so its pushed centre is broadcast and the wave resumes
//    at the record behind it.  Without a hit the wave steps 64 records on.  The resume position advances strictly: a container of c records ends after at most c rounds.
//    The scenery is walked once per kind that the tile holds, in scenery_group::check_sphere_coll's order; a lane whose record is of another kind does not hit.
// k_cube_int_trees: the same wave per query; the test is an order-free "any" over the valid deciduous records, so one ballot per 64 records answers it.
constexpr uint32_t COLL_THREADS = 256;
__device__ __forceinline__ void coll_wave_take(coll_pt_t &c, coll_pt_t const &m, int l) {c.x = __shfl(m.x, l); c.y = __shfl(m.y, l); c.z = __shfl(m.z, l);}
// the chain over records [0, cnt): test(j, m) -> whether record j moves the centre m
template<class TEST> __device__ __forceinline__ uint32_t coll_wave_chain(uint32_t cnt, uint32_t lane, coll_pt_t &c, TEST test) {
	uint32_t nhits = 0;
	for (uint32_t start = 0; start < cnt;) {
		uint32_t const j = start + lane;
		coll_pt_t m = c;
		bool const hit = j < cnt && test(j, m);
		unsigned long long const mask = __ballot(hit);
		if (mask == 0ull) {start += 64u; continue;}
		int const l = __ffsll((long long)mask) - 1;
		coll_wave_take(c, m, l);
		++nhits; start += (uint32_t)l + 1u;
	}
	return nhits;
}
// calc_bcube of the deciduous container by the wave; -> the number of valid records
__device__ __forceinline__ uint32_t coll_wave_decid_bcube(collide_consts_t const &c, collide_in_t const &in, uint32_t t, uint32_t nd, uint32_t lane, float bc[6]) {
	decid_view_union_t un;
	decid_view_union_init(un);
	uint32_t nv = 0;
	for (uint32_t j = lane; j < nd; j += 64u) {
		decid_place_pod_t r;
		if (!coll_decid_rec(c, in, t, j, r)) continue;
		++nv;
		float b[6], l[6];
		decid_view_bounds(in.data[r.tree_id], r.pos, b, l);
		decid_view_union_add(un, j, b, l);
	}
	for (int off = 32; off; off >>= 1) {
		decid_view_union_t ot;
#pragma unroll
		for (int k = 0; k < 6; ++k) {ot.b[k] = __shfl_xor(un.b[k], off); ot.l[k] = __shfl_xor(un.l[k], off);}
		ot.first = __shfl_xor(un.first, off); ot.last_zero = __shfl_xor(un.last_zero, off);
		decid_view_union_merge(un, ot);
		nv += __shfl_xor(nv, off);
	}
	decid_view_union_result(un, bc);
	return nv;
}
__device__ __forceinline__ coll_result_t coll_query_wave(collide_consts_t const &c, collide_in_t const &in, uint32_t t, float const pos[3], float radius, uint32_t flags, uint32_t lane) {
	coll_result_t o; o.c.x = pos[0]; o.c.y = pos[1]; o.c.z = pos[2]; o.word = 0u; o.nhits = 0u;
	float const INF = __builtin_inff();
	uint32_t const np = (flags & COLL_INC_PTREES) ? coll_pine_count(c, in, t) : 0u;
	if (np != 0u) {
		float box[6] = {INF, -INF, INF, -INF, INF, -INF}; // (coll_pine_bcube assigns the first box and then unions: the same bounds but for the sign of a zero, which no comparison of the gate sees)
		uint32_t nv = 0, nb = 0;
		for (uint32_t j = lane; j < np; j += 64u) {
			tree_view_rec_t rec;
			if (!coll_pine_rec(c, in, t, j, rec)) continue;
			++nv;
			float d[6];
			if (!tree_view_bounds(rec, d)) continue;
			++nb;
			box_union(box, d);
		}
		for (int off = 32; off; off >>= 1) {
			nv += __shfl_xor(nv, off); nb += __shfl_xor(nb, off);
#pragma unroll
			for (int k = 0; k < 6; k += 2) {box[k] = min_std(box[k], __shfl_xor(box[k], off)); box[k + 1] = max_std(box[k + 1], __shfl_xor(box[k + 1], off));}
		}
		if (nv != 0u) { // inc_ptrees && !pine_trees.empty()
			if (nb == 0u) {
#pragma unroll
				for (int k = 0; k < 6; ++k) {box[k] = 0.0f;}
			}
			o.c.x -= c.pv.a.offx; o.c.y -= c.pv.a.offy; o.c.z -= 0.0f;
			if (!coll_gate_exits(o.c, radius, box)) {
				uint32_t const nh = coll_wave_chain(np, lane, o.c, [&](uint32_t j, coll_pt_t &m) {
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
		float bc[6];
		if (coll_wave_decid_bcube(c, in, t, nd, lane, bc) != 0u) {
			o.c.x -= c.doffx; o.c.y -= c.doffy; o.c.z -= 0.0f;
			if (!coll_gate_exits(o.c, radius, bc)) {
				uint32_t const nh = coll_wave_chain(nd, lane, o.c, [&](uint32_t j, coll_pt_t &m) {
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
		uint32_t present = 0; // bit k: the tile holds a record of kind k; bit 31: a rock_shape without an override
		for (uint32_t j = lane; j < ns; j += 64u) {
			int const kind = in.scen[base + j].kind;
			if (kind >= 0 && kind < SCENERY_KINDS) {present |= 1u << kind;}
			if (kind == SCENERY_ROCK_SHAPE && !((in.rov ? in.rov[base + j] : 0.0f) > 0.0f)) {present |= 0x80000000u;}
		}
		for (int off = 32; off; off >>= 1) {present |= __shfl_xor(present, off);}
		if (present & 0x80000000u) {o.word |= COLL_ROCK_SHAPE_UNDECIDED;}
		o.c.x -= c.soffx; o.c.y -= c.soffy; o.c.z -= 0.0f;
		for (int k = 0; k < COLL_SCENERY_PASSES; ++k) {
			int const kind = coll_scenery_pass_kind(k);
			if (!((present >> kind) & 1u)) continue;
			uint32_t const nh = coll_wave_chain(ns, lane, o.c, [&](uint32_t j, coll_pt_t &m) {
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
__global__ __launch_bounds__(COLL_THREADS) void k_sphere_collide(collide_consts_t c, collide_in_t in, sphere_query_pod_t const *__restrict__ queries, uint32_t nq,
	sphere_hit_pod_t *__restrict__ hits)
{
	uint32_t const lane = threadIdx.x & 63u;
	uint32_t const qi = blockIdx.x*(COLL_THREADS/64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (qi >= nq) return; // (the whole wave)
	sphere_query_pod_t const q = queries[qi];
	sphere_hit_pod_t const h = coll_query(c, in, q, [&](uint32_t t) {return coll_query_wave(c, in, t, q.pos, q.radius, q.flags, lane);});
	if (lane == 0u) {hits[qi] = h;}
}
__global__ __launch_bounds__(COLL_THREADS) void k_cube_int_trees(collide_consts_t c, collide_in_t in, float const *__restrict__ cubes, int32_t const *__restrict__ cube_tile, uint32_t nq,
	uint8_t *__restrict__ result, int32_t *__restrict__ tile_out)
{
	uint32_t const lane = threadIdx.x & 63u;
	uint32_t const qi = blockIdx.x*(COLL_THREADS/64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (qi >= nq) return; // (the whole wave)
	float d[6];
#pragma unroll
	for (int k = 0; k < 6; ++k) {d[k] = cubes[(size_t)qi*6u + k];}
	uint32_t res = 0;
	int32_t t = -1;
	if (!coll_cube_ok(d)) {res = CUBE_INT_BAD_QUERY;}
	else {
		t = coll_cube_tile(c, in, cube_tile ? cube_tile[qi] : -1, d);
		if (t < 0) {res = CUBE_INT_NO_TILE;}
		else {
			uint32_t const nd = coll_decid_count(c, in, (uint32_t)t);
			float bc[6], loc[6];
			if (nd != 0u && coll_wave_decid_bcube(c, in, (uint32_t)t, nd, lane, bc) != 0u) {
				coll_cube_local(c, d, loc);
				if (coll_zero_area(bc) || coll_cubes_intersect(bc, loc)) {
					for (uint32_t start = 0; start < nd && !res; start += 64u) {
						uint32_t const j = start + lane;
						decid_place_pod_t r;
						bool const hit = j < nd && coll_decid_rec(c, in, (uint32_t)t, j, r) && coll_decid_cube(in.data[r.tree_id], r.pos, loc);
						if (__ballot(hit) != 0ull) {res = CUBE_INT_HIT;}
					}
				}
			}
		}
	}
	if (lane == 0u) {result[qi] = (uint8_t)res; if (tile_out) {tile_out[qi] = t;}}
}

// ------------------------------------------------------------------ tree AO shadows from the placement records (tile_t::apply_tree_ao_shadows, src/tiled_mesh.cpp:740-828;
// terra_treeao.hpp), three launches: k_tree_ao_sources, k_tree_ao_gather, then k_tree_map (above, unchanged) on the lists the gather wrote.
// k_tree_ao_sources: a thread per record slot, a block = 256 slots of one tile (so a wave never spans two tiles).  {pt.x, pt.y, get_ao_radius()} of every record goes
// into the tile's part of the source array, pine first; get_radius() is reduced over the wave and one lane raises trmax[t] with an atomic max on the float's bits
// (the values are non-negative, so unsigned order is float order; the driver zeroes trmax first).  It also clears `updated`.
__global__ __launch_bounds__(256) void k_tree_ao_sources(tree_ao_consts_t c, tree_inst_pod_t const *__restrict__ insts, tree_place_pod_t const *__restrict__ pine,
	uint32_t const *__restrict__ pine_counts, decid_place_pod_t const *__restrict__ decid, uint32_t const *__restrict__ decid_counts, float const *__restrict__ decid_radius,
	float const *__restrict__ decid_radius_by_id, tree_splat_in_t *__restrict__ src, float *__restrict__ trmax, uint8_t *__restrict__ updated)
{
	uint32_t const t = blockIdx.x, j = blockIdx.y*256u + threadIdx.x;
	if (j == 0) {updated[t] = 0;}
	float radius = 0.0f;
	if (j < c.pine_cap) {
		if (pine_counts && j < min_u32(pine_counts[t], c.pine_cap)) {src[(size_t)t*c.src_cap + j] = tree_ao_source_pine(c, insts, pine[(size_t)t*c.pine_cap + j], radius);}
	}
	else if (j < c.src_cap) {
		uint32_t const k = j - c.pine_cap;
		if (decid_counts && k < min_u32(decid_counts[t], c.decid_cap)) {
			size_t const i = (size_t)t*c.decid_cap + k;
			src[(size_t)t*c.src_cap + j] = tree_ao_source_decid(c, decid[i], decid_radius ? decid_radius + i : nullptr, decid_radius_by_id, radius);
		}
	}
	for (int m = 32; m > 0; m >>= 1) {radius = fmaxf(radius, __shfl_xor(radius, m));}
	if ((threadIdx.x & 63u) == 0 && radius > 0.0f) {atomicMax((unsigned int *)(trmax + t), __float_as_uint(radius));}
}
// k_tree_ao_gather: a workgroup per destination tile t.  It walks t's segments in list order -- own, the pulls in dy, dx order, the pushes in batch order -- 256
// source entries at a time; every thread runs the filter of its entry (the box cull of :793, or the integer test of :769-775 in the source tile's frame) and the
// survivors are appended in order through a ballot per wave and a prefix over the four waves, already parameterised against t's frame for k_tree_map.  The tile's
// pod (first = t*list_cap, count) is written here: nothing of the lists ever exists on the host.
__global__ __launch_bounds__(TREEP_THREADS) void k_tree_ao_gather(tree_ao_consts_t c, tree_frame_t const *__restrict__ frames, int32_t const *__restrict__ nbr,
	uint8_t const *__restrict__ flags, float const *__restrict__ trmax, uint32_t const *__restrict__ pine_counts, uint32_t const *__restrict__ decid_counts,
	tree_splat_in_t const *__restrict__ src, tree_tile_pod_t *__restrict__ tiles, tree_splat_pod_t *__restrict__ par, uint32_t *__restrict__ list_counts)
{
	__shared__ uint32_t s_wave[TREEP_THREADS/64];
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	tree_frame_t const ft = frames[t];
	int32_t nb[9];
	for (int k = 0; k < 9; ++k) {nb[k] = nbr[(size_t)t*9 + k];}
	tree_splat_pod_t *const out = par + (size_t)t*c.list_cap;
	uint32_t count = 0, last = t; // (the same in every thread)
	for (int k = 0; k < 17; ++k) {
		int mode = TREE_AO_OWN, slot = 4;
		uint32_t u = t;
		if (k >= 1 && k <= 8) { // pull: the neighbours in dy, dx order that come earlier in the batch
			slot = (k <= 4) ? k - 1 : k;
			if (nb[slot] < 0 || (uint32_t)nb[slot] >= t) continue;
			mode = TREE_AO_PULL; u = (uint32_t)nb[slot];
		}
		else if (k >= 9) { // push: the neighbours that come later, in batch order
			if (!tree_ao_next_push(nb, last, slot)) break;
			mode = TREE_AO_PUSH; u = last;
		}
		tree_ao_seg_t sg;
		if (!tree_ao_segment(c, t, mode, u, slot, flags, trmax, pine_counts, decid_counts, sg)) continue;
		tree_frame_t const fu = frames[u];
		uint32_t const total = sg.np + sg.nd;
		for (uint32_t base = 0; base < total; base += TREEP_THREADS) {
			uint32_t const j = base + tid;
			bool keep = false;
			tree_splat_in_t s = {0.0f, 0.0f, -1.0f};
			if (j < total) {
				s = src[tree_ao_entry(c, sg, j)];
				keep = tree_ao_keep(c, sg, s, ft.x, ft.y, fu.x, fu.y);
			}
			tp_emit(keep, [&] {return tree_splat_params(s, ft.x, ft.y, c.dxv, c.dyv);}, out, c.list_cap, count, s_wave);
		}
	}
	if (tid == 0) {
		tree_tile_pod_t tt;
		tt.xstart = ft.x; tt.ystart = ft.y; tt.first = t*c.list_cap; tt.count = min_u32(count, c.list_cap);
		tiles[t] = tt;
		if (list_counts) {list_counts[t] = count;}
	}
}

// ------------------------------------------------------------------ the tree brush on the record arrays of a batch (tile_draw_t::add_or_remove_trees_at,
// src/tiled_mesh.cpp:3746-3843; terra_treeedit.hpp), three launches: k_tree_edit, k_tree_edit_append (only when adding, after the two brush placements), k_tree_edit_finish.
// The removal of one group of k_tree_edit: tp_block_remove's three sweeps written out, the first one also taking the removed records' box.  Kept apart because
// k_tree_edit on tp_block_remove measured slower on a whole-batch stroke (106.4 and 108.5 us against the parent's 102.7-105.5 and 96.6-103.0 in two alternating runs;
// same instructions in another schedule): this is the form those figures of the parent belong to.
template<class REC, class BOX> __device__ __forceinline__ uint32_t te_remove_group(tree_edit_consts_t const &c, REC *v, float *radius, uint32_t cnt, uint32_t *idx, uint32_t *s_wave, BOX box_of) {
	uint32_t const tid = threadIdx.x;
	uint32_t m = 0, nk;
	for (uint32_t base = 0; base < cnt; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool keep = false;
		if (i < cnt) {
			keep = !tree_edit_removed(c, v[i].pos[0], v[i].pos[1]);
			if (!keep) {box_of(v[i], radius ? radius + i : nullptr);}
		}
		tp_block_rank(keep, s_wave, nk);
		m += nk;
	}
	if (m == cnt) return m;
	uint32_t h = 0;
	for (uint32_t base = m; base < cnt; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool const keep = i < cnt && !tree_edit_removed(c, v[i].pos[0], v[i].pos[1]);
		uint32_t const rank = tp_block_rank(keep, s_wave, nk);
		if (keep) {idx[h + rank] = i;}
		h += nk;
	}
	__syncthreads(); // idx[] is complete
	uint32_t k0 = 0;
	for (uint32_t base = 0; base < m; base += TREEP_THREADS) {
		uint32_t const i = base + tid;
		bool const hole = i < m && tree_edit_removed(c, v[i].pos[0], v[i].pos[1]);
		uint32_t const rank = tp_block_rank(hole, s_wave, nk);
		if (hole) {
			uint32_t const src = idx[h - 1u - (k0 + rank)];
			v[i] = v[src];
			if (radius) {radius[i] = radius[src];}
		}
		k0 += nk;
	}
	return m;
}
// the threads' boxes -> one per wave (xor butterfly), then the six atomics of tree_box_commit from lane 0
__device__ __forceinline__ void te_box_commit_wave(tree_box_t b, uint32_t *box) {
	for (int m = 32; m > 0; m >>= 1) {
		for (int i = 0; i < 3; ++i) {b.lo[i] = min_std(b.lo[i], __shfl_xor(b.lo[i], m)); b.hi[i] = max_std(b.hi[i], __shfl_xor(b.hi[i], m));}
	}
	if ((threadIdx.x & 63u) == 0) {tree_box_commit(b, box);}
}
// k_tree_edit: a workgroup per tile.  The two culls are one wave-uniform test on the tile's frame, stats and trmax: a brush touches a handful of the tiles of a batch and
// every other workgroup ends there.  A tile that is hit runs the removal of both groups and leaves M in its counts and its state in `status`.
__global__ __launch_bounds__(TREEP_THREADS) void k_tree_edit(tree_edit_consts_t c, tree_edit_frame_t const *__restrict__ frames, terra_tile_stats const *__restrict__ stats,
	tree_inst_pod_t const *__restrict__ insts, tree_place_pod_t *pine, uint32_t *pine_counts, decid_place_pod_t *decid, uint32_t *decid_counts, float *decid_radius,
	float const *__restrict__ by_id, float const *__restrict__ trmax, uint32_t *idx, uint32_t *box, uint8_t *status, uint8_t const *__restrict__ skip, uint8_t const *__restrict__ gen_flags, uint8_t *__restrict__ place_skip)
{
	__shared__ uint32_t s_wave[TREEP_THREADS/64];
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	uint32_t state = tree_edit_cull(c, frames[t], stats[t].mzmin, stats[t].mzmax, stats[t].radius, trmax[t]);
	if (tid == 0 && place_skip) { // (adding: the brush placements leave at once every tile that is not hit and every group that is gated)
		uint32_t const sk = skip ? skip[t] : 0u, gf = gen_flags ? gen_flags[t] : 0u;
		place_skip[t] = tree_edit_place_skip(state, sk, gf & TREE_EDIT_NO_PINE_GEN); place_skip[gridDim.x + t] = tree_edit_place_skip(state, sk, gf & TREE_EDIT_NO_DECID_GEN);
	}
	if (!(state & TREE_EDIT_HIT)) {if (tid == 0) {status[t] = (uint8_t)state;} return;}
	tree_box_t b;
	tree_box_clear(b);
	uint32_t const idx_cap = (c.a.pine_cap < c.a.decid_cap) ? c.a.decid_cap : c.a.pine_cap;
	uint32_t *const my_idx = idx + (size_t)t*idx_cap;
	if (pine_counts) {
		uint32_t const cnt = min_u32(pine_counts[t], c.a.pine_cap);
		uint32_t const m = te_remove_group(c, pine + (size_t)t*c.a.pine_cap, (float *)nullptr, cnt, my_idx, s_wave,
			[&](tree_place_pod_t const &r, float const *) {tree_edit_box_pine(c, insts, r, b);});
		if (m != cnt) {state |= TREE_EDIT_CHANGED;}
		__syncthreads(); // every thread has read the count
		if (tid == 0) {pine_counts[t] = m;}
	}
	if (decid_counts) {
		uint32_t const cnt = min_u32(decid_counts[t], c.a.decid_cap);
		uint32_t const m = te_remove_group(c, decid + (size_t)t*c.a.decid_cap, decid_radius ? decid_radius + (size_t)t*c.a.decid_cap : nullptr, cnt, my_idx, s_wave,
			[&](decid_place_pod_t const &r, float const *rad) {tree_edit_box_decid(c, r, rad, by_id, b);});
		if (m != cnt) {state |= TREE_EDIT_CHANGED;}
		__syncthreads();
		if (tid == 0) {decid_counts[t] = m;}
	}
	te_box_commit_wave(b, box);
	if (tid == 0) {status[t] = (uint8_t)state;}
}
// k_tree_edit_append: a workgroup per tile; only the tiles k_tree_edit found hit do anything.  The records the brush placements left in the arena go behind the M
// survivors as far as the array has room, counts[t] = M + all of them; the stored records raise trmax[t] (an atomic max on the bits of a positive float) and widen the box.
__global__ __launch_bounds__(TREEP_THREADS) void k_tree_edit_append(tree_edit_consts_t c, uint8_t const *__restrict__ gen_flags, tree_inst_pod_t const *__restrict__ insts,
	tree_place_pod_t const *__restrict__ new_pine, uint32_t const *__restrict__ new_pine_counts, tree_place_pod_t *pine, uint32_t *pine_counts,
	decid_place_pod_t const *__restrict__ new_decid, uint32_t const *__restrict__ new_decid_counts, decid_place_pod_t *decid, uint32_t *decid_counts, float *decid_radius,
	float const *__restrict__ by_id, float *trmax, uint32_t *box, uint8_t *status)
{
	uint32_t const t = blockIdx.x, tid = threadIdx.x;
	uint32_t state = status[t];
	if (!(state & TREE_EDIT_HIT)) return;
	uint32_t const gf = gen_flags ? gen_flags[t] : 0u;
	bool const do_pine = new_pine && !(gf & TREE_EDIT_NO_PINE_GEN), do_decid = new_decid && !(gf & TREE_EDIT_NO_DECID_GEN);
	uint32_t const mp = do_pine ? pine_counts[t] : 0u, np = do_pine ? new_pine_counts[t] : 0u, md = do_decid ? decid_counts[t] : 0u, nd = do_decid ? new_decid_counts[t] : 0u;
	__syncthreads(); // every thread has read the state and the counts
	tree_box_t b;
	tree_box_clear(b);
	float rmax = 0.0f;
	uint32_t const sp = min_u32(np, c.a.pine_cap - min_u32(mp, c.a.pine_cap)), sd = min_u32(nd, c.a.decid_cap - min_u32(md, c.a.decid_cap)); // how many are stored
	for (uint32_t j = tid; j < sp; j += TREEP_THREADS) {
		tree_place_pod_t const r = new_pine[(size_t)t*c.a.pine_cap + j];
		pine[(size_t)t*c.a.pine_cap + mp + j] = r;
		rmax = max_std(rmax, tree_edit_box_pine(c, insts, r, b));
	}
	for (uint32_t j = tid; j < sd; j += TREEP_THREADS) {
		decid_place_pod_t const r = new_decid[(size_t)t*c.a.decid_cap + j];
		float const rad = tree_edit_new_decid_radius(c, r, by_id);
		decid[(size_t)t*c.a.decid_cap + md + j] = r;
		if (decid_radius) {decid_radius[(size_t)t*c.a.decid_cap + md + j] = rad;}
		rmax = max_std(rmax, tree_edit_box_decid(c, r, &rad, nullptr, b));
	}
	te_box_commit_wave(b, box);
	for (int m = 32; m > 0; m >>= 1) {rmax = max_std(rmax, __shfl_xor(rmax, m));}
	if ((tid & 63u) == 0 && rmax > 0.0f) {atomicMax((unsigned int *)(trmax + t), __float_as_uint(rmax));}
	if (tid == 0) {
		if (do_pine) {pine_counts[t] = mp + np;}
		if (do_decid) {decid_counts[t] = md + nd;}
		if (np | nd) {status[t] = (uint8_t)(state | TREE_EDIT_CHANGED);}
	}
}
// k_tree_edit_finish: a thread per tile, after the box is complete: the state byte becomes the status, changed follows from it and from the box
__global__ __launch_bounds__(256) void k_tree_edit_finish(tree_edit_consts_t c, uint32_t n, tree_edit_frame_t const *__restrict__ frames, terra_tile_stats const *__restrict__ stats,
	uint32_t const *__restrict__ box, uint8_t *status, uint8_t *__restrict__ changed, float *__restrict__ update_bcube)
{
	uint32_t const t = blockIdx.x*256u + threadIdx.x;
	if (t >= n) return;
	uint8_t st, ch;
	tree_edit_finish(c, frames[t], stats[t].mzmin, stats[t].mzmax, status[t], box, st, ch, (t == 0) ? update_bcube : nullptr);
	status[t] = st; changed[t] = ch;
}

// ------------------------------------------------------------------ K10: 16-bit quantise (heightmap_t::from_floats + write_pixel_16_bits, src/heightmap.cpp:205-215, src/Textures.cpp:1889-1893)
// HBM-bound, 4 B read + 2 B written per cell: eight cells per thread = two 16-byte loads and one 16-byte store of {fraction, integer} byte pairs
__device__ __forceinline__ uint32_t q16_pair(float z, float val_add, float val_div) {
	float const v = (z - val_add)*val_div;
	uint8_t const hi = (uint8_t)v;
	uint8_t const lo = (uint8_t)(256.0f*(v - (float)hi));
	return (uint32_t)lo | ((uint32_t)hi << 8);
}
__global__ __launch_bounds__(256) void k_quantize16(float const *__restrict__ vals, size_t n8, float val_add, float val_div, st_u4 *__restrict__ pix) {
	size_t const i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n8) return;
	st_f4 const a = __builtin_nontemporal_load((st_f4 const *)vals + 2*i), b = __builtin_nontemporal_load((st_f4 const *)vals + 2*i + 1);
	st_u4 o;
	o.x = q16_pair(a.x, val_add, val_div) | (q16_pair(a.y, val_add, val_div) << 16);
	o.y = q16_pair(a.z, val_add, val_div) | (q16_pair(a.w, val_add, val_div) << 16);
	o.z = q16_pair(b.x, val_add, val_div) | (q16_pair(b.y, val_add, val_div) << 16);
	o.w = q16_pair(b.z, val_add, val_div) | (q16_pair(b.w, val_add, val_div) << 16);
	__builtin_nontemporal_store(o, &pix[i]);
}

// ------------------------------------------------------------------ K8: voxel sine field (noise_gen_3d::get_val, src/upsurface.cpp:60-70)
// val[y][x][z] = sum_k (xv[x][k]*yv[y][k])*zv[z][k], z fastest.  fp32-VALU bound (60 mul + 60 add per voxel for 4 B written).
// One lane = one z: its 60 zv values stay in registers (30 register pairs); the block walks VX_PER_BLOCK (x,y) columns TWO AT A TIME: the products
// P[k] = xv*yv of a column pair are stored interleaved, so one scalar load delivers {P_a[k], P_b[k]} as an SGPR pair and one v_pk_mul_f32 / v_pk_add_f32
// (zv broadcast from either half of its pair by op_sel) advances both columns -- same multiplies and adds, half the instructions.
// (Measured with tools/pk_rate.hip: gfx950 issues a plain fp32 VALU op in ~1.0 ns per SIMD and a packed one in ~1.8 ns, so packing buys ~10%, not 2x.)
// Output rows are contiguous along z: coalesced stores.
constexpr int VX_PER_BLOCK = 32;
constexpr int VX_PSTRIDE = 128; // floats per column pair in P: 60 interleaved pairs, padded to whole 16-float scalar loads
typedef float vx_v16f __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void k_voxel_P(float *__restrict__ P, float *__restrict__ ZT, uint32_t nx, uint32_t ny, uint32_t nz, float const *__restrict__ tab) {
	// P[(col/2)*128 + k*2 + (col & 1)], columns padded to an even count with zeros; ZT[k][z] = the z table transposed, so that lane z of the main kernel reads it coalesced
	// a thread makes BOTH products of a column pair for one k and writes them as one 8-byte word: consecutive threads write consecutive words (one product per thread wrote
	// every other float of a line: 34 us for the 63 MB of a 512 x 512 field, half of what the 512 x 512 x 64 field's own kernel takes)
	size_t i = (size_t)blockIdx.x*256 + threadIdx.x; size_t const ncol = (size_t)nx*ny, ncol2 = (ncol + 1) & ~(size_t)1;
	if (i < (ncol2/2)*VOX_SINES) {
		uint32_t const k = (uint32_t)(i % VOX_SINES); size_t const pr = i / VOX_SINES;
		sg_v2f v = {0.0f, 0.0f};
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			size_t const c = 2*pr + (size_t)h;
			if (c < ncol) {uint32_t const x = (uint32_t)(c % nx), y = (uint32_t)(c / nx); v[h] = __fmul_rn(tab[(size_t)x*VOX_SINES + k], tab[((size_t)nx + y)*VOX_SINES + k]);}
		}
		*(sg_v2f *)&P[pr*VX_PSTRIDE + k*2] = v;
		return;
	}
	if (i < ncol2*VOX_SINES) return; // (the launch is sized for one thread per product: the upper half of those threads has nothing to do)
	i -= ncol2*VOX_SINES;
	if (i >= (size_t)nz*VOX_SINES) return;
	uint32_t const z = (uint32_t)(i % nz), k = (uint32_t)(i / nz);
	ZT[i] = tab[((size_t)nx + ny + z)*VOX_SINES + k];
}
template<int E> __device__ __forceinline__ void vx_mul_add(sg_v2f &val, sg_v2f p2, sg_v2f zpair) { // val += {P_a*z, P_b*z}: product rounded, then added
	sg_v2f t;
	if (E == 0) {asm("v_pk_mul_f32 %1, %2, %3 op_sel:[0,0] op_sel_hi:[1,0]\n\tv_pk_add_f32 %0, %0, %1" : "+v"(val), "=&v"(t) : "s"(p2), "v"(zpair));}
	else        {asm("v_pk_mul_f32 %1, %2, %3 op_sel:[0,1] op_sel_hi:[1,1]\n\tv_pk_add_f32 %0, %0, %1" : "+v"(val), "=&v"(t) : "s"(p2), "v"(zpair));}
}
__global__ __launch_bounds__(256) void k_voxel_sines(float *__restrict__ out, uint32_t nx, uint32_t ny, uint32_t nz, float const *__restrict__ ZT, float const *__restrict__ P, float zscale, int normalize) {
	uint32_t const z = blockIdx.y*blockDim.x + threadIdx.x;
	bool const active = z < nz;
	sg_v2f zv[VOX_SINES/2];
	float const *zcol = ZT + (active ? z : 0);
#pragma unroll
	for (unsigned k = 0; k < VOX_SINES/2; ++k) {zv[k] = sg_v2f{zcol[(size_t)(2*k)*nz], zcol[(size_t)(2*k + 1)*nz]};}
	float const zterm = __fmul_rn((float)z, zscale);
	size_t const c0 = (size_t)blockIdx.x*VX_PER_BLOCK, ncol = (size_t)nx*ny;
	if (c0 >= ncol) return;
	// The P stream is software-pipelined by hand.  Scalar loads return out of order, so the only usable wait is lgkmcnt(0) -- left to the compiler, every second 64-byte load was
	// issued directly in front of such a wait (its whole latency exposed: SQ_WAIT_ANY 0.65 of the wave cycles).  Here a stage is TWO 64-byte loads (16 k of a column pair), in
	// flight while the 32 packed instructions of the previous stage run: wait, issue the next stage into the other buffers, compute.  The buffers are asm operands from issue
	// to use, nothing else touches them.  P itself streams from HBM (63 MB at 512^3, no reuse): each wave first touches its share of the block's 8 KB slice with ONE vector load
	// (a lane per 64-byte line), so that the scalar loads find the lines in the L2 instead of paying the HBM latency chunk by chunk.
	size_t const last_pair = (ncol - 1) >> 1;
	float const *pp = P + (c0 >> 1)*VX_PSTRIDE; // chunk 0 of this block's first column pair
	float touched, touched2;
	{
		// 128 lines of 64 B = 16 column pairs x 512 B.  A block of four waves (nz >= 256) touches 32 lines per wave; a block of ONE wave (the reference's own 64-deep field)
		// must touch them all itself -- with lines 32 .. 127 left to the scalar loads the 512 x 512 x 64 field took 83 us instead of ~45
		// (two loads per lane at most; both destination registers stay allocated until the waits at the end of the kernel: the loads are asynchronous to the compiler)
		unsigned const nw = blockDim.x >> 6, per_wave = 128u/nw, base = (threadIdx.x >> 6)*per_wave, l0 = threadIdx.x & 63u;
		unsigned const la = base + ((l0 < per_wave) ? l0 : 0u), lb = base + ((l0 + 64u < per_wave) ? l0 + 64u : ((l0 < per_wave) ? l0 : 0u));
		size_t const pa = (c0 >> 1) + (la >> 3), pb = (c0 >> 1) + (lb >> 3);
		float const *ta = P + ((pa <= last_pair) ? pa : last_pair)*VX_PSTRIDE + (la & 7u)*16u, *tb = P + ((pb <= last_pair) ? pb : last_pair)*VX_PSTRIDE + (lb & 7u)*16u;
		asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off" : "=&v"(touched), "=&v"(touched2) : "v"(ta), "v"(tb));
	}
	vx_v16f b0, b1, b2, b3;
	asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40" : "=&s"(b0), "=&s"(b1) : "s"(pp));
#define VX_NEXT(CA, CB, NA, NB, ADDR) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %2, %4, 0x0\n\ts_load_dwordx16 %3, %4, 0x40" : "+s"(CA), "+s"(CB), "=&s"(NA), "=&s"(NB) : "s"(ADDR))
#define VX_STEP(BUF, Q, J, LO, HI) if (Q*8 + J < VOX_SINES) {vx_mul_add<(J & 1)>(val, sg_v2f{BUF.LO, BUF.HI}, zv[(Q*8 + J < VOX_SINES) ? ((Q*8 + J) >> 1) : 0]);}
#define VX_CHUNK(BUF, Q) VX_STEP(BUF, Q, 0, s0, s1) VX_STEP(BUF, Q, 1, s2, s3) VX_STEP(BUF, Q, 2, s4, s5) VX_STEP(BUF, Q, 3, s6, s7) VX_STEP(BUF, Q, 4, s8, s9) VX_STEP(BUF, Q, 5, sa, sb) VX_STEP(BUF, Q, 6, sc, sd) VX_STEP(BUF, Q, 7, se, sf)
	for (int c = 0; c < VX_PER_BLOCK; c += 2) {
		size_t const col = c0 + c; // = x + y*nx of the pair's first column (even), wave-uniform
		if (col >= ncol) break;
		size_t const np = ((col >> 1) + 1 <= last_pair) ? (col >> 1) + 1 : last_pair; // the pair whose first stage is fetched under this pair's last one (past the end: any valid address)
		float const *pn = P + np*VX_PSTRIDE;
		sg_v2f val = {0.0f, 0.0f}; // (xv*yv)*zv, summed in k order; 8 pairs per 64-byte scalar load
		VX_NEXT(b0, b1, b2, b3, pp + 32); VX_CHUNK(b0, 0) VX_CHUNK(b1, 1)
		VX_NEXT(b2, b3, b0, b1, pp + 64); VX_CHUNK(b2, 2) VX_CHUNK(b3, 3)
		VX_NEXT(b0, b1, b2, b3, pp + 96); VX_CHUNK(b0, 4) VX_CHUNK(b1, 5)
		VX_NEXT(b2, b3, b0, b1, pn);      VX_CHUNK(b2, 6) VX_CHUNK(b3, 7)
		pp = pn;
		float va = __fadd_rn(val.x, zterm), vb = __fadd_rn(val.y, zterm);
		if (normalize) {va = clip_pm1(va); vb = clip_pm1(vb);}
		if (active) {
			__builtin_nontemporal_store(va, &out[col*nz + z]); // written once, never read back by this kernel: keep it out of the L2's way
			if (col + 1 < ncol) {__builtin_nontemporal_store(vb, &out[(col + 1)*nz + z]);}
		}
	}
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(touched), "+v"(touched2)); // the last prefetch and the touch loads land before the wave ends
#undef VX_CHUNK
#undef VX_STEP
#undef VX_NEXT
}

// ---- the same field with a LANE PER COLUMN (round 6).  k_voxel_sines streams a 63 MB array of products P = xv*yv (for a 512 x 512 field) through the scalar unit: as much
// traffic as a 64-deep field's own output, a launch to make it, and per wave a chain of 64 waits on scalar loads -- the reference's own 512 x 512 x 64 field
// (scene_config/config_voxel_params.txt:1-3) ran at a third of the 512^3 field's rate per voxel.  Here a lane owns a column: its 60 products live in 30 register pairs (made from
// the x / y tables once per block and 64 z: no P array, no launch for it) and the z table -- uniform over the wave -- arrives as SCALAR operands (s_load_dwordx8 of the
// transposed table ZT[k][z]: 15 KB per block, shared by its four waves and hot in the scalar cache), eight z per pass = four independent packed accumulator chains.  (The z
// slice in LDS, read as 16-byte broadcasts, was LDS-bound: a broadcast still moves 1 KB per wave and read.)  The results leave through a 64 x 16 transposition piece in LDS so
// that the stores are 16-byte words of whole 64-byte segments.  Same arithmetic, same order as k_voxel_sines: product rounded, then added, k ascending.
// (Pipelining the scalar loads by hand -- stages of two loads, double-buffered, the next stage issued behind the wait for this one -- was measured EQUAL, 47.4 vs 45.7 us for
// 512 x 512 x 64, with the scalar registers at their limit: the compiler's schedule stays.  What is left against the 29 us of packed instructions at full issue is not the waits.)
constexpr unsigned VC_COLS = 256, VC_Z = 64, VC_PIECE = 16, VC_TSTRIDE = 20; // columns per block (a lane each), z per block, z per transposition piece, floats per column in it
typedef float vc_v8f __attribute__((ext_vector_type(8)));
// the table is read through the CONSTANT address space: nothing writes it while the kernel runs, and a uniform load from there is a scalar load whatever stores lie around it
// (as a plain global pointer the compiler kept the loads of the first pass scalar and made vector loads + readfirstlane of the rest, behind the kernel's own stores)
typedef float vc_v16f __attribute__((ext_vector_type(16)));
typedef vc_v16f const __attribute__((address_space(4))) *vc_zt_ptr;
template<int ODD> __device__ __forceinline__ void vc_mul_add4(sg_v2f (&acc)[4], sg_v2f pp, vc_v8f zz) {
	sg_v2f t0, t1, t2, t3;
	sg_v2f const z0 = {zz.s0, zz.s1}, z1 = {zz.s2, zz.s3}, z2 = {zz.s4, zz.s5}, z3 = {zz.s6, zz.s7};
	if (ODD == 0) {
		asm("v_pk_mul_f32 %4, %8, %9 op_sel:[0,0] op_sel_hi:[0,1]\n\tv_pk_mul_f32 %5, %8, %10 op_sel:[0,0] op_sel_hi:[0,1]\n\tv_pk_mul_f32 %6, %8, %11 op_sel:[0,0] op_sel_hi:[0,1]\n\tv_pk_mul_f32 %7, %8, %12 op_sel:[0,0] op_sel_hi:[0,1]\n\t"
		    "v_pk_add_f32 %0, %0, %4\n\tv_pk_add_f32 %1, %1, %5\n\tv_pk_add_f32 %2, %2, %6\n\tv_pk_add_f32 %3, %3, %7"
		    : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3) : "v"(pp), "s"(z0), "s"(z1), "s"(z2), "s"(z3));
	}
	else {
		asm("v_pk_mul_f32 %4, %8, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\tv_pk_mul_f32 %5, %8, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\tv_pk_mul_f32 %6, %8, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\tv_pk_mul_f32 %7, %8, %12 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
		    "v_pk_add_f32 %0, %0, %4\n\tv_pk_add_f32 %1, %1, %5\n\tv_pk_add_f32 %2, %2, %6\n\tv_pk_add_f32 %3, %3, %7"
		    : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3) : "v"(pp), "s"(z0), "s"(z1), "s"(z2), "s"(z3));
	}
}
// ZT[z/8][k][z%8]: the z table in passes of eight z (written by the table launch of terra_engine::voxel_fill_dev; nzp/8 passes: whole 64-z slices) -- the 60 rows of a pass are
// 1920 contiguous bytes, two rows per 64-byte scalar load; what lies behind nz is never stored
__global__ __launch_bounds__(256, 4) void k_voxel_sines_cols(float *__restrict__ out, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t nzp, float const *__restrict__ tab, float const *__restrict__ ZT, float zscale, int normalize) {
	__shared__ __attribute__((aligned(16))) float s_tp[4][64*VC_TSTRIDE];         // per wave: 64 columns x 16 z, 20 floats per column (16-byte aligned rows)
	size_t const ncol = (size_t)nx*ny, c = (size_t)blockIdx.x*VC_COLS + threadIdx.x;
	uint32_t const z0 = blockIdx.y*VC_Z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	sg_v2f pp[VOX_SINES/2];
	{
		bool const live = c < ncol;
		uint32_t const x = live ? (uint32_t)(c % nx) : 0u, y = live ? (uint32_t)(c / nx) : 0u;
		float const *xt = tab + (size_t)x*VOX_SINES, *yt = tab + ((size_t)nx + y)*VOX_SINES;
#pragma unroll
		for (unsigned j = 0; j < VOX_SINES/2; ++j) {pp[j] = sg_v2f{__fmul_rn(xt[2*j], yt[2*j]), __fmul_rn(xt[2*j + 1], yt[2*j + 1])};}
	}
	float *tp = s_tp[wave];
	size_t const wc0 = (size_t)blockIdx.x*VC_COLS + (size_t)wave*64; // the wave's first column
#pragma unroll 1
	for (unsigned piece = 0; piece < VC_Z/VC_PIECE; ++piece) {
		if (z0 + piece*VC_PIECE >= nz) break;
#pragma unroll
		for (unsigned half = 0; half < 2; ++half) { // eight z per pass
			unsigned const zl = piece*VC_PIECE + half*8;
			float const *zrow = ZT + (size_t)((z0 + zl) >> 3)*(VOX_SINES*8); // (wave-uniform: scalar loads)
			sg_v2f acc[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
			for (unsigned j = 0; j < VOX_SINES/2; ++j) {
				vc_v16f const zz = *(vc_zt_ptr)(uintptr_t)(zrow + 16*j); // the eight z of this pass for k = 2j and k = 2j + 1: one 64-byte scalar load
				vc_mul_add4<0>(acc, pp[j], vc_v8f{zz.s0, zz.s1, zz.s2, zz.s3, zz.s4, zz.s5, zz.s6, zz.s7});
				vc_mul_add4<1>(acc, pp[j], vc_v8f{zz.s8, zz.s9, zz.sa, zz.sb, zz.sc, zz.sd, zz.se, zz.sf});
			}
			float v[8] = {acc[0].x, acc[0].y, acc[1].x, acc[1].y, acc[2].x, acc[2].y, acc[3].x, acc[3].y};
#pragma unroll
			for (unsigned q = 0; q < 8; ++q) {
				float r = __fadd_rn(v[q], __fmul_rn((float)(z0 + zl + q), zscale));
				if (normalize) {r = clip_pm1(r);}
				v[q] = r;
			}
			*(st_f4 *)&tp[lane*VC_TSTRIDE + half*8]     = st_f4{v[0], v[1], v[2], v[3]};
			*(st_f4 *)&tp[lane*VC_TSTRIDE + half*8 + 4] = st_f4{v[4], v[5], v[6], v[7]};
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
		// the piece leaves transposed: a lane stores four consecutive z of one column (16 bytes), four lanes a column's 64-byte segment
		uint32_t const zp = z0 + piece*VC_PIECE;
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) {
			unsigned const idx = q*64 + lane, col = idx >> 2, zq = (idx & 3u)*4u;
			st_f4 const w = *(st_f4 const *)&tp[col*VC_TSTRIDE + zq];
			if (wc0 + col < ncol && zp + zq < nz) {__builtin_nontemporal_store(w, (st_f4 *)&out[(wc0 + col)*nz + zp + zq]);}
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); __builtin_amdgcn_wave_barrier();
	}
}
} // namespace terra
