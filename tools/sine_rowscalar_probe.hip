// Probe for the main loop of k_sine_grid<false, false, 27> (3dworld_amd/csrc/terra_kernels.hpp): does the sum run faster when a row's operand is a SCALAR?
//   form A   today's loop, instruction for instruction: 128 x 128 cells per block, 8 x 8 per lane, X and Y chunks in LDS, four ds_read_b128 per term, Y in registers
//   form B   a wave is 64 lanes along x, a lane owns 4 columns x 16 rows (the same 32 packed accumulators), a block is four waves stacked in y (256 x 64 cells): only X is
//            staged in LDS (one ds_read_b128 per term), the 16 row values of a term arrive by ONE 64-byte scalar load and feed v_pk_mul_f32 from SGPR pairs through op_sel
// Both hold the staging and the sum of the headline's shape (terms kstart .. 89 in chunks of at most KC = 27: three chunks of 27, 27, 26 for 80 terms) and nothing else: no
// epilogue, no store (the accumulators are kept alive by an empty asm).  The tables are random and non-zero.  A checking instantiation writes the sums out; the host
// compares the forms bit for bit on a small grid and samples them against the product-rounded-then-added chain in k order.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/sine_rowscalar_probe.hip -o tools/_bin/sine_rowscalar_probe
//   hipcc ... -DRS_STAMPS tools/sine_rowscalar_probe.hip -o tools/_bin/sine_rowscalar_probe_stamps    (diagnostic build: the in-kernel clock around the loop)
//   sine_rowscalar_probe [n=16384] [kstart=10] [seconds=2.0] [reps=5] [sweeps=1]
// Form B's variants: TOUCH = every wave first reads its Y lines with vector loads (a lane per 64-byte line), so that the scalar loads find them in the L2;
// the launch can carry dynamic LDS that is never used, which limits a CU to four or three blocks (waves per SIMD) instead of five.
//   sine_rowscalar_probe n kstart seconds reps 0 epilogue    form B's loop as cumulative STAGES up to k_sine_grid_rs<27>, and the candidates as variants of the last stage
//     B0 = form B;  B1 = B0 + the packed interior epilogue (glaciate and island term on; island columns from LDS row KC + 1, the 16 row terms by one scalar load; folded
//     into the lane's min / max, nothing stored);  B2 = B1 + the sixteen 1 KB row stores per wave;  B3 = B2 + the wave min / max publish = the library kernel's interior path.
//     Variants of B3: nontemporal stores; two chunks of 40 terms (42 KB of LDS); the island operands asked for in front of the last chunk's last term, in the place of the
//     prefetch nobody uses; s_setprio 1 from the first epilogue instruction on.  Every stage that writes is checked on 1024^2 against form A's sums put through the same
//     epilogue statements on the host, and its min / max words against the host's.  "pmc" in the place of "epilogue": a few launches per form, for a counter pass.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cmath>
#include <vector>
#include <random>
#include <algorithm>

#define CK(e) do {hipError_t const e_ = (e); if (e_ != hipSuccess) {printf("%s: %s\n", #e, hipGetErrorString(e_)); exit(1);}} while (0)

constexpr int F_TABLE_SIZE = 90, KC = 27, TABLE_ROWS = F_TABLE_SIZE + 1; // a zero row behind the last term, as the library's tables have: form A's staging and form B's last prefetch read it
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));   // scalar operands are kept in integer types: uniform integers stay in SGPRs across loop-carried copies
typedef unsigned u16 __attribute__((ext_vector_type(16)));

struct job_t {
	float const *xt, *yt; // [TABLE_ROWS][nxp], [TABLE_ROWS][nyp]
	unsigned nxp, nyp, ntx, nty, rowgroup, n;
	int kstart;
	float *out;                  // checking instantiations and the stages that store: [n][n]
	float const *smx, *smy;      // the stages' island terms, [n] each
	float zme, inv, z2, off;     // the stages' epilogue constants (zmax_est, 1/(2 zmax_est), 2 zmax_est, sine_offset)
	unsigned *mm;                // stage B3: the two min / max words
	unsigned long long *stamps;  // -DRS_STAMPS: per block {shader clock ticks, 100 MHz ticks} around the chunk loop
};

__host__ __device__ constexpr int chunk_len(int kstart, int kc) {int const nk = F_TABLE_SIZE - kstart, n = (nk + kc - 1)/kc; return (nk > 0 && n > 0) ? (nk + n - 1)/n : 0;}

// ---- copied from terra_kernels.hpp (K1): tile order, the packed 2 x 8 step, the wave-uniform helpers, the direct-to-LDS load
__device__ __forceinline__ bool tile_of_block(unsigned b, unsigned ntx, unsigned nty, unsigned rowgroup, unsigned &bx, unsigned &by) {
	unsigned const nb = ntx*nty, per_xcd = (nb + 7)/8;
	unsigned const lin = (b & 7)*per_xcd + (b >> 3);
	if (lin >= nb) return false;
	unsigned const group = lin/(rowgroup*ntx), r = lin % (rowgroup*ntx);
	unsigned const rows_here = (nty - group*rowgroup < rowgroup) ? nty - group*rowgroup : rowgroup;
	bx = r/rows_here; by = group*rowgroup + r % rows_here;
	return bx < ntx;
}
__device__ __forceinline__ void mul_add_2x8(v2f (&r0)[4], v2f (&r1)[4], v2f const (&xp)[4], v2f yp) {
	v2f t0, t1;
#define RS_2X2(A0, A1, X) \
	"v_pk_mul_f32 %8, " X ", %13 op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %9, " X ", %13 op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " A0 ", " A0 ", %8\n\t" \
	"v_pk_add_f32 " A1 ", " A1 ", %9\n\t"
	asm(RS_2X2("%0", "%4", "%10") RS_2X2("%1", "%5", "%11") RS_2X2("%2", "%6", "%12") RS_2X2("%3", "%7", "%14")
	    : "+v"(r0[0]), "+v"(r0[1]), "+v"(r0[2]), "+v"(r0[3]), "+v"(r1[0]), "+v"(r1[1]), "+v"(r1[2]), "+v"(r1[3]), "=&v"(t0), "=&v"(t1)
	    : "v"(xp[0]), "v"(xp[1]), "v"(xp[2]), "v"(yp), "v"(xp[3]));
#undef RS_2X2
}
struct xop_t {float4 a, b;};
__device__ __forceinline__ xop_t load_x(float const *px, int k) {return xop_t{*(float4 const *)(px + k*128), *(float4 const *)(px + k*128 + 64)};}
__device__ __forceinline__ void accumulate_half(v2f (&acc)[8][4], xop_t const &x, float4 const &y, int h) {
	v2f const xp[4] = {{x.a.x, x.a.y}, {x.a.z, x.a.w}, {x.b.x, x.b.y}, {x.b.z, x.b.w}};
	mul_add_2x8(acc[4*h], acc[4*h + 1], xp, v2f{y.x, y.y});
	mul_add_2x8(acc[4*h + 2], acc[4*h + 3], xp, v2f{y.z, y.w});
}
__device__ __forceinline__ unsigned wave_uniform(unsigned v) {return (unsigned)__builtin_amdgcn_readfirstlane((int)v);}
__device__ __forceinline__ char const *wave_uniform_ptr(void const *p) {uint64_t const v = (uint64_t)(uintptr_t)p; return (char const *)(uintptr_t)(((uint64_t)wave_uniform((unsigned)(v >> 32)) << 32) | wave_uniform((unsigned)v));}
__device__ __forceinline__ void load16_to_lds(void const *g, float *lds) {
	__builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(uintptr_t)g, (__attribute__((address_space(3))) void *)lds, 16, 0, 0);
}

__device__ __forceinline__ void load4_to_lds(void const *g, float *lds) {
	__builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(uintptr_t)g, (__attribute__((address_space(3))) void *)lds, 4, 0, 0);
}
// ---- copied from terra_noise_kernels.hpp / terra_common.hpp: the order-preserving words and the publish of a wave whose 64 lanes are all active
__host__ __device__ inline unsigned f2ord(float f) {unsigned u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u);}
__device__ __forceinline__ unsigned wave_min_u32_full(unsigned v) {
#define RS_DPP_MIN(CTRL) {unsigned const o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false); v = (o < v) ? o : v;}
	RS_DPP_MIN(0xB1) RS_DPP_MIN(0x4E) RS_DPP_MIN(0x141) RS_DPP_MIN(0x140)
#undef RS_DPP_MIN
	unsigned const a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16), c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
	unsigned const ab = (a < b) ? a : b, cd = (c < d) ? c : d;
	return (ab < cd) ? ab : cd;
}
__device__ __forceinline__ void wave_minmax_publish_full(unsigned lo, unsigned hi, unsigned *mm) {
	lo = wave_min_u32_full(lo); hi = wave_min_u32_full(hi);
	if ((threadIdx.x & 63) == 0 && lo != 0xFFFFFFFFu) {
		if (lo < __hip_atomic_load(&mm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {atomicMin(&mm[0], lo);}
		if (hi < __hip_atomic_load(&mm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {atomicMin(&mm[1], hi);}
	}
}
__device__ __forceinline__ float min3(float a, float b, float c) {float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;}
__device__ __forceinline__ float max3(float a, float b, float c) {float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;}
template<int SEL> __device__ __forceinline__ v2f pk_mul_bcast_s(v2f a, u2 yp) {
	v2f r;
	if (SEL) {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "s"(yp));}
	else     {asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "s"(yp));}
	return r;
}
typedef u16 const __attribute__((address_space(4))) *row16_ptr;

#ifdef RS_STAMPS
#define RS_STAMP_BEGIN unsigned long long const st_c0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
#define RS_STAMP_END(J, B) {unsigned long long const st_c1 = __builtin_amdgcn_s_memtime(), st_r1 = __builtin_amdgcn_s_memrealtime(); \
	if (threadIdx.x == 0 && (J).stamps) {(J).stamps[2*(size_t)(B)] = st_c1 - st_c0; (J).stamps[2*(size_t)(B) + 1] = st_r1 - st_r0;}}
#else
#define RS_STAMP_BEGIN
#define RS_STAMP_END(J, B)
#endif

// ---- form A: the staging and the loop of k_sine_grid<false, false, 27> as they stand
template<bool CHECK> __global__ __launch_bounds__(256) void k_form_a(job_t const J) {
	__shared__ __attribute__((aligned(16))) float sX[(KC + 2)*128];
	__shared__ __attribute__((aligned(16))) float sY[(KC + 2)*128];
	unsigned bxi, byi;
	if (!tile_of_block(blockIdx.x, J.ntx, J.nty, J.rowgroup, bxi, byi)) return;
	unsigned const tid = threadIdx.x, bx0 = bxi*128, by0 = byi*128;
	unsigned const tx = tid & 15, ty = tid >> 4;
	float const *px = sX + tx*4, *py = sY + ty*4;
	v2f acc[8][4];
#pragma unroll
	for (int i = 0; i < 8; ++i) {
#pragma unroll
		for (int jp = 0; jp < 4; ++jp) {acc[i][jp] = v2f{0.0f, 0.0f};}
	}
	int const nk = F_TABLE_SIZE - J.kstart, nchunks = (nk + KC - 1)/KC, per_chunk = chunk_len(J.kstart, KC);
	RS_STAMP_BEGIN
	for (int c = 0; c < nchunks; ++c) {
		int const k0 = J.kstart + c*per_chunk, kn = ((k0 + per_chunk > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per_chunk);
		if (c > 0) {__syncthreads();}
		{
			unsigned const w2 = wave_uniform(tid >> 6)*2u, lane = tid & 63u;
			unsigned const vx = ((lane >> 5)*J.nxp + (lane & 31u)*4u)*4u, vy = ((lane >> 5)*J.nyp + (lane & 31u)*4u)*4u;
			char const *gx = wave_uniform_ptr(J.xt + (size_t)(k0 + (int)w2)*J.nxp + bx0), *gy = wave_uniform_ptr(J.yt + (size_t)(k0 + (int)w2)*J.nyp + by0);
			for (int r = (int)w2; r < kn; r += 8) {
				load16_to_lds(gx + vx, sX + r*128); load16_to_lds(gy + vy, sY + r*128);
				gx += (size_t)J.nxp*32u; gy += (size_t)J.nyp*32u;
			}
		}
		__syncthreads();
		xop_t XA = load_x(px, 0), XB = load_x(px, 1);
		float4 ya = *(float4 const *)py, yb = *(float4 const *)(py + 64);
		int k = 0;
		for (; k + 1 < kn; k += 2) {
			accumulate_half(acc, XA, ya, 0); __builtin_amdgcn_sched_barrier(0); ya = *(float4 const *)(py + (k + 1)*128);
			accumulate_half(acc, XA, yb, 1); __builtin_amdgcn_sched_barrier(0); yb = *(float4 const *)(py + (k + 1)*128 + 64); XA = load_x(px, k + 2);
			accumulate_half(acc, XB, ya, 0); __builtin_amdgcn_sched_barrier(0); ya = *(float4 const *)(py + (k + 2)*128);
			accumulate_half(acc, XB, yb, 1); __builtin_amdgcn_sched_barrier(0); yb = *(float4 const *)(py + (k + 2)*128 + 64); XB = load_x(px, k + 3);
		}
		if (k < kn) {accumulate_half(acc, XA, ya, 0); accumulate_half(acc, XA, yb, 1);}
	}
	RS_STAMP_END(J, blockIdx.x)
	if (CHECK) { // lane (tx, ty): columns {4 tx ..} u {64 + 4 tx ..}, rows {4 ty ..} u {64 + 4 ty ..}
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			unsigned const y = by0 + (i >> 2)*64 + ty*4 + (i & 3);
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				*(float4 *)(J.out + (size_t)y*J.n + bx0 + half*64 + tx*4) = make_float4(acc[i][half*2].x, acc[i][half*2].y, acc[i][half*2 + 1].x, acc[i][half*2 + 1].y);
			}
		}
	}
	else {
#pragma unroll
		for (int i = 0; i < 8; ++i) {
#pragma unroll
			for (int jp = 0; jp < 4; ++jp) {asm volatile("" :: "v"(acc[i][jp]));}
		}
	}
}

// ---- form B: rows from scalar loads
// Eight rows x four columns per asm statement (two statements per term: the compiler puts an s_nop behind every statement).  Per row pair, r0 += {x0*y0, x1*y0}, {x2*y0, x3*y0}
// and r1 the same with y1: (y0, y1) is an SGPR pair, the row's value broadcast from either half by op_sel.  mul / mul / add / add as in form A: one independent instruction
// between a product and the add that takes it; product rounded by v_pk_mul_f32, then added by v_pk_add_f32, never fused.
#define RS_2X4(R00, R01, R10, R11, Y) \
	"v_pk_mul_f32 %16, %18, " Y " op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %17, %18, " Y " op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " R00 ", " R00 ", %16\n\t" \
	"v_pk_add_f32 " R10 ", " R10 ", %17\n\t" \
	"v_pk_mul_f32 %16, %19, " Y " op_sel:[0,0] op_sel_hi:[1,0]\n\t" \
	"v_pk_mul_f32 %17, %19, " Y " op_sel:[0,1] op_sel_hi:[1,1]\n\t" \
	"v_pk_add_f32 " R01 ", " R01 ", %16\n\t" \
	"v_pk_add_f32 " R11 ", " R11 ", %17\n\t"
__device__ __forceinline__ void mul_add_8x4_s(v2f (&acc)[16][2], int r, v2f x01, v2f x23, u2 y01, u2 y23, u2 y45, u2 y67) { // rows r .. r + 7
	v2f t0, t1;
	asm(RS_2X4("%0", "%1", "%2", "%3", "%20") RS_2X4("%4", "%5", "%6", "%7", "%21") RS_2X4("%8", "%9", "%10", "%11", "%22") RS_2X4("%12", "%13", "%14", "%15", "%23")
	    : "+v"(acc[r][0]), "+v"(acc[r][1]), "+v"(acc[r + 1][0]), "+v"(acc[r + 1][1]), "+v"(acc[r + 2][0]), "+v"(acc[r + 2][1]), "+v"(acc[r + 3][0]), "+v"(acc[r + 3][1]),
	      "+v"(acc[r + 4][0]), "+v"(acc[r + 4][1]), "+v"(acc[r + 5][0]), "+v"(acc[r + 5][1]), "+v"(acc[r + 6][0]), "+v"(acc[r + 6][1]), "+v"(acc[r + 7][0]), "+v"(acc[r + 7][1]),
	      "=&v"(t0), "=&v"(t1)
	    : "v"(x01), "v"(x23), "s"(y01), "s"(y23), "s"(y45), "s"(y67));
}
#undef RS_2X4
__device__ __forceinline__ void accumulate_term(v2f (&acc)[16][2], v4f const &x, u16 const &y) {
	v2f const x01 = {x.x, x.y}, x23 = {x.z, x.w};
	mul_add_8x4_s(acc, 0, x01, x23, u2{y.s0, y.s1}, u2{y.s2, y.s3}, u2{y.s4, y.s5}, u2{y.s6, y.s7});
	mul_add_8x4_s(acc, 8, x01, x23, u2{y.s8, y.s9}, u2{y.sa, y.sb}, u2{y.sc, y.sd}, u2{y.se, y.sf});
}
// A stage is one term: wait for this term's operands (LDS reads and scalar loads share the counter and scalar loads return out of order, so the only wait is lgkmcnt(0)),
// then put the next term's ds_read_b128 and 64-byte scalar load in flight, then run this term's 64 packed instructions.  The buffers are asm operands from issue to use.
// (Two asm statements per stage, in this order: an asm whose outputs mix vector and scalar registers makes all of them divergent values for the compiler, which then cannot
// carry the scalar buffers around the loop.)
#define RS_NEXT(CX, CY, NX, NY, LADDR, OFF, YP) \
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %1, %2, 0x0" : "+s"(CY), "=&s"(NY) : "s"(YP)); \
	asm volatile("ds_read_b128 %1, %2 offset:" #OFF : "+v"(CX), "=&v"(NX) : "v"(LADDR))
#define RS_WAIT(X, Y) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(Y)); asm volatile("" : "+v"(X))
// STAGE 0 is form B.  STAGE 1 .. 3 add, cumulatively, what k_sine_grid_rs<27> runs behind the loop in a block inside the grid with glaciate and the island term on: the island
// columns' direct-to-LDS load in front of the chunks and the packed epilogue (1), the row stores (2), the min / max publish (3).  KCC: terms per chunk.  VAR: candidates.
enum {V_NT = 1, V_EARLY = 2, V_PRIO = 4};
template<bool TOUCH, bool CHECK, int STAGE = 0, int KCC = KC, int VAR = 0> __global__ __launch_bounds__(256) void k_form_b(job_t const J) {
	__shared__ __attribute__((aligned(16))) float sX[(KCC + 2)*256]; // rows kn, kn + 1 may be read, never used; row KCC + 1 holds the island columns (STAGE >= 1)
	unsigned bxi, byi;
	if (!tile_of_block(blockIdx.x, J.ntx, J.nty, J.rowgroup, bxi, byi)) return;
	unsigned const tid = threadIdx.x, bx0 = bxi*256, by0 = byi*64;
	unsigned const w = wave_uniform(tid >> 6), lane = tid & 63u;
	v2f acc[16][2];
#pragma unroll
	for (int i = 0; i < 16; ++i) {acc[i][0] = v2f{0.0f, 0.0f}; acc[i][1] = v2f{0.0f, 0.0f};}
	int const nk = F_TABLE_SIZE - J.kstart, nchunks = (nk + KCC - 1)/KCC, per_chunk = chunk_len(J.kstart, KCC);
	if (STAGE >= 1) { // as the kernel: the block's 256 island column terms into the spare LDS row, 64 per wave; the first chunk's barrier waits for them
		load4_to_lds(J.smx + bx0 + w*64u + lane, sX + (KCC + 1)*256 + w*64u);
		if (nchunks <= 0) {__syncthreads();}
	}
	size_t const rowb = (size_t)J.nyp*4u;
	char const *const ybase = wave_uniform_ptr(J.yt + by0 + w*16u); // the wave's 16 rows of table row 0: 64 bytes, 64-byte aligned
	float touched0 = 0.0f, touched1 = 0.0f;
	if (TOUCH) { // rows kstart .. kstart + 127 <= TABLE_ROWS - 1 clamped: a lane per 64-byte line
		unsigned const r0 = (unsigned)J.kstart + lane, r1 = r0 + 64u, last = TABLE_ROWS - 1;
		float const *ta = J.yt + (size_t)((r0 < last) ? r0 : last)*J.nyp + by0 + w*16u, *tb = J.yt + (size_t)((r1 < last) ? r1 : last)*J.nyp + by0 + w*16u;
		asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off" : "=&v"(touched0), "=&v"(touched1) : "v"(ta), "v"(tb));
	}
	RS_STAMP_BEGIN
	v4f xa, xb; u16 ya, yb;
	unsigned const la = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)sX + lane*16u; // the lane's four columns of LDS row 0
	// V_EARLY: the last prefetch of the last chunk, which nobody uses when the chunk's length is even, asks for the epilogue's operands instead -- the lane's four island
	// columns and the wave's 16 island row terms -- so they arrive under the last term's 64 packed instructions
	constexpr bool EARLY = (VAR & V_EARLY) && STAGE >= 1;
	char const *const isl_y = wave_uniform_ptr(J.smy + by0 + w*16u);
	bool early_got = false;
	for (int c = 0; c < nchunks; ++c) {
		int const k0 = J.kstart + c*per_chunk, kn = ((k0 + per_chunk > F_TABLE_SIZE) ? F_TABLE_SIZE - k0 : per_chunk);
		if (c > 0) {__syncthreads();}
		// the chunk's first row operands are asked for in front of the staging and land under it.  No scalar buffer is live from one chunk to the next: a buffer whose load is
		// in flight must never meet a copy, and the compiler puts copies where two paths join (it did, in front of the wait, when the odd and the even end of a chunk handed
		// the next chunk's operands on)
		char const *yp = ybase + (size_t)k0*rowb;
		asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(ya) : "s"(yp));
		{	// one 16-byte direct-to-LDS load per wave is one whole 256-float row; wave w takes rows w, w + 4, ... below kn
			char const *gx = wave_uniform_ptr(J.xt + (size_t)(k0 + (int)w)*J.nxp + bx0);
			for (int r = (int)w; r < kn; r += 4) {load16_to_lds(gx + lane*16u, sX + r*256); gx += (size_t)J.nxp*16u;}
		}
		__syncthreads();
		asm volatile("ds_read_b128 %0, %1" : "=&v"(xa) : "v"(la));
		unsigned a = la;
		int k = 0;
		bool const early_chunk = EARLY && c == nchunks - 1 && !(kn & 1);
		for (; k + 1 < kn; k += 2) { // (the last pair's second stage asks for LDS row kn and table row k0 + kn <= 90: both exist, neither is used)
			RS_NEXT(xa, ya, xb, yb, a, 1024, yp + rowb);   accumulate_term(acc, xa, ya); __builtin_amdgcn_sched_barrier(0);
			if (EARLY) {
				bool const fin = early_chunk && k + 2 >= kn;
				unsigned const a2 = a + (fin ? (unsigned)(KCC + 1)*1024u - (unsigned)k*1024u : 2048u);
				char const *const y2 = fin ? isl_y : yp + 2*rowb;
				RS_NEXT(xb, yb, xa, ya, a2, 0, y2);
			}
			else {RS_NEXT(xb, yb, xa, ya, a, 2048, yp + 2*rowb);}
			accumulate_term(acc, xb, yb); __builtin_amdgcn_sched_barrier(0);
			a += 2048u; yp += 2*rowb;
		}
		RS_WAIT(xa, ya); // nothing is in flight when the block meets at the next barrier
		if (k < kn) {accumulate_term(acc, xa, ya); __builtin_amdgcn_sched_barrier(0);}
		early_got = early_chunk && kn >= 2;
	}
	if (STAGE == 0) {RS_STAMP_END(J, blockIdx.x)}
	if (TOUCH) {asm volatile("s_waitcnt vmcnt(0)" : "+v"(touched0), "+v"(touched1));}
	if (STAGE >= 1) { // ---- the interior epilogue of k_sine_grid_rs, glaciate and island term on
		if (VAR & V_PRIO) {__builtin_amdgcn_s_setprio(1);}
		v4f sx; u16 sy;
		if (EARLY && early_got) {sx = xa; sy = ya;}
		else {sx = *(v4f const *)(sX + (KCC + 1)*256 + lane*4u); sy = *(row16_ptr)(uintptr_t)(J.smy + by0 + w*16u);}
		v2f const zme = {J.zme, J.zme}, inv = {J.inv, J.inv}, z2 = {J.z2, J.z2}, off = {J.off, J.off};
		float fmn = INFINITY, fmx = -INFINITY;
		unsigned const voff = lane*16u;
		char *const ob = (char *)(J.out + (size_t)(by0 + w*16u)*J.n + bx0);
		size_t const rowbytes = (size_t)J.n*4u;
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			v2f z01 = acc[i][0], z23 = acc[i][1];
			v2f const r01 = (z01 + zme)*inv, r23 = (z23 + zme)*inv;
			z01 = ((r01*r01)*r01)*z2 - zme; z23 = ((r23*r23)*r23)*z2 - zme;
			v2f const s01 = {sx.x, sx.y}, s23 = {sx.z, sx.w};
			u2 const syp = {sy[i & ~1], sy[i | 1]};
			z01 = z01 + (((i & 1) ? pk_mul_bcast_s<1>(s01, syp) : pk_mul_bcast_s<0>(s01, syp)) + off); z23 = z23 + (((i & 1) ? pk_mul_bcast_s<1>(s23, syp) : pk_mul_bcast_s<0>(s23, syp)) + off);
			fmn = min3(min3(fmn, z01.x, z01.y), z23.x, z23.y);
			fmx = max3(max3(fmx, z01.x, z01.y), z23.x, z23.y);
			if (STAGE >= 2) {
				if (VAR & V_NT) {__builtin_nontemporal_store(v4f{z01.x, z01.y, z23.x, z23.y}, (v4f *)(ob + (size_t)i*rowbytes + voff));}
				else {*(float4 *)(ob + (size_t)i*rowbytes + voff) = make_float4(z01.x, z01.y, z23.x, z23.y);}
			}
		}
		if (STAGE >= 3) {
			unsigned mm_lo = 0xFFFFFFFFu, mm_hi = 0xFFFFFFFFu;
			if (fmn <= fmx) {mm_lo = f2ord(fmn); mm_hi = ~f2ord(fmx);}
			wave_minmax_publish_full(mm_lo, mm_hi, J.mm);
		}
		else {asm volatile("" :: "v"(fmn), "v"(fmx));}
		RS_STAMP_END(J, blockIdx.x)
	}
	else if (CHECK) { // lane: columns bx0 + 4 lane .., rows by0 + 16 w + i
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			*(float4 *)(J.out + (size_t)(by0 + w*16u + (unsigned)i)*J.n + bx0 + lane*4u) = make_float4(acc[i][0].x, acc[i][0].y, acc[i][1].x, acc[i][1].y);
		}
	}
	else {
#pragma unroll
		for (int i = 0; i < 16; ++i) {asm volatile("" :: "v"(acc[i][0])); asm volatile("" :: "v"(acc[i][1]));}
	}
}

// ---- host
static uint32_t bits(float f) {uint32_t u; memcpy(&u, &f, 4); return u;}
enum {FORM_A = 0, FORM_B, FORM_BT, NFORMS};
static char const *const form_name[NFORMS] = {"A  8x8 per lane, X and Y in LDS   ", "B  4x16 per lane, Y scalar        ", "Bt 4x16 per lane, Y scalar, touch "};

static void launch(int form, bool check, job_t J, unsigned n, unsigned rowgroup, unsigned extra_lds) {
	if (form == FORM_A) {J.ntx = n/128; J.nty = n/128;} else {J.ntx = n/256; J.nty = n/64;}
	J.rowgroup = rowgroup;
	unsigned const grid = (J.ntx*J.nty + 7)/8*8;
	if (form == FORM_A) {if (check) hipLaunchKernelGGL(k_form_a<true>, dim3(grid), dim3(256), extra_lds, 0, J); else hipLaunchKernelGGL(k_form_a<false>, dim3(grid), dim3(256), extra_lds, 0, J);}
	else if (form == FORM_B) {if (check) hipLaunchKernelGGL((k_form_b<false, true>), dim3(grid), dim3(256), extra_lds, 0, J); else hipLaunchKernelGGL((k_form_b<false, false>), dim3(grid), dim3(256), extra_lds, 0, J);}
	else {if (check) hipLaunchKernelGGL((k_form_b<true, true>), dim3(grid), dim3(256), extra_lds, 0, J); else hipLaunchKernelGGL((k_form_b<true, false>), dim3(grid), dim3(256), extra_lds, 0, J);}
}
// back-to-back launches for at least `seconds`: ms per launch
static double time_form(int form, job_t const &J, unsigned n, unsigned rowgroup, unsigned extra_lds, double seconds, hipEvent_t e0, hipEvent_t e1, long *launches = nullptr) {
	for (int r = 0; r < 10; ++r) {launch(form, false, J, n, rowgroup, extra_lds);}
	CK(hipDeviceSynchronize());
	double total = 0.0; long count = 0;
	while (total < seconds*1e3) {
		int const batch = 200;
		CK(hipEventRecord(e0));
		for (int r = 0; r < batch; ++r) {launch(form, false, J, n, rowgroup, extra_lds);}
		CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
		float ms; CK(hipEventElapsedTime(&ms, e0, e1)); total += ms; count += batch;
	}
	CK(hipGetLastError());
	if (launches) {*launches = count;}
	return total/count;
}

// ---- the stages of form B up to the library kernel, and the candidates as variants of the last stage
struct eform_t {char const *name; int stage, kc, var;};
static eform_t const eforms[] = {
	{"B0  the loop alone (form B)         ", 0, 27, 0},
	{"B1  B0 + epilogue, nothing stored   ", 1, 27, 0},
	{"B2  B1 + 16 row stores per wave     ", 2, 27, 0},
	{"B3  B2 + min/max publish (= kernel) ", 3, 27, 0},
	{"B3n B3, nontemporal stores          ", 3, 27, V_NT},
	{"B3c B3, two chunks of 40 terms      ", 3, 40, 0},
	{"B3e B3, island operands early       ", 3, 27, V_EARLY},
	{"B3p B3, s_setprio 1 in the epilogue ", 3, 27, V_PRIO},
	{"B3x B3, all four                    ", 3, 40, V_NT | V_EARLY | V_PRIO}};
constexpr int NEFORMS = (int)(sizeof(eforms)/sizeof(eforms[0])), EFORM_B3 = 3;
static void launch_e(int f, job_t J, unsigned n, unsigned rowgroup) {
	J.ntx = n/256; J.nty = n/64; J.rowgroup = rowgroup;
	dim3 const grid((J.ntx*J.nty + 7)/8*8), block(256);
	switch (f) {
	case 0: hipLaunchKernelGGL((k_form_b<false, false, 0, 27, 0>), grid, block, 0, 0, J); break;
	case 1: hipLaunchKernelGGL((k_form_b<false, false, 1, 27, 0>), grid, block, 0, 0, J); break;
	case 2: hipLaunchKernelGGL((k_form_b<false, false, 2, 27, 0>), grid, block, 0, 0, J); break;
	case 3: hipLaunchKernelGGL((k_form_b<false, false, 3, 27, 0>), grid, block, 0, 0, J); break;
	case 4: hipLaunchKernelGGL((k_form_b<false, false, 3, 27, V_NT>), grid, block, 0, 0, J); break;
	case 5: hipLaunchKernelGGL((k_form_b<false, false, 3, 40, 0>), grid, block, 0, 0, J); break;
	case 6: hipLaunchKernelGGL((k_form_b<false, false, 3, 27, V_EARLY>), grid, block, 0, 0, J); break;
	case 7: hipLaunchKernelGGL((k_form_b<false, false, 3, 27, V_PRIO>), grid, block, 0, 0, J); break;
	default: hipLaunchKernelGGL((k_form_b<false, false, 3, 40, V_NT | V_EARLY | V_PRIO>), grid, block, 0, 0, J); break;
	}
}
static double time_eform(int f, job_t const &J, unsigned n, double seconds, hipEvent_t e0, hipEvent_t e1, long *launches = nullptr, int warm = 10, int batch = 200) {
	for (int r = 0; r < warm; ++r) {launch_e(f, J, n, 8u);}
	CK(hipDeviceSynchronize());
	double total = 0.0; long count = 0;
	do {
		CK(hipEventRecord(e0));
		for (int r = 0; r < batch; ++r) {launch_e(f, J, n, 8u);}
		CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
		float ms; CK(hipEventElapsedTime(&ms, e0, e1)); total += ms; count += batch;
	} while (total < seconds*1e3);
	CK(hipGetLastError());
	if (launches) {*launches = count;}
	return total/count;
}
// the epilogue's statements on the host (compiled with -ffp-contract=off; the volatiles keep every product and sum a rounded float)
static float host_epilogue(float z, float sx, float sy, job_t const &J) {
	volatile float r = z + J.zme; r = r*J.inv;
	volatile float c = r*r; c = c*r; c = c*J.z2; c = c - J.zme;
	volatile float s = sx*sy; s = s + J.off;
	volatile float o = c + s;
	return o;
}
// 0 = every stage that writes gives, on the nc x nc corner, the bits of `sums` (form A's) put through host_epilogue, and stage 3 the min / max words of that grid
static int check_eforms(job_t const &J, unsigned nc, std::vector<float> const &sums, std::vector<float> const &hsx, std::vector<float> const &hsy) {
	std::vector<float> want((size_t)nc*nc), got((size_t)nc*nc);
	float lo = INFINITY, hi = -INFINITY;
	for (unsigned y = 0; y < nc; ++y) {for (unsigned x = 0; x < nc; ++x) {float const v = host_epilogue(sums[(size_t)y*nc + x], hsx[x], hsy[y], J); want[(size_t)y*nc + x] = v; lo = std::min(lo, v); hi = std::max(hi, v);}}
	job_t C = J; C.n = nc;
	float *o; unsigned *mm; CK(hipMalloc(&o, (size_t)nc*nc*4)); CK(hipMalloc(&mm, 8));
	C.out = o; C.mm = mm;
	int failed = 0;
	for (int f = 0; f < NEFORMS; ++f) {
		if (eforms[f].stage < 2) continue;
		CK(hipMemset(o, 0xFF, (size_t)nc*nc*4)); CK(hipMemset(mm, 0xFF, 8));
		launch_e(f, C, nc, 8u); CK(hipDeviceSynchronize()); CK(hipGetLastError());
		unsigned hmm[2]; CK(hipMemcpy(got.data(), o, (size_t)nc*nc*4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hmm, mm, 8, hipMemcpyDeviceToHost));
		unsigned long long diff = 0;
		for (size_t i = 0; i < (size_t)nc*nc; ++i) {diff += bits(want[i]) != bits(got[i]);}
		bool const mm_ok = eforms[f].stage < 3 || (hmm[0] == f2ord(lo) && hmm[1] == ~f2ord(hi));
		printf("check %u^2 form %s cells that differ from form A's sums through the host's epilogue: %llu; min / max words %s\n", nc, eforms[f].name, diff, eforms[f].stage < 3 ? "not written" : (mm_ok ? "equal" : "DIFFER"));
		failed += (diff != 0) || !mm_ok;
	}
	CK(hipFree(o)); CK(hipFree(mm));
	return failed;
}

int main(int argc, char **argv) {
	unsigned const n = (argc > 1) ? atoi(argv[1]) : 16384;
	int const kstart = (argc > 2) ? atoi(argv[2]) : 10;
	double const seconds = (argc > 3) ? atof(argv[3]) : 2.0;
	int const reps = (argc > 4) ? atoi(argv[4]) : 5;
	int const sweeps = (argc > 5) ? atoi(argv[5]) : 1;
	bool const pmc = argc > 6 && !strcmp(argv[6], "pmc"), stages = pmc || (argc > 6 && !strcmp(argv[6], "epilogue"));
	if (n == 0 || n % 256 != 0 || kstart < 0 || kstart >= F_TABLE_SIZE) {printf("n must be a multiple of 256, kstart in 0 .. 89\n"); return 1;}
	unsigned const nc = 1024; // the checked grid
	std::mt19937 rng(11);
	std::uniform_real_distribution<float> U(0.05f, 1.0f);
	auto const rnd = [&]() {float const v = U(rng); return (rng() & 1u) ? v : -v;}; // never zero, either sign
	job_t J; memset(&J, 0, sizeof(J));
	J.nxp = J.nyp = n; J.n = n; J.kstart = kstart;
	std::vector<float> hx((size_t)TABLE_ROWS*n, 0.0f), hy((size_t)TABLE_ROWS*n, 0.0f);
	for (int k = 0; k < F_TABLE_SIZE; ++k) {float const amp = 1.0f/(1.0f + 0.1f*k); for (unsigned i = 0; i < n; ++i) {hx[(size_t)k*n + i] = amp*rnd(); hy[(size_t)k*n + i] = rnd();}}
	float *dx, *dy, *out[NFORMS];
	CK(hipMalloc(&dx, hx.size()*4)); CK(hipMalloc(&dy, hy.size()*4));
	CK(hipMemcpy(dx, hx.data(), hx.size()*4, hipMemcpyHostToDevice)); CK(hipMemcpy(dy, hy.data(), hy.size()*4, hipMemcpyHostToDevice));
	J.xt = dx; J.yt = dy;
	std::vector<float> hsx(n), hsy(n), sums_a;
	if (stages) { // island terms, epilogue constants, the whole output grid and the min / max words
		for (unsigned i = 0; i < n; ++i) {hsx[i] = 0.5f*rnd(); hsy[i] = rnd();}
		float *dsx, *dsy, *full; unsigned *dmm;
		CK(hipMalloc(&dsx, (size_t)n*4)); CK(hipMalloc(&dsy, (size_t)n*4)); CK(hipMalloc(&full, (size_t)n*n*4)); CK(hipMalloc(&dmm, 8));
		CK(hipMemcpy(dsx, hsx.data(), (size_t)n*4, hipMemcpyHostToDevice)); CK(hipMemcpy(dsy, hsy.data(), (size_t)n*4, hipMemcpyHostToDevice)); CK(hipMemset(dmm, 0xFF, 8));
		J.smx = dsx; J.smy = dsy; J.out = full; J.mm = dmm;
		J.zme = 3.5f; J.z2 = 7.0f; J.inv = 1.0f/7.0f; J.off = 0.25f;
	}
	hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	int const nk = F_TABLE_SIZE - kstart;
	double const waves = (double)(n/128)*(n/128)*4.0, slots = waves/1024.0; // the same for both forms; 256 CUs x 4 SIMDs
	printf("sine_rowscalar_probe: %u^2 cells, terms %d .. 89 (%d) in chunks of %d, %.0f waves per launch, at least %.1f s back to back per line\n", n, kstart, nk, chunk_len(kstart, KC), waves, seconds);

	{	// ---- the forms against each other and against the chain, on the nc x nc corner of the same tables (row stride n)
		job_t C = J; C.n = nc;
		std::vector<float> h[NFORMS];
		for (int f = 0; f < NFORMS; ++f) {
			CK(hipMalloc(&out[f], (size_t)nc*nc*4)); CK(hipMemset(out[f], 0xFF, (size_t)nc*nc*4));
			C.out = out[f]; launch(f, true, C, nc, (f == FORM_A) ? 4u : 8u, 0); CK(hipDeviceSynchronize()); CK(hipGetLastError());
			h[f].resize((size_t)nc*nc); CK(hipMemcpy(h[f].data(), out[f], (size_t)nc*nc*4, hipMemcpyDeviceToHost));
		}
		unsigned long long diff_b = 0, diff_bt = 0, bad = 0, cnt = 0;
		for (size_t i = 0; i < (size_t)nc*nc; ++i) {diff_b += bits(h[FORM_A][i]) != bits(h[FORM_B][i]); diff_bt += bits(h[FORM_A][i]) != bits(h[FORM_BT][i]);}
		for (unsigned yi = 0; yi < 64; ++yi) {
			unsigned const y = (yi < 32) ? yi*33 % nc : (unsigned)(rng() % nc);
			for (unsigned x = 0; x < nc; ++x) {
				float z = 0.0f;
				for (int k = kstart; k < F_TABLE_SIZE; ++k) {volatile float const t = hx[(size_t)k*n + x]*hy[(size_t)k*n + y]; z = z + t;}
				++cnt; bad += bits(z) != bits(h[FORM_A][(size_t)y*nc + x]);
			}
		}
		printf("check %u^2: cells where B differs from A %llu, Bt from A %llu; A against the rounded-product chain in k order: %llu of %llu sampled cells differ\n", nc, diff_b, diff_bt, bad, cnt);
		for (int f = 0; f < NFORMS; ++f) {CK(hipFree(out[f]));}
		if (diff_b || diff_bt || bad) {printf("FAILED\n"); return 2;}
		sums_a = h[FORM_A];
	}
	if (stages) {
		if (check_eforms(J, nc, sums_a, hsx, hsy)) {printf("FAILED\n"); return 2;}
		unsigned const grid = (n/256)*(n/64);
		if (pmc) { // a counter pass: a few launches per form, told apart by their template arguments
			for (int f = 0; f < NEFORMS; ++f) {printf("pmc form %s %.4f ms per launch (20 launches)\n", eforms[f].name, time_eform(f, J, n, 0.0, e0, e1, nullptr, 2, 20));}
			return 0;
		}
#ifdef RS_STAMPS
		unsigned long long *ds; CK(hipMalloc(&ds, (size_t)grid*16)); J.stamps = ds;
		std::vector<unsigned long long> hs((size_t)grid*2);
#endif
		std::vector<double> t[NEFORMS];
		for (int rep = 0; rep < reps; ++rep) {
			for (int i = 0; i < NEFORMS; ++i) {
				int const f = (rep & 1) ? NEFORMS - 1 - i : i; // the order is reversed every other repetition
#ifdef RS_STAMPS
				CK(hipMemset(ds, 0, (size_t)grid*16));
#endif
				long cnt; double const ms = time_eform(f, J, n, seconds, e0, e1, &cnt);
				t[f].push_back(ms);
#ifdef RS_STAMPS
				CK(hipMemcpy(hs.data(), ds, (size_t)grid*16, hipMemcpyDeviceToHost));
				std::vector<double> mhz, cyc;
				for (unsigned b = 0; b < grid; ++b) {if (hs[2*b + 1]) {mhz.push_back((double)hs[2*b]/(double)hs[2*b + 1]*100.0); cyc.push_back((double)hs[2*b]);}}
				std::sort(mhz.begin(), mhz.end()); std::sort(cyc.begin(), cyc.end());
				if (mhz.empty()) {printf("no stamps\n"); return 3;}
				printf("stamps rep %d form %s %.4f ms per launch (stamped build)  in-kernel clock, median over %zu blocks: %.0f MHz (p10 %.0f, p90 %.0f)  shader ticks per block, loop to end, median %.0f\n",
				       rep, eforms[f].name, ms, mhz.size(), mhz[mhz.size()/2], mhz[mhz.size()/10], mhz[mhz.size()*9/10], cyc[cyc.size()/2]);
#else
				printf("rep %d form %s %.4f ms per launch (%ld launches)\n", rep, eforms[f].name, ms, cnt);
#endif
				fflush(stdout);
			}
		}
		double med[NEFORMS], spread[NEFORMS];
		for (int f = 0; f < NEFORMS; ++f) {std::vector<double> v = t[f]; std::sort(v.begin(), v.end()); med[f] = v[v.size()/2]; spread[f] = v.back() - v.front();}
		for (int f = 0; f < NEFORMS; ++f) {
			std::vector<double> v = t[f]; std::sort(v.begin(), v.end());
			printf("summary form %s n %zu min %.4f median %.4f max %.4f ms  spread %.1f us", eforms[f].name, v.size(), v.front(), med[f], v.back(), spread[f]*1e3);
			if (f > 0 && f <= EFORM_B3) {printf("  against the stage before %+.1f us\n", (med[f] - med[f - 1])*1e3);}
			else if (f > EFORM_B3) {printf("  against B3 %+.1f us (B3's spread %.1f us): gate %s\n", (med[f] - med[EFORM_B3])*1e3, spread[EFORM_B3]*1e3, (med[EFORM_B3] - med[f] > spread[EFORM_B3]) ? "passed" : "not passed");}
			else {printf("\n");}
		}
		return 0;
	}
#ifdef RS_STAMPS
	{	// ---- the in-kernel clock: stamps of the last launch after `seconds` of back-to-back launches
		unsigned const nb = (n/128)*(n/128), grid = (nb + 7)/8*8;
		unsigned long long *ds; CK(hipMalloc(&ds, (size_t)grid*16)); J.stamps = ds;
		std::vector<unsigned long long> hs((size_t)grid*2);
		for (int rep = 0; rep < reps; ++rep) {
			for (int f = 0; f < NFORMS; ++f) {
				CK(hipMemset(ds, 0, (size_t)grid*16));
				double const ms = time_form(f, J, n, (f == FORM_A) ? 4u : 8u, 0, seconds, e0, e1);
				CK(hipMemcpy(hs.data(), ds, (size_t)grid*16, hipMemcpyDeviceToHost));
				std::vector<double> mhz, cyc;
				for (unsigned b = 0; b < grid; ++b) {if (hs[2*b + 1]) {mhz.push_back((double)hs[2*b]/(double)hs[2*b + 1]*100.0); cyc.push_back((double)hs[2*b]);}}
				std::sort(mhz.begin(), mhz.end()); std::sort(cyc.begin(), cyc.end());
				if (mhz.empty()) {printf("no stamps\n"); return 3;}
				printf("stamps rep %d form %s %.4f ms per launch (stamped build)  in-kernel clock, median over %zu blocks: %.0f MHz (p10 %.0f, p90 %.0f)  shader ticks around the loop, median %.0f\n",
				       rep, form_name[f], ms, mhz.size(), mhz[mhz.size()/2], mhz[mhz.size()/10], mhz[mhz.size()*9/10], cyc[cyc.size()/2]);
			}
		}
		return 0;
	}
#endif
	// ---- alternating timed runs
	std::vector<double> t[NFORMS];
	for (int rep = 0; rep < reps; ++rep) {
		for (int i = 0; i < NFORMS; ++i) {
			int const f = (rep & 1) ? NFORMS - 1 - i : i; // the order is reversed every other repetition
			long cnt; double const ms = time_form(f, J, n, (f == FORM_A) ? 4u : 8u, 0, seconds, e0, e1, &cnt);
			t[f].push_back(ms);
			printf("rep %d form %s %.4f ms per launch (%ld launches)  %.3f ns per term and wave on its SIMD  %.1f Gcells/s\n", rep, form_name[f], ms, cnt, ms*1e6/nk/slots, (double)n*n/ms*1e-6);
			fflush(stdout);
		}
	}
	for (int f = 0; f < NFORMS; ++f) {
		std::vector<double> s = t[f]; std::sort(s.begin(), s.end());
		printf("summary form %s n %zu min %.4f median %.4f max %.4f ms  spread %.2f %%  median against A's %+.2f %%\n", form_name[f], s.size(), s.front(), s[s.size()/2], s.back(),
		       (s.back() - s.front())/s[s.size()/2]*100.0, (s[s.size()/2]/[&]() {std::vector<double> a = t[FORM_A]; std::sort(a.begin(), a.end()); return a[a.size()/2];}() - 1.0)*100.0);
	}
	if (sweeps) {
		// rowgroup: tile rows walked together (A: 128-row tiles, B: 64-row tiles)
		unsigned const rgs[] = {1, 2, 4, 8, 16, 64};
		for (int f = 0; f < NFORMS; ++f) {
			for (unsigned rg : rgs) {printf("sweep form %s rowgroup %3u: %.4f ms per launch\n", form_name[f], rg, time_form(f, J, n, rg, 0, seconds*0.5, e0, e1)); fflush(stdout);}
		}
		// blocks per CU: 29.7 KB of LDS and 80 VGPRs admit five blocks of form B (five waves per SIMD); dynamic LDS that nobody uses limits a CU (160 KB) to four blocks
		// (8 KB more each) or three (12 KB more each)
		for (int rep = 0; rep < 2; ++rep) {
			for (int f = FORM_B; f < NFORMS; ++f) {
				printf("sweep form %s blocks per CU: up to five %.4f ms", form_name[f], time_form(f, J, n, 8u, 0, seconds*0.5, e0, e1));
				printf("   four (8 KB of unused LDS) %.4f ms", time_form(f, J, n, 8u, 8192u, seconds*0.5, e0, e1));
				printf("   three (12 KB of unused LDS) %.4f ms per launch\n", time_form(f, J, n, 8u, 12288u, seconds*0.5, e0, e1)); fflush(stdout);
			}
		}
	}
	return 0;
}
