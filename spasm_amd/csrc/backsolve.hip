// Back-substituted factor image and the Schur complement computed from it.
//
// The reference reduces every non-pivotal row a of A by a sparse triangular solve against U
// (spasm_schur.c:86-171 -> spasm_triangular.c:109-146): x = a U_pp^-1, then s = a_n - x U_pn.  The
// same product can be bracketed the other way round:
//
//       S = A_n - A_p (U_pp^-1 U_pn) = A_n - A_p R,
//
// where row c of R is the non-pivotal part of the fully reduced pivot row c (the rows spasm_rref would
// produce, spasm_rref.c:25).  R is dense, r x Sm (Sm = number of non-pivotal columns).  When Sm is small
// -- a Schur complement that is going to be dense anyway -- building R costs nnz(U') * Sm multiply-adds,
// streaming and free of atomics, and every reduced row is then a combination of the few rows of R its
// pivotal entries select.  mk13.b5: 130183 x 4952 (1.3 GB in 16-bit entries) against 3.97e9 (row, pivot) eliminations.
// Arithmetic mod p is exact, so the result is the same matrix, bit for bit.
//
// R[c] = U_n[c] - sum_{t pivotal in U'[c]} u_ct R[t], and t always lies in a later elimination level
// than c.  The columns of R are independent: one workgroup owns a slab of 32 or 64 columns and walks the
// rows from the last level to the first, with no communication between workgroups at all.  Inside a
// workgroup the chain of levels runs in LDS: rows are cut into chunks of <= RING consecutive rows;
//   phase A: every row of the chunk gathers what it needs from outside the chunk (rows of R that are
//            final, in HBM) into an LDS ring; the plan hands those rows over as ready offsets (no multiply per
//            access), the head of a row -- two offsets, two coefficients -- is read from LDS once, and a row starts
//            at zero in registers: the few entries of U_n are added to the ring afterwards, by the threads that hold them,
//   phase B: level by level, rows pick up their dependencies inside the chunk from the ring -- every WAVE
//            on its own columns of every row, so that the levels need no barrier,
//   phase C: the ring is written back to R.
// The rows of S then come from bs_apply_*: one wave per row, a few rows of R each.
#include <algorithm>
#include <cinttypes>
#include <type_traits>
#include <thread>
#include <vector>

#include "device_types.h"
#include "field_dev.h"
#include "sgn_dev.h"

namespace sh {

int usable_cpus();          // host_pivots.cpp

namespace {

constexpr int BS_RING = 768;       // rows per chunk (the LDS ring holds RING rows of one slab)
constexpr int BS_NEARCAP = 1024;   // dependencies inside a chunk that do not fit the pass table (rows with more than two)
constexpr int BS_PASSCAP = 80;     // phase-B passes of a chunk (32 rows of one level each)
constexpr int BS_PASSROWS = 32;
// an empty slot of the pass table points at a spare row of the ring (row BS_RING, i.e. word offset RING * RSTR: bs_pass_empty)
// with coefficient 0: the signed kernels run every lane through the same reads, multiply-adds and write, without a branch
constexpr uint32_t BS_NONE = 0xFFFFFFFFu;
constexpr int BS_XCDS = 8;         // XCDs of an MI355X in its default partition (backsolve_kernel: which slabs share an L2; any value gives the same R)

template <typename T> T *dalloc(int64_t count)
{
	return static_cast<T *>(sh::big_alloc((size_t) (count > 0 ? count : 1) * sizeof(T)));
}

template <typename T> void upload(T *dst, const std::vector<T> &src, hipStream_t s)
{
	if (!src.empty())
		sh::h2d(dst, src.data(), src.size() * sizeof(T), s);
}

struct BsArgs {
	void *R;                      // r x ldR elements of T (uint16_t when p < 2^16, else uint32_t)
	int64_t ldR;
	int nchunks;
	const BsChunk *chunk;
	const int *chunk_extra;       // per chunk: 1 when some row has more than two dependencies outside the chunk
	const uint4 *ptab;
	const uint2 *near;
	const uint4 *far_head;
	const uint64_t *far_rp;
	const uint2 *far;
	const uint64_t *np_rp;
	const uint2 *np;
	const int *np_row;            // compact row of every entry of np
	int plain;                    // coefficients (y) are plain residues (p < 2^16), not Montgomery form
	int sparse_init;              // 1: the kernel scatters U_n itself (few entries); 0: R was pre-filled by bs_init_kernel
	int r;
	int Sm;                       // columns of R
	unsigned long long *prof;    // SPASM_HIP_BS_PROFILE=1: 8 counters, shader-clock cycles of workgroup 0 per stage of a chunk, summed over the chunks
	int sgn;                      // signed 16-bit entries (the SGN kernels); coefficients are negated balanced residues
	MontDev F;
	SgnDev G;
};

// ---- storage of R ---------------------------------------------------------------------------------
// A lane always moves 32-bit WORDS.  PACKED = false: a word is one entry of R (any odd p < 2^32).  PACKED = true
// (p < 2^16; 42013, the reference's default, qualifies): a word holds two consecutive 16-bit entries -- half the
// traffic, half the LDS, the same number of memory instructions.
template <bool PACKED> struct Word {
	static constexpr int CPL = PACKED ? 2 : 1;            // columns per lane
	using Elem = typename std::conditional<PACKED, uint16_t, uint32_t>::type;
};

// x - v * y, component-wise.  Coefficients y are in Montgomery form (value * 2^32 mod p) for p >= 2^16; for p < 2^16
// (PLAIN) they are the plain residues: v * y < 2^32 is one full-rate 24-bit multiply and a Barrett reduction (one
// quarter-rate multiply instead of the four of a Montgomery product), bm = floor(2^32 / p).
template <bool PACKED, bool PLAIN> __device__ __forceinline__ uint32_t w_submul(uint32_t x, uint32_t v, uint32_t y, const MontDev &F, uint32_t bm)
{
	auto small = [&](uint32_t xe, uint32_t ve) -> uint32_t {
		const uint32_t t = __umul24(ve, y);                  // ve, y < p < 2^16
		const uint32_t q = __umulhi(t, bm);                   // floor(t / p) - 2 <= q <= floor(t / p); q < p
		uint32_t rem = t - __umul24(q, F.p);
		rem = (rem >= F.p) ? rem - F.p : rem;
		rem = (rem >= F.p) ? rem - F.p : rem;
		return (xe >= rem) ? xe - rem : xe + F.p - rem;
	};
	if constexpr (PACKED) {
		static_assert(PLAIN, "packed entries only exist for p < 2^16");
		return small(x & 0xFFFFu, v & 0xFFFFu) | (small(x >> 16, v >> 16) << 16);
	} else if constexpr (PLAIN) {
		return small(x, v);
	} else {
		return submod(x, montmul(v, y, F), F);
	}
}

// R <- U_n (values out of Montgomery form); R was zeroed before.  Only for factors whose rows hold many non-pivotal
// entries: otherwise the backsolve kernel scatters them itself and R is never pre-filled.
template <typename T> __global__ __launch_bounds__(256) void bs_init_kernel(BsArgs b)          // (b.plain: entries hold plain residues)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= b.r)
		return;
	T *row = static_cast<T *>(b.R) + (int64_t) c * b.ldR;
	for (uint64_t e = b.np_rp[c]; e < b.np_rp[c + 1]; e++) {
		const uint2 en = b.np[e];
		row[en.x] = b.sgn ? (T) (uint16_t) (int16_t) sgn_from_residue(en.y, b.G) : (T) (b.plain ? en.y : montmul(en.y, 1u, b.F));
	}
}

// A fixed number of values that must stay in REGISTERS across a long stretch of code.  A local array would do in
// principle, but an array of more than 16 dwords is not turned into registers by the compiler (it becomes scratch memory,
// i.e. global memory behind the cache: measured on the metadata of backsolve_kernel, whose 20-dword table part went
// through scratch_store / scratch_load and cost two memory round trips per chunk); members of a struct, reached with
// compile-time indices, always are.
template <typename T, int N> struct RegFile {
	T head;
	RegFile<T, N - 1> tail;
	template <int I> __device__ __forceinline__ T &at()
	{
		if constexpr (I == 0)
			return head;
		else
			return tail.template at<I - 1>();
	}
};
template <typename T> struct RegFile<T, 0> {
};

template <int I, int N, typename Fn> __device__ __forceinline__ void bs_static_for(Fn &&f)
{
	if constexpr (I < N) {
		f(std::integral_constant<int, I>{});
		bs_static_for<I + 1, N>(f);
	}
}

// ---- the head of a row: its first two dependencies outside its chunk --------------------------------
// Rows are OFFSETS (row * ldw / 256, see backsolve_kernel), BS_NONE = no such dependency (its coefficient is 0).
//   p < 2^16 (PLAIN): {offset 0, offset 1, coefficient 0 | coefficient 1 << 16, -}: both coefficients fit 16 bits (the signed
//                     kernels' v_mad_i32_i16 takes either half of a register as it is), so ONE register per row in flight
//                     carries them from the read of the head (before the loads are issued) to the arithmetic (after they landed);
//   otherwise:        {offset 0, coefficient 0, offset 1, coefficient 1}, coefficients in Montgomery form.
// A dependency is present iff its coefficient is not 0 (entries of U are not).
template <bool PLAIN> __host__ __device__ __forceinline__ uint4 bs_head(uint32_t off0, uint32_t c0, uint32_t off1, uint32_t c1)
{
	if constexpr (PLAIN)
		return uint4{off0, off1, (c0 & 0xFFFFu) | (c1 << 16), 0u};
	else
		return uint4{off0, c0, off1, c1};
}

// lo (hi) = low (high) half of w * the low (HI = 0) or high (HI = 1) half of c2, added to lo (hi) unless FIRST
template <int HI, bool FIRST> __device__ __forceinline__ void sgn_mad_half(uint32_t w, uint32_t c2, int &lo, int &hi)
{
	if constexpr (FIRST) {
		static_assert(HI == 0, "the first term takes the low coefficient");
		asm("v_mad_i32_i16 %0, %1, %2, 0" : "=v"(lo) : "v"(w), "v"(c2));
		asm("v_mad_i32_i16 %0, %1, %2, 0 op_sel:[1,0,0,0]" : "=v"(hi) : "v"(w), "v"(c2));
	} else if constexpr (HI == 0) {
		asm("v_mad_i32_i16 %0, %1, %2, %0" : "+v"(lo) : "v"(w), "v"(c2));
		asm("v_mad_i32_i16 %0, %1, %2, %0 op_sel:[1,0,0,0]" : "+v"(hi) : "v"(w), "v"(c2));
	} else {
		asm("v_mad_i32_i16 %0, %1, %2, %0 op_sel:[0,1,0,0]" : "+v"(lo) : "v"(w), "v"(c2));
		asm("v_mad_i32_i16 %0, %1, %2, %0 op_sel:[1,1,0,0]" : "+v"(hi) : "v"(w), "v"(c2));
	}
}

// ---- the table of phase-B passes: one 16-byte entry per row slot of a pass ------------------------------
// Rows of the ring are OFFSETS in words, slot * RSTR (RSTR = BsGeom::RSTR of the kernel the plan was cut for; (RING + 1) * RSTR
// fits 16 bits for every shape, backsolve_plan checks it): an LDS address is one v_mad_u32_u16 that picks its half of the word.
//   ordinary row (one or two dependencies inside the chunk):
//     .x = own offset, .y = offset of dependency 0 | offset of dependency 1 << 16 (one dependency: the same row again),
//     p < 2^16 (PLAIN): .z = coefficient 0 | coefficient 1 << 16 (as bs_head: v_mad_i32_i16 takes either half), .w = 0;
//     otherwise:        .z = coefficient 0, .w = coefficient 1 (Montgomery form);
//   long row (more than two): .x = own offset | number of dependencies << 16, .y = offset of dependency 0, .z = coefficient 0,
//     .w = where the others start in the chunk's list (`near`: {offset, coefficient}).
// Long rows sit in passes of their own, after the ordinary passes of their level (the order inside a level is free).  The
// kernel never looks for them: the chunk descriptor says how many ordinary passes come before the first long pass, and the
// high half of .y of EVERY slot of a long pass how many ordinary passes follow it before the next one.
// An empty slot is the spare row with coefficient 0.
__host__ __device__ __forceinline__ uint4 bs_pass_empty(uint32_t spare_off)
{
	return uint4{spare_off, spare_off | (spare_off << 16), 0u, 0u};
}

// byte address in LDS of the word `base` (a byte address) + 4 * the low (HI = 0) or high (HI = 1) half of `packed`
template <int HI> __device__ __forceinline__ uint32_t bs_ring_at(uint32_t packed, uint32_t base)
{
	uint32_t a;
	if constexpr (HI == 0)
		asm("v_mad_u32_u16 %0, %1, 4, %2" : "=v"(a) : "v"(packed), "v"(base));
	else
		asm("v_mad_u32_u16 %0, %1, 4, %2 op_sel:[1,0,0,0]" : "=v"(a) : "v"(packed), "v"(base));
	return a;
}
using bs_lds_word = __attribute__((address_space(3))) uint32_t;

// WPL consecutive words of a row of R, as a lane moves them in phases A and C: one access of WPL * 4 bytes (WPL = 4: 16-byte
// aligned, the caller sees to it).  `present` false: nothing is read, the words are 0.
template <int WPL> __device__ __forceinline__ void bs_load_words(bool present, const uint32_t *at, uint32_t (&w)[WPL])
{
	static_assert(WPL == 1 || WPL == 4, "a lane moves one word or four");
	if constexpr (WPL == 4) {
		const uint4 t = present ? *reinterpret_cast<const uint4 *>(at) : uint4{0u, 0u, 0u, 0u};
		w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
	} else {
		w[0] = present ? *at : 0u;
	}
}
template <int WPL> __device__ __forceinline__ void bs_store_words(uint32_t *at, const uint32_t (&w)[WPL])
{
	if constexpr (WPL == 4)
		*reinterpret_cast<uint4 *>(at) = uint4{w[0], w[1], w[2], w[3]};
	else
		*at = w[0];
}

// the largest number of rows <= `rows` for which `nw` waves of that many rows divide `ring`
constexpr int bs_rows_dividing(int rows, int nw, int ring)
{
	return (rows <= 1 || ring % (rows * nw) == 0) ? rows : bs_rows_dividing(rows - 1, nw, ring);
}

// LPR words per row of a slab: a row of a slab is LPR * 4 bytes (128 B with LPR = 32: whole cache lines, half
// as many requests as 64-byte segments -- the kernel is bound by the rate of such requests).
// NW waves per workgroup.  In phases A and C a lane holds WPL consecutive words of a row, a row is QPR = LPR / WPL lanes and a
// wave instruction covers RS rows.  WPL = 4 where every wave has one word of a row in phase B and the row is whole quads
// (slabs of 12 and 8 words): whatever is done per row and not per word -- the head, its selects, the addresses, the guard --
// is then paid once per four words, and memory is reached 16 bytes at a time.  Elsewhere a lane holds one word.
// RING / PASSROWS / PASSCAP: rows per chunk, rows per phase-B pass, passes per chunk -- the plan (backsolve_plan) is built
// for the values of the kernel that will run it, and for its RSTR (BsImage::ring, passrows, passcap, rstr).
template <bool PACKED, int LPR, int NW, int RING = BS_RING, int PASSROWS = BS_PASSROWS, int PASSCAP = BS_PASSCAP> struct BsGeom {
	static constexpr int RING_ = RING, PASSROWS_ = PASSROWS, PASSCAP_ = PASSCAP;
	static constexpr int THREADS = 64 * NW;
	static constexpr int WPL = (NW == LPR && LPR % 4 == 0) ? 4 : 1;
	static constexpr int QPR = LPR / WPL;
	// rows per wave instruction: as many as the wave has lanes for; WPL = 4: the largest such number for which an iteration
	// of the workgroup divides the chunk (12 words: 20 rows on 60 lanes, 240 per iteration, 5 iterations; 8 words: 32, 256, 3)
	static constexpr int RS = (WPL == 1) ? 64 / QPR : bs_rows_dividing(64 / QPR, NW, RING);
	static constexpr int RS1 = 64 / LPR;                   // the same with one word per lane (the long lists of outside dependencies)
	static constexpr int CW = LPR * Word<PACKED>::CPL;     // columns per slab
	static constexpr int ROWS_PER_ITER = RS * NW;
	static constexpr int ITERS = RING / ROWS_PER_ITER;
	// rows in flight per lane in phase A.  Eight waves (two per SIMD: 256 registers each) take a whole chunk in ONE pass --
	// a pass is a round trip to memory, and a chunk has little else to hide it behind
	static constexpr int UNR = (NW >= 8 && ITERS <= 24) ? ITERS : (ITERS % 12 == 0) ? 12 : 8;
	static constexpr int LANES_USED = RS * QPR;            // (the lanes beyond RS whole rows idle in phases A and C)
	static_assert(LPR % WPL == 0 && LANES_USED <= 64, "a row is whole lanes, a wave instruction whole rows");
	static_assert(RING % ROWS_PER_ITER == 0 && ITERS % UNR == 0, "phase A is unrolled in passes of UNR rows");
	static constexpr int N_NEAR = (BS_NEARCAP + THREADS - 1) / THREADS;      // metadata words a thread carries for the next chunk
	static constexpr int N_ROW = (RING + THREADS - 1) / THREADS;
	static constexpr int N_PTAB = (PASSCAP * PASSROWS + THREADS - 1) / THREADS;
	static constexpr size_t FH_BYTES = (size_t) RING * sizeof(uint4);
	static constexpr size_t PTAB_BYTES = (size_t) PASSCAP * PASSROWS * sizeof(uint4);
	static constexpr int RSTR = LPR + 1;                    // row stride of the ring in words: odd, so that a wave instruction over
	                                                        // consecutive rows AND one over consecutive words both spread over the banks
	static constexpr size_t LDS_BYTES = FH_BYTES + PTAB_BYTES + (size_t) BS_NEARCAP * sizeof(uint2) + (size_t) (RING + 1) * RSTR * 4;          // (+ the spare row)
};

template <bool PACKED, bool PLAIN, int LPR, int NW, bool SGN = false, int RING = BS_RING, int PASSROWS = BS_PASSROWS, int PASSCAP = BS_PASSCAP, int WGS_PER_CU = 1>
__global__ __launch_bounds__(64 * NW, WGS_PER_CU) void backsolve_kernel(BsArgs b)
{
	static_assert(!SGN || (PACKED && PLAIN), "signed entries are packed 16-bit entries");
	// For speed only (any one-to-one assignment of slabs to workgroups computes the same R: a workgroup reads nothing but what it
	// wrote itself).  Every XCD has an L2 of its own, and workgroups have been observed to go to the XCDs in turn (workgroup i
	// to XCD i mod 8; the hardware does not promise it).  A slab row is a fraction of a 128-byte line: with slab = workgroup,
	// the slabs that share a line sit on different XCDs, each L2 pulls the line in for phase A and writes its part of it back
	// after phase C.  So workgroups i, i + 8, i + 16, ... take a RUN of neighbouring slabs: on such a chip a line of R is read
	// into, and written from, one L2 (but for the lines where two runs meet).  The grid is BS_XCDS whole runs.
	const int nslabs = (b.Sm + LPR * Word<PACKED>::CPL - 1) / (LPR * Word<PACKED>::CPL);
	const int slab = (int) (blockIdx.x % BS_XCDS) * (int) (gridDim.x / BS_XCDS) + (int) (blockIdx.x / BS_XCDS);
	if (slab >= nslabs)
		return;
	const uint32_t bm = PLAIN ? (uint32_t) (0x100000000ull / b.F.p) : 0u;
	const SgnDev G = b.G;
	using Geo = BsGeom<PACKED, LPR, NW, RING, PASSROWS, PASSCAP>;
	using Elem = typename Word<PACKED>::Elem;
	extern __shared__ __attribute__((aligned(16))) unsigned char bs_lds[];
	uint4 *fh = reinterpret_cast<uint4 *>(bs_lds);                          // first two outside dependencies of every row
	uint4 *ptab = reinterpret_cast<uint4 *>(bs_lds + Geo::FH_BYTES);       // phase-B passes
	uint2 *near = reinterpret_cast<uint2 *>(bs_lds + Geo::FH_BYTES + Geo::PTAB_BYTES);
	uint32_t *ring = reinterpret_cast<uint32_t *>(near + BS_NEARCAP);
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	// workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains the vector-memory counter,
	// i.e. the metadata of the NEXT chunk that was asked for at the top of this one: the first barrier of every chunk then
	// costs a round trip to memory (170 chunks x ~1 us on mk13.b5).  Between the phases only the ring (LDS) is handed
	// from wave to wave; the one place where global stores must be visible to other waves (after phase C) keeps
	// __syncthreads().
	auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
	constexpr int WPL = Geo::WPL;
	const int rs = lane / Geo::QPR, wl = lane % Geo::QPR * WPL;          // row slot of the lane, its first word inside the row (phases A and C)
	constexpr int RSTR = Geo::RSTR;                        // words between two rows of the ring
	constexpr uint32_t SPARE = (uint32_t) (RING * RSTR);   // the spare row (row RING), where the empty slots of the pass table point
	// phase B splits the COLUMNS among the waves: a wave owns WPW words of every row, a wave instruction covers RSB rows
	constexpr int WPW = LPR / NW, RSB = 64 / WPW;
	static_assert(WPW >= 1 && LPR % NW == 0 && 64 % WPW == 0, "every wave takes the same number of words of a row through phase B");
	static_assert(PASSROWS % RSB == 0, "a pass is a whole number of wave instructions");
	const MontDev F = b.F;
	const int64_t ldw = b.ldR / Word<PACKED>::CPL;       // row stride of R in words
	uint32_t *Rs = static_cast<uint32_t *>(b.R) + (int64_t) slab * LPR + wl;
	// a row of R starts at row * ldw words; ldw is a multiple of 256 (rows are padded to 512 columns), and row * (ldw / 256)
	// fits 32 bits for any R below 4 TB.  The plan hands every dependency over as that product (its OFFSET, in units of 256
	// words): an address is a shift and an add.  The chunk's own rows are the offset of its first row (one scalar multiply
	// per chunk) plus the lane's own (one multiply per kernel) plus a uniform step per iteration
	const uint32_t ldw256 = (uint32_t) (ldw >> 8);
	auto at_off = [&](uint32_t off) -> uint32_t * { return Rs + ((uint64_t) off << 8); };
	const int slot0 = wave * Geo::RS + rs;          // this lane's row slot within an iteration
	const uint32_t slot0_off = (uint32_t) slot0 * ldw256;
	const uint32_t iter_off = (uint32_t) Geo::ROWS_PER_ITER * ldw256;          // (uniform)
	// lanes that hold words of a row in phases A and C: all of them when the rows of a wave instruction fill it; and the words
	// must exist (the last slab of a row may reach beyond the padded row when LPR does not divide its length; the length and
	// the start of a slab are multiples of WPL, so the lane's words are all inside or all outside)
	static_assert(WPL == 1 || (LPR % WPL == 0 && 256 % WPL == 0), "WPL words at a multiple of WPL: one aligned access, inside the padded row or outside it");
	const bool lane_ok = lane < Geo::LANES_USED && (int64_t) slab * LPR + wl < ldw;
	const int col_lo = slab * Geo::CW;        // columns [col_lo, col_lo + CW) belong to this workgroup

	// metadata of a chunk (the same for every slab: served by the L2) travels through registers: the loads for chunk
	// k + 1 are issued when chunk k starts and land in LDS when it is done
	RegFile<uint2, Geo::N_NEAR> m_near;
	RegFile<uint4, Geo::N_ROW> m_fh;
	RegFile<uint4, Geo::N_PTAB> m_ptab;
	auto load_meta = [&](const BsChunk &c) {
		bs_static_for<0, Geo::N_NEAR>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			const int t = tid + q * Geo::THREADS;
			// (the load is unconditional, from a valid address, and the VALUE is selected: `cond ? *p : constant` makes the
			//  compiler select between p and the address of the constant, which then has to live in scratch memory, and turns
			//  the load into a FLAT one)
			const uint2 v = b.near[(t < c.nnear) ? c.near0 + t : 0];
			m_near.template at<q>() = (t < c.nnear) ? v : uint2{0u, 0u};
		});
		bs_static_for<0, Geo::N_ROW>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			const int t = tid + q * Geo::THREADS;
			const uint4 v = b.far_head[(t < c.hi - c.lo) ? c.lo + t : 0];
			m_fh.template at<q>() = (t < c.hi - c.lo) ? v : bs_head<PLAIN>(BS_NONE, 0u, BS_NONE, 0u);
		});
		// (the addresses of these loads are formed here, chunk by chunk, from a thread id the compiler cannot see through: formed
		//  once before the loop of the chunks they are 64-bit values kept through phase A, which has no registers to spare)
		int tid_m = tid;
		asm volatile("" : "+v"(tid_m));
		bs_static_for<0, Geo::N_PTAB>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			const int t = tid_m + q * Geo::THREADS;
			const uint4 v = b.ptab[(t < c.npass * PASSROWS) ? (int64_t) c.pass0 * PASSROWS + t : 0];
			m_ptab.template at<q>() = (t < c.npass * PASSROWS) ? v : bs_pass_empty(SPARE);
		});
	};
	auto store_meta = [&]() {
		bs_static_for<0, Geo::N_NEAR>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			if (tid + q * Geo::THREADS < BS_NEARCAP)
				near[tid + q * Geo::THREADS] = m_near.template at<q>();
		});
		bs_static_for<0, Geo::N_ROW>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			if (tid + q * Geo::THREADS < RING)
				fh[tid + q * Geo::THREADS] = m_fh.template at<q>();
		});
		bs_static_for<0, Geo::N_PTAB>([&](auto qq) {
			constexpr int q = decltype(qq)::value;
			if (tid + q * Geo::THREADS < PASSCAP * PASSROWS)
				ptab[tid + q * Geo::THREADS] = m_ptab.template at<q>();
		});
	};
	// chunk descriptors travel one chunk ahead too: the descriptor of chunk k + 1 is in registers when chunk k starts, so
	// that the loads of its metadata (whose addresses it holds) can be issued at once instead of after a round trip
	// (read with VECTOR loads -- every lane the same 32 bytes: a scalar load shares its counter with the LDS, and the first
	//  LDS access after it would wait for the round trip)
	static_assert(sizeof(BsChunk) == 32, "a chunk descriptor is two 16-byte loads");
	int vzero;
	asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));          // (a zero the compiler cannot see through: keeps the address in a VGPR)
	uint4 raw_a = uint4{0u, 0u, 0u, 0u}, raw_b = uint4{0u, 0u, 0u, 0u};
	auto fetch_chunk = [&](int k) {
		const uint4 *src = reinterpret_cast<const uint4 *>(b.chunk + k) + vzero;
		raw_a = src[0];
		raw_b = src[1];
	};
	auto fetched_chunk = [&]() {
		BsChunk c;
		c.lo = __builtin_amdgcn_readfirstlane((int) raw_a.x);
		c.hi = __builtin_amdgcn_readfirstlane((int) raw_a.y);
		c.pass0 = __builtin_amdgcn_readfirstlane((int) raw_a.z);
		c.npass = (unsigned short) __builtin_amdgcn_readfirstlane((int) (raw_a.w & 0xFFFFu));
		c.nord = (unsigned short) __builtin_amdgcn_readfirstlane((int) (raw_a.w >> 16));
		c.near0 = __builtin_amdgcn_readfirstlane((int) raw_b.x);
		c.nnear = __builtin_amdgcn_readfirstlane((int) raw_b.y);
		c.np0 = __builtin_amdgcn_readfirstlane((int) raw_b.z);
		c.npn = __builtin_amdgcn_readfirstlane((int) raw_b.w);
		return c;
	};
	BsChunk ch_next{};
	if (b.nchunks > 0) {
		fetch_chunk(0);
		ch_next = fetched_chunk();
		load_meta(ch_next);
		store_meta();
	}
	if (b.nchunks > 1)
		fetch_chunk(1);
	__syncthreads();

	// stage timer (SPASM_HIP_BS_PROFILE): thread 0 of workgroup 0 reads the shader clock at every stage boundary
	unsigned long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	unsigned long long t_last = 0;
	const bool profiling = b.prof != nullptr && slab == 0 && tid == 0;
	auto tick = [&](int q) {
		if (profiling) {
			const unsigned long long now = __builtin_readcyclecounter();
			pt[q] += now - t_last;
			t_last = now;
		}
	};
	if (profiling)
		t_last = __builtin_readcyclecounter();
	for (int k = 0; k < b.nchunks; k++) {
		const BsChunk ch = ch_next;
		const int nrows = ch.hi - ch.lo;
		// the first THREADS non-pivotal entries of the chunk (mk13.b5: 61 per chunk), one per thread: asked for now, added to the
		// rows after phase A; the rest -- if any -- is read then
		uint2 c_np = uint2{0u, 0u};
		int c_np_row = 0;
		if (b.sparse_init) {
			const int cnt = ch.npn & 0x7FFFFFFF;
			c_np = b.np[(tid < cnt) ? ch.np0 + tid : 0];
			c_np_row = b.np_row[(tid < cnt) ? ch.np0 + tid : 0];
		}
		if (k + 1 < b.nchunks) {
			ch_next = fetched_chunk();
			load_meta(ch_next);
		}
		if (k + 2 < b.nchunks)
			fetch_chunk(k + 2);
		tick(0);          // descriptor + issue of the next chunk's metadata

		// ---- phase A: own row + dependencies outside the chunk, up to 3 * UNR loads (of WPL words) in flight per lane ----
		// SPARSE (sparse_init): the rows start at zero IN REGISTERS -- R is not read for them, the ring is neither zeroed nor read --
		// and the few entries of U_n are added to the ring afterwards.  Otherwise a row starts as what bs_init_kernel put into R.
		const uint32_t lo_off = (uint32_t) ch.lo * ldw256;          // (uniform: a scalar multiply)
		auto phase_a = [&](auto sparse_tag) {
			constexpr bool SPARSE = decltype(sparse_tag)::value;
			for (int pass = 0; pass < Geo::ITERS / Geo::UNR; pass++) {
				if (pass * Geo::UNR * Geo::ROWS_PER_ITER >= nrows)
					break;
				// SPARSE: the coefficients of the head are read with its addresses and kept until the loads have landed (the head is read
				// once).  The pre-filled path has the row's own word in flight as well: no registers for them, it reads them again;
				// so do 32-bit coefficients in the workgroups of sixteen waves.
				constexpr bool KEEP = SPARSE && (PLAIN || NW < 16);          // (sixteen waves have 128 registers each)
				uint32_t acc[SPARSE ? 1 : Geo::UNR][WPL], v0[Geo::UNR][WPL], v1[Geo::UNR][WPL], c0[KEEP ? Geo::UNR : 1], c1[(KEEP && !PLAIN) ? Geo::UNR : 1];
				// offset of the lane's own row, stepped from iteration to iteration (hidden from the compiler's algebra, which
				// would turn the sum back into (first row + slot) * stride: a quarter-rate multiply per access)
				uint32_t own_off = lo_off + (uint32_t) (pass * Geo::UNR) * iter_off + slot0_off;
				asm volatile("" : "+v"(own_off));
#pragma unroll
				for (int u = 0; u < Geo::UNR; u++) {
					const int s = (pass * Geo::UNR + u) * Geo::ROWS_PER_ITER + slot0;
					const bool ok = s < nrows && lane_ok;
					const uint4 h = fh[ok ? s : 0];
					const uint32_t a0 = h.x, a1 = PLAIN ? h.y : h.z;
					if constexpr (KEEP) {
						c0[u] = PLAIN ? h.z : h.y;
						if constexpr (!PLAIN)
							c1[u] = h.w;
					}
					if constexpr (!SPARSE) {
						bs_load_words<WPL>(ok, at_off(own_off), acc[u]);
						own_off += iter_off;
					}
					if constexpr (LPR <= 16 && 64 % LPR == 0) {
						// no branch around the loads: an absent dependency reads the chunk's own first row -- a valid address -- and
						// is multiplied by the coefficient 0 of its slot, or skipped, below (64-byte rows: 2.84 -> 2.75 ms on mk13.b5,
						// 9.2 -> 6.1 ms with 32-bit entries; with 128-byte rows the wasted lines cost more than the branches)
						bs_load_words<WPL>(true, at_off((ok && a0 != BS_NONE) ? a0 : lo_off), v0[u]);
						bs_load_words<WPL>(true, at_off((ok && a1 != BS_NONE) ? a1 : lo_off), v1[u]);
					} else {
						bs_load_words<WPL>(ok && a0 != BS_NONE, at_off(a0), v0[u]);
						bs_load_words<WPL>(ok && a1 != BS_NONE, at_off(a1), v1[u]);
					}
				}
#pragma unroll
				for (int u = 0; u < Geo::UNR; u++) {
					const int s = (pass * Geo::UNR + u) * Geo::ROWS_PER_ITER + slot0;          // (< RING: a head that exists, whatever it holds)
					uint32_t k0, k1;          // coefficients: both in k0 when PLAIN
					if constexpr (KEEP) {
						k0 = c0[u];
						k1 = PLAIN ? 0u : c1[u];
					} else if constexpr (PLAIN) {
						k0 = fh[s].z;
						k1 = 0u;
					} else {
						const uint4 h = fh[s];
						k0 = h.y;
						k1 = h.w;
					}
					uint32_t x[WPL];
#pragma unroll
					for (int j = 0; j < WPL; j++) {
						x[j] = SPARSE ? 0u : acc[u][j];
						if constexpr (SGN) {
							// no flags: an absent dependency has the coefficient 0 (and was loaded as 0, or as a row that exists), and a row
							// without dependencies comes out of the reduction as it went in (|x| <= p/2: the nearest multiple of p is 0)
							int lo, hi;
							if constexpr (SPARSE) {
								sgn_mad_half<0, true>(v0[u][j], k0, lo, hi);
							} else {
								sgn_unpack(x[j], lo, hi);
								sgn_mad_half<0, false>(v0[u][j], k0, lo, hi);
							}
							sgn_mad_half<1, false>(v1[u][j], k0, lo, hi);
							x[j] = sgn_pack(sgn_reduce(lo, G), sgn_reduce(hi, G));
						} else {
							// (no kernel without signed entries has WPL = 4 today: this form is compiled with one word per lane only)
							const uint32_t q0 = PLAIN ? (k0 & 0xFFFFu) : k0, q1 = PLAIN ? (k0 >> 16) : k1;
							if (q0 != 0u)
								x[j] = w_submul<PACKED, PLAIN>(x[j], v0[u][j], q0, F, bm);
							if (q1 != 0u)
								x[j] = w_submul<PACKED, PLAIN>(x[j], v1[u][j], q1, F, bm);
						}
					}
					// (the ring's rows are an odd number of words apart: WPL = 4 goes in as two pairs of words, not as 16 aligned bytes)
					if (s < nrows && lane_ok) {
#pragma unroll
						for (int j = 0; j < WPL; j++)
							ring[s * RSTR + wl + j] = x[j];
					}
				}
			}
		};
		if (b.sparse_init)
			phase_a(std::true_type{});
		else
			phase_a(std::false_type{});
		lds_barrier();
		tick(1);          // phase A
		if (b.sparse_init) {
			// the entries of U_n, from the list, each added to its element of the ring by the thread that holds it (distinct rows and
			// columns are distinct elements: no two threads meet).  The sum is brought back into the range of an entry.
			const int np_count = ch.npn & 0x7FFFFFFF;
			auto put = [&](const uint2 en, int row) {
				const int cc = (int) en.x - col_lo;
				if (cc >= 0 && cc < Geo::CW) {
					Elem *at = reinterpret_cast<Elem *>(ring) + (row - ch.lo) * (RSTR * Word<PACKED>::CPL) + cc;
					if constexpr (SGN) {
						// |entry| <= p/2 + p/64 + 1, |U_n| <= p/2: one step brings the sum into [-p/2, p/2]
						*at = (Elem) (uint16_t) (int16_t) sgn_canonical((int) (int16_t) *at + sgn_from_residue(en.y, G), G);
					} else {
						const uint32_t v = PLAIN ? en.y : montmul(en.y, 1u, F);
						uint32_t sum = (uint32_t) *at + v;
						if (sum < v || sum >= F.p)
							sum -= F.p;
						*at = (Elem) sum;
					}
				}
			};
			if (tid < np_count)
				put(c_np, c_np_row);
			for (int e = Geo::THREADS + tid; e < np_count; e += Geo::THREADS)
				put(b.np[ch.np0 + e], b.np_row[ch.np0 + e]);
			lds_barrier();
		}
		tick(2);          // non-pivotal entries of U added to the rows
		if (ch.npn < 0) {          // (bit 31 of the descriptor)
			// rows with more than two outside dependencies (long rows of U): the rest of their lists
			// (few rows have them: this stage keeps ONE word of a row per lane, RS1 rows per wave instruction.  WPL = 4: its
			//  mapping is worked out here, as phase B's is, instead of living in registers through phase A)
			int slot1 = slot0, wl1 = wl;
			bool ok1 = lane_ok;
			const uint32_t *R1 = Rs;
			if constexpr (WPL > 1) {
				int tid_l = tid;
				asm volatile("" : "+v"(tid_l));
				wl1 = (tid_l & 63) % LPR;
				slot1 = (tid_l >> 6) * Geo::RS1 + (tid_l & 63) / LPR;
				ok1 = (tid_l & 63) < Geo::RS1 * LPR && (int64_t) slab * LPR + wl1 < ldw;
				R1 = static_cast<const uint32_t *>(b.R) + (int64_t) slab * LPR + wl1;
			}
			auto at_off1 = [&](uint32_t off) -> const uint32_t * { return R1 + ((uint64_t) off << 8); };
			for (int s = slot1; s < nrows; s += Geo::RS1 * NW) {
				const int c = ch.lo + s;
				const uint64_t e0 = b.far_rp[c], e1 = b.far_rp[c + 1];
				if (e0 == e1 || !ok1)
					continue;
				uint32_t x = ring[s * RSTR + wl1];
				if constexpr (SGN) {
					int lo, hi;
					sgn_unpack(x, lo, hi);
					for (uint64_t e = e0; e < e1; e += 4) {          // four terms per reduction
#pragma unroll
						for (int t = 0; t < 4; t++) {
							const uint2 en = (e + t < e1) ? b.far[e + t] : uint2{0u, 0u};
							sgn_mad((e + t < e1) ? *at_off1(en.x) : 0u, (int) en.y, lo, hi);          // (en.x: the row's offset)
						}
						lo = sgn_reduce(lo, G);
						hi = sgn_reduce(hi, G);
					}
					x = sgn_pack(lo, hi);
				} else {
					for (uint64_t e = e0; e < e1; e++) {
						const uint2 en = b.far[e];
						x = w_submul<PACKED, PLAIN>(x, *at_off1(en.x), en.y, F, bm);
					}
				}
				ring[s * RSTR + wl1] = x;
			}
			lds_barrier();
		}

		tick(3);          // long lists of outside dependencies
		// ---- phase B: the chain of levels, in LDS ----
		// Columns never meet in a triangular solve, so every wave takes ITS columns (WPW words of every row) through all the
		// levels of the chunk on its own: no barrier between the levels -- the LDS serves a wave's reads and writes in
		// order.  The rows come as a flat table of passes (PASSROWS rows of one level each, levels in order): one 16-byte entry
		// (layout: bs_pass_empty above) holds everything a row with one or two dependencies inside the chunk needs, ring
		// offsets ready and scaled, and the entry of the next trip is in flight during the arithmetic of this one.  (Every wave
		// decodes every entry: the table is what keeps that cheap.)  The ordinary pass knows nothing of rows with more than
		// two dependencies: those have passes of their own, and the table says where (runs of ordinary passes between them).
		{
			constexpr int IPP = PASSROWS / RSB;          // wave instructions (trips) per pass
			const int niter = ch.npass * IPP;
			// the lane's row slot of a trip and its word of a row, worked out here, from a thread id the compiler cannot see through:
			// what hangs on them would otherwise be kept in registers through phase A, which has none to spare
			int tid_b = tid;
			asm volatile("" : "+v"(tid_b));
			const int rsb = (tid_b & 63) / WPW, wlb = (tid_b >> 6) * WPW + (tid_b & 63) % WPW;
			const uint4 *pe = ptab + rsb;
			// byte address in LDS of this lane's word of row 0 of the ring: the entries' offsets are added to it
			const uint32_t wlb_at = (uint32_t) (uintptr_t) (bs_lds_word *) (ring + wlb);
			auto word = [&](uint32_t at) -> bs_lds_word & { return *reinterpret_cast<bs_lds_word *>((uintptr_t) at); };
			auto ordinary = [&](const uint4 e) {
				const uint32_t at_x = bs_ring_at<0>(e.x, wlb_at), at_0 = bs_ring_at<0>(e.y, wlb_at), at_1 = bs_ring_at<1>(e.y, wlb_at);
				if constexpr (SGN) {
					// no branch: an empty slot reads and writes the spare row.  (With a branch around the reads the compiler has
					// to wait for the write of a pass before it may look at the next table entry.)
					const uint32_t x0 = word(at_x), v0 = word(at_0), v1 = word(at_1);          // (one dependency: the same row again, coefficient 0)
					int lo, hi;
					sgn_unpack(x0, lo, hi);
					sgn_mad_half<0, false>(v0, e.z, lo, hi);
					sgn_mad_half<1, false>(v1, e.z, lo, hi);
					word(at_x) = sgn_pack(sgn_reduce(lo, G), sgn_reduce(hi, G));
				} else {
					const uint32_t c0 = PLAIN ? (e.z & 0xFFFFu) : e.z, c1 = PLAIN ? (e.z >> 16) : e.w;
					if (c0 != 0u) {          // (an empty slot has no coefficient)
						uint32_t x = w_submul<PACKED, PLAIN>(word(at_x), word(at_0), c0, F, bm);
						if (c1 != 0u)
							x = w_submul<PACKED, PLAIN>(x, word(at_1), c1, F, bm);
						word(at_x) = x;
					}
				}
			};
			// a row of a long pass: the first dependency inline, the others in the list; an empty slot has cnt = 0
			auto long_row = [&](const uint4 e) {
				const int rest = (int) (e.x >> 16) - 1;
				const uint32_t at_x = bs_ring_at<0>(e.x, wlb_at);
				if constexpr (SGN) {
					const uint32_t x0 = word(at_x), v0 = word(bs_ring_at<0>(e.y, wlb_at));
					int lo, hi;
					sgn_unpack(x0, lo, hi);
					sgn_mad(v0, (int) e.z, lo, hi);
					for (int j = 0; j < rest; j += 4) {
						uint2 em[4];
						uint32_t wm[4];
#pragma unroll
						for (int t = 0; t < 4; t++)
							em[t] = (j + t < rest) ? near[e.w + j + t] : uint2{e.x, 0u};
#pragma unroll
						for (int t = 0; t < 4; t++)
							wm[t] = word(bs_ring_at<0>(em[t].x, wlb_at));
						lo = sgn_reduce(lo, G);          // (one term or four are in already: four more need a fresh start)
						hi = sgn_reduce(hi, G);
#pragma unroll
						for (int t = 0; t < 4; t++)
							sgn_mad(wm[t], (int) em[t].y, lo, hi);
					}
					word(at_x) = sgn_pack(sgn_reduce(lo, G), sgn_reduce(hi, G));
				} else if (rest >= 0) {
					uint32_t x = w_submul<PACKED, PLAIN>(word(at_x), word(bs_ring_at<0>(e.y, wlb_at)), PLAIN ? (e.z & 0xFFFFu) : e.z, F, bm);
					for (int j = 0; j < rest; j++) {
						const uint2 en = near[e.w + j];
						x = w_submul<PACKED, PLAIN>(x, word(bs_ring_at<0>(en.x, wlb_at)), en.y, F, bm);
					}
					word(at_x) = x;
				}
			};
			// (the entry read ahead in the last trip is never used: it lies in the table, or in the first slots of the list behind it)
			uint4 e = pe[0];
			int it = 0, run = ch.nord * IPP;          // trips before the first long pass
			while (it < niter) {
				// (two trips per turn: the entry at hand and the one read ahead swap registers instead of being copied)
				const int stop = min(it + run, niter);
				for (; it + 1 < stop; it += 2) {
					const uint4 e_odd = pe[(it + 1) * RSB];
					ordinary(e);
					e = pe[(it + 2) * RSB];
					ordinary(e_odd);
				}
				if (it < stop) {
					const uint4 e_next = pe[(it + 1) * RSB];
					ordinary(e);
					e = e_next;
					it += 1;
				}
				if (it < niter) {
					run = __builtin_amdgcn_readfirstlane((int) (e.y >> 16)) * IPP;          // ordinary trips up to the next long pass
					for (int q = 0; q < IPP; q++, it++) {
						const uint4 e_next = pe[(it + 1) * RSB];
						long_row(e);
						e = e_next;
					}
				}
			}
		}
		lds_barrier();
		tick(4);          // phase B

		// ---- phase C: write the chunk back ----
		{
			uint32_t off = lo_off + slot0_off;
			asm volatile("" : "+v"(off));          // (as in phase A: stepped, not multiplied)
			for (int s = slot0; s < nrows; s += Geo::ROWS_PER_ITER, off += iter_off)
				if (lane_ok) {
					uint32_t x[WPL];
#pragma unroll
					for (int j = 0; j < WPL; j++)
						x[j] = ring[s * RSTR + wl + j];
					bs_store_words<WPL>(at_off(off), x);
				}
		}
		tick(5);          // phase C: the ring read and the stores issued
		// the metadata of the next chunk goes into LDS behind the stores: its targets (fh, ptab, near) were last read in phase B,
		// which the barrier above has ended, and phase C reads the ring alone.  ONE barrier then ends both
		if (k + 1 < b.nchunks)
			store_meta();
		__syncthreads();          // (workgroup-scope release/acquire: later chunks read these rows; the metadata is in place)
		tick(6);          // metadata of the next chunk into LDS + the barrier (which waits for LDS traffic only: the compiler puts no
		                  // vmcnt(0) in front of a workgroup-scope barrier here, the waves of a workgroup share the CU's L1)
	}
	if (profiling)
		for (int q = 0; q < 8; q++)
			b.prof[q] = pt[q];
}

// --------------------------------------------------------------------------
// S = A_n - A_p R, one wave per row.  The row of S is accumulated in LDS (one word per lane and tile), the pivotal
// entries of the input row are collected in a small LDS list and applied tile by tile.
// --------------------------------------------------------------------------
constexpr int AP_LIST = 64;        // pivotal entries applied per pass (one batch of input entries)
constexpr int AP_TU = 4;           // 64-word tiles per inner step

struct ApplyArgs {
	SchurArgs a;
	const void *R;
	int64_t ldR;                  // in entries
	const int *col;               // column -> compact id
	int r;                        // rows of R
	int Smpad;                    // Sm rounded up to whole tile groups (= ldR)
	int seg_words;                // bs_apply_s16_kernel: words of a row a wave holds in LDS at a time (a multiple of 64 * AP_TU; >= the row: one segment)
	int waves;                    // waves per workgroup
	size_t wave_bytes;            // LDS per wave: row buffer + list
	uint32_t *dense_out;
	int64_t ldS;
	// direct sparse output (no pool, no gather pass): rows are handed out in order through a ticket, every row
	// publishes its length and finds its offset by looking back over the rows before it (single-pass chained scan)
	int direct;
	unsigned long long *status;   // per row: flag << 62 | value; flag 1: value = length of the row, 2: = offset past the row
	int *ticket;                  // LB_TICKETS counters, LB_TICKET_STRIDE ints apart, zeroed before the launch
	int ntickets;                 // counters in use (<= LB_TICKETS, <= workgroups)
	int64_t *Sp;
	int *Sj;
	int *Sx;
	int64_t cap;
	int dbg;                      // always 0 (bit 3 = no loads of R, 5 = no output stores: timing experiments, wrong results).  Kept:
	                              // bs_apply_s16_kernel measured ~3 % slower without the branches on it (close to its run-to-run
	                              // spread; not settled)
	int sgn;                      // R holds signed 16-bit entries (SgnDev)
	SgnDev G;
	unsigned long long *block_sum; // staged output: sum of the lengths of every block of SCAN_BLOCK rows (zeroed before the launch)
	uint32_t *stage;              // staged output (bs_apply_s16_kernel): the packed row of S, Smpad / 2 words per row, and its
	                              // number of entries in a.row_len; bs_expand_kernel writes the sparse rows afterwards
};

constexpr unsigned long long LB_FLAG_LEN = 1ull << 62, LB_FLAG_END = 2ull << 62, LB_VALUE = (1ull << 62) - 1;

// Rows are handed out in (nearly) increasing order, each to a wave that starts it at once: whoever waits for a row in the
// look-back below knows a running wave holds it.  One counter would serve every wave of the chip -- returning atomics on
// one address are served one after the other at the memory side, and a wave waited ~20 us for its row (0.9 ms of a
// 3.5 ms kernel on mk13.b5).  LB_TICKETS counters on separate cache lines each hand out the rows of one residue class;
// the classes advance at the same pace (every class is served by workgroups spread over the whole chip).
constexpr int LB_TICKETS = 16, LB_TICKET_STRIDE = 32;          // (ints: one 128-byte line per counter)

__device__ __forceinline__ int next_ticket(const ApplyArgs &d, int lane)
{
	const int c = (int) (blockIdx.x % (unsigned) d.ntickets);
	int t = 0;
	if (lane == 0)
		t = atomicAdd(d.ticket + c * LB_TICKET_STRIDE, 1);
	t = __builtin_amdgcn_readfirstlane(t);
	const long long k = (long long) t * d.ntickets + c;
	return (k < (long long) d.a.nrows) ? (int) k : d.a.nrows;
}

// Ordered output without a second pass (single-pass chained scan): row k publishes its length, adds up the lengths of
// the rows before it, back to the nearest row that already knows where it ends, and publishes its own end.  Rows are
// handed out by next_ticket().
__device__ __forceinline__ void lb_publish_length(const ApplyArgs &d, int k, int count, int lane)
{
	if (lane == 0)
		__hip_atomic_store(&d.status[k], LB_FLAG_LEN | (unsigned long long) count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One look back from row k (its length published): the status words of row k and the 63 rows before it, then further back
// while no end is found.  true: end = offset past row k.  false: a row in between has not published its length yet -- only
// without `wait`; with it the look is repeated (after 2^24 polls `lost` is set and true returned).  A look that succeeds also
// publishes the ends of the rows of its first window that had only their lengths (row k among them), so that the next look
// stops close by.
__device__ __forceinline__ bool lookback_probe(const ApplyArgs &d, int k, int lane, bool wait, unsigned long long &end, bool &lost)
{
	unsigned long long total = 0, near = 0;          // near: length of this lane's row in the first window (rows before its nearest end)
	int near_end = -1;                               // position of that end in the first window (-1: window not complete yet)
	long long polls = 0;
	for (int j = k; j >= 0;) {
		const int idx = j - lane;
		const unsigned long long val = (idx >= 0) ? __hip_atomic_load(&d.status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : LB_FLAG_END;
		const uint64_t m_end = __ballot((val >> 62) == 2);
		const int first_end = m_end ? __builtin_ctzll(m_end) : 64;
		const bool counts = lane <= first_end;
		if (__ballot(counts && (val >> 62) == 0) != 0) {          // a row in between has not published its length yet
			if (!wait)
				return false;
			if (++polls > (1ll << 24)) {
				lost = true;
				break;
			}
			__builtin_amdgcn_s_sleep(2);
			continue;
		}
		unsigned long long v = counts ? (val & LB_VALUE) : 0ull;
		if (near_end < 0) {
			near_end = first_end;
			near = (lane < first_end) ? v : 0ull;
		}
		for (int sft = 32; sft >= 1; sft >>= 1) {
			const uint32_t lo32 = (uint32_t) __shfl_xor((int) (uint32_t) v, sft);
			const uint32_t hi32 = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), sft);
			v += ((unsigned long long) hi32 << 32) | lo32;
		}
		total += v;
		if (first_end < 64)
			break;
		j -= 64;
	}
	end = total;
	if (!lost && near_end > 0) {
		// the end of row k - lane is `total` less the lengths of the rows after it (the lanes before this one)
		unsigned long long incl = near;
		for (int sft = 1; sft < 64; sft <<= 1) {
			const uint32_t lo32 = (uint32_t) __shfl_up((int) (uint32_t) incl, sft);
			const uint32_t hi32 = (uint32_t) __shfl_up((int) (uint32_t) (incl >> 32), sft);
			if (lane >= sft)
				incl += ((unsigned long long) hi32 << 32) | lo32;
		}
		if (lane < near_end)
			__hip_atomic_store(&d.status[k - lane], LB_FLAG_END | ((total - (incl - near)) & LB_VALUE), __ATOMIC_RELAXED,
			                   __HIP_MEMORY_SCOPE_AGENT);
	}
	return true;
}

// The header of row k of `count` entries, whose look back gave `end`: Sp[k], Sp[nrows] behind the last row, the overflow bit.
// Returns whether the row fits Sj / Sx; off = where it starts.
__device__ __forceinline__ bool lb_row_header(const ApplyArgs &d, int k, int count, unsigned long long end, bool lost, int lane, int64_t &off)
{
	off = (int64_t) (end - (unsigned long long) count);
	const bool fits = !lost && end <= (unsigned long long) d.cap;
	if (lane == 0) {
		d.Sp[k] = off;
		if (k == d.a.nrows - 1)
			d.Sp[d.a.nrows] = (int64_t) end;
		if (!fits)
			atomicOr(&d.a.ctr[CTR_STATUS], 1);
	}
	return fits;
}

// what a wave of an apply kernel leaves in the statistics (lost: a look back gave up)
__device__ __forceinline__ void apply_statistics(const SchurArgs &a, int lane, unsigned long long st_input, unsigned long long st_piv, int st_done, bool lost)
{
	if (lane == 0) {
		if (lost)
			atomicOr(&a.ctr[CTR_STATUS], 4);
		atomicAdd(&a.ctr64[C64_INPUT], st_input);
		atomicAdd(&a.ctr64[C64_ELIM], st_piv);          // rows of R combined (not the reference's count of eliminations)
		atomicAdd(&a.ctr[a.done_ctr], st_done);
	}
}

template <bool PACKED, bool PLAIN> __global__ __launch_bounds__(512) void bs_apply_kernel(ApplyArgs d)
{
	const uint32_t bm = PLAIN ? (uint32_t) (0x100000000ull / d.a.F.p) : 0u;
	constexpr int CPL = Word<PACKED>::CPL;
	using Elem = typename Word<PACKED>::Elem;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	const SchurArgs &a = d.a;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const MontDev F = a.F;
	const int Sm = a.Sm;
	const int nwords = d.Smpad / CPL;                     // a multiple of 64 * AP_TU / CPL >= 128
	uint2 *plist = reinterpret_cast<uint2 *>(lds_raw + (size_t) wave * d.wave_bytes);
	uint32_t *xw = reinterpret_cast<uint32_t *>(plist + AP_LIST);
	Elem *xe = reinterpret_cast<Elem *>(xw);
	const uint32_t *R = static_cast<const uint32_t *>(d.R);
	const int64_t ldw = d.ldR / CPL;
	unsigned long long st_input = 0, st_piv = 0;
	int st_done = 0;
	bool lost = false;

	for (int k = blockIdx.x * d.waves + wave;; k += gridDim.x * d.waves) {
		if (d.direct)
			k = next_ticket(d, lane);
		if (k >= a.nrows)
			break;
		const int i = a.rows[k];
		const int64_t lo = a.Ap[i], hi = a.Ap[i + 1];
		st_input += (unsigned long long) (hi - lo);
		for (int t = lane; t < nwords; t += 64)
			xw[t] = 0;
		int npl = 0;                         // entries waiting in plist (wave-uniform)
		for (int64_t base = lo;; base += 64) {
			// non-pivotal entries go straight into the row buffer, pivotal ones are queued
			bool piv = false;
			uint32_t cid = 0, v = 0;
			if (base + lane < hi) {
				cid = (uint32_t) d.col[a.Aj[base + lane]];
				v = reduce_sum(from_balanced(a.Ax[base + lane], F), F);
				if (cid >= (uint32_t) d.r) {
					const uint32_t t = cid - (uint32_t) d.r;
					uint32_t sum = (uint32_t) xe[t] + v;
					if (sum < v || sum >= F.p)
						sum -= F.p;
					xe[t] = (Elem) sum;
				} else {
					piv = v != 0;
				}
			}
			const uint64_t mk = __ballot(piv);
			if (piv)
				plist[npl + __popcll(mk & ((1ull << lane) - 1ull))] = uint2{cid, PLAIN ? v : montmul(v, F.r2, F)};
			npl += __popcll(mk);
			st_piv += (unsigned long long) __popcll(mk);
			const bool last = base + 64 >= hi;
			if (npl > 0 && (last || npl + 64 > AP_LIST)) {
				// apply the queued pivotal entries: x[tile] -= sum_e a_e R[e][tile]
				for (int t0 = 0; t0 < nwords; t0 += 64 * AP_TU) {
					uint32_t acc[AP_TU];
#pragma unroll
					for (int u = 0; u < AP_TU; u++)
						acc[u] = (t0 + u * 64 < nwords) ? xw[t0 + u * 64 + lane] : 0u;
					// four rows of R at a time: up to 16 loads in flight per lane (a row of mk13.b5 has three pivotal entries:
					// one round trip per tile group)
					for (int e = 0; e < npl; e += 4) {
						uint2 pe[4];
						uint32_t w[4][AP_TU];
#pragma unroll
						for (int q = 0; q < 4; q++) {
							pe[q] = (e + q < npl) ? plist[e + q] : uint2{0u, 0u};          // (coefficient 0: row 0 of R, no effect)
							const uint32_t *rq = R + (int64_t) pe[q].x * ldw + t0 + lane;
#pragma unroll
							for (int u = 0; u < AP_TU; u++)
								w[q][u] = (d.dbg & 8) ? (uint32_t) (lane + u) : (e + q < npl && t0 + u * 64 < nwords) ? rq[u * 64] : 0u;
						}
#pragma unroll
						for (int q = 0; q < 4; q++)
#pragma unroll
							for (int u = 0; u < AP_TU; u++)
								acc[u] = w_submul<PACKED, PLAIN>(acc[u], w[q][u], pe[q].y, F, bm);
					}
#pragma unroll
					for (int u = 0; u < AP_TU; u++)
						if (t0 + u * 64 < nwords)
							xw[t0 + u * 64 + lane] = acc[u];
				}
				npl = 0;
			}
			if (last)
				break;
		}

		// ---- output ----
		if (d.dense_out != nullptr) {
			uint32_t *out = d.dense_out + (int64_t) k * d.ldS;
			for (int t = lane; t < Sm; t += 64)
				out[t] = xe[t];
			if (lane == 0)
				a.row_len[k] = Sm;
			st_done += 1;
			continue;
		}
		// lane l of a tile holds columns CPL * (t0 + l) ..: entries come out sorted by column
		int count = 0;
		for (int t0 = 0; t0 < nwords; t0 += 64) {
			const uint32_t w = xw[t0 + lane];
			if constexpr (PACKED)
				count += __popcll(__ballot((w & 0xFFFFu) != 0)) + __popcll(__ballot((w >> 16) != 0));
			else
				count += __popcll(__ballot(w != 0));
		}
		if (d.stage != nullptr) {          // staged output: the row as it stands + its length (see bs_expand_kernel)
			uint32_t *out = d.stage + (int64_t) k * nwords;
			for (int t = lane; t < nwords; t += 64)
				out[t] = xw[t];
			if (lane == 0) {
				a.row_len[k] = count;
				atomicAdd(&d.block_sum[k / 1024], (unsigned long long) count);          // (SCAN_BLOCK rows per block)
			}
			st_done += 1;
			continue;
		}
		int64_t off = 0;
		int *out_j = a.pool_j, *out_x = a.pool_x;
		bool fits;
		if (d.direct) {
			unsigned long long end = 0;
			lb_publish_length(d, k, count, lane);
			lookback_probe(d, k, lane, true, end, lost);
			fits = lb_row_header(d, k, count, end, lost, lane, off);
			out_j = d.Sj;
			out_x = d.Sx;
		} else {
			unsigned long long got = 0;
			if (lane == 0)
				got = atomicAdd(&a.ctr64[C64_POOL], (unsigned long long) count);
			const uint32_t g_lo = __builtin_amdgcn_readfirstlane((uint32_t) got);
			const uint32_t g_hi = __builtin_amdgcn_readfirstlane((uint32_t) (got >> 32));
			off = (int64_t) (((uint64_t) g_hi << 32) | g_lo);
			fits = off + count <= a.pool_cap;
		}
		if (fits && !(d.dbg & 32)) {
			int64_t wpos = off;
			const uint64_t below = (1ull << lane) - 1ull;
			for (int t0 = 0; t0 < nwords; t0 += 64) {
				const uint32_t w = xw[t0 + lane];
				if constexpr (PACKED) {
					const uint32_t v0 = w & 0xFFFFu, v1 = w >> 16;
					const uint64_t m0 = __ballot(v0 != 0), m1 = __ballot(v1 != 0);
					const int before = __popcll(m0 & below) + __popcll(m1 & below);
					const int c0 = 2 * (t0 + lane);
					if (v0 != 0) {
						out_j[wpos + before] = a.q[c0];
						out_x[wpos + before] = to_balanced(v0, F);
					}
					if (v1 != 0) {
						const int64_t dst = wpos + before + (v0 != 0 ? 1 : 0);
						out_j[dst] = a.q[c0 + 1];
						out_x[dst] = to_balanced(v1, F);
					}
					wpos += __popcll(m0) + __popcll(m1);
				} else {
					const uint64_t mk = __ballot(w != 0);
					if (w != 0) {
						const int64_t dst = wpos + __popcll(mk & below);
						out_j[dst] = a.q[t0 + lane];
						out_x[dst] = to_balanced(w, F);
					}
					wpos += __popcll(mk);
				}
			}
		}
		if (lane == 0 && !d.direct) {          // (lb_row_header has written the header of a direct row)
			if (fits) {
				a.row_off[k] = off | (1LL << 62);       // sorted by column already
				a.row_len[k] = count;
			} else {
				atomicOr(&a.ctr[CTR_STATUS], 1);
				a.row_len[k] = -1;
			}
		}
		st_done += fits ? 1 : 0;
	}
	apply_statistics(a, lane, st_input, st_piv, st_done, lost);
}

// The same with signed 16-bit entries (SgnDev):
//   * one v_mad_i32_i16 per term and component, one reduction per four rows of R;
//   * the rows of R of the next tile group are in flight while the current one is multiplied;
//   * the entries are counted while the last batch is applied (no separate pass over the row), the output loop works on
//     32-bit offsets from a uniform base.
// One segment of a row of S (words w0 .. w0 + nwords of the packed row) into the LDS buffer xw: the non-pivotal entries of
// the input row [lo, hi) are added in, the pivotal ones queued in plist and applied.  Returns the entries of the segment,
// or -1 when the last batch had no pivotal entry (the segment was not swept: the caller counts if it needs them).
// DEEP: two units of loads in flight while one is multiplied instead of one (for a caller whose occupancy the LDS limits,
// not the registers).
template <bool DEEP>
__device__ __forceinline__ int s16_reduce_segment(const ApplyArgs &d, const MontDev &F, const SgnDev &G, int64_t lo, int64_t hi, int w0, int nwords,
                                                  uint2 *plist, uint32_t *xw, int lane, bool first_seg, unsigned long long &st_piv)
{
	short *xe = reinterpret_cast<short *>(xw);
	const uint32_t *R = static_cast<const uint32_t *>(d.R);
	const uint32_t ldw256 = (uint32_t) (d.ldR / 2 / 256);          // row stride of R in units of 256 words (rows are padded to 512 columns):
	                                                               // the offset of a row in these units fits 32 bits for any R below 4 TB
	for (int t = lane; t < nwords; t += 64)
		xw[t] = 0;
	int npl = 0;                         // entries waiting in plist (wave-uniform)
	int count = -1;                      // entries of the finished segment, once known
	for (int64_t base = lo;; base += 64) {
		bool piv = false;
		uint32_t cid = 0;
		int bal = 0;
		if (base + lane < hi) {
			cid = (uint32_t) d.col[d.a.Aj[base + lane]];
			bal = sgn_from_residue(reduce_sum(from_balanced(d.a.Ax[base + lane], F), F), G);
			if (cid >= (uint32_t) d.r) {
				const uint32_t t = cid - (uint32_t) d.r - 2u * (uint32_t) w0;          // (unsigned: columns before the segment wrap around)
				if (t < 2u * (uint32_t) nwords)
					xe[t] = (short) sgn_canonical((int) xe[t] + bal, G);
			} else {
				piv = bal != 0;
			}
		}
		const uint64_t mk = __ballot(piv);
		if (piv)
			plist[npl + __popcll(mk & ((1ull << lane) - 1ull))] = uint2{cid * ldw256, (uint32_t) (-bal)};          // (where the row of R starts, in units of 256 words)
		npl += __popcll(mk);
		st_piv += first_seg ? (unsigned long long) __popcll(mk) : 0ull;
		const bool last = base + 64 >= hi;
		if (npl > 0 && (last || npl + 64 > AP_LIST)) {
			// apply the queued pivotal entries: x[tile group] += sum_e (-a_e) R[e][tile group], four rows of R at a
			// time.  A unit = (tile group, four entries of the list); the loads of unit u + 1 are issued before unit
			// u is multiplied.
			const int ne = (npl + 3) >> 2;
			const int nunits = (nwords / (64 * AP_TU)) * ne;
			int cnt = 0;
			int alo[AP_TU], ahi[AP_TU];
			uint32_t wa[4][AP_TU], wb[4][AP_TU], wc[4][AP_TU];
			int ca[4], cb[4], cc[4];
			int pf_t0 = 0, pf_e = 0;                 // unit the next issue() will load
			// (no branch in here: the wait counts of the multiplications are static, and a path that skips an issue
			//  would force them all to the count of that path.  Past the last unit the last tile group is read again.)
			const int t0_last = nwords - 64 * AP_TU;
			const int64_t row_mask = (d.dbg & 8) ? 0 : -1;
			auto issue = [&](uint32_t (&w)[4][AP_TU], int (&cf)[4]) {
				const int t0c = (pf_t0 < t0_last) ? pf_t0 : t0_last;
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const int idx = (pf_e + q < npl) ? pf_e + q : npl - 1;
					const uint2 pe = plist[idx];
					cf[q] = (pf_e + q < npl) ? (int) pe.y : 0;          // (coefficient 0: no effect)
					const uint32_t *rq = R + ((((uint64_t) pe.x) << 8) & (uint64_t) row_mask) + w0 + t0c + lane;
#pragma unroll
					for (int u = 0; u < AP_TU; u++)
						w[q][u] = rq[u * 64];          // (rows are padded to whole tile groups)
				}
				pf_e += 4;
				const bool wrap = pf_e >= npl;
				pf_e = wrap ? 0 : pf_e;
				pf_t0 += wrap ? 64 * AP_TU : 0;
			};
			int t0 = 0, e = 0;                       // unit being multiplied
			auto multiply = [&](const uint32_t (&w)[4][AP_TU], const int (&cf)[4]) {
				if (e == 0) {
#pragma unroll
					for (int u = 0; u < AP_TU; u++)
						sgn_unpack(xw[t0 + u * 64 + lane], alo[u], ahi[u]);
				} else {                 // four terms were added already
#pragma unroll
					for (int u = 0; u < AP_TU; u++) {
						alo[u] = sgn_reduce(alo[u], G);
						ahi[u] = sgn_reduce(ahi[u], G);
					}
				}
#pragma unroll
				for (int q = 0; q < 4; q++)
#pragma unroll
					for (int u = 0; u < AP_TU; u++)
						sgn_mad(w[q][u], cf[q], alo[u], ahi[u]);
				e += 4;
				if (e >= npl) {
#pragma unroll
					for (int u = 0; u < AP_TU; u++) {
						const int rl = sgn_reduce(alo[u], G), rh = sgn_reduce(ahi[u], G);
						xw[t0 + u * 64 + lane] = sgn_pack(rl, rh);
						cnt += __popcll(__ballot(rl != 0)) + __popcll(__ballot(rh != 0));
					}
					e = 0;
					t0 += 64 * AP_TU;
				}
			};
			issue(wa, ca);
			if constexpr (DEEP) {
				issue(wb, cb);
				for (int u = 0; u < nunits; u += 3) {
					issue(wc, cc);
					multiply(wa, ca);
					issue(wa, ca);
					if (u + 1 < nunits)
						multiply(wb, cb);
					issue(wb, cb);
					if (u + 2 < nunits)
						multiply(wc, cc);
				}
			} else {
				for (int u = 0; u < nunits; u += 2) {
					issue(wb, cb);
					multiply(wa, ca);
					issue(wa, ca);
					if (u + 1 < nunits)
						multiply(wb, cb);
				}
			}
			if (last)
				count = cnt;
			npl = 0;
		}
		if (last)
			break;
	}
	return count;
}

// entries of the packed words xw[0 .. nwords) (a segment that s16_reduce_segment did not sweep)
__device__ __forceinline__ int s16_count_entries(const uint32_t *xw, int nwords, int lane)
{
	int count = 0;
	for (int t0 = 0; t0 < nwords; t0 += 64) {
		const uint32_t w = xw[t0 + lane];
		count += __popcll(__ballot((w & 0xFFFFu) != 0)) + __popcll(__ballot((w >> 16) != 0));
	}
	return count;
}

__global__ __launch_bounds__(512) void bs_apply_s16_kernel(ApplyArgs d)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	const SchurArgs &a = d.a;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const MontDev F = a.F;
	const SgnDev G = d.G;
	const int Sm = a.Sm;
	const int nwords_row = d.Smpad / 2;                   // a multiple of 64 * AP_TU
	// A row wider than the LDS a wave may have (mk14.b4: 42,356 non-pivotal columns = 85 KB) is produced in SEGMENTS of
	// seg_words words: the few entries of the input row are walked once per segment, the rows of R are read segment by
	// segment -- every byte of R once, as before.  Staged and dense output only (the offset of a sparse row is known once
	// its last segment is).
	const int nseg = (nwords_row + d.seg_words - 1) / d.seg_words;
	uint2 *plist = reinterpret_cast<uint2 *>(lds_raw + (size_t) wave * d.wave_bytes);
	uint32_t *xw = reinterpret_cast<uint32_t *>(plist + AP_LIST);
	short *xe = reinterpret_cast<short *>(xw);
	const int2 *q2 = reinterpret_cast<const int2 *>(a.q);          // (the array is padded to whole tile groups)
	unsigned long long st_input = 0, st_piv = 0;
	int st_done = 0;
	bool lost = false;

	for (int k = blockIdx.x * d.waves + wave;; k += gridDim.x * d.waves) {
		if (d.direct)
			k = next_ticket(d, lane);
		if (k >= a.nrows)
			break;
		const int i = a.rows[k];
		const int64_t lo = a.Ap[i], hi = a.Ap[i + 1];
		st_input += (unsigned long long) (hi - lo);
		int total = 0;                       // entries of the segments done so far
	  for (int seg = 0; seg < nseg; seg++) {
		const int w0 = seg * d.seg_words, nwords = min(d.seg_words, nwords_row - w0);
		int count = s16_reduce_segment<false>(d, F, G, lo, hi, w0, nwords, plist, xw, lane, seg == 0, st_piv);

		// ---- output ----
		if (d.dense_out != nullptr) {
			uint32_t *out = d.dense_out + (int64_t) k * d.ldS + 2 * w0;
			for (int t = lane; t < min(2 * nwords, Sm - 2 * w0); t += 64) {
				const int v = (int) xe[t];
				out[t] = (uint32_t) (v < 0 ? v + G.p : v);
			}
			if (seg + 1 < nseg)
				continue;
			if (lane == 0)
				a.row_len[k] = Sm;
			st_done += 1;
			continue;
		}
		if (count < 0)                       // no pivotal entry in the last batch: the segment was not swept
			count = s16_count_entries(xw, nwords, lane);
		total += count;
		if (d.stage != nullptr) {
			uint32_t *out = d.stage + (int64_t) k * nwords_row + w0;
			for (int t = lane; t < nwords; t += 64)
				out[t] = xw[t];
			if (seg + 1 < nseg)
				continue;
			if (lane == 0) {
				a.row_len[k] = total;
				atomicAdd(&d.block_sum[k / 1024], (unsigned long long) total);          // (SCAN_BLOCK rows per block)
			}
			st_done += 1;
			continue;
		}
		// (sparse rows straight from the LDS: one segment, the launcher sees to it)
		int64_t off = 0;
		int *out_j = a.pool_j, *out_x = a.pool_x;
		bool fits;
		if (d.direct) {
			unsigned long long end = 0;
			lb_publish_length(d, k, count, lane);
			lookback_probe(d, k, lane, true, end, lost);
			fits = lb_row_header(d, k, count, end, lost, lane, off);
			out_j = d.Sj;
			out_x = d.Sx;
		} else {
			unsigned long long got = 0;
			if (lane == 0)
				got = atomicAdd(&a.ctr64[C64_POOL], (unsigned long long) count);
			const uint32_t g_lo = __builtin_amdgcn_readfirstlane((uint32_t) got);
			const uint32_t g_hi = __builtin_amdgcn_readfirstlane((uint32_t) (got >> 32));
			off = (int64_t) (((uint64_t) g_hi << 32) | g_lo);
			fits = off + count <= a.pool_cap;
		}
		if (fits && !(d.dbg & 32)) {
			// lane l of a tile holds columns 2 (t0 + l) and 2 (t0 + l) + 1: entries come out sorted by column
			int *oj = out_j + off, *ox = out_x + off;
			uint32_t wpos = 0;
			for (int t0 = 0; t0 < nwords; t0 += 64) {
				int v0, v1;
				sgn_unpack(xw[t0 + lane], v0, v1);
				v0 = sgn_canonical(v0, G);
				v1 = sgn_canonical(v1, G);
				const uint64_t m0 = __ballot(v0 != 0), m1 = __ballot(v1 != 0);
				const int2 qq = q2[t0 + lane];
				uint32_t dst = wpos;
				dst = __builtin_amdgcn_mbcnt_hi((uint32_t) (m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m0, dst));
				dst = __builtin_amdgcn_mbcnt_hi((uint32_t) (m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m1, dst));
				if (v0 != 0) {
					oj[dst] = qq.x;
					ox[dst] = v0;
					dst += 1;
				}
				if (v1 != 0) {
					oj[dst] = qq.y;
					ox[dst] = v1;
				}
				wpos += (uint32_t) (__popcll(m0) + __popcll(m1));
			}
		}
		if (lane == 0 && !d.direct) {          // (lb_row_header has written the header of a direct row)
			if (fits) {
				a.row_off[k] = off | (1LL << 62);       // sorted by column already
				a.row_len[k] = count;
			} else {
				atomicOr(&a.ctr[CTR_STATUS], 1);
				a.row_len[k] = -1;
			}
		}
		st_done += fits ? 1 : 0;
	  }          // segments
	}
	apply_statistics(a, lane, st_input, st_piv, st_done, lost);
}

// ---- CSR output straight from the apply (signed 16-bit entries, rows of one segment) ---------------------------------------
// bs_apply_s16_csr_kernel writes every row of S at its final place in Sj / Sx, without the staging pass below.  A wave computes
// a row in its LDS row buffer; the finished row publishes its length (look-back status word, as the `direct` output above) and
// stays PENDING while the wave computes the next row: at every row boundary the wave takes ONE look, without waiting, whether
// the offset of its older pending row is known (every row before it has published its length), and once it is, writes that
// row.  A wave waits only when two rows are pending, and at the end of the batch.  (The `direct` output makes every row wait
// for its slowest running predecessor with its LDS held: a third of its time on mk13.b5.)  Where the older pending row waits
// is a policy (PendingLds, PendingRegs below).
constexpr int CSR_SCRATCH_BYTES = 512 * 4;          // per wave: the list of pivotal entries while a row is computed, the
                                                    // compaction area of the output (512 ints) while a row is written
static_assert(CSR_SCRATCH_BYTES >= AP_LIST * (int) sizeof(uint2), "the list shares the compaction area");

// One tile group of a row to oj / ox from entry wpos on: word(u) is the packed word of this lane in tile u of the group
// (u an integral constant), qq the two columns it holds.  As bs_expand_kernel, the entries of the four tiles are compacted in
// LDS and leave in stores of 64 consecutive entries -- here through ONE area: the columns first, then the values.
// Lane l of a tile holds columns 2 (t0 + l) and 2 (t0 + l) + 1: entries come out sorted by column.
template <typename WordAt>
__device__ __forceinline__ void csr_emit_group(WordAt &&word, const int2 (&qq)[AP_TU], const SgnDev &G, int *cbuf, int *oj, int *ox, uint32_t &wpos, int lane)
{
	int v0[AP_TU], v1[AP_TU];
	uint32_t dst[AP_TU], gpos = 0;
	bs_static_for<0, AP_TU>([&](auto uu) {
		constexpr int u = decltype(uu)::value;
		sgn_unpack(word(uu), v0[u], v1[u]);
		v0[u] = sgn_canonical(v0[u], G);
		v1[u] = sgn_canonical(v1[u], G);
		const uint64_t m0 = __ballot(v0[u] != 0), m1 = __ballot(v1[u] != 0);
		uint32_t at = gpos;
		at = __builtin_amdgcn_mbcnt_hi((uint32_t) (m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m0, at));
		at = __builtin_amdgcn_mbcnt_hi((uint32_t) (m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m1, at));
		dst[u] = at;
		if (v0[u] != 0)
			cbuf[at] = qq[u].x;
		if (v1[u] != 0)
			cbuf[at + (v0[u] != 0 ? 1u : 0u)] = qq[u].y;
		gpos += (uint32_t) (__popcll(m0) + __popcll(m1));
	});
	for (uint32_t t = lane; t < gpos; t += 64)
		oj[wpos + t] = cbuf[t];
#pragma unroll
	for (int u = 0; u < AP_TU; u++) {
		if (v0[u] != 0)
			cbuf[dst[u]] = v0[u];
		if (v1[u] != 0)
			cbuf[dst[u] + (v0[u] != 0 ? 1u : 0u)] = v1[u];
	}
	for (uint32_t t = lane; t < gpos; t += 64)
		ox[wpos + t] = cbuf[t];
	wpos += gpos;
}

// The next row of the batch into the row buffer xw (nwords words: the whole row), its length published.  Returns the row
// (>= nrows: none left), count = its entries.
template <bool DEEP>
__device__ __forceinline__ int csr_produce_row(const ApplyArgs &d, const MontDev &F, const SgnDev &G, int nwords, uint2 *plist, uint32_t *xw, int lane,
                                               int &count, unsigned long long &st_input, unsigned long long &st_piv)
{
	const int k = next_ticket(d, lane);
	if (k >= d.a.nrows)
		return k;
	const int i = d.a.rows[k];
	const int64_t lo = d.a.Ap[i], hi = d.a.Ap[i + 1];
	st_input += (unsigned long long) (hi - lo);
	count = s16_reduce_segment<DEEP>(d, F, G, lo, hi, 0, nwords, plist, xw, lane, true, st_piv);
	if (count < 0)                       // no pivotal entry in the last batch: the row was not swept
		count = s16_count_entries(xw, nwords, lane);
	lb_publish_length(d, k, count, lane);
	return k;
}

// Where the older pending row of a wave waits.  A policy sets up the row buffers of the wave (`rows`: its LDS past the scratch
// area; xc = the buffer rows are computed in), hands the row in xc over to the pending place, and sweeps the pending row for
// the output: emit(word, qq) once per tile group, in order, word and qq as csr_emit_group takes them.  The columns of the next
// two groups are in flight during the stores of a group.
//
// PendingLds: a second LDS buffer (LDS per wave: CSR_SCRATCH_BYTES, then two buffers of Smpad / 2 words); the hand-over swaps
// the two.  Rows of any width that fits.
struct PendingLds {
	int nwords;                                          // the whole row: one segment (a multiple of 64 * AP_TU)
	uint32_t *xc, *xp;

	__device__ __forceinline__ PendingLds(const ApplyArgs &d, uint32_t *rows) : nwords(d.Smpad / 2), xc(rows), xp(rows + d.Smpad / 2) {}

	__device__ __forceinline__ void hand_over(int)
	{
		uint32_t *const t = xp;
		xp = xc;
		xc = t;
	}

	template <typename Emit> __device__ __forceinline__ void sweep(const int *q, int lane, Emit &&emit)
	{
		constexpr int GW = 64 * AP_TU;          // words of a group
		const int2 *q2 = reinterpret_cast<const int2 *>(q) + lane;          // (the array is padded to whole tile groups)
		const int last = nwords - GW;
		int2 qa[AP_TU], qb[AP_TU], qc[AP_TU];
		// (no branch around an issue: past the end the last group is read again)
		auto issue = [&](int t0, int2 (&qq)[AP_TU]) {
			const int t = (t0 < last) ? t0 : last;
#pragma unroll
			for (int u = 0; u < AP_TU; u++)
				qq[u] = q2[t + 64 * u];
		};
		auto group = [&](int t0, const int2 (&qq)[AP_TU]) {
			emit([&](auto uu) -> uint32_t { return xp[t0 + 64 * decltype(uu)::value + lane]; }, qq);
		};
		issue(0, qa);
		issue(GW, qb);
		for (int t0 = 0; t0 < nwords; t0 += 3 * GW) {
			issue(t0 + 2 * GW, qc);
			group(t0, qa);
			issue(t0 + 3 * GW, qa);
			if (t0 + GW < nwords)
				group(t0 + GW, qb);
			issue(t0 + 4 * GW, qb);
			if (t0 + 2 * GW < nwords)
				group(t0 + 2 * GW, qc);
		}
	}
};

// PendingRegs<NT>: a static register file, one packed word per lane and tile -- half the LDS per wave, so twice the waves on a
// CU (mk13.b5: 12 KB against 22 KB).  NT = 64-word tiles of a row (Smpad = 128 NT columns, a multiple of AP_TU).  The hand-over
// is NT ds_reads at static indices.  Every index into the register file is a compile-time constant (the sweep is unrolled over
// the tile groups): a dynamic one would turn the file into scratch.
constexpr int CSR_ROWREG_MAX_TILES = 40;            // widest instantiation: Smpad = 5,120 columns, 40 registers
constexpr bool CSR_ROWREG_DEEP = false;
constexpr int CSR_ROWREG_WPE = 4;

template <int NT> struct PendingRegs {
	static_assert(NT % AP_TU == 0 && NT >= AP_TU && NT <= CSR_ROWREG_MAX_TILES, "whole tile groups");
	static constexpr int nwords = 64 * NT;               // the whole row: one segment
	uint32_t *xc;
	RegFile<uint32_t, NT> xr;

	__device__ __forceinline__ PendingRegs(const ApplyArgs &, uint32_t *rows) : xc(rows) {}

	__device__ __forceinline__ void hand_over(int lane)
	{
		bs_static_for<0, NT>([&](auto tt) {
			constexpr int t = decltype(tt)::value;
			xr.template at<t>() = xc[64 * t + lane];
		});
	}

	template <typename Emit> __device__ __forceinline__ void sweep(const int *q, int lane, Emit &&emit)
	{
		constexpr int NG = NT / AP_TU;          // tile groups of a row
		constexpr int GW = 64 * AP_TU;          // words of a group
		int2 qa[AP_TU], qb[AP_TU], qc[AP_TU];
		// (the byte offset of a group goes through an empty asm: as constants, the 64-bit addresses of every group would be
		//  formed once before the loop over the rows and held in two registers each)
		auto issue = [&](int t0, int2 (&qq)[AP_TU]) {
			uint32_t at = (uint32_t) (t0 + lane) * (uint32_t) sizeof(int2);
			asm volatile("" : "+v"(at));
			const int2 *qg = reinterpret_cast<const int2 *>(reinterpret_cast<const char *>(q) + at);
#pragma unroll
			for (int u = 0; u < AP_TU; u++)
				qq[u] = qg[64 * u];
		};
		issue(0, qa);
		if constexpr (NG > 1)
			issue(GW, qb);
		bs_static_for<0, NG>([&](auto gg) {
			constexpr int g = decltype(gg)::value;
			auto word = [&](auto uu) -> uint32_t { return xr.template at<g * AP_TU + decltype(uu)::value>(); };
			if constexpr (g % 3 == 0) {
				if constexpr (g + 2 < NG)
					issue((g + 2) * GW, qc);
				emit(word, qa);
			} else if constexpr (g % 3 == 1) {
				if constexpr (g + 2 < NG)
					issue((g + 2) * GW, qa);
				emit(word, qb);
			} else {
				if constexpr (g + 2 < NG)
					issue((g + 2) * GW, qb);
				emit(word, qc);
			}
		});
	}
};

// Rows are handed out by next_ticket(); every workgroup of the grid must be resident (the launcher sees to it).
// DEEP: as s16_reduce_segment.  WPE: waves per SIMD the register allocation must leave room for (0: no bound).
template <typename Pending, bool DEEP, int WPE>
__global__ __launch_bounds__(512, WPE) void bs_apply_s16_csr_kernel(ApplyArgs d)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	const SchurArgs &a = d.a;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const MontDev F = a.F;
	const SgnDev G = d.G;
	unsigned char *area = lds_raw + (size_t) wave * d.wave_bytes;
	uint2 *plist = reinterpret_cast<uint2 *>(area);
	int *cbuf = reinterpret_cast<int *>(area);           // (the list is not in use while a row is written)
	Pending pend(d, reinterpret_cast<uint32_t *>(area + CSR_SCRATCH_BYTES));
	unsigned long long st_input = 0, st_piv = 0;
	int st_done = 0;
	bool lost = false;
	// rows whose offset was not known yet (-1: none; wave-uniform): k0 in the pending place (the older one), k1 in the buffer xc
	int k0 = -1, c0 = 0, k1 = -1, c1 = 0;

	// row k0 to Sj / Sx once its offset is known (one look, or looks until it is with `wait`)
	auto settle = [&](bool wait) {
		unsigned long long end = 0;
		if (!lookback_probe(d, k0, lane, wait, end, lost))
			return;
		int64_t off = 0;
		const bool fits = lb_row_header(d, k0, c0, end, lost, lane, off);
		if (fits && c0 > 0) {
			int *oj = d.Sj + off, *ox = d.Sx + off;
			uint32_t wpos = 0;
			pend.sweep(a.q, lane, [&](auto &&word, const int2 (&qq)[AP_TU]) { csr_emit_group(word, qq, G, cbuf, oj, ox, wpos, lane); });
		}
		st_done += fits ? 1 : 0;
		k0 = -1;
	};
	// the row in xc becomes the older pending row (the pending place is free)
	auto hand_over = [&]() {
		pend.hand_over(lane);
		k0 = k1;
		c0 = c1;
		k1 = -1;
	};

	// at the top of a turn: nothing pending, or k1 alone (the row of the last turn), or both
	for (bool finishing = false;;) {
		if (k1 >= 0 && k0 < 0)
			hand_over();
		if (k0 >= 0)
			settle(k1 >= 0 || finishing);          // one look; with both taken (and at the end), until the older row is written
		if (k1 >= 0)
			hand_over();
		if (finishing)
			break;
		int count = 0;
		const int k = csr_produce_row<DEEP>(d, F, G, pend.nwords, plist, pend.xc, lane, count, st_input, st_piv);
		if (k >= a.nrows) {
			finishing = true;
			continue;
		}
		k1 = k;
		c1 = count;
	}
	apply_statistics(a, lane, st_input, st_piv, st_done, lost);
}

// ---- staged sparse output (signed 16-bit entries) --------------------------------------------------
// Writing the rows of S in order from ONE kernel makes every row wait for the lengths of the rows before it -- with
// 3584 rows in flight a row waits for the slowest of its several hundred running predecessors, a third of its own time
// on mk13.b5 -- and the waiting rows keep their LDS.  Two kernels instead: bs_apply_s16_kernel leaves the packed row
// (2 bytes per column) and its length, one small scan turns lengths into offsets, bs_expand_kernel streams the
// packed rows out as (column, value) pairs.  Nobody waits for anybody; the price is one write and one read of the
// packed rows (a third of the bytes of the result).
// offsets from lengths.  The apply kernel has added every length to the sum of its block of SCAN_BLOCK rows
// (block_sum); workgroup g adds up the sums of the blocks before it and scans its own block.
constexpr int SCAN_BLOCK = 1024;

__global__ __launch_bounds__(SCAN_BLOCK) void bs_scan_lengths_kernel(const int *len, int n, const unsigned long long *block_sum, int64_t *Sp, int64_t cap,
                                                                      int *ctr)
{
	__shared__ long long part[SCAN_BLOCK / 64];
	__shared__ long long s_base;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int g = blockIdx.x;
	auto wave_sum = [](long long v) -> long long {
		for (int sft = 32; sft >= 1; sft >>= 1) {
			const uint32_t lo32 = (uint32_t) __shfl_xor((int) (uint32_t) v, sft);
			const uint32_t hi32 = (uint32_t) __shfl_xor((int) (uint32_t) ((unsigned long long) v >> 32), sft);
			v += (long long) (((unsigned long long) hi32 << 32) | lo32);
		}
		return v;
	};
	// blocks before this one
	long long before = 0;
	for (int b = tid; b < g; b += SCAN_BLOCK)
		before += (long long) block_sum[b];
	before = wave_sum(before);
	if (lane == 0)
		part[wave] = before;
	__syncthreads();
	if (tid == 0) {
		long long t = Sp[0];                 // (where this slice of rows starts)
		for (int w = 0; w < SCAN_BLOCK / 64; w++)
			t += part[w];
		s_base = t;
	}
	__syncthreads();
	const long long base = s_base;
	__syncthreads();
	// inclusive scan of the block: inside a wave, then over the waves
	const int k = g * SCAN_BLOCK + tid;
	const long long mine = (k < n) ? (long long) len[k] : 0;
	long long incl = mine;
	for (int sft = 1; sft < 64; sft <<= 1) {
		const uint32_t lo32 = (uint32_t) __shfl_up((int) (uint32_t) incl, sft);
		const uint32_t hi32 = (uint32_t) __shfl_up((int) (uint32_t) ((unsigned long long) incl >> 32), sft);
		if (lane >= sft)
			incl += (long long) (((unsigned long long) hi32 << 32) | lo32);
	}
	if (lane == 63)
		part[wave] = incl;
	__syncthreads();
	long long waves_before = 0;
	for (int w = 0; w < wave; w++)
		waves_before += part[w];
	const long long end = base + waves_before + incl;
	if (k < n) {
		Sp[k + 1] = end;
		if (k == n - 1 && end > cap)
			atomicOr(&ctr[CTR_STATUS], 1);
	}
}

struct ExpandArgs {
	const uint32_t *stage;
	int nwords, nrows;
	const int64_t *Sp;
	int *Sj, *Sx;
	int64_t cap;
	const int *q;
	SgnDev G;                     // (p, -p, p / 2: every format uses them)
};

// FMT 0: signed 16-bit entries, two per word; 1: residues in 16 bits, two per word; 2: residues, one per word

template <int FMT> __global__ __launch_bounds__(256) void bs_expand_kernel(ExpandArgs e)
{
	constexpr int TU = 4;                // tiles per group (rows are padded to whole groups of four tiles)
	// The entries of a group are compacted in LDS and leave as dense, contiguous stores (64 consecutive entries per
	// instruction).  Written straight from the lanes that hold them, an instruction covers every other slot of a
	// 512-byte span and the holes are filled by the next one: the same bytes took 1.74 ms instead of 1.1.
	__shared__ int stage_j[4][128 * TU], stage_x[4][128 * TU];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int wave = (int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int) ((gridDim.x * blockDim.x) >> 6);
	const int2 *q2 = reinterpret_cast<const int2 *>(e.q) + lane;          // (two columns per word)
	const int *q1 = e.q + lane;                                             // (one column per word: FMT 2)
	const SgnDev G = e.G;
	const uint32_t pu = (uint32_t) G.p, halfu = (uint32_t) G.half;
	auto balanced = [&](uint32_t v) -> int { return (v > halfu) ? (int) (v - pu) : (int) v; };          // residue -> [-p/2, p/2]
	const int last = e.nwords - 64 * TU;
	int *sj = stage_j[wv], *sx = stage_x[wv];
	for (int k = wave; k < e.nrows; k += nwaves) {
		const int64_t off = e.Sp[k], end = e.Sp[k + 1];
		if (end > e.cap || end == off)
			continue;                    // (the scan has raised the overflow flag) / empty row
		const uint32_t *row = e.stage + (int64_t) k * e.nwords + lane;
		int *oj = e.Sj + off, *ox = e.Sx + off;
		uint32_t wpos = 0;
		// The loads of the next group are issued BEFORE the stores of this one: stores and loads share one in-order
		// counter.  (No branch around the issue -- the wait counts are static; past the end the last group is read again.)
		uint32_t wa[TU], wb[TU];
		int2 qa[TU], qb[TU];
		auto issue = [&](int t0, uint32_t (&w)[TU], int2 (&qq)[TU]) {
			const int t = (t0 < last) ? t0 : last;
#pragma unroll
			for (int u = 0; u < TU; u++)
				w[u] = __builtin_nontemporal_load(row + t + 64 * u);
#pragma unroll
			for (int u = 0; u < TU; u++)
				qq[u] = (FMT == 2) ? int2{q1[t + 64 * u], 0} : q2[t + 64 * u];
		};
		// lane l of a tile holds columns 2 (t0 + l) and 2 (t0 + l) + 1: entries come out sorted by column
		auto emit = [&](const uint32_t (&w)[TU], const int2 (&qq)[TU]) {
			uint32_t gpos = 0;
#pragma unroll
			for (int u = 0; u < TU; u++) {
				int v0, v1;
				if constexpr (FMT == 0) {
					sgn_unpack(w[u], v0, v1);
					v0 = sgn_canonical(v0, G);
					v1 = sgn_canonical(v1, G);
				} else if constexpr (FMT == 1) {
					v0 = balanced(w[u] & 0xFFFFu);
					v1 = balanced(w[u] >> 16);
				} else {
					v0 = balanced(w[u]);
					v1 = 0;
				}
				const uint64_t m0 = __ballot(v0 != 0), m1 = __ballot(v1 != 0);
				uint32_t dst = gpos;
				dst = __builtin_amdgcn_mbcnt_hi((uint32_t) (m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m0, dst));
				dst = __builtin_amdgcn_mbcnt_hi((uint32_t) (m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m1, dst));
				if (v0 != 0) {
					sj[dst] = qq[u].x;
					sx[dst] = v0;
					dst += 1;
				}
				if (v1 != 0) {
					sj[dst] = qq[u].y;
					sx[dst] = v1;
				}
				gpos += (uint32_t) (__popcll(m0) + __popcll(m1));
			}
			for (uint32_t t = lane; t < gpos; t += 64) {
				oj[wpos + t] = sj[t];
				ox[wpos + t] = sx[t];
			}
			wpos += gpos;
		};
		issue(0, wa, qa);
		for (int t0 = 0; t0 < e.nwords; t0 += 2 * 64 * TU) {
			issue(t0 + 64 * TU, wb, qb);
			emit(wa, qa);
			issue(t0 + 2 * 64 * TU, wa, qa);
			if (t0 + 64 * TU < e.nwords)
				emit(wb, qb);
		}
	}
}

// Dense rows for FEW, LONG input rows (the completion test combines every remaining row: ~10 rows of ~10^5 entries):
// one wave per row would leave the chip idle, so a workgroup takes (row, group of 256 words) and its waves split the
// entries of the row; partial sums meet in LDS.
constexpr int AW_NW = 8;

template <bool PACKED, bool PLAIN> __global__ __launch_bounds__(64 * AW_NW) void bs_apply_wide_kernel(ApplyArgs d)
{
	const uint32_t bm = PLAIN ? (uint32_t) (0x100000000ull / d.a.F.p) : 0u;
	constexpr int CPL = Word<PACKED>::CPL;
	__shared__ uint32_t part[AW_NW][AP_TU * 64];
	const SchurArgs &a = d.a;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const MontDev F = a.F;
	const int k = blockIdx.y;
	const int w0 = blockIdx.x * 64 * AP_TU;                 // first word of this workgroup's tile group
	const int nwords = d.Smpad / CPL;
	const uint32_t *R = static_cast<const uint32_t *>(d.R);
	const int64_t ldw = d.ldR / CPL;
	const int i = a.rows[k];
	const int64_t lo = a.Ap[i], hi = a.Ap[i + 1];
	uint32_t acc[AP_TU];
#pragma unroll
	for (int u = 0; u < AP_TU; u++)
		acc[u] = 0;
	for (int64_t base = lo + 64 * wave; base < hi; base += 64 * AW_NW) {
		uint32_t cid = 0xFFFFFFFFu, v = 0;
		if (base + lane < hi) {
			cid = (uint32_t) d.col[a.Aj[base + lane]];
			v = reduce_sum(from_balanced(a.Ax[base + lane], F), F);
		}
		// non-pivotal entries of this tile group: added by the lane that owns the column
		const bool np_here = v != 0 && cid != 0xFFFFFFFFu && cid >= (uint32_t) d.r;
		uint64_t todo = __ballot(np_here);
		while (todo != 0) {
			const int src = __builtin_ctzll(todo);
			todo &= todo - 1;
			const uint32_t t = (uint32_t) __shfl((int) cid, src) - (uint32_t) d.r;      // column among the non-pivotal ones
			const uint32_t val = (uint32_t) __shfl((int) v, src);
			const int word = (int) (t / CPL) - w0;
			if (word >= 0 && word < 64 * AP_TU && (word & 63) == lane) {
				const int u = word >> 6;
#pragma unroll
				for (int q = 0; q < AP_TU; q++)
					if (q == u) {
						if constexpr (PACKED) {
							const int sh = (t & 1) ? 16 : 0;
							uint32_t part_v = ((acc[q] >> sh) & 0xFFFFu) + val;
							if (part_v >= F.p)
								part_v -= F.p;
							acc[q] = (acc[q] & ~(0xFFFFu << sh)) | (part_v << sh);
						} else {
							uint32_t sum = acc[q] + val;
							if (sum < val || sum >= F.p)
								sum -= F.p;
							acc[q] = sum;
						}
					}
			}
		}
		// pivotal entries: their rows of R, tile group by tile group
		const bool piv = v != 0 && cid < (uint32_t) d.r;
		const uint32_t ay = piv ? (PLAIN ? v : montmul(v, F.r2, F)) : 0u;
		todo = __ballot(piv);
		while (todo != 0) {
			const int s0 = __builtin_ctzll(todo);
			todo &= todo - 1;
			int s1 = -1;
			if (todo != 0) {
				s1 = __builtin_ctzll(todo);
				todo &= todo - 1;
			}
			const uint32_t c0 = (uint32_t) __shfl((int) cid, s0), y0 = (uint32_t) __shfl((int) ay, s0);
			const uint32_t *r0 = R + (int64_t) c0 * ldw + w0 + lane;
			uint32_t x0[AP_TU], x1[AP_TU];
			// (signed 16-bit entries are brought back to residues: this kernel runs for a handful of rows)
			auto residues = [&](uint32_t w) -> uint32_t {
				if constexpr (PACKED) {
					if (d.sgn) {
						int l, h;
						sgn_unpack(w, l, h);
						l = (l < 0) ? l + d.G.p : l;
						h = (h < 0) ? h + d.G.p : h;
						return (uint32_t) l | ((uint32_t) h << 16);
					}
				}
				return w;
			};
#pragma unroll
			for (int u = 0; u < AP_TU; u++)
				x0[u] = (w0 + u * 64 < nwords) ? residues(r0[u * 64]) : 0u;
			uint32_t y1 = 0;
			if (s1 >= 0) {
				const uint32_t c1 = (uint32_t) __shfl((int) cid, s1);
				y1 = (uint32_t) __shfl((int) ay, s1);
				const uint32_t *r1 = R + (int64_t) c1 * ldw + w0 + lane;
#pragma unroll
				for (int u = 0; u < AP_TU; u++)
					x1[u] = (w0 + u * 64 < nwords) ? residues(r1[u * 64]) : 0u;
			}
#pragma unroll
			for (int u = 0; u < AP_TU; u++) {
				acc[u] = w_submul<PACKED, PLAIN>(acc[u], x0[u], y0, F, bm);
				if (s1 >= 0)
					acc[u] = w_submul<PACKED, PLAIN>(acc[u], x1[u], y1, F, bm);
			}
		}
	}
#pragma unroll
	for (int u = 0; u < AP_TU; u++)
		part[wave][u * 64 + lane] = acc[u];
	__syncthreads();
	if (wave == 0) {
		uint32_t *out = d.dense_out + (int64_t) k * d.ldS;
#pragma unroll
		for (int u = 0; u < AP_TU; u++) {
			uint32_t lo_s = 0, hi_s = 0;
			for (int w = 0; w < AW_NW; w++) {
				const uint32_t x = part[w][u * 64 + lane];
				if constexpr (PACKED) {
					lo_s += x & 0xFFFFu;
					hi_s += x >> 16;
					if (lo_s >= F.p)
						lo_s -= F.p;
					if (hi_s >= F.p)
						hi_s -= F.p;
				} else {
					const uint32_t sum = lo_s + x;
					lo_s = (sum < x || sum >= F.p) ? sum - F.p : sum;
				}
			}
			const int word = w0 + u * 64 + lane;
			if constexpr (PACKED) {
				if (2 * word < a.Sm)
					out[2 * word] = lo_s;
				if (2 * word + 1 < a.Sm)
					out[2 * word + 1] = hi_s;
			} else {
				if (word < a.Sm)
					out[word] = lo_s;
			}
		}
		if (lane == 0 && blockIdx.x == 0) {
			a.row_len[k] = a.Sm;
			atomicAdd(&a.ctr[a.done_ctr], 1);
			atomicAdd(&a.ctr64[C64_INPUT], (unsigned long long) (hi - lo));
		}
	}
}

template <bool PACKED, bool PLAIN, int LPR, int NW, bool SGN = false, int RING = BS_RING, int PASSROWS = BS_PASSROWS, int PASSCAP = BS_PASSCAP, int WGS_PER_CU = 1>
void launch_backsolve_variant(const BsArgs &b, int Sm, hipStream_t stream, const BsImage &B)
{
	using G = BsGeom<PACKED, LPR, NW, RING, PASSROWS, PASSCAP>;
	if (B.ring != RING || B.passrows != PASSROWS || B.passcap != PASSCAP || B.rstr != G::RSTR)
		die("backsolve: the plan was built for chunks of %d rows, passes of %d rows, %d passes, ring rows %d words apart; this kernel takes %d / %d / %d / %d",
		    B.ring, B.passrows, B.passcap, B.rstr, RING, PASSROWS, PASSCAP, G::RSTR);
	static bool configured = false;
	if (!configured) {
		HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&backsolve_kernel<PACKED, PLAIN, LPR, NW, SGN, RING, PASSROWS, PASSCAP, WGS_PER_CU>),
		                              hipFuncAttributeMaxDynamicSharedMemorySize, (int) G::LDS_BYTES));
		configured = true;
	}
	const int nslabs = (Sm + G::CW - 1) / G::CW;
	hipLaunchKernelGGL((backsolve_kernel<PACKED, PLAIN, LPR, NW, SGN, RING, PASSROWS, PASSCAP, WGS_PER_CU>),
	                   dim3((unsigned) ((nslabs + BS_XCDS - 1) / BS_XCDS * BS_XCDS)), dim3(64 * NW), G::LDS_BYTES, stream, b);
}

template <bool PACKED, bool PLAIN> void launch_apply_variant(const ApplyArgs &d, int blocks, size_t lds, hipStream_t stream)
{
	static size_t configured = 0;
	if (lds > configured) {
		HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&bs_apply_kernel<PACKED, PLAIN>),
		                              hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
		configured = lds;
	}
	hipLaunchKernelGGL((bs_apply_kernel<PACKED, PLAIN>), dim3(blocks), dim3(64 * d.waves), lds, stream, d);
}

}  // namespace

// offsets from row lengths + per-block sums (bs_scan_lengths_kernel), for the other producers of staged rows (sparse_image.hip)
void launch_scan_lengths(const int *len, int n, const unsigned long long *block_sum, int64_t *Sp, int64_t cap, int *ctr, hipStream_t stream)
{
	if (n <= 0)
		return;
	hipLaunchKernelGGL(bs_scan_lengths_kernel, dim3((n + SCAN_BLOCK - 1) / SCAN_BLOCK), dim3(SCAN_BLOCK), 0, stream, len, n, block_sum, Sp, cap, ctr);
}

// --------------------------------------------------------------------------
// host plan
// --------------------------------------------------------------------------
// Is the back-substituted image worth having for this factor?  Memory: r x Sm words.  Work: nnz(U') * Sm.
bool backsolve_eligible(int r, int Sm, int64_t nnz_u, int64_t *bytes, int64_t prime)
{
	const int64_t ldR = ((int64_t) Sm + 511) / 512 * 512;
	*bytes = (int64_t) r * ldR * 4;          // (2 bytes per entry when p < 2^16)
	if (r <= 0 || Sm <= 0)
		return false;
	// the apply kernels keep one row of S in LDS (96 KB); the one for signed 16-bit entries (p <= 44,927) goes through wider
	// rows in segments
	const bool segments = prime < 65536 && sgn_eligible(prime) && env_int("SPASM_HIP_BS_SIGNED", 1) != 0 &&
	                      env_int("SPASM_HIP_BS_STAGED", 1) != 0;
	if (Sm > (segments ? 131072 : 24576))
		return false;
	if ((double) (nnz_u + r) * (double) Sm > 1.5e11)
		return false;
	return true;
}

void backsolve_plan(const FactPlan &P, spasm_hip_dfact *F, hipStream_t stream)
{
	BsImage &B = F->bs;
	const int r = P.r, rpad = P.rpad, m = P.m;
	B.r = r;
	B.Sm = m - r;
	B.ldR = ((int64_t) B.Sm + 511) / 512 * 512;          // whole tile groups of the apply kernels (64 * AP_TU words of two entries): the padding stays zero
	// p < 2^16: coefficients are kept as plain residues (the kernels multiply with 24-bit products + Barrett); small p: signed
	// 16-bit entries of R, coefficients of the dependencies are NEGATED balanced residues (SgnDev above)
	B.plain = P.prime < 65536;
	B.sgn = B.plain && sgn_eligible(P.prime) && env_int("SPASM_HIP_BS_SIGNED", 1) != 0;
	// Shape of the build kernel (the plan is cut for it).  0 = 128-byte slab rows, 16 waves; 1 = 128 B, 8 waves; 2 = 64 B, 8
	// waves; 3 = 32-byte slab rows (16 columns), 8 waves, passes of 64 rows, TWO workgroups per CU.  The build is a chain
	// (DESIGN.md section 5): a workgroup takes the same time whatever the width of its slab, phase A being bound by the
	// instruction issue of ONE CU and phase B by LDS latency; so narrower slabs -- half the phase-A instructions per
	// workgroup, a whole level of up to 64 rows per pass -- and two workgroups sharing a CU, one in its issue-bound phase
	// while the other waits on the LDS, use the chip better as long as all of them are resident at once.
	{
		int cus = 0, dev = 0;
		HIP_CHECK(hipGetDevice(&dev));
		hipDeviceProp_t prop;
		HIP_CHECK(hipGetDeviceProperties(&prop, dev));
		cus = prop.multiProcessorCount;
		const bool packed = P.prime < 65536;
		const int slabs_small = packed ? (B.Sm + 31) / 32 : (B.Sm + 15) / 16;
		int shape = slabs_small <= (packed ? 2 * cus : cus) ? 2 : 0;
		// 4 / 5 = slabs of 10 / 12 words, as many waves as words (every wave ONE word of every row through phase B: passes of 64
		// rows), chunks of 1,260 / 1,200 rows.  A workgroup's time is the vector work of its slab on ONE CU (phases A and B are
		// ~61 and ~45 instructions per row and word) plus ~8,000 cycles of latency per chunk: narrower
		// slabs mean less work per workgroup and more workgroups (207 instead of 155 on mk13.b5, on a chip of 256 CUs), thinner
		// rows put more of them into the same LDS (fewer chunks), and the slab must stay wide enough for every workgroup to
		// have a CU of its own -- 8 words would be 310 workgroups.
		const int words = (B.Sm + 1) / 2;
		// (twelve waves = three per SIMD on all four; ten leave two SIMDs with three and two with two, and the fuller ones set
		//  the pace: 2.18 against 2.26 ms on mk13.b5, 2.66 for the 64-byte slabs of round 2)
		if (B.sgn && (words + 11) / 12 <= cus)
			shape = 5;
		shape = env_int("SPASM_HIP_BS_SHAPE", shape);
		if (shape >= 3 && !B.sgn)
			shape = 2;
		B.shape = shape;
		B.ring = (shape == 4) ? 1260 : (shape == 5) ? 1200 : BS_RING;
		B.passrows = (shape >= 3) ? 64 : BS_PASSROWS;
		B.passcap = (shape == 3) ? 31 : (shape == 4) ? 48 : (shape == 5) ? 44 : BS_PASSCAP;
		// words of a slab row of that kernel (LPR in backsolve_build's table of shapes) + 1: BsGeom::RSTR
		B.rstr = ((shape == 3) ? 8 : (shape == 4) ? 10 : (shape == 5) ? 12 : (shape == 2) ? 16 : 32) + 1;
	}
	const int PLAN_RING = B.ring, PLAN_PASSROWS = B.passrows, PLAN_PASSCAP = B.passcap;
	// rows of the ring go into the tables as word offsets, slot * RSTR, in 16 bits (the spare row included)
	const uint32_t PLAN_RSTR = (uint32_t) B.rstr;
	if ((uint32_t) (PLAN_RING + 1) * PLAN_RSTR > 65535u)
		die("backsolve_plan: a ring of %d + 1 rows, %u words apart: the offset of a row does not fit 16 bits", PLAN_RING, PLAN_RSTR);
	const uint4 PLAN_EMPTY = bs_pass_empty((uint32_t) PLAN_RING * PLAN_RSTR);
	// compact ids: labels that hold a row, in label (= level) order
	std::vector<int> cid((size_t) (rpad > 0 ? rpad : 1), -1);
	std::vector<int> label_of((size_t) (r > 0 ? r : 1), 0);
	{
		int n = 0;
		for (int c = 0; c < rpad; c++)
			if (P.kof[c] >= 0) {
				cid[c] = n;
				label_of[n] = c;
				n += 1;
			}
		if (n != r)
			die("backsolve_plan: %d labelled rows, %d expected", n, r);
	}
	// level of every compact row (levels are consecutive runs of labelled rows)
	std::vector<int> level((size_t) (r > 0 ? r : 1), 0);
	{
		int n = 0;
		for (int l = 0; l < P.nlevels; l++)
			for (int t = 0; t < P.lvl_count[l]; t++)
				level[n++] = l;
	}
	std::vector<int> colmap((size_t) (m > 0 ? m : 1), 0);
	for (int j = 0; j < m; j++)
		colmap[j] = (P.lab[j] < (uint32_t) rpad) ? cid[P.lab[j]] : r + (int) (P.lab[j] - (uint32_t) rpad);

	uint64_t unmont = 1;                 // 2^-32 mod p
	if (B.plain) {
		const uint64_t R1 = (uint64_t) ((1ull << 32) % (uint64_t) P.prime);
		// inverse by Fermat (p is prime in every use; for a composite odd modulus the extended Euclid below still works)
		int64_t t0 = 0, t1 = 1, r0 = P.prime, r1 = (int64_t) R1;
		while (r1 != 0) {
			const int64_t qq = r0 / r1;
			const int64_t t2 = t0 - qq * t1, r2 = r0 - qq * r1;
			t0 = t1;
			t1 = t2;
			r0 = r1;
			r1 = r2;
		}
		if (r0 != 1)
			die("backsolve_plan: 2^32 is not invertible mod %lld", (long long) P.prime);
		unmont = (uint64_t) ((t0 % P.prime + P.prime) % P.prime);
	}
	// (x mod p for x < 2^64 without a division per entry: q = floor(x * floor(2^64 / p) / 2^64) is the quotient or one less)
	const uint64_t pu64 = (uint64_t) P.prime, barrett = ~0ull / pu64;
	auto mod_p = [&](uint64_t x) -> uint32_t {
		uint64_t rem = x - (uint64_t) (((unsigned __int128) x * barrett) >> 64) * pu64;
		while (rem >= pu64)
			rem -= pu64;
		return (uint32_t) rem;
	};
	auto coeff = [&](uint32_t y_mont) -> uint32_t { return B.plain ? mod_p((uint64_t) y_mont * unmont) : y_mont; };
	auto dep_coeff = [&](uint32_t y_mont) -> uint32_t {
		const uint32_t c = coeff(y_mont);
		if (!B.sgn)
			return c;
		const int64_t bal = ((int64_t) c > P.prime / 2) ? (int64_t) c - P.prime : (int64_t) c;
		return (uint32_t) (int32_t) (-bal);
	};
	double t_mark = wtime();
	auto lap = [&](const char *what) {
		if (verbose() >= 3)
			logmsg("[factor image/back-substitution plan] %s %.2f ms\n", what, 1e3 * (wtime() - t_mark));
		t_mark = wtime();
	};
	// split every row into pivotal dependencies (compact ids) and non-pivotal entries: counted, then filled, by a few threads
	// (the entries of boundary matrices are +-1: their Montgomery forms are recognised, no reduction)
	std::vector<uint64_t> dep_rp((size_t) r + 1, 0), np_rp((size_t) r + 1, 0);
	std::vector<uint2> dep, np;
	std::vector<int> np_row;
	{
		const int T = (r < 50000) ? 1 : std::max(1, std::min(8, usable_cpus()));
		auto for_rows = [&](auto &&body) { sh::pool_run(T, [&](int t) { body((int) ((int64_t) r * t / T), (int) ((int64_t) r * (t + 1) / T)); }); };
		for_rows([&](int n_lo, int n_hi) {
			for (int n = n_lo; n < n_hi; n++) {
				const int c = label_of[n];
				uint64_t nd = 0;
				for (uint64_t e = P.rp[c]; e < P.rp[c + 1]; e++)
					nd += P.ent[e].x < (uint32_t) rpad;
				dep_rp[n + 1] = nd;
				np_rp[n + 1] = (P.rp[c + 1] - P.rp[c]) - nd;
			}
		});
		for (int n = 0; n < r; n++) {
			dep_rp[n + 1] += dep_rp[n];
			np_rp[n + 1] += np_rp[n];
		}
		dep.resize((size_t) dep_rp[r]);
		np.resize((size_t) np_rp[r]);
		np_row.resize((size_t) np_rp[r]);
		const uint32_t mont_one = (uint32_t) ((1ull << 32) % (uint64_t) P.prime), mont_minus_one = (uint32_t) ((uint64_t) P.prime - mont_one);
		const uint32_t one_c = coeff(mont_one), minus_c = coeff(mont_minus_one), one_d = dep_coeff(mont_one), minus_d = dep_coeff(mont_minus_one);
		for_rows([&](int n_lo, int n_hi) {
			for (int n = n_lo; n < n_hi; n++) {
				const int c = label_of[n];
				uint64_t wd = dep_rp[n], wn = np_rp[n];
				for (uint64_t e = P.rp[c]; e < P.rp[c + 1]; e++) {
					const uint2 en = P.ent[e];
					if (en.x < (uint32_t) rpad) {
						dep[wd++] = uint2{(uint32_t) cid[en.x], en.y == mont_one ? one_d : en.y == mont_minus_one ? minus_d : dep_coeff(en.y)};
					} else {
						np[wn] = uint2{en.x - (uint32_t) rpad, en.y == mont_one ? one_c : en.y == mont_minus_one ? minus_c : coeff(en.y)};
						np_row[wn] = n;
						wn += 1;
					}
				}
			}
		});
	}

	lap("dependencies / non-pivotal entries");
	// chunks, from the last row to the first
	std::vector<BsChunk> chunks;
	std::vector<int> chunk_extra;
	std::vector<int> chunk_long;          // per chunk: passes of rows with more than two dependencies inside it
	std::vector<uint4> ptab;
	std::vector<uint2> near;
	// rows of R go to the kernel as offsets, row * (words of a row / 256): see backsolve_kernel
	const uint32_t ldw256 = (uint32_t) ((B.ldR / (P.prime < 65536 ? 2 : 1)) >> 8);
	if ((uint64_t) (r > 0 ? r : 1) * ldw256 >= (uint64_t) BS_NONE)
		die("backsolve_plan: %d rows of %lld columns: the offset of a row does not fit 32 bits", r, (long long) B.ldR);
	auto make_head = [&](uint32_t off0, uint32_t c0, uint32_t off1, uint32_t c1) { return B.plain ? bs_head<true>(off0, c0, off1, c1) : bs_head<false>(off0, c0, off1, c1); };
	std::vector<uint4> far_head((size_t) (r > 0 ? r : 1), make_head(BS_NONE, 0u, BS_NONE, 0u));
	std::vector<uint64_t> far_rp((size_t) r + 1, 0);
	std::vector<uint2> far;
	std::vector<uint64_t> far_cnt((size_t) (r > 0 ? r : 1), 0);
	// first pass: chunk boundaries (a chunk grows downwards while its rows, the passes of its rows that have
	// dependencies inside the chunk -- 32 rows of one level each -- and the dependencies beyond the second fit the LDS
	// arrays of the kernel)
	int hi = r;
	while (hi > 0) {
		BsChunk ch{};
		ch.hi = hi;
		int lo = hi, nnear = 0, npass = 0, in_level[2] = {0, 0}, last_level = -1;          // (in_level: ordinary rows, long rows)
		while (lo > 0 && hi - lo < PLAN_RING) {
			const int c = lo - 1;
			int nc = 0;
			for (uint64_t e = dep_rp[c]; e < dep_rp[c + 1]; e++)
				nc += dep[e].x < (uint32_t) hi;
			// rows with more than two dependencies inside the chunk (long rows) have passes of their own, behind their level's others
			const int kind = nc > 2 ? 1 : 0;
			if (nc > 0 && level[c] != last_level)
				in_level[0] = in_level[1] = 0;
			const bool new_pass = nc > 0 && in_level[kind] % PLAN_PASSROWS == 0;
			const int extra = nc > 2 ? nc - 1 : 0;
			if (nnear + extra > BS_NEARCAP || nc > 65535 || (new_pass && npass + 1 > PLAN_PASSCAP))
				break;                           // (the first row of a chunk never has dependencies inside it)
			if (nc > 0) {
				npass += new_pass ? 1 : 0;
				in_level[kind] += 1;
				last_level = level[c];
				nnear += extra;
			}
			lo = c;
		}
		ch.lo = lo;
		ch.npass = (unsigned short) npass;          // (<= PLAN_PASSCAP)
		ch.nnear = nnear;
		chunks.push_back(ch);
		chunk_extra.push_back(0);
		hi = lo;
	}
	// second pass: the tables of every chunk, slots relative to its first row.  The first pass has counted the passes and the list
	// entries of every chunk: the tables are sized at once (empty table slots are what the padding of a pass is) and the chunks
	// filled by a few threads, each at its own place (4.1 of the 7.2 ms of mk13.b5's image went into this loop and its push_backs).
	{
		int64_t total_pass = 0, total_near = 0;
		for (BsChunk &ch : chunks) {
			ch.pass0 = (int) total_pass;
			ch.near0 = (int) total_near;
			total_pass += ch.npass;
			total_near += ch.nnear;
		}
		ptab.assign((size_t) total_pass * (size_t) PLAN_PASSROWS, PLAN_EMPTY);
		chunk_long.assign(chunks.size(), 0);
		near.assign((size_t) total_near, uint2{0u, 0u});
		auto fill_chunk = [&](size_t k) {
			BsChunk &ch = chunks[k];
			const size_t pt_end = (size_t) (ch.pass0 + ch.npass) * (size_t) PLAN_PASSROWS;
			size_t pt = (size_t) ch.pass0 * (size_t) PLAN_PASSROWS;          // next slot of the table of passes
			int nn = 0;                                                       // list entries of the chunk so far
			int extra = 0;
			std::vector<int> rows[2];          // rows of the level at hand with dependencies inside the chunk: ordinary, long
			std::vector<int> long_at;          // the passes of long rows, counted from the chunk's first pass
			auto off = [&](uint32_t row) -> uint32_t { return (row - (uint32_t) ch.lo) * PLAN_RSTR; };          // offset in the ring
			auto put = [&](int c, bool is_long) {
				int nc = 0;
				for (uint64_t e = dep_rp[c]; e < dep_rp[c + 1]; e++)
					nc += dep[e].x < (uint32_t) ch.hi;
				uint4 en{off((uint32_t) c) | (is_long ? (uint32_t) nc << 16 : 0u), 0u, 0u, 0u};
				int seen = 0;
				for (uint64_t e = dep_rp[c]; e < dep_rp[c + 1]; e++) {
					if (dep[e].x >= (uint32_t) ch.hi)
						continue;
					const uint32_t at = off(dep[e].x);
					if (seen == 0) {
						en.y = is_long ? at : at | (at << 16);          // (one dependency: the second slot repeats it with coefficient 0)
						en.z = B.plain ? (dep[e].y & 0xFFFFu) : dep[e].y;
						if (is_long)
							en.w = (uint32_t) nn;
					} else if (!is_long) {
						en.y = (en.y & 0xFFFFu) | (at << 16);
						if (B.plain)
							en.z |= dep[e].y << 16;
						else
							en.w = dep[e].y;
					} else {
						if (nn >= ch.nnear)
							die("backsolve_plan: chunk %zu holds more list entries than the %d counted", k, ch.nnear);
						near[(size_t) ch.near0 + (size_t) nn] = uint2{at, dep[e].y};
						nn += 1;
					}
					seen += 1;
				}
				if (pt >= pt_end)
					die("backsolve_plan: chunk %zu needs more than the %d passes counted", k, (int) ch.npass);
				ptab[pt++] = en;
			};
			for (int c = ch.hi - 1; c >= ch.lo;) {
				const int lvl = level[c];
				rows[0].clear();
				rows[1].clear();
				for (; c >= ch.lo && level[c] == lvl; c--) {
					int nc = 0, nf = 0;
					uint2 first[2] = {uint2{BS_NONE, 0u}, uint2{BS_NONE, 0u}};
					for (uint64_t e = dep_rp[c]; e < dep_rp[c + 1]; e++) {
						if (dep[e].x < (uint32_t) ch.hi) {
							nc += 1;
						} else {
							if (nf < 2) {
								first[nf] = uint2{dep[e].x * ldw256, dep[e].y};
							} else {
								far_cnt[c] += 1;
								extra = 1;
							}
							nf += 1;
						}
					}
					if (nf > 0)
						far_head[c] = make_head(first[0].x, first[0].y, first[1].x, first[1].y);
					if (nc > 0)
						rows[nc > 2 ? 1 : 0].push_back(c);
				}
				// the ordinary rows of the level, then its long rows: each kind starts a pass, the rest of the one before stays empty
				for (int kind = 0; kind < 2; kind++)
					for (size_t q = 0; q < rows[kind].size(); q++) {
						if (q % (size_t) PLAN_PASSROWS == 0) {
							pt = (pt + (size_t) PLAN_PASSROWS - 1) / (size_t) PLAN_PASSROWS * (size_t) PLAN_PASSROWS;
							if (kind == 1)
								long_at.push_back((int) (pt / (size_t) PLAN_PASSROWS) - ch.pass0);
						}
						put(rows[kind][q], kind == 1);
					}
			}
			const int passes = (int) ((pt + (size_t) PLAN_PASSROWS - 1) / (size_t) PLAN_PASSROWS) - ch.pass0;
			if (passes != ch.npass || nn != ch.nnear)
				die("backsolve_plan: chunk %zu was counted differently on the second pass (%d passes against %d, %d list entries against %d)", k, passes,
				    (int) ch.npass, nn, ch.nnear);
			// where the long passes are: the descriptor leads to the first, every slot of a long pass (.y, high half) to the next
			ch.nord = long_at.empty() ? ch.npass : (unsigned short) long_at[0];
			for (size_t q = 0; q < long_at.size(); q++) {
				const uint32_t ordinary_after = (uint32_t) ((q + 1 < long_at.size() ? long_at[q + 1] : (int) ch.npass) - long_at[q] - 1);
				uint4 *pass = &ptab[(size_t) (ch.pass0 + long_at[q]) * (size_t) PLAN_PASSROWS];
				for (int t = 0; t < PLAN_PASSROWS; t++)
					pass[t].y = (pass[t].y & 0xFFFFu) | (ordinary_after << 16);
			}
			chunk_long[k] = (int) long_at.size();
			chunk_extra[k] = extra;
			// everything the kernel needs to start a chunk sits in its descriptor (no dependent loads at the top of a chunk)
			ch.np0 = (int) std::min<uint64_t>(np_rp[ch.lo], 0x7FFFFFFFull);
			ch.npn = (int) std::min<uint64_t>(np_rp[ch.hi] - np_rp[ch.lo], 0x7FFFFFFFull) | (extra ? (int) 0x80000000u : 0);
		};
		sh::pool_run((int) chunks.size(), [&](int k) { fill_chunk((size_t) k); });
	}
	if (np.size() >= 0x7FFFFFFFull)
		die("backsolve_plan: %zu non-pivotal entries in the factor (the chunk descriptors index them with 31 bits)", np.size());
	// dependencies beyond the first two outside the chunk, CSR by row
	for (int c = 0; c < r; c++)
		far_rp[c + 1] = far_rp[c] + far_cnt[c];
	far.assign((size_t) (far_rp[r] > 0 ? far_rp[r] : 1), uint2{0, 0});
	{
		// chunk of a row: chunks are stored from the last rows to the first
		std::vector<int> chunk_hi((size_t) (r > 0 ? r : 1), 0);
		for (size_t k = 0; k < chunks.size(); k++)
			for (int c = chunks[k].lo; c < chunks[k].hi; c++)
				chunk_hi[c] = chunks[k].hi;
		for (int c = 0; c < r; c++) {
			if (far_cnt[c] == 0)
				continue;
			uint64_t w = far_rp[c];
			int nf = 0;
			for (uint64_t e = dep_rp[c]; e < dep_rp[c + 1]; e++)
				if (dep[e].x >= (uint32_t) chunk_hi[c]) {
					if (nf >= 2)
						far[w++] = uint2{dep[e].x * ldw256, dep[e].y};
					nf += 1;
				}
		}
	}

	lap("chunks, passes, near and far tables");
	if (verbose() >= 3) {
		// how full the passes of phase B are (an empty slot costs a lane what a row does), and why: the widths of the levels
		int64_t passes = 0, used = 0, long_passes = 0;
		for (const BsChunk &ch : chunks)
			passes += ch.npass;
		for (const int n : chunk_long)
			long_passes += n;
		for (const uint4 &en : ptab)
			used += en.z != 0u;          // (a row in the table has a first coefficient; entries of U are not 0)
		logmsg("[factor image/back-substitution plan] shape %d: %zu chunks of <= %d rows, %lld passes of %d slots, %lld of them of long rows (more than two "
		       "dependencies inside the chunk), %lld of %lld slots occupied (%.1f%%), %d rows in %d levels\n", B.shape, chunks.size(), PLAN_RING,
		       (long long) passes, PLAN_PASSROWS, (long long) long_passes, (long long) used, (long long) passes * PLAN_PASSROWS,
		       passes > 0 ? 100.0 * (double) used / (double) (passes * PLAN_PASSROWS) : 0.0, r, P.nlevels);
		int64_t hist_levels[32] = {0}, hist_rows[32] = {0};          // bucket b: widths in (2^(b-1), 2^b]
		for (int l = 0; l < P.nlevels; l++) {
			const int w = P.lvl_count[l];
			if (w <= 0)
				continue;
			int bkt = 0;
			while ((1ll << bkt) < w)
				bkt += 1;
			hist_levels[bkt] += 1;
			hist_rows[bkt] += w;
		}
		for (int bkt = 0; bkt < 32; bkt++)
			if (hist_levels[bkt] > 0)
				logmsg("[factor image/back-substitution plan]   levels of %lld..%lld rows: %lld levels, %lld rows\n", bkt == 0 ? 1ll : (1ll << (bkt - 1)) + 1,
				       1ll << bkt, (long long) hist_levels[bkt], (long long) hist_rows[bkt]);
	}
	B.nchunks = (int) chunks.size();
	B.nnear = (int64_t) near.size();
	B.nfar = (int64_t) far_rp[r];
	B.nnp = (int64_t) np.size();
	B.ndeps = (int64_t) dep.size();
	B.d_col = dalloc<int>(m);
	B.d_chunk = dalloc<BsChunk>((int64_t) chunks.size());
	B.d_ptab = dalloc<uint4>((int64_t) ptab.size());
	B.d_near = dalloc<uint2>((int64_t) near.size());
	B.d_far_head = dalloc<uint4>(r);
	B.d_far_rp = dalloc<uint64_t>((int64_t) r + 1);
	B.d_far = dalloc<uint2>((int64_t) far.size());
	B.d_np_rp = dalloc<uint64_t>((int64_t) r + 1);
	B.d_np = dalloc<uint2>((int64_t) np.size());
	B.d_np_row = dalloc<int>((int64_t) np_row.size());
	B.d_chunk_extra = dalloc<int>((int64_t) chunk_extra.size());
	lap("device buffers");
	upload(B.d_col, colmap, stream);
	upload(B.d_chunk, chunks, stream);
	upload(B.d_chunk_extra, chunk_extra, stream);
	upload(B.d_ptab, ptab, stream);
	upload(B.d_near, near, stream);
	upload(B.d_far_head, far_head, stream);
	upload(B.d_far_rp, far_rp, stream);
	upload(B.d_far, far, stream);
	upload(B.d_np_rp, np_rp, stream);
	upload(B.d_np, np, stream);
	upload(B.d_np_row, np_row, stream);
	HIP_CHECK(hipStreamSynchronize(stream));      // the host vectors die here
	lap("uploads");
	B.planned = true;
	B.valid = false;
}

void backsolve_free(spasm_hip_dfact *F)
{
	BsImage &B = F->bs;
	big_free(B.d_R);
	sh::big_free(B.d_col);
	sh::big_free(B.d_chunk);
	sh::big_free(B.d_chunk_extra);
	sh::big_free(B.d_ptab);
	sh::big_free(B.d_near);
	sh::big_free(B.d_far_head);
	sh::big_free(B.d_far_rp);
	sh::big_free(B.d_far);
	sh::big_free(B.d_np_rp);
	sh::big_free(B.d_np);
	sh::big_free(B.d_np_row);
	if (B.ev0 != nullptr)
		(void) hipEventDestroy(B.ev0);
	if (B.ev1 != nullptr)
		(void) hipEventDestroy(B.ev1);
	B = BsImage{};
}

// (re)computes R on `stream`.  The caller synchronises before reading the events.
void backsolve_build(const spasm_hip_dfact *F, hipStream_t stream)
{
	BsImage &B = F->bs;
	if (!B.planned && F->bs_deferred && F->host_plan) {
		// (a factor with the tables of the sparse image: the plan of the dense one was left for the batch that wants it)
		backsolve_plan(*F->host_plan, const_cast<spasm_hip_dfact *>(F), stream);
		F->bs_deferred = false;
	}
	if (!B.planned)
		die("backsolve_build: the factor has no back-substitution plan");
	// R is stored in 16 bits when the prime allows (42013, the reference's default, does): half the traffic, half the LDS
	const bool packed = F->prime < 65536;
	const int elem = packed ? 2 : 4;
	const size_t bytes = (size_t) B.r * (size_t) B.ldR * (size_t) elem;
	if (B.d_R != nullptr && B.elem_bytes != elem) {
		big_free(B.d_R);
		B.d_R = nullptr;
	}
	bool fresh = false;
	if (B.d_R == nullptr) {
		B.d_R = big_alloc(bytes);          // (from the block cache: tens of GB on a wide factor)
		B.elem_bytes = elem;
		fresh = true;
	}
	if (B.ev0 == nullptr) {
		HIP_CHECK(hipEventCreate(&B.ev0));
		HIP_CHECK(hipEventCreate(&B.ev1));
	}
	BsArgs b{};
	b.R = B.d_R;
	b.ldR = B.ldR;
	b.nchunks = B.nchunks;
	b.chunk = B.d_chunk;
	b.chunk_extra = B.d_chunk_extra;
	b.ptab = B.d_ptab;
	b.near = B.d_near;
	b.far_head = B.d_far_head;
	b.far_rp = B.d_far_rp;
	b.far = B.d_far;
	b.np_rp = B.d_np_rp;
	b.np = B.d_np;
	b.np_row = B.d_np_row;
	b.r = B.r;
	b.Sm = B.Sm;
	b.plain = B.plain ? 1 : 0;
	b.sgn = B.sgn ? 1 : 0;
	b.G = sgn_setup(F->prime);
	b.F = to_dev(F->mont);
	b.prof = nullptr;
	if (env_int("SPASM_HIP_BS_PROFILE", 0)) {
		b.prof = dalloc<unsigned long long>(8);
		HIP_CHECK(hipMemsetAsync(b.prof, 0, 8 * sizeof(unsigned long long), stream));
	}
	// few non-pivotal entries per row of U (mk13.b5: 0.08): the kernel scatters them into its LDS ring itself and R is
	// neither zeroed nor read for them; many (factors that already hold dense rows): R is pre-filled instead
	b.sparse_init = (B.nnp <= 4 * (int64_t) B.r && env_int("SPASM_HIP_BS_SPARSE_INIT", 1) != 0) ? 1 : 0;
	HIP_CHECK(hipEventRecord(B.ev0, stream));
	if (fresh || !b.sparse_init)        // (the padding columns beyond the last slab must be zero: once is enough for them)
		HIP_CHECK(hipMemsetAsync(B.d_R, 0, bytes, stream));
	if (!b.sparse_init) {
		if (packed)
			hipLaunchKernelGGL(bs_init_kernel<uint16_t>, dim3((B.r + 255) / 256), dim3(256), 0, stream, b);
		else
			hipLaunchKernelGGL(bs_init_kernel<uint32_t>, dim3((B.r + 255) / 256), dim3(256), 0, stream, b);
	}
	// shape of a workgroup: 0 = 128-byte slab rows, 16 waves; 1 = 128 B, 8 waves; 2 = 64 B, 8 waves.  The chain of levels
	// (phase B) is bound by instruction issue -- every wave runs every step -- so the small workgroup wins while all its
	// slabs are resident at once (mk13.b5: 4.4 against 4.9 ms); with more slabs than that, whole cache lines per request
	// matter more (phase A is bound by the rate of memory requests)
	const int shape = B.shape;
	if (shape == 3)
		snprintf(B.kernel_build, sizeof(B.kernel_build), "backsolve_kernel<true,true,8,8,true,768,64,31,2>");
	else if (shape == 4)
		snprintf(B.kernel_build, sizeof(B.kernel_build), "backsolve_kernel<true,true,10,10,true,1260,64,48,1>");
	else if (shape == 5)
		snprintf(B.kernel_build, sizeof(B.kernel_build), "backsolve_kernel<true,true,12,12,true,1200,64,44,1>");
	else
		snprintf(B.kernel_build, sizeof(B.kernel_build), "backsolve_kernel<%s,%s,%d,%d,%s,%d,%d,%d,1>", packed ? "true" : "false", B.plain ? "true" : "false",
		         shape == 2 ? 16 : 32, (shape == 0 || (!packed && B.plain && shape == 1)) ? 16 : 8, B.sgn ? "true" : "false", BS_RING, BS_PASSROWS,
		         BS_PASSCAP);          // (as rocprofv3 prints it: bench.py looks the counters of the profile passes up by this name)
	if (B.sgn) {
		if (shape == 3)
			launch_backsolve_variant<true, true, 8, 8, true, 768, 64, 31, 2>(b, B.Sm, stream, B);
		else if (shape == 4)
			launch_backsolve_variant<true, true, 10, 10, true, 1260, 64, 48, 1>(b, B.Sm, stream, B);
		else if (shape == 5)
			launch_backsolve_variant<true, true, 12, 12, true, 1200, 64, 44, 1>(b, B.Sm, stream, B);
		else if (shape == 1)
			launch_backsolve_variant<true, true, 32, 8, true>(b, B.Sm, stream, B);
		else if (shape == 2)
			launch_backsolve_variant<true, true, 16, 8, true>(b, B.Sm, stream, B);
		else
			launch_backsolve_variant<true, true, 32, 16, true>(b, B.Sm, stream, B);
	} else if (packed) {
		if (shape == 1)
			launch_backsolve_variant<true, true, 32, 8>(b, B.Sm, stream, B);
		else if (shape == 2)
			launch_backsolve_variant<true, true, 16, 8>(b, B.Sm, stream, B);
		else
			launch_backsolve_variant<true, true, 32, 16>(b, B.Sm, stream, B);
	} else if (B.plain) {          // (p < 2^16 with 32-bit entries of R: no plan asks for them, every p < 2^16 is packed)
		if (shape == 2)
			launch_backsolve_variant<false, true, 16, 8>(b, B.Sm, stream, B);
		else
			launch_backsolve_variant<false, true, 32, 16>(b, B.Sm, stream, B);
	} else {
		if (shape == 1)
			launch_backsolve_variant<false, false, 32, 8>(b, B.Sm, stream, B);
		else if (shape == 2)
			launch_backsolve_variant<false, false, 16, 8>(b, B.Sm, stream, B);
		else
			launch_backsolve_variant<false, false, 32, 16>(b, B.Sm, stream, B);
	}
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(B.ev1, stream));
	B.valid = true;
	B.builds += 1;
	if (b.prof != nullptr) {
		unsigned long long h[8];
		HIP_CHECK(hipMemcpyAsync(h, b.prof, sizeof(h), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipStreamSynchronize(stream));
		static const char *const stage[7] = {"descriptor + metadata issue", "phase A", "non-pivotal entries added", "long outside lists", "phase B", "phase C (issue)",
		                                     "metadata into LDS + barrier"};
		unsigned long long tot = 0;
		for (int q = 0; q < 7; q++)
			tot += h[q];
		fprintf(stderr, "[bs profile] %s, %d chunks, workgroup 0, shader-clock cycles per chunk:", B.kernel_build, B.nchunks);
		for (int q = 0; q < 7; q++)
			fprintf(stderr, " %s %.0f (%.0f%%);", stage[q], (double) h[q] / B.nchunks, 100.0 * (double) h[q] / (double) (tot ? tot : 1));
		fprintf(stderr, " total %.0f\n", (double) tot / B.nchunks);
		sh::big_free(b.prof);
	}
}

// staged sparse output available for this factor?  *row_bytes = size of one packed row of the staging buffer
bool backsolve_stages_output(const spasm_hip_dfact *F, int64_t *row_bytes)
{
	const BsImage &B = F->bs;
	*row_bytes = B.ldR * (B.valid ? B.elem_bytes : 4);          // (asked after the build: the entry size is known)
	return B.planned && env_int("SPASM_HIP_BS_STAGED", 1) != 0;
}

// bytes of LDS a wave of bs_apply_s16_csr_kernel needs: the list / compaction area and its row buffers (two with PendingLds,
// one beside the register file of PendingRegs)
static size_t csr_wave_bytes(int64_t ldR, int buffers)
{
	return (size_t) CSR_SCRATCH_BYTES + (size_t) buffers * (size_t) ldR * 2;
}

// 64-word tiles of a row when the batch goes to PendingRegs; 0: rows wider than its widest instantiation, or
// SPASM_HIP_BS_CSR_ROWREG=0 (A/B runs, tests): PendingLds
static int csr_rowreg_tiles(int64_t ldR)
{
	if (ldR > 128 * CSR_ROWREG_MAX_TILES || env_int("SPASM_HIP_BS_CSR_ROWREG", 1) == 0)
		return 0;
	return (int) (ldR / 128);
}

using CsrKernel = void (*)(ApplyArgs);
static CsrKernel csr_kernel(int tiles)
{
	switch (tiles) {
	case 0: return bs_apply_s16_csr_kernel<PendingLds, true, 0>;
#define ROWREG_CASE(NT) case NT: return bs_apply_s16_csr_kernel<PendingRegs<NT>, CSR_ROWREG_DEEP, CSR_ROWREG_WPE>;
	ROWREG_CASE(4) ROWREG_CASE(8) ROWREG_CASE(12) ROWREG_CASE(16) ROWREG_CASE(20)
	ROWREG_CASE(24) ROWREG_CASE(28) ROWREG_CASE(32) ROWREG_CASE(36) ROWREG_CASE(40)
#undef ROWREG_CASE
	}
	die("launch_backsolve_apply: no CSR-output kernel for rows of %d tiles", tiles);
	return nullptr;
}

// The staged output of a batch replaced by the CSR-output kernels (rows of S straight to Sj / Sx)?  Signed 16-bit entries,
// rows of one segment (<= 24,576 columns), the whole batch in one slice of the staging buffer, the row buffers of a wave within
// what a workgroup may have.  SPASM_HIP_BS_CSR=0 keeps the staged kernels (A/B runs, tests).
bool backsolve_output_csr(const spasm_hip_dfact *F, int64_t nrows, int64_t stage_rows)
{
	const BsImage &B = F->bs;
	if (!B.valid || !B.sgn || B.ldR > 24576 || stage_rows < nrows || env_int("SPASM_HIP_BS_CSR", 1) == 0)
		return false;
	int dev = 0, per_block = 0;
	HIP_CHECK(hipGetDevice(&dev));
	HIP_CHECK(hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
	return csr_wave_bytes(B.ldR, csr_rowreg_tiles(B.ldR) > 0 ? 1 : 2) <= (size_t) per_block;
}

// S rows from R: sparse rows into the pool of `a` (dense_out == nullptr) or dense rows.
void launch_backsolve_apply(const SchurArgs &a, const spasm_hip_dfact *F, uint32_t *dense_out, int64_t ldS, hipStream_t stream,
                            BsDirectOut *direct)
{
	const BsImage &B = F->bs;
	if (!B.valid)
		die("launch_backsolve_apply: R has not been built");
	ApplyArgs d{};
	d.a = a;
	d.R = B.d_R;
	d.ldR = B.ldR;
	d.col = B.d_col;
	d.r = B.r;
	static_assert(2 * 64 * AP_TU == 512, "ldR is padded to whole tile groups of the apply kernels");
	d.Smpad = (int) B.ldR;
	d.dense_out = dense_out;
	d.ldS = ldS;
	d.sgn = B.sgn ? 1 : 0;
	d.G = sgn_setup(F->prime);
	if (direct != nullptr && dense_out == nullptr) {
		d.direct = 1;
		d.status = direct->status;
		d.ticket = direct->ticket;
		d.Sp = direct->Sp;
		d.Sj = direct->Sj;
		d.Sx = direct->Sx;
		d.cap = direct->cap;
	}
	const bool packed = B.elem_bytes == 2;
	int dev = 0;
	HIP_CHECK(hipGetDevice(&dev));
	hipDeviceProp_t prop;
	HIP_CHECK(hipGetDeviceProperties(&prop, dev));
	// few long rows asked for as dense rows (the completion test: combinations of every remaining row): workgroups split
	// the columns AND the entries of a row; otherwise one wave per row
	if (dense_out != nullptr && a.nrows > 0 && a.nrows < prop.multiProcessorCount && a.avg_row_entries >= 1024) {
		const int nwords = d.Smpad / (packed ? 2 : 1);
		const dim3 grid((unsigned) ((nwords + 64 * AP_TU - 1) / (64 * AP_TU)), (unsigned) a.nrows);
		if (packed)
			hipLaunchKernelGGL((bs_apply_wide_kernel<true, true>), grid, dim3(64 * AW_NW), 0, stream, d);
		else if (B.plain)
			hipLaunchKernelGGL((bs_apply_wide_kernel<false, true>), grid, dim3(64 * AW_NW), 0, stream, d);
		else
			hipLaunchKernelGGL((bs_apply_wide_kernel<false, false>), grid, dim3(64 * AW_NW), 0, stream, d);
		HIP_CHECK(hipGetLastError());
		return;
	}
	if (direct != nullptr && direct->csr && dense_out == nullptr) {
		// rows of S straight to Sj / Sx: the older pending row of a wave in registers (rows of up to 5,120 columns), or both in LDS
		const int tiles = csr_rowreg_tiles(B.ldR);
		const CsrKernel kernel = csr_kernel(tiles);
		const size_t per_wave = csr_wave_bytes(B.ldR, tiles > 0 ? 1 : 2);
		int per_block = 0;
		HIP_CHECK(hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
		const int max_waves = (int) std::min<size_t>(8, (size_t) per_block / per_wave);
		// (set at every launch: the attribute belongs to the device the call runs on, and a process may drive several)
		HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
		                              (int) (per_wave * (size_t) max_waves)));
		// Workgroup shape: the one that puts the most waves on a CU, the larger workgroup on a tie.  What a CU holds is asked of
		// the kernel that is launched, with its LDS (160 KB per CU) and its registers.  A row's offset waits for the lengths of
		// rows that other workgroups hold: every workgroup of the grid must be resident, so this figure also bounds the grid.
		int waves = 1, per_cu = 0;
		for (int w = 1; w <= max_waves; w++) {
			const size_t lds_w = per_wave * (size_t) w;
			int fit = 0;
			HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, 64 * w, lds_w));
			fit = std::min(fit, (int) ((size_t) (160 * 1024) / lds_w));
			if (fit * w >= per_cu * waves) {
				per_cu = fit;
				waves = w;
			}
		}
		d.waves = waves;
		d.wave_bytes = per_wave;
		d.seg_words = d.Smpad / 2;
		const size_t lds = per_wave * (size_t) waves;
		if (per_cu < 1)
			die("launch_backsolve_apply: %zu bytes of LDS per workgroup leave no room for the CSR output", lds);
		const int blocks = std::max(1, std::min((a.nrows + waves - 1) / waves, prop.multiProcessorCount * per_cu));
		d.ntickets = std::min(LB_TICKETS, blocks);
		direct->csr_tiles = tiles;
		if (verbose() >= 3)
			logmsg("[dense image] CSR output (%s): %d workgroups of %d waves, %zu bytes of LDS each, %d per CU\n",
			       tiles > 0 ? "pending row in registers" : "two row buffers", blocks, waves, lds, per_cu);
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * waves), lds, stream, d);
		HIP_CHECK(hipGetLastError());
		return;
	}
	// rows of more than 24,576 columns are produced in segments of 8,192 columns (signed 16-bit entries, staged or dense
	// output): 16.5 KB of LDS per wave, eight waves per CU, where the whole row would leave one wave per CU
	const bool staged_call = direct != nullptr && direct->stage != nullptr && dense_out == nullptr;
	int seg_cols = d.Smpad;
	if (B.sgn && d.Smpad > 24576 && (staged_call || dense_out != nullptr))
		seg_cols = 8192;
	d.seg_words = seg_cols / 2;
	const size_t per_wave = ((size_t) seg_cols * (size_t) B.elem_bytes + (size_t) AP_LIST * sizeof(uint2) + 15) / 16 * 16;
	if (per_wave > 150 * 1024)
		die("launch_backsolve_apply: %d non-pivotal columns do not fit the LDS row buffer", B.Sm);
	// as many waves as fit half of a CU's LDS (two workgroups per CU), at most 8, at least 1
	const int waves = (int) std::max<size_t>(1, std::min<size_t>(8, (size_t) (76 * 1024) / per_wave));
	d.waves = waves;
	d.wave_bytes = per_wave;
	const size_t lds = per_wave * (size_t) waves;
	int blocks = std::max(1, std::min((a.nrows + waves - 1) / waves, prop.multiProcessorCount * 8));
	if (d.direct) {
		// look-back output: a row waits for rows held by OTHER workgroups, so every workgroup of the grid must be resident
		// (a workgroup that has not started cannot publish the lengths its ticket class owes): at most what the LDS of the
		// chip holds at once
		const int per_cu = (int) std::max<size_t>(1, (size_t) (160 * 1024) / std::max<size_t>(lds, 1));
		blocks = std::min(blocks, prop.multiProcessorCount * per_cu);
	}
	d.ntickets = std::min(LB_TICKETS, blocks);
	// one launch of the apply kernel that fits the arithmetic of R
	auto launch_apply = [&](const ApplyArgs &dd, int nblocks_apply) {
		if (B.sgn) {
			static size_t configured = 0;
			if (lds > configured) {
				HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&bs_apply_s16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
				configured = lds;
			}
			hipLaunchKernelGGL(bs_apply_s16_kernel, dim3(nblocks_apply), dim3(64 * dd.waves), lds, stream, dd);
		} else if (packed) {
			launch_apply_variant<true, true>(dd, nblocks_apply, lds, stream);
		} else if (B.plain) {
			launch_apply_variant<false, true>(dd, nblocks_apply, lds, stream);
		} else {
			launch_apply_variant<false, false>(dd, nblocks_apply, lds, stream);
		}
	};
	if (direct != nullptr && direct->stage != nullptr && dense_out == nullptr) {
		// staged output: rows as they stand + lengths, offsets by a scan, sparse rows by a streaming kernel; slices of
		// stage_rows rows when the staging buffer is smaller than the batch
		const int nwords = d.Smpad / (packed ? 2 : 1);
		HIP_CHECK(hipMemsetAsync(direct->Sp, 0, sizeof(int64_t), stream));
		auto expand_slice = [&](int64_t r0, int n, const uint32_t *stage, const unsigned long long *block_sum, hipStream_t s2) {
			const int nblocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
			hipLaunchKernelGGL(bs_scan_lengths_kernel, dim3(nblocks), dim3(SCAN_BLOCK), 0, s2, a.row_len + r0, n, block_sum, direct->Sp + r0, direct->cap, a.ctr);
			ExpandArgs e{stage, nwords, n, direct->Sp + r0, direct->Sj, direct->Sx, direct->cap, a.q, d.G};
			const int blocks3 = std::max(1, std::min((n + 3) / 4, prop.multiProcessorCount * 8));
			if (B.sgn)
				hipLaunchKernelGGL(bs_expand_kernel<0>, dim3(blocks3), dim3(256), 0, s2, e);
			else if (packed)
				hipLaunchKernelGGL(bs_expand_kernel<1>, dim3(blocks3), dim3(256), 0, s2, e);
			else
				hipLaunchKernelGGL(bs_expand_kernel<2>, dim3(blocks3), dim3(256), 0, s2, e);
		};
		// (round 5, measured and dropped: the batch cut into 2 / 4 / 8 parts, each with its own part of the staging buffer, the parts
		//  applied one after the other on the caller's stream while a second stream scanned and expanded each part as soon as it was
		//  there -- expansion of part k beside the apply of part k + 1, two kernels bound by the memory at 4.5 and 4.1 TB/s of the
		//  8 the device has.  The step of mk13.b5 went from 4.63 ms to 4.74 / 5.19 / 6.30: two workgroup shapes that both want
		//  the LDS and the memory queues of the same CUs take more from each other than the overlap gives back.)
		for (int64_t r0 = 0; r0 < a.nrows; r0 += direct->stage_rows) {
			const int n = (int) std::min<int64_t>(direct->stage_rows, a.nrows - r0);
			ApplyArgs d2 = d;
			d2.direct = 0;
			d2.stage = direct->stage;
			d2.a.rows = a.rows + r0;
			d2.a.row_len = a.row_len + r0;
			d2.a.nrows = n;
			const int blocks2 = std::max(1, std::min((n + waves - 1) / waves, prop.multiProcessorCount * 8));
			const int nblocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
			d2.block_sum = direct->status;          // (the look-back words are not used by the staged output)
			HIP_CHECK(hipMemsetAsync(d2.block_sum, 0, (size_t) nblocks * sizeof(unsigned long long), stream));
			launch_apply(d2, blocks2);
			if (direct->ev_expand != nullptr)
				HIP_CHECK(hipEventRecord(direct->ev_expand, stream));
			expand_slice(r0, n, direct->stage, d2.block_sum, stream);
			direct->staged = true;
			direct->slices += 1;
		}
	} else {
		launch_apply(d, blocks);
	}
	HIP_CHECK(hipGetLastError());
}

}  // namespace sh
