// X.A = B over the PLUQ factorization (replaces spasm_solve / spasm_gesv, spasm_solve.c:13-96, and the two dense triangular
// solves they run per right-hand side, spasm_triangular.c:21-87).
//
// The reference solves one right-hand side at a time: z.U = b (forward, row by row of U), then y.L_piv = z (back, pivot by
// pivot of L, from the last one), x[p[j]] = y_j.  Here all right-hand sides of a call are solved together by three sweeps of
// one "pull" kernel family -- every unknown is written exactly once, by one wave, from values that are final:
//   F (forward)  z_i = b[q_i] - sum over the rows i' < i of U with an entry in pivot column q_i of U[i', q_i] z_i'
//   C (check)    r_c = b_c - sum_i U[i, c] z_i for every column c no pivot eliminates; ok = (no r_c != 0)
//   B (back)     y_j = (z_j - sum over j' > j of L[p[j'], j] y_j') / L[p[j], j]
// Restricting the sums to the rows the reference's loops have already visited (i' < i, j' > j) reproduces its values exactly,
// whatever the order of U's rows.  A pivot column that a LATER row of U also touches is not left at zero by the reference's
// forward loop: such columns are checked by C too (with no b term).
//
// Layout: right-hand sides in blocks of 64, unknown-major (V[block][unknown][64], u32 residues in [0, p)).  A wave owns one
// unknown of one block, lane = right-hand side: a dependency is one coalesced 256-byte load, the dependency lists
// ((unknown, coefficient * 2^32 mod p) pairs) are wave-uniform.  F and B are level-scheduled: one launch per level serves
// every block of the call; runs of consecutive thin levels go to one launch whose workgroups (one per block) step through
// them with a barrier between levels; where the unknowns carry long dependency lists, a whole workgroup shares each list.
// No workgroup waits on another.  (There is no separate variant for fewer than 64 right-hand sides: the idle lanes of a block
// cost nothing but their share of the 256-byte lines.)
#include <algorithm>
#include <mutex>
#include <numeric>

#include "colmajor.h"
#include "field_dev.h"

namespace sh {

namespace {

constexpr int SV_WAVES = 4;          // waves of a workgroup in a one-level launch (one unknown each)
constexpr int SV_TAIL_WAVES = 16;    // waves of the workgroup that steps through a run of thin levels
constexpr int SV_THIN = 16;          // a level with at most this many unknowns is thin
constexpr int SV_RUN = 2;            // ... and a run of at least this many thin levels gets one launch
constexpr int SV_SPLIT = 64;         // dependencies per unknown (on average over a launch) above which a workgroup shares each list

struct SweepArgs {
	const int *node;          // unknown written by position k (level order)
	const int *src;           // line of `base` it starts from
	const int64_t *dptr;      // dependencies of position k: [dptr[k], dptr[k + 1])
	const int *didx;          // unknown depended on
	const uint32_t *dval;     // coefficient * 2^32 mod p
	const uint32_t *scale;    // per position, * 2^32 mod p (nullptr: none)
	const uint32_t *base;
	int64_t base_ld;          // unknowns per block of `base`
	uint32_t *out;
	int64_t out_ld;
};

__device__ __forceinline__ void sweep_one(const SweepArgs &a, int k, int blk, int lane, const MontDev &F)
{
	uint32_t *O = a.out + (int64_t) blk * a.out_ld * 64;
	int64_t d = a.dptr[k];
	const int64_t e = a.dptr[k + 1];
	unsigned long long acc = 0;
	for (; d + 4 <= e; d += 4) {
		const int i0 = a.didx[d], i1 = a.didx[d + 1], i2 = a.didx[d + 2], i3 = a.didx[d + 3];
		const uint32_t c0 = a.dval[d], c1 = a.dval[d + 1], c2 = a.dval[d + 2], c3 = a.dval[d + 3];
		const uint32_t z0 = O[(int64_t) i0 * 64 + lane], z1 = O[(int64_t) i1 * 64 + lane];
		const uint32_t z2 = O[(int64_t) i2 * 64 + lane], z3 = O[(int64_t) i3 * 64 + lane];
		acc += (unsigned long long) montmul(c0, z0, F) + montmul(c1, z1, F);
		acc += (unsigned long long) montmul(c2, z2, F) + montmul(c3, z3, F);
	}
	for (; d < e; d++)
		acc += montmul(a.dval[d], O[(int64_t) a.didx[d] * 64 + lane], F);
	const uint32_t b = a.base[(int64_t) blk * a.base_ld * 64 + (int64_t) a.src[k] * 64 + lane];
	uint32_t v = submod(b, reduce_sum(acc, F), F);
	if (a.scale != nullptr)
		v = montmul(v, a.scale[k], F);
	O[(int64_t) a.node[k] * 64 + lane] = v;
}

// one level: positions [lo, hi), grid (ceil((hi - lo) / SV_WAVES), blocks)
__global__ __launch_bounds__(64 * SV_WAVES) void solve_sweep_kernel(SweepArgs a, int lo, int hi, MontDev F)
{
	const int k = __builtin_amdgcn_readfirstlane(lo + blockIdx.x * SV_WAVES + (int) (threadIdx.x >> 6));
	if (k < hi)
		sweep_one(a, k, blockIdx.y, threadIdx.x & 63, F);
}

// a run of levels [l0, l1) (level l: positions [lptr[l], lptr[l + 1])), one workgroup per block
__global__ __launch_bounds__(64 * SV_TAIL_WAVES) void solve_sweep_run_kernel(SweepArgs a, const int *lptr, int l0, int l1, MontDev F)
{
	const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	for (int l = l0; l < l1; l++) {
		const int hi = lptr[l + 1];
		for (int k = lptr[l] + w; k < hi; k += SV_TAIL_WAVES)
			sweep_one(a, k, blockIdx.y, lane, F);
		__syncthreads();
	}
}

// Long dependency lists (the factors of the large workloads hold unknowns with thousands of them): all SV_TAIL_WAVES waves of
// the workgroup take a slice of the list of ONE unknown, the partial sums meet in LDS, wave 0 writes.  One level, one unknown
// per workgroup (grid (unknowns, blocks)); or a run of levels [l0, l1), the workgroup of a block stepping through its unknowns.
__device__ __forceinline__ void sweep_split(const SweepArgs &a, int k, int blk, int w, int lane, uint32_t (*red)[64], const MontDev &F)
{
	const uint32_t *O = a.out + (int64_t) blk * a.out_ld * 64;
	const int64_t d0 = a.dptr[k], n = a.dptr[k + 1] - d0;
	int64_t d = d0 + n * w / SV_TAIL_WAVES;
	const int64_t e = d0 + n * (w + 1) / SV_TAIL_WAVES;
	unsigned long long acc = 0;
	for (; d + 4 <= e; d += 4) {
		const uint32_t z0 = O[(int64_t) a.didx[d] * 64 + lane], z1 = O[(int64_t) a.didx[d + 1] * 64 + lane];
		const uint32_t z2 = O[(int64_t) a.didx[d + 2] * 64 + lane], z3 = O[(int64_t) a.didx[d + 3] * 64 + lane];
		acc += (unsigned long long) montmul(a.dval[d], z0, F) + montmul(a.dval[d + 1], z1, F);
		acc += (unsigned long long) montmul(a.dval[d + 2], z2, F) + montmul(a.dval[d + 3], z3, F);
	}
	for (; d < e; d++)
		acc += montmul(a.dval[d], O[(int64_t) a.didx[d] * 64 + lane], F);
	red[w][lane] = reduce_sum(acc, F);
	__syncthreads();
	if (w == 0) {
		unsigned long long sum = 0;
		for (int t = 0; t < SV_TAIL_WAVES; t++)
			sum += red[t][lane];
		const uint32_t b = a.base[(int64_t) blk * a.base_ld * 64 + (int64_t) a.src[k] * 64 + lane];
		uint32_t v = submod(b, reduce_sum(sum, F), F);
		if (a.scale != nullptr)
			v = montmul(v, a.scale[k], F);
		a.out[(int64_t) blk * a.out_ld * 64 + (int64_t) a.node[k] * 64 + lane] = v;
	}
	__syncthreads();
}

__global__ __launch_bounds__(64 * SV_TAIL_WAVES) void solve_sweep_split_kernel(SweepArgs a, const int *lptr, int l0, int l1, MontDev F)
{
	__shared__ uint32_t red[SV_TAIL_WAVES][64];
	const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (l1 < 0) {                                   // one level l0, one unknown per workgroup
		sweep_split(a, lptr[l0] + blockIdx.x, blockIdx.y, w, lane, red, F);
		return;
	}
	for (int l = l0; l < l1; l++)
		for (int k = lptr[l]; k < lptr[l + 1]; k++)
			sweep_split(a, k, blockIdx.y, w, lane, red, F);
}

// C: checked columns handed out round-robin to G waves per block; wave g writes its verdict for the 64 right-hand sides of the
// block to part[(blk * G + g) * 64 + lane]
__global__ __launch_bounds__(64 * SV_WAVES) void solve_check_kernel(const int *ccol, const int64_t *cptr, const int *cidx, const uint32_t *cval,
                                                                    int ncheck, const uint32_t *Bd, int64_t m, const uint32_t *Z, int64_t r, int G,
                                                                    uint32_t *part, MontDev F)
{
	const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * SV_WAVES + (int) (threadIdx.x >> 6)), lane = threadIdx.x & 63, blk = blockIdx.y;
	if (g >= G)
		return;
	const uint32_t *Zb = Z + (int64_t) blk * r * 64;
	const uint32_t *Bb = Bd + (int64_t) blk * m * 64;
	uint32_t bad = 0;
	for (int k = g; k < ncheck; k += G) {
		unsigned long long acc = 0;
		int64_t d = cptr[k];
		const int64_t e = cptr[k + 1];
		for (; d + 4 <= e; d += 4) {
			const uint32_t z0 = Zb[(int64_t) cidx[d] * 64 + lane], z1 = Zb[(int64_t) cidx[d + 1] * 64 + lane];
			const uint32_t z2 = Zb[(int64_t) cidx[d + 2] * 64 + lane], z3 = Zb[(int64_t) cidx[d + 3] * 64 + lane];
			acc += (unsigned long long) montmul(cval[d], z0, F) + montmul(cval[d + 1], z1, F);
			acc += (unsigned long long) montmul(cval[d + 2], z2, F) + montmul(cval[d + 3], z3, F);
		}
		for (; d < e; d++)
			acc += montmul(cval[d], Zb[(int64_t) cidx[d] * 64 + lane], F);
		const int c = ccol[k];
		const uint32_t b = c >= 0 ? Bb[(int64_t) c * 64 + lane] : 0u;
		bad |= (uint32_t) (submod(b, reduce_sum(acc, F), F) != 0);
	}
	part[((int64_t) blk * G + g) * 64 + lane] = bad;
}

// ok[t] for the kb right-hand sides of the batch
__global__ void solve_ok_kernel(const uint32_t *part, int G, int kb, unsigned char *ok)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= kb)
		return;
	const int blk = t >> 6, lane = t & 63;
	uint32_t bad = 0;
	for (int g = 0; g < G; g++)
		bad |= part[((int64_t) blk * G + g) * 64 + lane];
	ok[t] = bad ? 0 : 1;
}

// right-hand sides t < kb of the batch (rows of B, balanced values) into Bd[blk][column][lane]: one thread per row, so every
// word has one writer (a row with a repeated column adds up, as spasm_scatter does)
__global__ void solve_scatter_kernel(const int64_t *Bp, const int *Bj, const int *Bx, int kb, int64_t m, uint32_t *Bd, MontDev F)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= kb)
		return;
	uint32_t *D = Bd + (int64_t) (t >> 6) * m * 64 + (t & 63);
	for (int64_t px = Bp[t]; px < Bp[t + 1]; px++) {
		uint32_t *w = D + (int64_t) Bj[px] * 64;
		const uint32_t v = from_balanced(Bx[px], F);
		const uint32_t s = *w + v;                      // both < p < 2^32: one correction
		*w = (s < v || s >= F.p) ? s - F.p : s;
	}
}

// emit, pass 1 (write = false): non-zero y of the emit positions [lo, hi) of chunk c, per right-hand side, into
// cnt[(blk * nchunk + c) * 64 + lane].  Pass 2 (write = true): the entries themselves, at Xp[t] + cnt (the scanned offsets)
template <bool WRITE>
__global__ __launch_bounds__(64 * SV_WAVES) void solve_emit_kernel(const uint32_t *Y, int64_t r, const int *ej, const int *ecol, int nchunk, uint32_t *cnt,
                                                                  const int64_t *Xp, int kb, int *Xj, int *Xx, MontDev F)
{
	const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * SV_WAVES + (int) (threadIdx.x >> 6)), lane = threadIdx.x & 63, blk = blockIdx.y;
	if (c >= nchunk)
		return;
	const int lo = (int) ((int64_t) r * c / nchunk), hi = (int) ((int64_t) r * (c + 1) / nchunk);
	const uint32_t *Yb = Y + (int64_t) blk * r * 64;
	uint32_t *cw = cnt + ((int64_t) blk * nchunk + c) * 64 + lane;
	if (!WRITE) {
		uint32_t n = 0;
		for (int e = lo; e < hi; e++)
			n += Yb[(int64_t) ej[e] * 64 + lane] != 0;
		*cw = n;
		return;
	}
	const int t = blk * 64 + lane;
	if (t >= kb)
		return;
	int64_t w = Xp[t] + *cw;
	for (int e = lo; e < hi; e++) {
		const uint32_t v = Yb[(int64_t) ej[e] * 64 + lane];
		if (v != 0) {
			Xj[w] = ecol[e];
			Xx[w] = to_balanced(v, F);
			w += 1;
		}
	}
}

// emit, scan: per right-hand side the chunk counts become offsets inside its row, then one workgroup turns the row lengths
// into the row pointers Xp[0..kb]
__global__ void solve_row_scan_kernel(uint32_t *cnt, int nchunk, int kb, int64_t *len)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= kb)
		return;
	uint32_t *c = cnt + (int64_t) (t >> 6) * nchunk * 64 + (t & 63);
	uint32_t run = 0;
	for (int k = 0; k < nchunk; k++) {
		const uint32_t v = c[(int64_t) k * 64];
		c[(int64_t) k * 64] = run;
		run += v;
	}
	len[t] = run;
}

uint32_t to_mont(const Mont &M, spasm_ZZp a)
{
	return (uint32_t) (((uint64_t) zp_unsigned(M.p, a) << 32) % M.p);
}

// one level-scheduled sweep (F or B) as the host plans it
struct SweepPlan {
	std::vector<int> node, src, didx, lptr;
	std::vector<int64_t> dptr;
	std::vector<uint32_t> dval, scale;
	std::vector<int2> steps;          // (first level, last level + 1): one launch each
	std::vector<char> split;          // ... whose unknowns have long dependency lists (solve_sweep_split_kernel)
	int64_t bytes_per_block = 0;      // algorithmic bytes of one block of 64 right-hand sides
};

// positions in level order from per-unknown levels and dependency lists (deps[u]: (unknown, coefficient))
void finish_sweep(SweepPlan &S, int n, const std::vector<int> &level, int nlev, const std::vector<int> &srcof,
                  const std::vector<std::vector<std::pair<int, uint32_t>>> &deps, const std::vector<uint32_t> *scale)
{
	S.lptr.assign((size_t) nlev + 1, 0);
	for (int u = 0; u < n; u++)
		S.lptr[level[u] + 1] += 1;
	for (int l = 0; l < nlev; l++)
		S.lptr[l + 1] += S.lptr[l];
	std::vector<int> at(S.lptr.begin(), S.lptr.end() - 1);
	S.node.assign((size_t) n, 0);
	for (int u = 0; u < n; u++)
		S.node[at[level[u]]++] = u;
	S.src.resize((size_t) n);
	S.dptr.assign((size_t) n + 1, 0);
	for (int k = 0; k < n; k++) {
		const int u = S.node[k];
		S.src[k] = srcof[u];
		S.dptr[k + 1] = S.dptr[k] + (int64_t) deps[u].size();
		if (scale != nullptr)
			S.scale.push_back((*scale)[u]);
	}
	S.didx.reserve((size_t) S.dptr[n]);
	S.dval.reserve((size_t) S.dptr[n]);
	for (int k = 0; k < n; k++)
		for (const auto &d : deps[S.node[k]]) {
			S.didx.push_back(d.first);
			S.dval.push_back(d.second);
		}
	// a dependency: its 256-byte line + 8 bytes of list; an unknown: its base line, its own line, its list pointer (+ scale)
	S.bytes_per_block = S.dptr[n] * (256 + 8) + (int64_t) n * (512 + 8 + 8 + (scale ? 4 : 0));
	for (int l = 0; l < nlev;) {
		int e = l;
		while (e < nlev && S.lptr[e + 1] - S.lptr[e] <= SV_THIN)
			e += 1;
		if (e - l < SV_RUN)
			e = l + 1;
		S.steps.push_back(make_int2(l, e));
		// long lists: on average more dependencies per unknown than a wave has lanes
		const int64_t deps = S.dptr[S.lptr[e]] - S.dptr[S.lptr[l]], nodes = S.lptr[e] - S.lptr[l];
		S.split.push_back(deps >= SV_SPLIT * nodes);
		l = e;
	}
}

struct DevSweep {
	int *node = nullptr, *src = nullptr, *didx = nullptr, *lptr = nullptr;
	int64_t *dptr = nullptr;
	uint32_t *dval = nullptr, *scale = nullptr;
};

template <typename T> T *upload(const std::vector<T> &v)
{
	T *d = nullptr;
	HIP_CHECK(malloc_or_trim((void **) &d, std::max<size_t>(v.size(), 1) * sizeof(T)));
	if (!v.empty())
		HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
	return d;
}

DevSweep upload_sweep(const SweepPlan &S)
{
	DevSweep D;
	D.node = upload(S.node);
	D.src = upload(S.src);
	D.didx = upload(S.didx);
	D.lptr = upload(S.lptr);
	D.dptr = upload(S.dptr);
	D.dval = upload(S.dval);
	if (!S.scale.empty())
		D.scale = upload(S.scale);
	return D;
}

void free_sweep(DevSweep &D)
{
	for (void *p : {(void *) D.node, (void *) D.src, (void *) D.didx, (void *) D.lptr, (void *) D.dptr, (void *) D.dval, (void *) D.scale})
		if (p != nullptr)
			(void) hipFree(p);
	D = DevSweep();
}

}  // namespace

}  // namespace sh

using namespace sh;

struct spasm_hip_solver {
	int n = 0, m = 0, r = 0;          // rows of A (columns of X), columns of A and B, rank
	int64_t prime = 0;
	Mont M{};
	SweepPlan F, B;
	// C: checked columns (column of b, or -1: a pivot column touched by a later row of U), their rows of U
	std::vector<int> ccol, cidx;
	std::vector<int64_t> cptr;
	std::vector<uint32_t> cval;
	int64_t bytes_check_per_block = 0;
	// emit order: positions j of the pivots by increasing row p[j] of A
	std::vector<int> ej, ecol;
	DevSweep dF, dB;
	int *d_ccol = nullptr, *d_cidx = nullptr, *d_ej = nullptr, *d_ecol = nullptr;
	int64_t *d_cptr = nullptr;
	uint32_t *d_cval = nullptr;
	double plan_seconds = 0;
	double last[16] = {0};
	std::mutex mutex;
};

namespace {

// checks the factorization and builds the three sweeps (host only)
void plan_solver(const struct spasm_lu *fact, spasm_hip_solver *S)
{
	const struct spasm_csr *U = fact->U, *L = fact->L;
	if (L == nullptr)
		die("spasm_hip_gesv: fact->L is NULL (echelonize with opts->L = 1)");
	if (U == nullptr || fact->qinv == nullptr || (U->n > 0 && fact->p == nullptr))
		die("spasm_hip_gesv: the factorization has no U, qinv or p");
	const int r = U->n, m = U->m, n = L->n;
	if (L->m != r)
		die("spasm_hip_gesv: L has %d columns, U has %d rows", L->m, r);
	if (L->field->p != U->field->p)
		die("spasm_hip_gesv: L is mod %lld, U mod %lld", (long long) L->field->p, (long long) U->field->p);
	S->n = n;
	S->m = m;
	S->r = r;
	S->prime = U->field->p;
	S->M = mont_setup(S->prime);
	const Mont &M = S->M;
	const int *qinv = fact->qinv;
	std::vector<int> q((size_t) r, -1);
	for (int c = 0; c < m; c++) {
		const int i = qinv[c];
		if (i < -1 || i >= r)
			die("spasm_hip_gesv: qinv[%d] = %d out of range (rank %d)", c, i, r);
		if (i >= 0) {
			if (q[i] >= 0)
				die("spasm_hip_gesv: row %d of U holds two pivots (columns %d and %d)", i, q[i], c);
			q[i] = c;
		}
	}
	for (int i = 0; i < r; i++) {
		const int64_t px = U->p[i];
		if (q[i] < 0 || px >= U->p[i + 1] || U->j[px] != q[i] || U->x[px] != 1)
			die("spasm_hip_gesv: the pivot of row %d of U is not a unit entry at the start of the row", i);
	}
	const int *Lpiv = fact->p;
	std::vector<int> jof((size_t) n, -1);
	for (int j = 0; j < r; j++) {
		const int i = Lpiv[j];
		if (i < 0 || i >= n)
			die("spasm_hip_gesv: p[%d] = %d is not a row of L (%d rows)", j, i, n);
		if (jof[i] >= 0)
			die("spasm_hip_gesv: rows p[%d] and p[%d] of L are the same row %d", jof[i], j, i);
		jof[i] = j;
	}
	auto plan_forward = [&] {
		// dependencies of F by pivot column: U[i', q_i] for the rows i' < i; the entries of LATER rows in pivot columns and
		// every entry in a non-pivotal column go to C
		std::vector<std::vector<std::pair<int, uint32_t>>> deps((size_t) r);
		std::vector<std::vector<std::pair<int, uint32_t>>> cdeps((size_t) m);
		std::vector<char> late((size_t) m, 0);
		for (int i = 0; i < r; i++)
			for (int64_t px = U->p[i] + 1; px < U->p[i + 1]; px++) {
				const int c = U->j[px];
				if (c < 0 || c >= m)
					die("spasm_hip_gesv: column %d of U out of range", c);
				if (U->x[px] == 0)
					continue;
				const int t = qinv[c];
				if (t == i)
					die("spasm_hip_gesv: row %d of U has its pivot column twice", i);
				const uint32_t v = to_mont(M, U->x[px]);
				if (t > i)
					deps[t].push_back({i, v});
				else {
					cdeps[c].push_back({i, v});
					if (t >= 0)
						late[c] = 1;
				}
			}
		std::vector<int> level((size_t) r, 0);
		int nlev = 0;
		for (int i = 0; i < r; i++) {
			int l = 0;
			for (const auto &d : deps[i])
				l = std::max(l, level[d.first] + 1);
			level[i] = l;
			nlev = std::max(nlev, l + 1);
		}
		finish_sweep(S->F, r, level, nlev, q, deps, nullptr);
		S->cptr.assign(1, 0);
		for (int c = 0; c < m; c++) {
			if (qinv[c] >= 0 && !late[c])
				continue;
			S->ccol.push_back(qinv[c] >= 0 ? -1 : c);
			for (const auto &d : cdeps[c]) {
				S->cidx.push_back(d.first);
				S->cval.push_back(d.second);
			}
			S->cptr.push_back((int64_t) S->cidx.size());
		}
		S->bytes_check_per_block = (int64_t) S->cidx.size() * (256 + 8) + (int64_t) S->ccol.size() * (256 + 12);
	};
	auto plan_back = [&] {
		// dependencies of B: L[p[j'], j] for j' > j, and the diagonal L[p[j], j] (its inverse scales y_j)
		std::vector<std::vector<std::pair<int, uint32_t>>> deps((size_t) r);
		std::vector<uint32_t> dinv((size_t) r, 0);
		for (int jp = 0; jp < r; jp++) {
			const int i = Lpiv[jp];
			spasm_ZZp diag = 0;
			for (int64_t px = L->p[i]; px < L->p[i + 1]; px++) {
				const int j = L->j[px];
				if (j < 0 || j >= r)
					die("spasm_hip_gesv: column %d of L out of range (rank %d)", j, r);
				if (j == jp) {
					if (diag == 0)             // (the reference takes the first entry on the diagonal)
						diag = L->x[px];
				} else if (j < jp && L->x[px] != 0)
					deps[j].push_back({jp, to_mont(M, L->x[px])});
			}
			if (zp_init(M.p, diag) == 0)
				die("spasm_hip_gesv: row p[%d] = %d of L has no non-zero entry in column %d", jp, i, jp);
			dinv[jp] = to_mont(M, zp_inverse(M.p, zp_init(M.p, diag)));
		}
		std::vector<int> level((size_t) r, 0), self((size_t) r);
		int nlev = 0;
		for (int j = r - 1; j >= 0; j--) {
			int l = 0;
			for (const auto &d : deps[j])
				l = std::max(l, level[d.first] + 1);
			level[j] = l;
			nlev = std::max(nlev, l + 1);
			self[j] = j;
		}
		finish_sweep(S->B, r, level, nlev, self, deps, &dinv);
		std::vector<int> order((size_t) r);
		std::iota(order.begin(), order.end(), 0);
		std::sort(order.begin(), order.end(), [&](int a, int b) { return Lpiv[a] < Lpiv[b]; });
		S->ej = order;
		S->ecol.resize((size_t) r);
		for (int e = 0; e < r; e++)
			S->ecol[e] = Lpiv[order[e]];
	};
	pool_run(2, [&](int t) {
		if (t == 0)
			plan_forward();
		else
			plan_back();
	});
}

int launch_sweep(const SweepPlan &P, const DevSweep &D, const uint32_t *base, int64_t base_ld, uint32_t *out, int64_t out_ld, int nblk,
                 const MontDev &F, hipStream_t stream)
{
	SweepArgs a;
	a.node = D.node;
	a.src = D.src;
	a.dptr = D.dptr;
	a.didx = D.didx;
	a.dval = D.dval;
	a.scale = D.scale;
	a.base = base;
	a.base_ld = base_ld;
	a.out = out;
	a.out_ld = out_ld;
	for (size_t t = 0; t < P.steps.size(); t++) {
		const int2 s = P.steps[t];
		if (P.split[t]) {
			const bool one = s.y - s.x == 1;
			hipLaunchKernelGGL(solve_sweep_split_kernel, dim3(one ? P.lptr[s.x + 1] - P.lptr[s.x] : 1, nblk), dim3(64 * SV_TAIL_WAVES), 0, stream, a,
			                   D.lptr, s.x, one ? -1 : s.y, F);
		} else if (s.y - s.x == 1) {
			const int lo = P.lptr[s.x], hi = P.lptr[s.x + 1];
			hipLaunchKernelGGL(solve_sweep_kernel, dim3((hi - lo + SV_WAVES - 1) / SV_WAVES, nblk), dim3(64 * SV_WAVES), 0, stream, a, lo, hi, F);
		} else
			hipLaunchKernelGGL(solve_sweep_run_kernel, dim3(1, nblk), dim3(64 * SV_TAIL_WAVES), 0, stream, a, D.lptr, s.x, s.y, F);
	}
	HIP_CHECK(hipGetLastError());
	return (int) P.steps.size();
}

int check_waves(const spasm_hip_solver *S)
{
	const int nc = (int) S->ccol.size();
	return std::max(1, std::min(512, (nc + 7) / 8));
}

int emit_chunks(const spasm_hip_solver *S) { return std::max(1, std::min(256, S->r / 512)); }

}  // namespace

extern "C" {

spasm_hip_solver *spasm_hip_solver_create(const struct spasm_lu *fact)
{
	if (fact == nullptr)
		die("spasm_hip_solver_create: fact is NULL");
	if (fact->L == nullptr)
		die("spasm_hip_gesv: fact->L is NULL (echelonize with opts->L = 1)");
	if (spasm_hip_device_count() == 0)
		die("spasm_hip_solver_create: no HIP device (this library has no CPU path)");
	const double t0 = wtime();
	spasm_hip_solver *S = new spasm_hip_solver();
	plan_solver(fact, S);
	S->dF = upload_sweep(S->F);
	S->dB = upload_sweep(S->B);
	S->d_ccol = upload(S->ccol);
	S->d_cptr = upload(S->cptr);
	S->d_cidx = upload(S->cidx);
	S->d_cval = upload(S->cval);
	S->d_ej = upload(S->ej);
	S->d_ecol = upload(S->ecol);
	S->plan_seconds = wtime() - t0;
	logmsg("[solve] plan: rank %d, %d + %d levels (%zu + %zu launches), %zu checked columns, %.3f s\n", S->r, (int) S->F.lptr.size() - 1,
	       (int) S->B.lptr.size() - 1, S->F.steps.size(), S->B.steps.size(), S->ccol.size(), S->plan_seconds);
	return S;
}

void spasm_hip_solver_destroy(spasm_hip_solver *S)
{
	if (S == nullptr)
		return;
	free_sweep(S->dF);
	free_sweep(S->dB);
	for (void *p : {(void *) S->d_ccol, (void *) S->d_cptr, (void *) S->d_cidx, (void *) S->d_cval, (void *) S->d_ej, (void *) S->d_ecol})
		(void) hipFree(p);
	delete S;
}

void spasm_hip_solver_levels(const spasm_hip_solver *S, int *out)
{
	out[0] = (int) S->F.lptr.size() - 1;
	out[1] = (int) S->B.lptr.size() - 1;
	out[2] = (int) S->F.steps.size();
	out[3] = (int) S->B.steps.size();
}

int spasm_hip_solver_stats(const spasm_hip_solver *S, double *out, int count)
{
	const int k = std::min(count, 16);
	for (int t = 0; t < k; t++)
		out[t] = S->last[t];
	if (count > 0)
		out[0] = S->plan_seconds;
	// [12] [13] launches of F and of B that share each list over a workgroup, [14] [15] that step through a run of thin levels
	// (properties of the plan: there before the first gesv)
	const SweepPlan *P[2] = {&S->F, &S->B};
	for (int h = 0; h < 2; h++) {
		int split = 0, run = 0;
		for (size_t t = 0; t < P[h]->steps.size(); t++) {
			split += P[h]->split[t] != 0;
			run += P[h]->steps[t].y - P[h]->steps[t].x > 1;
		}
		if (12 + h < k)
			out[12 + h] = split;
		if (14 + h < k)
			out[14 + h] = run;
	}
	return 16;
}

struct spasm_csr *spasm_hip_solver_gesv(spasm_hip_solver *S, const struct spasm_csr *Bm, bool *ok)
{
	if (Bm == nullptr)
		die("spasm_hip_gesv: B is NULL");
	if (Bm->m != S->m)
		die("spasm_hip_gesv: B has %d columns, U has %d", Bm->m, S->m);
	if (Bm->field->p != S->prime)
		die("spasm_hip_gesv: B is mod %lld, the factorization mod %lld", (long long) Bm->field->p, (long long) S->prime);
	const int k = Bm->n;
	const int64_t bnz = Bm->p[k];
	for (int t = 0; t < k; t++)
		if (Bm->p[t] > Bm->p[t + 1])
			die("spasm_hip_gesv: row pointers of B decrease at row %d", t);
	for (int64_t px = 0; px < bnz; px++)
		if (Bm->j[px] < 0 || Bm->j[px] >= S->m)
			die("spasm_hip_gesv: column %d of B out of range (%d columns)", Bm->j[px], S->m);
	std::lock_guard<std::mutex> guard(S->mutex);
	const int64_t m = S->m, r = S->r;
	const MontDev F = to_dev(S->M);
	const int G = check_waves(S), nchunk = emit_chunks(S);
	// per right-hand side: b (its region later holds y), z, the check verdicts, the emit counts, ok
	const int64_t per_rhs = 4 * (std::max<int64_t>(m, r) + r + G + nchunk + 4) + 1;
	size_t free_b = 0, total_b = 0;
	mem_info(&free_b, &total_b);
	int64_t kb_max = (int64_t) (free_b / 2) / per_rhs / 64 * 64;
	kb_max = std::max<int64_t>(64, std::min<int64_t>(kb_max, (int64_t) 65535 * 64));
	const int batch_env = env_int("SPASM_HIP_SOLVE_BATCH", 0);          // (tests: several batches on small inputs)
	if (batch_env > 0)
		kb_max = std::min<int64_t>(kb_max, std::max(64, batch_env / 64 * 64));
	const int kb_cap = (int) std::min<int64_t>(kb_max, ((int64_t) std::max(k, 1) + 63) / 64 * 64);
	const int nblk_cap = kb_cap / 64;
	uint32_t *d_Bd = (uint32_t *) big_alloc((size_t) nblk_cap * 64 * std::max<int64_t>(std::max<int64_t>(m, r), 1) * 4);
	uint32_t *d_Z = (uint32_t *) big_alloc((size_t) nblk_cap * 64 * std::max<int64_t>(r, 1) * 4);
	uint32_t *d_part = (uint32_t *) big_alloc((size_t) nblk_cap * 64 * G * 4);
	uint32_t *d_cnt = (uint32_t *) big_alloc((size_t) nblk_cap * 64 * nchunk * 4);
	int64_t *d_len = (int64_t *) big_alloc((size_t) kb_cap * 8);
	int64_t *d_Xp = (int64_t *) big_alloc((size_t) (kb_cap + 1) * 8);
	unsigned char *d_ok = (unsigned char *) big_alloc((size_t) kb_cap);
	hipStream_t stream = 0;
	hipEvent_t ev[6];
	for (auto &e : ev)
		HIP_CHECK(hipEventCreate(&e));
	double ms[5] = {0, 0, 0, 0, 0};
	int launches_F = 0, launches_B = 0, launches = 0, batches = 0;
	int64_t bytes = 0;

	struct spasm_csr *X = spasm_hip_csr_alloc(k, S->n, 1, S->prime, true);
	X->p[0] = 0;
	int64_t xnz = 0;
	std::vector<unsigned char> okh((size_t) std::max(k, 1));
	std::vector<int64_t> Xp_h((size_t) kb_cap + 1);
	for (int t0 = 0; t0 < k; t0 += kb_cap) {
		const int kb = std::min(kb_cap, k - t0), nblk = (kb + 63) / 64;
		batches += 1;
		// the batch's rows of B, row pointers rebased
		const int64_t b0 = Bm->p[t0], b1 = Bm->p[t0 + kb];
		std::vector<int64_t> bp((size_t) kb + 1);
		for (int t = 0; t <= kb; t++)
			bp[t] = Bm->p[t0 + t] - b0;
		int64_t *d_bp = (int64_t *) big_alloc((size_t) (kb + 1) * 8);
		int *d_bj = (int *) big_alloc((size_t) std::max<int64_t>(b1 - b0, 1) * 4);
		int *d_bx = (int *) big_alloc((size_t) std::max<int64_t>(b1 - b0, 1) * 4);
		h2d(d_bp, bp.data(), (size_t) (kb + 1) * 8, stream);
		h2d(d_bj, Bm->j + b0, (size_t) (b1 - b0) * 4, stream);
		std::vector<int> bx((size_t) (b1 - b0));
		for (int64_t px = b0; px < b1; px++)
			bx[px - b0] = zp_init(S->prime, Bm->x[px]);      // balanced, whatever the caller stored
		h2d(d_bx, bx.data(), (size_t) (b1 - b0) * 4, stream);
		HIP_CHECK(hipEventRecord(ev[0], stream));
		HIP_CHECK(hipMemsetAsync(d_Bd, 0, (size_t) nblk * 64 * m * 4, stream));
		hipLaunchKernelGGL(solve_scatter_kernel, dim3((kb + 255) / 256), dim3(256), 0, stream, d_bp, d_bj, d_bx, kb, m, d_Bd, F);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(ev[1], stream));
		launches_F += launch_sweep(S->F, S->dF, d_Bd, m, d_Z, r, nblk, F, stream);
		HIP_CHECK(hipEventRecord(ev[2], stream));
		hipLaunchKernelGGL(solve_check_kernel, dim3((G + SV_WAVES - 1) / SV_WAVES, nblk), dim3(64 * SV_WAVES), 0, stream, S->d_ccol, S->d_cptr,
		                   S->d_cidx, S->d_cval, (int) S->ccol.size(), d_Bd, m, d_Z, r, G, d_part, F);
		hipLaunchKernelGGL(solve_ok_kernel, dim3((kb + 255) / 256), dim3(256), 0, stream, d_part, G, kb, d_ok);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(ev[3], stream));
		// y goes where b was (b is not read after C)
		uint32_t *d_Y = d_Bd;
		launches_B += launch_sweep(S->B, S->dB, d_Z, r, d_Y, r, nblk, F, stream);
		HIP_CHECK(hipEventRecord(ev[4], stream));
		hipLaunchKernelGGL(solve_emit_kernel<false>, dim3((nchunk + SV_WAVES - 1) / SV_WAVES, nblk), dim3(64 * SV_WAVES), 0, stream, d_Y, r,
		                   S->d_ej, S->d_ecol, nchunk, d_cnt, nullptr, kb, nullptr, nullptr, F);
		hipLaunchKernelGGL(solve_row_scan_kernel, dim3((kb + 255) / 256), dim3(256), 0, stream, d_cnt, nchunk, kb, d_len);
		launch_pointer_scan(d_len, kb, d_Xp, stream);
		HIP_CHECK(hipGetLastError());
		d2h(Xp_h.data(), d_Xp, (size_t) (kb + 1) * 8, stream);
		const int64_t nnz = Xp_h[kb];
		int *d_Xj = (int *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4);
		int *d_Xx = (int *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4);
		hipLaunchKernelGGL(solve_emit_kernel<true>, dim3((nchunk + SV_WAVES - 1) / SV_WAVES, nblk), dim3(64 * SV_WAVES), 0, stream, d_Y, r,
		                   S->d_ej, S->d_ecol, nchunk, d_cnt, d_Xp, kb, d_Xj, d_Xx, F);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(ev[5], stream));
		if (xnz + nnz > X->nzmax)
			spasm_hip_csr_realloc(X, std::max<int64_t>(xnz + nnz, 2 * X->nzmax));
		d2h(X->j + xnz, d_Xj, (size_t) nnz * 4, stream);
		d2h(X->x + xnz, d_Xx, (size_t) nnz * 4, stream);
		d2h(okh.data() + t0, d_ok, (size_t) kb, stream);
		for (int t = 1; t <= kb; t++)
			X->p[t0 + t] = xnz + Xp_h[t];
		xnz += nnz;
		float e;
		for (int s = 0; s < 5; s++) {
			HIP_CHECK(hipEventElapsedTime(&e, ev[s], ev[s + 1]));
			ms[s] += e;
		}
		launches += 7;                  // scatter, check, ok, emit count, row scan, scan, emit write
		bytes += (S->F.bytes_per_block + S->bytes_check_per_block + S->B.bytes_per_block) * nblk;
		big_free(d_Xj);
		big_free(d_Xx);
		big_free(d_bp);
		big_free(d_bj);
		big_free(d_bx);
	}
	for (auto &e : ev)
		HIP_CHECK(hipEventDestroy(e));
	big_free(d_Bd);
	big_free(d_Z);
	big_free(d_part);
	big_free(d_cnt);
	big_free(d_len);
	big_free(d_Xp);
	big_free(d_ok);
	if (ok != nullptr)
		for (int t = 0; t < k; t++)
			ok[t] = okh[t] != 0;
	spasm_hip_csr_realloc(X, -1);
	// [1] scatter of B, [2] F, [3] C, [4] B, [5] emit (device ms), [6] F launches, [7] B launches, [8] all launches,
	// [9] algorithmic bytes of the three sweeps, [10] batches, [11] right-hand sides per batch
	for (int s = 0; s < 5; s++)
		S->last[1 + s] = ms[s];
	S->last[6] = launches_F;
	S->last[7] = launches_B;
	S->last[8] = launches + launches_F + launches_B;
	S->last[9] = (double) bytes;
	S->last[10] = batches;
	S->last[11] = kb_cap;
	return X;
}

// spasm_gesv (spasm_solve.c:52): plan, solve, drop the plan
struct spasm_csr *spasm_hip_gesv(const struct spasm_lu *fact, const struct spasm_csr *B, bool *ok)
{
	if (fact == nullptr || fact->L == nullptr)
		die("spasm_hip_gesv: fact->L is NULL (echelonize with opts->L = 1)");
	spasm_hip_solver *S = spasm_hip_solver_create(fact);
	struct spasm_csr *X = spasm_hip_solver_gesv(S, B, ok);
	spasm_hip_solver_destroy(S);
	return X;
}

// spasm_solve (spasm_solve.c:13): one dense right-hand side b (U->m entries) -> dense x (L->n entries)
bool spasm_hip_solve(const struct spasm_lu *fact, const spasm_ZZp *b, spasm_ZZp *x)
{
	if (fact == nullptr || fact->L == nullptr)
		die("spasm_hip_solve: fact->L is NULL (echelonize with opts->L = 1)");
	const int m = fact->U->m, n = fact->L->n;
	struct spasm_csr *B = spasm_hip_csr_alloc(1, m, std::max(m, 1), fact->L->field->p, true);
	int64_t w = 0;
	for (int c = 0; c < m; c++)
		if (b[c] != 0) {
			B->j[w] = c;
			B->x[w] = b[c];
			w += 1;
		}
	B->p[0] = 0;
	B->p[1] = w;
	bool ok = false;
	struct spasm_csr *X = spasm_hip_gesv(fact, B, &ok);
	for (int i = 0; i < n; i++)
		x[i] = 0;
	for (int64_t px = X->p[0]; px < X->p[1]; px++)
		x[X->j[px]] = X->x[px];
	spasm_hip_csr_free(X);
	spasm_hip_csr_free(B);
	return ok;
}

}  // extern "C"
