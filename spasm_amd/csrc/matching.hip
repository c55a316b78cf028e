// Maximum bipartite matching of a sparse pattern on the device -- replaces spasm_maximum_matching (spasm_matching.c:103) -- and
// the two alternating searches of the coarse Dulmage-Mendelsohn decomposition (the bfs of spasm_dm.c:22-58).
//
// The rows x of the smaller side are matched to their neighbours y (the pattern of A when n <= m, of its transpose otherwise:
// the transpose is built on the device as a column-major image, colmajor.h).
//   Greedy rounds: every free x picks its smallest free neighbour and claims it with atomicMin on x; a second kernel hands each
//   claimed y to its smallest claimant.
//   Augmenting phases (APFB / MS-BFS style): a level-synchronous BFS from all free x at once over alternating paths.  A level
//   expands the frontier rows: every y not reached in an earlier level is claimed with atomicMin on x (parent[y] = the smallest
//   claimant, whatever the order of arrival); a second pass settles the ys the level reached: a free y ends its tree (each tree
//   keeps the smallest free y it reached, atomicMin), a matched y puts its mate in the next frontier.  A tree that has ended
//   stops growing, every y is reached once per phase, so the trees and the paths they end in are vertex-disjoint and one kernel
//   augments all of them.  Phases repeat until one finds no path (Berge).
//   Short frontiers (a long chain: one augmenting path of length O(n)) run the rest of the phase inside one workgroup and one
//   launch, __syncthreads() between the passes; the frontier goes back to the grid-wide passes when it grows past SMALL.
//   Words that another thread of the same launch wrote are read with agent-scope atomic loads (no stale L1 copy).
//   Every decision depends on sets and minima only, never on the order in which threads arrive: two calls give the same
//   matching.  Every device loop is bounded (n + m levels per phase, n + m steps per path): passing a bound sets an error bit
//   that the host turns into a fatal error.
// The last phase, which finds no path, has reached exactly the ys that alternating paths reach from the free xs; one more
// phase on the other orientation (mates swapped) reaches the other coarse set.  Both go back to the host as flags.
#include <algorithm>
#include <vector>

#include "colmajor.h"
#include "dm.h"

namespace sh {

namespace {

constexpr int NONE = 0x7f7f7f7f;     // every byte 0x7f (hipMemset): above every index
constexpr int SMALL = 4096;          // frontiers up to this many rows run their levels inside one workgroup
constexpr int SMALL_THREADS = 1024;
constexpr int GREEDY_ROUNDS = 8;

enum { C_NEXT = 0, C_FOUND, C_AUG, C_ERR, C_CUR, C_FRONT, C_LEVELS, C_NEW, C_COUNT = 8 };
enum { ERR_LEVELS = 1, ERR_PATH = 2 };

template <typename T> __device__ __forceinline__ T ld(const T *p)
{
	return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T> __device__ __forceinline__ void st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct Side {                  // one orientation: the rows x of a pattern and their neighbours y
	const int64_t *gp;
	const int *gj;
	int nx, ny;
	int *mx, *my;              // mate of x / of y, or -1
};

struct Search {                // the workspace of a phase (room for max(n, m) in every array)
	int *parent;               // y -> the smallest x that reached it (NONE: not reached); the greedy's claims
	int *seen;                 // y -> 1 once a level has settled it
	int *root;                 // x -> root of its tree
	int *end;                  // root -> smallest free y its tree reached (NONE)
	int *found;                // the ys the current level reached
	int *buf0, *buf1;          // frontiers
	int *ctr;                  // C_COUNT counters
};

__device__ void expand(const Side &G, const Search &S, const int *F, int f, int t0, int stride)
{
	for (int t = t0; t < f; t += stride) {
		const int x = ld(F + t);
		if (ld(S.end + ld(S.root + x)) != NONE)
			continue;                               // its tree has a path already
		for (int64_t e = G.gp[x]; e < G.gp[x + 1]; e++) {
			const int y = G.gj[e];
			if (ld(S.seen + y))
				continue;
			if (atomicMin(S.parent + y, x) == NONE)
				st(S.found + atomicAdd(S.ctr + C_FOUND, 1), y);
		}
	}
}

__device__ void settle(const Side &G, const Search &S, int *Fn, int nfound, int t0, int stride)
{
	for (int t = t0; t < nfound; t += stride) {
		const int y = ld(S.found + t);
		st(S.seen + y, 1);
		const int r = ld(S.root + ld(S.parent + y));
		const int x2 = ld(G.my + y);
		if (x2 < 0) {
			atomicMin(S.end + r, y);
		} else {
			st(S.root + x2, r);
			st(Fn + atomicAdd(S.ctr + C_NEXT, 1), x2);
		}
	}
}

__global__ void dm_expand_kernel(Side G, Search S, const int *F, int f)
{
	expand(G, S, F, f, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

__global__ void dm_settle_kernel(Side G, Search S, int *Fn)
{
	settle(G, S, Fn, S.ctr[C_FOUND], blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// levels of one phase inside one workgroup while the frontier has at most SMALL rows; leaves the frontier's buffer (C_CUR), its
// size (C_FRONT) and the phase's level count (C_LEVELS)
__global__ __launch_bounds__(SMALL_THREADS) void dm_levels_small_kernel(Side G, Search S, int cur, int f, int levels, int max_levels)
{
	const int t0 = threadIdx.x, stride = blockDim.x;
	while (f > 0 && f <= SMALL) {
		if (levels >= max_levels) {
			if (t0 == 0)
				atomicOr(S.ctr + C_ERR, ERR_LEVELS);
			break;
		}
		expand(G, S, cur ? S.buf1 : S.buf0, f, t0, stride);
		__syncthreads();
		settle(G, S, cur ? S.buf0 : S.buf1, ld(S.ctr + C_FOUND), t0, stride);
		__syncthreads();
		const int next = ld(S.ctr + C_NEXT);
		__syncthreads();                                    // every thread has its count before they are reset
		if (t0 == 0) {
			st(S.ctr + C_FOUND, 0);
			st(S.ctr + C_NEXT, 0);
		}
		__syncthreads();
		cur ^= 1;
		f = next;
		levels++;
	}
	if (t0 == 0) {
		st(S.ctr + C_CUR, cur);
		st(S.ctr + C_FRONT, f);
		st(S.ctr + C_LEVELS, levels);
	}
}

// the roots of a phase: every free x with a neighbour
__global__ void dm_roots_kernel(Side G, Search S)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= G.nx || G.mx[x] >= 0 || G.gp[x + 1] == G.gp[x])
		return;
	S.root[x] = x;
	S.buf0[atomicAdd(S.ctr + C_NEXT, 1)] = x;
}

// one lane per root whose tree ended in a free y: flips the path (the trees are disjoint: no two lanes touch the same vertex)
__global__ void dm_augment_kernel(Side G, Search S, int bound)
{
	const int x0 = blockIdx.x * blockDim.x + threadIdx.x;
	if (x0 >= G.nx)
		return;
	int y = S.end[x0];
	if (y == NONE)
		return;
	for (int steps = 0;; steps++) {
		const int x = S.parent[y];
		const int prev = G.mx[x];
		G.mx[x] = y;
		G.my[y] = x;
		if (x == x0)
			break;
		if (prev < 0 || steps >= bound) {
			atomicOr(S.ctr + C_ERR, ERR_PATH);
			return;
		}
		y = prev;
	}
	atomicAdd(S.ctr + C_AUG, 1);
}

__global__ void dm_greedy_claim_kernel(Side G, int *claim)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= G.nx || G.mx[x] >= 0)
		return;
	int best = NONE;
	for (int64_t e = G.gp[x]; e < G.gp[x + 1]; e++) {
		const int y = G.gj[e];
		if (G.my[y] < 0)
			best = min(best, y);
	}
	if (best != NONE)
		atomicMin(claim + best, x);
}

__global__ void dm_greedy_take_kernel(Side G, int *claim, int *ctr)
{
	const int y = blockIdx.x * blockDim.x + threadIdx.x;
	if (y >= G.ny)
		return;
	const int x = claim[y];
	if (x == NONE)
		return;
	claim[y] = NONE;
	G.my[y] = x;
	G.mx[x] = y;
	atomicAdd(ctr + C_NEW, 1);
}

inline unsigned blocks_for(int64_t threads) { return (unsigned) std::max<int64_t>((threads + 255) / 256, 1); }

struct PhaseResult {
	int augmented = 0;
	long long levels = 0, small_levels = 0;
};

// one phase on G: BFS from all free xs, then every path found is augmented.  S.seen is left with the ys it reached.
PhaseResult run_phase(const Side &G, const Search &S, hipStream_t stream, const char *who)
{
	PhaseResult R;
	HIP_CHECK(hipMemsetAsync(S.parent, 0x7f, (size_t) std::max(G.ny, 1) * 4, stream));
	HIP_CHECK(hipMemsetAsync(S.seen, 0, (size_t) std::max(G.ny, 1) * 4, stream));
	HIP_CHECK(hipMemsetAsync(S.end, 0x7f, (size_t) std::max(G.nx, 1) * 4, stream));
	HIP_CHECK(hipMemsetAsync(S.ctr, 0, C_COUNT * 4, stream));
	if (G.nx > 0)
		hipLaunchKernelGGL(dm_roots_kernel, dim3(blocks_for(G.nx)), dim3(256), 0, stream, G, S);
	HIP_CHECK(hipGetLastError());
	int ctr[C_COUNT];
	d2h(ctr, S.ctr, sizeof(ctr), stream);
	int f = ctr[C_NEXT], cur = 0, levels = 0;
	const int max_levels = G.ny + 2;                     // a level that goes on has reached a y no earlier level reached
	while (f > 0) {
		HIP_CHECK(hipMemsetAsync(S.ctr, 0, 2 * 4, stream));          // C_NEXT, C_FOUND
		if (f <= SMALL) {
			hipLaunchKernelGGL(dm_levels_small_kernel, dim3(1), dim3(SMALL_THREADS), 0, stream, G, S, cur, f, levels, max_levels);
			HIP_CHECK(hipGetLastError());
			d2h(ctr, S.ctr, sizeof(ctr), stream);
			if (ctr[C_ERR] != 0)
				die("%s: an alternating search passed its bound of %d levels", who, max_levels);
			R.small_levels += ctr[C_LEVELS] - levels;
			cur = ctr[C_CUR];
			f = ctr[C_FRONT];
			levels = ctr[C_LEVELS];
		} else {
			if (levels >= max_levels)
				die("%s: an alternating search passed its bound of %d levels", who, max_levels);
			hipLaunchKernelGGL(dm_expand_kernel, dim3(blocks_for(f)), dim3(256), 0, stream, G, S, cur ? S.buf1 : S.buf0, f);
			hipLaunchKernelGGL(dm_settle_kernel, dim3(blocks_for(std::min<int64_t>(G.ny, 1 << 20))), dim3(256), 0, stream, G, S,
			                   cur ? S.buf0 : S.buf1);
			HIP_CHECK(hipGetLastError());
			d2h(ctr, S.ctr, sizeof(ctr), stream);
			cur ^= 1;
			f = ctr[C_NEXT];
			levels++;
		}
	}
	R.levels = levels;
	if (G.nx > 0)
		hipLaunchKernelGGL(dm_augment_kernel, dim3(blocks_for(G.nx)), dim3(256), 0, stream, G, S, G.nx + G.ny);
	HIP_CHECK(hipGetLastError());
	d2h(ctr, S.ctr, sizeof(ctr), stream);
	if (ctr[C_ERR] != 0)
		die("%s: an augmenting path passed its bound of %d steps", who, G.nx + G.ny);
	R.augmented = ctr[C_AUG];
	return R;
}

}  // namespace

int dm_match(const struct spasm_csr *A, const char *who, int *jmatch, int *imatch, std::vector<char> *row_r1, std::vector<char> *col_c3,
             DmMatchStats *stats)
{
	check_host_csr(A, who);
	if (spasm_hip_device_count() == 0)
		die("%s: no HIP device (this library has no CPU path)", who);
	const int n = A->n, m = A->m;
	DmMatchStats St;
	hipStream_t stream = 0;
	double t0 = wtime();
	const int nm = std::max(std::max(n, m), 1);
	CsrUpload dA(A, false);
	const int64_t nnz = dA.nnz;
	int64_t *const d_Ap = dA.p;
	int *const d_Aj = dA.j;
	const size_t ents = (size_t) std::max<int64_t>(nnz, 1);
	int64_t *d_Cp = (int64_t *) big_alloc((size_t) (m + 1) * 8);
	int *d_Ci = (int *) big_alloc(ents * 4);
	int *d_jmatch = (int *) big_alloc((size_t) std::max(n, 1) * 4);
	int *d_imatch = (int *) big_alloc((size_t) std::max(m, 1) * 4);
	int *d_ws = (int *) big_alloc((size_t) nm * 4 * 7 + C_COUNT * 4);
	Search S;
	S.parent = d_ws;
	S.seen = d_ws + nm;
	S.root = d_ws + 2 * (size_t) nm;
	S.end = d_ws + 3 * (size_t) nm;
	S.found = d_ws + 4 * (size_t) nm;
	S.buf0 = d_ws + 5 * (size_t) nm;
	S.buf1 = d_ws + 6 * (size_t) nm;
	S.ctr = d_ws + 7 * (size_t) nm;
	dA.send(A, stream);
	// the column-major pattern; its count / fill counters borrow the phase workspace
	HIP_CHECK(hipMemsetAsync(S.ctr, 0, 4, stream));
	colmajor_count_scan(d_Ap, d_Aj, n, m, nnz, (uint32_t *) S.parent, S.ctr, d_Cp, stream);
	colmajor_fill(d_Ap, d_Aj, n, m, nnz, d_Cp, (uint32_t *) S.parent, d_Ci, NoValues{}, stream);
	HIP_CHECK(hipGetLastError());
	int bad = 0;
	d2h(&bad, S.ctr, sizeof(bad), stream);
	if (bad != 0) {
		for (void *q : {(void *) d_Cp, (void *) d_Ci, (void *) d_jmatch, (void *) d_imatch, (void *) d_ws})
			big_free(q);
		die("%s: a column index of A lies outside [0, %d)", who, m);
	}
	HIP_CHECK(hipMemsetAsync(d_jmatch, 0xff, (size_t) std::max(n, 1) * 4, stream));
	HIP_CHECK(hipMemsetAsync(d_imatch, 0xff, (size_t) std::max(m, 1) * 4, stream));
	HIP_CHECK(hipStreamSynchronize(stream));
	double t1 = wtime();
	St.upload_ms = (t1 - t0) * 1e3;

	const Side rows{d_Ap, d_Aj, n, m, d_jmatch, d_imatch};
	const Side cols{d_Cp, d_Ci, m, n, d_imatch, d_jmatch};
	const Side &G = n <= m ? rows : cols;
	// greedy rounds
	HIP_CHECK(hipMemsetAsync(S.parent, 0x7f, (size_t) nm * 4, stream));
	int ctr[C_COUNT];
	for (int round = 0; round < GREEDY_ROUNDS && nnz > 0; round++) {
		HIP_CHECK(hipMemsetAsync(S.ctr, 0, C_COUNT * 4, stream));
		hipLaunchKernelGGL(dm_greedy_claim_kernel, dim3(blocks_for(G.nx)), dim3(256), 0, stream, G, S.parent);
		hipLaunchKernelGGL(dm_greedy_take_kernel, dim3(blocks_for(G.ny)), dim3(256), 0, stream, G, S.parent, S.ctr);
		HIP_CHECK(hipGetLastError());
		d2h(ctr, S.ctr, sizeof(ctr), stream);
		St.greedy_size += ctr[C_NEW];
		if ((int64_t) ctr[C_NEW] * 256 <= G.nx)               // the rounds have stopped paying
			break;
	}
	double t2 = wtime();
	St.greedy_ms = (t2 - t1) * 1e3;
	// augmenting phases until one finds nothing
	St.size = St.greedy_size;
	for (;;) {
		if (St.phases > std::min(G.nx, G.ny) + 1)
			die("%s: %d augmenting phases, more than a maximum matching needs", who, St.phases);
		const PhaseResult R = run_phase(G, S, stream, who);
		St.phases++;
		St.levels += R.levels;
		St.small_levels += R.small_levels;
		St.size += R.augmented;
		if (R.augmented == 0)
			break;
	}
	double t3 = wtime();
	St.phases_ms = (t3 - t2) * 1e3;
	if (row_r1 != nullptr && col_c3 != nullptr) {
		// the last phase reached the ys of G from its free xs; one phase on the other orientation reaches the other set
		std::vector<int> reach_g((size_t) G.ny), reach_o((size_t) G.nx);
		if (G.ny > 0)
			d2h(reach_g.data(), S.seen, (size_t) G.ny * 4, stream);
		const Side &O = n <= m ? cols : rows;
		const PhaseResult R = run_phase(O, S, stream, who);
		if (R.augmented != 0)
			die("%s: the matching is not maximum (%d augmenting paths from the other side)", who, R.augmented);
		St.levels += R.levels;
		St.small_levels += R.small_levels;
		if (O.ny > 0)
			d2h(reach_o.data(), S.seen, (size_t) O.ny * 4, stream);
		const std::vector<int> &c3 = n <= m ? reach_g : reach_o, &r1 = n <= m ? reach_o : reach_g;
		row_r1->assign((size_t) n, 0);
		col_c3->assign((size_t) m, 0);
		for (int i = 0; i < n; i++)
			(*row_r1)[i] = (char) (r1[i] != 0);
		for (int j = 0; j < m; j++)
			(*col_c3)[j] = (char) (c3[j] != 0);
	}
	if (n > 0)
		d2h(jmatch, d_jmatch, (size_t) n * 4, stream);
	if (m > 0)
		d2h(imatch, d_imatch, (size_t) m * 4, stream);
	St.reach_ms = (wtime() - t3) * 1e3;
	for (void *q : {(void *) d_Cp, (void *) d_Ci, (void *) d_jmatch, (void *) d_imatch, (void *) d_ws})
		big_free(q);
	if (stats != nullptr)
		*stats = St;
	return St.size;
}

}  // namespace sh
