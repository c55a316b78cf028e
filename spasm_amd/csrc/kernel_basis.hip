// A basis of the right kernel of the factor's U, formed on the device: the array spasm_hip_kernel (host_echelonize.cpp) returns on
// the same fact, bit for bit.  Row k of K belongs to the k-th non-pivotal column j:  -e_j + sum_i R[i][j] e_{pivot(i)}, R the
// reduced rows of U.
//
// What runs where.  Host: the rows of U without their pivot entries (the input of the reduction), the lists of pivotal and
// non-pivotal columns, the plan of the factor image (spasm_hip_dfact_create).  Device: S = those rows reduced against the whole of
// U (spasm_hip_dschur, every row of U at once; a pool that was too small: again with a larger one), S^T in the stable order
// (transpose.hip), and the assembly.  S has no entry on a pivotal column, so the row pointers of S^T over the non-pivotal columns
// are those of K but for the one (j, -1) that opens every row: Kp[k] = S^Tp[j_k] + k.  Every entry of K is written once; the entries
// of a row come by increasing row i of U, as the stable transposition left them, relabelled pivot(i).  One download at the end.
#include <algorithm>
#include <cinttypes>
#include <mutex>
#include <vector>

#include "device_types.h"

namespace sh {

// transpose.hip
void dtranspose_run(const spasm_hip_dcsr *A, int keep_values, int64_t *d_Tp, int *d_Tj, int *d_Tx, hipStream_t stream, const char *who,
                    double *ms, double *counts);

namespace {

constexpr int KB_MAX_BLOCKS = 1 << 20;

// a pivotal column that holds an entry of S: the reduction did not clear it (*bad = 1)
__global__ void kb_check_kernel(const int64_t *Stp, const int *piv, int n, int *bad)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && Stp[piv[i] + 1] != Stp[piv[i]])
		atomicOr(bad, 1);
}

// rows k = blockIdx.x, + gridDim.x, ... of K; the entries of a row are shared by the gridDim.y workgroups of its column of the grid
__global__ __launch_bounds__(256) void kb_assemble_kernel(const int64_t *Stp, const int *Stj, const int *Stx, const int *nonpiv, int Kn,
                                                          const int *piv, int minus_one, int64_t *Kp, int *Kj, int *Kx)
{
	for (int k = blockIdx.x; k < Kn; k += gridDim.x) {
		const int j = nonpiv[k];
		const int64_t lo = Stp[j], hi = Stp[j + 1];
		if (blockIdx.y == 0 && threadIdx.x == 0) {
			Kp[k] = lo + k;
			Kj[lo + k] = j;
			Kx[lo + k] = minus_one;
			if (k == Kn - 1)
				Kp[Kn] = hi + Kn;
		}
		for (int64_t e = lo + (int64_t) blockIdx.y * 256 + threadIdx.x; e < hi; e += (int64_t) gridDim.y * 256) {
			Kj[e + k + 1] = piv[Stj[e]];
			Kx[e + k + 1] = Stx[e];
		}
	}
}

std::mutex kb_stats_mutex;
double kb_last[9];

template <typename T> T *dalloc(int64_t count)
{
	return static_cast<T *>(big_alloc((size_t) (count > 0 ? count : 1) * sizeof(T)));
}

}  // namespace

}  // namespace sh

using namespace sh;

extern "C" {

struct spasm_csr *spasm_hip_kernel_basis(const struct spasm_lu *fact)
{
	const char *who = "spasm_hip_kernel_basis";
	if (fact == nullptr || fact->U == nullptr || fact->qinv == nullptr)
		die("%s: the factorization, its U or its qinv is NULL", who);
	if (spasm_hip_device_count() == 0)
		die("%s: no HIP device (this library has no CPU path)", who);
	const struct spasm_csr *U = fact->U;
	const int n = U->n, m = U->m;
	const i64 prime = U->field->p;
	if (prime < 3 || prime > 0xfffffffbLL || (prime & 1) == 0)
		die("%s: modulus %lld unsupported on the GPU path", who, (long long) prime);
	if (n < 0 || m < 0 || n > m)
		die("%s: U is %d x %d", who, n, m);
	const double t_begin = wtime();
	double stage[5] = {0, 0, 0, 0, 0};
	int retries = 0;
	// pivotal and non-pivotal columns (the pivot of a row of U is its first entry)
	std::vector<int> piv((size_t) std::max(n, 1)), nonpiv;
	std::vector<char> pivotal((size_t) std::max(m, 1), 0);
	for (int i = 0; i < n; i++) {
		if (U->p[i] >= U->p[i + 1])
			die("%s: row %d of U is empty", who, i);
		const int c = U->j[U->p[i]];
		if (c < 0 || c >= m || pivotal[c])
			die("%s: row %d of U has its pivot on column %d (outside [0, %d), or the pivot of an earlier row)", who, i, c, m);
		pivotal[c] = 1;
		piv[i] = c;
	}
	const int Kn = m - n;
	nonpiv.reserve((size_t) std::max(Kn, 1));
	for (int j = 0; j < m; j++)
		if (!pivotal[j])
			nonpiv.push_back(j);
	const i64 nnzT = U->p[n] - n;
	hipStream_t stream = 0;
	struct spasm_csr *K = nullptr;
	if (Kn == 0) {                  // full column rank: no rows
		K = spasm_hip_csr_alloc(0, m, 0, prime, true);
	} else {
		// ---- [0] uploads + factor image ----
		i64 *d_Sp = dalloc<i64>((i64) n + 1);
		int *d_Sj = nullptr, *d_Sx = nullptr;
		i64 nnzS = 0;
		int *d_piv = dalloc<int>(n), *d_nonpiv = dalloc<int>(Kn);
		if (n > 0)
			h2d(d_piv, piv.data(), (size_t) n * 4, stream);
		h2d(d_nonpiv, nonpiv.data(), (size_t) Kn * 4, stream);
		if (n > 0 && nnzT > 0) {
			std::vector<i64> Tp((size_t) n + 1);
			std::vector<int> Tj((size_t) nnzT), Tx((size_t) nnzT), rows((size_t) n);
			i64 w = 0;
			Tp[0] = 0;
			for (int i = 0; i < n; i++) {
				rows[i] = i;
				for (i64 px = U->p[i] + 1; px < U->p[i + 1]; px++) {
					Tj[w] = U->j[px];
					Tx[w] = U->x[px];
					w += 1;
				}
				Tp[i + 1] = w;
			}
			i64 *d_Tp = dalloc<i64>((i64) n + 1);
			int *d_Tj = dalloc<int>(nnzT), *d_Tx = dalloc<int>(nnzT), *d_rows = dalloc<int>(n);
			h2d(d_Tp, Tp.data(), (size_t) (n + 1) * 8, stream);
			h2d(d_Tj, Tj.data(), (size_t) nnzT * 4, stream);
			h2d(d_Tx, Tx.data(), (size_t) nnzT * 4, stream);
			h2d(d_rows, rows.data(), (size_t) n * 4, stream);
			spasm_hip_dfact *F = spasm_hip_dfact_create(U, fact->qinv, stream);
			HIP_CHECK(hipStreamSynchronize(stream));
			stage[0] = (wtime() - t_begin) * 1e3;
			// ---- [1] the rows of R: S = T reduced against U ----
			const double t1 = wtime();
			const spasm_hip_dcsr dT{n, m, nnzT, d_Tp, d_Tj, d_Tx};
			// the pool as spasm_hip_schur sizes it without a density estimate; never more than the dense size (+ what the waves
			// strand in their arenas), which also bounds the retries.  SPASM_HIP_KERNEL_POOL: the first pool, for the tests
			const i64 pool_max = (i64) n * (i64) Kn + (i64) 4096 * 4096;
			i64 pool = std::min<i64>(pool_max, 4 * nnzT + (i64) 4096 * 4096);
			if (env_int("SPASM_HIP_KERNEL_POOL", 0) > 0)
				pool = std::min<i64>(pool_max, env_int("SPASM_HIP_KERNEL_POOL", 0));
			spasm_hip_schur_stats st{};
			spasm_hip_dwork *W = nullptr;
			for (;;) {
				W = spasm_hip_dwork_create(n, m, pool);
				W->scratch_budget = (i64) 24 << 30;          // (as spasm_hip_schur: a one-shot call does not map half the HBM)
				const int rc = spasm_hip_dschur(&dT, d_rows, n, F, W, stream, &st);
				if (rc == 0)
					break;
				spasm_hip_dwork_destroy(W);
				if (rc != 1 || pool >= pool_max)
					die("%s: spasm_hip_dschur returned %d with a pool of %" PRId64 " entries", who, rc, pool);
				pool = std::min<i64>(pool_max, 2 * pool + m);
				retries += 1;
				logmsg("[kernel/hip] pool too small, retrying with %" PRId64 " entries\n", pool);
			}
			nnzS = st.nnz;
			d_Sj = dalloc<int>(nnzS);
			d_Sx = dalloc<int>(nnzS);
			spasm_hip_dschur_fetch(W, d_Sp, d_Sj, d_Sx, stream);          // (synchronises the stream)
			spasm_hip_dwork_destroy(W);
			spasm_hip_dfact_destroy(F);
			for (void *q : {(void *) d_Tp, (void *) d_Tj, (void *) d_Tx, (void *) d_rows})
				big_free(q);
			stage[1] = (wtime() - t1) * 1e3;
		} else {
			HIP_CHECK(hipMemsetAsync(d_Sp, 0, (size_t) (n + 1) * 8, stream));
			d_Sj = dalloc<int>(0);
			d_Sx = dalloc<int>(0);
			HIP_CHECK(hipStreamSynchronize(stream));
			stage[0] = (wtime() - t_begin) * 1e3;
		}
		// ---- [2] S^T, stable ----
		const double t2 = wtime();
		i64 *d_Stp = dalloc<i64>((i64) m + 1);
		int *d_Stj = dalloc<int>(nnzS), *d_Stx = dalloc<int>(nnzS);
		const spasm_hip_dcsr dS{n, m, nnzS, d_Sp, d_Sj, d_Sx};
		double tr_ms[3], tr_counts[4];
		dtranspose_run(&dS, 1, d_Stp, d_Stj, d_Stx, stream, who, tr_ms, tr_counts);
		stage[2] = (wtime() - t2) * 1e3;
		// ---- [3] assembly ----
		const double t3 = wtime();
		const i64 nnzK = nnzS + Kn;
		i64 *d_Kp = dalloc<i64>((i64) Kn + 1);
		int *d_Kj = dalloc<int>(nnzK), *d_Kx = dalloc<int>(nnzK), *d_bad = dalloc<int>(1);
		HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, stream));
		if (n > 0)
			hipLaunchKernelGGL(kb_check_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_Stp, d_piv, n, d_bad);
		const int gx = std::min(Kn, KB_MAX_BLOCKS);
		const int gy = (int) std::max<i64>(1, std::min<i64>({((i64) tr_counts[2] + 4095) / 4096, (i64) KB_MAX_BLOCKS / gx, (i64) 65535}));
		hipLaunchKernelGGL(kb_assemble_kernel, dim3(gx, gy), dim3(256), 0, stream, d_Stp, d_Stj, d_Stx, d_nonpiv, Kn, d_piv,
		                   (int) zp_init(prime, prime - 1), d_Kp, d_Kj, d_Kx);
		HIP_CHECK(hipGetLastError());
		int bad = 0;
		d2h(&bad, d_bad, sizeof(bad), stream);
		if (bad != 0)
			die("%s: the reduced rows of U keep an entry on a pivotal column", who);
		stage[3] = (wtime() - t3) * 1e3;
		// ---- [4] download ----
		const double t4 = wtime();
		K = spasm_hip_csr_alloc(Kn, m, nnzK, prime, true);
		d2h(K->p, d_Kp, (size_t) (Kn + 1) * 8, stream);
		d2h(K->j, d_Kj, (size_t) nnzK * 4, stream);
		d2h(K->x, d_Kx, (size_t) nnzK * 4, stream);
		stage[4] = (wtime() - t4) * 1e3;
		for (void *q : {(void *) d_Sp, (void *) d_Sj, (void *) d_Sx, (void *) d_piv, (void *) d_nonpiv, (void *) d_Stp, (void *) d_Stj,
		                (void *) d_Stx, (void *) d_Kp, (void *) d_Kj, (void *) d_Kx, (void *) d_bad})
			big_free(q);
	}
	std::lock_guard<std::mutex> guard(kb_stats_mutex);
	for (int t = 0; t < 5; t++)
		kb_last[t] = stage[t];
	kb_last[5] = (wtime() - t_begin) * 1e3;
	kb_last[6] = (double) K->p[K->n];
	kb_last[7] = retries;
	kb_last[8] = K->n;
	return K;
}

int spasm_hip_kernel_stats(double *out, int count)
{
	std::lock_guard<std::mutex> guard(kb_stats_mutex);
	for (int t = 0; t < std::min(count, 9); t++)
		out[t] = kb_last[t];
	return 9;
}

}  // extern "C"
