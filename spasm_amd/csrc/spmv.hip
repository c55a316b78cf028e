// Y = X.A + Y mod p for k dense vectors X (k x n) and a CSR matrix A (n x m) -- replaces spasm_xApy (spasm_spmv.c:9-21), all k
// vectors in one pass over A.  The products behind the rank certificates (host_cert.cpp) and the factorization checks.
//
// Pull form.  A is first turned into a column-major image on the device (colmajor.h): row index and value * 2^32 mod p of every
// entry.  The order of the entries inside a column is whatever the fill produced; integer sums mod p are exact in any order,
// so the result does not depend on it.  Then every output Y[v][j] is written once, by plain stores:
//   short columns (at most XA_LONG entries): one lane per (column, vector), the lane walks the column;
//   long columns: one wave per column, the lanes stride the column, a wave reduction, lane 0 writes.
// The columns are put in the two lists by a kernel that reads the column pointers, the empty columns among the short ones.
// Vectors are stored unknown-major on the device (X[i * k + v], Y[j * k + v]): the k lanes of one column read k adjacent words.
// Products are montmul(x, a * 2^32) = x * a mod p in [0, p); sums are kept in 64 bits and reduced once (reduce_sum).  Any odd
// p < 2^32.
#include <algorithm>
#include <mutex>

#include "colmajor.h"
#include "field_dev.h"
#include "xa.h"

namespace sh {

namespace {

constexpr int XA_LONG = 32;          // a column with more entries than this gets a whole wave
constexpr int XA_WAVES = 4;          // waves per workgroup of the long-column kernel
constexpr int XA_CHUNK = 4;          // vectors a lane of the long-column kernel carries at once

__device__ __forceinline__ uint32_t addmod(uint32_t a, uint32_t b, const MontDev &F)
{
	const uint32_t c = F.p - b;
	return (a >= c) ? a - c : a + b;
}

// one lane per (column of the short list, vector): t = c * k + v
__global__ void xa_short_kernel(const int *cols, int ncols, const int64_t *cp, const int *ri, const uint32_t *val, int k,
                                const uint32_t *X, uint32_t *Y, MontDev F)
{
	const int64_t t = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
	if (t >= (int64_t) ncols * k)
		return;
	const int c = (int) (t / k), v = (int) (t - (int64_t) c * k);
	const int j = cols[c];
	unsigned long long acc = 0;
	for (int64_t e = cp[j]; e < cp[j + 1]; e++)
		acc += montmul(X[(int64_t) ri[e] * k + v], val[e], F);
	uint32_t *y = Y + (int64_t) j * k + v;
	*y = addmod(*y, reduce_sum(acc, F), F);
}

// one wave per column of the long list; the vectors XA_CHUNK at a time
__global__ __launch_bounds__(64 * XA_WAVES) void xa_long_kernel(const int *cols, int ncols, const int64_t *cp, const int *ri,
                                                                 const uint32_t *val, int k, const uint32_t *X, uint32_t *Y, MontDev F)
{
	const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * XA_WAVES + (int) (threadIdx.x >> 6)), lane = threadIdx.x & 63;
	if (c >= ncols)
		return;
	const int j = cols[c];
	const int64_t lo = cp[j], hi = cp[j + 1];
	for (int v0 = 0; v0 < k; v0 += XA_CHUNK) {
		const int nv = min(XA_CHUNK, k - v0);
		unsigned long long acc[XA_CHUNK] = {0, 0, 0, 0};
		for (int64_t e = lo + lane; e < hi; e += 64) {
			const int64_t xi = (int64_t) ri[e] * k + v0;
			const uint32_t a = val[e];
#pragma unroll
			for (int u = 0; u < XA_CHUNK; u++)
				if (u < nv)
					acc[u] += montmul(X[xi + u], a, F);
		}
#pragma unroll
		for (int u = 0; u < XA_CHUNK; u++) {
			uint32_t s = reduce_sum(acc[u], F);
			for (int off = 32; off > 0; off >>= 1)
				s = addmod(s, (uint32_t) __shfl_xor((int) s, off, 64), F);
			if (lane == 0 && u < nv) {
				uint32_t *y = Y + (int64_t) j * k + v0 + u;
				*y = addmod(*y, s, F);
			}
		}
	}
}

inline uint32_t canonical(int64_t p, int64_t a)
{
	a %= p;
	return (uint32_t) (a < 0 ? a + p : a);
}

std::mutex xa_stats_mutex;
double xa_last[8];

}  // namespace

struct XaPlan {
	int n = 0, m = 0;
	int64_t nnz = 0;
	int64_t prime = 0;
	Mont M;
	int64_t *cp = nullptr;       // m + 1 column pointers
	int *ri = nullptr;           // row of each entry, column-major
	uint32_t *val = nullptr;     // value * 2^32 mod p
	int *cols = nullptr;         // short columns, then long columns
	int nshort = 0, nlong = 0;
	double build_ms = 0, upload_ms = 0;
};

XaPlan *xa_plan_create(const struct spasm_csr *A, const char *who)
{
	check_host_csr(A, who);
	if (spasm_hip_device_count() == 0)
		die("%s: no HIP device (this library has no CPU path)", who);
	const int64_t prime = A->field->p;
	if (prime < 3 || prime > 0xfffffffbLL || (prime & 1) == 0)
		die("%s: modulus %lld unsupported on the GPU path", who, (long long) prime);
	const int n = A->n, m = A->m;
	CsrUpload dA(A, true);
	const int64_t nnz = dA.nnz;
	XaPlan *P = new XaPlan();
	P->n = n;
	P->m = m;
	P->nnz = nnz;
	P->prime = prime;
	P->M = mont_setup(prime);
	hipStream_t stream = 0;
	hipEvent_t ev[3];
	for (auto &e : ev)
		HIP_CHECK(hipEventCreate(&e));
	uint32_t *d_work = (uint32_t *) big_alloc((size_t) std::max(m, 1) * 4 * 2);     // the builder's counts and positions
	int *d_flags = (int *) big_alloc(4 * 4);                                         // bad, short count, long count, (longest)
	P->cp = (int64_t *) big_alloc((size_t) (m + 1) * 8);
	P->ri = (int *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4);
	P->val = (uint32_t *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4);
	P->cols = (int *) big_alloc((size_t) std::max(m, 1) * 4 * 2);
	HIP_CHECK(hipEventRecord(ev[0], stream));
	dA.send(A, stream);
	HIP_CHECK(hipEventRecord(ev[1], stream));
	HIP_CHECK(hipMemsetAsync(d_flags, 0, 4 * 4, stream));
	colmajor_count_scan(dA.p, dA.j, n, m, nnz, d_work, d_flags, P->cp, stream);
	colmajor_fill(dA.p, dA.j, n, m, nnz, P->cp, d_work, P->ri, MontValues{dA.x, P->val, to_dev(P->M)}, stream);
	colmajor_bucket(P->cp, m, XA_LONG, true, P->cols, P->cols + m, d_flags + 1, stream);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(ev[2], stream));
	int flags[4];
	d2h(flags, d_flags, sizeof(flags), stream);
	float e01 = 0, e12 = 0;
	HIP_CHECK(hipEventElapsedTime(&e01, ev[0], ev[1]));
	HIP_CHECK(hipEventElapsedTime(&e12, ev[1], ev[2]));
	for (auto &e : ev)
		HIP_CHECK(hipEventDestroy(e));
	big_free(d_work);
	big_free(d_flags);
	if (flags[0] != 0) {
		xa_plan_destroy(P);
		die("%s: a column index of A lies outside [0, %d)", who, m);
	}
	P->nshort = flags[1];
	P->nlong = flags[2];
	if (P->nlong > 0)             // the long list sits at cols + m: bring it next to the short one
		HIP_CHECK(hipMemcpyAsync(P->cols + P->nshort, P->cols + m, (size_t) P->nlong * 4, hipMemcpyDeviceToDevice, stream));
	P->upload_ms = e01;
	P->build_ms = e12;
	return P;
}

void xa_plan_destroy(XaPlan *P)
{
	if (P == nullptr)
		return;
	HIP_CHECK(hipStreamSynchronize(0));
	for (void *q : {(void *) P->cp, (void *) P->ri, (void *) P->val, (void *) P->cols})
		big_free(q);
	delete P;
}

// Y (k x m, row-major) += X (k x n, row-major) . A; values balanced or any other representative
void xa_plan_apply(XaPlan *P, int k, const spasm_ZZp *X, spasm_ZZp *Y)
{
	if (k < 0)
		die("spasm_hip_xApy_batch: k = %d", k);
	const int n = P->n, m = P->m;
	if (k == 0 || m == 0)
		return;
	const int64_t p = P->prime;
	std::vector<uint32_t> Xh((size_t) n * k), Yh((size_t) m * k);
	for (int v = 0; v < k; v++)
		for (int i = 0; i < n; i++)
			Xh[(size_t) i * k + v] = canonical(p, X[(size_t) v * n + i]);
	for (int v = 0; v < k; v++)
		for (int j = 0; j < m; j++)
			Yh[(size_t) j * k + v] = canonical(p, Y[(size_t) v * m + j]);
	const MontDev F = to_dev(P->M);
	hipStream_t stream = 0;
	uint32_t *d_X = (uint32_t *) big_alloc(std::max<size_t>((size_t) n * k, 1) * 4);
	uint32_t *d_Y = (uint32_t *) big_alloc((size_t) m * k * 4);
	if (n > 0)
		h2d(d_X, Xh.data(), (size_t) n * k * 4, stream);
	h2d(d_Y, Yh.data(), (size_t) m * k * 4, stream);
	hipEvent_t ev[2];
	for (auto &e : ev)
		HIP_CHECK(hipEventCreate(&e));
	HIP_CHECK(hipEventRecord(ev[0], stream));
	const int64_t short_threads = (int64_t) P->nshort * k;
	if (short_threads > 0)
		hipLaunchKernelGGL(xa_short_kernel, dim3((unsigned) ((short_threads + 255) / 256)), dim3(256), 0, stream, P->cols, P->nshort, P->cp,
		                   P->ri, P->val, k, d_X, d_Y, F);
	if (P->nlong > 0)
		hipLaunchKernelGGL(xa_long_kernel, dim3((P->nlong + XA_WAVES - 1) / XA_WAVES), dim3(64 * XA_WAVES), 0, stream, P->cols + P->nshort,
		                   P->nlong, P->cp, P->ri, P->val, k, d_X, d_Y, F);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(ev[1], stream));
	d2h(Yh.data(), d_Y, (size_t) m * k * 4, stream);
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	for (auto &e : ev)
		HIP_CHECK(hipEventDestroy(e));
	big_free(d_X);
	big_free(d_Y);
	for (int v = 0; v < k; v++)
		for (int j = 0; j < m; j++) {
			const uint32_t u = Yh[(size_t) j * k + v];
			Y[(size_t) v * m + j] = (u > P->M.half) ? (spasm_ZZp) ((int64_t) u - p) : (spasm_ZZp) u;
		}
	// algorithmic bytes: per entry its row index, its value and k gathered words of X; per column its two pointers and k words
	// of Y read and written
	const double bytes = (double) P->nnz * (8.0 + 4.0 * k) + (double) m * (16.0 + 8.0 * k);
	std::lock_guard<std::mutex> guard(xa_stats_mutex);
	xa_last[0] = P->upload_ms;
	xa_last[1] = P->build_ms;
	xa_last[2] = ms;
	xa_last[3] = bytes;
	xa_last[4] = k;
	xa_last[5] = P->nshort;
	xa_last[6] = P->nlong;
	xa_last[7] = (double) P->nnz;
}

}  // namespace sh

using namespace sh;

extern "C" {

void spasm_hip_xApy_batch(const struct spasm_csr *A, int k, const spasm_ZZp *X, spasm_ZZp *Y)
{
	XaPlan *P = xa_plan_create(A, "spasm_hip_xApy_batch");
	xa_plan_apply(P, k, X, Y);
	xa_plan_destroy(P);
}

void spasm_hip_xApy(const spasm_ZZp *x, const struct spasm_csr *A, spasm_ZZp *y)
{
	spasm_hip_xApy_batch(A, 1, x, y);
}

int spasm_hip_xApy_stats(double *out, int count)
{
	std::lock_guard<std::mutex> guard(xa_stats_mutex);
	for (int t = 0; t < std::min(count, 8); t++)
		out[t] = xa_last[t];
	return 8;
}

}  // extern "C"
