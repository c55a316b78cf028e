// T = A^T for a CSR matrix resident on the device, in the STABLE order: the entries of a row of T come by increasing row of A --
// the array spasm_transpose (spasm_transpose.c:5) and spasm_hip_transpose (host_util.cpp) return, bit for bit, whatever the launch.
//
// Count, scan, fill, order.  The first three are the column-major image of colmajor.h, built into a staging copy: the order
// inside the slice of a column is whatever the fill produced.  Then every slice is put in order by source row on its way from
// the staging copy to T, each entry moved once:
//   short slices (at most tr_short() entries): one wave per slice.  The keys go to LDS; every lane ranks its keys by counting the
//     smaller ones (broadcast reads, four keys per read).  A key that meets its own value twice is a repeated (i, j).
//   long slices: one workgroup per slice.  The keys of a slice are DISTINCT row indices in [0, n): the slice sets its bits in a
//     bitmap over a chunk of tr_chunk() rows held in LDS, one packed scan of the popcounts (16-bit offsets inside tiles of 256
//     words, one 32-bit base per tile) turns the bitmap into ranks, and every entry of the chunk finds its place with three LDS
//     reads.  Rows beyond one chunk: chunk by chunk with a running base.  Popcounts that do not add up to the length of the slice
//     are a repeated (i, j).
// The result depends on the keys alone (they are distinct inside a slice), not on the order the fill left: two calls return the
// same arrays.  Values travel with their keys as the 32-bit words they are.  No workgroup waits for another; every loop runs over
// the data it was given.
#include <algorithm>
#include <climits>
#include <mutex>

#include "colmajor.h"

namespace sh {

namespace {

constexpr int TR_SHORT_DEFAULT = 256;        // slices up to this length take the short route (SPASM_HIP_TRANSPOSE_SHORT)
constexpr int TR_SHORT_MAX = 1024;           // ... at most: 4 KB of keys per wave
constexpr int TR_CHUNK_MAX = 262144;         // rows per bitmap chunk (SPASM_HIP_TRANSPOSE_CHUNK): 32 KB of bits + 16 KB of offsets
constexpr int TR_WAVES = 4;                  // waves per workgroup of the short route

enum { TR_BAD = 0, TR_NSHORT, TR_NLONG, TR_LONGEST, TR_INFO };      // the words of d_info; TR_BAD bit 0: column index outside
                                                                  // [0, m), bit 1: a repeated (i, j); the next three in the
                                                                  // order of colmajor_bucket's counters

int tr_short()
{
	return std::max(1, std::min(TR_SHORT_MAX, env_int("SPASM_HIP_TRANSPOSE_SHORT", TR_SHORT_DEFAULT)));
}

int tr_chunk()
{
	const int c = std::max(32, std::min(TR_CHUNK_MAX, env_int("SPASM_HIP_TRANSPOSE_CHUNK", TR_CHUNK_MAX)));
	return (c + 31) & ~31;
}

// short route: one wave per slice of at most short_max <= L4 entries; L4 keys of LDS per wave, L4 a multiple of 4
__global__ __launch_bounds__(64 * TR_WAVES) void tr_short_kernel(const int *cols, int ncols, const int64_t *Tp, const int *sj, const int *sx,
                                                                 int *Tj, int *Tx, int L4, int *info)
{
	extern __shared__ __align__(16) int tr_keys[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int c = blockIdx.x * TR_WAVES + wave;
	int *keys = tr_keys + wave * L4;
	int64_t lo = 0;
	int len = 0;
	if (c < ncols) {
		const int j = cols[c];
		lo = Tp[j];
		len = (int) (Tp[j + 1] - lo);
	}
	const int len4 = (len + 3) & ~3;
	for (int t = lane; t < len4; t += 64)
		keys[t] = t < len ? sj[lo + t] : INT_MAX;          // (a row index is below n <= INT_MAX: the padding is larger than every key)
	__syncthreads();
	for (int t = lane; t < len; t += 64) {
		const int key = keys[t];
		int rank = 0, same = 0;
		for (int u = 0; u < len4; u += 4) {
			const int4 k = *reinterpret_cast<const int4 *>(keys + u);
			rank += (k.x < key) + (k.y < key) + (k.z < key) + (k.w < key);
			same += (k.x == key) + (k.y == key) + (k.z == key) + (k.w == key);
		}
		if (same != 1)
			atomicOr(&info[TR_BAD], 2);
		// rank < len in every case (the key itself is not smaller than itself): the store stays inside the slice
		Tj[lo + rank] = key;
		if (sx != nullptr)
			Tx[lo + rank] = sx[lo + t];
	}
}

// long route: one workgroup per slice
__global__ __launch_bounds__(256) void tr_long_kernel(const int *cols, const int64_t *Tp, const int *sj, const int *sx, int *Tj, int *Tx,
                                                      int n, int chunk, int *info)
{
	__shared__ uint32_t bm[TR_CHUNK_MAX / 32];              // bit d of the chunk: row r0 + d is in the slice
	__shared__ uint16_t pre[TR_CHUNK_MAX / 32];             // set bits in the words of the same tile of 256 words before this one (<= 8160)
	__shared__ uint32_t tile_base[TR_CHUNK_MAX / 32 / 256]; // set bits of the chunk before the tile
	__shared__ uint32_t wsum[4];
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int j = cols[blockIdx.x];
	const int64_t lo = Tp[j], len = Tp[j + 1] - lo;
	int64_t base = 0;                                       // entries of the slice in the chunks before this one
	for (int64_t r0 = 0; r0 < n; r0 += chunk) {
		const int rows = (n - r0 < chunk) ? (int) (n - r0) : chunk;
		const int words = (rows + 31) >> 5;
		for (int w = tid; w < words; w += 256)
			bm[w] = 0;
		__syncthreads();
		for (int64_t e = tid; e < len; e += 256) {
			const int64_t d = (int64_t) sj[lo + e] - r0;
			if (d >= 0 && d < rows)
				atomicOr(&bm[d >> 5], 1u << (d & 31));
		}
		__syncthreads();
		uint32_t in_chunk = 0;                              // (the same in every thread)
		for (int t0 = 0; t0 < words; t0 += 256) {
			const int w = t0 + tid;
			const uint32_t v = w < words ? (uint32_t) __popc(bm[w]) : 0u;
			uint32_t s = v;
			for (int off = 1; off < 64; off <<= 1) {
				const uint32_t u = (uint32_t) __shfl_up((int) s, off, 64);
				if (lane >= off)
					s += u;
			}
			if (lane == 63)
				wsum[wave] = s;
			__syncthreads();
			uint32_t before = 0;
			for (int k = 0; k < wave; k++)
				before += wsum[k];
			if (w < words)
				pre[w] = (uint16_t) (before + s - v);
			if (tid == 0)
				tile_base[t0 >> 8] = in_chunk;
			in_chunk += wsum[0] + wsum[1] + wsum[2] + wsum[3];
			__syncthreads();
		}
		if (in_chunk != 0)
			for (int64_t e = tid; e < len; e += 256) {
				const int r = sj[lo + e];
				const int64_t d = (int64_t) r - r0;
				if (d < 0 || d >= rows)
					continue;
				const int w = (int) (d >> 5);
				// (distinct keys: rank < len; repeated keys share bits: fewer ranks than entries, still inside the slice)
				const int64_t rank = base + tile_base[w >> 8] + pre[w] + __popc(bm[w] & ((1u << (d & 31)) - 1u));
				Tj[lo + rank] = r;
				if (sx != nullptr)
					Tx[lo + rank] = sx[lo + e];
			}
		base += in_chunk;
		__syncthreads();
	}
	if (tid == 0 && base != len)
		atomicOr(&info[TR_BAD], 2);
}

std::mutex tr_stats_mutex;
double tr_last[9];

}  // namespace

// the device part: everything on `stream`, which is synchronised before the return (the route lists and the verdict on the input
// are read back).  ms: [0] count + scan, [1] fill, [2] ordering; counts: [0] short, [1] long slices, [2] the longest, [3] row chunks
void dtranspose_run(const spasm_hip_dcsr *A, int keep_values, int64_t *d_Tp, int *d_Tj, int *d_Tx, hipStream_t stream, const char *who,
                    double *ms, double *counts)
{
	const int n = A->n, m = A->m;
	if (n < 0 || m < 0)
		die("%s: A is %d x %d", who, n, m);
	int64_t nnz = A->nnz;
	if (nnz < 0) {
		nnz = 0;
		if (n > 0)
			d2h(&nnz, A->p + n, sizeof(nnz), stream);
	}
	const bool vals = keep_values != 0 && A->x != nullptr;
	if (d_Tj == nullptr && nnz > 0)
		die("%s: no array for the column indices of the result", who);
	if (vals && d_Tx == nullptr && nnz > 0)
		die("%s: values asked for and no array to put them in", who);
	const int short_max = tr_short(), chunk = tr_chunk();
	const int mm = std::max(m, 1);
	uint32_t *d_work = (uint32_t *) big_alloc((size_t) mm * 4 * 2);                   // the builder's counts and positions
	int *d_info = (int *) big_alloc(TR_INFO * 4);
	int *d_cols = (int *) big_alloc((size_t) mm * 4 * 2);                           // short list, long list
	int *d_sj = (int *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4);
	int *d_sx = vals ? (int *) big_alloc((size_t) std::max<int64_t>(nnz, 1) * 4) : nullptr;
	hipEvent_t ev[4];
	for (auto &e : ev)
		HIP_CHECK(hipEventCreate(&e));
	HIP_CHECK(hipEventRecord(ev[0], stream));
	HIP_CHECK(hipMemsetAsync(d_info, 0, TR_INFO * 4, stream));
	colmajor_count_scan(A->p, A->j, n, m, nnz, d_work, d_info + TR_BAD, d_Tp, stream);
	HIP_CHECK(hipEventRecord(ev[1], stream));
	if (vals)
		colmajor_fill(A->p, A->j, n, m, nnz, d_Tp, d_work, d_sj, RawValues{A->x, d_sx}, stream);
	else
		colmajor_fill(A->p, A->j, n, m, nnz, d_Tp, d_work, d_sj, NoValues{}, stream);
	HIP_CHECK(hipEventRecord(ev[2], stream));
	colmajor_bucket(d_Tp, m, short_max, false, d_cols, d_cols + mm, d_info + TR_NSHORT, stream);
	HIP_CHECK(hipGetLastError());
	int info[TR_INFO];
	d2h(info, d_info, sizeof(info), stream);
	if ((info[TR_BAD] & 1) == 0) {
		if (info[TR_NSHORT] > 0) {
			const int L4 = (short_max + 3) & ~3;
			hipLaunchKernelGGL(tr_short_kernel, dim3((info[TR_NSHORT] + TR_WAVES - 1) / TR_WAVES), dim3(64 * TR_WAVES), (size_t) TR_WAVES * L4 * 4,
			                   stream, d_cols, info[TR_NSHORT], d_Tp, d_sj, d_sx, d_Tj, d_Tx, L4, d_info);
		}
		if (info[TR_NLONG] > 0)
			hipLaunchKernelGGL(tr_long_kernel, dim3(info[TR_NLONG]), dim3(256), 0, stream, d_cols + mm, d_Tp, d_sj, d_sx, d_Tj, d_Tx, n, chunk,
			                   d_info);
		HIP_CHECK(hipGetLastError());
	}
	HIP_CHECK(hipEventRecord(ev[3], stream));
	int bad = 0;
	d2h(&bad, d_info + TR_BAD, sizeof(bad), stream);
	float e01 = 0, e12 = 0, e23 = 0;
	HIP_CHECK(hipEventElapsedTime(&e01, ev[0], ev[1]));
	HIP_CHECK(hipEventElapsedTime(&e12, ev[1], ev[2]));
	HIP_CHECK(hipEventElapsedTime(&e23, ev[2], ev[3]));
	for (auto &e : ev)
		HIP_CHECK(hipEventDestroy(e));
	big_free(d_work);
	big_free(d_info);
	big_free(d_cols);
	big_free(d_sj);
	if (d_sx != nullptr)
		big_free(d_sx);
	if (bad & 1)
		die("%s: a column index of A lies outside [0, %d)", who, m);
	if (bad & 2)
		die("%s: A holds the same (row, column) twice: its transpose has no stable order", who);
	ms[0] = e01;
	ms[1] = e12;
	ms[2] = e23;
	counts[0] = info[TR_NSHORT];
	counts[1] = info[TR_NLONG];
	counts[2] = info[TR_LONGEST];
	counts[3] = info[TR_NLONG] > 0 ? (double) (((int64_t) n + chunk - 1) / chunk) : 0.0;
}

void transpose_record(double upload_ms, const double *ms, double download_ms, const double *counts)
{
	std::lock_guard<std::mutex> guard(tr_stats_mutex);
	tr_last[0] = upload_ms;
	for (int t = 0; t < 3; t++)
		tr_last[1 + t] = ms[t];
	tr_last[4] = download_ms;
	for (int t = 0; t < 4; t++)
		tr_last[5 + t] = counts[t];
}

}  // namespace sh

using namespace sh;

extern "C" {

int spasm_hip_dtranspose(const spasm_hip_dcsr *A, int keep_values, i64 *d_Tp, int *d_Tj, spasm_ZZp *d_Tx, void *stream)
{
	if (A == nullptr || d_Tp == nullptr)
		die("spasm_hip_dtranspose: A or the row pointers of the result are NULL");
	double ms[3], counts[4];
	dtranspose_run(A, keep_values, d_Tp, d_Tj, d_Tx, (hipStream_t) stream, "spasm_hip_dtranspose", ms, counts);
	transpose_record(0.0, ms, 0.0, counts);
	return 0;
}

struct spasm_csr *spasm_hip_transpose_device(const struct spasm_csr *A, int keep_values)
{
	const char *who = "spasm_hip_transpose_device";
	check_host_csr(A, who);
	if (spasm_hip_device_count() == 0)
		die("%s: no HIP device (this library has no CPU path)", who);
	const int n = A->n, m = A->m;
	const bool vals = keep_values != 0 && A->x != nullptr;
	hipStream_t stream = 0;
	CsrUpload up(A, vals);
	const i64 nnz = up.nnz;
	const size_t entries = (size_t) std::max<i64>(nnz, 1) * 4;
	i64 *d_Tp = (i64 *) big_alloc((size_t) (m + 1) * 8);
	int *d_Tj = (int *) big_alloc(entries);
	int *d_Tx = vals ? (int *) big_alloc(entries) : nullptr;
	const double t0 = wtime();
	up.send(A, stream);
	HIP_CHECK(hipStreamSynchronize(stream));
	const double t1 = wtime();
	const spasm_hip_dcsr dA{n, m, nnz, up.p, up.j, up.x};
	double ms[3], counts[4];
	dtranspose_run(&dA, keep_values, d_Tp, d_Tj, d_Tx, stream, who, ms, counts);
	const double t2 = wtime();
	struct spasm_csr *T = spasm_hip_csr_alloc(m, n, nnz, A->field->p, vals);
	d2h(T->p, d_Tp, (size_t) (m + 1) * 8, stream);
	if (nnz > 0) {
		d2h(T->j, d_Tj, (size_t) nnz * 4, stream);
		if (vals)
			d2h(T->x, d_Tx, (size_t) nnz * 4, stream);
	}
	transpose_record((t1 - t0) * 1e3, ms, (wtime() - t2) * 1e3, counts);
	big_free(d_Tp);
	big_free(d_Tj);
	if (d_Tx != nullptr)
		big_free(d_Tx);
	return T;
}

int spasm_hip_transpose_stats(double *out, int count)
{
	std::lock_guard<std::mutex> guard(tr_stats_mutex);
	for (int t = 0; t < std::min(count, 9); t++)
		out[t] = tr_last[t];
	return 9;
}

}  // extern "C"
