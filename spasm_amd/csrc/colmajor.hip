// The column-major image of a CSR matrix on the device: see colmajor.h.
#include <algorithm>

#include "colmajor.h"
#include "field_dev.h"

namespace sh {

namespace {

constexpr int CM_MAX_BLOCKS = 1 << 20;       // count and fill: grid-stride over the rows beyond this many workgroups

unsigned row_blocks(int n)
{
	return (unsigned) std::max<int64_t>(1, std::min<int64_t>(CM_MAX_BLOCKS, ((int64_t) n + 3) / 4));
}

__global__ __launch_bounds__(256) void colmajor_count_kernel(const int64_t *Ap, const int *Aj, int n, int m, uint32_t *cnt, int *bad)
{
	const int lane = threadIdx.x & 63;
	const int64_t waves = (int64_t) gridDim.x * 4;
	for (int64_t row = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves)
		for (int64_t px = Ap[row] + lane; px < Ap[row + 1]; px += 64) {
			const int j = Aj[px];
			if (j < 0 || j >= m) {
				atomicOr(bad, 1);
				continue;
			}
			atomicAdd(&cnt[j], 1u);
		}
}

template <typename T> __global__ __launch_bounds__(1024) void pointer_scan_kernel(const T *len, int n, int64_t *out)
{
	__shared__ int64_t s[1024];
	int64_t carry = 0;
	for (int base = 0; base < n; base += 1024) {
		const int t = base + (int) threadIdx.x;
		s[threadIdx.x] = t < n ? len[t] : 0;
		__syncthreads();
		for (int off = 1; off < 1024; off <<= 1) {
			const int64_t v = threadIdx.x >= (unsigned) off ? s[threadIdx.x - off] : 0;
			__syncthreads();
			s[threadIdx.x] += v;
			__syncthreads();
		}
		if (t < n)
			out[t + 1] = carry + s[threadIdx.x];
		carry += s[1023];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		out[0] = 0;
}

__device__ __forceinline__ void store_value(const NoValues &, int64_t, int64_t) {}
__device__ __forceinline__ void store_value(const RawValues &V, int64_t at, int64_t px) { V.out[at] = V.Ax[px]; }
__device__ __forceinline__ void store_value(const MontValues &V, int64_t at, int64_t px)
{
	int64_t a = V.Ax[px];
	if (a <= -(int64_t) V.F.p || a >= (int64_t) V.F.p) {
		a %= (int64_t) V.F.p;
	}
	const uint32_t u = a < 0 ? (uint32_t) (a + V.F.p) : (uint32_t) a;
	V.out[at] = montmul(u, V.F.r2, V.F);        // u * 2^32 mod p
}

template <typename V>
__global__ __launch_bounds__(256) void colmajor_fill_kernel(const int64_t *Ap, const int *Aj, int n, int m, const int64_t *cp, uint32_t *pos,
                                                            int *ri, V values)
{
	const int lane = threadIdx.x & 63;
	const int64_t waves = (int64_t) gridDim.x * 4;
	for (int64_t row = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves)
		for (int64_t px = Ap[row] + lane; px < Ap[row + 1]; px += 64) {
			const int j = Aj[px];
			if (j < 0 || j >= m)
				continue;
			const int64_t at = cp[j] + atomicAdd(&pos[j], 1u);
			ri[at] = (int) row;
			store_value(values, at, px);
		}
}

__global__ void colmajor_bucket_kernel(const int64_t *cp, int m, int threshold, bool list_empty, int *short_cols, int *long_cols, int *counters)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m)
		return;
	const int64_t len = cp[j + 1] - cp[j];
	if (len == 0 && !list_empty)
		return;
	atomicMax(&counters[2], (int) len);
	if (len > threshold)
		long_cols[atomicAdd(&counters[1], 1)] = j;
	else
		short_cols[atomicAdd(&counters[0], 1)] = j;
}

}  // namespace

CsrUpload::CsrUpload(const struct spasm_csr *A, bool values) : n(A->n), nnz(A->n > 0 ? A->p[A->n] : 0)
{
	const size_t entries = (size_t) std::max<int64_t>(nnz, 1) * 4;
	p = (int64_t *) big_alloc((size_t) (n + 1) * 8);
	j = (int *) big_alloc(entries);
	if (values)
		x = (int *) big_alloc(entries);
}

void CsrUpload::send(const struct spasm_csr *A, hipStream_t stream)
{
	if (n == 0) {
		HIP_CHECK(hipMemsetAsync(p, 0, 8, stream));
		return;
	}
	h2d(p, A->p, (size_t) (n + 1) * 8, stream);
	if (nnz > 0) {
		h2d(j, A->j, (size_t) nnz * 4, stream);
		if (x != nullptr)
			h2d(x, A->x, (size_t) nnz * 4, stream);
	}
}

CsrUpload::~CsrUpload()
{
	big_free(p);
	big_free(j);
	if (x != nullptr)
		big_free(x);
}

template <typename T> void launch_pointer_scan(const T *len, int n, int64_t *out, hipStream_t stream)
{
	hipLaunchKernelGGL(pointer_scan_kernel<T>, dim3(1), dim3(1024), 0, stream, len, n, out);
}
template void launch_pointer_scan<uint32_t>(const uint32_t *, int, int64_t *, hipStream_t);
template void launch_pointer_scan<int64_t>(const int64_t *, int, int64_t *, hipStream_t);

void colmajor_count_scan(const int64_t *Ap, const int *Aj, int n, int m, int64_t nnz, uint32_t *work, int *bad, int64_t *cp,
                         hipStream_t stream)
{
	HIP_CHECK(hipMemsetAsync(work, 0, (size_t) std::max(m, 1) * 4 * 2, stream));
	if (n > 0 && m > 0 && nnz > 0)
		hipLaunchKernelGGL(colmajor_count_kernel, dim3(row_blocks(n)), dim3(256), 0, stream, Ap, Aj, n, m, work, bad);
	launch_pointer_scan(work, m, cp, stream);
}

template <typename V>
void colmajor_fill(const int64_t *Ap, const int *Aj, int n, int m, int64_t nnz, const int64_t *cp, uint32_t *work, int *ri, V values,
                   hipStream_t stream)
{
	if (n > 0 && m > 0 && nnz > 0)
		hipLaunchKernelGGL(colmajor_fill_kernel<V>, dim3(row_blocks(n)), dim3(256), 0, stream, Ap, Aj, n, m, cp, work + std::max(m, 1), ri,
		                   values);
}
template void colmajor_fill<NoValues>(const int64_t *, const int *, int, int, int64_t, const int64_t *, uint32_t *, int *, NoValues, hipStream_t);
template void colmajor_fill<RawValues>(const int64_t *, const int *, int, int, int64_t, const int64_t *, uint32_t *, int *, RawValues, hipStream_t);
template void colmajor_fill<MontValues>(const int64_t *, const int *, int, int, int64_t, const int64_t *, uint32_t *, int *, MontValues, hipStream_t);

void colmajor_bucket(const int64_t *cp, int m, int threshold, bool list_empty, int *short_cols, int *long_cols, int *counters,
                     hipStream_t stream)
{
	if (m > 0)
		hipLaunchKernelGGL(colmajor_bucket_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, cp, m, threshold, list_empty, short_cols,
		                   long_cols, counters);
}

}  // namespace sh
