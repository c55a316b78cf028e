// The entries of a CSR matrix column by column on the device (colmajor.hip): what x.A (spmv.hip), the matching's pattern of A^T
// (matching.hip) and the stable transpose (transpose.hip) all start from.  Count per column (u32 atomics), one workgroup scans
// the counts into column pointers, every entry goes to the slice of its column at (its turn): one u32 position counter per
// column, the only other atomics -- the order inside a slice is whatever the fill produced.
//
// Count and fill run a wave per row, four waves per workgroup, on min(2^20, ceil(n / 4)) workgroups that stride over the rows:
// below 4,194,304 rows every wave has one row; beyond that the grid stops growing and the waves take several rows each, for
// x.A and the matching as for the transpose.  Nothing here synchronises the stream or reads a flag back: the callers do, where they need to.
#pragma once

#include "device_types.h"

namespace sh {

// a host CSR matrix on the device for the duration of a call.  Always a copy of its own: these calls upload A themselves and
// never take the driver's resident one (DeviceMatrix)
struct CsrUpload {
	int n;
	int64_t nnz;
	int64_t *p = nullptr;        // n + 1; one zero when n == 0
	int *j = nullptr, *x = nullptr;          // x: nullptr without values
	CsrUpload(const struct spasm_csr *A, bool values);          // (checked by check_host_csr) allocates
	void send(const struct spasm_csr *A, hipStream_t stream);   // queues the copies
	~CsrUpload();
	CsrUpload(const CsrUpload &) = delete;
	CsrUpload &operator=(const CsrUpload &) = delete;
};

// out[0] = 0, out[t + 1] = len[0] + ... + len[t]: one workgroup.  T: uint32_t or int64_t
template <typename T> void launch_pointer_scan(const T *len, int n, int64_t *out, hipStream_t stream);

// what the fill stores beside the row index of an entry at position `at` of the image
struct NoValues {};
struct RawValues {           // the 32-bit word as it is
	const int *Ax;
	int *out;
};
struct MontValues {          // value * 2^32 mod p, whatever integer the caller stored
	const int *Ax;
	uint32_t *out;
	MontDev F;
};

// Step 1: cp[0 .. m] from the n x m matrix (Ap, Aj) of nnz entries.  work: 2 max(m, 1) words, zeroed here: the counts, then the
// positions of step 2.  A column index outside [0, m) sets bit 0 of *bad (zeroed by the caller) and is skipped, in both steps.
void colmajor_count_scan(const int64_t *Ap, const int *Aj, int n, int m, int64_t nnz, uint32_t *work, int *bad, int64_t *cp,
                         hipStream_t stream);
// Step 2: ri[at] = row of every entry, its value as V says.  V: NoValues, RawValues or MontValues
template <typename V>
void colmajor_fill(const int64_t *Ap, const int *Aj, int n, int m, int64_t nnz, const int64_t *cp, uint32_t *work, int *ri, V values,
                   hipStream_t stream);

// The columns in two lists, in no particular order: longer than threshold in long_cols, the others in short_cols -- the empty
// ones too when list_empty.  counters (zeroed by the caller): [0] short columns, [1] long columns, [2] the longest listed one
void colmajor_bucket(const int64_t *cp, int m, int threshold, bool list_empty, int *short_cols, int *long_cols, int *counters,
                     hipStream_t stream);

}  // namespace sh
