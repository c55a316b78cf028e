// Y = X.A + Y mod p on the device (spmv.hip): a column-major image of A built once, applied to any number of batches of vectors.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

namespace sh {

struct XaPlan;
// uploads A and builds its column-major image; dies (message prefixed with who) on a malformed A or an unsupported modulus
XaPlan *xa_plan_create(const struct spasm_csr *A, const char *who);
// Y (k x m, row-major) += X (k x n, row-major) . A; any integer representatives in, balanced ones out
void xa_plan_apply(XaPlan *P, int k, const spasm_ZZp *X, spasm_ZZp *Y);
void xa_plan_destroy(XaPlan *P);
// the pattern of the n x m matrix (d_Ap, d_Aj) column by column on the device: d_cp (m + 1 pointers), d_ri (row of each entry;
// inside a column in no particular order); d_work has room for 2 max(m, 1) words, d_bad for one.  false: a column index lies
// outside [0, m).  Synchronises the stream.
bool xa_pattern_image(const int64_t *d_Ap, const int *d_Aj, int n, int m, int64_t *d_cp, int *d_ri, uint32_t *d_work, int *d_bad,
                      hipStream_t stream);

}  // namespace sh
