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

}  // namespace sh
