// General sparse matrix products and transpose (see spgemm.hip): the smoothed-prolongator path.
#pragma once
#include "common.h"

namespace saamge_amd {

// C = beta E + alpha diag(d) A B.  E (optional) has A's rows and B's columns; d (optional) has one
// entry per row of A.  Rows of C come out sorted by column; summation order is fixed.
void spgemm(hipStream_t s, const DCsr &A, const DCsr &B, const DCsr *E, const double *d, double alpha,
            double beta, DCsr &C);
// Which way the last spgemm call of the calling thread went (the tests of the C ABI ask): 0, 1, 2 = the hash-table product
// and the table tier (256, 2048, 8192 slots) that held every row; SPGEMM_ROUTE_DENSE_B; SPGEMM_ROUTE_NONE = no kernel ran
// (no rows) or the product was refused.  Recorded on the host: no device work, no synchronisation.
constexpr int SPGEMM_ROUTE_NONE = -1, SPGEMM_ROUTE_DENSE_B = 3;
int spgemm_last_route();
// R = P^T, rows sorted by column
void csr_transpose(hipStream_t s, const DCsr &P, DCsr &R);
// C = entries of A with |v| > tol, order kept (AltThreshold, amg/src/interp.cpp:89-170)
void csr_threshold(hipStream_t s, const DCsr &A, double tol, DCsr &C);

}  // namespace saamge_amd
