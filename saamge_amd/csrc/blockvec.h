// Tall-skinny block-vector kernels of the eigensolver (fp64): blocks are column-major, n rows, a leading dimension >= n,
// at most BV_MAX_COLS columns.  All pointers are device pointers; every reduction is deterministic (a grid fixed by n, a
// fixed order inside a workgroup, the workgroups' partials added in a fixed order by a final kernel, as `dot` does).
#pragma once
#include "common.h"

namespace saamge_amd {

constexpr int BV_MAX_COLS = 48;
constexpr int BV_MAX_NORMS = 16;

// doubles of scratch bv_gram needs for n rows and a p x q result
size_t bv_gram_scratch(int n, int p, int q);
// G (p x q, column-major, leading dimension p) = S^T T.  T == S with ldt == lds and q == p computes the upper 16 x 16
// tiles only and mirrors them.  Each operand column is read once.
void bv_gram(hipStream_t s, int n, int p, const double *S, long lds, int q, const double *T, long ldt, double *scratch,
             double *G);

// Y_b = S_b C (accumulate: Y_b += S_b C) for b < count <= 3 blocks that share C (p x q, column-major, leading dimension
// p) and the leading dimensions, in one launch.  A thread holds its whole row of S_b before it writes, so Y_b == S_b
// (the same first column, ldy == lds) is allowed; any other overlap is the caller's error (bv_combine_aliasing_ok).
struct BvBlocks {
    const double *S[3];
    double *Y[3];
    int count;
};
void bv_combine(hipStream_t s, int n, int p, int q, const double *C, bool accumulate, const BvBlocks &B, long lds, long ldy);
// the host's check of the rule above for one (S, Y) pair
bool bv_combine_aliasing_ok(int n, int p, const double *S, long lds, int q, const double *Y, long ldy);

// R_j = AX_j - lam_j MX_j for j < nb <= BV_MAX_NORMS, and norms[j] = ||R_j||_2, norms[BV_MAX_NORMS + j] = ||MX_j||_2.
// scratch: bv_residual_scratch(n) doubles; lam, norms (2 BV_MAX_NORMS doubles) on the device.
size_t bv_residual_scratch(int n);
void bv_residual(hipStream_t s, int n, int nb, const double *AX, const double *MX, long ld, const double *lam, double *R,
                 long ldr, double *scratch, double *norms);

// zero the rows of V (ncols columns) whose flag has `bit` set
void bv_mask(hipStream_t s, int n, int ncols, const signed char *flags, int bit, double *V, long ld);
// the start block of lobpcg_model.hash_start: entry (i, j) from a counter hash of (seed, i, j), in [-1, 1)
void bv_hash_start(hipStream_t s, int n, int nb, unsigned seed, double *X, long ld);

}  // namespace saamge_amd
