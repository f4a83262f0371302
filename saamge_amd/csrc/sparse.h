// CSR SpMV family, fused polynomial-smoother step, vector kernels (launch wrappers).
#pragma once
#include "block_chunks.h"
#include "common.h"
#include "options.h"

namespace saamge_amd {

// Optional row range of an operator application (row-partitioned solve: a rank applies only its
// own rows; x stays indexed by global column).  nrows < 0 = all rows.
struct RowRange {
    int row0 = 0, nrows = -1;
};

// build the SELL-64 copy of A (used by every routine below when present); of `opt`: sell and debug
void build_sell(hipStream_t s, DCsr &A, const Options &opt);
// y = A x
void spmv(hipStream_t s, const DCsr &A, const double *x, double *y, RowRange rr = RowRange());
// r = b - A x                                   (reference: amg/src/tg.cpp:115-116)
void spmv_residual(hipStream_t s, const DCsr &A, const double *x, const double *b, double *r,
                   RowRange rr = RowRange());
// x += P xc                                     (reference: amg/src/tg.cpp:129)
void spmv_add(hipStream_t s, const DCsr &P, const double *xc, double *x, RowRange rr = RowRange());
// xout = xin + scale * dinv_neg .* (A xin - b)  (reference: amg/inc/smpr.hpp:330-338)
void smooth_step(hipStream_t s, const DCsr &A, const double *dinv_neg, const double *b,
                 const double *xin, double *xout, double scale, RowRange rr = RowRange());
// xout = scale * dinv_neg .* (-b)   (the same step for xin == 0, no matrix traffic)
void smooth_first(hipStream_t s, int n, const double *dinv_neg, const double *b, double *xout,
                  double scale);
// dinv_neg_i = -1 / ( sqrt|a_ii| * sum_j |a_ij| / sqrt|a_jj| )
//                                               (reference: amg/src/mbox.cpp:1839-1861)
void build_dinv_neg(hipStream_t s, const DCsr &A, double *sqrt_diag_tmp, double *dinv_neg);
// byte codes of the smoother's diagonal factor (operators with <= 256 distinct values of it and the staged coded format)
void build_dinv_codes(hipStream_t s, DCsr &A, const double *dinv_neg, const Options &opt);

// the sum of v over a workgroup of 256 lanes in a fixed order (valid on thread 0); sh: 4 doubles of LDS.  Shared by the
// deterministic reductions: dot below and the column norms of blockvec.hip.
__device__ inline double block_sum_256(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// deterministic dot product: out[0] = sum a_i b_i ; `partials` holds >= 1024 doubles
void dot(hipStream_t s, int n, const double *a, const double *b, double *partials, double *out);
// PCG fused vector updates, scalars on the device:
// sc[0]=nom sc[1]=den sc[2]=betanom
void pcg_update_xr(hipStream_t s, int n, const double *sc, double *x, double *r,
                   const double *d, const double *z);   // alpha = nom/den
void pcg_update_d(hipStream_t s, int n, const double *sc, double *d, const double *z);  // beta = betanom/nom
void vec_copy(hipStream_t s, int n, const double *src, double *dst);
void vec_zero(hipStream_t s, int n, double *dst);
void vec_axpy(hipStream_t s, int n, double a, const double *x, double *y);  // y += a x

// ---- block members: the same operations on k <= BLOCK_MAX columns per launch ----------------------------
// Column j of every result holds the bits the single-vector routine above gives for column j alone: a block kernel reads
// the matrix entry once and keeps one set of accumulators per column, in the single kernel's order.  The columns of a block
// are a list of pointers (they need be neither contiguous nor equally strided); k == 1 goes through the single routine.
struct Cols {
    int k = 0;
    double *p[BLOCK_MAX] = {};
    Cols() {}
    // columns c[0 .. k) of a column-major block (c == null: columns 0 .. k - 1)
    Cols(const double *base, long ld, int k_, const int *c = nullptr) : k(k_) {
        for (int j = 0; j < k; ++j) p[j] = const_cast<double *>(base) + (size_t)(c ? c[j] : j) * (size_t)ld;
    }
};
void spmv_block(hipStream_t s, const DCsr &A, const Cols &x, const Cols &y);
void spmv_residual_block(hipStream_t s, const DCsr &A, const Cols &x, const Cols &b, const Cols &r);
void spmv_add_block(hipStream_t s, const DCsr &P, const Cols &xc, const Cols &x);
void smooth_step_block(hipStream_t s, const DCsr &A, const double *dinv_neg, const Cols &b, const Cols &xin, const Cols &xout,
                       double scale);
void smooth_first_block(hipStream_t s, int n, const double *dinv_neg, const Cols &b, const Cols &xout, double scale);
// out.p[j][slot] = a_j . b_j ; `partials` holds >= 1024 k doubles
void dot_block(hipStream_t s, int n, const Cols &a, const Cols &b, double *partials, const Cols &out, int slot);
// sc.p[j]: the three scalars of column j
void pcg_update_xr_block(hipStream_t s, int n, const Cols &sc, const Cols &x, const Cols &r, const Cols &d, const Cols &z);
void pcg_update_d_block(hipStream_t s, int n, const Cols &sc, const Cols &d, const Cols &z);
void pcg_shift_nom_block(hipStream_t s, const Cols &sc);      // sc_j[0] = sc_j[2]
void vec_copy_block(hipStream_t s, int n, const Cols &src, const Cols &dst);
void vec_zero_block(hipStream_t s, int n, const Cols &dst);
void vec_axpy_block(hipStream_t s, int n, double a, const Cols &x, const Cols &y);

}  // namespace saamge_amd
