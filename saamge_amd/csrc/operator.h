// The fine operator assembled on the device from the element matrices (operator.hip).  saamge_amd/assemble_model.py defines
// the result -- pattern, summation order, elimination -- and the kernels give the same bits.
#pragma once
#include "common.h"

namespace saamge_amd {

// the ids i in [0, n) with cls[i] == which, ascending (flag: n ints, pos: n + 1 ints of scratch); returns their number
int make_list(hipStream_t s, int n, const int *cls, int which, DBuf<int> &flag, DBuf<int> &pos, DBuf<int> &list);

constexpr int OP_SHORT_CAND = 64;    // candidates of a row of the short path (LDS: 64 ints per row, 16 rows per workgroup)
constexpr int OP_LDS_CAND = 4096;    // candidates of a row of the LDS path (16 KB)

// Rows go by their number of CANDIDATES: the sum of the sizes of the elements that hold the dof.
struct OperatorLimits {
    int short_cand = OP_SHORT_CAND;  // <= : several rows per wavefront
    int lds_cand = OP_LDS_CAND;      // <= : one workgroup per row, sorted in LDS; above: through global memory
};

struct AssembledOperator {
    int device = 0;
    hipStream_t stream = nullptr;
    int n = 0, NE = 0;
    int nde = 0;                     // > 0: every element has nde dofs (moff empty)
    long nconn = 0;
    int64_t nnz = 0, elmat_len = 0;
    // the mesh, kept for the numeric pass: elements -> dofs, dofs -> elements (ascending), offsets of the packed matrices
    DBuf<int> eI, eJ, d2e_I, d2e_J;
    DBuf<roff_t> moff;
    DBuf<signed char> bdr;           // empty: no essential dof
    DBuf<roff_t> rowptr;
    DBuf<int> col;
    DBuf<double> val;
    // rows of the numeric pass by path (short, LDS table, global)
    DBuf<int> num_list[3];
    int num_count[3] = {0, 0, 0};
    long long sym_count[3] = {0, 0, 0};
};

// Inputs host or device pointers; checked before anything is read through them.  Runs on s and returns with s idle.
void operator_assemble(hipStream_t s, int n, int NE, int nde, const int *elem_ptr, const int *elem_to_dof,
                       const double *elmat, const signed char *bdr_dofs, const OperatorLimits &lim, AssembledOperator &op);
// val from new element matrices (host or device pointer), on op.stream
void operator_numeric(AssembledOperator &op, const double *elmat);
// b (n, in place) for the essential values x_ess, both on the device; elmat a host or device pointer
void operator_eliminate_rhs(const AssembledOperator &op, const double *elmat, const double *x_ess, double *b);
// b (n, on the device, overwritten) from the packed element vectors (element e at the offset of its dof list; host or device
// pointer): assemble_model.assemble_rhs
void operator_assemble_rhs(const AssembledOperator &op, const double *elvec, double *b);

}  // namespace saamge_amd
