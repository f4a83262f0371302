// The fine operator assembled on the device from elem_to_dof and the element matrices.  saamge_amd/assemble_model.py defines
// the result; this file restates it and gives the same bits.
//
// Symbolic pass: dof -> elements (ascending), then per row the union of the dof lists of its elements ("candidates"),
// sorted, duplicates removed; a count pass, a 64-bit scan, a fill pass.  Nothing with one slot per (element, local pair)
// is ever stored: the workspace beyond the output is the dof -> element table and a few arrays of n integers.  Rows go by
// their candidate count:
//   short   <= 64     16 lanes per row, 16 rows per workgroup: candidates in LDS, a candidate is kept when no earlier one
//                     equals it and lands at the number of kept candidates below it
//   LDS     <= 4096   one workgroup per row: bitonic sort in LDS, neighbours compared, positions by a block scan
//   global  above     one workgroup per row: a candidate is kept when no earlier element of the row holds it (the lists are
//                     read from global memory), then the row is sorted in place by odd-even transposition
// Numeric pass (all that a coefficient update runs): the owner of entry (i, j) adds the terms of the elements of i in
// ascending id, the first term taken as it is.  The short and the LDS path read every dof list of the row ONCE: each
// candidate finds its column by bisection in the row and leaves its local index in an LDS table [entry][element of the
// row]; the owner of an entry then walks its line of the table.  Rows whose table does not fit walk the dof lists in
// global memory per entry.  No floating-point atomics, no reduction whose order could vary.
#include "operator.h"
#include "devtab.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>

#include "partition.h"

namespace saamge_amd {

namespace {

constexpr int OP_LPR = 16;                 // lanes per row of the short paths
constexpr int OP_RPB = 256 / OP_LPR;       // their rows per workgroup
constexpr int OP_TBL_SHORT = 256;          // bytes of a short row's table: entries x elements
constexpr int OP_TBL_LDS = 8192;           // 16-bit slots of the LDS path's table
constexpr int OP_ELEMS_LDS = 64;           // elements of a row of the LDS numeric path
constexpr int OP_ESS = 0x02;               // SAAMGE_AMD_ON_ESS_DOMAIN_BORDER
constexpr int OP_MAX_ND = 46340;           // nd * nd stays below 2^31

// ---- tables ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void op_first_free_kernel(int n, const int *__restrict__ cnt, int *__restrict__ first) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && cnt[i] == 0) atomicMin(first, (int)i);
}
__global__ __launch_bounds__(256) void op_sq_kernel(int NE, const int *__restrict__ eI, int *__restrict__ sq, int *__restrict__ err) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int nd = eI[e + 1] - eI[e];
    if (nd > OP_MAX_ND) { atomicOr(err, 1); sq[e] = 0; return; }
    sq[e] = nd * nd;
}
// candidates of every row and its symbolic path
__global__ __launch_bounds__(256) void op_cand_kernel(int n, const int *__restrict__ d2e_I, const int *__restrict__ d2e_J,
                                                      const int *__restrict__ eI, int short_cand, int lds_cand,
                                                      int *__restrict__ cand, int *__restrict__ cls) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long c = 0;
    for (int x = d2e_I[i], x1 = d2e_I[i + 1]; x < x1; ++x) {
        const int e = d2e_J[x];
        c += eI[e + 1] - eI[e];
    }
    cand[i] = c < INT_MAX ? (int)c : INT_MAX;
    cls[i] = c <= short_cand ? 0 : (c <= lds_cand ? 1 : 2);
}
// the numeric path: the table [entries of the row][elements of the row] has to fit
__global__ __launch_bounds__(256) void op_numcls_kernel(int n, const int *__restrict__ cand, const int *__restrict__ d2e_I,
                                                        const roff_t *__restrict__ rowptr, int short_cand, int lds_cand,
                                                        int *__restrict__ cls) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long nelem = d2e_I[i + 1] - d2e_I[i], len = (long)(rowptr[i + 1] - rowptr[i]);
    const int c = cand[i];
    int k = 2;
    if (c <= short_cand && nelem * len <= OP_TBL_SHORT) k = 0;
    else if (c <= lds_cand && nelem <= OP_ELEMS_LDS && nelem * len <= OP_TBL_LDS) k = 1;
    cls[i] = k;
}
__global__ __launch_bounds__(256) void op_flag_kernel(int n, const int *__restrict__ cls, int which, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = cls[i] == which;
}
// ---- symbolic pass --------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void op_sym_short_kernel(int nrows, const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                           const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                           const int *__restrict__ eJ, int *__restrict__ cnt,
                                                           const roff_t *__restrict__ rowptr, int *__restrict__ col) {
    __shared__ int c[OP_RPB][OP_SHORT_CAND];
    __shared__ unsigned char kept[OP_RPB][OP_SHORT_CAND];
    const int r = threadIdx.x / OP_LPR, lane = threadIdx.x % OP_LPR;
    const long slot = (long)blockIdx.x * OP_RPB + r;
    const bool valid = slot < nrows;
    int i = 0, ncand = 0;
    if (valid) {
        i = list[slot];
        for (int x = d2e_I[i], x1 = d2e_I[i + 1]; x < x1; ++x) {
            const int e = d2e_J[x], eb = eI[e], nd = eI[e + 1] - eb;
            for (int a = lane; a < nd; a += OP_LPR) c[r][ncand + a] = eJ[eb + a];   // (ncand + nd <= OP_SHORT_CAND: op_cand_kernel)
            ncand += nd;
        }
    }
    __syncthreads();
    unsigned first = 0;
    int nfirst = 0;
    for (int t = 0; t < OP_SHORT_CAND / OP_LPR; ++t) {
        const int q = lane + t * OP_LPR;
        if (q >= ncand) continue;
        const int v = c[r][q];
        bool f = true;
        for (int p = 0; p < q; ++p) f &= c[r][p] != v;
        if (f) { first |= 1u << t; ++nfirst; }
        if (FILL) kept[r][q] = f;
    }
    if (!FILL) {
        for (int m = OP_LPR / 2; m; m >>= 1) nfirst += __shfl_xor(nfirst, m);
        if (valid && lane == 0) cnt[i] = nfirst;
        return;
    }
    __syncthreads();
    for (int t = 0; t < OP_SHORT_CAND / OP_LPR; ++t) {
        if (!(first >> t & 1u)) continue;
        const int v = c[r][lane + t * OP_LPR];
        int rank = 0;
        for (int p = 0; p < ncand; ++p) rank += kept[r][p] && c[r][p] < v;
        col[rowptr[i] + rank] = v;
    }
}

template <bool FILL>
__global__ __launch_bounds__(256) void op_sym_lds_kernel(const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                         const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                         const int *__restrict__ eJ, int *__restrict__ cnt,
                                                         const roff_t *__restrict__ rowptr, int *__restrict__ col) {
    typedef hipcub::BlockScan<int, 256> Scan;
    __shared__ int c[OP_LDS_CAND];
    __shared__ typename Scan::TempStorage tmp;
    const int tid = threadIdx.x, i = list[blockIdx.x];
    int ncand = 0;
    for (int x = d2e_I[i], x1 = d2e_I[i + 1]; x < x1; ++x) {
        const int e = d2e_J[x], eb = eI[e], nd = eI[e + 1] - eb;
        for (int a = tid; a < nd; a += 256) c[ncand + a] = eJ[eb + a];              // (ncand + nd <= OP_LDS_CAND: op_cand_kernel)
        ncand += nd;
    }
    int P = 2;
    while (P < ncand) P <<= 1;
    for (int q = ncand + tid; q < P; q += 256) c[q] = INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < P; idx += 256) {
                const int ixj = idx ^ j;
                if (ixj > idx) {
                    const int a = c[idx], b = c[ixj];
                    if ((a > b) == ((idx & k) == 0)) { c[idx] = b; c[ixj] = a; }
                }
            }
            __syncthreads();
        }
    int out = 0;
    for (int q0 = 0; q0 < ncand; q0 += 256) {
        const int q = q0 + tid;
        const int f = (q < ncand && (q == 0 || c[q] != c[q - 1])) ? 1 : 0;
        int pos, total;
        Scan(tmp).ExclusiveSum(f, pos, total);
        if (FILL && f) col[rowptr[i] + out + pos] = c[q];
        out += total;
        __syncthreads();
    }
    if (!FILL && tid == 0) cnt[i] = out;
}

template <bool FILL>
__global__ __launch_bounds__(256) void op_sym_global_kernel(const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                            const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                            const int *__restrict__ eJ, int *__restrict__ cnt,
                                                            const roff_t *__restrict__ rowptr, int *col) {
    typedef hipcub::BlockScan<int, 256> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int tid = threadIdx.x, i = list[blockIdx.x];
    const int x0 = d2e_I[i], x1 = d2e_I[i + 1];
    int out = 0;
    for (int x = x0; x < x1; ++x) {
        const int e = d2e_J[x], eb = eI[e], nd = eI[e + 1] - eb;
        for (int a0 = 0; a0 < nd; a0 += 256) {
            const int a = a0 + tid;
            int f = 0, v = 0;
            if (a < nd) {
                v = eJ[eb + a];
                f = 1;
                for (int y = x0; y < x && f; ++y) {      // an earlier element of the row holds it: not kept
                    const int g = d2e_J[y];
                    for (int z = eI[g], z1 = eI[g + 1]; z < z1; ++z)
                        if (eJ[z] == v) { f = 0; break; }
                }
            }
            int pos, total;
            Scan(tmp).ExclusiveSum(f, pos, total);
            if (FILL && f) col[rowptr[i] + out + pos] = v;
            out += total;
            __syncthreads();
        }
    }
    if (!FILL) {
        if (tid == 0) cnt[i] = out;
        return;
    }
    volatile int *row = col + rowptr[i];
    for (int ph = 0; ph < out; ++ph) {                   // odd-even transposition: out phases sort out entries
        for (int p = 2 * tid + (ph & 1); p + 1 < out; p += 512) {
            const int a = row[p], b = row[p + 1];
            if (a > b) { row[p] = b; row[p + 1] = a; }
        }
        __syncthreads();
    }
}

// ---- numeric pass ---------------------------------------------------------------------------------------------------
__device__ inline int op_find(const int *__restrict__ row, int len, int v) {   // v is in the ascending row
    int lo = 0, hi = len - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline roff_t op_moff(const roff_t *__restrict__ moff, int nde, int e) {
    return moff ? moff[e] : (roff_t)e * nde * nde;
}
__device__ inline double op_eliminated(double v, int i, int j, const signed char *__restrict__ bdr) {
    return (bdr && i != j && ((bdr[i] | bdr[j]) & OP_ESS)) ? 0.0 : v;
}
// a_ij before elimination, by walking the dof lists of the elements of i in global memory
__device__ inline double op_entry_value(int i, int j, const int *__restrict__ d2e_I, const int *__restrict__ d2e_J,
                                        const int *__restrict__ eI, const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                        int nde, const double *__restrict__ elmat) {
    double sum = 0.0;
    bool have = false;
    for (int x = d2e_I[i], x1 = d2e_I[i + 1]; x < x1; ++x) {
        const int e = d2e_J[x], eb = eI[e], nd = eI[e + 1] - eb;
        int la = -1, lb = -1;
        for (int a = 0; a < nd; ++a) {
            const int v = eJ[eb + a];
            if (v == i) la = a;
            if (v == j) lb = a;
        }
        if (lb < 0) continue;
        const double term = elmat[op_moff(moff, nde, e) + (roff_t)la * nd + lb];
        sum = have ? sum + term : term;
        have = true;
    }
    return sum;
}

__global__ __launch_bounds__(256) void op_num_short_kernel(int nrows, const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                           const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                           const int *__restrict__ eJ, const roff_t *__restrict__ moff, int nde,
                                                           const double *__restrict__ elmat, const signed char *__restrict__ bdr,
                                                           const roff_t *__restrict__ rowptr, const int *__restrict__ col,
                                                           double *__restrict__ val) {
    __shared__ unsigned tab[OP_RPB][OP_TBL_SHORT / 4];
    __shared__ unsigned char la[OP_RPB][OP_SHORT_CAND];
    const int r = threadIdx.x / OP_LPR, lane = threadIdx.x % OP_LPR;
    const long slot = (long)blockIdx.x * OP_RPB + r;
    const bool valid = slot < nrows;
    unsigned char *T = (unsigned char *)tab[r];          // T[entry * nelem + element of the row] = local index + 1, 0: not held
    for (int q = lane; q < OP_TBL_SHORT / 4; q += OP_LPR) tab[r][q] = 0u;
    __syncthreads();
    int i = 0, x0 = 0, nelem = 0, len = 0;
    roff_t rp = 0;
    if (valid) {
        i = list[slot];
        x0 = d2e_I[i];
        nelem = d2e_I[i + 1] - x0;
        rp = rowptr[i];
        len = (int)(rowptr[i + 1] - rp);
        for (int xi = 0; xi < nelem; ++xi) {
            const int e = d2e_J[x0 + xi], eb = eI[e], nd = eI[e + 1] - eb;
            for (int a = lane; a < nd; a += OP_LPR) {    // (nd <= OP_SHORT_CAND, nelem * len <= OP_TBL_SHORT: op_numcls_kernel)
                const int v = eJ[eb + a];
                if (v == i) la[r][xi] = (unsigned char)a;
                T[op_find(col + rp, len, v) * nelem + xi] = (unsigned char)(a + 1);
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    for (int k = lane; k < len; k += OP_LPR) {
        double sum = 0.0;
        bool have = false;
        for (int xi = 0; xi < nelem; ++xi) {
            const int lb1 = T[k * nelem + xi];
            if (!lb1) continue;
            const int e = d2e_J[x0 + xi], nd = eI[e + 1] - eI[e];
            const double term = elmat[op_moff(moff, nde, e) + (roff_t)la[r][xi] * nd + (lb1 - 1)];
            sum = have ? sum + term : term;
            have = true;
        }
        val[rp + k] = op_eliminated(sum, i, col[rp + k], bdr);
    }
}

__global__ __launch_bounds__(256) void op_num_lds_kernel(const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                         const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                         const int *__restrict__ eJ, const roff_t *__restrict__ moff, int nde,
                                                         const double *__restrict__ elmat, const signed char *__restrict__ bdr,
                                                         const roff_t *__restrict__ rowptr, const int *__restrict__ col,
                                                         double *__restrict__ val) {
    __shared__ unsigned short T[OP_TBL_LDS];
    __shared__ int la[OP_ELEMS_LDS], el[OP_ELEMS_LDS];
    const int tid = threadIdx.x, i = list[blockIdx.x];
    const int x0 = d2e_I[i], nelem = d2e_I[i + 1] - x0;
    const roff_t rp = rowptr[i];
    const int len = (int)(rowptr[i + 1] - rp);
    for (int q = tid; q < nelem * len; q += 256) T[q] = 0;          // (nelem * len <= OP_TBL_LDS, nelem <= OP_ELEMS_LDS)
    __syncthreads();
    for (int xi = 0; xi < nelem; ++xi) {
        const int e = d2e_J[x0 + xi], eb = eI[e], nd = eI[e + 1] - eb;
        if (tid == 0) el[xi] = e;
        for (int a = tid; a < nd; a += 256) {                       // (nd <= OP_LDS_CAND: a + 1 fits 16 bits)
            const int v = eJ[eb + a];
            if (v == i) la[xi] = a;
            T[op_find(col + rp, len, v) * nelem + xi] = (unsigned short)(a + 1);
        }
    }
    __syncthreads();
    for (int k = tid; k < len; k += 256) {
        double sum = 0.0;
        bool have = false;
        for (int xi = 0; xi < nelem; ++xi) {
            const int lb1 = T[k * nelem + xi];
            if (!lb1) continue;
            const int e = el[xi], nd = eI[e + 1] - eI[e];
            const double term = elmat[op_moff(moff, nde, e) + (roff_t)la[xi] * nd + (lb1 - 1)];
            sum = have ? sum + term : term;
            have = true;
        }
        val[rp + k] = op_eliminated(sum, i, col[rp + k], bdr);
    }
}

__global__ __launch_bounds__(256) void op_num_global_kernel(const int *__restrict__ list, const int *__restrict__ d2e_I,
                                                            const int *__restrict__ d2e_J, const int *__restrict__ eI,
                                                            const int *__restrict__ eJ, const roff_t *__restrict__ moff, int nde,
                                                            const double *__restrict__ elmat, const signed char *__restrict__ bdr,
                                                            const roff_t *__restrict__ rowptr, const int *__restrict__ col,
                                                            double *__restrict__ val) {
    const int i = list[blockIdx.x];
    for (roff_t k = rowptr[i] + threadIdx.x, k1 = rowptr[i + 1]; k < k1; k += 256) {
        const int j = col[k];
        val[k] = op_eliminated(op_entry_value(i, j, d2e_I, d2e_J, eI, eJ, moff, nde, elmat), i, j, bdr);
    }
}

// One thread per row: few rows have an essential column at all, and only those entries are computed.  The product and the
// difference are rounded one after the other, as the model does (no fused multiply-add).
__global__ __launch_bounds__(256) void op_rhs_kernel(int n, const int *__restrict__ d2e_I, const int *__restrict__ d2e_J,
                                                     const int *__restrict__ eI, const int *__restrict__ eJ,
                                                     const roff_t *__restrict__ moff, int nde, const double *__restrict__ elmat,
                                                     const signed char *__restrict__ bdr, const roff_t *__restrict__ rowptr,
                                                     const int *__restrict__ col, const double *__restrict__ x, double *__restrict__ b) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = (int)t;
    if (bdr[i] & OP_ESS) {
        b[i] = op_entry_value(i, i, d2e_I, d2e_J, eI, eJ, moff, nde, elmat) * x[i];
        return;
    }
    double bi = b[i];
    bool any = false;
    for (roff_t k = rowptr[i], k1 = rowptr[i + 1]; k < k1; ++k) {
        const int j = col[k];
        if (!(bdr[j] & OP_ESS)) continue;
        const double prod = op_entry_value(i, j, d2e_I, d2e_J, eI, eJ, moff, nde, elmat) * x[j];
        bi = bi - prod;
        any = true;
    }
    if (any) b[i] = bi;
}

// One thread per dof: the terms of its elements in ascending element id, the first one taken as it is.  The element vectors
// are packed like the dof lists, so a term lies at the position of the dof in eJ.
__global__ __launch_bounds__(256) void op_rhs_assemble_kernel(int n, const int *__restrict__ d2e_I, const int *__restrict__ d2e_J,
                                                              const int *__restrict__ eI, const int *__restrict__ eJ,
                                                              const double *__restrict__ elvec, double *__restrict__ b) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = (int)t;
    double sum = 0.0;
    bool have = false;
    for (int x = d2e_I[i], x1 = d2e_I[i + 1]; x < x1; ++x) {
        const int e = d2e_J[x], eb = eI[e], nd = eI[e + 1] - eb;
        for (int a = 0; a < nd; ++a) {
            if (eJ[eb + a] != i) continue;
            const double term = elvec[eb + a];
            sum = have ? sum + term : term;
            have = true;
            break;
        }
    }
    b[i] = sum;
}

template <bool FILL>
void symbolic_pass(hipStream_t s, const AssembledOperator &op, const DBuf<int> *list, const int *count, int *cnt, int *col) {
    const int *dI = op.d2e_I.p, *dJ = op.d2e_J.p, *eI = op.eI.p, *eJ = op.eJ.p;
    const roff_t *rp = op.rowptr.p;
    if (count[0])
        hipLaunchKernelGGL(op_sym_short_kernel<FILL>, dim3((unsigned)div_up(count[0], OP_RPB)), dim3(256), 0, s, count[0],
                           (const int *)list[0].p, dI, dJ, eI, eJ, cnt, rp, col);
    if (count[1])
        hipLaunchKernelGGL(op_sym_lds_kernel<FILL>, dim3((unsigned)count[1]), dim3(256), 0, s, (const int *)list[1].p, dI, dJ, eI,
                           eJ, cnt, rp, col);
    if (count[2])
        hipLaunchKernelGGL(op_sym_global_kernel<FILL>, dim3((unsigned)count[2]), dim3(256), 0, s, (const int *)list[2].p, dI, dJ,
                           eI, eJ, cnt, rp, col);
    SA_HIP_CHECK(hipGetLastError());
}

void numeric_pass(hipStream_t s, AssembledOperator &op, const double *elmat) {
    const int *dI = op.d2e_I.p, *dJ = op.d2e_J.p, *eI = op.eI.p, *eJ = op.eJ.p;
    const roff_t *moff = op.moff.p;
    const signed char *bdr = op.bdr.p;
    if (op.num_count[0])
        hipLaunchKernelGGL(op_num_short_kernel, dim3((unsigned)div_up(op.num_count[0], OP_RPB)), dim3(256), 0, s, op.num_count[0],
                           (const int *)op.num_list[0].p, dI, dJ, eI, eJ, moff, op.nde, elmat, bdr, (const roff_t *)op.rowptr.p,
                           (const int *)op.col.p, op.val.p);
    if (op.num_count[1])
        hipLaunchKernelGGL(op_num_lds_kernel, dim3((unsigned)op.num_count[1]), dim3(256), 0, s, (const int *)op.num_list[1].p, dI, dJ,
                           eI, eJ, moff, op.nde, elmat, bdr, (const roff_t *)op.rowptr.p, (const int *)op.col.p, op.val.p);
    if (op.num_count[2])
        hipLaunchKernelGGL(op_num_global_kernel, dim3((unsigned)op.num_count[2]), dim3(256), 0, s, (const int *)op.num_list[2].p, dI,
                           dJ, eI, eJ, moff, op.nde, elmat, bdr, (const roff_t *)op.rowptr.p, (const int *)op.col.p, op.val.p);
    SA_HIP_CHECK(hipGetLastError());
}

}  // namespace

int make_list(hipStream_t s, int n, const int *cls, int which, DBuf<int> &flag, DBuf<int> &pos, DBuf<int> &list) {
    hipLaunchKernelGGL(op_flag_kernel, grid_flat(n), dim3(256), 0, s, n, cls, which, flag.p);
    SA_HIP_CHECK(hipGetLastError());
    return dev_compact(s, n, flag.p, pos.p, list);
}

void operator_assemble(hipStream_t s, int n, int NE, int nde, const int *elem_ptr, const int *elem_to_dof,
                       const double *elmat, const signed char *bdr_dofs, const OperatorLimits &lim, AssembledOperator &op) {
    SA_REQUIRE(n >= 0 && NE >= 0, "n < 0 or NE < 0");
    SA_REQUIRE(elem_ptr || nde >= 1, "elem_ptr or a uniform nde >= 1 is needed");
    SA_REQUIRE(NE == 0 || (elem_to_dof && elmat), "null argument");
    SA_REQUIRE(lim.short_cand >= 0 && lim.short_cand <= OP_SHORT_CAND && lim.lds_cand >= 0 && lim.lds_cand <= OP_LDS_CAND,
               "operator path limits: 0 .. 64 candidates for the short path, 0 .. 4096 for the LDS path");
    op.device = current_device();
    op.stream = s;
    op.n = n;
    op.NE = NE;
    op.nde = elem_ptr ? 0 : nde;
    // the mesh: offsets first, they say how much of elem_to_dof there is
    if (elem_ptr) {
        upload(op.eI, elem_ptr, (size_t)NE + 1, s);
    } else {
        SA_REQUIRE(nde <= OP_MAX_ND && (int64_t)NE * nde < INT_MAX, "NE * nde beyond 32 bits");
        std::vector<int> h((size_t)NE + 1);
        for (int e = 0; e <= NE; ++e) h[(size_t)e] = e * nde;
        op.eI.from_host(h, s);
    }
    if (NE && !is_device_ptr(elem_to_dof)) {
        const auto hI = op.eI.to_host(s);
        for (int e = 0; e < NE; ++e)
            SA_REQUIRE(hI[0] == 0 && hI[(size_t)e + 1] > hI[(size_t)e], "elem_ptr: must start at 0 and every element needs a dof");
        upload(op.eJ, elem_to_dof, (size_t)hI[(size_t)NE], s);
        op.nconn = check_mesh_device(s, NE, op.eI.p, op.eJ.p, n);
    } else if (NE) {
        op.nconn = check_mesh_device(s, NE, op.eI.p, elem_to_dof, n);
        upload(op.eJ, elem_to_dof, (size_t)op.nconn, s);
    }
    if (bdr_dofs && n) upload(op.bdr, bdr_dofs, (size_t)n, s);
    op.rowptr.alloc((size_t)n + 1);
    if (n == 0) {           // (NE > 0 would have had a dof out of range)
        op.rowptr.zero(s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    // dof -> elements, ascending
    DBuf<int> cnt((size_t)n + 1), info(1);
    cnt.zero(s);
    if (op.nconn) dev_histogram(s, op.nconn, op.eJ.p, cnt.p);
    SA_HIP_CHECK(hipMemsetAsync(info.p, 0x7f, sizeof(int), s));
    hipLaunchKernelGGL(op_first_free_kernel, grid_flat(n), dim3(256), 0, s, n, (const int *)cnt.p, info.p);
    SA_HIP_CHECK(hipGetLastError());
    {
        const int first_free = info.to_host(s)[0];
        SA_REQUIRE(first_free >= n, "dof " + std::to_string(first_free) + " lies in no element");
    }
    op.d2e_I.alloc((size_t)n + 1);
    op.d2e_J.alloc((size_t)op.nconn);
    dev_table_finish(s, NE, op.eI.p, op.eJ.p, n, cnt.p, op.d2e_I.p, op.d2e_J.p, true);
    // offsets of the packed element matrices
    if (elem_ptr) {
        DBuf<int> sq((size_t)NE);
        info.zero(s);
        hipLaunchKernelGGL(op_sq_kernel, grid_flat(NE), dim3(256), 0, s, NE, (const int *)op.eI.p, sq.p, info.p);
        SA_HIP_CHECK(hipGetLastError());
        SA_REQUIRE(!info.to_host(s)[0], "an element with more than 46340 dofs");
        op.moff.alloc((size_t)NE + 1);
        exclusive_scan_off(s, NE, sq.p, op.moff.p);
        op.elmat_len = read_one(op.moff.p + NE, s);
    } else {
        op.elmat_len = (int64_t)NE * nde * nde;
    }
    // symbolic pass
    DBuf<int> cand((size_t)n), cls((size_t)n), flag((size_t)n), pos((size_t)n + 1), list[3];
    int count[3];
    hipLaunchKernelGGL(op_cand_kernel, grid_flat(n), dim3(256), 0, s, n, (const int *)op.d2e_I.p, (const int *)op.d2e_J.p,
                       (const int *)op.eI.p, lim.short_cand, lim.lds_cand, cand.p, cls.p);
    SA_HIP_CHECK(hipGetLastError());
    for (int k = 0; k < 3; ++k) {
        count[k] = make_list(s, n, cls.p, k, flag, pos, list[k]);
        op.sym_count[k] = count[k];
    }
    symbolic_pass<false>(s, op, list, count, cnt.p, nullptr);
    exclusive_scan_off(s, n, cnt.p, op.rowptr.p);
    op.nnz = read_one(op.rowptr.p + n, s);
    op.col.alloc((size_t)op.nnz);
    op.val.alloc((size_t)op.nnz);
    symbolic_pass<true>(s, op, list, count, nullptr, op.col.p);
    // numeric pass
    hipLaunchKernelGGL(op_numcls_kernel, grid_flat(n), dim3(256), 0, s, n, (const int *)cand.p, (const int *)op.d2e_I.p,
                       (const roff_t *)op.rowptr.p, lim.short_cand, lim.lds_cand, cls.p);
    SA_HIP_CHECK(hipGetLastError());
    for (int k = 0; k < 3; ++k) op.num_count[k] = make_list(s, n, cls.p, k, flag, pos, op.num_list[k]);
    operator_numeric(op, elmat);
}

void operator_numeric(AssembledOperator &op, const double *elmat) {
    SA_REQUIRE(elmat || !op.elmat_len, "null argument: elmat");
    if (!op.nnz) return;
    hipStream_t s = op.stream;
    const DevIn<double> in(elmat, (size_t)op.elmat_len, s);
    const double *d = in.p;
    numeric_pass(s, op, d);
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

void operator_eliminate_rhs(const AssembledOperator &op, const double *elmat, const double *x_ess, double *b) {
    SA_REQUIRE(elmat || !op.elmat_len, "null argument: elmat");
    if (!op.n || !op.bdr.p) return;      // no essential dof
    hipStream_t s = op.stream;
    const DevIn<double> in(elmat, (size_t)op.elmat_len, s);
    const double *d = in.p;
    hipLaunchKernelGGL(op_rhs_kernel, grid_flat(op.n), dim3(256), 0, s, op.n, (const int *)op.d2e_I.p, (const int *)op.d2e_J.p,
                       (const int *)op.eI.p, (const int *)op.eJ.p, (const roff_t *)op.moff.p, op.nde, d,
                       (const signed char *)op.bdr.p, (const roff_t *)op.rowptr.p, (const int *)op.col.p, x_ess, b);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

void operator_assemble_rhs(const AssembledOperator &op, const double *elvec, double *b) {
    SA_REQUIRE(elvec || !op.nconn, "null argument: elvec");
    if (!op.n) return;
    hipStream_t s = op.stream;
    const DevIn<double> in(elvec, (size_t)op.nconn, s);
    const double *d = in.p;
    hipLaunchKernelGGL(op_rhs_assemble_kernel, grid_flat(op.n), dim3(256), 0, s, op.n, (const int *)op.d2e_I.p,
                       (const int *)op.d2e_J.p, (const int *)op.eI.p, (const int *)op.eJ.p, d, b);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
