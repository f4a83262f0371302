// Element matrices on the device from vertex coordinates, element -> vertex lists and per-element coefficients: diffusion with
// a scalar / diagonal / symmetric tensor and isotropic linear elasticity on the order-1 triangle, quadrilateral, tetrahedron,
// wedge and hexahedron.  saamge_amd/elmat_model.py defines the result; this file restates it and gives the same bits.
//
// One lane per (element, node): a group of ND lanes owns an element, BLOCK / ND elements per workgroup.  The group stages its
// vertices through LDS and every lane keeps all of them.  Per quadrature point every lane forms the Jacobian, its cofactors and
// determinant (the same operations in every lane of the group, so the same bits), then the gradient of ITS node (times det) and,
// for diffusion, its flux K G_a; the group shares these through LDS (two buffers, one barrier per point).  The lane of node a
// accumulates row block a.  Diffusion entry (a, b) is formed from the operands of the model's a <= b order by both of its
// owners; an elasticity entry is a sum of products whose factors commute, so the two owners agree as well.  The rows go to an
// LDS tile and the workgroup writes the tile as consecutive doubles of the packed output.  A mesh of several types is split
// into one element list per type (make_list, as operator.hip lists rows by path) and each list gets its own launch.
// No floating-point atomics, no cross-lane reduction of values; the only atomic is the integer minimum that names the first
// element with a non-positive determinant.
//
// The order-2 quadrilateral (9 nodes) and hexahedron (27 nodes) have their own kernel, em2_kernel, with its own decomposition
// (27 divides no wavefront and a node's row block of the hex is 243 accumulators): lanes own ENTRIES, see there.  The order-2
// triangle (6 nodes) and tetrahedron (10 nodes) are two more node counts of the same kernel, with the simplex rules.
//
// The zeroth-order forms -- mass matrices, with or without a target they are added to, and load vectors of a nodal source --
// have a kernel family of their own for all nine types (mass_kernel, load_kernel) in em2_kernel's phase structure.
//
// Data at the points of the mass rule -- where the points are, a nodal field and its gradient there, the loads of a source given
// there, the squared errors per element -- has kernels on the first phases of load_kernel with a lane per (element, point,
// component) after them (qp_points_kernel, qp_eval_kernel, qp_load_kernel, qp_error_kernel).
//
// Coefficients at those points -- the stiffness forms and the mass with a coefficient row per point in the place of one per
// element -- run the bodies of em2_kernel and mass_kernel on the mass rule of all nine types (emkq_kernel, mass_kq_kernel).
//
// The boundary forms -- the mass and the loads of a list of faces, added into the owning elements' matrices and vectors -- have
// kernels templated on the face type (bdr_mass_kernel, bdr_load_kernel) and run one pass per local face index.
//
// Where things are.  elmat_ref.h (plain C++, held to the model by a host test): the shape functions of every type, the rules, the
// table builders, the list of the types with with_elem_type / with_face_type / with_vdim, the one dispatch.  This file: the
// device objects of the tables, the kernels with the pieces they share (em_cofactors, em_write_tile), one launcher per family
// that turns a type index into a launch (em_launch_type, mass_launch_type, qp_launch_type, bdr_launch_face), the frame of a
// call (EmFrame: mesh, launch arguments, outputs on the host or the device, the bad word, the loop over the types, the
// refusal, the copy home) and the four drivers on it (stiffness, mass_or_loads, points_call, boundary_forms).  DESIGN.md 4.9.7.
//
// Boundary data at the face points -- where the points of the listed faces are, the outward unit normals, the trace and the whole
// gradient of a nodal field there, the face mass with a coefficient per point and the face loads of data given at the points -- runs
// on the stage and point phases of the boundary forms (bdr_stage_points; bdr_points_kernel, bdr_mass_q_kernel, bdr_load_q_kernel)
// and, for the gradient, on a kernel templated on the element type that stages all nodes of the owning element (bdr_eval_kernel).
// DESIGN.md 4.9.8.
#include "elmat.h"
#include "elmat_ref.h"
#include "devtab.h"

#include <algorithm>
#include <climits>
#include <utility>
#include <vector>

#include "operator.h"

// every rounding of the model is one IEEE operation: no product is fused with the sum that follows it, anywhere in this file
#pragma clang fp contract(off)

namespace saamge_amd {

namespace {

// ---- the reference elements: elmat_ref.h has the shape functions, the rules and the table builders; here are the device objects
// the rule's table of the order-1 types: one set of gradients per point.  The point loop of em_kernel is a real loop (unrolled,
// the compiler forms the Jacobians of all points ahead of the first barrier and runs out of registers) that reads its point's
// line through a wave-uniform index.
template <int DIM, int ND>
__device__ const EmTable<DIM, ND> EM_TABLE = em_table<DIM, ND>();
// the mass rule of all nine types: reference gradients, shape values, weights (RefTable)
template <int DIM, int ND>
__device__ const MassTable<DIM, ND> MASS_TABLE = mass_table<DIM, ND>();
// the stiffness rule of the order-2 types, the two segments: only the tables that are not a mass table are objects of their own
template <int DIM, int ND>
__device__ const Em2Table<DIM, ND> EM2_TABLE = em2_table<DIM, ND>();
template <int FN>
__device__ const BdrTable<2, FN> SEG_TABLE = bdr_table<2, FN>();
template <int DIM, int ND>
__device__ __forceinline__ const Em2Table<DIM, ND> &em2_rule_table() {
    if constexpr (EM2_IS_MASS<DIM, ND>) return MASS_TABLE<DIM, ND>;
    else return EM2_TABLE<DIM, ND>;
}
template <int DIM, int FN>
__device__ __forceinline__ const BdrTable<DIM, FN> &bdr_rule_table() {
    if constexpr (DIM == 3) return MASS_TABLE<2, FN>;
    else return SEG_TABLE<FN>;
}

// threads per workgroup: 256 where the tile of 256 / nd matrices stays within 40 KB of LDS, else one wavefront
constexpr int em_block(int dim, int nd, int kind) {
    const int size = nd * (kind ? dim : 1);
    return (256 / nd) * size * size * 8 <= 40960 ? 256 : 64;
}

// ---- pieces the kernels share (a piece is shared only where the kernel's gfx950 body stays the parent's) ------
// the cofactors C[i][j] of J[i][j] and the determinant (elmat_model._cofactors), in the statement order of em_kernel and em2_body:
// the order of the source decides the operand order of the compiled products
template <int DIM>
__device__ __forceinline__ void em_cofactors(const double (&J)[DIM][DIM], double (&C)[DIM][DIM], double &det) {
    if constexpr (DIM == 2) {
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        C[0][0] = J[1][1];
        C[0][1] = -J[1][0];
        C[1][0] = -J[0][1];
        C[1][1] = J[0][0];
    } else {
        C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        C[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        C[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        C[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        C[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        C[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        C[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        det = (J[0][0] * C[0][0] + J[0][1] * C[0][1]) + J[0][2] * C[0][2];
    }
}
// the doubles of the workgroup's tile that belong to elements (the last workgroup may hold fewer than EPB) ...
template <int EPB, int SS>
__device__ __forceinline__ int em_tile_doubles(int count) {
    const long left = (long)count - (long)blockIdx.x * EPB;
    return (int)(left < EPB ? left : EPB) * SS;
}
// ... and their way out: consecutive lanes write consecutive doubles of the packed output, element l of the tile at obase[l]
template <int BLOCK, int SS>
__device__ __forceinline__ void em_write_tile(int total, const roff_t *obase, const double *tile, double *__restrict__ out) {
    for (int t = threadIdx.x; t < total; t += BLOCK) {
        const int l = t / SS;
        out[obase[l] + (t - l * SS)] = tile[t];
    }
}

// ---- the element matrices -------------------------------------------------------------------------------------------------
// list: the elements of this launch (nullptr: elements 0 .. count - 1); eI nullptr: element e has its vertices at e * ND;
// moff nullptr: its matrix at e * size^2; out nullptr: only the determinants are checked.
template <int DIM, int ND, int KIND>
__global__ __launch_bounds__(em_block(DIM, ND, KIND)) void em_kernel(int count, const int *__restrict__ list,
                                                                      const int *__restrict__ eI, const int *__restrict__ eJ,
                                                                      const roff_t *__restrict__ moff,
                                                                      const double *__restrict__ coords,
                                                                      const double *__restrict__ coef, int ncoef,
                                                                      double *__restrict__ out, int *__restrict__ bad) {
    typedef EmTable<DIM, ND> T;                   // NQ points, the weight W of each
    constexpr int BLOCK = em_block(DIM, ND, KIND), EPB = BLOCK / ND, COMP = KIND ? DIM : 1, S = ND * COMP, SS = S * S;
    constexpr int W = KIND ? DIM : 2 * DIM;       // doubles a node shares per point: G_a, and F_a for diffusion
    __shared__ double tile[EPB * SS];
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sG[2][EPB * ND * W];
    __shared__ roff_t obase[EPB];
    const int tid = threadIdx.x, el = tid / ND, a = tid - el * ND;
    const bool lane = el < EPB;                   // (BLOCK need not be a multiple of ND: the last lanes own nothing)
    const int elc = lane ? el : EPB - 1;
    const long slot = (long)blockIdx.x * EPB + el;
    const bool valid = lane && slot < count;
    int e = 0;
    double lam = 1.0, mu = 1.0, K[DIM][DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int j = 0; j < DIM; ++j) K[i][j] = i == j ? 1.0 : 0.0;
    if (valid) {
        e = list ? list[slot] : (int)slot;
        const long vb = eI ? (long)eI[e] : (long)e * ND;
        const int v = eJ[vb + a];
#pragma unroll
        for (int d = 0; d < DIM; ++d) sX[(el * ND + a) * DIM + d] = coords[(long)v * DIM + d];
        if (a == 0) obase[el] = moff ? moff[e] : (roff_t)e * SS;
        const double *c = coef + (long)e * ncoef;
        if (KIND) {
            lam = c[0];
            mu = c[1];
        } else {
#pragma unroll
            for (int i = 0; i < DIM; ++i) K[i][i] = ncoef == 1 ? c[0] : c[i];
            if (ncoef > DIM) {                    // xx, yy, zz, xy, yz, xz / xx, yy, xy
                K[0][1] = K[1][0] = c[DIM];
                if (DIM == 3) {
                    K[1][DIM - 1] = K[DIM - 1][1] = c[DIM + 1];
                    K[0][DIM - 1] = K[DIM - 1][0] = c[DIM + 2];
                }
            }
        }
    } else if (lane) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) sX[(el * ND + a) * DIM + d] = 0.0;
    }
    __syncthreads();
    double X[ND][DIM];
#pragma unroll
    for (int b = 0; b < ND; ++b)
#pragma unroll
        for (int d = 0; d < DIM; ++d) X[b][d] = sX[(elc * ND + b) * DIM + d];
    double acc[COMP][S];
    bool flag = false;
#pragma unroll
    for (int i = 0; i < COMP; ++i)
#pragma unroll
        for (int c = 0; c < S; ++c) acc[i][c] = 0.0;
#pragma unroll 1
    for (int q = 0; q < T::NQ; ++q) {
        const EmGrad<DIM, ND> &dN = EM_TABLE<DIM, ND>.p[q];
        double J[DIM][DIM], C[DIM][DIM], det;
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
            for (int j = 0; j < DIM; ++j) {
                double t = X[0][i] * dN.v[0][j];
#pragma unroll
                for (int b = 1; b < ND; ++b) t = t + X[b][i] * dN.v[b][j];
                J[i][j] = t;
            }
        em_cofactors<DIM>(J, C, det);
        if (!(det > 0.0)) flag = true;
        const double s = T::W / det;
        // this lane's node: its reference gradient picked from the constants, G_a = C dN_a, F_a = K G_a
        double dA[DIM], Ga[DIM], Fa[DIM];
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            double g = dN.v[0][j];
#pragma unroll
            for (int b = 1; b < ND; ++b) g = a == b ? dN.v[b][j] : g;
            dA[j] = g;
        }
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
            double t = dA[0] * C[i][0] + dA[1] * C[i][1];
            if constexpr (DIM == 3) t = t + dA[2] * C[i][2];
            Ga[i] = t;
        }
        double *share = sG[q & 1];
        if (lane) {
#pragma unroll
            for (int i = 0; i < DIM; ++i) share[(el * ND + a) * W + i] = Ga[i];
        }
        if constexpr (KIND == 0) {
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                double t = K[i][0] * Ga[0] + K[i][1] * Ga[1];
                if constexpr (DIM == 3) t = t + K[i][2] * Ga[2];
                Fa[i] = t;
            }
            if (lane) {
#pragma unroll
                for (int i = 0; i < DIM; ++i) share[(el * ND + a) * W + DIM + i] = Fa[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < ND; ++b) {
            double Gb[DIM];
#pragma unroll
            for (int i = 0; i < DIM; ++i) Gb[i] = share[(elc * ND + b) * W + i];
            if constexpr (KIND == 0) {
                double Fb[DIM];
#pragma unroll
                for (int i = 0; i < DIM; ++i) Fb[i] = share[(elc * ND + b) * W + DIM + i];
                const bool first = a <= b;        // the entry is F_lo . G_hi with lo <= hi
                double t = (first ? Fa[0] : Fb[0]) * (first ? Gb[0] : Ga[0]) + (first ? Fa[1] : Fb[1]) * (first ? Gb[1] : Ga[1]);
                if constexpr (DIM == 3) t = t + (first ? Fa[2] : Fb[2]) * (first ? Gb[2] : Ga[2]);
                const double term = s * t;
                acc[0][b] = acc[0][b] + term;
            } else {
                double dot = Ga[0] * Gb[0] + Ga[1] * Gb[1];
                if constexpr (DIM == 3) dot = dot + Ga[2] * Gb[2];
                const double md = mu * dot;
#pragma unroll
                for (int i = 0; i < DIM; ++i)
#pragma unroll
                    for (int j = 0; j < DIM; ++j) {
                        double t = lam * (Ga[i] * Gb[j]) + mu * (Ga[j] * Gb[i]);
                        if (i == j) t = t + md;
                        const double term = s * t;
                        acc[i][DIM * b + j] = acc[i][DIM * b + j] + term;
                    }
            }
        }
    }
    if (valid && flag) atomicMin(bad, e);
    if (!out) return;                             // (the same in every lane of the grid)
    if (lane) {
#pragma unroll
        for (int i = 0; i < COMP; ++i)
#pragma unroll
            for (int c = 0; c < S; ++c) tile[(el * S + COMP * a + i) * S + c] = acc[i][c];
    }
    __syncthreads();
    const long left = (long)count - (long)blockIdx.x * EPB;
    const int total = (int)(left < EPB ? left : EPB) * SS;
    for (int t = tid; t < total; t += BLOCK) {
        const int l = t / SS;
        out[obase[l] + (t - l * SS)] = tile[t];
    }
}

// ---- order 2: the 9-node quadrilateral, the 27-node hexahedron, the 6-node triangle and the 10-node tetrahedron ------------
// (shape functions, rules and tables: elmat_ref.h; the tensor-product types have as many points as nodes, the triangle 3, the
// tetrahedron 4)
// BLOCK threads, EPB elements per workgroup, BS x BS node pairs per lane in the entry phase, QC points per pass.
// The hex of elasticity: one element (its tile is 52 KB), 378 node pairs on 384 lanes.  The hex of diffusion: lanes own
// 3 x 3 node pairs (the flux of 3 nodes and the gradient of 3 nodes from LDS feed 9 entries: one pair per lane would wait
// for LDS), 45 lanes per element; the gradients of 3 points at a time keep four elements within 27 KB.
// The simplices are small: 21 / 55 node pairs, 3 / 4 points in one pass; 12 triangles (252 lanes, the tile of elasticity
// 13.8 KB) and 4 tetrahedra (220 lanes, 28.8 KB) per workgroup of 256 keep five or more workgroups on a compute unit.
template <int DIM, int ND, int KIND> struct Em2Cfg;
template <> struct Em2Cfg<2, 9, 0> { static constexpr int BLOCK = 256, EPB = 5, BS = 1, QC = 9; };
template <> struct Em2Cfg<2, 9, 1> { static constexpr int BLOCK = 256, EPB = 5, BS = 1, QC = 9; };
template <> struct Em2Cfg<3, 27, 0> { static constexpr int BLOCK = 192, EPB = 4, BS = 3, QC = 3; };
template <> struct Em2Cfg<3, 27, 1> { static constexpr int BLOCK = 384, EPB = 1, BS = 1, QC = 27; };
template <int KIND> struct Em2Cfg<2, 6, KIND> { static constexpr int BLOCK = 256, EPB = 12, BS = 1, QC = 3; };
template <int KIND> struct Em2Cfg<3, 10, KIND> { static constexpr int BLOCK = 256, EPB = 4, BS = 1, QC = 4; };

// list, eI, moff, out: as in em_kernel.  Phases, a barrier between each:
//   stage   the nodes' coordinates and the coefficients of the workgroup's elements into LDS
//   J       one lane per (element, point, i, j): J[i][j], the sum over the nodes in ascending order
//   point   one lane per (element, point): cofactors, det (not positive: the element id to *bad), s = weight / det
//   then per pass of QC points
//   G       one lane per (element, point, node): G_a = C dN_a and, for diffusion, F_a = K G_a
//   entry   one lane per (element, BS x BS block of node pairs a <= b): a real loop over the pass's points, in ascending
//           order, that adds the point's term to the lane's accumulators -- the whole sum of an entry lives in one lane, so
//           the bits are the model's, and no entry is computed twice
//   tile    the entries and their mirror images to an LDS tile (over the dead gradients), written out as consecutive doubles
// K[i * DIM + j] from a row of ncoef coefficients (elmat_model._tensor): ncoef 1 fills the diagonal with c[0], DIM gives the
// diagonal, more the symmetric tensor as xx, yy, zz, xy, yz, xz / xx, yy, xy
template <int DIM>
__device__ __forceinline__ void em_tensor(const double *c, int ncoef, double *K) {
#pragma unroll
    for (int i = 0; i < DIM * DIM; ++i) K[i] = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) K[i * DIM + i] = ncoef == 1 ? c[0] : c[i];
    if (ncoef > DIM) {
        K[0 * DIM + 1] = K[1 * DIM + 0] = c[DIM];
        if (DIM == 3) {
            K[1 * DIM + DIM - 1] = K[(DIM - 1) * DIM + 1] = c[DIM + 1];
            K[0 * DIM + DIM - 1] = K[(DIM - 1) * DIM + 0] = c[DIM + 2];
        }
    }
}

// The body serves two kernels.  em2_kernel: the order-2 types with their stiffness rule (Em2Table) and one coefficient row per
// element (KQ false: coef + e * ncoef, expanded to K[i][j] / lambda, mu in the stage phase).  emkq_kernel, after the mass
// tables: all nine types with their MASS rule (MassTable, the same dN[a][q][j] and w[q]) and one coefficient row per POINT (KQ
// true): the stage phase copies the NQ * ncoef doubles of every element of the workgroup, at coef + qoff[e] * ncoef, as they
// are; the G phase forms K_q from the row of ITS point -- the global q = q0 + qq, not the index in the pass -- and the entry
// phase of elasticity reads lambda_q, mu_q of the point of its term.
template <int DIM, int ND, int KIND, class Cfg, bool KQ, class Table>
__device__ __forceinline__ void em2_body(const Table &T, int count, const int *__restrict__ list, const int *__restrict__ eI,
                                         const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                         const roff_t *__restrict__ qoff, const double *__restrict__ coords,
                                         const double *__restrict__ coef, int ncoef, double *__restrict__ out,
                                         int *__restrict__ bad) {
    constexpr int BLOCK = Cfg::BLOCK, EPB = Cfg::EPB, BS = Cfg::BS, QC = Cfg::QC;
    constexpr int NQ = Table::NQ, COMP = KIND ? DIM : 1, S = ND * COMP, SS = S * S;
    constexpr int NB = ND / BS, NBP = NB * (NB + 1) / 2;      // blocks of nodes, pairs A <= B of them
    constexpr int DD = DIM * DIM, PW = DD + 1;                // a point keeps its cofactors and s
    constexpr int GW = KIND ? DIM : 2 * DIM;                  // a node keeps G_a, and F_a for diffusion
    constexpr int NACC = KIND ? DD : BS * BS;
    constexpr int NP = EPB * NQ * PW, NG = EPB * QC * ND * GW, NT = EPB * SS, WORK = NP + NG > NT ? NP + NG : NT;
    constexpr int NK = KQ ? EPB * NQ * (KIND ? 2 : DIM * (DIM + 1) / 2) : EPB * DD;      // (the longest row a point may have)
    static_assert(EPB * NBP <= BLOCK && NQ % QC == 0 && ND % BS == 0 && NG >= EPB * NQ * DD && (KIND == 0 || BS == 1), "em2 plan");
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sK[NK];                                 // K[i][j], or lambda, mu; KQ: the rows of the points as given
    __shared__ double work[WORK];
    __shared__ roff_t obase[EPB];
    __shared__ int sE[EPB];                                   // the element of a slot, -1: none
    double *const sP = work, *const sG = work + NP, *const sJ = sG, *const tile = work;
    const int tid = threadIdx.x;
    // ---- stage
    for (int idx = tid; idx < EPB * ND; idx += BLOCK) {
        const int el = idx / ND, a = idx - el * ND;
        const long slot = (long)blockIdx.x * EPB + el;
        double x[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) x[d] = 0.0;
        if (slot < count) {
            const int e = list ? list[slot] : (int)slot;
            const long vb = eI ? (long)eI[e] : (long)e * ND;
            const int v = eJ[vb + a];
#pragma unroll
            for (int d = 0; d < DIM; ++d) x[d] = coords[(long)v * DIM + d];
            if (a == 0) {
                sE[el] = e;
                obase[el] = moff ? moff[e] : (roff_t)e * SS;
                if constexpr (!KQ) {
                    const double *c = coef + (long)e * ncoef;
                    double *K = sK + el * DD;
                    if (KIND) {
                        K[0] = c[0];
                        K[1] = c[1];
                    } else {
                        em_tensor<DIM>(c, ncoef, K);
                    }
                }
            }
        } else if (a == 0) {
            sE[el] = -1;
            if constexpr (!KQ) {
#pragma unroll
                for (int i = 0; i < DD; ++i) sK[el * DD + i] = 0.0;
            }
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) sX[idx * DIM + d] = x[d];
    }
    if constexpr (KQ) {       // the rows of the points: NQ * ncoef consecutive doubles per element, point q at (el * NQ + q) * ncoef
        const int row = NQ * ncoef;
        for (int idx = tid; idx < EPB * row; idx += BLOCK) {
            const int el = idx / row;
            const long slot = (long)blockIdx.x * EPB + el;
            double c = 0.0;
            if (slot < count) c = coef[qoff[list ? list[slot] : (int)slot] * ncoef + (idx - el * row)];
            sK[idx] = c;
        }
    }
    __syncthreads();
    // ---- J
    for (int idx = tid; idx < EPB * NQ * DD; idx += BLOCK) {
        const int el = idx / (NQ * DD), r = idx - el * (NQ * DD), q = r / DD, ij = r - q * DD, i = ij / DIM, j = ij - i * DIM;
        const double *X = sX + el * ND * DIM + i;
        double t = X[0] * T.dN[0][q][j];
        for (int a = 1; a < ND; ++a) t = t + X[a * DIM] * T.dN[a][q][j];
        sJ[idx] = t;
    }
    __syncthreads();
    // ---- point
    for (int idx = tid; idx < EPB * NQ; idx += BLOCK) {
        const int el = idx / NQ, q = idx - el * NQ;
        double J[DIM][DIM], C[DIM][DIM], det;
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
            for (int j = 0; j < DIM; ++j) J[i][j] = sJ[idx * DD + i * DIM + j];
        em_cofactors<DIM>(J, C, det);
        if (!(det > 0.0) && sE[el] >= 0) atomicMin(bad, sE[el]);
        double *P = sP + idx * PW;
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
            for (int j = 0; j < DIM; ++j) P[i * DIM + j] = C[i][j];
        P[DD] = T.w[q] / det;
    }
    if (!out) return;                             // (the same in every lane of the grid)
    // ---- this lane's block of node pairs
    const bool own = tid < EPB * NBP;
    const int eb = own ? tid / NBP : 0;
    int A = 0, B = own ? tid - eb * NBP : 0;
    while (B >= NB - A) {
        B -= NB - A;
        ++A;
    }
    B += A;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (int q0 = 0; q0 < NQ; q0 += QC) {
        __syncthreads();                          // the points are there; the last pass (and J) has been read
        // ---- G
        for (int idx = tid; idx < EPB * QC * ND; idx += BLOCK) {
            const int el = idx / (QC * ND), r = idx - el * (QC * ND), qq = r / ND, a = r - qq * ND, q = q0 + qq;
            const double *P = sP + (el * NQ + q) * PW;
            double dA[DIM], G[DIM];
#pragma unroll
            for (int j = 0; j < DIM; ++j) dA[j] = T.dN[a][q][j];
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                double t = dA[0] * P[i * DIM + 0] + dA[1] * P[i * DIM + 1];
                if constexpr (DIM == 3) t = t + dA[2] * P[i * DIM + 2];
                G[i] = t;
            }
            double *g = sG + idx * GW;
#pragma unroll
            for (int i = 0; i < DIM; ++i) g[i] = G[i];
            if constexpr (KIND == 0) {
                const double *K = sK + el * DD;
                double Kq[KQ ? DD : 1];
                if constexpr (KQ) {                           // K_q of THIS point, from its row
                    em_tensor<DIM>(sK + (el * NQ + q) * ncoef, ncoef, Kq);
                    K = Kq;
                }
#pragma unroll
                for (int i = 0; i < DIM; ++i) {
                    double t = K[i * DIM + 0] * G[0] + K[i * DIM + 1] * G[1];
                    if constexpr (DIM == 3) t = t + K[i * DIM + 2] * G[2];
                    g[DIM + i] = t;
                }
            }
        }
        __syncthreads();
        // ---- entry
        const double *Pq = sP + (eb * NQ + q0) * PW + DD;
        const double *ga = sG + (eb * QC * ND + A * BS) * GW, *gb = sG + (eb * QC * ND + B * BS) * GW;
#pragma unroll 1
        for (int qq = 0; qq < QC; ++qq) {
            const double s = Pq[qq * PW];
            const double *pa = ga + qq * ND * GW, *pb = gb + qq * ND * GW;
            if constexpr (KIND == 0) {
                double Fa[BS][DIM], Gb[BS][DIM];
#pragma unroll
                for (int k = 0; k < BS; ++k)
#pragma unroll
                    for (int i = 0; i < DIM; ++i) {
                        Fa[k][i] = pa[k * GW + DIM + i];
                        Gb[k][i] = pb[k * GW + i];
                    }
#pragma unroll
                for (int k = 0; k < BS; ++k)
#pragma unroll
                    for (int l = 0; l < BS; ++l) {            // (a > b inside a diagonal block: computed, never stored)
                        double t = Fa[k][0] * Gb[l][0] + Fa[k][1] * Gb[l][1];
                        if constexpr (DIM == 3) t = t + Fa[k][2] * Gb[l][2];
                        const double term = s * t;
                        acc[k * BS + l] = acc[k * BS + l] + term;
                    }
            } else {
                const double *c = KQ ? sK + (eb * NQ + q0 + qq) * 2 : sK + eb * DD;      // (KQ: the row of the term's point)
                const double lam = c[0], mu = c[1];
                double Ga[DIM], Gb[DIM];
#pragma unroll
                for (int i = 0; i < DIM; ++i) {
                    Ga[i] = pa[i];
                    Gb[i] = pb[i];
                }
                double dot = Ga[0] * Gb[0] + Ga[1] * Gb[1];
                if constexpr (DIM == 3) dot = dot + Ga[2] * Gb[2];
                const double md = mu * dot;
#pragma unroll
                for (int i = 0; i < DIM; ++i)
#pragma unroll
                    for (int j = 0; j < DIM; ++j) {
                        double t = lam * (Ga[i] * Gb[j]) + mu * (Ga[j] * Gb[i]);
                        if (i == j) t = t + md;
                        const double term = s * t;
                        acc[i * DIM + j] = acc[i * DIM + j] + term;
                    }
            }
        }
    }
    __syncthreads();                              // the gradients are dead: the tile takes their place
    // ---- tile
    if (own) {
        double *t = tile + eb * SS;
        if constexpr (KIND == 0) {
#pragma unroll
            for (int k = 0; k < BS; ++k)
#pragma unroll
                for (int l = 0; l < BS; ++l) {
                    const int a = A * BS + k, b = B * BS + l;
                    if (a <= b) t[a * S + b] = t[b * S + a] = acc[k * BS + l];
                }
        } else {
#pragma unroll
            for (int i = 0; i < DIM; ++i)
#pragma unroll
                for (int j = 0; j < DIM; ++j) {
                    const int r = DIM * A + i, c = DIM * B + j;
                    if (r <= c) t[r * S + c] = t[c * S + r] = acc[i * DIM + j];
                }
        }
    }
    __syncthreads();
    em_write_tile<BLOCK, SS>(em_tile_doubles<EPB, SS>(count), obase, tile, out);
}

template <int DIM, int ND, int KIND>
__global__ __launch_bounds__((Em2Cfg<DIM, ND, KIND>::BLOCK)) void em2_kernel(int count, const int *__restrict__ list,
                                                                           const int *__restrict__ eI, const int *__restrict__ eJ,
                                                                           const roff_t *__restrict__ moff,
                                                                           const double *__restrict__ coords,
                                                                           const double *__restrict__ coef, int ncoef,
                                                                           double *__restrict__ out, int *__restrict__ bad) {
    em2_body<DIM, ND, KIND, Em2Cfg<DIM, ND, KIND>, false>(em2_rule_table<DIM, ND>(), count, list, eI, eJ, moff, nullptr, coords, coef,
                                                          ncoef, out, bad);
}

// ---- mass matrices and load vectors ------------------------------------------------------------------------------------------
// elmat_model.py's element_mass / element_loads.  The rule of a type is its stiffness rule, except for the simplices: three
// points (EM_WEDGE_TRI, weight 1/6) on the triangle and four (EM_TET_A / EM_TET_B, weight 1/24) on the tetrahedron.  The order-2
// simplices: 6 points (degree 4) on the triangle, 14 (degree 5) on the tetrahedron -- elmat_model's P2_TRI_POINTS / P2_TET_POINTS.
// (ref_mass_rule and MASS_TABLE, above)

// the node pairs a <= b of an element, row by row: a * 32 + b
template <int ND>
struct MassPairs {
    unsigned short ab[ND * (ND + 1) / 2];
};
template <int ND>
constexpr MassPairs<ND> mass_pairs() {
    MassPairs<ND> p{};
    int k = 0;
    for (int a = 0; a < ND; ++a)
        for (int b = a; b < ND; ++b) p.ab[k++] = (unsigned short)(a * 32 + b);
    return p;
}
template <int ND>
__device__ const MassPairs<ND> MASS_PAIRS = mass_pairs<ND>();

constexpr int MASS_BLOCK = 256;
// elements per workgroup: a tile of at most 24 KB, at most 32 elements; the order-2 hexahedron of the vector form alone (52 KB)
// the tetrahedron of order 2, scalar form: 16, its 14 Jacobians per element (not the tile) fill the work space
constexpr int mass_epb(int nd, int vdim) {
    const int e = 24576 / (nd * vdim * nd * vdim * 8);
    return nd == 10 && vdim == 1 ? 16 : (e < 1 ? 1 : (e > 32 ? 32 : e));
}
constexpr int load_epb(int nd) { return nd >= 27 ? 8 : (nd >= 8 ? 16 : 32); }

// The first phases of both kernels (em2_kernel's, for every type), a barrier after each:
//   J       one lane per (element, point, i, j): J[i][j], the sum over the nodes in ascending order
//   point   one lane per (element, point): det from the cofactors (not positive: the element id to *bad),
//           s = (weight * det) * c -- no division
// Order 1 (at most 8 nodes): the lane of a point forms its whole Jacobian in registers -- per node 6 doubles from LDS feed 9
// products, where a lane per J[i][j] reads 2 doubles per product and the phase waits for LDS -- and goes on to the point's
// det without a barrier; J[i][j] is the same sum in the same order.
// sX: the nodes' coordinates, sD: the rule's reference gradients (dN[a][q][j], the LDS copy mass_stage made: a lane of J
// reads ND of them at addresses that differ from lane to lane, which the vector memory path serves a few lanes per clock),
// sC: c per element, sE: the element of a slot (-1: none); sJ and sD may lie over anything that is written after the barrier
// that follows.
// KEEP: the point's cofactors C[i][j] (elmat_model._cofactors) and det go to sP as DIM * DIM + 1 doubles per (element, point).
// CQ: the coefficient of a point stands in sS where its s goes, in the place of sC[el] (elmat_model.element_mass_points).
template <int DIM, int ND, int EPB, bool KEEP = false, bool CQ = false>
__device__ inline void mass_point_phases(const double *sX, const double *sD, const double *sC, const int *sE, double *sJ, double *sS,
                                         int *bad, double *sP = nullptr) {
    constexpr int NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    const MassTable<DIM, ND> &T = MASS_TABLE<DIM, ND>;
    const int tid = threadIdx.x;
    constexpr bool WHOLE = ND <= 8;
    if constexpr (!WHOLE) {
        for (int idx = tid; idx < EPB * NQ * DD; idx += MASS_BLOCK) {
            const int el = idx / (NQ * DD), r = idx - el * (NQ * DD), q = r / DD, ij = r - q * DD, i = ij / DIM, j = ij - i * DIM;
            const double *X = sX + el * ND * DIM + i, *D = sD + q * DIM + j;
            double t = X[0] * D[0];
            for (int a = 1; a < ND; ++a) t = t + X[a * DIM] * D[a * NQ * DIM];
            sJ[idx] = t;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < EPB * NQ; idx += MASS_BLOCK) {
        const int el = idx / NQ, q = idx - el * NQ;
        double J[DIM][DIM], det;
        if constexpr (WHOLE) {
            const double *X = sX + el * ND * DIM, *D = sD + q * DIM;
#pragma unroll
            for (int a = 0; a < ND; ++a)
#pragma unroll
                for (int i = 0; i < DIM; ++i)
#pragma unroll
                    for (int j = 0; j < DIM; ++j) {
                        const double p = X[a * DIM + i] * D[a * NQ * DIM + j];
                        J[i][j] = a ? J[i][j] + p : p;
                    }
        } else {
#pragma unroll
            for (int i = 0; i < DIM; ++i)
#pragma unroll
                for (int j = 0; j < DIM; ++j) J[i][j] = sJ[idx * DD + i * DIM + j];
        }
        if constexpr (DIM == 2) {
            det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            if constexpr (KEEP) {
                double *P = sP + idx * (DD + 1);
                P[0] = J[1][1];
                P[1] = -J[1][0];
                P[2] = -J[0][1];
                P[3] = J[0][0];
            }
        } else {
            const double C00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
            const double C01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
            const double C02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            det = (J[0][0] * C00 + J[0][1] * C01) + J[0][2] * C02;
            if constexpr (KEEP) {
                double *P = sP + idx * (DD + 1);
                P[0] = C00;
                P[1] = C01;
                P[2] = C02;
                P[3] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
                P[4] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
                P[5] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
                P[6] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
                P[7] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
                P[8] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            }
        }
        if constexpr (KEEP) sP[idx * (DD + 1) + DD] = det;
        if (!(det > 0.0) && sE[el] >= 0) atomicMin(bad, sE[el]);
        sS[idx] = (T.w[q] * det) * (CQ ? sS[idx] : sC[el]);
    }
    __syncthreads();
}

// stage of both kernels: coordinates, coefficient (coef nullptr: 1.0), element id, the rule's shape values and reference
// gradients; src (nullptr: none): the nodal source (NV x VDIM) of the nodes to sF.  COEF false: sC is left to the caller.
template <int DIM, int ND, int VDIM, int EPB, bool COEF = true>
__device__ inline void mass_stage(int count, const int *__restrict__ list, const int *__restrict__ eI, const int *__restrict__ eJ,
                                  const double *__restrict__ coords, const double *__restrict__ coef,
                                  const double *__restrict__ src, double *sX, double *sC, int *sE, double *sN, double *sD,
                                  double *sF) {
    constexpr int NQ = MassTable<DIM, ND>::NQ;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < EPB * ND; idx += MASS_BLOCK) {
        const int el = idx / ND, a = idx - el * ND;
        const long slot = (long)blockIdx.x * EPB + el;
        double x[DIM], f[VDIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) x[d] = 0.0;
#pragma unroll
        for (int i = 0; i < VDIM; ++i) f[i] = 0.0;
        if (slot < count) {
            const int e = list ? list[slot] : (int)slot;
            const long vb = eI ? (long)eI[e] : (long)e * ND;
            const int v = eJ[vb + a];
#pragma unroll
            for (int d = 0; d < DIM; ++d) x[d] = coords[(long)v * DIM + d];
            if (src) {
#pragma unroll
                for (int i = 0; i < VDIM; ++i) f[i] = src[(long)v * VDIM + i];
            }
            if (a == 0) {
                sE[el] = e;
                if constexpr (COEF) sC[el] = coef ? coef[e] : 1.0;
            }
        } else if (a == 0) {
            sE[el] = -1;
            if constexpr (COEF) sC[el] = 0.0;
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) sX[idx * DIM + d] = x[d];
        if (src) {
#pragma unroll
            for (int i = 0; i < VDIM; ++i) sF[idx * VDIM + i] = f[i];
        }
    }
    const double *N = &MASS_TABLE<DIM, ND>.N[0][0];
    for (int idx = tid; idx < NQ * ND; idx += MASS_BLOCK) sN[idx] = N[idx];
    const double *D = &MASS_TABLE<DIM, ND>.dN[0][0][0];
    for (int idx = tid; idx < ND * NQ * DIM; idx += MASS_BLOCK) sD[idx] = D[idx];
    __syncthreads();
}

// The mass matrices.  list, eI, moff, out: as in em_kernel; out holds the matrices to add to when accumulate.  Phases:
//   stage, J, point   above
//   fill    (vector form or accumulate) the tile from zeros or from the target, as consecutive doubles; an entry between two
//           components gets its + 0.0 here
//   entry   one lane per (element, node pair a <= b): the whole sum over the points, in ascending order, lives in the lane; it
//           goes (is added) to the tile at (a, b) and (b, a) of every component
//   tile    written out as consecutive doubles
// The body serves mass_kernel (CQ false: coef one double per element) and mass_kq_kernel (CQ true: coef one double per POINT,
// point q of element e at qoff[e] + q, staged into sS ahead of mass_stage, whose barrier covers it; the point phase replaces
// it by s, so the workgroup takes no more LDS than mass_kernel's).
template <int DIM, int ND, int VDIM, bool CQ>
__device__ __forceinline__ void mass_body(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                          const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                          const roff_t *__restrict__ qoff, const double *__restrict__ coords,
                                          const double *__restrict__ coef, int accumulate, double *out, int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = mass_epb(ND, VDIM), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    constexpr int S = ND * VDIM, SS = S * S, NPAIR = ND * (ND + 1) / 2;
    constexpr int NT = EPB * SS, NJ = ND <= 8 ? 0 : EPB * NQ * DD;      // (order 1 keeps J in registers)
    constexpr int ND_ = ND * NQ * DIM, WORK = NT > NJ + ND_ ? NT : NJ + ND_;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double work[WORK];
    __shared__ roff_t obase[EPB];
    __shared__ int sE[EPB];
    double *const tile = work;
    const int tid = threadIdx.x;
    if constexpr (CQ) {
        for (int idx = tid; idx < EPB * NQ; idx += BLOCK) {
            const int el = idx / NQ;
            const long slot = (long)blockIdx.x * EPB + el;
            sS[idx] = slot < count ? coef[qoff[list ? list[slot] : (int)slot] + (idx - el * NQ)] : 0.0;
        }
    }
    mass_stage<DIM, ND, 1, EPB, !CQ>(count, list, eI, eJ, coords, coef, nullptr, sX, sC, sE, sN, work + NJ, nullptr);
    mass_point_phases<DIM, ND, EPB, false, CQ>(sX, work + NJ, sC, sE, work, sS, bad);      // (J and the gradients lie under the tile)
    if (!out) return;                             // (the same in every lane of the grid)
    if (tid < EPB) obase[tid] = sE[tid] < 0 ? 0 : (moff ? moff[sE[tid]] : (roff_t)sE[tid] * SS);
    __syncthreads();
    const int total = em_tile_doubles<EPB, SS>(count);
    const bool fill = VDIM > 1 || accumulate;
    if (fill) {
        // ---- fill
        for (int t = tid; t < total; t += BLOCK) {
            const int l = t / SS, rc = t - l * SS, r = rc / S, c = rc - r * S;
            double v = accumulate ? out[obase[l] + rc] : 0.0;
            if (r % VDIM != c % VDIM) v = v + 0.0;
            tile[t] = v;
        }
        __syncthreads();
    }
    // ---- entry
    for (int idx = tid; idx < EPB * NPAIR; idx += BLOCK) {
        const int el = idx / NPAIR, ab = MASS_PAIRS<ND>.ab[idx - el * NPAIR], a = ab >> 5, b = ab & 31;
        const double *s = sS + el * NQ;
        double acc = 0.0;
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) {
            const double term = s[q] * (sN[q * ND + a] * sN[q * ND + b]);
            acc = acc + term;
        }
        double *t = tile + el * SS;
#pragma unroll
        for (int i = 0; i < VDIM; ++i) {
            const int r = VDIM * a + i, c = VDIM * b + i;
            t[r * S + c] = fill ? t[r * S + c] + acc : acc;
            if (a != b) t[c * S + r] = fill ? t[c * S + r] + acc : acc;
        }
    }
    __syncthreads();
    // ---- tile
    em_write_tile<BLOCK, SS>(total, obase, tile, out);
}

template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void mass_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                          const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                                          const double *__restrict__ coords, const double *__restrict__ coef,
                                                          int accumulate, double *out, int *__restrict__ bad) {
    mass_body<DIM, ND, VDIM, false>(count, list, eI, eJ, moff, nullptr, coords, coef, accumulate, out, bad);
}
// coefq: one coefficient per point, point q of element e at qoff[e] + q
template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void mass_kq_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                             const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                                             const roff_t *__restrict__ qoff, const double *__restrict__ coords,
                                                             const double *__restrict__ coefq, int accumulate, double *out,
                                                             int *__restrict__ bad) {
    mass_body<DIM, ND, VDIM, true>(count, list, eI, eJ, moff, qoff, coords, coefq, accumulate, out, bad);
}

// ---- the element matrices with coefficients at the points (elmat_model.element_matrices_points) -------------------------------
// em2_kernel's body on the MASS rule of every type, a coefficient row per point.  The plans of the order-1 types: one node pair
// per lane, all points in one pass (the hexahedron of diffusion: two passes of 4, which halves the gradients kept), as many
// elements as fill 256 lanes: 42 triangles (252 lanes), 25 quadrilaterals / tetrahedra (250), 12 wedges (252), 7 hexahedra (252).
// The order-2 types keep Em2Cfg's plans; the 10-node tetrahedron has 14 points here and takes two passes of 7 (4 does not
// divide 14).  The largest workgroups: the 27-node hexahedron (Em2Cfg's 27 / 53 KB plus the rows of its points) and the tiles of
// elasticity of the wedge and the hexahedron (31 / 32 KB).
template <int DIM, int ND, int KIND> struct EmKqCfg : Em2Cfg<DIM, ND, KIND> {};
template <int KIND> struct EmKqCfg<2, 3, KIND> { static constexpr int BLOCK = 256, EPB = 42, BS = 1, QC = 3; };
template <int KIND> struct EmKqCfg<2, 4, KIND> { static constexpr int BLOCK = 256, EPB = 25, BS = 1, QC = 4; };
template <int KIND> struct EmKqCfg<3, 4, KIND> { static constexpr int BLOCK = 256, EPB = 25, BS = 1, QC = 4; };
template <int KIND> struct EmKqCfg<3, 6, KIND> { static constexpr int BLOCK = 256, EPB = 12, BS = 1, QC = 6; };
template <> struct EmKqCfg<3, 8, 0> { static constexpr int BLOCK = 256, EPB = 7, BS = 1, QC = 4; };
template <> struct EmKqCfg<3, 8, 1> { static constexpr int BLOCK = 256, EPB = 7, BS = 1, QC = 8; };
template <int KIND> struct EmKqCfg<3, 10, KIND> { static constexpr int BLOCK = 256, EPB = 4, BS = 1, QC = 7; };

// coefq: NQ x ncoef, the row of point q of element e at (qoff[e] + q) * ncoef; everything else as em2_kernel
template <int DIM, int ND, int KIND>
__global__ __launch_bounds__((EmKqCfg<DIM, ND, KIND>::BLOCK)) void emkq_kernel(int count, const int *__restrict__ list,
                                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                                             const roff_t *__restrict__ moff,
                                                                             const roff_t *__restrict__ qoff,
                                                                             const double *__restrict__ coords,
                                                                             const double *__restrict__ coefq, int ncoef,
                                                                             double *__restrict__ out, int *__restrict__ bad) {
    em2_body<DIM, ND, KIND, EmKqCfg<DIM, ND, KIND>, true>(MASS_TABLE<DIM, ND>, count, list, eI, eJ, moff, qoff, coords, coefq, ncoef,
                                                          out, bad);
}

// the last phase of the load kernels: sQ holds s * fq per (element, point, component)
template <int ND, int VDIM, int EPB, int NQ>
__device__ inline void load_dof_phase(const int *__restrict__ eI, const int *sE, const double *sQ, const double *sN,
                                      double *__restrict__ out) {
    for (int idx = threadIdx.x; idx < EPB * ND * VDIM; idx += MASS_BLOCK) {
        const int el = idx / (ND * VDIM), r = idx - el * (ND * VDIM), a = r / VDIM, i = r - a * VDIM;
        const int e = sE[el];
        if (e < 0) continue;
        const double *Q = sQ + el * NQ * VDIM + i;
        double acc = 0.0;
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) {
            const double term = Q[q * VDIM] * sN[q * ND + a];
            acc = acc + term;
        }
        const long vb = eI ? (long)eI[e] : (long)e * ND;
        out[vb * VDIM + r] = acc;
    }
}

// The load vectors: element e's ND * VDIM doubles at VDIM * (its offset in the vertex lists).  Phases:
//   stage, J, point   above; the nodal source of the element's nodes is staged with the coordinates
//   source  one lane per (element, point, component): fq = sum over the nodes, ascending, of N_c * src_c; s * fq is kept
//   dof     one lane per (element, node, component): the whole sum over the points of (s * fq) * N_a, written where it belongs
template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void load_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                          const int *__restrict__ eJ, const double *__restrict__ coords,
                                                          const double *__restrict__ coef, const double *__restrict__ src,
                                                          double *__restrict__ out, int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = load_epb(ND), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sF[EPB * ND * VDIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double sJ[ND <= 8 ? 1 : EPB * NQ * DD];      // (order 1 keeps J in registers)
    __shared__ double sD[ND * NQ * DIM];
    __shared__ double sQ[EPB * NQ * VDIM];
    __shared__ int sE[EPB];
    const int tid = threadIdx.x;
    mass_stage<DIM, ND, VDIM, EPB>(count, list, eI, eJ, coords, coef, src, sX, sC, sE, sN, sD, sF);
    mass_point_phases<DIM, ND, EPB>(sX, sD, sC, sE, sJ, sS, bad);
    if (!out) return;                             // (the same in every lane of the grid)
    // ---- source
    for (int idx = tid; idx < EPB * NQ * VDIM; idx += BLOCK) {
        const int el = idx / (NQ * VDIM), r = idx - el * (NQ * VDIM), q = r / VDIM, i = r - q * VDIM;
        const double *F = sF + el * ND * VDIM + i, *N = sN + q * ND;
        double fq = N[0] * F[0];
        for (int c = 1; c < ND; ++c) fq = fq + N[c] * F[c * VDIM];
        sQ[idx] = sS[el * NQ + q] * fq;
    }
    __syncthreads();
    load_dof_phase<ND, VDIM, EPB, NQ>(eI, sE, sQ, sN, out);
}

// ---- data at the points of the mass rule --------------------------------------------------------------------------------------
// elmat_model.py's element_points / element_eval / element_loads_points / element_errors.  Point q of element e has the global
// index qoff[e] + q (qoff: NE + 1 offsets, 64 bits).  The kernels are load_kernel's: stage, J and point as above (the rules are
// MASS_TABLE's, nothing is restated), then ONE LANE PER (element, point, component) -- the outputs are point-major, and the
// points of the consecutive elements of a workgroup are consecutive in them, so consecutive lanes store consecutive doubles (a
// lane per element would store NQ * DIM doubles apart).  No lane adds to what another lane wrote and no total is formed.
// Elements per workgroup: load_kernel's, except the order-2 hexahedron, where eval and errors keep the cofactors of 27 points per
// element too (qp_load_kernel keeps none and takes load_epb).
constexpr int qp_epb(int nd) { return nd >= 27 ? 4 : load_epb(nd); }

// uq = sum over the nodes, ascending, of N_a * f_a and, GRAD, g[j] = (r[0] * C[j][0] + r[1] * C[j][1] (+ r[2] * C[j][2])) / det
// with r[k] = sum over the nodes, ascending, of f_a * dN_a[k].  F: the component's nodal values (stride VDIM), N: the point's
// shape values, D: the point's reference gradients (node stride NQ * DIM), P: the point's cofactors and det.
template <int DIM, int ND, int VDIM, bool GRAD>
__device__ inline void qp_value(const double *F, const double *N, const double *D, const double *P, double &uq, double g[DIM]) {
    constexpr int NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    double r[DIM];
    uq = N[0] * F[0];
    if constexpr (GRAD) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) r[k] = F[0] * D[k];
    }
    for (int a = 1; a < ND; ++a) {
        const double f = F[a * VDIM];
        uq = uq + N[a] * f;
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < DIM; ++k) r[k] = r[k] + f * D[a * NQ * DIM + k];
        }
    }
    if constexpr (GRAD) {
        const double det = P[DD];
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            double t = r[0] * P[j * DIM + 0] + r[1] * P[j * DIM + 1];
            if constexpr (DIM == 3) t = t + r[2] * P[j * DIM + 2];
            g[j] = t / det;
        }
    }
}

// the points: xq (NQ x DIM) and wdet (NQ); either may be nullptr
template <int DIM, int ND>
__global__ __launch_bounds__(MASS_BLOCK) void qp_points_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                               const int *__restrict__ eJ, const roff_t *__restrict__ qoff,
                                                               const double *__restrict__ coords, double *__restrict__ xq,
                                                               double *__restrict__ wdet, int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = qp_epb(ND), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double sJ[ND <= 8 ? 1 : EPB * NQ * DD];
    __shared__ double sD[ND * NQ * DIM];
    __shared__ roff_t sO[EPB];
    __shared__ int sE[EPB];
    const int tid = threadIdx.x;
    mass_stage<DIM, ND, 1, EPB>(count, list, eI, eJ, coords, nullptr, nullptr, sX, sC, sE, sN, sD, nullptr);
    if (tid < EPB) sO[tid] = sE[tid] < 0 ? 0 : qoff[sE[tid]];
    mass_point_phases<DIM, ND, EPB>(sX, sD, sC, sE, sJ, sS, bad);      // (the coefficient is 1.0: s = weight * det)
    if (wdet) {
        for (int idx = tid; idx < EPB * NQ; idx += BLOCK) {
            const int el = idx / NQ;
            if (sE[el] >= 0) wdet[sO[el] + (idx - el * NQ)] = sS[idx];
        }
    }
    if (xq) {
        for (int idx = tid; idx < EPB * NQ * DIM; idx += BLOCK) {
            const int el = idx / (NQ * DIM), r = idx - el * (NQ * DIM), q = r / DIM, i = r - q * DIM;
            if (sE[el] < 0) continue;
            double x, unused[DIM];
            qp_value<DIM, ND, DIM, false>(sX + el * ND * DIM + i, sN + q * ND, nullptr, nullptr, x, unused);
            xq[sO[el] * DIM + r] = x;
        }
    }
}

// the nodal u (NV x VDIM) at the points: uq (NQ x VDIM) and gradq (NQ x VDIM x DIM); either may be nullptr
template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void qp_eval_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                             const int *__restrict__ eJ, const roff_t *__restrict__ qoff,
                                                             const double *__restrict__ coords, const double *__restrict__ u,
                                                             double *__restrict__ uq, double *__restrict__ gradq,
                                                             int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = qp_epb(ND), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM, PW = DD + 1;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sF[EPB * ND * VDIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double sJ[ND <= 8 ? 1 : EPB * NQ * DD];
    __shared__ double sD[ND * NQ * DIM];
    __shared__ double sP[EPB * NQ * PW];
    __shared__ roff_t sO[EPB];
    __shared__ int sE[EPB];
    const int tid = threadIdx.x;
    mass_stage<DIM, ND, VDIM, EPB>(count, list, eI, eJ, coords, nullptr, u, sX, sC, sE, sN, sD, sF);
    if (tid < EPB) sO[tid] = sE[tid] < 0 ? 0 : qoff[sE[tid]];
    mass_point_phases<DIM, ND, EPB, true>(sX, sD, sC, sE, sJ, sS, bad, sP);
    for (int idx = tid; idx < EPB * NQ * VDIM; idx += BLOCK) {
        const int el = idx / (NQ * VDIM), r = idx - el * (NQ * VDIM), q = r / VDIM, i = r - q * VDIM;
        if (sE[el] < 0) continue;
        const double *F = sF + el * ND * VDIM + i, *N = sN + q * ND, *D = sD + q * DIM, *P = sP + (el * NQ + q) * PW;
        const roff_t at = sO[el] * VDIM + r;
        double v, g[DIM];
        if (gradq) {
            qp_value<DIM, ND, VDIM, true>(F, N, D, P, v, g);
#pragma unroll
            for (int j = 0; j < DIM; ++j) gradq[at * DIM + j] = g[j];
        } else {
            qp_value<DIM, ND, VDIM, false>(F, N, D, P, v, g);
        }
        if (uq) uq[at] = v;
    }
}

// the load vectors of fq (NQ x VDIM) given at the points: load_kernel with the source read where load_kernel interpolates it
template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void qp_load_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                             const int *__restrict__ eJ, const roff_t *__restrict__ qoff,
                                                             const double *__restrict__ coords, const double *__restrict__ coef,
                                                             const double *__restrict__ fq, double *__restrict__ out,
                                                             int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = load_epb(ND), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double sJ[ND <= 8 ? 1 : EPB * NQ * DD];
    __shared__ double sD[ND * NQ * DIM];
    __shared__ double sQ[EPB * NQ * VDIM];
    __shared__ roff_t sO[EPB];
    __shared__ int sE[EPB];
    const int tid = threadIdx.x;
    mass_stage<DIM, ND, 1, EPB>(count, list, eI, eJ, coords, coef, nullptr, sX, sC, sE, sN, sD, nullptr);
    if (tid < EPB) sO[tid] = sE[tid] < 0 ? 0 : qoff[sE[tid]];
    mass_point_phases<DIM, ND, EPB>(sX, sD, sC, sE, sJ, sS, bad);
    // ---- source
    for (int idx = tid; idx < EPB * NQ * VDIM; idx += BLOCK) {
        const int el = idx / (NQ * VDIM), r = idx - el * (NQ * VDIM);
        sQ[idx] = sE[el] < 0 ? 0.0 : sS[el * NQ + r / VDIM] * fq[sO[el] * VDIM + r];
    }
    __syncthreads();
    load_dof_phase<ND, VDIM, EPB, NQ>(eI, sE, sQ, sN, out);
}

// the squared errors of the nodal u per element: err[e][0] against exq (NQ x VDIM), err[e][1] of the gradient against exgradq
// (NQ x VDIM x DIM); exact data nullptr: 0.0.  After stage, J and point:
//   point   one lane per (element, point): the components in ascending order, wdet * d to LDS
//   sum     one lane per (element, column): the whole sum over the points, in ascending order, lives in the lane
template <int DIM, int ND, int VDIM>
__global__ __launch_bounds__(MASS_BLOCK) void qp_error_kernel(int count, const int *__restrict__ list, const int *__restrict__ eI,
                                                              const int *__restrict__ eJ, const roff_t *__restrict__ qoff,
                                                              const double *__restrict__ coords, const double *__restrict__ u,
                                                              const double *__restrict__ exq, const double *__restrict__ exgradq,
                                                              double *__restrict__ err, int *__restrict__ bad) {
    constexpr int BLOCK = MASS_BLOCK, EPB = qp_epb(ND), NQ = MassTable<DIM, ND>::NQ, DD = DIM * DIM, PW = DD + 1;
    __shared__ double sX[EPB * ND * DIM];
    __shared__ double sF[EPB * ND * VDIM];
    __shared__ double sN[NQ * ND];
    __shared__ double sS[EPB * NQ];
    __shared__ double sC[EPB];
    __shared__ double sJ[ND <= 8 ? 1 : EPB * NQ * DD];
    __shared__ double sD[ND * NQ * DIM];
    __shared__ double sP[EPB * NQ * PW];
    __shared__ double sQ[EPB * NQ * 2];
    __shared__ roff_t sO[EPB];
    __shared__ int sE[EPB];
    const int tid = threadIdx.x;
    mass_stage<DIM, ND, VDIM, EPB>(count, list, eI, eJ, coords, nullptr, u, sX, sC, sE, sN, sD, sF);
    if (tid < EPB) sO[tid] = sE[tid] < 0 ? 0 : qoff[sE[tid]];
    mass_point_phases<DIM, ND, EPB, true>(sX, sD, sC, sE, sJ, sS, bad, sP);
    // ---- point
    for (int idx = tid; idx < EPB * NQ; idx += BLOCK) {
        const int el = idx / NQ, q = idx - el * NQ;
        double d0 = 0.0, d1 = 0.0;
        if (sE[el] >= 0) {
            const roff_t at = (sO[el] + q) * VDIM;
            for (int i = 0; i < VDIM; ++i) {
                const double *F = sF + el * ND * VDIM + i, *N = sN + q * ND, *D = sD + q * DIM, *P = sP + idx * PW;
                double v, g[DIM];
                if (exgradq) {
                    qp_value<DIM, ND, VDIM, true>(F, N, D, P, v, g);
#pragma unroll
                    for (int j = 0; j < DIM; ++j) {
                        const double d = g[j] - exgradq[(at + i) * DIM + j];
                        const double dd = d * d;
                        d1 = i + j ? d1 + dd : dd;
                    }
                } else {
                    qp_value<DIM, ND, VDIM, false>(F, N, D, P, v, g);
                }
                if (exq) {
                    const double d = v - exq[at + i];
                    const double dd = d * d;
                    d0 = i ? d0 + dd : dd;
                }
            }
        }
        sQ[idx * 2] = exq ? sS[idx] * d0 : 0.0;
        sQ[idx * 2 + 1] = exgradq ? sS[idx] * d1 : 0.0;
    }
    __syncthreads();
    // ---- sum
    for (int idx = tid; idx < EPB * 2; idx += BLOCK) {
        const int el = idx >> 1, e = sE[el];
        if (e < 0) continue;
        const double *Q = sQ + el * NQ * 2 + (idx & 1);
        double acc = 0.0;
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) acc = acc + Q[q * 2];
        err[(long)e * 2 + (idx & 1)] = acc;
    }
}

// ---- boundary forms: the face mass and the face loads -----------------------------------------------------------------------
// elmat_model.py's boundary_mass / boundary_loads.  A face is (element, local face index); the face types are the 2-node and
// 3-node segment (DIM 2) and the triangle, the 4-node and the 9-node quadrilateral and the 6-node triangle (DIM 3).  The kernels are templated on the
// FACE type <DIM, FN>; the element type enters through the local node ids of the face (BdrFace, a kernel argument), the
// element's node count nd and its offsets.  The host buckets the faces by (element type, local face) and runs one pass per local
// face index in ascending order on the stream: within a pass an element occurs at most once, so the read-modify-write of its
// entries needs no atomic and the model's order of additions holds by construction.
// info[0 .. 4]: 2-node segments, 3-node segments (of 9-node quadrilaterals and of 6-node triangles), triangles of 3 and of 6
// nodes, 4-node quadrilaterals, 9-node quadrilaterals
constexpr int bdr_face_type(int dim, int fn) { return dim == 2 ? fn - 2 : (fn == 3 || fn == 6 ? 2 : (fn == 4 ? 3 : 4)); }
// (BdrFace, bdr_num_faces, BDR_FACE_NODES and bdr_face: elmat_types.h)

// (the rule of a face type: ref_face_rule; its table: bdr_rule_table, above)

constexpr int BDR_BLOCK = 256;
constexpr int bdr_fpb(int fn) { return fn == 9 ? 5 : (fn == 4 ? 16 : 32); }      // faces per workgroup

// (the checks of a face list: check_face_list, mesh.hip)

// Phases of both kernels, a barrier after each:
//   stage   one lane per (face, face node): the node's coordinates (and g) into LDS; the face's element, coefficient, offsets
//   point   one lane per (face, point): the tangents, m2, meas = sqrt(m2) and s = (w * meas) * c in registers; a measure that
//           is not positive sends the face's index in the list to the integer minimum *bad
// list: the faces of this launch (indices into face_elem / coef), all of one element type (nd nodes) and one local face F.
// fp (the calls on data at the face points; nullptr: none): the offsets of the faces' points, fp[f] of every staged face to sO.
// CQ: coef holds one coefficient per POINT, point q of face f at fp[f] + q, in the place of one per face.  GEOM: the unit normal
// of every point to sNrm, DIM doubles per (face, point): (n0, n1, n2) / meas, in 2D (t_y, -t_x) / meas, the division last.
template <int DIM, int FN, int VDIM, int FPB, bool CQ = false, bool GEOM = false>
__device__ inline void bdr_stage_points(int count, const int *__restrict__ list, const BdrFace &F, int nd, const int *__restrict__ eI,
                                        const int *__restrict__ eJ, const int *__restrict__ face_elem,
                                        const double *__restrict__ coords, const double *__restrict__ coef,
                                        const double *__restrict__ g, double *sX, double *sG, double *sS, int *sE, int *bad,
                                        const roff_t *__restrict__ fp = nullptr, roff_t *sO = nullptr, double *sNrm = nullptr) {
    constexpr int NQ = BdrTable<DIM, FN>::NQ;
    const BdrTable<DIM, FN> &T = bdr_rule_table<DIM, FN>();
    __shared__ double sC[FPB];
    __shared__ int sF[FPB];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < FPB * FN; idx += BDR_BLOCK) {
        const int fl = idx / FN, a = idx - fl * FN;
        const long slot = (long)blockIdx.x * FPB + fl;
        double x[DIM], gv[VDIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) x[d] = 0.0;
#pragma unroll
        for (int i = 0; i < VDIM; ++i) gv[i] = 0.0;
        if (slot < count) {
            const int f = list[slot], e = face_elem[f];
            const long vb = eI ? (long)eI[e] : (long)e * nd;
            const int v = eJ[vb + F.node[a]];
#pragma unroll
            for (int d = 0; d < DIM; ++d) x[d] = coords[(long)v * DIM + d];
            if (g) {
#pragma unroll
                for (int i = 0; i < VDIM; ++i) gv[i] = g[(long)v * VDIM + i];
            }
            if (a == 0) {
                sE[fl] = e;
                sF[fl] = f;
                sC[fl] = coef && !CQ ? coef[f] : 1.0;
                if (fp) sO[fl] = fp[f];
            }
        } else if (a == 0) {
            sE[fl] = -1;
            sF[fl] = -1;
            sC[fl] = 0.0;
            if (fp) sO[fl] = 0;
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) sX[idx * DIM + d] = x[d];
        if (g) {
#pragma unroll
            for (int i = 0; i < VDIM; ++i) sG[idx * VDIM + i] = gv[i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < FPB * NQ; idx += BDR_BLOCK) {
        const int fl = idx / NQ, q = idx - fl * NQ;
        const double *X = sX + fl * FN * DIM;
        double t[DIM - 1][DIM], m2;
#pragma unroll
        for (int j = 0; j < DIM - 1; ++j)
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                double v = X[i] * T.dN[0][q][j];
#pragma unroll
                for (int c = 1; c < FN; ++c) v = v + X[c * DIM + i] * T.dN[c][q][j];
                t[j][i] = v;
            }
        double n[DIM];
        if constexpr (DIM == 2) {
            m2 = t[0][0] * t[0][0] + t[0][1] * t[0][1];
            n[0] = t[0][1];
            n[1] = -t[0][0];
        } else {
            n[0] = t[0][1] * t[DIM - 2][2] - t[0][2] * t[DIM - 2][1];
            n[1] = t[0][2] * t[DIM - 2][0] - t[0][0] * t[DIM - 2][2];
            n[2] = t[0][0] * t[DIM - 2][1] - t[0][1] * t[DIM - 2][0];
            m2 = (n[0] * n[0] + n[1] * n[1]) + n[DIM - 1] * n[DIM - 1];
        }
        const double meas = sqrt(m2);
        if (!(meas > 0.0) && sF[fl] >= 0) atomicMin(bad, sF[fl]);
        double c = sC[fl];
        if constexpr (CQ) c = sF[fl] >= 0 ? coef[sO[fl] + q] : 0.0;
        sS[idx] = (T.w[q] * meas) * c;
        if constexpr (GEOM) {
#pragma unroll
            for (int i = 0; i < DIM; ++i) sNrm[idx * DIM + i] = n[i] / meas;
        }
    }
    __syncthreads();
}

// The face mass, added to the matrices in out (nullptr: the checks only).  After stage and point:
//   entry   one lane per (face, node pair a <= b of the face): the whole sum over the points, in ascending order, lives in the
//           lane and is added to the element's entries (a, b) and (b, a) of every component in global memory
// The body serves bdr_mass_kernel (fp nullptr: coef one double per face) and, at the face points, saamge_amd_boundary_mass_points
// (coef one double per POINT, point q of face f at fp[f] + q).
template <int DIM, int FN, int VDIM, bool CQ>
__device__ __forceinline__ void bdr_mass_body(int count, const int *__restrict__ list, const BdrFace &F, int nd,
                                              const int *__restrict__ eI, const int *__restrict__ eJ, const roff_t *__restrict__ moff,
                                              const int *__restrict__ face_elem, const double *__restrict__ coords,
                                              const double *__restrict__ coef, const roff_t *__restrict__ fp, double *out,
                                              int *__restrict__ bad) {
    constexpr int FPB = bdr_fpb(FN), NQ = BdrTable<DIM, FN>::NQ, NPAIR = FN * (FN + 1) / 2;
    const BdrTable<DIM, FN> &T = bdr_rule_table<DIM, FN>();
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sS[FPB * NQ];
    __shared__ roff_t sO[CQ ? FPB : 1];
    __shared__ int sE[FPB];
    bdr_stage_points<DIM, FN, VDIM, FPB, CQ>(count, list, F, nd, eI, eJ, face_elem, coords, coef, nullptr, sX, nullptr, sS, sE, bad, fp,
                                             sO);
    if (!out) return;                             // (the same in every lane of the grid)
    const int S = nd * VDIM;
    for (int idx = threadIdx.x; idx < FPB * NPAIR; idx += BDR_BLOCK) {
        const int fl = idx / NPAIR, ab = MASS_PAIRS<FN>.ab[idx - fl * NPAIR], a = ab >> 5, b = ab & 31;
        const int e = sE[fl];
        if (e < 0) continue;
        const double *s = sS + fl * NQ;
        double acc = 0.0;
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) {
            const double term = s[q] * (T.N[q][a] * T.N[q][b]);
            acc = acc + term;
        }
        double *m = out + (moff ? moff[e] : (roff_t)e * S * S);
        const int na = F.node[a], nb = F.node[b];
#pragma unroll
        for (int i = 0; i < VDIM; ++i) {
            const long r = VDIM * na + i, c = VDIM * nb + i;
            m[r * S + c] = m[r * S + c] + acc;
            if (a != b) m[c * S + r] = m[c * S + r] + acc;
        }
    }
}
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_mass_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                             const roff_t *__restrict__ moff, const int *__restrict__ face_elem,
                                                             const double *__restrict__ coords, const double *__restrict__ coef,
                                                             double *out, int *__restrict__ bad) {
    bdr_mass_body<DIM, FN, VDIM, false>(count, list, F, nd, eI, eJ, moff, face_elem, coords, coef, nullptr, out, bad);
}
// coefq: one coefficient per point, point q of face f at fp[f] + q
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_mass_q_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                               const int *__restrict__ eI, const int *__restrict__ eJ,
                                                               const roff_t *__restrict__ moff, const int *__restrict__ face_elem,
                                                               const double *__restrict__ coords, const double *__restrict__ coefq,
                                                               const roff_t *__restrict__ fp, double *out, int *__restrict__ bad) {
    bdr_mass_body<DIM, FN, VDIM, true>(count, list, F, nd, eI, eJ, moff, face_elem, coords, coefq, fp, out, bad);
}

// The face loads of the nodal g (NV x VDIM), added to the vectors in out (nullptr: the checks only).  After stage and point:
//   source  one lane per (face, point, component): gq = sum over the face nodes, ascending, of N_c * g_c; s * gq is kept
//   dof     one lane per (face, face node, component): the whole sum over the points of (s * gq) * N_a, added to the element's
//           vector at the dof of the node in global memory
// The body serves bdr_load_kernel (GQ false) and, at the face points, saamge_amd_boundary_loads_points (GQ true: g holds the data
// AT THE POINTS, row fp[f] + q for point q of face f, read where bdr_load_kernel interpolates the nodal data).
template <int DIM, int FN, int VDIM, bool GQ>
__device__ __forceinline__ void bdr_load_body(int count, const int *__restrict__ list, const BdrFace &F, int nd,
                                              const int *__restrict__ eI, const int *__restrict__ eJ, const int *__restrict__ face_elem,
                                              const double *__restrict__ coords, const double *__restrict__ coef,
                                              const double *__restrict__ g, const roff_t *__restrict__ fp, double *out,
                                              int *__restrict__ bad) {
    constexpr int FPB = bdr_fpb(FN), NQ = BdrTable<DIM, FN>::NQ;
    const BdrTable<DIM, FN> &T = bdr_rule_table<DIM, FN>();
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sG[GQ ? 1 : FPB * FN * VDIM];
    __shared__ double sS[FPB * NQ];
    __shared__ double sQ[FPB * NQ * VDIM];
    __shared__ roff_t sO[GQ ? FPB : 1];
    __shared__ int sE[FPB];
    bdr_stage_points<DIM, FN, VDIM, FPB>(count, list, F, nd, eI, eJ, face_elem, coords, coef, GQ ? nullptr : g, sX, sG, sS, sE, bad, fp,
                                         sO);
    if (!out) return;                             // (the same in every lane of the grid)
    const int tid = threadIdx.x;
    for (int idx = tid; idx < FPB * NQ * VDIM; idx += BDR_BLOCK) {
        const int fl = idx / (NQ * VDIM), r = idx - fl * (NQ * VDIM), q = r / VDIM, i = r - q * VDIM;
        double gq;
        if constexpr (GQ) {
            gq = sE[fl] < 0 ? 0.0 : g[sO[fl] * VDIM + r];
        } else {
            const double *G = sG + fl * FN * VDIM + i;
            gq = T.N[q][0] * G[0];
            for (int c = 1; c < FN; ++c) gq = gq + T.N[q][c] * G[c * VDIM];
        }
        sQ[idx] = sS[fl * NQ + q] * gq;
    }
    __syncthreads();
    for (int idx = tid; idx < FPB * FN * VDIM; idx += BDR_BLOCK) {
        const int fl = idx / (FN * VDIM), r = idx - fl * (FN * VDIM), a = r / VDIM, i = r - a * VDIM;
        const int e = sE[fl];
        if (e < 0) continue;
        const double *Q = sQ + fl * NQ * VDIM + i;
        double acc = 0.0;
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) {
            const double term = Q[q * VDIM] * T.N[q][a];
            acc = acc + term;
        }
        const long vb = eI ? (long)eI[e] : (long)e * nd;
        double *v = out + (vb + F.node[a]) * VDIM + i;
        *v = *v + acc;
    }
}
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_load_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                             const int *__restrict__ face_elem, const double *__restrict__ coords,
                                                             const double *__restrict__ coef, const double *__restrict__ g,
                                                             double *out, int *__restrict__ bad) {
    bdr_load_body<DIM, FN, VDIM, false>(count, list, F, nd, eI, eJ, face_elem, coords, coef, g, nullptr, out, bad);
}
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_load_q_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                               const int *__restrict__ eI, const int *__restrict__ eJ,
                                                               const int *__restrict__ face_elem, const double *__restrict__ coords,
                                                               const double *__restrict__ coef, const double *__restrict__ gq,
                                                               const roff_t *__restrict__ fp, double *out, int *__restrict__ bad) {
    bdr_load_body<DIM, FN, VDIM, true>(count, list, F, nd, eI, eJ, face_elem, coords, coef, gq, fp, out, bad);
}

// ---- boundary data at the face points ---------------------------------------------------------------------------------------------
// elmat_model.py's boundary_points / boundary_eval (boundary_mass_points and boundary_loads_points: the bodies above).  Point q of
// face f OF THE LIST has the global index fp[f] + q (fp: NF + 1 offsets, 64 bits), whatever bucket the face is worked in: the
// kernels place what they write through fp[f] of the face's index in the list.
// The points of the faces: xq (NFQ x DIM), wmeas (NFQ), normal (NFQ x DIM); any may be nullptr.  After stage and point, one lane
// per (face, point, coordinate): consecutive lanes store consecutive doubles of a face's rows.
template <int DIM, int FN>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_points_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                               const int *__restrict__ eI, const int *__restrict__ eJ,
                                                               const int *__restrict__ face_elem, const double *__restrict__ coords,
                                                               const roff_t *__restrict__ fp, double *__restrict__ xq,
                                                               double *__restrict__ wmeas, double *__restrict__ normal,
                                                               int *__restrict__ bad) {
    constexpr int FPB = bdr_fpb(FN), NQ = BdrTable<DIM, FN>::NQ;
    const BdrTable<DIM, FN> &T = bdr_rule_table<DIM, FN>();
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sS[FPB * NQ];
    __shared__ double sNrm[FPB * NQ * DIM];
    __shared__ roff_t sO[FPB];
    __shared__ int sE[FPB];
    bdr_stage_points<DIM, FN, 1, FPB, false, true>(count, list, F, nd, eI, eJ, face_elem, coords, nullptr, nullptr, sX, nullptr, sS, sE,
                                                   bad, fp, sO, sNrm);      // (the coefficient is 1.0: s = weight * meas)
    for (int idx = threadIdx.x; idx < FPB * NQ * DIM; idx += BDR_BLOCK) {
        const int fl = idx / (NQ * DIM), r = idx - fl * (NQ * DIM), q = r / DIM, i = r - q * DIM;
        if (sE[fl] < 0) continue;
        const roff_t at = sO[fl] * DIM + r;
        if (normal) normal[at] = sNrm[idx];
        if (wmeas && i == 0) wmeas[sO[fl] + q] = sS[fl * NQ + q];
        if (xq) {
            const double *X = sX + fl * FN * DIM + i;
            double x = T.N[q][0] * X[0];
            for (int c = 1; c < FN; ++c) x = x + T.N[q][c] * X[c * DIM];
            xq[at] = x;
        }
    }
}

// the element's gradients at the points of its local faces (FaceGradTable, elmat_ref.h): the largest, the 27-node hexahedron's,
// has 6 x 27 x 9 x 3 doubles (35 KB).  The objects live in global memory like the tables of the rules; a launch works one local
// face, whose block (at most 5.8 KB) the workgroup copies to LDS: the lanes of the J phase read it at addresses that differ from
// lane to lane, as mass_point_phases reads sD.
template <int DIM, int ND>
__device__ const FaceGradTable<DIM, ND> FACE_GRAD_TABLE = face_grad_table<DIM, ND>();
// faces per workgroup: bdr_fpb's, except where an element of 10 or more nodes per face would take the LDS past 32 KB
constexpr int bdr_eval_fpb(int nd, int fn) { return nd >= 10 && fn != 9 ? 16 : bdr_fpb(fn); }

// The nodal u (NV x VDIM) at the face points: uq (NFQ x VDIM), the trace through the face's own shape functions (gq of
// bdr_load_kernel), and gradq (NFQ x VDIM x DIM), the whole gradient of the owning element's field; either may be nullptr.
// Templated on the ELEMENT type <DIM, ND> and on the face type FN; lf: the local face of this launch.  Phases:
//   element the coordinates and u of ALL ND nodes of the owning element and the block of the face's gradients into LDS
//   stage, point   bdr_stage_points: the face's nodes (with u), the measures (not positive: the face to *bad)
//   J       one lane per (face, point): J[i][j] = sum over the element's nodes, ascending, of x_a[i] * dN_a[j], the cofactors and
//           det (not positive: the face's index in the list to *bad_det) to sP, as mass_point_phases keeps them
//   value   one lane per (face, point, component): uq and, as qp_value forms it, r[k] = sum over the nodes of u_a * dN_a[k],
//           g[j] = (r . C[j]) / det
template <int DIM, int ND, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_eval_kernel(int count, const int *__restrict__ list, const BdrFace F, int lf,
                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                             const int *__restrict__ face_elem, const double *__restrict__ coords,
                                                             const double *__restrict__ u, const roff_t *__restrict__ fp,
                                                             double *__restrict__ uq, double *__restrict__ gradq,
                                                             int *__restrict__ bad, int *__restrict__ bad_det) {
    constexpr int FPB = bdr_eval_fpb(ND, FN), NQ = BdrTable<DIM, FN>::NQ, MQ = FaceGradTable<DIM, ND>::MAXQ, DD = DIM * DIM, PW = DD + 1;
    const BdrTable<DIM, FN> &T = bdr_rule_table<DIM, FN>();
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sG[FPB * FN * VDIM];
    __shared__ double sS[FPB * NQ];
    __shared__ double sXe[FPB * ND * DIM];
    __shared__ double sUe[FPB * ND * VDIM];
    __shared__ double sD[ND * MQ * DIM];
    __shared__ double sP[FPB * NQ * PW];
    __shared__ roff_t sO[FPB];
    __shared__ int sE[FPB];
    const int tid = threadIdx.x;
    // ---- element (the barriers of bdr_stage_points cover it)
    for (int idx = tid; idx < FPB * ND; idx += BDR_BLOCK) {
        const int fl = idx / ND, a = idx - fl * ND;
        const long slot = (long)blockIdx.x * FPB + fl;
        double x[DIM], uv[VDIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) x[d] = 0.0;
#pragma unroll
        for (int i = 0; i < VDIM; ++i) uv[i] = 0.0;
        if (slot < count) {
            const int e = face_elem[list[slot]];
            const long vb = eI ? (long)eI[e] : (long)e * ND;
            const int v = eJ[vb + a];
#pragma unroll
            for (int d = 0; d < DIM; ++d) x[d] = coords[(long)v * DIM + d];
#pragma unroll
            for (int i = 0; i < VDIM; ++i) uv[i] = u[(long)v * VDIM + i];
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) sXe[idx * DIM + d] = x[d];
#pragma unroll
        for (int i = 0; i < VDIM; ++i) sUe[idx * VDIM + i] = uv[i];
    }
    const double *D = &FACE_GRAD_TABLE<DIM, ND>.dN[lf][0][0][0];
    for (int idx = tid; idx < ND * MQ * DIM; idx += BDR_BLOCK) sD[idx] = D[idx];
    bdr_stage_points<DIM, FN, VDIM, FPB>(count, list, F, ND, eI, eJ, face_elem, coords, nullptr, u, sX, sG, sS, sE, bad, fp, sO);
    // ---- J
    for (int idx = tid; idx < FPB * NQ; idx += BDR_BLOCK) {
        const int fl = idx / NQ, q = idx - fl * NQ;
        const double *X = sXe + fl * ND * DIM, *Dq = sD + q * DIM;
        double J[DIM][DIM], C[DIM][DIM], det;
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
            for (int j = 0; j < DIM; ++j) {
                double t = X[i] * Dq[j];
                for (int a = 1; a < ND; ++a) t = t + X[a * DIM + i] * Dq[a * MQ * DIM + j];
                J[i][j] = t;
            }
        em_cofactors<DIM>(J, C, det);
        if (!(det > 0.0) && sE[fl] >= 0) atomicMin(bad_det, list[(long)blockIdx.x * FPB + fl]);
        double *P = sP + idx * PW;
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
            for (int j = 0; j < DIM; ++j) P[i * DIM + j] = C[i][j];
        P[DD] = det;
    }
    if (!uq && !gradq) return;                    // (the same in every lane of the grid)
    __syncthreads();
    // ---- value
    for (int idx = tid; idx < FPB * NQ * VDIM; idx += BDR_BLOCK) {
        const int fl = idx / (NQ * VDIM), r = idx - fl * (NQ * VDIM), q = r / VDIM, i = r - q * VDIM;
        if (sE[fl] < 0) continue;
        const roff_t at = sO[fl] * VDIM + r;
        if (uq) {
            const double *G = sG + fl * FN * VDIM + i;
            double v = T.N[q][0] * G[0];
            for (int c = 1; c < FN; ++c) v = v + T.N[q][c] * G[c * VDIM];
            uq[at] = v;
        }
        if (gradq) {
            const double *U = sUe + fl * ND * VDIM + i, *Dq = sD + q * DIM, *P = sP + (fl * NQ + q) * PW;
            double rr[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) rr[k] = U[0] * Dq[k];
            for (int a = 1; a < ND; ++a) {
                const double f = U[a * VDIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) rr[k] = rr[k] + f * Dq[a * MQ * DIM + k];
            }
            const double det = P[DD];
#pragma unroll
            for (int j = 0; j < DIM; ++j) {
                double t = rr[0] * P[j * DIM + 0] + rr[1] * P[j * DIM + 1];
                if constexpr (DIM == 3) t = t + rr[2] * P[j * DIM + 2];
                gradq[at * DIM + j] = t / det;
            }
        }
    }
}

// ---- tables ---------------------------------------------------------------------------------------------------------------
// type of every element (-1: none, and the smallest such element in *first) and the size of its matrix
__global__ __launch_bounds__(256) void em_classify_kernel(int NE, int dim, int comp, const int *__restrict__ eI,
                                                          int *__restrict__ cls, int *__restrict__ sq, int *__restrict__ first) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int nd = eI[e + 1] - eI[e], t = em_type_index(dim, nd);
    cls[e] = t;
    sq[e] = t < 0 ? 0 : nd * comp * nd * comp;
    if (t < 0) atomicMin(first, (int)e);
}
__global__ __launch_bounds__(256) void em_dof_ptr_kernel(int NE, int comp, const int *__restrict__ eI, int *__restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e <= NE) out[e] = comp * eI[e];
}
__global__ __launch_bounds__(256) void em_dofs_kernel(long nconn, int comp, const int *__restrict__ eJ, int *__restrict__ out) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= nconn) return;
    for (int c = 0; c < comp; ++c) out[k * comp + c] = comp * eJ[k] + c;
}

// ---- the launches ---------------------------------------------------------------------------------------------------------------
// what the kernels of every family are launched with; EmFrame fills it
struct EmLaunch {
    hipStream_t s;
    const int *eI, *eJ;
    const roff_t *moff;
    const double *coords, *coef;
    int ncoef;
    double *out;
    int *bad;
    const roff_t *qoff;      // the offsets of the points: coef then holds a row per POINT (emkq_kernel, mass_kq_kernel)
};
// one launch on the stream, the launch error checked
template <class... P, class... A>
void em_run(void (*kernel)(P...), hipStream_t s, int blocks, int threads, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), 0, s, args...);
    SA_HIP_CHECK(hipGetLastError());
}

// the stiffness forms of `count` elements of one type: order 1 em_kernel, order 2 em2_kernel, rows per point emkq_kernel
template <int KIND>
void em_launch_type(const EmLaunch &L, int type, int count, const int *list) {
    with_elem_type(type, [&](auto tag) {
        constexpr int DIM = decltype(tag)::DIM, ND = decltype(tag)::ND;
        if (L.qoff) {
            typedef EmKqCfg<DIM, ND, KIND> Cfg;
            em_run(emkq_kernel<DIM, ND, KIND>, L.s, div_up(count, Cfg::EPB), Cfg::BLOCK, count, list, L.eI, L.eJ, L.moff, L.qoff, L.coords,
                   L.coef, L.ncoef, L.out, L.bad);
        } else if constexpr (em_order1(DIM, ND)) {
            constexpr int BLOCK = em_block(DIM, ND, KIND);
            em_run(em_kernel<DIM, ND, KIND>, L.s, div_up(count, BLOCK / ND), BLOCK, count, list, L.eI, L.eJ, L.moff, L.coords, L.coef,
                   L.ncoef, L.out, L.bad);
        } else {
            typedef Em2Cfg<DIM, ND, KIND> Cfg;
            em_run(em2_kernel<DIM, ND, KIND>, L.s, div_up(count, Cfg::EPB), Cfg::BLOCK, count, list, L.eI, L.eJ, L.moff, L.coords, L.coef,
                   L.ncoef, L.out, L.bad);
        }
    });
}
// src nullptr: the mass matrices (L.qoff: with a coefficient per point), else the load vectors
void mass_launch_type(const EmLaunch &L, int type, int vdim, int accumulate, const double *src, int count, const int *list) {
    with_elem_type(type, [&](auto tag) {
        with_vdim(tag, vdim, [&](auto t, auto vd) {
            constexpr int DIM = decltype(t)::DIM, ND = decltype(t)::ND, VDIM = decltype(vd)::value;
            if (src)
                em_run(load_kernel<DIM, ND, VDIM>, L.s, div_up(count, load_epb(ND)), MASS_BLOCK, count, list, L.eI, L.eJ, L.coords, L.coef,
                       src, L.out, L.bad);
            else if (L.qoff)
                em_run(mass_kq_kernel<DIM, ND, VDIM>, L.s, div_up(count, mass_epb(ND, VDIM)), MASS_BLOCK, count, list, L.eI, L.eJ, L.moff,
                       L.qoff, L.coords, L.coef, accumulate, L.out, L.bad);
            else
                em_run(mass_kernel<DIM, ND, VDIM>, L.s, div_up(count, mass_epb(ND, VDIM)), MASS_BLOCK, count, list, L.eI, L.eJ, L.moff,
                       L.coords, L.coef, accumulate, L.out, L.bad);
        });
    });
}

// the calls on data at the points: what they launch with beyond EmLaunch (its coef: of QP_LOADS; its out: the vectors of QP_LOADS)
enum QpCall { QP_POINTS, QP_EVAL, QP_LOADS, QP_ERRORS };
struct QpLaunch {
    const roff_t *qoff;
    const double *in;         // u (QP_EVAL, QP_ERRORS) or fq (QP_LOADS)
    const double *exq, *exgradq;
    double *a, *b;            // xq, wdet / uq, gradq / -, - / err, -
};
void qp_launch_type(QpCall call, const EmLaunch &L, const QpLaunch &Q, int type, int vdim, int count, const int *list) {
    with_elem_type(type, [&](auto tag) {
        with_vdim(tag, vdim, [&](auto t, auto vd) {
            constexpr int DIM = decltype(t)::DIM, ND = decltype(t)::ND, VDIM = decltype(vd)::value;
            const int blocks = div_up(count, call == QP_LOADS ? load_epb(ND) : qp_epb(ND));
            if (call == QP_POINTS)
                em_run(qp_points_kernel<DIM, ND>, L.s, blocks, MASS_BLOCK, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.a, Q.b, L.bad);
            else if (call == QP_EVAL)
                em_run(qp_eval_kernel<DIM, ND, VDIM>, L.s, blocks, MASS_BLOCK, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.in, Q.a, Q.b,
                       L.bad);
            else if (call == QP_LOADS)
                em_run(qp_load_kernel<DIM, ND, VDIM>, L.s, blocks, MASS_BLOCK, count, list, L.eI, L.eJ, Q.qoff, L.coords, L.coef, Q.in,
                       L.out, L.bad);
            else
                em_run(qp_error_kernel<DIM, ND, VDIM>, L.s, blocks, MASS_BLOCK, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.in, Q.exq,
                       Q.exgradq, Q.a, L.bad);
        });
    });
}

// the calls on a face list: what they launch with beyond EmLaunch (its coef: per face, or per point for BDR_MASS with fp; its out:
// the matrices / vectors of BDR_MASS / BDR_LOADS)
enum BdrCall { BDR_MASS, BDR_LOADS, BDR_POINTS, BDR_EVAL };
struct BdrLaunch {
    const int *face_elem;
    const double *in;         // g at the nodes, or with fp at the points (BDR_LOADS); u (BDR_EVAL)
    const roff_t *fp;         // the offsets of the faces' points; nullptr: the forms with data per face / at the nodes
    double *a, *b, *c;        // xq, wmeas, normal / uq, gradq, -
    int *bad_det;             // BDR_EVAL: the first face whose element has a non-positive determinant at a face point
};
// the call on the faces `list` of elements of type `type` (em_type_index) with the local face index lf
void bdr_launch_face(BdrCall call, const EmLaunch &L, const BdrLaunch &B, int dim, int vdim, int type, int lf, int count,
                     const int *list) {
    const BdrFace F = bdr_face(type, lf);
    const int nd = EM_TYPE_ND[type], fn = BDR_FACE_NODES[type][lf];
    bool found = false;
    if (call == BDR_EVAL) {      // templated on the element type too
        with_elem_type(type, [&](auto etag) {
            with_face_nodes(etag, fn, [&](auto fc) {
                with_vdim(etag, vdim, [&](auto t, auto vd) {
                    constexpr int DIM = decltype(t)::DIM, ND = decltype(t)::ND, FN = decltype(fc)::value, VDIM = decltype(vd)::value;
                    em_run(bdr_eval_kernel<DIM, ND, FN, VDIM>, L.s, div_up(count, bdr_eval_fpb(ND, FN)), BDR_BLOCK, count, list, F, lf, L.eI,
                           L.eJ, B.face_elem, L.coords, B.in, B.fp, B.a, B.b, L.bad, B.bad_det);
                    found = true;
                });
            });
        });
        SA_REQUIRE(found, "boundary forms: no such face type");
        return;
    }
    found = with_face_type(dim, fn, [&](auto tag) {
        with_vdim(tag, vdim, [&](auto t, auto vd) {
            constexpr int DIM = decltype(t)::DIM, FN = decltype(t)::ND, VDIM = decltype(vd)::value;
            const int blocks = div_up(count, bdr_fpb(FN));
            if (call == BDR_POINTS)
                em_run(bdr_points_kernel<DIM, FN>, L.s, blocks, BDR_BLOCK, count, list, F, nd, L.eI, L.eJ, B.face_elem, L.coords, B.fp, B.a,
                       B.b, B.c, L.bad);
            else if (call == BDR_LOADS && B.fp)
                em_run(bdr_load_q_kernel<DIM, FN, VDIM>, L.s, blocks, BDR_BLOCK, count, list, F, nd, L.eI, L.eJ, B.face_elem, L.coords,
                       L.coef, B.in, B.fp, L.out, L.bad);
            else if (call == BDR_LOADS)
                em_run(bdr_load_kernel<DIM, FN, VDIM>, L.s, blocks, BDR_BLOCK, count, list, F, nd, L.eI, L.eJ, B.face_elem, L.coords, L.coef,
                       B.in, L.out, L.bad);
            else if (B.fp)
                em_run(bdr_mass_q_kernel<DIM, FN, VDIM>, L.s, blocks, BDR_BLOCK, count, list, F, nd, L.eI, L.eJ, L.moff, B.face_elem,
                       L.coords, L.coef, B.fp, L.out, L.bad);
            else
                em_run(bdr_mass_kernel<DIM, FN, VDIM>, L.s, blocks, BDR_BLOCK, count, list, F, nd, L.eI, L.eJ, L.moff, B.face_elem, L.coords,
                       L.coef, L.out, L.bad);
        });
    });
    SA_REQUIRE(found, "boundary forms: no such face type");
}

// ---- what the entry points share ------------------------------------------------------------------------------------------
// (the checks that need no device: mesh_begin, then the call's own, then mesh_check_sizes -- mesh.h)

// the mesh on the device, checked; the elements of every type; square: the offsets of the packed matrices
struct EmMesh : DeviceMesh {
    DBuf<int> list[EM_TYPES], word;
    DBuf<roff_t> moff;
    int count[EM_TYPES] = {};
    int64_t doubles = 0;          // of the packed result: sum of size^2 (square) or of size
};
void em_mesh(hipStream_t s, const std::string &name, const MeshArgs &m, int comp, bool square, EmMesh &M, long long info[8]) {
    const int dim = m.dim, NE = m.NE, nde = m.nde;
    import_mesh(s, name, m, M);
    SA_REQUIRE((int64_t)M.nconn * comp <= INT_MAX, name + "dim * elem_ptr[NE] beyond 32 bits");
    // ---- types, lists, offsets of the packed matrices
    M.word.alloc(1);
    if (m.elem_ptr) {
        DBuf<int> sq((size_t)NE), cls((size_t)NE), flag, pos;
        SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s));
        em_run(em_classify_kernel, s, div_up(NE, 256), 256, NE, dim, comp, M.eI, cls.p, sq.p, M.word.p);
        const int first = read_one(M.word.p, s);
        if (first < NE) refuse_element_type(s, name, dim, M.eI, first);
        flag.alloc((size_t)NE);
        pos.alloc((size_t)NE + 1);
        for (int t = 0; t < EM_TYPES; ++t)
            if (em_type_index(dim, EM_TYPE_ND[t]) == t) M.count[t] = make_list(s, NE, cls.p, t, flag, pos, M.list[t]);
        if (square) {
            M.moff.alloc((size_t)NE + 1);
            exclusive_scan_off(s, NE, sq.p, M.moff.p);
            M.doubles = read_one(M.moff.p + NE, s);
        } else {
            M.doubles = (int64_t)M.nconn * comp;
        }
    } else {
        M.count[em_type_index(dim, nde)] = NE;
        M.doubles = square ? (int64_t)NE * (nde * comp) * (nde * comp) : (int64_t)NE * nde * comp;
    }
    if (info) {
        for (int t = 0; t < 5; ++t) info[t] = M.count[t];
        info[5] = (long long)M.doubles;
        info[7] = (long long)M.count[5] + M.count[6] + M.count[7] + M.count[8];      // the order-2 elements
    }
}

// ---- the offsets of the points of the mass rule ------------------------------------------------------------------------------
// the number of points of every element (its type has been checked)
__global__ __launch_bounds__(256) void qp_count_kernel(int NE, int dim, const int *__restrict__ eI, int *__restrict__ cnt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < NE) cnt[e] = mass_points(dim, eI[e + 1] - eI[e]);
}
__global__ __launch_bounds__(256) void qp_offsets_kernel(int NE, int nq, roff_t *__restrict__ qoff) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e <= NE) qoff[e] = (roff_t)e * nq;
}
// qoff: the NE + 1 offsets on the device; returns NQ
int64_t qp_offsets(hipStream_t s, const MeshArgs &m, const EmMesh &M, DBuf<roff_t> &qoff) {
    const int NE = m.NE;
    qoff.alloc((size_t)NE + 1);
    if (m.elem_ptr) {
        DBuf<int> cnt((size_t)NE);
        em_run(qp_count_kernel, s, div_up(NE, 256), 256, NE, m.dim, M.eI, cnt.p);
        exclusive_scan_off(s, NE, cnt.p, qoff.p);
        return read_one(qoff.p + NE, s);
    }
    const int nq = mass_points(m.dim, m.nde);
    em_run(qp_offsets_kernel, s, div_up((int64_t)NE + 1, 256), 256, NE, nq, qoff.p);
    return (int64_t)NE * nq;
}

// ---- the frame of a call ----------------------------------------------------------------------------------------------------------
// What every driver does around its launches, in the order the stream sees it: open (the mesh, checked), points (the offsets of
// the points, where the call has any), inputs (the launch arguments: device views of the coordinates and the coefficients),
// target / out[] (outputs, host or device), run (the bad word reset, the types looped, the first bad element refused), then
// copy_home and sync.  A refusal writes no output: the kernels of a call that refuses have written to the frame's buffers at most.
struct EmFrame {
    const hipStream_t s;
    const std::string &name;
    const MeshArgs &m;
    long long *const info;
    EmMesh M;
    EmLaunch L{};
    DBuf<roff_t> qoff;
    DevIn<double> in_X, in_c;
    DevOut<double> out[2];      // [0]: what L.out writes, or the first output of a call on data at the points

    EmFrame(hipStream_t s_, const std::string &name_, const MeshArgs &m_, long long *info_) : s(s_), name(name_), m(m_), info(info_) {}
    // comp: dofs per node; square: the results are packed matrices; mesh_info: info[0 .. 5] and info[7] as em_mesh fills them
    void open(int comp, bool square, bool mesh_info = true) { em_mesh(s, name, m, comp, square, M, mesh_info ? info : nullptr); }
    // returns NQ; rows: the coefficients of this call come one row per point
    int64_t points(bool rows) {
        const int64_t NQ = qp_offsets(s, m, M, qoff);
        coef_rows = rows;
        return NQ;
    }
    // coef: n doubles in rows of ncoef, nullptr: none
    void inputs(const double *coef = nullptr, size_t n = 0, int ncoef = 1) {
        L = EmLaunch{s, m.elem_ptr ? M.eI : nullptr, M.eJ, M.moff.p, in_X.bind(m.coords, (size_t)m.NV * m.dim, s), nullptr,
                     ncoef, nullptr, M.word.p, coef_rows ? qoff.p : nullptr};
        coefficients(coef, n);
    }
    void coefficients(const double *coef, size_t n) { L.coef = in_c.bind(coef, n, s); }
    void target(double *p, size_t n, bool load = false) { L.out = out[0].bind(p, n, s, load); }
    void reset_bad() { SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s)); }
    // f(type, count, list) for the elements of every type the mesh has
    template <class F>
    void for_types(F &&f) {
        for (int t = 0; t < EM_TYPES; ++t)
            if (M.count[t]) f(t, M.count[t], (const int *)M.list[t].p);
    }
    // the integer minimum the kernels left in the bad word: the first element (face) of `limit` that is refused
    void refuse_bad(int limit, const char *noun, const char *what, const int *word = nullptr) {
        const int bad = read_one(word ? word : (const int *)M.word.p, s);
        if (bad < limit) {
            if (info) info[6] = bad;
            SA_REQUIRE(false, name + noun + std::to_string(bad) + what);
        }
    }
    template <class F>
    void run(F &&f) {
        reset_bad();
        for_types(f);
        refuse_bad(m.NE, "element ", ": the Jacobian determinant is not positive");
    }
    void copy_home() {
        out[0].finish();
        out[1].finish();
    }
    void sync() { SA_HIP_CHECK(hipStreamSynchronize(s)); }

  private:
    bool coef_rows = false;
};

// ---- the drivers ------------------------------------------------------------------------------------------------------------------
// saamge_amd_element_matrices and, at_points, saamge_amd_element_matrices_points: coef then holds a row per point of the mass rule
void stiffness(hipStream_t s, const std::string &name, bool at_points, const MeshArgs &m, int kind, int ncoef, const double *coef,
               double *elmat_out, int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    const int dim = m.dim, NE = m.NE;
    // ---- what needs no device
    mesh_begin(name, m, info);
    SA_REQUIRE(kind == 0 || kind == 1, name + "kind must be 0 (diffusion) or 1 (elasticity)");
    if (kind == 1)
        SA_REQUIRE(ncoef == 2, name + "ncoef must be 2 (lambda, mu) for elasticity");
    else
        SA_REQUIRE(ncoef == 1 || ncoef == dim || ncoef == dim * (dim + 1) / 2,
                   name + "ncoef must be 1, dim or dim (dim + 1) / 2 for diffusion");
    SA_REQUIRE(NE == 0 || (m.coords && m.elem_to_vertex && coef),
               name + "null argument: coords, elem_to_vertex or " + (at_points ? "coefq" : "coef"));
    const int comp = kind ? dim : 1;
    mesh_check_sizes(name, m, comp, false);
    if (NE == 0) return;
    // ---- the matrices (elmat_out NULL: the determinants are still checked)
    EmFrame F(s, name, m, info);
    F.open(comp, true);
    const size_t rows = at_points ? (size_t)F.points(true) : (size_t)NE;
    F.inputs(coef, rows * ncoef, ncoef);
    F.target(elmat_out, (size_t)F.M.doubles);
    F.run([&](int t, int count, const int *list) {
        if (kind) em_launch_type<1>(F.L, t, count, list);
        else em_launch_type<0>(F.L, t, count, list);
    });
    F.copy_home();
    // ---- the dof lists the matrices are indexed by
    const long nconn = F.M.nconn;
    DBuf<int> dptr, dofs;
    if (dof_ptr_out) {
        dptr.alloc((size_t)NE + 1);
        em_run(em_dof_ptr_kernel, s, div_up((int64_t)NE + 1, 256), 256, NE, comp, F.M.eI, dptr.p);
        copy_to_caller(dof_ptr_out, dptr, s);
    }
    if (elem_to_dof_out) {
        dofs.alloc((size_t)nconn * comp);
        em_run(em_dofs_kernel, s, std::max(1, div_up(nconn, 256)), 256, nconn, comp, F.M.eJ, dofs.p);
        copy_to_caller(elem_to_dof_out, dofs, s);
    }
    F.sync();
}

// the mass matrices (src nullptr) or the load vectors of the arguments of saamge_amd_element_mass / _loads, already checked;
// at_points (saamge_amd_element_mass_points): coef holds one double per point of the mass rule
void mass_or_loads(hipStream_t s, const std::string &name, const MeshArgs &m, int vdim, const double *coef, const double *src,
                   int accumulate, double *out, long long info[8], bool at_points = false) {
    if (m.NE == 0) return;
    EmFrame F(s, name, m, info);
    F.open(vdim, !src);
    F.inputs(coef, at_points ? (size_t)F.points(true) : (size_t)m.NE);
    F.target(out, (size_t)F.M.doubles, accumulate);
    const DevIn<double> in_src(src, (size_t)m.NV * vdim, s);
    const double *dsrc = in_src.p;
    F.run([&](int t, int count, const int *list) { mass_launch_type(F.L, t, vdim, accumulate, dsrc, count, list); });
    F.copy_home();
    F.sync();
}
// saamge_amd_element_mass and, at_points, saamge_amd_element_mass_points (coef_name: what the C ABI calls the coefficients)
void mass_entry(hipStream_t s, const std::string &name, bool at_points, const char *coef_name, const MeshArgs &m, int vdim,
                const double *coef, int accumulate, double *elmat_inout, long long info[8]) {
    mesh_begin(name, m, info);
    SA_REQUIRE(vdim == 1 || vdim == m.dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(m.NE == 0 || coef, name + "null argument: " + coef_name);
    SA_REQUIRE(m.NE == 0 || (m.coords && m.elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    SA_REQUIRE(!accumulate || elmat_inout, name + "null argument: accumulate needs the matrices in elmat_inout");
    mesh_check_sizes(name, m, vdim, false);
    mass_or_loads(s, name, m, vdim, coef, nullptr, accumulate ? 1 : 0, elmat_inout, info, at_points);
}

// The four calls on data at the points, the arguments the C ABI names.  A refusal writes no output: the determinants of the
// whole mesh are checked (mass_kernel without an output) before the first kernel that writes.
void points_call(QpCall call, hipStream_t s, const std::string &name, const MeshArgs &m, int vdim, const double *coef,
                 const double *in, const char *in_name, const double *exq, const double *exgradq, long long *qp_ptr_out, double *out_a,
                 double *out_b, long long info[8]) {
    const int dim = m.dim, NE = m.NE;
    mesh_begin(name, m, info);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NE == 0 || (m.coords && m.elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    mesh_check_sizes(name, m, vdim, false);
    EmFrame F(s, name, m, info);
    if (NE) F.open(vdim, false);
    if (info) info[5] = 0;
    SA_REQUIRE(call == QP_POINTS || in, name + "null argument: " + in_name);
    if (NE == 0) {
        const long long zero = 0;
        copy_to_caller(qp_ptr_out, &zero, 1, s);
        F.sync();
        return;
    }
    const size_t nq = (size_t)F.points(false);
    if (info) info[5] = (long long)nq;
    // ---- the determinants, before anything is written
    F.inputs();
    F.run([&](int t, int count, const int *list) { mass_launch_type(F.L, t, 1, 0, nullptr, count, list); });
    // ---- the call
    const DevIn<double> in_in(in, call == QP_LOADS ? nq * vdim : (size_t)m.NV * vdim, s), in_e(exq, nq * vdim, s),
        in_g(exgradq, nq * vdim * dim, s);
    double *a = nullptr, *b = nullptr;
    if (call == QP_POINTS) {
        a = F.out[0].bind(out_a, nq * dim, s, false);
        b = F.out[1].bind(out_b, nq, s, false);
    } else if (call == QP_EVAL) {
        a = F.out[0].bind(out_a, nq * vdim, s, false);
        b = F.out[1].bind(out_b, nq * vdim * dim, s, false);
    } else if (call == QP_LOADS) {
        F.coefficients(coef, (size_t)NE);
        F.target(out_a, (size_t)F.M.doubles);
    } else {
        a = F.out[0].bind(out_a, (size_t)NE * 2, s, false);
    }
    const QpLaunch Q{F.qoff.p, in_in.p, in_e.p, in_g.p, a, b};
    if (a || b || F.L.out) F.for_types([&](int t, int count, const int *list) { qp_launch_type(call, F.L, Q, t, vdim, count, list); });
    F.copy_home();
    copy_to_caller((roff_t *)qp_ptr_out, (const roff_t *)F.qoff.p, (size_t)NE + 1, s);
    F.sync();
}

// ---- the offsets of the points of a face list ---------------------------------------------------------------------------------------
// the points of the rule of local face lf of element type t, by the key t * 8 + lf that bdr_check_kernel gives every face
struct BdrPointCounts {
    unsigned char n[EM_TYPES * 8];
};
constexpr BdrPointCounts bdr_point_counts() {
    BdrPointCounts c{};
    for (int t = 0; t < EM_TYPES; ++t)
        for (int lf = 0; lf < bdr_num_faces(t); ++lf)
            c.n[t * 8 + lf] = (unsigned char)face_points(em_type_dim(t), BDR_FACE_NODES[t][lf]);
    return c;
}
__device__ const BdrPointCounts BDR_POINT_COUNTS = bdr_point_counts();
__global__ __launch_bounds__(256) void bdr_point_count_kernel(int NF, const int *__restrict__ key, int *__restrict__ cnt) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f < NF) cnt[f] = BDR_POINT_COUNTS.n[key[f]];      // (the list has been checked: no key is negative)
}
// fp: the NF + 1 offsets on the device, in the order of the list; returns NFQ
int64_t bdr_offsets(hipStream_t s, int NF, const int *key, DBuf<roff_t> &fp) {
    DBuf<int> cnt((size_t)NF);
    fp.alloc((size_t)NF + 1);
    em_run(bdr_point_count_kernel, s, div_up(NF, 256), 256, NF, key, cnt.p);
    exclusive_scan_off(s, NF, cnt.p, fp.p);
    return read_one(fp.p + NF, s);
}

// The calls on a face list, their arguments already checked.  BDR_MASS / BDR_LOADS with at_points false: saamge_amd_boundary_mass
// / _loads (coef per face, `in` the nodal g; out_a the matrices / vectors added to).  at_points: the four calls on data at the face
// points -- BDR_MASS: coef per POINT; BDR_LOADS: `in` the data at the points; BDR_POINTS: fp_out, out_a / _b / _c = xq, wmeas,
// normal; BDR_EVAL: `in` the nodal u, out_a / _b = uq, gradq.  These four refuse before they write: a pass of their kernels without
// outputs checks every measure (and determinant) first.
void boundary_forms(BdrCall call, bool at_points, hipStream_t s, const std::string &name, const MeshArgs &m, int NF,
                    const int *face_elem, const int *face_local, int vdim, const double *coef, const double *in, long long *fp_out,
                    double *out_a, double *out_b, double *out_c, long long info[8]) {
    const int dim = m.dim, NE = m.NE;
    if (NF == 0) {
        if (fp_out) {      // (the one offset of an empty list; without it an empty list touches no device)
            const long long zero = 0;
            copy_to_caller(fp_out, &zero, 1, s);
        }
        return;
    }
    if (NE == 0 && info) info[6] = 0;
    SA_REQUIRE(NE > 0, name + "face 0: face_elem is outside [0, NE)");
    EmFrame F(s, name, m, info);
    F.open(vdim, call == BDR_MASS, false);
    // ---- the face list: ranges, repeated pairs, the key of every face
    FaceList FL;
    check_face_list(s, name, dim, NE, F.M.eI, NF, face_elem, face_local, FL, info ? info + 6 : nullptr);
    DBuf<int> flag((size_t)NF), pos((size_t)NF + 1);
    // ---- one list per (element type, local face)
    DBuf<int> list[EM_TYPES][BDR_MAX_FACES];
    int count[EM_TYPES][BDR_MAX_FACES] = {};
    int64_t doubles = 0;
    F.for_types([&](int t, int, const int *) {
        for (int lf = 0; lf < bdr_num_faces(t); ++lf) {
            const int c = count[t][lf] = make_list(s, NF, FL.key.p, t * 8 + lf, flag, pos, list[t][lf]);
            const int fn = BDR_FACE_NODES[t][lf];
            if (info) info[bdr_face_type(dim, fn)] += c;
            doubles += (int64_t)c * (call == BDR_MASS ? fn * fn * vdim : fn * vdim);
        }
    });
    // ---- the offsets of the points, in the order of the LIST
    DBuf<roff_t> fp;
    const size_t nfq = at_points ? (size_t)bdr_offsets(s, NF, FL.key.p, fp) : 0;
    if (info) {
        info[5] = call == BDR_POINTS || call == BDR_EVAL ? (long long)nfq : (long long)doubles;
        info[7] = FL.touched;
    }
    // ---- the passes: ascending local face, so that the faces of one element are added in that order
    F.inputs(coef, call == BDR_MASS && at_points ? nfq : (size_t)NF);
    const DevIn<double> in_in(in, call == BDR_LOADS && at_points ? nfq * vdim : (size_t)m.NV * vdim, s);
    DBuf<int> bad_det;
    if (call == BDR_EVAL) {
        bad_det.alloc(1);
        SA_HIP_CHECK(hipMemsetAsync(bad_det.p, 0x7f, sizeof(int), s));
    }
    BdrLaunch B{FL.fe, in_in.p, fp.p, nullptr, nullptr, nullptr, bad_det.p};
    auto passes = [&] {
        for (int lf = 0; lf < BDR_MAX_FACES; ++lf)
            for (int t = 0; t < EM_TYPES; ++t)
                if (count[t][lf]) bdr_launch_face(call, F.L, B, dim, vdim, t, lf, count[t][lf], list[t][lf].p);
    };
    auto refuse = [&] {
        F.refuse_bad(NF, "face ", ": the measure is not positive");
        if (call == BDR_EVAL) F.refuse_bad(NF, "face ", ": the Jacobian determinant of the element is not positive", bad_det.p);
    };
    F.reset_bad();
    DevOut<double> third;
    bool write = true;
    if (at_points) {      // nothing is written before every face has passed
        passes();
        refuse();
        write = out_a || out_b || out_c;
    }
    if (call == BDR_MASS || call == BDR_LOADS) {
        F.target(out_a, (size_t)F.M.doubles, true);
    } else {
        B.a = F.out[0].bind(out_a, nfq * (call == BDR_POINTS ? dim : vdim), s, false);
        B.b = F.out[1].bind(out_b, call == BDR_POINTS ? nfq : nfq * vdim * dim, s, false);
        B.c = third.bind(out_c, nfq * dim, s, false);
    }
    if (write) passes();
    if (!at_points) refuse();
    F.copy_home();
    third.finish();
    copy_to_caller((roff_t *)fp_out, (const roff_t *)fp.p, (size_t)NF + 1, s);
    F.sync();
}
// the checks of both entry points that need no device
void bdr_begin(const std::string &name, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim,
               long long info[8]) {
    mesh_begin(name, m, info);
    SA_REQUIRE(NF >= 0, name + "NF < 0");
    SA_REQUIRE(vdim == 1 || vdim == m.dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NF == 0 || (face_elem && face_local), name + "null argument: face_elem or face_local");
    SA_REQUIRE(NF == 0 || m.NE == 0 || (m.coords && m.elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    mesh_check_sizes(name, m, vdim, false);
}
}  // namespace

// ---- the entry points (elmat.h) -----------------------------------------------------------------------------------------------
void element_matrices(hipStream_t s, const MeshArgs &m, int kind, int ncoef, const double *coef, double *elmat_out, int *dof_ptr_out,
                      int *elem_to_dof_out, long long info[8]) {
    stiffness(s, "saamge_amd_element_matrices: ", false, m, kind, ncoef, coef, elmat_out, dof_ptr_out, elem_to_dof_out, info);
}
void element_matrices_points(hipStream_t s, const MeshArgs &m, int kind, int ncoef, const double *coefq, double *elmat_out,
                             int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    stiffness(s, "saamge_amd_element_matrices_points: ", true, m, kind, ncoef, coefq, elmat_out, dof_ptr_out, elem_to_dof_out, info);
}

void element_mass(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, int accumulate, double *elmat_inout,
                  long long info[8]) {
    mass_entry(s, "saamge_amd_element_mass: ", false, "coef", m, vdim, coef, accumulate, elmat_inout, info);
}
void element_mass_points(hipStream_t s, const MeshArgs &m, int vdim, const double *coefq, int accumulate, double *elmat_inout,
                         long long info[8]) {
    mass_entry(s, "saamge_amd_element_mass_points: ", true, "coefq", m, vdim, coefq, accumulate, elmat_inout, info);
}

void element_loads(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, const double *src, double *elvec_out,
                   long long info[8]) {
    const std::string name("saamge_amd_element_loads: ");
    mesh_begin(name, m, info);
    SA_REQUIRE(vdim == 1 || vdim == m.dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(src, name + "null argument: src");
    SA_REQUIRE(m.NE == 0 || (m.coords && m.elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    mesh_check_sizes(name, m, vdim, false);
    mass_or_loads(s, name, m, vdim, coef, src, 0, elvec_out, info);
}

void boundary_mass(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                   double *elmat_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_mass: ");
    bdr_begin(name, m, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(NF == 0 || coef, name + "null argument: coef");
    boundary_forms(BDR_MASS, false, s, name, m, NF, face_elem, face_local, vdim, coef, nullptr, nullptr, elmat_inout, nullptr, nullptr,
                   info);
}
void boundary_loads(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                    const double *g, double *elvec_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_loads: ");
    bdr_begin(name, m, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(g, name + "null argument: g");
    boundary_forms(BDR_LOADS, false, s, name, m, NF, face_elem, face_local, vdim, coef, g, nullptr, elvec_inout, nullptr, nullptr, info);
}

void boundary_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, long long *fp_ptr_out,
                     double *xq_out, double *wmeas_out, double *normal_out, long long info[8]) {
    const std::string name("saamge_amd_boundary_points: ");
    bdr_begin(name, m, NF, face_elem, face_local, 1, info);
    boundary_forms(BDR_POINTS, true, s, name, m, NF, face_elem, face_local, 1, nullptr, nullptr, fp_ptr_out, xq_out, wmeas_out,
                   normal_out, info);
}
void boundary_eval(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, const double *u,
                   double *uq_out, double *gradq_out, long long info[8]) {
    const std::string name("saamge_amd_boundary_eval: ");
    bdr_begin(name, m, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(u, name + "null argument: u");
    boundary_forms(BDR_EVAL, true, s, name, m, NF, face_elem, face_local, vdim, nullptr, u, nullptr, uq_out, gradq_out, nullptr, info);
}
void boundary_mass_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim,
                          const double *coefq, double *elmat_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_mass_points: ");
    bdr_begin(name, m, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(NF == 0 || coefq, name + "null argument: coefq");
    boundary_forms(BDR_MASS, true, s, name, m, NF, face_elem, face_local, vdim, coefq, nullptr, nullptr, elmat_inout, nullptr, nullptr,
                   info);
}
void boundary_loads_points(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim,
                           const double *coef, const double *gq, double *elvec_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_loads_points: ");
    bdr_begin(name, m, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(NF == 0 || gq, name + "null argument: gq");
    boundary_forms(BDR_LOADS, true, s, name, m, NF, face_elem, face_local, vdim, coef, gq, nullptr, elvec_inout, nullptr, nullptr, info);
}

void element_points(hipStream_t s, const MeshArgs &m, long long *qp_ptr_out, double *xq_out, double *wdet_out, long long info[8]) {
    points_call(QP_POINTS, s, "saamge_amd_element_points: ", m, 1, nullptr, nullptr, "", nullptr, nullptr, qp_ptr_out, xq_out, wdet_out,
                info);
}
void element_eval(hipStream_t s, const MeshArgs &m, int vdim, const double *u, double *uq_out, double *gradq_out, long long info[8]) {
    points_call(QP_EVAL, s, "saamge_amd_element_eval: ", m, vdim, nullptr, u, "u", nullptr, nullptr, nullptr, uq_out, gradq_out, info);
}
void element_loads_points(hipStream_t s, const MeshArgs &m, int vdim, const double *coef, const double *fq, double *elvec_out,
                          long long info[8]) {
    points_call(QP_LOADS, s, "saamge_amd_element_loads_points: ", m, vdim, coef, fq, "fq", nullptr, nullptr, nullptr, elvec_out, nullptr,
                info);
}
void element_errors(hipStream_t s, const MeshArgs &m, int vdim, const double *u, const double *exq, const double *exgradq,
                    double *err_out, long long info[8]) {
    points_call(QP_ERRORS, s, "saamge_amd_element_errors: ", m, vdim, nullptr, u, "u", exq, exgradq, nullptr, err_out, nullptr, info);
}

}  // namespace saamge_amd
