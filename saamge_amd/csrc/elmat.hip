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
#include "elmat.h"
#include "elmat_types.h"

#include <algorithm>
#include <climits>
#include <utility>
#include <vector>

#include "operator.h"
#include "partition.h"

// every rounding of the model is one IEEE operation: no product is fused with the sum that follows it, anywhere in this file
#pragma clang fp contract(off)

namespace saamge_amd {

namespace {

// ---- the rules: the literals of elmat_model.py --------------------------------------------------------------------------
constexpr double EM_GAUSS[2] = {0.21132486540518713, 0.7886751345948129};
constexpr double EM_TRI_A = 0.16666666666666666, EM_TRI_B = 0.6666666666666666;
constexpr int EM_QUAD_LOC[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
constexpr double EM_TRI_D[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
constexpr double EM_TET_D[4][3] = {{-1.0, -1.0, -1.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
constexpr double EM_WEDGE_TRI[3][2] = {{EM_TRI_A, EM_TRI_A}, {EM_TRI_B, EM_TRI_A}, {EM_TRI_A, EM_TRI_B}};

// points of the rule, weight of one point
template <int DIM, int ND> struct EmType;
template <> struct EmType<2, 3> { static constexpr int NQ = 1; static constexpr double W = 0.5; };
template <> struct EmType<2, 4> { static constexpr int NQ = 4; static constexpr double W = 0.25; };
template <> struct EmType<3, 4> { static constexpr int NQ = 1; static constexpr double W = 0.16666666666666666; };
template <> struct EmType<3, 6> { static constexpr int NQ = 6; static constexpr double W = 0.08333333333333333; };
template <> struct EmType<3, 8> { static constexpr int NQ = 8; static constexpr double W = 0.125; };

// (the type indices -- EM_TYPES, em_type_index, EM_TYPE_ND -- and the local faces are in elmat_types.h)

constexpr double em_f(int l, double p) { return l ? p : 1.0 - p; }
constexpr double em_df(int l) { return l ? 1.0 : -1.0; }

template <int DIM, int ND>
struct EmGrad {
    double v[ND][DIM];
};
// gradients of the reference shape functions at point q (elmat_model.reference_gradients), folded at compile time
template <int DIM, int ND>
constexpr EmGrad<DIM, ND> em_ref_grad(int q) {
    EmGrad<DIM, ND> g{};
    if constexpr (DIM == 2 && ND == 3) {
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 2; ++j) g.v[a][j] = EM_TRI_D[a][j];
    } else if constexpr (DIM == 3 && ND == 4) {
        for (int a = 0; a < 4; ++a)
            for (int j = 0; j < 3; ++j) g.v[a][j] = EM_TET_D[a][j];
    } else if constexpr (DIM == 2 && ND == 4) {
        const double px = EM_GAUSS[q & 1], py = EM_GAUSS[(q >> 1) & 1];
        for (int a = 0; a < 4; ++a) {
            const int lx = EM_QUAD_LOC[a][0], ly = EM_QUAD_LOC[a][1];
            g.v[a][0] = em_df(lx) * em_f(ly, py);
            g.v[a][1] = em_f(lx, px) * em_df(ly);
        }
    } else if constexpr (DIM == 3 && ND == 8) {
        const double px = EM_GAUSS[q & 1], py = EM_GAUSS[(q >> 1) & 1], pz = EM_GAUSS[(q >> 2) & 1];
        for (int a = 0; a < 8; ++a) {
            const int lx = EM_HEX_LOC[a][0], ly = EM_HEX_LOC[a][1], lz = EM_HEX_LOC[a][2];
            g.v[a][0] = em_df(lx) * (em_f(ly, py) * em_f(lz, pz));
            g.v[a][1] = em_df(ly) * (em_f(lx, px) * em_f(lz, pz));
            g.v[a][2] = em_df(lz) * (em_f(lx, px) * em_f(ly, py));
        }
    } else {
        static_assert(DIM == 3 && ND == 6, "no such element type");
        const double xi = EM_WEDGE_TRI[q % 3][0], eta = EM_WEDGE_TRI[q % 3][1], zeta = EM_GAUSS[q / 3];
        const double T[3] = {(1.0 - xi) - eta, xi, eta};
        const double L[2] = {1.0 - zeta, zeta};
        for (int a = 0; a < 2; ++a)
            for (int i = 0; i < 3; ++i) {
                g.v[a * 3 + i][0] = EM_TRI_D[i][0] * L[a];
                g.v[a * 3 + i][1] = EM_TRI_D[i][1] * L[a];
                g.v[a * 3 + i][2] = T[i] * em_df(a);
            }
    }
    return g;
}

// the rule's table: one set of gradients per point.  The point loop of the kernel is a real loop (unrolled, the compiler forms
// the Jacobians of all points ahead of the first barrier and runs out of registers) that reads its point's line through a
// wave-uniform index.
template <int DIM, int ND>
struct EmTable {
    EmGrad<DIM, ND> p[EmType<DIM, ND>::NQ];
};
template <int DIM, int ND>
constexpr EmTable<DIM, ND> em_table() {
    EmTable<DIM, ND> t{};
    for (int q = 0; q < EmType<DIM, ND>::NQ; ++q) t.p[q] = em_ref_grad<DIM, ND>(q);
    return t;
}
template <int DIM, int ND>
__device__ const EmTable<DIM, ND> EM_TABLE = em_table<DIM, ND>();

// threads per workgroup: 256 where the tile of 256 / nd matrices stays within 40 KB of LDS, else one wavefront
constexpr int em_block(int dim, int nd, int kind) {
    const int size = nd * (kind ? dim : 1);
    return (256 / nd) * size * size * 8 <= 40960 ? 256 : 64;
}

inline dim3 grid_flat(long n) { return dim3((unsigned)std::max<long>(1, (n + 255) / 256)); }

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
    typedef EmType<DIM, ND> T;
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
// The literals and the expressions of elmat_model.py (GAUSS3, GAUSS3_W, _n2, _d2, Q2_QUAD_LOC; the hex is lexicographic).
constexpr double EM2_GAUSS[3] = {0.11270166537925831, 0.5, 0.8872983346207417};
constexpr double EM2_W[3] = {0.2777777777777778, 0.4444444444444444, 0.2777777777777778};
constexpr double em2_n(int l, double p) {
    return l == 0 ? (2.0 * p - 1.0) * (p - 1.0) : (l == 1 ? (4.0 * p) * (1.0 - p) : p * (2.0 * p - 1.0));
}
constexpr double em2_d(int l, double p) { return l == 0 ? 4.0 * p - 3.0 : (l == 1 ? 4.0 - 8.0 * p : 4.0 * p - 1.0); }
constexpr int em2_nodes(int dim) { return dim == 2 ? 9 : 27; }

// The order-2 simplices (elmat_model._p2_simplex): the vertices, then the midpoints of the edges EM_P2_TRI_EDGES / EM_P2_TET_EDGES.  N and dN at the
// reference point pt from the barycentric coordinates L and their constant gradients EM_TRI_D / EM_TET_D.
constexpr int p2s_nodes(int dim) { return dim == 2 ? 6 : 10; }
constexpr bool p2s_type(int dim, int nd) { return nd == p2s_nodes(dim); }
constexpr int EM_P2_TRI_EDGES[3][2] = {{0, 1}, {1, 2}, {2, 0}};
constexpr int EM_P2_TET_EDGES[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
template <int DIM>
struct P2Simplex {
    double N[p2s_nodes(DIM)];
    double dN[p2s_nodes(DIM)][DIM];
};
template <int DIM>
constexpr P2Simplex<DIM> p2_simplex(const double *pt) {
    P2Simplex<DIM> r{};
    double L[4] = {0.0, 0.0, 0.0, 0.0}, D[4][3] = {};
    if (DIM == 2) L[0] = (1.0 - pt[0]) - pt[1];
    else L[0] = ((1.0 - pt[0]) - pt[1]) - pt[DIM - 1];
    for (int k = 0; k < DIM; ++k) L[1 + k] = pt[k];
    for (int i = 0; i <= DIM; ++i)
        for (int k = 0; k < DIM; ++k) D[i][k] = DIM == 2 ? EM_TRI_D[i % 3][k % 2] : EM_TET_D[i][k];
    for (int i = 0; i <= DIM; ++i) {
        r.N[i] = L[i] * (2.0 * L[i] - 1.0);
        for (int k = 0; k < DIM; ++k) r.dN[i][k] = (4.0 * L[i] - 1.0) * D[i][k];
    }
    for (int e = 0; e < p2s_nodes(DIM) - DIM - 1; ++e) {
        const int i = DIM == 2 ? EM_P2_TRI_EDGES[e % 3][0] : EM_P2_TET_EDGES[e][0];
        const int j = DIM == 2 ? EM_P2_TRI_EDGES[e % 3][1] : EM_P2_TET_EDGES[e][1];
        r.N[DIM + 1 + e] = (4.0 * L[i]) * L[j];
        for (int k = 0; k < DIM; ++k) r.dN[DIM + 1 + e][k] = (4.0 * L[i]) * D[j][k] + (4.0 * L[j]) * D[i][k];
    }
    return r;
}
constexpr double EM_TET_A = 0.1381966011250105, EM_TET_B = 0.5854101966249685;
// point q of the stiffness rules of the order-2 simplices: the order-1 mass rules (EM_WEDGE_TRI; EM_TET_A / EM_TET_B)
struct EmPoint {
    double x[3];
};
constexpr EmPoint p2s_point(int dim, int q) {
    if (dim == 2) return EmPoint{{EM_WEDGE_TRI[q % 3][0], EM_WEDGE_TRI[q % 3][1], 0.0}};
    return EmPoint{{q == 1 ? EM_TET_B : EM_TET_A, q == 2 ? EM_TET_B : EM_TET_A, q == 3 ? EM_TET_B : EM_TET_A}};
}

// the rule's table, folded at compile time: the reference gradient of node a at point q (node-major, so that lanes that differ
// in the point read neighbouring doubles) and the weight of point q.  The tensor-product types have as many points as nodes;
// the triangle has 3 and the tetrahedron 4.
constexpr int em2_points(int dim, int nd) { return p2s_type(dim, nd) ? dim + 1 : nd; }
template <int DIM, int ND>
struct Em2Table {
    static constexpr int NQ = em2_points(DIM, ND);
    double dN[ND][em2_points(DIM, ND)][DIM];
    double w[em2_points(DIM, ND)];
};
template <int DIM, int ND>
constexpr Em2Table<DIM, ND> em2_table() {
    Em2Table<DIM, ND> t{};
    if constexpr (p2s_type(DIM, ND)) {
        for (int q = 0; q <= DIM; ++q) {
            const EmPoint pt = p2s_point(DIM, q);
            const P2Simplex<DIM> f = p2_simplex<DIM>(pt.x);
            t.w[q] = DIM == 2 ? 0.16666666666666666 : 0.041666666666666664;
            for (int a = 0; a < ND; ++a)
                for (int j = 0; j < DIM; ++j) t.dN[a][q][j] = f.dN[a][j];
        }
    } else {
        for (int q = 0; q < em2_nodes(DIM); ++q) {
            const int qx = q % 3, qy = (q / 3) % 3, qz = q / 9;
            const double px = EM2_GAUSS[qx], py = EM2_GAUSS[qy], pz = EM2_GAUSS[qz];
            t.w[q] = DIM == 2 ? EM2_W[qx] * EM2_W[qy] : (EM2_W[qx] * EM2_W[qy]) * EM2_W[qz];
            for (int a = 0; a < em2_nodes(DIM); ++a) {
                if (DIM == 2) {
                    const int ix = EM2_QUAD_LOC[a][0], iy = EM2_QUAD_LOC[a][1];
                    t.dN[a][q][0] = em2_d(ix, px) * em2_n(iy, py);
                    t.dN[a][q][1] = em2_n(ix, px) * em2_d(iy, py);
                } else {
                    const int ix = a % 3, iy = (a / 3) % 3, iz = a / 9;
                    t.dN[a][q][0] = em2_d(ix, px) * (em2_n(iy, py) * em2_n(iz, pz));
                    t.dN[a][q][1] = em2_d(iy, py) * (em2_n(ix, px) * em2_n(iz, pz));
                    t.dN[a][q][DIM - 1] = em2_d(iz, pz) * (em2_n(ix, px) * em2_n(iy, py));
                }
            }
        }
    }
    return t;
}
template <int DIM, int ND>
__device__ const Em2Table<DIM, ND> EM2_TABLE = em2_table<DIM, ND>();

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
template <int DIM, int ND, int KIND, class Cfg, class Table, bool KQ>
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
    const long left = (long)count - (long)blockIdx.x * EPB;
    const int total = (int)(left < EPB ? left : EPB) * SS;
    for (int t = tid; t < total; t += BLOCK) {
        const int l = t / SS;
        out[obase[l] + (t - l * SS)] = tile[t];
    }
}

template <int DIM, int ND, int KIND>
__global__ __launch_bounds__((Em2Cfg<DIM, ND, KIND>::BLOCK)) void em2_kernel(int count, const int *__restrict__ list,
                                                                           const int *__restrict__ eI, const int *__restrict__ eJ,
                                                                           const roff_t *__restrict__ moff,
                                                                           const double *__restrict__ coords,
                                                                           const double *__restrict__ coef, int ncoef,
                                                                           double *__restrict__ out, int *__restrict__ bad) {
    em2_body<DIM, ND, KIND, Em2Cfg<DIM, ND, KIND>, Em2Table<DIM, ND>, false>(EM2_TABLE<DIM, ND>, count, list, eI, eJ, moff, nullptr,
                                                                             coords, coef, ncoef, out, bad);
}

// ---- mass matrices and load vectors ------------------------------------------------------------------------------------------
// elmat_model.py's element_mass / element_loads.  The rule of a type is its stiffness rule, except for the simplices: three
// points (EM_WEDGE_TRI, weight 1/6) on the triangle and four (EM_TET_A / EM_TET_B, weight 1/24) on the tetrahedron.  The order-2
// simplices: 6 points (degree 4) on the triangle, 14 (degree 5) on the tetrahedron -- elmat_model's P2_TRI_POINTS / P2_TET_POINTS.
constexpr int mass_points(int dim, int nd) {
    return nd == 9 || nd == 27 ? nd : (dim == 2 ? (nd == 3 ? 3 : (nd == 6 ? 6 : 4)) : (nd == 4 ? 4 : (nd == 10 ? 14 : nd)));
}
constexpr double EM_P2_TRI_A[2] = {0.44594849091596483, 0.09157621350977073};
constexpr double EM_P2_TRI_W[2] = {0.11169079483900572, 0.054975871827660935};
constexpr double EM_P2_TET_A[2] = {0.3108859192633006, 0.09273525031089122};
constexpr double EM_P2_TET_W[3] = {0.018781320953002643, 0.012248840519393659, 0.007091003462846911};
constexpr double EM_P2_TET_EDGE_A = 0.04550370412564965;
// point q of the mass rule of an order-2 simplex and its weight
constexpr EmPoint p2s_mass_point(int dim, int q) {
    if (dim == 2) {
        const double a = EM_P2_TRI_A[q / 3], b = 1.0 - 2.0 * a;
        return EmPoint{{q % 3 == 1 ? b : a, q % 3 == 2 ? b : a, 0.0}};
    }
    if (q < 8) {
        const double a = EM_P2_TET_A[q / 4], b = 1.0 - 3.0 * a;
        return EmPoint{{q % 4 == 1 ? b : a, q % 4 == 2 ? b : a, q % 4 == 3 ? b : a}};
    }
    const double a = EM_P2_TET_EDGE_A, b = 0.5 - a;
    const int i = EM_P2_TET_EDGES[q - 8][0], j = EM_P2_TET_EDGES[q - 8][1];      // barycentrics i and j are b, the point (L1, L2, L3)
    return EmPoint{{i == 1 || j == 1 ? b : a, i == 2 || j == 2 ? b : a, i == 3 || j == 3 ? b : a}};
}
constexpr double p2s_mass_weight(int dim, int q) { return dim == 2 ? EM_P2_TRI_W[q / 3] : EM_P2_TET_W[q < 8 ? q / 4 : 2]; }

// the rule's table, folded at compile time: reference gradients and shape values of node a at point q (dN node-major as in
// Em2Table, N point-major: the entry phase reads N of neighbouring nodes at one point) and the weight of point q
template <int DIM, int ND>
struct MassTable {
    static constexpr int NQ = mass_points(DIM, ND);
    double dN[ND][NQ][DIM];
    double N[NQ][ND];
    double w[NQ];
};
template <int DIM, int ND>
constexpr MassTable<DIM, ND> mass_table() {
    MassTable<DIM, ND> t{};
    constexpr int NQ = MassTable<DIM, ND>::NQ;
    if constexpr (p2s_type(DIM, ND)) {
        for (int q = 0; q < NQ; ++q) {
            const EmPoint pt = p2s_mass_point(DIM, q);
            const P2Simplex<DIM> f = p2_simplex<DIM>(pt.x);
            t.w[q] = p2s_mass_weight(DIM, q);
            for (int a = 0; a < ND; ++a) {
                t.N[q][a] = f.N[a];
                for (int j = 0; j < DIM; ++j) t.dN[a][q][j] = f.dN[a][j];
            }
        }
    } else if constexpr (ND == em2_nodes(DIM)) {
        const Em2Table<DIM, ND> g = em2_table<DIM, ND>();
        for (int q = 0; q < NQ; ++q) {
            const double px = EM2_GAUSS[q % 3], py = EM2_GAUSS[(q / 3) % 3], pz = EM2_GAUSS[q / 9];
            t.w[q] = g.w[q];
            for (int a = 0; a < ND; ++a) {
                for (int j = 0; j < DIM; ++j) t.dN[a][q][j] = g.dN[a][q][j];
                if (DIM == 2)
                    t.N[q][a] = em2_n(EM2_QUAD_LOC[a % 9][0], px) * em2_n(EM2_QUAD_LOC[a % 9][1], py);
                else
                    t.N[q][a] = em2_n(a % 3, px) * (em2_n((a / 3) % 3, py) * em2_n(a / 9, pz));
            }
        }
    } else {
        for (int q = 0; q < NQ; ++q) {
            const EmGrad<DIM, ND> g = em_ref_grad<DIM, ND>(q);     // (the simplices': the same at every point)
            for (int a = 0; a < ND; ++a)
                for (int j = 0; j < DIM; ++j) t.dN[a][q][j] = g.v[a][j];
            t.w[q] = EmType<DIM, ND>::W;
            if constexpr (DIM == 2 && ND == 3) {
                const double x = EM_WEDGE_TRI[q][0], y = EM_WEDGE_TRI[q][1];
                t.w[q] = 0.16666666666666666;
                t.N[q][0] = (1.0 - x) - y;
                t.N[q][1] = x;
                t.N[q][2] = y;
            } else if constexpr (DIM == 3 && ND == 4) {
                const double x = q == 1 ? EM_TET_B : EM_TET_A, y = q == 2 ? EM_TET_B : EM_TET_A, z = q == 3 ? EM_TET_B : EM_TET_A;
                t.w[q] = 0.041666666666666664;
                t.N[q][0] = ((1.0 - x) - y) - z;
                t.N[q][1] = x;
                t.N[q][2] = y;
                t.N[q][3] = z;
            } else if constexpr (DIM == 2 && ND == 4) {
                const double px = EM_GAUSS[q & 1], py = EM_GAUSS[(q >> 1) & 1];
                for (int a = 0; a < 4; ++a) t.N[q][a] = em_f(EM_QUAD_LOC[a][0], px) * em_f(EM_QUAD_LOC[a][1], py);
            } else if constexpr (DIM == 3 && ND == 8) {
                const double px = EM_GAUSS[q & 1], py = EM_GAUSS[(q >> 1) & 1], pz = EM_GAUSS[(q >> 2) & 1];
                for (int a = 0; a < 8; ++a)
                    t.N[q][a] = em_f(EM_HEX_LOC[a][0], px) * (em_f(EM_HEX_LOC[a][1], py) * em_f(EM_HEX_LOC[a][2], pz));
            } else {
                const double xi = EM_WEDGE_TRI[q % 3][0], eta = EM_WEDGE_TRI[q % 3][1], zeta = EM_GAUSS[q / 3];
                const double T[3] = {(1.0 - xi) - eta, xi, eta};
                const double L[2] = {1.0 - zeta, zeta};
                for (int a = 0; a < 2; ++a)
                    for (int i = 0; i < 3; ++i) t.N[q][a * 3 + i] = T[i] * L[a];
            }
        }
    }
    return t;
}
template <int DIM, int ND>
__device__ const MassTable<DIM, ND> MASS_TABLE = mass_table<DIM, ND>();

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
    const long left = (long)count - (long)blockIdx.x * EPB;
    const int total = (int)(left < EPB ? left : EPB) * SS;
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
    for (int t = tid; t < total; t += BLOCK) {
        const int l = t / SS;
        out[obase[l] + (t - l * SS)] = tile[t];
    }
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
    em2_body<DIM, ND, KIND, EmKqCfg<DIM, ND, KIND>, MassTable<DIM, ND>, true>(MASS_TABLE<DIM, ND>, count, list, eI, eJ, moff, qoff,
                                                                              coords, coefq, ncoef, out, bad);
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

// the rule of a face type, folded at compile time from the expressions of mass_table: the segments have their own lines
// (em_f / em_df on the 2 Gauss points, em2_n / em2_d on the 3), a face of DIM 3 is the element type (2, FN)
constexpr int bdr_points(int dim, int fn) { return dim == 2 ? fn : mass_points(2, fn); }
template <int DIM, int FN>
struct BdrTable {
    static constexpr int NQ = bdr_points(DIM, FN);
    double dN[FN][NQ][DIM - 1];
    double N[NQ][FN];
    double w[NQ];
};
template <int DIM, int FN>
constexpr BdrTable<DIM, FN> bdr_table() {
    BdrTable<DIM, FN> t{};
    constexpr int NQ = BdrTable<DIM, FN>::NQ;
    if constexpr (DIM == 3) {
        const MassTable<2, FN> m = mass_table<2, FN>();
        for (int q = 0; q < NQ; ++q) {
            t.w[q] = m.w[q];
            for (int a = 0; a < FN; ++a) {
                t.N[q][a] = m.N[q][a];
                t.dN[a][q][0] = m.dN[a][q][0];
                t.dN[a][q][DIM - 2] = m.dN[a][q][1];
            }
        }
    } else {
        for (int q = 0; q < NQ; ++q) {
            const double p = FN == 2 ? EM_GAUSS[q % 2] : EM2_GAUSS[q];
            t.w[q] = FN == 2 ? 0.5 : EM2_W[q];
            for (int a = 0; a < FN; ++a) {
                t.N[q][a] = FN == 2 ? em_f(a, p) : em2_n(a, p);
                t.dN[a][q][0] = FN == 2 ? em_df(a) : em2_d(a, p);
            }
        }
    }
    return t;
}
template <int DIM, int FN>
__device__ const BdrTable<DIM, FN> BDR_TABLE = bdr_table<DIM, FN>();

constexpr int BDR_BLOCK = 256;
constexpr int bdr_fpb(int fn) { return fn == 9 ? 5 : (fn == 4 ? 16 : 32); }      // faces per workgroup

// The checks of the face list.  Face f with face_elem outside [0, NE) or face_local outside the range of the element's type:
// key[f] = -1 and f to the integer minimum words[0]; else key[f] = type * 8 + local face, and the face's bit is set in the byte
// of its element (mask: one byte per element, four to a word) -- a bit that was already set raises words[1].
__global__ __launch_bounds__(256) void bdr_check_kernel(int NF, int NE, int dim, const int *__restrict__ eI,
                                                        const int *__restrict__ face_elem, const int *__restrict__ face_local,
                                                        unsigned *__restrict__ mask, int *__restrict__ key, int *__restrict__ words) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int e = face_elem[f], lf = face_local[f];
    int k = -1;
    if (e >= 0 && e < NE) {
        const int t = em_type_index(dim, eI[e + 1] - eI[e]);      // (the mesh has been checked: t >= 0)
        if (t >= 0 && lf >= 0 && lf < bdr_num_faces(t)) {
            k = t * 8 + lf;
            const unsigned bit = 1u << (8 * (e & 3) + lf);
            if (atomicOr(mask + (e >> 2), bit) & bit) atomicOr(words + 1, 1);
        }
    }
    key[f] = k;
    if (k < 0) atomicMin(words, (int)f);
}
// the number of elements whose byte of the mask is not zero, added to *count
__global__ __launch_bounds__(256) void bdr_touched_kernel(int nwords, const unsigned *__restrict__ mask, int *__restrict__ count) {
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const unsigned m = mask[w];
    const int n = ((m & 0xffu) != 0) + ((m & 0xff00u) != 0) + ((m & 0xff0000u) != 0) + ((m & 0xff000000u) != 0);
    if (n) atomicAdd(count, n);
}

// Phases of both kernels, a barrier after each:
//   stage   one lane per (face, face node): the node's coordinates (and g) into LDS; the face's element, coefficient, offsets
//   point   one lane per (face, point): the tangents, m2, meas = sqrt(m2) and s = (w * meas) * c in registers; a measure that
//           is not positive sends the face's index in the list to the integer minimum *bad
// list: the faces of this launch (indices into face_elem / coef), all of one element type (nd nodes) and one local face F.
template <int DIM, int FN, int VDIM, int FPB>
__device__ inline void bdr_stage_points(int count, const int *__restrict__ list, const BdrFace &F, int nd, const int *__restrict__ eI,
                                        const int *__restrict__ eJ, const int *__restrict__ face_elem,
                                        const double *__restrict__ coords, const double *__restrict__ coef,
                                        const double *__restrict__ g, double *sX, double *sG, double *sS, int *sE, int *bad) {
    constexpr int NQ = BdrTable<DIM, FN>::NQ;
    const BdrTable<DIM, FN> &T = BDR_TABLE<DIM, FN>;
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
                sC[fl] = coef ? coef[f] : 1.0;
            }
        } else if (a == 0) {
            sE[fl] = -1;
            sF[fl] = -1;
            sC[fl] = 0.0;
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
        if constexpr (DIM == 2) {
            m2 = t[0][0] * t[0][0] + t[0][1] * t[0][1];
        } else {
            const double n0 = t[0][1] * t[DIM - 2][2] - t[0][2] * t[DIM - 2][1];
            const double n1 = t[0][2] * t[DIM - 2][0] - t[0][0] * t[DIM - 2][2];
            const double n2 = t[0][0] * t[DIM - 2][1] - t[0][1] * t[DIM - 2][0];
            m2 = (n0 * n0 + n1 * n1) + n2 * n2;
        }
        const double meas = sqrt(m2);
        if (!(meas > 0.0) && sF[fl] >= 0) atomicMin(bad, sF[fl]);
        sS[idx] = (T.w[q] * meas) * sC[fl];
    }
    __syncthreads();
}

// The face mass, added to the matrices in out (nullptr: the checks only).  After stage and point:
//   entry   one lane per (face, node pair a <= b of the face): the whole sum over the points, in ascending order, lives in the
//           lane and is added to the element's entries (a, b) and (b, a) of every component in global memory
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_mass_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                             const roff_t *__restrict__ moff, const int *__restrict__ face_elem,
                                                             const double *__restrict__ coords, const double *__restrict__ coef,
                                                             double *out, int *__restrict__ bad) {
    constexpr int FPB = bdr_fpb(FN), NQ = BdrTable<DIM, FN>::NQ, NPAIR = FN * (FN + 1) / 2;
    const BdrTable<DIM, FN> &T = BDR_TABLE<DIM, FN>;
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sS[FPB * NQ];
    __shared__ int sE[FPB];
    bdr_stage_points<DIM, FN, VDIM, FPB>(count, list, F, nd, eI, eJ, face_elem, coords, coef, nullptr, sX, nullptr, sS, sE, bad);
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

// The face loads of the nodal g (NV x VDIM), added to the vectors in out (nullptr: the checks only).  After stage and point:
//   source  one lane per (face, point, component): gq = sum over the face nodes, ascending, of N_c * g_c; s * gq is kept
//   dof     one lane per (face, face node, component): the whole sum over the points of (s * gq) * N_a, added to the element's
//           vector at the dof of the node in global memory
template <int DIM, int FN, int VDIM>
__global__ __launch_bounds__(BDR_BLOCK) void bdr_load_kernel(int count, const int *__restrict__ list, const BdrFace F, int nd,
                                                             const int *__restrict__ eI, const int *__restrict__ eJ,
                                                             const int *__restrict__ face_elem, const double *__restrict__ coords,
                                                             const double *__restrict__ coef, const double *__restrict__ g,
                                                             double *out, int *__restrict__ bad) {
    constexpr int FPB = bdr_fpb(FN), NQ = BdrTable<DIM, FN>::NQ;
    const BdrTable<DIM, FN> &T = BDR_TABLE<DIM, FN>;
    __shared__ double sX[FPB * FN * DIM];
    __shared__ double sG[FPB * FN * VDIM];
    __shared__ double sS[FPB * NQ];
    __shared__ double sQ[FPB * NQ * VDIM];
    __shared__ int sE[FPB];
    bdr_stage_points<DIM, FN, VDIM, FPB>(count, list, F, nd, eI, eJ, face_elem, coords, coef, g, sX, sG, sS, sE, bad);
    if (!out) return;                             // (the same in every lane of the grid)
    const int tid = threadIdx.x;
    for (int idx = tid; idx < FPB * NQ * VDIM; idx += BDR_BLOCK) {
        const int fl = idx / (NQ * VDIM), r = idx - fl * (NQ * VDIM), q = r / VDIM, i = r - q * VDIM;
        const double *G = sG + fl * FN * VDIM + i;
        double gq = T.N[q][0] * G[0];
        for (int c = 1; c < FN; ++c) gq = gq + T.N[q][c] * G[c * VDIM];
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

// ---- tables ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void em_offsets_kernel(int NE, int nd, int *__restrict__ eI) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e <= NE) eI[e] = (int)(e * nd);
}
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

struct EmLaunch {
    hipStream_t s;
    const int *eI, *eJ;
    const roff_t *moff;
    const double *coords, *coef;
    int ncoef;
    double *out;
    int *bad;
    const roff_t *qoff = nullptr;      // the offsets of the points: coef then holds a row per POINT (emkq_kernel, mass_kq_kernel)
};

template <int DIM, int ND, int KIND>
void em_launch(const EmLaunch &L, int count, const int *list) {
    constexpr int BLOCK = em_block(DIM, ND, KIND), EPB = BLOCK / ND;
    hipLaunchKernelGGL((em_kernel<DIM, ND, KIND>), dim3((unsigned)div_up(count, EPB)), dim3(BLOCK), 0, L.s, count, list, L.eI, L.eJ,
                       L.moff, L.coords, L.coef, L.ncoef, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
template <int DIM, int ND, int KIND>
void em2_launch(const EmLaunch &L, int count, const int *list) {
    typedef Em2Cfg<DIM, ND, KIND> Cfg;
    hipLaunchKernelGGL((em2_kernel<DIM, ND, KIND>), dim3((unsigned)div_up(count, Cfg::EPB)), dim3(Cfg::BLOCK), 0, L.s, count, list, L.eI,
                       L.eJ, L.moff, L.coords, L.coef, L.ncoef, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
template <int DIM, int ND, int KIND>
void emkq_launch(const EmLaunch &L, int count, const int *list) {
    typedef EmKqCfg<DIM, ND, KIND> Cfg;
    hipLaunchKernelGGL((emkq_kernel<DIM, ND, KIND>), dim3((unsigned)div_up(count, Cfg::EPB)), dim3(Cfg::BLOCK), 0, L.s, count, list, L.eI,
                       L.eJ, L.moff, L.qoff, L.coords, L.coef, L.ncoef, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
template <int KIND>
void emkq_launch_type(const EmLaunch &L, int type, int count, const int *list) {
    switch (type) {
        case 0: emkq_launch<2, 3, KIND>(L, count, list); break;
        case 1: emkq_launch<2, 4, KIND>(L, count, list); break;
        case 2: emkq_launch<3, 4, KIND>(L, count, list); break;
        case 3: emkq_launch<3, 6, KIND>(L, count, list); break;
        case 4: emkq_launch<3, 8, KIND>(L, count, list); break;
        case 5: emkq_launch<2, 9, KIND>(L, count, list); break;
        case 6: emkq_launch<3, 27, KIND>(L, count, list); break;
        case 7: emkq_launch<2, 6, KIND>(L, count, list); break;
        default: emkq_launch<3, 10, KIND>(L, count, list); break;
    }
}
template <int KIND>
void em_launch_type(const EmLaunch &L, int type, int count, const int *list) {
    if (L.qoff) return emkq_launch_type<KIND>(L, type, count, list);
    switch (type) {
        case 0: em_launch<2, 3, KIND>(L, count, list); break;
        case 1: em_launch<2, 4, KIND>(L, count, list); break;
        case 2: em_launch<3, 4, KIND>(L, count, list); break;
        case 3: em_launch<3, 6, KIND>(L, count, list); break;
        case 4: em_launch<3, 8, KIND>(L, count, list); break;
        case 5: em2_launch<2, 9, KIND>(L, count, list); break;
        case 6: em2_launch<3, 27, KIND>(L, count, list); break;
        case 7: em2_launch<2, 6, KIND>(L, count, list); break;
        default: em2_launch<3, 10, KIND>(L, count, list); break;
    }
}

template <int DIM, int ND>
void mass_launch(const EmLaunch &L, int vdim, int accumulate, int count, const int *list) {
    if (L.qoff && vdim == 1)
        hipLaunchKernelGGL((mass_kq_kernel<DIM, ND, 1>), dim3((unsigned)div_up(count, mass_epb(ND, 1))), dim3(MASS_BLOCK), 0, L.s, count,
                           list, L.eI, L.eJ, L.moff, L.qoff, L.coords, L.coef, accumulate, L.out, L.bad);
    else if (L.qoff)
        hipLaunchKernelGGL((mass_kq_kernel<DIM, ND, DIM>), dim3((unsigned)div_up(count, mass_epb(ND, DIM))), dim3(MASS_BLOCK), 0, L.s,
                           count, list, L.eI, L.eJ, L.moff, L.qoff, L.coords, L.coef, accumulate, L.out, L.bad);
    else if (vdim == 1)
        hipLaunchKernelGGL((mass_kernel<DIM, ND, 1>), dim3((unsigned)div_up(count, mass_epb(ND, 1))), dim3(MASS_BLOCK), 0, L.s, count,
                           list, L.eI, L.eJ, L.moff, L.coords, L.coef, accumulate, L.out, L.bad);
    else
        hipLaunchKernelGGL((mass_kernel<DIM, ND, DIM>), dim3((unsigned)div_up(count, mass_epb(ND, DIM))), dim3(MASS_BLOCK), 0, L.s,
                           count, list, L.eI, L.eJ, L.moff, L.coords, L.coef, accumulate, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
template <int DIM, int ND>
void load_launch(const EmLaunch &L, int vdim, const double *src, int count, const int *list) {
    const dim3 grid((unsigned)div_up(count, load_epb(ND)));
    if (vdim == 1)
        hipLaunchKernelGGL((load_kernel<DIM, ND, 1>), grid, dim3(MASS_BLOCK), 0, L.s, count, list, L.eI, L.eJ, L.coords, L.coef, src,
                           L.out, L.bad);
    else
        hipLaunchKernelGGL((load_kernel<DIM, ND, DIM>), grid, dim3(MASS_BLOCK), 0, L.s, count, list, L.eI, L.eJ, L.coords, L.coef,
                           src, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
// src nullptr: the mass matrices, else the load vectors
void mass_launch_type(const EmLaunch &L, int type, int vdim, int accumulate, const double *src, int count, const int *list) {
#define SA_MASS_CASE(T, DIM, ND)                                       \
    case T:                                                            \
        if (src) load_launch<DIM, ND>(L, vdim, src, count, list);      \
        else mass_launch<DIM, ND>(L, vdim, accumulate, count, list);   \
        break;
    switch (type) {
        SA_MASS_CASE(0, 2, 3)
        SA_MASS_CASE(1, 2, 4)
        SA_MASS_CASE(2, 3, 4)
        SA_MASS_CASE(3, 3, 6)
        SA_MASS_CASE(4, 3, 8)
        SA_MASS_CASE(5, 2, 9)
        SA_MASS_CASE(6, 3, 27)
        SA_MASS_CASE(7, 2, 6)
        default: SA_MASS_CASE(8, 3, 10)
    }
#undef SA_MASS_CASE
}

const char *const EM_NAME = "saamge_amd_element_matrices: ";

// ---- what the three entry points share ------------------------------------------------------------------------------------
// the checks that need no device: info as a call without elements leaves it, the dimension and the counts ...
void em_begin(const std::string &name, int NV, int dim, int NE, long long info[8]) {
    if (info) {
        for (int k = 0; k < 8; ++k) info[k] = 0;
        info[6] = -1;
    }
    SA_REQUIRE(dim == 2 || dim == 3, name + "dim must be 2 or 3");
    SA_REQUIRE(NV >= 0 && NE >= 0, name + "NV < 0 or NE < 0");
}
// ... and the sizes; comp: dofs per node
void em_check_sizes(const std::string &name, int NV, int dim, int NE, int nde, const int *elem_ptr, int comp) {
    SA_REQUIRE((int64_t)NV * comp <= INT_MAX, name + "dim * NV beyond 32 bits");
    if (!elem_ptr) {
        SA_REQUIRE(em_type_index(dim, nde) >= 0,
                   name + "nde = " + std::to_string(nde) + " nodes are no supported element type in " + std::to_string(dim) + "D");
        SA_REQUIRE((int64_t)NE * nde * comp <= INT_MAX, name + "NE * nde beyond 32 bits");
    }
}

// the mesh on the device, checked; the elements of every type; square: the offsets of the packed matrices
struct EmMesh : DeviceMesh {
    DBuf<int> list[EM_TYPES], word;
    DBuf<roff_t> moff;
    int count[EM_TYPES] = {};
    int64_t doubles = 0;          // of the packed result: sum of size^2 (square) or of size
};
void em_mesh(hipStream_t s, const std::string &name, int NV, int dim, int NE, int nde, const int *elem_ptr,
             const int *elem_to_vertex, int comp, bool square, EmMesh &M, long long info[8]) {
    import_mesh(s, name, NV, NE, nde, elem_ptr, elem_to_vertex, M);
    SA_REQUIRE((int64_t)M.nconn * comp <= INT_MAX, name + "dim * elem_ptr[NE] beyond 32 bits");
    // ---- types, lists, offsets of the packed matrices
    M.word.alloc(1);
    if (elem_ptr) {
        DBuf<int> sq((size_t)NE), cls((size_t)NE), flag, pos;
        SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s));
        hipLaunchKernelGGL(em_classify_kernel, grid_flat(NE), dim3(256), 0, s, NE, dim, comp, M.eI, cls.p, sq.p, M.word.p);
        SA_HIP_CHECK(hipGetLastError());
        const int first = read_one(M.word.p, s);
        if (first < NE) {
            const int nd = read_one(M.eI + first + 1, s) - read_one(M.eI + first, s);
            SA_REQUIRE(false, name + "element " + std::to_string(first) + ": " + std::to_string(nd) +
                                  " nodes are no supported element type in " + std::to_string(dim) + "D");
        }
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

// the integer minimum the kernels left in M.word: the first element with a non-positive determinant
void em_refuse_bad(hipStream_t s, const std::string &name, const EmMesh &M, int NE, long long info[8]) {
    const int bad = read_one(M.word.p, s);
    if (bad < NE) {
        if (info) info[6] = bad;
        SA_REQUIRE(false, name + "element " + std::to_string(bad) + ": the Jacobian determinant is not positive");
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
int64_t qp_offsets(hipStream_t s, int dim, int NE, int nde, const int *elem_ptr, const EmMesh &M, DBuf<roff_t> &qoff) {
    qoff.alloc((size_t)NE + 1);
    if (elem_ptr) {
        DBuf<int> cnt((size_t)NE);
        hipLaunchKernelGGL(qp_count_kernel, grid_flat(NE), dim3(256), 0, s, NE, dim, M.eI, cnt.p);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_off(s, NE, cnt.p, qoff.p);
        return read_one(qoff.p + NE, s);
    }
    const int nq = mass_points(dim, nde);
    hipLaunchKernelGGL(qp_offsets_kernel, grid_flat((long)NE + 1), dim3(256), 0, s, NE, nq, qoff.p);
    SA_HIP_CHECK(hipGetLastError());
    return (int64_t)NE * nq;
}

// the mass matrices (src nullptr) or the load vectors of the arguments of saamge_amd_element_mass / _loads, already checked;
// at_points (saamge_amd_element_mass_points): coef holds one double per point of the mass rule
void mass_or_loads(hipStream_t s, const std::string &name, int NV, int dim, const double *coords, int NE, int nde,
                   const int *elem_ptr, const int *elem_to_vertex, int vdim, const double *coef, const double *src, int accumulate,
                   double *out, long long info[8], bool at_points = false) {
    if (NE == 0) return;
    EmMesh M;
    em_mesh(s, name, NV, dim, NE, nde, elem_ptr, elem_to_vertex, vdim, !src, M, info);
    DBuf<double> hold_X, hold_c, hold_src, hold_out;
    DBuf<roff_t> qoff;
    const size_t ncoef = at_points ? (size_t)qp_offsets(s, dim, NE, nde, elem_ptr, M, qoff) : (size_t)NE;
    EmLaunch L;
    L.qoff = qoff.p;
    L.s = s;
    L.eI = elem_ptr ? M.eI : nullptr;
    L.eJ = M.eJ;
    L.moff = M.moff.p;
    L.coords = device_view(hold_X, coords, (size_t)NV * dim, s);
    L.coef = coef ? device_view(hold_c, coef, ncoef, s) : nullptr;
    L.ncoef = 1;
    L.out = out;
    if (out && !is_device_ptr(out)) {
        if (accumulate) upload(hold_out, (const double *)out, (size_t)M.doubles, s);
        else hold_out.alloc((size_t)M.doubles);
        L.out = hold_out.p;
    }
    L.bad = M.word.p;
    const double *dsrc = src ? device_view(hold_src, src, (size_t)NV * vdim, s) : nullptr;
    SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s));
    for (int t = 0; t < EM_TYPES; ++t)
        if (M.count[t]) mass_launch_type(L, t, vdim, accumulate, dsrc, M.count[t], M.list[t].p);
    em_refuse_bad(s, name, M, NE, info);
    if (hold_out.p) SA_HIP_CHECK(hipMemcpyAsync(out, hold_out.p, (size_t)M.doubles * sizeof(double), hipMemcpyDeviceToHost, s));
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- data at the points of the mass rule --------------------------------------------------------------------------------------

enum QpCall { QP_POINTS, QP_EVAL, QP_LOADS, QP_ERRORS };
struct QpLaunch {
    EmLaunch L;               // (coef: of QP_LOADS; out: its vectors)
    const roff_t *qoff;
    const double *in;         // u (QP_EVAL, QP_ERRORS) or fq (QP_LOADS)
    const double *exq, *exgradq;
    double *a, *b;            // xq, wdet / uq, gradq / -, - / err, -
};
template <int DIM, int ND, int VDIM>
void qp_launch(QpCall call, const QpLaunch &Q, int count, const int *list) {
    const EmLaunch &L = Q.L;
    const dim3 grid((unsigned)div_up(count, call == QP_LOADS ? load_epb(ND) : qp_epb(ND))), block(MASS_BLOCK);
    if (call == QP_POINTS)
        hipLaunchKernelGGL((qp_points_kernel<DIM, ND>), grid, block, 0, L.s, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.a, Q.b, L.bad);
    else if (call == QP_EVAL)
        hipLaunchKernelGGL((qp_eval_kernel<DIM, ND, VDIM>), grid, block, 0, L.s, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.in, Q.a,
                           Q.b, L.bad);
    else if (call == QP_LOADS)
        hipLaunchKernelGGL((qp_load_kernel<DIM, ND, VDIM>), grid, block, 0, L.s, count, list, L.eI, L.eJ, Q.qoff, L.coords, L.coef, Q.in,
                           L.out, L.bad);
    else
        hipLaunchKernelGGL((qp_error_kernel<DIM, ND, VDIM>), grid, block, 0, L.s, count, list, L.eI, L.eJ, Q.qoff, L.coords, Q.in, Q.exq,
                           Q.exgradq, Q.a, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
void qp_launch_type(QpCall call, const QpLaunch &Q, int type, int vdim, int count, const int *list) {
#define SA_QP_CASE(T, DIM, ND)                                                  \
    case T:                                                                     \
        if (vdim == 1) qp_launch<DIM, ND, 1>(call, Q, count, list);             \
        else qp_launch<DIM, ND, DIM>(call, Q, count, list);                     \
        break;
    switch (type) {
        SA_QP_CASE(0, 2, 3)
        SA_QP_CASE(1, 2, 4)
        SA_QP_CASE(2, 3, 4)
        SA_QP_CASE(3, 3, 6)
        SA_QP_CASE(4, 3, 8)
        SA_QP_CASE(5, 2, 9)
        SA_QP_CASE(6, 3, 27)
        SA_QP_CASE(7, 2, 6)
        default: SA_QP_CASE(8, 3, 10)
    }
#undef SA_QP_CASE
}

// an output of `n` doubles that may be a host pointer: the kernels write to dev(), finish() copies it home
struct QpOut {
    double *user = nullptr;
    DBuf<double> hold;
    size_t n = 0;
    double *dev(double *p, size_t count) {
        user = p;
        n = count;
        if (!p || is_device_ptr(p)) return p;
        hold.alloc(count);
        return hold.p;
    }
    void finish(hipStream_t s) {
        if (hold.p && n) SA_HIP_CHECK(hipMemcpyAsync(user, hold.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    }
};

// The four calls on data at the points, the arguments the C ABI names.  A refusal writes no output: the determinants of the
// whole mesh are checked (mass_kernel without an output) before the first kernel that writes.
void points_call(QpCall call, hipStream_t s, const std::string &name, int NV, int dim, const double *coords, int NE, int nde,
                 const int *elem_ptr, const int *elem_to_vertex, int vdim, const double *coef, const double *in, const char *in_name,
                 const double *exq, const double *exgradq, long long *qp_ptr_out, double *out_a, double *out_b, long long info[8]) {
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NE == 0 || (coords && elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, vdim);
    EmMesh M;
    if (NE) em_mesh(s, name, NV, dim, NE, nde, elem_ptr, elem_to_vertex, vdim, false, M, info);
    if (info) info[5] = 0;
    SA_REQUIRE(call == QP_POINTS || in, name + "null argument: " + in_name);
    if (NE == 0) {
        const long long zero = 0;
        if (qp_ptr_out) SA_HIP_CHECK(hipMemcpyAsync(qp_ptr_out, &zero, sizeof(zero), hipMemcpyDefault, s));
        SA_HIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    // ---- the offsets of the points
    DBuf<roff_t> qoff;
    const int64_t NQ = qp_offsets(s, dim, NE, nde, elem_ptr, M, qoff);
    if (info) info[5] = (long long)NQ;
    // ---- the determinants, before anything is written
    DBuf<double> hold_X, hold_c, hold_in, hold_e, hold_g;
    QpLaunch Q;
    EmLaunch &L = Q.L;
    L.s = s;
    L.eI = elem_ptr ? M.eI : nullptr;
    L.eJ = M.eJ;
    L.moff = nullptr;
    L.coords = device_view(hold_X, coords, (size_t)NV * dim, s);
    L.coef = nullptr;
    L.ncoef = 1;
    L.out = nullptr;
    L.bad = M.word.p;
    SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s));
    for (int t = 0; t < EM_TYPES; ++t)
        if (M.count[t]) mass_launch_type(L, t, 1, 0, nullptr, M.count[t], M.list[t].p);
    em_refuse_bad(s, name, M, NE, info);
    // ---- the call
    QpOut oa, ob;
    const size_t nq = (size_t)NQ;
    Q.qoff = qoff.p;
    Q.in = in ? device_view(hold_in, in, call == QP_LOADS ? nq * vdim : (size_t)NV * vdim, s) : nullptr;
    Q.exq = exq ? device_view(hold_e, exq, nq * vdim, s) : nullptr;
    Q.exgradq = exgradq ? device_view(hold_g, exgradq, nq * vdim * dim, s) : nullptr;
    Q.a = Q.b = nullptr;
    if (call == QP_POINTS) {
        Q.a = oa.dev(out_a, nq * dim);
        Q.b = ob.dev(out_b, nq);
    } else if (call == QP_EVAL) {
        Q.a = oa.dev(out_a, nq * vdim);
        Q.b = ob.dev(out_b, nq * vdim * dim);
    } else if (call == QP_LOADS) {
        L.coef = coef ? device_view(hold_c, coef, (size_t)NE, s) : nullptr;
        L.out = oa.dev(out_a, (size_t)M.doubles);
    } else {
        Q.a = oa.dev(out_a, (size_t)NE * 2);
    }
    if (Q.a || Q.b || L.out) {
        for (int t = 0; t < EM_TYPES; ++t)
            if (M.count[t]) qp_launch_type(call, Q, t, vdim, M.count[t], M.list[t].p);
    }
    oa.finish(s);
    ob.finish(s);
    if (qp_ptr_out) SA_HIP_CHECK(hipMemcpyAsync(qp_ptr_out, qoff.p, ((size_t)NE + 1) * sizeof(roff_t), hipMemcpyDefault, s));
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- boundary forms ---------------------------------------------------------------------------------------------------------
struct BdrLaunch {
    hipStream_t s;
    const int *eI, *eJ, *face_elem;
    const roff_t *moff;
    const double *coords, *coef, *g;
    double *out;
    int *bad;
};
template <int DIM, int FN, int VDIM>
void bdr_launch(const BdrLaunch &L, const BdrFace &F, int nd, int count, const int *list) {
    const dim3 grid((unsigned)div_up(count, bdr_fpb(FN)));
    if (L.g)
        hipLaunchKernelGGL((bdr_load_kernel<DIM, FN, VDIM>), grid, dim3(BDR_BLOCK), 0, L.s, count, list, F, nd, L.eI, L.eJ, L.face_elem,
                           L.coords, L.coef, L.g, L.out, L.bad);
    else
        hipLaunchKernelGGL((bdr_mass_kernel<DIM, FN, VDIM>), grid, dim3(BDR_BLOCK), 0, L.s, count, list, F, nd, L.eI, L.eJ, L.moff,
                           L.face_elem, L.coords, L.coef, L.out, L.bad);
    SA_HIP_CHECK(hipGetLastError());
}
// the faces `list` of elements of type `type` (em_type_index) with the local face index lf
void bdr_launch_face(const BdrLaunch &L, int dim, int vdim, int type, int lf, int count, const int *list) {
    const BdrFace F = bdr_face(type, lf);
    const int nd = EM_TYPE_ND[type], fn = BDR_FACE_NODES[type][lf];
#define SA_BDR_CASE(DIM, FN)                                            \
    if (dim == DIM && fn == FN) {                                       \
        if (vdim == 1) bdr_launch<DIM, FN, 1>(L, F, nd, count, list);   \
        else bdr_launch<DIM, FN, DIM>(L, F, nd, count, list);           \
        return;                                                         \
    }
    SA_BDR_CASE(2, 2)
    SA_BDR_CASE(2, 3)
    SA_BDR_CASE(3, 3)
    SA_BDR_CASE(3, 4)
    SA_BDR_CASE(3, 9)
    SA_BDR_CASE(3, 6)
#undef SA_BDR_CASE
    SA_REQUIRE(false, "boundary forms: no such face type");
}

// the face mass (g nullptr) or the face loads of the arguments of saamge_amd_boundary_mass / _loads, already checked
void boundary_forms(hipStream_t s, const std::string &name, int NV, int dim, const double *coords, int NE, int nde,
                    const int *elem_ptr, const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                    const double *coef, const double *g, double *out, long long info[8]) {
    if (NF == 0) return;
    if (NE == 0 && info) info[6] = 0;
    SA_REQUIRE(NE > 0, name + "face 0: face_elem is outside [0, NE)");
    EmMesh M;
    em_mesh(s, name, NV, dim, NE, nde, elem_ptr, elem_to_vertex, vdim, !g, M, nullptr);
    // ---- the face list: ranges, repeated pairs, the key of every face
    FaceList FL;
    check_face_list(s, name, dim, NE, M.eI, NF, face_elem, face_local, FL, info ? info + 6 : nullptr);
    const int *fe = FL.fe;
    const DBuf<int> &key = FL.key;
    DBuf<int> words(1), flag((size_t)NF), pos((size_t)NF + 1);
    // ---- one list per (element type, local face)
    DBuf<int> list[EM_TYPES][BDR_MAX_FACES];
    int count[EM_TYPES][BDR_MAX_FACES] = {};
    int64_t doubles = 0;
    for (int t = 0; t < EM_TYPES; ++t) {
        if (!M.count[t]) continue;
        for (int lf = 0; lf < bdr_num_faces(t); ++lf) {
            const int c = count[t][lf] = make_list(s, NF, key.p, t * 8 + lf, flag, pos, list[t][lf]);
            const int fn = BDR_FACE_NODES[t][lf];
            if (info) info[bdr_face_type(dim, fn)] += c;
            doubles += (int64_t)c * (g ? fn * vdim : fn * fn * vdim);
        }
    }
    if (info) {
        info[5] = (long long)doubles;
        info[7] = FL.touched;
    }
    // ---- the passes: ascending local face, so that the faces of one element are added in that order
    DBuf<double> hold_X, hold_c, hold_g, hold_out;
    BdrLaunch L;
    L.s = s;
    L.eI = elem_ptr ? M.eI : nullptr;
    L.eJ = M.eJ;
    L.face_elem = fe;
    L.moff = M.moff.p;
    L.coords = device_view(hold_X, coords, (size_t)NV * dim, s);
    L.coef = coef ? device_view(hold_c, coef, (size_t)NF, s) : nullptr;
    L.g = g ? device_view(hold_g, g, (size_t)NV * vdim, s) : nullptr;
    L.out = out;
    if (out && !is_device_ptr(out)) {
        upload(hold_out, (const double *)out, (size_t)M.doubles, s);
        L.out = hold_out.p;
    }
    L.bad = words.p;
    SA_HIP_CHECK(hipMemsetAsync(words.p, 0x7f, sizeof(int), s));
    for (int lf = 0; lf < BDR_MAX_FACES; ++lf)
        for (int t = 0; t < EM_TYPES; ++t)
            if (count[t][lf]) bdr_launch_face(L, dim, vdim, t, lf, count[t][lf], list[t][lf].p);
    const int bad = read_one((const int *)words.p, s);
    if (bad < NF) {
        if (info) info[6] = bad;
        SA_REQUIRE(false, name + "face " + std::to_string(bad) + ": the measure is not positive");
    }
    if (hold_out.p) SA_HIP_CHECK(hipMemcpyAsync(out, hold_out.p, (size_t)M.doubles * sizeof(double), hipMemcpyDeviceToHost, s));
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

// the checks of both entry points that need no device
void bdr_begin(const std::string &name, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
               const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim, long long info[8]) {
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(NF >= 0, name + "NF < 0");
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NF == 0 || (face_elem && face_local), name + "null argument: face_elem or face_local");
    SA_REQUIRE(NF == 0 || NE == 0 || (coords && elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, vdim);
}

}  // namespace

// The mesh argument of every call of this file and of mesh_faces.hip (elmat.h)
void import_mesh(hipStream_t s, const std::string &name, int NV, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex,
                 DeviceMesh &M) {
    // ---- the mesh: offsets first, they say how much of elem_to_vertex there is
    if (elem_ptr) {
        M.eI = device_view(M.hold_I, elem_ptr, (size_t)NE + 1, s);
    } else {
        M.hold_I.alloc((size_t)NE + 1);
        hipLaunchKernelGGL(em_offsets_kernel, grid_flat((long)NE + 1), dim3(256), 0, s, NE, nde, M.hold_I.p);
        SA_HIP_CHECK(hipGetLastError());
        M.eI = M.hold_I.p;
    }
    M.eJ = elem_to_vertex;
    if (!is_device_ptr(elem_to_vertex)) {
        long total = (long)NE * nde;
        if (elem_ptr) {
            const hvec<int> hI = fetch_host(M.eI, (size_t)NE + 1, s);
            for (int e = 0; e < NE; ++e)
                SA_REQUIRE(hI[0] == 0 && hI[(size_t)e + 1] > hI[(size_t)e], name + "elem_ptr: must start at 0 and every element needs a vertex");
            total = hI[(size_t)NE];
        }
        upload(M.hold_J, elem_to_vertex, (size_t)total, s);
        M.eJ = M.hold_J.p;
    }
    M.nconn = check_mesh_device(s, NE, M.eI, M.eJ, NV);      // offsets, vertex ids in [0, NV), no vertex twice in an element
}

// The checks of a face list (elmat.h): shared by the boundary forms and the face-list calls of mesh_faces.hip.
void check_face_list(hipStream_t s, const std::string &name, int dim, int NE, const int *eI, int NF, const int *face_elem,
                     const int *face_local, FaceList &L, long long *refused) {
    L.key.alloc((size_t)NF);
    DBuf<int> words(3);
    const int *fe = L.fe = device_view(L.hold_fe, face_elem, (size_t)NF, s);
    const int *fl = L.fl = device_view(L.hold_fl, face_local, (size_t)NF, s);
    const int nwords = (int)(((int64_t)NE + 3) / 4);
    DBuf<unsigned> mask((size_t)nwords);
    mask.zero(s);
    const int init[3] = {INT_MAX, 0, 0};
    SA_HIP_CHECK(hipMemcpyAsync(words.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(bdr_check_kernel, grid_flat(NF), dim3(256), 0, s, NF, NE, dim, eI, fe, fl, mask.p, L.key.p, words.p);
    SA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bdr_touched_kernel, grid_flat(nwords), dim3(256), 0, s, nwords, (const unsigned *)mask.p, words.p + 2);
    SA_HIP_CHECK(hipGetLastError());
    int w[3];
    read_back(w, (const int *)words.p, 3, s);
    if (w[0] < NF) {
        if (refused) *refused = w[0];
        const int e = read_one(fe + w[0], s);
        SA_REQUIRE(false, name + "face " + std::to_string(w[0]) + ": " +
                              (e < 0 || e >= NE ? "face_elem is outside [0, NE)" : "face_local is outside the element type's range"));
    }
    if (w[1]) {      // a pair is listed twice: the first face of the list that is one of a repeated pair, found on the host
        const hvec<int> he = fetch_host(fe, (size_t)NF, s), hl = fetch_host(fl, (size_t)NF, s);
        std::vector<std::pair<int64_t, int>> pairs((size_t)NF);
        for (int f = 0; f < NF; ++f) pairs[(size_t)f] = {(int64_t)he[(size_t)f] * 8 + hl[(size_t)f], f};
        std::sort(pairs.begin(), pairs.end());
        int first = NF;
        for (size_t k = 0; k + 1 < pairs.size(); ++k)
            if (pairs[k].first == pairs[k + 1].first && (k == 0 || pairs[k - 1].first != pairs[k].first)) first = std::min(first, pairs[k].second);
        if (refused) *refused = first;
        SA_REQUIRE(false, name + "face " + std::to_string(first) + ": the same (element, local face) is listed twice");
    }
    L.touched = w[2];
}

namespace {
// saamge_amd_element_matrices and, at_points, saamge_amd_element_matrices_points: coef then holds a row per point of the mass rule
void stiffness(hipStream_t s, const std::string &name, bool at_points, int NV, int dim, const double *coords, int NE, int nde,
               const int *elem_ptr, const int *elem_to_vertex, int kind, int ncoef, const double *coef, double *elmat_out,
               int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    // ---- what needs no device
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(kind == 0 || kind == 1, name + "kind must be 0 (diffusion) or 1 (elasticity)");
    if (kind == 1)
        SA_REQUIRE(ncoef == 2, name + "ncoef must be 2 (lambda, mu) for elasticity");
    else
        SA_REQUIRE(ncoef == 1 || ncoef == dim || ncoef == dim * (dim + 1) / 2,
                   name + "ncoef must be 1, dim or dim (dim + 1) / 2 for diffusion");
    SA_REQUIRE(NE == 0 || (coords && elem_to_vertex && coef),
               name + "null argument: coords, elem_to_vertex or " + (at_points ? "coefq" : "coef"));
    const int comp = kind ? dim : 1;
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, comp);
    if (NE == 0) return;
    EmMesh M;
    em_mesh(s, name, NV, dim, NE, nde, elem_ptr, elem_to_vertex, comp, true, M, info);
    const int *eI = M.eI, *eJ = M.eJ;
    const long nconn = M.nconn;
    const int64_t doubles = M.doubles;      // (info[5])
    // ---- the matrices (elmat_out NULL: the determinants are still checked)
    DBuf<double> hold_X, hold_c, hold_out;
    DBuf<roff_t> qoff;
    const size_t rows = at_points ? (size_t)qp_offsets(s, dim, NE, nde, elem_ptr, M, qoff) : (size_t)NE;
    EmLaunch L;
    L.s = s;
    L.eI = elem_ptr ? eI : nullptr;
    L.eJ = eJ;
    L.moff = M.moff.p;
    L.qoff = qoff.p;
    L.coords = device_view(hold_X, coords, (size_t)NV * dim, s);
    L.coef = device_view(hold_c, coef, rows * ncoef, s);
    L.ncoef = ncoef;
    L.out = elmat_out;
    if (elmat_out && !is_device_ptr(elmat_out)) {
        hold_out.alloc((size_t)doubles);
        L.out = hold_out.p;
    }
    L.bad = M.word.p;
    SA_HIP_CHECK(hipMemsetAsync(M.word.p, 0x7f, sizeof(int), s));
    for (int t = 0; t < EM_TYPES; ++t) {
        if (!M.count[t]) continue;
        if (kind) em_launch_type<1>(L, t, M.count[t], M.list[t].p);
        else em_launch_type<0>(L, t, M.count[t], M.list[t].p);
    }
    em_refuse_bad(s, name, M, NE, info);
    if (hold_out.p) SA_HIP_CHECK(hipMemcpyAsync(elmat_out, hold_out.p, (size_t)doubles * sizeof(double), hipMemcpyDeviceToHost, s));
    // ---- the dof lists the matrices are indexed by
    DBuf<int> dptr, dofs;
    if (dof_ptr_out) {
        dptr.alloc((size_t)NE + 1);
        hipLaunchKernelGGL(em_dof_ptr_kernel, grid_flat((long)NE + 1), dim3(256), 0, s, NE, comp, eI, dptr.p);
        SA_HIP_CHECK(hipGetLastError());
        SA_HIP_CHECK(hipMemcpyAsync(dof_ptr_out, dptr.p, ((size_t)NE + 1) * sizeof(int), hipMemcpyDefault, s));
    }
    if (elem_to_dof_out) {
        dofs.alloc((size_t)nconn * comp);
        hipLaunchKernelGGL(em_dofs_kernel, grid_flat(nconn), dim3(256), 0, s, nconn, comp, eJ, dofs.p);
        SA_HIP_CHECK(hipGetLastError());
        SA_HIP_CHECK(hipMemcpyAsync(elem_to_dof_out, dofs.p, (size_t)nconn * comp * sizeof(int), hipMemcpyDefault, s));
    }
    SA_HIP_CHECK(hipStreamSynchronize(s));
}
}  // namespace

void element_matrices(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                      const int *elem_to_vertex, int kind, int ncoef, const double *coef, double *elmat_out, int *dof_ptr_out,
                      int *elem_to_dof_out, long long info[8]) {
    stiffness(s, EM_NAME, false, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, kind, ncoef, coef, elmat_out, dof_ptr_out,
              elem_to_dof_out, info);
}

void element_matrices_points(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int kind, int ncoef, const double *coefq, double *elmat_out,
                             int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    stiffness(s, "saamge_amd_element_matrices_points: ", true, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, kind, ncoef, coefq,
              elmat_out, dof_ptr_out, elem_to_dof_out, info);
}

void element_mass_points(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                         const int *elem_to_vertex, int vdim, const double *coefq, int accumulate, double *elmat_inout,
                         long long info[8]) {
    const std::string name("saamge_amd_element_mass_points: ");
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NE == 0 || coefq, name + "null argument: coefq");
    SA_REQUIRE(NE == 0 || (coords && elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    SA_REQUIRE(!accumulate || elmat_inout, name + "null argument: accumulate needs the matrices in elmat_inout");
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, vdim);
    mass_or_loads(s, name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coefq, nullptr, accumulate ? 1 : 0, elmat_inout,
                  info, true);
}

void element_mass(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                  const int *elem_to_vertex, int vdim, const double *coef, int accumulate, double *elmat_inout, long long info[8]) {
    const std::string name("saamge_amd_element_mass: ");
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(NE == 0 || coef, name + "null argument: coef");
    SA_REQUIRE(NE == 0 || (coords && elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    SA_REQUIRE(!accumulate || elmat_inout, name + "null argument: accumulate needs the matrices in elmat_inout");
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, vdim);
    mass_or_loads(s, name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, nullptr, accumulate ? 1 : 0, elmat_inout,
                  info);
}

void element_loads(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                   const int *elem_to_vertex, int vdim, const double *coef, const double *src, double *elvec_out,
                   long long info[8]) {
    const std::string name("saamge_amd_element_loads: ");
    em_begin(name, NV, dim, NE, info);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(src, name + "null argument: src");
    SA_REQUIRE(NE == 0 || (coords && elem_to_vertex), name + "null argument: coords or elem_to_vertex");
    em_check_sizes(name, NV, dim, NE, nde, elem_ptr, vdim);
    mass_or_loads(s, name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, src, 0, elvec_out, info);
}

void boundary_mass(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                   const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                   double *elmat_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_mass: ");
    bdr_begin(name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(NF == 0 || coef, name + "null argument: coef");
    boundary_forms(s, name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coef, nullptr,
                   elmat_inout, info);
}

void boundary_loads(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                    const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim, const double *coef,
                    const double *g, double *elvec_inout, long long info[8]) {
    const std::string name("saamge_amd_boundary_loads: ");
    bdr_begin(name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, info);
    SA_REQUIRE(g, name + "null argument: g");
    boundary_forms(s, name, NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coef, g,
                   elvec_inout, info);
}

void element_points(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                    const int *elem_to_vertex, long long *qp_ptr_out, double *xq_out, double *wdet_out, long long info[8]) {
    points_call(QP_POINTS, s, "saamge_amd_element_points: ", NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, 1, nullptr, nullptr,
                "", nullptr, nullptr, qp_ptr_out, xq_out, wdet_out, info);
}

void element_eval(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                  const int *elem_to_vertex, int vdim, const double *u, double *uq_out, double *gradq_out, long long info[8]) {
    points_call(QP_EVAL, s, "saamge_amd_element_eval: ", NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, nullptr, u, "u",
                nullptr, nullptr, nullptr, uq_out, gradq_out, info);
}

void element_loads_points(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                          const int *elem_to_vertex, int vdim, const double *coef, const double *fq, double *elvec_out,
                          long long info[8]) {
    points_call(QP_LOADS, s, "saamge_amd_element_loads_points: ", NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, fq,
                "fq", nullptr, nullptr, nullptr, elvec_out, nullptr, info);
}

void element_errors(hipStream_t s, int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                    const int *elem_to_vertex, int vdim, const double *u, const double *exq, const double *exgradq, double *err_out,
                    long long info[8]) {
    points_call(QP_ERRORS, s, "saamge_amd_element_errors: ", NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, nullptr, u, "u",
                exq, exgradq, nullptr, err_out, nullptr, info);
}

}  // namespace saamge_amd
