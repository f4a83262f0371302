// The reference elements of the element layer (elmat.hip), each written once: the shape functions of the nine element types and
// of the two segments, the quadrature rules, the tables the kernels read and the dispatch over the types.  Plain constexpr C++17,
// no HIP: saamge_amd/elmat_model.py defines every value, tests/cxx/elmat_ref_test.cpp prints the tables on the host and
// tests/test_cxx_elmat_ref.py holds them to the model bit for bit.  The expressions, their order and their parentheses are the
// model's: every product and sum below is one rounding of the definition.
#pragma once
#include "elmat_types.h"

#include <type_traits>

namespace saamge_amd {

// ---- the literals of elmat_model.py -------------------------------------------------------------------------------------------
constexpr double EM_GAUSS[2] = {0.21132486540518713, 0.7886751345948129};
constexpr double EM2_GAUSS[3] = {0.11270166537925831, 0.5, 0.8872983346207417};
constexpr double EM2_W[3] = {0.2777777777777778, 0.4444444444444444, 0.2777777777777778};
constexpr double EM_SIXTH = 0.16666666666666666, EM_24TH = 0.041666666666666664;      // the weights 1/6 and 1/24
constexpr double EM_TRI_A = EM_SIXTH, EM_TRI_B = 0.6666666666666666;
constexpr double EM_TET_A = 0.1381966011250105, EM_TET_B = 0.5854101966249685;
constexpr double EM_P2_TRI_A[2] = {0.44594849091596483, 0.09157621350977073};
constexpr double EM_P2_TRI_W[2] = {0.11169079483900572, 0.054975871827660935};
constexpr double EM_P2_TET_A[2] = {0.3108859192633006, 0.09273525031089122};
constexpr double EM_P2_TET_W[3] = {0.018781320953002643, 0.012248840519393659, 0.007091003462846911};
constexpr double EM_P2_TET_EDGE_A = 0.04550370412564965;
constexpr int EM_QUAD_LOC[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
constexpr double EM_TRI_D[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
constexpr double EM_TET_D[4][3] = {{-1.0, -1.0, -1.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
constexpr double EM_WEDGE_TRI[3][2] = {{EM_TRI_A, EM_TRI_A}, {EM_TRI_B, EM_TRI_A}, {EM_TRI_A, EM_TRI_B}};
constexpr int EM_P2_TRI_EDGES[3][2] = {{0, 1}, {1, 2}, {2, 0}};
constexpr int EM_P2_TET_EDGES[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// (EM_HEX_LOC, EM2_QUAD_LOC and the type indices -- EM_TYPES, em_type_index, EM_TYPE_ND -- are in elmat_types.h)

// the 1-D shape functions and their derivatives: order 1 on the nodes 0, 1 (_f, _df), order 2 on 0, 1/2, 1 (_n2, _d2)
constexpr double em_f(int l, double p) { return l ? p : 1.0 - p; }
constexpr double em_df(int l) { return l ? 1.0 : -1.0; }
constexpr double em2_n(int l, double p) {
    return l == 0 ? (2.0 * p - 1.0) * (p - 1.0) : (l == 1 ? (4.0 * p) * (1.0 - p) : p * (2.0 * p - 1.0));
}
constexpr double em2_d(int l, double p) { return l == 0 ? 4.0 * p - 3.0 : (l == 1 ? 4.0 - 8.0 * p : 4.0 * p - 1.0); }

// ---- the shape functions: N[a] and dN[a][j] of the type <DIM, ND> at the reference point pt -----------------------------------
// DIM 1: the 2-node and the 3-node segment (the faces of the 2-D types)
template <int DIM, int ND>
struct RefShape {
    double N[ND];
    double dN[ND][DIM];
};
// the order-2 simplices (elmat_model._p2_simplex): the vertices, then the midpoints of the edges EM_P2_TRI_EDGES / EM_P2_TET_EDGES,
// from the barycentric coordinates L and their constant gradients EM_TRI_D / EM_TET_D
template <int DIM>
constexpr RefShape<DIM, (DIM == 2 ? 6 : 10)> ref_shape_p2_simplex(const double *pt) {
    constexpr int ND = DIM == 2 ? 6 : 10;
    RefShape<DIM, ND> r{};
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
    for (int e = 0; e < ND - DIM - 1; ++e) {
        const int i = DIM == 2 ? EM_P2_TRI_EDGES[e % 3][0] : EM_P2_TET_EDGES[e][0];
        const int j = DIM == 2 ? EM_P2_TRI_EDGES[e % 3][1] : EM_P2_TET_EDGES[e][1];
        r.N[DIM + 1 + e] = (4.0 * L[i]) * L[j];
        for (int k = 0; k < DIM; ++k) r.dN[DIM + 1 + e][k] = (4.0 * L[i]) * D[j][k] + (4.0 * L[j]) * D[i][k];
    }
    return r;
}
template <int DIM, int ND>
constexpr RefShape<DIM, ND> ref_shape(const double *pt) {
    RefShape<DIM, ND> r{};
    const double px = pt[0], py = pt[DIM > 1 ? 1 : 0], pz = pt[DIM - 1];
    (void)px, (void)py, (void)pz;
    if constexpr (DIM == 1 && ND == 2) {                  // the 2-node segment
        for (int a = 0; a < 2; ++a) {
            r.N[a] = em_f(a, px);
            r.dN[a][0] = em_df(a);
        }
    } else if constexpr (DIM == 1 && ND == 3) {           // the 3-node segment
        for (int a = 0; a < 3; ++a) {
            r.N[a] = em2_n(a, px);
            r.dN[a][0] = em2_d(a, px);
        }
    } else if constexpr (DIM == 2 && ND == 3) {           // the triangle
        r.N[0] = (1.0 - px) - py;
        r.N[1] = px;
        r.N[2] = py;
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 2; ++j) r.dN[a][j] = EM_TRI_D[a][j];
    } else if constexpr (DIM == 3 && ND == 4) {           // the tetrahedron
        r.N[0] = ((1.0 - px) - py) - pz;
        r.N[1] = px;
        r.N[2] = py;
        r.N[3] = pz;
        for (int a = 0; a < 4; ++a)
            for (int j = 0; j < 3; ++j) r.dN[a][j] = EM_TET_D[a][j];
    } else if constexpr (DIM == 2 && ND == 4) {           // the quadrilateral
        for (int a = 0; a < 4; ++a) {
            const int lx = EM_QUAD_LOC[a][0], ly = EM_QUAD_LOC[a][1];
            r.N[a] = em_f(lx, px) * em_f(ly, py);
            r.dN[a][0] = em_df(lx) * em_f(ly, py);
            r.dN[a][1] = em_f(lx, px) * em_df(ly);
        }
    } else if constexpr (DIM == 3 && ND == 8) {           // the hexahedron
        for (int a = 0; a < 8; ++a) {
            const int lx = EM_HEX_LOC[a][0], ly = EM_HEX_LOC[a][1], lz = EM_HEX_LOC[a][2];
            r.N[a] = em_f(lx, px) * (em_f(ly, py) * em_f(lz, pz));
            r.dN[a][0] = em_df(lx) * (em_f(ly, py) * em_f(lz, pz));
            r.dN[a][1] = em_df(ly) * (em_f(lx, px) * em_f(lz, pz));
            r.dN[a][2] = em_df(lz) * (em_f(lx, px) * em_f(ly, py));
        }
    } else if constexpr (DIM == 3 && ND == 6) {           // the wedge: node a * 3 + i, triangle vertex i on the face a
        const double T[3] = {(1.0 - px) - py, px, py};
        const double L[2] = {1.0 - pz, pz};
        for (int a = 0; a < 2; ++a)
            for (int i = 0; i < 3; ++i) {
                r.N[a * 3 + i] = T[i] * L[a];
                r.dN[a * 3 + i][0] = EM_TRI_D[i][0] * L[a];
                r.dN[a * 3 + i][1] = EM_TRI_D[i][1] * L[a];
                r.dN[a * 3 + i][2] = T[i] * em_df(a);
            }
    } else if constexpr (DIM == 2 && ND == 9) {           // the 9-node quadrilateral (EM2_QUAD_LOC)
        for (int a = 0; a < 9; ++a) {
            const int ix = EM2_QUAD_LOC[a][0], iy = EM2_QUAD_LOC[a][1];
            r.N[a] = em2_n(ix, px) * em2_n(iy, py);
            r.dN[a][0] = em2_d(ix, px) * em2_n(iy, py);
            r.dN[a][1] = em2_n(ix, px) * em2_d(iy, py);
        }
    } else if constexpr (DIM == 3 && ND == 27) {          // the 27-node hexahedron (lexicographic)
        for (int a = 0; a < 27; ++a) {
            const int ix = a % 3, iy = (a / 3) % 3, iz = a / 9;
            r.N[a] = em2_n(ix, px) * (em2_n(iy, py) * em2_n(iz, pz));
            r.dN[a][0] = em2_d(ix, px) * (em2_n(iy, py) * em2_n(iz, pz));
            r.dN[a][1] = em2_d(iy, py) * (em2_n(ix, px) * em2_n(iz, pz));
            r.dN[a][2] = em2_d(iz, pz) * (em2_n(ix, px) * em2_n(iy, py));
        }
    } else {                                              // the 6-node triangle and the 10-node tetrahedron
        static_assert((DIM == 2 && ND == 6) || (DIM == 3 && ND == 10), "no such element type");
        r = ref_shape_p2_simplex<DIM>(pt);
    }
    return r;
}

// ---- the rules: points and weights --------------------------------------------------------------------------------------------
template <int DIM, int NQ_>
struct RefRule {
    static constexpr int NQ = NQ_;
    double x[NQ_][DIM];
    double w[NQ_];
};
constexpr int ref_pow(int b, int e) { return e ? b * ref_pow(b, e - 1) : 1; }
// one point, the weight the reference measure: the stiffness rule of the order-1 simplices, whose gradients are constant (the
// point, the centroid, enters no table value)
template <int DIM>
constexpr RefRule<DIM, 1> rule_simplex_1() {
    RefRule<DIM, 1> r{};
    for (int d = 0; d < DIM; ++d) r.x[0][d] = 1.0 / (DIM + 1);
    r.w[0] = DIM == 2 ? 0.5 : EM_SIXTH;
    return r;
}
// 2 Gauss points per axis: axis d of point q takes EM_GAUSS[(q >> d) & 1]
template <int DIM>
constexpr RefRule<DIM, (1 << DIM)> rule_gauss2() {
    RefRule<DIM, (1 << DIM)> r{};
    for (int q = 0; q < (1 << DIM); ++q) {
        for (int d = 0; d < DIM; ++d) r.x[q][d] = EM_GAUSS[(q >> d) & 1];
        r.w[q] = DIM == 1 ? 0.5 : (DIM == 2 ? 0.25 : 0.125);
    }
    return r;
}
// 3 Gauss points per axis: point q = (qz * 3 + qy) * 3 + qx, weight (wx * wy) * wz
template <int DIM>
constexpr RefRule<DIM, ref_pow(3, DIM)> rule_gauss3() {
    RefRule<DIM, ref_pow(3, DIM)> r{};
    for (int q = 0; q < ref_pow(3, DIM); ++q) {
        const int qx = q % 3, qy = (q / 3) % 3, qz = q / 9;
        for (int d = 0; d < DIM; ++d) r.x[q][d] = EM2_GAUSS[(q / ref_pow(3, d)) % 3];
        r.w[q] = DIM == 1 ? EM2_W[qx] : (DIM == 2 ? EM2_W[qx] * EM2_W[qy] : (EM2_W[qx] * EM2_W[qy]) * EM2_W[qz]);
    }
    return r;
}
// the triangle's 3 points (degree 2), weight 1/6, and the tetrahedron's 4, weight 1/24
constexpr RefRule<2, 3> rule_tri3() {
    RefRule<2, 3> r{};
    for (int q = 0; q < 3; ++q) {
        r.x[q][0] = EM_WEDGE_TRI[q][0];
        r.x[q][1] = EM_WEDGE_TRI[q][1];
        r.w[q] = EM_SIXTH;
    }
    return r;
}
constexpr RefRule<3, 4> rule_tet4() {
    RefRule<3, 4> r{};
    for (int q = 0; q < 4; ++q) {
        for (int d = 0; d < 3; ++d) r.x[q][d] = q == d + 1 ? EM_TET_B : EM_TET_A;
        r.w[q] = EM_24TH;
    }
    return r;
}
// the wedge: point q = 3 * qz + qt, the triangle's 3 points times 2 Gauss points
constexpr RefRule<3, 6> rule_wedge6() {
    RefRule<3, 6> r{};
    for (int q = 0; q < 6; ++q) {
        r.x[q][0] = EM_WEDGE_TRI[q % 3][0];
        r.x[q][1] = EM_WEDGE_TRI[q % 3][1];
        r.x[q][2] = EM_GAUSS[q / 3];
        r.w[q] = 0.08333333333333333;
    }
    return r;
}
// the mass rules of the order-2 simplices (P2_TRI_POINTS, degree 4; P2_TET_POINTS, degree 5)
constexpr RefRule<2, 6> rule_tri6() {
    RefRule<2, 6> r{};
    for (int q = 0; q < 6; ++q) {
        const double a = EM_P2_TRI_A[q / 3], b = 1.0 - 2.0 * a;
        r.x[q][0] = q % 3 == 1 ? b : a;
        r.x[q][1] = q % 3 == 2 ? b : a;
        r.w[q] = EM_P2_TRI_W[q / 3];
    }
    return r;
}
constexpr RefRule<3, 14> rule_tet14() {
    RefRule<3, 14> r{};
    for (int q = 0; q < 8; ++q) {
        const double a = EM_P2_TET_A[q / 4], b = 1.0 - 3.0 * a;
        for (int d = 0; d < 3; ++d) r.x[q][d] = q % 4 == d + 1 ? b : a;
        r.w[q] = EM_P2_TET_W[q / 4];
    }
    for (int q = 8; q < 14; ++q) {      // one point per edge (i, j): the barycentrics i and j are b, the point (L1, L2, L3)
        const double a = EM_P2_TET_EDGE_A, b = 0.5 - a;
        const int i = EM_P2_TET_EDGES[q - 8][0], j = EM_P2_TET_EDGES[q - 8][1];
        for (int d = 0; d < 3; ++d) r.x[q][d] = i == d + 1 || j == d + 1 ? b : a;
        r.w[q] = EM_P2_TET_W[2];
    }
    return r;
}

// which rule a type takes.  Stiffness: elmat_model.NPOINTS / point_weight; the order-2 simplices take the order-1 mass rules
template <int DIM, int ND>
constexpr auto ref_stiff_rule() {
    if constexpr (ND == DIM + 1) return rule_simplex_1<DIM>();
    else if constexpr (ND == (1 << DIM)) return rule_gauss2<DIM>();
    else if constexpr (ND == ref_pow(3, DIM)) return rule_gauss3<DIM>();
    else if constexpr (DIM == 3 && ND == 6) return rule_wedge6();
    else if constexpr (DIM == 2) return rule_tri3();
    else return rule_tet4();
}
// mass, loads, data at the points: the stiffness rule except for the simplices (elmat_model.MASS_NPOINTS / mass_point_weight)
template <int DIM, int ND>
constexpr auto ref_mass_rule() {
    if constexpr (DIM == 2 && ND == 3) return rule_tri3();
    else if constexpr (DIM == 3 && ND == 4) return rule_tet4();
    else if constexpr (DIM == 2 && ND == 6) return rule_tri6();
    else if constexpr (DIM == 3 && ND == 10) return rule_tet14();
    else return ref_stiff_rule<DIM, ND>();
}
// a face with FN nodes of an element of dimension DIM (elmat_model.face_rule): a segment has the Gauss points of its order, a
// face of a 3-D element is the 2-D element of its node count with that element's mass rule
template <int DIM, int FN>
constexpr auto ref_face_rule() {
    if constexpr (DIM == 3) return ref_mass_rule<2, FN>();
    else if constexpr (FN == 2) return rule_gauss2<1>();
    else return rule_gauss3<1>();
}

// ---- the tables -----------------------------------------------------------------------------------------------------------------
// Reference gradients and shape values of node a at point q and the weight of point q: dN node-major (lanes that differ in the
// point read neighbouring doubles), N point-major (the entry phases read N of neighbouring nodes at one point).
template <int DIM, int ND, int NQ_>
struct RefTable {
    static constexpr int NQ = NQ_;
    double dN[ND][NQ_][DIM];
    double N[NQ_][ND];
    double w[NQ_];
};
template <int ND, int DIM, int NQ>
constexpr RefTable<DIM, ND, NQ> ref_table(const RefRule<DIM, NQ> &rule) {
    RefTable<DIM, ND, NQ> t{};
    for (int q = 0; q < NQ; ++q) {
        const RefShape<DIM, ND> f = ref_shape<DIM, ND>(rule.x[q]);
        t.w[q] = rule.w[q];
        for (int a = 0; a < ND; ++a) {
            t.N[q][a] = f.N[a];
            for (int j = 0; j < DIM; ++j) t.dN[a][q][j] = f.dN[a][j];
        }
    }
    return t;
}
template <int DIM, int ND> using StiffRule = decltype(ref_stiff_rule<DIM, ND>());
template <int DIM, int ND> using MassRule = decltype(ref_mass_rule<DIM, ND>());
template <int DIM, int FN> using FaceRule = decltype(ref_face_rule<DIM, FN>());
// the stiffness tables of the order-2 types, the mass tables of all nine, the face tables (a face has DIM - 1 reference axes)
template <int DIM, int ND> using Em2Table = RefTable<DIM, ND, StiffRule<DIM, ND>::NQ>;
template <int DIM, int ND> using MassTable = RefTable<DIM, ND, MassRule<DIM, ND>::NQ>;
template <int DIM, int FN> using BdrTable = RefTable<DIM - 1, FN, FaceRule<DIM, FN>::NQ>;
template <int DIM, int ND> constexpr Em2Table<DIM, ND> em2_table() { return ref_table<ND>(ref_stiff_rule<DIM, ND>()); }
template <int DIM, int ND> constexpr MassTable<DIM, ND> mass_table() { return ref_table<ND>(ref_mass_rule<DIM, ND>()); }
template <int DIM, int FN> constexpr BdrTable<DIM, FN> bdr_table() { return ref_table<FN>(ref_face_rule<DIM, FN>()); }
// Two tables of one type from one rule are one object.  The stiffness rule of the 9-node quadrilateral and of the 27-node
// hexahedron is their mass rule; the table of a face of a 3-D element is the mass table of the 2-D type.
template <int DIM, int ND>
constexpr bool EM2_IS_MASS = std::is_same<StiffRule<DIM, ND>, MassRule<DIM, ND>>::value;

// The stiffness table of the order-1 types, point-major: em_kernel reads the line of its point through a wave-uniform index.
// Every point of such a rule has the same weight, W.
template <int DIM, int ND>
struct EmGrad {
    double v[ND][DIM];
};
template <int DIM, int ND>
struct EmTable {
    static constexpr int NQ = StiffRule<DIM, ND>::NQ;
    static constexpr double W = ref_stiff_rule<DIM, ND>().w[0];
    EmGrad<DIM, ND> p[NQ];
};
template <int DIM, int ND>
constexpr EmTable<DIM, ND> em_table() {
    constexpr StiffRule<DIM, ND> rule = ref_stiff_rule<DIM, ND>();
    EmTable<DIM, ND> t{};
    for (int q = 0; q < rule.NQ; ++q) {
        const RefShape<DIM, ND> f = ref_shape<DIM, ND>(rule.x[q]);
        for (int a = 0; a < ND; ++a)
            for (int j = 0; j < DIM; ++j) t.p[q].v[a][j] = f.dN[a][j];
    }
    return t;
}

// ---- the dispatch over the types ------------------------------------------------------------------------------------------------
// The element types in the order of their index (em_type_index, elmat_model.ALL_TYPE_INDEX) and the face types in the order of
// elmat_model.FACE_TYPE_INDEX: the one list of each.  with_elem_type / with_face_type call f with the tag of the type, a value
// whose type carries DIM and ND (FN) as constants; they return whether there is such a type.
template <int DIM_, int ND_>
struct ElemTag {
    static constexpr int DIM = DIM_, ND = ND_;
};
template <class... T>
struct TagList {
    static constexpr int SIZE = sizeof...(T);
};
typedef TagList<ElemTag<2, 3>, ElemTag<2, 4>, ElemTag<3, 4>, ElemTag<3, 6>, ElemTag<3, 8>, ElemTag<2, 9>, ElemTag<3, 27>, ElemTag<2, 6>,
                ElemTag<3, 10>> ElemTypes;
typedef TagList<ElemTag<2, 2>, ElemTag<2, 3>, ElemTag<3, 3>, ElemTag<3, 4>, ElemTag<3, 9>, ElemTag<3, 6>> FaceTypes;      // <DIM, FN>

template <class... T>
constexpr bool elem_types_agree(TagList<T...>) {
    int i = 0;
    bool ok = sizeof...(T) == EM_TYPES;
    ((ok = ok && em_type_index(T::DIM, T::ND) == i && EM_TYPE_ND[i] == T::ND, ++i), ...);
    return ok;
}
static_assert(elem_types_agree(ElemTypes{}), "ElemTypes, em_type_index and EM_TYPE_ND name the same nine types in the same order");

template <class F, class... T>
bool with_tag_at(TagList<T...>, int index, F &&f) {
    int i = 0;
    return ((i++ == index ? (f(T{}), true) : false) || ...);
}
template <class... T>
constexpr int tag_index(TagList<T...>, int dim, int nd) {
    int i = 0, at = -1;
    ((at = T::DIM == dim && T::ND == nd ? i : at, ++i), ...);
    return at;
}
template <class F>
bool with_elem_type(int type, F &&f) {
    return with_tag_at(ElemTypes{}, type, f);
}
template <class F>
bool with_face_type(int dim, int fn, F &&f) {
    return with_tag_at(FaceTypes{}, tag_index(FaceTypes{}, dim, fn), f);
}
// the fork on the components of a form, written once: f(tag, the constant 1 or DIM)
template <class Tag, class F>
void with_vdim(Tag tag, int vdim, F &&f) {
    if (vdim == 1) f(tag, std::integral_constant<int, 1>{});
    else f(tag, std::integral_constant<int, Tag::DIM>{});
}

// the points of the rules: the rules' sizes.  mass_points: of the mass rule of the element type (dim, nd), 0: no such type
template <class... T>
constexpr int mass_points_of(TagList<T...>, int dim, int nd) {
    int n = 0;
    ((n = T::DIM == dim && T::ND == nd ? MassRule<T::DIM, T::ND>::NQ : n), ...);
    return n;
}
constexpr int mass_points(int dim, int nd) { return mass_points_of(ElemTypes{}, dim, nd); }
constexpr bool em_order1(int dim, int nd) { return em_type_index(dim, nd) >= 0 && em_type_index(dim, nd) < 5; }
// face_points: of the rule of the face type (dim, fn), 0: no such face type
template <class... T>
constexpr int face_points_of(TagList<T...>, int dim, int fn) {
    int n = 0;
    ((n = T::DIM == dim && T::ND == fn ? FaceRule<T::DIM, T::ND>::NQ : n), ...);
    return n;
}
constexpr int face_points(int dim, int fn) { return face_points_of(FaceTypes{}, dim, fn); }
// the dimension of the element type with this index, 0: no such type
template <class... T>
constexpr int elem_dim_of(TagList<T...>, int type) {
    int i = 0, d = 0;
    ((d = i++ == type ? T::DIM : d), ...);
    return d;
}
constexpr int em_type_dim(int type) { return elem_dim_of(ElemTypes{}, type); }
// the fork on the node count of a local face of an element type, written once: f(the constant FN).  The faces of a type have
// one node count, except the wedge's (triangles first, then quadrilaterals)
template <int DIM, int ND, class F>
void with_face_nodes(ElemTag<DIM, ND>, int fn, F &&f) {
    constexpr int T = em_type_index(DIM, ND), A = BDR_FACE_NODES[T][0], B = BDR_FACE_NODES[T][bdr_num_faces(T) - 1];
    if (fn == A) f(std::integral_constant<int, A>{});
    else if constexpr (B != A) {
        if (fn == B) f(std::integral_constant<int, B>{});
    }
}

// ---- the element's gradients at the face points (elmat_model.REF_NODES, face_ref_point, face_gradients) -----------------------------
// the reference position of node a of the type, coordinate k
template <int DIM, int ND>
constexpr double ref_node(int a, int k) {
    if constexpr (ND == DIM + 1) {                            // the vertices of the simplex
        return a == k + 1 ? 1.0 : 0.0;
    } else if constexpr (DIM == 2 && ND == 4) {
        return EM_QUAD_LOC[a][k];
    } else if constexpr (DIM == 3 && ND == 8) {
        return EM_HEX_LOC[a][k];
    } else if constexpr (DIM == 3 && ND == 6) {               // node a = 3 * layer + triangle vertex
        return k == 2 ? a / 3 : (a % 3 == k + 1 ? 1.0 : 0.0);
    } else if constexpr (DIM == 2 && ND == 9) {
        return 0.5 * EM2_QUAD_LOC[a][k];
    } else if constexpr (DIM == 3 && ND == 27) {
        return 0.5 * (k == 0 ? a % 3 : (k == 1 ? (a / 3) % 3 : a / 9));
    } else {                                                  // the order-2 simplices: the vertices, then the midpoints of the edges
        if (a <= DIM) return a == k + 1 ? 1.0 : 0.0;
        const int i = DIM == 2 ? EM_P2_TRI_EDGES[(a - DIM - 1) % 3][0] : EM_P2_TET_EDGES[(a - DIM - 1) % 6][0];
        const int j = DIM == 2 ? EM_P2_TRI_EDGES[(a - DIM - 1) % 3][1] : EM_P2_TET_EDGES[(a - DIM - 1) % 6][1];
        return 0.5 * ((i == k + 1 ? 1.0 : 0.0) + (j == k + 1 ? 1.0 : 0.0));
    }
}
// xi, the reference position in the element <DIM, ND> of point q of a face F with the table `face`: the sum over the face nodes
// c, ascending, of N_c(q) * ref_node(node c), the first product as it is, N from the face's own table (ref_table, the one builder)
template <int DIM, int ND, int FN>
constexpr void face_ref_point(const BdrTable<DIM, FN> &face, const BdrFace &F, int q, double (&xi)[DIM]) {
    for (int k = 0; k < DIM; ++k) {
        double v = face.N[q][0] * ref_node<DIM, ND>(F.node[0], k);
        for (int c = 1; c < FN; ++c) v = v + face.N[q][c] * ref_node<DIM, ND>(F.node[c], k);
        xi[k] = v;
    }
}
// Per local face lf of the element type <DIM, ND> and per point q of the face's rule: dN[a][q][k], the gradients of ALL nodes of
// the element at face_ref_point (ref_shape).  A face's block is node-major like RefTable::dN, the points MAXQ apart (the wedge's
// triangles have 3 points, its quadrilaterals 4).
template <int DIM, int ND>
struct FaceGradTable {
    static constexpr int TYPE = em_type_index(DIM, ND), NF = bdr_num_faces(TYPE);
    static constexpr int MAXQ = face_points(DIM, BDR_FACE_NODES[TYPE][0]) > face_points(DIM, BDR_FACE_NODES[TYPE][NF - 1])
                                    ? face_points(DIM, BDR_FACE_NODES[TYPE][0])
                                    : face_points(DIM, BDR_FACE_NODES[TYPE][NF - 1]);
    double dN[NF][ND][MAXQ][DIM];
};
template <int DIM, int ND, int FN>
constexpr void face_grad_fill(FaceGradTable<DIM, ND> &t, int lf) {
    if constexpr (tag_index(FaceTypes{}, DIM, FN) >= 0) {
        const BdrTable<DIM, FN> face = bdr_table<DIM, FN>();
        const BdrFace F = bdr_face(em_type_index(DIM, ND), lf);
        for (int q = 0; q < BdrTable<DIM, FN>::NQ; ++q) {
            double xi[DIM] = {};
            face_ref_point<DIM, ND, FN>(face, F, q, xi);
            const RefShape<DIM, ND> f = ref_shape<DIM, ND>(xi);
            for (int a = 0; a < ND; ++a)
                for (int k = 0; k < DIM; ++k) t.dN[lf][a][q][k] = f.dN[a][k];
        }
    }
}
template <int DIM, int ND>
constexpr FaceGradTable<DIM, ND> face_grad_table() {
    FaceGradTable<DIM, ND> t{};
    for (int lf = 0; lf < t.NF; ++lf) {
        const int fn = BDR_FACE_NODES[t.TYPE][lf];
        if (fn == 2) face_grad_fill<DIM, ND, 2>(t, lf);
        else if (fn == 3) face_grad_fill<DIM, ND, 3>(t, lf);
        else if (fn == 4) face_grad_fill<DIM, ND, 4>(t, lf);
        else if (fn == 6) face_grad_fill<DIM, ND, 6>(t, lf);
        else face_grad_fill<DIM, ND, 9>(t, lf);
    }
    return t;
}

}  // namespace saamge_amd
