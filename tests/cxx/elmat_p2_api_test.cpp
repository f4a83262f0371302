// TEST: the order-2 simplices through saamge_amd::api and libsaamge_amd.so.  Without an argument only the checks that need no
// GPU run: 6 nodes in 2D and 10 nodes in 3D pass the size checks of all five calls (a call without elements), 10 nodes in 2D
// and 5 in 3D are refused with the library's message.  With "gpu": the unit 6-node triangle and the unit 10-node tetrahedron,
// straight-sided, against the closed forms of their diffusion matrix (6 K and 30 K are integer tables) and their mass matrix
// (area / 180 and volume / 420 times integer tables), the load vector of the source 1 (the row sums of the mass matrix: 0 at a
// vertex of the triangle, area / 3 at a midside node; - volume / 20 and volume / 5 on the tetrahedron), the face mass of one
// face of the tetrahedron (the triangle's table times the face's area) and a face index that the type does not have.
// The bounds are the model's own deviation from these closed forms on these two elements (mass 2.47, stiffness 0.79 units of
// 2^-52 of the largest entry; the device gives the model's bits) with the project's margin of 8.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

static const double EPS = 2.220446049250313e-16, MASS_UNITS = 8 * 2.47, STIFF_UNITS = 8 * 0.79;

static bool refused(const char *what, int NV, int dim, const double *coords, int NE, int nde, const int *lists) {
    const double c[2] = {1, 1};
    try {
        element_matrices(NV, dim, coords, NE, nde, nullptr, lists, 0, 1, c);
    } catch (const std::runtime_error &e) {
        return std::strstr(e.what(), what) != nullptr;
    }
    return false;
}

// |got - scale * table| <= units * 2^-52 * the largest |scale * table|
static bool close_to(const std::vector<double> &got, const int *table, size_t n, double scale, double units) {
    double big = 0.0, worst = 0.0;
    for (size_t k = 0; k < n; ++k) {
        big = std::fmax(big, std::fabs(scale * table[k]));
        worst = std::fmax(worst, std::fabs(got[k] - scale * table[k]));
    }
    std::printf("  worst %.3f units of 2^-52 (asserted %.2f)\n", worst / (big * EPS), units);
    return got.size() == n && worst <= units * EPS * big;
}

static const int TRI_K[36] = {6, 1, 1, -4, 0, -4, 1, 3, 0, -4, 0, 0, 1, 0, 3, 0, 0, -4, -4, -4, 0, 16, -8, 0, 0, 0, 0, -8, 16, -8,
                              -4, 0, -4, 0, -8, 16};
static const int TRI_M[36] = {6, -1, -1, 0, -4, 0, -1, 6, -1, 0, 0, -4, -1, -1, 6, -4, 0, 0, 0, 0, -4, 32, 16, 16, -4, 0, 0, 16, 32, 16,
                              0, -4, 0, 16, 16, 32};
static const int TET_K[100] = {9,  1,  1,  1,  -6, -6, -6, 2,  2,  2,  1,  3,  0,  0,  -4, 1,  1,  -1, -1, 0,  1,  0,  3,  0,  1,
                               -4, 1,  -1, 0,  -1, 1,  0,  0,  3,  1,  1,  -4, 0,  -1, -1, -6, -4, 1,  1,  24, 4,  4,  -8, -8, -8,
                               -6, 1,  -4, 1,  4,  24, 4,  -8, -8, -8, -6, 1,  1,  -4, 4,  4,  24, -8, -8, -8, 2,  -1, -1, 0,  -8,
                               -8, -8, 16, 4,  4,  2,  -1, 0,  -1, -8, -8, -8, 4,  16, 4,  2,  0,  -1, -1, -8, -8, -8, 4,  4,  16};
static const int TET_M[100] = {6,  1,  1,  1,  -4, -4, -4, -6, -6, -6, 1,  6,  1,  1,  -4, -6, -6, -4, -4, -6, 1,  1,  6,  1,  -6,
                               -4, -6, -4, -6, -4, 1,  1,  1,  6,  -6, -6, -4, -6, -4, -4, -4, -4, -6, -6, 32, 16, 16, 16, 16, 8,
                               -4, -6, -4, -6, 16, 32, 16, 16, 8,  16, -4, -6, -6, -4, 16, 16, 32, 8,  16, 16, -6, -4, -4, -6, 16,
                               16, 8,  32, 16, 16, -6, -4, -6, -4, 16, 8,  16, 16, 32, 16, -6, -6, -4, -4, 8,  16, 16, 16, 16, 32};

int main(int argc, char **argv) {
    std::vector<double> x(30, 0.0);
    std::vector<int> v(10);
    for (int k = 0; k < 10; ++k) v[(size_t)k] = k;
    // a call without elements passes the size checks of the two node counts, in all five calls
    const double one[2] = {1, 1};
    long long info[8];
    if (saamge_amd_element_matrices(10, 3, x.data(), 0, 10, nullptr, v.data(), 0, 1, one, nullptr, nullptr, nullptr, nullptr, info)) return 1;
    if (saamge_amd_element_matrices(10, 2, x.data(), 0, 6, nullptr, v.data(), 1, 2, one, nullptr, nullptr, nullptr, nullptr, info)) return 2;
    if (saamge_amd_element_mass(10, 3, x.data(), 0, 10, nullptr, v.data(), 3, one, nullptr, 0, nullptr, info)) return 3;
    if (saamge_amd_element_loads(10, 2, x.data(), 0, 6, nullptr, v.data(), 1, nullptr, x.data(), nullptr, nullptr, info)) return 4;
    if (saamge_amd_boundary_mass(10, 3, x.data(), 0, 10, nullptr, v.data(), 0, nullptr, nullptr, 1, nullptr, nullptr, nullptr, info)) return 5;
    if (saamge_amd_boundary_loads(10, 2, x.data(), 0, 6, nullptr, v.data(), 0, nullptr, nullptr, 1, nullptr, x.data(), nullptr, nullptr, info))
        return 6;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 7;
    if (!refused("nde = 10 nodes are no supported element type in 2D", 10, 2, x.data(), 1, 10, v.data())) return 8;
    if (!refused("nde = 5 nodes are no supported element type in 3D", 10, 3, x.data(), 1, 5, v.data())) return 9;
    if (!refused("nde = 7 nodes are no supported element type in 2D", 10, 2, x.data(), 1, 7, v.data())) return 10;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const double c[1] = {1.0};
        // the unit triangle: vertices, then the midpoints of (0,1), (1,2), (2,0)
        const double tri[12] = {0, 0, 1, 0, 0, 1, 0.5, 0, 0.5, 0.5, 0, 0.5};
        const ElementMatrices K2 = element_matrices(6, 2, tri, 1, 6, nullptr, v.data(), 0, 1, c);
        if (K2.info.order2 != 1 || K2.info.triangles != 0 || K2.info.doubles != 36 || K2.info.first_bad_element != -1) return 11;
        std::printf("tri6 stiffness\n");
        if (!close_to(K2.elmat, TRI_K, 36, 1.0 / 6.0, STIFF_UNITS)) return 12;
        std::vector<double> M2(36, 0.0), L2(6, 0.0);
        if (element_mass_into(6, 2, tri, 1, 6, nullptr, v.data(), 1, c, M2.data()).order2 != 1) return 13;
        std::printf("tri6 mass\n");
        if (!close_to(M2, TRI_M, 36, 0.5 / 180.0, MASS_UNITS)) return 14;
        const double ones[10] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
        element_loads_into(6, 2, tri, 1, 6, nullptr, v.data(), 1, nullptr, ones, L2.data());
        const int tri_l[6] = {0, 0, 0, 1, 1, 1};
        std::printf("tri6 loads\n");
        if (!close_to(L2, tri_l, 6, 0.5 / 3.0, MASS_UNITS)) return 15;
        // the unit tetrahedron: vertices, then the midpoints of (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)
        const double tet[30] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5, 0.5, 0.5, 0, 0.5, 0, 0.5, 0, 0.5, 0.5};
        const ElementMatrices K3 = element_matrices(10, 3, tet, 1, 10, nullptr, v.data(), 0, 1, c);
        if (K3.info.order2 != 1 || K3.info.tetrahedra != 0 || K3.info.doubles != 100) return 16;
        std::printf("tet10 stiffness\n");
        if (!close_to(K3.elmat, TET_K, 100, 1.0 / 30.0, STIFF_UNITS)) return 17;
        const double lm[2] = {1.0, 1.0};
        const ElementMatrices E3 = element_matrices(10, 3, tet, 1, 10, nullptr, v.data(), 1, 2, lm);
        if (E3.info.doubles != 900 || E3.elem_to_dof.size() != 30 || E3.dof_ptr[1] != 30 || E3.elem_to_dof[29] != 29) return 18;
        for (int r = 0; r < 30; ++r)
            for (int s = 0; s < 30; ++s)
                if (E3.elmat[(size_t)(r * 30 + s)] != E3.elmat[(size_t)(s * 30 + r)]) return 19;
        std::vector<double> M3(100, 0.0), L3(10, 0.0);
        if (element_mass_into(10, 3, tet, 1, 10, nullptr, v.data(), 1, c, M3.data()).order2 != 1) return 20;
        std::printf("tet10 mass\n");
        if (!close_to(M3, TET_M, 100, 1.0 / 6.0 / 420.0, MASS_UNITS)) return 21;
        element_loads_into(10, 3, tet, 1, 10, nullptr, v.data(), 1, nullptr, ones, L3.data());
        const int tet_l[10] = {-1, -1, -1, -1, 4, 4, 4, 4, 4, 4};
        std::printf("tet10 loads\n");
        if (!close_to(L3, tet_l, 10, 1.0 / 6.0 / 20.0, MASS_UNITS)) return 22;
        // local face 3 = nodes (0, 2, 1, 5, 7, 4), the side z = 0 of area 1/2: the triangle's mass table on those nodes
        const int fe[1] = {0}, f3[1] = {3}, f4[1] = {4};
        std::vector<double> F(100, 0.0);
        const BoundaryFormsInfo bi = boundary_mass_into(10, 3, tet, 1, 10, nullptr, v.data(), 1, fe, f3, 1, c, F.data());
        if (bi.triangles != 1 || bi.additions != 36 || bi.elements != 1 || bi.first_bad_face != -1) return 23;
        const int nodes[6] = {0, 2, 1, 5, 7, 4};
        int face_table[100] = {0};
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) face_table[nodes[a] * 10 + nodes[b]] = TRI_M[a * 6 + b];
        std::printf("tet10 face mass\n");
        if (!close_to(F, face_table, 100, 0.5 / 180.0, MASS_UNITS)) return 24;
        try {
            boundary_mass_into(10, 3, tet, 1, 10, nullptr, v.data(), 1, fe, f4, 1, c, F.data());
            return 25;
        } catch (const std::runtime_error &e) {
            if (!std::strstr(e.what(), "face 0: face_local is outside the element type's range")) return 26;
        }
    }
    std::printf("elmat p2 api test ok\n");
    return 0;
}
