// TEST: saamge_amd::api::boundary_mass_into and boundary_loads_into through libsaamge_amd.so.
// Without an argument only the checks that need no GPU run: vdim = 2 in 3D, a NULL g, a NULL coef for the mass and NF < 0 are
// refused with the library's message, and an empty face list is a no-op.  With "gpu" three faces of a 2 x 1 x 1 grid of sheared
// 8-node hexes (two of element 0, one of element 1, not in ascending order) are added to the diffusion matrices, to the
// elasticity matrices (vector form) and to the load vectors, which are printed as hexadecimal floats.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

template <class F>
static bool refused(const char *what, F call) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return std::strstr(e.what(), what) != nullptr;
    }
    return false;
}

static void print(const char *tag, const std::vector<double> &v) {
    std::printf("%s", tag);
    for (size_t k = 0; k < v.size(); ++k) std::printf(" %a", v[k]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    std::vector<double> x(24, 0.0), c(1, 1.0), g(24, 1.0), out(576, 0.0);
    std::vector<int> v(8), fe(1, 0), fl(1, 0);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("vdim must be 1 or dim",
                 [&] { boundary_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, c.data(), out.data()); }))
        return 1;
    if (!refused("vdim must be 1 or dim", [&] {
            boundary_loads_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, c.data(), g.data(), out.data());
        }))
        return 2;
    if (!refused("null argument: g", [&] {
            boundary_loads_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, nullptr, nullptr, out.data());
        }))
        return 3;
    if (!refused("null argument: coef",
                 [&] { boundary_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, nullptr, out.data()); }))
        return 4;
    if (!refused("NF < 0",
                 [&] { boundary_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), -1, fe.data(), fl.data(), 1, c.data(), out.data()); }))
        return 5;
    const BoundaryFormsInfo none = boundary_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 0, nullptr, nullptr, 1, nullptr, out.data());
    if (none.additions != 0 || none.first_bad_face != -1 || none.elements != 0 || none.quadrilaterals4 != 0) return 6;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_boundary_loads(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, nullptr, g.data(), nullptr,
                                   out.data(), info))
        return 7;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 8;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2, NF = 3;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> coords, g1, g3;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared: no face is a rectangle
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                    g1.push_back(1.0 + 0.125 * i - 0.25 * j + 0.5 * k);
                    for (int d = 0; d < 3; ++d) g3.push_back(0.5 * d + 0.125 * i * j - 0.0625 * k);
                }
        const int face_elem[NF] = {0, 1, 0}, face_local[NF] = {4, 2, 0};      // element 0: its faces 4 and 0, listed 4 first
        const double alpha[NF] = {1.0, 1.25, 1.5};
        std::vector<double> one((size_t)NE, 1.0), lm;
        for (int e = 0; e < NE; ++e) {
            lm.push_back(1.0 + 0.125 * e);
            lm.push_back(0.5 + 0.0625 * e);
        }
        const BoundaryFormsInfo sizes = boundary_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 3,
                                                           alpha, nullptr);
        if (sizes.quadrilaterals4 != NF || sizes.additions != 3 * 16 * NF || sizes.first_bad_face != -1 || sizes.elements != 2) return 9;
        ElementMatrices K = element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 0, 1, one.data());
        const BoundaryFormsInfo mi = boundary_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 1,
                                                        alpha, K.elmat.data());
        if (mi.additions != 16 * NF || mi.triangles != 0) return 10;
        ElementMatrices E = element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, 2, lm.data());
        boundary_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 3, alpha, E.elmat.data());
        std::vector<double> b1((size_t)8 * NE, 0.0), b3((size_t)24 * NE, 0.0);
        element_loads_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, nullptr, g1.data(), b1.data());
        const BoundaryFormsInfo li = boundary_loads_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 1,
                                                         alpha, g1.data(), b1.data());
        if (li.additions != 4 * NF) return 11;
        boundary_loads_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 3, nullptr, g3.data(), b3.data());
        print("diffusion_plus_robin", K.elmat);
        print("elasticity_plus_robin", E.elmat);
        print("loads1", b1);
        print("loads3", b3);
    }
    std::printf("bdr forms api test ok\n");
    return 0;
}
