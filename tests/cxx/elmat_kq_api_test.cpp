// TEST: saamge_amd::api::element_matrices_points_into and element_mass_points_into through libsaamge_amd.so.  Without an
// argument only the checks that need no GPU run: kind, ncoef, vdim, the NULL arguments and a node count that is no type are
// refused with the library's message, and a call without elements fills info.  With "gpu" the matrices of a 2 x 1 x 1 grid of
// sheared 8-node hexes with eight different coefficients each -- diffusion with a symmetric tensor per point, elasticity, the
// mass written and accumulated onto the diffusion matrices -- are computed and printed as hexadecimal floats.
#include <cstdio>
#include <cstring>
#include <utility>

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
    std::vector<double> x(24, 0.0), c(48, 1.0), out(576, 0.0);
    std::vector<int> v(8);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("kind must be 0", [&] { element_matrices_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, 1, c.data(), out.data()); }))
        return 1;
    if (!refused("ncoef must be 1, dim or", [&] { element_matrices_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 0, 2, c.data(), out.data()); }))
        return 2;
    if (!refused("ncoef must be 2", [&] { element_matrices_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, 6, c.data(), out.data()); }))
        return 3;
    if (!refused("null argument: coords, elem_to_vertex or coefq",
                 [&] { element_matrices_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 0, 6, nullptr, out.data()); }))
        return 4;
    if (!refused("nde = 5 nodes are no supported element type in 3D",
                 [&] { element_matrices_points_into(8, 3, x.data(), 1, 5, nullptr, v.data(), 0, 6, c.data(), out.data()); }))
        return 5;
    if (!refused("dim must be 2 or 3", [&] { element_matrices_points_into(8, 4, x.data(), 1, 8, nullptr, v.data(), 0, 1, c.data(), out.data()); }))
        return 6;
    if (!refused("vdim must be 1 or dim", [&] { element_mass_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, c.data(), out.data()); }))
        return 7;
    if (!refused("null argument: coefq", [&] { element_mass_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, nullptr, out.data()); }))
        return 8;
    if (!refused("null argument: coords or elem_to_vertex",
                 [&] { element_mass_points_into(8, 3, nullptr, 1, 8, nullptr, v.data(), 1, c.data(), out.data()); }))
        return 9;
    if (!refused("accumulate needs the matrices", [&] { element_mass_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, c.data(), nullptr, true); }))
        return 10;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_element_matrices_points(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, 1, c.data(), nullptr, out.data(), nullptr, nullptr, info))
        return 11;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 12;
    // no element: nothing touches the device, info is what a call without elements leaves
    const ElementMatricesInfo zi = element_matrices_points_into(8, 3, x.data(), 0, 8, nullptr, nullptr, 0, 6, nullptr, nullptr);
    if (zi.doubles != 0 || zi.hexahedra != 0 || zi.first_bad_element != -1) return 13;
    const ElementMatricesInfo zm = element_mass_points_into(8, 3, x.data(), 0, 8, nullptr, nullptr, 3, nullptr, nullptr);
    if (zm.doubles != 0 || zm.first_bad_element != -1) return 14;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2, NQ = 8 * NE;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> coords;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared: no element is a box
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                }
        // a different coefficient at every point: K_q symmetric (xx, yy, zz, xy, yz, xz), lambda_q / mu_q, sigma_q
        std::vector<double> kq, lm, sigma;
        for (int q = 0; q < NQ; ++q) {
            for (int d = 0; d < 3; ++d) kq.push_back(1.0 + 0.0625 * q + 0.25 * d);
            for (int d = 0; d < 3; ++d) kq.push_back(0.03125 * (q % 5) - 0.015625 * d);
            lm.push_back(2.0 - 0.03125 * q);
            lm.push_back(0.5 + 0.0625 * q);
            sigma.push_back(1.0 + 0.125 * q);
        }
        const ElementMatricesInfo sizes = element_matrices_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 0, 6, kq.data(), nullptr);
        if (sizes.doubles != 64 * NE || sizes.hexahedra != NE || sizes.order2 != 0 || sizes.first_bad_element != -1) return 15;
        std::vector<double> K((size_t)64 * NE, 0.0), E((size_t)576 * NE, 0.0), M((size_t)64 * NE, 0.0);
        std::vector<int> dptr((size_t)NE + 1, -1), dofs((size_t)24 * NE, -1);
        element_matrices_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 0, 6, kq.data(), K.data());
        const ElementMatricesInfo ei =
            element_matrices_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, 2, lm.data(), E.data(), dptr.data(), dofs.data());
        if (ei.doubles != 576 * NE) return 16;
        for (int e = 0; e <= NE; ++e)
            if (dptr[(size_t)e] != 24 * e) return 17;
        for (int k = 0; k < 8 * NE; ++k)
            for (int d = 0; d < 3; ++d)
                if (dofs[(size_t)(3 * k + d)] != 3 * e2v[(size_t)k] + d) return 18;
        element_mass_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, sigma.data(), M.data());
        std::vector<double> KM(K);
        element_mass_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, sigma.data(), KM.data(), true);
        // an inverted element is refused and named
        std::vector<int> bad(e2v);
        std::swap(bad[8], bad[10]);
        if (!refused("element 1: the Jacobian determinant is not positive",
                     [&] { element_matrices_points_into(NV, 3, coords.data(), NE, 8, nullptr, bad.data(), 0, 6, kq.data(), out.data()); }))
            return 19;
        print("diffusion", K);
        print("elasticity", E);
        print("mass", M);
        print("sum", KM);
    }
    std::printf("elmat kq api test ok\n");
    return 0;
}
