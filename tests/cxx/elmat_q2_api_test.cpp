// TEST: the order-2 types of saamge_amd::api::element_matrices through libsaamge_amd.so.  Without an argument only the checks
// that need no GPU run: a 9-node element in 3D and a 27-node element in 2D are refused with the library's message.  With "gpu"
// the diffusion and elasticity matrices of a 2 x 1 x 1 grid of sheared 27-node hexes with per-element coefficients are computed
// and printed as hexadecimal floats, and the order-2 count is checked.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

static bool refused(const char *what, int NV, int dim, const double *coords, int NE, int nde, const int *lists) {
    const double c[2] = {1, 1};
    try {
        element_matrices(NV, dim, coords, NE, nde, nullptr, lists, 0, 1, c);
    } catch (const std::runtime_error &e) {
        return std::strstr(e.what(), what) != nullptr;
    }
    return false;
}

int main(int argc, char **argv) {
    std::vector<double> x(81, 0.0);
    std::vector<int> v(27);
    for (int k = 0; k < 27; ++k) v[(size_t)k] = k;
    if (!refused("nde = 9 nodes are no supported element type in 3D", 27, 3, x.data(), 1, 9, v.data())) return 1;
    if (!refused("nde = 27 nodes are no supported element type in 2D", 27, 2, x.data(), 1, 27, v.data())) return 2;
    if (!refused("nde = 18 nodes are no supported element type in 2D", 27, 2, x.data(), 1, 18, v.data())) return 3;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    const double c[1] = {1};
    if (!saamge_amd_element_matrices(27, 3, x.data(), 1, 9, nullptr, v.data(), 0, 1, c, nullptr, nullptr, nullptr, nullptr, info)) return 4;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 5;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = 2 * nx + 1, gy = 3, gz = 3, NE = nx, NV = gx * gy * gz;
        std::vector<int> e2n;
        for (int e = 0; e < nx; ++e)
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i) e2n.push_back((k * gy + j) * gx + 2 * e + i);
        std::vector<double> coords;
        for (int k = 0; k < gz; ++k)
            for (int j = 0; j < gy; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared and bent: the elements are curved
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                }
        std::vector<double> k6, lm;
        for (int e = 0; e < NE; ++e) {
            const double d[6] = {1.0 + 0.0625 * e, 1.5, 2.0 - 0.03125 * e, 0.125, -0.0625, 0.25};
            k6.insert(k6.end(), d, d + 6);
            lm.push_back(1.0 + 0.125 * e);
            lm.push_back(0.5 + 0.0625 * e);
        }
        const ElementMatrices D = element_matrices(NV, 3, coords.data(), NE, 27, nullptr, e2n.data(), 0, 6, k6.data());
        const ElementMatrices E = element_matrices(NV, 3, coords.data(), NE, 27, nullptr, e2n.data(), 1, 2, lm.data());
        if (D.info.order2 != NE || D.info.hexahedra != 0 || D.info.doubles != 729 * NE || D.info.first_bad_element != -1) return 6;
        if (E.info.order2 != NE || E.info.doubles != 6561 * NE || E.elem_to_dof.size() != (size_t)81 * NE || E.dof_ptr[(size_t)NE] != 81 * NE)
            return 7;
        const ElementMatricesInfo sizes = element_matrices_into(NV, 3, coords.data(), NE, 27, nullptr, e2n.data(), 1, 2, lm.data(), nullptr);
        if (sizes.doubles != 6561 * NE || sizes.order2 != NE) return 8;
        std::printf("diffusion");
        for (size_t k = 0; k < D.elmat.size(); ++k) std::printf(" %a", D.elmat[k]);
        std::printf("\nelasticity");
        for (size_t k = 0; k < E.elmat.size(); ++k) std::printf(" %a", E.elmat[k]);
        std::printf("\ndofs");
        for (size_t k = 0; k < E.elem_to_dof.size(); ++k) std::printf(" %d", E.elem_to_dof[k]);
        std::printf("\n");
    }
    std::printf("elmat q2 api test ok\n");
    return 0;
}
