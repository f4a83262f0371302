// TEST: saamge_amd::api::element_matrices through libsaamge_amd.so.  Without an argument only the checks that need no GPU run;
// with "gpu" the diffusion and elasticity matrices of a 3 x 2 x 2 grid of Q1 hexes with sheared vertices and per-element
// coefficients are computed and printed as hexadecimal floats, with the dof lists they are indexed by.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

static bool refused(const char *what, int NV, int dim, const double *coords, int NE, int nde, const int *lists, int kind, int ncoef,
                    const double *coef) {
    try {
        element_matrices(NV, dim, coords, NE, nde, nullptr, lists, kind, ncoef, coef);
    } catch (const std::runtime_error &e) {
        return std::strstr(e.what(), what) != nullptr;
    }
    return false;
}

int main(int argc, char **argv) {
    const double x[24] = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1};
    const int v[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const double c[6] = {1, 1, 1, 0, 0, 0};
    if (!refused("dim must be 2 or 3", 8, 4, x, 1, 8, v, 0, 1, c)) return 1;
    if (!refused("kind must be 0", 8, 3, x, 1, 8, v, 2, 1, c)) return 2;
    if (!refused("ncoef must be 1, dim or", 8, 3, x, 1, 8, v, 0, 2, c)) return 3;
    if (!refused("ncoef must be 2", 8, 3, x, 1, 8, v, 1, 3, c)) return 4;
    if (!refused("null argument", 8, 3, nullptr, 1, 8, v, 0, 1, c)) return 5;
    if (!refused("null argument", 8, 3, x, 1, 8, nullptr, 0, 1, c)) return 6;
    if (!refused("null argument", 8, 3, x, 1, 8, v, 0, 1, nullptr)) return 7;
    if (!refused("nde = 5 nodes are no supported element type in 3D", 8, 3, x, 1, 5, v, 0, 1, c)) return 8;
    if (!refused("nde = 8 nodes are no supported element type in 2D", 8, 2, x, 1, 8, v, 0, 1, c)) return 9;
    if (!refused("NE < 0", 8, 3, x, -1, 8, v, 0, 1, c)) return 10;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_element_matrices(8, 3, x, 1, 8, nullptr, v, 0, 2, c, nullptr, nullptr, nullptr, nullptr, info)) return 11;
    if (info[5] != 0 || info[6] != -1) return 12;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 3, ny = 2, nz = 2, vx = nx + 1, vy = ny + 1, vz = nz + 1, NE = nx * ny * nz, NV = vx * vy * vz;
        std::vector<int> e2v;
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y)
                for (int xx = 0; xx < nx; ++xx)
                    for (int k = 0; k < 8; ++k) {
                        const int a = (k == 1 || k == 2 || k == 5 || k == 6), b = (k == 2 || k == 3 || k == 6 || k == 7), cc = k >> 2;
                        e2v.push_back(((z + cc) * vy + y + b) * vx + xx + a);
                    }
        std::vector<double> coords;
        for (int k = 0; k < vz; ++k)
            for (int j = 0; j < vy; ++j)
                for (int i = 0; i < vx; ++i) {      // a sheared grid: every hex a different parallelepiped-like cell
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
        const ElementMatrices D = element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 0, 6, k6.data());
        const ElementMatrices E = element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, 2, lm.data());
        if (D.info.hexahedra != NE || D.info.doubles != 64 * NE || D.info.first_bad_element != -1 || D.elmat.size() != (size_t)64 * NE) return 13;
        if (E.info.doubles != 576 * NE || E.elem_to_dof.size() != (size_t)24 * NE || E.dof_ptr[(size_t)NE] != 24 * NE) return 14;
        const ElementMatricesInfo sizes = element_matrices_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, 2, lm.data(), nullptr);
        if (sizes.doubles != 576 * NE) return 15;
        std::printf("diffusion");
        for (size_t k = 0; k < D.elmat.size(); ++k) std::printf(" %a", D.elmat[k]);
        std::printf("\nelasticity");
        for (size_t k = 0; k < E.elmat.size(); ++k) std::printf(" %a", E.elmat[k]);
        std::printf("\ndofs");
        for (size_t k = 0; k < E.elem_to_dof.size(); ++k) std::printf(" %d", E.elem_to_dof[k]);
        std::printf("\n");
        std::swap(e2v[8 * 5], e2v[8 * 5 + 1]);      // element 5 inverted
        try {
            element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 0, 6, k6.data());
            return 16;
        } catch (const std::runtime_error &e) {
            if (!std::strstr(e.what(), "element 5: the Jacobian determinant is not positive")) return 17;
        }
    }
    std::printf("elmat api test ok\n");
    return 0;
}
