// TEST: saamge_amd::api::element_mass_into, element_loads_into and AssembledOperator::assemble_rhs through libsaamge_amd.so.
// Without an argument only the checks that need no GPU run: vdim = 2 in 3D and a NULL src are refused with the library's
// message.  With "gpu" the mass matrices of a 2 x 1 x 1 grid of sheared 8-node hexes (scalar, and the vector form added to
// the elasticity matrices), the load vectors and the assembled right-hand side are computed and printed as hexadecimal floats.
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
    std::vector<double> x(24, 0.0), c(1, 1.0), f(24, 1.0), out(576, 0.0);
    std::vector<int> v(8);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("vdim must be 1 or dim", [&] { element_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, c.data(), out.data()); }))
        return 1;
    if (!refused("vdim must be 1 or dim",
                 [&] { element_loads_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, c.data(), f.data(), out.data()); }))
        return 2;
    if (!refused("null argument: src",
                 [&] { element_loads_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, nullptr, nullptr, out.data()); }))
        return 3;
    if (!refused("null argument: coef", [&] { element_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, nullptr, out.data()); }))
        return 4;
    if (!refused("accumulate", [&] { element_mass_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, c.data(), nullptr, true); }))
        return 5;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_element_mass(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, c.data(), nullptr, 0, out.data(), info)) return 6;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 7;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> coords, src1, src3;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared: no element is a box
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                    src1.push_back(1.0 + 0.125 * i - 0.25 * j + 0.5 * k);
                    for (int d = 0; d < 3; ++d) src3.push_back(0.5 * d + 0.125 * i * j - 0.0625 * k);
                }
        std::vector<double> sigma, lm;
        for (int e = 0; e < NE; ++e) {
            sigma.push_back(1.0 + 0.125 * e);
            lm.push_back(1.0 + 0.125 * e);
            lm.push_back(0.5 + 0.0625 * e);
        }
        std::vector<double> M((size_t)64 * NE, 0.0), b1((size_t)8 * NE, 0.0), b3((size_t)24 * NE, 0.0), rhs((size_t)NV, 0.0);
        const ElementMatricesInfo sizes = element_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, sigma.data(), nullptr);
        if (sizes.doubles != 576 * NE || sizes.hexahedra != NE || sizes.first_bad_element != -1) return 8;
        const ElementMatricesInfo mi = element_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, sigma.data(), M.data());
        if (mi.doubles != 64 * NE || mi.hexahedra != NE || mi.order2 != 0) return 9;
        ElementMatrices E = element_matrices(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, 2, lm.data());
        element_mass_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, sigma.data(), E.elmat.data(), true);
        const ElementMatricesInfo li = element_loads_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 1, sigma.data(), src1.data(), b1.data());
        if (li.doubles != 8 * NE) return 10;
        element_loads_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, nullptr, src3.data(), b3.data());
        const AssembledOperator op(NV, NE, 8, nullptr, e2v.data(), M.data(), nullptr);
        op.assemble_rhs(b1.data(), rhs.data());
        print("mass", M);
        print("elasticity_plus_mass", E.elmat);
        print("loads1", b1);
        print("loads3", b3);
        print("rhs", rhs);
    }
    std::printf("mass api test ok\n");
    return 0;
}
