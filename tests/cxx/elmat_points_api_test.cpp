// TEST: saamge_amd::api::element_points_into, element_eval_into, element_loads_points_into and element_errors_into through
// libsaamge_amd.so.  Without an argument only the checks that need no GPU run: vdim = 2 in 3D and the NULL mesh arguments are
// refused with the library's message, and a call without elements fills info and qp_ptr[0].  With "gpu" the points of a
// 2 x 1 x 1 grid of sheared 8-node hexes, a nodal field and its gradient there, the loads of a source given at the points and
// the squared errors are computed and printed as hexadecimal floats.
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
    std::vector<double> x(24, 0.0), f(24, 1.0), out(576, 0.0);
    std::vector<int> v(8);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("vdim must be 1 or dim", [&] { element_eval_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, f.data(), out.data(), nullptr); }))
        return 1;
    if (!refused("vdim must be 1 or dim",
                 [&] { element_loads_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, nullptr, f.data(), out.data()); }))
        return 2;
    if (!refused("vdim must be 1 or dim",
                 [&] { element_errors_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, f.data(), nullptr, nullptr, out.data()); }))
        return 3;
    if (!refused("null argument: coords or elem_to_vertex",
                 [&] { element_points_into(8, 3, nullptr, 1, 8, nullptr, v.data(), nullptr, out.data(), nullptr); }))
        return 4;
    if (!refused("nde = 5 nodes are no supported element type in 3D",
                 [&] { element_points_into(8, 3, x.data(), 1, 5, nullptr, v.data(), nullptr, out.data(), nullptr); }))
        return 5;
    if (!refused("dim must be 2 or 3", [&] { element_points_into(8, 4, x.data(), 1, 8, nullptr, v.data(), nullptr, out.data(), nullptr); }))
        return 6;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_element_eval(8, 3, x.data(), 1, 8, nullptr, v.data(), 2, f.data(), nullptr, out.data(), nullptr, info)) return 7;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 8;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2, NQ = 8 * NE;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> coords, u3;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared: no element is a box
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                    for (int d = 0; d < 3; ++d) u3.push_back(0.5 * d + 0.125 * i * j - 0.0625 * k);
                }
        std::vector<double> sigma;
        for (int e = 0; e < NE; ++e) sigma.push_back(1.0 + 0.125 * e);
        // a call without elements: info and qp_ptr[0]
        long long none = 7;
        const ElementMatricesInfo zi = element_points_into(NV, 3, coords.data(), 0, 8, nullptr, nullptr, &none, nullptr, nullptr);
        if (none != 0 || zi.doubles != 0 || zi.hexahedra != 0 || zi.first_bad_element != -1) return 9;
        std::vector<long long> qp((size_t)NE + 1, -1);
        std::vector<double> xq((size_t)NQ * 3, 0.0), wdet((size_t)NQ, 0.0), uq((size_t)NQ * 3, 0.0), gq((size_t)NQ * 9, 0.0);
        std::vector<double> b3((size_t)24 * NE, 0.0), err((size_t)2 * NE, 0.0);
        const ElementMatricesInfo pi = element_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), qp.data(), xq.data(), wdet.data());
        if (pi.doubles != NQ || pi.hexahedra != NE || pi.order2 != 0 || pi.first_bad_element != -1) return 10;
        for (int e = 0; e <= NE; ++e)
            if (qp[(size_t)e] != 8 * e) return 11;
        const ElementMatricesInfo sizes = element_eval_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, u3.data(), nullptr, nullptr);
        if (sizes.doubles != NQ || sizes.hexahedra != NE) return 12;
        element_eval_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, u3.data(), uq.data(), gq.data());
        // the source at the points is the field there; the exact data the coordinates of the points
        element_loads_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, sigma.data(), uq.data(), b3.data());
        element_errors_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), 3, u3.data(), xq.data(), nullptr, err.data());
        if (err[1] != 0.0 || err[3] != 0.0) return 13;
        // an inverted element is refused and nothing is written
        std::vector<int> bad(e2v);
        std::swap(bad[8], bad[10]);
        std::vector<double> keep(xq);
        if (!refused("element 1: the Jacobian determinant is not positive",
                     [&] { element_points_into(NV, 3, coords.data(), NE, 8, nullptr, bad.data(), qp.data(), keep.data(), nullptr); }))
            return 14;
        if (keep != xq) return 15;
        print("xq", xq);
        print("wdet", wdet);
        print("uq", uq);
        print("gradq", gq);
        print("loads3", b3);
        print("errors", err);
    }
    std::printf("elmat points api test ok\n");
    return 0;
}
