// TEST: saamge_amd::api::boundary_points_into, boundary_eval_into, boundary_mass_points_into and boundary_loads_points_into through
// libsaamge_amd.so.  Without an argument only the checks that need no GPU run: vdim = 2 in 3D, a NULL u, coefq or gq, NULL face
// lists and NF < 0 are refused with the library's message, and an empty face list is a no-op.  With "gpu" three faces of a
// 2 x 1 x 1 grid of sheared 8-node hexes (two of element 0, one of element 1, not in ascending order) give their points, normals,
// a trace and a gradient, and are added with point data to zero matrices and vectors; everything is printed as hexadecimal floats.
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
    std::vector<double> x(24, 0.0), c(4, 1.0), g(24, 1.0), out(576, 0.0);
    std::vector<int> v(8), fe(1, 0), fl(1, 0);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("vdim must be 1 or dim", [&] {
            boundary_eval_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, g.data(), out.data(), nullptr);
        }))
        return 1;
    if (!refused("vdim must be 1 or dim", [&] {
            boundary_mass_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, c.data(), out.data());
        }))
        return 2;
    if (!refused("vdim must be 1 or dim", [&] {
            boundary_loads_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, nullptr, c.data(), out.data());
        }))
        return 3;
    if (!refused("null argument: u", [&] {
            boundary_eval_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, nullptr, out.data(), nullptr);
        }))
        return 4;
    if (!refused("null argument: coefq", [&] {
            boundary_mass_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, nullptr, out.data());
        }))
        return 5;
    if (!refused("null argument: gq", [&] {
            boundary_loads_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, nullptr, nullptr, out.data());
        }))
        return 6;
    if (!refused("null argument: face_elem or face_local", [&] {
            boundary_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), nullptr, nullptr, out.data(), nullptr, nullptr);
        }))
        return 7;
    if (!refused("NF < 0", [&] {
            boundary_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), -1, fe.data(), fl.data(), nullptr, out.data(), nullptr, nullptr);
        }))
        return 8;
    const BoundaryFormsInfo none =
        boundary_points_into(8, 3, x.data(), 1, 8, nullptr, v.data(), 0, nullptr, nullptr, nullptr, out.data(), nullptr, nullptr);
    if (none.additions != 0 || none.first_bad_face != -1 || none.elements != 0 || none.quadrilaterals4 != 0) return 9;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    if (!saamge_amd_boundary_loads_points(8, 3, x.data(), 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 2, nullptr, c.data(), nullptr,
                                          out.data(), info))
        return 10;
    if (info[5] != 0 || info[6] != -1 || info[7] != 0) return 11;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2, NF = 3, NFQ = 4 * NF;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> coords, u3;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < gx; ++i) {      // sheared: no face is a rectangle
                    coords.push_back(0.25 * i + 0.03125 * j * k);
                    coords.push_back(0.5 * j + 0.015625 * i * k);
                    coords.push_back(0.5 * k + 0.0078125 * i * j);
                    for (int d = 0; d < 3; ++d) u3.push_back(0.5 * d + 0.125 * i * j - 0.0625 * k + 0.25 * i * k);
                }
        const int face_elem[NF] = {0, 1, 0}, face_local[NF] = {4, 2, 0};      // element 0: its faces 4 and 0, listed 4 first
        std::vector<long long> fp((size_t)NF + 1, -1);
        std::vector<double> xq((size_t)NFQ * 3), wmeas((size_t)NFQ), normal((size_t)NFQ * 3), uq((size_t)NFQ * 3), gradq((size_t)NFQ * 9);
        const BoundaryFormsInfo sizes = boundary_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local,
                                                             nullptr, nullptr, nullptr, nullptr);
        if (sizes.quadrilaterals4 != NF || sizes.additions != NFQ || sizes.first_bad_face != -1 || sizes.elements != 2) return 12;
        boundary_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, fp.data(), xq.data(), wmeas.data(),
                             normal.data());
        for (int f = 0; f <= NF; ++f)
            if (fp[(size_t)f] != 4 * f) return 13;
        const BoundaryFormsInfo ei = boundary_eval_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 3,
                                                        u3.data(), uq.data(), gradq.data());
        if (ei.additions != NFQ) return 14;
        std::vector<double> coefq, K((size_t)64 * NE, 0.0), b3((size_t)24 * NE, 0.0);
        for (int q = 0; q < NFQ; ++q) coefq.push_back(1.0 + 0.0625 * q);
        const BoundaryFormsInfo mi = boundary_mass_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 1,
                                                               coefq.data(), K.data());
        if (mi.additions != 16 * NF) return 15;
        boundary_loads_points_into(NV, 3, coords.data(), NE, 8, nullptr, e2v.data(), NF, face_elem, face_local, 3, nullptr, uq.data(),
                                   b3.data());
        print("xq", xq);
        print("wmeas", wmeas);
        print("normal", normal);
        print("uq", uq);
        print("gradq", gradq);
        print("mass_points", K);
        print("loads_points", b3);
    }
    std::printf("bdr points api test ok\n");
    return 0;
}
