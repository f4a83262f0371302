// TEST: saamge_amd::api::MeshRefine through libsaamge_amd.so.
// Without an argument only the checks that need no GPU run: levels = 0 and levels above the cap, dim = 4, a NULL vertex list and
// a node count that is no type are refused with the library's message, and a refusal leaves the handle argument untouched.  With
// "gpu" a sheared 2 x 1 x 1 grid of 8-node hexes refined twice is printed: the integers, the coordinates and the values of the
// interpolations as bits.
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

template <class T>
static void print(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (size_t k = 0; k < v.size(); ++k) std::printf(" %lld", (long long)v[k]);
    std::printf("\n");
}
static void print_bits(const char *tag, const std::vector<double> &v) {
    std::printf("%s", tag);
    for (size_t k = 0; k < v.size(); ++k) {
        long long bits;
        std::memcpy(&bits, &v[k], sizeof(bits));
        std::printf(" %lld", bits);
    }
    std::printf("\n");
}

int main(int argc, char **argv) {
    std::vector<int> v(8);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("levels must be at least 1", [&] { MeshRefine m(8, 3, nullptr, 1, 8, nullptr, v.data(), 0); })) return 1;
    if (!refused("levels above 15", [&] { MeshRefine m(8, 3, nullptr, 1, 8, nullptr, v.data(), 16); })) return 2;
    if (!refused("dim must be 2 or 3", [&] { MeshRefine m(8, 4, nullptr, 1, 8, nullptr, v.data()); })) return 3;
    if (!refused("null argument: elem_to_vertex", [&] { MeshRefine m(8, 3, nullptr, 1, 8, nullptr, nullptr); })) return 4;
    if (!refused("nodes are no supported element type", [&] { MeshRefine m(8, 3, nullptr, 1, 5, nullptr, v.data(), 2, true); })) return 5;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    int sentinel = 0;
    saamge_amd_refined_mesh *h = (saamge_amd_refined_mesh *)&sentinel;
    if (!saamge_amd_mesh_refine(8, 3, nullptr, 1, 8, nullptr, v.data(), 0, 1, nullptr, &h, info)) return 6;
    if (h != (saamge_amd_refined_mesh *)&sentinel) return 7;      // a refusal leaves *out untouched
    for (int k = 0; k < 8; ++k)
        if (info[k] != (k == 6 ? -1 : 0)) return 8;
    if (!saamge_amd_mesh_refine(8, 3, nullptr, 1, 8, nullptr, v.data(), 1, 0, nullptr, nullptr, info)) return 9;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        std::vector<double> X;
        for (int k = 0; k < NV; ++k) {      // a sheared grid: no coordinate is a round number
            const int i = k % gx, j = (k / gx) % 2, l = k / (2 * gx);
            X.push_back(i / 3.0 + 0.1 * j);
            X.push_back(j / 7.0 + 0.1 * l);
            X.push_back(l / 11.0 + 0.1 * i);
        }
        MeshRefine first(NV, 3, X.data(), NE, 8, nullptr, e2v.data(), 2, true);
        MeshRefine m(std::move(first));                            // the handle moves; `first` frees nothing
        if (first.handle() || !m.handle() || m.elements() != 64 * NE || m.levels() != 2) return 10;
        const MeshRefineInfo &ri = m.info();
        if (ri.vertices != 9 * 5 * 5 || ri.elements != 128 || ri.entries != 1024 || ri.levels != 2 || ri.max_owned_edges != 4 ||
            ri.first_bad_element != -1 || ri.unlisted_vertices != 0 || m.vertices() != 225)
            return 11;
        if (!m.coords() || !m.elem_ptr() || !m.elem_to_vertex()) return 12;
        const MeshRefineLevelInfo l0 = m.level_info(0), l1 = m.level_info(1), l2 = m.level_info(2);
        if (l0.vertices != 12 || l0.elements != 2 || l0.edges != 20 || l0.face_nodes != 11 || l0.centre_nodes != 2) return 13;
        if (l1.vertices != 45 || l1.elements != 16 || l1.entries != 128 || l2.vertices != 225 || l2.edges != -1) return 14;
        if (ri.interp_nnz != l0.interp_nnz + l1.interp_nnz || l0.interp_nnz != 12 + 2 * 20 + 4 * 11 + 8 * 2) return 15;
        if (!refused("outside [0, levels]", [&] { m.level_info(3); })) return 16;
        if (!refused("outside [0, levels)", [&] { m.interp(2); })) return 17;
        std::vector<double> coords;
        std::vector<int> elem_ptr, elem_to_vertex;
        m.get(coords, elem_ptr, elem_to_vertex);
        print_bits("coords", coords);
        print("elem_ptr", elem_ptr);
        print("elem_to_vertex", elem_to_vertex);
        for (int j = 0; j < 2; ++j) {
            const MeshInterp P = m.interp(j);
            if (P.nrows != (j ? 225 : 45) || P.ncols != (j ? 45 : 12)) return 18;
            print(j ? "rowptr1" : "rowptr0", P.rowptr);
            print(j ? "col1" : "col0", P.col);
            print_bits(j ? "val1" : "val0", P.val);
        }
        // without coordinates and interpolations; one level twice through the handle's own device arrays
        MeshRefine once(NV, 3, nullptr, NE, 8, nullptr, e2v.data());
        if (once.coords() || once.vertices() != 45 || once.info().interp_nnz != 0) return 19;
        if (!refused("without want_interp", [&] { once.interp(0); })) return 20;
        MeshRefine twice(once.vertices(), 3, nullptr, once.elements(), 0, once.elem_ptr(), once.elem_to_vertex());
        std::vector<int> elem_to_vertex_twice;
        twice.get(coords, elem_ptr, elem_to_vertex_twice);
        if (!coords.empty() || elem_to_vertex_twice != elem_to_vertex) return 21;
        // the face table of the refined mesh, from the handle's device arrays
        FaceTable t(m.vertices(), 3, m.elements(), 0, m.elem_ptr(), m.elem_to_vertex());
        if (t.info().slots != 6 * 128 || t.info().boundary_faces != 16 * 10) return 22;
        m = std::move(once);
        if (once.handle() || m.coords() || m.vertices() != 45) return 23;
    }
    std::printf("mesh refine api test ok\n");
    return 0;
}
