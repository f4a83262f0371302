// TEST: saamge_amd::api::FaceTable, face_nodes and face_dofs_into through libsaamge_amd.so.
// Without an argument only the checks that need no GPU run: dim = 4, a NULL vertex list and comp_mask = 0 are refused with the
// library's message, and an empty face list is a no-op.  With "gpu" the table of a 2 x 1 x 1 grid of 8-node hexes, the nodes of
// one face and the flags of that face are printed as integers.
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

int main(int argc, char **argv) {
    std::vector<int> v(8), fe(1, 0), fl(1, 0);
    std::vector<signed char> flags(8, 4);
    for (int k = 0; k < 8; ++k) v[(size_t)k] = k;
    if (!refused("dim must be 2 or 3", [&] { FaceTable t(8, 4, 1, 8, nullptr, v.data()); })) return 1;
    if (!refused("null argument: elem_to_vertex", [&] { FaceTable t(8, 3, 1, 8, nullptr, nullptr); })) return 2;
    if (!refused("comp_mask", [&] { face_dofs_into(8, 3, 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, 0u, flags.data()); }))
        return 3;
    if (!refused("dim must be 2 or 3", [&] { face_nodes(8, 4, 1, 8, nullptr, v.data(), 1, fe.data(), fl.data()); })) return 4;
    if (!refused("flag must lie in 1 .. 127",
                 [&] { face_dofs_into(8, 3, 1, 8, nullptr, v.data(), 1, fe.data(), fl.data(), 1, 1u, flags.data(), 128); }))
        return 5;
    if (!refused("nodes are no supported element type", [&] { FaceTable t(8, 3, 1, 5, nullptr, v.data()); })) return 6;
    const FaceDofsInfo none = face_dofs_into(8, 3, 1, 8, nullptr, v.data(), 0, nullptr, nullptr, 1, 1u, flags.data());
    if (none.faces != 0 || none.nodes != 0 || none.changed != 0 || none.first_bad_face != -1) return 7;
    const FaceNodes empty = face_nodes(8, 3, 1, 8, nullptr, v.data(), 0, nullptr, nullptr);
    if (empty.face_ptr.size() != 1 || empty.face_ptr[0] != 0 || !empty.nodes.empty()) return 8;
    for (size_t k = 0; k < flags.size(); ++k)
        if (flags[k] != 4) return 9;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    saamge_amd_face_table *h = nullptr;
    if (!saamge_amd_face_table_build(8, 4, 1, 8, nullptr, v.data(), nullptr, &h, info) || h) return 10;
    if (info[0] != 0 || info[6] != -1 || info[7] != 0) return 11;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 2, gx = nx + 1, NE = nx, NV = gx * 2 * 2;
        static const int LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        std::vector<int> e2v;
        for (int e = 0; e < nx; ++e)
            for (int a = 0; a < 8; ++a) e2v.push_back((LOC[a][2] * 2 + LOC[a][1]) * gx + e + LOC[a][0]);
        FaceTable first(NV, 3, NE, 8, nullptr, e2v.data());
        FaceTable t(std::move(first));                           // the handle moves; `first` frees nothing
        if (first.handle() || !t.handle() || t.elements() != NE) return 12;
        const FaceTableInfo &fi = t.info();
        if (fi.slots != 12 || fi.pairs != 1 || fi.boundary_faces != 10 || fi.graph_entries != 2 || fi.mixed_pairs != 0 ||
            fi.max_valence != 2 || fi.first_bad_element != -1 || fi.isolated_elements != 0)
            return 13;
        std::vector<long long> slot_ptr, xadj;
        std::vector<int> nbr_elem, nbr_local, bdr_elem, bdr_local, adj;
        t.get(slot_ptr, nbr_elem, nbr_local, bdr_elem, bdr_local, xadj, adj);
        print("slot_ptr", slot_ptr);
        print("nbr_elem", nbr_elem);
        print("nbr_local", nbr_local);
        print("bdr_elem", bdr_elem);
        print("bdr_local", bdr_local);
        print("xadj", xadj);
        print("adj", adj);
        // the side x = 0: local face 4 of element 0, taken from the table's own device arrays through a one-face host list
        const int face_elem[1] = {0}, face_local[1] = {4};
        const FaceNodes fn = face_nodes(NV, 3, NE, 8, nullptr, e2v.data(), 1, face_elem, face_local);
        print("face_ptr", fn.face_ptr);
        print("face_nodes", fn.nodes);
        std::vector<signed char> bdr((size_t)3 * NV, 1);
        const FaceDofsInfo di = face_dofs_into(NV, 3, NE, 8, nullptr, e2v.data(), 1, face_elem, face_local, 3, 5u, bdr.data());
        if (di.faces != 1 || di.nodes != 4 || di.changed != 8 || di.first_bad_face != -1) return 14;
        print("flags", bdr);
        // every boundary face, straight from the handle's device pointers
        std::vector<signed char> all((size_t)NV, 0);
        const FaceDofsInfo ai = face_dofs_into(NV, 3, NE, 8, nullptr, e2v.data(), (int)t.boundary_faces(), t.bdr_elem(), t.bdr_local(), 1,
                                               1u, all.data());
        if (ai.faces != 10 || ai.nodes != NV || ai.changed != NV) return 15;
        print("all_flags", all);
    }
    std::printf("mesh faces api test ok\n");
    return 0;
}
