// TEST: saamge_amd::api::MeshLift through libsaamge_amd.so.
// Without an argument only the checks that need no GPU run: dim = 4, a NULL vertex list and a node count that is no type are
// refused with the library's message, and a refusal leaves the handle argument untouched.  With "gpu" the lift of a 2 x 1 x 1 grid
// of 8-node hexes -- with the face table built inside, then handed in -- is printed: the integers, and the coordinates as bits.
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
    if (!refused("dim must be 2 or 3", [&] { MeshLift m(8, 4, nullptr, 1, 8, nullptr, v.data()); })) return 1;
    if (!refused("null argument: elem_to_vertex", [&] { MeshLift m(8, 3, nullptr, 1, 8, nullptr, nullptr); })) return 2;
    if (!refused("nodes are no supported element type", [&] { MeshLift m(8, 3, nullptr, 1, 5, nullptr, v.data()); })) return 3;
    if (!refused("NV < 0 or NE < 0", [&] { MeshLift m(8, 3, nullptr, -1, 8, nullptr, v.data()); })) return 4;
    long long info[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    int sentinel = 0;
    saamge_amd_mesh_lift *h = (saamge_amd_mesh_lift *)&sentinel;
    if (!saamge_amd_mesh_lift_order2(8, 4, nullptr, 1, 8, nullptr, v.data(), nullptr, nullptr, &h, info)) return 5;
    if (h != (saamge_amd_mesh_lift *)&sentinel) return 6;      // a refusal leaves *out untouched
    if (info[0] != 0 || info[6] != -1 || info[7] != 0) return 7;
    if (!saamge_amd_mesh_lift_order2(8, 3, nullptr, 1, 8, nullptr, v.data(), nullptr, nullptr, nullptr, info)) return 8;
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
        MeshLift first(NV, 3, X.data(), NE, 8, nullptr, e2v.data());
        MeshLift m(std::move(first));                            // the handle moves; `first` frees nothing
        if (first.handle() || !m.handle() || m.elements() != NE) return 9;
        const MeshLiftInfo &li = m.info();
        if (li.nodes != 45 || li.edges != 20 || li.face_nodes != 11 || li.centre_nodes != 2 || li.entries != 54 ||
            li.max_owned_edges != 3 || li.first_bad_element != -1 || li.unlisted_vertices != 0 || m.nodes() != 45)
            return 10;
        if (!m.coords2() || !m.elem_ptr2() || !m.elem_to_node() || !m.edge_ptr() || !m.edge_hi() || !m.face_slot()) return 11;
        std::vector<double> coords2;
        std::vector<int> elem_ptr2, elem_to_node, edge_hi;
        std::vector<long long> edge_ptr, face_slot;
        m.get(coords2, elem_ptr2, elem_to_node, edge_ptr, edge_hi, face_slot);
        print_bits("coords2", coords2);
        print("elem_ptr2", elem_ptr2);
        print("elem_to_node", elem_to_node);
        print("edge_ptr", edge_ptr);
        print("edge_hi", edge_hi);
        print("face_slot", face_slot);
        // the same with the face table handed in, and without coordinates
        FaceTable t(NV, 3, NE, 8, nullptr, e2v.data());
        MeshLift again(NV, 3, nullptr, NE, 8, nullptr, e2v.data(), &t);
        if (again.coords2() || again.nodes() != 45) return 12;
        std::vector<int> elem_to_node_again;
        again.get(coords2, elem_ptr2, elem_to_node_again, edge_ptr, edge_hi, face_slot);
        if (!coords2.empty() || elem_to_node_again != elem_to_node) return 13;
        // the face table of the lifted mesh, from the handle's device arrays
        FaceTable t2(m.nodes(), 3, NE, 0, m.elem_ptr2(), m.elem_to_node());
        if (t2.info().slots != 12 || t2.info().pairs != 1 || t2.info().boundary_faces != 10) return 14;
        m = std::move(again);
        if (again.handle() || m.coords2()) return 15;
    }
    std::printf("mesh lift api test ok\n");
    return 0;
}
