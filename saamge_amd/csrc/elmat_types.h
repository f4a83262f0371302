// The element types and their local faces (elmat_model.py: ALL_TYPE_INDEX, FACE_NODES), folded at compile time: shared by the
// element layer (elmat.hip) and the mesh layer (mesh_faces.hip, mesh_lift.hip, mesh_refine.hip).
#pragma once

namespace saamge_amd {

constexpr int EM_HEX_LOC[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
constexpr int EM2_QUAD_LOC[9][2] = {{0, 0}, {2, 0}, {2, 2}, {0, 2}, {1, 0}, {2, 1}, {1, 2}, {0, 1}, {1, 1}};
// the 27-node hexahedron is lexicographic: the node at reference position (x, y, z) in {0, 1, 2}^3; corner j is HEX_LOC[j] doubled
constexpr int em_hex27_node(int x, int y, int z) { return (z * 3 + y) * 3 + x; }
constexpr int em_hex27_corner(int j) { return em_hex27_node(2 * EM_HEX_LOC[j][0], 2 * EM_HEX_LOC[j][1], 2 * EM_HEX_LOC[j][2]); }

// types 0 .. 4: order 1 (info[0 .. 4]); 5, 6: the order-2 quadrilateral and hexahedron; 7, 8: the order-2 triangle (6 nodes)
// and tetrahedron (10 nodes); info[7] counts all four
constexpr int EM_TYPES = 9;
constexpr int em_type_index(int dim, int nd) {
    return dim == 2 ? (nd == 3 ? 0 : (nd == 4 ? 1 : (nd == 9 ? 5 : (nd == 6 ? 7 : -1))))
                    : (nd == 4 ? 2 : (nd == 6 ? 3 : (nd == 8 ? 4 : (nd == 27 ? 6 : (nd == 10 ? 8 : -1)))));
}
constexpr int EM_TYPE_ND[EM_TYPES] = {3, 4, 4, 6, 8, 9, 27, 6, 10};

constexpr int BDR_MAX_FACES = 6;
struct BdrFace {
    int node[9];
};
// elmat_model.FACE_NODES, by the type index of em_type_index
constexpr int bdr_num_faces(int type) { return type == 0 || type == 7 ? 3 : (type == 3 ? 5 : (type == 4 || type == 6 ? 6 : 4)); }
constexpr int BDR_FACE_NODES[EM_TYPES][BDR_MAX_FACES] = {{2, 2, 2, 0, 0, 0}, {2, 2, 2, 2, 0, 0}, {3, 3, 3, 3, 0, 0}, {3, 3, 4, 4, 4, 0},
                                                          {4, 4, 4, 4, 4, 4}, {3, 3, 3, 3, 0, 0}, {9, 9, 9, 9, 9, 9}, {3, 3, 3, 0, 0, 0},
                                                          {6, 6, 6, 6, 0, 0}};
constexpr int BDR_HEX_FACES[6][4] = {{3, 2, 1, 0}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}, {4, 5, 6, 7}};
constexpr BdrFace bdr_face(int type, int lf) {
    constexpr int TRI[3][2] = {{0, 1}, {1, 2}, {2, 0}};
    constexpr int QUAD[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}};
    constexpr int QUAD9[4][3] = {{0, 4, 1}, {1, 5, 2}, {2, 6, 3}, {3, 7, 0}};
    constexpr int TET[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
    constexpr int WEDGE[5][4] = {{0, 2, 1, 0}, {3, 4, 5, 0}, {0, 1, 4, 3}, {1, 2, 5, 4}, {2, 0, 3, 5}};
    constexpr int TRI6[3][3] = {{0, 3, 1}, {1, 4, 2}, {2, 5, 0}};
    constexpr int TET10[4][6] = {{1, 2, 3, 7, 9, 8}, {0, 3, 2, 6, 9, 5}, {0, 1, 3, 4, 8, 6}, {0, 2, 1, 5, 7, 4}};
    BdrFace f{};
    const int fn = BDR_FACE_NODES[type][lf];
    for (int k = 0; k < fn; ++k) {
        if (type == 0) f.node[k] = TRI[lf][k];
        else if (type == 1) f.node[k] = QUAD[lf][k];
        else if (type == 2) f.node[k] = TET[lf][k];
        else if (type == 3) f.node[k] = WEDGE[lf][k];
        else if (type == 4) f.node[k] = BDR_HEX_FACES[lf][k];
        else if (type == 5) f.node[k] = QUAD9[lf][k];
        else if (type == 7) f.node[k] = TRI6[lf][k];
        else if (type == 8) f.node[k] = TET10[lf][k];
        else {      // the node at face position (u, v) of Q2_QUAD_LOC: P(c0) + u (P(c1) - P(c0)) / 2 + v (P(c3) - P(c0)) / 2
            const int *c = BDR_HEX_FACES[lf];
            int p[3] = {0, 0, 0};
            for (int d = 0; d < 3; ++d)
                p[d] = 2 * EM_HEX_LOC[c[0]][d] + EM2_QUAD_LOC[k][0] * (EM_HEX_LOC[c[1]][d] - EM_HEX_LOC[c[0]][d]) +
                       EM2_QUAD_LOC[k][1] * (EM_HEX_LOC[c[3]][d] - EM_HEX_LOC[c[0]][d]);
            f.node[k] = em_hex27_node(p[0], p[1], p[2]);
        }
    }
    return f;
}

}  // namespace saamge_amd
