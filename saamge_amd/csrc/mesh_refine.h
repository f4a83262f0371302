// An order-1 mesh refined uniformly on the device (mesh_refine.hip): every triangle and quadrilateral becomes 4, every
// tetrahedron and hexahedron 8 elements of its own type, `levels` times, with the vertex -> vertex interpolation between two
// levels where asked for.  saamge_amd/mesh_refine_model.py defines every integer and every coordinate bit and the kernels give
// the same.
//
// GUARANTEED numbering: child k of element e is element nc * e + k of the next level (nc = 4 in 2D, 8 in 3D), so the parent of
// element c is c / nc and its ancestor s levels up is c >> (2 s) in 2D, c >> (3 s) in 3D.  The descendants of one element are a
// connected agglomerate of the refined mesh: the nested partitions the setup takes are arange(NE) >> (2 s | 3 s), without a call.
// The vertices of level j keep their ids in level j + 1 (hierarchical numbering); after them come the edges, the quadrilateral
// faces of hexahedra and the centres of level j, in the order of the lift (mesh_lift.h).
#pragma once
#include "common.h"
#include "mesh.h"

namespace saamge_amd {

constexpr int MESH_REFINE_MAX_LEVELS = 15;      // 3 * 4^16 entries are beyond 32 bits already

struct MeshRefineLevel {      // level j of [0, levels]; level `levels` was not lifted: its NEd .. nnz are -1
    long long NV = 0, NE = 0, entries = 0, NEd = -1, NFq = -1, NC = -1, max_owned = -1, nnz = -1;      // nnz of P_j; 0: not kept
};
struct MeshInterp {           // P_j: one row per vertex of level j + 1, one column per vertex of level j
    int nrows = 0, ncols = 0;
    long long nnz = 0;
    DBuf<int> rowptr, col;
    DBuf<double> val;
};
struct MeshRefine {
    int device = 0;
    int dim = 0, levels = 0, NV = 0, NE = 0;
    long long entries = 0;
    DBuf<double> coords;                          // NV x dim, empty without coords
    DBuf<int> elem_ptr;                           // NE + 1
    DBuf<int> elem_to_vertex;                     // entries
    std::vector<MeshRefineLevel> level;           // levels + 1
    std::vector<MeshInterp> P;                    // levels with want_interp, else none
};

// The arguments of saamge_amd_mesh_refine.  Every level is lifted by mesh_lift_order2, with its checks; the lifted node list
// of a level is released before the next level is lifted.  Runs on s and returns with s idle.
void mesh_refine(hipStream_t s, const MeshArgs &m, int levels, int want_interp, MeshRefine &R, long long info[8]);

}  // namespace saamge_amd
