// An order-1 mesh lifted to order 2 on the device (mesh_lift.hip): the edges of the mesh, the node lists of the 6-node triangle,
// 9-node quadrilateral, 10-node tetrahedron and 27-node hexahedron on the same elements, and the coordinates of all nodes.
// saamge_amd/mesh_lift_model.py defines every integer and every coordinate bit and the kernels give the same.
#pragma once
#include "common.h"
#include "mesh_faces.h"

namespace saamge_amd {

struct MeshLift {
    int device = 0;
    int NV = 0, NE = 0, dim = 0, NV2 = 0;
    long long NEd = 0, NFq = 0, NC = 0, entries = 0;
    DBuf<double> coords2;                         // NV2 x dim, empty without coords
    DBuf<int> elem_ptr2;                          // NE + 1
    DBuf<int> elem_to_node;                       // entries
    DBuf<roff_t> edge_ptr;                        // NV + 1
    DBuf<int> edge_hi;                            // NEd
    DBuf<roff_t> face_slot;                       // NFq
};

// The arguments of saamge_amd_mesh_lift_order2; faces NULL: the face table is built inside where the mesh has a hexahedron.
// The checks that need no device run before the first HIP call; the vertex ids are checked before any kernel reads through
// them.  Runs on s and returns with s idle.
void mesh_lift_order2(hipStream_t s, const MeshArgs &m, const FaceTable *faces, MeshLift &L, long long info[8]);

}  // namespace saamge_amd
