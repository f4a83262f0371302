// The faces of a mesh on the device (mesh_faces.hip): which element lies across each local face, the boundary faces, the
// element graph through faces, and the nodes / essential-dof flags of a list of faces.  saamge_amd/mesh_model.py defines every
// integer and the kernels give the same.
#pragma once
#include "common.h"
#include "mesh.h"

namespace saamge_amd {

struct FaceTable {
    int device = 0;
    int NE = 0;
    long long NB = 0, nnz = 0;
    DBuf<roff_t> slot_ptr, xadj;                  // NE + 1 each
    DBuf<int> nbr_elem, nbr_local;                // one per slot
    DBuf<int> bdr_elem, bdr_local;                // NB
    DBuf<int> adj;                                // nnz
};

// The arguments of saamge_amd_face_table_build.  The checks that need no device run before the first HIP call; the vertex ids
// are checked before any kernel reads through them.  Runs on s and returns with s idle.
void face_table_build(hipStream_t s, const MeshArgs &m, FaceTable &T, long long info[8]);
// The arguments of saamge_amd_face_nodes; outputs host or device pointers, NULL: the count only.
void face_nodes(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int *face_ptr_out,
                int *face_nodes_out, long long *count_out);
// The arguments of saamge_amd_face_dofs; bdr_dofs_inout a host or device pointer of vdim * NV bytes.
void face_dofs(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, unsigned comp_mask,
               int flag, signed char *bdr_dofs_inout, long long info[4]);

}  // namespace saamge_amd
