// The mesh argument of the element layer (elmat.hip) and the mesh layer (mesh_faces.hip, mesh_lift.hip, mesh_refine.hip), and what
// every call does with it before its own work (mesh.hip): the checks that need no device, the lists brought to the device and
// checked, the type of every element, the refusal of an element of no type, the checks of a face list.
#pragma once
#include "common.h"

#include <string>

#include "elmat_types.h"
#include "mesh_helpers.h"

namespace saamge_amd {

// The mesh arguments every entry point of the C ABI starts with (include/saamge_amd.h): NV vertices with dim coordinates each
// (coords NULL where the call takes none), NE elements of nde nodes each or, elem_ptr not NULL, with the offsets elem_ptr into
// elem_to_vertex.  Host or device pointers.
struct MeshArgs {
    int NV, dim;
    const double *coords;
    int NE, nde;
    const int *elem_ptr, *elem_to_vertex;
};

// ---- the checks that need no device, in the order every entry point has had them ------------------------------------------------
// info (8 words, may be NULL) as a call without elements leaves it ...
inline void mesh_info_begin(long long info[8]) {
    if (!info) return;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[6] = -1;
}
// ... that, the dimension and the counts ...
void mesh_begin(const std::string &name, const MeshArgs &m, long long info[8]);
// ... and the sizes.  comp: dofs per node in the 32-bit limits (0: the call has no dofs); used: elem_to_vertex is read, NULL is
// refused; wider: an element's list grows to that many entries (the lift), with `limit` the text of its refusal.
void mesh_check_sizes(const std::string &name, const MeshArgs &m, int comp, bool used, int wider = 0,
                      const char *limit = "NE * nde beyond 32 bits");

// A mesh argument brought to the device and checked.  elem_ptr NULL: NE elements of nde nodes each.  Host arrays are uploaded (the
// offsets first: they say how much of elem_to_vertex there is), device arrays are used where they are.  Refused with `name` in
// front or by check_mesh_device: malformed offsets, a vertex id outside [0, NV) -- before any kernel reads through the ids --, a
// vertex listed twice in an element.  NE > 0.
struct DeviceMesh {
    DBuf<int> hold_I, hold_J;
    const int *eI = nullptr, *eJ = nullptr;      // NE + 1 offsets, the flat vertex lists
    long nconn = 0;                              // eI[NE]
};
void import_mesh(hipStream_t s, const std::string &name, const MeshArgs &m, DeviceMesh &M);

// ---- the type of every element ------------------------------------------------------------------------------------------------------
// One lane per element: count[e] = store(type index, e) -- what the caller keeps per element; store may write more of its own --
// and the first element of no type (index < 0) goes to the integer minimum *first.
template <class F>
__global__ __launch_bounds__(256) void mesh_classify_kernel(int NE, int dim, const int *__restrict__ eI, int *__restrict__ count,
                                                            int *__restrict__ first, F store) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int t = em_type_index(dim, eI[e + 1] - eI[e]);
    count[e] = store(t, (int)e);
    if (t < 0) atomicMin(first, (int)e);
}
template <class F>
void mesh_classify(hipStream_t s, int NE, int dim, const int *eI, int *count, int *first, F store) {
    hipLaunchKernelGGL(mesh_classify_kernel<F>, grid_flat(NE), dim3(256), 0, s, NE, dim, eI, count, first, store);
    SA_HIP_CHECK(hipGetLastError());
}
// the refusal of element e, which has no type: throws "element e: N nodes are no supported element type in dD"
[[noreturn]] void refuse_element_type(hipStream_t s, const std::string &name, int dim, const int *eI, int e);

// The mesh on the device, checked and classified: count[e] = store(type, e) of every element; an element of no type is refused.
// stride is the caller's: the most lanes an element of this mesh needs in its kernels.
struct ClassifiedMesh : DeviceMesh {
    DBuf<int> count;
    int stride = 0;
};
template <class F>
void classified_mesh(hipStream_t s, const std::string &name, const MeshArgs &m, ClassifiedMesh &M, F store) {
    import_mesh(s, name, m, M);
    M.count.alloc((size_t)m.NE);
    DBuf<int> word(1);
    SA_HIP_CHECK(hipMemsetAsync(word.p, 0x7f, sizeof(int), s));
    mesh_classify(s, m.NE, m.dim, M.eI, M.count.p, word.p, store);
    const int first = read_one((const int *)word.p, s);
    if (first < m.NE) refuse_element_type(s, name, m.dim, M.eI, first);
}

// raise the maximum word *out to c (*out only grows: a stale read costs an atomic, never the result)
__device__ inline void raise_max(int *out, int c) {
    if (c > *(volatile int *)out) atomicMax(out, c);
}

// The checks of a face list, shared by the boundary forms and the face-list calls of mesh_faces.hip.  The mesh (NE > 0
// elements, offsets eI on the device) has been checked.  Refused with `name` in front: the first face (lowest index) with
// face_elem outside [0, NE) or face_local outside the range of the element's type, then the first face whose (element, local
// face) the list holds more than once; *refused (may be NULL) gets that index.  face_elem / face_local: host or device pointers.
struct FaceList {
    DevIn<int> in_fe, in_fl;
    DBuf<int> key;                        // key[f] = type * 8 + local face (em_type_index)
    const int *fe = nullptr, *fl = nullptr;      // the lists on the device
    int touched = 0;                      // distinct elements of the list
};
void check_face_list(hipStream_t s, const std::string &name, int dim, int NE, const int *eI, int NF, const int *face_elem,
                     const int *face_local, FaceList &L, long long *refused);

}  // namespace saamge_amd
