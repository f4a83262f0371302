// The face table of a mesh (mesh_faces.h): saamge_amd/mesh_model.py restated for gfx950.  Every output is an integer the mesh
// fixes uniquely, so nothing here depends on the order in which lanes run.
//
// A SLOT is (element, local face), s = slot_ptr[e] + lf; two slots match when their sorted corner vertex ids are equal.  The
// matching goes through the vertex -> element table (DESIGN.md 4.13 says why not through a sort):
//   mf_match_kernel   one lane per slot.  The lane reads the corners of its face (at most 4 ids, in registers), takes the
//                     smallest as the anchor and walks the elements at the anchor.  For a candidate it reads the candidate's
//                     CORNER nodes (at most 8) once and marks those that are corners of its own face: a bit mask over the
//                     candidate's corner nodes.  The candidate holds the face iff the mask has as many bits as the face has
//                     corners and equals the mask of one of the candidate's local faces (MF.face_mask, folded at compile time
//                     from elmat_types.h) -- no sort, no second walk of the candidate's faces through memory.  0 matches: a
//                     boundary face; 1: the neighbour; 2 or more: non-manifold, the element goes to an integer minimum.
//   mf_rows_kernel    one lane per element, twice (count, then fill after two scans over the elements, which is slot order):
//                     the boundary faces of the element in ascending local face, and its distinct neighbours sorted by a fixed
//                     network over its at most 6 slots.  No appended lists; the only atomics are integer counters and minima.
// The face-list calls (face_nodes, face_dofs) share the checks of the boundary forms (check_face_list, mesh.hip).
#include "mesh_faces.h"
#include "devtab.h"

#include <algorithm>
#include <climits>

#include "mesh.h"

namespace saamge_amd {

namespace {

typedef unsigned long long u64;

// ---- the tables of mesh_model.py, folded from FACE_NODES (elmat_types.h) ----------------------------------------------------
struct MfTables {
    int nfaces[EM_TYPES];
    int ncn[EM_TYPES];                             // corner nodes of the element type ...
    int corner_node[EM_TYPES][8];                  // ... and their local node ids
    int face_fn[EM_TYPES][BDR_MAX_FACES];          // nodes of the face
    int face_nc[EM_TYPES][BDR_MAX_FACES];          // corners of the face
    int face_corner[EM_TYPES][BDR_MAX_FACES][4];   // their local node ids
    int face_mask[EM_TYPES][BDR_MAX_FACES];        // the corners as bits over corner_node
    int face_node[EM_TYPES][BDR_MAX_FACES][9];
};
constexpr int mf_dim(int type) { return type == 0 || type == 1 || type == 5 || type == 7 ? 2 : 3; }
constexpr MfTables mf_tables() {
    MfTables t{};
    constexpr int NCN[EM_TYPES] = {3, 4, 4, 6, 8, 4, 8, 3, 4};
    for (int ty = 0; ty < EM_TYPES; ++ty) {
        t.nfaces[ty] = bdr_num_faces(ty);
        t.ncn[ty] = NCN[ty];
        for (int j = 0; j < NCN[ty]; ++j) t.corner_node[ty][j] = ty == 6 ? em_hex27_corner(j) : j;
        for (int lf = 0; lf < t.nfaces[ty]; ++lf) {
            const BdrFace f = bdr_face(ty, lf);
            const int fn = BDR_FACE_NODES[ty][lf];
            const int nc = mf_dim(ty) == 2 ? 2 : (fn == 3 || fn == 6 ? 3 : 4);
            t.face_fn[ty][lf] = fn;
            t.face_nc[ty][lf] = nc;
            for (int k = 0; k < fn; ++k) t.face_node[ty][lf][k] = f.node[k];
            for (int k = 0; k < nc; ++k) {
                const int node = mf_dim(ty) == 2 ? (k == 0 ? f.node[0] : f.node[fn - 1]) : f.node[k];
                t.face_corner[ty][lf][k] = node;
                for (int j = 0; j < NCN[ty]; ++j)
                    if (t.corner_node[ty][j] == node) t.face_mask[ty][lf] |= 1 << j;
            }
        }
    }
    return t;
}
constexpr bool mf_tables_ok() {      // every face corner is a corner node of its element type, and no two faces share a mask
    const MfTables t = mf_tables();
    for (int ty = 0; ty < EM_TYPES; ++ty)
        for (int lf = 0; lf < t.nfaces[ty]; ++lf) {
            int bits = 0;
            for (int j = 0; j < 8; ++j) bits += (t.face_mask[ty][lf] >> j) & 1;
            if (bits != t.face_nc[ty][lf]) return false;
            for (int l2 = 0; l2 < lf; ++l2)
                if (t.face_mask[ty][l2] == t.face_mask[ty][lf]) return false;
        }
    return true;
}
static_assert(mf_tables_ok(), "mesh_faces: the corner tables");
__device__ const MfTables MF = mf_tables();
constexpr MfTables MF_HOST = mf_tables();

// words of a build: [0] first element of no type / with a non-manifold face (minimum), [1] mixed-order pairs, [2] elements
// without a neighbour, [3] the largest number of elements at one vertex
constexpr int MF_WORDS = 4;

// what mesh_classify_kernel keeps per element: the number of its local faces
struct MfFaceCount {
    __device__ int operator()(int t, int) const { return t < 0 ? 0 : MF.nfaces[t]; }
};
// the maximum of cnt[0 .. n) into *out
__global__ __launch_bounds__(256) void mf_max_kernel(int n, const int *__restrict__ cnt, int *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) raise_max(out, cnt[i]);
}

// One lane per slot: lane t is local face t % stride of element t / stride (stride: the most faces an element of this mesh can
// have).  v2e_I / v2e_J: the elements at every vertex, in any order.
__global__ __launch_bounds__(256) void mf_match_kernel(long total, int stride, int dim, const int *__restrict__ eI,
                                                       const int *__restrict__ eJ, const int *__restrict__ v2e_I,
                                                       const int *__restrict__ v2e_J, const roff_t *__restrict__ slot_ptr,
                                                       int *__restrict__ nbr_elem, int *__restrict__ nbr_local,
                                                       int *__restrict__ words) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int e = (int)(t / stride), lf = (int)(t - (long)e * stride);
    const int b = eI[e], type = em_type_index(dim, eI[e + 1] - b);      // (the mesh has been classified: type >= 0)
    if (lf >= MF.nfaces[type]) return;
    const int nc = MF.face_nc[type][lf], fn = MF.face_fn[type][lf];
    int c[4] = {-1, -1, -1, -1};                                        // (no vertex id is -1)
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nc) c[k] = eJ[b + MF.face_corner[type][lf][k]];
    int anchor = c[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < nc) anchor = min(anchor, c[k]);
    int matches = 0, me = -1, ml = -1, mfn = 0;
    for (int p = v2e_I[anchor]; p < v2e_I[anchor + 1]; ++p) {
        const int ce = v2e_J[p];
        if (ce == e) continue;
        const int cb = eI[ce], ct = em_type_index(dim, eI[ce + 1] - cb);
        const int ncn = MF.ncn[ct];
        int mask = 0;
        for (int j = 0; j < ncn; ++j) {
            const int v = eJ[cb + MF.corner_node[ct][j]];
            mask |= (int)(v == c[0] || v == c[1] || v == c[2] || v == c[3]) << j;
        }
        if (__popc((unsigned)mask) != nc) continue;
        for (int f = 0; f < MF.nfaces[ct]; ++f)
            if (MF.face_mask[ct][f] == mask) {
                ++matches;
                me = ce;
                ml = f;
                mfn = MF.face_fn[ct][f];
            }
    }
    const roff_t slot = slot_ptr[e] + lf;
    nbr_elem[slot] = matches == 1 ? me : -1;
    nbr_local[slot] = matches == 1 ? ml : -1;
    if (matches > 1) atomicMin(words, e);
    if (matches == 1 && mfn != fn && e < me) atomicAdd(words + 1, 1);      // (once per pair; rare)
}

// One lane per element.  FILL false: the numbers of its boundary faces and of its distinct neighbours; FILL true: both lists at
// the offsets the scans gave.
template <bool FILL>
__global__ __launch_bounds__(256) void mf_rows_kernel(int NE, const roff_t *__restrict__ slot_ptr, const int *__restrict__ nbr_elem,
                                                      int *__restrict__ nbdr, int *__restrict__ nadj,
                                                      const roff_t *__restrict__ boff, const roff_t *__restrict__ xadj,
                                                      int *__restrict__ bdr_elem, int *__restrict__ bdr_local,
                                                      int *__restrict__ adj, int *__restrict__ words) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const roff_t s0 = slot_ptr[e];
    const int nf = (int)(slot_ptr[e + 1] - s0);
    int v[BDR_MAX_FACES];
    unsigned bm = 0;
#pragma unroll
    for (int k = 0; k < BDR_MAX_FACES; ++k) {
        const int n = k < nf ? nbr_elem[s0 + k] : INT_MAX;
        bm |= (unsigned)(n < 0) << k;
        v[k] = n < 0 ? INT_MAX : n;
    }
#pragma unroll
    for (int i = 0; i < BDR_MAX_FACES - 1; ++i)      // a fixed network: every index is a compile-time constant
#pragma unroll
        for (int k = 0; k < BDR_MAX_FACES - 1 - i; ++k) {
            const int lo = min(v[k], v[k + 1]), hi = max(v[k], v[k + 1]);
            v[k] = lo;
            v[k + 1] = hi;
        }
    if (!FILL) {
        int distinct = 0;
#pragma unroll
        for (int k = 0; k < BDR_MAX_FACES; ++k) distinct += (int)(v[k] != INT_MAX && (k == 0 || v[k] != v[k - 1]));
        nbdr[e] = __popc(bm);
        nadj[e] = distinct;
        if (distinct == 0) atomicAdd(words + 2, 1);
    } else {
        roff_t pb = boff[e], pa = xadj[e];
#pragma unroll
        for (int k = 0; k < BDR_MAX_FACES; ++k)
            if ((bm >> k) & 1u) {
                bdr_elem[pb] = (int)e;
                bdr_local[pb] = k;
                ++pb;
            }
#pragma unroll
        for (int k = 0; k < BDR_MAX_FACES; ++k)
            if (v[k] != INT_MAX && (k == 0 || v[k] != v[k - 1])) adj[pa++] = v[k];
    }
}

// ---- the face-list calls ------------------------------------------------------------------------------------------------------
// key[f] = type * 8 + local face (check_face_list)
__global__ __launch_bounds__(256) void mf_face_sizes_kernel(int NF, const int *__restrict__ key, int *__restrict__ fn) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f < NF) fn[f] = MF.face_fn[key[f] >> 3][key[f] & 7];
}
__global__ __launch_bounds__(256) void mf_face_nodes_kernel(int NF, const int *__restrict__ key, const int *__restrict__ fe,
                                                            const int *__restrict__ eI, const int *__restrict__ eJ,
                                                            const int *__restrict__ fptr, int *__restrict__ out) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int type = key[f] >> 3, lf = key[f] & 7, b = eI[fe[f]], fn = MF.face_fn[type][lf];
    for (int k = 0; k < fn; ++k) out[fptr[f] + k] = eJ[b + MF.face_node[type][lf][k]];
}
// One lane per face: flag into byte vdim * a + i of every node a of the face and every component i of comp_mask, by a 32-bit
// atomic OR on the word that holds the byte -- the other three bytes are ORed with 0, so no lane can change a neighbouring byte
// or another bit.  The word is the ALIGNED word around the byte's address: it lies in the byte's page, whatever the length of the
// array.  A byte changed iff the OR found a bit of flag missing, which exactly one lane sees; nodes: one bit per vertex, the
// lane that sets it counts the node.  counts: [0] distinct nodes, [1] bytes changed.
__global__ __launch_bounds__(256) void mf_face_dofs_kernel(int NF, const int *__restrict__ key, const int *__restrict__ fe,
                                                           const int *__restrict__ eI, const int *__restrict__ eJ, int vdim,
                                                           unsigned comp_mask, unsigned flag, signed char *bdr,
                                                           unsigned *__restrict__ nodes, u64 *__restrict__ counts) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int type = key[f] >> 3, lf = key[f] & 7, b = eI[fe[f]], fn = MF.face_fn[type][lf];
    int touched = 0, changed = 0;
    for (int k = 0; k < fn; ++k) {
        const int a = eJ[b + MF.face_node[type][lf][k]];
        const unsigned bit = 1u << (a & 31);
        if (!(atomicOr(nodes + (a >> 5), bit) & bit)) ++touched;
        for (int i = 0; i < vdim; ++i) {
            if (!((comp_mask >> i) & 1u)) continue;
            const uintptr_t addr = (uintptr_t)(bdr + ((long)vdim * a + i));
            const unsigned sh = 8u * (unsigned)(addr & 3u);
            const unsigned old = atomicOr((unsigned *)(addr & ~(uintptr_t)3), flag << sh);
            if (((old >> sh) & flag) != flag) ++changed;
        }
    }
    if (touched) atomicAdd(counts, (u64)touched);
    if (changed) atomicAdd(counts + 1, (u64)changed);
}

// ---- the mesh: on the device, checked, with the number of faces of every element (ClassifiedMesh::count) ----------------------
void mf_mesh(hipStream_t s, const std::string &name, const MeshArgs &m, ClassifiedMesh &M) {
    classified_mesh(s, name, m, M, MfFaceCount());
    M.stride = m.elem_ptr ? (m.dim == 2 ? 4 : BDR_MAX_FACES) : MF_HOST.nfaces[em_type_index(m.dim, m.nde)];      // the most faces
}

// what face_nodes and face_dofs share: the checks without a device of the mesh and of the face list
void mf_face_begin(const std::string &name, const MeshArgs &m, int NF, const int *face_elem, const int *face_local) {
    SA_REQUIRE(m.dim == 2 || m.dim == 3, name + "dim must be 2 or 3");
    SA_REQUIRE(NF >= 0, name + "NF < 0");
    SA_REQUIRE(NF == 0 || (face_elem && face_local), name + "null argument: face_elem or face_local");
    mesh_begin(name, m, nullptr);
    mesh_check_sizes(name, m, 0, NF > 0);      // (elem_to_vertex may be NULL when there is nothing to read)
}

}  // namespace

void face_table_build(hipStream_t s, const MeshArgs &m, FaceTable &T, long long info[8]) {
    const std::string name("saamge_amd_face_table_build: ");
    const int NV = m.NV, dim = m.dim, NE = m.NE;
    mesh_begin(name, m, info);
    mesh_check_sizes(name, m, 0, true);
    T.device = current_device();
    T.NE = NE;
    T.slot_ptr.alloc((size_t)NE + 1);
    T.xadj.alloc((size_t)NE + 1);
    if (NE == 0) {
        T.slot_ptr.zero(s);
        T.xadj.zero(s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    ClassifiedMesh M;
    mf_mesh(s, name, m, M);
    exclusive_scan_off(s, NE, M.count.p, T.slot_ptr.p);
    const roff_t slots = read_one((const roff_t *)T.slot_ptr.p + NE, s);
    // ---- the elements at every vertex
    DBuf<int> v2e_I((size_t)NV + 1), v2e_J((size_t)M.nconn), cnt((size_t)NV), words(MF_WORDS);
    const int init[MF_WORDS] = {INT_MAX, 0, 0, 0};
    upload_async(words.p, init, MF_WORDS, s);
    cnt.zero(s);
    dev_histogram(s, M.nconn, M.eJ, cnt.p);
    hipLaunchKernelGGL(mf_max_kernel, grid_flat(NV), dim3(256), 0, s, NV, (const int *)cnt.p, words.p + 3);
    SA_HIP_CHECK(hipGetLastError());
    dev_table_finish(s, NE, M.eI, M.eJ, NV, cnt.p, v2e_I.p, v2e_J.p, false);
    // ---- the matching
    T.nbr_elem.alloc((size_t)slots);
    T.nbr_local.alloc((size_t)slots);
    const long total = (long)NE * M.stride;
    hipLaunchKernelGGL(mf_match_kernel, grid_flat(total), dim3(256), 0, s, total, M.stride, dim, M.eI, M.eJ, (const int *)v2e_I.p,
                       (const int *)v2e_J.p, (const roff_t *)T.slot_ptr.p, T.nbr_elem.p, T.nbr_local.p, words.p);
    SA_HIP_CHECK(hipGetLastError());
    // ---- the boundary list and the graph rows: counts, scans over the elements, fill
    DBuf<int> nbdr((size_t)NE), nadj((size_t)NE);
    DBuf<roff_t> boff((size_t)NE + 1);
    hipLaunchKernelGGL(mf_rows_kernel<false>, grid_flat(NE), dim3(256), 0, s, NE, (const roff_t *)T.slot_ptr.p,
                       (const int *)T.nbr_elem.p, nbdr.p, nadj.p, (const roff_t *)nullptr, (const roff_t *)nullptr, (int *)nullptr,
                       (int *)nullptr, (int *)nullptr, words.p);
    SA_HIP_CHECK(hipGetLastError());
    int w[MF_WORDS];
    read_back(w, (const int *)words.p, MF_WORDS, s);
    if (info) {
        info[0] = (long long)slots;
        info[5] = w[3];
    }
    if (w[0] < NE) {
        if (info) info[6] = w[0];
        SA_REQUIRE(false, name + "element " + std::to_string(w[0]) + ": a face is shared by more than two elements");
    }
    exclusive_scan_off(s, NE, nbdr.p, boff.p);
    exclusive_scan_off(s, NE, nadj.p, T.xadj.p);
    T.NB = (long long)read_one((const roff_t *)boff.p + NE, s);
    T.nnz = (long long)read_one((const roff_t *)T.xadj.p + NE, s);
    SA_REQUIRE(T.NB <= INT_MAX, name + "more than 2^31 - 1 boundary faces");
    T.bdr_elem.alloc((size_t)T.NB);
    T.bdr_local.alloc((size_t)T.NB);
    T.adj.alloc((size_t)T.nnz);
    hipLaunchKernelGGL(mf_rows_kernel<true>, grid_flat(NE), dim3(256), 0, s, NE, (const roff_t *)T.slot_ptr.p,
                       (const int *)T.nbr_elem.p, (int *)nullptr, (int *)nullptr, (const roff_t *)boff.p, (const roff_t *)T.xadj.p,
                       T.bdr_elem.p, T.bdr_local.p, T.adj.p, (int *)nullptr);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
    if (info) {
        info[1] = ((long long)slots - T.NB) / 2;
        info[2] = T.NB;
        info[3] = T.nnz;
        info[4] = w[1];
        info[7] = w[2];
    }
}

void face_nodes(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int *face_ptr_out,
                int *face_nodes_out, long long *count_out) {
    const std::string name("saamge_amd_face_nodes: ");
    const int dim = m.dim, NE = m.NE;
    if (count_out) *count_out = 0;
    mf_face_begin(name, m, NF, face_elem, face_local);
    if (NF == 0) return;
    SA_REQUIRE(NE > 0, name + "face 0: face_elem is outside [0, NE)");
    ClassifiedMesh M;
    mf_mesh(s, name, m, M);
    FaceList L;
    check_face_list(s, name, dim, NE, M.eI, NF, face_elem, face_local, L, nullptr);
    DBuf<int> fn((size_t)NF), fptr((size_t)NF + 1);
    hipLaunchKernelGGL(mf_face_sizes_kernel, grid_flat(NF), dim3(256), 0, s, NF, (const int *)L.key.p, fn.p);
    SA_HIP_CHECK(hipGetLastError());
    exclusive_scan_int(s, NF, fn.p, fptr.p);      // (at most 9 NF: NF is a count of int-indexed entries)
    const int count = read_one((const int *)fptr.p + NF, s);
    if (count_out) *count_out = count;
    copy_to_caller(face_ptr_out, fptr, s);
    if (face_nodes_out) {
        DevOut<int> out(face_nodes_out, (size_t)count, s, false);
        hipLaunchKernelGGL(mf_face_nodes_kernel, grid_flat(NF), dim3(256), 0, s, NF, (const int *)L.key.p, L.fe, M.eI, M.eJ,
                           (const int *)fptr.p, out.p);
        SA_HIP_CHECK(hipGetLastError());
        out.finish();
    }
}

void face_dofs(hipStream_t s, const MeshArgs &m, int NF, const int *face_elem, const int *face_local, int vdim, unsigned comp_mask,
               int flag, signed char *bdr_dofs_inout, long long info[4]) {
    const std::string name("saamge_amd_face_dofs: ");
    const int NV = m.NV, dim = m.dim, NE = m.NE;
    if (info) {
        info[0] = info[1] = info[2] = 0;
        info[3] = -1;
    }
    mf_face_begin(name, m, NF, face_elem, face_local);
    SA_REQUIRE(vdim == 1 || vdim == dim, name + "vdim must be 1 or dim");
    SA_REQUIRE(comp_mask >= 1u && comp_mask < (1u << vdim), name + "comp_mask must lie in 1 .. 2^vdim - 1");
    SA_REQUIRE(flag >= 1 && flag <= 127, name + "flag must lie in 1 .. 127");
    SA_REQUIRE((int64_t)NV * vdim <= INT_MAX, name + "vdim * NV beyond 32 bits");
    SA_REQUIRE(NF == 0 || bdr_dofs_inout, name + "null argument: bdr_dofs_inout");
    if (NF == 0) return;
    if (NE == 0 && info) info[3] = 0;
    SA_REQUIRE(NE > 0, name + "face 0: face_elem is outside [0, NE)");
    ClassifiedMesh M;
    mf_mesh(s, name, m, M);
    FaceList L;
    check_face_list(s, name, dim, NE, M.eI, NF, face_elem, face_local, L, info ? info + 3 : nullptr);
    DevOut<signed char> bdr(bdr_dofs_inout, (size_t)NV * vdim, s, true);
    DBuf<unsigned> nodes(((size_t)NV + 31) / 32);
    DBuf<u64> counts(2);
    nodes.zero(s);
    counts.zero(s);
    hipLaunchKernelGGL(mf_face_dofs_kernel, grid_flat(NF), dim3(256), 0, s, NF, (const int *)L.key.p, L.fe, M.eI, M.eJ, vdim, comp_mask,
                       (unsigned)flag, bdr.p, nodes.p, counts.p);
    SA_HIP_CHECK(hipGetLastError());
    u64 c[2];
    read_back(c, (const u64 *)counts.p, 2, s);
    bdr.finish();
    if (info) {
        info[0] = NF;
        info[1] = (long long)c[0];
        info[2] = (long long)c[1];
    }
}

}  // namespace saamge_amd
