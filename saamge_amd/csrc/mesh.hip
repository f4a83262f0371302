// What every call on a mesh starts with (mesh.h): the checks without a device, the lists on the device, the refusal of an element
// of no type, the checks of a face list.
#include "mesh.h"

#include <algorithm>
#include <climits>
#include <utility>
#include <vector>

#include "partition.h"      // check_mesh_device

namespace saamge_amd {

namespace {

__global__ __launch_bounds__(256) void mesh_offsets_kernel(int NE, int nd, int *__restrict__ eI) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e <= NE) eI[e] = (int)(e * nd);
}

// The checks of the face list.  Face f with face_elem outside [0, NE) or face_local outside the range of the element's type:
// key[f] = -1 and f to the integer minimum words[0]; else key[f] = type * 8 + local face, and the face's bit is set in the byte
// of its element (mask: one byte per element, four to a word) -- a bit that was already set raises words[1].
__global__ __launch_bounds__(256) void bdr_check_kernel(int NF, int NE, int dim, const int *__restrict__ eI,
                                                        const int *__restrict__ face_elem, const int *__restrict__ face_local,
                                                        unsigned *__restrict__ mask, int *__restrict__ key, int *__restrict__ words) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int e = face_elem[f], lf = face_local[f];
    int k = -1;
    if (e >= 0 && e < NE) {
        const int t = em_type_index(dim, eI[e + 1] - eI[e]);      // (the mesh has been checked: t >= 0)
        if (t >= 0 && lf >= 0 && lf < bdr_num_faces(t)) {
            k = t * 8 + lf;
            const unsigned bit = 1u << (8 * (e & 3) + lf);
            if (atomicOr(mask + (e >> 2), bit) & bit) atomicOr(words + 1, 1);
        }
    }
    key[f] = k;
    if (k < 0) atomicMin(words, (int)f);
}
// the number of elements whose byte of the mask is not zero, added to *count
__global__ __launch_bounds__(256) void bdr_touched_kernel(int nwords, const unsigned *__restrict__ mask, int *__restrict__ count) {
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const unsigned m = mask[w];
    const int n = ((m & 0xffu) != 0) + ((m & 0xff00u) != 0) + ((m & 0xff0000u) != 0) + ((m & 0xff000000u) != 0);
    if (n) atomicAdd(count, n);
}

}  // namespace

void mesh_begin(const std::string &name, const MeshArgs &m, long long info[8]) {
    mesh_info_begin(info);
    SA_REQUIRE(m.dim == 2 || m.dim == 3, name + "dim must be 2 or 3");
    SA_REQUIRE(m.NV >= 0 && m.NE >= 0, name + "NV < 0 or NE < 0");
}

void mesh_check_sizes(const std::string &name, const MeshArgs &m, int comp, bool used, int wider, const char *limit) {
    SA_REQUIRE((int64_t)m.NV * comp <= INT_MAX, name + "dim * NV beyond 32 bits");
    SA_REQUIRE(!used || m.NE == 0 || m.elem_to_vertex, name + "null argument: elem_to_vertex");
    if (!m.elem_ptr) {
        SA_REQUIRE(em_type_index(m.dim, m.nde) >= 0, name + "nde = " + std::to_string(m.nde) +
                                                         " nodes are no supported element type in " + std::to_string(m.dim) + "D");
        SA_REQUIRE((int64_t)m.NE * std::max(m.nde, wider) * std::max(comp, 1) <= INT_MAX, name + limit);
    }
}

void import_mesh(hipStream_t s, const std::string &name, const MeshArgs &m, DeviceMesh &M) {
    const int NE = m.NE;
    // ---- the mesh: offsets first, they say how much of elem_to_vertex there is
    if (m.elem_ptr) {
        M.hold_I = DevIn<int>(m.elem_ptr, (size_t)NE + 1, s).take();
    } else {
        M.hold_I.alloc((size_t)NE + 1);
        hipLaunchKernelGGL(mesh_offsets_kernel, grid_flat((long)NE + 1), dim3(256), 0, s, NE, m.nde, M.hold_I.p);
        SA_HIP_CHECK(hipGetLastError());
    }
    M.eI = M.hold_I.p;
    M.eJ = m.elem_to_vertex;
    if (!is_device_ptr(m.elem_to_vertex)) {
        long total = (long)NE * m.nde;
        if (m.elem_ptr) {
            const hvec<int> hI = fetch_host(M.eI, (size_t)NE + 1, s);
            for (int e = 0; e < NE; ++e)
                SA_REQUIRE(hI[0] == 0 && hI[(size_t)e + 1] > hI[(size_t)e], name + "elem_ptr: must start at 0 and every element needs a vertex");
            total = hI[(size_t)NE];
        }
        upload(M.hold_J, m.elem_to_vertex, (size_t)total, s);
        M.eJ = M.hold_J.p;
    }
    M.nconn = check_mesh_device(s, NE, M.eI, M.eJ, m.NV);      // offsets, vertex ids in [0, NV), no vertex twice in an element
}

void refuse_element_type(hipStream_t s, const std::string &name, int dim, const int *eI, int e) {
    const int nd = read_one(eI + e + 1, s) - read_one(eI + e, s);
    throw Error(1, std::string(__FILE__) + ":" + std::to_string(__LINE__) + " " + name + "element " + std::to_string(e) + ": " +
                       std::to_string(nd) + " nodes are no supported element type in " + std::to_string(dim) + "D");
}

void check_face_list(hipStream_t s, const std::string &name, int dim, int NE, const int *eI, int NF, const int *face_elem,
                     const int *face_local, FaceList &L, long long *refused) {
    L.key.alloc((size_t)NF);
    DBuf<int> words(3);
    const int *fe = L.fe = L.in_fe.bind(face_elem, (size_t)NF, s);
    const int *fl = L.fl = L.in_fl.bind(face_local, (size_t)NF, s);
    const int nwords = (int)(((int64_t)NE + 3) / 4);
    DBuf<unsigned> mask((size_t)nwords);
    mask.zero(s);
    const int init[3] = {INT_MAX, 0, 0};
    upload_async(words.p, init, 3, s);
    hipLaunchKernelGGL(bdr_check_kernel, grid_flat(NF), dim3(256), 0, s, NF, NE, dim, eI, fe, fl, mask.p, L.key.p, words.p);
    SA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bdr_touched_kernel, grid_flat(nwords), dim3(256), 0, s, nwords, (const unsigned *)mask.p, words.p + 2);
    SA_HIP_CHECK(hipGetLastError());
    int w[3];
    read_back(w, (const int *)words.p, 3, s);
    if (w[0] < NF) {
        if (refused) *refused = w[0];
        const int e = read_one(fe + w[0], s);
        SA_REQUIRE(false, name + "face " + std::to_string(w[0]) + ": " +
                              (e < 0 || e >= NE ? "face_elem is outside [0, NE)" : "face_local is outside the element type's range"));
    }
    if (w[1]) {      // a pair is listed twice: the first face of the list that is one of a repeated pair, found on the host
        const hvec<int> he = fetch_host(fe, (size_t)NF, s), hl = fetch_host(fl, (size_t)NF, s);
        std::vector<std::pair<int64_t, int>> pairs((size_t)NF);
        for (int f = 0; f < NF; ++f) pairs[(size_t)f] = {(int64_t)he[(size_t)f] * 8 + hl[(size_t)f], f};
        std::sort(pairs.begin(), pairs.end());
        int first = NF;
        for (size_t k = 0; k + 1 < pairs.size(); ++k)
            if (pairs[k].first == pairs[k + 1].first && (k == 0 || pairs[k - 1].first != pairs[k].first)) first = std::min(first, pairs[k].second);
        if (refused) *refused = first;
        SA_REQUIRE(false, name + "face " + std::to_string(first) + ": the same (element, local face) is listed twice");
    }
    L.touched = w[2];
}

}  // namespace saamge_amd
