// An order-1 mesh lifted to order 2 (mesh_lift.h): saamge_amd/mesh_lift_model.py restated for gfx950.  Every output is an
// integer the mesh fixes uniquely, or a coordinate whose operations and their order the model fixes, so nothing here depends on
// the order in which lanes run.
//
// An edge is the vertex pair a < b and a OWNS it; edge k is the k-th pair in ascending (a, b) order.  The numbering is a bucket
// sort by owner with a short sort inside each bucket (DESIGN.md 4.14 says why not a device-wide sort, and why the vertex ->
// element table is not needed):
//   ml_edges_kernel   one lane per (element, local edge), twice: count the slots of every owner, then -- after a scan over the
//                     vertices -- write b into the owner's segment at a position an atomic counter hands out.  The order inside
//                     a segment is the order in which the atomics land; the next kernel removes it.
//   ml_sort_kernel    one lane per vertex: sorts its segment in place (insertion below 33 entries, heap sort above: no limit on
//                     the edges of a vertex and no quadratic cost on a fan), drops the repeats -- an interior edge of a hexahedral
//                     mesh arrives from four elements -- and counts what is left.  A scan over the vertices gives edge_ptr, a
//                     copy edge_hi.
//   ml_face_*         one flag per slot of the face table of the order-1 mesh: the slot is a hexahedron's and is the lower of
//                     its pair (or alone); a scan over the slots ranks the flagged slots, which are face_slot.
//   ml_nodes_kernel   one lane per (element, local node of the lifted element): a corner copies its vertex id, an edge node
//                     finds its pair by bisection in its owner's segment of edge_hi, a face node reads the rank of its slot's
//                     representative, a centre the rank of its element.  With coordinates the same lane writes the node's
//                     coordinates; the lanes of several elements write the same bits to a shared edge or face node.
#include "mesh_lift.h"
#include "devtab.h"

#include <algorithm>
#include <climits>

#include "mesh.h"

namespace saamge_amd {

namespace {

// ---- the tables of mesh_lift_model.py: LOCAL_EDGES and, per local node of the lifted element, what it is ---------------------------
constexpr int ML_MAX_EDGES = 12, ML_MAX_ND2 = 27;
enum { ML_VERTEX = 0, ML_EDGE = 1, ML_FACE = 2, ML_CENTRE = 3 };
struct MlTables {
    int nd2[EM_TYPES];                             // nodes of the lifted element; 0: the type has no lift
    int nedges[EM_TYPES];
    int edge[EM_TYPES][ML_MAX_EDGES][2];           // local corner nodes
    int kind[EM_TYPES][ML_MAX_ND2], arg[EM_TYPES][ML_MAX_ND2];      // arg: the corner, local edge or local face
};
constexpr MlTables ml_tables() {
    MlTables t{};
    constexpr int TRI[3][2] = {{0, 1}, {1, 2}, {2, 0}};
    constexpr int QUAD[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}};
    constexpr int TET[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    for (int ty = 0; ty < 3; ++ty) {      // triangle, quadrilateral, tetrahedron: the vertices, the edges, (the centre)
        const int nv = ty == 0 ? 3 : 4, ne = ty == 0 ? 3 : (ty == 1 ? 4 : 6);
        t.nedges[ty] = ne;
        t.nd2[ty] = nv + ne + (ty == 1 ? 1 : 0);
        for (int k = 0; k < ne; ++k)
            for (int i = 0; i < 2; ++i) t.edge[ty][k][i] = ty == 0 ? TRI[k][i] : (ty == 1 ? QUAD[k][i] : TET[k][i]);
        for (int p = 0; p < t.nd2[ty]; ++p) {
            t.kind[ty][p] = p < nv ? ML_VERTEX : (p < nv + ne ? ML_EDGE : ML_CENTRE);
            t.arg[ty][p] = p < nv ? p : (p < nv + ne ? p - nv : 0);
        }
    }
    // the hexahedron: the 12 corner pairs that differ in one coordinate, i < j ascending; the 27 nodes are lexicographic
    int masks[ML_MAX_EDGES] = {};
    for (int i = 0; i < 8; ++i)
        for (int j = i + 1; j < 8; ++j) {
            int differ = 0;
            for (int d = 0; d < 3; ++d) differ += EM_HEX_LOC[i][d] != EM_HEX_LOC[j][d];
            if (differ != 1) continue;
            t.edge[4][t.nedges[4]][0] = i;
            t.edge[4][t.nedges[4]][1] = j;
            masks[t.nedges[4]++] = (1 << i) | (1 << j);
        }
    t.nd2[4] = 27;
    for (int p = 0; p < 27; ++p) {
        const int pos[3] = {p % 3, (p / 3) % 3, p / 9};
        int mask = 0, bits = 0, first = -1;
        for (int c = 0; c < 8; ++c) {
            bool in = true;
            for (int d = 0; d < 3; ++d) in = in && (pos[d] == 1 || pos[d] == 2 * EM_HEX_LOC[c][d]);
            if (in) {
                mask |= 1 << c;
                ++bits;
                if (first < 0) first = c;
            }
        }
        t.kind[4][p] = bits == 1 ? ML_VERTEX : (bits == 2 ? ML_EDGE : (bits == 4 ? ML_FACE : ML_CENTRE));
        t.arg[4][p] = bits == 1 ? first : -1;
        for (int k = 0; k < ML_MAX_EDGES && bits == 2; ++k)
            if (masks[k] == mask) t.arg[4][p] = k;
        for (int lf = 0; lf < 6 && bits == 4; ++lf) {
            int fm = 0;
            for (int k = 0; k < 4; ++k) fm |= 1 << BDR_HEX_FACES[lf][k];
            if (fm == mask) t.arg[4][p] = lf;
        }
        if (bits == 8) t.arg[4][p] = 0;
    }
    return t;
}
constexpr bool ml_tables_ok() {      // the hexahedron has 8 + 12 + 6 + 1 nodes, each found; the quad9 edge nodes follow EM2_QUAD_LOC
    const MlTables t = ml_tables();
    int n[4] = {0, 0, 0, 0};
    for (int p = 0; p < 27; ++p) {
        if (t.arg[4][p] < 0) return false;
        ++n[t.kind[4][p]];
    }
    if (t.nedges[4] != 12 || n[0] != 8 || n[1] != 12 || n[2] != 6 || n[3] != 1) return false;
    for (int k = 0; k < 4; ++k)
        for (int d = 0; d < 2; ++d)
            if (2 * EM2_QUAD_LOC[4 + k][d] != EM2_QUAD_LOC[t.edge[1][k][0]][d] + EM2_QUAD_LOC[t.edge[1][k][1]][d]) return false;
    return EM2_QUAD_LOC[8][0] == 1 && EM2_QUAD_LOC[8][1] == 1;
}
static_assert(ml_tables_ok(), "mesh_lift: the node tables");
__device__ const MlTables ML = ml_tables();
constexpr MlTables ML_HOST = ml_tables();

// words of a lift: [0] first element of no type, [1] first element without a lift, [2] first element whose slots in the given
// face table are not those of its type (minima), [3] the most edges one vertex owns
constexpr int ML_WORDS = 4;

// what mesh_classify_kernel keeps per element: the nodes of the lifted element and whether it has a centre node; an element
// without a lift goes to the minimum *no_lift
struct MlLiftedNodes {
    int *centre, *no_lift;
    __device__ int operator()(int t, int e) const {
        const int n2 = t < 0 ? 0 : ML.nd2[t];
        centre[e] = (int)(t == 1 || t == 4);
        if (t >= 0 && n2 == 0) atomicMin(no_lift, e);
        return n2;
    }
};
// a face table handed in: every element has the slots of its type
__global__ __launch_bounds__(256) void ml_fits_kernel(int NE, int dim, const int *__restrict__ eI, const roff_t *__restrict__ slot_ptr,
                                                      int *__restrict__ words) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int t = em_type_index(dim, eI[e + 1] - eI[e]);
    if (slot_ptr[e + 1] - slot_ptr[e] != (roff_t)bdr_num_faces(t)) atomicMin(words + 2, (int)e);
}
// mark[v] = 1 for every vertex an element lists (every lane stores the same value)
__global__ __launch_bounds__(256) void ml_mark_kernel(long nconn, const int *__restrict__ eJ, int *__restrict__ mark) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < nconn) mark[eJ[i]] = 1;
}

// One lane per (element, local edge): lane t is local edge t % stride of element t / stride (stride: the most edges an element of
// this mesh can have).  FILL false: cnt[a] counts the slots of owner a.  FILL true: b goes into the owner's segment, cnt the cursor.
template <bool FILL>
__global__ __launch_bounds__(256) void ml_edges_kernel(long total, int stride, int dim, const int *__restrict__ eI,
                                                       const int *__restrict__ eJ, int *__restrict__ cnt,
                                                       const roff_t *__restrict__ raw_ptr, int *__restrict__ raw) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int e = (int)(t / stride), le = (int)(t - (long)e * stride);
    const int b = eI[e], type = em_type_index(dim, eI[e + 1] - b);      // (the mesh has been classified: a type with a lift)
    if (le >= ML.nedges[type]) return;
    const int v0 = eJ[b + ML.edge[type][le][0]], v1 = eJ[b + ML.edge[type][le][1]];
    const int a = min(v0, v1), hi = max(v0, v1);
    if (!FILL) atomicAdd(cnt + a, 1);
    else raw[raw_ptr[a] + atomicAdd(cnt + a, 1)] = hi;      // (the cursor stays below the count of the first pass)
}

__device__ inline void ml_sift(int *__restrict__ a, long i, long n) {
    const int x = a[i];
    for (;;) {
        long c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && a[c + 1] > a[c]) ++c;
        if (a[c] <= x) break;
        a[i] = a[c];
        i = c;
    }
    a[i] = x;
}
// One lane per vertex: its segment of raw sorted ascending in place, repeats dropped, the remaining entries counted.
__global__ __launch_bounds__(256) void ml_sort_kernel(int NV, const roff_t *__restrict__ raw_ptr, int *__restrict__ raw,
                                                      int *__restrict__ owned, int *__restrict__ words) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= NV) return;
    int *a = raw + raw_ptr[v];
    const long n = (long)(raw_ptr[v + 1] - raw_ptr[v]);
    if (n <= 32) {
        for (long i = 1; i < n; ++i) {
            const int x = a[i];
            long j = i;
            for (; j > 0 && a[j - 1] > x; --j) a[j] = a[j - 1];
            a[j] = x;
        }
    } else {
        for (long i = n / 2 - 1; i >= 0; --i) ml_sift(a, i, n);
        for (long end = n - 1; end > 0; --end) {
            const int x = a[0];
            a[0] = a[end];
            a[end] = x;
            ml_sift(a, 0, end);
        }
    }
    long w = 0;
    int prev = -1;                                                       // (no vertex id is -1)
    for (long i = 0; i < n; ++i) {
        const int x = a[i];
        if (x != prev) a[w++] = x;
        prev = x;
    }
    owned[v] = (int)w;
    raise_max(words + 3, (int)w);
}
__global__ __launch_bounds__(256) void ml_edge_hi_kernel(int NV, const roff_t *__restrict__ raw_ptr, const int *__restrict__ raw,
                                                         const roff_t *__restrict__ edge_ptr, int *__restrict__ edge_hi) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= NV) return;
    const roff_t src = raw_ptr[v], dst = edge_ptr[v], n = edge_ptr[v + 1] - dst;
    for (roff_t k = 0; k < n; ++k) edge_hi[dst + k] = raw[src + k];
}

// One lane per slot of the face table (lane t: local face t % 6 of element t / 6): flag[s] = 1 iff slot s is a hexahedron's and
// the representative of its face -- alone, or the lower slot of its pair.
__global__ __launch_bounds__(256) void ml_face_flag_kernel(long total, int dim, const int *__restrict__ eI,
                                                           const roff_t *__restrict__ slot_ptr, const int *__restrict__ nbr_elem,
                                                           const int *__restrict__ nbr_local, int *__restrict__ flag) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int e = (int)(t / BDR_MAX_FACES), lf = (int)(t - (long)e * BDR_MAX_FACES);
    const roff_t s0 = slot_ptr[e];
    if (lf >= (int)(slot_ptr[e + 1] - s0)) return;
    const roff_t s = s0 + lf;
    flag[s] = (int)(em_type_index(dim, eI[e + 1] - eI[e]) == 4 && opposite_slot(slot_ptr, nbr_elem, nbr_local, s) >= s);
}
__global__ __launch_bounds__(256) void ml_face_slot_kernel(long slots, const int *__restrict__ flag, const roff_t *__restrict__ rank,
                                                           roff_t *__restrict__ face_slot) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s < slots && flag[s]) face_slot[rank[s]] = s;
}

// One lane per (element, local node of the lifted element): lane t is node t % stride of element t / stride.  X2: all
// coordinates, rows [0, NV) hold the vertices already; the lane writes the row of its own node (no row below NV).
template <bool COORDS>
__global__ __launch_bounds__(256) void ml_nodes_kernel(long total, int stride, int dim, int NV, long NEd, long NFq,
                                                       const int *__restrict__ eI, const int *__restrict__ eJ,
                                                       const int *__restrict__ ep2, const roff_t *__restrict__ edge_ptr,
                                                       const int *__restrict__ edge_hi, const roff_t *__restrict__ slot_ptr,
                                                       const int *__restrict__ nbr_elem, const int *__restrict__ nbr_local,
                                                       const roff_t *__restrict__ face_rank, const int *__restrict__ centre_rank,
                                                       int *__restrict__ out, double *X2) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int e = (int)(t / stride), p = (int)(t - (long)e * stride);
    const int b = eI[e], type = em_type_index(dim, eI[e + 1] - b);
    if (p >= ML.nd2[type]) return;
    const int kind = ML.kind[type][p], arg = ML.arg[type][p];
    int node;
    if (kind == ML_VERTEX) {
        node = eJ[b + arg];
    } else if (kind == ML_EDGE) {
        const int v0 = eJ[b + ML.edge[type][arg][0]], v1 = eJ[b + ML.edge[type][arg][1]];
        const int a = min(v0, v1), hi = max(v0, v1);
        node = (int)(NV + last_le(edge_hi, edge_ptr[a], edge_ptr[a + 1], hi));      // the last entry <= hi: the pair itself
        if (COORDS)
            for (int d = 0; d < dim; ++d) X2[(long)node * dim + d] = 0.5 * (X2[(long)a * dim + d] + X2[(long)hi * dim + d]);
    } else if (kind == ML_FACE) {
        const roff_t s = slot_ptr[e] + arg;
        node = (int)(NV + NEd + face_rank[min(s, opposite_slot(slot_ptr, nbr_elem, nbr_local, s))]);
        if (COORDS) {
            int v[4] = {eJ[b + BDR_HEX_FACES[arg][0]], eJ[b + BDR_HEX_FACES[arg][1]], eJ[b + BDR_HEX_FACES[arg][2]],
                        eJ[b + BDR_HEX_FACES[arg][3]]};
            sort4(v);
            for (int d = 0; d < dim; ++d)
                X2[(long)node * dim + d] = 0.25 * ((X2[(long)v[0] * dim + d] + X2[(long)v[1] * dim + d]) +
                                                   (X2[(long)v[2] * dim + d] + X2[(long)v[3] * dim + d]));
        }
    } else {
        node = (int)(NV + NEd + NFq + centre_rank[e]);
        if (COORDS)
            for (int d = 0; d < dim; ++d) {
                const double q = (X2[(long)eJ[b] * dim + d] + X2[(long)eJ[b + 1] * dim + d]) +
                                 (X2[(long)eJ[b + 2] * dim + d] + X2[(long)eJ[b + 3] * dim + d]);
                if (type == 1) {
                    X2[(long)node * dim + d] = 0.25 * q;
                } else {
                    const double r = (X2[(long)eJ[b + 4] * dim + d] + X2[(long)eJ[b + 5] * dim + d]) +
                                     (X2[(long)eJ[b + 6] * dim + d] + X2[(long)eJ[b + 7] * dim + d]);
                    X2[(long)node * dim + d] = 0.125 * (q + r);
                }
            }
    }
    out[ep2[e] + p] = node;
}

}  // namespace

void mesh_lift_order2(hipStream_t s, const MeshArgs &m, const FaceTable *faces, MeshLift &L, long long info[8]) {
    const std::string name("saamge_amd_mesh_lift_order2: ");
    const int NV = m.NV, dim = m.dim, NE = m.NE, nde = m.nde;
    const int *const elem_ptr = m.elem_ptr;
    const double *const coords = m.coords;
    // ---- the checks that need no device; the limit is the lift's own: the lifted lists are the longer ones
    mesh_begin(name, m, info);
    const int t1 = em_type_index(dim, nde);
    mesh_check_sizes(name, m, 0, true, t1 < 0 ? 0 : ML_HOST.nd2[t1], "the element -> node lists are beyond 32 bits");
    SA_REQUIRE(!faces || faces->NE == NE, name + "faces: the face table does not fit the mesh (its number of elements)");
    L.device = current_device();
    SA_REQUIRE(!faces || faces->device == L.device, name + "faces: the face table lives on another device");
    L.NV = NV;
    L.NE = NE;
    L.dim = dim;
    L.edge_ptr.alloc((size_t)NV + 1);
    L.elem_ptr2.alloc((size_t)NE + 1);
    const DevIn<double> in_X(coords, (size_t)NV * dim, s);
    const double *X = in_X.p;
    if (NE == 0) {
        L.edge_ptr.zero(s);
        L.elem_ptr2.zero(s);
        L.NV2 = NV;
        if (coords) {
            L.coords2.alloc((size_t)NV * dim);
            copy_device(L.coords2.p, X, (size_t)NV * dim, s);
        }
        SA_HIP_CHECK(hipStreamSynchronize(s));
        if (info) info[0] = info[7] = NV;
        return;
    }
    DeviceMesh M;
    import_mesh(s, name, m, M);
    // ---- the type of every element
    DBuf<int> nd2((size_t)NE), centre((size_t)NE), words(ML_WORDS);
    const int init[ML_WORDS] = {INT_MAX, INT_MAX, INT_MAX, 0};
    upload_async(words.p, init, ML_WORDS, s);
    mesh_classify(s, NE, dim, M.eI, nd2.p, words.p, MlLiftedNodes{centre.p, words.p + 1});
    int w[ML_WORDS];
    read_back(w, (const int *)words.p, ML_WORDS, s);
    if (w[0] < NE) refuse_element_type(s, name, dim, M.eI, w[0]);
    if (w[1] < NE) {
        const int nd = read_one(M.eI + w[1] + 1, s) - read_one(M.eI + w[1], s);
        const std::string which = name + "element " + std::to_string(w[1]) + ": ";
        if (info) info[6] = w[1];
        SA_REQUIRE(nd != 6 || dim != 3, which + "a wedge has no order-2 type");
        SA_REQUIRE(false, which + std::to_string(nd) + " nodes: the element is of order 2 already");
    }
    if (faces) {
        hipLaunchKernelGGL(ml_fits_kernel, grid_flat(NE), dim3(256), 0, s, NE, dim, M.eI, (const roff_t *)faces->slot_ptr.p, words.p);
        SA_HIP_CHECK(hipGetLastError());
        const int bad = read_one((const int *)words.p + 2, s);
        SA_REQUIRE(bad >= NE, name + "faces: the face table does not fit the mesh (the slots of element " + std::to_string(bad) + ")");
    }
    DBuf<roff_t> ep2_wide((size_t)NE + 1);
    DBuf<int> centre_rank((size_t)NE + 1);
    exclusive_scan_off(s, NE, nd2.p, ep2_wide.p);
    exclusive_scan_int(s, NE, centre.p, centre_rank.p);
    L.entries = (long long)read_one((const roff_t *)ep2_wide.p + NE, s);
    L.NC = read_one((const int *)centre_rank.p + NE, s);
    SA_REQUIRE(L.entries <= INT_MAX, name + "the element -> node lists are beyond 32 bits");
    dev_convert(s, (long)NE + 1, (const roff_t *)ep2_wide.p, L.elem_ptr2.p);
    ep2_wide.release();
    nd2.release();
    centre.release();
    // ---- the vertices that no element lists
    long long unlisted = 0;
    {
        DBuf<int> mark((size_t)NV), mark_ptr((size_t)NV + 1);
        mark.zero(s);
        hipLaunchKernelGGL(ml_mark_kernel, grid_flat(M.nconn), dim3(256), 0, s, M.nconn, M.eJ, mark.p);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_int(s, NV, mark.p, mark_ptr.p);
        unlisted = NV - read_one((const int *)mark_ptr.p + NV, s);
    }
    // ---- the edges: bucket by owner, sort and drop the repeats inside each bucket
    {
        const int stride = elem_ptr ? (dim == 2 ? 4 : ML_MAX_EDGES) : ML_HOST.nedges[em_type_index(dim, nde)];
        const long total = (long)NE * stride;
        DBuf<int> cnt((size_t)NV);
        DBuf<roff_t> raw_ptr((size_t)NV + 1);
        cnt.zero(s);
        hipLaunchKernelGGL(ml_edges_kernel<false>, grid_flat(total), dim3(256), 0, s, total, stride, dim, M.eI, M.eJ, cnt.p,
                           (const roff_t *)nullptr, (int *)nullptr);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_off(s, NV, cnt.p, raw_ptr.p);
        DBuf<int> raw((size_t)read_one((const roff_t *)raw_ptr.p + NV, s));
        cnt.zero(s);
        hipLaunchKernelGGL(ml_edges_kernel<true>, grid_flat(total), dim3(256), 0, s, total, stride, dim, M.eI, M.eJ, cnt.p,
                           (const roff_t *)raw_ptr.p, raw.p);
        hipLaunchKernelGGL(ml_sort_kernel, grid_flat(NV), dim3(256), 0, s, NV, (const roff_t *)raw_ptr.p, raw.p, cnt.p, words.p);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_off(s, NV, cnt.p, L.edge_ptr.p);
        L.NEd = (long long)read_one((const roff_t *)L.edge_ptr.p + NV, s);
        L.edge_hi.alloc((size_t)L.NEd);
        hipLaunchKernelGGL(ml_edge_hi_kernel, grid_flat(NV), dim3(256), 0, s, NV, (const roff_t *)raw_ptr.p, (const int *)raw.p,
                           (const roff_t *)L.edge_ptr.p, L.edge_hi.p);
        SA_HIP_CHECK(hipGetLastError());
    }
    // ---- the quadrilateral faces of the hexahedra: the representative slots of the face table of the order-1 mesh
    FaceTable own;
    const FaceTable *T = nullptr;
    DBuf<roff_t> face_rank;
    if (dim == 3 && L.NC > 0) {
        T = faces;
        if (!T) {
            long long finfo[8];
            try {
                face_table_build(s, MeshArgs{NV, dim, nullptr, NE, nde, elem_ptr ? M.eI : nullptr, M.eJ}, own, finfo);
            } catch (const Error &) {
                if (info) info[6] = finfo[6];
                throw;
            }
            T = &own;
        }
        const long slots = (long)T->nbr_elem.n, total = (long)NE * BDR_MAX_FACES;
        DBuf<int> flag((size_t)slots);
        face_rank.alloc((size_t)slots + 1);
        hipLaunchKernelGGL(ml_face_flag_kernel, grid_flat(total), dim3(256), 0, s, total, dim, M.eI, (const roff_t *)T->slot_ptr.p,
                           (const int *)T->nbr_elem.p, (const int *)T->nbr_local.p, flag.p);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_off(s, (int)slots, flag.p, face_rank.p);
        L.NFq = (long long)read_one((const roff_t *)face_rank.p + slots, s);
        L.face_slot.alloc((size_t)L.NFq);
        hipLaunchKernelGGL(ml_face_slot_kernel, grid_flat(slots), dim3(256), 0, s, slots, (const int *)flag.p,
                           (const roff_t *)face_rank.p, L.face_slot.p);
        SA_HIP_CHECK(hipGetLastError());
    }
    const long long NV2 = (long long)NV + L.NEd + L.NFq + L.NC;
    if (info) {
        info[0] = NV2;
        info[1] = L.NEd;
        info[2] = L.NFq;
        info[3] = L.NC;
        info[4] = L.entries;
        info[5] = read_one((const int *)words.p + 3, s);
        info[7] = unlisted;
    }
    SA_REQUIRE(NV2 <= INT_MAX, name + "NV2 = " + std::to_string(NV2) + " nodes are beyond 32 bits");
    L.NV2 = (int)NV2;
    // ---- the node lists and the coordinates
    L.elem_to_node.alloc((size_t)L.entries);
    if (coords) {
        L.coords2.alloc((size_t)NV2 * dim);
        copy_device(L.coords2.p, X, (size_t)NV * dim, s);
    }
    const int stride = elem_ptr ? (dim == 2 ? 9 : ML_MAX_ND2) : ML_HOST.nd2[em_type_index(dim, nde)];
    const long total = (long)NE * stride;
    const auto nodes = coords ? ml_nodes_kernel<true> : ml_nodes_kernel<false>;
    hipLaunchKernelGGL(nodes, grid_flat(total), dim3(256), 0, s, total, stride, dim, NV, (long)L.NEd, (long)L.NFq, M.eI, M.eJ,
                       (const int *)L.elem_ptr2.p, (const roff_t *)L.edge_ptr.p, (const int *)L.edge_hi.p,
                       T ? (const roff_t *)T->slot_ptr.p : (const roff_t *)nullptr, T ? (const int *)T->nbr_elem.p : (const int *)nullptr,
                       T ? (const int *)T->nbr_local.p : (const int *)nullptr, (const roff_t *)face_rank.p,
                       (const int *)centre_rank.p, L.elem_to_node.p, L.coords2.p);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
