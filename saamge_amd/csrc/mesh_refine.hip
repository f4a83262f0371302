// An order-1 mesh refined uniformly (mesh_refine.h): saamge_amd/mesh_refine_model.py restated for gfx950.  One step is the
// order-2 lift of the mesh (mesh_lift.hip: the nodes of the lifted mesh are the vertices of the refined one, with their
// coordinates) and two kernels of its own; every output is an integer the mesh fixes uniquely or one of the values 1, 0.5,
// 0.25, 0.125, so nothing here depends on the order in which lanes run.
//   mr_children_kernel  one lane per (child, local corner): the corner's vertex is read from the parent's row of the lifted
//                       node list through the compile-time table of the parent's type; the lane of corner 0 writes the child's
//                       offset.  The lanes of a wavefront write consecutive entries of the child list.
//   mr_interp_kernel    one lane per row of P (and one for rowptr[nrows]): the offsets are closed-form -- 1 entry per kept
//                       vertex, 2 per edge, 4 per face, 4 | 8 per centre --, the owner of an edge is found by bisection in
//                       edge_ptr, the vertices of a face from its slot of face_slot, and the columns of a face or centre row are
//                       put in ascending order by a fixed network of exchanges.
// A list that mixes types needs, for the rows of faces and centres, the element of a slot and of a centre: mesh_classify_kernel and
// two scans give the offsets both are found in by bisection.  A list of one type needs neither (slot s is face s % 6 of
// hexahedron s / 6, centre c is element c).
#include "mesh_refine.h"
#include "devtab.h"

#include <algorithm>
#include <climits>

#include "mesh.h"
#include "mesh_lift.h"

namespace saamge_amd {

namespace {

// ---- mesh_refine_model.CHILDREN: local corner j of child k as an index into the parent's lifted local node list ---------------
constexpr int MR_MAX_CHILDREN = 8, MR_MAX_ND = 8;
struct MrTables {
    int child[EM_TYPES][MR_MAX_CHILDREN][MR_MAX_ND];
};
constexpr MrTables mr_tables() {
    MrTables t{};
    constexpr int TRI[4][3] = {{0, 3, 5}, {3, 1, 4}, {5, 4, 2}, {3, 4, 5}};
    // the corner children, then the inner octahedron cut along m02 - m13 (Bey); DESIGN.md 4.15 says why these four
    constexpr int TET[8][4] = {{0, 4, 5, 6}, {4, 1, 7, 8}, {5, 7, 2, 9}, {6, 8, 9, 3}, {4, 5, 6, 8}, {7, 5, 4, 8}, {5, 6, 8, 9}, {8, 7, 5, 9}};
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j) t.child[0][k][j] = TRI[k][j];
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 4; ++j) t.child[2][k][j] = TET[k][j];
    // quadrilateral and hexahedron: the lifted node at reference position LOC[k] + LOC[j]
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 4; ++j) {
            const int x = (EM2_QUAD_LOC[k][0] + EM2_QUAD_LOC[j][0]) / 2, y = (EM2_QUAD_LOC[k][1] + EM2_QUAD_LOC[j][1]) / 2;
            t.child[1][k][j] = -1;
            for (int p = 0; p < 9; ++p)
                if (EM2_QUAD_LOC[p][0] == x && EM2_QUAD_LOC[p][1] == y) t.child[1][k][j] = p;
        }
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 8; ++j)
            t.child[4][k][j] = em_hex27_node(EM_HEX_LOC[k][0] + EM_HEX_LOC[j][0], EM_HEX_LOC[k][1] + EM_HEX_LOC[j][1],
                                             EM_HEX_LOC[k][2] + EM_HEX_LOC[j][2]);
    return t;
}
// a lifted node with m ones in its reference position is listed by 2^m children (a corner by 1, an edge node by 2, a face node
// by 4, a hexahedron's centre by 8), child k holds the parent's corner k at its own position k, and the quadrilateral's children
// are the four the model names
constexpr bool mr_tables_ok() {
    const MrTables t = mr_tables();
    constexpr int QUAD[4][4] = {{0, 4, 8, 7}, {4, 1, 5, 8}, {8, 5, 2, 6}, {7, 8, 6, 3}};
    int used2[9] = {}, used3[27] = {};
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 4; ++j) {
            if (t.child[1][k][j] != QUAD[k][j]) return false;
            ++used2[t.child[1][k][j]];
        }
    for (int p = 0; p < 9; ++p)
        if (used2[p] != (1 << ((EM2_QUAD_LOC[p][0] == 1) + (EM2_QUAD_LOC[p][1] == 1)))) return false;
    for (int k = 0; k < 8; ++k) {
        if (t.child[4][k][k] != em_hex27_corner(k)) return false;
        for (int j = 0; j < 8; ++j) {
            if (t.child[4][k][j] < 0 || t.child[4][k][j] >= 27) return false;
            ++used3[t.child[4][k][j]];
        }
    }
    for (int p = 0; p < 27; ++p)
        if (used3[p] != (1 << ((p % 3 == 1) + ((p / 3) % 3 == 1) + (p / 9 == 1)))) return false;
    int tri[6] = {}, tet[10] = {};
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j) ++tri[t.child[0][k][j]];
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 4; ++j) ++tet[t.child[2][k][j]];
    for (int p = 0; p < 6; ++p)
        if (tri[p] != (p < 3 ? 1 : 3)) return false;
    for (int p = 0; p < 10; ++p)      // m02 (5) and m13 (8) are the ends of the diagonal: in all four inner children
        if (tet[p] != (p < 4 ? 1 : (p == 5 || p == 8 ? 6 : 4))) return false;
    return true;
}
static_assert(mr_tables_ok(), "mesh_refine: the child tables");
__device__ const MrTables MR = mr_tables();

// One lane per (child, local corner): lane t is corner t % stride of child t / stride (stride: the most corners an element of
// this mesh can have).  eI NULL: NE elements of nde corners each.  Child c of a parent whose list starts at b and has nd
// entries starts at nc * b + k * nd: all elements before the parent have nc children of their own size.
__global__ __launch_bounds__(256) void mr_children_kernel(long total, int stride, int log_nc, int dim, int NE, int nde,
                                                          const int *__restrict__ eI, const int *__restrict__ ep2,
                                                          const int *__restrict__ e2n, int *__restrict__ out_ptr,
                                                          int *__restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long c = t / stride;
    const int j = (int)(t - c * stride), e = (int)(c >> log_nc), k = (int)(c - ((long)e << log_nc));
    const long b = eI ? (long)eI[e] : (long)e * nde;
    const int nd = eI ? eI[e + 1] - (int)b : nde;
    if (j >= nd) return;
    const int type = em_type_index(dim, nd);                              // (the lift has classified the mesh: a type with children)
    const long o = (b << log_nc) + (long)k * nd;
    out[o + j] = e2n[ep2[e] + MR.child[type][k][j]];
    if (j == 0) {
        out_ptr[c] = (int)o;
        if (c == ((long)NE << log_nc) - 1) out_ptr[c + 1] = (int)(o + nd);
    }
}

// what mesh_classify_kernel keeps per element of a mixed list with the interpolation asked for: the number of its faces and
// whether it has a centre node (the lift has classified the mesh: every element has a type)
struct MrFacesAndCentre {
    int *centre;
    __device__ int operator()(int t, int e) const {
        centre[e] = (int)(t == 1 || t == 4);
        return bdr_num_faces(t);
    }
};

// One lane per row r of P, r in [0, NV2], NV2 = NV + NEd + NFq + NC; lane NV2 writes rowptr[NV2] = nnz.  slot_ptr NULL: slot s
// is face s % 6 of element s / 6; centre_rank NULL: centre c is element c.
__global__ __launch_bounds__(256) void mr_interp_kernel(int NV, long NEd, long NFq, long NC, int dim, int NE, int nde,
                                                        const int *__restrict__ eI, const int *__restrict__ eJ,
                                                        const roff_t *__restrict__ edge_ptr, const int *__restrict__ edge_hi,
                                                        const roff_t *__restrict__ face_slot, const roff_t *__restrict__ slot_ptr,
                                                        const roff_t *__restrict__ centre_rank, int *__restrict__ rowptr,
                                                        int *__restrict__ col, double *__restrict__ val) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const long NV2 = NV + NEd + NFq + NC;
    if (r > NV2) return;
    const int cc = dim == 2 ? 4 : 8;
    const long edges0 = NV, faces0 = edges0 + 2 * NEd, centres0 = faces0 + 4 * NFq;      // the first entry of each block of rows
    if (r < NV) {
        rowptr[r] = (int)r;
        col[r] = (int)r;
        val[r] = 1.0;
    } else if (r < NV + NEd) {
        const long k = r - NV, o = edges0 + 2 * k;
        rowptr[r] = (int)o;
        col[o] = (int)last_le(edge_ptr, 0, NV, (roff_t)k);      // the owner a: edge_ptr[a] <= k < edge_ptr[a + 1]
        col[o + 1] = edge_hi[k];                                // b > a
        val[o] = val[o + 1] = 0.5;
    } else if (r < NV + NEd + NFq) {
        const long f = r - NV - NEd, o = faces0 + 4 * f;
        const roff_t s = face_slot[f];
        const long e = slot_ptr ? last_le(slot_ptr, 0, NE, s) : (long)(s / BDR_MAX_FACES);
        const int lf = (int)(s - (slot_ptr ? slot_ptr[e] : (roff_t)e * BDR_MAX_FACES));
        const long b = eI ? (long)eI[e] : e * nde;
        int v[4];
        for (int i = 0; i < 4; ++i) v[i] = eJ[b + BDR_HEX_FACES[lf][i]];
        sort4(v);
        rowptr[r] = (int)o;
        for (int i = 0; i < 4; ++i) {
            col[o + i] = v[i];
            val[o + i] = 0.25;
        }
    } else if (r < NV2) {
        const long c = r - NV - NEd - NFq, o = centres0 + (long)cc * c;
        const long e = centre_rank ? last_le(centre_rank, 0, NE, (roff_t)c) : c;
        const long b = eI ? (long)eI[e] : e * nde;
        rowptr[r] = (int)o;
        if (cc == 4) {
            int v[4];
            for (int i = 0; i < 4; ++i) v[i] = eJ[b + i];
            sort4(v);
            for (int i = 0; i < 4; ++i) {
                col[o + i] = v[i];
                val[o + i] = 0.25;
            }
        } else {
            int v[8];
            for (int i = 0; i < 8; ++i) v[i] = eJ[b + i];
            sort8(v);
            for (int i = 0; i < 8; ++i) {
                col[o + i] = v[i];
                val[o + i] = 0.125;
            }
        }
    } else {
        rowptr[r] = (int)(centres0 + (long)cc * NC);
    }
}

}  // namespace

void mesh_refine(hipStream_t s, const MeshArgs &m, int levels, int want_interp, MeshRefine &R, long long info[8]) {
    const std::string name("saamge_amd_mesh_refine: ");
    const int NV = m.NV, dim = m.dim, NE = m.NE, nde = m.nde;
    const double *const coords = m.coords;
    const int *const elem_ptr = m.elem_ptr, *const elem_to_vertex = m.elem_to_vertex;
    mesh_info_begin(info);      // (the levels come first here; the lift of level 0 checks the mesh)
    SA_REQUIRE(levels >= 1, name + "levels must be at least 1");
    SA_REQUIRE(levels <= MESH_REFINE_MAX_LEVELS, name + "levels above " + std::to_string(MESH_REFINE_MAX_LEVELS));
    const bool uniform = !elem_ptr;
    // the mesh of the level at hand: the caller's at level 0 (host or device pointers, until the lift has checked them), then
    // what the buffers hold
    DBuf<double> bufX;
    DBuf<int> bufI, bufJ;
    const double *X = coords;
    const int *I = elem_ptr, *J = elem_to_vertex;
    int nv = NV, ne = NE;
    long long conn = 0, max_owned = 0, unlisted = 0, total_nnz = 0;
    R.level.clear();
    R.P.clear();
    for (int j = 0; j < levels; ++j) {
        MeshLift L;
        long long li[8] = {0, 0, 0, 0, 0, 0, -1, 0};
        try {
            mesh_lift_order2(s, MeshArgs{nv, dim, X, ne, nde, uniform ? nullptr : I, J}, nullptr, L, li);
        } catch (const Error &e) {
            if (info) info[6] = li[6];
            throw Error(e.code, name + "level " + std::to_string(j) + ": " + e.what());
        }
        const int log_nc = dim == 2 ? 2 : 3, cc = dim == 2 ? 4 : 8;
        if (j == 0) {      // the lift has checked the caller's lists: bring them to the device for the kernels here
            R.device = L.device;
            R.dim = dim;
            unlisted = li[7];
            if (ne > 0) {
                if (!uniform) I = (bufI = DevIn<int>(elem_ptr, (size_t)ne + 1, s).take()).p;
                conn = uniform ? (long long)ne * nde : (long long)read_one(I + ne, s);
                J = (bufJ = DevIn<int>(elem_to_vertex, (size_t)conn, s).take()).p;
            }
        }
        const long long nnz = (long long)nv + 2 * L.NEd + 4 * L.NFq + (long long)cc * L.NC;
        SA_REQUIRE((conn << log_nc) <= INT_MAX, name + "level " + std::to_string(j + 1) + ": the element -> vertex lists are beyond 32 bits");
        SA_REQUIRE(!want_interp || nnz <= INT_MAX,
                   name + "level " + std::to_string(j) + ": nnz = " + std::to_string(nnz) + " entries of the interpolation are beyond 32 bits");
        MeshRefineLevel lv;
        lv.NV = nv; lv.NE = ne; lv.entries = conn; lv.NEd = L.NEd; lv.NFq = L.NFq; lv.NC = L.NC; lv.max_owned = li[5];
        lv.nnz = want_interp ? nnz : 0;
        R.level.push_back(lv);
        max_owned = std::max(max_owned, li[5]);
        // ---- the children
        DBuf<int> nextI(((size_t)ne << log_nc) + 1), nextJ((size_t)(conn << log_nc));
        if (ne == 0) nextI.zero(s);
        else {
            const int stride = uniform ? nde : (dim == 2 ? 4 : MR_MAX_ND);
            const long total = ((long)ne << log_nc) * stride;
            hipLaunchKernelGGL(mr_children_kernel, grid_flat(total), dim3(256), 0, s, total, stride, log_nc, dim, ne, nde,
                               uniform ? (const int *)nullptr : I, (const int *)L.elem_ptr2.p, (const int *)L.elem_to_node.p, nextI.p,
                               nextJ.p);
            SA_HIP_CHECK(hipGetLastError());
        }
        // ---- the interpolation
        if (want_interp) {
            R.P.emplace_back();
            MeshInterp &P = R.P.back();
            P.nrows = L.NV2;
            P.ncols = nv;
            P.nnz = nnz;
            P.rowptr.alloc((size_t)L.NV2 + 1);
            P.col.alloc((size_t)nnz);
            P.val.alloc((size_t)nnz);
            DBuf<roff_t> slot_ptr, centre_rank;
            if (!uniform && L.NFq + L.NC > 0) {
                DBuf<int> nf((size_t)ne), centre((size_t)ne);
                slot_ptr.alloc((size_t)ne + 1);
                centre_rank.alloc((size_t)ne + 1);
                mesh_classify(s, ne, dim, I, nf.p, (int *)nullptr, MrFacesAndCentre{centre.p});      // (no element without a type)
                exclusive_scan_off(s, ne, nf.p, slot_ptr.p);
                exclusive_scan_off(s, ne, centre.p, centre_rank.p);
            }
            hipLaunchKernelGGL(mr_interp_kernel, grid_flat((long)L.NV2 + 1), dim3(256), 0, s, nv, (long)L.NEd, (long)L.NFq, (long)L.NC,
                               dim, ne, nde, uniform ? (const int *)nullptr : I, J, (const roff_t *)L.edge_ptr.p,
                               (const int *)L.edge_hi.p, (const roff_t *)L.face_slot.p, (const roff_t *)slot_ptr.p,
                               (const roff_t *)centre_rank.p, P.rowptr.p, P.col.p, P.val.p);
            SA_HIP_CHECK(hipGetLastError());
            total_nnz += nnz;
        }
        // ---- the next level takes the place of this one; the lifted node list goes with L
        bufX = std::move(L.coords2);
        bufI = std::move(nextI);
        bufJ = std::move(nextJ);
        X = bufX.p;
        I = bufI.p;
        J = bufJ.p;
        nv = L.NV2;
        ne <<= log_nc;
        conn <<= log_nc;
    }
    SA_HIP_CHECK(hipStreamSynchronize(s));
    MeshRefineLevel last;
    last.NV = nv; last.NE = ne; last.entries = conn;
    R.level.push_back(last);
    R.levels = levels;
    R.NV = nv;
    R.NE = ne;
    R.entries = conn;
    R.coords = std::move(bufX);
    R.elem_ptr = std::move(bufI);
    R.elem_to_vertex = std::move(bufJ);
    if (info) {
        info[0] = nv;
        info[1] = ne;
        info[2] = conn;
        info[3] = levels;
        info[4] = total_nnz;
        info[5] = max_owned;
        info[7] = unlisted;
    }
}

}  // namespace saamge_amd
