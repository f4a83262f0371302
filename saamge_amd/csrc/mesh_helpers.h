// Small pieces the mesh kernels share (mesh_faces.hip, mesh_lift.hip, mesh_refine.hip): plain constexpr C++ like elmat_ref.h, so
// the kernels call them as they are and tests/cxx/mesh_helpers_test.cpp holds them on the host without HIP.
#pragma once

namespace saamge_amd {

// ---- fixed sorting networks: every index is a compile-time constant, so the values stay in registers -------------------------
constexpr void sort2(int &x, int &y) {
    const int lo = x < y ? x : y, hi = x < y ? y : x;
    x = lo;
    y = hi;
}
// ascending order of 4 values by five exchanges, of 8 by Batcher's odd-even merge (19 exchanges)
constexpr void sort4(int *v) {
    sort2(v[0], v[1]);
    sort2(v[2], v[3]);
    sort2(v[0], v[2]);
    sort2(v[1], v[3]);
    sort2(v[1], v[2]);
}
constexpr void sort8(int *v) {
    sort2(v[0], v[1]); sort2(v[2], v[3]); sort2(v[4], v[5]); sort2(v[6], v[7]);
    sort2(v[0], v[2]); sort2(v[1], v[3]); sort2(v[4], v[6]); sort2(v[5], v[7]);
    sort2(v[1], v[2]); sort2(v[5], v[6]);
    sort2(v[0], v[4]); sort2(v[1], v[5]); sort2(v[2], v[6]); sort2(v[3], v[7]);
    sort2(v[2], v[4]); sort2(v[3], v[5]);
    sort2(v[1], v[2]); sort2(v[3], v[4]); sort2(v[5], v[6]);
}
template <int N>
constexpr bool sorts_zero_one(void (*sort)(int *)) {      // a network that sorts every sequence of zeros and ones sorts every sequence
    for (int m = 0; m < (1 << N); ++m) {
        int v[N] = {};
        for (int i = 0; i < N; ++i) v[i] = (m >> i) & 1;
        sort(v);
        for (int i = 0; i + 1 < N; ++i)
            if (v[i] > v[i + 1]) return false;
    }
    return true;
}
static_assert(sorts_zero_one<4>(sort4), "mesh_helpers: the network of four");
static_assert(sorts_zero_one<8>(sort8), "mesh_helpers: the network of eight");

// the last i of [lo, up) with ptr[i] <= x (ptr ascending on [lo, up), ptr[lo] <= x)
template <class T>
constexpr long last_le(const T *ptr, long lo, long up, T x) {
    while (up - lo > 1) {
        const long mid = lo + (up - lo) / 2;
        if (ptr[mid] <= x) lo = mid;
        else up = mid;
    }
    return lo;
}

// the slot across the face of slot s of a face table (mesh_faces.h): s itself on the boundary
template <class O>
constexpr O opposite_slot(const O *slot_ptr, const int *nbr_elem, const int *nbr_local, O s) {
    const int ne = nbr_elem[s];
    return ne < 0 ? s : slot_ptr[ne] + nbr_local[s];
}

}  // namespace saamge_amd
