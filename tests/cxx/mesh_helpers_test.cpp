// The pieces the mesh kernels share (csrc/mesh_helpers.h, and the corner formula of csrc/elmat_types.h) on the host: plain C++,
// no HIP.  The kernels call the same functions.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "elmat_types.h"
#include "mesh_helpers.h"

using namespace saamge_amd;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: %s fails\n", __FILE__, __LINE__, #cond);     \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static unsigned next_random(unsigned &state) {      // a fixed sequence: xorshift32
    state ^= state << 13;
    state ^= state >> 17;
    state ^= state << 5;
    return state;
}

int main() {
    // ---- sort4: all 24 orders of four distinct values, and of values with a repeat
    {
        int p[4] = {0, 1, 2, 3}, count = 0;
        do {
            int v[4] = {10 * p[0], 10 * p[1], 10 * p[2], 10 * p[3]};
            sort4(v);
            for (int i = 0; i < 4; ++i) CHECK(v[i] == 10 * i);
            int w[4] = {p[0] / 2, p[1] / 2, p[2] / 2, p[3] / 2};      // 0, 0, 1, 1 in every order
            sort4(w);
            CHECK(w[0] == 0 && w[1] == 0 && w[2] == 1 && w[3] == 1);
            ++count;
        } while (std::next_permutation(p, p + 4));
        CHECK(count == 24);
    }
    // ---- sort8: all 256 sequences of zeros and ones, then 400 fixed pseudo-random sequences with repeats (values in [0, 6))
    for (int m = 0; m < 256; ++m) {
        int v[8], ones = 0;
        for (int i = 0; i < 8; ++i) ones += v[i] = (m >> i) & 1;
        sort8(v);
        for (int i = 0; i < 8; ++i) CHECK(v[i] == (int)(i >= 8 - ones));
    }
    {
        unsigned state = 2463534242u;
        for (int round = 0; round < 400; ++round) {
            int v[8], w[8];
            const unsigned range = round % 2 ? 6u : 1000000u;
            for (int i = 0; i < 8; ++i) w[i] = v[i] = (int)(next_random(state) % range) - 3;
            sort8(v);
            std::sort(w, w + 8);
            for (int i = 0; i < 8; ++i) CHECK(v[i] == w[i]);
        }
    }
    // ---- last_le against std::upper_bound: offsets with empty segments, x at the first and the last entry, a range of one entry
    {
        const std::vector<long long> ptr = {0, 0, 3, 3, 3, 7, 8, 8, 12};      // 8 segments, four of them empty
        const long n = (long)ptr.size() - 1;                                   // the offsets of the segments: ptr[0 .. n)
        for (long long x = ptr.front(); x < ptr.back(); ++x) {
            const long want = (long)(std::upper_bound(ptr.begin(), ptr.begin() + n, x) - ptr.begin()) - 1;
            CHECK(last_le(ptr.data(), 0, n, x) == want);
            CHECK(ptr[(size_t)want] <= x && x < ptr[(size_t)want + 1]);        // x lies in segment `want`, which is not empty
        }
        CHECK(last_le(ptr.data(), 0, n, 0ll) == 1 && last_le(ptr.data(), 0, n, 11ll) == 7);
        CHECK(last_le(ptr.data(), 0, n + 1, 12ll) == n);                       // x at the last entry
        CHECK(last_le(ptr.data(), 5, 6, 7ll) == 5);                            // one entry
        // a segment of a sorted list, as the lift looks an edge up: the upper ends {4, 6, 9} of vertex 2 at [3, 6)
        const std::vector<int> hi = {1, 2, 3, 4, 6, 9, 5};
        for (long k = 3; k < 6; ++k) CHECK(last_le(hi.data(), 3, 6, hi[(size_t)k]) == k);
    }
    // ---- opposite_slot: a tetrahedron (slots 0 .. 3) and a second one (4 .. 7) that share face 2 of the first, face 0 of the second
    {
        const long long slot_ptr[3] = {0, 4, 8};
        const int nbr_elem[8] = {-1, -1, 1, -1, 0, -1, -1, -1}, nbr_local[8] = {-1, -1, 0, -1, 2, -1, -1, -1};
        for (long long s = 0; s < 8; ++s) {
            const long long want = s == 2 ? 4 : (s == 4 ? 2 : s);
            CHECK(opposite_slot(slot_ptr, nbr_elem, nbr_local, s) == want);
        }
    }
    // ---- the corners of the 27-node hexahedron
    {
        const int want[8] = {0, 2, 8, 6, 18, 20, 26, 24};
        for (int j = 0; j < 8; ++j) CHECK(em_hex27_corner(j) == want[j]);
        CHECK(em_hex27_node(1, 1, 1) == 13 && em_hex27_node(2, 0, 0) == 2 && em_hex27_node(0, 2, 0) == 6 && em_hex27_node(0, 0, 2) == 18);
    }
    std::printf("mesh helpers test ok\n");
    return 0;
}
