// The stable radix sorts of the device index tables (hipcub's DeviceRadixSort::SortPairs): the only header of the library
// that includes hipcub, for the two files that sort (topology_mis.hip, partition.hip).
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "devtab.h"

namespace saamge_amd {

// the bits that hold the keys 0 .. n - 1 (at least one)
inline int bits_for(int n) {
    int b = 1;
    while ((1ll << b) < n) ++b;
    return b;
}

// The stable radix sorts of (key, value) pairs of one phase, WIDE / int and int / int, at most n pairs each (WIDE: the
// phase's wide key type, u64 in the partitioner).  It owns the sort's temporary storage, sized once by the library's queries
// for n pairs.
template <class WIDE>
class PairSorter {
    hipStream_t s;
    size_t tmp_bytes;
    DBuf<char> tmp;
    template <class K, class V>
    size_t query(const K *kin, K *kout, const V *vin, V *vout, int m, int end_bit) const {   // (a host call, nothing is launched)
        size_t b = 0;
        SA_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, b, kin, kout, vin, vout, m, 0, end_bit, s));
        return b;
    }

  public:
    // key_bits, label_bits: the widest bit range the phase sorts WIDE keys and int keys over (label_bits 0: it sorts no int keys)
    PairSorter(hipStream_t s_, int n, int key_bits, int label_bits = 0) : s(s_) {
        const int *ci = nullptr;
        int *i = nullptr;
        tmp_bytes = query((const WIDE *)nullptr, (WIDE *)nullptr, ci, i, n, key_bits);
        if (label_bits) tmp_bytes = std::max(tmp_bytes, query(ci, i, ci, i, n, label_bits));
        tmp.alloc(tmp_bytes + 16);
    }
    // (kout, vout) = the first m <= n pairs of (kin, vin), stably ordered by the bits [0, end_bit) of the keys
    template <class K, class V>
    void sort(const K *kin, K *kout, const V *vin, V *vout, int m, int end_bit) {
        // tmp was sized by the queries for n pairs and serves the m <= n of this call.  That rests on the assumption that the
        // sort never asks for more temporary storage for fewer pairs or fewer bits; the library chooses its path by the count,
        // so the assumption is checked by a query for this call and not relied on.
        size_t b = query(kin, kout, vin, vout, m, end_bit);
        SA_REQUIRE(b <= tmp_bytes, "the sort asks for more temporary storage than the phase sized it for");
        SA_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs((void *)tmp.p, b, kin, kout, vin, vout, m, 0, end_bit, s));
    }
};

// stable sort of the pairs (key[i], i) by key, keys in [0, nkeys); out_vals = the permutation.  n = 0 does nothing;
// otherwise it synchronises the stream (the temporaries go out of scope).
inline void stable_sort_by_key(hipStream_t s, int n, const int *key, int nkeys, int *out_vals) {
    if (n == 0) return;
    DBuf<int> iota((size_t)n), keys_out((size_t)n);
    dev_iota(s, n, 1, iota.p);
    PairSorter<int> sorter(s, n, bits_for(nkeys));
    sorter.sort(key, keys_out.p, (const int *)iota.p, out_vals, n, bits_for(nkeys));
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
