// How a list of k columns is dealt to the block kernels (sparse.hip, cycle.hip): chunks of at most BLOCK_MAX columns, each
// run by the narrowest instantiated kernel width that holds it; the slots past the chunk's columns are masked (never stored)
// and point at the chunk's first column, so that every load a kernel makes for them stays valid.  Plain constexpr C++: the
// rule is held on the CPU by tests/test_cxx_cycle_block.py.
#pragma once

namespace saamge_amd {

constexpr int BLOCK_MAX = 8;                        // columns of one kernel launch
constexpr int BLOCK_WIDTHS[] = {1, 2, 4, 8};        // 1: the single-vector kernels; 2, 4, 8: the instantiated block kernels

// the narrowest width that holds n columns (1 <= n <= BLOCK_MAX)
constexpr int block_width(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : 8; }
constexpr int block_num_chunks(int k) { return (k + BLOCK_MAX - 1) / BLOCK_MAX; }

struct BlockChunk {
    int first, count, width;      // columns [first, first + count) of the list in a kernel of `width` slots
    unsigned mask;                // bit j set: slot j is a column of the list and is stored
};
constexpr BlockChunk block_chunk(int k, int c) {
    const int first = c * BLOCK_MAX;
    const int count = k - first < BLOCK_MAX ? k - first : BLOCK_MAX;
    return BlockChunk{first, count, block_width(count), (1u << count) - 1u};
}
// the column of the list that slot j of the chunk points at
constexpr int block_slot_column(const BlockChunk &ch, int j) { return j < ch.count ? ch.first + j : ch.first; }

}  // namespace saamge_amd
