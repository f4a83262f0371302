// The SELL-64 copy of a device CSR operator, DCsr::sell: build_sell fills it, the SpMV family of sparse.hip reads it.
#pragma once
namespace saamge_amd {

constexpr int SELL_SEG_MAX = 16;      // segments per staged tile
constexpr int SELL_STAGE_CAP = 3584;  // doubles of x one tile may stage (28 KB of LDS)
constexpr int SELL_PMAX = 16;         // row patterns per staged tile (Sell::Stage::row_pat)

// (Sell() is "no copy": build_sell starts from one, so that a rebuild inherits nothing.  Included by common.h.)
struct Sell {
    // optional SELL-64 copy for the SpMV family: slice s = rows 64s..64s+63, entry (k, lane)
    // at ptr[s] + 64 k + lane (padded with zero values), fully coalesced per wavefront
    bool built = false; int nslices = 0; int64_t size = 0;
    DBuf<roff_t> ptr; DBuf<int> col; DBuf<double> val;
    // coded slices: <= 64 distinct offsets col - row -> tab[64 s + code], one byte per entry
    // in code (four consecutive entries of a row per word); ntab[s] = -1: plain slice
    // pair-coded slices (ntab >= 256): <= 64 distinct (offset, VALUE) pairs, vtab holds the values
    DBuf<int> ntab, tab; DBuf<unsigned> code; DBuf<double> vtab;
    // census of the copy (build_sell): slices and stored entries per format [pair-coded, offset-coded, plain], the
    // bytes of matrix data one application streams in the formats in use, and whether the short-chain path of the
    // pair-coded slices may be used (32-bit byte offsets into x)
    int64_t class_slices[3] = {0, 0, 0}, class_entries[3] = {0, 0, 0};
    double stream_bytes = 0.0; bool fast_ok = false;
    // operator-level pair dictionary (sell_gdict_kernel): an operator none of whose slices could be coded per slice but
    // whose (offset, value) pairs repeat across the WHOLE operator (a uniform high-order mesh: Q2 elasticity has 243
    // entries per row and ~4 900 distinct pairs) stores a 16-bit code per entry into one table of 16-byte pairs:
    // 2 B instead of 12 B per stored entry.  gcode: four codes of a row per 8-byte word, laid out like Sell::code.
    struct Dict {
        bool on = false;
        bool bs3 = false;         // 3 x 3 node blocks: the lanes of a node share their gathers of x (sell_gpair_kernel)
        int nirr = 0;             // rows outside regular node blocks ...
        DBuf<int> irr;            // ... listed: sell_gpair3_fix_kernel redoes them
        int ng = 0;
        DBuf<unsigned long long> gcode;
        DBuf<double2> gtab;       // {offset (as the low 32 bits of .x's pattern), value}: see GPair in sparse.hip
    } dict;
    // x-staging of the pair-coded slices (sell_stage_kernel): a TILE = 4 consecutive slices = the 256 rows of one workgroup.
    // Where the column offsets of a tile cluster into few runs (a stencil: 9), the x-entries those runs touch are
    // contiguous segments: tile_nseg[t] of them (0: not staged), tile_seg[SELL_SEG_MAX t + s] = {first offset
    // relative to the tile's first row, doubles to load}; the workgroup loads them into LDS with wide coalesced loads
    // and the products read LDS instead of gathering from global memory.  cap = doubles of the largest tile.
    struct Stage {
        DBuf<int> tile_nseg;
        DBuf<int2> tile_seg;
        int cap = 0;
        bool one_table = false;   // every staged tile shares one pair table among its four slices
        DBuf<int> unstaged;       // tiles left to the gather kernel (nunstaged of them)
        int nunstaged = 0;
        // sell_staged2_kernel (one-table operators): the staged tiles' code words once more in a regular layout (word q of thread t
        // of tile T at (T wq + q) 256 + t) and one descriptor word per tile (segments | the four slice widths)
        int wq = 0;
        DBuf<unsigned> codeR;
        DBuf<int> tile_desc;
        // row patterns (sell_row_patterns_kernel; Options::sell bit 6 set: none): the distinct code-word rows of a staged tile,
        // at most SELL_PMAX of them, in tile_pat[(T SELL_PMAX + p) 8 + q] (zero past wq words and past the tile's count),
        // and one byte per row, row_pat[256 T + t], naming its pattern.  tile_pinfo[T] > 0: the pattern count;
        // <= 0: the tile has more patterns and keeps its code words in codeR at slot -tile_pinfo[T] (then only such
        // tiles have slots there).  Census: pattern tiles and the largest count.
        DBuf<unsigned char> row_pat; DBuf<unsigned> tile_pat; DBuf<int> tile_pinfo;
        int pat_tiles = 0, pat_max = 0;
        bool on() const { return cap > 0; }                 // the operator runs the staged kernels
        bool regular() const { return cap > 0 && wq > 0; }  // ... sell_staged2_kernel, from codeR / the patterns
        bool patterns() const { return row_pat.p != nullptr; }
    } stage;
    // the smoother's diagonal factor as byte codes into a table of <= 256 values (operators whose rows repeat: a 256-row tile
    // then reads 256 bytes of it instead of 2 KB); src: the array the codes were made from (build_dinv_codes)
    struct DCode {
        DBuf<unsigned char> code;
        DBuf<unsigned long long> tab;
        const double *src = nullptr;
        bool for_(const double *dinv) const { return dinv && code.p && dinv == src; }   // `dinv` is read through the codes
    } dcode;
};
}  // namespace saamge_amd
