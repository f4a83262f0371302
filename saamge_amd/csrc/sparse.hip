// CSR SpMV family for gfx950: L lanes of a 64-wide wavefront cooperate on one row
// (L chosen from the average row length), val/col streamed with non-temporal loads so
// the XCD L2 keeps the gathered x entries, fused epilogues for the residual, the
// prolongation-add and the polynomial-smoother step.  HBM-bound: 12 B per nonzero.
#include "sparse.h"
#include "devtab.h"
#include <array>
#include <climits>

namespace saamge_amd {

enum { MODE_PLAIN = 0, MODE_RESIDUAL = 1, MODE_ADD = 2, MODE_SMOOTH = 3 };

// ---- what every kernel of the family shares --------------------------------------------------------------------------
// The vectors of one application as a kernel indexes them: x by column, the others by the row a kernel computes (xrow: x at
// those rows).  row_terms takes them as one bundle, filled from the kernel's own __restrict__ parameters.
struct SpmvVecs {
    const double *x;
    double *y;
    const double *b, *dinv;
    double scale;
    const double *xrow;
};
// The row's terms of the four modes: y = sum / b - sum / y + sum / x + scale * dinv_neg * (sum - b).  row_terms loads what the
// mode needs for a live row, spmv_epilogue stores.  The kernels behind the fine smoother -- sell_slice, sell_staged_kernel,
// sell_staged2 -- load their terms themselves, each where its own streams want them (sell_staged2 also in its own way), and
// share the epilogue: through row_terms, as through argument bundles, a shared staging routine or a shared product loop, the
// instruction stream of sell_staged2_kernel<3> is no longer the measured one (profiles/spmv_refactor_resource_usage.txt).
struct RowTerms { double b, d, x; };
template <int MODE>
__device__ __forceinline__ RowTerms row_terms(const SpmvVecs &v, long row, bool live = true) {
    RowTerms t{0.0, 0.0, 0.0};
    if (MODE == MODE_RESIDUAL && live) t.b = v.b[row];
    if (MODE == MODE_ADD && live) t.x = v.y[row];
    if (MODE == MODE_SMOOTH && live) { t.b = v.b[row]; t.d = v.dinv[row]; t.x = v.xrow[row]; }
    return t;
}
template <int MODE>
__device__ __forceinline__ void spmv_epilogue(double sum, const RowTerms &t, double scale, double *y, long row) {
    if (MODE == MODE_PLAIN) {
        y[row] = sum;
    } else if (MODE == MODE_RESIDUAL) {
        y[row] = t.b - sum;
    } else if (MODE == MODE_ADD) {
        y[row] = t.x + sum;
    } else {
        y[row] = t.x + scale * (t.d * (sum - t.b));
    }
}
// The XCD deal: consecutive workgroups go to the XCDs round-robin (block -> XCD = block % 8, position = block / 8), so XCD k
// walks the k-th contiguous run of per_xcd tiles (tile_deal on the host; 0: no deal).
__device__ __forceinline__ int xcd_block(int per_xcd) {
    return per_xcd > 0 ? (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
}

template <int L, int MODE>
__global__ __launch_bounds__(256) void spmv_kernel(int nrows, const roff_t *__restrict__ rowptr,
                                                   const int *__restrict__ col,
                                                   const double *__restrict__ val,
                                                   const double *__restrict__ x,
                                                   double *__restrict__ y,
                                                   const double *__restrict__ b,
                                                   const double *__restrict__ dinv, double scale,
                                                   const double *__restrict__ xrow) {
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (L - 1);
    const long row = gtid / L;
    if (row >= nrows) return;  // whole L-group leaves together (256 % L == 0)
    const roff_t beg = rowptr[row], end = rowptr[row + 1];
    double sum = 0.0;
    for (roff_t k = beg + lane; k < end; k += L) {
        const double v = __builtin_nontemporal_load(val + k);
        const int c = __builtin_nontemporal_load(col + k);
        sum = fma(v, x[c], sum);
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    const SpmvVecs v{x, y, b, dinv, scale, xrow};
    if (lane == 0) spmv_epilogue<MODE>(sum, row_terms<MODE>(v, row), scale, y, row);
}

// SELL-64: one lane per row, the wavefront walks its slice column by column; val/col loads are
// 512 B / 256 B contiguous per step and, for stencil-like matrices, so are the x gathers.
// Slices whose entries use at most 64 distinct column offsets (col - row) -- every slice of a
// stencil matrix -- carry ONE BYTE per entry instead of the 4-byte column: a code into the slice's
// offset table, which sits one entry per lane in a register and is read with a cross-lane
// permute.  9 instead of 12 bytes per stored entry on the level that dominates the solve.
// pair-coded slices: ntab = 256 + pairs (own table at tab[64 slice ..]) or 512 + pairs (the table of the slice's tile of
// four, at the tile's first slice: sell_code_kernel's merge)
__device__ __forceinline__ int pair_count(int nt) { return nt >= 512 ? nt - 512 : nt - 256; }
__device__ __forceinline__ size_t pair_table_at(int gslice, int nt) { return (size_t)(nt >= 512 ? (gslice & ~3) : gslice) * 64; }
// A lane's first code word: the codes of four consecutive entries of a row share one word, the words of a slice that starts at
// entry `beg` sit at codes[beg / 4 + 64 gslice + 64 (k / 4) + lane] (Sell::code, and Sell::Dict::gcode with 8-byte words).
template <class W>
__device__ __forceinline__ W *code_words(W *codes, roff_t beg, int gslice, int lane) {
    return codes + ((size_t)(beg >> 2) + (size_t)gslice * 64 + lane);
}
// All code words of a row of at most 32 entries, requested before the first one is used (a loop would wait for one word per
// trip: load -> look-up -> gather is a dependent chain); zero past the row's width.
__device__ __forceinline__ void load_code_words(const unsigned *wp, int w, unsigned (&cws)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) cws[q] = (4 * q < w) ? __builtin_nontemporal_load(wp + 64 * q) : 0u;
}

// general path: any mix of slice formats, any width.  Returns the row's sum; `slice` / `gslice` are wave-uniform.
__device__ __forceinline__ double sell_row_general(int lane, int grow, int gslice, roff_t beg, roff_t end, int nt,
                                                   const int *__restrict__ col, const double *__restrict__ val,
                                                   const int *__restrict__ tab, const unsigned *__restrict__ codes,
                                                   const double *__restrict__ x, const double *__restrict__ vtab) {
    const int *cp = col + beg + lane;
    const double *vp = val + beg + lane;
    const int w = (int)((end - beg) >> 6);
    double s0 = 0.0, s1 = 0.0;
    int k = 0;
    if (nt >= 256) {
        // pair-coded slice: the byte indexes a table of (offset, VALUE) pairs -- at most 64 distinct ones in
        // the slice, which is every slice of a constant-coefficient stencil matrix (the whole fine level of the
        // headline problem).  Neither columns nor values are streamed: 1 byte per stored entry instead of 12.
        const int np = pair_count(nt);
        const int mytab = (lane < np) ? tab[pair_table_at(gslice, nt) + lane] : 0;
        const double myval = (lane < np) ? vtab[pair_table_at(gslice, nt) + lane] : 0.0;
        const unsigned *wp = code_words(codes, beg, gslice, lane);
        auto quad = [&](unsigned cw) {
            const int i0 = (int)(cw & 255u), i1 = (int)((cw >> 8) & 255u), i2 = (int)((cw >> 16) & 255u), i3 = (int)(cw >> 24);
            const int c0 = grow + __shfl(mytab, i0), c1 = grow + __shfl(mytab, i1);
            const int c2 = grow + __shfl(mytab, i2), c3 = grow + __shfl(mytab, i3);
            const double v0 = __shfl(myval, i0), v1 = __shfl(myval, i1), v2 = __shfl(myval, i2), v3 = __shfl(myval, i3);
            s0 = fma(v0, x[c0], s0);
            s1 = fma(v1, x[c1], s1);
            s0 = fma(v2, x[c2], s0);
            s1 = fma(v3, x[c3], s1);
        };
        if (w <= 32) {
            // every code word of the row is requested before the first one is used (the loop would wait for one
            // word per trip: load -> permute -> gather is a dependent chain)
            unsigned cws[8];
            load_code_words(wp, w, cws);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (4 * q + 4 <= w) quad(cws[q]);
                else if (4 * q < w) {
                    unsigned cw = cws[q];
                    for (int kk = 4 * q; kk < w; ++kk, cw >>= 8) {
                        const int i0 = (int)(cw & 255u);
                        s0 = fma(__shfl(myval, i0), x[grow + __shfl(mytab, i0)], s0);
                    }
                }
            }
            k = w;
        }
        for (; k + 4 <= w; k += 4) quad(__builtin_nontemporal_load(wp + 16 * k));
        if (k < w) {
            unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            for (; k < w; ++k, cw >>= 8) {
                const int i0 = (int)(cw & 255u);
                s0 = fma(__shfl(myval, i0), x[grow + __shfl(mytab, i0)], s0);
            }
        }
    } else if (nt >= 0) {
        const int mytab = tab[(size_t)gslice * 64 + lane];
        const unsigned *wp = code_words(codes, beg, gslice, lane);
        for (; k + 4 <= w; k += 4) {
            const unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            const double v0 = __builtin_nontemporal_load(vp + 64 * k), v1 = __builtin_nontemporal_load(vp + 64 * (k + 1));
            const double v2 = __builtin_nontemporal_load(vp + 64 * (k + 2)), v3 = __builtin_nontemporal_load(vp + 64 * (k + 3));
            const int c0 = grow + __shfl(mytab, (int)(cw & 255u)), c1 = grow + __shfl(mytab, (int)((cw >> 8) & 255u));
            const int c2 = grow + __shfl(mytab, (int)((cw >> 16) & 255u)), c3 = grow + __shfl(mytab, (int)(cw >> 24));
            s0 = fma(v0, x[c0], s0);
            s1 = fma(v1, x[c1], s1);
            s0 = fma(v2, x[c2], s0);
            s1 = fma(v3, x[c3], s1);
        }
        if (k < w) {
            unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            for (; k < w; ++k, cw >>= 8)
                s0 = fma(__builtin_nontemporal_load(vp + 64 * k), x[grow + __shfl(mytab, (int)(cw & 255u))], s0);
        }
    }
    for (; k + 4 <= w; k += 4) {
        const int c0 = __builtin_nontemporal_load(cp + 64 * k), c1 = __builtin_nontemporal_load(cp + 64 * (k + 1));
        const int c2 = __builtin_nontemporal_load(cp + 64 * (k + 2)), c3 = __builtin_nontemporal_load(cp + 64 * (k + 3));
        const double v0 = __builtin_nontemporal_load(vp + 64 * k), v1 = __builtin_nontemporal_load(vp + 64 * (k + 1));
        const double v2 = __builtin_nontemporal_load(vp + 64 * (k + 2)), v3 = __builtin_nontemporal_load(vp + 64 * (k + 3));
        s0 = fma(v0, x[c0], s0);
        s1 = fma(v1, x[c1], s1);
        s0 = fma(v2, x[c2], s0);
        s1 = fma(v3, x[c3], s1);
    }
    for (; k < w; ++k) s0 = fma(__builtin_nontemporal_load(vp + 64 * k), x[__builtin_nontemporal_load(cp + 64 * k)], s0);
    return s0 + s1;
}

struct alignas(16) PairEntry {
    int off, pad;
    double val;
};
// (Measured, round 4: the whole 16-byte entry with ONE LDS instruction -- ds_read_b128 instead of the ds_read_b32 + ds_read_b64 a
// member-wise read becomes -- 233 against 230 us per fine-level smoother step: the LDS data path, not its instruction count.)

// ---- the SELL-64 kernels of the whole SpMV family: one wavefront per slice, one lane per row ----------------------
// What bounds them (MI355X, 257^3 rows x 27 entries, counters + tools/spmv_lab, tools/vmem_rate): not HBM.  A
// vector-memory wave-instruction of 8 or 16 bytes per lane occupies the CU's address / L1 path for ~17 cycles
// whatever it returns (4 bytes per lane: 5-9), and a row-per-lane SpMV issues one such instruction PER STORED ENTRY
// for the gather of x: 27 + 17 others per slice = ~620 of the ~890 cycles a CU spends per slice, at 2.9 TB/s of the
// bytes the format needs (a pure stream of the same bytes: 5.1 TB/s).  Before that the cross-lane permutes of the
// table look-ups (96 LDS instructions x 8 cycles per slice) held the same place.  Hence:
//   * sell_staged_kernel, sell_staged2_kernel: where the offsets of a 256-row tile cluster into few runs, the workgroup
//     loads the x-segments those runs touch into LDS with 16-byte coalesced loads (27 gathers per wavefront -> ~7 loads) and the products
//     read LDS; the slice's (offset, value) table sits in LDS too, one 16-byte entry per lane, read with plain LDS
//     loads (a broadcast for the lanes that share an entry) instead of three permutes per entry.
//   * sell_slice: the same per slice with gathers from global memory (tiles that cannot be staged), up to 16 in
//     flight; offset-coded, plain and wide slices go through sell_row_general.
//   * Consecutive workgroups are dealt to the XCDs round-robin (block -> XCD = block % 8, position = block / 8): XCD k
//     walks the k-th contiguous eighth of the tiles, so that the x-planes a stencil row touches are fetched into ONE L2
//     instead of all eight (PMC: 2.0 -> 1.14 GB per launch, the format's own bytes being 1.12 GB; speed only, any
//     placement gives the same result).
//   * The slice is wave-uniform (readfirstlane): its offsets, width and format come through the scalar cache.
// Same arithmetic and THE order of additions of the whole family on every path, so that all formats give the same bits: two
// accumulators over whole groups of four entries -- even entries into the first, odd ones into the second -- the tail of up to
// three entries into the first, then their sum.
template <int MODE>
__device__ __forceinline__ void sell_slice(PairEntry *lt, int nrows, int row0, long row, int slice, int fast_ok,
                                           const roff_t *__restrict__ sptr, const int *__restrict__ col,
                                           const double *__restrict__ val, const int *__restrict__ ntab,
                                           const int *__restrict__ tab, const unsigned *__restrict__ codes,
                                           const double *__restrict__ x, double *__restrict__ y,
                                           const double *__restrict__ b, const double *__restrict__ dinv, double scale,
                                           const double *__restrict__ xrow, const double *__restrict__ vtab) {
    const int lane = threadIdx.x & 63;
    if ((long)slice * 64 >= nrows) return;
    const roff_t beg = sptr[slice], end = sptr[slice + 1];
    const int gslice = (row0 >> 6) + slice;
    const int nt = ntab[gslice];
    const int w = (int)((end - beg) >> 6);
    const bool live = row < nrows;
    const int grow = row0 + (int)row;
    double e_b = 0.0, e_d = 0.0, e_x = 0.0, sum;
    if (fast_ok && nt >= 256 && w <= 32) {
        const int np = pair_count(nt);
        const unsigned *wp = code_words(codes, beg, gslice, lane);
        unsigned cws[8];
        load_code_words(wp, w, cws);
        const int mytab = (lane < np) ? tab[pair_table_at(gslice, nt) + lane] : 0;
        const double myval = (lane < np) ? vtab[pair_table_at(gslice, nt) + lane] : 0.0;
        if (MODE == MODE_RESIDUAL && live) e_b = b[row];
        if (MODE == MODE_ADD && live) e_x = y[row];
        if (MODE == MODE_SMOOTH && live) { e_b = b[row]; e_d = dinv[row]; e_x = xrow[row]; }
        lt[lane] = PairEntry{mytab, 0, myval};      // (a region private to this wavefront)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const char *xb = (const char *)x;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (16 * h < w) {
                double xs[16], vs[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int idx = (int)((cws[4 * h + (j >> 2)] >> (8 * (j & 3))) & 255u);
                    const PairEntry e = lt[idx];
                    vs[j] = e.val;
                    // (entries past the slice's width carry code 0: no address is formed from them -- table entry 0 belongs
                    // to the tile's FIRST row and can point outside x from a later one)
                    xs[j] = (16 * h + j < w) ? *(const double *)(xb + ((unsigned)(grow + e.off) << 3)) : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (16 * h + j < w) {
                        if ((j & 1) && 16 * h + j < (w & ~3)) s1 = fma(vs[j], xs[j], s1);
                        else s0 = fma(vs[j], xs[j], s0);
                    }
                }
            }
        }
        sum = s0 + s1;
    } else {
        sum = sell_row_general(lane, grow, gslice, beg, end, nt, col, val, tab, codes, x, vtab);
        if (MODE == MODE_RESIDUAL && live) e_b = b[row];
        if (MODE == MODE_ADD && live) e_x = y[row];
        if (MODE == MODE_SMOOTH && live) { e_b = b[row]; e_d = dinv[row]; e_x = xrow[row]; }
    }
    if (!live) return;
    spmv_epilogue<MODE>(sum, RowTerms{e_b, e_d, e_x}, scale, y, row);
}

template <int MODE>
__global__ __launch_bounds__(256) void sell_spmv_kernel(int nrows, int row0, int nblocks, int per_xcd, int fast_ok,
                                                        const roff_t *__restrict__ sptr,
                                                        const int *__restrict__ col,
                                                        const double *__restrict__ val,
                                                        const int *__restrict__ ntab,
                                                        const int *__restrict__ tab,
                                                        const unsigned *__restrict__ codes,
                                                        const double *__restrict__ x,
                                                        double *__restrict__ y,
                                                        const double *__restrict__ b,
                                                        const double *__restrict__ dinv, double scale,
                                                        const double *__restrict__ xrow,
                                                        const double *__restrict__ vtab) {
    __shared__ PairEntry ltab[4][64];
    const int blk = xcd_block(per_xcd);
    if (blk >= nblocks) return;
    const long row = (long)blk * 256 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane((int)(row >> 6));
    sell_slice<MODE>(ltab[threadIdx.x >> 6], nrows, row0, row, slice, fast_ok, sptr, col, val, ntab, tab, codes, x, y, b,
                     dinv, scale, xrow, vtab);
}

// Staged tiles only (the others are left to sell_tiles_kernel).  row0 must be a multiple of 256 (tiles are global);
// dynamic LDS: stage_cap doubles + 4 slice tables.
template <int MODE>
__global__ __launch_bounds__(256) void sell_staged_kernel(int nrows, int row0, int nblocks, int per_xcd, int stage_cap,
                                                          int ncols, int one_table, const roff_t *__restrict__ sptr,
                                                          const int *__restrict__ ntab,
                                                          const int *__restrict__ tab,
                                                          const unsigned *__restrict__ codes,
                                                          const double *__restrict__ x,
                                                          double *__restrict__ y,
                                                          const double *__restrict__ b,
                                                          const double *__restrict__ dinv, double scale,
                                                          const double *__restrict__ xrow,
                                                          const double *__restrict__ vtab,
                                                          const int *__restrict__ tile_nseg,
                                                          const int2 *__restrict__ tile_seg) {
    extern __shared__ __align__(16) double lds[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // one_table: every staged tile of the operator shares one pair table among its four slices -- 1 KB of LDS for it
    // instead of 4 (one more workgroup per CU); the wavefront's row offset then goes into the x-address, not the table
    PairEntry *lt = (PairEntry *)(lds + stage_cap) + (one_table ? 0 : 64 * wv);
    const int blk = per_xcd > 0 ? (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (blk >= nblocks || (long)blk * 256 + 256 > nrows) return;
    const long row = (long)blk * 256 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane((int)(row >> 6));
    const int gtile = (row0 >> 8) + blk;
    const int nseg = tile_nseg[gtile];
    if (nseg == 0) return;
    // this slice's streams first: they are in flight while the segments are staged
    const roff_t beg = sptr[slice], end = sptr[slice + 1];
    const int gslice = (row0 >> 6) + slice;
    const int nt = ntab[gslice];
    const int np = pair_count(nt);
    const int w = (int)((end - beg) >> 6);
    unsigned cws[8];
    load_code_words(code_words(codes, beg, gslice, lane), w, cws);
    const int mytab = (lane < np) ? tab[pair_table_at(gslice, nt) + lane] : 0;
    const double myval = (lane < np) ? vtab[pair_table_at(gslice, nt) + lane] : 0.0;
    const RowTerms t = row_terms<MODE>(SpmvVecs{x, y, b, dinv, scale, xrow}, row);
    // the tile's segments: x[R0 + lo .. R0 + lo + len) -> lds[pre ..), 16 bytes per lane (starts and lengths are even).
    // Four segments at a time: the loads of their first two passes (512 doubles per pass of the workgroup), then the
    // LDS stores -- one memory latency per batch, not one per segment; the thread assignment rotates by one wavefront
    // per segment so that the partial last passes land on different wavefronts.
    const int2 *sg = tile_seg + (size_t)gtile * SELL_SEG_MAX;
    const int R0 = row0 + blk * 256;
    auto fetch = [&](int g) {
        // (a tile's table is the union over its rows: near the ends of the operator a segment reaches outside
        // [0, ncols), where no row of the tile has an entry)
        double2 v = make_double2(0.0, 0.0);
        if (g >= 0 && g + 1 < ncols) v = *(const double2 *)(x + g);
        else if (g >= 0 && g < ncols) v.x = x[g];
        else if (g == -1 && ncols > 0) v.y = x[0];
        return v;
    };
    int pre = 0, mybase = 0;
    bool longer = false;
#pragma unroll
    for (int batch = 0; batch < SELL_SEG_MAX; batch += 4) {
        if (batch < nseg) {
            double2 st[8];
            int pre_k[4], len_k[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sidx = batch + k;
                pre_k[k] = pre;
                len_k[k] = 0;
                if (sidx < nseg) {
                    const int2 d = sg[sidx];
                    len_k[k] = d.y;
                    const int i = 2 * (int)((threadIdx.x + 64u * sidx) & 255u);
                    if (i < d.y) st[2 * k] = fetch(R0 + d.x + i);
                    if (i + 512 < d.y) st[2 * k + 1] = fetch(R0 + d.x + i + 512);
                    longer = longer || d.y > 1024;
                    if (mytab >= d.x) mybase = pre - d.x;      // (segments ascend: the last one at or below the offset holds it)
                    pre += d.y;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 2 * (int)((threadIdx.x + 64u * (batch + k)) & 255u);
                if (i < len_k[k]) *(double2 *)(lds + pre_k[k] + i) = st[2 * k];
                if (i + 512 < len_k[k]) *(double2 *)(lds + pre_k[k] + i + 512) = st[2 * k + 1];
            }
        }
    }
    if (longer) {      // segments beyond two passes (1024 doubles): the rest of them
        int p2 = 0;
        for (int sidx = 0; sidx < nseg; ++sidx) {
            const int2 d = sg[sidx];
            for (int i = 2 * (int)((threadIdx.x + 64u * sidx) & 255u) + 1024; i < d.y; i += 512) *(double2 *)(lds + p2 + i) = fetch(R0 + d.x + i);
            p2 += d.y;
        }
    }
    // byte offset of the x-entry of the wavefront's (one_table: the tile's) first row in lds
    if (!one_table) lt[lane] = PairEntry{(mybase + mytab + 64 * wv) << 3, 0, myval};
    else if (wv == 0) lt[lane] = PairEntry{(mybase + mytab) << 3, 0, myval};
    __syncthreads();
    const char *lb = (const char *)lds + 8 * (lane + (one_table ? 64 * wv : 0));
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        if (4 * g + 4 <= w) {
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                const PairEntry e = lt[(cws[g] >> (8 * e4)) & 255u];
                const double xv = *(const double *)(lb + e.off);
                if (e4 & 1) s1 = fma(e.val, xv, s1);
                else s0 = fma(e.val, xv, s0);
            }
        } else if (4 * g < w) {
#pragma unroll
            for (int e4 = 0; e4 < 3; ++e4) {
                if (4 * g + e4 < w) {
                    const PairEntry e = lt[(cws[g] >> (8 * e4)) & 255u];
                    s0 = fma(e.val, *(const double *)(lb + e.off), s0);
                }
            }
        }
    }
    const double sum = s0 + s1;
    spmv_epilogue<MODE>(sum, t, scale, y, row);
}

// ---- the staged kernel with descriptor-free streams (round 4) -------------------------------------------------------
// sell_staged_kernel starts with a chain: scalar loads of the slice's offset, width and table size (streaming data: they miss
// every cache), THEN the vector loads whose addresses they give -- two memory latencies before the first product, a quarter
// of a tile's ~8 us life at eight workgroups per CU (SQ_WAIT_ANY 66 %, round 3's counters).  Here the code words of the
// staged tiles live a second time in a REGULAR layout -- word q of the row of thread t of tile T at (T wq + q) 256 + t, wq =
// the widest staged row in words -- and the widths of the four slices ride in one descriptor word per tile next to the
// segment count: codes, right-hand side, diagonal, x-row and the tile's one table are requested before any descriptor
// has arrived; only the x-segments wait for their (scalar-loaded) descriptors.  Operators whose staged tiles all share one
// table per tile (Sell::Stage::one_table); same products in the same order as sell_staged_kernel.
// pinfo (row patterns, sell_row_patterns_kernel): code words only for the tiles that have no patterns, at their slot.
__global__ __launch_bounds__(256) void sell_regular_codes_kernel(int ntiles, int wq, int ncols, const roff_t *__restrict__ sptr,
                                                                 const int *__restrict__ tile_nseg, const int2 *__restrict__ tile_seg,
                                                                 const unsigned *__restrict__ codes, const int *__restrict__ pinfo,
                                                                 unsigned *__restrict__ codesR, int *__restrict__ tile_desc) {
    const int t = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nseg = tile_nseg[t];
    if (nseg == 0) {
        if (threadIdx.x == 0) tile_desc[t] = 0;
        return;
    }
    const int slice = 4 * t + wv;
    const roff_t beg = sptr[slice];
    const int w = (int)((sptr[slice + 1] - beg) >> 6);
    const unsigned *wp = code_words(codes, beg, slice, lane);
    const int slot = pinfo ? -pinfo[t] : t;
    if (slot >= 0)
        for (int q = 0; q < wq; ++q) codesR[((size_t)slot * wq + q) * 256 + threadIdx.x] = (4 * q < w) ? wp[64 * q] : 0u;
    __shared__ int ws[4];
    if (lane == 0) ws[wv] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        // bit 7: every segment lies inside x[0 .. ncols) -- the staging loads of such a tile (all but the first and last few
        // of an operator) need no bounds checks
        bool inside = true;
        for (int q = 0; q < nseg; ++q) {
            const int2 d = tile_seg[(size_t)t * SELL_SEG_MAX + q];
            const long g0 = (long)t * 256 + d.x;
            inside = inside && g0 >= 0 && g0 + d.y <= ncols;
        }
        tile_desc[t] = nseg | (inside ? 128 : 0) | (ws[0] << 8) | (ws[1] << 14) | (ws[2] << 20) | (ws[3] << 26);
    }
}

// Row patterns of the staged tiles (Sell::Stage::row_pat), one workgroup per tile at a time.  The code words of a 256-row tile of a
// constant-coefficient stencil repeat: the interior rows share one sequence, only rows at line ends and near boundary faces
// differ.  Pattern p is the row of the p-th row (in row order) that equals none before it: round p takes the first row not
// yet named (a ballot per wavefront: one barrier per round, no atomics), and every unnamed row compares its words, zero
// padding included, with that one's.  A tile with more than SELL_PMAX patterns takes a slot for its code words in codeR
// instead (census[0] counts the slots); census[1]: pattern tiles, census[2]: the largest count, census[3]: the code words of
// the pattern tiles' slices (no longer streamed).  (A workgroup walks many tiles and adds to the census once: one atomic per
// tile on the same word took 2.4 ms for the 66 307 tiles of the headline.)
__global__ __launch_bounds__(256) void sell_row_patterns_kernel(int ntiles, int wq, const roff_t *__restrict__ sptr, const int *__restrict__ tile_nseg,
                                                                const unsigned *__restrict__ codes, unsigned char *__restrict__ row_pat,
                                                                unsigned *__restrict__ tile_pat, int *__restrict__ pinfo,
                                                                unsigned long long *__restrict__ census) {
    __shared__ unsigned ws[8][256];
    __shared__ int first[2][4], leaders[SELL_PMAX], nwords;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long ntile = 0, nmax = 0, nw = 0;      // (thread 0's share of the census)
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        if (tile_nseg[t] == 0) {      // (not staged: nothing reads its entries)
            if (threadIdx.x == 0) pinfo[t] = 0;
            continue;
        }
        const int slice = 4 * t + wv;
        const roff_t beg = sptr[slice];
        const int w = (int)((sptr[slice + 1] - beg) >> 6);
        const unsigned *wp = code_words(codes, beg, slice, lane);
        unsigned my[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            my[q] = (q < wq && 4 * q < w) ? wp[64 * q] : 0u;      // (as sell_regular_codes_kernel lays them out)
            ws[q][threadIdx.x] = my[q];
        }
        if (threadIdx.x == 0) nwords = 0;
        __syncthreads();
        if (lane == 0) atomicAdd(&nwords, (w + 3) / 4 * 64);
        int pid = -1, np = 0;
        for (;;) {
            // (two sets of slots: round np + 1 writes the other while a late wavefront may still read this one)
            const unsigned long long open = __ballot(pid < 0);
            if (lane == 0) first[np & 1][wv] = open ? 64 * wv + __ffsll((long long)open) - 1 : 256;
            __syncthreads();
            const int L = min(min(first[np & 1][0], first[np & 1][1]), min(first[np & 1][2], first[np & 1][3]));
            if (L == 256) break;
            if (np == SELL_PMAX) {
                np = SELL_PMAX + 1;
                break;
            }
            if (threadIdx.x == 0) leaders[np] = L;
            if (pid < 0) {
                bool eq = true;
#pragma unroll
                for (int q = 0; q < 8; ++q) eq = eq && my[q] == ws[q][L];
                if (eq) pid = np;
            }
            ++np;
        }
        const bool over = np > SELL_PMAX;
        if (threadIdx.x == 0) {
            if (over) {
                pinfo[t] = -(int)atomicAdd(census, 1ull);
            } else {
                pinfo[t] = np;
                ntile += 1;
                nmax = max(nmax, (unsigned long long)np);
                nw += nwords;
            }
        }
        row_pat[(size_t)t * 256 + threadIdx.x] = over ? 0 : (unsigned char)pid;
        if (threadIdx.x < SELL_PMAX * 8) {
            const int p = threadIdx.x >> 3, q = threadIdx.x & 7;
            tile_pat[(size_t)t * SELL_PMAX * 8 + threadIdx.x] = (!over && p < np) ? ws[q][leaders[p]] : 0u;
        }
        __syncthreads();      // (the tile's tables are read to the end before the next one's overwrite them)
    }
    if (threadIdx.x == 0 && ntile) {
        atomicAdd(census + 1, ntile);
        atomicMax(census + 2, nmax);
        atomicAdd(census + 3, nw);
    }
}

// The few tiles the staging plan leaves out (an operator whose row count is not a multiple of 256: its last tile), done by the
// trailing workgroups of sell_staged2_kernel -- what sell_tiles_kernel does in a launch of its own, 5 us behind every one of
// the 456 smoother steps of the headline's solve for a single row.  Through sell_slice's general path (fast_ok = 0: the same
// sums in the same order; its sixteen gathers in flight would take the kernel from 63 to 84 registers and from eight to six
// workgroups per CU).
struct SellLeftover {
    int grid_main, n;            // workgroups of the staged tiles; tiles left over (0: none are done here)
    const int *tiles;
    const roff_t *sptr;
    const int *col;
    const double *val;
    const int *ntab;
    const unsigned *codes;
};
// PAT: the tiles' row patterns (sell_staged2_kernel); without: every staged tile's code words (sell_staged2_codes_kernel,
// Options::sell bit 6).  Two kernels, not a run-time switch: the code words of the second are in flight across the staging,
// and one body holding both would need 66 registers (seven workgroups per CU instead of eight).
template <int MODE, bool PAT>
__device__ __forceinline__ void sell_staged2(double *lds, const SellLeftover &left, int nrows, int row0, int nblocks, int per_xcd,
                                             int stage_cap, int ncols, int wq, const unsigned *__restrict__ codesR,
                                             const int *__restrict__ tab, const double *__restrict__ vtab,
                                             const int *__restrict__ tile_desc, const int2 *__restrict__ tile_seg,
                                             const double *__restrict__ x, double *__restrict__ y,
                                             const double *__restrict__ b, const double *__restrict__ dinv,
                                             double scale, const double *__restrict__ xrow,
                                             const unsigned char *__restrict__ row_pat, const unsigned *__restrict__ tile_pat,
                                             const int *__restrict__ tile_pinfo,
                                             const unsigned char *__restrict__ dcode, const double *__restrict__ dtab) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int)blockIdx.x >= left.grid_main) {      // (a trailing workgroup: one of the tiles that are not staged)
        const long lrow0 = (long)left.tiles[blockIdx.x - left.grid_main] * 256 - row0;      // the tile's first row, local to the range
        if (lrow0 < 0 || lrow0 >= nrows) return;
        const long trow = lrow0 + threadIdx.x;
        const int slice = __builtin_amdgcn_readfirstlane((int)(trow >> 6));
        sell_slice<MODE>((PairEntry *)lds + 64 * wv, nrows, row0, trow, slice, 0, left.sptr, left.col, left.val, left.ntab, tab, left.codes, x, y,
                         b, dinv, scale, xrow, vtab);
        return;
    }
    PairEntry *lt = (PairEntry *)(lds + stage_cap);
    unsigned *pt = (unsigned *)(lt + 64);      // (row patterns: the tile's SELL_PMAX x 8 pattern words)
    const int blk = xcd_block(per_xcd);
    if (blk >= nblocks || (long)blk * 256 + 256 > nrows) return;
    const long row = (long)blk * 256 + threadIdx.x;
    const int gtile = (row0 >> 8) + blk;
    // every stream whose address the block index gives: requested before any descriptor is looked at.  With row patterns
    // (DCsr::sell_row_pat) that is one byte per row and the tile's pattern table instead of the row's code words: 0.75 instead
    // of 8 KB per tile for the 27-point stencil (whether the tile has patterns is known only from its descriptor: both are
    // requested, and a tile without them reads its code words after the barrier)
    unsigned cws[8];
    int pid = 0;
    unsigned pw = 0u;
    if (PAT) {
        pid = __builtin_nontemporal_load(row_pat + (size_t)gtile * 256 + threadIdx.x);
        if (threadIdx.x < SELL_PMAX * 8) pw = __builtin_nontemporal_load(tile_pat + (size_t)gtile * SELL_PMAX * 8 + threadIdx.x);
    } else {
        const unsigned *wp = codesR + ((size_t)gtile * wq) * 256 + threadIdx.x;
#pragma unroll
        for (int q = 0; q < 8; ++q) cws[q] = (q < wq) ? __builtin_nontemporal_load(wp + 256 * q) : 0u;
    }
    double e_b = 0.0, e_d = 0.0, e_x = 0.0;
    // (b and D^-1 are read once per application: streamed past the caches like the code words, so that the L2 keeps x)
    if (MODE == MODE_RESIDUAL) e_b = __builtin_nontemporal_load(b + row);
    if (MODE == MODE_ADD) e_x = y[row];
    // (the smoother's x-row is x itself at the tile's own rows: taken from the staged segment that holds them, below)
    // (D^-1 as a byte code into a small table where the operator's rows repeat: 1 instead of 8 bytes per row)
    if (MODE == MODE_SMOOTH) { e_b = __builtin_nontemporal_load(b + row); e_d = dcode ? dtab[__builtin_nontemporal_load(dcode + row)] : __builtin_nontemporal_load(dinv + row); }
    int mytab = 0;
    double myval = 0.0;
    if (wv == 0) {          // the tile's one table sits at its first slice
        mytab = tab[(size_t)gtile * 256 + lane];
        myval = vtab[(size_t)gtile * 256 + lane];
    }
    const int desc = tile_desc[gtile];
    const int pinfo = PAT ? tile_pinfo[gtile] : 0;
    const int nseg = desc & 127;
    if (nseg == 0) return;      // (left to sell_tiles_kernel)
    const int w = __builtin_amdgcn_readfirstlane((desc >> (8 + 6 * wv)) & 63);
    const int2 *sg = tile_seg + (size_t)gtile * SELL_SEG_MAX;
    const int R0 = row0 + blk * 256;
    int mybase = 0, zbase = -1;      // zbase: LDS index of x[R0] when a segment holds the tile's own rows
    // the tile's segments x[R0 + lo .. R0 + lo + len) -> lds[pre ..), 16 bytes per lane, four segments per batch (their loads
    // first, then the LDS stores).  CHECK = false: the descriptor says that every segment lies inside x (bit 7)
    auto stage = [&](auto check_tag) {
        constexpr bool CHECK = decltype(check_tag)::value;
        auto fetch = [&](int g) {
            if (!CHECK) return *(const double2 *)(x + g);
            double2 v = make_double2(0.0, 0.0);
            if (g >= 0 && g + 1 < ncols) v = *(const double2 *)(x + g);
            else if (g >= 0 && g < ncols) v.x = x[g];
            else if (g == -1 && ncols > 0) v.y = x[0];
            return v;
        };
        int pre = 0;
        bool longer = false;
#pragma unroll
        for (int batch = 0; batch < SELL_SEG_MAX; batch += 4) {
            if (batch < nseg) {
                double2 st[8];
                int pre_k[4], len_k[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sidx = batch + k;
                    pre_k[k] = pre;
                    len_k[k] = 0;
                    if (sidx < nseg) {
                        const int2 d = sg[sidx];
                        len_k[k] = d.y;
                        const int i = 2 * (int)((threadIdx.x + 64u * sidx) & 255u);
                        if (i < d.y) st[2 * k] = fetch(R0 + d.x + i);
                        if (i + 512 < d.y) st[2 * k + 1] = fetch(R0 + d.x + i + 512);
                        longer = longer || d.y > 1024;
                        if (wv == 0 && mytab >= d.x) mybase = pre - d.x;
                        if (MODE == MODE_SMOOTH && d.x <= 0 && d.x + d.y >= 256) zbase = pre - d.x;
                        pre += d.y;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = 2 * (int)((threadIdx.x + 64u * (batch + k)) & 255u);
                    if (i < len_k[k]) *(double2 *)(lds + pre_k[k] + i) = st[2 * k];
                    if (i + 512 < len_k[k]) *(double2 *)(lds + pre_k[k] + i + 512) = st[2 * k + 1];
                }
            }
        }
        if (longer) {
            int p2 = 0;
            for (int sidx = 0; sidx < nseg; ++sidx) {
                const int2 d = sg[sidx];
                for (int i = 2 * (int)((threadIdx.x + 64u * sidx) & 255u) + 1024; i < d.y; i += 512) *(double2 *)(lds + p2 + i) = fetch(R0 + d.x + i);
                p2 += d.y;
            }
        }
    };
    if (desc & 128) stage(std::false_type());
    else stage(std::true_type());
    if (wv == 0) lt[lane] = PairEntry{(mybase + mytab) << 3, 0, myval};
    if (PAT && threadIdx.x < SELL_PMAX * 8) pt[threadIdx.x] = pw;
    if (MODE == MODE_SMOOTH && zbase < 0) e_x = xrow[row];      // (no segment holds the own rows: an operator without a diagonal run)
    __syncthreads();
    if (MODE == MODE_SMOOTH && zbase >= 0) e_x = lds[zbase + threadIdx.x];
    if (PAT && pinfo > 0) {
        const uint4 c0 = *(const uint4 *)(pt + 8 * pid), c1 = *(const uint4 *)(pt + 8 * pid + 4);
        cws[0] = c0.x; cws[1] = c0.y; cws[2] = c0.z; cws[3] = c0.w;
        cws[4] = c1.x; cws[5] = c1.y; cws[6] = c1.z; cws[7] = c1.w;
    } else if (PAT) {      // (more than SELL_PMAX patterns: the tile's code words, at its slot)
        const unsigned *wp = codesR + ((size_t)(-pinfo) * wq) * 256 + threadIdx.x;
#pragma unroll
        for (int q = 0; q < 8; ++q) cws[q] = (q < wq) ? __builtin_nontemporal_load(wp + 256 * q) : 0u;
    }
    const char *lb = (const char *)lds + 8 * (lane + 64 * wv);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        if (4 * g + 4 <= w) {
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                const PairEntry e = lt[(cws[g] >> (8 * e4)) & 255u];
                const double xv = *(const double *)(lb + e.off);
                if (e4 & 1) s1 = fma(e.val, xv, s1);
                else s0 = fma(e.val, xv, s0);
            }
        } else if (4 * g < w) {
#pragma unroll
            for (int e4 = 0; e4 < 3; ++e4) {
                if (4 * g + e4 < w) {
                    const PairEntry e = lt[(cws[g] >> (8 * e4)) & 255u];
                    s0 = fma(e.val, *(const double *)(lb + e.off), s0);
                }
            }
        }
    }
    const double sum = s0 + s1;
    spmv_epilogue<MODE>(sum, RowTerms{e_b, e_d, e_x}, scale, y, row);
}
#define SA_STAGED2_PARAMS                                                                                                         \
    SellLeftover left, int nrows, int row0, int nblocks, int per_xcd, int stage_cap, int ncols, int wq,                           \
        const unsigned *__restrict__ codesR, const int *__restrict__ tab, const double *__restrict__ vtab,                        \
        const int *__restrict__ tile_desc, const int2 *__restrict__ tile_seg, const double *__restrict__ x, double *__restrict__ y, \
        const double *__restrict__ b, const double *__restrict__ dinv, double scale, const double *__restrict__ xrow,             \
        const unsigned char *__restrict__ row_pat, const unsigned *__restrict__ tile_pat, const int *__restrict__ tile_pinfo,     \
        const unsigned char *__restrict__ dcode, const double *__restrict__ dtab
#define SA_STAGED2_ARGS                                                                                                           \
    lds, left, nrows, row0, nblocks, per_xcd, stage_cap, ncols, wq, codesR, tab, vtab, tile_desc, tile_seg, x, y, b, dinv, scale, \
        xrow, row_pat, tile_pat, tile_pinfo, dcode, dtab
template <int MODE>
__global__ __launch_bounds__(256) void sell_staged2_kernel(SA_STAGED2_PARAMS) {
    extern __shared__ __align__(16) double lds[];
    sell_staged2<MODE, true>(SA_STAGED2_ARGS);
}
template <int MODE>
__global__ __launch_bounds__(256) void sell_staged2_codes_kernel(SA_STAGED2_PARAMS) {
    extern __shared__ __align__(16) double lds[];
    sell_staged2<MODE, false>(SA_STAGED2_ARGS);
}
#undef SA_STAGED2_PARAMS
#undef SA_STAGED2_ARGS

// The tiles the staged kernel leaves out, from the list the staging plan made (ids of the whole operator; those
// outside the row range are skipped), one workgroup per tile through sell_slice.
template <int MODE>
__global__ __launch_bounds__(256) void sell_tiles_kernel(int ntl, const int *__restrict__ tiles, int nrows, int row0,
                                                         const roff_t *__restrict__ sptr, const int *__restrict__ col,
                                                         const double *__restrict__ val, const int *__restrict__ ntab,
                                                         const int *__restrict__ tab, const unsigned *__restrict__ codes,
                                                         const double *__restrict__ x, double *__restrict__ y,
                                                         const double *__restrict__ b, const double *__restrict__ dinv,
                                                         double scale, const double *__restrict__ xrow,
                                                         const double *__restrict__ vtab) {
    __shared__ PairEntry ltab[4][64];
    const long lrow0 = (long)tiles[blockIdx.x] * 256 - row0;      // the tile's first row, local to the range
    if (lrow0 < 0 || lrow0 >= nrows) return;
    const long row = lrow0 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane((int)(row >> 6));
    sell_slice<MODE>(ltab[threadIdx.x >> 6], nrows, row0, row, slice, 1, sptr, col, val, ntab, tab, codes, x, y, b, dinv,
                     scale, xrow, vtab);
}

// x-staging plan of the pair-coded tiles (see Sell::Stage::tile_seg): one wavefront per tile of 4 slices.  The
// distinct column offsets of the four slice tables are sorted (bitonic, 256 keys in LDS).  An offset o needs
// x[R0 + o .. R0 + o + 255] for the tile's 256 rows R0..: offsets no more than 256 + STAGE_GAP apart have ranges that
// touch or overlap and become one segment [lo, hi] covering x[R0 + lo .. R0 + hi + 255] (a 27-point stencil: one
// segment per z-plane, three of 772 doubles), its start moved down to an even index (16-byte aligned loads) and its
// length made even.  Tiles with
// a slice that is not pair-coded / wider than 32, with more than SELL_SEG_MAX segments or more than SELL_STAGE_CAP
// doubles are not staged (nseg = 0) and take the gather path.
constexpr int STAGE_GAP = 32;
__global__ __launch_bounds__(64) void sell_stage_kernel(int ntiles, int nslices, int nrows, const roff_t *__restrict__ sptr,
                                                        const int *__restrict__ ntab, const int *__restrict__ tab,
                                                        int *__restrict__ tile_nseg, int2 *__restrict__ tile_seg,
                                                        int *__restrict__ max_total, int *__restrict__ unstaged) {
    __shared__ int v[256];
    __shared__ int lo[SELL_SEG_MAX], hi[SELL_SEG_MAX];
    const int t = blockIdx.x, lane = threadIdx.x;
    bool ok = (long)(4 * t + 4) * 64 <= nrows;      // four whole slices
    for (int q = 0; q < 4 && ok; ++q) {
        const int sl = 4 * t + q;
        const int nt = ntab[sl];
        const int w = (int)((sptr[sl + 1] - sptr[sl]) >> 6);
        ok = nt >= 256 && w <= 32;
        // (a tile that shares one table: listed once, by its first slice)
        if (ok) v[64 * q + lane] = (lane < pair_count(nt) && (nt < 512 || q == 0)) ? tab[pair_table_at(sl, nt) + lane] : INT_MAX;
    }
    auto give_up = [&]() {      // max_total[2]: number of tiles left to the gather kernel, listed in `unstaged`
        if (lane == 0) {
            tile_nseg[t] = 0;
            unstaged[atomicAdd(max_total + 2, 1)] = t;
        }
    };
    if (!ok) {
        give_up();
        return;
    }
    __syncthreads();
    for (int k = 2; k <= 256; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < 256; i += 64) {
                const int p = i ^ j;
                if (p > i) {
                    const int a = v[i], b = v[p];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { v[i] = b; v[p] = a; }
                }
            }
            __syncthreads();
        }
    // segment starts among the sorted keys (duplicates and the INT_MAX padding start nothing)
    int nseg = 0, nend = 0;
    for (int c = 0; c < 4; ++c) {
        const int i = 64 * c + lane;
        const int a = v[i];
        const int prev = i ? v[i - 1] : INT_MIN;
        const bool valid = a != INT_MAX;
        const bool start = valid && (i == 0 || (long)a - (long)prev > 256 + STAGE_GAP);
        const int next = i < 255 ? v[i + 1] : INT_MAX;
        const bool end = valid && (next == INT_MAX || (long)next - (long)a > 256 + STAGE_GAP);
        const unsigned long long sm = __ballot(start), em = __ballot(end);
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (start) { const int sidx = nseg + __popcll(sm & below); if (sidx < SELL_SEG_MAX) lo[sidx] = a; }
        if (end) { const int eidx = nend + __popcll(em & below); if (eidx < SELL_SEG_MAX) hi[eidx] = a; }
        nseg += __popcll(sm);
        nend += __popcll(em);
    }
    __syncthreads();
    if (nseg > SELL_SEG_MAX) {
        give_up();
        return;
    }
    const long R0 = (long)t * 256;
    int mylo = 0, mylen = 0;
    if (lane < nseg) {
        mylo = lo[lane];
        if ((R0 + mylo) & 1) mylo -= 1;
        mylen = 256 + (hi[lane] - mylo);
        mylen += mylen & 1;
    }
    int total = mylen;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    if (total > SELL_STAGE_CAP) {
        give_up();
        return;
    }
    if (lane < SELL_SEG_MAX) tile_seg[(size_t)t * SELL_SEG_MAX + lane] = make_int2(mylo, mylen);
    if (lane == 0) {
        tile_nseg[t] = nseg;
        atomicMax(max_total, total);
        atomicAdd(max_total + 1, 1);
        bool shared_all = true;
        for (int q = 0; q < 4; ++q) shared_all = shared_all && ntab[4 * t + q] >= 512;
        if (!shared_all) atomicAdd(max_total + 3, 1);      // staged tiles whose slices keep tables of their own
    }
}


// ---- operator-level pair dictionary (Sell::Dict) -------------------------------------------------------------------
struct alignas(16) GPair {
    int off, pad;      // off: (col - row) * 8, a byte offset into x (operators below 2^28 columns)
    double val;
};
// x[row + offset]: scalar base + 32-bit byte offset (one add per gather)
__device__ __forceinline__ double gp_x(const double *__restrict__ x, unsigned row8, int off8) {
    return *(const double *)((const char *)x + (row8 + (unsigned)off8));
}
constexpr int GD_CAP = 1 << 18;      // hash slots
constexpr int GP_MAX = 6144;         // pairs accepted: the table has to fit LDS (96 KB; see sell_gpair_kernel)
// One wavefront per slice, one lane per row: every stored entry (padding included) looks its (col - row, value) pair
// up in a hash table shared by the whole operator, inserting it on first sight (the pair's code = order of insertion:
// run-dependent, immaterial -- a code only names its pair).
// A slot is a 16-byte record {value bits; offset, code + 1} that is written once (its second word last, with release
// order, after the slot was claimed through state[]: 0 -> 1 by atomicCAS) and never changes.  The common case -- the
// pair is there -- is ONE ordinary cached 16-byte load: a record whose second word is non-zero is complete (both words
// sit in one cache line and the first was written first) and final, whichever cache it comes from.  Only a record that
// looks empty is looked at again with device-coherent accesses: those bypass the XCD's L2 (the eight L2s are not
// coherent with one another), and with every look-up made of them the build of the 64^3 Q2 operator's dictionary
// (1.6e9 entries) took 205 ms; a workgroup-level LDS cache in front of them did not change that, nor did one look-up
// per distinct pair of a wavefront's 64 entries (570 ms: look-ups one after the other instead of side by side).
// counter[0] = pairs so far; beyond GP_MAX the build is abandoned (counter[1] = 1) and every wavefront leaves.
__device__ __forceinline__ int gdict_lookup(int off, unsigned long long vb, int *__restrict__ state,
                                            unsigned long long *rec, int *__restrict__ counter, GPair *__restrict__ gtab) {
    const unsigned long long hsh = (vb ^ (vb >> 29)) * 0x9E3779B97F4A7C15ull + (unsigned long long)(unsigned)off * 0xC2B2AE3D27D4EB4Full;
    unsigned slot = (unsigned)(hsh >> 40) & (GD_CAP - 1);
    for (int probes = 0; probes < GD_CAP; ++probes) {
        // (an operator without repeated pairs -- a general coarse operator -- can have every resident lane claim a slot
        // before the first of them sees the abandon flag: more claims than GD_CAP slots, and a look-up in a full table
        // would walk all of it.  The flag is looked at every 32 probes, and 1 024 probes without a hit abandon the build.)
        if ((probes & 31) == 31) {
            if (__hip_atomic_load(&counter[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;
            if (probes >= 1023) {
                __hip_atomic_store(&counter[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return 0;
            }
        }
        typedef unsigned long long gd_u2 __attribute__((ext_vector_type(2)));
        const gd_u2 r = *(const gd_u2 *)(rec + 2 * (size_t)slot);      // (ordinary, cached)
        unsigned long long w1 = r[1], w0 = r[0];
        if (w1 == 0) {      // empty, or not visible here yet
            int st = __hip_atomic_load(&state[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 0) {
                if (__hip_atomic_load(&counter[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;      // abandoned
                if (__hip_atomic_load(&counter[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= GP_MAX) {   // no room for a new pair: abandon before claiming
                    __hip_atomic_store(&counter[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return 0;
                }
                if (atomicCAS(&state[slot], 0, 1) == 0) {
                    const int id = atomicAdd(&counter[0], 1);
                    int code = id;
                    if (id >= GP_MAX) {
                        __hip_atomic_store(&counter[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        code = 0;
                    } else {
                        gtab[id] = GPair{off * 8, 0, __longlong_as_double((long long)vb)};      // (byte offset)
                    }
                    __hip_atomic_store(&rec[2 * (size_t)slot], vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&rec[2 * (size_t)slot + 1], ((unsigned long long)(unsigned)(code + 1) << 32) | (unsigned)off,
                                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    return code;
                }
            }
            // claimed by somebody else: the record again, with device-coherent loads; not there yet -> the same slot
            // again through the whole loop body (the claimer may be a lane of this wavefront: it publishes inside the
            // body, so waiting anywhere else would wait for a lane that is not running)
            w1 = __hip_atomic_load(&rec[2 * (size_t)slot + 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (w1 == 0) {
                if (__hip_atomic_load(&counter[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;      // abandoned
                --probes;
                continue;
            }
            w0 = __hip_atomic_load(&rec[2 * (size_t)slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if ((int)(unsigned)(w1 & 0xffffffffull) == off && w0 == vb) return (int)(w1 >> 32) - 1;
        slot = (slot + 1) & (GD_CAP - 1);
    }
    return 0;
}
__global__ __launch_bounds__(256) void sell_gdict_kernel(int nslices, const roff_t *__restrict__ sptr,
                                                         const int *__restrict__ scol, const double *__restrict__ sval,
                                                         int *__restrict__ state, unsigned long long *rec,
                                                         int *__restrict__ counter, GPair *__restrict__ gtab,
                                                         unsigned long long *__restrict__ gcode) {
    const int slice = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slice >= nslices) return;
    const roff_t beg = sptr[slice];
    const int w = (int)((sptr[slice + 1] - beg) >> 6);
    const int row = slice * 64 + lane;
    unsigned long long *wp = code_words(gcode, beg, slice, lane);
    unsigned long long word = 0;      // four codes of the row per 8-byte word
    for (int k = 0; k < w; ++k) {
        const int off = scol[beg + 64 * k + lane] - row;
        const unsigned long long vb = (unsigned long long)__double_as_longlong(sval[beg + 64 * k + lane]);
        if ((k & 15) == 0 && __hip_atomic_load(&counter[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;      // abandoned (wave-uniform)
        const int code = gdict_lookup(off, vb, state, rec, counter, gtab);
        word |= (unsigned long long)(unsigned)(code & 0xffff) << (16 * (k & 3));
        if ((k & 3) == 3 || k + 1 == w) {
            wp[64 * (size_t)(k >> 2)] = word;      // (the rest of the last word stays 0)
            word = 0;
        }
    }
}

// 3 x 3 node blocks?  One wavefront per 63 rows (21 nodes: sell_gpair3_kernel's waves), one lane per row.  A row is
// REGULAR when its node's rows 3i, 3i+1, 3i+2 hold the same columns, in runs 3j, 3j+1, 3j+2; the others (rows eliminated
// for essential conditions, a last partial node) are listed in irr_rows (count[0] of them, in no particular order).
__global__ __launch_bounds__(256) void sell_bs3_kernel(int nrows, int nwaves, const roff_t *__restrict__ rowptr,
                                                       const int *__restrict__ col, int *__restrict__ irr_rows, int cap,
                                                       int *__restrict__ count) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= nwaves) return;
    const int row = wave * 63 + lane;
    const int a = lane % 3, first = row - a;
    bool ok = lane < 63 && first + 2 < nrows;
    if (ok) {
        const roff_t rb = rowptr[row], fb = rowptr[first];
        const int len = (int)(rowptr[row + 1] - rb);
        ok = len % 3 == 0 && len == (int)(rowptr[first + 1] - fb);
        for (int k = 0; ok && k < len; ++k) {
            const int c = col[rb + k];
            ok = c % 3 == k % 3 && c == col[fb + k] && (k % 3 == 0 || c == col[rb + k - 1] + 1);
        }
    }
    const unsigned long long good = __ballot(ok);      // a node is regular only if its three rows are
    const bool node_ok = lane < 63 && ((good >> (lane - a)) & 7ull) == 7ull;
    if (lane < 63 && row < nrows && !node_ok) {
        const int at = atomicAdd(count, 1);
        if (at < cap) irr_rows[at] = row;
    }
}

// SpMV family on a dictionary-coded operator.  The table lives in LDS (at most GP_MAX pairs = 96 KB: one workgroup of
// 16 wavefronts per CU, persistent -- it copies the table once and then walks the slices of its XCD's contiguous eighth,
// interleaved with the other 31 workgroups of that XCD).  One wavefront per slice, one lane per row; per four entries one
// 8-byte code word, four LDS table reads and four gathers of x, eight entries in flight.  With the table in global
// memory the table look-ups were vector-memory gathers like those of x (scattered 16-byte entries: ~50 cycles each on
// the CU's address path) and the kernel was SLOWER than the plain slices it replaces although it moves a sixth of their
// bytes (3.3 against 3.2 ms per application of the 64^3 Q2 operator); from LDS they cost an LDS read.
// The order of additions is the family's (see sell_slice), here eight entries per trip: bit-identical results.
template <int MODE>
__global__ __launch_bounds__(1024) void sell_gpair_kernel(int nrows, int row0, int nslices, int per_xcd, int wg_per_xcd, int ng,
                                                          const roff_t *__restrict__ sptr,
                                                          const unsigned long long *__restrict__ gcode,
                                                          const GPair *__restrict__ gtab,
                                                          const double *__restrict__ x, double *__restrict__ y,
                                                          const double *__restrict__ b,
                                                          const double *__restrict__ dinv, double scale,
                                                          const double *__restrict__ xrow) {
    extern __shared__ __align__(16) GPair ltab[];
    for (int i = threadIdx.x; i < ng; i += 1024) ltab[i] = gtab[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xcd = (int)(blockIdx.x & 7u), p = (int)(blockIdx.x >> 3);
    const int c0 = xcd * per_xcd, c1 = min(c0 + per_xcd, nslices);
    const int g0 = row0 >> 6;
    for (int slice = c0 + p * 16 + wv; slice < c1; slice += wg_per_xcd * 16) {
        const roff_t beg = sptr[slice], end = sptr[slice + 1];
        const int gslice = g0 + slice;
        const int w = (int)((end - beg) >> 6);
        const long row = (long)slice * 64 + lane;
        const bool live = row < nrows;
        const int grow = row0 + (int)row;
        const RowTerms t = row_terms<MODE>(SpmvVecs{x, y, b, dinv, scale, xrow}, row, live);
        const unsigned long long *wp = code_words(gcode, beg, gslice, lane);
        const unsigned grow8 = (unsigned)grow << 3;
        double s0 = 0.0, s1 = 0.0;
        int k = 0;
        for (; k + 8 <= w; k += 8) {
            const unsigned long long ca = __builtin_nontemporal_load(wp + 16 * k), cb = __builtin_nontemporal_load(wp + 16 * (k + 4));
            GPair e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = ltab[(unsigned)(((j < 4 ? ca : cb) >> (16 * (j & 3))) & 0xffffull)];
            double xs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xs[j] = gp_x(x, grow8, e[j].off);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j & 1) s1 = fma(e[j].val, xs[j], s1);
                else s0 = fma(e[j].val, xs[j], s0);
            }
        }
        for (; k + 4 <= w; k += 4) {
            const unsigned long long ca = __builtin_nontemporal_load(wp + 16 * k);
            GPair e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ltab[(unsigned)((ca >> (16 * j)) & 0xffffull)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double xv = gp_x(x, grow8, e[j].off);
                if (j & 1) s1 = fma(e[j].val, xv, s1);
                else s0 = fma(e[j].val, xv, s0);
            }
        }
        if (k < w) {
            unsigned long long ca = __builtin_nontemporal_load(wp + 16 * k);
            for (; k < w; ++k, ca >>= 16) {
                const GPair e = ltab[(unsigned)(ca & 0xffffull)];
                s0 = fma(e.val, gp_x(x, grow8, e.off), s0);
            }
        }
        if (live) spmv_epilogue<MODE>(s0 + s1, t, scale, y, row);
    }
}

// The same for operators with 3 x 3 NODE BLOCKS (vector problems numbered node by node, three components each: rows
// 3i..3i+2 store the same columns, in runs 3j..3j+2 -- sell_bs3_kernel).  The three lanes of a node would gather the
// same three entries of x one after the other; here each lane gathers ONE of them (entry 3s + a of its row, a = its
// component: x[3j + a]) and takes the other two from its neighbours with wave shifts (v_mov_b32_dpp wave_shr / wave_shl):
// a third of the gathers, which are what bounds the kernel above (~39 cycles of the CU's address path per instruction,
// whatever the number of active lanes: extra loads for a few lanes of a wave cost as much as for all of them).
// So that no node is cut, a wavefront takes 63 ROWS (21 nodes; lane 63 idles): rows 63 j .. 63 j + 62 of the operator,
// which lie in one or two storage slices -- slice, width and code address are per lane.  Irregular rows (eliminated for
// essential conditions: their lanes compute nothing useful here) are redone by sell_gpair3_fix_kernel afterwards.
// Same products in the same order per row: entries below w & ~3 (w = the row's slice width) alternate between the two
// accumulators, the rest goes to the first; entries past the row's slice (the wave's other slice is wider) add nothing.
__device__ __forceinline__ double wave_from_prev(double v) {      // lane l <- lane l - 1
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ double wave_from_next(double v) {      // lane l <- lane l + 1
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true));
}
// x of the three entries of one node block from the lane's own gather (its component a) and its neighbours'
__device__ __forceinline__ void bs3_share(double own, int a, double &x0, double &x1, double &x2) {
    const double m1 = wave_from_prev(own), m2 = wave_from_prev(m1), p1 = wave_from_next(own), p2 = wave_from_next(p1);
    x0 = a == 0 ? own : (a == 1 ? m1 : m2);
    x1 = a == 0 ? p1 : (a == 1 ? own : m1);
    x2 = a == 0 ? p2 : (a == 1 ? p1 : own);
}
// code of entry 3 t + a of a group of 12 (code words cw[0..2], four codes each; a = the lane's component, t constant)
__device__ __forceinline__ unsigned bs3_own_code(const unsigned long long (&cw)[3], int t, int a) {
    unsigned c[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = (unsigned)((cw[(3 * t + q) >> 2] >> (16 * ((3 * t + q) & 3))) & 0xffffull);
    return a == 0 ? c[0] : (a == 1 ? c[1] : c[2]);
}
// Lean enough for TWO workgroups per CU (32 wavefronts): the table split into values (8 B) and byte offsets (4 B) -- 12 B
// per pair, 66 KB for 5 540 pairs -- and 63 VGPRs.  A version with one 16-byte table (one workgroup per CU) and a software
// pipeline over two register sets (code words of group g + 2 and the look-ups + gathers of group g + 1 issued before the
// products of group g; 95 VGPRs) ran at 1.22 ms per application of the 64^3 Q2 operator against 1.47 without the pipeline;
// its counters showed 71 % of the wave-cycles waiting at four wavefronts per SIMD, and this one, with eight and no
// pipeline, takes 1.05 ms (git history: sell_gpair3_kernel before "two workgroups per CU").
template <int MODE>
__global__ __launch_bounds__(1024, 2) void sell_gpair3_kernel(int nrows_all, int row_lo, int row_hi, int wave0, int nwaves, int per_xcd,
                                                               int wg_per_xcd, int ng, const roff_t *__restrict__ sptr,
                                                               const unsigned long long *__restrict__ gcode,
                                                               const GPair *__restrict__ gtab, const double *__restrict__ x,
                                                               double *__restrict__ y, const double *__restrict__ b,
                                                               const double *__restrict__ dinv, double scale) {
    extern __shared__ __align__(16) double lval[];      // [ng] values, then [ng] byte offsets
    int *loff = (int *)(lval + ng);
    for (int i = threadIdx.x; i < ng; i += 1024) { const GPair e = gtab[i]; lval[i] = e.val; loff[i] = e.off; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xcd = (int)(blockIdx.x & 7u), p = (int)(blockIdx.x >> 3);
    const int c0 = xcd * per_xcd, c1 = min(c0 + per_xcd, nwaves);
    const int a = lane % 3;
    for (int wi = c0 + p * 16 + wv; wi < c1; wi += wg_per_xcd * 16) {
        const int first = (wave0 + wi) * 63;
        const int row = min(first + min(lane, 62), nrows_all - 1);
        const bool live = lane < 63 && first + lane >= row_lo && first + lane < row_hi;
        const int slice = row >> 6;
        const roff_t beg = sptr[slice];
        const int w = (int)((sptr[slice + 1] - beg) >> 6), w4 = w & ~3;
        const unsigned long long *wp = code_words(gcode, beg, slice, row & 63);
        const unsigned short *cp = (const unsigned short *)wp;
        const unsigned row8 = (unsigned)row << 3;
        const int wa = __builtin_amdgcn_readfirstlane(w), wb = __builtin_amdgcn_readlane(w, 62);
        const int wmin = min(wa, wb), wmax = max(wa, wb);
        double s0 = 0.0, s1 = 0.0;
        int k = 0;
        for (; k + 12 <= wmin; k += 12) {
            unsigned long long cw[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) cw[q] = __builtin_nontemporal_load(wp + 16 * (k + 4 * q));
            double own[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) own[t] = gp_x(x, row8, loff[bs3_own_code(cw, t, a)]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                double xs[3];
                bs3_share(own[t], a, xs[0], xs[1], xs[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int j = 3 * t + c;
                    const double v = lval[(unsigned)((cw[j >> 2] >> (16 * (j & 3))) & 0xffffull)];
                    if (j & 1) s1 = fma(v, xs[c], s1);
                    else s0 = fma(v, xs[c], s0);
                }
            }
        }
        for (; k < wmax; k += 3) {
            int o[3];
            double v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int kk = k + c;
                const unsigned code = kk < w ? cp[64 * (size_t)(kk - (kk & 3)) + (kk & 3)] : 0xffffu;
                o[c] = code != 0xffffu ? loff[code] : 0;
                v[c] = code != 0xffffu ? lval[code] : 0.0;
            }
            asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]));
            const double own = gp_x(x, row8, a == 0 ? o[0] : (a == 1 ? o[1] : o[2]));
            double xs[3];
            bs3_share(own, a, xs[0], xs[1], xs[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (k + c < w4 && ((k + c) & 1)) s1 = fma(v[c], xs[c], s1);
                else s0 = fma(v[c], xs[c], s0);
            }
        }
        // (whole-operator arrays: the smoother's x-row is x itself.  The row's terms behind the products: 63 VGPRs)
        if (live) spmv_epilogue<MODE>(s0 + s1, row_terms<MODE>(SpmvVecs{x, y, b, dinv, scale, x}, row), scale, y, row);
    }
}
// The irregular rows of a node-block operator, one lane per row (a few rows per thousand: strided reads do not matter).
template <int MODE>
__global__ __launch_bounds__(256) void sell_gpair3_fix_kernel(int nirr, const int *__restrict__ irr_rows, int row_lo, int row_hi,
                                                              const roff_t *__restrict__ sptr,
                                                              const unsigned long long *__restrict__ gcode,
                                                              const GPair *__restrict__ gtab,
                                                              const double *__restrict__ x, double *__restrict__ y,
                                                              const double *__restrict__ b,
                                                              const double *__restrict__ dinv, double scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nirr) return;
    const int row = irr_rows[i];
    if (row < row_lo || row >= row_hi) return;
    const int slice = row >> 6;
    const roff_t beg = sptr[slice];
    const int w = (int)((sptr[slice + 1] - beg) >> 6), w4 = w & ~3;
    const unsigned short *cp = (const unsigned short *)code_words(gcode, beg, slice, row & 63);
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < w; ++k) {
        const GPair e = gtab[cp[64 * (size_t)(k - (k & 3)) + (k & 3)]];
        if (k < w4 && (k & 1)) s1 = fma(e.val, gp_x(x, (unsigned)row << 3, e.off), s1);
        else s0 = fma(e.val, gp_x(x, (unsigned)row << 3, e.off), s0);
    }
    spmv_epilogue<MODE>(s0 + s1, row_terms<MODE>(SpmvVecs{x, y, b, dinv, scale, x}, row), scale, y, row);
}

// Slice census of a SELL copy: cls[0..2] = pair-coded / offset-coded / plain slices, cls[3..5] = their stored entries
// (64 x width), cls[6] = code words of the coded slices, cls[7] = widest slice
__global__ __launch_bounds__(256) void sell_census_kernel(int nslices, const roff_t *__restrict__ sptr,
                                                          const int *__restrict__ ntab,
                                                          unsigned long long *__restrict__ cls) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const bool in = s < nslices;
    const int w = in ? (int)((sptr[s + 1] - sptr[s]) >> 6) : 0;
    const int nt = in ? ntab[s] : -1;
    const int c = nt >= 256 ? 0 : (nt >= 0 ? 1 : 2);
    // (one atomic per wavefront and counter: 265 000 threads adding to the same eight words took 6.5 ms)
    unsigned long long part[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        part[k] = in && c == k ? 1ull : 0ull;
        part[3 + k] = in && c == k ? (unsigned long long)w * 64ull : 0ull;
    }
    part[6] = in && c < 2 ? (unsigned long long)((w + 3) / 4) * 64ull : 0ull;
    part[7] = (unsigned long long)w;
    // (a slice that reads its tile's table has none of its own: counted as a negative share of the table bytes below)
    part[8] = in && nt >= 512 && (s & 3) != 0 ? 1ull : 0ull;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(part[k], o, 64);
            part[k] = k == 7 ? (other > part[k] ? other : part[k]) : part[k] + other;
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (part[k]) atomicAdd(cls + k, part[k]);
        atomicMax(cls + 7, part[7]);
        if (part[8]) atomicAdd(cls + 8, part[8]);
    }
}

__global__ __launch_bounds__(256) void sell_width_kernel(int nrows, const roff_t *__restrict__ rowptr,
                                                         int *__restrict__ width64) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    int len = (row < nrows) ? (int)(rowptr[row + 1] - rowptr[row]) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o, 64));
    const long slice = row >> 6;
    if ((threadIdx.x & 63) == 0 && slice * 64 < nrows) width64[slice] = len * 64;
}

// CSR -> SELL-64, one wavefront per slice.  The slice's CSR entries are one contiguous range: it is read
// with coalesced loads into LDS and every lane then picks its row's entries from there (the column-major
// SELL stores are coalesced by construction).  A lane walking its own CSR row instead touches 64 different
// cache lines per load instruction (measured: 110 GB fetched to convert 5.5 GB).  Slices with more than
// SF_CAP entries (dense coarse-level rows) take that slow walk.
constexpr int SF_CAP = 2048;
// the contiguous CSR range [r0, r0 + len) of a slice into LDS, one wavefront: eight entries per lane and trip are requested
// before the first is stored (one entry per trip waited for a global round trip 27 times per slice of a 27-point operator)
__device__ __forceinline__ void stage_slice(const int *__restrict__ col, const double *__restrict__ val, roff_t r0, int len, int lane,
                                            int *lc, double *lv) {
    constexpr int U = 8;
    for (int t0 = lane; t0 < len; t0 += 64 * U) {
        int c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(t0 + 64 * u, len - 1);
            c[u] = col[r0 + t];
            v[u] = val[r0 + t];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t0 + 64 * u < len) {
                lc[t0 + 64 * u] = c[u];
                lv[t0 + 64 * u] = v[u];
            }
    }
}
__global__ __launch_bounds__(64) void sell_fill_kernel(int nrows, const roff_t *__restrict__ rowptr,
                                                       const int *__restrict__ col,
                                                       const double *__restrict__ val,
                                                       const roff_t *__restrict__ sptr,
                                                       int *__restrict__ scol, double *__restrict__ sval) {
    __shared__ double lv[SF_CAP];
    __shared__ int lc[SF_CAP];
    const int slice = blockIdx.x, lane = threadIdx.x;
    const long row = (long)slice * 64 + lane;
    const roff_t beg = sptr[slice];
    const int w = (int)((sptr[slice + 1] - beg) >> 6);
    roff_t rb = 0, re = 0;
    if (row < nrows) { rb = rowptr[row]; re = rowptr[row + 1]; }
    const int pad = (row < nrows) ? (int)row : nrows - 1;
    const roff_t r0 = rowptr[(long)slice * 64], r1 = rowptr[min((long)slice * 64 + 64, (long)nrows)];
    if (r1 - r0 <= SF_CAP) {
        stage_slice(col, val, r0, (int)(r1 - r0), lane, lc, lv);
        __syncthreads();
        for (int k = 0; k < w; ++k) {
            const bool in = rb + k < re;
            scol[beg + 64 * k + lane] = in ? lc[rb - r0 + k] : pad;
            sval[beg + 64 * k + lane] = in ? lv[rb - r0 + k] : 0.0;
        }
        return;
    }
    for (int k = 0; k < w; ++k) {
        const bool in = rb + k < re;
        scol[beg + 64 * k + lane] = in ? col[rb + k] : pad;
        sval[beg + 64 * k + lane] = in ? val[rb + k] : 0.0;
    }
}

// Tables and byte codes of the coded slices (see sell_spmv_kernel): one wavefront per slice.  First
// the distinct (offset, value) PAIRS are collected in first-appearance order, one table entry per lane
// (ntab = 256 + count: neither columns nor values are streamed for such a slice); a slice with more than
// 64 pairs falls back to the distinct offsets col - row alone (ntab = count, values streamed), and one with
// more than 64 offsets keeps its 4-byte columns (ntab = -1).  The codes of four consecutive entries of a
// row share one 32-bit word at codes[sptr/4 + 64 slice + 64 (k / 4) + lane].
__global__ __launch_bounds__(256) void sell_code_kernel(int nslices, const roff_t *__restrict__ sptr,
                                                        const int *__restrict__ scol, const double *__restrict__ sval,
                                                        int *__restrict__ ntab, int *__restrict__ tab,
                                                        double *__restrict__ vtab, unsigned *__restrict__ codes,
                                                        int with_values, int share_tables) {
    // (tile = the four slices of this block; merge phase below)
    __shared__ int m_off[4][64];
    __shared__ long long m_val[4][64];
    __shared__ int m_np[4];                 // pairs of the slice's own table, -1: the slice is not (short) pair-coded
    __shared__ unsigned char m_map[4][64];  // own code -> code in the tile's table
    __shared__ int m_ok, m_nt;
    const int wv = threadIdx.x >> 6;
    const int slice = blockIdx.x * 4 + wv, lane = threadIdx.x & 63;
    const bool have = slice < nslices;
    const roff_t beg = have ? sptr[slice] : 0;
    const int w = have ? (int)((sptr[slice + 1] - beg) >> 6) : 0;
    const int row = slice * 64 + lane;
    unsigned *wp = code_words(codes, beg, slice, lane);
    int my_np = -1;
    for (int pass = with_values ? 0 : 1; pass < 2 && have; ++pass) {
        const bool pairs = pass == 0;
        int mytab = 0, nt = 0;
        long long myval = 0;
        unsigned cw = 0;
        bool ok = true;
        for (int k = 0; k < w && ok; ++k) {
            const int delta = scol[beg + 64 * k + lane] - row;
            const long long vb = pairs ? __double_as_longlong(sval[beg + 64 * k + lane]) : 0;
            // One trip per DISTINCT pair among the 64 entries of this column of the slice (one to three on a stencil operator):
            // the first lane without a code broadcasts its pair, the table -- entry t in lane t -- answers with one ballot, and a
            // pair that is not in it is appended.  (Until round 4 every lane first walked the whole table through two shuffles
            // per entry -- 27 x 27 x 3 cross-lane reads per slice of a 27-point operator, the kernel's bound -- before this loop
            // added what was missing.  Same tables, same codes: the pairs are appended in the order of the lanes that bring them.)
            int code = -1;
            unsigned long long pending = ~0ull;
            while (pending) {
                const int leader = __ffsll((long long)pending) - 1;
                // (both shuffles outside any condition: a cross-lane read under a divergent branch returns nothing from
                // the lanes that did not take it)
                const int d = __shfl(delta, leader);
                const long long dv = __shfl(vb, leader);
                const unsigned long long hit = __ballot(lane < nt && mytab == d && myval == dv);
                int c;
                if (hit) c = __ffsll((long long)hit) - 1;
                else {
                    if (nt == 64) { ok = false; break; }
                    if (lane == nt) { mytab = d; myval = dv; }
                    c = nt++;
                }
                if (code < 0 && delta == d && vb == dv) code = c;
                pending = __ballot(code < 0);
            }
            cw |= (unsigned)(code & 255) << (8 * (k & 3));
            if ((k & 3) == 3 || k == w - 1) {
                wp[16 * (k & ~3)] = cw;
                cw = 0;
            }
        }
        if (ok || !pairs) {
            tab[(size_t)slice * 64 + lane] = mytab;
            if (pairs) vtab[(size_t)slice * 64 + lane] = __longlong_as_double(myval);
            if (lane == 0) ntab[slice] = ok ? (pairs ? 256 + nt : nt) : -1;
            if (ok && pairs && w <= 32) {
                my_np = nt;
                m_off[wv][lane] = mytab;
                m_val[wv][lane] = myval;
            }
            break;
        }
    }
    // ---- one table for the tile (share_tables): the four slice tables of a stencil operator hold the same pairs in
    // different orders (12 bytes per row of table traffic, a third of the matrix stream); merged into one of at most
    // 64 pairs the tile's four wavefronts read the same 768 bytes.  ntab = 512 + pairs marks "table at the tile's
    // first slice".  Lossless: every code still names the same (offset, value) pair.
    if (!share_tables) return;
    if (lane == 0) m_np[wv] = my_np;
    if (threadIdx.x == 0) m_ok = 1;
    __syncthreads();
    if (m_np[0] < 0 || m_np[1] < 0 || m_np[2] < 0 || m_np[3] < 0) return;      // (uniform: a partial or mixed tile keeps its own tables)
    if (wv == 0) {
        int t_off = m_off[0][lane];
        long long t_val = m_val[0][lane];
        int nT = m_np[0];
        m_map[0][lane] = (unsigned char)lane;
        bool ok = true;
        for (int q = 1; q < 4 && ok; ++q)
            for (int e = 0; e < m_np[q]; ++e) {
                const int d = m_off[q][e];
                const long long dv = m_val[q][e];
                const unsigned long long hit = __ballot(lane < nT && t_off == d && t_val == dv);
                int code;
                if (hit) code = __ffsll((long long)hit) - 1;
                else {
                    if (nT == 64) { ok = false; break; }
                    if (lane == nT) { t_off = d; t_val = dv; }
                    code = nT++;
                }
                if (lane == 0) m_map[q][e] = (unsigned char)code;
            }
        if (lane == 0) { m_ok = ok ? 1 : 0; m_nt = nT; }
        if (ok) {
            m_off[0][lane] = t_off;
            m_val[0][lane] = t_val;
        }
    }
    __syncthreads();
    if (!m_ok) return;
    // every wavefront rewrites ITS OWN code words (written above by the same lanes) through the map
    for (int q4 = 0; 4 * q4 < w; ++q4) {
        const unsigned cw = wp[64 * q4];
        unsigned out = 0;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
            if (4 * q4 + e4 < w) out |= (unsigned)m_map[wv][(cw >> (8 * e4)) & 63u] << (8 * e4);
        wp[64 * q4] = out;
    }
    const int first = blockIdx.x * 4;
    if (wv == 0) {
        tab[(size_t)first * 64 + lane] = lane < m_nt ? m_off[0][lane] : 0;
        vtab[(size_t)first * 64 + lane] = lane < m_nt ? __longlong_as_double(m_val[0][lane]) : 0.0;
    }
    if (lane == 0) ntab[slice] = 512 + m_nt;
}

void import_rowptr(DBuf<roff_t> &dst, const void *src, int bits, size_t n, hipStream_t s) {
    SA_REQUIRE(bits == 32 || bits == 64, "row offsets must be 32 or 64 bits wide");
    if (bits == 64) {
        dst = DevIn<roff_t>((const roff_t *)src, n, s).take();
        return;
    }
    const DevIn<int> narrow((const int *)src, n, s);
    dst.alloc(n);
    if (n) dev_convert(s, (long)n, (const int *)narrow.p, dst.p);
    SA_HIP_CHECK(hipStreamSynchronize(s));      // `narrow` may be an upload that is freed on return
}

void export_rowptr32(int *dst_host, const DBuf<roff_t> &src, size_t n, hipStream_t s) {
    if (!n) return;
    const roff_t last = read_one(src.p + (n - 1), s);
    SA_REQUIRE(last < ((roff_t)1 << 31), "operator has more than 2^31 entries: use the 64-bit getter");
    DBuf<int> narrow(n);
    dev_convert(s, (long)n, (const roff_t *)src.p, narrow.p);
    read_back(dst_host, narrow.p, n, s);
}

// ---- build_sell, step by step.  A.sell starts out as Sell(): every step only fills ---------------------------------
// slice widths, their scan, the entries
static void fill_slices(hipStream_t s, DCsr &A) {
    Sell &S = A.sell;
    S.nslices = div_up(A.nrows, 64);
    DBuf<int> w64((size_t)S.nslices);
    const int grid = div_up((long)S.nslices * 64, 256);
    hipLaunchKernelGGL(sell_width_kernel, dim3(grid), dim3(256), 0, s, A.nrows, A.rowptr.p, w64.p);
    S.ptr.alloc((size_t)S.nslices + 1);
    exclusive_scan_off(s, S.nslices, w64.p, S.ptr.p);
    S.size = read_one(S.ptr.p + S.nslices, s);
    S.col.alloc((size_t)S.size + 64);
    S.val.alloc((size_t)S.size + 64);
    hipLaunchKernelGGL(sell_fill_kernel, dim3(S.nslices), dim3(64), 0, s, A.nrows, A.rowptr.p, A.col.p, A.val.p, S.ptr.p, S.col.p, S.val.p);
    SA_HIP_CHECK(hipGetLastError());
}
// byte codes for the slices with few distinct column offsets (saamge_amd_options.sell bit 0 cleared: none;
// bit 1 cleared: offset codes only, values always streamed)
static void code_slices(hipStream_t s, DCsr &A, const Options &opt) {
    Sell &S = A.sell;
    S.ntab.alloc((size_t)S.nslices);
    S.tab.alloc((size_t)S.nslices * 64);
    S.code.alloc((size_t)S.size / 4 + (size_t)S.nslices * 64 + 64);
    S.vtab.alloc((size_t)S.nslices * 64);
    if (!(opt.sell & 1))
        SA_HIP_CHECK(hipMemsetAsync(S.ntab.p, 0xff, sizeof(int) * (size_t)S.nslices, s));
    else
        hipLaunchKernelGGL(sell_code_kernel, dim3(div_up(S.nslices, 4)), dim3(256), 0, s, S.nslices, S.ptr.p,
                           S.col.p, S.val.p, S.ntab.p, S.tab.p, S.vtab.p, S.code.p, (opt.sell & 2) ? 1 : 0, 1);
    SA_HIP_CHECK(hipGetLastError());
}
// what the copy holds, per slice format: the bytes one application has to move (the roofline of the SpMV family
// prices THESE, bench.py).  Returns sell_census_kernel's nine counters.
static std::array<unsigned long long, 9> census(hipStream_t s, DCsr &A) {
    Sell &S = A.sell;
    DBuf<unsigned long long> cls(9);
    cls.zero(s);
    hipLaunchKernelGGL(sell_census_kernel, dim3(div_up(S.nslices, 256)), dim3(256), 0, s, S.nslices, S.ptr.p, S.ntab.p, cls.p);
    SA_HIP_CHECK(hipGetLastError());
    std::array<unsigned long long, 9> h;
    read_back(h.data(), cls.p, h.size(), s);
    for (int c = 0; c < 3; ++c) { S.class_slices[c] = (int64_t)h[c]; S.class_entries[c] = (int64_t)h[3 + c]; }
    // codes 4 B per word, tables 4 (+8) B per lane of a coded slice, values / columns of the formats that stream them,
    // 8 B slice offset + 4 B table size per slice
    S.stream_bytes = 4.0 * (double)h[6] + 12.0 * 64.0 * (double)(h[0] - h[8]) + 4.0 * 64.0 * (double)h[1] +
                     8.0 * (double)h[4] + 12.0 * (double)h[5] + 12.0 * (double)S.nslices;
    return h;
}
// operator-level pair dictionary for operators that are all plain slices (bit 3 cleared: never), and their 3 x 3 node
// blocks (bit 4 cleared: never)
static void try_dictionary(hipStream_t s, DCsr &A, const Options &opt, const std::array<unsigned long long, 9> &h) {
    if (!(opt.sell & 8) || !(opt.sell & 1) || h[0] != 0 || h[1] != 0 || A.nnz < (1 << 22) || A.ncols >= (1 << 28)) return;
    Sell &S = A.sell;
    Sell::Dict D;
    DBuf<int> st((size_t)GD_CAP), ctr(2);
    DBuf<unsigned long long> rec(2 * (size_t)GD_CAP);
    st.zero(s);
    rec.zero(s);
    ctr.zero(s);
    D.gcode.alloc((size_t)S.size / 4 + (size_t)S.nslices * 64 + 64);
    D.gtab.alloc(GP_MAX);
    hipLaunchKernelGGL(sell_gdict_kernel, dim3(div_up(S.nslices, 4)), dim3(256), 0, s, S.nslices, S.ptr.p, S.col.p,
                       S.val.p, st.p, rec.p, ctr.p, (GPair *)D.gtab.p, D.gcode.p);
    SA_HIP_CHECK(hipGetLastError());
    int hc[2];      // (pairs, abandoned: one transfer)
    read_back(hc, ctr.p, 2, s);
    if (!hc[1] && hc[0] <= GP_MAX) {      // (the table has to fit LDS: see sell_gpair_kernel; otherwise D is dropped)
        D.on = true; D.ng = hc[0];
        // codes 2 B per stored entry (rounded up to four per row), the table, 8 B per slice
        const double words = (double)S.size / 4.0 + 64.0 * (double)S.nslices;           // upper bound of the 8-byte code words
        S.stream_bytes = 8.0 * words + 16.0 * (double)hc[0] + 8.0 * (double)S.nslices;
        S.col.release(); S.val.release();      // the dictionary replaces the streamed columns and values (12 B per stored entry)
        if ((opt.sell & 16) && A.ncols == A.nrows && A.nrows >= 63) {
            const int nwaves = div_up(A.nrows, 63), cap = A.nrows / 16 + 1;      // at most a sixteenth of the rows on their own
            D.irr.alloc((size_t)cap);
            SA_HIP_CHECK(hipMemsetAsync(ctr.p, 0, sizeof(int), s));
            hipLaunchKernelGGL(sell_bs3_kernel, dim3(div_up(nwaves, 4)), dim3(256), 0, s, A.nrows, nwaves, A.rowptr.p, A.col.p,
                               D.irr.p, cap, ctr.p);
            SA_HIP_CHECK(hipGetLastError());
            D.nirr = read_one(ctr.p, s);
            D.bs3 = D.nirr <= cap;
            if (!D.bs3) D.irr.release();
        }
        S.dict = std::move(D);
    }
    if ((opt.debug & 2))
        std::fprintf(stderr, "build_sell: operator-level pair dictionary: %d pairs%s%s\n", hc[0], S.dict.on ? "" : " (abandoned)",
                     S.dict.on && S.dict.bs3 ? ", 3 x 3 node blocks" : "");
    if ((opt.debug & 2) && S.dict.on)
        std::fprintf(stderr, "build_sell: %d of %d rows outside regular node blocks\n", S.dict.nirr, A.nrows);
}
// x-staging plan of the pair-coded tiles, where most slices are pair-coded; returns the number of staged tiles
static int plan_staging(hipStream_t s, DCsr &A, const Options &opt, const std::array<unsigned long long, 9> &h) {
    Sell &S = A.sell; Sell::Stage &G = S.stage;
    if (!S.fast_ok || h[0] * 2 < (unsigned long long)S.nslices) return 0;
    const int ntiles = div_up(S.nslices, 4);
    G.tile_nseg.alloc((size_t)ntiles);
    G.tile_seg.alloc((size_t)ntiles * SELL_SEG_MAX);
    G.unstaged.alloc((size_t)ntiles);
    DBuf<int> mx(4);
    mx.zero(s);
    hipLaunchKernelGGL(sell_stage_kernel, dim3(ntiles), dim3(64), 0, s, ntiles, S.nslices, A.nrows, S.ptr.p, S.ntab.p,
                       S.tab.p, G.tile_nseg.p, G.tile_seg.p, mx.p, G.unstaged.p);
    SA_HIP_CHECK(hipGetLastError());
    int hm[4];      // (largest tile, staged tiles, tiles left out, staged tiles with tables of their own)
    read_back(hm, mx.p, 4, s);
    const int staged_tiles = hm[1];
    G.nunstaged = hm[2];
    G.cap = G.nunstaged * 4 > ntiles ? 0 : hm[0];      // (0: too few tiles staged to be worth two launches)
    G.one_table = hm[3] == 0;
    S.stream_bytes += (4.0 + 8.0 * SELL_SEG_MAX) * ntiles;
    if (!G.on() || !G.one_table) return staged_tiles;
    // the regular second copy of the staged tiles' code words + one descriptor word per tile (sell_staged2_kernel)
    G.wq = (int)std::min<unsigned long long>(8, (h[7] + 3) / 4);      // (h[7]: the widest slice; staged ones are <= 32)
    G.tile_desc.alloc((size_t)ntiles);
    // row patterns (bit 6 set: none, every staged tile keeps its code words)
    int nslots = ntiles;
    if (!(opt.sell & 64)) {
        G.row_pat.alloc((size_t)ntiles * 256);
        G.tile_pat.alloc((size_t)ntiles * SELL_PMAX * 8);
        G.tile_pinfo.alloc((size_t)ntiles);
        DBuf<unsigned long long> census(4);
        census.zero(s);
        hipLaunchKernelGGL(sell_row_patterns_kernel, dim3(std::min(ntiles, 2048)), dim3(256), 0, s, ntiles, G.wq, S.ptr.p, G.tile_nseg.p,
                           S.code.p, G.row_pat.p, G.tile_pat.p, G.tile_pinfo.p, census.p);
        SA_HIP_CHECK(hipGetLastError());
        unsigned long long hc[4];
        read_back(hc, census.p, 4, s);
        nslots = (int)hc[0]; G.pat_tiles = (int)hc[1]; G.pat_max = (int)hc[2];
        // every staged tile reads a byte per row, the pattern table and its count; the pattern tiles no code words
        S.stream_bytes += (256.0 + 4.0 * SELL_PMAX * 8 + 4.0) * staged_tiles - 4.0 * (double)hc[3];
    }
    G.codeR.alloc((size_t)nslots * G.wq * 256);
    hipLaunchKernelGGL(sell_regular_codes_kernel, dim3(ntiles), dim3(256), 0, s, ntiles, G.wq, A.ncols, S.ptr.p,
                       G.tile_nseg.p, G.tile_seg.p, S.code.p, G.tile_pinfo.p, G.codeR.p, G.tile_desc.p);
    SA_HIP_CHECK(hipGetLastError());
    return staged_tiles;
}

void build_sell(hipStream_t s, DCsr &A, const Options &opt) {
    A.sell = Sell();      // (a rebuild inherits nothing -- nor the codes of the smoother's diagonal: build_dinv_codes)
    if (A.nrows == 0) return;
    fill_slices(s, A);
    code_slices(s, A, opt);
    const std::array<unsigned long long, 9> h = census(s, A);
    try_dictionary(s, A, opt, h);
    A.sell.fast_ok = (opt.sell & 4) && A.ncols < (1 << 29);      // (bit 2; 32-bit byte offsets into x on the short-chain path)
    const int staged_tiles = plan_staging(s, A, opt, h);
    if ((opt.debug & 2))
        std::fprintf(stderr, "build_sell: staging plan: %d of %d tiles, largest %d doubles, row patterns in %d tiles (at most %d)\n",
                     staged_tiles, div_up(A.sell.nslices, 4), A.sell.stage.cap, A.sell.stage.pat_tiles, A.sell.stage.pat_max);
    if ((opt.debug & 2))
        std::fprintf(stderr, "build_sell: %d rows, slices pair/offset/plain %lld/%lld/%lld, widest %llu, stream bytes %.0f, fast path %d\n",
                     A.nrows, (long long)h[0], (long long)h[1], (long long)h[2], h[7], A.sell.stream_bytes, (int)A.sell.fast_ok);
    A.sell.built = true;
}

// ---- the SpMV family's launches: launch_spmv chooses the format, one launcher per format holds its grid and LDS arithmetic -----
// the rows [row0, row0 + nrows) of the operator: y, b, dinv and dcode start at row0, x is indexed by GLOBAL column (xrow = x + row0)
struct SpmvArgs { int row0, nrows; const double *x, *xrow; double *y; const double *b, *dinv; double scale; const unsigned char *dcode; };
// The XCD deal of the tile kernels (xcd_block): the range's 256-row tiles, eight equal runs of them, one workgroup per tile.
struct TileDeal { int nblocks, per_xcd, grid; };
static TileDeal tile_deal(int nrows) {
    const int nblocks = div_up((long)div_up(nrows, 64) * 64, 256), per_xcd = div_up(nblocks, 8);
    return {nblocks, per_xcd, per_xcd * 8};
}
// ... and of the persistent dictionary kernels: n wavefront-units (slices, or waves of 63 rows) in eight runs, each a whole
// number of 16-wavefront workgroups' trips, walked by at most wg_cap workgroups per XCD.
struct WaveDeal { int per_xcd, wg_per_xcd; };
static WaveDeal wave_deal(int n, int wg_cap) {
    const int per_xcd = div_up(div_up(n, 8), 16) * 16;
    return {per_xcd, std::min(wg_cap, div_up(per_xcd, 16))};
}
// dictionary with 3 x 3 node blocks: waves of 63 rows, numbered over the whole operator; the kernels take whole-operator arrays
template <int MODE> static void launch_dict3(hipStream_t s, const DCsr &A, const SpmvArgs &a) {
    const Sell::Dict &D = A.sell.dict;
    const int row0 = a.row0, nrows = a.nrows;
    const int wave0 = row0 / 63, nw = (row0 + nrows - 1) / 63 - wave0 + 1;
    const WaveDeal d = wave_deal(nw, 64);      // (two workgroups per CU)
    auto kern = sell_gpair3_kernel<MODE>;
    SA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 12 * GP_MAX + 16));
    hipLaunchKernelGGL(kern, dim3(d.wg_per_xcd * 8), dim3(1024), 12 * (size_t)D.ng + 16, s, A.nrows, row0, row0 + nrows, wave0, nw, d.per_xcd,
                       d.wg_per_xcd, D.ng, A.sell.ptr.p, D.gcode.p, (const GPair *)D.gtab.p, a.x, a.y - row0, a.b ? a.b - row0 : nullptr,
                       a.dinv ? a.dinv - row0 : nullptr, a.scale);
    if (!D.nirr) return;
    SA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sell_gpair3_fix_kernel<MODE>, dim3(div_up(D.nirr, 256)), dim3(256), 0, s, D.nirr, D.irr.p, row0, row0 + nrows, A.sell.ptr.p,
                       D.gcode.p, (const GPair *)D.gtab.p, a.x, a.y - row0, a.b ? a.b - row0 : nullptr, a.dinv ? a.dinv - row0 : nullptr, a.scale);
}
template <int MODE> static void launch_dict(hipStream_t s, const DCsr &A, const SpmvArgs &a) {
    const Sell::Dict &D = A.sell.dict;
    const int nsl = div_up(a.nrows, 64);
    const WaveDeal d = wave_deal(nsl, 32);      // (one workgroup per CU)
    const size_t lds = sizeof(GPair) * (size_t)D.ng;
    auto kern = sell_gpair_kernel<MODE>;
    SA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(GPair) * GP_MAX)));
    hipLaunchKernelGGL(kern, dim3(d.wg_per_xcd * 8), dim3(1024), lds, s, a.nrows, a.row0, nsl, d.per_xcd, d.wg_per_xcd, D.ng,
                       A.sell.ptr.p + a.row0 / 64, D.gcode.p, (const GPair *)D.gtab.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow);
}
// staged tiles (a row range of whole tiles: see launch_spmv), and the gather kernel for the tiles that are not staged
template <int MODE> static void launch_staged(hipStream_t s, const DCsr &A, const SpmvArgs &a) {
    const Sell &S = A.sell; const Sell::Stage &G = S.stage;
    const TileDeal d = tile_deal(a.nrows);
    const roff_t *sptr = S.ptr.p + a.row0 / 64;
    const size_t lds_bytes = 8 * (size_t)G.cap + (G.one_table ? 1 : 4) * 64 * sizeof(PairEntry) +
                             (G.patterns() ? SELL_PMAX * 8 * sizeof(unsigned) : 0);
    // (up to eight tiles that are not staged ride at the end of the staged kernel's grid instead of a launch of their own)
    const bool fold = G.regular() && G.nunstaged > 0 && G.nunstaged <= 8 && 8 * (size_t)G.cap >= 4 * 64 * sizeof(PairEntry);
    if (G.regular()) {
        const SellLeftover left{d.grid, fold ? G.nunstaged : 0, G.unstaged.p, sptr, S.col.p, S.val.p, S.ntab.p, S.code.p};
        auto kern = G.patterns() ? sell_staged2_kernel<MODE> : sell_staged2_codes_kernel<MODE>;
        hipLaunchKernelGGL(kern, dim3(d.grid + left.n), dim3(256), lds_bytes, s, left, a.nrows, a.row0, d.nblocks, d.per_xcd, G.cap, A.ncols, G.wq,
                           G.codeR.p, S.tab.p, S.vtab.p, G.tile_desc.p, G.tile_seg.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow, G.row_pat.p, G.tile_pat.p,
                           G.tile_pinfo.p, a.dcode, (const double *)S.dcode.tab.p);
    } else
        hipLaunchKernelGGL((sell_staged_kernel<MODE>), dim3(d.grid), dim3(256), lds_bytes, s, a.nrows, a.row0, d.nblocks, d.per_xcd, G.cap, A.ncols,
                           (int)G.one_table, sptr, S.ntab.p, S.tab.p, S.code.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow, S.vtab.p, G.tile_nseg.p, G.tile_seg.p);
    if (G.nunstaged > 0 && !fold)
        hipLaunchKernelGGL((sell_tiles_kernel<MODE>), dim3(G.nunstaged), dim3(256), 0, s, G.nunstaged, G.unstaged.p, a.nrows, a.row0,
                           sptr, S.col.p, S.val.p, S.ntab.p, S.tab.p, S.code.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow, S.vtab.p);
}
template <int MODE> static void launch_slices(hipStream_t s, const DCsr &A, const SpmvArgs &a) {
    const Sell &S = A.sell;
    const TileDeal d = tile_deal(a.nrows);
    hipLaunchKernelGGL((sell_spmv_kernel<MODE>), dim3(d.grid), dim3(256), 0, s, a.nrows, a.row0, d.nblocks, d.per_xcd, (int)S.fast_ok,
                       S.ptr.p + a.row0 / 64, S.col.p, S.val.p, S.ntab.p, S.tab.p, S.code.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow, S.vtab.p);
}
template <int MODE> static void launch_csr(hipStream_t s, const DCsr &A, const SpmvArgs &a) {
    const int L = A.lanes_per_row;
    const int grid = div_up((long)a.nrows * L, 256);
#define SA_CASE(LL)                                                                              \
    case LL:                                                                                     \
        hipLaunchKernelGGL((spmv_kernel<LL, MODE>), dim3(grid), dim3(256), 0, s, a.nrows,        \
                           A.rowptr.p + a.row0, A.col.p, A.val.p, a.x, a.y, a.b, a.dinv, a.scale, a.xrow); \
        break;
    switch (L) {
        SA_CASE(1) SA_CASE(2) SA_CASE(4) SA_CASE(8) SA_CASE(16) SA_CASE(32) SA_CASE(64)
        default: SA_REQUIRE(false, "bad lanes_per_row");
    }
#undef SA_CASE
}

// Rows [rr.row0, rr.row0 + rr.nrows) of A (row0 a multiple of 64 so that SELL slices line up);
// x is indexed by GLOBAL column, the row-indexed arrays y, b, dinv are global-length too.
template <int MODE>
static void launch_spmv(hipStream_t s, const DCsr &A, RowRange rr, const double *x, double *y, const double *b, const double *dinv, double scale) {
    const int row0 = rr.nrows < 0 ? 0 : rr.row0;
    const int nrows = rr.nrows < 0 ? A.nrows : rr.nrows;
    if (nrows == 0) return;
    SA_REQUIRE(row0 % 64 == 0 && row0 + nrows <= A.nrows, "bad row range");
    const Sell &S = A.sell;
    const SpmvArgs a{row0, nrows, x, x + row0, y + row0, b ? b + row0 : nullptr, dinv ? dinv + row0 : nullptr, scale,
                     S.dcode.for_(dinv) ? S.dcode.code.p + row0 : nullptr};
    // (y += A x with irregular rows: the wave kernel's result for them would be added before the fix kernel adds the right
    // one -- the plain dictionary kernel takes that case)
    if (S.built && S.dict.on && S.dict.bs3 && !(MODE == MODE_ADD && S.dict.nirr > 0)) launch_dict3<MODE>(s, A, a);
    else if (S.built && S.dict.on) launch_dict<MODE>(s, A, a);
    // (tiles are global: a row range takes the staged kernel when it starts on a tile and ends on one or with the operator)
    else if (S.built && S.stage.on() && row0 % 256 == 0 && (nrows % 256 == 0 || row0 + nrows == A.nrows)) launch_staged<MODE>(s, A, a);
    else if (S.built) launch_slices<MODE>(s, A, a);
    else launch_csr<MODE>(s, A, a);
    SA_HIP_CHECK(hipGetLastError());
}

static inline double spmv_bytes(const DCsr &A, RowRange rr) {
    const double frac = (rr.nrows < 0 || A.nrows == 0) ? 1.0 : (double)rr.nrows / A.nrows;
    return (12.0 * A.nnz + 20.0 * A.nrows) * frac;
}
static inline double spmv_rows(const DCsr &A, RowRange rr) { return rr.nrows < 0 ? A.nrows : rr.nrows; }
// bytes of matrix data in the format the kernels run (build_sell's census) + x read and y written once
static inline double spmv_fmt_bytes(const DCsr &A, RowRange rr) {
    if (!A.sell.built) return 0.0;
    const double frac = (rr.nrows < 0 || A.nrows == 0) ? 1.0 : (double)rr.nrows / A.nrows;
    return (A.sell.stream_bytes + 16.0 * A.nrows) * frac;
}
// the SpMV family is listed per operator size: "<name>@<rows>" (the levels of a hierarchy have very different formats)
static inline std::string spmv_label(const char *name, const DCsr &A) { return std::string(name) + "@" + std::to_string(A.nrows); }
static inline double spmv_flops(const DCsr &A, RowRange rr) {
    return 2.0 * A.nnz * ((rr.nrows < 0 || A.nrows == 0) ? 1.0 : (double)rr.nrows / A.nrows);
}

void spmv(hipStream_t s, const DCsr &A, const double *x, double *y, RowRange rr) {
    profiler().begin(s);
    launch_spmv<MODE_PLAIN>(s, A, rr, x, y, nullptr, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv", A).c_str(), spmv_bytes(A, rr), spmv_flops(A, rr), spmv_fmt_bytes(A, rr));
}
void spmv_residual(hipStream_t s, const DCsr &A, const double *x, const double *b, double *r, RowRange rr) {
    profiler().begin(s);
    launch_spmv<MODE_RESIDUAL>(s, A, rr, x, r, b, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv_residual", A).c_str(), spmv_bytes(A, rr) + 8.0 * spmv_rows(A, rr), spmv_flops(A, rr),
                   spmv_fmt_bytes(A, rr) + (A.sell.built ? 8.0 * spmv_rows(A, rr) : 0.0));
}
void spmv_add(hipStream_t s, const DCsr &P, const double *xc, double *x, RowRange rr) {
    profiler().begin(s);
    launch_spmv<MODE_ADD>(s, P, rr, xc, x, nullptr, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv_add", P).c_str(), spmv_bytes(P, rr) + 8.0 * spmv_rows(P, rr), spmv_flops(P, rr),
                   spmv_fmt_bytes(P, rr) + (P.sell.built ? 8.0 * spmv_rows(P, rr) : 0.0));
}
void smooth_step(hipStream_t s, const DCsr &A, const double *dinv_neg, const double *b,
                 const double *xin, double *xout, double scale, RowRange rr) {
    profiler().begin(s);
    launch_spmv<MODE_SMOOTH>(s, A, rr, xin, xout, b, dinv_neg, scale);
    // (b, and D^-1 as it is read: 8 bytes per row, or its byte code where the operator carries one -- build_dinv_codes)
    profiler().end(s, spmv_label("smooth_step", A).c_str(), spmv_bytes(A, rr) + 24.0 * spmv_rows(A, rr), spmv_flops(A, rr),
                   spmv_fmt_bytes(A, rr) + (A.sell.built ? (A.sell.dcode.for_(dinv_neg) ? 9.0 : 16.0) * spmv_rows(A, rr) : 0.0));
}

__global__ __launch_bounds__(256) void smooth_first_kernel(int n, const double *__restrict__ dinv,
                                                           const double *__restrict__ b,
                                                           double *__restrict__ xout, double scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) xout[i] = scale * (dinv[i] * (0.0 - b[i]));
}
void smooth_first(hipStream_t s, int n, const double *dinv_neg, const double *b, double *xout,
                  double scale) {
    if (!n) return;
    profiler().begin(s);
    hipLaunchKernelGGL(smooth_first_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, n, dinv_neg, b,
                       xout, scale);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "smooth_first", 24.0 * n, 2.0 * n);
}

// ---- weighted-l1 smoother diagonal ----------------------------------------------------
// (8 lanes per row: a lane walking its own row alone touches one cache line per lane and load)
__global__ __launch_bounds__(256) void sqrt_abs_diag_kernel(int nrows, const roff_t *__restrict__ rowptr,
                                                            const int *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            double *__restrict__ sd) {
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 7;
    const long row = gtid >> 3;
    if (row >= nrows) return;
    double d = 0.0;
    for (roff_t k = rowptr[row] + lane; k < rowptr[row + 1]; k += 8)
        if (col[k] == row) d += val[k];
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) d += __shfl_down(d, o, 8);
    if (lane == 0) sd[row] = sqrt(fabs(d));
}

template <int L>
__global__ __launch_bounds__(256) void dinv_neg_kernel(int nrows, const roff_t *__restrict__ rowptr,
                                                       const int *__restrict__ col,
                                                       const double *__restrict__ val,
                                                       const double *__restrict__ sd,
                                                       double *__restrict__ out) {
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (L - 1);
    const long row = gtid / L;
    if (row >= nrows) return;
    double sum = 0.0;
    for (roff_t k = rowptr[row] + lane; k < rowptr[row + 1]; k += L) sum += fabs(val[k]) / sd[col[k]];
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, L);
    if (lane == 0) out[row] = -1.0 / (sd[row] * sum);
}

void build_dinv_neg(hipStream_t s, const DCsr &A, double *sd, double *out) {
    if (!A.nrows) return;
    hipLaunchKernelGGL(sqrt_abs_diag_kernel, dim3(div_up((long)A.nrows * 8, 256)), dim3(256), 0, s, A.nrows,
                       A.rowptr.p, A.col.p, A.val.p, sd);
    const int grid = div_up((long)A.nrows * 8, 256);
    hipLaunchKernelGGL((dinv_neg_kernel<8>), dim3(grid), dim3(256), 0, s, A.nrows, A.rowptr.p,
                       A.col.p, A.val.p, sd, out);
    SA_HIP_CHECK(hipGetLastError());
}

// The smoother's diagonal factor as byte codes (Sell::dcode): every value goes into an open-addressing table of 256
// slots (key = its bits); more than 256 distinct values (variable coefficients) -- no codes.  The code of a row is the
// slot of its value, the table is read as doubles.
constexpr unsigned long long DINV_EMPTY = 0x7FF8DEADBEEF0001ull;      // (a NaN payload no diagonal produces)
__device__ inline unsigned dinv_slot0(unsigned long long bits) {
    bits ^= bits >> 33; bits *= 0xFF51AFD7ED558CCDull; bits ^= bits >> 29;
    return (unsigned)bits & 255u;
}
__global__ __launch_bounds__(256) void dinv_tab_kernel(int n, const double *__restrict__ dinv, unsigned long long *__restrict__ tab,
                                                       int *__restrict__ overflow) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || *overflow) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dinv[i]);
    unsigned h = dinv_slot0(bits);
    for (int probe = 0; probe < 256; ++probe, h = (h + 1) & 255u) {
        unsigned long long cur = tab[h];
        if (cur == bits) return;
        if (cur == DINV_EMPTY) {
            cur = atomicCAS(tab + h, DINV_EMPTY, bits);
            if (cur == DINV_EMPTY || cur == bits) return;
        }
    }
    *overflow = 1;
}
__global__ __launch_bounds__(256) void dinv_code_kernel(int n, const double *__restrict__ dinv, const unsigned long long *__restrict__ tab,
                                                        unsigned char *__restrict__ code) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dinv[i]);
    unsigned h = dinv_slot0(bits);
    for (int probe = 0; probe < 256 && tab[h] != bits; ++probe) h = (h + 1) & 255u;
    code[i] = (unsigned char)h;
}
void build_dinv_codes(hipStream_t s, DCsr &A, const double *dinv, const Options &opt) {
    Sell::DCode &D = A.sell.dcode;
    D = {};
    // (only the staged kernel of the coded formats reads them.  Options::sell bit 5, off by default: measured on the 256^3
    // problem, 960 instead of 1 079 MB per application (PMC: 967 / 1 086) and 205.1 instead of 210.5 us -- the kernel is not
    // bound by its bytes alone, 2.3 % for 11 % of them)
    if (!A.nrows || !A.sell.built || !A.sell.stage.regular() || !(opt.sell & 32)) return;
    D.tab.alloc(256);
    std::vector<unsigned long long> empty(256, DINV_EMPTY);
    upload_async(D.tab.p, (const unsigned long long *)empty.data(), 256, s);
    DBuf<int> overflow(1);
    overflow.zero(s);
    SA_HIP_CHECK(hipStreamSynchronize(s));      // (empty is a local)
    hipLaunchKernelGGL(dinv_tab_kernel, dim3(div_up(A.nrows, 256)), dim3(256), 0, s, A.nrows, dinv, D.tab.p, overflow.p);
    SA_HIP_CHECK(hipGetLastError());
    if (overflow.to_host(s)[0]) return;
    D.code.alloc((size_t)A.nrows);
    hipLaunchKernelGGL(dinv_code_kernel, dim3(div_up(A.nrows, 256)), dim3(256), 0, s, A.nrows, dinv, D.tab.p, D.code.p);
    SA_HIP_CHECK(hipGetLastError());
    D.src = dinv;
}

// ---- deterministic dot product (block_sum_256: sparse.h) -----------------------------------
__global__ __launch_bounds__(256) void dot_partial_kernel(int n, const double *__restrict__ a,
                                                          const double *__restrict__ b,
                                                          double *__restrict__ partials) {
    __shared__ double sh[4];
    double v = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        v = fma(a[i], b[i], v);
    const double r = block_sum_256(v, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void dot_final_kernel(int np, const double *__restrict__ partials,
                                                        double *__restrict__ out) {
    __shared__ double sh[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) v += partials[i];
    const double r = block_sum_256(v, sh);
    if (threadIdx.x == 0) out[0] = r;
}

void dot(hipStream_t s, int n, const double *a, const double *b, double *partials, double *out) {
    int grid = div_up(n, 256 * 8);
    if (grid > 1024) grid = 1024;
    if (grid < 1) grid = 1;
    profiler().begin(s);
    hipLaunchKernelGGL(dot_partial_kernel, dim3(grid), dim3(256), 0, s, n, a, b, partials);
    hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, s, grid, partials, out);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "dot", 16.0 * n, 2.0 * n);
}

__global__ __launch_bounds__(256) void pcg_update_xr_kernel(int n, const double *__restrict__ sc,
                                                            double *__restrict__ x,
                                                            double *__restrict__ r,
                                                            const double *__restrict__ d,
                                                            const double *__restrict__ z) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double alpha = sc[0] / sc[1];
    x[i] = fma(alpha, d[i], x[i]);
    r[i] = fma(-alpha, z[i], r[i]);
}
void pcg_update_xr(hipStream_t s, int n, const double *sc, double *x, double *r, const double *d,
                   const double *z) {
    if (!n) return;
    profiler().begin(s);
    hipLaunchKernelGGL(pcg_update_xr_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, n, sc, x, r, d, z);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "pcg_update_xr", 48.0 * n, 4.0 * n);
}

__global__ __launch_bounds__(256) void pcg_update_d_kernel(int n, const double *__restrict__ sc,
                                                           double *__restrict__ d,
                                                           const double *__restrict__ z) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double beta = sc[2] / sc[0];
    d[i] = fma(beta, d[i], z[i]);
}
void pcg_update_d(hipStream_t s, int n, const double *sc, double *d, const double *z) {
    if (!n) return;
    profiler().begin(s);
    hipLaunchKernelGGL(pcg_update_d_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, n, sc, d, z);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "pcg_update_d", 24.0 * n, 2.0 * n);
}

void vec_copy(hipStream_t s, int n, const double *src, double *dst) {
    if (n > 0) copy_device(dst, src, (size_t)n, s);
}
void vec_zero(hipStream_t s, int n, double *dst) {
    if (n) SA_HIP_CHECK(hipMemsetAsync(dst, 0, sizeof(double) * n, s));
}
__global__ __launch_bounds__(256) void axpy_kernel(int n, double a, const double *__restrict__ x,
                                                   double *__restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = fma(a, x[i], y[i]);
}
void vec_axpy(hipStream_t s, int n, double a, const double *x, double *y) {
    if (!n) return;
    hipLaunchKernelGGL(axpy_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, n, a, x, y);
    SA_HIP_CHECK(hipGetLastError());
}

// ---- block members: K columns per launch, every column with the bits of the single kernels ----------------
// The columns of a launch, by value: R roles of BLOCK_MAX pointers each and the mask of the slots that are stored.  A kernel
// of width K reads slots 0 .. K - 1 with compile-time indices (they stay in scalar registers); a slot whose bit is clear
// repeats slot 0, so its loads are valid and its sums are dropped.
template <int R>
struct BlockPtrs {
    double *p[R][BLOCK_MAX];
    unsigned mask;
};
enum { ROLE_X = 0, ROLE_Y = 1, ROLE_B = 2, ROLE_XROW = 3 };
template <int R>
static void set_role(BlockPtrs<R> &v, int role, const Cols &c) {
    for (int j = 0; j < BLOCK_MAX; ++j) v.p[role][j] = c.p[j < c.k ? j : 0];
}
static unsigned cols_mask(const Cols &c) { return (1u << c.k) - 1u; }

// The row's K sums over a slice, as sell_row_general takes its one: the same decoding of the three slice formats, the entry's
// column, value and code loaded ONCE, then K gathers and K fmas into accumulator pair j -- s0 and s1 alternately over whole
// groups of four entries, the tail into s0.  No LDS staging, no preloaded code words: neither changes a sum.
template <int K>
__device__ __forceinline__ void sell_row_general_block(int lane, int grow, int gslice, roff_t beg, roff_t end, int nt,
                                                       const int *__restrict__ col, const double *__restrict__ val,
                                                       const int *__restrict__ tab, const unsigned *__restrict__ codes,
                                                       const double *__restrict__ vtab, double *const (&x)[BLOCK_MAX],
                                                       double (&sum)[K]) {
    const int *cp = col + beg + lane;
    const double *vp = val + beg + lane;
    const int w = (int)((end - beg) >> 6);
    double s0[K], s1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s0[j] = s1[j] = 0.0;
    auto quad = [&](int c0, int c1, int c2, int c3, double v0, double v1, double v2, double v3) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xj = x[j];
            s0[j] = fma(v0, xj[c0], s0[j]);
            s1[j] = fma(v1, xj[c1], s1[j]);
            s0[j] = fma(v2, xj[c2], s0[j]);
            s1[j] = fma(v3, xj[c3], s1[j]);
        }
    };
    auto one = [&](int c, double v) {
#pragma unroll
        for (int j = 0; j < K; ++j) s0[j] = fma(v, x[j][c], s0[j]);
    };
    int k = 0;
    if (nt >= 256) {
        const int np = pair_count(nt);
        const int mytab = (lane < np) ? tab[pair_table_at(gslice, nt) + lane] : 0;
        const double myval = (lane < np) ? vtab[pair_table_at(gslice, nt) + lane] : 0.0;
        const unsigned *wp = code_words(codes, beg, gslice, lane);
        for (; k + 4 <= w; k += 4) {
            const unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            const int i0 = (int)(cw & 255u), i1 = (int)((cw >> 8) & 255u), i2 = (int)((cw >> 16) & 255u), i3 = (int)(cw >> 24);
            quad(grow + __shfl(mytab, i0), grow + __shfl(mytab, i1), grow + __shfl(mytab, i2), grow + __shfl(mytab, i3),
                 __shfl(myval, i0), __shfl(myval, i1), __shfl(myval, i2), __shfl(myval, i3));
        }
        if (k < w) {
            unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            for (; k < w; ++k, cw >>= 8) {
                const int i0 = (int)(cw & 255u);
                one(grow + __shfl(mytab, i0), __shfl(myval, i0));
            }
        }
    } else if (nt >= 0) {
        const int mytab = tab[(size_t)gslice * 64 + lane];
        const unsigned *wp = code_words(codes, beg, gslice, lane);
        for (; k + 4 <= w; k += 4) {
            const unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            const double v0 = __builtin_nontemporal_load(vp + 64 * k), v1 = __builtin_nontemporal_load(vp + 64 * (k + 1));
            const double v2 = __builtin_nontemporal_load(vp + 64 * (k + 2)), v3 = __builtin_nontemporal_load(vp + 64 * (k + 3));
            quad(grow + __shfl(mytab, (int)(cw & 255u)), grow + __shfl(mytab, (int)((cw >> 8) & 255u)),
                 grow + __shfl(mytab, (int)((cw >> 16) & 255u)), grow + __shfl(mytab, (int)(cw >> 24)), v0, v1, v2, v3);
        }
        if (k < w) {
            unsigned cw = __builtin_nontemporal_load(wp + 16 * k);
            for (; k < w; ++k, cw >>= 8) one(grow + __shfl(mytab, (int)(cw & 255u)), __builtin_nontemporal_load(vp + 64 * k));
        }
    }
    for (; k + 4 <= w; k += 4) {
        const int c0 = __builtin_nontemporal_load(cp + 64 * k), c1 = __builtin_nontemporal_load(cp + 64 * (k + 1));
        const int c2 = __builtin_nontemporal_load(cp + 64 * (k + 2)), c3 = __builtin_nontemporal_load(cp + 64 * (k + 3));
        const double v0 = __builtin_nontemporal_load(vp + 64 * k), v1 = __builtin_nontemporal_load(vp + 64 * (k + 1));
        const double v2 = __builtin_nontemporal_load(vp + 64 * (k + 2)), v3 = __builtin_nontemporal_load(vp + 64 * (k + 3));
        quad(c0, c1, c2, c3, v0, v1, v2, v3);
    }
    for (; k < w; ++k) one(__builtin_nontemporal_load(cp + 64 * k), __builtin_nontemporal_load(vp + 64 * k));
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = s0[j] + s1[j];
}

// Whole operators (row0 = 0), one lane per row, 256-row tiles dealt to the XCDs like the single kernels' (tile_deal).
template <int MODE, int K>
__global__ __launch_bounds__(256) void sell_block_kernel(int nrows, int nblocks, int per_xcd, const roff_t *__restrict__ sptr,
                                                         const int *__restrict__ col, const double *__restrict__ val,
                                                         const int *__restrict__ ntab, const int *__restrict__ tab,
                                                         const unsigned *__restrict__ codes, const double *__restrict__ vtab,
                                                         const double *__restrict__ dinv, double scale, BlockPtrs<4> v) {
    const int blk = xcd_block(per_xcd);
    if (blk >= nblocks) return;
    const long row = (long)blk * 256 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane((int)(row >> 6));
    const int lane = threadIdx.x & 63;
    if ((long)slice * 64 >= nrows) return;
    const roff_t beg = sptr[slice], end = sptr[slice + 1];
    const int nt = ntab[slice];
    double sum[K];
    sell_row_general_block<K>(lane, (int)row, slice, beg, end, nt, col, val, tab, codes, vtab, v.p[ROLE_X], sum);
    if (row >= nrows) return;
    const double d = (MODE == MODE_SMOOTH) ? dinv[row] : 0.0;      // (once per row, whatever K)
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (!((v.mask >> j) & 1u)) continue;
        RowTerms t{0.0, d, 0.0};
        if (MODE == MODE_RESIDUAL || MODE == MODE_SMOOTH) t.b = v.p[ROLE_B][j][row];
        if (MODE == MODE_ADD) t.x = v.p[ROLE_Y][j][row];
        if (MODE == MODE_SMOOTH) t.x = v.p[ROLE_XROW][j][row];
        spmv_epilogue<MODE>(sum[j], t, scale, v.p[ROLE_Y][j], row);
    }
}

// The CSR order of spmv_kernel per column: lane l of L takes entries beg + l, beg + l + L, ..., then the __shfl_down tree.
// Plain and add: the modes the cycle (P, R) and the eigensolver (M) use on CSR operators.
template <int L, int MODE, int K>
__global__ __launch_bounds__(256) void spmv_block_kernel(int nrows, const roff_t *__restrict__ rowptr, const int *__restrict__ col,
                                                         const double *__restrict__ val, BlockPtrs<4> v) {
    static_assert(MODE == MODE_PLAIN || MODE == MODE_ADD, "the CSR block kernel has no b and no diagonal");
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (L - 1);
    const long row = gtid / L;
    if (row >= nrows) return;
    const roff_t beg = rowptr[row], end = rowptr[row + 1];
    double sum[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = 0.0;
    for (roff_t k = beg + lane; k < end; k += L) {
        const double a = __builtin_nontemporal_load(val + k);
        const int c = __builtin_nontemporal_load(col + k);
#pragma unroll
        for (int j = 0; j < K; ++j) sum[j] = fma(a, v.p[ROLE_X][j][c], sum[j]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int o = L / 2; o > 0; o >>= 1) sum[j] += __shfl_down(sum[j], o, L);
    }
    if (lane != 0) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (!((v.mask >> j) & 1u)) continue;
        RowTerms t{0.0, 0.0, 0.0};
        if (MODE == MODE_ADD) t.x = v.p[ROLE_Y][j][row];
        spmv_epilogue<MODE>(sum[j], t, 0.0, v.p[ROLE_Y][j], row);
    }
}

template <int MODE, int K>
static void launch_sell_block(hipStream_t s, const DCsr &A, const double *dinv, double scale, const BlockPtrs<4> &v) {
    const Sell &S = A.sell;
    const TileDeal d = tile_deal(A.nrows);
    hipLaunchKernelGGL((sell_block_kernel<MODE, K>), dim3(d.grid), dim3(256), 0, s, A.nrows, d.nblocks, d.per_xcd, S.ptr.p, S.col.p,
                       S.val.p, S.ntab.p, S.tab.p, S.code.p, S.vtab.p, dinv, scale, v);
}
template <int MODE, int K>
static void launch_csr_block(hipStream_t s, const DCsr &A, const BlockPtrs<4> &v) {
    const int L = A.lanes_per_row;
    const int grid = div_up((long)A.nrows * L, 256);
#define SA_CASE(LL)                                                                                                          \
    case LL:                                                                                                                 \
        hipLaunchKernelGGL((spmv_block_kernel<LL, MODE, K>), dim3(grid), dim3(256), 0, s, A.nrows, A.rowptr.p, A.col.p, A.val.p, v); \
        break;
    switch (L) {
        SA_CASE(1) SA_CASE(2) SA_CASE(4) SA_CASE(8) SA_CASE(16) SA_CASE(32) SA_CASE(64)
        default: SA_REQUIRE(false, "bad lanes_per_row");
    }
#undef SA_CASE
}
// The block application of a whole operator.  Which operators run a block kernel is decided by their FORMAT, an observable:
//   SELL copy with the operator-level dictionary   column by column through the single routine (its kernels walk 16-bit codes in a
//                                                  persistent grid: no block form in this change)
//   SELL copy otherwise                            sell_block_kernel (any mix of pair-coded, offset-coded and plain slices)
//   no SELL copy (P, R, a caller's M), plain / add spmv_block_kernel; the other two modes column by column
template <int MODE>
static bool block_kernel_applies(const DCsr &A, int k) {
    const bool csr_ok = MODE == MODE_PLAIN || MODE == MODE_ADD;
    return k > 1 && !(A.sell.built && A.sell.dict.on) && (A.sell.built || csr_ok);
}
template <int MODE>
static void launch_spmv_block(hipStream_t s, const DCsr &A, const Cols &x, const Cols &y, const Cols *b, const double *dinv, double scale) {
    const int k = x.k;
    const Sell &S = A.sell;
    BlockPtrs<4> v;
    set_role(v, ROLE_X, x);
    set_role(v, ROLE_Y, y);
    set_role(v, ROLE_B, b ? *b : x);
    set_role(v, ROLE_XROW, x);
    v.mask = cols_mask(x);
#define SA_WIDTHS(CALL)                          \
    switch (block_width(k)) {                    \
        case 2: CALL(2); break;                  \
        case 4: CALL(4); break;                  \
        default: CALL(8); break;                 \
    }
    if (S.built) {
#define SA_SELL(KK) launch_sell_block<MODE, KK>(s, A, dinv, scale, v)
        SA_WIDTHS(SA_SELL)
#undef SA_SELL
    } else {
        constexpr int CM = (MODE == MODE_PLAIN || MODE == MODE_ADD) ? MODE : MODE_PLAIN;      // (block_kernel_applies: never the other two)
#define SA_CSR(KK) launch_csr_block<CM, KK>(s, A, v)
        SA_WIDTHS(SA_CSR)
#undef SA_CSR
    }
#undef SA_WIDTHS
    SA_HIP_CHECK(hipGetLastError());
}
static void require_spmv_cols(const Cols &x, const Cols &y, const Cols *b) {
    SA_REQUIRE(x.k >= 1 && x.k <= BLOCK_MAX && y.k == x.k && (!b || b->k == x.k), "block SpMV: bad column lists");
}
// bytes in the format the block kernel runs: the matrix data once, the vectors (`per_row` doubles per row) k times
static inline double block_fmt_bytes(const DCsr &A, int k, double per_row) {
    return A.sell.built ? A.sell.stream_bytes + per_row * 8.0 * k * A.nrows : 0.0;
}
// The profile lists a block launch on k columns as k applications under the single-vector label (tests and tools count
// applications per label), with the algorithmic bytes and flops of all k.
void spmv_block(hipStream_t s, const DCsr &A, const Cols &x, const Cols &y) {
    require_spmv_cols(x, y, nullptr);
    if (A.nrows == 0) return;
    if (!block_kernel_applies<MODE_PLAIN>(A, x.k)) {
        for (int j = 0; j < x.k; ++j) spmv(s, A, x.p[j], y.p[j]);
        return;
    }
    profiler().begin(s);
    launch_spmv_block<MODE_PLAIN>(s, A, x, y, nullptr, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv", A).c_str(), x.k * spmv_bytes(A, RowRange()), x.k * spmv_flops(A, RowRange()),
                   block_fmt_bytes(A, x.k, 2.0), x.k);
}
void spmv_residual_block(hipStream_t s, const DCsr &A, const Cols &x, const Cols &b, const Cols &r) {
    require_spmv_cols(x, r, &b);
    if (A.nrows == 0) return;
    if (!block_kernel_applies<MODE_RESIDUAL>(A, x.k)) {
        for (int j = 0; j < x.k; ++j) spmv_residual(s, A, x.p[j], b.p[j], r.p[j]);
        return;
    }
    profiler().begin(s);
    launch_spmv_block<MODE_RESIDUAL>(s, A, x, r, &b, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv_residual", A).c_str(), x.k * (spmv_bytes(A, RowRange()) + 8.0 * A.nrows),
                   x.k * spmv_flops(A, RowRange()), block_fmt_bytes(A, x.k, 3.0), x.k);
}
void spmv_add_block(hipStream_t s, const DCsr &P, const Cols &xc, const Cols &x) {
    require_spmv_cols(xc, x, nullptr);
    if (P.nrows == 0) return;
    if (!block_kernel_applies<MODE_ADD>(P, xc.k)) {
        for (int j = 0; j < xc.k; ++j) spmv_add(s, P, xc.p[j], x.p[j]);
        return;
    }
    profiler().begin(s);
    launch_spmv_block<MODE_ADD>(s, P, xc, x, nullptr, nullptr, 0.0);
    profiler().end(s, spmv_label("spmv_add", P).c_str(), xc.k * (spmv_bytes(P, RowRange()) + 8.0 * P.nrows),
                   xc.k * spmv_flops(P, RowRange()), block_fmt_bytes(P, xc.k, 3.0), xc.k);
}
void smooth_step_block(hipStream_t s, const DCsr &A, const double *dinv_neg, const Cols &b, const Cols &xin, const Cols &xout,
                       double scale) {
    require_spmv_cols(xin, xout, &b);
    if (A.nrows == 0) return;
    if (!block_kernel_applies<MODE_SMOOTH>(A, xin.k)) {
        for (int j = 0; j < xin.k; ++j) smooth_step(s, A, dinv_neg, b.p[j], xin.p[j], xout.p[j], scale);
        return;
    }
    profiler().begin(s);
    launch_spmv_block<MODE_SMOOTH>(s, A, xin, xout, &b, dinv_neg, scale);
    profiler().end(s, spmv_label("smooth_step", A).c_str(), xin.k * (spmv_bytes(A, RowRange()) + 24.0 * A.nrows),
                   xin.k * spmv_flops(A, RowRange()), block_fmt_bytes(A, xin.k, 3.0) + (A.sell.built ? 8.0 * A.nrows : 0.0), xin.k);
}

// ---- block forms of the vector kernels: blockIdx.y is the column, the grid in x and every index are the single kernel's ----
// (the column's pointer by a chain of uniform selects: a run-time index into the by-value struct would go through scratch)
template <int R>
__device__ __forceinline__ double *block_col(const BlockPtrs<R> &v, int role, int j) {
    double *p = v.p[role][0];
#pragma unroll
    for (int q = 1; q < BLOCK_MAX; ++q) p = (j == q) ? v.p[role][q] : p;
    return p;
}
__global__ __launch_bounds__(256) void smooth_first_block_kernel(int n, const double *__restrict__ dinv, double scale, BlockPtrs<2> v) {
    const double *b = block_col(v, 0, blockIdx.y);
    double *xout = block_col(v, 1, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) xout[i] = scale * (dinv[i] * (0.0 - b[i]));
}
__global__ __launch_bounds__(256) void copy_block_kernel(int n, BlockPtrs<2> v) {
    const double *src = block_col(v, 0, blockIdx.y);
    double *dst = block_col(v, 1, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void zero_block_kernel(int n, BlockPtrs<1> v) {
    double *dst = block_col(v, 0, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = 0.0;
}
__global__ __launch_bounds__(256) void axpy_block_kernel(int n, double a, BlockPtrs<2> v) {
    const double *x = block_col(v, 0, blockIdx.y);
    double *y = block_col(v, 1, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = fma(a, x[i], y[i]);
}
// dot's partial and final order per column: column j's partials at partials[1024 j ..]
__global__ __launch_bounds__(256) void dot_partial_block_kernel(int n, BlockPtrs<2> v, double *__restrict__ partials) {
    __shared__ double sh[4];
    const double *a = block_col(v, 0, blockIdx.y), *b = block_col(v, 1, blockIdx.y);
    double acc = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) acc = fma(a[i], b[i], acc);
    const double r = block_sum_256(acc, sh);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * 1024 + blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void dot_final_block_kernel(int np, const double *__restrict__ partials, BlockPtrs<1> v, int slot) {
    __shared__ double sh[4];
    double *out = block_col(v, 0, blockIdx.x);
    const double *mine = partials + (size_t)blockIdx.x * 1024;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += mine[i];
    const double r = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[slot] = r;
}
enum { PCG_SC = 0, PCG_X = 1, PCG_R = 2, PCG_D = 3, PCG_Z = 4 };
__global__ __launch_bounds__(256) void pcg_update_xr_block_kernel(int n, BlockPtrs<5> v) {
    const double *sc = block_col(v, PCG_SC, blockIdx.y);
    double *x = block_col(v, PCG_X, blockIdx.y), *r = block_col(v, PCG_R, blockIdx.y);
    const double *d = block_col(v, PCG_D, blockIdx.y), *z = block_col(v, PCG_Z, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double alpha = sc[0] / sc[1];
    x[i] = fma(alpha, d[i], x[i]);
    r[i] = fma(-alpha, z[i], r[i]);
}
__global__ __launch_bounds__(256) void pcg_update_d_block_kernel(int n, BlockPtrs<3> v) {
    const double *sc = block_col(v, 0, blockIdx.y);
    double *d = block_col(v, 1, blockIdx.y);
    const double *z = block_col(v, 2, blockIdx.y);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double beta = sc[2] / sc[0];
    d[i] = fma(beta, d[i], z[i]);
}
__global__ __launch_bounds__(64) void pcg_shift_nom_block_kernel(BlockPtrs<1> v) {
    double *sc = block_col(v, 0, blockIdx.x);
    if (threadIdx.x == 0) sc[0] = sc[2];
}

static void require_cols(int k, std::initializer_list<const Cols *> cs) {
    SA_REQUIRE(k >= 1 && k <= BLOCK_MAX, "block vector kernel: bad column count");
    for (const Cols *c : cs) SA_REQUIRE(c->k == k, "block vector kernel: column lists of different lengths");
}
void smooth_first_block(hipStream_t s, int n, const double *dinv_neg, const Cols &b, const Cols &xout, double scale) {
    require_cols(b.k, {&xout});
    if (!n) return;
    if (b.k == 1) return smooth_first(s, n, dinv_neg, b.p[0], xout.p[0], scale);
    BlockPtrs<2> v;
    set_role(v, 0, b);
    set_role(v, 1, xout);
    v.mask = cols_mask(b);
    profiler().begin(s);
    hipLaunchKernelGGL(smooth_first_block_kernel, dim3(div_up(n, 256), b.k), dim3(256), 0, s, n, dinv_neg, scale, v);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "smooth_first", 24.0 * n * b.k, 2.0 * n * b.k, 0.0, b.k);
}
void vec_copy_block(hipStream_t s, int n, const Cols &src, const Cols &dst) {
    require_cols(src.k, {&dst});
    if (n <= 0) return;
    if (src.k == 1) return vec_copy(s, n, src.p[0], dst.p[0]);
    BlockPtrs<2> v;
    set_role(v, 0, src);
    set_role(v, 1, dst);
    v.mask = cols_mask(src);
    hipLaunchKernelGGL(copy_block_kernel, dim3(div_up(n, 256), src.k), dim3(256), 0, s, n, v);
    SA_HIP_CHECK(hipGetLastError());
}
void vec_zero_block(hipStream_t s, int n, const Cols &dst) {
    require_cols(dst.k, {});
    if (n <= 0) return;
    if (dst.k == 1) return vec_zero(s, n, dst.p[0]);
    BlockPtrs<1> v;
    set_role(v, 0, dst);
    v.mask = cols_mask(dst);
    hipLaunchKernelGGL(zero_block_kernel, dim3(div_up(n, 256), dst.k), dim3(256), 0, s, n, v);
    SA_HIP_CHECK(hipGetLastError());
}
void vec_axpy_block(hipStream_t s, int n, double a, const Cols &x, const Cols &y) {
    require_cols(x.k, {&y});
    if (!n) return;
    if (x.k == 1) return vec_axpy(s, n, a, x.p[0], y.p[0]);
    BlockPtrs<2> v;
    set_role(v, 0, x);
    set_role(v, 1, y);
    v.mask = cols_mask(x);
    hipLaunchKernelGGL(axpy_block_kernel, dim3(div_up(n, 256), x.k), dim3(256), 0, s, n, a, v);
    SA_HIP_CHECK(hipGetLastError());
}
void dot_block(hipStream_t s, int n, const Cols &a, const Cols &b, double *partials, const Cols &out, int slot) {
    require_cols(a.k, {&b, &out});
    if (a.k == 1) return dot(s, n, a.p[0], b.p[0], partials, out.p[0] + slot);
    int grid = div_up(n, 256 * 8);      // (dot's grid: the partial sums of a column depend on it)
    if (grid > 1024) grid = 1024;
    if (grid < 1) grid = 1;
    BlockPtrs<2> v;
    set_role(v, 0, a);
    set_role(v, 1, b);
    v.mask = cols_mask(a);
    BlockPtrs<1> o;
    set_role(o, 0, out);
    o.mask = v.mask;
    profiler().begin(s);
    hipLaunchKernelGGL(dot_partial_block_kernel, dim3(grid, a.k), dim3(256), 0, s, n, v, partials);
    hipLaunchKernelGGL(dot_final_block_kernel, dim3(a.k), dim3(256), 0, s, grid, partials, o, slot);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "dot", 16.0 * n * a.k, 2.0 * n * a.k, 0.0, a.k);
}
void pcg_update_xr_block(hipStream_t s, int n, const Cols &sc, const Cols &x, const Cols &r, const Cols &d, const Cols &z) {
    require_cols(sc.k, {&x, &r, &d, &z});
    if (!n) return;
    if (sc.k == 1) return pcg_update_xr(s, n, sc.p[0], x.p[0], r.p[0], d.p[0], z.p[0]);
    BlockPtrs<5> v;
    set_role(v, PCG_SC, sc);
    set_role(v, PCG_X, x);
    set_role(v, PCG_R, r);
    set_role(v, PCG_D, d);
    set_role(v, PCG_Z, z);
    v.mask = cols_mask(sc);
    profiler().begin(s);
    hipLaunchKernelGGL(pcg_update_xr_block_kernel, dim3(div_up(n, 256), sc.k), dim3(256), 0, s, n, v);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "pcg_update_xr", 48.0 * n * sc.k, 4.0 * n * sc.k, 0.0, sc.k);
}
void pcg_update_d_block(hipStream_t s, int n, const Cols &sc, const Cols &d, const Cols &z) {
    require_cols(sc.k, {&d, &z});
    if (!n) return;
    if (sc.k == 1) return pcg_update_d(s, n, sc.p[0], d.p[0], z.p[0]);
    BlockPtrs<3> v;
    set_role(v, 0, sc);
    set_role(v, 1, d);
    set_role(v, 2, z);
    v.mask = cols_mask(sc);
    profiler().begin(s);
    hipLaunchKernelGGL(pcg_update_d_block_kernel, dim3(div_up(n, 256), sc.k), dim3(256), 0, s, n, v);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "pcg_update_d", 24.0 * n * sc.k, 2.0 * n * sc.k, 0.0, sc.k);
}
void pcg_shift_nom_block(hipStream_t s, const Cols &sc) {
    require_cols(sc.k, {});
    if (sc.k == 1) return copy_device(sc.p[0], (const double *)sc.p[0] + 2, 1, s);
    BlockPtrs<1> v;
    set_role(v, 0, sc);
    v.mask = cols_mask(sc);
    hipLaunchKernelGGL(pcg_shift_nom_block_kernel, dim3(sc.k), dim3(64), 0, s, v);
    SA_HIP_CHECK(hipGetLastError());
}

}  // namespace saamge_amd
