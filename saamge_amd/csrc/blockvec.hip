// Block-vector kernels of the eigensolver (blockvec.h): one kernel per operation, the widths are arguments.
#include "blockvec.h"

#include "sparse.h"

namespace saamge_amd {

typedef double bv_v4d __attribute__((ext_vector_type(4)));

constexpr int BV_TILES = BV_MAX_COLS / 16;      // 16-column tiles of a block
constexpr int BV_GRAM_MAX_GRID = 512;
constexpr int BV_CHUNKS_PER_WAVE = 8;           // 16-row chunks a wavefront takes at the least before the grid grows

// ---- G = S^T T ------------------------------------------------------------------------------------------------------
// A wavefront takes 16 rows at a time.  Lane l = (l15, l4) holds rows l4, 4 + l4, 8 + l4, 12 + l4 of column 16 t + l15 of
// every tile t: the four lanes of a column read one whole 32-byte sector per load and the 128-byte run over the four
// loads, and element e of every lane is the k-slot l4 of the e-th v_mfma_f64_16x16x4_f64 (A operand: row = lane & 15,
// k = lane >> 4; B operand: column = lane & 15, k = lane >> 4; the same rows on both sides, so which four rows share an
// instruction does not matter).  D register r of tile (ti, tj):
// row 16 ti + l4 + 4 r of G, column 16 tj + l15.  The four wavefronts of a workgroup are added in a fixed order through
// LDS; `partials` holds entry e of workgroup b's p x q sum at e * gridDim.x + b.
__global__ __launch_bounds__(256) void bv_gram_kernel(int n, int p, const double *__restrict__ S, long lds, int q,
                                                      const double *__restrict__ T, long ldt, int sym,
                                                      double *__restrict__ partials) {
    __shared__ double red[3][BV_TILES * BV_TILES * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int pt = (p + 15) >> 4, qt = (q + 15) >> 4;
    bv_v4d acc[BV_TILES][BV_TILES];
#pragma unroll
    for (int ti = 0; ti < BV_TILES; ++ti)
#pragma unroll
        for (int tj = 0; tj < BV_TILES; ++tj) acc[ti][tj] = bv_v4d{0.0, 0.0, 0.0, 0.0};
    const long nchunk = ((long)n + 15) >> 4;
    for (long c = (long)blockIdx.x * 4 + wave; c < nchunk; c += (long)gridDim.x * 4) {
        const long r0 = c * 16 + l4;
        double a[BV_TILES][4], b[BV_TILES][4];
#pragma unroll
        for (int t = 0; t < BV_TILES; ++t) {
            const int col = 16 * t + l15;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[t][e] = (col < p && r0 + 4 * e < n) ? S[(long)col * lds + r0 + 4 * e] : 0.0;
                b[t][e] = sym ? a[t][e] : ((col < q && r0 + 4 * e < n) ? T[(long)col * ldt + r0 + 4 * e] : 0.0);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int ti = 0; ti < BV_TILES; ++ti)
#pragma unroll
                for (int tj = 0; tj < BV_TILES; ++tj)
                    if (ti < pt && tj < qt && (!sym || ti <= tj))
                        acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti][e], b[tj][e], acc[ti][tj], 0, 0, 0);
    }
#pragma unroll
    for (int ti = 0; ti < BV_TILES; ++ti)
#pragma unroll
        for (int tj = 0; tj < BV_TILES; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (wave > 0) red[wave - 1][((ti * BV_TILES + tj) * 4 + r) * 64 + lane] = acc[ti][tj][r];
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int ti = 0; ti < BV_TILES; ++ti)
#pragma unroll
        for (int tj = 0; tj < BV_TILES; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti + l4 + 4 * r, j = 16 * tj + l15, at = ((ti * BV_TILES + tj) * 4 + r) * 64 + lane;
                if (i < p && j < q && (!sym || ti <= tj))
                    partials[(i + (size_t)j * p) * gridDim.x + blockIdx.x] = (acc[ti][tj][r] + red[0][at]) + (red[1][at] + red[2][at]);
            }
}

// The sum of the nslab partials of one entry by one wavefront, in a fixed order: lane l adds the partials l, l + 64, ... in
// index order, then the lanes are added by the shuffle tree of block_sum_256 (valid on lane 0).
__device__ inline double wave_sum_partials(const double *__restrict__ p, int nslab) {
    double v = 0.0;
    for (int b = threadIdx.x & 63; b < nslab; b += 64) v += p[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// G: one wavefront per entry; the tiles below the diagonal of a symmetric product are the mirrored ones
__global__ __launch_bounds__(256) void bv_gram_final_kernel(int p, int q, int sym, int nslab, const double *__restrict__ partials,
                                                            double *__restrict__ G) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= p * q) return;
    const int i = e % p, j = e / p;
    const int src = (sym && (i >> 4) > (j >> 4)) ? j + i * p : e;
    const double v = wave_sum_partials(partials + (size_t)src * nslab, nslab);
    if ((threadIdx.x & 63) == 0) G[e] = v;
}

static int gram_grid(int n) {
    const long nchunk = ((long)n + 15) / 16;
    const long g = (nchunk + 4 * BV_CHUNKS_PER_WAVE - 1) / (4 * BV_CHUNKS_PER_WAVE);
    return (int)std::max(1L, std::min(g, (long)BV_GRAM_MAX_GRID));
}

size_t bv_gram_scratch(int n, int p, int q) { return (size_t)gram_grid(n) * p * q; }

void bv_gram(hipStream_t s, int n, int p, const double *S, long lds, int q, const double *T, long ldt, double *scratch,
             double *G) {
    SA_REQUIRE(n >= 1 && p >= 1 && p <= BV_MAX_COLS && q >= 1 && q <= BV_MAX_COLS && lds >= n && ldt >= n, "bv_gram: bad shape");
    const int sym = (T == S && ldt == lds && q == p) ? 1 : 0, grid = gram_grid(n);
    profiler().begin(s);
    hipLaunchKernelGGL(bv_gram_kernel, dim3(grid), dim3(256), 0, s, n, p, S, lds, q, T, ldt, sym, scratch);
    hipLaunchKernelGGL(bv_gram_final_kernel, dim3(div_up(p * q, 4)), dim3(256), 0, s, p, q, sym, grid, scratch, G);
    SA_HIP_CHECK(hipGetLastError());
    const double pairs = sym ? 0.5 * p * (p + 1) : (double)p * q;
    profiler().end(s, "bv_gram", 8.0 * n * (sym ? p : p + q), 2.0 * n * pairs);
}

// ---- Y = S C --------------------------------------------------------------------------------------------------------
// One thread per row: its row of S in registers (the columns beyond p are zero, and so are those rows of the LDS copy of
// C, so the products run over whole 16-column tiles), one fused multiply-add chain per output column in the order of k.
__global__ __launch_bounds__(256) void bv_combine_kernel(int n, int p, int q, const double *__restrict__ C, int accumulate,
                                                         BvBlocks B, long lds, long ldy) {
    __shared__ double Cs[BV_MAX_COLS * BV_MAX_COLS];     // Cs[j][k]
    for (int e = threadIdx.x; e < BV_MAX_COLS * q; e += 256) {
        const int k = e % BV_MAX_COLS, j = e / BV_MAX_COLS;
        Cs[e] = k < p ? C[k + (size_t)j * p] : 0.0;
    }
    __syncthreads();
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const double *S = B.S[blockIdx.y];      // may alias Y: no __restrict__
    double *Y = B.Y[blockIdx.y];
    const int pt = (p + 15) >> 4;
    double sv[BV_MAX_COLS];
#pragma unroll
    for (int t = 0; t < BV_TILES; ++t)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = 16 * t + u;
            sv[k] = (t < pt && k < p) ? S[(long)k * lds + row] : 0.0;
        }
    for (int j = 0; j < q; ++j) {
        double acc = accumulate ? Y[(long)j * ldy + row] : 0.0;
#pragma unroll
        for (int t = 0; t < BV_TILES; ++t)
            if (t < pt) {
#pragma unroll
                for (int u = 0; u < 16; ++u) acc = fma(sv[16 * t + u], Cs[j * BV_MAX_COLS + 16 * t + u], acc);
            }
        Y[(long)j * ldy + row] = acc;
    }
}

void bv_combine(hipStream_t s, int n, int p, int q, const double *C, bool accumulate, const BvBlocks &B, long lds, long ldy) {
    SA_REQUIRE(n >= 1 && p >= 1 && p <= BV_MAX_COLS && q >= 1 && q <= BV_MAX_COLS && lds >= n && ldy >= n &&
               B.count >= 1 && B.count <= 3, "bv_combine: bad shape");
    profiler().begin(s);
    hipLaunchKernelGGL(bv_combine_kernel, dim3(div_up(n, 256), B.count), dim3(256), 0, s, n, p, q, C, accumulate ? 1 : 0, B, lds, ldy);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "bv_combine", 8.0 * n * B.count * (p + q + (accumulate ? q : 0)), 2.0 * n * B.count * p * q);
}

bool bv_combine_aliasing_ok(int n, int p, const double *S, long lds, int q, const double *Y, long ldy) {
    if (Y == S && ldy == lds) return true;
    const double *s_end = S + (size_t)(p - 1) * lds + n, *y_end = Y + (size_t)(q - 1) * ldy + n;
    return y_end <= S || s_end <= Y;
}

// ---- R = AX - MX diag(lam) and the column norms -----------------------------------------------------------------------
constexpr int BV_RES_MAX_GRID = 256;      // workgroups per column

// blockIdx.y is the column: two running sums per lane and coalesced columns
__global__ __launch_bounds__(256) void bv_residual_kernel(int n, const double *__restrict__ AX, const double *MX, long ld,
                                                          const double *__restrict__ lam, double *__restrict__ R, long ldr,
                                                          double *__restrict__ partials) {
    __shared__ double sh[4];
    const int j = blockIdx.y;
    const double *ax = AX + (long)j * ld, *mx = MX + (long)j * ld;
    double *r_out = R + (long)j * ldr;
    const double l = lam[j];
    double rr = 0.0, mm = 0.0;
    for (long row = (long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long)gridDim.x * 256) {
        const double m = mx[row];
        const double r = fma(-l, m, ax[row]);
        r_out[row] = r;
        rr = fma(r, r, rr);
        mm = fma(m, m, mm);
    }
    const double a = block_sum_256(rr, sh), b = block_sum_256(mm, sh);
    if (threadIdx.x == 0) {
        partials[(size_t)j * gridDim.x + blockIdx.x] = a;
        partials[(size_t)(BV_MAX_NORMS + j) * gridDim.x + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(256) void bv_residual_final_kernel(int nb, int nslab, const double *__restrict__ partials,
                                                                double *__restrict__ norms) {
    for (int e = threadIdx.x >> 6; e < 2 * BV_MAX_NORMS; e += 4) {
        const bool on = (e & (BV_MAX_NORMS - 1)) < nb;
        const double v = on ? wave_sum_partials(partials + (size_t)e * nslab, nslab) : 0.0;
        if ((threadIdx.x & 63) == 0) norms[e] = sqrt(v);
    }
}

static int residual_grid(int n) { return std::max(1, std::min(div_up(n, 256 * 4), BV_RES_MAX_GRID)); }

size_t bv_residual_scratch(int n) { return (size_t)residual_grid(n) * 2 * BV_MAX_NORMS; }

void bv_residual(hipStream_t s, int n, int nb, const double *AX, const double *MX, long ld, const double *lam, double *R,
                 long ldr, double *scratch, double *norms) {
    SA_REQUIRE(n >= 1 && nb >= 1 && nb <= BV_MAX_NORMS && ld >= n && ldr >= n, "bv_residual: bad shape");
    const int grid = residual_grid(n);
    profiler().begin(s);
    hipLaunchKernelGGL(bv_residual_kernel, dim3(grid, nb), dim3(256), 0, s, n, AX, MX, ld, lam, R, ldr, scratch);
    hipLaunchKernelGGL(bv_residual_final_kernel, dim3(1), dim3(256), 0, s, nb, grid, scratch, norms);
    SA_HIP_CHECK(hipGetLastError());
    profiler().end(s, "bv_residual", 8.0 * n * nb * 3, 6.0 * n * nb);
}

// ---- mask and start block --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bv_mask_kernel(int n, const signed char *__restrict__ flags, int bit, double *__restrict__ V,
                                                      long ld) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row < n && (flags[row] & bit)) V[(long)blockIdx.y * ld + row] = 0.0;
}

void bv_mask(hipStream_t s, int n, int ncols, const signed char *flags, int bit, double *V, long ld) {
    if (ncols < 1) return;
    hipLaunchKernelGGL(bv_mask_kernel, dim3(div_up(n, 256), ncols), dim3(256), 0, s, n, flags, bit, V, ld);
    SA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void bv_hash_start_kernel(int n, unsigned seed, double *__restrict__ X, long ld) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const unsigned j = blockIdx.y;
    unsigned h = (seed * 0x9E3779B9u) ^ ((unsigned)row * 0x85EBCA6Bu) ^ (j * 0xC2B2AE35u + 0x27D4EB2Fu);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    X[(long)j * ld + row] = (double)h * 0x1p-31 - 1.0;
}

void bv_hash_start(hipStream_t s, int n, int nb, unsigned seed, double *X, long ld) {
    hipLaunchKernelGGL(bv_hash_start_kernel, dim3(div_up(n, 256), nb), dim3(256), 0, s, n, seed, X, ld);
    SA_HIP_CHECK(hipGetLastError());
}

}  // namespace saamge_amd
