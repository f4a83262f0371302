// The shared pieces of the device index tables that are not templates: see devtab.h.
#include "devtab.h"

namespace saamge_amd {

__global__ __launch_bounds__(256) void dev_histogram_kernel(long n, const int *__restrict__ key, int *__restrict__ cnt) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[key[i]], 1);
}
void dev_histogram(hipStream_t s, long n, const int *key, int *cnt) { launch_flat(s, n, dev_histogram_kernel, key, cnt); }

// exclusive scan of ints, three small kernels (tile = 1024); OUT = int, or roff_t for the row offsets of an
// operator (counts are int, their running sum may pass 2^31)
template <class OUT>
__global__ __launch_bounds__(256) void scan_tile_kernel(int n, const int *__restrict__ in,
                                                        OUT *__restrict__ out, OUT *__restrict__ tsum) {
    __shared__ OUT sh[256];
    const long base = (long)blockIdx.x * 1024;
    int v[4];
    OUT run = 0;
    for (int q = 0; q < 4; ++q) {
        const long i = base + threadIdx.x * 4 + q;
        v[q] = (i < n) ? in[i] : 0;
        run += v[q];
    }
    sh[threadIdx.x] = run;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const OUT t = (threadIdx.x >= o) ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    OUT excl = sh[threadIdx.x] - run;
    for (int q = 0; q < 4; ++q) {
        const long i = base + threadIdx.x * 4 + q;
        if (i < n) out[i] = excl;
        excl += v[q];
    }
    if (threadIdx.x == 255) tsum[blockIdx.x] = sh[255];
}
template <class OUT>
__global__ __launch_bounds__(256) void scan_sums_kernel(int nt, OUT *__restrict__ tsum, OUT *__restrict__ total) {
    __shared__ OUT sh[256];
    __shared__ OUT carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nt; base += 256) {
        const int i = base + threadIdx.x;
        const OUT x = (i < nt) ? tsum[i] : 0;
        sh[threadIdx.x] = x;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const OUT t = (threadIdx.x >= o) ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nt) tsum[i] = carry + sh[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 255) carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
template <class OUT>
__global__ __launch_bounds__(256) void scan_add_kernel(int n, OUT *__restrict__ out,
                                                       const OUT *__restrict__ tsum,
                                                       const OUT *__restrict__ total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += tsum[i >> 10];
    if (i == 0) out[n] = *total;
}

// out has n+1 entries
template <class OUT>
static void exclusive_scan_t(hipStream_t s, int n, const int *in, OUT *out) {
    const int nt = div_up(n, 1024);
    DBuf<OUT> tsum((size_t)nt + 1);
    hipLaunchKernelGGL(scan_tile_kernel<OUT>, dim3(nt), dim3(256), 0, s, n, in, out, tsum.p);
    hipLaunchKernelGGL(scan_sums_kernel<OUT>, dim3(1), dim3(256), 0, s, nt, tsum.p, tsum.p + nt);
    hipLaunchKernelGGL(scan_add_kernel<OUT>, dim3(div_up(n, 256)), dim3(256), 0, s, n, out, (const OUT *)tsum.p, (const OUT *)(tsum.p + nt));
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));  // tsum is freed on return
}
void exclusive_scan_int(hipStream_t s, int n, const int *in, int *out) { exclusive_scan_t<int>(s, n, in, out); }
void exclusive_scan_int_async(hipStream_t s, int n, const int *in, int *out, int *tsum) {
    const int nt = div_up(n, 1024);
    hipLaunchKernelGGL(scan_tile_kernel<int>, dim3(nt), dim3(256), 0, s, n, in, out, tsum);
    hipLaunchKernelGGL(scan_sums_kernel<int>, dim3(1), dim3(256), 0, s, nt, tsum, tsum + nt);
    hipLaunchKernelGGL(scan_add_kernel<int>, dim3(div_up(n, 256)), dim3(256), 0, s, n, out, (const int *)tsum, (const int *)(tsum + nt));
    SA_HIP_CHECK(hipGetLastError());
}
void exclusive_scan_off(hipStream_t s, int n, const int *in, roff_t *out) { exclusive_scan_t<roff_t>(s, n, in, out); }

// ---- transpose of an int CSR table ---------------------------------------------------------------------------------------
// one lane per row of (I, J): its entries go to the rows of (TI, TJ) they name, at the places the cursors hand out
__global__ __launch_bounds__(256) void dev_table_fill_kernel(int nrows, const int *__restrict__ I, const int *__restrict__ J,
                                                             const int *__restrict__ TI, int *__restrict__ cursor,
                                                             int *__restrict__ TJ) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nrows) return;
    for (int k = I[e]; k < I[e + 1]; ++k) {
        const int d = J[k];
        TJ[TI[d] + atomicAdd(&cursor[d], 1)] = (int)e;
    }
}
__global__ __launch_bounds__(256) void dev_table_sort_kernel(int nrows, const int *__restrict__ TI, int *__restrict__ TJ) {
    const long d = (long)blockIdx.x * 256 + threadIdx.x;
    if (d >= nrows) return;
    const int b = TI[d], e = TI[d + 1];
    for (int i = b + 1; i < e; ++i) {  // insertion sort, rows are short
        const int v = TJ[i];
        int j = i - 1;
        while (j >= b && TJ[j] > v) { TJ[j + 1] = TJ[j]; --j; }
        TJ[j + 1] = v;
    }
}
// after the scan: the counters become the cursors
static void table_fill(hipStream_t s, int nrows, const int *I, const int *J, int ncols, int *cnt, const int *TI, int *TJ,
                       bool sort_rows) {
    SA_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)ncols, s));
    launch_flat(s, nrows, dev_table_fill_kernel, I, J, TI, cnt, TJ);
    if (sort_rows) launch_flat(s, ncols, dev_table_sort_kernel, TI, TJ);
}
void dev_table_finish(hipStream_t s, int nrows, const int *I, const int *J, int ncols, int *cnt, int *TI, int *TJ, bool sort_rows) {
    exclusive_scan_int(s, ncols, cnt, TI);
    table_fill(s, nrows, I, J, ncols, cnt, TI, TJ, sort_rows);
}
void dev_table_transpose(hipStream_t s, int nrows, const int *I, const int *J, long nnz, int ncols, int *TI, int *TJ, bool sort_rows,
                         int *cnt) {
    SA_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)ncols, s));
    dev_histogram(s, nnz, J, cnt);
    dev_table_finish(s, nrows, I, J, ncols, cnt, TI, TJ, sort_rows);
}
void dev_table_transpose_async(hipStream_t s, int nrows, const int *I, const int *J, long nnz, int ncols, int *TI, int *TJ,
                               bool sort_rows, int *cnt, int *tile_sums) {
    SA_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)ncols, s));
    dev_histogram(s, nnz, J, cnt);
    exclusive_scan_int_async(s, ncols, cnt, TI, tile_sums);
    table_fill(s, nrows, I, J, ncols, cnt, TI, TJ, sort_rows);
}

// ---- compaction by flag ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dev_compact_kernel(long n, const int *__restrict__ flag, const int *__restrict__ pos,
                                                          int *__restrict__ list) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) list[pos[i]] = (int)i;
}
void dev_compact_scatter(hipStream_t s, int n, const int *flag, const int *pos, int *list) {
    launch_flat(s, n, dev_compact_kernel, flag, pos, list);
}
int dev_compact(hipStream_t s, int n, const int *flag, int *pos, DBuf<int> &list) {
    exclusive_scan_int(s, n, flag, pos);
    const int m = read_one((const int *)pos + n, s);
    list.alloc((size_t)m);
    if (m) dev_compact_scatter(s, n, flag, pos, list.p);
    return m;
}

}  // namespace saamge_amd
