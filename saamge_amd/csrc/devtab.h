// The shared pieces of the device index tables (dof -> element, agglomerate -> element, MIS -> dof, coarse row lists, halo
// lists, face tables, the partitioner's graphs): the flat launch, the elementwise kernels, the exclusive scans, the transpose
// of an int CSR table and the compaction by flag.  The radix sorts are in devsort.h (the only header that brings in hipcub).
// DESIGN.md section 4.19 says what each piece promises and which call sites kept a shape of their own.
#pragma once
#include "common.h"

namespace saamge_amd {

// One lane per item, 256 lanes per workgroup: kernel(n, args...).  n = 0 launches one workgroup that finds nothing to do
// (grid_flat); callers that skip the launch for n = 0 guard it themselves.
template <class K, class... A>
inline void launch_flat(hipStream_t s, long n, K kernel, A... args) {
    hipLaunchKernelGGL(kernel, grid_flat(n), dim3(256), 0, s, n, args...);
    SA_HIP_CHECK(hipGetLastError());
}

// ---- elementwise: one kernel template and one wrapper each; n = 0 is launch_flat's empty workgroup ---------------------------
template <class T>
__global__ __launch_bounds__(256) void dev_fill_kernel(long n, T v, T *__restrict__ p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
template <class T>
__global__ __launch_bounds__(256) void dev_iota_kernel(long n, T scale, T *__restrict__ p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = (T)(i * scale);
}
template <class Out, class In>
__global__ __launch_bounds__(256) void dev_convert_kernel(long n, const In *__restrict__ in, Out *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (Out)in[i];
}
template <class T>
__global__ __launch_bounds__(256) void dev_gather_kernel(long n, const int *__restrict__ idx, const T *__restrict__ src,
                                                         T *__restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
template <class T>
__global__ __launch_bounds__(256) void dev_scatter_kernel(long n, const int *__restrict__ idx, const T *__restrict__ src,
                                                          T *__restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[idx[i]] = src[i];
}
// p[i] = v
template <class T>
inline void dev_fill(hipStream_t s, long n, T v, T *p) { launch_flat(s, n, dev_fill_kernel<T>, v, p); }
// p[i] = i * scale
template <class T>
inline void dev_iota(hipStream_t s, long n, T scale, T *p) { launch_flat(s, n, dev_iota_kernel<T>, scale, p); }
// out[i] = in[i], widened or narrowed (the caller has checked that narrowed values fit)
template <class Out, class In>
inline void dev_convert(hipStream_t s, long n, const In *in, Out *out) { launch_flat(s, n, dev_convert_kernel<Out, In>, in, out); }
// dst[i] = src[idx[i]]
template <class T>
inline void dev_gather(hipStream_t s, long n, const int *idx, const T *src, T *dst) {
    launch_flat(s, n, dev_gather_kernel<T>, idx, src, dst);
}
// dst[idx[i]] = src[i]
template <class T>
inline void dev_scatter(hipStream_t s, long n, const int *idx, const T *src, T *dst) {
    launch_flat(s, n, dev_scatter_kernel<T>, idx, src, dst);
}

// ---- devtab.hip ------------------------------------------------------------------------------------------------------------
// cnt[key[i]] += 1, one atomic per item; the caller has zeroed cnt
void dev_histogram(hipStream_t s, long n, const int *key, int *cnt);

// Exclusive scans of n ints; out has n + 1 entries, out[n] is the total.  n = 0 is not served: the tile and add kernels
// would be launched over a grid of no workgroups, which the runtime reports as an error -- callers keep n = 0 away.
// exclusive_scan_int and exclusive_scan_off synchronise the stream (callers read host values right after them).
void exclusive_scan_int(hipStream_t s, int n, const int *in, int *out);
// the same without any host synchronisation: `tile_sums` is the caller's scratch of div_up(n, 1024) + 1 ints
void exclusive_scan_int_async(hipStream_t s, int n, const int *in, int *out, int *tile_sums);
// roff_t sums of int counts (the running sum may pass 2^31)
void exclusive_scan_off(hipStream_t s, int n, const int *in, roff_t *out);

// Transpose of an int CSR table (I, J) of nrows rows, nnz entries and columns [0, ncols) into (TI, TJ): TI has ncols + 1
// entries, TJ nnz.  With sort_rows every row of TJ ascends (one lane per row, insertion sort: rows are short); without, a row
// holds its entries in the order the atomics gave.  ncols = 0 is the scan's n = 0 (an error); nrows = 0 or nnz = 0 are
// launch_flat's empty workgroups.
// `cnt` is the caller's scratch of ncols ints in every form (it must outlive the queued fill, and none of the forms waits
// for that): the counters first, the cursors of the fill afterwards.
//   dev_table_transpose        zeroes and counts, scans with exclusive_scan_int (which synchronises); the fill and the sort
//                              are enqueued after that and not waited for
//   dev_table_finish           the same after the count, for a caller that looks at the counts in between: `cnt` holds the
//                              caller's dev_histogram of J
//   dev_table_transpose_async  scans with exclusive_scan_int_async into the caller's `tile_sums` (div_up(ncols, 1024) + 1
//                              ints); enqueues on `s` alone and never synchronises
void dev_table_transpose(hipStream_t s, int nrows, const int *I, const int *J, long nnz, int ncols, int *TI, int *TJ, bool sort_rows,
                         int *cnt);
void dev_table_finish(hipStream_t s, int nrows, const int *I, const int *J, int ncols, int *cnt, int *TI, int *TJ, bool sort_rows);
void dev_table_transpose_async(hipStream_t s, int nrows, const int *I, const int *J, long nnz, int ncols, int *TI, int *TJ,
                               bool sort_rows, int *cnt, int *tile_sums);

// list[pos[i]] = i for every i < n with flag[i] != 0: the scatter of a compaction whose positions are already scanned
void dev_compact_scatter(hipStream_t s, int n, const int *flag, const int *pos, int *list);
// list = the i < n with flag[i] != 0, ascending; pos: scratch of n + 1 ints.  Returns their number (synchronises: the scan
// and the read of the total); the scatter is skipped when there are none.  n = 0 is the scan's n = 0.
int dev_compact(hipStream_t s, int n, const int *flag, int *pos, DBuf<int> &list);

}  // namespace saamge_amd
