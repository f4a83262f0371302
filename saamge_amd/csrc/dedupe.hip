// Duplicate inputs of the setup: the class search every stage shares, the words of an agglomerate matrix, the registry of a
// level's classes (dedupe.h).
#include "dedupe.h"
#include "eig.h"

#include <algorithm>

namespace saamge_amd {

// ---------------------------------------------------------------------------------------
// Duplicate agglomerate matrices (round 4)
// ---------------------------------------------------------------------------------------
// On a structured mesh with piecewise constant coefficients most agglomerates are translates of one another: their
// scaled matrices C, scalings D and row orders are IDENTICAL bit for bit (the 256^3 Poisson problem: 65 536 agglomerates
// on the fine level, a few hundred distinct ones; the same on the coarse levels, whose element matrices are built from
// identical eigenvectors by order-preserving sums).  The eigenpairs of a matrix are a function of those bits alone -- no
// kernel of the few-eigenpairs or the dense path looks at a matrix's position in its batch, the start vectors are seeded
// by (row, n) -- so one member of every class is solved and the others receive copies: the hierarchy is the one the
// per-agglomerate computation builds.  Classes are found by a 128-bit hash of everything the eigensolvers read (n, the
// half bandwidth, the band of C in both triangles, D^-1/2, the row order, the coarse start vector) and CONFIRMED by a
// word-by-word comparison with the class representative; a batch with fewer than a quarter of duplicates is left alone
// (variable coefficients, unstructured meshes: the cost is the hash, one pass over the bands).
// saamge_amd_options.eig_dedupe = 0 switches it off.
// The same search -- hash, group, "fewer than a quarter duplicates: leave alone", verify -- runs on the inputs of the assembly,
// on the inputs of the coarse element matrices (assemble.hip) and, grouped on the device, on the MISes (mis.hip): the stages
// bring their own walk over the words of an item and share dd_mix / DdHash (dedupe.h) and dedupe_classes below.

// The words a matrix consists of, in a fixed order (DdSource, dedupe.h).  kind 1, the assembled matrix: the band of C in both
// triangles (column by column, 2 bw + 1 slots per column, slots outside the matrix = 0), D^-1/2, the row order, the coarse
// start vector, n and bw.  kind 0, the sparse rows the fused fine-level assembly builds the matrix from: values, columns,
// the row order, n.
__device__ inline long dd_count(const DdSource &v, int b) {
    return dd_words(v.kind, v.ns[b], v.kind == 0 ? 0 : v.bws[b], v.RW);
}
__device__ inline unsigned long long dd_word(const DdSource &v, int b, long idx) {
    const long n = v.ns[b];
    const int64_t vo = v.voff[b];
    if (v.kind == 0) {
        const long nr = n * v.RW;
        if (idx < nr) return (unsigned long long)__double_as_longlong(v.rvals[(size_t)vo * v.RW + idx]);
        if (idx < 2 * nr) return (unsigned long long)(unsigned short)v.rcols[(size_t)vo * v.RW + (idx - nr)];
        if (idx < 2 * nr + n) return v.perm ? (unsigned long long)(unsigned short)v.perm[vo + (idx - 2 * nr)] : 0ull;
        return (unsigned long long)n;
    }
    const long bw = min(v.bws[b], (int)n - 1), w2 = 2 * bw + 1, nb = n * w2;
    if (idx < nb) {
        const long j = idx / w2, i = j - bw + (idx - j * w2);
        return (i >= 0 && i < n) ? (unsigned long long)__double_as_longlong(v.W[v.moff[b] + (size_t)j * n + i]) : 0ull;
    }
    idx -= nb;
    if (idx < n) return (unsigned long long)__double_as_longlong(v.dis[vo + idx]);
    if (idx < 2 * n) return v.perm ? (unsigned long long)(unsigned short)v.perm[vo + (idx - n)] : 0ull;
    if (idx < 3 * n) return v.x0c ? (unsigned long long)__double_as_longlong(v.x0c[vo + (idx - 2 * n)]) : 0ull;
    return idx == 3 * n ? (unsigned long long)n : (unsigned long long)bw;
}
// kind 0, the two long arrays of a matrix (values, then columns): four words per thread and trip, their loads requested
// together (dd_word's chain of branches kept one load in flight per thread).  fn(word, idx) sees every word of [0, 2 nr).
template <class F>
__device__ inline void dd_rows_words(const DdSource &v, int b, long start, long stride, F fn) {
    const long nr = (long)v.ns[b] * v.RW;
    const double *rv = v.rvals + (size_t)v.voff[b] * v.RW;
    const short *rc = v.rcols + (size_t)v.voff[b] * v.RW;
    for (long i0 = start; i0 < nr; i0 += 4 * stride) {
        double x[4];
        short c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = min(i0 + u * stride, nr - 1);
            x[u] = rv[i];
            c[u] = rc[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * stride < nr) {
                fn((unsigned long long)__double_as_longlong(x[u]), i0 + u * stride);
                fn((unsigned long long)(unsigned short)c[u], nr + i0 + u * stride);
            }
    }
}
// grid (matrices, y): partial 128-bit sums of the mixed (word, position) pairs, added into out[2 q], out[2 q + 1] (zeroed);
// list = null: matrix q of the batch, otherwise matrix list[q]
__global__ __launch_bounds__(256) void dd_hash_kernel(DdSource v, const int *__restrict__ list, unsigned long long *__restrict__ out) {
    const int b = list ? list[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
    const long cnt = dd_count(v, b);
    DdHash h;
    auto add = [&](unsigned long long w, long idx) { h.add(w, (unsigned long long)idx); };
    long first = 0;
    if (v.kind == 0) {
        dd_rows_words(v, b, (long)blockIdx.y * 256 + tid, 256l * gridDim.y, add);
        first = 2l * v.ns[b] * v.RW;      // (the short tail -- row order, n -- through dd_word)
    }
    for (long idx = first + (long)blockIdx.y * 256 + tid; idx < cnt; idx += 256l * gridDim.y) add(dd_word(v, b, idx), idx);
    h.block_finish<true>(out, blockIdx.x);
}
// every matrix against the first of its class (rep[b] = that matrix): differ[b] = 1 unless every word is the same
__global__ __launch_bounds__(256) void dd_verify_kernel(DdSource v, const int *__restrict__ rep, int *__restrict__ differ) {
    const int b = blockIdx.x, r0 = rep[b], tid = threadIdx.x;
    if (r0 == b) return;
    const long cnt = dd_count(v, b);
    if (cnt != dd_count(v, r0)) { if (tid == 0) differ[b] = 1; return; }
    int bad = 0;
    long first = 0;
    if (v.kind == 0) {      // (the two long arrays four words at a time, both matrices' loads in flight together)
        const long nr = (long)v.ns[b] * v.RW, stride = 256l * gridDim.y;
        const double *rv = v.rvals + (size_t)v.voff[b] * v.RW, *rv0 = v.rvals + (size_t)v.voff[r0] * v.RW;
        const short *rc = v.rcols + (size_t)v.voff[b] * v.RW, *rc0 = v.rcols + (size_t)v.voff[r0] * v.RW;
        for (long i0 = (long)blockIdx.y * 256 + tid; i0 < nr; i0 += 4 * stride) {
            long long x[4], y[4];
            short c[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = min(i0 + u * stride, nr - 1);
                x[u] = __double_as_longlong(rv[i]);
                y[u] = __double_as_longlong(rv0[i]);
                c[u] = rc[i];
                d[u] = rc0[i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) bad |= (x[u] != y[u]) | (c[u] != d[u]);
        }
        first = 2 * nr;
    }
    for (long idx = first + (long)blockIdx.y * 256 + tid; idx < cnt; idx += 256l * gridDim.y) bad |= dd_word(v, b, idx) != dd_word(v, r0, idx);
    if (bad) differ[b] = 1;
}
// list[q] = a matrix of the batch, blobs[q] = where its words go / what they are compared with (differ[q] = 1: not the same)
__global__ __launch_bounds__(256) void dd_pack_kernel(DdSource v, const int *__restrict__ list, unsigned long long *const *__restrict__ blobs) {
    const int b = list[blockIdx.x];
    const long cnt = dd_count(v, b);
    unsigned long long *out = blobs[blockIdx.x];
    for (long idx = (long)blockIdx.y * 256 + threadIdx.x; idx < cnt; idx += 256l * gridDim.y) out[idx] = dd_word(v, b, idx);
}
__global__ __launch_bounds__(256) void dd_compare_kernel(DdSource v, const int *__restrict__ list, const unsigned long long *const *__restrict__ blobs,
                                                         const long *__restrict__ blob_words, int *__restrict__ differ) {
    const int b = list[blockIdx.x];
    const long cnt = dd_count(v, b);
    if (cnt != blob_words[blockIdx.x]) { if (threadIdx.x == 0) differ[blockIdx.x] = 1; return; }
    const unsigned long long *ref = blobs[blockIdx.x];
    int bad = 0;
    for (long idx = (long)blockIdx.y * 256 + threadIdx.x; idx < cnt; idx += 256l * gridDim.y) bad |= dd_word(v, b, idx) != ref[idx];
    if (bad) differ[blockIdx.x] = 1;
}
// results to every member of the classes: block i copies the eigenvalues and eigenvectors its class was given
__global__ __launch_bounds__(256) void dedupe_expand_kernel(const double *const *__restrict__ src_evals, const double *const *__restrict__ src_evecs,
                                                            const int64_t *__restrict__ eoff, const int64_t *__restrict__ xoff,
                                                            double *__restrict__ evals, double *__restrict__ evecs) {
    const int i = blockIdx.x;
    const int64_t ne = eoff[i + 1] - eoff[i], nx = xoff[i + 1] - xoff[i];
    const double *se = src_evals[i], *sx = src_evecs[i];
    if (blockIdx.y == 0)
        for (int64_t t = threadIdx.x; t < ne; t += 256) evals[eoff[i] + t] = se[t];
    for (int64_t t = blockIdx.y * 256 + threadIdx.x; t < nx; t += 256 * (int64_t)gridDim.y) evecs[xoff[i] + t] = sx[t];
}
void eig_dedupe_expand(hipStream_t s, int count, int max_n, const double *const *src_evals, const double *const *src_evecs,
                       const int64_t *eoff, const int64_t *xoff, double *evals, double *evecs) {
    if (!count) return;
    const int ny = std::max(1, std::min(64, std::min(max_n / 128, 65536 / std::max(1, count))));
    hipLaunchKernelGGL(dedupe_expand_kernel, dim3(count, ny), dim3(256), 0, s, src_evals, src_evecs, eoff, xoff, evals, evecs);
    SA_HIP_CHECK(hipGetLastError());
}

// rep[i] = the first matrix with matrix i's 128-bit hash (hashes: two words per matrix); returns the number of classes
int eig_dedupe_group(const unsigned long long *hh, int count, std::vector<int> &rep) {
    std::unordered_map<DdKey, int, DdKeyHash> first;
    first.reserve((size_t)count / 8 + 16);
    rep.resize((size_t)count);
    int nuniq = 0;
    for (int i = 0; i < count; ++i) {
        auto it = first.emplace(DdKey{hh[2 * (size_t)i], hh[2 * (size_t)i + 1]}, i);
        rep[i] = it.first->second;
        nuniq += it.second ? 1 : 0;
    }
    return nuniq;
}
static int dd_grid_y(const DdSource &src, int count, int max_n) {      // workgroups per matrix: few large matrices need several
    const long words = src.kind == 0 ? 2l * max_n * src.RW : (long)max_n * std::min(2 * max_n, 2048);
    return (int)std::max(1l, std::min(std::min(64l, words / 65536), 4096l / std::max(1, count)));
}

bool dedupe_classes(hipStream_t s, int count, const DdHashFn &hash, const DdVerifyFn &verify, DdClasses &out, std::vector<int> *rep_out) {
    out.reps.clear();
    out.rep_of.clear();
    out.rep_hash.clear();
    if (rep_out) rep_out->clear();
    if (count < 16) return false;
    profiler().begin(s);
    DBuf<unsigned long long> d_hash(2 * (size_t)count);
    d_hash.zero(s);
    hash(d_hash.p);
    SA_HIP_CHECK(hipGetLastError());
    auto hh = d_hash.to_host(s);
    std::vector<int> rep;
    const int nuniq = eig_dedupe_group(hh.data(), count, rep);
    if ((long)nuniq * 4 > (long)count * 3) { profiler().end(s, "eig_dedupe", 0.0, 0.0); return false; }
    DBuf<int> d_rep, differ((size_t)count);
    d_rep.from_host(rep, s);
    differ.zero(s);
    verify(d_rep.p, differ.p);
    SA_HIP_CHECK(hipGetLastError());
    auto hd = differ.to_host(s);
    for (int i = 0; i < count; ++i)
        if (hd[i]) rep[i] = i;      // (a collision of the hash: the item stands for itself)
    std::vector<int> pos((size_t)count, -1);
    for (int i = 0; i < count; ++i)
        if (rep[i] == i) {
            pos[i] = (int)out.reps.size();
            out.reps.push_back(i);
            out.rep_hash.push_back(hh[2 * (size_t)i]);
            out.rep_hash.push_back(hh[2 * (size_t)i + 1]);
        }
    out.rep_of.resize((size_t)count);
    for (int i = 0; i < count; ++i) out.rep_of[i] = pos[rep[i]];
    profiler().end(s, "eig_dedupe", 0.0, 0.0);
    if (rep_out) *rep_out = std::move(rep);
    return true;
}

bool eig_dedupe_find(hipStream_t s, const DdSource &src, int count, int max_n, DdClasses &out, int debug) {
    const dim3 grid(count, dd_grid_y(src, count, max_n));
    const bool found = dedupe_classes(
        s, count, [&](unsigned long long *h) { hipLaunchKernelGGL(dd_hash_kernel, grid, dim3(256), 0, s, src, (const int *)nullptr, h); },
        [&](const int *rep, int *differ) { hipLaunchKernelGGL(dd_verify_kernel, grid, dim3(256), 0, s, src, rep, differ); }, out);
    if (found && (debug & 1)) std::fprintf(stderr, "duplicate agglomerates (%s): %d distinct of %d\n", src.kind ? "bands" : "sparse rows", (int)out.reps.size(), count);
    return found;
}
// the hashes of SOME matrices of the batch (two words each, in the order of the list)
std::vector<unsigned long long> eig_dedupe_hash_list(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list) {
    if (list.empty()) return {};
    DBuf<int> d_list;
    d_list.from_host(list, s);
    DBuf<unsigned long long> hash(2 * list.size());
    hash.zero(s);
    hipLaunchKernelGGL(dd_hash_kernel, dim3((unsigned)list.size(), dd_grid_y(src, (int)list.size(), max_n)), dim3(256), 0, s, src, d_list.p, hash.p);
    SA_HIP_CHECK(hipGetLastError());
    auto hh = hash.to_host(s);
    return std::vector<unsigned long long>(hh.begin(), hh.end());
}
// the words of some matrices of the batch, kept for comparisons with matrices of later batches
void eig_dedupe_pack(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list, const std::vector<long> &words,
                     std::vector<DBuf<unsigned long long>> &blobs) {
    blobs.clear();
    blobs.resize(list.size());
    if (list.empty()) return;
    std::vector<unsigned long long *> ptrs(list.size());
    for (size_t q = 0; q < list.size(); ++q) { blobs[q].alloc((size_t)words[q]); ptrs[q] = blobs[q].p; }
    DBuf<int> d_list;
    DBuf<unsigned long long *> d_ptrs;
    d_list.from_host(list, s);
    d_ptrs.from_host(ptrs, s);
    hipLaunchKernelGGL(dd_pack_kernel, dim3((unsigned)list.size(), dd_grid_y(src, (int)list.size(), max_n)), dim3(256), 0, s, src, d_list.p, d_ptrs.p);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
}
// same[q] = matrix list[q] of the batch consists of exactly the words blobs[q]
void eig_dedupe_compare(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list,
                        const std::vector<const unsigned long long *> &blobs, const std::vector<long> &blob_words, std::vector<char> &same) {
    same.assign(list.size(), 0);
    if (list.empty()) return;
    DBuf<int> d_list, differ(list.size());
    DBuf<const unsigned long long *> d_ptrs;
    DBuf<long> d_words;
    d_list.from_host(list, s);
    d_ptrs.from_host(blobs, s);
    d_words.from_host(blob_words, s);
    differ.zero(s);
    hipLaunchKernelGGL(dd_compare_kernel, dim3((unsigned)list.size(), dd_grid_y(src, (int)list.size(), max_n)), dim3(256), 0, s, src, d_list.p, d_ptrs.p,
                       d_words.p, differ.p);
    SA_HIP_CHECK(hipGetLastError());
    auto hd = differ.to_host(s);
    for (size_t q = 0; q < list.size(); ++q) same[q] = hd[q] ? 0 : 1;
}
// word counts of some matrices (host): the half bandwidths come from the device
std::vector<long> eig_dedupe_words(hipStream_t s, const DdSource &src, const hvec<int> &h_n, const std::vector<int> &list) {
    std::vector<long> w(list.size());
    hvec<int> hb;
    if (src.kind == 1) { DBuf<int> tmp; tmp.view(const_cast<int *>(src.bws), h_n.size()); hb = tmp.to_host(s); }
    for (size_t q = 0; q < list.size(); ++q) w[q] = dd_words(src.kind, h_n[list[q]], src.kind == 0 ? 0 : hb[list[q]], src.RW);
    return w;
}
DdSource eig_dedupe_source(const EigBatch &b) {
    DdSource v{};
    v.kind = 1;
    v.ns = b.n.p; v.moff = b.moff.p; v.voff = b.voff.p; v.W = b.W.p; v.bws = b.bw.p; v.dis = b.dis.p;
    v.perm = b.has_perm ? b.perm.p : nullptr;
    v.x0c = b.has_x0c ? b.x0c.p : nullptr;
    return v;
}

std::vector<int> LevelClasses::admit(hipStream_t s, const DdSource &src, const hvec<int> &h_n, int max_n, const DdClasses &cl,
                                     std::vector<int> &solve_ids, std::vector<int> &class_of) {
    const int nl = (int)cl.reps.size();
    std::vector<int> l2g((size_t)nl, -1);
    // against the classes of the earlier chunks: same hash, then word by word against the class's first member
    std::vector<int> list, qidx, cand;
    std::vector<const unsigned long long *> blobs;
    std::vector<long> bwords;
    for (int q = 0; q < nl; ++q) {
        auto it = by_hash.find(cl.key(q));
        if (it == by_hash.end()) continue;
        for (int id : it->second)
            if (entries[id].kind == src.kind) {
                list.push_back(cl.reps[q]); qidx.push_back(q); cand.push_back(id);
                blobs.push_back(entries[id].blob.p); bwords.push_back(entries[id].words);
            }
    }
    std::vector<char> same;
    eig_dedupe_compare(s, src, max_n, list, blobs, bwords, same);
    for (size_t t = 0; t < list.size(); ++t)
        if (same[t] && l2g[qidx[t]] < 0) l2g[qidx[t]] = cand[t];
    // the new classes: their words are kept, their first members are what this chunk solves
    std::vector<int> newq, newlist;
    for (int q = 0; q < nl; ++q)
        if (l2g[q] < 0) { newq.push_back(q); newlist.push_back(cl.reps[q]); }
    const std::vector<long> nwords = eig_dedupe_words(s, src, h_n, newlist);
    std::vector<DBuf<unsigned long long>> nblobs;
    eig_dedupe_pack(s, src, max_n, newlist, nwords, nblobs);
    // (local classes found on the INPUTS of the assembly can share their assembled matrix -- agglomerates that differ
    // in the flags of their surface dofs only: candidates with the hash of an earlier candidate are compared with it)
    std::vector<int> alias(newq.size(), -1);
    {
        std::unordered_map<DdKey, int, DdKeyHash> firstc;
        std::vector<int> clist, cwho, cfirst;
        std::vector<const unsigned long long *> cblobs;
        std::vector<long> cwords;
        for (size_t t = 0; t < newq.size(); ++t) {
            auto it = firstc.emplace(cl.key(newq[t]), (int)t);
            if (it.second) continue;
            clist.push_back(newlist[t]); cwho.push_back((int)t); cfirst.push_back(it.first->second);
            cblobs.push_back(nblobs[it.first->second].p); cwords.push_back(nwords[it.first->second]);
        }
        std::vector<char> csame;
        eig_dedupe_compare(s, src, max_n, clist, cblobs, cwords, csame);
        for (size_t u = 0; u < clist.size(); ++u)
            if (csame[u]) alias[cwho[u]] = cfirst[u];
    }
    std::vector<int> solve_list, id_of(newq.size(), -1);
    solve_ids.clear();
    for (size_t t = 0; t < newq.size(); ++t) {
        if (alias[t] >= 0) { id_of[t] = id_of[alias[t]]; l2g[newq[t]] = id_of[t]; continue; }
        solve_list.push_back(newlist[t]);
        const int id = (int)entries.size();
        id_of[t] = id;
        entries.emplace_back();
        Entry &e = entries.back();
        e.n = h_n[newlist[t]];
        e.kind = src.kind;
        e.words = nwords[t];
        e.blob = std::move(nblobs[t]);
        by_hash[cl.key(newq[t])].push_back(id);
        l2g[newq[t]] = id;
        solve_ids.push_back(id);
    }
    class_of.resize(cl.rep_of.size());
    for (size_t i = 0; i < cl.rep_of.size(); ++i) class_of[i] = l2g[cl.rep_of[i]];
    return solve_list;
}

}  // namespace saamge_amd
