// Classes of bitwise identical inputs (dedupe.hip, "Duplicate agglomerate matrices"): the hash pieces and the host sequence every
// stage of the setup shares, the words of an agglomerate matrix (DdSource), the registry of a level's classes (LevelClasses).
#pragma once
#include "common.h"

#include <functional>
#include <unordered_map>

namespace saamge_amd {

struct EigBatch;

// DdSource: where the words of the matrices of a batch are (kind 1: the assembled matrices; kind 0: the sparse rows the
// fused fine-level assembly builds them from).
struct DdSource {
    int kind = 1;
    const int *ns = nullptr;
    const int64_t *moff = nullptr, *voff = nullptr;
    const double *W = nullptr;
    const int *bws = nullptr;
    const double *dis = nullptr;
    const short *perm = nullptr;      // or null
    const double *x0c = nullptr;      // or null
    const double *rvals = nullptr;    // kind 0
    const short *rcols = nullptr;
    int RW = 0;
};
struct DdKey { unsigned long long a, b; bool operator==(const DdKey &o) const { return a == o.a && b == o.b; } };
struct DdKeyHash { size_t operator()(const DdKey &k) const { return (size_t)(k.a ^ (k.b * 0x9E3779B97F4A7C15ull)); } };
// classes of a batch: reps = the first matrix of every class of bitwise identical matrices (confirmed word by word),
// rep_of[i] = the position in reps of matrix i's class, rep_hash = the 128-bit hash of every class (two words each)
struct DdClasses {
    std::vector<int> reps, rep_of;
    std::vector<unsigned long long> rep_hash;
    DdKey key(int q) const { return DdKey{rep_hash[2 * (size_t)q], rep_hash[2 * (size_t)q + 1]}; }
};
// The words a matrix consists of (dd_word, dedupe.hip): how many.  bw is read for kind 1 only.
__host__ __device__ inline long dd_words(int kind, long n, long bw, int RW) {
    if (kind == 0) return 2 * n * RW + n + 1;
    bw = bw < n - 1 ? bw : n - 1;
    return n * (2 * bw + 1) + 3 * n + 2;
}

// The host sequence of a class search over `count` items.  hash(out) launches the stage's hash kernel (two words per item, out
// zeroed), verify(rep, differ) the kernel that compares every item with the first of its hash (differ[i] = 1: item i stands for
// itself).  false: fewer than 16 items or fewer than a quarter duplicates.  rep (optional): the first member of every item's class.
using DdHashFn = std::function<void(unsigned long long *out)>;
using DdVerifyFn = std::function<void(const int *rep, int *differ)>;
bool dedupe_classes(hipStream_t s, int count, const DdHashFn &hash, const DdVerifyFn &verify, DdClasses &out, std::vector<int> *rep = nullptr);

DdSource eig_dedupe_source(const EigBatch &b);
bool eig_dedupe_find(hipStream_t s, const DdSource &src, int count, int max_n, DdClasses &out, int debug);      // false: fewer than a quarter duplicates
int eig_dedupe_group(const unsigned long long *hh, int count, std::vector<int> &rep);      // rep[i] = first matrix with i's hash; returns the classes
std::vector<unsigned long long> eig_dedupe_hash_list(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list);
std::vector<long> eig_dedupe_words(hipStream_t s, const DdSource &src, const hvec<int> &h_n, const std::vector<int> &list);
void eig_dedupe_pack(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list, const std::vector<long> &words,
                     std::vector<DBuf<unsigned long long>> &blobs);
void eig_dedupe_compare(hipStream_t s, const DdSource &src, int max_n, const std::vector<int> &list,
                        const std::vector<const unsigned long long *> &blobs, const std::vector<long> &blob_words, std::vector<char> &same);
// results to every member of the classes
void eig_dedupe_expand(hipStream_t s, int count, int max_n, const double *const *src_evals, const double *const *src_evecs,
                       const int64_t *eoff, const int64_t *xoff, double *evals, double *evecs);

// Classes of bitwise identical agglomerates of a level (a rank's part of it), carried from chunk to chunk: the first member
// met is solved, in the chunk it sits in; every later member -- of that chunk or a later one -- receives a copy.  A class
// keeps the words it consists of (the first member's: sparse rows or band, DdSource), against which the candidates of later
// chunks are compared word by word, and where its eigenpairs are.  Everything here allocates on the calling thread.
struct LevelClasses {
    struct Entry {
        int n = 0, m = 0, kind = 0;
        bool bad = false;           // the few-eigenpairs path gave up on it: every member is redone by the dense path
        long words = 0;
        DBuf<unsigned long long> blob;
        const double *evals = nullptr, *evecs = nullptr;
    };
    // The classes of one chunk (cl, found on src) against those of earlier chunks; new ones are registered with their words.
    // Returns the batch-local indices to solve (first members of the new classes), their ids, and per matrix its class id.
    std::vector<int> admit(hipStream_t s, const DdSource &src, const hvec<int> &h_n, int max_n, const DdClasses &cl,
                           std::vector<int> &solve_ids, std::vector<int> &class_of);
    void set_result(int id, int m, bool bad, const double *evals, const double *evecs) { Entry &e = entries[id]; e.m = m; e.bad = bad; e.evals = evals; e.evecs = evecs; }
    void mark_bad(int id) { entries[id].bad = true; }
    const Entry &operator[](int id) const { return entries[id]; }
    bool empty() const { return entries.empty(); }

private:
    std::vector<Entry> entries;
    std::unordered_map<DdKey, std::vector<int>, DdKeyHash> by_hash;
};

// ---- device side: what every stage's hash kernel is made of ----
__device__ inline unsigned long long dd_mix(unsigned long long x) {      // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// Two sums over the mixed (word, position) pairs of an item: independent of the order the words are visited in.
struct DdHash {
    unsigned long long h1 = 0, h2 = 0;
    __device__ void add(unsigned long long w, unsigned long long pos) {
        const unsigned long long k = dd_mix(w + 0x9E3779B97F4A7C15ull * (pos + 1));
        h1 += k;
        h2 += (k >> 32) * (k & 0xffffffffull);      // (second sum: the product of the halves of the mixed word; a full second mix was half of the kernel)
    }
    __device__ void wave_sum() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { h1 += __shfl_xor(h1, o, 64); h2 += __shfl_xor(h2, o, 64); }
    }
    // workgroups of 256 threads: their sums added into out[2 b], out[2 b + 1] (several workgroups per item, out zeroed) or stored
    template <bool ATOMIC>
    __device__ void block_finish(unsigned long long *__restrict__ out, size_t b) {
        __shared__ unsigned long long red[2][4];
        const int tid = threadIdx.x;
        wave_sum();
        if ((tid & 63) == 0) { red[0][tid >> 6] = h1; red[1][tid >> 6] = h2; }
        __syncthreads();
        if (tid == 0) {
            const unsigned long long s1 = red[0][0] + red[0][1] + red[0][2] + red[0][3], s2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
            if (ATOMIC) { atomicAdd(out + 2 * b, s1); atomicAdd(out + 2 * b + 1, s2); }
            else { out[2 * b] = s1; out[2 * b + 1] = s2; }
        }
    }
};

}  // namespace saamge_amd
