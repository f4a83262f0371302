// Agglomerate partitions on the device: element graph from elem_to_dof, seeded level-synchronous growth, recentring,
// size repair, renumbering and the quotient graph of the next level.  saamge_amd/partition_model.py defines every step;
// this file restates it.  Every decision is a minimum / maximum / count over integers (atomicMin / atomicMax on packed
// keys, atomicAdd on counters), so the output does not depend on the order in which threads run.
//
// Sweeps over the CSR use PT_LPR lanes per row: the lanes of a group read consecutive entries of the row, reduce by
// shuffles, and lane 0 writes.  Growth is the pull form with two label buffers (no atomics on labels); the ball sweeps of the
// spaced seeding are the same form with two key / two flag buffers.  Balanced growth (`growth = 1`) sweeps once per round for
// the claims, orders the compacted claimants by two stable radix sorts and labels the first quota[p] of every part.
//
// What the phases share is written once, ahead of them.  On the device: row_lane / row_entries (which lane of which row a
// thread is, and the walk over its entries), group_reduce (the shuffles, over a row's lanes or a wavefront) and pt_run_start
// (the rank within a sorted run, for the quotas).  On the host: GraphView with sweep (the row launch; the flat one is devtab.h's launch_flat), ball_min /
// ball_flag (the ball sweeps by run-time first / last); the radix sorts of a phase and their temporary storage are devsort.h's
// PairSorter.  The counts of a call go back to the caller (PartitionStats, RefineStats); nothing here remembers a call.
#include "partition.h"
#include "devsort.h"

#include <algorithm>
#include <climits>
#include <type_traits>

namespace saamge_amd {

namespace {

typedef unsigned long long u64;
constexpr int PT_LPR = 8;          // lanes per row of the CSR sweeps
constexpr int PT_WAVE = 64;
constexpr u64 PT_NONE = ~0ull;

inline dim3 grid_rows(long n) { return dim3((unsigned)((n * PT_LPR + 255) / 256)); }

__device__ inline unsigned pt_prio(unsigned i, unsigned seed) {
    unsigned x = i + seed * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// ---- the row sweep --------------------------------------------------------------------------------------------------
// Thread t of a grid_rows(n) launch is lane t % PT_LPR of row t / PT_LPR.  The lanes of a row are adjacent lanes of one
// wavefront, and a kernel keeps all of them up to its group_reduce, whether the row is valid or not.
struct RowLane {
    long v;
    int lane;
    bool valid;   // v < n
};
__device__ inline RowLane row_lane(int n) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    return {t / PT_LPR, (int)(t % PT_LPR), t / PT_LPR < n};
}
// f(k) for the entries k of a row that fall to this lane.  The offsets are read here and nowhere else, so a row whose walk
// is skipped reads none.
template <class F>
__device__ inline void row_entries(roff_t b, roff_t e, int lane, F &&f) {
    for (roff_t k = b + lane; k < e; k += PT_LPR) f(k);
}
template <class F>
__device__ inline void row_entries(const roff_t *__restrict__ xadj, long v, int lane, F &&f) {
    row_entries(xadj[v], xadj[v + 1], lane, f);
}
__device__ inline u64 shfl_xor_u64(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}
// op over the WIDTH adjacent lanes that hold this one (PT_LPR: a row, PT_WAVE: the wavefront); every lane gets the result
struct OpMin { template <class T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct OpMax { template <class T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
struct OpOr { template <class T> __device__ T operator()(T a, T b) const { return a | b; } };
struct OpSum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
template <int WIDTH, class T, class Op>
__device__ inline T group_reduce(T v, Op op) {
    for (int m = WIDTH / 2; m; m >>= 1) {
        if constexpr (sizeof(T) == 8) v = op(v, (T)shfl_xor_u64((u64)v, m));
        else v = op(v, __shfl_xor(v, m));
    }
    return v;
}
// the start of the run of lab[j] in the ascending lab: j minus it is the rank of j among the entries of its label
__device__ inline int pt_run_start(const int *lab, int j) {
    const int p = lab[j];
    int lo = 0, hi = j;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (lab[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- growth ---------------------------------------------------------------------------------------------------------
// counters[0] += nodes labelled in this round, counters[1] += nodes still unlabelled after it
__global__ __launch_bounds__(256) void pt_grow_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                      const int *__restrict__ cur, const int *__restrict__ dom,
                                                      int *__restrict__ next, int *__restrict__ counters) {
    const RowLane r = row_lane(n);
    const int mine = r.valid ? cur[r.v] : 0;
    int best = INT_MAX;
    if (r.valid && mine < 0) {
        const int dv = dom ? dom[r.v] : 0;
        row_entries(xadj, r.v, r.lane, [&](roff_t k) {
            const int u = adj[k], lu = cur[u];
            if (lu >= 0 && lu < best && (!dom || dom[u] == dv)) best = lu;
        });
    }
    best = group_reduce<PT_LPR>(best, OpMin());
    if (r.valid && r.lane == 0) {
        if (mine >= 0) next[r.v] = mine;
        else if (best != INT_MAX) { next[r.v] = best; atomicAdd(&counters[0], 1); }
        else { next[r.v] = -1; atomicAdd(&counters[1], 1); }
    }
}
// lowest (priority, id) among the unlabelled nodes
__global__ __launch_bounds__(256) void pt_min_unlabelled_kernel(int n, const int *__restrict__ label, unsigned seed,
                                                                u64 *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    u64 key = PT_NONE;
    if (i < n && label[i] < 0) key = ((u64)pt_prio((unsigned)i, seed) << 32) | (unsigned)i;
    key = group_reduce<PT_WAVE>(key, OpMin());
    if (threadIdx.x % PT_WAVE == 0 && key != PT_NONE) atomicMin(out, key);
}
__global__ void pt_stall_seed_kernel(const u64 *__restrict__ key, int newlabel, int *__restrict__ label,
                                     int *__restrict__ isseed) {
    const unsigned i = (unsigned)(*key & 0xFFFFFFFFull);
    label[i] = newlabel;
    isseed[i] = 1;
}


// ---- balanced growth (partition_model.py, "balanced growth") --------------------------------------------------------------
constexpr int PT_HITS_MAX = 65535;
// sizes of the parts; unlabelled nodes (during growth) are not counted
__global__ __launch_bounds__(256) void pt_count_kernel(int n, const int *__restrict__ label, int *__restrict__ sizes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && label[i] >= 0) atomicAdd(&sizes[label[i]], 1);
}
// The claim sweep.  An unlabelled node with a neighbour in an open part (sizes < cap) claims the smallest such label c; a
// second pass over the row counts the neighbours labelled c.  Claimants are compacted in any order (the sorts that follow
// order them by keys that never tie): keys[j] = (HITS_MAX - hits, priority), ids[j] = the node, claim[node] = c.
// counters[0] += claimants, counters[1] += unlabelled nodes (claimants included).
__global__ __launch_bounds__(256) void pt_claim_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                       const int *__restrict__ label, const int *__restrict__ sizes, int cap,
                                                       unsigned seed, int *__restrict__ claim, u64 *__restrict__ keys,
                                                       int *__restrict__ ids, int *__restrict__ counters) {
    const RowLane r = row_lane(n);
    const bool open_row = r.valid && label[r.v] < 0;
    int best = INT_MAX;
    if (open_row)
        row_entries(xadj, r.v, r.lane, [&](roff_t k) {
            const int lu = label[adj[k]];
            if (lu >= 0 && lu < best && sizes[lu] < cap) best = lu;
        });
    best = group_reduce<PT_LPR>(best, OpMin());
    int hits = 0;
    if (open_row && best != INT_MAX) row_entries(xadj, r.v, r.lane, [&](roff_t k) { hits += label[adj[k]] == best; });
    hits = group_reduce<PT_LPR>(hits, OpSum());
    if (open_row && r.lane == 0) {
        atomicAdd(&counters[1], 1);
        if (best != INT_MAX) {
            const int j = atomicAdd(&counters[0], 1);
            keys[j] = ((u64)(unsigned)(PT_HITS_MAX - min(hits, PT_HITS_MAX)) << 32) | pt_prio((unsigned)r.v, seed);
            ids[j] = (int)r.v;
            claim[r.v] = best;
        }
    }
}
__global__ __launch_bounds__(256) void pt_claim_gather_kernel(int m, const int *__restrict__ ids, const int *__restrict__ claim,
                                                              int *__restrict__ lab) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < m) lab[j] = claim[ids[j]];
}
// lab ascending, the claimants of one part in their order: the rank in the own run against the quota.  A node stands once
// in ids and the sweep that read the labels is over, so the labels are written in place.
__global__ __launch_bounds__(256) void pt_claim_apply_kernel(int m, const int *__restrict__ lab, const int *__restrict__ ids,
                                                             const int *__restrict__ sizes, int cap, int *__restrict__ label) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int p = lab[j];
    if ((int)j - pt_run_start(lab, (int)j) < cap - sizes[p]) label[ids[j]] = p;
}
__global__ __launch_bounds__(256) void pt_count_open_kernel(int nlabels, const int *__restrict__ sizes, int cap,
                                                            int *__restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < nlabels && sizes[p] < cap) atomicAdd(out, 1);
}

// ---- seeding --------------------------------------------------------------------------------------------------------
// k[p] = seeds of an oversized part (0: not flagged), km1[p] = the labels it needs beyond its own; info[0] += flagged parts
__global__ __launch_bounds__(256) void pt_over_kernel(int nlabels, const int *__restrict__ sizes, int max_size, int epa,
                                                      int *__restrict__ k, int *__restrict__ km1, int *__restrict__ info) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nlabels) return;
    const int sz = sizes[p];
    int kp = 0;
    if (sz > max_size) { kp = max(2, (sz + epa - 1) / epa); atomicAdd(&info[0], 1); }
    k[p] = kp;
    km1[p] = kp ? kp - 1 : 0;
}
__global__ __launch_bounds__(256) void pt_sort_keys_kernel(int n, const int *__restrict__ label, unsigned seed,
                                                           u64 *__restrict__ keys, int *__restrict__ ids) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((u64)(unsigned)label[i] << 32) | pt_prio((unsigned)i, seed);
    ids[i] = (int)i;
}
__global__ __launch_bounds__(256) void pt_reseed_kernel(int n, const u64 *__restrict__ keys, const int *__restrict__ ids,
                                                        const int *__restrict__ start, const int *__restrict__ k,
                                                        const int *__restrict__ off, int nlabels, int *__restrict__ label,
                                                        int *__restrict__ isseed) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int p = (int)(keys[j] >> 32), node = ids[j], kp = k[p];
    if (!kp) return;
    const int r = (int)j - start[p];
    if (r < kp) { label[node] = r == 0 ? p : nlabels + off[p] + r - 1; isseed[node] = 1; }
    else { label[node] = -1; isseed[node] = 0; }
}

// ---- spaced seeding: greedy distance-r independent sets by rounds (partition_model.py, "fixed point") ----------------------
constexpr int PT_UNDECIDED = 0, PT_SEED = 1, PT_OUT = 2, PT_EXT = 3;  // PT_EXT: a seed of the top-up's extension
constexpr int PT_RADIUS_MAX = 32;

// One hop of the min-priority ball sweep over closed neighbourhoods.  Keys are priorities in 64 bits, so that PT_NONE lies
// outside them.  FIRST: the source is the state array, an undecided node offers its priority.  LAST: the minimum is not
// stored; an undecided node that holds its own priority is flagged as a new seed.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void pt_ball_min_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                          const int *__restrict__ state, unsigned seed,
                                                          const u64 *__restrict__ src, u64 *__restrict__ dst,
                                                          int *__restrict__ newseed) {
    const RowLane r = row_lane(n);
    const auto offer = [&](int u) { return FIRST ? (state[u] == PT_UNDECIDED ? (u64)pt_prio((unsigned)u, seed) : PT_NONE) : src[u]; };
    u64 best = PT_NONE;
    if (r.valid) {
        if (r.lane == 0) best = offer((int)r.v);
        row_entries(xadj, r.v, r.lane, [&](roff_t k) {
            const u64 key = offer(adj[k]);
            best = key < best ? key : best;
        });
    }
    best = group_reduce<PT_LPR>(best, OpMin());
    if (r.valid && r.lane == 0) {
        if (LAST) newseed[r.v] = state[r.v] == PT_UNDECIDED && best == (u64)pt_prio((unsigned)r.v, seed);
        else dst[r.v] = best;
    }
}
// One hop of the flag's ball sweep.  LAST: the flag is not stored; an undecided node becomes `seedval` when it is a new seed
// and out when the flag reached it.  counters[0] += new seeds, counters[1] += nodes still undecided.
template <bool LAST>
__global__ __launch_bounds__(256) void pt_ball_flag_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                           const int *__restrict__ src, int *__restrict__ dst,
                                                           const int *__restrict__ newseed, int seedval,
                                                           int *__restrict__ state, int *__restrict__ counters) {
    const RowLane r = row_lane(n);
    int f = 0;
    if (r.valid) {
        if (r.lane == 0) f = src[r.v];
        row_entries(xadj, r.v, r.lane, [&](roff_t k) { f |= src[adj[k]]; });
    }
    f = group_reduce<PT_LPR>(f, OpOr());
    if (r.valid && r.lane == 0) {
        if (!LAST) dst[r.v] = f;
        else if (state[r.v] == PT_UNDECIDED) {
            if (newseed[r.v]) { state[r.v] = seedval; atomicAdd(&counters[0], 1); }
            else if (f) state[r.v] = PT_OUT;
            else atomicAdd(&counters[1], 1);
        }
    }
}
// before the extension: the first-stage seeds stay and are flagged, every other node becomes `other`
__global__ __launch_bounds__(256) void pt_ext_init_kernel(int n, int other, int *__restrict__ state, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = state[i] == PT_SEED;
    flag[i] = s;
    if (!s) state[i] = other;
}
// (class, priority): first-stage seeds, then the extension, then the rest
__global__ __launch_bounds__(256) void pt_spaced_keys_kernel(int n, const int *__restrict__ state, unsigned seed,
                                                             u64 *__restrict__ keys, int *__restrict__ ids) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int st = state[i];
    keys[i] = ((u64)(st == PT_SEED ? 0u : st == PT_EXT ? 1u : 2u) << 32) | pt_prio((unsigned)i, seed);
    ids[i] = (int)i;
}
// Sorted keys: [0, ns) the first-stage seeds, [ns, nsel) the members of the extension that top them up, each by priority.
// The label of a seed is its rank by priority among all of them: its rank in its own run plus, by bisection, the number of
// lower priorities in the other run.
__global__ __launch_bounds__(256) void pt_spaced_label_kernel(int n, const u64 *__restrict__ keys, const int *__restrict__ ids,
                                                              int ns, int nsel, int *__restrict__ label, int *__restrict__ isseed) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int node = ids[j];
    if (j >= nsel) { label[node] = -1; isseed[node] = 0; return; }
    const unsigned prio = (unsigned)(keys[j] & 0xFFFFFFFFull);
    int lo = j < ns ? ns : 0, hi = j < ns ? nsel : ns;
    const int base = lo;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((unsigned)(keys[mid] & 0xFFFFFFFFull) < prio) lo = mid + 1;
        else hi = mid;
    }
    label[node] = (int)(j < ns ? j : j - ns) + (lo - base);
    isseed[node] = 1;
}

// ---- recentring -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_boundary_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                          const int *__restrict__ label, int *__restrict__ depth) {
    const RowLane r = row_lane(n);
    int b = 0;
    if (r.valid) {
        const int lv = label[r.v];
        row_entries(xadj, r.v, r.lane, [&](roff_t k) { b |= label[adj[k]] != lv; });
    }
    b = group_reduce<PT_LPR>(b, OpOr());
    if (r.valid && r.lane == 0) depth[r.v] = b ? 0 : -1;
}
// In place: a node without depth takes d when a neighbour of its part has d - 1.  A depth written in this launch is d, never
// d - 1, so what a concurrent reader sees of it does not change the outcome.
__global__ __launch_bounds__(256) void pt_depth_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                       const int *__restrict__ label, int d, int *depth,
                                                       int *__restrict__ counters) {
    const RowLane r = row_lane(n);
    int hit = 0;
    if (r.valid && depth[r.v] < 0) {
        const int lv = label[r.v];
        row_entries(xadj, r.v, r.lane, [&](roff_t k) {
            const int u = adj[k];
            hit |= label[u] == lv && depth[u] == d - 1;
        });
    }
    hit = group_reduce<PT_LPR>(hit, OpOr());
    if (r.valid && r.lane == 0 && hit) { depth[r.v] = d; atomicAdd(&counters[0], 1); }
}
__device__ inline u64 centre_key(int depth, unsigned prio) { return ((u64)(unsigned)(depth + 1) << 32) | (0xFFFFFFFFu - prio); }
__global__ __launch_bounds__(256) void pt_centre_max_kernel(int n, const int *__restrict__ label, const int *__restrict__ depth,
                                                            const int *__restrict__ isseed, unsigned seed,
                                                            u64 *__restrict__ best) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int d = depth[i];
    if (d >= 0 || isseed[i]) atomicMax(&best[label[i]], centre_key(d, pt_prio((unsigned)i, seed)));
}
__global__ __launch_bounds__(256) void pt_centre_pick_kernel(int n, int *__restrict__ label, const int *__restrict__ depth,
                                                             int *__restrict__ isseed, unsigned seed,
                                                             const u64 *__restrict__ best) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int d = depth[i];
    const bool pick = (d >= 0 || isseed[i]) && centre_key(d, pt_prio((unsigned)i, seed)) == best[label[i]];
    isseed[i] = pick ? 1 : 0;
    if (!pick) label[i] = -1;
}

// ---- merging of small parts -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_propose_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                         const int *__restrict__ label, const int *__restrict__ sizes,
                                                         int min_size, int max_size, u64 *__restrict__ prop) {
    const RowLane r = row_lane(n);
    u64 best = PT_NONE;
    int lp = 0;
    if (r.valid) {
        lp = label[r.v];
        const int sp = sizes[lp];
        if (sp < min_size)
            row_entries(xadj, r.v, r.lane, [&](roff_t k) {
                const int lq = label[adj[k]];
                if (lq == lp) return;
                const int sq = sizes[lq];
                if (max_size > 0 && sp + sq > max_size) return;
                const u64 key = ((u64)(unsigned)sq << 32) | (unsigned)lq;
                best = key < best ? key : best;
            });
    }
    best = group_reduce<PT_LPR>(best, OpMin());
    if (r.valid && r.lane == 0 && best != PT_NONE) atomicMin(&prop[lp], best);
}
__global__ __launch_bounds__(256) void pt_win_kernel(int nlabels, const u64 *__restrict__ prop, const int *__restrict__ sizes,
                                                     u64 *__restrict__ win) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nlabels || prop[p] == PT_NONE) return;
    atomicMin(&win[(unsigned)(prop[p] & 0xFFFFFFFFull)], ((u64)(unsigned)sizes[p] << 32) | (unsigned)p);
}
__device__ inline bool pt_stationary(const u64 *prop, int q) {
    if (prop[q] == PT_NONE) return true;
    const int r = (int)(prop[q] & 0xFFFFFFFFull);
    return prop[r] != PT_NONE && (int)(prop[r] & 0xFFFFFFFFull) == q && q < r;
}
__global__ __launch_bounds__(256) void pt_decide_kernel(int nlabels, const u64 *__restrict__ prop, const u64 *__restrict__ win,
                                                        int *__restrict__ target, int *__restrict__ info) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nlabels) return;
    int t = (int)p;
    if (prop[p] != PT_NONE && !pt_stationary(prop, (int)p)) {
        const int q = (int)(prop[p] & 0xFFFFFFFFull);
        if (pt_stationary(prop, q) && (int)(win[q] & 0xFFFFFFFFull) == (int)p) { t = q; atomicAdd(&info[0], 1); }
    }
    target[p] = t;
}
__global__ __launch_bounds__(256) void pt_relabel_kernel(int n, const int *__restrict__ target, int *__restrict__ label) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = target[label[i]];
}

// ---- renumbering ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_minid_kernel(int n, const int *__restrict__ label, int *__restrict__ minid) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicMin(&minid[label[i]], (int)i);
}
__global__ __launch_bounds__(256) void pt_first_kernel(int n, const int *__restrict__ label, const int *__restrict__ minid,
                                                       int *__restrict__ first) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) first[i] = minid[label[i]] == (int)i;
}
__global__ __launch_bounds__(256) void pt_newnum_kernel(int n, const int *__restrict__ label, const int *__restrict__ first,
                                                        const int *__restrict__ rank, int *__restrict__ newnum) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && first[i]) newnum[label[i]] = rank[i];
}
__global__ __launch_bounds__(256) void pt_apply_kernel(int n, const int *__restrict__ label, const int *__restrict__ newnum,
                                                       int *__restrict__ part) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) part[i] = newnum[label[i]];
}

// ---- boundary refinement (partition_model.py, "refine") ---------------------------------------------------------------------
constexpr int PT_REFINE_DEG_MAX = 1024, PT_REFINE_LOCAL_MAX = 64, PT_GAIN_MAX = 65535;

// The counts.  One sweep gives own(v); a row with a foreign neighbour that can still be a candidate (own >= 1, its part above
// the floor, at most PT_REFINE_DEG_MAX entries) is swept again, now from the cache: every foreign entry counts the entries of
// its label, and the maximum of (count, -label) is the target.  Rows with gain > 0 whose target has room are compacted in any
// order (nothing that follows depends on it): cand[j] = v, target[v], gain[v].  counters[0] += such rows.
__global__ __launch_bounds__(256) void pt_refine_count_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                              const int *__restrict__ label, const int *__restrict__ sizes,
                                                              int max_size, int floor_size, int *__restrict__ target,
                                                              int *__restrict__ gain, int *__restrict__ cand,
                                                              int *__restrict__ counters) {
    const RowLane r = row_lane(n);
    const roff_t b = r.valid ? xadj[r.v] : 0, e = r.valid ? xadj[r.v + 1] : 0;   // (the degree enters below: read once)
    const int p = r.valid ? label[r.v] : 0;
    int own = 0, foreign = 0;
    row_entries(b, e, r.lane, [&](roff_t k) {
        const int u = adj[k];
        if (u == (int)r.v) return;
        const int lu = label[u];
        own += lu == p;
        foreign |= lu != p;
    });
    own = group_reduce<PT_LPR>(own, OpSum());
    foreign = group_reduce<PT_LPR>(foreign, OpOr());
    const bool second = r.valid && foreign && own >= 1 && e - b <= PT_REFINE_DEG_MAX && sizes[p] > floor_size;
    u64 best = 0;
    if (second)
        row_entries(b, e, r.lane, [&](roff_t k) {
            const int q = label[adj[k]];
            if (q == p) return;      // (the entry v itself has the label p)
            int c = 0;
            for (roff_t j = b; j < e; ++j) c += label[adj[j]] == q;
            const u64 key = ((u64)(unsigned)c << 32) | (0xFFFFFFFFu - (unsigned)q);
            best = key > best ? key : best;
        });
    best = group_reduce<PT_LPR>(best, OpMax());
    if (second && r.lane == 0) {
        const int q = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
        const int g = (int)(best >> 32) - own;
        if (g > 0 && (max_size == 0 || sizes[q] < max_size)) {
            const int j = atomicAdd(&counters[0], 1);
            cand[j] = (int)r.v;
            target[r.v] = q;
            gain[r.v] = g;
        }
    }
}
// The free check, one wavefront per compacted row v of part p.  N, the neighbours of v labelled p, is gathered into LDS (at
// most 64, else v is not free) and ordered; lane i owns member i and builds the 64-bit mask of the members it is linked to:
// those among its neighbours of part p, and those among the neighbours of such a neighbour x != v, found by bisection.  The
// closure from member 0 is a repeated OR over the wavefront until it is stable; it is tried on the adjacent members alone
// before the neighbours' neighbours are walked.  A free row gets its key; counters[1] += free
// rows.  The loop bounds are the same for the four wavefronts of a block, so the barriers are met by all of them.
__global__ __launch_bounds__(256) void pt_refine_free_kernel(const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                             const int *__restrict__ label, const int *__restrict__ cand,
                                                             const int *__restrict__ gain, unsigned seed,
                                                             u64 *__restrict__ key, int *__restrict__ counters) {
    __shared__ int raw[256 / PT_WAVE][PT_REFINE_LOCAL_MAX], mem[256 / PT_WAVE][PT_REFINE_LOCAL_MAX];
    const int w = threadIdx.x / PT_WAVE, lane = threadIdx.x % PT_WAVE;
    const int m = counters[0];
    for (long base = (long)blockIdx.x * (256 / PT_WAVE); base < m; base += (long)gridDim.x * (256 / PT_WAVE)) {
        const bool active = base + w < m;
        const int v = active ? cand[base + w] : 0;
        const int p = active ? label[v] : 0;
        const roff_t b = active ? xadj[v] : 0, e = active ? xadj[v + 1] : 0;
        int cnt = 0;
        for (roff_t k0 = b; k0 < e; k0 += PT_WAVE) {
            const roff_t k = k0 + lane;
            int u = -1;
            bool in = false;
            if (k < e) { u = adj[k]; in = u != v && label[u] == p; }
            const u64 bal = __ballot(in);
            const int idx = cnt + __popcll(bal & ((1ull << lane) - 1ull));
            if (in && idx < PT_REFINE_LOCAL_MAX) raw[w][idx] = u;
            cnt += __popcll(bal);
        }
        const bool local = cnt >= 2 && cnt <= PT_REFINE_LOCAL_MAX;
        __syncthreads();
        if (local && lane < cnt) {   // rank sort: rows of the library's graphs ascend already, a caller's need not
            const int mine = raw[w][lane];
            int r = 0;
            for (int j = 0; j < cnt; ++j) { const int o = raw[w][j]; r += o < mine || (o == mine && j < lane); }
            mem[w][r] = mine;
        }
        __syncthreads();
        u64 mask = 0;
        const int *N = mem[w];
        const auto find = [&](int y) {
            int lo = 0, hi = cnt;
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (N[mid] < y) lo = mid + 1;
                else hi = mid;
            }
            if (lo < cnt && N[lo] == y) mask |= 1ull << lo;
        };
        // the links of member `lane`: itself, the members among its neighbours of part p and, with TWO_HOP, those among the
        // neighbours of such a neighbour x != v
        const auto links = [&](auto two_hop) {
            constexpr bool TWO_HOP = decltype(two_hop)::value;
            const int a = N[lane];
            mask |= 1ull << lane;
            if (lane > 0 && N[lane - 1] == a) mask |= 1ull << (lane - 1);       // an entry listed twice is one member
            if (lane + 1 < cnt && N[lane + 1] == a) mask |= 1ull << (lane + 1);
            for (roff_t k = xadj[a], ke = xadj[a + 1]; k < ke; ++k) {
                const int x = adj[k];
                if (x == v || label[x] != p) continue;
                find(x);
                if constexpr (TWO_HOP)
                    for (roff_t j = xadj[x], je = xadj[x + 1]; j < je; ++j) find(adj[j]);
            }
        };
        // the closure from member 0: a repeated OR over the wavefront until it is stable (every lane takes part)
        const auto connected = [&]() {
            const u64 all = cnt == 64 ? ~0ull : (1ull << cnt) - 1ull;
            u64 reach = 1ull;
            for (;;) {
                const u64 nr = group_reduce<PT_WAVE>(((reach >> lane) & 1ull) ? mask : 0ull, OpOr()) | reach;
                if (nr == reach) break;
                reach = nr;
            }
            return reach == all;
        };
        bool isfree = cnt == 1;
        if (local) {     // (uniform in the wavefront)
            // the adjacent members first: where the graph has triangles they mostly connect N already, and the walk over the
            // neighbours' neighbours, the long part, is only for the rows they leave open
            if (lane < cnt) links(std::false_type());
            isfree = connected();
            if (!isfree) {
                if (lane < cnt) links(std::true_type());
                isfree = connected();
            }
        }
        if (active && isfree && lane == 0) {
            key[v] = ((u64)(unsigned)(PT_GAIN_MAX - min(gain[v], PT_GAIN_MAX)) << 32) | pt_prio((unsigned)v, seed);
            atomicAdd(&counters[1], 1);
        }
        __syncthreads();
    }
}
// ball = the minimum key within 2 hops: a candidate that holds it wins.  Winners are compacted: counters[2] += winners.
__global__ __launch_bounds__(256) void pt_refine_winner_kernel(int n, const u64 *__restrict__ key, const u64 *__restrict__ ball,
                                                               u64 *__restrict__ wkeys, int *__restrict__ wids,
                                                               int *__restrict__ counters) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if (k == PT_NONE || ball[i] != k) return;
    const int j = atomicAdd(&counters[2], 1);
    wkeys[j] = k;
    wids[j] = (int)i;
}
// the winners in key order: lab[j] = the target, pos[j] = j
__global__ __launch_bounds__(256) void pt_refine_target_kernel(int m, const int *__restrict__ ids, const int *__restrict__ target,
                                                               int *__restrict__ lab, int *__restrict__ pos) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < m) { lab[j] = target[ids[j]]; pos[j] = (int)j; }
}
// lab ascending, the winners of one target in their order: the first max_size - size are admitted (all without a cap).  The
// answer goes to the winner's place in key order, with the label of its source, or nparts when it is not admitted.
__global__ __launch_bounds__(256) void pt_refine_admit_kernel(int m, const int *__restrict__ lab, const int *__restrict__ pos,
                                                              const int *__restrict__ ids, const int *__restrict__ label,
                                                              const int *__restrict__ sizes, int max_size, int nparts,
                                                              int *__restrict__ src) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const bool in = max_size == 0 || (int)j - pt_run_start(lab, (int)j) < max_size - sizes[lab[j]];
    src[pos[j]] = in ? label[ids[pos[j]]] : nparts;
}
// lab ascending, the admitted of one source in their order (the others at the end under nparts): the first size - floor move.
// A node stands once in ids and the sweeps that read the labels are over, so the labels are written in place.
// totals[0] += movers, totals[1] += their gains.
__global__ __launch_bounds__(256) void pt_refine_apply_kernel(int m, const int *__restrict__ lab, const int *__restrict__ ids,
                                                              const int *__restrict__ sizes, int floor_size, int nparts,
                                                              const int *__restrict__ target, const int *__restrict__ gain,
                                                              int *__restrict__ label, u64 *__restrict__ totals) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int p = lab[j];
    if (p == nparts || (int)j - pt_run_start(lab, (int)j) >= sizes[p] - floor_size) return;
    const int v = ids[j];
    label[v] = target[v];
    atomicAdd(&totals[0], 1ull);
    atomicAdd(&totals[1], (u64)gain[v]);
}
__global__ __launch_bounds__(256) void pt_check_labels_kernel(int n, const int *__restrict__ label, int nparts, int *__restrict__ sizes,
                                                              int *__restrict__ err) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = label[i];
    if (l < 0 || l >= nparts) atomicOr(err, 1);
    else atomicAdd(&sizes[l], 1);
}
__global__ __launch_bounds__(256) void pt_check_empty_kernel(int nparts, const int *__restrict__ sizes, int *__restrict__ err) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < nparts && sizes[p] == 0) atomicOr(err, 2);
}

// ---- quotient graph -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_cut_count_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                           const int *__restrict__ part, int *__restrict__ cnt) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int pv = part[v];
    int c = 0;
    for (roff_t k = xadj[v], e = xadj[v + 1]; k < e; ++k) c += part[adj[k]] != pv;
    cnt[v] = c;
}
__global__ __launch_bounds__(256) void pt_cut_fill_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                          const int *__restrict__ part, const roff_t *__restrict__ pos,
                                                          u64 *__restrict__ keys) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int pv = part[v];
    roff_t o = pos[v];
    for (roff_t k = xadj[v], e = xadj[v + 1]; k < e; ++k) {
        const int pu = part[adj[k]];
        if (pu != pv) keys[o++] = ((u64)(unsigned)pv << 32) | (unsigned)pu;
    }
}
__global__ __launch_bounds__(256) void pt_quot_rows_kernel(long m, const u64 *__restrict__ keys, int *__restrict__ cnt,
                                                           int *__restrict__ aq) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    atomicAdd(&cnt[(unsigned)(keys[j] >> 32)], 1);
    aq[j] = (int)(keys[j] & 0xFFFFFFFFull);
}

// ---- element graph --------------------------------------------------------------------------------------------------
// One thread per element e.  A candidate f reached through dof number a of e is taken there only when a is the first dof of
// e that f holds, so every neighbour is seen once; then the dofs from a on are counted.  FILL = false counts, true writes.
template <bool FILL>
__global__ __launch_bounds__(256) void pt_elem_graph_kernel(int NE, const int *__restrict__ e2d_I, const int *__restrict__ e2d_J,
                                                            const int *__restrict__ d2e_I, const int *__restrict__ d2e_J,
                                                            int min_shared, int *__restrict__ cnt,
                                                            const roff_t *__restrict__ xadj, int *__restrict__ adj) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int b0 = e2d_I[e], b1 = e2d_I[e + 1];
    int c = 0;
    roff_t o = FILL ? xadj[e] : 0;
    for (int a = b0; a < b1; ++a) {
        const int d = e2d_J[a];
        for (int x = d2e_I[d], x1 = d2e_I[d + 1]; x < x1; ++x) {
            const int f = d2e_J[x];
            if (f == (int)e) continue;
            const int f0 = e2d_I[f], f1 = e2d_I[f + 1];
            bool earlier = false;
            for (int b = b0; b < a && !earlier; ++b) {
                const int db = e2d_J[b];
                for (int y = f0; y < f1; ++y) earlier |= e2d_J[y] == db;
            }
            if (earlier) continue;
            int shared = 1;
            for (int b = a + 1; b < b1; ++b) {
                const int db = e2d_J[b];
                for (int y = f0; y < f1; ++y) shared += e2d_J[y] == db;
            }
            if (shared < min_shared) continue;
            if (FILL) adj[o++] = f;
            ++c;
        }
    }
    if (!FILL) cnt[e] = c;
}
__global__ __launch_bounds__(256) void pt_row_sort_kernel(int n, const roff_t *__restrict__ xadj, int *__restrict__ adj) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const roff_t b = xadj[v], e = xadj[v + 1];
    for (roff_t i = b + 1; i < e; ++i) {  // insertion sort, rows are short
        const int x = adj[i];
        roff_t j = i - 1;
        while (j >= b && adj[j] > x) { adj[j + 1] = adj[j]; --j; }
        adj[j + 1] = x;
    }
}

// ---- checks ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_check_xadj_kernel(int n, const roff_t *__restrict__ xadj, int *__restrict__ err) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if ((i == 0 && xadj[0] != 0) || xadj[i + 1] < xadj[i]) atomicOr(err, 1);
}
__global__ __launch_bounds__(256) void pt_check_adj_kernel(int n, const roff_t *__restrict__ xadj, const int *__restrict__ adj,
                                                           int *__restrict__ err) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    for (roff_t k = xadj[v], e = xadj[v + 1]; k < e; ++k) {
        const int u = adj[k];
        if (u < 0 || u >= n) { atomicOr(err, 2); continue; }
        bool back = false;
        for (roff_t j = xadj[u], je = xadj[u + 1]; j < je && !back; ++j) back = adj[j] == (int)v;
        if (!back) atomicOr(err, 4);
    }
}
__global__ __launch_bounds__(256) void pt_check_eptr_kernel(int NE, const int *__restrict__ ptr, int *__restrict__ err) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    if ((e == 0 && ptr[0] != 0) || ptr[e + 1] <= ptr[e]) atomicOr(err, 1);
}
__global__ __launch_bounds__(256) void pt_check_repeat_kernel(int NE, const int *__restrict__ ptr, const int *__restrict__ J,
                                                              int *__restrict__ err) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    for (int a = ptr[e], e1 = ptr[e + 1]; a < e1; ++a)
        for (int b = a + 1; b < e1; ++b)
            if (J[a] == J[b]) atomicOr(err, 4);
}
__global__ __launch_bounds__(256) void pt_check_dofs_kernel(long nconn, int ND, const int *__restrict__ J, int *__restrict__ err) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < nconn && (J[k] < 0 || J[k] >= ND)) atomicOr(err, 2);
}

// ---- launches ---------------------------------------------------------------------------------------------------------
// the graph of a call with its stream and the seed of its priorities: what the row sweeps are launched with
struct GraphView {
    hipStream_t s;
    int n;
    const roff_t *xadj;
    const int *adj;
    unsigned seed;
};
// one group of PT_LPR lanes per row: kernel(n, xadj, adj, args...)
template <class K, class... A>
void sweep(const GraphView &g, K kernel, A... args) {
    hipLaunchKernelGGL(kernel, grid_rows(g.n), dim3(256), 0, g.s, g.n, g.xadj, g.adj, args...);
    SA_HIP_CHECK(hipGetLastError());
}
// fills of lists that may be empty
void fill_int(hipStream_t s, long n, int v, int *a) {
    if (n) dev_fill(s, n, v, a);
}
void fill_u64(hipStream_t s, long n, u64 v, u64 *a) {
    if (n) dev_fill(s, n, v, a);
}
// one hop of a ball sweep; first / last pick the instantiation (state and newseed are read by those forms alone)
void ball_min(const GraphView &g, bool first, bool last, const int *state, const u64 *src, u64 *dst, int *newseed) {
    const auto kernel = first ? (last ? pt_ball_min_kernel<true, true> : pt_ball_min_kernel<true, false>)
                              : (last ? pt_ball_min_kernel<false, true> : pt_ball_min_kernel<false, false>);
    sweep(g, kernel, state, g.seed, src, dst, newseed);
}
void ball_flag(const GraphView &g, bool last, const int *src, int *dst, const int *newseed, int seedval, int *state,
               int *counters) {
    sweep(g, last ? pt_ball_flag_kernel<true> : pt_ball_flag_kernel<false>, src, dst, newseed, seedval, state, counters);
}

struct Grower {
    const GraphView g;
    const hipStream_t s;   // = g.s
    const int n;           // = g.n
    DBuf<int> a, b, isseed, counters;
    DBuf<u64> key;
    int *label = nullptr;  // a.p or b.p: the current labels
    int nlabels = 0;
    explicit Grower(const GraphView &g_)
        : g(g_), s(g_.s), n(g_.n), a((size_t)n), b((size_t)n), isseed((size_t)n), counters(2), key(1) {
        label = a.p;
        isseed.zero(s);
    }
    int *other() const { return label == a.p ? b.p : a.p; }
    void grow(const int *dom) {
        for (;;) {
            counters.zero(s);
            sweep(g, pt_grow_kernel, label, dom, other(), counters.p);
            label = other();
            const auto c = counters.to_host(s);
            if (c[1] == 0) return;
            if (c[0] == 0) {  // a component without a seed
                fill_u64(s, 1, PT_NONE, key.p);
                launch_flat(s, n, pt_min_unlabelled_kernel, label, g.seed, key.p);
                hipLaunchKernelGGL(pt_stall_seed_kernel, dim3(1), dim3(1), 0, s, key.p, nlabels, label, isseed.p);
                SA_HIP_CHECK(hipGetLastError());
                ++nlabels;
            }
        }
    }
    // `growth = 1`: rounds of the claim sweep, the two sorts and the apply step, one read of the counters per round; then the
    // release to grow().  The round that finds every node labelled, or no claimant, labels nothing and is not counted.
    GrowthStats grow_balanced(int cap) {
        GrowthStats st;
        DBuf<int> sizes((size_t)nlabels), claim((size_t)n), ids((size_t)n), ids2((size_t)n), lab((size_t)n), lab2((size_t)n);
        DBuf<u64> keys((size_t)n), keys2((size_t)n);
        const int lab_bits = bits_for(nlabels);
        PairSorter<u64> sorter(s, n, 48, lab_bits);
        int first_unlabelled = -1;
        for (;;) {
            sizes.zero(s);
            counters.zero(s);
            launch_flat(s, n, pt_count_kernel, label, sizes.p);
            sweep(g, pt_claim_kernel, label, sizes.p, cap, g.seed, claim.p, keys.p, ids.p, counters.p);
            const auto c = counters.to_host(s);
            const int m = c[0], unlabelled = c[1];
            if (first_unlabelled < 0) first_unlabelled = unlabelled;
            st.quota_nodes = first_unlabelled - unlabelled;
            if (unlabelled == 0) break;
            if (m == 0) {   // release
                DBuf<int> nopen(1);
                nopen.zero(s);
                launch_flat(s, nlabels, pt_count_open_kernel, sizes.p, cap, nopen.p);
                st.open_parts = nopen.to_host(s)[0];
                st.released_nodes = unlabelled;
                break;
            }
            ++st.rounds;
            sorter.sort(keys.p, keys2.p, ids.p, ids2.p, m, 48);
            launch_flat(s, m, pt_claim_gather_kernel, ids2.p, claim.p, lab.p);
            sorter.sort(lab.p, lab2.p, ids2.p, ids.p, m, lab_bits);
            launch_flat(s, m, pt_claim_apply_kernel, lab2.p, ids.p, sizes.p, cap, label);
        }
        SA_HIP_CHECK(hipStreamSynchronize(s));   // the temporaries go out of scope
        if (st.released_nodes) grow(nullptr);
        return st;
    }
    // sizes of the current labels (nlabels + 1 entries allocated, the last unused by the count)
    void sizes_of(DBuf<int> &sizes) {
        sizes.alloc((size_t)nlabels + 1);
        sizes.zero(s);
        launch_flat(s, n, pt_count_kernel, label, sizes.p);
    }
    // the parts with k[p] > 0 are cleared down to their k[p] nodes of lowest priority; km1 = max(k - 1, 0)
    void reseed(const DBuf<int> &sizes, const DBuf<int> &k, const DBuf<int> &km1) {
        DBuf<int> start((size_t)nlabels + 1), off((size_t)nlabels + 1);
        exclusive_scan_int(s, nlabels, sizes.p, start.p);
        exclusive_scan_int(s, nlabels, km1.p, off.p);
        DBuf<u64> keys((size_t)n), keys2((size_t)n);
        DBuf<int> ids((size_t)n), ids2((size_t)n);
        launch_flat(s, n, pt_sort_keys_kernel, label, g.seed, keys.p, ids.p);
        const int end_bit = 32 + bits_for(nlabels);
        PairSorter<u64> sorter(s, n, end_bit);
        sorter.sort(keys.p, keys2.p, ids.p, ids2.p, n, end_bit);
        launch_flat(s, n, pt_reseed_kernel, keys2.p, ids2.p, start.p, k.p, off.p, nlabels, label, isseed.p);
        nlabels += read_one(off.p + nlabels, s);  // (synchronises: the temporaries go out of scope)
    }
    // Spaced first seeding.  One independent set: rounds of r min sweeps, the decision and r flag sweeps, one read of the
    // counters per round.  Returns the seeds found; gives up once they exceed `limit` (the set is then not needed).
    struct Spaced {
        DBuf<int> state, newseed, fa, fb;
        DBuf<u64> ka, kb;
    };
    int independent_set(Spaced &w, int r, int seedval, int limit, int &rounds) {
        int found = 0;
        for (;;) {
            for (int j = 1; j <= r; ++j)   // (the first sweep reads no src, the last writes no dst)
                ball_min(g, j == 1, j == r, w.state.p, j % 2 ? w.kb.p : w.ka.p, j % 2 ? w.ka.p : w.kb.p, w.newseed.p);
            counters.zero(s);
            spread(w, r, seedval);
            const auto c = counters.to_host(s);
            ++rounds;
            found += c[0];
            if (c[1] == 0 || found > limit) return found;
        }
    }
    // r flag sweeps from newseed; the last one applies the round to the states and counts
    void spread(Spaced &w, int r, int seedval) {
        for (int j = 1; j <= r; ++j)
            ball_flag(g, j == r, j == 1 ? w.newseed.p : (j % 2 ? w.fb.p : w.fa.p), j % 2 ? w.fa.p : w.fb.p, w.newseed.p, seedval,
                      w.state.p, counters.p);
    }
    SeedingStats seed_spaced(int target) {
        SeedingStats st;
        Spaced w;
        w.state.alloc((size_t)n);
        w.newseed.alloc((size_t)n);
        w.fa.alloc((size_t)n);
        w.fb.alloc((size_t)n);
        w.ka.alloc((size_t)n);
        w.kb.alloc((size_t)n);
        int r = 1, ns = 0;
        for (;; ++r) {   // the smallest radius whose set is within the target
            w.state.zero(s);
            ns = independent_set(w, r, PT_SEED, r < PT_RADIUS_MAX ? target : INT_MAX, st.rounds);
            if (ns <= target || r == PT_RADIUS_MAX) break;
        }
        int ne = 0;
        if (ns < target) {   // top-up from the greedy (r - 1)-independent extension
            launch_flat(s, n, pt_ext_init_kernel, r == 1 ? PT_EXT : PT_UNDECIDED, w.state.p, w.newseed.p);
            if (r == 1) ne = n - ns;
            else {
                counters.zero(s);
                spread(w, r - 1, PT_SEED);   // the nodes within r - 1 hops of the first stage are out
                if (counters.to_host(s)[1]) ne = independent_set(w, r - 1, PT_EXT, INT_MAX, st.rounds);
            }
        }
        const int nsel = ns < target ? std::min(target, ns + ne) : ns;
        DBuf<u64> keys((size_t)n), keys2((size_t)n);
        DBuf<int> ids((size_t)n), ids2((size_t)n);
        launch_flat(s, n, pt_spaced_keys_kernel, w.state.p, g.seed, keys.p, ids.p);
        PairSorter<u64> sorter(s, n, 34);
        sorter.sort(keys.p, keys2.p, ids.p, ids2.p, n, 34);
        label = a.p;
        launch_flat(s, n, pt_spaced_label_kernel, keys2.p, ids2.p, ns, nsel, label, isseed.p);
        SA_HIP_CHECK(hipStreamSynchronize(s));   // the temporaries go out of scope
        nlabels = nsel;
        st.radius = r;
        st.seeds_first = ns;
        st.seeds = nsel;
        return st;
    }
    void recentre() {
        DBuf<int> depth((size_t)n);
        sweep(g, pt_boundary_kernel, label, depth.p);
        for (int d = 1;; ++d) {
            counters.zero(s);
            sweep(g, pt_depth_kernel, label, d, depth.p, counters.p);
            if (counters.to_host(s)[0] == 0) break;
        }
        DBuf<u64> best((size_t)nlabels);
        best.zero(s);
        launch_flat(s, n, pt_centre_max_kernel, label, depth.p, isseed.p, g.seed, best.p);
        launch_flat(s, n, pt_centre_pick_kernel, label, depth.p, isseed.p, g.seed, best.p);
        SA_HIP_CHECK(hipStreamSynchronize(s));
    }
    bool merge_round(int min_size, int max_size) {
        DBuf<int> sizes, target((size_t)nlabels), info(1);
        DBuf<u64> prop((size_t)nlabels), win((size_t)nlabels);
        sizes_of(sizes);
        fill_u64(s, nlabels, PT_NONE, prop.p);
        fill_u64(s, nlabels, PT_NONE, win.p);
        info.zero(s);
        sweep(g, pt_propose_kernel, label, sizes.p, min_size, max_size, prop.p);
        launch_flat(s, nlabels, pt_win_kernel, prop.p, sizes.p, win.p);
        launch_flat(s, nlabels, pt_decide_kernel, prop.p, win.p, target.p, info.p);
        launch_flat(s, n, pt_relabel_kernel, target.p, label);
        return info.to_host(s)[0] != 0;
    }
};

constexpr int PT_MERGE_ROUNDS = 8;
constexpr int PT_REPAIR_ROUNDS = 32;

}  // namespace

int64_t check_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj) {
    if (n == 0) return 0;
    DBuf<int> err(1);
    err.zero(s);
    launch_flat(s, n, pt_check_xadj_kernel, xadj, err.p);
    SA_REQUIRE(!err.to_host(s)[0], "xadj: must start at 0 and ascend");
    const roff_t nnz = read_one(xadj + n, s);
    SA_REQUIRE(nnz == 0 || adj, "null argument: adj");
    launch_flat(s, n, pt_check_adj_kernel, xadj, adj, err.p);
    const int bits = err.to_host(s)[0];
    SA_REQUIRE(!(bits & 2), "adj: entry outside [0, n)");
    SA_REQUIRE(!(bits & 4), "graph is not symmetric: an entry without its transpose");
    return nnz;
}

long check_mesh_device(hipStream_t s, int NE, const int *e2d_I, const int *e2d_J, int ND) {
    if (NE == 0) return 0;
    DBuf<int> err(1);
    err.zero(s);
    launch_flat(s, NE, pt_check_eptr_kernel, e2d_I, err.p);
    SA_REQUIRE(!err.to_host(s)[0], "elem_ptr: must start at 0 and every element needs a dof");
    const long nconn = read_one(e2d_I + NE, s);
    launch_flat(s, nconn, pt_check_dofs_kernel, ND, e2d_J, err.p);
    launch_flat(s, NE, pt_check_repeat_kernel, e2d_I, e2d_J, err.p);
    const int bits = err.to_host(s)[0];
    SA_REQUIRE(!(bits & 2), "elem_to_dof entry out of range");
    SA_REQUIRE(!(bits & 4), "elem_to_dof: an element lists a dof twice");
    return nconn;
}

void resolve_partition_sizes(int epa, const PartitionOptions &o, int *max_size, int *min_size) {
    *max_size = o.max_size < 0 ? (int)std::min<int64_t>(2ll * epa, INT_MAX) : o.max_size;
    *min_size = o.min_size < 0 ? epa / 4 : o.min_size;
}

void partition_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, int epa, const PartitionOptions &o,
                            int *part, int *nparts_out, PartitionStats *stats) {
    SA_REQUIRE(n >= 0, "n < 0");
    SA_REQUIRE(epa >= 1, "elems_per_agg < 1");
    SA_REQUIRE(o.lloyd_iters >= 0 && o.max_size >= -1 && o.min_size >= -1, "partition options: lloyd_iters >= 0, sizes >= -1");
    SA_REQUIRE(o.seeding == 0 || o.seeding == 1, "partition options: seeding must be 0 or 1");
    SA_REQUIRE(o.growth == 0 || o.growth == 1, "partition options: growth must be 0 or 1");
    *nparts_out = 0;
    *stats = PartitionStats();
    if (n == 0) return;
    int max_size = 0, min_size = 0;
    resolve_partition_sizes(epa, o, &max_size, &min_size);
    Grower g(GraphView{s, n, xadj, adj, o.seed});
    const int target = (int)(((int64_t)n + epa - 1) / epa);
    if (o.seeding == 1) {
        stats->seeding = g.seed_spaced(target);
    } else {   // first seeding: one part 0 that holds every node, target seeds
        g.label = g.a.p;
        g.a.zero(s);
        g.nlabels = 1;
        DBuf<int> sizes(2), k(1), km1(2);
        const int hs[2] = {n, 0}, hk[2] = {target - 1, 0};
        upload_async(sizes.p, hs, 2, s);
        upload_async(k.p, &target, 1, s);
        upload_async(km1.p, hk, 2, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));      // (the sources are locals)
        g.reseed(sizes, k, km1);
    }
    const auto grow = [&] {
        if (o.growth == 1) stats->growth = g.grow_balanced(epa);
        else g.grow(nullptr);
    };
    grow();
    for (int it = 0; it < o.lloyd_iters; ++it) {
        g.recentre();
        grow();
    }
    if (max_size > 0)
        for (int r = 0; r < PT_REPAIR_ROUNDS; ++r) {  // pieces are strictly smaller; the bound is for hubs (partition_model.py)
            DBuf<int> sizes, k((size_t)g.nlabels), km1((size_t)g.nlabels + 1), info(1);
            g.sizes_of(sizes);
            info.zero(s);
            launch_flat(s, g.nlabels, pt_over_kernel, sizes.p, max_size, epa, k.p, km1.p, info.p);
            if (info.to_host(s)[0] == 0) break;
            DBuf<int> old((size_t)n);
            copy_device(old.p, (const int *)g.label, (size_t)n, s);
            g.reseed(sizes, k, km1);
            g.grow(old.p);
            SA_HIP_CHECK(hipStreamSynchronize(s));
        }
    if (min_size > 0)
        for (int r = 0; r < PT_MERGE_ROUNDS; ++r)
            if (!g.merge_round(min_size, max_size)) break;
    renumber_device(s, n, g.label, g.nlabels, part, nparts_out);
}

// parts numbered by their smallest member; label and part are different arrays
void renumber_device(hipStream_t s, int n, const int *label, int nlabels, int *part, int *nparts_out) {
    DBuf<int> minid((size_t)nlabels), first((size_t)n), rank((size_t)n + 1), newnum((size_t)nlabels);
    fill_int(s, nlabels, n, minid.p);
    launch_flat(s, n, pt_minid_kernel, label, minid.p);
    launch_flat(s, n, pt_first_kernel, label, minid.p, first.p);
    exclusive_scan_int(s, n, first.p, rank.p);
    launch_flat(s, n, pt_newnum_kernel, label, first.p, rank.p, newnum.p);
    launch_flat(s, n, pt_apply_kernel, label, newnum.p, part);
    *nparts_out = read_one(rank.p + n, s);
}

void check_partition_device(hipStream_t s, int n, const int *label, int nparts) {
    SA_REQUIRE(nparts >= 0 && nparts <= n, "nparts outside [0, n]");
    if (n == 0) return;
    DBuf<int> sizes((size_t)nparts), err(1);
    sizes.zero(s);
    err.zero(s);
    launch_flat(s, n, pt_check_labels_kernel, label, nparts, sizes.p, err.p);
    launch_flat(s, nparts, pt_check_empty_kernel, sizes.p, err.p);
    const int bits = err.to_host(s)[0];
    SA_REQUIRE(!(bits & 1), "part: label outside [0, nparts)");
    SA_REQUIRE(!(bits & 2), "part: an empty part");
}

// Rounds of: sizes, the count sweep, the free check over the compacted rows, two ball sweeps of the keys, the winners, then
// the two quotas (sort by key, stable sort by target, stable sort by source) and the apply step.  One read of the counters per
// round (free rows and winners); the movers and their gains are summed on the device and read once at the end.
RefineStats refine_partition_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, int nparts, int *label, int rounds,
                                    int max_size, int min_size, unsigned seed) {
    SA_REQUIRE(rounds >= 0 && max_size >= 0 && min_size >= 0, "refinement: rounds, max_size and min_size must be >= 0");
    RefineStats st;
    if (n == 0 || rounds == 0) return st;
    const GraphView g{s, n, xadj, adj, seed};
    const int floor_size = std::max(min_size, 1);
    DBuf<int> sizes((size_t)nparts), target((size_t)n), gain((size_t)n), cand((size_t)n), counters(3);
    DBuf<int> ids((size_t)n), ids2((size_t)n), lab((size_t)n), lab2((size_t)n), pos((size_t)n), pos2((size_t)n);
    DBuf<u64> key((size_t)n), ka((size_t)n), kb((size_t)n), wkeys((size_t)n), wkeys2((size_t)n), totals(2);
    const int lab_bits = bits_for(nparts + 1);
    PairSorter<u64> sorter(s, n, 48, lab_bits);
    totals.zero(s);
    const dim3 free_grid((unsigned)std::min<long>(((long)n + 3) / 4, 2048));
    while (st.rounds < rounds) {
        sizes.zero(s);
        counters.zero(s);
        fill_u64(s, n, PT_NONE, key.p);
        launch_flat(s, n, pt_count_kernel, label, sizes.p);
        sweep(g, pt_refine_count_kernel, label, sizes.p, max_size, floor_size, target.p, gain.p, cand.p, counters.p);
        hipLaunchKernelGGL(pt_refine_free_kernel, free_grid, dim3(256), 0, s, xadj, adj, label, cand.p, gain.p, seed, key.p,
                           counters.p);
        SA_HIP_CHECK(hipGetLastError());
        ball_min(g, false, false, nullptr, key.p, ka.p, nullptr);
        ball_min(g, false, false, nullptr, ka.p, kb.p, nullptr);
        launch_flat(s, n, pt_refine_winner_kernel, key.p, kb.p, wkeys.p, ids.p, counters.p);
        const auto c = counters.to_host(s);
        if (c[1] == 0) { st.converged = 1; break; }
        const int m = c[2];
        SA_REQUIRE(m >= 1 && m <= n, "refinement: candidates without a winner");
        ++st.rounds;
        sorter.sort(wkeys.p, wkeys2.p, ids.p, ids2.p, m, 48);
        launch_flat(s, m, pt_refine_target_kernel, ids2.p, target.p, lab.p, pos.p);
        sorter.sort(lab.p, lab2.p, pos.p, pos2.p, m, lab_bits);
        launch_flat(s, m, pt_refine_admit_kernel, lab2.p, pos2.p, ids2.p, label, sizes.p, max_size, nparts, lab.p);
        sorter.sort(lab.p, lab2.p, ids2.p, ids.p, m, lab_bits);
        launch_flat(s, m, pt_refine_apply_kernel, lab2.p, ids.p, sizes.p, floor_size, nparts, target.p, gain.p, label, totals.p);
    }
    const auto tot = totals.to_host(s);   // (synchronises: the temporaries go out of scope)
    st.moved = (long long)tot[0];
    st.gain = (long long)tot[1];
    return st;
}

void element_graph_device(hipStream_t s, int NE, const int *e2d_I, const int *e2d_J, int ND, int min_shared,
                          DBuf<roff_t> &xadj, DBuf<int> &adj) {
    SA_REQUIRE(min_shared >= 1, "min_shared < 1");
    xadj.alloc((size_t)NE + 1);
    if (NE == 0) { xadj.zero(s); adj.alloc(0); return; }
    const long nconn = read_one(e2d_I + NE, s);
    DBuf<int> d2e_I((size_t)ND + 1), d2e_J((size_t)nconn), cnt((size_t)std::max(ND, NE) + 1);
    // (the lists need no order: every row of the graph is sorted at the end)
    dev_table_transpose(s, NE, e2d_I, e2d_J, nconn, ND, d2e_I.p, d2e_J.p, false, cnt.p);
    hipLaunchKernelGGL(pt_elem_graph_kernel<false>, grid_flat(NE), dim3(256), 0, s, NE, e2d_I, e2d_J, (const int *)d2e_I.p,
                       (const int *)d2e_J.p, min_shared, cnt.p, (const roff_t *)nullptr, (int *)nullptr);
    SA_HIP_CHECK(hipGetLastError());
    exclusive_scan_off(s, NE, cnt.p, xadj.p);
    const roff_t nnz = read_one(xadj.p + NE, s);
    adj.alloc((size_t)nnz);
    hipLaunchKernelGGL(pt_elem_graph_kernel<true>, grid_flat(NE), dim3(256), 0, s, NE, e2d_I, e2d_J, (const int *)d2e_I.p,
                       (const int *)d2e_J.p, min_shared, (int *)nullptr, (const roff_t *)xadj.p, adj.p);
    hipLaunchKernelGGL(pt_row_sort_kernel, grid_flat(NE), dim3(256), 0, s, NE, (const roff_t *)xadj.p, adj.p);
    SA_HIP_CHECK(hipGetLastError());
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

void quotient_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, const int *part, int nparts,
                           DBuf<roff_t> &xq, DBuf<int> &aq) {
    xq.alloc((size_t)nparts + 1);
    DBuf<int> cnt((size_t)std::max(n, nparts) + 1);
    DBuf<roff_t> pos((size_t)n + 1);
    roff_t ncut = 0;
    if (n) {
        hipLaunchKernelGGL(pt_cut_count_kernel, grid_flat(n), dim3(256), 0, s, n, xadj, adj, part, cnt.p);
        SA_HIP_CHECK(hipGetLastError());
        exclusive_scan_off(s, n, cnt.p, pos.p);
        ncut = read_one(pos.p + n, s);
    }
    SA_REQUIRE(ncut < (roff_t)INT_MAX, "quotient graph: more than 2^31 cut edges");
    DBuf<u64> keys((size_t)ncut), sorted((size_t)ncut), uniq((size_t)ncut);
    DBuf<int> nsel(1);
    int m = 0;
    if (ncut) {
        hipLaunchKernelGGL(pt_cut_fill_kernel, grid_flat(n), dim3(256), 0, s, n, xadj, adj, part, (const roff_t *)pos.p, keys.p);
        SA_HIP_CHECK(hipGetLastError());
        size_t tb = 0, tb2 = 0;
        const int end_bit = 32 + bits_for(nparts);
        SA_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys.p, sorted.p, (int)ncut, 0, end_bit, s));
        SA_HIP_CHECK(hipcub::DeviceSelect::Unique(nullptr, tb2, sorted.p, uniq.p, nsel.p, (int)ncut, s));
        DBuf<char> tmp(std::max(tb, tb2) + 16);
        SA_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys((void *)tmp.p, tb, keys.p, sorted.p, (int)ncut, 0, end_bit, s));
        SA_HIP_CHECK(hipcub::DeviceSelect::Unique((void *)tmp.p, tb2, sorted.p, uniq.p, nsel.p, (int)ncut, s));
        m = read_one(nsel.p, s);
    }
    aq.alloc((size_t)m);
    SA_HIP_CHECK(hipMemsetAsync(cnt.p, 0, ((size_t)nparts + 1) * sizeof(int), s));
    if (m) {
        hipLaunchKernelGGL(pt_quot_rows_kernel, grid_flat(m), dim3(256), 0, s, (long)m, (const u64 *)uniq.p, cnt.p, aq.p);
        SA_HIP_CHECK(hipGetLastError());
    }
    if (nparts) exclusive_scan_off(s, nparts, cnt.p, xq.p);
    else xq.zero(s);
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
