// Setup (ml_produce_data, adapt_update_operators) orchestration; the solve phase is cycle.hip.  Host C++ driving the
// HIP kernels; all numerics run on the device, the integer topology on the host.
#include "hierarchy.h"
#include "dist.h"
#include "spgemm.h"
#include "devtab.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace saamge_amd {

// grow-only scratch buffers that survive across chunks / levels / hierarchies
static DBuf<double> &scratch_pool(int slot) {
    static DBuf<double> *pools = new DBuf<double>[4];     // never destroyed: no HIP calls from static destructors
    return pools[slot];
}
static double *scratch_get(int slot, size_t need) {
    DBuf<double> &p = scratch_pool(slot);
    if (p.n < need) p.alloc(need + need / 8 + 64);
    return p.p;
}

static void finish_csr(DCsr &A) { A.lanes_per_row = pick_lanes_per_row(A.nnz, A.nrows > 0 ? A.nrows : 1); }

// Mixed elements: checks of a device-resident elem_ptr (NE + 1 entries) and elem_to_dof (elem_ptr[NE] entries, read only
// after the offsets passed), the sizes of the elements and their squares.  info = {error bits, MAX_ELEM_DOFS - smallest element,
// largest element}, zero-initialised.
constexpr int MAX_ELEM_DOFS = 32767;
__global__ __launch_bounds__(256) void elem_ptr_check_kernel(long NE, const int *__restrict__ ptr, int *__restrict__ info) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e == 0 && ptr[0] != 0) atomicOr(&info[0], 1);
    if (e >= NE) return;
    const int nd = ptr[e + 1] - ptr[e];
    if (nd <= 0) atomicOr(&info[0], 2);
    else if (nd > MAX_ELEM_DOFS) atomicOr(&info[0], 4);
    else { atomicMax(&info[1], MAX_ELEM_DOFS - nd); atomicMax(&info[2], nd); }
}
__global__ __launch_bounds__(256) void dof_range_kernel(long nconn, int ND, const int *__restrict__ J, int *__restrict__ err) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < nconn && (J[k] < 0 || J[k] >= ND)) atomicOr(err, 8);
}
__global__ __launch_bounds__(256) void elem_sq_kernel(long NE, const int *__restrict__ ptr, int *__restrict__ sq) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < NE) { const int nd = ptr[e + 1] - ptr[e]; sq[e] = nd * nd; }
}

// Checks elem_ptr / elem_to_dof of the mixed entries before any other use: host-resident offsets on the host, device-resident
// ones by the kernels above.  Returns the element size if all elements have the same, 0 otherwise; max_nd = the largest.
static int check_elem_ptr(int NE, const int *elem_ptr, const int *elem_to_dof, int ND, int &max_nd, hipStream_t s) {
    int bits = 0, mn = 0, mx = 0;
    long nconn = 0;
    if (!is_device_ptr(elem_ptr)) {
        bits |= elem_ptr[0] != 0 ? 1 : 0;
        mn = MAX_ELEM_DOFS;
        for (int e = 0; e < NE && !bits; ++e) {
            const int nd = elem_ptr[e + 1] - elem_ptr[e];
            if (nd <= 0) bits |= 2;
            else if (nd > MAX_ELEM_DOFS) bits |= 4;
            else { mn = std::min(mn, nd); mx = std::max(mx, nd); }
        }
        if (!bits) nconn = elem_ptr[NE];
    } else {
        DBuf<int> info(3);
        info.zero(s);
        hipLaunchKernelGGL(elem_ptr_check_kernel, dim3(div_up((long)NE, 256)), dim3(256), 0, s, (long)NE, elem_ptr, info.p);
        SA_HIP_CHECK(hipGetLastError());
        const auto h = info.to_host(s);
        bits = h[0]; mn = MAX_ELEM_DOFS - h[1]; mx = h[2];
        if (!bits) {
            int last = read_one(elem_ptr + NE, s);
            nconn = last;
        }
    }
    SA_REQUIRE(!(bits & 1), "elem_ptr[0] must be 0");
    SA_REQUIRE(!(bits & 2), "elem_ptr: an element without dofs or decreasing offsets");
    SA_REQUIRE(!(bits & 4), "elem_ptr: an element with more than 32767 dofs");
    if (!is_device_ptr(elem_to_dof)) {
        for (long k = 0; k < nconn; ++k)
            SA_REQUIRE(elem_to_dof[k] >= 0 && elem_to_dof[k] < ND, "elem_to_dof entry out of range");
    } else {
        DBuf<int> err(1);
        err.zero(s);
        hipLaunchKernelGGL(dof_range_kernel, dim3(div_up(nconn, 256)), dim3(256), 0, s, nconn, ND, elem_to_dof, err.p);
        SA_HIP_CHECK(hipGetLastError());
        SA_REQUIRE(!err.to_host(s)[0], "elem_to_dof entry out of range");
    }
    max_nd = mx;
    return mn == mx ? mx : 0;
}


// In-place all-gather of an array of which rank r holds the elements [at(begin[r]), at(begin[r + 1])), `bytes` bytes each.
template <class Begin, class At>
static void allgather_ranges(const Params &P, void *p, long long bytes, const Begin &begin, At at, const char *what) {
    std::vector<long long> off(begin.size());
    for (size_t r = 0; r < off.size(); ++r) off[r] = bytes * (long long)at(begin[r]);
    SA_REQUIRE(P.allgather(P.allgather_ctx, p, off.data()) == 0, std::string("all-gather (") + what + ") failed");
}
static const auto same_index = [](long long i) { return i; };
// how many items from i0 on (at least one, below i1) fit `budget` bytes
template <class Bytes>
static int fit_count(int i0, int i1, size_t budget, Bytes bytes_of) {
    size_t bytes = 0;
    int cnt = 0;
    for (; i0 + cnt < i1; ++cnt) {
        const size_t add = bytes_of(i0 + cnt);
        if (cnt > 0 && bytes + add > budget) break;
        bytes += add;
    }
    return cnt;
}

// Ac = R (A P) as general sparse products (mfem::RAP, amg/inc/tg.hpp:696-709)
static void galerkin_general(hipStream_t s, const DCsr &A, const DCsr &P, const DCsr &R, DCsr &Ac) {
    DCsr AP;
    spgemm(s, A, P, nullptr, nullptr, 1.0, 0.0, AP);
    Ac = DCsr();      // (an operator update: the old product goes before the new one is made)
    spgemm(s, R, AP, nullptr, nullptr, 1.0, 0.0, Ac);
}

// ---------------------------------------------------------------------------------------
// one coarsening: tg_init_data + tg_build_hierarchy + tg_update_coarse_operator
// ---------------------------------------------------------------------------------------
// P (smoothed when nu_pro > 0), R and Ac = R A P of level `lev` from its tentative prolongator
// (tg_smooth_interp + tg_coarse_matr, amg/inc/tg.hpp:679-709).  `first`: P / R still hold the
// tentative pair just built; otherwise (operator update) the stored tentative one is re-smoothed.
static void level_galerkin(Hierarchy &H, int lev, bool first, hipStream_t s) {
    Level &L = *H.levels[lev];
    const Params &P = H.params;
    const Relations &rel = L.rel;
    const int world = P.world > 1 ? P.world : 1;
    if (P.nu_pro[lev] == 0) {
        std::vector<long long> nnz_off;
        rap_mis(s, L.drel, rel, L.A, L.mis_k, L.mis_coloff, L.d_mis_k.p, L.d_mis_coloff.p,
                L.d_mis_u_off.p, L.mis_U.p, L.Ac, P.rank, world, world > 1 ? &nnz_off : nullptr);
        if (world > 1 && L.Ac.nnz > 0) {   // every rank computed the row blocks of its MIS range
            allgather_ranges(P, L.Ac.col.p, 4, nnz_off, same_index, "Ac columns");
            allgather_ranges(P, L.Ac.val.p, 8, nnz_off, same_index, "Ac values");
        }
    } else {
        // interp_smooth (amg/src/interp.cpp:172-229): P = prod_k (I + (1/tau_k) Dinv_neg A) P_tent with
        // tau_k = sin^2(k pi / (2 nu + 1)) (smpr_sa_poly_roots, amg/src/smpr.cpp:266-280); then
        // R = P^T and Ac = R A P (galerkin_general).
        const int nu = P.nu_pro[lev];
        if (first) L.Ptent = std::move(L.P);
        DCsr tmp[2];
        const DCsr *cur = &L.Ptent;
        for (int k = 1; k <= nu; ++k) {
            const double sn = std::sin((double)k * M_PI / (double)(2 * nu + 1));
            DCsr &dst = tmp[k & 1];
            dst = DCsr();
            spgemm(s, L.A, *cur, cur, L.sm.dinv_neg.p, 1.0 / (sn * sn), 1.0, dst);
            cur = &dst;
        }
        if (P.smooth_drop_tol != 0.0)   // AltThreshold (amg/src/interp.cpp:219-227)
            csr_threshold(s, tmp[nu & 1], P.smooth_drop_tol, L.P);
        else
            L.P = std::move(tmp[nu & 1]);
        csr_transpose(s, L.P, L.R);
        galerkin_general(s, L.A, L.P, L.R, L.Ac);
    }
}

// fn as the body of a side task (side_task.h) that works on GPU `dev` and allocates, copies and frees on `stream`
template <class F>
static auto on_gpu(int dev, hipStream_t stream, F fn) {
    return [dev, stream, fn = std::move(fn)]() mutable { adopt_device(dev); set_thread_stream(stream); fn(); };
}

// The deferred Galerkin product (see Hierarchy::galerkin_task): wait for it and hand its result to the next level.
static void join_galerkin(Hierarchy &H) {
    if (H.galerkin_lev < 0) return;
    const int lev = H.galerkin_lev;
    H.galerkin_lev = -1;
    H.galerkin_task.join();
    H.levels[lev + 1]->A = std::move(H.levels[lev]->Ac);     // A_{l+1} = Ac_l  (amg/src/ml.cpp:134)
}

struct DeviceInputs {   // level-0 inputs that already live on the device (see hierarchy_create)
    const int *e2d = nullptr, *part = nullptr;
    const int *e2d_I = nullptr;     // mixed elements (nde = 0): the checked offsets
    const signed char *bdr = nullptr;
    int NE = 0, nde = 0;
};

static void prepare_next_host(const Level &L, const roff_t *p_rowptr_dev, const double *p_val_dev, int p_nrows,
                              int64_t p_nnz, hipStream_t s, NextPrep &out);

// ---- build_level: one coarsening as a sequence of stages over the state below ----
// packed eigenpairs of the agglomerates of one chunk of the eigenproblem stage
struct Chunk { int ae0, count; DBuf<double> evals, evecs; std::vector<int64_t> eoff, xoff; DBuf<int64_t> d_eoff, d_xoff; };
struct LevelBuild {
    Hierarchy &H;
    const int lev;
    Level &L;
    const Params &P;
    hipStream_t s;
    const int nparts, world, dev;
    PhaseTimer tm;
    // topology: the MIS tables are built on a host thread while the GPU solves the local eigenproblems
    HostCsr aggA;
    bool aggregates = false;
    bool operator_pending = false;      // the level's operator is still in the making (deferred Galerkin product of the finer level)
    // local eigenproblems: sizes and ownership of the agglomerates, the chunks' results
    bool keep_rows = false;
    std::vector<int> sizes, ae_begin;
    int ae_lo = 0, ae_hi = 0;
    std::vector<Chunk> chunks;
    // (batches: what the eigensolvers run on -- the assembled batch itself, or the batch of the representatives of its
    // classes of bitwise identical matrices, dedupe.hip "Duplicate agglomerate matrices")
    EigBatch batches[2], assembled[2];
    LevelClasses classes;
    std::vector<DBuf<double>> kept;          // packed eigenpairs of the chunks' representatives
    std::vector<int> cls_of[2];              // per slot: class of every agglomerate of the chunk (empty: no classes)
    std::vector<int> solve_cls[2];           // per slot: classes of the matrices of the batch that is solved, in its order
    bool dedupe = false, dedupe_level = true;
    int pend_ae0[2] = {0, 0}, pend_cnt[2] = {0, 0};
    int64_t pend_row0[2] = {0, 0};
    bool counted[2] = {false, false};
    bool overlap_iter = false;
    hipStream_t iter_stream = nullptr;
    SideTask mis_task, iter_task;      // (last: joined before anything they work on goes away)

    LevelBuild(Hierarchy &H_, int lev_, int nparts_) : H(H_), lev(lev_), L(*H_.levels[lev_]), P(H_.params), s(H_.stream), nparts(nparts_),
                                                       world(H_.params.world > 1 ? H_.params.world : 1), dev(current_device()), tm(H_.stream) {}
    const DCsr *fine_A() const { return lev == 0 ? &L.A : nullptr; }
};

// positions of agglomerate ae's rows among the rows of the agglomerates [ae_lo, ae_hi) of this rank
static RowsSpan rows_span(const Relations &rel, int ae, int ae_lo, int ae_hi) {
    const auto &I = rel.AE_to_dof.I;
    return RowsSpan{(int64_t)I[ae] - (int64_t)I[ae_lo], (int64_t)I[ae_hi] - (int64_t)I[ae_lo]};
}
// offsets of packed eigenvalues (m_i each) and eigenvectors (n_i x m_i each)
static void packed_offsets(int count, const int *m, const int *n, std::vector<int64_t> &eoff, std::vector<int64_t> &xoff) {
    eoff.assign((size_t)count + 1, 0);
    xoff.assign((size_t)count + 1, 0);
    for (int i = 0; i < count; ++i) {
        eoff[i + 1] = eoff[i] + m[i];
        xoff[i + 1] = xoff[i] + (int64_t)m[i] * n[i];
    }
}
// contiguous ranges of [0, n), one per rank, balanced by cost(i): begin[r] .. begin[r + 1]
template <class Cost>
static std::vector<int> balanced_ranges(int n, int world, Cost cost) {
    std::vector<int> begin((size_t)world + 1, n);
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += cost(i);
    double run = 0.0;
    int r = 0;
    begin[0] = 0;
    for (int i = 0; i < n && r + 1 < world; ++i) {
        run += cost(i);
        while (r + 1 < world && run >= total * (r + 1) / world) begin[++r] = i + 1;
    }
    begin[world] = n;
    return begin;
}

// Stage 1: the agglomerate tables, the start of the MIS-table thread, the operator's SELL copy and smoother data.
static void level_topology(LevelBuild &B, Table &&e2d, const hvec<int> &part, const signed char *bdr_host, const DeviceInputs *din) {
    Hierarchy &H = B.H; Level &L = B.L; const Params &P = B.P; hipStream_t s = B.s;
    const int lev = B.lev, nparts = B.nparts;
    // Fine level, device-resident inputs: the SELL copy of the operator and the smoother diagonal (bandwidth work on A alone) are
    // built on a thread and stream of their own BESIDE the device build of the AE tables (integer work on elem_to_dof: sorts,
    // hash sets, atomics), and joined where they used to run, before the eigenproblems.
    SideTask op_task;
    const bool op_early = lev == 0 && din && !env_serial() && !profiler().enabled && H.galerkin_lev < 0 && (P.opt.overlap & 8);
    if (op_early) {
        hipStream_t os = side_stream(6);
        SA_HIP_CHECK(hipStreamSynchronize(s));          // (the operator's arrays are complete)
        op_task.start(on_gpu(B.dev, os, [&L, &P, os]() { operator_data(os, L.A, P.opt, true, L.sm); }));
    }
    bool on_device = false;
    if (din) {
        on_device = build_relations_ae_device(L.rel, L.drel, din->e2d, din->NE, din->nde, din->e2d_I, din->part, nparts,
                                              L.A.nrows, din->bdr, s);
        B.tm.lap("device topology (AE tables)", lev);
    }
    if (!on_device) {
        hvec<int> part_h;
        hvec<signed char> bdr_h;
        if (din) {   // agglomerates too large for the device kernels: fetch and take the host path
            if (din->e2d_I) {
                e2d.I = fetch_host(din->e2d_I, (size_t)din->NE + 1, s);
            } else {
                e2d.I.resize((size_t)din->NE + 1);
                for (int e = 0; e <= din->NE; ++e) e2d.I[e] = e * din->nde;
            }
            e2d.J = fetch_host(din->e2d, (size_t)e2d.I[din->NE], s);
            e2d.ncols = L.A.nrows;
            part_h = fetch_host(din->part, (size_t)din->NE, s);
            if (din->bdr) bdr_h = fetch_host(din->bdr, (size_t)L.A.nrows, s);
        }
        if (!L.rel_prebuilt)
            build_relations_ae(L.rel, std::move(e2d), din ? part_h : part, nparts, L.A.nrows,
                               din ? (din->bdr ? bdr_h.data() : nullptr) : bdr_host);
        B.tm.lap(L.rel_prebuilt ? "host topology (built beside the element matrices)" : "host topology (AE tables)", lev);
        upload_relations_ae(L.drel, L.rel, s);
        B.tm.lap("upload topology", lev);
    }
    // the MIS tables are built on a host thread while the GPU solves the local eigenproblems (do_aggregates, amg/src/ml.cpp:149:
    // aggregates with arbitration on the LAST coarsening; the greedy arbitration reads the level matrix on the host)
    HostCsr &aggA = B.aggA;
    B.aggregates = P.do_aggregates && lev == P.num_coarsenings - 1;
    if (B.aggregates) {
        join_galerkin(H);     // the arbitration reads this level's operator
        aggA.nrows = L.A.nrows;
        download(aggA.rowptr, L.A.rowptr, (size_t)L.A.nrows + 1, s);
        download(aggA.col, L.A.col, (size_t)L.A.nnz, s);
        download(aggA.val, L.A.val, (size_t)L.A.nnz, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
    }
    // (the tables go to the device from the same thread, on a side stream, while the eigensolver runs)
    hipStream_t mis_stream = side_stream(0);
    // SAAMGE_AMD_SERIAL=1: no worker threads anywhere in the setup (counter passes attribute launches per thread; the
    // work runs in line, same streams).  The "stream_stack.cpp: Check failed" aborts once seen under rocprofv3 --pmc came
    // from static destructors calling HIP at exit (fixed in round 4: those objects are never destroyed), not from threads
    B.mis_task.start(on_gpu(B.dev, mis_stream, [&B, mis_stream]() {      // (the worker allocates and copies: same GPU as the caller)
        Level &L = B.L;
        // MIS tables on the device; aggregates with arbitration are sequential by definition and stay on the host, which
        // is also the fallback after a hash collision
        PhaseTimer tmis(mis_stream);
        if (!B.aggregates && build_relations_mis_device(L.rel, L.drel, mis_stream)) {
            tmis.lap("    device MIS tables", B.lev);
        } else {
            fetch_relations_ae_host(L.rel, L.drel, mis_stream);
            build_relations_mis(L.rel, B.aggregates ? &B.aggA : nullptr);
            upload_relations_mis(L.drel, L.rel, mis_stream);
        }
        SA_HIP_CHECK(hipStreamSynchronize(mis_stream));
    }), env_serial());
    if (env_serial()) set_thread_stream(s);
    // the operator's SELL copy and smoother data; on a coarse level the operator may still be in the making (deferred
    // Galerkin product of the finer level): then after the eigenproblems, which do not read it
    B.operator_pending = H.galerkin_lev >= 0;
    // (Measured in round 4 and dropped: the fine level's SELL copy and D^-1 -- 13 ms of bandwidth work the setup itself does not
    // need -- on a thread and stream of their own beside the next level: setup 247 -> 243 ms, but the smoother then ran at 221
    // instead of 216 us per step and the step took 399 instead of 390 ms.)
    if (op_early) op_task.join();
    else if (!B.operator_pending) { join_galerkin(H); operator_data(s, L.A, P.opt, true, L.sm); }
    L.sm.roots = sas_poly_roots(L.nu_relax);
}

// ---- stage 2: local spectral problems, chunked over AEs (interp_compute_vectors) ----
// sizes and ownership of the agglomerates, the level's per-agglomerate results cleared
static void eig_stage_begin(LevelBuild &B) {
    Hierarchy &H = B.H; Level &L = B.L; const Params &P = B.P; const Relations &rel = L.rel;
    const int lev = B.lev, nparts = B.nparts, world = B.world;
    // (the sparse rows of the fine AE matrices are kept for the coarse element matrices of the next
    // level when there is one: ~10 bytes per stored entry of the overlapping AE rows)
    B.keep_rows = lev == 0 && lev + 1 < P.num_coarsenings && (double)rel.AE_to_dof.I[nparts] * 30.0 * 10.0 < 32e9;
    std::vector<int> &sizes = B.sizes;
    sizes.resize((size_t)nparts);
    for (int p = 0; p < nparts; ++p) sizes[p] = rel.AE_to_dof.row_size(p);
    L.ae_m.assign((size_t)nparts, 0);
    L.ae_solved = 0;
    if (L.order_info.n != 4) L.order_info.alloc(4);
    L.order_info.zero(B.s);
    L.order_chunks.clear();
    L.ae_class.assign((size_t)nparts, -1);
    L.ae_evclass.assign((size_t)nparts, -1);
    if (P.keep_debug) L.ae_D.alloc((size_t)rel.AE_to_dof.I[nparts]);
    // AE ownership: contiguous ranges balanced by the n^3 cost of the eigenproblems
    B.ae_begin = balanced_ranges(nparts, world, [&](int p) { return (double)sizes[p] * sizes[p] * sizes[p]; });
    if (H.dist_in && lev < (int)H.dist_in->ae_begin.size()) {
        // per-rank inputs: a rank owns the agglomerates made of its own elements (only their element matrices are here)
        const std::vector<long long> &ab = H.dist_in->ae_begin[lev];
        SA_REQUIRE((int)ab.size() == world + 1 && ab[world] == nparts, "per-rank inputs: agglomerate ranges do not match the level");
        for (int r = 0; r <= world; ++r) B.ae_begin[r] = (int)ab[r];
    }
    if (world > 1) {
        SA_REQUIRE(P.allgather != nullptr, "world > 1 needs an all-gather callback");
        SA_REQUIRE(!(P.testmesh && lev == 0), "the mltest fixture is single-rank only");
    }
    B.ae_lo = B.ae_begin[world > 1 ? P.rank : 0];
    B.ae_hi = B.ae_begin[world > 1 ? P.rank + 1 : 1];
    L.ae_begin = B.ae_begin;
    B.dedupe = P.opt.eig_dedupe != 0 && !(P.testmesh && lev == 0);
    // The subspace iteration of a chunk (a few hundred to a few thousand small matrices still active: launches that
    // fill a fraction of the chip, with a host round trip every few iterations) runs on its own thread and stream
    // BESIDE the assembly and the factorisations of the next chunk (Options::overlap bit 0 cleared: one after the other).
    // Only eig_subspace_iterate runs there: it touches its own batch (the other workspace slot) and nothing else;
    // everything that assembles or allocates workspace stays on this thread.
    B.overlap_iter = (P.opt.overlap & 1) && !env_serial() && !profiler().enabled;
    B.iter_stream = B.overlap_iter ? side_stream(3) : B.s;
}
static void eig_start_iterate(LevelBuild &B, int slot) {
    EigBatch &batch = B.batches[slot];
    B.counted[slot] = false;
    if (!B.overlap_iter || !batch.subspace || batch.ss_failed || !batch.count) return;
    B.counted[slot] = true;
    B.iter_task.start(on_gpu(B.dev, B.iter_stream, [&B, slot]() {
        eig_count(B.iter_stream, B.batches[slot], -1.0, B.L.theta);
        SA_HIP_CHECK(hipStreamSynchronize(B.iter_stream));
    }));
}
// the dense path on (re-)assembled matrices: batch b = the agglomerates from ae0 on, whose first row is row0 of the rank's
static void eig_dense_pass(LevelBuild &B, EigBatch &b, int ae0, int64_t row0) {
    const RowsSpan span = rows_span(B.L.rel, ae0, B.ae_lo, B.ae_hi);
    ae_build(B.s, B.L.drel, B.fine_A(), B.L.elmat, ae0, b, true, B.P.keep_debug ? B.L.ae_D.p + row0 : nullptr, B.keep_rows ? &span : nullptr);
    eig_tridiagonalize(B.s, b, 3);
    eig_count(B.s, b, -1.0, B.L.theta);
}
// The few-eigenpairs path finished all but a few matrices of chunk c (bad): those are redone by the dense path, as
// contiguous runs of agglomerates (runs closer than three apart are joined), in the workspace the chunk has just left;
// then the chunk's packed results are put together.  m_all: eigenvector counts of the first pass (0 for the bad ones).
static void eig_redo_bad(LevelBuild &B, int slot, Chunk &c, std::vector<int> m_all, std::vector<char> bad) {
    Level &L = B.L; const Params &P = B.P; hipStream_t s = B.s;
    const int ae0 = c.ae0, cnt = c.count;
    const int *sizes = B.sizes.data() + ae0;
    for (int i = 0; i < cnt; ++i)
        if (bad[i])
            for (int j = i + 1; j < std::min(cnt, i + 4); ++j)
                if (bad[j]) { for (int q = i + 1; q < j; ++q) bad[q] = 1; break; }
    std::vector<Chunk> redo;      // (a run: ae0 = its first agglomerate within the chunk)
    for (int a = 0; a < cnt;) {
        if (!bad[a]) { ++a; continue; }
        int e = a;
        while (e < cnt && bad[e]) ++e;
        redo.emplace_back();
        Chunk &r = redo.back();
        r.ae0 = a;
        r.count = e - a;
        EigBatch sub;
        eig_batch_alloc(sub, std::vector<int>(sizes + a, sizes + e), P.opt, s, slot);
        sub.dense_only = true;
        sub.set_window(L.theta);
        eig_dense_pass(B, sub, ae0 + a, B.pend_row0[slot] + L.rel.AE_to_dof.I[ae0 + a] - L.rel.AE_to_dof.I[ae0]);
        std::copy(sub.h_m.begin(), sub.h_m.begin() + (e - a), m_all.begin() + a);
        packed_offsets(e - a, sub.h_m.data(), sizes + a, r.eoff, r.xoff);
        r.evals.alloc((size_t)r.eoff.back() + 1);
        r.evecs.alloc((size_t)r.xoff.back() + 1);
        r.d_eoff.from_host(r.eoff, s);
        r.d_xoff.from_host(r.xoff, s);
        eig_vectors(s, sub, r.d_eoff.p, r.d_xoff.p, r.evals.p, r.evecs.p);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        a = e;
    }
    // packed results of the whole chunk: stretches of finished matrices from the first pass, the runs from `redo`
    std::vector<int64_t> eoff, xoff;
    std::copy(m_all.begin(), m_all.end(), L.ae_m.begin() + ae0);
    packed_offsets(cnt, m_all.data(), sizes, eoff, xoff);
    DBuf<double> evals((size_t)eoff[cnt]), evecs((size_t)xoff[cnt]);
    auto copy = [&](double *dst, const double *src, int64_t n_) {
        if (n_ > 0) copy_device(dst, src, (size_t)n_, s);
    };
    size_t ri = 0;
    for (int i = 0; i < cnt;) {
        if (ri < redo.size() && redo[ri].ae0 == i) {
            const Chunk &r = redo[ri++];
            copy(evals.p + eoff[i], r.evals.p, r.eoff.back());
            copy(evecs.p + xoff[i], r.evecs.p, r.xoff.back());
            i = r.ae0 + r.count;
        } else {
            const int e = ri < redo.size() ? redo[ri].ae0 : cnt;       // finished matrices i .. e - 1: contiguous in both
            copy(evals.p + eoff[i], c.evals.p + c.eoff[i], c.eoff[e] - c.eoff[i]);
            copy(evecs.p + xoff[i], c.evecs.p + c.xoff[i], c.xoff[e] - c.xoff[i]);
            i = e;
        }
    }
    SA_HIP_CHECK(hipStreamSynchronize(s));
    c.evals = std::move(evals);
    c.evecs = std::move(evecs);
    c.eoff = eoff;
    c.xoff = xoff;
}
// band -> tridiagonal, counts, eigenvectors of the chunk in `slot`
static void eig_chunk_finish(LevelBuild &B, int slot) {
    Level &L = B.L; hipStream_t s = B.s;
    EigBatch &batch = B.batches[slot];
    const int ae0 = B.pend_ae0[slot], cnt = B.pend_cnt[slot];
    const int *sizes = B.sizes.data() + ae0;
    const std::vector<int> &co = B.cls_of[slot];
    bool have = batch.count > 0;      // (with classes: the batch of the NEW classes' representatives, possibly empty)
    if (have && !B.counted[slot]) {
        eig_tridiagonalize(s, batch, 2);
        eig_count(s, batch, -1.0, L.theta);
    }
    if (have && batch.ss_failed && !co.empty()) {      // the new classes go to the dense path, member by member (below)
        for (int id : B.solve_cls[slot]) B.classes.mark_bad(id);
        have = false;
    }
    if (have && batch.ss_failed) {   // few-eigenpairs path gave up on this chunk: dense path on re-assembled matrices
        batch.dense_only = true;
        batch.subspace = batch.ss_failed = false;
        eig_dense_pass(B, batch, ae0, B.pend_row0[slot]);
    }
    B.chunks.emplace_back();
    Chunk &c = B.chunks.back();
    c.ae0 = ae0;
    c.count = cnt;
    // per agglomerate of the chunk: eigenvector count and "redo by the dense path" -- its own, or its class's
    std::vector<int> hm((size_t)cnt);
    std::vector<char> hbad((size_t)cnt, 0);
    bool some_bad = have && batch.subspace && batch.nbad > 0;
    if (!co.empty() && have) {      // the eigenpairs of the classes solved in this chunk, packed; kept for the later members
        const int nr = batch.count;
        std::vector<int64_t> re, rx;
        packed_offsets(nr, batch.h_m.data(), batch.h_n.data(), re, rx);
        B.kept.emplace_back((size_t)re[nr] + 1);
        double *revals = B.kept.back().p;
        B.kept.emplace_back((size_t)rx[nr] + 1);
        double *revecs = B.kept.back().p;
        DBuf<int64_t> d_re, d_rx;
        d_re.from_host(re, s);
        d_rx.from_host(rx, s);
        eig_vectors(s, batch, d_re.p, d_rx.p, revals, revecs);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        for (int r = 0; r < nr; ++r)
            B.classes.set_result(B.solve_cls[slot][r], batch.h_m[r], some_bad && batch.h_bad[r], revals + re[r], revecs + rx[r]);
    }
    some_bad = co.empty() ? some_bad : false;
    for (int i = 0; i < cnt; ++i) {
        if (co.empty()) {
            hm[i] = batch.h_m[i];
            if (some_bad) hbad[i] = batch.h_bad[i];
        } else {
            const LevelClasses::Entry &sc = B.classes[co[i]];
            if (sc.kind == 0) L.ae_class[ae0 + i] = co[i];
            if (!sc.bad) L.ae_evclass[ae0 + i] = co[i];
            hm[i] = sc.bad ? 0 : sc.m;
            hbad[i] = sc.bad ? 1 : 0;
            some_bad = some_bad || sc.bad;
        }
    }
    std::copy(hm.begin(), hm.end(), L.ae_m.begin() + ae0);
    packed_offsets(cnt, hm.data(), sizes, c.eoff, c.xoff);
    c.evals.alloc((size_t)c.eoff[cnt]);
    c.evecs.alloc((size_t)c.xoff[cnt]);
    c.d_eoff.from_host(c.eoff, s);
    c.d_xoff.from_host(c.xoff, s);
    if (co.empty()) {
        eig_vectors(s, batch, c.d_eoff.p, c.d_xoff.p, c.evals.p, c.evecs.p);
    } else {      // a copy of its class's eigenpairs to every agglomerate
        std::vector<const double *> pe((size_t)cnt), px((size_t)cnt);
        for (int i = 0; i < cnt; ++i) { pe[i] = B.classes[co[i]].evals; px[i] = B.classes[co[i]].evecs; }
        DBuf<const double *> d_pe, d_px;
        d_pe.from_host(pe, s);
        d_px.from_host(px, s);
        eig_dedupe_expand(s, cnt, B.sizes.empty() ? 1 : *std::max_element(sizes, sizes + cnt), d_pe.p, d_px.p,
                          c.d_eoff.p, c.d_xoff.p, c.evals.p, c.evecs.p);
    }
    SA_HIP_CHECK(hipStreamSynchronize(s));
    if (some_bad) eig_redo_bad(B, slot, c, hm, hbad);
}
// how many agglomerates from ae0 on make the next chunk: what fits the workspace
static int eig_chunk_count(const LevelBuild &B, int ae0) {
    int cnt = fit_count(ae0, B.ae_hi, B.P.workspace_bytes, [&](int p) { return eig_workspace_bytes(B.sizes[p]); });
    // Large agglomerates (the wide-band path: one workgroup per matrix in the panel and solve kernels, one or two
    // workgroups per CU): a chunk of 577 of them is two full rounds over the 256 CUs and a third at a quarter of
    // the card -- whole multiples of 512 instead (config 5: 27 chunks of 512 instead of 24 of 577).
    constexpr bool round_chunks = true;
    if (round_chunks && cnt > 512 && ae0 + cnt < B.ae_hi && B.sizes[ae0] > 1280) cnt = (cnt / 512) * 512;
    return cnt;
}
// Classes within the chunk in `slot` -- known before its matrices were built (asm_cls: the assembly found them on its inputs)
// or found on the matrices -- against those of the earlier chunks: the batch becomes the batch of the new classes' first members.
static void eig_chunk_classes(LevelBuild &B, int slot, AeClasses &asm_cls) {
    EigBatch &batch = B.batches[slot];
    DdSource src = asm_cls.src;
    bool found = asm_cls.early;
    if (!found && !asm_cls.searched && batch.has_bw) {      // (distinct sparse rows: distinct matrices)
        src = eig_dedupe_source(batch);
        found = eig_dedupe_find(B.s, src, batch.count, batch.max_n, asm_cls.cls, B.P.opt.debug);
    }
    // a level whose first chunk has (almost) no identical agglomerates is not searched further: variable coefficients
    if (!found && B.classes.empty()) B.dedupe_level = false;
    if (!found) return;
    const std::vector<int> solve_list = B.classes.admit(B.s, src, batch.h_n, batch.max_n, asm_cls.cls, B.solve_cls[slot], B.cls_of[slot]);
    B.assembled[slot] = std::move(batch);
    eig_batch_compact(B.s, batch, B.assembled[slot], solve_list);
}
static void level_eigenproblems(LevelBuild &B) {
    Hierarchy &H = B.H; Level &L = B.L; const Params &P = B.P; hipStream_t s = B.s;
    const int lev = B.lev;
    eig_stage_begin(B);
    int64_t row0 = L.rel.AE_to_dof.I[B.ae_lo];      // (rows of the agglomerates before this rank's)
    // (a two-stream pipeline over the chunks -- band reduction of chunk i beside the chase of chunk
    // i-1 -- was measured without gain on MI355X, 256^3: 3.48 s vs 3.29 s, and removed)
    SA_HIP_CHECK(hipStreamSynchronize(s));
    int prev = -1, idx = 0;
    for (int ae0 = B.ae_lo; ae0 < B.ae_hi; ++idx) {
        const int cnt = eig_chunk_count(B, ae0);
        const int slot = idx & 1;
        EigBatch &batch = B.batches[slot];
        batch = EigBatch();
        eig_batch_alloc(batch, std::vector<int>(B.sizes.begin() + ae0, B.sizes.begin() + ae0 + cnt), P.opt, s, slot);
        batch.dense_only = P.eigensolver == 1;
        batch.ss_tol = P.eig_tol;
        batch.set_window(L.theta);
        batch.order_stats = L.order_info.p;
        if (lev > 0 && H.levels[lev - 1]->cvec_next.n == (size_t)L.A.nrows) {
            const size_t rows = (size_t)batch.h_voff[cnt];
            batch.x0c.alloc(rows);
            dev_gather(s, (long)rows, L.drel.ae2d_J.p + L.rel.AE_to_dof.I[ae0], H.levels[lev - 1]->cvec_next.p, batch.x0c.p);
            batch.has_x0c = true;
        }
        const RowsSpan span = rows_span(L.rel, ae0, B.ae_lo, B.ae_hi);
        const bool search = B.dedupe && B.dedupe_level && !batch.dense_only;
        AeClasses asm_cls;
        ae_build(s, L.drel, B.fine_A(), L.elmat, ae0, batch, true, P.keep_debug ? L.ae_D.p + row0 : nullptr,
                 B.keep_rows ? &span : nullptr, search ? &asm_cls : nullptr);
        if (batch.order_ran) L.order_chunks.emplace_back(ae0, cnt);
        const int64_t rows_chunk = batch.h_voff[cnt];
        B.cls_of[slot].clear();
        B.solve_cls[slot].clear();
        if (search) eig_chunk_classes(B, slot, asm_cls);
        if (batch.count) eig_tridiagonalize(s, batch, 1);
        L.ae_solved += batch.count;      // (eigenproblems that are solved, not copied)
        B.pend_ae0[slot] = ae0;
        B.pend_cnt[slot] = cnt;
        B.pend_row0[slot] = row0;
        if (prev >= 0) { B.iter_task.join(); eig_chunk_finish(B, prev); }
        eig_start_iterate(B, slot);
        prev = slot;
        row0 += rows_chunk;
        ae0 += cnt;
    }
    if (prev >= 0) { B.iter_task.join(); eig_chunk_finish(B, prev); }
    B.tm.lap("local eigenproblems", lev);
    if (B.operator_pending) {
        join_galerkin(H);
        operator_data(s, L.A, P.opt, true, L.sm);
        B.tm.lap("operator (deferred Galerkin product) + SELL + D", lev);
    }
}

// Stage 3: the chunks' eigenpairs as the level's arrays; several ranks: counts and eigenvectors all-gathered.
static void level_concatenate(LevelBuild &B) {
    Level &L = B.L; const Params &P = B.P; hipStream_t s = B.s;
    const int lev = B.lev, nparts = B.nparts, world = B.world;
    const std::vector<int> &sizes = B.sizes, &ae_begin = B.ae_begin;
    if (world > 1) {   // exchange the number of eigenvectors per AE
        DBuf<int> d_m;
        d_m.from_host(L.ae_m, s);
        allgather_ranges(P, d_m.p, 4, ae_begin, same_index, "counts");
        auto t_ = d_m.to_host(s);
        L.ae_m.assign(t_.begin(), t_.end());
    }
    // concatenate (+ the mltest fixture's extra all-ones vector on AE 0 of the finest level)
    const bool extra = (P.testmesh && lev == 0);
    L.ae_xoff.assign((size_t)nparts + 1, 0);
    L.ae_eoff.assign((size_t)nparts + 1, 0);
    std::vector<int> m_tot = L.ae_m;
    if (extra) m_tot[0] += 1;
    for (int p = 0; p < nparts; ++p) {
        L.ae_xoff[p + 1] = L.ae_xoff[p] + (int64_t)m_tot[p] * sizes[p];
        L.ae_eoff[p + 1] = L.ae_eoff[p] + L.ae_m[p];
    }
    L.evals.alloc((size_t)L.ae_eoff[nparts]);
    L.evecs.alloc((size_t)L.ae_xoff[nparts]);
    for (Chunk &c : B.chunks) {
        copy_device(L.evals.p + L.ae_eoff[c.ae0], (const double *)c.evals.p, c.evals.n, s);
        if (extra && c.ae0 == 0) {
            const int64_t first = (int64_t)L.ae_m[0] * sizes[0];
            copy_device(L.evecs.p, (const double *)c.evecs.p, (size_t)first, s);
            dev_fill(s, (long)sizes[0], 1.0, L.evecs.p + first);
            if (c.evecs.n > (size_t)first)
                copy_device(L.evecs.p + L.ae_xoff[1], (const double *)c.evecs.p + first, c.evecs.n - (size_t)first, s);
        } else {
            copy_device(L.evecs.p + L.ae_xoff[c.ae0], (const double *)c.evecs.p, c.evecs.n, s);
        }
    }
    SA_HIP_CHECK(hipStreamSynchronize(s));
    B.chunks.clear();
    L.ae_m = m_tot;
    if (world > 1) {   // all-gather the eigenvectors (and, for inspection, eigenvalues and D) in place
        allgather_ranges(P, L.evecs.p, 8, ae_begin, [&](int p) { return L.ae_xoff[p]; }, "eigenvectors");
        if (P.keep_debug) {
            allgather_ranges(P, L.evals.p, 8, ae_begin, [&](int p) { return L.ae_eoff[p]; }, "eigenvalues");
            allgather_ranges(P, L.ae_D.p, 8, ae_begin, [&](int p) { return L.rel.AE_to_dof.I[p]; }, "D");      // (rows before agglomerate p)
        }
        B.tm.lap("all-gather eigenvectors", lev);
    }
}

// Stage 4: the MIS stage (ContribTent::contrib_mises): gather the eigenvectors on every MIS, SVD.
static void level_mis_svd(LevelBuild &B) {
    Level &L = B.L; const Params &P = B.P; const Relations &rel = L.rel; hipStream_t s = B.s;
    const int lev = B.lev, world = B.world;
    B.mis_task.join();
    B.tm.lap("MIS tables (join)", lev);
    const int nm = rel.num_mises;
    std::vector<int64_t> g_off((size_t)nm + 1, 0);
    L.mis_u_off.assign((size_t)nm + 1, 0);
    L.mis_s_off.assign((size_t)nm + 1, 0);
    int max_ctot = 0;
    const int nextra = (lev == 0 && P.extra_modes) ? P.num_extra_modes : 0;
    if (nextra) L.extra = DevIn<double>(P.extra_modes, (size_t)nextra * L.A.nrows, s).take();
    for (int m = 0; m < nm; ++m) {
        int ctot = nextra;
        for (int q = rel.mis_to_AE.I[m]; q < rel.mis_to_AE.I[m + 1]; ++q) ctot += L.ae_m[rel.mis_to_AE.J[q]];
        const int r = rel.mis_to_dof.row_size(m);
        g_off[m + 1] = g_off[m] + (int64_t)r * ctot;
        L.mis_u_off[m + 1] = L.mis_u_off[m] + (int64_t)r * std::max(1, std::min(r, ctot));
        L.mis_s_off[m + 1] = L.mis_s_off[m] + ctot;
        max_ctot = std::max(max_ctot, ctot);
    }
    L.mis_U.alloc((size_t)L.mis_u_off[nm]);
    L.mis_sig.alloc((size_t)L.mis_s_off[nm] + 1);
    L.mis_sig.zero(s);
    L.d_mis_k.alloc((size_t)nm);
    {
        double *gather = scratch_get(1, (size_t)g_off[nm] + 1);
        DBuf<int64_t> d_goff, d_soff, d_xoff;
        DBuf<int> d_aem, d_ncols((size_t)nm);
        d_goff.from_host(g_off, s);
        d_soff.from_host(L.mis_s_off, s);
        L.d_mis_u_off.from_host(L.mis_u_off, s);
        d_xoff.from_host(L.ae_xoff, s);
        d_aem.from_host(L.ae_m, s);
        MisSvdIO io;
        io.ae_m = d_aem.p; io.ae_xoff = d_xoff.p; io.evecs = L.evecs.p;
        io.g_off = d_goff.p; io.gather = gather;
        io.u_off = L.d_mis_u_off.p; io.s_off = d_soff.p; io.U = L.mis_U.p; io.sig = L.mis_sig.p;
        io.k = L.d_mis_k.p; io.ncols = d_ncols.p;
        io.avoid_ess = P.avoid_ess_bdr_dofs; io.extra = nextra ? L.extra.p : nullptr; io.nextra = nextra;
        io.ND = L.A.nrows; io.debug = P.opt.debug;
        if (world > 1) {
            // every rank takes a contiguous range of MISes (balanced by the r c^2 cost of the SVDs) and the bases,
            // singular values and counts are all-gathered in place: the counterpart of the reference's
            // owner-computes SVD + broadcast (SharedEntityCommunication, amg/src/contrib.cpp:519-548)
            const std::vector<int> mb = balanced_ranges(nm, world, [&](int m) {
                const double r = rel.mis_to_dof.row_size(m), c = (double)(L.mis_s_off[m + 1] - L.mis_s_off[m]);
                return r * std::min(r, c) * std::max(r, c) + 64.0;
            });
            L.d_mis_k.zero(s);
            d_ncols.zero(s);
            mis_svd(s, L.drel, mb[P.rank + 1] - mb[P.rank], max_ctot, io, mb[P.rank]);
            allgather_ranges(P, L.mis_U.p, 8, mb, [&](int m) { return L.mis_u_off[m]; }, "MIS bases");
            allgather_ranges(P, L.mis_sig.p, 8, mb, [&](int m) { return L.mis_s_off[m]; }, "singular values");
            allgather_ranges(P, L.d_mis_k.p, 4, mb, same_index, "MIS counts");
            allgather_ranges(P, d_ncols.p, 4, mb, same_index, "MIS columns");
        } else {
            // (agglomerates that hold copies of one class's eigenpairs: MISes with identical inputs are decomposed once)
            DBuf<int> d_ev;
            bool any = false;
            for (int v_ : L.ae_evclass) any = any || v_ >= 0;
            if (any && B.dedupe) d_ev.from_host(L.ae_evclass, s);
            mis_svd(s, L.drel, nm, max_ctot, io, 0, d_ev.n ? d_ev.p : nullptr);
        }
        { auto t_ = L.d_mis_k.to_host(s); L.mis_k.assign(t_.begin(), t_.end()); }
        { auto t_ = d_ncols.to_host(s); L.mis_ncols.assign(t_.begin(), t_.end()); }
    }
    B.tm.lap("MIS gather + SVD", lev);
}

// Stage 5: P and R, the host half of the next level's inputs, the Galerkin product (deferred where it can run beside the next level).
static void level_transfer(LevelBuild &B) {
    Hierarchy &H = B.H; Level &L = B.L; const Params &P = B.P; const Relations &rel = L.rel; hipStream_t s = B.s;
    const int lev = B.lev, dev = B.dev, nm = rel.num_mises;
    L.mis_coloff.assign((size_t)nm + 1, 0);
    for (int m = 0; m < nm; ++m) L.mis_coloff[m + 1] = L.mis_coloff[m] + L.mis_k[m];
    L.d_mis_coloff.from_host(L.mis_coloff, s);
    build_P_R(s, L.drel, rel, L.mis_k, L.d_mis_k.p, L.d_mis_coloff.p, L.d_mis_u_off.p, L.mis_U.p, L.P, L.R);
    if (lev + 1 < P.num_coarsenings) {     // the next level's representation of the constant vector (P^T P = I)
        L.cvec_next.alloc((size_t)L.R.nrows);
        const double *cv = nullptr;
        DBuf<double> ones;
        if (lev > 0 && H.levels[lev - 1]->cvec_next.n == (size_t)L.A.nrows) cv = H.levels[lev - 1]->cvec_next.p;
        else {
            ones.alloc((size_t)L.A.nrows);
            dev_fill(s, (long)L.A.nrows, 1.0, ones.p);
            cv = ones.p;
        }
        spmv(s, L.R, cv, L.cvec_next.p);
        SA_HIP_CHECK(hipStreamSynchronize(s));
    }
    // The next level's element lists from the tentative P.  Device build first (~1 ms on the main stream); its fallback for AEs with
    // more coarse dofs than the kernel's LDS holds is the host half, on a thread and stream of its own beside the Galerkin product.
    // With a smoothed prolongator level_galerkin moves P, so both are left to prepare_next_level.
    SideTask prep_task;
    const bool tent_next = lev + 1 < P.num_coarsenings && P.nu_pro[lev] == 0;
    if (tent_next) {
        NextPrep &np = L.next_prep;
        np.ready = np.on_device = coarse_e2d_device(s, L.drel, rel, L.d_mis_k.p, L.d_mis_coloff.p, L.mis_coloff.back(),
                                                    L.P.rowptr.p, L.P.val.p, np.d_colpos_ptr, np.d_colpos, np.e2d);
    }
    if (tent_next && !L.next_prep.ready) {
        hipStream_t side = side_stream(1);
        SA_HIP_CHECK(hipStreamSynchronize(s));       // P is complete
        prep_task.start(on_gpu(dev, side, [&L, prp = L.P.rowptr.p, pvl = L.P.val.p, pnr = L.P.nrows, pnz = L.P.nnz, sd = side]() {
            prepare_next_host(L, prp, pvl, pnr, pnz, sd, L.next_prep);
            SA_HIP_CHECK(hipStreamSynchronize(sd));      // nothing of this thread is in flight after the join
        }));
    }
    // With another spectral level to come the product runs beside that level's element matrices and
    // eigenproblems (they need its size only); Options::overlap bit 2 cleared and the profiled step keep it in line.
    const bool defer = tent_next && B.world == 1 && (P.opt.overlap & 4) && !env_serial() && !profiler().enabled;
    if (defer) {
        SA_HIP_CHECK(hipStreamSynchronize(s));       // the operands are complete
        hipStream_t gs = side_stream(2);
        H.galerkin_lev = lev;
        H.galerkin_task.start(on_gpu(dev, gs, [&H, lev, gs]() {
            level_galerkin(H, lev, true, gs);
            SA_HIP_CHECK(hipStreamSynchronize(gs));
        }));
    } else {
        level_galerkin(H, lev, true, s);
    }
    prep_task.join();
    B.tm.lap(defer ? "P, R (RAP deferred)" : "P, R, RAP", lev);
}

static void build_level(Hierarchy &H, int lev, Table &&e2d, const hvec<int> &part, int nparts,
                        const signed char *bdr_host, const DeviceInputs *din = nullptr) {
    SA_REQUIRE(H.params.nu_pro[lev] >= 0 && H.params.nu_pro[lev] <= 8, "bad prolongator smoothing degree");
    LevelBuild B(H, lev, nparts);
    Level &L = B.L;
    L.theta = B.P.theta[lev];
    L.nu_relax = B.P.nu_relax[lev];
    level_topology(B, std::move(e2d), part, bdr_host, din);
    level_eigenproblems(B);
    level_concatenate(B);
    level_mis_svd(B);
    level_transfer(B);
    if (!B.P.keep_debug) {
        L.evals.release();
        L.evecs.release();
        L.mis_sig.release();
    }
    // work vectors
    const size_t n = (size_t)L.A.nrows;
    L.x.alloc(n); L.b.alloc(n); L.r.alloc(n); L.sm.tmp.alloc(n);
}

// ---------------------------------------------------------------------------------------
// next level's inputs: coarse elements = AEs, coarse element matrices = P_loc^T A_e P_loc
// (agg_create_partitioning_coarse / elmat_parallel)
// ---------------------------------------------------------------------------------------
// Host half of the next level's inputs (everything that needs only the topology, the MIS sizes
// and the numerically non-zero pattern of the tentative prolongator).  Runs on its own thread
// and stream beside the Galerkin product when the prolongator is not smoothed.
static void prepare_next_host(const Level &L, const roff_t *p_rowptr_dev, const double *p_val_dev, int p_nrows,
                              int64_t p_nnz, hipStream_t s, NextPrep &out) {
    fetch_relations_ae_host(const_cast<Relations &>(L.rel), L.drel, s);
    const Relations &rel = L.rel;
    const int nparts = rel.nparts;
    // coarse elem_to_dof = AE_to_dof x pattern(P_tent), first-encounter order
    // (agg_create_rels_except_elem_coarse, amg/src/aggregates.cpp:1510-1514).  The pattern is
    // the *numerically non-zero* entries of P_tent (contrib_tent_insert_simple drops exact
    // zeros, amg/src/contrib.cpp:186-187), so P's values are inspected on the host.
    Table &e2d = out.e2d;
    e2d.ncols = L.mis_coloff.back();
    e2d.I.assign((size_t)nparts + 1, 0);
    hvec<roff_t> p_rowptr;
    hvec<double> p_val;
    download(p_rowptr, p_rowptr_dev, (size_t)p_nrows + 1, s);
    download(p_val, p_val_dev, (size_t)p_nnz, s);
    SA_HIP_CHECK(hipStreamSynchronize(s));
    // colpos: for every (AE, MIS) incidence (aligned with AE_to_mis.J) the position of each of
    // the MIS's coarse dofs in the coarse element's dof list
    std::vector<int> &colpos_ptr = out.colpos_ptr;
    colpos_ptr.assign(rel.AE_to_mis.J.size() + 1, 0);
    for (int e = 0; e < nparts; ++e)
        for (int t = rel.AE_to_mis.I[e]; t < rel.AE_to_mis.I[e + 1]; ++t)
            colpos_ptr[(size_t)t + 1] = colpos_ptr[t] + L.mis_k[rel.AE_to_mis.J[t]];
    std::vector<int> &colpos = out.colpos;
    colpos.assign((size_t)colpos_ptr.back(), -1);
    // two passes over the AEs (count, then fill), both split over host threads
    {
        int T = (int)SideTask::hardware_threads();
        if (T < 1) T = 1;
        if (T > 16) T = 16;
        if (nparts < 64) T = 1;
        auto walk = [&](int e, std::vector<int> &stamp, int *dst, bool fill) -> int {
            int run = 0;
            const int *misrow = rel.AE_to_mis.row(e);
            const int nmis = rel.AE_to_mis.row_size(e);
            for (int k = rel.AE_to_dof.I[e]; k < rel.AE_to_dof.I[e + 1]; ++k) {
                const int dof = rel.AE_to_dof.J[k];
                const int m = rel.mises[dof];
                const int km = L.mis_k[m];
                if (km == 0) continue;
                const int t = rel.AE_to_mis.I[e] + (int)(std::lower_bound(misrow, misrow + nmis, m) - misrow);
                for (int v = 0; v < km; ++v) {
                    const int cd = L.mis_coloff[m] + v;
                    if (stamp[cd] == e) continue;
                    if (p_val[(size_t)p_rowptr[dof] + v] == 0.0) continue;
                    stamp[cd] = e;
                    if (fill) {
                        colpos[(size_t)colpos_ptr[t] + v] = run;
                        dst[run] = cd;
                    }
                    ++run;
                }
            }
            return run;
        };
        const int dev = current_device();
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<SideTask> th((size_t)T);
            for (int t = 0; t < T; ++t)
                th[(size_t)t].start([&, t, pass]() {
                    (void)hipSetDevice(dev);
                    std::vector<int> stamp((size_t)e2d.ncols, -1);
                    const int eb = (int)((int64_t)nparts * t / T), ee = (int)((int64_t)nparts * (t + 1) / T);
                    for (int e = eb; e < ee; ++e) {
                        if (pass == 0) e2d.I[e + 1] = walk(e, stamp, nullptr, false);
                        else walk(e, stamp, e2d.J.data() + e2d.I[e], true);
                    }
                });
            for (auto &x : th) x.join();
            if (pass == 0) {
                for (int e = 0; e < nparts; ++e) e2d.I[e + 1] += e2d.I[e];
                e2d.J.resize((size_t)e2d.I[nparts]);
            }
        }
    }
    out.ready = true;
}

static Table prepare_next_level(Hierarchy &H, int lev) {
    Level &L = *H.levels[lev];
    hipStream_t s = H.stream;
    const Relations &rel = L.rel;
    const int nparts = rel.nparts;
    if (!L.next_prep.ready) {
        // (always the TENTATIVE prolongator: the coarse elements are built from mis_tent_interps)
        const DCsr &PT = L.Ptent.nrows ? L.Ptent : L.P;
        NextPrep &np = L.next_prep;
        np.on_device = coarse_e2d_device(s, L.drel, rel, L.d_mis_k.p, L.d_mis_coloff.p, L.mis_coloff.back(),
                                         PT.rowptr.p, PT.val.p, np.d_colpos_ptr, np.d_colpos, np.e2d);
        if (!np.on_device) prepare_next_host(L, PT.rowptr.p, PT.val.p, PT.nrows, PT.nnz, s, L.next_prep);
    }
    Table e2d = std::move(L.next_prep.e2d);
    DBuf<int> d_colpos_ptr, d_colpos;
    if (L.next_prep.on_device) {
        d_colpos_ptr = std::move(L.next_prep.d_colpos_ptr);
        d_colpos = std::move(L.next_prep.d_colpos);
    } else {
        for (int v : L.next_prep.colpos) SA_REQUIRE(v >= 0, "coarse dof with an all-zero prolongator column in an AE");
        d_colpos_ptr.from_host(L.next_prep.colpos_ptr, s);
        d_colpos.from_host(L.next_prep.colpos, s);
    }
    L.next_prep = NextPrep();
    // coarse element matrices
    Level &N = *H.levels[lev + 1];
    std::vector<int64_t> out_off((size_t)nparts + 1, 0);
    for (int e = 0; e < nparts; ++e) {
        const int64_t ke = e2d.row_size(e);
        out_off[e + 1] = out_off[e] + ke * ke;
    }
    N.elmat.off.from_host(out_off, s);
    N.elmat.val.alloc((size_t)out_off[nparts] + 1);
    // The next level's AE tables are a HOST build (7.8 ms on the headline's level 1).  Its inputs are complete here -- the coarse
    // element lists just made, the caller's partition -- and nothing below needs its result: it runs on a thread of its own
    // beside the coarse element matrices (20 ms of device work during which this thread only waits).
    SideTask topo_task;
    if (lev + 1 < H.params.num_coarsenings && lev + 1 < (int)H.coarse_parts.size() && !H.coarse_parts[(size_t)lev + 1].empty() &&
        !env_serial()) {
        const int dev = current_device();
        const int nd_next = L.mis_coloff.back(), np_next = H.nparts_in[(size_t)lev + 1];
        const hvec<int> *part_next = &H.coarse_parts[(size_t)lev + 1];
        topo_task.start([&N, own = Table(e2d), part_next, nd_next, np_next, dev]() mutable {      // (host work only: no stream)
            adopt_device(dev);
            build_relations_ae(N.rel, std::move(own), *part_next, np_next, nd_next, nullptr);
            N.rel_prebuilt = true;
        });
    }
    std::vector<int> sizes((size_t)nparts);
    for (int p = 0; p < nparts; ++p) sizes[p] = rel.AE_to_dof.row_size(p);
    // several ranks: each computes the coarse element matrices of its AE range (the ranges of
    // the eigenproblems), then one in-place all-gather
    const int world = H.params.world > 1 ? H.params.world : 1;
    const int ae_lo = world > 1 ? L.ae_begin[H.params.rank] : 0;
    const int ae_hi = world > 1 ? L.ae_begin[H.params.rank + 1] : nparts;
    DBuf<int> d_ae_class;
    for (int ae0 = ae_lo; ae0 < ae_hi;) {
        const int cnt = fit_count(ae0, ae_hi, H.params.workspace_bytes, [&](int p) {
            const size_t n = (size_t)sizes[p];
            return 8 * (n * n + n * (EIG_NB + 8) + n * (size_t)e2d.row_size(p));
        });
        EigBatch batch;
        eig_batch_alloc(batch, std::vector<int>(sizes.begin() + ae0, sizes.begin() + ae0 + cnt), H.params.opt, s);
        std::vector<int64_t> soff((size_t)cnt + 1, 0);
        for (int i = 0; i < cnt; ++i) soff[i + 1] = soff[i] + (int64_t)sizes[ae0 + i] * e2d.row_size(ae0 + i);
        DBuf<int64_t> d_soff;
        d_soff.from_host(soff, s);
        double *scratch = scratch_get(0, (size_t)soff[cnt] + 1);
        int RW = 0;
        const double *rv = nullptr;
        const short *rc = nullptr;
        const RowsSpan span = rows_span(rel, ae0, ae_lo, ae_hi);
        if (lev == 0 && ae_sparse_rows(s, L.drel, L.A, L.elmat, ae0, batch, RW, rv, rc, &span)) {
            // fine level: straight from the sparse rows of the AE matrices
            int kmax = 0;
            for (int km : L.mis_k) kmax = std::max(kmax, km);
            // (classes of the agglomerates' sparse rows, where the eigenproblem stage found them for every agglomerate of the range)
            bool have_classes = H.params.opt.eig_dedupe != 0 && (int)L.ae_class.size() == nparts;
            for (int i = ae0; have_classes && i < ae0 + cnt; ++i) have_classes = L.ae_class[i] >= 0;
            if (have_classes && !d_ae_class.n) d_ae_class.from_host(L.ae_class, s);
            coarse_elmats_sparse(s, L.drel, ae0, batch, RW, rv, rc, L.d_mis_k.p, L.d_mis_u_off.p, L.mis_U.p,
                                 d_colpos_ptr.p, d_colpos.p, N.elmat.off.p, N.elmat.val.p, scratch, d_soff.p, kmax,
                                 have_classes ? d_ae_class.p : nullptr);
        } else {
            ae_build(s, L.drel, lev == 0 ? &L.A : nullptr, L.elmat, ae0, batch, false, nullptr);
            coarse_elmats(s, L.drel, ae0, batch, L.d_mis_k.p, L.d_mis_u_off.p, L.mis_U.p, d_colpos_ptr.p,
                          d_colpos.p, N.elmat.off.p, N.elmat.val.p, scratch, d_soff.p);
        }
        // (single rank, last chunk: no wait -- everything that reads the element matrices follows on this stream,
        // the buffers released here are stream-ordered, and the host goes on to the next level's topology while
        // the kernel runs)
        if (world > 1 || ae0 + cnt < ae_hi) SA_HIP_CHECK(hipStreamSynchronize(s));
        ae0 += cnt;
    }
    if (world > 1) allgather_ranges(H.params, N.elmat.val.p, 8, L.ae_begin, [&](int p) { return out_off[p]; }, "coarse element matrices");
    topo_task.join();
    return e2d;
}

// ---------------------------------------------------------------------------------------
// corrected null-space level (CorrectNullspace, amg/src/solve.cpp:52-164, configured by
// amg/src/ml.cpp:225-236): one more two-grid level under the coarsest spectral operator.
// interp = scaling_P (amg/src/contrib.cpp:655-668, amg/src/interp.cpp:842-909): one column per
// MIS that has coarse dofs, holding the normalised coefficients of the constant vector in the
// MIS's orthonormal basis (x = U^T 1 / |U^T 1|).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void scaling_p_kernel(const int *__restrict__ mis2d_I, const int *__restrict__ k,
                                                       const int *__restrict__ coloff,
                                                       const int64_t *__restrict__ u_off,
                                                       const double *__restrict__ U,
                                                       const int *__restrict__ active, roff_t *__restrict__ prow,
                                                       int *__restrict__ pcol, double *__restrict__ pval) {
    extern __shared__ double xs[];
    const int m = blockIdx.x, lane = threadIdx.x;
    const int km = k[m];
    if (km == 0) return;
    const int r = mis2d_I[m + 1] - mis2d_I[m];
    const double *Um = U + u_off[m];
    double nn = 0.0;
    for (int v = 0; v < km; ++v) {
        double sum = 0.0;
        for (int i = lane; i < r; i += 64) sum += Um[(size_t)v * r + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) xs[v] = sum;
        nn = fma(sum, sum, nn);
    }
    __syncthreads();
    const double inv = 1.0 / sqrt(nn);
    for (int v = lane; v < km; v += 64) {
        const int row = coloff[m] + v;
        prow[row] = row;
        pcol[row] = active[m];
        pval[row] = xs[v] * inv;
    }
}

static void add_nullspace_level(Hierarchy &H) {
    hipStream_t s = H.stream;
    Level &L = *H.levels.back();
    const int nm = L.rel.num_mises;
    const int nc = L.Ac.nrows;
    SA_REQUIRE(!H.params.testmesh, "the corrected null-space level is not available with the mltest fixture vectors");
    std::vector<int> active((size_t)nm, -1);
    int nact = 0, kmax = 1;
    for (int m = 0; m < nm; ++m)
        if (L.mis_k[m] > 0) { active[m] = nact++; kmax = std::max(kmax, L.mis_k[m]); }
    H.levels.emplace_back(new Level);
    Level &N = *H.levels.back();
    N.A = std::move(L.Ac);
    N.theta = 0.0;
    N.nu_relax = 3;
    N.sm.roots = sas_poly_roots(3);
    operator_data(s, N.A, H.params.opt, false, N.sm);
    N.P.nrows = nc;
    N.P.ncols = nact;
    N.P.nnz = nc;
    N.P.rowptr.alloc((size_t)nc + 1);
    N.P.col.alloc((size_t)nc + 1);
    N.P.val.alloc((size_t)nc + 1);
    DBuf<int> d_active;
    d_active.from_host(active, s);
    hipLaunchKernelGGL(scaling_p_kernel, dim3(nm), dim3(64), sizeof(double) * (size_t)kmax, s, L.drel.mis2d_I.p,
                       L.d_mis_k.p, L.d_mis_coloff.p, L.d_mis_u_off.p, L.mis_U.p, d_active.p, N.P.rowptr.p,
                       N.P.col.p, N.P.val.p);
    SA_HIP_CHECK(hipGetLastError());
    const roff_t nc_off = nc;
    upload_async(N.P.rowptr.p + nc, &nc_off, 1, s);
    SA_HIP_CHECK(hipStreamSynchronize(s));
    N.P.lanes_per_row = 1;
    csr_transpose(s, N.P, N.R);
    galerkin_general(s, N.A, N.P, N.R, N.Ac);
    N.rel.ND = nc;
    N.rel.nparts = nact;
    N.x.alloc((size_t)nc); N.b.alloc((size_t)nc); N.r.alloc((size_t)nc); N.sm.tmp.alloc((size_t)nc);
}

// ---------------------------------------------------------------------------------------
// ml_produce_data
// ---------------------------------------------------------------------------------------
Hierarchy *hierarchy_create(int n, const void *Arow, int rowptr_bits, const int *Acol, const double *Aval, int NE,
                            int nde, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                            const signed char *bdr, const int *const *partitions,
                            const int *nparts, const Params &p, hipStream_t stream, std::unique_ptr<DistIn> dist_inputs) {
    SA_REQUIRE(p.num_coarsenings >= 1 && p.num_coarsenings < MAX_LEVELS, "bad number of coarsenings");
    ae_rows_new_build();     // nothing cached from an earlier hierarchy is reused
    // element-free mode: elements = dofs (identity elem_to_dof generated here), no element matrices
    DBuf<int> iota_e2d;   // (moved into the hierarchy below: the device topology views it)
    if (p.algebraic) {
        NE = n;
        nde = 1;
        iota_e2d.alloc((size_t)n);
        dev_iota(stream, (long)n, 1, iota_e2d.p);
        elem_to_dof = iota_e2d.p;
        elmat = nullptr;
        bdr = nullptr;
    }
    int max_nd = 0;
    if (elem_ptr) {       // mixed entries: checked here; elements of one size take the path of the uniform entries from here on
        SA_REQUIRE(!p.algebraic && !dist_inputs && elem_to_dof && elmat, "elem_ptr needs element arrays");
        SA_REQUIRE(n > 0 && NE > 0, "empty problem");
        nde = check_elem_ptr(NE, elem_ptr, elem_to_dof, n, max_nd, stream);
        if (nde) elem_ptr = nullptr;
    }
    SA_REQUIRE(n > 0 && NE > 0 && (nde > 0 || elem_ptr), "empty problem");
    PhaseTimer tm_all(stream), tm0(stream);
    std::unique_ptr<Hierarchy> Hp(new Hierarchy);
    Hierarchy &H = *Hp;
    H.params = p;
    H.stream = stream;
    H.device = current_device();
    H.own_e2d = std::move(iota_e2d);
    H.dist_in = std::move(dist_inputs);
    hipStream_t s = stream;
    H.scal.alloc(8);
    H.partials.alloc(1024);
    for (int l = 0; l < p.num_coarsenings; ++l) H.levels.emplace_back(new Level);
    // level 0 inputs
    Level &L0 = *H.levels[0];
    {
        import_rowptr(L0.A.rowptr, Arow, rowptr_bits, (size_t)n + 1, s);
        roff_t nnz = read_one(L0.A.rowptr.p + n, s);
        L0.A.nrows = L0.A.ncols = n;
        L0.A.nnz = nnz;
        L0.A.col = DevIn<int>(Acol, (size_t)nnz, s).take();
        L0.A.val = DevIn<double>(Aval, (size_t)nnz, s).take();
        finish_csr(L0.A);
    }
    {
        L0.elmat.off.alloc((size_t)NE + 1);
        if (H.dist_in) {
            // per-rank inputs: only the matrices of the rank's own elements exist (they are never exchanged); the offsets of
            // the other elements stay 0 -- no kernel of this rank touches an agglomerate made of them
            L0.elmat.off.zero(s);
            dev_iota(s, (long)H.dist_in->NE_loc + 1, (int64_t)nde * nde, L0.elmat.off.p + H.dist_in->elem0);
            L0.elmat.val = DevIn<double>(elmat, (size_t)H.dist_in->NE_loc * nde * nde, s).take();
            L0.elmat.first = H.dist_in->elem0;
        } else if (elem_ptr) {
            // mixed elements: element e's matrix at sum_{f<e} nd_f^2
            H.e2d_ptr = DevIn<int>(elem_ptr, (size_t)NE + 1, s).take();
            DBuf<int> sq((size_t)NE);
            hipLaunchKernelGGL(elem_sq_kernel, dim3(div_up((long)NE, 256)), dim3(256), 0, s, (long)NE, H.e2d_ptr.p, sq.p);
            SA_HIP_CHECK(hipGetLastError());
            exclusive_scan_off(s, NE, sq.p, L0.elmat.off.p);
            int64_t total = read_one(L0.elmat.off.p + NE, s);
            L0.elmat.val = DevIn<double>(elmat, (size_t)total, s).take();
            L0.elmat.max_nd = max_nd;
        } else {
        dev_iota(s, (long)NE + 1, (int64_t)nde * nde, L0.elmat.off.p);
        if (!p.algebraic) L0.elmat.val = DevIn<double>(elmat, (size_t)NE * nde * nde, s).take();
        }
        L0.elmat.nde = nde;
        L0.elmat.algebraic = p.algebraic;
    }
    // Level-0 topology inputs that are device-resident stay there (device build of the AE tables); host inputs take the host build
    DeviceInputs din;
    const bool dev_inputs = is_device_ptr(elem_to_dof) && is_device_ptr(partitions[0]) &&
                            (!bdr || is_device_ptr(bdr));
    Table e2d;
    hvec<signed char> bdr_h;
    if (dev_inputs) {
        din.e2d = elem_to_dof;
        din.part = partitions[0];
        din.bdr = bdr;
        din.NE = NE;
        din.nde = nde;
        din.e2d_I = elem_ptr ? H.e2d_ptr.p : nullptr;
    } else if (elem_ptr) {
        e2d.I = fetch_host(H.e2d_ptr.p, (size_t)NE + 1, s);
        e2d.J = fetch_host(elem_to_dof, (size_t)e2d.I[NE], s);
        e2d.ncols = n;
        if (bdr) bdr_h = fetch_host(bdr, (size_t)n, s);
    } else {
        auto J = fetch_host(elem_to_dof, (size_t)NE * nde, s);
        e2d.J = std::move(J);
        e2d.I.resize((size_t)NE + 1);
        for (int e = 0; e <= NE; ++e) e2d.I[e] = e * nde;
        e2d.ncols = n;
        if (bdr) bdr_h = fetch_host(bdr, (size_t)n, s);
    }
    H.coarse_parts.resize((size_t)p.num_coarsenings);
    H.nparts_in.assign(nparts, nparts + p.num_coarsenings);
    {
        int ne = nparts[0];
        for (int lev = 1; lev < p.num_coarsenings; ++lev) {       // (level-lev elements = level-(lev - 1) agglomerates)
            H.coarse_parts[(size_t)lev] = fetch_host(partitions[lev], (size_t)ne, s);
            ne = nparts[lev];
        }
    }
    tm0.lap("inputs fetched/imported", 0);
    int n_elem = NE;
    for (int lev = 0; lev < p.num_coarsenings; ++lev) {
        hvec<int> part;
        if (lev > 0) part = H.coarse_parts[(size_t)lev];
        else if (!dev_inputs) part = fetch_host(partitions[lev], (size_t)n_elem, s);
        const bool tag_levels = (H.params.opt.debug & 4) != 0;
        profiler().level_tag = tag_levels ? lev : 0;
        build_level(H, lev, std::move(e2d), part, nparts[lev], (lev == 0 && bdr && !dev_inputs) ? bdr_h.data() : nullptr,
                    (lev == 0 && dev_inputs) ? &din : nullptr);
        Level &L = *H.levels[lev];
        if (lev + 1 < p.num_coarsenings) {
            PhaseTimer tm(s);
            e2d = prepare_next_level(H, lev);
            tm.lap("next-level elements", lev);
            Level &N = *H.levels[lev + 1];
            if (H.galerkin_lev == lev) {       // product still running: the size is known, the arrays follow at the join
                N.A = DCsr();
                N.A.nrows = N.A.ncols = L.mis_coloff.back();
            } else {
                N.A = std::move(L.Ac);  // A_{l+1} = Ac_l  (amg/src/ml.cpp:134)
            }
            n_elem = L.rel.nparts;
        }
    }
    profiler().level_tag = 0;
    join_galerkin(H);
    tm0 = PhaseTimer(s);
    if (p.correct_nullspace) {
        add_nullspace_level(H);
        tm0.lap("corrected null-space level", 0);
    }
    setup_coarse_solver(H);
    H.pcg.alloc((size_t)n);
    H.pcg.sc = H.scal.p;
    SA_HIP_CHECK(hipStreamSynchronize(s));
    tm0.lap("coarse solver + vectors", 0);
    if (p.world > 1 && p.alltoallv) {
        for (int lev = 0; lev < p.num_coarsenings; ++lev)
            if (!dist_setup_level(H, lev)) break;
        tm0.lap("row-partitioned solve: halo lists", 0);
    }
    tm_all.lap("TOTAL ml_produce_data", 0);
    if (env_timing()) {
        long nm_ = 0, nf_ = 0;
        size_t mb_ = 0;
        dev_pool_counts(&nm_, &nf_, &mb_, true);
        std::fprintf(stderr, "TIMING: device pool: %ld hipMalloc (%.1f MB), %ld hipFree of cached blocks, %.1f GB idle\n", nm_, mb_ / 1048576.0, nf_,
                     dev_pool_idle_bytes() / 1073741824.0);
    }
    return Hp.release();
}

// adapt_update_operators (amg/src/adapt.cpp:171-219): the matrix changed (same sparsity, same topology): keep every
// interpolation (the eigenproblems are NOT solved again), refresh every operator's solve data (operator_data), re-smooth P
// where nu_pro > 0, rebuild all Galerkin operators and the coarsest solver.
void hierarchy_update_operators(Hierarchy &H, const double *new_val) {
    hipStream_t s = H.stream;
    Level &L0 = *H.levels[0];
    if (new_val && new_val != L0.A.val.p) {
        if (is_device_ptr(new_val)) {
            L0.A.val.view(const_cast<double *>(new_val), (size_t)L0.A.nnz);   // device arrays are used in place
        } else {
            if (!L0.A.val.owned) L0.A.val.alloc((size_t)L0.A.nnz);           // never write into the caller's array
            upload(L0.A.val.p, new_val, (size_t)L0.A.nnz, s);
        }
    }
    for (int lev = 0; lev < H.params.num_coarsenings; ++lev) {
        Level &L = *H.levels[lev];
        operator_data(s, L.A, H.params.opt, true, L.sm);
        L.Ac = DCsr();
        level_galerkin(H, lev, false, s);
        if (lev + 1 < (int)H.levels.size()) H.levels[lev + 1]->A = std::move(L.Ac);
    }
    if (H.params.correct_nullspace) {   // the scaling_P level: same interpolation, new operators
        Level &N = *H.levels.back();
        operator_data(s, N.A, H.params.opt, false, N.sm);
        galerkin_general(s, N.A, N.P, N.R, N.Ac);
    }
    setup_coarse_solver(H);
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
