// extern "C" boundary (include/saamge_amd.h).  Exceptions stop here.
#include <cstdlib>
#include "../../include/saamge_amd.h"

#include <cmath>
#include <memory>
#include <string>

#include "blockvec.h"
#include "cycle.h"
#include "elmat.h"
#include "hierarchy.h"
#include "lobpcg.h"
#include "mesh_faces.h"
#include "mesh_lift.h"
#include "mesh_refine.h"
#include "operator.h"
#include "partition.h"
#include "spgemm.h"

using namespace saamge_amd;

struct saamge_amd_hierarchy {
    Hierarchy *H;
};

// saamge_amd_partition_mesh: level k partitions graph k; graph num_levels is the quotient graph of the last level
struct saamge_amd_partitioning {
    int device = 0;
    std::vector<DBuf<int>> part;             // device
    std::vector<hvec<int>> part_host;
    std::vector<const int *> part_ptr, part_host_ptr;
    std::vector<int> n_elem, nparts;
    std::vector<DBuf<roff_t>> xadj;
    std::vector<DBuf<int>> adj;
    std::vector<int64_t> nnz;
};

// saamge_amd_operator_assemble: the assembled operator and the device copies of the mesh tables its numeric pass needs
struct saamge_amd_operator {
    AssembledOperator op;
};
struct saamge_amd_face_table {
    FaceTable t;
};
struct saamge_amd_mesh_lift {
    MeshLift l;
};
struct saamge_amd_refined_mesh {
    MeshRefine r;
};
static OperatorLimits g_operator_limits;     // saamge_amd_operator_set_path_limits (tests)

static std::string g_last_error;

#define SA_API_BEGIN try {
#define SA_API_END                                   \
    }                                                \
    catch (const Error &e) {                         \
        g_last_error = e.what();                     \
        return e.code ? e.code : 1;                  \
    }                                                \
    catch (const std::exception &e) {                \
        g_last_error = e.what();                     \
        return 1;                                    \
    }                                                \
    return 0;

// every call on a hierarchy must come from a thread whose current HIP device is the one the
// hierarchy was built on (HIP's current device is per host thread)
static void require_device(const Hierarchy &H) {
    SA_REQUIRE(current_device() == H.device, "the calling thread's current HIP device is not the hierarchy's device");
    set_thread_stream(H.stream);     // device blocks freed by this call are ordered after the hierarchy's stream
}

// The prologue of every entry point of the element layer and the mesh layer: the call's stream is the thread's while it runs, the
// mesh arguments travel as one, errors become the return code.
template <class F>
static int mesh_call(const MeshArgs &m, void *stream, F call) {
    SA_API_BEGIN
    hipStream_t s = (hipStream_t)stream;
    ThreadStreamScope scope(s);
    call(s, m);
    SA_API_END
}
// mesh_call for an entry point that makes a handle: *out gets the handle once `build` has filled it.  On a refusal *out stays
// unwritten, or (clear) is NULL from the entry on.
template <class H, class F>
static int mesh_handle_call(const char *name, H **out, bool clear, const MeshArgs &m, void *stream, F build) {
    return mesh_call(m, stream, [&](hipStream_t s, const MeshArgs &mm) {
        SA_REQUIRE(out, std::string(name) + ": null argument: out");
        if (clear) *out = nullptr;
        std::unique_ptr<H> P(new H);
        build(s, mm, *P);
        *out = P.release();
    });
}
// what the getters of the mesh handles share
static void require_device(int device, const char *what) {
    SA_REQUIRE(current_device() == device, std::string("the calling thread's current HIP device is not the ") + what + "'s device");
}
// an output of a getter of a handle without a stream (the call that built it has synchronised its own): on the null stream
template <class T>
static void copy_out(void *dst, const DBuf<T> &src) { copy_to_caller((T *)dst, src, (hipStream_t) nullptr); }

extern "C" int saamge_amd_comm_native_stream(const saamge_amd_params *p, void **stream);      // comm.hip

extern "C" {

const char *saamge_amd_last_error(void) { return g_last_error.c_str(); }

static void options_to_c(const Options &o, saamge_amd_options *c) {
    c->eig_strict = o.eig_strict; c->eig_certify = o.eig_certify; c->eig_min_n = o.eig_min_n;
    c->eig_force_fallback = o.eig_force_fallback; c->eig_dense_only = o.eig_dense_only; c->eig_dense_one_stage = o.eig_dense_one_stage;
    c->eig_nullcheck = o.eig_nullcheck; c->eig_keep_inertia_factor = o.eig_keep_inertia_factor; c->band_assembly = o.band_assembly;
    c->eig_dedupe = o.eig_dedupe; c->eig_outer_panels = o.eig_outer_panels; c->overlap = o.overlap; c->sell = o.sell; c->spmv_sell = o.spmv_sell; c->debug = o.debug;
    c->host_heap_pad_mb = o.host_heap_pad_mb;
    c->ae_order = o.ae_order;
}
static Options options_from_c(const saamge_amd_options *c) {
    Options o;
    o.eig_strict = c->eig_strict; o.eig_certify = c->eig_certify; o.eig_min_n = c->eig_min_n;
    o.eig_force_fallback = c->eig_force_fallback; o.eig_dense_only = c->eig_dense_only; o.eig_dense_one_stage = c->eig_dense_one_stage;
    o.eig_nullcheck = c->eig_nullcheck; o.eig_keep_inertia_factor = c->eig_keep_inertia_factor; o.band_assembly = c->band_assembly;
    o.eig_dedupe = c->eig_dedupe; o.eig_outer_panels = c->eig_outer_panels; o.overlap = c->overlap; o.sell = c->sell; o.spmv_sell = c->spmv_sell; o.debug = c->debug;
    o.host_heap_pad_mb = c->host_heap_pad_mb;
    o.ae_order = c->ae_order;
    return o;
}
// Called on the options a hierarchy or a hierarchy-free entry point is about to use.
static void validate_options(const Options &o) {
    auto flag = [](int v) { return v == 0 || v == 1; };
    SA_REQUIRE(flag(o.eig_strict), "options: eig_strict must be 0 or 1");
    SA_REQUIRE(flag(o.eig_certify), "options: eig_certify must be 0 or 1");
    SA_REQUIRE(o.eig_min_n >= 0, "options: eig_min_n must not be negative");
    SA_REQUIRE(o.eig_force_fallback >= 0, "options: eig_force_fallback must not be negative");
    SA_REQUIRE(flag(o.eig_dense_only), "options: eig_dense_only must be 0 or 1");
    SA_REQUIRE(flag(o.eig_dense_one_stage), "options: eig_dense_one_stage must be 0 or 1");
    SA_REQUIRE(flag(o.eig_nullcheck), "options: eig_nullcheck must be 0 or 1");
    SA_REQUIRE(flag(o.eig_keep_inertia_factor), "options: eig_keep_inertia_factor must be 0 or 1");
    SA_REQUIRE(flag(o.band_assembly), "options: band_assembly must be 0 or 1");
    SA_REQUIRE(flag(o.eig_dedupe), "options: eig_dedupe must be 0 or 1");
    SA_REQUIRE(o.eig_outer_panels == 2 || o.eig_outer_panels == 4 || o.eig_outer_panels == 8, "options: eig_outer_panels must be 2, 4 or 8");
    SA_REQUIRE((o.overlap & ~15) == 0, "options: overlap has bits 0-3");
    SA_REQUIRE((o.sell & ~127) == 0, "options: sell has bits 0-6");
    SA_REQUIRE(flag(o.spmv_sell), "options: spmv_sell must be 0 or 1");
    SA_REQUIRE((o.debug & ~7) == 0, "options: debug has bits 0-2");
    SA_REQUIRE(o.host_heap_pad_mb >= 0, "options: host_heap_pad_mb must not be negative");
    SA_REQUIRE(flag(o.ae_order), "options: ae_order must be 0 or 1");
}
// The process-wide default: what saamge_amd_get_options returns and the entry points without a hierarchy use.
static Options g_default_options;
void saamge_amd_options_default(saamge_amd_options *o) { options_to_c(Options(), o); }
void saamge_amd_get_options(saamge_amd_options *o) { options_to_c(g_default_options, o); }
void saamge_amd_set_options(const saamge_amd_options *c) { g_default_options = options_from_c(c); }

void saamge_amd_params_default(saamge_amd_params *p) {
    // defaults of test/mltest/mltest.cpp:332-419
    p->num_coarsenings = 1;
    for (int i = 0; i < SAAMGE_AMD_MAX_LEVELS; ++i) {
        p->theta[i] = 0.003;
        p->nu_relax[i] = 3;
        p->nu_pro[i] = 0;
    }
    p->avoid_ess_bdr_dofs = 1;
    p->testmesh = 0;
    p->coarse_solver = 0;
    p->coarse_rtol = 1e-14;
    p->coarse_max_iter = 2000;
    p->workspace_bytes = (long long)32 << 30;
    p->keep_debug = 0;
    p->rank = 0;
    p->world = 1;
    p->allgather = nullptr;
    p->allgather_ctx = nullptr;
    p->allreduce_sum = nullptr;
    p->alltoallv = nullptr;
    p->dist_min_local_rows = 262144;
    p->comm_stream_ordered = 0;
    p->correct_nullspace = 0;
    p->extra_modes = nullptr;
    p->num_extra_modes = 0;
    p->algebraic = 0;
    p->smooth_drop_tol = 0.0;
    p->do_aggregates = 0;
    p->eigensolver = 0;
    p->eig_tol = 1e-12;
    saamge_amd_options_default(&p->options);
}

int saamge_amd_memcpy(void *dst, const void *src, long long bytes) {
    if (bytes <= 0) return 0;
    if (hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDefault) != hipSuccess) {
        g_last_error = "saamge_amd_memcpy failed";
        (void)hipGetLastError();
        return 2;
    }
    return 0;
}

static Params convert_params(const saamge_amd_params *params, void *stream) {
    Params p;
    p.opt = options_from_c(&params->options);
    validate_options(p.opt);
    host_heap_policy(p.opt.host_heap_pad_mb);
    p.num_coarsenings = params->num_coarsenings;
    SA_REQUIRE(p.num_coarsenings >= 1 && p.num_coarsenings < MAX_LEVELS, "bad num_coarsenings");
    for (int i = 0; i < MAX_LEVELS; ++i) {
        p.theta[i] = params->theta[i];
        p.nu_relax[i] = params->nu_relax[i];
        p.nu_pro[i] = params->nu_pro[i];
    }
    // refused here, before any kernel runs, and not by sas_poly_roots in the middle of a coarse level's setup
    for (int i = 0; i < p.num_coarsenings; ++i) SA_REQUIRE(p.nu_relax[i] > 0, "nu_relax must be positive");
    p.avoid_ess_bdr_dofs = params->avoid_ess_bdr_dofs;
    p.testmesh = params->testmesh;
    p.coarse_solver = params->coarse_solver;
    p.coarse_rtol = params->coarse_rtol;
    p.coarse_max_iter = params->coarse_max_iter;
    p.workspace_bytes = (size_t)params->workspace_bytes;
    p.keep_debug = params->keep_debug;
    p.rank = params->rank;
    p.world = params->world > 1 ? params->world : 1;
    p.allgather = params->allgather;
    p.allgather_ctx = params->allgather_ctx;
    p.allreduce_sum = params->allreduce_sum;
    p.alltoallv = params->alltoallv;
    p.dist_min_local_rows = params->dist_min_local_rows;
    p.comm_stream_ordered = params->comm_stream_ordered;
    {   // a native communicator enqueues its collectives on the stream it was created with: only on the hierarchy's own
        // stream are they ordered with the hierarchy's kernels (round-2 advisor finding: nothing checked this on the C side)
        void *cs = nullptr;
        SA_REQUIRE(!saamge_amd_comm_native_stream(params, &cs) || cs == stream,
                   "the communicator was created on another stream than the one given to saamge_amd_ml_produce_data: "
                   "create it with saamge_amd_comm_create(..., stream, ...) on the hierarchy's stream");
    }
    p.correct_nullspace = params->correct_nullspace;
    p.extra_modes = params->extra_modes;
    p.num_extra_modes = params->num_extra_modes;
    p.algebraic = params->algebraic;
    p.smooth_drop_tol = params->smooth_drop_tol;
    p.do_aggregates = params->do_aggregates;
    p.eigensolver = params->eigensolver;
    SA_REQUIRE(p.eigensolver == 0 || p.eigensolver == 1, "bad eigensolver selector");
    p.eig_tol = params->eig_tol;
    SA_REQUIRE(p.eig_tol >= 1e-15 && p.eig_tol <= 1e-8, "eig_tol must lie in [1e-15, 1e-8] (saamge_amd_params_default sets 1e-12)");
    SA_REQUIRE(p.world == 1 || (p.rank >= 0 && p.rank < p.world), "bad rank");
    return p;
}

static int produce_data(int n, const void *rowptr, int rowptr_bits, const int *col, const double *val,
                        int NE, int nde, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                        const signed char *bdr_dofs, const int *const *partitions,
                        const int *nparts, const saamge_amd_params *params, void *stream,
                        saamge_amd_hierarchy **out) {
    SA_API_BEGIN
    SA_REQUIRE(out && params && rowptr && col && val && (params->algebraic || (elem_to_dof && elmat)) && partitions && nparts,
               "null argument");
    const Params p = convert_params(params, stream);
    set_thread_stream((hipStream_t)stream);
    Hierarchy *H = hierarchy_create(n, rowptr, rowptr_bits, col, val, NE, nde, elem_ptr, elem_to_dof, elmat, bdr_dofs,
                                    partitions, nparts, p, (hipStream_t)stream);
    *out = new saamge_amd_hierarchy{H};
    SA_API_END
}

int saamge_amd_ml_produce_data_parcsr(const saamge_amd_parcsr *A, int NE_local, int nde, const int *elem_to_dof,
                                      const double *elmat, const signed char *bdr_dofs, const int *const *partitions,
                                      const int *nparts_local, const saamge_amd_params *params, void *stream,
                                      saamge_amd_hierarchy **out) {
    SA_API_BEGIN
    SA_REQUIRE(out && params && A && A->diag_i && (A->nrows == 0 || (A->diag_j && A->diag_a)) && partitions && nparts_local &&
                   (NE_local == 0 || (elem_to_dof && elmat)), "null argument");
    SA_REQUIRE(!A->offd_i || A->num_cols_offd == 0 || (A->offd_j && A->offd_a && A->col_map_offd), "offd block without its arrays");
    const Params p = convert_params(params, stream);
    ParCsrIn in;
    in.global_rows = A->global_rows;
    in.row_starts = A->row_starts;
    in.nrows = A->nrows;
    in.diag_i = A->diag_i; in.diag_j = A->diag_j; in.diag_a = A->diag_a;
    in.offd_i = (A->offd_i && A->num_cols_offd > 0) ? A->offd_i : nullptr;
    in.offd_j = A->offd_j; in.offd_a = A->offd_a;
    in.num_cols_offd = A->num_cols_offd;
    in.col_map_offd = A->col_map_offd;
    set_thread_stream((hipStream_t)stream);
    Hierarchy *H = hierarchy_create_dist(in, NE_local, nde, elem_to_dof, elmat, bdr_dofs, partitions, nparts_local, p, (hipStream_t)stream);
    *out = new saamge_amd_hierarchy{H};
    SA_API_END
}

int saamge_amd_ml_produce_data(int n, const int *rowptr, const int *col, const double *val,
                               int NE, int nde, const int *elem_to_dof, const double *elmat,
                               const signed char *bdr_dofs, const int *const *partitions,
                               const int *nparts, const saamge_amd_params *params, void *stream,
                               saamge_amd_hierarchy **out) {
    return produce_data(n, rowptr, 32, col, val, NE, nde, nullptr, elem_to_dof, elmat, bdr_dofs, partitions, nparts, params, stream, out);
}

int saamge_amd_ml_produce_data64(int n, const long long *rowptr, const int *col, const double *val,
                                 int NE, int nde, const int *elem_to_dof, const double *elmat,
                                 const signed char *bdr_dofs, const int *const *partitions,
                                 const int *nparts, const saamge_amd_params *params, void *stream,
                                 saamge_amd_hierarchy **out) {
    return produce_data(n, rowptr, 64, col, val, NE, nde, nullptr, elem_to_dof, elmat, bdr_dofs, partitions, nparts, params, stream, out);
}

int saamge_amd_ml_produce_data_mixed(int n, const int *rowptr, const int *col, const double *val,
                                     int NE, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                                     const signed char *bdr_dofs, const int *const *partitions,
                                     const int *nparts, const saamge_amd_params *params, void *stream,
                                     saamge_amd_hierarchy **out) {
    if (!elem_ptr) { g_last_error = "null argument: elem_ptr"; return 1; }
    return produce_data(n, rowptr, 32, col, val, NE, 0, elem_ptr, elem_to_dof, elmat, bdr_dofs, partitions, nparts, params, stream, out);
}

int saamge_amd_ml_produce_data_mixed64(int n, const long long *rowptr, const int *col, const double *val,
                                       int NE, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                                       const signed char *bdr_dofs, const int *const *partitions,
                                       const int *nparts, const saamge_amd_params *params, void *stream,
                                       saamge_amd_hierarchy **out) {
    if (!elem_ptr) { g_last_error = "null argument: elem_ptr"; return 1; }
    return produce_data(n, rowptr, 64, col, val, NE, 0, elem_ptr, elem_to_dof, elmat, bdr_dofs, partitions, nparts, params, stream, out);
}

int saamge_amd_update_operators(saamge_amd_hierarchy *h, const double *new_val) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    require_device(*h->H);
    hierarchy_update_operators(*h->H, new_val);
    SA_API_END
}

int saamge_amd_update_operators2(saamge_amd_hierarchy *h, const double *new_val, int coarse_solver) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    SA_REQUIRE(coarse_solver >= -1 && coarse_solver <= 3, "coarse_solver: -1 (keep), 0 (auto), 1 (direct), 2 (inner PCG) or 3 (block-tridiagonal direct)");
    require_device(*h->H);
    if (coarse_solver >= 0) h->H->params.coarse_solver = coarse_solver;
    hierarchy_update_operators(*h->H, new_val);
    SA_API_END
}

void saamge_amd_ml_free_data(saamge_amd_hierarchy *h) {
    if (!h) return;
    hipStream_t hs = nullptr;
    const bool had = h->H != nullptr;
    if (had) {
        hs = h->H->stream;
        set_thread_stream(hs);
    }
    delete h->H;
    delete h;
    // the caller may destroy its stream right after this call: no batch of frees stays open on it
    if (had) {
        dev_pool_close_stream(hs);
        unset_thread_stream();      // ... and this thread no longer frees into it
    }
}

// the vectors of a call: host arrays are staged on the device (xfer.h)
typedef DevIn<double> VecIn;
typedef DevOut<double> VecOut;

int saamge_amd_vcycle_mult(saamge_amd_hierarchy *h, const double *b, double *x) {
    SA_API_BEGIN
    SA_REQUIRE(h && b && x, "null argument");
    Hierarchy &H = *h->H;
    require_device(H);
    const size_t n = (size_t)H.levels[0]->A.nrows;
    VecIn vb(b, n, H.stream);
    VecOut vx(x, n, H.stream, false);
    vcycle_apply(H, 0, vb.p, vx.p);
    vx.finish();
    SA_API_END
}

int saamge_amd_vcycle(saamge_amd_hierarchy *h, const double *b, double *x, int iterative_mode) {
    if (!iterative_mode) return saamge_amd_vcycle_mult(h, b, x);
    SA_API_BEGIN
    SA_REQUIRE(h && b && x, "null argument");
    Hierarchy &H = *h->H;
    require_device(H);
    Level &L0 = *H.levels[0];
    SA_REQUIRE(!L0.dist.on, "iterative_mode is not available on a row-partitioned hierarchy");
    const size_t n = (size_t)L0.A.nrows;
    VecIn vb(b, n, H.stream);
    VecOut vx(x, n, H.stream, true);
    vcycle_iterate(H, vb.p, vx.p);      // x <- x + B (b - A x)
    vx.finish();
    SA_API_END
}

int saamge_amd_set_coarse_solver(saamge_amd_hierarchy *h, saamge_amd_coarse_solve_fn fn, void *ctx) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    h->H->coarse.user_solve = fn;
    h->H->coarse.user_ctx = ctx;
    SA_API_END
}

int saamge_amd_set_smoother(saamge_amd_hierarchy *h, int level, saamge_amd_smoother_fn pre, saamge_amd_smoother_fn post,
                            void *ctx) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    Hierarchy &H = *h->H;
    SA_REQUIRE(level >= 0 && level < (int)H.levels.size(), "bad level");
    if (H.user_smoothers.size() < H.levels.size()) H.user_smoothers.resize(H.levels.size());
    H.user_smoothers[(size_t)level].pre = pre;
    H.user_smoothers[(size_t)level].post = post;
    H.user_smoothers[(size_t)level].ctx = ctx;
    SA_API_END
}

int saamge_amd_smoother(saamge_amd_hierarchy *h, int level, const double *b, double *x) {
    SA_API_BEGIN
    SA_REQUIRE(h && b && x, "null argument");
    Hierarchy &H = *h->H;
    require_device(H);
    SA_REQUIRE(level >= 0 && level < (int)H.levels.size(), "bad level");
    const size_t n = (size_t)H.levels[level]->A.nrows;
    VecIn vb(b, n, H.stream);
    VecOut vx(x, n, H.stream, true);
    smoother_apply(H, level, vb.p, vx.p);
    vx.finish();
    SA_API_END
}

int saamge_amd_pcg(saamge_amd_hierarchy *h, const double *b, double *x, double rel_tol,
                   double abs_tol, int max_iter, int squared_tol, int zero_guess, int *iters,
                   int *converged, double *hist) {
    SA_API_BEGIN
    SA_REQUIRE(h && b && x && iters, "null argument");
    Hierarchy &H = *h->H;
    require_device(H);
    const size_t n = (size_t)H.levels[0]->A.nrows;
    VecIn vb(b, n, H.stream);
    VecOut vx(x, n, H.stream, !zero_guess);
    int conv = 0;
    *iters = pcg_solve(H, vb.p, vx.p, rel_tol, abs_tol, max_iter, squared_tol, zero_guess, &conv, hist);
    if (converged) *converged = conv;
    vx.finish();
    SA_API_END
}

int saamge_amd_num_levels(const saamge_amd_hierarchy *h) { return h ? (int)h->H->levels.size() + 1 : 0; }

static const DCsr &level_op(const Hierarchy &H, int level, int which) {
    const int nl = (int)H.levels.size();
    SA_REQUIRE(level >= 0 && level < nl, "bad level");
    const Level &L = *H.levels[level];
    switch (which) {
        case 0: return L.A;
        case 1: return L.P;
        case 2: return L.R;
        case 3: return (level + 1 < nl) ? H.levels[level + 1]->A : L.Ac;
    }
    throw Error(1, "bad operator selector");
}

int saamge_amd_level_info(const saamge_amd_hierarchy *h, int level, long long info[16]) {
    SA_API_BEGIN
    SA_REQUIRE(h && info, "null argument");
    const Hierarchy &H = *h->H;
    for (int i = 0; i < 16; ++i) info[i] = 0;
    const Level &L = *H.levels.at(level);
    info[0] = L.A.nrows;
    info[1] = L.A.nnz;
    info[2] = L.rel.nparts;
    info[3] = L.rel.num_mises;
    info[4] = L.P.ncols;
    info[5] = L.P.nnz;
    info[6] = level_op(H, level, 3).nnz;
    long long tot = 0;
    for (int m : L.ae_m) tot += m;
    info[7] = tot;
    info[8] = H.coarse.last_iters;
    info[9] = L.ae_xoff.empty() ? 0 : L.ae_xoff.back();
    info[10] = L.mis_s_off.empty() ? 0 : L.mis_s_off.back();
    long long usz = 0;
    for (int m = 0; m < L.rel.num_mises; ++m) usz += (long long)L.mis_k[m] * L.rel.mis_to_dof.row_size(m);
    info[11] = usz;
    info[12] = L.dist.on ? 1 : 0;
    info[13] = L.dist.row0;
    info[14] = L.dist.nloc;
    info[15] = L.dist.nrecv;
    SA_API_END
}

int saamge_amd_level_format(const saamge_amd_hierarchy *h, int level, long long info[12]) {
    SA_API_BEGIN
    SA_REQUIRE(h && info, "null argument");
    const Hierarchy &H = *h->H;
    for (int i = 0; i < 12; ++i) info[i] = 0;
    const Sell &S = H.levels.at(level)->A.sell;      // (all zero for an operator without a copy)
    for (int c = 0; c < 3; ++c) { info[c] = S.class_slices[c]; info[3 + c] = S.class_entries[c]; }
    if (S.dict.on) { info[8] = S.dict.ng; info[9] = S.dict.bs3 ? 1 : 0; info[10] = S.dict.bs3 ? S.dict.nirr : 0; }
    info[6] = S.stage.on() ? (long long)div_up(S.nslices, 4) - S.stage.nunstaged : 0;
    info[7] = (long long)S.stream_bytes;
    info[11] = H.levels.at(level)->ae_solved;
    SA_API_END
}

int saamge_amd_level_order_info(const saamge_amd_hierarchy *h, int level, long long info[4]) {
    SA_API_BEGIN
    SA_REQUIRE(h && info, "null argument");
    const Hierarchy &H = *h->H;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    SA_REQUIRE(level >= 0 && level < (int)H.levels.size(), "no such level");
    const Level &L = *H.levels[(size_t)level];
    require_device(H);
    hipStream_t s = H.stream;
    if (H.params.opt.ae_order == 1) {      // what the setup's ordering pass added up
        if (L.order_info.n == 4) {
            int v[4];
            read_back(v, (const int *)L.order_info.p, 4, s);
            for (int i = 0; i < 4; ++i) info[i] = v[i];
        }
    } else {      // ae_order = 0: the setup measures nothing; the band of the rank / box order of those chunks, now
        for (const std::pair<int, int> &c : L.order_chunks) {
            EigBatch b;
            b.count = c.second;
            b.h_voff.assign((size_t)b.count + 1, 0);
            for (int i = 0; i < b.count; ++i) {
                const int n = L.rel.AE_to_dof.row_size(c.first + i);
                b.h_n.push_back(n);
                b.h_voff[(size_t)i + 1] = b.h_voff[(size_t)i] + n;
                b.max_n = std::max(b.max_n, n);
            }
            info[0] += b.count;
            if (b.max_n > 8192) continue;      // (ae_order_only's limit)
            b.n.from_host(b.h_n, s);
            b.voff.from_host(b.h_voff, s);
            DBuf<int> res(3 * (size_t)b.count);
            ae_order_only(s, L.drel, c.first, b, 0, res.p);
            const hvec<int> hr = res.to_host(s);
            for (int i = 0; i < b.count; ++i) info[2] = std::max<long long>(info[2], hr[3 * (size_t)i]);
        }
        info[3] = info[2];
    }
    SA_API_END
}

int saamge_amd_coarse_solver_info(const saamge_amd_hierarchy *h, long long info[8]) {
    SA_API_BEGIN
    SA_REQUIRE(h && info, "null argument");
    const Hierarchy &H = *h->H;
    for (int i = 0; i < 8; ++i) info[i] = 0;
    SA_REQUIRE(!H.levels.empty(), "no levels");
    const CoarseSolver &C = H.coarse;
    info[0] = C.user_solve ? 0 : C.kind;
    info[1] = H.levels.back()->Ac.nrows;
    if (C.kind == 3) {
        info[2] = C.bt.nblk;
        info[3] = C.bt.max_block;
        info[4] = (long long)C.bt.Sinv.n;
    } else if (C.kind == 1) {
        info[4] = (long long)C.inv.n;
    }
    SA_API_END
}

static int get_csr(const saamge_amd_hierarchy *h, int level, int which, void *rowptr, int rowptr_bits, int *col, double *val) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    const Hierarchy &H = *h->H;
    require_device(H);
    const DCsr &M = level_op(H, level, which);
    hipStream_t s = H.stream;
    if (rowptr && rowptr_bits == 64)
        copy_to_caller((roff_t *)rowptr, (const roff_t *)M.rowptr.p, (size_t)M.nrows + 1, s);
    else if (rowptr)
        export_rowptr32((int *)rowptr, M.rowptr, (size_t)M.nrows + 1, s);
    copy_to_caller(col, (const int *)M.col.p, (size_t)M.nnz, s);
    copy_to_caller(val, (const double *)M.val.p, (size_t)M.nnz, s);
    SA_API_END
}
int saamge_amd_get_csr(const saamge_amd_hierarchy *h, int level, int which, int *rowptr, int *col, double *val) {
    return get_csr(h, level, which, rowptr, 32, col, val);
}
int saamge_amd_get_csr64(const saamge_amd_hierarchy *h, int level, int which, long long *rowptr, int *col, double *val) {
    return get_csr(h, level, which, rowptr, 64, col, val);
}

int saamge_amd_get_table(const saamge_amd_hierarchy *h, int level, int which, int *nrows,
                         long long *nconn, int *I, int *J) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    require_device(*h->H);
    {   // tables kept on the device by the device topology build: host copies on demand
        Level &Lw = *h->H->levels.at(level);
        fetch_relations_ae_host(Lw.rel, Lw.drel, h->H->stream);
    }
    const Relations &r = h->H->levels.at(level)->rel;
    const Table *T = nullptr;
    switch (which) {
        case 0: T = &r.AE_to_dof; break;
        case 1: T = &r.dof_to_AE; break;
        case 2: T = &r.mis_to_dof; break;
        case 3: T = &r.mis_to_AE; break;
        case 4: T = &r.AE_to_mis; break;
        case 5: {
            if (r.elem_to_dof.I.empty()) {   // built on the device: fetch the host copy on demand
                Level &L = *h->H->levels.at(level);
                Relations &rw = L.rel;
                rw.elem_to_dof.I = L.drel.e2d_I.to_host(h->H->stream);
                rw.elem_to_dof.J = L.drel.e2d_J.to_host(h->H->stream);
                rw.elem_to_dof.ncols = rw.ND;
            }
            T = &r.elem_to_dof;
            break;
        }
        default: throw Error(1, "bad table selector");
    }
    if (nrows) *nrows = T->nrows();
    if (nconn) *nconn = (long long)T->J.size();
    if (I) std::copy(T->I.begin(), T->I.end(), I);
    if (J) std::copy(T->J.begin(), T->J.end(), J);
    SA_API_END
}

int saamge_amd_get_mis(const saamge_amd_hierarchy *h, int level, int *mises, int *mis_k,
                       int *mis_ncols, signed char *agg_flags) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    require_device(*h->H);
    {
        Level &Lw = *h->H->levels.at(level);
        fetch_relations_ae_host(Lw.rel, Lw.drel, h->H->stream);
    }
    const Level &L = *h->H->levels.at(level);
    if (mises) std::copy(L.rel.mises.begin(), L.rel.mises.end(), mises);
    if (mis_k) std::copy(L.mis_k.begin(), L.mis_k.end(), mis_k);
    if (mis_ncols) std::copy(L.mis_ncols.begin(), L.mis_ncols.end(), mis_ncols);
    if (agg_flags) std::copy(L.rel.agg_flags.begin(), L.rel.agg_flags.end(), agg_flags);
    SA_API_END
}

int saamge_amd_get_ae_eigens(const saamge_amd_hierarchy *h, int level, int *ae_m, double *evals,
                             double *evecs, double *ae_D) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    const Hierarchy &H = *h->H;
    const Level &L = *H.levels.at(level);
    hipStream_t s = H.stream;
    if (ae_m) std::copy(L.ae_m.begin(), L.ae_m.end(), ae_m);
    if (evals || evecs || ae_D) SA_REQUIRE(H.params.keep_debug, "hierarchy was built without keep_debug");
    copy_to_caller(evals, L.evals, s);
    copy_to_caller(evecs, L.evecs, s);
    copy_to_caller(ae_D, L.ae_D, s);
    SA_API_END
}

int saamge_amd_get_mis_svd(const saamge_amd_hierarchy *h, int level, long long *sig_off,
                           double *sig, double *U) {
    SA_API_BEGIN
    SA_REQUIRE(h, "null argument");
    const Hierarchy &H = *h->H;
    const Level &L = *H.levels.at(level);
    hipStream_t s = H.stream;
    const int nm = L.rel.num_mises;
    if (sig_off) for (int m = 0; m <= nm; ++m) sig_off[m] = L.mis_s_off[m];
    if (sig) {
        SA_REQUIRE(H.params.keep_debug, "hierarchy was built without keep_debug");
        copy_to_caller(sig, (const double *)L.mis_sig.p, (size_t)L.mis_s_off[nm], s);
    }
    if (U) {
        auto all = L.mis_U.to_host(s);
        size_t o = 0;
        for (int m = 0; m < nm; ++m) {
            const size_t cnt = (size_t)L.mis_k[m] * L.rel.mis_to_dof.row_size(m);
            std::copy(all.begin() + L.mis_u_off[m], all.begin() + L.mis_u_off[m] + cnt, U + o);
            o += cnt;
        }
    }
    SA_API_END
}

static int spmv_entry(int nrows, int ncols, const void *rowptr, int rowptr_bits, const int *col, const double *val,
                      const double *x, double *y) {
    SA_API_BEGIN
    SA_REQUIRE(rowptr && col && val && x && y && nrows >= 0, "bad argument");
    const Options opt = g_default_options;
    validate_options(opt);
    hipStream_t s = 0;
    set_thread_stream(s);
    DCsr A;
    A.nrows = nrows;
    A.ncols = ncols;
    import_rowptr(A.rowptr, rowptr, rowptr_bits, (size_t)nrows + 1, s);
    roff_t nnz = read_one(A.rowptr.p + nrows, s);
    A.nnz = nnz;
    A.col = DevIn<int>(col, (size_t)A.nnz, s).take();
    A.val = DevIn<double>(val, (size_t)A.nnz, s).take();
    A.lanes_per_row = pick_lanes_per_row(A.nnz, nrows > 0 ? nrows : 1);
    // spmv_sell (tests): through the SELL-64 copy and its coded slices, the format of the level operators
    if (nrows == ncols && opt.spmv_sell) build_sell(s, A, opt);
    VecIn vx(x, (size_t)ncols, s);
    VecOut vy(y, (size_t)nrows, s, false);
    spmv(s, A, vx.p, vy.p);
    vy.finish();
    SA_API_END
}
int saamge_amd_spmv(int nrows, int ncols, const int *rowptr, const int *col, const double *val,
                    const double *x, double *y) {
    return spmv_entry(nrows, ncols, rowptr, 32, col, val, x, y);
}
int saamge_amd_spmv64(int nrows, int ncols, const long long *rowptr, const int *col, const double *val,
                      const double *x, double *y) {
    return spmv_entry(nrows, ncols, rowptr, 64, col, val, x, y);
}

// ---- the general sparse products on their own (spgemm.hip; tests) -------------------------------------------------------
// A host CSR matrix on the device.  The arrays are checked first: the kernels trust offsets and column indices.
static void import_host_csr(DCsr &M, const char *name, int nrows, int ncols, const int *rowptr, const int *col,
                            const double *val, hipStream_t s) {
    const std::string who(name);
    SA_REQUIRE(nrows >= 0 && ncols >= 0 && rowptr, who + ": bad dimensions or no row offsets");
    SA_REQUIRE(rowptr[0] == 0, who + ": the row offsets must start at 0");
    for (int i = 0; i < nrows; ++i) SA_REQUIRE(rowptr[i + 1] >= rowptr[i], who + ": the row offsets must ascend");
    const size_t nnz = (size_t)rowptr[nrows];
    SA_REQUIRE(nnz == 0 || (col && val), who + ": entries without their arrays");
    for (size_t k = 0; k < nnz; ++k) SA_REQUIRE(col[k] >= 0 && col[k] < ncols, who + ": a column index out of range");
    M.nrows = nrows;
    M.ncols = ncols;
    M.nnz = (int64_t)nnz;
    import_rowptr(M.rowptr, rowptr, 32, (size_t)nrows + 1, s);
    M.col.assign(col, nnz, s);
    M.val.assign(val, nnz, s);
    M.lanes_per_row = pick_lanes_per_row(M.nnz, nrows > 0 ? nrows : 1);
}
// row offsets and *nnz always; the entries when both arrays are given (the first call of a caller asks for the sizes)
static void export_host_csr(const DCsr &M, int *rowptr, long long *nnz, int *col, double *val, hipStream_t s) {
    if (rowptr) export_rowptr32(rowptr, M.rowptr, (size_t)M.nrows + 1, s);
    if (nnz) *nnz = (long long)M.nnz;
    if (col && val) {
        copy_to_caller(col, (const int *)M.col.p, (size_t)M.nnz, s);
        copy_to_caller(val, (const double *)M.val.p, (size_t)M.nnz, s);
    }
}

int saamge_amd_spgemm(int nrows, int ninner, int ncols, const int *Arow, const int *Acol, const double *Aval,
                      const int *Brow, const int *Bcol, const double *Bval, const int *Erow, const int *Ecol,
                      const double *Eval, const double *d, double alpha, double beta, int *Crow, long long *Cnnz,
                      int *Ccol, double *Cval, int *route) {
    if (route) *route = SPGEMM_ROUTE_NONE;
    SA_API_BEGIN
    hipStream_t s = 0;
    set_thread_stream(s);
    DCsr A, B, E, Cm;
    import_host_csr(A, "A", nrows, ninner, Arow, Acol, Aval, s);
    import_host_csr(B, "B", ninner, ncols, Brow, Bcol, Bval, s);
    // E given as B's own arrays is B's device copy as well (interp_smooth: P <- P - w D^-1 A P)
    const bool alias = Erow && Erow == Brow && Ecol == Bcol && Eval == Bval && nrows == ninner;
    if (Erow && !alias) import_host_csr(E, "E", nrows, ncols, Erow, Ecol, Eval, s);
    DBuf<double> dd;
    if (d) dd.assign(d, (size_t)nrows, s);
    spgemm(s, A, B, Erow ? (alias ? &B : &E) : nullptr, d ? dd.p : nullptr, alpha, beta, Cm);
    if (route) *route = spgemm_last_route();
    export_host_csr(Cm, Crow, Cnnz, Ccol, Cval, s);
    SA_API_END
}

int saamge_amd_ae_order(int ND, int NE, int nde, const int *elem_ptr, const int *elem_to_dof, const int *elem_to_ae,
                        int nparts, int mode, int *ae_ptr, long long *nconn, int *ae_to_dof, int *pos, int *bw0, int *bw,
                        int *choice) {
    SA_API_BEGIN
    SA_REQUIRE(mode == 0 || mode == 1, "saamge_amd_ae_order: ae_order must be 0 or 1");
    SA_REQUIRE(elem_to_dof && elem_to_ae && ae_ptr && nconn, "saamge_amd_ae_order: null argument");
    SA_REQUIRE(ND >= 1 && NE >= 1 && nparts >= 1 && (elem_ptr || nde >= 1), "saamge_amd_ae_order: bad size");
    Table e2d;
    e2d.I.resize((size_t)NE + 1);
    if (elem_ptr) {
        SA_REQUIRE(elem_ptr[0] == 0, "saamge_amd_ae_order: elem_ptr must start at 0");
        for (int e = 0; e < NE; ++e) SA_REQUIRE(elem_ptr[e + 1] > elem_ptr[e], "saamge_amd_ae_order: every element needs a dof");
        for (int e = 0; e <= NE; ++e) e2d.I[(size_t)e] = elem_ptr[e];
    } else {
        SA_REQUIRE((long long)NE * nde <= 2147483647LL, "saamge_amd_ae_order: mesh too large");
        for (int e = 0; e <= NE; ++e) e2d.I[(size_t)e] = e * nde;
    }
    e2d.J.assign(elem_to_dof, elem_to_dof + e2d.I[(size_t)NE]);
    hvec<int> part(elem_to_ae, elem_to_ae + NE);
    Relations rel;
    build_relations_ae(rel, std::move(e2d), part, nparts, ND, nullptr);      // (checks the ranges)
    for (int p = 0; p <= nparts; ++p) ae_ptr[p] = rel.AE_to_dof.I[(size_t)p];
    const size_t rows = (size_t)rel.AE_to_dof.I[(size_t)nparts];
    *nconn = (long long)rows;
    if (ae_to_dof && pos) {
        SA_REQUIRE(bw0 && bw && choice, "saamge_amd_ae_order: null argument");
        hipStream_t s = 0;
        set_thread_stream(s);
        DevRelations drel;
        upload_relations_ae(drel, rel, s);
        std::vector<int> sizes((size_t)nparts);
        for (int p = 0; p < nparts; ++p) sizes[(size_t)p] = rel.AE_to_dof.row_size(p);
        // (no eigensolver workspace: the sizes and row offsets of the batch only)
        EigBatch b;
        b.count = nparts;
        b.h_n.assign(sizes.begin(), sizes.end());
        b.h_voff.assign((size_t)nparts + 1, 0);
        for (int p = 0; p < nparts; ++p) {
            b.h_voff[(size_t)p + 1] = b.h_voff[(size_t)p] + sizes[(size_t)p];
            b.max_n = std::max(b.max_n, sizes[(size_t)p]);
        }
        b.n.from_host(b.h_n, s);
        b.voff.from_host(b.h_voff, s);
        DBuf<int> res(3 * (size_t)nparts);
        ae_order_only(s, drel, 0, b, mode, res.p);
        const hvec<int> hr = res.to_host(s);
        const hvec<short> hp = b.perm.to_host(s);
        for (int p = 0; p < nparts; ++p) { bw0[p] = hr[3 * (size_t)p]; bw[p] = hr[3 * (size_t)p + 1]; choice[p] = hr[3 * (size_t)p + 2]; }
        for (size_t k = 0; k < rows; ++k) { ae_to_dof[k] = rel.AE_to_dof.J[k]; pos[k] = hp[k]; }
    }
    SA_API_END
}

int saamge_amd_element_matrices(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                const int *elem_to_vertex, int kind, int ncoef, const double *coef, void *stream,
                                double *elmat_out, int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_matrices(s, m, kind, ncoef, coef, elmat_out, dof_ptr_out, elem_to_dof_out, info);
    });
}

int saamge_amd_element_mass(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                            const int *elem_to_vertex, int vdim, const double *coef, void *stream, int accumulate,
                            double *elmat_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_mass(s, m, vdim, coef, accumulate, elmat_inout, info);
    });
}

int saamge_amd_element_loads(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int vdim, const double *coef, const double *src, void *stream,
                             double *elvec_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_loads(s, m, vdim, coef, src, elvec_out, info);
    });
}

int saamge_amd_boundary_mass(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                             const double *coef, void *stream, double *elmat_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_mass(s, m, NF, face_elem, face_local, vdim, coef, elmat_inout, info);
    });
}

int saamge_amd_boundary_loads(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                              const double *coef, const double *g, void *stream, double *elvec_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_loads(s, m, NF, face_elem, face_local, vdim, coef, g, elvec_inout, info);
    });
}

int saamge_amd_boundary_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                               const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, void *stream,
                               long long *fp_ptr_out, double *xq_out, double *wmeas_out, double *normal_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_points(s, m, NF, face_elem, face_local, fp_ptr_out, xq_out, wmeas_out, normal_out, info);
    });
}

int saamge_amd_boundary_eval(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                             const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                             const double *u, void *stream, double *uq_out, double *gradq_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_eval(s, m, NF, face_elem, face_local, vdim, u, uq_out, gradq_out, info);
    });
}

int saamge_amd_boundary_mass_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                    const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                                    const double *coefq, void *stream, double *elmat_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_mass_points(s, m, NF, face_elem, face_local, vdim, coefq, elmat_inout, info);
    });
}

int saamge_amd_boundary_loads_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                     const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local, int vdim,
                                     const double *coef, const double *gq, void *stream, double *elvec_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        boundary_loads_points(s, m, NF, face_elem, face_local, vdim, coef, gq, elvec_inout, info);
    });
}

int saamge_amd_element_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, void *stream, long long *qp_ptr_out, double *xq_out, double *wdet_out,
                              long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_points(s, m, qp_ptr_out, xq_out, wdet_out, info);
    });
}

int saamge_amd_element_eval(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                            const int *elem_to_vertex, int vdim, const double *u, void *stream, double *uq_out, double *gradq_out,
                            long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_eval(s, m, vdim, u, uq_out, gradq_out, info);
    });
}

int saamge_amd_element_loads_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                    const int *elem_to_vertex, int vdim, const double *coef, const double *fq, void *stream,
                                    double *elvec_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_loads_points(s, m, vdim, coef, fq, elvec_out, info);
    });
}

int saamge_amd_element_errors(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                              const int *elem_to_vertex, int vdim, const double *u, const double *exq, const double *exgradq,
                              void *stream, double *err_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_errors(s, m, vdim, u, exq, exgradq, err_out, info);
    });
}

int saamge_amd_element_matrices_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                       const int *elem_to_vertex, int kind, int ncoef, const double *coefq, void *stream,
                                       double *elmat_out, int *dof_ptr_out, int *elem_to_dof_out, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_matrices_points(s, m, kind, ncoef, coefq, elmat_out, dof_ptr_out, elem_to_dof_out, info);
    });
}

int saamge_amd_element_mass_points(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                   const int *elem_to_vertex, int vdim, const double *coefq, void *stream, int accumulate,
                                   double *elmat_inout, long long info[8]) {
    return mesh_call({NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        element_mass_points(s, m, vdim, coefq, accumulate, elmat_inout, info);
    });
}

// ---- the faces of a mesh (mesh_faces.hip) -----------------------------------------------------------------------------------
int saamge_amd_face_table_build(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, void *stream,
                                saamge_amd_face_table **out, long long info[8]) {
    return mesh_handle_call("saamge_amd_face_table_build", out, true, {NV, dim, nullptr, NE, nde, elem_ptr, elem_to_vertex}, stream,
                            [&](hipStream_t s, const MeshArgs &m, saamge_amd_face_table &h) { face_table_build(s, m, h.t, info); });
}

int saamge_amd_face_table_arrays(const saamge_amd_face_table *t, const long long **slot_ptr, const int **nbr_elem,
                                 const int **nbr_local, long long *NB, const int **bdr_elem, const int **bdr_local,
                                 const long long **xadj, const int **adj, long long *nnz) {
    SA_API_BEGIN
    SA_REQUIRE(t, "saamge_amd_face_table_arrays: null argument");
    if (slot_ptr) *slot_ptr = (const long long *)t->t.slot_ptr.p;
    if (nbr_elem) *nbr_elem = t->t.nbr_elem.p;
    if (nbr_local) *nbr_local = t->t.nbr_local.p;
    if (NB) *NB = t->t.NB;
    if (bdr_elem) *bdr_elem = t->t.bdr_elem.p;
    if (bdr_local) *bdr_local = t->t.bdr_local.p;
    if (xadj) *xadj = (const long long *)t->t.xadj.p;
    if (adj) *adj = t->t.adj.p;
    if (nnz) *nnz = t->t.nnz;
    SA_API_END
}

int saamge_amd_face_table_get(const saamge_amd_face_table *t, long long *slot_ptr, int *nbr_elem, int *nbr_local, long long *NB,
                              int *bdr_elem, int *bdr_local, long long *xadj, int *adj, long long *nnz) {
    SA_API_BEGIN
    SA_REQUIRE(t, "saamge_amd_face_table_get: null argument");
    const FaceTable &T = t->t;
    if (NB) *NB = T.NB;
    if (nnz) *nnz = T.nnz;
    if (slot_ptr || nbr_elem || nbr_local || bdr_elem || bdr_local || xadj || adj) require_device(T.device, "face table");
    copy_out(slot_ptr, T.slot_ptr);
    copy_out(nbr_elem, T.nbr_elem);
    copy_out(nbr_local, T.nbr_local);
    copy_out(bdr_elem, T.bdr_elem);
    copy_out(bdr_local, T.bdr_local);
    copy_out(xadj, T.xadj);
    copy_out(adj, T.adj);
    SA_API_END
}

void saamge_amd_face_table_free(saamge_amd_face_table *t) { delete t; }

int saamge_amd_face_nodes(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                          const int *face_elem, const int *face_local, void *stream, int *face_ptr_out, int *face_nodes_out,
                          long long *count_out) {
    return mesh_call({NV, dim, nullptr, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        face_nodes(s, m, NF, face_elem, face_local, face_ptr_out, face_nodes_out, count_out);
    });
}

int saamge_amd_face_dofs(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                         const int *face_elem, const int *face_local, int vdim, unsigned comp_mask, int flag, void *stream,
                         signed char *bdr_dofs_inout, long long info[4]) {
    return mesh_call({NV, dim, nullptr, NE, nde, elem_ptr, elem_to_vertex}, stream, [&](hipStream_t s, const MeshArgs &m) {
        face_dofs(s, m, NF, face_elem, face_local, vdim, comp_mask, flag, bdr_dofs_inout, info);
    });
}

// ---- an order-1 mesh lifted to order 2 (mesh_lift.hip) ------------------------------------------------------------------------
int saamge_amd_mesh_lift_order2(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                const int *elem_to_vertex, const saamge_amd_face_table *faces, void *stream,
                                saamge_amd_mesh_lift **out, long long info[8]) {
    return mesh_handle_call("saamge_amd_mesh_lift_order2", out, false, {NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream,
                            [&](hipStream_t s, const MeshArgs &m, saamge_amd_mesh_lift &h) {
                                mesh_lift_order2(s, m, faces ? &faces->t : nullptr, h.l, info);
                            });
}

int saamge_amd_mesh_lift_arrays(const saamge_amd_mesh_lift *m, int *NV2, const double **coords2, const int **elem_ptr2,
                                const int **elem_to_node, const long long **edge_ptr, const int **edge_hi,
                                const long long **face_slot) {
    SA_API_BEGIN
    SA_REQUIRE(m, "saamge_amd_mesh_lift_arrays: null argument");
    if (NV2) *NV2 = m->l.NV2;
    if (coords2) *coords2 = m->l.coords2.p;
    if (elem_ptr2) *elem_ptr2 = m->l.elem_ptr2.p;
    if (elem_to_node) *elem_to_node = m->l.elem_to_node.p;
    if (edge_ptr) *edge_ptr = (const long long *)m->l.edge_ptr.p;
    if (edge_hi) *edge_hi = m->l.edge_hi.p;
    if (face_slot) *face_slot = (const long long *)m->l.face_slot.p;
    SA_API_END
}

int saamge_amd_mesh_lift_get(const saamge_amd_mesh_lift *m, int *NV2, double *coords2, int *elem_ptr2, int *elem_to_node,
                             long long *edge_ptr, int *edge_hi, long long *face_slot) {
    SA_API_BEGIN
    SA_REQUIRE(m, "saamge_amd_mesh_lift_get: null argument");
    const MeshLift &L = m->l;
    if (NV2) *NV2 = L.NV2;
    if (coords2 || elem_ptr2 || elem_to_node || edge_ptr || edge_hi || face_slot) require_device(L.device, "lifted mesh");
    copy_out(coords2, L.coords2);
    copy_out(elem_ptr2, L.elem_ptr2);
    copy_out(elem_to_node, L.elem_to_node);
    copy_out(edge_ptr, L.edge_ptr);
    copy_out(edge_hi, L.edge_hi);
    copy_out(face_slot, L.face_slot);
    SA_API_END
}

void saamge_amd_mesh_lift_free(saamge_amd_mesh_lift *m) { delete m; }

// ---- an order-1 mesh refined uniformly (mesh_refine.hip) ------------------------------------------------------------------------
int saamge_amd_mesh_refine(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex,
                           int levels, int want_interp, void *stream, saamge_amd_refined_mesh **out, long long info[8]) {
    return mesh_handle_call("saamge_amd_mesh_refine", out, false, {NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex}, stream,
                            [&](hipStream_t s, const MeshArgs &m, saamge_amd_refined_mesh &h) {
                                mesh_refine(s, m, levels, want_interp, h.r, info);
                            });
}

int saamge_amd_mesh_refine_arrays(const saamge_amd_refined_mesh *m, int *NV, int *NE, const double **coords, const int **elem_ptr,
                                  const int **elem_to_vertex) {
    SA_API_BEGIN
    SA_REQUIRE(m, "saamge_amd_mesh_refine_arrays: null argument");
    if (NV) *NV = m->r.NV;
    if (NE) *NE = m->r.NE;
    if (coords) *coords = m->r.coords.p;
    if (elem_ptr) *elem_ptr = m->r.elem_ptr.p;
    if (elem_to_vertex) *elem_to_vertex = m->r.elem_to_vertex.p;
    SA_API_END
}

int saamge_amd_mesh_refine_get(const saamge_amd_refined_mesh *m, int *NV, int *NE, double *coords, int *elem_ptr,
                               int *elem_to_vertex) {
    SA_API_BEGIN
    SA_REQUIRE(m, "saamge_amd_mesh_refine_get: null argument");
    const MeshRefine &R = m->r;
    if (NV) *NV = R.NV;
    if (NE) *NE = R.NE;
    if (coords || elem_ptr || elem_to_vertex) require_device(R.device, "refined mesh");
    copy_out(coords, R.coords);
    copy_out(elem_ptr, R.elem_ptr);
    copy_out(elem_to_vertex, R.elem_to_vertex);
    SA_API_END
}

int saamge_amd_mesh_refine_level_info(const saamge_amd_refined_mesh *m, int level, long long info[8]) {
    SA_API_BEGIN
    SA_REQUIRE(m && info, "saamge_amd_mesh_refine_level_info: null argument");
    SA_REQUIRE(level >= 0 && level <= m->r.levels, "saamge_amd_mesh_refine_level_info: level is outside [0, levels]");
    const MeshRefineLevel &l = m->r.level[(size_t)level];
    const long long v[8] = {l.NV, l.NE, l.entries, l.NEd, l.NFq, l.NC, l.max_owned, l.nnz};
    for (int k = 0; k < 8; ++k) info[k] = v[k];
    SA_API_END
}

static const MeshInterp &refine_interp(const saamge_amd_refined_mesh *m, int level, const std::string &name) {
    SA_REQUIRE(m, name + "null argument");
    SA_REQUIRE(!m->r.P.empty(), name + "the mesh was refined without want_interp");
    SA_REQUIRE(level >= 0 && level < m->r.levels, name + "level is outside [0, levels)");
    return m->r.P[(size_t)level];
}

int saamge_amd_mesh_refine_interp_arrays(const saamge_amd_refined_mesh *m, int level, int *nrows, int *ncols, long long *nnz,
                                         const int **rowptr, const int **col, const double **val) {
    SA_API_BEGIN
    const MeshInterp &P = refine_interp(m, level, "saamge_amd_mesh_refine_interp_arrays: ");
    if (nrows) *nrows = P.nrows;
    if (ncols) *ncols = P.ncols;
    if (nnz) *nnz = P.nnz;
    if (rowptr) *rowptr = P.rowptr.p;
    if (col) *col = P.col.p;
    if (val) *val = P.val.p;
    SA_API_END
}

int saamge_amd_mesh_refine_interp_get(const saamge_amd_refined_mesh *m, int level, int *nrows, int *ncols, long long *nnz,
                                      int *rowptr, int *col, double *val) {
    SA_API_BEGIN
    const MeshInterp &P = refine_interp(m, level, "saamge_amd_mesh_refine_interp_get: ");
    if (nrows) *nrows = P.nrows;
    if (ncols) *ncols = P.ncols;
    if (nnz) *nnz = P.nnz;
    if (rowptr || col || val) require_device(m->r.device, "refined mesh");
    copy_out(rowptr, P.rowptr);
    copy_out(col, P.col);
    copy_out(val, P.val);
    SA_API_END
}

void saamge_amd_mesh_refine_free(saamge_amd_refined_mesh *m) { delete m; }

int saamge_amd_csr_transpose(int nrows, int ncols, const int *rowptr, const int *col, const double *val, int *Rrow,
                             long long *Rnnz, int *Rcol, double *Rval) {
    SA_API_BEGIN
    hipStream_t s = 0;
    set_thread_stream(s);
    DCsr P, R;
    import_host_csr(P, "P", nrows, ncols, rowptr, col, val, s);
    csr_transpose(s, P, R);
    export_host_csr(R, Rrow, Rnnz, Rcol, Rval, s);
    SA_API_END
}

int saamge_amd_csr_threshold(int nrows, int ncols, const int *rowptr, const int *col, const double *val, double tol,
                             int *Crow, long long *Cnnz, int *Ccol, double *Cval) {
    SA_API_BEGIN
    hipStream_t s = 0;
    set_thread_stream(s);
    DCsr A, Cm;
    import_host_csr(A, "A", nrows, ncols, rowptr, col, val, s);
    csr_threshold(s, A, tol, Cm);
    export_host_csr(Cm, Crow, Cnnz, Ccol, Cval, s);
    SA_API_END
}

__global__ void apply_dscale_kernel(int count, const int *ns, const int64_t *moff, const int64_t *voff,
                                    double *W, const double *D, double *dis) {
    const int b = blockIdx.x;
    const int n = ns[b];
    double *Wm = W + moff[b];
    const double *Dm = D + voff[b];
    for (int i = threadIdx.x; i < n; i += blockDim.x) dis[voff[b] + i] = 1.0 / sqrt(Dm[i]);
    __syncthreads();
    for (size_t idx = threadIdx.x; idx < (size_t)n * n; idx += blockDim.x) {
        const int r = (int)(idx % n), c = (int)(idx / n);
        Wm[idx] = dis[voff[b] + r] * Wm[idx] * dis[voff[b] + c];
    }
}

// W = D^-1/2 A D^-1/2 of every matrix of the batch, from the caller's A (host or device) and the diagonals dD (device)
static void upload_scaled(hipStream_t s, EigBatch &b, const double *A, const double *dD) {
    upload(b.W.p, A, (size_t)b.h_moff[b.count], s);
    hipLaunchKernelGGL(apply_dscale_kernel, dim3(b.count), dim3(256), 0, s, b.count, b.n.p, b.moff.p, b.voff.p, b.W.p, dD,
                       b.dis.p);
}

int saamge_amd_lower_eigens_batched(int count, const int *n, const double *A, const double *D,
                                    double vl, double vu, int *m, double *evals, double *evecs) {
    SA_API_BEGIN
    SA_REQUIRE(count >= 0 && n && A && D && m && evals && evecs, "bad argument");
    const Options opt = g_default_options;
    validate_options(opt);
    hipStream_t s = 0;
    set_thread_stream(s);
    std::vector<int> sizes(n, n + count);
    EigBatch b;
    eig_batch_alloc(b, sizes, opt, s);
    b.set_window(vu);
    b.dense_only = opt.eig_dense_only != 0;
    DBuf<double> dD;
    dD.assign(D, (size_t)b.h_voff[count], s);
    upload_scaled(s, b, A, dD.p);
    eig_tridiagonalize(s, b);
    eig_count(s, b, vl, vu);
    if (b.ss_failed || b.nbad) {     // few-eigenpairs path gave up (on the batch or on some matrices): the dense path on a fresh copy
        b.dense_only = true;
        b.subspace = b.ss_failed = false;
        upload_scaled(s, b, A, dD.p);
        eig_tridiagonalize(s, b);
        eig_count(s, b, vl, vu);
    }
    std::vector<int64_t> eoff((size_t)count + 1, 0), xoff((size_t)count + 1, 0);
    for (int i = 0; i < count; ++i) {
        eoff[i + 1] = eoff[i] + b.h_m[i];
        xoff[i + 1] = xoff[i] + (int64_t)b.h_m[i] * sizes[i];
        m[i] = b.h_m[i];
    }
    DBuf<int64_t> de, dx;
    de.from_host(eoff, s);
    dx.from_host(xoff, s);
    DBuf<double> ev((size_t)eoff[count] + 1), xv((size_t)xoff[count] + 1);
    eig_vectors(s, b, de.p, dx.p, ev.p, xv.p);
    auto hev = ev.to_host(s);
    auto hxv = xv.to_host(s);
    for (int i = 0; i < count; ++i) {
        std::copy(hev.begin() + eoff[i], hev.begin() + eoff[i + 1], evals + b.h_voff[i]);
        std::copy(hxv.begin() + xoff[i], hxv.begin() + xoff[i + 1], evecs + b.h_moff[i]);
    }
    SA_API_END
}

int saamge_amd_inertia_batched(int count, const int *n, const double *A, const double *D, double vu, int *neg) {
    SA_API_BEGIN
    SA_REQUIRE(count >= 0 && n && A && D && neg, "bad argument");
    const Options opt = g_default_options;
    validate_options(opt);
    hipStream_t s = 0;
    set_thread_stream(s);
    std::vector<int> sizes(n, n + count);
    EigBatch b;
    eig_batch_alloc(b, sizes, opt, s);
    b.set_window(vu);
    DBuf<double> dD;
    dD.assign(D, (size_t)b.h_voff[count], s);
    upload_scaled(s, b, A, dD.p);
    (void)eig_subspace_factor(s, b);      // (the inertia pass runs ahead of the Cholesky factorisation)
    SA_REQUIRE((int)b.h_inertia.size() == count, "the inertia pass is switched off");
    std::copy(b.h_inertia.begin(), b.h_inertia.end(), neg);
    SA_API_END
}

void saamge_amd_release_cached_memory(void) {
    (void)hipDeviceSynchronize();
    eig_arena_release();
    dev_pool_release();
    pinned_pool_release();      // the idle page-locked blocks as well (not counted by saamge_amd_cached_memory_bytes)
}
long long saamge_amd_cached_memory_bytes(void) { return (long long)dev_pool_idle_bytes(); }
void saamge_amd_memory_stats(long long *live_bytes, long long *peak_bytes, int reset_peak) {
    size_t l = 0, pk = 0;
    dev_memory_stats(&l, &pk, reset_peak != 0);
    if (live_bytes) *live_bytes = (long long)l;
    if (peak_bytes) *peak_bytes = (long long)pk;
}
void saamge_amd_pool_counts(long long counts[4], int reset) {
    long nm = 0, nf = 0;
    size_t mb = 0;
    dev_pool_counts(&nm, &nf, &mb, reset != 0);
    if (counts) { counts[0] = nm; counts[1] = (long long)mb; counts[2] = nf; counts[3] = (long long)dev_pool_idle_bytes(); }
}

void saamge_amd_profile_enable(int on) { profiler().enabled = on != 0; }
void saamge_amd_profile_reset(void) { profiler().stats.clear(); }
int saamge_amd_profile_count(void) { return (int)profiler().stats.size(); }
int saamge_amd_profile_get(int i, char *name, int name_len, double *ms, long long *launches,
                           double *bytes, double *flops) {
    if (i < 0 || i >= (int)profiler().stats.size()) return 1;
    const KernelStat &k = profiler().stats[i];
    if (name && name_len > 0) {
        std::snprintf(name, (size_t)name_len, "%s", k.name.c_str());
    }
    if (ms) *ms = k.ms;
    if (launches) *launches = k.launches;
    if (bytes) *bytes = k.bytes;
    if (flops) *flops = k.flops;
    return 0;
}

// the same with the bytes of the format in use (KernelStat::fmt_bytes) and, for the SpMV family, the operator's slice census
int saamge_amd_profile_get2(int i, char *name, int name_len, double *ms, long long *launches, double *bytes, double *flops,
                            double *fmt_bytes) {
    if (saamge_amd_profile_get(i, name, name_len, ms, launches, bytes, flops)) return 1;
    if (fmt_bytes) *fmt_bytes = profiler().stats[i].fmt_bytes;
    return 0;
}

// ---- partitions from a graph / a mesh (partition.hip) ------------------------------------------------------------------
static PartitionOptions convert_partition_options(const saamge_amd_partition_options_v2 *o) {
    PartitionOptions p;
    if (o) { p.min_shared = o->min_shared; p.lloyd_iters = o->lloyd_iters; p.max_size = o->max_size; p.min_size = o->min_size; p.seed = o->seed; p.seeding = o->seeding; p.growth = o->growth; }
    SA_REQUIRE(p.seeding == 0 || p.seeding == 1, "partition options: seeding must be 0 or 1");
    SA_REQUIRE(p.growth == 0 || p.growth == 1, "partition options: growth must be 0 or 1");
    return p;
}
// the entry points without _v2: the same fields, growth = 0
struct PartitionOptionsV1 {
    saamge_amd_partition_options_v2 v2;
    bool given;
    explicit PartitionOptionsV1(const saamge_amd_partition_options *o) : given(o != nullptr) {
        if (o) v2 = {o->min_shared, o->lloyd_iters, o->max_size, o->min_size, o->seed, o->seeding, 0};
    }
    const saamge_amd_partition_options_v2 *ptr() const { return given ? &v2 : nullptr; }
};

void saamge_amd_partition_options_default(saamge_amd_partition_options *o) {
    const PartitionOptions p;
    o->min_shared = p.min_shared; o->lloyd_iters = p.lloyd_iters; o->max_size = p.max_size; o->min_size = p.min_size; o->seed = p.seed; o->seeding = p.seeding;
}
void saamge_amd_partition_options_v2_default(saamge_amd_partition_options_v2 *o) {
    const PartitionOptions p;
    o->min_shared = p.min_shared; o->lloyd_iters = p.lloyd_iters; o->max_size = p.max_size; o->min_size = p.min_size; o->seed = p.seed; o->seeding = p.seeding; o->growth = p.growth;
}

// The counts of the calling thread's last partition and its last refinement pass, for the three _info calls.  The device layer
// zeroes the partition's record when it accepts its arguments and fills it as it goes; the refinement's record is zeroed here
// before a pass is entered and set when it returns, so a pass that throws leaves zeros.  A call refused before it reaches the
// device layer leaves both as they were.
static thread_local PartitionStats t_partition_stats;
static thread_local RefineStats t_refine_stats;

void saamge_amd_partition_seeding_info(long long info[4]) {
    const SeedingStats st = t_partition_stats.seeding;
    info[0] = st.radius; info[1] = st.rounds; info[2] = st.seeds_first; info[3] = st.seeds;
}

void saamge_amd_partition_growth_info(long long info[4]) {
    const GrowthStats st = t_partition_stats.growth;
    info[0] = st.rounds; info[1] = st.quota_nodes; info[2] = st.open_parts; info[3] = st.released_nodes;
}

// a caller's graph on the device, checked: host columns need host offsets, which are checked before they say how much to copy
static void import_graph(hipStream_t s, int n, const long long *xadj, const int *adj, DBuf<roff_t> &dx, DBuf<int> &da) {
    DevIn<roff_t> in_x((const roff_t *)xadj, (size_t)n + 1, s);
    dx = in_x.take();
    if (!is_device_ptr(adj)) {
        const bool xh = !in_x.on_device;
        if (xh) for (int i = 0; i < n; ++i) SA_REQUIRE(xadj[0] == 0 && xadj[i + 1] >= xadj[i], "xadj: must start at 0 and ascend");
        const roff_t nnz = n == 0 ? 0 : (xh ? (roff_t)xadj[n] : 0);
        SA_REQUIRE(xh || n == 0, "xadj on the device with adj on the host");
        SA_REQUIRE(nnz == 0 || adj, "null argument: adj");
        da.assign(adj, (size_t)nnz, s);
    } else {
        da.view(const_cast<int *>(adj), 0);
    }
    check_graph_device(s, n, dx.p, da.p);
}

void saamge_amd_partition_refine_info(long long info[4]) {
    const RefineStats st = t_refine_stats;
    info[0] = st.rounds; info[1] = st.moved; info[2] = st.gain; info[3] = st.converged;
}

int saamge_amd_partition_graph(int n, const long long *xadj, const int *adj, int elems_per_agg,
                               const saamge_amd_partition_options *o, void *stream, int *part, int *nparts_out) {
    const PartitionOptionsV1 v1(o);
    return saamge_amd_partition_graph_v2(n, xadj, adj, elems_per_agg, v1.ptr(), stream, part, nparts_out);
}

int saamge_amd_partition_graph_v2(int n, const long long *xadj, const int *adj, int elems_per_agg,
                                  const saamge_amd_partition_options_v2 *o, void *stream, int *part, int *nparts_out) {
    SA_API_BEGIN
    SA_REQUIRE(n >= 0, "n < 0");
    SA_REQUIRE(elems_per_agg >= 1, "elems_per_agg < 1");
    SA_REQUIRE(xadj && nparts_out && (n == 0 || part), "null argument");
    const PartitionOptions po = convert_partition_options(o);
    hipStream_t s = (hipStream_t)stream;
    ThreadStreamScope scope(s);
    {
        DBuf<roff_t> dx;
        DBuf<int> da;
        import_graph(s, n, xadj, adj, dx, da);
        DevOut<int> dp(part, (size_t)n, s, false);
        partition_graph_device(s, n, dx.p, da.p, elems_per_agg, po, dp.p, nparts_out, &t_partition_stats);
        dp.finish();
    }
    SA_API_END
}

// the refinement pass on a caller's partition (partition.hip): everything is checked, and the work done on a copy, before part
// is written
int saamge_amd_partition_refine(int n, const long long *xadj, const int *adj, int nparts, int *part, int rounds, int max_size,
                                int min_size, unsigned seed, int renumber, void *stream, long long info[4]) {
    SA_API_BEGIN
    SA_REQUIRE(n >= 0, "n < 0");
    SA_REQUIRE(xadj && (n == 0 || part), "null argument");
    SA_REQUIRE(rounds >= 0 && max_size >= 0 && min_size >= 0, "rounds, max_size and min_size must be >= 0");
    SA_REQUIRE(renumber == 0 || renumber == 1, "renumber must be 0 or 1");
    SA_REQUIRE(nparts >= 0 && nparts <= n && (nparts > 0 || n == 0), "nparts outside [1, n]");
    hipStream_t s = (hipStream_t)stream;
    ThreadStreamScope scope(s);
    {
        DBuf<roff_t> dx;
        DBuf<int> da, lab((size_t)n), out;
        import_graph(s, n, xadj, adj, dx, da);
        upload(lab.p, (const int *)part, (size_t)n, s);
        check_partition_device(s, n, lab.p, nparts);
        t_refine_stats = RefineStats();
        const RefineStats st = t_refine_stats = refine_partition_device(s, n, dx.p, da.p, nparts, lab.p, rounds, max_size, min_size, seed);
        const int *result = lab.p;
        if (renumber && n) {
            int np = 0;
            out.alloc((size_t)n);
            renumber_device(s, n, lab.p, nparts, out.p, &np);
            result = out.p;
        }
        copy_to_caller(part, result, (size_t)n, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        if (info) { info[0] = st.rounds; info[1] = st.moved; info[2] = st.gain; info[3] = st.converged; }
    }
    SA_API_END
}

int saamge_amd_partition_mesh(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                              const int *elems_per_agg, const saamge_amd_partition_options *o, void *stream,
                              saamge_amd_partitioning **out) {
    const PartitionOptionsV1 v1(o);
    return saamge_amd_partition_mesh_v2(NE, nde, elem_ptr, elem_to_dof, ND, num_coarsenings, elems_per_agg, v1.ptr(), stream, out);
}

int saamge_amd_partition_mesh_v2(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                                 const int *elems_per_agg, const saamge_amd_partition_options_v2 *o, void *stream,
                                 saamge_amd_partitioning **out) {
    return saamge_amd_partition_mesh_refined(NE, nde, elem_ptr, elem_to_dof, ND, num_coarsenings, elems_per_agg, o, nullptr, stream, out);
}

int saamge_amd_partition_mesh_refined(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND, int num_coarsenings,
                                      const int *elems_per_agg, const saamge_amd_partition_options_v2 *o, const int *refine_rounds,
                                      void *stream, saamge_amd_partitioning **out) {
    SA_API_BEGIN
    SA_REQUIRE(out && elems_per_agg && (NE == 0 || elem_to_dof), "null argument");
    SA_REQUIRE(NE >= 0 && ND >= 0, "NE < 0 or ND < 0");
    SA_REQUIRE(elem_ptr || nde >= 1, "elem_ptr or a uniform nde >= 1 is needed");
    SA_REQUIRE(num_coarsenings >= 1 && num_coarsenings < SAAMGE_AMD_MAX_LEVELS, "num_coarsenings out of range");
    for (int k = 0; k < num_coarsenings; ++k) SA_REQUIRE(elems_per_agg[k] >= 1, "elems_per_agg < 1");
    for (int k = 0; refine_rounds && k < num_coarsenings; ++k) SA_REQUIRE(refine_rounds[k] >= 0, "refine_rounds < 0");
    const PartitionOptions po = convert_partition_options(o);
    hipStream_t s = (hipStream_t)stream;
    ThreadStreamScope scope(s);
    std::unique_ptr<saamge_amd_partitioning> P(new saamge_amd_partitioning);
    P->device = current_device();
    {
        DBuf<int> eI, eJ;
        if (elem_ptr) {
            eI = DevIn<int>(elem_ptr, (size_t)NE + 1, s).take();
        } else {
            SA_REQUIRE((int64_t)NE * nde < INT_MAX, "NE * nde beyond 32 bits");
            std::vector<int> h((size_t)NE + 1);
            for (int e = 0; e <= NE; ++e) h[(size_t)e] = e * nde;
            eI.from_host(h, s);
        }
        if (!is_device_ptr(elem_to_dof) && NE) {   // the offsets say how much to copy: checked first
            const auto hI = eI.to_host(s);
            for (int e = 0; e < NE; ++e) SA_REQUIRE(hI[0] == 0 && hI[(size_t)e + 1] > hI[(size_t)e], "elem_ptr: must start at 0 and every element needs a dof");
            eJ.assign(elem_to_dof, (size_t)hI[(size_t)NE], s);
        } else {
            eJ.view(const_cast<int *>(elem_to_dof), 0);
        }
        check_mesh_device(s, NE, eI.p, eJ.p, ND);
        P->xadj.emplace_back();
        P->adj.emplace_back();
        element_graph_device(s, NE, eI.p, eJ.p, ND, po.min_shared, P->xadj[0], P->adj[0]);
        SA_HIP_CHECK(hipStreamSynchronize(s));
    }
    int n = NE;
    for (int k = 0; k < num_coarsenings; ++k) {
        P->part.emplace_back((size_t)n);
        int np = 0;
        partition_graph_device(s, n, P->xadj[(size_t)k].p, P->adj[(size_t)k].p, elems_per_agg[k], po, P->part.back().p, &np,
                               &t_partition_stats);
        if (refine_rounds) t_refine_stats = RefineStats();   // a level without rounds reports zeros; NULL leaves the record alone
        if (refine_rounds && refine_rounds[k] > 0 && n) {   // on the numbered parts, which are numbered again afterwards
            int max_size = 0, min_size = 0;
            resolve_partition_sizes(elems_per_agg[k], po, &max_size, &min_size);
            DBuf<int> lab((size_t)n);
            copy_device(lab.p, (const int *)P->part.back().p, (size_t)n, s);
            t_refine_stats = refine_partition_device(s, n, P->xadj[(size_t)k].p, P->adj[(size_t)k].p, np, lab.p, refine_rounds[k],
                                                     max_size, min_size, po.seed);
            renumber_device(s, n, lab.p, np, P->part.back().p, &np);
        }
        P->n_elem.push_back(n);
        P->nparts.push_back(np);
        P->part_host.push_back(P->part.back().to_host(s));
        P->xadj.emplace_back();
        P->adj.emplace_back();
        quotient_graph_device(s, n, P->xadj[(size_t)k].p, P->adj[(size_t)k].p, P->part.back().p, np, P->xadj.back(), P->adj.back());
        n = np;
    }
    for (size_t k = 0; k < P->part.size(); ++k) {
        P->part_ptr.push_back(P->part[k].p);
        P->part_host_ptr.push_back(P->part_host[k].data());
    }
    for (size_t k = 0; k < P->xadj.size(); ++k) P->nnz.push_back((int64_t)P->adj[k].n);
    *out = P.release();
    SA_API_END
}

int saamge_amd_partitioning_arrays(const saamge_amd_partitioning *p, int on_host, const int *const **partitions,
                                   const int **nparts_host) {
    SA_API_BEGIN
    SA_REQUIRE(p, "null argument");
    if (partitions) *partitions = on_host ? p->part_host_ptr.data() : p->part_ptr.data();
    if (nparts_host) *nparts_host = p->nparts.data();
    SA_API_END
}

int saamge_amd_partitioning_get(const saamge_amd_partitioning *p, int level, int *part_host, int *n_elem, int *nparts) {
    SA_API_BEGIN
    SA_REQUIRE(p, "null argument");
    SA_REQUIRE(level >= 0 && level < (int)p->part.size(), "level out of range");
    const hvec<int> &h = p->part_host[(size_t)level];
    if (part_host && !h.empty()) std::memcpy(part_host, h.data(), h.size() * sizeof(int));
    if (n_elem) *n_elem = p->n_elem[(size_t)level];
    if (nparts) *nparts = p->nparts[(size_t)level];
    SA_API_END
}

int saamge_amd_partitioning_graph(const saamge_amd_partitioning *p, int level, long long *xadj, int *adj, int *n,
                                  long long *nnz) {
    SA_API_BEGIN
    SA_REQUIRE(p, "null argument");
    SA_REQUIRE(level >= 0 && level < (int)p->xadj.size(), "level out of range");
    SA_REQUIRE(current_device() == p->device, "the calling thread's current HIP device is not the partitioning's device");
    const size_t l = (size_t)level;
    const size_t nn = p->xadj[l].n - 1;
    if (n) *n = (int)nn;
    if (nnz) *nnz = p->nnz[l];
    copy_to_caller((roff_t *)xadj, (const roff_t *)p->xadj[l].p, nn + 1, nullptr);
    copy_to_caller(adj, (const int *)p->adj[l].p, (size_t)p->nnz[l], nullptr);
    SA_API_END
}

void saamge_amd_partitioning_free(saamge_amd_partitioning *p) { delete p; }

// ---- the operator assembled on the device (operator.hip) ---------------------------------------------------------------
static void require_operator_device(const AssembledOperator &op) {
    SA_REQUIRE(current_device() == op.device, "the calling thread's current HIP device is not the operator's device");
}

int saamge_amd_operator_assemble(int n, int NE, int nde, const int *elem_ptr, const int *elem_to_dof,
                                 const double *elmat, const signed char *bdr_dofs, void *stream,
                                 saamge_amd_operator **out) {
    SA_API_BEGIN
    SA_REQUIRE(out, "null argument");
    hipStream_t s = (hipStream_t)stream;
    ThreadStreamScope scope(s);
    std::unique_ptr<saamge_amd_operator> P(new saamge_amd_operator);
    operator_assemble(s, n, NE, nde, elem_ptr, elem_to_dof, elmat, bdr_dofs, g_operator_limits, P->op);
    *out = P.release();
    SA_API_END
}

int saamge_amd_operator_arrays(const saamge_amd_operator *op, const long long **rowptr_dev, const int **col_dev,
                               const double **val_dev, long long *nnz) {
    SA_API_BEGIN
    SA_REQUIRE(op, "null argument");
    if (rowptr_dev) *rowptr_dev = (const long long *)op->op.rowptr.p;
    if (col_dev) *col_dev = op->op.col.p;
    if (val_dev) *val_dev = op->op.val.p;
    if (nnz) *nnz = (long long)op->op.nnz;
    SA_API_END
}

int saamge_amd_operator_get(const saamge_amd_operator *op, long long *rowptr, int *col, double *val, long long *nnz) {
    SA_API_BEGIN
    SA_REQUIRE(op, "null argument");
    const AssembledOperator &o = op->op;
    require_operator_device(o);
    if (nnz) *nnz = (long long)o.nnz;
    // (on the null stream, as the other getters of handles)
    copy_to_caller((roff_t *)rowptr, (const roff_t *)o.rowptr.p, (size_t)o.n + 1, nullptr);
    copy_to_caller(col, (const int *)o.col.p, (size_t)o.nnz, nullptr);
    copy_to_caller(val, (const double *)o.val.p, (size_t)o.nnz, nullptr);
    SA_API_END
}

int saamge_amd_operator_update(saamge_amd_operator *op, const double *elmat) {
    SA_API_BEGIN
    SA_REQUIRE(op, "null argument");
    require_operator_device(op->op);
    ThreadStreamScope scope(op->op.stream);
    operator_numeric(op->op, elmat);
    SA_API_END
}

int saamge_amd_operator_eliminate_rhs(const saamge_amd_operator *op, const double *elmat, const double *x_ess, double *b) {
    SA_API_BEGIN
    SA_REQUIRE(op && x_ess && b, "null argument");
    const AssembledOperator &o = op->op;
    require_operator_device(o);
    ThreadStreamScope scope(o.stream);
    {
        VecIn vx(x_ess, (size_t)o.n, o.stream);
        VecOut vb(b, (size_t)o.n, o.stream, true);
        operator_eliminate_rhs(o, elmat, vx.p, vb.p);
        vb.finish();
    }
    SA_API_END
}

int saamge_amd_operator_assemble_rhs(const saamge_amd_operator *op, const double *elvec, double *b) {
    SA_API_BEGIN
    SA_REQUIRE(op && b, "null argument");
    const AssembledOperator &o = op->op;
    require_operator_device(o);
    ThreadStreamScope scope(o.stream);
    {
        VecOut vb(b, (size_t)o.n, o.stream, false);
        operator_assemble_rhs(o, elvec, vb.p);
        vb.finish();
    }
    SA_API_END
}

int saamge_amd_operator_path_counts(const saamge_amd_operator *op, long long counts[6]) {
    SA_API_BEGIN
    SA_REQUIRE(op && counts, "null argument");
    for (int k = 0; k < 3; ++k) { counts[k] = op->op.sym_count[k]; counts[3 + k] = op->op.num_count[k]; }
    SA_API_END
}

int saamge_amd_operator_set_path_limits(int short_candidates, int lds_candidates) {
    SA_API_BEGIN
    OperatorLimits l;
    if (short_candidates >= 0) l.short_cand = short_candidates;
    if (lds_candidates >= 0) l.lds_cand = lds_candidates;
    SA_REQUIRE(l.short_cand <= OP_SHORT_CAND && l.lds_cand <= OP_LDS_CAND,
               "operator path limits: at most 64 candidates for the short path and 4096 for the LDS path");
    g_operator_limits = l;
    SA_API_END
}

void saamge_amd_operator_free(saamge_amd_operator *op) {
    if (!op) return;
    {   // the blocks go back to the cache ordered after the operator's stream; the caller may destroy the stream next
        hipStream_t s = op->op.stream;
        ThreadStreamScope scope(s);
        delete op;
        dev_pool_close_stream(s);
    }
}

// ---- lowest eigenpairs (lobpcg.hip) and its block kernels on their own (blockvec.hip) ------------------------------------
void saamge_amd_lobpcg_options_default(saamge_amd_lobpcg_options *o) {
    if (!o) return;
    o->nev = 1;
    o->block = 0;
    o->tol = 1e-8;
    o->max_iter = 100;
    o->constrain_essential = 1;
    o->seed = 0;
}

int saamge_amd_lobpcg(saamge_amd_hierarchy *h, const long long *Mrowptr, const int *Mcol, const double *Mval,
                      const saamge_amd_lobpcg_options *o, const double *x0, double *evals, double *evecs,
                      double *res, int *iters, int *converged, double *hist) {
    SA_API_BEGIN
    SA_REQUIRE(h, "lobpcg: null argument: h");
    SA_REQUIRE(o, "lobpcg: null argument: o");
    SA_REQUIRE(evals, "lobpcg: null argument: evals");
    SA_REQUIRE(evecs, "lobpcg: null argument: evecs");
    LobpcgOptions lo;
    SA_REQUIRE(o->nev >= 1 && o->nev <= BV_MAX_NORMS, "lobpcg: nev must lie in 1 .. 16");
    SA_REQUIRE(o->block == 0 || (o->block >= o->nev && o->block <= BV_MAX_NORMS), "lobpcg: block must be 0 or lie in nev .. 16");
    SA_REQUIRE(std::isfinite(o->tol) && o->tol > 0.0, "lobpcg: tol must be positive");
    SA_REQUIRE(o->max_iter >= 0, "lobpcg: max_iter must not be negative");
    lo.nev = o->nev;
    lo.nb = o->block ? o->block : o->nev;
    lo.tol = o->tol;
    lo.max_iter = o->max_iter;
    lo.constrain_essential = o->constrain_essential != 0;
    lo.seed = o->seed;
    Hierarchy &H = *h->H;
    require_device(H);
    Level &L0 = *H.levels[0];
    SA_REQUIRE(!L0.dist.on, "lobpcg: h: level 0 is row-partitioned over several ranks (multi-rank is not supported)");
    hipStream_t s = H.stream;
    const int n = L0.A.nrows;
    long nfree = n;
    if (lo.constrain_essential) {
        fetch_relations_ae_host(L0.rel, L0.drel, s);
        SA_REQUIRE((int)L0.rel.agg_flags.size() == n && (int)L0.drel.flags.n == n, "lobpcg: h: the hierarchy holds no flags of its rows");
        for (signed char f : L0.rel.agg_flags) nfree -= (f & FLAG_ON_ESS_BORDER) ? 1 : 0;
    }
    SA_REQUIRE(3L * lo.nb <= nfree, "lobpcg: block: 3 nb exceeds the number of unconstrained rows");
    DCsr M;
    if (Mrowptr) {
        SA_REQUIRE(Mcol && Mval, "lobpcg: Mcol, Mval: null with row offsets given");
        const hvec<long long> rp = fetch_host(Mrowptr, (size_t)n + 1, s);
        SA_REQUIRE(rp[0] == 0, "lobpcg: Mrowptr: the row offsets must start at 0");
        for (int i = 0; i < n; ++i) SA_REQUIRE(rp[i + 1] >= rp[i], "lobpcg: Mrowptr: the row offsets must not decrease");
        const hvec<int> cols = fetch_host(Mcol, (size_t)rp[n], s);
        for (int c : cols) SA_REQUIRE(c >= 0 && c < n, "lobpcg: Mcol: a column index outside [0, n)");
        M.nrows = M.ncols = n;
        M.nnz = rp[n];
        import_rowptr(M.rowptr, Mrowptr, 64, (size_t)n + 1, s);
        M.col = DevIn<int>(Mcol, (size_t)M.nnz, s).take();
        M.val = DevIn<double>(Mval, (size_t)M.nnz, s).take();
        M.lanes_per_row = pick_lanes_per_row(M.nnz, n);
    }
    DevIn<double> start;
    start.bind(x0, (size_t)n * lo.nb, s);
    std::vector<double> ev(lo.nev), rs(lo.nev);
    int it = 0, conv = 0;
    {
        VecOut vx(evecs, (size_t)n * lo.nev, s, false);
        lobpcg_solve(H, Mrowptr ? &M : nullptr, lo, start.p, ev.data(), vx.p, rs.data(), &it, &conv, hist);
        vx.finish();
    }
    std::copy(ev.begin(), ev.end(), evals);
    if (res) std::copy(rs.begin(), rs.end(), res);
    if (iters) *iters = it;
    if (converged) *converged = conv;
    SA_API_END
}

// a column-major block (rows x cols, leading dimension ld) of a host or device pointer, on the device
static size_t block_extent(int rows, int cols, long long ld) { return (size_t)(cols - 1) * (size_t)ld + (size_t)rows; }

int saamge_amd_blockvec_gram(int n, int p, const double *S, long long lds, int q, const double *T, long long ldt, double *G_host) {
    SA_API_BEGIN
    SA_REQUIRE(S && T && G_host, "blockvec_gram: null argument");
    SA_REQUIRE(n >= 1, "blockvec_gram: n must be positive");
    SA_REQUIRE(p >= 1 && p <= BV_MAX_COLS, "blockvec_gram: p must lie in 1 .. 48");
    SA_REQUIRE(q >= 1 && q <= BV_MAX_COLS, "blockvec_gram: q must lie in 1 .. 48");
    SA_REQUIRE(lds >= n, "blockvec_gram: lds is below n");
    SA_REQUIRE(ldt >= n, "blockvec_gram: ldt is below n");
    hipStream_t s = 0;
    set_thread_stream(s);
    VecIn vs(S, block_extent(n, p, lds), s);
    const bool same = T == S && ldt == lds && q == p;
    std::unique_ptr<VecIn> vt(same ? nullptr : new VecIn(T, block_extent(n, q, ldt), s));
    DBuf<double> scratch(bv_gram_scratch(n, p, q)), G((size_t)p * q);
    bv_gram(s, n, p, vs.p, (long)lds, q, same ? vs.p : vt->p, (long)ldt, scratch.p, G.p);
    read_back(G_host, G.p, (size_t)p * q, s);
    SA_API_END
}

int saamge_amd_blockvec_combine(int n, int p, const double *S, long long lds, int q, const double *C_host, double *Y,
                                long long ldy, int accumulate) {
    SA_API_BEGIN
    SA_REQUIRE(S && C_host && Y, "blockvec_combine: null argument");
    SA_REQUIRE(n >= 1, "blockvec_combine: n must be positive");
    SA_REQUIRE(p >= 1 && p <= BV_MAX_COLS, "blockvec_combine: p must lie in 1 .. 48");
    SA_REQUIRE(q >= 1 && q <= BV_MAX_COLS, "blockvec_combine: q must lie in 1 .. 48");
    SA_REQUIRE(lds >= n, "blockvec_combine: lds is below n");
    SA_REQUIRE(ldy >= n, "blockvec_combine: ldy is below n");
    SA_REQUIRE(bv_combine_aliasing_ok(n, p, S, (long)lds, q, Y, (long)ldy),
               "blockvec_combine: Y overlaps S without being S itself (the same pointer and leading dimension)");
    hipStream_t s = 0;
    set_thread_stream(s);
    const bool in_place = Y == S;
    // in place the block is max(p, q) columns wide: one buffer that is read as S and written as Y
    VecOut vy(Y, block_extent(n, in_place ? std::max(p, q) : q, ldy), s, accumulate != 0 || in_place || ldy > n);
    std::unique_ptr<VecIn> vs(in_place ? nullptr : new VecIn(S, block_extent(n, p, lds), s));
    DBuf<double> C;
    C.assign(C_host, (size_t)p * q, s);
    BvBlocks B{{in_place ? vy.p : vs->p, nullptr, nullptr}, {vy.p, nullptr, nullptr}, 1};
    bv_combine(s, n, p, q, C.p, accumulate != 0, B, (long)lds, (long)ldy);
    vy.finish();
    SA_API_END
}

// ---- block solves: k columns per call (cycle.hip) ---------------------------------------------------------
// What every block call refuses, before any HIP call and before anything is written.
static void require_blocks(const char *who, int k, long long nb, const double *B, long long ldb, long long nx, const double *X,
                           long long ldx) {
    const std::string w(who);
    SA_REQUIRE(k >= 1 && k <= 64, w + ": k must lie in 1 .. 64");
    SA_REQUIRE(B && X, w + ": null block");
    SA_REQUIRE(ldb >= nb && ldx >= nx, w + ": a leading dimension is below the row count");
    const double *Be = B + block_extent((int)nb, k, ldb), *Xe = X + block_extent((int)nx, k, ldx);
    SA_REQUIRE(Xe <= B || Be <= X, w + ": X overlaps B");
}
static Hierarchy &block_hierarchy(const char *who, saamge_amd_hierarchy *h) {
    SA_REQUIRE(h && h->H, std::string(who) + ": null hierarchy");
    for (auto &L : h->H->levels)
        SA_REQUIRE(!L->dist.on, std::string(who) + ": the hierarchy is row-partitioned over several ranks (block solves are not available)");
    return *h->H;
}
// the blocks of a call on the device: a host block is staged whole (rows past the row count come home as they went)
struct BlockArgs {
    VecIn vb;
    VecOut vx;
    std::vector<double *> b, x;
    BlockArgs(int n, int k, const double *B, long long ldb, double *X, long long ldx, bool load, hipStream_t s)
        : vb(B, block_extent(n, k, ldb), s), vx(X, block_extent(n, k, ldx), s, load || ldx > n),
          b(block_columns(vb.p, (long)ldb, k)), x(block_columns(vx.p, (long)ldx, k)) {}
};

int saamge_amd_spmv_block(int nrows, int ncols, const int *rowptr, const int *col, const double *val, int k, const double *X,
                          long long ldx, double *Y, long long ldy) {
    SA_API_BEGIN
    SA_REQUIRE(rowptr && col && val && nrows >= 0 && ncols >= 0, "spmv_block: bad argument");
    require_blocks("spmv_block", k, ncols, X, ldx, nrows, Y, ldy);
    const Options opt = g_default_options;
    validate_options(opt);
    hipStream_t s = 0;
    set_thread_stream(s);
    DCsr A;
    A.nrows = nrows;
    A.ncols = ncols;
    import_rowptr(A.rowptr, rowptr, 32, (size_t)nrows + 1, s);
    A.nnz = read_one(A.rowptr.p + nrows, s);
    A.col = DevIn<int>(col, (size_t)A.nnz, s).take();
    A.val = DevIn<double>(val, (size_t)A.nnz, s).take();
    A.lanes_per_row = pick_lanes_per_row(A.nnz, nrows > 0 ? nrows : 1);
    if (nrows == ncols && opt.spmv_sell) build_sell(s, A, opt);      // (as saamge_amd_spmv)
    VecIn vx(X, block_extent(ncols, k, ldx), s);
    VecOut vy(Y, block_extent(nrows, k, ldy), s, ldy > nrows);
    for (int c = 0; c < block_num_chunks(k); ++c) {
        const BlockChunk ch = block_chunk(k, c);
        spmv_block(s, A, Cols(vx.p + (size_t)ch.first * ldx, (long)ldx, ch.count), Cols(vy.p + (size_t)ch.first * ldy, (long)ldy, ch.count));
    }
    vy.finish();
    SA_API_END
}

int saamge_amd_smoother_block(saamge_amd_hierarchy *h, int level, int k, const double *B, long long ldb, double *X, long long ldx) {
    SA_API_BEGIN
    Hierarchy &H = block_hierarchy("smoother_block", h);
    SA_REQUIRE(level >= 0 && level < (int)H.levels.size(), "smoother_block: bad level");
    const int n = H.levels[level]->A.nrows;
    require_blocks("smoother_block", k, n, B, ldb, n, X, ldx);
    require_device(H);
    BlockArgs a(n, k, B, ldb, X, ldx, true, H.stream);
    smoother_apply_block(H, level, k, a.b.data(), a.x.data());
    a.vx.finish();
    SA_API_END
}

int saamge_amd_vcycle_block(saamge_amd_hierarchy *h, int k, const double *B, long long ldb, double *X, long long ldx, int iterative_mode) {
    SA_API_BEGIN
    Hierarchy &H = block_hierarchy("vcycle_block", h);
    const int n = H.levels[0]->A.nrows;
    require_blocks("vcycle_block", k, n, B, ldb, n, X, ldx);
    require_device(H);
    BlockArgs a(n, k, B, ldb, X, ldx, iterative_mode != 0, H.stream);
    if (iterative_mode) vcycle_iterate_block(H, k, a.b.data(), a.x.data());
    else vcycle_apply_block(H, k, a.b.data(), a.x.data());
    a.vx.finish();
    SA_API_END
}

int saamge_amd_pcg_block(saamge_amd_hierarchy *h, int k, const double *B, long long ldb, double *X, long long ldx, double rel_tol,
                         double abs_tol, int max_iter, int squared_tol, int zero_guess, int *iters, int *converged, double *hist) {
    SA_API_BEGIN
    Hierarchy &H = block_hierarchy("pcg_block", h);
    const int n = H.levels[0]->A.nrows;
    require_blocks("pcg_block", k, n, B, ldb, n, X, ldx);
    SA_REQUIRE(iters, "pcg_block: null argument: iters");
    require_device(H);
    BlockArgs a(n, k, B, ldb, X, ldx, !zero_guess, H.stream);
    pcg_solve_block(H, k, a.b.data(), a.x.data(), rel_tol, abs_tol, max_iter, squared_tol, zero_guess, iters, converged, hist);
    a.vx.finish();
    SA_API_END
}

}  // extern "C"
