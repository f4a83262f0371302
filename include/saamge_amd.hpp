// saamge_amd.hpp -- C++ host-side mirror of the SAAMGE solver/operator API for the hot path,
// implemented as thin adaptors over the C ABI (saamge_amd.h).
//
// Two layers:
//   1. namespace saamge_amd::api (this file) -- always available, raw arrays, same names / argument
//      order / error behaviour (negative iteration count on failure, inc/tg.hpp:291-293) as the
//      reference's free functions: MultilevelParameters, ml_produce_data, ml_free_data,
//      VCycleSolver::Mult, smpr_sym_poly, kalchev_pcg, adapt_update_operators.
//   2. namespace saamge (saamge_amd_mfem.hpp, included from here when SAAMGE_AMD_WITH_MFEM is
//      defined, i.e. where <mfem.hpp> and hypre exist -- not in the build container): the
//      reference's own types and entry points -- agg_partitioning_relations_t,
//      ElementMatrixProvider, MultilevelParameters, tg_data_t, ml_data_t, ml_produce_data,
//      tg_produce_data, VCycleSolver, SpectralAMGSolver, kalchev_pcg -- so that an amg/test driver
//      compiles and links against this library for the setup + solve path.
#ifndef SAAMGE_AMD_HPP
#define SAAMGE_AMD_HPP

#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "saamge_amd.h"

namespace saamge_amd {
namespace api {

// == MultilevelParameters (inc/ml.hpp:59-114): the reference's 11-argument constructor
// (inc/ml.hpp:66-70, src/ml.cpp:54-91), same argument order and getters.
class MultilevelParameters {
public:
    MultilevelParameters(int coarsenings, int *nparts_arr, int first_nu_pro, int nu_pro, int nu_relax,
                         double first_theta, double theta, int polynomial_coarse_space,
                         bool use_correct_nullspace, bool use_arpack, bool do_aggregates)
        : nparts_(nparts_arr, nparts_arr + coarsenings), polynomial_coarse_space_(coarsenings, polynomial_coarse_space),
          use_arpack_(use_arpack), use_double_cycle_(false), coarse_direct_(false) {
        if (coarsenings < 1 || coarsenings >= SAAMGE_AMD_MAX_LEVELS)
            throw std::invalid_argument("MultilevelParameters: 1 <= coarsenings < SAAMGE_AMD_MAX_LEVELS");
        saamge_amd_params_default(&p);
        p.num_coarsenings = coarsenings;
        for (int i = 0; i < coarsenings; ++i) {
            p.theta[i] = i ? theta : first_theta;
            p.nu_pro[i] = i ? nu_pro : first_nu_pro;
            p.nu_relax[i] = nu_relax;
        }
        p.correct_nullspace = use_correct_nullspace ? 1 : 0;   // CorrectNullspace on scaling_P (src/ml.cpp:225-236)
        p.do_aggregates = do_aggregates ? 1 : 0;               // src/ml.cpp:149
        p.avoid_ess_bdr_dofs = 1;                              // src/ml.cpp:64
        // use_arpack: the reference switches to ARPACK above ARPACK_SIZE_THRESHOLD (inc/interp.hpp:104);
        // this library always solves the local problems with its own batched eigensolver (same pairs).
        // polynomial_coarse_space >= 0 asks for ExtendWithPolynomials / ExtendWithRBMs: the modes need the
        // dof coordinates, so they are passed already evaluated through set_extra_coarse_modes(); a
        // non-negative order without modes is refused at ml_produce_data.
    }
    int get_num_coarsenings() const { return p.num_coarsenings; }
    int get_nu_pro(int j) const { return p.nu_pro[j]; }
    int get_nu_relax(int j) const { return p.nu_relax[j]; }
    double get_theta(int j) const { return p.theta[j]; }
    bool get_smooth_interp(int j) const { return p.nu_pro[j] > 0; }
    int get_polynomial_coarse_space(int j) const { return polynomial_coarse_space_[j]; }
    bool get_use_correct_nullspace() const { return p.correct_nullspace != 0; }
    bool get_use_arpack() const { return use_arpack_; }
    bool get_do_aggregates() const { return p.do_aggregates != 0; }
    int get_nparts(int j) const { return nparts_[j]; }
    bool get_avoid_ess_bdr_dofs() const { return p.avoid_ess_bdr_dofs != 0; }
    bool get_use_double_cycle() const { return use_double_cycle_; }
    double get_smooth_drop_tol() const { return p.smooth_drop_tol; }
    void set_polynomial_coarse_space(int j, int val) { polynomial_coarse_space_[j] = val; }
    void set_use_double_cycle(bool use) {
        if (use) throw std::invalid_argument("MultilevelParameters: the double cycle is outside the hot path (SURVEY section 2)");
        use_double_cycle_ = use;
    }
    bool get_coarse_direct() const { return coarse_direct_; }
    void set_coarse_direct(bool cd) { coarse_direct_ = cd; p.coarse_solver = cd ? 1 : 0; }
    void set_smooth_drop_tol(double tol) { p.smooth_drop_tol = tol; }
    // ---- additions of this library ----
    // polynomial / rigid-body coarse-space extension: modes evaluated by the caller, n x count column-major
    void set_extra_coarse_modes(const double *modes, int count) { p.extra_modes = modes; p.num_extra_modes = count; }
    // element-free mode (tg_produce_data_algebraic): pass NE = n, nde = 1 and NULL element arrays
    void set_algebraic(bool on, bool use_window = false) { p.algebraic = on ? (use_window ? 2 : 1) : 0; }
    void set_do_aggregates(bool on) { p.do_aggregates = on ? 1 : 0; }
    void set_eigensolver(int which) { p.eigensolver = which; }      // 0 few-eigenpairs (certified), 1 dense

    saamge_amd_params p;
    const int *nparts_data() const { return nparts_.data(); }

private:
    std::vector<int> nparts_, polynomial_coarse_space_;
    bool use_arpack_, use_double_cycle_, coarse_direct_;
};

// Raw-array view of the reference's setup inputs (HypreParMatrix Ag, elem_to_dof Table,
// ElementMatrixProvider, bdr flags, partitioning arrays).
struct ProblemArrays {
    int n = 0;
    const int *rowptr = nullptr, *col = nullptr;
    const double *val = nullptr;
    int NE = 0, nde = 0;
    const int *elem_to_dof = nullptr;
    const double *elmat = nullptr;
    const signed char *bdr_dofs = nullptr;
    std::vector<const int *> partitions;  // one per coarsening
    // elements of different sizes (saamge_amd_ml_produce_data_mixed): NE + 1 offsets into a flat elem_to_dof, elmat packed
    // in element order; nde is then ignored.  nullptr: every element has nde dofs.
    const int *elem_ptr = nullptr;
};

typedef saamge_amd_hierarchy ml_data_t;  // inc/ml.hpp:118-120

// ml_produce_data (inc/ml.hpp:192-194)
inline ml_data_t *ml_produce_data(const ProblemArrays &a, const MultilevelParameters &mlp, void *stream = nullptr) {
    for (int j = 0; j < mlp.get_num_coarsenings(); ++j)
        if (mlp.get_polynomial_coarse_space(j) >= 0 && mlp.p.num_extra_modes == 0)
            throw std::invalid_argument("polynomial_coarse_space >= 0: pass the evaluated modes with set_extra_coarse_modes()");
    if ((int)a.partitions.size() < mlp.get_num_coarsenings())
        throw std::invalid_argument("ml_produce_data: one partition array per coarsening is required");
    ml_data_t *h = nullptr;
    const int rc = a.elem_ptr
        ? saamge_amd_ml_produce_data_mixed(a.n, a.rowptr, a.col, a.val, a.NE, a.elem_ptr, a.elem_to_dof, a.elmat, a.bdr_dofs,
                                           a.partitions.data(), mlp.nparts_data(), &mlp.p, stream, &h)
        : saamge_amd_ml_produce_data(a.n, a.rowptr, a.col, a.val, a.NE, a.nde, a.elem_to_dof, a.elmat, a.bdr_dofs,
                                     a.partitions.data(), mlp.nparts_data(), &mlp.p, stream, &h);
    if (rc) throw std::runtime_error(saamge_amd_last_error());
    return h;
}
// ml_free_data (inc/ml.hpp:196)
inline void ml_free_data(ml_data_t *h) { saamge_amd_ml_free_data(h); }
// adapt_update_operators (inc/adapt.hpp, src/adapt.cpp:188-219): new matrix values, same pattern
inline void adapt_update_operators(ml_data_t *h, const double *new_values) {
    if (saamge_amd_update_operators(h, new_values)) throw std::runtime_error(saamge_amd_last_error());
}

// VCycleSolver (inc/solve.hpp:129-143, src/solve.cpp:309-323): Mult zeroes x unless iterative_mode.
class VCycleSolver {
    ml_data_t *h_;
    bool iterative_mode_;
public:
    explicit VCycleSolver(ml_data_t *h, bool iterative_mode = false) : h_(h), iterative_mode_(iterative_mode) {}
    void Mult(const double *b, double *x) const {
        if (saamge_amd_vcycle(h_, b, x, iterative_mode_ ? 1 : 0)) throw std::runtime_error(saamge_amd_last_error());
    }
};

// smpr_ft-shaped call (inc/smpr.hpp:59-60): x += M^-1 (b - A x) on `level`
inline void smpr_sym_poly(ml_data_t *h, int level, const double *b, double *x) {
    if (saamge_amd_smoother(h, level, b, x)) throw std::runtime_error(saamge_amd_last_error());
}

// kalchev_pcg (inc/mfem_addons.hpp:276, src/mfem_addons.cpp:106-248) with B = the hierarchy's V-cycle:
// iterates from the caller's x; stops when (B r, r) < max(RTOLERANCE (B r0, r0), ATOLERANCE);
// returns the iteration count, its negative when the loop did not converge, -1 when the start vector
// already satisfies the criterion (:150-162).  zero_rhs (the reference's A-norm stopping rule for b = 0,
// :142-148, :205) is not implemented: refused.
inline int kalchev_pcg(ml_data_t *h, const double *b, double *x, int print_iter = 0, int max_num_iter = 1000,
                       double RTOLERANCE = 10e-12, double ATOLERANCE = 10e-24, bool zero_rhs = false) {
    if (zero_rhs) throw std::invalid_argument("kalchev_pcg: zero_rhs (A-norm stopping rule) is not supported");
    (void)print_iter;
    int iters = 0, conv = 0;
    if (saamge_amd_pcg(h, b, x, RTOLERANCE, ATOLERANCE, max_num_iter, /*squared_tol=*/0, /*zero_guess=*/0, &iters, &conv,
                       nullptr))
        throw std::runtime_error(saamge_amd_last_error());
    if (conv && iters == 0) return -1;
    return conv ? iters : -iters;
}

// == lowest eigenpairs of A x = lambda M x (saamge_amd_lobpcg): LOBPCG with soft locking, B = the hierarchy's V-cycle ==
// Options with the library's defaults; a mass matrix as three arrays (host or device, 64-bit offsets; all null: identity).
struct LobpcgOptions : saamge_amd_lobpcg_options {
    LobpcgOptions() { saamge_amd_lobpcg_options_default(this); }
};
struct MassMatrix {
    const long long *rowptr = nullptr;
    const int *col = nullptr;
    const double *val = nullptr;
};
struct LobpcgResult {
    std::vector<double> evals, res;     // nev each; res: ||A x - lambda M x|| / (lambda ||M x||)
    std::vector<double> hist;           // (iters + 1) x nev, row-major
    int iters = 0;
    bool converged = false;             // false: max_iter reached or a breakdown; evals / evecs are the best pairs so far
};
// evecs: n x nev column-major, host or device; x0: n x nb column-major (host or device) or nullptr for the hashed start
inline LobpcgResult lobpcg(ml_data_t *h, const LobpcgOptions &o, double *evecs, const MassMatrix &M = MassMatrix(),
                           const double *x0 = nullptr) {
    LobpcgResult r;
    const size_t nev = o.nev > 0 ? (size_t)o.nev : 0, rows = o.max_iter >= 0 ? (size_t)o.max_iter + 1 : 0;
    r.evals.assign(nev, 0.0);
    r.res.assign(nev, 0.0);
    r.hist.assign(rows * nev, 0.0);
    int conv = 0;
    if (saamge_amd_lobpcg(h, M.rowptr, M.col, M.val, &o, x0, r.evals.data(), evecs, r.res.data(), &r.iters, &conv, r.hist.data()))
        throw std::runtime_error(saamge_amd_last_error());
    r.converged = conv != 0;
    r.hist.resize((size_t)(r.iters + 1) * nev);
    return r;
}

// == block solves: k columns per call (saamge_amd_*_block) ==
// Blocks are column-major with a leading dimension, host or device.  Column j of every result, its iteration count, flag
// and history are bit for bit what the single-vector call returns for column j alone.
inline void spmv_block(int nrows, int ncols, const int *rowptr, const int *col, const double *val, int k, const double *X,
                       long long ldx, double *Y, long long ldy) {
    if (saamge_amd_spmv_block(nrows, ncols, rowptr, col, val, k, X, ldx, Y, ldy)) throw std::runtime_error(saamge_amd_last_error());
}
inline void smoother_block(ml_data_t *h, int level, int k, const double *B, long long ldb, double *X, long long ldx) {
    if (saamge_amd_smoother_block(h, level, k, B, ldb, X, ldx)) throw std::runtime_error(saamge_amd_last_error());
}
inline void vcycle_block(ml_data_t *h, int k, const double *B, long long ldb, double *X, long long ldx, bool iterative_mode = false) {
    if (saamge_amd_vcycle_block(h, k, B, ldb, X, ldx, iterative_mode ? 1 : 0)) throw std::runtime_error(saamge_amd_last_error());
}
struct PcgBlockResult {
    std::vector<int> iters, converged;      // k each
    std::vector<double> hist;               // k x (max_iter + 1), column j first; NaN past column j's own last step
};
inline PcgBlockResult pcg_block(ml_data_t *h, int k, const double *B, long long ldb, double *X, long long ldx, double rel_tol,
                                double abs_tol, int max_iter, bool squared_tol = true, bool zero_guess = true) {
    PcgBlockResult r;
    const size_t kk = k > 0 ? (size_t)k : 0;
    r.iters.assign(kk, 0);
    r.converged.assign(kk, 0);
    r.hist.assign(kk * ((size_t)(max_iter > 0 ? max_iter : 0) + 1), std::numeric_limits<double>::quiet_NaN());
    if (saamge_amd_pcg_block(h, k, B, ldb, X, ldx, rel_tol, abs_tol, max_iter, squared_tol ? 1 : 0, zero_guess ? 1 : 0, r.iters.data(),
                             r.converged.data(), r.hist.data()))
        throw std::runtime_error(saamge_amd_last_error());
    return r;
}

// == agglomerate partitions built on the device (saamge_amd_partition_graph / saamge_amd_partition_mesh) ==
// One level on a symmetric CSR graph (host or device arrays): part is resized to n; returns the number of parts produced
// (elems_per_agg is a target).  o == nullptr: the library's defaults.  The options struct is handed on whole (o->seeding = 1:
// spaced seeds).  partition_graph_v2 takes saamge_amd_partition_options_v2, which carries `growth` as well (1: balanced
// growth); it has a name of its own so that a null pointer for the options means the same in every call written before it.
inline int partition_graph(int n, const long long *xadj, const int *adj, int elems_per_agg, std::vector<int> &part,
                           const saamge_amd_partition_options *o = nullptr, void *stream = nullptr) {
    part.assign((size_t)(n > 0 ? n : 0), 0);
    int nparts = 0;
    if (saamge_amd_partition_graph(n, xadj, adj, elems_per_agg, o, stream, part.data(), &nparts))
        throw std::runtime_error(saamge_amd_last_error());
    return nparts;
}
inline int partition_graph_v2(int n, const long long *xadj, const int *adj, int elems_per_agg, std::vector<int> &part,
                              const saamge_amd_partition_options_v2 *o = nullptr, void *stream = nullptr) {
    part.assign((size_t)(n > 0 ? n : 0), 0);
    int nparts = 0;
    if (saamge_amd_partition_graph_v2(n, xadj, adj, elems_per_agg, o, stream, part.data(), &nparts))
        throw std::runtime_error(saamge_amd_last_error());
    return nparts;
}
// All levels from a mesh, as host vectors: partitions[k] / nparts[k] for ProblemArrays::partitions and
// MultilevelParameters' nparts_arr.  elem_ptr == nullptr: every element has nde dofs.  partition_mesh_v2: with `growth`.
struct MeshPartitions {
    std::vector<std::vector<int> > partitions;
    std::vector<int> nparts;
    std::vector<const int *> pointers() const {
        std::vector<const int *> p;
        for (size_t k = 0; k < partitions.size(); ++k) p.push_back(partitions[k].data());
        return p;
    }
};
namespace detail {
// owner of a handle of the C interface: the library's free function runs when the owner dies, and the handle moves with it
template <class H>
using Handle = std::unique_ptr<H, void (*)(H *)>;
// copies the levels of P to the host and frees P
inline MeshPartitions take_partitions(saamge_amd_partitioning *P, int levels) {
    MeshPartitions out;
    for (int k = 0; k < levels; ++k) {
        int n_elem = 0, np = 0;
        int rc = saamge_amd_partitioning_get(P, k, nullptr, &n_elem, &np);
        out.partitions.push_back(std::vector<int>((size_t)n_elem));
        if (!rc) rc = saamge_amd_partitioning_get(P, k, out.partitions.back().data(), nullptr, nullptr);
        if (rc) {
            saamge_amd_partitioning_free(P);
            throw std::runtime_error(saamge_amd_last_error());
        }
        out.nparts.push_back(np);
    }
    saamge_amd_partitioning_free(P);
    return out;
}
}  // namespace detail
inline MeshPartitions partition_mesh(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND,
                                     const std::vector<int> &elems_per_agg, const saamge_amd_partition_options *o = nullptr,
                                     void *stream = nullptr) {
    saamge_amd_partitioning *P = nullptr;
    if (saamge_amd_partition_mesh(NE, nde, elem_ptr, elem_to_dof, ND, (int)elems_per_agg.size(), elems_per_agg.data(), o, stream, &P))
        throw std::runtime_error(saamge_amd_last_error());
    return detail::take_partitions(P, (int)elems_per_agg.size());
}
inline MeshPartitions partition_mesh_v2(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND,
                                        const std::vector<int> &elems_per_agg, const saamge_amd_partition_options_v2 *o = nullptr,
                                        void *stream = nullptr) {
    saamge_amd_partitioning *P = nullptr;
    if (saamge_amd_partition_mesh_v2(NE, nde, elem_ptr, elem_to_dof, ND, (int)elems_per_agg.size(), elems_per_agg.data(), o, stream, &P))
        throw std::runtime_error(saamge_amd_last_error());
    return detail::take_partitions(P, (int)elems_per_agg.size());
}
// The boundary refinement pass (saamge_amd_partition_refine) on any partition of a symmetric CSR graph: part (n labels in
// [0, nparts), host) is refined in place; max_size 0: no cap.  Returns info = {rounds that moved nodes, nodes moved, cut edges
// removed, 1 if no node could move any more}.
struct RefineInfo {
    long long rounds, moved, gain, converged;
};
inline RefineInfo partition_refine(int n, const long long *xadj, const int *adj, int nparts, std::vector<int> &part, int rounds,
                                   int max_size = 0, int min_size = 0, unsigned seed = 0, bool renumber = false,
                                   void *stream = nullptr) {
    if (part.size() != (size_t)(n > 0 ? n : 0)) throw std::invalid_argument("partition_refine: part must hold n labels");
    long long info[4] = {0, 0, 0, 0};
    if (saamge_amd_partition_refine(n, xadj, adj, nparts, part.data(), rounds, max_size, min_size, seed, renumber ? 1 : 0, stream, info))
        throw std::runtime_error(saamge_amd_last_error());
    const RefineInfo r = {info[0], info[1], info[2], info[3]};
    return r;
}
// partition_mesh_v2 with refine_rounds[k] rounds of the pass after the partition of coarsening k (empty: none)
inline MeshPartitions partition_mesh_refined(int NE, int nde, const int *elem_ptr, const int *elem_to_dof, int ND,
                                             const std::vector<int> &elems_per_agg, const std::vector<int> &refine_rounds,
                                             const saamge_amd_partition_options_v2 *o = nullptr, void *stream = nullptr) {
    if (!refine_rounds.empty() && refine_rounds.size() != elems_per_agg.size())
        throw std::invalid_argument("partition_mesh_refined: one refine_rounds entry per coarsening");
    saamge_amd_partitioning *P = nullptr;
    if (saamge_amd_partition_mesh_refined(NE, nde, elem_ptr, elem_to_dof, ND, (int)elems_per_agg.size(), elems_per_agg.data(), o,
                                          refine_rounds.empty() ? nullptr : refine_rounds.data(), stream, &P))
        throw std::runtime_error(saamge_amd_last_error());
    return detail::take_partitions(P, (int)elems_per_agg.size());
}

// == the local order of the agglomerate matrices (saamge_amd_options.ae_order) ==
// saamge_amd_ae_order on host arrays: the agglomerates' dof lists (ae_ptr / ae_to_dof, as the setup builds them), the position of
// every entry in its agglomerate's matrix, and per agglomerate the structural half bandwidth of the rank / box order (bw0), of
// the order in use (bw) and whether that is the level order (choice).  elem_ptr == nullptr: every element has nde dofs.
struct AeOrder {
    std::vector<int> ae_ptr, ae_to_dof, pos, bw0, bw, choice;
};
inline AeOrder ae_order(int ND, int NE, int nde, const int *elem_ptr, const int *elem_to_dof, const int *elem_to_ae, int nparts,
                        int mode) {
    AeOrder r;
    r.ae_ptr.assign((size_t)(nparts > 0 ? nparts : 0) + 1, 0);
    long long nconn = 0;
    if (saamge_amd_ae_order(ND, NE, nde, elem_ptr, elem_to_dof, elem_to_ae, nparts, mode, r.ae_ptr.data(), &nconn, nullptr, nullptr,
                            nullptr, nullptr, nullptr))
        throw std::runtime_error(saamge_amd_last_error());
    r.ae_to_dof.assign((size_t)nconn, 0);
    r.pos.assign((size_t)nconn, 0);
    r.bw0.assign((size_t)nparts, 0);
    r.bw.assign((size_t)nparts, 0);
    r.choice.assign((size_t)nparts, 0);
    if (saamge_amd_ae_order(ND, NE, nde, elem_ptr, elem_to_dof, elem_to_ae, nparts, mode, r.ae_ptr.data(), &nconn,
                            r.ae_to_dof.data(), r.pos.data(), r.bw0.data(), r.bw.data(), r.choice.data()))
        throw std::runtime_error(saamge_amd_last_error());
    return r;
}
// saamge_amd_level_order_info of a level: what the setup's ordering pass found
struct LevelOrderInfo {
    long long permuted, level_orders, max_bw0, max_bw;
};
inline LevelOrderInfo level_order_info(const ml_data_t *h, int level) {
    long long info[4] = {0, 0, 0, 0};
    if (saamge_amd_level_order_info(h, level, info)) throw std::runtime_error(saamge_amd_last_error());
    const LevelOrderInfo r = {info[0], info[1], info[2], info[3]};
    return r;
}

// == element matrices computed on the device (saamge_amd_element_matrices) ==
// From vertex coordinates (NV x dim), element -> vertex lists (elem_ptr == nullptr: nde vertices per element) and per-element
// coefficients (NE x ncoef); kind 0 diffusion, 1 elasticity.  nde 9 in 2D / 27 in 3D: the order-2 quadrilateral / hexahedron;
// nde 6 in 2D / 10 in 3D: the order-2 triangle / tetrahedron (vertices, then edge midpoints)
// (coords then holds all nodes; node orders in saamge_amd.h).  The matrices are packed in element order as the setup entry
// points and AssembledOperator take them.  Throws with saamge_amd_last_error on a refusal.
struct ElementMatricesInfo {
    long long triangles, quadrilaterals, tetrahedra, wedges, hexahedra, doubles, first_bad_element;
    long long order2;      // the order-2 elements (9-node quadrilaterals, 27-node hexahedra, 6-node triangles, 10-node
                           // tetrahedra); the five counts above are order 1
};
// Into the caller's arrays, each a host or a device pointer (elmat_out == nullptr: the sizes only; the dof lists may be nullptr).
inline ElementMatricesInfo element_matrices_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                 const int *elem_to_vertex, int kind, int ncoef, const double *coef,
                                                 double *elmat_out, int *dof_ptr_out = nullptr, int *elem_to_dof_out = nullptr,
                                                 void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_matrices(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, kind, ncoef, coef, stream, elmat_out,
                                    dof_ptr_out, elem_to_dof_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// From HOST arrays, as host vectors, with the dof lists the matrices are indexed by (kind 0: the vertex lists; kind 1:
// dim * vertex + component).
struct ElementMatrices {
    std::vector<double> elmat;
    std::vector<int> dof_ptr, elem_to_dof;
    ElementMatricesInfo info;
};
inline ElementMatrices element_matrices(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                        const int *elem_to_vertex, int kind, int ncoef, const double *coef, void *stream = nullptr) {
    ElementMatrices r;
    const size_t comp = kind == 1 && dim > 0 ? (size_t)dim : 1, ne = (size_t)(NE > 0 ? NE : 0);
    size_t doubles = 0, nconn = 0;
    for (size_t e = 0; e < ne && (elem_ptr || nde > 0); ++e) {      // (sizes of well-formed input; the call checks it)
        const size_t nd = elem_ptr ? (size_t)(elem_ptr[e + 1] > elem_ptr[e] ? elem_ptr[e + 1] - elem_ptr[e] : 0) : (size_t)nde;
        doubles += nd * comp * nd * comp;
        nconn += nd;
    }
    r.elmat.assign(doubles + 1, 0.0);      // (+ 1: data() of an empty vector may be null, which asks for the sizes only)
    r.dof_ptr.assign(ne + 1, 0);
    r.elem_to_dof.assign(nconn * comp + 1, 0);
    r.info = element_matrices_into(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, kind, ncoef, coef, r.elmat.data(),
                                   r.dof_ptr.data(), r.elem_to_dof.data(), stream);
    r.elmat.resize(doubles);
    r.elem_to_dof.resize(nconn * comp);
    return r;
}

// == mass matrices and load vectors computed on the device (saamge_amd_element_mass, saamge_amd_element_loads) ==
// Into the caller's arrays, each a host or a device pointer.  vdim 1 or dim; coef NE doubles.  accumulate: added to the
// matrices elmat_inout holds (K + sigma M); elmat_inout == nullptr without accumulate: the sizes only.
inline ElementMatricesInfo element_mass_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                             const int *elem_to_vertex, int vdim, const double *coef, double *elmat_inout,
                                             bool accumulate = false, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_mass(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, stream, accumulate ? 1 : 0,
                                elmat_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// src: the source at the nodes (NV x vdim); coef == nullptr: 1.  elvec_out: element e's vdim * nodes doubles, packed.
inline ElementMatricesInfo element_loads_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                              const int *elem_to_vertex, int vdim, const double *coef, const double *src,
                                              double *elvec_out, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_loads(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, src, stream, elvec_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}

// == data at the points of the mass rule (saamge_amd_element_points, _eval, _loads_points, _errors) ==
// Point q of element e has the global index qp_ptr[e] + q; NQ = qp_ptr[NE] comes back in `doubles`.  Into the caller's arrays,
// each a host or a device pointer; the outputs of points and eval may each be nullptr.  Layouts and operations in saamge_amd.h.
inline ElementMatricesInfo element_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                               const int *elem_to_vertex, long long *qp_ptr_out, double *xq_out, double *wdet_out,
                                               void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, stream, qp_ptr_out, xq_out, wdet_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// u: NV x vdim at the nodes; uq_out NQ x vdim, gradq_out NQ x vdim x dim
inline ElementMatricesInfo element_eval_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                             const int *elem_to_vertex, int vdim, const double *u, double *uq_out,
                                             double *gradq_out, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_eval(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, u, stream, uq_out, gradq_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// fq: the source at the points (NQ x vdim); coef == nullptr: 1.  elvec_out: the layout of element_loads_into.
inline ElementMatricesInfo element_loads_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                     const int *elem_to_vertex, int vdim, const double *coef, const double *fq,
                                                     double *elvec_out, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_loads_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coef, fq, stream, elvec_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// err_out NE x 2: the squared L2 error against exq and the squared error of the gradient against exgradq, per element; exact data
// nullptr: 0.0 in that column.  The caller sums and takes the root.
inline ElementMatricesInfo element_errors_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                               const int *elem_to_vertex, int vdim, const double *u, const double *exq,
                                               const double *exgradq, double *err_out, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_errors(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, u, exq, exgradq, stream, err_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}

// == coefficients at the points (saamge_amd_element_matrices_points, saamge_amd_element_mass_points) ==
// element_matrices_into / element_mass_into with a coefficient row per POINT of the mass rule in the place of one per element:
// coefq NQ x ncoef (stiffness) or NQ (mass), row qp_ptr[e] + q for point q of element e, the indexing of element_points_into /
// element_eval_into.  Both forms integrate with the mass rule here (saamge_amd.h).  Everything else as the calls they parallel.
inline ElementMatricesInfo element_matrices_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                        const int *elem_to_vertex, int kind, int ncoef, const double *coefq,
                                                        double *elmat_out, int *dof_ptr_out = nullptr,
                                                        int *elem_to_dof_out = nullptr, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_matrices_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, kind, ncoef, coefq, stream, elmat_out,
                                           dof_ptr_out, elem_to_dof_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
inline ElementMatricesInfo element_mass_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                    const int *elem_to_vertex, int vdim, const double *coefq, double *elmat_inout,
                                                    bool accumulate = false, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_element_mass_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, vdim, coefq, stream, accumulate ? 1 : 0,
                                       elmat_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const ElementMatricesInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}

// == boundary forms computed on the device (saamge_amd_boundary_mass, saamge_amd_boundary_loads) ==
// The face mass / face loads of the NF listed faces (element face_elem[f], local face face_local[f]; local faces in
// saamge_amd.h) added into the caller's packed matrices / vectors, each array a host or a device pointer; nullptr for
// elmat_inout / elvec_inout: the checks and the counts only.  segments3 counts the 3-node segments of 9-node quadrilaterals and of
// 6-node triangles, triangles the triangular faces of 3 nodes (tetrahedron, wedge) and of 6 nodes (10-node tetrahedron).
struct BoundaryFormsInfo {
    long long segments2, segments3, triangles, quadrilaterals4, quadrilaterals9, additions, first_bad_face, elements;
};
inline BoundaryFormsInfo boundary_mass_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                            const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                            int vdim, const double *coef, double *elmat_inout, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_mass(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coef, stream,
                                 elmat_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// g: the data at the nodes (NV x vdim); coef == nullptr: 1.
inline BoundaryFormsInfo boundary_loads_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                             const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                             int vdim, const double *coef, const double *g, double *elvec_inout,
                                             void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_loads(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coef, g,
                                  stream, elvec_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}

// == boundary data at the face points (saamge_amd_boundary_points, _eval, _mass_points, _loads_points) ==
// Point q of face f of the list has the global index fp_ptr[f] + q; NFQ = fp_ptr[NF] comes back in `additions` from points and
// eval.  Into the caller's arrays, each a host or a device pointer; the outputs of points and eval may each be nullptr.  Layouts
// and operations in saamge_amd.h.
inline BoundaryFormsInfo boundary_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                              const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                              long long *fp_ptr_out, double *xq_out, double *wmeas_out, double *normal_out,
                                              void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, stream, fp_ptr_out,
                                   xq_out, wmeas_out, normal_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// u: NV x vdim at the nodes; uq_out NFQ x vdim the trace, gradq_out NFQ x vdim x dim the whole gradient
inline BoundaryFormsInfo boundary_eval_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                            const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                            int vdim, const double *u, double *uq_out, double *gradq_out, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_eval(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, u, stream, uq_out,
                                 gradq_out, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// coefq: the coefficient at the face points (NFQ)
inline BoundaryFormsInfo boundary_mass_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                   const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                                   int vdim, const double *coefq, double *elmat_inout, void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_mass_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coefq,
                                        stream, elmat_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}
// gq: the data at the face points (NFQ x vdim); coef == nullptr: 1.
inline BoundaryFormsInfo boundary_loads_points_into(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr,
                                                    const int *elem_to_vertex, int NF, const int *face_elem, const int *face_local,
                                                    int vdim, const double *coef, const double *gq, double *elvec_inout,
                                                    void *stream = nullptr) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (saamge_amd_boundary_loads_points(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, coef, gq,
                                         stream, elvec_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const BoundaryFormsInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
    return r;
}

// == the operator assembled on the device (saamge_amd_operator_assemble) ==
// Owner of the handle.  rowptr() / col() / val() are device arrays that live as long as this object: hand them to
// saamge_amd_ml_produce_data64 / _mixed64 as A.  elem_ptr == nullptr: every element has nde dofs.
class AssembledOperator {
public:
    AssembledOperator(int n, int NE, int nde, const int *elem_ptr, const int *elem_to_dof, const double *elmat,
                      const signed char *bdr_dofs, void *stream = nullptr)
        : op_(nullptr, saamge_amd_operator_free), n_(n), nnz_(0), rowptr_(nullptr), col_(nullptr), val_(nullptr) {
        saamge_amd_operator *op = nullptr;
        if (saamge_amd_operator_assemble(n, NE, nde, elem_ptr, elem_to_dof, elmat, bdr_dofs, stream, &op))
            throw std::runtime_error(saamge_amd_last_error());
        op_.reset(op);
        if (saamge_amd_operator_arrays(op, &rowptr_, &col_, &val_, &nnz_)) throw std::runtime_error(saamge_amd_last_error());
    }
    AssembledOperator(AssembledOperator &&) = default;
    AssembledOperator &operator=(AssembledOperator &&) = default;
    int rows() const { return n_; }
    long long nnz() const { return nnz_; }
    const long long *rowptr() const { return rowptr_; }
    const int *col() const { return col_; }
    const double *val() const { return val_; }
    saamge_amd_operator *handle() const { return op_.get(); }
    // host copies
    void get(std::vector<long long> &rowptr, std::vector<int> &col, std::vector<double> &val) const {
        rowptr.assign((size_t)n_ + 1, 0);
        col.assign((size_t)nnz_, 0);
        val.assign((size_t)nnz_, 0.0);
        if (saamge_amd_operator_get(op_.get(), rowptr.data(), col.data(), val.data(), nullptr)) throw std::runtime_error(saamge_amd_last_error());
    }
    // new element matrices, same mesh: val() rewritten in place (then adapt_update_operators(h, nullptr))
    void update(const double *elmat) {
        if (saamge_amd_operator_update(op_.get(), elmat)) throw std::runtime_error(saamge_amd_last_error());
    }
    void eliminate_rhs(const double *elmat, const double *x_ess, double *b) const {
        if (saamge_amd_operator_eliminate_rhs(op_.get(), elmat, x_ess, b)) throw std::runtime_error(saamge_amd_last_error());
    }
    // b (n, overwritten) from the packed element vectors of element_loads_into on the operator's mesh
    void assemble_rhs(const double *elvec, double *b) const {
        if (saamge_amd_operator_assemble_rhs(op_.get(), elvec, b)) throw std::runtime_error(saamge_amd_last_error());
    }

private:
    detail::Handle<saamge_amd_operator> op_;
    int n_;
    long long nnz_;
    const long long *rowptr_;
    const int *col_;
    const double *val_;
};

// == the faces of a mesh found on the device (saamge_amd_face_table_build, _face_nodes, _face_dofs) ==
// Owner of the handle: which element lies across each local face, the boundary faces and the element graph through faces
// (definitions in saamge_amd.h).  The pointers are device arrays that live as long as this object: bdr_elem() / bdr_local() go
// to boundary_mass_into / boundary_loads_into / face_dofs_into, xadj() / adj() to saamge_amd_partition_graph.  Movable, not
// copyable.  elem_ptr == nullptr: every element has nde nodes.
struct FaceTableInfo {
    long long slots, pairs, boundary_faces, graph_entries, mixed_pairs, max_valence, first_bad_element, isolated_elements;
};
class FaceTable {
public:
    FaceTable(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, void *stream = nullptr)
        : t_(nullptr, saamge_amd_face_table_free), NE_(NE), NB_(0), nnz_(0), info_(), slot_ptr_(nullptr), xadj_(nullptr),
          nbr_elem_(nullptr), nbr_local_(nullptr), bdr_elem_(nullptr), bdr_local_(nullptr), adj_(nullptr) {
        long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        saamge_amd_face_table *t = nullptr;
        if (saamge_amd_face_table_build(NV, dim, NE, nde, elem_ptr, elem_to_vertex, stream, &t, info))
            throw std::runtime_error(saamge_amd_last_error());
        t_.reset(t);
        const FaceTableInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
        info_ = r;
        if (saamge_amd_face_table_arrays(t, &slot_ptr_, &nbr_elem_, &nbr_local_, &NB_, &bdr_elem_, &bdr_local_, &xadj_, &adj_, &nnz_))
            throw std::runtime_error(saamge_amd_last_error());
    }
    FaceTable(FaceTable &&) = default;
    FaceTable &operator=(FaceTable &&) = default;
    int elements() const { return NE_; }
    long long slots() const { return info_.slots; }
    long long boundary_faces() const { return NB_; }
    long long nnz() const { return nnz_; }
    const FaceTableInfo &info() const { return info_; }
    const long long *slot_ptr() const { return slot_ptr_; }
    const int *nbr_elem() const { return nbr_elem_; }
    const int *nbr_local() const { return nbr_local_; }
    const int *bdr_elem() const { return bdr_elem_; }
    const int *bdr_local() const { return bdr_local_; }
    const long long *xadj() const { return xadj_; }
    const int *adj() const { return adj_; }
    saamge_amd_face_table *handle() const { return t_.get(); }
    // host copies
    void get(std::vector<long long> &slot_ptr, std::vector<int> &nbr_elem, std::vector<int> &nbr_local, std::vector<int> &bdr_elem,
             std::vector<int> &bdr_local, std::vector<long long> &xadj, std::vector<int> &adj) const {
        slot_ptr.assign((size_t)NE_ + 1, 0);
        xadj.assign((size_t)NE_ + 1, 0);
        nbr_elem.assign((size_t)info_.slots, 0);
        nbr_local.assign((size_t)info_.slots, 0);
        bdr_elem.assign((size_t)NB_, 0);
        bdr_local.assign((size_t)NB_, 0);
        adj.assign((size_t)nnz_, 0);
        if (saamge_amd_face_table_get(t_.get(), slot_ptr.data(), nbr_elem.data(), nbr_local.data(), nullptr, bdr_elem.data(),
                                      bdr_local.data(), xadj.data(), adj.data(), nullptr))
            throw std::runtime_error(saamge_amd_last_error());
    }

private:
    detail::Handle<saamge_amd_face_table> t_;
    int NE_;
    long long NB_, nnz_;
    FaceTableInfo info_;
    const long long *slot_ptr_, *xadj_;
    const int *nbr_elem_, *nbr_local_, *bdr_elem_, *bdr_local_, *adj_;
};
// An order-1 mesh lifted to order 2 on the same elements, owned by the library (saamge_amd_mesh_lift_order2; definitions in
// saamge_amd.h).  The pointers are device arrays that live as long as this object: coords2() (nullptr without coords),
// elem_ptr2() and elem_to_node() go to element_matrices_into and its kin and to FaceTable.  faces: the FaceTable of the same
// order-1 mesh, used where the mesh has a hexahedron; nullptr: built inside.  Movable, not copyable.
struct MeshLiftInfo {
    long long nodes, edges, face_nodes, centre_nodes, entries, max_owned_edges, first_bad_element, unlisted_vertices;
};
class MeshLift {
public:
    MeshLift(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex,
             const FaceTable *faces = nullptr, void *stream = nullptr)
        : m_(nullptr, saamge_amd_mesh_lift_free), NV_(NV), NE_(NE), dim_(dim), NV2_(0), info_(), coords2_(nullptr),
          elem_ptr2_(nullptr), elem_to_node_(nullptr), edge_hi_(nullptr), edge_ptr_(nullptr), face_slot_(nullptr) {
        long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        saamge_amd_mesh_lift *m = nullptr;
        if (saamge_amd_mesh_lift_order2(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, faces ? faces->handle() : nullptr, stream,
                                        &m, info))
            throw std::runtime_error(saamge_amd_last_error());
        m_.reset(m);
        const MeshLiftInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
        info_ = r;
        if (saamge_amd_mesh_lift_arrays(m, &NV2_, &coords2_, &elem_ptr2_, &elem_to_node_, &edge_ptr_, &edge_hi_, &face_slot_))
            throw std::runtime_error(saamge_amd_last_error());
    }
    MeshLift(MeshLift &&) = default;
    MeshLift &operator=(MeshLift &&) = default;
    int elements() const { return NE_; }
    int nodes() const { return NV2_; }
    const MeshLiftInfo &info() const { return info_; }
    const double *coords2() const { return coords2_; }
    const int *elem_ptr2() const { return elem_ptr2_; }
    const int *elem_to_node() const { return elem_to_node_; }
    const long long *edge_ptr() const { return edge_ptr_; }
    const int *edge_hi() const { return edge_hi_; }
    const long long *face_slot() const { return face_slot_; }
    saamge_amd_mesh_lift *handle() const { return m_.get(); }
    // host copies; coords2 stays empty where the lift was made without coordinates
    void get(std::vector<double> &coords2, std::vector<int> &elem_ptr2, std::vector<int> &elem_to_node, std::vector<long long> &edge_ptr,
             std::vector<int> &edge_hi, std::vector<long long> &face_slot) const {
        coords2.assign(coords2_ ? (size_t)NV2_ * (size_t)dim_ : 0, 0.0);
        elem_ptr2.assign((size_t)NE_ + 1, 0);
        elem_to_node.assign((size_t)info_.entries, 0);
        edge_ptr.assign((size_t)NV_ + 1, 0);
        edge_hi.assign((size_t)info_.edges, 0);
        face_slot.assign((size_t)info_.face_nodes, 0);
        if (saamge_amd_mesh_lift_get(m_.get(), nullptr, coords2.data(), elem_ptr2.data(), elem_to_node.data(), edge_ptr.data(), edge_hi.data(),
                                     face_slot.data()))
            throw std::runtime_error(saamge_amd_last_error());
    }

private:
    detail::Handle<saamge_amd_mesh_lift> m_;
    int NV_, NE_, dim_, NV2_;
    MeshLiftInfo info_;
    const double *coords2_;
    const int *elem_ptr2_, *elem_to_node_, *edge_hi_;
    const long long *edge_ptr_, *face_slot_;
};
// An order-1 mesh refined uniformly `levels` times, owned by the library (saamge_amd_mesh_refine; definitions in saamge_amd.h).
// The pointers are device arrays that live as long as this object: coords() (nullptr without coords), elem_ptr() and
// elem_to_vertex() go to element_matrices_into and its kin, to FaceTable and to MeshLift.  Child k of element e is element
// nc * e + k of the next level (nc = 4 in 2D, 8 in 3D): the ancestor s levels up is c >> (2 s) or c >> (3 s).  Movable, not
// copyable.
struct MeshRefineInfo {
    long long vertices, elements, entries, levels, interp_nnz, max_owned_edges, first_bad_element, unlisted_vertices;
};
struct MeshRefineLevelInfo {      // of one level; the last level was not lifted: -1 from `edges` on
    long long vertices, elements, entries, edges, face_nodes, centre_nodes, max_owned_edges, interp_nnz;
};
struct MeshInterp {               // P_level on the host (CSR, columns ascending)
    int nrows, ncols;
    std::vector<int> rowptr, col;
    std::vector<double> val;
};
class MeshRefine {
public:
    MeshRefine(int NV, int dim, const double *coords, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int levels = 1,
               bool want_interp = false, void *stream = nullptr)
        : m_(nullptr, saamge_amd_mesh_refine_free), dim_(dim), NV_(0), NE_(0), info_(), coords_(nullptr), elem_ptr_(nullptr),
          elem_to_vertex_(nullptr) {
        long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        saamge_amd_refined_mesh *m = nullptr;
        if (saamge_amd_mesh_refine(NV, dim, coords, NE, nde, elem_ptr, elem_to_vertex, levels, want_interp ? 1 : 0, stream, &m, info))
            throw std::runtime_error(saamge_amd_last_error());
        m_.reset(m);
        const MeshRefineInfo r = {info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7]};
        info_ = r;
        if (saamge_amd_mesh_refine_arrays(m, &NV_, &NE_, &coords_, &elem_ptr_, &elem_to_vertex_))
            throw std::runtime_error(saamge_amd_last_error());
    }
    MeshRefine(MeshRefine &&) = default;
    MeshRefine &operator=(MeshRefine &&) = default;
    int vertices() const { return NV_; }
    int elements() const { return NE_; }
    int levels() const { return (int)info_.levels; }
    const MeshRefineInfo &info() const { return info_; }
    const double *coords() const { return coords_; }
    const int *elem_ptr() const { return elem_ptr_; }
    const int *elem_to_vertex() const { return elem_to_vertex_; }
    saamge_amd_refined_mesh *handle() const { return m_.get(); }
    MeshRefineLevelInfo level_info(int level) const {
        long long v[8];
        if (saamge_amd_mesh_refine_level_info(m_.get(), level, v)) throw std::runtime_error(saamge_amd_last_error());
        const MeshRefineLevelInfo r = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
        return r;
    }
    // host copies; coords stays empty where the mesh was refined without coordinates
    void get(std::vector<double> &coords, std::vector<int> &elem_ptr, std::vector<int> &elem_to_vertex) const {
        coords.assign(coords_ ? (size_t)NV_ * (size_t)dim_ : 0, 0.0);
        elem_ptr.assign((size_t)NE_ + 1, 0);
        elem_to_vertex.assign((size_t)info_.entries, 0);
        if (saamge_amd_mesh_refine_get(m_.get(), nullptr, nullptr, coords.data(), elem_ptr.data(), elem_to_vertex.data()))
            throw std::runtime_error(saamge_amd_last_error());
    }
    // P_level on the host (the mesh was refined with want_interp)
    MeshInterp interp(int level) const {
        MeshInterp P;
        long long nnz = 0;
        if (saamge_amd_mesh_refine_interp_get(m_.get(), level, &P.nrows, &P.ncols, &nnz, nullptr, nullptr, nullptr))
            throw std::runtime_error(saamge_amd_last_error());
        P.rowptr.assign((size_t)P.nrows + 1, 0);
        P.col.assign((size_t)nnz, 0);
        P.val.assign((size_t)nnz, 0.0);
        if (saamge_amd_mesh_refine_interp_get(m_.get(), level, nullptr, nullptr, nullptr, P.rowptr.data(), P.col.data(), P.val.data()))
            throw std::runtime_error(saamge_amd_last_error());
        return P;
    }

private:
    detail::Handle<saamge_amd_refined_mesh> m_;
    int dim_, NV_, NE_;
    MeshRefineInfo info_;
    const double *coords_;
    const int *elem_ptr_, *elem_to_vertex_;
};
// the global node ids of the listed faces, in each face's own node order, on the host: face f is nodes[face_ptr[f] ..
// face_ptr[f + 1]).  The inputs are host or device pointers, each on its own.
struct FaceNodes {
    std::vector<int> face_ptr, nodes;
};
inline FaceNodes face_nodes(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                            const int *face_elem, const int *face_local, void *stream = nullptr) {
    long long count = 0;
    if (saamge_amd_face_nodes(NV, dim, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, stream, nullptr, nullptr, &count))
        throw std::runtime_error(saamge_amd_last_error());
    FaceNodes r;
    r.face_ptr.assign((size_t)(NF > 0 ? NF : 0) + 1, 0);
    r.nodes.assign((size_t)count, 0);
    if (NF > 0 && saamge_amd_face_nodes(NV, dim, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, stream,
                                        r.face_ptr.data(), r.nodes.data(), &count))
        throw std::runtime_error(saamge_amd_last_error());
    return r;
}
// bdr_dofs_inout[vdim * a + i] |= flag for every node a of the listed faces and every component i of comp_mask, in place (a host
// or a device pointer of vdim * NV bytes)
struct FaceDofsInfo {
    long long faces, nodes, changed, first_bad_face;
};
inline FaceDofsInfo face_dofs_into(int NV, int dim, int NE, int nde, const int *elem_ptr, const int *elem_to_vertex, int NF,
                                   const int *face_elem, const int *face_local, int vdim, unsigned comp_mask,
                                   signed char *bdr_dofs_inout, int flag = SAAMGE_AMD_ON_ESS_DOMAIN_BORDER, void *stream = nullptr) {
    long long info[4] = {0, 0, 0, 0};
    if (saamge_amd_face_dofs(NV, dim, NE, nde, elem_ptr, elem_to_vertex, NF, face_elem, face_local, vdim, comp_mask, flag, stream,
                             bdr_dofs_inout, info))
        throw std::runtime_error(saamge_amd_last_error());
    const FaceDofsInfo r = {info[0], info[1], info[2], info[3]};
    return r;
}

}  // namespace api
}  // namespace saamge_amd

#ifdef SAAMGE_AMD_WITH_MFEM
#include "saamge_amd_mfem.hpp"
#endif
#endif  // SAAMGE_AMD_HPP
