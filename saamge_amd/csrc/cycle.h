// The solve phase (cycle.hip): polynomial smoother, V-cycle, PCG, the coarsest solver, and the state each of them keeps.
// hierarchy.h includes this header for the types; the functions take the Hierarchy they work on.
#pragma once
#include <vector>

#include "blocktri.h"
#include "common.h"
#include "options.h"
#include "sparse.h"

namespace saamge_amd {

struct Hierarchy;

// One polynomial smoother (smpr_poly_data_t): a level's, or the preconditioner of the coarsest solver's inner PCG.
struct Smoother {
    DBuf<double> dinv_neg;      // Dinv_neg of the operator it smooths (operator_data)
    std::vector<double> roots;  // SAS roots, one step each (sas_poly_roots)
    DBuf<double> tmp;           // ping-pong partner of the vector being smoothed
};
// Vectors of one PCG and its three scalars sc[0..2] on the device.  The scalars live in Hierarchy::scal -- the outer solve's in
// slots 0-2, the inner solve's from slot 4, so that an inner solve leaves the outer scalars alone; Hierarchy::partials is shared.
struct PcgWork {
    DBuf<double> r, z, d, q;
    double *sc = nullptr;
    void alloc(size_t n) { r.alloc(n); z.alloc(n); d.alloc(n); q.alloc(n); }
};
struct CoarseSolver {
    int kind = 2;               // 1 explicit dense inverse, 2 inner PCG, 3 block-tridiagonal direct solve (blocktri.hip)
    BlockTri bt;
    DBuf<double> inv;           // explicit inverse of the coarsest operator (kind 1)
    Smoother sm;                // preconditioner of the inner PCG
    PcgWork w;                  // inner PCG; w.r is also the residual of kind 1's refinement step
    DBuf<double> b, x;          // restricted residual and correction on the coarsest operator
    int last_iters = 0;
    // tg_data_t::coarse_solver plug: host callback replacing the built-in coarsest solve
    int (*user_solve)(void *ctx, int n, const double *rc_host, double *xc_host) = nullptr;
    void *user_ctx = nullptr;
};

// Workspace of the block solve phase (Hierarchy::block): `width` columns of every vector the single-vector cycle keeps once.
// Empty until the first block call, grown only when a wider call arrives (at most BLOCK_MAX columns: wider calls run in
// chunks), released with the hierarchy.
struct BlockWork {
    int width = 0;
    struct Vecs { DBuf<double> b, x, r, tmp; };      // b, x: the levels below the finest and the coarsest operator
    std::vector<Vecs> lv;
    Vecs coarse;                                     // coarse.tmp: ping-pong partner of the inner PCG's smoother
    struct Pcg { DBuf<double> r, z, d, q; double *sc = nullptr; };
    Pcg pcg, cpcg;                                   // the outer solve and the coarsest solver's inner PCG
    DBuf<double> scal, partials;                     // 4 scalars per column and PCG; 1024 partials per column
};

// smpr_sas_poly_roots (amg/src/smpr.cpp:282-306)
std::vector<double> sas_poly_roots(int nu);
// What an operator needs before it can be smoothed (smpr_init_poly_data, amg/src/smpr.cpp:359-423): its SELL-64 copy for the SpMV
// family, sm.dinv_neg (allocated here unless it has the operator's size already), with `codes` the byte codes of dinv_neg
// (build_dinv_codes), then a synchronisation of s.  sm.roots and sm.tmp are the caller's.
// codes: set for the spectral levels, clear for the corrected null-space level and the coarsest operator.  Only the staged kernel
// of the coded SELL formats reads the codes, behind Options::sell bit 5 (off by default), and their effect was measured on the fine
// level of the 256^3 problem alone.  On the two coarsest operators: not measured.
void operator_data(hipStream_t s, DCsr &A, const Options &opt, bool codes, Smoother &sm);
// (re)builds Hierarchy::coarse for the coarsest operator levels.back()->Ac; Params::coarse_solver decides the kind
void setup_coarse_solver(Hierarchy &h);

// VCycleSolver::Mult with iterative_mode = false (amg/src/solve.cpp:309-323): x = B b.
void vcycle_apply(Hierarchy &h, int level, const double *b, double *x);
// ... with iterative_mode = true, level 0, not row-partitioned: x <- x + B (b - A x)
void vcycle_iterate(Hierarchy &h, const double *b, double *x);
// smpr_sym_poly (amg/src/smpr.cpp:213-234): x += M^-1 (b - A x)
void smoother_apply(Hierarchy &h, int level, const double *b, double *x);
// MFEM CGSolver / kalchev_pcg (amg/src/mfem_addons.cpp:106-248).  b, x device pointers.
// Returns iterations; hist (host, may be null) receives (B r_k, r_k), k = 0..iters.
int pcg_solve(Hierarchy &h, const double *b, double *x, double rel_tol, double abs_tol,
              int max_iter, int squared_tol, int zero_guess, int *converged, double *hist);

// ---- the same on k >= 1 columns (device pointers, one per column; any k: more than BLOCK_MAX columns run in chunks) ----------
// Column j of every result, its iteration count, flag and history are bit for bit what the call above returns for column j
// alone.  Row-partitioned hierarchies are refused.
void smoother_apply_block(Hierarchy &h, int level, int k, const double *const *b, double *const *x);
void vcycle_apply_block(Hierarchy &h, int k, const double *const *b, double *const *x);
void vcycle_iterate_block(Hierarchy &h, int k, const double *const *b, double *const *x);
// iters, converged (may be null): k ints; hist (host, may be null): column j's history at hist + j (max_iter + 1)
void pcg_solve_block(Hierarchy &h, int k, const double *const *b, double *const *x, double rel_tol, double abs_tol, int max_iter,
                     int squared_tol, int zero_guess, int *iters, int *converged, double *hist);
// the columns c[0 .. k) (null: 0 .. k - 1) of a column-major block as a pointer list
std::vector<double *> block_columns(const double *base, long ld, int k, const int *c = nullptr);

}  // namespace saamge_amd
