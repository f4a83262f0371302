// Solve phase: polynomial smoother, V-cycle, PCG and the coarsest solver.  Host C++ driving the HIP kernels of the SpMV
// family (sparse.hip); the setup that fills the hierarchy is hierarchy.hip.
#include "cycle.h"
#include "dense.h"
#include "dist.h"
#include "hierarchy.h"

#include <algorithm>
#include <cmath>
#include <functional>

namespace saamge_amd {

std::vector<double> sas_poly_roots(int nu) {
    SA_REQUIRE(nu > 0, "nu_relax must be positive");
    std::vector<double> r;
    const double denom = (double)(2 * nu + 1);
    for (int i = 0; i <= 2 * nu; ++i) {
        const double v = std::cos(((double)i * M_PI) / denom);
        r.push_back(v * v);
    }
    for (int i = 1; i <= nu; ++i) {
        const double v = std::sin(((double)i * M_PI) / denom);
        r.push_back(v * v);
    }
    return r;
}

void operator_data(hipStream_t s, DCsr &A, const Options &opt, bool codes, Smoother &sm) {
    const size_t n = (size_t)A.nrows;
    build_sell(s, A, opt);
    if (sm.dinv_neg.n != n) sm.dinv_neg.alloc(n);
    if (!n) return;
    DBuf<double> tmp(n);
    build_dinv_neg(s, A, tmp.p, sm.dinv_neg.p);
    if (codes) build_dinv_codes(s, A, sm.dinv_neg.p, opt);
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

// coarsest solver: PCG on the coarsest operator, preconditioned by its own polynomial smoother (the reference's parallel
// "coarse direct" is likewise an inner PCG to 1e-16, amg/src/tg.cpp:998-1003)
void setup_coarse_solver(Hierarchy &H) {
    DCsr &Ac = H.levels.back()->Ac;
    CoarseSolver &C = H.coarse;
    hipStream_t s = H.stream;
    const size_t n = (size_t)Ac.nrows;
    C.inv.release();
    operator_data(s, Ac, H.params.opt, false, C.sm);
    C.kind = 2;
    C.w.alloc(n);
    C.w.sc = H.scal.p + 4;
    C.sm.tmp.alloc(n);
    C.sm.roots = sas_poly_roots(H.levels.back()->nu_relax);
    // Dense direct solve (the reference's serial `--coarse-direct`, amg/src/tg.cpp:979-1014) as an explicit
    // inverse when the coarsest operator is small enough (coarse_solver 0 = auto: n <= 8192, i.e. up to 512 MiB;
    // 1 = always): at n = 3317 the inverse costs a few ms once and 20 us per V-cycle, the inner PCG ~2.4 ms per
    // V-cycle.  A non-positive pivot (semi-definite operator) falls back to the inner PCG.
    const int want = H.params.coarse_solver;
    constexpr long dense_max = 8192;
    C.bt = BlockTri();
    if (n && (want == 1 || (want == 0 && (long)n <= dense_max)) && n <= 16384) {
        if (dense_inverse_spd(s, Ac, C.inv)) C.kind = 1;
        else C.inv.release();
    } else if (n && (want == 1 || want == 3)) {
        // a DIRECT solve was asked for (the reference's coarse_direct, src/tg.cpp:990-996) on an operator beyond one dense
        // inverse: block-tridiagonal elimination over a level structure of its graph (blocktri.hip)
        if (blocktri_factor(s, Ac, C.bt)) C.kind = 3;
    }
    C.b.alloc(n);
    C.x.alloc(n);
}

static inline RowRange rows_of(const Level::Dist *D) {
    RowRange rr;
    if (D) { rr.row0 = D->row0; rr.nrows = D->nloc; }
    return rr;
}
static Level::Dist *dist_of(Level &L) { return L.dist.on ? &L.dist : nullptr; }

// x = poly(b) starting from x = 0; result lands in x, sm.tmp is the ping-pong partner.  Row-partitioned (D != null): own rows
// only; the halo of the result is NOT refreshed (the next operator application does that, halo_then).
static void smooth_from_zero(Hierarchy &H, const DCsr &A, const Smoother &sm, const double *b, double *x,
                             Level::Dist *D = nullptr) {
    const double *dinv = sm.dinv_neg.p;
    const int deg = (int)sm.roots.size();
    const int off = D ? D->row0 : 0, nl = D ? D->nloc : A.nrows;
    double *cur = ((deg - 1) % 2 == 0) ? x : sm.tmp.p;
    double *oth = (cur == x) ? sm.tmp.p : x;
    smooth_first(H.stream, nl, dinv + off, b + off, cur + off, 1.0 / sm.roots[0]);
    for (int i = 1; i < deg; ++i) {
        const double scale = 1.0 / sm.roots[i];
        halo_then(H, D, cur, [&](hipStream_t q, RowRange rr) { smooth_step(q, A, dinv, b, cur, oth, scale, rr); });
        std::swap(cur, oth);
    }
}

// x += M^-1 (b - A x).  Row-partitioned: x is valid on the own rows on entry and on return (every step refreshes the halo it reads).
static void smooth_inplace(Hierarchy &H, const DCsr &A, const Smoother &sm, const double *b, double *x,
                           Level::Dist *D = nullptr) {
    const double *dinv = sm.dinv_neg.p;
    const int deg = (int)sm.roots.size();
    const int off = D ? D->row0 : 0, nl = D ? D->nloc : A.nrows;
    double *cur = x, *oth = sm.tmp.p;
    for (int i = 0; i < deg; ++i) {
        const double scale = 1.0 / sm.roots[i];
        halo_then(H, D, cur, [&](hipStream_t q, RowRange rr) { smooth_step(q, A, dinv, b, cur, oth, scale, rr); });
        std::swap(cur, oth);
    }
    if (cur != x) vec_copy(H.stream, nl, cur + off, x + off);
}

// The PCG loop shared by the outer solve and the coarsest solver (MFEM CGSolver::Mult order of operations == kalchev_pcg,
// amg/src/mfem_addons.cpp:106-248).  Row-partitioned (D != null): vector updates and inner products run on the own rows, the
// products are summed over ranks, the search direction's halo is refreshed before each A d.
static int pcg_loop(Hierarchy &H, const DCsr &A, const std::function<void(const double *, double *)> &prec,
                    const double *b, double *x, PcgWork &W, double rel_tol, double abs_tol, int max_iter,
                    bool squared, bool zero_guess, int *converged, double *hist, Level::Dist *D = nullptr) {
    hipStream_t s = H.stream;
    double *r = W.r.p, *z = W.z.p, *d = W.d.p, *q = W.q.p, *sc = W.sc;
    const int off = D ? D->row0 : 0, n = D ? D->nloc : A.nrows;
    auto pdot = [&](const double *u, const double *v, double *out) {
        dot(s, n, u + off, v + off, H.partials.p, out);
        if (D) dist_allreduce(H, out, 1);
    };
    if (zero_guess) {
        vec_zero(s, n, x + off);
        vec_copy(s, n, b + off, r + off);
    } else {
        halo_then(H, D, x, [&](hipStream_t q, RowRange rq) { spmv_residual(q, A, x, b, r, rq); });
    }
    prec(r, z);
    vec_copy(s, n, z + off, d + off);
    pdot(d, r, sc + 0);
    const double nom0 = read_one(sc + 0, s);
    if (hist) hist[0] = nom0;
    const double r0 = squared ? std::max(nom0 * rel_tol * rel_tol, abs_tol * abs_tol)
                              : std::max(nom0 * rel_tol, abs_tol);
    if (converged) *converged = 0;
    if (nom0 <= r0) {
        if (converged) *converged = 1;
        return 0;
    }
    halo_then(H, D, d, [&](hipStream_t st, RowRange rq) { spmv(st, A, d, q, rq); });
    pdot(q, d, sc + 1);
    if (read_one(sc + 1, s) == 0.0) return 0;
    int i = 1;
    int final_iter = max_iter;
    for (;;) {
        pcg_update_xr(s, n, sc, x + off, r + off, d + off, q + off);
        prec(r, z);
        pdot(r, z, sc + 2);
        const double betanom = read_one(sc + 2, s);
        if (hist && i <= max_iter) hist[i] = betanom;      // hist holds max_iter + 1 doubles: with max_iter <= 0 the one update still runs
        if (betanom < r0) {
            if (converged) *converged = 1;
            final_iter = i;
            break;
        }
        if (++i > max_iter) break;
        pcg_update_d(s, n, sc, d + off, z + off);
        halo_then(H, D, d, [&](hipStream_t st, RowRange rq) { spmv(st, A, d, q, rq); });
        pdot(d, q, sc + 1);
        copy_device(sc + 0, (const double *)sc + 2, 1, s);
    }
    return final_iter;
}

static void coarse_solve(Hierarchy &H, const double *rc, double *xc) {
    const DCsr &Ac = H.levels.back()->Ac;
    CoarseSolver &C = H.coarse;
    if (Ac.nrows == 0) return;
    C.last_iters = 0;
    if (C.user_solve) {      // tg_data_t::coarse_solver assigned by the caller (host solver)
        const size_t n = (size_t)Ac.nrows;
        hvec<double> hr = fetch_host(rc, n, H.stream), hx(n, 0.0);
        SA_REQUIRE(C.user_solve(C.user_ctx, (int)n, hr.data(), hx.data()) == 0, "user coarse solver failed");
        upload(xc, (const double *)hx.data(), n, H.stream);
    } else if (C.kind == 1) {
        // x = X b and one step of iterative refinement, x += X (b - Ac x): the elimination's round-off
        // (~cond(Ac) eps) is pushed to the level of the residual evaluation
        const int n = Ac.nrows;
        dense_symv(H.stream, n, C.inv.p, rc, xc, false);
        spmv_residual(H.stream, Ac, xc, rc, C.w.r.p);
        dense_symv(H.stream, n, C.inv.p, C.w.r.p, xc, true);
    } else if (C.kind == 3) {
        blocktri_solve(H.stream, Ac, C.bt, rc, xc);
    } else {
        auto prec = [&](const double *r, double *z) { smooth_from_zero(H, Ac, C.sm, r, z); };
        int conv = 0;
        C.last_iters = pcg_loop(H, Ac, prec, rc, xc, C.w, H.params.coarse_rtol, 0.0, H.params.coarse_max_iter, false, true,
                                &conv, nullptr);
    }
}

// a caller's smoother (saamge_amd_set_smoother; the reference's smpr_ft plug, src/tg.cpp:113,131): x += M^-1 (b - A x)
// on host copies.  zero_start: the cycle's x is not initialised yet, the callback receives x = 0.
static void user_smooth(Hierarchy &H, int level, int (*fn)(void *, int, int, const double *, double *), void *ctx,
                        const double *b, double *x, bool zero_start) {
    Level &L = *H.levels[level];
    SA_REQUIRE(!L.dist.on, "a caller's smoother cannot run on a level that is row-partitioned over several ranks");
    const size_t n = (size_t)L.A.nrows;
    hvec<double> hb = fetch_host(b, n, H.stream), hx = zero_start ? hvec<double>(n, 0.0) : fetch_host((const double *)x, n, H.stream);
    SA_REQUIRE(fn(ctx, level, (int)n, hb.data(), hx.data()) == 0, "the caller's smoother failed");
    upload(x, (const double *)hx.data(), n, H.stream);
}

// One V(1,1)-cycle from x = 0 (tg_cycle_atb, amg/src/tg.cpp:91-132).  On a row-partitioned
// level b is read and x is written on the own rows only.
static void vcycle_rec(Hierarchy &H, int level, const double *b, double *x) {
    Level &L = *H.levels[level];
    hipStream_t s = H.stream;
    Level::Dist *D = dist_of(L);
    const bool last = (level + 1 == (int)H.levels.size());
    const Hierarchy::UserSmoother us = level < (int)H.user_smoothers.size() ? H.user_smoothers[level] : Hierarchy::UserSmoother();
    if (us.pre) user_smooth(H, level, us.pre, us.ctx, b, x, true);
    else smooth_from_zero(H, L.A, L.sm, b, x, D);                       // pre_smoother, x0 = 0
    halo_then(H, D, x, [&](hipStream_t q, RowRange rr) { spmv_residual(q, L.A, x, b, L.r.p, rr); });   // res = b - A x
    double *rc = last ? H.coarse.b.p : H.levels[level + 1]->b.p;
    double *xc = last ? H.coarse.x.p : H.levels[level + 1]->x.p;
    spmv(s, L.R, L.r.p, rc);                                            // resc = R res
    if (D) {      // res is zero outside the own rows: partial sums
        // a row-partitioned coarser level reads the restricted residual on its own rows only: reduce-scatter
        if (!last && H.levels[level + 1]->dist.on) dist_reduce_scatter_rows(H, H.levels[level + 1]->dist, rc);
        else dist_allreduce(H, rc, L.R.nrows);
    }
    if (last) {
        coarse_solve(H, rc, xc);
    } else {
        vcycle_rec(H, level + 1, rc, xc);
        Level &N = *H.levels[level + 1];
        if (N.dist.on) dist_allgather_rows(H, N.dist, xc);
    }
    spmv_add(s, L.P, xc, x, rows_of(D));                                // x += P xc
    if (us.post) user_smooth(H, level, us.post, us.ctx, b, x, false);
    else smooth_inplace(H, L.A, L.sm, b, x, D);                         // post_smoother
}

void smoother_apply(Hierarchy &H, int level, const double *b, double *x) {
    Level &L = *H.levels[level];
    Level::Dist *D = dist_of(L);
    smooth_inplace(H, L.A, L.sm, b, x, D);
    if (D) dist_allgather_rows(H, *D, x);
}

void vcycle_apply(Hierarchy &H, int level, const double *b, double *x) {
    vcycle_rec(H, level, b, x);
    Level &L = *H.levels[level];
    if (L.dist.on) dist_allgather_rows(H, L.dist, x);
}

void vcycle_iterate(Hierarchy &H, const double *b, double *x) {
    const DCsr &A = H.levels[0]->A;
    spmv_residual(H.stream, A, x, b, H.pcg.r.p);
    vcycle_apply(H, 0, H.pcg.r.p, H.pcg.z.p);
    vec_axpy(H.stream, A.nrows, 1.0, H.pcg.z.p, x);
}

int pcg_solve(Hierarchy &H, const double *b, double *x, double rel_tol, double abs_tol,
              int max_iter, int squared_tol, int zero_guess, int *converged, double *hist) {
    Level &L0 = *H.levels[0];
    Level::Dist *D = dist_of(L0);
    auto prec = [&](const double *r, double *z) { vcycle_rec(H, 0, r, z); };
    PhaseTimer tm(H.stream);
    struct Lap { PhaseTimer &t; ~Lap() { t.lap("TOTAL pcg_solve", 0); } } lap{tm};
    const int it = pcg_loop(H, L0.A, prec, b, x, H.pcg, rel_tol, abs_tol, max_iter, squared_tol != 0, zero_guess != 0,
                            converged, hist, D);
    if (D) dist_allgather_rows(H, *D, x);  // every rank returns the full solution
    return it;
}

}  // namespace saamge_amd
