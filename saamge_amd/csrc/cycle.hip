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

// ---- the block solve phase ----------------------------------------------------------------------------
// The functions above once more on a list of at most BLOCK_MAX columns: the same steps in the same order, each step one
// block member of the SpMV family (sparse.h) in place of the single one, so that every column keeps its bits.  They stand
// beside the single-vector functions and do not replace them: those carry the row-partitioned solve (halo_then, the
// reductions over ranks, own-row offsets) through every step, which has no block form, and their launches are left as they
// are.  A list of one column runs the single-vector kernels (every block member does that for k = 1).
static void require_block(Hierarchy &H, int k) {
    SA_REQUIRE(k >= 1, "block solve: k must be positive");
    for (auto &L : H.levels)
        SA_REQUIRE(!L->dist.on, "block solves are not available on a row-partitioned hierarchy");
    BlockWork &W = H.block;
    const size_t w = (size_t)std::min(k, BLOCK_MAX);
    if ((int)w <= W.width) return;
    const size_t nl = H.levels.size();
    W.lv.resize(nl);
    for (size_t l = 0; l < nl; ++l) {
        const size_t n = (size_t)H.levels[l]->A.nrows;
        if (l > 0) { W.lv[l].b.alloc(n * w); W.lv[l].x.alloc(n * w); }
        W.lv[l].r.alloc(n * w);
        W.lv[l].tmp.alloc(n * w);
    }
    const size_t nc = (size_t)H.levels.back()->Ac.nrows, n0 = (size_t)H.levels[0]->A.nrows;
    W.coarse.b.alloc(nc * w);
    W.coarse.x.alloc(nc * w);
    W.coarse.tmp.alloc(nc * w);
    for (DBuf<double> *v : {&W.pcg.r, &W.pcg.z, &W.pcg.d, &W.pcg.q}) v->alloc(n0 * w);
    for (DBuf<double> *v : {&W.cpcg.r, &W.cpcg.z, &W.cpcg.d, &W.cpcg.q}) v->alloc(nc * w);
    W.scal.alloc(2 * 4 * BLOCK_MAX);
    W.partials.alloc(1024 * BLOCK_MAX);
    W.pcg.sc = W.scal.p;
    W.cpcg.sc = W.scal.p + 4 * BLOCK_MAX;
    W.width = (int)w;
}
static Cols work_cols(const DBuf<double> &v, int n, int k) { return Cols(v.p, n, k); }

static void smooth_from_zero_block(Hierarchy &H, const DCsr &A, const Smoother &sm, const Cols &tmp, const Cols &b, const Cols &x) {
    const double *dinv = sm.dinv_neg.p;
    const int deg = (int)sm.roots.size();
    const Cols *cur = ((deg - 1) % 2 == 0) ? &x : &tmp;
    const Cols *oth = (cur == &x) ? &tmp : &x;
    smooth_first_block(H.stream, A.nrows, dinv, b, *cur, 1.0 / sm.roots[0]);
    for (int i = 1; i < deg; ++i) {
        smooth_step_block(H.stream, A, dinv, b, *cur, *oth, 1.0 / sm.roots[i]);
        std::swap(cur, oth);
    }
}
static void smooth_inplace_block(Hierarchy &H, const DCsr &A, const Smoother &sm, const Cols &tmp, const Cols &b, const Cols &x) {
    const double *dinv = sm.dinv_neg.p;
    const int deg = (int)sm.roots.size();
    const Cols *cur = &x, *oth = &tmp;
    for (int i = 0; i < deg; ++i) {
        smooth_step_block(H.stream, A, dinv, b, *cur, *oth, 1.0 / sm.roots[i]);
        std::swap(cur, oth);
    }
    if (cur != &x) vec_copy_block(H.stream, A.nrows, *cur, x);
}

// pcg_loop on the columns of b / x.  All columns still in the loop are at the same step i; a column that meets one of
// pcg_loop's exits leaves the list at exactly that step, with pcg_loop's return value and flag.  The scalars of column j are
// W.sc[4 j ..]; the host reads all of them back in one copy per step.  hist: column j's history at hist[j] (or null).
static void pcg_loop_block(Hierarchy &H, const DCsr &A, const std::function<void(const Cols &, const Cols &)> &prec, const Cols &b,
                           const Cols &x, BlockWork::Pcg &W, double rel_tol, double abs_tol, int max_iter, bool squared,
                           bool zero_guess, int *iters, int *converged, double *const *hist) {
    hipStream_t s = H.stream;
    const int n = A.nrows, k = b.k;
    const Cols R = work_cols(W.r, n, k), Z = work_cols(W.z, n, k), Dd = work_cols(W.d, n, k), Q = work_cols(W.q, n, k);
    const Cols SC(W.sc, 4, k);
    double *partials = H.block.partials.p;
    std::vector<int> act(k);
    for (int j = 0; j < k; ++j) act[j] = j;
    auto pick = [&](const Cols &c) {
        Cols r;
        r.k = (int)act.size();
        for (int j = 0; j < r.k; ++j) r.p[j] = c.p[act[j]];
        return r;
    };
    double sc[4 * BLOCK_MAX], r0[BLOCK_MAX];
    // leave(keep): the columns for which keep(j) is false leave the list
    auto leave = [&](const std::function<bool(int)> &keep) {
        std::vector<int> rest;
        for (int j : act) if (keep(j)) rest.push_back(j);
        act.swap(rest);
    };
    if (zero_guess) {
        vec_zero_block(s, n, x);
        vec_copy_block(s, n, b, R);
    } else {
        spmv_residual_block(s, A, x, b, R);
    }
    prec(R, Z);
    vec_copy_block(s, n, Z, Dd);
    dot_block(s, n, Dd, R, partials, SC, 0);
    read_back(sc, (const double *)W.sc, (size_t)4 * k, s);
    leave([&](int j) {
        const double nom0 = sc[4 * j];
        if (hist) hist[j][0] = nom0;
        r0[j] = squared ? std::max(nom0 * rel_tol * rel_tol, abs_tol * abs_tol) : std::max(nom0 * rel_tol, abs_tol);
        iters[j] = 0;
        if (converged) converged[j] = nom0 <= r0[j] ? 1 : 0;
        return !(nom0 <= r0[j]);
    });
    if (act.empty()) return;
    spmv_block(s, A, pick(Dd), pick(Q));
    dot_block(s, n, pick(Q), pick(Dd), partials, pick(SC), 1);
    read_back(sc, (const double *)W.sc, (size_t)4 * k, s);
    leave([&](int j) { return !(sc[4 * j + 1] == 0.0); });
    int i = 1;
    while (!act.empty()) {
        pcg_update_xr_block(s, n, pick(SC), pick(x), pick(R), pick(Dd), pick(Q));
        prec(pick(R), pick(Z));
        dot_block(s, n, pick(R), pick(Z), partials, pick(SC), 2);
        read_back(sc, (const double *)W.sc, (size_t)4 * k, s);
        leave([&](int j) {
            const double betanom = sc[4 * j + 2];
            if (hist && i <= max_iter) hist[j][i] = betanom;
            if (betanom < r0[j]) {
                if (converged) converged[j] = 1;
                iters[j] = i;
                return false;
            }
            return true;
        });
        if (++i > max_iter) {
            for (int j : act) iters[j] = max_iter;
            break;
        }
        if (act.empty()) break;
        pcg_update_d_block(s, n, pick(SC), pick(Dd), pick(Z));
        spmv_block(s, A, pick(Dd), pick(Q));
        dot_block(s, n, pick(Dd), pick(Q), partials, pick(SC), 1);
        pcg_shift_nom_block(s, pick(SC));
    }
}

// The coarsest solve of a block.  The inner PCG (kind 2) is the block loop; the dense inverse with its refinement step
// (kind 1), the block-tridiagonal solve (kind 3) and a caller's solver run column by column through coarse_solve.
static void coarse_solve_block(Hierarchy &H, const Cols &rc, const Cols &xc) {
    const DCsr &Ac = H.levels.back()->Ac;
    CoarseSolver &C = H.coarse;
    if (Ac.nrows == 0) return;
    if (C.user_solve || C.kind != 2) {
        for (int j = 0; j < rc.k; ++j) coarse_solve(H, rc.p[j], xc.p[j]);
        return;
    }
    const Cols tmp = work_cols(H.block.coarse.tmp, Ac.nrows, rc.k);
    auto prec = [&](const Cols &r, const Cols &z) {
        Cols t = tmp;
        t.k = r.k;
        smooth_from_zero_block(H, Ac, C.sm, t, r, z);
    };
    int its[BLOCK_MAX], conv[BLOCK_MAX];
    pcg_loop_block(H, Ac, prec, rc, xc, H.block.cpcg, H.params.coarse_rtol, 0.0, H.params.coarse_max_iter, false, true, its, conv,
                   nullptr);
    C.last_iters = its[rc.k - 1];
}

static void vcycle_rec_block(Hierarchy &H, int level, const Cols &b, const Cols &x) {
    Level &L = *H.levels[level];
    hipStream_t s = H.stream;
    BlockWork &W = H.block;
    const int k = b.k, n = L.A.nrows;
    const bool last = (level + 1 == (int)H.levels.size());
    const Hierarchy::UserSmoother us = level < (int)H.user_smoothers.size() ? H.user_smoothers[level] : Hierarchy::UserSmoother();
    const Cols tmp = work_cols(W.lv[level].tmp, n, k), res = work_cols(W.lv[level].r, n, k);
    if (us.pre) for (int j = 0; j < k; ++j) user_smooth(H, level, us.pre, us.ctx, b.p[j], x.p[j], true);      // (a plug: per column)
    else smooth_from_zero_block(H, L.A, L.sm, tmp, b, x);
    spmv_residual_block(s, L.A, x, b, res);
    const int nc = L.R.nrows;
    const Cols rc = work_cols(last ? W.coarse.b : W.lv[level + 1].b, nc, k), xc = work_cols(last ? W.coarse.x : W.lv[level + 1].x, nc, k);
    spmv_block(s, L.R, res, rc);
    if (last) coarse_solve_block(H, rc, xc);
    else vcycle_rec_block(H, level + 1, rc, xc);
    spmv_add_block(s, L.P, xc, x);
    if (us.post) for (int j = 0; j < k; ++j) user_smooth(H, level, us.post, us.ctx, b.p[j], x.p[j], false);
    else smooth_inplace_block(H, L.A, L.sm, tmp, b, x);
}

std::vector<double *> block_columns(const double *base, long ld, int k, const int *c) {
    std::vector<double *> p((size_t)k);
    for (int j = 0; j < k; ++j) p[j] = const_cast<double *>(base) + (size_t)(c ? c[j] : j) * (size_t)ld;
    return p;
}
// chunk c of the two pointer lists (block_chunks.h)
static Cols chunk_cols(const BlockChunk &ch, const double *const *p) {
    Cols r;
    r.k = ch.count;
    for (int j = 0; j < ch.count; ++j) r.p[j] = const_cast<double *>(p[ch.first + j]);
    return r;
}
template <class F>
static void for_chunks(int k, const double *const *b, double *const *x, F &&f) {
    for (int c = 0; c < block_num_chunks(k); ++c) {
        const BlockChunk ch = block_chunk(k, c);
        f(ch, chunk_cols(ch, b), chunk_cols(ch, x));
    }
}

void smoother_apply_block(Hierarchy &H, int level, int k, const double *const *b, double *const *x) {
    require_block(H, k);
    Level &L = *H.levels[level];
    for_chunks(k, b, x, [&](const BlockChunk &ch, const Cols &bc, const Cols &xc) {
        smooth_inplace_block(H, L.A, L.sm, work_cols(H.block.lv[level].tmp, L.A.nrows, ch.count), bc, xc);
    });
}
void vcycle_apply_block(Hierarchy &H, int k, const double *const *b, double *const *x) {
    require_block(H, k);
    for_chunks(k, b, x, [&](const BlockChunk &, const Cols &bc, const Cols &xc) { vcycle_rec_block(H, 0, bc, xc); });
}
void vcycle_iterate_block(Hierarchy &H, int k, const double *const *b, double *const *x) {
    require_block(H, k);
    const DCsr &A = H.levels[0]->A;
    for_chunks(k, b, x, [&](const BlockChunk &ch, const Cols &bc, const Cols &xc) {
        const Cols r = work_cols(H.block.pcg.r, A.nrows, ch.count), z = work_cols(H.block.pcg.z, A.nrows, ch.count);
        spmv_residual_block(H.stream, A, xc, bc, r);
        vcycle_rec_block(H, 0, r, z);
        vec_axpy_block(H.stream, A.nrows, 1.0, z, xc);
    });
}
void pcg_solve_block(Hierarchy &H, int k, const double *const *b, double *const *x, double rel_tol, double abs_tol, int max_iter,
                     int squared_tol, int zero_guess, int *iters, int *converged, double *hist) {
    require_block(H, k);
    const size_t stride = (size_t)std::max(max_iter, 0) + 1;
    auto prec = [&](const Cols &r, const Cols &z) { vcycle_rec_block(H, 0, r, z); };
    for_chunks(k, b, x, [&](const BlockChunk &ch, const Cols &bc, const Cols &xc) {
        double *hp[BLOCK_MAX];
        for (int j = 0; j < ch.count; ++j) hp[j] = hist ? hist + (size_t)(ch.first + j) * stride : nullptr;
        pcg_loop_block(H, H.levels[0]->A, prec, bc, xc, H.block.pcg, rel_tol, abs_tol, max_iter, squared_tol != 0, zero_guess != 0,
                       iters + ch.first, converged ? converged + ch.first : nullptr, hist ? hp : nullptr);
    });
}

}  // namespace saamge_amd
