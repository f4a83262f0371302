// LOBPCG with soft locking, step for step what saamge_amd/lobpcg_model.py defines.  The basis lives in three buffers of
// 3 nb columns (S, A S, M S; without M the third is S itself): X in columns [0, nb), P_j in column nb + j, W_j in column
// 2 nb + j, so that one in-place combination of the whole buffer writes the new X and P side by side.  Per iteration: two
// Gram products of the whole buffer, one transfer of both to the host (lobpcg_host.h picks the basis columns in the
// model's order X, W, P and returns the coefficients), one combination applied to the three buffers in one launch, the
// residuals (stored where A W goes next), and for the unlocked columns together one block V-cycle, one block A product and one
// block M product (cycle.h, sparse.h: each column with the bits of the single-vector call).
#include "lobpcg.h"

#include <cmath>
#include <limits>

#include "blockvec.h"
#include "cycle.h"
#include "lobpcg_host.h"
#include "sparse.h"

namespace saamge_amd {

namespace lh = lobpcg_host;

void lobpcg_solve(Hierarchy &H, const DCsr *M, const LobpcgOptions &o, const double *x0, double *evals, double *evecs,
                  double *res, int *iters, int *converged, double *hist) {
    Level &L0 = *H.levels[0];
    const DCsr &A = L0.A;
    hipStream_t s = H.stream;
    const int n = A.nrows, nb = o.nb, nev = o.nev, width = 3 * nb;
    const long ld = n;
    const size_t block = (size_t)width * n;
    DBuf<double> Sbuf(block), ASbuf(block), MSbuf(M ? block : 0);
    double *S = Sbuf.p, *AS = ASbuf.p, *MS = M ? MSbuf.p : S;
    Sbuf.zero(s);       // columns outside the basis take zero coefficients: they only have to stay finite
    ASbuf.zero(s);
    MSbuf.zero(s);
    DBuf<double> scratch(std::max(bv_gram_scratch(n, width, width), bv_residual_scratch(n)));
    DBuf<double> Gdev(2 * (size_t)width * width), Cdev((size_t)width * 2 * nb), lam_dev((size_t)nb), norms_dev(2 * BV_MAX_NORMS);
    const signed char *flags = o.constrain_essential ? L0.drel.flags.p : nullptr;
    auto column = [&](double *buf, int c) { return buf + (size_t)c * ld; };
    // the operator products of new basis columns: block members of the SpMV family, each column with the bits of spmv
    auto products = [&](const std::vector<int> &cols) {
        for (int c = 0; c < block_num_chunks((int)cols.size()); ++c) {
            const BlockChunk ch = block_chunk((int)cols.size(), c);
            const Cols xs(S, ld, ch.count, cols.data() + ch.first);
            spmv_block(s, A, xs, Cols(AS, ld, ch.count, cols.data() + ch.first));
            if (M) spmv_block(s, *M, xs, Cols(MS, ld, ch.count, cols.data() + ch.first));
        }
    };

    if (x0) copy_device(S, x0, (size_t)nb * n, s);
    else bv_hash_start(s, n, nb, o.seed, S, ld);
    if (flags) bv_mask(s, n, nb, flags, FLAG_ON_ESS_BORDER, S, ld);
    std::vector<int> cols(nb);
    for (int j = 0; j < nb; ++j) cols[j] = j;
    products(cols);

    bool have_w[lh::MAX_BLOCK] = {}, have_p[lh::MAX_BLOCK] = {}, active[lh::MAX_BLOCK] = {};
    std::vector<double> G(2 * (size_t)width * width), GA, GM, theta(width), C, Cfull((size_t)width * 2 * nb);
    std::vector<double> lam(nb, 0.0), rho(nb, std::numeric_limits<double>::infinity()), norms(2 * BV_MAX_NORMS);
    // R = A X - M X diag(lam) into the W columns of the A S buffer, and the rho_j
    auto residuals = [&]() {
        upload_async(lam_dev.p, (const double *)lam.data(), (size_t)nb, s);      // (read_back below synchronises)
        bv_residual(s, n, nb, AS, MS, ld, lam_dev.p, column(AS, 2 * nb), ld, scratch.p, norms_dev.p);
        read_back(norms.data(), norms_dev.p, norms.size(), s);
        for (int j = 0; j < nb; ++j) {
            const double den = std::fabs(lam[j]) * norms[BV_MAX_NORMS + j];
            rho[j] = (std::isfinite(den) && den > 0.0) ? norms[j] / den : std::numeric_limits<double>::infinity();
        }
    };
    int it = 0, conv = 0;
    for (;;) {
        bv_gram(s, n, width, S, ld, width, AS, ld, scratch.p, Gdev.p);
        bv_gram(s, n, width, S, ld, width, MS, ld, scratch.p, Gdev.p + (size_t)width * width);
        read_back(G.data(), Gdev.p, G.size(), s);
        int idx[lh::MAX_BASIS], m = 0, bad = -1;
        for (int attempt = 0; attempt < 2; ++attempt) {     // a breakdown drops P and repeats the step once: a restart
            m = 0;
            for (int j = 0; j < nb; ++j) idx[m++] = j;
            for (int j = 0; j < nb; ++j) if (have_w[j]) idx[m++] = 2 * nb + j;
            for (int j = 0; j < nb; ++j) if (have_p[j]) idx[m++] = nb + j;
            GA.resize((size_t)m * m);
            GM.resize((size_t)m * m);
            C.resize((size_t)m * m);
            lh::gather_gram(width, G.data(), m, idx, GA.data());
            lh::gather_gram(width, G.data() + (size_t)width * width, m, idx, GM.data());
            bad = lh::rayleigh_ritz(m, GA.data(), GM.data(), theta.data(), C.data());
            if (bad < 0) break;
            std::fill(have_p, have_p + nb, false);
        }
        if (bad >= 0) {         // a breakdown right after a restart: the best X so far
            if (it == 0) {
                for (int j = 0; j < nb; ++j) {
                    const double g = GM[j + (size_t)j * m];
                    lam[j] = (std::isfinite(g) && g > 0.0) ? GA[j + (size_t)j * m] / g : 0.0;
                }
                residuals();
                if (hist) std::copy(rho.begin(), rho.begin() + nev, hist);
            } else {
                it -= 1;
            }
            break;
        }
        lh::assemble_coefficients(width, nb, m, idx, C.data(), have_w, Cfull.data());
        upload_async(Cdev.p, (const double *)Cfull.data(), Cfull.size(), s);      // (residuals() synchronises before Cfull changes)
        // The whole buffer is combined: columns outside the basis meet zero rows of Cfull.  They must be FINITE (0 * inf
        // would poison X): the buffers start as zeros, and every column written since is a finite vector of an earlier basis.
        BvBlocks B{{S, AS, MS}, {S, AS, MS}, M ? 3 : 2};
        bv_combine(s, n, width, 2 * nb, Cdev.p, false, B, ld, ld);
        std::copy(have_w, have_w + nb, have_p);
        std::copy(theta.begin(), theta.begin() + nb, lam.begin());
        residuals();
        if (hist) std::copy(rho.begin(), rho.begin() + nev, hist + (size_t)it * nev);
        bool done = true;
        for (int j = 0; j < nev; ++j) done = done && rho[j] <= o.tol;
        if (done) { conv = 1; break; }
        if (it == o.max_iter) break;
        // the unlocked columns as one block: V-cycles, then the mask, then the products of the new W columns
        cols.clear();
        for (int j = 0; j < nb; ++j) {
            active[j] = !(rho[j] <= o.tol);
            have_w[j] = active[j];
            if (active[j]) cols.push_back(2 * nb + j);
        }
        const std::vector<double *> rs = block_columns(AS, ld, (int)cols.size(), cols.data());
        const std::vector<double *> ws = block_columns(S, ld, (int)cols.size(), cols.data());
        if (!cols.empty()) vcycle_apply_block(H, (int)cols.size(), rs.data(), ws.data());
        if (flags) for (int c : cols) bv_mask(s, n, 1, flags, FLAG_ON_ESS_BORDER, column(S, c), ld);
        products(cols);
        it += 1;
    }
    std::copy(lam.begin(), lam.begin() + nev, evals);
    if (res) std::copy(rho.begin(), rho.begin() + nev, res);
    if (iters) *iters = it;
    if (converged) *converged = conv;
    copy_device(evecs, (const double *)S, (size_t)nev * n, s);
    SA_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace saamge_amd
