// The small dense half of the eigensolver (saamge_amd/csrc/lobpcg_host.h) on the host, under the address and
// undefined-behaviour sanitizers: Cholesky with a reported pivot, the triangular solves, the symmetric generalised
// eigenproblem by Cholesky reduction and cyclic Jacobi, and the assembly of the coefficients.  The pencils are closed
// forms that numpy evaluates to the same bits (one division per entry); EXPECT_m holds scipy.linalg.eigh(GA, GM) of them,
// written out with repr().  A computed pair (theta, c) with c^T GM c = 1 has an eigenvalue within
// beta = ||GA c - theta GM c||_{GM^-1} of theta; the written-out values carry LAPACK's own rounding, for which
// 8 m eps max|lambda| is allowed (an allowance of the usual size of a backward-stable solver's error, not a bound).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "lobpcg_host.h"

using namespace saamge_amd::lobpcg_host;

static const double EXPECT_1[1] = {
    2.8571428571428563
};
static const double EXPECT_2[2] = {
    2.013990699266239, 2.976615620118901
};
static const double EXPECT_3[3] = {
    1.983528224368025, 2.031248774987588, 3.014970508601521
};
static const double EXPECT_47[47] = {
    1.98349527781923, 2.028450841318159, 2.9441074019604114, 3.4749205882875667, 3.956563238856653,
    4.890681163906182, 4.9210605177182964, 5.849379066424167, 6.351865288438934, 7.667674153129656,
    7.77140231296557, 7.849002875967768, 9.24323393034957, 9.709503436904336, 10.564120603603534, 10.71277194965254,
    11.635573942008653, 12.168567431399376, 13.387183735082854, 13.560724304743099, 13.684142693799714,
    15.05486287602751, 15.521207304865738, 16.30866479151314, 16.53319394563396, 17.446621910762765,
    17.995997108407536, 19.150174307441585, 19.363962528324294, 19.514627101245683, 20.903843717929757,
    21.339426523059647, 22.06458361464656, 22.42514523327625, 23.273142995297643, 24.918238409975675,
    25.217281625653566, 27.121710363098302, 27.81781111787566, 29.068480432232455, 30.67765645612937,
    31.052583634631194, 33.561025020664395, 36.430851934757584, 39.303267917400255, 42.186764111939326,
    45.14122920688917
};
static const double EXPECT_48[48] = {
    1.9834952232192216, 2.0284494723724262, 2.944103411831535, 3.474918249127091, 3.9565608505040686,
    4.89068107849495, 4.921057568943273, 5.849378690308293, 6.351865287627822, 7.667673854489911, 7.771401465742405,
    7.8490026382011475, 9.24322607224747, 9.709500640784052, 10.56411427262038, 10.712754634658545,
    11.635556200819723, 12.168519930707413, 13.387103491038554, 13.560659932700654, 13.684120184874219,
    15.054541881708193, 15.521150983737254, 16.3085584176573, 16.532650000802214, 17.446330387284604,
    17.99474210988902, 19.149338421875314, 19.362142815727818, 19.513483172504504, 20.893738462540092,
    21.339114478751693, 22.063681801703733, 22.392404823906155, 23.269343996032394, 23.917322171024406,
    24.92198853391983, 25.22458297261783, 27.13238139443511, 27.81825073300761, 29.08553347547939,
    30.680116339172304, 31.087521822483268, 33.561508027171094, 36.43212097992869, 39.30603451172653,
    42.19297076930638, 45.1554154475862
};

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void pencil(int m, std::vector<double> &GA, std::vector<double> &GM) {
    GA.assign((size_t)m * m, 0.0);
    GM.assign((size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            GA[i + (size_t)j * m] = 1.0 / (1.0 + i + j) + (i == j ? 2.0 + i : 0.0);
            GM[i + (size_t)j * m] = 0.1 / (2.0 + std::abs(i - j)) + (i == j ? 1.0 + 0.5 * (i % 3) : 0.0);
        }
}

static std::vector<double> matvec(int m, const std::vector<double> &A, const double *x) {
    std::vector<double> y(m, 0.0);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) y[i] += A[i + (size_t)j * m] * x[j];
    return y;
}

static double dot(int m, const double *a, const double *b) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += a[i] * b[i];
    return s;
}

// ||r||_{GM^-1} through the factor GM = D L L^T D: || L^-1 D^-1 r ||_2
static double minv_norm(int m, const std::vector<double> &GM, std::vector<double> r) {
    std::vector<double> d(m), L((size_t)m * m);
    CHECK(cholesky_scaled(m, GM.data(), d.data(), L.data()) == -1);
    for (int i = 0; i < m; ++i) r[i] /= d[i];
    solve_lower(m, L.data(), 1, r.data());
    return std::sqrt(dot(m, r.data(), r.data()));
}

static void check_pencil(int m, const std::vector<double> &GA, const std::vector<double> &GM, const double *expect) {
    const double eps = std::numeric_limits<double>::epsilon();
    std::vector<double> theta(m), C((size_t)m * m);
    CHECK(rayleigh_ritz(m, GA.data(), GM.data(), theta.data(), C.data()) == -1);
    double top = 0.0;
    for (int j = 0; j < m; ++j) top = std::fmax(top, std::fabs(expect[j]));
    for (int j = 0; j < m; ++j) {
        const double *c = C.data() + (size_t)j * m;
        CHECK(j == 0 || theta[j] >= theta[j - 1]);
        std::vector<double> ac = matvec(m, GA, c), mc = matvec(m, GM, c);
        const double norm2 = dot(m, c, mc.data());
        CHECK(std::fabs(norm2 - 1.0) <= 64.0 * m * eps);
        std::vector<double> r(m);
        for (int i = 0; i < m; ++i) r[i] = ac[i] - theta[j] * mc[i];
        const double beta = minv_norm(m, GM, r) / std::sqrt(norm2);
        CHECK(std::fabs(theta[j] - expect[j]) <= beta + 8.0 * m * eps * top);
        CHECK(beta <= 64.0 * m * eps * top);        // the pairs are converged: the residual is rounding of order m
        for (int k = 0; k < j; ++k)                 // M-orthogonal to the pairs before it
            CHECK(std::fabs(dot(m, C.data() + (size_t)k * m, mc.data())) <= 64.0 * m * eps);
    }
}

int main() {
    const double eps = std::numeric_limits<double>::epsilon();
    std::vector<double> GA, GM;
    const int orders[5] = {1, 2, 3, 47, 48};
    const double *expect[5] = {EXPECT_1, EXPECT_2, EXPECT_3, EXPECT_47, EXPECT_48};
    for (int t = 0; t < 5; ++t) {
        pencil(orders[t], GA, GM);
        check_pencil(orders[t], GA, GM, expect[t]);
    }
    {   // Cholesky and the triangular solves on their own: D L L^T D reproduces GM, L^-1 and L^-T invert L and L^T
        const int m = 48;
        pencil(m, GA, GM);
        std::vector<double> d(m), L((size_t)m * m), B, X;
        CHECK(cholesky_scaled(m, GM.data(), d.data(), L.data()) == -1);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {
                double s = 0.0;
                for (int k = 0; k <= std::min(i, j); ++k) s += L[i + (size_t)k * m] * L[j + (size_t)k * m];
                CHECK(std::fabs(s * d[i] * d[j] - GM[i + (size_t)j * m]) <= 8.0 * m * eps * d[i] * d[j]);
                if (i < j) CHECK(L[i + (size_t)j * m] == 0.0);
            }
        B = GA;
        X = GA;
        solve_lower(m, L.data(), m, X.data());
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {          // L X = B
                double s = 0.0;
                for (int k = 0; k <= i; ++k) s += L[i + (size_t)k * m] * X[k + (size_t)j * m];
                CHECK(std::fabs(s - B[i + (size_t)j * m]) <= 64.0 * m * eps * (1.0 + std::fabs(B[i + (size_t)j * m])));
            }
        X = GA;
        solve_upper_t(m, L.data(), m, X.data());
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {          // L^T X = B
                double s = 0.0;
                for (int k = i; k < m; ++k) s += L[k + (size_t)i * m] * X[k + (size_t)j * m];
                CHECK(std::fabs(s - B[i + (size_t)j * m]) <= 64.0 * m * eps * (1.0 + std::fabs(B[i + (size_t)j * m])));
            }
    }
    {   // a repeated eigenvalue: (T^T diag(2, 4, 6, 12) T, T^T diag(1, 2, 3, 4) T) with the unit upper triangle of ones T
        // has the eigenvalues 2, 2, 2, 3 (integers throughout: the pencil is exact)
        const int m = 4;
        const double da[4] = {2, 4, 6, 12}, dm[4] = {1, 2, 3, 4}, want[4] = {2, 2, 2, 3};
        GA.assign(16, 0.0);
        GM.assign(16, 0.0);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i)
                for (int k = 0; k <= std::min(i, j); ++k) {     // T(k, i) = 1 for k <= i
                    GA[i + j * m] += da[k];
                    GM[i + j * m] += dm[k];
                }
        check_pencil(m, GA, GM, want);
    }
    {   // Gram matrices that are not safely positive definite report the column and leave the outputs alone
        const double sentinel = -3.5;
        std::vector<double> theta(3, sentinel), C(9, sentinel), d(3), L(9);
        const double indefinite[4] = {1, 2, 2, 1};
        CHECK(cholesky_scaled(2, indefinite, d.data(), L.data()) == 1);
        CHECK(rayleigh_ritz(2, indefinite, indefinite, theta.data(), C.data()) == 1);
        const double repeated[9] = {2, 1, 2, 1, 3, 1, 2, 1, 2};       // column 2 repeats column 0: a zero pivot
        CHECK(rayleigh_ritz(3, repeated, repeated, theta.data(), C.data()) == 2);
        const double zero_diag[4] = {1, 0, 0, 0}, negative[1] = {-1.0};
        CHECK(cholesky_scaled(2, zero_diag, d.data(), L.data()) == 1);
        CHECK(cholesky_scaled(1, negative, d.data(), L.data()) == 0);
        const double not_a_number[4] = {1, 0, 0, std::nan("")}, infinite[1] = {INFINITY};
        CHECK(cholesky_scaled(2, not_a_number, d.data(), L.data()) == 1);
        CHECK(cholesky_scaled(1, infinite, d.data(), L.data()) == 0);
        for (double v : theta) CHECK(v == sentinel);
        for (double v : C) CHECK(v == sentinel);
        CHECK(pivot_floor(48) > 0.0 && pivot_floor(48) < 1e-12);
    }
    {   // the basis in a buffer of 3 nb columns: X in [0, nb), P_j in nb + j, W_j in 2 nb + j; model order X, W, P
        const int nb = 2, width = 6, m = 4;
        const int idx[4] = {0, 1, 2 * nb + 1, nb + 0};            // X_0, X_1, W_1, P_0
        std::vector<double> Gfull(36), G(16), C(16), Cfull((size_t)width * 2 * nb, -1.0);
        for (int i = 0; i < 36; ++i) Gfull[i] = i;
        gather_gram(width, Gfull.data(), m, idx, G.data());
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) CHECK(G[i + j * m] == idx[i] + 6 * idx[j]);
        for (int i = 0; i < 16; ++i) C[i] = 100 + i;
        const bool active[2] = {false, true};
        assemble_coefficients(width, nb, m, idx, C.data(), active, Cfull.data());
        for (int j = 0; j < 2 * nb; ++j)
            for (int r = 0; r < width; ++r) {
                double want = 0.0;
                for (int i = 0; i < m; ++i)
                    if (idx[i] == r) {
                        if (j < nb) want = C[i + j * m];
                        else if (j - nb == 1 && i >= nb) want = C[i + (j - nb) * m];      // P of the active column only
                    }
                CHECK(Cfull[r + (size_t)j * width] == want);
            }
    }
    std::printf("lobpcg host test ok\n");
    return 0;
}
