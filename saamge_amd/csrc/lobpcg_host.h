// The small dense half of the eigensolver (lobpcg.hip), plain host C++17 without HIP: what saamge_amd/lobpcg_model.py does
// with the Gram pair of the basis S = [X, W, P] of at most 48 columns.  Matrices are column-major, order m, leading
// dimension m.  The library links no LAPACK: Cholesky, triangular solves and a cyclic Jacobi iteration are written out.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace saamge_amd {
namespace lobpcg_host {

constexpr int MAX_BLOCK = 16;
constexpr int MAX_BASIS = 48;

// A pivot of the Cholesky factor of a unit-diagonal Gram matrix of order m at or below this is a breakdown: the squared
// sine of the angle to the span of the columns before it is within the rounding of its own evaluation.
inline double pivot_floor(int m) { return 64.0 * m * DBL_EPSILON; }

// G = D L L^T D with D = sqrt(diag G), L lower triangular (its upper triangle is set to zero).  Returns -1, or the first
// column whose diagonal entry or pivot is not safely positive (not finite included).
inline int cholesky_scaled(int m, const double *G, double *d, double *L) {
    std::fill(L, L + (size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j) {
        const double g = G[j + (size_t)j * m];
        if (!(std::isfinite(g) && g > 0.0)) return j;
        d[j] = std::sqrt(g);
    }
    const double floor = pivot_floor(m);
    for (int j = 0; j < m; ++j) {
        for (int i = j; i < m; ++i) {
            double v = G[i + (size_t)j * m] / (d[i] * d[j]);
            for (int k = 0; k < j; ++k) v -= L[i + (size_t)k * m] * L[j + (size_t)k * m];
            L[i + (size_t)j * m] = v;
        }
        const double piv = L[j + (size_t)j * m];
        if (!(std::isfinite(piv) && piv > floor)) return j;
        const double r = std::sqrt(piv);
        for (int i = j; i < m; ++i) L[i + (size_t)j * m] /= r;
    }
    return -1;
}

// B (m x ncol) <- L^-1 B
inline void solve_lower(int m, const double *L, int ncol, double *B) {
    for (int c = 0; c < ncol; ++c) {
        double *b = B + (size_t)c * m;
        for (int i = 0; i < m; ++i) {
            double v = b[i];
            for (int k = 0; k < i; ++k) v -= L[i + (size_t)k * m] * b[k];
            b[i] = v / L[i + (size_t)i * m];
        }
    }
}

// B (m x ncol) <- L^-T B
inline void solve_upper_t(int m, const double *L, int ncol, double *B) {
    for (int c = 0; c < ncol; ++c) {
        double *b = B + (size_t)c * m;
        for (int i = m - 1; i >= 0; --i) {
            double v = b[i];
            for (int k = i + 1; k < m; ++k) v -= L[k + (size_t)i * m] * b[k];
            b[i] = v / L[i + (size_t)i * m];
        }
    }
}

inline void transpose_in_place(int m, double *A) {
    for (int j = 0; j < m; ++j)
        for (int i = j + 1; i < m; ++i) std::swap(A[i + (size_t)j * m], A[j + (size_t)i * m]);
}

inline void symmetrise(int m, double *A) {
    for (int j = 0; j < m; ++j)
        for (int i = j + 1; i < m; ++i) {
            const double v = 0.5 * (A[i + (size_t)j * m] + A[j + (size_t)i * m]);
            A[i + (size_t)j * m] = A[j + (size_t)i * m] = v;
        }
}

// Eigenpairs of the symmetric A (destroyed) by cyclic Jacobi rotations: w ascending, Q the orthonormal eigenvectors by
// column.  A rotation is skipped once its entry no longer changes the two diagonal entries; the sweeps end when one
// makes no rotation.  Returns the number of sweeps.
inline int jacobi_eigh(int m, double *A, double *Q, double *w) {
    std::fill(Q, Q + (size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) Q[i + (size_t)i * m] = 1.0;
    int sweep = 0;
    for (; sweep < 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p + (size_t)q * m], app = A[p + (size_t)p * m], aqq = A[q + (size_t)q * m];
                if (std::fabs(apq) <= 0.125 * DBL_EPSILON * (std::fabs(app) + std::fabs(aqq))) {
                    A[p + (size_t)q * m] = A[q + (size_t)p * m] = 0.0;
                    continue;
                }
                rotated = true;
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < m; ++k) {      // columns p, q of A and Q
                    const double akp = A[k + (size_t)p * m], akq = A[k + (size_t)q * m];
                    A[k + (size_t)p * m] = c * akp - s * akq;
                    A[k + (size_t)q * m] = s * akp + c * akq;
                    const double qkp = Q[k + (size_t)p * m], qkq = Q[k + (size_t)q * m];
                    Q[k + (size_t)p * m] = c * qkp - s * qkq;
                    Q[k + (size_t)q * m] = s * qkp + c * qkq;
                }
                for (int k = 0; k < m; ++k) {      // rows p, q of A
                    const double apk = A[p + (size_t)k * m], aqk = A[q + (size_t)k * m];
                    A[p + (size_t)k * m] = c * apk - s * aqk;
                    A[q + (size_t)k * m] = s * apk + c * aqk;
                }
                A[p + (size_t)q * m] = A[q + (size_t)p * m] = 0.0;
            }
        if (!rotated) break;
    }
    std::vector<int> order(m);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[a + (size_t)a * m] < A[b + (size_t)b * m]; });
    std::vector<double> Qs((size_t)m * m);
    for (int j = 0; j < m; ++j) {
        w[j] = A[order[j] + (size_t)order[j] * m];
        std::copy(Q + (size_t)order[j] * m, Q + (size_t)order[j] * m + m, Qs.begin() + (size_t)j * m);
    }
    std::copy(Qs.begin(), Qs.end(), Q);
    return sweep;
}

// The symmetric generalised eigenproblem of the Gram pair (GA, GM), both symmetrised first: theta ascending and C (m x m)
// with C^T GM C = I, C^T GA C = diag(theta).  Returns -1, or the column of the breakdown (theta, C untouched).
inline int rayleigh_ritz(int m, const double *GA, const double *GM, double *theta, double *C) {
    const size_t mm = (size_t)m * m;
    std::vector<double> ga(GA, GA + mm), gm(GM, GM + mm), d(m), L(mm), Q(mm);
    symmetrise(m, ga.data());
    symmetrise(m, gm.data());
    const int bad = cholesky_scaled(m, gm.data(), d.data(), L.data());
    if (bad >= 0) return bad;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) ga[i + (size_t)j * m] /= d[i] * d[j];
    solve_lower(m, L.data(), m, ga.data());         // L^-1 B
    transpose_in_place(m, ga.data());               // B^T L^-T  (B symmetric)
    solve_lower(m, L.data(), m, ga.data());         // L^-1 B L^-T
    symmetrise(m, ga.data());
    jacobi_eigh(m, ga.data(), Q.data(), theta);
    solve_upper_t(m, L.data(), m, Q.data());
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) C[i + (size_t)j * m] = Q[i + (size_t)j * m] / d[i];
    return -1;
}

// The basis lives in a buffer of `width` columns, basis column i (model order X, W, P) in buffer column idx[i].
// Gram matrix of the basis out of the Gram matrix of the whole buffer:
inline void gather_gram(int width, const double *Gfull, int m, const int *idx, double *G) {
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) G[i + (size_t)j * m] = Gfull[idx[i] + (size_t)idx[j] * width];
}

// The coefficients of one in-place update of the buffer, Cfull (width x 2 nb, zero where nothing is named):
//     column j < nb          new X_j = S C[:, j]
//     column nb + j, active  new P_j = the part of S C[:, j] that comes from W and P (the rows of X set to zero)
inline void assemble_coefficients(int width, int nb, int m, const int *idx, const double *C, const bool *active,
                                  double *Cfull) {
    std::fill(Cfull, Cfull + (size_t)width * 2 * nb, 0.0);
    for (int j = 0; j < nb; ++j)
        for (int i = 0; i < m; ++i) {
            Cfull[idx[i] + (size_t)j * width] = C[i + (size_t)j * m];
            if (active[j] && i >= nb) Cfull[idx[i] + (size_t)(nb + j) * width] = C[i + (size_t)j * m];
        }
}

}  // namespace lobpcg_host
}  // namespace saamge_amd
