// TEST: saamge_amd::api::AssembledOperator through libsaamge_amd.so.  Without an argument only the checks that need no GPU
// run; with "gpu" the operator of a 3 x 2 x 2 grid of Q1 hexes (matrices scaled per element, essential dofs on x = 0) is
// assembled, updated with other scalings and printed with its values as hexadecimal floats, and a right-hand side is
// eliminated.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

static std::vector<double> matrices(int NE, double step) {
    std::vector<double> m;
    for (int e = 0; e < NE; ++e)
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b) m.push_back((a == b ? 8.0 : -1.0 - 0.125 * ((a ^ b) & 3)) * (1.0 + step * e));
    return m;
}

static void print(const char *tag, const AssembledOperator &A) {
    std::vector<long long> rp;
    std::vector<int> col;
    std::vector<double> val;
    A.get(rp, col, val);
    std::printf("%s rowptr", tag);
    for (size_t i = 0; i < rp.size(); ++i) std::printf(" %lld", rp[i]);
    std::printf("\n%s col", tag);
    for (size_t k = 0; k < col.size(); ++k) std::printf(" %d", col[k]);
    std::printf("\n%s val", tag);
    for (size_t k = 0; k < val.size(); ++k) std::printf(" %a", val[k]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    bool threw = false;
    int one = 0;
    double m = 1.0;
    try { AssembledOperator A(-1, 0, 1, nullptr, nullptr, nullptr, nullptr); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "n < 0") != nullptr; }
    if (!threw) return 1;
    threw = false;
    try { AssembledOperator A(1, 1, 1, nullptr, nullptr, &m, nullptr); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "null argument") != nullptr; }
    if (!threw) return 2;
    threw = false;
    try { AssembledOperator A(1, 1, 0, nullptr, &one, &m, nullptr); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "nde") != nullptr; }
    if (!threw) return 3;
    if (!saamge_amd_operator_set_path_limits(65, -1) || !std::strstr(saamge_amd_last_error(), "path limits")) return 4;
    if (saamge_amd_operator_set_path_limits(-1, -1)) return 5;
    saamge_amd_operator_free(nullptr);
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 3, ny = 2, nz = 2, vx = nx + 1, vy = ny + 1, vz = nz + 1, NE = nx * ny * nz, n = vx * vy * vz;
        std::vector<int> e2d;
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x)
                    for (int c = 0; c < 8; ++c) e2d.push_back(((z + (c >> 2)) * vy + y + ((c >> 1) & 1)) * vx + x + (c & 1));
        std::vector<signed char> bdr((size_t)n, SAAMGE_AMD_OWNED);
        for (int i = 0; i < n; ++i)
            if (i % vx == 0) bdr[(size_t)i] |= SAAMGE_AMD_ON_ESS_DOMAIN_BORDER;
        const std::vector<double> m1 = matrices(NE, 0.0625), m2 = matrices(NE, 0.3);
        AssembledOperator A(n, NE, 8, nullptr, e2d.data(), m1.data(), bdr.data());
        if (A.rows() != n || !A.rowptr() || !A.col() || !A.val() || A.nnz() <= n) return 6;
        print("first", A);
        std::vector<double> x((size_t)n), b((size_t)n);
        for (int i = 0; i < n; ++i) { x[(size_t)i] = 0.25 + 0.0625 * i; b[(size_t)i] = 1.0 - 0.03125 * i; }
        A.eliminate_rhs(m1.data(), x.data(), b.data());
        std::printf("rhs");
        for (int i = 0; i < n; ++i) std::printf(" %a", b[(size_t)i]);
        std::printf("\n");
        const double *before = A.val();
        A.update(m2.data());
        if (A.val() != before) return 7;
        print("second", A);
    }
    std::printf("operator api test ok\n");
    return 0;
}
