// The eigensolver through the C++ layer (saamge_amd::api::lobpcg).  Without arguments: links the library and checks the
// refusals that need no GPU.  "gpu <problem> <out>": reads a problem tests/test_cxx_lobpcg.py wrote (ints n, nnz, NE, nde,
// nparts; then rowptr, col, val, elem_to_dof, elmat, bdr, partition, x0 n x 4 column-major), solves for four pairs and
// writes evals, res (4 each) and the vectors (n x 4) to <out> for the Python side to hold to the bounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

template <class F>
static std::string refused(F call) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}

template <class T>
static std::vector<T> read_array(std::FILE *f, size_t count) {
    std::vector<T> v(count);
    CHECK(std::fread(v.data(), sizeof(T), count, f) == count);
    return v;
}

static void refusals() {
    LobpcgOptions o;
    CHECK(o.nev == 1 && o.block == 0 && o.tol == 1e-8 && o.max_iter == 100 && o.constrain_essential == 1 && o.seed == 0);
    std::vector<double> X(16, -1.0);
    std::string msg = refused([&] { lobpcg(nullptr, o, X.data()); });
    CHECK(msg.find("null argument: h") != std::string::npos);
    for (double v : X) CHECK(v == -1.0);
    std::vector<double> S(64 * 4, 1.0), G(16, -1.0), C(16, 1.0);
    CHECK(saamge_amd_blockvec_gram(64, 0, S.data(), 64, 4, S.data(), 64, G.data()) != 0);
    CHECK(std::strstr(saamge_amd_last_error(), " p ") != nullptr);
    CHECK(saamge_amd_blockvec_gram(64, 4, S.data(), 64, 49, S.data(), 64, G.data()) != 0);
    CHECK(std::strstr(saamge_amd_last_error(), " q ") != nullptr);
    CHECK(saamge_amd_blockvec_gram(64, 4, S.data(), 63, 4, S.data(), 64, G.data()) != 0);
    CHECK(std::strstr(saamge_amd_last_error(), "lds") != nullptr);
    CHECK(saamge_amd_blockvec_combine(64, 4, S.data(), 64, 4, C.data(), S.data() + 64, 64, 0) != 0);
    CHECK(std::strstr(saamge_amd_last_error(), "overlaps") != nullptr);
    CHECK(saamge_amd_blockvec_combine(64, 4, S.data(), 64, 4, C.data(), G.data(), 63, 0) != 0);
    CHECK(std::strstr(saamge_amd_last_error(), "ldy") != nullptr);
    for (double v : G) CHECK(v == -1.0);
    for (double v : S) CHECK(v == 1.0);
}

static void solve(const char *problem, const char *out) {
    std::FILE *f = std::fopen(problem, "rb");
    CHECK(f);
    const std::vector<int> head = read_array<int>(f, 5);
    const int n = head[0], nnz = head[1], NE = head[2], nde = head[3];
    int nparts[1] = {head[4]};
    const std::vector<int> rowptr = read_array<int>(f, (size_t)n + 1), col = read_array<int>(f, (size_t)nnz);
    const std::vector<double> val = read_array<double>(f, (size_t)nnz);
    const std::vector<int> e2d = read_array<int>(f, (size_t)NE * nde);
    const std::vector<double> elmat = read_array<double>(f, (size_t)NE * nde * nde);
    const std::vector<signed char> bdr = read_array<signed char>(f, (size_t)n);
    const std::vector<int> part = read_array<int>(f, (size_t)NE);
    const std::vector<double> x0 = read_array<double>(f, (size_t)n * 4);
    std::fclose(f);
    ProblemArrays a;
    a.n = n;
    a.rowptr = rowptr.data();
    a.col = col.data();
    a.val = val.data();
    a.NE = NE;
    a.nde = nde;
    a.elem_to_dof = e2d.data();
    a.elmat = elmat.data();
    a.bdr_dofs = bdr.data();
    a.partitions.push_back(part.data());
    MultilevelParameters mlp(1, nparts, 0, 0, 3, 0.003, 0.003, -1, false, false, false);
    ml_data_t *h = ml_produce_data(a, mlp);
    LobpcgOptions o;
    o.nev = 4;
    o.max_iter = 80;
    std::vector<double> X((size_t)n * 4, 0.0);
    // out of range: refused by name, nothing written
    LobpcgOptions bad = o;
    bad.block = 3;
    CHECK(refused([&] { lobpcg(h, bad, X.data()); }).find("block") != std::string::npos);
    for (double v : X) CHECK(v == 0.0);
    const LobpcgResult r = lobpcg(h, o, X.data(), MassMatrix(), x0.data());
    CHECK(r.converged && r.iters <= 80 && r.hist.size() == (size_t)(r.iters + 1) * 4);
    for (int j = 0; j < 4; ++j) CHECK(r.hist[(size_t)r.iters * 4 + j] == r.res[j] && r.res[j] <= 1e-8);
    ml_free_data(h);
    std::FILE *g = std::fopen(out, "wb");
    CHECK(g);
    CHECK(std::fwrite(r.evals.data(), 8, 4, g) == 4 && std::fwrite(r.res.data(), 8, 4, g) == 4);
    CHECK(std::fwrite(X.data(), 8, X.size(), g) == X.size());
    std::fclose(g);
    std::printf("iters %d\n", r.iters);
}

int main(int argc, char **argv) {
    refusals();
    if (argc == 4 && std::strcmp(argv[1], "gpu") == 0) solve(argv[2], argv[3]);
    std::printf("lobpcg api test ok\n");
    return 0;
}
