// The block solve calls through the C++ layer (saamge_amd::api::spmv_block, smoother_block, vcycle_block, pcg_block) and the
// chunking rule of the block kernels (saamge_amd/csrc/block_chunks.h).  Without arguments: holds the chunking rule on the CPU,
// links the library and checks the refusals that need no GPU.  "gpu <problem>": reads a problem tests/test_cxx_cycle_block.py
// wrote (ints n, nnz, NE, nde, nparts; then rowptr, col, val, elem_to_dof, elmat, bdr, partition, K columns n x K
// column-major), and compares each of the four block calls with the single-vector call per column, byte for byte.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "block_chunks.h"
#include "saamge_amd.hpp"

using namespace saamge_amd::api;
namespace sa = saamge_amd;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

// ---- the chunking rule ---------------------------------------------------------------------------------------------------
static_assert(sa::block_width(1) == 1 && sa::block_width(2) == 2 && sa::block_width(3) == 4 && sa::block_width(4) == 4 &&
                  sa::block_width(5) == 8 && sa::block_width(8) == 8,
              "the narrowest instantiated width that holds the columns");
static_assert(sa::block_num_chunks(1) == 1 && sa::block_num_chunks(8) == 1 && sa::block_num_chunks(9) == 2 &&
                  sa::block_num_chunks(64) == 8,
              "chunks of at most BLOCK_MAX columns");
static_assert(sa::block_chunk(11, 1).first == 8 && sa::block_chunk(11, 1).count == 3 && sa::block_chunk(11, 1).width == 4 &&
                  sa::block_chunk(11, 1).mask == 7u,
              "the last chunk of 11 columns");

static void chunk_rule() {
    for (int k = 1; k <= 64; ++k) {
        std::vector<int> seen((size_t)k, 0);
        for (int c = 0; c < sa::block_num_chunks(k); ++c) {
            const sa::BlockChunk ch = sa::block_chunk(k, c);
            CHECK(ch.count >= 1 && ch.count <= sa::BLOCK_MAX && ch.count <= ch.width);
            bool instantiated = false;
            for (int w : sa::BLOCK_WIDTHS) instantiated = instantiated || w == ch.width;
            CHECK(instantiated);
            CHECK(ch.width == 1 || ch.width / 2 < ch.count);      // the narrowest width that holds the chunk
            for (int j = 0; j < ch.width; ++j) {
                const bool stored = ((ch.mask >> j) & 1u) != 0;
                const int col = sa::block_slot_column(ch, j);
                CHECK(col >= 0 && col < k);
                CHECK(stored == (j < ch.count));
                if (stored) seen[(size_t)col] += 1;
                else CHECK(col >= ch.first && col < ch.first + ch.count);      // a padded slot points at an active column
            }
            CHECK((ch.mask >> ch.width) == 0u);
        }
        for (int v : seen) CHECK(v == 1);      // every column in exactly one chunk, stored once
    }
}

template <class F>
static std::string refused(F call) {
    try {
        call();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}
static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

template <class T>
static std::vector<T> read_array(std::FILE *f, size_t count) {
    std::vector<T> v(count);
    CHECK(std::fread(v.data(), sizeof(T), count, f) == count);
    return v;
}

static void refusals() {
    const int rowptr[4] = {0, 1, 2, 3}, col[3] = {0, 1, 2};
    const double val[3] = {1.0, 2.0, 3.0};
    std::vector<double> X(12, 1.0), Y(12, -1.0);
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 0, X.data(), 3, Y.data(), 3); }), "k must lie"));
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 65, X.data(), 3, Y.data(), 3); }), "k must lie"));
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 2, X.data(), 2, Y.data(), 3); }), "leading dimension"));
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 2, X.data(), 3, Y.data(), 2); }), "leading dimension"));
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 2, nullptr, 3, Y.data(), 3); }), "null block"));
    CHECK(has(refused([&] { spmv_block(3, 3, rowptr, col, val, 2, X.data(), 3, X.data() + 2, 3); }), "overlaps"));
    CHECK(has(refused([&] { smoother_block(nullptr, 0, 2, X.data(), 3, Y.data(), 3); }), "null hierarchy"));
    CHECK(has(refused([&] { vcycle_block(nullptr, 2, X.data(), 3, Y.data(), 3); }), "null hierarchy"));
    CHECK(has(refused([&] { pcg_block(nullptr, 2, X.data(), 3, Y.data(), 3, 1e-6, 0.0, 3); }), "null hierarchy"));
    for (double v : Y) CHECK(v == -1.0);
    for (double v : X) CHECK(v == 1.0);
}

static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

static void solve(const char *problem) {
    const int K = 3, PAD = 5, MAX_ITER = 3;
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
    const std::vector<double> cols = read_array<double>(f, (size_t)n * K);
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
    const size_t ld = (size_t)n + PAD;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> B(ld * K, nan), X(ld * K, nan), one((size_t)n);
    for (int j = 0; j < K; ++j) std::memcpy(&B[ld * j], &cols[(size_t)n * j], sizeof(double) * n);
    auto padding_untouched = [&] {
        for (int j = 0; j < K; ++j)
            for (int i = n; i < (int)ld; ++i) CHECK(std::isnan(X[ld * j + i]));
    };
    // spmv_block against saamge_amd_spmv
    spmv_block(n, n, rowptr.data(), col.data(), val.data(), K, B.data(), (long long)ld, X.data(), (long long)ld);
    for (int j = 0; j < K; ++j) {
        CHECK(saamge_amd_spmv(n, n, rowptr.data(), col.data(), val.data(), &cols[(size_t)n * j], one.data()) == 0);
        CHECK(same(&X[ld * j], one.data(), (size_t)n));
    }
    padding_untouched();
    // vcycle_block against VCycleSolver::Mult
    vcycle_block(h, K, B.data(), (long long)ld, X.data(), (long long)ld);
    for (int j = 0; j < K; ++j) {
        VCycleSolver(h).Mult(&cols[(size_t)n * j], one.data());
        CHECK(same(&X[ld * j], one.data(), (size_t)n));
    }
    padding_untouched();
    // smoother_block from the V-cycle's result against smpr_sym_poly
    std::vector<double> start = X;
    smoother_block(h, 0, K, B.data(), (long long)ld, X.data(), (long long)ld);
    for (int j = 0; j < K; ++j) {
        std::memcpy(one.data(), &start[ld * j], sizeof(double) * n);
        smpr_sym_poly(h, 0, &cols[(size_t)n * j], one.data());
        CHECK(same(&X[ld * j], one.data(), (size_t)n));
    }
    padding_untouched();
    // pcg_block against saamge_amd_pcg
    std::fill(X.begin(), X.end(), nan);
    const PcgBlockResult r = pcg_block(h, K, B.data(), (long long)ld, X.data(), (long long)ld, 1e-8, 0.0, MAX_ITER);
    for (int j = 0; j < K; ++j) {
        int it = 0, conv = 0;
        std::vector<double> hist((size_t)MAX_ITER + 1, nan);
        CHECK(saamge_amd_pcg(h, &cols[(size_t)n * j], one.data(), 1e-8, 0.0, MAX_ITER, 1, 1, &it, &conv, hist.data()) == 0);
        CHECK(same(&X[ld * j], one.data(), (size_t)n));
        CHECK(r.iters[(size_t)j] == it && r.converged[(size_t)j] == conv);
        CHECK(same(&r.hist[(size_t)j * (MAX_ITER + 1)], hist.data(), (size_t)it + 1));
        for (int i = it + 1; i <= MAX_ITER; ++i) CHECK(std::isnan(r.hist[(size_t)j * (MAX_ITER + 1) + i]));
    }
    padding_untouched();
    ml_free_data(h);
}

int main(int argc, char **argv) {
    chunk_rule();
    refusals();
    if (argc == 3 && std::strcmp(argv[1], "gpu") == 0) solve(argv[2]);
    std::printf("cycle block api test ok\n");
    return 0;
}
