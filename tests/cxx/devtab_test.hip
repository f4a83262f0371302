// Self-checking program of the device index-table pieces (csrc/devtab.h, csrc/devsort.h): every result is compared with a
// serial host loop written here.  Prints one line per group and "devtab test ok" at the end; exits non-zero at the first
// mismatch with the case and the first differing index.  Built by csrc/Makefile next to the library:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Isaamge_amd/csrc tests/cxx/devtab_test.hip -Lsaamge_amd -lsaamge_amd
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "devsort.h"
#include "devtab.h"

using namespace saamge_amd;

namespace {

typedef unsigned long long u64;

struct Lcg {      // the inputs: one fixed generator
    u64 x = 0x9E3779B97F4A7C15ull;
    unsigned next() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)(x >> 33);
    }
    int below(int m) { return (int)(next() % (unsigned)m); }
};

[[noreturn]] void fail(const std::string &what, long index, double got, double want) {
    std::printf("devtab test FAILED: %s: index %ld: got %.17g, expected %.17g\n", what.c_str(), index, got, want);
    std::exit(1);
}
template <class T>
void expect_equal(const std::string &what, const std::vector<T> &got, const std::vector<T> &want) {
    if (got.size() != want.size()) fail(what + " (length)", -1, (double)got.size(), (double)want.size());
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i]) fail(what, (long)i, (double)got[i], (double)want[i]);
}
template <class T>
DBuf<T> to_device(const std::vector<T> &v, hipStream_t s, size_t extra = 0) {
    DBuf<T> d(v.size() + extra);
    if (!v.empty()) SA_HIP_CHECK(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    SA_HIP_CHECK(hipStreamSynchronize(s));
    return d;
}
template <class T>
std::vector<T> to_host(const T *p, size_t n, hipStream_t s) {
    std::vector<T> v(n);
    if (n) read_back(v.data(), p, n, s);
    return v;
}
std::string tag(const char *name, long a, long b = -1) {
    return std::string(name) + " " + std::to_string(a) + (b >= 0 ? "/" + std::to_string(b) : "");
}

// ---- scans -----------------------------------------------------------------------------------------------------------------
template <class OUT>
std::vector<OUT> host_scan(const std::vector<int> &in) {
    std::vector<OUT> out(in.size() + 1);
    OUT run = 0;
    for (size_t i = 0; i < in.size(); ++i) { out[i] = run; run += in[i]; }
    out[in.size()] = run;
    return out;
}
void scan_int_case(hipStream_t s, const std::vector<int> &in, const char *name) {
    const int n = (int)in.size();
    const auto want = host_scan<int>(in);
    DBuf<int> d_in = to_device(in, s), out((size_t)n + 1), sums((size_t)div_up(n, 1024) + 1);
    SA_HIP_CHECK(hipMemsetAsync(out.p, 0xff, sizeof(int) * ((size_t)n + 1), s));
    exclusive_scan_int(s, n, d_in.p, out.p);
    expect_equal(tag(name, n) + " sync", to_host((const int *)out.p, (size_t)n + 1, s), want);
    SA_HIP_CHECK(hipMemsetAsync(out.p, 0xff, sizeof(int) * ((size_t)n + 1), s));
    exclusive_scan_int_async(s, n, d_in.p, out.p, sums.p);
    expect_equal(tag(name, n) + " async", to_host((const int *)out.p, (size_t)n + 1, s), want);
}
void test_scan_int(hipStream_t s) {
    Lcg g;
    for (int n : {1, 255, 256, 257, 1023, 1024, 1025, 4096, 262144, 262145, 263170}) {
        std::vector<int> in((size_t)n);
        for (auto &v : in) v = g.below(8);
        scan_int_case(s, in, "scan int");
    }
    scan_int_case(s, std::vector<int>(1025, 0), "scan int zeros");
    std::printf("scan int: ok\n");
}
void test_scan_off(hipStream_t s) {
    const int ns[2] = {5, 1025}, vals[2] = {1 << 30, 1 << 21};
    for (int c = 0; c < 2; ++c) {
        const std::vector<int> in((size_t)ns[c], vals[c]);
        DBuf<int> d_in = to_device(in, s);
        DBuf<roff_t> out((size_t)ns[c] + 1);
        exclusive_scan_off(s, ns[c], d_in.p, out.p);
        expect_equal(tag("scan roff_t", ns[c]), to_host((const roff_t *)out.p, (size_t)ns[c] + 1, s), host_scan<roff_t>(in));
    }
    std::printf("scan roff_t: ok\n");
}

// ---- transpose -------------------------------------------------------------------------------------------------------------
struct Table {
    int nrows = 0, ncols = 0;
    std::vector<int> I{0}, J;
    void row(const std::vector<int> &cols) {
        J.insert(J.end(), cols.begin(), cols.end());
        I.push_back((int)J.size());
        ++nrows;
    }
};
// rows of the transpose ascending: rows are visited upwards
void host_transpose(const Table &t, std::vector<int> &TI, std::vector<int> &TJ) {
    std::vector<int> cnt((size_t)t.ncols, 0);
    for (int c : t.J) ++cnt[(size_t)c];
    TI = host_scan<int>(cnt);
    TJ.assign(t.J.size(), -1);
    std::vector<int> cur(TI.begin(), TI.end() - 1);
    for (int r = 0; r < t.nrows; ++r)
        for (int k = t.I[(size_t)r]; k < t.I[(size_t)r + 1]; ++k) TJ[(size_t)cur[(size_t)t.J[(size_t)k]]++] = r;
}
void transpose_case(hipStream_t s, hipStream_t side, const Table &t, const std::string &name) {
    std::vector<int> wantI, wantJ;
    host_transpose(t, wantI, wantJ);
    const long nnz = (long)t.J.size();
    DBuf<int> I = to_device(t.I, s), J = to_device(t.J, s, 1), cnt((size_t)t.ncols), sums((size_t)div_up(t.ncols, 1024) + 1);
    DBuf<int> TI((size_t)t.ncols + 1), TJ((size_t)nnz + 1);
    auto poison = [&](hipStream_t q) {
        SA_HIP_CHECK(hipMemsetAsync(TI.p, 0xff, sizeof(int) * TI.n, q));
        SA_HIP_CHECK(hipMemsetAsync(TJ.p, 0xff, sizeof(int) * TJ.n, q));
    };
    // sorted: the host's transpose exactly
    poison(s);
    dev_table_transpose(s, t.nrows, I.p, J.p, nnz, t.ncols, TI.p, TJ.p, true, cnt.p);
    expect_equal(name + " sorted I", to_host((const int *)TI.p, TI.n, s), wantI);
    expect_equal(name + " sorted J", to_host((const int *)TJ.p, (size_t)nnz, s), wantJ);
    // the same through the two halves
    poison(s);
    cnt.zero(s);
    dev_histogram(s, nnz, J.p, cnt.p);
    dev_table_finish(s, t.nrows, I.p, J.p, t.ncols, cnt.p, TI.p, TJ.p, true);
    expect_equal(name + " two-step I", to_host((const int *)TI.p, TI.n, s), wantI);
    expect_equal(name + " two-step J", to_host((const int *)TJ.p, (size_t)nnz, s), wantJ);
    // unsorted: every row as a multiset
    poison(s);
    dev_table_transpose(s, t.nrows, I.p, J.p, nnz, t.ncols, TI.p, TJ.p, false, cnt.p);
    expect_equal(name + " unsorted I", to_host((const int *)TI.p, TI.n, s), wantI);
    {
        auto got = to_host((const int *)TJ.p, (size_t)nnz, s);
        for (int c = 0; c < t.ncols; ++c) std::sort(got.begin() + wantI[(size_t)c], got.begin() + wantI[(size_t)c + 1]);
        expect_equal(name + " unsorted J (rows as multisets)", got, wantJ);
    }
    // async: a stream of its own, no host call between the enqueue and this program's synchronise
    poison(side);
    SA_HIP_CHECK(hipStreamSynchronize(side));
    dev_table_transpose_async(side, t.nrows, I.p, J.p, nnz, t.ncols, TI.p, TJ.p, true, cnt.p, sums.p);
    SA_HIP_CHECK(hipStreamSynchronize(side));
    expect_equal(name + " async I", to_host((const int *)TI.p, TI.n, s), wantI);
    expect_equal(name + " async J", to_host((const int *)TJ.p, (size_t)nnz, s), wantJ);
}
void test_transpose(hipStream_t s, hipStream_t side) {
    Lcg g;
    {
        Table t;
        t.ncols = 4;
        t.row({2, 0, 3});
        transpose_case(s, side, t, "transpose one row");
    }
    for (int wide = 0; wide < 2; ++wide) {      // empty rows, columns nobody lists; more columns than rows and fewer
        Table t;
        t.ncols = wide ? 90 : 11;
        const int nrows = wide ? 23 : 70;
        for (int r = 0; r < nrows; ++r) {
            std::vector<int> cols;
            if (r % 3 != 1)
                for (int k = g.below(5); k >= 0; --k) {
                    const int c = g.below(t.ncols);
                    if (c % 4 != 2 && std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
                }
            t.row(cols);
        }
        transpose_case(s, side, t, wide ? "transpose more columns than rows" : "transpose fewer columns than rows");
    }
    {
        Table t;      // one counter under contention, one row of the transpose longer than a workgroup
        t.ncols = 301;
        for (int r = 0; r < 300; ++r) t.row({1 + g.below(300), 0});
        transpose_case(s, side, t, "transpose 300 rows on column 0");
    }
    {
        Table t;      // 257 entries
        t.ncols = 40;
        int left = 257;
        while (left) {
            const int len = std::min(left, 1 + g.below(6));
            std::vector<int> cols;
            while ((int)cols.size() < len) {
                const int c = g.below(t.ncols);
                if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
            }
            t.row(cols);
            left -= len;
        }
        transpose_case(s, side, t, "transpose 257 entries");
    }
    std::printf("transpose (sorted, two-step, unsorted, async): ok\n");
}

// ---- compact ---------------------------------------------------------------------------------------------------------------
void test_compact(hipStream_t s) {
    Lcg g;
    const char *kinds[4] = {"none", "all", "alternating", "lcg"};
    for (int n : {1, 256, 257, 1025})
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<int> flag((size_t)n), want;
            for (int i = 0; i < n; ++i) {
                flag[(size_t)i] = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? (i & 1) : (g.below(3) == 0);
                if (flag[(size_t)i]) want.push_back(i);
            }
            DBuf<int> d_flag = to_device(flag, s), pos((size_t)n + 1), list;
            const int m = dev_compact(s, n, d_flag.p, pos.p, list);
            const std::string name = tag("compact", n) + " " + kinds[kind];
            if (m != (int)want.size()) fail(name + " (count)", -1, m, (double)want.size());
            if (list.n != (size_t)m) fail(name + " (list length)", -1, (double)list.n, m);
            expect_equal(name, to_host((const int *)list.p, (size_t)m, s), want);
        }
    std::printf("compact: ok\n");
}

// ---- elementwise -----------------------------------------------------------------------------------------------------------
template <class T>
void fill_case(hipStream_t s, int n, T v, const char *type) {
    DBuf<T> p((size_t)n + 1);
    SA_HIP_CHECK(hipMemsetAsync(p.p, 0, sizeof(T) * ((size_t)n + 1), s));
    dev_fill(s, n, v, p.p);
    std::vector<T> want((size_t)n + 1, v);
    want[(size_t)n] = 0;      // one past the end stays
    expect_equal(tag("fill", n) + " " + type, to_host((const T *)p.p, (size_t)n + 1, s), want);
}
template <class T>
void iota_case(hipStream_t s, int n, T scale, const char *type) {
    DBuf<T> p((size_t)n);
    dev_iota(s, n, scale, p.p);
    std::vector<T> want((size_t)n);
    for (int i = 0; i < n; ++i) want[(size_t)i] = (T)((long)i * scale);
    expect_equal(tag("iota", n) + " " + type, to_host((const T *)p.p, (size_t)n, s), want);
}
template <class T>
void gather_scatter_case(hipStream_t s, int n, Lcg &g, const char *type) {
    std::vector<int> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    for (int i = n - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)g.below(i + 1)]);
    std::vector<T> src((size_t)n), want_g((size_t)n), want_s((size_t)n);
    for (auto &v : src) v = (T)g.below(1000);
    for (int i = 0; i < n; ++i) {
        want_g[(size_t)i] = src[(size_t)perm[(size_t)i]];
        want_s[(size_t)perm[(size_t)i]] = src[(size_t)i];
    }
    DBuf<int> idx = to_device(perm, s);
    DBuf<T> d_src = to_device(src, s), dst((size_t)n);
    dev_gather(s, n, (const int *)idx.p, (const T *)d_src.p, dst.p);
    expect_equal(tag("gather", n) + " " + type, to_host((const T *)dst.p, (size_t)n, s), want_g);
    dev_scatter(s, n, (const int *)idx.p, (const T *)d_src.p, dst.p);
    expect_equal(tag("scatter", n) + " " + type, to_host((const T *)dst.p, (size_t)n, s), want_s);
}
void test_elementwise(hipStream_t s) {
    Lcg g;
    for (int n : {1, 256, 257}) {
        fill_case<int>(s, n, 0x7fffffff, "int");
        fill_case<u64>(s, n, ~0ull, "u64");
        fill_case<double>(s, n, 1.0, "double");
        iota_case<int>(s, n, 1, "int");
        iota_case<int>(s, n, 27, "int scaled");
        iota_case<int64_t>(s, n, (int64_t)1 << 31, "int64 past 2^31");      // i * scale passes 2^31 from i = 1
        // widening, and narrowing of values that fit
        std::vector<int> narrow((size_t)n);
        std::vector<roff_t> wide((size_t)n);
        for (int i = 0; i < n; ++i) {
            narrow[(size_t)i] = g.below(1 << 30) - (i & 1);
            wide[(size_t)i] = narrow[(size_t)i];
        }
        DBuf<int> d_narrow = to_device(narrow, s), back((size_t)n);
        DBuf<roff_t> d_wide((size_t)n);
        dev_convert(s, n, (const int *)d_narrow.p, d_wide.p);
        expect_equal(tag("widen", n), to_host((const roff_t *)d_wide.p, (size_t)n, s), wide);
        dev_convert(s, n, (const roff_t *)d_wide.p, back.p);
        expect_equal(tag("narrow", n), to_host((const int *)back.p, (size_t)n, s), narrow);
        gather_scatter_case<int>(s, n, g, "int");
        gather_scatter_case<double>(s, n, g, "double");
    }
    std::printf("fill, iota, convert, gather, scatter: ok\n");
}

void test_histogram(hipStream_t s) {
    Lcg g;
    for (int kind = 0; kind < 2; ++kind) {
        const int n = 1025, bins = 37;
        std::vector<int> key((size_t)n), want((size_t)bins, 0);
        for (auto &k : key) {
            k = kind ? g.below(bins) : 5;
            ++want[(size_t)k];
        }
        DBuf<int> d_key = to_device(key, s), cnt((size_t)bins);
        cnt.zero(s);
        dev_histogram(s, n, d_key.p, cnt.p);
        expect_equal(kind ? "histogram lcg keys" : "histogram equal keys", to_host((const int *)cnt.p, (size_t)bins, s), want);
    }
    std::printf("histogram: ok\n");
}

void test_sort(hipStream_t s) {
    Lcg g;
    if (bits_for(1) != 1 || bits_for(2) != 1 || bits_for(3) != 2 || bits_for(37) != 6 || bits_for(64) != 6 || bits_for(65) != 7)
        fail("bits_for", -1, bits_for(37), 6);
    for (int n : {1, 257, 5000})
        for (int nkeys : {1, 2, 37}) {
            std::vector<int> key((size_t)n), want((size_t)n);
            for (auto &k : key) k = g.below(nkeys);
            std::iota(want.begin(), want.end(), 0);
            std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
            DBuf<int> d_key = to_device(key, s), perm((size_t)n);
            stable_sort_by_key(s, n, d_key.p, nkeys, perm.p);
            expect_equal(tag("stable sort", n, nkeys), to_host((const int *)perm.p, (size_t)n, s), want);
        }
    std::printf("stable sort by key: ok\n");
}

}  // namespace

int main() {
    try {
        hipStream_t s = nullptr, side = nullptr;
        SA_HIP_CHECK(hipStreamCreate(&s));
        SA_HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        test_scan_int(s);
        test_scan_off(s);
        test_transpose(s, side);
        test_compact(s);
        test_elementwise(s);
        test_histogram(s);
        test_sort(s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        SA_HIP_CHECK(hipStreamSynchronize(side));
        SA_HIP_CHECK(hipStreamDestroy(s));
        SA_HIP_CHECK(hipStreamDestroy(side));
    } catch (const std::exception &e) {
        std::printf("devtab test FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("devtab test ok\n");
    return 0;
}
