// The kernel plan of the few-eigenpairs driver (saamge_amd/csrc/eig_ss_plan.h) against the values its thresholds had as
// conditions inside the driver.  Every expected value below is written out: none is computed by the header under test.
#include "eig_ss_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace saamge_amd;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void solve(int max_n, int bwmax, int nb, int nact, SsSolve kind, int threads, int wr, long lds_bytes, int copy_ny, int line) {
    const SsSolvePlan p = ss_solve_plan(max_n, bwmax, nb, nact);
    const bool ok = p.kind == kind && p.threads == threads && p.wr == wr && (lds_bytes < 0 || (long)p.lds_bytes == lds_bytes) &&
                    p.copy_ny == copy_ny;
    if (!ok) {
        std::printf("FAILED line %d: ss_solve_plan(%d, %d, %d, %d) = kind %d, threads %d, wr %d, lds %zu, copy_ny %d\n", line, max_n, bwmax, nb,
                    nact, (int)p.kind, p.threads, p.wr, p.lds_bytes, p.copy_ny);
        ++failures;
    }
}
#define SOLVE(...) solve(__VA_ARGS__, __LINE__)

int main() {
    // ---- LDS window of the banded Cholesky ----
    for (int bw = 0; bw <= 51; ++bw) CHECK(ss_lds_window(bw) == 67);
    CHECK(ss_lds_window(52) == 68);
    for (int bw = 53; bw <= 64; ++bw) CHECK(ss_lds_window(bw) == 80);
    for (int bw = 65; bw <= 112; ++bw) CHECK(ss_lds_window(bw) == 128);
    CHECK(ss_lds_window(113) == 0);
    CHECK(ss_lds_window(4000) == 0);
    CHECK(SS_NARROWEST_WINDOW_BAND == 51);

    // ---- width of the iteration block, and the wanted pairs a width accepts ----
    CHECK(ss_block_width(405, 6) == 8);
    CHECK(ss_block_width(405, 12) == 8);
    CHECK(ss_block_width(405, 13) == 16);
    CHECK(ss_block_width(405, 14) == 16);
    CHECK(ss_block_width(405, 15) == 8);
    CHECK(ss_block_width(1280, 7) == 8);
    CHECK(ss_block_width(1281, 6) == 8);
    CHECK(ss_block_width(1281, 7) == 16);
    CHECK(ss_block_width(1281, 14) == 16);
    CHECK(ss_block_width(1281, 15) == 8);
    CHECK(ss_want_limit(8) == 12);
    CHECK(ss_want_limit(16) == 14);

    // ---- solves: block of eight, at most 1 280 rows: right-hand sides in LDS ----
    SOLVE(405, 51, 8, 100, SsSolve::LdsPrefetch128, 128, 0, 8L * 405 * 9 + 64, 0);
    SOLVE(405, 112, 8, 100, SsSolve::LdsPrefetch128, 128, 0, 29224, 0);
    SOLVE(405, 113, 8, 100, SsSolve::Lds256, 256, 0, 29224, 0);
    SOLVE(405, 240, 8, 100, SsSolve::Lds256, 256, 0, 29224, 0);
    SOLVE(405, 241, 8, 100, SsSolve::Lds512, 512, 0, 29224, 0);
    SOLVE(1280, 600, 8, 100, SsSolve::Lds512, 512, 0, 8L * 1280 * 9 + 64, 0);
    SOLVE(100, 99, 8, 1, SsSolve::LdsPrefetch128, 128, 0, 7264, 0);      // (rows = min(max_n, bwmax + 16) = 100)
    // ---- solves: otherwise ----
    SOLVE(1281, 600, 8, 10, SsSolve::Window4, 1024, 633, 40512, 5);
    SOLVE(1281, 600, 8, 256, SsSolve::Window4, 1024, 633, 40512, 5);
    SOLVE(1281, 600, 8, 257, SsSolve::Window0x2, 1024, 633, 40512, 5);
    SOLVE(1281, 1100, 8, 257, SsSolve::Window4, 1024, 1133, 72512, 5);      // 72 512 B > 70 KB
    SOLVE(2500, 2367, 8, 1, SsSolve::Window4, 1024, 2399, 153536, 9);
    SOLVE(2500, 2368, 8, 1, SsSolve::Stream1024, 1024, 0, 0, 9);             // window 153 664 B > 150 KB
    SOLVE(560, 5, 16, 3, SsSolve::Stream256, 256, 0, 0, 2);
    SOLVE(768, 5, 16, 3, SsSolve::Stream256, 256, 0, 0, 3);
    SOLVE(769, 5, 16, 3, SsSolve::Window4, 1024, 49, 6272, 3);
    SOLVE(1300, 1200, 16, 1, SsSolve::Stream1024, 1024, 0, 0, 5);            // window 157 824 B
    SOLVE(8000, 700, 8, 1, SsSolve::Window4, 1024, 733, 46912, 16);
    SOLVE(200, 5, 16, 3, SsSolve::Stream256, 256, 0, 0, 1);

    // ---- panel threads of the two factor walks ----
    CHECK(ss_blocked_panel_threads(449, 400, 8) == 512);
    CHECK(ss_blocked_panel_threads(448, 400, 8) == 256);
    CHECK(ss_blocked_panel_threads(2000, 320, 8) == 256);
    CHECK(ss_blocked_panel_threads(2000, 321, 8) == 512);
    CHECK(ss_blocked_panel_threads(2000, 384, 4) == 256);
    CHECK(ss_blocked_panel_threads(2000, 385, 4) == 512);
    CHECK(ss_two_panel_threads(769, 737) == 1024);
    CHECK(ss_two_panel_threads(768, 767) == 256);
    CHECK(ss_two_panel_threads(2000, 736) == 256);
    CHECK(ss_two_panel_threads(2000, 737) == 1024);

    // ---- the two-panel walk on two streams ----
    { const SsSplit s = ss_two_stream_split(64, false, false); CHECK(s.two && s.first == 32); }
    { const SsSplit s = ss_two_stream_split(63, false, false); CHECK(!s.two && s.first == 63); }
    { const SsSplit s = ss_two_stream_split(70, false, false); CHECK(s.two && s.first == 40); }
    { const SsSplit s = ss_two_stream_split(64, true, false); CHECK(!s.two && s.first == 64); }
    { const SsSplit s = ss_two_stream_split(64, false, true); CHECK(!s.two && s.first == 64); }

    // ---- iterations that read the state back ----
    CHECK(!ss_reads_state(405, 0));
    CHECK(!ss_reads_state(1281, 0));
    CHECK(ss_reads_state(405, 1));
    CHECK(!ss_reads_state(405, 2));
    CHECK(ss_reads_state(405, 3));
    CHECK(!ss_reads_state(405, 4));
    CHECK(ss_reads_state(405, 6));
    CHECK(ss_reads_state(1281, 2));
    CHECK(!ss_reads_state(1280, 2));

    // ---- workgroups that share a matrix in the band copies ----
    CHECK(ss_band_copy_ny(1) == 64);
    CHECK(ss_band_copy_ny(128) == 64);
    CHECK(ss_band_copy_ny(577) == 14);
    CHECK(ss_band_copy_ny(10000) == 1);

    if (failures) { std::printf("eig_ss plan test: %d failures\n", failures); return 1; }
    std::printf("eig_ss plan test ok\n");
    return 0;
}
