// Kernel plan of the few-eigenpairs driver (eig2.hip, "Few-eigenpairs path"): every threshold by which the driver picks
// a kernel, a thread count or a launch size, as pure host functions of the batch's sizes.  The driver switches on their
// results and holds no such number itself.  A wrong threshold usually still gives correct eigenpairs and costs only
// speed, so no test of the results would notice it: tests/cxx/eig_ss_plan_test.cpp holds these functions to the values they had
// when they were conditions inside the driver (DESIGN.md section 4.12 has the table and the measurements behind it).
// Host-only C++, no HIP includes.
#pragma once

#include <algorithm>
#include <cstddef>

namespace saamge_amd {

constexpr int SS_PLAN_SB = 16;      // the block of the banded factorisations and solves (EIG_SB; asserted in eig2.hip)
constexpr int SS_PLAN_B = 8;        // vectors of the narrow iteration block (SS_B)

// Window (rows) of the LDS-resident banded Cholesky, chol_band_lds2_kernel<window, .>, for a batch whose widest half
// bandwidth is bwmax: a window holds bands up to window - SB.  0: the band does not fit LDS, the factorisations walk
// the matrices in HBM.  (128: one workgroup per CU, 80: two, 68: three, 67: four -- see bc_pitch.)
constexpr int ss_lds_window(int bwmax) {
    return bwmax <= 67 - SS_PLAN_SB ? 67 : bwmax <= 68 - SS_PLAN_SB ? 68 : bwmax <= 80 - SS_PLAN_SB ? 80 : bwmax <= 128 - SS_PLAN_SB ? 128 : 0;
}
// the widest band the narrowest window takes (the agglomerate order of assemble.hip leaves such a band alone)
constexpr int SS_NARROWEST_WINDOW_BAND = ss_lds_window(0) - SS_PLAN_SB;

// Width of the iteration block: sixteen vectors where a matrix wants more pairs than the block of eight reaches -- more
// than its six for matrices whose solves stream the factor anyway (above 1 280 rows), more than the twelve that one
// lock adds for the others -- as long as sixteen reach (fourteen pairs).
constexpr int ss_want_limit(int nb) { return nb == 16 ? 16 - 2 : 2 * (SS_PLAN_B - 2); }
constexpr int ss_block_width(int max_n, int maxwant) {
    return (maxwant <= ss_want_limit(16) && ((max_n > 1280 && maxwant > SS_PLAN_B - 2) || maxwant > ss_want_limit(8))) ? 16 : 8;
}

// The two triangular solves of an iteration.
enum class SsSolve {
    LdsPrefetch128,      // ss_solve_lds_pf_kernel<128>: right-hand sides in LDS, factor entries three steps ahead
    Lds256,              // ss_solve_lds_kernel<256>
    Lds512,              // ss_solve_lds_kernel<512>
    Window4,             // ss_trsolve_win_kernel<., 4, 1, nb>: four tiles requested ahead, one workgroup per CU
    Window0x2,           // ss_trsolve_win_kernel<., 0, 2, nb>: nothing ahead, two workgroups per CU
    Stream1024,          // ss_trsolve_kernel<., 1024, nb>
    Stream256            // ss_trsolve_kernel<., 256, nb>
};
struct SsSolvePlan {
    SsSolve kind;
    int threads;             // per workgroup
    int wr;                  // rows of the LDS window of the window kernels (odd), 0 otherwise
    std::size_t lds_bytes;   // dynamic LDS of the launch
    int copy_ny;             // grid-y of ss_copy_active_kernel (the LDS kernels copy nothing: 0)
    bool lds() const { return kind == SsSolve::LdsPrefetch128 || kind == SsSolve::Lds256 || kind == SsSolve::Lds512; }
};
inline SsSolvePlan ss_solve_plan(int max_n, int bwmax, int nb, int nact) {
    if (max_n <= 1280 && nb == 8) {
        // right-hand sides resident in LDS (row pitch 9 doubles).  Narrow bands: the deep-prefetch kernel; wider ones: the
        // plain kernel, 256 (>= SB * SB threads: the block loads) or 512 threads by the rows a block step updates
        const int rows = std::min(max_n, bwmax + SS_PLAN_SB);
        const std::size_t bytes = sizeof(double) * (std::size_t)max_n * (SS_PLAN_B + 1) + 64;
        if (rows <= 128) return {SsSolve::LdsPrefetch128, 128, 0, bytes, 0};
        if (rows <= 256) return {SsSolve::Lds256, 256, 0, bytes, 0};
        return {SsSolve::Lds512, 512, 0, bytes, 0};
    }
    const int copy_ny = std::max(1, std::min(16, max_n / 256));
    const int wr = (std::min(max_n, std::max(bwmax, SS_PLAN_SB)) + 2 * SS_PLAN_SB) | 1;
    const std::size_t win_bytes = sizeof(double) * (std::size_t)nb * (std::size_t)wr;
    if (max_n > 768 && win_bytes <= 150 * 1024) {
        // more matrices than CUs: the variant without requests ahead, two workgroups per CU (config 5 at 64^3: solves
        // 448 -> 397 ms per step)
        if (nact > 256 && win_bytes <= 70 * 1024) return {SsSolve::Window0x2, 1024, wr, win_bytes, copy_ny};
        return {SsSolve::Window4, 1024, wr, win_bytes, copy_ny};
    }
    if (max_n > 768) return {SsSolve::Stream1024, 1024, 0, 0, copy_ny};
    return {SsSolve::Stream256, 256, 0, 0, copy_ny};
}

// Threads of a panel workgroup, by the rows a panel can have below its diagonal block.
// Blocked walk (outer blocks of G sub-panels, chol_panel_ll_kernel), rows_left = max_n - k0:
constexpr int ss_blocked_panel_threads(int rows_left, int bwmax, int G) {
    return std::min(rows_left, bwmax + SS_PLAN_SB * G) > 448 ? 512 : 256;
}
// Two-panel walk (chol_panel_kernel):
constexpr int ss_two_panel_threads(int max_n, int bwmax) { return std::min(max_n, bwmax + 2 * SS_PLAN_SB) > 768 ? 1024 : 256; }

// The two-panel walk runs the two halves of a batch on two streams (one half's panels beside the other half's updates):
// not under the profiler (its event pair brackets one stream), not in serial mode, not for small batches.  first: the
// matrices of the first half, a multiple of 8 (the XCD decode of the tiled kernels); first == count: one stream.
struct SsSplit {
    bool two;
    int first;
};
constexpr SsSplit ss_two_stream_split(int count, bool profiling, bool serial) {
    return (!profiling && !serial && count >= 64) ? SsSplit{true, (count / 2 + 7) / 8 * 8} : SsSplit{false, count};
}

// Does iteration `iter` read the state back (and rebuild the active list)?  After every iteration of the large matrices,
// whose iterations cost milliseconds; the small ones (LDS solves, ~0.1 ms for the few hundred survivors of a chunk) after
// iterations 1, 3, 6, 9, ...: the read-back's host round trip (~0.25 ms) was most of an iteration, an accepted matrix
// leaves the kernels at once, up to two spare iterations are cheap.
constexpr bool ss_reads_state(int max_n, int iter) { return iter >= 1 && (max_n > 1280 || iter == 1 || iter % 3 == 0); }

// grid-y of band_copy_kernel / ss_keep_transpose_kernel (workgroups that share a matrix)
constexpr int ss_band_copy_ny(int count) { return std::max(1, std::min(64, 8192 / std::max(1, count))); }

}  // namespace saamge_amd
