// Kernel plan of the dense eigensolver (eig.hip; eig2.hip, "host driver" of the two-stage reduction): every threshold by
// which the drivers pick a kernel, a thread count, a grid or an LDS size, as pure host functions of the batch's sizes.  The
// drivers switch on their results and hold no such number themselves.  A wrong threshold usually still gives correct
// eigenpairs and costs only speed, or picks a kernel no test has run, so no test of the results would notice it:
// tests/cxx/eig_dense_plan_test.cpp holds these functions to the values they had when they were conditions inside the
// drivers (DESIGN.md section 4.17 has the table).  Host-only C++, no HIP includes.
#pragma once

#include <cstddef>
#include <cstdint>

namespace saamge_amd {

constexpr int DENSE_PLAN_SB = 16;        // band width of the two-stage reduction (EIG_SB; asserted in eig2.hip)
constexpr int DENSE_PLAN_NB = 32;        // panel width of the one-stage reduction (EIG_NB; asserted in eig.hip)
constexpr int DENSE_PLAN_TRI_NT = 1024;  // threads of the one-stage kernel (TRI_NT; asserted in eig.hip)
constexpr int DENSE_PLAN_VEC_MAXB = 254; // decoupled blocks of the inverse iteration (VEC_MAXB; asserted in eig.hip)
constexpr std::size_t DENSE_LDS_MAX = 160 * 1024;   // LDS of a workgroup

constexpr int dense_div_up(int a, int b) { return (a + b - 1) / b; }
// the tiled kernels decode (matrix, tile) from a linear id dealt over the 8 XCDs: their grids are dense_cnt8(count) * tiles
constexpr int dense_cnt8(int count) { return 8 * dense_div_up(count, 8); }

// ---- stage 1, dense -> band: the panels k0 = 0, SB, 2 SB, ... of a batch whose largest matrix has nmax rows ----
struct DensePanel {
    int npmax;       // order of the trailing matrix A22(k0) of the largest matrix; the panel exists iff npmax >= 2
    int npn;         // order of A22' = A22(k0 + SB)
    bool exists;     // the loop over k0 runs while this holds
    bool has_next;   // a panel k0 + SB exists: its QR and its Z are launched
    bool fused;      // the fused update (with the next panel's product riding on it) is launched
};
constexpr DensePanel dense_panel(int nmax, int k0) {
    return {nmax - k0 - DENSE_PLAN_SB, nmax - k0 - 2 * DENSE_PLAN_SB, nmax - k0 - DENSE_PLAN_SB >= 2,
            nmax - k0 - 2 * DENSE_PLAN_SB >= 2, nmax - k0 - 2 * DENSE_PLAN_SB >= 1};
}

// QR of a panel with at most npmax rows below the band
enum class DenseQr {
    Reg256,      // sbr_qr_reg_kernel: the panel in registers, two rows per thread
    Lds256,      // sbr_qr_kernel<256, true>: the panel in LDS
    Global1024   // sbr_qr_kernel<1024, false>: the panel in place
};
struct DenseQrPlan {
    DenseQr kind;
    int threads;
    std::size_t lds_bytes;   // dynamic LDS of the launch
};
constexpr std::size_t DENSE_QR_LDS_MAX = 96 * 1024;   // what sbr_qr_kernel<256, true> is allowed
constexpr DenseQrPlan dense_qr_plan(int npmax) {
    return npmax <= 512 ? DenseQrPlan{DenseQr::Reg256, 256, 0}
         : (std::size_t)npmax * DENSE_PLAN_SB * sizeof(double) <= DENSE_QR_LDS_MAX
             ? DenseQrPlan{DenseQr::Lds256, 256, (std::size_t)npmax * DENSE_PLAN_SB * sizeof(double)}
             : DenseQrPlan{DenseQr::Global1024, 1024, 0};
}

// Rows per lane of sbr_fused_kernel<true, .>: two rows per lane are ~10 % faster per row slot but pad the strip count to
// 128 rows.  (One row per lane throughout measured slower on the dense reduction.)
constexpr int DENSE_FUSED_ROWS = 64;     // rows of a lane-row (SF_ROWS; asserted in eig2.hip)
constexpr int dense_fused_rows_per_lane(int npn) {
    return (double)dense_div_up(npn, 2 * DENSE_FUSED_ROWS) * (2 * DENSE_FUSED_ROWS) <
                   1.10 * (double)dense_div_up(npn, DENSE_FUSED_ROWS) * DENSE_FUSED_ROWS
               ? 2 : 1;
}
constexpr int dense_fused_tiles(int npn) { return dense_div_up(npn, DENSE_FUSED_ROWS * dense_fused_rows_per_lane(npn)); }
// tiles per matrix of the other stage-1 kernels
constexpr int dense_symm_tiles(int npmax) { return dense_div_up(npmax, 64); }            // sbr_symm_kernel: 64-row blocks
constexpr int dense_z_tiles(int npmax) { return dense_div_up(npmax, 256); }              // sbr_z_kernel (SM_NT rows)
constexpr int dense_panel_update_tiles(int npmax) { return dense_div_up(npmax, 256); }   // sbr_panel_update_kernel

// ---- stage 2, band -> tridiagonal ----
// number of chase steps of sweep s (also what the kernels call)
constexpr int chase_steps(int n, int s) { return (n - 1 - s + DENSE_PLAN_SB - 1) / DENSE_PLAN_SB; }
// reflectors the chase of a matrix of n rows writes
inline std::int64_t chase_reflector_count(int n) {
    std::int64_t r = 0;
    for (int s = 0; s + 3 <= n; ++s) r += chase_steps(n, s);
    return r;
}
// doubles of the per-(64-row block) partial products V^T X of a matrix
constexpr std::int64_t dense_g_block(int n) { return (std::int64_t)((n + 63) / 64) * DENSE_PLAN_SB * DENSE_PLAN_SB; }

// A whole wavefront per chase step and 16 sweeps in flight per workgroup.  Measured at 128^3 (n = 405, 8 192 matrices):
// 64 lanes per step 42.9 ms, 32 lanes 70.2 ms, 16 lanes 96 ms, and 32 slots instead of 16 do not help the 2 600-row
// level-1 matrices either (80 vs 60 ms): a step is a chain of ~180 dependent operations (LDS round trips, 64-bit DPP
// sums, the reflector's rsq / rcp), and spreading a step over more lanes shortens that chain -- fewer lanes per step
// save instructions but the kernel is bound by the chain, not by issue slots.
constexpr int DENSE_CHASE_THREADS = 1024, DENSE_CHASE_SLOTS = 16;
constexpr int DENSE_CHASE_HAND = 4 * DENSE_PLAN_SB + 2;   // doubles of a slot's LDS scratch (HAND; asserted in eig2.hip)
struct DenseChasePlan {
    bool band_in_lds;        // band_chase_kernel<true>; false: the band and its bulge in EigBatch::bandg
    std::size_t lds_bytes;   // dynamic LDS of the launch
};
constexpr DenseChasePlan dense_chase_plan(int nmax) {
    // the slots' scratch and the cum / start tables, then the band (distances 0 .. 2 SB - 1) when all of it fits
    const std::size_t fixed = sizeof(double) * (DENSE_CHASE_SLOTS * DENSE_CHASE_HAND) + sizeof(int) * (2 * (std::size_t)nmax + 4);
    const std::size_t band = sizeof(double) * (std::size_t)nmax * 2 * DENSE_PLAN_SB;
    return fixed + band + 64 <= DENSE_LDS_MAX ? DenseChasePlan{true, fixed + band + 64} : DenseChasePlan{false, fixed + 64};
}

// ---- back-transformation of the two-stage path ----
struct DenseBackPlan {
    int threads;             // backtransform2_kernel<threads>
    std::size_t lds_bytes;   // above DENSE_LDS_MAX the driver refuses the batch
};
constexpr DenseBackPlan dense_back_plan(int nmax) {
    return {nmax > 1024 ? 1024 : 256,
            sizeof(double) * ((std::size_t)nmax + 2 * DENSE_PLAN_SB) + sizeof(int) * ((std::size_t)nmax + 4) + 64};
}

// ---- one-stage kernel, Sturm counts, inverse iteration (eig.hip) ----
// tridiag_kernel; above DENSE_LDS_MAX the driver refuses the batch
constexpr std::size_t dense_tri_lds_bytes(int nmax) {
    return sizeof(double) * (2 * (std::size_t)nmax + DENSE_PLAN_TRI_NT + 2 * DENSE_PLAN_NB + DENSE_PLAN_TRI_NT / 64);
}
// count_kernel; above DENSE_LDS_MAX the driver refuses the batch
constexpr std::size_t dense_sturm_lds_bytes(int nmax) { return sizeof(double) * 2 * (std::size_t)nmax; }
// eigvec_kernel: its work arrays (~59 nmax bytes) in LDS, or, where they do not fit, in a global workspace
struct DenseVecPlan {
    bool global_ws;          // eigvec_kernel<true>
    std::size_t lds_bytes;   // dynamic LDS of the launch
    std::size_t ws_doubles;  // doubles of workspace per matrix (0: none)
};
constexpr std::size_t dense_vec_work_bytes(int nmax) {
    return sizeof(double) * (7 * (std::size_t)nmax + 8) + sizeof(int) * 8 +
           sizeof(unsigned short) * ((std::size_t)nmax + 3 * (DENSE_PLAN_VEC_MAXB + 2)) + (std::size_t)nmax + 64;
}
constexpr int DENSE_VEC_GLOBAL_MAX_N = 65536;    // (exclusive) the 16-bit block tables of the inverse iteration
constexpr DenseVecPlan dense_vec_plan(int nmax) {
    return dense_vec_work_bytes(nmax) > DENSE_LDS_MAX ? DenseVecPlan{true, 64, dense_vec_work_bytes(nmax) / 8 + 2}
                                                      : DenseVecPlan{false, dense_vec_work_bytes(nmax), 0};
}

// ---- chunk sizing: bytes of device workspace one matrix of n rows needs ----
constexpr std::size_t dense_workspace_bytes(int n) {
    // (sub: the packed sub-panels of the blocked wide-band factorisation, only for matrices that can have a band beyond the
    // LDS window)
    return 8 * ((std::size_t)n * n + (std::size_t)n * (DENSE_PLAN_NB + 8) + (std::size_t)n * n / 2 +
                (std::size_t)n * (3 * DENSE_PLAN_SB + 2 * DENSE_PLAN_SB + ((std::size_t)n > 512 ? 16 * DENSE_PLAN_SB : 0)) + 64);
}

}  // namespace saamge_amd
