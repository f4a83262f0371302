// The kernel plan of the dense eigensolver (saamge_amd/csrc/eig_dense_plan.h) against the values its thresholds had as
// conditions inside the drivers of eig.hip and eig2.hip.  Every expected value below is written out (they come from those
// conditions, evaluated on their own): none is computed by the header under test.
#include "eig_dense_plan.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace saamge_amd;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void panel(int nmax, int k0, int npmax, int npn, bool exists, bool has_next, bool fused, int line) {
    const DensePanel p = dense_panel(nmax, k0);
    if (!(p.npmax == npmax && p.npn == npn && p.exists == exists && p.has_next == has_next && p.fused == fused)) {
        std::printf("FAILED line %d: dense_panel(%d, %d) = npmax %d, npn %d, exists %d, has_next %d, fused %d\n", line, nmax, k0, p.npmax,
                    p.npn, p.exists, p.has_next, p.fused);
        ++failures;
    }
}
#define PANEL(...) panel(__VA_ARGS__, __LINE__)

static int panels(int nmax) {     // the loop of the driver
    int count = 0;
    for (int k0 = 0; dense_panel(nmax, k0).exists; k0 += 16) ++count;
    return count;
}

static void qr(int npmax, DenseQr kind, int threads, long lds, int line) {
    const DenseQrPlan q = dense_qr_plan(npmax);
    if (!(q.kind == kind && q.threads == threads && (long)q.lds_bytes == lds)) {
        std::printf("FAILED line %d: dense_qr_plan(%d) = kind %d, threads %d, lds %zu\n", line, npmax, (int)q.kind, q.threads, q.lds_bytes);
        ++failures;
    }
}
#define QR(...) qr(__VA_ARGS__, __LINE__)

static void fused(int npn, int rows, int tiles, int line) {
    if (!(dense_fused_rows_per_lane(npn) == rows && dense_fused_tiles(npn) == tiles)) {
        std::printf("FAILED line %d: npn %d: rows per lane %d, tiles %d\n", line, npn, dense_fused_rows_per_lane(npn), dense_fused_tiles(npn));
        ++failures;
    }
}
#define FUSED(...) fused(__VA_ARGS__, __LINE__)

static void chase(int nmax, bool in_lds, long lds, int line) {
    const DenseChasePlan c = dense_chase_plan(nmax);
    if (!(c.band_in_lds == in_lds && (long)c.lds_bytes == lds)) {
        std::printf("FAILED line %d: dense_chase_plan(%d) = in LDS %d, lds %zu\n", line, nmax, c.band_in_lds, c.lds_bytes);
        ++failures;
    }
}
#define CHASE(...) chase(__VA_ARGS__, __LINE__)

static void vec(int nmax, bool global_ws, long lds, long ws_doubles, int line) {
    const DenseVecPlan v = dense_vec_plan(nmax);
    if (!(v.global_ws == global_ws && (long)v.lds_bytes == lds && (long)v.ws_doubles == ws_doubles)) {
        std::printf("FAILED line %d: dense_vec_plan(%d) = global %d, lds %zu, workspace %zu\n", line, nmax, v.global_ws, v.lds_bytes,
                    v.ws_doubles);
        ++failures;
    }
}
#define VEC(...) vec(__VA_ARGS__, __LINE__)

int main() {
    // ---- panels of stage 1: k0 = 0, 16, ... while nmax - k0 - 16 >= 2 ----
    CHECK(panels(1) == 0);
    CHECK(panels(2) == 0);
    CHECK(panels(17) == 0);
    CHECK(panels(18) == 1);
    CHECK(panels(19) == 1);
    CHECK(panels(33) == 1);
    CHECK(panels(34) == 2);
    CHECK(panels(50) == 3);
    CHECK(panels(405) == 25);
    PANEL(17, 0, 1, -15, false, false, false);
    PANEL(18, 0, 2, -14, true, false, false);
    PANEL(19, 0, 3, -13, true, false, false);
    PANEL(32, 0, 16, 0, true, false, false);      // npn = 0: nothing left to update
    PANEL(33, 0, 17, 1, true, false, true);       // npn = 1: the fused update runs, no next panel
    PANEL(34, 0, 18, 2, true, true, true);        // npn = 2: a next panel
    PANEL(34, 16, 2, -14, true, false, false);
    PANEL(34, 32, -14, -30, false, false, false);
    PANEL(405, 0, 389, 373, true, true, true);
    PANEL(405, 384, 5, -11, true, false, false);
    PANEL(405, 400, -11, -27, false, false, false);

    // ---- QR of a panel ----
    QR(2, DenseQr::Reg256, 256, 0);
    QR(389, DenseQr::Reg256, 256, 0);
    QR(512, DenseQr::Reg256, 256, 0);
    QR(513, DenseQr::Lds256, 256, 65664);
    QR(713, DenseQr::Lds256, 256, 91264);
    QR(768, DenseQr::Lds256, 256, 98304);         // 96 KiB exactly
    QR(769, DenseQr::Global1024, 1024, 0);
    QR(2171, DenseQr::Global1024, 1024, 0);
    CHECK(DENSE_QR_LDS_MAX == 98304);

    // ---- rows per lane and tiles of the fused update: two rows iff ceil(npn / 128) 128 < 1.10 ceil(npn / 64) 64 ----
    FUSED(-14, 1, 0);
    FUSED(0, 1, 0);
    FUSED(1, 1, 1);
    FUSED(2, 1, 1);
    FUSED(64, 1, 1);
    FUSED(65, 2, 1);
    FUSED(128, 2, 1);
    FUSED(129, 1, 3);
    FUSED(192, 1, 3);
    FUSED(193, 2, 2);
    FUSED(256, 2, 2);
    FUSED(257, 1, 5);
    FUSED(320, 1, 5);
    FUSED(321, 2, 3);
    FUSED(373, 2, 3);
    FUSED(384, 2, 3);
    FUSED(385, 1, 7);
    FUSED(448, 1, 7);
    FUSED(449, 2, 4);
    FUSED(512, 2, 4);
    FUSED(513, 1, 9);
    FUSED(576, 1, 9);
    FUSED(577, 2, 5);                              // from here on the padding stays below 10 %
    FUSED(697, 2, 6);
    FUSED(2155, 2, 17);

    // ---- grids of the other stage-1 kernels ----
    CHECK(dense_cnt8(1) == 8);
    CHECK(dense_cnt8(8) == 8);
    CHECK(dense_cnt8(9) == 16);
    CHECK(dense_cnt8(512) == 512);
    CHECK(dense_symm_tiles(2) == 1 && dense_z_tiles(2) == 1 && dense_panel_update_tiles(2) == 1);
    CHECK(dense_symm_tiles(64) == 1 && dense_symm_tiles(65) == 2);
    CHECK(dense_z_tiles(256) == 1 && dense_z_tiles(257) == 2);
    CHECK(dense_panel_update_tiles(256) == 1 && dense_panel_update_tiles(257) == 2);
    CHECK(dense_symm_tiles(389) == 7 && dense_z_tiles(389) == 2 && dense_panel_update_tiles(389) == 2);
    CHECK(dense_symm_tiles(2171) == 34 && dense_z_tiles(2171) == 9 && dense_panel_update_tiles(2171) == 9);

    // ---- chase: 1 024 threads, 16 slots; the band in LDS up to 588 rows ----
    CHECK(DENSE_CHASE_THREADS == 1024 && DENSE_CHASE_SLOTS == 16 && DENSE_CHASE_HAND == 66);
    CHASE(1, true, 8792);
    CHASE(405, true, 115448);
    CHASE(588, true, 163760);
    CHASE(589, false, 13240);
    CHASE(729, false, 14360);
    CHASE(2187, false, 26024);
    CHECK(DENSE_LDS_MAX == 163840);

    // ---- reflector and G offsets ----
    for (int n : {1, 2, 3, 18, 405}) {
        long sum = 0;
        for (int s = 0; s <= n - 3; ++s) sum += (n - 1 - s + 15) / 16;
        CHECK(chase_reflector_count(n) == sum);
    }
    CHECK(chase_reflector_count(1) == 0);
    CHECK(chase_reflector_count(2) == 0);
    CHECK(chase_reflector_count(3) == 1);
    CHECK(chase_reflector_count(18) == 17);
    CHECK(chase_reflector_count(405) == 5303);
    CHECK(chase_steps(405, 0) == 26 && chase_steps(405, 402) == 1);
    CHECK(dense_g_block(1) == 256);
    CHECK(dense_g_block(64) == 256);
    CHECK(dense_g_block(65) == 512);
    CHECK(dense_g_block(405) == 1792);
    CHECK(dense_g_block(2187) == 8960);

    // ---- back-transformation ----
    { const DenseBackPlan p = dense_back_plan(405); CHECK(p.threads == 256 && p.lds_bytes == 5196); }
    { const DenseBackPlan p = dense_back_plan(1024); CHECK(p.threads == 256 && p.lds_bytes == 12624); }
    { const DenseBackPlan p = dense_back_plan(1025); CHECK(p.threads == 1024 && p.lds_bytes == 12636); }
    { const DenseBackPlan p = dense_back_plan(2187); CHECK(p.threads == 1024 && p.lds_bytes == 26580); }
    CHECK(dense_back_plan(13625).lds_bytes == 163836);        // the last one the driver takes
    CHECK(dense_back_plan(13626).lds_bytes == 163848);        // refused

    // ---- one-stage kernel and Sturm counts: refused above 160 KiB ----
    CHECK(dense_tri_lds_bytes(405) == 15312);
    CHECK(dense_tri_lds_bytes(9688) == 163840);
    CHECK(dense_tri_lds_bytes(9689) == 163856);
    CHECK(dense_sturm_lds_bytes(405) == 6480);
    CHECK(dense_sturm_lds_bytes(10240) == 163840);
    CHECK(dense_sturm_lds_bytes(10241) == 163856);

    // ---- eigenvectors: the global workspace from 2 749 rows on ----
    VEC(405, false, 25591, 0);
    VEC(2187, false, 130729, 0);
    VEC(2748, false, 163828, 0);
    VEC(2749, true, 64, 20487);
    VEC(65535, true, 64, 483534);
    CHECK(DENSE_VEC_GLOBAL_MAX_N == 65536);

    // ---- chunk sizing ----
    CHECK(dense_workspace_bytes(1) == 1480);
    CHECK(dense_workspace_bytes(405) == 2357608);
    CHECK(dense_workspace_bytes(512) == 3637760);
    CHECK(dense_workspace_bytes(513) == 4701640);
    CHECK(dense_workspace_bytes(2187) == 63974632);

    if (failures) { std::printf("eig_dense plan test: %d failures\n", failures); return 1; }
    std::printf("eig_dense plan test ok\n");
    return 0;
}
