// TEST: the `ae_order` field of saamge_amd_options and saamge_amd::api::ae_order / level_order_info.
// Without an argument only the checks that need no GPU run; with "gpu" a 12 x 12 sheet of quads whose vertices carry scrambled
// numbers, split into two agglomerates, is ordered with mode 1 and mode 0 and printed.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

int main(int argc, char **argv) {
    saamge_amd_options o;
    saamge_amd_options_default(&o);
    if (o.ae_order != 0) return 1;
    // the new field is the last one, behind host_heap_pad_mb
    if ((char *)&o.ae_order - (char *)&o.host_heap_pad_mb != (long)sizeof(int) ||
        (char *)&o.ae_order - (char *)&o + sizeof(int) != sizeof(saamge_amd_options)) return 2;
    saamge_amd_params p;
    saamge_amd_params_default(&p);
    if (p.options.ae_order != 0) return 3;
    const int e2d1[4] = {0, 1, 2, 3}, part1[1] = {0};
    const int bad[2] = {2, -1};
    for (int b = 0; b < 2; ++b) {
        int ae_ptr[2] = {-7, -7};
        long long nconn = -7;
        if (!saamge_amd_ae_order(4, 1, 4, nullptr, e2d1, part1, 1, bad[b], ae_ptr, &nconn, nullptr, nullptr, nullptr, nullptr, nullptr)) return 4;
        if (!std::strstr(saamge_amd_last_error(), "ae_order") || ae_ptr[0] != -7 || nconn != -7) return 5;
        bool threw = false;
        try { (void)ae_order(4, 1, 4, nullptr, e2d1, part1, 1, bad[b]); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "ae_order") != nullptr; }
        if (!threw) return 6;
    }
    {
        bool threw = false;
        try { (void)level_order_info(nullptr, 0); } catch (const std::runtime_error &) { threw = true; }
        if (!threw) return 7;
    }
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int nx = 12, ny = 12, vx = nx + 1, nv = vx * (ny + 1);
        std::vector<int> num((size_t)nv), e2d, part;
        for (int v = 0; v < nv; ++v) num[(size_t)v] = (int)(((long long)v * 59) % nv);      // 59 and 169 are coprime
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int c[4] = {y * vx + x, y * vx + x + 1, (y + 1) * vx + x + 1, (y + 1) * vx + x};
                for (int k = 0; k < 4; ++k) e2d.push_back(num[(size_t)c[k]]);
                part.push_back(y < 8 ? 0 : 1);
            }
        for (int mode = 1; mode >= 0; --mode) {
            const AeOrder r = ae_order(nv, nx * ny, 4, nullptr, e2d.data(), part.data(), 2, mode);
            if (r.ae_ptr.size() != 3 || r.pos.size() != (size_t)r.ae_ptr[2] || r.ae_to_dof.size() != r.pos.size()) return 8;
            for (int a = 0; a < 2; ++a) {
                std::printf("mode %d ae %d bw0 %d bw %d choice %d pos", mode, a, r.bw0[(size_t)a], r.bw[(size_t)a], r.choice[(size_t)a]);
                for (int k = r.ae_ptr[(size_t)a]; k < r.ae_ptr[(size_t)a + 1]; ++k) std::printf(" %d:%d", r.ae_to_dof[(size_t)k], r.pos[(size_t)k]);
                std::printf("\n");
            }
        }
    }
    std::printf("ae order api test ok\n");
    return 0;
}
