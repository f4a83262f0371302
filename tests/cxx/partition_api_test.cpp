// TEST: saamge_amd::api::partition_graph / partition_mesh through libsaamge_amd.so.  Without an argument only the checks
// that need no GPU run; with "gpu" a 4 x 4 x 4 grid of Q1 hexes is partitioned and printed (elems_per_agg 8 and 4).
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

int main(int argc, char **argv) {
    std::vector<int> part;
    long long xadj[2] = {0, 0};
    bool threw = false;
    try { (void)partition_graph(1, xadj, nullptr, 0, part); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "elems_per_agg") != nullptr; }
    if (!threw) return 1;
    threw = false;
    try { (void)partition_mesh(1, 8, nullptr, nullptr, 8, std::vector<int>(1, 4)); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "null argument") != nullptr; }
    if (!threw) return 2;
    saamge_amd_partition_options o;
    saamge_amd_partition_options_default(&o);
    if (o.min_shared != 1 || o.max_size != -1 || o.min_size != -1 || o.seed != 0) return 3;
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        const int n = 4, nv = n + 1;
        std::vector<int> e2d;
        for (int z = 0; z < n; ++z)
            for (int y = 0; y < n; ++y)
                for (int x = 0; x < n; ++x)
                    for (int c = 0; c < 8; ++c) e2d.push_back(((z + (c >> 2)) * nv + y + ((c >> 1) & 1)) * nv + x + (c & 1));
        std::vector<int> epa;
        epa.push_back(8);
        epa.push_back(4);
        const MeshPartitions P = partition_mesh(n * n * n, 8, nullptr, e2d.data(), nv * nv * nv, epa);
        if (P.partitions.size() != 2 || P.pointers().size() != 2 || (int)P.partitions[1].size() != P.nparts[0]) return 4;
        for (int k = 0; k < 2; ++k) {
            std::printf("level %d nparts %d part", k, P.nparts[(size_t)k]);
            for (size_t e = 0; e < P.partitions[(size_t)k].size(); ++e) std::printf(" %d", P.partitions[(size_t)k][e]);
            std::printf("\n");
        }
    }
    std::printf("partition api test ok\n");
    return 0;
}
