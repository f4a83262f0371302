// TEST: the boundary refinement through saamge_amd::api::partition_refine / partition_mesh_refined.  Without an argument only
// the checks that need no GPU run (the refusals that come before the graph is looked at); with "gpu" a 6 x 6 x 4 grid of Q1
// hexes is partitioned with refinement (elems_per_agg 8 and 4, 8 rounds each) and printed with the counts of the last level,
// and a partition of one level is refined in place.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

int main(int argc, char **argv) {
    long long xadj2[3] = {0, 1, 2};
    const int adj2[2] = {1, 0};
    std::vector<int> part(2, 0);
    part[1] = 1;
    struct { int rounds, max_size, min_size; const char *word; } bad[3] = {{-1, 0, 0, "rounds"}, {1, -1, 0, "max_size"}, {1, 0, -1, "min_size"}};
    for (int b = 0; b < 3; ++b) {
        bool threw = false;
        try { (void)partition_refine(2, xadj2, adj2, 2, part, bad[b].rounds, bad[b].max_size, bad[b].min_size); }
        catch (const std::runtime_error &e) { threw = std::strstr(e.what(), bad[b].word) != nullptr; }
        if (!threw || part[0] != 0 || part[1] != 1) return 1;
    }
    long long info[4] = {-7, -7, -7, -7};
    if (!saamge_amd_partition_refine(2, xadj2, adj2, 2, part.data(), 1, 0, 0, 0u, 2, nullptr, info)) return 2;
    if (!std::strstr(saamge_amd_last_error(), "renumber") || info[0] != -7 || part[1] != 1) return 2;
    {
        std::vector<int> wrong(3, 0);
        bool threw = false;
        try { (void)partition_refine(2, xadj2, adj2, 2, wrong, 1); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) return 3;
        const int e2d[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        threw = false;
        try { (void)partition_mesh_refined(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), std::vector<int>(2, 1)); }
        catch (const std::invalid_argument &) { threw = true; }
        if (!threw) return 3;
        threw = false;
        try { (void)partition_mesh_refined(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), std::vector<int>(1, -1)); }
        catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "refine_rounds") != nullptr; }
        if (!threw) return 4;
    }
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        // calls written before this change, a literal null for the options included
        {
            const int e2d[8] = {0, 1, 2, 3, 4, 5, 6, 7};
            long long xadj[2] = {0, 0};
            std::vector<int> p1;
            void *stream = nullptr;
            if (partition_graph(1, xadj, nullptr, 4, p1, nullptr, stream) != 1 || p1[0] != 0) return 5;
            if (partition_graph_v2(1, xadj, nullptr, 4, p1, NULL, stream) != 1) return 5;
            if (partition_mesh_v2(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), nullptr, stream).nparts[0] != 1) return 5;
            if (partition_mesh_refined(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), std::vector<int>()).nparts[0] != 1) return 5;
        }
        const int nx = 6, ny = 6, nz = 4, vx = nx + 1, vy = ny + 1;
        std::vector<int> e2d;
        for (int z3 = 0; z3 < nz; ++z3)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x)
                    for (int c = 0; c < 8; ++c) e2d.push_back(((z3 + (c >> 2)) * vy + y + ((c >> 1) & 1)) * vx + x + (c & 1));
        std::vector<int> epa, rounds(2, 8);
        epa.push_back(8);
        epa.push_back(4);
        const MeshPartitions P = partition_mesh_refined(nx * ny * nz, 8, nullptr, e2d.data(), vx * vy * (nz + 1), epa, rounds);
        if (P.partitions.size() != 2 || (int)P.partitions[1].size() != P.nparts[0]) return 6;
        for (int k = 0; k < 2; ++k) {
            std::printf("level %d nparts %d part", k, P.nparts[(size_t)k]);
            for (size_t e = 0; e < P.partitions[(size_t)k].size(); ++e) std::printf(" %d", P.partitions[(size_t)k][e]);
            std::printf("\n");
        }
        saamge_amd_partition_refine_info(info);
        std::printf("refine info %lld %lld %lld %lld\n", info[0], info[1], info[2], info[3]);
        // two nodes, two parts: nothing can move, and the pass says so
        const RefineInfo r = partition_refine(2, xadj2, adj2, 2, part, 4, 0, 0, 0u, true);
        if (r.rounds != 0 || r.moved != 0 || r.gain != 0 || r.converged != 1 || part[0] != 0 || part[1] != 1) return 7;
    }
    std::printf("partition refine api test ok\n");
    return 0;
}
