// TEST: the `growth` field of saamge_amd_partition_options_v2 through saamge_amd::api::partition_graph_v2 / partition_mesh_v2.
// Without an argument only the checks that need no GPU run; with "gpu" a 6 x 6 x 4 grid of Q1 hexes is partitioned with
// balanced growth (growth = 1) and printed (elems_per_agg 8 and 4), then the counts of the last level.
#include <cstdio>
#include <cstring>

#include "saamge_amd.hpp"

using namespace saamge_amd::api;

int main(int argc, char **argv) {
    saamge_amd_partition_options_v2 o;
    saamge_amd_partition_options_v2_default(&o);
    saamge_amd_partition_options o1;
    saamge_amd_partition_options_default(&o1);
    if (o.growth != 0 || o.seeding != 0) return 1;
    saamge_amd_partition_options_v2 z;
    std::memset(&z, 0, sizeof z);       // a zero-filled struct asks for today's growth
    if (z.growth != o.growth) return 2;
    // the new field is the last one, behind `seeding`; the fields before it lie and default as in saamge_amd_partition_options
    if ((char *)&o.growth - (char *)&o.seeding != (long)sizeof(int) ||
        (char *)&o.growth - (char *)&o + sizeof(int) != sizeof(saamge_amd_partition_options_v2)) return 3;
    if ((char *)&o.growth - (char *)&o != (long)sizeof(saamge_amd_partition_options) || std::memcmp(&o, &o1, sizeof o1)) return 3;
    const int bad[2] = {2, -1};
    for (int b = 0; b < 2; ++b) {
        o.growth = bad[b];
        std::vector<int> part(1, -7);
        long long xadj[2] = {0, 0};
        int nparts = -7;
        if (!saamge_amd_partition_graph_v2(1, xadj, nullptr, 4, &o, nullptr, part.data(), &nparts)) return 4;
        if (!std::strstr(saamge_amd_last_error(), "growth") || part[0] != -7 || nparts != -7) return 5;
        const int e2d[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        bool threw = false;
        try { (void)partition_mesh_v2(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), &o); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "growth") != nullptr; }
        if (!threw) return 6;
        threw = false;
        try { (void)partition_graph_v2(1, xadj, nullptr, 4, part, &o); } catch (const std::runtime_error &e) { threw = std::strstr(e.what(), "growth") != nullptr; }
        if (!threw) return 7;
    }
    if (argc > 1 && !std::strcmp(argv[1], "gpu")) {
        // a literal null for the options with a stream behind it, as a call written before the field existed: the defaults
        {
            const int e2d[8] = {0, 1, 2, 3, 4, 5, 6, 7};
            long long xadj[2] = {0, 0};
            std::vector<int> part;
            void *stream = nullptr;
            if (partition_graph(1, xadj, nullptr, 4, part, nullptr, stream) != 1 || part[0] != 0) return 13;
            if (partition_graph(1, xadj, nullptr, 4, part, NULL, stream) != 1) return 13;
            if (partition_graph_v2(1, xadj, nullptr, 4, part, nullptr, stream) != 1) return 13;
            if (partition_mesh(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), nullptr, stream).nparts[0] != 1) return 14;
            if (partition_mesh_v2(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), nullptr, stream).nparts[0] != 1) return 14;
        }
        const int nx = 6, ny = 6, nz = 4, vx = nx + 1, vy = ny + 1;
        std::vector<int> e2d;
        for (int z3 = 0; z3 < nz; ++z3)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x)
                    for (int c = 0; c < 8; ++c) e2d.push_back(((z3 + (c >> 2)) * vy + y + ((c >> 1) & 1)) * vx + x + (c & 1));
        std::vector<int> epa;
        epa.push_back(8);
        epa.push_back(4);
        o.growth = 1;
        const MeshPartitions P = partition_mesh_v2(nx * ny * nz, 8, nullptr, e2d.data(), vx * vy * (nz + 1), epa, &o);
        if (P.partitions.size() != 2 || (int)P.partitions[1].size() != P.nparts[0]) return 8;
        for (int k = 0; k < 2; ++k) {
            std::printf("level %d nparts %d part", k, P.nparts[(size_t)k]);
            for (size_t e = 0; e < P.partitions[(size_t)k].size(); ++e) std::printf(" %d", P.partitions[(size_t)k][e]);
            std::printf("\n");
        }
        long long info[4] = {-1, -1, -1, -1};
        saamge_amd_partition_growth_info(info);
        std::printf("growth info %lld %lld %lld %lld\n", info[0], info[1], info[2], info[3]);
        // one level through partition_graph on a graph without edges: every node alone, nothing for a quota to label
        std::vector<int> part;
        std::vector<long long> xadj((size_t)P.nparts[1] + 1, 0);
        if (partition_graph_v2(P.nparts[1], xadj.data(), nullptr, 8, part, &o) != P.nparts[1]) return 9;
        saamge_amd_partition_growth_info(info);
        if (info[0] != 0 || info[1] != 0) return 10;
        o.growth = 0;
        if (partition_graph_v2(P.nparts[1], xadj.data(), nullptr, 8, part, &o) != P.nparts[1]) return 11;
        saamge_amd_partition_growth_info(info);
        if (info[0] || info[1] || info[2] || info[3]) return 12;
    }
    std::printf("partition growth api test ok\n");
    return 0;
}
