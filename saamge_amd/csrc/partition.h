// Agglomerate partitions built on the device from a graph (partition.hip).  The algorithm is defined by
// saamge_amd/partition_model.py; the kernels restate it and give the same integers.
#pragma once
#include "common.h"

namespace saamge_amd {

struct PartitionOptions {
    int min_shared = 1;   // dofs two elements share to be adjacent (mesh entry only)
    int lloyd_iters = 0;  // recentring passes
    int max_size = -1;    // -1: 2 * elems_per_agg, 0: off
    int min_size = -1;    // -1: elems_per_agg / 4, 0: off
    unsigned seed = 0;
    int seeding = 0;      // 0: lowest priorities, 1: spaced (greedy distance-r independent set, topped up)
    int growth = 0;       // 0: level-synchronous, 1: balanced (a per-round quota per part, then release)
};
// the spaced seeding of a partition_graph_device; zeros after seeding = 0
struct SeedingStats {
    int radius = 0, rounds = 0, seeds_first = 0, seeds = 0;
};
// the balanced growth of a partition_graph_device (its last growth, with recentring); zeros after growth = 0.  rounds: those
// that labelled nodes; open_parts / released_nodes: at the release, 0 when there was none
struct GrowthStats {
    int rounds = 0, quota_nodes = 0, open_parts = 0, released_nodes = 0;
};
struct PartitionStats {
    SeedingStats seeding;
    GrowthStats growth;
};
// a refine_partition_device: rounds that moved nodes, nodes moved, the sum of their gains (= cut edges removed), and whether
// it stopped for want of a candidate
struct RefineStats {
    long long rounds = 0, moved = 0, gain = 0;
    int converged = 0;
};

// Refuses offsets that are not 0-based and ascending, columns outside [0, n) and entries without their transpose.  Reads
// adj only after xadj has been checked.  Returns xadj[n].
int64_t check_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj);
// part (device, n entries) and the number of parts produced; the graph is trusted (check_graph_device).  *stats is zeroed
// once the arguments are accepted, before any work, and filled as the seeding and each growth end.
void partition_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, int elems_per_agg,
                            const PartitionOptions &o, int *part, int *nparts_out, PartitionStats *stats);
// the caps partition_graph_device works with
void resolve_partition_sizes(int elems_per_agg, const PartitionOptions &o, int *max_size, int *min_size);
// refuses a label outside [0, nparts) and an empty part (label on the device)
void check_partition_device(hipStream_t s, int n, const int *label, int nparts);
// The boundary refinement pass (partition_model.py, "refine") on a checked partition, labels in place on the device.
// max_size 0: no cap.  The graph is trusted (check_graph_device).
RefineStats refine_partition_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, int nparts, int *label, int rounds,
                                    int max_size, int min_size, unsigned seed);
// part (another array than label) = the parts numbered by their smallest member
void renumber_device(hipStream_t s, int n, const int *label, int nlabels, int *part, int *nparts_out);
// e2d_I / e2d_J on the device and already checked
void element_graph_device(hipStream_t s, int NE, const int *e2d_I, const int *e2d_J, int ND, int min_shared,
                          DBuf<roff_t> &xadj, DBuf<int> &adj);
void quotient_graph_device(hipStream_t s, int n, const roff_t *xadj, const int *adj, const int *part, int nparts,
                           DBuf<roff_t> &xq, DBuf<int> &aq);
// bounded checks of a mesh given as offsets and flat dofs, both on the device; returns elem_ptr[NE]
long check_mesh_device(hipStream_t s, int NE, const int *e2d_I, const int *e2d_J, int ND);

}  // namespace saamge_amd
