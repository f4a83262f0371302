// TEST: a driver that installs the device partitioner in the MFEM adaptor, compiled (not linked) against tests/mfem_stub.
#include "saamge_amd.hpp"

using namespace mfem;
using namespace saamge;

int mock_partition_driver(HypreParMatrix *Ag, agg_partitioning_relations_t *agg_part_rels, ElementMatrixProvider *emp,
                          Table *elem_to_elem, int *nparts_arr, int *partitioning) {
    saamge_amd_partition_options o;
    saamge_amd_partition_options_default(&o);
    o.lloyd_iters = 1;
    ml_set_fine_partitioner(ml_device_partitioner(&o));       // the adaptor counts the parts of these hooks itself
    ml_set_coarse_partitioner(ml_device_partitioner());
    if (!detail::partitioner_counts()[0] || !detail::partitioner_counts()[1]) return 1;
    ml_fine_partitioner()(0, elem_to_elem->Size(), nparts_arr[0], *elem_to_elem, partitioning);
    MultilevelParameters mlp(2, nparts_arr, 0, 0, 3, 0.003, 0.003, -1, true, false, false);
    ml_data_t *ml_data = ml_produce_data(*Ag, agg_part_rels, emp, mlp);
    // a hook of the caller's own is a plain std::function again: the parameters' numbers hold
    ml_set_coarse_partitioner([](int, int n_elem, int nparts, const Table &, int *out) {
        for (int e = 0; e < n_elem; ++e) out[e] = e % nparts;
    });
    if (detail::partitioner_counts()[1]) return 2;
    ml_free_data(ml_data);
    return 0;
}
