// TEST: a driver that installs the device partitioner with spaced seeds in the MFEM adaptor, compiled (not linked) against
// tests/mfem_stub.  The hook keeps the whole options struct, the new last field included.
#include "saamge_amd.hpp"

using namespace mfem;
using namespace saamge;

int mock_partition_seeding_driver(Table *elem_to_elem, int *nparts_arr, int *partitioning) {
    saamge_amd_partition_options o;
    saamge_amd_partition_options_default(&o);
    o.seeding = 1;
    const ml_device_partitioner_t hook = ml_device_partitioner(&o);
    if (hook.options.seeding != 1 || ml_device_partitioner().options.seeding != 0) return 1;
    ml_set_fine_partitioner(hook);
    ml_fine_partitioner()(0, elem_to_elem->Size(), nparts_arr[0], *elem_to_elem, partitioning);
    return 0;
}
