// TEST: a driver that installs the device partitioner with balanced growth in the MFEM adaptor, compiled (not linked)
// against tests/mfem_stub.  The hook keeps the options struct as it was and the new field beside it; a null pointer for the options still
// compiles and means the defaults, in whichever spelling.
#include "saamge_amd.hpp"

using namespace mfem;
using namespace saamge;

int mock_partition_growth_driver(Table *elem_to_elem, int *nparts_arr, int *partitioning) {
    saamge_amd_partition_options_v2 o;
    saamge_amd_partition_options_v2_default(&o);
    o.growth = 1;
    o.seeding = 1;
    const ml_device_partitioner_t hook = ml_device_partitioner_v2(&o);
    if (hook.growth != 1 || hook.options.seeding != 1 || ml_device_partitioner_v2().growth != 0) return 1;
    saamge_amd_partition_options o1;       // the struct without the field: its fields are kept, growth is 0
    saamge_amd_partition_options_default(&o1);
    o1.seeding = 1;
    if (ml_device_partitioner(&o1).growth != 0 || ml_device_partitioner(&o1).options.seeding != 1) return 2;
    // calls written before the field existed: a literal null for the options, and the member handed to the C entry point
    if (ml_device_partitioner(nullptr).growth != 0 || ml_device_partitioner(NULL).growth != 0 || ml_device_partitioner().growth != 0)
        return 3;
    const saamge_amd_partition_options *old_member = &hook.options;
    o1 = hook.options;
    if (old_member->seeding != 1 || o1.seeding != 1) return 4;
    ml_set_fine_partitioner(hook);
    ml_fine_partitioner()(0, elem_to_elem->Size(), nparts_arr[0], *elem_to_elem, partitioning);
    return 0;
}
