// TEST: a driver that installs the device partitioner with boundary refinement in the MFEM adaptor, compiled (not linked)
// against tests/mfem_stub.  `refine_rounds` is a member of the hook beside `growth`, 0 unless it is set; the makers of the hook
// and the calls written before the member existed compile as they did.
#include "saamge_amd.hpp"

using namespace mfem;
using namespace saamge;

int mock_partition_refine_driver(Table *elem_to_elem, int *nparts_arr, int *partitioning) {
    saamge_amd_partition_options_v2 o;
    saamge_amd_partition_options_v2_default(&o);
    o.growth = 1;
    ml_device_partitioner_t hook = ml_device_partitioner_v2(&o);
    if (hook.refine_rounds != 0 || hook.growth != 1) return 1;
    hook.refine_rounds = 32;
    if (ml_device_partitioner(nullptr).refine_rounds != 0 || ml_device_partitioner(NULL).refine_rounds != 0 ||
        ml_device_partitioner().refine_rounds != 0 || ml_device_partitioner_v2().refine_rounds != 0)
        return 2;
    saamge_amd_partition_options o1 = hook.options;      // the members from before
    if (o1.seeding != 0 || hook.growth != 1) return 3;
    ml_set_fine_partitioner(hook);
    ml_set_coarse_partitioner(hook);
    ml_fine_partitioner()(0, elem_to_elem->Size(), nparts_arr[0], *elem_to_elem, partitioning);
    // the api wrappers beside the adaptor
    std::vector<int> part(1, 0);
    long long xadj[2] = {0, 0};
    const saamge_amd::api::RefineInfo r = saamge_amd::api::partition_refine(1, xadj, nullptr, 1, part, 4);
    const int e2d[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const saamge_amd::api::MeshPartitions P =
        saamge_amd::api::partition_mesh_refined(1, 8, nullptr, e2d, 8, std::vector<int>(1, 4), std::vector<int>(1, 2), &o);
    return (int)r.converged + P.nparts[0];
}
