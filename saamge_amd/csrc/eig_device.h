// Device helpers that the dense path (eig.hip) and the two-stage / few-eigenpairs file (eig2.hip) both use: one text each.
// Only helpers whose text was the same in both files live here.  Reductions that add in another order stay where they
// are (wave_sum, wsum64, gsum16 / rsum16): merging those would move results by a bit.
#pragma once

#include <hip/hip_runtime.h>

namespace saamge_amd {

// Sum over a workgroup of NT threads (shuffle-down inside each wavefront, then the NT / 64 partials in order).  red: NT / 64
// doubles of LDS.  Every thread gets the sum.
template <int NT>
__device__ inline double block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) r += red[i];
    return r;
}

__device__ inline double unit_rand(unsigned a, unsigned b) {  // deterministic uniform(-1,1)
    unsigned h = a * 2654435761u ^ (b + 0x9e3779b9u + (a << 6) + (a >> 2));
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return ((double)h + 0.5) * (2.0 / 4294967296.0) - 1.0;
}

}  // namespace saamge_amd
