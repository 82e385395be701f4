// lk_dev.h -- what the lookup permutation (lookup.hip) and the witness check (check.hip) share on the device: Fr's order on
// canonical keys and the workgroup scan of their count / scan / compact tails.  Device code only; kept out of the headers embedded
// into the run-time compiled gates kernel, as fe_io.h is.
#pragma once
#include "fe_io.h"

namespace h2 {

#define LK_THREADS 256

// a < b as 256-bit integers (limb 7 most significant): Fr's Ord on canonical values
__device__ __forceinline__ bool key_lt(const Fe& a, const Fe& b) {
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
// exclusive sum over the workgroup's threads in order; *total = sum of all
__device__ __forceinline__ uint32_t lk_scan_excl(uint32_t v, uint32_t* lds, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < LK_THREADS; off <<= 1) {
        const uint32_t x = tid >= off ? lds[tid - off] : 0u;
        __syncthreads();
        lds[tid] += x;
        __syncthreads();
    }
    const uint32_t inc = lds[tid];
    *total = lds[LK_THREADS - 1];
    __syncthreads();
    return inc - v;
}

}  // namespace h2
