// fe_io.h -- the 32-byte vector load / store of an Fe (two uint4) that the stage kernels use on global memory: product.hip,
// opening.hip, lookup.hip, keygen.hip.  Device code only.  Kept out of field.h and the other headers that are embedded into the
// run-time compiled gates kernel's source (whose hash keys its disk cache), and out of engine.h, which api.hip's plain C++ build reads.
#pragma once
#include "field.h"

namespace h2 {

__device__ __forceinline__ Fe fe_ld(const Fe* p, uint64_t i) {
    const uint4* q = (const uint4*)(p + i);
    uint4 a = q[0], b = q[1];
    Fe o;
    o.l[0] = a.x, o.l[1] = a.y, o.l[2] = a.z, o.l[3] = a.w, o.l[4] = b.x, o.l[5] = b.y, o.l[6] = b.z, o.l[7] = b.w;
    return o;
}
__device__ __forceinline__ void fe_st(Fe* p, uint64_t i, const Fe& v) {
    uint4* q = (uint4*)(p + i);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

}  // namespace h2
