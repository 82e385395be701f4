// msm_pair.h -- the index and plan arithmetic of the pair MSM of an IPA round (msm.hip, msm_pair_device):
//   L = <p[half .. 2 half), g[0 .. half)>,  R = <p[0 .. half), g[half .. 2 half)>     (ipa/commitment/prover.rs:109-110)
// are ONE MSM over the 2 half points of g whose buckets are kept in two sets: point i takes the scalar p[(i + half) mod 2 half] and
// adds into set (i >= half).  Plain integer code that compiles for the host alone (tests/cpp/test_msm_pair_host.cpp walks it, plain
// and under ASan + UBSan) and for the device.
#ifndef H2_MSM_PAIR_H
#define H2_MSM_PAIR_H
#include <stddef.h>
#include <stdint.h>

#ifndef H2_HD
#if defined(__HIPCC__)
#define H2_HD __host__ __device__ __forceinline__
#else
#define H2_HD inline
#endif
#endif

namespace h2 {

// the point a lane works on: lane t of the tiles of MSM y (blockIdx.y of the digit passes) of a two-set run over `half` pairs each
H2_HD uint32_t msm_pair_point(uint32_t y, uint32_t t, uint32_t half) { return y * half + t; }
// the scalar of point i < 2 half: the index rotated by half
H2_HD uint32_t msm_pair_scalar_index(uint32_t i, uint32_t half) { return i < half ? i + half : i - half; }
// the bucket set of point i: 0 collects L, 1 collects R
H2_HD uint32_t msm_pair_set(uint32_t i, uint32_t half) { return i >= half ? 1u : 0u; }

// Does the two-set run fit one fused run?  W windows of cb-bit bucket ids per set (the fused plan at `half` pairs); the limits are
// those of every fused batch: Tuning::msm_fuse_max_n pairs per MSM, Tuning::msm_fuse_entries entries per run, and the sort's
// max_buckets buckets and max_sets bucket sets (MSM_MAX_C1 << MSM_MAX_L, MSM_MAX_C1).
H2_HD bool msm_pair_fits(size_t half, uint32_t W, uint32_t cb, size_t fuse_entries, size_t fuse_max_n, uint64_t max_buckets, uint32_t max_sets) {
    if (half < 1 || half > fuse_max_n || W < 1) return false;
    if (half > fuse_entries / 2 / W) return false;  // 2 half W entries
    if (2 * W > max_sets) return false;
    if (cb >= 63 || ((uint64_t)(2 * W) << cb) > max_buckets) return false;
    return true;
}

struct MsmPairWindows {
    uint32_t W, cb;
};

// The largest half msm_pair_fits takes (0: none), for a plan that depends on floor(log2 half) only: windows(lg) -> {W, cb}.  Within one
// class 2^lg <= half < 2^(lg + 1) the test is monotone in half, so the classes are walked from the top and the first that admits one
// of its sizes gives the answer.
template <class F>
inline size_t msm_pair_max_half(F&& windows, size_t fuse_entries, size_t fuse_max_n, uint64_t max_buckets, uint32_t max_sets, size_t limit) {
    size_t top = fuse_max_n < limit ? fuse_max_n : limit;
    if (top < 1) return 0;
    uint32_t lg = 0;
    while (lg + 1 < 8 * sizeof(size_t) && ((size_t)1 << (lg + 1)) <= top) lg++;
    for (;; lg--) {
        const size_t lo = (size_t)1 << lg;
        size_t hi = lg + 1 < 8 * sizeof(size_t) ? ((size_t)1 << (lg + 1)) - 1 : top;
        if (hi > top) hi = top;
        const MsmPairWindows w = windows(lg);
        if (w.W >= 1) {
            const size_t by_entries = fuse_entries / 2 / w.W;
            const size_t h = hi < by_entries ? hi : by_entries;
            if (h >= lo && msm_pair_fits(h, w.W, w.cb, fuse_entries, fuse_max_n, max_buckets, max_sets)) return h;
        }
        if (lg == 0) return 0;
    }
}

}  // namespace h2
#endif
