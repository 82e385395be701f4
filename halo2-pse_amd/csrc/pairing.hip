// pairing.hip -- the entry points of include/halo2hip_pairing.h over csrc/pairing_host.h.  Host code on the calling thread: no Entry,
// no engine lock, no HIP call; a rejected call writes nothing.
#include "../../include/halo2hip_pairing.h"
#include "engine.h"
#include "pairing_host.h"

using namespace h2;

extern "C" {

int h2hip_pairing_check_bn254(const uint64_t* g1_xy, const uint64_t* g2_raw, size_t n, int* ok) {
    char why[160];
    if (!ok) {
        set_error("pairing_check: null ok");
        return H2HIP_EINVAL;
    }
    pairing::F12 f;
    if (pairing::pairing_product(g1_xy, g2_raw, n, &f, why, sizeof(why))) {
        set_error("pairing_check: %s", why);
        return H2HIP_EINVAL;
    }
    *ok = pairing::f12_is_one(f) ? 1 : 0;
    return 0;
}

int h2hip_pairing_bn254(const uint64_t* g1_xy, const uint64_t* g2_raw, size_t n, uint64_t out_gt[48]) {
    char why[160];
    if (!out_gt) {
        set_error("pairing: null out_gt");
        return H2HIP_EINVAL;
    }
    pairing::F12 f;
    if (pairing::pairing_product(g1_xy, g2_raw, n, &f, why, sizeof(why))) {
        set_error("pairing: %s", why);
        return H2HIP_EINVAL;
    }
    pairing::gt_store(f, out_gt);
    return 0;
}

int h2hip_g2_mul_bn254(const uint64_t g2_raw[16], const uint64_t scalar[4], uint64_t out_raw[16]) {
    char why[160];
    if (pairing::g2_scalar_mul(g2_raw, scalar, out_raw, why, sizeof(why))) {
        set_error("g2_mul: %s", why);
        return H2HIP_EINVAL;
    }
    return 0;
}

int h2hip_g2_check_bn254(const uint64_t g2_raw[16], int* on_curve, int* in_subgroup) {
    char why[160];
    if (pairing::g2_check(g2_raw, on_curve, in_subgroup, why, sizeof(why))) {
        set_error("g2_check: %s", why);
        return H2HIP_EINVAL;
    }
    return 0;
}

}  // extern "C"
