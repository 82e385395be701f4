/*
 * halo2hip_ipa_round.h -- a round of the inner-product argument's opening (ipa/commitment/prover.rs:102-142) as ONE engine call, and
 * its two MSMs as one run of the MSM pipeline.  Part of halo2hip_ipa.h, which includes it and whose preamble holds: layouts, return
 * codes, H2HIP_EINVAL (a null pointer, a size outside the stated range, a scalar that is not reduced, a device pointer that is not
 * 16-byte aligned) with its text before the engine is entered.  The declarations live in a file of their own so that they have binding
 * tables of their own (halo2-pse_amd/_abi_ipa_round.py, halo2hip-sys/src/ffi_ipa_round.rs, generated from this file).
 */
#ifndef HALO2HIP_IPA_ROUND_H
#define HALO2HIP_IPA_ROUND_H

#include "halo2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* L = sum_{i<half} p[half+i] * g[i],  R = sum_{i<half} p[i] * g[half+i]   (ipa/commitment/prover.rs:109-110)
 * out_l, out_r: Jacobian, Montgomery, as h2hip_msm_bn254_device writes them; waits for `stream`. 1 <= half <= 2^26.
 * half need not be a power of two; p holds 2 * half scalars and g 2 * half points, both read only.
 * Up to h2hip_ipa_round_msms_fused_max_half() -- 2^19 with the default settings: at most Tuning::msm_fuse_max_n pairs per sum and
 * 2 * half * windows <= Tuning::msm_fuse_entries entries -- the two sums come from ONE run of the MSM pipeline over the 2 * half points
 * (point i takes the scalar p[(i + half) mod 2 half] and the bucket sets chosen by i >= half): one digit pass, one sort, one
 * accumulation launch, one reduction, one wait.  Above that the library runs the two MSMs pipelined over its internal streams: still
 * one call and one wait. */
int h2hip_ipa_round_msms_bn254_device(const void* d_p, const void* d_g_xy, size_t half, uint64_t out_l[12], uint64_t out_r[12], void* stream);
/* the largest half that takes the single run under the settings in force (0: none does) */
size_t h2hip_ipa_round_msms_fused_max_half(void);

/* One round of commitment::create_proof after the challenge of the round before it (prover.rs:102-142).
 * u != NULL: p, b hold 4*half elements and g 4*half points; first fold p and b by (u_inv, u) and collapse g by u,
 * exactly as h2hip_ipa_fold / h2hip_ipa_collapse at 2*half do.   u == NULL (first round): skip that.
 * Then: out_l / out_r as above at `half`, values[8] as h2hip_ipa_inner_products at `half`.  One wait for `stream`.
 * u and u_inv come together or not at all, both reduced (that they are inverses is the caller's business, as in h2hip_ipa_fold).
 * Everything is queued on `stream`; the only synchronisation is the one that delivers the outputs.  1 <= half <= 2^26.
 * Afterwards p, b and g[0 .. 2*half) hold, limb for limb, what the separate calls leave; g above 2*half is unspecified, as after
 * h2hip_ipa_collapse.  After the last round (half = 1) the caller makes one plain h2hip_ipa_fold at half = 1 to read c = p'[0]; the
 * reference's last collapse (prover.rs:137) yields a g' that nothing reads and may be dropped. */
int h2hip_ipa_round_bn254_device(void* d_p, void* d_b, void* d_g_xy, size_t half, const uint64_t u[4], const uint64_t u_inv[4],
                                 uint64_t out_l[12], uint64_t out_r[12], uint64_t values[8], void* stream);

/* Tuning: the wrappers' openings (ipa.py and host/ipa.hpp create_proof, and whoever else asks) run one h2hip_ipa_round call per round
 * (on != 0, the default) or the separate calls (0).  The entry points above do not read it.  get returns 1 or 0. */
int h2hip_ipa_set_round_call(int on);
int h2hip_ipa_get_round_call(void);

#ifdef __cplusplus
}
#endif
#endif
