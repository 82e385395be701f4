/*
 * halo2hip_ipa.h -- C ABI of libhalo2hip.so for the inner-product-argument commitment scheme (halo2_proofs/src/poly/ipa/) at
 * C = bn256::G1Affine: the per-round kernels of commitment::create_proof (ipa/commitment/prover.rs:29-153) and the vector s of the
 * verifier (ipa/strategy.rs:161-176).  Layouts, return codes and h2hip_last_error() are halo2hip.h's: elements are 4 x uint64_t
 * Montgomery limbs, G1Affine is x || y with the identity (0, 0), every function returns 0 or an H2HIP_E* code, and H2HIP_EINVAL (a null
 * pointer, a size outside the stated range, a scalar that is not reduced, a device pointer that is not 16-byte aligned) is returned
 * with its text before the engine is entered, so it needs no GPU.
 *
 * The engine draws and orders nothing: challenges are the caller's (the transcript's), and so is the order of the rounds.  The L_j / R_j
 * of a round are h2hip_msm_bn254_device on (p + half, g, half) and (p, g + half, half), or both from h2hip_ipa_round_msms / h2hip_ipa_round
 * below; their [value * z] U + [rand] W parts, and every other handful of group operations, stay with the caller.
 *
 * The round calls (powers, inner_products, fold) exist only in _device form: the state of an opening -- p', b and g' -- lives in
 * device memory across its k rounds, and the wrappers own the single upload.  _device forms queue on `stream` and do not synchronise
 * unless stated.
 */
#ifndef HALO2HIP_IPA_H
#define HALO2HIP_IPA_H

#include "halo2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* parallel_generator_collapse (ipa/commitment/prover.rs:155-167): g holds 2 * half affine points; g[i] <- affine(g[i] + [u] g[half + i])
 * for i < half, 1 <= half <= 2^27, half need not be a power of two.  The identity is (0, 0), in and out; g[i] = +-[u] g[half + i] and
 * identities on either side are legal.  u is any reduced scalar (0 leaves g[i]).  After the _device call the upper half is
 * unspecified.  The host form uploads 2 * half points and downloads half. */
int h2hip_ipa_collapse_bn254(uint64_t* g_xy, size_t half, const uint64_t u[4]);
int h2hip_ipa_collapse_bn254_device(void* d_g_xy, size_t half, const uint64_t u[4], void* stream);

/* The vector b of an opening at x (prover.rs:84-91): d_out[i] = x^i, i < n, 1 <= n <= 2^28. */
int h2hip_ipa_powers_bn254_fr_device(const uint64_t x[4], size_t n, void* d_out, void* stream);

/* values[0..4) = <p[half .. 2 half), b[0 .. half)>, values[4..8) = <p[0 .. half), b[half .. 2 half)>  (value_l_j, value_r_j of
 * prover.rs:102-105), 1 <= half <= 2^27.  A fixed reduction order, no atomics: the same inputs give the same limbs.  Waits for
 * `stream` to deliver the 8 limbs. */
int h2hip_ipa_inner_products_bn254_fr_device(const void* d_p, const void* d_b, size_t half, uint64_t values[8], void* stream);

/* The fold of a round (prover.rs:118-131): p[i] += u_inv * p[half + i] and b[i] += u * b[half + i] for i < half, in place, in one pass
 * over both vectors; 1 <= half <= 2^27.  next_values != NULL (half even): the same launch also leaves the next round's
 * h2hip_ipa_inner_products of the folded vectors at half / 2 in next_values[8], and the call waits for `stream`.  next_values == NULL:
 * the call neither reduces nor synchronises. */
int h2hip_ipa_fold_bn254_fr_device(void* d_p, void* d_b, size_t half, const uint64_t u_inv[4], const uint64_t u[4], uint64_t* next_values,
                                   void* stream);

/* compute_s (ipa/strategy.rs:161-176): s[i] = init * prod_{t < k, bit t of i set} u[k - 1 - t] for i < 2^k, 1 <= k <= 28; u: k reduced
 * scalars in host memory (u_1 .. u_k in the transcript's order). */
int h2hip_ipa_compute_s_bn254_fr(const uint64_t* u, uint32_t k, const uint64_t init[4], uint64_t* s);
int h2hip_ipa_compute_s_bn254_fr_device(const uint64_t* u, uint32_t k, const uint64_t init[4], void* d_s, void* stream);

/* Tuning: a collapse of at most max_half points per half runs one quad of lanes per point (a ladder is a latency chain, and a small
 * collapse leaves most of the chip idle), above it one lane per point.  0 restores the default (2^13).  get returns the value in force. */
int h2hip_ipa_set_collapse_quad(size_t max_half);
size_t h2hip_ipa_get_collapse_quad(void);

#ifdef __cplusplus
}
#endif

/* a round as one call -- h2hip_ipa_round_msms_bn254_device, h2hip_ipa_round_bn254_device and their knob: declared in a file of their
 * own (with its own generated binding tables), and part of this header */
#include "halo2hip_ipa_round.h"
#endif
