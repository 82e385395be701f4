/*
 * halo2hip_pairing.h -- C ABI of libhalo2hip.so for the BN254 optimal ate pairing and the G2 arithmetic a KZG verifier closes with
 * (halo2_proofs/src/poly/kzg/msm.rs:122-169, DualMSM::check: e(left, s_g2) e(right, -g2) = 1).  A check is two Miller loops and one
 * final exponentiation, a dependent chain of some 10^4 Fq products with nothing to spread over lanes, and a batch of proofs folds into
 * one check by a random linear combination; so the call is host code on the calling thread and launches nothing, as
 * halo2hip_g1.h's is.  No call here needs h2hip_init, reads engine state or takes the engine lock; all are re-entrant and
 * variable-time (a verifier's inputs are public).  Return codes and h2hip_last_error() are halo2hip.h's.
 *
 * Layouts.  Field elements are 4 x uint64_t Montgomery limbs.  G1Affine is x || y with the identity (0, 0).  A G2 point is 16 limbs,
 * x.c0 || x.c1 || y.c0 || y.c1 over Fq2 = Fq[u] / (u^2 + 1), affine on the twist y^2 = x^3 + 3 / (9 + u), all zero the identity:
 * the 128 raw bytes of a params file's g2 / s_g2 (SerdeFormat::RawBytes).
 * A Gt value is 48 limbs: twelve Montgomery Fq a_0, b_0, a_1, b_1, ..., a_5, b_5 with the value sum_{i<6} (a_i + b_i u) w^i in
 * Fq12 = Fq2[w] / (w^6 - (9 + u)).  Over Fq alone that is sum_{i<12} c_i w^i in Fq[w] / (w^12 - 18 w^6 + 82) with c_i = a_i - 9 b_i
 * and c_{i+6} = b_i.
 *
 * The pairing is e(P, Q) = ( f_{6t+2,Q}(P) l_{T,pi(Q)}(P) l_{T+pi(Q),-pi^2(Q)}(P) )^((q^12 - 1) / r), t = 4965661367192848881, pi
 * the q-power Frobenius on the untwisted point (x' w^2, y' w^3); the exponent is exactly (q^12 - 1) / r, not a multiple of it.  A pair
 * with the identity on either side contributes 1.
 */
#ifndef HALO2HIP_PAIRING_H
#define HALO2HIP_PAIRING_H

#include "halo2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *ok = 1 iff prod_{i < n} e(P_i, Q_i) = 1, else 0: one shared Miller squaring chain and one final exponentiation.
 *   g1_xy   n x 8 limbs     g2_raw   n x 16 limbs
 * n = 0 gives 1 and reads neither array.
 * H2HIP_EINVAL, with its text, and *ok left as it was: a null pointer that is needed (ok; g1_xy and g2_raw when n > 0); n > 65536 (fold
 * a larger batch into one pair of sums first); a coordinate that is not below q; a G1 point that is neither on the curve nor (0, 0);
 * a G2 point that is not on the twist, or on it and outside the subgroup of order r. */
int h2hip_pairing_check_bn254(const uint64_t* g1_xy, const uint64_t* g2_raw, size_t n, int* ok);

/* out_gt = prod_{i < n} e(P_i, Q_i), in the Gt layout above; n = 0 gives 1.  The same rejections, out_gt in place of ok. */
int h2hip_pairing_bn254(const uint64_t* g1_xy, const uint64_t* g2_raw, size_t n, uint64_t out_gt[48]);

/* out_raw = [scalar] Q, affine.  scalar: one Fr element, 4 Montgomery limbs, reduced.  Q must be on the twist or the identity; it need
 * not be in the subgroup (h2hip_g2_check_bn254 tells).  out_raw may be g2_raw.
 * H2HIP_EINVAL: a null pointer; a scalar that is not reduced; a coordinate that is not below q; a point that is not on the twist. */
int h2hip_g2_mul_bn254(const uint64_t g2_raw[16], const uint64_t scalar[4], uint64_t out_raw[16]);

/* *on_curve = 1 iff Q is on the twist or the identity; *in_subgroup = 1 iff it is also in the subgroup of order r ([r] Q = O; the
 * twist's group has order r (2q - r)).  H2HIP_EINVAL: a null pointer; a coordinate that is not below q. */
int h2hip_g2_check_bn254(const uint64_t g2_raw[16], int* on_curve, int* in_subgroup);

#ifdef __cplusplus
}
#endif
#endif
