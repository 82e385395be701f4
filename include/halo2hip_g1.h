/*
 * halo2hip_g1.h -- C ABI of libhalo2hip.so for few-term sums of BN254 G1 points on the host: the group operations a commitment scheme
 * makes between its MSMs -- the [r] W of a blinded commitment, the [value * z] U + [rand] W of an inner-product round, the handful of
 * "other" terms of a verifier's MSM (halo2_proofs/src/poly/ipa/msm.rs:141-174).  These are dependent chains of a few hundred group
 * operations; a host core runs such a chain faster than a GPU lane, so the call is host code and launches nothing.  Layouts, return
 * codes and h2hip_last_error() are halo2hip.h's: elements are 4 x uint64_t Montgomery limbs, G1Affine is x || y with the identity
 * (0, 0), G1 is Jacobian x || y || z with the identity z = 0.
 */
#ifndef HALO2HIP_G1_H
#define HALO2HIP_G1_H

#include "halo2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[j] = addends[j] + sum_{i < t} [scalars[j * t + i]] points[i] for j < m, all m results brought to affine form with one shared
 * field inversion.
 *   addends_xyz  m x 12 limbs, Jacobian as the MSM entry points return them (z = 0: the identity); NULL: no addends.  They are engine
 *                output and are not checked for curve membership
 *   scalars      m x t x 4 limbs, Montgomery form, reduced
 *   points_xy    t x 8 limbs, affine, (0, 0) the identity; the same t points serve all m sums
 *   out_xy       m x 8 limbs, affine, (0, 0) the identity
 * One doubling chain is shared by the t points of a sum (Straus) and every addition is complete: equal operands, opposite operands
 * and identities on either side are legal inputs.  t = 0 is a batch normalisation of the addends; m = 0 succeeds and writes nothing.
 * The call runs on the calling thread, needs no GPU and takes no engine lock.  It is variable-time in its scalars, as every MSM of this
 * library is: do not pass it a secret that must not leak through timing.
 * H2HIP_EINVAL, with its text: a scalar that is not reduced; a point that is neither on the curve nor (0, 0); a null pointer that is
 * needed (out_xy when m > 0; scalars and points_xy when also t > 0); m * t > 4096 -- that is MSM territory, use h2hip_msm_bn254*. */
int h2hip_g1_linear_combinations_bn254(const uint64_t* addends_xyz, const uint64_t* scalars, const uint64_t* points_xy, size_t m, size_t t,
                                       uint64_t* out_xy);

#ifdef __cplusplus
}
#endif
#endif
