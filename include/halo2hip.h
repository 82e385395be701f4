/*
 * halo2hip.h -- C ABI of libhalo2hip.so, the MI355X (gfx950) engine for the halo2_proofs
 * proving hot path: BN254 G1 multi-scalar multiplication and the radix-2 NTT over BN254 Fr.
 *
 * The reference (eldenpark/halo2-pse, Rust) has no FFI layer: the seam is two generic free
 * functions plus the KZG commit methods built on them.  Each entry point below names the
 * reference interface it replaces (paths relative to halo2_proofs/src/ in the reference);
 * the Rust side ships as files: halo2hip-sys/ (extern block generated from this header, safe wrappers) and
 * patches/0001..0003 against the reference.
 *
 * Data layout at the boundary (identical to halo2curves 0.3.1 in memory and to
 * SerdeFormat::RawBytes, helpers.rs:13-19):
 *   Fr / Fq element : 4 x uint64_t little-endian limbs, Montgomery form (R = 2^256), < modulus
 *   G1Affine        : x || y            (8 x uint64_t, 64 B), identity = all zero
 *   G1 (projective) : x || y || z       (12 x uint64_t, 96 B), Jacobian, identity z = 0
 *
 * Conventions: every function returns 0 on success and a non-zero H2HIP_E* code otherwise
 * (never throws / unwinds; the Rust shim falls back to the original CPU body on non-zero).
 * h2hip_last_error() describes the last failure on the calling thread.  All entry points are
 * thread-safe and blocking.  One process drives the GPUs named at h2hip_init: host-pointer MSMs
 * are sharded over all of them inside the call (the fan-out and fold best_multiexp performs over
 * rayon threads, arithmetic.rs:137-153), everything else runs on the first device, or -- for the
 * _device entry points -- on the device that owns the pointers, under that device's lock only (calls
 * on different devices overlap; a batched transform whose columns live on several devices is split by owner).
 * There is no CPU fallback inside the library: without a usable GPU every compute entry
 * point fails with H2HIP_EDEVICE.
 *
 * Environment (read at init): HALO2_HIP_DEVICES="0,1,.." device list when h2hip_init gets none;
 * HALO2_HIP_MULTI_GPU_MIN_N (default 2^18) smallest MSM that is sharded; HALO2_HIP_GATHER=host|rccl
 * how the devices' partial sums meet (default host: each device's sum has come back with its run, the
 * calling thread folds them; rccl: ncclAllGather from the devices' HBM over xGMI, fixed-base form);
 * HALO2_HIP_MSM_WINDOW; HALO2_HIP_STREAM=0 uploads a host-slice MSM's arrays whole instead of streaming them in chunks
 * (no copier thread), HALO2_HIP_STREAM_MIN_N (default 2^19) is the smallest MSM that streams; HALO2_HIP_FIXED_BASE=0 and
 * HALO2_HIP_TABLE_MAX_GB for h2hip_bases_pin's window tables; HALO2_HIP_MSM_MIN_N /
 * HALO2_HIP_NTT_MIN_LOGN thresholds the Rust shim reads back through h2hip_msm_min_n() /
 * h2hip_ntt_min_log_n(); HALO2_HIP_ROCTX=1 roctx ranges around every entry point;
 * HALO2_HIP_NTT_TWIDDLE_MB (default 4096) HBM per device for the full inter-pass twiddle tables of 2^20-, 2^21-, 2^23- and 2^24-point
 * transforms (36 bytes per point, domain and direction; without room the two-level table serves, one multiplication more per point);
 * HALO2_HIP_LAZY_PIN=k (default 0 = off) lets the library pin a host bases array by itself once a
 * host-pointer MSM has seen it k times (see h2hip_bases_pin); HALO2_HIP_EVALH_CODEGEN=0|1|2 the kernels the evaluate_h calls generate per
 * circuit: the gates', one per lookup, shuffle and mv-lookup argument (0: byte-code interpreter only; 1, default: compiled by hiprtc on a background
 * thread, the interpreter serves until then; 2: inline; + 32 / + 64: no / both stage kernels) and HALO2_HIP_CACHE_DIR a directory that keeps those code objects across processes
 * (files there are loaded as GPU code, keyed by a hash of their source: the directory must be writable by the prover's user only);
 * HALO2_HIP_RANDOM_MIN_N (default 2^9, read at the first call) the element count from which the host forms of h2hip_fr_random_bn254 /
 * h2hip_fr_from_bytes_wide_bn254 go to the device; below it they are a handful of draws on the calling thread, by design and not as a fallback;
 * HALO2_HIP_COLUMN_CACHE_GB (default 64) the HBM that h2hip_columns_pin's columns and h2hip_part_cosets_pin's part cosets may take
 * together, least recently used entries of either kind dropped first.
 */
#ifndef HALO2HIP_H
#define HALO2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2HIP_OK 0
#define H2HIP_EINVAL 1   /* contract violation (the reference would panic: arithmetic.rs:133,184) */
#define H2HIP_EDEVICE 2  /* HIP runtime / device error, or no GPU */
#define H2HIP_ENOMEM 3
#define H2HIP_ELOOKUP 4  /* a lookup's input holds a value its table lacks (lookup::Argument::commit_permuted: Error::ConstraintSystemFailure) */
#define H2HIP_EENCODING 5  /* an element fails its format's checks (the reference's io::Error "invalid point encoding" / "Invalid prime field point encoding") */

/* ---- lifecycle ------------------------------------------------------------------------- */

/* Bind the engine to n_devices GPUs (HIP device ordinals).  device_ids == NULL or n_devices == 0: the
 * HALO2_HIP_DEVICES list, else the calling thread's current HIP device.  Idempotent for the same list;
 * a different list needs h2hip_shutdown first (H2HIP_EINVAL otherwise).  With more than one device the
 * engine starts one host thread and one stream per device and, with HALO2_HIP_GATHER=rccl and librccl
 * present, one RCCL communicator per device (ncclCommInitAll) for the gather of the MSM partials.  An id out of range or
 * listed twice is H2HIP_EINVAL. */
int h2hip_init(const int* device_ids, int n_devices);
void h2hip_shutdown(void);
const char* h2hip_last_error(void);
const char* h2hip_version(void);
/* number of visible HIP devices, or -1 when the runtime reports an error */
int h2hip_device_count(void);
/* devices the engine is bound to (0 before init) */
int h2hip_num_devices(void);
/* dispatch thresholds for the shim: below them the reference's CPU body is the faster path.  Without a usable GPU they answer
 * "never" (SIZE_MAX / UINT32_MAX) from a cached failure -- no lock, no HIP call -- so the CPU-fallback path of a prover on a GPU-less host costs nothing;
 * h2hip_init or h2hip_shutdown makes the library look for a device again. */
size_t h2hip_msm_min_n(void);
uint32_t h2hip_ntt_min_log_n(void);

/* ---- best_multiexp: arithmetic.rs:132-159 ------------------------------------------------ */

/* out = sum_i scalars[i] * bases[i].  Replaces
 *   pub fn best_multiexp<C: CurveAffine>(coeffs: &[C::Scalar], bases: &[C]) -> C::Curve
 * for C = bn256::G1Affine, and through it ParamsKZG::commit / commit_lagrange
 * (poly/kzg/commitment.rs:281-292, :327-334) and MSMKZG::eval (poly/kzg/msm.rs:65-70).
 * Host pointers; n == 0 gives the identity.  The group element equals the reference's for
 * every thread count; Jacobian coordinates are not specified by the reference
 * (they depend on rayon's thread count, arithmetic.rs:153) and may differ from call to call here too.
 * The slices are the caller's (pageable) memory, borrowed for the call.  From 2^19 pairs up the scalars -- and, when
 * the bases are not pinned, the points -- cross PCIe in chunks that stream in under the work and add into one bucket
 * set, so only the first chunk's upload is exposed (2^20 pairs over pinned bases: 1.6 ms against 1.25 ms for
 * device-resident inputs).  With several devices every device's share streams over its own link.  Blocking and
 * thread-safe: concurrent callers (rayon workers) are serialised per device. */
int h2hip_msm_bn254(const uint64_t* scalars, const uint64_t* bases_xy, size_t n, uint64_t out_xyz[12]);

/* Keep `bases_xy[0..n)` on the GPU(s), keyed by the host pointer: later h2hip_msm_bn254[_batch] calls
 * whose bases pointer equals `bases_xy` (and n' <= n) skip the upload.  For ParamsKZG::{g, g_lagrange}
 * (poly/kzg/commitment.rs:26-27), which live as long as the params; call unpin before the Vec is dropped
 * or mutated (downsize, :267-275).  With several devices each one keeps its contiguous share.
 * Pinning also builds the fixed-base window table 2^(pos_j) * P_i (pos_j = first bit of window j, W = ceil(255/c) windows; n <= 2^26; from 2^13
 * points W * n * 128 bytes of HBM -- the multiplier's own limb form, one record per line: 1.7 GB at 2^20, 26 GB at 2^24 -- and W * n * 64 bytes
 * below that, or where the larger table exceeds HALO2_HIP_TABLE_MAX_GB or does not fit; h2hip_bases_pinned_info reports the bytes in use):
 * all windows of an MSM then share one bucket set, the windows are wider (c = 20 instead of 16 at 2^20) and no Horner pass is needed.
 * The cache is safe against stale pointers: every lookup compares 16 sampled points of the caller's array (the first
 * point and a geometric ladder of indices up to the last, so that a shorter prefix still sees several) with the ones seen
 * at pin time and falls back to a plain upload (dropping the entry) on a mismatch. */
int h2hip_bases_pin(const uint64_t* bases_xy, size_t n);
/* The lazy cache (HALO2_HIP_LAZY_PIN=k): for the unpatched two-line drop-in, whose best_multiexp(coeffs, bases) has no
 * handle in its signature.  A host array that reaches h2hip_msm_bn254[_batch] unpinned for the k-th time with the same
 * address, length and sampled points is pinned as above by the library (at most 4 such arrays, least recently used
 * dropped first; h2hip_bases_unpin removes one, h2hip_shutdown all).  Lookups validate it like any pinned entry.  What the
 * samples cannot see is a caller rewriting part of a live array in place; ParamsKZG never does, hence opt-in. */
uint32_t h2hip_lazy_pin_after(void);
/* the same for points that already live in HBM (keyed by the device pointer, used by the _device MSMs).  The points are
 * copied into the table, but the caller's buffer stays the KEY: keep it alive and unchanged until h2hip_bases_unpin, as a
 * ParamsKZG keeps g.  Should it be freed and its address reused all the same, the cache notices: a one-wave kernel ahead
 * of every MSM compares 16 sampled points of the buffer with the ones seen at pin time (no extra synchronisation; the
 * verdict is read with the MSM's result), and on a mismatch the entry is dropped and the MSM runs over the caller's points. */
int h2hip_bases_pin_device(const void* d_bases_xy, size_t n, void* stream);
/* drops a pinned host array or device buffer; H2HIP_EINVAL when the pointer is not pinned (also when the engine is not
 * initialised: the call never starts it) */
int h2hip_bases_unpin(const void* bases_xy);
/* what a pinned pointer holds: points, window width / windows of its table (0 / 0 without one), bytes of HBM */
int h2hip_bases_pinned_info(const void* bases_xy, size_t* n_points, uint32_t* window_bits, uint32_t* windows, size_t* device_bytes);

/* Same computation on device-resident inputs (scalars n x 32 B, bases n x 64 B in HBM);
 * `stream` is a hipStream_t; NULL is HIP's default (null) stream, as everywhere in HIP.  All
 * kernels are enqueued on that stream, so the inputs may be produced by earlier work on it;
 * the call returns after the stream is synchronised and the result is in host memory. */
int h2hip_msm_bn254_device(const void* d_scalars, const void* d_bases_xy, size_t n, uint64_t out_xyz[12], void* stream);

/* `count` independent MSMs of n pairs each over the SAME bases: out_xyz[12*j..] = sum_i scalars[j][i] * bases[i].
 * This is what create_proof does when it commits its columns back to back (plonk/prover.rs:361-365:
 * `params.commit_lagrange(poly, blind)` for every advice polynomial; lookup/prover.rs:127-132, :291;
 * vanishing/prover.rs:104).  Results equal `count` separate h2hip_msm_bn254 calls.  Up to 2^19 pairs the MSMs of a batch
 * run fused (one sort / accumulate / reduce over the windows of all of them); larger ones are pipelined whole over three
 * streams (sort of j+1 and reduction of j-1 under the accumulation of j). */
int h2hip_msm_bn254_batch(const uint64_t* const* scalars, const uint64_t* bases_xy, size_t n, size_t count, uint64_t* out_xyz);
int h2hip_msm_bn254_batch_device(const void* const* d_scalars, const void* d_bases_xy, size_t n, size_t count, uint64_t* out_xyz, void* stream);

/* CurveExt::batch_normalize (plonk/prover.rs:368-371 normalises the advice commitments before writing them to the
 * transcript): k Jacobian points -> k affine points with one field inversion; identity -> (0,0).  Host-side. */
int h2hip_g1_batch_normalize(const uint64_t* xyz, size_t k, uint64_t* xy);

/* Left fold of k Jacobian partial sums from the identity -- the fold at arithmetic.rs:153.
 * Inside one process h2hip_msm_bn254 does this itself over the devices of h2hip_init.  With one process per
 * GPU (bench.py --gpus N) each rank computes its shard's partial with h2hip_msm_bn254[_device], the
 * 96-byte partials are all-gathered (RCCL, bytes), and every rank folds them with this. */
int h2hip_g1_fold(const uint64_t* partials_xyz, size_t k, uint64_t out_xyz[12]);
/* Curve::to_affine; identity -> (0,0) */
int h2hip_g1_to_affine(const uint64_t xyz[12], uint64_t xy[8]);

/* ---- best_fft and the EvaluationDomain conversions built on it --------------------------- */

/* In-place radix-2 NTT, natural order in and out: a[i] <- sum_j a[j] * omega^(i*j).  Replaces
 *   pub fn best_fft<G: Group>(a: &mut [G], omega: G::Scalar, log_n: u32)       arithmetic.rs:171
 * for G = bn256::Fr.  `a` has 2^log_n elements; omega must have exact order 2^log_n (true for
 * every in-crate caller: poly/domain.rs:248,354); log_n <= 28. */
int h2hip_ntt_bn254_fr(uint64_t* a, const uint64_t omega[4], uint32_t log_n);
int h2hip_ntt_bn254_fr_device(void* d_a, const uint64_t omega[4], uint32_t log_n, void* stream);

/* EvaluationDomain::ifft (poly/domain.rs:353-361): best_fft(a, omega_inv, log_n) then
 * a[i] *= divisor, fused into one device round trip.  lagrange_to_coeff (:226-236) is this
 * with (omega_inv, k, ifft_divisor). */
int h2hip_ifft_bn254_fr(uint64_t* a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]);
int h2hip_ifft_bn254_fr_device(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void* stream);

/* EvaluationDomain::coeff_to_extended (poly/domain.rs:240-254): out[0..2^extended_k) =
 * best_fft(zero-pad(distribute_powers_zeta(a[0..2^k), into_coset = true)), extended_omega).
 * g_coset = ZETA, g_coset_inv = ZETA^2 as stored in the domain (:81-82). */
int h2hip_coeff_to_extended_bn254_fr(const uint64_t* a, uint32_t k, uint64_t* out, uint32_t extended_k,
                                     const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]);
/* device form: d_a holds 2^extended_k elements of which the first 2^k are the input */
int h2hip_coeff_to_extended_bn254_fr_device(void* d_a, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                                            const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* stream);

/* One part of coeff_to_extended (upstream halo2's coeff_to_extended_part), 2^k elements in and out:
 * out[j] = row j * P + part of h2hip_coeff_to_extended_bn254_fr(a): the 2^k-point transform of a[m] * g_p^m over omega = extended_omega^P,
 * g_p = g_coset * extended_omega^part, P = 2^(extended_k - k), part < P.  Limb for limb the full conversion's rows.  The scaling by g_p^m
 * is fused into the transform's first-pass load.  k > extended_k, extended_k > 28, part >= P or a null pointer: H2HIP_EINVAL before any
 * device work. */
int h2hip_coeff_to_extended_part_bn254_fr(const uint64_t* a, uint32_t k, uint32_t extended_k, uint32_t part, const uint64_t extended_omega[4],
                                          const uint64_t g_coset[4], const uint64_t g_coset_inv[4], uint64_t* out);      /* out may equal a */
/* device form: d_a and d_out hold 2^k elements each and may be equal */
int h2hip_coeff_to_extended_part_bn254_fr_device(const void* d_a, uint32_t k, uint32_t extended_k, uint32_t part, const uint64_t extended_omega[4],
                                                 const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* d_out, void* stream);
/* count transforms in one launch per pass; d_a[i] / d_out[i] device pointers in host arrays, parts[i] the part of transform i (host array), so
 * all P parts of one polynomial are one call with d_a[i] equal for all i.  d_out[i] may equal d_a[i] only where that source feeds no other i.
 * count == 0 writes nothing.  The transforms run on the device that owns d_out[0]. */
int h2hip_coeff_to_extended_part_bn254_fr_batch_device(const void* const* d_a, void* const* d_out, const uint32_t* parts, size_t count, uint32_t k,
                                                       uint32_t extended_k, const uint64_t extended_omega[4], const uint64_t g_coset[4],
                                                       const uint64_t g_coset_inv[4], void* stream);

/* EvaluationDomain::extended_to_coeff (poly/domain.rs:281-303) without the final truncate:
 * ifft(a, extended_omega_inv, extended_k, extended_ifft_divisor) then
 * distribute_powers_zeta(a, into_coset = false), in place on 2^extended_k elements. */
int h2hip_extended_to_coeff_bn254_fr(uint64_t* a, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                     const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]);
int h2hip_extended_to_coeff_bn254_fr_device(void* d_a, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                            const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4],
                                            const uint64_t g_coset_inv[4], void* stream);

/* EvaluationDomain::divide_by_vanishing_poly (poly/domain.rs:307-326): a[i] *= t_evaluations[i % t_len] on the
 * 2^extended_k coset evaluations, t_evaluations = the domain's inverted t(X) = X^n - 1 values (:84-124). */
int h2hip_divide_by_vanishing_poly_bn254_fr(uint64_t* a, uint32_t extended_k, const uint64_t* t_evaluations, uint32_t t_len);
int h2hip_divide_by_vanishing_poly_bn254_fr_device(void* d_a, uint32_t extended_k, const uint64_t* t_evaluations, uint32_t t_len, void* stream);

/* ---- device-resident polynomials ---------------------------------------------------------
 * A caller without a HIP binding (the Rust shim) keeps columns on the GPU across calls -- commit a column with
 * h2hip_msm_bn254_device, then h2hip_ifft_bn254_fr_device / h2hip_coeff_to_extended_bn254_fr_device on the same
 * buffer -- instead of crossing PCIe for every call.  Plain hipMalloc'd memory; `stream` as elsewhere. */
int h2hip_device_alloc(size_t bytes, void** d_ptr);
int h2hip_device_free(void* d_ptr);
int h2hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int h2hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int h2hip_memset_zero(void* d_dst, size_t bytes, void* stream);
int h2hip_stream_synchronize(void* stream);

/* ---- batched device-resident transforms: `count` columns of one size in one launch per NTT pass.  d_a is a HOST array of
 * `count` device pointers; semantics per column are those of the unbatched _device entry points.  create_proof converts
 * its columns back to back (plonk/prover.rs:487 lagrange_to_coeff per advice column; plonk/evaluation.rs:306-323
 * coeff_to_extended per advice / instance column): at 2^17..2^20 points per column one transform does not fill the GPU. */
int h2hip_ntt_bn254_fr_batch_device(void* const* d_a, size_t count, const uint64_t omega[4], uint32_t log_n, void* stream);
int h2hip_ifft_bn254_fr_batch_device(void* const* d_a, size_t count, const uint64_t omega_inv[4], uint32_t log_n,
                                     const uint64_t divisor[4], void* stream);
int h2hip_coeff_to_extended_bn254_fr_batch_device(void* const* d_a, size_t count, uint32_t k, uint32_t extended_k,
                                                  const uint64_t extended_omega[4], const uint64_t g_coset[4],
                                                  const uint64_t g_coset_inv[4], void* stream);

/* ---- batched transforms on HOST columns: what the prover has when its polynomials are `Vec<F>`s (plonk/prover.rs:476-490 converts
 * every advice column with lagrange_to_coeff; plonk/evaluation.rs:306-323 extends every advice / instance column with coeff_to_extended).
 * `a` / `out` are host arrays of `count` host pointers; semantics per column are those of the unbatched host entry points.  The columns
 * run as a three-stage pipeline -- column i + 1 crosses PCIe upwards and column i - 1 downwards while column i is transformed -- so a
 * column costs max(upload, transform, download) instead of their sum (2^22: 5.4 ms one call each).  With several devices the columns
 * are dealt to them in contiguous shares, each share over its own PCIe link (NTT replicas; no column crosses xGMI).  Blocking. */
int h2hip_ntt_bn254_fr_batch(uint64_t* const* a, size_t count, const uint64_t omega[4], uint32_t log_n);
int h2hip_ifft_bn254_fr_batch(uint64_t* const* a, size_t count, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]);
/* a[i]: 2^k coefficients in, out[i]: 2^extended_k evaluations out (a[i] and out[i] may not overlap unless equal) */
int h2hip_coeff_to_extended_bn254_fr_batch(const uint64_t* const* a, uint32_t k, uint64_t* const* out, size_t count, uint32_t extended_k,
                                           const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]);
int h2hip_extended_to_coeff_bn254_fr_batch(uint64_t* const* a, size_t count, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                           const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]);

/* ---- g_to_lagrange: arithmetic.rs:277-301 (best_fft with G = G1, then 1/n and batch_normalize); called by
 * ParamsKZG::downsize, poly/kzg/commitment.rs:267-275.  g_xy: 2^k affine points (the coefficient-basis SRS, possibly
 * truncated); g_lagrange_xy: 2^k affine points out.  k <= 28.  Input and output may not overlap. */
int h2hip_g_to_lagrange_bn254(const uint64_t* g_xy, uint32_t k, uint64_t* g_lagrange_xy);
int h2hip_g_to_lagrange_bn254_device(const void* d_g_xy, uint32_t k, void* d_g_lagrange_xy, void* stream);

/* best_fft with G = bn256::G1 and a caller-supplied omega (arithmetic.rs:171-234; in the crate only g_to_lagrange calls it, :285): in place on
 * 2^log_n Jacobian points (96 B each, identity z = 0), a[i] <- sum_j [omega^(i*j)] a[j].  omega of exact order 2^log_n; log_n <= 28.  Only
 * the group elements are defined by the reference (its Jacobian coordinates depend on the butterfly order and rayon's thread count): the
 * points come back with z = 1 (identity: (0, 1, 0)), compare after normalising. */
int h2hip_fft_bn254_g1(uint64_t* a_xyz, const uint64_t omega[4], uint32_t log_n);
int h2hip_fft_bn254_g1_device(void* d_a_xyz, const uint64_t omega[4], uint32_t log_n, void* stream);

/* ---- ParamsKZG::setup: poly/kzg/commitment.rs:61-129, with the secret supplied by the caller (the reference draws it from
 * an rng at :72): g[i] = [s^i] G1 and g_lagrange[i] = [l_i(s)] G1 for i < 2^k, affine, as batch_normalize leaves them.
 * k <= 28; a secret that is a 2^k-th root of unity is H2HIP_EINVAL (the reference panics on the inversion at :100).
 * The G2 half of the parameters (g2, s_g2: :118-119) belongs to the verifier and is not produced here. */
int h2hip_kzg_setup_bn254(uint32_t k, const uint64_t secret[4], uint64_t* g_xy, uint64_t* g_lagrange_xy);
int h2hip_kzg_setup_bn254_device(uint32_t k, const uint64_t secret[4], void* d_g_xy, void* d_g_lagrange_xy, void* stream);

/* ---- Evaluator::evaluate_h: plonk/evaluation.rs:280-522 ---------------------------------------
 * The quotient numerator h(X) on the extended coset: per row, the custom-gate graph (GraphEvaluator, :191-201,
 * :708-749), the permutation argument's constraints (:362-441) and every lookup's constraints (:443-518), folded
 * with powers of y.  The reference's Rust structures are passed flattened:
 *   ValueSource  (evaluation.rs:37-60)   -> h2hip_value_source {kind, a, b}
 *   Calculation + CalculationInfo (:108-127, :213-219) -> h2hip_calculation
 *   GraphEvaluator (:191-201)            -> h2hip_graph
 * One call handles one circuit instance; `values` is read and written (the reference folds all instances into
 * the same polynomial, :326-332), so pass zeros for the first instance. */
enum {
    H2HIP_VS_CONSTANT = 0, H2HIP_VS_INTERMEDIATE = 1, H2HIP_VS_FIXED = 2, H2HIP_VS_ADVICE = 3, H2HIP_VS_INSTANCE = 4,
    H2HIP_VS_CHALLENGE = 5, H2HIP_VS_BETA = 6, H2HIP_VS_GAMMA = 7, H2HIP_VS_THETA = 8, H2HIP_VS_Y = 9, H2HIP_VS_PREVIOUS = 10
};
enum {
    H2HIP_CALC_ADD = 0, H2HIP_CALC_SUB = 1, H2HIP_CALC_MUL = 2, H2HIP_CALC_SQUARE = 3, H2HIP_CALC_DOUBLE = 4,
    H2HIP_CALC_NEGATE = 5, H2HIP_CALC_HORNER = 6, H2HIP_CALC_STORE = 7
};
enum { H2HIP_ANY_ADVICE = 0, H2HIP_ANY_FIXED = 1, H2HIP_ANY_INSTANCE = 2 };

typedef struct {
    uint32_t kind; /* H2HIP_VS_* */
    uint32_t a;    /* constant / intermediate / challenge index, or column index */
    uint32_t b;    /* index into the graph's rotations for Fixed / Advice / Instance */
} h2hip_value_source;

typedef struct {
    uint32_t op;     /* H2HIP_CALC_* */
    uint32_t target; /* intermediate written (CalculationInfo::target) */
    h2hip_value_source x, y; /* operands; Horner: x = start value, y = factor */
    uint32_t parts_offset, parts_count; /* Horner parts in h2hip_graph::parts */
} h2hip_calculation;

typedef struct {
    const uint64_t* constants; /* n_constants x 4 */
    uint32_t n_constants;
    const int32_t* rotations;
    uint32_t n_rotations;
    const h2hip_calculation* calculations;
    uint32_t n_calculations;
    const h2hip_value_source* parts;
    uint32_t n_parts;
    uint32_t num_intermediates; /* <= 256 in this engine */
} h2hip_graph;

typedef struct {
    /* domain (poly/domain.rs:18-34) */
    uint32_t k, extended_k;
    const uint64_t *extended_omega, *g_coset, *g_coset_inv;
    /* columns: pk.fixed_cosets (extended), advice / instance polynomials in coefficient form (2^k each; their cosets
     * are formed here with coeff_to_extended as at evaluation.rs:306-323) */
    uint32_t n_fixed, n_advice, n_instance, n_challenges;
    const uint64_t* const* fixed_cosets;
    const uint64_t* const* advice_polys;
    const uint64_t* const* instance_polys;
    const uint64_t* challenges;              /* n_challenges x 4 */
    const uint64_t *y, *beta, *gamma, *theta;
    const uint64_t *l0, *l_last, *l_active_row; /* pk.l0 / l_last / l_active_row, extended */
    h2hip_graph custom_gates;                /* Evaluator::custom_gates */
    /* permutation argument (evaluation.rs:362-441); n_perm_sets == 0 skips it */
    uint32_t n_perm_sets, n_perm_columns, chunk_len; /* chunk_len = cs.degree() - 2 */
    int32_t last_rotation;                   /* -(blinding_factors + 1) */
    const uint64_t* const* perm_product_cosets; /* sets[i].permutation_product_coset, extended */
    const uint32_t* perm_column_kind;        /* H2HIP_ANY_* of p.columns[j] */
    const uint32_t* perm_column_index;
    const uint64_t* const* perm_cosets;      /* pk.permutation.cosets[j], extended */
    const uint64_t *zeta, *delta;            /* Fr::ZETA, Fr::DELTA */
    /* lookups (evaluation.rs:443-518) */
    uint32_t n_lookups;
    const h2hip_graph* lookup_graphs;        /* Evaluator::lookups[n] */
    const uint64_t* const* lookup_product_polys;        /* coefficient form, 2^k each */
    const uint64_t* const* lookup_permuted_input_polys;
    const uint64_t* const* lookup_permuted_table_polys;
} h2hip_evalh_desc;

/* The constant columns of a proving key -- pk.fixed_cosets, pk.l0 / l_last / l_active_row, pk.permutation.cosets (plonk.rs:262-272): extended-coset
 * form, `elems` = 2^extended_k elements each -- kept in HBM across h2hip_evaluate_h_bn254 calls, keyed by their host pointers: the host-pointer
 * evaluate_h then uploads only what changes from proof to proof (at k = 18 in the bench system 22 of its 27 full-size columns are constant:
 * 2.8 of 3.5 GB per call).  Idempotent; guarded like h2hip_bases_pin (16 sampled elements of the caller's memory are compared on every use, a
 * mismatch drops the copy and uploads); HALO2_HIP_COLUMN_CACHE_GB (default 64) bounds the HBM taken, least recently used columns go first.
 * Unpin before the Vecs are dropped (ProvingKey's Drop); unknown pointers are ignored; neither call changes any result. */
int h2hip_columns_pin(const uint64_t* const* cols, size_t count, size_t elems);
int h2hip_columns_unpin(const uint64_t* const* cols, size_t count);
int h2hip_columns_pinned_info(size_t* n_columns, size_t* device_bytes);

/* values: 2^extended_k elements, in/out, host memory; every column pointer in desc is host memory */
int h2hip_evaluate_h_bn254(const h2hip_evalh_desc* desc, uint64_t* values);
/* Device-resident form for a prover whose columns already live in HBM: every column pointer in desc (fixed_cosets[i],
 * advice_polys[i], instance_polys[i], l0 / l_last / l_active_row, perm_product_cosets[i], perm_cosets[j], the lookup
 * polynomials) and d_values are device pointers; extended cosets are read where they lie, coefficient-form polynomials
 * are copied device-to-device before they are extended, so no input is modified.  The pointer tables themselves,
 * the graphs, challenges and scalars stay host memory.  Kernels are queued on `stream` (NULL = the default stream);
 * the call does not wait for them. */
int h2hip_evaluate_h_bn254_device(const h2hip_evalh_desc* desc, void* d_values, void* stream);

/* evaluate_h one coset of the 2^k domain at a time.  With P = 2^(extended_k - k), extended row j * P + p lies at g_p * omega^j with
 * g_p = g_coset * extended_omega^p and omega = extended_omega^P, so the rows of part p are the 2^k-point transform of f(g_p X) and are
 * closed under every rotation the constraints use.  Every column is given as a coefficient-form polynomial of 2^k elements -- the key's
 * too: pk.fixed_polys, pk.l0 / l_last / l_active_row as polynomials, pk.permutation.polys -- and the engine forms one part's cosets at a
 * time, so it holds columns of 2^k elements where the full form holds columns of 2^extended_k, and a proving key need not keep its
 * extended cosets at all.  The result is the full form's, limb for limb.  Fields up to lookup_permuted_table_polys mirror
 * h2hip_evalh_desc. */
typedef struct h2hip_evalh_parts_desc {
    uint32_t k, extended_k;
    const uint64_t *extended_omega, *g_coset, *g_coset_inv;
    uint32_t n_fixed, n_advice, n_instance, n_challenges;
    const uint64_t* const* fixed_polys;      /* every column below: coefficient form, 2^k elements */
    const uint64_t* const* advice_polys;
    const uint64_t* const* instance_polys;
    const uint64_t* challenges;              /* n_challenges x 4 */
    const uint64_t *y, *beta, *gamma, *theta;
    const uint64_t *l0_poly, *l_last_poly, *l_active_row_poly;
    h2hip_graph custom_gates;
    uint32_t n_perm_sets, n_perm_columns, chunk_len;
    int32_t last_rotation;
    const uint64_t* const* perm_product_polys; /* sets[i].permutation_product_poly */
    const uint32_t* perm_column_kind;
    const uint32_t* perm_column_index;
    const uint64_t* const* perm_polys;       /* pk.permutation.polys[j] */
    const uint64_t *zeta, *delta;
    uint32_t n_lookups;
    const h2hip_graph* lookup_graphs;
    const uint64_t* const* lookup_product_polys;
    const uint64_t* const* lookup_permuted_input_polys;
    const uint64_t* const* lookup_permuted_table_polys;
    /* the parts this call computes: part_begin .. part_begin + part_count - 1 of the P; 0, 0 = all of them.  Rows of `values` that
     * belong to other parts are neither read nor written, so two devices, or two calls, can split one h(X). */
    uint32_t part_begin, part_count;
    /* NULL, or the P elements of EvaluationDomain::t_evaluations: part p's rows then leave multiplied by t_evaluations[p], which makes
     * the result divide_by_vanishing_poly(h) (poly/domain.rs:307-326).  Set it on the call of the last circuit instance only. */
    const uint64_t* t_evaluations;
} h2hip_evalh_parts_desc;

/* values: 2^extended_k elements, in/out, host memory, in the reference's row order; every column pointer in desc is host memory.  Each
 * column is uploaded once per call (2^k elements), not once per part. */
int h2hip_evaluate_h_parts_bn254(const h2hip_evalh_parts_desc* desc, uint64_t* values);
/* Device-resident form: the columns and d_values are device pointers, no input is modified; kernels are queued on `stream` only and the
 * call does not wait for them. */
int h2hip_evaluate_h_parts_bn254_device(const h2hip_evalh_parts_desc* desc, void* d_values, void* stream);
/* HBM the engine itself allocates for the columns of one evaluate_h call and, in the host-pointer forms, its copy of `values` (the
 * metadata and the slot workspace of programs with more than 256 live values come on top).  parts_form / device_form select among the
 * four entry points above.  For the parts form this is the upper bound, reached when no part cosets are pinned (below): a pinned
 * polynomial takes no arena column.  Host only: needs no device. */
int h2hip_evaluate_h_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                     uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, int parts_form, int device_form,
                                     size_t* bytes);

/* The shuffle argument's share of h(X) (upstream PSE halo2's Evaluator::shuffles; later than the reference).  The
 * two descriptors above carry no size field and keep their layout; a circuit's shuffles travel beside them:
 *   graphs[2j]      the input side of shuffle j:  add_expression of each input expression, Horner(Constant(0), parts, Theta), Add(that, Gamma)
 *   graphs[2j + 1]  the shuffle side, built the same way
 *   product_polys[j]  the grand product z_j in coefficient form, 2^k elements (h2hip_shuffle_products_bn254, then lagrange_to_coeff)
 * A graph's value is the target of its last calculation (zero for an empty graph); call the two a = A + gamma and s = S + gamma.  After
 * the custom gates, the permutation argument and every lookup of the instance, shuffle j (before shuffle j + 1) folds, with zc the
 * extended coset of z_j and r_next the row one rotation on,
 *   v = v y + (1 - zc[idx]) l0[idx];   v = v y + (zc[idx]^2 - zc[idx]) l_last[idx];   v = v y + l_active_row[idx] (zc[r_next] s - zc[idx] a).
 * A shuffle graph may read fixed, advice, instance, challenge, constant, intermediate, theta and gamma; beta, y or the previous value is
 * H2HIP_EINVAL before any device work.  A shuffle's two graphs run as one kernel generated for the pair, or on the byte-code interpreter.
 * shuffles == NULL or n_shuffles == 0 is the call without the suffix, limb for limb; in the parts form t_evaluations still multiplies
 * last.  n_shuffles <= 65535. */
typedef struct h2hip_evalh_shuffles {
    uint32_t n_shuffles;
    const h2hip_graph* graphs;
    const uint64_t* const* product_polys;
} h2hip_evalh_shuffles;
int h2hip_evaluate_h_shuffles_bn254(const h2hip_evalh_desc* desc, const h2hip_evalh_shuffles* shuffles, uint64_t* values);
int h2hip_evaluate_h_shuffles_bn254_device(const h2hip_evalh_desc* desc, const h2hip_evalh_shuffles* shuffles, void* d_values, void* stream);
int h2hip_evaluate_h_parts_shuffles_bn254(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_shuffles* shuffles, uint64_t* values);
int h2hip_evaluate_h_parts_shuffles_bn254_device(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_shuffles* shuffles, void* d_values,
                                                 void* stream);
/* h2hip_evaluate_h_workspace_bytes for a call with n_shuffles shuffles (0: the same number): the product cosets of one group of shuffles
 * come on top, and in the host parts form their coefficient columns */
int h2hip_evaluate_h_shuffles_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                              uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, uint32_t n_shuffles,
                                              int parts_form, int device_form, size_t* bytes);

/* The logUp (mv-lookup) argument's share of h(X) (the definitions: "grand products" below, h2hip_mvlookup_multiplicities_bn254; DESIGN.md
 * section 2).  Like the shuffles, a circuit's mv-lookups travel beside the unchanged descriptors.  Argument j has K_j = n_inputs[j] input
 * tuples sharing one table; its K_j + 1 graphs lie consecutively in `graphs`, behind those of argument j - 1: the input graphs, then the
 * table graph, each add_expression of the tuple's expressions, Horner(Constant(0), parts, Theta), Add(that, Beta).  A graph's value is
 * the target of its last calculation (zero for an empty graph); call them f_0 .. f_{K-1} and tau, and
 *   P = prod_c f_c,   Q = sum_c prod_{l != c} f_l   (streamed as Q <- Q f + P; P <- P f: no inversion on the coset).
 * phi_polys[j] / m_polys[j] are the grand sum and the multiplicities in coefficient form, 2^k elements (h2hip_mvlookup_sums_bn254 /
 * h2hip_mvlookup_multiplicities_bn254, then lagrange_to_coeff); pc, mc their extended cosets, r_next the row one rotation on.  After the
 * custom gates, the permutation argument and every halo2 lookup of the descriptor, and before the shuffles, argument j folds
 *   v = v y + l0[idx] pc[idx];   v = v y + l_last[idx] pc[idx];
 *   v = v y + l_active_row[idx] (tau P (pc[r_next] - pc[idx]) - tau Q + mc[idx] P).
 * A graph may read fixed, advice, instance, challenge, constant, intermediate, theta and beta; gamma, y or the previous value is
 * H2HIP_EINVAL before any device work.  An argument's K + 1 graphs run as one kernel generated for them, or on the byte-code interpreter.
 * required_degree = 2 + d_t + sum_c d_c, each d the largest degree in that tuple, at least 1.  K_j in [1, 255], n_args <= 65535. */
typedef struct h2hip_evalh_mvlookups {
    uint32_t n_args;
    const uint32_t* n_inputs;
    const h2hip_graph* graphs;
    const uint64_t* const* phi_polys;
    const uint64_t* const* m_polys;
} h2hip_evalh_mvlookups;
/* evaluate_h with every argument that travels beside the descriptors; this family ends the growth of suffixes.  Either extra may be
 * NULL (or empty): mvlookups == NULL is the _shuffles call, both NULL the call without a suffix, limb for limb. */
int h2hip_evaluate_h_ext_bn254(const h2hip_evalh_desc* desc, const h2hip_evalh_mvlookups* mvlookups, const h2hip_evalh_shuffles* shuffles,
                               uint64_t* values);
int h2hip_evaluate_h_ext_bn254_device(const h2hip_evalh_desc* desc, const h2hip_evalh_mvlookups* mvlookups, const h2hip_evalh_shuffles* shuffles,
                                      void* d_values, void* stream);
int h2hip_evaluate_h_parts_ext_bn254(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_mvlookups* mvlookups,
                                     const h2hip_evalh_shuffles* shuffles, uint64_t* values);
int h2hip_evaluate_h_parts_ext_bn254_device(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_mvlookups* mvlookups,
                                            const h2hip_evalh_shuffles* shuffles, void* d_values, void* stream);
/* h2hip_evaluate_h_shuffles_workspace_bytes for a call with n_mvlookups mv-lookup arguments as well (0: the same number): the phi and m
 * cosets of one group of arguments come on top, and in the host parts form their coefficient columns */
int h2hip_evaluate_h_ext_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                         uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, uint32_t n_mvlookups,
                                         uint32_t n_shuffles, int parts_form, int device_form, size_t* bytes);

/* ---- pinned part cosets: the parts form's counterpart of h2hip_columns_pin.
 * Keep all P part cosets of each coefficient-form polynomial (2^k elements; pk.fixed_polys, pk.l0 / l_last / l_active_row as polynomials,
 * pk.permutation.polys) in HBM, 2^extended_k elements per polynomial, part-major, keyed by the pointer and the domain.
 * h2hip_evaluate_h_parts_bn254[_device] looks up fixed_polys, the three Lagrange polynomials and perm_polys; for a pinned one, part p is
 * read where the pin holds it: no upload, no scaling, no transform, no arena column.  Any subset may be pinned, and results are limb for
 * limb those of the unpinned call.
 * Host keys behave as h2hip_columns_pin's: idempotent; 16 sampled elements are compared with the caller's memory on every use, and on a
 * mismatch the entry is dropped and the call uploads and transforms as if nothing were pinned; HALO2_HIP_COLUMN_CACHE_GB and its LRU
 * are shared with the pinned columns; a polynomial larger than the budget is left unpinned.  The same pointer may also be pinned with
 * h2hip_columns_pin (elems = 2^k, for the opening calls): the two are separate entries.
 * Device keys: the device form never waits for its kernels, so no verdict could be read back.  Instead of a guard there is a contract: the
 * buffer stays alive and unchanged from the pin until h2hip_part_cosets_unpin.  The pin reads it on `stream` and returns when the entry
 * is built.
 * k <= extended_k <= 28, extended_k - k <= 8; count == 0 does nothing. */
int h2hip_part_cosets_pin(const uint64_t* const* polys, size_t count, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                          const uint64_t g_coset[4], const uint64_t g_coset_inv[4]);
int h2hip_part_cosets_pin_device(const void* const* d_polys, size_t count, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                                 const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* stream);
int h2hip_part_cosets_unpin(const void* const* polys, size_t count);       /* host or device keys; unknown pointers ignored */
int h2hip_part_cosets_pinned_info(size_t* n_polys, size_t* device_bytes);

/* ---- grand products: permutation::Argument::commit (plonk/permutation/prover.rs:96-166) and lookup::Permuted::commit_product
 * (plonk/lookup/prover.rs:194-249) -- the z columns create_proof builds between the advice commits and evaluate_h ----------------
 * n = 2^k, b = blinding_factors, u = n - b - 1; every column is 2^k Fr elements in Lagrange form.
 * Permutation: columns[c] = p_c (the permutation's columns, resolved from advice / fixed / instance), permutations[c] = pkey.permutations[c];
 * sets of chunk_len columns (the last may be shorter), n_sets = ceil(n_columns / chunk_len) outputs z[t]:
 *   z_t[0] = last_z (one for set 0), z_t[i] = z_t[i-1] * prod_c (p_c + beta delta^c omega^(i-1) + gamma) * inv(prod_c (p_c + beta s_c + gamma))
 *   at row i - 1 (c the global column index), rows n - b .. n - 1 = blinding[t * b ..], last_z = z_t[u] (computed, never a blinding row).
 * Lookups: z_j[0] = 1, z_j[i] = z_j[i-1] * (A + beta)(S + gamma) * inv((A' + beta)(S' + gamma)) at row i - 1, rows n - b .. = blinding[j * b ..].
 * inv is ff's BatchInvert: a zero denominator stays zero, so z is zero from the next row on.  The caller draws the blinding values (b per set
 * or lookup, in the reference's order); the engine draws no randomness.  k <= 28, chunk_len >= 1, b + 1 < n; n_columns == 0 / count == 0 write
 * nothing.  Host forms: a permutations[c] pinned with h2hip_columns_pin (elems = 2^k) is not uploaded.  _device forms: every column and output
 * is a device pointer (the pointer tables, scalars and blinding values are host memory, read before the call returns); kernels are queued on
 * `stream` and the call does not wait for them. */
int h2hip_permutation_products_bn254(uint32_t k, const uint64_t omega[4], const uint64_t delta[4], const uint64_t beta[4], const uint64_t gamma[4],
                                     const uint64_t* const* columns, const uint64_t* const* permutations, uint32_t n_columns, uint32_t chunk_len,
                                     const uint64_t* blinding, uint32_t blinding_factors, uint64_t* const* z);
int h2hip_permutation_products_bn254_device(uint32_t k, const uint64_t omega[4], const uint64_t delta[4], const uint64_t beta[4],
                                            const uint64_t gamma[4], const void* const* d_columns, const void* const* d_permutations,
                                            uint32_t n_columns, uint32_t chunk_len, const uint64_t* blinding, uint32_t blinding_factors,
                                            void* const* d_z, void* stream);
int h2hip_lookup_products_bn254(uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* const* compressed_input,
                                const uint64_t* const* compressed_table, const uint64_t* const* permuted_input,
                                const uint64_t* const* permuted_table, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                uint64_t* const* z);
int h2hip_lookup_products_bn254_device(uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const void* const* d_compressed_input,
                                       const void* const* d_compressed_table, const void* const* d_permuted_input,
                                       const void* const* d_permuted_table, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                       void* const* d_z, void* stream);
/* The shuffle argument's grand product (shuffle::Argument::commit_product of upstream PSE halo2, which is later than the reference this
 * engine follows: DESIGN.md section 2).  With A_j, S_j the compressed input and shuffle expressions of shuffle j -- the theta fold
 * h2hip_lookup_compress_bn254 computes -- z_j[0] = 1, z_j[i] = z_j[i-1] * (A_j + gamma) * inv(S_j + gamma) at row i - 1 for 1 <= i <= u,
 * rows n - b .. n - 1 = blinding[j * b ..].  inv is ff's BatchInvert as above: after a zero denominator z is zero.  A valid shuffle ends in
 * z[u] = 1; the engine does not check that.  Pointer tables, blinding order, the _device form and count == 0 are the lookup call's. */
int h2hip_shuffle_products_bn254(uint32_t k, const uint64_t gamma[4], const uint64_t* const* compressed_input,
                                 const uint64_t* const* compressed_shuffle, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                 uint64_t* const* z);
int h2hip_shuffle_products_bn254_device(uint32_t k, const uint64_t gamma[4], const void* const* d_compressed_input,
                                        const void* const* d_compressed_shuffle, size_t count, const uint64_t* blinding,
                                        uint32_t blinding_factors, void* const* d_z, void* stream);
/* The logarithmic-derivative lookup argument ("mv-lookup", logUp) of the upstream forks that replaced the permuted-column lookup.  It is
 * later than the reference this engine follows and its source is not part of this repository, so the definitions are stated here
 *  and a Python-integer model pins them (tests/mvlookup_util.py).  n = 2^k, b = blinding_factors, u = n - b - 1.
 * Argument j has K_j = n_inputs[j] >= 1 compressed input columns F_{j,0} .. F_{j,K_j-1} and one compressed table column T_j, each the
 * theta fold h2hip_lookup_compress_bn254 computes (one graph per column).  compressed_inputs is one flat table, argument-major:
 * F_{0,0} .. F_{0,K_0-1}, F_{1,0}, ...
 *
 * Multiplicities.  For i < u: M_j[i] = 0 if some i' < i has T_j[i'] = T_j[i]; otherwise the number of pairs (c, r), r < u, with
 * F_{j,c}[r] = T_j[i].  Rows u .. n - 1 are zero (no blinding rows go into m).  The output is Montgomery form, ready to commit.  Upstream
 * finds the table row by a binary search in a sorted list, so with repeated table values it is implementation-defined which row of a run
 * takes the count; this engine fixes the LOWEST row.  A proof is valid either way, but not byte-identical to a given upstream build when
 * a table repeats values.  If an input row r < u holds a value absent from T_j[0 .. u), every output is still written (the counts of the
 * values that were found) and the call returns H2HIP_ELOOKUP; h2hip_last_error() names the lowest failing (argument, input column).
 * The _device form queues on `stream` and waits for it once to read that verdict, as h2hip_lookup_permute_bn254_device does.
 * K_j in [1, 255] with K_j * 2^k < 2^32 (the counts are 32-bit), count <= 65535, blinding_factors + 1 < n; count == 0 writes nothing.
 *
 * Grand sum.  phi_j[0] = 0; for 1 <= i <= u: phi_j[i] = phi_j[i-1] + sum_c inv(F_{j,c}[i-1] + beta) - M_j[i-1] * inv(T_j[i-1] + beta);
 * rows n - b .. n - 1 = blinding[j * b ..], drawn by the caller in argument order.  inv is ff's BatchInvert, inv(0) = 0: that term is
 * zero and the sum simply goes on (no "zero from here on", unlike the products).  The whole call takes one field inversion.  A valid
 * argument ends in phi_j[u] = 0; the engine does not check that.  The (sum_j K_j + count) * 2^k denominators of a call must not
 * exceed 2^30.  The _device form queues on `stream` and does not wait. */
int h2hip_mvlookup_multiplicities_bn254(uint32_t k, const uint64_t* const* compressed_inputs, const uint32_t* n_inputs,
                                        const uint64_t* const* compressed_tables, size_t count, uint32_t blinding_factors, uint64_t* const* m);
int h2hip_mvlookup_multiplicities_bn254_device(uint32_t k, const void* const* d_compressed_inputs, const uint32_t* n_inputs,
                                               const void* const* d_compressed_tables, size_t count, uint32_t blinding_factors, void* const* d_m,
                                               void* stream);
int h2hip_mvlookup_sums_bn254(uint32_t k, const uint64_t beta[4], const uint64_t* const* compressed_inputs, const uint32_t* n_inputs,
                              const uint64_t* const* compressed_tables, const uint64_t* const* m, size_t count, const uint64_t* blinding,
                              uint32_t blinding_factors, uint64_t* const* phi);
int h2hip_mvlookup_sums_bn254_device(uint32_t k, const uint64_t beta[4], const void* const* d_compressed_inputs, const uint32_t* n_inputs,
                                     const void* const* d_compressed_tables, const void* const* d_m, size_t count, const uint64_t* blinding,
                                     uint32_t blinding_factors, void* const* d_phi, void* stream);
/* ff::BatchInvert (permutation/prover.rs:117, lookup/prover.rs:208): a[i] <- a[i]^-1 in place, zeros stay zero; n <= 2^30 */
int h2hip_batch_invert_bn254_fr(uint64_t* a, size_t n);
int h2hip_batch_invert_bn254_fr_device(void* d_a, size_t n, void* stream);

/* ---- lookup compression and permutation: lookup::Argument::commit_permuted (plonk/lookup/prover.rs:64-170), between the theta and the
 * beta squeeze of create_proof -------------------------------------------------------------------------------------------------------
 * n = 2^k, b = blinding_factors, u = n - b - 1 (usable_rows; here rows u .. n - 1, b + 1 of them, are blinding rows).
 * Compress (:90-115): out[g][i] = graph g evaluated at row i < n over the Lagrange columns fixed / advice / instance (2^k Fr elements
 * each), the challenges and theta, with rotations wrapping modulo n.  Graph g is GraphEvaluator::add_expression of each of a lookup's
 * input (or table) expressions, then Horner(Constant(0), parts, Theta) -- C = theta^(m-1) e_0 + ... + e_(m-1) (evaluation.py
 * lookup_compress_graphs).  A graph that reads beta, gamma, y or the previous value, or an index out of range, is H2HIP_EINVAL.
 * Permute (permute_expression_pair, :391-475), per lookup j: A' = compressed_input[0 .. u) sorted by Fr's Ord (the canonical integers);
 * S'[i] = A'[i] on the first row of each distinct value, taking one copy of it out of the multiset T = compressed_table[0 .. u); the
 * leftovers L (ascending) fill the repeated rows R (ascending) as S'[R[t]] = L[|L| - 1 - t].  blinding holds 2(b + 1) values per lookup,
 * A' rows u .. n - 1 then S' rows u .. n - 1, drawn by the caller in the reference's order; the engine draws nothing.  An input value
 * missing from its table is H2HIP_ELOOKUP: h2hip_last_error() names the lowest such lookup, and the outputs are unspecified;
 * h2hip_check_lookups_bn254 on the same compressed columns gives the failing rows of every lookup.
 * k <= 28, b + 1 < n (permute), count <= 32767, n_graphs <= 65535; n_graphs == 0 / count == 0 write nothing.  Host forms: a fixed column
 * pinned with h2hip_columns_pin (elems = 2^k) is not uploaded.  _device forms: columns and outputs are device pointers (the pointer tables,
 * graphs, challenges, theta and blinding values are host memory, read before the call returns) and kernels are queued on `stream`; the
 * compress call does not wait for them, the permute call synchronises `stream` once, to read the not-found flags. */
int h2hip_lookup_compress_bn254(uint32_t k, const uint64_t* const* fixed_values, uint32_t n_fixed, const uint64_t* const* advice_values,
                                uint32_t n_advice, const uint64_t* const* instance_values, uint32_t n_instance, const uint64_t* challenges,
                                uint32_t n_challenges, const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, uint64_t* const* out);
int h2hip_lookup_compress_bn254_device(uint32_t k, const void* const* d_fixed_values, uint32_t n_fixed, const void* const* d_advice_values,
                                       uint32_t n_advice, const void* const* d_instance_values, uint32_t n_instance, const uint64_t* challenges,
                                       uint32_t n_challenges, const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, void* const* d_out,
                                       void* stream);
int h2hip_lookup_permute_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_table, size_t count,
                               const uint64_t* blinding, uint32_t blinding_factors, uint64_t* const* permuted_input, uint64_t* const* permuted_table);
int h2hip_lookup_permute_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_table, size_t count,
                                      const uint64_t* blinding, uint32_t blinding_factors, void* const* d_permuted_input,
                                      void* const* d_permuted_table, void* stream);

/* ---- opening: the query evaluations and the KZG multiopen quotients that follow evaluate_h --------------------------------------
 * Evaluation (eval_polynomial, arithmetic.rs:304-328): evals[q] = polys[query_poly[q]] evaluated at points[q], for n_queries queries
 * (4 limbs each); polys[j] has lens[j] coefficients (0 evaluates to zero), query_poly[q] < n_polys.  Queries of one polynomial share
 * its reads.  Both forms write evals (host memory) before they return.
 * Combine (gwc/prover.rs:61-89, shplonk/prover.rs:26-31 and 138-275, vanishing/prover.rs:131-135, kate_division arithmetic.rs:348-366):
 *   a = sum_j scalars[j] polys[j] - sub      every polys[j] has len coefficients; sub: sub_len <= min(len, 16) low coefficients
 *   q = a, then q = kate_division(q, r) for each r of roots in order (n_roots <= 16; q has len - n_roots coefficients)
 *   out[0 .. len - n_roots) = scale q, out[len - n_roots .. out_len) = 0;  with accumulate = 1: out[0 .. len - n_roots) += scale q only.
 * remainder (4 limbs, host, or NULL) receives a(roots[0]) = a[0] + roots[0] q[0] of the first division (H2HIP_EINVAL without roots).
 * Scalars, sub, roots and scale are host memory and reduced Fr elements; len, lens and out_len <= 2^28, out_len >= len - n_roots.
 * n_polys == 0 / n_queries == 0 write nothing.  The engine draws no challenge and orders nothing: the caller passes the y / v powers,
 * the interpolant and the points as the reference computes them.  Host forms: a polynomial pinned with h2hip_columns_pin (elems = its
 * length) is not uploaded.  _device forms: polynomials and out are device pointers, out aliases no input (the accumulator is read when
 * accumulate is set); kernels are queued on `stream`; the evaluation synchronises (its results go to the transcript), the combine
 * does not unless it is asked for a remainder. */
int h2hip_eval_polynomials_bn254(const uint64_t* const* polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly, const uint64_t* points,
                                 size_t n_queries, uint64_t* evals);
int h2hip_eval_polynomials_bn254_device(const void* const* d_polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly,
                                        const uint64_t* points, size_t n_queries, uint64_t* evals, void* stream);
int h2hip_poly_combine_bn254_fr(const uint64_t* const* polys, size_t len, const uint64_t* scalars, size_t n_polys, const uint64_t* sub,
                                size_t sub_len, const uint64_t* roots, size_t n_roots, const uint64_t scale[4], uint32_t accumulate, uint64_t* out,
                                size_t out_len, uint64_t* remainder);
int h2hip_poly_combine_bn254_fr_device(const void* const* d_polys, size_t len, const uint64_t* scalars, size_t n_polys, const uint64_t* sub,
                                       size_t sub_len, const uint64_t* roots, size_t n_roots, const uint64_t scale[4], uint32_t accumulate,
                                       void* d_out, size_t out_len, uint64_t* remainder, void* stream);

/* ---- keygen: the data-parallel columns of keygen_vk / keygen_pk (plonk/keygen.rs:203-367, plonk/permutation/keygen.rs:105-242) and
 * batch_invert_assigned (poly.rs:180-209), which the prover also applies to every advice column (plonk/prover.rs:334) ------------------
 * n = 2^k; the domain constants are the EvaluationDomain's (poly/domain.rs:18-34), passed as h2hip_ifft_bn254_fr and
 * h2hip_coeff_to_extended_bn254_fr take them; k <= extended_k <= 28.
 * Permutation key (Assembly::build_vk :105-165, build_pk :167-242): mapping[j] is Assembly::mapping[j], 2^k (column, row) pairs as
 * interleaved uint32_t (8 bytes per cell), n_columns <= 65535.  Each of the three output tables holds n_columns pointers and may be NULL as a whole:
 *   permutations[j][i] = delta^c omega^r, (c, r) = mapping[j][i]      Lagrange form, 2^k elements (:111-151, :173-212);
 *   polys[j]  = lagrange_to_coeff(permutations[j])                   2^k elements (:214-223);
 *   cosets[j] = coeff_to_extended(polys[j])                          2^extended_k elements (:225-234).
 * With only permutations this is build_vk's table (its commitments are one h2hip_msm_bn254_batch over the pinned g_lagrange), with all
 * three build_pk.  Every element is the reduced Montgomery representative the reference stores.  A pair with column >= n_columns or
 * row >= 2^k is H2HIP_EINVAL: the host form finds it before any device work and names it; the _device form raises a flag in the kernel,
 * takes that cell's sigma value as zero, and synchronises `stream` once at the end of the call to read it.  After such a call permutations
 * is complete but for the zero at that cell, and polys / cosets are the transforms of that column with the zero in it: not a key.
 * n_columns == 0, or all three tables NULL, writes nothing.  Host form: only the mapping is uploaded; the columns are built, transformed
 * and downloaded in groups (bounded HBM whatever n_columns is), the download of one group under the work of the next.  _device form:
 * mapping[j] and the outputs are device pointers, no output aliases another or the mapping; the pointer tables and scalars are host
 * memory read before the call returns; kernels are queued on `stream`. */
int h2hip_permutation_keygen_bn254(uint32_t k, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t ifft_divisor[4],
                                   uint32_t extended_k, const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                   const uint64_t delta[4], const uint32_t* const* mapping, uint32_t n_columns, uint64_t* const* permutations,
                                   uint64_t* const* polys, uint64_t* const* cosets);
int h2hip_permutation_keygen_bn254_device(uint32_t k, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t ifft_divisor[4],
                                          uint32_t extended_k, const uint64_t extended_omega[4], const uint64_t g_coset[4],
                                          const uint64_t g_coset_inv[4], const uint64_t delta[4], const void* const* d_mapping, uint32_t n_columns,
                                          void* const* d_permutations, void* const* d_polys, void* const* d_cosets, void* stream);
/* batch_invert_assigned (poly.rs:180-209).  Rust's Assigned<F> has no stable layout, so per column j: numerators[j], 2^k elements (zero for
 * Zero, x for Trivial(x), the numerator for Rational); rat_rows[j], the rat_counts[j] strictly ascending row indices of its Rational cells;
 * rat_denoms[j], their denominators (rat_counts NULL, or a count of 0 with NULL arrays: no Rational cell).  out[j][i] = numerators[j][i],
 * except out[j][rat_rows[j][t]] = numerator * inv(rat_denoms[j][t]), where a zero denominator inverts to zero as ff's BatchInvert leaves it
 * (Assigned evaluates x / 0 to 0).  One inversion over the denominators of all columns together (:192-200; at most 2^30 of them).
 * out[j] may equal numerators[j].  Host form: rows out of range or not ascending and unreduced denominators are H2HIP_EINVAL; the
 * numerators are not examined, and a column without a Rational cell is copied on the host (its out[j] == numerators[j]: not touched) and
 * never crosses PCIe.  _device form: every array is a device pointer (the tables and rat_counts are host memory); the rows are
 * the caller's contract, an index >= 2^k is skipped; queued on `stream`, not waited for. */
int h2hip_batch_invert_assigned_bn254(uint32_t k, const uint64_t* const* numerators, const uint32_t* const* rat_rows, const size_t* rat_counts,
                                      const uint64_t* const* rat_denoms, size_t n_columns, uint64_t* const* out);
int h2hip_batch_invert_assigned_bn254_device(uint32_t k, const void* const* d_numerators, const void* const* d_rat_rows, const size_t* rat_counts,
                                             const void* const* d_rat_denoms, size_t n_columns, void* const* d_out, void* stream);
/* pk.l0, pk.l_last, pk.l_active_row (plonk/keygen.rs:320-351), 2^extended_k elements each: coeff_to_extended(lagrange_to_coeff(.)) of the
 * Lagrange columns e_0 and e_u (u = 2^k - blinding_factors - 1), and 1 - (l_last + l_blind) with l_blind the same transform of the column
 * that is one on the last blinding_factors rows (an intermediate, not returned).  blinding_factors + 1 < 2^k.  The _device form writes
 * three device buffers, queues on `stream` and does not wait. */
int h2hip_key_lagrange_columns_bn254(uint32_t k, const uint64_t omega_inv[4], const uint64_t ifft_divisor[4], uint32_t extended_k,
                                     const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                     uint32_t blinding_factors, uint64_t* l0, uint64_t* l_last, uint64_t* l_active_row);
int h2hip_key_lagrange_columns_bn254_device(uint32_t k, const uint64_t omega_inv[4], const uint64_t ifft_divisor[4], uint32_t extended_k,
                                            const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                            uint32_t blinding_factors, void* d_l0, void* d_l_last, void* d_l_active_row, void* stream);
/* Permutation mapping from copy constraints: the `mapping` that h2hip_permutation_keygen_bn254, h2hip_check_permutation_bn254 and their
 * _device forms take, built from the list of a circuit's copies instead of by Assembly::copy (plonk/permutation/keygen.rs:46-103), whose
 * result depends on the order of the calls and which is serial by construction.  The definition is later than the reference (upstream PSE
 * halo2's thread-safe-region assembly builds such an ordered mapping); it is stated here and pinned by tests/copies_util.py:
 *   cells are numbered id(c, r) = c 2^k + r, for c < n_columns and r < 2^k;
 *   a copy is four uint32_t (left_column, left_row, right_column, right_row), 16 bytes; the copies are the edges of a graph on the cells;
 *   for every cell x, mapping[c][r] is the cell of x's connected component with the least id greater than id(x), or, if there is none,
 *   the component's least cell;
 *   a cell that no copy touches maps to itself; self-copies and repeated copies change nothing;
 *   the result does not depend on the order of the copies or on which side of a copy is left.
 * The permutation has the same cycles (as sets of cells) as Assembly::copy produces for the same constraints, so any key built from it is
 * a valid key for the circuit: valid, not byte-identical -- it is not the reference's sigma polynomials or verifying key for that circuit,
 * and a prover and a verifier must both use keys from the same mapping.
 * mapping[j] receives 2^k interleaved (column, row) pairs, 8 bytes per cell.  k <= 28, n_columns <= 65535, n_columns 2^k <= 2^32 (cell
 * ids are 32-bit) and n_copies <= 2^30: beyond any of these the call returns H2HIP_EINVAL.  n_copies == 0 writes the identity;
 * n_columns == 0 writes nothing.  A copy with a column >= n_columns or a row >= 2^k is H2HIP_EINVAL: the host form finds it before any
 * device work and names the lowest offending copy index; the _device form ignores the bad copies, writes the mapping of the valid ones,
 * synchronises `stream` once at the end of the call to read its flag and returns H2HIP_EINVAL.  Host form: only the copies are uploaded
 * and the mapping is downloaded.  _device form: d_copies (16-byte aligned) and d_mapping[j] (8-byte aligned, else H2HIP_EINVAL; no column
 * aliases another or the copies) are device pointers, the pointer table is host memory read before the call returns, kernels are queued on `stream`. */
int h2hip_permutation_mapping(uint32_t k, uint32_t n_columns, const uint32_t* copies, size_t n_copies, uint32_t* const* mapping);
int h2hip_permutation_mapping_device(uint32_t k, uint32_t n_columns, const void* d_copies, size_t n_copies, void* const* d_mapping, void* stream);

/* ---- witness check: the three column-wide loops of MockProver::verify (dev.rs:603-1300) over the prover's own columns -----------------
 * n = 2^k, k <= 28.  Each call checks n_items constraints over the rows and reports, per constraint, how many rows fail and which are
 * the lowest: counts (host memory) receives one uint64_t per item; rows (host memory, n_items x max_rows uint32_t, item-major; may be
 * NULL when max_rows == 0; max_rows <= 65535) receives in rows[j][t], t < min(counts[j], max_rows), the lowest failing rows of item j in
 * ascending order, and UINT32_MAX in the remaining slots.  The result is a function of the inputs alone: two runs are byte-identical.
 * Failures are data: a call that finds some returns H2HIP_OK; a non-zero status is a contract violation or a device error.  Zero items
 * write nothing.  MockProver's regions, names, CellNotAssigned, Poison and selector checks are host bookkeeping and not done here.
 * Gates (:676-746): graphs[g] is GraphEvaluator::add_expression of ONE gate polynomial, its value designated by a closing Store
 * calculation (evaluation.py gate_check_graphs), so a bare query or a constant is a legal polynomial; an empty graph is the zero
 * polynomial.  Item g fails at row i when that value is non-zero at Lagrange row i, rotations wrapping modulo n.  ALL n rows are
 * checked, the blinding rows included (verify's default, and what divisibility by X^n - 1 demands): on the prover's real columns
 * those rows hold random values where MockProver holds Poison, and a gate that is not switched off there fails there.  n_graphs <=
 * 65535.  A graph that reads beta, gamma, theta, y or the previous value, or an index out of range, is H2HIP_EINVAL before any device work.
 * Permutation (:889-931): columns are the n_columns <= 65535 Lagrange columns of the argument, already resolved from advice / fixed /
 * instance as h2hip_permutation_products_bn254 takes them; mapping as h2hip_permutation_keygen_bn254 takes it.  Item j fails at row i
 * when columns[j][i] != columns[c][r], (c, r) = mapping[j][i]: equality of reduced elements, over all n rows.  A wrong cell in a cycle
 * of length >= 2 is therefore reported twice, at the cell and at its predecessor, as in the reference.  A pair with column >=
 * n_columns or row >= 2^k is H2HIP_EINVAL: the host form finds it before any device work and names it; the _device form checks the
 * bounds in the kernel, never dereferences the pair, raises a flag and returns H2HIP_EINVAL after its one synchronisation.
 * Lookups (:751-886): with u = n - blinding_factors - 1 (blinding_factors + 1 < n), lookup j fails at row i < u when
 * compressed_input[j][i] equals none of compressed_table[j][0 .. u).  Rows >= u are never reported and table rows >= u never satisfy
 * an input (:818-836).  count <= 32767.  The columns are what h2hip_lookup_compress_bn254 produces for a theta of the caller's
 * choosing: for single-expression lookups this is MockProver's check exactly; for tuples it is that check up to a theta collision
 * (two different tuples compressing to one value), which is the soundness the proof itself has.
 * Host forms upload their columns; one pinned with h2hip_columns_pin (elems = 2^k) is not uploaded.  _device forms: columns (and the
 * mapping) are device pointers, the pointer tables, graphs and challenges host memory read before the call returns; kernels are
 * queued on `stream`, which is synchronised once to deliver counts / rows (as h2hip_eval_polynomials_bn254_device does for its results). */
int h2hip_check_gates_bn254(uint32_t k, const uint64_t* const* fixed_values, uint32_t n_fixed, const uint64_t* const* advice_values,
                            uint32_t n_advice, const uint64_t* const* instance_values, uint32_t n_instance, const uint64_t* challenges,
                            uint32_t n_challenges, const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, uint64_t* counts, uint32_t* rows);
int h2hip_check_gates_bn254_device(uint32_t k, const void* const* d_fixed_values, uint32_t n_fixed, const void* const* d_advice_values,
                                   uint32_t n_advice, const void* const* d_instance_values, uint32_t n_instance, const uint64_t* challenges,
                                   uint32_t n_challenges, const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, uint64_t* counts,
                                   uint32_t* rows, void* stream);
int h2hip_check_permutation_bn254(uint32_t k, const uint64_t* const* columns, const uint32_t* const* mapping, uint32_t n_columns, uint32_t max_rows,
                                  uint64_t* counts, uint32_t* rows);
int h2hip_check_permutation_bn254_device(uint32_t k, const void* const* d_columns, const void* const* d_mapping, uint32_t n_columns,
                                         uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream);
int h2hip_check_lookups_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_table, size_t count,
                              uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows);
int h2hip_check_lookups_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_table, size_t count,
                                     uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream);
/* Shuffles (the argument of upstream PSE halo2): shuffle j fails at input row i < u when compressed_input[j][i]
 * occurs a different number of times among compressed_input[j][0 .. u) than among compressed_shuffle[j][0 .. u).  Rows >= u are never
 * reported and never counted.  Both multisets have u elements, so they differ exactly when some row fails.  Upstream's MockProver
 * reports the mismatching positions of the two sorted lists instead; this is the per-row form the counts / rows convention above needs.
 * blinding_factors + 1 < n, count <= 32767; the columns and the theta-collision caveat are those of the lookup check. */
int h2hip_check_shuffles_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_shuffle, size_t count,
                               uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows);
int h2hip_check_shuffles_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_shuffle, size_t count,
                                      uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream);

/* ---- serialisation: the per-element work of SerdeFormat (helpers.rs:8-20) in ParamsKZG::read_custom / write_custom
 * (poly/kzg/commitment.rs:142-244) and Polynomial::read / write (poly.rs:152-177) ------------------------------------------------------
 * n <= 2^30 elements, one GPU lane each; n == 0 succeeds and touches nothing but invalid[].  Byte buffers are plain bytes (no alignment
 * is asked of host memory).  Encodings (halo2curves 0.3.1 GroupEncoding / SerdePrimeField as DESIGN.md section 2 records them):
 *   compressed G1 : 32 B, canonical (non-Montgomery) x little-endian, bit 7 of byte 31 = the low bit of canonical y; identity = 32 zero bytes
 *   Fr repr       : 32 B, the canonical integer little-endian
 * g1_decompress (SerdeFormat::Processed read, helpers.rs:36-40): points[i] = x || y, 64 B Montgomery.  An encoding is invalid when
 * x >= q (bit 254 set included), when x^3 + 3 is not a square, or when it is x = 0 with the sign bit set.
 * g1_compress (Processed write, helpers.rs:49-57) is the inverse; (0, 0) gives 32 zero bytes.  Points are taken as reduced and on the curve.
 * g1_validate (SerdeFormat::RawBytes read, read_raw): a point is invalid unless both coordinates are below q and it is (0, 0) or
 * satisfies y^2 = x^3 + 3.
 * fr_from_repr / fr_to_repr (SerdePrimeField, helpers.rs:61-93): canonical integer <-> Montgomery form; a value >= r is invalid.  The
 * output may be the input buffer.
 * The three fallible calls write ALL of their output -- an invalid element as zero bytes -- and invalid[] (host memory) =
 * {number of invalid elements, lowest invalid index} ({0, 0} when there is none), a function of the input alone; they return
 * H2HIP_EENCODING exactly when invalid[0] > 0.  Host forms upload, convert and download on the engine's stream.  _device forms take
 * device pointers and queue on `stream`; the fallible ones synchronise it once to deliver invalid[] (as the witness check does for its
 * counts), g1_compress / fr_to_repr return with their kernel queued. */
int h2hip_g1_decompress_bn254(const void* bytes, size_t n, uint64_t* points_xy, uint64_t invalid[2]);
int h2hip_g1_decompress_bn254_device(const void* d_bytes, size_t n, void* d_points_xy, uint64_t invalid[2], void* stream);
int h2hip_g1_compress_bn254(const uint64_t* points_xy, size_t n, void* bytes);
int h2hip_g1_compress_bn254_device(const void* d_points_xy, size_t n, void* d_bytes, void* stream);
int h2hip_g1_validate_bn254(const uint64_t* points_xy, size_t n, uint64_t invalid[2]);
int h2hip_g1_validate_bn254_device(const void* d_points_xy, size_t n, uint64_t invalid[2], void* stream);
int h2hip_fr_from_repr_bn254(const void* repr, size_t n, uint64_t* out, uint64_t invalid[2]);
int h2hip_fr_from_repr_bn254_device(const void* d_repr, size_t n, void* d_out, uint64_t invalid[2], void* stream);
int h2hip_fr_to_repr_bn254(const uint64_t* in, size_t n, void* repr);
int h2hip_fr_to_repr_bn254_device(const void* d_in, size_t n, void* d_repr, void* stream);

/* ---- randomness: C::Scalar::random over a whole column, the loop of vanishing::Argument::commit (plonk/vanishing/prover.rs:49-58) ------
 * Definitions (halo2curves 0.3.1 and rand_chacha 0.3 as DESIGN.md section 2 records them):
 *   Fr::from_bytes_wide : the 64 bytes read as one little-endian 512-bit integer, reduced mod r; Fr::random = that map on eight next_u64
 *   ChaCha20Rng::from_seed(seed) : 20 rounds, key = seed, state words 12-13 = 64-bit block counter from 0, words 14-15 = 64-bit stream id
 * One Fr::random consumes exactly one 64-byte block, so
 *   fr_random : out[i] = from_bytes_wide(ChaCha20 block (first_block + i) of (seed, stream_id)),  4 x u64 Montgomery limbs,
 * limb for limb what the reference's loop stores when it is handed ChaCha20Rng::from_seed(seed) that has made first_block draws.  The
 * generator is counter-based: any range in any order, in one call or several.  fr_from_bytes_wide is the reduction alone over n
 * 64-byte strings (out must not overlap bytes).
 * THE SEED IS AS SECRET AS THE POLYNOMIAL: whoever learns it learns every element.  The engine is a deterministic expander and adds no
 * entropy; the 32 seed bytes are the caller's, from the rng the reference would have drawn the elements from.  The library wipes its
 * own host copies of the key before a call returns (the kernel receives it as an argument).
 * n <= 2^32; n == 0 returns 0 and touches nothing.  H2HIP_EINVAL: a null seed, input or output with n > 0; first_block + n > 2^64; a
 * device pointer that is not 16-byte aligned.  Host forms run the per-element code on the calling thread below HALO2_HIP_RANDOM_MIN_N
 * elements (default 2^9; no GPU is needed or touched: blinding scalars and blinding rows are a handful of draws) and from there on
 * generate on the device and download.  _device forms queue their kernel on `stream` and do not wait. */
int h2hip_fr_random_bn254(const uint8_t seed[32], uint64_t stream_id, uint64_t first_block, size_t n, uint64_t* out);
int h2hip_fr_random_bn254_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first_block, size_t n, void* d_out, void* stream);
int h2hip_fr_from_bytes_wide_bn254(const uint8_t* bytes /* n x 64 */, size_t n, uint64_t* out);
int h2hip_fr_from_bytes_wide_bn254_device(const void* d_bytes, size_t n, void* d_out, void* stream);

/* ---- synthetic workload; same streams as oracle_gen_{scalars,points} ---- */

int h2hip_gen_scalars_device(uint64_t seed, uint64_t start, size_t n, void* d_out, void* stream);
int h2hip_gen_points_device(uint64_t seed, uint64_t start, size_t n, void* d_out, void* stream);

/* ---- tuning and measurement ----------------------------------------------------------------- */

/* MSM window width in bits (2..24); 0 restores the size-based default.  Applies to the plain form at once
 * and to window tables built by later h2hip_bases_pin* calls. */
int h2hip_set_msm_window(uint32_t c);
/* window width the engine would use for n pairs: plain form / a window table over n pinned points */
uint32_t h2hip_get_msm_window(size_t n);
uint32_t h2hip_get_msm_window_fixed_base(size_t n);
/* Per-stage HIP-event timers recorded on the stream each kernel group is launched on.
 * Stages: "ntt", "msm_total", "msm_digits", "msm_sort", "msm_accum" (over-full buckets included), "msm_reduce", "g_to_lagrange", "kzg_setup",
 * "evalh_cosets", "evalh_gates", "evalh_perm", "evalh_lookups", "evalh_part_scale" (inside "evalh_cosets") and "evalh_part_io" (the parts form), "products", "opening_eval", "opening_combine", "lookup_compress",
 * "lookup_permute", "check_gates", "check_permutation", "check_lookups" (each check: its kernels, without the delivery of counts / rows),
 * "g1_decompress", "g1_validate", "fr_from_repr" (each with its failure count; the _device forms too), "g1_compress", "fr_to_repr" (host forms),
 * "fr_random", "fr_from_wide" (the _device forms, and the host forms from their threshold on), "copies_components", "copies_sort",
 * "copies_scatter" (the three parts of h2hip_permutation_mapping[_device]). */
/* on = 1: every stage (each event record costs the stream ~10 us of gap); on = 2: only the dominant kernel ("msm_accum"),
 * timed through its own dispatch packet with no gap; 0: off */
int h2hip_profile_enable(int on);
int h2hip_profile_reset(void);
int h2hip_profile_get(const char* stage, double* total_ms, uint64_t* count);

/* Test and tuning hooks (h2hip_debug_*) are declared in halo2hip_debug.h; they are not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* HALO2HIP_H */
