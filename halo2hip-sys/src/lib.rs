//! halo2hip-sys -- the `unsafe` half of the drop-in: halo2_proofs forbids unsafe code (`halo2_proofs/src/lib.rs:23`), so
//! the `extern "C"` block for libhalo2hip.so (include/halo2hip.h) and the reinterpretation of halo2curves' types as limb
//! arrays live here.  halo2_proofs gains two dispatch lines (patches/0001-arithmetic-dispatch.patch):
//!
//! ```ignore
//! if let Some(r) = halo2hip_sys::try_multiexp::<C>(coeffs, bases) { return r; }   // best_multiexp, arithmetic.rs:133
//! if halo2hip_sys::try_fft(a, &omega, log_n) { return; }                          // best_fft,      arithmetic.rs:184
//! ```
//!
//! Every wrapper returns `None` / `false` when the engine does not take the call (another curve, a size below the
//! threshold, no GPU, any non-zero status): the caller then runs the original CPU body.  Nothing panics or unwinds across
//! the FFI boundary.
//!
//! Not compiled in the repository that ships it (its build image has no Rust toolchain): `tests/test_binding.py` checks the
//! extern block against the header and the shared library, and that the patches apply to the reference tree.
#![allow(non_camel_case_types)]
#![allow(clippy::missing_safety_doc)]

pub mod evalh;
pub mod ffi;
mod ffi_g1;
mod ffi_ipa;
mod ffi_ipa_round;
mod ffi_pairing;
pub mod g1;
pub mod ipa;
pub mod ipa_round;
pub mod pairing;

use ff::{Field, PrimeField};
use halo2curves::bn256::{Fr, G1Affine, G1};
use halo2curves::CurveAffine;
use std::any::TypeId;
use std::sync::atomic::{AtomicU8, Ordering};

pub const H2HIP_OK: i32 = 0;
pub const H2HIP_EINVAL: i32 = 1;
pub const H2HIP_EDEVICE: i32 = 2;
pub const H2HIP_ENOMEM: i32 = 3;
/// a lookup's input holds a value its table lacks: the reference's `Error::ConstraintSystemFailure`
pub const H2HIP_ELOOKUP: i32 = 4;

/// Initialise the engine on the given GPUs (one context, stream and worker thread each; host-pointer MSMs shard over
/// them).  Optional: the first call initialises lazily on the current device, or on `HALO2_HIP_DEVICES`.
pub fn init(device_ids: &[i32]) -> Result<(), String> {
    let rc = unsafe { ffi::h2hip_init(device_ids.as_ptr(), device_ids.len() as i32) };
    if rc == 0 {
        Ok(())
    } else {
        Err(last_error())
    }
}

pub fn shutdown() {
    unsafe { ffi::h2hip_shutdown() }
}

pub fn last_error() -> String {
    unsafe { std::ffi::CStr::from_ptr(ffi::h2hip_last_error()) }.to_string_lossy().into_owned()
}

/// The layout the engine assumes, checked once per process: `Fr` = 4 x u64 Montgomery limbs, `G1Affine` = x || y with the
/// identity as (0, 0), `G1` = x || y || z.  halo2curves' types are not `#[repr(C)]`; `SerdeObject::to_raw_bytes` is the
/// layout-defined view ("uncompressed, internal Montgomery representation", halo2_proofs/src/helpers.rs:13-19), so the
/// in-memory bytes of a few values are compared with it.
fn layout_ok() -> bool {
    // 0 = not checked yet, 1 = ok, 2 = mismatch.  An atomic rather than `static mut` (a hard error under the 2024 edition's
    // static_mut_refs lint) or OnceLock (Rust 1.70; the reference's toolchain pin is older).  Two threads may both run the check
    // the first time; they store the same answer.
    static STATE: AtomicU8 = AtomicU8::new(0);
    match STATE.load(Ordering::Acquire) {
        1 => return true,
        2 => return false,
        _ => {}
    }
    use halo2curves::serde::SerdeObject;
    let mut ok = std::mem::size_of::<Fr>() == 32 && std::mem::size_of::<G1Affine>() == 64 && std::mem::size_of::<G1>() == 96;
    if ok {
        let raw_of = |p: *const u8, n: usize| unsafe { std::slice::from_raw_parts(p, n) }.to_vec();
        let two = Fr::one() + Fr::one();
        ok &= raw_of(&two as *const Fr as *const u8, 32) == two.to_raw_bytes();
        let g = G1Affine::generator();
        ok &= raw_of(&g as *const G1Affine as *const u8, 64) == g.to_raw_bytes();
        let id = G1Affine::default();
        ok &= raw_of(&id as *const G1Affine as *const u8, 64) == vec![0u8; 64];
    }
    STATE.store(if ok { 1 } else { 2 }, Ordering::Release);
    ok
}

fn is<A: 'static, B: 'static>() -> bool {
    TypeId::of::<A>() == TypeId::of::<B>()
}

/// `best_multiexp` on the GPU: `Some(sum)` when the engine took the call.
pub fn try_multiexp<C: CurveAffine>(coeffs: &[C::Scalar], bases: &[C]) -> Option<C::Curve> {
    if !is::<C, G1Affine>() || coeffs.len() != bases.len() || coeffs.len() < unsafe { ffi::h2hip_msm_min_n() } || !layout_ok() {
        return None;
    }
    let mut out = [0u64; 12];
    let rc = unsafe { ffi::h2hip_msm_bn254(coeffs.as_ptr() as *const u64, bases.as_ptr() as *const u64, coeffs.len(), out.as_mut_ptr()) };
    if rc != 0 || std::mem::size_of::<C::Curve>() != 96 {
        return None;
    }
    Some(unsafe { std::mem::transmute_copy::<[u64; 12], C::Curve>(&out) }) // C::Curve = G1 = (x, y, z)
}

/// `count` commitments over the same bases in one call (the advice-column loop of plonk/prover.rs:361-365).
pub fn try_multiexp_batch<C: CurveAffine>(columns: &[&[C::Scalar]], bases: &[C]) -> Option<Vec<C::Curve>> {
    if !is::<C, G1Affine>() || columns.is_empty() || !layout_ok() || std::mem::size_of::<C::Curve>() != 96 {
        return None;
    }
    let n = columns[0].len();
    if n > bases.len() || columns.iter().any(|c| c.len() != n) {
        return None;
    }
    let ptrs: Vec<*const u64> = columns.iter().map(|c| c.as_ptr() as *const u64).collect();
    let mut out = vec![[0u64; 12]; columns.len()];
    let rc = unsafe { ffi::h2hip_msm_bn254_batch(ptrs.as_ptr(), bases.as_ptr() as *const u64, n, columns.len(), out.as_mut_ptr() as *mut u64) };
    if rc != 0 {
        return None;
    }
    Some(out.iter().map(|o| unsafe { std::mem::transmute_copy::<[u64; 12], C::Curve>(o) }).collect())
}

/// `best_fft` on the GPU (G = bn256::Fr, or G = bn256::G1 for the curve-point FFT): true when the engine took the call (`a` then holds the transform).
/// Parity is defined for `omega` of exact order 2^log_n (every in-crate caller); anything else keeps the CPU body.
pub fn try_fft<G: 'static, S: 'static>(a: &mut [G], omega: &S, log_n: u32) -> bool {
    if log_n >= usize::BITS || a.len() != 1usize << log_n {
        return false;
    }
    if is::<G, G1>() {
        // best_fft over curve points (g_to_lagrange, arithmetic.rs:285): one 254-bit scalar multiplication per butterfly
        return match fft_guards::<Fr, S>(omega, log_n) {
            Some(w) => unsafe { ffi::h2hip_fft_bn254_g1(a.as_mut_ptr() as *mut u64, w as *const Fr as *const u64, log_n) == 0 },
            None => false,
        };
    }
    match fft_guards::<G, S>(omega, log_n) {
        Some(w) => unsafe { ffi::h2hip_ntt_bn254_fr(a.as_mut_ptr() as *mut u64, w as *const Fr as *const u64, log_n) == 0 },
        None => false,
    }
}

/// Keep `bases` (a `ParamsKZG`'s `g` or `g_lagrange`) on the GPU with its fixed-base window table until `unpin_bases`.
/// Keyed by the slice's address; a no-op for other curves.  Returns whether the engine holds the array now.
pub fn pin_bases<C: 'static>(bases: &[C]) -> bool {
    if !is::<C, G1Affine>() || bases.is_empty() || !layout_ok() {
        return false;
    }
    unsafe { ffi::h2hip_bases_pin(bases.as_ptr() as *const u64, bases.len()) == 0 }
}

/// Drop a pinned array (before its `Vec` is freed or rewritten).  Harmless when the array was never pinned.
pub fn unpin_bases<C: 'static>(bases: &[C]) {
    if is::<C, G1Affine>() && !bases.is_empty() {
        unsafe { ffi::h2hip_bases_unpin(bases.as_ptr() as *const std::os::raw::c_void) };
    }
}

/// `g_to_lagrange` (arithmetic.rs:277-301) for `ParamsKZG::downsize`: affine in, affine out.
pub fn try_g_to_lagrange<C: CurveAffine>(g: &[C], k: u32) -> Option<Vec<C>> {
    if !is::<C, G1Affine>() || g.len() != 1usize << k || !layout_ok() {
        return None;
    }
    let mut out = vec![C::identity(); g.len()];
    let rc = unsafe { ffi::h2hip_g_to_lagrange_bn254(g.as_ptr() as *const u64, k, out.as_mut_ptr() as *mut u64) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// Whether the engine takes a transform of 2^log_n elements of `G` at all (callers that would allocate for the engine ask first).
pub fn takes_fft<G: 'static>(log_n: u32) -> bool {
    is::<G, Fr>() && log_n != 0 && log_n <= Fr::S && log_n >= unsafe { ffi::h2hip_ntt_min_log_n() } && layout_ok()
}

/// The guards `try_fft` applies, for every transform wrapper: G = S = bn256::Fr, 1 <= log_n <= Fr::S and at least the engine's
/// threshold, and `omega` of exact order 2^log_n (the engine's parity is defined for nothing else; the C side rejects a
/// non-reduced element but cannot know the order the caller meant).
fn fft_guards<G: 'static, S: 'static>(omega: &S, log_n: u32) -> Option<&Fr> {
    if !is::<S, Fr>() || !takes_fft::<G>(log_n) {
        return None;
    }
    let w: &Fr = unsafe { &*(omega as *const S as *const Fr) };
    if w.pow_vartime(&[1u64 << (log_n - 1)]) != -Fr::one() {
        return None;
    }
    Some(w)
}

fn fr_ptr<S>(x: &S) -> *const u64 {
    x as *const S as *const u64
}

/// `EvaluationDomain::ifft` (poly/domain.rs:353-361) in one device round trip: NTT with `omega_inv`, scaled by `divisor`.
pub fn try_ifft<G: 'static, S: 'static>(a: &mut [G], omega_inv: &S, log_n: u32, divisor: &S) -> bool {
    if log_n >= usize::BITS || a.len() != 1usize << log_n || fft_guards::<G, S>(omega_inv, log_n).is_none() {
        return false;
    }
    unsafe { ffi::h2hip_ifft_bn254_fr(a.as_mut_ptr() as *mut u64, fr_ptr(omega_inv), log_n, fr_ptr(divisor)) == 0 }
}

/// `ifft` for several columns of one size in one call: upload i + 1, transform i and download i - 1 overlap (h2hip_ifft_bn254_fr_batch).
pub fn try_ifft_batch<G: 'static, S: 'static>(columns: &mut [&mut [G]], omega_inv: &S, log_n: u32, divisor: &S) -> bool {
    if columns.is_empty() || log_n >= usize::BITS || columns.iter().any(|c| c.len() != 1usize << log_n) || fft_guards::<G, S>(omega_inv, log_n).is_none() {
        return false;
    }
    let ptrs: Vec<*mut u64> = columns.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    unsafe { ffi::h2hip_ifft_bn254_fr_batch(ptrs.as_ptr(), ptrs.len(), fr_ptr(omega_inv), log_n, fr_ptr(divisor)) == 0 }
}

/// `EvaluationDomain::coeff_to_extended` (poly/domain.rs:240-254): zero-pad, distribute powers of zeta, extended NTT.
/// `a` holds 2^k coefficients, `out` receives 2^extended_k evaluations.
pub fn try_coeff_to_extended<G: 'static, S: 'static>(a: &[G], k: u32, out: &mut [G], extended_k: u32, extended_omega: &S, g_coset: &S, g_coset_inv: &S) -> bool {
    if k > extended_k || extended_k >= usize::BITS || a.len() != 1usize << k || out.len() != 1usize << extended_k {
        return false;
    }
    if fft_guards::<G, S>(extended_omega, extended_k).is_none() {
        return false;
    }
    unsafe {
        ffi::h2hip_coeff_to_extended_bn254_fr(a.as_ptr() as *const u64, k, out.as_mut_ptr() as *mut u64, extended_k, fr_ptr(extended_omega), fr_ptr(g_coset), fr_ptr(g_coset_inv)) == 0
    }
}

/// The same in place, as the reference does it: `a` has been resized to 2^extended_k elements, of which the first 2^k are the
/// coefficients (the engine reads only those and writes all 2^extended_k).
pub fn try_coeff_to_extended_in_place<G: 'static, S: 'static>(a: &mut [G], k: u32, extended_k: u32, extended_omega: &S, g_coset: &S, g_coset_inv: &S) -> bool {
    if k > extended_k || extended_k >= usize::BITS || a.len() != 1usize << extended_k || fft_guards::<G, S>(extended_omega, extended_k).is_none() {
        return false;
    }
    let p = a.as_mut_ptr() as *mut u64;
    unsafe { ffi::h2hip_coeff_to_extended_bn254_fr(p as *const u64, k, p, extended_k, fr_ptr(extended_omega), fr_ptr(g_coset), fr_ptr(g_coset_inv)) == 0 }
}

/// Upstream halo2's `coeff_to_extended_part`: rows `j * P + part` (P = 2^(extended_k - k)) of `coeff_to_extended(a)`; `a` and `out` hold
/// 2^k elements each.  The coset scaling is fused into the transform's first pass.
#[allow(clippy::too_many_arguments)]
pub fn try_coeff_to_extended_part<G: 'static, S: 'static>(a: &[G], k: u32, extended_k: u32, part: u32, extended_omega: &S, g_coset: &S, g_coset_inv: &S, out: &mut [G]) -> bool {
    if k > extended_k || extended_k >= usize::BITS || a.len() != 1usize << k || out.len() != 1usize << k || (part >> (extended_k - k)) != 0 {
        return false;
    }
    if fft_guards::<G, S>(extended_omega, extended_k).is_none() {
        return false;
    }
    unsafe {
        ffi::h2hip_coeff_to_extended_part_bn254_fr(a.as_ptr() as *const u64, k, extended_k, part, fr_ptr(extended_omega), fr_ptr(g_coset), fr_ptr(g_coset_inv), out.as_mut_ptr() as *mut u64) == 0
    }
}

/// Keep all P part cosets of a proving key's coefficient-form polynomials (`pk.fixed_polys`, `pk.l0` / `l_last` / `l_active_row` as
/// polynomials, `pk.permutation.polys`; 2^k elements each) in HBM for `try_evaluate_h_parts`: idempotent, fingerprint-guarded like the
/// pinned columns, and sharing their budget.  `false` only means the polynomials are transformed per call.  Call `part_cosets_unpin`
/// before the `Vec`s are freed (`ProvingKey`'s `Drop`).
pub fn try_part_cosets_pin<F: 'static, S: 'static>(polys: &[&[F]], k: u32, extended_k: u32, extended_omega: &S, g_coset: &S, g_coset_inv: &S) -> bool {
    if !is::<F, Fr>() || !is::<S, Fr>() || polys.is_empty() || k > extended_k || extended_k >= usize::BITS || polys.iter().any(|c| c.len() != 1usize << k) {
        return false;
    }
    let ptrs: Vec<*const u64> = polys.iter().map(|c| c.as_ptr() as *const u64).collect();
    unsafe { ffi::h2hip_part_cosets_pin(ptrs.as_ptr(), ptrs.len(), k, extended_k, fr_ptr(extended_omega), fr_ptr(g_coset), fr_ptr(g_coset_inv)) == 0 }
}

/// Release the part cosets `try_part_cosets_pin` keeps (unknown pointers are ignored, other element types are a no-op).
pub fn part_cosets_unpin<F: 'static>(polys: &[&[F]]) {
    if !is::<F, Fr>() || polys.is_empty() {
        return;
    }
    let ptrs: Vec<*const std::os::raw::c_void> = polys.iter().map(|c| c.as_ptr() as *const std::os::raw::c_void).collect();
    unsafe { ffi::h2hip_part_cosets_unpin(ptrs.as_ptr(), ptrs.len()) };
}

/// `coeff_to_extended` for several polynomials in one pipelined call (plonk/evaluation.rs:306-323 extends every advice and
/// instance column): `a[i]` holds 2^k coefficients, `out[i]` receives 2^extended_k evaluations.
pub fn try_coeff_to_extended_batch<G: 'static, S: 'static>(a: &[&[G]], k: u32, out: &mut [&mut [G]], extended_k: u32, extended_omega: &S, g_coset: &S, g_coset_inv: &S) -> bool {
    if a.is_empty() || a.len() != out.len() || k > extended_k || extended_k >= usize::BITS {
        return false;
    }
    if a.iter().any(|c| c.len() != 1usize << k) || out.iter().any(|c| c.len() != 1usize << extended_k) || fft_guards::<G, S>(extended_omega, extended_k).is_none() {
        return false;
    }
    let ins: Vec<*const u64> = a.iter().map(|c| c.as_ptr() as *const u64).collect();
    let outs: Vec<*mut u64> = out.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    unsafe {
        ffi::h2hip_coeff_to_extended_bn254_fr_batch(ins.as_ptr(), k, outs.as_ptr(), ins.len(), extended_k, fr_ptr(extended_omega), fr_ptr(g_coset), fr_ptr(g_coset_inv)) == 0
    }
}

/// `EvaluationDomain::extended_to_coeff` (poly/domain.rs:281-303) before its `truncate`.
pub fn try_extended_to_coeff<G: 'static, S: 'static>(a: &mut [G], extended_k: u32, extended_omega_inv: &S, extended_ifft_divisor: &S, g_coset: &S, g_coset_inv: &S) -> bool {
    if extended_k >= usize::BITS || a.len() != 1usize << extended_k || fft_guards::<G, S>(extended_omega_inv, extended_k).is_none() {
        return false;
    }
    unsafe {
        ffi::h2hip_extended_to_coeff_bn254_fr(a.as_mut_ptr() as *mut u64, extended_k, fr_ptr(extended_omega_inv), fr_ptr(extended_ifft_divisor), fr_ptr(g_coset), fr_ptr(g_coset_inv)) == 0
    }
}

/// `permutation::Argument::commit`'s z columns (plonk/permutation/prover.rs:96-166) for every set in one call: `columns[c]` are the
/// permutation's columns resolved from advice / fixed / instance, `permutations[c]` is `pkey.permutations[c]`, `blinding` the
/// `blinding_factors` values of each set, set-major, drawn by the caller in the reference's rng order.
/// `Some(z)` (one column per set) when the engine took the call; `None` for any other field, shape or engine failure.
#[allow(clippy::too_many_arguments)]
pub fn try_permutation_products<F: Field + 'static>(k: u32, omega: &F, delta: &F, beta: &F, gamma: &F, columns: &[&[F]], permutations: &[&[F]],
                                                    chunk_len: usize, blinding: &[F], blinding_factors: usize) -> Option<Vec<Vec<F>>> {
    if !is::<F, Fr>() || !layout_ok() || k > 28 || chunk_len == 0 || columns.len() != permutations.len() || chunk_len > u32::MAX as usize {
        return None;
    }
    let n = 1usize << k;
    let n_sets = (columns.len() + chunk_len - 1) / chunk_len;
    if columns.iter().chain(permutations.iter()).any(|c| c.len() != n) || blinding.len() != n_sets * blinding_factors || blinding_factors + 1 >= n {
        return None;
    }
    let p: Vec<*const u64> = columns.iter().map(|c| c.as_ptr() as *const u64).collect();
    let s: Vec<*const u64> = permutations.iter().map(|c| c.as_ptr() as *const u64).collect();
    let mut z: Vec<Vec<F>> = (0..n_sets).map(|_| vec![F::zero(); n]).collect();
    let zp: Vec<*mut u64> = z.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_permutation_products_bn254(k, fr_ptr(omega), fr_ptr(delta), fr_ptr(beta), fr_ptr(gamma), p.as_ptr(), s.as_ptr(), p.len() as u32,
                                              chunk_len as u32, blinding.as_ptr() as *const u64, blinding_factors as u32, zp.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(z)
}

/// `lookup::Permuted::commit_product`'s z columns (plonk/lookup/prover.rs:194-249) for several lookups in one call: the compressed
/// input / table expressions and the permuted columns of each lookup, `blinding` lookup-major.  `None` on any failure.
#[allow(clippy::too_many_arguments)]
pub fn try_lookup_products<F: Field + 'static>(k: u32, beta: &F, gamma: &F, compressed_inputs: &[&[F]], compressed_tables: &[&[F]],
                                               permuted_inputs: &[&[F]], permuted_tables: &[&[F]], blinding: &[F],
                                               blinding_factors: usize) -> Option<Vec<Vec<F>>> {
    let count = compressed_inputs.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || compressed_tables.len() != count || permuted_inputs.len() != count || permuted_tables.len() != count {
        return None;
    }
    let n = 1usize << k;
    let all = compressed_inputs.iter().chain(compressed_tables.iter()).chain(permuted_inputs.iter()).chain(permuted_tables.iter());
    if all.clone().any(|c| c.len() != n) || blinding.len() != count * blinding_factors || blinding_factors + 1 >= n {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (a, s, ap, sp) = (ptrs(compressed_inputs), ptrs(compressed_tables), ptrs(permuted_inputs), ptrs(permuted_tables));
    let mut z: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let zp: Vec<*mut u64> = z.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_lookup_products_bn254(k, fr_ptr(beta), fr_ptr(gamma), a.as_ptr(), s.as_ptr(), ap.as_ptr(), sp.as_ptr(), count,
                                         blinding.as_ptr() as *const u64, blinding_factors as u32, zp.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(z)
}

/// The shuffle argument's z columns (`shuffle::Argument::commit_product` of upstream PSE halo2, later than the reference; the
/// definition is include/halo2hip.h's) for several shuffles in one call: the compressed input and shuffle expressions of each, as
/// `try_lookup_compress` folds them, `blinding` shuffle-major.  `None` on any failure.
pub fn try_shuffle_products<F: Field + 'static>(k: u32, gamma: &F, compressed_inputs: &[&[F]], compressed_shuffles: &[&[F]], blinding: &[F],
                                                blinding_factors: usize) -> Option<Vec<Vec<F>>> {
    let count = compressed_inputs.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || compressed_shuffles.len() != count {
        return None;
    }
    let n = 1usize << k;
    if compressed_inputs.iter().chain(compressed_shuffles.iter()).any(|c| c.len() != n) || blinding.len() != count * blinding_factors || blinding_factors + 1 >= n {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (a, s) = (ptrs(compressed_inputs), ptrs(compressed_shuffles));
    let mut z: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let zp: Vec<*mut u64> = z.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_shuffle_products_bn254(k, fr_ptr(gamma), a.as_ptr(), s.as_ptr(), count, blinding.as_ptr() as *const u64, blinding_factors as u32,
                                          zp.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(z)
}

/// The logUp (mv-lookup) argument's multiplicity columns (the definition is include/halo2hip.h's): `compressed_inputs[j]` holds the
/// compressed input columns of argument j, which share `compressed_tables[j]`.  The count of a value goes to the lowest table row that
/// holds it.  `None` on any failure, a value missing from its table (`H2HIP_ELOOKUP`) included.
pub fn try_mvlookup_multiplicities<F: Field + 'static>(k: u32, compressed_inputs: &[&[&[F]]], compressed_tables: &[&[F]],
                                                       blinding_factors: usize) -> Option<Vec<Vec<F>>> {
    let count = compressed_tables.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || count > 65535 || compressed_inputs.len() != count {
        return None;
    }
    let n = 1usize << k;
    if compressed_inputs.iter().any(|cols| cols.is_empty() || cols.len() > 255 || cols.iter().any(|c| c.len() != n)) {
        return None;
    }
    if compressed_tables.iter().any(|c| c.len() != n) || blinding_factors + 1 >= n {
        return None;
    }
    let n_inputs: Vec<u32> = compressed_inputs.iter().map(|cols| cols.len() as u32).collect();
    let f: Vec<*const u64> = compressed_inputs.iter().flat_map(|cols| cols.iter().map(|c| c.as_ptr() as *const u64)).collect();
    let t: Vec<*const u64> = compressed_tables.iter().map(|c| c.as_ptr() as *const u64).collect();
    let mut m: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let mp: Vec<*mut u64> = m.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_mvlookup_multiplicities_bn254(k, f.as_ptr(), n_inputs.as_ptr(), t.as_ptr(), count, blinding_factors as u32, mp.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(m)
}

/// The mv-lookup grand sums phi (include/halo2hip.h): inputs and tables as for `try_mvlookup_multiplicities`, `m` their multiplicity
/// columns, `blinding` argument-major (`blinding_factors` values per argument).  `None` on any failure.
pub fn try_mvlookup_sums<F: Field + 'static>(k: u32, beta: &F, compressed_inputs: &[&[&[F]]], compressed_tables: &[&[F]], m: &[&[F]],
                                             blinding: &[F], blinding_factors: usize) -> Option<Vec<Vec<F>>> {
    let count = compressed_tables.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || count > 65535 || compressed_inputs.len() != count || m.len() != count {
        return None;
    }
    let n = 1usize << k;
    if compressed_inputs.iter().any(|cols| cols.is_empty() || cols.len() > 255 || cols.iter().any(|c| c.len() != n)) {
        return None;
    }
    if compressed_tables.iter().chain(m.iter()).any(|c| c.len() != n) || blinding.len() != count * blinding_factors || blinding_factors + 1 >= n {
        return None;
    }
    let n_inputs: Vec<u32> = compressed_inputs.iter().map(|cols| cols.len() as u32).collect();
    let f: Vec<*const u64> = compressed_inputs.iter().flat_map(|cols| cols.iter().map(|c| c.as_ptr() as *const u64)).collect();
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (t, mm) = (ptrs(compressed_tables), ptrs(m));
    let mut phi: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let pp: Vec<*mut u64> = phi.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_mvlookup_sums_bn254(k, fr_ptr(beta), f.as_ptr(), n_inputs.as_ptr(), t.as_ptr(), mm.as_ptr(), count, blinding.as_ptr() as *const u64,
                                       blinding_factors as u32, pp.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(phi)
}

/// `commit_permuted`'s compressed expressions (plonk/lookup/prover.rs:90-115): `graphs[g]` (an input or table side of a lookup, built
/// as `add_expression` of each expression and `Horner(Constant(0), parts, Theta)`) over the Lagrange columns.  `None` on any failure.
#[allow(clippy::too_many_arguments)]
pub fn try_lookup_compress<F: Field + 'static>(k: u32, fixed: &[&[F]], advice: &[&[F]], instance: &[&[F]], challenges: &[F], theta: &F,
                                               graphs: &[&evalh::FlatGraph]) -> Option<Vec<Vec<F>>> {
    if !is::<F, Fr>() || !layout_ok() || k > 28 {
        return None;
    }
    let n = 1usize << k;
    if fixed.iter().chain(advice.iter()).chain(instance.iter()).any(|c| c.len() != n) {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (f, a, i) = (ptrs(fixed), ptrs(advice), ptrs(instance));
    let views: Vec<evalh::h2hip_graph> = graphs.iter().map(|g| g.view()).collect();
    let mut out: Vec<Vec<F>> = (0..graphs.len()).map(|_| vec![F::zero(); n]).collect();
    let op: Vec<*mut u64> = out.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_lookup_compress_bn254(k, f.as_ptr(), f.len() as u32, a.as_ptr(), a.len() as u32, i.as_ptr(), i.len() as u32,
                                         challenges.as_ptr() as *const u64, challenges.len() as u32, fr_ptr(theta), views.as_ptr(),
                                         views.len(), op.as_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `permute_expression_pair` (plonk/lookup/prover.rs:391-475) for several lookups in one call: `blinding` holds 2(b + 1) values per
/// lookup, the A' rows then the S' rows, drawn by the caller in the reference's order.  `Ok(None)` when the engine did not take the
/// call, `Err(H2HIP_ELOOKUP)` when an input value is missing from its table (`Error::ConstraintSystemFailure`).
#[allow(clippy::type_complexity)]
pub fn try_lookup_permute<F: Field + 'static>(k: u32, compressed_inputs: &[&[F]], compressed_tables: &[&[F]], blinding: &[F],
                                              blinding_factors: usize) -> Result<Option<(Vec<Vec<F>>, Vec<Vec<F>>)>, i32> {
    let count = compressed_inputs.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || compressed_tables.len() != count {
        return Ok(None);
    }
    let n = 1usize << k;
    if compressed_inputs.iter().chain(compressed_tables.iter()).any(|c| c.len() != n) || blinding_factors + 1 >= n
        || blinding.len() != count * 2 * (blinding_factors + 1) {
        return Ok(None);
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (a, s) = (ptrs(compressed_inputs), ptrs(compressed_tables));
    let mut pa: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let mut pt: Vec<Vec<F>> = (0..count).map(|_| vec![F::zero(); n]).collect();
    let pap: Vec<*mut u64> = pa.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let ptp: Vec<*mut u64> = pt.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe {
        ffi::h2hip_lookup_permute_bn254(k, a.as_ptr(), s.as_ptr(), count, blinding.as_ptr() as *const u64, blinding_factors as u32,
                                        pap.as_ptr(), ptp.as_ptr())
    };
    match rc {
        0 => Ok(Some((pa, pt))),
        H2HIP_ELOOKUP => Err(H2HIP_ELOOKUP),
        _ => Ok(None),
    }
}

/// `eval_polynomial` (arithmetic.rs:304-328) for every query of a proof in one call: query `q` evaluates `polys[query_poly[q]]` at
/// `points[q]`; queries of one polynomial share its reads.  `Some(evals)` when the engine took the call; `None` on any failure.
pub fn try_eval_polynomials<F: Field + 'static>(polys: &[&[F]], query_poly: &[u32], points: &[F]) -> Option<Vec<F>> {
    if !is::<F, Fr>() || !layout_ok() || query_poly.len() != points.len() || query_poly.iter().any(|&j| j as usize >= polys.len()) {
        return None;
    }
    if polys.iter().any(|p| p.len() > 1usize << 28) {
        return None;
    }
    let ptrs: Vec<*const u64> = polys.iter().map(|p| p.as_ptr() as *const u64).collect();
    let lens: Vec<usize> = polys.iter().map(|p| p.len()).collect();
    let mut evals = vec![F::zero(); points.len()];
    let rc = unsafe {
        ffi::h2hip_eval_polynomials_bn254(ptrs.as_ptr(), lens.as_ptr(), ptrs.len(), query_poly.as_ptr(), points.as_ptr() as *const u64,
                                          points.len(), evals.as_mut_ptr() as *mut u64)
    };
    if rc != 0 {
        return None;
    }
    Some(evals)
}

/// The opening's combine / divide / scale primitive (h2hip_poly_combine_bn254_fr): `(sum_j scalars[j] polys[j] - sub)` divided by
/// `(X - r)` for each `r` of `roots` in order, times `scale`, zero-padded to `out_len` coefficients.  Covers GWC's witnesses
/// (gwc/prover.rs:61-89), SHPLONK's quotients (shplonk/prover.rs:138-275) and the h_poly fold (vanishing/prover.rs:131-135).
/// Every polynomial has the same length.  `None` on any failure.
#[allow(clippy::too_many_arguments)]
pub fn try_poly_combine<F: Field + 'static>(polys: &[&[F]], scalars: &[F], sub: &[F], roots: &[F], scale: &F, out_len: usize) -> Option<Vec<F>> {
    if !is::<F, Fr>() || !layout_ok() || polys.is_empty() || scalars.len() != polys.len() {
        return None;
    }
    let len = polys[0].len();
    if polys.iter().any(|p| p.len() != len) || len > 1usize << 28 || roots.len() > 16 || len < roots.len() || sub.len() > len.min(16)
        || out_len < len - roots.len() || out_len > 1usize << 28 {
        return None;
    }
    let ptrs: Vec<*const u64> = polys.iter().map(|p| p.as_ptr() as *const u64).collect();
    let mut out = vec![F::zero(); out_len];
    let rc = unsafe {
        ffi::h2hip_poly_combine_bn254_fr(ptrs.as_ptr(), len, scalars.as_ptr() as *const u64, ptrs.len(), sub.as_ptr() as *const u64, sub.len(),
                                         roots.as_ptr() as *const u64, roots.len(), fr_ptr(scale), 0, out.as_mut_ptr() as *mut u64, out_len,
                                         std::ptr::null_mut())
    };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `kate_division` (arithmetic.rs:348-366): `a(X) / (X - b)` without the remainder, `a.len() - 1` coefficients.
pub fn try_kate_division<F: Field + 'static>(a: &[F], b: &F) -> Option<Vec<F>> {
    if a.is_empty() {
        return None;
    }
    try_poly_combine(&[a], &[F::one()], &[], std::slice::from_ref(b), &F::one(), a.len() - 1)
}

/// `div_by_vanishing` (shplonk/prover.rs:26-31): `kate_division` by each root in order, `a.len() - roots.len()` coefficients.
pub fn try_div_by_vanishing<F: Field + 'static>(a: &[F], roots: &[F]) -> Option<Vec<F>> {
    if a.len() < roots.len() {
        return None;
    }
    try_poly_combine(&[a], &[F::one()], &[], roots, &F::one(), a.len() - roots.len())
}

/// The domain constants the keygen entry points take, as `EvaluationDomain` holds them (poly/domain.rs:18-34).
pub struct KeygenDomain<'a, F> {
    pub k: u32,
    pub extended_k: u32,
    pub omega: &'a F,
    pub omega_inv: &'a F,
    pub ifft_divisor: &'a F,
    pub extended_omega: &'a F,
    pub g_coset: &'a F,
    pub g_coset_inv: &'a F,
}

/// What `try_permutation_keygen` returns: the forms that were asked for, one column per permutation column.
pub struct PermutationKeyColumns<F> {
    pub permutations: Option<Vec<Vec<F>>>,
    pub polys: Option<Vec<Vec<F>>>,
    pub cosets: Option<Vec<Vec<F>>>,
}

/// `Assembly::build_vk` / `build_pk`'s columns (plonk/permutation/keygen.rs:105-242) from `Assembly::mapping`, flattened per column to
/// `(column, row)` pairs of `u32`: `permutations[j][i] = delta^c omega^r`, its `lagrange_to_coeff` and its `coeff_to_extended`.
/// `want = (permutations, polys, cosets)`; build_vk asks for the first alone.  `None` on any failure (the CPU body then runs).
pub fn try_permutation_keygen<F: Field + 'static>(domain: &KeygenDomain<F>, delta: &F, mapping: &[&[[u32; 2]]],
                                                  want: (bool, bool, bool)) -> Option<PermutationKeyColumns<F>> {
    let (k, ek) = (domain.k, domain.extended_k);
    if !is::<F, Fr>() || !layout_ok() || k > ek || ek > 28 || mapping.len() > 65535 {
        return None;
    }
    let (n, len, m) = (1usize << k, 1usize << ek, mapping.len());
    if mapping.iter().any(|c| c.len() != n) {
        return None;
    }
    let mp: Vec<*const u32> = mapping.iter().map(|c| c.as_ptr() as *const u32).collect();
    let alloc = |on: bool, rows: usize| -> Option<Vec<Vec<F>>> { if on { Some((0..m).map(|_| vec![F::zero(); rows]).collect()) } else { None } };
    let (mut perms, mut polys, mut cosets) = (alloc(want.0, n), alloc(want.1, n), alloc(want.2, len));
    let table = |cols: &mut Option<Vec<Vec<F>>>| -> Vec<*mut u64> {
        cols.as_mut().map(|v| v.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect()).unwrap_or_default()
    };
    let (pp, qp, cp) = (table(&mut perms), table(&mut polys), table(&mut cosets));
    let arg = |t: &Vec<*mut u64>, on: bool| if on { t.as_ptr() } else { std::ptr::null() };
    let rc = unsafe {
        ffi::h2hip_permutation_keygen_bn254(k, fr_ptr(domain.omega), fr_ptr(domain.omega_inv), fr_ptr(domain.ifft_divisor), ek,
                                            fr_ptr(domain.extended_omega), fr_ptr(domain.g_coset), fr_ptr(domain.g_coset_inv), fr_ptr(delta),
                                            mp.as_ptr(), m as u32, arg(&pp, want.0), arg(&qp, want.1), arg(&cp, want.2))
    };
    if rc != 0 {
        return None;
    }
    Some(PermutationKeyColumns { permutations: perms, polys, cosets })
}

/// The permutation mapping from the copy constraints themselves, `[left_column, left_row, right_column, right_row]` each, in place of
/// the serial `Assembly::copy` loop (plonk/permutation/keygen.rs:46-103): every cell maps to the next cell of its connected component in
/// ascending `column * 2^k + row` order, the last one to the least (include/halo2hip.h).  The result is what `try_permutation_keygen` and
/// `try_check_permutation` take as `mapping`.  It has the cycles `Assembly::copy` builds for the same constraints, in an order of its
/// own, so a key built from it is valid, not byte-identical: prover and verifier must both use it.  `None` on any failure, a copy out
/// of range included.
pub fn try_permutation_mapping(k: u32, n_columns: usize, copies: &[[u32; 4]]) -> Option<Vec<Vec<[u32; 2]>>> {
    if k > 28 || n_columns > 65535 || ((n_columns as u64) << k) > (1u64 << 32) || copies.len() > (1usize << 30) {
        return None;
    }
    let n = 1usize << k;
    let mut mapping: Vec<Vec<[u32; 2]>> = (0..n_columns).map(|_| vec![[0u32; 2]; n]).collect();
    let mp: Vec<*mut u32> = mapping.iter_mut().map(|c| c.as_mut_ptr() as *mut u32).collect();
    let cp = if copies.is_empty() { std::ptr::null() } else { copies.as_ptr() as *const u32 };
    let rc = unsafe { ffi::h2hip_permutation_mapping(k, n_columns as u32, cp, copies.len(), mp.as_ptr()) };
    if rc != 0 {
        return None;
    }
    Some(mapping)
}

/// `batch_invert_assigned` (poly.rs:180-209) over columns the caller has flattened from `Assigned<F>`: `numerators[j]` (zero for `Zero`,
/// `x` for `Trivial(x)`), and for the `Rational` cells their ascending rows `rat_rows[j]` and denominators `rat_denoms[j]`.  One
/// inversion over all columns.  `None` on any failure.
pub fn try_batch_invert_assigned<F: Field + 'static>(k: u32, numerators: &[&[F]], rat_rows: &[&[u32]], rat_denoms: &[&[F]]) -> Option<Vec<Vec<F>>> {
    let m = numerators.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || rat_rows.len() != m || rat_denoms.len() != m {
        return None;
    }
    let n = 1usize << k;
    if numerators.iter().any(|c| c.len() != n) || rat_rows.iter().zip(rat_denoms.iter()).any(|(r, d)| r.len() != d.len() || r.len() > n) {
        return None;
    }
    let np: Vec<*const u64> = numerators.iter().map(|c| c.as_ptr() as *const u64).collect();
    let rp: Vec<*const u32> = rat_rows.iter().map(|c| if c.is_empty() { std::ptr::null() } else { c.as_ptr() }).collect();
    let dp: Vec<*const u64> = rat_denoms.iter().map(|c| if c.is_empty() { std::ptr::null() } else { c.as_ptr() as *const u64 }).collect();
    let counts: Vec<usize> = rat_rows.iter().map(|c| c.len()).collect();
    let mut out: Vec<Vec<F>> = (0..m).map(|_| vec![F::zero(); n]).collect();
    let op: Vec<*mut u64> = out.iter_mut().map(|c| c.as_mut_ptr() as *mut u64).collect();
    let rc = unsafe { ffi::h2hip_batch_invert_assigned_bn254(k, np.as_ptr(), rp.as_ptr(), counts.as_ptr(), dp.as_ptr(), m, op.as_ptr()) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `pk.l0`, `pk.l_last`, `pk.l_active_row` (plonk/keygen.rs:320-351) in extended-coset form.  `None` on any failure.
pub fn try_key_lagrange_columns<F: Field + 'static>(domain: &KeygenDomain<F>, blinding_factors: usize) -> Option<(Vec<F>, Vec<F>, Vec<F>)> {
    let (k, ek) = (domain.k, domain.extended_k);
    if !is::<F, Fr>() || !layout_ok() || k > ek || ek > 28 || blinding_factors + 1 >= 1usize << k {
        return None;
    }
    let len = 1usize << ek;
    let (mut l0, mut l_last, mut l_active_row) = (vec![F::zero(); len], vec![F::zero(); len], vec![F::zero(); len]);
    let rc = unsafe {
        ffi::h2hip_key_lagrange_columns_bn254(k, fr_ptr(domain.omega_inv), fr_ptr(domain.ifft_divisor), ek, fr_ptr(domain.extended_omega),
                                              fr_ptr(domain.g_coset), fr_ptr(domain.g_coset_inv), blinding_factors as u32,
                                              l0.as_mut_ptr() as *mut u64, l_last.as_mut_ptr() as *mut u64, l_active_row.as_mut_ptr() as *mut u64)
    };
    if rc != 0 {
        return None;
    }
    Some((l0, l_last, l_active_row))
}

/// What a witness check returns: per constraint how many rows fail, and the lowest `max_rows` of them in ascending order.
pub struct CheckReport {
    pub counts: Vec<u64>,
    pub rows: Vec<Vec<u32>>,
}

fn check_report(counts: Vec<u64>, flat: Vec<u32>, max_rows: usize) -> CheckReport {
    let rows = counts.iter().enumerate().map(|(j, &c)| flat[j * max_rows..j * max_rows + (c as usize).min(max_rows)].to_vec()).collect();
    CheckReport { counts, rows }
}

/// `MockProver::verify`'s gate loop (dev.rs:676-746) over the prover's own Lagrange columns, all 2^k rows: `graphs[g]` is
/// `add_expression` of one gate polynomial closed by a `Store` of its value.  Failures are data; `None` when the engine did not take
/// the call.
#[allow(clippy::too_many_arguments)]
pub fn try_check_gates<F: Field + 'static>(k: u32, fixed: &[&[F]], advice: &[&[F]], instance: &[&[F]], challenges: &[F],
                                           graphs: &[&evalh::FlatGraph], max_rows: usize) -> Option<CheckReport> {
    if !is::<F, Fr>() || !layout_ok() || k > 28 || graphs.len() > 65535 || max_rows > 65535 {
        return None;
    }
    let n = 1usize << k;
    if fixed.iter().chain(advice.iter()).chain(instance.iter()).any(|c| c.len() != n) {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (f, a, i) = (ptrs(fixed), ptrs(advice), ptrs(instance));
    let views: Vec<evalh::h2hip_graph> = graphs.iter().map(|g| g.view()).collect();
    let mut counts = vec![0u64; graphs.len()];
    let mut rows = vec![u32::MAX; graphs.len() * max_rows];
    let rc = unsafe {
        ffi::h2hip_check_gates_bn254(k, f.as_ptr(), f.len() as u32, a.as_ptr(), a.len() as u32, i.as_ptr(), i.len() as u32,
                                     challenges.as_ptr() as *const u64, challenges.len() as u32, views.as_ptr(), views.len(),
                                     max_rows as u32, counts.as_mut_ptr(), rows.as_mut_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(check_report(counts, rows, max_rows))
}

/// `MockProver::verify`'s copy-constraint loop (dev.rs:889-931): `columns` are the permutation argument's Lagrange columns, `mapping`
/// is `Assembly::mapping` as `try_permutation_keygen` takes it.  `None` when the engine did not take the call (a pair out of range
/// included).
pub fn try_check_permutation<F: Field + 'static>(k: u32, columns: &[&[F]], mapping: &[&[[u32; 2]]], max_rows: usize) -> Option<CheckReport> {
    let m = columns.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || m > 65535 || mapping.len() != m || max_rows > 65535 {
        return None;
    }
    let n = 1usize << k;
    if columns.iter().any(|c| c.len() != n) || mapping.iter().any(|c| c.len() != n) {
        return None;
    }
    let cp: Vec<*const u64> = columns.iter().map(|c| c.as_ptr() as *const u64).collect();
    let mp: Vec<*const u32> = mapping.iter().map(|c| c.as_ptr() as *const u32).collect();
    let mut counts = vec![0u64; m];
    let mut rows = vec![u32::MAX; m * max_rows];
    let rc = unsafe {
        ffi::h2hip_check_permutation_bn254(k, cp.as_ptr(), mp.as_ptr(), m as u32, max_rows as u32, counts.as_mut_ptr(), rows.as_mut_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(check_report(counts, rows, max_rows))
}

/// `MockProver::verify`'s lookup loop (dev.rs:751-886) on the columns `try_lookup_compress` produces for a theta of the caller's
/// choosing: the input rows below u = 2^k - blinding_factors - 1 whose value no table row below u holds.
pub fn try_check_lookups<F: Field + 'static>(k: u32, compressed_inputs: &[&[F]], compressed_tables: &[&[F]], blinding_factors: usize,
                                             max_rows: usize) -> Option<CheckReport> {
    let count = compressed_inputs.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || count > 32767 || compressed_tables.len() != count || max_rows > 65535 {
        return None;
    }
    let n = 1usize << k;
    if compressed_inputs.iter().chain(compressed_tables.iter()).any(|c| c.len() != n) || blinding_factors + 1 >= n {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (a, s) = (ptrs(compressed_inputs), ptrs(compressed_tables));
    let mut counts = vec![0u64; count];
    let mut rows = vec![u32::MAX; count * max_rows];
    let rc = unsafe {
        ffi::h2hip_check_lookups_bn254(k, a.as_ptr(), s.as_ptr(), count, blinding_factors as u32, max_rows as u32, counts.as_mut_ptr(),
                                       rows.as_mut_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(check_report(counts, rows, max_rows))
}

/// The shuffle argument's witness check on compressed columns: the input rows below u = 2^k - blinding_factors - 1 whose value occurs
/// a different number of times among the input rows below u than among the shuffle rows below u (`h2hip_check_shuffles_bn254`).
pub fn try_check_shuffles<F: Field + 'static>(k: u32, compressed_inputs: &[&[F]], compressed_shuffles: &[&[F]], blinding_factors: usize,
                                              max_rows: usize) -> Option<CheckReport> {
    let count = compressed_inputs.len();
    if !is::<F, Fr>() || !layout_ok() || k > 28 || count > 32767 || compressed_shuffles.len() != count || max_rows > 65535 {
        return None;
    }
    let n = 1usize << k;
    if compressed_inputs.iter().chain(compressed_shuffles.iter()).any(|c| c.len() != n) || blinding_factors + 1 >= n {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    let (a, s) = (ptrs(compressed_inputs), ptrs(compressed_shuffles));
    let mut counts = vec![0u64; count];
    let mut rows = vec![u32::MAX; count * max_rows];
    let rc = unsafe {
        ffi::h2hip_check_shuffles_bn254(k, a.as_ptr(), s.as_ptr(), count, blinding_factors as u32, max_rows as u32, counts.as_mut_ptr(),
                                        rows.as_mut_ptr())
    };
    if rc != 0 {
        return None;
    }
    Some(check_report(counts, rows, max_rows))
}

/// What a fallible conversion found: how many elements fail the format's checks, and the lowest index of them.  The caller turns
/// it into the reference's `io::Error` ("invalid point encoding" / "Invalid prime field point encoding").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct InvalidEncoding {
    pub count: u64,
    pub first: u64,
}

/// an element fails its format's checks
pub const H2HIP_EENCODING: i32 = 5;

/// `rc` and `invalid[]` of a fallible call: `None` when the engine did not take it, `Some(Err)` when it did and elements are invalid
fn encoding_result<T>(rc: i32, invalid: [u64; 2], value: T) -> Option<Result<T, InvalidEncoding>> {
    match rc {
        H2HIP_OK => Some(Ok(value)),
        H2HIP_EENCODING => Some(Err(InvalidEncoding { count: invalid[0], first: invalid[1] })),
        _ => None,
    }
}

/// `SerdeFormat::Processed` read of `bytes.len()` G1 points (`G1Affine::from_bytes` per element, one square root each) on the GPU.
pub fn try_g1_decompress<C: CurveAffine>(bytes: &[[u8; 32]]) -> Option<Result<Vec<C>, InvalidEncoding>> {
    if !is::<C, G1Affine>() || !layout_ok() || bytes.len() > 1 << 30 {
        return None;
    }
    let mut out = vec![C::identity(); bytes.len()];
    let mut invalid = [0u64; 2];
    let rc = unsafe {
        ffi::h2hip_g1_decompress_bn254(bytes.as_ptr() as *const std::os::raw::c_void, bytes.len(), out.as_mut_ptr() as *mut u64, invalid.as_mut_ptr())
    };
    encoding_result(rc, invalid, out)
}

/// `SerdeFormat::Processed` write: `G1Affine::to_bytes` per element.
pub fn try_g1_compress<C: CurveAffine>(points: &[C]) -> Option<Vec<[u8; 32]>> {
    if !is::<C, G1Affine>() || !layout_ok() || points.len() > 1 << 30 {
        return None;
    }
    let mut out = vec![[0u8; 32]; points.len()];
    let rc = unsafe { ffi::h2hip_g1_compress_bn254(points.as_ptr() as *const u64, points.len(), out.as_mut_ptr() as *mut std::os::raw::c_void) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `SerdeFormat::RawBytes` read: `read_raw`'s checks (coordinates below the modulus, point on the curve) on points read with
/// `read_raw_unchecked`.
pub fn try_g1_validate<C: CurveAffine>(points: &[C]) -> Option<Result<(), InvalidEncoding>> {
    if !is::<C, G1Affine>() || !layout_ok() || points.len() > 1 << 30 {
        return None;
    }
    let mut invalid = [0u64; 2];
    let rc = unsafe { ffi::h2hip_g1_validate_bn254(points.as_ptr() as *const u64, points.len(), invalid.as_mut_ptr()) };
    encoding_result(rc, invalid, ())
}

/// `Fr::from_repr` over a vector (`SerdePrimeField::read`, `Processed`): canonical little-endian to Montgomery, values >= r invalid.
pub fn try_fr_from_repr<F: Field + 'static>(repr: &[[u8; 32]]) -> Option<Result<Vec<F>, InvalidEncoding>> {
    if !is::<F, Fr>() || !layout_ok() || repr.len() > 1 << 30 {
        return None;
    }
    let mut out = vec![F::zero(); repr.len()];
    let mut invalid = [0u64; 2];
    let rc = unsafe {
        ffi::h2hip_fr_from_repr_bn254(repr.as_ptr() as *const std::os::raw::c_void, repr.len(), out.as_mut_ptr() as *mut u64, invalid.as_mut_ptr())
    };
    encoding_result(rc, invalid, out)
}

/// `Fr::to_repr` over a vector (`SerdePrimeField::write`, `Processed`).
pub fn try_fr_to_repr<F: Field + 'static>(values: &[F]) -> Option<Vec<[u8; 32]>> {
    if !is::<F, Fr>() || !layout_ok() || values.len() > 1 << 30 {
        return None;
    }
    let mut out = vec![[0u8; 32]; values.len()];
    let rc = unsafe { ffi::h2hip_fr_to_repr_bn254(values.as_ptr() as *const u64, values.len(), out.as_mut_ptr() as *mut std::os::raw::c_void) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

// ---- randomness (include/halo2hip.h, "randomness") ------------------------------------------------------------------------------------

/// `n` draws of `F::random` as `ChaCha20Rng::from_seed(*seed)` yields them after `first_block` earlier draws: element `i` is
/// `Fr::from_bytes_wide` of ChaCha20 block `first_block + i` (one draw = eight `next_u64` = one block).  The loop of
/// `vanishing::Argument::commit` (plonk/vanishing/prover.rs:53-55) as one call.  The seed is the caller's entropy
/// (`rng.fill_bytes`) and as secret as the polynomial; the engine only expands it.  `None`: not taken, run the original loop.
pub fn try_fr_random<F: Field + 'static>(seed: &[u8; 32], stream_id: u64, first_block: u64, n: usize) -> Option<Vec<F>> {
    if !is::<F, Fr>() || !layout_ok() {
        return None;
    }
    let mut out = vec![F::zero(); n];
    let rc = unsafe { ffi::h2hip_fr_random_bn254(seed.as_ptr(), stream_id, first_block, n, out.as_mut_ptr() as *mut u64) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `Fr::from_bytes_wide` over a vector: each 64 bytes as one little-endian integer, reduced mod r.
pub fn try_fr_from_bytes_wide<F: Field + 'static>(bytes: &[[u8; 64]]) -> Option<Vec<F>> {
    if !is::<F, Fr>() || !layout_ok() {
        return None;
    }
    let mut out = vec![F::zero(); bytes.len()];
    let rc = unsafe { ffi::h2hip_fr_from_bytes_wide_bn254(bytes.as_ptr() as *const u8, bytes.len(), out.as_mut_ptr() as *mut u64) };
    if rc != 0 {
        return None;
    }
    Some(out)
}
