//! A round of the inner-product argument's opening as one engine call (include/halo2hip_ipa_round.h, part of halo2hip_ipa.h), over the
//! generated `ffi_ipa_round.rs`: the two MSMs `L_j`, `R_j` of `commitment::create_proof` (poly/ipa/commitment/prover.rs:109-110) from one
//! run of the MSM pipeline, and the whole round -- the fold and the collapse by the challenge before it, the inner products and both
//! MSMs -- with one wait.  The state of an opening lives in HBM, so both take device pointers and a stream and are `unsafe`: nothing
//! here can check that those pointers hold the stated number of elements.
//!
//! As everywhere in this crate a wrapper returns `None` when the engine does not take the call, and the caller runs the reference's CPU
//! body.  Not compiled in the repository that ships it; `tests/test_ipa_round_abi.py` checks the extern block against
//! the header and the shared library.
use super::ffi_ipa_round as ffi;
use super::{is, layout_ok};
use ff::Field;
use halo2curves::bn256::{Fr, G1};
use halo2curves::CurveAffine;
use std::os::raw::c_void;

/// `(L, R) = (<p[half..2 half], g[..half]>, <p[..half], g[half..2 half]>)`; waits for `stream`.
///
/// # Safety
/// `d_p` is device memory of at least `2 * half` scalars of 32 bytes, `d_g` of at least `2 * half` affine points of 64 bytes, both
/// 16-byte aligned; `stream` is a HIP stream of their device or null.
pub unsafe fn try_ipa_round_msms<C: CurveAffine>(d_p: *const c_void, d_g: *const c_void, half: usize, stream: *mut c_void) -> Option<(C::Curve, C::Curve)> {
    if !is::<C::Curve, G1>() || !is::<C::Scalar, Fr>() || !layout_ok() || half == 0 || half > 1usize << 26 {
        return None;
    }
    let mut out = [[0u64; 12]; 2];
    let (l, r) = out.split_at_mut(1);
    if ffi::h2hip_ipa_round_msms_bn254_device(d_p, d_g, half, l[0].as_mut_ptr(), r[0].as_mut_ptr(), stream) != 0 {
        return None;
    }
    Some((std::mem::transmute_copy(&out[0]), std::mem::transmute_copy(&out[1])))
}

/// One round after the challenge of the round before it.  `challenge = Some((u, u_inv))`: `p`, `b` hold `4 * half` elements and `g`
/// `4 * half` points, which are first folded and collapsed by it at `2 * half`; `None`: the first round.  Returns `(L, R, value_l,
/// value_r)` at `half`; waits for `stream` once.  After the last round (`half == 1`) the caller makes one `try_ipa_fold` at `half = 1`
/// to read `c = p'[0]`.
///
/// # Safety
/// As `try_ipa_round_msms`, with `d_b` like `d_p`; all three arrays are written.
pub unsafe fn try_ipa_round<C: CurveAffine>(d_p: *mut c_void, d_b: *mut c_void, d_g: *mut c_void, half: usize, challenge: Option<(&C::Scalar, &C::Scalar)>,
                                            stream: *mut c_void) -> Option<(C::Curve, C::Curve, C::Scalar, C::Scalar)> {
    if !is::<C::Curve, G1>() || !is::<C::Scalar, Fr>() || !layout_ok() || half == 0 || half > 1usize << 26 {
        return None;
    }
    let (u, u_inv) = match challenge {
        Some((u, u_inv)) => (u as *const C::Scalar as *const u64, u_inv as *const C::Scalar as *const u64),
        None => (std::ptr::null(), std::ptr::null()),
    };
    let mut out = [[0u64; 12]; 2];
    let mut values = [C::Scalar::zero(); 2];
    let (l, r) = out.split_at_mut(1);
    if ffi::h2hip_ipa_round_bn254_device(d_p, d_b, d_g, half, u, u_inv, l[0].as_mut_ptr(), r[0].as_mut_ptr(), values.as_mut_ptr() as *mut u64, stream) != 0 {
        return None;
    }
    Some((std::mem::transmute_copy(&out[0]), std::mem::transmute_copy(&out[1]), values[0], values[1]))
}

/// Whether the wrappers' openings use the round call (the default) or the separate calls.
pub fn ipa_round_call() -> bool {
    unsafe { ffi::h2hip_ipa_get_round_call() != 0 }
}

pub fn set_ipa_round_call(on: bool) {
    unsafe {
        ffi::h2hip_ipa_set_round_call(on as i32);
    }
}

/// The largest `half` whose two MSMs run as one two-set run under the settings in force.
pub fn ipa_round_msms_fused_max_half() -> usize {
    unsafe { ffi::h2hip_ipa_round_msms_fused_max_half() }
}
