//! The inner-product argument's entry points (include/halo2hip_ipa.h) behind safe signatures, over the generated `ffi_ipa.rs`:
//! `parallel_generator_collapse` (poly/ipa/commitment/prover.rs:155-167) and `compute_s` (poly/ipa/strategy.rs:161-176) on host
//! slices, and the round calls of `commitment::create_proof` on device memory the caller owns.  The state of an opening -- `p'`, `b`,
//! `G'` -- lives in HBM across its k rounds, so `try_ipa_powers`, `try_ipa_inner_products` and `try_ipa_fold` take device pointers and
//! a stream; they are `unsafe` because nothing here can check that those pointers hold the stated number of elements.
//!
//! As everywhere in this crate a wrapper returns `None` / `false` when the engine does not take the call, and the caller runs the
//! reference's CPU body.  Not compiled in the repository that ships it; `tests/test_ipa_abi.py` checks the extern
//! block against the header and the shared library.
use super::ffi_ipa as ffi;
use super::{is, layout_ok};
use ff::Field;
use halo2curves::bn256::{Fr, G1Affine};
use halo2curves::CurveAffine;
use std::os::raw::c_void;

/// `parallel_generator_collapse`: `g[i] <- g[i] + [challenge] g[len / 2 + i]` for the lower half of `g`, in place; the upper half is
/// left as it was.  `false`: not taken, `g` untouched.
pub fn try_ipa_collapse<C: CurveAffine>(g: &mut [C], challenge: &C::Scalar) -> bool {
    let half = g.len() / 2;
    if !is::<C, G1Affine>() || !is::<C::Scalar, Fr>() || !layout_ok() || half == 0 || g.len() != 2 * half || half > 1usize << 27 {
        return false;
    }
    // the engine writes the lower half of what it is given: hand it a copy, so that a failed call leaves `g` as it was
    let mut work = g.to_vec();
    let rc = unsafe { ffi::h2hip_ipa_collapse_bn254(work.as_mut_ptr() as *mut u64, half, challenge as *const C::Scalar as *const u64) };
    if rc != 0 {
        return false;
    }
    g[..half].copy_from_slice(&work[..half]);
    true
}

/// `compute_s(u, init)`: the 2^k coefficients of `init * prod (1 + u_{k - 1 - i} X^(2^i))`.
pub fn try_ipa_compute_s<F: Field + 'static>(u: &[F], init: &F) -> Option<Vec<F>> {
    if !is::<F, Fr>() || !layout_ok() || u.is_empty() || u.len() > 28 {
        return None;
    }
    let mut s = vec![F::zero(); 1usize << u.len()];
    let rc = unsafe {
        ffi::h2hip_ipa_compute_s_bn254_fr(u.as_ptr() as *const u64, u.len() as u32, init as *const F as *const u64, s.as_mut_ptr() as *mut u64)
    };
    if rc != 0 {
        return None;
    }
    Some(s)
}

/// `d_out[i] = x^i` for `i < n` (the vector `b`), queued on `stream`.
///
/// # Safety
/// `d_out` is device memory of at least `n` elements of 32 bytes, 16-byte aligned; `stream` is a HIP stream of its device or null.
pub unsafe fn try_ipa_powers<F: Field + 'static>(x: &F, n: usize, d_out: *mut c_void, stream: *mut c_void) -> bool {
    is::<F, Fr>() && layout_ok() && ffi::h2hip_ipa_powers_bn254_fr_device(x as *const F as *const u64, n, d_out, stream) == 0
}

/// `(<p[half..], b[..half]>, <p[..half], b[half..]>)`; waits for `stream`.
///
/// # Safety
/// `d_p` and `d_b` are device memory of at least `2 * half` elements of 32 bytes each, 16-byte aligned.
pub unsafe fn try_ipa_inner_products<F: Field + 'static>(d_p: *const c_void, d_b: *const c_void, half: usize, stream: *mut c_void) -> Option<(F, F)> {
    if !is::<F, Fr>() || !layout_ok() {
        return None;
    }
    let mut values = [F::zero(); 2];
    if ffi::h2hip_ipa_inner_products_bn254_fr_device(d_p, d_b, half, values.as_mut_ptr() as *mut u64, stream) != 0 {
        return None;
    }
    Some((values[0], values[1]))
}

/// The fold of a round in place: `p[i] += u_inv * p[half + i]`, `b[i] += u * b[half + i]`.  `want_next`: the same launch also computes
/// the next round's inner products (at `half / 2`; `half` even), and the call waits for `stream`; otherwise it is only queued and the
/// result is `Some(None)`.  `None`: not taken.
///
/// # Safety
/// As `try_ipa_inner_products`; both vectors are written.
pub unsafe fn try_ipa_fold<F: Field + 'static>(d_p: *mut c_void, d_b: *mut c_void, half: usize, u_inv: &F, u: &F, want_next: bool,
                                                stream: *mut c_void) -> Option<Option<(F, F)>> {
    if !is::<F, Fr>() || !layout_ok() {
        return None;
    }
    let mut values = [F::zero(); 2];
    let next = if want_next { values.as_mut_ptr() as *mut u64 } else { std::ptr::null_mut() };
    if ffi::h2hip_ipa_fold_bn254_fr_device(d_p, d_b, half, u_inv as *const F as *const u64, u as *const F as *const u64, next, stream) != 0 {
        return None;
    }
    Some(if want_next { Some((values[0], values[1])) } else { None })
}
