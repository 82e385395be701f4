//! The BN254 pairing and G2 scalar multiplication on the host (include/halo2hip_pairing.h) behind safe signatures, over the generated
//! `ffi_pairing.rs`: what `DualMSM::check` (poly/kzg/msm.rs:151-169) and `ParamsKZG::setup` (poly/kzg/commitment.rs:118-119) need of
//! `halo2curves::pairing`.  The calls are host code in the library: they need no GPU and launch nothing.
//!
//! `G2Affine`'s in-memory form is the header's raw layout: x.c0, x.c1, y.c0, y.c1 as Montgomery limbs, the identity (0, 0), as the
//! macro that defines `G1Affine` defines it.  The library's `Gt` layout (twelve Montgomery `Fq`, a_0, b_0, ..., a_5, b_5 for
//! sum (a_i + b_i u) w^i) is returned as limbs: whether `halo2curves::bn256::Gt` lays its `Fq12` out the same way has not been checked
//! against the crate, so no transmute into `Gt` is offered.
//!
//! As everywhere in this crate a wrapper returns `None` when the library does not take the call, and the caller runs the reference's
//! CPU body.  Not compiled in the repository that ships it; `tests/test_pairing.py` checks the extern block against
//! the header and the shared library.
use super::ffi_pairing as ffi;
use super::layout_ok;
use halo2curves::bn256::{Fr, G1Affine, G2Affine};
use halo2curves::group::prime::PrimeCurveAffine;

fn g2_raw(q: &G2Affine) -> [u64; 16] {
    let mut raw = [0u64; 16];
    unsafe { std::ptr::copy_nonoverlapping(q as *const G2Affine as *const u64, raw.as_mut_ptr(), 16) };
    raw
}

fn pairs(terms: &[(G1Affine, G2Affine)]) -> Option<(Vec<G1Affine>, Vec<[u64; 16]>)> {
    if !layout_ok() || terms.len() > 65536 {
        return None;
    }
    Some((terms.iter().map(|t| t.0).collect(), terms.iter().map(|t| g2_raw(&t.1)).collect()))
}

/// `prod_i e(P_i, Q_i) == 1`: one shared squaring chain, one final exponentiation.  Variable-time.
pub fn try_pairing_check(terms: &[(G1Affine, G2Affine)]) -> Option<bool> {
    let (g1, g2) = pairs(terms)?;
    let mut ok: std::os::raw::c_int = 0;
    let rc = unsafe { ffi::h2hip_pairing_check_bn254(g1.as_ptr() as *const u64, g2.as_ptr() as *const u64, terms.len(), &mut ok) };
    if rc != 0 {
        return None;
    }
    Some(ok == 1)
}

/// `prod_i e(P_i, Q_i)` in the library's `Gt` layout (see the module's note).
pub fn try_pairing(terms: &[(G1Affine, G2Affine)]) -> Option<[u64; 48]> {
    let (g1, g2) = pairs(terms)?;
    let mut out = [0u64; 48];
    let rc = unsafe { ffi::h2hip_pairing_bn254(g1.as_ptr() as *const u64, g2.as_ptr() as *const u64, terms.len(), out.as_mut_ptr()) };
    if rc != 0 {
        return None;
    }
    Some(out)
}

/// `[scalar] Q`, affine.
pub fn try_g2_mul(q: &G2Affine, scalar: &Fr) -> Option<G2Affine> {
    if !layout_ok() {
        return None;
    }
    let raw = g2_raw(q);
    let mut out = [0u64; 16];
    let rc = unsafe { ffi::h2hip_g2_mul_bn254(raw.as_ptr(), scalar as *const Fr as *const u64, out.as_mut_ptr()) };
    if rc != 0 {
        return None;
    }
    let mut p = G2Affine::identity();
    unsafe { std::ptr::copy_nonoverlapping(out.as_ptr(), &mut p as *mut G2Affine as *mut u64, 16) };
    Some(p)
}
