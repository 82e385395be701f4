//! Few-term sums of G1 points on the host (include/halo2hip_g1.h) behind a safe signature, over the generated `ffi_g1.rs`: the
//! `+ [r] W` of a blinded commitment, the `[value * z] U + [rand] W` of an inner-product round, the "other" terms of `MSMIPA::eval`
//! (poly/ipa/msm.rs:141-174).  The call is host code in the library: it needs no GPU and launches nothing.
//!
//! As everywhere in this crate the wrapper returns `None` when the library does not take the call, and the caller runs the reference's
//! CPU body.  Not compiled in the repository that ships it; `tests/test_g1_lincomb.py` checks the extern block against
//! the header and the shared library.
use super::ffi_g1 as ffi;
use super::{is, layout_ok};
use halo2curves::bn256::{Fr, G1Affine, G1};
use halo2curves::CurveAffine;

/// `out[j] = addends[j] + sum_i [scalars[j * t + i]] points[i]` with `t = points.len()`, all results affine through one shared
/// inversion.  `addends`: `None`, or one projective sum per result (an MSM's output); `scalars.len()` is `m * t`.  With `addends`
/// absent and `t = 0` there is nothing to size `m` by and the result is empty.  Variable-time in the scalars.
pub fn try_g1_linear_combinations<C: CurveAffine>(addends: Option<&[C::Curve]>, scalars: &[C::Scalar], points: &[C]) -> Option<Vec<C>> {
    if !is::<C, G1Affine>() || !is::<C::Curve, G1>() || !is::<C::Scalar, Fr>() || !layout_ok() {
        return None;
    }
    let t = points.len();
    let m = match addends {
        Some(a) => a.len(),
        None if t == 0 => 0,
        None => scalars.len() / t,
    };
    if scalars.len() != m * t || m.checked_mul(t).map_or(true, |terms| terms > 4096) {
        return None;
    }
    let mut out = vec![C::identity(); m];
    let rc = unsafe {
        ffi::h2hip_g1_linear_combinations_bn254(
            addends.map_or(std::ptr::null(), |a| a.as_ptr() as *const u64),
            scalars.as_ptr() as *const u64,
            points.as_ptr() as *const u64,
            m,
            t,
            out.as_mut_ptr() as *mut u64,
        )
    };
    if rc != 0 {
        return None;
    }
    Some(out)
}
