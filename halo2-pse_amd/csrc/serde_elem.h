// serde_elem.h -- what serde.hip's kernels do to ONE element, host and device: the conversions of SerdeFormat::Processed and the checks
// of SerdeFormat::RawBytes (helpers.rs:8-20).  Kept apart from the kernels so that tests/cpp/test_serde_host.cpp runs the same source on
// the host with H2_FU_CHECK, where every product asserts fieldu.h's limb bounds.  A value is passed as the Fe its 32 bytes load as.
#pragma once
#include "ecu.h"

namespace h2 {

H2_HD Fu fu_small(uint32_t v) {  // the integer v < 2^29 as limbs
    Fu o = fu_zero();
    o.l[0] = (int32_t)v;
    return o;
}

// 32 B compressed G1 -> x || y, Montgomery (R = 2^256); false: an invalid encoding, *out is (0, 0).  The identity (32 zero bytes) is valid
// and gives (0, 0) too.  Every lane runs the whole chain whatever its bytes are, so that a wave walks fu_sqrt together.
H2_HD bool g1_decompress_elem(Fe xc, Affine* out) {
    const uint32_t sign = xc.l[7] >> 31;
    xc.l[7] &= 0x7fffffffu;
    const bool identity = fe_is_zero(xc) && !sign;
    // x is an integer below 2^255 whatever the bytes were (limbs < 2^29, top limb < 2^23): inside fu_mul's bound also when x >= q
    const Fu x = fu_mul<FqU>(fu_slice(xc), fu_const<FqU>(FqU::R2_I));                            // I-form, in (0, 1.1 p)
    const Fu t = fu_norm(fu_add(fu_mul<FqU>(fu_sqr<FqU>(x), x), fu_const<FqU>(FqU::THREE_I)));  // x^3 + 3, in (-0.1 p, 2.1 p)
    const Fu y = fu_sqrt<FqU>(t);
    const bool square = fe_is_zero(fu_canon_fast<FqU>(fu_sub(fu_sqr<FqU>(y), t)));               // |value| < 2.4 p
    const Fe yc = fu_mul_canon<FqU>(y, fu_small(1));                                             // (y 2^261) / 2^261: canonical y
    const bool flip = (yc.l[0] & 1u) != sign;
    const bool ok = identity || (fe_is_canonical<FqP>(xc) && square);
    out->x = fu_mul_canon<FqU>(x, fu_one_e<FqU>());
    out->y = fu_mul_canon<FqU>(flip ? fu_neg(y) : y, fu_one_e<FqU>());
    if (identity || !ok) out->x = out->y = fe_zero<FqP>();
    return ok;
}

// x || y (reduced, on the curve) -> 32 B: canonical x, the low bit of canonical y in the top bit; (0, 0) -> zeros
H2_HD Fe g1_compress_elem(const Affine& p) {
    Fe o = fe_zero<FqP>();
    if (affine_is_identity(p)) return o;
    o = fe_to_canonical<FqP>(p.x);
    o.l[7] |= (fe_to_canonical<FqP>(p.y).l[0] & 1u) << 31;
    return o;
}

// read_raw's checks: both coordinates below q, and (0, 0) or y^2 = x^3 + 3
H2_HD bool g1_validate_elem(const Affine& p) { return fe_is_canonical<FqP>(p.x) && fe_is_canonical<FqP>(p.y) && affine_on_curve(p); }

// canonical integer -> Montgomery; false (and zero) for a value >= r
H2_HD bool fr_from_repr_elem(const Fe& c, Fe* out) {
    const bool ok = fe_is_canonical<FrP>(c);
    *out = ok ? fe_from_canonical<FrP>(c) : fe_zero<FrP>();
    return ok;
}

}  // namespace h2
