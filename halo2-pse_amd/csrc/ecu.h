// ecu.h -- BN254 G1 in XYZZ coordinates over the unsaturated field of fieldu.h (I-form
// values, lazily reduced).  Same group law and the same exceptional-case handling as ec.h
// (which stays the host-side / reference implementation and the thing this file is fuzzed
// against in tests/cpp/test_fieldu.cpp, test_ecu_native.cpp and test_ecu_unit.cpp); this is what the MSM kernels run.
//
// Invariants of an XYZZu accumulator: every coordinate is "normalised" (limbs 0..7 in [0, 2^29),
// small signed top limb) with |x|, |y| < 4.5 p and zz, zzz in (-0.1 p, 1.4 p); the identity is
// marked by zz having all limbs exactly zero (a valid point never has zz == 0 as an integer).
// Bound bookkeeping (units of p; a Montgomery product of magnitudes a, b lies in
// (-ab/169, ab/169 + 1)): mixed add with a freshly loaded point (|32 x| < 32):
//   U2, S2 in (-0.25, 1.25); |P|, |R| < 5.8; PP, RR < 1.4; |PPP|, |Q| < 1.1; |X3| < 4.5; |Y3| < 2.3.
// Mixed add with a native table record (x in [0, 1), |y| < 1: tighter everywhere): U2, S2 in (-0.01, 1.01); |P|, |R| < 5.6; the rest as above.
// A bucket's first record becomes the accumulator as it is: x, +-y (normalised), one, one, all below 1.
// Mixed add onto such a UNIT accumulator (zz = zzz = one exactly; the affine + affine form mmadd-2008-s), native record (x1, x2 in [0, 1),
// |y1|, |y2| < 1): P = x2 - x1 in (-1, 1), R = +-y2 - y1 in (-2, 2), so |P|, |R| < 2; PP in [0, 1.01), RR in [0, 1.03); PPP in (-0.01, 1.01);
// Q = x1 PP in [0, 1.01); X3 = RR - PPP - 2Q in (-3.03, 1.04); |Q - X3| < 4.1; Y3 = R (Q - X3) - y1 PPP in (-0.06, 1.06); ZZ3 = PP and
// ZZZ3 = PPP are inside (-0.1, 1.4).  E-form point onto a unit accumulator (x1, y1 in (-0.2, 1.2) from the first point's products by one):
// U2 and S2 stay products (they are what brings 32x inside the bounds), |P|, |R| < 1.5, the rest as in the native case.
// Limb bookkeeping: products always see one operand with |l| < 2^29 and the other < 2^30 (the record's limbs are in [0, 2^29), its
// negated y in (-2^29, 0]; as the accumulator's y it is normalised first, so R = S2 - Y1 keeps |l| < 2^29 for the square).
// The unit form on a native record takes x2 for U2 as it is (P = x2 - x1, |l| < 2^29) and normalises +-y2 for S2 (R = S2 - y1, |l| < 2^29).
#pragma once
#include "ec.h"
#include "fieldu.h"

namespace h2 {

typedef FqU QU;

struct XYZZu {
    Fu x, y, zz, zzz;
};

H2_HD XYZZu xyzzu_identity() {
    XYZZu o;
    o.x = fu_zero();
    o.y = fu_zero();
    o.zz = fu_zero();
    o.zzz = fu_zero();
    return o;
}

H2_HD bool xyzzu_is_identity(const XYZZu& p) { return fu_all_zero(p.zz); }

// The three functions of the bucket-accumulation inner loop take the field flavour as a template parameter: the
// accumulate kernel instantiates them with FqUA (explicit-mad multiplier), everything else with QU.

// 2 * (x, y) for a non-identity affine point in I-form with normalised coordinates, |x|, |y| < 1.2 p (mdbl-2008-s-1)
template <class QU = FqU>
H2_HD XYZZu xyzzu_double_affine_reduced(const Fu& x, const Fu& y) {
    XYZZu o;
    Fu u = fu_norm(fu_dbl(y));
    Fu v = fu_sqr<QU>(u);
    Fu w = fu_mul<QU>(u, v);
    Fu s = fu_mul<QU>(x, v);
    Fu xx = fu_sqr<QU>(x);
    Fu m = fu_norm(fu_add(fu_dbl(xx), xx));
    o.x = fu_sqr_sub<QU>(m, fu_dbl(s));                       // M^2 - 2S, one reduction, normalised
    o.y = fu_mul_sub<QU>(m, fu_sub(s, o.x), w, y);            // M*(S - X3) - W*Y1, one reduction
    o.zz = v;
    o.zzz = w;
    return o;
}

// the same for fu_from_ext output (32x, 32y, |.| < 32 p)
template <class QU = FqU>
H2_HD XYZZu xyzzu_double_affine(const Fu& px, const Fu& py) {
    const Fu one = fu_one_i<QU>();
    return xyzzu_double_affine_reduced<QU>(fu_mul<QU>(px, one), fu_mul<QU>(py, one));  // 32x -> (-0.2 p, 1.2 p), same residue
}

// dbl-2008-s-1
template <class QU = FqU>
H2_HD XYZZu xyzzu_double(const XYZZu& p) {
    if (xyzzu_is_identity(p)) return p;
    XYZZu o;
    Fu u = fu_norm(fu_dbl(p.y));
    Fu v = fu_sqr<QU>(u);
    Fu w = fu_mul<QU>(u, v);
    Fu s = fu_mul<QU>(p.x, v);
    Fu xx = fu_sqr<QU>(p.x);
    Fu m = fu_norm(fu_add(fu_dbl(xx), xx));
    o.x = fu_sqr_sub<QU>(m, fu_dbl(s));
    o.y = fu_mul_sub<QU>(m, fu_sub(s, o.x), w, p.y);
    o.zz = fu_mul<QU>(v, p.zz);
    o.zzz = fu_mul<QU>(w, p.zzz);
    return o;
}

// acc += (px, py) for an accumulator that is NOT the identity: madd-2008-s.  (px, py) is a non-identity affine point in I-form with
// limbs of magnitude < 2^29: fu_from_ext output, possibly negated (REDUCED = false: |32 x| < 32 p), or the coordinates of a native
// table record, y possibly negated (REDUCED = true: |x|, |y| < p).  All exceptional cases of the group law are exact: the cheap
// residue filter on P sends possible hits to an exact reduction.  Returns false when the sum is the identity (acc is then marked so).
// `unit`: the caller knows that acc is a unit point, zz = zzz = one exactly, as the copy of a bucket's first record leaves it.  The four
// products by zz and zzz are known then and are not formed: U2 = px, S2 = py, ZZ3 = PP, ZZZ3 = PPP (mmadd-2008-s: 1 square, 2 products,
// fu_sqr_sub, fu_mul_sub).  Without REDUCED U2 = px * one and S2 = py * one stay, because that product is what brings 32x inside the
// bounds, and only the last two go.  Everything between is one body for both, so the flag costs two short branches and no second copy of
// the addition; on the device the caller passes a value that is the same in all lanes of the wave (xyzzu_none below).
template <class QU, bool REDUCED>
H2_HD bool xyzzu_add_mixed_nonid(XYZZu& acc, const Fu& px, const Fu& py, bool unit) {
    Fu u2, s2;
    if (REDUCED && unit) {
        u2 = px;
        s2 = fu_norm(py);
    } else {
        u2 = fu_mul<QU>(px, acc.zz);
        s2 = fu_mul<QU>(py, acc.zzz);
    }
    Fu p_ = fu_sub(u2, acc.x);
    Fu r = fu_sub(s2, acc.y);
    if (fu_maybe_zero_mod_p<QU>(p_)) {
        if (fu_is_zero_mod_p<QU>(p_)) {
            if (fu_is_zero_mod_p<QU>(r)) {
                if constexpr (REDUCED) acc = xyzzu_double_affine_reduced<QU>(px, fu_norm(py));
                else acc = xyzzu_double_affine<QU>(px, py);
                return true;
            }
            acc = xyzzu_identity();
            return false;
        }
    }
    Fu pp = fu_sqr<QU>(p_);
    Fu ppp = fu_mul<QU>(p_, pp);
    Fu q = fu_mul<QU>(acc.x, pp);
    Fu x3 = fu_sqr_sub<QU>(r, fu_add(ppp, fu_dbl(q)));    // R^2 - PPP - 2Q, one reduction, already normalised
    Fu t = fu_sub(q, x3);
    Fu y3 = fu_mul_sub<QU>(r, t, acc.y, ppp);             // R*(Q - X3) - Y1*PPP, one reduction
    acc.x = x3;
    acc.y = y3;
    if (unit) {
        acc.zz = pp;
        acc.zzz = ppp;
    } else {
        acc.zz = fu_mul<QU>(acc.zz, pp);
        acc.zzz = fu_mul<QU>(acc.zzz, ppp);
    }
    return true;
}

template <class QU, bool REDUCED>
H2_HD bool xyzzu_add_mixed_nonid(XYZZu& acc, const Fu& px, const Fu& py) {
    return xyzzu_add_mixed_nonid<QU, REDUCED>(acc, px, py, false);
}

// The accumulate loops keep what they know of an accumulator in one word beside it, so that a lane tests a word instead of or-ing the
// limbs of zz: ACC_IDENTITY for a fresh accumulator or after a cancellation, ACC_UNIT between the copy of a bucket's first point and the
// next addition, ACC_POINT otherwise (and for an accumulator loaded from memory that is not the identity).  ACC_IDENTITY is the only odd
// value: xyzzu_add_native(acc, acc_id, ...) below keeps the same word with the values 0 and 1.
enum : uint32_t { ACC_POINT = 0, ACC_IDENTITY = 1, ACC_UNIT = 2 };

// No active lane has `pred` set?  On the device the answer is the same in all lanes of the wave (a ballot), so a branch on it is a scalar
// one; the host runs one lane.  The unit form is taken only when EVERY lane that adds has a unit accumulator: a wave whose lanes differ
// would otherwise run both forms in sequence, and the general form is correct for a unit accumulator too.
H2_HD bool xyzzu_none(bool pred) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(pred) == 0;
#else
    return !pred;
#endif
}

// acc += (px, py), fu_from_ext output (possibly negated), any accumulator
template <class QU = FqU>
H2_HD void xyzzu_add_mixed(XYZZu& acc, const Fu& px, const Fu& py) {
    if (xyzzu_is_identity(acc)) {
        // first point of a bucket: bring 32x, 32y (|.| < 32 p) inside the accumulator bounds
        const Fu one = fu_one_i<QU>();
        acc.x = fu_mul<QU>(px, one);
        acc.y = fu_mul<QU>(py, one);
        acc.zz = one;
        acc.zzz = one;
        return;
    }
    xyzzu_add_mixed_nonid<QU, false>(acc, px, py);
}

// The same with the accumulator's state word (ACC_*) kept beside it; `skip`: this lane has nothing to add (an identity point).  It is a
// parameter because the lanes decide together which form the addition takes, before they part ways.
template <class QU = FqU>
H2_HD void xyzzu_add_mixed(XYZZu& acc, uint32_t& acc_st, const Fu& px, const Fu& py, bool skip) {
    const bool adds = !skip && !(acc_st & 1);
    const bool unit = xyzzu_none(adds && acc_st != ACC_UNIT);
    if (adds) {
        acc_st = xyzzu_add_mixed_nonid<QU, false>(acc, px, py, unit) ? ACC_POINT : ACC_IDENTITY;
    } else if (!skip) {
        // first point of a bucket: bring 32x, 32y (|.| < 32 p) inside the accumulator bounds
        const Fu one = fu_one_i<QU>();
        acc.x = fu_mul<QU>(px, one);
        acc.y = fu_mul<QU>(py, one);
        acc.zz = one;
        acc.zzz = one;
        acc_st = ACC_UNIT;
    }
}

// a += b: add-2008-s with exceptional cases
template <class QU = FqU>
H2_HD void xyzzu_add(XYZZu& a, const XYZZu& b) {
    if (xyzzu_is_identity(b)) return;
    if (xyzzu_is_identity(a)) {
        a = b;
        return;
    }
    Fu u1 = fu_mul<QU>(a.x, b.zz);
    Fu u2 = fu_mul<QU>(b.x, a.zz);
    Fu s1 = fu_mul<QU>(a.y, b.zzz);
    Fu s2 = fu_mul<QU>(b.y, a.zzz);
    Fu p_ = fu_sub(u2, u1);
    Fu r = fu_sub(s2, s1);
    if (fu_maybe_zero_mod_p<QU>(p_)) {
        if (fu_is_zero_mod_p<QU>(p_)) {
            if (fu_is_zero_mod_p<QU>(r)) {
                a = xyzzu_double<QU>(a);
            } else {
                a = xyzzu_identity();
            }
            return;
        }
    }
    Fu pp = fu_sqr<QU>(p_);
    Fu ppp = fu_mul<QU>(p_, pp);
    Fu q = fu_mul<QU>(u1, pp);
    Fu x3 = fu_sqr_sub<QU>(r, fu_add(ppp, fu_dbl(q)));
    Fu t = fu_sub(q, x3);
    Fu y3 = fu_mul_sub<QU>(r, t, s1, ppp);
    a.x = x3;
    a.y = y3;
    a.zz = fu_mul<QU>(fu_mul<QU>(a.zz, b.zz), pp);
    a.zzz = fu_mul<QU>(fu_mul<QU>(a.zzz, b.zzz), ppp);
}

// acc += p for an affine point in the reference's layout (E-form Fe, identity = (0,0)), optionally negated
template <class QU = FqU>
H2_HD void xyzzu_add_affine(XYZZu& acc, const Affine& p, bool negate) {
    if (affine_is_identity(p)) return;
    Fu px = fu_from_ext(p.x);
    Fu py = fu_from_ext(p.y);
    if (negate) py = fu_neg(py);
    xyzzu_add_mixed<QU>(acc, px, py);
}

template <class QU = FqU>
H2_HD void xyzzu_add_affine(XYZZu& acc, uint32_t& acc_st, const Affine& p, bool negate) {
    Fu px = fu_from_ext(p.x);
    Fu py = fu_from_ext(p.y);
    if (negate) py = fu_neg(py);
    xyzzu_add_mixed<QU>(acc, acc_st, px, py, affine_is_identity(p));
}

// ---- native records of the fixed-base window table ----------------------------------------------------------------------------
// The table is the engine's own data, built once at pin time, so its records are kept in the form xyzzu_add_mixed_nonid multiplies:
// both coordinates I-form and canonical (the integer in [0, p)) as 9 limbs of 29 bits, limbs 0..7 in [0, 2^29), top limb in [0, 2^22).
// `valid` is 1 for a point of the curve; the identity is the all-zero record.  80 bytes: five 16-byte pieces for the accumulate kernel's
// LDS-DMA fetch; in the table the records lie a 128-byte line apart (engine.h H2_TABLE_REC_NATIVE).  Against an E-form Affine the kernel saves fu_from_ext on both coordinates, and the first point of a bucket needs no
// product: x, +-y, one, one are inside the accumulator's bounds as they are.
struct AffineU {
    Fu x, y;
    uint32_t valid, pad;
};
static_assert(sizeof(AffineU) == 80, "five 16-byte pieces");

// E-form Fe (canonical) -> the canonical I-form limbs of a native record, and back
H2_HD Fu fu_native_from_ext(const Fe& e) { return fu_slice(fu_canon<QU>(fu_mul<QU>(fu_from_ext(e), fu_one_i<QU>()))); }
H2_HD Fe fu_native_to_ext(const Fu& a) { return fu_mul_canon<QU>(a, fu_one_e<QU>()); }

H2_HD AffineU affineu_from_ext(const Affine& p) {
    AffineU o;
    const bool id = affine_is_identity(p);
    o.x = id ? fu_zero() : fu_native_from_ext(p.x);
    o.y = id ? fu_zero() : fu_native_from_ext(p.y);
    o.valid = id ? 0u : 1u;
    o.pad = 0;
    return o;
}

H2_HD Affine affineu_to_ext(const AffineU& p) {
    Affine o;
    if (!p.valid) {
        o.x = fe_zero<Q>();
        o.y = fe_zero<Q>();
        return o;
    }
    o.x = fu_native_to_ext(p.x);
    o.y = fu_native_to_ext(p.y);
    return o;
}

// acc += +-p for a native record.  acc_st (ACC_*) says what the caller knows of acc: it sets the word once (ACC_IDENTITY for a fresh
// accumulator, ACC_POINT or ACC_IDENTITY for one loaded from memory) and this function keeps it, so the loop tests one word against the
// record's marker instead of or-ing the nine limbs of zz and the sixteen words of the point on every entry.  The copy of a first record
// leaves ACC_UNIT, and the addition that follows takes the unit form when all the lanes that add are in that state.  The sign is applied
// without a branch: (y ^ m) - m with m = 0 or -1.
template <class QU = FqU>
H2_HD void xyzzu_add_native_st(XYZZu& acc, uint32_t& acc_st, const AffineU& p, bool negate) {
    const int32_t m = -(int32_t)negate, one_if = (int32_t)negate;
    Fu py;
#pragma unroll
    for (int i = 0; i < 9; i++) py.l[i] = (p.y.l[i] ^ m) + one_if;  // |l| < 2^29, |value| < p
    const bool adds = p.valid > (acc_st & 1);
    const bool unit = xyzzu_none(adds && acc_st != ACC_UNIT);
    if (!adds) {  // rare: an identity record (nothing to add), or an identity accumulator (the first point of a bucket, or after a cancellation)
        if (p.valid) {
            acc.x = p.x;
            acc.y = fu_norm(py);  // limbs 0..7 back in [0, 2^29): the accumulator's invariant
            acc.zz = fu_one_i<QU>();
            acc.zzz = acc.zz;
            acc_st = ACC_UNIT;
        }
        return;
    }
    acc_st = xyzzu_add_mixed_nonid<QU, true>(acc, p.x, py, unit) ? ACC_POINT : ACC_IDENTITY;
}

// The same with a two-valued word, acc_id = 1 while acc is the identity and 0 otherwise: the unit state is forgotten between calls, so
// every addition takes the general form.  No kernel calls it; tests/cpp/test_ecu_native.cpp does.
template <class QU = FqU>
H2_HD void xyzzu_add_native(XYZZu& acc, uint32_t& acc_id, const AffineU& p, bool negate) {
    uint32_t st = acc_id;
    xyzzu_add_native_st<QU>(acc, st, p, negate);
    acc_id = st & 1;
}

// I-form accumulator -> the E-form XYZZ of ec.h with canonical coordinates
H2_HD XYZZ xyzzu_to_ext(const XYZZu& p) {
    if (xyzzu_is_identity(p)) return xyzz_identity();
    XYZZ o;
    const Fu one_e = fu_one_e<QU>();
    o.x = fu_mul_canon<QU>(p.x, one_e);
    o.y = fu_mul_canon<QU>(p.y, one_e);
    o.zz = fu_mul_canon<QU>(p.zz, one_e);
    o.zzz = fu_mul_canon<QU>(p.zzz, one_e);
    return o;
}

H2_HD XYZZu xyzzu_from_ext(const XYZZ& p) {
    XYZZu o;
    if (xyzz_is_identity(p)) return xyzzu_identity();
    const Fu one = fu_one_i<QU>();
    o.x = fu_mul<QU>(fu_from_ext(p.x), one);
    o.y = fu_mul<QU>(fu_from_ext(p.y), one);
    o.zz = fu_mul<QU>(fu_from_ext(p.zz), one);
    o.zzz = fu_mul<QU>(fu_from_ext(p.zzz), one);
    return o;
}

// k * p for a small non-negative integer k < 2^nbits (double-and-add, vartime)
H2_HD XYZZu xyzzu_mul_small(const XYZZu& p, uint32_t k, uint32_t nbits = 32) {
    XYZZu acc = xyzzu_identity();
    for (int i = (int)nbits - 1; i >= 0; i--) {
        acc = xyzzu_double(acc);
        if ((k >> i) & 1) xyzzu_add(acc, p);
    }
    return acc;
}

// k * p for k < 32 (5-bit double-and-add)
H2_HD XYZZu xyzzu_mul_small5(const XYZZu& p, uint32_t k) {
    XYZZu acc = xyzzu_identity();
    for (int i = 4; i >= 0; i--) {
        acc = xyzzu_double(acc);
        if ((k >> i) & 1) xyzzu_add(acc, p);
    }
    return acc;
}

}  // namespace h2
