// ipa_elem.h -- what ipa.hip's kernels do to ONE element, host and device: the uniform-scalar ladder of the generator collapse
// (poly/ipa/commitment/prover.rs:155-167), the fold of the two scalar vectors (:118-131), and the byte-table product behind both
// compute_s (poly/ipa/strategy.rs:161-176) and the powers of x_3 (the vector b, prover.rs:84-91).  Kept apart from the kernels so that
// tests/cpp/test_ipa_host.cpp runs the same source on the host with H2_FU_CHECK, where every product asserts fieldu.h's limb bounds.
#pragma once
#include "ecu.h"
#include "glv.h"

namespace h2 {

// ---- the collapse's scalar, recoded once on the host ----------------------------------------------------------------------------------
// u = k1 + k2 * LAMBDA (glv.h), |k1|, |k2| < 2^130, and the pair (|k1|, |k2|) in joint sparse form (Solinas, "Low-weight binary
// representations for pairs of integers"): signed digits d1, d2 in {-1, 0, 1}, at most one column in two non-zero.  The scalar is the
// same for every point of a collapse, so every lane walks the same columns and a wave never diverges: where the per-lane digits of
// ecfft.hip's ladder need a 15-entry table indexed at run time (scratch memory), a uniform branch picks one of four per-lane points
// that live in registers: p1 = +-p, p2 = +-phi(p) (mixed additions), p1 + p2, p1 - p2 (general additions), each possibly negated.
#define IPA_MAX_COLUMNS 132
struct IpaDigits {
    uint32_t w[(IPA_MAX_COLUMNS * 4 + 31) / 32];  // column j: bits [4 j, 4 j + 4) = (d1 + 1) | (d2 + 1) << 2
    uint32_t len;                                 // columns; 0 for u = 0
    uint32_t neg1, neg2;                          // the signs of k1, k2: they go into p1, p2
};

namespace ipa {
H2_HD bool nonzero5(const uint32_t a[5]) { return (a[0] | a[1] | a[2] | a[3] | a[4]) != 0; }
H2_HD void shr5(uint32_t a[5]) {
    for (int i = 0; i < 4; i++) a[i] = a[i] >> 1 | a[i + 1] << 31;
    a[4] >>= 1;
}
// the digit of l, given the other scalar's l (both mod 8, carries included)
H2_HD int jsf_digit(uint32_t l, uint32_t other) {
    if (!(l & 1)) return 0;
    int u = (l & 3) == 1 ? 1 : -1;
    if (((l & 7) == 3 || (l & 7) == 5) && (other & 3) == 2) u = -u;
    return u;
}
}  // namespace ipa

// k: canonical scalar (< r), 8 little-endian 32-bit limbs
H2_HD IpaDigits ipa_digits(const uint32_t k[8]) {
    const GlvScalar g = glv_decompose(k);
    uint32_t a[5], b[5];
    for (int i = 0; i < 5; i++) a[i] = g.k1[i], b[i] = g.k2[i];
    IpaDigits o;
    for (uint32_t i = 0; i < sizeof(o.w) / 4; i++) o.w[i] = 0;
    o.neg1 = g.neg1;
    o.neg2 = g.neg2;
    uint32_t ca = 0, cb = 0, j = 0;
    while (j < IPA_MAX_COLUMNS && (ipa::nonzero5(a) || ipa::nonzero5(b) || ca || cb)) {
        const uint32_t la = (a[0] & 7) + ca, lb = (b[0] & 7) + cb;
        const int ua = ipa::jsf_digit(la, lb), ub = ipa::jsf_digit(lb, la);
        o.w[j >> 3] |= ((uint32_t)(ua + 1) | (uint32_t)(ub + 1) << 2) << ((j & 7) * 4);
        if (2 * (int)ca == 1 + ua) ca = 1 - ca;
        if (2 * (int)cb == 1 + ub) cb = 1 - cb;
        ipa::shr5(a);
        ipa::shr5(b);
        j++;
    }
    o.len = j;
    return o;
}

H2_HD uint32_t ipa_column(const IpaDigits& dg, uint32_t j) { return (dg.w[j >> 3] >> ((j & 7) * 4)) & 15; }

// the four per-lane points of a ladder: p1 = (x1, y1) and p2 = (x2, y2) as xyzzu_add_mixed takes them, s = p1 + p2, d = p1 - p2
struct IpaBase {
    Fu x1, y1, x2, y2;
    XYZZu s, d;
};

// p: an affine point that is not the identity
H2_HD IpaBase ipa_base(const Affine& p, const IpaDigits& dg) {
    const uint32_t BETA_I[9] = {0x0a337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu, 0x0176f16du, 0x0eed93bau, 0x14291140u, 0x000c0afeu};
    IpaBase t;
    t.x1 = fu_from_ext(p.x);
    t.y1 = fu_from_ext(p.y);
    t.y2 = t.y1;
    t.x2 = fu_mul<QU>(t.x1, fu_const<QU>(BETA_I));  // I-form of BETA * x, in (-0.2 q, 1.2 q)
    if (dg.neg1) t.y1 = fu_neg(t.y1);
    if (dg.neg2) t.y2 = fu_neg(t.y2);
    t.s = xyzzu_identity();
    xyzzu_add_mixed<QU>(t.s, t.x1, t.y1);
    t.d = t.s;
    xyzzu_add_mixed<QU>(t.s, t.x2, t.y2);
    xyzzu_add_mixed<QU>(t.d, t.x2, fu_neg(t.y2));
    return t;
}

// One column of the ladder: acc <- 2 acc + d1 p1 + d2 p2.  `col` is the same in every lane, so the branches are scalar ones.
H2_HD void ipa_ladder_step(XYZZu& acc, const IpaBase& t, uint32_t col) {
    acc = xyzzu_double(acc);
    const int d1 = (int)(col & 3) - 1, d2 = (int)(col >> 2) - 1;
    if (d1 != 0 && d2 != 0) {
        XYZZu q = d1 == d2 ? t.s : t.d;
        if (d1 < 0) q.y = fu_norm(fu_neg(q.y));
        xyzzu_add(acc, q);
    } else if (d1 != 0) {
        xyzzu_add_mixed<QU>(acc, t.x1, d1 < 0 ? fu_neg(t.y1) : t.y1);
    } else if (d2 != 0) {
        xyzzu_add_mixed<QU>(acc, t.x2, d2 < 0 ? fu_neg(t.y2) : t.y2);
    }
}

// [u] p for an affine p (E-form, identity = (0, 0)) and the recoded u
H2_HD XYZZu ipa_mul_affine(const Affine& p, const IpaDigits& dg) {
    XYZZu acc = xyzzu_identity();
    if (dg.len == 0 || affine_is_identity(p)) return acc;
    const IpaBase t = ipa_base(p, dg);
    for (int j = (int)dg.len - 1; j >= 0; j--) ipa_ladder_step(acc, t, ipa_column(dg, (uint32_t)j));
    return acc;
}

// g[i] <- g[i] + [u] g[half + i], still XYZZ: the closing addition is ec.h's complete mixed addition, because lo = +-[u] hi and an
// identity on either side are legal inputs
H2_HD XYZZ ipa_collapse_elem(const Affine& lo, const Affine& hi, const IpaDigits& dg) {
    XYZZ t = xyzzu_to_ext(ipa_mul_affine(hi, dg));
    xyzz_add_mixed(t, lo);
    return t;
}

// ---- Fr: every value below is a canonical E-form Fe (what the reference stores) ---------------------------------------------------------
// a * b: fu_from_ext(a) is the I-form of a for free (32 a < 32 r, limbs < 2^29), fu_slice(b) keeps b's form, the product is E-form in
// [0, 1.25 r) and one fast reduction makes it canonical
H2_HD Fe ipa_fr_mul(const Fe& a, const Fe& b) { return fu_canon_fast<FrU>(fu_mul<FrU>(fu_from_ext(a), fu_slice(b))); }

// lo + c * hi, the fold of one element (c = u_j^-1 for the polynomial, u_j for b): the product in [0, 1.25 r) plus lo < r, one reduction
H2_HD Fe ipa_fold_elem(const Fe& lo, const Fe& hi, const Fe& c) {
    return fu_canon_fast<FrU>(fu_add(fu_mul<FrU>(fu_from_ext(c), fu_slice(hi)), fu_slice(lo)));
}

// Byte tables: element i of a vector whose entry is a product over the bits (compute_s) or the bytes (powers) of its index is
// prod_{l < levels} T[256 l + byte l of i]: levels - 1 products per element from at most 4 x 256 entries
#define IPA_TABLE_LEVELS 4
#define IPA_TABLE_ELEMS (IPA_TABLE_LEVELS * 256)
H2_HD Fe ipa_table_elem(const Fe* T, uint32_t levels, uint64_t i) {
    Fe acc = T[i & 255];
    for (uint32_t l = 1; l < levels; l++) acc = ipa_fr_mul(acc, T[256 * l + ((i >> (8 * l)) & 255)]);
    return acc;
}

// the table of x^i, i < n (n <= 2^32): T[256 l + d] = x^(d 256^l); returns the levels
H2_HD uint32_t ipa_powers_table(const Fe& x, uint64_t n, Fe* T) {
    uint32_t levels = 1;
    while (levels < IPA_TABLE_LEVELS && ((n - 1) >> (8 * levels)) != 0) levels++;
    Fe base = x;
    for (uint32_t l = 0; l < levels; l++) {
        T[256 * l] = fe_one<FrP>();
        for (uint32_t d = 1; d < 256; d++) T[256 * l + d] = ipa_fr_mul(T[256 * l + d - 1], base);
        base = ipa_fr_mul(T[256 * l + 255], base);
    }
    return levels;
}

// the table of compute_s: s[i] = init * prod_{t < k, bit t of i set} u[k - 1 - t]  (strategy.rs:161-176: the outer loop runs over the
// challenges in reverse, and each doubles the filled prefix); T[256 l + d] = prod_{bit t of d set, 8 l + t < k} u[k - 1 - 8 l - t], the
// level-0 entries times init.  1 <= k <= 28; returns the levels
H2_HD uint32_t ipa_s_table(const Fe* u, uint32_t k, const Fe& init, Fe* T) {
    const uint32_t levels = (k + 7) / 8;
    for (uint32_t l = 0; l < levels; l++) {
        T[256 * l] = l == 0 ? init : fe_one<FrP>();
        for (uint32_t d = 1; d < 256; d++) {
            uint32_t t = 0;
            while (!((d >> t) & 1)) t++;
            const Fe rest = T[256 * l + (d & (d - 1))];
            T[256 * l + d] = 8 * l + t < k ? ipa_fr_mul(rest, u[k - 1 - 8 * l - t]) : rest;
        }
    }
    return levels;
}

}  // namespace h2
