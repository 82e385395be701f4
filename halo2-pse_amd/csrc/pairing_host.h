// pairing_host.h -- the BN254 optimal ate pairing and G2 arithmetic on the calling thread (include/halo2hip_pairing.h), over host64.h's
// 4 x 64 Montgomery field.  Host only: no HIP call, no engine state, no lock, re-entrant; the constants are built once (a function-local
// static).  Variable-time: every input of a verifier is public.  The library's entry points and tests/cpp/test_pairing_host.cpp share
// this one definition.
//
//   Fq2 = Fq[u] / (u^2 + 1),   Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u,   Fq12 = Fq6[w] / (w^2 - v)
//   G2: y^2 = x^3 + 3 / xi over Fq2 (the D-type twist); (x', y') untwists to (x' w^2, y' w^3)
//   e(P, Q) = ( f_{6t+2,Q}(P) * l_{T,pi(Q)}(P) * l_{T+pi(Q),-pi^2(Q)}(P) )^((q^12 - 1) / r),   t = 4965661367192848881
//
// An Fq12 element is sum_{i<6} z_i w^i with z_i in Fq2: z_0, z_2, z_4 are c0's coefficients of 1, v, v^2 and z_1, z_3, z_5 are c1's.
// A line through twist points is l(P) = y_P - lambda' x_P w + (lambda' x'_T - y'_T) w^3 times a factor in Fq2: three of the six z_i
// (0, 1, 3), which mul_by_line uses.  The Miller loop keeps T in homogeneous projective coordinates, so a step has no inversion; the
// factors this leaves in Fq2 are killed by the easy part of the exponent.
// The exponent is exactly (q^12 - 1) / r: the easy part (q^6 - 1)(q^2 + 1), then
//   (q^4 - q^2 + 1) / r = q^3 + (6t^2 + 1) q^2 + (-36t^3 - 18t^2 - 12t + 1) q + (-36t^3 - 30t^2 - 18t - 2)
// through f^t, f^(t^2), f^(t^3) (cyclotomic squarings), three Frobenius maps and the addition chain of Scott et al. (2009).
#pragma once
#include <stdio.h>

#include <vector>

#include "g1_host.h"

namespace h2 {
namespace pairing {

using h64::F;
typedef unsigned __int128 u128;

static const uint64_t BN_T = 4965661367192848881ULL;
static const size_t MAX_PAIRS = 65536;  // a batch beyond this is folded first (a random linear combination, two MSMs)

// ---- Fq helpers ----------------------------------------------------------------------------------------------------------------------
static inline F f_zero() {
    F o;
    memset(&o, 0, sizeof(o));
    return o;
}
static inline F f_neg(const F& a) { return h64::sub(f_zero(), a); }
static inline bool f_eq(const F& a, const F& b) { return memcmp(&a, &b, 32) == 0; }
static inline F f_small(uint64_t v) {  // v in Montgomery form
    F c = {{v, 0, 0, 0}}, r2;
    memcpy(&r2, Q::R2, 32);
    return h64::mul(c, r2);
}
static inline bool f_canonical(const uint64_t a[4]) { return !h64::geq(a); }

// ---- Fq2 -----------------------------------------------------------------------------------------------------------------------------
struct F2 {
    F c0, c1;
};
static inline F2 f2_zero() { return {f_zero(), f_zero()}; }
static inline F2 f2_one() { return {g1h::f_one(), f_zero()}; }
static inline bool f2_is_zero(const F2& a) { return h64::is_zero(a.c0) && h64::is_zero(a.c1); }
static inline bool f2_eq(const F2& a, const F2& b) { return f_eq(a.c0, b.c0) && f_eq(a.c1, b.c1); }
static inline F2 f2_add(const F2& a, const F2& b) { return {h64::add(a.c0, b.c0), h64::add(a.c1, b.c1)}; }
static inline F2 f2_sub(const F2& a, const F2& b) { return {h64::sub(a.c0, b.c0), h64::sub(a.c1, b.c1)}; }
static inline F2 f2_dbl(const F2& a) { return f2_add(a, a); }
static inline F2 f2_neg(const F2& a) { return {f_neg(a.c0), f_neg(a.c1)}; }
static inline F2 f2_conj(const F2& a) { return {a.c0, f_neg(a.c1)}; }
static inline F2 f2_mul(const F2& a, const F2& b) {  // Karatsuba: three products
    F v0 = h64::mul(a.c0, b.c0), v1 = h64::mul(a.c1, b.c1);
    F s = h64::mul(h64::add(a.c0, a.c1), h64::add(b.c0, b.c1));
    return {h64::sub(v0, v1), h64::sub(h64::sub(s, v0), v1)};
}
static inline F2 f2_sqr(const F2& a) {  // (a0 + a1)(a0 - a1) + 2 a0 a1 u
    F p = h64::mul(a.c0, a.c1);
    return {h64::mul(h64::add(a.c0, a.c1), h64::sub(a.c0, a.c1)), h64::dbl(p)};
}
static inline F2 f2_scale(const F2& a, const F& s) { return {h64::mul(a.c0, s), h64::mul(a.c1, s)}; }
static inline F2 f2_mul_xi(const F2& a) {  // (9 + u)(a0 + a1 u) = (9 a0 - a1) + (a0 + 9 a1) u
    F a8 = h64::dbl(h64::dbl(h64::dbl(a.c0))), b8 = h64::dbl(h64::dbl(h64::dbl(a.c1)));
    return {h64::sub(h64::add(a8, a.c0), a.c1), h64::add(h64::add(b8, a.c1), a.c0)};
}
static inline F2 f2_inv(const F2& a) {  // conj(a) / (a0^2 + a1^2); 0 -> 0
    F d = g1h::f_inv(h64::add(h64::sqr(a.c0), h64::sqr(a.c1)));
    return {h64::mul(a.c0, d), f_neg(h64::mul(a.c1, d))};
}
static inline F2 f2_pow(const F2& a, const uint64_t* e, int limbs) {
    F2 r = f2_one();
    for (int i = 64 * limbs - 1; i >= 0; i--) {
        r = f2_sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = f2_mul(r, a);
    }
    return r;
}

// ---- Fq6 -----------------------------------------------------------------------------------------------------------------------------
struct F6 {
    F2 c0, c1, c2;
};
static inline F6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
static inline F6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
static inline F6 f6_add(const F6& a, const F6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
static inline F6 f6_sub(const F6& a, const F6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
static inline F6 f6_neg(const F6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
static inline bool f6_eq(const F6& a, const F6& b) { return f2_eq(a.c0, b.c0) && f2_eq(a.c1, b.c1) && f2_eq(a.c2, b.c2); }
static inline F6 f6_mul_v(const F6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }
static inline F6 f6_mul(const F6& a, const F6& b) {  // Karatsuba: six Fq2 products
    F2 v0 = f2_mul(a.c0, b.c0), v1 = f2_mul(a.c1, b.c1), v2 = f2_mul(a.c2, b.c2);
    F2 t0 = f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), v1), v2);
    F2 t1 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), v0), v1);
    F2 t2 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), v0), v2);
    return {f2_add(v0, f2_mul_xi(t0)), f2_add(t1, f2_mul_xi(v2)), f2_add(t2, v1)};
}
static inline F6 f6_sqr(const F6& a) { return f6_mul(a, a); }
static inline F6 f6_scale(const F6& a, const F2& s) { return {f2_mul(a.c0, s), f2_mul(a.c1, s), f2_mul(a.c2, s)}; }
// a * (b0 + b1 v)
static inline F6 f6_mul_by_01(const F6& a, const F2& b0, const F2& b1) {
    return {f2_add(f2_mul(a.c0, b0), f2_mul_xi(f2_mul(a.c2, b1))), f2_add(f2_mul(a.c0, b1), f2_mul(a.c1, b0)),
            f2_add(f2_mul(a.c1, b1), f2_mul(a.c2, b0))};
}
static inline F6 f6_inv(const F6& a) {
    F2 t0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    F2 t1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    F2 t2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    F2 d = f2_add(f2_mul(a.c0, t0), f2_mul_xi(f2_add(f2_mul(a.c2, t1), f2_mul(a.c1, t2))));
    return f6_scale({t0, t1, t2}, f2_inv(d));
}

// ---- Fq12 ----------------------------------------------------------------------------------------------------------------------------
struct F12 {
    F6 c0, c1;
};
static inline F12 f12_one() { return {f6_one(), f6_zero()}; }
static inline bool f12_eq(const F12& a, const F12& b) { return f6_eq(a.c0, b.c0) && f6_eq(a.c1, b.c1); }
static inline bool f12_is_one(const F12& a) { return f12_eq(a, f12_one()); }
// z_i, the coefficient of w^i
static inline F2& f12_coeff(F12& a, int i) {
    F6& h = (i & 1) ? a.c1 : a.c0;
    return i >> 1 == 0 ? h.c0 : (i >> 1 == 1 ? h.c1 : h.c2);
}
static inline F12 f12_mul(const F12& a, const F12& b) {
    F6 v0 = f6_mul(a.c0, b.c0), v1 = f6_mul(a.c1, b.c1);
    F6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1));
    return {f6_add(v0, f6_mul_v(v1)), f6_sub(f6_sub(s, v0), v1)};
}
static inline F12 f12_sqr(const F12& a) {  // (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1, 2 a0 a1
    F6 ab = f6_mul(a.c0, a.c1);
    F6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return {f6_sub(f6_sub(s, ab), f6_mul_v(ab)), f6_add(ab, ab)};
}
static inline F12 f12_conj(const F12& a) { return {a.c0, f6_neg(a.c1)}; }  // the q^6-power map
static inline F12 f12_inv(const F12& a) {
    F6 d = f6_inv(f6_sub(f6_sqr(a.c0), f6_mul_v(f6_sqr(a.c1))));
    return {f6_mul(a.c0, d), f6_neg(f6_mul(a.c1, d))};
}
// a * (l0 + l1 w + l3 w^3): a's product with c0 = (l0, 0, 0), c1 = (l1, l3, 0)
static inline F12 f12_mul_by_line(const F12& a, const F2& l0, const F2& l1, const F2& l3) {
    F6 v0 = f6_scale(a.c0, l0), v1 = f6_mul_by_01(a.c1, l1, l3);
    F6 s = f6_mul_by_01(f6_add(a.c0, a.c1), f2_add(l0, l1), l3);
    return {f6_add(v0, f6_mul_v(v1)), f6_sub(f6_sub(s, v0), v1)};
}
// a^2 for a in the cyclotomic subgroup (a^(q^6 + 1) = ... = 1 after the easy part): Granger-Scott, three Fq4 squarings
static inline void fp4_sqr(const F2& a, const F2& b, F2& t0, F2& t1) {  // (a + b y)^2, y^2 = xi
    F2 ab = f2_mul(a, b);
    t0 = f2_sub(f2_sub(f2_mul(f2_add(a, b), f2_add(f2_mul_xi(b), a)), ab), f2_mul_xi(ab));
    t1 = f2_dbl(ab);
}
static inline F12 f12_cyclotomic_sqr(const F12& a) {
    const F2 &r0 = a.c0.c0, &r4 = a.c0.c1, &r3 = a.c0.c2, &r2 = a.c1.c0, &r1 = a.c1.c1, &r5 = a.c1.c2;
    F2 t0, t1, t2, t3, t4, t5;
    fp4_sqr(r0, r1, t0, t1);
    fp4_sqr(r2, r3, t2, t3);
    fp4_sqr(r4, r5, t4, t5);
    F2 x5 = f2_mul_xi(t5);
    auto minus = [](const F2& t, const F2& z) { return f2_add(f2_dbl(f2_sub(t, z)), t); };  // 3 t - 2 z
    auto plus = [](const F2& t, const F2& z) { return f2_add(f2_dbl(f2_add(t, z)), t); };   // 3 t + 2 z
    F12 o;
    o.c0.c0 = minus(t0, r0);
    o.c1.c1 = plus(t1, r1);
    o.c1.c0 = plus(x5, r2);
    o.c0.c2 = minus(t4, r3);
    o.c0.c1 = minus(t2, r4);
    o.c1.c2 = plus(t3, r5);
    return o;
}

// ---- constants -----------------------------------------------------------------------------------------------------------------------
struct Consts {
    F2 gamma[4][6];  // gamma[k][i] = xi^(i (q^k - 1) / 6), k = 1, 2, 3: the q^k-power map takes z_i w^i to frob^k(z_i) gamma[k][i] w^i
    F2 b2;           // 3 / xi
    F two_inv;
};
static inline const Consts& consts() {
    static const Consts C = [] {
        Consts c;
        uint64_t e[4];  // (q - 1) / 6
        memcpy(e, h64::QMOD, 32);
        e[0] -= 1;
        u128 rem = 0;
        for (int i = 3; i >= 0; i--) {
            u128 cur = (rem << 64) | e[i];
            e[i] = (uint64_t)(cur / 6);
            rem = cur % 6;
        }
        const F2 xi = {f_small(9), f_small(1)};
        F2 g1 = f2_pow(xi, e, 4);
        F2 g2 = f2_mul(g1, f2_conj(g1));  // xi^((q - 1)(q + 1) / 6)
        F2 g3 = f2_mul(g2, g1);           // xi^((q - 1)(q^2 + q + 1) / 6): g1^(q^2) = g1
        const F2 base[4] = {f2_one(), g1, g2, g3};
        for (int k = 0; k < 4; k++) {
            c.gamma[k][0] = f2_one();
            for (int i = 1; i < 6; i++) c.gamma[k][i] = f2_mul(c.gamma[k][i - 1], base[k]);
        }
        c.b2 = f2_scale(f2_inv(xi), f_small(3));
        c.two_inv = g1h::f_inv(f_small(2));
        return c;
    }();
    return C;
}

// a^(q^k), k = 1, 2, 3
static inline F12 f12_frobenius(const F12& a, int k) {
    const Consts& C = consts();
    F12 o = a;
    for (int i = 0; i < 6; i++) {
        F2& z = f12_coeff(o, i);
        if (k & 1) z = f2_conj(z);
        if (i) z = f2_mul(z, C.gamma[k][i]);
    }
    return o;
}

// ---- G2 ------------------------------------------------------------------------------------------------------------------------------
struct G2A {  // affine; the identity is (0, 0)
    F2 x, y;
};
struct G2J {  // Jacobian; the identity is z = 0
    F2 x, y, z;
};
static inline bool g2_is_identity(const G2A& p) { return f2_is_zero(p.x) && f2_is_zero(p.y); }
static inline G2A g2_identity() { return {f2_zero(), f2_zero()}; }
static inline G2A g2_neg(const G2A& p) { return {p.x, f2_neg(p.y)}; }
static inline bool g2_eq(const G2A& a, const G2A& b) { return f2_eq(a.x, b.x) && f2_eq(a.y, b.y); }
// false when a coordinate is not below q
static inline bool g2_load(const uint64_t raw[16], G2A* p) {
    for (int i = 0; i < 4; i++)
        if (!f_canonical(raw + 4 * i)) return false;
    memcpy(p, raw, 128);
    return true;
}
static inline void g2_store(const G2A& p, uint64_t raw[16]) { memcpy(raw, &p, 128); }
static inline bool g2_on_curve(const G2A& p) {
    if (g2_is_identity(p)) return true;
    return f2_eq(f2_sqr(p.y), f2_add(f2_mul(f2_sqr(p.x), p.x), consts().b2));
}
static inline G2J g2_to_jacobian(const G2A& p) {
    if (g2_is_identity(p)) return {f2_zero(), f2_one(), f2_zero()};
    return {p.x, p.y, f2_one()};
}
static inline G2A g2_to_affine(const G2J& p) {
    if (f2_is_zero(p.z)) return g2_identity();
    F2 zi = f2_inv(p.z), zi2 = f2_sqr(zi);
    return {f2_mul(p.x, zi2), f2_mul(p.y, f2_mul(zi2, zi))};
}
static inline G2J g2_double(const G2J& p) {  // dbl-2009-l
    if (f2_is_zero(p.z)) return p;
    F2 a = f2_sqr(p.x), b = f2_sqr(p.y), c = f2_sqr(b);
    F2 d = f2_dbl(f2_sub(f2_sub(f2_sqr(f2_add(p.x, b)), a), c));
    F2 e = f2_add(f2_dbl(a), a), f = f2_sqr(e);
    G2J o;
    o.x = f2_sub(f, f2_dbl(d));
    o.y = f2_sub(f2_mul(e, f2_sub(d, o.x)), f2_dbl(f2_dbl(f2_dbl(c))));
    o.z = f2_dbl(f2_mul(p.y, p.z));
    return o;
}
// complete: equal operands double, opposite operands cancel, an identity on either side is returned as it is
static inline G2J g2_add(const G2J& p, const G2J& q) {
    if (f2_is_zero(q.z)) return p;
    if (f2_is_zero(p.z)) return q;
    F2 z1z1 = f2_sqr(p.z), z2z2 = f2_sqr(q.z);
    F2 u1 = f2_mul(p.x, z2z2), u2 = f2_mul(q.x, z1z1);
    F2 s1 = f2_mul(p.y, f2_mul(q.z, z2z2)), s2 = f2_mul(q.y, f2_mul(p.z, z1z1));
    F2 h = f2_sub(u2, u1), r = f2_sub(s2, s1);
    if (f2_is_zero(h)) return f2_is_zero(r) ? g2_double(p) : G2J{f2_zero(), f2_one(), f2_zero()};
    F2 hh = f2_sqr(h), hhh = f2_mul(h, hh), v = f2_mul(u1, hh);
    G2J o;
    o.x = f2_sub(f2_sub(f2_sqr(r), hhh), f2_dbl(v));
    o.y = f2_sub(f2_mul(r, f2_sub(v, o.x)), f2_mul(s1, hhh));
    o.z = f2_mul(f2_mul(p.z, q.z), h);
    return o;
}
// [k] p, k a canonical integer of `limbs` 64-bit limbs
static inline G2J g2_mul(const G2A& p, const uint64_t* k, int limbs) {
    G2J acc = g2_to_jacobian(g2_identity()), base = g2_to_jacobian(p);
    int top = 64 * limbs - 1;
    while (top >= 0 && !((k[top >> 6] >> (top & 63)) & 1)) top--;
    for (int i = top; i >= 0; i--) {
        acc = g2_double(acc);
        if ((k[i >> 6] >> (i & 63)) & 1) acc = g2_add(acc, base);
    }
    return acc;
}
// [r] p = O.  The twist's group has order r (2q - r), so a curve point need not be in the r-torsion
static inline bool g2_in_subgroup(const G2A& p) {
    uint64_t r[4];
    memcpy(r, FrP::MOD, 32);
    return f2_is_zero(g2_mul(p, r, 4).z);
}
// pi^k on the untwisted point, in twist coordinates: (conj^k(x) gamma[k][2], conj^k(y) gamma[k][3])
static inline G2A g2_frobenius(const G2A& p, int k) {
    const Consts& C = consts();
    if (k & 1) return {f2_mul(f2_conj(p.x), C.gamma[k][2]), f2_mul(f2_conj(p.y), C.gamma[k][3])};
    return {f2_mul(p.x, C.gamma[k][2]), f2_mul(p.y, C.gamma[k][3])};
}

// ---- Miller loop ---------------------------------------------------------------------------------------------------------------------
struct G2H {  // homogeneous projective: x = X / Z, y = Y / Z
    F2 x, y, z;
};
struct Line {  // l0 y_P + l1 x_P w + l3 w^3
    F2 l0, l1, l3;
};
// T <- 2T and the tangent at T (Costello, Lange, Naehrig 2010)
static inline Line step_double(G2H& t) {
    const Consts& C = consts();
    F2 a = f2_scale(f2_mul(t.x, t.y), C.two_inv), b = f2_sqr(t.y), c = f2_sqr(t.z);
    F2 e = f2_mul(C.b2, f2_add(f2_dbl(c), c)), f = f2_add(f2_dbl(e), e);
    F2 g = f2_scale(f2_add(b, f), C.two_inv), h = f2_sub(f2_sqr(f2_add(t.y, t.z)), f2_add(b, c));
    F2 i = f2_sub(e, b), j = f2_sqr(t.x), ee = f2_sqr(e);
    t.x = f2_mul(a, f2_sub(b, f));
    t.y = f2_sub(f2_sqr(g), f2_add(f2_dbl(ee), ee));
    t.z = f2_mul(b, h);
    return {f2_neg(h), f2_add(f2_dbl(j), j), i};
}
// T <- T + Q and the line through them; T != +-Q (true inside the loop for Q of order r)
static inline Line step_add(G2H& t, const G2A& q) {
    F2 theta = f2_sub(t.y, f2_mul(q.y, t.z)), lambda = f2_sub(t.x, f2_mul(q.x, t.z));
    F2 c = f2_sqr(theta), d = f2_sqr(lambda), e = f2_mul(lambda, d), f = f2_mul(t.z, c), g = f2_mul(t.x, d);
    F2 h = f2_sub(f2_add(e, f), f2_dbl(g));
    t.x = f2_mul(lambda, h);
    t.y = f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, t.y));
    t.z = f2_mul(t.z, e);
    return {lambda, f2_neg(theta), f2_sub(f2_mul(theta, q.x), f2_mul(lambda, q.y))};
}
struct Pair {
    F px, py;
    G2A q;
    G2H t;
};
static inline void apply(F12& f, const Line& l, const Pair& p) { f = f12_mul_by_line(f, f2_scale(l.l0, p.py), f2_scale(l.l1, p.px), l.l3); }
// prod_i f_{6t+2,Q_i}(P_i) l(P_i) l(P_i) over pairs without an identity: one squaring chain serves them all
static inline F12 miller_loop(std::vector<Pair>& pairs) {
    F12 f = f12_one();
    if (pairs.empty()) return f;
    const u128 ate = (u128)6 * BN_T + 2;  // 65 bits
    for (Pair& p : pairs) p.t = {p.q.x, p.q.y, f2_one()};
    for (int i = 63; i >= 0; i--) {
        if (i != 63) f = f12_sqr(f);
        for (Pair& p : pairs) apply(f, step_double(p.t), p);
        if ((ate >> i) & 1)
            for (Pair& p : pairs) apply(f, step_add(p.t, p.q), p);
    }
    for (Pair& p : pairs) {
        G2A q1 = g2_frobenius(p.q, 1), q2 = g2_neg(g2_frobenius(p.q, 2));
        apply(f, step_add(p.t, q1), p);
        apply(f, step_add(p.t, q2), p);
    }
    return f;
}

// ---- final exponentiation ------------------------------------------------------------------------------------------------------------
static inline F12 easy_part(const F12& f) {  // f^((q^6 - 1)(q^2 + 1)); f != 0
    F12 a = f12_mul(f12_conj(f), f12_inv(f));
    return f12_mul(f12_frobenius(a, 2), a);
}
static inline F12 cyclotomic_exp_t(const F12& a) {
    F12 r = a;
    for (int i = 61; i >= 0; i--) {  // t has 63 bits
        r = f12_cyclotomic_sqr(r);
        if ((BN_T >> i) & 1) r = f12_mul(r, a);
    }
    return r;
}
static inline F12 hard_part(const F12& f) {  // f^((q^4 - q^2 + 1) / r), f in the cyclotomic subgroup (inverse = conjugate)
    F12 ft = cyclotomic_exp_t(f), ft2 = cyclotomic_exp_t(ft), ft3 = cyclotomic_exp_t(ft2);
    F12 y0 = f12_mul(f12_mul(f12_frobenius(f, 1), f12_frobenius(f, 2)), f12_frobenius(f, 3));
    F12 y1 = f12_conj(f);
    F12 y2 = f12_frobenius(ft2, 2);
    F12 y3 = f12_conj(f12_frobenius(ft, 1));
    F12 y4 = f12_conj(f12_mul(ft, f12_frobenius(ft2, 1)));
    F12 y5 = f12_conj(ft2);
    F12 y6 = f12_conj(f12_mul(ft3, f12_frobenius(ft3, 1)));
    // y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36
    F12 t0 = f12_mul(f12_mul(f12_cyclotomic_sqr(y6), y4), y5);
    F12 t1 = f12_mul(f12_mul(y3, y5), t0);
    t0 = f12_mul(t0, y2);
    t1 = f12_cyclotomic_sqr(f12_mul(f12_cyclotomic_sqr(t1), t0));
    t0 = f12_cyclotomic_sqr(f12_mul(t1, y1));
    return f12_mul(t0, f12_mul(t1, y0));
}
static inline F12 final_exponentiation(const F12& f) { return hard_part(easy_part(f)); }

// ---- the calls of include/halo2hip_pairing.h -----------------------------------------------------------------------------------------
// a_0, b_0, ..., a_5, b_5 with the value sum_i (a_i + b_i u) w^i
static inline void gt_store(const F12& f, uint64_t out[48]) {
    F12 c = f;
    for (int i = 0; i < 6; i++) memcpy(out + 8 * i, &f12_coeff(c, i), 64);
}

// prod_i e(P_i, Q_i) into *out.  0, or 1 with the reason in err (the text after the call's name)
static inline int pairing_product(const uint64_t* g1_xy, const uint64_t* g2_raw, size_t n, F12* out, char* err, size_t err_len) {
    if (n > MAX_PAIRS) {
        snprintf(err, err_len, "n = %zu pairs are more than %zu: fold the batch first", n, MAX_PAIRS);
        return 1;
    }
    if (n && !g1_xy) {
        snprintf(err, err_len, "null g1_xy");
        return 1;
    }
    if (n && !g2_raw) {
        snprintf(err, err_len, "null g2_raw");
        return 1;
    }
    std::vector<Pair> pairs;
    pairs.reserve(n);
    for (size_t i = 0; i < n; i++) {
        Affine a;
        memcpy(&a, g1_xy + 8 * i, 64);
        if (!fe_is_canonical<Q>(a.x) || !fe_is_canonical<Q>(a.y)) {
            snprintf(err, err_len, "g1_xy[%zu] has a coordinate that is not below q", i);
            return 1;
        }
        if (!affine_on_curve(a)) {
            snprintf(err, err_len, "g1_xy[%zu] is neither on the curve nor (0, 0)", i);
            return 1;
        }
        Pair p;
        if (!g2_load(g2_raw + 16 * i, &p.q)) {
            snprintf(err, err_len, "g2_raw[%zu] has a coordinate that is not below q", i);
            return 1;
        }
        if (!g2_on_curve(p.q)) {
            snprintf(err, err_len, "g2_raw[%zu] is neither on the twist nor the identity", i);
            return 1;
        }
        if (!g2_in_subgroup(p.q)) {
            snprintf(err, err_len, "g2_raw[%zu] is not in the subgroup of order r", i);
            return 1;
        }
        if (affine_is_identity(a) || g2_is_identity(p.q)) continue;  // contributes 1
        memcpy(&p.px, &a.x, 32);
        memcpy(&p.py, &a.y, 32);
        pairs.push_back(p);
    }
    *out = final_exponentiation(miller_loop(pairs));
    return 0;
}

// [scalar] Q, the scalar an Fr element in Montgomery form.  The point is checked to be on the twist, not to be in the subgroup
static inline int g2_scalar_mul(const uint64_t* g2_raw, const uint64_t* scalar, uint64_t* out_raw, char* err, size_t err_len) {
    if (!g2_raw || !scalar || !out_raw) {
        snprintf(err, err_len, "null %s", !g2_raw ? "g2_raw" : (!scalar ? "scalar" : "out_raw"));
        return 1;
    }
    Fe s;
    memcpy(&s, scalar, 32);
    if (!fe_is_canonical<FrP>(s)) {
        snprintf(err, err_len, "the scalar is not a reduced Fr element");
        return 1;
    }
    G2A q;
    if (!g2_load(g2_raw, &q)) {
        snprintf(err, err_len, "g2_raw has a coordinate that is not below q");
        return 1;
    }
    if (!g2_on_curve(q)) {
        snprintf(err, err_len, "g2_raw is neither on the twist nor the identity");
        return 1;
    }
    Fe c = fe_to_canonical<FrP>(s);
    uint64_t k[4];
    memcpy(k, &c, 32);
    g2_store(g2_to_affine(g2_mul(q, k, 4)), out_raw);
    return 0;
}

static inline int g2_check(const uint64_t* g2_raw, int* on_curve, int* in_subgroup, char* err, size_t err_len) {
    if (!g2_raw || !on_curve || !in_subgroup) {
        snprintf(err, err_len, "null %s", !g2_raw ? "g2_raw" : (!on_curve ? "on_curve" : "in_subgroup"));
        return 1;
    }
    G2A q;
    if (!g2_load(g2_raw, &q)) {
        snprintf(err, err_len, "g2_raw has a coordinate that is not below q");
        return 1;
    }
    *on_curve = g2_on_curve(q) ? 1 : 0;
    *in_subgroup = *on_curve && g2_in_subgroup(q) ? 1 : 0;
    return 0;
}

}  // namespace pairing
}  // namespace h2
