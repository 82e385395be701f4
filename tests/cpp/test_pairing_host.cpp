// Host-side test of csrc/pairing_host.h as a program of its own: the tower, the G2 group law and the pairing the library exports,
// compiled here without the library, against definitions that do not share the header's shortcuts --
//   * Fq2, Fq6 and Fq12 products against schoolbook products (Fq12 as six Fq2 coefficients of w^i, w^6 = xi), a a^-1 = 1;
//   * Frobenius^k against a plain pow by q^k, twelve Frobenius steps the identity;
//   * the sparse line product against the full product, cyclotomic squaring against squaring on elements taken after the easy part;
//   * the hard part against a plain pow by (q^4 - q^2 + 1) / r;
//   * the G2 group law: (a + b) Q = a Q + b Q, [r] G2 = O, complete additions;
//   * the subgroup test on a twist point outside the r-torsion (y solved for a small x) against a right-to-left [r] Q and against the
//     cofactor 2q - r, which takes every twist point into the subgroup;
//   * bilinearity and non-degeneracy of the pairing, a product that closes to 1, identities, and the rejections with their texts.
// It prints e(G1, G2) in the library's Gt layout; tests/test_pairing.py compares that line with tests/golden/pairing.json.
// No GPU and no library; tests/test_pairing.py builds and runs it plain and under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../halo2-pse_amd/csrc/pairing_host.h"

using namespace h2;
using namespace h2::pairing;

static uint64_t rs = 0x9a121c;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
static int failures = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// canonical limbs -> Montgomery
static F from_canonical(const uint64_t c[4]) {
    F a, r2;
    memcpy(&a, c, 32);
    memcpy(&r2, Q::R2, 32);
    return h64::mul(a, r2);
}
static F rnd_f() {
    uint64_t c[4] = {rnd(), rnd(), rnd(), rnd() & 0x0fffffffffffffffULL};  // < 2^252 < q
    return from_canonical(c);
}
static F2 rnd_f2() { return {rnd_f(), rnd_f()}; }
static F6 rnd_f6() { return {rnd_f2(), rnd_f2(), rnd_f2()}; }
static F12 rnd_f12() { return {rnd_f6(), rnd_f6()}; }
static void rnd_scalar(uint64_t k[4]) {
    for (int i = 0; i < 4; i++) k[i] = rnd();
    k[3] &= 0x0fffffffffffffffULL;  // < 2^252 < r
}

// ---- schoolbook references -----------------------------------------------------------------------------------------------------------
static F2 f2_school(const F2& a, const F2& b) {
    return {h64::sub(h64::mul(a.c0, b.c0), h64::mul(a.c1, b.c1)), h64::add(h64::mul(a.c0, b.c1), h64::mul(a.c1, b.c0))};
}
static F2 xi_times(const F2& a) { return f2_school(a, {f_small(9), f_small(1)}); }
static F6 f6_school(const F6& a, const F6& b) {
    const F2 x[3] = {a.c0, a.c1, a.c2}, y[3] = {b.c0, b.c1, b.c2};
    F2 t[5] = {f2_zero(), f2_zero(), f2_zero(), f2_zero(), f2_zero()};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[i + j] = f2_add(t[i + j], f2_school(x[i], y[j]));
    return {f2_add(t[0], xi_times(t[3])), f2_add(t[1], xi_times(t[4])), t[2]};
}
static F12 f12_school(const F12& a, const F12& b) {
    F12 x = a, y = b, o;
    F2 t[11];
    for (int i = 0; i < 11; i++) t[i] = f2_zero();
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) t[i + j] = f2_add(t[i + j], f2_school(f12_coeff(x, i), f12_coeff(y, j)));
    for (int i = 0; i < 6; i++) f12_coeff(o, i) = i < 5 ? f2_add(t[i], xi_times(t[i + 6])) : t[i];
    return o;
}
static F12 f12_pow(const F12& a, const uint64_t* e, int limbs) {
    F12 r = f12_one();
    for (int i = 64 * limbs - 1; i >= 0; i--) {
        r = f12_school(r, r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = f12_school(r, a);
    }
    return r;
}
// out (na + nb limbs) = a * b
static void big_mul(const uint64_t* a, int na, const uint64_t* b, int nb, uint64_t* out) {
    memset(out, 0, 8 * (na + nb));
    for (int i = 0; i < na; i++) {
        u128 c = 0;
        for (int j = 0; j < nb; j++) {
            c += (u128)a[i] * b[j] + out[i + j];
            out[i + j] = (uint64_t)c;
            c >>= 64;
        }
        out[i + nb] = (uint64_t)c;
    }
}

static const uint64_t HARD_EXPONENT[12] = {  // (q^4 - q^2 + 1) / r
    0xe81bb482ccdf42b1ULL, 0x5abf5cc4f49c36d4ULL, 0xf1154e7e1da014fdULL, 0xdcc7b44c87cdbacfULL, 0xaaa441e3954bcf8aULL, 0x6b887d56d5095f23ULL,
    0x79581e16f3fd90c6ULL, 0x3b1b1355d189227dULL, 0x4e529a5861876f6bULL, 0x6c0eb522d5b12278ULL, 0x331ec15183177fafULL, 0x01baaa710b0759adULL};
static const uint64_t G2_GEN[4][4] = {  // EIP-197's generator: x.c0, x.c1, y.c0, y.c1, canonical
    {0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL},
    {0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL},
    {0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL},
    {0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL}};

static G2A generator2() {
    return {{from_canonical(G2_GEN[0]), from_canonical(G2_GEN[1])}, {from_canonical(G2_GEN[2]), from_canonical(G2_GEN[3])}};
}
static void g1_limbs(uint64_t k, uint64_t out[8]) {  // [k] (1, 2), affine Montgomery
    Affine g;
    g.x = fe_from_u64<FqP>(1);
    g.y = fe_from_u64<FqP>(2);
    Affine a = xyzz_to_affine(xyzz_mul_small(xyzz_from_affine(g), (uint32_t)k));
    memcpy(out, &a, 64);
}

static void test_tower() {
    for (int it = 0; it < 20; it++) {
        F2 a = rnd_f2(), b = rnd_f2();
        CHECK(f2_eq(f2_mul(a, b), f2_school(a, b)));
        CHECK(f2_eq(f2_sqr(a), f2_school(a, a)));
        CHECK(f2_eq(f2_mul_xi(a), xi_times(a)));
        CHECK(f2_eq(f2_mul(a, f2_inv(a)), f2_one()));
        F6 c = rnd_f6(), d = rnd_f6();
        CHECK(f6_eq(f6_mul(c, d), f6_school(c, d)));
        CHECK(f6_eq(f6_mul(c, f6_inv(c)), f6_one()));
        CHECK(f6_eq(f6_mul_v(c), f6_school(c, {f2_zero(), f2_one(), f2_zero()})));
        CHECK(f6_eq(f6_mul_by_01(c, a, b), f6_school(c, {a, b, f2_zero()})));
        F12 e = rnd_f12(), f = rnd_f12();
        CHECK(f12_eq(f12_mul(e, f), f12_school(e, f)));
        CHECK(f12_eq(f12_sqr(e), f12_school(e, e)));
        CHECK(f12_is_one(f12_mul(e, f12_inv(e))));
        // the sparse product: l0 + l1 w + l3 w^3
        F2 l0 = rnd_f2(), l1 = rnd_f2(), l3 = rnd_f2();
        F12 line = {f6_zero(), f6_zero()};
        f12_coeff(line, 0) = l0;
        f12_coeff(line, 1) = l1;
        f12_coeff(line, 3) = l3;
        CHECK(f12_eq(f12_mul_by_line(e, l0, l1, l3), f12_school(e, line)));
    }
    CHECK(f2_is_zero(f2_inv(f2_zero())));
    CHECK(f2_eq(f2_school({f_zero(), f_small(1)}, {f_zero(), f_small(1)}), f2_neg(f2_one())));  // u^2 = -1
}

static void test_frobenius() {
    uint64_t q1[4], q2[8], q3[12];
    memcpy(q1, h64::QMOD, 32);
    big_mul(q1, 4, q1, 4, q2);
    big_mul(q2, 8, q1, 4, q3);
    for (int it = 0; it < 2; it++) {
        F12 a = rnd_f12();
        CHECK(f12_eq(f12_frobenius(a, 1), f12_pow(a, q1, 4)));
        CHECK(f12_eq(f12_frobenius(a, 2), f12_pow(a, q2, 8)));
        CHECK(f12_eq(f12_frobenius(a, 3), f12_pow(a, q3, 12)));
        CHECK(f12_eq(f12_frobenius(f12_frobenius(f12_frobenius(a, 2), 2), 2), f12_conj(a)));  // q^6
        F12 b = a;
        for (int i = 0; i < 12; i++) b = f12_frobenius(b, 1);
        CHECK(f12_eq(a, b));
    }
}

static void test_final_exponentiation() {
    for (int it = 0; it < 3; it++) {
        F12 c = easy_part(rnd_f12());
        CHECK(f12_is_one(f12_mul(c, f12_conj(c))));  // in the cyclotomic subgroup the conjugate is the inverse
        CHECK(f12_eq(f12_cyclotomic_sqr(c), f12_school(c, c)));
        CHECK(f12_eq(cyclotomic_exp_t(c), f12_pow(c, &BN_T, 1)));
        CHECK(f12_eq(hard_part(c), f12_pow(c, HARD_EXPONENT, 12)));
    }
    CHECK(f12_is_one(final_exponentiation(f12_one())));
}

// ---- square roots, to find a twist point outside the subgroup ---------------------------------------------------------------------
static bool f_sqrt(const F& a, F* out) {  // q = 3 mod 4
    uint64_t e[4];
    memcpy(e, h64::QMOD, 32);
    e[0] += 1;  // no carry: the low limb of q is ...47
    for (int i = 0; i < 4; i++) e[i] = (e[i] >> 2) | (i < 3 ? e[i + 1] << 62 : 0);
    F r = g1h::f_one();
    for (int i = 255; i >= 0; i--) {
        r = h64::sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = h64::mul(r, a);
    }
    *out = r;
    return f_eq(h64::sqr(r), a);
}
static bool f2_sqrt(const F2& a, F2* out) {  // x0^2 = (a0 +- |a|) / 2, x1 = a1 / (2 x0)
    F n;
    if (!f_sqrt(h64::add(h64::sqr(a.c0), h64::sqr(a.c1)), &n)) return false;
    const F half = consts().two_inv;
    for (int s = 0; s < 2; s++) {
        F x0;
        if (f_sqrt(h64::mul(s ? h64::sub(a.c0, n) : h64::add(a.c0, n), half), &x0) && !h64::is_zero(x0)) {
            F2 r = {x0, h64::mul(a.c1, g1h::f_inv(h64::dbl(x0)))};
            if (f2_eq(f2_school(r, r), a)) {
                *out = r;
                return true;
            }
        }
    }
    return false;
}

static G2A mul_u64(const G2A& p, uint64_t k) { return g2_to_affine(g2_mul(p, &k, 1)); }

static void test_g2() {
    const G2A g = generator2();
    CHECK(g2_on_curve(g) && g2_in_subgroup(g) && g2_on_curve(g2_identity()) && g2_in_subgroup(g2_identity()));
    uint64_t r[4];
    memcpy(r, FrP::MOD, 32);
    CHECK(g2_is_identity(g2_to_affine(g2_mul(g, r, 4))));
    for (int it = 0; it < 4; it++) {
        uint64_t a[4], b[4], s[5];
        rnd_scalar(a);
        rnd_scalar(b);
        u128 c = 0;
        for (int i = 0; i < 4; i++) {
            c += (u128)a[i] + b[i];
            s[i] = (uint64_t)c;
            c >>= 64;
        }
        s[4] = (uint64_t)c;
        G2J pa = g2_mul(g, a, 4), pb = g2_mul(g, b, 4);
        G2A sum = g2_to_affine(g2_add(pa, pb));
        CHECK(g2_on_curve(sum) && g2_eq(sum, g2_to_affine(g2_mul(g, s, 5))));
        CHECK(g2_eq(g2_to_affine(g2_add(pa, pa)), g2_to_affine(g2_double(pa))));                      // equal operands
        CHECK(g2_is_identity(g2_to_affine(g2_add(pa, g2_to_jacobian(g2_neg(g2_to_affine(pa)))))));    // opposite operands
        CHECK(g2_eq(g2_to_affine(g2_add(pa, g2_to_jacobian(g2_identity()))), g2_to_affine(pa)));
        CHECK(g2_eq(g2_to_affine(g2_add(g2_to_jacobian(g2_identity()), pa)), g2_to_affine(pa)));
    }
    CHECK(g2_eq(mul_u64(g, 6), g2_to_affine(g2_add(g2_mul(g, (const uint64_t[]){2}, 1), g2_mul(g, (const uint64_t[]){4}, 1)))));
    CHECK(g2_is_identity(mul_u64(g, 0)) && g2_eq(mul_u64(g, 1), g));
    // pi(Q) = [q] Q on the r-torsion of the twist's trace-zero subgroup
    uint64_t q[4];
    memcpy(q, h64::QMOD, 32);
    CHECK(g2_eq(g2_frobenius(g, 1), g2_to_affine(g2_mul(g, q, 4))));
    CHECK(g2_eq(g2_frobenius(g2_frobenius(g, 1), 1), g2_frobenius(g, 2)));
    // a twist point outside the subgroup: x = c + u for the first small c with a root
    G2A out = g2_identity();
    for (uint64_t c = 1; c < 100 && g2_is_identity(out); c++) {
        F2 x = {f_small(c), f_small(1)}, y;
        if (f2_sqrt(f2_add(f2_school(f2_school(x, x), x), consts().b2), &y)) out = {x, y};
    }
    CHECK(!g2_is_identity(out) && g2_on_curve(out));
    G2J acc = g2_to_jacobian(g2_identity()), run = g2_to_jacobian(out);  // [r] Q right to left
    for (int i = 0; i < 254; i++) {
        if ((r[i >> 6] >> (i & 63)) & 1) acc = g2_add(acc, run);
        run = g2_double(run);
    }
    CHECK(!f2_is_zero(acc.z));
    CHECK(!g2_in_subgroup(out));
    uint64_t h[5];  // the cofactor 2q - r
    u128 carry = 0, borrow = 0;
    for (int i = 0; i < 4; i++) {
        carry += (u128)q[i] * 2;
        u128 d = (u128)(uint64_t)carry - r[i] - (uint64_t)borrow;
        h[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
        carry >>= 64;
    }
    h[4] = (uint64_t)carry - (uint64_t)borrow;
    G2A cleared = g2_to_affine(g2_mul(out, h, 5));
    CHECK(!g2_is_identity(cleared) && g2_on_curve(cleared) && g2_in_subgroup(cleared));
    int on = -1, in = -1;
    char why[160];
    uint64_t raw[16];
    g2_store(out, raw);
    CHECK(g2_check(raw, &on, &in, why, sizeof(why)) == 0 && on == 1 && in == 0);
    g2_store(g, raw);
    CHECK(g2_check(raw, &on, &in, why, sizeof(why)) == 0 && on == 1 && in == 1);
    raw[8] ^= 1;
    CHECK(g2_check(raw, &on, &in, why, sizeof(why)) == 0 && on == 0 && in == 0);
}

static void test_pairing() {
    char why[200];
    const G2A g = generator2();
    uint64_t p1[8], q1[16];
    g1_limbs(1, p1);
    g2_store(g, q1);
    F12 e;
    CHECK(pairing_product(p1, q1, 1, &e, why, sizeof(why)) == 0);
    uint64_t r[4];
    memcpy(r, FrP::MOD, 32);
    CHECK(!f12_is_one(e) && f12_is_one(f12_pow(e, r, 4)));
    uint64_t gt[48];
    gt_store(e, gt);
    printf("gt");
    for (int i = 0; i < 48; i++) printf(" %016llx", (unsigned long long)gt[i]);
    printf("\n");
    // e(2 P, 3 Q) = e(P, Q)^6 = e(6 P, Q)
    uint64_t p2[8], p6[8], q3[16];
    g1_limbs(2, p2);
    g1_limbs(6, p6);
    g2_store(mul_u64(g, 3), q3);
    F12 e23, e61;
    const uint64_t six = 6;
    CHECK(pairing_product(p2, q3, 1, &e23, why, sizeof(why)) == 0 && f12_eq(e23, f12_pow(e, &six, 1)));
    CHECK(pairing_product(p6, q1, 1, &e61, why, sizeof(why)) == 0 && f12_eq(e61, e23));
    // e(2 P, 3 Q) e(-6 P, Q) = 1, and not with 7 P; identities contribute 1; n = 0 gives 1
    uint64_t ps[3 * 8], qs[3 * 16];
    memcpy(ps, p2, 64);
    memcpy(qs, q3, 128);
    Affine m6;
    memcpy(&m6, p6, 64);
    m6 = affine_neg(m6);
    memcpy(ps + 8, &m6, 64);
    memcpy(qs + 16, q1, 128);
    memset(ps + 16, 0, 64);
    memcpy(qs + 32, q3, 128);
    F12 prod;
    CHECK(pairing_product(ps, qs, 3, &prod, why, sizeof(why)) == 0 && f12_is_one(prod));
    memcpy(ps + 16, p1, 64);
    memset(qs + 32, 0, 128);
    CHECK(pairing_product(ps, qs, 3, &prod, why, sizeof(why)) == 0 && f12_is_one(prod));
    g1_limbs(7, ps + 8);
    CHECK(pairing_product(ps, qs, 2, &prod, why, sizeof(why)) == 0 && !f12_is_one(prod));
    CHECK(pairing_product(nullptr, nullptr, 0, &prod, why, sizeof(why)) == 0 && f12_is_one(prod));
    // rejections
    CHECK(pairing_product(nullptr, qs, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "null g1_xy");
    CHECK(pairing_product(ps, nullptr, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "null g2_raw");
    CHECK(pairing_product(ps, qs, MAX_PAIRS + 1, &prod, why, sizeof(why)) == 1 && strstr(why, "more than 65536"));
    uint64_t bad[8];
    memcpy(bad, p1, 64);
    bad[4] ^= 1;
    CHECK(pairing_product(bad, q1, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "g1_xy[0] is neither on the curve nor (0, 0)");
    memset(bad, 0xff, 32);
    CHECK(pairing_product(bad, q1, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "g1_xy[0] has a coordinate that is not below q");
    uint64_t badq[16];
    memcpy(badq, q1, 128);
    badq[0] ^= 1;
    CHECK(pairing_product(p1, badq, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "g2_raw[0] is neither on the twist nor the identity");
    memset(badq + 12, 0xff, 32);
    CHECK(pairing_product(p1, badq, 1, &prod, why, sizeof(why)) == 1 && std::string(why) == "g2_raw[0] has a coordinate that is not below q");
    // g2_scalar_mul: Montgomery scalars
    Fe five = fe_from_u64<FrP>(5);
    uint64_t out[16], want[16];
    CHECK(g2_scalar_mul(q1, (const uint64_t*)&five, out, why, sizeof(why)) == 0);
    g2_store(mul_u64(g, 5), want);
    CHECK(memcmp(out, want, 128) == 0);
    uint64_t big[4] = {~0ULL, ~0ULL, ~0ULL, ~0ULL};
    CHECK(g2_scalar_mul(q1, big, out, why, sizeof(why)) == 1 && std::string(why) == "the scalar is not a reduced Fr element");
    CHECK(g2_scalar_mul(q1, (const uint64_t*)&five, nullptr, why, sizeof(why)) == 1 && std::string(why) == "null out_raw");
}

int main() {
    test_tower();
    test_frobenius();
    test_final_exponentiation();
    test_g2();
    test_pairing();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("pairing host tests ok\n");
    return 0;
}
