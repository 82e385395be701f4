// Host-side test of what csrc/serde.hip's kernels do to one element (csrc/serde_elem.h) and of fu_sqrt (csrc/fieldu.h), against the
// saturated arithmetic of csrc/field.h: fe_pow for the square root, fe_mul for everything else.  Built with -DH2_FU_CHECK, so every
// product of the unsaturated chain asserts its limb bounds.  No GPU needed: the same H2_HD source compiles for the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../halo2-pse_amd/csrc/serde_elem.h"

using namespace h2;

static uint64_t rs = 0x5e2de;
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

template <class P>
static Fe rand_canonical() {  // a canonical integer below the modulus (a Montgomery-form value of some element just as well)
    Fe a;
    for (int j = 0; j < 8; j++) a.l[j] = (uint32_t)rnd();
    a.l[7] &= 0x3fffffff;
    if (!fe_is_canonical<P>(a)) a.l[7] &= 0x1fffffff;
    return a;
}
static Fe small(uint32_t v) {
    Fe a = fe_zero<FqP>();
    a.l[0] = v;
    return a;
}

// t (E-form): fu_sqrt against fe_pow(t, (q + 1) / 4); returns whether t is a square
static bool check_sqrt(const Fe& t) {
    const Fe want = fe_pow<FqP>(t, FqU::SQRT_E);
    const Fu y = fu_sqrt<FqU>(fu_from_ext(t));  // fu_from_ext: E-form -> I-form, value < 32 q, the loosest input of the contract
    for (int i = 0; i < 8; i++) CHECK(y.l[i] >= 0 && y.l[i] < (1 << 29));
    CHECK(y.l[8] >= -(1 << 22) && y.l[8] < (1 << 23));  // value in (-0.2 q, 1.2 q)
    CHECK(fe_eq(fu_mul_canon<FqU>(y, fu_one_e<FqU>()), want));
    return fe_eq(fe_sqr<FqP>(want), t);
}

// the 32 bytes of x with the sign bit, as the Fe they load as
static Fe encode(const Fe& x_canonical, uint32_t sign) {
    Fe b = x_canonical;
    b.l[7] |= sign << 31;
    return b;
}

int main() {
    // ---- fu_sqrt ----
    int squares = 0;
    CHECK(check_sqrt(fe_zero<FqP>()) && check_sqrt(fe_one<FqP>()) && check_sqrt(fe_from_u64<FqP>(4)));
    CHECK(!check_sqrt(fe_neg<FqP>(fe_one<FqP>())));  // t = q - 1; q = 3 (mod 4): -1 is not a square
    for (int it = 0; it < 10000; it++) squares += check_sqrt(rand_canonical<FqP>());
    CHECK(squares > 4700 && squares < 5300);  // half of the field

    // ---- decompression against the saturated arithmetic, both signs; compression back ----
    const Fe three = fe_from_u64<FqP>(3);
    int valid = 0;
    for (int it = 0; it < 3000; it++) {
        Fe xc = it < 16 ? small((uint32_t)it) : rand_canonical<FqP>();
        const Fe x = fe_from_canonical<FqP>(xc);
        const Fe t = fe_add<FqP>(fe_mul<FqP>(fe_sqr<FqP>(x), x), three);
        Fe y = fe_pow<FqP>(t, FqU::SQRT_E);
        const bool on_curve = fe_eq(fe_sqr<FqP>(y), t);
        for (uint32_t sign = 0; sign < 2; sign++) {
            Affine got;
            const bool ok = g1_decompress_elem(encode(xc, sign), &got);
            if (fe_is_zero(xc) && !sign) {  // the identity
                CHECK(ok && affine_is_identity(got));
                continue;
            }
            CHECK(ok == on_curve);
            if (!on_curve) {
                CHECK(affine_is_identity(got));
                continue;
            }
            valid++;
            if ((fe_to_canonical<FqP>(y).l[0] & 1u) != sign) y = fe_neg<FqP>(y);
            CHECK(fe_eq(got.x, x) && fe_eq(got.y, y));
            CHECK(g1_validate_elem(got));
            CHECK(fe_eq(g1_compress_elem(got), encode(xc, sign)));
        }
    }
    CHECK(valid > 2600 && valid < 3400);
    // x >= q: q itself, x = 1 with bit 254 set, all ones below the sign bit
    Affine got;
    Fe bad;
    memcpy(bad.l, FqP::MOD, 32);
    CHECK(!g1_decompress_elem(bad, &got) && affine_is_identity(got));
    bad = small(1);
    bad.l[7] |= 1u << 30;
    CHECK(!g1_decompress_elem(bad, &got) && affine_is_identity(got));
    bad.l[7] |= 1u << 31;
    CHECK(!g1_decompress_elem(bad, &got) && affine_is_identity(got));
    for (int j = 0; j < 8; j++) bad.l[j] = 0xffffffffu;
    CHECK(!g1_decompress_elem(bad, &got) && affine_is_identity(got));
    bad.l[7] = 0x7fffffffu;
    CHECK(!g1_decompress_elem(bad, &got) && affine_is_identity(got));
    // (1, 2) and (1, q - 2)
    Fe one_x = small(1);
    CHECK(g1_decompress_elem(encode(one_x, 0), &got) && fe_eq(got.x, fe_one<FqP>()) && fe_eq(got.y, fe_from_u64<FqP>(2)));
    CHECK(g1_decompress_elem(encode(one_x, 1), &got) && fe_eq(got.x, fe_one<FqP>()) && fe_eq(got.y, fe_neg<FqP>(fe_from_u64<FqP>(2))));

    // ---- validation ----
    Affine p;
    p.x = fe_one<FqP>(), p.y = fe_from_u64<FqP>(2);
    CHECK(g1_validate_elem(p));
    p.y = fe_from_u64<FqP>(3);
    CHECK(!g1_validate_elem(p));
    p.x = p.y = fe_zero<FqP>();
    CHECK(g1_validate_elem(p));
    p.y = fe_one<FqP>();
    CHECK(!g1_validate_elem(p));
    p.x = fe_one<FqP>();
    memcpy(p.y.l, FqP::MOD, 32);  // y = q: not reduced
    CHECK(!g1_validate_elem(p));

    // ---- Fr ----
    for (int it = 0; it < 2000; it++) {
        Fe c = rand_canonical<FrP>(), m;
        CHECK(fr_from_repr_elem(c, &m) && fe_eq(fe_to_canonical<FrP>(m), c));
    }
    Fe r, m;
    memcpy(r.l, FrP::MOD, 32);
    CHECK(!fr_from_repr_elem(r, &m) && fe_is_zero(m));
    for (int j = 0; j < 8; j++) r.l[j] = 0xffffffffu;
    CHECK(!fr_from_repr_elem(r, &m) && fe_is_zero(m));

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("serde host tests ok\n");
    return 0;
}
