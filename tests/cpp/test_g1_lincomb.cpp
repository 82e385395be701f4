// Host-side test of h2hip_g1_linear_combinations_bn254's body (csrc/g1_host.h) as a program of its own: the same function the library
// exports, compiled here without the library, against a term-by-term double-and-add over ec.h's 8 x 32 field (the function itself runs
// on host64.h's 4 x 64 field and shares one doubling chain, so the two share the curve equation only).  The cases are those of
// tests/test_g1_lincomb.py: random sums at several (m, t), the scalars 0, 1 and r - 1, identities among points and addends, a closing
// addition that doubles or cancels, equal and opposite points under equal scalars, m = 0, t = 0 and every rejection with its text.
// No GPU; tests/test_g1_lincomb.py builds and runs it plain and under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../halo2-pse_amd/csrc/g1_host.h"

using namespace h2;

static uint64_t rs = 0x61c0b;
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

static Fe canon_u64(uint64_t v) {
    Fe c = fe_zero<FrP>();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return c;
}
static Fe rnd_canon() {
    Fe c;
    for (int j = 0; j < 8; j++) c.l[j] = (uint32_t)rnd();
    c.l[7] &= 0x0fffffffu;  // < 2^252 < r
    return c;
}
static Fe r_minus_1() {
    Fe c;
    for (int j = 0; j < 8; j++) c.l[j] = FrP::MOD[j];
    c.l[0] -= 1;
    return c;
}

// [k] p by double-and-add over all 254 bits, ec.h only
static XYZZ ref_mul(const Affine& p, const Fe& k_canon) {
    XYZZ acc = xyzz_identity();
    for (int i = 253; i >= 0; i--) {
        acc = xyzz_double(acc);
        if ((k_canon.l[i >> 5] >> (i & 31)) & 1) xyzz_add_mixed(acc, p);
    }
    return acc;
}
static Affine generator() {
    Affine g;
    g.x = fe_from_u64<FqP>(1);
    g.y = fe_from_u64<FqP>(2);
    return g;
}
static Affine rnd_point() { return xyzz_to_affine(ref_mul(generator(), rnd_canon())); }
static Affine identity() {
    Affine a = {fe_zero<FqP>(), fe_zero<FqP>()};
    return a;
}
static bool same(const Affine& a, const Affine& b) { return fe_eq(a.x, b.x) && fe_eq(a.y, b.y); }

// an affine point as the Jacobian limbs an MSM would return, with a random z (the identity: z = 0)
static Jac as_jacobian(const Affine& a) {
    Jac j;
    if (affine_is_identity(a)) {
        j.x = fe_zero<FqP>();
        j.y = fe_one<FqP>();
        j.z = fe_zero<FqP>();
        return j;
    }
    Fe z = fe_from_u64<FqP>(rnd() | 1);
    Fe z2 = fe_sqr<FqP>(z);
    j.x = fe_mul<FqP>(a.x, z2);
    j.y = fe_mul<FqP>(a.y, fe_mul<FqP>(z2, z));
    j.z = z;
    return j;
}

struct Case {
    std::vector<Affine> addends;  // empty: none
    std::vector<Fe> scalars;      // canonical, m x t
    std::vector<Affine> points;
    size_t m;
};

static void run(const Case& c) {
    const size_t m = c.m, t = c.points.size();
    std::vector<Jac> jac;
    for (const Affine& a : c.addends) jac.push_back(as_jacobian(a));
    std::vector<Fe> mont;
    for (const Fe& s : c.scalars) mont.push_back(fe_from_canonical<FrP>(s));
    std::vector<Affine> out(m);
    char why[160] = "";
    int rc = g1h::linear_combinations(jac.empty() ? nullptr : (const uint64_t*)jac.data(), mont.empty() ? nullptr : (const uint64_t*)mont.data(),
                                      t ? (const uint64_t*)c.points.data() : nullptr, m, t, m ? (uint64_t*)out.data() : nullptr, why, sizeof(why));
    CHECK(rc == 0);
    if (rc) {
        printf("  rejected: %s\n", why);
        return;
    }
    for (size_t j = 0; j < m; j++) {
        XYZZ acc = c.addends.empty() ? xyzz_identity() : xyzz_from_affine(c.addends[j]);
        for (size_t i = 0; i < t; i++) xyzz_add(acc, ref_mul(c.points[i], c.scalars[j * t + i]));
        CHECK(same(out[j], xyzz_to_affine(acc)));
        CHECK(affine_on_curve(out[j]));
    }
}

static void rejected(const uint64_t* addends, const uint64_t* scalars, const uint64_t* points, size_t m, size_t t, uint64_t* out, const char* text) {
    char why[160] = "";
    int rc = g1h::linear_combinations(addends, scalars, points, m, t, out, why, sizeof(why));
    CHECK(rc == 1);
    if (std::string(why) != text) {
        printf("  got \"%s\", want \"%s\"\n", why, text);
        failures++;
    }
}

int main() {
    const size_t shapes[5][2] = {{1, 1}, {2, 2}, {5, 1}, {1, 40}, {3, 0}};
    for (auto& sh : shapes) {
        Case c;
        c.m = sh[0];
        for (size_t i = 0; i < sh[1]; i++) c.points.push_back(rnd_point());
        for (size_t i = 0; i < sh[0] * sh[1]; i++) c.scalars.push_back(rnd_canon());
        for (size_t j = 0; j < sh[0]; j++) c.addends.push_back(rnd_point());
        run(c);
        if (sh[1]) {
            c.addends.clear();
            run(c);
        }
    }
    const Affine P = rnd_point(), S = rnd_point(), A = rnd_point();
    const Fe s = rnd_canon(), zero = canon_u64(0), one = canon_u64(1), three = canon_u64(3), top = r_minus_1();
    // the scalars 0, 1 and r - 1, with and without addends
    run({{A, A, A, A}, {zero, one, one, top, top, zero, zero, zero}, {P, S}, 4});
    run({{}, {zero, one, one, top, top, zero, zero, zero}, {P, S}, 4});
    // a (0, 0) point; an identity addend
    run({{A}, {s, three}, {identity(), S}, 1});
    run({{}, {s}, {identity()}, 1});
    run({{identity(), identity()}, {s, three, zero, zero}, {P, S}, 2});
    // the addend equals the rest of the sum (a doubling closes it), then its negative (the identity comes out)
    XYZZ rest_x = ref_mul(P, s);
    xyzz_add(rest_x, ref_mul(S, three));
    const Affine rest = xyzz_to_affine(rest_x);
    run({{rest}, {s, three}, {P, S}, 1});
    run({{affine_neg(rest), A}, {s, three, s, three}, {P, S}, 2});
    // equal and opposite points under equal scalars
    run({{A}, {s, s}, {P, P}, 1});
    run({{A}, {s, s}, {P, affine_neg(P)}, 1});
    run({{}, {s, s}, {P, affine_neg(P)}, 1});
    run({{}, {one, one}, {P, P}, 1});
    // t = 0 (a batch normalisation with an identity in the middle) and m = 0
    run({{A, identity(), P}, {}, {}, 3});
    run({{}, {}, {P}, 0});
    char why[8];
    CHECK(g1h::linear_combinations(nullptr, nullptr, nullptr, 0, 3, nullptr, why, sizeof(why)) == 0);

    // every rejection, with its text
    uint64_t out[16], big[8], sc[8], pts[16], off[8];
    const Fe m1 = fe_one<FrP>(), q3 = fe_from_u64<FqP>(3);
    memset(big, 0xff, sizeof(big));
    memcpy(sc, &m1, 32);
    memcpy(sc + 4, big, 32);
    memcpy(pts, &P, 64);
    memcpy(pts + 8, &P, 64);
    memcpy(off, &P, 64);
    memcpy(off + 4, &q3, 32);  // P's x with y = 3: off the curve
    rejected(nullptr, sc, pts, 1, 2, out, "scalars[1] is not a reduced Fr element");
    memcpy(pts + 8, off, 64);
    memcpy(sc + 4, &m1, 32);
    rejected(nullptr, sc, pts, 1, 2, out, "points_xy[1] is neither on the curve nor (0, 0)");
    memcpy(pts, big, 32);
    rejected(nullptr, sc, pts, 1, 1, out, "points_xy[0] is neither on the curve nor (0, 0)");
    memcpy(pts, &P, 64);
    rejected(nullptr, sc, pts, 1, 1, nullptr, "null out_xy");
    rejected(nullptr, nullptr, pts, 1, 1, out, "null scalars");
    rejected(nullptr, sc, nullptr, 1, 1, out, "null points_xy");
    rejected(nullptr, sc, pts, 4097, 1, out, "m = 4097 sums of t = 1 terms are more than 4096 terms: that is an MSM");
    rejected(nullptr, sc, pts, 2, 2049, out, "m = 2 sums of t = 2049 terms are more than 4096 terms: that is an MSM");
    rejected(nullptr, sc, pts, (size_t)1 << 63, 4, out, "m = 9223372036854775808 sums of t = 4 terms are more than 4096 terms: that is an MSM");

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("g1 lincomb host tests ok\n");
    return 0;
}
