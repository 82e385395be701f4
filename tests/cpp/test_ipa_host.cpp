// Host-side test of what csrc/ipa.hip's kernels do to one element (csrc/ipa_elem.h), against arithmetic that shares nothing with it but
// the 256-bit field of field.h: the uniform-scalar ladder and the collapse of one pair against plain double-and-add over the whole
// 254-bit scalar in ec.h's canonical coordinates; the fold, the byte-table product of compute_s and the powers against fe_mul / fe_add /
// fe_pow_u64.  Built with -DH2_FU_CHECK, so every product and every limb-wise sum asserts fieldu.h's bounds -- on u = 0, 1, r - 1, the
// scalar with the longest GLV halves found, and random scalars.  No GPU and no library: the same H2_HD source compiles for the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-pse_amd/csrc/ipa_elem.h"

using namespace h2;

static uint64_t rs = 0x19a2d0;
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

// a random canonical scalar below r, and the same in Montgomery form
static Fe rnd_canon() {
    Fe c;
    for (int j = 0; j < 8; j++) c.l[j] = (uint32_t)rnd();
    c.l[7] &= 0x0fffffffu;  // < 2^252 < r
    return c;
}
static Fe rnd_fr() { return fe_from_canonical<FrP>(rnd_canon()); }

// [k] p by double-and-add over all 254 bits, ec.h only
static Affine ref_mul(const Affine& p, const Fe& k_canon) {
    XYZZ acc = xyzz_identity();
    for (int i = 253; i >= 0; i--) {
        acc = xyzz_double(acc);
        if ((k_canon.l[i >> 5] >> (i & 31)) & 1) xyzz_add_mixed(acc, p);
    }
    return xyzz_to_affine(acc);
}
static Affine ref_add(const Affine& a, const Affine& b) {
    XYZZ t = xyzz_from_affine(a);
    xyzz_add_mixed(t, b);
    return xyzz_to_affine(t);
}
static bool same(const Affine& a, const Affine& b) { return fe_eq(a.x, b.x) && fe_eq(a.y, b.y); }

static int bits5(const uint32_t a[5]) {
    for (int i = 159; i >= 0; i--)
        if ((a[i >> 5] >> (i & 31)) & 1) return i + 1;
    return 0;
}

static void check_scalar(const Fe& k_canon, const std::vector<Affine>& pts) {
    const IpaDigits dg = ipa_digits(k_canon.l);
    CHECK(dg.len <= IPA_MAX_COLUMNS - 1);
    const Affine id = {fe_zero<FqP>(), fe_zero<FqP>()};
    for (const Affine& p : pts) {
        const Affine want = ref_mul(p, k_canon);
        CHECK(same(xyzz_to_affine(xyzzu_to_ext(ipa_mul_affine(p, dg))), want));
        CHECK(affine_on_curve(want) || affine_is_identity(want));
        // the collapse of one pair: a general lo, and the rows the group law treats apart
        const Affine lo = pts[(size_t)(rnd() % pts.size())];
        CHECK(same(xyzz_to_affine(ipa_collapse_elem(lo, p, dg)), ref_add(lo, want)));
        CHECK(same(xyzz_to_affine(ipa_collapse_elem(id, p, dg)), want));                          // g[i] the identity
        CHECK(same(xyzz_to_affine(ipa_collapse_elem(lo, id, dg)), lo));                           // g[half + i] the identity
        CHECK(affine_is_identity(xyzz_to_affine(ipa_collapse_elem(id, id, dg))));                 // both
        CHECK(same(xyzz_to_affine(ipa_collapse_elem(want, p, dg)), ref_add(want, want)));         // a doubling
        CHECK(affine_is_identity(xyzz_to_affine(ipa_collapse_elem(affine_neg(want), p, dg))));    // the result is (0, 0)
    }
}

int main(int argc, char** argv) {
    const int divide = argc > 1 ? atoi(argv[1]) : 1;  // the sanitised build runs a fraction of the random cases
    // ---- points: the generator (1, 2) and multiples of it ----
    Affine gen;
    gen.x = fe_from_u64<FqP>(1);
    gen.y = fe_from_u64<FqP>(2);
    CHECK(affine_on_curve(gen));
    std::vector<Affine> pts = {gen};
    for (int i = 0; i < 3; i++) pts.push_back(ref_mul(gen, rnd_canon()));

    // ---- the ladder and the collapse ----
    Fe zero, one, rm1;
    memset(zero.l, 0, 32);
    one = zero, one.l[0] = 1;
    memcpy(rm1.l, FrP::MOD, 32), rm1.l[0] -= 1;
    CHECK(ipa_digits(zero.l).len == 0);
    check_scalar(zero, pts);
    check_scalar(one, pts);
    check_scalar(rm1, pts);
    // the scalar whose GLV halves are the longest of many: the ladder's column count and the carries of the recoding at their maximum
    Fe longest = one;
    int longest_bits = 0;
    for (int it = 0; it < 200000 / divide; it++) {
        Fe k = rnd_canon();
        if (it % 3 == 0) k.l[7] |= 0x20000000u;  // up to 2^254: may exceed r, reduce
        Fe red;
        fe_cond_sub<FrP>(red, k.l);
        const GlvScalar g = glv_decompose(red.l);
        const int b = bits5(g.k1) > bits5(g.k2) ? bits5(g.k1) : bits5(g.k2);
        if (b > longest_bits) longest_bits = b, longest = red;
    }
    CHECK(longest_bits >= 126 && longest_bits <= 130);
    check_scalar(longest, pts);
    for (int it = 0; it < 60 / divide + 2; it++) check_scalar(rnd_canon(), pts);
    // powers of two and their neighbours: long carry chains in the recoding
    for (int bit = 1; bit < 253; bit += 31) {
        Fe k = zero;
        k.l[bit >> 5] = 1u << (bit & 31);
        check_scalar(k, pts);
        for (int j = 0; j < (bit >> 5); j++) k.l[j] = 0xffffffffu;  // 2^bit - 1
        k.l[bit >> 5] = (1u << (bit & 31)) - 1;
        check_scalar(k, pts);
    }

    // ---- Fr: product, fold ----
    const Fe fr_edge[] = {fe_zero<FrP>(), fe_one<FrP>(), fe_from_canonical<FrP>(rm1), fe_from_u64<FrP>(2)};
    std::vector<Fe> frs(fr_edge, fr_edge + 4);
    for (int i = 0; i < 40; i++) frs.push_back(rnd_fr());
    {   // raw limb patterns just below r: the largest canonical E-form values
        Fe top;
        memcpy(top.l, FrP::MOD, 32);
        top.l[0] -= 1;
        frs.push_back(top);
        top.l[0] -= 1;
        frs.push_back(top);
    }
    for (const Fe& a : frs)
        for (const Fe& b : frs) {
            const Fe m = ipa_fr_mul(a, b);
            CHECK(fe_is_canonical<FrP>(m) && fe_eq(m, fe_mul<FrP>(a, b)));
            const Fe c = frs[(size_t)(rnd() % frs.size())];
            const Fe f = ipa_fold_elem(a, b, c);
            CHECK(fe_is_canonical<FrP>(f) && fe_eq(f, fe_add<FrP>(a, fe_mul<FrP>(c, b))));
        }

    // ---- the byte tables: powers and compute_s ----
    std::vector<Fe> T(IPA_TABLE_ELEMS);
    for (const Fe& x : {fe_zero<FrP>(), fe_one<FrP>(), fe_from_canonical<FrP>(rm1), rnd_fr()}) {
        for (uint64_t n : {1ull, 2ull, 255ull, 256ull, 257ull, 65536ull, 65537ull, 1ull << 24, (1ull << 24) + 1, 1ull << 28}) {
            const uint32_t levels = ipa_powers_table(x, n, T.data());
            CHECK(levels == (n <= 256 ? 1u : n <= 65536 ? 2u : n <= (1ull << 24) ? 3u : 4u));
            const uint64_t at[] = {0, 1, n / 2, n - 1, (n - 1) & 0x00ff00ffull, (n - 1) & 0xff00ff00ull, rnd() % n};
            for (uint64_t i : at) CHECK(fe_eq(ipa_table_elem(T.data(), levels, i), fe_pow_u64<FrP>(x, i)));
        }
    }
    for (uint32_t k = 1; k <= 28; k++) {
        std::vector<Fe> u(k);
        for (uint32_t j = 0; j < k; j++) u[j] = rnd_fr();
        if (k % 5 == 0) u[k / 2] = fe_one<FrP>();
        if (k % 7 == 0) u[0] = fe_from_canonical<FrP>(rm1);
        const Fe init = k % 3 == 0 ? fe_one<FrP>() : rnd_fr();
        const uint32_t levels = ipa_s_table(u.data(), k, init, T.data());
        CHECK(levels == (k + 7) / 8);
        const uint64_t n = 1ull << k;
        const int samples = k <= 8 ? (int)n : 300 / divide + 8;
        for (int it = 0; it < samples; it++) {
            const uint64_t i = k <= 8 ? (uint64_t)it : it == 0 ? n - 1 : rnd() % n;
            Fe want = init;  // strategy.rs:161-176 as a product: bit t of i selects u[k - 1 - t]
            for (uint32_t t = 0; t < k; t++)
                if ((i >> t) & 1) want = fe_mul<FrP>(want, u[k - 1 - t]);
            CHECK(fe_eq(ipa_table_elem(T.data(), levels, i), want));
        }
    }

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ipa host tests ok\n");
    return 0;
}
