// Host-side fuzz of the native table records of csrc/ecu.h (AffineU, xyzzu_add_native: what msm_accum_kernel runs over a fixed-base
// window table) against csrc/ec.h.  Built with -DH2_FU_CHECK so that every product and every limb-wise addition asserts its bounds.
// No GPU and no library: the same H2_HD source compiles for the host.  Driven by tests/test_ecu_native_host.py (plain and sanitised).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-pse_amd/csrc/ecu.h"

using namespace h2;

static uint64_t rs = 0x7ab1e5;
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

static bool fe_same(const Fe& a, const Fe& b) { return memcmp(a.l, b.l, sizeof(a.l)) == 0; }

static bool same_point(const XYZZu& u, const XYZZ& s) {
    if (xyzz_is_identity(s) || xyzzu_is_identity(u)) return xyzz_is_identity(s) && xyzzu_is_identity(u);
    const Affine a = xyzz_to_affine(xyzzu_to_ext(u)), b = xyzz_to_affine(s);
    return fe_same(a.x, b.x) && fe_same(a.y, b.y);
}

// the accumulator's invariants at the top of ecu.h: limbs 0..7 in [0, 2^29), a small top limb
static bool normalised(const Fu& a) {
    for (int i = 0; i < 8; i++)
        if (a.l[i] < 0 || a.l[i] >= (1 << 29)) return false;
    return a.l[8] > -(1 << 26) && a.l[8] < (1 << 26);
}
static bool acc_ok(const XYZZu& u) { return normalised(u.x) && normalised(u.y) && normalised(u.zz) && normalised(u.zzz); }

// the record's contract: canonical limbs, top limb below 2^22, the marker; the identity is the all-zero record
static bool record_ok(const AffineU& r) {
    if (!r.valid) {
        const AffineU z = {};
        return memcmp(&r, &z, sizeof(r)) == 0;
    }
    for (int i = 0; i < 9; i++)
        if (r.x.l[i] < 0 || r.y.l[i] < 0 || r.x.l[i] >= (i < 8 ? 1 << 29 : 1 << 22) || r.y.l[i] >= (i < 8 ? 1 << 29 : 1 << 22)) return false;
    return r.valid == 1 && r.pad == 0 && fe_is_canonical<Q>(fu_canon<QU>(r.x)) && fe_same(fu_canon<QU>(r.x), fu_canon<QU>(fu_norm(r.x)));
}

struct Both {  // the same chain on both sides
    XYZZ s = xyzz_identity();
    XYZZu u = xyzzu_identity();
    uint32_t id = 1;
    void add(const Affine& p, bool neg) {
        xyzz_add_mixed(s, neg ? affine_neg(p) : p);
        xyzzu_add_native(u, id, affineu_from_ext(p), neg);
        CHECK(id == (xyzzu_is_identity(u) ? 1u : 0u));
        CHECK(acc_ok(u));
    }
    bool same() const { return same_point(u, s); }
};

static void test_conversion() {
    // field elements: 0, 1, p - 1 as E-form values and as the integers behind them, limbs all ones, random
    for (int it = 0; it < 20000; it++) {
        Fe a;
        for (int j = 0; j < 8; j++) a.l[j] = (uint32_t)rnd();
        a.l[7] &= 0x1fffffff;
        if (it == 0) a = fe_zero<Q>();
        if (it == 1) a = fe_one<Q>();
        if (it == 2) a = fe_neg<Q>(fe_one<Q>());  // the field's p - 1
        if (it == 3) {  // the integer 1 / p - 1 as stored words
            a = fe_zero<Q>();
            a.l[0] = 1;
        }
        if (it == 4) {
            a = fe_zero<Q>();
            a.l[0] = 1;
            a = fe_neg<Q>(a);
        }
        if (it == 5)
            for (int j = 0; j < 8; j++) a.l[j] = 0xffffffffu;  // all ones: not canonical, brought below p next
        if (!fe_is_canonical<Q>(a)) a.l[7] &= 0x0fffffff;
        if (!fe_is_canonical<Q>(a)) a.l[7] = 0;
        const Fu n = fu_native_from_ext(a);
        for (int i = 0; i < 9; i++) CHECK(n.l[i] >= 0 && n.l[i] < (i < 8 ? 1 << 29 : 1 << 22));
        CHECK(fe_same(fu_native_to_ext(n), a));
        // the value: I-form = E-form * 2^5
        Fe a32 = a;
        for (int k = 0; k < 5; k++) a32 = fe_dbl<Q>(a32);
        CHECK(fe_same(fu_canon<QU>(n), a32));
    }
    // limbs all ones: the largest record limbs the multiplier can meet (not a field element below p: only the bounds are checked)
    Fu ones;
    for (int i = 0; i < 9; i++) ones.l[i] = i < 8 ? (1 << 29) - 1 : (1 << 22) - 1;
    (void)fu_mul<QU>(ones, ones);
    (void)fu_mul<QU>(fu_neg(ones), ones);
    (void)fu_native_to_ext(ones);
    // points: identity <-> the all-zero record
    Affine ident;
    ident.x = fe_zero<Q>();
    ident.y = fe_zero<Q>();
    const AffineU z = affineu_from_ext(ident);
    CHECK(record_ok(z) && !z.valid && affine_is_identity(affineu_to_ext(z)));
}

int main() {
    test_conversion();
    // points: multiples of the generator (1, 2), x coordinates spread
    Affine g;
    g.x = fe_from_u64<Q>(1);
    g.y = fe_from_u64<Q>(2);
    const int NP = 64;
    std::vector<Affine> pts;
    XYZZ cur = xyzz_identity();
    for (int i = 0; i < NP; i++) {
        xyzz_add_mixed(cur, g);
        XYZZ big = cur;
        for (int k = 0; k < 40 + i; k++) big = xyzz_double(big);
        xyzz_add(big, cur);
        pts.push_back(xyzz_to_affine(big));
        const AffineU r = affineu_from_ext(pts.back());
        CHECK(record_ok(r));
        const Affine back = affineu_to_ext(r);
        CHECK(fe_same(back.x, pts.back().x) && fe_same(back.y, pts.back().y));
    }
    Affine ident;
    ident.x = fe_zero<Q>();
    ident.y = fe_zero<Q>();

    // 10^5 additions in random signed chains, with repeats (doubling), inverses (cancellation) and identity records; every chain
    // starts from a fresh accumulator (the first-entry path) or from a loaded one (a streamed MSM's continued sum)
    int adds = 0;
    while (adds < 100000) {
        Both b;
        if (rnd() & 1) {  // continued: the accumulator comes from memory, the flag from its marker
            XYZZ s = xyzz_identity();
            const int k = (int)(rnd() % 4);
            for (int i = 0; i < k; i++) xyzz_add_mixed(s, pts[rnd() % NP]);
            b.s = s;
            b.u = xyzzu_from_ext(s);
            b.id = xyzzu_is_identity(b.u) ? 1u : 0u;
        }
        const int len = 1 + (int)(rnd() % 300);
        int last = 0;
        bool lastneg = false;
        for (int i = 0; i < len; i++, adds++) {
            const int r = (int)(rnd() % 100);
            int idx = (int)(rnd() % NP);
            bool neg = rnd() & 1;
            if (r < 5) { idx = last; neg = lastneg; }
            else if (r < 10) { idx = last; neg = !lastneg; }
            b.add((r >= 10 && r < 13) ? ident : pts[idx], neg);
            last = idx;
            lastneg = neg;
            if ((i & 15) == 0) CHECK(b.same());
        }
        CHECK(b.same());
    }
    // the exceptional cases, entry by entry, from a fresh accumulator and both signs
    for (int i = 0; i < NP; i++)
        for (int sg = 0; sg < 2; sg++) {
            const bool n = sg != 0;
            const Affine &P = pts[i], &Qp = pts[(i + 7) % NP];
            {  // P, P
                Both b;
                b.add(P, n); b.add(P, n);
                CHECK(b.same() && !b.id);
            }
            {  // P, -P, Q
                Both b;
                b.add(P, n); b.add(P, !n);
                CHECK(b.id == 1 && xyzz_is_identity(b.s));
                b.add(Qp, n);
                CHECK(b.same() && !b.id);
            }
            {  // P, -P, Q, Q
                Both b;
                b.add(P, n); b.add(P, !n); b.add(Qp, n); b.add(Qp, n);
                CHECK(b.same() && !b.id);
            }
            {  // identity records: first, in the middle, all of them
                Both b;
                b.add(ident, n); b.add(P, n); b.add(ident, !n); b.add(Qp, n);
                CHECK(b.same());
                Both c;
                c.add(ident, n); c.add(ident, !n); c.add(ident, n);
                CHECK(c.id == 1 && xyzzu_is_identity(c.u));
            }
            {  // 2P then -P then -P: a doubling's result cancelled in two steps
                Both b;
                b.add(P, n); b.add(P, n); b.add(P, !n); b.add(P, !n);
                CHECK(b.id == 1 && xyzz_is_identity(b.s));
            }
        }
    printf(failures ? "ECU NATIVE TESTS FAILED (%d)\n" : "ecu native tests ok (%d additions)\n", failures ? failures : adds);
    return failures ? 1 : 0;
}
