// Host-side fuzz of the unit form of the mixed addition in csrc/ecu.h (xyzzu_add_mixed_nonid with unit = true: the addition onto an
// accumulator that is a bucket's first record, zz = zzz = one) and of the state word the accumulate loops carry (xyzzu_add_native_st,
// xyzzu_add_affine with ACC_*), against csrc/ec.h.  Built with -DH2_FU_CHECK so that every product and every limb-wise addition asserts
// its bounds.  No GPU and no library: the same H2_HD source compiles for the host, where a "wave" is one lane, so the unit form is taken
// exactly when the lane's accumulator is a unit point.  Driven by tests/test_ecu_unit_host.py (plain and sanitised).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-pse_amd/csrc/ecu.h"

using namespace h2;

static uint64_t rs = 0x0171ce;
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
static bool fu_same(const Fu& a, const Fu& b) { return memcmp(a.l, b.l, sizeof(a.l)) == 0; }

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

// value bounds of the header comment: |x|, |y| < 4.5 p, zz and zzz in (-0.1 p, 1.4 p); checked on the canonical-plus-k p decomposition
// of the top limb (p's top limb is 0x30644e, so the top limb of k p is about k * 0x30644e)
static bool value_ok(const XYZZu& u) {
    const int64_t P8 = 0x30644e;
    auto within = [&](const Fu& a, double lo, double hi) { return (double)a.l[8] > lo * (double)P8 - 2 && (double)a.l[8] < hi * (double)P8 + 2; };
    return within(u.x, -4.5, 4.5) && within(u.y, -4.5, 4.5) && within(u.zz, -0.1, 1.4) && within(u.zzz, -0.1, 1.4);
}

static Affine ident_point() {
    Affine o;
    o.x = fe_zero<Q>();
    o.y = fe_zero<Q>();
    return o;
}

// the same chain on three sides: ec.h, native records with the state word, E-form points with the state word
struct Chain {
    XYZZ s = xyzz_identity();
    XYZZu n = xyzzu_identity(), e = xyzzu_identity();
    uint32_t nst = ACC_IDENTITY, est = ACC_IDENTITY;
    void add(const Affine& p, bool neg) {
        xyzz_add_mixed(s, neg ? affine_neg(p) : p);
        const uint32_t nb = nst, eb = est;
        xyzzu_add_native_st(n, nst, affineu_from_ext(p), neg);
        xyzzu_add_affine(e, est, p, neg);
        const bool id = affine_is_identity(p);
        for (int k = 0; k < 2; k++) {
            const XYZZu& u = k ? e : n;
            const uint32_t before = k ? eb : nb, st = k ? est : nst;
            CHECK(acc_ok(u) && value_ok(u));
            CHECK((st == ACC_IDENTITY) == xyzzu_is_identity(u));
            if (id) CHECK(st == before);                                      // an identity record changes nothing
            else if (before == ACC_IDENTITY) CHECK(st == ACC_UNIT);           // the copy of a first record
            else CHECK(st == ACC_POINT || st == ACC_IDENTITY);                // any addition clears the unit state
            if (st == ACC_UNIT) CHECK(fu_same(u.zz, fu_one_i<QU>()) && fu_same(u.zzz, fu_one_i<QU>()));
        }
    }
    bool same() const { return same_point(n, s) && same_point(e, s); }
};

// the unit form and the general form from the same unit accumulator: the same group element, and the unit form's ZZ3 = PP, ZZZ3 = PPP
static void both_forms(const Affine& a, bool na, const Affine& b, bool nb) {
    XYZZ s = xyzz_identity();
    xyzz_add_mixed(s, na ? affine_neg(a) : a);
    xyzz_add_mixed(s, nb ? affine_neg(b) : b);
    {  // native
        XYZZu u = xyzzu_identity();
        uint32_t st = ACC_IDENTITY;
        xyzzu_add_native_st(u, st, affineu_from_ext(a), na);
        CHECK(st == ACC_UNIT);
        XYZZu g = u;
        const AffineU r = affineu_from_ext(b);
        Fu py = r.y;
        if (nb) py = fu_neg(py);
        const bool ok_u = xyzzu_add_mixed_nonid<QU, true>(u, r.x, py, true);
        const bool ok_g = xyzzu_add_mixed_nonid<QU, true>(g, r.x, py, false);
        CHECK(ok_u == ok_g && ok_u == !xyzz_is_identity(s));
        CHECK(same_point(u, s) && same_point(g, s) && acc_ok(u) && value_ok(u));
    }
    {  // E-form
        XYZZu u = xyzzu_identity();
        uint32_t st = ACC_IDENTITY;
        xyzzu_add_affine(u, st, a, na);
        CHECK(st == ACC_UNIT);
        XYZZu g = u;
        Fu px = fu_from_ext(b.x), py = fu_from_ext(b.y);
        if (nb) py = fu_neg(py);
        const bool ok_u = xyzzu_add_mixed_nonid<QU, false>(u, px, py, true);
        const bool ok_g = xyzzu_add_mixed_nonid<QU, false>(g, px, py, false);
        CHECK(ok_u == ok_g && ok_u == !xyzz_is_identity(s));
        CHECK(same_point(u, s) && same_point(g, s) && acc_ok(u) && value_ok(u));
    }
}

// the asserted bounds at their extremes: coordinates 0, 1 and p - 1 (as integers behind the native limbs and as field elements), in
// every pairing and both signs.  These are not points of the curve: only H2_FU_CHECK's assertions and the invariants are checked.
static void test_extremes() {
    std::vector<Fe> vals;
    Fe one_int = fe_zero<Q>();
    one_int.l[0] = 1;
    vals.push_back(fe_zero<Q>());               // 0
    vals.push_back(fe_one<Q>());                // the field's 1
    vals.push_back(fe_neg<Q>(fe_one<Q>()));     // the field's p - 1
    vals.push_back(one_int);                    // the stored integer 1
    vals.push_back(fe_neg<Q>(one_int));         // the stored integer p - 1
    int runs = 0;
    for (const Fe& x1 : vals)
        for (const Fe& y1 : vals)
            for (const Fe& x2 : vals)
                for (const Fe& y2 : vals)
                    for (int sg = 0; sg < 4; sg++) {
                        if (fe_same(x1, x2)) continue;  // equal x: the exceptional cases, exercised on real points below
                        AffineU a, b;
                        a.x = fu_native_from_ext(x1); a.y = fu_native_from_ext(y1); a.valid = 1; a.pad = 0;
                        b.x = fu_native_from_ext(x2); b.y = fu_native_from_ext(y2); b.valid = 1; b.pad = 0;
                        XYZZu u = xyzzu_identity();
                        uint32_t st = ACC_IDENTITY;
                        xyzzu_add_native_st(u, st, a, (sg & 1) != 0);
                        CHECK(st == ACC_UNIT && acc_ok(u));
                        xyzzu_add_native_st(u, st, b, (sg & 2) != 0);
                        CHECK(st == ACC_POINT && acc_ok(u) && value_ok(u));
                        Affine ea, eb;
                        ea.x = x1; ea.y = y1; eb.x = x2; eb.y = y2;
                        if (affine_is_identity(ea) || affine_is_identity(eb)) continue;
                        XYZZu v = xyzzu_identity();
                        uint32_t vst = ACC_IDENTITY;
                        xyzzu_add_affine(v, vst, ea, (sg & 1) != 0);
                        xyzzu_add_affine(v, vst, eb, (sg & 2) != 0);
                        CHECK(vst == ACC_POINT && acc_ok(v) && value_ok(v));
                        runs++;
                    }
    CHECK(runs > 1000);
    // limbs all ones: the largest record limbs the unit form can meet, against the smallest
    AffineU hi, lo;
    for (int i = 0; i < 9; i++) {
        hi.x.l[i] = hi.y.l[i] = i < 8 ? (1 << 29) - 1 : (1 << 22) - 1;
        lo.x.l[i] = lo.y.l[i] = 0;
    }
    lo.x.l[0] = 1;
    hi.valid = lo.valid = 1;
    hi.pad = lo.pad = 0;
    for (int sg = 0; sg < 4; sg++)
        for (int ord = 0; ord < 2; ord++) {
            XYZZu u = xyzzu_identity();
            uint32_t st = ACC_IDENTITY;
            xyzzu_add_native_st(u, st, ord ? hi : lo, (sg & 1) != 0);
            xyzzu_add_native_st(u, st, ord ? lo : hi, (sg & 2) != 0);
            CHECK(st == ACC_POINT && acc_ok(u));
        }
}

int main(int argc, char** argv) {
    // an optional argument divides the fuzz counts (the sanitised build runs a tenth); the exceptional cases always run in full
    const int divide = argc > 1 ? atoi(argv[1]) : 1;
    if (divide < 1) return 2;
    test_extremes();
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
    }
    const Affine ident = ident_point();

    // random pairs and every exceptional pairing, the unit form against the general form and ec.h
    int pairs = 0;
    for (int i = 0; i < NP; i++)
        for (int j = 0; j < NP; j++)
            if (j == i || (i + j) % divide == 0)
                for (int sg = 0; sg < 4; sg++, pairs++) both_forms(pts[i], (sg & 1) != 0, pts[j], (sg & 2) != 0);  // j == i: P + P and P + (-P)
    {  // the same x and a different y is -P, the only other point of the curve with that x: a pairing of its own for the record
        const Affine m = affine_neg(pts[3]);
        both_forms(pts[3], false, m, false);
        both_forms(m, true, pts[3], true);
    }

    // short chains, as the buckets of a wide window hold them: 1 to 4 records with repeats, inverses and identity records anywhere
    int adds = 0;
    while (adds < 60000 / divide) {
        Chain c;
        const int len = 1 + (int)(rnd() % 4);
        int last = (int)(rnd() % NP);
        bool lastneg = rnd() & 1;
        for (int i = 0; i < len; i++, adds++) {
            const int r = (int)(rnd() % 100);
            int idx = (int)(rnd() % NP);
            bool neg = rnd() & 1;
            if (i > 0 && r < 15) { idx = last; neg = lastneg; }
            else if (i > 0 && r < 30) { idx = last; neg = !lastneg; }
            c.add((r >= 30 && r < 40) ? ident : pts[idx], neg);
            if (!(r >= 30 && r < 40)) { last = idx; lastneg = neg; }
            CHECK(c.same());
        }
    }
    // the exceptional cases on the SECOND record, entry by entry, both signs
    for (int i = 0; i < NP; i++)
        for (int sg = 0; sg < 2; sg++) {
            const bool n = sg != 0;
            const Affine &P = pts[i], &Qp = pts[(i + 7) % NP];
            {  // P, P: a doubling on the second record, then an ordinary addition
                Chain c;
                c.add(P, n); c.add(P, n);
                CHECK(c.same() && c.nst == ACC_POINT && c.est == ACC_POINT);
                c.add(Qp, n);
                CHECK(c.same());
            }
            {  // P, -P, Q: a cancellation on the second record, then a copy onto the identity, then the unit form again
                Chain c;
                c.add(P, n); c.add(P, !n);
                CHECK(c.nst == ACC_IDENTITY && c.est == ACC_IDENTITY && xyzz_is_identity(c.s));
                c.add(Qp, n);
                CHECK(c.same() && c.nst == ACC_UNIT && c.est == ACC_UNIT);
                c.add(P, n);
                CHECK(c.same() && c.nst == ACC_POINT);
            }
            {  // an identity record first, and an identity record second (the unit state survives it)
                Chain c;
                c.add(ident, n); c.add(P, n);
                CHECK(c.nst == ACC_UNIT && c.est == ACC_UNIT);
                c.add(ident, !n);
                CHECK(c.nst == ACC_UNIT && c.est == ACC_UNIT);
                c.add(Qp, !n);
                CHECK(c.same() && c.nst == ACC_POINT && c.est == ACC_POINT);
                c.add(Qp, !n);  // and a doubling-free third: 2Q - ... stays a point
                CHECK(c.same());
            }
            {  // P, P, -P, -P: a doubling's result cancelled in two general steps
                Chain c;
                c.add(P, n); c.add(P, n); c.add(P, !n); c.add(P, !n);
                CHECK(c.nst == ACC_IDENTITY && c.est == ACC_IDENTITY && xyzz_is_identity(c.s));
            }
        }
    // the two-valued word of xyzzu_add_native (0 / 1) never takes the unit form and still agrees
    for (int i = 0; i < NP; i++) {
        XYZZu u = xyzzu_identity();
        uint32_t id = 1;
        XYZZ s = xyzz_identity();
        for (int k = 0; k < 3; k++) {
            xyzzu_add_native(u, id, affineu_from_ext(pts[(i + 5 * k) % NP]), k == 1);
            xyzz_add_mixed(s, k == 1 ? affine_neg(pts[(i + 5 * k) % NP]) : pts[(i + 5 * k) % NP]);
        }
        CHECK(id == 0 && same_point(u, s));
    }
    printf(failures ? "ECU UNIT TESTS FAILED (%d)\n" : "ecu unit tests ok (%d pairs, %d chained additions)\n", failures ? failures : pairs, adds);
    return failures ? 1 : 0;
}
