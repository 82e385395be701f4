// The part mode of the NTT's first-pass load (csrc/ntt.hip, ntt_load<true>) under bound assertions, on the host.
//
// coeff_to_extended_part multiplies element m by g_p^m = c3[m mod 3] * extended_omega^(part * m) while the first pass loads it, the power
// combined from the extended domain's two-level table: two fu_mul for the power, one for the data.  tests/cpp/test_ntt_bounds.cpp
// asserts the tiles' bounds for the loads that existed before (plain, and the zeta constant by pick3); this program asserts that the
// new load hands the first butterfly round nothing that round does not already accept from the zeta path:
//   * every fu_mul operand limb below 2^30 (table entries, c3, the combined power, the sliced data),
//   * the loaded value in [0, 1.125 r) with limbs 0..7 in [0, 2^29) -- "four fresh values add up to < 4.5 r", the bound the first
//     stage pair of dft_lds / dft_col is written for (ntt.hip) --, and in fact below 1.01 r, the bound the zeta path's product has,
//   * and equal, once reduced, to a[m] * g_p^m computed with field.h.
// Then whole tiles run from that load through the restated schedules of dft_lds (s = 1..10) and dft_col (s = 8..11) to both closing
// stores, with the store's bounds asserted (|value| < 16 r, loose limbs below 2^31) and the result compared with a plain field.h DFT.
// Built with -DH2_FU_CHECK, so the H2_FU_ASSERTs of fieldu.h are live.  Inputs: the extreme stored words (0, 1, r - 1, r - 2, ...),
// constant, alternating and single-coefficient columns, and seeded mixtures; parts 0, 1 and P - 1 for P = 2, 4, 8.
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <vector>

#include "../../halo2-pse_amd/csrc/fieldu.h"

using namespace h2;
typedef FrUA U;
typedef FrP P;

static char g_ctx[200] = "start";
static void on_abort(int) {
    const char* m = "\nbound assertion fired in: ";
    (void)!write(2, m, strlen(m));
    (void)!write(2, g_ctx, strlen(g_ctx));
    (void)!write(2, "\n", 1);
}
static int failures = 0;
#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            if (failures < 20) printf("FAIL line %d: %s   [%s]\n", __LINE__, #c, g_ctx); \
            failures++;                                                                 \
        }                                                                               \
    } while (0)

static uint64_t rs = 0x9A27C05E7;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

struct Stats {
    long double load = 0;   // largest value / r the load hands to the first round
    long double power = 0;  // largest value / r of the combined power g
    long double store = 0;  // largest |value| / r at a canonicalising store
    int64_t operand = 0;    // largest |limb| of a fu_mul operand
    int64_t loose = 0;      // largest |limb| at a store
};
static Stats* g_st;

static int64_t max_limb(const Fu& a) {
    int64_t m = 0;
    for (int i = 0; i < 9; i++) {
        const int64_t x = a.l[i] < 0 ? -(int64_t)a.l[i] : a.l[i];
        if (x > m) m = x;
    }
    return m;
}
static long double value_over_p(const Fu& a, bool* negative = nullptr) {
    long double v = 0, p = 0;
    for (int i = 8; i >= 0; i--) {
        v = v * 536870912.0L + (long double)a.l[i];
        p = p * 536870912.0L + (long double)U::P[i];
    }
    if (negative) *negative = v < 0;
    return (v < 0 ? -v : v) / p;
}
static int sign_16p_plus(const Fu& a, int sgn) {
    int64_t t[9], c = 0;
    for (int i = 0; i < 9; i++) {
        const int64_t v = (int64_t)U::P16[i] + sgn * (int64_t)a.l[i] + c;
        if (i < 8) {
            t[i] = v & H2_MASK29;
            c = v >> 29;
        } else {
            t[i] = v;
        }
    }
    if (t[8]) return t[8] < 0 ? -1 : 1;
    for (int i = 0; i < 8; i++)
        if (t[i]) return 1;
    return 0;
}
static Fu mul(const Fu& a, const Fu& w) {
    const int64_t ma = max_limb(a), mw = max_limb(w);
    if (ma > g_st->operand) g_st->operand = ma;
    if (mw > g_st->operand) g_st->operand = mw;
    CHECK(ma < (1ll << 30) && mw < (1ll << 30));
    return fu_mul<U>(a, w);
}
static void at_store(const Fu& x) {
    const long double q = value_over_p(x);
    if (q > g_st->store) g_st->store = q;
    const int64_t m = max_limb(x);
    if (m > g_st->loose) g_st->loose = m;
    CHECK(m < (1ll << 31));
    CHECK(sign_16p_plus(x, 1) > 0 && sign_16p_plus(x, -1) > 0);
}
static Fe store_direct(const Fu& x) {
    at_store(x);
    return fu_canon_fast<U>(x);
}
static Fe store_mul(const Fu& x, const Fu& w) {
    at_store(x);
    const Fu xp = fu_norm(fu_add(x, fu_const<U>(U::P16)));
    const int64_t m = max_limb(xp), mw = max_limb(w);
    if (m > g_st->operand) g_st->operand = m;
    if (mw > g_st->operand) g_st->operand = mw;
    CHECK(m < (1ll << 30) && mw < (1ll << 30));
    return fu_mul_canon<U>(x, w);
}

static Fu fu_i_from_fe(const Fe& x) {  // ntt.hip, fu_i_from_fe
    Fe t = x;
    for (int k = 0; k < 5; k++) t = fe_dbl<P>(t);
    return fu_slice(t);
}
static Fe root_of_order(uint32_t s) {
    Fe w;
    for (int i = 0; i < 8; i++) w.l[i] = P::ROOT_OF_UNITY[i];
    for (uint32_t i = s; i < P::S; i++) w = fe_sqr<P>(w);
    return w;
}
static uint32_t bitrev(uint32_t k, uint32_t s) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < s; i++) r |= ((k >> i) & 1) << (s - 1 - i);
    return r;
}
static void ref_fft(std::vector<Fe>& a, const Fe& w, uint32_t s) {  // the reference's radix-2 network (arithmetic.rs:186-230)
    const uint32_t n = 1u << s;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t r = bitrev(i, s);
        if (i < r) std::swap(a[i], a[r]);
    }
    for (uint32_t st = 0; st < s; st++) {
        const uint32_t h = 1u << st;
        const Fe step = fe_pow_u64<P>(w, n >> (st + 1));
        for (uint32_t base = 0; base < n; base += 2 * h) {
            Fe tw = fe_one<P>();
            for (uint32_t i = 0; i < h; i++) {
                const Fe t = fe_mul<P>(a[base + i + h], tw), u = a[base + i];
                a[base + i] = fe_add<P>(u, t);
                a[base + i + h] = fe_sub<P>(u, t);
                tw = fe_mul<P>(tw, step);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the part load
// One column of R = 2^s coefficients taken as a whole polynomial (k = s) of a domain extended by P = 2^log_p: the tables are the
// extended domain's, as twiddle_build_kernel fills them (lo_bits = min(ek, 10)).
struct PartTile {
    uint32_t s, log_p, ek, lo_bits;
    Fe omega, ext_omega;
    std::vector<Fu> wtab, close;
    std::vector<Fe> close_fe;
    std::vector<Fu> pow_lo, pow_hi;
    Fu c3[3];
    Fe c3_fe[3];
};

static PartTile make_tile(uint32_t s, uint32_t log_p) {
    PartTile t;
    t.s = s, t.log_p = log_p, t.ek = s + log_p;
    t.lo_bits = t.ek < 10 ? t.ek : 10;
    t.ext_omega = root_of_order(t.ek);
    t.omega = fe_pow_u64<P>(t.ext_omega, 1ull << log_p);
    const uint32_t R = 1u << s;
    Fe p = fe_one<P>();
    for (uint32_t i = 0; i < (R >> 1) || i < 1; i++) {
        t.wtab.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, t.omega);
    }
    const Fe wn = fe_pow_u64<P>(root_of_order(s + 11 > P::S ? P::S : s + 11), 1365);
    p = fe_one<P>();
    for (uint32_t k = 0; k < R; k++) {
        t.close_fe.push_back(p);
        t.close.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, wn);
    }
    p = fe_one<P>();
    for (uint32_t i = 0; i < (1u << t.lo_bits); i++) {
        t.pow_lo.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, t.ext_omega);
    }
    const Fe hi_step = p;  // ext_omega^(2^lo_bits)
    p = fe_one<P>();
    for (uint32_t i = 0; i < (1u << (t.ek - t.lo_bits)); i++) {
        t.pow_hi.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, hi_step);
    }
    t.c3_fe[0] = fe_one<P>();
    for (int i = 0; i < 8; i++) t.c3_fe[1].l[i] = P::ZETA[i];
    t.c3_fe[2] = fe_sqr<P>(t.c3_fe[1]);
    for (int i = 0; i < 3; i++) t.c3[i] = fu_i_from_fe(t.c3_fe[i]);
    return t;
}

// ntt_load<true>: element gi of the column, part `part`
static Fu load(const PartTile& t, const std::vector<Fe>& a, uint32_t gi, uint32_t part) {
    const uint32_t e = part * gi;
    CHECK((e & ((1u << t.lo_bits) - 1)) < t.pow_lo.size() && (e >> t.lo_bits) < t.pow_hi.size());  // part * gi < 2^ek: no reduction needed
    Fu g = mul(t.pow_lo[e & ((1u << t.lo_bits) - 1)], t.pow_hi[e >> t.lo_bits]);
    g = mul(g, t.c3[gi % 3u]);
    const long double gq = value_over_p(g);
    if (gq > g_st->power) g_st->power = gq;
    const Fu v = mul(fu_slice(a[gi]), g);
    bool neg;
    const long double q = value_over_p(v, &neg);
    if (q > g_st->load) g_st->load = q;
    CHECK(!neg && q < 1.125L);  // a fresh value: four of them stay below 4.5 r
    for (int i = 0; i < 8; i++) CHECK(v.l[i] >= 0 && v.l[i] < (1 << 29));
    return v;
}
static Fe load_ref(const PartTile& t, const std::vector<Fe>& a, uint32_t gi, uint32_t part) {
    const Fe g = fe_mul<P>(t.c3_fe[gi % 3u], fe_pow_u64<P>(t.ext_omega, (uint64_t)part * gi));
    return fe_mul<P>(a[gi], g);
}

// ------------------------------------------------------------------------------------------------ the tiles (ntt.hip's schedules)
static void dft_lds(std::vector<Fu>& x, const PartTile& t) {
    const uint32_t s = t.s, R = 1u << s;
    const Fu* wtab = t.wtab.data();
    uint32_t log_h = 0;
    for (; log_h + 2 <= s; log_h += 2) {
        const uint32_t h = 1u << log_h;
        for (uint32_t i = 0; i < (R >> 2); i++) {
            const uint32_t off = i & (h - 1), blk = i >> log_h;
            const uint32_t base = (blk << (log_h + 2)) + off, e1 = base + h, e2 = base + 2 * h, e3 = base + 3 * h;
            Fu x0 = x[base], x1 = x[e1], x2 = x[e2], x3 = x[e3];
            if (log_h) {
                const Fu wa = wtab[off << (s - 1 - log_h)];
                x1 = mul(x1, wa);
                x3 = mul(x3, wa);
            }
            const Fu y0 = fu_add(x0, x1), y1 = fu_sub(x0, x1), y2 = fu_add(x2, x3), y3 = fu_sub(x2, x3);
            const Fu u2 = log_h ? mul(y2, wtab[off << (s - 2 - log_h)]) : y2;
            const Fu u3 = mul(y3, wtab[(off + h) << (s - 2 - log_h)]);
            x[base] = fu_norm(fu_add(y0, u2));
            x[e2] = fu_norm(fu_sub(y0, u2));
            x[e1] = fu_norm(fu_add(y1, u3));
            x[e3] = fu_norm(fu_sub(y1, u3));
        }
    }
    if (log_h < s) {
        const uint32_t h = 1u << log_h;
        for (uint32_t i = 0; i < (R >> 1); i++) {
            const uint32_t off = i & (h - 1), blk = i >> log_h;
            const uint32_t i0 = (blk << (log_h + 1)) + off, i1 = i0 + h;
            const Fu a = x[i0];
            Fu tt = x[i1];
            if (log_h) tt = mul(tt, wtab[off << (s - 1 - log_h)]);
            x[i0] = fu_add(a, tt);
            x[i1] = fu_sub(a, tt);
        }
    }
}

static void dft_col(std::vector<Fu>& x, const PartTile& tl, const std::vector<Fu>& rows, std::vector<Fu>& out) {
    const uint32_t s = tl.s, R = 1u << s, T = R >> 2;
    const Fu* wtab = tl.wtab.data();
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b0 = bitrev(t, s - 2) << 2;
        const Fu v[4] = {rows[t], rows[t + T], rows[t + 2 * T], rows[t + 3 * T]};
        const Fu y0 = fu_add(v[0], v[2]), y1 = fu_sub(v[0], v[2]), y2 = fu_add(v[1], v[3]), y3 = fu_sub(v[1], v[3]);
        const Fu u3 = mul(y3, wtab[1u << (s - 2)]);
        x[b0] = fu_norm(fu_add(y0, y2));
        x[b0 ^ 2] = fu_norm(fu_sub(y0, y2));
        x[b0 ^ 1] = fu_norm(fu_add(y1, u3));
        x[b0 ^ 3] = fu_norm(fu_sub(y1, u3));
    }
    uint32_t log_h = 2;
    for (; log_h + 2 <= s; log_h += 2) {
        const bool last = log_h + 2 == s;
        const uint32_t h = 1u << log_h;
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t off = t & (h - 1), blk = t >> log_h;
            const uint32_t base = (blk << (log_h + 2)) + off, e1 = base + h, e2 = base + 2 * h, e3 = base + 3 * h;
            Fu x0 = x[base], x1 = x[e1], x2 = x[e2], x3 = x[e3];
            const Fu wa = wtab[off << (s - 1 - log_h)];
            x1 = mul(x1, wa);
            x3 = mul(x3, wa);
            const Fu y0 = fu_add(x0, x1), y1 = fu_sub(x0, x1), y2 = fu_add(x2, x3), y3 = fu_sub(x2, x3);
            const Fu u2 = mul(y2, wtab[off << (s - 2 - log_h)]);
            const Fu u3 = mul(y3, wtab[(off + h) << (s - 2 - log_h)]);
            if (last) {
                out[t] = fu_add(y0, u2);
                out[t + 2 * T] = fu_sub(y0, u2);
                out[t + T] = fu_add(y1, u3);
                out[t + 3 * T] = fu_sub(y1, u3);
                continue;
            }
            x[base] = fu_norm(fu_add(y0, u2));
            x[e2] = fu_norm(fu_sub(y0, u2));
            x[e1] = fu_norm(fu_add(y1, u3));
            x[e3] = fu_norm(fu_sub(y1, u3));
        }
        if (last) break;
    }
    if (s & 1) {
        const uint32_t q = T;
        for (uint32_t t = 0; t < T; t++) {
            const Fu a0 = x[t], a1 = x[t + q];
            const Fu t0 = mul(x[t + 2 * q], wtab[t]);
            const Fu t1 = mul(x[t + 3 * q], wtab[t + q]);
            out[t] = fu_add(a0, t0);
            out[t + 2 * q] = fu_sub(a0, t0);
            out[t + q] = fu_add(a1, t1);
            out[t + 3 * q] = fu_sub(a1, t1);
        }
    }
}

enum Kernel { LDS, COL };

static void run_column(Kernel kern, const PartTile& t, const std::vector<Fe>& a, uint32_t part) {
    const uint32_t s = t.s, R = 1u << s;
    std::vector<Fe> want(R);
    for (uint32_t r = 0; r < R; r++) want[r] = load_ref(t, a, r, part);
    std::vector<Fu> out(R);
    if (kern == LDS) {
        for (uint32_t r = 0; r < R; r++) {
            const Fu v = load(t, a, r, part);
            CHECK(fe_eq(fu_canon_fast<U>(v), want[r]));
            out[bitrev(r, s)] = v;
        }
        ref_fft(want, t.omega, s);
        dft_lds(out, t);
    } else {
        std::vector<Fu> rows(R), x(R);
        for (uint32_t r = 0; r < R; r++) rows[r] = load(t, a, r, part);
        ref_fft(want, t.omega, s);
        dft_col(x, t, rows, out);
    }
    for (uint32_t k = 0; k < R; k++) {
        CHECK(fe_eq(store_direct(out[k]), want[k]));
        CHECK(fe_eq(store_mul(out[k], t.close[k]), fe_mul<P>(want[k], t.close_fe[k])));
    }
}

static Fe fe_raw(uint32_t w7, uint32_t fill) {
    Fe a;
    for (int i = 0; i < 7; i++) a.l[i] = fill;
    a.l[7] = w7;
    return a;
}
static std::vector<Fe> values() {  // stored words, every one below r
    Fe rm;
    for (int i = 0; i < 8; i++) rm.l[i] = P::MOD[i];
    Fe zero = fe_zero<P>(), one = zero;
    one.l[0] = 1;
    Fe rm1 = rm, rm2 = rm, half;
    rm1.l[0] -= 1;
    rm2.l[0] -= 2;
    for (int i = 0; i < 8; i++) half.l[i] = (rm1.l[i] >> 1) | (i < 7 ? rm1.l[i + 1] << 31 : 0);
    Fe p253 = zero;
    p253.l[7] = 1u << 29;
    return {zero, one, rm1, rm2, fe_raw(0x30644dffu, 0xffffffffu), p253, half, fe_one<P>(), fe_neg<P>(fe_one<P>())};
}
static const char* VALUE_NAMES[] = {"0", "1", "r-1", "r-2", "limbmax", "2^253", "(r-1)/2", "ONE_E", "r-ONE_E"};

// light: the three stored words with the largest limbs and value only (r - 1, limbmax, ONE_E), for the large tiles
static void run_inputs(Kernel kern, const PartTile& t, uint32_t part, int seeded, const char* what, bool light = false) {
    const uint32_t s = t.s, n = 1u << s;
    const std::vector<Fe> vals = values();
    const Fe zero = fe_zero<P>();
    std::vector<Fe> a(n, zero);
    auto go = [&](const char* pat, size_t ci, uint32_t arg) {
        snprintf(g_ctx, sizeof g_ctx, "%s s=%u P=%u part=%u %s(%s, %u)", what, s, 1u << t.log_p, part, pat, VALUE_NAMES[ci], arg);
        run_column(kern, t, a, part);
    };
    for (size_t ci = 0; ci < vals.size(); ci++) {
        if (light && ci != 2 && ci != 4 && ci != 7) continue;
        const Fe c = vals[ci], nc = fe_neg<P>(c);
        for (uint32_t j = 0; j < n; j++) a[j] = c;
        go("const", ci, 0);
        for (uint32_t j = 0; j < n; j++) a[j] = (j & 1) ? nc : c;
        go("nyquist", ci, 0);
        const uint32_t rows[4] = {0, 1, 2 % n, n - 1};
        for (uint32_t m : rows) {
            for (uint32_t j = 0; j < n; j++) a[j] = zero;
            a[m] = c;
            go("delta", ci, m);
        }
        // a[j] = c g_p^(-j): the load turns every element into c, the column the tiles' bounds are tightest on
        {
            const Fe g = fe_mul<P>(t.c3_fe[1], fe_pow_u64<P>(t.ext_omega, part));
            const Fe gi = fe_pow_u64<P>(g, (3ull << t.ek) - 1);  // g^(3 * 2^ek) = 1
            Fe p = fe_one<P>();
            for (uint32_t j = 0; j < n; j++) {
                a[j] = fe_mul<P>(c, p);
                p = fe_mul<P>(p, gi);
            }
            go("undo", ci, 0);
        }
    }
    for (int k = 0; k < seeded; k++) {
        for (uint32_t j = 0; j < n; j++) a[j] = vals[rnd() % vals.size()];
        snprintf(g_ctx, sizeof g_ctx, "%s s=%u P=%u part=%u extremes #%d", what, s, 1u << t.log_p, part, k);
        run_column(kern, t, a, part);
    }
}

static void report(const char* name, uint32_t s, const Stats& st) {
    printf("%-18s s=%2u  max load value/r %.5Lf (of 1.125)  max power value/r %.5Lf  max |value|/r at a store %7.4Lf (of 16)  "
           "max fu_mul operand limb 2^%.3f (of 2^30)  max loose limb 2^%.3f (of 2^31)\n",
           name, s, st.load, st.power, st.store, __builtin_log2((double)(st.operand ? st.operand : 1)),
           __builtin_log2((double)(st.loose ? st.loose : 1)));
    CHECK(st.load < 1.01L);   // what the zeta path's product is bounded by: (r * r) / 2^261 + r
    CHECK(st.power < 1.01L);  // evalh_part_scale_kernel's bound for the same operands
    CHECK(st.store < 16.0L);
}

int main() {
    signal(SIGABRT, on_abort);
    for (uint32_t s = 1; s <= 10; s++) {
        Stats st;
        g_st = &st;
        for (uint32_t log_p = s <= 7 ? 1 : 3; log_p <= 3; log_p++) {  // the large tiles: P = 8 alone, whose exponents range widest
            const PartTile t = make_tile(s, log_p);
            const uint32_t Pn = 1u << log_p;
            const uint32_t parts[3] = {Pn - 1, 1, 0};
            for (int i = 0; i < (s > 7 ? 2 : Pn == 2 ? 2 : 3); i++) run_inputs(LDS, t, parts[i], s <= 7 ? 12 : 2, "dft_lds part load", s > 7);
        }
        report("dft_lds part load", s, st);
    }
    for (uint32_t s = 8; s <= 11; s++) {
        Stats st;
        g_st = &st;
        const PartTile t = make_tile(s, 3);
        run_inputs(COL, t, 7, 2, "dft_col part load", true);
        if (s == 8) run_inputs(COL, t, 1, 2, "dft_col part load", true);
        report("dft_col part load", s, st);
    }
    printf(failures ? "NTT PART BOUND TESTS FAILED (%d)\n" : "ntt part bounds ok\n", failures);
    return failures ? 1 : 0;
}
