// The NTT tiles' lazily reduced arithmetic under bound assertions, on the host.
//
// csrc/ntt.hip keeps a tile's values unreduced across butterfly stages and relies on bounds its comments state: four fresh values add
// up to < 4.5 p, every later round adds < 2.3 p, the canonicalising store accepts 16 p, every fu_mul operand stays below 2^30 per
// limb, loose limbs below 2^31.  tests/cpp/test_fieldu.cpp asserts the bounds of single operations; this program asserts them for
// the composition the tiles make, on the inputs that walk the worst paths (tests/ntt_edge_util.py names the same ones).
//
// It restates, serially and with the H2_HD functions of csrc/fieldu.h, the schedules of
//   dft_lds   ntt.hip:143-190  (s = 1..10: stage pairs in "LDS", a lone last stage for odd s)
//   dft_col   ntt.hip:280-341  (s = 8..11: the first stage pair on the loaded values or the `quarter` copy, rounds through the
//                               image, the last round or the lone last stage left loose in registers)
//   ntt_load  ntt.hip:192-203  (the coset constant by pick3 on load, zero beyond in_len)
// and their closing stores (ntt.hip:228, :255, :387, :413: fu_mul_canon by a twiddle, or fu_canon_fast), with the same stage
// pairing, the same places of fu_norm and the same skipped unit twiddles.  The LDS swizzle is a bijection of the image's indices and
// is left out; a column is a column whichever lane takes it.  Built with -DH2_FU_CHECK, so the H2_FU_ASSERTs of fieldu.h are live.
//
// Asserted: |value| < 16 p at every canonicalising store, every fu_mul operand limb below 2^30, every limb that stays loose below
// 2^31 (fu_add / fu_sub assert it), and the canonical result equal to a plain field.h DFT of the tile.  Printed: the largest
// |value| / p at a store and the largest operand and loose limbs, per kernel and s (DESIGN.md records them).
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <vector>

#include "../../halo2-pse_amd/csrc/fieldu.h"

using namespace h2;
typedef FrUA U;  // what the kernels instantiate; on the host its multiplier is the plain column scan
typedef FrP P;

static char g_ctx[160] = "start";  // what runs now: printed when an assert of fieldu.h aborts
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

static uint64_t rs = 0x7E57ED6E;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------------------------------------ measurements
struct Stats {
    long double store = 0;  // largest |value| / p at a canonicalising store
    int64_t operand = 0;    // largest |limb| of a fu_mul operand (data or twiddle)
    int64_t loose = 0;      // largest |limb| of a value that reaches a store without fu_norm
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

static long double value_over_p(const Fu& a) {
    long double v = 0, p = 0;
    for (int i = 8; i >= 0; i--) {
        v = v * 536870912.0L + (long double)a.l[i];
        p = p * 536870912.0L + (long double)U::P[i];
    }
    return (v < 0 ? -v : v) / p;
}

// the sign of 16 p + sgn * value, exactly (64-bit limbs, carries propagated)
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

static Fu mul(const Fu& a, const Fu& w) {  // a butterfly's product, its operands measured
    const int64_t ma = max_limb(a), mw = max_limb(w);
    if (ma > g_st->operand) g_st->operand = ma;
    if (mw > g_st->operand) g_st->operand = mw;
    CHECK(ma < (1ll << 30) && mw < (1ll << 30));
    return fu_mul<U>(a, w);
}

static void at_store(const Fu& x) {  // what both closing reductions require of their operand
    const long double q = value_over_p(x);
    if (q > g_st->store) g_st->store = q;
    const int64_t m = max_limb(x);
    if (m > g_st->loose) g_st->loose = m;
    CHECK(m < (1ll << 31));
    CHECK(sign_16p_plus(x, 1) > 0 && sign_16p_plus(x, -1) > 0);  // -16 p < value < 16 p
}

static Fe store_direct(const Fu& x) {  // ntt.hip:255, :413 without an output constant
    at_store(x);
    return fu_canon_fast<U>(x);
}

static Fe store_mul(const Fu& x, const Fu& w) {  // ntt.hip:228, :387, and :255, :413 with one
    at_store(x);
    const Fu xp = fu_norm(fu_add(x, fu_const<U>(U::P16)));  // the operand fu_mul_canon forms
    const int64_t m = max_limb(xp), mw = max_limb(w);
    if (m > g_st->operand) g_st->operand = m;
    if (mw > g_st->operand) g_st->operand = mw;
    CHECK(m < (1ll << 30) && mw < (1ll << 30));
    return fu_mul_canon<U>(x, w);
}

// ------------------------------------------------------------------------------------------------ field.h side
static Fe fe_raw(uint32_t w7, uint32_t fill) {
    Fe a;
    for (int i = 0; i < 7; i++) a.l[i] = fill;
    a.l[7] = w7;
    return a;
}

static Fu fu_i_from_fe(const Fe& x) {  // ntt.hip:260-264
    Fe t = x;
    for (int k = 0; k < 5; k++) t = fe_dbl<P>(t);
    return fu_slice(t);
}

static Fe root_of_order(uint32_t s) {  // omega of exact order 2^s
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

// the reference's radix-2 network on canonical values (arithmetic.rs:186-230), checked below against the O(n^2) sum
static void ref_fft(std::vector<Fe>& a, const Fe& w, uint32_t s) {
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

static void check_ref_fft() {
    for (uint32_t s = 0; s <= 6; s++) {
        const uint32_t n = 1u << s;
        const Fe w = root_of_order(s);
        std::vector<Fe> a(n);
        for (auto& v : a) {
            for (int j = 0; j < 8; j++) v.l[j] = (uint32_t)rnd();
            v.l[7] &= 0x1fffffff;
        }
        std::vector<Fe> f = a;
        ref_fft(f, w, s);
        for (uint32_t i = 0; i < n; i++) {
            Fe sum = fe_zero<P>();
            for (uint32_t j = 0; j < n; j++) sum = fe_add<P>(sum, fe_mul<P>(a[j], fe_pow_u64<P>(w, (uint64_t)i * j)));
            CHECK(fe_eq(sum, f[i]));
        }
    }
}

// ------------------------------------------------------------------------------------------------ the tiles
struct Tile {
    uint32_t s;
    Fe omega;               // of order 2^s
    std::vector<Fu> wtab;   // w_R^i, i < R / 2, I-form (stage_twiddle_build_kernel)
    std::vector<Fu> close;  // an inter-pass twiddle per output, I-form canonical ...
    std::vector<Fe> close_fe;  // ... and the same as field.h sees it
    Fu in3[3];
    Fe in3_fe[3];
};

static Tile make_tile(uint32_t s) {
    Tile t;
    t.s = s;
    t.omega = root_of_order(s);
    const uint32_t R = 1u << s;
    Fe p = fe_one<P>();
    for (uint32_t i = 0; i < (R >> 1) || i < 1; i++) {
        t.wtab.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, t.omega);
    }
    // w_N^(k lo) for N = 2^(s + 11), lo = 1365: what a first pass of 2^11 columns multiplies output k by
    const Fe wn = fe_pow_u64<P>(root_of_order(s + 11 > P::S ? P::S : s + 11), 1365);
    p = fe_one<P>();
    for (uint32_t k = 0; k < R; k++) {
        t.close_fe.push_back(p);
        t.close.push_back(fu_i_from_fe(p));
        p = fe_mul<P>(p, wn);
    }
    t.in3_fe[0] = fe_one<P>();  // NttScale::into_coset: 1, zeta, zeta^2
    for (int i = 0; i < 8; i++) t.in3_fe[1].l[i] = P::ZETA[i];
    t.in3_fe[2] = fe_sqr<P>(t.in3_fe[1]);
    for (int i = 0; i < 3; i++) t.in3[i] = fu_i_from_fe(t.in3_fe[i]);
    return t;
}

// ntt_load: row r of the tile lies at global index r * stride + lo; `coset` 0: plain, else the index's residue picks the constant
static Fu load(const Tile& t, const std::vector<Fe>& a, uint32_t r, uint32_t in_len, uint32_t coset) {
    if (r >= in_len) return fu_zero();
    Fu v = fu_slice(a[r]);
    if (coset) {
        const uint32_t m = (r * coset + 1) % 3u;  // stride 2^x = 1 or 2 mod 3, lo = 1
        if (m) v = mul(v, t.in3[m]);
    }
    return v;
}

static Fe load_ref(const Tile& t, const std::vector<Fe>& a, uint32_t r, uint32_t in_len, uint32_t coset) {
    if (r >= in_len) return fe_zero<P>();
    return coset ? fe_mul<P>(a[r], t.in3_fe[(r * coset + 1) % 3u]) : a[r];
}

// dft_lds on one column: x[bitrev(r)] on entry, x[k] on exit
static void dft_lds(std::vector<Fu>& x, const Tile& t) {
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

// dft_col for every lane t of R / 4, one after the other per round: lane t brings v[m] = row t + m R/4 (the OWN form brings other rows
// to other lanes, the same four to one lane) and leaves with outputs t + m R/4
static void dft_col(std::vector<Fu>& x, const Tile& tl, const std::vector<Fu>& rows, std::vector<Fu>& out, bool quarter) {
    const uint32_t s = tl.s, R = 1u << s, T = R >> 2;
    const Fu* wtab = tl.wtab.data();
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b0 = bitrev(t, s - 2) << 2;
        const Fu v[4] = {rows[t], rows[t + T], rows[t + 2 * T], rows[t + 3 * T]};
        if (quarter) {
            const Fu n0 = fu_norm(v[0]);
            x[b0] = n0;
            x[b0 ^ 1] = n0;
            x[b0 ^ 2] = n0;
            x[b0 ^ 3] = n0;
        } else {
            const Fu y0 = fu_add(v[0], v[2]), y1 = fu_sub(v[0], v[2]), y2 = fu_add(v[1], v[3]), y3 = fu_sub(v[1], v[3]);
            const Fu u3 = mul(y3, wtab[1u << (s - 2)]);
            x[b0] = fu_norm(fu_add(y0, y2));
            x[b0 ^ 2] = fu_norm(fu_sub(y0, y2));
            x[b0 ^ 1] = fu_norm(fu_add(y1, u3));
            x[b0 ^ 3] = fu_norm(fu_sub(y1, u3));
        }
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
            if (last) {  // base = t here: the group of half-size R / 4 is the lane's own outputs
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

// one column through one kernel: load, transform, both closing stores, against field.h
static void run_column(Kernel kern, const Tile& t, const std::vector<Fe>& a, uint32_t in_len, uint32_t coset) {
    const uint32_t s = t.s, R = 1u << s;
    std::vector<Fe> want(R);
    for (uint32_t r = 0; r < R; r++) want[r] = load_ref(t, a, r, in_len, coset);
    ref_fft(want, t.omega, s);
    std::vector<Fu> out(R);
    if (kern == LDS) {
        for (uint32_t r = 0; r < R; r++) out[bitrev(r, s)] = load(t, a, r, in_len, coset);
        dft_lds(out, t);
    } else {
        std::vector<Fu> rows(R), x(R);
        for (uint32_t r = 0; r < R; r++) rows[r] = load(t, a, r, in_len, coset);
        dft_col(x, t, rows, out, in_len * 4 <= R);
    }
    for (uint32_t k = 0; k < R; k++) {
        CHECK(fe_eq(store_direct(out[k]), want[k]));
        CHECK(fe_eq(store_mul(out[k], t.close[k]), fe_mul<P>(want[k], t.close_fe[k])));
    }
}

// ------------------------------------------------------------------------------------------------ the inputs
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

static void run_inputs(Kernel kern, const Tile& t, uint32_t in_len, uint32_t coset, int seeded, const char* what) {
    const uint32_t s = t.s, R = 1u << s, n = in_len;  // the patterns fill the rows that are read
    const std::vector<Fe> vals = values();
    const Fe zero = fe_zero<P>();
    std::vector<Fe> a(R, zero);
    auto go = [&](const char* pat, size_t ci, uint32_t arg) {
        snprintf(g_ctx, sizeof g_ctx, "%s s=%u in_len=%u coset=%u %s(%s, %u)", what, s, in_len, coset, pat, VALUE_NAMES[ci], arg);
        run_column(kern, t, a, in_len, coset);
    };
    for (size_t ci = 0; ci < vals.size(); ci++) {
        const Fe c = vals[ci], nc = fe_neg<P>(c);
        for (uint32_t j = 0; j < n; j++) a[j] = c;
        go("const", ci, 0);
        for (uint32_t j = 0; j < n; j++) a[j] = (j & 1) ? nc : c;
        go("nyquist", ci, 0);
        for (uint32_t j = 0; j < n; j++) a[j] = (j & 1) ? zero : c;
        go("even_only", ci, 0);
        const uint32_t rows[4] = {0, 1, n / 2, n - 1};
        for (uint32_t m : rows) {
            for (uint32_t j = 0; j < n; j++) a[j] = zero;
            a[m] = c;
            go("delta", ci, m);
        }
        const uint32_t tones[2] = {1, R - 1};
        for (uint32_t tn : tones) {  // a[j] = c w^(-tone j): every stage's twiddle turns the operands back onto one another
            const Fe step = fe_pow_u64<P>(t.omega, (uint64_t)(R - tn) % R);
            Fe p = fe_one<P>();
            for (uint32_t j = 0; j < n; j++) {
                a[j] = fe_mul<P>(c, p);
                p = fe_mul<P>(p, step);
            }
            go("tone", ci, tn);
        }
        for (int k = 0; k < 3; k++) {
            for (uint32_t j = 0; j < n; j++) a[j] = (rnd() & 1) ? nc : c;
            go("signs", ci, (uint32_t)k);
        }
    }
    for (int k = 0; k < seeded; k++) {
        for (uint32_t j = 0; j < n; j++) a[j] = vals[rnd() % vals.size()];
        snprintf(g_ctx, sizeof g_ctx, "%s s=%u in_len=%u coset=%u extremes #%d", what, s, in_len, coset, k);
        run_column(kern, t, a, in_len, coset);
    }
}

static void report(const char* name, uint32_t s, const Stats& st) {
    printf("%-22s s=%2u  max |value|/p at a store %7.4Lf (of 16)  max fu_mul operand limb %lld = 2^%.3f (of 2^30)  max loose limb %lld = 2^%.3f (of 2^31)\n",
           name, s, st.store, (long long)st.operand, __builtin_log2((double)(st.operand ? st.operand : 1)), (long long)st.loose,
           __builtin_log2((double)(st.loose ? st.loose : 1)));
    CHECK(st.store < 16.0L);
}

int main() {
    signal(SIGABRT, on_abort);
    check_ref_fft();
    for (uint32_t s = 1; s <= 10; s++) {
        const Tile t = make_tile(s);
        const uint32_t R = 1u << s;
        const int seeded = s <= 8 ? 240 : 90;
        Stats st;
        g_st = &st;
        run_inputs(LDS, t, R, 0, seeded, "dft_lds");
        report("dft_lds", s, st);
        Stats sc;
        g_st = &sc;
        run_inputs(LDS, t, R, 1, seeded / 3, "dft_lds coset");
        run_inputs(LDS, t, R, 2, seeded / 3, "dft_lds coset");
        run_inputs(LDS, t, R >> 1, 1, seeded / 3, "dft_lds coset padded");
        report("dft_lds coset load", s, sc);
    }
    for (uint32_t s = 8; s <= 11; s++) {
        const Tile t = make_tile(s);
        const uint32_t R = 1u << s;
        const int seeded = s <= 9 ? 150 : 60;
        Stats st;
        g_st = &st;
        run_inputs(COL, t, R, 0, seeded, "dft_col");
        report("dft_col", s, st);
        Stats sc;
        g_st = &sc;
        run_inputs(COL, t, R, 1, seeded / 3, "dft_col coset");
        run_inputs(COL, t, R, 2, seeded / 3, "dft_col coset");
        run_inputs(COL, t, R >> 1, 2, seeded / 3, "dft_col coset padded");
        report("dft_col coset load", s, sc);
        Stats sq;
        g_st = &sq;
        run_inputs(COL, t, R >> 2, 1, seeded / 3, "dft_col quarter");
        run_inputs(COL, t, R >> 3, 2, seeded / 3, "dft_col quarter");
        report("dft_col quarter", s, sq);
    }
    printf(failures ? "NTT BOUND TESTS FAILED (%d)\n" : "ntt bounds ok\n", failures);
    return failures ? 1 : 0;
}
