// evaluate_h's lazily reduced arithmetic under bound assertions, on the host.
//
// csrc/evalh.hip runs every custom-gate and lookup graph as a program over the 9 x 29-bit multiplier of csrc/fieldu.h and keeps the
// values unreduced between operations.  compile_graph tracks a magnitude per operation (a column is < 32 r, a product of a and b is
// < a b / 169 + 1, sums add), requests a reduction where a value would pass 100 r and a closing one where the result would pass 15 r;
// evalh_perm_kernel and lookup_row (csrc/evalh_dev.h) carry their bounds as bracketed figures in comments; the per-circuit generated
// kernel emits two products that meet in a sum as ONE reduction (fu_mul_sub).  This program measures all of that on the inputs that
// walk the worst paths (tests/evalh_edge_util.py writes them: argv[1]).
//
// For every (graph, scenario) record and every row it runs
//   the interpreter leg   prog_eval (evalh.hip) op for op with the helpers of evalh_dev.h itself: addn, subn, mul_i, fu_sqr,
//                         fu_norm(fu_dbl), fu_norm(fu_neg), the FMA form, mul_i(out, one) on a reduce flag, out_e at the end
//   the fused leg         the same program as gen_source emits it with the reported fusion plan: fu_mul_sub for a fused ADD / SUB
//                         and for a Horner step whose addend is a product
//   the reference         the GRAPH (not the program) calculation by calculation with the saturated fe_add / fe_sub / fe_mul of field.h
// and restates, statement for statement, the row bodies of evalh_perm_kernel (evalh.hip) and lookup_row (evalh_dev.h; the header's own
// function runs beside the restatement and must store the same element).  Built with -DH2_FU_CHECK: the H2_FU_ASSERTs of fieldu.h and
// the accumulator assertion of fu_fused are live.
//
// Asserted, per row and op: the exact |value| / r is at most the magnitude compile_graph tracked for that op (both legs) or the
// bracketed figure of the kernel's comment at that statement; limbs 0..7 of every multiplier operand lie in [0, 2^29); |value| < 16 r at
// every out_e; the stored element is below r and equals the reference.  Over the corpus: a reduce flag was executed on each of ADD,
// SUB, DBL and FMA and (a hand-flagged copy of one program: the compiler itself cannot flag a product, 100 * 100 / 169 + 1 < 100) on
// MUL, the closing MOV|REDUCE ran, both fused shapes ran, some value passed 100 r before its reduction and some result was negative at
// out_e.  Printed: the maxima per op kind and per perm / lookup statement (DESIGN.md records them).
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#pragma GCC diagnostic ignored "-Wattributes"  // the address-space and vector-type attributes of the device helpers mean nothing to g++
#define __device__
#define __forceinline__ inline
#include "../../halo2-pse_amd/csrc/evalh_dev.h"

using namespace h2;
typedef FrP P;

static char g_ctx[256] = "start";  // what runs now: printed when an assert of fieldu.h aborts
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

static uint64_t rs = 0xE7A1B0D5;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------------------------------------ exact measurements
// the sign of M * r - sgn * value * 2^40 for an integer M >= 0, exactly: limb-wise in 128 bits, carries propagated
static int sign_of_mr_minus(const Fu& a, int sgn, __int128 M) {
    __int128 c = 0, t = 0;
    bool low = false;
    for (int i = 0; i < 9; i++) {
        t = M * (__int128)FrU::P[i] - (__int128)sgn * (__int128)a.l[i] * ((__int128)1 << 40) + c;
        if (i < 8) {
            if (t & H2_MASK29) low = true;
            c = t >> 29;  // arithmetic: floor
        }
    }
    return t > 0 ? 1 : t < 0 ? -1 : low ? 1 : 0;
}
static int value_sign(const Fu& a) { return -sign_of_mr_minus(a, 1, 0); }
// |value| <= floor(mag * 2^40) / 2^40 * r, exactly (the figure rounded DOWN to 2^-40: never laxer than the figure itself)
static bool abs_le(const Fu& a, double mag) {
    const __int128 M = (__int128)((long double)mag * 1099511627776.0L);
    return sign_of_mr_minus(a, 1, M) >= 0 && sign_of_mr_minus(a, -1, M) >= 0;
}
static bool abs_lt_16r(const Fu& a) { return sign_of_mr_minus(a, 1, (__int128)16 << 40) > 0 && sign_of_mr_minus(a, -1, (__int128)16 << 40) > 0; }
static long double over_r(const Fu& a) {  // |value| / r for the printed maxima
    long double v = 0, p = 0;
    for (int i = 8; i >= 0; i--) {
        v = v * 536870912.0L + (long double)a.l[i];
        p = p * 536870912.0L + (long double)FrU::P[i];
    }
    return (v < 0 ? -v : v) / p;
}

static int64_t g_max_operand_top = 0;
static void operand(const Fu& a) {  // what fu_mul asks of an operand: limbs 0..7 in [0, 2^29) (the top limb is covered by fu_fused's assertion)
    for (int i = 0; i < 8; i++) CHECK(a.l[i] >= 0 && a.l[i] < (1 << 29));
    const int64_t t = a.l[8] < 0 ? -(int64_t)a.l[8] : a.l[8];
    if (t > g_max_operand_top) g_max_operand_top = t;
}
static Fu MUL(const Fu& a, const Fu& b) {
    operand(a);
    operand(b);
    return mul_i(a, b);
}
static Fu SQR(const Fu& a) {
    operand(a);
    return fu_sqr<UF>(a);
}
// a b - c d (neg_c false) or a b + c d (neg_c true: the generator passes fu_neg(c)), one reduction
static Fu MULSUB(const Fu& a, const Fu& b, const Fu& c, const Fu& d, bool neg_c) {
    operand(a);
    operand(b);
    operand(c);
    operand(d);
    return fu_mul_sub<UF>(a, b, neg_c ? fu_neg(c) : c, d);
}
static Fu FOLD(const Fu& v, const Fu& y, const Fu& a, const Fu& b) {  // fold_y with its operands checked
    operand(v);
    operand(y);
    operand(a);
    operand(b);
    return fold_y(v, y, a, b);
}
static Fe OUT(const Fu& r) {
    CHECK(abs_lt_16r(r));
    const Fe e = out_e(r);
    CHECK(fe_is_canonical<P>(e));
    return e;
}

// E-form canonical element -> I-form canonical limbs (evalh.hip's to_i): x * 2^5 mod r, sliced
static Fu to_i(const Fe& x) {
    Fe t = x;
    for (int k = 0; k < 5; k++) t = fe_dbl<P>(t);
    return fu_slice(t);
}
static Fe fe_of(const uint8_t* p) {
    Fe x;
    memcpy(x.l, p, 32);
    return x;
}

// ------------------------------------------------------------------------------------------------ the records
enum { OP_ADD = 0, OP_SUB, OP_MUL, OP_SQR, OP_DBL, OP_NEG, OP_MOV, OP_FMA, OP_REDUCE_FLAG = 0x100 };
enum { VS_CONSTANT = 0, VS_INTERMEDIATE, VS_FIXED, VS_ADVICE, VS_INSTANCE, VS_CHALLENGE, VS_BETA, VS_GAMMA, VS_THETA, VS_Y, VS_PREVIOUS, VS_ZERO };
enum { CALC_ADD = 0, CALC_SUB, CALC_MUL, CALC_SQUARE, CALC_DOUBLE, CALC_NEGATE, CALC_HORNER, CALC_STORE };
static const char* const OP_NAME[8] = {"ADD", "SUB", "MUL", "SQR", "DBL", "NEG", "MOV", "FMA"};

struct Src {
    uint32_t kind, a, b;
};
struct Op {
    uint32_t op, dst;
    Src x, y;
};
struct Rec {
    char name[64];
    uint32_t log_rows, n_ops, n_slots;
    Src result;
    uint32_t n_constants, n_rotations, n_calcs, n_parts, num_intermediates, n_fixed, n_advice, n_instance, n_challenges;
    std::vector<Op> ops;
    std::vector<double> mags;
    std::vector<int32_t> fused_on, fused_off;
    std::vector<Fe> constants;
    std::vector<int32_t> rotations;
    std::vector<uint32_t> calcs, parts;
    std::vector<std::vector<Fe>> cols[3];  // fixed, advice, instance
    std::vector<Fe> challenges, previous;
    Fe beta, gamma, theta, y;
    // I-form canonical, as the host hands them to the kernels
    std::vector<Fu> constants_i, challenges_i;
    Fu beta_i, gamma_i, theta_i, y_i;
};

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    void take(void* dst, size_t n) {
        if (at + n > buf.size()) {
            printf("corpus file truncated at %zu\n", at);
            exit(2);
        }
        memcpy(dst, buf.data() + at, n);
        at += n;
    }
    uint32_t u32() {
        uint32_t v;
        take(&v, 4);
        return v;
    }
    template <class T>
    void vec(std::vector<T>& v, size_t n) {
        v.resize(n);
        if (n) take(v.data(), n * sizeof(T));
    }
};

static void read_rec(Reader& r, Rec& R) {
    r.take(R.name, 64);
    R.name[63] = 0;
    R.log_rows = r.u32();
    R.n_ops = r.u32();
    R.n_slots = r.u32();
    r.take(&R.result, 12);
    R.n_constants = r.u32();
    R.n_rotations = r.u32();
    R.n_calcs = r.u32();
    R.n_parts = r.u32();
    R.num_intermediates = r.u32();
    R.n_fixed = r.u32();
    R.n_advice = r.u32();
    R.n_instance = r.u32();
    R.n_challenges = r.u32();
    static_assert(sizeof(Op) == 32 && sizeof(Fe) == 32, "layouts of the file");
    r.vec(R.ops, R.n_ops);
    r.vec(R.mags, R.n_ops);
    r.vec(R.fused_on, R.n_ops);
    r.vec(R.fused_off, R.n_ops);
    r.vec(R.constants, R.n_constants);
    r.vec(R.rotations, R.n_rotations);
    r.vec(R.calcs, (size_t)R.n_calcs * 10);
    r.vec(R.parts, (size_t)R.n_parts * 3);
    const size_t n = (size_t)1 << R.log_rows;
    const uint32_t counts[3] = {R.n_fixed, R.n_advice, R.n_instance};
    for (int t = 0; t < 3; t++) {
        R.cols[t].resize(counts[t]);
        for (auto& c : R.cols[t]) r.vec(c, n);
    }
    r.vec(R.challenges, R.n_challenges);
    r.take(&R.beta, 32);
    r.take(&R.gamma, 32);
    r.take(&R.theta, 32);
    r.take(&R.y, 32);
    r.vec(R.previous, n);
    R.constants_i.clear();
    R.challenges_i.clear();
    for (const Fe& c : R.constants) R.constants_i.push_back(to_i(c));
    for (const Fe& c : R.challenges) R.challenges_i.push_back(to_i(c));
    R.beta_i = to_i(R.beta);
    R.gamma_i = to_i(R.gamma);
    R.theta_i = to_i(R.theta);
    R.y_i = to_i(R.y);
}

// ------------------------------------------------------------------------------------------------ counters over the corpus
struct KindStats {
    long double max_out = 0, max_pre = 0;  // |value| / r of the op's result, and of the value a reduce flag met
    uint64_t run = 0, flagged = 0;
};
static KindStats g_kind[2][8];  // [leg][op kind]
static uint64_t g_closing_mov = 0, g_fused_sum = 0, g_fused_horner = 0, g_negative_results = 0, g_rows = 0, g_out_e = 0;
static long double g_max_result = 0, g_max_pre_reduction = 0, g_min_slack = 1e9;

// ------------------------------------------------------------------------------------------------ the two legs
static uint32_t row_of(const Rec& R, uint32_t idx, uint32_t rot) { return rot_idx(idx, R.rotations[rot], 1, R.log_rows); }

static Fu get_i(const Rec& R, const Src& v, uint32_t idx, const std::vector<Fu>& slots, const Fu& previous) {  // vs_get
    switch (v.kind) {
        case VS_CONSTANT: return R.constants_i[v.a];
        case VS_INTERMEDIATE: return slots[v.a];
        case VS_FIXED: return ld_i(R.cols[0][v.a][row_of(R, idx, v.b)]);
        case VS_ADVICE: return ld_i(R.cols[1][v.a][row_of(R, idx, v.b)]);
        case VS_INSTANCE: return ld_i(R.cols[2][v.a][row_of(R, idx, v.b)]);
        case VS_CHALLENGE: return R.challenges_i[v.a];
        case VS_BETA: return R.beta_i;
        case VS_GAMMA: return R.gamma_i;
        case VS_THETA: return R.theta_i;
        case VS_Y: return R.y_i;
        case VS_PREVIOUS: return previous;
        default: return fu_zero();
    }
}

static void after_op(const Rec& R, int leg, uint32_t q, Fu& out) {
    const Op& o = R.ops[q];
    KindStats& s = g_kind[leg][o.op & 0xff];
    s.run++;
    if (o.op & OP_REDUCE_FLAG) {
        const long double pre = over_r(out);
        if (pre > s.max_pre) s.max_pre = pre;
        if (pre > g_max_pre_reduction) g_max_pre_reduction = pre;
        s.flagged++;
        if ((o.op & 0xff) == OP_MOV) g_closing_mov++;
        out = MUL(out, fu_one_i<UF>());
    }
    const long double m = over_r(out);
    if (m > s.max_out) s.max_out = m;
    if (R.mags[q] - (double)m < (double)g_min_slack) g_min_slack = R.mags[q] - (double)m;
    CHECK(abs_le(out, R.mags[q]));  // the magnitude compile_graph tracked for this op
    for (int i = 0; i < 8; i++) CHECK(out.l[i] >= 0 && out.l[i] < (1 << 29));  // every op leaves a normalised value
}

static const Op* product_of(const Rec& R, const std::vector<int32_t>& fused, uint32_t j, const Src& v) {  // gen_source's
    for (uint32_t i = 0; i < j; i++)
        if (fused[i] == (int32_t)j && v.kind == VS_INTERMEDIATE && R.ops[i].dst == v.a) return &R.ops[i];
    return nullptr;
}

// leg 0: prog_eval; leg 1: the generated kernel's statements under the fusion plan
static Fu run_program(const Rec& R, int leg, const std::vector<int32_t>& fused, uint32_t idx, const Fu& previous) {
    std::vector<Fu> slots(R.n_slots ? R.n_slots : 1, fu_zero());
    for (uint32_t q = 0; q < R.n_ops; q++) {
        const Op& o = R.ops[q];
        snprintf(g_ctx, sizeof(g_ctx), "%s row %u leg %d op %u (%s%s)", R.name, idx, leg, q, OP_NAME[o.op & 7], o.op & OP_REDUCE_FLAG ? "|REDUCE" : "");
        if (leg == 1 && fused[q] >= 0) continue;  // emitted inside its reader
        const uint32_t kind = o.op & 0xff;
        const Op *px = leg == 1 ? product_of(R, fused, q, o.x) : nullptr, *py = leg == 1 ? product_of(R, fused, q, o.y) : nullptr;
        Fu out;
        if ((kind == OP_ADD || kind == OP_SUB) && px && py) {
            out = MULSUB(get_i(R, px->x, idx, slots, previous), get_i(R, px->y, idx, slots, previous), get_i(R, py->x, idx, slots, previous),
                         get_i(R, py->y, idx, slots, previous), kind == OP_ADD);
            g_fused_sum++;
        } else if (kind == OP_FMA && px) {
            out = FOLD(slots[o.dst], get_i(R, o.y, idx, slots, previous), get_i(R, px->x, idx, slots, previous), get_i(R, px->y, idx, slots, previous));
            g_fused_horner++;
        } else {
            CHECK(!px && !py);  // a product is emitted inside a reader of exactly these two shapes
            const Fu a = get_i(R, o.x, idx, slots, previous);
            switch (kind) {
                case OP_ADD: out = addn(a, get_i(R, o.y, idx, slots, previous)); break;
                case OP_SUB: out = subn(a, get_i(R, o.y, idx, slots, previous)); break;
                case OP_MUL: out = MUL(a, get_i(R, o.y, idx, slots, previous)); break;
                case OP_SQR: out = SQR(a); break;
                case OP_DBL: out = fu_norm(fu_dbl(a)); break;
                case OP_NEG: out = fu_norm(fu_neg(a)); break;
                case OP_FMA: out = addn(MUL(slots[o.dst], get_i(R, o.y, idx, slots, previous)), a); break;
                default: out = a;  // OP_MOV
            }
        }
        after_op(R, leg, q, out);
        slots[o.dst] = out;
    }
    return get_i(R, R.result, idx, slots, previous);
}

static Fe result_e(const Rec& R, uint32_t idx, const Fu& r) {  // prog_result_e
    switch (R.result.kind) {
        case VS_FIXED: return R.cols[0][R.result.a][row_of(R, idx, R.result.b)];
        case VS_ADVICE: return R.cols[1][R.result.a][row_of(R, idx, R.result.b)];
        case VS_INSTANCE: return R.cols[2][R.result.a][row_of(R, idx, R.result.b)];
        case VS_PREVIOUS: return R.previous[idx];
        case VS_ZERO: return fe_zero<P>();
        default: {
            const long double m = over_r(r);
            if (m > g_max_result) g_max_result = m;
            if (value_sign(r) < 0) g_negative_results++;
            g_out_e++;
            return OUT(r);
        }
    }
}

// the graph itself (GraphEvaluator::evaluate, evaluation.rs:708-749) on canonical elements
static Fe get_e(const Rec& R, const uint32_t* v, uint32_t idx, const std::vector<Fe>& inter) {
    switch (v[0]) {
        case VS_CONSTANT: return R.constants[v[1]];
        case VS_INTERMEDIATE: return inter[v[1]];
        case VS_FIXED: return R.cols[0][v[1]][row_of(R, idx, v[2])];
        case VS_ADVICE: return R.cols[1][v[1]][row_of(R, idx, v[2])];
        case VS_INSTANCE: return R.cols[2][v[1]][row_of(R, idx, v[2])];
        case VS_CHALLENGE: return R.challenges[v[1]];
        case VS_BETA: return R.beta;
        case VS_GAMMA: return R.gamma;
        case VS_THETA: return R.theta;
        case VS_Y: return R.y;
        case VS_PREVIOUS: return R.previous[idx];
        default: return fe_zero<P>();
    }
}
static Fe reference(const Rec& R, uint32_t idx) {
    std::vector<Fe> inter(R.num_intermediates ? R.num_intermediates : 1, fe_zero<P>());
    Fe last = fe_zero<P>();
    for (uint32_t q = 0; q < R.n_calcs; q++) {
        const uint32_t* c = &R.calcs[(size_t)q * 10];
        const Fe x = get_e(R, c + 2, idx, inter);
        Fe v;
        switch (c[0]) {
            case CALC_ADD: v = fe_add<P>(x, get_e(R, c + 5, idx, inter)); break;
            case CALC_SUB: v = fe_sub<P>(x, get_e(R, c + 5, idx, inter)); break;
            case CALC_MUL: v = fe_mul<P>(x, get_e(R, c + 5, idx, inter)); break;
            case CALC_SQUARE: v = fe_mul<P>(x, x); break;
            case CALC_DOUBLE: v = fe_add<P>(x, x); break;
            case CALC_NEGATE: v = fe_sub<P>(fe_zero<P>(), x); break;
            case CALC_HORNER: {
                const Fe y = get_e(R, c + 5, idx, inter);
                v = x;
                for (uint32_t t = 0; t < c[9]; t++) v = fe_add<P>(fe_mul<P>(v, y), get_e(R, &R.parts[(size_t)(c[8] + t) * 3], idx, inter));
                break;
            }
            default: v = x;  // CALC_STORE
        }
        inter[c[1]] = v;
        last = v;
    }
    return last;
}

static void run_record(const Rec& R) {
    for (uint32_t q = 0; q < R.n_ops; q++) CHECK(R.fused_off[q] == -1);  // with the fusion off the generated kernel is the interpreter's statements
    for (uint32_t idx = 0; idx < (1u << R.log_rows); idx++) {
        const Fu prev = ld_i(R.previous[idx]);
        const Fe want = reference(R, idx);
        CHECK(fe_is_canonical<P>(want));
        for (int leg = 0; leg < 2; leg++) {
            const Fu r = run_program(R, leg, R.fused_on, idx, prev);
            snprintf(g_ctx, sizeof(g_ctx), "%s row %u leg %d result", R.name, idx, leg);
            const Fe got = result_e(R, idx, r);
            CHECK(fe_eq(got, want));
        }
        g_rows++;
    }
}

// ------------------------------------------------------------------------------------------------ the permutation and lookup rows
struct Stmt {
    const char* name;
    double figure;  // the bracketed figure of the kernel's comment
    long double max = 0;
};
static Stmt g_perm[] = {{"perm v loaded", 32}, {"perm 1 - z_0", 33}, {"perm fold l_0 (1 - z_0)", 8.5}, {"perm z_l^2 - z_l", 39.1}, {"perm fold l_last", 9.5},
                        {"perm z_i - z_(i-1)", 64}, {"perm fold l_0 (z_i - z_(i-1))", 14.3}, {"perm current_delta", 2}, {"perm left / right loaded", 32},
                        {"perm lterm", 34.2}, {"perm rterm", 35}, {"perm current_delta * delta", 1.1}, {"perm diff, one column", 14.1},
                        {"perm diff, more columns", 4.1}, {"perm left", 7.5}, {"perm right", 7.7}, {"perm fold l_active diff", 4.8},
                        {"perm stored", 15}};
enum { PV, P1Z, PF0, PZZ, PFL, PZD, PFZ, PCD, PLR, PLT, PRT, PCDD, PD1, PDN, PL, PR, PFA, PST };
static Stmt g_look[] = {{"lookup z / a' / s' / l_0 / l_active / v loaded", 32}, {"lookup a' - s'", 64}, {"lookup fold l_0 (1 - z)", 8.5},
                        {"lookup fold l_last (z^2 - z)", 9.5}, {"lookup z(wX) (a' + beta)", 7.3}, {"lookup diff", 8.5}, {"lookup fold l_active diff", 3.7},
                        {"lookup fold l_0 (a' - s')", 14.3}, {"lookup (a' - s')(a' - a'(w^-1 X))", 25.3}, {"lookup fold l_active", 6.9}};
enum { LLD, LAS, LF0, LFL, LZAB, LDIFF, LFD, LFAS, LMUL, LFA };
static Fu B(Stmt* tab, int s, const Fu& x) {  // the bracketed figure at a statement
    const long double m = over_r(x);
    if (m > tab[s].max) tab[s].max = m;
    if (!abs_le(x, tab[s].figure) && failures < 20) printf("FAIL: |value| / r = %.4Lf above the figure %.1f at '%s'   [%s]\n", m, tab[s].figure, tab[s].name, g_ctx);
    if (!abs_le(x, tab[s].figure)) failures++;
    return x;
}

struct PermRow {  // what one row of evalh_perm_kernel reads
    uint32_t n_sets, n_cols, chunk_len;
    std::vector<Fe> z, z_next, z_last;  // per set: z_s(X), z_s(wX), z_s(w^last X)
    std::vector<Fe> cols, cosets;       // per permuted column
    Fe l0, l_last, l_active, value, beta, gamma, y, delta, delta_start, pow_lo, pow_hi;
    bool use_hi;
};

// evalh_perm_kernel's row body, statement for statement
static Fe perm_row(const PermRow& p) {
    const Fu beta = to_i(p.beta), gamma = to_i(p.gamma), y = to_i(p.y), delta = to_i(p.delta);
    const Fu one = fu_one_i<UF>();
    Fu v = B(g_perm, PV, ld_i(p.value));
    v = B(g_perm, PF0, FOLD(v, y, B(g_perm, P1Z, subn(one, ld_i(p.z[0]))), ld_i(p.l0)));
    {
        const Fu zl = ld_i(p.z[p.n_sets - 1]);
        v = B(g_perm, PFL, FOLD(v, y, B(g_perm, PZZ, subn(SQR(zl), zl)), ld_i(p.l_last)));
    }
    for (uint32_t s = 1; s < p.n_sets; s++) v = B(g_perm, PFZ, FOLD(v, y, B(g_perm, PZD, subn(ld_i(p.z[s]), ld_i(p.z_last[s - 1]))), ld_i(p.l0)));
    Fu current_delta = to_i(p.delta_start);
    current_delta = B(g_perm, PCD, MUL(current_delta, to_i(p.pow_lo)));
    if (p.use_hi) current_delta = B(g_perm, PCD, MUL(current_delta, to_i(p.pow_hi)));
    for (uint32_t s = 0; s < p.n_sets; s++) {
        const uint32_t j0 = s * p.chunk_len, j1 = j0 + p.chunk_len < p.n_cols ? j0 + p.chunk_len : p.n_cols;
        Fu left = B(g_perm, PLR, ld_i(p.z_next[s])), right = B(g_perm, PLR, ld_i(p.z[s]));
        Fu diff = subn(left, right);
        for (uint32_t j = j0; j < j1; j++) {
            const Fu cg = fu_add(ld_i(p.cols[j]), gamma);
            for (int i = 0; i < 9; i++) CHECK(cg.l[i] >= 0 && cg.l[i] < (1 << 30));  // "limbs below 2^30 (not normalised)"
            operand(beta);
            const Fu sj = ld_i(p.cosets[j]);
            operand(sj);
            const Fu lterm = B(g_perm, PLT, fu_mul_subh<UF>(beta, sj, fu_neg(cg)));
            const Fu rterm = B(g_perm, PRT, addn(cg, current_delta));
            current_delta = B(g_perm, PCDD, MUL(current_delta, delta));
            if (j + 1 == j1) {
                diff = B(g_perm, j == j0 ? PD1 : PDN, MULSUB(left, lterm, right, rterm, false));
                break;
            }
            left = B(g_perm, PL, MUL(left, lterm));
            right = B(g_perm, PR, MUL(right, rterm));
        }
        v = B(g_perm, PFA, FOLD(v, y, diff, ld_i(p.l_active)));
    }
    B(g_perm, PST, v);
    return OUT(v);
}

// the same row on canonical elements (evaluation.rs:362-441)
static Fe perm_row_ref(const PermRow& p) {
    const Fe one = fe_one<P>();
    Fe v = p.value;
    v = fe_add<P>(fe_mul<P>(v, p.y), fe_mul<P>(fe_sub<P>(one, p.z[0]), p.l0));
    const Fe zl = p.z[p.n_sets - 1];
    v = fe_add<P>(fe_mul<P>(v, p.y), fe_mul<P>(fe_sub<P>(fe_mul<P>(zl, zl), zl), p.l_last));
    for (uint32_t s = 1; s < p.n_sets; s++) v = fe_add<P>(fe_mul<P>(v, p.y), fe_mul<P>(fe_sub<P>(p.z[s], p.z_last[s - 1]), p.l0));
    Fe cd = fe_mul<P>(p.delta_start, p.pow_lo);
    if (p.use_hi) cd = fe_mul<P>(cd, p.pow_hi);
    for (uint32_t s = 0; s < p.n_sets; s++) {
        const uint32_t j0 = s * p.chunk_len, j1 = j0 + p.chunk_len < p.n_cols ? j0 + p.chunk_len : p.n_cols;
        Fe left = p.z_next[s], right = p.z[s];
        for (uint32_t j = j0; j < j1; j++) {
            left = fe_mul<P>(left, fe_add<P>(fe_add<P>(p.cols[j], fe_mul<P>(p.beta, p.cosets[j])), p.gamma));
            right = fe_mul<P>(right, fe_add<P>(fe_add<P>(p.cols[j], cd), p.gamma));
            cd = fe_mul<P>(cd, p.delta);
        }
        v = fe_add<P>(fe_mul<P>(v, p.y), fe_mul<P>(fe_sub<P>(left, right), p.l_active));
    }
    return v;
}

struct LookRow {  // columns of four rows, the row under test is 1: its neighbours are rows 2 (wX) and 0 (w^-1 X)
    Fe product[4], pin[4], ptab[4], l0[4], l_last[4], l_active[4], values[4];
    Fe table_value, beta, gamma, y;
};

// lookup_row's body, statement for statement
static Fe look_row(const LookRow& l) {
    const uint32_t idx = 1, r_next = 2, r_prev = 0;
    const Fu beta = to_i(l.beta), gamma = to_i(l.gamma), y = to_i(l.y), table_value = ld_i(l.table_value);
    const Fu one = fu_one_i<UF>();
    const Fu z = B(g_look, LLD, ld_i(l.product[idx])), a_ = B(g_look, LLD, ld_i(l.pin[idx])), s_ = B(g_look, LLD, ld_i(l.ptab[idx]));
    const Fu l0 = B(g_look, LLD, ld_i(l.l0[idx])), l_active = B(g_look, LLD, ld_i(l.l_active[idx]));
    const Fu a_minus_s = B(g_look, LAS, subn(a_, s_));
    Fu v = B(g_look, LLD, ld_i(l.values[idx]));
    v = B(g_look, LF0, FOLD(v, y, subn(one, z), l0));
    v = B(g_look, LFL, FOLD(v, y, subn(SQR(z), z), ld_i(l.l_last[idx])));
    {
        const Fu zab = B(g_look, LZAB, MUL(ld_i(l.product[r_next]), addn(a_, beta)));
        const Fu diff = B(g_look, LDIFF, MULSUB(zab, addn(s_, gamma), z, table_value, false));
        v = B(g_look, LFD, FOLD(v, y, diff, l_active));
    }
    v = B(g_look, LFAS, FOLD(v, y, a_minus_s, l0));
    v = B(g_look, LFA, FOLD(v, y, B(g_look, LMUL, MUL(a_minus_s, subn(a_, ld_i(l.pin[r_prev])))), l_active));
    return OUT(v);
}

static Fe look_row_ref(const LookRow& l) {  // evaluation.rs:443-518
    const Fe one = fe_one<P>();
    const Fe z = l.product[1], a_ = l.pin[1], s_ = l.ptab[1], ams = fe_sub<P>(a_, s_);
    Fe v = l.values[1];
    v = fe_add<P>(fe_mul<P>(v, l.y), fe_mul<P>(fe_sub<P>(one, z), l.l0[1]));
    v = fe_add<P>(fe_mul<P>(v, l.y), fe_mul<P>(fe_sub<P>(fe_mul<P>(z, z), z), l.l_last[1]));
    const Fe lhs = fe_mul<P>(fe_mul<P>(l.product[2], fe_add<P>(a_, l.beta)), fe_add<P>(s_, l.gamma));
    v = fe_add<P>(fe_mul<P>(v, l.y), fe_mul<P>(fe_sub<P>(lhs, fe_mul<P>(z, l.table_value)), l.l_active[1]));
    v = fe_add<P>(fe_mul<P>(v, l.y), fe_mul<P>(ams, l.l0[1]));
    v = fe_add<P>(fe_mul<P>(v, l.y), fe_mul<P>(fe_mul<P>(ams, fe_sub<P>(a_, l.pin[0])), l.l_active[1]));
    return v;
}

static std::vector<Fe> g_values;  // the stored words of the corpus (tests/evalh_edge_util.py VALUES)
static Fe word(int mode) {        // 0: r - 1, 1: zero, 2: drawn from the values, 3: uniform below r
    if (mode == 0) return g_values[2];
    if (mode == 1) return fe_zero<P>();
    if (mode == 2) return g_values[rnd() % g_values.size()];
    Fe x;
    for (int i = 0; i < 8; i++) x.l[i] = (uint32_t)rnd();
    x.l[7] &= 0x1fffffffu;  // below 2^253 < r
    return x;
}

static uint64_t g_perm_rows = 0, g_look_rows = 0, g_satisfied = 0;

static void perm_rows() {
    struct Layout { uint32_t n_sets, n_cols, chunk_len; };
    // chunk_len 1, 2, 3; one and three sets; a ragged last set (3 sets of 2 over 5 columns, 3 of 3 over 7) and full ones
    const Layout layouts[] = {{1, 1, 1}, {3, 3, 1}, {1, 2, 2}, {3, 5, 2}, {3, 6, 2}, {1, 3, 3}, {3, 7, 3}, {3, 9, 3}, {1, 2, 3}};
    for (const Layout& L : layouts)
        for (int mode = 0; mode < 5; mode++) {  // 4: a satisfied row over extreme operands
            const int trials = (mode < 2) ? 1 : 400;
            for (int t = 0; t < trials; t++) {
                const int m = mode == 4 ? 2 : mode;
                PermRow p;
                p.n_sets = L.n_sets;
                p.n_cols = L.n_cols;
                p.chunk_len = L.chunk_len;
                for (uint32_t s = 0; s < L.n_sets; s++) {
                    p.z.push_back(word(m));
                    p.z_next.push_back(word(m));
                    p.z_last.push_back(word(m));
                }
                for (uint32_t j = 0; j < L.n_cols; j++) {
                    p.cols.push_back(word(m));
                    p.cosets.push_back(word(m));
                }
                p.l0 = word(m);
                p.l_last = word(m);
                p.l_active = word(m);
                p.value = word(m);
                p.beta = word(m);
                p.gamma = word(m);
                p.y = word(m);
                p.delta = word(m);
                p.delta_start = word(m);
                p.pow_lo = word(m);
                p.pow_hi = word(m);
                p.use_hi = (t & 1) != 0;
                snprintf(g_ctx, sizeof(g_ctx), "perm row: %u sets, %u columns, chunk_len %u, mode %d, trial %d", L.n_sets, L.n_cols, L.chunk_len, mode, t);
                if (mode == 4) {
                    // l_0 = l_last = 0 on this row and every set's z(wX) = z(X) right / left: every constraint holds and the row is value y^k
                    p.l0 = p.l_last = fe_zero<P>();
                    Fe cd = fe_mul<P>(p.delta_start, p.pow_lo);
                    if (p.use_hi) cd = fe_mul<P>(cd, p.pow_hi);
                    bool ok = true;
                    for (uint32_t s = 0; s < L.n_sets; s++) {
                        const uint32_t j0 = s * L.chunk_len, j1 = j0 + L.chunk_len < L.n_cols ? j0 + L.chunk_len : L.n_cols;
                        Fe left = fe_one<P>(), right = fe_one<P>();
                        for (uint32_t j = j0; j < j1; j++) {
                            left = fe_mul<P>(left, fe_add<P>(fe_add<P>(p.cols[j], fe_mul<P>(p.beta, p.cosets[j])), p.gamma));
                            right = fe_mul<P>(right, fe_add<P>(fe_add<P>(p.cols[j], cd), p.gamma));
                            cd = fe_mul<P>(cd, p.delta);
                        }
                        if (fe_is_zero(left)) ok = false;
                        else p.z_next[s] = fe_mul<P>(fe_mul<P>(p.z[s], right), fe_inv<P>(left));
                    }
                    if (!ok) continue;
                    Fe want = p.value;
                    for (uint32_t k = 0; k < 2 * L.n_sets + 1; k++) want = fe_mul<P>(want, p.y);
                    CHECK(fe_eq(perm_row_ref(p), want));
                    g_satisfied++;
                }
                const Fe got = perm_row(p);
                CHECK(fe_eq(got, perm_row_ref(p)));
                g_perm_rows++;
            }
        }
}

static void look_rows() {
    ColsDev c;
    memset(&c, 0, sizeof(c));
    c.log_size = 2;
    c.rot_scale = 1;
    for (int mode = 0; mode < 5; mode++) {
        const int trials = (mode < 2) ? 1 : 3000;
        for (int t = 0; t < trials; t++) {
            const int m = mode == 4 ? 2 : mode;
            LookRow l;
            for (int i = 0; i < 4; i++) {
                l.product[i] = word(m);
                l.pin[i] = word(m);
                l.ptab[i] = word(m);
                l.l0[i] = word(m);
                l.l_last[i] = word(m);
                l.l_active[i] = word(m);
                l.values[i] = word(m);
            }
            l.table_value = word(m);
            l.beta = word(m);
            l.gamma = word(m);
            l.y = word(m);
            snprintf(g_ctx, sizeof(g_ctx), "lookup row: mode %d, trial %d", mode, t);
            if (mode == 4) {
                // l_0 = l_last = 0, a' = s' and z(wX) = z table_value / ((a' + beta)(s' + gamma)): the row is value y^5
                l.l0[1] = l.l_last[1] = fe_zero<P>();
                l.ptab[1] = l.pin[1];
                const Fe den = fe_mul<P>(fe_add<P>(l.pin[1], l.beta), fe_add<P>(l.ptab[1], l.gamma));
                if (fe_is_zero(den)) continue;
                l.product[2] = fe_mul<P>(fe_mul<P>(l.product[1], l.table_value), fe_inv<P>(den));
                Fe want = l.values[1];
                for (int k = 0; k < 5; k++) want = fe_mul<P>(want, l.y);
                CHECK(fe_eq(look_row_ref(l), want));
                g_satisfied++;
            }
            const Fe want = look_row_ref(l);
            CHECK(fe_eq(look_row(l), want));
            // the header's own lookup_row on the same row (its H2_FU_ASSERTs live): the element the restatement stores
            LookupDev d = {l.product, l.pin, l.ptab, l.l0, l.l_last, l.l_active};
            c.beta = to_i(l.beta);
            c.gamma = to_i(l.gamma);
            c.y = to_i(l.y);
            Fe vals[4];
            memcpy(vals, l.values, sizeof(vals));
            lookup_row(d, c, 1, ld_i(l.table_value), vals);
            CHECK(fe_eq(vals[1], want) && fe_is_canonical<P>(vals[1]));
            for (int i = 0; i < 4; i++)
                if (i != 1) CHECK(fe_eq(vals[i], l.values[i]));
            g_look_rows++;
        }
    }
}

int main(int argc, char** argv) {
    signal(SIGABRT, on_abort);
    if (argc < 2) {
        printf("usage: test_evalh_bounds corpus.bin\n");
        return 2;
    }
    Reader r;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 2;
        }
        fseek(f, 0, SEEK_END);
        r.buf.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
        fclose(f);
    }
    if (r.u32() != 0x48564245u) {
        printf("not a corpus file\n");
        return 2;
    }
    const uint32_t n_records = r.u32(), n_values = r.u32();
    r.vec(g_values, n_values);
    for (const Fe& v : g_values) CHECK(fe_is_canonical<P>(v));
    CHECK(n_values >= 3);
    {   // the saturated operand the corpus adds: limbs 0..7 of fu_from_ext at their maximum
        bool saturated = false;
        for (const Fe& v : g_values) {
            const Fu u = ld_i(v);
            bool all = u.l[0] == (int32_t)(H2_MASK29 & ~31u);
            for (int i = 1; i < 8; i++) all = all && u.l[i] == (int32_t)H2_MASK29;
            saturated = saturated || all;
        }
        CHECK(saturated);
    }
    Rec R;
    for (uint32_t i = 0; i < n_records; i++) {
        read_rec(r, R);
        run_record(R);
    }
    CHECK(r.at == r.buf.size());
    perm_rows();
    look_rows();

    printf("%u records, %llu rows, %llu values through out_e; %llu perm rows, %llu lookup rows, %llu of them satisfied\n", n_records, (unsigned long long)g_rows,
           (unsigned long long)g_out_e, (unsigned long long)g_perm_rows, (unsigned long long)g_look_rows, (unsigned long long)g_satisfied);
    for (int leg = 0; leg < 2; leg++)
        for (int k = 0; k < 8; k++)
            printf("%s %s: run %llu, with a reduce flag %llu, max |value|/r %.4Lf, max before a reduction %.4Lf\n", leg ? "generated" : "interpreter", OP_NAME[k],
                   (unsigned long long)g_kind[leg][k].run, (unsigned long long)g_kind[leg][k].flagged, g_kind[leg][k].max_out, g_kind[leg][k].max_pre);
    printf("max |value|/r at out_e %.4Lf (negative results: %llu); max before any reduction %.4Lf; least slack under a tracked magnitude %.4Lf; max |top limb| of a product operand %lld\n",
           g_max_result, (unsigned long long)g_negative_results, g_max_pre_reduction, g_min_slack, (long long)g_max_operand_top);
    printf("fused sums %llu, fused Horner steps %llu, closing MOV|REDUCE %llu\n", (unsigned long long)g_fused_sum, (unsigned long long)g_fused_horner,
           (unsigned long long)g_closing_mov);
    for (const Stmt& s : g_perm) printf("statement %-48s figure %5.1f  max |value|/r %.4Lf\n", s.name, s.figure, s.max);
    for (const Stmt& s : g_look) printf("statement %-48s figure %5.1f  max |value|/r %.4Lf\n", s.name, s.figure, s.max);

    // so that nothing above passed vacuously
    snprintf(g_ctx, sizeof(g_ctx), "coverage of the corpus");
    for (int k : {OP_ADD, OP_SUB, OP_DBL, OP_MUL, OP_FMA}) CHECK(g_kind[0][k].flagged > 0);
    CHECK(g_closing_mov > 0);
    CHECK(g_fused_sum > 0 && g_fused_horner > 0);
    CHECK(g_max_pre_reduction > 100.0L);
    CHECK(g_negative_results > 0);
    CHECK(g_perm_rows > 0 && g_look_rows > 0 && g_satisfied > 0);
    for (const Stmt& s : g_perm) CHECK(s.max > 0);
    for (const Stmt& s : g_look) CHECK(s.max > 0);
    if (failures) {
        printf("%d FAILURES\n", failures);
        return 1;
    }
    printf("evalh bounds ok\n");
    return 0;
}
