// evalh.hip -- Evaluator::evaluate_h on the GPU (halo2_proofs/src/plonk/evaluation.rs:280-522).
//
// One lane per row of the extended coset.  Three kernels, in the reference's order, each folding its constraints
// into values[idx] with powers of y exactly as the reference does:
//   evalh_gates_kernel   GraphEvaluator::evaluate of Evaluator::custom_gates (:334-360, :708-749): an interpreter over
//                        the flattened calculations (include/halo2hip.h), intermediates in per-lane scratch
//   evalh_perm_kernel    the permutation argument's constraints (:362-441)
//   evalh_lookup_kernel  one lookup's constraints (:443-518), its compressed-expression graph evaluated in place
// Advice / instance / lookup polynomials arrive in coefficient form and are taken to the extended coset on the
// device with the engine's own coeff_to_extended (ntt.hip), as evaluate_h does at :306-323 and :447-457.
// Arithmetic is the saturated field.h (always canonical): this path is bandwidth- and latency-mixed, not the
// VALU-bound inner loop of the MSM, and canonical values make bit-exactness with the reference immediate.
#include <dlfcn.h>
#include <hip/hiprtc.h>
#include <stdlib.h>
#include <string.h>

#include <stdarg.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/halo2hip.h"
#include "../../include/halo2hip_debug.h"
#include "engine.h"
#include "evalh_dev.h"

namespace h2 {

#define EVALH_VS_ZERO 11  // internal operand kind: the field's zero (an empty graph's value, evaluation.rs:745-749)

// The flattened graph is compiled on the host (compile_graph below) into a short register-machine program before it is
// run: Store calculations become direct column operands, a Horner calculation becomes one FMA per part placed as soon
// as that part exists, dead calculations are dropped and the surviving intermediates are packed into as few slots as
// their lifetimes allow.  A slot is 36 B of LDS (up to 8 slots), per-lane scratch (up to 256) or a row of a global workspace, so a
// circuit with tens of thousands of calculations still runs with a few dozen slots per lane.  The field operations
// performed per row are the reference's, operation for operation; only where a value waits between them differs.
//
// Arithmetic: the unsaturated 9 x 29-bit multiplier of fieldu.h (the MSM's and the NTT's), about half the
// instructions of the saturated CIOS.  Inside a kernel every value is I-form (a * 2^261, lazily reduced): a column
// element (E-form, canonical) becomes I-form for free as the limbs of 32 * x (fu_from_ext), I * I -> I, constants and
// challenges are converted on the host, and the one value a row writes back goes through the exact reduction
// fu_mul_canon(x, 2^256) -> canonical E-form.  So what is stored is the reference's field element, limb for limb.
// Magnitudes (in units of the modulus r) are tracked statically: a loaded column is < 32, a product of magnitudes a, b is
// < a*b/169 + 1, sums add.  For the interpreter the host walks the straight-line program with these rules and marks the
// operations after which a reduction (one multiplication by 2^261) must be inserted to stay below EVALH_MAG_LIMIT; the
// hand-written constraint code below carries its bounds in comments.  Every addition is followed by a carry propagation so
// that limbs 0..7 are back in [0, 2^29) (fu_mul's operand contract).
enum { OP_ADD = 0, OP_SUB, OP_MUL, OP_SQR, OP_DBL, OP_NEG, OP_MOV, OP_FMA /* dst = dst * y + x */, OP_REDUCE_FLAG = 0x100 };
#define EVALH_MAG_LIMIT 100.0   // |value| < 100 r keeps the top limb below 2^28.3
#define EVALH_MAG_RESULT 15.0   // fu_mul_canon needs |value| < 16 r
#define EVALH_MAG_COLUMN 32.0   // fu_from_ext of a canonical element

struct DevOp {
    uint32_t op, dst;
    h2hip_value_source x, y;  // kind INTERMEDIATE: a = slot
};

struct ProgDev {
    const Fu* constants;  // I-form, canonical
    const int32_t* rotations;
    const DevOp* ops;
    uint32_t n_ops;
    h2hip_value_source result;
};

__device__ __forceinline__ DevOp ld_op(const DevOp* ops, uint32_t q) {
    const H2_CONST_AS u32x8* p = (const H2_CONST_AS u32x8*)(uintptr_t)ops;
    const u32x8 w = p[q];
    DevOp o;
    o.op = w[0];
    o.dst = w[1];
    o.x.kind = w[2];
    o.x.a = w[3];
    o.x.b = w[4];
    o.y.kind = w[5];
    o.y.a = w[6];
    o.y.b = w[7];
    return o;
}
// slot storage: MAXI > 0 -> per-lane scratch; MAXI == 0 -> a global workspace laid out [slot][lane] (coalesced per slot)
extern __shared__ int32_t evalh_lds[];
#define EVALH_LDS_HOT 4  // slots of a scratch-tier program that live in LDS (measured, 100 / 400 gates at 2^20 rows: 2 -> 13.1 / 38.7 ms,
                         // 3 -> 11.9 / 38.3, 4 -> 11.5 / 36.3, 8 -> 12.2 / 40.7; all scratch: 14.6 / 45.4)
__device__ __forceinline__ Fu lds_slot_get(uint32_t i) {
    Fu r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.l[k] = evalh_lds[(i * 9 + k) * 256 + threadIdx.x];
    return r;
}
__device__ __forceinline__ void lds_slot_set(uint32_t i, const Fu& x) {
#pragma unroll
    for (int k = 0; k < 9; k++) evalh_lds[(i * 9 + k) * 256 + threadIdx.x] = x.l[k];
}
// 16 / 64 / 256 slots: the first EVALH_LDS_HOT in LDS, the rest in per-lane scratch; compile_graph numbers the slots by
// how often the program touches them, busiest first.
template <int MAXI>
struct Slots {
    Fu v[MAXI - EVALH_LDS_HOT];
    __device__ __forceinline__ Slots(Fu*, size_t) {}
    __device__ __forceinline__ Fu get(uint32_t i) const { return i < EVALH_LDS_HOT ? lds_slot_get(i) : v[i - EVALH_LDS_HOT]; }
    __device__ __forceinline__ void set(uint32_t i, const Fu& x) {
        if (i < EVALH_LDS_HOT) lds_slot_set(i, x);
        else v[i - EVALH_LDS_HOT] = x;
    }
};
// few slots (the common case: a gate polynomial is folded as soon as it exists): LDS, laid out [slot][limb][thread] so
// that a wave's access is one conflict-free row.  (Registers would be better still, but the slot index is only known at
// run time and LLVM turns any select chain over would-be register slots back into an indexed scratch access.)
template <int N>
struct LdsSlots {
    __device__ __forceinline__ LdsSlots(Fu*, size_t) {}
    __device__ __forceinline__ Fu get(uint32_t i) const { return lds_slot_get(i); }
    __device__ __forceinline__ void set(uint32_t i, const Fu& x) { lds_slot_set(i, x); }
};
template <>
struct Slots<4> : LdsSlots<4> {
    __device__ __forceinline__ Slots(Fu* b, size_t s) : LdsSlots<4>(b, s) {}
};
template <>
struct Slots<8> : LdsSlots<8> {
    __device__ __forceinline__ Slots(Fu* b, size_t s) : LdsSlots<8>(b, s) {}
};
template <>
struct Slots<0> {
    Fu* base;
    size_t stride;
    __device__ __forceinline__ Slots(Fu* b, size_t s) : base(b), stride(s) {}
    __device__ __forceinline__ Fu get(uint32_t i) const { return base[i * stride]; }
    __device__ __forceinline__ void set(uint32_t i, const Fu& x) { base[i * stride] = x; }
};

// ValueSource::get (evaluation.rs:68-103)
template <class S>
__device__ __forceinline__ Fu vs_get(const ProgDev& g, const ColsDev& c, const h2hip_value_source& v, uint32_t idx, const S& slots,
                                     const Fu& previous) {
    switch (v.kind) {
        case H2HIP_VS_CONSTANT: return ld_const_fu(g.constants, v.a);
        case H2HIP_VS_INTERMEDIATE: return slots.get(v.a);
        case H2HIP_VS_FIXED: return ld_i(ld_const_col(c.fixed, v.a)[rot_idx(idx, ld_const_i32(g.rotations, v.b), c.rot_scale, c.log_size)]);
        case H2HIP_VS_ADVICE: return ld_i(ld_const_col(c.advice, v.a)[rot_idx(idx, ld_const_i32(g.rotations, v.b), c.rot_scale, c.log_size)]);
        case H2HIP_VS_INSTANCE: return ld_i(ld_const_col(c.instance, v.a)[rot_idx(idx, ld_const_i32(g.rotations, v.b), c.rot_scale, c.log_size)]);
        case H2HIP_VS_CHALLENGE: return ld_const_fu(c.challenges, v.a);
        case H2HIP_VS_BETA: return c.beta;
        case H2HIP_VS_GAMMA: return c.gamma;
        case H2HIP_VS_THETA: return c.theta;
        case H2HIP_VS_Y: return c.y;
        case H2HIP_VS_PREVIOUS: return previous;
        default: return fu_zero();
    }
}

// GraphEvaluator::evaluate (evaluation.rs:708-749) with Calculation::evaluate (:129-178), over the compiled program.
// Returns the I-form result; the host guarantees its magnitude is below EVALH_MAG_RESULT when it is a slot (a column or a
// constant can also be the result of a degenerate graph: < 32).
template <class S>
__device__ __forceinline__ Fu prog_eval(const ProgDev& g, const ColsDev& c, uint32_t idx, const Fu& previous, S& slots) {
    for (uint32_t q = 0; q < g.n_ops; q++) {
        const DevOp o = ld_op(g.ops, q);
        const Fu a = vs_get(g, c, o.x, idx, slots, previous);
        Fu out;
        switch (o.op & 0xff) {
            case OP_ADD: out = addn(a, vs_get(g, c, o.y, idx, slots, previous)); break;
            case OP_SUB: out = subn(a, vs_get(g, c, o.y, idx, slots, previous)); break;
            case OP_MUL: out = mul_i(a, vs_get(g, c, o.y, idx, slots, previous)); break;
            case OP_SQR: out = fu_sqr<UF>(a); break;
            case OP_DBL: out = fu_norm(fu_dbl(a)); break;
            case OP_NEG: out = fu_norm(fu_neg(a)); break;
            case OP_FMA: out = addn(mul_i(slots.get(o.dst), vs_get(g, c, o.y, idx, slots, previous)), a); break;
            default: out = a;  // OP_MOV
        }
        if (o.op & OP_REDUCE_FLAG) out = mul_i(out, fu_one_i<UF>());
        slots.set(o.dst, out);
    }
    return vs_get(g, c, g.result, idx, slots, previous);
}

// the value a row stores: a column / PreviousValue result is already the canonical element
template <class S>
__device__ __forceinline__ Fe prog_result_e(const ProgDev& g, const ColsDev& c, uint32_t idx, const Fe& previous_e, const Fu& r) {
    switch (g.result.kind) {
        case H2HIP_VS_FIXED: return ld_const_col(c.fixed, g.result.a)[rot_idx(idx, ld_const_i32(g.rotations, g.result.b), c.rot_scale, c.log_size)];
        case H2HIP_VS_ADVICE: return ld_const_col(c.advice, g.result.a)[rot_idx(idx, ld_const_i32(g.rotations, g.result.b), c.rot_scale, c.log_size)];
        case H2HIP_VS_INSTANCE: return ld_const_col(c.instance, g.result.a)[rot_idx(idx, ld_const_i32(g.rotations, g.result.b), c.rot_scale, c.log_size)];
        case H2HIP_VS_PREVIOUS: return previous_e;
        case EVALH_VS_ZERO: return fe_zero<FrP>();
        default: return out_e(r);
    }
}

// lanes = threads in the grid; rows beyond it are taken grid-stride (only the global-workspace form launches fewer lanes than rows)
template <int MAXI>
__global__ void __launch_bounds__(256) evalh_gates_kernel(ProgDev g, ColsDev c, Fe* values, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        const Fe prev = values[idx];
        const Fu r = prog_eval(g, c, idx, ld_i(prev), slots);
        values[idx] = prog_result_e<Slots<MAXI>>(g, c, idx, prev, r);
    }
}

struct PermDev {
    const Fe* const* z;       // permutation_product_coset per set
    const Fe* const* cols;    // the permuted columns' extended cosets, already resolved by (kind, index)
    const Fe* const* cosets;  // pk.permutation.cosets
    const Fe *l0, *l_last, *l_active;
    Fu delta, delta_start;    // I-form canonical; delta_start = beta * ZETA (:368)
    const Fu *pow_lo, *pow_hi;  // the extended domain's two-level power table (the NTT's: omega^i, i < 2^pow_bits; omega^(i << pow_bits)), I-form canonical
    uint32_t pow_bits;
    uint32_t n_sets, n_cols, chunk_len;
    int32_t last_rotation;
};

// Magnitudes in units of r are given in brackets.
__global__ void __launch_bounds__(256) evalh_perm_kernel(PermDev p, ColsDev c, Fe* values) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (1u << c.log_size)) return;
    const Fu one = fu_one_i<UF>();
    const uint32_t r_next = rot_idx(idx, 1, c.rot_scale, c.log_size);
    const uint32_t r_last = rot_idx(idx, p.last_rotation, c.rot_scale, c.log_size);
    Fu v = ld_i(values[idx]);  // [32]
    // l_0(X) * (1 - z_0(X)) = 0                                                   :382-386
    v = fold_y(v, c.y, subn(one, ld_i(ld_const_col(p.z, 0)[idx])), ld_i(p.l0[idx]));  // [1.2] + [33 * 32 / 169 + 1 = 7.3] = [8.5]
    // l_last(X) * (z_l(X)^2 - z_l(X)) = 0                                         :387-393
    {
        const Fu zl = ld_i(ld_const_col(p.z, p.n_sets - 1)[idx]);                                          // [32]
        v = fold_y(v, c.y, subn(fu_sqr<UF>(zl), zl), ld_i(p.l_last[idx]));                  // [1.1] + [(7.1 + 32) * 32 / 169 + 1 = 8.4] = [9.5]
    }
    // l_0(X) * (z_i(X) - z_{i-1}(omega^(last) X)) = 0                              :394-404
    for (uint32_t s = 1; s < p.n_sets; s++)
        v = fold_y(v, c.y, subn(ld_i(ld_const_col(p.z, s)[idx]), ld_i(ld_const_col(p.z, s - 1)[r_last])), ld_i(p.l0[idx]));  // [1.1] + [64 * 32 / 169 + 1 = 13.2] = [14.3]
    // (1 - (l_last + l_blind)) * (z_i(wX) prod(p + beta s_j + gamma) - z_i(X) prod(p + delta^j beta X + gamma))   :405-438
    Fu current_delta = p.delta_start;  // beta * ZETA * extended_omega^idx (beta_term, :366-368 and :412)   [1 .. 2]
    current_delta = mul_i(current_delta, p.pow_lo[idx & ((1u << p.pow_bits) - 1)]);
    if (idx >> p.pow_bits) current_delta = mul_i(current_delta, p.pow_hi[idx >> p.pow_bits]);  // uniform over a workgroup
    for (uint32_t s = 0; s < p.n_sets; s++) {
        const uint32_t j0 = s * p.chunk_len, j1 = j0 + p.chunk_len < p.n_cols ? j0 + p.chunk_len : p.n_cols;
        const Fe* zs = ld_const_col(p.z, s);
        Fu left = ld_i(zs[r_next]), right = ld_i(zs[idx]);  // [32]
        Fu diff = subn(left, right);  // (a set without columns)
        for (uint32_t j = j0; j < j1; j++) {  // both products in one walk over the set's columns: a column's value is read once
            const Fu cg = fu_add(ld_i(ld_const_col(p.cols, j)[idx]), c.gamma);                                // column + gamma, limbs below 2^30 (not normalised)
            const Fu lterm = fu_mul_subh<UF>(c.beta, ld_i(ld_const_col(p.cosets, j)[idx]), fu_neg(cg));        // beta * s_j + (column + gamma) in one pass   [32 + 1.2 + 1 = 34.2]
            const Fu rterm = addn(cg, current_delta);                                                          // [35]
            current_delta = mul_i(current_delta, p.delta);                                                     // [1.1]
            if (j + 1 == j1) {
                // the last column's two products leave as their difference, one reduction for both: [(32 * 34.2 + 32 * 35) / 169 + 1 = 14.1] for a set of
                // one column, [(7.5 * 34.2 + 7.7 * 35) / 169 + 1 = 4.1] otherwise
                diff = fu_mul_sub<UF>(left, lterm, right, rterm);
                break;
            }
            left = mul_i(left, lterm);                                                                         // [32 * 34.2 / 169 + 1 = 7.5], then smaller
            right = mul_i(right, rterm);                                                                       // [7.7]
        }
        v = fold_y(v, c.y, diff, ld_i(p.l_active[idx]));                              // [1.1] + [14.1 * 32 / 169 + 1 = 3.7] = [4.8]
    }
    values[idx] = out_e(v);  // [< 15]
}

template <int MAXI>
__global__ void __launch_bounds__(256) evalh_lookup_kernel(ProgDev g, LookupDev l, ColsDev c, Fe* values, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        const Fu table_value = prog_eval(g, c, idx, fu_zero(), slots);  // :466-480   [< 32]
        lookup_row(l, c, idx, table_value, values);
    }
}

// One shuffle argument's share of a row: ga and gs are the input and the shuffle side's programs, a = A + gamma and s = S + gamma their
// values; both run on one Slots object, which the host sizes for the larger plan of the two, and a is held in registers while gs runs.
// The three terms are shuffle_row's (evalh_dev.h), which the kernel generated per argument ends with too.
template <int MAXI>
__global__ void __launch_bounds__(256) evalh_shuffle_kernel(ProgDev ga, ProgDev gs, ShuffleDev sh, ColsDev c, Fe* values, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        const Fu a = prog_eval(ga, c, idx, fu_zero(), slots);  // [< 15 a slot, < 32 a column or a constant]
        const Fu s = prog_eval(gs, c, idx, fu_zero(), slots);  // [< 32]
        shuffle_row(sh, c, idx, a, s, values);
    }
}

// One logUp (mv-lookup) argument's share of a row.  progs holds the argument's K input programs, then its table program; each value is
// (theta fold) + beta.  The programs run in turn on one Slots object, which the host sizes for the largest plan among them, and between
// two of them only P = prod f_c, Q = sum_c prod_{l != c} f_l (streamed as Q <- Q f + P; P <- P f: no inversion on the coset) stay in
// registers; the table program runs last, so tau is never held across one.  The three terms are mvlookup_row's (evalh_dev.h).
// Magnitudes in units of r in brackets: P_0 = 1, P <- P f [P 32 / 169 + 1 <= 1.3]; Q_0 = 0, Q <- Q f + P [Q 32 / 169 + 1 + 1.3 <= 2.9].
template <int MAXI>
__global__ void __launch_bounds__(256) evalh_mvlookup_kernel(const ProgDev* __restrict__ progs, uint32_t n_inputs, MvLookupDev mv, ColsDev c,
                                                             Fe* values, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        Fu P = fu_one_i<UF>(), Q = fu_zero();
        for (uint32_t t = 0; t < n_inputs; t++) {
            const Fu f = prog_eval(progs[t], c, idx, fu_zero(), slots);  // [< 32]
            Q = addn(mul_i(Q, f), P);                                    // [<= 2.9]
            P = mul_i(P, f);                                             // [<= 1.3]
        }
        const Fu tau = prog_eval(progs[n_inputs], c, idx, fu_zero(), slots);  // [< 32]
        mvlookup_row(mv, c, idx, tau, P, Q, values);
    }
}

// ---------------------------------------------------------------------------------------------- host side

// E-form canonical element -> I-form canonical limbs (x * 2^5 mod r, sliced): how constants, challenges and the
// y / beta / gamma / theta scalars enter the kernels
static inline Fu to_i(const Fe& x) {
    Fe t = x;
    for (int k = 0; k < 5; k++) t = fe_dbl<FrP>(t);
    return fu_slice(t);
}

static bool vs_ok(const h2hip_value_source& v, const h2hip_graph& g, const h2hip_evalh_desc& d) {
    switch (v.kind) {
        case H2HIP_VS_CONSTANT: return v.a < g.n_constants;
        case H2HIP_VS_INTERMEDIATE: return v.a < g.num_intermediates;
        case H2HIP_VS_FIXED: return v.a < d.n_fixed && v.b < g.n_rotations;
        case H2HIP_VS_ADVICE: return v.a < d.n_advice && v.b < g.n_rotations;
        case H2HIP_VS_INSTANCE: return v.a < d.n_instance && v.b < g.n_rotations;
        case H2HIP_VS_CHALLENGE: return v.a < d.n_challenges;
        case H2HIP_VS_BETA: case H2HIP_VS_GAMMA: case H2HIP_VS_THETA: case H2HIP_VS_Y: case H2HIP_VS_PREVIOUS: return true;
        default: return false;
    }
}

// Every index a kernel will dereference is checked here: a malformed graph must be an error, never a GPU fault.  The
// graph must also be in the single-assignment form GraphEvaluator builds (add_calculation, evaluation.rs:570-588:
// every calculation writes a fresh intermediate, operands refer to earlier ones) -- compile_graph relies on it.
static int graph_validate(const h2hip_graph& g, const h2hip_evalh_desc& d, const char* what) {
    if ((g.n_constants && !g.constants) || (g.n_rotations && !g.rotations) || (g.n_calculations && !g.calculations) || (g.n_parts && !g.parts)) {
        set_error("evaluate_h: %s graph has null arrays", what);
        return 1;
    }
    if (g.num_intermediates > (1u << 24) || g.n_calculations > (1u << 24)) {
        set_error("evaluate_h: %s graph too large (%u calculations)", what, g.n_calculations);
        return 1;
    }
    std::vector<uint8_t> defined(g.num_intermediates, 0);
    auto ok_src = [&](const h2hip_value_source& v) { return vs_ok(v, g, d) && (v.kind != H2HIP_VS_INTERMEDIATE || defined[v.a]); };
    for (uint32_t q = 0; q < g.n_calculations; q++) {
        const h2hip_calculation& c = g.calculations[q];
        bool ok = c.op <= H2HIP_CALC_STORE && c.target < g.num_intermediates && !defined[c.target] && ok_src(c.x);
        if (c.op == H2HIP_CALC_ADD || c.op == H2HIP_CALC_SUB || c.op == H2HIP_CALC_MUL || c.op == H2HIP_CALC_HORNER) ok = ok && ok_src(c.y);
        if (c.op == H2HIP_CALC_HORNER) {
            ok = ok && (uint64_t)c.parts_offset + c.parts_count <= g.n_parts;
            for (uint32_t t = 0; ok && t < c.parts_count; t++) ok = ok_src(g.parts[c.parts_offset + t]);
        }
        if (!ok) {
            set_error("evaluate_h: %s graph, calculation %u is malformed (bad index, or not in single-assignment order)", what, q);
            return 1;
        }
        defined[c.target] = 1;
    }
    return 0;
}

// ---- graph -> program (see the comment at DevOp).  Assumes graph_validate passed.
struct Program {
    std::vector<DevOp> ops;
    std::vector<double> mags;  // per op: the tracked magnitude of its result in units of r (step 4 of compile_graph)
    uint32_t n_slots = 0;
    h2hip_value_source result = {EVALH_VS_ZERO, 0, 0};
};

static Program compile_graph(const h2hip_graph& g) {
    const uint32_t n = g.n_calculations;
    const h2hip_value_source none = {EVALH_VS_ZERO, 0, 0};
    Program P;
    if (n == 0) return P;
    std::vector<uint32_t> def_of(g.num_intermediates, 0);
    for (uint32_t q = 0; q < n; q++) def_of[g.calculations[q].target] = q;
    // a Store is not materialised: whoever reads its target reads its source (ValueSource::get is a pure load)
    auto resolve = [&](h2hip_value_source v) {
        while (v.kind == H2HIP_VS_INTERMEDIATE && g.calculations[def_of[v.a]].op == H2HIP_CALC_STORE) v = g.calculations[def_of[v.a]].x;
        return v;
    };
    // 1. emission order; Horner steps are hoisted to the earliest point their part exists.  The value is unchanged:
    //    ((x*y + p0)*y + p1)... is the same field element whenever each step is executed.
    struct Hoist { uint32_t q, next; bool started; };
    std::vector<Hoist> hs;
    for (uint32_t q = 0; q < n; q++)
        if (g.calculations[q].op == H2HIP_CALC_HORNER) hs.push_back({q, 0, false});
    std::vector<DevOp> ops;
    ops.reserve(n + 16);
    auto avail = [&](const h2hip_value_source& v, uint32_t q) { return v.kind != H2HIP_VS_INTERMEDIATE || def_of[v.a] <= q; };
    auto advance = [&](Hoist& h, uint32_t q) {
        const h2hip_calculation& c = g.calculations[h.q];
        const h2hip_value_source x = resolve(c.x), y = resolve(c.y);
        if (!h.started) {
            if (!avail(x, q) || !avail(y, q)) return;
            ops.push_back({OP_MOV, c.target, x, none});
            h.started = true;
        }
        while (h.next < c.parts_count) {
            const h2hip_value_source p = resolve(g.parts[c.parts_offset + h.next]);
            if (!avail(p, q)) break;
            ops.push_back({OP_FMA, c.target, p, y});
            h.next++;
        }
    };
    static const uint32_t op_of[6] = {OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_DBL, OP_NEG};
    size_t h_lo = 0;  // Horners before hs[h_lo] are complete
    for (uint32_t q = 0; q < n; q++) {
        const h2hip_calculation& c = g.calculations[q];
        if (c.op <= H2HIP_CALC_NEGATE) {
            const bool binary = c.op <= H2HIP_CALC_MUL;
            ops.push_back({op_of[c.op], c.target, resolve(c.x), binary ? resolve(c.y) : none});
        }
        while (h_lo < hs.size() && hs[h_lo].q <= q) {
            if (hs[h_lo].q == q) advance(hs[h_lo], q);  // its own position: everything it reads exists, so this completes it
            h_lo++;
        }
        if (c.op != H2HIP_CALC_STORE || q + 1 == n)
            for (size_t i = h_lo; i < hs.size() && i < h_lo + 4; i++) advance(hs[i], q);  // look a few Horners ahead (the reference builds 1-2)
    }
    h2hip_value_source result = resolve({H2HIP_VS_INTERMEDIATE, g.calculations[n - 1].target, 0});
    // 2. drop what nothing reads (walking back, every reader of a value is seen before its definition)
    std::vector<uint8_t> needed(g.num_intermediates, 0);
    if (result.kind == H2HIP_VS_INTERMEDIATE) needed[result.a] = 1;
    std::vector<uint8_t> keep(ops.size(), 0);
    for (size_t i = ops.size(); i-- > 0;) {
        const DevOp& o = ops[i];
        if (!needed[o.dst]) continue;
        keep[i] = 1;
        if (o.x.kind == H2HIP_VS_INTERMEDIATE) needed[o.x.a] = 1;
        if (o.y.kind == H2HIP_VS_INTERMEDIATE) needed[o.y.a] = 1;
    }
    // 3. lifetimes -> slots.  An operand whose last reader is this op gives its slot to the op's result (operands are
    //    read into registers before the result is stored).
    const uint32_t never = 0xffffffffu;
    std::vector<uint32_t> last_use(g.num_intermediates, 0), slot(g.num_intermediates, never);
    {
        uint32_t pos = 0;
        for (size_t i = 0; i < ops.size(); i++) {
            if (!keep[i]) continue;
            const DevOp& o = ops[i];
            if (o.x.kind == H2HIP_VS_INTERMEDIATE) last_use[o.x.a] = pos;
            if (o.y.kind == H2HIP_VS_INTERMEDIATE) last_use[o.y.a] = pos;
            if (o.op == OP_FMA) last_use[o.dst] = pos;
            pos++;
        }
        if (result.kind == H2HIP_VS_INTERMEDIATE) last_use[result.a] = never;
    }
    // 4. magnitudes (see the comment at DevOp): walked with the slots, a reduction is requested wherever a sum would
    //    pass EVALH_MAG_LIMIT, and the result is brought below EVALH_MAG_RESULT for the exact final reduction
    std::vector<double> slot_mag;
    auto mag = [&](const h2hip_value_source& v) -> double {
        switch (v.kind) {
            case H2HIP_VS_INTERMEDIATE: return slot_mag[v.a];
            case H2HIP_VS_FIXED: case H2HIP_VS_ADVICE: case H2HIP_VS_INSTANCE: case H2HIP_VS_PREVIOUS: return EVALH_MAG_COLUMN;
            case EVALH_VS_ZERO: return 0.0;
            default: return 1.0;  // constants, challenges, beta / gamma / theta / y: canonical
        }
    };
    std::vector<uint32_t> free_slots;
    uint32_t pos = 0;
    for (size_t i = 0; i < ops.size(); i++) {
        if (!keep[i]) continue;
        DevOp o = ops[i];
        const bool xi = o.x.kind == H2HIP_VS_INTERMEDIATE, yi = o.y.kind == H2HIP_VS_INTERMEDIATE;
        const uint32_t xv = o.x.a, yv = o.y.a;
        if (xi) o.x.a = slot[xv];
        if (yi) o.y.a = slot[yv];
        const double mx = mag(o.x), my = mag(o.y), md = (o.op == OP_FMA) ? slot_mag[slot[o.dst]] : 0.0;
        if (xi && last_use[xv] == pos) free_slots.push_back(slot[xv]);
        if (yi && last_use[yv] == pos && !(xi && yv == xv)) free_slots.push_back(slot[yv]);
        if (slot[o.dst] == never) {  // a definition (FMA steps reuse the slot their MOV took)
            if (!free_slots.empty()) {
                slot[o.dst] = free_slots.back();
                free_slots.pop_back();
            } else {
                slot[o.dst] = P.n_slots++;
            }
        }
        o.dst = slot[o.dst];
        if (slot_mag.size() < P.n_slots) slot_mag.resize(P.n_slots, 0.0);
        double m;
        switch (o.op) {
            case OP_ADD: case OP_SUB: m = mx + my; break;
            case OP_MUL: m = mx * my / 169.0 + 1.0; break;
            case OP_SQR: m = mx * mx / 169.0 + 1.0; break;
            case OP_DBL: m = 2.0 * mx; break;
            case OP_FMA: m = md * my / 169.0 + 1.0 + mx; break;
            default: m = mx;  // NEG, MOV
        }
        if (m > EVALH_MAG_LIMIT) {
            o.op |= OP_REDUCE_FLAG;
            m = m / 169.0 + 1.0;
        }
        slot_mag[o.dst] = m;
        P.ops.push_back(o);
        P.mags.push_back(m);
        pos++;
    }
    if (result.kind == H2HIP_VS_INTERMEDIATE) {
        result.a = slot[result.a];
        if (slot_mag[result.a] > EVALH_MAG_RESULT) {
            P.ops.push_back({OP_MOV | OP_REDUCE_FLAG, result.a, result, none});
            P.mags.push_back(slot_mag[result.a] / 169.0 + 1.0);
        }
    }
    // 5. renumber the slots by how often the program touches them, busiest first: the kernels keep the lowest-numbered
    //    slots in LDS and the rest in scratch
    {
        std::vector<uint64_t> touches(P.n_slots, 0);
        for (const DevOp& o : P.ops) {
            touches[o.dst] += (o.op & 0xff) == OP_FMA ? 2 : 1;
            if (o.x.kind == H2HIP_VS_INTERMEDIATE) touches[o.x.a]++;
            if (o.y.kind == H2HIP_VS_INTERMEDIATE) touches[o.y.a]++;
        }
        std::vector<uint32_t> order(P.n_slots), renum(P.n_slots);
        for (uint32_t i = 0; i < P.n_slots; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a_, uint32_t b_) { return touches[a_] > touches[b_]; });
        for (uint32_t i = 0; i < P.n_slots; i++) renum[order[i]] = i;
        for (DevOp& o : P.ops) {
            o.dst = renum[o.dst];
            if (o.x.kind == H2HIP_VS_INTERMEDIATE) o.x.a = renum[o.x.a];
            if (o.y.kind == H2HIP_VS_INTERMEDIATE) o.y.a = renum[o.y.a];
        }
        if (result.kind == H2HIP_VS_INTERMEDIATE) result.a = renum[result.a];
    }
    P.result = result;
    return P;
}

// The no-GPU hooks (test / tooling) are given a graph alone: column counts are not known there, so every column index is accepted
static int compile_any(const h2hip_graph* g, Program* P) {
    h2hip_evalh_desc any;
    memset(&any, 0, sizeof(any));
    any.n_fixed = any.n_advice = any.n_instance = any.n_challenges = 0xffffffffu;
    if (graph_validate(*g, any, "given")) return 1;
    *P = compile_graph(*g);
    return 0;
}

// ---- the gates kernel generated per circuit (round 4) -------------------------------------------------------------------------------
// The interpreter above pays, per operation and wave, an eight-dword scalar load of the op, two wave-uniform switches and nine LDS
// dwords in and out of a slot: 38 k VALU instructions per wave for a 24-gate program whose arithmetic is ~31 k, at 64-75 % of the
// issue rate because every operation waits for its LDS traffic.  A circuit's program never changes, so it is also emitted as
// straight-line HIP source -- one statement per operation, slots as local variables (registers, allocated by the compiler),
// constants as literals, rotations folded into index variables -- and compiled for gfx950 by hiprtc (dlopen'ed; in-memory headers =
// the library's own field.h / fieldu.h / evalh_dev.h, embedded as text).  The arithmetic per row is the interpreter's,
// operation for operation, so the values are the same limb for limb.  Compilation takes a second or more: it runs on a background
// thread the first time a program is seen (HALO2_HIP_EVALH_CODEGEN=1, default) while the interpreter serves the calls in between;
// code objects are cached per process by source hash and, with HALO2_HIP_CACHE_DIR set, on disk.  =2 compiles inline (tests), =0 off.
// Programs of more than Tuning::evalh_codegen_max_ops operations, or with more values alive at once than this, stay with the interpreter.
// A halo2 lookup's table expression, a shuffle's two programs and an mv-lookup argument's K + 1 are generated the same way, one kernel
// per argument that ends with the stage's row function of evalh_dev.h (GenKind below); the limits then count a kernel's programs together.
#define EVALH_CODEGEN_MAX_SLOTS 48
// mode: 0 off, 1 background compile (default), 2 compile inline; + 16: without the fusion of two products; the two-bit field at + 32 / + 64
// selects the generated kernels of the shuffle and mv-lookup stages: 0 the default set (Tuning::evalh_gen_shuffle / evalh_gen_mvlookup),
// + 32 none (gates and lookups keep theirs), + 64 both; max_ops 0 restores the default
extern "C" int h2hip_debug_set_evalh_codegen(int mode, uint32_t max_ops) {
    TuneWrite t;
    evalh_codegen_apply(t.operator->(), mode, max_ops);
    return 0;
}
struct RtcStats {
    std::atomic<uint64_t> compiled{0}, failed{0}, launches{0}, interpreted{0}, disk_hits{0};
    // per kind (GenKind): launches of a generated kernel and of the interpreter.  launches / interpreted above are the gates' and the
    // lookups' alone, as before the stage kernels existed (tools/evalh_bench.py reads them)
    std::atomic<uint64_t> gen[4] = {}, interp[4] = {};
    std::atomic<uint64_t> pending{0};  // background compilations queued or running
    void launched(int kind, bool generated) {
        (generated ? gen : interp)[kind]++;
        if (kind <= 1) (generated ? launches : interpreted)++;
    }
};
static RtcStats g_rtc_stats;
extern "C" int h2hip_debug_evalh_codegen_stats(uint64_t out[5]) {
    if (!out) return H2HIP_EINVAL;
    out[0] = g_rtc_stats.compiled;
    out[1] = g_rtc_stats.failed;
    out[2] = g_rtc_stats.launches;
    out[3] = g_rtc_stats.interpreted;
    out[4] = g_rtc_stats.disk_hits;
    return 0;
}
extern "C" int h2hip_debug_evalh_codegen_stage_stats(uint64_t out[9]) {
    if (!out) return H2HIP_EINVAL;
    for (int k = 0; k < 4; k++) {
        out[2 * k] = g_rtc_stats.gen[k];
        out[2 * k + 1] = g_rtc_stats.interp[k];
    }
    out[8] = g_rtc_stats.pending;
    return 0;
}

#include "rtc_headers.inc"

struct Hiprtc {
    void* lib = nullptr;
    hiprtcResult (*Create)(hiprtcProgram*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    hiprtcResult (*Compile)(hiprtcProgram, int, const char* const*) = nullptr;
    hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t*) = nullptr;
    hiprtcResult (*GetCode)(hiprtcProgram, char*) = nullptr;
    hiprtcResult (*GetLogSize)(hiprtcProgram, size_t*) = nullptr;
    hiprtcResult (*GetLog)(hiprtcProgram, char*) = nullptr;
    hiprtcResult (*Destroy)(hiprtcProgram*) = nullptr;
};
static Hiprtc g_hiprtc;
static std::mutex g_rtc_mu;  // g_hiprtc, g_rtc

static bool hiprtc_load() {  // under g_rtc_mu
    Hiprtc& r = g_hiprtc;
    if (r.lib) return true;
    void* h = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return false;
    r.Create = (decltype(r.Create))dlsym(h, "hiprtcCreateProgram");
    r.Compile = (decltype(r.Compile))dlsym(h, "hiprtcCompileProgram");
    r.GetCodeSize = (decltype(r.GetCodeSize))dlsym(h, "hiprtcGetCodeSize");
    r.GetCode = (decltype(r.GetCode))dlsym(h, "hiprtcGetCode");
    r.GetLogSize = (decltype(r.GetLogSize))dlsym(h, "hiprtcGetProgramLogSize");
    r.GetLog = (decltype(r.GetLog))dlsym(h, "hiprtcGetProgramLog");
    r.Destroy = (decltype(r.Destroy))dlsym(h, "hiprtcDestroyProgram");
    if (!r.Create || !r.Compile || !r.GetCodeSize || !r.GetCode || !r.GetLogSize || !r.GetLog || !r.Destroy) return false;
    r.lib = h;
    return true;
}

// Two products that meet in a sum or difference share ONE Montgomery reduction (fu_mul_sub: (ab - cd) / 2^261, the columns of both
// products in one accumulator; a sum passes -c): a product whose only reader is the next ADD / SUB / Horner step on its slot is not
// emitted where the program has it but inside that reader.  Per gate of the usual shape -- selector * (product - product + ...)
// folded with y -- that is two of six reductions.  The value is the same field element (the reduced representative may differ by a
// multiple of r before the closing exact reduction, which the interpreter's magnitude bounds cover: the fused form's bound,
// (|a||b| + |c||d|) / 169 + 1, is below the sum of the two separate ones).
// The decision alone, for gen_source and for the program hook (h2hip_debug_evalh_program): per op, the op it is emitted inside, or -1.
static std::vector<int> fusion_plan(const Program& P, bool fuse) {
    const size_t n_ops = P.ops.size();
    std::vector<int> fused_into(n_ops, -1);  // product i is emitted inside op fused_into[i]
    if (fuse) {
        auto is_slot = [](const h2hip_value_source& v) { return v.kind == H2HIP_VS_INTERMEDIATE; };
        for (size_t i = 0; i < n_ops; i++) {
            const DevOp& m = P.ops[i];
            if (m.op != OP_MUL) continue;  // (a product carrying a reduction request stays where it is)
            const uint32_t X = m.dst;
            int reader = -1;
            bool ok = true;
            for (size_t j = i + 1; j < n_ops && ok; j++) {
                const DevOp& o = P.ops[j];
                const uint32_t k = o.op & 0xff;
                const bool rx = is_slot(o.x) && o.x.a == X, ry = is_slot(o.y) && o.y.a == X, rd = k == OP_FMA && o.dst == X;
                if (reader < 0) {
                    if (rx || ry || rd) {
                        // the one reader: an ADD / SUB taking it as either operand (not both), or a Horner step taking it as the addend
                        if ((k == OP_ADD || k == OP_SUB) && rx != ry && !rd) reader = (int)j;
                        else if (k == OP_FMA && rx && !ry && !rd) reader = (int)j;
                        else ok = false;
                        if (ok && o.dst == X) break;  // the reader overwrites the slot: nothing later sees the product
                        continue;
                    }
                    if (o.dst == X) ok = false;  // overwritten unread: dead code the compiler kept (cannot happen), leave it alone
                    // the product's own operands must still hold their values when the reader runs
                    if ((is_slot(m.x) && o.dst == m.x.a) || (is_slot(m.y) && o.dst == m.y.a)) ok = false;
                } else {
                    if (rx || ry || rd) ok = false;   // a second reader
                    else if (o.dst == X) break;       // overwritten: the product was dead after its one reader
                }
            }
            if (ok && reader >= 0 && !(is_slot(P.result) && P.result.a == X && P.ops[reader].dst != X)) fused_into[i] = reader;
        }
        // an ADD / SUB fuses only when BOTH operands are such products; a Horner step when its addend is
        std::vector<int> cnt(n_ops, 0);
        for (size_t i = 0; i < n_ops; i++)
            if (fused_into[i] >= 0) cnt[fused_into[i]]++;
        for (size_t i = 0; i < n_ops; i++)
            if (fused_into[i] >= 0) {
                const uint32_t k = P.ops[fused_into[i]].op & 0xff;
                if ((k == OP_ADD || k == OP_SUB) && cnt[fused_into[i]] != 2) fused_into[i] = -1;
            }
    }
    return fused_into;
}

// the program as HIP source.  Operands: constants are literals (I-form limbs), slots are locals, a column operand is a load at the
// row index of its rotation (one index variable per distinct rotation), challenges and beta / gamma / theta / y come with the launch.
static constexpr bool EVALH_GEN_BARRIERS = true;
// What one generated kernel is made of: kind and the programs in the order the kernel runs them.
//   gates     one program; the row stores its result
//   lookup    one program, a lookup argument's compressed table expression (evaluated with PreviousValue = 0, :466-480); the kernel ends
//             with that argument's five constraints (lookup_row, evalh_dev.h) instead of storing the program's result
//   shuffle   two programs, the input side's then the shuffle side's; the kernel ends with shuffle_row
//   mvlookup  K + 1 programs, the K input tuples' in argument order then the table's; the kernel ends with mvlookup_row
enum GenKind { GEN_GATES = 0, GEN_LOOKUP = 1, GEN_SHUFFLE = 2, GEN_MVLOOKUP = 3, GEN_KINDS = 4 };
static const char* const GEN_KERNEL_NAME[GEN_KINDS] = {"evalh_gates_gen", "evalh_lookup_gen", "evalh_shuffle_gen", "evalh_mvlookup_gen"};
struct GenUnit {
    GenKind kind;
    std::vector<const h2hip_graph*> graphs;
    std::vector<const Program*> progs;
    bool stage() const { return kind >= GEN_SHUFFLE; }
    size_t n_ops() const {
        size_t n = 0;
        for (const Program* P : progs) n += P->ops.size();
        return n;
    }
    uint32_t n_slots() const {  // locals the programs share: slot s of one program is slot s of the next
        uint32_t n = 0;
        for (const Program* P : progs) n = std::max(n, P->n_slots);
        return n;
    }
    // values alive at once: the largest program's slots and what the kernel holds across programs (a shuffle's a; an mv-lookup's P and Q)
    uint32_t n_live() const { return n_slots() + (kind == GEN_SHUFFLE ? 1u : kind == GEN_MVLOOKUP ? 2u : 0u); }
};
static GenUnit gen_unit(GenKind kind, const h2hip_graph* const* graphs, const Program* progs, size_t n) {
    GenUnit u;
    u.kind = kind;
    for (size_t i = 0; i < n; i++) {
        u.graphs.push_back(graphs[i]);
        u.progs.push_back(progs + i);
    }
    return u;
}
// within the generator's limits (beyond them the stage keeps the interpreter): an empty gates program has no kernel, an empty graph of
// another kind has value zero and is generated as that
static bool gen_within_limits(const GenUnit& u) {
    if (u.kind == GEN_GATES && u.progs[0]->ops.empty()) return false;
    return u.n_ops() <= tune().evalh_codegen_max_ops && u.n_live() <= EVALH_CODEGEN_MAX_SLOTS;
}

// How program `prog` of a kernel spells its operands.  The lone program of a gates / lookup kernel: constants K<i>, one row index r<i> per
// entry of its rotations table.  A program of a stage kernel: constants K<prog>_<i> (literals per program), row indices by rotation VALUE
// (rp<v> / rm<v>), so that a rotation two programs use is formed once; column pointers are named by (kind, index) in both.
struct GenNames {
    const h2hip_graph* g;
    int prog;  // < 0: the lone program
};
static const char* const gen_tab_name[3] = {"fixed", "advice", "instance"};
static const char gen_col_name[3] = {'F', 'A', 'N'};
static std::string gen_rot_value_name(int32_t rotation) {
    char t[32];
    const int64_t v = rotation;
    snprintf(t, sizeof(t), v < 0 ? "rm%lld" : "rp%lld", (long long)(v < 0 ? -v : v));
    return t;
}
static std::string gen_rot_name(const GenNames& nm, uint32_t b) {
    if (nm.prog >= 0) return gen_rot_value_name(nm.g->rotations[b]);
    char t[32];
    snprintf(t, sizeof(t), "r%u", b);
    return t;
}
static std::string gen_operand(const GenNames& nm, const h2hip_value_source& v) {
    char t[96];
    switch (v.kind) {
        case H2HIP_VS_CONSTANT:
            if (nm.prog < 0) snprintf(t, sizeof(t), "K%u", v.a);
            else snprintf(t, sizeof(t), "K%d_%u", nm.prog, v.a);
            break;
        case H2HIP_VS_INTERMEDIATE: snprintf(t, sizeof(t), "s%u", v.a); break;
        case H2HIP_VS_FIXED: case H2HIP_VS_ADVICE: case H2HIP_VS_INSTANCE:
            snprintf(t, sizeof(t), "ld_i(%c%u[%s])", gen_col_name[v.kind - H2HIP_VS_FIXED], v.a, gen_rot_name(nm, v.b).c_str());
            break;
        case H2HIP_VS_CHALLENGE: snprintf(t, sizeof(t), "ld_const_fu(c.challenges, %u)", v.a); break;
        case H2HIP_VS_BETA: return "c.beta";
        case H2HIP_VS_GAMMA: return "c.gamma";
        case H2HIP_VS_THETA: return "c.theta";
        case H2HIP_VS_Y: return "c.y";
        case H2HIP_VS_PREVIOUS: return "prev";
        default: return "fu_zero()";
    }
    return t;
}
static void gen_add(std::string& src, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    src += buf;
}
// what a program reads, noted for the declarations in front of the first statement
struct GenUses {
    std::vector<uint8_t> consts, rots;
    std::vector<uint8_t> cols[3];
};
static GenUses gen_uses(const h2hip_graph& g, const Program& P) {
    GenUses u;
    u.consts.assign(g.n_constants, 0);
    u.rots.assign(g.n_rotations, 0);
    auto note = [&](const h2hip_value_source& v) {
        if (v.kind == H2HIP_VS_CONSTANT) u.consts[v.a] = 1;
        if (v.kind == H2HIP_VS_FIXED || v.kind == H2HIP_VS_ADVICE || v.kind == H2HIP_VS_INSTANCE) {
            std::vector<uint8_t>& c = u.cols[v.kind - H2HIP_VS_FIXED];
            if (c.size() <= v.a) c.resize((size_t)v.a + 1, 0);
            c[v.a] = 1;
            u.rots[v.b] = 1;
        }
    };
    for (const DevOp& o : P.ops) {
        note(o.x);
        note(o.y);
    }
    note(P.result);
    return u;
}
static void gen_constants(std::string& src, const GenNames& nm, const GenUses& u) {
    for (uint32_t i = 0; i < nm.g->n_constants; i++)
        if (u.consts[i]) {
            const Fu k = to_i(fe_from_u64x4(nm.g->constants + 4 * (size_t)i));
            gen_add(src, "    const Fu %s = {{%d, %d, %d, %d, %d, %d, %d, %d, %d}};\n", gen_operand(nm, {H2HIP_VS_CONSTANT, i, 0}).c_str(), k.l[0], k.l[1],
                    k.l[2], k.l[3], k.l[4], k.l[5], k.l[6], k.l[7], k.l[8]);
        }
}
// the statements of one program: one per operation, a fused product inside its reader (fusion_plan), one scheduling region each
static void gen_ops(std::string& src, const GenNames& nm, const Program& P) {
    const size_t n_ops = P.ops.size();
    const std::vector<int> fused_into = fusion_plan(P, tune().evalh_gen_fuse);  // product i is emitted inside op fused_into[i]
    auto operand = [&](const h2hip_value_source& v) { return gen_operand(nm, v); };
    auto product_of = [&](size_t j, const h2hip_value_source& v) -> const DevOp* {  // the product fused into op j that v names
        for (size_t i = 0; i < j; i++)
            if (fused_into[i] == (int)j && v.kind == H2HIP_VS_INTERMEDIATE && P.ops[i].dst == v.a) return &P.ops[i];
        return nullptr;
    };
    for (size_t q = 0; q < n_ops; q++) {
        const DevOp& o = P.ops[q];
        if (fused_into[q] >= 0) continue;  // emitted inside its reader
        const std::string x = operand(o.x), y = operand(o.y);
        const uint32_t dst = o.dst;
        const DevOp *px = product_of(q, o.x), *py = product_of(q, o.y);
        const uint32_t kind = o.op & 0xff;
        if ((kind == OP_ADD || kind == OP_SUB) && px && py) {
            gen_add(src, "    s%u = fu_mul_sub<UF>(%s, %s, ", dst, operand(px->x).c_str(), operand(px->y).c_str());
            gen_add(src, kind == OP_SUB ? "%s, %s);\n" : "fu_neg(%s), %s);\n", operand(py->x).c_str(), operand(py->y).c_str());
        } else if (kind == OP_FMA && px) {
            gen_add(src, "    s%u = fu_mul_sub<UF>(s%u, %s, fu_neg(%s), %s);\n", dst, dst, y.c_str(), operand(px->x).c_str(), operand(px->y).c_str());
        } else
        switch (kind) {
            case OP_ADD: gen_add(src, "    s%u = addn(%s, %s);\n", dst, x.c_str(), y.c_str()); break;
            case OP_SUB: gen_add(src, "    s%u = subn(%s, %s);\n", dst, x.c_str(), y.c_str()); break;
            case OP_MUL: gen_add(src, "    s%u = mul_i(%s, %s);\n", dst, x.c_str(), y.c_str()); break;
            case OP_SQR: gen_add(src, "    s%u = fu_sqr<UF>(%s);\n", dst, x.c_str()); break;
            case OP_DBL: gen_add(src, "    s%u = fu_norm(fu_dbl(%s));\n", dst, x.c_str()); break;
            case OP_NEG: gen_add(src, "    s%u = fu_norm(fu_neg(%s));\n", dst, x.c_str()); break;
            case OP_FMA: gen_add(src, "    s%u = addn(mul_i(s%u, %s), %s);\n", dst, dst, y.c_str(), x.c_str()); break;
            default: gen_add(src, "    s%u = %s;\n", dst, x.c_str());  // OP_MOV
        }
        if (o.op & OP_REDUCE_FLAG) gen_add(src, "    s%u = mul_i(s%u, fu_one_i<UF>());\n", dst, dst);
        // one scheduling region per operation: the whole program as ONE basic block (tens of thousands of instructions) costs the
        // scheduler and the register allocator minutes and buys nothing -- a field multiplication already fills the pipeline
        if (EVALH_GEN_BARRIERS) src += "    __builtin_amdgcn_sched_barrier(0);\n";
    }
}
static void gen_slots(std::string& src, uint32_t n_slots) {
    if (!n_slots) return;
    src += "    Fu s0";
    for (uint32_t i = 1; i < n_slots; i++) gen_add(src, ", s%u", i);
    src += ";\n";
}

// a gates or a lookup kernel: one program
static std::string gen_source(const h2hip_graph& g, const Program& P, bool lookup = false) {
    std::string src;
    src.reserve(64 * P.ops.size() + 4096);
    const GenNames nm = {&g, -1};
    const GenUses u = gen_uses(g, P);
    src += "#include \"evalh_dev.h\"\nusing namespace h2;\n";
    src += lookup ? "extern \"C\" __global__ void __launch_bounds__(256) evalh_lookup_gen(ColsDev c, LookupDev l, Fe* values) {\n"
                  : "extern \"C\" __global__ void __launch_bounds__(256) evalh_gates_gen(ColsDev c, Fe* __restrict__ values) {\n";
    src += "    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;\n"
           "    if (idx >= (1u << c.log_size)) return;\n";
    src += lookup ? "    const Fu prev = fu_zero();\n"
                  : "    const Fe prev_e = values[idx];\n"
                    "    const Fu prev = ld_i(prev_e);\n";
    src += "    (void)prev;\n";
    gen_constants(src, nm, u);
    for (int t = 0; t < 3; t++)
        for (uint32_t i = 0; i < u.cols[t].size(); i++)
            if (u.cols[t][i]) gen_add(src, "    const Fe* __restrict__ %c%u = ld_const_col(c.%s, %u);\n", gen_col_name[t], i, gen_tab_name[t], i);
    for (uint32_t i = 0; i < g.n_rotations; i++)
        if (u.rots[i]) gen_add(src, "    const uint32_t r%u = rot_idx(idx, %d, c.rot_scale, c.log_size);\n", i, g.rotations[i]);
    gen_slots(src, P.n_slots);
    gen_ops(src, nm, P);
    if (lookup) {
        gen_add(src, "    lookup_row(l, c, idx, %s, values);\n}\n", gen_operand(nm, P.result).c_str());
        return src;
    }
    switch (P.result.kind) {  // prog_result_e
        case H2HIP_VS_FIXED: case H2HIP_VS_ADVICE: case H2HIP_VS_INSTANCE:
            gen_add(src, "    values[idx] = %c%u[r%u];\n", gen_col_name[P.result.kind - H2HIP_VS_FIXED], P.result.a, P.result.b);
            break;
        case H2HIP_VS_PREVIOUS: src += "    (void)prev_e;\n"; break;
        case EVALH_VS_ZERO: src += "    values[idx] = fe_zero<FrP>();\n"; break;
        default: gen_add(src, "    values[idx] = out_e(%s);\n", gen_operand(nm, P.result).c_str());
    }
    src += "}\n";
    return src;
}

// A stage kernel: the programs of one shuffle or one mv-lookup argument in ONE straight-line kernel that ends with the stage's row
// function.  A column pointer is loaded once per distinct (kind, index) and a rotated row index formed once per distinct rotation value
// across all the programs -- the tuples of an argument typically share selectors and columns, which the interpreter loads once per
// program; the slot locals are one set, reused from one program to the next, and what crosses from one program to the next is held in
// locals of its own (a; P and Q).  Magnitudes entering the row functions: each program's result is what the interpreter's is -- a slot
// [< 15] (compile_graph's closing reduction is an operation of the program like any other; a fused pair's bound is below the separate
// ones', see fusion_plan), a column [< 32], a constant, challenge, theta, beta or gamma [<= 1], an empty graph [0] -- so a, s, f_c and
// tau are [< 32], P [<= 1.3] and Q [<= 2.9] as shuffle_row and mvlookup_row assume (evalh_dev.h).
static std::string gen_stage_source(const GenUnit& u) {
    std::string src;
    src.reserve(64 * u.n_ops() + 4096);
    const size_t n = u.progs.size();
    src += "#include \"evalh_dev.h\"\nusing namespace h2;\n";
    src += u.kind == GEN_SHUFFLE ? "extern \"C\" __global__ void __launch_bounds__(256) evalh_shuffle_gen(ColsDev c, ShuffleDev sh, Fe* values) {\n"
                                 : "extern \"C\" __global__ void __launch_bounds__(256) evalh_mvlookup_gen(ColsDev c, MvLookupDev mv, Fe* values) {\n";
    src += "    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;\n"
           "    if (idx >= (1u << c.log_size)) return;\n";
    std::vector<GenUses> uses(n);
    std::vector<uint8_t> cols[3];
    std::vector<int32_t> rots;  // distinct rotation values, in order of first use
    for (size_t p = 0; p < n; p++) {
        uses[p] = gen_uses(*u.graphs[p], *u.progs[p]);
        gen_constants(src, {u.graphs[p], (int)p}, uses[p]);
        for (int t = 0; t < 3; t++) {
            if (cols[t].size() < uses[p].cols[t].size()) cols[t].resize(uses[p].cols[t].size(), 0);
            for (size_t i = 0; i < uses[p].cols[t].size(); i++) cols[t][i] |= uses[p].cols[t][i];
        }
        for (uint32_t i = 0; i < u.graphs[p]->n_rotations; i++)
            if (uses[p].rots[i] && std::find(rots.begin(), rots.end(), u.graphs[p]->rotations[i]) == rots.end()) rots.push_back(u.graphs[p]->rotations[i]);
    }
    for (int t = 0; t < 3; t++)
        for (uint32_t i = 0; i < cols[t].size(); i++)
            if (cols[t][i]) gen_add(src, "    const Fe* __restrict__ %c%u = ld_const_col(c.%s, %u);\n", gen_col_name[t], i, gen_tab_name[t], i);
    for (int32_t v : rots) gen_add(src, "    const uint32_t %s = rot_idx(idx, %d, c.rot_scale, c.log_size);\n", gen_rot_value_name(v).c_str(), v);
    gen_slots(src, u.n_slots());
    if (u.kind == GEN_MVLOOKUP) src += "    Fu P = fu_one_i<UF>(), Q = fu_zero();\n";
    for (size_t p = 0; p < n; p++) {
        const GenNames nm = {u.graphs[p], (int)p};
        gen_ops(src, nm, *u.progs[p]);
        const std::string r = gen_operand(nm, u.progs[p]->result);
        if (u.kind == GEN_SHUFFLE) {
            if (p == 0) gen_add(src, "    const Fu a = %s;\n", r.c_str());
            else gen_add(src, "    shuffle_row(sh, c, idx, a, %s, values);\n", r.c_str());
        } else if (p + 1 < n) {  // input tuple p: Q = Q f + P; P = P f
            gen_add(src, "    {\n        const Fu f = %s;\n        Q = addn(mul_i(Q, f), P);\n        P = mul_i(P, f);\n    }\n", r.c_str());
            if (EVALH_GEN_BARRIERS) src += "    __builtin_amdgcn_sched_barrier(0);\n";
        } else {
            gen_add(src, "    mvlookup_row(mv, c, idx, %s, P, Q, values);\n", r.c_str());
        }
    }
    src += "}\n";
    return src;
}
static std::string gen_unit_source(const GenUnit& u) { return u.stage() ? gen_stage_source(u) : gen_source(*u.graphs[0], *u.progs[0], u.kind == GEN_LOOKUP); }

static uint64_t fnv1a64_raw(const char* p, size_t n, uint64_t h) {
    for (size_t i = 0; i < n; i++) {
        h ^= (unsigned char)p[i];
        h *= 0x100000001b3ull;
    }
    return h;
}
// key of a generated kernel: its source AND the embedded headers it is compiled against (a code object left in HALO2_HIP_CACHE_DIR by
// another build of the library, whose arithmetic headers differ, must not be picked up)
static uint64_t fnv1a64(const std::string& s) {
    static const uint64_t headers = [] {
        uint64_t h = 0xcbf29ce484222325ull;
        for (int i = 0; i < H2_RTC_N_HEADERS; i++) h = fnv1a64_raw(H2_RTC_HEADER_TEXT[i], strlen(H2_RTC_HEADER_TEXT[i]), h);
        return h;
    }();
    return fnv1a64_raw(s.data(), s.size(), headers);
}

struct RtcEntry {
    std::mutex m;
    int state = 0;  // 0 compiling, 1 ready, 2 failed
    std::vector<char> code;
    std::string log;
    std::thread th;
    double compile_s = 0.0;
    // a process that exits without h2hip_shutdown still destroys the cache (static destruction): a joinable std::thread must not meet its destructor
    ~RtcEntry() {
        if (th.joinable()) th.join();
    }
};
static std::map<uint64_t, std::shared_ptr<RtcEntry>> g_rtc;
// Background compilations (mode 1) that may be queued or running when a stage kernel asks for one more.  At the bound the call skips its
// request -- nothing is recorded, a later call asks again -- and the interpreter serves: a process that meets many distinct arguments once
// each (a test suite does) then leaves seconds of queued compiles behind it, not minutes.  Gates and lookup kernels are always queued.
static constexpr uint64_t EVALH_RTC_MAX_PENDING = 8;

static std::string rtc_cache_path(uint64_t key) {
    const char* dir = getenv("HALO2_HIP_CACHE_DIR");
    if (!dir || !*dir) return std::string();
    char name[64];
    snprintf(name, sizeof(name), "/evalh_gates_%016llx_gfx950.co", (unsigned long long)key);
    return std::string(dir) + name;
}

static void rtc_compile(std::shared_ptr<RtcEntry> e, std::string src, uint64_t key) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<char> code;
    std::string log;
    bool ok = false;
    const std::string path = rtc_cache_path(key);
    if (!path.empty()) {  // a code object an earlier process left for this very source
        if (FILE* f = fopen(path.c_str(), "rb")) {
            fseek(f, 0, SEEK_END);
            const long sz = ftell(f);
            fseek(f, 0, SEEK_SET);
            if (sz > 0) {
                code.resize((size_t)sz);
                ok = fread(code.data(), 1, (size_t)sz, f) == (size_t)sz;
            }
            fclose(f);
            if (ok) g_rtc_stats.disk_hits++;
        }
    }
    if (!ok) {
        // one compilation at a time: a circuit brings a gates kernel and one kernel per lookup, shuffle and mv-lookup argument, each on its
        // own background thread, and nothing here relies on the run-time compiler being re-entrant.  So queued compilations wait in
        // line, at ~20 ms per operation, and a process joins them when it ends: EVALH_RTC_MAX_PENDING bounds the line for stage kernels.
        static std::mutex compile_mu;
        std::lock_guard<std::mutex> one(compile_mu);
        hiprtcProgram prog = nullptr;
        hiprtcResult r = g_hiprtc.Create(&prog, src.c_str(), "evalh_gates_gen.hip", H2_RTC_N_HEADERS, H2_RTC_HEADER_TEXT, H2_RTC_HEADER_NAMES);
        if (r == HIPRTC_SUCCESS) {
            const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
            r = g_hiprtc.Compile(prog, 3, opts);
            size_t ls = 0;
            if (g_hiprtc.GetLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
                log.resize(ls);
                (void)g_hiprtc.GetLog(prog, &log[0]);
            }
            size_t cs = 0;
            if (r == HIPRTC_SUCCESS && g_hiprtc.GetCodeSize(prog, &cs) == HIPRTC_SUCCESS && cs) {
                code.resize(cs);
                ok = g_hiprtc.GetCode(prog, code.data()) == HIPRTC_SUCCESS;
            }
            (void)g_hiprtc.Destroy(&prog);
        }
        if (ok && !path.empty()) {  // write-then-rename: a concurrent reader sees the whole file or none
            const std::string tmp = path + ".tmp" + std::to_string((unsigned long long)key ^ (unsigned long long)(uintptr_t)&code);
            if (FILE* f = fopen(tmp.c_str(), "wb")) {
                const bool w = fwrite(code.data(), 1, code.size(), f) == code.size();
                fclose(f);
                if (!w || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());
            }
        }
    }
    std::lock_guard<std::mutex> lk(e->m);
    e->compile_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    e->log.swap(log);
    if (ok) {
        e->code.swap(code);
        e->state = 1;
        g_rtc_stats.compiled++;
    } else {
        e->state = 2;
        g_rtc_stats.failed++;
    }
}

static int rtc_compile_for_hook(const std::string& src, double* seconds, size_t* code_bytes) {
    {
        std::lock_guard<std::mutex> lk(g_rtc_mu);
        if (!hiprtc_load()) {
            set_error("evaluate_h: libhiprtc.so could not be loaded");
            return 2;
        }
    }
    auto e = std::make_shared<RtcEntry>();
    rtc_compile(e, src, fnv1a64(src));
    if (seconds) *seconds = e->compile_s;
    if (code_bytes) *code_bytes = e->code.size();
    if (e->state != 1) {
        set_error("evaluate_h: hiprtc rejected the generated kernel: %.300s", e->log.c_str());
        return 2;
    }
    return 0;
}
static void copy_source(const std::string& src, char* buf, size_t cap, size_t* len) {
    *len = src.size();
    if (buf && cap) {
        const size_t m = src.size() < cap - 1 ? src.size() : cap - 1;
        memcpy(buf, src.data(), m);
        buf[m] = 0;
    }
}

// test / tooling hook, no GPU needed: the source a graph's program is emitted as, and (compile != 0) what hiprtc makes of it
extern "C" int h2hip_debug_evalh_codegen_source(const h2hip_graph* g, char* buf, size_t cap, size_t* len, int compile, double* seconds,
                                                size_t* code_bytes) {
    if (!g || !len) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    Program P;
    TuneRead r;
    if (compile_any(g, &P)) return 1;
    const std::string src = gen_source(*g, P, (compile & 2) != 0);  // bit 1: the graph as a lookup's table expression (evalh_lookup_gen)
    copy_source(src, buf, cap, len);
    if (!(compile & 1)) return 0;
    return rtc_compile_for_hook(src, seconds, code_bytes);
}

// The three grouped arguments behind the gates and the permutation, in the order of the call plan and of the pass.  Per argument a stage
// has `cosets` product polynomials, formed as cosets in buffers that a group of arguments shares (stage_group), and one kernel that folds
// the argument's programs into `values`: 1 per lookup, K_j + 1 per mv-lookup argument, 2 per shuffle.
// `eager` is what the lookups alone have from before the other two existed: the cosets of their first group are formed in the batch of
// the advice and instance columns (later groups on demand, like every group of the other stages), and their profile interval is one per
// pass, those later transforms included, where the others' is one per argument without its group's transform.
enum { ST_LOOKUP = 0, ST_MVLOOKUP = 1, ST_SHUFFLE = 2, N_STAGES = 3 };
#define VS_BIT(kind) (1u << H2HIP_VS_##kind)
struct Stage {
    GenKind kind;
    uint32_t cosets;
    const char* profile;
    uint32_t barred;  // value sources (VS_BIT) the stage's graphs may not read: no kernel of the stage supplies them
    bool eager;
};
static const Stage STAGES[N_STAGES] = {
    {GEN_LOOKUP, 3, "evalh_lookups", 0, true},
    {GEN_MVLOOKUP, 2, "evalh_mvlookups", VS_BIT(GAMMA) | VS_BIT(Y) | VS_BIT(PREVIOUS), false},
    {GEN_SHUFFLE, 1, "evalh_shuffles", VS_BIT(BETA) | VS_BIT(Y) | VS_BIT(PREVIOUS), false},
};

// every operand of every calculation of g, Horner parts included, is a value source of a kind in `allowed` (VS_BIT); *bad: the first
// calculation that reads another
static bool graph_reads_only(const h2hip_graph& g, uint32_t allowed, uint32_t* bad) {
    auto ok = [&](const h2hip_value_source& v) { return v.kind < 32 && (allowed >> v.kind & 1); };
    for (uint32_t q = 0; q < g.n_calculations; q++) {
        const h2hip_calculation& cl = g.calculations[q];
        bool fine = ok(cl.x);
        if (cl.op == H2HIP_CALC_ADD || cl.op == H2HIP_CALC_SUB || cl.op == H2HIP_CALC_MUL || cl.op == H2HIP_CALC_HORNER) fine = fine && ok(cl.y);
        if (cl.op == H2HIP_CALC_HORNER)
            for (uint32_t t = 0; fine && t < cl.parts_count; t++) fine = ok(g.parts[cl.parts_offset + t]);
        if (!fine) {
            *bad = q;
            return false;
        }
    }
    return true;
}

// ... and the source of a stage kernel: kind 1 = a shuffle's two graphs (input side, shuffle side), kind 2 = an mv-lookup argument's
// K + 1 graphs (the K input tuples', then the table's).  3: beyond the generator's limits -- the engine keeps the interpreter
extern "C" int h2hip_debug_evalh_codegen_stage_source(const h2hip_graph* graphs, uint32_t n_graphs, int kind, char* buf, size_t cap, size_t* len,
                                                      int compile, double* seconds, size_t* code_bytes) {
    if (!graphs || !len || (kind != 1 && kind != 2) || (kind == 1 && n_graphs != 2) || (kind == 2 && (n_graphs < 2 || n_graphs > 256))) {
        set_error("evaluate_h: stage source: null argument, or a kind / number of graphs that is no shuffle (1: two graphs) or mv-lookup (2: K + 1)");
        return 1;
    }
    TuneRead r;
    const Stage& st = STAGES[kind == 1 ? ST_SHUFFLE : ST_MVLOOKUP];
    std::vector<Program> progs(n_graphs);
    std::vector<const h2hip_graph*> gp(n_graphs);
    for (uint32_t i = 0, q; i < n_graphs; i++) {
        if (compile_any(&graphs[i], &progs[i])) return 1;
        gp[i] = &graphs[i];
        if (!graph_reads_only(graphs[i], ~st.barred, &q)) {
            set_error("evaluate_h: %s graph %u, calculation %u reads a value the stage does not supply", kind == 1 ? "shuffle" : "mv-lookup", i, q);
            return 1;
        }
    }
    const GenUnit u = gen_unit(st.kind, gp.data(), progs.data(), n_graphs);
    if (!gen_within_limits(u)) {
        *len = 0;
        set_error("evaluate_h: stage kernel beyond the generator's limits (%zu operations, %u live values)", u.n_ops(), u.n_live());
        return 3;
    }
    const std::string src = gen_stage_source(u);
    copy_source(src, buf, cap, len);
    if (!(compile & 1)) return 0;
    return rtc_compile_for_hook(src, seconds, code_bytes);
}

// join the compile threads (h2hip_shutdown, after the contexts are released); the compiled code stays cached for a later init
void evalh_rtc_shutdown() {
    std::lock_guard<std::mutex> lk(g_rtc_mu);
    for (auto& kv : g_rtc)
        if (kv.second->th.joinable()) kv.second->th.join();
}

void evalh_modules_free(Ctx* c) {
    for (auto& kv : c->evalh_mods)
        if (kv.second.first) (void)hipModuleUnload((hipModule_t)kv.second.first);
    c->evalh_mods.clear();
}

// what the generator reads of a kernel's programs, hashed: every call of evaluate_h comes here, and writing (and hashing) 20 KB of source
// each time to find a kernel that is already loaded is ~150 us of host time per call.  The kind and every program of the kernel.
static uint64_t unit_fingerprint(const GenUnit& u) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t p = 0; p < u.progs.size(); p++) {
        const h2hip_graph& g = *u.graphs[p];
        const Program& P = *u.progs[p];
        if (!P.ops.empty()) h = fnv1a64_raw((const char*)P.ops.data(), P.ops.size() * sizeof(DevOp), h);
        if (g.n_constants) h = fnv1a64_raw((const char*)g.constants, (size_t)g.n_constants * 32, h);
        if (g.n_rotations) h = fnv1a64_raw((const char*)g.rotations, (size_t)g.n_rotations * sizeof(int32_t), h);
        const uint32_t tail[7] = {P.result.kind, P.result.a, P.result.b, P.n_slots, (uint32_t)P.ops.size(), g.n_constants, g.n_rotations};
        h = fnv1a64_raw((const char*)tail, sizeof(tail), h);
    }
    const uint32_t tail[3] = {(uint32_t)u.kind, (uint32_t)u.progs.size(), (tune().evalh_gen_fuse ? 1u : 0u) | (EVALH_GEN_BARRIERS ? 2u : 0u)};
    return fnv1a64_raw((const char*)tail, sizeof(tail), h);
}
// fingerprint -> the kernel's source key and how far it has come (under g_rtc_mu).  A kernel that failed, or is still compiling, costs a
// call this lookup, not a gen_source and a hash of its source.
struct RtcKnown {
    uint64_t key;
    int state;  // RtcEntry's: 0 compiling, 1 ready, 2 failed
};
static std::map<uint64_t, RtcKnown> g_rtc_known;

static void rtc_compile_background(std::shared_ptr<RtcEntry> e, std::string src, uint64_t key) {
    rtc_compile(e, std::move(src), key);
    g_rtc_stats.pending--;
}

// the generated kernel for these programs on this device, or nullptr: not wanted, not compiled yet (the interpreter serves this call), or
// not compilable (it serves every call)
static hipFunction_t kernel_for(Ctx* c, const GenUnit& u) {
    const int mode = tune().evalh_codegen;
    if (mode <= 0 || !gen_within_limits(u)) return nullptr;
    if ((u.kind == GEN_SHUFFLE && !tune().evalh_gen_shuffle) || (u.kind == GEN_MVLOOKUP && !tune().evalh_gen_mvlookup)) return nullptr;
    const uint64_t fp = unit_fingerprint(u);
    std::shared_ptr<RtcEntry> e;
    uint64_t key = 0;
    {
        std::lock_guard<std::mutex> lk(g_rtc_mu);
        auto known = g_rtc_known.find(fp);
        if (known != g_rtc_known.end()) {
            if (known->second.state == 2) return nullptr;
            key = known->second.key;
            auto hit = c->evalh_mods.find(key);
            if (hit != c->evalh_mods.end()) return (hipFunction_t)hit->second.second;
            e = g_rtc[key];
            if (known->second.state == 0) {
                if (mode >= 2 && e->th.joinable()) e->th.join();  // tests: wait for a compile another call started
                std::lock_guard<std::mutex> le(e->m);
                known->second.state = e->state;
                if (e->state != 1) return nullptr;
            }
        } else if (u.stage() && mode == 1 && g_rtc_stats.pending >= EVALH_RTC_MAX_PENDING) {
            return nullptr;  // the line of background compilations is full: ask again on a later call
        }
    }
    if (!e) {
        std::string src = gen_unit_source(u);
        key = fnv1a64(src);
        auto hit = c->evalh_mods.find(key);
        if (hit != c->evalh_mods.end()) {  // the source of another fingerprint, already on this device (the fusion switch left it unchanged)
            std::lock_guard<std::mutex> lk(g_rtc_mu);
            g_rtc_known[fp] = {key, hit->second.second ? 1 : 2};
            return (hipFunction_t)hit->second.second;
        }
        bool mine = false;  // this call created the entry and compiles it inline
        {
            std::lock_guard<std::mutex> lk(g_rtc_mu);
            auto it = g_rtc.find(key);
            if (it != g_rtc.end()) {
                e = it->second;
                if (mode >= 2 && e->th.joinable()) e->th.join();
            } else {
                if (!hiprtc_load()) return nullptr;
                try {
                    e = std::make_shared<RtcEntry>();
                    g_rtc[key] = e;
                } catch (...) {
                    return nullptr;
                }
                mine = true;
                if (mode == 1) {
                    g_rtc_stats.pending++;
                    try {
                        e->th = std::thread(rtc_compile_background, e, src, key);
                        mine = false;
                    } catch (...) {  // no thread to be had: compile inline
                        g_rtc_stats.pending--;
                    }
                }
            }
            g_rtc_known[fp] = {key, 0};
        }
        if (mine) rtc_compile(e, src, key);
        int state;
        {
            std::lock_guard<std::mutex> le(e->m);
            state = e->state;
        }
        if (state != 0) {
            std::lock_guard<std::mutex> lk(g_rtc_mu);
            g_rtc_known[fp].state = state;
        }
        if (state != 1) return nullptr;
    }
    std::lock_guard<std::mutex> lk(e->m);
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (hipModuleLoadData(&mod, e->code.data()) != hipSuccess || hipModuleGetFunction(&fn, mod, GEN_KERNEL_NAME[u.kind]) != hipSuccess) {
        (void)hipGetLastError();
        if (mod) (void)hipModuleUnload(mod);
        c->evalh_mods[key] = {nullptr, nullptr};  // do not try again on this device
        return nullptr;
    }
    c->evalh_mods[key] = {(void*)mod, (void*)fn};
    return fn;
}
// programs first .. first + n of a call's plan as one kernel
static hipFunction_t kernel_for(Ctx* c, GenKind kind, const struct CallPlan& cp, size_t first, size_t n);

struct Arena {
    char* base = nullptr;
    size_t off = 0, cap = 0;
    void* take(size_t bytes) {
        size_t o = off;
        off = (off + bytes + 255) / 256 * 256;
        return off <= cap ? base + o : nullptr;
    }
};

static size_t prog_bytes(const h2hip_graph& g, const Program& P) {
    return 3 * 256 + g.n_constants * sizeof(Fu) + g.n_rotations * 4 + P.ops.size() * sizeof(DevOp);
}

// Where the slots of a program live: per-lane scratch in three sizes, or (past 256) a global workspace of
// n_slots x lanes elements with the rows taken grid-stride by `lanes` threads.
struct SlotPlan {
    int tier;        // 4, 8 (LDS), 16, 64, 256 (scratch) or 0 (global workspace)
    uint32_t lanes;  // threads launched
    size_t ws_bytes; // global workspace (tier 0)
};

static int slot_plan(uint32_t n_slots, size_t size, SlotPlan* out) {
    const uint32_t all = (uint32_t)((size + 255) / 256 * 256);
    if (n_slots <= tune().evalh_max_local_slots && n_slots <= 256) {
        out->tier = n_slots <= 4 ? 4 : n_slots <= 8 ? 8 : n_slots <= 16 ? 16 : n_slots <= 64 ? 64 : 256;
        out->lanes = all;
        out->ws_bytes = 0;
        return 0;
    }
    uint32_t lanes = all < 256u * 2048u ? all : 256u * 2048u;  // at most every wave slot of the chip
    const size_t budget = (size_t)32 << 30;
    while ((size_t)n_slots * lanes * sizeof(Fu) > budget && lanes > 16384) lanes /= 2;
    if ((size_t)n_slots * lanes * sizeof(Fu) > budget) {
        set_error("evaluate_h: a graph with %u simultaneously live intermediates does not fit this engine's workspace", n_slots);
        return H2HIP_ENOMEM;
    }
    out->tier = 0;
    out->lanes = lanes;
    out->ws_bytes = (size_t)n_slots * lanes * sizeof(Fu);
    return 0;
}

// test hook: programs needing more slots than v use the global-workspace form of the evaluate_h kernels (default 256)
extern "C" int h2hip_debug_set_evalh_max_local_slots(uint32_t v) { TuneWrite()->evalh_max_local_slots = v; return 0; }
// test hook: HBM one group of lookup cosets may take in evaluate_h (0 restores the default); a small value forces one lookup per group
extern "C" int h2hip_debug_set_evalh_lookup_group_bytes(uint64_t v) { TuneWrite()->evalh_lookup_group_bytes = v ? (size_t)v : Tuning{}.evalh_lookup_group_bytes; return 0; }

// field multiplications one row of the compiled program performs (products, squares, Horner steps, inserted reductions, and the
// exact reduction of the stored value): the numerator of the gates kernel's valu_roofline in bench.py
// test / tuning hook, needs no GPU: compile a graph as evaluate_h would and report the program's size
extern "C" int h2hip_debug_evalh_program_muls(const h2hip_graph* g, uint32_t* n_mul) {
    if (!g || !n_mul) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    Program P;
    if (compile_any(g, &P)) return 1;
    uint32_t m = 0;
    for (const DevOp& o : P.ops) {
        const uint32_t k = o.op & 0xff;
        if (k == OP_MUL || k == OP_SQR || k == OP_FMA) m++;
        if (o.op & OP_REDUCE_FLAG) m++;
    }
    if (P.result.kind == H2HIP_VS_INTERMEDIATE || P.result.kind <= H2HIP_VS_CONSTANT || (P.result.kind >= H2HIP_VS_CHALLENGE && P.result.kind <= H2HIP_VS_Y)) m++;
    *n_mul = m;
    return 0;
}

extern "C" int h2hip_debug_evalh_compile_stats(const h2hip_graph* g, uint32_t* n_ops, uint32_t* n_slots) {
    if (!g || !n_ops || !n_slots) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    Program P;
    if (compile_any(g, &P)) return 1;
    *n_ops = (uint32_t)P.ops.size();
    *n_slots = P.n_slots;
    return 0;
}

// test hook, needs no GPU: the program itself, as the kernels read it (DevOp words, reduce flags included), the magnitude compile_graph
// tracked after each op and the generator's fusion decision with fusion on and off
extern "C" int h2hip_debug_evalh_program(const h2hip_graph* g, uint32_t* ops, size_t cap_ops, uint32_t* n_ops, uint32_t* n_slots, uint32_t result[3],
                                         double* mags, int32_t* fused_on, int32_t* fused_off) {
    if (!g || !n_ops || !n_slots || !result) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    Program P;
    if (compile_any(g, &P)) return 1;
    static_assert(sizeof(DevOp) == 8 * sizeof(uint32_t), "a DevOp is the eight words ld_op reads");
    const size_t n = P.ops.size();
    *n_ops = (uint32_t)n;
    *n_slots = P.n_slots;
    result[0] = P.result.kind;
    result[1] = P.result.a;
    result[2] = P.result.b;
    if (n > cap_ops) return 0;  // the sizes alone: call again with room for n_ops
    const std::vector<int> on = fusion_plan(P, true), off = fusion_plan(P, false);
    for (size_t i = 0; i < n; i++) {
        if (ops) memcpy(ops + 8 * i, &P.ops[i], sizeof(DevOp));
        if (mags) mags[i] = P.mags[i];
        if (fused_on) fused_on[i] = on[i];
        if (fused_off) fused_off[i] = off[i];
    }
    return 0;
}

// Everything a kernel will dereference is checked here, on the host, before any device work: a malformed description is
// H2HIP_EINVAL, never a GPU fault.  Needs no device (the entry points call it before the engine is entered).
int evaluate_h_validate(const h2hip_evalh_desc* d, const void* values) {
    const uint32_t k = d->k, ek = d->extended_k;
    if (k > ek || ek > 28 || ek - k > 8) {
        set_error("evaluate_h: bad domain (k = %u, extended_k = %u)", k, ek);
        return 1;
    }
    if (!d->extended_omega || !d->g_coset || !d->g_coset_inv || !d->y || !d->beta || !d->gamma || !d->theta || !d->l0 || !d->l_last ||
        !d->l_active_row || !values || (d->n_fixed && !d->fixed_cosets) || (d->n_advice && !d->advice_polys) ||
        (d->n_instance && !d->instance_polys) || (d->n_challenges && !d->challenges)) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    if (graph_validate(d->custom_gates, *d, "custom gates")) return 1;
    if (d->n_lookups && (!d->lookup_graphs || !d->lookup_product_polys || !d->lookup_permuted_input_polys || !d->lookup_permuted_table_polys)) {
        set_error("evaluate_h: null lookup arrays");
        return 1;
    }
    for (uint32_t i = 0; i < d->n_lookups; i++)
        if (graph_validate(d->lookup_graphs[i], *d, "lookup")) return 1;
    if (d->n_perm_sets) {
        if (!d->perm_product_cosets || !d->perm_cosets || !d->perm_column_kind || !d->perm_column_index || !d->zeta || !d->delta || d->chunk_len == 0 ||
            (uint64_t)d->n_perm_sets * d->chunk_len < d->n_perm_columns) {
            set_error("evaluate_h: malformed permutation description");
            return 1;
        }
        for (uint32_t j = 0; j < d->n_perm_columns; j++) {
            uint32_t kind = d->perm_column_kind[j], idx = d->perm_column_index[j];
            uint32_t lim = kind == H2HIP_ANY_ADVICE ? d->n_advice : kind == H2HIP_ANY_FIXED ? d->n_fixed : kind == H2HIP_ANY_INSTANCE ? d->n_instance : 0;
            if (idx >= lim) {
                set_error("evaluate_h: permutation column %u out of range", j);
                return 1;
            }
        }
    }
    return 0;
}

// The shuffle stage of a call whose description `d` passed evaluate_h_validate: the tables, every graph's indices, and what a shuffle
// graph may read -- not beta, y or the previous value, which no kernel of the stage supplies.  Needs no device.
static int evaluate_h_shuffles_validate(const h2hip_evalh_desc* d, const h2hip_evalh_shuffles* sh) {
    if (!sh || !sh->n_shuffles) return 0;
    if (sh->n_shuffles > 65535) {
        set_error("evaluate_h: %u shuffles > 65535", sh->n_shuffles);
        return 1;
    }
    if (!sh->graphs) {
        set_error("evaluate_h: null shuffle graphs");
        return 1;
    }
    if (check_ptrs("evaluate_h", (const void* const*)sh->product_polys, sh->n_shuffles, "shuffle product_polys")) return 1;
    uint32_t q;
    for (size_t i = 0; i < 2 * (size_t)sh->n_shuffles; i++) {
        if (graph_validate(sh->graphs[i], *d, "shuffle")) return 1;
        if (!graph_reads_only(sh->graphs[i], ~STAGES[ST_SHUFFLE].barred, &q)) {
            set_error("evaluate_h: shuffle graph %zu, calculation %u reads beta, y or the previous value", i, q);
            return 1;
        }
    }
    return 0;
}

// The mv-lookup stage of such a call (h2hip_evalh_mvlookups): the tables, the limits, every graph's indices, and what a graph may read --
// not gamma, y or the previous value.  Needs no device.
static int evaluate_h_mvlookups_validate(const h2hip_evalh_desc* d, const h2hip_evalh_mvlookups* mv) {
    if (!mv || !mv->n_args) return 0;
    if (mv->n_args > 65535) {
        set_error("evaluate_h: %u mv-lookup arguments > 65535", mv->n_args);
        return 1;
    }
    if (!mv->n_inputs || !mv->graphs) {
        set_error("evaluate_h: null mv-lookup n_inputs or graphs");
        return 1;
    }
    if (check_ptrs("evaluate_h", (const void* const*)mv->phi_polys, mv->n_args, "mv-lookup phi_polys") ||
        check_ptrs("evaluate_h", (const void* const*)mv->m_polys, mv->n_args, "mv-lookup m_polys"))
        return 1;
    size_t n_graphs = 0;
    for (uint32_t j = 0; j < mv->n_args; j++) {
        if (mv->n_inputs[j] < 1 || mv->n_inputs[j] > 255) {
            set_error("evaluate_h: mv-lookup n_inputs[%u] = %u, not in [1, 255]", j, mv->n_inputs[j]);
            return 1;
        }
        n_graphs += mv->n_inputs[j] + 1;
    }
    uint32_t q;
    for (size_t i = 0; i < n_graphs; i++) {
        if (graph_validate(mv->graphs[i], *d, "mv-lookup")) return 1;
        if (!graph_reads_only(mv->graphs[i], ~STAGES[ST_MVLOOKUP].barred, &q)) {
            set_error("evaluate_h: mv-lookup graph %zu, calculation %u reads gamma, y or the previous value", i, q);
            return 1;
        }
    }
    return 0;
}

// Everything small the kernels read (programs, constants, rotations, column-pointer tables, challenges, the power table)
// is laid out in one host image of a metadata region at the head of the arena and uploaded with ONE copy before any kernel
// is queued.  A copy from pageable memory is synchronous in HIP and ordered after the stream's earlier work, so a copy
// between two kernels would make the host wait for the first and leave the GPU idle until the second is launched.
struct MetaBlob {
    std::vector<char> host;
    char* dev_base = nullptr;
    size_t cap = 0;
    bool overflow = false;
    template <class T>
    T* put(const T* src, size_t count) {
        size_t off = (host.size() + 255) / 256 * 256;
        const size_t bytes = count * sizeof(T);
        if (off + bytes > cap) {
            overflow = true;
            return (T*)dev_base;
        }
        host.resize(off + bytes);
        if (bytes) memcpy(host.data() + off, src, bytes);
        return (T*)(dev_base + off);
    }
};

// What a call works out before it touches the device: the program of each of its graphs, where that program's slots live, the largest
// global slot workspace among them and what the programs take of the metadata region.  Both forms of evaluate_h and the row-graph
// drivers (lookup compression, the witness check's gates) build one.
struct CallPlan {
    std::vector<const h2hip_graph*> graphs;  // the gates graph first when the call has one, then its further graphs in order
    struct Arg { size_t first, n; };         // an argument's programs: first .. first + n of the plan
    std::vector<Arg> args[N_STAGES];         // evaluate_h: the further graphs are the lookups', the mv-lookups', then the shuffles', argument by argument
    std::vector<Program> progs;
    std::vector<SlotPlan> plans;
    size_t largest = 0;     // the program with the most slots: its plan serves a launch that runs every graph of the call
    size_t slots_ws = 0;    // bytes of the largest global slot workspace
    size_t meta_bytes = 0;  // what progs_put takes of the metadata region
};

static int call_plan(const h2hip_graph* gates, const h2hip_graph* more, size_t n_more, size_t rows, CallPlan* cp,
                     const h2hip_evalh_shuffles* sh = nullptr, const h2hip_evalh_mvlookups* mv = nullptr) {
    if (gates) cp->graphs.push_back(gates);
    auto argument = [&](int stage, const h2hip_graph* g, size_t n) {  // the next n graphs of a stage's table are one argument's
        cp->args[stage].push_back({cp->graphs.size(), n});
        for (size_t i = 0; i < n; i++) cp->graphs.push_back(g + i);
        return g + n;
    };
    for (size_t i = 0; i < n_more; i++) argument(ST_LOOKUP, more + i, 1);
    const h2hip_graph* g = mv ? mv->graphs : nullptr;
    for (uint32_t j = 0; mv && j < mv->n_args; j++) g = argument(ST_MVLOOKUP, g, (size_t)mv->n_inputs[j] + 1);  // the K_j input tuples', then the table's
    if (mv && mv->n_args) cp->meta_bytes += (size_t)(g - mv->graphs) * sizeof(ProgDev) + 256;  // the device table of their programs (mv_progs_put)
    for (uint32_t j = 0; sh && j < sh->n_shuffles; j++) argument(ST_SHUFFLE, sh->graphs + 2 * (size_t)j, 2);  // the input side's, then the shuffle side's
    const size_t count = cp->graphs.size();
    cp->progs.resize(count);
    cp->plans.resize(count);
    for (size_t i = 0; i < count; i++) {
        cp->progs[i] = compile_graph(*cp->graphs[i]);
        if (int rc = slot_plan(cp->progs[i].n_slots, rows, &cp->plans[i])) return rc;
        if (cp->plans[i].ws_bytes > cp->slots_ws) cp->slots_ws = cp->plans[i].ws_bytes;
        if (cp->progs[i].n_slots > cp->progs[cp->largest].n_slots) cp->largest = i;
        cp->meta_bytes += prog_bytes(*cp->graphs[i], cp->progs[i]);
    }
    return 0;
}

// Capacity of the metadata region of an evaluate_h call: the programs, the challenges and scalars, a pointer (and the alignment of its
// table) per column, and `extra_ptrs` pointers in tables of the caller's own
static size_t evalh_meta_cap(const CallPlan& cp, const h2hip_evalh_desc& d, size_t extra_ptrs) {
    return align256(64 * 1024 + cp.meta_bytes + ((size_t)d.n_challenges + 28) * sizeof(Fu) +
                    (8 + 256) * ((size_t)d.n_fixed + d.n_advice + d.n_instance + d.n_perm_sets + 2 * (size_t)d.n_perm_columns + 16) + 8 * extra_ptrs);
}

// the plan's programs into the metadata image, in the plan's order
static std::vector<ProgDev> progs_put(MetaBlob& mb, const CallPlan& cp) {
    std::vector<ProgDev> out(cp.progs.size());
    std::vector<Fu> hc;
    for (size_t i = 0; i < out.size(); i++) {
        const h2hip_graph& g = *cp.graphs[i];
        hc.resize(g.n_constants);
        for (uint32_t j = 0; j < g.n_constants; j++) hc[j] = to_i(fe_from_u64x4(g.constants + 4 * (size_t)j));
        out[i].constants = mb.put(hc.data(), hc.size());
        out[i].rotations = mb.put(g.rotations, g.n_rotations);
        out[i].ops = mb.put(cp.progs[i].ops.data(), cp.progs[i].ops.size());
        out[i].n_ops = (uint32_t)cp.progs[i].ops.size();
        out[i].result = cp.progs[i].result;
    }
    return out;
}

// the mv-lookup programs once more, as the one device table evalh_mvlookup_kernel indexes (nullptr for a call without mv-lookups)
static const ProgDev* mv_progs_put(MetaBlob& mb, const CallPlan& cp, const std::vector<ProgDev>& pds) {
    const std::vector<CallPlan::Arg>& args = cp.args[ST_MVLOOKUP];
    if (args.empty()) return nullptr;
    return mb.put(pds.data() + args.front().first, args.back().first + args.back().n - args.front().first);
}

// The column tables (device pointers, d's counts), d's challenges and its scalars into the metadata image.  Of d only the counts, the
// challenges and y / beta / gamma / theta are read; a scalar no graph of the call can read may be null and stays zero.
static ColsDev cols_put(MetaBlob& mb, const h2hip_evalh_desc& d, const Fe* const* fixed, const Fe* const* advice, const Fe* const* instance,
                        uint32_t log_size, int32_t rot_scale) {
    ColsDev cols;
    cols.fixed = mb.put(fixed, d.n_fixed);
    cols.advice = mb.put(advice, d.n_advice);
    cols.instance = mb.put(instance, d.n_instance);
    std::vector<Fu> hch(d.n_challenges);
    for (uint32_t i = 0; i < d.n_challenges; i++) hch[i] = to_i(fe_from_u64x4(d.challenges + 4 * (size_t)i));
    cols.challenges = mb.put(hch.data(), hch.size());
    auto scalar = [](const uint64_t* v) { return v ? to_i(fe_from_u64x4(v)) : fu_zero(); };
    cols.beta = scalar(d.beta);
    cols.gamma = scalar(d.gamma);
    cols.theta = scalar(d.theta);
    cols.y = scalar(d.y);
    cols.log_size = log_size;
    cols.rot_scale = rot_scale;
    return cols;
}

// The permutation argument's tables and scalars (all zero for a system without one).  fixed / advice / instance are the host copies of
// the tables cols_put stored: a permuted column is one of them, by (kind, index) (:404-408).  z, cosets: n_perm_sets and n_perm_columns
// device pointers; l: l0, l_last, l_active.  delta_start is left to the caller, whose rows decide it.
static PermDev perm_put(MetaBlob& mb, const h2hip_evalh_desc& d, const Fe* const* fixed, const Fe* const* advice, const Fe* const* instance,
                        const Fe* const* z, const Fe* const* cosets, const Fe* const* l, const Fu* pow_lo, const Fu* pow_hi, uint32_t pow_bits) {
    PermDev pd;
    memset(&pd, 0, sizeof(pd));
    if (!d.n_perm_sets) return pd;
    std::vector<const Fe*> pcols(d.n_perm_columns);
    for (uint32_t j = 0; j < d.n_perm_columns; j++) {
        const uint32_t kind = d.perm_column_kind[j], idx = d.perm_column_index[j];
        pcols[j] = kind == H2HIP_ANY_ADVICE ? advice[idx] : kind == H2HIP_ANY_FIXED ? fixed[idx] : instance[idx];
    }
    pd.z = mb.put(z, d.n_perm_sets);
    pd.cols = mb.put(pcols.data(), pcols.size());
    pd.cosets = mb.put(cosets, d.n_perm_columns);
    pd.l0 = l[0];
    pd.l_last = l[1];
    pd.l_active = l[2];
    pd.delta = to_i(fe_from_u64x4(d.delta));
    pd.pow_lo = pow_lo;
    pd.pow_hi = pow_hi;
    pd.pow_bits = pow_bits;
    pd.n_sets = d.n_perm_sets;
    pd.n_cols = d.n_perm_columns;
    pd.chunk_len = d.chunk_len;
    pd.last_rotation = d.last_rotation;
    return pd;
}

// f(std::integral_constant<int, T>, bytes): a slot plan's tier as the interpreter kernels' template argument, with the dynamic LDS
// that tier's slots take
template <class F>
static void with_tier(int tier, F f) {
    switch (tier) {
        case 4: f(std::integral_constant<int, 4>{}, (size_t)4 * 9 * 256 * 4); break;
        case 8: f(std::integral_constant<int, 8>{}, (size_t)8 * 9 * 256 * 4); break;
        case 16: f(std::integral_constant<int, 16>{}, (size_t)EVALH_LDS_HOT * 9 * 256 * 4); break;
        case 64: f(std::integral_constant<int, 64>{}, (size_t)EVALH_LDS_HOT * 9 * 256 * 4); break;
        case 256: f(std::integral_constant<int, 256>{}, (size_t)EVALH_LDS_HOT * 9 * 256 * 4); break;
        default: f(std::integral_constant<int, 0>{}, (size_t)0);
    }
}

static hipFunction_t kernel_for(Ctx* c, GenKind kind, const CallPlan& cp, size_t first, size_t n) {
    return kernel_for(c, gen_unit(kind, cp.graphs.data() + first, cp.progs.data() + first, n));
}
// a generated kernel takes one lane per row: (columns, [the stage's descriptor,] values)
static int launch_generated(hipFunction_t fn, GenKind kind, const ColsDev& cols, const void* stage, Fe* d_values, hipStream_t s) {
    Fe* vals = d_values;
    void* with_stage[] = {(void*)&cols, (void*)stage, (void*)&vals};
    void* without[] = {(void*)&cols, (void*)&vals};
    const size_t rows = (size_t)1 << cols.log_size;
    H2_CHECK(hipModuleLaunchKernel(fn, (uint32_t)((rows + 255) / 256), 1, 1, 256, 1, 1, 0, s, stage ? with_stage : without, nullptr));
    g_rtc_stats.launched(kind, true);
    return 0;
}

// One launch of the custom gates (the plan's first program) over `rows` rows of `values`: the kernel generated for this circuit once
// it is compiled, the interpreter until then (and for programs beyond the generator's limits)
static int enqueue_gates(Ctx* c, const CallPlan& cp, const ProgDev& gd, const ColsDev& cols, Fe* d_values, size_t rows, hipStream_t s) {
    const SlotPlan& plan = cp.plans[0];
    if (hipFunction_t gen = plan.tier != 0 ? kernel_for(c, GEN_GATES, cp, 0, 1) : nullptr) return launch_generated(gen, GEN_GATES, cols, nullptr, d_values, s);
    g_rtc_stats.launched(GEN_GATES, false);
    with_tier(plan.tier, [&](auto tier, size_t lds) {
        hipLaunchKernelGGL(evalh_gates_kernel<decltype(tier)::value>, dim3(plan.lanes / 256), dim3(256), lds, s, gd, cols, d_values,
                           (Fu*)c->evalh_slots.p, plan.lanes);
    });
    H2_CHECK(hipGetLastError());
    return 0;
}

// What a pass reads of the metadata region: the plan's programs (pds, and mv_progs, the device table of the mv-lookups'), the column
// tables, the permutation's, and l0, l_last, l_active
struct PassMeta {
    const std::vector<ProgDev>& pds;
    const ProgDev* mv_progs;
    const ColsDev& cols;
    const PermDev& pd;
    const Fe* const* l;
};

// ... and of one argument of a stage (programs a.first .. a.first + a.n of the plan; z: its cosets, STAGES[stage].cosets of them): the
// kernel generated for its programs where that is wanted (a stage's switch, Tuning::evalh_gen_shuffle / evalh_gen_mvlookup), within the
// generator's limits and compiled; otherwise the interpreter, on the slot plan of the first program with the most slots among them -- its
// tier holds the others' slots too, and its global workspace, if it needs one, is within the call's largest
static int enqueue_argument(Ctx* c, int stage, const CallPlan& cp, CallPlan::Arg a, const PassMeta& m, const Fe* const* z, Fe* d_values,
                            hipStream_t s) {
    const GenKind kind = STAGES[stage].kind;
    const Fe* const* l = m.l;
    union {
        LookupDev lookup;
        MvLookupDev mv;
        ShuffleDev shuffle;
    } dev;  // the stage's descriptor: its cosets, then l0, l_last, l_active
    switch (stage) {
        case ST_LOOKUP: dev.lookup = {z[0], z[1], z[2], l[0], l[1], l[2]}; break;
        case ST_MVLOOKUP: dev.mv = {z[0], z[1], l[0], l[1], l[2]}; break;
        default: dev.shuffle = {z[0], l[0], l[1], l[2]};
    }
    if (hipFunction_t gen = kernel_for(c, kind, cp, a.first, a.n)) return launch_generated(gen, kind, m.cols, &dev, d_values, s);
    g_rtc_stats.launched(kind, false);
    size_t big = a.first;
    for (size_t t = a.first; t < a.first + a.n; t++)
        if (cp.progs[t].n_slots > cp.progs[big].n_slots) big = t;
    const SlotPlan& sp = cp.plans[big];
    const dim3 grid(sp.lanes / 256), block(256);
    Fu* const slots = (Fu*)c->evalh_slots.p;
    const ProgDev* pd = m.pds.data() + a.first;
    switch (stage) {
        case ST_LOOKUP:
            with_tier(sp.tier, [&](auto tier, size_t lds) {
                hipLaunchKernelGGL(evalh_lookup_kernel<decltype(tier)::value>, grid, block, lds, s, pd[0], dev.lookup, m.cols, d_values, slots, sp.lanes);
            });
            break;
        case ST_SHUFFLE:
            with_tier(sp.tier, [&](auto tier, size_t lds) {
                hipLaunchKernelGGL(evalh_shuffle_kernel<decltype(tier)::value>, grid, block, lds, s, pd[0], pd[1], dev.shuffle, m.cols, d_values, slots, sp.lanes);
            });
            break;
        default:  // the kernel indexes the device table: this argument's programs lie where they do among the stage's
            with_tier(sp.tier, [&](auto tier, size_t lds) {
                hipLaunchKernelGGL(evalh_mvlookup_kernel<decltype(tier)::value>, grid, block, lds, s,
                                   m.mv_progs + (a.first - cp.args[ST_MVLOOKUP][0].first), (uint32_t)(a.n - 1), dev.mv, m.cols, d_values, slots, sp.lanes);
            });
    }
    H2_CHECK(hipGetLastError());
    return 0;
}

// arguments of a stage whose cosets are resident at once (a group): as many as Tuning::evalh_lookup_group_bytes hold, at least one
static size_t stage_group(size_t n_args, size_t cosets, size_t col_bytes) {
    if (!n_args) return 0;
    const size_t fit = tune().evalh_lookup_group_bytes / (cosets * col_bytes);
    return n_args <= fit ? n_args : fit ? fit : 1;
}
// a stage's group as a pass sees it: z[cosets * g ..] are the cosets of the group's g-th argument, `group` arguments share the buffers
struct StageBufs {
    const Fe* const* z;
    size_t group;
};

// The constraints of the rows of `values` (2^cols.log_size of them), folded in the reference's order: the custom gates (:334-360), the
// permutation argument (:362-441) when the system has one, the lookups (:443-518), then the mv-lookups (h2hip_evalh_mvlookups) and the
// shuffles (h2hip_evalh_shuffles): the plan's first program, then the arguments of STAGES row by row.  Every column the kernels read is
// in place before the call, but for two kinds the pass asks for when their turn comes: perm_ready() before the permutation kernel is
// queued, and form_group(stage, first, count) before the kernel of argument `first` of a stage when that argument opens a group -- the
// caller then forms the cosets of arguments first .. first + count in the group's buffers, which the kernels of the group before, all
// queued by then, were the last to read.  An eager stage is not asked for its first group: those cosets are there from the start.
template <class PermReady, class FormGroup>
static int constraint_pass(Ctx* c, const CallPlan& cp, const PassMeta& m, const StageBufs (&bufs)[N_STAGES], Fe* d_values, hipStream_t s,
                           PermReady perm_ready, FormGroup form_group) {
    int rc;
    const size_t rows = (size_t)1 << m.cols.log_size;
    int t_g = c->timer_begin("evalh_gates", s);
    if ((rc = enqueue_gates(c, cp, m.pds[0], m.cols, d_values, rows, s))) return rc;
    c->timer_end(t_g, s);
    if (m.pd.n_sets) {
        if ((rc = perm_ready())) return rc;
        int t_p = c->timer_begin("evalh_perm", s);
        hipLaunchKernelGGL(evalh_perm_kernel, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, s, m.pd, m.cols, d_values);
        H2_CHECK(hipGetLastError());
        c->timer_end(t_p, s);
    }
    for (int st = 0; st < N_STAGES; st++) {
        const std::vector<CallPlan::Arg>& args = cp.args[st];
        const bool eager = STAGES[st].eager;
        const size_t group = bufs[st].group;
        int t_pass = eager && !args.empty() ? c->timer_begin(STAGES[st].profile, s) : -1;
        for (size_t j = 0; j < args.size(); j++) {
            const size_t g = j % group;
            if (g == 0 && (j || !eager) && (rc = form_group(st, j, args.size() - j < group ? args.size() - j : group))) return rc;
            int t_arg = eager ? -1 : c->timer_begin(STAGES[st].profile, s);  // the group's transforms are not the argument's own time
            if ((rc = enqueue_argument(c, st, cp, args[j], m, bufs[st].z + STAGES[st].cosets * g, d_values, s))) return rc;
            c->timer_end(t_arg, s);
        }
        c->timer_end(t_pass, s);
    }
    return 0;
}

// The arena every form of evaluate_h allocates behind its metadata region: the columns the engine itself keeps resident and, in the
// host-pointer forms, its copy of `values`.  The call paths size their arena here and h2hip_evaluate_h_workspace_bytes reports it.
//   full form:  columns of 2^ek.  Host: every column of the description, the lookup cosets of one group and `values`; device: only
//               the cosets the call itself forms (advice, instance, one group of lookups).
//   parts form: columns of 2^k.  One part's cosets of EVERY column (the key's too: they arrive as polynomials), one group of lookups
//               and the part's rows of `values`; host: also the coefficient columns, uploaded once, and `values`.
//   Both forms: one product coset per shuffle of a group (h2hip_evalh_shuffles) and two cosets per mv-lookup argument of a group
//               (h2hip_evalh_mvlookups) on top; nothing for a call without them.
// n_args: the arguments of each stage of STAGES.
static int evaluate_h_workspace_bytes(uint32_t k, uint32_t ek, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_perm_sets,
                                      uint32_t n_perm_columns, const size_t (&n_args)[N_STAGES], bool parts, bool dev, size_t* bytes) {
    if (!bytes) {
        set_error("evaluate_h: null argument");
        return 1;
    }
    if (k > ek || ek > 28 || ek - k > 8) {
        set_error("evaluate_h: bad domain (k = %u, extended_k = %u)", k, ek);
        return 1;
    }
    const size_t col_bytes = sizeof(Fe) << ek, part_bytes = align256(sizeof(Fe) << k);
    size_t group_cols = 0, stage_polys = 0;  // the cosets of one group of every stage (reused per group); every argument's polynomials
    for (int st = 0; st < N_STAGES; st++) {
        group_cols += STAGES[st].cosets * stage_group(n_args[st], STAGES[st].cosets, parts ? part_bytes : col_bytes);
        stage_polys += STAGES[st].cosets * n_args[st];
    }
    if (!parts) {
        const size_t n_cols = dev ? (size_t)n_advice + n_instance
                                  : (size_t)n_fixed + n_advice + n_instance + 3 /* l0, l_last, l_active */ + n_perm_sets + n_perm_columns + 1 /* values */;
        *bytes = (n_cols + group_cols) * (col_bytes + 256) + 4096;
        return 0;
    }
    const size_t key_and_witness = (size_t)n_fixed + n_advice + n_instance + 3 + (n_perm_sets ? (size_t)n_perm_sets + n_perm_columns : 0);
    *bytes = (key_and_witness + group_cols + 1 /* the part's rows of values */) * part_bytes;
    if (!dev) *bytes += (key_and_witness + stage_polys) * part_bytes + align256(col_bytes);
    return 0;
}

// polynomial q (of STAGES[stage].cosets) of a stage's argument j, in the order the stage's descriptor holds their cosets.  Of d only the
// lookup tables are read: parts_as_full carries them for the parts form.
static const uint64_t* stage_poly(int stage, size_t j, size_t q, const h2hip_evalh_desc& d, const h2hip_evalh_mvlookups* mv,
                                  const h2hip_evalh_shuffles* sh) {
    switch (stage) {
        case ST_LOOKUP: return (q == 0 ? d.lookup_product_polys : q == 1 ? d.lookup_permuted_input_polys : d.lookup_permuted_table_polys)[j];
        case ST_MVLOOKUP: return (q == 0 ? mv->phi_polys : mv->m_polys)[j];
        default: return sh->product_polys[j];
    }
}

// dev = false: every column pointer in `d` and `values` are host memory (the reference's Vec<F>s); values is updated in place
//              and the call returns when it is.
// dev = true:  the columns and `values` are device memory (extended cosets are used where they lie, the first NTT pass reads
//              coefficient-form polynomials where they lie); the graphs, challenges and scalars stay host pointers; the
//              kernels are queued on `s` and the call returns without waiting for them.
int evaluate_h_host(Ctx* c, const h2hip_evalh_desc* d, const h2hip_evalh_mvlookups* mv, const h2hip_evalh_shuffles* sh, uint64_t* values,
                    bool dev, hipStream_t s) {
    const uint32_t k = d->k, ek = d->extended_k;
    const size_t n = (size_t)1 << k, size = (size_t)1 << ek;
    const size_t col_bytes = size * sizeof(Fe);
    int rc;
    CallPlan cp;  // programs first: their slot counts size the workspaces
    if ((rc = call_plan(&d->custom_gates, d->lookup_graphs, d->n_lookups, size, &cp, sh, mv))) return rc;
    // ---- device arena: [metadata | columns the engine owns]
    // a stage's cosets: buffers for as many of its arguments as 2 GB hold (a group), reused once the kernels of the group before are
    // queued; the first group of the lookups joins the advice / instance batch
    size_t n_args[N_STAGES];
    StageBufs bufs[N_STAGES];
    for (int st = 0; st < N_STAGES; st++) {
        n_args[st] = cp.args[st].size();
        bufs[st].group = stage_group(n_args[st], STAGES[st].cosets, col_bytes);
    }
    size_t arena_bytes;
    if ((rc = evaluate_h_workspace_bytes(k, ek, d->n_fixed, d->n_advice, d->n_instance, d->n_perm_sets, d->n_perm_columns, n_args, false, dev,
                                         &arena_bytes)))
        return rc;
    const size_t meta_cap = evalh_meta_cap(cp, *d, 0);
    if ((rc = c->evalh_ws.ensure(meta_cap + arena_bytes))) return rc;
    if (cp.slots_ws && (rc = c->evalh_slots.ensure(cp.slots_ws))) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    Arena ar;
    ar.base = (char*)c->evalh_ws.p;
    ar.cap = meta_cap + arena_bytes;  // what was asked for, not what the buffer happens to hold: the sizing function is the contract
    MetaBlob mb;
    mb.dev_base = (char*)ar.take(meta_cap);
    mb.cap = meta_cap;
    // ---- where every column will live: an extended coset already in HBM is used in place, anything else gets arena space
    struct Upload { Fe* dst; const uint64_t* src; size_t elems; bool late; };
    std::vector<Upload> uploads;  // host -> device column copies, issued after the metadata; `late`: only the permutation kernel reads it
    bool bad = false, any_late = false;
    auto place = [&](const uint64_t* h, size_t elems, bool late = false) -> Fe* {
        if (!h) {
            bad = true;
            return nullptr;
        }
        if (dev && elems == size) return (Fe*)h;
        if (!dev && elems == size)  // a proving key's constant column the caller pinned (h2hip_columns_pin): already in HBM, fingerprint checked
            if (const Fe* hit = pinned_column_lookup(c, h, elems)) return (Fe*)hit;
        Fe* p = (Fe*)ar.take(col_bytes);
        if (!p) bad = true;
        else if (!dev) {
            uploads.push_back({p, h, elems, late});
            any_late = any_late || late;
        }
        return p;
    };
    std::vector<const Fe*> fixed(d->n_fixed), advice(d->n_advice), instance(d->n_instance);
    for (uint32_t i = 0; i < d->n_fixed; i++) fixed[i] = place(d->fixed_cosets[i], size);
    const size_t n_polys = (size_t)d->n_advice + d->n_instance;
    std::vector<Fe*> poly_dst(n_polys);
    std::vector<const Fe*> poly_src(n_polys, nullptr);
    for (size_t i = 0; i < n_polys; i++) {
        const uint64_t* h = i < d->n_advice ? d->advice_polys[i] : d->instance_polys[i - d->n_advice];
        Fe* p = (Fe*)ar.take(col_bytes);
        if (!p || !h) bad = true;
        if (dev) poly_src[i] = (const Fe*)h;  // the first NTT pass reads the coefficients where they lie
        else uploads.push_back({p, h, n, false});
        poly_dst[i] = p;
        (i < d->n_advice ? advice[i] : instance[i - d->n_advice]) = p;
    }
    const Fe* const l[3] = {place(d->l0, size), place(d->l_last, size), place(d->l_active_row, size)};
    Fe* const d_values = place(values, size);
    std::vector<const Fe*> z(d->n_perm_sets), pcosets(d->n_perm_sets ? d->n_perm_columns : 0);
    for (size_t i = 0; i < z.size(); i++) z[i] = place(d->perm_product_cosets[i], size, true);
    for (size_t j = 0; j < pcosets.size(); j++) pcosets[j] = place(d->perm_cosets[j], size, true);
    std::vector<Fe*> zbuf[N_STAGES];  // one group of each stage's cosets, argument by argument
    for (int st = 0; st < N_STAGES; st++) {
        zbuf[st].assign(STAGES[st].cosets * bufs[st].group, nullptr);
        for (Fe*& p : zbuf[st])
            if (!(p = (Fe*)ar.take(col_bytes))) bad = true;
        bufs[st].z = zbuf[st].data();
        for (size_t q = 0; q < STAGES[st].cosets * n_args[st]; q++)
            if (!stage_poly(st, q / STAGES[st].cosets, q % STAGES[st].cosets, *d, mv, sh)) bad = true;
    }
    if (!mb.dev_base || bad) {
        set_error("evaluate_h: null column or arena overflow");
        return 1;
    }
    // arguments first .. first + count of a stage: their polynomials into the stage's buffers -- queued for the transform in place
    // (device form: read where they lie, srcs says where)
    auto stage_polys = [&](int st, size_t first, size_t count, std::vector<const Fe*>* srcs) -> int {
        const size_t cosets = STAGES[st].cosets;
        for (size_t q = 0; q < cosets * count; q++) {
            const uint64_t* h = stage_poly(st, first + q / cosets, q % cosets, *d, mv, sh);
            srcs->push_back(dev ? (const Fe*)h : nullptr);
            if (!dev) H2_CHECK(hipMemcpyAsync(zbuf[st][q], h, n * sizeof(Fe), hipMemcpyHostToDevice, s));
        }
        return 0;
    };
    // The late uploads (below) go on aux2, which nothing orders after the arena's previous user: ws_acquire made only `s` wait.  What `s`
    // holds now is earlier calls' work and none of this call's; aux2 will wait for that much.
    if (any_late) {
        if ((rc = c->ensure_aux(2))) return rc;
        H2_CHECK(hipEventRecord(c->aux_events[1], s));
    }
    // ---- metadata image
    const ColsDev cols = cols_put(mb, *d, fixed.data(), advice.data(), instance.data(), ek, 1 << (ek - k));
    const std::vector<ProgDev> pds = progs_put(mb, cp);
    const ProgDev* d_mv_progs = mv_progs_put(mb, cp, pds);
    const Fe ext_omega = fe_from_u64x4(d->extended_omega);
    const Fu *pow_lo = nullptr, *pow_hi = nullptr;
    uint32_t pow_bits = 0;
    if (d->n_perm_sets && (rc = ntt_power_table(c, ext_omega, ek, s, &pow_lo, &pow_hi, &pow_bits))) return rc;
    PermDev pd = perm_put(mb, *d, fixed.data(), advice.data(), instance.data(), z.data(), pcosets.data(), l, pow_lo, pow_hi, pow_bits);
    if (d->n_perm_sets) pd.delta_start = to_i(fe_mul<FrP>(fe_from_u64x4(d->beta), fe_from_u64x4(d->zeta)));  // beta * ZETA (:368)
    if (mb.overflow) {
        set_error("evaluate_h: metadata region overflow");
        return 1;
    }
    // ---- upload: the metadata through the pinned ring (or a synchronous copy when large; mb.host dies with this frame), then the
    //      host-pointer form's columns.  The permutation argument's own columns -- the product cosets of this proof, and the key's
    //      permutation cosets when they are not pinned -- cross later, on a second stream under the coset transforms and the gates
    //      kernel: a copy from pageable memory blocks the calling thread, not the kernels already queued.
    if (!mb.host.empty() && (rc = c->stage_h2d(mb.dev_base, mb.host.data(), mb.host.size(), s))) return rc;
    for (const Upload& u : uploads)
        if (!u.late) H2_CHECK(hipMemcpyAsync(u.dst, u.src, u.elems * sizeof(Fe), hipMemcpyHostToDevice, s));
    for (int st = 0; st < N_STAGES; st++) {  // the first group of an eager stage (the lookups) rides in the main batch
        if (!STAGES[st].eager) continue;
        if ((rc = stage_polys(st, 0, bufs[st].group, &poly_src))) return rc;
        poly_dst.insert(poly_dst.end(), zbuf[st].begin(), zbuf[st].end());
    }
    // ---- cosets: advice / instance polynomials -> extended cosets (:306-323) in one batched transform: distribute_powers_zeta(into_coset)
    //      + zero-pad + NTT, as h2hip_coeff_to_extended does
    NttScale sc = NttScale::into_coset(fe_from_u64x4(d->g_coset), fe_from_u64x4(d->g_coset_inv), n);
    int t_c = c->timer_begin("evalh_cosets", s);
    if ((rc = ntt_device_batch(c, poly_dst.data(), poly_src.data(), poly_dst.size(), ext_omega, ek, &sc, s))) return rc;
    c->timer_end(t_c, s);
    // ---- the pass
    auto late_uploads = [&]() -> int {
        if (!any_late) return 0;
        H2_CHECK(hipStreamWaitEvent(c->aux2, c->aux_events[1], 0));
        for (const Upload& u : uploads)
            if (u.late) H2_CHECK(hipMemcpyAsync(u.dst, u.src, u.elems * sizeof(Fe), hipMemcpyHostToDevice, c->aux2));
        H2_CHECK(hipEventRecord(c->aux_events[0], c->aux2));
        H2_CHECK(hipStreamWaitEvent(s, c->aux_events[0], 0));
        return 0;
    };
    auto form_group = [&](int st, size_t first, size_t count) -> int {  // the group's buffers are free: the kernels of the group before are queued
        std::vector<const Fe*> zsrc;
        if (int rc_up = stage_polys(st, first, count, &zsrc)) return rc_up;
        return ntt_device_batch(c, zbuf[st].data(), zsrc.data(), zsrc.size(), ext_omega, ek, &sc, s);
    };
    if ((rc = constraint_pass(c, cp, {pds, d_mv_progs, cols, pd, l}, bufs, d_values, s, late_uploads, form_group))) return rc;
    if ((rc = guard.release())) return rc;
    if (dev) return 0;
    // ---- download
    H2_CHECK(hipMemcpyAsync(values, d_values, col_bytes, hipMemcpyDeviceToHost, s));
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}


// ---- evaluate_h one coset of the 2^k domain at a time (h2hip_evaluate_h_parts_bn254[_device]) ---------------------------------------
// With P = 2^(ek - k), extended row i = j P + p lies at X_i = g_p omega^j, where g_p = zeta extended_omega^p and omega =
// extended_omega^P is the 2^k-th root.  The rows of part p are therefore the size-2^k transform of f(g_p X), and a rotation by r rows of
// the 2^k domain moves (j, p) to (j + r, p): a part is closed under every rotation the constraints use.  The kernels above run on a part
// as they are, with log_size = k and rot_scale = 1 (as lookup_compress runs them), the permutation kernel with the 2^k domain's power
// table and delta_start = beta g_p.  What is new is the scaling f_m -> f_m g_p^m in front of the transform and the gather / scatter
// between a part's 2^k rows and values[j P + p].  Every column arrives as a polynomial of 2^k coefficients, the proving key's too, so the
// engine holds columns of 2^k elements where the full form holds columns of 2^ek.

// One of three kernel-argument constants by a lane-dependent residue, as bit-mask arithmetic (ntt.hip's pick3, where the reason is given)
__device__ __forceinline__ Fu pick3(const Fu (&c)[3], uint32_t m) {
    const int32_t m1 = -(int32_t)(m == 1), m2 = -(int32_t)(m == 2);
    Fu r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = c[0].l[i] ^ ((c[0].l[i] ^ c[1].l[i]) & m1) ^ ((c[0].l[i] ^ c[2].l[i]) & m2);
    return r;
}

struct PartScaleDev {
    const Fe* const* src;        // n_cols coefficient-form columns of 2^log_n elements
    const Fe* const* dst;        // where each goes, scaled (arena columns; written through)
    uint32_t n_cols, log_n, part;
    Fu c3[3];                    // 1, zeta, zeta^2: I-form canonical
    const Fu *pow_lo, *pow_hi;   // the EXTENDED domain's two-level power table (ntt_power_table), I-form canonical
    uint32_t pow_bits;
};
#define EVALH_SCALE_COLS 8  // columns one lane scales with the power it formed

// out_c[m] = f_c[m] g_p^m for the columns of a batch.  g_p^m = zeta^(m mod 3) extended_omega^(p m): zeta is a cube root of one, and
// p m < P 2^k = 2^ek indexes the extended domain's table without a reduction.  The lane of row m forms the power once (two
// multiplications) and spends one more per column.  Data is E-form, the power I-form, and the product leaves canonical, as every NTT
// pass stores it.  Magnitudes: table entries and c3 are canonical, so each fu_mul result lies in [0, 1.01 r) -- fu_mul_canon's
// constant operand.
__global__ void __launch_bounds__(256) evalh_part_scale_kernel(PartScaleDev a) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << a.log_n)) return;
    const uint32_t e = a.part * m;
    Fu g = fu_mul<UF>(a.pow_lo[e & ((1u << a.pow_bits) - 1)], a.pow_hi[e >> a.pow_bits]);
    g = fu_mul<UF>(g, pick3(a.c3, m % 3u));
    const uint32_t c0 = blockIdx.y * EVALH_SCALE_COLS, c1 = c0 + EVALH_SCALE_COLS < a.n_cols ? c0 + EVALH_SCALE_COLS : a.n_cols;
    for (uint32_t col = c0; col < c1; col++) {
        Fe* out = (Fe*)ld_const_col(a.dst, col);
        out[m] = fu_mul_canon<UF>(fu_slice(ld_const_col(a.src, col)[m]), g);
    }
}

// A part's rows of `values` lie 32 P bytes apart: a lane moves one row (two 16-byte accesses), a wave touches 64 consecutive lines (of
// 128 bytes, at P = 4) and a quarter of each.  The other quarters belong to other parts and must stay as they are -- a call may be given a
// range of parts -- so the lines cannot be written whole; the hardware merges the partial writes in L2.
__global__ void __launch_bounds__(256) evalh_part_gather_kernel(const Fe* __restrict__ values, Fe* __restrict__ part, uint32_t log_n,
                                                                uint32_t log_p, uint32_t p) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (1u << log_n)) return;
    part[j] = values[((size_t)j << log_p) + p];
}
// scaled: the rows leave multiplied by t_evaluations[p] (t_i: I-form canonical), which is divide_by_vanishing_poly on this part
__global__ void __launch_bounds__(256) evalh_part_scatter_kernel(const Fe* __restrict__ part, Fe* __restrict__ values, uint32_t log_n,
                                                                 uint32_t log_p, uint32_t p, Fu t_i, int scaled) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (1u << log_n)) return;
    const Fe v = part[j];
    values[((size_t)j << log_p) + p] = scaled ? fu_mul_canon<UF>(fu_slice(v), t_i) : v;
}

// the full form's view of a parts description, for the checks the two share (the graphs, the scalars, the permutation layout); the
// pointers the full form expects as extended cosets carry the polynomials here, and only their presence is looked at
static h2hip_evalh_desc parts_as_full(const h2hip_evalh_parts_desc& d) {
    h2hip_evalh_desc f;
    memset(&f, 0, sizeof(f));
    f.k = d.k, f.extended_k = d.extended_k;
    f.extended_omega = d.extended_omega, f.g_coset = d.g_coset, f.g_coset_inv = d.g_coset_inv;
    f.n_fixed = d.n_fixed, f.n_advice = d.n_advice, f.n_instance = d.n_instance, f.n_challenges = d.n_challenges;
    f.fixed_cosets = d.fixed_polys, f.advice_polys = d.advice_polys, f.instance_polys = d.instance_polys;
    f.challenges = d.challenges;
    f.y = d.y, f.beta = d.beta, f.gamma = d.gamma, f.theta = d.theta;
    f.l0 = d.l0_poly, f.l_last = d.l_last_poly, f.l_active_row = d.l_active_row_poly;
    f.custom_gates = d.custom_gates;
    f.n_perm_sets = d.n_perm_sets, f.n_perm_columns = d.n_perm_columns, f.chunk_len = d.chunk_len, f.last_rotation = d.last_rotation;
    f.perm_product_cosets = d.perm_product_polys, f.perm_column_kind = d.perm_column_kind, f.perm_column_index = d.perm_column_index;
    f.perm_cosets = d.perm_polys;
    f.zeta = d.zeta, f.delta = d.delta;
    f.n_lookups = d.n_lookups, f.lookup_graphs = d.lookup_graphs;
    f.lookup_product_polys = d.lookup_product_polys, f.lookup_permuted_input_polys = d.lookup_permuted_input_polys;
    f.lookup_permuted_table_polys = d.lookup_permuted_table_polys;
    return f;
}

// As evaluate_h_validate, and what only this form can get wrong: a null polynomial in any table (the full form finds those while it
// places its columns; here nothing is placed before the device is in use) and a part range beyond P.  Needs no device.
static int evaluate_h_parts_validate(const h2hip_evalh_parts_desc* d, const void* values) {
    const h2hip_evalh_desc f = parts_as_full(*d);
    if (evaluate_h_validate(&f, values)) return 1;
    const uint32_t P = 1u << (d->extended_k - d->k);
    if ((uint64_t)d->part_begin + d->part_count > P || (d->part_count == 0 && d->part_begin != 0)) {
        set_error("evaluate_h: parts %u .. %u + %u of %u", d->part_begin, d->part_begin, d->part_count, P);
        return 1;
    }
    const struct { const uint64_t* const* tab; size_t count; const char* name; } tabs[] = {
        {d->fixed_polys, d->n_fixed, "fixed_polys"},
        {d->advice_polys, d->n_advice, "advice_polys"},
        {d->instance_polys, d->n_instance, "instance_polys"},
        {d->perm_product_polys, d->n_perm_sets, "perm_product_polys"},
        {d->perm_polys, d->n_perm_sets ? d->n_perm_columns : 0, "perm_polys"},
        {d->lookup_product_polys, d->n_lookups, "lookup_product_polys"},
        {d->lookup_permuted_input_polys, d->n_lookups, "lookup_permuted_input_polys"},
        {d->lookup_permuted_table_polys, d->n_lookups, "lookup_permuted_table_polys"},
    };
    for (const auto& t : tabs)
        if (check_ptrs("evaluate_h", (const void* const*)t.tab, t.count, t.name)) return 1;
    return 0;
}

// ---- pinned part cosets (h2hip_part_cosets_pin below).  The entry of `key` for this domain: part p is the 2^k elements at the result
// + p * 2^k (engine.h, PinCache::lookup: a stale host key is dropped and the call goes on as if nothing were pinned)
static const Fe* part_cosets_lookup(Ctx* c, const void* key, bool dev, const PinDomain& dom) {
    return c->pins.lookup(PinCache::PARTS, key, dev, (size_t)1 << dom.k, dom);
}

// what the last parts call of this thread did (h2hip_debug_evalh_parts_stats): columns scaled and transformed and columns served from
// pins, both summed over the call's parts; column bytes uploaded (host form); arena bytes taken behind the metadata
static thread_local uint64_t g_parts_stats[4];

// dev as in evaluate_h_host.  Host form: every coefficient column that is not pinned crosses once (2^k elements), `values` crosses both
// ways once.  A key polynomial (fixed_polys, the three Lagrange polynomials, perm_polys) whose part cosets are pinned is read, for part p,
// where the pin holds that part: no upload, no scale, no transform, no copy and no arena slot.  Any subset of them may hit.
static int evaluate_h_parts_host(Ctx* c, const h2hip_evalh_parts_desc* d, const h2hip_evalh_mvlookups* mv, const h2hip_evalh_shuffles* sh,
                                 uint64_t* values, bool dev, hipStream_t s) {
    const uint32_t k = d->k, ek = d->extended_k, log_p = ek - k;
    const size_t n = (size_t)1 << k, size = (size_t)1 << ek;
    const size_t part_bytes = align256(n * sizeof(Fe));
    const uint32_t p_begin = d->part_count ? d->part_begin : 0, p_end = d->part_count ? d->part_begin + d->part_count : 1u << log_p;
    const h2hip_evalh_desc f = parts_as_full(*d);  // the counts, the scalars and the permutation layout, where the shared builders read them
    int rc;
    CallPlan cp;
    if ((rc = call_plan(&d->custom_gates, d->lookup_graphs, d->n_lookups, n, &cp, sh, mv))) return rc;
    // ---- the coefficient columns, in the order of the batch that transforms them: key and witness columns, then the lookups'
    std::vector<const uint64_t*> polys;
    for (uint32_t i = 0; i < d->n_fixed; i++) polys.push_back(d->fixed_polys[i]);
    for (uint32_t i = 0; i < d->n_advice; i++) polys.push_back(d->advice_polys[i]);
    for (uint32_t i = 0; i < d->n_instance; i++) polys.push_back(d->instance_polys[i]);
    const size_t at_l0 = polys.size();
    polys.push_back(d->l0_poly), polys.push_back(d->l_last_poly), polys.push_back(d->l_active_row_poly);
    const size_t at_z = polys.size();
    if (d->n_perm_sets) {
        for (uint32_t i = 0; i < d->n_perm_sets; i++) polys.push_back(d->perm_product_polys[i]);
        for (uint32_t j = 0; j < d->n_perm_columns; j++) polys.push_back(d->perm_polys[j]);
    }
    const size_t n_main = polys.size();  // every part transforms these; the stages' polynomials follow, argument by argument, in groups
    size_t n_args[N_STAGES], at_stage[N_STAGES], group[N_STAGES];
    for (int st = 0; st < N_STAGES; st++) {
        n_args[st] = cp.args[st].size();
        at_stage[st] = polys.size();
        for (size_t q = 0; q < STAGES[st].cosets * n_args[st]; q++) polys.push_back(stage_poly(st, q / STAGES[st].cosets, q % STAGES[st].cosets, f, mv, sh));
        group[st] = stage_group(n_args[st], STAGES[st].cosets, part_bytes);
    }
    const Fe ext_omega = fe_from_u64x4(d->extended_omega);
    const Fe omega = fe_pow_u64<FrP>(ext_omega, (uint64_t)1 << log_p);
    const Fe g_coset = fe_from_u64x4(d->g_coset), g_coset_inv = fe_from_u64x4(d->g_coset_inv);
    // ---- the key's polynomials whose part cosets are pinned; the others are `live`: uploaded (host form), scaled and transformed per part
    std::vector<const Fe*> pin(n_main, nullptr);
    {
        PinDomain dom;
        dom.k = k, dom.ek = ek, dom.ext_omega = ext_omega, dom.g_coset = g_coset;
        auto look = [&](size_t i) { pin[i] = part_cosets_lookup(c, polys[i], dev, dom); };
        for (uint32_t i = 0; i < d->n_fixed; i++) look(i);
        for (size_t i = 0; i < 3; i++) look(at_l0 + i);
        if (d->n_perm_sets)
            for (uint32_t j = 0; j < d->n_perm_columns; j++) look(at_z + d->n_perm_sets + j);
    }
    std::vector<size_t> slot(polys.size(), SIZE_MAX);  // polys index -> index among the live columns
    std::vector<const uint64_t*> live;
    size_t n_live_main = 0;
    for (size_t i = 0; i < polys.size(); i++) {
        if (i < n_main && pin[i]) continue;
        slot[i] = live.size();
        live.push_back(polys[i]);
        if (i < n_main) n_live_main++;
    }
    const size_t n_pinned = n_main - n_live_main;
    size_t cols_at[N_STAGES + 1];  // arena columns of one part: the live key and witness columns, then one group of cosets per stage
    cols_at[0] = n_live_main;
    for (int st = 0; st < N_STAGES; st++) cols_at[st + 1] = cols_at[st] + STAGES[st].cosets * group[st];
    const size_t n_first_cols = cols_at[ST_LOOKUP + 1];  // what a part transforms at once: the live columns and the first group of lookups
    const size_t n_part_cols = cols_at[N_STAGES];
    const size_t n_sets = n_pinned ? p_end - p_begin : 1;   // column-pointer tables: one set per part once a pinned column's address depends on it
    // ---- device arena: [metadata | (host form) the live coefficient columns | one part's cosets of them | the part's rows of values |
    //      (host form) values].  h2hip_evaluate_h_workspace_bytes is the upper bound, reached when nothing is pinned: a pinned column takes
    //      neither a coset slot nor, in the host form, a coefficient slot.
    size_t arena_bytes;
    if ((rc = evaluate_h_workspace_bytes(k, ek, d->n_fixed, d->n_advice, d->n_instance, d->n_perm_sets, d->n_perm_columns, n_args, true, dev,
                                         &arena_bytes)))
        return rc;
    arena_bytes -= n_pinned * part_bytes * (dev ? 1 : 2);
    const size_t set_bytes = (8 + 256) * ((size_t)d->n_fixed + d->n_advice + d->n_instance + d->n_perm_sets + 2 * (size_t)d->n_perm_columns + 16) +
                             ((size_t)d->n_challenges + 28) * sizeof(Fu) + 256;
    // this form's own tables: where the live polynomials lie, where a part's cosets go; and the further sets of column tables
    const size_t meta_cap = evalh_meta_cap(cp, f, live.size() + n_part_cols) + align256((n_sets - 1) * set_bytes);
    if ((rc = c->evalh_ws.ensure(meta_cap + arena_bytes))) return rc;
    if (cp.slots_ws && (rc = c->evalh_slots.ensure(cp.slots_ws))) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    Arena ar;
    ar.base = (char*)c->evalh_ws.p;
    ar.cap = meta_cap + arena_bytes;  // what was asked for, not what the buffer happens to hold: the sizing function is the contract
    MetaBlob mb;
    mb.dev_base = (char*)ar.take(meta_cap);
    mb.cap = meta_cap;
    const size_t arena_begin = ar.off;
    std::vector<const Fe*> src(live.size());
    for (size_t i = 0; i < live.size(); i++) src[i] = dev ? (const Fe*)live[i] : (const Fe*)ar.take(part_bytes);
    std::vector<Fe*> part_cols(n_part_cols);
    for (size_t i = 0; i < n_part_cols; i++) part_cols[i] = (Fe*)ar.take(part_bytes);
    Fe* const d_part = (Fe*)ar.take(part_bytes);
    Fe* const d_values = dev ? (Fe*)values : (Fe*)ar.take(size * sizeof(Fe));
    if (!mb.dev_base || !d_part || !d_values || ar.off > ar.cap) {
        set_error("evaluate_h: arena overflow");
        return 1;
    }
    g_parts_stats[0] = g_parts_stats[1] = 0;
    g_parts_stats[2] = dev ? 0 : live.size() * n * sizeof(Fe);
    g_parts_stats[3] = ar.off - arena_begin;
    // ---- the two domains' power tables.  A table handed out by ntt_power_table lives until the twiddle cache is cleared, which only
    // the insertion of a domain the cache does not hold yet can do (ntt.hip, get_twiddles).  So both domains are brought into the cache
    // first -- the second request may clear it, in which case the third puts the extended domain back into a cache of one -- and only
    // then are the pointers kept.  Everything this call transforms afterwards is over (omega, k), a cache hit that inserts nothing, and
    // the context's lock keeps other calls out until this one has queued its last kernel: no kernel queued below can outlive its table.
    PartScaleDev sd;
    memset(&sd, 0, sizeof(sd));
    const Fu *pow_lo, *pow_hi;  // the 2^k domain's, for the permutation kernel
    uint32_t pow_bits;
    if ((rc = ntt_power_table(c, ext_omega, ek, s, &sd.pow_lo, &sd.pow_hi, &sd.pow_bits))) return rc;
    if ((rc = ntt_power_table(c, omega, k, s, &pow_lo, &pow_hi, &pow_bits))) return rc;
    if ((rc = ntt_power_table(c, ext_omega, ek, s, &sd.pow_lo, &sd.pow_hi, &sd.pow_bits))) return rc;
    // ---- metadata image.  A part's cosets in the order of `polys`: a pinned column where the pin holds that part, a live one in its arena
    // slot, which every part reuses; without a pin the one set serves every part
    const Fe* const* d_src = mb.put(src.data(), src.size());
    const Fe* const* d_dst = (const Fe* const*)mb.put(part_cols.data(), part_cols.size());
    std::vector<std::vector<const Fe*>> colp(n_sets, std::vector<const Fe*>(n_main));
    std::vector<ColsDev> cols_p(n_sets);
    std::vector<PermDev> pd_p(n_sets);
    for (size_t t = 0; t < n_sets; t++) {
        const size_t p = p_begin + t;
        for (size_t i = 0; i < n_main; i++) colp[t][i] = pin[i] ? pin[i] + p * n : part_cols[slot[i]];
        const Fe* const* col = colp[t].data();
        const Fe* const* advice = col + d->n_fixed;
        cols_p[t] = cols_put(mb, f, col, advice, advice + d->n_advice, k, 1);
        pd_p[t] = perm_put(mb, f, col, advice, advice + d->n_advice, col + at_z, col + at_z + d->n_perm_sets, col + at_l0, pow_lo, pow_hi, pow_bits);
    }
    const std::vector<ProgDev> pds = progs_put(mb, cp);
    const ProgDev* d_mv_progs = mv_progs_put(mb, cp, pds);
    if (mb.overflow) {
        set_error("evaluate_h: metadata region overflow");
        return 1;
    }
    // ---- upload.  Host form: every live coefficient column and `values` cross once, on `s` like everything else of this call.  Of `values`
    // only the rows of this call's parts cross, in either direction: P rows of consecutive parts are contiguous, so a range of parts is a 2-D copy
    if ((rc = c->stage_h2d(mb.dev_base, mb.host.data(), mb.host.size(), s))) return rc;
    auto copy_values = [&](Fe* dst, const Fe* from, hipMemcpyKind kind) -> int {
        if (p_end - p_begin == 1u << log_p) {
            H2_CHECK(hipMemcpyAsync(dst, from, size * sizeof(Fe), kind, s));
        } else {
            const size_t pitch = sizeof(Fe) << log_p;
            H2_CHECK(hipMemcpy2DAsync(dst + p_begin, pitch, from + p_begin, pitch, (p_end - p_begin) * sizeof(Fe), n, kind, s));
        }
        return 0;
    };
    if (!dev) {
        for (size_t i = 0; i < live.size(); i++) H2_CHECK(hipMemcpyAsync((void*)src[i], live[i], n * sizeof(Fe), hipMemcpyHostToDevice, s));
        if ((rc = copy_values(d_values, (const Fe*)values, hipMemcpyHostToDevice))) return rc;
    }
    sd.log_n = k;
    sd.c3[0] = fu_one_i<UF>();
    sd.c3[1] = to_i(g_coset);
    sd.c3[2] = to_i(g_coset_inv);
    const bool fused = tune().evalh_part_fused;
    std::vector<uint32_t> same_part;
    // live columns first .. first + count -> part_cols[to ..], scaled for part p and transformed over the 2^k domain: the scale kernel and
    // a plain transform, or (Tuning::evalh_part_fused) the transform whose first-pass load scales
    auto to_part = [&](uint32_t p, size_t first, size_t to, size_t count) -> int {
        if (!count) return 0;
        g_parts_stats[0] += count;
        if (fused) {
            same_part.assign(count, p);
            return ntt_part_device_batch(c, part_cols.data() + to, src.data() + first, same_part.data(), count, k, ek, ext_omega, g_coset, g_coset_inv, s);
        }
        sd.src = d_src + first;
        sd.dst = d_dst + to;
        sd.n_cols = (uint32_t)count;
        sd.part = p;
        const dim3 g((uint32_t)((n + 255) / 256), (uint32_t)((count + EVALH_SCALE_COLS - 1) / EVALH_SCALE_COLS));
        int t_s = c->timer_begin("evalh_part_scale", s);
        hipLaunchKernelGGL(evalh_part_scale_kernel, g, dim3(256), 0, s, sd);
        H2_CHECK(hipGetLastError());
        c->timer_end(t_s, s);
        return ntt_device_batch(c, part_cols.data() + to, nullptr, count, omega, k, nullptr, s);
    };
    StageBufs bufs[N_STAGES];  // the stages' groups of cosets are the same arena columns in every part
    for (int st = 0; st < N_STAGES; st++) bufs[st] = {part_cols.data() + cols_at[st], group[st]};
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    const Fe beta_zeta = d->n_perm_sets ? fe_mul<FrP>(fe_from_u64x4(d->beta), fe_from_u64x4(d->zeta)) : fe_zero<FrP>();
    for (uint32_t p = p_begin; p < p_end; p++) {
        const size_t t = n_sets > 1 ? p - p_begin : 0;
        const Fe* const* col = colp[t].data();
        PermDev& pd = pd_p[t];
        g_parts_stats[1] += n_pinned;
        // ---- scale and transform: the part's cosets of the live key and witness columns and of the first group of lookups
        int t_c = c->timer_begin("evalh_cosets", s);
        if ((rc = to_part(p, 0, 0, n_first_cols))) return rc;
        c->timer_end(t_c, s);
        // ---- gather
        int t_io = c->timer_begin("evalh_part_io", s);
        hipLaunchKernelGGL(evalh_part_gather_kernel, grid, block, 0, s, (const Fe*)d_values, d_part, k, log_p, p);
        H2_CHECK(hipGetLastError());
        c->timer_end(t_io, s);
        // ---- the pass, over the part's rows: nothing of the permutation's arrives late here, and a group of a stage's arguments is
        //      scaled and transformed into the stage's buffers as the first group of lookups was
        if (d->n_perm_sets) pd.delta_start = to_i(fe_mul<FrP>(beta_zeta, fe_pow_u64<FrP>(ext_omega, p)));  // beta g_p; the kernel multiplies by omega^j
        if ((rc = constraint_pass(c, cp, {pds, d_mv_progs, cols_p[t], pd, col + at_l0}, bufs, d_part, s, [] { return 0; },
                                  [&](int st, size_t first, size_t count) {  // a stage's live columns lie in the order of its arguments
                                      return to_part(p, slot[at_stage[st]] + STAGES[st].cosets * first, cols_at[st], STAGES[st].cosets * count);
                                  })))
            return rc;
        // ---- scatter
        t_io = c->timer_begin("evalh_part_io", s);
        const Fu t_i = d->t_evaluations ? to_i(fe_from_u64x4(d->t_evaluations + 4 * (size_t)p)) : fu_one_i<UF>();
        hipLaunchKernelGGL(evalh_part_scatter_kernel, grid, block, 0, s, (const Fe*)d_part, d_values, k, log_p, p, t_i, d->t_evaluations ? 1 : 0);
        H2_CHECK(hipGetLastError());
        c->timer_end(t_io, s);
    }
    if ((rc = guard.release())) return rc;
    if (dev) return 0;
    if ((rc = copy_values((Fe*)values, d_values, hipMemcpyDeviceToHost))) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}


// ---- lookup compression (plonk/lookup/prover.rs:90-115): the compressed input / table expressions of commit_permuted over the n
// Lagrange rows.  Each graph is Horner(Constant(0), parts, Theta) over the lookup's expressions (evaluation.py lookup_compress_graphs),
// run by the interpreter above with rot_scale = 1 over the 2^k rows; one launch serves every graph of a call.
template <int MAXI>
__global__ void __launch_bounds__(256) lookup_compress_kernel(const ProgDev* progs, ColsDev c, Fe* const* outs, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    const ProgDev g = progs[blockIdx.y];
    Fe* out = outs[blockIdx.y];
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        const Fu r = prog_eval(g, c, idx, fu_zero(), slots);
        out[idx] = prog_result_e<Slots<MAXI>>(g, c, idx, fe_zero<FrP>(), r);
    }
}

// graphs the interpreter runs over Lagrange rows: `theta`: the compression's graphs may read theta, a gate polynomial's may not
static int row_graphs_validate(const char* what, bool theta, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                               const h2hip_graph* graphs, size_t n_graphs) {
    if (n_graphs && !graphs) {
        set_error("%s: null graphs", what);
        return H2HIP_EINVAL;
    }
    if (n_graphs > 65535) {
        set_error("%s: %zu graphs > 65535", what, n_graphs);
        return H2HIP_EINVAL;
    }
    h2hip_evalh_desc d;
    memset(&d, 0, sizeof(d));
    d.n_fixed = n_fixed;
    d.n_advice = n_advice;
    d.n_instance = n_instance;
    d.n_challenges = n_challenges;
    const uint32_t barred = VS_BIT(BETA) | VS_BIT(GAMMA) | VS_BIT(Y) | VS_BIT(PREVIOUS) | (theta ? 0 : VS_BIT(THETA));
    uint32_t q;
    for (size_t i = 0; i < n_graphs; i++) {
        if (graph_validate(graphs[i], d, theta ? "lookup compression" : "gate check")) return H2HIP_EINVAL;
        if (!graph_reads_only(graphs[i], ~barred, &q)) {
            set_error("%s: graph %zu, calculation %u reads beta, gamma, %sy or the previous value", what, i, q, theta ? "" : "theta, ");
            return H2HIP_EINVAL;
        }
    }
    return 0;
}

int lookup_compress_validate(uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges, const h2hip_graph* graphs,
                             size_t n_graphs) {
    return row_graphs_validate("lookup_compress", true, n_fixed, n_advice, n_instance, n_challenges, graphs, n_graphs);
}

int check_gates_validate(uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges, const h2hip_graph* graphs,
                         size_t n_graphs) {
    return row_graphs_validate("check_gates", false, n_fixed, n_advice, n_instance, n_challenges, graphs, n_graphs);
}

// What the two drivers of row graphs share (the compression below, the witness check's gate loop after it): the graphs compiled, one slot
// plan for the call (the tier of its largest program), programs, column tables, challenges and `tail` (a per-graph table of the caller's, or
// nothing) in one metadata image, one copy, and one launch for every graph -- one per graph in the global-workspace form, whose workspace
// is shared.  launch(tier, grid, lds_bytes, progs, cols, g0, d_tail, gws, lanes) starts the caller's kernel instance of that tier for
// the graphs from g0 on.  The caller holds the workspaces (ws_acquire); this only enqueues on s.  theta may be null (a graph that cannot read it).
template <class Launch>
static int row_graphs_enqueue(Ctx* c, const char* what, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice,
                              uint32_t n_advice, const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                              const uint64_t* theta, const h2hip_graph* graphs, size_t n_graphs, const void* tail, size_t tail_bytes, hipStream_t s,
                              Launch launch) {
    if (n_graphs == 0) return 0;
    CallPlan cp;
    int rc = call_plan(nullptr, graphs, n_graphs, (size_t)1 << k, &cp);
    if (rc) return rc;
    const SlotPlan& plan = cp.plans[cp.largest];
    const size_t meta_cap = align256(4096 + ((size_t)n_challenges + n_fixed + n_advice + n_instance) * sizeof(Fu) + n_graphs * (sizeof(ProgDev) + 512) +
                                     tail_bytes + cp.meta_bytes);
    if ((rc = c->evalh_ws.ensure(meta_cap))) return rc;
    if (cp.slots_ws && (rc = c->evalh_slots.ensure(cp.slots_ws))) return rc;
    MetaBlob mb;
    mb.dev_base = (char*)c->evalh_ws.p;
    mb.cap = meta_cap;
    h2hip_evalh_desc d;  // what cols_put reads: rows are read by graphs that see no y, beta or gamma
    memset(&d, 0, sizeof(d));
    d.n_fixed = n_fixed, d.n_advice = n_advice, d.n_instance = n_instance;
    d.challenges = challenges, d.n_challenges = n_challenges;
    d.theta = theta;
    const ColsDev cols = cols_put(mb, d, fixed, advice, instance, k, 1);
    const std::vector<ProgDev> pd = progs_put(mb, cp);
    const ProgDev* d_progs = mb.put(pd.data(), pd.size());
    const void* d_tail = mb.put((const char*)tail, tail_bytes);
    if (mb.overflow) {
        set_error("%s: metadata region overflow", what);
        return 1;
    }
    if ((rc = c->stage_h2d(mb.dev_base, mb.host.data(), mb.host.size(), s))) return rc;
    // the global-workspace form (a graph with more than 256 live values) shares one workspace: one graph per launch
    const uint32_t per_launch = plan.tier == 0 ? 1u : (uint32_t)n_graphs;
    for (size_t g0 = 0; g0 < n_graphs; g0 += per_launch) {
        with_tier(plan.tier, [&](auto tier, size_t lds) {
            launch(tier, dim3(plan.lanes / 256, per_launch), lds, d_progs + g0, cols, g0, d_tail, (Fu*)c->evalh_slots.p, plan.lanes);
        });
        H2_CHECK(hipGetLastError());
    }
    return 0;
}

// Validated arguments (lookup_compress_validate); columns and outputs are device pointers, the rest host memory.  Enqueued on s.
int lookup_compress_device(Ctx* c, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice, uint32_t n_advice,
                           const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                           const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, Fe* const* out, hipStream_t s) {
    if (n_graphs == 0) return 0;
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    int tm = c->timer_begin("lookup_compress", s);
    rc = row_graphs_enqueue(c, "lookup_compress", k, fixed, n_fixed, advice, n_advice, instance, n_instance, challenges, n_challenges, theta, graphs,
                            n_graphs, out, n_graphs * sizeof(Fe*), s,
                            [&](auto tier, dim3 grid, size_t lds, const ProgDev* p, const ColsDev& cols, size_t g0, const void* d_outs, Fu* gws,
                                uint32_t lanes) {
                                hipLaunchKernelGGL(lookup_compress_kernel<decltype(tier)::value>, grid, dim3(256), lds, s, p, cols,
                                                   (Fe* const*)d_outs + g0, gws, lanes);
                            });
    if (rc) return rc;
    c->timer_end(tm, s);
    return guard.release();
}

// ---- witness check, gates (check.hip; MockProver::verify's gate loop, dev.rs:676-746): graph g is ONE gate polynomial, run by the
// interpreter exactly as the compression above runs its graphs, but the row's exact canonical value never leaves the registers: it is
// tested for zero and goes out as one bit of mask[g][row / 64], a wave's ballot stored by the lane of the word's first row.  lanes is a
// multiple of 256 and 2^k one of 64 (or below 64: one partial wave), so the 64 rows of a word are one wave's in one turn of the loop.
template <int MAXI>
__global__ void __launch_bounds__(256) check_gates_kernel(const ProgDev* progs, ColsDev c, uint64_t* mask, uint32_t words, Fu* gws, uint32_t lanes) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    const ProgDev g = progs[blockIdx.y];
    uint64_t* m = mask + (size_t)blockIdx.y * words;
    Slots<MAXI> slots(gws + tid, lanes);
    for (uint64_t row = tid; row < (1ull << c.log_size); row += lanes) {
        const uint32_t idx = (uint32_t)row;
        const Fu r = prog_eval(g, c, idx, fu_zero(), slots);
        const Fe e = prog_result_e<Slots<MAXI>>(g, c, idx, fe_zero<FrP>(), r);
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) any |= e.l[j];
        const uint64_t bits = __ballot(any != 0);
        if ((idx & 63) == 0) m[idx >> 6] = bits;
    }
}

// Validated arguments (check_gates_validate); columns and d_mask (n_graphs x words 64-bit words, words = max(1, 2^k / 64)) are device
// memory.  The caller holds the workspaces (ws_acquire): this only enqueues on s.
int check_gates_enqueue(Ctx* c, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice, uint32_t n_advice,
                        const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                        const h2hip_graph* graphs, size_t n_graphs, uint64_t* d_mask, uint32_t words, hipStream_t s) {
    return row_graphs_enqueue(c, "check_gates", k, fixed, n_fixed, advice, n_advice, instance, n_instance, challenges, n_challenges, nullptr, graphs,
                              n_graphs, nullptr, 0, s,
                              [&](auto tier, dim3 grid, size_t lds, const ProgDev* p, const ColsDev& cols, size_t g0, const void*, Fu* gws,
                                  uint32_t lanes) {
                                  hipLaunchKernelGGL(check_gates_kernel<decltype(tier)::value>, grid, dim3(256), lds, s, p, cols,
                                                     d_mask + g0 * words, words, gws, lanes);
                              });
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, evaluate_h) ----------------------------------------------------------------------------------------
// The eight calls without _ext are NULL cases of the four with it: one validation, one code path.
int h2hip_evaluate_h_ext_bn254(const h2hip_evalh_desc* desc, const h2hip_evalh_mvlookups* mvlookups, const h2hip_evalh_shuffles* shuffles,
                               uint64_t* values) {
    if (!desc || !values) {
        set_error("evaluate_h: null argument");
        return H2HIP_EINVAL;
    }
    if (evaluate_h_validate(desc, values) || evaluate_h_mvlookups_validate(desc, mvlookups) || evaluate_h_shuffles_validate(desc, shuffles))
        return H2HIP_EINVAL;
    Entry en("h2hip_evaluate_h_bn254");
    if (en.rc) return en.rc;
    return evaluate_h_host(en.c, desc, mvlookups, shuffles, values, false, en.c->stream);
}
int h2hip_evaluate_h_shuffles_bn254(const h2hip_evalh_desc* desc, const h2hip_evalh_shuffles* shuffles, uint64_t* values) {
    return h2hip_evaluate_h_ext_bn254(desc, nullptr, shuffles, values);
}
int h2hip_evaluate_h_bn254(const h2hip_evalh_desc* desc, uint64_t* values) { return h2hip_evaluate_h_ext_bn254(desc, nullptr, nullptr, values); }

int h2hip_evaluate_h_ext_bn254_device(const h2hip_evalh_desc* desc, const h2hip_evalh_mvlookups* mvlookups, const h2hip_evalh_shuffles* shuffles,
                                      void* d_values, void* stream) {
    if (!desc || !d_values) {
        set_error("evaluate_h: null argument");
        return H2HIP_EINVAL;
    }
    if (evaluate_h_validate(desc, d_values) || evaluate_h_mvlookups_validate(desc, mvlookups) || evaluate_h_shuffles_validate(desc, shuffles))
        return H2HIP_EINVAL;
    Entry en("h2hip_evaluate_h_bn254_device", d_values);
    if (en.rc) return en.rc;
    return evaluate_h_host(en.c, desc, mvlookups, shuffles, (uint64_t*)d_values, true, (hipStream_t)stream);
}
int h2hip_evaluate_h_shuffles_bn254_device(const h2hip_evalh_desc* desc, const h2hip_evalh_shuffles* shuffles, void* d_values, void* stream) {
    return h2hip_evaluate_h_ext_bn254_device(desc, nullptr, shuffles, d_values, stream);
}
int h2hip_evaluate_h_bn254_device(const h2hip_evalh_desc* desc, void* d_values, void* stream) {
    return h2hip_evaluate_h_ext_bn254_device(desc, nullptr, nullptr, d_values, stream);
}

// ---- evaluate_h one coset of the 2^k domain at a time ---------------------------------------------------------------------------------
static int parts_extras_validate(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_mvlookups* mvlookups, const h2hip_evalh_shuffles* shuffles) {
    const h2hip_evalh_desc f = parts_as_full(*desc);
    return evaluate_h_mvlookups_validate(&f, mvlookups) || evaluate_h_shuffles_validate(&f, shuffles);
}
int h2hip_evaluate_h_parts_ext_bn254(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_mvlookups* mvlookups,
                                     const h2hip_evalh_shuffles* shuffles, uint64_t* values) {
    if (!desc || !values) {
        set_error("evaluate_h: null argument");
        return H2HIP_EINVAL;
    }
    if (evaluate_h_parts_validate(desc, values) || parts_extras_validate(desc, mvlookups, shuffles)) return H2HIP_EINVAL;
    Entry en("h2hip_evaluate_h_parts_bn254");
    if (en.rc) return en.rc;
    return evaluate_h_parts_host(en.c, desc, mvlookups, shuffles, values, false, en.c->stream);
}
int h2hip_evaluate_h_parts_shuffles_bn254(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_shuffles* shuffles, uint64_t* values) {
    return h2hip_evaluate_h_parts_ext_bn254(desc, nullptr, shuffles, values);
}
int h2hip_evaluate_h_parts_bn254(const h2hip_evalh_parts_desc* desc, uint64_t* values) {
    return h2hip_evaluate_h_parts_ext_bn254(desc, nullptr, nullptr, values);
}

int h2hip_evaluate_h_parts_ext_bn254_device(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_mvlookups* mvlookups,
                                            const h2hip_evalh_shuffles* shuffles, void* d_values, void* stream) {
    if (!desc || !d_values) {
        set_error("evaluate_h: null argument");
        return H2HIP_EINVAL;
    }
    if (evaluate_h_parts_validate(desc, d_values) || parts_extras_validate(desc, mvlookups, shuffles)) return H2HIP_EINVAL;
    Entry en("h2hip_evaluate_h_parts_bn254_device", d_values);
    if (en.rc) return en.rc;
    return evaluate_h_parts_host(en.c, desc, mvlookups, shuffles, (uint64_t*)d_values, true, (hipStream_t)stream);
}
int h2hip_evaluate_h_parts_shuffles_bn254_device(const h2hip_evalh_parts_desc* desc, const h2hip_evalh_shuffles* shuffles, void* d_values,
                                                 void* stream) {
    return h2hip_evaluate_h_parts_ext_bn254_device(desc, nullptr, shuffles, d_values, stream);
}
int h2hip_evaluate_h_parts_bn254_device(const h2hip_evalh_parts_desc* desc, void* d_values, void* stream) {
    return h2hip_evaluate_h_parts_ext_bn254_device(desc, nullptr, nullptr, d_values, stream);
}

int h2hip_evaluate_h_ext_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                         uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, uint32_t n_mvlookups,
                                         uint32_t n_shuffles, int parts_form, int device_form, size_t* bytes) {
    const size_t n_args[N_STAGES] = {n_lookups, n_mvlookups, n_shuffles};  // in the order of STAGES
    return evaluate_h_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_args, parts_form != 0,
                                      device_form != 0, bytes)
               ? H2HIP_EINVAL
               : 0;
}
int h2hip_evaluate_h_shuffles_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                              uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, uint32_t n_shuffles,
                                              int parts_form, int device_form, size_t* bytes) {
    return h2hip_evaluate_h_ext_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_lookups, 0,
                                                n_shuffles, parts_form, device_form, bytes);
}
int h2hip_evaluate_h_workspace_bytes(uint32_t k, uint32_t extended_k, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                                     uint32_t n_perm_sets, uint32_t n_perm_columns, uint32_t n_lookups, int parts_form, int device_form,
                                     size_t* bytes) {
    return h2hip_evaluate_h_shuffles_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_lookups, 0,
                                                     parts_form, device_form, bytes);
}

// ---- pinned part cosets ------------------------------------------------------------------------------------------------------------
// The parts form takes every column as a polynomial of 2^k coefficients and transforms it once per part; a proving key's polynomials are
// the same for every proof.  A pin keeps all P part cosets of such a polynomial in HBM (2^extended_k elements, part-major), built with one
// batched coeff_to_extended_part call per polynomial (its source read P times, P outputs), and evaluate_h_parts_host reads a part where
// the pin holds it.  The budget and its LRU clock are the pinned columns' (HALO2_HIP_COLUMN_CACHE_GB).
static int part_cosets_pin(const void* const* polys, size_t count, uint32_t k, uint32_t ek, const uint64_t* extended_omega, const uint64_t* g_coset,
                           const uint64_t* g_coset_inv, bool dev, hipStream_t stream) {
    if ((count && !polys) || !extended_omega || !g_coset || !g_coset_inv || k > ek || ek > 28 || ek - k > 8) {
        set_error("part_cosets_pin: bad argument");
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < count; i++)
        if (!polys[i]) {
            set_error("part_cosets_pin: null polynomial %zu", i);
            return H2HIP_EINVAL;
        }
    if (check_fr(extended_omega, "extended_omega") || check_fr(g_coset, "g_coset") || check_fr(g_coset_inv, "g_coset_inv")) return H2HIP_EINVAL;
    if (!count) return 0;
    Entry en("h2hip_part_cosets_pin");  // evaluate_h runs on the engine's first device
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = dev ? stream : c->stream;
    const Fe w = fe_from_u64x4(extended_omega), g = fe_from_u64x4(g_coset), gi = fe_from_u64x4(g_coset_inv);
    const size_t n = (size_t)1 << k, P = (size_t)1 << (ek - k), bytes = sizeof(Fe) << ek;
    PinDomain dom;
    dom.k = k, dom.ek = ek, dom.ext_omega = w, dom.g_coset = g;
    for (size_t i = 0; i < count; i++) {
        if (part_cosets_lookup(c, polys[i], dev, dom)) continue;  // already there (and, a host key, still the same array)
        if (Pin* old = c->pins.find(PinCache::PARTS, polys[i])) {  // pinned for another domain: this one replaces it
            H2_CHECK(hipDeviceSynchronize());
            c->pins.drop(old);
        }
        bool fits;
        if (int rc = pinned_make_room(c, bytes, &fits)) return rc;
        if (!fits) continue;  // larger than the whole budget: left unpinned, every call stays correct
        Pin pp;
        pp.kind = PinCache::PARTS, pp.key = polys[i], pp.bytes = bytes, pp.elems = n, pp.device_key = dev, pp.dom = dom;
        if (hipMalloc(&pp.d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("part_cosets_pin: out of device memory after %zu of %zu polynomials (the rest is transformed per call)", i, count);
            return H2HIP_ENOMEM;
        }
        const Fe* src = (const Fe*)polys[i];
        int rc = 0;
        if (!dev) {  // the coefficients cross once, into the transform staging buffer: no output may be the source of the others
            if ((rc = c->ntt_io.ensure(n * sizeof(Fe))) == 0 &&
                hipMemcpyAsync(c->ntt_io.p, polys[i], n * sizeof(Fe), hipMemcpyHostToDevice, s) != hipSuccess) {
                set_error("part_cosets_pin: upload failed");
                rc = H2HIP_EDEVICE;
            }
            src = (const Fe*)c->ntt_io.p;
        }
        std::vector<Fe*> outs(P);
        std::vector<const Fe*> srcs(P, src);
        std::vector<uint32_t> parts(P);
        for (size_t p = 0; p < P; p++) outs[p] = (Fe*)pp.d + p * n, parts[p] = (uint32_t)p;
        if (!rc) rc = ntt_part_device_batch(c, outs.data(), srcs.data(), parts.data(), P, k, ek, w, g, gi, s);
        if (!rc && hipStreamSynchronize(s) != hipSuccess) {  // the staging buffer is free again, and the entry is complete before it is listed
            set_error("part_cosets_pin: building the part cosets failed");
            rc = H2HIP_EDEVICE;
        }
        if (rc) {
            (void)hipDeviceSynchronize();
            c->pins.drop(&pp);
            return rc;
        }
        c->pins.insert(pp);
    }
    return 0;
}

int h2hip_part_cosets_pin(const uint64_t* const* polys, size_t count, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                          const uint64_t g_coset[4], const uint64_t g_coset_inv[4]) {
    return part_cosets_pin((const void* const*)polys, count, k, extended_k, extended_omega, g_coset, g_coset_inv, false, nullptr);
}

int h2hip_part_cosets_pin_device(const void* const* d_polys, size_t count, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                                 const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* stream) {
    return part_cosets_pin(d_polys, count, k, extended_k, extended_omega, g_coset, g_coset_inv, true, (hipStream_t)stream);
}

int h2hip_part_cosets_unpin(const void* const* polys, size_t count) { return pinned_unpin(PinCache::PARTS, polys, count, "h2hip_part_cosets_unpin"); }

int h2hip_part_cosets_pinned_info(size_t* n_polys, size_t* device_bytes) {
    return pinned_info(PinCache::PARTS, n_polys, device_bytes, "h2hip_part_cosets_pinned_info");
}

// test hook: what the last parts call of the calling thread did (g_parts_stats)
int h2hip_debug_evalh_parts_stats(uint64_t out[4]) {
    if (!out) return H2HIP_EINVAL;
    memcpy(out, g_parts_stats, sizeof(g_parts_stats));
    return 0;
}
// A/B hook: 1 = the parts form scales its unpinned columns in the transform's first-pass load, 0 = with evalh_part_scale_kernel (default)
int h2hip_debug_evalh_part_fused(int on) { TuneWrite()->evalh_part_fused = on != 0; return 0; }

int h2hip_debug_evalh_power_table_bits(const uint64_t omega[4], uint32_t log_n, uint32_t* lo_bits) {
    if (!omega || !lo_bits || log_n > 28) {
        set_error("evaluate_h: bad power table query");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_debug_evalh_power_table_bits");
    if (en.rc) return en.rc;
    const Fu *lo, *hi;
    return ntt_power_table(en.c, fe_from_u64x4(omega), log_n, en.c->stream, &lo, &hi, lo_bits);
}
}  // extern "C"
