// evaluation.hpp -- C++ host-side mirror of halo2_proofs::plonk::evaluation (plonk/evaluation.rs) over the C ABI.
//
//   plonk::Expression        plonk/circuit.rs Expression<F> (the variants evaluate_h can meet: no Selector, :593)
//   plonk::ValueSource       evaluation.rs:37-60   (same variant order: the derived PartialOrd is (kind, a, b))
//   plonk::Calculation       evaluation.rs:108-127
//   plonk::GraphEvaluator    evaluation.rs:191-201, :526-706  add_rotation / add_constant / add_calculation / add_expression
//   plonk::shuffle::Argument the shuffle argument of upstream PSE halo2 (later than the reference): required_degree, compress, commit_product
//   plonk::mv_lookup::Argument the logUp (mv-lookup) argument of the upstream forks that replaced the permuted-column lookup (later than the
//                            reference): required_degree, compress, commit_multiplicities, commit_sum
//   plonk::Evaluator         evaluation.rs:182-189, new :221-279, evaluate_h :280-522 -> h2hip_evaluate_h_bn254, and coset by coset of the
//                            2^k domain from coefficient-form columns (evaluate_h_parts -> h2hip_evaluate_h_parts_bn254)
//
// The graph builder is a faithful restatement (same deduplication by linear search, same operand ordering and
// constant folding), so the flattened graph has the calculations the reference builds, in the same order.
// There is no CPU evaluation here: evaluate_h hands the flattened description to the engine.
#pragma once
#include <algorithm>
#include <memory>
#include <tuple>

#include "halo2hip.hpp"

namespace halo2_proofs {
namespace plonk {

struct Expression;
using Expr = std::shared_ptr<const Expression>;

struct Expression {
    enum Kind { Constant, Fixed, Advice, Instance, Challenge, Negated, Sum, Product, Scaled };
    Kind kind;
    Fr scalar = Fr::zero();  // Constant value / Scaled factor
    uint32_t index = 0;      // column_index / challenge index
    int32_t rotation = 0;
    Expr a, b;

    static Expr constant(const Fr& v) { return mk(Constant, v, 0, 0, nullptr, nullptr); }
    static Expr fixed(uint32_t column, int32_t rot = 0) { return mk(Fixed, Fr::zero(), column, rot, nullptr, nullptr); }
    static Expr advice(uint32_t column, int32_t rot = 0) { return mk(Advice, Fr::zero(), column, rot, nullptr, nullptr); }
    static Expr instance(uint32_t column, int32_t rot = 0) { return mk(Instance, Fr::zero(), column, rot, nullptr, nullptr); }
    static Expr challenge(uint32_t i) { return mk(Challenge, Fr::zero(), i, 0, nullptr, nullptr); }
    static Expr negated(Expr e) { return mk(Negated, Fr::zero(), 0, 0, std::move(e), nullptr); }
    static Expr sum(Expr x, Expr y) { return mk(Sum, Fr::zero(), 0, 0, std::move(x), std::move(y)); }
    static Expr product(Expr x, Expr y) { return mk(Product, Fr::zero(), 0, 0, std::move(x), std::move(y)); }
    static Expr scaled(Expr e, const Fr& f) { return mk(Scaled, f, 0, 0, std::move(e), nullptr); }

  private:
    static Expr mk(Kind k, const Fr& s, uint32_t i, int32_t r, Expr x, Expr y) {
        auto e = std::make_shared<Expression>();
        e->kind = k;
        e->scalar = s;
        e->index = i;
        e->rotation = r;
        e->a = std::move(x);
        e->b = std::move(y);
        return e;
    }
};
// impl Neg / Add / Sub / Mul for Expression<F> (plonk/circuit.rs): a - b is Sum(a, Negated(b)), e * F is Scaled
inline Expr operator-(const Expr& e) { return Expression::negated(e); }
inline Expr operator+(const Expr& x, const Expr& y) { return Expression::sum(x, y); }
inline Expr operator-(const Expr& x, const Expr& y) { return Expression::sum(x, Expression::negated(y)); }
inline Expr operator*(const Expr& x, const Expr& y) { return Expression::product(x, y); }
inline Expr operator*(const Expr& x, const Fr& f) { return Expression::scaled(x, f); }

// evaluation.rs:37-60; laid out as the ABI's h2hip_value_source
struct ValueSource : h2hip_value_source {
    ValueSource() : h2hip_value_source{H2HIP_VS_CONSTANT, 0, 0} {}
    ValueSource(uint32_t k, uint32_t a_ = 0, uint32_t b_ = 0) : h2hip_value_source{k, a_, b_} {}
    static ValueSource Constant(uint32_t i) { return {H2HIP_VS_CONSTANT, i, 0}; }
    static ValueSource Intermediate(uint32_t i) { return {H2HIP_VS_INTERMEDIATE, i, 0}; }
    static ValueSource Fixed(uint32_t c, uint32_t r) { return {H2HIP_VS_FIXED, c, r}; }
    static ValueSource Advice(uint32_t c, uint32_t r) { return {H2HIP_VS_ADVICE, c, r}; }
    static ValueSource Instance(uint32_t c, uint32_t r) { return {H2HIP_VS_INSTANCE, c, r}; }
    static ValueSource Challenge(uint32_t i) { return {H2HIP_VS_CHALLENGE, i, 0}; }
    static ValueSource Beta() { return {H2HIP_VS_BETA}; }
    static ValueSource Gamma() { return {H2HIP_VS_GAMMA}; }
    static ValueSource Theta() { return {H2HIP_VS_THETA}; }
    static ValueSource Y() { return {H2HIP_VS_Y}; }
    static ValueSource PreviousValue() { return {H2HIP_VS_PREVIOUS}; }
    std::tuple<uint32_t, uint32_t, uint32_t> key() const { return {kind, a, b}; }
    bool operator==(const ValueSource& o) const { return key() == o.key(); }
    bool operator!=(const ValueSource& o) const { return key() != o.key(); }
    bool operator<=(const ValueSource& o) const { return key() <= o.key(); }
};

// evaluation.rs:108-127
struct Calculation {
    uint32_t op = H2HIP_CALC_STORE;  // H2HIP_CALC_*
    ValueSource x, y;                // Horner(start, parts, factor): x = start, y = factor
    std::vector<ValueSource> parts;
    static Calculation Add(ValueSource a, ValueSource b) { return {H2HIP_CALC_ADD, a, b, {}}; }
    static Calculation Sub(ValueSource a, ValueSource b) { return {H2HIP_CALC_SUB, a, b, {}}; }
    static Calculation Mul(ValueSource a, ValueSource b) { return {H2HIP_CALC_MUL, a, b, {}}; }
    static Calculation Square(ValueSource a) { return {H2HIP_CALC_SQUARE, a, {}, {}}; }
    static Calculation Double(ValueSource a) { return {H2HIP_CALC_DOUBLE, a, {}, {}}; }
    static Calculation Negate(ValueSource a) { return {H2HIP_CALC_NEGATE, a, {}, {}}; }
    static Calculation Horner(ValueSource start, std::vector<ValueSource> p, ValueSource factor) { return {H2HIP_CALC_HORNER, start, factor, std::move(p)}; }
    static Calculation Store(ValueSource a) { return {H2HIP_CALC_STORE, a, {}, {}}; }
    bool operator==(const Calculation& o) const { return op == o.op && x == o.x && y == o.y && parts == o.parts; }
};

struct CalculationInfo {  // :213-219
    Calculation calculation;
    uint32_t target;
};

// a GraphEvaluator flattened for the ABI; owns the arrays h2hip_graph points into
struct FlatGraph {
    std::vector<Fr> constants;
    std::vector<int32_t> rotations;
    std::vector<h2hip_calculation> calculations;
    std::vector<h2hip_value_source> parts;
    uint32_t num_intermediates = 0;
    h2hip_graph abi() const {
        h2hip_graph g;
        g.constants = constants.empty() ? nullptr : constants[0].l;
        g.n_constants = (uint32_t)constants.size();
        g.rotations = rotations.data();
        g.n_rotations = (uint32_t)rotations.size();
        g.calculations = calculations.data();
        g.n_calculations = (uint32_t)calculations.size();
        g.parts = parts.data();
        g.n_parts = (uint32_t)parts.size();
        g.num_intermediates = num_intermediates;
        return g;
    }
};

class GraphEvaluator {
  public:
    std::vector<Fr> constants{Fr::zero(), Fr::one(), Fr::from(2)};  // Default, :526-539
    std::vector<int32_t> rotations;
    std::vector<CalculationInfo> calculations;
    uint32_t num_intermediates = 0;

    uint32_t add_rotation(int32_t rotation) {  // :543-552
        for (size_t i = 0; i < rotations.size(); i++)
            if (rotations[i] == rotation) return (uint32_t)i;
        rotations.push_back(rotation);
        return (uint32_t)rotations.size() - 1;
    }
    ValueSource add_constant(const Fr& constant) {  // :555-564
        for (size_t i = 0; i < constants.size(); i++)
            if (constants[i] == constant) return ValueSource::Constant((uint32_t)i);
        constants.push_back(constant);
        return ValueSource::Constant((uint32_t)constants.size() - 1);
    }
    ValueSource add_calculation(const Calculation& calculation) {  // :570-588
        for (const auto& c : calculations)
            if (c.calculation == calculation) return ValueSource::Intermediate(c.target);
        const uint32_t target = num_intermediates;
        calculations.push_back({calculation, target});
        num_intermediates++;
        return ValueSource::Intermediate(target);
    }
    ValueSource add_expression(const Expr& expr) {  // :591-706
        const ValueSource zero = ValueSource::Constant(0), one = ValueSource::Constant(1), two = ValueSource::Constant(2);
        switch (expr->kind) {
            case Expression::Constant: return add_constant(expr->scalar);
            case Expression::Fixed: {
                const uint32_t rot_idx = add_rotation(expr->rotation);
                return add_calculation(Calculation::Store(ValueSource::Fixed(expr->index, rot_idx)));
            }
            case Expression::Advice: {
                const uint32_t rot_idx = add_rotation(expr->rotation);
                return add_calculation(Calculation::Store(ValueSource::Advice(expr->index, rot_idx)));
            }
            case Expression::Instance: {
                const uint32_t rot_idx = add_rotation(expr->rotation);
                return add_calculation(Calculation::Store(ValueSource::Instance(expr->index, rot_idx)));
            }
            case Expression::Challenge: return add_calculation(Calculation::Store(ValueSource::Challenge(expr->index)));
            case Expression::Negated: {
                if (expr->a->kind == Expression::Constant) return add_constant(Fr::zero() - expr->a->scalar);
                const ValueSource result_a = add_expression(expr->a);
                return result_a == zero ? result_a : add_calculation(Calculation::Negate(result_a));
            }
            case Expression::Sum: {
                if (expr->b->kind == Expression::Negated) {  // undo subtraction stored as a + (-b)
                    const ValueSource result_a = add_expression(expr->a);
                    const ValueSource result_b = add_expression(expr->b->a);
                    if (result_a == zero) return add_calculation(Calculation::Negate(result_b));
                    if (result_b == zero) return result_a;
                    return add_calculation(Calculation::Sub(result_a, result_b));
                }
                const ValueSource result_a = add_expression(expr->a);
                const ValueSource result_b = add_expression(expr->b);
                if (result_a == zero) return result_b;
                if (result_b == zero) return result_a;
                return result_a <= result_b ? add_calculation(Calculation::Add(result_a, result_b))
                                            : add_calculation(Calculation::Add(result_b, result_a));
            }
            case Expression::Product: {
                const ValueSource result_a = add_expression(expr->a);
                const ValueSource result_b = add_expression(expr->b);
                if (result_a == zero || result_b == zero) return zero;
                if (result_a == one) return result_b;
                if (result_b == one) return result_a;
                if (result_a == two) return add_calculation(Calculation::Double(result_b));
                if (result_b == two) return add_calculation(Calculation::Double(result_a));
                if (result_a == result_b) return add_calculation(Calculation::Square(result_a));
                return result_a <= result_b ? add_calculation(Calculation::Mul(result_a, result_b))
                                            : add_calculation(Calculation::Mul(result_b, result_a));
            }
            case Expression::Scaled: {
                if (expr->scalar == Fr::zero()) return zero;
                if (expr->scalar == Fr::one()) return add_expression(expr->a);
                const ValueSource cst = add_constant(expr->scalar);
                const ValueSource result_a = add_expression(expr->a);
                return add_calculation(Calculation::Mul(result_a, cst));
            }
        }
        throw std::logic_error("unreachable");  // Expression::Selector => unreachable!() (:593)
    }

    FlatGraph flatten() const {
        FlatGraph f;
        f.constants = constants;
        f.rotations = rotations;
        f.num_intermediates = num_intermediates;
        for (const auto& ci : calculations) {
            h2hip_calculation c;
            c.op = ci.calculation.op;
            c.target = ci.target;
            c.x = ci.calculation.x;
            c.y = ci.calculation.y;
            c.parts_offset = (uint32_t)f.parts.size();
            c.parts_count = (uint32_t)ci.calculation.parts.size();
            for (const auto& p : ci.calculation.parts) f.parts.push_back(p);
            f.calculations.push_back(c);
        }
        return f;
    }
};

// one lookup argument's expressions (plonk/lookup.rs Argument: input_expressions, table_expressions)
struct LookupArgument {
    std::vector<Expr> input_expressions, table_expressions;
};

// Expression::degree (plonk/circuit.rs): a column query counts one, a constant or a challenge nothing
inline size_t expression_degree(const Expr& e) {
    switch (e->kind) {
        case Expression::Constant:
        case Expression::Challenge: return 0;
        case Expression::Fixed:
        case Expression::Advice:
        case Expression::Instance: return 1;
        case Expression::Negated:
        case Expression::Scaled: return expression_degree(e->a);
        case Expression::Sum: return std::max(expression_degree(e->a), expression_degree(e->b));
        case Expression::Product: return expression_degree(e->a) + expression_degree(e->b);
    }
    throw std::logic_error("unreachable");
}

// The shuffle argument of upstream PSE halo2 (plonk/shuffle.rs there; later than the reference, so include/halo2hip.h states the
// definitions): m >= 1 input expressions and as many shuffle expressions.
namespace shuffle {
struct Argument {
    std::vector<Expr> input_expressions, shuffle_expressions;

    // 2 + max(1, the degree of every input expression, of every shuffle expression)
    size_t required_degree() const {
        if (input_expressions.empty() || input_expressions.size() != shuffle_expressions.size())
            throw std::logic_error("shuffle: m >= 1 input expressions and as many shuffle expressions expected");
        size_t d = 1;
        for (const auto& e : input_expressions) d = std::max(d, expression_degree(e));
        for (const auto& e : shuffle_expressions) d = std::max(d, expression_degree(e));
        return 2 + d;
    }

    // one side's graph: add_expression of each expression, Horner(Constant(0), parts, Theta) -- the theta fold lookup_compress_graphs
    // builds for a lookup -- and, for the evaluator, Add(that, Gamma) last
    static GraphEvaluator side_graph(const std::vector<Expr>& expressions, bool add_gamma) {
        GraphEvaluator g;
        std::vector<ValueSource> p;
        for (const auto& e : expressions) p.push_back(g.add_expression(e));
        const ValueSource compressed = g.add_calculation(Calculation::Horner(ValueSource::Constant(0), p, ValueSource::Theta()));
        if (add_gamma) g.add_calculation(Calculation::Add(compressed, ValueSource::Gamma()));
        return g;
    }
    // the compression's two graphs, input side then shuffle side: their values are A and S
    std::pair<GraphEvaluator, GraphEvaluator> compress_graphs() const {
        return {side_graph(input_expressions, false), side_graph(shuffle_expressions, false)};
    }
    // the evaluator's two graphs (h2hip_evalh_shuffles): their values are A + gamma and S + gamma
    std::pair<GraphEvaluator, GraphEvaluator> evaluator_graphs() const {
        return {side_graph(input_expressions, true), side_graph(shuffle_expressions, true)};
    }

    using Col = poly::Polynomial<poly::LagrangeCoeff>;
    // A and S over the n Lagrange rows (h2hip_lookup_compress_bn254)
    std::pair<Col, Col> compress(const poly::EvaluationDomain& domain, const std::vector<const Col*>& fixed, const std::vector<const Col*>& advice,
                                 const std::vector<const Col*>& instance, const std::vector<Fr>& challenges, const Fr& theta) const {
        const auto g = compress_graphs();
        const FlatGraph fi = g.first.flatten(), fs = g.second.flatten();
        auto out = lookup_compress(domain, {fi.abi(), fs.abi()}, fixed, advice, instance, challenges, theta);
        return {std::move(out[0]), std::move(out[1])};
    }

    // commit_product: compress, then the grand product z (h2hip_shuffle_products_bn254) with the caller's blinding_factors blinding
    // values.  Committing z and taking it to coefficient form stay with the caller, as for the lookups' products.
    Col commit_product(const poly::EvaluationDomain& domain, const std::vector<const Col*>& fixed, const std::vector<const Col*>& advice,
                       const std::vector<const Col*>& instance, const std::vector<Fr>& challenges, const Fr& theta, const Fr& gamma,
                       const std::vector<Fr>& blinding, size_t blinding_factors) const {
        const auto c = compress(domain, fixed, advice, instance, challenges, theta);
        return std::move(shuffle_products(domain, {&c.first}, {&c.second}, gamma, blinding, blinding_factors)[0]);
    }
};
}  // namespace shuffle

// The logUp (mv-lookup) argument (include/halo2hip.h states the definitions): K >= 1 input tuples that share one table tuple.
namespace mv_lookup {
struct Argument {
    std::vector<std::vector<Expr>> inputs_expressions;
    std::vector<Expr> table_expressions;

    // 2 + d_t + sum_c d_c: each d the largest degree in that tuple, at least 1
    size_t required_degree() const {
        if (inputs_expressions.empty()) throw std::logic_error("mv_lookup: K >= 1 input tuples expected");
        auto d = [](const std::vector<Expr>& exprs) {
            size_t m = 1;
            for (const auto& e : exprs) m = std::max(m, expression_degree(e));
            return m;
        };
        size_t sum = 2 + d(table_expressions);
        for (const auto& inp : inputs_expressions) sum += d(inp);
        return sum;
    }

    // the compression's K + 1 graphs, inputs then table: their values are F_c and T
    std::vector<GraphEvaluator> compress_graphs() const { return graphs(false); }
    // the evaluator's K + 1 graphs (h2hip_evalh_mvlookups): their values are F_c + beta and T + beta
    std::vector<GraphEvaluator> evaluator_graphs() const { return graphs(true); }

    using Col = poly::Polynomial<poly::LagrangeCoeff>;
    // F_0 .. F_{K-1}, then T, over the n Lagrange rows (h2hip_lookup_compress_bn254)
    std::vector<Col> compress(const poly::EvaluationDomain& domain, const std::vector<const Col*>& fixed, const std::vector<const Col*>& advice,
                              const std::vector<const Col*>& instance, const std::vector<Fr>& challenges, const Fr& theta) const {
        std::vector<FlatGraph> flat;
        for (const auto& g : compress_graphs()) flat.push_back(g.flatten());
        std::vector<h2hip_graph> abi;
        for (const auto& f : flat) abi.push_back(f.abi());
        return lookup_compress(domain, abi, fixed, advice, instance, challenges, theta);
    }
    // the multiplicity column m of compressed columns (compress()'s result): h2hip_mvlookup_multiplicities_bn254.  Committing m stays
    // with the caller.
    Col commit_multiplicities(const poly::EvaluationDomain& domain, const std::vector<Col>& compressed, size_t blinding_factors) const {
        return std::move(mvlookup_multiplicities(domain, {input_ptrs(compressed)}, {&compressed.back()}, blinding_factors)[0]);
    }
    // the grand sum phi (h2hip_mvlookup_sums_bn254) with the caller's blinding_factors blinding values
    Col commit_sum(const poly::EvaluationDomain& domain, const std::vector<Col>& compressed, const Col& m, const Fr& beta,
                   const std::vector<Fr>& blinding, size_t blinding_factors) const {
        return std::move(mvlookup_sums(domain, {input_ptrs(compressed)}, {&compressed.back()}, {&m}, beta, blinding, blinding_factors)[0]);
    }

  private:
    std::vector<GraphEvaluator> graphs(bool add_beta) const {
        if (inputs_expressions.empty()) throw std::logic_error("mv_lookup: K >= 1 input tuples expected");
        std::vector<GraphEvaluator> out;
        for (size_t t = 0; t <= inputs_expressions.size(); t++) {
            const std::vector<Expr>& exprs = t < inputs_expressions.size() ? inputs_expressions[t] : table_expressions;
            GraphEvaluator g;
            std::vector<ValueSource> p;
            for (const auto& e : exprs) p.push_back(g.add_expression(e));
            const ValueSource compressed = g.add_calculation(Calculation::Horner(ValueSource::Constant(0), p, ValueSource::Theta()));
            if (add_beta) g.add_calculation(Calculation::Add(compressed, ValueSource::Beta()));
            out.push_back(std::move(g));
        }
        return out;
    }
    std::vector<const Col*> input_ptrs(const std::vector<Col>& compressed) const {
        if (compressed.size() != inputs_expressions.size() + 1) throw std::logic_error("mv_lookup: K + 1 compressed columns expected");
        std::vector<const Col*> p;
        for (size_t t = 0; t + 1 < compressed.size(); t++) p.push_back(&compressed[t]);
        return p;
    }
};
}  // namespace mv_lookup

// the per-instance inputs of evaluate_h that are not part of the Evaluator (evaluation.rs:280-305): what the reference
// reads from pk, the domain and the prover's committed structures.  Every vector of Fr is one polynomial.
struct EvaluateHInputs {
    const poly::EvaluationDomain* domain = nullptr;
    std::vector<const std::vector<Fr>*> fixed_cosets;                  // pk.fixed_cosets (extended)
    std::vector<const std::vector<Fr>*> advice_polys, instance_polys;  // coefficient form, n each
    std::vector<Fr> challenges;
    Fr y, beta, gamma, theta;
    const std::vector<Fr>*l0 = nullptr, *l_last = nullptr, *l_active_row = nullptr;  // pk.l0 / l_last / l_active_row (extended)
    // permutation (pk.vk.cs.permutation, pk.permutation, permutation::prover::Committed)
    std::vector<std::pair<uint32_t, uint32_t>> permutation_columns;    // (H2HIP_ANY_*, index) of p.columns
    std::vector<const std::vector<Fr>*> permutation_cosets;            // pk.permutation.cosets
    std::vector<const std::vector<Fr>*> permutation_product_cosets;    // sets[i].permutation_product_coset
    uint32_t cs_degree = 3;                                            // chunk_len = cs.degree() - 2 (:364)
    uint32_t blinding_factors = 5;                                     // last_rotation = -(blinding_factors + 1) (:365)
    // lookups (lookup::prover::Committed): product_poly, permuted_input_poly, permuted_table_poly per lookup
    std::vector<std::array<const std::vector<Fr>*, 3>> lookups;
    // shuffles: product_poly per shuffle, coefficient form, n each (one per shuffle of the Evaluator)
    std::vector<const std::vector<Fr>*> shuffles;
    // mv-lookups: (phi_poly, m_poly) per argument of the Evaluator, coefficient form, n each
    std::vector<std::array<const std::vector<Fr>*, 2>> mv_lookups;
};

// evaluate_h_parts' inputs: EvaluateHInputs with every column a polynomial of n coefficients -- pk.fixed_polys, pk.l0 / l_last /
// l_active_row as polynomials, pk.permutation.polys, the product polynomials -- so neither the key nor the engine holds an extended coset
struct EvaluateHPartsInputs {
    const poly::EvaluationDomain* domain = nullptr;
    std::vector<const std::vector<Fr>*> fixed_polys, advice_polys, instance_polys;
    std::vector<Fr> challenges;
    Fr y, beta, gamma, theta;
    const std::vector<Fr>*l0_poly = nullptr, *l_last_poly = nullptr, *l_active_row_poly = nullptr;
    std::vector<std::pair<uint32_t, uint32_t>> permutation_columns;
    std::vector<const std::vector<Fr>*> permutation_polys;             // pk.permutation.polys
    std::vector<const std::vector<Fr>*> permutation_product_polys;     // sets[i].permutation_product_poly
    uint32_t cs_degree = 3;
    uint32_t blinding_factors = 5;
    std::vector<std::array<const std::vector<Fr>*, 3>> lookups;
    std::vector<const std::vector<Fr>*> shuffles;  // product_poly per shuffle
    std::vector<std::array<const std::vector<Fr>*, 2>> mv_lookups;  // (phi_poly, m_poly) per mv-lookup argument
    uint32_t part_begin = 0, part_count = 0;  // the parts (cosets of the 2^k domain) to compute; 0, 0 = all 2^(extended_k - k)
    bool divide_by_vanishing_poly = false;    // the last instance's call: the rows leave multiplied by domain->t_evaluations
};

// commit_permuted's compression (plonk/lookup/prover.rs:90-115) as two graphs, input side then table side: each expression added with
// add_expression, then Horner(Constant(0), parts, Theta) -- Evaluator::create's evaluate_lc on a graph of its own (halo2hip.hpp
// lookup_compress runs them)
inline std::pair<GraphEvaluator, GraphEvaluator> lookup_compress_graphs(const LookupArgument& lookup) {
    auto side = [](const std::vector<Expr>& expressions) {
        GraphEvaluator g;
        std::vector<ValueSource> p;
        for (const auto& e : expressions) p.push_back(g.add_expression(e));
        g.add_calculation(Calculation::Horner(ValueSource::Constant(0), p, ValueSource::Theta()));
        return g;
    };
    return {side(lookup.input_expressions), side(lookup.table_expressions)};
}

// The witness check's graphs (halo2hip.hpp dev::verify, h2hip_check_gates_bn254): one per gate polynomial, add_expression of that
// polynomial alone, its value designated by a closing Store calculation; a null Expr stands for the zero polynomial, an empty graph
inline std::vector<GraphEvaluator> gate_check_graphs(const std::vector<Expr>& gate_polys) {
    std::vector<GraphEvaluator> out;
    for (const auto& poly : gate_polys) {
        GraphEvaluator g;
        if (poly) g.add_calculation(Calculation::Store(g.add_expression(poly)));
        out.push_back(std::move(g));
    }
    return out;
}

class Evaluator {  // :182-189
  public:
    GraphEvaluator custom_gates;
    std::vector<GraphEvaluator> lookups;
    std::vector<std::pair<GraphEvaluator, GraphEvaluator>> shuffles;  // upstream PSE halo2's: input side, shuffle side per shuffle

    // the shuffles' graphs and product polynomials as h2hip_evalh_shuffles; owns what the struct points into
    struct ShufflesAbi {
        std::vector<FlatGraph> flat;
        std::vector<h2hip_graph> graphs;
        std::vector<const uint64_t*> polys;
        h2hip_evalh_shuffles abi;
        const h2hip_evalh_shuffles* ptr() const { return abi.n_shuffles ? &abi : nullptr; }
    };
    void shuffles_abi(const std::vector<const std::vector<Fr>*>& product_polys, size_t n, ShufflesAbi& out) const {
        if (product_polys.size() != shuffles.size()) throw std::logic_error("evaluate_h: one product polynomial per shuffle expected");
        for (size_t j = 0; j < shuffles.size(); j++) {
            if (!product_polys[j] || product_polys[j]->size() != n) throw std::logic_error("evaluate_h: polynomial of the wrong length");
            out.flat.push_back(shuffles[j].first.flatten());
            out.flat.push_back(shuffles[j].second.flatten());
            out.polys.push_back(product_polys[j]->data()->l);
        }
        for (const auto& f : out.flat) out.graphs.push_back(f.abi());
        out.abi.n_shuffles = (uint32_t)shuffles.size();
        out.abi.graphs = out.graphs.data();
        out.abi.product_polys = out.polys.data();
    }

    std::vector<std::vector<GraphEvaluator>> mv_lookups;  // the logUp argument's: K input graphs, then the table graph, per argument

    // the mv-lookups' graphs and polynomials as h2hip_evalh_mvlookups; owns what the struct points into
    struct MvLookupsAbi {
        std::vector<FlatGraph> flat;
        std::vector<h2hip_graph> graphs;
        std::vector<uint32_t> n_inputs;
        std::vector<const uint64_t*> phi, m;
        h2hip_evalh_mvlookups abi;
        const h2hip_evalh_mvlookups* ptr() const { return abi.n_args ? &abi : nullptr; }
    };
    void mv_lookups_abi(const std::vector<std::array<const std::vector<Fr>*, 2>>& polys, size_t n, MvLookupsAbi& out) const {
        if (polys.size() != mv_lookups.size()) throw std::logic_error("evaluate_h: one (phi, m) pair of polynomials per mv-lookup expected");
        for (size_t j = 0; j < mv_lookups.size(); j++) {
            for (const auto* p : polys[j])
                if (!p || p->size() != n) throw std::logic_error("evaluate_h: polynomial of the wrong length");
            for (const auto& g : mv_lookups[j]) out.flat.push_back(g.flatten());
            out.n_inputs.push_back((uint32_t)mv_lookups[j].size() - 1);
            out.phi.push_back(polys[j][0]->data()->l);
            out.m.push_back(polys[j][1]->data()->l);
        }
        for (const auto& f : out.flat) out.graphs.push_back(f.abi());
        out.abi.n_args = (uint32_t)mv_lookups.size();
        out.abi.n_inputs = out.n_inputs.data();
        out.abi.graphs = out.graphs.data();
        out.abi.phi_polys = out.phi.data();
        out.abi.m_polys = out.m.data();
    }

    // Evaluator::new (:221-279): gate_polys = cs.gates.iter().flat_map(|gate| gate.polynomials()), lookups = cs.lookups
    static Evaluator create(const std::vector<Expr>& gate_polys, const std::vector<LookupArgument>& lookup_arguments,
                            const std::vector<shuffle::Argument>& shuffle_arguments = {},
                            const std::vector<mv_lookup::Argument>& mvlookup_arguments = {}) {
        Evaluator ev;
        std::vector<ValueSource> parts;
        for (const auto& poly : gate_polys) parts.push_back(ev.custom_gates.add_expression(poly));
        ev.custom_gates.add_calculation(Calculation::Horner(ValueSource::PreviousValue(), parts, ValueSource::Y()));
        for (const auto& lookup : lookup_arguments) {
            GraphEvaluator graph;
            auto evaluate_lc = [&](const std::vector<Expr>& expressions) {
                std::vector<ValueSource> p;
                for (const auto& e : expressions) p.push_back(graph.add_expression(e));
                return graph.add_calculation(Calculation::Horner(ValueSource::Constant(0), p, ValueSource::Theta()));
            };
            const ValueSource compressed_input_coset = evaluate_lc(lookup.input_expressions);
            const ValueSource compressed_table_coset = evaluate_lc(lookup.table_expressions);
            const ValueSource right_gamma = graph.add_calculation(Calculation::Add(compressed_table_coset, ValueSource::Gamma()));
            const ValueSource lc = graph.add_calculation(Calculation::Add(compressed_input_coset, ValueSource::Beta()));
            graph.add_calculation(Calculation::Mul(lc, right_gamma));
            ev.lookups.push_back(std::move(graph));
        }
        for (const auto& sh : shuffle_arguments) ev.shuffles.push_back(sh.evaluator_graphs());
        for (const auto& mv : mvlookup_arguments) ev.mv_lookups.push_back(mv.evaluator_graphs());
        return ev;
    }

    // evaluate_h for one circuit instance (:280-522): `values` (extended length) is folded in place
    void evaluate_h(const EvaluateHInputs& in, std::vector<Fr>& values) const {
        const poly::EvaluationDomain& d = *in.domain;
        const size_t n = (size_t)1 << d.k, size = d.extended_len();
        auto need = [&](const std::vector<Fr>* v, size_t len) {
            if (!v || v->size() != len) throw std::logic_error("evaluate_h: polynomial of the wrong length");
            return v->data()->l;
        };
        if (values.size() != size || in.lookups.size() != lookups.size() || in.permutation_cosets.size() != in.permutation_columns.size())
            throw std::logic_error("evaluate_h: inconsistent inputs");
        auto table = [&](const std::vector<const std::vector<Fr>*>& cols, size_t len) {
            std::vector<const uint64_t*> t;
            for (auto* c : cols) t.push_back(need(c, len));
            return t;
        };
        const auto fixed = table(in.fixed_cosets, size), advice = table(in.advice_polys, n), instance = table(in.instance_polys, n);
        const auto pcosets = table(in.permutation_cosets, size), pprod = table(in.permutation_product_cosets, size);
        std::vector<uint32_t> pkind, pindex;
        for (auto& c : in.permutation_columns) {
            pkind.push_back(c.first);
            pindex.push_back(c.second);
        }
        const FlatGraph cg = custom_gates.flatten();
        std::vector<FlatGraph> lg;
        std::vector<h2hip_graph> lg_abi;
        std::vector<const uint64_t*> lprod, lpin, lptab;
        for (size_t i = 0; i < lookups.size(); i++) {
            lg.push_back(lookups[i].flatten());
            lprod.push_back(need(in.lookups[i][0], n));
            lpin.push_back(need(in.lookups[i][1], n));
            lptab.push_back(need(in.lookups[i][2], n));
        }
        for (auto& g : lg) lg_abi.push_back(g.abi());
        const Fr zeta = Fr::zeta(), delta = Fr::delta();
        h2hip_evalh_desc desc;
        std::memset(&desc, 0, sizeof(desc));
        desc.k = d.k;
        desc.extended_k = d.extended_k;
        desc.extended_omega = d.extended_omega.l;
        desc.g_coset = d.g_coset.l;
        desc.g_coset_inv = d.g_coset_inv.l;
        desc.n_fixed = (uint32_t)fixed.size();
        desc.n_advice = (uint32_t)advice.size();
        desc.n_instance = (uint32_t)instance.size();
        desc.n_challenges = (uint32_t)in.challenges.size();
        desc.fixed_cosets = fixed.data();
        desc.advice_polys = advice.data();
        desc.instance_polys = instance.data();
        desc.challenges = in.challenges.empty() ? nullptr : in.challenges[0].l;
        desc.y = in.y.l;
        desc.beta = in.beta.l;
        desc.gamma = in.gamma.l;
        desc.theta = in.theta.l;
        desc.l0 = need(in.l0, size);
        desc.l_last = need(in.l_last, size);
        desc.l_active_row = need(in.l_active_row, size);
        desc.custom_gates = cg.abi();
        desc.n_perm_sets = (uint32_t)pprod.size();
        desc.n_perm_columns = (uint32_t)pcosets.size();
        desc.chunk_len = in.cs_degree - 2;
        desc.last_rotation = -(int32_t)(in.blinding_factors + 1);
        desc.perm_product_cosets = pprod.data();
        desc.perm_column_kind = pkind.data();
        desc.perm_column_index = pindex.data();
        desc.perm_cosets = pcosets.data();
        desc.zeta = zeta.l;
        desc.delta = delta.l;
        desc.n_lookups = (uint32_t)lookups.size();
        desc.lookup_graphs = lg_abi.data();
        desc.lookup_product_polys = lprod.data();
        desc.lookup_permuted_input_polys = lpin.data();
        desc.lookup_permuted_table_polys = lptab.data();
        {   // the proving key's constant columns stay in HBM across calls (as halo2hip-sys' try_evaluate_h does; `release_key_columns` below
            // is the counterpart of patch 0006's Drop); a failure only means they are uploaded per call
            std::vector<const uint64_t*> key = fixed;
            key.insert(key.end(), pcosets.begin(), pcosets.end());
            key.push_back(desc.l0);
            key.push_back(desc.l_last);
            key.push_back(desc.l_active_row);
            (void)h2hip_columns_pin(key.data(), key.size(), size);
        }
        ShufflesAbi sh;
        shuffles_abi(in.shuffles, n, sh);
        MvLookupsAbi mv;
        mv_lookups_abi(in.mv_lookups, n, mv);
        engine_check(h2hip_evaluate_h_ext_bn254(&desc, mv.ptr(), sh.ptr(), values[0].l), "h2hip_evaluate_h_bn254");
    }

    // the same one coset of the 2^k domain at a time (h2hip_evaluate_h_parts_bn254): rows of `values` outside the parts asked for are
    // left as they are
    void evaluate_h_parts(const EvaluateHPartsInputs& in, std::vector<Fr>& values) const {
        const poly::EvaluationDomain& d = *in.domain;
        const size_t n = (size_t)1 << d.k, size = d.extended_len();
        auto need = [&](const std::vector<Fr>* v) {
            if (!v || v->size() != n) throw std::logic_error("evaluate_h_parts: polynomial of the wrong length");
            return v->data()->l;
        };
        if (values.size() != size || in.lookups.size() != lookups.size() || in.permutation_polys.size() != in.permutation_columns.size() ||
            (in.divide_by_vanishing_poly && d.t_evaluations.size() != size / n))
            throw std::logic_error("evaluate_h_parts: inconsistent inputs");
        auto table = [&](const std::vector<const std::vector<Fr>*>& cols) {
            std::vector<const uint64_t*> t;
            for (auto* c : cols) t.push_back(need(c));
            return t;
        };
        const auto fixed = table(in.fixed_polys), advice = table(in.advice_polys), instance = table(in.instance_polys);
        const auto ppolys = table(in.permutation_polys), pprod = table(in.permutation_product_polys);
        std::vector<uint32_t> pkind, pindex;
        for (auto& c : in.permutation_columns) {
            pkind.push_back(c.first);
            pindex.push_back(c.second);
        }
        const FlatGraph cg = custom_gates.flatten();
        std::vector<FlatGraph> lg;
        std::vector<h2hip_graph> lg_abi;
        std::vector<const uint64_t*> lprod, lpin, lptab;
        for (size_t i = 0; i < lookups.size(); i++) {
            lg.push_back(lookups[i].flatten());
            lprod.push_back(need(in.lookups[i][0]));
            lpin.push_back(need(in.lookups[i][1]));
            lptab.push_back(need(in.lookups[i][2]));
        }
        for (auto& g : lg) lg_abi.push_back(g.abi());
        const Fr zeta = Fr::zeta(), delta = Fr::delta();
        h2hip_evalh_parts_desc desc;
        std::memset(&desc, 0, sizeof(desc));
        desc.k = d.k;
        desc.extended_k = d.extended_k;
        desc.extended_omega = d.extended_omega.l;
        desc.g_coset = d.g_coset.l;
        desc.g_coset_inv = d.g_coset_inv.l;
        desc.n_fixed = (uint32_t)fixed.size();
        desc.n_advice = (uint32_t)advice.size();
        desc.n_instance = (uint32_t)instance.size();
        desc.n_challenges = (uint32_t)in.challenges.size();
        desc.fixed_polys = fixed.data();
        desc.advice_polys = advice.data();
        desc.instance_polys = instance.data();
        desc.challenges = in.challenges.empty() ? nullptr : in.challenges[0].l;
        desc.y = in.y.l;
        desc.beta = in.beta.l;
        desc.gamma = in.gamma.l;
        desc.theta = in.theta.l;
        desc.l0_poly = need(in.l0_poly);
        desc.l_last_poly = need(in.l_last_poly);
        desc.l_active_row_poly = need(in.l_active_row_poly);
        desc.custom_gates = cg.abi();
        desc.n_perm_sets = (uint32_t)pprod.size();
        desc.n_perm_columns = (uint32_t)ppolys.size();
        desc.chunk_len = in.cs_degree - 2;
        desc.last_rotation = -(int32_t)(in.blinding_factors + 1);
        desc.perm_product_polys = pprod.data();
        desc.perm_column_kind = pkind.data();
        desc.perm_column_index = pindex.data();
        desc.perm_polys = ppolys.data();
        desc.zeta = zeta.l;
        desc.delta = delta.l;
        desc.n_lookups = (uint32_t)lookups.size();
        desc.lookup_graphs = lg_abi.data();
        desc.lookup_product_polys = lprod.data();
        desc.lookup_permuted_input_polys = lpin.data();
        desc.lookup_permuted_table_polys = lptab.data();
        desc.part_begin = in.part_begin;
        desc.part_count = in.part_count;
        desc.t_evaluations = in.divide_by_vanishing_poly ? d.t_evaluations[0].l : nullptr;
        ShufflesAbi sh;
        shuffles_abi(in.shuffles, n, sh);
        MvLookupsAbi mv;
        mv_lookups_abi(in.mv_lookups, n, mv);
        engine_check(h2hip_evaluate_h_parts_ext_bn254(&desc, mv.ptr(), sh.ptr(), values[0].l), "h2hip_evaluate_h_parts_bn254");
    }

    // The part cosets of a proving key's coefficient-form polynomials (fixed_polys, l0 / l_last / l_active_row, permutation.polys) kept in
    // HBM for evaluate_h_parts while this object lives: the pin in the constructor, the unpin in the destructor, so an exception between
    // the two cannot leave entries keyed by freed vectors.  A polynomial the engine does not pin (budget, memory) is transformed per call.
    class PartCosetsPin {
    public:
        template <class Domain>
        PartCosetsPin(const Domain& d, const std::vector<const std::vector<Fr>*>& polys) {
            for (auto* c : polys)
                if (c && c->size() == (size_t(1) << d.k)) ptrs_.push_back((*c)[0].l);
            if (!ptrs_.empty())
                (void)h2hip_part_cosets_pin(ptrs_.data(), ptrs_.size(), d.k, d.extended_k, d.extended_omega.l, d.g_coset.l, d.g_coset_inv.l);
        }
        PartCosetsPin(const PartCosetsPin&) = delete;
        PartCosetsPin& operator=(const PartCosetsPin&) = delete;
        ~PartCosetsPin() {
            if (!ptrs_.empty()) (void)h2hip_part_cosets_unpin((const void* const*)ptrs_.data(), ptrs_.size());
        }

    private:
        std::vector<const uint64_t*> ptrs_;
    };

    // ProvingKey's Drop (patch 0006): release the device copies of the key's constant columns
    static void release_key_columns(const std::vector<const std::vector<Fr>*>& columns) {
        std::vector<const uint64_t*> ptrs;
        for (auto* c : columns)
            if (c && !c->empty()) ptrs.push_back((*c)[0].l);
        if (!ptrs.empty()) (void)h2hip_columns_unpin(ptrs.data(), ptrs.size());
    }
};

}  // namespace plonk
}  // namespace halo2_proofs
