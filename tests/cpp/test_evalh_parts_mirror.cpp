// C++ test of Evaluator::evaluate_h_parts (halo2-pse_amd/host/evaluation.hpp): h(X) evaluated one coset of the 2^k domain at a time from
// coefficient-form columns equals Evaluator::evaluate_h over the extended cosets the domain makes of the same polynomials -- gates,
// permutation argument and a lookup, a second instance folded into the first's values, a range of parts, and the closing
// divide_by_vanishing_poly.  Needs an MI355X; driven by tests/test_evalh_parts.py (which checks both forms against the oracle).
#include <cstdio>
#include <string>

#include "../../halo2-pse_amd/host/evaluation.hpp"
#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::poly;
using namespace halo2_proofs::plonk;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static void test_parts_equal_full(uint32_t j, uint32_t k) {
    EvaluationDomain domain(j, k);
    const size_t n = size_t(1) << k, size = domain.extended_len(), P = size / n;
    auto A = [](uint32_t c, int32_t r = 0) { return Expression::advice(c, r); };
    auto F = [](uint32_t c, int32_t r = 0) { return Expression::fixed(c, r); };
    const std::vector<Expr> gates = {A(0) * F(0) + A(1, 1) * A(2, -1) * F(1) - A(2) * F(2, 2), (A(1) * A(1)) * Fr::from(7) + F(0, -2) * A(0, 2)};
    const std::vector<LookupArgument> lookups = {LookupArgument{{A(0), A(1) * F(1)}, {F(2), F(0, 1)}}};
    Evaluator ev = Evaluator::create(gates, lookups);
    Fr x = Fr::from(5);
    auto next = [&] {
        x = x * x + Fr::from(13);
        return x;
    };
    auto polys = [&](size_t count) {
        std::vector<std::vector<Fr>> out(count, std::vector<Fr>(n));
        for (auto& c : out)
            for (auto& v : c) v = next();
        return out;
    };
    auto cosets = [&](const std::vector<std::vector<Fr>>& ps) {
        std::vector<std::vector<Fr>> out;
        for (auto& c : ps) out.push_back(domain.coeff_to_extended(Polynomial<Coeff>{c}).values);
        return out;
    };
    // fixed 0..2, advice 0..2, l0 / l_last / l_active_row, two permutation sets over three columns, one lookup's three polynomials
    const auto fixed = polys(3), advice = polys(3), ls = polys(3), z = polys(2), sigma = polys(3), lk = polys(3);
    const auto fixed_c = cosets(fixed), ls_c = cosets(ls), z_c = cosets(z), sigma_c = cosets(sigma);
    EvaluateHInputs full;
    EvaluateHPartsInputs parts;
    full.domain = parts.domain = &domain;
    for (size_t i = 0; i < 3; i++) {
        full.fixed_cosets.push_back(&fixed_c[i]);
        parts.fixed_polys.push_back(&fixed[i]);
        full.advice_polys.push_back(&advice[i]);
        parts.advice_polys.push_back(&advice[i]);
        full.permutation_cosets.push_back(&sigma_c[i]);
        parts.permutation_polys.push_back(&sigma[i]);
    }
    full.permutation_columns = parts.permutation_columns = {{H2HIP_ANY_ADVICE, 1}, {H2HIP_ANY_FIXED, 2}, {H2HIP_ANY_ADVICE, 0}};
    for (size_t i = 0; i < 2; i++) {
        full.permutation_product_cosets.push_back(&z_c[i]);
        parts.permutation_product_polys.push_back(&z[i]);
    }
    full.cs_degree = parts.cs_degree = 4;  // chunk_len 2: a ragged second set
    full.blinding_factors = parts.blinding_factors = 5;
    full.y = parts.y = next();
    full.beta = parts.beta = next();
    full.gamma = parts.gamma = next();
    full.theta = parts.theta = next();
    full.l0 = &ls_c[0], full.l_last = &ls_c[1], full.l_active_row = &ls_c[2];
    parts.l0_poly = &ls[0], parts.l_last_poly = &ls[1], parts.l_active_row_poly = &ls[2];
    full.lookups = parts.lookups = {{&lk[0], &lk[1], &lk[2]}};
    std::vector<Fr> start(size);
    for (auto& v : start) v = next();
    // two instances chained through `values`
    std::vector<Fr> want = start, got = start;
    ev.evaluate_h(full, want);
    ev.evaluate_h(full, want);
    ev.evaluate_h_parts(parts, got);
    const std::vector<Fr> after_one = got;
    ev.evaluate_h_parts(parts, got);
    CHECK(got == want);
    // part 0 alone, then the others: together the whole, and part 0's call leaves the other parts' rows alone
    if (P > 1) {
        std::vector<Fr> split = after_one;
        parts.part_begin = 0, parts.part_count = 1;
        ev.evaluate_h_parts(parts, split);
        bool untouched = true;
        for (size_t i = 0; i < size; i++)
            if (i % P != 0) untouched = untouched && split[i] == after_one[i];
        CHECK(untouched);
        parts.part_begin = 1, parts.part_count = (uint32_t)(P - 1);
        ev.evaluate_h_parts(parts, split);
        CHECK(split == want);
        parts.part_begin = parts.part_count = 0;
    }
    // the last instance's call divides by the vanishing polynomial on the way out
    std::vector<Fr> divided = after_one;
    parts.divide_by_vanishing_poly = true;
    ev.evaluate_h_parts(parts, divided);
    Polynomial<ExtendedLagrangeCoeff> h{want};
    CHECK(divided == domain.divide_by_vanishing_poly(h).values);
    Evaluator::release_key_columns({&fixed_c[0], &fixed_c[1], &fixed_c[2], &sigma_c[0], &sigma_c[1], &sigma_c[2], &ls_c[0], &ls_c[1], &ls_c[2]});
}

int main() {
    if (h2hip_init(nullptr, 0) != 0) {
        std::printf("h2hip_init failed: %s\n", h2hip_last_error());
        return 2;
    }
    test_parts_equal_full(3, 5);  // P = 2
    test_parts_equal_full(9, 6);  // P = 8
    h2hip_shutdown();
    std::printf(failures ? "EVALH PARTS MIRROR TESTS FAILED (%d)\n" : "evalh parts mirror tests ok\n", failures);
    return failures ? 1 : 0;
}
