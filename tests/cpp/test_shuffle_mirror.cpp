// C++ test of the shuffle mirror (halo2-pse_amd/host/evaluation.hpp plonk::shuffle::Argument, Evaluator::shuffles, and halo2hip.hpp
// shuffle_products / dev::verify).  Needs an MI355X.  tests/test_shuffle_mirror.py writes the input and compares the output with the
// Python model of tests/shuffle_util.py.  The system: fixed f; advice a, b, c, d; one challenge;
//   shuffle  input [a, b * f], shuffle [c, d(wX) + challenge_0]
//   no gate, no lookup, no permutation: h(X) on entry is `values`
//   usage: test_shuffle_mirror <in> <out>
//   in (u64 words): k, blinding_factors, max_rows, theta, gamma, y, challenge_0 (x 4 each), f, a, b, c, d (2^k x 4 each, Lagrange),
//                   l0, l_last, l_active_row (2^k x 4 each, coefficients), blinding (blinding_factors x 4), values (2^extended_k x 4)
//   out (u64 words): required_degree, A, S, z (2^k x 4 each), the number of failures, (kind, index, row) per failure,
//                    h from evaluate_h, h from evaluate_h_parts (2^extended_k x 4 each)
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../halo2-pse_amd/host/evaluation.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::plonk;
using Col = poly::Polynomial<poly::LagrangeCoeff>;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    std::vector<uint64_t> w;
    {
        std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
        w.resize(size_t(f.tellg()) / 8);
        f.seekg(0);
        f.read((char*)w.data(), std::streamsize(w.size() * 8));
    }
    size_t at = 0;
    auto fr = [&]() {
        Fr x;
        for (int i = 0; i < 4; i++) x.l[i] = w.at(at++);
        return x;
    };
    auto frs = [&](size_t count) {
        std::vector<Fr> v;
        for (size_t i = 0; i < count; i++) v.push_back(fr());
        return v;
    };
    if (h2hip_init(nullptr, 0) != 0) {
        std::printf("h2hip_init failed: %s\n", h2hip_last_error());
        return 2;
    }
    const uint32_t k = uint32_t(w.at(at++));
    const size_t b = w.at(at++), n = size_t(1) << k;
    const uint32_t max_rows = uint32_t(w.at(at++));
    const Fr theta = fr(), gamma = fr(), y = fr(), challenge = fr();
    std::vector<Col> cols;  // f, a, b, c, d
    for (int i = 0; i < 5; i++) cols.push_back(Col{frs(n)});
    const std::vector<Fr> l0 = frs(n), l_last = frs(n), l_active = frs(n), blinding = frs(b);
    const poly::EvaluationDomain domain(4, k);
    std::vector<Fr> values = frs(domain.extended_len());

    const Expr f = Expression::fixed(0);
    const shuffle::Argument arg{{Expression::advice(0), Expression::advice(1) * f},
                                {Expression::advice(2), Expression::advice(3, 1) + Expression::challenge(0)}};
    std::vector<uint64_t> out = {arg.required_degree()};
    auto put = [&](const std::vector<Fr>& v) {
        for (const Fr& x : v) out.insert(out.end(), x.l, x.l + 4);
    };
    const std::vector<const Col*> fixed = {&cols[0]}, advice = {&cols[1], &cols[2], &cols[3], &cols[4]};
    const auto comp = arg.compress(domain, fixed, advice, {}, {challenge}, theta);
    put(comp.first.values);
    put(comp.second.values);
    const Col z = arg.commit_product(domain, fixed, advice, {}, {challenge}, theta, gamma, blinding, b);
    put(z.values);

    dev::Columns columns;
    columns.fixed = fixed;
    columns.advice = advice;
    columns.challenges = {challenge};
    const auto cg = arg.compress_graphs();
    const FlatGraph fi = cg.first.flatten(), fs = cg.second.flatten();
    const auto failures = dev::verify(domain, columns, {}, {}, theta, b, {}, nullptr, max_rows, {fi.abi(), fs.abi()});
    out.push_back(failures.size());
    for (const auto& fl : failures) {
        out.push_back(uint64_t(fl.kind));
        out.push_back(fl.index);
        out.push_back(fl.row);
    }

    const Evaluator ev = Evaluator::create({}, {}, {arg});
    std::vector<std::vector<Fr>> polys;  // f, a, b, c, d, z in coefficient form
    for (const auto& c : cols) polys.push_back(domain.lagrange_to_coeff(c).values);
    polys.push_back(domain.lagrange_to_coeff(z).values);
    const std::vector<Fr> f_coset = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{polys[0]}).values;
    const std::vector<Fr> l0_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l0}).values;
    const std::vector<Fr> l_last_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l_last}).values;
    const std::vector<Fr> l_active_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l_active}).values;
    EvaluateHInputs full;
    EvaluateHPartsInputs parts;
    full.domain = parts.domain = &domain;
    full.fixed_cosets = {&f_coset};
    parts.fixed_polys = {&polys[0]};
    full.advice_polys = parts.advice_polys = {&polys[1], &polys[2], &polys[3], &polys[4]};
    full.challenges = parts.challenges = {challenge};
    full.y = parts.y = y;
    full.beta = parts.beta = Fr::zero();
    full.gamma = parts.gamma = gamma;
    full.theta = parts.theta = theta;
    full.l0 = &l0_c, full.l_last = &l_last_c, full.l_active_row = &l_active_c;
    parts.l0_poly = &l0, parts.l_last_poly = &l_last, parts.l_active_row_poly = &l_active;
    full.blinding_factors = parts.blinding_factors = uint32_t(b);
    full.shuffles = parts.shuffles = {&polys[5]};
    std::vector<Fr> h_full = values, h_parts = values;
    ev.evaluate_h(full, h_full);
    ev.evaluate_h_parts(parts, h_parts);
    put(h_full);
    put(h_parts);
    Evaluator::release_key_columns({&f_coset, &l0_c, &l_last_c, &l_active_c});

    // evaluate_h may have started a background compile of the circuit's kernels: join it and release the engine before the process's
    // static destructors run, as tests/cpp/test_evalh_parts_mirror.cpp does
    h2hip_shutdown();
    std::ofstream of(argv[2], std::ios::binary);
    of.write((const char*)out.data(), std::streamsize(out.size() * 8));
    std::printf("shuffle mirror: degree %zu, %zu failures at k = %u\n", arg.required_degree(), failures.size(), k);
    return 0;
}
