// C++ test of the mv-lookup mirror (halo2-pse_amd/host/evaluation.hpp plonk::mv_lookup::Argument, Evaluator::mv_lookups, and halo2hip.hpp
// mvlookup_multiplicities / mvlookup_sums / dev::verify).  Needs an MI355X.  tests/test_mvlookup_mirror.py writes the input and compares
// the output with the Python model of tests/mvlookup_util.py.  The system: fixed f, t; advice a, b, c, d; one challenge;
//   prover argument     inputs [a], [b], table [t]                                  (a, b drawn from t: valid)
//   a failing argument  inputs [c], table [t]                                       (for dev::verify)
//   evaluator argument  inputs [a, b * f], [c, d(wX) + challenge_0], table [t, a(w^-1 X)]
//   no gate, no lookup, no permutation, no shuffle: h(X) on entry is `values`
//   usage: test_mvlookup_mirror <in> <out>
//   in (u64 words): k, blinding_factors, max_rows, theta, beta, y, challenge_0 (x 4 each), f, t, a, b, c, d (2^k x 4 each, Lagrange),
//                   l0, l_last, l_active_row (2^k x 4 each, coefficients), blinding (blinding_factors x 4), values (2^extended_k x 4)
//   out (u64 words): required_degree of the evaluator and of the prover argument, F_0, F_1, T, m, phi (2^k x 4 each), the number of
//                    failures, (kind, index, row) per failure, h from evaluate_h, h from evaluate_h_parts (2^extended_k x 4 each)
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
    const Fr theta = fr(), beta = fr(), y = fr(), challenge = fr();
    std::vector<Col> cols;  // f, t, a, b, c, d
    for (int i = 0; i < 6; i++) cols.push_back(Col{frs(n)});
    const std::vector<Fr> l0 = frs(n), l_last = frs(n), l_active = frs(n), blinding = frs(b);
    const poly::EvaluationDomain domain(4, k);
    std::vector<Fr> values = frs(domain.extended_len());

    const Expr f = Expression::fixed(0), t = Expression::fixed(1);
    const mv_lookup::Argument arg{{{Expression::advice(0)}, {Expression::advice(1)}}, {t}};
    const mv_lookup::Argument bad{{{Expression::advice(2)}}, {t}};
    const mv_lookup::Argument arg_ev{{{Expression::advice(0), Expression::advice(1) * f},
                                      {Expression::advice(2), Expression::advice(3, 1) + Expression::challenge(0)}},
                                     {t, Expression::advice(0, -1)}};
    std::vector<uint64_t> out = {arg_ev.required_degree(), arg.required_degree()};
    auto put = [&](const std::vector<Fr>& v) {
        for (const Fr& x : v) out.insert(out.end(), x.l, x.l + 4);
    };
    const std::vector<const Col*> fixed = {&cols[0], &cols[1]}, advice = {&cols[2], &cols[3], &cols[4], &cols[5]};
    const std::vector<Col> comp = arg.compress(domain, fixed, advice, {}, {challenge}, theta);
    for (const Col& c : comp) put(c.values);
    const Col m = arg.commit_multiplicities(domain, comp, b);
    put(m.values);
    const Col phi = arg.commit_sum(domain, comp, m, beta, blinding, b);
    put(phi.values);

    dev::Columns columns;
    columns.fixed = fixed;
    columns.advice = advice;
    columns.challenges = {challenge};
    std::vector<FlatGraph> flat;
    for (const auto& g : arg.compress_graphs()) flat.push_back(g.flatten());
    for (const auto& g : bad.compress_graphs()) flat.push_back(g.flatten());
    std::vector<h2hip_graph> graphs;
    for (const auto& fg : flat) graphs.push_back(fg.abi());
    const auto failures = dev::verify(domain, columns, {}, {}, theta, b, {}, nullptr, max_rows, {}, graphs, {2, 1});
    out.push_back(failures.size());
    for (const auto& fl : failures) {
        out.push_back(uint64_t(fl.kind));
        out.push_back(fl.index);
        out.push_back(fl.row);
    }

    const Evaluator ev = Evaluator::create({}, {}, {}, {arg_ev});
    std::vector<std::vector<Fr>> polys;  // f, t, a, b, c, d, phi, m in coefficient form
    for (const auto& c : cols) polys.push_back(domain.lagrange_to_coeff(c).values);
    polys.push_back(domain.lagrange_to_coeff(phi).values);
    polys.push_back(domain.lagrange_to_coeff(m).values);
    const std::vector<Fr> f_coset = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{polys[0]}).values;
    const std::vector<Fr> t_coset = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{polys[1]}).values;
    const std::vector<Fr> l0_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l0}).values;
    const std::vector<Fr> l_last_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l_last}).values;
    const std::vector<Fr> l_active_c = domain.coeff_to_extended(poly::Polynomial<poly::Coeff>{l_active}).values;
    EvaluateHInputs full;
    EvaluateHPartsInputs parts;
    full.domain = parts.domain = &domain;
    full.fixed_cosets = {&f_coset, &t_coset};
    parts.fixed_polys = {&polys[0], &polys[1]};
    full.advice_polys = parts.advice_polys = {&polys[2], &polys[3], &polys[4], &polys[5]};
    full.challenges = parts.challenges = {challenge};
    full.y = parts.y = y;
    full.beta = parts.beta = beta;
    full.gamma = parts.gamma = Fr::zero();
    full.theta = parts.theta = theta;
    full.l0 = &l0_c, full.l_last = &l_last_c, full.l_active_row = &l_active_c;
    parts.l0_poly = &l0, parts.l_last_poly = &l_last, parts.l_active_row_poly = &l_active;
    full.blinding_factors = parts.blinding_factors = uint32_t(b);
    full.mv_lookups = parts.mv_lookups = {{&polys[6], &polys[7]}};
    std::vector<Fr> h_full = values, h_parts = values;
    ev.evaluate_h(full, h_full);
    ev.evaluate_h_parts(parts, h_parts);
    put(h_full);
    put(h_parts);
    Evaluator::release_key_columns({&f_coset, &t_coset, &l0_c, &l_last_c, &l_active_c});

    // evaluate_h may have started a background compile of the circuit's kernels: join it and release the engine before the process's
    // static destructors run, as tests/cpp/test_evalh_parts_mirror.cpp does
    h2hip_shutdown();
    std::ofstream of(argv[2], std::ios::binary);
    of.write((const char*)out.data(), std::streamsize(out.size() * 8));
    std::printf("mv-lookup mirror: degree %zu, %zu failures at k = %u\n", arg_ev.required_degree(), failures.size(), k);
    return 0;
}
