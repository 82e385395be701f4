// C++ test of the witness-check mirror (halo2-pse_amd/host/halo2hip.hpp dev::verify, with the graphs of evaluation.hpp
// gate_check_graphs / lookup_compress_graphs).  Needs an MI355X.  tests/test_check.py writes the input and compares the output with its
// Python restatement of MockProver::verify's three loops.  The system (tests/check_util.py SYSTEM): fixed s, t; advice a, b, c; instance p;
//   gates   s(X) (a(X) b(wX) - c(w^-1 X)),   s(X) (c(X) - p(X)) challenge_0,   the zero polynomial
//   lookup  input [a], table [t]
//   permutation columns a, b, p with the copies of the input
//   usage: test_check_mirror <in> <out>
//   in (u64 words): k, blinding_factors, max_rows, n_copies, theta (x 4), challenge_0 (x 4), s, t, a, b, c, p (2^k x 4 each),
//                   n_copies x (left column, left row, right column, right row)
//   out (u64 words): the number of failures, then (kind, index, row) per failure in dev::verify's order
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
    const uint32_t k = uint32_t(w.at(at++));
    const size_t b = w.at(at++), n = size_t(1) << k;
    const uint32_t max_rows = uint32_t(w.at(at++));
    const size_t n_copies = w.at(at++);
    const Fr theta = fr(), challenge = fr();
    std::vector<Col> cols(6);  // s, t, a, b, c, p
    for (auto& c : cols)
        for (size_t i = 0; i < n; i++) c.values.push_back(fr());
    permutation::keygen::Assembly assembly(n, 3);
    for (size_t i = 0; i < n_copies; i++, at += 4) assembly.copy(w.at(at), w.at(at + 1), w.at(at + 2), w.at(at + 3));

    const poly::EvaluationDomain domain(3, k);
    const Expr s = Expression::fixed(0), a = Expression::advice(0), c = Expression::advice(2), p = Expression::instance(0);
    const std::vector<Expr> gate_polys = {s * (a * Expression::advice(1, 1) - Expression::advice(2, -1)), (s * (c - p)) * Expression::challenge(0),
                                          nullptr};
    std::vector<FlatGraph> flat_gates, flat_lookups;
    for (const auto& g : gate_check_graphs(gate_polys)) flat_gates.push_back(g.flatten());
    const auto lg = lookup_compress_graphs({{a}, {Expression::fixed(1)}});
    flat_lookups.push_back(lg.first.flatten());
    flat_lookups.push_back(lg.second.flatten());
    std::vector<h2hip_graph> gate_graphs, lookup_graphs;
    for (const auto& f : flat_gates) gate_graphs.push_back(f.abi());
    for (const auto& f : flat_lookups) lookup_graphs.push_back(f.abi());

    dev::Columns columns;
    columns.fixed = {&cols[0], &cols[1]};
    columns.advice = {&cols[2], &cols[3], &cols[4]};
    columns.instance = {&cols[5]};
    columns.challenges = {challenge};
    const std::vector<dev::VerifyFailure> failures =
        dev::verify(domain, columns, gate_graphs, lookup_graphs, theta, b, {&cols[2], &cols[3], &cols[5]}, &assembly, max_rows);

    std::vector<uint64_t> out = {failures.size()};
    for (const auto& f : failures) {
        out.push_back(uint64_t(f.kind));
        out.push_back(f.index);
        out.push_back(f.row);
    }
    std::ofstream of(argv[2], std::ios::binary);
    of.write((const char*)out.data(), std::streamsize(out.size() * 8));
    std::printf("check mirror: %zu failures at k = %u\n", failures.size(), k);
    return 0;
}
