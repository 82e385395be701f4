// C++ test of the lookup mirror (halo2-pse_amd/host/halo2hip.hpp: plonk::lookup_compress / lookup_permute, with the graphs of
// evaluation.hpp lookup_compress_graphs).  Needs an MI355X.  tests/test_lookup_permute.py writes the input and compares the output with
// its Python restatement.  Two lookups: a tuple lookup, input [A0, A1] over table [F0, F1], and a range lookup, input [A2] over table [F2].
//   usage: test_lookup_mirror <in> <out>
//   in (u64 words): k, blinding_factors, theta (x 4), F0, F1, F2, A0, A1, A2 (2^k x 4 each), blinding (2 x 2(b + 1) x 4)
//   out: per lookup the compressed input, the compressed table, A', S' (2^k x 4 each)
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
    const Fr theta = fr();
    std::vector<Col> fixed(3), advice(3);
    for (auto* cols : {&fixed, &advice})
        for (auto& c : *cols)
            for (size_t i = 0; i < n; i++) c.values.push_back(fr());
    std::vector<Fr> blinding;
    for (size_t i = 0; i < 2 * 2 * (b + 1); i++) blinding.push_back(fr());

    const poly::EvaluationDomain domain(3, k);
    const std::vector<LookupArgument> lookups = {
        {{Expression::advice(0), Expression::advice(1)}, {Expression::fixed(0), Expression::fixed(1)}},
        {{Expression::advice(2)}, {Expression::fixed(2)}},
    };
    std::vector<FlatGraph> flat;
    for (const auto& l : lookups) {
        auto g = lookup_compress_graphs(l);
        flat.push_back(g.first.flatten());
        flat.push_back(g.second.flatten());
    }
    std::vector<h2hip_graph> graphs;
    for (const auto& f : flat) graphs.push_back(f.abi());
    const std::vector<Col> comp = lookup_compress(domain, graphs, {&fixed[0], &fixed[1], &fixed[2]}, {&advice[0], &advice[1], &advice[2]}, {}, {}, theta);
    const auto perm = lookup_permute(domain, {&comp[0], &comp[2]}, {&comp[1], &comp[3]}, blinding, b);

    std::ofstream out(argv[2], std::ios::binary);
    for (size_t j = 0; j < lookups.size(); j++)
        for (const Col* c : {&comp[2 * j], &comp[2 * j + 1], &perm[j].first, &perm[j].second})
            out.write((const char*)c->values.data(), std::streamsize(n * sizeof(Fr)));
    std::printf("lookup mirror: 2 lookups at k = %u\n", k);
    return 0;
}
