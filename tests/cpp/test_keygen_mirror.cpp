// C++ test of the keygen mirror (halo2-pse_amd/host/halo2hip.hpp: plonk::permutation::keygen::Assembly, plonk::batch_invert_assigned,
// plonk::keygen_pk).  Needs an MI355X.  tests/test_keygen.py writes the input and compares the output with its Python restatement.
//   usage: test_keygen_mirror <in> <out>
//   in (u64 words): k, j (EvaluationDomain::new's first argument), blinding_factors, n_perm, n_fixed, n_copies,
//                   copies (left_column, left_row, right_column, right_row each),
//                   per fixed column 2^k cells of (kind, numerator x 4, denominator x 4), kind 0 Zero / 1 Trivial / 2 Rational
//   out: the assembly's mapping (n_perm x 2^k x (column, row) as u32), then in Fr columns: fixed_values, fixed_polys (2^k each),
//        fixed_cosets (2^extended_k), permutations, polys (2^k), cosets (2^extended_k), l0, l_last, l_active_row (2^extended_k);
//        then build_vk's commitments (n_perm affine points)
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::plonk;

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
    const uint32_t k = uint32_t(w.at(at++)), j = uint32_t(w.at(at++));
    const size_t b = w.at(at++), n_perm = w.at(at++), n_fixed = w.at(at++), n_copies = w.at(at++), n = size_t(1) << k;
    permutation::keygen::Assembly assembly(n, n_perm);
    for (size_t i = 0; i < n_copies; i++) {
        const size_t lc = w.at(at++), lr = w.at(at++), rc = w.at(at++), rr = w.at(at++);
        assembly.copy(lc, lr, rc, rr);
    }
    std::vector<std::vector<Assigned>> fixed(n_fixed, std::vector<Assigned>(n));
    for (auto& col : fixed)
        for (auto& cell : col) {
            const uint64_t kind = w.at(at++);
            const Fr num = fr(), den = fr();
            cell = kind == 0 ? Assigned{} : kind == 1 ? Assigned::trivial(num) : Assigned::rational(num, den);
        }

    const poly::EvaluationDomain domain(j, k);
    const ProvingKeyColumns pk = keygen_pk(domain, fixed, assembly, b);
    poly::kzg::ParamsKZG params;
    const Fr secret = Fr::from(0x5eed0007);
    poly::kzg::ParamsKZG::setup(k, secret, params);
    const permutation::VerifyingKey vk = assembly.build_vk(params, domain);

    std::ofstream out(argv[2], std::ios::binary);
    for (auto& col : assembly.mapping) out.write((const char*)col.data(), std::streamsize(col.size() * 8));
    auto put = [&](const std::vector<Fr>& v) { out.write((const char*)v.data(), std::streamsize(v.size() * sizeof(Fr))); };
    for (auto& c : pk.fixed_values) put(c.values);
    for (auto& c : pk.fixed_polys) put(c.values);
    for (auto& c : pk.fixed_cosets) put(c.values);
    for (auto& c : pk.permutation.permutations) put(c.values);
    for (auto& c : pk.permutation.polys) put(c.values);
    for (auto& c : pk.permutation.cosets) put(c.values);
    put(pk.l0.values);
    put(pk.l_last.values);
    put(pk.l_active_row.values);
    out.write((const char*)vk.commitments.data(), std::streamsize(vk.commitments.size() * sizeof(G1Affine)));
    std::printf("keygen mirror: %zu permutation and %zu fixed columns at k = %u\n", n_perm, n_fixed, k);
    return 0;
}
