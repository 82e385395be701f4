// C++ test of the copy-list mirror (halo2-pse_amd/host/halo2hip.hpp: plonk::permutation::keygen::CopyAssembly, keygen_pk's overload for
// it).  Needs an MI355X.  tests/test_permutation_mapping.py writes the input and compares the output with its Python restatement.
//   usage: test_copies_mirror <in> <out>
//   in (u64 words): k, j (EvaluationDomain::new's first argument), blinding_factors, n_perm, n_copies,
//                   copies (left_column, left_row, right_column, right_row each)
//   out: the mapping (n_perm x 2^k x (column, row) as u32), then in Fr columns: permutations, polys (2^k each), cosets (2^extended_k);
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
    const uint32_t k = uint32_t(w.at(at++)), j = uint32_t(w.at(at++));
    const size_t b = w.at(at++), n_perm = w.at(at++), n_copies = w.at(at++), n = size_t(1) << k;
    permutation::keygen::CopyAssembly assembly(n, n_perm);
    for (size_t i = 0; i < n_copies; i++) {
        const size_t lc = w.at(at++), lr = w.at(at++), rc = w.at(at++), rr = w.at(at++);
        assembly.copy(lc, lr, rc, rr);
    }
    bool threw = false;  // Assembly::copy's checks
    try {
        assembly.copy(n_perm, 0, 0, 0);
    } catch (const std::out_of_range&) {
        threw = true;
    }
    try {
        assembly.copy(0, 0, 0, n);
        threw = false;
    } catch (const std::out_of_range&) {
    }
    if (!threw || assembly.copies.size() != 4 * n_copies) {
        std::fprintf(stderr, "CopyAssembly::copy took a cell out of range\n");
        return 1;
    }

    const poly::EvaluationDomain domain(j, k);
    const std::vector<std::vector<Assigned>> fixed(1, std::vector<Assigned>(n, Assigned::trivial(Fr::from(7))));
    const ProvingKeyColumns pk = keygen_pk(domain, fixed, assembly, b);
    poly::kzg::ParamsKZG params;
    const Fr secret = Fr::from(0x5eed0007);
    poly::kzg::ParamsKZG::setup(k, secret, params);
    const permutation::VerifyingKey vk = assembly.build_vk(params, domain);

    std::ofstream out(argv[2], std::ios::binary);
    for (auto& col : assembly.mapping()) out.write((const char*)col.data(), std::streamsize(col.size() * 8));
    auto put = [&](const std::vector<Fr>& v) { out.write((const char*)v.data(), std::streamsize(v.size() * sizeof(Fr))); };
    for (auto& c : pk.permutation.permutations) put(c.values);
    for (auto& c : pk.permutation.polys) put(c.values);
    for (auto& c : pk.permutation.cosets) put(c.values);
    out.write((const char*)vk.commitments.data(), std::streamsize(vk.commitments.size() * sizeof(G1Affine)));
    std::printf("copies mirror: %zu permutation columns, %zu copies at k = %u\n", n_perm, n_copies, k);
    return 0;
}
