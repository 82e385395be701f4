// Driver-side program of tests/test_pairing_mirror.py: poly::kzg::{MSMKZG, DualMSM, SingleStrategy, AccumulatorStrategy} and
// pairing (host/kzg.hpp) on term lists the Python driver makes by hand.  Usage: test_pairing_mirror <file> [lincomb_terms]
// The file: u64 nl, u64 nr, then nl + nr terms (32-B Montgomery scalar, 64-B affine point), then g2 and s_g2 (128 raw bytes each).
// Prints the verdict of DualMSM::check, the Gt bytes of e(left, s_g2) e(right, -g2), what SingleStrategy does with the lists and what
// AccumulatorStrategy finalizes after taking them twice.  With lincomb_terms below the lists' lengths both sides go through the
// engine's MSM, which needs a GPU; without it nothing here does.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::poly::kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const size_t lincomb_terms = argc > 2 ? strtoull(argv[2], nullptr, 10) : MSMKZG::LINCOMB_TERMS;
    std::ifstream in(argv[1], std::ios::binary);
    uint64_t counts[2];
    in.read(reinterpret_cast<char*>(counts), 16);
    ParamsKZG params;
    DualMSM dual(params);
    MSMKZG* sides[2] = {&dual.left, &dual.right};
    for (int side = 0; side < 2; side++)
        for (uint64_t i = 0; i < counts[side]; i++) {
            Fr s;
            G1Affine p;
            in.read(reinterpret_cast<char*>(s.l), 32);
            in.read(reinterpret_cast<char*>(p.x), 64);
            sides[side]->append_term(s, p);
        }
    in.read(reinterpret_cast<char*>(params.g2.data()), 128);
    in.read(reinterpret_cast<char*>(params.s_g2.data()), 128);
    if (!in) {
        printf("FAIL: short input\n");
        return 1;
    }
    try {
        printf("check %d\n", dual.check(lincomb_terms) ? 1 : 0);
        const Gt gt = pairing({dual.left.eval(lincomb_terms), dual.right.eval(lincomb_terms)}, {params.s_g2, g2_neg(params.g2)});
        printf("gt");
        for (uint64_t limb : gt) printf(" %016llx", (unsigned long long)limb);
        printf("\n");
        const auto opening = [&](DualMSM acc) {
            acc.add_msm(dual);
            return GuardKZG{acc};
        };
        try {
            SingleStrategy(params).process(opening);
            printf("single accepted\n");
        } catch (const Error& e) {
            printf("single refused: %s\n", e.what());
        }
        std::array<uint8_t, 32> seed;
        seed.fill(5);
        FrRng rng(seed);
        AccumulatorStrategy acc(params, rng);
        acc.process(opening).process(opening);
        printf("accumulated %zu %d\n", acc.msm_accumulator.left.scalars.size(), acc.finalize(lincomb_terms) ? 1 : 0);
        ParamsKZG none;
        try {
            DualMSM(none).check();
            printf("FAIL: params without G2 points gave a verdict\n");
        } catch (const Error&) {
            printf("no g2: error\n");
        }
    } catch (const std::exception& e) {
        printf("FAIL: %s\n", e.what());
        return 1;
    }
    printf("pairing mirror ok\n");
    return 0;
}
