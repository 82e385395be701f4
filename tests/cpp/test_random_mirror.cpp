// C++ test of the randomness mirror (host/halo2hip.hpp: FrRng, fr_from_bytes_wide, plonk::vanishing::Argument::commit) against values the
// Python reference computed (tests/test_random.py writes the file named on the command line):
//   u32 k | u32 c | seed (32 B) | u64 stream id | Fr s | c x Fr (the stream's first c draws) | 2^k x Fr (draws c .. c + 2^k) |
//   Fr (draw c + 2^k) | G1Affine (the commitment of the polynomial over ParamsKZG::setup(k, s).g)           all little-endian, Fr Montgomery
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;

static int failures = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

template <class T>
static void rd(std::istream& f, T* p, size_t count = 1) {
    f.read(reinterpret_cast<char*>(p), std::streamsize(sizeof(T) * count));
    if (!f) throw std::runtime_error("short vector file");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: %s <vector file>\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream f(argv[1], std::ios::binary);
        uint32_t k, c;
        std::array<uint8_t, 32> seed;
        uint64_t stream_id;
        Fr s, want_blind;
        G1Affine want_commit;
        rd(f, &k), rd(f, &c), rd(f, seed.data(), 32), rd(f, &stream_id), rd(f, &s);
        std::vector<Fr> want_pre(c), want_poly(size_t(1) << k);
        rd(f, want_pre.data(), c), rd(f, want_poly.data(), want_poly.size()), rd(f, &want_blind), rd(f, &want_commit);

        engine_check(h2hip_init(nullptr, 0), "h2hip_init");
        poly::kzg::ParamsKZG params;
        poly::kzg::ParamsKZG::setup(k, static_cast<const Fr&>(s), params);  // the overload that takes the secret, not an rng
        const poly::EvaluationDomain domain(3, k);

        FrRng rng(seed, stream_id);
        for (uint32_t i = 0; i < c; i++) CHECK(rng() == want_pre[i]);  // one at a time: the host path
        CHECK(rng.block() == c);
        G1 commitment;
        const plonk::vanishing::Committed got = plonk::vanishing::Argument::commit(params, domain, rng, &commitment);
        CHECK(got.random_poly.len() == want_poly.size() && got.random_poly.values == want_poly);
        CHECK(got.random_blind.r == want_blind);
        CHECK(commitment.to_affine() == want_commit);
        CHECK(rng.block() == c + want_poly.size() + 1);

        // the same column in two pieces, and through the device path whatever the threshold is
        FrRng again(seed, stream_id);
        std::vector<Fr> pieces(c + want_poly.size() + 1);
        again.fill(pieces.data(), 5);
        again.fill(pieces.data() + 5, pieces.size() - 5);
        CHECK(std::equal(want_pre.begin(), want_pre.end(), pieces.begin()));
        CHECK(std::equal(want_poly.begin(), want_poly.end(), pieces.begin() + c) && pieces.back() == want_blind);

        // from_bytes_wide: 1 and 2^256
        uint8_t wide[64] = {1};
        CHECK(fr_from_bytes_wide(wide) == Fr::one());
        wide[0] = 0, wide[32] = 1;
        CHECK(fr_from_bytes_wide(wide) == Fr::from_limbs32(h2::FrP::R2));  // 2^256 in Montgomery form is 2^512 mod r

        // rejections
        Fr one;
        CHECK(h2hip_fr_random_bn254(nullptr, 0, 0, 1, one.l) == H2HIP_EINVAL && h2hip_fr_random_bn254(seed.data(), 0, 0, 1, nullptr) == H2HIP_EINVAL);
        CHECK(h2hip_fr_random_bn254(seed.data(), 0, ~uint64_t(0) - 1, 3, one.l) == H2HIP_EINVAL);
        CHECK(h2hip_fr_random_bn254(seed.data(), 0, ~uint64_t(0), 1, one.l) == H2HIP_OK);
        CHECK(h2hip_fr_random_bn254(nullptr, 0, 0, 0, nullptr) == H2HIP_OK && h2hip_fr_from_bytes_wide_bn254(nullptr, 0, nullptr) == H2HIP_OK);
        CHECK(h2hip_fr_from_bytes_wide_bn254(nullptr, 1, one.l) == H2HIP_EINVAL && h2hip_fr_from_bytes_wide_bn254(wide, 1, nullptr) == H2HIP_EINVAL);
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("random mirror tests ok\n");
    return 0;
}
