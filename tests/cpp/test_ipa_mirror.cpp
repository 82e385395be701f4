// C++ test of the inner-product-argument mirror (host/ipa.hpp: transcript::Blake2b{Write,Read}, poly::ipa over the engine), after
// poly/multiopen_test.rs::test_roundtrip_ipa: three polynomials (the second and third with equal coefficients), a and b opened at x, c at
// y, with ParamsIPA::new_(K)'s derived generators.  The proof must verify with SingleStrategy, a wrong claimed evaluation and a flipped
// byte in every field of the multiopen proof must not, and the proof bytes are printed so that tests/test_ipa_mirror.py can compare them
// with halo2-pse_amd/ipa.py's for the same seed.  Usage: test_ipa_mirror K   (needs a GPU)
#include <cstdio>
#include <cstdlib>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
namespace ipa = halo2_proofs::poly::ipa;

static int failures = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAIL line %d: %s\n", __LINE__, #c);          \
            failures++;                                          \
        }                                                        \
    } while (0)

static std::vector<uint8_t> prove(const ipa::ParamsIPA& params, const std::array<uint8_t, 32>& seed) {
    const size_t n = params.n;
    std::vector<Fr> ax(n), bx(n), cx(n);
    for (size_t i = 0; i < n; i++) ax[i] = Fr::from(10 + i), bx[i] = Fr::from(100 + i), cx[i] = Fr::from(100 + i);
    FrRng rng(seed);
    const Fr blind = rng();
    transcript::Blake2bWrite tr;
    tr.write_point(params.commit(ax, blind));
    tr.write_point(params.commit(bx, blind));
    tr.write_point(params.commit(cx, blind));
    const Fr x = tr.squeeze_challenge(), y = tr.squeeze_challenge();
    tr.write_scalar(arithmetic::eval_polynomial(ax, x));
    tr.write_scalar(arithmetic::eval_polynomial(bx, x));
    tr.write_scalar(arithmetic::eval_polynomial(cx, y));
    ipa::ProverIPA(params).create_proof(rng, tr, {{x, &ax, blind}, {x, &bx, blind}, {y, &cx, blind}});
    return tr.finalize();
}

// true when SingleStrategy accepts
static bool verify(const ipa::ParamsIPA& params, const std::vector<uint8_t>& proof, bool wrong_eval) {
    try {
        transcript::Blake2bRead tr(proof);
        const G1Affine a = tr.read_point(), b = tr.read_point(), c = tr.read_point();  // b == c as points, two commitments by address
        const Fr x = tr.squeeze_challenge(), y = tr.squeeze_challenge();
        const Fr avx = tr.read_scalar(), bvx = tr.read_scalar(), cvy = tr.read_scalar();
        const std::vector<ipa::VerifierQuery> queries = {{&a, x, avx}, {&b, x, wrong_eval ? avx : bvx}, {&c, y, cvy}};
        ipa::SingleStrategy(params).process([&](ipa::MSMIPA msm) { return ipa::VerifierIPA(params).verify_proof(tr, queries, std::move(msm)); });
        return true;
    } catch (const ipa::Error&) {
        return false;
    } catch (const transcript::Error&) {
        return false;
    }
}

int main(int argc, char** argv) {
    const uint32_t K = argc > 1 ? uint32_t(atoi(argv[1])) : 4;
    std::array<uint8_t, 32> seed;
    for (int i = 0; i < 32; i++) seed[i] = uint8_t(7 + i);
    try {
        // BLAKE2b itself: the RFC 7693 "abc" digest, with an all-zero personalisation
        {
            const char zero[16] = {0};
            Blake2b st(zero);
            st.update(reinterpret_cast<const uint8_t*>("abc"), 3);
            const auto d = st.digest();
            CHECK(d[0] == 0xba && d[1] == 0x80 && d[2] == 0xa5 && d[3] == 0x3f && d[62] == 0x99 && d[63] == 0x23);
        }
        const ipa::ParamsIPA params = ipa::ParamsIPA::new_(K);
        const std::vector<uint8_t> proof = prove(params, seed);
        // a, b, c | avx, bvx, cvy | q_prime | u_0, u_1 | S | (L_j, R_j) x K | c, f
        CHECK(proof.size() == 32 * (6 + 1 + 2 + 1 + 2 * size_t(K) + 2));
        printf("proof ");
        for (uint8_t v : proof) printf("%02x", v);
        printf("\n");
        CHECK(verify(params, proof, false));
        CHECK(!verify(params, proof, true));
        const size_t base = 6, fields[] = {base, base + 1, base + 2, base + 3, base + 4 + 2, base + 4 + 2 * (K - 1) + 1, base + 4 + 2 * K, base + 4 + 2 * K + 1};
        for (size_t field : fields) {  // q_prime, u_0, u_1, S, L_1, R_{K-1}, c, f
            std::vector<uint8_t> bad = proof;
            bad[32 * field + 5] ^= 0x10;
            CHECK(!verify(params, bad, false));
        }
        // one opening by itself, and the other way to name G
        {
            FrRng rng(seed);
            std::vector<Fr> poly(params.n);
            rng.fill(poly.data(), params.n);
            const Fr blind = rng(), x = rng();
            const G1Affine commitment = params.commit(poly, blind);
            transcript::Blake2bWrite w;
            w.write_point(commitment);
            ipa::create_proof(params, rng, w, poly, blind, x);
            transcript::Blake2bRead r(w.finalize());
            ipa::MSMIPA msm(params);
            msm.append_term(Fr::one(), r.read_point());
            ipa::GuardIPA guard = ipa::verify_proof(params, msm, r, x, arithmetic::eval_polynomial(poly, x));
            const G1Affine g = guard.compute_g();
            CHECK(guard.use_challenges().check());
            CHECK(!g1::is_identity(g));
            // commit_lagrange of the evaluations is the same commitment
            poly::EvaluationDomain domain(1, K);
            std::vector<Fr> evals = poly;
            arithmetic::best_fft(evals, domain.omega, K);
            CHECK(params.commit_lagrange(evals, blind) == commitment);
        }
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    h2hip_shutdown();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ipa mirror ok\n");
    return 0;
}
