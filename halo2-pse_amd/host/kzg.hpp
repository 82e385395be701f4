// kzg.hpp -- the C++ mirror of what closes a KZG check in the reference at E = Bn256, over the C ABI (include/halo2hip_pairing.h,
// include/halo2hip_g1.h and the MSM of include/halo2hip.h).  Included by halo2hip.hpp; same error behaviour.
//
//   poly::kzg::MSMKZG                                  poly/kzg/msm.rs:13-82
//   poly::kzg::DualMSM                                 poly/kzg/msm.rs:120-170
//   poly::kzg::{GuardKZG, SingleStrategy, AccumulatorStrategy}   poly/kzg/strategy.rs
//   poly::kzg::{pairing_check, pairing, g2_mul, g2_neg}          halo2curves' pairing engine as far as the above use it
//
// DualMSM::check is e(left, s_g2) e(right, -g2) = 1: each side is evaluated in the library (up to 4096 terms on the host with
// h2hip_g1_linear_combinations_bn254, above that with the engine's MSM), then one h2hip_pairing_check_bn254 call runs two Miller
// loops and one final exponentiation on the calling thread.  AccumulatorStrategy's scale factor comes from the caller's FrRng where
// the reference draws from OsRng.  halo2-pse_amd/kzg.py is the same composition in Python, and tests/test_pairing_mirror.py compares
// the two.
#pragma once
#include <functional>

#include "../../include/halo2hip_g1.h"
#include "../../include/halo2hip_pairing.h"
#include "halo2hip.hpp"

namespace halo2_proofs {
namespace poly {
namespace kzg {

struct Error : std::runtime_error {  // Error::ConstraintSystemFailure, or params that cannot decide a check
    using std::runtime_error::runtime_error;
};

typedef std::array<uint8_t, 128> G2Raw;  // x.c0 || x.c1 || y.c0 || y.c1, Montgomery; all zero: the identity
typedef std::array<uint64_t, 48> Gt;     // a_0, b_0, ..., a_5, b_5: sum (a_i + b_i u) w^i (include/halo2hip_pairing.h)

namespace detail {
inline std::vector<uint64_t> g2_limbs(const std::vector<G2Raw>& g2) {
    std::vector<uint64_t> out(16 * g2.size());
    for (size_t i = 0; i < g2.size(); i++) std::memcpy(out.data() + 16 * i, g2[i].data(), 128);
    return out;
}
}  // namespace detail

// prod_i e(g1[i], g2[i]) = 1
inline bool pairing_check(const std::vector<G1Affine>& g1, const std::vector<G2Raw>& g2) {
    if (g1.size() != g2.size()) throw std::logic_error("pairing_check: one G2 point per G1 point");
    const std::vector<uint64_t> q = detail::g2_limbs(g2);
    int ok = 0;
    engine_check(h2hip_pairing_check_bn254(g1.empty() ? nullptr : g1[0].x, q.data(), g1.size(), &ok), "h2hip_pairing_check_bn254");
    return ok == 1;
}
// prod_i e(g1[i], g2[i])
inline Gt pairing(const std::vector<G1Affine>& g1, const std::vector<G2Raw>& g2) {
    if (g1.size() != g2.size()) throw std::logic_error("pairing: one G2 point per G1 point");
    const std::vector<uint64_t> q = detail::g2_limbs(g2);
    Gt out;
    engine_check(h2hip_pairing_bn254(g1.empty() ? nullptr : g1[0].x, q.data(), g1.size(), out.data()), "h2hip_pairing_bn254");
    return out;
}
inline G2Raw g2_mul(const G2Raw& q, const Fr& scalar) {
    uint64_t in[16], out[16];
    std::memcpy(in, q.data(), 128);
    engine_check(h2hip_g2_mul_bn254(in, scalar.l, out), "h2hip_g2_mul_bn254");
    G2Raw r;
    std::memcpy(r.data(), out, 128);
    return r;
}
inline G2Raw g2_neg(const G2Raw& q) {  // the identity stays
    h2::Fe c[4];
    std::memcpy(c, q.data(), 128);
    c[2] = h2::fe_neg<h2::FqP>(c[2]);
    c[3] = h2::fe_neg<h2::FqP>(c[3]);
    G2Raw r;
    std::memcpy(r.data(), c, 128);
    return r;
}

// msm.rs:13-82: a list of (scalar, base) terms
class MSMKZG {
   public:
    static constexpr size_t LINCOMB_TERMS = 4096;  // the most terms one h2hip_g1_linear_combinations_bn254 call takes
    std::vector<Fr> scalars;
    std::vector<G1Affine> bases;

    void append_term(const Fr& scalar, const G1Affine& point) {  // :47-50
        scalars.push_back(scalar);
        bases.push_back(point);
    }
    void add_msm(const MSMKZG& other) {  // :52-55
        scalars.insert(scalars.end(), other.scalars.begin(), other.scalars.end());
        bases.insert(bases.end(), other.bases.begin(), other.bases.end());
    }
    void scale(const Fr& factor) {  // :57-60
        for (Fr& s : scalars) s = s * factor;
    }
    // :62-67, affine: up to lincomb_terms terms on the host, more through the engine's MSM
    G1Affine eval(size_t lincomb_terms = LINCOMB_TERMS) const {
        G1Affine out{};
        if (scalars.empty()) return out;
        if (scalars.size() <= std::min(lincomb_terms, LINCOMB_TERMS)) {
            engine_check(h2hip_g1_linear_combinations_bn254(nullptr, scalars[0].l, bases[0].x, 1, scalars.size(), out.x),
                         "h2hip_g1_linear_combinations_bn254");
            return out;
        }
        std::vector<Fr> s;  // an identity base contributes nothing and is left out, as kzg.py's eval_msm leaves it out
        std::vector<G1Affine> b;
        for (size_t i = 0; i < bases.size(); i++)
            if (!(bases[i] == G1Affine{})) s.push_back(scalars[i]), b.push_back(bases[i]);
        return arithmetic::best_multiexp(s, b).to_affine();
    }
};

// msm.rs:120-170
class DualMSM {
   public:
    const ParamsKZG* params;
    MSMKZG left, right;

    explicit DualMSM(const ParamsKZG& p) : params(&p) {}  // :130-136
    void scale(const Fr& e) {                             // :139-142
        left.scale(e);
        right.scale(e);
    }
    void add_msm(const DualMSM& other) {  // :145-148
        left.add_msm(other.left);
        right.add_msm(other.right);
    }
    // :151-169.  Params whose g2 or s_g2 is the identity cannot decide anything (a pairing with the identity is 1): an Error
    bool check(size_t lincomb_terms = MSMKZG::LINCOMB_TERMS) const {
        if (serde::all_zero(params->g2.data(), 128) || serde::all_zero(params->s_g2.data(), 128))
            throw Error("the params carry no G2 points: g2 or s_g2 is the identity");
        return pairing_check({left.eval(lincomb_terms), right.eval(lincomb_terms)}, {params->s_g2, g2_neg(params->g2)});
    }
};

// strategy.rs:26-47
struct GuardKZG {
    DualMSM msm_accumulator;
};

// strategy.rs:69-82, :122-159
class SingleStrategy {
   public:
    explicit SingleStrategy(const ParamsKZG& params) : msm_(params) {}
    // f: DualMSM -> GuardKZG; Error (Error::ConstraintSystemFailure) unless the pairing check holds
    void process(const std::function<GuardKZG(DualMSM)>& f) {
        if (!f(msm_).msm_accumulator.check()) throw Error("ConstraintSystemFailure: the pairing check does not hold");
    }

   private:
    DualMSM msm_;
};

// strategy.rs:49-67, :84-120; the scale factor is the next draw of the caller's rng
class AccumulatorStrategy {
   public:
    AccumulatorStrategy(const ParamsKZG& params, FrRng& rng) : msm_accumulator(params), rng_(&rng) {}
    AccumulatorStrategy& process(const std::function<GuardKZG(DualMSM)>& f) {
        msm_accumulator.scale((*rng_)());               // :108
        msm_accumulator = f(msm_accumulator).msm_accumulator;  // :111-114
        return *this;
    }
    bool finalize(size_t lincomb_terms = MSMKZG::LINCOMB_TERMS) const { return msm_accumulator.check(lincomb_terms); }  // :117-119

    DualMSM msm_accumulator;

   private:
    FrRng* rng_;
};

}  // namespace kzg
}  // namespace poly
}  // namespace halo2_proofs
