// halo2hip.hpp -- C++ host-side mirror of the reference's Rust interface for the accelerated
// path, layered on the C ABI (include/halo2hip.h).  The reference is Rust and no Rust toolchain
// exists in the build image, so this header plays the role the patched `halo2_proofs` modules
// would: same names, same argument meaning, same contract checks.
//
//   halo2_proofs::arithmetic::best_multiexp      halo2_proofs/src/arithmetic.rs:132-159
//   halo2_proofs::arithmetic::best_fft           halo2_proofs/src/arithmetic.rs:171-234
//   halo2_proofs::poly::EvaluationDomain         halo2_proofs/src/poly/domain.rs:18-361
//   halo2_proofs::poly::kzg::ParamsKZG           halo2_proofs/src/poly/kzg/commitment.rs:22-339
//   halo2_proofs::plonk::{GraphEvaluator, Evaluator}   halo2_proofs/src/plonk/evaluation.rs   (in evaluation.hpp)
//   halo2_proofs::plonk::permutation::keygen::Assembly, batch_invert_assigned, keygen_pk's columns
//                                                halo2_proofs/src/plonk/permutation/keygen.rs, poly.rs:180-209, plonk/keygen.rs:298-366
//
// Error behaviour: where the reference panics on a contract violation (assert_eq! / assert!),
// this mirror throws std::logic_error; a non-zero engine status throws std::runtime_error
// (the Rust shim would fall back to the CPU body instead -- there is none in this library).
// Header-only; plain C++17; link with -lhalo2hip.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <istream>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/halo2hip.h"
#include "../../include/halo2hip_pairing.h"
#include "../csrc/ec.h"  // host-side Fr / Fq / G1 arithmetic for domain constants and SRS checks (no HIP needed)

namespace halo2_proofs {

// bn256::Fr, G1Affine, G1 in halo2curves' in-memory layout (4 x u64 LE limbs, Montgomery)
struct Fr {
    uint64_t l[4];
    bool operator==(const Fr& o) const { return std::memcmp(l, o.l, 32) == 0; }
    bool operator!=(const Fr& o) const { return !(*this == o); }
    static Fr zero() { return Fr{{0, 0, 0, 0}}; }
    static Fr one() { return from_fe(h2::fe_one<h2::FrP>()); }
    static Fr from(uint64_t v) { return from_fe(h2::fe_from_u64<h2::FrP>(v)); }  // Fr::from(u64)
    Fr operator*(const Fr& o) const { return from_fe(h2::fe_mul<h2::FrP>(fe(), o.fe())); }
    Fr operator+(const Fr& o) const { return from_fe(h2::fe_add<h2::FrP>(fe(), o.fe())); }
    Fr operator-(const Fr& o) const { return from_fe(h2::fe_sub<h2::FrP>(fe(), o.fe())); }
    Fr square() const { return *this * *this; }
    Fr invert() const { return from_fe(h2::fe_inv<h2::FrP>(fe())); }
    Fr pow_vartime(uint64_t e) const { return from_fe(h2::fe_pow_u64<h2::FrP>(fe(), e)); }
    static Fr root_of_unity() { return from_limbs32(h2::FrP::ROOT_OF_UNITY); }
    static Fr zeta() { return from_limbs32(h2::FrP::ZETA); }
    static Fr delta() { return from(7).pow_vartime(uint64_t(1) << S_); }  // Fr::DELTA = MULTIPLICATIVE_GENERATOR^(2^S)
    static constexpr uint32_t S = 28;
    static constexpr uint32_t S_ = 28;
    h2::Fe fe() const {
        h2::Fe f;
        std::memcpy(f.l, l, 32);
        return f;
    }
    static Fr from_fe(const h2::Fe& f) {
        Fr r;
        std::memcpy(r.l, f.l, 32);
        return r;
    }
    static Fr from_limbs32(const uint32_t v[8]) {
        Fr r;
        std::memcpy(r.l, v, 32);
        return r;
    }
};
static_assert(sizeof(Fr) == 32, "Fr layout");

struct G1Affine {
    uint64_t x[4], y[4];
    bool operator==(const G1Affine& o) const { return std::memcmp(this, &o, 64) == 0; }
};
static_assert(sizeof(G1Affine) == 64, "G1Affine layout");

struct G1 {
    uint64_t x[4], y[4], z[4];
    G1Affine to_affine() const {  // Curve::to_affine
        G1Affine a;
        if (h2hip_g1_to_affine(x, a.x) != 0) throw std::runtime_error(h2hip_last_error());
        return a;
    }
    // projective equality, as halo2curves' PartialEq for G1
    bool operator==(const G1& o) const { return to_affine() == o.to_affine(); }
};
static_assert(sizeof(G1) == 96, "G1 layout");

// SerdeFormat (helpers.rs:8-20)
enum class SerdeFormat {
    Processed,          // curve points compressed, field elements canonical; every element checked
    RawBytes,           // the in-memory Montgomery limbs; coordinates below the modulus and points on the curve checked
    RawBytesUnchecked,  // the same bytes, no checks
};

// The host-only part of the formats: the two G2 points of a params file (Fq2 = Fq[u] / (u^2 + 1), the twist y^2 = x^3 + 3 / (9 + u))
// over field.h, and a host decompression of one G1 point by fe_pow, the yardstick tools/serde_host.cpp times the GPU against.
// Raw G2: x.c0 || x.c1 || y.c0 || y.c1, 32-B Montgomery each; compressed: x.c0 || x.c1 canonical little-endian with the low bit of
// canonical y.c0 in bit 7 of byte 63; all zero bytes: the identity.
namespace serde {
typedef h2::FqP Q;
using h2::Fe;
struct Fq2 {
    Fe c0, c1;
};
inline const uint32_t* fq_sqrt_exponent() {  // (q + 1) / 4
    static const uint32_t e[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    return e;
}
// q = 3 (mod 4): t^((q + 1) / 4) is a root of every square
inline bool fq_sqrt(const Fe& t, Fe* y) {
    *y = h2::fe_pow<Q>(t, fq_sqrt_exponent());
    return h2::fe_eq(h2::fe_sqr<Q>(*y), t);
}
inline Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
    return {h2::fe_sub<Q>(h2::fe_mul<Q>(a.c0, b.c0), h2::fe_mul<Q>(a.c1, b.c1)), h2::fe_add<Q>(h2::fe_mul<Q>(a.c0, b.c1), h2::fe_mul<Q>(a.c1, b.c0))};
}
inline bool fq2_eq(const Fq2& a, const Fq2& b) { return h2::fe_eq(a.c0, b.c0) && h2::fe_eq(a.c1, b.c1); }
// x^3 + 3 / (9 + u), with 3 / (9 + u) = 3 (9 - u) / 82
inline Fq2 g2_rhs(const Fq2& x) {
    const Fe i82 = h2::fe_inv<Q>(h2::fe_from_u64<Q>(82));
    const Fq2 b = {h2::fe_mul<Q>(h2::fe_from_u64<Q>(27), i82), h2::fe_neg<Q>(h2::fe_mul<Q>(h2::fe_from_u64<Q>(3), i82))};
    const Fq2 x3 = fq2_mul(fq2_mul(x, x), x);
    return {h2::fe_add<Q>(x3.c0, b.c0), h2::fe_add<Q>(x3.c1, b.c1)};
}
// a root of a, any of the two: with s^2 = a0^2 + a1^2, x0^2 = (a0 + s) / 2 or (a0 - s) / 2 and x1 = a1 / (2 x0)
inline bool fq2_sqrt(const Fq2& a, Fq2* r) {
    if (h2::fe_is_zero(a.c0) && h2::fe_is_zero(a.c1)) {
        *r = a;
        return true;
    }
    Fe s, x0;
    if (!fq_sqrt(h2::fe_add<Q>(h2::fe_sqr<Q>(a.c0), h2::fe_sqr<Q>(a.c1)), &s)) return false;
    const Fe half = h2::fe_inv<Q>(h2::fe_from_u64<Q>(2));
    for (const Fe& cand : {h2::fe_mul<Q>(h2::fe_add<Q>(a.c0, s), half), h2::fe_mul<Q>(h2::fe_sub<Q>(a.c0, s), half)}) {
        if (!fq_sqrt(cand, &x0) || h2::fe_is_zero(x0)) continue;
        *r = {x0, h2::fe_mul<Q>(a.c1, h2::fe_inv<Q>(h2::fe_dbl<Q>(x0)))};
        if (fq2_eq(fq2_mul(*r, *r), a)) return true;
    }
    if (h2::fe_is_zero(a.c1) && fq_sqrt(h2::fe_neg<Q>(a.c0), &x0)) {  // a = -c^2 in Fq: the root is purely imaginary
        *r = {h2::fe_zero<Q>(), x0};
        return true;
    }
    return false;
}
// G2Affine::generator(): EIP-197's generator, raw
inline std::array<uint8_t, 128> g2_generator() {
    static const uint32_t canonical[4][8] = {
        {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},   // x.c0
        {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},   // x.c1
        {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},   // y.c0
        {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};  // y.c1
    std::array<uint8_t, 128> raw;
    for (int i = 0; i < 4; i++) {
        Fe c;
        std::memcpy(c.l, canonical[i], 32);
        const Fe m = h2::fe_from_canonical<Q>(c);
        std::memcpy(raw.data() + 32 * i, m.l, 32);
    }
    return raw;
}
inline bool all_zero(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (p[i]) return false;
    return true;
}
// read_raw's checks for a raw G2 point
inline bool g2_is_valid(const std::array<uint8_t, 128>& raw) {
    if (all_zero(raw.data(), 128)) return true;
    Fe c[4];
    std::memcpy(c, raw.data(), 128);
    for (const Fe& v : c)
        if (!h2::fe_is_canonical<Q>(v)) return false;
    const Fq2 y = {c[2], c[3]};
    return fq2_eq(fq2_mul(y, y), g2_rhs({c[0], c[1]}));
}
inline bool g2_from_bytes(const uint8_t in[64], std::array<uint8_t, 128>& raw) {
    raw.fill(0);
    if (all_zero(in, 64)) return true;
    Fe c[2];
    std::memcpy(c, in, 64);
    const uint32_t sign = c[1].l[7] >> 31;
    c[1].l[7] &= 0x7fffffffu;
    if (!h2::fe_is_canonical<Q>(c[0]) || !h2::fe_is_canonical<Q>(c[1])) return false;
    const Fq2 x = {h2::fe_from_canonical<Q>(c[0]), h2::fe_from_canonical<Q>(c[1])};
    Fq2 y;
    if ((h2::fe_is_zero(x.c0) && h2::fe_is_zero(x.c1)) || !fq2_sqrt(g2_rhs(x), &y)) return false;
    if ((h2::fe_to_canonical<Q>(y.c0).l[0] & 1u) != sign) y = {h2::fe_neg<Q>(y.c0), h2::fe_neg<Q>(y.c1)};
    const Fe out[4] = {x.c0, x.c1, y.c0, y.c1};
    std::memcpy(raw.data(), out, 128);
    return true;
}
inline void g2_to_bytes(const std::array<uint8_t, 128>& raw, uint8_t out[64]) {
    std::memset(out, 0, 64);
    if (all_zero(raw.data(), 128)) return;
    Fe c[4];
    std::memcpy(c, raw.data(), 128);
    Fe x[2] = {h2::fe_to_canonical<Q>(c[0]), h2::fe_to_canonical<Q>(c[1])};
    x[1].l[7] |= (h2::fe_to_canonical<Q>(c[2]).l[0] & 1u) << 31;
    std::memcpy(out, x, 64);
}
// G1Affine::from_bytes on the host, one point: what h2hip_g1_decompress_bn254 does per lane
inline bool g1_from_bytes_host(const uint8_t in[32], G1Affine& out) {
    std::memset(&out, 0, 64);
    Fe xc;
    std::memcpy(xc.l, in, 32);
    const uint32_t sign = xc.l[7] >> 31;
    xc.l[7] &= 0x7fffffffu;
    if (h2::fe_is_zero(xc)) return !sign;
    if (!h2::fe_is_canonical<Q>(xc)) return false;
    const Fe x = h2::fe_from_canonical<Q>(xc);
    Fe y;
    if (!fq_sqrt(h2::fe_add<Q>(h2::fe_mul<Q>(h2::fe_sqr<Q>(x), x), h2::fe_from_u64<Q>(3)), &y)) return false;
    if ((h2::fe_to_canonical<Q>(y).l[0] & 1u) != sign) y = h2::fe_neg<Q>(y);
    std::memcpy(out.x, x.l, 32);
    std::memcpy(out.y, y.l, 32);
    return true;
}
inline void read_exact(std::istream& reader, void* dst, size_t n, const char* what) {
    reader.read(reinterpret_cast<char*>(dst), std::streamsize(n));
    if (!reader || size_t(reader.gcount()) != n) throw std::runtime_error(std::string(what) + ": short read");
}
inline uint32_t read_u32_be(std::istream& reader, const char* what) {
    uint8_t b[4];
    read_exact(reader, b, 4, what);
    return uint32_t(b[0]) << 24 | uint32_t(b[1]) << 16 | uint32_t(b[2]) << 8 | uint32_t(b[3]);
}
inline void write_u32_be(std::ostream& writer, uint32_t v) {
    const char b[4] = {char(v >> 24), char(v >> 16), char(v >> 8), char(v)};
    writer.write(b, 4);
}
}  // namespace serde

inline void engine_check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + h2hip_last_error());
}

// ChaCha20Rng::from_seed(seed) as far as Fr::random uses it (rand_chacha 0.3, halo2curves 0.3.1 as DESIGN.md section 2 records them):
// every draw consumes one 64-byte block, so the state is the number of the next block, and a whole column of draws is one engine call
// (h2hip_fr_random_bn254: on the calling thread for a handful, on the GPU from HALO2_HIP_RANDOM_MIN_N elements on).  Draws come out in
// the stream's order whichever way they are made.  The seed is the caller's entropy and as secret as what is drawn; wiped on destruction.
class FrRng {
   public:
    explicit FrRng(const std::array<uint8_t, 32>& seed, uint64_t stream_id = 0) : seed_(seed), stream_id_(stream_id) {}
    FrRng(const FrRng&) = delete;
    FrRng& operator=(const FrRng&) = delete;
    ~FrRng() {
        volatile uint8_t* p = seed_.data();
        for (size_t i = 0; i < 32; i++) p[i] = 0;
    }
    uint64_t block() const { return block_; }  // draws made so far
    // n draws of <Fr as Field>::random(&mut rng)
    void fill(Fr* out, size_t n) {
        engine_check(h2hip_fr_random_bn254(seed_.data(), stream_id_, block_, n, n ? out[0].l : nullptr), "h2hip_fr_random_bn254");
        block_ += n;
    }
    Fr operator()() {
        Fr v;
        fill(&v, 1);
        return v;
    }

   private:
    std::array<uint8_t, 32> seed_;
    uint64_t stream_id_, block_ = 0;
};

// Fr::from_bytes_wide: 64 bytes as one little-endian integer, reduced mod r
inline Fr fr_from_bytes_wide(const uint8_t bytes[64]) {
    Fr v;
    engine_check(h2hip_fr_from_bytes_wide_bn254(bytes, 1, v.l), "h2hip_fr_from_bytes_wide_bn254");
    return v;
}

namespace arithmetic {

// pub fn best_multiexp<C: CurveAffine>(coeffs: &[C::Scalar], bases: &[C]) -> C::Curve   (arithmetic.rs:132)
inline G1 best_multiexp(const std::vector<Fr>& coeffs, const G1Affine* bases, size_t bases_len) {
    if (coeffs.size() != bases_len) throw std::logic_error("assertion failed: coeffs.len() == bases.len()");  // :133
    G1 out;
    engine_check(h2hip_msm_bn254(coeffs.empty() ? nullptr : coeffs[0].l, bases_len ? bases[0].x : nullptr, coeffs.size(), out.x),
                 "best_multiexp");
    return out;
}
inline G1 best_multiexp(const std::vector<Fr>& coeffs, const std::vector<G1Affine>& bases) {
    return best_multiexp(coeffs, bases.data(), bases.size());
}

// pub fn best_fft<G: Group>(a: &mut [G], omega: G::Scalar, log_n: u32)                  (arithmetic.rs:171)
inline void best_fft(std::vector<Fr>& a, const Fr& omega, uint32_t log_n) {
    if (log_n > 63 || a.size() != (size_t(1) << log_n)) throw std::logic_error("assertion failed: n == 1 << log_n");  // :184
    engine_check(h2hip_ntt_bn254_fr(a[0].l, omega.l, log_n), "best_fft");
}

// best_fft with G = G1 (arithmetic.rs:171-234; in the crate: g_to_lagrange, :285): in place on Jacobian points, the caller's omega.
// Only the group elements are defined by the reference; they come back with z = 1 (identity: z = 0).
inline void best_fft(std::vector<G1>& a, const Fr& omega, uint32_t log_n) {
    if (log_n > 63 || a.size() != (size_t(1) << log_n)) throw std::logic_error("assertion failed: n == 1 << log_n");  // :184
    engine_check(h2hip_fft_bn254_g1(a[0].x, omega.l, log_n), "best_fft::<G1>");
}

// g_to_lagrange (arithmetic.rs:277-301); takes the affine points (the reference converts them with to_curve() at the call site)
inline std::vector<G1Affine> g_to_lagrange(const std::vector<G1Affine>& g, uint32_t k) {
    if (g.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.len() == 1 << log_n");  // best_fft, :184
    std::vector<G1Affine> out(g.size());
    engine_check(h2hip_g_to_lagrange_bn254(g[0].x, k, out[0].x), "h2hip_g_to_lagrange_bn254");
    return out;
}

// eval_polynomial (arithmetic.rs:304-328) on the engine (h2hip_eval_polynomials_bn254); a batch of queries is one call
inline std::vector<Fr> eval_polynomials(const std::vector<const std::vector<Fr>*>& polys, const std::vector<uint32_t>& query_poly,
                                        const std::vector<Fr>& points) {
    if (query_poly.size() != points.size()) throw std::logic_error("query_poly and points differ in length");
    std::vector<const uint64_t*> p;
    std::vector<size_t> lens;
    for (auto* v : polys) {
        p.push_back(v->empty() ? nullptr : (*v)[0].l);
        lens.push_back(v->size());
    }
    std::vector<Fr> evals(points.size());
    if (!points.empty())
        engine_check(h2hip_eval_polynomials_bn254(p.data(), lens.data(), p.size(), query_poly.data(), points[0].l, points.size(), evals[0].l),
                     "eval_polynomials");
    return evals;
}

inline Fr eval_polynomial(const std::vector<Fr>& poly, const Fr& point) { return eval_polynomials({&poly}, {0}, {point})[0]; }

// The engine's combine / divide / scale primitive (h2hip_poly_combine_bn254_fr): (sum_j scalars[j] polys[j] - sub) / prod (X - r), times
// scale; out_len coefficients (at least len - roots.size()), zero past the quotient
inline std::vector<Fr> poly_combine(const std::vector<const std::vector<Fr>*>& polys, const std::vector<Fr>& scalars, const std::vector<Fr>& sub,
                                    const std::vector<Fr>& roots, const Fr& scale, size_t out_len) {
    if (polys.empty() || scalars.size() != polys.size()) throw std::logic_error("poly_combine: one scalar per polynomial");
    const size_t len = polys[0]->size();
    std::vector<const uint64_t*> p;
    for (auto* v : polys) {
        if (v->size() != len) throw std::logic_error("poly_combine: polynomials differ in length");
        p.push_back(len ? (*v)[0].l : nullptr);
    }
    std::vector<Fr> out(out_len);
    engine_check(h2hip_poly_combine_bn254_fr(p.data(), len, scalars[0].l, p.size(), sub.empty() ? nullptr : sub[0].l, sub.size(),
                                             roots.empty() ? nullptr : roots[0].l, roots.size(), scale.l, 0, out.empty() ? nullptr : out[0].l,
                                             out_len, nullptr),
                 "poly_combine");
    return out;
}

// kate_division (arithmetic.rs:348-366): a(X) / (X - b) without the remainder; panics (logic_error) on an empty a, as the reference does
inline std::vector<Fr> kate_division(const std::vector<Fr>& a, const Fr& b) {
    if (a.empty()) throw std::logic_error("kate_division of an empty polynomial");
    return poly_combine({&a}, {Fr::one()}, {}, {b}, Fr::one(), a.size() - 1);
}

// the host-side O(points^2) helpers the multiopen provers keep: powers, evaluate_vanishing_polynomial, lagrange_interpolate (:405-460)
inline std::vector<Fr> powers(const Fr& x, size_t m) {
    std::vector<Fr> out;
    Fr acc = Fr::one();
    for (size_t i = 0; i < m; i++, acc = acc * x) out.push_back(acc);
    return out;
}

inline Fr evaluate_vanishing_polynomial(const std::vector<Fr>& roots, const Fr& z) {
    Fr acc = Fr::one();
    for (auto& r : roots) acc = acc * (z - r);
    return acc;
}

inline std::vector<Fr> lagrange_interpolate(const std::vector<Fr>& points, const std::vector<Fr>& evals) {
    if (points.size() != evals.size()) throw std::logic_error("lagrange_interpolate: lengths differ");
    const size_t m = points.size();
    std::vector<Fr> out(m, Fr::zero());
    for (size_t j = 0; j < m; j++) {
        std::vector<Fr> basis{Fr::one()};
        Fr denom = Fr::one();
        for (size_t k = 0; k < m; k++) {
            if (k == j) continue;
            std::vector<Fr> next(basis.size() + 1, Fr::zero());
            for (size_t i = 0; i < basis.size(); i++) {
                next[i + 1] = next[i + 1] + basis[i];
                next[i] = next[i] - basis[i] * points[k];
            }
            basis.swap(next);
            denom = denom * (points[j] - points[k]);
        }
        const Fr f = evals[j] * denom.invert();
        for (size_t i = 0; i < m; i++) out[i] = out[i] + f * basis[i];
    }
    return out;
}

}  // namespace arithmetic

namespace poly {

struct Coeff {};
struct LagrangeCoeff {};
struct ExtendedLagrangeCoeff {};

// Polynomial<F, B> (poly.rs:66-72): a Vec<F> plus a basis marker
template <class Basis>
struct Polynomial {
    std::vector<Fr> values;
    size_t len() const { return values.size(); }
    Fr& operator[](size_t i) { return values[i]; }
    const Fr& operator[](size_t i) const { return values[i]; }
};

// Polynomial::read (poly.rs:152-165): a big-endian u32 length, then that many Fr in the format's encoding (SerdePrimeField,
// helpers.rs:61-93).  Processed: canonical little-endian, converted and checked on the GPU (h2hip_fr_from_repr_bn254); RawBytes: the
// Montgomery limbs, checked to be below r; RawBytesUnchecked: no checks.  A failed check throws where the reference returns io::Error.
template <class Basis>
inline Polynomial<Basis> read_polynomial(std::istream& reader, SerdeFormat format) {
    const uint32_t len = serde::read_u32_be(reader, "Polynomial::read");
    Polynomial<Basis> p{std::vector<Fr>(len)};
    if (len == 0) return p;
    serde::read_exact(reader, p.values.data(), size_t(len) * 32, "Polynomial::read");
    if (format == SerdeFormat::Processed) {
        uint64_t invalid[2];
        engine_check(h2hip_fr_from_repr_bn254(p.values[0].l, len, p.values[0].l, invalid), "Invalid prime field point encoding");
    } else if (format == SerdeFormat::RawBytes) {
        for (const Fr& v : p.values)
            if (!h2::fe_is_canonical<h2::FrP>(v.fe())) throw std::runtime_error("Polynomial::read: Invalid prime field point encoding");
    }
    return p;
}
// Polynomial::write (poly.rs:167-177)
template <class Basis>
inline void write_polynomial(const Polynomial<Basis>& p, std::ostream& writer, SerdeFormat format) {
    serde::write_u32_be(writer, uint32_t(p.len()));
    if (p.len() == 0) return;
    if (format == SerdeFormat::Processed) {
        std::vector<uint8_t> repr(p.len() * 32);
        engine_check(h2hip_fr_to_repr_bn254(p.values[0].l, p.len(), repr.data()), "h2hip_fr_to_repr_bn254");
        writer.write(reinterpret_cast<const char*>(repr.data()), std::streamsize(repr.size()));
    } else {
        writer.write(reinterpret_cast<const char*>(p.values.data()), std::streamsize(p.len() * 32));
    }
}
// read_polynomial_vec / write_polynomial_slice (helpers.rs:116-140): a big-endian u32 count, then the polynomials
template <class Basis>
inline std::vector<Polynomial<Basis>> read_polynomial_vec(std::istream& reader, SerdeFormat format) {
    const uint32_t count = serde::read_u32_be(reader, "read_polynomial_vec");
    std::vector<Polynomial<Basis>> out;
    for (uint32_t i = 0; i < count; i++) out.push_back(read_polynomial<Basis>(reader, format));
    return out;
}
template <class Basis>
inline void write_polynomial_slice(const std::vector<Polynomial<Basis>>& slice, std::ostream& writer, SerdeFormat format) {
    serde::write_u32_be(writer, uint32_t(slice.size()));
    for (const auto& p : slice) write_polynomial(p, writer, format);
}

// EvaluationDomain<Fr> (poly/domain.rs:18-34)
class EvaluationDomain {
   public:
    uint64_t n;
    uint32_t k, extended_k;
    Fr omega, omega_inv, extended_omega, extended_omega_inv, g_coset, g_coset_inv;
    uint64_t quotient_poly_degree;
    Fr ifft_divisor, extended_ifft_divisor;
    std::vector<Fr> t_evaluations;
    Fr barycentric_weight;

    // EvaluationDomain::new (poly/domain.rs:39-142)
    EvaluationDomain(uint32_t j, uint32_t k_) {
        quotient_poly_degree = uint64_t(j - 1);                     // :41
        k = k_;
        n = uint64_t(1) << k;                                       // :44
        extended_k = k;                                             // :49-52
        while ((uint64_t(1) << extended_k) < n * quotient_poly_degree) extended_k++;
        if (extended_k > Fr::S) throw std::logic_error("extended_k exceeds the 2-adicity of Fr");
        extended_omega = Fr::root_of_unity();                       // :54-61
        for (uint32_t i = extended_k; i < Fr::S; i++) extended_omega = extended_omega.square();
        omega = extended_omega;                                     // :70-73
        for (uint32_t i = k; i < extended_k; i++) omega = omega.square();
        g_coset = Fr::zeta();                                       // :81
        g_coset_inv = g_coset.square();                             // :82
        {                                                           // :84-107
            Fr orig = Fr::zeta().pow_vartime(n), step = extended_omega.pow_vartime(n), cur = orig;
            do {
                t_evaluations.push_back(cur);
                cur = cur * step;
            } while (cur != orig);
            if (t_evaluations.size() != (size_t(1) << (extended_k - k))) throw std::logic_error("t_evaluations length");  // :98
            for (auto& c : t_evaluations) c = (c - Fr::one()).invert();  // :101-103, :117-124
        }
        ifft_divisor = Fr::from(uint64_t(1) << k).invert();               // :109
        extended_ifft_divisor = Fr::from(uint64_t(1) << extended_k).invert();  // :110
        barycentric_weight = Fr::from(n).invert();                        // :114
        extended_omega_inv = extended_omega.invert();
        omega_inv = omega.invert();
    }

    size_t extended_len() const { return size_t(1) << extended_k; }       // :374-376

    Polynomial<LagrangeCoeff> empty_lagrange() const { return {std::vector<Fr>(n, Fr::zero())}; }  // :177-182

    // lagrange_to_coeff (poly/domain.rs:226-236)
    Polynomial<Coeff> lagrange_to_coeff(Polynomial<LagrangeCoeff> a) const {
        if (a.values.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.values.len() == 1 << self.k");  // :227
        engine_check(h2hip_ifft_bn254_fr(a.values[0].l, omega_inv.l, k, ifft_divisor.l), "lagrange_to_coeff");            // :230
        return {std::move(a.values)};
    }

    // the same for the columns create_proof converts back to back (plonk/prover.rs:476-490; patch 0004's lagrange_to_coeff_batch): one
    // pipelined engine call -- column i + 1 goes up and column i - 1 comes down while column i is transformed
    std::vector<Polynomial<Coeff>> lagrange_to_coeff_batch(std::vector<Polynomial<LagrangeCoeff>> polys) const {
        std::vector<uint64_t*> cols;
        for (auto& a : polys) {
            if (a.values.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.values.len() == 1 << self.k");
            cols.push_back(a.values[0].l);
        }
        engine_check(h2hip_ifft_bn254_fr_batch(cols.data(), cols.size(), omega_inv.l, k, ifft_divisor.l), "lagrange_to_coeff_batch");
        std::vector<Polynomial<Coeff>> out;
        for (auto& a : polys) out.push_back({std::move(a.values)});
        return out;
    }

    // coeff_to_extended for several polynomials (plonk/evaluation.rs:306-323; patch 0004's coeff_to_extended_batch)
    std::vector<Polynomial<ExtendedLagrangeCoeff>> coeff_to_extended_batch(const std::vector<Polynomial<Coeff>>& polys) const {
        std::vector<Polynomial<ExtendedLagrangeCoeff>> out(polys.size());
        std::vector<const uint64_t*> ins;
        std::vector<uint64_t*> outs;
        for (size_t i = 0; i < polys.size(); i++) {
            if (polys[i].values.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.values.len() == 1 << self.k");
            out[i].values.resize(extended_len());
            ins.push_back(polys[i].values[0].l);
            outs.push_back(out[i].values[0].l);
        }
        engine_check(h2hip_coeff_to_extended_bn254_fr_batch(ins.data(), k, outs.data(), ins.size(), extended_k, extended_omega.l, g_coset.l, g_coset_inv.l),
                     "coeff_to_extended_batch");
        return out;
    }

    // coeff_to_extended (poly/domain.rs:240-254)
    Polynomial<ExtendedLagrangeCoeff> coeff_to_extended(const Polynomial<Coeff>& a) const {
        if (a.values.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.values.len() == 1 << self.k");  // :244
        Polynomial<ExtendedLagrangeCoeff> out{std::vector<Fr>(extended_len())};
        engine_check(h2hip_coeff_to_extended_bn254_fr(a.values[0].l, k, out.values[0].l, extended_k, extended_omega.l, g_coset.l, g_coset_inv.l),
                     "coeff_to_extended");
        return out;
    }

    // upstream halo2's coeff_to_extended_part: rows j * P + part (P = 2^(extended_k - k)) of coeff_to_extended(a), 2^k elements
    std::vector<Fr> coeff_to_extended_part(const Polynomial<Coeff>& a, uint32_t part) const {
        if (a.values.size() != (size_t(1) << k)) throw std::logic_error("assertion failed: a.values.len() == 1 << self.k");
        if (part >> (extended_k - k)) throw std::logic_error("assertion failed: part < 1 << (self.extended_k - self.k)");
        std::vector<Fr> out(size_t(1) << k);
        engine_check(h2hip_coeff_to_extended_part_bn254_fr(a.values[0].l, k, extended_k, part, extended_omega.l, g_coset.l, g_coset_inv.l, out[0].l),
                     "coeff_to_extended_part");
        return out;
    }

    // extended_to_coeff (poly/domain.rs:281-303)
    std::vector<Fr> extended_to_coeff(Polynomial<ExtendedLagrangeCoeff> a) const {
        if (a.values.size() != extended_len()) throw std::logic_error("assertion failed: a.values.len() == self.extended_len()");  // :282
        engine_check(h2hip_extended_to_coeff_bn254_fr(a.values[0].l, extended_k, extended_omega_inv.l, extended_ifft_divisor.l, g_coset.l,
                                                      g_coset_inv.l),
                     "extended_to_coeff");
        a.values.resize(size_t(n * quotient_poly_degree));                                                                   // :299-300
        return std::move(a.values);
    }

    // divide_by_vanishing_poly (poly/domain.rs:307-326)
    Polynomial<ExtendedLagrangeCoeff> divide_by_vanishing_poly(Polynomial<ExtendedLagrangeCoeff> a) const {
        if (a.values.size() != extended_len()) throw std::logic_error("assertion failed: a.values.len() == self.extended_len()");  // :311
        engine_check(h2hip_divide_by_vanishing_poly_bn254_fr(a.values[0].l, extended_k, t_evaluations[0].l, uint32_t(t_evaluations.size())),
                     "divide_by_vanishing_poly");
        return a;
    }
};

struct Blind {
    Fr r;
};

namespace kzg {

// ParamsKZG<Bn256> (poly/kzg/commitment.rs:22-30): g / g_lagrange are pinned on the GPU for the
// life of the object (h2hip_bases_pin), the hook INTEGRATION.md section 3 describes.
class ParamsKZG {
   public:
    uint32_t k = 0;
    uint64_t n = 0;
    std::vector<G1Affine> g, g_lagrange;
    std::array<uint8_t, 128> g2{}, s_g2{};  // raw bytes: what poly::kzg::DualMSM::check (kzg.hpp) pairs with

    ParamsKZG() = default;
    ParamsKZG(const ParamsKZG&) = delete;
    ParamsKZG& operator=(const ParamsKZG&) = delete;
    ~ParamsKZG() { unpin(); }

    // setup (poly/kzg/commitment.rs:61-129) with the secret supplied: the reference draws `s` from its rng argument
    // (:72, "MUST NOT be used in production"); everything after that line is what runs here, on the GPU.
    // g2 = G2Affine::generator() and s_g2 = [s] g2 (:118-119) on the host (h2hip_g2_mul_bn254).
    static void setup(uint32_t k, const Fr& s, ParamsKZG& p) {
        if (k > Fr::S) throw std::logic_error("assertion failed: k <= E::Scalar::S");  // :64
        p.unpin();
        p.k = k;
        p.n = uint64_t(1) << k;
        p.g.resize(p.n);
        p.g_lagrange.resize(p.n);
        engine_check(h2hip_kzg_setup_bn254(k, s.l, p.g[0].x, p.g_lagrange[0].x), "h2hip_kzg_setup_bn254");
        p.g2 = serde::g2_generator();
        uint64_t in[16], out[16];
        std::memcpy(in, p.g2.data(), 128);
        engine_check(h2hip_g2_mul_bn254(in, s.l, out), "h2hip_g2_mul_bn254");
        std::memcpy(p.s_g2.data(), out, 128);
        p.pin();
    }
    // the reference's signature: `rng` is any callable returning an Fr (<E::Scalar>::random(rng), :72)
    template <class Rng>
    static void setup(uint32_t k, Rng&& rng, ParamsKZG& p) {
        const Fr s = rng();
        setup(k, s, p);
    }

    using SerdeFormat = halo2_proofs::SerdeFormat;  // helpers.rs:8-20

    // Params::read = read_custom(reader, SerdeFormat::RawBytes) (poly/kzg/commitment.rs:160-244, :300-302): k as u32 LE, then g,
    // g_lagrange, g2, s_g2 in the format's point encoding.  Processed: 32-B compressed G1 points, decompressed on the GPU
    // (h2hip_g1_decompress_bn254: one square root per point), 64-B compressed G2 points on the host.  RawBytes: 64-B Montgomery
    // points whose checks -- every coordinate below the modulus, every point on the curve (helpers.rs:15-18, read_raw) -- run on the
    // GPU (h2hip_g1_validate_bn254).  RawBytesUnchecked performs no checks (:19-20).
    static void read(std::istream& reader, ParamsKZG& p) { read_custom(reader, p, SerdeFormat::RawBytes); }
    static void read_custom(std::istream& reader, ParamsKZG& p, SerdeFormat format) {
        uint8_t kb[4];
        serde::read_exact(reader, kb, 4, "ParamsKZG::read");
        p.unpin();
        p.k = uint32_t(kb[0]) | uint32_t(kb[1]) << 8 | uint32_t(kb[2]) << 16 | uint32_t(kb[3]) << 24;
        if (p.k > Fr::S) throw std::runtime_error("ParamsKZG::read: k too large");
        p.n = uint64_t(1) << p.k;
        p.g.resize(p.n);
        p.g_lagrange.resize(p.n);
        uint64_t invalid[2];
        std::vector<uint8_t> packed(format == SerdeFormat::Processed ? p.n * 32 : 0);
        for (auto* v : {&p.g, &p.g_lagrange}) {
            if (format == SerdeFormat::Processed) {
                serde::read_exact(reader, packed.data(), packed.size(), "ParamsKZG::read");
                engine_check(h2hip_g1_decompress_bn254(packed.data(), p.n, (*v)[0].x, invalid), "ParamsKZG::read: invalid point encoding");
            } else {
                serde::read_exact(reader, v->data(), p.n * 64, "ParamsKZG::read");
                if (format == SerdeFormat::RawBytes)
                    engine_check(h2hip_g1_validate_bn254((*v)[0].x, p.n, invalid), "ParamsKZG::read: invalid point encoding");
            }
        }
        for (auto* pt : {&p.g2, &p.s_g2}) {
            if (format == SerdeFormat::Processed) {
                uint8_t c[64];
                serde::read_exact(reader, c, 64, "ParamsKZG::read");
                if (!serde::g2_from_bytes(c, *pt)) throw std::runtime_error("ParamsKZG::read: invalid point encoding");
            } else {
                serde::read_exact(reader, pt->data(), 128, "ParamsKZG::read");
                if (format == SerdeFormat::RawBytes && !serde::g2_is_valid(*pt)) throw std::runtime_error("ParamsKZG::read: invalid point encoding");
            }
        }
        p.pin();
    }

    // Params::write = write_custom(writer, SerdeFormat::RawBytes) (poly/kzg/commitment.rs:142-157, :296-298)
    void write(std::ostream& writer) const { write_custom(writer, SerdeFormat::RawBytes); }
    void write_custom(std::ostream& writer, SerdeFormat format) const {
        const char kb[4] = {char(k), char(k >> 8), char(k >> 16), char(k >> 24)};
        writer.write(kb, 4);
        std::vector<uint8_t> packed(format == SerdeFormat::Processed ? n * 32 : 0);
        for (const auto* v : {&g, &g_lagrange}) {
            if (format == SerdeFormat::Processed) {
                engine_check(h2hip_g1_compress_bn254((*v)[0].x, n, packed.data()), "h2hip_g1_compress_bn254");
                writer.write(reinterpret_cast<const char*>(packed.data()), std::streamsize(packed.size()));
            } else {
                writer.write(reinterpret_cast<const char*>(v->data()), std::streamsize(n * 64));
            }
        }
        for (const auto* pt : {&g2, &s_g2}) {
            if (format == SerdeFormat::Processed) {
                uint8_t c[64];
                serde::g2_to_bytes(*pt, c);
                writer.write(reinterpret_cast<const char*>(c), 64);
            } else {
                writer.write(reinterpret_cast<const char*>(pt->data()), 128);
            }
        }
    }

    // downsize (poly/kzg/commitment.rs:267-275)
    void downsize(uint32_t k_) {
        if (k_ > k) throw std::logic_error("assertion failed: k <= self.k");  // :268
        unpin();
        k = k_;
        n = uint64_t(1) << k;
        g.resize(n);                                                          // truncate, :273
        g_lagrange = arithmetic::g_to_lagrange(g, k);                         // :274
        pin();
    }

    // commit_lagrange (poly/kzg/commitment.rs:281-292); the blind is ignored there too
    G1 commit_lagrange(const Polynomial<LagrangeCoeff>& poly, const Blind&) const {
        if (g_lagrange.size() < poly.len()) throw std::logic_error("assertion failed: bases.len() >= size");  // :290
        return arithmetic::best_multiexp(poly.values, g_lagrange.data(), poly.len());                           // :291
    }

    // The column loop of create_proof (plonk/prover.rs:361-365: `params.commit_lagrange(poly, blind)` over all advice
    // polynomials) as one engine call; equal to calling commit_lagrange on each.
    std::vector<G1> commit_lagrange_many(const std::vector<const Polynomial<LagrangeCoeff>*>& polys) const {
        std::vector<G1> out(polys.size());
        if (polys.empty()) return out;
        const size_t size = polys[0]->len();
        if (g_lagrange.size() < size) throw std::logic_error("assertion failed: bases.len() >= size");            // :290
        std::vector<const uint64_t*> ptrs;
        for (auto* p : polys) {
            if (p->len() != size) throw std::logic_error("commit_lagrange_many: polynomials of different lengths");
            ptrs.push_back(p->values[0].l);
        }
        engine_check(h2hip_msm_bn254_batch(ptrs.data(), g_lagrange[0].x, size, ptrs.size(), out[0].x), "h2hip_msm_bn254_batch");
        return out;
    }

    // commit (poly/kzg/commitment.rs:327-334)
    G1 commit(const Polynomial<Coeff>& poly, const Blind&) const {
        if (g.size() < poly.len()) throw std::logic_error("assertion failed: bases.len() >= size");           // :332
        return arithmetic::best_multiexp(poly.values, g.data(), poly.len());                                   // :333
    }

    const std::vector<G1Affine>& get_g() const { return g; }  // :336-338

   private:
    bool pinned_ = false;
    void pin() {
        engine_check(h2hip_bases_pin(g[0].x, g.size()), "bases_pin(g)");
        if (int rc = h2hip_bases_pin(g_lagrange[0].x, g_lagrange.size())) {  // do not leave g pinned behind a failed object
            std::string msg = std::string("bases_pin(g_lagrange): ") + h2hip_last_error();
            (void)h2hip_bases_unpin(g[0].x);
            (void)rc;
            throw std::runtime_error(msg);
        }
        pinned_ = true;
    }
    void unpin() {
        if (!pinned_) return;
        (void)h2hip_bases_unpin(g[0].x);
        (void)h2hip_bases_unpin(g_lagrange[0].x);
        pinned_ = false;
    }
};

}  // namespace kzg
}  // namespace poly

// The grand-product columns of create_proof (h2hip_permutation_products_bn254 / h2hip_lookup_products_bn254).  Blinding values are the
// caller's, drawn in the reference's order: b per set or lookup, set-major.
namespace plonk {

// vanishing::Argument::commit (plonk/vanishing/prover.rs:36-67): the random polynomial of 2^k coefficients as ONE engine call instead of
// 2^k serial draws, then its blind -- the stream's blocks [c, c + 2^k) and c + 2^k, the order the reference's loop draws in -- and the
// commitment over the pinned g.  This mirror holds host vectors, so the column is generated on the GPU and comes back once; the
// resident form, where it never leaves HBM, is h2hip_fr_random_bn254_device followed by h2hip_msm_bn254_device.  Writing the
// commitment to the transcript (:61) stays with the caller.
namespace vanishing {
struct Committed {
    poly::Polynomial<poly::Coeff> random_poly;
    poly::Blind random_blind;
};
struct Argument {
    static Committed commit(const poly::kzg::ParamsKZG& params, const poly::EvaluationDomain& domain, FrRng& rng, G1* commitment) {
        Committed c{{std::vector<Fr>(domain.n)}, {Fr::zero()}};  // domain.empty_coeff(), :52
        rng.fill(c.random_poly.values.data(), c.random_poly.len());  // :53-55
        c.random_blind.r = rng();                                     // :57
        *commitment = params.commit(c.random_poly, c.random_blind);   // :60
        return c;
    }
};
}  // namespace vanishing

// permutation::Argument::commit's z columns (plonk/permutation/prover.rs:96-166): one per set of chunk_len columns, last_z carried
// from set to set.  columns[c] = p_c resolved from advice / fixed / instance, permutations[c] = pkey.permutations[c].
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> permutation_products(
    const poly::EvaluationDomain& domain, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& columns,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& permutations, size_t chunk_len, const Fr& beta, const Fr& gamma,
    const std::vector<Fr>& blinding, size_t blinding_factors) {
    if (columns.size() != permutations.size()) throw std::logic_error("columns and permutations differ in length");
    if (chunk_len == 0) throw std::logic_error("chunk_len == 0");
    const size_t n_sets = (columns.size() + chunk_len - 1) / chunk_len;
    if (blinding.size() != n_sets * blinding_factors) throw std::logic_error("blinding: n_sets * blinding_factors values expected");
    std::vector<const uint64_t*> p, s;
    for (size_t c = 0; c < columns.size(); c++) {
        if (columns[c]->len() != domain.n || permutations[c]->len() != domain.n) throw std::logic_error("column length != n");
        p.push_back(columns[c]->values[0].l);
        s.push_back(permutations[c]->values[0].l);
    }
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> z(n_sets, poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> zp;
    for (auto& col : z) zp.push_back(col.values[0].l);
    Fr delta = Fr::delta();
    engine_check(h2hip_permutation_products_bn254(domain.k, domain.omega.l, delta.l, beta.l, gamma.l, p.data(), s.data(), uint32_t(p.size()),
                                                  uint32_t(chunk_len), blinding.empty() ? nullptr : blinding[0].l, uint32_t(blinding_factors),
                                                  zp.data()),
                 "permutation_products");
    return z;
}

// lookup::Permuted::commit_product's z columns (plonk/lookup/prover.rs:194-249), one per lookup: inputs / tables are the compressed
// expressions A, S, permuted_inputs / permuted_tables A', S'
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> lookup_products(
    const poly::EvaluationDomain& domain, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& tables,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& permuted_inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& permuted_tables, const Fr& beta, const Fr& gamma,
    const std::vector<Fr>& blinding, size_t blinding_factors) {
    const size_t count = inputs.size();
    if (tables.size() != count || permuted_inputs.size() != count || permuted_tables.size() != count)
        throw std::logic_error("lookup columns differ in count");
    if (blinding.size() != count * blinding_factors) throw std::logic_error("blinding: count * blinding_factors values expected");
    std::vector<const uint64_t*> a, s, ap, sp;
    for (size_t j = 0; j < count; j++) {
        for (auto* col : {inputs[j], tables[j], permuted_inputs[j], permuted_tables[j]})
            if (col->len() != domain.n) throw std::logic_error("column length != n");
        a.push_back(inputs[j]->values[0].l);
        s.push_back(tables[j]->values[0].l);
        ap.push_back(permuted_inputs[j]->values[0].l);
        sp.push_back(permuted_tables[j]->values[0].l);
    }
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> z(count, poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> zp;
    for (auto& col : z) zp.push_back(col.values[0].l);
    engine_check(h2hip_lookup_products_bn254(domain.k, beta.l, gamma.l, a.data(), s.data(), ap.data(), sp.data(), count,
                                             blinding.empty() ? nullptr : blinding[0].l, uint32_t(blinding_factors), zp.data()),
                 "lookup_products");
    return z;
}

// The shuffle argument's z columns (shuffle::Argument::commit_product of upstream PSE halo2, which is later than the reference:
// include/halo2hip.h states the definition), one per shuffle: inputs / shuffles are the compressed expressions A, S
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> shuffle_products(
    const poly::EvaluationDomain& domain, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& shuffles, const Fr& gamma, const std::vector<Fr>& blinding,
    size_t blinding_factors) {
    const size_t count = inputs.size();
    if (shuffles.size() != count) throw std::logic_error("shuffle columns differ in count");
    if (blinding.size() != count * blinding_factors) throw std::logic_error("blinding: count * blinding_factors values expected");
    std::vector<const uint64_t*> a, s;
    for (size_t j = 0; j < count; j++) {
        if (inputs[j]->len() != domain.n || shuffles[j]->len() != domain.n) throw std::logic_error("column length != n");
        a.push_back(inputs[j]->values[0].l);
        s.push_back(shuffles[j]->values[0].l);
    }
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> z(count, poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> zp;
    for (auto& col : z) zp.push_back(col.values[0].l);
    engine_check(h2hip_shuffle_products_bn254(domain.k, gamma.l, a.data(), s.data(), count, blinding.empty() ? nullptr : blinding[0].l,
                                              uint32_t(blinding_factors), zp.data()),
                 "shuffle_products");
    return z;
}

// The logUp (mv-lookup) argument's multiplicity columns, one per argument (include/halo2hip.h states the definition): inputs[j] are the
// compressed input columns that share tables[j].  Throws EngineError when an input value is missing from its table.
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> mvlookup_multiplicities(
    const poly::EvaluationDomain& domain, const std::vector<std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>>& inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& tables, size_t blinding_factors) {
    const size_t count = tables.size();
    if (inputs.size() != count) throw std::logic_error("mv-lookup inputs and tables differ in count");
    std::vector<const uint64_t*> f, t;
    std::vector<uint32_t> n_inputs;
    for (size_t j = 0; j < count; j++) {
        if (tables[j]->len() != domain.n) throw std::logic_error("column length != n");
        t.push_back(tables[j]->values[0].l);
        n_inputs.push_back(uint32_t(inputs[j].size()));
        for (const auto* c : inputs[j]) {
            if (c->len() != domain.n) throw std::logic_error("column length != n");
            f.push_back(c->values[0].l);
        }
    }
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> m(count, poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> mp;
    for (auto& col : m) mp.push_back(col.values[0].l);
    engine_check(h2hip_mvlookup_multiplicities_bn254(domain.k, f.data(), n_inputs.data(), t.data(), count, uint32_t(blinding_factors), mp.data()),
                 "mvlookup_multiplicities");
    return m;
}

// ... and its grand sums phi, one per argument, from the same columns and the multiplicities
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> mvlookup_sums(
    const poly::EvaluationDomain& domain, const std::vector<std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>>& inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& tables, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& m,
    const Fr& beta, const std::vector<Fr>& blinding, size_t blinding_factors) {
    const size_t count = tables.size();
    if (inputs.size() != count || m.size() != count) throw std::logic_error("mv-lookup columns differ in count");
    if (blinding.size() != count * blinding_factors) throw std::logic_error("blinding: count * blinding_factors values expected");
    std::vector<const uint64_t*> f, t, mm;
    std::vector<uint32_t> n_inputs;
    for (size_t j = 0; j < count; j++) {
        if (tables[j]->len() != domain.n || m[j]->len() != domain.n) throw std::logic_error("column length != n");
        t.push_back(tables[j]->values[0].l);
        mm.push_back(m[j]->values[0].l);
        n_inputs.push_back(uint32_t(inputs[j].size()));
        for (const auto* c : inputs[j]) {
            if (c->len() != domain.n) throw std::logic_error("column length != n");
            f.push_back(c->values[0].l);
        }
    }
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> phi(count, poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> pp;
    for (auto& col : phi) pp.push_back(col.values[0].l);
    engine_check(h2hip_mvlookup_sums_bn254(domain.k, beta.l, f.data(), n_inputs.data(), t.data(), mm.data(), count,
                                           blinding.empty() ? nullptr : blinding[0].l, uint32_t(blinding_factors), pp.data()),
                 "mvlookup_sums");
    return phi;
}

// lookup::Argument::commit_permuted's compression (plonk/lookup/prover.rs:90-115): out[g] = graphs[g] over the n Lagrange rows.  Each
// graph is one side of a lookup, add_expression of its expressions then Horner(Constant(0), parts, Theta) (evaluation.hpp
// lookup_compress_graphs builds them); fixed / advice / instance are the Lagrange columns the graphs index.
inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> lookup_compress(
    const poly::EvaluationDomain& domain, const std::vector<h2hip_graph>& graphs, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& fixed,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& advice, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& instance,
    const std::vector<Fr>& challenges, const Fr& theta) {
    auto ptrs = [&](const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& cols) {
        std::vector<const uint64_t*> p;
        for (auto* c : cols) {
            if (c->len() != domain.n) throw std::logic_error("column length != n");
            p.push_back(c->values[0].l);
        }
        return p;
    };
    const auto f = ptrs(fixed), a = ptrs(advice), i = ptrs(instance);
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> out(graphs.size(), poly::Polynomial<poly::LagrangeCoeff>{std::vector<Fr>(domain.n)});
    std::vector<uint64_t*> op;
    for (auto& col : out) op.push_back(col.values[0].l);
    engine_check(h2hip_lookup_compress_bn254(domain.k, f.data(), uint32_t(f.size()), a.data(), uint32_t(a.size()), i.data(), uint32_t(i.size()),
                                             challenges.empty() ? nullptr : challenges[0].l, uint32_t(challenges.size()), theta.l, graphs.data(),
                                             graphs.size(), op.data()),
                 "lookup_compress");
    return out;
}

// permute_expression_pair (plonk/lookup/prover.rs:391-475) for every lookup: returns (A'_j, S'_j) per lookup.  blinding holds
// 2(blinding_factors + 1) values per lookup, the A' rows then the S' rows, drawn in the reference's order.
// A value of an input missing from its table is the reference's Error::ConstraintSystemFailure: std::domain_error here.
inline std::vector<std::pair<poly::Polynomial<poly::LagrangeCoeff>, poly::Polynomial<poly::LagrangeCoeff>>> lookup_permute(
    const poly::EvaluationDomain& domain, const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& inputs,
    const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& tables, const std::vector<Fr>& blinding, size_t blinding_factors) {
    const size_t count = inputs.size();
    if (tables.size() != count) throw std::logic_error("lookup columns differ in count");
    if (blinding.size() != count * 2 * (blinding_factors + 1)) throw std::logic_error("blinding: count * 2(blinding_factors + 1) values expected");
    std::vector<const uint64_t*> a, s;
    for (size_t j = 0; j < count; j++) {
        if (inputs[j]->len() != domain.n || tables[j]->len() != domain.n) throw std::logic_error("column length != n");
        a.push_back(inputs[j]->values[0].l);
        s.push_back(tables[j]->values[0].l);
    }
    using Col = poly::Polynomial<poly::LagrangeCoeff>;
    std::vector<std::pair<Col, Col>> out(count, {Col{std::vector<Fr>(domain.n)}, Col{std::vector<Fr>(domain.n)}});
    std::vector<uint64_t*> pa, pt;
    for (auto& p : out) {
        pa.push_back(p.first.values[0].l);
        pt.push_back(p.second.values[0].l);
    }
    const int rc = h2hip_lookup_permute_bn254(domain.k, a.data(), s.data(), count, blinding.empty() ? nullptr : blinding[0].l,
                                              uint32_t(blinding_factors), pa.data(), pt.data());
    if (rc == H2HIP_ELOOKUP) throw std::domain_error(std::string("lookup_permute: ") + h2hip_last_error());
    engine_check(rc, "lookup_permute");
    return out;
}

// batch_invert_assigned (poly.rs:180-209).  Assigned<F> (plonk/assigned.rs): Zero, Trivial(x) or Rational(numerator, denominator).
struct Assigned {
    enum Kind { Zero, Trivial, Rational } kind = Zero;
    Fr numerator = Fr::zero(), denominator = Fr::one();
    static Assigned trivial(const Fr& x) { return {Trivial, x, Fr::one()}; }
    static Assigned rational(const Fr& n, const Fr& d) { return {Rational, n, d}; }
};

inline std::vector<poly::Polynomial<poly::LagrangeCoeff>> batch_invert_assigned(const poly::EvaluationDomain& domain,
                                                                                const std::vector<std::vector<Assigned>>& assigned) {
    const size_t m = assigned.size();
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> out(m);
    std::vector<std::vector<uint32_t>> rows(m);
    std::vector<std::vector<Fr>> denoms(m);
    std::vector<const uint32_t*> rp(m);
    std::vector<const uint64_t*> np(m), dp(m);
    std::vector<uint64_t*> op(m);
    std::vector<size_t> counts(m);
    for (size_t j = 0; j < m; j++) {
        if (assigned[j].size() != domain.n) throw std::logic_error("column length != n");
        out[j].values.resize(domain.n);
        for (size_t i = 0; i < domain.n; i++) {
            const Assigned& a = assigned[j][i];
            out[j].values[i] = a.kind == Assigned::Zero ? Fr::zero() : a.numerator;  // numerator(), assigned.rs
            if (a.kind == Assigned::Rational) {                                       // denominator() is Some: :183-200
                rows[j].push_back(uint32_t(i));
                denoms[j].push_back(a.denominator);
            }
        }
        counts[j] = rows[j].size();
        rp[j] = rows[j].data();
        dp[j] = denoms[j].empty() ? nullptr : denoms[j][0].l;
        np[j] = op[j] = out[j].values[0].l;  // in place: out == numerators
    }
    engine_check(h2hip_batch_invert_assigned_bn254(domain.k, np.data(), rp.data(), counts.data(), dp.data(), m, op.data()), "batch_invert_assigned");
    return out;
}

namespace permutation {
struct ProvingKey {  // plonk/permutation.rs ProvingKey
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> permutations;
    std::vector<poly::Polynomial<poly::Coeff>> polys;
    std::vector<poly::Polynomial<poly::ExtendedLagrangeCoeff>> cosets;
};
struct VerifyingKey {
    std::vector<G1Affine> commitments;
};

namespace keygen {
using Cell = std::pair<uint32_t, uint32_t>;  // (column, row)

// What Assembly and CopyAssembly share: build_vk / build_pk's columns (:105-242) from a mapping, on the engine
inline ProvingKey build_from_mapping(const std::vector<std::vector<Cell>>& mapping, const poly::EvaluationDomain& domain, bool perms, bool polys,
                                     bool cosets) {
    const size_t m = mapping.size();
    static_assert(sizeof(Cell) == 8, "a (column, row) pair is two interleaved uint32_t");
    ProvingKey pk;
    std::vector<const uint32_t*> mp(m);
    std::vector<uint64_t*> a(m), b(m), c(m);
    if (perms) pk.permutations.resize(m);
    if (polys) pk.polys.resize(m);
    if (cosets) pk.cosets.resize(m);
    for (size_t j = 0; j < m; j++) {
        if (mapping[j].size() != domain.n) throw std::logic_error("mapping column length != n");
        mp[j] = &mapping[j][0].first;
        if (perms) pk.permutations[j].values.resize(domain.n), a[j] = pk.permutations[j].values[0].l;
        if (polys) pk.polys[j].values.resize(domain.n), b[j] = pk.polys[j].values[0].l;
        if (cosets) pk.cosets[j].values.resize(domain.extended_len()), c[j] = pk.cosets[j].values[0].l;
    }
    Fr delta = Fr::delta();
    engine_check(h2hip_permutation_keygen_bn254(domain.k, domain.omega.l, domain.omega_inv.l, domain.ifft_divisor.l, domain.extended_k,
                                                domain.extended_omega.l, domain.g_coset.l, domain.g_coset_inv.l, delta.l, mp.data(), uint32_t(m),
                                                perms ? a.data() : nullptr, polys ? b.data() : nullptr, cosets ? c.data() : nullptr),
                 "permutation_keygen");
    return pk;
}
// build_vk's commitments (:153-162): the sigma columns committed in Lagrange form as one batch
inline VerifyingKey commit_permutations(const poly::kzg::ParamsKZG& params, const ProvingKey& pk) {
    std::vector<const poly::Polynomial<poly::LagrangeCoeff>*> ptrs;
    for (auto& c : pk.permutations) ptrs.push_back(&c);
    VerifyingKey vk;
    for (auto& c : params.commit_lagrange_many(ptrs)) vk.commitments.push_back(c.to_affine());
    return vk;
}

// permutation::keygen::Assembly (plonk/permutation/keygen.rs:16-242); columns are the argument's column indices
struct Assembly {
    using Cell = keygen::Cell;
    std::vector<std::vector<Cell>> mapping, aux;
    std::vector<std::vector<size_t>> sizes;

    Assembly(size_t n, size_t n_columns) {  // :28-46
        for (size_t i = 0; i < n_columns; i++) {
            std::vector<Cell> col;
            for (size_t j = 0; j < n; j++) col.push_back({uint32_t(i), uint32_t(j)});
            mapping.push_back(col);
        }
        aux = mapping;
        sizes.assign(n_columns, std::vector<size_t>(n, 1));
    }

    void copy(size_t left_column, size_t left_row, size_t right_column, size_t right_row) {  // :48-103
        if (left_column >= mapping.size() || right_column >= mapping.size()) throw std::out_of_range("ColumnNotInPermutation");
        if (left_row >= mapping[left_column].size() || right_row >= mapping[right_column].size()) throw std::out_of_range("BoundsFailure");  // :67-71
        Cell left_cycle = aux[left_column][left_row], right_cycle = aux[right_column][right_row];  // :75-76
        if (left_cycle == right_cycle) return;                                                      // :79-81
        if (sizes[left_cycle.first][left_cycle.second] < sizes[right_cycle.first][right_cycle.second]) std::swap(left_cycle, right_cycle);
        sizes[left_cycle.first][left_cycle.second] += sizes[right_cycle.first][right_cycle.second];  // :88
        Cell i = right_cycle;                                                                       // :89-96
        do {
            aux[i.first][i.second] = left_cycle;
            i = mapping[i.first][i.second];
        } while (i != right_cycle);
        std::swap(mapping[left_column][left_row], mapping[right_column][right_row]);                // :98-100
    }

    // build_vk (:105-165): the sigma columns on the engine, committed in Lagrange form as one batch
    VerifyingKey build_vk(const poly::kzg::ParamsKZG& params, const poly::EvaluationDomain& domain) const {
        return commit_permutations(params, build(domain, true, false, false));  // :153-162
    }

    // build_pk (:167-242)
    ProvingKey build_pk(const poly::EvaluationDomain& domain) const { return build(domain, true, true, true); }

   private:
    ProvingKey build(const poly::EvaluationDomain& domain, bool perms, bool polys, bool cosets) const {
        return build_from_mapping(mapping, domain, perms, polys, cosets);
    }
};

// The copy constraints recorded, and the mapping built from them on the engine (h2hip_permutation_mapping): the ordered mapping of
// include/halo2hip.h -- every cell to the next cell of its connected component in ascending column * n + row order -- which does not depend
// on the order of the copy calls.  Same copy / build_vk / build_pk surface as Assembly, same cycles for the same constraints; the key is
// valid for the circuit, not byte-identical to the one Assembly builds.
struct CopyAssembly {
    using Cell = keygen::Cell;
    size_t n, n_columns;
    std::vector<uint32_t> copies;  // (left_column, left_row, right_column, right_row) per copy

    CopyAssembly(size_t n_, size_t n_columns_) : n(n_), n_columns(n_columns_) {
        if (n == 0 || (n & (n - 1))) throw std::logic_error("n must be a power of two");
    }

    void copy(size_t left_column, size_t left_row, size_t right_column, size_t right_row) {  // Assembly::copy's checks (:55-71)
        if (left_column >= n_columns || right_column >= n_columns) throw std::out_of_range("ColumnNotInPermutation");
        if (left_row >= n || right_row >= n) throw std::out_of_range("BoundsFailure");
        for (size_t v : {left_column, left_row, right_column, right_row}) copies.push_back(uint32_t(v));
    }

    std::vector<std::vector<Cell>> mapping() const {
        uint32_t k = 0;
        while ((size_t(1) << k) < n) k++;
        std::vector<std::vector<Cell>> mp(n_columns, std::vector<Cell>(n));
        std::vector<uint32_t*> ptrs(n_columns);
        for (size_t j = 0; j < n_columns; j++) ptrs[j] = &mp[j][0].first;
        engine_check(h2hip_permutation_mapping(k, uint32_t(n_columns), copies.data(), copies.size() / 4, ptrs.data()), "permutation_mapping");
        return mp;
    }

    VerifyingKey build_vk(const poly::kzg::ParamsKZG& params, const poly::EvaluationDomain& domain) const {
        return commit_permutations(params, build_from_mapping(mapping(), domain, true, false, false));
    }
    ProvingKey build_pk(const poly::EvaluationDomain& domain) const { return build_from_mapping(mapping(), domain, true, true, true); }
};
}  // namespace keygen
}  // namespace permutation

// The columns of plonk::ProvingKey that keygen_pk computes (plonk/keygen.rs:298-366), given what synthesis left behind: the fixed columns
// as Assigned values and the permutation assembly
struct ProvingKeyColumns {
    poly::Polynomial<poly::ExtendedLagrangeCoeff> l0, l_last, l_active_row;
    std::vector<poly::Polynomial<poly::LagrangeCoeff>> fixed_values;
    std::vector<poly::Polynomial<poly::Coeff>> fixed_polys;
    std::vector<poly::Polynomial<poly::ExtendedLagrangeCoeff>> fixed_cosets;
    permutation::ProvingKey permutation;
};

template <class AssemblyT>  // permutation::keygen::Assembly or CopyAssembly
inline ProvingKeyColumns keygen_pk_with(const poly::EvaluationDomain& domain, const std::vector<std::vector<Assigned>>& fixed,
                                        const AssemblyT& assembly, size_t blinding_factors) {
    ProvingKeyColumns pk;
    pk.fixed_values = batch_invert_assigned(domain, fixed);                    // :298
    pk.fixed_polys = domain.lagrange_to_coeff_batch(pk.fixed_values);          // :306-309
    pk.fixed_cosets = domain.coeff_to_extended_batch(pk.fixed_polys);          // :311-314
    pk.permutation = assembly.build_pk(domain);                                // :316-318
    for (auto* c : {&pk.l0, &pk.l_last, &pk.l_active_row}) c->values.resize(domain.extended_len());
    engine_check(h2hip_key_lagrange_columns_bn254(domain.k, domain.omega_inv.l, domain.ifft_divisor.l, domain.extended_k, domain.extended_omega.l,
                                                  domain.g_coset.l, domain.g_coset_inv.l, uint32_t(blinding_factors), pk.l0.values[0].l,
                                                  pk.l_last.values[0].l, pk.l_active_row.values[0].l),
                 "key_lagrange_columns");                                      // :320-351
    return pk;
}
inline ProvingKeyColumns keygen_pk(const poly::EvaluationDomain& domain, const std::vector<std::vector<Assigned>>& fixed,
                                   const permutation::keygen::Assembly& assembly, size_t blinding_factors) {
    return keygen_pk_with(domain, fixed, assembly, blinding_factors);
}
// ... from the recorded copy constraints: the permutation's columns are those of the ordered mapping (valid, not byte-identical)
inline ProvingKeyColumns keygen_pk(const poly::EvaluationDomain& domain, const std::vector<std::vector<Assigned>>& fixed,
                                   const permutation::keygen::CopyAssembly& assembly, size_t blinding_factors) {
    return keygen_pk_with(domain, fixed, assembly, blinding_factors);
}

}  // namespace plonk

// The three column-wide loops of MockProver::verify (dev.rs:603-1300) over the prover's own columns: h2hip_check_gates_bn254,
// h2hip_check_lookups_bn254 (on columns compressed with the caller's theta) and h2hip_check_permutation_bn254.  MockProver's regions,
// names, CellNotAssigned, Poison and selector checks are host bookkeeping and not mirrored.
namespace dev {

struct VerifyFailure {
    // index: the gate polynomial (graph), the lookup, the permutation column, the shuffle, the mv-lookup's input column (counted over all arguments)
    enum Kind { Gate, Lookup, Permutation, Shuffle, MvLookup } kind;
    size_t index;
    uint32_t row;
    bool operator==(const VerifyFailure& o) const { return kind == o.kind && index == o.index && row == o.row; }
};

struct Columns {
    std::vector<const poly::Polynomial<poly::LagrangeCoeff>*> fixed, advice, instance;
    std::vector<Fr> challenges;
};

// gate_graphs: one graph per gate polynomial (evaluation.hpp gate_check_graphs); lookup_graphs: input side then table side of every lookup
// (evaluation.hpp lookup_compress_graphs), compressed with theta; permutation_columns: the argument's columns, resolved, with their
// assembly (nullptr: no copy constraint).  Failures in verify's order (dev.rs:933-938): gates, lookups, permutation; of each
// constraint at most its max_rows lowest rows.  An empty vector is a satisfied witness.  shuffle_graphs: input side then shuffle side of
// every shuffle (the argument of upstream PSE halo2; the same compression graphs), reported after the lookups; none by default.
inline std::vector<VerifyFailure> verify(const poly::EvaluationDomain& domain, const Columns& cols, const std::vector<h2hip_graph>& gate_graphs,
                                         const std::vector<h2hip_graph>& lookup_graphs, const Fr& theta, size_t blinding_factors,
                                         const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& permutation_columns,
                                         const plonk::permutation::keygen::Assembly* assembly, uint32_t max_rows = 64,
                                         const std::vector<h2hip_graph>& shuffle_graphs = {}, const std::vector<h2hip_graph>& mvlookup_graphs = {},
                                         const std::vector<uint32_t>& mvlookup_n_inputs = {}) {
    auto ptrs = [&](const std::vector<const poly::Polynomial<poly::LagrangeCoeff>*>& cs) {
        std::vector<const uint64_t*> p;
        for (auto* c : cs) {
            if (c->len() != domain.n) throw std::logic_error("column length != n");
            p.push_back(c->values[0].l);
        }
        return p;
    };
    std::vector<VerifyFailure> out;
    std::vector<uint64_t> counts;
    std::vector<uint32_t> rows;
    auto prepare = [&](size_t items) {
        counts.assign(items, 0);
        rows.assign(items * max_rows, UINT32_MAX);
    };
    auto collect = [&](VerifyFailure::Kind kind) {
        for (size_t j = 0; j < counts.size(); j++)
            for (size_t t = 0; t < max_rows && t < counts[j]; t++) out.push_back({kind, j, rows[j * max_rows + t]});
    };
    if (!gate_graphs.empty()) {
        const auto f = ptrs(cols.fixed), a = ptrs(cols.advice), i = ptrs(cols.instance);
        prepare(gate_graphs.size());
        engine_check(h2hip_check_gates_bn254(domain.k, f.data(), uint32_t(f.size()), a.data(), uint32_t(a.size()), i.data(), uint32_t(i.size()),
                                             cols.challenges.empty() ? nullptr : cols.challenges[0].l, uint32_t(cols.challenges.size()),
                                             gate_graphs.data(), gate_graphs.size(), max_rows, counts.data(), rows.data()),
                     "check_gates");
        collect(VerifyFailure::Gate);
    }
    if (!lookup_graphs.empty()) {
        if (lookup_graphs.size() % 2) throw std::logic_error("lookup_graphs: an input and a table graph per lookup expected");
        const auto comp = plonk::lookup_compress(domain, lookup_graphs, cols.fixed, cols.advice, cols.instance, cols.challenges, theta);
        std::vector<const uint64_t*> in, tab;
        for (size_t j = 0; j < comp.size(); j += 2) {
            in.push_back(comp[j].values[0].l);
            tab.push_back(comp[j + 1].values[0].l);
        }
        prepare(in.size());
        engine_check(h2hip_check_lookups_bn254(domain.k, in.data(), tab.data(), in.size(), uint32_t(blinding_factors), max_rows, counts.data(),
                                               rows.data()),
                     "check_lookups");
        collect(VerifyFailure::Lookup);
    }
    if (!shuffle_graphs.empty()) {
        if (shuffle_graphs.size() % 2) throw std::logic_error("shuffle_graphs: an input and a shuffle graph per shuffle expected");
        const auto comp = plonk::lookup_compress(domain, shuffle_graphs, cols.fixed, cols.advice, cols.instance, cols.challenges, theta);
        std::vector<const uint64_t*> in, sh;
        for (size_t j = 0; j < comp.size(); j += 2) {
            in.push_back(comp[j].values[0].l);
            sh.push_back(comp[j + 1].values[0].l);
        }
        prepare(in.size());
        engine_check(h2hip_check_shuffles_bn254(domain.k, in.data(), sh.data(), in.size(), uint32_t(blinding_factors), max_rows, counts.data(),
                                                rows.data()),
                     "check_shuffles");
        collect(VerifyFailure::Shuffle);
    }
    // mv-lookups (the logUp argument; mv_lookup::Argument::compress_graphs of every argument, K_j inputs then the table, with
    // mvlookup_n_inputs[j] = K_j): the lookup check with the table repeated per input column, reported after the shuffles
    if (!mvlookup_graphs.empty()) {
        const auto comp = plonk::lookup_compress(domain, mvlookup_graphs, cols.fixed, cols.advice, cols.instance, cols.challenges, theta);
        std::vector<const uint64_t*> in, tab;
        size_t at = 0;
        for (uint32_t K : mvlookup_n_inputs) {
            if (at + K + 1 > comp.size()) throw std::logic_error("mvlookup_graphs: K + 1 graphs per argument expected");
            for (uint32_t t = 0; t < K; t++) {
                in.push_back(comp[at + t].values[0].l);
                tab.push_back(comp[at + K].values[0].l);
            }
            at += K + 1;
        }
        if (at != comp.size()) throw std::logic_error("mvlookup_graphs: K + 1 graphs per argument expected");
        prepare(in.size());
        engine_check(h2hip_check_lookups_bn254(domain.k, in.data(), tab.data(), in.size(), uint32_t(blinding_factors), max_rows, counts.data(),
                                               rows.data()),
                     "check_lookups");
        collect(VerifyFailure::MvLookup);
    }
    if (assembly && !permutation_columns.empty()) {
        const auto p = ptrs(permutation_columns);
        if (assembly->mapping.size() != p.size()) throw std::logic_error("permutation columns and assembly differ in count");
        std::vector<const uint32_t*> mp;
        for (const auto& col : assembly->mapping) {
            if (col.size() != domain.n) throw std::logic_error("mapping column length != n");
            mp.push_back(&col[0].first);
        }
        prepare(p.size());
        engine_check(h2hip_check_permutation_bn254(domain.k, p.data(), mp.data(), uint32_t(p.size()), max_rows, counts.data(), rows.data()),
                     "check_permutation");
        collect(VerifyFailure::Permutation);
    }
    return out;
}

}  // namespace dev

// The KZG multiopen provers restated over the engine's primitive.  The caller builds the sets (construct_intermediate_sets), draws the
// challenges from its transcript and commits; the engine takes ordered scalars only.
namespace poly {
namespace kzg {
namespace multiopen {

// one point of GWC with the polynomials queried there and their evaluations, in construct_intermediate_sets' order
struct PointQueries {
    Fr point;
    std::vector<std::pair<const Polynomial<Coeff>*, Fr>> queries;
};

// GWC's witness polynomials (gwc/prover.rs:61-89): per point, (sum v^i p_i - sum v^i e_i) / (X - z), n - 1 coefficients each
inline std::vector<Polynomial<Coeff>> gwc_witnesses(const std::vector<PointQueries>& sets, const Fr& v) {
    std::vector<Polynomial<Coeff>> out;
    for (auto& set : sets) {
        const auto pw = arithmetic::powers(v, set.queries.size());
        std::vector<const std::vector<Fr>*> polys;
        Fr eval_batch = Fr::zero();
        for (size_t i = 0; i < set.queries.size(); i++) {
            polys.push_back(&set.queries[i].first->values);
            eval_batch = eval_batch + pw[i] * set.queries[i].second;
        }
        const size_t n = polys.at(0)->size();
        out.push_back(Polynomial<Coeff>{arithmetic::poly_combine(polys, pw, {eval_batch}, {set.point}, Fr::one(), n - 1)});
    }
    return out;
}

// one rotation set of SHPLONK: its points and, per polynomial, the evaluations at each point
struct RotationSet {
    std::vector<Fr> points;
    std::vector<std::pair<const Polynomial<Coeff>*, std::vector<Fr>>> commitments;
};

struct ShplonkQuotients {
    Polynomial<Coeff> h_x;    // the first quotient (shplonk/prover.rs:196-203), n coefficients
    Polynomial<Coeff> final_poly;  // l_x / (X - u) normalised by z_diffs[0]^-1 (:261-275), n - 1 coefficients
};

// SHPLONK's two stages (shplonk/prover.rs:138-275).  squeeze_u(h_x) is called after the first quotient is formed: the caller commits h_x,
// writes it to the transcript and returns u, so that u is drawn after h as in the reference.
template <class SqueezeU>
inline ShplonkQuotients shplonk(const std::vector<RotationSet>& sets, const Fr& y, const Fr& v, SqueezeU squeeze_u) {
    if (sets.empty()) throw std::logic_error("shplonk: no rotation sets");
    const size_t n = sets[0].commitments.at(0).first->len();
    std::vector<std::vector<Fr>> interp;  // low_degree_equivalent of every commitment, set-major
    std::vector<Fr> super_set;
    for (auto& set : sets) {
        for (auto& c : set.commitments) interp.push_back(arithmetic::lagrange_interpolate(set.points, c.second));
        for (auto& p : set.points) {
            bool seen = false;
            for (auto& q : super_set) seen = seen || q == p;
            if (!seen) super_set.push_back(p);
        }
    }
    // stage 1: h_x = sum_i v^i div_by_vanishing(sum_j y^j (p_ij - R_ij), points_i), each zero-padded to n
    std::vector<Fr> h(n, Fr::zero());
    const auto pv = arithmetic::powers(v, sets.size());
    size_t c0 = 0;
    for (size_t i = 0; i < sets.size(); i++) {
        const auto& set = sets[i];
        const auto py = arithmetic::powers(y, set.commitments.size());
        std::vector<const std::vector<Fr>*> polys;
        std::vector<Fr> sub(set.points.size(), Fr::zero());
        for (size_t j = 0; j < set.commitments.size(); j++) {
            polys.push_back(&set.commitments[j].first->values);
            for (size_t t = 0; t < sub.size(); t++) sub[t] = sub[t] + py[j] * interp[c0 + j][t];
        }
        c0 += set.commitments.size();
        auto q = arithmetic::poly_combine(polys, py, sub, set.points, pv[i], n);
        for (size_t t = 0; t < n; t++) h[t] = h[t] + q[t];  // the host form; a resident prover accumulates on the device
    }
    ShplonkQuotients out{Polynomial<Coeff>{h}, Polynomial<Coeff>{}};
    const Fr u = squeeze_u(out.h_x);
    // stage 2: l_x = sum_i v^i z_i sum_j y^j (p_ij - R_ij(u)) - Z_T(u) h_x, divided by (X - u), times z_diffs[0]^-1
    std::vector<const std::vector<Fr>*> polys;
    std::vector<Fr> scalars;
    Fr constant = Fr::zero(), z0 = Fr::zero();
    c0 = 0;
    for (size_t i = 0; i < sets.size(); i++) {
        const auto& set = sets[i];
        std::vector<Fr> diffs;
        for (auto& p : super_set) {
            bool in = false;
            for (auto& q : set.points) in = in || q == p;
            if (!in) diffs.push_back(p);
        }
        const Fr z_i = arithmetic::evaluate_vanishing_polynomial(diffs, u);
        if (i == 0) z0 = z_i;
        const auto py = arithmetic::powers(y, set.commitments.size());
        for (size_t j = 0; j < set.commitments.size(); j++) {
            const Fr w = pv[i] * z_i * py[j];
            polys.push_back(&set.commitments[j].first->values);
            scalars.push_back(w);
            Fr r = Fr::zero();  // R_ij(u), Horner on the host (|points| coefficients)
            for (size_t t = interp[c0 + j].size(); t-- > 0;) r = r * u + interp[c0 + j][t];
            constant = constant + w * r;
        }
        c0 += set.commitments.size();
    }
    polys.push_back(&out.h_x.values);
    scalars.push_back(Fr::zero() - arithmetic::evaluate_vanishing_polynomial(super_set, u));
    out.final_poly.values = arithmetic::poly_combine(polys, scalars, {constant}, {u}, z0.invert(), n - 1);
    return out;
}

}  // namespace multiopen
}  // namespace kzg
}  // namespace poly
}  // namespace halo2_proofs

#include "ipa.hpp"  // transcript::Blake2b{Write,Read} and poly::ipa, the inner-product-argument commitment scheme
#include "kzg.hpp"  // poly::kzg::{MSMKZG, DualMSM, GuardKZG, SingleStrategy, AccumulatorStrategy}: the pairing that closes a KZG check
