// C++ test of the mirror's SerdeFormat paths (halo2-pse_amd/host/halo2hip.hpp: ParamsKZG::read_custom / write_custom in the three
// formats, the polynomial readers and writers, the host-only G2 encoding) and of the C ABI's failure reporting, over the two k = 6
// fixtures.  Needs an MI355X; driven by tests/test_serde.py.  usage: test_serde_mirror <tests/golden dir>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::poly;
using halo2_proofs::poly::kzg::ParamsKZG;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                 \
        }                                                               \
    } while (0)

template <class F>
static bool fails(F f) {  // the reference's io::Error
    try {
        f();
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static std::string written(const ParamsKZG& p, SerdeFormat format) {
    std::ostringstream w;
    p.write_custom(w, format);
    return w.str();
}

static void test_params(const std::string& raw, const std::string& proc) {
    CHECK(raw.size() == 4 + 2 * 64 * 64 + 256 && proc.size() == 4 + 2 * 64 * 32 + 128);
    ParamsKZG a, b, c;
    {
        std::istringstream r(raw), p(proc), u(raw);
        ParamsKZG::read(r, a);
        ParamsKZG::read_custom(p, b, SerdeFormat::Processed);
        ParamsKZG::read_custom(u, c, SerdeFormat::RawBytesUnchecked);
    }
    EvaluationDomain domain(1, 6);
    auto poly = domain.empty_lagrange();
    for (size_t i = 0; i < poly.len(); i++) poly[i] = Fr::from(i * i + 3);
    const G1Affine want = a.commit_lagrange(poly, Blind{Fr::one()}).to_affine();
    for (const ParamsKZG* p : {&a, &b, &c}) {
        CHECK(p->k == 6 && p->g == a.g && p->g_lagrange == a.g_lagrange && p->g2 == a.g2 && p->s_g2 == a.s_g2);
        CHECK(p->commit_lagrange(poly, Blind{Fr::one()}).to_affine() == want);
        CHECK(written(*p, SerdeFormat::RawBytes) == raw && written(*p, SerdeFormat::RawBytesUnchecked) == raw);
        CHECK(written(*p, SerdeFormat::Processed) == proc);
        std::ostringstream w;
        p->write(w);
        CHECK(w.str() == raw);
    }
    CHECK(std::memcmp(a.g.data(), raw.data() + 4, 64 * 64) == 0);
    // truncated files
    for (size_t cut : {size_t(2), size_t(4 + 100), raw.size() - 1}) {
        CHECK(fails([&] {
            ParamsKZG t;
            std::istringstream r(raw.substr(0, cut));
            ParamsKZG::read(r, t);
        }));
        CHECK(fails([&] {
            ParamsKZG t;
            std::istringstream r(proc.substr(0, cut < proc.size() ? cut : proc.size() - 1));
            ParamsKZG::read_custom(r, t, SerdeFormat::Processed);
        }));
    }
    // one corrupted point in each format; the unchecked read takes the raw one
    std::string bad = proc;
    std::memset(&bad[4 + 32 * 70], 0, 32);
    bad[4 + 32 * 70] = 4;  // g_lagrange[6]: x = 4, 4^3 + 3 is not a square
    CHECK(fails([&] {
        ParamsKZG t;
        std::istringstream r(bad);
        ParamsKZG::read_custom(r, t, SerdeFormat::Processed);
    }));
    bad = raw;
    bad[4 + 64 * 9 + 32] ^= 1;  // g[9].y
    CHECK(fails([&] {
        ParamsKZG t;
        std::istringstream r(bad);
        ParamsKZG::read(r, t);
    }));
    {
        ParamsKZG t;
        std::istringstream r(bad);
        ParamsKZG::read_custom(r, t, SerdeFormat::RawBytesUnchecked);
        CHECK(t.g[8] == a.g[8] && !(t.g[9] == a.g[9]));
    }
}

// EIP-197's G2 generator, canonical little-endian limbs: x.c0, x.c1, y.c0, y.c1
static const uint64_t G2_GEN[4][4] = {
    {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
    {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
    {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
    {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};

static void test_g2(const std::string& raw, const std::string& proc) {
    h2::Fe c[4];
    for (int i = 0; i < 4; i++) {
        h2::Fe v;
        std::memcpy(v.l, G2_GEN[i], 32);
        c[i] = h2::fe_from_canonical<h2::FqP>(v);
    }
    std::array<uint8_t, 128> gen, neg, back, zero{};
    std::memcpy(gen.data(), c, 128);
    c[2] = h2::fe_neg<h2::FqP>(c[2]);
    c[3] = h2::fe_neg<h2::FqP>(c[3]);
    std::memcpy(neg.data(), c, 128);
    CHECK(serde::g2_is_valid(gen) && serde::g2_is_valid(neg) && serde::g2_is_valid(zero));
    uint8_t cg[64], cn[64], cz[64];
    serde::g2_to_bytes(gen, cg);
    serde::g2_to_bytes(neg, cn);
    serde::g2_to_bytes(zero, cz);
    CHECK(std::memcmp(cg, G2_GEN[0], 32) == 0 && std::memcmp(cg + 32, G2_GEN[1], 31) == 0);
    CHECK((cg[63] >> 7) == (G2_GEN[2][0] & 1) && (cn[63] >> 7) == ((G2_GEN[2][0] & 1) ^ 1) && std::memcmp(cg, cn, 63) == 0);
    CHECK(serde::all_zero(cz, 64));
    CHECK(serde::g2_from_bytes(cg, back) && back == gen);
    CHECK(serde::g2_from_bytes(cn, back) && back == neg);
    CHECK(serde::g2_from_bytes(cz, back) && back == zero);
    std::array<uint8_t, 128> off = gen;
    off[64] ^= 1;
    CHECK(!serde::g2_is_valid(off));
    uint8_t bad[64] = {};
    std::memcpy(bad + 32, h2::FqP::MOD, 32);  // x.c1 = q
    CHECK(!serde::g2_from_bytes(bad, back));
    // through a params file, both formats
    ParamsKZG p, q;
    {
        std::istringstream r(raw);
        ParamsKZG::read(r, p);
    }
    p.g2 = gen;
    p.s_g2 = neg;
    const std::string w = written(p, SerdeFormat::Processed);
    CHECK(w.size() == proc.size() && w.compare(0, proc.size() - 128, proc, 0, proc.size() - 128) == 0);
    CHECK(std::memcmp(w.data() + w.size() - 128, cg, 64) == 0 && std::memcmp(w.data() + w.size() - 64, cn, 64) == 0);
    {
        std::istringstream r(w);
        ParamsKZG::read_custom(r, q, SerdeFormat::Processed);
    }
    CHECK(q.g2 == gen && q.s_g2 == neg && q.g == p.g);
    {
        std::istringstream r(written(p, SerdeFormat::RawBytes));
        ParamsKZG::read(r, q);
    }
    CHECK(q.g2 == gen && q.s_g2 == neg);
    std::string broken = written(p, SerdeFormat::RawBytes);
    broken[broken.size() - 1 - 128] ^= 1;
    CHECK(fails([&] {
        ParamsKZG t;
        std::istringstream r(broken);
        ParamsKZG::read(r, t);
    }));
}

static void test_polynomials() {
    std::vector<Polynomial<Coeff>> polys(3);
    Fr x = Fr::from(5);
    for (size_t j = 0; j < 3; j++)
        for (size_t i = 0; i < 100 * j + 1; i++) {  // lengths 1, 101, 201
            polys[j].values.push_back(x);
            x = x * x + Fr::from(i);
        }
    polys[1][0] = Fr::zero();
    polys[1][1] = Fr::zero() - Fr::one();
    for (SerdeFormat f : {SerdeFormat::Processed, SerdeFormat::RawBytes, SerdeFormat::RawBytesUnchecked}) {
        std::ostringstream w;
        write_polynomial_slice(polys, w, f);
        CHECK(w.str().size() == 4 + 3 * 4 + 303 * 32);
        std::istringstream r(w.str());
        auto back = read_polynomial_vec<Coeff>(r, f);
        CHECK(back.size() == 3);
        for (size_t j = 0; j < back.size() && j < 3; j++) CHECK(back[j].values == polys[j].values);
        CHECK(fails([&] {
            std::istringstream t(w.str().substr(0, w.str().size() - 1));
            read_polynomial_vec<Coeff>(t, f);
        }));
    }
    // the Processed form of 1 is the integer 1; r itself is rejected in the two checked formats
    Polynomial<Coeff> one{{Fr::one()}};
    std::ostringstream w;
    write_polynomial(one, w, SerdeFormat::Processed);
    std::string s = w.str();
    CHECK(s.size() == 36 && s[3] == 1 && s[4] == 1 && serde::all_zero(reinterpret_cast<const uint8_t*>(s.data()) + 5, 31));
    std::memcpy(&s[4], h2::FrP::MOD, 32);
    for (SerdeFormat f : {SerdeFormat::Processed, SerdeFormat::RawBytes})
        CHECK(fails([&] {
            std::istringstream t(s);
            read_polynomial<Coeff>(t, f);
        }));
    std::istringstream t(s);
    CHECK(read_polynomial<Coeff>(t, SerdeFormat::RawBytesUnchecked).len() == 1);
}

static void test_abi(const std::string& proc) {
    uint64_t invalid[2] = {9, 9}, pts[64 * 8];
    uint8_t bytes[64 * 32];
    CHECK(h2hip_g1_decompress_bn254(nullptr, 0, nullptr, invalid) == H2HIP_OK && invalid[0] == 0 && invalid[1] == 0);
    CHECK(h2hip_g1_decompress_bn254(nullptr, 4, pts, invalid) == H2HIP_EINVAL);
    CHECK(h2hip_g1_decompress_bn254(bytes, 4, nullptr, invalid) == H2HIP_EINVAL);
    CHECK(h2hip_g1_decompress_bn254(bytes, 4, pts, nullptr) == H2HIP_EINVAL);
    CHECK(h2hip_g1_validate_bn254(nullptr, 1, invalid) == H2HIP_EINVAL && h2hip_g1_validate_bn254(pts, 1, nullptr) == H2HIP_EINVAL);
    CHECK(h2hip_g1_compress_bn254(pts, 1, nullptr) == H2HIP_EINVAL && h2hip_g1_compress_bn254(nullptr, 0, nullptr) == H2HIP_OK);
    CHECK(h2hip_fr_from_repr_bn254(bytes, 1, nullptr, invalid) == H2HIP_EINVAL && h2hip_fr_to_repr_bn254(nullptr, 1, bytes) == H2HIP_EINVAL);
    CHECK(h2hip_fr_to_repr_bn254(nullptr, 0, nullptr) == H2HIP_OK && h2hip_g1_validate_bn254(nullptr, 0, invalid) == H2HIP_OK);
    // g of the fixture with three encodings spoilt: the count, the lowest index, zeros there and the points elsewhere
    std::memcpy(bytes, proc.data() + 4, sizeof bytes);
    CHECK(h2hip_g1_decompress_bn254(bytes, 64, pts, invalid) == H2HIP_OK && invalid[0] == 0 && invalid[1] == 0);
    uint64_t good[64 * 8];
    std::memcpy(good, pts, sizeof good);
    for (size_t at : {size_t(63), size_t(17), size_t(40)}) {
        std::memset(bytes + 32 * at, 0, 32);
        bytes[32 * at] = 4;
    }
    CHECK(h2hip_g1_decompress_bn254(bytes, 64, pts, invalid) == H2HIP_EENCODING && invalid[0] == 3 && invalid[1] == 17);
    for (size_t i = 0; i < 64; i++) {
        const bool planted = i == 17 || i == 40 || i == 63;
        CHECK(planted ? serde::all_zero(reinterpret_cast<const uint8_t*>(pts + 8 * i), 64) : std::memcmp(pts + 8 * i, good + 8 * i, 64) == 0);
        G1Affine host;
        CHECK(serde::g1_from_bytes_host(bytes + 32 * i, host) == !planted && std::memcmp(&host, pts + 8 * i, 64) == 0);
    }
    CHECK(h2hip_g1_validate_bn254(good, 64, invalid) == H2HIP_OK);
    good[8 * 5 + 4] ^= 1;
    CHECK(h2hip_g1_validate_bn254(good, 64, invalid) == H2HIP_EENCODING && invalid[0] == 1 && invalid[1] == 5);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s <tests/golden dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], raw = slurp(dir + "/kzg_6_params.rawbytes"), proc = slurp(dir + "/kzg_6_params.processed");
    try {
        test_params(raw, proc);
        test_g2(raw, proc);
        test_polynomials();
        test_abi(proc);
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        failures++;
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("serde mirror tests ok\n");
    return 0;
}
