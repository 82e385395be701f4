// Single-thread host timing of the reference's kate_division loop (arithmetic.rs:348-366): one dependent Montgomery multiply and one
// subtraction per coefficient, over 4 x 64-bit limbs with a plain CIOS multiply (what halo2curves does without its assembly).  The result
// is cross-checked against field.h's multiply.  Prints one JSON line per size, median of 7 runs.
//   g++ -O3 -march=native -std=c++17 -o tools/kate_host tools/kate_host.cpp && tools/kate_host
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2-pse_amd/csrc/field.h"

typedef unsigned __int128 u128;
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t INV = 0xc2e1f593efffffffull;  // -p^-1 mod 2^64

struct F {
    uint64_t l[4];
};

static inline F mont_mul(const F& a, const F& b) {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * INV;
        c = (u128)m * P[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * P[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    F r;
    uint64_t s[4], br = 0;
    for (int j = 0; j < 4; j++) {
        u128 d = (u128)t[j] - P[j] - br;
        s[j] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
    const bool keep = br && !t[4];
    for (int j = 0; j < 4; j++) r.l[j] = keep ? t[j] : s[j];
    return r;
}

static inline F sub(const F& a, const F& b) {
    F r;
    uint64_t br = 0;
    for (int j = 0; j < 4; j++) {
        u128 d = (u128)a.l[j] - b.l[j] - br;
        r.l[j] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
    if (br) {
        uint64_t c = 0;
        for (int j = 0; j < 4; j++) {
            u128 s = (u128)r.l[j] + P[j] + c;
            r.l[j] = (uint64_t)s;
            c = (uint64_t)(s >> 64);
        }
    }
    return r;
}

static void kate(const std::vector<F>& a, F b, std::vector<F>& q) {  // b = -b; lead = r - tmp; tmp = lead * b
    b = sub(F{{0, 0, 0, 0}}, b);
    F tmp{{0, 0, 0, 0}};
    for (size_t i = a.size() - 1; i > 0; i--) {
        F lead = sub(a[i], tmp);
        q[i - 1] = lead;
        tmp = mont_mul(lead, b);
    }
}

int main() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int k : {17, 20}) {
        const size_t n = (size_t)1 << k;
        std::vector<F> a(n), q(n - 1);
        for (auto& e : a) e = F{{rnd(), rnd(), rnd(), rnd() & 0x0fffffffffffffffull}};
        const F b{{rnd(), rnd(), rnd(), rnd() & 0x0fffffffffffffffull}};
        std::vector<double> ms;
        for (int r = 0; r < 7; r++) {
            auto t0 = std::chrono::steady_clock::now();
            kate(a, b, q);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        // cross-check one step against field.h: q[n-3] = a[n-2] + b q[n-2]
        h2::Fe fb, fq, fa;
        memcpy(fb.l, b.l, 32), memcpy(fq.l, q[n - 2].l, 32), memcpy(fa.l, a[n - 2].l, 32);
        h2::Fe want = h2::fe_add<h2::FrP>(fa, h2::fe_mul<h2::FrP>(fb, fq));
        const bool ok = memcmp(want.l, q[n - 3].l, 32) == 0;
        std::printf("{\"k\": %d, \"kate_division_host_ms_median\": %.3f, \"ns_per_coefficient\": %.1f, \"checked\": %s}\n", k, ms[3],
                    ms[3] * 1e6 / (double)n, ok ? "true" : "false");
        if (!ok) return 1;
    }
    return 0;
}
