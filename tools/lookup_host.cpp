// Single-thread host timing of the reference's permute_expression_pair (plonk/lookup/prover.rs:391-475), the step
// h2hip_lookup_permute_bn254 replaces: sort() of the compressed input and a BTreeMap count of the table, both ordering Fr through Ord,
// which compares to_repr() -- every comparison takes both operands out of Montgomery form (here a plain 4 x 64-bit CIOS multiply by one,
// what halo2curves does without its assembly) and compares the canonical limbs from the top.  Then the first rows, the leftovers and the
// fill of the repeated rows.  The lookup_bench.py shape: a tuple lookup with full-width keys (input rows copied from random table rows)
// and a 16-bit range lookup, blinding_factors 5.  The output is checked by the identities of tests/test_lookup_permute.py.  Prints one
// JSON line per size, median of 5 runs.
//   g++ -O3 -std=c++17 -o tools/lookup_host tools/lookup_host.cpp && tools/lookup_host [k ...]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

typedef unsigned __int128 u128;
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t INV = 0xc2e1f593efffffffull;  // -p^-1 mod 2^64
static const uint64_t R2[4] = {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull};

struct F {
    uint64_t l[4];
    bool operator==(const F& o) const { return l[0] == o.l[0] && l[1] == o.l[1] && l[2] == o.l[2] && l[3] == o.l[3]; }
    bool operator!=(const F& o) const { return !(*this == o); }
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

static inline F to_repr(const F& a) { return mont_mul(a, F{{1, 0, 0, 0}}); }
static inline F from_canonical(const F& a) { return mont_mul(a, F{{R2[0], R2[1], R2[2], R2[3]}}); }

// Fr: Ord -- to_repr() of both operands, compared from the most significant end
struct OrdLess {
    bool operator()(const F& a, const F& b) const {
        const F x = to_repr(a), y = to_repr(b);
        for (int j = 3; j >= 0; j--)
            if (x.l[j] != y.l[j]) return x.l[j] < y.l[j];
        return false;
    }
};

// permute_expression_pair over rows [0, u); returns false on ConstraintSystemFailure
static bool permute(const std::vector<F>& input, const std::vector<F>& table, size_t u, std::vector<F>& pa, std::vector<F>& pt) {
    pa.assign(input.begin(), input.begin() + u);
    std::sort(pa.begin(), pa.end(), OrdLess());
    std::map<F, uint32_t, OrdLess> leftover;
    for (size_t i = 0; i < u; i++) leftover[table[i]]++;
    pt.assign(u, F{{0, 0, 0, 0}});
    std::vector<size_t> repeated;
    for (size_t row = 0; row < u; row++) {
        if (row == 0 || pa[row] != pa[row - 1]) {
            pt[row] = pa[row];
            auto it = leftover.find(pa[row]);
            if (it == leftover.end()) return false;
            it->second--;
        } else {
            repeated.push_back(row);
        }
    }
    for (const auto& kv : leftover)
        for (uint32_t c = 0; c < kv.second; c++) {
            pt[repeated.back()] = kv.first;
            repeated.pop_back();
        }
    return repeated.empty();
}

static bool identities(const std::vector<F>& pa, const std::vector<F>& pt) {
    OrdLess lt;
    for (size_t i = 0; i < pa.size(); i++) {
        if (i && lt(pa[i], pa[i - 1])) return false;
        if (pa[i] != pt[i] && !(i && pa[i] == pa[i - 1])) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    std::vector<int> ks;
    for (int i = 1; i < argc; i++) ks.push_back(std::atoi(argv[i]));
    if (ks.empty()) ks = {17, 20, 22};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const size_t b = 5;
    for (int k : ks) {
        const size_t n = (size_t)1 << k, u = n - b - 1;
        // tuple lookup: full-width table values, the input copied from random table rows < u; range lookup: i mod 2^16
        std::vector<F> t0(n), a0(n), t1(n), a1(n);
        for (auto& e : t0) e = from_canonical(F{{rnd(), rnd(), rnd(), rnd() & 0x0fffffffffffffffull}});
        for (auto& e : a0) e = t0[rnd() % u];
        for (size_t i = 0; i < n; i++) t1[i] = from_canonical(F{{i & 0xffff, 0, 0, 0}});
        for (auto& e : a1) e = t1[rnd() % std::min<size_t>(u, 1 << 16)];
        std::vector<double> ms_tuple, ms_range;
        bool ok = true;
        std::vector<F> pa, pt;
        for (int r = 0; r < 5; r++) {
            auto c0 = std::chrono::steady_clock::now();
            ok = permute(a0, t0, u, pa, pt) && ok;
            auto c1 = std::chrono::steady_clock::now();
            if (r == 0) ok = identities(pa, pt) && ok;
            ok = permute(a1, t1, u, pa, pt) && ok;
            auto c2 = std::chrono::steady_clock::now();
            if (r == 0) ok = identities(pa, pt) && ok;
            ms_tuple.push_back(std::chrono::duration<double, std::milli>(c1 - c0).count());
            ms_range.push_back(std::chrono::duration<double, std::milli>(c2 - c1).count());
        }
        std::sort(ms_tuple.begin(), ms_tuple.end());
        std::sort(ms_range.begin(), ms_range.end());
        std::printf("{\"k\": %d, \"permute_tuple_host_ms_median\": %.1f, \"permute_range_host_ms_median\": %.1f, \"both_lookups_host_ms\": %.1f, "
                    "\"checked\": %s}\n",
                    k, ms_tuple[2], ms_range[2], ms_tuple[2] + ms_range[2], ok ? "true" : "false");
        std::fflush(stdout);
        if (!ok) return 1;
    }
    return 0;
}
