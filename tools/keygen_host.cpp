// Host timing, on 16 threads, of the two loops of key generation that csrc/keygen.hip replaces, as the reference writes them:
//   Assembly::build_pk's tables (plonk/permutation/keygen.rs:173-212): omega_powers (2^k), deltaomega (m copies of it, each times
//   delta^c), then permutations[i][j] = deltaomega[c][r] for (c, r) = mapping[i][j] -- `parallelize` splits each of the three over the
//   threads;
//   batch_invert_assigned (poly.rs:180-209): one BatchInvert over the Rational denominators of all fixed columns (serial in the
//   reference: ff's BatchInvert is one running product, one inversion and a back sweep), then numerator * inverse per cell.
// The arithmetic is a plain 4 x 64-bit CIOS Montgomery multiply, what halo2curves does without its assembly.  The transforms that
// follow in the reference are timed elsewhere (README, ntt.cpu_baseline).  The keygen_bench.py shape: 9 permutation columns, the mapping
// the identity with a tenth of the cells joined into cycles; 4 fixed columns with 1 % Rational cells.  Prints one JSON line per size,
// median of 5 runs.
//   g++ -O3 -std=c++17 -pthread -o tools/keygen_host tools/keygen_host.cpp && tools/keygen_host [k ...]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

typedef unsigned __int128 u128;
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t INV = 0xc2e1f593efffffffull;  // -p^-1 mod 2^64
static const uint64_t R2[4] = {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull};
static const int THREADS = 16;

struct F {
    uint64_t l[4];
};

static inline F mont_mul(const F& a, const F& b) {
    uint64_t t[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        const uint64_t hi = t[4] + (uint64_t)c;  // p < 2^254: no carry out of the fifth word
        const uint64_t m = t[0] * INV;
        c = ((u128)m * P[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * P[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += hi;
        t[3] = (uint64_t)c;
        t[4] = (uint64_t)(c >> 64);
    }
    uint64_t s[4], br = 0;
    for (int j = 0; j < 4; j++) {
        const u128 d = (u128)t[j] - P[j] - br;
        s[j] = (uint64_t)d;
        br = (uint64_t)(d >> 64) & 1;
    }
    const bool keep = br && !t[4];
    F r;
    for (int j = 0; j < 4; j++) r.l[j] = keep ? t[j] : s[j];
    return r;
}

static inline F from_u64(uint64_t v) { return mont_mul(F{{v, 0, 0, 0}}, F{{R2[0], R2[1], R2[2], R2[3]}}); }
static const F ONE = from_u64(1);
static inline bool is_zero(const F& a) { return !(a.l[0] | a.l[1] | a.l[2] | a.l[3]); }

static F pow_limbs(const F& a, const uint64_t e[4]) {
    F r = ONE;
    for (int i = 255; i >= 0; i--) {
        r = mont_mul(r, r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = mont_mul(r, a);
    }
    return r;
}
static F pow_u64(const F& a, uint64_t e) {
    const uint64_t limbs[4] = {e, 0, 0, 0};
    return pow_limbs(a, limbs);
}
static F invert(const F& a) {
    const uint64_t e[4] = {P[0] - 2, P[1], P[2], P[3]};
    return pow_limbs(a, e);
}

// arithmetic.rs parallelize: contiguous chunks, one per thread
static void parallelize(size_t len, const std::function<void(size_t, size_t)>& f) {
    std::vector<std::thread> ts;
    const size_t chunk = (len + THREADS - 1) / THREADS;
    for (size_t s = 0; s < len; s += chunk) ts.emplace_back(f, s, std::min(len, s + chunk));
    for (auto& t : ts) t.join();
}

int main(int argc, char** argv) {
    std::vector<int> ks;
    for (int i = 1; i < argc; i++) ks.push_back(std::atoi(argv[i]));
    if (ks.empty()) ks = {17, 20, 22};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const size_t m = 9, n_fixed = 4;
    {  // the arithmetic checks itself: R mod p, 1 * 1 = 1, a * a^-1 = 1
        const F a = from_u64(0x1234567), p1 = mont_mul(a, invert(a)), o = mont_mul(ONE, ONE);
        if (ONE.l[0] != 0xac96341c4ffffffbull || ONE.l[3] != 0x0e0a77c19a07df2full || o.l[0] != ONE.l[0] || o.l[3] != ONE.l[3] || p1.l[0] != ONE.l[0] ||
            p1.l[1] != ONE.l[1] || p1.l[2] != ONE.l[2] || p1.l[3] != ONE.l[3]) {
            std::fprintf(stderr, "Montgomery self-check failed\n");
            return 1;
        }
    }
    const F root = from_u64(5);  // any element will do for the timing: 5^((p - 1) / 2^k) has order dividing 2^k
    for (int k : ks) {
        const size_t n = (size_t)1 << k;
        uint64_t e[4] = {P[0] - 1, P[1], P[2], P[3]};
        for (int s = 0; s < k; s++) {  // (p - 1) >> k
            for (int j = 0; j < 3; j++) e[j] = (e[j] >> 1) | (e[j + 1] << 63);
            e[3] >>= 1;
        }
        const F omega = pow_limbs(root, e), delta = pow_u64(from_u64(7), (uint64_t)1 << 28);
        // the identity with a tenth of the cells joined into cycles of 2..5 cells
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> mapping(m, std::vector<std::pair<uint32_t, uint32_t>>(n));
        for (size_t c = 0; c < m; c++)
            for (size_t r = 0; r < n; r++) mapping[c][r] = {(uint32_t)c, (uint32_t)r};
        for (size_t done = 0; done < m * n / 10;) {
            const size_t len = 2 + rnd() % 4;
            std::pair<uint32_t, uint32_t> cells[5];
            for (size_t i = 0; i < len; i++) cells[i] = {(uint32_t)(rnd() % m), (uint32_t)(rnd() % n)};
            for (size_t i = 0; i + 1 < len; i++) std::swap(mapping[cells[i].first][cells[i].second], mapping[cells[i + 1].first][cells[i + 1].second]);
            done += len;
        }
        std::vector<std::vector<F>> fixed(n_fixed, std::vector<F>(n));
        std::vector<std::vector<uint32_t>> rat_rows(n_fixed);
        std::vector<std::vector<F>> rat_denoms(n_fixed);
        for (size_t j = 0; j < n_fixed; j++)
            for (size_t r = 0; r < n; r++) {
                fixed[j][r] = from_u64(rnd());
                if (rnd() % 100 == 0) {
                    rat_rows[j].push_back((uint32_t)r);
                    rat_denoms[j].push_back(from_u64(rnd() | 1));
                }
            }
        std::vector<double> ms_sigma, ms_inv;
        F check = ONE;
        for (int rep = 0; rep < 5; rep++) {
            auto c0 = std::chrono::steady_clock::now();
            std::vector<F> omega_powers(n);                                  // :174-184
            parallelize(n, [&](size_t s, size_t t) {
                F cur = pow_u64(omega, s);
                for (size_t i = s; i < t; i++) {
                    omega_powers[i] = cur;
                    cur = mont_mul(cur, omega);
                }
            });
            std::vector<std::vector<F>> deltaomega(m, omega_powers);          // :187-198
            parallelize(m, [&](size_t s, size_t t) {
                F cur = pow_u64(delta, s);
                for (size_t c = s; c < t; c++) {
                    for (auto& v : deltaomega[c]) v = mont_mul(v, cur);
                    cur = mont_mul(cur, delta);
                }
            });
            std::vector<std::vector<F>> permutations(m, std::vector<F>(n));   // :201-212
            parallelize(m, [&](size_t s, size_t t) {
                for (size_t i = s; i < t; i++)
                    for (size_t j = 0; j < n; j++) permutations[i][j] = deltaomega[mapping[i][j].first][mapping[i][j].second];
            });
            auto c1 = std::chrono::steady_clock::now();
            // batch_invert_assigned: the denominators of all columns in one BatchInvert (poly.rs:183-200), then poly.invert (:202-208)
            std::vector<F*> dens;
            std::vector<std::vector<F>> inv = rat_denoms;
            for (auto& col : inv)
                for (auto& d : col) dens.push_back(&d);
            std::vector<F> tmp(dens.size());
            F acc = ONE;
            for (size_t i = 0; i < dens.size(); i++) {
                tmp[i] = acc;
                if (!is_zero(*dens[i])) acc = mont_mul(acc, *dens[i]);
            }
            acc = invert(acc);
            for (size_t i = dens.size(); i-- > 0;) {
                if (is_zero(*dens[i])) continue;
                const F nw = mont_mul(acc, tmp[i]);
                acc = mont_mul(acc, *dens[i]);
                *dens[i] = nw;
            }
            std::vector<std::vector<F>> out = fixed;
            for (size_t j = 0; j < n_fixed; j++)
                for (size_t t = 0; t < rat_rows[j].size(); t++) out[j][rat_rows[j][t]] = mont_mul(out[j][rat_rows[j][t]], inv[j][t]);
            auto c2 = std::chrono::steady_clock::now();
            ms_sigma.push_back(std::chrono::duration<double, std::milli>(c1 - c0).count());
            ms_inv.push_back(std::chrono::duration<double, std::milli>(c2 - c1).count());
            check = mont_mul(permutations[m - 1][n - 1], out[0][rat_rows[0].empty() ? 0 : rat_rows[0][0]]);
        }
        std::sort(ms_sigma.begin(), ms_sigma.end());
        std::sort(ms_inv.begin(), ms_inv.end());
        std::printf("{\"k\": %d, \"threads\": %d, \"permutation_columns\": %zu, \"fixed_columns\": %zu, \"sigma_tables_host_ms_median\": %.1f, "
                    "\"batch_invert_assigned_host_ms_median\": %.1f, \"check\": \"%016llx\"}\n",
                    k, THREADS, m, n_fixed, ms_sigma[2], ms_inv[2], (unsigned long long)check.l[0]);
        std::fflush(stdout);
    }
    return 0;
}
