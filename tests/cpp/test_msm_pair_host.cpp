// Host-side test of the pair MSM's index and plan arithmetic (csrc/msm_pair.h): the rotated scalar index, the set assignment and the
// boundary of the single two-set run, against definitions written out here.  No GPU and no library: the same source the digit kernels
// and msm_pair_device compile.  Run plain and under ASan + UBSan (tests/test_ipa_round_abi.py): the arrays below are sized exactly, so an
// index one past 2 half - 1 is an error the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../halo2-pse_amd/csrc/msm_pair.h"

using namespace h2;

static int failures = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// L = sum_{i < half} p[half + i] g[i], R = sum_{i < half} p[i] g[half + i] over the integers mod a small prime, "points" being numbers
static const uint64_t M = 1000003;

static void sums_by_definition(const std::vector<uint64_t>& p, const std::vector<uint64_t>& g, uint32_t half, uint64_t out[2]) {
    out[0] = out[1] = 0;
    for (uint32_t i = 0; i < half; i++) {
        out[0] = (out[0] + p[half + i] * g[i]) % M;
        out[1] = (out[1] + p[i] * g[half + i]) % M;
    }
}

// the same the way the run forms them: MSM y of the two, tiles of `tile` lanes, lane t -> point, scalar index, set
static void sums_by_pair_run(const std::vector<uint64_t>& p, const std::vector<uint64_t>& g, uint32_t half, uint32_t tile, uint64_t out[2]) {
    out[0] = out[1] = 0;
    std::vector<uint32_t> seen(2 * (size_t)half, 0);
    const uint32_t tiles = (half + tile - 1) / tile;
    for (uint32_t y = 0; y < 2; y++)
        for (uint32_t bx = 0; bx < tiles; bx++)
            for (uint32_t t = 0; t < tile; t++) {
                const uint32_t i = bx * tile + t;
                if (i >= half) continue;  // the kernels' guard
                const uint32_t point = msm_pair_point(y, i, half);
                const uint32_t si = msm_pair_scalar_index(point, half);
                CHECK(point < 2 * half && si < 2 * half);
                CHECK(msm_pair_set(point, half) == y);
                CHECK(si == (point + half) % (2 * half));
                seen.at(point)++;
                out[y] = (out[y] + p.at(si) * g.at(point)) % M;
            }
    for (uint32_t v : seen) CHECK(v == 1);  // every point exactly once
}

static uint64_t rs = 0x5eed;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// a plan that depends on floor(log2 half) only, shaped like the library's: narrow windows for small sizes
static MsmPairWindows windows_of(uint32_t lg) {
    const uint32_t c = lg <= 8 ? 7 : lg <= 12 ? 10 : lg <= 16 ? 12 : lg == 17 ? 13 : lg == 18 ? 14 : 17;
    const uint32_t W = (255 + c - 1) / c, cw = (255 + W - 1) / W;
    return MsmPairWindows{W, cw - 1};
}
static uint32_t floor_log2(size_t n) {
    uint32_t lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) lg++;
    return lg;
}
static bool fits(size_t half, size_t entries, size_t max_n, uint64_t max_buckets, uint32_t max_sets) {
    const MsmPairWindows w = windows_of(floor_log2(half));
    return msm_pair_fits(half, w.W, w.cb, entries, max_n, max_buckets, max_sets);
}

int main() {
    // ---- indices
    for (uint32_t half : {1u, 2u, 3u, 5u, 64u, 257u, 1024u, 1000u, 4097u})
        for (uint32_t tile : {64u, 448u, 1024u}) {
            std::vector<uint64_t> p(2 * (size_t)half), g(2 * (size_t)half);
            for (auto& v : p) v = rnd() % M;
            for (auto& v : g) v = rnd() % M;
            uint64_t want[2], got[2];
            sums_by_definition(p, g, half, want);
            sums_by_pair_run(p, g, half, tile, got);
            CHECK(want[0] == got[0] && want[1] == got[1]);
        }
    // the largest size of the call: the indices stay below 2^27 <= 2^31 (the entry's 31 bits)
    {
        const uint32_t half = 1u << 26;
        CHECK(msm_pair_point(1, half - 1, half) == 2 * half - 1);
        CHECK(msm_pair_scalar_index(2 * half - 1, half) == half - 1);
        CHECK(msm_pair_scalar_index(0, half) == half);
        CHECK(msm_pair_scalar_index(half - 1, half) == 2 * half - 1);
        CHECK(msm_pair_scalar_index(half, half) == 0);
        CHECK(msm_pair_set(half - 1, half) == 0 && msm_pair_set(half, half) == 1);
    }
    // ---- the test itself: every limit
    const uint64_t MB = (uint64_t)1024 << 12;  // the sort's bucket limit
    CHECK(msm_pair_fits(1, 37, 6, (size_t)1 << 26, (size_t)1 << 19, MB, 1024));
    CHECK(!msm_pair_fits(0, 37, 6, (size_t)1 << 26, (size_t)1 << 19, MB, 1024));
    CHECK(msm_pair_fits((size_t)1 << 19, 15, 16, (size_t)1 << 26, (size_t)1 << 19, MB, 1024));
    CHECK(!msm_pair_fits(((size_t)1 << 19) + 1, 15, 16, (size_t)1 << 26, (size_t)1 << 19, MB, 1024));  // pairs per sum
    CHECK(msm_pair_fits(100, 10, 5, 2000, 1000, MB, 1024) && !msm_pair_fits(101, 10, 5, 2000, 1000, MB, 1024));  // entries: 2 half W
    CHECK(!msm_pair_fits(100, 10, 5, 1999, 1000, MB, 1024));
    CHECK(msm_pair_fits(8, 512, 3, (size_t)1 << 26, 1000, MB, 1024) && !msm_pair_fits(8, 513, 3, (size_t)1 << 26, 1000, MB, 1024));  // sets: 2 W
    CHECK(msm_pair_fits(8, 11, 17, (size_t)1 << 26, 1000, MB, 1024) && !msm_pair_fits(8, 11, 23, (size_t)1 << 26, 1000, MB, 1024));  // buckets
    CHECK(!msm_pair_fits(8, 11, 63, (size_t)1 << 26, 1000, ~(uint64_t)0, 1024) && !msm_pair_fits(8, 0, 3, (size_t)1 << 26, 1000, MB, 1024));
    CHECK(!msm_pair_fits(8, 1, 3, 0, 1000, MB, 1024));
    CHECK(msm_pair_fits(((size_t)-1) / 6, 3, 3, (size_t)-1, (size_t)-1, MB, 1024) && !msm_pair_fits((size_t)-1, 3, 3, (size_t)-1, (size_t)-1, MB, 1024));  // no overflow on the way
    // ---- the boundary against a scan, over limits that cut inside a class, at a class edge, below every class and above all
    const size_t limit = (size_t)1 << 26;
    for (size_t max_n : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000, (size_t)1 << 11, (size_t)5000, (size_t)1 << 13})
        for (size_t entries : {(size_t)0, (size_t)1, (size_t)73, (size_t)74, (size_t)75, (size_t)1000, (size_t)20000, (size_t)100000, (size_t)123456,
                               (size_t)1 << 20, (size_t)1 << 26}) {
            size_t want = 0;
            for (size_t h = max_n < limit ? max_n : limit; h >= 1; h--)
                if (fits(h, entries, max_n, MB, 1024)) {
                    want = h;
                    break;
                }
            const size_t got = msm_pair_max_half(windows_of, entries, max_n, MB, 1024, limit);
            CHECK(got == want);
            if (got) CHECK(fits(got, entries, max_n, MB, 1024));
        }
    // the defaults: 2^19 pairs per sum, 2^26 entries -> 2^19; a limit below it wins; limits beyond every size do not overflow
    CHECK(msm_pair_max_half(windows_of, (size_t)1 << 26, (size_t)1 << 19, MB, 1024, limit) == (size_t)1 << 19);
    CHECK(msm_pair_max_half(windows_of, (size_t)1 << 26, (size_t)1 << 19, MB, 1024, 1000) == 1000);
    CHECK(msm_pair_max_half(windows_of, (size_t)-1, (size_t)-1, MB, 1024, limit) == limit);
    CHECK(msm_pair_max_half(windows_of, (size_t)-1, (size_t)-1, MB, 1024, (size_t)-1) == ((size_t)-1) / 2 / 15);  // the entries, at W = 15
    CHECK(msm_pair_max_half(windows_of, (size_t)1 << 26, (size_t)1 << 19, 1, 1024, limit) == 0);  // no buckets at all: nothing fits
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("msm pair host tests ok\n");
    return 0;
}
