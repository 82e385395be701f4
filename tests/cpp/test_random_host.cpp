// Host-side test of what csrc/random.hip's kernels do to one element (csrc/random_elem.h): the ChaCha20 block against rand_chacha's
// zero-seed vector and RFC 7539 2.3.2, and Fr::from_bytes_wide against a schoolbook 512-bit remainder written here (shift and subtract,
// one bit at a time) followed by field.h's fe_from_canonical.  Built with -DH2_FU_CHECK, so the product asserts its limb bounds.
// No GPU needed: the same H2_HD source compiles for the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../halo2-pse_amd/csrc/random_elem.h"

using namespace h2;

static uint64_t rs = 0x7a2d0;
static uint64_t rnd() {
    rs += 0x9E3779B97F4A7C15ULL;
    uint64_t x = rs;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
static int failures = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (failures < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// v mod r for the 16-word little-endian integer v: rem = 2 rem + bit, minus r when that reaches r; rem < r < 2^254 throughout
static Fe wide_mod_r(const uint32_t w[16]) {
    uint32_t rem[8] = {0};
    for (int bit = 511; bit >= 0; bit--) {
        uint32_t carry = (w[bit >> 5] >> (bit & 31)) & 1u;
        for (int j = 0; j < 8; j++) {
            const uint32_t top = rem[j] >> 31;
            rem[j] = rem[j] << 1 | carry;
            carry = top;
        }
        Fe o;
        fe_cond_sub<FrP>(o, rem);
        memcpy(rem, o.l, 32);
    }
    Fe o;
    memcpy(o.l, rem, 32);
    return o;
}

static void check_wide(const uint32_t w[16]) {
    const Fe want = fe_from_canonical<FrP>(wide_mod_r(w));
    const Fe got = fr_from_wide_elem(w);
    CHECK(fe_is_canonical<FrP>(got));
    CHECK(fe_eq(got, want));
}

struct Wide {
    uint32_t w[16];
};
static Wide wide(const uint32_t lo[8], const uint32_t hi[8]) {
    Wide v;
    memset(v.w, 0, 64);
    if (lo) memcpy(v.w, lo, 32);
    if (hi) memcpy(v.w + 8, hi, 32);
    return v;
}

static bool block_is(const uint8_t seed[32], uint64_t counter, uint64_t stream, const char* hex_first, const char* hex_last) {
    uint32_t out[16];
    chacha20_block(chacha_key(seed, stream), counter, out);
    char hex[129];
    for (int i = 0; i < 64; i++) snprintf(hex + 2 * i, 3, "%02x", (out[i / 4] >> (8 * (i % 4))) & 0xffu);
    return !strncmp(hex, hex_first, strlen(hex_first)) && !strcmp(hex + 128 - strlen(hex_last), hex_last);
}

int main() {
    // ---- the block function ----
    uint8_t seed[32] = {0};
    CHECK(block_is(seed, 0, 0, "76b8e0ada0f13d90405d6ae55386bd28", "b2ee6586"));  // rand_chacha's zero-seed vector: first word 0xade0b876
    uint32_t out[16];
    chacha20_block(chacha_key(seed, 0), 0, out);
    CHECK(out[0] == 0xade0b876u);
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)i;
    // RFC 7539 2.3.2: counter word 1, nonce 00000009 0000004a 00000000 -> counter = 1 | 0x09000000 << 32, stream = 0x4a000000
    CHECK(block_is(seed, 1ull | 0x09000000ull << 32, 0x4a000000ull,
                   "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e", ""));
    // the counter's two words: blocks 2^32 - 1 and 2^32 differ, and block 2^32 is not block 0
    uint32_t a[16], b[16], c[16];
    chacha20_block(chacha_key(seed, 0), 0xffffffffull, a);
    chacha20_block(chacha_key(seed, 0), 0x100000000ull, b);
    chacha20_block(chacha_key(seed, 0), 0, c);
    CHECK(memcmp(a, b, 64) && memcmp(b, c, 64));

    // ---- one pinned draw: zero seed, block 0 -> canonical 0x1c59a59b...dd6dfcba ----
    memset(seed, 0, 32);
    static const uint32_t PINNED[8] = {0xdd6dfcbau, 0xc89586bcu, 0x7a67269cu, 0x09f71b33u, 0x6ade1d8cu, 0x74094352u, 0x6cff4308u, 0x1c59a59bu};
    Fe pinned;
    memcpy(pinned.l, PINNED, 32);
    CHECK(fe_eq(fe_to_canonical<FrP>(fr_random_elem(chacha_key(seed, 0), 0)), pinned));

    // ---- the wide reduction on crafted inputs ----
    uint32_t zero[8] = {0}, one[8] = {1}, ones[8], r[8], rm1[8], rp1[8];
    memset(ones, 0xff, 32);
    memcpy(r, FrP::MOD, 32);
    memcpy(rm1, r, 32), rm1[0] -= 1;  // r is odd and its low word is not all ones
    memcpy(rp1, r, 32), rp1[0] += 1;
    const Wide crafted[] = {
        wide(zero, nullptr), wide(one, nullptr), wide(rm1, nullptr), wide(r, nullptr), wide(rp1, nullptr), wide(ones, nullptr),  // .. 2^256 - 1
        wide(nullptr, one),   // 2^256
        wide(nullptr, r),     // r * 2^256
        wide(ones, ones),     // 2^512 - 1
        wide(ones, zero), wide(zero, ones), wide(rm1, rm1), wide(r, r),
    };
    for (const Wide& v : crafted) check_wide(v.w);
    CHECK(fe_is_zero(fr_from_wide_elem(wide(r, r).w)) && fe_is_zero(fr_from_wide_elem(wide(zero, nullptr).w)));
    CHECK(fe_eq(fr_from_wide_elem(wide(one, nullptr).w), fe_one<FrP>()));
    Wide top = wide(nullptr, nullptr);
    for (int bit = 0; bit < 512; bit++) {  // every power of two
        memset(top.w, 0, 64);
        top.w[bit >> 5] = 1u << (bit & 31);
        check_wide(top.w);
    }
    for (int it = 0; it < 4000; it++) {
        Wide v;
        for (int j = 0; j < 16; j++) v.w[j] = (uint32_t)rnd();
        if (it % 4 == 1) memset(v.w + 8, 0xff, 32);
        if (it % 4 == 2) memset(v.w, 0xff, 32);
        check_wide(v.w);
    }
    // ... and on what the generator feeds it
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)rnd();
    const ChaChaKey key = chacha_key(seed, 0x1234567890abcdefull);
    for (uint64_t i = 0; i < 1000; i++) {
        uint32_t w[16];
        chacha20_block(key, 0xfffffff0ull + i, w);
        check_wide(w);
        CHECK(fe_eq(fr_random_elem(key, 0xfffffff0ull + i), fr_from_wide_elem(w)));
    }

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("random host tests ok\n");
    return 0;
}
