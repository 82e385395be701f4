// random_elem.h -- what random.hip's kernels do to ONE element, host and device: the ChaCha20 block of rand_chacha 0.3's ChaCha20Rng
// and halo2curves 0.3.1's Fr::from_bytes_wide (= Fr::from_u512, what Fr::random computes from eight next_u64 draws), as DESIGN.md
// section 2 records them.  Kept apart from the kernels so that tests/cpp/test_random_host.cpp runs the same source on the host with
// H2_FU_CHECK, where the product asserts fieldu.h's limb bounds, and so that the host forms of the C ABI run it below their threshold.
#pragma once
#include "fieldu.h"

namespace h2 {

// the key of a stream: the 32 seed bytes as 8 little-endian words, and the 64-bit stream id (state words 14, 15)
struct ChaChaKey {
    uint32_t k[8];
    uint32_t s[2];
};

H2_HD ChaChaKey chacha_key(const uint8_t seed[32], uint64_t stream_id) {
    ChaChaKey key;
#pragma unroll
    for (int i = 0; i < 8; i++)
        key.k[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
    key.s[0] = (uint32_t)stream_id;
    key.s[1] = (uint32_t)(stream_id >> 32);
    return key;
}

// one funnel shift (v_alignbit_b32) on gfx950; g++, which builds the host tests, has no such builtin
H2_HD uint32_t rotl32(uint32_t x, uint32_t s) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateleft32)
    return __builtin_rotateleft32(x, s);
#else
    return x << s | x >> (32 - s);
#endif
#else
    return x << s | x >> (32 - s);
#endif
}

#define H2_CHACHA_QR(a, b, c, d)         \
    do {                                 \
        a += b, d = rotl32(d ^ a, 16);   \
        c += d, b = rotl32(b ^ c, 12);   \
        a += b, d = rotl32(d ^ a, 8);    \
        c += d, b = rotl32(b ^ c, 7);    \
    } while (0)

// ChaCha20, 20 rounds: state = "expand 32-byte k" | key | 64-bit block counter (words 12, 13) | 64-bit stream id (words 14, 15);
// out = the 16 output words in the order the generator hands them out.  Named scalars, not an array: nothing is indexed at run time.
H2_HD void chacha20_block(const ChaChaKey& key, uint64_t counter, uint32_t out[16]) {
    const uint32_t i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;
    const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32);
    uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3, x4 = key.k[0], x5 = key.k[1], x6 = key.k[2], x7 = key.k[3], x8 = key.k[4], x9 = key.k[5],
             x10 = key.k[6], x11 = key.k[7], x12 = i12, x13 = i13, x14 = key.s[0], x15 = key.s[1];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        H2_CHACHA_QR(x0, x4, x8, x12);
        H2_CHACHA_QR(x1, x5, x9, x13);
        H2_CHACHA_QR(x2, x6, x10, x14);
        H2_CHACHA_QR(x3, x7, x11, x15);
        H2_CHACHA_QR(x0, x5, x10, x15);
        H2_CHACHA_QR(x1, x6, x11, x12);
        H2_CHACHA_QR(x2, x7, x8, x13);
        H2_CHACHA_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + i0, out[1] = x1 + i1, out[2] = x2 + i2, out[3] = x3 + i3;
    out[4] = x4 + key.k[0], out[5] = x5 + key.k[1], out[6] = x6 + key.k[2], out[7] = x7 + key.k[3];
    out[8] = x8 + key.k[4], out[9] = x9 + key.k[5], out[10] = x10 + key.k[6], out[11] = x11 + key.k[7];
    out[12] = x12 + i12, out[13] = x13 + i13, out[14] = x14 + key.s[0], out[15] = x15 + key.s[1];
}
#undef H2_CHACHA_QR

// Fr::from_bytes_wide: w = 16 little-endian words of an integer v = lo + hi * 2^256 < 2^512 -> v mod r, Montgomery (R = 2^256).
// fu_slice gives each half limbs in [0, 2^29) (top limb < 2^24) whatever its 256 bits are, so the two products
// lo * (2^517 mod r) + hi * (2^773 mod r) share one column scan and one reduction inside fu_fused's two-product bound
// (27 * 2^58 < 2^63).  Their sum X is non-negative and below 2 * 2^256 * r, so the result X / 2^261 (+ r at most) lies in
// [0, 1.07 r): its top limb is non-negative, it packs into 8 words, and one conditional subtraction finishes.
H2_HD Fe fr_from_wide_elem(const uint32_t w[16]) {
    Fe lo, hi;
#pragma unroll
    for (int i = 0; i < 8; i++) lo.l[i] = w[i], hi.l[i] = w[8 + i];
    // (lo * WIDE_LO_I - hi * (-WIDE_HI_I)) / 2^261
    const Fu e = fu_mul_sub<FrU>(fu_slice(lo), fu_const<FrU>(FrU::WIDE_LO_I), fu_slice(hi), fu_neg(fu_const<FrU>(FrU::WIDE_HI_I)));
    H2_FU_ASSERT(e.l[8] >= 0 && e.l[8] < (1 << 23));
    uint32_t t[8];
    fu_pack(e, t);
    Fe o;
    fe_cond_sub<FrP>(o, t);
    return o;
}

// element `counter` of the stream: Fr::random's value for the draw that consumes block `counter`
H2_HD Fe fr_random_elem(const ChaChaKey& key, uint64_t counter) {
    uint32_t w[16];
    chacha20_block(key, counter, w);
    return fr_from_wide_elem(w);
}

}  // namespace h2
