// random.hip -- C::Scalar::random over a whole column on the GPU: the loop of vanishing::Argument::commit
// (plonk/vanishing/prover.rs:49-58), which fills a polynomial of 2^k coefficients one draw after the other.  One lane per element:
//   fr_random_kernel     element i = Fr::from_bytes_wide(ChaCha20 block first_block + i of the stream keyed by the seed): what the
//                        reference's loop stores when it is handed ChaCha20Rng::from_seed(seed) positioned at that block.  A draw is
//                        eight next_u64 = exactly one 64-byte block, so the generator is counter-based: any range, in any order;
//   fr_from_wide_kernel  Fr::from_bytes_wide alone over n given 64-byte strings (Challenge255's map as well).
// The per-element code is random_elem.h (ChaCha20 in plain C++, the reduction as one two-product pass of fieldu.h's multiplier); a lane
// forms its 64-bit counter, runs the block in registers and stores its 32 bytes as two 16-byte stores.  No LDS, no atomics, no
// divergence but the grid's tail.  The definitions are rand_chacha 0.3's and halo2curves 0.3.1's as DESIGN.md section 2 records them.
// The engine is a deterministic expander: the seed is the caller's entropy and as secret as the polynomial.  The key reaches the kernel
// as an argument (kernarg memory, read into scalar registers); the host copies this file makes of it are wiped before a call returns.
#include <stdlib.h>

#include "../../include/halo2hip_debug.h"
#include "engine.h"
#include "fe_io.h"
#include "random_elem.h"

namespace h2 {

#define RN_THREADS 256
#define RN_MAX_N ((size_t)1 << 32)  // one launch: 2^24 workgroups
// host forms: below this many elements the per-element code runs on the calling thread (no GPU is touched); from it on the elements
// are generated on the device and downloaded.  HALO2_HIP_RANDOM_MIN_N; the default is the measured break-even ("Randomness")
#define RN_HOST_MIN_N_DEFAULT ((size_t)1 << 9)

// Read before any Entry (a call below the threshold never starts the engine), hence under a TuneRead; for the same reason the
// environment is read here, on the first call, and not with the engine's configuration at init.
static size_t rn_host_min_n() {
    {
        TuneRead r;
        if (tune().random_min_n) return tune().random_min_n;
    }
    static const size_t v = [] {
        const char* e = getenv("HALO2_HIP_RANDOM_MIN_N");
        if (!e || !*e) return RN_HOST_MIN_N_DEFAULT;
        char* end = nullptr;
        const unsigned long long x = strtoull(e, &end, 0);
        return end == e ? RN_HOST_MIN_N_DEFAULT : (size_t)x;
    }();
    return v;
}

// the compiler may not drop these stores though the object dies right after them
static void rn_wipe(void* p, size_t bytes) {
    volatile uint8_t* q = (volatile uint8_t*)p;
    for (size_t i = 0; i < bytes; i++) q[i] = 0;
}

__global__ void __launch_bounds__(RN_THREADS) fr_random_kernel(ChaChaKey key, uint64_t first_block, Fe* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)RN_THREADS + threadIdx.x;
    if (i >= n) return;
    fe_st(out, i, fr_random_elem(key, first_block + i));  // the caller has checked that first_block + n does not pass 2^64
}

// `bytes`: n x 64 B, 16-byte aligned
__global__ void __launch_bounds__(RN_THREADS) fr_from_wide_kernel(const uint4* bytes, Fe* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)RN_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint4* q = bytes + 4 * i;
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    const uint32_t w[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    fe_st(out, i, fr_from_wide_elem(w));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static int rn_random_device(Ctx* c, const ChaChaKey& key, uint64_t first_block, size_t n, void* d_out, hipStream_t s) {
    const dim3 grid((uint32_t)((n + RN_THREADS - 1) / RN_THREADS)), block(RN_THREADS);
    int tm = c->timer_begin("fr_random", s);
    hipLaunchKernelGGL(fr_random_kernel, grid, block, 0, s, key, first_block, (Fe*)d_out, (uint64_t)n);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return 0;
}

static int rn_wide_device(Ctx* c, const void* d_bytes, size_t n, void* d_out, hipStream_t s) {
    const dim3 grid((uint32_t)((n + RN_THREADS - 1) / RN_THREADS)), block(RN_THREADS);
    int tm = c->timer_begin("fr_from_wide", s);
    hipLaunchKernelGGL(fr_from_wide_kernel, grid, block, 0, s, (const uint4*)d_bytes, (Fe*)d_out, (uint64_t)n);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return 0;
}

// The host forms from the threshold on: generate into the staging buffer (engine.h, HostIo), download.
static int rn_random_host(const ChaChaKey& key, uint64_t first_block, size_t n, uint64_t* out) {
    Entry en("h2hip_fr_random_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    char* d_out = nullptr;
    HostIo io(c, c->host_io, s);
    io.out(out, n * 32, &d_out);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = rn_random_device(c, key, first_block, n, d_out, s))) return rc;
    return io.finish();
}

static int rn_wide_host(const uint8_t* bytes, size_t n, uint64_t* out) {
    Entry en("h2hip_fr_from_bytes_wide_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    char *d_in = nullptr, *d_out = nullptr;
    HostIo io(c, c->host_io, s, true);
    io.in(bytes, n * 64, &d_in);
    io.out(out, n * 32, &d_out);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = rn_wide_device(c, d_in, n, d_out, s))) return rc;
    return io.finish();
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "randomness") --------------------------------------------------------------------------------------------
static int rn_args(const char* what, const void* in, const char* in_name, const void* out, size_t n) {
    if (n > RN_MAX_N) {
        set_error("%s: n = %zu > 2^32", what, n);
        return H2HIP_EINVAL;
    }
    if (n && !in) {
        set_error("%s: null %s", what, in_name);
        return H2HIP_EINVAL;
    }
    if (n && !out) {
        set_error("%s: null output", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int rn_random_args(const char* what, const uint8_t* seed, uint64_t first_block, size_t n, const void* out) {
    if (int rc = rn_args(what, seed, "seed", out, n)) return rc;
    if (n && (uint64_t)(n - 1) > ~first_block) {  // the last block, first_block + n - 1, must be below 2^64
        set_error("%s: first_block + n = %llu + %zu exceeds 2^64", what, (unsigned long long)first_block, n);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int rn_aligned(const char* what, const void* p, const char* name) {
    if ((uintptr_t)p & 15) {
        set_error("%s: %s is not 16-byte aligned", what, name);
        return H2HIP_EINVAL;
    }
    return 0;
}

int h2hip_fr_random_bn254_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first_block, size_t n, void* d_out, void* stream) {
    if (int rc = rn_random_args("fr_random", seed, first_block, n, d_out)) return rc;
    if (n == 0) return 0;
    if (int rc = rn_aligned("fr_random", d_out, "d_out")) return rc;
    Entry en("h2hip_fr_random_bn254_device", d_out);
    if (en.rc) return en.rc;
    ChaChaKey key = chacha_key(seed, stream_id);
    const int rc = rn_random_device(en.c, key, first_block, n, d_out, (hipStream_t)stream);
    rn_wipe(&key, sizeof key);
    return rc;
}

int h2hip_fr_random_bn254(const uint8_t seed[32], uint64_t stream_id, uint64_t first_block, size_t n, uint64_t* out) {
    if (int rc = rn_random_args("fr_random", seed, first_block, n, out)) return rc;
    if (n == 0) return 0;
    ChaChaKey key = chacha_key(seed, stream_id);
    int rc = 0;
    if (n < rn_host_min_n()) {
        for (size_t i = 0; i < n; i++) {
            const Fe e = fr_random_elem(key, first_block + i);
            memcpy(out + 4 * i, e.l, 32);  // caller memory is only 8-byte aligned
        }
    } else {
        rc = rn_random_host(key, first_block, n, out);
    }
    rn_wipe(&key, sizeof key);
    return rc;
}

int h2hip_fr_from_bytes_wide_bn254_device(const void* d_bytes, size_t n, void* d_out, void* stream) {
    if (int rc = rn_args("fr_from_bytes_wide", d_bytes, "bytes", d_out, n)) return rc;
    if (n == 0) return 0;
    if (int rc = rn_aligned("fr_from_bytes_wide", d_bytes, "d_bytes")) return rc;
    if (int rc = rn_aligned("fr_from_bytes_wide", d_out, "d_out")) return rc;
    Entry en("h2hip_fr_from_bytes_wide_bn254_device", d_bytes);
    if (en.rc) return en.rc;
    return rn_wide_device(en.c, d_bytes, n, d_out, (hipStream_t)stream);
}

int h2hip_fr_from_bytes_wide_bn254(const uint8_t* bytes, size_t n, uint64_t* out) {
    if (int rc = rn_args("fr_from_bytes_wide", bytes, "bytes", out, n)) return rc;
    if (n == 0) return 0;
    if (n >= rn_host_min_n()) return rn_wide_host(bytes, n, out);
    for (size_t i = 0; i < n; i++) {
        uint32_t w[16];
        memcpy(w, bytes + 64 * i, 64);
        const Fe e = fr_from_wide_elem(w);
        memcpy(out + 4 * i, e.l, 32);
    }
    return 0;
}

// ---- debug hook (include/halo2hip_debug.h) ------------------------------------------------------------------------------------------------
int h2hip_debug_set_random_min_n(size_t n) {
    TuneWrite()->random_min_n = n;
    return 0;
}

}  // extern "C"
