// serde.hip -- the per-element work of the reference's SerdeFormat (helpers.rs:8-20) on the GPU: what ParamsKZG::read_custom /
// write_custom (poly/kzg/commitment.rs:142-244) and Polynomial::read / write (poly.rs:152-177) do to every point and every scalar
// of a file.  One lane per element:
//   g1_decompress_kernel   Processed read: 32 B (x canonical little-endian, the parity of canonical y in bit 7 of byte 31) -> x || y,
//                          64 B Montgomery (R = 2^256).  One square root per point: fu_sqrt, 251 squarings and 64 products in Fq;
//   g1_compress_kernel     Processed write, the inverse;
//   g1_validate_kernel     RawBytes read (read_raw): both coordinates below q and the point on y^2 = x^3 + 3, or (0, 0);
//   fr_from_repr_kernel    SerdePrimeField, Processed: canonical little-endian -> Montgomery, values >= r rejected (in place allowed);
//   fr_to_repr_kernel      ... and back.
// The encodings are halo2curves 0.3.1's GroupEncoding as DESIGN.md section 2 records them.
// Failure reporting.  A fallible kernel stores 64 zero bytes (32 for Fr) for an element that fails, and leaves ONE BIT per element in
// mask[n / 64], a wave's ballot stored by one lane, as check.hip's first kernels do: nothing is appended and no atomic is issued.
//   sd_count_kernel  (tiles): the set bits of a tile of 256 words and the lowest set bit's index;
//   sd_total_kernel  one workgroup: the sum and the minimum over the tiles -> {invalid elements, lowest invalid index}.
// The result is a function of the input alone.  The two words reach the caller with the call's one synchronisation.
#include "engine.h"
#include "fe_io.h"
#include "lk_dev.h"
#include "serde_elem.h"

namespace h2 {

#define SD_THREADS LK_THREADS
#define SD_MAX_N ((size_t)1 << 30)
#define SD_NONE 0xffffffffu  // no invalid element in this tile (n <= 2^30: every index fits)

// every lane of the workgroup comes here, the ones past n with bad = false; a wave wholly past n stores nothing
__device__ __forceinline__ void sd_mark(uint64_t* mask, uint64_t i, uint64_t n, bool bad) {
    const uint64_t bits = __ballot(bad);
    if ((i & 63) == 0 && i < n) mask[i >> 6] = bits;
}

// `bytes`: n x 32 B; `points`: n x 64 B
__global__ void __launch_bounds__(SD_THREADS, 2) g1_decompress_kernel(const Fe* bytes, Affine* points, uint64_t* mask, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)SD_THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        Affine o;
        bad = !g1_decompress_elem(fe_ld(bytes, i), &o);
        fe_st(&points[i].x, 0, o.x);
        fe_st(&points[i].y, 0, o.y);
    }
    sd_mark(mask, i, n, bad);
}

__global__ void __launch_bounds__(SD_THREADS) g1_compress_kernel(const Affine* points, Fe* bytes, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)SD_THREADS + threadIdx.x;
    if (i >= n) return;
    Affine p;
    p.x = fe_ld(&points[i].x, 0);
    p.y = fe_ld(&points[i].y, 0);
    fe_st(bytes, i, g1_compress_elem(p));
}

__global__ void __launch_bounds__(SD_THREADS) g1_validate_kernel(const Affine* points, uint64_t* mask, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)SD_THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        Affine p;
        p.x = fe_ld(&points[i].x, 0);
        p.y = fe_ld(&points[i].y, 0);
        bad = !g1_validate_elem(p);
    }
    sd_mark(mask, i, n, bad);
}

// out may be repr: a lane reads its element before it writes it
__global__ void __launch_bounds__(SD_THREADS) fr_from_repr_kernel(const Fe* repr, Fe* out, uint64_t* mask, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)SD_THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        Fe o;
        bad = !fr_from_repr_elem(fe_ld(repr, i), &o);
        fe_st(out, i, o);
    }
    sd_mark(mask, i, n, bad);
}

__global__ void __launch_bounds__(SD_THREADS) fr_to_repr_kernel(const Fe* in, Fe* repr, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)SD_THREADS + threadIdx.x;
    if (i >= n) return;
    fe_st(repr, i, fe_to_canonical<FrP>(fe_ld(in, i)));
}

// ---- mask -> {count, lowest index} ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sd_min(uint32_t v, uint32_t* lds) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t off = SD_THREADS / 2; off; off >>= 1) {
        if (tid < off) lds[tid] = min(lds[tid], lds[tid + off]);
        __syncthreads();
    }
    const uint32_t m = lds[0];
    __syncthreads();
    return m;
}

__global__ void __launch_bounds__(SD_THREADS) sd_count_kernel(const uint64_t* mask, uint32_t words, uint32_t* tile_cnt, uint32_t* tile_first) {
    __shared__ uint32_t lds[SD_THREADS];
    const uint32_t w = blockIdx.x * SD_THREADS + threadIdx.x;
    const uint64_t bits = w < words ? mask[w] : 0ull;
    uint32_t total;
    (void)lk_scan_excl((uint32_t)__popcll(bits), lds, &total);
    const uint32_t first = sd_min(bits ? w * 64u + (uint32_t)(__ffsll((unsigned long long)bits) - 1) : SD_NONE, lds);
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = total;
        tile_first[blockIdx.x] = first;
    }
}

__global__ void __launch_bounds__(SD_THREADS) sd_total_kernel(const uint32_t* tile_cnt, const uint32_t* tile_first, uint32_t tiles, uint64_t* invalid) {
    __shared__ uint32_t lds[SD_THREADS];
    uint32_t cnt = 0, first = SD_NONE;  // at most 2^30 elements
    for (uint32_t t = threadIdx.x; t < tiles; t += SD_THREADS) {
        cnt += tile_cnt[t];
        first = min(first, tile_first[t]);
    }
    uint32_t total;
    (void)lk_scan_excl(cnt, lds, &total);
    first = sd_min(first, lds);
    if (threadIdx.x == 0) {
        invalid[0] = total;
        invalid[1] = total ? first : 0u;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
enum SdOp { SD_DECOMPRESS, SD_VALIDATE, SD_FROM_REPR };
static const char* const SD_STAGE[] = {"g1_decompress", "g1_validate", "fr_from_repr"};

// One fallible conversion on s over device memory; waits for s once and leaves the two words in invalid[] (host memory).
static int sd_fallible_device(Ctx* c, SdOp op, const void* d_in, void* d_out, size_t n, uint64_t invalid[2], hipStream_t s) {
    const uint32_t words = (uint32_t)((n + 63) / 64), tiles = (words + SD_THREADS - 1) / SD_THREADS;
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    Carve ws;
    const size_t o_mask = ws.take(words * sizeof(uint64_t)), o_cnt = ws.take(tiles * sizeof(uint32_t)), o_first = ws.take(tiles * sizeof(uint32_t)),
                 o_inv = ws.take(2 * sizeof(uint64_t));
    if ((rc = c->serde_ws.ensure(ws.total))) return rc;
    char* base = (char*)c->serde_ws.p;
    uint64_t* mask = (uint64_t*)(base + o_mask);
    uint32_t *cnt = (uint32_t*)(base + o_cnt), *first = (uint32_t*)(base + o_first);
    uint64_t* d_inv = (uint64_t*)(base + o_inv);
    const dim3 grid((uint32_t)((n + SD_THREADS - 1) / SD_THREADS)), block(SD_THREADS);
    int tm = c->timer_begin(SD_STAGE[op], s);
    if (op == SD_DECOMPRESS) hipLaunchKernelGGL(g1_decompress_kernel, grid, block, 0, s, (const Fe*)d_in, (Affine*)d_out, mask, (uint64_t)n);
    else if (op == SD_VALIDATE) hipLaunchKernelGGL(g1_validate_kernel, grid, block, 0, s, (const Affine*)d_in, mask, (uint64_t)n);
    else hipLaunchKernelGGL(fr_from_repr_kernel, grid, block, 0, s, (const Fe*)d_in, (Fe*)d_out, mask, (uint64_t)n);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sd_count_kernel, dim3(tiles), block, 0, s, mask, words, cnt, first);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sd_total_kernel, dim3(1), block, 0, s, cnt, first, tiles, d_inv);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    H2_CHECK(hipMemcpyAsync(invalid, d_inv, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));  // the workspace's last reader
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    if (invalid[0]) {
        set_error("%s: %llu of %zu elements fail the format's checks, the first at index %llu", SD_STAGE[op], (unsigned long long)invalid[0], n,
                  (unsigned long long)invalid[1]);
        return H2HIP_EENCODING;
    }
    return 0;
}

// The host forms: upload into the staging buffer (engine.h, HostIo), convert there, download.
static int sd_fallible_host(const char* name, SdOp op, const void* in, size_t in_elem, void* out, size_t out_elem, size_t n, uint64_t invalid[2]) {
    Entry en(name);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    char *d_in = nullptr, *d_out = nullptr;
    HostIo io(c, c->host_io, s, true);
    io.in(in, n * in_elem, &d_in);
    io.out(out, n * out_elem, &d_out);  // (nothing when out_elem is 0: the validation)
    if (int rc = io.upload()) return rc;
    const int verdict = sd_fallible_device(c, op, d_in, d_out, n, invalid, s);
    if (verdict && verdict != H2HIP_EENCODING) return verdict;
    if (int rc = io.finish()) return rc;  // all of the output is written, the failing elements as zeros
    return verdict;
}

static int sd_plain_device(bool compress, const void* d_in, void* d_out, size_t n, hipStream_t s) {
    const dim3 grid((uint32_t)((n + SD_THREADS - 1) / SD_THREADS)), block(SD_THREADS);
    if (compress) hipLaunchKernelGGL(g1_compress_kernel, grid, block, 0, s, (const Affine*)d_in, (Fe*)d_out, (uint64_t)n);
    else hipLaunchKernelGGL(fr_to_repr_kernel, grid, block, 0, s, (const Fe*)d_in, (Fe*)d_out, (uint64_t)n);
    H2_CHECK(hipGetLastError());
    return 0;
}

static int sd_plain_host(const char* name, bool compress, const void* in, size_t in_elem, void* out, size_t n) {
    Entry en(name);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    char *d_in = nullptr, *d_out = nullptr;
    HostIo io(c, c->host_io, s, true);
    io.in(in, n * in_elem, &d_in);
    io.out(out, n * 32, &d_out);
    int rc = io.upload();
    if (rc) return rc;
    int tm = c->timer_begin(compress ? "g1_compress" : "fr_to_repr", s);
    if ((rc = sd_plain_device(compress, d_in, d_out, n, s))) return rc;
    c->timer_end(tm, s);
    return io.finish();
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "serialisation") ---------------------------------------------------------------------------------------
static int sd_args(const char* what, const void* in, const void* out, bool has_out, size_t n, const uint64_t* invalid, bool has_invalid) {
    if (n > SD_MAX_N) {
        set_error("%s: n = %zu > 2^30", what, n);
        return H2HIP_EINVAL;
    }
    if (has_invalid && !invalid) {
        set_error("%s: null invalid", what);
        return H2HIP_EINVAL;
    }
    if (n && (!in || (has_out && !out))) {
        set_error("%s: null argument", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

// a fallible call's arguments; invalid[] is cleared so that every successful return, n == 0 included, leaves {0, 0} there
static int sd_fallible_args(const char* what, const void* in, const void* out, bool has_out, size_t n, uint64_t* invalid) {
    if (int rc = sd_args(what, in, out, has_out, n, invalid, true)) return rc;
    invalid[0] = invalid[1] = 0;
    return 0;
}

int h2hip_g1_decompress_bn254_device(const void* d_bytes, size_t n, void* d_points_xy, uint64_t invalid[2], void* stream) {
    if (int rc = sd_fallible_args("g1_decompress", d_bytes, d_points_xy, true, n, invalid)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_g1_decompress_bn254_device", d_bytes);
    if (en.rc) return en.rc;
    return sd_fallible_device(en.c, SD_DECOMPRESS, d_bytes, d_points_xy, n, invalid, (hipStream_t)stream);
}

int h2hip_g1_decompress_bn254(const void* bytes, size_t n, uint64_t* points_xy, uint64_t invalid[2]) {
    if (int rc = sd_fallible_args("g1_decompress", bytes, points_xy, true, n, invalid)) return rc;
    if (n == 0) return 0;
    return sd_fallible_host("h2hip_g1_decompress_bn254", SD_DECOMPRESS, bytes, 32, points_xy, 64, n, invalid);
}

int h2hip_g1_validate_bn254_device(const void* d_points_xy, size_t n, uint64_t invalid[2], void* stream) {
    if (int rc = sd_fallible_args("g1_validate", d_points_xy, nullptr, false, n, invalid)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_g1_validate_bn254_device", d_points_xy);
    if (en.rc) return en.rc;
    return sd_fallible_device(en.c, SD_VALIDATE, d_points_xy, nullptr, n, invalid, (hipStream_t)stream);
}

int h2hip_g1_validate_bn254(const uint64_t* points_xy, size_t n, uint64_t invalid[2]) {
    if (int rc = sd_fallible_args("g1_validate", points_xy, nullptr, false, n, invalid)) return rc;
    if (n == 0) return 0;
    return sd_fallible_host("h2hip_g1_validate_bn254", SD_VALIDATE, points_xy, 64, nullptr, 0, n, invalid);
}

int h2hip_fr_from_repr_bn254_device(const void* d_repr, size_t n, void* d_out, uint64_t invalid[2], void* stream) {
    if (int rc = sd_fallible_args("fr_from_repr", d_repr, d_out, true, n, invalid)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_fr_from_repr_bn254_device", d_repr);
    if (en.rc) return en.rc;
    return sd_fallible_device(en.c, SD_FROM_REPR, d_repr, d_out, n, invalid, (hipStream_t)stream);
}

int h2hip_fr_from_repr_bn254(const void* repr, size_t n, uint64_t* out, uint64_t invalid[2]) {
    if (int rc = sd_fallible_args("fr_from_repr", repr, out, true, n, invalid)) return rc;
    if (n == 0) return 0;
    return sd_fallible_host("h2hip_fr_from_repr_bn254", SD_FROM_REPR, repr, 32, out, 32, n, invalid);
}

int h2hip_g1_compress_bn254_device(const void* d_points_xy, size_t n, void* d_bytes, void* stream) {
    if (int rc = sd_args("g1_compress", d_points_xy, d_bytes, true, n, nullptr, false)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_g1_compress_bn254_device", d_points_xy);
    if (en.rc) return en.rc;
    return sd_plain_device(true, d_points_xy, d_bytes, n, (hipStream_t)stream);
}

int h2hip_g1_compress_bn254(const uint64_t* points_xy, size_t n, void* bytes) {
    if (int rc = sd_args("g1_compress", points_xy, bytes, true, n, nullptr, false)) return rc;
    if (n == 0) return 0;
    return sd_plain_host("h2hip_g1_compress_bn254", true, points_xy, 64, bytes, n);
}

int h2hip_fr_to_repr_bn254_device(const void* d_in, size_t n, void* d_repr, void* stream) {
    if (int rc = sd_args("fr_to_repr", d_in, d_repr, true, n, nullptr, false)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_fr_to_repr_bn254_device", d_in);
    if (en.rc) return en.rc;
    return sd_plain_device(false, d_in, d_repr, n, (hipStream_t)stream);
}

int h2hip_fr_to_repr_bn254(const uint64_t* in, size_t n, void* repr) {
    if (int rc = sd_args("fr_to_repr", in, repr, true, n, nullptr, false)) return rc;
    if (n == 0) return 0;
    return sd_plain_host("h2hip_fr_to_repr_bn254", false, in, 32, repr, n);
}

}  // extern "C"
