// sigma_gather.hip -- A/B of the two ways to build the permutation key's sigma table (Keygen, "Tried"):
//   gather    the reference's shape (plonk/permutation/keygen.rs:124-151): deltaomega, m tables of 2^k elements, materialised once, then
//             out[j][i] = deltaomega[c][r] for (c, r) = mapping[j][i] -- a 32-byte load by data-dependent row, no arithmetic;
//   factored  what csrc/keygen.hip does: out[j][i] = LO[r mod 2^h] * HI_c[r >> h], h = ceil(k / 2), m + 1 tables of at most 2^14 entries.
// Both kernels read the same mapping and write the same bytes (checked on the device).  Mappings: "tenth" = the identity with a tenth of
// the cells pointing at random cells (tools/keygen_bench.py's shape), "random" = every cell at a random cell.  m = 9; the table builds are
// not timed (the gather's costs m * 2^k products once per key, the factored one's (m + 1) * 2^(k/2)).  Median of 7 after 2 warm-ups.
//   hipcc -O3 --offload-arch=gfx950 -Ihalo2-pse_amd/csrc -o tools/sigma_gather tools/sigma_gather.hip && tools/sigma_gather [k ...]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "field.h"
using namespace h2;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
#define THREADS 256
#define M 9u

__device__ __forceinline__ Fe ld(const Fe* p, uint64_t i) {
    const uint4* q = (const uint4*)(p + i);
    uint4 a = q[0], b = q[1];
    Fe o;
    o.l[0] = a.x, o.l[1] = a.y, o.l[2] = a.z, o.l[3] = a.w, o.l[4] = b.x, o.l[5] = b.y, o.l[6] = b.z, o.l[7] = b.w;
    return o;
}
__device__ __forceinline__ void st(Fe* p, uint64_t i, const Fe& v) {
    uint4* q = (uint4*)(p + i);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// map[j * n + i]: kind 0 = identity with one cell in ten at a random cell, 1 = every cell at a random cell
__global__ void map_kernel(uint2* map, uint32_t k, int kind) {
    const uint64_t t = blockIdx.x * (uint64_t)THREADS + threadIdx.x, n = 1ull << k;
    if (t >= M * n) return;
    const uint32_t h = mix((uint32_t)t * 2654435761u + 17u), g = mix(h + 0x9e3779b9u);
    const bool far = kind == 1 || h % 10 == 0;
    map[t] = far ? make_uint2(g % M, mix(g) & (uint32_t)(n - 1)) : make_uint2((uint32_t)(t >> k), (uint32_t)(t & (n - 1)));
}
// full[c * n + r] = delta^c omega^r; lohi: LO[i] = omega^i, i < lo_n, then HI_c[i] = delta^c omega^(i lo_n), i < hi_n
__global__ void tables_kernel(Fe* full, Fe* lohi, Fe omega, Fe delta, uint32_t k, uint32_t lo_bits) {
    const uint64_t t = blockIdx.x * (uint64_t)THREADS + threadIdx.x, n = 1ull << k;
    if (t >= M * n) return;
    const uint32_t c = (uint32_t)(t >> k), r = (uint32_t)(t & (n - 1)), lo_n = 1u << lo_bits, hi_n = 1u << (k - lo_bits);
    const Fe v = fe_mul<FrP>(fe_pow_u64<FrP>(delta, c), fe_pow_u64<FrP>(omega, r));
    st(full, t, v);
    if (c == 0 && r < lo_n) st(lohi, r, v);
    if ((r & (lo_n - 1)) == 0) st(lohi, lo_n + (uint64_t)c * hi_n + (r >> lo_bits), v);
}
__global__ void __launch_bounds__(THREADS) gather_kernel(const uint2* map, const Fe* full, Fe* out, uint32_t k) {
    const uint64_t n = 1ull << k;
    const uint2* mp = map + blockIdx.y * n;
    Fe* o = out + blockIdx.y * n;
    for (uint64_t i = blockIdx.x * (uint64_t)THREADS + threadIdx.x; i < n; i += gridDim.x * (uint64_t)THREADS) {
        const uint2 cr = mp[i];
        st(o, i, ld(full, ((uint64_t)cr.x << k) + cr.y));
    }
}
__global__ void __launch_bounds__(THREADS) factored_kernel(const uint2* map, const Fe* lohi, Fe* out, uint32_t k, uint32_t lo_bits) {
    const uint64_t n = 1ull << k;
    const uint32_t lo_n = 1u << lo_bits, hi_n = 1u << (k - lo_bits);
    const uint2* mp = map + blockIdx.y * n;
    Fe* o = out + blockIdx.y * n;
    for (uint64_t i = blockIdx.x * (uint64_t)THREADS + threadIdx.x; i < n; i += gridDim.x * (uint64_t)THREADS) {
        const uint2 cr = mp[i];
        st(o, i, fe_mul<FrP>(ld(lohi, cr.y & (lo_n - 1)), ld(lohi, lo_n + (uint64_t)cr.x * hi_n + (cr.y >> lo_bits))));
    }
}
__global__ void diff_kernel(const uint4* a, const uint4* b, uint64_t words, uint32_t* bad) {
    const uint64_t t = blockIdx.x * (uint64_t)THREADS + threadIdx.x;
    if (t >= words) return;
    const uint4 x = a[t], y = b[t];
    if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) atomicAdd(bad, 1u);
}

int main(int argc, char** argv) {
    std::vector<uint32_t> ks;
    for (int i = 1; i < argc; i++) ks.push_back((uint32_t)atoi(argv[i]));
    if (ks.empty()) ks = {17, 20, 22};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    Fe root, seven = fe_from_u64<FrP>(7);
    for (int i = 0; i < 8; i++) root.l[i] = FrP::ROOT_OF_UNITY[i];
    const Fe delta = fe_pow_u64<FrP>(seven, 1ull << 28);
    for (uint32_t k : ks) {
        if (k < 2 || k > 24) continue;
        const uint64_t n = 1ull << k, cells = M * n;
        const uint32_t lo_bits = (k + 1) / 2, lo_n = 1u << lo_bits, hi_n = 1u << (k - lo_bits);
        Fe omega = root;
        for (uint32_t i = k; i < FrP::S; i++) omega = fe_sqr<FrP>(omega);
        uint2* map;
        Fe *full, *lohi, *out_a, *out_b;
        uint32_t* bad;
        CK(hipMalloc(&map, cells * 8));
        CK(hipMalloc(&full, cells * 32));
        CK(hipMalloc(&lohi, ((uint64_t)lo_n + (uint64_t)M * hi_n) * 32));
        CK(hipMalloc(&out_a, cells * 32));
        CK(hipMalloc(&out_b, cells * 32));
        CK(hipMalloc(&bad, 4));
        const uint32_t blocks = (uint32_t)((cells + THREADS - 1) / THREADS);
        hipLaunchKernelGGL(tables_kernel, dim3(blocks), dim3(THREADS), 0, 0, full, lohi, omega, delta, k, lo_bits);
        CK(hipDeviceSynchronize());
        const dim3 grid((uint32_t)std::min<uint64_t>((n + THREADS - 1) / THREADS, 8192), M);
        for (int kind = 0; kind < 2; kind++) {
            hipLaunchKernelGGL(map_kernel, dim3(blocks), dim3(THREADS), 0, 0, map, k, kind);
            CK(hipDeviceSynchronize());
            float med[2];
            for (int variant = 0; variant < 2; variant++) {
                std::vector<float> ms;
                for (int r = 0; r < 9; r++) {
                    CK(hipEventRecord(e0));
                    if (variant == 0) hipLaunchKernelGGL(gather_kernel, grid, dim3(THREADS), 0, 0, map, full, out_a, k);
                    else hipLaunchKernelGGL(factored_kernel, grid, dim3(THREADS), 0, 0, map, lohi, out_b, k, lo_bits);
                    CK(hipEventRecord(e1));
                    CK(hipEventSynchronize(e1));
                    float t;
                    CK(hipEventElapsedTime(&t, e0, e1));
                    if (r >= 2) ms.push_back(t);
                }
                std::sort(ms.begin(), ms.end());
                med[variant] = ms[ms.size() / 2];
            }
            CK(hipMemset(bad, 0, 4));
            hipLaunchKernelGGL(diff_kernel, dim3((uint32_t)((cells * 2 + THREADS - 1) / THREADS)), dim3(THREADS), 0, 0, (const uint4*)out_a,
                               (const uint4*)out_b, cells * 2, bad);
            uint32_t h_bad = 1;
            CK(hipMemcpy(&h_bad, bad, 4, hipMemcpyDeviceToHost));
            printf("{\"k\": %u, \"columns\": %u, \"mapping\": \"%s\", \"gather_ms\": %.4f, \"factored_ms\": %.4f, \"floor_ms_40B_at_6.3TBps\": %.4f, "
                   "\"gather_table_MB\": %.0f, \"factored_tables_KB\": %.0f, \"outputs_equal\": %s}\n",
                   k, M, kind ? "random" : "tenth", med[0], med[1], cells * 40.0 / 6.3e9, cells * 32.0 / 1048576.0,
                   ((double)lo_n + (double)M * hi_n) * 32.0 / 1024.0, h_bad ? "false" : "true");
            fflush(stdout);
            if (h_bad) return 1;
        }
        CK(hipFree(map)); CK(hipFree(full)); CK(hipFree(lohi)); CK(hipFree(out_a)); CK(hipFree(out_b)); CK(hipFree(bad));
    }
    return 0;
}
