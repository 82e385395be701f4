// copies.hip -- the permutation mapping from a circuit's copy constraints on the GPU.
//
// Replaces the host loop permutation::keygen::Assembly::copy (plonk/permutation/keygen.rs:46-103) for callers that can take the ordered
// mapping include/halo2hip.h defines ("permutation mapping from copy constraints"): every cell maps to the next cell of its connected
// component in ascending id(c, r) = c 2^k + r order, the last one back to the least.  A pure function of the set of copies, so:
//
// Plan (Keygen, "Mapping from copies").
//   1. components  cp_init_kernel    parent[x] = x over all n_columns 2^k cells;
//                  cp_hook_kernel    one copy per lane: union-find, the larger root hooked under the smaller by a compare-and-swap, so a
//                                    component's root ends as its least cell;
//                  cp_keys_kernel    a launch of its own after the hooking: the 2 n_copies endpoints flattened to their roots and packed as
//                                    64-bit keys (label << 32) | cell (copies_elem.h), the last sort tile padded with CP_PAD_KEY;
//   2. order       cp_block_sort_kernel / cp_merge_kernel   lookup.hip's design on 64-bit keys: tiles of CP_TILE keys sorted in LDS by a
//                                    bitonic network, then merge-path passes, runs of w keys -> 2w, over a key count that is any multiple of
//                                    the tile (the last pair of runs may be short or single).  Equal keys (a cell that several copies
//                                    touch) stay in: the scatter reads past them;
//   3. scatter     cp_identity_kernel  mapping[c][r] = (c, r), 16-byte stores;
//                  cp_scatter_kernel   the last key of every run of equal keys stores its cell's successor (cp_successor): the next key's
//                                    cell when that has the same label, else the label -- the root, which is the component's least cell
//                                    and, being an endpoint of some copy of a non-trivial component, its first key.
//
// Visibility (cdna_hip_programming.md Guideline 16; the per-XCD L2s are not coherent and a CU's L1 is never refreshed within a launch).
// INVARIANT: parent[x] <= x at all times, and every write to parent[x] inside the hooking and the flattening launch is an agent-scope
// atomic (a compare-and-swap or a min) that lowers it to another cell of x's component.  A load of parent -- however stale: any value
// the word has held since the launch began -- is therefore a cell of x's component that is <= x, and "x is a root" can only be stale
// in one direction (x has been hooked since).  Nothing is decided on a load alone: the one decision, hooking root a under b, is the
// compare-and-swap parent[a]: a -> b, which the memory side settles; when it fails it returns the current parent[a] < a and the lane
// goes on from there.  cp_init_kernel's plain stores are a launch of their own, before.  Every loop strictly lowers a cell id (cp_find:
// x; cp_union: a + b), so each is bounded by the ids themselves; no lane waits for another lane, wave or workgroup.
#include <string.h>
#include <vector>
#include "copies_elem.h"
#include "engine.h"

namespace h2 {

#define CP_THREADS 256
#define CP_TILE 2048                    // keys one workgroup sorts or merges (16 KB of LDS)
#define CP_E (CP_TILE / CP_THREADS)     // consecutive keys per thread of a merge
#define CP_MAX_COLUMNS 65535            // one grid row per column
#define CP_MAX_COPIES ((size_t)1 << 30)

__device__ __forceinline__ uint32_t cp_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this lane can see, halving the path on the way: parent[x] drops to its grandparent by an atomic min.
// x strictly decreases from one round to the next.
__device__ __forceinline__ uint32_t cp_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cp_ld(parent + x);
        if (p >= x) return x;  // p == x: a root (p > x never holds; read as a root, the loop still ends)
        const uint32_t g = cp_ld(parent + p);
        if (g >= p) return p;
        (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// join the components of a and b.  Each round ends the loop or lowers a + b: cp_find never raises either, and a failed compare-and-swap
// hands back a parent below a.
__device__ __forceinline__ void cp_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cp_find(parent, a);
        b = cp_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t seen = a;  // hook the larger root a under b, if a is still a root
        if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = seen;           // it was hooked meanwhile, under seen < a
    }
}

__device__ __forceinline__ bool cp_copy_ok(const uint4& cp, uint32_t k, uint32_t m) {
    const uint64_t n = 1ull << k;
    return cp.x < m && cp.z < m && cp.y < n && cp.w < n;
}

// ---- 1. components ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CP_THREADS) cp_init_kernel(uint32_t* parent, uint64_t cells) {
    const uint64_t quads = cells / 4, stride = gridDim.x * (uint64_t)CP_THREADS, t = blockIdx.x * (uint64_t)CP_THREADS + threadIdx.x;
    for (uint64_t q = t; q < quads; q += stride) {
        const uint32_t x = (uint32_t)(4 * q);
        ((uint4*)parent)[q] = make_uint4(x, x + 1, x + 2, x + 3);
    }
    if (t < cells - 4 * quads) parent[4 * quads + t] = (uint32_t)(4 * quads + t);
}

__global__ void __launch_bounds__(CP_THREADS) cp_hook_kernel(const uint4* copies, uint64_t n_copies, uint32_t* parent, uint32_t k, uint32_t m,
                                                             uint32_t* flag) {
    for (uint64_t i = blockIdx.x * (uint64_t)CP_THREADS + threadIdx.x; i < n_copies; i += gridDim.x * (uint64_t)CP_THREADS) {
        const uint4 cp = copies[i];
        if (!cp_copy_ok(cp, k, m)) {
            atomicOr(flag, 1u);
            continue;
        }
        cp_union(parent, cp_cell(cp.x, cp.y, k), cp_cell(cp.z, cp.w, k));
    }
}

// keys[2 i], keys[2 i + 1] = the two endpoints of copy i under their roots; CP_PAD_KEY for a copy out of range and from 2 n_copies on
__global__ void __launch_bounds__(CP_THREADS) cp_keys_kernel(const uint4* copies, uint64_t n_copies, uint32_t* parent, uint64_t* keys,
                                                             uint64_t total, uint32_t k, uint32_t m) {
    for (uint64_t i = blockIdx.x * (uint64_t)CP_THREADS + threadIdx.x; i < total; i += gridDim.x * (uint64_t)CP_THREADS) {
        uint64_t key = CP_PAD_KEY;
        if (i < 2 * n_copies) {
            const uint4 cp = copies[i >> 1];
            if (cp_copy_ok(cp, k, m)) {
                const uint32_t cell = i & 1 ? cp_cell(cp.z, cp.w, k) : cp_cell(cp.x, cp.y, k);
                key = cp_key(cp_find(parent, cell), cell);
            }
        }
        keys[i] = key;
    }
}

// ---- 2. order ---------------------------------------------------------------------------------------------------------------------
// every tile of CP_TILE keys sorted ascending, in place
__global__ void __launch_bounds__(CP_THREADS) cp_block_sort_kernel(uint64_t* keys) {
    __shared__ uint64_t sk[CP_TILE];
    uint64_t* g = keys + (uint64_t)blockIdx.x * CP_TILE;
    for (uint32_t i = threadIdx.x; i < CP_TILE; i += CP_THREADS) sk[i] = g[i];
    __syncthreads();
    for (uint32_t kk = 2; kk <= CP_TILE; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < CP_TILE / 2; t += CP_THREADS) {
                const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;  // the pair (i, i + j), bit j of i clear
                const bool asc = (i & kk) == 0;                       // kk == CP_TILE: bit kk of i is clear, the whole tile ascends
                const uint64_t a = sk[i], b = sk[l];
                if (cp_key_lt(b, a) == asc && a != b) {
                    sk[i] = b;
                    sk[l] = a;
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < CP_TILE; i += CP_THREADS) g[i] = sk[i];
}

// merge path: how many of the first d outputs of merge(A[0 .. na), B[0 .. nb)) come from A (on ties A first)
template <class I>
__device__ __forceinline__ I cp_split(const uint64_t* A, I na, const uint64_t* B, I nb, I d) {
    I lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (!cp_key_lt(B[d - 1 - mid], A[mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one merge pass over `total` keys (a multiple of CP_TILE): sorted runs of w keys (w a multiple of CP_TILE) -> runs of 2w.  The last
// pair may hold a short second run or none.  A workgroup produces one tile of the output: its slices of the two runs, found by merge
// path on global memory, are staged in LDS and merged there.
__global__ void __launch_bounds__(CP_THREADS) cp_merge_kernel(const uint64_t* src, uint64_t* dst, uint64_t total, uint64_t w) {
    __shared__ uint64_t sk[CP_TILE];
    __shared__ uint64_t s_a[2];
    const uint64_t o0 = (uint64_t)blockIdx.x * CP_TILE;
    const uint64_t pbase = o0 / (2 * w) * (2 * w);
    const uint64_t left = total - pbase, run_a = left < w ? left : w, run_b = left - run_a < w ? left - run_a : w;
    const uint64_t* gA = src + pbase;
    const uint64_t* gB = gA + run_a;
    const uint64_t d0 = o0 - pbase;  // d0 + CP_TILE <= run_a + run_b: total and w are multiples of the tile
    const uint32_t tid = threadIdx.x;
    if (tid < 2) s_a[tid] = cp_split<uint64_t>(gA, run_a, gB, run_b, d0 + tid * CP_TILE);
    __syncthreads();
    const uint64_t a0 = s_a[0], b0 = d0 - a0;
    const uint32_t na = (uint32_t)(s_a[1] - a0), nb = CP_TILE - na;
    for (uint32_t i = tid; i < CP_TILE; i += CP_THREADS) sk[i] = i < na ? gA[a0 + i] : gB[b0 + (i - na)];
    __syncthreads();
    const uint64_t* A = sk;
    const uint64_t* B = sk + na;
    const uint32_t d = tid * CP_E;
    uint32_t ia = cp_split<uint32_t>(A, na, B, nb, d), ib = d - ia;
    uint64_t r[CP_E];
#pragma unroll
    for (int e = 0; e < CP_E; e++) {
        const bool take_a = ib >= nb || (ia < na && !cp_key_lt(B[ib], A[ia]));
        r[e] = take_a ? A[ia] : B[ib];
        if (take_a) ia++;
        else ib++;
    }
    __syncthreads();  // every lane has read its inputs: the tile goes back through LDS so that the stores are coalesced
#pragma unroll
    for (int e = 0; e < CP_E; e++) sk[d + e] = r[e];
    __syncthreads();
    for (uint32_t i = tid; i < CP_TILE; i += CP_THREADS) dst[o0 + i] = sk[i];
}

// ---- 3. scatter -------------------------------------------------------------------------------------------------------------------
// maps[j][i] = (j, i), j = blockIdx.y; 16-byte stores where the column's pointer allows them
__global__ void __launch_bounds__(CP_THREADS) cp_identity_kernel(uint2* const* maps, uint64_t n) {
    uint2* map = maps[blockIdx.y];
    const uint32_t j = blockIdx.y;
    const uint64_t t = blockIdx.x * (uint64_t)CP_THREADS + threadIdx.x, stride = gridDim.x * (uint64_t)CP_THREADS;
    if (((uintptr_t)map & 15) == 0 && (n & 1) == 0) {
        for (uint64_t q = t; q < n / 2; q += stride) ((uint4*)map)[q] = make_uint4(j, (uint32_t)(2 * q), j, (uint32_t)(2 * q + 1));
    } else {
        for (uint64_t i = t; i < n; i += stride) map[i] = make_uint2(j, (uint32_t)i);
    }
}

// keys: sorted, `total` of them.  The last key of each run of equal keys stores its cell's successor; CP_PAD_KEY stores nothing.
__global__ void __launch_bounds__(CP_THREADS) cp_scatter_kernel(const uint64_t* keys, uint64_t total, uint2* const* maps, uint32_t k) {
    for (uint64_t i = blockIdx.x * (uint64_t)CP_THREADS + threadIdx.x; i < total; i += gridDim.x * (uint64_t)CP_THREADS) {
        const uint64_t key = keys[i];
        if (key == CP_PAD_KEY) continue;
        const uint64_t next = i + 1 < total ? keys[i + 1] : CP_PAD_KEY;
        if (next == key) continue;
        const uint32_t cell = cp_key_cell(key), succ = cp_successor(key, next);
        maps[cp_cell_column(cell, k)][cp_cell_row(cell, k)] = make_uint2(cp_cell_column(succ, k), cp_cell_row(succ, k));
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static uint32_t cp_grid(uint64_t items) {
    uint64_t g = (items + CP_THREADS - 1) / CP_THREADS;
    return (uint32_t)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}
static uint64_t cp_total_keys(size_t n_copies) { return (2 * (uint64_t)n_copies + CP_TILE - 1) / CP_TILE * CP_TILE; }
static uint32_t cp_passes(uint64_t total) {
    uint32_t passes = 0;
    for (uint64_t w = CP_TILE; w < total; w <<= 1) passes++;
    return passes;
}

// Validated arguments; d_copies device memory, maps a host array of m device pointers.  The caller holds the workspaces.  Everything is
// enqueued on s; *d_flag_out points at the word the hooking kernel raises for a copy out of range.
static int copies_mapping_enqueue(Ctx* c, uint32_t k, uint32_t m, const void* d_copies, size_t n_copies, void* const* maps, hipStream_t s,
                                  uint32_t** d_flag_out) {
    const uint64_t n = 1ull << k, cells = (uint64_t)m << k, total = cp_total_keys(n_copies);
    Carve ws;
    const size_t o_flag = ws.take(256), o_blob = ws.take((size_t)m * sizeof(void*)), o_parent = ws.take(n_copies ? cells * sizeof(uint32_t) : 0),
                 o_k0 = ws.take(total * sizeof(uint64_t)), o_k1 = ws.take(total * sizeof(uint64_t));
    int rc = c->copies_ws.ensure(ws.total);
    if (rc) return rc;
    char* base = (char*)c->copies_ws.p;
    uint32_t* d_flag = (uint32_t*)(base + o_flag);
    uint2* const* d_maps = (uint2* const*)(base + o_blob);
    uint32_t* parent = (uint32_t*)(base + o_parent);
    uint64_t* k0 = (uint64_t*)(base + o_k0);
    uint64_t* k1 = (uint64_t*)(base + o_k1);
    *d_flag_out = d_flag;
    H2_CHECK(hipMemsetAsync(d_flag, 0, 256, s));
    if ((rc = c->stage_h2d(base + o_blob, maps, (size_t)m * sizeof(void*), s))) return rc;
    const uint64_t* sorted = k0;
    if (n_copies) {
        int tm = c->timer_begin("copies_components", s);
        hipLaunchKernelGGL(cp_init_kernel, dim3(cp_grid(cells / 4 + 4)), dim3(CP_THREADS), 0, s, parent, cells);
        H2_CHECK(hipGetLastError());
        hipLaunchKernelGGL(cp_hook_kernel, dim3(cp_grid(n_copies)), dim3(CP_THREADS), 0, s, (const uint4*)d_copies, (uint64_t)n_copies, parent, k, m,
                           d_flag);
        H2_CHECK(hipGetLastError());
        hipLaunchKernelGGL(cp_keys_kernel, dim3(cp_grid(total)), dim3(CP_THREADS), 0, s, (const uint4*)d_copies, (uint64_t)n_copies, parent, k0, total,
                           k, m);
        H2_CHECK(hipGetLastError());
        c->timer_end(tm, s);
        tm = c->timer_begin("copies_sort", s);
        hipLaunchKernelGGL(cp_block_sort_kernel, dim3((uint32_t)(total / CP_TILE)), dim3(CP_THREADS), 0, s, k0);
        H2_CHECK(hipGetLastError());
        uint64_t* from = k0;
        uint64_t* to = k1;
        for (uint64_t w = CP_TILE; w < total; w <<= 1) {
            hipLaunchKernelGGL(cp_merge_kernel, dim3((uint32_t)(total / CP_TILE)), dim3(CP_THREADS), 0, s, (const uint64_t*)from, to, total, w);
            H2_CHECK(hipGetLastError());
            uint64_t* t = from;
            from = to;
            to = t;
        }
        sorted = from;
        c->timer_end(tm, s);
    }
    int tm = c->timer_begin("copies_scatter", s);
    hipLaunchKernelGGL(cp_identity_kernel, dim3(cp_grid((n + 1) / 2), m), dim3(CP_THREADS), 0, s, d_maps, n);
    H2_CHECK(hipGetLastError());
    if (n_copies) {
        hipLaunchKernelGGL(cp_scatter_kernel, dim3(cp_grid(total)), dim3(CP_THREADS), 0, s, sorted, total, d_maps, k);
        H2_CHECK(hipGetLastError());
    }
    c->timer_end(tm, s);
    return 0;
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "permutation mapping from copy constraints") ---------------------------------------------------------
static int cp_args_check(const char* what, uint32_t k, uint32_t m, const void* copies, size_t n_copies, const void* const* mapping) {
    if (int rc = check_k(what, k)) return rc;
    if (m > CP_MAX_COLUMNS) {
        set_error("%s: n_columns %u > %d", what, m, CP_MAX_COLUMNS);
        return H2HIP_EINVAL;
    }
    if (((uint64_t)m << k) > (1ull << 32)) {
        set_error("%s: n_columns * 2^k = %u * 2^%u > 2^32: cell ids are 32-bit", what, m, k);
        return H2HIP_EINVAL;
    }
    if (n_copies > CP_MAX_COPIES) {
        set_error("%s: n_copies %zu > 2^30", what, n_copies);
        return H2HIP_EINVAL;
    }
    if (n_copies && !copies) {
        set_error("%s: null copies", what);
        return H2HIP_EINVAL;
    }
    return check_ptrs(what, mapping, m, "mapping");
}

int h2hip_permutation_mapping_device(uint32_t k, uint32_t n_columns, const void* d_copies, size_t n_copies, void* const* d_mapping, void* stream) {
    const char* what = "permutation_mapping";
    if (int rc = cp_args_check(what, k, n_columns, d_copies, n_copies, (const void* const*)d_mapping)) return rc;
    if (n_copies && ((uintptr_t)d_copies & 15)) {
        set_error("%s: d_copies is not 16-byte aligned", what);
        return H2HIP_EINVAL;
    }
    for (uint32_t j = 0; j < n_columns; j++)
        if ((uintptr_t)d_mapping[j] & 7) {
            set_error("%s: d_mapping[%u] is not 8-byte aligned", what, j);
            return H2HIP_EINVAL;
        }
    if (n_columns == 0) return 0;
    Entry en("h2hip_permutation_mapping_device", d_mapping[0]);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = (hipStream_t)stream;
    int rc = c->copies_flag.ensure(sizeof(uint32_t));
    if (rc) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    uint32_t* d_flag = nullptr;
    if ((rc = copies_mapping_enqueue(c, k, n_columns, d_copies, n_copies, d_mapping, s, &d_flag))) return rc;
    H2_CHECK(hipMemcpyAsync(c->copies_flag.p, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    if (*(const uint32_t*)c->copies_flag.p) {
        set_error("%s: a copy has a column >= n_columns or a row >= 2^k; such copies were ignored, the mapping is that of the others", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

int h2hip_permutation_mapping(uint32_t k, uint32_t n_columns, const uint32_t* copies, size_t n_copies, uint32_t* const* mapping) {
    const char* what = "permutation_mapping";
    if (int rc = cp_args_check(what, k, n_columns, copies, n_copies, (const void* const*)mapping)) return rc;
    const size_t n = (size_t)1 << k;
    for (size_t i = 0; i < n_copies; i++) {  // the copies are host memory: a bad one answers the same with and without a GPU
        const uint32_t* cp = copies + 4 * i;
        if (cp[0] >= n_columns || cp[2] >= n_columns || cp[1] >= n || cp[3] >= n) {
            set_error("%s: copies[%zu] = (%u, %u) - (%u, %u) is out of range (n_columns = %u, 2^k = %zu)", what, i, cp[0], cp[1], cp[2], cp[3],
                      n_columns, n);
            return H2HIP_EINVAL;
        }
    }
    if (n_columns == 0) return 0;
    Entry en("h2hip_permutation_mapping");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t map_b = n * 8;
    char *d_copies = nullptr, *d_map = nullptr;
    HostIo io(c, c->host_io, s, true);
    io.in(copies, n_copies * 16, &d_copies);
    const size_t o_maps = io.room((size_t)n_columns * map_b, &d_map);
    for (uint32_t j = 0; j < n_columns; j++) io.out_at(mapping[j], map_b, o_maps + j * map_b);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = io.upload())) return rc;
    std::vector<void*> d_maps(n_columns);
    for (uint32_t j = 0; j < n_columns; j++) d_maps[j] = d_map + j * map_b;
    uint32_t* d_flag = nullptr;
    if ((rc = copies_mapping_enqueue(c, k, n_columns, d_copies, n_copies, d_maps.data(), s, &d_flag))) return rc;
    if ((rc = io.finish())) return rc;
    return guard.release();
}

int h2hip_debug_copies_sort_plan(size_t n_copies, uint32_t out[2]) {
    if (!out || n_copies > CP_MAX_COPIES) {
        set_error("debug_copies_sort_plan: null argument, or n_copies > 2^30");
        return H2HIP_EINVAL;
    }
    out[0] = CP_TILE;
    out[1] = cp_passes(cp_total_keys(n_copies));
    return 0;
}
}  // extern "C"
