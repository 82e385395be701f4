// check.hip -- the three column-wide loops of MockProver::verify (dev.rs:603-1300) over the prover's own columns on the GPU: every gate
// polynomial at every row (:676-746), every lookup input against its table (:751-886), every cell of the permutation against the cell
// it maps to (:889-931).  The rest of MockProver (regions, names, CellNotAssigned, Poison, selector checks) is host bookkeeping and
// stays out.
//
// Plan (Witness check).  A check has `items` constraints (gate polynomials, permutation columns, lookups) over n = 2^k
// rows.  Its first kernel leaves ONE BIT per (item, row) in mask[item][n / 64], a wave's ballot stored by one lane, so nothing is
// appended and no global atomic is issued per row:
//   gates        check_gates_kernel (evalh.hip, on evaluate_h's interpreter: the canonical value is tested for zero in registers);
//   permutation  ck_perm_kernel     one lane per cell, columns[j][i] against columns[c][r] as two uint4 pairs; a pair out of range is
//                                   never dereferenced and raises the call's flag;
//   lookups      lookup.hip's sort of table[0 .. u) (rows >= u become all-ones keys, above every canonical value), then
//                ck_lookup_kernel   one binary search per input row i < u on canonical keys.
//   shuffles     (the argument of upstream PSE halo2) the same sort of input[0 .. u) and shuffle[0 .. u), then
//                ck_shuffle_kernel  the value of input row i < u must occur equally often in both: lower and upper bound in each.
//                Upstream's MockProver reports the mismatching positions of the two sorted lists; this is the per-row form that the
//                counts / rows convention needs, and it fails somewhere exactly when the multisets differ.
// The same tail follows, in the pattern of lk_count_kernel / lk_scan_kernel:
//   ck_count_kernel    (tiles x items): the set bits of a tile of 256 words (16 384 rows);
//   ck_scan_kernel     one workgroup per item: exclusive scan of the tile counts, the total is the item's count;
//   ck_compact_kernel  (tiles x items): the rows of the set bits in ascending order at their scanned offset, up to max_rows; a tile
//                      whose offset is past max_rows leaves at once.  The row lists are preset to UINT32_MAX.
// The result is a function of the mask alone, hence of the inputs alone.  All of a call's kernels and copies run on the caller's stream
// under one ws_acquire / WsGuard; counts and rows reach the caller with the call's one synchronisation.  No kernel uses scratch
// outside the interpreter's scratch tiers (profiles/check_resources.txt).
#include <string.h>
#include <vector>
#include "engine.h"
#include "fe_io.h"
#include "lk_dev.h"

namespace h2 {

#define CK_THREADS LK_THREADS
#define CK_MAX_ITEMS 65535   // one grid row per item
#define CK_MAX_LOOKUPS 32767
#define CK_MAX_ROWS 65535

// ---- the first kernels of the permutation and lookup checks ------------------------------------------------------------------------
__global__ void __launch_bounds__(CK_THREADS) ck_perm_kernel(const Fe* const* cols, const uint2* const* maps, uint64_t* mask, uint32_t words,
                                                             uint32_t k, uint32_t m, uint32_t* flag) {
    const uint64_t n = 1ull << k, i = blockIdx.x * (uint64_t)CK_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = blockIdx.y;
    const uint2 cr = maps[j][i];
    bool bad = false;
    if (cr.x >= m || cr.y >= n) atomicOr(flag, 1u);  // the caller's contract is broken: H2HIP_EINVAL, the pair is not followed
    else bad = !fe_eq(fe_ld(cols[j], i), fe_ld(cols[cr.x], cr.y));
    const uint64_t bits = __ballot(bad);
    if ((i & 63) == 0) mask[(size_t)j * words + (i >> 6)] = bits;
}

// in[j]: the compressed input, Montgomery form; sorted[j]: the canonical keys of table rows 0 .. u - 1 in ascending order
__global__ void __launch_bounds__(CK_THREADS) ck_lookup_kernel(const Fe* const* in, const Fe* const* sorted, uint64_t* mask, uint32_t words,
                                                               uint32_t k, uint64_t u) {
    const uint64_t n = 1ull << k, i = blockIdx.x * (uint64_t)CK_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = blockIdx.y;
    bool bad = false;
    if (i < u) {
        const Fe v = fe_to_canonical<FrP>(fe_ld(in[j], i));
        const Fe* t = sorted[j];
        uint64_t lo = 0, hi = u;  // lower bound: every t[< lo] < v
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key_lt(fe_ld(t, mid), v)) lo = mid + 1;
            else hi = mid;
        }
        bad = lo >= u || !fe_eq(fe_ld(t, lo), v);
    }
    const uint64_t bits = __ballot(bad);
    if ((i & 63) == 0) mask[(size_t)j * words + (i >> 6)] = bits;
}

// first index in t[0 .. u) (canonical keys, ascending) whose key is not below v (upper: is above v)
__device__ __forceinline__ uint64_t ck_bound(const Fe* t, uint64_t u, const Fe& v, bool upper) {
    uint64_t lo = 0, hi = u;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const Fe m = fe_ld(t, mid);
        if (upper ? !key_lt(v, m) : key_lt(m, v)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// in[j]: the compressed input, Montgomery form; sa[j], ss[j]: the canonical keys of input and shuffle rows 0 .. u - 1 in ascending order.
// Row i < u fails when its value's multiplicity differs between the two: four binary searches, every index below u.
__global__ void __launch_bounds__(CK_THREADS) ck_shuffle_kernel(const Fe* const* in, const Fe* const* sa, const Fe* const* ss, uint64_t* mask,
                                                                uint32_t words, uint32_t k, uint64_t u) {
    const uint64_t n = 1ull << k, i = blockIdx.x * (uint64_t)CK_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = blockIdx.y;
    bool bad = false;
    if (i < u) {
        const Fe v = fe_to_canonical<FrP>(fe_ld(in[j], i));
        const uint64_t in_a = ck_bound(sa[j], u, v, true) - ck_bound(sa[j], u, v, false);
        const uint64_t in_s = ck_bound(ss[j], u, v, true) - ck_bound(ss[j], u, v, false);
        bad = in_a != in_s;
    }
    const uint64_t bits = __ballot(bad);
    if ((i & 63) == 0) mask[(size_t)j * words + (i >> 6)] = bits;
}

// ---- the tail: mask -> counts and the lowest failing rows ---------------------------------------------------------------------------
// tile_cnt[item][tiles + 1]: per-tile counts, then their exclusive scan
__global__ void __launch_bounds__(CK_THREADS) ck_count_kernel(const uint64_t* mask, uint32_t words, uint32_t* tile_cnt, uint32_t tiles) {
    __shared__ uint32_t lds[CK_THREADS];
    const uint32_t w = blockIdx.x * CK_THREADS + threadIdx.x;
    const uint32_t pc = w < words ? (uint32_t)__popcll(mask[(size_t)blockIdx.y * words + w]) : 0u;
    uint32_t total;
    (void)lk_scan_excl(pc, lds, &total);
    if (threadIdx.x == 0) tile_cnt[(size_t)blockIdx.y * (tiles + 1) + blockIdx.x] = total;
}

__global__ void __launch_bounds__(CK_THREADS) ck_scan_kernel(uint32_t* tile_cnt, uint32_t tiles, uint64_t* counts) {
    __shared__ uint32_t lds[CK_THREADS];
    uint32_t* cnt = tile_cnt + (size_t)blockIdx.x * (tiles + 1);
    uint32_t carry = 0;  // at most 2^28 rows
    for (uint32_t base = 0; base < tiles; base += CK_THREADS) {
        const uint32_t t = base + threadIdx.x;
        uint32_t total;
        const uint32_t e = lk_scan_excl(t < tiles ? cnt[t] : 0u, lds, &total);
        if (t < tiles) cnt[t] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) {
        cnt[tiles] = carry;
        counts[blockIdx.x] = carry;
    }
}

__global__ void __launch_bounds__(CK_THREADS) ck_compact_kernel(const uint64_t* mask, uint32_t words, const uint32_t* tile_cnt, uint32_t tiles,
                                                                uint32_t* rows, uint32_t max_rows) {
    __shared__ uint32_t lds[CK_THREADS];
    const uint32_t off = tile_cnt[(size_t)blockIdx.y * (tiles + 1) + blockIdx.x];
    if (off >= max_rows) return;  // the whole workgroup: the lowest max_rows rows lie in earlier tiles
    const uint32_t w = blockIdx.x * CK_THREADS + threadIdx.x;
    uint64_t bits = w < words ? mask[(size_t)blockIdx.y * words + w] : 0ull;
    uint32_t total;
    uint32_t at = off + lk_scan_excl((uint32_t)__popcll(bits), lds, &total);
    uint32_t* out = rows + (size_t)blockIdx.y * max_rows;
    while (bits && at < max_rows) {
        out[at++] = w * 64u + (uint32_t)(__ffsll((unsigned long long)bits) - 1);
        bits &= bits - 1;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// One call's share of check_ws: the mask, the tile counts, the counts and the row lists (what the tail reads and writes), the flag, and
// `extra` bytes for the check's own tables and buffers.
struct CkWs {
    uint32_t words = 0, tiles = 0;
    uint64_t* mask = nullptr;
    uint32_t* tile_cnt = nullptr;
    uint64_t* counts = nullptr;
    uint32_t* rows = nullptr;
    uint32_t* flag = nullptr;
    char* extra = nullptr;
};

static int ck_prepare(Ctx* c, uint32_t k, size_t items, uint32_t max_rows, size_t extra, hipStream_t s, CkWs* w) {
    const uint64_t n = 1ull << k;
    w->words = (uint32_t)(n < 64 ? 1 : n / 64);
    w->tiles = (w->words + CK_THREADS - 1) / CK_THREADS;
    const size_t rows_bytes = items * (size_t)max_rows * sizeof(uint32_t);
    Carve ws;
    const size_t o_mask = ws.take(items * w->words * sizeof(uint64_t)), o_cnt = ws.take(items * ((size_t)w->tiles + 1) * sizeof(uint32_t)),
                 o_counts = ws.take(items * sizeof(uint64_t)), o_rows = ws.take(rows_bytes), o_flag = ws.take(256), o_extra = ws.take(extra);
    int rc = c->check_ws.ensure(ws.total);
    if (rc) return rc;
    char* base = (char*)c->check_ws.p;
    w->mask = (uint64_t*)(base + o_mask);
    w->tile_cnt = (uint32_t*)(base + o_cnt);
    w->counts = (uint64_t*)(base + o_counts);
    w->rows = (uint32_t*)(base + o_rows);
    w->flag = (uint32_t*)(base + o_flag);
    w->extra = base + o_extra;
    H2_CHECK(hipMemsetAsync(w->flag, 0, 256, s));
    if (rows_bytes) H2_CHECK(hipMemsetAsync(w->rows, 0xff, rows_bytes, s));
    return 0;
}

// the tail's kernels ...
static int ck_tail(const CkWs& w, size_t items, uint32_t max_rows, hipStream_t s) {
    const dim3 grid(w.tiles, (uint32_t)items), block(CK_THREADS);
    hipLaunchKernelGGL(ck_count_kernel, grid, block, 0, s, w.mask, w.words, w.tile_cnt, w.tiles);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ck_scan_kernel, dim3((uint32_t)items), block, 0, s, w.tile_cnt, w.tiles, w.counts);
    H2_CHECK(hipGetLastError());
    if (max_rows) {
        hipLaunchKernelGGL(ck_compact_kernel, grid, block, 0, s, w.mask, w.words, w.tile_cnt, w.tiles, w.rows, max_rows);
        H2_CHECK(hipGetLastError());
    }
    return 0;
}
// ... then counts and rows to the caller's memory: the copies are the workspace's last readers
static int ck_deliver(const CkWs& w, size_t items, uint32_t max_rows, uint64_t* counts, uint32_t* rows, hipStream_t s) {
    H2_CHECK(hipMemcpyAsync(counts, w.counts, items * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (max_rows) H2_CHECK(hipMemcpyAsync(rows, w.rows, items * (size_t)max_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return 0;
}

// Validated arguments, device columns.  Waits for s once.
static int check_gates_device(Ctx* c, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice, uint32_t n_advice,
                              const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                              const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, uint64_t* counts, uint32_t* rows, hipStream_t s) {
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    CkWs w;
    if ((rc = ck_prepare(c, k, n_graphs, max_rows, 0, s, &w))) return rc;
    int tm = c->timer_begin("check_gates", s);
    if ((rc = check_gates_enqueue(c, k, fixed, n_fixed, advice, n_advice, instance, n_instance, challenges, n_challenges, graphs, n_graphs, w.mask,
                                  w.words, s)))
        return rc;
    if ((rc = ck_tail(w, n_graphs, max_rows, s))) return rc;
    c->timer_end(tm, s);
    if ((rc = ck_deliver(w, n_graphs, max_rows, counts, rows, s))) return rc;
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}

// maps[j]: 2^k (column, row) pairs, device memory.  Waits for s once; H2HIP_EINVAL when the kernel met a pair out of range.
static int check_permutation_device(Ctx* c, uint32_t k, const Fe* const* cols, const uint32_t* const* maps, uint32_t m, uint32_t max_rows,
                                    uint64_t* counts, uint32_t* rows, hipStream_t s) {
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    CkWs w;
    if ((rc = ck_prepare(c, k, m, max_rows, 2 * (size_t)m * sizeof(void*), s, &w))) return rc;
    if ((rc = c->check_flag.ensure(sizeof(uint32_t)))) return rc;
    std::vector<const void*> blob(2 * (size_t)m);
    for (uint32_t j = 0; j < m; j++) {
        blob[j] = cols[j];
        blob[m + j] = maps[j];
    }
    if ((rc = c->stage_h2d(w.extra, blob.data(), blob.size() * sizeof(void*), s))) return rc;
    const uint64_t n = 1ull << k;
    int tm = c->timer_begin("check_permutation", s);
    hipLaunchKernelGGL(ck_perm_kernel, dim3((uint32_t)((n + CK_THREADS - 1) / CK_THREADS), m), dim3(CK_THREADS), 0, s, (const Fe* const*)w.extra,
                       (const uint2* const*)(w.extra + m * sizeof(void*)), w.mask, w.words, k, m, w.flag);
    H2_CHECK(hipGetLastError());
    if ((rc = ck_tail(w, m, max_rows, s))) return rc;
    c->timer_end(tm, s);
    H2_CHECK(hipMemcpyAsync(c->check_flag.p, w.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = ck_deliver(w, m, max_rows, counts, rows, s))) return rc;
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    if (*(const uint32_t*)c->check_flag.p) {
        set_error("check_permutation: a mapping pair has column >= n_columns or row >= 2^k; it was not followed, counts and rows are unspecified");
        return H2HIP_EINVAL;
    }
    return 0;
}

static int check_lookups_device(Ctx* c, uint32_t k, const Fe* const* in, const Fe* const* tab, size_t count, uint32_t bf, uint32_t max_rows,
                                uint64_t* counts, uint32_t* rows, hipStream_t s) {
    const uint64_t n = 1ull << k, u = n - bf - 1;
    const size_t col_bytes = n * sizeof(Fe);
    // the check's own share: four pointer tables (inputs, tables, key buffers 0 and 1), then two key buffers per lookup
    Carve ex;
    const size_t o_ptr = ex.take(4 * count * sizeof(void*)), o_keys = ex.take_packed(2 * count * col_bytes);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    CkWs w;
    if ((rc = ck_prepare(c, k, count, max_rows, ex.total, s, &w))) return rc;
    Fe* keys = (Fe*)(w.extra + o_keys);
    std::vector<const void*> blob(4 * count);
    for (size_t j = 0; j < count; j++) {
        blob[j] = in[j];
        blob[count + j] = tab[j];
        blob[2 * count + j] = keys + j * n;
        blob[3 * count + j] = keys + (count + j) * n;
    }
    if ((rc = c->stage_h2d(w.extra + o_ptr, blob.data(), blob.size() * sizeof(void*), s))) return rc;
    const Fe* const* d_in = (const Fe* const*)(w.extra + o_ptr);
    const Fe* const* d_tab = d_in + count;
    Fe* const* d_k0 = (Fe* const*)(d_in + 2 * count);
    Fe* const* d_k1 = (Fe* const*)(d_in + 3 * count);
    int tm = c->timer_begin("check_lookups", s);
    if ((rc = lookup_sort_enqueue(d_tab, d_k0, d_k1, (uint32_t)count, k, u, s))) return rc;
    const Fe* const* d_sorted = lookup_sort_passes(k) & 1 ? (const Fe* const*)d_k1 : (const Fe* const*)d_k0;
    hipLaunchKernelGGL(ck_lookup_kernel, dim3((uint32_t)((n + CK_THREADS - 1) / CK_THREADS), (uint32_t)count), dim3(CK_THREADS), 0, s, d_in,
                       d_sorted, w.mask, w.words, k, u);
    H2_CHECK(hipGetLastError());
    if ((rc = ck_tail(w, count, max_rows, s))) return rc;
    c->timer_end(tm, s);
    if ((rc = ck_deliver(w, count, max_rows, counts, rows, s))) return rc;
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}

// Both columns of every shuffle go through the lookup sort in one batch (2 count columns), then one multiplicity test per input row.
static int check_shuffles_device(Ctx* c, uint32_t k, const Fe* const* in, const Fe* const* sh, size_t count, uint32_t bf, uint32_t max_rows,
                                 uint64_t* counts, uint32_t* rows, hipStream_t s) {
    const uint64_t n = 1ull << k, u = n - bf - 1;
    const size_t col_bytes = n * sizeof(Fe), cols = 2 * count;
    // the check's own share: three pointer tables of 2 count entries (sources: inputs then shuffles; key buffers 0 and 1), then the buffers
    Carve ex;
    const size_t o_ptr = ex.take(3 * cols * sizeof(void*)), o_keys = ex.take_packed(2 * cols * col_bytes);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    CkWs w;
    if ((rc = ck_prepare(c, k, count, max_rows, ex.total, s, &w))) return rc;
    Fe* keys = (Fe*)(w.extra + o_keys);
    std::vector<const void*> blob(3 * cols);
    for (size_t j = 0; j < count; j++) {
        blob[j] = in[j];
        blob[count + j] = sh[j];
    }
    for (size_t q = 0; q < cols; q++) {
        blob[cols + q] = keys + q * n;
        blob[2 * cols + q] = keys + (cols + q) * n;
    }
    if ((rc = c->stage_h2d(w.extra + o_ptr, blob.data(), blob.size() * sizeof(void*), s))) return rc;
    const Fe* const* d_src = (const Fe* const*)(w.extra + o_ptr);
    Fe* const* d_k0 = (Fe* const*)(d_src + cols);
    Fe* const* d_k1 = (Fe* const*)(d_src + 2 * cols);
    int tm = c->timer_begin("check_shuffles", s);
    if ((rc = lookup_sort_enqueue(d_src, d_k0, d_k1, (uint32_t)cols, k, u, s))) return rc;
    const Fe* const* d_sorted = lookup_sort_passes(k) & 1 ? (const Fe* const*)d_k1 : (const Fe* const*)d_k0;
    hipLaunchKernelGGL(ck_shuffle_kernel, dim3((uint32_t)((n + CK_THREADS - 1) / CK_THREADS), (uint32_t)count), dim3(CK_THREADS), 0, s, d_src,
                       d_sorted, d_sorted + count, w.mask, w.words, k, u);
    H2_CHECK(hipGetLastError());
    if ((rc = ck_tail(w, count, max_rows, s))) return rc;
    c->timer_end(tm, s);
    if ((rc = ck_deliver(w, count, max_rows, counts, rows, s))) return rc;
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "witness check") --------------------------------------------------------------------------------------
static int ck_out_check(const char* what, uint32_t k, size_t items, uint32_t max_rows, const uint64_t* counts, const uint32_t* rows) {
    if (int rc = check_k(what, k)) return rc;
    if (max_rows > CK_MAX_ROWS) {
        set_error("%s: max_rows %u > %d", what, max_rows, CK_MAX_ROWS);
        return H2HIP_EINVAL;
    }
    if (items && !counts) {
        set_error("%s: null counts", what);
        return H2HIP_EINVAL;
    }
    if (items && max_rows && !rows) {
        set_error("%s: null rows with max_rows = %u", what, max_rows);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int ck_gates_check(uint32_t k, const void* const* fixed, uint32_t n_fixed, const void* const* advice, uint32_t n_advice,
                          const void* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                          const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, const uint64_t* counts, const uint32_t* rows) {
    const char* what = "check_gates";
    if (n_graphs > CK_MAX_ITEMS) {
        set_error("%s: %zu graphs > %d", what, n_graphs, CK_MAX_ITEMS);
        return H2HIP_EINVAL;
    }
    if (int rc = ck_out_check(what, k, n_graphs, max_rows, counts, rows)) return rc;
    if (check_frs(what, challenges, n_challenges, "challenge")) return H2HIP_EINVAL;
    if (check_ptrs(what, fixed, n_fixed, "fixed_values") || check_ptrs(what, advice, n_advice, "advice_values") ||
        check_ptrs(what, instance, n_instance, "instance_values"))
        return H2HIP_EINVAL;
    return check_gates_validate(n_fixed, n_advice, n_instance, n_challenges, graphs, n_graphs);
}

int h2hip_check_gates_bn254_device(uint32_t k, const void* const* d_fixed_values, uint32_t n_fixed, const void* const* d_advice_values,
                                   uint32_t n_advice, const void* const* d_instance_values, uint32_t n_instance, const uint64_t* challenges,
                                   uint32_t n_challenges, const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, uint64_t* counts,
                                   uint32_t* rows, void* stream) {
    if (int rc = ck_gates_check(k, d_fixed_values, n_fixed, d_advice_values, n_advice, d_instance_values, n_instance, challenges, n_challenges,
                                graphs, n_graphs, max_rows, counts, rows))
        return rc;
    if (n_graphs == 0) return 0;
    Entry en("h2hip_check_gates_bn254_device", n_advice ? d_advice_values[0] : n_fixed ? d_fixed_values[0] : n_instance ? d_instance_values[0] : nullptr);
    if (en.rc) return en.rc;
    return check_gates_device(en.c, k, (const Fe* const*)d_fixed_values, n_fixed, (const Fe* const*)d_advice_values, n_advice,
                              (const Fe* const*)d_instance_values, n_instance, challenges, n_challenges, graphs, n_graphs, max_rows, counts, rows,
                              (hipStream_t)stream);
}

int h2hip_check_gates_bn254(uint32_t k, const uint64_t* const* fixed_values, uint32_t n_fixed, const uint64_t* const* advice_values,
                            uint32_t n_advice, const uint64_t* const* instance_values, uint32_t n_instance, const uint64_t* challenges,
                            uint32_t n_challenges, const h2hip_graph* graphs, size_t n_graphs, uint32_t max_rows, uint64_t* counts, uint32_t* rows) {
    if (int rc = ck_gates_check(k, (const void* const*)fixed_values, n_fixed, (const void* const*)advice_values, n_advice,
                                (const void* const*)instance_values, n_instance, challenges, n_challenges, graphs, n_graphs, max_rows, counts, rows))
        return rc;
    if (n_graphs == 0) return 0;
    Entry en("h2hip_check_gates_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    std::vector<const Fe*> d_fixed(n_fixed), d_advice(n_advice), d_instance(n_instance);
    const size_t bytes = sizeof(Fe) << k;
    HostIo io(c, c->host_io, c->stream);  // the host forms' columns: one pinned with h2hip_columns_pin is read where it lies
    for (uint32_t j = 0; j < n_fixed; j++) io.in(fixed_values[j], bytes, &d_fixed[j], true);
    for (uint32_t j = 0; j < n_advice; j++) io.in(advice_values[j], bytes, &d_advice[j], true);
    for (uint32_t j = 0; j < n_instance; j++) io.in(instance_values[j], bytes, &d_instance[j], true);
    if (int rc = io.upload()) return rc;
    if (int rc = check_gates_device(c, k, d_fixed.data(), n_fixed, d_advice.data(), n_advice, d_instance.data(), n_instance, challenges,
                                    n_challenges, graphs, n_graphs, max_rows, counts, rows, c->stream))
        return rc;
    return io.finish();
}

static int ck_perm_check(uint32_t k, const void* const* columns, const void* const* mapping, uint32_t m, uint32_t max_rows, const uint64_t* counts,
                         const uint32_t* rows) {
    const char* what = "check_permutation";
    if (m > CK_MAX_ITEMS) {
        set_error("%s: n_columns %u > %d", what, m, CK_MAX_ITEMS);
        return H2HIP_EINVAL;
    }
    if (int rc = ck_out_check(what, k, m, max_rows, counts, rows)) return rc;
    if (check_ptrs(what, columns, m, "columns") || check_ptrs(what, mapping, m, "mapping")) return H2HIP_EINVAL;
    return 0;
}

int h2hip_check_permutation_bn254_device(uint32_t k, const void* const* d_columns, const void* const* d_mapping, uint32_t n_columns,
                                         uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream) {
    if (int rc = ck_perm_check(k, d_columns, d_mapping, n_columns, max_rows, counts, rows)) return rc;
    if (n_columns == 0) return 0;
    Entry en("h2hip_check_permutation_bn254_device", d_columns[0]);
    if (en.rc) return en.rc;
    return check_permutation_device(en.c, k, (const Fe* const*)d_columns, (const uint32_t* const*)d_mapping, n_columns, max_rows, counts, rows,
                                    (hipStream_t)stream);
}

int h2hip_check_permutation_bn254(uint32_t k, const uint64_t* const* columns, const uint32_t* const* mapping, uint32_t n_columns, uint32_t max_rows,
                                  uint64_t* counts, uint32_t* rows) {
    if (int rc = ck_perm_check(k, (const void* const*)columns, (const void* const*)mapping, n_columns, max_rows, counts, rows)) return rc;
    const size_t n = (size_t)1 << k;
    for (uint32_t j = 0; j < n_columns; j++)  // the mapping is host memory: a bad pair answers the same with and without a GPU
        for (size_t i = 0; i < n; i++)
            if (mapping[j][2 * i] >= n_columns || mapping[j][2 * i + 1] >= n) {
                set_error("check_permutation: mapping[%u][%zu] = (%u, %u) is out of range (n_columns = %u, 2^k = %zu)", j, i, mapping[j][2 * i],
                          mapping[j][2 * i + 1], n_columns, n);
                return H2HIP_EINVAL;
            }
    if (n_columns == 0) return 0;
    Entry en("h2hip_check_permutation_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    std::vector<const Fe*> d_cols(n_columns);
    std::vector<const uint32_t*> d_maps(n_columns);
    HostIo io(c, c->host_io, s);
    for (uint32_t j = 0; j < n_columns; j++) io.in(columns[j], n * sizeof(Fe), &d_cols[j], true);
    for (uint32_t j = 0; j < n_columns; j++) io.in(mapping[j], n * 8, &d_maps[j]);  // the mapping follows the columns
    if (int rc = io.upload()) return rc;
    if (int rc = check_permutation_device(c, k, d_cols.data(), d_maps.data(), n_columns, max_rows, counts, rows, s)) return rc;
    return io.finish();
}

static int ck_lookups_check(uint32_t k, const void* const* in, const void* const* tab, size_t count, uint32_t bf, uint32_t max_rows,
                            const uint64_t* counts, const uint32_t* rows) {
    const char* what = "check_lookups";
    if (int rc = check_k_blinding(what, k, bf)) return rc;
    if (count > CK_MAX_LOOKUPS) {
        set_error("%s: count %zu > %d", what, count, CK_MAX_LOOKUPS);
        return H2HIP_EINVAL;
    }
    if (int rc = ck_out_check(what, k, count, max_rows, counts, rows)) return rc;
    if (check_ptrs(what, in, count, "compressed_input") || check_ptrs(what, tab, count, "compressed_table")) return H2HIP_EINVAL;
    return 0;
}

int h2hip_check_lookups_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_table, size_t count,
                                     uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream) {
    if (int rc = ck_lookups_check(k, d_compressed_input, d_compressed_table, count, blinding_factors, max_rows, counts, rows)) return rc;
    if (count == 0) return 0;
    Entry en("h2hip_check_lookups_bn254_device", d_compressed_input[0]);
    if (en.rc) return en.rc;
    return check_lookups_device(en.c, k, (const Fe* const*)d_compressed_input, (const Fe* const*)d_compressed_table, count, blinding_factors,
                                max_rows, counts, rows, (hipStream_t)stream);
}

int h2hip_check_lookups_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_table, size_t count,
                              uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows) {
    if (int rc = ck_lookups_check(k, (const void* const*)compressed_input, (const void* const*)compressed_table, count, blinding_factors, max_rows,
                                  counts, rows))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_check_lookups_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    std::vector<const Fe*> d_in(count), d_tab(count);
    HostIo io(c, c->host_io, c->stream);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_input[j], sizeof(Fe) << k, &d_in[j], true);
        io.in(compressed_table[j], sizeof(Fe) << k, &d_tab[j], true);
    }
    if (int rc = io.upload()) return rc;
    if (int rc = check_lookups_device(c, k, d_in.data(), d_tab.data(), count, blinding_factors, max_rows, counts, rows, c->stream)) return rc;
    return io.finish();
}

static int ck_shuffles_check(uint32_t k, const void* const* in, const void* const* sh, size_t count, uint32_t bf, uint32_t max_rows,
                             const uint64_t* counts, const uint32_t* rows) {
    const char* what = "check_shuffles";
    if (int rc = check_k_blinding(what, k, bf)) return rc;
    if (count > CK_MAX_LOOKUPS) {
        set_error("%s: count %zu > %d", what, count, CK_MAX_LOOKUPS);
        return H2HIP_EINVAL;
    }
    if (int rc = ck_out_check(what, k, count, max_rows, counts, rows)) return rc;
    if (check_ptrs(what, in, count, "compressed_input") || check_ptrs(what, sh, count, "compressed_shuffle")) return H2HIP_EINVAL;
    return 0;
}

int h2hip_check_shuffles_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_shuffle, size_t count,
                                      uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows, void* stream) {
    if (int rc = ck_shuffles_check(k, d_compressed_input, d_compressed_shuffle, count, blinding_factors, max_rows, counts, rows)) return rc;
    if (count == 0) return 0;
    Entry en("h2hip_check_shuffles_bn254_device", d_compressed_input[0]);
    if (en.rc) return en.rc;
    return check_shuffles_device(en.c, k, (const Fe* const*)d_compressed_input, (const Fe* const*)d_compressed_shuffle, count, blinding_factors,
                                 max_rows, counts, rows, (hipStream_t)stream);
}

int h2hip_check_shuffles_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_shuffle, size_t count,
                               uint32_t blinding_factors, uint32_t max_rows, uint64_t* counts, uint32_t* rows) {
    if (int rc = ck_shuffles_check(k, (const void* const*)compressed_input, (const void* const*)compressed_shuffle, count, blinding_factors,
                                   max_rows, counts, rows))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_check_shuffles_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    std::vector<const Fe*> d_in(count), d_sh(count);
    HostIo io(c, c->host_io, c->stream);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_input[j], sizeof(Fe) << k, &d_in[j], true);
        io.in(compressed_shuffle[j], sizeof(Fe) << k, &d_sh[j], true);
    }
    if (int rc = io.upload()) return rc;
    if (int rc = check_shuffles_device(c, k, d_in.data(), d_sh.data(), count, blinding_factors, max_rows, counts, rows, c->stream)) return rc;
    return io.finish();
}

}  // extern "C"
