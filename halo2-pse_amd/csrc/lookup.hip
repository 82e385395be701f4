// lookup.hip -- lookup::Argument::commit_permuted (plonk/lookup/prover.rs:64-170) on the GPU: the permuted input A' and the permuted
// table S' of every lookup, from the compressed input and table columns (the compression itself runs on evaluate_h's interpreter,
// evalh.hip lookup_compress_device).
//
// The reference (permute_expression_pair, :391-475), with n = 2^k, b = blinding_factors and u = n - b - 1:
//   A'[0 .. u) = C_in[0 .. u) sorted by Fr's Ord -- the order of the canonical integers (halo2curves' to_repr compared from the top);
//   S'[i] = A'[i] on every first row (i = 0 or A'[i] != A'[i-1]), each taking one copy of its value out of the table multiset
//   T = C_tab[0 .. u); the leftovers L (ascending) go to the repeated rows R (ascending) as S'[R[j]] = L[|L| - 1 - j]
//   (repeated_input_rows.pop() while the BTreeMap is walked upwards); rows u .. n - 1 of both are the caller's blinding values.
//   An input value missing from T is Error::ConstraintSystemFailure, here H2HIP_ELOOKUP.
//
// Plan (Lookup permutation).  Keys are the canonical 256-bit values (one Montgomery reduction per element on the way
// in, one multiplication by R^2 on the way out).  Every input and table column of a call is sorted by the same launches:
//   1. lk_block_sort_kernel  (tiles x columns): blocks of up to LK_TILE keys sorted in LDS by a bitonic network over full 256-bit
//                            compares; rows u .. n - 1 enter as all-ones keys, above every canonical value, and stay at the end;
//   2. lk_merge_kernel       (tiles x columns, log2(n / block) launches): merge path -- every workgroup finds the split of its
//                            output range in the two runs by a binary search, stages both slices in LDS and merges them there.
// A comparison sort is exact for every key distribution (one repeated value, 16-bit keys, keys sharing their high or low bits)
// with a launch count fixed by n alone, so no pass waits on a count the host has to read back.  Then per lookup:
//   3. lk_mark_kernel        first rows; each one's value found in the sorted table (galloping search from the thread's previous
//                            hit), that slot marked used, or the lookup's not-found flag raised;
//   4. lk_count_kernel       per tile: unused table slots (L) and repeated rows (R);
//   5. lk_scan_kernel        one workgroup per lookup: exclusive scans of the tile counts (reduce-then-scan, no workgroup waits
//                            on another);
//   6. lk_compact_kernel     L compacted in ascending order;
//   7. lk_final_kernel       A', S'[first] = A'[first], S'[R[j]] = L[|L| - 1 - j], the blinding rows, back to Montgomery form.
// The host reads the not-found flags once, after the last kernel.  No kernel uses scratch (profiles/lookup_resources.txt).
// The sort also serves the logUp (mv-lookup) argument's multiplicity column, in a variant that carries each key's row (further down).
#include <string.h>
#include <vector>
#include "engine.h"
#include "fe_io.h"
#include "lk_dev.h"

namespace h2 {

#define LK_TILE 1024                  // keys one workgroup sorts, merges or permutes (32 KB of LDS)
#define LK_E (LK_TILE / LK_THREADS)   // consecutive keys / rows per thread
#define LK_MAX_COUNT 32767            // lookups per call: 2 count sorted columns in grid.y

static uint32_t g_lk_last[2] = {0, 0};     // block keys and merge passes of the last sort (a permute or a lookup-check call)

// merge path: how many of the first d outputs of merge(A[0 .. na), B[0 .. nb)) come from A (on ties A first)
__device__ __forceinline__ uint32_t lk_split(const Fe* A, uint32_t na, const Fe* B, uint32_t nb, uint32_t d) {
    uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (!key_lt(fe_ld(B, d - 1 - mid), fe_ld(A, mid))) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- 1. canonical keys, blocks of `block` keys sorted in LDS --------------------------------------------------------------------
// ts = min(LK_TILE, n) keys per workgroup; block <= ts, both powers of two.  ROWS: every key carries its row as a ninth word, the
// tie-break of equal keys (the mv-lookup multiplicities: a lower bound in the sorted table then lands on the lowest row of a run);
// rdst[q] receives the rows.  The key-only instantiation compiles to what it was before the template (profiles/lookup_resources.txt).
template <bool ROWS>
__device__ __forceinline__ bool lk_pair_lt(const Fe& a, uint32_t ra, const Fe& b, uint32_t rb) {
    if (!ROWS) return key_lt(a, b);
    return key_lt(a, b) || (ra < rb && !key_lt(b, a));
}
template <bool ROWS>
__global__ __launch_bounds__(LK_THREADS) void lk_block_sort_kernel(const Fe* const* src, Fe* const* dst, uint32_t* const* rdst, uint64_t u,
                                                                   uint32_t ts, uint32_t block) {
    __shared__ Fe sk[LK_TILE];
    __shared__ uint32_t sr[ROWS ? LK_TILE : 1];
    const Fe* in = src[blockIdx.y];
    Fe* out = dst[blockIdx.y];
    const uint64_t base = (uint64_t)blockIdx.x * ts;
    for (uint32_t i = threadIdx.x; i < ts; i += LK_THREADS) {
        const uint64_t r = base + i;
        Fe v;
        if (r < u) {
            v = fe_to_canonical<FrP>(fe_ld(in, r));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) v.l[j] = 0xffffffffu;
        }
        sk[i] = v;
        if (ROWS) sr[i] = (uint32_t)r;
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= block; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < ts / 2; t += LK_THREADS) {
                const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;  // the pair (i, i + j), bit j of i clear
                const bool asc = kk == block || (i & kk) == 0;         // the last stage sorts every block ascending
                const Fe a = sk[i], b = sk[l];
                const uint32_t ra = ROWS ? sr[i] : 0u, rb = ROWS ? sr[l] : 0u;
                if (lk_pair_lt<ROWS>(b, rb, a, ra) == asc) {
                    sk[i] = b;
                    sk[l] = a;
                    if (ROWS) {
                        sr[i] = rb;
                        sr[l] = ra;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < ts; i += LK_THREADS) fe_st(out, base + i, sk[i]);
    if (ROWS) {
        uint32_t* rout = rdst[blockIdx.y];
        for (uint32_t i = threadIdx.x; i < ts; i += LK_THREADS) rout[base + i] = sr[i];
    }
}

// ---- 2. one merge pass: sorted runs of w keys -> runs of 2w ---------------------------------------------------------------------
// ROWS: the rows travel with their keys (rsrc[q] -> rdst[q]).  The merge takes run A first on ties and every row of A is below every
// row of B (runs are consecutive row ranges), so equal keys stay in row order without a compare of the rows.
template <bool ROWS>
__global__ __launch_bounds__(LK_THREADS) void lk_merge_kernel(const Fe* const* src, Fe* const* dst, const uint32_t* const* rsrc,
                                                              uint32_t* const* rdst, uint32_t w, uint32_t ts) {
    __shared__ Fe sk[LK_TILE];
    __shared__ uint32_t sr[ROWS ? LK_TILE : 1];
    __shared__ uint32_t s_a[2];
    const Fe* in = src[blockIdx.y];
    Fe* out = dst[blockIdx.y];
    const uint32_t* rin = ROWS ? rsrc[blockIdx.y] : nullptr;
    uint32_t* rout = ROWS ? rdst[blockIdx.y] : nullptr;
    const uint64_t o0 = (uint64_t)blockIdx.x * ts;
    const uint32_t tid = threadIdx.x, t = tid * LK_E;
    const Fe *A, *B;
    uint32_t na, nb, d;
    if (2ull * w >= ts) {  // the tile lies in one pair of runs: its slices of both, found by merge path on global memory
        const uint64_t pbase = o0 / (2ull * w) * (2ull * w);
        const Fe* gA = in + pbase;
        const Fe* gB = gA + w;
        const uint32_t d0 = (uint32_t)(o0 - pbase);
        if (tid < 2) s_a[tid] = lk_split(gA, w, gB, w, d0 + tid * ts);
        __syncthreads();
        const uint32_t a0 = s_a[0], a1 = s_a[1], b0 = d0 - a0;
        na = a1 - a0;
        nb = ts - na;
        for (uint32_t i = tid; i < ts; i += LK_THREADS) sk[i] = i < na ? fe_ld(gA, a0 + i) : fe_ld(gB, b0 + (i - na));
        if (ROWS)
            for (uint32_t i = tid; i < ts; i += LK_THREADS) sr[i] = i < na ? rin[pbase + a0 + i] : rin[pbase + w + b0 + (i - na)];
        __syncthreads();
        A = sk;
        B = sk + na;
        d = t;
    } else {  // whole pairs of runs inside the tile
        for (uint32_t i = tid; i < ts; i += LK_THREADS) sk[i] = fe_ld(in, o0 + i);
        if (ROWS)
            for (uint32_t i = tid; i < ts; i += LK_THREADS) sr[i] = rin[o0 + i];
        __syncthreads();
        const uint32_t pb = t / (2 * w) * (2 * w);
        A = sk + pb;
        B = A + w;
        na = nb = w;
        d = t - pb;
    }
    if (t >= ts) return;
    uint32_t ia = lk_split(A, na, B, nb, d), ib = d - ia;
#pragma unroll
    for (int e = 0; e < LK_E; e++) {  // LK_E <= 2w: a thread's outputs lie in one pair
        const bool take_a = ib >= nb || (ia < na && !key_lt(B[ib], A[ia]));
        const Fe x = take_a ? A[ia] : B[ib];
        if (ROWS) rout[o0 + t + e] = sr[(take_a ? A + ia : B + ib) - sk];
        if (take_a) ia++;
        else ib++;
        fe_st(out, o0 + t + e, x);
    }
}

// ---- 3.-7. the permutation ------------------------------------------------------------------------------------------------------
struct LkPerm {           // one lookup
    const Fe* a;          // sorted canonical input keys (A'), all-ones from row u on
    const Fe* t;          // sorted canonical table keys
    uint32_t* used;       // table slots taken by a first row
    Fe* lc;               // the leftovers L, compacted
    uint32_t* cnt_l;      // per-tile counts of L, then their exclusive scan; [tiles] = |L|
    uint32_t* cnt_r;      // the same for the repeated rows R
    uint32_t* flag;       // an input value is not in the table
    Fe* pa;               // outputs, Montgomery form
    Fe* pt;
    const Fe* blind;      // 2 (b + 1) values: A' rows u .. n - 1, then S' rows u .. n - 1
};

__device__ __forceinline__ bool lk_repeated(const Fe* a, uint64_t i) { return i > 0 && fe_eq(fe_ld(a, i), fe_ld(a, i - 1)); }

__global__ __launch_bounds__(LK_THREADS) void lk_mark_kernel(const LkPerm* P, uint64_t u) {
    const LkPerm D = P[blockIdx.y];
    const uint64_t r0 = ((uint64_t)blockIdx.x * LK_THREADS + threadIdx.x) * LK_E;
    uint64_t pos = 0;
    bool have = false;
    for (int e = 0; e < LK_E; e++) {
        const uint64_t i = r0 + e;
        if (i >= u) break;
        if (lk_repeated(D.a, i)) continue;
        const Fe v = fe_ld(D.a, i);
        // lower bound of v in T[0 .. u): every T[< lo] < v; galloping from the previous hit, whose value is smaller
        uint64_t lo = have ? pos : 0, hi = u;
        if (have) {
            uint64_t step = 1;
            hi = lo;
            while (hi < u && key_lt(fe_ld(D.t, hi), v)) {
                lo = hi + 1;
                hi = lo + step;
                step <<= 1;
            }
            if (hi > u) hi = u;
        }
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key_lt(fe_ld(D.t, mid), v)) lo = mid + 1;
            else hi = mid;
        }
        pos = lo;
        have = true;
        if (pos >= u || !fe_eq(fe_ld(D.t, pos), v)) atomicOr(D.flag, 1u);
        else D.used[pos] = 1u;  // distinct first values land on distinct slots
    }
}

__device__ __forceinline__ void lk_local_counts(const LkPerm& D, uint64_t r0, uint64_t u, uint32_t* nl, uint32_t* nr) {
    uint32_t l = 0, r = 0;
    for (int e = 0; e < LK_E; e++) {
        const uint64_t i = r0 + e;
        if (i >= u) break;
        l += D.used[i] == 0u;
        r += lk_repeated(D.a, i);
    }
    *nl = l;
    *nr = r;
}

__global__ __launch_bounds__(LK_THREADS) void lk_count_kernel(const LkPerm* P, uint64_t u) {
    __shared__ uint32_t lds[LK_THREADS];
    const LkPerm D = P[blockIdx.y];
    const uint64_t r0 = ((uint64_t)blockIdx.x * LK_THREADS + threadIdx.x) * LK_E;
    uint32_t nl, nr, tl, tr;
    lk_local_counts(D, r0, u, &nl, &nr);
    (void)lk_scan_excl(nl, lds, &tl);
    (void)lk_scan_excl(nr, lds, &tr);
    if (threadIdx.x == 0) {
        D.cnt_l[blockIdx.x] = tl;
        D.cnt_r[blockIdx.x] = tr;
    }
}

__global__ __launch_bounds__(LK_THREADS) void lk_scan_kernel(const LkPerm* P, uint32_t tiles) {
    __shared__ uint32_t lds[LK_THREADS];
    const LkPerm D = P[blockIdx.x];
    uint32_t carry_l = 0, carry_r = 0;
    for (uint32_t base = 0; base < tiles; base += LK_THREADS) {
        const uint32_t j = base + threadIdx.x;
        uint32_t tl, tr;
        const uint32_t el = lk_scan_excl(j < tiles ? D.cnt_l[j] : 0u, lds, &tl);
        const uint32_t er = lk_scan_excl(j < tiles ? D.cnt_r[j] : 0u, lds, &tr);
        if (j < tiles) {
            D.cnt_l[j] = carry_l + el;
            D.cnt_r[j] = carry_r + er;
        }
        carry_l += tl;
        carry_r += tr;
    }
    if (threadIdx.x == 0) {
        D.cnt_l[tiles] = carry_l;
        D.cnt_r[tiles] = carry_r;
    }
}

__global__ __launch_bounds__(LK_THREADS) void lk_compact_kernel(const LkPerm* P, uint64_t u) {
    __shared__ uint32_t lds[LK_THREADS];
    const LkPerm D = P[blockIdx.y];
    const uint64_t r0 = ((uint64_t)blockIdx.x * LK_THREADS + threadIdx.x) * LK_E;
    uint32_t nl = 0, tot;
    for (int e = 0; e < LK_E; e++)
        if (r0 + e < u) nl += D.used[r0 + e] == 0u;
    uint32_t at = D.cnt_l[blockIdx.x] + lk_scan_excl(nl, lds, &tot);
    for (int e = 0; e < LK_E; e++) {
        const uint64_t i = r0 + e;
        if (i >= u) break;
        if (D.used[i] == 0u) fe_st(D.lc, at++, fe_ld(D.t, i));
    }
}

__global__ __launch_bounds__(LK_THREADS) void lk_final_kernel(const LkPerm* P, uint64_t u, uint64_t n, uint32_t tiles) {
    __shared__ uint32_t lds[LK_THREADS];
    const LkPerm D = P[blockIdx.y];
    const uint64_t r0 = ((uint64_t)blockIdx.x * LK_THREADS + threadIdx.x) * LK_E;
    uint32_t nr = 0, tot;
    for (int e = 0; e < LK_E; e++)
        if (r0 + e < u) nr += lk_repeated(D.a, r0 + e);
    uint32_t rank = D.cnt_r[blockIdx.x] + lk_scan_excl(nr, lds, &tot);  // repeated rows before this thread's first row
    const uint32_t n_l = D.cnt_l[tiles];                                // |L| (>= |R|; equal unless a value was missing)
    for (int e = 0; e < LK_E; e++) {
        const uint64_t i = r0 + e;
        if (i >= n) break;
        if (i >= u) {
            fe_st(D.pa, i, D.blind[i - u]);
            fe_st(D.pt, i, D.blind[(n - u) + (i - u)]);
            continue;
        }
        const Fe v = fe_ld(D.a, i);
        Fe s = v;
        if (lk_repeated(D.a, i)) {
            if (rank < n_l) s = fe_ld(D.lc, n_l - 1 - rank);
            rank++;
        }
        fe_st(D.pa, i, fe_from_canonical<FrP>(v));
        fe_st(D.pt, i, fe_from_canonical<FrP>(s));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// The sort alone (steps 1 and 2), for lookup_permute_device below and the witness check (check.hip): `cols` columns of 2^k elements,
// src[q] -> canonical keys, rows u .. n - 1 as all-ones keys at the end.  src, k0 and k1 are device tables of `cols` device pointers
// (k0[q], k1[q]: two key buffers of 2^k elements per column); the sorted keys end in k1[q] when lookup_sort_passes(k) is odd, else in k0[q].
static uint32_t lk_sort_block(uint32_t ts) {
    const uint32_t block = tune().lookup_sort_block ? tune().lookup_sort_block : LK_TILE;
    return block > ts ? ts : block;
}
uint32_t lookup_sort_passes(uint32_t k) {
    const uint64_t n = 1ull << k;
    uint32_t passes = 0;
    for (uint64_t w = lk_sort_block((uint32_t)(n < LK_TILE ? n : LK_TILE)); w < n; w <<= 1) passes++;
    return passes;
}
// d_r0 / d_r1 (both or neither): two row buffers of 2^k words per column; the sort then carries each key's row and breaks ties by it
static int lk_sort_enqueue(const Fe* const* d_src, Fe* const* d_k0, Fe* const* d_k1, uint32_t* const* d_r0, uint32_t* const* d_r1, uint32_t cols,
                           uint32_t k, uint64_t u, hipStream_t s) {
    const uint64_t n = 1ull << k;
    const uint32_t ts = (uint32_t)(n < LK_TILE ? n : LK_TILE), tiles = (uint32_t)(n / ts), block = lk_sort_block(ts);
    const uint32_t passes = lookup_sort_passes(k);
    uint32_t* const* no_rows = nullptr;
    if (d_r0) hipLaunchKernelGGL(lk_block_sort_kernel<true>, dim3(tiles, cols), dim3(LK_THREADS), 0, s, d_src, d_k0, d_r0, u, ts, block);
    else hipLaunchKernelGGL(lk_block_sort_kernel<false>, dim3(tiles, cols), dim3(LK_THREADS), 0, s, d_src, d_k0, no_rows, u, ts, block);
    H2_CHECK(hipGetLastError());
    uint32_t w = block;
    for (uint32_t p = 0; p < passes; p++, w <<= 1) {
        const Fe* const* from = p & 1 ? (const Fe* const*)d_k1 : (const Fe* const*)d_k0;
        if (d_r0)
            hipLaunchKernelGGL(lk_merge_kernel<true>, dim3(tiles, cols), dim3(LK_THREADS), 0, s, from, p & 1 ? d_k0 : d_k1,
                               (const uint32_t* const*)(p & 1 ? d_r1 : d_r0), p & 1 ? d_r0 : d_r1, w, ts);
        else
            hipLaunchKernelGGL(lk_merge_kernel<false>, dim3(tiles, cols), dim3(LK_THREADS), 0, s, from, p & 1 ? d_k0 : d_k1,
                               (const uint32_t* const*)nullptr, no_rows, w, ts);
        H2_CHECK(hipGetLastError());
    }
    g_lk_last[0] = block;
    g_lk_last[1] = passes;
    return 0;
}
int lookup_sort_enqueue(const Fe* const* d_src, Fe* const* d_k0, Fe* const* d_k1, uint32_t cols, uint32_t k, uint64_t u, hipStream_t s) {
    return lk_sort_enqueue(d_src, d_k0, d_k1, nullptr, nullptr, cols, k, u, s);
}

// Validated arguments; columns and outputs are device pointers (in[j], tab[j], pa[j], pt[j] for lookup j), blinding host memory.
// Enqueues everything on s, then waits for s once to read the not-found flags: H2HIP_ELOOKUP names the lowest failing lookup.
int lookup_permute_device(Ctx* c, uint32_t k, const Fe* const* in, const Fe* const* tab, size_t count, const uint64_t* blinding, uint32_t bf,
                          Fe* const* pa, Fe* const* pt, hipStream_t s) {
    if (count == 0) return 0;
    const uint64_t n = 1ull << k, u = n - bf - 1;
    const uint32_t ts = (uint32_t)(n < LK_TILE ? n : LK_TILE);
    const uint32_t tiles = (uint32_t)(n / ts), passes = lookup_sort_passes(k);
    const size_t cols = 2 * count, col_bytes = n * sizeof(Fe);
    const size_t nb = (size_t)bf + 1;
    // one lookup's workspace: the used marks, L (a column, packed), the tile counts of L and of R
    const size_t used_bytes = align256(n * sizeof(uint32_t)), cnt_bytes = ((size_t)tiles + 1) * sizeof(uint32_t);
    Carve lk;
    const size_t o_used = lk.take(used_bytes), o_lc = lk.take_packed(col_bytes), o_cnt_l = lk.take(cnt_bytes), o_cnt_r = lk.take(cnt_bytes);
    // the blob the kernels read: descriptors, three pointer tables of `cols` entries (sources, key buffers 0 and 1), blinding
    Carve blob;
    const size_t o_perm = blob.take(count * sizeof(LkPerm)), o_ptr = blob.take(3 * cols * sizeof(void*)),
                 o_blind = blob.take(count * 2 * nb * sizeof(Fe));
    // the call's workspace: two key buffers per sorted column ([buffer][column][n]), every lookup's, the flags, the blob
    Carve ws;
    const size_t o_keys = ws.take_packed(2 * cols * col_bytes), o_per = ws.take_packed(count * lk.total);
    const size_t o_flag = ws.take(count * sizeof(uint32_t)), o_blob = ws.take(blob.total);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->lookup_ws.ensure(ws.total))) return rc;
    if ((rc = c->lookup_flag.ensure(count * sizeof(uint32_t)))) return rc;
    char* base = (char*)c->lookup_ws.p;
    Fe* keys = (Fe*)(base + o_keys);
    char* per = base + o_per;
    uint32_t* d_flag = (uint32_t*)(base + o_flag);
    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<LkPerm> perm = img.at<LkPerm>(o_perm);
    const Mirror<const Fe*> src = img.at<const Fe*>(o_ptr);  // one table: the sources in entries [0, cols) ...
    const Mirror<Fe*> kbuf = img.at<Fe*>(o_ptr);             // ... key buffer 0 in [cols, 2 cols), key buffer 1 in [2 cols, 3 cols)
    const Mirror<Fe> blind = img.at<Fe>(o_blind);
    if (nb) memcpy(blind.h, blinding, count * 2 * nb * sizeof(Fe));
    Fe** hk0 = kbuf.h + cols;
    Fe** hk1 = kbuf.h + 2 * cols;
    const Fe* const* d_src = src.d;
    Fe* const* d_k0 = kbuf.d + cols;
    Fe* const* d_k1 = kbuf.d + 2 * cols;
    for (size_t q = 0; q < cols; q++) {
        src.h[q] = q & 1 ? tab[q / 2] : in[q / 2];
        hk0[q] = keys + q * n;
        hk1[q] = keys + (cols + q) * n;
    }
    Fe* const* h_sorted = passes & 1 ? hk1 : hk0;  // where the last pass leaves the keys
    for (size_t j = 0; j < count; j++) {
        char* pj = per + j * lk.total;
        LkPerm& D = perm.h[j];
        D.a = h_sorted[2 * j];
        D.t = h_sorted[2 * j + 1];
        D.used = (uint32_t*)(pj + o_used);
        D.lc = (Fe*)(pj + o_lc);
        D.cnt_l = (uint32_t*)(pj + o_cnt_l);
        D.cnt_r = (uint32_t*)(pj + o_cnt_r);
        D.flag = d_flag + j;
        D.pa = pa[j];
        D.pt = pt[j];
        D.blind = blind.d + j * 2 * nb;
    }
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;
    for (size_t j = 0; j < count; j++) H2_CHECK(hipMemsetAsync(per + j * lk.total + o_used, 0, used_bytes, s));
    H2_CHECK(hipMemsetAsync(d_flag, 0, count * sizeof(uint32_t), s));
    const LkPerm* d_perm = perm.d;
    int tm = c->timer_begin("lookup_permute", s);
    if ((rc = lookup_sort_enqueue(d_src, d_k0, d_k1, (uint32_t)cols, k, u, s))) return rc;
    const dim3 grid(tiles, (uint32_t)count);
    hipLaunchKernelGGL(lk_mark_kernel, grid, dim3(LK_THREADS), 0, s, d_perm, u);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lk_count_kernel, grid, dim3(LK_THREADS), 0, s, d_perm, u);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lk_scan_kernel, dim3((uint32_t)count), dim3(LK_THREADS), 0, s, d_perm, tiles);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lk_compact_kernel, grid, dim3(LK_THREADS), 0, s, d_perm, u);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lk_final_kernel, grid, dim3(LK_THREADS), 0, s, d_perm, u, n, tiles);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    H2_CHECK(hipMemcpyAsync(c->lookup_flag.p, d_flag, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));  // the caller must know before it commits
    const uint32_t* flags = (const uint32_t*)c->lookup_flag.p;
    for (size_t j = 0; j < count; j++)
        if (flags[j]) {
            set_error("lookup_permute: lookup %zu: an input value is not in the table (ConstraintSystemFailure)", j);
            return H2HIP_ELOOKUP;
        }
    return 0;
}

// ---- the logUp (mv-lookup) argument's multiplicity column (include/halo2hip.h, h2hip_mvlookup_multiplicities_bn254) ---------------
// Plan (mv-lookup).  Per argument the table's (canonical key, row) pairs of rows < u are sorted by the launches above,
// the row breaking ties, so the lower bound of a value is the lowest table row that holds it.  Then
//   mv_count_kernel   (tiles x input columns): one lane per input cell -- lower bound in the sorted table, one 32-bit atomic add at the
//                     found row.  Integer counts do not depend on the order of the additions.  Lanes of a wave that found the same row
//                     are added up first (MV_ROUNDS leaders, each one atomic for all its followers): the rows of a disabled selector
//                     all hit one value, and without this every one of them is an atomic on one address;
//   mv_final_kernel   (tiles x arguments): counts -> Montgomery form, rows >= u zero.
// A missing value raises its input column's flag: a ballot per wave, an OR over the workgroup's waves, one plain store.  The host reads
// the flags once and names the lowest (argument, input).
#ifndef MV_ROUNDS
#define MV_ROUNDS 4  // leaders per wave; measured against 0, 1 and 64 (mv-lookup)
#endif
struct MvArg {             // one argument
    const Fe* tkeys;       // sorted canonical table keys, all-ones from position u on
    const uint32_t* trows; // their rows
    uint32_t* cnt;         // 2^k counts, zero on entry
    Fe* m;                 // output, Montgomery form
};
struct MvCol {             // one input column
    const Fe* in;          // compressed input, Montgomery form
    uint32_t arg;
    uint32_t pad;
};

__global__ __launch_bounds__(LK_THREADS) void mv_count_kernel(const MvArg* args, const MvCol* cols, uint32_t* flags, uint64_t u) {
    __shared__ uint32_t s_bad[LK_THREADS / 64];
    const MvCol C = cols[blockIdx.y];
    const MvArg A = args[C.arg];
    const uint64_t i = (uint64_t)blockIdx.x * LK_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool found = false, bad = false;
    uint32_t row = 0xffffffffu;
    if (i < u) {
        const Fe v = fe_to_canonical<FrP>(fe_ld(C.in, i));
        uint64_t lo = 0, hi = u;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key_lt(fe_ld(A.tkeys, mid), v)) lo = mid + 1;
            else hi = mid;
        }
        found = lo < u && fe_eq(fe_ld(A.tkeys, lo), v);
        bad = !found;
        if (found) row = A.trows[lo];
    }
    // every lane of the wave is here: the lanes that found the leader's row leave with one atomic
    uint64_t todo = __ballot(found);
    for (int round = 0; round < MV_ROUNDS && todo; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t r = (uint32_t)__shfl((int)row, leader);
        const uint64_t same = __ballot(found && row == r) & todo;
        if (lane == (uint32_t)leader) atomicAdd(A.cnt + r, (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(A.cnt + row, 1u);
    const uint64_t wave_bad = __ballot(bad);
    if (lane == 0) s_bad[threadIdx.x >> 6] = wave_bad != 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t any = 0;
        for (uint32_t w = 0; w < LK_THREADS / 64; w++) any |= s_bad[w];
        if (any) flags[blockIdx.y] = 1u;
    }
}

__global__ __launch_bounds__(LK_THREADS) void mv_final_kernel(const MvArg* args, uint64_t u, uint64_t n) {
    const MvArg A = args[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= n) return;
    Fe v = fe_zero<FrP>();
    if (i < u) {
        v.l[0] = A.cnt[i];
        v = fe_from_canonical<FrP>(v);
    }
    fe_st(A.m, i, v);
}

// Validated arguments; in (flat, argument-major), tab and m are device pointers.  Enqueues everything on s, then waits for s once to
// read the flags: H2HIP_ELOOKUP names the lowest failing (argument, input column); every m is written either way.
int mvlookup_multiplicities_device(Ctx* c, uint32_t k, const Fe* const* in, const uint32_t* n_inputs, const Fe* const* tab, size_t count,
                                   uint32_t bf, Fe* const* m, hipStream_t s) {
    if (count == 0) return 0;
    const uint64_t n = 1ull << k, u = n - bf - 1;
    const uint32_t passes = lookup_sort_passes(k);
    size_t total_in = 0;
    for (size_t j = 0; j < count; j++) total_in += n_inputs[j];
    const size_t col_bytes = n * sizeof(Fe), row_bytes = n * sizeof(uint32_t);
    Carve blob;
    const size_t o_arg = blob.take(count * sizeof(MvArg)), o_col = blob.take(total_in * sizeof(MvCol)), o_ptr = blob.take(5 * count * sizeof(void*));
    Carve ws;
    const size_t o_keys = ws.take_packed(2 * count * col_bytes), o_rows = ws.take_packed(2 * count * row_bytes);
    const size_t o_cnt = ws.take(count * row_bytes), o_flag = ws.take(total_in * sizeof(uint32_t)), o_blob = ws.take(blob.total);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->lookup_ws.ensure(ws.total))) return rc;
    if ((rc = c->lookup_flag.ensure(total_in * sizeof(uint32_t)))) return rc;
    char* base = (char*)c->lookup_ws.p;
    Fe* keys = (Fe*)(base + o_keys);
    uint32_t* rows = (uint32_t*)(base + o_rows);
    uint32_t* cnt = (uint32_t*)(base + o_cnt);
    uint32_t* d_flag = (uint32_t*)(base + o_flag);
    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<MvArg> arg = img.at<MvArg>(o_arg);
    const Mirror<MvCol> col = img.at<MvCol>(o_col);
    const Mirror<const Fe*> src = img.at<const Fe*>(o_ptr);  // one table: sources [0, count), key buffers 0 and 1, row buffers 0 and 1
    const Mirror<Fe*> kbuf = img.at<Fe*>(o_ptr);
    const Mirror<uint32_t*> rbuf = img.at<uint32_t*>(o_ptr);
    size_t q = 0;
    for (size_t j = 0; j < count; j++) {
        src.h[j] = tab[j];
        kbuf.h[count + j] = keys + j * n;
        kbuf.h[2 * count + j] = keys + (count + j) * n;
        rbuf.h[3 * count + j] = rows + j * n;
        rbuf.h[4 * count + j] = rows + (count + j) * n;
        MvArg& A = arg.h[j];
        A.tkeys = passes & 1 ? kbuf.h[2 * count + j] : kbuf.h[count + j];  // where the last pass leaves them
        A.trows = passes & 1 ? rbuf.h[4 * count + j] : rbuf.h[3 * count + j];
        A.cnt = cnt + j * n;
        A.m = m[j];
        for (uint32_t t = 0; t < n_inputs[j]; t++, q++) {
            col.h[q].in = in[q];
            col.h[q].arg = (uint32_t)j;
        }
    }
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;
    H2_CHECK(hipMemsetAsync(cnt, 0, count * row_bytes, s));
    H2_CHECK(hipMemsetAsync(d_flag, 0, total_in * sizeof(uint32_t), s));
    int tm = c->timer_begin("mvlookup_multiplicities", s);
    if ((rc = lk_sort_enqueue(src.d, kbuf.d + count, kbuf.d + 2 * count, rbuf.d + 3 * count, rbuf.d + 4 * count, (uint32_t)count, k, u, s))) return rc;
    const uint32_t tiles_u = (uint32_t)((u + LK_THREADS - 1) / LK_THREADS), tiles_n = (uint32_t)((n + LK_THREADS - 1) / LK_THREADS);
    for (size_t c0 = 0; c0 < total_in; c0 += 65535) {  // grid.y holds 65535 columns
        const size_t cn = total_in - c0 < 65535 ? total_in - c0 : 65535;
        hipLaunchKernelGGL(mv_count_kernel, dim3(tiles_u, (uint32_t)cn), dim3(LK_THREADS), 0, s, arg.d, col.d + c0, d_flag + c0, u);
        H2_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(mv_final_kernel, dim3(tiles_n, (uint32_t)count), dim3(LK_THREADS), 0, s, arg.d, u, n);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    H2_CHECK(hipMemcpyAsync(c->lookup_flag.p, d_flag, total_in * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = guard.release())) return rc;
    H2_CHECK(hipStreamSynchronize(s));  // the caller must know before it commits
    const uint32_t* flags = (const uint32_t*)c->lookup_flag.p;
    q = 0;
    for (size_t j = 0; j < count; j++)
        for (uint32_t t = 0; t < n_inputs[j]; t++, q++)
            if (flags[q]) {
                set_error("mvlookup_multiplicities: argument %zu, input %u: an input value is not in the table (ConstraintSystemFailure)", j, t);
                return H2HIP_ELOOKUP;
            }
    return 0;
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "lookup compression and permutation") -----------------------------------------------------------
static int compress_check(uint32_t k, const void* const* fixed, uint32_t n_fixed, const void* const* advice, uint32_t n_advice,
                          const void* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                          const uint64_t* theta, const h2hip_graph* graphs, size_t n_graphs, const void* const* out) {
    const char* what = "lookup_compress";
    if (int rc = check_k(what, k)) return rc;
    if (!theta || (n_challenges && !challenges)) {
        set_error("%s: null theta or challenges", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(theta, "theta")) return H2HIP_EINVAL;
    if (check_frs(what, challenges, n_challenges, "challenge")) return H2HIP_EINVAL;
    if (check_ptrs(what, fixed, n_fixed, "fixed_values") || check_ptrs(what, advice, n_advice, "advice_values") ||
        check_ptrs(what, instance, n_instance, "instance_values") || check_ptrs(what, out, n_graphs, "out"))
        return H2HIP_EINVAL;
    return lookup_compress_validate(n_fixed, n_advice, n_instance, n_challenges, graphs, n_graphs);
}

static int permute_check(uint32_t k, const void* const* in, const void* const* tab, size_t count, const uint64_t* blinding, uint32_t bf,
                         const void* const* pa, const void* const* pt) {
    const char* what = "lookup_permute";
    if (int rc = check_k_blinding(what, k, bf)) return rc;
    if (count > LK_MAX_COUNT) {
        set_error("%s: count %zu > %d", what, count, LK_MAX_COUNT);
        return H2HIP_EINVAL;
    }
    if (count && !blinding) {
        set_error("%s: null blinding", what);
        return H2HIP_EINVAL;
    }
    if (check_frs(what, blinding, count * 2 * ((size_t)bf + 1), "blinding value")) return H2HIP_EINVAL;
    if (check_ptrs(what, in, count, "compressed_input") || check_ptrs(what, tab, count, "compressed_table") ||
        check_ptrs(what, pa, count, "permuted_input") || check_ptrs(what, pt, count, "permuted_table"))
        return H2HIP_EINVAL;
    return 0;
}

int h2hip_lookup_compress_bn254_device(uint32_t k, const void* const* d_fixed_values, uint32_t n_fixed, const void* const* d_advice_values,
                                       uint32_t n_advice, const void* const* d_instance_values, uint32_t n_instance, const uint64_t* challenges,
                                       uint32_t n_challenges, const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, void* const* d_out,
                                       void* stream) {
    if (int rc = compress_check(k, d_fixed_values, n_fixed, d_advice_values, n_advice, d_instance_values, n_instance, challenges, n_challenges,
                                theta, graphs, n_graphs, (const void* const*)d_out))
        return rc;
    if (n_graphs == 0) return 0;
    Entry en("h2hip_lookup_compress_bn254_device", d_out[0]);
    if (en.rc) return en.rc;
    return lookup_compress_device(en.c, k, (const Fe* const*)d_fixed_values, n_fixed, (const Fe* const*)d_advice_values, n_advice,
                                  (const Fe* const*)d_instance_values, n_instance, challenges, n_challenges, theta, graphs, n_graphs,
                                  (Fe* const*)d_out, (hipStream_t)stream);
}

int h2hip_lookup_compress_bn254(uint32_t k, const uint64_t* const* fixed_values, uint32_t n_fixed, const uint64_t* const* advice_values,
                                uint32_t n_advice, const uint64_t* const* instance_values, uint32_t n_instance, const uint64_t* challenges,
                                uint32_t n_challenges, const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, uint64_t* const* out) {
    if (int rc = compress_check(k, (const void* const*)fixed_values, n_fixed, (const void* const*)advice_values, n_advice,
                                (const void* const*)instance_values, n_instance, challenges, n_challenges, theta, graphs, n_graphs,
                                (const void* const*)out))
        return rc;
    if (n_graphs == 0) return 0;
    Entry en("h2hip_lookup_compress_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> d_fixed(n_fixed), d_advice(n_advice), d_instance(n_instance);
    std::vector<Fe*> d_out(n_graphs);
    HostIo io(c, c->host_io, s);
    // fixed columns pinned with h2hip_columns_pin are read where they lie; the witness columns and the rest cross PCIe
    for (uint32_t j = 0; j < n_fixed; j++) io.in(fixed_values[j], bytes, &d_fixed[j], true);
    for (uint32_t j = 0; j < n_advice; j++) io.in(advice_values[j], bytes, &d_advice[j]);
    for (uint32_t j = 0; j < n_instance; j++) io.in(instance_values[j], bytes, &d_instance[j]);
    for (size_t g = 0; g < n_graphs; g++) io.out(out[g], bytes, &d_out[g]);
    int rc = io.upload();
    if (rc) return rc;
    rc = lookup_compress_device(c, k, d_fixed.data(), n_fixed, d_advice.data(), n_advice, d_instance.data(), n_instance, challenges, n_challenges,
                                theta, graphs, n_graphs, d_out.data(), s);
    if (rc) return rc;
    return io.finish();
}

int h2hip_lookup_permute_bn254_device(uint32_t k, const void* const* d_compressed_input, const void* const* d_compressed_table, size_t count,
                                      const uint64_t* blinding, uint32_t blinding_factors, void* const* d_permuted_input,
                                      void* const* d_permuted_table, void* stream) {
    if (int rc = permute_check(k, d_compressed_input, d_compressed_table, count, blinding, blinding_factors, (const void* const*)d_permuted_input,
                               (const void* const*)d_permuted_table))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_lookup_permute_bn254_device", d_permuted_input[0]);
    if (en.rc) return en.rc;
    return lookup_permute_device(en.c, k, (const Fe* const*)d_compressed_input, (const Fe* const*)d_compressed_table, count, blinding,
                                 blinding_factors, (Fe* const*)d_permuted_input, (Fe* const*)d_permuted_table, (hipStream_t)stream);
}

int h2hip_lookup_permute_bn254(uint32_t k, const uint64_t* const* compressed_input, const uint64_t* const* compressed_table, size_t count,
                               const uint64_t* blinding, uint32_t blinding_factors, uint64_t* const* permuted_input, uint64_t* const* permuted_table) {
    if (int rc = permute_check(k, (const void* const*)compressed_input, (const void* const*)compressed_table, count, blinding, blinding_factors,
                               (const void* const*)permuted_input, (const void* const*)permuted_table))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_lookup_permute_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> in(count), tab(count);
    std::vector<Fe*> pa(count), pt(count);
    HostIo io(c, c->host_io, s);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_input[j], bytes, &in[j]);
        io.in(compressed_table[j], bytes, &tab[j]);
        io.out(permuted_input[j], bytes, &pa[j]);
        io.out(permuted_table[j], bytes, &pt[j]);
    }
    int rc = io.upload();
    if (rc) return rc;
    rc = lookup_permute_device(c, k, in.data(), tab.data(), count, blinding, blinding_factors, pa.data(), pt.data(), s);
    if (rc) return rc;
    return io.finish();
}

// ---- the mv-lookup multiplicities ------------------------------------------------------------------------------------------------
static int multiplicities_check(uint32_t k, const void* const* in, const uint32_t* n_inputs, const void* const* tab, size_t count, uint32_t bf,
                                const void* const* m, size_t* total_in) {
    const char* what = "mvlookup_multiplicities";
    if (int rc = check_k_blinding(what, k, bf)) return rc;
    if (count > 65535) {
        set_error("%s: count %zu > 65535", what, count);
        return H2HIP_EINVAL;
    }
    if (count && !n_inputs) {
        set_error("%s: null n_inputs", what);
        return H2HIP_EINVAL;
    }
    size_t total = 0;
    for (size_t j = 0; j < count; j++) {
        if (n_inputs[j] < 1 || n_inputs[j] > 255) {
            set_error("%s: n_inputs[%zu] = %u, not in [1, 255]", what, j, n_inputs[j]);
            return H2HIP_EINVAL;
        }
        if (((uint64_t)n_inputs[j] << k) > 0xffffffffull) {  // every cell could hit one row: the counts are 32-bit
            set_error("%s: n_inputs[%zu] = %u columns of 2^%u rows exceed a 32-bit count", what, j, n_inputs[j], k);
            return H2HIP_EINVAL;
        }
        total += n_inputs[j];
    }
    if (check_ptrs(what, in, total, "compressed_input") || check_ptrs(what, tab, count, "compressed_table") || check_ptrs(what, m, count, "m"))
        return H2HIP_EINVAL;
    *total_in = total;
    return 0;
}

int h2hip_mvlookup_multiplicities_bn254_device(uint32_t k, const void* const* d_compressed_inputs, const uint32_t* n_inputs,
                                               const void* const* d_compressed_tables, size_t count, uint32_t blinding_factors, void* const* d_m,
                                               void* stream) {
    size_t total_in;
    if (int rc = multiplicities_check(k, d_compressed_inputs, n_inputs, d_compressed_tables, count, blinding_factors, (const void* const*)d_m, &total_in))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_mvlookup_multiplicities_bn254_device", d_m[0]);
    if (en.rc) return en.rc;
    return mvlookup_multiplicities_device(en.c, k, (const Fe* const*)d_compressed_inputs, n_inputs, (const Fe* const*)d_compressed_tables, count,
                                          blinding_factors, (Fe* const*)d_m, (hipStream_t)stream);
}

int h2hip_mvlookup_multiplicities_bn254(uint32_t k, const uint64_t* const* compressed_inputs, const uint32_t* n_inputs,
                                        const uint64_t* const* compressed_tables, size_t count, uint32_t blinding_factors, uint64_t* const* m) {
    size_t total_in;
    if (int rc = multiplicities_check(k, (const void* const*)compressed_inputs, n_inputs, (const void* const*)compressed_tables, count,
                                      blinding_factors, (const void* const*)m, &total_in))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_mvlookup_multiplicities_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> in(total_in), tab(count);
    std::vector<Fe*> d_m(count);
    HostIo io(c, c->host_io, s);
    for (size_t q = 0; q < total_in; q++) io.in(compressed_inputs[q], bytes, &in[q]);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_tables[j], bytes, &tab[j]);
        io.out(m[j], bytes, &d_m[j]);
    }
    if (int rc = io.upload()) return rc;
    const int verdict = mvlookup_multiplicities_device(c, k, in.data(), n_inputs, tab.data(), count, blinding_factors, d_m.data(), s);
    if (verdict && verdict != H2HIP_ELOOKUP) return verdict;
    if (int rc = io.finish()) return rc;  // the m are written either way
    return verdict;
}

int h2hip_debug_set_lookup_sort(uint32_t lds_keys) {
    if (lds_keys && (lds_keys < 4 || lds_keys > LK_TILE || (lds_keys & (lds_keys - 1)))) {
        set_error("debug_set_lookup_sort: the in-LDS sort block must be a power of two in [4, %d], or 0", LK_TILE);
        return H2HIP_EINVAL;
    }
    TuneWrite()->lookup_sort_block = lds_keys;
    return 0;
}

int h2hip_debug_lookup_sort_stats(uint32_t out[2]) {
    if (!out) {
        set_error("debug_lookup_sort_stats: null argument");
        return H2HIP_EINVAL;
    }
    out[0] = g_lk_last[0];
    out[1] = g_lk_last[1];
    return 0;
}

}  // extern "C"
