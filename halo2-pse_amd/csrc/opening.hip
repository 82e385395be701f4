// opening.hip -- the opening phase of create_proof on the GPU: batched polynomial evaluation and the combine / divide / scale
// primitive that GWC, both SHPLONK stages, the vanishing argument's h_poly fold and plain kate_division are built from.
//
// Replaces the host loops after evaluate_h:
//   eval_polynomial (arithmetic.rs:304-328) at every query site (plonk/prover.rs:529, :550, :568, vanishing/prover.rs:145,
//       permutation/prover.rs:227-275, lookup/prover.rs:319-323) and again in ProverQuery::get_eval (poly/query.rs:51-53);
//   kate_division (arithmetic.rs:348-366), div_by_vanishing (poly/kzg/multiopen/shplonk/prover.rs:26-31) and the linear
//       combinations of gwc/prover.rs:61-89, shplonk/prover.rs:138-275 and vanishing/prover.rs:131-135.
//
// Plan (Opening).
//   Evaluation: queries grouped by polynomial, up to OPEN_MAX_POINTS points per pass, so that one read of a polynomial serves
//   all of them.  Thread t of tile g reads coefficients g T + t + j B (j < R; coalesced) and runs Horner in y = x^B, a weighted
//   tree over the tile's threads multiplies by x^t, lane 0 by x^(g T) (table x^(2^b)); open_eval_sum_kernel adds the tiles.
//   Division: with S(i) = sum_{j >= i} a[j] r^(j - i), kate_division's q[i] = S(i + 1) and a(r) = S(0).  S is a suffix
//   recurrence S(i) = a[i] + r S(i + 1), computed as a reduce-then-scan over descending indices, no workgroup waiting on another:
//     1. open_scan_kernel   (tiles): a = sum_j s_j p_j - sub fused into the loads (a is never written), each thread's local
//                           suffix over R consecutive indices -> w, a descending scan of the thread totals weighted by r^R;
//     2. open_tiles_kernel  (one workgroup): the tile totals scanned with r^(R B): each tile's carry S(tile end), and S(0);
//     3. open_apply_kernel  (tiles): S(i) = w[i] + r^(end - i) carry, stored as q[i - 1] (times scale, added to out).
//   Several roots run as successive scans over two scratch columns.  With no roots open_combine_kernel writes a directly.
// Row passes use fieldu.h's lazy 29-bit limbs (explicit-mad flavour); stored values are canonical E-form Fe, as everywhere.
#include <string.h>
#include <algorithm>
#include <vector>
#include "engine.h"
#include "fe_io.h"
#include "fieldu.h"
#include "../../include/halo2hip_debug.h"

namespace h2 {

#define OPEN_MAX_THREADS 256
#define OPEN_MAX_POINTS 8   // points one pass over a polynomial serves
#define OPEN_MAX_ROOTS 16
#define OPEN_MAX_SUB 16
#define OPEN_POW 48         // tables of v^(2^b), b < OPEN_POW
#define OPEN_MAX_LEN ((uint64_t)1 << 28)

typedef FrUA OpU;

// s + y * v for canonical s, v (E-form) and an I-form power y (fu_from_ext): value < 0.2 p + 2 p, back to canonical
__device__ __forceinline__ Fe op_axpy(const Fe& s, const Fu& y, const Fe& v) {
    return fu_canon_fast<OpU>(fu_mul_subh<OpU>(fu_slice(v), y, fu_neg(fu_slice(s))));
}

// ---- evaluation ----------------------------------------------------------------------------------------------------------
struct EvalPass {
    const Fe* poly;
    uint64_t len;
    uint32_t tiles;                  // tiles of R B coefficients this pass covers (0: a length-0 polynomial)
    uint32_t np;
    uint32_t q[OPEN_MAX_POINTS];     // query indices: rows of the power tables and of the partials
};

struct EvalParams {
    const EvalPass* passes;
    const Fu* xpow;                  // query q: x^(2^b) at [q OPEN_POW + b], I-form
    Fe* partial;                     // [q max_tiles + tile]
    uint32_t R, B, logB, max_tiles;
};

template <int NP>
__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_eval_kernel(EvalParams P) {
    __shared__ Fe lds[OPEN_MAX_THREADS];
    const EvalPass& D = P.passes[blockIdx.y];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    if (tile >= D.tiles) return;  // uniform over the workgroup
    const uint64_t tile_lo = (uint64_t)tile * P.R * P.B, base = tile_lo + tid;
    Fu y[NP], acc[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        y[k] = P.xpow[(size_t)D.q[k] * OPEN_POW + P.logB];
        acc[k] = fu_zero();
    }
    for (int j = (int)P.R - 1; j >= 0; j--) {  // indices above len come first and leave acc at zero
        const uint64_t i = base + (uint64_t)j * P.B;
        if (i >= D.len) continue;
        const Fu nc = fu_neg(fu_slice(fe_ld(D.poly, i)));
#pragma unroll
        for (int k = 0; k < NP; k++) acc[k] = fu_mul_subh<OpU>(acc[k], y[k], nc);  // acc y + c: value stays below 2.5 p
    }
    Fe fin[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) fin[k] = fu_canon_fast<OpU>(acc[k]);
#pragma unroll NP
    for (int k = 0; k < NP; k++) {
        const Fu* xp = P.xpow + (size_t)D.q[k] * OPEN_POW;
        lds[tid] = fin[k];
        __syncthreads();
        for (uint32_t h = P.B >> 1, b = P.logB; h >= 1; h >>= 1) {  // v[t] += x^h v[t + h]: sum_t acc_t x^t
            b--;
            if (tid < h) lds[tid] = op_axpy(lds[tid], xp[b], lds[tid + h]);
            __syncthreads();
        }
        if (tid == 0) {
            Fu v = fu_slice(lds[0]);
            for (uint32_t b = 0; b < 40; b++)
                if ((tile_lo >> b) & 1) v = fu_mul<OpU>(v, xp[b]);
            fe_st(P.partial, (size_t)D.q[k] * P.max_tiles + tile, fu_canon_fast<OpU>(v));
        }
        __syncthreads();
    }
}

// evals[q] = sum of the query's tile partials (one workgroup per query)
__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_eval_sum_kernel(const Fe* partial, const uint32_t* qtiles, uint32_t max_tiles, Fe* evals) {
    __shared__ Fe lds[OPEN_MAX_THREADS];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, T = qtiles[q];
    Fe s = fe_zero<FrP>();
    for (uint32_t t = tid; t < T; t += OPEN_MAX_THREADS) s = fe_add<FrP>(s, fe_ld(partial, (size_t)q * max_tiles + t));
    lds[tid] = s;
    __syncthreads();
    for (uint32_t h = OPEN_MAX_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) lds[tid] = fe_add<FrP>(lds[tid], lds[tid + h]);
        __syncthreads();
    }
    if (tid == 0) fe_st(evals, q, lds[0]);
}

// ---- combine / divide ----------------------------------------------------------------------------------------------------
struct CombParams {
    const Fe* const* polys;  // stage 0: the polynomials, n_polys of them
    const Fu* scal;          // [2 j] = s_j, [2 j + 1] = -s_j, I-form
    const Fe* sub;           // sub_len low coefficients subtracted from the combination (canonical)
    const Fe* in;            // later stages: the previous quotient
    Fe* w;                   // local suffixes (may be `in`)
    Fe* thr;                 // per-thread carries inside a tile, tiles x B
    Fe* tile;                // tile totals, then each tile's carry
    Fe* out;
    Fe* rem;                 // S(0) of this stage, or nullptr
    const Fu* rpow;          // r^(2^b), I-form
    uint64_t L;              // input length of the stage
    uint32_t n_polys, sub_len, R, B, logR, logB, tiles, log_per;
    uint32_t first, last, accumulate, scale_one;
    Fu scale;                // canonical I-form limbs of scale (fu_mul_canon operand)
};

// a[i] = sum_j s_j p_j[i] - sub[i]: E-form, |value| < 14 p
__device__ __forceinline__ Fu comb_load(const CombParams& P, uint64_t i) {
    if (!P.first) return fu_slice(fe_ld(P.in, i));
    Fu acc = fu_zero();
    uint32_t j = 0, cnt = 0;
    for (; j + 1 < P.n_polys; j += 2) {  // two products, one reduction: (p_j s_j - p_{j+1} (-s_{j+1})) / 2^261, value < 1.4 p
        Fu t = fu_mul_sub<OpU>(fu_slice(fe_ld(P.polys[j], i)), P.scal[2 * j], fu_slice(fe_ld(P.polys[j + 1], i)), P.scal[2 * j + 3]);
        acc = fu_norm(fu_add(acc, t));
        if (++cnt == 8) {  // < p + 8 x 1.4 p: back to canonical before the sum leaves fu_canon_fast's range
            acc = fu_slice(fu_canon_fast<OpU>(acc));
            cnt = 0;
        }
    }
    if (j < P.n_polys) acc = fu_norm(fu_add(acc, fu_mul<OpU>(fu_slice(fe_ld(P.polys[j], i)), P.scal[2 * j])));
    if (i < P.sub_len) acc = fu_norm(fu_sub(acc, fu_slice(P.sub[i])));
    return acc;
}

__device__ __forceinline__ void comb_store(const CombParams& P, uint64_t o, const Fu& v) {
    if (!P.last) {
        fe_st(P.out, o, fu_canon_fast<OpU>(v));
        return;
    }
    Fe r = P.scale_one ? fu_canon_fast<OpU>(v) : fu_mul_canon<OpU>(v, P.scale);
    if (P.accumulate) r = fe_add<FrP>(r, fe_ld(P.out, o));
    fe_st(P.out, o, r);
}

// descending inclusive scan over the B threads of a workgroup: I_t = v_t + m I_{t+1}, m^(2^l) = pw[l]; returns I_{t+1} (0 for the last)
__device__ Fe block_suffix_scan(Fe v, const Fu* pw, uint32_t B, Fe* lds) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t off = 1, l = 0; off < B; off <<= 1, l++) {
        const bool on = tid + off < B;
        Fe o = on ? lds[tid + off] : v;
        __syncthreads();
        if (on) v = op_axpy(v, pw[l], o);
        lds[tid] = v;
        __syncthreads();
    }
    Fe ex = tid + 1 < B ? lds[tid + 1] : fe_zero<FrP>();
    __syncthreads();
    return ex;
}

__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_combine_kernel(CombParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.L) comb_store(P, i, comb_load(P, i));
}

__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_scan_kernel(CombParams P) {
    __shared__ Fe lds[OPEN_MAX_THREADS];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t lo = ((uint64_t)tile * P.B + tid) * P.R;
    const Fu r = P.rpow[0];
    Fe S = fe_zero<FrP>();
    if (lo < P.L) {
        const uint64_t hi = lo + P.R < P.L ? lo + P.R : P.L;
        for (uint64_t i = hi; i-- > lo;) {  // S = a[i] + r S: value < 0.2 p + 14 p + p
            S = fu_canon_fast<OpU>(fu_mul_subh<OpU>(fu_slice(S), r, fu_neg(comb_load(P, i))));
            fe_st(P.w, i, S);
        }
    }
    const Fe ex = block_suffix_scan(S, P.rpow + P.logR, P.B, lds);  // the suffix of the threads above, weighted by r^R per thread
    fe_st(P.thr, (size_t)tile * P.B + tid, ex);
    if (tid == 0) fe_st(P.tile, tile, op_axpy(S, P.rpow[P.logR], ex));
}

// one workgroup of OPEN_MAX_THREADS: thread t takes tiles [t 2^log_per, (t + 1) 2^log_per)
__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_tiles_kernel(CombParams P) {
    __shared__ Fe lds[OPEN_MAX_THREADS];
    const uint32_t tid = threadIdx.x, lm = P.logR + P.logB;
    const Fu m = P.rpow[lm];
    const uint64_t lo = (uint64_t)tid << P.log_per, T = P.tiles;
    const uint64_t hi = lo + (1ull << P.log_per) < T ? lo + (1ull << P.log_per) : T;
    Fe S = fe_zero<FrP>();
    for (uint64_t u = hi; u-- > lo;) S = op_axpy(fe_ld(P.tile, u), m, S);
    Fe c = block_suffix_scan(S, P.rpow + lm + P.log_per, OPEN_MAX_THREADS, lds);
    for (uint64_t u = hi; u-- > lo;) {
        const Fe agg = fe_ld(P.tile, u);
        fe_st(P.tile, u, c);
        c = op_axpy(agg, m, c);
    }
    if (tid == 0 && P.rem) fe_st(P.rem, 0, c);  // S(0) = a(r)
}

__global__ __launch_bounds__(OPEN_MAX_THREADS) void open_apply_kernel(CombParams P) {
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t lo = ((uint64_t)tile * P.B + tid) * P.R;
    if (lo >= P.L) return;
    // this thread's carry S(lo + R) = (suffix of the threads above in the tile) + r^(R (B - 1 - tid)) (the tile's carry)
    Fu pc = fu_slice(fe_ld(P.tile, tile));
    const uint32_t e = P.B - 1 - tid;
    for (uint32_t b = 0; b < P.logB; b++)
        if ((e >> b) & 1) pc = fu_mul<OpU>(pc, P.rpow[P.logR + b]);
    Fu p = fu_slice(fu_canon_fast<OpU>(fu_norm(fu_add(pc, fu_slice(fe_ld(P.thr, (size_t)tile * P.B + tid))))));
    const Fu r = P.rpow[0];
    const uint64_t hi = lo + P.R < P.L ? lo + P.R : P.L;  // past L the carry is zero
    for (uint64_t i = hi; i-- > lo;) {
        p = fu_mul<OpU>(p, r);  // r^(lo + R - i) carry: value below 1.25 p
        if (i == 0) break;      // S(0) is the remainder (open_tiles_kernel)
        comb_store(P, i - 1, fu_norm(fu_add(fu_slice(fe_ld(P.w, i)), p)));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static uint32_t ilog2(uint64_t v) {
    uint32_t l = 0;
    while ((1ull << (l + 1)) <= v) l++;
    return l;
}

// rows per thread and threads per tile: about 2^17 threads over the call (8 waves per CU), or the debug hook's shape
static void open_shape(uint64_t elems, uint32_t max_r, uint32_t* R, uint32_t* B) {
    uint32_t r = 1;
    while (r < max_r && ((uint64_t)r * 2) << 17 <= elems) r *= 2;
    *R = tune().open_rows ? tune().open_rows : r;
    *B = tune().open_threads ? tune().open_threads : OPEN_MAX_THREADS;
}

static void pow_table(const Fe& x, Fu* out) {  // x^(2^b), I-form
    Fe w = x;
    for (int b = 0; b < OPEN_POW; b++) {
        out[b] = fu_from_ext(w);
        w = fe_mul<FrP>(w, w);
    }
}

// evals (device, n_queries) of the polynomials at the queries' points; enqueued on s
static int eval_run(Ctx* c, const Fe* const* polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly, const Fe* points,
                    size_t n_queries, Fe* d_evals, hipStream_t s) {
    // group the queries by polynomial, OPEN_MAX_POINTS per pass
    std::vector<std::vector<uint32_t>> by_poly(n_polys);
    for (size_t q = 0; q < n_queries; q++) by_poly[query_poly[q]].push_back((uint32_t)q);
    std::vector<EvalPass> passes;
    uint64_t elems = 0;
    for (size_t j = 0; j < n_polys; j++)
        for (size_t f = 0; f < by_poly[j].size(); f += OPEN_MAX_POINTS) {
            EvalPass p;
            memset(&p, 0, sizeof(p));
            p.poly = polys[j];
            p.len = lens[j];
            p.np = (uint32_t)std::min<size_t>(OPEN_MAX_POINTS, by_poly[j].size() - f);
            for (uint32_t k = 0; k < p.np; k++) p.q[k] = by_poly[j][f + k];
            passes.push_back(p);
            elems += lens[j];
        }
    uint32_t R, B;
    open_shape(elems, 32, &R, &B);
    const uint64_t T = (uint64_t)R * B;
    uint32_t max_tiles = 1;
    std::vector<uint32_t> qtiles(n_queries, 0);
    for (auto& p : passes) {
        p.tiles = (uint32_t)((p.len + T - 1) / T);
        max_tiles = std::max(max_tiles, p.tiles);
        for (uint32_t k = 0; k < p.np; k++) qtiles[p.q[k]] = p.tiles;
    }
    // passes sorted by point count: one launch per count
    std::stable_sort(passes.begin(), passes.end(), [](const EvalPass& a, const EvalPass& b) { return a.np < b.np; });
    // the blob the kernels read (passes, power tables, tile counts), then the tile partials
    Carve blob;
    const size_t o_pass = blob.take(passes.size() * sizeof(EvalPass)), o_pow = blob.take(n_queries * OPEN_POW * sizeof(Fu)),
                 o_qt = blob.take(n_queries * sizeof(uint32_t));
    Carve ws;
    const size_t o_blob = ws.take(blob.total), o_part = ws.take(n_queries * (size_t)max_tiles * sizeof(Fe));
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->open_ws.ensure(ws.total))) return rc;
    char* base = (char*)c->open_ws.p;
    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<EvalPass> pass = img.at<EvalPass>(o_pass);
    const Mirror<Fu> xpow = img.at<Fu>(o_pow);
    const Mirror<uint32_t> qt = img.at<uint32_t>(o_qt);
    memcpy(pass.h, passes.data(), passes.size() * sizeof(EvalPass));
    for (size_t q = 0; q < n_queries; q++) pow_table(points[q], xpow.h + q * OPEN_POW);
    memcpy(qt.h, qtiles.data(), n_queries * sizeof(uint32_t));
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;
    EvalParams P;
    P.xpow = xpow.d;
    P.partial = (Fe*)(base + o_part);
    P.R = R;
    P.B = B;
    P.logB = ilog2(B);
    P.max_tiles = max_tiles;
    int tm = c->timer_begin("opening_eval", s);
    for (size_t first = 0; first < passes.size();) {
        size_t end = first;
        while (end < passes.size() && passes[end].np == passes[first].np) end++;
        P.passes = pass.d + first;
        dim3 grid(max_tiles, (uint32_t)(end - first));
        switch (passes[first].np) {
#define OPEN_EVAL_CASE(N) \
    case N: hipLaunchKernelGGL(open_eval_kernel<N>, grid, dim3(B), 0, s, P); break;
            OPEN_EVAL_CASE(1) OPEN_EVAL_CASE(2) OPEN_EVAL_CASE(3) OPEN_EVAL_CASE(4)
            OPEN_EVAL_CASE(5) OPEN_EVAL_CASE(6) OPEN_EVAL_CASE(7) OPEN_EVAL_CASE(8)
#undef OPEN_EVAL_CASE
        }
        H2_CHECK(hipGetLastError());
        first = end;
    }
    hipLaunchKernelGGL(open_eval_sum_kernel, dim3((uint32_t)n_queries), dim3(OPEN_MAX_THREADS), 0, s, P.partial, qt.d, max_tiles, d_evals);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return guard.release();
}

// out[0 .. L - n_roots) = (or +=) scale * q; rem (device, 1 element) = a(roots[0]) when non-null.  polys: device pointers
static int combine_run(Ctx* c, const Fe* const* polys, uint64_t L, const Fe* scalars, size_t n_polys, const Fe* sub, size_t sub_len,
                       const Fe* roots, size_t n_roots, const Fe& scale, bool accumulate, Fe* d_out, bool want_rem, Fe* h_rem, hipStream_t s) {
    if (L == 0) return 0;  // (a remainder needs a root, so len >= 1)
    uint32_t R, B;
    open_shape(L, 16, &R, &B);
    const uint64_t T = (uint64_t)R * B;
    const uint64_t tiles = (L + T - 1) / T;
    if (tiles > 0x7fffffffull) {
        set_error("poly_combine: %llu tiles", (unsigned long long)tiles);
        return H2HIP_EINVAL;
    }
    // workspace: two scratch columns (one with a single root, none without), per-thread and per-tile carries, the remainder, the blob
    const size_t col = L * sizeof(Fe);
    Carve ws;
    const size_t o_x = ws.take(n_roots >= 1 ? col : 0), o_y = ws.take(n_roots >= 2 ? col : 0);  // a column that is not there is never touched
    const size_t o_thr = ws.take(tiles * B * sizeof(Fe)), o_tile = ws.take(tiles * sizeof(Fe)), o_rem = ws.take(sizeof(Fe));
    Carve blob;
    const size_t o_ptr = blob.take(n_polys * sizeof(void*)), o_scal = blob.take(2 * n_polys * sizeof(Fu)),
                 o_sub = blob.take(OPEN_MAX_SUB * sizeof(Fe)), o_pow = blob.take(std::max<size_t>(1, n_roots) * OPEN_POW * sizeof(Fu));
    const size_t o_blob = ws.take(blob.total);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->open_ws.ensure(ws.total))) return rc;
    char* base = (char*)c->open_ws.p;
    Fe* X = (Fe*)(base + o_x);
    Fe* Y = (Fe*)(base + o_y);
    Fe* d_rem = (Fe*)(base + o_rem);
    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<const Fe*> ptr = img.at<const Fe*>(o_ptr);
    const Mirror<Fu> scal = img.at<Fu>(o_scal), rpow = img.at<Fu>(o_pow);
    const Mirror<Fe> subs = img.at<Fe>(o_sub);
    memcpy(ptr.h, polys, n_polys * sizeof(void*));
    for (size_t j = 0; j < n_polys; j++) {
        scal.h[2 * j] = fu_from_ext(scalars[j]);
        scal.h[2 * j + 1] = fu_neg(scal.h[2 * j]);
    }
    if (sub_len) memcpy(subs.h, sub, sub_len * sizeof(Fe));
    for (size_t t = 0; t < n_roots; t++) pow_table(roots[t], rpow.h + t * OPEN_POW);
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;

    CombParams P;
    memset(&P, 0, sizeof(P));
    P.polys = ptr.d;
    P.scal = scal.d;
    P.sub = subs.d;
    P.thr = (Fe*)(base + o_thr);
    P.tile = (Fe*)(base + o_tile);
    P.n_polys = (uint32_t)n_polys;
    P.sub_len = (uint32_t)sub_len;
    P.R = R;
    P.B = B;
    P.logR = ilog2(R);
    P.logB = ilog2(B);
    P.accumulate = accumulate;
    Fe one = fe_one<FrP>(), s32 = scale;
    P.scale_one = fe_eq(scale, one);
    for (int b = 0; b < 5; b++) s32 = fe_add<FrP>(s32, s32);  // scale 2^261 mod p: canonical I-form
    P.scale = fu_slice(s32);
    int tm = c->timer_begin("opening_combine", s);
    if (n_roots == 0) {
        P.first = P.last = 1;
        P.L = L;
        P.out = d_out;
        hipLaunchKernelGGL(open_combine_kernel, dim3((uint32_t)((L + OPEN_MAX_THREADS - 1) / OPEN_MAX_THREADS)), dim3(OPEN_MAX_THREADS), 0, s, P);
        H2_CHECK(hipGetLastError());
    }
    for (size_t t = 0; t < n_roots; t++) {
        P.first = t == 0;
        P.last = t + 1 == n_roots;
        P.L = L - t;
        P.tiles = (uint32_t)((P.L + T - 1) / T);
        P.in = t == 0 ? nullptr : (t % 2 ? Y : X);
        P.w = t == 0 ? X : (Fe*)P.in;
        P.out = P.last ? d_out : (t % 2 ? X : Y);
        P.rem = t == 0 && want_rem ? d_rem : nullptr;
        P.rpow = rpow.d + t * OPEN_POW;
        uint32_t lp = 0;
        while (((uint64_t)OPEN_MAX_THREADS << lp) < P.tiles) lp++;
        P.log_per = lp;
        hipLaunchKernelGGL(open_scan_kernel, dim3(P.tiles), dim3(B), 0, s, P);
        H2_CHECK(hipGetLastError());
        hipLaunchKernelGGL(open_tiles_kernel, dim3(1), dim3(OPEN_MAX_THREADS), 0, s, P);
        H2_CHECK(hipGetLastError());
        hipLaunchKernelGGL(open_apply_kernel, dim3(P.tiles), dim3(B), 0, s, P);
        H2_CHECK(hipGetLastError());
    }
    c->timer_end(tm, s);
    if (want_rem && n_roots) {
        H2_CHECK(hipMemcpyAsync(h_rem, d_rem, sizeof(Fe), hipMemcpyDeviceToHost, s));
        H2_CHECK(hipStreamSynchronize(s));
    }
    return guard.release();
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "opening") ---------------------------------------------------------------------------------
static int eval_check(const void* const* polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly, const uint64_t* points,
                      size_t n_queries, const uint64_t* evals) {
    const char* what = "eval_polynomials";
    if (n_polys && !lens) {
        set_error("%s: null lens", what);
        return H2HIP_EINVAL;
    }
    for (size_t j = 0; j < n_polys; j++) {
        if (lens[j] > OPEN_MAX_LEN) {
            set_error("%s: lens[%zu] = %zu > 2^28", what, j, lens[j]);
            return H2HIP_EINVAL;
        }
        if (lens[j] && (!polys || !polys[j])) {
            set_error("%s: polys[%zu] is null", what, j);
            return H2HIP_EINVAL;
        }
    }
    if (n_queries && (!query_poly || !evals)) {
        set_error("%s: null query_poly or evals", what);
        return H2HIP_EINVAL;
    }
    if (n_queries > 0x7fffffffu) {
        set_error("%s: %zu queries", what, n_queries);
        return H2HIP_EINVAL;
    }
    for (size_t q = 0; q < n_queries; q++)
        if (query_poly[q] >= n_polys) {
            set_error("%s: query_poly[%zu] = %u out of range (%zu polynomials)", what, q, query_poly[q], n_polys);
            return H2HIP_EINVAL;
        }
    return check_frs(what, points, n_queries, "point");
}

static int eval_finish(Ctx* c, const Fe* const* d_polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly, const uint64_t* points,
                       size_t n_queries, uint64_t* evals, hipStream_t s) {
    std::vector<Fe> pts(n_queries);
    memcpy(pts.data(), points, n_queries * sizeof(Fe));
    int rc = c->open_io.ensure(align256(n_queries * sizeof(Fe)));
    if (rc) return rc;
    // open_io holds the evaluations of both forms (the host form's uploaded polynomials are in host_io): this form runs on any stream
    if ((rc = eval_run(c, d_polys, lens, n_polys, query_poly, pts.data(), n_queries, (Fe*)c->open_io.p, s))) return rc;
    H2_CHECK(hipMemcpyAsync(evals, c->open_io.p, n_queries * sizeof(Fe), hipMemcpyDeviceToHost, s));
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}

int h2hip_eval_polynomials_bn254_device(const void* const* d_polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly,
                                        const uint64_t* points, size_t n_queries, uint64_t* evals, void* stream) {
    if (int rc = eval_check(d_polys, lens, n_polys, query_poly, points, n_queries, evals)) return rc;
    if (n_queries == 0) return 0;
    const void* any = nullptr;
    for (size_t j = 0; j < n_polys && !any; j++) any = lens[j] ? d_polys[j] : nullptr;
    Entry en("h2hip_eval_polynomials_bn254_device", any);
    if (en.rc) return en.rc;
    std::vector<const Fe*> p(n_polys);
    for (size_t j = 0; j < n_polys; j++) p[j] = (const Fe*)d_polys[j];
    return eval_finish(en.c, p.data(), lens, n_polys, query_poly, points, n_queries, evals, (hipStream_t)stream);
}

int h2hip_eval_polynomials_bn254(const uint64_t* const* polys, const size_t* lens, size_t n_polys, const uint32_t* query_poly,
                                 const uint64_t* points, size_t n_queries, uint64_t* evals) {
    if (int rc = eval_check((const void* const*)polys, lens, n_polys, query_poly, points, n_queries, evals)) return rc;
    if (n_queries == 0) return 0;
    Entry en("h2hip_eval_polynomials_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    // upload the queried polynomials that are not pinned (h2hip_columns_pin), each once
    std::vector<char> queried(n_polys, 0);
    for (size_t q = 0; q < n_queries; q++) queried[query_poly[q]] = 1;
    std::vector<const Fe*> d(n_polys, nullptr);
    HostIo io(c, c->host_io, s, true);
    for (size_t j = 0; j < n_polys; j++)
        if (queried[j] && lens[j]) io.in(polys[j], lens[j] * sizeof(Fe), &d[j], true);
    if (int rc = io.upload()) return rc;
    if (int rc = eval_finish(c, d.data(), lens, n_polys, query_poly, points, n_queries, evals, s)) return rc;
    return io.finish();
}

static int combine_check(const void* const* polys, size_t len, const uint64_t* scalars, size_t n_polys, const uint64_t* sub, size_t sub_len,
                         const uint64_t* roots, size_t n_roots, const uint64_t* scale, const void* out, size_t out_len, const uint64_t* remainder) {
    const char* what = "poly_combine";
    if (len > OPEN_MAX_LEN) {
        set_error("%s: len = %zu > 2^28", what, len);
        return H2HIP_EINVAL;
    }
    if (n_roots > OPEN_MAX_ROOTS) {
        set_error("%s: %zu roots > %d", what, n_roots, OPEN_MAX_ROOTS);
        return H2HIP_EINVAL;
    }
    if (len < n_roots) {
        set_error("%s: len = %zu < %zu roots", what, len, n_roots);
        return H2HIP_EINVAL;
    }
    if (sub_len > std::min<size_t>(len, OPEN_MAX_SUB)) {
        set_error("%s: sub_len = %zu > min(len, %d)", what, sub_len, OPEN_MAX_SUB);
        return H2HIP_EINVAL;
    }
    if (out_len < len - n_roots) {
        set_error("%s: out_len = %zu < len - n_roots = %zu", what, out_len, len - n_roots);
        return H2HIP_EINVAL;
    }
    if (out_len > OPEN_MAX_LEN) {
        set_error("%s: out_len = %zu > 2^28", what, out_len);
        return H2HIP_EINVAL;
    }
    if (remainder && n_roots == 0) {
        set_error("%s: a remainder needs a root", what);
        return H2HIP_EINVAL;
    }
    if (out_len && !out) {
        set_error("%s: null out", what);
        return H2HIP_EINVAL;
    }
    if (!scale) {
        set_error("%s: null scale", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(scale, "scale")) return H2HIP_EINVAL;
    if (check_frs(what, scalars, n_polys, "scalar") || check_frs(what, sub, sub_len, "sub") ||
        check_frs(what, roots, n_roots, "root"))
        return H2HIP_EINVAL;
    if (len && check_ptrs(what, polys, n_polys, "polys")) return H2HIP_EINVAL;
    for (size_t j = 0; j < n_polys && len; j++)
        if (polys[j] == out) {
            set_error("%s: out aliases polys[%zu]", what, j);
            return H2HIP_EINVAL;
        }
    return 0;
}

int h2hip_poly_combine_bn254_fr_device(const void* const* d_polys, size_t len, const uint64_t* scalars, size_t n_polys, const uint64_t* sub,
                                       size_t sub_len, const uint64_t* roots, size_t n_roots, const uint64_t scale[4], uint32_t accumulate,
                                       void* d_out, size_t out_len, uint64_t* remainder, void* stream) {
    if (int rc = combine_check(d_polys, len, scalars, n_polys, sub, sub_len, roots, n_roots, scale, d_out, out_len, remainder)) return rc;
    if (n_polys == 0) return 0;
    Entry en("h2hip_poly_combine_bn254_fr_device", d_out);
    if (en.rc) return en.rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t Lout = len - n_roots;
    if (!accumulate && out_len > Lout) H2_CHECK(hipMemsetAsync((Fe*)d_out + Lout, 0, (out_len - Lout) * sizeof(Fe), s));
    std::vector<Fe> h_rem(1);
    int rc = combine_run(en.c, (const Fe* const*)d_polys, len, (const Fe*)scalars, n_polys, (const Fe*)sub, sub_len, (const Fe*)roots, n_roots,
                         fe_from_u64x4(scale), accumulate != 0, (Fe*)d_out, remainder != nullptr, h_rem.data(), s);
    if (rc) return rc;
    if (remainder) memcpy(remainder, h_rem.data(), sizeof(Fe));
    return 0;
}

int h2hip_poly_combine_bn254_fr(const uint64_t* const* polys, size_t len, const uint64_t* scalars, size_t n_polys, const uint64_t* sub,
                                size_t sub_len, const uint64_t* roots, size_t n_roots, const uint64_t scale[4], uint32_t accumulate, uint64_t* out,
                                size_t out_len, uint64_t* remainder) {
    if (int rc = combine_check((const void* const*)polys, len, scalars, n_polys, sub, sub_len, roots, n_roots, scale, out, out_len, remainder))
        return rc;
    if (n_polys == 0) return 0;
    const size_t Lout = len - n_roots;
    if (accumulate)
        for (size_t i = 0; i < Lout; i++)
            if (check_fr(out + 4 * i, "out (accumulator)")) return H2HIP_EINVAL;
    Entry en("h2hip_poly_combine_bn254_fr");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    std::vector<const Fe*> d(n_polys, nullptr);
    Fe* d_out = nullptr;
    HostIo io(c, c->host_io, s, true);
    const size_t o_out = io.room(len * sizeof(Fe), &d_out);  // the output first
    for (size_t j = 0; j < n_polys; j++)
        if (len) io.in(polys[j], len * sizeof(Fe), &d[j], true);
    if (accumulate) io.in_at(out, Lout * sizeof(Fe), o_out);
    io.out_at(out, Lout * sizeof(Fe), o_out);
    int rc = io.upload();
    if (rc) return rc;
    std::vector<Fe> h_rem(1);
    rc = combine_run(c, d.data(), len, (const Fe*)scalars, n_polys, (const Fe*)sub, sub_len, (const Fe*)roots, n_roots, fe_from_u64x4(scale),
                     accumulate != 0, d_out, remainder != nullptr, h_rem.data(), s);
    if (rc) return rc;
    if ((rc = io.finish())) return rc;
    if (!accumulate && out_len > Lout) memset(out + 4 * Lout, 0, (out_len - Lout) * sizeof(Fe));
    if (remainder) memcpy(remainder, h_rem.data(), sizeof(Fe));
    return 0;
}

int h2hip_debug_set_opening_tile(uint32_t rows_per_thread, uint32_t threads_per_tile) {
    const bool pow2_r = rows_per_thread == 0 || (rows_per_thread <= 64 && !(rows_per_thread & (rows_per_thread - 1)));
    const bool pow2_b = threads_per_tile == 0 || (threads_per_tile <= OPEN_MAX_THREADS && !(threads_per_tile & (threads_per_tile - 1)));
    if (!pow2_r || !pow2_b) {
        set_error("debug_set_opening_tile: rows per thread (<= 64) and threads per tile (<= %d) must be powers of two or 0", OPEN_MAX_THREADS);
        return H2HIP_EINVAL;
    }
    TuneWrite t;
    t->open_rows = rows_per_thread;
    t->open_threads = threads_per_tile;
    return 0;
}

}  // extern "C"
