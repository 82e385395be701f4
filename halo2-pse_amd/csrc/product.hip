// product.hip -- the grand-product columns z of the permutation and lookup arguments, and ff's BatchInvert, on the GPU.
//
// Replaces the host loops of create_proof between the advice commits and evaluate_h:
//   permutation::Argument::commit   (plonk/permutation/prover.rs:96-166): per set of chunk_len columns
//       mv_i = prod_c (p_c[i] + beta delta^c omega^i + gamma) * inv(prod_c (p_c[i] + beta s_c[i] + gamma)),
//       z[0] = last_z, z[i] = z[i-1] mv_{i-1}, blinding rows, last_z = z[u] carried into the next set;
//   lookup::Permuted::commit_product (plonk/lookup/prover.rs:194-249): the same with
//       lp_i = (A_i + beta)(S_i + gamma) * inv((A'_i + beta)(S'_i + gamma)), z[0] = 1;
//   shuffle::Argument::commit_product (upstream PSE halo2, later than the reference: DESIGN.md §2): the same with
//       sp_i = (A_i + gamma) * inv(S_i + gamma), z[0] = 1;
//   the logUp (mv-lookup) argument's grand sum (later than the reference too: DESIGN.md §2), additive where those are products:
//       phi[0] = 0, phi[i] = phi[i-1] + sum_c inv(F_c[i-1] + beta) - M[i-1] inv(T[i-1] + beta) -- its kernels are mvs_* below;
//   ff::BatchInvert (prover.rs:117, lookup/prover.rs:208), where a zero stays zero.
//
// Plan (Grand products).  With e_0 = 1, e_i = num_{i-1} and d_i = den_i (d_u = 1), every z row i <= u is
//     z[i] = last_z * (prod_{t<=i} e_t) * (prod_{t>=i} d'_t) * inv(prod_t d'_t) * [i <= j0]
// where d' is d with zeros read as one and j0 is the first row < u whose denominator is zero (u if none): before j0 this is
// prod_{t<i} num_t / den_t, after it ff's zero-skipping inversion has made a factor zero.  So a whole argument needs ONE field
// inversion, a forward product scan of e and a backward one of d, all reduce-then-scan with no inter-workgroup waiting:
//   1. prod_fraction_kernel  (tiles x arguments): e -> z, d -> w, per-thread and per-tile products, atomicMin of j0;
//   2. prod_tiles_kernel     (one workgroup per argument): exclusive scans of the tile products in both directions, the
//                            inversion (binary extended Euclid in one lane; the kernel takes 0.17-0.29 ms, measured, and is
//                            the floor of a small call: DESIGN.md §5, Grand products), the argument's end value z[u] / last_z;
//   3. prod_apply_kernel     (tiles x arguments): the set chain (last_z = product of the earlier sets' end values, read on
//                            the device), the local scans, the final products, zeros after j0, the blinding rows.
// BatchInvert is the same with exclusive scans of one array: inv(a_i) = prod_{t<i} a'_t * prod_{t>i} a'_t * inv(prod a').
#include <string.h>
#include <vector>
#include "engine.h"
#include "fe_io.h"

namespace h2 {

#define PROD_THREADS 256

struct ProdDesc {         // one argument (permutation set, lookup, or the array of a batch inversion)
    Fe* z;                // output column (2^k); also holds e while the kernels run
    const Fe* e;          // array the forward scan reads: z (products) or w (inversion)
    Fe* w;                // d, L elements of scratch
    Fe* thr_e;            // per-thread products, tiles x PROD_THREADS each
    Fe* thr_d;
    Fe* tile_e;           // per-tile products, then their exclusive scans
    Fe* tile_d;
    Fe* meta;             // [0] = inv(prod d'), [1] = end value z[u] / last_z
    uint32_t* j0;
    const Fe* const* p;   // permutation: the set's columns p_c; lookup: {A, S}; shuffle: {A}
    const Fe* const* s;   // permutation: the set's s_c; lookup: {A', S'}; shuffle: {S}
    const Fe* blind;      // blinding_factors values for rows n - b .. n - 1
    uint32_t ncols;       // columns in the set
    uint32_t col0;        // global index of the set's first column (delta^c)
    uint32_t chain_first; // first argument of this one's chain (the permutation sets), == own index otherwise
    uint32_t pad;
};

struct ProdParams {
    uint64_t n;           // rows of a column
    uint64_t L;           // indices scanned: u + 1 (products) or n (inversion)
    uint64_t u;           // last computed row (products)
    uint32_t R;           // consecutive indices per thread
    uint32_t tiles;       // tiles per argument
    uint32_t bf;          // blinding factors
    uint32_t pad;
    Fe beta, gamma;
    const Fe* omega_pow2; // omega^(2^b), b < 32 (permutation)
    const Fe* delta_pow;  // delta^c, c < n_columns (permutation)
};

enum { PROD_PERM = 0, PROD_LOOKUP = 1, PROD_INVERT = 2, PROD_SHUFFLE = 3 };

__device__ __forceinline__ Fe prod_one() { return fe_one<FrP>(); }
__device__ __forceinline__ Fe prod_nz(const Fe& x) { return fe_is_zero(x) ? prod_one() : x; }

// ---- inversion: binary extended Euclid (Guide to ECC, Alg. 2.22) on the canonical integer, one lane ----------------------
H2_HD bool big_is_one(const Fe& a) {
    uint32_t x = a.l[0] ^ 1u;
#pragma unroll
    for (int i = 1; i < 8; i++) x |= a.l[i];
    return x == 0;
}
H2_HD bool big_geq(const Fe& a, const Fe& b) {
    for (int i = 7; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
    return true;
}
H2_HD void big_sub(Fe& a, const Fe& b) {  // a -= b, a >= b
    uint32_t br = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint64_t d = (uint64_t)a.l[j] - b.l[j] - br;
        a.l[j] = (uint32_t)d;
        br = (uint32_t)(d >> 63);
    }
}
H2_HD void big_shr1(Fe& a) {
#pragma unroll
    for (int j = 0; j < 7; j++) a.l[j] = (a.l[j] >> 1) | (a.l[j + 1] << 31);
    a.l[7] >>= 1;
}
// x / 2 mod r for x < r (r odd, r < 2^254: x + r does not overflow)
H2_HD void half_mod(Fe& x) {
    if (x.l[0] & 1) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t s = (uint64_t)x.l[j] + FrP::MOD[j] + c;
            x.l[j] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
    }
    big_shr1(x);
}
// Montgomery a R -> a^-1 R; 0 -> 0
H2_HD Fe fr_inv_binary(const Fe& a) {
    if (fe_is_zero(a)) return a;
    Fe u = a, v, x1 = fe_zero<FrP>(), x2 = fe_zero<FrP>();
#pragma unroll
    for (int j = 0; j < 8; j++) v.l[j] = FrP::MOD[j];
    x1.l[0] = 1;
    while (!big_is_one(u) && !big_is_one(v)) {
        while (!(u.l[0] & 1)) {
            big_shr1(u);
            half_mod(x1);
        }
        while (!(v.l[0] & 1)) {
            big_shr1(v);
            half_mod(x2);
        }
        if (big_geq(u, v)) {
            big_sub(u, v);
            x1 = fe_sub<FrP>(x1, x2);
        } else {
            big_sub(v, u);
            x2 = fe_sub<FrP>(x2, x1);
        }
    }
    Fe y = big_is_one(u) ? x1 : x2;  // (a R)^-1 as an integer; times R^3 / R gives a^-1 R
    Fe r2;
#pragma unroll
    for (int j = 0; j < 8; j++) r2.l[j] = FrP::R2[j];
    return fe_mul<FrP>(y, fe_mul<FrP>(r2, r2));
}

// ---- block-wide helpers (PROD_THREADS threads) ----------------------------------------------------------------------------
// inclusive product scan over the threads in order (rev: from the last thread down); lds holds PROD_THREADS elements
__device__ Fe block_scan_incl(Fe v, Fe* lds, bool rev) {
    const uint32_t t = threadIdx.x, pos = rev ? PROD_THREADS - 1 - t : t;
    lds[pos] = v;
    __syncthreads();
    for (uint32_t off = 1; off < PROD_THREADS; off <<= 1) {
        Fe o = pos >= off ? lds[pos - off] : prod_one();
        __syncthreads();
        v = fe_mul<FrP>(v, o);
        lds[pos] = v;
        __syncthreads();
    }
    return v;
}
// exclusive form: the product of the threads strictly before (rev: after) this one; *total = product of all
__device__ Fe block_scan_excl(Fe v, Fe* lds, bool rev, Fe* total) {
    const uint32_t t = threadIdx.x, pos = rev ? PROD_THREADS - 1 - t : t;
    Fe inc = block_scan_incl(v, lds, rev);
    Fe ex = pos ? lds[pos - 1] : prod_one();
    if (total) *total = lds[PROD_THREADS - 1];
    __syncthreads();
    (void)inc;
    return ex;
}

// ---- 1. e and d, per-thread and per-tile products ------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(PROD_THREADS) void prod_fraction_kernel(const ProdDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const ProdDesc D = descs[blockIdx.y];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t i0 = ((uint64_t)tile * PROD_THREADS + tid) * P.R;
    const Fe one = prod_one();
    Fe pe = one, pd = one;
    if (i0 < P.L) {
        const uint64_t i1 = i0 + P.R < P.L ? i0 + P.R : P.L;
        if (KIND == PROD_INVERT) {
            for (uint64_t i = i0; i < i1; i++) {
                Fe a = fe_ld(D.z, i);
                fe_st(D.w, i, a);
                pe = fe_mul<FrP>(pe, prod_nz(a));
            }
            pd = pe;
        } else {
            Fe bw = P.beta;  // beta omega^(i - 1) for the numerator of index i (row i - 1)
            if (KIND == PROD_PERM && i0 > 0) {
                const uint64_t t0 = i0 - 1;
                Fe w = one;
                for (int b = 0; b < 32; b++)
                    if ((t0 >> b) & 1) w = fe_mul<FrP>(w, P.omega_pow2[b]);
                bw = fe_mul<FrP>(bw, w);
            }
            const Fe omega = P.omega_pow2[0];
            uint32_t zmin = 0xffffffffu;
            for (uint64_t i = i0; i < i1; i++) {
                Fe e = one, d = one;
                if (i > 0) {  // e_i = num_{i-1}
                    const uint64_t t = i - 1;
                    if (KIND == PROD_PERM) {
                        for (uint32_t c = 0; c < D.ncols; c++) {
                            Fe f = fe_add<FrP>(fe_add<FrP>(fe_ld(D.p[c], t), fe_mul<FrP>(bw, P.delta_pow[D.col0 + c])), P.gamma);
                            e = c ? fe_mul<FrP>(e, f) : f;
                        }
                        bw = fe_mul<FrP>(bw, omega);
                    } else if (KIND == PROD_SHUFFLE) {
                        e = fe_add<FrP>(fe_ld(D.p[0], t), P.gamma);
                    } else {
                        e = fe_mul<FrP>(fe_add<FrP>(fe_ld(D.p[0], t), P.beta), fe_add<FrP>(fe_ld(D.p[1], t), P.gamma));
                    }
                }
                if (i < P.u) {  // d_i = den_i
                    if (KIND == PROD_PERM) {
                        for (uint32_t c = 0; c < D.ncols; c++) {
                            Fe f = fe_add<FrP>(fe_add<FrP>(fe_ld(D.p[c], i), fe_mul<FrP>(P.beta, fe_ld(D.s[c], i))), P.gamma);
                            d = c ? fe_mul<FrP>(d, f) : f;
                        }
                    } else if (KIND == PROD_SHUFFLE) {
                        d = fe_add<FrP>(fe_ld(D.s[0], i), P.gamma);
                    } else {
                        d = fe_mul<FrP>(fe_add<FrP>(fe_ld(D.s[0], i), P.beta), fe_add<FrP>(fe_ld(D.s[1], i), P.gamma));
                    }
                    if (fe_is_zero(d) && zmin == 0xffffffffu) zmin = (uint32_t)i;
                }
                fe_st(D.z, i, e);
                fe_st(D.w, i, d);
                pe = fe_mul<FrP>(pe, e);
                pd = fe_mul<FrP>(pd, prod_nz(d));
            }
            if (zmin != 0xffffffffu) atomicMin(D.j0, zmin);
        }
    }
    const uint64_t ti = (uint64_t)tile * PROD_THREADS + tid;
    fe_st(D.thr_e, ti, pe);
    fe_st(D.thr_d, ti, pd);
    // tile products: a tree over the threads
    Fe te, td;
    lds[tid] = pe;
    __syncthreads();
    for (uint32_t h = PROD_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) lds[tid] = fe_mul<FrP>(lds[tid], lds[tid + h]);
        __syncthreads();
    }
    te = lds[0];
    __syncthreads();
    lds[tid] = pd;
    __syncthreads();
    for (uint32_t h = PROD_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) lds[tid] = fe_mul<FrP>(lds[tid], lds[tid + h]);
        __syncthreads();
    }
    td = lds[0];
    if (tid == 0) {
        fe_st(D.tile_e, tile, te);
        fe_st(D.tile_d, tile, td);
    }
}

// ---- 2. scans of the tile products, the inversion, the end value ---------------------------------------------------------
__global__ __launch_bounds__(PROD_THREADS) void prod_tiles_kernel(const ProdDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const ProdDesc D = descs[blockIdx.x];
    const uint32_t tid = threadIdx.x, T = P.tiles;
    Fe carry_e = prod_one(), carry_d = prod_one(), tot;
    for (uint32_t base = 0; base < T; base += PROD_THREADS) {  // forward, exclusive
        const uint32_t j = base + tid;
        Fe v = j < T ? fe_ld(D.tile_e, j) : prod_one();
        Fe ex = block_scan_excl(v, lds, false, &tot);
        if (j < T) fe_st(D.tile_e, j, fe_mul<FrP>(carry_e, ex));
        carry_e = fe_mul<FrP>(carry_e, tot);
    }
    for (uint32_t base = 0; base < T; base += PROD_THREADS) {  // backward, exclusive: chunks from the last tile down
        const int64_t j = (int64_t)T - 1 - base - (PROD_THREADS - 1 - tid);  // thread order == tile order inside the chunk
        Fe v = j >= 0 ? fe_ld(D.tile_d, (uint64_t)j) : prod_one();
        Fe ex = block_scan_excl(v, lds, true, &tot);
        if (j >= 0) fe_st(D.tile_d, (uint64_t)j, fe_mul<FrP>(carry_d, ex));
        carry_d = fe_mul<FrP>(carry_d, tot);
    }
    if (tid == 0) {
        Fe inv = fr_inv_binary(carry_d);  // prod d' is never zero
        fe_st(D.meta, 0, inv);
        Fe end = fe_mul<FrP>(carry_e, inv);  // z[u] / last_z = prod_{t<u} num_t / den_t while no denominator is zero
        if (*D.j0 != (uint32_t)P.u) end = fe_zero<FrP>();
        fe_st(D.meta, 1, end);
    }
}

// ---- 3. final values ----------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(PROD_THREADS) void prod_apply_kernel(const ProdDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const uint32_t a = blockIdx.y;
    const ProdDesc D = descs[a];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t ti = (uint64_t)tile * PROD_THREADS + tid;
    Fe scale = fe_ld(D.meta, 0);
    uint64_t j0 = P.L;
    if (KIND != PROD_INVERT) {
        for (uint32_t s = D.chain_first; s < a; s++) scale = fe_mul<FrP>(scale, fe_ld(descs[s].meta, 1));  // last_z
        j0 = *D.j0;
    }
    Fe fwd = fe_mul<FrP>(fe_ld(D.tile_e, tile), block_scan_excl(fe_ld(D.thr_e, ti), lds, false, nullptr));
    Fe bwd = fe_mul<FrP>(fe_ld(D.tile_d, tile), block_scan_excl(fe_ld(D.thr_d, ti), lds, true, nullptr));
    const uint64_t i0 = ti * P.R;
    if (i0 < P.L) {
        const uint64_t i1 = i0 + P.R < P.L ? i0 + P.R : P.L;
        for (uint64_t i = i0; i < i1; i++) {  // forward: prefix of e (inclusive for the products, exclusive for the inversion)
            Fe e = fe_ld(D.e, i);
            if (KIND == PROD_INVERT) {
                fe_st(D.z, i, fwd);
                fwd = fe_mul<FrP>(fwd, prod_nz(e));
            } else {
                fwd = fe_mul<FrP>(fwd, e);
                fe_st(D.z, i, fwd);
            }
        }
        for (uint64_t i = i1; i-- > i0;) {  // backward: suffix of d', the scale, the zero rule
            Fe d = fe_ld(D.w, i);
            Fe v;
            if (KIND == PROD_INVERT) {
                v = fe_mul<FrP>(fe_mul<FrP>(fe_ld(D.z, i), bwd), scale);
                bwd = fe_mul<FrP>(bwd, prod_nz(d));
                if (fe_is_zero(d)) v = fe_zero<FrP>();
            } else {
                bwd = fe_mul<FrP>(bwd, prod_nz(d));
                v = fe_mul<FrP>(fe_mul<FrP>(fe_ld(D.z, i), bwd), scale);
                if (i > j0) v = fe_zero<FrP>();
            }
            fe_st(D.z, i, v);
        }
    }
    if (KIND != PROD_INVERT && tile == 0)
        for (uint32_t j = tid; j < P.bf; j += PROD_THREADS) fe_st(D.z, P.u + 1 + j, D.blind[j]);
}

// ---- the logUp (mv-lookup) argument's grand sum (include/halo2hip.h, h2hip_mvlookup_sums_bn254) ----------------------------
// phi[0] = 0, phi[i] = phi[i-1] + sum_c inv(F_c[i-1] + beta) - M[i-1] inv(T[i-1] + beta) for 1 <= i <= u.  Plan (DESIGN.md §5,
// mv-lookup): every denominator of the call -- (K_j + 1) u per argument -- goes into one array, which the PROD_INVERT path above
// inverts with ONE field inversion (a zero stays zero, so that term drops out and the sum goes on); then an additive reduce-then-scan
// with the products' three stages and no inter-workgroup waiting:
//   mvs_sum_kernel    (tiles x arguments): the terms of R consecutive rows per thread, per-thread and per-tile sums;
//   mvs_tiles_kernel  (one workgroup per argument): exclusive scan of the tile sums;
//   mvs_apply_kernel  (tiles x arguments): phi rows 0 .. u from the prefixes (the terms are formed again: K + 1 loads and one product
//                     are cheaper than a column of terms written and read), the blinding rows.
struct MvSumDesc {        // one argument
    const Fe* inv;        // the inverted denominators: input c at inv + c u, the table at inv + K u
    const Fe* m;          // multiplicities (2^k)
    Fe* phi;              // output column (2^k)
    Fe* thr;              // per-thread sums, tiles x PROD_THREADS
    Fe* tile;             // per-tile sums, then their exclusive scan
    const Fe* blind;      // blinding_factors values for rows n - b .. n - 1
    uint32_t K;           // input columns
    uint32_t pad;
};
struct MvDenCol {         // one column of denominators
    const Fe* col;
    Fe* out;
};

__global__ __launch_bounds__(PROD_THREADS) void mvs_den_kernel(const MvDenCol* cols, uint64_t u, Fe beta) {
    const MvDenCol C = cols[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * PROD_THREADS + threadIdx.x;
    if (i < u) fe_st(C.out, i, fe_add<FrP>(fe_ld(C.col, i), beta));
}

__device__ __forceinline__ Fe mvs_term(const MvSumDesc& D, uint64_t u, uint64_t i) {
    Fe t = fe_ld(D.inv, i);
    for (uint32_t c = 1; c < D.K; c++) t = fe_add<FrP>(t, fe_ld(D.inv, c * u + i));
    return fe_sub<FrP>(t, fe_mul<FrP>(fe_ld(D.m, i), fe_ld(D.inv, D.K * u + i)));
}

// exclusive sum over the threads in order; *total = sum of all; lds holds PROD_THREADS elements
__device__ Fe block_sum_excl(Fe v, Fe* lds, Fe* total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < PROD_THREADS; off <<= 1) {
        Fe o = t >= off ? lds[t - off] : fe_zero<FrP>();
        __syncthreads();
        v = fe_add<FrP>(v, o);
        lds[t] = v;
        __syncthreads();
    }
    Fe ex = t ? lds[t - 1] : fe_zero<FrP>();
    if (total) *total = lds[PROD_THREADS - 1];
    __syncthreads();
    return ex;
}

// P.L = u + 1 indices (the rows of phi the scan writes); index i < u carries the term of row i
__global__ __launch_bounds__(PROD_THREADS) void mvs_sum_kernel(const MvSumDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const MvSumDesc D = descs[blockIdx.y];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t ti = (uint64_t)tile * PROD_THREADS + tid, i0 = ti * P.R;
    Fe sum = fe_zero<FrP>();
    if (i0 < P.u) {
        const uint64_t i1 = i0 + P.R < P.u ? i0 + P.R : P.u;
        for (uint64_t i = i0; i < i1; i++) sum = fe_add<FrP>(sum, mvs_term(D, P.u, i));
    }
    fe_st(D.thr, ti, sum);
    lds[tid] = sum;
    __syncthreads();
    for (uint32_t h = PROD_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) lds[tid] = fe_add<FrP>(lds[tid], lds[tid + h]);
        __syncthreads();
    }
    if (tid == 0) fe_st(D.tile, tile, lds[0]);
}

__global__ __launch_bounds__(PROD_THREADS) void mvs_tiles_kernel(const MvSumDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const MvSumDesc D = descs[blockIdx.x];
    const uint32_t tid = threadIdx.x, T = P.tiles;
    Fe carry = fe_zero<FrP>(), tot;
    for (uint32_t base = 0; base < T; base += PROD_THREADS) {
        const uint32_t j = base + tid;
        Fe ex = block_sum_excl(j < T ? fe_ld(D.tile, j) : fe_zero<FrP>(), lds, &tot);
        if (j < T) fe_st(D.tile, j, fe_add<FrP>(carry, ex));
        carry = fe_add<FrP>(carry, tot);
    }
}

__global__ __launch_bounds__(PROD_THREADS) void mvs_apply_kernel(const MvSumDesc* descs, ProdParams P) {
    __shared__ Fe lds[PROD_THREADS];
    const MvSumDesc D = descs[blockIdx.y];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t ti = (uint64_t)tile * PROD_THREADS + tid, i0 = ti * P.R;
    Fe acc = fe_add<FrP>(fe_ld(D.tile, tile), block_sum_excl(fe_ld(D.thr, ti), lds, nullptr));
    if (i0 < P.L) {
        const uint64_t i1 = i0 + P.R < P.L ? i0 + P.R : P.L;
        for (uint64_t i = i0; i < i1; i++) {
            fe_st(D.phi, i, acc);
            if (i < P.u) acc = fe_add<FrP>(acc, mvs_term(D, P.u, i));
        }
    }
    if (tile == 0)
        for (uint32_t j = tid; j < P.bf; j += PROD_THREADS) fe_st(D.phi, P.u + 1 + j, D.blind[j]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static uint32_t prod_rows_per_thread(uint64_t L, size_t n_args) {
    // about 2^17 threads in flight over all arguments (8 waves per CU): fewer rows per thread when the call is small
    uint64_t want = (L * n_args) >> 17;
    uint32_t R = 1;
    while (R < 16 && (uint64_t)R * 2 <= want) R *= 2;
    return R;
}

// kind: PROD_PERM / PROD_LOOKUP / PROD_INVERT / PROD_SHUFFLE.  cols / perms: host arrays of device pointers (for lookups cols[2j],
// cols[2j + 1] = A, S and perms[2j], perms[2j + 1] = A', S' of lookup j; for shuffles cols[j] = A, perms[j] = S of shuffle j).  n_args outputs z[a] (2^k or n elements, device).  Enqueued on s.
static int products_run(Ctx* c, int kind, uint64_t n, uint64_t L, uint64_t u, const Fe& omega, const Fe& delta, const Fe& beta,
                        const Fe& gamma, const Fe* const* cols, const Fe* const* perms, uint32_t n_columns, uint32_t chunk_len,
                        size_t n_args, const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s) {
    if (n_args == 0 || L == 0) return 0;
    const uint32_t R = prod_rows_per_thread(L, n_args);
    const uint64_t tile_rows = (uint64_t)PROD_THREADS * R;
    const uint64_t tiles = (L + tile_rows - 1) / tile_rows;
    if (tiles > 65535u * 256u) {
        set_error("products: %llu tiles", (unsigned long long)tiles);
        return H2HIP_EINVAL;
    }
    // one argument's workspace: w (L), per-thread products (2 x tiles x 256), tile products (2 x tiles), meta (2)
    Carve arg;
    const size_t o_w = arg.take(L * sizeof(Fe));
    const size_t o_thr_e = arg.take(tiles * PROD_THREADS * sizeof(Fe)), o_thr_d = arg.take(tiles * PROD_THREADS * sizeof(Fe));
    const size_t o_tile_e = arg.take(tiles * sizeof(Fe)), o_tile_d = arg.take(tiles * sizeof(Fe));
    const size_t o_meta = arg.take(2 * sizeof(Fe));
    // the blob the kernels read: descriptors, pointer tables, omega^(2^b), delta^c, blinding
    const size_t n_ptr = kind == PROD_PERM ? 2 * (size_t)n_columns : kind == PROD_LOOKUP ? 4 * n_args : kind == PROD_SHUFFLE ? 2 * n_args : 0;
    const size_t n_delta = kind == PROD_PERM ? n_columns : 0;
    Carve blob;
    const size_t o_desc = blob.take(n_args * sizeof(ProdDesc));
    const size_t o_ptr = blob.take(n_ptr * sizeof(void*));
    const size_t o_fe = blob.take((32 + n_delta + n_args * (size_t)bf) * sizeof(Fe));
    // the call's workspace: every argument's, the j0 words, the blob
    Carve ws;
    const size_t o_args = ws.take(n_args * arg.total), o_j0 = ws.take(n_args * sizeof(uint32_t)), o_blob = ws.take(blob.total);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->prod_ws.ensure(ws.total))) return rc;
    char* base = (char*)c->prod_ws.p;
    uint32_t* d_j0 = (uint32_t*)(base + o_j0);

    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<ProdDesc> desc = img.at<ProdDesc>(o_desc);
    const Mirror<const Fe*> ptr = img.at<const Fe*>(o_ptr);
    const Mirror<Fe> fe = img.at<Fe>(o_fe);
    Fe w = omega;
    for (int b = 0; b < 32; b++) {  // omega^(2^b)
        fe.h[b] = w;
        w = fe_mul<FrP>(w, w);
    }
    Fe dl = fe_one<FrP>();
    for (size_t c2 = 0; c2 < n_delta; c2++) {
        fe.h[32 + c2] = dl;
        dl = fe_mul<FrP>(dl, delta);
    }
    if (bf) memcpy(fe.h + 32 + n_delta, blinding, n_args * (size_t)bf * sizeof(Fe));
    for (size_t a = 0; a < n_args; a++) {
        ProdDesc& D = desc.h[a];
        char* ab = base + o_args + a * arg.total;
        D.z = z[a];
        D.w = (Fe*)(ab + o_w);
        D.e = kind == PROD_INVERT ? D.w : D.z;
        D.thr_e = (Fe*)(ab + o_thr_e);
        D.thr_d = (Fe*)(ab + o_thr_d);
        D.tile_e = (Fe*)(ab + o_tile_e);
        D.tile_d = (Fe*)(ab + o_tile_d);
        D.meta = (Fe*)(ab + o_meta);
        D.j0 = d_j0 + a;
        D.blind = fe.d + 32 + n_delta + a * (size_t)bf;
        D.chain_first = kind == PROD_PERM ? 0 : (uint32_t)a;
        if (kind == PROD_PERM) {
            D.col0 = (uint32_t)(a * chunk_len);
            D.ncols = (uint32_t)(n_columns - D.col0 < chunk_len ? n_columns - D.col0 : chunk_len);
            D.p = ptr.d + D.col0;
            D.s = ptr.d + n_columns + D.col0;
        } else if (kind == PROD_LOOKUP) {
            D.ncols = 2;
            D.p = ptr.d + 4 * a;
            D.s = ptr.d + 4 * a + 2;
        } else if (kind == PROD_SHUFFLE) {
            D.ncols = 1;
            D.p = ptr.d + 2 * a;
            D.s = ptr.d + 2 * a + 1;
        }
    }
    if (kind == PROD_PERM) {
        for (uint32_t j = 0; j < n_columns; j++) {
            ptr.h[j] = cols[j];
            ptr.h[n_columns + j] = perms[j];
        }
    } else if (kind == PROD_LOOKUP) {
        for (size_t a = 0; a < n_args; a++) {
            ptr.h[4 * a] = cols[2 * a];
            ptr.h[4 * a + 1] = cols[2 * a + 1];
            ptr.h[4 * a + 2] = perms[2 * a];
            ptr.h[4 * a + 3] = perms[2 * a + 1];
        }
    } else if (kind == PROD_SHUFFLE) {
        for (size_t a = 0; a < n_args; a++) {
            ptr.h[2 * a] = cols[a];
            ptr.h[2 * a + 1] = perms[a];
        }
    }
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;
    H2_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_j0, (int)(uint32_t)u, n_args, s));

    ProdParams P;
    memset(&P, 0, sizeof(P));
    P.n = n;
    P.L = L;
    P.u = u;
    P.R = R;
    P.tiles = (uint32_t)tiles;
    P.bf = bf;
    P.beta = beta;
    P.gamma = gamma;
    P.omega_pow2 = fe.d;
    P.delta_pow = fe.d + 32;
    dim3 grid((uint32_t)tiles, (uint32_t)n_args);
    int tm = c->timer_begin("products", s);
    if (kind == PROD_PERM) {
        hipLaunchKernelGGL(prod_fraction_kernel<PROD_PERM>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    } else if (kind == PROD_LOOKUP) {
        hipLaunchKernelGGL(prod_fraction_kernel<PROD_LOOKUP>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    } else if (kind == PROD_SHUFFLE) {
        hipLaunchKernelGGL(prod_fraction_kernel<PROD_SHUFFLE>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    } else {
        hipLaunchKernelGGL(prod_fraction_kernel<PROD_INVERT>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    }
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(prod_tiles_kernel, dim3((uint32_t)n_args), dim3(PROD_THREADS), 0, s, desc.d, P);
    H2_CHECK(hipGetLastError());
    if (kind == PROD_INVERT) {
        hipLaunchKernelGGL(prod_apply_kernel<PROD_INVERT>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    } else {
        hipLaunchKernelGGL(prod_apply_kernel<PROD_PERM>, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    }
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return guard.release();
}

int permutation_products_device(Ctx* c, uint32_t k, const Fe& omega, const Fe& delta, const Fe& beta, const Fe& gamma,
                                const Fe* const* cols, const Fe* const* perms, uint32_t n_columns, uint32_t chunk_len,
                                const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s) {
    const uint64_t n = 1ull << k, u = n - bf - 1;
    const size_t n_sets = (n_columns + chunk_len - 1) / chunk_len;
    return products_run(c, PROD_PERM, n, u + 1, u, omega, delta, beta, gamma, cols, perms, n_columns, chunk_len, n_sets, blinding, bf, z, s);
}

int lookup_products_device(Ctx* c, uint32_t k, const Fe& beta, const Fe& gamma, const Fe* const* inputs_tables,
                           const Fe* const* permuted, size_t count, const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s) {
    const uint64_t n = 1ull << k, u = n - bf - 1;
    Fe one = fe_one<FrP>();
    return products_run(c, PROD_LOOKUP, n, u + 1, u, one, one, beta, gamma, inputs_tables, permuted, 0, 1, count, blinding, bf, z, s);
}

// shuffle::Argument::commit_product: z[0] = 1, z[i] = z[i-1] (A[i-1] + gamma) inv(S[i-1] + gamma); the fraction kernel's PROD_SHUFFLE
// branch is the only code of its own, the scans, the one inversion and the zero rule are the lookups'
int shuffle_products_device(Ctx* c, uint32_t k, const Fe& gamma, const Fe* const* inputs, const Fe* const* shuffles, size_t count,
                            const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s) {
    const uint64_t n = 1ull << k, u = n - bf - 1;
    Fe one = fe_one<FrP>();
    return products_run(c, PROD_SHUFFLE, n, u + 1, u, one, one, one, gamma, inputs, shuffles, 0, 1, count, blinding, bf, z, s);
}

int batch_invert_device(Ctx* c, Fe* d_a, uint64_t n, hipStream_t s) {
    Fe one = fe_one<FrP>();
    Fe* z[1] = {d_a};
    return products_run(c, PROD_INVERT, n, n, n, one, one, one, one, nullptr, nullptr, 0, 1, 1, nullptr, 0, z, s);
}

// The grand sums of `count` mv-lookup arguments.  The denominators live in mvsum_ws, not in the workspace batch_invert_device takes.
int mvlookup_sums_device(Ctx* c, uint32_t k, const Fe& beta, const Fe* const* inputs, const uint32_t* n_inputs, const Fe* const* tables,
                         const Fe* const* m, size_t count, const uint64_t* blinding, uint32_t bf, Fe* const* phi, hipStream_t s) {
    if (count == 0) return 0;
    const uint64_t n = 1ull << k, u = n - bf - 1, L = u + 1;
    size_t n_cols = count;  // denominator columns: every input, every table
    for (size_t j = 0; j < count; j++) n_cols += n_inputs[j];
    const uint32_t R = prod_rows_per_thread(L, count);
    const uint64_t tile_rows = (uint64_t)PROD_THREADS * R, tiles = (L + tile_rows - 1) / tile_rows;
    Carve arg;
    const size_t o_thr = arg.take(tiles * PROD_THREADS * sizeof(Fe)), o_tile = arg.take(tiles * sizeof(Fe));
    Carve blob;
    const size_t o_desc = blob.take(count * sizeof(MvSumDesc)), o_col = blob.take(n_cols * sizeof(MvDenCol));
    const size_t o_blind = blob.take(count * (size_t)bf * sizeof(Fe));
    Carve ws;
    const size_t o_den = ws.take(n_cols * u * sizeof(Fe)), o_args = ws.take(count * arg.total), o_blob = ws.take(blob.total);
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->mvsum_ws.ensure(ws.total))) return rc;
    char* base = (char*)c->mvsum_ws.p;
    Fe* den = (Fe*)(base + o_den);
    std::vector<char> h(blob.total, 0);
    const Blob img{h.data(), base + o_blob};
    const Mirror<MvSumDesc> desc = img.at<MvSumDesc>(o_desc);
    const Mirror<MvDenCol> col = img.at<MvDenCol>(o_col);
    const Mirror<Fe> blind = img.at<Fe>(o_blind);
    if (bf) memcpy(blind.h, blinding, count * (size_t)bf * sizeof(Fe));
    size_t q = 0, qi = 0;
    for (size_t j = 0; j < count; j++) {
        MvSumDesc& D = desc.h[j];
        char* ab = base + o_args + j * arg.total;
        D.inv = den + q * u;
        D.m = m[j];
        D.phi = phi[j];
        D.thr = (Fe*)(ab + o_thr);
        D.tile = (Fe*)(ab + o_tile);
        D.blind = blind.d + j * (size_t)bf;
        D.K = n_inputs[j];
        for (uint32_t t = 0; t <= n_inputs[j]; t++, q++) {
            col.h[q].col = t < n_inputs[j] ? inputs[qi++] : tables[j];
            col.h[q].out = den + q * u;
        }
    }
    if ((rc = c->stage_h2d(img.d, img.h, blob.total, s))) return rc;
    ProdParams P;
    memset(&P, 0, sizeof(P));
    P.n = n;
    P.L = L;
    P.u = u;
    P.R = R;
    P.tiles = (uint32_t)tiles;
    P.bf = bf;
    int tm = c->timer_begin("mvlookup_sums", s);
    const uint32_t den_tiles = (uint32_t)((u + PROD_THREADS - 1) / PROD_THREADS);
    for (size_t c0 = 0; c0 < n_cols; c0 += 65535) {  // grid.y holds 65535 columns
        const size_t cn = n_cols - c0 < 65535 ? n_cols - c0 : 65535;
        hipLaunchKernelGGL(mvs_den_kernel, dim3(den_tiles, (uint32_t)cn), dim3(PROD_THREADS), 0, s, col.d + c0, u, beta);
        H2_CHECK(hipGetLastError());
    }
    if ((rc = batch_invert_device(c, den, n_cols * u, s))) return rc;  // the call's one field inversion
    const dim3 grid((uint32_t)tiles, (uint32_t)count);
    hipLaunchKernelGGL(mvs_sum_kernel, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mvs_tiles_kernel, dim3((uint32_t)count), dim3(PROD_THREADS), 0, s, desc.d, P);
    H2_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mvs_apply_kernel, grid, dim3(PROD_THREADS), 0, s, desc.d, P);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return guard.release();
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "grand products") ----------------------------------------------------------------------------------
static int products_check_common(const char* what, uint32_t k, uint32_t bf, const uint64_t* blinding, size_t n_outputs) {
    if (int rc = check_k_blinding(what, k, bf)) return rc;
    if (bf && n_outputs && !blinding) {
        set_error("%s: null blinding", what);
        return H2HIP_EINVAL;
    }
    return check_frs(what, blinding, n_outputs * (size_t)bf, "blinding value");
}

static int permutation_check(uint32_t k, const uint64_t omega[4], const uint64_t delta[4], const uint64_t beta[4], const uint64_t gamma[4],
                             const void* const* columns, const void* const* permutations, uint32_t n_columns, uint32_t chunk_len,
                             const uint64_t* blinding, uint32_t bf, const void* const* z) {
    const char* what = "permutation_products";
    if (!omega || !delta || !beta || !gamma) {
        set_error("%s: null scalar", what);
        return H2HIP_EINVAL;
    }
    if (chunk_len == 0) {
        set_error("%s: chunk_len == 0", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(omega, "omega") || check_fr(delta, "delta") || check_fr(beta, "beta") || check_fr(gamma, "gamma")) return H2HIP_EINVAL;
    const size_t n_sets = ((size_t)n_columns + chunk_len - 1) / chunk_len;
    if (int rc = products_check_common(what, k, bf, blinding, n_sets)) return rc;
    if (check_ptrs(what, columns, n_columns, "columns") || check_ptrs(what, permutations, n_columns, "permutations") || check_ptrs(what, z, n_sets, "z"))
        return H2HIP_EINVAL;
    return 0;
}

static int lookup_check(uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const void* const* a, const void* const* s,
                        const void* const* ap, const void* const* sp, size_t count, const uint64_t* blinding, uint32_t bf, const void* const* z) {
    const char* what = "lookup_products";
    if (!beta || !gamma) {
        set_error("%s: null scalar", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(beta, "beta") || check_fr(gamma, "gamma")) return H2HIP_EINVAL;
    if (count > 65535) {
        set_error("%s: count %zu > 65535", what, count);
        return H2HIP_EINVAL;
    }
    if (int rc = products_check_common(what, k, bf, blinding, count)) return rc;
    if (check_ptrs(what, a, count, "compressed_input") || check_ptrs(what, s, count, "compressed_table") ||
        check_ptrs(what, ap, count, "permuted_input") || check_ptrs(what, sp, count, "permuted_table") || check_ptrs(what, z, count, "z"))
        return H2HIP_EINVAL;
    return 0;
}

int h2hip_permutation_products_bn254_device(uint32_t k, const uint64_t omega[4], const uint64_t delta[4], const uint64_t beta[4],
                                            const uint64_t gamma[4], const void* const* d_columns, const void* const* d_permutations,
                                            uint32_t n_columns, uint32_t chunk_len, const uint64_t* blinding, uint32_t blinding_factors,
                                            void* const* d_z, void* stream) {
    if (int rc = permutation_check(k, omega, delta, beta, gamma, d_columns, d_permutations, n_columns, chunk_len, blinding, blinding_factors,
                                   (const void* const*)d_z))
        return rc;
    if (n_columns == 0) return 0;
    if ((n_columns + chunk_len - 1) / chunk_len > 65535) {
        set_error("permutation_products: more than 65535 sets");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_permutation_products_bn254_device", d_z[0]);
    if (en.rc) return en.rc;
    return permutation_products_device(en.c, k, fe_from_u64x4(omega), fe_from_u64x4(delta), fe_from_u64x4(beta), fe_from_u64x4(gamma),
                                       (const Fe* const*)d_columns, (const Fe* const*)d_permutations, n_columns, chunk_len, blinding,
                                       blinding_factors, (Fe* const*)d_z, (hipStream_t)stream);
}

int h2hip_permutation_products_bn254(uint32_t k, const uint64_t omega[4], const uint64_t delta[4], const uint64_t beta[4], const uint64_t gamma[4],
                                     const uint64_t* const* columns, const uint64_t* const* permutations, uint32_t n_columns, uint32_t chunk_len,
                                     const uint64_t* blinding, uint32_t blinding_factors, uint64_t* const* z) {
    if (int rc = permutation_check(k, omega, delta, beta, gamma, (const void* const*)columns, (const void* const*)permutations, n_columns,
                                   chunk_len, blinding, blinding_factors, (const void* const*)z))
        return rc;
    if (n_columns == 0) return 0;
    const size_t n_sets = ((size_t)n_columns + chunk_len - 1) / chunk_len;
    if (n_sets > 65535) {
        set_error("permutation_products: more than 65535 sets");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_permutation_products_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> d_cols(n_columns), d_perm(n_columns);
    std::vector<Fe*> d_z(n_sets);
    HostIo io(c, c->host_io, s);
    for (uint32_t j = 0; j < n_columns; j++) io.in(columns[j], bytes, &d_cols[j]);
    // the key's columns s_c come from the h2hip_columns_pin cache when pinned; only the witness columns and the rest cross PCIe
    for (uint32_t j = 0; j < n_columns; j++) io.in(permutations[j], bytes, &d_perm[j], true);
    for (size_t t = 0; t < n_sets; t++) io.out(z[t], bytes, &d_z[t]);
    int rc = io.upload();  // on the call's own stream, ahead of its kernels
    if (rc) return rc;
    rc = permutation_products_device(c, k, fe_from_u64x4(omega), fe_from_u64x4(delta), fe_from_u64x4(beta), fe_from_u64x4(gamma),
                                     d_cols.data(), d_perm.data(), n_columns, chunk_len, blinding, blinding_factors, d_z.data(), s);
    if (rc) return rc;
    return io.finish();
}

int h2hip_lookup_products_bn254_device(uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const void* const* d_compressed_input,
                                       const void* const* d_compressed_table, const void* const* d_permuted_input,
                                       const void* const* d_permuted_table, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                       void* const* d_z, void* stream) {
    if (int rc = lookup_check(k, beta, gamma, d_compressed_input, d_compressed_table, d_permuted_input, d_permuted_table, count, blinding,
                              blinding_factors, (const void* const*)d_z))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_lookup_products_bn254_device", d_z[0]);
    if (en.rc) return en.rc;
    std::vector<const Fe*> in(2 * count), perm(2 * count);
    for (size_t j = 0; j < count; j++) {
        in[2 * j] = (const Fe*)d_compressed_input[j];
        in[2 * j + 1] = (const Fe*)d_compressed_table[j];
        perm[2 * j] = (const Fe*)d_permuted_input[j];
        perm[2 * j + 1] = (const Fe*)d_permuted_table[j];
    }
    return lookup_products_device(en.c, k, fe_from_u64x4(beta), fe_from_u64x4(gamma), in.data(), perm.data(), count, blinding, blinding_factors,
                                  (Fe* const*)d_z, (hipStream_t)stream);
}

int h2hip_lookup_products_bn254(uint32_t k, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* const* compressed_input,
                                const uint64_t* const* compressed_table, const uint64_t* const* permuted_input,
                                const uint64_t* const* permuted_table, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                uint64_t* const* z) {
    if (int rc = lookup_check(k, beta, gamma, (const void* const*)compressed_input, (const void* const*)compressed_table,
                              (const void* const*)permuted_input, (const void* const*)permuted_table, count, blinding, blinding_factors,
                              (const void* const*)z))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_lookup_products_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> in(2 * count), perm(2 * count);
    std::vector<Fe*> d_z(count);
    HostIo io(c, c->host_io, s);
    for (size_t j = 0; j < count; j++) {  // A, S, A', S', z per lookup
        io.in(compressed_input[j], bytes, &in[2 * j]);
        io.in(compressed_table[j], bytes, &in[2 * j + 1]);
        io.in(permuted_input[j], bytes, &perm[2 * j]);
        io.in(permuted_table[j], bytes, &perm[2 * j + 1]);
        io.out(z[j], bytes, &d_z[j]);
    }
    int rc = io.upload();
    if (rc) return rc;
    rc = lookup_products_device(c, k, fe_from_u64x4(beta), fe_from_u64x4(gamma), in.data(), perm.data(), count, blinding, blinding_factors,
                                d_z.data(), s);
    if (rc) return rc;
    return io.finish();
}

static int shuffle_check(uint32_t k, const uint64_t gamma[4], const void* const* a, const void* const* s, size_t count, const uint64_t* blinding,
                         uint32_t bf, const void* const* z) {
    const char* what = "shuffle_products";
    if (!gamma) {
        set_error("%s: null scalar", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(gamma, "gamma")) return H2HIP_EINVAL;
    if (count > 65535) {
        set_error("%s: count %zu > 65535", what, count);
        return H2HIP_EINVAL;
    }
    if (int rc = products_check_common(what, k, bf, blinding, count)) return rc;
    if (check_ptrs(what, a, count, "compressed_input") || check_ptrs(what, s, count, "compressed_shuffle") || check_ptrs(what, z, count, "z"))
        return H2HIP_EINVAL;
    return 0;
}

int h2hip_shuffle_products_bn254_device(uint32_t k, const uint64_t gamma[4], const void* const* d_compressed_input,
                                        const void* const* d_compressed_shuffle, size_t count, const uint64_t* blinding,
                                        uint32_t blinding_factors, void* const* d_z, void* stream) {
    if (int rc = shuffle_check(k, gamma, d_compressed_input, d_compressed_shuffle, count, blinding, blinding_factors, (const void* const*)d_z))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_shuffle_products_bn254_device", d_z[0]);
    if (en.rc) return en.rc;
    return shuffle_products_device(en.c, k, fe_from_u64x4(gamma), (const Fe* const*)d_compressed_input, (const Fe* const*)d_compressed_shuffle,
                                   count, blinding, blinding_factors, (Fe* const*)d_z, (hipStream_t)stream);
}

int h2hip_shuffle_products_bn254(uint32_t k, const uint64_t gamma[4], const uint64_t* const* compressed_input,
                                 const uint64_t* const* compressed_shuffle, size_t count, const uint64_t* blinding, uint32_t blinding_factors,
                                 uint64_t* const* z) {
    if (int rc = shuffle_check(k, gamma, (const void* const*)compressed_input, (const void* const*)compressed_shuffle, count, blinding,
                               blinding_factors, (const void* const*)z))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_shuffle_products_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> in(count), sh(count);
    std::vector<Fe*> d_z(count);
    HostIo io(c, c->host_io, s);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_input[j], bytes, &in[j]);
        io.in(compressed_shuffle[j], bytes, &sh[j]);
        io.out(z[j], bytes, &d_z[j]);
    }
    int rc = io.upload();
    if (rc) return rc;
    rc = shuffle_products_device(c, k, fe_from_u64x4(gamma), in.data(), sh.data(), count, blinding, blinding_factors, d_z.data(), s);
    if (rc) return rc;
    return io.finish();
}

static int mvsums_check(uint32_t k, const uint64_t beta[4], const void* const* in, const uint32_t* n_inputs, const void* const* tab,
                        const void* const* m, size_t count, const uint64_t* blinding, uint32_t bf, const void* const* phi, size_t* total_in) {
    const char* what = "mvlookup_sums";
    if (!beta) {
        set_error("%s: null scalar", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(beta, "beta")) return H2HIP_EINVAL;
    if (count > 65535) {
        set_error("%s: count %zu > 65535", what, count);
        return H2HIP_EINVAL;
    }
    if (int rc = products_check_common(what, k, bf, blinding, count)) return rc;
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
        total += n_inputs[j];
    }
    if (((total + count) << k) > ((size_t)1 << 30)) {  // one batch inversion takes them all
        set_error("%s: %zu columns of 2^%u denominators > 2^30", what, total + count, k);
        return H2HIP_EINVAL;
    }
    if (check_ptrs(what, in, total, "compressed_input") || check_ptrs(what, tab, count, "compressed_table") || check_ptrs(what, m, count, "m") ||
        check_ptrs(what, phi, count, "phi"))
        return H2HIP_EINVAL;
    *total_in = total;
    return 0;
}

int h2hip_mvlookup_sums_bn254_device(uint32_t k, const uint64_t beta[4], const void* const* d_compressed_inputs, const uint32_t* n_inputs,
                                     const void* const* d_compressed_tables, const void* const* d_m, size_t count, const uint64_t* blinding,
                                     uint32_t blinding_factors, void* const* d_phi, void* stream) {
    size_t total_in;
    if (int rc = mvsums_check(k, beta, d_compressed_inputs, n_inputs, d_compressed_tables, d_m, count, blinding, blinding_factors,
                              (const void* const*)d_phi, &total_in))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_mvlookup_sums_bn254_device", d_phi[0]);
    if (en.rc) return en.rc;
    return mvlookup_sums_device(en.c, k, fe_from_u64x4(beta), (const Fe* const*)d_compressed_inputs, n_inputs, (const Fe* const*)d_compressed_tables,
                                (const Fe* const*)d_m, count, blinding, blinding_factors, (Fe* const*)d_phi, (hipStream_t)stream);
}

int h2hip_mvlookup_sums_bn254(uint32_t k, const uint64_t beta[4], const uint64_t* const* compressed_inputs, const uint32_t* n_inputs,
                              const uint64_t* const* compressed_tables, const uint64_t* const* m, size_t count, const uint64_t* blinding,
                              uint32_t blinding_factors, uint64_t* const* phi) {
    size_t total_in;
    if (int rc = mvsums_check(k, beta, (const void* const*)compressed_inputs, n_inputs, (const void* const*)compressed_tables,
                              (const void* const*)m, count, blinding, blinding_factors, (const void* const*)phi, &total_in))
        return rc;
    if (count == 0) return 0;
    Entry en("h2hip_mvlookup_sums_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(Fe) << k;
    std::vector<const Fe*> in(total_in), tab(count), d_m(count);
    std::vector<Fe*> d_phi(count);
    HostIo io(c, c->host_io, s);
    for (size_t q = 0; q < total_in; q++) io.in(compressed_inputs[q], bytes, &in[q]);
    for (size_t j = 0; j < count; j++) {
        io.in(compressed_tables[j], bytes, &tab[j]);
        io.in(m[j], bytes, &d_m[j]);
        io.out(phi[j], bytes, &d_phi[j]);
    }
    int rc = io.upload();
    if (rc) return rc;
    rc = mvlookup_sums_device(c, k, fe_from_u64x4(beta), in.data(), n_inputs, tab.data(), d_m.data(), count, blinding, blinding_factors,
                              d_phi.data(), s);
    if (rc) return rc;
    return io.finish();
}

// rows per thread of the grand sum's scan for a call of `count` arguments: the rule the code itself applies (tests pick their case by it)
int h2hip_debug_mvlookup_sum_rows(uint32_t k, uint32_t blinding_factors, size_t count, uint32_t* rows) {
    if (!rows || check_k_blinding("debug_mvlookup_sum_rows", k, blinding_factors)) {
        if (!rows) set_error("debug_mvlookup_sum_rows: null argument");
        return H2HIP_EINVAL;
    }
    *rows = prod_rows_per_thread(((uint64_t)1 << k) - blinding_factors, count);
    return 0;
}

static int batch_invert_check(const void* a, size_t n) {
    if (n && !a) {
        set_error("batch_invert: null argument");
        return H2HIP_EINVAL;
    }
    if (n > ((size_t)1 << 30)) {
        set_error("batch_invert: n = %zu > 2^30", n);
        return H2HIP_EINVAL;
    }
    return 0;
}

int h2hip_batch_invert_bn254_fr_device(void* d_a, size_t n, void* stream) {
    if (int rc = batch_invert_check(d_a, n)) return rc;
    if (n == 0) return 0;
    Entry en("h2hip_batch_invert_bn254_fr_device", d_a);
    if (en.rc) return en.rc;
    return batch_invert_device(en.c, (Fe*)d_a, n, (hipStream_t)stream);
}

int h2hip_batch_invert_bn254_fr(uint64_t* a, size_t n) {
    if (int rc = batch_invert_check(a, n)) return rc;
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++)
        if (check_fr(a + 4 * i, "a[i]")) return H2HIP_EINVAL;
    Entry en("h2hip_batch_invert_bn254_fr");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    Fe* d_a = nullptr;
    HostIo io(c, c->host_io, s);
    io.in_at(a, n * sizeof(Fe), io.out(a, n * sizeof(Fe), &d_a));  // in place: one slot both ways
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = batch_invert_device(c, d_a, n, s))) return rc;
    return io.finish();
}

}  // extern "C"
