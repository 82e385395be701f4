// ipa.hip -- the inner-product argument over BN254 G1 (halo2_proofs/src/poly/ipa/): what an opening's k rounds and the verifier's
// vector s do to 2^k elements.  The composition -- transcript, draws, the L_j / R_j MSMs (msm.hip) and the handful of host group
// operations per round -- is the caller's; include/halo2hip_ipa.h states the contract.  A round is also ONE call (ipa_round_device,
// include/halo2hip_ipa_round.h): the fold and the collapse by the challenge before it, the inner products and both MSMs as one run of the
// MSM pipeline (msm.hip msm_pair_device), queued on one stream with one wait.
//   ipa_collapse_kernel       g[i] + [u] g[half + i] (prover.rs:155-167), one lane per point: the scalar is the same for every point, so
//                             it is recoded once on the host (ipa_elem.h: GLV halves in joint sparse form) and every lane walks the same
//                             columns -- a uniform branch over four per-lane points in registers instead of ecfft.hip's 15-entry
//                             per-lane table in scratch; the closing addition is ec.h's complete mixed addition
//   ipa_collapse_quad_kernel  the same with one quad of lanes per point (ecq.h), for halves that leave most of the chip idle
//   (ec_normalize_kernel, ecfft.hip, brings the sums back to affine)
//   ipa_table_kernel          out[i] = prod_l T[256 l + byte l of i]: the powers of x_3 and compute_s (strategy.rs:161-176)
//   ipa_inner_kernel          the two inner products of a round (prover.rs:102-105): per-block sums in a fixed order ...
//   ipa_fold_kernel           the fold of p' and b (prover.rs:118-131), one lane per element, no reduction
//   ipa_fold_inner_kernel     ... the fold with the NEXT round's inner products in the same pass: a lane folds elements i and i + half / 2
//                             of both vectors and multiplies what it has just written
//   ipa_final_kernel          ... and one workgroup adds the blocks' sums, again in a fixed order: no atomics, the same limbs every run
#include "../../include/halo2hip_ipa.h"
#include "ecq.h"
#include "engine.h"
#include "fe_io.h"
#include "ipa_elem.h"

namespace h2 {

#define IPA_THREADS 256
#define IPA_MAX_BLOCKS 1024  // of the reducing kernels: four workgroups per CU
#define IPA_MAX_HALF ((size_t)1 << 27)

struct IpaCollapse {
    const Affine* g;  // 2 * half points
    XYZZ* out;        // half sums
    uint64_t half;
    IpaDigits dg;
};

__global__ void __launch_bounds__(IPA_THREADS) ipa_collapse_kernel(IpaCollapse a) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= a.half) return;
    a.out[tid] = ipa_collapse_elem(a.g[tid], a.g[a.half + tid], a.dg);
}

// ipa_mul_affine over a quad: the four lanes hold the same point and walk the same columns; all four table points are XYZZ and every
// addition is the general one (ecq.h has no mixed form: its products are spread over the lanes either way).  Every lane builds the table
// for itself with the lane form's ipa_base (one product and three mixed additions, of ~200 group operations per ladder), so the table is
// the one tests/cpp/test_ipa_host.cpp walks with the limb bounds asserted.  What xyzzu_sum_q receives, against ecq.h's contract (every
// coordinate normalised, |x|, |y| < 4.5 p, zz, zzz in (-0.1 p, 1.4 p)): p1 and p2 are xyzzu_add_mixed onto the identity, i.e. x, y =
// products by one in (-0.2 p, 1.2 p) and zz = zzz = the constant one (< p), all fu_mul outputs; s and d are outputs of
// xyzzu_add_mixed_nonid, whose X3 and Y3 come normalised from the fused forms with |X3| < 4.5 p, |Y3| < 2.3 p and zz, zzz products
// (ecu.h's bound bookkeeping); a negated entry is fu_norm(fu_neg(y)), the same magnitude, normalised again; acc is only ever an output of
// xyzzu_double_q / xyzzu_sum_q.
__device__ XYZZu ipa_mul_affine_q(const Affine& p, const IpaDigits& dg, uint32_t role) {
    XYZZu acc = xyzzu_identity();
    if (dg.len == 0 || affine_is_identity(p)) return acc;
    const IpaBase t = ipa_base(p, dg);
    XYZZu p1 = xyzzu_identity(), p2 = xyzzu_identity();
    xyzzu_add_mixed<QU>(p1, t.x1, t.y1);
    xyzzu_add_mixed<QU>(p2, t.x2, t.y2);
    for (int j = (int)dg.len - 1; j >= 0; j--) {
        acc = xyzzu_double_q(acc, role);
        const uint32_t col = ipa_column(dg, (uint32_t)j);
        const int d1 = (int)(col & 3) - 1, d2 = (int)(col >> 2) - 1;
        if (d1 == 0 && d2 == 0) continue;
        XYZZu q = d1 != 0 && d2 != 0 ? (d1 == d2 ? t.s : t.d) : d1 != 0 ? p1 : p2;
        if ((d1 != 0 ? d1 : d2) < 0) q.y = fu_norm(fu_neg(q.y));
        acc = xyzzu_sum_q(acc, q, role);
    }
    return acc;
}

__global__ void __launch_bounds__(IPA_THREADS) ipa_collapse_quad_kernel(IpaCollapse a) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t tid = gid >> 2;
    const uint32_t role = (uint32_t)gid & 3;
    if (tid >= a.half) return;
    const Affine lo = a.g[tid], hi = a.g[a.half + tid];
    XYZZ t = xyzzu_to_ext(ipa_mul_affine_q(hi, a.dg, role));
    if (role != 0) return;  // the closing addition is canonical arithmetic: one lane
    xyzz_add_mixed(t, lo);
    a.out[tid] = t;
}

__global__ void __launch_bounds__(IPA_THREADS) ipa_table_kernel(const Fe* T, uint32_t levels, Fe* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * IPA_THREADS + threadIdx.x;
    if (i >= n) return;
    fe_st(out, i, ipa_table_elem(T, levels, i));
}

// the workgroup's sums of v0 and v1, in a fixed tree order, into part[2 * block], part[2 * block + 1]
__device__ __forceinline__ void ipa_block_sums(Fe v0, Fe v1, Fe* part) {
    __shared__ Fe sh[2][IPA_THREADS];
    const uint32_t t = threadIdx.x;
    sh[0][t] = v0;
    sh[1][t] = v1;
    __syncthreads();
    for (uint32_t w = IPA_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) {
            sh[0][t] = fe_add<FrP>(sh[0][t], sh[0][t + w]);
            sh[1][t] = fe_add<FrP>(sh[1][t], sh[1][t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        fe_st(part, 2 * (uint64_t)blockIdx.x, sh[0][0]);
        fe_st(part, 2 * (uint64_t)blockIdx.x + 1, sh[1][0]);
    }
}

// every workgroup of the launch runs ipa_block_sums, so no lane leaves before it: lanes past the end add zeros
__global__ void __launch_bounds__(IPA_THREADS) ipa_inner_kernel(const Fe* p, const Fe* b, uint64_t half, Fe* part) {
    Fe v0 = fe_zero<FrP>(), v1 = v0;
    for (uint64_t i = (uint64_t)blockIdx.x * IPA_THREADS + threadIdx.x; i < half; i += (uint64_t)gridDim.x * IPA_THREADS) {
        v0 = fe_add<FrP>(v0, ipa_fr_mul(fe_ld(p, half + i), fe_ld(b, i)));
        v1 = fe_add<FrP>(v1, ipa_fr_mul(fe_ld(p, i), fe_ld(b, half + i)));
    }
    ipa_block_sums(v0, v1, part);
}

__global__ void __launch_bounds__(IPA_THREADS) ipa_fold_kernel(Fe* p, Fe* b, uint64_t half, Fe u_inv, Fe u) {
    const uint64_t i = (uint64_t)blockIdx.x * IPA_THREADS + threadIdx.x;
    if (i >= half) return;
    fe_st(p, i, ipa_fold_elem(fe_ld(p, i), fe_ld(p, half + i), u_inv));
    fe_st(b, i, ipa_fold_elem(fe_ld(b, i), fe_ld(b, half + i), u));
}

// half = 2 q: lane i < q folds elements i and q + i of both vectors (it alone reads and writes them and their partners half + i,
// half + q + i), then adds p'[q + i] b'[i] and p'[i] b'[q + i] to its sums
__global__ void __launch_bounds__(IPA_THREADS) ipa_fold_inner_kernel(Fe* p, Fe* b, uint64_t half, Fe u_inv, Fe u, Fe* part) {
    const uint64_t q = half / 2;
    Fe v0 = fe_zero<FrP>(), v1 = v0;
    for (uint64_t i = (uint64_t)blockIdx.x * IPA_THREADS + threadIdx.x; i < q; i += (uint64_t)gridDim.x * IPA_THREADS) {
        const Fe p_lo = ipa_fold_elem(fe_ld(p, i), fe_ld(p, half + i), u_inv);
        const Fe p_hi = ipa_fold_elem(fe_ld(p, q + i), fe_ld(p, half + q + i), u_inv);
        const Fe b_lo = ipa_fold_elem(fe_ld(b, i), fe_ld(b, half + i), u);
        const Fe b_hi = ipa_fold_elem(fe_ld(b, q + i), fe_ld(b, half + q + i), u);
        fe_st(p, i, p_lo);
        fe_st(p, q + i, p_hi);
        fe_st(b, i, b_lo);
        fe_st(b, q + i, b_hi);
        v0 = fe_add<FrP>(v0, ipa_fr_mul(p_hi, b_lo));
        v1 = fe_add<FrP>(v1, ipa_fr_mul(p_lo, b_hi));
    }
    ipa_block_sums(v0, v1, part);
}

// one workgroup: lane t adds the sums of blocks t, t + 256, ..., then the tree
__global__ void __launch_bounds__(IPA_THREADS) ipa_final_kernel(const Fe* part, uint32_t blocks, Fe* vals) {
    Fe v0 = fe_zero<FrP>(), v1 = v0;
    for (uint32_t j = threadIdx.x; j < blocks; j += IPA_THREADS) {
        v0 = fe_add<FrP>(v0, fe_ld(part, 2 * (uint64_t)j));
        v1 = fe_add<FrP>(v1, fe_ld(part, 2 * (uint64_t)j + 1));
    }
    ipa_block_sums(v0, v1, vals);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// Ctx::ipa_ws, one size for every call: the byte table | the blocks' sums | the two values
struct IpaWs {
    Fe *table, *part, *vals;
};
static int ipa_ws(Ctx* c, IpaWs* w) {
    Carve cv;
    const size_t table = cv.take(IPA_TABLE_ELEMS * sizeof(Fe)), part = cv.take(2 * IPA_MAX_BLOCKS * sizeof(Fe)), vals = cv.take(2 * sizeof(Fe));
    if (int rc = c->ipa_ws.ensure(cv.total)) return rc;
    char* base = (char*)c->ipa_ws.p;
    w->table = (Fe*)(base + table);
    w->part = (Fe*)(base + part);
    w->vals = (Fe*)(base + vals);
    return 0;
}

static uint32_t ipa_blocks(uint64_t lanes) {
    const uint64_t b = (lanes + IPA_THREADS - 1) / IPA_THREADS;
    return (uint32_t)(b < IPA_MAX_BLOCKS ? (b ? b : 1) : IPA_MAX_BLOCKS);
}

static int ipa_collapse_device(Ctx* c, Affine* d_g, size_t half, const Fe& u, hipStream_t s) {
    const Fe uc = fe_to_canonical<FrP>(u);
    IpaCollapse a;
    a.dg = ipa_digits(uc.l);
    int rc = c->ecfft_ws.ensure(half * sizeof(XYZZ) + 256);
    if (rc) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    a.g = d_g;
    a.out = (XYZZ*)c->ecfft_ws.p;
    a.half = half;
    int tm = c->timer_begin("ipa_collapse", s);
    if (half <= tune().ipa_quad_max_half)
        hipLaunchKernelGGL(ipa_collapse_quad_kernel, dim3((uint32_t)((4 * half + IPA_THREADS - 1) / IPA_THREADS)), dim3(IPA_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(ipa_collapse_kernel, dim3((uint32_t)((half + IPA_THREADS - 1) / IPA_THREADS)), dim3(IPA_THREADS), 0, s, a);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    tm = c->timer_begin("ipa_normalize", s);
    if ((rc = ec_normalize_device(a.out, d_g, half, s))) return rc;
    c->timer_end(tm, s);
    return guard.release();
}

// out[i] = prod_l T[256 l + byte l of i], T a host table of 256 * levels elements
static int ipa_table_device(Ctx* c, const Fe* T, uint32_t levels, Fe* d_out, uint64_t n, const char* timer, hipStream_t s) {
    IpaWs w;
    int rc = ipa_ws(c, &w);
    if (rc) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    if ((rc = c->stage_h2d(w.table, T, 256 * (size_t)levels * sizeof(Fe), s))) return rc;
    int tm = c->timer_begin(timer, s);
    hipLaunchKernelGGL(ipa_table_kernel, dim3((uint32_t)((n + IPA_THREADS - 1) / IPA_THREADS)), dim3(IPA_THREADS), 0, s, (const Fe*)w.table, levels, d_out, n);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    return guard.release();
}

// the blocks' sums in w.part -> the two values in the caller's memory; waits for s
static int ipa_deliver(Ctx* c, const IpaWs& w, uint32_t blocks, uint64_t* values, hipStream_t s) {
    hipLaunchKernelGGL(ipa_final_kernel, dim3(1), dim3(IPA_THREADS), 0, s, (const Fe*)w.part, blocks, w.vals);
    H2_CHECK(hipGetLastError());
    int rc = c->ipa_vals.ensure(2 * sizeof(Fe));
    if (rc) return rc;
    H2_CHECK(hipMemcpyAsync(c->ipa_vals.p, w.vals, 2 * sizeof(Fe), hipMemcpyDeviceToHost, s));
    H2_CHECK(hipStreamSynchronize(s));
    memcpy(values, c->ipa_vals.p, 2 * sizeof(Fe));
    return 0;
}

static int ipa_inner_device(Ctx* c, const Fe* d_p, const Fe* d_b, size_t half, uint64_t* values, hipStream_t s) {
    IpaWs w;
    int rc = ipa_ws(c, &w);
    if (rc) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    const uint32_t blocks = ipa_blocks(half);
    int tm = c->timer_begin("ipa_inner_products", s);
    hipLaunchKernelGGL(ipa_inner_kernel, dim3(blocks), dim3(IPA_THREADS), 0, s, d_p, d_b, (uint64_t)half, w.part);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    if ((rc = ipa_deliver(c, w, blocks, values, s))) return rc;
    return guard.release();
}

static int ipa_fold_device(Ctx* c, Fe* d_p, Fe* d_b, size_t half, const Fe& u_inv, const Fe& u, uint64_t* next_values, hipStream_t s) {
    int tm = c->timer_begin("ipa_fold", s);
    if (!next_values) {
        hipLaunchKernelGGL(ipa_fold_kernel, dim3((uint32_t)((half + IPA_THREADS - 1) / IPA_THREADS)), dim3(IPA_THREADS), 0, s, d_p, d_b, (uint64_t)half, u_inv, u);
        H2_CHECK(hipGetLastError());
        c->timer_end(tm, s);
        return 0;
    }
    IpaWs w;
    int rc = ipa_ws(c, &w);
    if (rc) return rc;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    const uint32_t blocks = ipa_blocks(half / 2);
    hipLaunchKernelGGL(ipa_fold_inner_kernel, dim3(blocks), dim3(IPA_THREADS), 0, s, d_p, d_b, (uint64_t)half, u_inv, u, w.part);
    H2_CHECK(hipGetLastError());
    c->timer_end(tm, s);
    if ((rc = ipa_deliver(c, w, blocks, next_values, s))) return rc;
    return guard.release();
}

// One round after the challenge of the round before it: [the fold of p and b and the collapse of g at 2 half, by that challenge,] the
// inner products and the two MSMs at half -- everything queued on s, and the one wait is the pair MSM's.  The values travel ahead of
// it: their copy into pinned memory is queued before the collapse and the MSM stages, so the MSM's wait delivers them too.  With u the
// fold and the inner products are ipa_fold_inner_kernel, as in h2hip_ipa_fold with next_values.
static int ipa_round_device(Ctx* c, Fe* d_p, Fe* d_b, Affine* d_g, size_t half, const Fe* u, const Fe* u_inv, XYZZ* h_sums, uint64_t* values,
                            hipStream_t s) {
    {
        IpaWs w;
        int rc = ipa_ws(c, &w);
        if (rc) return rc;
        if ((rc = c->ipa_vals.ensure(2 * sizeof(Fe)))) return rc;
        if ((rc = c->ws_acquire(s))) return rc;
        WsGuard guard(c, s);
        const uint32_t blocks = ipa_blocks(half);
        if (u) {
            int tm = c->timer_begin("ipa_fold", s);
            hipLaunchKernelGGL(ipa_fold_inner_kernel, dim3(blocks), dim3(IPA_THREADS), 0, s, d_p, d_b, (uint64_t)(2 * half), *u_inv, *u, w.part);
            H2_CHECK(hipGetLastError());
            c->timer_end(tm, s);
        } else {
            int tm = c->timer_begin("ipa_inner_products", s);
            hipLaunchKernelGGL(ipa_inner_kernel, dim3(blocks), dim3(IPA_THREADS), 0, s, (const Fe*)d_p, (const Fe*)d_b, (uint64_t)half, w.part);
            H2_CHECK(hipGetLastError());
            c->timer_end(tm, s);
        }
        hipLaunchKernelGGL(ipa_final_kernel, dim3(1), dim3(IPA_THREADS), 0, s, (const Fe*)w.part, blocks, w.vals);
        H2_CHECK(hipGetLastError());
        H2_CHECK(hipMemcpyAsync(c->ipa_vals.p, w.vals, 2 * sizeof(Fe), hipMemcpyDeviceToHost, s));
        if ((rc = guard.release())) return rc;
    }
    if (u)
        if (int rc = ipa_collapse_device(c, d_g, 2 * half, *u, s)) return rc;
    if (int rc = msm_pair_device(c, d_p, d_g, half, h_sums, s)) return rc;  // waits for s
    memcpy(values, c->ipa_vals.p, 2 * sizeof(Fe));
    return 0;
}

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip_ipa.h) ------------------------------------------------------------------------------------------------------
static int ipa_ptr(const char* what, const void* p, const char* name) {
    if (!p) {
        set_error("%s: null %s", what, name);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int ipa_dptr(const char* what, const void* p, const char* name) {
    if (int rc = ipa_ptr(what, p, name)) return rc;
    if ((uintptr_t)p & 15) {
        set_error("%s: %s is not 16-byte aligned", what, name);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int ipa_half(const char* what, size_t half) {
    if (half < 1 || half > IPA_MAX_HALF) {
        set_error("%s: half = %zu is outside 1 .. 2^27", what, half);
        return H2HIP_EINVAL;
    }
    return 0;
}

static int ipa_scalar(const char* what, const uint64_t* v, const char* name) {
    if (int rc = ipa_ptr(what, v, name)) return rc;
    return check_fr(v, name);
}

static int ipa_s_args(const char* what, const uint64_t* u, uint32_t k, const uint64_t* init, const void* s) {
    if (k < 1 || k > 28) {
        set_error("%s: k = %u is outside 1 .. 28", what, k);
        return H2HIP_EINVAL;
    }
    if (int rc = ipa_ptr(what, u, "u")) return rc;
    if (int rc = check_frs(what, u, k, "u")) return rc;
    if (int rc = ipa_scalar(what, init, "init")) return rc;
    return ipa_ptr(what, s, "s");
}

int h2hip_ipa_collapse_bn254_device(void* d_g_xy, size_t half, const uint64_t u[4], void* stream) {
    if (int rc = ipa_half("ipa_collapse", half)) return rc;
    if (int rc = ipa_dptr("ipa_collapse", d_g_xy, "d_g_xy")) return rc;
    if (int rc = ipa_scalar("ipa_collapse", u, "u")) return rc;
    Entry en("h2hip_ipa_collapse_bn254_device", d_g_xy);
    if (en.rc) return en.rc;
    return ipa_collapse_device(en.c, (Affine*)d_g_xy, half, fe_from_u64x4(u), (hipStream_t)stream);
}

int h2hip_ipa_collapse_bn254(uint64_t* g_xy, size_t half, const uint64_t u[4]) {
    if (int rc = ipa_half("ipa_collapse", half)) return rc;
    if (int rc = ipa_ptr("ipa_collapse", g_xy, "g_xy")) return rc;
    if (int rc = ipa_scalar("ipa_collapse", u, "u")) return rc;
    Entry en("h2hip_ipa_collapse_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    Affine* d_g = nullptr;
    HostIo io(c, c->host_io, s, true);
    const size_t off = io.room(2 * half * sizeof(Affine), &d_g);
    io.in_at(g_xy, 2 * half * sizeof(Affine), off);
    io.out_at(g_xy, half * sizeof(Affine), off);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = ipa_collapse_device(c, d_g, half, fe_from_u64x4(u), s))) return rc;
    return io.finish();
}

int h2hip_ipa_powers_bn254_fr_device(const uint64_t x[4], size_t n, void* d_out, void* stream) {
    if (n < 1 || n > ((size_t)1 << 28)) {
        set_error("ipa_powers: n = %zu is outside 1 .. 2^28", n);
        return H2HIP_EINVAL;
    }
    if (int rc = ipa_scalar("ipa_powers", x, "x")) return rc;
    if (int rc = ipa_dptr("ipa_powers", d_out, "d_out")) return rc;
    Entry en("h2hip_ipa_powers_bn254_fr_device", d_out);
    if (en.rc) return en.rc;
    std::vector<Fe> T(IPA_TABLE_ELEMS);
    const uint32_t levels = ipa_powers_table(fe_from_u64x4(x), n, T.data());
    return ipa_table_device(en.c, T.data(), levels, (Fe*)d_out, n, "ipa_powers", (hipStream_t)stream);
}

int h2hip_ipa_inner_products_bn254_fr_device(const void* d_p, const void* d_b, size_t half, uint64_t values[8], void* stream) {
    if (int rc = ipa_half("ipa_inner_products", half)) return rc;
    if (int rc = ipa_dptr("ipa_inner_products", d_p, "d_p")) return rc;
    if (int rc = ipa_dptr("ipa_inner_products", d_b, "d_b")) return rc;
    if (int rc = ipa_ptr("ipa_inner_products", values, "values")) return rc;
    Entry en("h2hip_ipa_inner_products_bn254_fr_device", d_p);
    if (en.rc) return en.rc;
    return ipa_inner_device(en.c, (const Fe*)d_p, (const Fe*)d_b, half, values, (hipStream_t)stream);
}

int h2hip_ipa_fold_bn254_fr_device(void* d_p, void* d_b, size_t half, const uint64_t u_inv[4], const uint64_t u[4], uint64_t* next_values,
                                   void* stream) {
    if (int rc = ipa_half("ipa_fold", half)) return rc;
    if (int rc = ipa_dptr("ipa_fold", d_p, "d_p")) return rc;
    if (int rc = ipa_dptr("ipa_fold", d_b, "d_b")) return rc;
    if (int rc = ipa_scalar("ipa_fold", u_inv, "u_inv")) return rc;
    if (int rc = ipa_scalar("ipa_fold", u, "u")) return rc;
    if (next_values && (half & 1)) {
        set_error("ipa_fold: next_values asked for an odd half = %zu", half);
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_ipa_fold_bn254_fr_device", d_p);
    if (en.rc) return en.rc;
    return ipa_fold_device(en.c, (Fe*)d_p, (Fe*)d_b, half, fe_from_u64x4(u_inv), fe_from_u64x4(u), next_values, (hipStream_t)stream);
}

static int ipa_s_run(Ctx* c, const uint64_t* u, uint32_t k, const uint64_t* init, Fe* d_s, hipStream_t s) {
    std::vector<Fe> T(IPA_TABLE_ELEMS), uf(k);
    for (uint32_t i = 0; i < k; i++) uf[i] = fe_from_u64x4(u + 4 * i);
    const uint32_t levels = ipa_s_table(uf.data(), k, fe_from_u64x4(init), T.data());
    return ipa_table_device(c, T.data(), levels, d_s, 1ull << k, "ipa_compute_s", s);
}

int h2hip_ipa_compute_s_bn254_fr_device(const uint64_t* u, uint32_t k, const uint64_t init[4], void* d_s, void* stream) {
    if (int rc = ipa_s_args("ipa_compute_s", u, k, init, d_s)) return rc;
    if (int rc = ipa_dptr("ipa_compute_s", d_s, "d_s")) return rc;
    Entry en("h2hip_ipa_compute_s_bn254_fr_device", d_s);
    if (en.rc) return en.rc;
    return ipa_s_run(en.c, u, k, init, (Fe*)d_s, (hipStream_t)stream);
}

int h2hip_ipa_compute_s_bn254_fr(const uint64_t* u, uint32_t k, const uint64_t init[4], uint64_t* s) {
    if (int rc = ipa_s_args("ipa_compute_s", u, k, init, s)) return rc;
    Entry en("h2hip_ipa_compute_s_bn254_fr");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    Fe* d_s = nullptr;
    HostIo io(c, c->host_io, c->stream, true);
    io.out(s, sizeof(Fe) << k, &d_s);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = ipa_s_run(c, u, k, init, d_s, c->stream))) return rc;
    return io.finish();
}

static int ipa_round_half(const char* what, size_t half) {
    if (half < 1 || half > IPA_MAX_HALF / 2) {
        set_error("%s: half = %zu is outside 1 .. 2^26", what, half);
        return H2HIP_EINVAL;
    }
    return 0;
}

static void ipa_sum_out(const XYZZ& r, uint64_t out_xyz[12]) {
    const Jac j = xyzz_to_jac(r);
    memcpy(out_xyz, &j, 96);
}

int h2hip_ipa_round_msms_bn254_device(const void* d_p, const void* d_g_xy, size_t half, uint64_t out_l[12], uint64_t out_r[12], void* stream) {
    if (int rc = ipa_round_half("ipa_round_msms", half)) return rc;
    if (int rc = ipa_dptr("ipa_round_msms", d_p, "d_p")) return rc;
    if (int rc = ipa_dptr("ipa_round_msms", d_g_xy, "d_g_xy")) return rc;
    if (int rc = ipa_ptr("ipa_round_msms", out_l, "out_l")) return rc;
    if (int rc = ipa_ptr("ipa_round_msms", out_r, "out_r")) return rc;
    Entry en("h2hip_ipa_round_msms_bn254_device", d_p);
    if (en.rc) return en.rc;
    XYZZ sums[2];
    if (int rc = msm_pair_device(en.c, (const Fe*)d_p, (const Affine*)d_g_xy, half, sums, (hipStream_t)stream)) return rc;
    ipa_sum_out(sums[0], out_l);
    ipa_sum_out(sums[1], out_r);
    return 0;
}

int h2hip_ipa_round_bn254_device(void* d_p, void* d_b, void* d_g_xy, size_t half, const uint64_t u[4], const uint64_t u_inv[4], uint64_t out_l[12],
                                 uint64_t out_r[12], uint64_t values[8], void* stream) {
    if (int rc = ipa_round_half("ipa_round", half)) return rc;
    if (int rc = ipa_dptr("ipa_round", d_p, "d_p")) return rc;
    if (int rc = ipa_dptr("ipa_round", d_b, "d_b")) return rc;
    if (int rc = ipa_dptr("ipa_round", d_g_xy, "d_g_xy")) return rc;
    if (int rc = ipa_ptr("ipa_round", out_l, "out_l")) return rc;
    if (int rc = ipa_ptr("ipa_round", out_r, "out_r")) return rc;
    if (int rc = ipa_ptr("ipa_round", values, "values")) return rc;
    if ((u != nullptr) != (u_inv != nullptr)) {
        set_error("ipa_round: %s given without %s", u ? "u" : "u_inv", u ? "u_inv" : "u");
        return H2HIP_EINVAL;
    }
    Fe fu, fu_inv;
    if (u) {
        if (int rc = ipa_scalar("ipa_round", u, "u")) return rc;
        if (int rc = ipa_scalar("ipa_round", u_inv, "u_inv")) return rc;
        fu = fe_from_u64x4(u);
        fu_inv = fe_from_u64x4(u_inv);
    }
    Entry en("h2hip_ipa_round_bn254_device", d_p);
    if (en.rc) return en.rc;
    XYZZ sums[2];
    if (int rc = ipa_round_device(en.c, (Fe*)d_p, (Fe*)d_b, (Affine*)d_g_xy, half, u ? &fu : nullptr, u ? &fu_inv : nullptr, sums, values,
                                  (hipStream_t)stream))
        return rc;
    ipa_sum_out(sums[0], out_l);
    ipa_sum_out(sums[1], out_r);
    return 0;
}

size_t h2hip_ipa_round_msms_fused_max_half(void) {
    TuneRead r;
    return msm_pair_fused_max_half(IPA_MAX_HALF / 2);
}

int h2hip_ipa_set_round_call(int on) {
    TuneWrite()->ipa_round_call = on != 0;
    return 0;
}

int h2hip_ipa_get_round_call(void) {
    TuneRead r;
    return tune().ipa_round_call ? 1 : 0;
}

int h2hip_ipa_set_collapse_quad(size_t max_half) {
    TuneWrite()->ipa_quad_max_half = max_half ? max_half : Tuning{}.ipa_quad_max_half;
    return 0;
}

size_t h2hip_ipa_get_collapse_quad(void) {
    TuneRead r;
    return tune().ipa_quad_max_half;
}

}  // extern "C"
