// keygen.hip -- the data-parallel columns of keygen_vk / keygen_pk on the GPU.
//
// Replaces the host loops that build what create_proof consumes:
//   permutation::keygen::Assembly::build_vk / build_pk (plonk/permutation/keygen.rs:105-242): per permutation column the sigma table
//       permutations[j][i] = delta^c omega^r, (c, r) = mapping[j][i], its lagrange_to_coeff and its coeff_to_extended;
//   batch_invert_assigned (poly.rs:180-209): one BatchInvert over every column's Rational denominators, then numerator * inverse;
//   l0, l_last, l_active_row (plonk/keygen.rs:320-351) in extended-coset form.
//
// Plan (Keygen).  The reference gathers from deltaomega, m tables of 2^k elements, by data-dependent row: 64 lanes in 64 rows
// of a table of up to 8 GB.  Montgomery products are exact, so any factorisation gives the same limbs:
//     delta^c omega^r = LO[r mod 2^h] * HI_c[r >> h],   LO[i] = omega^i,   HI_c[i] = delta^c omega^(i 2^h),   h = ceil(k / 2)
// m + 1 tables of at most 2^14 entries that stay in L2; per cell 8 bytes read, one product, 32 bytes written, coalesced.
//   kg_tables_kernel   LO and the HI_c, one power per thread;
//   kg_sigma_kernel    (row tiles x columns): the product per cell; a pair out of range raises a flag and writes zero;
//   the transforms are the batched NTT kernels (ntt.hip), out of place from one form into the next, so no column is copied;
//   kg_scatter_kernel  out[row] *= inverse, over the sparse Rational cells of every column (the inversion is product.hip's);
//   kg_units_kernel / kg_active_kernel  the three unit-like columns and 1 - (l_last + l_blind) around their transforms.
#include <string.h>
#include <vector>
#include "engine.h"
#include "fe_io.h"

namespace h2 {

#define KG_THREADS 256
#define KG_MAX_COLUMNS 65535  // one grid row per column

struct KgDomain {
    uint32_t k, ek;
    Fe omega, omega_inv, divisor, ext_omega, g_coset, g_coset_inv;
};

struct KgScatter {
    Fe* out;
    const uint32_t* rows;
    uint64_t off;  // of this column's inverses in the concatenated array
    uint32_t count;
    uint32_t pad;
};

// a^e from the top set bit of e down
__device__ Fe kg_pow(const Fe& a, uint32_t e) {
    Fe r = fe_one<FrP>();
    for (int i = 31 - (e ? __clz(e) : 32); i >= 0; i--) {
        r = fe_sqr<FrP>(r);
        if ((e >> i) & 1) r = fe_mul<FrP>(r, a);
    }
    return r;
}

// tab[0 .. lo_n) = omega^i; tab[lo_n + c hi_n + i] = delta^c omega_hi^i (omega_hi = omega^lo_n), c < m, i < hi_n
__global__ void __launch_bounds__(KG_THREADS) kg_tables_kernel(Fe* tab, Fe omega, Fe omega_hi, Fe delta, uint32_t lo_n, uint32_t hi_n, uint32_t m) {
    const uint64_t t = blockIdx.x * (uint64_t)KG_THREADS + threadIdx.x;
    if (t >= lo_n + (uint64_t)m * hi_n) return;
    Fe v;
    if (t < lo_n) {
        v = kg_pow(omega, (uint32_t)t);
    } else {
        const uint64_t q = t - lo_n;
        v = fe_mul<FrP>(kg_pow(delta, (uint32_t)(q / hi_n)), kg_pow(omega_hi, (uint32_t)(q % hi_n)));
    }
    fe_st(tab, t, v);
}

// outs[j][i] = delta^c omega^r for (c, r) = maps[j][i], j = blockIdx.y < columns of this launch; c is checked against m_total (the
// tables' columns), r against 2^k
__global__ void __launch_bounds__(KG_THREADS) kg_sigma_kernel(const uint2* const* maps, Fe* const* outs, const Fe* tab, uint32_t k,
                                                              uint32_t lo_bits, uint32_t m_total, uint32_t* flag) {
    const uint2* map = maps[blockIdx.y];
    Fe* out = outs[blockIdx.y];
    const uint64_t n = 1ull << k;
    const uint32_t lo_n = 1u << lo_bits, hi_n = 1u << (k - lo_bits);
    for (uint64_t i = blockIdx.x * (uint64_t)KG_THREADS + threadIdx.x; i < n; i += gridDim.x * (uint64_t)KG_THREADS) {
        const uint2 cr = map[i];
        Fe v;
        if (cr.x >= m_total || cr.y >= n) {
            atomicOr(flag, 1u);
            v = fe_zero<FrP>();
        } else {
            v = fe_mul<FrP>(fe_ld(tab, cr.y & (lo_n - 1)), fe_ld(tab, lo_n + (uint64_t)cr.x * hi_n + (cr.y >> lo_bits)));
        }
        fe_st(out, i, v);
    }
}

// out[rows[t]] *= inv[off + t]; a row index out of range is skipped
__global__ void __launch_bounds__(KG_THREADS) kg_scatter_kernel(const KgScatter* descs, const Fe* inv, uint64_t n) {
    const KgScatter d = descs[blockIdx.y];
    for (uint64_t t = blockIdx.x * (uint64_t)KG_THREADS + threadIdx.x; t < d.count; t += gridDim.x * (uint64_t)KG_THREADS) {
        const uint32_t r = d.rows[t];
        if (r < n) fe_st(d.out, r, fe_mul<FrP>(fe_ld(d.out, r), fe_ld(inv, d.off + t)));
    }
}

// rows 0 .. n - 1 of the Lagrange columns l0 = e_0, l_last = e_u, l_blind = sum of e_i, i >= n - b (plonk/keygen.rs:322-339)
__global__ void __launch_bounds__(KG_THREADS) kg_units_kernel(Fe* l0, Fe* l_last, Fe* l_blind, uint64_t n, uint64_t b) {
    const uint64_t i = blockIdx.x * (uint64_t)KG_THREADS + threadIdx.x;
    if (i >= n) return;
    const Fe one = fe_one<FrP>(), zero = fe_zero<FrP>();
    fe_st(l0, i, i == 0 ? one : zero);
    fe_st(l_last, i, i == n - b - 1 ? one : zero);
    fe_st(l_blind, i, i >= n - b ? one : zero);
}

// l_active_row = 1 - (l_last + l_blind) (plonk/keygen.rs:344-351), in place over l_blind
__global__ void __launch_bounds__(KG_THREADS) kg_active_kernel(Fe* l_active, const Fe* l_last, uint64_t len) {
    const uint64_t i = blockIdx.x * (uint64_t)KG_THREADS + threadIdx.x;
    if (i >= len) return;
    fe_st(l_active, i, fe_sub<FrP>(fe_one<FrP>(), fe_add<FrP>(fe_ld(l_last, i), fe_ld(l_active, i))));
}

static uint32_t kg_grid(uint64_t items) {
    uint64_t g = (items + KG_THREADS - 1) / KG_THREADS;
    return (uint32_t)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// the workspace of one permutation keygen call: the power tables of all m_total columns, the flag, one group's pointer blob
struct KgPerm {
    const Fe* tab = nullptr;
    uint32_t* flag = nullptr;
    char* blob = nullptr;
    uint32_t lo_bits = 0, m_total = 0;
};

static int kg_perm_prepare(Ctx* c, const KgDomain& d, const Fe& delta, uint32_t m_total, uint32_t group_cols, hipStream_t s, KgPerm* w) {
    const uint32_t lo_bits = (d.k + 1) / 2;
    const uint32_t lo_n = 1u << lo_bits, hi_n = 1u << (d.k - lo_bits);
    Carve ws;
    const size_t o_tab = ws.take(((size_t)lo_n + (size_t)m_total * hi_n) * sizeof(Fe)), o_flag = ws.take(256),
                 o_blob = ws.take(2 * (size_t)group_cols * sizeof(void*));
    int rc = c->keygen_ws.ensure(ws.total);
    if (rc) return rc;
    char* base = (char*)c->keygen_ws.p;
    w->tab = (const Fe*)(base + o_tab);
    w->flag = (uint32_t*)(base + o_flag);
    w->blob = base + o_blob;
    w->lo_bits = lo_bits;
    w->m_total = m_total;
    H2_CHECK(hipMemsetAsync(w->flag, 0, 256, s));
    Fe omega_hi = d.omega;
    for (uint32_t i = 0; i < lo_bits; i++) omega_hi = fe_sqr<FrP>(omega_hi);
    const uint64_t total = lo_n + (uint64_t)m_total * hi_n;
    hipLaunchKernelGGL(kg_tables_kernel, dim3((uint32_t)((total + KG_THREADS - 1) / KG_THREADS)), dim3(KG_THREADS), 0, s, (Fe*)(base + o_tab), d.omega,
                       omega_hi, delta, lo_n, hi_n, m_total);
    H2_CHECK(hipGetLastError());
    return 0;
}

// `count` columns (count <= the group_cols of kg_perm_prepare): sigma into the first wanted form, then each later form out of place from
// the one before.  Table entries of a form that is not wanted are nullptr tables.  With only cosets wanted everything runs inside them.
static int kg_perm_group(Ctx* c, const KgDomain& d, const KgPerm& w, const uint32_t* const* maps, uint32_t count, Fe* const* perms,
                         Fe* const* polys, Fe* const* cosets, hipStream_t s) {
    Fe* const* sigma = perms ? perms : polys ? polys : cosets;
    std::vector<const void*> blob(2 * (size_t)count);
    for (uint32_t j = 0; j < count; j++) {
        blob[j] = maps[j];
        blob[count + j] = sigma[j];
    }
    int rc = c->stage_h2d(w.blob, blob.data(), blob.size() * sizeof(void*), s);
    if (rc) return rc;
    hipLaunchKernelGGL(kg_sigma_kernel, dim3(kg_grid(1ull << d.k), count), dim3(KG_THREADS), 0, s, (const uint2* const*)w.blob,
                       (Fe* const*)(w.blob + count * sizeof(void*)), w.tab, d.k, w.lo_bits, w.m_total, w.flag);
    H2_CHECK(hipGetLastError());
    if (!polys && !cosets) return 0;
    Fe* const* coeff = polys ? polys : cosets;
    NttScale isc = NttScale::inverse(d.divisor);
    if ((rc = ntt_device_batch(c, coeff, coeff == sigma ? nullptr : (const Fe* const*)sigma, count, d.omega_inv, d.k, &isc, s))) return rc;
    if (!cosets) return 0;
    NttScale csc = NttScale::into_coset(d.g_coset, d.g_coset_inv, 1ull << d.k);
    return ntt_device_batch(c, cosets, cosets == coeff ? nullptr : (const Fe* const*)coeff, count, d.ext_omega, d.ek, &csc, s);
}

// waits for s; H2HIP_EINVAL when a pair of the mapping was out of range
static int kg_perm_verdict(Ctx* c, const KgPerm& w, hipStream_t s) {
    int rc = c->keygen_flag.ensure(sizeof(uint32_t));
    if (rc) return rc;
    H2_CHECK(hipMemcpyAsync(c->keygen_flag.p, w.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    H2_CHECK(hipStreamSynchronize(s));
    if (*(const uint32_t*)c->keygen_flag.p) {
        set_error("permutation_keygen: a mapping pair has column >= n_columns or row >= 2^k; its sigma value was taken as zero");
        return H2HIP_EINVAL;
    }
    return 0;
}

static int kg_scatter(Ctx* c, uint64_t n, const std::vector<KgScatter>& descs, char* d_descs, const Fe* d_inv, hipStream_t s) {
    for (size_t i0 = 0; i0 < descs.size(); i0 += KG_MAX_COLUMNS) {
        const size_t cnt = descs.size() - i0 < KG_MAX_COLUMNS ? descs.size() - i0 : KG_MAX_COLUMNS;
        uint32_t most = 0;
        for (size_t i = i0; i < i0 + cnt; i++) most = descs[i].count > most ? descs[i].count : most;
        int rc = c->stage_h2d(d_descs + i0 * sizeof(KgScatter), descs.data() + i0, cnt * sizeof(KgScatter), s);
        if (rc) return rc;
        hipLaunchKernelGGL(kg_scatter_kernel, dim3(kg_grid(most), (uint32_t)cnt), dim3(KG_THREADS), 0, s,
                           (const KgScatter*)(d_descs + i0 * sizeof(KgScatter)), d_inv, n);
        H2_CHECK(hipGetLastError());
    }
    return 0;
}

static int kg_lagrange_device(Ctx* c, const KgDomain& d, uint32_t bf, Fe* l0, Fe* l_last, Fe* l_active, hipStream_t s) {
    const uint64_t n = 1ull << d.k, len = 1ull << d.ek;
    hipLaunchKernelGGL(kg_units_kernel, dim3((uint32_t)((n + KG_THREADS - 1) / KG_THREADS)), dim3(KG_THREADS), 0, s, l0, l_last, l_active, n,
                       (uint64_t)bf);
    H2_CHECK(hipGetLastError());
    Fe* cols[3] = {l0, l_last, l_active};
    NttScale isc = NttScale::inverse(d.divisor), csc = NttScale::into_coset(d.g_coset, d.g_coset_inv, 1ull << d.k);
    int rc;
    if ((rc = ntt_device_batch(c, cols, nullptr, 3, d.omega_inv, d.k, &isc, s))) return rc;
    if ((rc = ntt_device_batch(c, cols, nullptr, 3, d.ext_omega, d.ek, &csc, s))) return rc;
    hipLaunchKernelGGL(kg_active_kernel, dim3((uint32_t)((len + KG_THREADS - 1) / KG_THREADS)), dim3(KG_THREADS), 0, s, l_active, l_last, len);
    H2_CHECK(hipGetLastError());
    return 0;
}

struct KgDrain {  // every exit of a pipelined host call: the download copier idle, its stream drained
    Ctx* c;
    hipStream_t sd;
    bool on;
    ~KgDrain() {
        if (!on) return;
        copier_abort(c, true, SIZE_MAX);
        (void)hipStreamSynchronize(sd);
    }
};

}  // namespace h2

using namespace h2;

extern "C" {
// ---- C ABI (include/halo2hip.h, "keygen") -----------------------------------------------------------------------------------------
static int kg_domain_check(const char* what, uint32_t k, const uint64_t* omega, const uint64_t* omega_inv, const uint64_t* divisor, uint32_t ek,
                           const uint64_t* ext_omega, const uint64_t* g_coset, const uint64_t* g_coset_inv, KgDomain* d) {
    if (k > 28 || ek > 28 || ek < k) {
        set_error("%s: k = %u, extended_k = %u: need k <= extended_k <= 28", what, k, ek);
        return H2HIP_EINVAL;
    }
    if (!omega || !omega_inv || !divisor || !ext_omega || !g_coset || !g_coset_inv) {
        set_error("%s: null domain constant", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(omega, "omega") || check_fr(omega_inv, "omega_inv") || check_fr(divisor, "ifft_divisor") ||
        check_fr(ext_omega, "extended_omega") || check_fr(g_coset, "g_coset") || check_fr(g_coset_inv, "g_coset_inv"))
        return H2HIP_EINVAL;
    d->k = k;
    d->ek = ek;
    d->omega = fe_from_u64x4(omega);
    d->omega_inv = fe_from_u64x4(omega_inv);
    d->divisor = fe_from_u64x4(divisor);
    d->ext_omega = fe_from_u64x4(ext_omega);
    d->g_coset = fe_from_u64x4(g_coset);
    d->g_coset_inv = fe_from_u64x4(g_coset_inv);
    return 0;
}

static int kg_perm_check(uint32_t k, const uint64_t* omega, const uint64_t* omega_inv, const uint64_t* divisor, uint32_t ek,
                         const uint64_t* ext_omega, const uint64_t* g_coset, const uint64_t* g_coset_inv, const uint64_t* delta,
                         const void* const* mapping, uint32_t m, const void* const* perms, const void* const* polys, const void* const* cosets,
                         KgDomain* d) {
    const char* what = "permutation_keygen";
    if (int rc = kg_domain_check(what, k, omega, omega_inv, divisor, ek, ext_omega, g_coset, g_coset_inv, d)) return rc;
    if (!delta) {
        set_error("%s: null delta", what);
        return H2HIP_EINVAL;
    }
    if (check_fr(delta, "delta")) return H2HIP_EINVAL;
    if (m > KG_MAX_COLUMNS) {
        set_error("%s: n_columns %u > %d", what, m, KG_MAX_COLUMNS);
        return H2HIP_EINVAL;
    }
    if (check_ptrs(what, mapping, m, "mapping") || check_ptrs(what, perms, m, "permutations", true) || check_ptrs(what, polys, m, "polys", true) ||
        check_ptrs(what, cosets, m, "cosets", true))
        return H2HIP_EINVAL;
    return 0;
}

int h2hip_permutation_keygen_bn254_device(uint32_t k, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t ifft_divisor[4],
                                          uint32_t extended_k, const uint64_t extended_omega[4], const uint64_t g_coset[4],
                                          const uint64_t g_coset_inv[4], const uint64_t delta[4], const void* const* d_mapping, uint32_t n_columns,
                                          void* const* d_permutations, void* const* d_polys, void* const* d_cosets, void* stream) {
    KgDomain d;
    if (int rc = kg_perm_check(k, omega, omega_inv, ifft_divisor, extended_k, extended_omega, g_coset, g_coset_inv, delta, d_mapping, n_columns,
                               (const void* const*)d_permutations, (const void* const*)d_polys, (const void* const*)d_cosets, &d))
        return rc;
    if (n_columns == 0 || (!d_permutations && !d_polys && !d_cosets)) return 0;
    Entry en("h2hip_permutation_keygen_bn254_device", d_mapping[0]);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = (hipStream_t)stream;
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    KgPerm w;
    if ((rc = kg_perm_prepare(c, d, fe_from_u64x4(delta), n_columns, n_columns, s, &w))) return rc;
    if ((rc = kg_perm_group(c, d, w, (const uint32_t* const*)d_mapping, n_columns, (Fe* const*)d_permutations, (Fe* const*)d_polys,
                            (Fe* const*)d_cosets, s)))
        return rc;
    if ((rc = guard.release())) return rc;
    return kg_perm_verdict(c, w, s);
}

int h2hip_permutation_keygen_bn254(uint32_t k, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t ifft_divisor[4],
                                   uint32_t extended_k, const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                   const uint64_t delta[4], const uint32_t* const* mapping, uint32_t n_columns, uint64_t* const* permutations,
                                   uint64_t* const* polys, uint64_t* const* cosets) {
    KgDomain d;
    if (int rc = kg_perm_check(k, omega, omega_inv, ifft_divisor, extended_k, extended_omega, g_coset, g_coset_inv, delta,
                               (const void* const*)mapping, n_columns, (const void* const*)permutations, (const void* const*)polys,
                               (const void* const*)cosets, &d))
        return rc;
    const size_t n = (size_t)1 << k, len = (size_t)1 << extended_k;
    for (uint32_t j = 0; j < n_columns; j++)  // the mapping is host memory: a bad pair answers the same with and without a GPU
        for (size_t i = 0; i < n; i++)
            if (mapping[j][2 * i] >= n_columns || mapping[j][2 * i + 1] >= n) {
                set_error("permutation_keygen: mapping[%u][%zu] = (%u, %u) is out of range (n_columns = %u, 2^k = %zu)", j, i, mapping[j][2 * i],
                          mapping[j][2 * i + 1], n_columns, n);
                return H2HIP_EINVAL;
            }
    if (n_columns == 0 || (!permutations && !polys && !cosets)) return 0;
    Entry en("h2hip_permutation_keygen_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    // a group of columns: the mapping, the sigma table (always: the first form), the coefficients when they or the cosets are wanted, the cosets
    const bool need_poly = polys || cosets;
    const size_t map_b = n * 8, col_b = n * sizeof(Fe), ext_b = len * sizeof(Fe);
    const size_t per_col = map_b + col_b + (need_poly ? col_b : 0) + (cosets ? ext_b : 0);
    size_t gc = tune().keygen_group_bytes / per_col;
    if (gc < 1) gc = 1;
    if (gc > n_columns) gc = n_columns;
    const size_t groups = (n_columns + gc - 1) / gc;
    const size_t bufs = groups > 1 ? 2 : 1;
    int rc = c->host_io.ensure(bufs * gc * per_col);
    if (rc) return rc;
    const bool piped = groups > 1 && copier_ready(c, true);
    if (piped && (rc = c->ensure_aux(2))) return rc;
    hipStream_t sd = piped ? c->aux1 : nullptr;
    if ((rc = c->ws_acquire(s))) return rc;
    WsGuard guard(c, s);
    KgPerm w;
    if ((rc = kg_perm_prepare(c, d, fe_from_u64x4(delta), n_columns, (uint32_t)gc, s, &w))) return rc;
    if (piped) {
        H2_CHECK(hipStreamSynchronize(s));
        if ((rc = copier_begin(c, true, sd))) return rc;
    }
    KgDrain drain{c, sd, piped};
    std::vector<CopyJob> jobs;
    std::vector<size_t> jobs_through(groups, 0);
    size_t n_jobs = 0;
    for (size_t g = 0; g < groups; g++) {
        const size_t j0 = g * gc, cnt = n_columns - j0 < gc ? n_columns - j0 : gc;
        if (piped && g >= 2 && (rc = copier_wait(c, true, jobs_through[g - 2]))) return rc;  // this buffer's earlier columns have left
        char* base = (char*)c->host_io.p + (g % bufs) * gc * per_col;
        std::vector<const uint32_t*> d_map(cnt);
        std::vector<Fe*> d_perm(cnt), d_poly(cnt), d_coset(cnt);
        for (size_t j = 0; j < cnt; j++) {
            char* p = base + j * per_col;
            d_map[j] = (const uint32_t*)p;
            d_perm[j] = (Fe*)(p + map_b);
            d_poly[j] = (Fe*)(p + map_b + col_b);
            d_coset[j] = (Fe*)(p + map_b + col_b + (need_poly ? col_b : 0));
            H2_CHECK(hipMemcpyAsync(p, mapping[j0 + j], map_b, hipMemcpyHostToDevice, s));
        }
        if ((rc = kg_perm_group(c, d, w, d_map.data(), (uint32_t)cnt, d_perm.data(), need_poly ? d_poly.data() : nullptr,
                                cosets ? d_coset.data() : nullptr, s)))
            return rc;
        if (piped) {
            hipEvent_t ev = c->aux_events[g & 1];
            H2_CHECK(hipEventRecord(ev, s));
            for (size_t j = 0; j < cnt; j++) {
                if (permutations) jobs.push_back(CopyJob{permutations[j0 + j], d_perm[j], col_b, nullptr, jobs.empty() ? ev : nullptr, true});
                if (polys) jobs.push_back(CopyJob{polys[j0 + j], d_poly[j], col_b, nullptr, jobs.empty() ? ev : nullptr, true});
                if (cosets) jobs.push_back(CopyJob{cosets[j0 + j], d_coset[j], ext_b, nullptr, jobs.empty() ? ev : nullptr, true});
            }
            n_jobs += jobs.size();
            jobs_through[g] = n_jobs;
            if ((rc = copier_push(c, true, jobs))) return rc;
        } else {
            for (size_t j = 0; j < cnt; j++) {
                if (permutations) H2_CHECK(hipMemcpyAsync(permutations[j0 + j], d_perm[j], col_b, hipMemcpyDeviceToHost, s));
                if (polys) H2_CHECK(hipMemcpyAsync(polys[j0 + j], d_poly[j], col_b, hipMemcpyDeviceToHost, s));
                if (cosets) H2_CHECK(hipMemcpyAsync(cosets[j0 + j], d_coset[j], ext_b, hipMemcpyDeviceToHost, s));
            }
            H2_CHECK(hipStreamSynchronize(s));
        }
    }
    if (piped) {
        if ((rc = copier_wait(c, true, n_jobs))) return rc;
        H2_CHECK(hipStreamSynchronize(sd));
    }
    H2_CHECK(hipStreamSynchronize(s));
    return guard.release();
}

// ---- batch_invert_assigned ----------------------------------------------------------------------------------------------------------
static int kg_assigned_check(uint32_t k, const void* const* numerators, const void* const* rat_rows, const size_t* rat_counts,
                             const void* const* rat_denoms, size_t m, const void* const* out, size_t* total) {
    const char* what = "batch_invert_assigned";
    if (int rc = check_k(what, k)) return rc;
    if (check_ptrs(what, numerators, m, "numerators") || check_ptrs(what, out, m, "out")) return H2HIP_EINVAL;
    size_t t = 0;
    for (size_t j = 0; j < m; j++) {
        const size_t cnt = rat_counts ? rat_counts[j] : 0;
        if (cnt > ((size_t)1 << k)) {
            set_error("%s: rat_counts[%zu] = %zu > 2^k", what, j, cnt);
            return H2HIP_EINVAL;
        }
        if (cnt && (!rat_rows || !rat_rows[j] || !rat_denoms || !rat_denoms[j])) {
            set_error("%s: column %zu has %zu rational cells but null rat_rows or rat_denoms", what, j, cnt);
            return H2HIP_EINVAL;
        }
        t += cnt;
    }
    if (t > ((size_t)1 << 30)) {
        set_error("%s: %zu rational cells > 2^30", what, t);
        return H2HIP_EINVAL;
    }
    *total = t;
    return 0;
}

int h2hip_batch_invert_assigned_bn254_device(uint32_t k, const void* const* d_numerators, const void* const* d_rat_rows, const size_t* rat_counts,
                                             const void* const* d_rat_denoms, size_t n_columns, void* const* d_out, void* stream) {
    size_t total = 0;
    if (int rc = kg_assigned_check(k, d_numerators, d_rat_rows, rat_counts, d_rat_denoms, n_columns, (const void* const*)d_out, &total)) return rc;
    if (n_columns == 0) return 0;
    Entry en("h2hip_batch_invert_assigned_bn254_device", d_out[0]);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)1 << k;
    for (size_t j = 0; j < n_columns; j++)
        if (d_out[j] != d_numerators[j]) H2_CHECK(hipMemcpyAsync(d_out[j], d_numerators[j], n * sizeof(Fe), hipMemcpyDeviceToDevice, s));
    if (!total) return 0;
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    Carve ws;
    const size_t o_inv = ws.take(total * sizeof(Fe)), o_descs = ws.take(n_columns * sizeof(KgScatter));
    if ((rc = c->keygen_ws.ensure(ws.total))) return rc;
    Fe* inv = (Fe*)((char*)c->keygen_ws.p + o_inv);
    std::vector<KgScatter> descs;
    size_t off = 0;
    for (size_t j = 0; j < n_columns; j++) {
        const size_t cnt = rat_counts[j];
        if (!cnt) continue;
        H2_CHECK(hipMemcpyAsync(inv + off, d_rat_denoms[j], cnt * sizeof(Fe), hipMemcpyDeviceToDevice, s));
        descs.push_back(KgScatter{(Fe*)d_out[j], (const uint32_t*)d_rat_rows[j], off, (uint32_t)cnt, 0});
        off += cnt;
    }
    if ((rc = batch_invert_device(c, inv, total, s))) return rc;
    if ((rc = kg_scatter(c, n, descs, (char*)c->keygen_ws.p + o_descs, inv, s))) return rc;
    return guard.release();
}

int h2hip_batch_invert_assigned_bn254(uint32_t k, const uint64_t* const* numerators, const uint32_t* const* rat_rows, const size_t* rat_counts,
                                      const uint64_t* const* rat_denoms, size_t n_columns, uint64_t* const* out) {
    size_t total = 0;
    if (int rc = kg_assigned_check(k, (const void* const*)numerators, (const void* const*)rat_rows, rat_counts, (const void* const*)rat_denoms,
                                   n_columns, (const void* const*)out, &total))
        return rc;
    const size_t n = (size_t)1 << k;
    for (size_t j = 0; j < n_columns; j++) {
        const size_t cnt = rat_counts ? rat_counts[j] : 0;
        for (size_t t = 0; t < cnt; t++) {
            if (rat_rows[j][t] >= n || (t && rat_rows[j][t] <= rat_rows[j][t - 1])) {
                set_error("batch_invert_assigned: rat_rows[%zu][%zu] = %u is out of range or not ascending", j, t, rat_rows[j][t]);
                return H2HIP_EINVAL;
            }
            if (check_fr(rat_denoms[j] + 4 * t, "a denominator")) return H2HIP_EINVAL;
        }
    }
    if (n_columns == 0) return 0;
    const size_t col_b = n * sizeof(Fe);
    // a column without a Rational cell is its numerators: it never crosses PCIe (the prover's advice columns are mostly such)
    std::vector<size_t> rat_cols;
    for (size_t j = 0; j < n_columns; j++) {
        if (rat_counts && rat_counts[j])
            rat_cols.push_back(j);
        else if (out[j] != numerators[j])
            memcpy(out[j], numerators[j], col_b);
    }
    if (rat_cols.empty()) {
        // without a GPU the call still fails loudly, as every compute entry point does
        Entry en("h2hip_batch_invert_assigned_bn254");
        return en.rc;
    }
    Entry en("h2hip_batch_invert_assigned_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    // the sparse part whole (one inversion over all columns, poly.rs:192-200), the columns that have Rational cells in groups
    size_t gc = tune().keygen_group_bytes / col_b;
    if (gc < 1) gc = 1;
    if (gc > rat_cols.size()) gc = rat_cols.size();
    Fe* inv = nullptr;
    uint32_t* rows = nullptr;
    char* cols = nullptr;
    HostIo io(c, c->host_io, s, true);
    const size_t o_inv = io.room(total * sizeof(Fe), &inv), o_rows = io.room(total * sizeof(uint32_t), &rows);
    io.aligned = false;  // the columns of a group lie packed
    const size_t o_cols = io.room(gc * col_b, &cols);
    std::vector<size_t> offs(rat_cols.size(), 0);
    size_t off = 0;
    for (size_t q = 0; q < rat_cols.size(); q++) {
        const size_t j = rat_cols[q], cnt = rat_counts[j];
        offs[q] = off;
        io.in_at(rat_denoms[j], cnt * sizeof(Fe), o_inv + off * sizeof(Fe));
        io.in_at(rat_rows[j], cnt * sizeof(uint32_t), o_rows + off * sizeof(uint32_t));
        off += cnt;
    }
    int rc = c->ws_acquire(s);
    if (rc) return rc;
    WsGuard guard(c, s);
    if ((rc = c->keygen_ws.ensure(align256(gc * sizeof(KgScatter))))) return rc;
    if ((rc = io.upload())) return rc;
    if ((rc = batch_invert_device(c, inv, total, s))) return rc;
    for (size_t q0 = 0; q0 < rat_cols.size(); q0 += gc) {  // one round of the staging per group, over the same slots
        const size_t cnt = rat_cols.size() - q0 < gc ? rat_cols.size() - q0 : gc;
        std::vector<KgScatter> descs;
        for (size_t q = 0; q < cnt; q++) {
            const size_t j = rat_cols[q0 + q];
            io.in_at(numerators[j], col_b, o_cols + q * col_b);
            io.out_at(out[j], col_b, o_cols + q * col_b);
            descs.push_back(KgScatter{(Fe*)(cols + q * col_b), rows + offs[q0 + q], offs[q0 + q], (uint32_t)rat_counts[j], 0});
        }
        if ((rc = io.upload())) return rc;
        if ((rc = kg_scatter(c, n, descs, (char*)c->keygen_ws.p, inv, s))) return rc;
        if ((rc = io.finish())) return rc;
    }
    return guard.release();
}

// ---- l0, l_last, l_active_row -------------------------------------------------------------------------------------------------------
static int kg_lagrange_check(uint32_t k, const uint64_t* omega_inv, const uint64_t* divisor, uint32_t ek, const uint64_t* ext_omega,
                             const uint64_t* g_coset, const uint64_t* g_coset_inv, uint32_t bf, const void* l0, const void* l_last,
                             const void* l_active, KgDomain* d) {
    const char* what = "key_lagrange_columns";
    if (int rc = kg_domain_check(what, k, omega_inv, omega_inv, divisor, ek, ext_omega, g_coset, g_coset_inv, d)) return rc;
    if (int rc = check_k_blinding(what, k, bf)) return rc;  // (k itself has passed kg_domain_check)
    if (!l0 || !l_last || !l_active) {
        set_error("%s: null output", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

int h2hip_key_lagrange_columns_bn254_device(uint32_t k, const uint64_t omega_inv[4], const uint64_t ifft_divisor[4], uint32_t extended_k,
                                            const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                            uint32_t blinding_factors, void* d_l0, void* d_l_last, void* d_l_active_row, void* stream) {
    KgDomain d;
    if (int rc = kg_lagrange_check(k, omega_inv, ifft_divisor, extended_k, extended_omega, g_coset, g_coset_inv, blinding_factors, d_l0, d_l_last,
                                   d_l_active_row, &d))
        return rc;
    Entry en("h2hip_key_lagrange_columns_bn254_device", d_l0);
    if (en.rc) return en.rc;
    return kg_lagrange_device(en.c, d, blinding_factors, (Fe*)d_l0, (Fe*)d_l_last, (Fe*)d_l_active_row, (hipStream_t)stream);
}

int h2hip_key_lagrange_columns_bn254(uint32_t k, const uint64_t omega_inv[4], const uint64_t ifft_divisor[4], uint32_t extended_k,
                                     const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                     uint32_t blinding_factors, uint64_t* l0, uint64_t* l_last, uint64_t* l_active_row) {
    KgDomain d;
    if (int rc = kg_lagrange_check(k, omega_inv, ifft_divisor, extended_k, extended_omega, g_coset, g_coset_inv, blinding_factors, l0, l_last,
                                   l_active_row, &d))
        return rc;
    Entry en("h2hip_key_lagrange_columns_bn254");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    hipStream_t s = c->stream;
    const size_t ext_b = sizeof(Fe) << extended_k;
    Fe *d_l0 = nullptr, *d_l_last = nullptr, *d_l_active = nullptr;
    HostIo io(c, c->host_io, s);
    io.out(l0, ext_b, &d_l0);
    io.out(l_last, ext_b, &d_l_last);
    io.out(l_active_row, ext_b, &d_l_active);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = kg_lagrange_device(c, d, blinding_factors, d_l0, d_l_last, d_l_active, s))) return rc;
    return io.finish();
}

int h2hip_debug_set_keygen_group(uint64_t group_bytes) {
    TuneWrite()->keygen_group_bytes = group_bytes ? (size_t)group_bytes : Tuning{}.keygen_group_bytes;
    return 0;
}

}  // extern "C"
