// engine.h -- internal (not installed) declarations shared by the translation units of
// libhalo2hip.so: device context, workspace arena, per-stage HIP-event timers, error plumbing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/halo2hip.h"
#include "ecu.h"

namespace h2 {

void set_error(const char* fmt, ...);

#define H2_CHECK(expr)                                                                             \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            h2::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));    \
            return 2;                                                                              \
        }                                                                                          \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
};

// grow-only pinned host buffer
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
};

struct TwiddleKey {
    uint32_t omega[8];
    uint32_t log_n;
    bool operator<(const TwiddleKey& o) const {
        for (int i = 0; i < 8; i++)
            if (omega[i] != o.omega[i]) return omega[i] < o.omega[i];
        return log_n < o.log_n;
    }
};

struct TwiddleTable {
    Fu* lo = nullptr;  // omega^i, i < 2^lo_bits                                  (I-form limbs, fieldu.h)
    Fu* hi = nullptr;  // omega^(i << lo_bits), i < 2^(log_n - lo_bits) (at least 1 entry)
    uint32_t lo_bits = 0;
    // the tile DFT's own twiddles w_R^i, i < R / 2, for R = 2^s (ntt.hip get_stage_twiddles): one table per radix a plan has used on
    // this domain.  Keyed by s, not by plan: a lone transform and a batch of the same domain take different plans (three passes /
    // two), and until round 4 every switch freed and rebuilt the other plan's tables behind a device-wide synchronisation.
    Fu* stage_of[13] = {};
    // the inter-pass twiddles of a pass as one table, when the budget allows (ntt.hip get_full_twiddles); tag = layout << 31 |
    // scaled << 30 | log_m << 8 | s (layout 1: the two-pass plan's pass 1; scaled: every entry times full_scale[k], the 1/n of the inverse
    // transform that uses this domain -- its last pass then closes with the direct reduction instead of a multiplication).  Up to
    // H2_TW_FULL tables per domain, none is ever replaced.
#define H2_TW_FULL 12
    Fu* full[H2_TW_FULL] = {};
    uint32_t full_tag[H2_TW_FULL] = {};
    Fe full_scale[H2_TW_FULL] = {};
    // `lo` times one constant (the 1/n of the inverse transform that uses this domain): a first pass that combines its inter-pass
    // twiddles from the two-level table then scales for free, and the last pass closes with the direct reduction (ntt.hip ntt_run)
    Fu* lo_scaled = nullptr;
    Fe lo_scale;
};

// Fixed-base window table of a pinned base array (msm.hip): row j (of `stride` points) = 2^(c j) * P, j < W
struct MsmTable {
    const void* table = nullptr;
    size_t stride = 0;
    uint32_t c = 0, W = 0;
    uint32_t rec = 64;  // bytes from one record to the next: 64 = E-form Affine, otherwise native records (ecu.h AffineU) at that stride (128; 80 for A/B)
};

// Record form of the window tables.  Native records (80 bytes of limbs, one per 128-byte line) spare the accumulation the slicing of
// both coordinates, the branch around the negation and the first point's two products.  Packed at 80 bytes they straddle the 64-byte
// sectors and the gathers cost more than the instructions save ("Native table records"), so the stride is a line.  Below
// 2^13 points the MSM is all reduction tail (msm_table_window), a table twice the size buys nothing, and it stays E-form.
// `forced`: h2hip_debug_set_table_records (0 = no wish).
#define H2_TABLE_REC_NATIVE 128u
#define H2_TABLE_NATIVE_MIN_N ((size_t)1 << 13)
static inline uint32_t msm_table_rec(size_t n, uint32_t forced) { return forced ? forced : n >= H2_TABLE_NATIVE_MIN_N ? H2_TABLE_REC_NATIVE : 64u; }

#define H2_GATHER_OWN ((size_t)64 << 10)  // bytes of Ctx::gather a device's own set sums may take; the gathered ones follow
#define H2_PIN_SAMPLES 16
// index of fingerprint sample k of an array of `total` points
static inline __host__ __device__ size_t pin_sample_index(size_t total, uint32_t k) { return k == 0 ? 0 : (total - 1) >> (H2_PIN_SAMPLES - 1 - k); }
// One entry of the pinned-bases cache, keyed by the caller's pointer (host or device).
struct PinnedBases {
    void* d = nullptr;         // device copy: W x n records with the window table, or n points without one
    size_t n = 0;              // points per row
    uint32_t c = 0, W = 0;     // window width of the table; 0: no table (rows = 1)
    uint32_t rec = 64;         // bytes per record of the table (MsmTable::rec); without a table the points are E-form Affine
    bool device_key = false;   // the key is a device pointer (h2hip_bases_pin_device)
    // fingerprint of the caller's array at pin time: H2_PIN_SAMPLES points (pin_sample_index: the first one and a geometric
    // ladder up to the last, so that every prefix length still sees several), compared byte for byte on every lookup -- a
    // freed-and-reused allocation at the same address must not hit the stale copy.  Host keys: compared on the host
    // (pinned_validate); device keys: d_sample holds the same bytes in device memory and the first workgroup of the MSM's first
    // kernel compares them with the caller's buffer (Ctx::pin_chk -> msm_l1_count_kernel), its verdict is read when the MSM's own result arrives.
    uint8_t sample[H2_PIN_SAMPLES * 64];
    void* d_sample = nullptr;
    size_t lo = 0, hi = 0;     // multi-GPU: this device holds points [lo, hi) of the caller's array (n = hi - lo)
};

struct Ctx;

// ---- the pin cache (api.hip): a proving key's constant data kept in HBM across evaluate_h calls, under one budget
// (HALO2_HIP_COLUMN_CACHE_GB) and one LRU clock.  Two kinds of entry, keyed by (kind, the caller's pointer), so that the same pointer
// may be pinned as both:
//   COLUMN  h2hip_columns_pin: a column in evaluation form (pk.fixed_cosets, pk.l0 / l_last / l_active_row, pk.permutation.cosets),
//           `elems` elements, keyed by its host pointer;
//   PARTS   h2hip_part_cosets_pin (evalh.hip builds them): all P = 2^(ek - k) part cosets of one coefficient-form polynomial,
//           part-major -- part p is the 2^k elements at d + p * 2^k --, keyed by a host or a device pointer and tagged with the domain.
// A host key is guarded by a fingerprint as the pinned bases are: H2_COL_SAMPLES sampled elements of the caller's `elems`-element array
// (column_sample), compared on every lookup, so a freed and reused allocation at the same address misses; a device key rests on the
// caller's contract, because the device form never waits for a verdict.
#define H2_COL_SAMPLES 16
struct PinDomain {  // what a PARTS entry was built for; all zero in a COLUMN entry
    uint32_t k = 0, ek = 0;
    Fe ext_omega = {}, g_coset = {};
    bool operator==(const PinDomain& o) const {
        return k == o.k && ek == o.ek && memcmp(&ext_omega, &o.ext_omega, sizeof(Fe)) == 0 && memcmp(&g_coset, &o.g_coset, sizeof(Fe)) == 0;
    }
};
struct Pin {
    int kind = 0;               // PinCache::Kind
    const void* key = nullptr;  // the caller's pointer
    void* d = nullptr;
    size_t bytes = 0;
    size_t elems = 0;  // elements of the caller's array, the length the fingerprint sampled: the column's, or 2^k coefficients
    bool device_key = false;
    PinDomain dom;
    uint64_t last_use = 0;
    uint8_t sample[H2_COL_SAMPLES * 32] = {};
};
struct PinCache {
    enum Kind { COLUMN = 0, PARTS = 1 };
    std::map<std::pair<int, const void*>, Pin> pins;
    size_t count[2] = {0, 0}, bytes[2] = {0, 0};  // by kind
    uint64_t tick = 0;
    Pin* find(Kind kind, const void* key);
    // the device copy of `key` for this call, or nullptr.  An entry with the other kind of key or another domain is not this call's and
    // stays.  A host key whose array has another length now, or other sampled elements, is dropped (behind a device synchronisation: a
    // queued call may still read it).  A hit advances the clock.  COLUMN: dev = false, dom = PinDomain().
    const Fe* lookup(Kind kind, const void* key, bool dev, size_t elems, const PinDomain& dom);
    // room for `need` more bytes within `budget`: least recently used entries of either kind are dropped, each behind a device
    // synchronisation, until it fits.  *fits = false: `need` exceeds the whole budget, nothing was dropped.
    int make_room(size_t need, size_t budget, bool* fits);
    // list p (kind, key, d, bytes, elems, device_key, dom set by the caller, d filled and complete; no entry of that kind and key is
    // listed): takes a host key's fingerprint and stamps the clock
    void insert(Pin p);
    // The one place a pin's device memory is freed and its bytes leave the count.  p is a listed entry -- the caller has synchronised
    // the device if a queued kernel may read it, once per public call is enough -- or one whose upload or build failed before insert().
    void drop(Pin* p);
    void clear();  // release_ctx, behind its device synchronisation
};

struct StageTimer {
    std::string name;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double total_ms = 0.0;
    uint64_t count = 0;
    bool pending = false;
};

// ---- copier threads (api.hip): hipMemcpyAsync to or from the caller's pageable memory moves at PCIe speed but returns only
// when its piece has crossed, so the thread that enqueues kernels must not sit in it.  Each device context has two helper
// threads, one per direction (PCIe is full duplex: the uploads of column i + 1 and the downloads of column i - 1 overlap).
// A copier walks a job queue in order; per job: wait for `gate` on its stream (an event the enqueueing thread has already
// recorded), copy, record `ev`, bump `done`.  Users: the streamed host-slice MSM (msm.hip) and the host-pointer batched
// transforms (api.hip, ntt_host_batch).
struct CopyJob {
    void* dst;
    const void* src;
    size_t bytes;
    hipEvent_t ev;    // recorded on the copy stream after this job; nullptr: none
    hipEvent_t gate;  // the copy stream waits for it before this job; nullptr: none
    bool d2h;
};
struct Copier;
// begin a session on c's upload (down = false) or download (down = true) copier -- started on first use --: `done` and the
// error state are reset, later jobs go to `stream`.  H2HIP_ENOMEM / H2HIP_EDEVICE when the thread cannot be started.
bool copier_ready(Ctx* c, bool down);  // the thread exists (started now if need be); false: it cannot be started, take the unstreamed path
int copier_begin(Ctx* c, bool down, hipStream_t stream);
// append jobs to the session (the vector is left empty)
int copier_push(Ctx* c, bool down, std::vector<CopyJob>& jobs);
// block until the first n_jobs jobs of the session have been issued (for pageable memory: have crossed); non-zero: a copy failed
int copier_wait(Ctx* c, bool down, size_t n_jobs);
// error-path drain: the jobs not yet started are skipped, the call returns once the copier no longer touches the caller's memory
void copier_abort(Ctx* c, bool down, size_t n_jobs);

struct Ctx {
    int device = -1;
    bool ready = false;
    hipStream_t stream = nullptr;  // the engine's own stream (host-pointer entry points)
    std::recursive_mutex mu;       // serialises entry points: re-entrant callers (rayon workers) are safe
    DevBuf ntt_ws, ntt_io, msm_scalars[3], msm_bases, msm_slot[3], misc, evalh_ws, evalh_slots, ecfft_ws, ntt_ptrs, gather, gen_table;
    DevBuf host_io;                // every stage file's host-pointer forms: the caller's columns on their way in and out (HostIo, below)
    DevBuf prod_ws;                // product.hip: scans' workspace
    DevBuf mvsum_ws;               // product.hip: the mv-lookup grand sum's denominators, partial sums and descriptors
    DevBuf open_ws, open_io;       // opening.hip: scans' workspace and tables; the evaluations of both forms of eval_polynomials
    DevBuf lookup_ws;              // lookup.hip: sort keys, marks and scans
    HostBuf lookup_flag;           // lookup.hip: the per-lookup not-found flags read back at the end of a permute call
    DevBuf keygen_ws;              // keygen.hip: power tables, flag, pointer blobs and inverses
    HostBuf keygen_flag;           // keygen.hip: the out-of-range flag of a permutation keygen read back at the end of the call
    DevBuf check_ws;               // check.hip: failure masks, tile counts, row lists and sort keys
    HostBuf check_flag;            // check.hip: the out-of-range flag of a permutation check read back at the end of the call
    DevBuf copies_ws;              // copies.hip: parents, sort keys, flag and pointer blob
    HostBuf copies_flag;           // copies.hip: the invalid-copy flag of a device-form mapping call read back at the end of the call
    DevBuf serde_ws;               // serde.hip: failure mask, tile counts and the two result words
    DevBuf ipa_ws;                 // ipa.hip: the byte table, the blocks' partial inner products and the two values
    HostBuf ipa_vals;              // ipa.hip: the two inner products read back at the end of a call
    HostBuf host_ws;               // pinned host memory for the window sums coming back
    HostBuf host_planes;           // ... and for the bit-plane sums of a run whose tail the host finishes (msm.hip msm_planes_finish)
    HostBuf pin_flag;              // one word the device-key fingerprint check writes its verdict to
    // a fingerprint check the next MSM run's first kernel carries out (msm_l1_count_kernel's first workgroup: no launch of its own);
    // set by msm_device_keyed around its msm_batch_device call, taken by the first msm_stage_a
    struct PinCheck {
        const Affine* bases = nullptr;
        const Affine* samples = nullptr;
        uint32_t* flag = nullptr;
        size_t n = 0, total = 0;
    } pin_chk;
    uint32_t table_rec = 64;       // record stride of the table msm_table_build is to write (MsmTable::rec); set by pin_on_device around its call
    // Small host tables the kernels read (pointer lists, constants) go through this pinned ring, so that the
    // asynchronous copy never reads a caller's stack or a std::vector that is gone by the time the DMA runs.
    HostBuf stage;
    size_t stage_off = 0;
    int stage_h2d(void* d_dst, const void* h_src, size_t bytes, hipStream_t s);
    std::map<TwiddleKey, TwiddleTable> twiddles;
    size_t tw_full_bytes = 0;  // HBM held by the two-pass plan's full inter-pass twiddle tables
    std::map<const void*, PinnedBases> pinned;
    PinCache pins;  // h2hip_columns_pin, h2hip_part_cosets_pin: both forms of evaluate_h find a proving key's constant data here
    // profiling
    bool profiling = false;        // every stage bracketed by a pair of events (each record costs the stream ~10 us)
    bool profiling_kernel = false; // only the dominant kernel, timed through its own dispatch (hipExtLaunchKernelGGL): no gap
    std::vector<StageTimer> timers;
    int timer_begin(const char* name, hipStream_t s);
    void timer_end(int id, hipStream_t s);
    int timer_kernel(const char* name, hipEvent_t* e0, hipEvent_t* e1);  // events for hipExtLaunchKernelGGL; -1: not profiling
    void timers_collect();
    int sm_count = 256;
    // The workspaces above are shared by every call.  Calls are serialised on the host by `mu`, but
    // device entry points return while their kernels are still queued; a later call on a different
    // stream first waits (on the device) for the previous user's last kernel.
    hipEvent_t ws_event = nullptr;
    hipStream_t ws_last_stream = nullptr;
    bool ws_used = false;
    int ws_acquire(hipStream_t s);
    int ws_release(hipStream_t s);
    // internal streams + events for the MSM's window-group pipeline
    hipStream_t aux1 = nullptr, aux2 = nullptr, aux_b = nullptr;
    std::vector<hipEvent_t> aux_events;
    int ensure_aux(size_t n_events);
    // evalh.hip: the per-circuit gates kernels loaded on this device, by source hash -> (hipModule_t, hipFunction_t); a pair of nulls
    // marks a code object that would not load here
    std::map<uint64_t, std::pair<void*, void*>> evalh_mods;
    Copier* copier[2] = {nullptr, nullptr};  // [0] uploads, [1] downloads; created on first use, joined by copier_stop (release_ctx)
    // multi-device engine, HALO2_HIP_GATHER=rccl: stage C also leaves the run's set sums in `gather` (device memory), from where
    // ncclAllGather takes them; gather_off counts the bytes left there by this call (SIZE_MAX / 2 and up: not one run, unusable)
    bool gather_want = false;
    size_t gather_off = 0;
};

void copier_stop(Ctx* c);

// Between ws_acquire and ws_release a call owns the shared workspaces.  An error return in between must not leave kernels
// queued on the internal streams unaccounted for: the guard drains them and still records the release, so the next
// call (on whatever stream) waits for everything this one started.
struct WsGuard {
    Ctx* c;
    hipStream_t s;
    bool done = false;
    WsGuard(Ctx* c_, hipStream_t s_) : c(c_), s(s_) {}
    int release() {
        done = true;
        return c->ws_release(s);
    }
    ~WsGuard() {
        if (done) return;
        if (c->aux1) (void)hipStreamSynchronize(c->aux1);
        if (c->aux2) (void)hipStreamSynchronize(c->aux2);
        if (c->aux_b) (void)hipStreamSynchronize(c->aux_b);
        (void)hipStreamSynchronize(s);
        (void)c->ws_release(s);
    }
};

// api.hip: the guard every entry point takes -- the engine initialised and held shared, the context's lock, hipSetDevice, a roctx range.
// d_ptr: a device pointer of the call, or nullptr; with several devices the call runs on the device that owns it.
// all_devices: the call reads or changes every device's state (pinned caches, multi-device MSM).  rc != 0: the call must return it.
struct Entry {
    Ctx* c;
    std::shared_lock<std::shared_mutex> engine;
    std::vector<std::unique_lock<std::recursive_mutex>> held;  // the contexts this call owns, in list order
    int rc;
    bool ranged = false;
    explicit Entry(const char* name = nullptr, const void* d_ptr = nullptr, bool all_devices = false);
    ~Entry();
};
int check_fr(const uint64_t v[4], const char* what);  // H2HIP_EINVAL (and set_error) unless v is a reduced Fr element

// ---- tuning: every knob of the library, its default written once, here.  One instance lives in api.hip (which is also built alone,
// against the stub runtime).  The rule: an entry point reads tune() under the engine lock its Entry holds shared; a hook that reads
// without an Entry takes a TuneRead; a setter hook validates its arguments, takes a TuneWrite and assigns -- "0 restores the default"
// is Tuning{}.member.  read_config (api.hip) writes the environment-backed members under h2hip_init's exclusive lock.  The settings
// survive h2hip_shutdown; the environment-backed ones are read again at the next init.
struct Tuning {
    // -- MSM: plan and sort
    uint32_t msm_window = 0;      // h2hip_set_msm_window / HALO2_HIP_MSM_WINDOW: forced window width (0 = by size, plain_window / msm_table_window)
    size_t msm_heavy_div = 32768;  // buckets with more than (entries of the MSM) / this entries take the chunked path (make_plan)
    size_t msm_bin_entries = 8192;  // target entries per coarse bin of the two-level sort
    bool msm_split_records = true;  // level-1 records of runs with multi-tile bins as two arrays, or as (entry, bucket id) pairs (msm_l2_kernel)
    bool msm_split_buckets = true;  // several lanes per bucket in runs with few buckets, or always one
    size_t msm_max_chunk = (size_t)1 << 26;  // inputs above this many pairs are split into consecutive chunks: the 31-bit pair-index limit
    // -- MSM: reduction
    uint64_t msm_rowcol_lanes = 65536;  // lane budget of the first row/column pass: one wave per SIMD (rowcol_jobs)
    bool msm_quad_tail = true;   // the reduction tail with one quad of lanes per group operation, or one lane
    bool msm_plane_tail = true;  // runs with at most 4 bucket sets finish the reduction on the host from bit-plane sums, or keep the GPU tail
    // -- MSM: host-resident scalars (msm.hip, "the upload runs under the work": the sweep behind chunks and ratio is quoted there)
    uint32_t msm_stream_chunks = 0;  // pieces a streamed MSM is cut into; 1 = no streaming; 0 = by size: three, two below 2^20 pairs (stream_chunks)
    double msm_stream_ratio = 0.6;   // upload time over compute time per pair: the chunk sizes grow by its inverse
    size_t msm_stream_min_n = (size_t)1 << 19;  // 2^19 pairs: 1.13 -> 1.04 ms (two chunks); 2^18: 0.72 -> 0.80 ms, not worth it
    // -- MSM: batches.  measured (tools/fuse_big.py, 8 MSMs per batch, per MSM): 2^19 pairs fused 0.66 ms / pipelined 0.69 ms, 2^20 pairs
    // fused 1.24 / pipelined 1.16
    size_t msm_fuse_entries = (size_t)1 << 26, msm_fuse_max_n = (size_t)1 << 19;  // entries a fused run holds at most; pairs per MSM up to which batches are fused
    bool msm_fuse_small = true;  // batches of small MSMs run fused, or pipelined over streams
    // -- pins (api.hip)
    uint32_t table_records = 0;   // record form of the window tables pinned from now on (msm_table_rec): 0 = the engine's choice
    uint32_t lazy_pin_after = 0;  // HALO2_HIP_LAZY_PIN=k: a host bases array seen k times unpinned is pinned by the library (0 = never)
    // -- NTT: plans
    uint32_t ntt_smax = 8;  // largest log2 tile of a pass.  measured (tools/ntt_sweep.py): 256-point tiles are best up to 2^24; beyond, 512-point
                            // tiles save a whole pass, and while this is at its default plan_passes takes 9 there
    // Sizes 2^lo..2^hi take the two-pass plan (tiles of 2^10 or 2^11 points, ntt2_*_kernel): measured on MI355X
    // (tools/ntt_two_pass.py) 14 % faster than three passes at 2^20, 9 % at 2^21, 5 % at 2^22 with two columns per workgroup, 25 / 19 / 12 % with one
    // (round 3); below 2^19 a lone transform brings too few workgroups.
    // Batched columns of 2^17 / 2^18 points take it too once the batch brings ntt_two_batch_wgs workgroup pairs per pass (tools/ntt_batch_rate.py, with one
    // column per workgroup: a lone 2^18 transform 0.068 against 0.052 ms for three passes, two of them 0.041 against 0.048 each; four of 2^17 0.021 / 0.026;
    // a lone 2^19 already 0.078 / 0.091).
    uint32_t ntt_two_lo = 19, ntt_two_hi = 22, ntt_two_batch_lo = 17;
    uint64_t ntt_two_batch_wgs = 512;
    int ntt_two_log_j = -1;  // log2 columns per workgroup of the two-pass kernels (-1 = the plan's choice)
    // -- NTT: twiddle tables
    uint64_t ntt_full_budget = (uint64_t)4 << 30;  // HALO2_HIP_NTT_TWIDDLE_MB: HBM the full inter-pass tables may take per device (of 288 GB); 0 = two-level table only
    // Strided passes of the three-pass plan read their inter-pass twiddles from a table of up to 2^this entries (36 B each: 0.3 / 0.6 GB per domain
    // and direction at 2^23 / 2^24 for the first pass's, 2.4 MB for the second's) while the budget lasts: one multiplication per point fewer than
    // combining the two-level table (2^23 -5 %, 2^24 -2.5 %; at 2^25 and beyond the pass has no memory bandwidth to spare for it and nothing is gained).
    uint32_t ntt_full_max_log_m = 24;
    bool ntt_fold_tables = true;  // the inverse's 1/n rides in a scaled copy of the first pass's table; off: the last pass multiplies it in (rounds 1-3)
    // -- NTT: batches
    size_t ntt_batch_bytes = (size_t)2 << 30;       // columns + workspace one batched launch may span (ntt_device_batch)
    size_t ntt_host_batch_bytes = (size_t)4 << 30;  // host-pointer batches: device memory one pipelined run may hold; larger batches are cut into runs
    size_t ntt_host_group_bytes = (size_t)2 << 20;  // ... and columns smaller than this are grouped per pipeline step
    // -- evaluate_h.  codegen: the per-circuit gates kernel -- 0 off, 1 compiled on a background thread (HALO2_HIP_EVALH_CODEGEN), 2 inline (tests)
    int evalh_codegen = 1;
    // Programs beyond these stay with the interpreter.  hiprtc takes ~20 ms per operation (0.6 s for a dozen, 4 s for 190, 7 s for 315:
    // every field multiplication is ~200 inlined instructions), and a program with many values alive at once spends minutes in the
    // register allocator (100 live slots = 900 VGPRs of state: 205 s) for a kernel that would spill anyway (EVALH_CODEGEN_MAX_SLOTS).
    uint32_t evalh_codegen_max_ops = 1200;
    bool evalh_gen_fuse = true;  // two products meeting in a sum share one reduction (gen_source); codegen mode + 16 turns it off (A/B, tests)
    // the stages whose arguments get a generated kernel of their own beside the gates and the halo2 lookups (gen_stage_source): the default
    // set is what the measurement of DESIGN.md 5 decided; codegen mode + 32 turns both off, + 64 both on
    bool evalh_gen_shuffle = true, evalh_gen_mvlookup = true;
    uint32_t evalh_max_local_slots = 256;  // programs needing more slots use the global-workspace form of the kernels (tests force it)
    size_t evalh_lookup_group_bytes = (size_t)2 << 30;  // HBM one group of lookup cosets may take (tests shrink it to force several groups)
    bool evalh_part_fused = false;  // parts form: the unpinned columns' coset scaling in the transform's first-pass load (ntt_part_device_batch), or evalh_part_scale_kernel + plain transform (DESIGN.md 5 has the A/B)
    // -- the smaller stages
    bool ecfft_quad = true, ecfft_lazy = true;  // g_to_lagrange / fft_g1 up to k = 14: one quad of lanes per butterfly; the points stay XYZZ between the layers
    uint32_t lookup_sort_block = 0;  // forced in-LDS sort block of the lookup permutation (0 = LK_TILE)
    uint32_t open_rows = 0, open_threads = 0;  // opening: forced tile shape, rows per thread and threads per tile (0 = by size)
    size_t keygen_group_bytes = (size_t)1 << 30;  // HBM one group of columns of a host-pointer keygen call may take (two groups are alive)
    size_t ipa_quad_max_half = (size_t)1 << 13;  // h2hip_ipa_set_collapse_quad: a collapse of at most this many points per half takes one quad of lanes per point
    bool ipa_round_call = true;  // h2hip_ipa_set_round_call: the wrappers' openings run one h2hip_ipa_round call per round, or the separate calls
    size_t random_min_n = 0;  // element count from which the host forms of the randomness go to the device (0 = HALO2_HIP_RANDOM_MIN_N or its default, random.hip)
};
const Tuning& tune();
// h2hip_debug_set_evalh_codegen(mode, max_ops) and HALO2_HIP_EVALH_CODEGEN=mode: bits 0-3 the mode, + 16 without the fusion, the two-bit
// field at + 32 / + 64 the stage kernels (0 = the default set, + 32 none, + 64 both); max_ops 0 restores the default
inline void evalh_codegen_apply(Tuning* t, int mode, uint32_t max_ops) {
    t->evalh_codegen = mode & 15;
    t->evalh_gen_fuse = !(mode & 16);
    const int stages = (mode >> 5) & 3;
    t->evalh_gen_shuffle = stages == 0 ? Tuning{}.evalh_gen_shuffle : stages >= 2;
    t->evalh_gen_mvlookup = stages == 0 ? Tuning{}.evalh_gen_mvlookup : stages >= 2;
    t->evalh_codegen_max_ops = max_ops ? max_ops : Tuning{}.evalh_codegen_max_ops;
}
// A setter's hold on the settings: the engine lock taken exclusively, as h2hip_shutdown takes it, so it waits for every running call and
// the next one sees the new value.  It does not initialise the engine, touches no GPU and opens no roctx range.  Not from inside a
// call that holds an Entry or a TuneRead (a callback of the library): that would wait for itself.
struct TuneWrite {
    std::unique_lock<std::shared_mutex> engine;
    TuneWrite();
    Tuning* operator->() const;
};
// ... and a query hook's, which reads tune() without an Entry: the lock shared, again without initialising anything
struct TuneRead {
    std::shared_lock<std::shared_mutex> engine;
    TuneRead();
};

// ---- what the stage files' entry points and host drivers share (inline: api.hip is also built alone, as plain C++ against a stub
// runtime, for the sanitizer runs of the engine's host logic).  The rule that build rests on: a stage file owns the extern "C" entry
// points and the h2hip_debug_* hooks of its stage, api.hip keeps the engine and the entry points whose host logic is the engine's own, and
// what it calls in a stage file tests/cpp/engine_stubs.cpp stands in for. -----------------------------------------------------------
// caller memory is only 8-byte aligned (4 x u64); Fe is alignas(16)
inline Fe fe_from_u64x4(const uint64_t v[4]) {
    Fe o;
    memcpy(o.l, v, 32);
    return o;
}
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// a table of `count` pointers, none of them null; nullable: the table itself may be absent (an output form that is not wanted)
inline int check_ptrs(const char* what, const void* const* p, size_t count, const char* name, bool nullable = false) {
    if (!p) {
        if (nullable || !count) return 0;
        set_error("%s: null %s", what, name);
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < count; i++)
        if (!p[i]) {
            set_error("%s: %s[%zu] is null", what, name, i);
            return H2HIP_EINVAL;
        }
    return 0;
}
// an array of `count` reduced Fr elements
inline int check_frs(const char* what, const uint64_t* v, size_t count, const char* name) {
    if (count && !v) {
        set_error("%s: null %s", what, name);
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < count; i++)
        if (check_fr(v + 4 * i, name)) return H2HIP_EINVAL;
    return 0;
}
// columns of 2^k rows, k <= 28 ...
inline int check_k(const char* what, uint32_t k) {
    if (k > 28) {
        set_error("%s: k = %u > 28", what, k);
        return H2HIP_EINVAL;
    }
    return 0;
}
// ... of which the last blinding_factors + 1 are not the circuit's: at least one row must be
inline int check_k_blinding(const char* what, uint32_t k, uint32_t bf) {
    if (int rc = check_k(what, k)) return rc;
    if ((uint64_t)bf + 1 >= (1ull << k)) {
        set_error("%s: blinding_factors + 1 >= 2^k", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

// The layout of one workspace buffer.  Regions are taken in call order, each rounded up to 256 bytes, and `total` is what
// DevBuf::ensure is asked for.  A Carve owns nothing and points nowhere: it adds up offsets, so that a region's offset is written
// once and the buffer's size, the host image and the device pointers all come from it.  A layout that repeats (one argument's
// regions, the descriptor blob) is a Carve of its own whose total the outer one takes.
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t off = total;
        total += align256(bytes);
        return off;
    }
    size_t take_packed(size_t bytes) {  // not rounded: elements of a stride the kernels fix (columns of 2^k, one layout per argument)
        const size_t off = total;
        total += bytes;
        return off;
    }
};
// The descriptor blob of a call: filled in on the host (h), staged to the device in one copy (d).  A region's two pointers come
// from one offset, so what the host writes and what the kernels read cannot drift apart.
template <class T>
struct Mirror {
    T* h;
    T* d;
};
struct Blob {
    char* h;
    char* d;
    template <class T>
    Mirror<T> at(size_t off) const {
        return {(T*)(h + off), (T*)(d + off)};
    }
};
// api.hip: the device copy of a pinned host column whose fingerprint still matches the caller's memory, or nullptr
const Fe* pinned_column_lookup(Ctx* c, const uint64_t* h_col, size_t elems);

// The staging of a host-pointer form: the caller's columns cross PCIe through slots of Ctx::host_io, on the call's stream.  Plan
// first, without a HIP call: in / out / room take slots in call order through a Carve (packed, or each rounded to 256 bytes with
// `aligned`), and a column pinned with h2hip_columns_pin is read where it lies and takes none.  upload() then sizes the buffer
// once, fills in the device pointers and queues the uploads in the order they were registered; the device driver runs; finish()
// queues the downloads and waits for the stream.  A further round over the same slots registers its copies with in_at / out_at.
// The drain rule: once a copy from or into the caller's memory may be queued, no exit leaves it queued -- the destructor waits for
// the stream on every return that finish() did not complete, so a caller may free its columns after an error as after a success.
// host_io is not one of the shared workspaces the WsGuard orders: only the host forms touch it, always on the engine's own stream;
// each holds the context's lock until it returns and has waited for that stream by then, and none calls another, so two forms
// never hold the buffer at once and its uploads are queued ahead of the guard without a second user to order against.
// Everything the _device forms share with other calls is under the guard.
struct HostIo {
    struct Copy {
        void* h;
        size_t off, bytes;
    };
    Ctx* c;
    DevBuf& buf;
    hipStream_t s;
    bool aligned;
    Carve carve;
    std::vector<std::pair<void*, size_t>> ptrs;  // where a slot's device pointer goes (an object pointer of any type), and the slot's offset
    std::vector<Copy> ins, outs;
    bool queued = false;
    HostIo(Ctx* c_, DevBuf& buf_, hipStream_t s_, bool aligned_ = false) : c(c_), buf(buf_), s(s_), aligned(aligned_) {}
    HostIo(const HostIo&) = delete;
    ~HostIo() {
        if (queued) (void)hipStreamSynchronize(s);
    }
    template <class T>
    size_t room(size_t bytes, T** d) {  // a region only the device touches; the slot's offset, for in_at / out_at
        const size_t off = aligned ? carve.take(bytes) : carve.take_packed(bytes);
        ptrs.push_back({(void*)d, off});
        return off;
    }
    void in_at(const void* h, size_t bytes, size_t off) { ins.push_back({(void*)h, off, bytes}); }
    void out_at(void* h, size_t bytes, size_t off) { outs.push_back({h, off, bytes}); }
    template <class T>
    void in(const void* h, size_t bytes, T** d, bool try_pinned = false) {
        if (try_pinned && (*d = (T*)pinned_column_lookup(c, (const uint64_t*)h, bytes / sizeof(Fe)))) return;
        in_at(h, bytes, room(bytes, d));
    }
    template <class T>
    size_t out(void* h, size_t bytes, T** d) {
        const size_t off = room(bytes, d);
        out_at(h, bytes, off);
        return off;
    }
    int upload() {
        if (int rc = buf.ensure(carve.total)) return rc;
        for (const auto& pd : ptrs) {
            void* p = (char*)buf.p + pd.second;
            memcpy(pd.first, &p, sizeof p);
        }
        for (const Copy& j : ins) {
            if (!j.bytes) continue;
            queued = true;
            H2_CHECK(hipMemcpyAsync((char*)buf.p + j.off, j.h, j.bytes, hipMemcpyHostToDevice, s));
        }
        ins.clear();
        return 0;
    }
    int finish() {
        for (const Copy& j : outs) {
            if (!j.bytes) continue;
            queued = true;
            H2_CHECK(hipMemcpyAsync(j.h, (char*)buf.p + j.off, j.bytes, hipMemcpyDeviceToHost, s));
        }
        outs.clear();
        H2_CHECK(hipStreamSynchronize(s));
        queued = false;
        return 0;
    }
};

Ctx* ctx();             // the primary device's context (device_ids[0] of h2hip_init)
int n_devices();        // devices the engine was initialised with (>= 1 once ready)
Ctx* ctx_at(int i);     // context of the i-th device of h2hip_init's list
int ensure_init();      // lazily h2hip_init(NULL, 0), or the HALO2_HIP_DEVICES list

// ntt.hip
struct NttScale {
    // optional fused pointwise steps (poly/domain.rs:246-247, :294, :355-360)
    bool in_scale = false;    // a[i] *= in3[i % 3] on the first-pass load
    Fe in3[3];
    uint64_t in_len = 0;      // elements at index >= in_len are read as zero (resize(.., zero), domain.rs:247)
    bool out_scale = false;   // a[i] *= out3[i % 3] on the final-pass store
    Fe out3[3];
    // the inverse transform's 1 / n
    static NttScale inverse(const Fe& divisor) {
        NttScale sc;
        sc.out_scale = true;
        sc.out3[0] = sc.out3[1] = sc.out3[2] = divisor;
        return sc;
    }
    // distribute_powers_zeta (poly/domain.rs:335-351): a[i] *= [1, g_coset, g_coset_inv][i % 3] into the coset, zero-padded from in_len
    // elements when that is set (:240-254) ...
    static NttScale into_coset(const Fe& g_coset, const Fe& g_coset_inv, uint64_t in_len = 0) {
        NttScale sc;
        sc.in_scale = true;
        sc.in3[0] = fe_one<FrP>();
        sc.in3[1] = g_coset;
        sc.in3[2] = g_coset_inv;
        sc.in_len = in_len;
        return sc;
    }
    // ... and the two constants swapped on the way out, times the inverse transform's divisor
    static NttScale out_of_coset(const Fe& divisor, const Fe& g_coset, const Fe& g_coset_inv) {
        NttScale sc;
        sc.out_scale = true;
        sc.out3[0] = divisor;
        sc.out3[1] = fe_mul<FrP>(divisor, g_coset_inv);
        sc.out3[2] = fe_mul<FrP>(divisor, g_coset);
        return sc;
    }
};
// d_src (optional): the first pass reads its input there instead of d_data (which is then output only); with
// sc->in_len set only d_src[0 .. in_len) is read
void ntt_twiddles_free(Ctx* c);
int ntt_device(Ctx* c, Fe* d_data, const Fe& omega, uint32_t log_n, const NttScale* sc, hipStream_t s, const Fe* d_src = nullptr);

// the part mode of the first-pass load (ntt.hip, NttPart), as ntt_run takes it: the extended domain whose power table the load reads
// and the part of each transform of the launch (host array)
struct NttPartMode {
    Fe ext_omega;
    uint32_t ext_k;
    const uint32_t* parts;
};
int ntt_part_device_batch(Ctx* c, Fe* const* h_outs, const Fe* const* h_srcs, const uint32_t* parts, size_t count, uint32_t k, uint32_t ext_k,
                          const Fe& ext_omega, const Fe& g_coset, const Fe& g_coset_inv, hipStream_t s);
int ntt_power_table(Ctx* c, const Fe& omega, uint32_t log_n, hipStream_t s, const Fu** lo, const Fu** hi, uint32_t* lo_bits);
int ntt_device_batch(Ctx* c, Fe* const* h_datas, const Fe* const* h_srcs, size_t count, const Fe& omega, uint32_t log_n, const NttScale* sc,
                     hipStream_t s);

int scale_periodic_device(Ctx* c, Fe* d_a, uint64_t n, const uint64_t* h_t, uint32_t t_len, hipStream_t s);

// ecfft.hip
int g_to_lagrange_device(Ctx* c, const Affine* d_g, uint32_t k, Affine* d_out, hipStream_t s);
int ec_normalize_device(const XYZZ* d_in, Affine* d_out, uint64_t n, hipStream_t s);  // batched XYZZ -> affine
int fft_g1_device(Ctx* c, Jac* d_a, const Fe& omega, uint32_t log_n, hipStream_t s);   // best_fft::<G1>, in place on Jacobian points

// gen.hip
int gen_scalars_device(uint64_t seed, uint64_t start, size_t n, Fe* d_out, hipStream_t s);
int gen_points_device(uint64_t seed, uint64_t start, size_t n, Affine* d_out, hipStream_t s);

// product.hip: the permutation / lookup grand products and ff's BatchInvert, enqueued on s (no synchronisation).  cols / perms are
// host arrays of device pointers; for lookups inputs_tables[2j], [2j + 1] = A_j, S_j and permuted[2j], [2j + 1] = A'_j, S'_j
int permutation_products_device(Ctx* c, uint32_t k, const Fe& omega, const Fe& delta, const Fe& beta, const Fe& gamma,
                                const Fe* const* cols, const Fe* const* perms, uint32_t n_columns, uint32_t chunk_len,
                                const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s);
int lookup_products_device(Ctx* c, uint32_t k, const Fe& beta, const Fe& gamma, const Fe* const* inputs_tables,
                           const Fe* const* permuted, size_t count, const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s);
int batch_invert_device(Ctx* c, Fe* d_a, uint64_t n, hipStream_t s);
// the shuffle argument's grand products: inputs[j] = A_j, shuffles[j] = S_j
int shuffle_products_device(Ctx* c, uint32_t k, const Fe& gamma, const Fe* const* inputs, const Fe* const* shuffles, size_t count,
                            const uint64_t* blinding, uint32_t bf, Fe* const* z, hipStream_t s);
// the logUp (mv-lookup) argument's grand sums: inputs flat and argument-major (n_inputs[j] columns of argument j), tables[j], m[j] -> phi[j]
int mvlookup_sums_device(Ctx* c, uint32_t k, const Fe& beta, const Fe* const* inputs, const uint32_t* n_inputs, const Fe* const* tables,
                         const Fe* const* m, size_t count, const uint64_t* blinding, uint32_t bf, Fe* const* phi, hipStream_t s);
// lookup.hip: the mv-lookup multiplicity columns m[j]; waits for s once, H2HIP_ELOOKUP (every m still written) when an input value is missing
int mvlookup_multiplicities_device(Ctx* c, uint32_t k, const Fe* const* in, const uint32_t* n_inputs, const Fe* const* tab, size_t count,
                                   uint32_t bf, Fe* const* m, hipStream_t s);
// lookup.hip: commit_permuted's A' / S' of `count` lookups from device columns; waits for s once, H2HIP_ELOOKUP when an input value is
// missing from its table
int lookup_permute_device(Ctx* c, uint32_t k, const Fe* const* in, const Fe* const* tab, size_t count, const uint64_t* blinding, uint32_t bf,
                          Fe* const* pa, Fe* const* pt, hipStream_t s);
// lookup.hip: its sort alone, enqueued on s: d_src[q] -> canonical keys sorted ascending, rows u .. 2^k - 1 as all-ones keys at the end;
// the three device tables hold `cols` device pointers, and the keys end in d_k1[q] when lookup_sort_passes(k) is odd, else in d_k0[q]
uint32_t lookup_sort_passes(uint32_t k);
int lookup_sort_enqueue(const Fe* const* d_src, Fe* const* d_k0, Fe* const* d_k1, uint32_t cols, uint32_t k, uint64_t u, hipStream_t s);
// setup.hip
int kzg_setup_device(Ctx* c, uint32_t k, const Fe& s, Affine* d_g, Affine* d_gl, hipStream_t stream);

// api.hip: the fingerprint of a host column (H2_COL_SAMPLES elements); PinCache::make_room with the configured budget
// (HALO2_HIP_COLUMN_CACHE_GB); the bodies of the two kinds' unpin and pinned_info entry points -- unpin never starts a stopped engine
void column_sample(const uint64_t* h_col, size_t elems, uint8_t* out);
int pinned_make_room(Ctx* c, size_t bytes, bool* fits);
int pinned_unpin(PinCache::Kind kind, const void* const* keys, size_t count, const char* name);
int pinned_info(PinCache::Kind kind, size_t* n, size_t* device_bytes, const char* name);

// evalh.hip
void evalh_modules_free(Ctx* c);                            // unload this device's generated kernels (release_ctx)
void evalh_rtc_shutdown();                                  // join the compile threads (h2hip_shutdown)
int evaluate_h_validate(const h2hip_evalh_desc* d, const void* values);
int evaluate_h_host(Ctx* c, const h2hip_evalh_desc* d, const h2hip_evalh_mvlookups* mv, const h2hip_evalh_shuffles* sh, uint64_t* values,
                    bool dev, hipStream_t s);
// lookup compression (commit_permuted's compressed expressions) on the interpreter: validation needs no device; the run is enqueued on s
int lookup_compress_validate(uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges, const h2hip_graph* graphs,
                             size_t n_graphs);
int lookup_compress_device(Ctx* c, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice, uint32_t n_advice,
                           const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                           const uint64_t theta[4], const h2hip_graph* graphs, size_t n_graphs, Fe* const* out, hipStream_t s);
// the witness check's gate loop on the interpreter (check.hip drives it): bit (row % 64) of d_mask[g * words + row / 64] is set where
// gate polynomial g is non-zero at Lagrange row `row`; the caller holds the workspaces, this only enqueues on s
int check_gates_validate(uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges, const h2hip_graph* graphs,
                         size_t n_graphs);
int check_gates_enqueue(Ctx* c, uint32_t k, const Fe* const* fixed, uint32_t n_fixed, const Fe* const* advice, uint32_t n_advice,
                        const Fe* const* instance, uint32_t n_instance, const uint64_t* challenges, uint32_t n_challenges,
                        const h2hip_graph* graphs, size_t n_graphs, uint64_t* d_mask, uint32_t words, hipStream_t s);

// msm.hip
// tab != nullptr: fixed-base form over tab's window table (d_bases unused)
int msm_device(Ctx* c, const Fe* d_scalars, const Affine* d_bases, size_t n, XYZZ* h_out, hipStream_t s, const MsmTable* tab = nullptr);
int msm_batch_device(Ctx* c, const Fe* const* scalars, bool scalars_on_host, const Affine* d_bases, size_t n, size_t count, XYZZ* h_out,
                     hipStream_t s, const MsmTable* tab = nullptr, const Affine* h_bases = nullptr);
// the two MSMs of an IPA round over p (2 half scalars) and g (2 half points) -> h_out[0] = L, h_out[1] = R; waits for s once
int msm_pair_device(Ctx* c, const Fe* d_p, const Affine* d_g, size_t half, XYZZ h_out[2], hipStream_t s);
size_t msm_pair_fused_max_half(size_t limit);  // the largest half <= limit that runs as one two-set run under the tuning in force (0: none)
uint32_t msm_table_window(size_t n);  // window width a table for n pinned points is built with
int msm_table_build(Ctx* c, const Affine* d_points, size_t n, uint32_t cw, Affine* d_table, hipStream_t s);

}  // namespace h2
