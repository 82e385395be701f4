// api.hip -- the engine of libhalo2hip.so: the device contexts, their locks, worker and copier threads, workspace buffers and
// HIP-event stage timers, and the entry points whose host logic is the engine's own.
//
// The rule: a stage file owns the extern "C" entry points and the h2hip_debug_* hooks of its stage (msm.hip, ntt.hip, evalh.hip,
// ecfft.hip, setup.hip, gen.hip, product.hip, opening.hip, lookup.hip, keygen.hip, check.hip, serde.hip).  This file keeps init /
// shutdown / errors / profile, the device memory helpers, the MSM's host and device forms (sharding, fold, RCCL gather), the pins
// (bases, lazy, columns), the NTT / domain family (batch_over_devices, the host pipeline), h2hip_g1_fold / _batch_normalize /
// _to_affine, the one Tuning instance with its guards (engine.h), and the hooks of its own settings (h2hip_debug_set_ntt_host_batch, _set_lazy_pin, _set_table_records,
// _rccl_gather_selftest).  That is also all that runs in the stub build: this file compiled alone, as plain C++ against
// tests/cpp/hipstub, and linked with tests/cpp/engine_stubs.cpp, which stands in for what this file calls in the stage files.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <shared_mutex>
#include <thread>

#include "../../include/halo2hip.h"
#include "../../include/halo2hip_debug.h"
#include "../../include/halo2hip_g1.h"
#include "engine.h"
#include "g1_host.h"

// the optional lazy pin cache (further down, inside the extern "C" block: declared with that linkage here too, g++ insists)
extern "C" {
static void lazy_forget(const void* key);
static void lazy_reset();
static void lazy_pin_consider(const uint64_t* bases_xy, size_t n);
}

namespace h2 {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) {
        H2_CHECK(hipDeviceSynchronize());  // a previous call's kernels may still read the old block
        H2_CHECK(hipFree(p));
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes + bytes / 8 + 4096;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return H2HIP_ENOMEM;
    }
    cap = want;
    return 0;
}

int HostBuf::ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) {
        H2_CHECK(hipDeviceSynchronize());
        H2_CHECK(hipHostFree(p));
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes * 2 + 4096;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        p = nullptr;
        set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return H2HIP_ENOMEM;
    }
    cap = want;
    return 0;
}

void HostBuf::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

// ---- devices -----------------------------------------------------------------------------------------------------
// One Ctx per device of h2hip_init's list.  g_ctx is the primary (device_ids[0]); its mutex serialises the entry
// points.  The other devices only ever run MSM shards (best_multiexp splits its pairs the same way over rayon
// threads, arithmetic.rs:137-153), each from its own worker thread.
// Locking (round 3; one process-wide mutex before): g_engine_mu is held shared by every entry point and exclusively by
// h2hip_init / h2hip_shutdown and the setter hooks (TuneWrite), so neither the device list nor a setting can change under a
// running call.  Each device context has its own
// mutex: a `_device` entry point locks only the context that owns its pointers, so calls on different GPUs -- and concurrent
// best_fft callers spread over devices (plonk/permutation/keygen.rs:216-233) -- overlap.  Entry points that touch every
// device (host-pointer MSMs over several GPUs, pin / unpin, pinned_info) lock all contexts in list order; the lazy-pin
// bookkeeping and the configuration are only touched under the first context's mutex.
static std::shared_mutex g_engine_mu;
static Ctx g_ctx;
static std::vector<Ctx*> g_devs;  // g_devs[0] == &g_ctx once ready
Ctx* ctx() { return &g_ctx; }
int n_devices() { return (int)g_devs.size(); }
Ctx* ctx_at(int i) { return g_devs[(size_t)i]; }

int Ctx::stage_h2d(void* d_dst, const void* h_src, size_t bytes, hipStream_t s) {
    const size_t ring = (size_t)4 << 20;
    if (bytes > ring / 2) {  // too large for the ring: a synchronous copy
        H2_CHECK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, s));
        H2_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    if (!stage.p) {
        int rc = stage.ensure(ring);
        if (rc) return rc;
        stage_off = 0;
    }
    const size_t need = align256(bytes);
    if (stage_off + need > ring) {  // wrap: copies queued from the old contents must have left the ring
        H2_CHECK(hipDeviceSynchronize());
        stage_off = 0;
    }
    char* h = (char*)stage.p + stage_off;
    memcpy(h, h_src, bytes);
    stage_off += need;
    H2_CHECK(hipMemcpyAsync(d_dst, h, bytes, hipMemcpyHostToDevice, s));
    return 0;
}

int Ctx::timer_begin(const char* name, hipStream_t s) {
    if (!profiling) return -1;
    StageTimer t;
    t.name = name;
    if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) return -1;
    (void)hipEventRecord(t.e0, s);
    t.pending = true;
    timers.push_back(t);
    return (int)timers.size() - 1;
}

int Ctx::timer_kernel(const char* name, hipEvent_t* e0, hipEvent_t* e1) {
    if (!profiling_kernel || profiling) return -1;
    StageTimer t;
    t.name = name;
    if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) return -1;
    t.pending = true;
    timers.push_back(t);
    *e0 = t.e0;
    *e1 = t.e1;
    return (int)timers.size() - 1;
}

void Ctx::timer_end(int id, hipStream_t s) {
    if (id < 0 || id >= (int)timers.size()) return;
    (void)hipEventRecord(timers[id].e1, s);
}

// fold finished event pairs into per-name totals (kept in entries with e0 == nullptr)
void Ctx::timers_collect() {
    std::vector<StageTimer> totals;
    for (auto& t : timers) {
        double ms = t.total_ms;
        uint64_t cnt = t.count;
        if (t.pending) {
            float f = 0.f;
            (void)hipEventSynchronize(t.e1);
            if (hipEventElapsedTime(&f, t.e0, t.e1) == hipSuccess) {
                ms = f;
                cnt = 1;
            }
            (void)hipEventDestroy(t.e0);
            (void)hipEventDestroy(t.e1);
        }
        bool found = false;
        for (auto& u : totals)
            if (u.name == t.name) {
                u.total_ms += ms;
                u.count += cnt;
                found = true;
            }
        if (!found) {
            StageTimer u;
            u.name = t.name;
            u.total_ms = ms;
            u.count = cnt;
            totals.push_back(u);
        }
    }
    timers.swap(totals);
}

int Ctx::ws_acquire(hipStream_t s) {
    if (ws_used && ws_last_stream != s) H2_CHECK(hipStreamWaitEvent(s, ws_event, 0));
    return 0;
}

int Ctx::ws_release(hipStream_t s) {
    if (!ws_event) H2_CHECK(hipEventCreateWithFlags(&ws_event, hipEventDisableTiming));
    H2_CHECK(hipEventRecord(ws_event, s));
    ws_last_stream = s;
    ws_used = true;
    return 0;
}

// aux1 (stage A), aux2 (stage C) and aux_b (stage B) see every CU: a slice of the CUs reserved for the sort and reduce streams was
// slower for every split tried ("Tried ..., measured, not kept").  They are still created through the CU-mask call, with
// a full mask: as plain hipStreamCreate streams the pipelined batch of eight 2^20-pair MSMs measured 1.26 against 1.16 ms per MSM
// (profiles/tuning_struct/ab.md, first session).
int Ctx::ensure_aux(size_t n_events) {
    const std::vector<uint32_t> every_cu((size_t)(sm_count + 31) / 32, 0xffffffffu);
    for (hipStream_t* s : {&aux1, &aux2, &aux_b})
        if (!*s) H2_CHECK(hipExtStreamCreateWithCUMask(s, (uint32_t)every_cu.size(), every_cu.data()));
    while (aux_events.size() < n_events) {
        hipEvent_t e;
        H2_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        aux_events.push_back(e);
    }
    return 0;
}

// ---- configuration (environment, read once at init) -----------------------------------------------------
struct Config {
    size_t multi_gpu_min_n = (size_t)1 << 18;  // HALO2_HIP_MULTI_GPU_MIN_N: smaller MSMs stay on the primary device
    size_t msm_min_n = (size_t)1 << 10;        // HALO2_HIP_MSM_MIN_N: below this the Rust shim keeps the CPU body
    uint32_t ntt_min_log_n = 10;               // HALO2_HIP_NTT_MIN_LOGN: likewise for best_fft
    bool gather_rccl = false;                  // HALO2_HIP_GATHER=rccl: the devices' set sums meet through ncclAllGather (default: host fold)
    bool fixed_base = true;                    // HALO2_HIP_FIXED_BASE=0: h2hip_bases_pin keeps the points only
    size_t table_max_bytes = (size_t)160 << 30;  // HALO2_HIP_TABLE_MAX_GB: largest window table built at pin time
    bool allow_dup = false;                    // HALO2_HIP_ALLOW_DUPLICATE_DEVICES=1: rehearsal on a one-GPU box
    bool roctx = false;                        // HALO2_HIP_ROCTX=1: roctx range around every entry point
    size_t column_cache_bytes = (size_t)64 << 30;  // HALO2_HIP_COLUMN_CACHE_GB: HBM the pinned proving-key columns may take (least recently used dropped first)
};
static Config g_cfg;

// ---- tuning (engine.h): the one instance, its reader and the two guards -------------------------------------------------------------
static Tuning g_tuning;
const Tuning& tune() { return g_tuning; }
TuneWrite::TuneWrite() : engine(g_engine_mu) {}
Tuning* TuneWrite::operator->() const { return &g_tuning; }
TuneRead::TuneRead() : engine(g_engine_mu) {}

static bool env_u64(const char* name, uint64_t* out) {
    const char* v = getenv(name);
    if (!v || !*v) return false;
    char* end = nullptr;
    unsigned long long x = strtoull(v, &end, 0);
    if (end == v) return false;
    *out = x;
    return true;
}

// under do_init's exclusive hold of the engine lock: the members are written directly (a TuneWrite here would wait for itself)
static void read_config() {
    Config c;
    Tuning& t = g_tuning;
    uint64_t v;
    if (env_u64("HALO2_HIP_MULTI_GPU_MIN_N", &v)) c.multi_gpu_min_n = (size_t)v;
    if (env_u64("HALO2_HIP_MSM_MIN_N", &v)) c.msm_min_n = (size_t)v;
    if (env_u64("HALO2_HIP_NTT_MIN_LOGN", &v)) c.ntt_min_log_n = (uint32_t)v;
    if (env_u64("HALO2_HIP_FIXED_BASE", &v)) c.fixed_base = v != 0;
    if (env_u64("HALO2_HIP_TABLE_MAX_GB", &v)) c.table_max_bytes = (size_t)v << 30;
    if (env_u64("HALO2_HIP_ALLOW_DUPLICATE_DEVICES", &v)) c.allow_dup = v != 0;
    if (env_u64("HALO2_HIP_ROCTX", &v)) c.roctx = v != 0;
    if (env_u64("HALO2_HIP_LAZY_PIN", &v)) t.lazy_pin_after = (uint32_t)v;
    if (env_u64("HALO2_HIP_COLUMN_CACHE_GB", &v)) c.column_cache_bytes = (size_t)v << 30;
    if (env_u64("HALO2_HIP_NTT_TWIDDLE_MB", &v)) t.ntt_full_budget = v << 20;
    if (env_u64("HALO2_HIP_EVALH_CODEGEN", &v)) evalh_codegen_apply(&t, (int)v, 0);  // as h2hip_debug_set_evalh_codegen(v, 0)
    if (env_u64("HALO2_HIP_MSM_WINDOW", &v) && v >= 2 && v <= 24) t.msm_window = (uint32_t)v;
    {  // HALO2_HIP_STREAM=0: host-slice MSMs upload whole arrays ahead of the run (no copier thread); HALO2_HIP_STREAM_MIN_N: threshold
        uint64_t on = 1, min_n = 0;
        const bool has_on = env_u64("HALO2_HIP_STREAM", &on), has_min = env_u64("HALO2_HIP_STREAM_MIN_N", &min_n);
        if (has_on || has_min) {  // as h2hip_debug_set_msm_stream(HALO2_HIP_STREAM=0 ? 1 : 0, 0, min_n)
            t.msm_stream_chunks = has_on && on == 0 ? 1 : 0;
            t.msm_stream_ratio = Tuning{}.msm_stream_ratio;
            t.msm_stream_min_n = has_min && min_n ? (size_t)min_n : Tuning{}.msm_stream_min_n;
        }
    }
    const char* g = getenv("HALO2_HIP_GATHER");
    if (g && !strcmp(g, "rccl")) c.gather_rccl = true;
    g_cfg = c;
}

// ---- roctx ranges (optional; the library is dlopen'ed so that nothing links against the tracer) ------------------------
static int (*g_roctx_push)(const char*) = nullptr;
static int (*g_roctx_pop)() = nullptr;
static void roctx_load() {
    if (g_roctx_push) return;
    void* h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    g_roctx_push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    g_roctx_pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!g_roctx_push || !g_roctx_pop) g_roctx_push = nullptr, g_roctx_pop = nullptr;
}

// ---- RCCL (dlopen'ed: a single-GPU consumer never needs it) ---------------------------------------------------------------
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::vector<ncclComm_t> comms;  // one per device of the engine, empty when the host gathers
};
static Rccl g_rccl;

static bool rccl_load() {
    Rccl& r = g_rccl;
    if (r.lib) return true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);  // the copy torch loaded, if any (same SONAME)
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    r.CommInitAll = (decltype(r.CommInitAll))dlsym(h, "ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllGather || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) return false;
    r.lib = h;
    return true;
}

// one communicator per engine device (ncclCommInitAll); needs distinct devices.  0 on success.
static int rccl_comms_create() {
    if (!g_rccl.comms.empty()) return 0;
    std::vector<int> ids;
    for (Ctx* x : g_devs) ids.push_back(x->device);
    for (size_t i = 0; i < ids.size(); i++)
        for (size_t j = 0; j < i; j++)
            if (ids[i] == ids[j]) {
                set_error("RCCL needs distinct devices (device %d is listed twice); partials are gathered on the host", ids[i]);
                return H2HIP_EINVAL;
            }
    if (!rccl_load()) {
        set_error("librccl.so.1 not found; partials are gathered on the host");
        return H2HIP_EDEVICE;
    }
    g_rccl.comms.assign(ids.size(), nullptr);
    ncclResult_t r = g_rccl.CommInitAll(g_rccl.comms.data(), (int)ids.size(), ids.data());
    (void)hipSetDevice(ids[0]);
    if (r != ncclSuccess) {
        set_error("ncclCommInitAll failed (%s); partials are gathered on the host", g_rccl.GetErrorString(r));
        g_rccl.comms.clear();
        return H2HIP_EDEVICE;
    }
    return 0;
}

// ---- worker threads: one per secondary device, alive from init to shutdown -------------------------------------------------
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> task;
    bool has_task = false, done = false, quit = false;
    int rc = 0;
    std::string err;
};
static std::vector<Worker*> g_workers;  // g_workers[i] serves g_devs[i]; [0] is unused (the caller's thread runs device 0)

static void worker_main(Worker* w, int device) {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(w->m);
    for (;;) {
        w->cv.wait(lk, [&] { return w->has_task || w->quit; });
        if (w->quit) return;
        std::function<int()> t = std::move(w->task);
        w->has_task = false;
        lk.unlock();
        g_err[0] = 0;
        int rc = t();
        lk.lock();
        w->rc = rc;
        w->err = g_err;
        w->done = true;
        w->cv.notify_all();
    }
}

static void worker_post(int i, std::function<int()> f) {
    Worker* w = g_workers[(size_t)i];
    std::lock_guard<std::mutex> lk(w->m);
    w->task = std::move(f);
    w->has_task = true;
    w->done = false;
    w->cv.notify_all();
}

static int worker_wait(int i) {
    Worker* w = g_workers[(size_t)i];
    std::unique_lock<std::mutex> lk(w->m);
    w->cv.wait(lk, [&] { return w->done; });
    if (w->rc) set_error("device %d: %s", g_devs[(size_t)i]->device, w->err.c_str());
    return w->rc;
}

// Run f(i) for every engine device i < n_use: device 0 on the calling thread, the others on their workers.
static int on_devices(int n_use, const std::function<int(int)>& f) {
    for (int i = 1; i < n_use; i++) worker_post(i, [&f, i] { return f(i); });
    int rc = 0;
    if (hipSetDevice(g_devs[0]->device) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", g_devs[0]->device);
        rc = H2HIP_EDEVICE;
    } else {
        rc = f(0);
    }
    char first_err[sizeof(g_err)];
    memcpy(first_err, g_err, sizeof(g_err));
    for (int i = 1; i < n_use; i++) {
        int r = worker_wait(i);
        if (r && !rc) {
            rc = r;
            memcpy(first_err, g_err, sizeof(g_err));
        }
    }
    if (rc) memcpy(g_err, first_err, sizeof(g_err));
    return rc;
}

// ---- copier threads (engine.h) ----------------------------------------------------------------------------------------------
struct Copier {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;       // work for the thread
    std::condition_variable done_cv;  // progress for a blocked copier_wait
    std::deque<CopyJob> q;
    hipStream_t stream = nullptr;
    int device = 0;
    bool quit = false;
    size_t popped = 0;  // jobs taken off the queue this session (under m)
    std::atomic<size_t> done{0};
    std::atomic<int> err{0};
    std::atomic<int> waiters{0};
};

static void copier_main(Copier* cp) {
    (void)hipSetDevice(cp->device);
    std::unique_lock<std::mutex> lk(cp->m);
    for (;;) {
        cp->cv.wait(lk, [&] { return !cp->q.empty() || cp->quit; });
        if (cp->quit) return;
        const CopyJob j = cp->q.front();
        cp->q.pop_front();
        cp->popped++;
        hipStream_t st = cp->stream;
        lk.unlock();
        if (!cp->err.load(std::memory_order_relaxed)) {
            hipError_t e = j.gate ? hipStreamWaitEvent(st, j.gate, 0) : hipSuccess;
            if (e == hipSuccess) e = hipMemcpyAsync(j.dst, j.src, j.bytes, j.d2h ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, st);
            if (e == hipSuccess && j.ev) e = hipEventRecord(j.ev, st);
            if (e != hipSuccess) cp->err.store((int)e);
        }
        cp->done.fetch_add(1);
        lk.lock();
        if (cp->waiters.load()) cp->done_cv.notify_all();
    }
}

bool copier_ready(Ctx* c, bool down) {
    Copier*& cp = c->copier[down ? 1 : 0];
    if (cp) return true;
    try {
        cp = new Copier();
        cp->device = c->device;
        cp->th = std::thread(copier_main, cp);
    } catch (...) {  // no memory / no thread: nothing may unwind across the C ABI; the caller takes its unstreamed path
        if (cp) delete cp;
        cp = nullptr;
        set_error("copier thread for device %d could not be started", c->device);
        return false;
    }
    return true;
}

int copier_begin(Ctx* c, bool down, hipStream_t stream) {
    if (!copier_ready(c, down)) return H2HIP_ENOMEM;
    Copier* cp = c->copier[down ? 1 : 0];
    std::lock_guard<std::mutex> lk(cp->m);
    if (!cp->q.empty()) {  // a session is over only when its jobs are (copier_abort on every error path)
        set_error("copier: previous session still has jobs queued");
        return H2HIP_EDEVICE;
    }
    cp->stream = stream;
    cp->popped = 0;
    cp->done.store(0);
    cp->err.store(0);
    return 0;
}

int copier_push(Ctx* c, bool down, std::vector<CopyJob>& jobs) {
    Copier* cp = c->copier[down ? 1 : 0];
    try {
        std::lock_guard<std::mutex> lk(cp->m);
        for (const CopyJob& j : jobs) cp->q.push_back(j);
        cp->cv.notify_all();
    } catch (...) {
        set_error("copier: out of memory");
        return H2HIP_ENOMEM;
    }
    jobs.clear();
    return 0;
}

static void copier_block_until(Copier* cp, size_t n_jobs) {
    // a job is tens to hundreds of microseconds away: spin briefly (the enqueueing thread wants to react within a launch latency),
    // then sleep on the condition variable instead of holding a host core through a 10-ms upload
    for (uint32_t spins = 0; spins < 4000; spins++)
        if (cp->done.load(std::memory_order_acquire) >= n_jobs) return;
    cp->waiters.fetch_add(1);
    {
        std::unique_lock<std::mutex> lk(cp->m);
        cp->done_cv.wait(lk, [&] { return cp->done.load() >= n_jobs; });
    }
    cp->waiters.fetch_sub(1);
}

int copier_wait(Ctx* c, bool down, size_t n_jobs) {
    Copier* cp = c->copier[down ? 1 : 0];
    copier_block_until(cp, n_jobs);
    if (int e = cp->err.load()) {
        set_error("%s copy of a streamed piece failed: %s", down ? "device-to-host" : "host-to-device", hipGetErrorString((hipError_t)e));
        return H2HIP_EDEVICE;
    }
    return 0;
}

void copier_abort(Ctx* c, bool down, size_t n_jobs) {
    Copier* cp = c->copier[down ? 1 : 0];
    if (!cp || cp->done.load(std::memory_order_acquire) >= n_jobs) return;
    {
        std::lock_guard<std::mutex> lk(cp->m);
        if (cp->q.empty() && cp->done.load() == cp->popped) return;  // idle already
    }
    if (!cp->err.load()) cp->err.store((int)hipErrorUnknown);  // the jobs not yet started are skipped (and still counted)
    for (;;) {  // idle = nothing queued and every popped job counted: the thread no longer touches the caller's memory or events
        {
            std::lock_guard<std::mutex> lk(cp->m);
            if (cp->q.empty() && cp->done.load() == cp->popped) return;
        }
        std::this_thread::yield();
    }
}

void copier_stop(Ctx* c) {
    for (int k = 0; k < 2; k++) {
        Copier* cp = c->copier[k];
        if (!cp) continue;
        {
            std::lock_guard<std::mutex> lk(cp->m);
            cp->quit = true;
            cp->cv.notify_all();
        }
        cp->th.join();
        delete cp;
        c->copier[k] = nullptr;
    }
}

static bool unpin_everywhere(const void* key);
static bool pinned_validate(const uint64_t* bases_xy, size_t n);

static int init_one(Ctx* c, int dev) {
    H2_CHECK(hipSetDevice(dev));
    hipDeviceProp_t prop;
    H2_CHECK(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library carries gfx950 code objects only", dev, prop.gcnArchName);
        return H2HIP_EDEVICE;
    }
    c->device = dev;
    c->sm_count = prop.multiProcessorCount;
    H2_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->ready = true;
    return 0;
}

static void release_ctx(Ctx* c);

static std::atomic<int> g_init_failed{0};  // an attempt found no usable GPU; lazy initialisation does not try again (ensure_init)

static int do_init(const int* device_ids, int n_ids) {
    Ctx* c = ctx();
    std::unique_lock<std::shared_mutex> lk(g_engine_mu);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_error("no usable HIP device (%s); libhalo2hip has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        g_init_failed.store(1, std::memory_order_release);
        return H2HIP_EDEVICE;
    }
    g_init_failed.store(0, std::memory_order_release);
    if (!c->ready) read_config();  // a running engine keeps the configuration it started with: entry points read it under the shared lock
    // the device list: the caller's, else HALO2_HIP_DEVICES ("0,1,2,3"), else the calling thread's current device
    std::vector<int> ids;
    if (device_ids && n_ids > 0) {
        ids.assign(device_ids, device_ids + n_ids);
    } else if (const char* v = getenv("HALO2_HIP_DEVICES")) {
        for (const char* q = v; *q;) {
            char* end = nullptr;
            long d = strtol(q, &end, 10);
            if (end == q) break;
            ids.push_back((int)d);
            q = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') break;
        }
    }
    if (ids.empty()) {
        int dev = 0;
        H2_CHECK(hipGetDevice(&dev));
        ids.push_back(dev);
    }
    if (c->ready) {  // idempotent for the same list; a different one needs h2hip_shutdown first
        bool same = ids.size() == g_devs.size();
        for (size_t i = 0; same && i < ids.size(); i++) same = g_devs[i]->device == ids[i];
        if (same || !(device_ids && n_ids > 0)) return 0;
        set_error("h2hip_init: already initialised with a different device list; call h2hip_shutdown first");
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < ids.size(); i++) {
        if (ids[i] < 0 || ids[i] >= count) {
            set_error("device id %d out of range (0..%d)", ids[i], count - 1);
            return H2HIP_EINVAL;
        }
        for (size_t j = 0; j < i; j++)
            if (ids[j] == ids[i] && !g_cfg.allow_dup) {
                set_error("device id %d listed twice (HALO2_HIP_ALLOW_DUPLICATE_DEVICES=1 allows it for rehearsals)", ids[i]);
                return H2HIP_EINVAL;
            }
    }
    if (g_cfg.roctx) roctx_load();
    g_devs.clear();
    g_devs.push_back(c);
    int rc = init_one(c, ids[0]);
    for (size_t i = 1; !rc && i < ids.size(); i++) {
        Ctx* x = new Ctx();
        g_devs.push_back(x);
        rc = init_one(x, ids[i]);
    }
    if (rc) {
        for (size_t i = 0; i < g_devs.size(); i++) {
            release_ctx(g_devs[i]);
            if (i) delete g_devs[i];
        }
        g_devs.clear();
        return rc;
    }
    (void)hipSetDevice(ids[0]);
    // secondary devices: worker threads, and RCCL communicators for the gather of the partials (distinct devices only)
    g_workers.assign(ids.size(), nullptr);
    for (size_t i = 1; i < ids.size(); i++) {
        g_workers[i] = new Worker();
        g_workers[i]->th = std::thread(worker_main, g_workers[i], ids[i]);
    }
    if (ids.size() > 1 && g_cfg.gather_rccl) (void)rccl_comms_create();  // not fatal: the host gathers the partials instead
    return 0;
}

int ensure_init() {
    if (g_init_failed.load(std::memory_order_acquire)) {  // no usable GPU, found out once: the CPU-fallback path takes no lock and makes no HIP call
        set_error("no usable HIP device (cached from the first attempt; h2hip_init or h2hip_shutdown retries); libhalo2hip has no CPU fallback");
        return H2HIP_EDEVICE;
    }
    {
        std::shared_lock<std::shared_mutex> lk(g_engine_mu);
        if (ctx()->ready) return 0;
    }
    return do_init(nullptr, 0);  // takes the engine lock exclusively; a second thread arriving here finds the engine ready
}

static inline void xyzz_to_out(const XYZZ& r, uint64_t out_xyz[12]) {
    Jac j = xyzz_to_jac(r);
    memcpy(out_xyz, &j, 96);
}

int check_fr(const uint64_t v[4], const char* what) {
    Fe f = fe_from_u64x4(v);
    if (!fe_is_canonical<FrP>(f)) {
        set_error("%s is not a reduced Fr element", what);
        return H2HIP_EINVAL;
    }
    return 0;
}

Entry::Entry(const char* name, const void* d_ptr, bool all_devices) : c(ctx()), rc(0) {
    for (;;) {
        rc = ensure_init();
        if (rc) return;
        engine = std::shared_lock<std::shared_mutex>(g_engine_mu);
        if (ctx()->ready) break;
        engine.unlock();  // shut down by another thread in between: initialise again
    }
    if (d_ptr && g_devs.size() > 1) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_ptr) == hipSuccess) {
            Ctx* owner = nullptr;
            for (Ctx* x : g_devs)
                if (x->device == at.device) {
                    owner = x;
                    break;
                }
            if (!owner) {
                set_error("device pointer belongs to device %d, which is not in h2hip_init's list", at.device);
                rc = H2HIP_EINVAL;
                return;
            }
            c = owner;
        } else {
            (void)hipGetLastError();
        }
    }
    if (all_devices) {
        for (Ctx* x : g_devs) held.emplace_back(x->mu);
    } else {
        held.emplace_back(c->mu);
    }
    if (hipSetDevice(c->device) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", c->device);
        rc = H2HIP_EDEVICE;
        return;
    }
    if (name && g_roctx_push) {
        g_roctx_push(name);
        ranged = true;
    }
}
Entry::~Entry() {
    if (ranged) g_roctx_pop();
}

static int ntt_host(uint64_t* a, const Fe& omega, uint32_t log_n, const NttScale* sc, const uint64_t* src, size_t src_elems) {
    Entry en("h2hip_ntt_host");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    size_t bytes = sizeof(Fe) << log_n;
    int rc = c->ntt_io.ensure(bytes);
    if (rc) return rc;
    const void* from = src ? (const void*)src : (const void*)a;
    size_t in_bytes = src ? src_elems * sizeof(Fe) : bytes;
    H2_CHECK(hipMemcpyAsync(c->ntt_io.p, from, in_bytes, hipMemcpyHostToDevice, c->stream));
    rc = ntt_device(c, (Fe*)c->ntt_io.p, omega, log_n, sc, c->stream);
    if (rc) return rc;
    H2_CHECK(hipMemcpyAsync(a, c->ntt_io.p, bytes, hipMemcpyDeviceToHost, c->stream));
    H2_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- host-pointer batched transforms: a three-stage pipeline over the columns ----------------------------------------------------
// create_proof converts its columns back to back from `Vec<F>`s (plonk/prover.rs:487 lagrange_to_coeff per advice column,
// plonk/evaluation.rs:306-323 coeff_to_extended per advice / instance column).  One call each means upload -> transform ->
// download in series, 11.6 x the device-resident transform at 2^22 (round 3).  Here column i + 1 crosses PCIe upwards and column
// i - 1 downwards (full duplex, one copier thread per direction: pageable hipMemcpyAsync blocks its caller) while column i is
// transformed on the engine's stream: per column max(upload, transform, download) instead of their sum.
// A batch is cut into runs of Tuning::ntt_host_batch_bytes of device memory, and small columns are grouped per pipeline step.
struct PipeDrain {  // every exit: the copiers idle, their streams drained -- nothing touches the caller's columns after the call
    Ctx* c;
    hipStream_t su, sd;
    ~PipeDrain() {
        copier_abort(c, false, SIZE_MAX);
        copier_abort(c, true, SIZE_MAX);
        (void)hipStreamSynchronize(su);
        (void)hipStreamSynchronize(sd);
    }
};

// m columns: in[i] (in_elems elements) -> out[i] (2^log_n elements); in[i] == out[i] is fine (every column is read before it is written)
static int ntt_host_pipeline(Ctx* c, const uint64_t* const* in, size_t in_elems, uint64_t* const* out, size_t m, const Fe& omega, uint32_t log_n,
                             const NttScale* sc) {
    const size_t col = sizeof(Fe) << log_n, in_bytes = in_elems * sizeof(Fe);
    size_t gc = tune().ntt_host_group_bytes / col;
    if (gc < 1) gc = 1;
    const size_t G = (m + gc - 1) / gc;
    int rc;
    if ((rc = c->ntt_io.ensure(m * col))) return rc;
    if ((rc = c->ensure_aux(2 * G + 2))) return rc;
    hipStream_t s = c->stream, su = c->aux2, sd = c->aux1;
    hipEvent_t* ev = c->aux_events.data();  // [2g] group g uploaded, [2g + 1] group g transformed
    char* base = (char*)c->ntt_io.p;
    H2_CHECK(hipStreamSynchronize(s));
    if ((rc = copier_begin(c, false, su))) return rc;
    if ((rc = copier_begin(c, true, sd))) return rc;
    PipeDrain drain{c, su, sd};
    std::vector<CopyJob> jobs;
    std::vector<Fe*> cols(m);
    for (size_t i = 0; i < m; i++) {
        cols[i] = (Fe*)(base + i * col);
        jobs.push_back(CopyJob{cols[i], in[i], in_bytes, ((i + 1) % gc == 0 || i + 1 == m) ? ev[2 * (i / gc)] : nullptr, nullptr, false});
    }
    if ((rc = copier_push(c, false, jobs))) return rc;
    for (size_t g = 0; g < G; g++) {
        const size_t i0 = g * gc, cnt = m - i0 < gc ? m - i0 : gc;
        if ((rc = copier_wait(c, false, i0 + cnt))) return rc;
        H2_CHECK(hipStreamWaitEvent(s, ev[2 * g], 0));
        rc = cnt == 1 ? ntt_device(c, cols[i0], omega, log_n, sc, s) : ntt_device_batch(c, cols.data() + i0, nullptr, cnt, omega, log_n, sc, s);
        if (rc) return rc;
        H2_CHECK(hipEventRecord(ev[2 * g + 1], s));
        for (size_t i = i0; i < i0 + cnt; i++) jobs.push_back(CopyJob{out[i], cols[i], col, nullptr, i == i0 ? ev[2 * g + 1] : nullptr, true});
        if ((rc = copier_push(c, true, jobs))) return rc;
    }
    if ((rc = copier_wait(c, true, m))) return rc;
    H2_CHECK(hipStreamSynchronize(sd));
    H2_CHECK(hipStreamSynchronize(s));
    return 0;
}

static int ntt_host_batch_on(Ctx* c, const uint64_t* const* in, size_t in_elems, uint64_t* const* out, size_t count, const Fe& omega, uint32_t log_n,
                             const NttScale* sc) {
    const size_t col = sizeof(Fe) << log_n;
    size_t per = tune().ntt_host_batch_bytes / col;
    if (per < 2) per = 2;
    const bool threads = count > 1 && copier_ready(c, false) && copier_ready(c, true);
    for (size_t i0 = 0; i0 < count; i0 += per) {
        const size_t m = count - i0 < per ? count - i0 : per;
        if (m > 1 && threads) {
            int rc = ntt_host_pipeline(c, in + i0, in_elems, out + i0, m, omega, log_n, sc);
            if (rc) return rc;
            continue;
        }
        for (size_t i = i0; i < i0 + m; i++) {  // a lone column (or no copier threads): upload, transform, download in order
            int rc = c->ntt_io.ensure(col);
            if (rc) return rc;
            H2_CHECK(hipMemcpyAsync(c->ntt_io.p, in[i], in_elems * sizeof(Fe), hipMemcpyHostToDevice, c->stream));
            if ((rc = ntt_device(c, (Fe*)c->ntt_io.p, omega, log_n, sc, c->stream))) return rc;
            H2_CHECK(hipMemcpyAsync(out[i], c->ntt_io.p, col, hipMemcpyDeviceToHost, c->stream));
            H2_CHECK(hipStreamSynchronize(c->stream));
        }
    }
    return 0;
}

// NTT replicas (second bullet): with several devices the columns are dealt in contiguous shares, every device
// runs the pipeline on its share over its own PCIe link; no column crosses xGMI.
static int ntt_host_batch(const char* name, const uint64_t* const* in, size_t in_elems, uint64_t* const* out, size_t count, const Fe& omega,
                          uint32_t log_n, const NttScale* sc) {
    if (!count) return 0;
    bool multi;
    {
        Entry en(name);
        if (en.rc) return en.rc;
        multi = g_devs.size() > 1 && count > 1;
        if (!multi) return ntt_host_batch_on(en.c, in, in_elems, out, count, omega, log_n, sc);
    }
    Entry en(name, nullptr, true);
    if (en.rc) return en.rc;
    const size_t nd = g_devs.size() < count ? g_devs.size() : count;
    return on_devices((int)nd, [&](int d) -> int {
        const size_t lo = count * (size_t)d / nd, hi = count * ((size_t)d + 1) / nd;
        Ctx* x = g_devs[(size_t)d];
        H2_CHECK(hipSetDevice(x->device));
        return ntt_host_batch_on(x, in + lo, in_elems, out + lo, hi - lo, omega, log_n, sc);
    });
}

static void release_ctx(Ctx* c) {
    copier_stop(c);
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->ready) (void)hipDeviceSynchronize();
    c->timers_collect();
    c->timers.clear();
    ntt_twiddles_free(c);
    evalh_modules_free(c);
    for (auto& kv : c->pinned) {
        (void)hipFree(kv.second.d);
        if (kv.second.d_sample) (void)hipFree(kv.second.d_sample);
    }
    c->pinned.clear();
    c->pins.clear();
    c->pin_flag.release();
    c->ntt_ws.release();
    c->ntt_io.release();
    for (int k = 0; k < 3; k++) {
        c->msm_scalars[k].release();
        c->msm_slot[k].release();
    }
    c->msm_bases.release();
    c->host_ws.release();
    c->host_planes.release();
    c->stage.release();
    c->stage_off = 0;
    c->misc.release();
    c->evalh_ws.release();
    c->evalh_slots.release();
    c->ecfft_ws.release();
    c->ntt_ptrs.release();
    c->gather.release();
    c->gen_table.release();
    c->host_io.release();
    c->prod_ws.release();
    c->mvsum_ws.release();
    c->open_ws.release();
    c->open_io.release();
    c->lookup_ws.release();
    c->lookup_flag.release();
    c->keygen_ws.release();
    c->keygen_flag.release();
    c->check_ws.release();
    c->check_flag.release();
    c->copies_ws.release();
    c->copies_flag.release();
    c->serde_ws.release();
    c->ipa_ws.release();
    c->ipa_vals.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = nullptr;
    for (auto e : c->aux_events) (void)hipEventDestroy(e);
    c->aux_events.clear();
    if (c->aux1) (void)hipStreamDestroy(c->aux1);
    if (c->aux2) (void)hipStreamDestroy(c->aux2);
    if (c->aux_b) (void)hipStreamDestroy(c->aux_b);
    c->aux1 = c->aux2 = c->aux_b = nullptr;
    if (c->ws_event) (void)hipEventDestroy(c->ws_event);
    c->ws_event = nullptr;
    c->ws_used = false;
    c->ready = false;
}

// drop `key` from every device's pinned cache; true when it was there
static bool unpin_everywhere(const void* key) {
    bool found = false;
    for (Ctx* x : g_devs) {
        auto it = x->pinned.find(key);
        if (it == x->pinned.end()) continue;
        found = true;
        (void)hipSetDevice(x->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(it->second.d);
        if (it->second.d_sample) (void)hipFree(it->second.d_sample);
        x->pinned.erase(it);
    }
    if (!g_devs.empty()) (void)hipSetDevice(g_devs[0]->device);
    return found;
}

// A host-keyed pinned entry serves this call only if n fits and the caller's array still carries the sampled points:
// a mismatch means the allocation was freed and reused -- the entry is dropped on every device.  A prefix so short that
// fewer than four samples fall inside it (n <= total >> 12) is not vouched for by the fingerprint (point 0 of every KZG
// `g` is the generator): such a call bypasses the entry (returns false, entry kept) and uploads its few points.
static bool pinned_validate(const uint64_t* bases_xy, size_t n) {
    Ctx* c = ctx();
    auto it = c->pinned.find((const void*)bases_xy);
    if (it == c->pinned.end() || it->second.device_key) return true;
    size_t total = 0;
    for (Ctx* x : g_devs) {
        auto jt = x->pinned.find((const void*)bases_xy);
        if (jt != x->pinned.end() && jt->second.hi > total) total = jt->second.hi;
    }
    bool ok = n <= total;
    if (ok) {
        for (uint32_t k = 0; ok && k < H2_PIN_SAMPLES; k++) {
            const size_t i = pin_sample_index(total, k);
            if (i < n) ok = memcmp(it->second.sample + 64 * k, bases_xy + 8 * i, 64) == 0;
        }
    }
    if (!ok) {
        ::lazy_forget((const void*)bases_xy);
        (void)unpin_everywhere((const void*)bases_xy);
        return true;  // nothing left to bypass
    }
    return n == total || n > pin_sample_index(total, 3);
}

// ---- device-pointer keys (h2hip_bases_pin_device) ---------------------------------------------------------------------------
// The key is a device address; torch's caching allocator hands the same address out again readily, so a caller that freed a
// pinned buffer without unpinning it would get the OLD table's commitments.  Guard: the entry keeps H2_PIN_SAMPLES points of
// the array in device memory; the first workgroup of the MSM's first kernel (msm_l1_count_kernel) compares them with the caller's buffer and writes its
// verdict to a pinned host word, which is read when the MSM's own result has arrived (the call waits for that anyway: no extra
// synchronisation).  A mismatch drops the entry and the MSM is run again in the plain form over the caller's points.
__global__ void pin_sample_kernel(const Affine* __restrict__ src, size_t total, Affine* __restrict__ out) {
    if (threadIdx.x < H2_PIN_SAMPLES) out[threadIdx.x] = src[pin_sample_index(total, threadIdx.x)];
}

// window table of a device-pointer key on context c, if n fits; *entry gets the cache entry
static const MsmTable* pinned_table(Ctx* c, const void* key, size_t n, MsmTable* out, const PinnedBases** entry) {
    auto it = c->pinned.find(key);
    if (it == c->pinned.end() || !it->second.device_key || n > it->second.n || !it->second.c) return nullptr;
    out->table = it->second.d;
    out->stride = it->second.n;
    out->c = it->second.c;
    out->W = it->second.W;
    out->rec = it->second.rec;
    *entry = &it->second;
    return out;
}

// `count` MSMs over device-resident scalars and bases on context c: the fixed-base form when d_bases is a pinned key whose
// fingerprint still matches, else the plain form.  Synchronous (the sums come back through the host).
static int msm_device_keyed(Ctx* c, const Fe* const* d_scalars, const Affine* d_bases, size_t n, size_t count, XYZZ* out, hipStream_t s) {
    MsmTable tab;
    const PinnedBases* pb = nullptr;
    const MsmTable* t = (n && count) ? pinned_table(c, d_bases, n, &tab, &pb) : nullptr;
    if (t && n != pb->n && n <= pin_sample_index(pb->n, 3)) t = nullptr;  // too short a prefix for the fingerprint to vouch for: plain form
    volatile uint32_t* flag = nullptr;
    if (t && pb->d_sample) {
        int rc = c->pin_flag.ensure(64);
        if (rc) return rc;
        flag = (volatile uint32_t*)c->pin_flag.p;
        *flag = 0;
        c->pin_chk.bases = d_bases;
        c->pin_chk.samples = (const Affine*)pb->d_sample;
        c->pin_chk.flag = (uint32_t*)c->pin_flag.p;
        c->pin_chk.n = n;
        c->pin_chk.total = pb->n;
    }
    int rc = msm_batch_device(c, d_scalars, false, d_bases, n, count, out, s, t);
    c->pin_chk = Ctx::PinCheck();
    if (rc || !flag || !*flag) return rc;
    // stale: another array lives at the pinned address now
    H2_CHECK(hipDeviceSynchronize());
    auto it = c->pinned.find((const void*)d_bases);
    if (it != c->pinned.end()) {
        (void)hipFree(it->second.d);
        if (it->second.d_sample) (void)hipFree(it->second.d_sample);
        c->pinned.erase(it);
    }
    return msm_batch_device(c, d_scalars, false, d_bases, n, count, out, s, nullptr);
}

// (pinned proving-key columns: see h2hip_columns_pin further down)
void column_sample(const uint64_t* h_col, size_t elems, uint8_t* out) {
    for (uint32_t k = 0; k < H2_COL_SAMPLES; k++) memcpy(out + 32 * k, h_col + 4 * pin_sample_index(elems, k), 32);
}

// ---- the pin cache (engine.h, PinCache)
Pin* PinCache::find(Kind kind, const void* key) {
    auto it = pins.find({kind, key});
    return it == pins.end() ? nullptr : &it->second;
}

void PinCache::drop(Pin* p) {
    (void)hipFree(p->d);
    p->d = nullptr;
    auto it = pins.find({p->kind, p->key});
    if (it == pins.end() || &it->second != p) return;  // never listed
    bytes[p->kind] -= p->bytes;
    count[p->kind]--;
    pins.erase(it);
}

const Fe* PinCache::lookup(Kind kind, const void* key, bool dev, size_t elems, const PinDomain& dom) {
    Pin* p = find(kind, key);
    if (!p || p->device_key != dev || !(p->dom == dom)) return nullptr;
    if (!dev) {
        uint8_t now[H2_COL_SAMPLES * 32];
        if (p->elems == elems) column_sample((const uint64_t*)key, elems, now);
        if (p->elems != elems || memcmp(now, p->sample, sizeof(now)) != 0) {  // another array lives at this address now: forget the copy
            (void)hipDeviceSynchronize();
            drop(p);
            return nullptr;
        }
    }
    p->last_use = ++tick;
    return (const Fe*)p->d;
}

int PinCache::make_room(size_t need, size_t budget, bool* fits) {
    *fits = need <= budget;
    if (!*fits) return 0;
    while (bytes[COLUMN] + bytes[PARTS] + need > budget) {
        Pin* lru = nullptr;
        for (auto& kv : pins)
            if (!lru || kv.second.last_use < lru->last_use) lru = &kv.second;
        if (!lru) break;
        H2_CHECK(hipDeviceSynchronize());  // a queued evaluate_h may still read the copy
        drop(lru);
    }
    return 0;
}

void PinCache::insert(Pin p) {
    if (!p.device_key) column_sample((const uint64_t*)p.key, p.elems, p.sample);
    p.last_use = ++tick;
    bytes[p.kind] += p.bytes;
    count[p.kind]++;
    pins[{p.kind, p.key}] = p;
}

void PinCache::clear() {
    while (!pins.empty()) drop(&pins.begin()->second);
}

const Fe* pinned_column_lookup(Ctx* c, const uint64_t* h_col, size_t elems) {
    return c->pins.lookup(PinCache::COLUMN, h_col, false, elems, PinDomain());
}

// (the Entry of the caller holds the engine lock shared: the configuration cannot change under it)
int pinned_make_room(Ctx* c, size_t bytes, bool* fits) { return c->pins.make_room(bytes, g_cfg.column_cache_bytes, fits); }

int pinned_unpin(PinCache::Kind kind, const void* const* keys, size_t count, const char* name) {
    if (count && !keys) return H2HIP_EINVAL;
    {
        TuneRead r;  // the engine lock shared, without starting the engine: nothing is pinned in one that is not running
        if (!ctx()->ready) return 0;
    }
    Entry en(name);
    if (en.rc) return en.rc;
    bool synced = false;
    for (size_t i = 0; i < count; i++) {
        Pin* p = en.c->pins.find(kind, keys[i]);
        if (!p) continue;
        if (!synced) {
            H2_CHECK(hipDeviceSynchronize());  // a queued evaluate_h may still read the copy
            synced = true;
        }
        en.c->pins.drop(p);
    }
    return 0;
}

int pinned_info(PinCache::Kind kind, size_t* n, size_t* device_bytes, const char* name) {
    Entry en(name);
    if (en.rc) return en.rc;
    if (n) *n = en.c->pins.count[kind];
    if (device_bytes) *device_bytes = en.c->pins.bytes[kind];
    return 0;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2hip_init(const int* device_ids, int n_devices) { return do_init(device_ids, n_devices); }

void h2hip_shutdown(void) {
    Ctx* c = ctx();
    std::unique_lock<std::shared_mutex> lk(g_engine_mu);  // waits for every running entry point
    g_init_failed.store(0, std::memory_order_release);     // the next call looks for a GPU again
    if (!c->ready) return;
    for (size_t i = 1; i < g_workers.size(); i++) {
        Worker* w = g_workers[i];
        {
            std::lock_guard<std::mutex> wl(w->m);
            w->quit = true;
            w->cv.notify_all();
        }
        w->th.join();
        delete w;
    }
    g_workers.clear();
    for (ncclComm_t cm : g_rccl.comms)
        if (cm) (void)g_rccl.CommDestroy(cm);
    g_rccl.comms.clear();
    for (size_t i = g_devs.size(); i-- > 0;) {
        release_ctx(g_devs[i]);
        if (i) delete g_devs[i];
    }
    g_devs.clear();
    lazy_reset();
    evalh_rtc_shutdown();
}

const char* h2hip_last_error(void) { return g_err; }
const char* h2hip_version(void) { return "halo2hip 0.2 (gfx950)"; }

int h2hip_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return -1;
    return count;
}

int h2hip_num_devices(void) {
    std::shared_lock<std::shared_mutex> lk(g_engine_mu);
    return ctx()->ready ? (int)g_devs.size() : 0;
}

// The shim asks these on every best_multiexp / best_fft, from rayon workers: the configuration is read under the engine lock
// (h2hip_init may be rewriting it), and without a usable GPU they answer "never" from the cached failure -- no lock, no HIP call.
size_t h2hip_msm_min_n(void) {
    if (ensure_init()) return SIZE_MAX;
    std::shared_lock<std::shared_mutex> lk(g_engine_mu);
    return g_cfg.msm_min_n;
}

uint32_t h2hip_ntt_min_log_n(void) {
    if (ensure_init()) return UINT32_MAX;
    std::shared_lock<std::shared_mutex> lk(g_engine_mu);
    return g_cfg.ntt_min_log_n;
}

int h2hip_msm_bn254_device(const void* d_scalars, const void* d_bases_xy, size_t n, uint64_t out_xyz[12], void* stream) {
    if (!out_xyz || (n && (!d_scalars || !d_bases_xy))) {
        set_error("msm: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_msm_bn254_device", d_scalars);
    if (en.rc) return en.rc;
    hipStream_t s = (hipStream_t)stream;
    XYZZ r;
    const Fe* sc = (const Fe*)d_scalars;
    int rc = msm_device_keyed(en.c, &sc, (const Affine*)d_bases_xy, n, 1, &r, s);
    if (rc) return rc;
    xyzz_to_out(r, out_xyz);
    return 0;
}

// `count` MSMs of n pairs with host-resident scalars on device context c: the bases come from c's pinned copy of
// key[lo .. lo + n) when there is one (with its window table), else they are uploaded.
static int msm_shard_host(Ctx* c, const uint64_t* const* scalars, const uint64_t* bases_xy, size_t lo, size_t n, size_t count, XYZZ* out,
                          bool use_cache = true) {
    std::vector<const Fe*> sc(count);
    for (size_t j = 0; j < count; j++) sc[j] = (const Fe*)scalars[j] + lo;
    MsmTable tab;
    const Affine *d_bases = nullptr, *h_bases = nullptr;
    const MsmTable* t = nullptr;
    auto it = c->pinned.find((const void*)bases_xy);
    if (use_cache && it != c->pinned.end() && it->second.lo <= lo && lo + n <= it->second.hi) {
        const PinnedBases& pb = it->second;
        d_bases = (const Affine*)pb.d + (lo - pb.lo);  // (without a table: the points themselves)
        if (pb.c) {
            tab.table = (const char*)pb.d + (lo - pb.lo) * pb.rec;
            tab.stride = pb.n;
            tab.c = pb.c;
            tab.W = pb.W;
            tab.rec = pb.rec;
            t = &tab;
        }
    } else {
        h_bases = (const Affine*)bases_xy + lo;  // unpinned: the points cross PCIe inside the run, chunk by chunk when it streams
    }
    return msm_batch_device(c, sc.data(), true, d_bases, n, count, out, c->stream, t, h_bases);
}

// The partials of the devices meet on the host: every device's run has already returned its sums through pinned memory (the
// call is synchronous), so the left fold of arithmetic.rs:153 is n_use - 1 additions on numbers the calling thread holds.
static void fold_host(int n_use, size_t count, const std::vector<std::vector<XYZZ>>& parts, uint64_t* out_xyz) {
    for (size_t j = 0; j < count; j++) {
        XYZZ acc = xyzz_identity();
        for (int d = 0; d < n_use; d++) xyzz_add(acc, parts[(size_t)d][j]);
        xyzz_to_out(acc, out_xyz + 12 * j);
    }
}

// HALO2_HIP_GATHER=rccl (fixed-base form only: one set sum per MSM): the sums stage C left in every device's `gather` buffer
// (Ctx::gather_want) are all-gathered device to device over xGMI -- 128 B per (device, MSM), ncclUint8, one group call --
// copied down once from the first device and folded on the host.  all[d * count + j] = sum of MSM j on device d.
// Any failure leaves `all` untouched; the caller then folds the host copies instead.
static int gather_rccl(size_t count, std::vector<XYZZ>* all) {
    const int nd = (int)g_devs.size();
    const size_t bytes = count * sizeof(XYZZ);
    if (g_rccl.comms.size() != (size_t)nd || bytes > H2_GATHER_OWN) return H2HIP_EINVAL;
    ncclResult_t nr = g_rccl.GroupStart();
    for (int d = 0; nr == ncclSuccess && d < nd; d++) {
        Ctx* x = g_devs[(size_t)d];
        nr = g_rccl.AllGather(x->gather.p, (char*)x->gather.p + H2_GATHER_OWN, bytes, ncclUint8, g_rccl.comms[(size_t)d], x->stream);
    }
    ncclResult_t ne = g_rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) {
        set_error("ncclAllGather failed: %s", g_rccl.GetErrorString(nr));
        return H2HIP_EDEVICE;
    }
    std::vector<XYZZ> got((size_t)nd * count);
    Ctx* c0 = g_devs[0];
    H2_CHECK(hipSetDevice(c0->device));
    H2_CHECK(hipMemcpyAsync(got.data(), (char*)c0->gather.p + H2_GATHER_OWN, bytes * (size_t)nd, hipMemcpyDeviceToHost, c0->stream));
    H2_CHECK(hipStreamSynchronize(c0->stream));
    for (int d = 1; d < nd; d++) {  // every rank's collective has drained before the buffers are reused
        H2_CHECK(hipSetDevice(g_devs[(size_t)d]->device));
        H2_CHECK(hipStreamSynchronize(g_devs[(size_t)d]->stream));
    }
    H2_CHECK(hipSetDevice(c0->device));
    all->swap(got);
    return 0;
}

static int msm_host_common(const uint64_t* const* scalars, const uint64_t* bases_xy, size_t n, size_t count, uint64_t* out_xyz) {
    Entry en("h2hip_msm_bn254", nullptr, true);
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    if (n == 0 || count == 0) {
        for (size_t j = 0; j < count; j++) xyzz_to_out(xyzz_identity(), out_xyz + 12 * j);
        return 0;
    }
    // a pinned entry whose fingerprint no longer matches the caller's array is stale (the allocation was freed and
    // reused): drop it on every device and fall back to uploading
    const bool use_cache = pinned_validate(bases_xy, n);
    lazy_pin_consider(bases_xy, n);
    const int nd = (int)g_devs.size();
    if (nd == 1 || n < g_cfg.multi_gpu_min_n || !use_cache) {
        std::vector<XYZZ> r(count);
        int rc = msm_shard_host(c, scalars, bases_xy, 0, n, count, r.data(), use_cache);
        if (rc) return rc;
        for (size_t j = 0; j < count; j++) xyzz_to_out(r[j], out_xyz + 12 * j);
        return 0;
    }
    // Several devices: contiguous ranges of pairs per device, as best_multiexp chunks them over threads
    // (arithmetic.rs:137-152).  Pinned bases fix the partition (each device holds its range and its window table).
    std::vector<size_t> lo((size_t)nd), hi((size_t)nd);
    auto it0 = c->pinned.find((const void*)bases_xy);
    if (it0 != c->pinned.end()) {
        for (int d = 0; d < nd; d++) {
            auto it = g_devs[(size_t)d]->pinned.find((const void*)bases_xy);
            size_t l = it != g_devs[(size_t)d]->pinned.end() ? it->second.lo : n, h = it != g_devs[(size_t)d]->pinned.end() ? it->second.hi : n;
            lo[(size_t)d] = l < n ? l : n;
            hi[(size_t)d] = h < n ? h : n;
        }
    } else {
        const size_t per = n / (size_t)nd;
        for (int d = 0; d < nd; d++) {
            lo[(size_t)d] = (size_t)d * per;
            hi[(size_t)d] = d == nd - 1 ? n : (size_t)(d + 1) * per;
        }
    }
    std::vector<std::vector<XYZZ>> parts((size_t)nd, std::vector<XYZZ>(count, xyzz_identity()));
    // RCCL gather only when asked for, communicators exist and every device runs the fixed-base form over its pinned share
    bool use_rccl = g_cfg.gather_rccl && g_rccl.comms.size() == (size_t)nd && count * sizeof(XYZZ) <= H2_GATHER_OWN;
    for (int d = 0; use_rccl && d < nd; d++) {
        auto it = g_devs[(size_t)d]->pinned.find((const void*)bases_xy);
        const bool idle = hi[(size_t)d] == lo[(size_t)d];
        if (!idle && (it == g_devs[(size_t)d]->pinned.end() || !it->second.c)) use_rccl = false;
    }
    int rc = on_devices(nd, [&](int d) -> int {
        Ctx* x = g_devs[(size_t)d];
        const size_t m = hi[(size_t)d] - lo[(size_t)d];
        x->gather_want = false;
        x->gather_off = 0;
        if (use_rccl) {
            int r = x->gather.ensure(H2_GATHER_OWN * (size_t)(nd + 1));
            if (r) return r;
            H2_CHECK(hipMemsetAsync(x->gather.p, 0, count * sizeof(XYZZ), x->stream));  // an idle device contributes identities
            x->gather_want = true;
        }
        int r = m ? msm_shard_host(x, scalars, bases_xy, lo[(size_t)d], m, count, parts[(size_t)d].data()) : 0;
        x->gather_want = false;
        return r;
    });
    if (rc) return rc;
    if (use_rccl) {
        for (int d = 0; d < nd; d++)
            if (hi[(size_t)d] != lo[(size_t)d] && g_devs[(size_t)d]->gather_off != count * sizeof(XYZZ)) use_rccl = false;  // not one run per device
    }
    if (use_rccl) {
        std::vector<XYZZ> all;
        if (gather_rccl(count, &all) == 0) {
            for (int d = 0; d < nd; d++)
                for (size_t j = 0; j < count; j++) parts[(size_t)d][j] = all[(size_t)d * count + j];
        }  // else: the host copies are complete and correct -- fold those
    }
    fold_host(nd, count, parts, out_xyz);
    return 0;
}

int h2hip_msm_bn254(const uint64_t* scalars, const uint64_t* bases_xy, size_t n, uint64_t out_xyz[12]) {
    if (!out_xyz || (n && (!scalars || !bases_xy))) {
        set_error("msm: null argument");
        return H2HIP_EINVAL;
    }
    return msm_host_common(&scalars, bases_xy, n, 1, out_xyz);
}

int h2hip_msm_bn254_batch(const uint64_t* const* scalars, const uint64_t* bases_xy, size_t n, size_t count, uint64_t* out_xyz) {
    if ((count && (!out_xyz || !scalars)) || (n && count && !bases_xy)) {
        set_error("msm_batch: null argument");
        return H2HIP_EINVAL;
    }
    for (size_t j = 0; j < count; j++)
        if (n && !scalars[j]) {
            set_error("msm_batch: scalars[%zu] is null", j);
            return H2HIP_EINVAL;
        }
    return msm_host_common(scalars, bases_xy, n, count, out_xyz);
}

int h2hip_msm_bn254_batch_device(const void* const* d_scalars, const void* d_bases_xy, size_t n, size_t count, uint64_t* out_xyz, void* stream) {
    if ((count && (!out_xyz || !d_scalars)) || (n && count && !d_bases_xy)) {
        set_error("msm_batch: null argument");
        return H2HIP_EINVAL;
    }
    for (size_t j = 0; j < count; j++)
        if (n && !d_scalars[j]) {
            set_error("msm_batch: d_scalars[%zu] is null", j);
            return H2HIP_EINVAL;
        }
    Entry en("h2hip_msm_bn254_batch_device", count ? d_scalars[0] : nullptr);
    if (en.rc) return en.rc;
    std::vector<XYZZ> r(count);
    int rc = msm_device_keyed(en.c, (const Fe* const*)d_scalars, (const Affine*)d_bases_xy, n, count, r.data(), (hipStream_t)stream);
    if (rc) return rc;
    for (size_t j = 0; j < count; j++) xyzz_to_out(r[j], out_xyz + 12 * j);
    return 0;
}


// Pin points [lo, hi) of the caller's array on device context c (worker thread of that device, or the caller's for
// device 0): device copy + window table.  d_src != nullptr: the points already live on this device.
static int pin_on_device(Ctx* c, const void* key, const uint64_t* h_points, const void* d_src, size_t lo, size_t hi, size_t n_total,
                         const uint8_t* sample, bool device_key) {
    (void)n_total;
    auto it = c->pinned.find(key);
    if (it != c->pinned.end()) {
        H2_CHECK(hipDeviceSynchronize());
        (void)hipFree(it->second.d);
        if (it->second.d_sample) (void)hipFree(it->second.d_sample);
        c->pinned.erase(it);
    }
    if (hi <= lo) return 0;
    const size_t n = hi - lo;
    PinnedBases pb;
    pb.n = n;
    pb.lo = lo;
    pb.hi = hi;
    pb.device_key = device_key;
    if (sample) memcpy(pb.sample, sample, sizeof(pb.sample));
    uint32_t cw = 0, W = 1, rec = sizeof(Affine);
    if (g_cfg.fixed_base && n <= ((size_t)1 << 26)) {
        cw = msm_table_window(n);
        W = (255 + cw - 1) / cw;
        rec = msm_table_rec(n, tune().table_records);
        if ((size_t)W * n * rec > g_cfg.table_max_bytes) rec = sizeof(Affine);  // the native table would be refused: the E-form one may still fit
        if ((size_t)W * n * rec > g_cfg.table_max_bytes) cw = 0, W = 1;
    }
    hipError_t e = hipMalloc(&pb.d, (size_t)W * n * rec);
    if (e != hipSuccess && cw && rec != sizeof(Affine)) {  // no room for the native table: the E-form one
        (void)hipGetLastError();
        rec = sizeof(Affine);
        e = hipMalloc(&pb.d, (size_t)W * n * rec);
    }
    if (e != hipSuccess && cw) {  // no room for the table: keep the points only
        (void)hipGetLastError();
        cw = 0;
        W = 1;
        e = hipMalloc(&pb.d, n * sizeof(Affine));
    }
    if (e != hipSuccess) {
        set_error("bases_pin: hipMalloc(%zu) failed: %s", (size_t)W * n * rec, hipGetErrorString(e));
        return H2HIP_ENOMEM;
    }
    int rc = 0;
    if (d_src) {
        if (!cw) H2_CHECK(hipMemcpyAsync(pb.d, (const Affine*)d_src + lo, n * sizeof(Affine), hipMemcpyDeviceToDevice, c->stream));
    } else {  // (under a native table the points only pass through here: the build copies them out before it writes row 0 over them)
        H2_CHECK(hipMemcpyAsync(pb.d, (const Affine*)h_points + lo, n * sizeof(Affine), hipMemcpyHostToDevice, c->stream));
    }
    if (cw) {
        c->table_rec = rec;
        rc = msm_table_build(c, d_src ? (const Affine*)d_src + lo : (const Affine*)pb.d, n, cw, (Affine*)pb.d, c->stream);
        c->table_rec = sizeof(Affine);
    }
    if (!rc && device_key) {  // the fingerprint of a device key stays on the device
        if (hipMalloc(&pb.d_sample, H2_PIN_SAMPLES * sizeof(Affine)) != hipSuccess) {
            (void)hipGetLastError();
            pb.d_sample = nullptr;
            set_error("bases_pin: hipMalloc of the fingerprint failed");
            rc = H2HIP_ENOMEM;
        } else {
            hipLaunchKernelGGL(pin_sample_kernel, dim3(1), dim3(64), 0, c->stream, (const Affine*)d_src + lo, n, (Affine*)pb.d_sample);
        }
    }
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) {
        set_error("bases_pin: table build failed");
        rc = H2HIP_EDEVICE;
    }
    if (rc) {
        (void)hipFree(pb.d);
        if (pb.d_sample) (void)hipFree(pb.d_sample);
        return rc;
    }
    pb.c = cw;
    pb.W = cw ? W : 0;
    pb.rec = cw ? rec : (uint32_t)sizeof(Affine);
    c->pinned[key] = pb;
    return 0;
}

static void pin_sample(const uint64_t* bases_xy, size_t n, uint8_t* out) {
    for (uint32_t k = 0; k < H2_PIN_SAMPLES; k++) memcpy(out + 64 * k, bases_xy + 8 * pin_sample_index(n, k), 64);
}

// pin a host array on every device (its contiguous share each): the body of h2hip_bases_pin, also reached by the lazy cache
static int pin_host_everywhere(const uint64_t* bases_xy, size_t n) {
    uint8_t sample[H2_PIN_SAMPLES * 64];
    pin_sample(bases_xy, n, sample);
    const int nd = (int)g_devs.size();
    const int use = n >= g_cfg.multi_gpu_min_n ? nd : 1;
    const size_t per = n / (size_t)use;
    int rc = on_devices(nd, [&](int d) -> int {
        size_t lo = d < use ? (size_t)d * per : n, hi = d < use ? (d == use - 1 ? n : (size_t)(d + 1) * per) : n;
        return pin_on_device(g_devs[(size_t)d], (const void*)bases_xy, bases_xy, nullptr, lo, hi, n, sample, false);
    });
    if (rc) (void)unpin_everywhere((const void*)bases_xy);
    return rc;
}

int h2hip_bases_pin(const uint64_t* bases_xy, size_t n) {
    if (!bases_xy || !n) {
        set_error("bases_pin: null/empty");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_bases_pin", nullptr, true);
    if (en.rc) return en.rc;
    lazy_forget((const void*)bases_xy);  // an explicit pin is the caller's to unpin
    return pin_host_everywhere(bases_xy, n);
}

// ---- optional lazy cache (HALO2_HIP_LAZY_PIN=k, off by default) ----------------------------------------------------------
// The unpatched drop-in calls best_multiexp(coeffs, &params.g[..]) with no handle in the signature and uploads 64 B per
// point every time.  With the knob set, a host array that arrives unpinned for the k-th time with the same address and
// the same sampled points is pinned by the library itself (window table included).  From then on it is an ordinary
// pinned entry: every lookup re-checks the 16 sampled points and a mismatch drops it, so a freed and reused
// allocation costs an upload, not a wrong commitment; what the samples cannot see is a caller that rewrites part of a
// live array in place -- ParamsKZG never does (downsize truncates g and builds a new g_lagrange, kzg/commitment.rs:267-275),
// which is why the knob is opt-in.  At most H2_LAZY_MAX arrays are held this way, the least recently used goes first.
#define H2_LAZY_MAX 4
struct LazySeen {
    const void* key;
    size_t n;
    uint32_t count;
    uint8_t sample[H2_PIN_SAMPLES * 64];
};
static std::vector<LazySeen> g_lazy_seen;        // candidates, at most 8, oldest first
static std::vector<const void*> g_lazy_pinned;   // arrays this cache pinned, least recently used first

static void lazy_reset() {
    g_lazy_seen.clear();
    g_lazy_pinned.clear();
}

static void lazy_forget(const void* key) {
    for (size_t i = 0; i < g_lazy_seen.size(); i++)
        if (g_lazy_seen[i].key == key) {
            g_lazy_seen.erase(g_lazy_seen.begin() + (long)i);
            break;
        }
    for (size_t i = 0; i < g_lazy_pinned.size(); i++)
        if (g_lazy_pinned[i] == key) {
            g_lazy_pinned.erase(g_lazy_pinned.begin() + (long)i);
            break;
        }
}

// called by the host-pointer MSMs after pinned_validate; pins `bases_xy` when it has been seen often enough
static void lazy_pin_consider(const uint64_t* bases_xy, size_t n) {
    if (!tune().lazy_pin_after || n < 1024) return;
    const void* key = (const void*)bases_xy;
    if (ctx()->pinned.count(key)) {  // in use: refresh its place in the LRU order if it is ours
        for (size_t i = 0; i + 1 < g_lazy_pinned.size(); i++)
            if (g_lazy_pinned[i] == key) {
                g_lazy_pinned.erase(g_lazy_pinned.begin() + (long)i);
                g_lazy_pinned.push_back(key);
                break;
            }
        return;
    }
    for (size_t i = 0; i < g_lazy_pinned.size(); i++)  // ours once, dropped since by a failed validation
        if (g_lazy_pinned[i] == key) {
            g_lazy_pinned.erase(g_lazy_pinned.begin() + (long)i);
            break;
        }
    uint8_t sample[H2_PIN_SAMPLES * 64];
    pin_sample(bases_xy, n, sample);
    LazySeen* e = nullptr;
    for (auto& x : g_lazy_seen)
        if (x.key == key) e = &x;
    if (!e) {
        if (g_lazy_seen.size() >= 8) g_lazy_seen.erase(g_lazy_seen.begin());
        g_lazy_seen.push_back(LazySeen());
        e = &g_lazy_seen.back();
        e->key = key;
        e->count = 0;
    }
    if (e->count && (e->n != n || memcmp(e->sample, sample, sizeof(sample)) != 0)) e->count = 0;  // another array at this address
    e->n = n;
    memcpy(e->sample, sample, sizeof(sample));
    if (++e->count < tune().lazy_pin_after) return;
    lazy_forget(key);
    while (g_lazy_pinned.size() >= H2_LAZY_MAX) {
        (void)unpin_everywhere(g_lazy_pinned.front());
        g_lazy_pinned.erase(g_lazy_pinned.begin());
    }
    if (pin_host_everywhere(bases_xy, n) == 0) g_lazy_pinned.push_back(key);  // a failed pin (no room for the table) just leaves the upload path
}

uint32_t h2hip_lazy_pin_after(void) {
    if (ensure_init()) return 0;
    std::shared_lock<std::shared_mutex> lk(g_engine_mu);
    return tune().lazy_pin_after;
}

// test hook: the knob without the environment
int h2hip_debug_set_lazy_pin(uint32_t after) {
    TuneWrite()->lazy_pin_after = after;
    return 0;
}

int h2hip_bases_pin_device(const void* d_bases_xy, size_t n, void* stream) {
    if (!d_bases_xy || !n) {
        set_error("bases_pin_device: null/empty");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_bases_pin_device", d_bases_xy);
    if (en.rc) return en.rc;
    H2_CHECK(hipStreamSynchronize((hipStream_t)stream));  // the points may have been produced on the caller's stream
    return pin_on_device(en.c, d_bases_xy, nullptr, d_bases_xy, 0, n, n, nullptr, true);
}

int h2hip_bases_unpin(const void* bases_xy) {
    {
        std::shared_lock<std::shared_mutex> eng(g_engine_mu);
        if (!ctx()->ready) {  // nothing can be pinned; do not start the engine for this (interpreter teardown after h2hip_shutdown)
            set_error("bases_unpin: pointer was not pinned (engine not initialised)");
            return H2HIP_EINVAL;
        }
    }
    Entry en("h2hip_bases_unpin", nullptr, true);
    if (en.rc) return en.rc;
    lazy_forget(bases_xy);
    if (!unpin_everywhere(bases_xy)) {
        set_error("bases_unpin: pointer was not pinned");
        return H2HIP_EINVAL;
    }
    return 0;
}

// test hook: push `count` Jacobian partials per engine device through the library's RCCL gather (communicators are
// created on demand, also for a single device) and fold them; out = fold over the devices of partials_xyz[j].
int h2hip_debug_rccl_gather_selftest(const uint64_t* partials_xyz, size_t count, uint64_t* out_xyz) {
    if (!partials_xyz || !out_xyz || !count) {
        set_error("rccl_gather_selftest: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_debug_rccl_gather_selftest", nullptr, true);
    if (en.rc) return en.rc;
    int rc = rccl_comms_create();
    if (rc) return rc;
    const int nd = (int)g_devs.size();
    if (count * sizeof(XYZZ) > H2_GATHER_OWN) {
        set_error("rccl_gather_selftest: at most %zu partials", H2_GATHER_OWN / sizeof(XYZZ));
        return H2HIP_EINVAL;
    }
    std::vector<XYZZ> mine(count);
    for (size_t j = 0; j < count; j++) {
        Jac jc;
        memcpy(&jc, partials_xyz + 12 * j, 96);
        mine[j] = jac_to_xyzz(jc);
    }
    rc = on_devices(nd, [&](int d) -> int {  // stands in for stage C of a run: the device's sums land in its gather buffer
        Ctx* x = g_devs[(size_t)d];
        int r = x->gather.ensure(H2_GATHER_OWN * (size_t)(nd + 1));
        if (r) return r;
        H2_CHECK(hipMemcpyAsync(x->gather.p, mine.data(), count * sizeof(XYZZ), hipMemcpyHostToDevice, x->stream));
        H2_CHECK(hipStreamSynchronize(x->stream));
        return 0;
    });
    if (rc) return rc;
    std::vector<XYZZ> all;
    if ((rc = gather_rccl(count, &all))) return rc;
    std::vector<std::vector<XYZZ>> parts((size_t)nd, std::vector<XYZZ>(count));
    for (int d = 0; d < nd; d++)
        for (size_t j = 0; j < count; j++) parts[(size_t)d][j] = all[(size_t)d * count + j];
    fold_host(nd, count, parts, out_xyz);
    return 0;
}

int h2hip_bases_pinned_info(const void* bases_xy, size_t* n_points, uint32_t* window_bits, uint32_t* windows, size_t* device_bytes) {
    Entry en(nullptr, nullptr, true);
    if (en.rc) return en.rc;
    size_t n = 0, bytes = 0;
    uint32_t c = 0, W = 0;
    bool found = false;
    for (Ctx* x : g_devs) {
        auto it = x->pinned.find(bases_xy);
        if (it == x->pinned.end()) continue;
        found = true;
        n += it->second.n;
        bytes += (size_t)(it->second.c ? it->second.W : 1) * it->second.n * it->second.rec;
        if (it->second.c) c = it->second.c, W = it->second.W;
    }
    if (!found) {
        set_error("bases_pinned_info: pointer is not pinned");
        return H2HIP_EINVAL;
    }
    if (n_points) *n_points = n;
    if (window_bits) *window_bits = c;
    if (windows) *windows = W;
    if (device_bytes) *device_bytes = bytes;
    return 0;
}

int h2hip_g1_fold(const uint64_t* partials_xyz, size_t k, uint64_t out_xyz[12]) {
    if (!out_xyz || (k && !partials_xyz)) {
        set_error("g1_fold: null argument");
        return H2HIP_EINVAL;
    }
    XYZZ acc = xyzz_identity();
    for (size_t i = 0; i < k; i++) {
        Jac j;
        memcpy(&j, partials_xyz + 12 * i, 96);
        xyzz_add(acc, jac_to_xyzz(j));
    }
    xyzz_to_out(acc, out_xyz);
    return 0;
}

int h2hip_g1_batch_normalize(const uint64_t* xyz, size_t k, uint64_t* xy) {
    if (k && (!xyz || !xy)) {
        set_error("g1_batch_normalize: null argument");
        return H2HIP_EINVAL;
    }
    // Montgomery's trick on the z coordinates (identity points are skipped)
    std::vector<Fe> prefix(k);
    Fe acc = fe_one<Q>();
    for (size_t i = 0; i < k; i++) {
        Jac j;
        memcpy(&j, xyz + 12 * i, 96);
        prefix[i] = acc;
        if (!fe_is_zero(j.z)) acc = fe_mul<Q>(acc, j.z);
    }
    Fe inv = fe_inv<Q>(acc);
    for (size_t i = k; i-- > 0;) {
        Jac j;
        memcpy(&j, xyz + 12 * i, 96);
        Affine a;
        if (fe_is_zero(j.z)) {
            a.x = fe_zero<Q>();
            a.y = fe_zero<Q>();
        } else {
            Fe zi = fe_mul<Q>(inv, prefix[i]);
            inv = fe_mul<Q>(inv, j.z);
            Fe zi2 = fe_sqr<Q>(zi);
            a.x = fe_mul<Q>(j.x, zi2);
            a.y = fe_mul<Q>(j.y, fe_mul<Q>(zi2, zi));
        }
        memcpy(xy + 8 * i, &a, 64);
    }
    return 0;
}

int h2hip_device_alloc(size_t bytes, void** d_ptr) {
    if (!d_ptr) {
        set_error("device_alloc: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_device_alloc");
    if (en.rc) return en.rc;
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
    if (e != hipSuccess) {
        *d_ptr = nullptr;
        set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return H2HIP_ENOMEM;
    }
    return 0;
}

int h2hip_device_free(void* d_ptr) {
    Entry en("h2hip_device_free", d_ptr);
    if (en.rc) return en.rc;
    H2_CHECK(hipDeviceSynchronize());
    H2_CHECK(hipFree(d_ptr));
    return 0;
}

int h2hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    if (bytes && (!d_dst || !h_src)) {
        set_error("memcpy_h2d: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_memcpy_h2d", d_dst);
    if (en.rc) return en.rc;
    H2_CHECK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    H2_CHECK(hipStreamSynchronize((hipStream_t)stream));  // the source is a borrowed host slice
    return 0;
}

int h2hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes && (!h_dst || !d_src)) {
        set_error("memcpy_d2h: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_memcpy_d2h", d_src);
    if (en.rc) return en.rc;
    H2_CHECK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    H2_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int h2hip_memset_zero(void* d_dst, size_t bytes, void* stream) {
    if (bytes && !d_dst) {
        set_error("memset_zero: null argument");
        return H2HIP_EINVAL;
    }
    Entry en("h2hip_memset_zero", d_dst);
    if (en.rc) return en.rc;
    H2_CHECK(hipMemsetAsync(d_dst, 0, bytes, (hipStream_t)stream));
    return 0;
}

int h2hip_stream_synchronize(void* stream) {
    Entry en("h2hip_stream_synchronize");
    if (en.rc) return en.rc;
    H2_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int h2hip_g1_to_affine(const uint64_t xyz[12], uint64_t xy[8]) {
    if (!xyz || !xy) {
        set_error("g1_to_affine: null argument");
        return H2HIP_EINVAL;
    }
    Jac j;
    memcpy(&j, xyz, 96);
    Affine a = xyzz_to_affine(jac_to_xyzz(j));
    memcpy(xy, &a, 64);
    return 0;
}

// few-term sums on the calling thread (include/halo2hip_g1.h): no Entry, no engine lock, no HIP call
int h2hip_g1_linear_combinations_bn254(const uint64_t* addends_xyz, const uint64_t* scalars, const uint64_t* points_xy, size_t m, size_t t,
                                       uint64_t* out_xy) {
    char why[160];
    if (g1h::linear_combinations(addends_xyz, scalars, points_xy, m, t, out_xy, why, sizeof(why))) {
        set_error("g1_linear_combinations: %s", why);
        return H2HIP_EINVAL;
    }
    return 0;
}

// ---- the NTT / domain family ---------------------------------------------------------------------------------------------------------
// Four operations (ntt, ifft, coeff_to_extended, extended_to_coeff) in up to four forms each: _device, host, _batch_device and _batch.
// What an operation accepts is written once, in its parse_* below.  An entry point says what is its form's own (Form: its pointers, how its
// rejections are worded), has the operation parsed into a DomainOp and hands that to its form's runner: ntt_device under an Entry,
// ntt_host, batch_over_devices or ntt_host_batch.
// One struct for both kinds of form, because a batch form's column checks fall between the null / size checks and the check_fr list.
struct Form {
    // the single forms:
    bool ptrs;          // the form's own pointers are there
    const char* msg;    // text for a null pointer, a bad size or k > extended_k; nullptr (the batch forms): H2HIP_EINVAL without a text
    bool size;          // log_n > 28 is rejected under `msg` (the _device forms of ntt and ifft leave that to ntt_device)
    // the batch forms: the name their column checks speak of, and the tables of `count` columns (in == out: in place)
    const char* batch;
    const void* const* in;
    const void* const* out;
    size_t count;
};
static Form single(bool ptrs, const char* msg, bool size = true) { return {ptrs, msg, size, nullptr, nullptr, nullptr, 0}; }
static Form batch_host(const char* name, const uint64_t* const* in, uint64_t* const* out, size_t count) {  // host columns
    return {true, nullptr, false, name, (const void* const*)in, (const void* const*)out, count};
}
static Form batch_device(const char* name, void* const* d_a, size_t count) {  // device columns, in place
    return {true, nullptr, false, name, (const void* const*)d_a, (const void* const*)d_a, count};
}

// the checks that come before an operation's check_fr list; args_ok: its scalars are there and k <= extended_k
static int form_check(const Form& f, bool args_ok, uint32_t log_n) {
    if (!f.ptrs || !args_ok || (f.size && log_n > 28)) {
        if (f.msg) set_error("%s", f.msg);
        return H2HIP_EINVAL;
    }
    if (!f.batch) return 0;
    if (log_n > 28 || (f.count && (!f.in || !f.out))) {
        set_error("%s: bad argument", f.batch);
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < f.count; i++)
        if (!f.in[i] || !f.out[i]) {
            set_error("%s: null column %zu", f.batch, i);
            return H2HIP_EINVAL;
        }
    return 0;
}

struct DomainOp {  // a parsed call: the transform's root and size, log2 of the elements read per column, the fused scaling if any
    Fe omega;
    uint32_t log_n, in_log;
    bool scaled;
    NttScale scale;
    const NttScale* sc() const { return scaled ? &scale : nullptr; }
    size_t in_elems() const { return (size_t)1 << in_log; }  // for the host forms, whose sizes have been checked
};

static int parse_ntt(const Form& f, const uint64_t* omega, uint32_t log_n, DomainOp* op) {
    if (int rc = form_check(f, omega, log_n)) return rc;
    if (check_fr(omega, "omega")) return H2HIP_EINVAL;
    *op = {fe_from_u64x4(omega), log_n, log_n, false, NttScale()};
    return 0;
}

static int parse_ifft(const Form& f, const uint64_t* omega_inv, uint32_t log_n, const uint64_t* divisor, DomainOp* op) {
    if (int rc = form_check(f, omega_inv && divisor, log_n)) return rc;
    if (check_fr(omega_inv, "omega_inv") || check_fr(divisor, "divisor")) return H2HIP_EINVAL;
    *op = {fe_from_u64x4(omega_inv), log_n, log_n, true, NttScale::inverse(fe_from_u64x4(divisor))};
    return 0;
}

static int parse_coeff_to_extended(const Form& f, uint32_t k, uint32_t extended_k, const uint64_t* extended_omega, const uint64_t* g_coset,
                                   const uint64_t* g_coset_inv, DomainOp* op) {
    if (int rc = form_check(f, extended_omega && g_coset && g_coset_inv && k <= extended_k, extended_k)) return rc;
    if (check_fr(extended_omega, "extended_omega") || check_fr(g_coset, "g_coset") || check_fr(g_coset_inv, "g_coset_inv")) return H2HIP_EINVAL;
    *op = {fe_from_u64x4(extended_omega), extended_k, k, true, NttScale::into_coset(fe_from_u64x4(g_coset), fe_from_u64x4(g_coset_inv), 1ull << k)};
    return 0;
}

static int parse_extended_to_coeff(const Form& f, uint32_t extended_k, const uint64_t* extended_omega_inv, const uint64_t* extended_ifft_divisor,
                                   const uint64_t* g_coset, const uint64_t* g_coset_inv, DomainOp* op) {
    if (int rc = form_check(f, extended_omega_inv && extended_ifft_divisor && g_coset && g_coset_inv, extended_k)) return rc;
    if (check_fr(extended_omega_inv, "extended_omega_inv") || check_fr(extended_ifft_divisor, "extended_ifft_divisor") ||
        check_fr(g_coset, "g_coset") || check_fr(g_coset_inv, "g_coset_inv"))
        return H2HIP_EINVAL;
    *op = {fe_from_u64x4(extended_omega_inv), extended_k, extended_k, true,
           NttScale::out_of_coset(fe_from_u64x4(extended_ifft_divisor), fe_from_u64x4(g_coset), fe_from_u64x4(g_coset_inv))};
    return 0;
}

// the _device forms' runner: in place on a device column, under the Entry of the device that owns it
static int run_device(const char* name, void* d_a, const DomainOp& op, void* stream) {
    Entry en(name, d_a);
    if (en.rc) return en.rc;
    return ntt_device(en.c, (Fe*)d_a, op.omega, op.log_n, op.sc(), (hipStream_t)stream);
}

// SURVEY.md 8(e), second bullet: NTTs are single-GPU, but independent transforms (the coset NTTs of
// plonk/evaluation.rs:306-323) can run on several GPUs as whole columns.  A batch whose columns all live on one engine device
// runs there, asynchronously on the caller's stream, under that device's lock only.  A batch whose columns live on SEVERAL
// engine devices is split by owner: each device transforms its own columns as one batch on its engine stream, the groups run
// concurrently (one host thread per device), and the call returns when all of them are done (the caller's stream is
// synchronised first).  No column crosses xGMI: the caller decides the placement.  With the same device listed twice
// (HALO2_HIP_ALLOW_DUPLICATE_DEVICES, rehearsal) the columns of that device are dealt round-robin to its contexts.
// owner[i] = index (in the engine's device list) of the context that transforms column i; *mixed: more than one context is involved.
// Called with the engine lock held (inside an Entry).
static int batch_owners(const char* name, void* const* d_a, size_t count, std::vector<int>* owner, bool* mixed) {
    const int nd = (int)g_devs.size();
    owner->assign(count, 0);
    *mixed = false;
    if (nd <= 1) return 0;
    std::vector<int> next_dup((size_t)nd, 0);
    for (size_t i = 0; i < count; i++) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_a[i]) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: column %zu is not a device pointer", name, i);
            return H2HIP_EINVAL;
        }
        std::vector<int> cand;
        for (int d = 0; d < nd; d++)
            if (g_devs[(size_t)d]->device == at.device) cand.push_back(d);
        if (cand.empty()) {
            set_error("%s: column %zu lives on device %d, which is not in h2hip_init's list", name, i, at.device);
            return H2HIP_EINVAL;
        }
        (*owner)[i] = cand[(size_t)(next_dup[(size_t)cand[0]]++) % cand.size()];
        if ((*owner)[i] != (*owner)[0]) *mixed = true;
    }
    return 0;
}

static int batch_over_devices(const char* name, void* const* d_a, size_t count, void* stream, uint32_t log_n, const Fe& omega, const NttScale* sc) {
    if (!count) return 0;
    std::vector<int> owner;
    bool mixed = false;
    {
        Entry en(name, d_a[0]);
        if (en.rc) return en.rc;
        int rc = batch_owners(name, d_a, count, &owner, &mixed);
        if (rc) return rc;
        if (!mixed) return ntt_device_batch(en.c, (Fe* const*)d_a, nullptr, count, omega, log_n, sc, (hipStream_t)stream);
    }
    Entry en(name, nullptr, true);  // several devices: all their locks, in list order
    if (en.rc) return en.rc;
    int rc = batch_owners(name, d_a, count, &owner, &mixed);  // again, now that the device list cannot change under the call
    if (rc) return rc;
    const int nd = (int)g_devs.size();
    H2_CHECK(hipStreamSynchronize((hipStream_t)stream));  // the columns may have been produced on the caller's stream
    std::vector<std::vector<Fe*>> cols((size_t)nd);
    for (size_t i = 0; i < count; i++) cols[(size_t)owner[i]].push_back((Fe*)d_a[i]);
    return on_devices(nd, [&](int d) -> int {
        Ctx* x = g_devs[(size_t)d];
        if (cols[(size_t)d].empty()) return 0;
        H2_CHECK(hipSetDevice(x->device));
        int r = ntt_device_batch(x, cols[(size_t)d].data(), nullptr, cols[(size_t)d].size(), omega, log_n, sc, x->stream);
        if (r) return r;
        H2_CHECK(hipStreamSynchronize(x->stream));
        return 0;
    });
}

int h2hip_ntt_bn254_fr_device(void* d_a, const uint64_t omega[4], uint32_t log_n, void* stream) {
    DomainOp op;
    if (int rc = parse_ntt(single(d_a, "ntt: null argument", false), omega, log_n, &op)) return rc;
    return run_device("h2hip_ntt_bn254_fr_device", d_a, op, stream);
}

int h2hip_ntt_bn254_fr(uint64_t* a, const uint64_t omega[4], uint32_t log_n) {
    DomainOp op;
    if (int rc = parse_ntt(single(a, "ntt: bad argument"), omega, log_n, &op)) return rc;
    return ntt_host(a, op.omega, op.log_n, op.sc(), nullptr, 0);
}

int h2hip_ntt_bn254_fr_batch_device(void* const* d_a, size_t count, const uint64_t omega[4], uint32_t log_n, void* stream) {
    DomainOp op;
    if (int rc = parse_ntt(batch_device("ntt_batch", d_a, count), omega, log_n, &op)) return rc;
    return batch_over_devices("h2hip_ntt_bn254_fr_batch_device", d_a, count, stream, op.log_n, op.omega, op.sc());
}

int h2hip_ntt_bn254_fr_batch(uint64_t* const* a, size_t count, const uint64_t omega[4], uint32_t log_n) {
    DomainOp op;
    if (int rc = parse_ntt(batch_host("ntt_batch", a, a, count), omega, log_n, &op)) return rc;
    return ntt_host_batch("h2hip_ntt_bn254_fr_batch", a, op.in_elems(), a, count, op.omega, op.log_n, op.sc());
}

int h2hip_ifft_bn254_fr_device(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void* stream) {
    DomainOp op;
    if (int rc = parse_ifft(single(d_a, "ifft: null argument", false), omega_inv, log_n, divisor, &op)) return rc;
    return run_device("h2hip_ifft_bn254_fr_device", d_a, op, stream);
}

int h2hip_ifft_bn254_fr(uint64_t* a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]) {
    DomainOp op;
    if (int rc = parse_ifft(single(a, "ifft: bad argument"), omega_inv, log_n, divisor, &op)) return rc;
    return ntt_host(a, op.omega, op.log_n, op.sc(), nullptr, 0);
}

int h2hip_ifft_bn254_fr_batch_device(void* const* d_a, size_t count, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4],
                                     void* stream) {
    DomainOp op;
    if (int rc = parse_ifft(batch_device("ifft_batch", d_a, count), omega_inv, log_n, divisor, &op)) return rc;
    return batch_over_devices("h2hip_ifft_bn254_fr_batch_device", d_a, count, stream, op.log_n, op.omega, op.sc());
}

int h2hip_ifft_bn254_fr_batch(uint64_t* const* a, size_t count, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]) {
    DomainOp op;
    if (int rc = parse_ifft(batch_host("ifft_batch", a, a, count), omega_inv, log_n, divisor, &op)) return rc;
    return ntt_host_batch("h2hip_ifft_bn254_fr_batch", a, op.in_elems(), a, count, op.omega, op.log_n, op.sc());
}

int h2hip_coeff_to_extended_bn254_fr_device(void* d_a, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                                            const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* stream) {
    DomainOp op;
    const Form f = single(d_a, "coeff_to_extended: bad argument");
    if (int rc = parse_coeff_to_extended(f, k, extended_k, extended_omega, g_coset, g_coset_inv, &op)) return rc;
    return run_device("h2hip_coeff_to_extended_bn254_fr_device", d_a, op, stream);
}

int h2hip_coeff_to_extended_bn254_fr(const uint64_t* a, uint32_t k, uint64_t* out, uint32_t extended_k,
                                     const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]) {
    DomainOp op;
    const Form f = single(a && out, "coeff_to_extended: bad argument");
    if (int rc = parse_coeff_to_extended(f, k, extended_k, extended_omega, g_coset, g_coset_inv, &op)) return rc;
    return ntt_host(out, op.omega, op.log_n, op.sc(), a, op.in_elems());
}

int h2hip_coeff_to_extended_bn254_fr_batch_device(void* const* d_a, size_t count, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                                                  const uint64_t g_coset[4], const uint64_t g_coset_inv[4], void* stream) {
    DomainOp op;
    const Form f = batch_device("coeff_to_extended_batch", d_a, count);
    if (int rc = parse_coeff_to_extended(f, k, extended_k, extended_omega, g_coset, g_coset_inv, &op)) return rc;
    return batch_over_devices("h2hip_coeff_to_extended_bn254_fr_batch_device", d_a, count, stream, op.log_n, op.omega, op.sc());
}

int h2hip_coeff_to_extended_bn254_fr_batch(const uint64_t* const* a, uint32_t k, uint64_t* const* out, size_t count, uint32_t extended_k,
                                           const uint64_t extended_omega[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]) {
    DomainOp op;
    const Form f = batch_host("coeff_to_extended_batch", a, out, count);
    if (int rc = parse_coeff_to_extended(f, k, extended_k, extended_omega, g_coset, g_coset_inv, &op)) return rc;
    return ntt_host_batch("h2hip_coeff_to_extended_bn254_fr_batch", a, op.in_elems(), out, count, op.omega, op.log_n, op.sc());
}

int h2hip_extended_to_coeff_bn254_fr_device(void* d_a, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                            const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4],
                                            const uint64_t g_coset_inv[4], void* stream) {
    DomainOp op;
    const Form f = single(d_a, "extended_to_coeff: bad argument");
    if (int rc = parse_extended_to_coeff(f, extended_k, extended_omega_inv, extended_ifft_divisor, g_coset, g_coset_inv, &op)) return rc;
    return run_device("h2hip_extended_to_coeff_bn254_fr_device", d_a, op, stream);
}

int h2hip_extended_to_coeff_bn254_fr(uint64_t* a, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                     const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]) {
    DomainOp op;
    const Form f = single(a, "extended_to_coeff: bad argument");
    if (int rc = parse_extended_to_coeff(f, extended_k, extended_omega_inv, extended_ifft_divisor, g_coset, g_coset_inv, &op)) return rc;
    return ntt_host(a, op.omega, op.log_n, op.sc(), nullptr, 0);
}

int h2hip_extended_to_coeff_bn254_fr_batch(uint64_t* const* a, size_t count, uint32_t extended_k, const uint64_t extended_omega_inv[4],
                                           const uint64_t extended_ifft_divisor[4], const uint64_t g_coset[4], const uint64_t g_coset_inv[4]) {
    DomainOp op;
    const Form f = batch_host("extended_to_coeff_batch", a, a, count);
    if (int rc = parse_extended_to_coeff(f, extended_k, extended_omega_inv, extended_ifft_divisor, g_coset, g_coset_inv, &op)) return rc;
    return ntt_host_batch("h2hip_extended_to_coeff_bn254_fr_batch", a, op.in_elems(), a, count, op.omega, op.log_n, op.sc());
}

// EvaluationDomain::divide_by_vanishing_poly: what both forms reject
static int divide_check(const void* a, uint32_t extended_k, const uint64_t* t_evaluations, uint32_t t_len) {
    if (!a || !t_evaluations || extended_k > 28 || t_len == 0) {
        set_error("divide_by_vanishing_poly: bad argument");
        return H2HIP_EINVAL;
    }
    for (uint32_t i = 0; i < t_len; i++)
        if (check_fr(t_evaluations + 4 * i, "t_evaluations[i]")) return H2HIP_EINVAL;
    return 0;
}

int h2hip_divide_by_vanishing_poly_bn254_fr_device(void* d_a, uint32_t extended_k, const uint64_t* t_evaluations, uint32_t t_len, void* stream) {
    if (int rc = divide_check(d_a, extended_k, t_evaluations, t_len)) return rc;
    Entry en("h2hip_divide_by_vanishing_poly_bn254_fr_device", d_a);
    if (en.rc) return en.rc;
    return scale_periodic_device(en.c, (Fe*)d_a, 1ull << extended_k, t_evaluations, t_len, (hipStream_t)stream);
}

int h2hip_divide_by_vanishing_poly_bn254_fr(uint64_t* a, uint32_t extended_k, const uint64_t* t_evaluations, uint32_t t_len) {
    if (int rc = divide_check(a, extended_k, t_evaluations, t_len)) return rc;
    Entry en("h2hip_divide_by_vanishing_poly_bn254_fr");
    if (en.rc) return en.rc;
    Ctx* c = en.c;
    size_t bytes = sizeof(Fe) << extended_k;
    int rc = c->ntt_io.ensure(bytes);
    if (rc) return rc;
    H2_CHECK(hipMemcpyAsync(c->ntt_io.p, a, bytes, hipMemcpyHostToDevice, c->stream));
    rc = scale_periodic_device(c, (Fe*)c->ntt_io.p, 1ull << extended_k, t_evaluations, t_len, c->stream);
    if (rc) return rc;
    H2_CHECK(hipMemcpyAsync(a, c->ntt_io.p, bytes, hipMemcpyDeviceToHost, c->stream));
    H2_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int h2hip_debug_set_ntt_host_batch(uint64_t run_bytes, uint64_t group_bytes) {
    TuneWrite t;
    t->ntt_host_batch_bytes = run_bytes ? (size_t)run_bytes : Tuning{}.ntt_host_batch_bytes;
    t->ntt_host_group_bytes = group_bytes ? (size_t)group_bytes : Tuning{}.ntt_host_group_bytes;
    return 0;
}

// ---- pinned proving-key columns (round 4) ------------------------------------------------------------------------------------------
// The host-pointer evaluate_h (patch 0003's path) uploads every column it is given, and most of them never change between proofs:
// pk.fixed_cosets, pk.l0 / l_last / l_active_row and pk.permutation.cosets are functions of the proving key -- 22 of the 27 full-size
// columns of the k = 18 bench system, 2.8 GB of 3.5 GB per call.  h2hip_columns_pin keeps such columns in HBM keyed by their host
// pointer; evaluate_h_host looks every full-size host column up and skips the upload on a hit.  Guarded like the pinned bases: a
// lookup compares H2_COL_SAMPLES sampled elements of the caller's memory (the first, and a geometric ladder to the last) with what was
// seen at pin time, so a freed and reused allocation costs an upload, never a stale column.  What the samples cannot see is a caller
// rewriting a pinned column in place; a ProvingKey never does.
extern "C" int h2hip_columns_pin(const uint64_t* const* cols, size_t count, size_t elems) {
    if ((count && !cols) || elems == 0 || elems > ((size_t)1 << 28)) {
        set_error("columns_pin: bad argument");
        return H2HIP_EINVAL;
    }
    for (size_t i = 0; i < count; i++)
        if (!cols[i]) {
            set_error("columns_pin: null column %zu", i);
            return H2HIP_EINVAL;
        }
    Entry en("h2hip_columns_pin");
    if (en.rc) return en.rc;
    Ctx* c = en.c;  // evaluate_h runs on the engine's first device
    const size_t bytes = elems * sizeof(Fe);
    for (size_t i = 0; i < count; i++) {
        if (pinned_column_lookup(c, cols[i], elems)) continue;  // already there (and still the same array)
        bool fits;
        if (int rc = pinned_make_room(c, bytes, &fits)) return rc;  // the budget and its LRU are shared with the pinned part cosets
        if (!fits) continue;  // does not fit at all: the call stays correct, this column is uploaded per call
        Pin pc;
        pc.kind = PinCache::COLUMN, pc.key = cols[i], pc.bytes = bytes, pc.elems = elems;
        if (hipMalloc(&pc.d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("columns_pin: out of device memory after %zu of %zu columns (the rest is uploaded per call)", i, count);
            return H2HIP_ENOMEM;
        }
        hipError_t e = hipMemcpyAsync(pc.d, cols[i], bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            c->pins.drop(&pc);
            set_error("columns_pin: upload failed: %s", hipGetErrorString(e));
            return H2HIP_EDEVICE;
        }
        c->pins.insert(pc);
    }
    return 0;
}

extern "C" int h2hip_columns_unpin(const uint64_t* const* cols, size_t count) {
    return pinned_unpin(PinCache::COLUMN, (const void* const*)cols, count, "h2hip_columns_unpin");
}

extern "C" int h2hip_columns_pinned_info(size_t* n_columns, size_t* device_bytes) {
    return pinned_info(PinCache::COLUMN, n_columns, device_bytes, "h2hip_columns_pinned_info");
}

// record form of the window tables pinned from now on: 0 = the engine's choice, 64 = E-form, 80 / 128 = native records at that stride
int h2hip_debug_set_table_records(uint32_t bytes) {
    if (bytes != 0 && bytes != 64 && bytes != 80 && bytes != 128) {
        set_error("debug_set_table_records: 0, 64, 80 or 128 expected");
        return H2HIP_EINVAL;
    }
    TuneWrite()->table_records = bytes;
    return 0;
}

int h2hip_profile_enable(int on) {
    Ctx* c = ctx();
    std::shared_lock<std::shared_mutex> eng(g_engine_mu);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->profiling = on == 1;
    c->profiling_kernel = on == 2;
    return 0;
}

int h2hip_profile_reset(void) {
    Ctx* c = ctx();
    std::shared_lock<std::shared_mutex> eng(g_engine_mu);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->timers_collect();
    c->timers.clear();
    return 0;
}

int h2hip_profile_get(const char* stage, double* total_ms, uint64_t* count) {
    if (!stage || !total_ms || !count) {
        set_error("profile_get: null argument");
        return H2HIP_EINVAL;
    }
    Ctx* c = ctx();
    std::shared_lock<std::shared_mutex> eng(g_engine_mu);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->timers_collect();
    *total_ms = 0.0;
    *count = 0;
    for (auto& t : c->timers)
        if (t.name == stage) {
            *total_ms = t.total_ms;
            *count = t.count;
        }
    return 0;
}

}  // extern "C"
