// The pin cache (csrc/engine.h, PinCache: pinned columns and pinned part cosets under one budget and one LRU clock) driven directly on
// the stub HIP runtime, which logs every hipFree and hipDeviceSynchronize: eviction order across both kinds, the oversized request, the
// fingerprint and domain rules of a lookup, and that every entry is freed exactly once -- device memory is the stub's calloc, so a
// double free or a missed one is an AddressSanitizer / LeakSanitizer report.  Built as test_host_io is (api.hip as plain C++ with
// tests/cpp/hipstub and engine_stubs.cpp) with -fsanitize=address,undefined; driven by tests/test_host_cpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "engine.h"

using namespace h2;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static h2stub::Trace& T = h2stub::trace();
static void trace_reset() {
    T.on = T.frees = true;
    T.calls.clear();
}
static size_t count_kind(char kind) {
    size_t k = 0;
    for (const h2stub::Call& x : T.calls) k += x.kind == kind;
    return k;
}
// the log of one call holds exactly these frees, in this order, each with a device synchronisation somewhere before it
static void check_frees(const std::vector<const void*>& want) {
    size_t at = 0;
    bool synced = false;
    for (const h2stub::Call& x : T.calls) {
        if (x.kind == 'Y') synced = true;
        if (x.kind != 'F') continue;
        CHECK(synced && at < want.size() && x.dst == want[at]);
        at++;
    }
    CHECK(at == want.size());
}

static PinDomain domain(uint32_t k, uint32_t ek, uint32_t w = 5, uint32_t g = 7) {
    PinDomain d;
    d.k = k, d.ek = ek, d.ext_omega.l[0] = w, d.g_coset.l[3] = g;
    return d;
}
static const PinDomain NONE;  // a column's

// a caller's array of `elems` elements, every word distinct
static std::vector<uint64_t> column(size_t elems, uint64_t seed) {
    std::vector<uint64_t> v(4 * elems);
    for (size_t i = 0; i < v.size(); i++) v[i] = seed * 1000 + i;
    return v;
}

// what h2hip_columns_pin and part_cosets_pin do once their lookup has missed: room, device memory, (the fill), insert.  The device
// pointer of the new entry, or nullptr when the request exceeds the budget.
static const void* pin(PinCache& pc, size_t budget, PinCache::Kind kind, const void* key, size_t bytes, size_t elems, bool dev, const PinDomain& dom) {
    bool fits = true;
    CHECK(pc.make_room(bytes, budget, &fits) == 0);
    if (!fits) return nullptr;
    Pin p;
    p.kind = kind, p.key = key, p.bytes = bytes, p.elems = elems, p.device_key = dev, p.dom = dom;
    CHECK(hipMalloc(&p.d, bytes) == hipSuccess);
    pc.insert(p);
    return p.d;
}
static void check_totals(const PinCache& pc, size_t n_cols, size_t col_bytes, size_t n_parts, size_t part_bytes) {
    CHECK(pc.count[PinCache::COLUMN] == n_cols && pc.bytes[PinCache::COLUMN] == col_bytes);
    CHECK(pc.count[PinCache::PARTS] == n_parts && pc.bytes[PinCache::PARTS] == part_bytes);
    CHECK(pc.pins.size() == n_cols + n_parts);
}

// ---- 1 and 2: a budget of exactly three entries; the least recently used goes first, whatever its kind; too large a request drops nothing
static void eviction() {
    PinCache pc;
    const size_t budget = 64 + 128 + 128;
    const PinDomain dom = domain(1, 2);
    std::vector<uint64_t> a = column(2, 1), b = column(4, 2), c = column(2, 3), d = column(4, 4), e = column(2, 5), f = column(6, 6);
    trace_reset();
    const void* da = pin(pc, budget, PinCache::COLUMN, a.data(), 64, 2, false, NONE);
    const void* db = pin(pc, budget, PinCache::COLUMN, b.data(), 128, 4, false, NONE);
    const void* dc = pin(pc, budget, PinCache::PARTS, c.data(), 128, 2, false, dom);
    CHECK(da && db && dc && T.calls.empty());  // everything fitted: nothing freed, nothing waited for
    check_totals(pc, 2, 192, 1, 128);
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, 2, NONE) == da);  // the oldest is now the newest: b, c, a
    CHECK(T.calls.empty());

    trace_reset();
    const void* dd = pin(pc, budget, PinCache::COLUMN, d.data(), 128, 4, false, NONE);  // b, a column, goes
    check_frees({db});
    check_totals(pc, 2, 192, 1, 128);
    CHECK(!pc.find(PinCache::COLUMN, b.data()) && pc.find(PinCache::COLUMN, a.data()) && pc.find(PinCache::PARTS, c.data()));

    trace_reset();
    const void* de = pin(pc, budget, PinCache::PARTS, e.data(), 128, 2, false, dom);  // c, the part cosets, goes: a, d, e
    check_frees({dc});
    check_totals(pc, 2, 192, 1, 128);
    CHECK(!pc.find(PinCache::PARTS, c.data()) && pc.find(PinCache::PARTS, e.data()));

    trace_reset();
    CHECK(pin(pc, budget, PinCache::COLUMN, f.data(), 192, 6, false, NONE));  // needs two gone: a, then d; e stays
    check_frees({da, dd});
    check_totals(pc, 1, 192, 1, 128);
    CHECK(pc.find(PinCache::COLUMN, f.data()) && pc.find(PinCache::PARTS, e.data()));

    trace_reset();
    CHECK(pc.lookup(PinCache::PARTS, e.data(), false, 2, dom) == de);  // e, f -> f, e
    CHECK(pin(pc, budget, PinCache::PARTS, c.data(), 128, 2, false, dom));  // f goes
    CHECK(count_kind('F') == 1 && !pc.find(PinCache::COLUMN, f.data()));
    check_totals(pc, 0, 0, 2, 256);

    // an oversized request: not pinned, and nothing is dropped for it
    trace_reset();
    CHECK(pin(pc, budget, PinCache::COLUMN, a.data(), budget + 32, (budget + 32) / 32, false, NONE) == nullptr);
    CHECK(T.calls.empty());
    check_totals(pc, 0, 0, 2, 256);
    CHECK(pin(pc, budget, PinCache::COLUMN, a.data(), 64, 2, false, NONE));  // the rest of the budget is still there to be had
    CHECK(count_kind('F') == 0);
    check_totals(pc, 1, 64, 2, 256);

    trace_reset();
    pc.clear();
    CHECK(count_kind('F') == 3);
    check_totals(pc, 0, 0, 0, 0);
}

// ---- 3: a host key is its fingerprint, a device key is taken on trust
static void fingerprint() {
    PinCache pc;
    const size_t budget = 4096, elems = 8, bytes = elems * sizeof(Fe);
    std::vector<uint64_t> a = column(elems, 1);
    bool sampled[8] = {};
    for (uint32_t k = 0; k < H2_COL_SAMPLES; k++) sampled[pin_sample_index(elems, k)] = true;
    CHECK(sampled[3] && !sampled[2]);
    const void* da = pin(pc, budget, PinCache::COLUMN, a.data(), bytes, elems, false, NONE);
    trace_reset();
    a[4 * 2 + 1] ^= 1;  // an element the fingerprint does not see
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, elems, NONE) == da && T.calls.empty());
    a[4 * 3 + 1] ^= 1;  // one it does
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, elems, NONE) == nullptr);
    check_frees({da});
    check_totals(pc, 0, 0, 0, 0);

    da = pin(pc, budget, PinCache::COLUMN, a.data(), bytes, elems, false, NONE);
    trace_reset();
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, elems / 2, NONE) == nullptr);  // another array: it has another length
    check_frees({da});
    check_totals(pc, 0, 0, 0, 0);

    // part cosets under a host key: the same rule over the 2^k coefficients
    const PinDomain dom = domain(3, 4);
    const void* dp = pin(pc, budget, PinCache::PARTS, a.data(), 2 * bytes, elems, false, dom);
    trace_reset();
    a[4 * 2] ^= 1;
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, elems, dom) == dp && T.calls.empty());
    a[0] ^= 1;
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, elems, dom) == nullptr);
    check_frees({dp});

    // ... and under a device key: the caller's memory is never read (this key cannot be)
    const void* key = (const void*)(uintptr_t)64;
    dp = pin(pc, budget, PinCache::PARTS, key, 2 * bytes, elems, true, dom);
    trace_reset();
    CHECK(pc.lookup(PinCache::PARTS, key, true, elems, dom) == dp && T.calls.empty());
    check_totals(pc, 0, 0, 1, 2 * bytes);
    pc.clear();
}

// ---- 4: an entry for another domain, or with the other kind of key, is not this call's -- and stays
static void domains() {
    PinCache pc;
    const size_t budget = 4096;
    std::vector<uint64_t> a = column(2, 1);
    const PinDomain dom = domain(1, 2);
    const void* dp = pin(pc, budget, PinCache::PARTS, a.data(), 128, 2, false, dom);
    trace_reset();
    const uint64_t before = pc.find(PinCache::PARTS, a.data())->last_use;
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 1, domain(0, 2)) == nullptr);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 2, domain(1, 3)) == nullptr);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 2, domain(1, 2, 6, 7)) == nullptr);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 2, domain(1, 2, 5, 8)) == nullptr);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), true, 2, dom) == nullptr);
    CHECK(T.calls.empty() && pc.find(PinCache::PARTS, a.data())->last_use == before);
    check_totals(pc, 0, 0, 1, 128);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 2, dom) == dp);
    // pinned again for another domain, as part_cosets_pin does it: the old entry's bytes leave once, the new one's come once
    Pin* old = pc.find(PinCache::PARTS, a.data());
    CHECK(old && hipDeviceSynchronize() == hipSuccess);
    pc.drop(old);
    check_totals(pc, 0, 0, 0, 0);
    const void* dq = pin(pc, budget, PinCache::PARTS, a.data(), 256, 2, false, domain(1, 3));
    check_frees({dp});
    check_totals(pc, 0, 0, 1, 256);
    CHECK(pc.lookup(PinCache::PARTS, a.data(), false, 2, domain(1, 3)) == dq && pc.lookup(PinCache::PARTS, a.data(), false, 2, dom) == nullptr);
    pc.clear();
}

// ---- 5: one pointer under both kinds; an entry that never got listed; clear
static void coexistence() {
    PinCache pc;
    const size_t budget = 4096;
    std::vector<uint64_t> a = column(4, 1), b = column(4, 2);
    const PinDomain dom = domain(2, 3);
    const void* dc = pin(pc, budget, PinCache::COLUMN, a.data(), 128, 4, false, NONE);
    const void* dp = pin(pc, budget, PinCache::PARTS, a.data(), 256, 4, false, dom);
    check_totals(pc, 1, 128, 1, 256);
    CHECK(dc != dp && pc.lookup(PinCache::COLUMN, a.data(), false, 4, NONE) == dc && pc.lookup(PinCache::PARTS, a.data(), false, 4, dom) == dp);
    trace_reset();
    pc.drop(pc.find(PinCache::COLUMN, a.data()));
    CHECK(count_kind('F') == 1 && T.calls[0].dst == dc);
    check_totals(pc, 0, 0, 1, 256);
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, 4, NONE) == nullptr && pc.lookup(PinCache::PARTS, a.data(), false, 4, dom) == dp);
    dc = pin(pc, budget, PinCache::COLUMN, a.data(), 128, 4, false, NONE);
    trace_reset();
    pc.drop(pc.find(PinCache::PARTS, a.data()));
    CHECK(count_kind('F') == 1 && T.calls[0].dst == dp);
    check_totals(pc, 1, 128, 0, 0);
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, 4, NONE) == dc && pc.lookup(PinCache::PARTS, a.data(), false, 4, dom) == nullptr);
    dp = pin(pc, budget, PinCache::PARTS, a.data(), 256, 4, false, dom);
    CHECK(pin(pc, budget, PinCache::COLUMN, b.data(), 128, 4, false, NONE));

    // an upload or a build that failed before insert(): its memory is freed, the listed entry of the same kind and key is not touched
    Pin lost;
    lost.kind = PinCache::COLUMN, lost.key = a.data(), lost.bytes = 128, lost.elems = 4;
    CHECK(hipMalloc(&lost.d, 128) == hipSuccess);
    const void* dl = lost.d;
    trace_reset();
    pc.drop(&lost);
    CHECK(count_kind('F') == 1 && T.calls[0].dst == dl && lost.d == nullptr);
    check_totals(pc, 2, 256, 1, 256);
    CHECK(pc.lookup(PinCache::COLUMN, a.data(), false, 4, NONE) == dc);

    trace_reset();
    pc.clear();
    CHECK(count_kind('F') == 3);
    check_totals(pc, 0, 0, 0, 0);
    pc.clear();
    CHECK(count_kind('F') == 3);
}

int main() {
    eviction();
    fingerprint();
    domains();
    coexistence();
    T.on = false;
    printf("pin cache: ok\n");
    return 0;
}
