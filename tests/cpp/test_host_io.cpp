// The staging helper of the host-pointer forms (csrc/engine.h, HostIo) on the stub HIP runtime, which logs the copies and stream waits
// and fails one on request: the slot layout, the pinned-column lookup, the order of the copies and the one wait of a successful call,
// and the drain on every error exit.  Built as test_engine_tsan is (api.hip as plain C++ with tests/cpp/hipstub and engine_stubs.cpp)
// with -fsanitize=address,undefined; driven by tests/test_host_cpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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
    T.on = true;
    T.fail_malloc = false;
    T.fail_copy = -1;
    T.calls.clear();
    T.mallocs.clear();
}
static size_t count_kind(char kind) {
    size_t k = 0;
    for (const h2stub::Call& x : T.calls) k += x.kind == kind;
    return k;
}

// ---- layout: the device pointers are base + the running sum in call order; packed slots exact, aligned ones rounded to 256; the buffer
// is asked for exactly the total
static void layout(Ctx* c, bool aligned) {
    const size_t sizes[] = {32, 128, 256, 32 << 4, 32, 32 << 7, 128, 32 << 1};
    const int n = sizeof(sizes) / sizeof(sizes[0]);
    std::vector<std::vector<char>> h(n);
    std::vector<const Fe*> d(n, nullptr);
    trace_reset();
    DevBuf buf;
    {
        HostIo io(c, buf, c->stream, aligned);
        for (int i = 0; i < n; i++) {
            h[i].assign(sizes[i], (char)(i + 1));
            if (i % 3 == 0) io.in(h[i].data(), sizes[i], &d[i]);
            else if (i % 3 == 1) io.out(h[i].data(), sizes[i], &d[i]);
            else io.room(sizes[i], &d[i]);
        }
        CHECK(T.calls.empty() && T.mallocs.empty());  // the plan makes no HIP call
        CHECK(io.upload() == 0);
        size_t sum = 0;
        for (int i = 0; i < n; i++) {
            CHECK((const char*)d[i] == (const char*)buf.p + sum);
            sum += aligned ? align256(sizes[i]) : sizes[i];
        }
        CHECK(io.carve.total == sum);
        CHECK(T.mallocs.size() == 1 && T.mallocs[0] == sum + sum / 8 + 4096);  // DevBuf::ensure(total) -> one hipMalloc of its growth rule
        for (int i = 0; i < n; i += 3) CHECK(memcmp(d[i], h[i].data(), sizes[i]) == 0);
        CHECK(io.finish() == 0);
    }
    buf.release();
}

// ---- the pinned lookup: a pinned column is read where it lies and takes no slot with try_pinned, is uploaded without it, and is
// uploaded when its contents changed since the pin
static void pinned(Ctx* c) {
    const size_t elems = 64, bytes = elems * sizeof(Fe);
    std::vector<uint64_t> a(4 * elems), b(4 * elems);
    for (size_t i = 0; i < a.size(); i++) a[i] = i, b[i] = 7 * i;
    const uint64_t* cols[1] = {a.data()};
    T.on = false;
    CHECK(h2hip_columns_pin(cols, 1, elems) == 0);
    const Fe* where = pinned_column_lookup(c, a.data(), elems);
    CHECK(where != nullptr);
    DevBuf buf;
    for (int pass = 0; pass < 3; pass++) {  // 0: looked up and found; 1: not looked up; 2: looked up after the contents changed
        if (pass == 2) a[0] ^= 1;  // element 0 is always one of the fingerprint's samples
        trace_reset();
        const Fe *da = nullptr, *db = nullptr;
        HostIo io(c, buf, c->stream);
        io.in(a.data(), bytes, &da, pass != 1);
        io.in(b.data(), bytes, &db, pass != 1);  // never pinned
        CHECK(io.upload() == 0);
        if (pass == 0) {
            CHECK(da == where && io.carve.total == bytes && (const void*)db == buf.p);
            CHECK(count_kind('U') == 1 && T.calls[0].src == b.data());
        } else {
            CHECK((const void*)da == buf.p && (const char*)db == (const char*)buf.p + bytes && io.carve.total == 2 * bytes);
            CHECK(count_kind('U') == 2 && T.calls[0].src == a.data() && T.calls[1].src == b.data());
            CHECK(memcmp(da, a.data(), bytes) == 0);
        }
        CHECK(io.finish() == 0);
    }
    T.on = false;
    CHECK(pinned_column_lookup(c, a.data(), elems) == nullptr);  // the stale entry is gone
    buf.release();
}

// ---- one modelled host form: three uploads, a region of the device's own, two downloads; the "driver" copies slot 0 to the first output
// and returns drv_rc (with an error text of its own when non-zero).  The log is examined after the helper went out of scope.
struct Form {
    std::vector<char> in0, in1, in2, out0, out1;
    void* base = nullptr;
    Form() : in0(256, 1), in1(32, 2), in2(512, 3), out0(256, 0), out1(128, 0) {}
    int run(Ctx* c, DevBuf& buf, int drv_rc) {
        char *d0 = nullptr, *d1 = nullptr, *d2 = nullptr, *dr = nullptr, *o0 = nullptr, *o1 = nullptr;
        HostIo io(c, buf, c->stream);
        io.in(in0.data(), in0.size(), &d0);
        io.out(out0.data(), out0.size(), &o0);
        io.in(in1.data(), in1.size(), &d1);
        io.room(64, &dr);
        io.in(in2.data(), in2.size(), &d2);
        io.out(out1.data(), out1.size(), &o1);
        if (int rc = io.upload()) return rc;
        base = buf.p;
        if (drv_rc) {
            set_error("the driver's own text");
            return drv_rc;
        }
        memcpy(o0, d0, in0.size());
        memset(o1, 9, out1.size());
        return io.finish();
    }
};

static void success(Ctx* c) {
    DevBuf buf;
    Form f;
    trace_reset();
    CHECK(f.run(c, buf, 0) == 0);
    const char* base = (const char*)f.base;
    // uploads in registration order, then downloads in registration order, then exactly one wait on the stream
    CHECK(T.calls.size() == 6);
    const h2stub::Call want[6] = {{'U', base, f.in0.data(), 256, c->stream},         {'U', base + 512, f.in1.data(), 32, c->stream},
                                  {'U', base + 608, f.in2.data(), 512, c->stream},   {'D', f.out0.data(), base + 256, 256, c->stream},
                                  {'D', f.out1.data(), base + 1120, 128, c->stream}, {'S', nullptr, nullptr, 0, c->stream}};
    for (int i = 0; i < 6; i++) {
        const h2stub::Call& g = T.calls[i];
        CHECK(g.kind == want[i].kind && g.dst == want[i].dst && g.src == want[i].src && g.bytes == want[i].bytes && g.stream == want[i].stream);
    }
    CHECK(f.out0 == f.in0 && f.out1 == std::vector<char>(128, 9));
    // a further round over the same slots
    trace_reset();
    {
        char* d = nullptr;
        HostIo io(c, buf, c->stream);
        const size_t off = io.out(f.out0.data(), 256, &d);
        io.in_at(f.in2.data(), 256, off);
        CHECK(io.upload() == 0 && io.finish() == 0);
        io.in_at(f.in0.data(), 256, off);
        io.out_at(f.out0.data(), 256, off);
        CHECK(io.upload() == 0 && io.finish() == 0);
    }
    CHECK(T.calls.size() == 6 && T.mallocs.empty());
    const char kinds[] = "UDSUDS";
    for (int i = 0; i < 6; i++) CHECK(T.calls[i].kind == kinds[i]);
    CHECK(f.out0 == f.in0);
    buf.release();
}

// ---- error exits: the original code and text come back, no download follows a failed upload, and the last call on the stream before the
// helper is gone is a wait
static void errors(Ctx* c) {
    DevBuf buf;
    for (int fail_at = 0; fail_at < 5; fail_at++) {  // the three uploads, then the two downloads
        Form f;
        trace_reset();
        T.fail_copy = fail_at;
        CHECK(f.run(c, buf, 0) == H2HIP_EDEVICE);
        const std::string text = h2hip_last_error();
        CHECK(text.find("engine.h:") != std::string::npos && text.find("hipMemcpyAsync(") != std::string::npos &&
              text.find(" -> stub error") != std::string::npos);
        CHECK(T.calls.size() == (size_t)fail_at + 2);  // every copy up to the failing one, then the drain
        CHECK(T.calls.back().kind == 'S' && T.calls.back().stream == c->stream && count_kind('S') == 1);
        CHECK(count_kind('D') == (fail_at < 3 ? 0u : (size_t)fail_at - 2));
    }
    {  // the driver fails between upload() and finish()
        Form f;
        trace_reset();
        CHECK(f.run(c, buf, H2HIP_ELOOKUP) == H2HIP_ELOOKUP);
        CHECK(std::string(h2hip_last_error()) == "the driver's own text");
        CHECK(T.calls.size() == 4 && count_kind('U') == 3 && count_kind('D') == 0 && T.calls.back().kind == 'S' &&
              T.calls.back().stream == c->stream);
    }
    {  // the buffer cannot be had: nothing was queued, nothing is waited for
        DevBuf none;
        Form f;
        trace_reset();
        T.fail_malloc = true;
        CHECK(f.run(c, none, 0) == H2HIP_ENOMEM);
        CHECK(std::string(h2hip_last_error()).find("hipMalloc(") != std::string::npos);
        CHECK(T.calls.empty() && T.mallocs.size() == 1);
    }
    T.on = false;
    T.fail_malloc = false;
    buf.release();
}

int main() {
    setenv("H2_STUB_DEVICES", "1", 1);
    CHECK(h2hip_init(nullptr, 0) == 0);
    Ctx* c = ctx();
    CHECK(c && c->ready && c->stream);
    layout(c, false);
    layout(c, true);
    pinned(c);
    success(c);
    errors(c);
    T.on = false;
    h2hip_shutdown();
    printf("host io: ok\n");
    return 0;
}
