// Host timing, on 16 threads, of SerdeFormat::Processed's G1 read as the reference does it: ParamsKZG::read_custom's
// load_points_from_file_parallelly (poly/kzg/commitment.rs:173-190) spreads G1Affine::from_bytes, one square root in Fq per point, over
// the cores with `parallelize`.  The arithmetic is the C++ mirror's (host/halo2hip.hpp serde::g1_from_bytes_host: fe_pow over field.h's
// 8 x 32-bit CIOS), not halo2curves' 4 x 64-bit assembly, so the figure is this project's host path, not the reference's.
// tools/serde_bench.py writes the points the GPU decompresses to a file and runs this program on it in the same run.
//   g++ -O3 -std=c++17 -pthread -o tools/serde_host tools/serde_host.cpp -Lhalo2-pse_amd -lhalo2hip -Wl,-rpath,'$ORIGIN/../halo2-pse_amd' -Wl,-rpath,/opt/rocm/lib
//   tools/serde_host <file of n x 32 B> [threads]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <thread>
#include <vector>

#include "../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;

// arithmetic.rs parallelize: contiguous chunks, one per thread
static void parallelize(size_t len, int threads, const std::function<void(size_t, size_t)>& f) {
    std::vector<std::thread> ts;
    const size_t chunk = (len + threads - 1) / threads;
    for (size_t s = 0; s < len; s += chunk) ts.emplace_back(f, s, std::min(len, s + chunk));
    for (auto& t : ts) t.join();
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <file of n x 32 B> [threads]\n", argv[0]);
        return 2;
    }
    const int threads = argc > 2 ? std::atoi(argv[2]) : 16;
    std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
    const size_t n = size_t(f.tellg()) / 32;
    std::vector<uint8_t> bytes(n * 32);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(bytes.data()), std::streamsize(bytes.size()));
    if (!f || !n) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::vector<G1Affine> points(n);
    std::vector<size_t> bad(size_t(threads) + 1, 0);
    const auto c0 = std::chrono::steady_clock::now();
    parallelize(n, threads, [&](size_t s, size_t t) {
        size_t b = 0;
        for (size_t i = s; i < t; i++) b += !serde::g1_from_bytes_host(&bytes[32 * i], points[i]);
        bad[s / ((n + threads - 1) / threads)] = b;
    });
    const auto c1 = std::chrono::steady_clock::now();
    size_t invalid = 0;
    for (size_t b : bad) invalid += b;
    uint64_t check = 0;
    for (size_t i = 0; i < n; i += std::max<size_t>(1, n / 64)) check ^= points[i].y[0];
    std::printf("{\"n\": %zu, \"threads\": %d, \"g1_decompress_host_ms\": %.1f, \"invalid\": %zu, \"check\": \"%016llx\"}\n", n, threads,
                std::chrono::duration<double, std::milli>(c1 - c0).count(), invalid, (unsigned long long)check);
    return 0;
}
