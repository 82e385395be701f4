#!/usr/bin/python3
"""The serialisation kernels (csrc/serde.hip) at n = 2^20 and 2^22 elements: every _device call timed with HIP events (the fallible
ones synchronise their stream themselves to deliver the two result words, so their times include that round trip), the host-pointer
forms beside them (upload, kernel, download: PCIe included), and for the decompression the multiplications per second it sustains
against the 179 G mul/s of the explicit-mad multiplier (bench.py, tools/mul_rate.hip) and the time the C++ mirror's host decompression
(fe_pow, tools/serde_host.cpp) needs for the SAME points on 16 threads, measured in the same run.
Points come from the engine's on-device generator; odd indices carry the other sign bit.

  g++ -O3 -std=c++17 -pthread -o tools/serde_host tools/serde_host.cpp -Lhalo2-pse_amd -lhalo2hip -Wl,-rpath,'$ORIGIN/../halo2-pse_amd' -Wl,-rpath,/opt/rocm/lib
  python tools/serde_bench.py [--log-n 20 22] [--reps 7] [--out profiles/serde_bench.json]     (run on the GPU box)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402

# Fq multiplications of one decompressed point (csrc/serde_elem.h, fieldu.h fu_sqrt): x to Montgomery form 1, x^3 2, fu_sqrt 315
# (251 squarings, 1 product to bring t in range, 7 for the odd powers, 56 window products), y^2 1, the three reductions to canonical form 3
MULS_PER_POINT = 1 + 2 + 315 + 1 + 3
MUL_RATE_PEAK = 179e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    h2 = load_pkg()
    h2.init(0)
    host_exe = os.path.join(ROOT, "tools", "serde_host")
    if not os.path.exists(host_exe):
        raise SystemExit("tools/serde_host is not built (see this file's header)")

    def timed(call, reps=args.reps, warmup=args.warmup):
        ts = []
        for r in range(warmup + reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append(e0.elapsed_time(e1))
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    def timed_host(call, reps=3):
        ts = []
        for r in range(1 + reps):
            t0 = time.perf_counter()
            call()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    results = []
    for log_n in args.log_n:
        n = 1 << log_n
        d_pts = h2.gen_points_device(0x5E2DE, n)
        d_bytes = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        h2.g1_to_bytes_device(d_pts, d_bytes, n)
        d_bytes[1::2, 31] ^= 0x80
        d_out = torch.empty_like(d_pts)
        d_fr = h2.gen_scalars_device(0x5E2DF, n)
        d_repr = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rec = {"n": n, "device": {}, "host_form": {}}
        dev = rec["device"]
        dev["g1_decompress"] = timed(lambda: h2.g1_from_bytes_device(d_bytes, d_out, n))
        dev["g1_compress"] = timed(lambda: h2.g1_to_bytes_device(d_out, d_repr, n))
        dev["g1_validate"] = timed(lambda: h2.g1_validate_device(d_out, n))
        dev["fr_to_repr"] = timed(lambda: h2.fr_to_repr_device(d_fr, d_repr, n))
        dev["fr_from_repr"] = timed(lambda: h2.fr_from_repr_device(d_repr, d_repr, n))
        h2.profile_enable(1)
        h2.profile_reset()
        h2.g1_from_bytes_device(d_bytes, d_out, n)
        kernel_ms = h2.profile_get("g1_decompress")[0]
        h2.profile_enable(0)
        dev["g1_decompress"]["kernels_ms"] = kernel_ms   # the decompression and the two counting kernels, without the result's round trip
        rate = n * MULS_PER_POINT / (kernel_ms * 1e-3)
        dev["g1_decompress"].update(muls_per_point=MULS_PER_POINT, gmul_per_s=rate / 1e9, share_of_179_gmul_per_s=rate / MUL_RATE_PEAK)
        h_bytes, h_pts, h_fr = d_bytes.cpu().numpy(), h2.to_numpy_u64(d_out), h2.to_numpy_u64(d_fr)
        hf = rec["host_form"]
        hf["g1_decompress"] = timed_host(lambda: h2.g1_from_bytes(h_bytes))
        hf["g1_compress"] = timed_host(lambda: h2.g1_to_bytes(h_pts))
        hf["g1_validate"] = timed_host(lambda: h2.g1_validate(h_pts))
        h_repr = h2.fr_to_repr(h_fr)
        hf["fr_to_repr"] = timed_host(lambda: h2.fr_to_repr(h_fr))
        hf["fr_from_repr"] = timed_host(lambda: h2.fr_from_repr(h_repr))
        with tempfile.NamedTemporaryFile(suffix=".g1") as f:
            f.write(h_bytes.tobytes())
            f.flush()
            host = json.loads(subprocess.run([host_exe, f.name, str(args.host_threads)], check=True, capture_output=True, text=True).stdout)
        assert host["n"] == n and host["invalid"] == 0
        rec["mirror_host_fe_pow"] = host
        rec["host_over_device_decompress"] = host["g1_decompress_host_ms"] / dev["g1_decompress"]["median_ms"]
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del d_pts, d_bytes, d_out, d_fr, d_repr
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
