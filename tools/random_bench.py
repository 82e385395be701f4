#!/usr/bin/python3
"""The random-column kernels (csrc/random.hip) at 2^17 / 2^20 / 2^22 elements, the sizes of vanishing::Argument::commit's polynomial:
  (a) the device form (h2hip_fr_random_bn254_device): time per call by HIP events over a window of back-to-back calls, elements per
      second, and the vector instructions per second that is (the kernel's VALU count from its ISA, below) beside the chip's issue
      ceiling -- the kernel computes ~1400 instructions per 32 bytes written, so that is its bound, not HBM; the time HBM would need
      to take the output is printed beside it;
  (b) the library's own per-element loop on ONE host thread over the same n (the host form with its threshold lifted).  This is a
      STAND-IN for the reference's serial loop (plonk/vanishing/prover.rs:53-55) handed a user-space ChaCha20: no Rust toolchain
      exists here.  With the reference's usual OsRng every next_u64 is a system call and the loop is slower than this;
  (c) the upload of the 32 * 2^k bytes the resident form removes: a pageable host array to HBM, measured here;
  (d) vanishing_commit (draw in HBM + MSM over the pinned g) against host loop + upload + the same MSM;
and, at small n, the host forms' two paths against each other: where the device path (launch, download, synchronise) starts to win
is the default of HALO2_HIP_RANDOM_MIN_N.

  python tools/random_bench.py [--log-n 17 20 22] [--reps 7] [--out profiles/random_bench.json]     (run on the GPU box)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402

# VALU instructions of one lane of fr_random_kernel / fr_from_wide_kernel, counted in the gfx950 ISA (hipcc --save-temps): the block's
# 320 adds, 320 xors and 320 rotates (one v_alignbit_b32 each) + 16 output adds, and the reduction's 243 multiply-adds with its
# slicing, packing and conditional subtraction
VALU_PER_ELEM = {"fr_random": 1371, "fr_from_wide": 404}
# issue ceiling: 256 CUs x 4 SIMDs, one wave64 VALU instruction per 4 cycles at 2.4 GHz (tools/instr_rate.hip measures 4.3-5.5 cycles
# for the instructions used here, so the reachable ceiling is lower)
VALU_LANE_OPS_PEAK = 256 * 4 * 64 * 2.4e9 / 4
HBM_WRITE_BPS = 6.0e12
SEED = bytes(range(32))
SIZE_MAX = (1 << 64) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[17, 20, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="back-to-back calls per timed window are sized to last about this long")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    h2 = load_pkg()
    h2.init(0)
    L = h2.lib()

    def min_n(v):
        assert L.h2hip_debug_set_random_min_n(ctypes.c_size_t(v)) == 0

    def window(call, inner, reps=args.reps):
        """median per-call ms over `reps` windows of `inner` back-to-back calls, HIP events around each window"""
        ts = []
        for r in range(1 + reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            torch.cuda.synchronize()
            if r:
                ts.append(e0.elapsed_time(e1) / inner)
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "calls_per_window": inner}

    def host_clock(call, reps=3, warmup=1):
        """a host clock around work that ends synchronised"""
        ts = []
        for r in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    results = {"sizes": [], "threshold": []}
    for k in args.log_n:
        n = 1 << k
        rec = {"k": k, "n": n}
        d_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        call = lambda: h2.fr_random_device(SEED, n, out=d_out)
        once = window(call, 3, reps=2)["median_ms"]
        dev = window(call, max(3, int(args.window_ms / max(once, 1e-3))))
        rate = n / (dev["median_ms"] * 1e-3)
        dev.update(elements_per_s=rate, valu_per_element=VALU_PER_ELEM["fr_random"], valu_lane_ops_per_s=rate * VALU_PER_ELEM["fr_random"],
                   share_of_issue_ceiling=rate * VALU_PER_ELEM["fr_random"] / VALU_LANE_OPS_PEAK,
                   hbm_write_floor_ms=n * 32 / HBM_WRITE_BPS * 1e3, time_over_hbm_write_floor=dev["median_ms"] * 1e-3 / (n * 32 / HBM_WRITE_BPS))
        rec["a_device_form"] = dev
        d_wide = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device="cuda")
        wide = window(lambda: h2.fr_from_bytes_wide_device(d_wide, d_out, n), max(3, int(args.window_ms / max(once, 1e-3))))
        wide.update(elements_per_s=n / (wide["median_ms"] * 1e-3), hbm_traffic_floor_ms=n * 96 / HBM_WRITE_BPS * 1e3)
        rec["a2_from_bytes_wide_device"] = wide
        del d_wide

        min_n(SIZE_MAX)   # (b): the calling thread's loop at any n
        host = host_clock(lambda: h2.fr_random(SEED, n), reps=3 if k <= 20 else 2, warmup=1)
        host.update(ns_per_element=host["median_ms"] * 1e6 / n, threads=1,
                    note="stand-in for the reference's serial loop with a user-space ChaCha20; OsRng would be slower")
        rec["b_host_loop_one_thread"] = host
        min_n(0)

        h_poly = h2.fr_random(SEED, n)   # pageable numpy memory, as a Vec<Fr> is
        rec["c_upload_pageable"] = host_clock(lambda: torch.from_numpy(h_poly.view(np.int64)).cuda(), reps=5)
        rec["c_upload_pageable"]["gb_per_s"] = n * 32 / (rec["c_upload_pageable"]["median_ms"] * 1e-3) / 1e9

        params = h2.ParamsKZG.setup(k, 0x1234567 + k)
        dom = h2.EvaluationDomain.new(3, k)
        rng = h2.FrRng(SEED)
        h2.vanishing_commit(params, dom, rng)   # uploads and pins the resident g
        rec["d_vanishing_commit_resident"] = host_clock(lambda: h2.vanishing_commit(params, dom, rng), reps=5)
        rec["d_upload_plus_commit"] = host_clock(lambda: params.commit_device(torch.from_numpy(h_poly.view(np.int64)).cuda(), n), reps=5)
        d_poly = torch.from_numpy(h_poly.view(np.int64)).cuda()
        rec["d_commit_alone"] = host_clock(lambda: params.commit_device(d_poly, n), reps=5)
        base = host["median_ms"] + rec["d_upload_plus_commit"]["median_ms"]
        rec["d_host_loop_plus_upload_plus_commit_ms"] = base
        rec["d_speedup"] = base / rec["d_vanishing_commit_resident"]["median_ms"]
        params.close()
        del d_poly, d_out, params
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        results["sizes"].append(rec)

    # the host forms' two paths at small n
    for n in (16, 64, 128, 256, 512, 1024, 2048, 4096, 16384):
        row = {"n": n}
        for name, v in (("host_loop", SIZE_MAX), ("device_path", 1)):
            min_n(v)
            h2.fr_random(SEED, n)
            ts = []
            for _ in range(30):
                t0 = time.perf_counter()
                h2.fr_random(SEED, n)
                ts.append((time.perf_counter() - t0) * 1e6)
            row[name + "_us"] = statistics.median(ts)
        min_n(0)
        print(json.dumps(row), flush=True)
        results["threshold"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
