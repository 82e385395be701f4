#!/usr/bin/python3
"""commit_permuted's compression and permutation (h2hip_lookup_compress_bn254 / h2hip_lookup_permute_bn254) in the evalh-bench style:
a tuple lookup (input [A0, A1], table [F0, F1], the advice rows copied from random table rows: repeats, leftovers, full-width keys) and a
range lookup (input [A2], table [F2], F2[i] = i mod 2^16: small keys), blinding_factors 5.  Per k: the device-resident calls (HIP events
around compress + permute, after a synchronisation), the host-pointer calls with and without the fixed columns pinned (wall clock around
blocking calls), median of --reps runs after --warmup, and the algorithmic bytes of one call pair.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/lookup_bench.py ...` in a process of its own.

  python tools/lookup_bench.py [--k 17 20 22] [--reps 7] [--out profiles/lookup_bench.json]     (run on the GPU box)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402
import lookup_util as lu  # noqa: E402

B = 5
LOOKUPS = [([("advice", 0, 0), ("advice", 1, 0)], [("fixed", 0, 0), ("fixed", 1, 0)]), ([("advice", 2, 0)], [("fixed", 2, 0)])]


def shape_bytes(k):
    """algorithmic HBM bytes of one compress + permute call pair: compression reads 6 columns and writes 4; the sort reads and writes
    every key once per pass (1 LDS block pass + k - 10 merge passes) over 4 columns; the permutation reads both sorted columns about
    twice, L once, and writes A', S' per lookup"""
    n = 1 << k
    passes = 1 + max(0, k - 10)
    return n * 32 * (6 + 4) + 4 * passes * n * 64 + 2 * n * (32 * 6 + 4 * 3 + 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[17, 20, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    h2 = load_pkg()
    h2.init(0)
    ev = __import__("halo2_pse_amd.evaluation", fromlist=["x"])
    graphs = []
    for inp, tab in LOOKUPS:
        gi, gt = ev.lookup_compress_graphs(inp, tab)
        graphs += [ev.flatten_graph(gi), ev.flatten_graph(gt)]
    theta = lu.to_mont([0x7E7A])[0]
    results = []
    for k in args.k:
        n, u = 1 << k, (1 << k) - B - 1
        rng = np.random.default_rng(k)
        f0 = h2.to_numpy_u64(h2.gen_scalars_device(0xA000 + k, n)).copy()
        f1 = h2.to_numpy_u64(h2.gen_scalars_device(0xA100 + k, n)).copy()
        f2 = lu.to_mont([i % (1 << 16) for i in range(n)])
        rows = rng.integers(0, u, size=n)
        a0, a1 = f0[rows], f1[rows]
        a2 = f2[rng.integers(0, min(u, 1 << 16), size=n)]
        fixed, advice = [f0, f1, f2], [np.ascontiguousarray(a0), np.ascontiguousarray(a1), np.ascontiguousarray(a2)]
        blind = np.zeros((2 * 2 * (B + 1), 4), dtype=np.uint64)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()  # noqa: E731
        df, da = [dev(c) for c in fixed], [dev(c) for c in advice]
        dcomp = [torch.empty_like(df[0]) for _ in range(4)]
        dpa, dps = [torch.empty_like(df[0]) for _ in range(2)], [torch.empty_like(df[0]) for _ in range(2)]

        def device_once():
            h2.lookup_compress_device(k, graphs, theta, dcomp, df, da)
            h2.lookup_permute_device(k, dcomp[0::2], dcomp[1::2], blind, B, dpa, dps)

        times = []
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_once()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times.append(e0.elapsed_time(e1))
        rec = {"k": k, "lookups": 2, "blinding_factors": B, "device_ms": statistics.median(times), "device_ms_all": times,
               "algorithmic_bytes": shape_bytes(k)}
        rec["device_gbps"] = rec["algorithmic_bytes"] / (rec["device_ms"] * 1e6)
        # the host forms give what the device forms gave
        comp = h2.lookup_compress(k, graphs, theta, fixed, advice)
        pa, ps = h2.lookup_permute(k, comp[0::2], comp[1::2], blind, B)
        assert all(np.array_equal(pa[j], h2.to_numpy_u64(dpa[j])) and np.array_equal(ps[j], h2.to_numpy_u64(dps[j])) for j in range(2))
        if not args.no_host:
            for label, pin in (("host_unpinned_ms", False), ("host_pinned_ms", True)):
                if pin:
                    h2.columns_pin(fixed)
                ts = []
                for r in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    comp = h2.lookup_compress(k, graphs, theta, fixed, advice)
                    h2.lookup_permute(k, comp[0::2], comp[1::2], blind, B)
                    if r >= args.warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
                if pin:
                    h2.columns_unpin(fixed)
                rec[label] = statistics.median(ts)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del df, da, dcomp, dpa, dps
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
