#!/usr/bin/python3
"""The witness check (h2hip_check_gates_bn254 / h2hip_check_permutation_bn254 / h2hip_check_lookups_bn254) on the evalh-bench system:
its 24 gate polynomials over 12 advice and 10 fixed columns, 9 permutation columns, 2 lookups, blinding_factors 5, device-resident.
Columns come from the engine's on-device generator, so nearly every row fails every constraint: the first kernel and the count / scan do
the work of a satisfied witness, and the compaction stops at max_rows either way.  Per k, min and median of --reps calls (HIP events around
a call that synchronises its stream itself) of each check, and beside the gate check `lookup_compress_device` over the SAME gate graphs:
what has to run without the check to obtain the same verdict, before 32 bytes per (polynomial, row) are downloaded and scanned.  The
permutation and lookup checks are recorded beside the bytes they move (64 B, and about 32 B (1 + log2(u) / 8) per row) and the bandwidth
that implies.

  python tools/check_bench.py [--k 17 20] [--reps 7] [--out profiles/check_bench.json]     (run on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402
import evalh_bench  # noqa: E402

B = 5
MAX_ROWS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[17, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    h2 = load_pkg()
    h2.init(0)
    ev = __import__("halo2_pse_amd.evaluation", fromlist=["x"])
    sys_args = evalh_bench.default_args()
    gates, lookups = evalh_bench.system_expressions(sys_args, np.random.default_rng(1))
    gate_graphs = [ev.flatten_graph(g) for g in ev.gate_check_graphs(gates)]
    lookup_graphs = []
    for inp, tab in lookups:
        gi, gt = ev.lookup_compress_graphs(inp, tab)
        lookup_graphs += [ev.flatten_graph(gi), ev.flatten_graph(gt)]
    theta = h2.fr_from_int(0x7E7A)

    def timed(call):
        ts = []
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "all_ms": ts}

    results = []
    for k in args.k:
        n, u = 1 << k, (1 << k) - B - 1
        fixed = [h2.gen_scalars_device(0xC000 + i, n) for i in range(sys_args.fixed)]
        advice = [h2.gen_scalars_device(0xC100 + i, n) for i in range(sys_args.advice)]
        perm_cols = [advice[j % sys_args.advice] for j in range(sys_args.perm)]
        cells = np.random.default_rng(k).permutation(sys_args.perm * n)
        mapping = np.stack([cells // n, cells % n], axis=-1).astype(np.uint32).reshape(sys_args.perm, n, 2)
        d_map = [torch.from_numpy(mapping[j].view(np.int32).copy()).cuda() for j in range(sys_args.perm)]
        comp = [torch.empty_like(fixed[0]) for _ in lookup_graphs]
        h2.lookup_compress_device(k, lookup_graphs, theta, comp, fixed, advice)
        gate_out = [torch.empty_like(fixed[0]) for _ in gate_graphs]
        torch.cuda.synchronize()
        rec = {"k": k, "gate_polynomials": len(gate_graphs), "permutation_columns": sys_args.perm, "lookups": len(lookups), "blinding_factors": B,
               "max_rows": MAX_ROWS}
        rec["check_gates"] = timed(lambda: h2.check_gates_device(k, gate_graphs, fixed, advice, max_rows=MAX_ROWS))
        rec["lookup_compress_same_graphs"] = timed(lambda: (h2.lookup_compress_device(k, gate_graphs, theta, gate_out, fixed, advice),
                                                            torch.cuda.current_stream().synchronize()))
        rec["lookup_compress_same_graphs"]["bytes_written"] = len(gate_graphs) * n * 32
        rec["check_gates_over_compress"] = rec["check_gates"]["median_ms"] / rec["lookup_compress_same_graphs"]["median_ms"]
        rec["check_permutation"] = timed(lambda: h2.check_permutation_device(k, perm_cols, d_map, MAX_ROWS))
        pb = sys_args.perm * n * 64
        rec["check_permutation"].update(bytes=pb, gbps=pb / (rec["check_permutation"]["median_ms"] * 1e6))
        rec["check_lookups"] = timed(lambda: h2.check_lookups_device(k, comp[0::2], comp[1::2], B, MAX_ROWS))
        lb = int(len(lookups) * n * 32 * (1 + math.log2(u) / 8))
        rec["check_lookups"].update(bytes=lb, gbps=lb / (rec["check_lookups"]["median_ms"] * 1e6))
        counts = h2.check_gates_device(k, gate_graphs, fixed, advice, max_rows=MAX_ROWS)[0]
        rec["gate_failing_rows_of_polynomial_0"] = int(counts[0])
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del fixed, advice, perm_cols, d_map, comp, gate_out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
