#!/usr/bin/python3
"""Key generation columns (csrc/keygen.hip) in the evalh-bench shape: 9 permutation columns, 4 fixed columns with 1 % Rational cells,
blinding_factors 5, the mapping the identity with a random tenth of the cells joined into cycles (numpy code equivalent to `copy`).
Per k, median of --reps runs after --warmup:
  sigma_call_ms       h2hip_permutation_keygen_bn254_device with only `permutations`: the whole call (kg_tables_kernel, kg_sigma_kernel,
                      the flag copy and its synchronisation), HIP events.  The sigma kernel alone is a row of the kernel trace;
  ifft_ms             h2hip_ifft_bn254_fr_batch_device of the same columns, in the same process: the yardstick the issue sets;
  perm_key_device_ms  all three forms, device-resident;
  perm_key_host_ms    h2hip_permutation_keygen_bn254 from a host mapping to host columns (wall clock; PCIe bytes stated);
  keygen_columns_ms   the whole Python composition keygen_columns (fixed columns, permutation key, l columns, both commitment batches).
and the sigma kernel's traffic floor, 40 bytes per cell at 6.3 TB/s.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python3 tools/keygen_bench.py --k K --no-host` in a process of its own, one k per run so that the
averages are per size.  --out NAME writes NAME.json and NAME.txt (one JSON line per k).

  python3 tools/keygen_bench.py [--k 17 20 22] [--reps 7] [--out profiles/keygen_bench]     (run on the GPU box)
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
from __graft_entry__ import load_pkg  # noqa: E402

M, FIXED, B, J = 9, 4, 5, 4
HBM_TBPS = 6.3  # achievable streaming rate (MI355X microarchitecture guide)


def make_mapping(k, seed):
    """identity, then a tenth of the cells joined into cycles of 2..5 cells: each cycle is a rotation of its cells' images, what a chain
    of `copy` calls over distinct singletons leaves"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    flat = np.arange(M * n, dtype=np.int64)
    picked = rng.choice(M * n, size=(M * n // 10) // 5 * 5, replace=False)
    for length in (2, 3, 5):
        part, picked = picked[: len(picked) // 3 // length * length], picked[len(picked) // 3 // length * length:]
        groups = part.reshape(-1, length)
        flat[groups] = np.roll(groups, -1, axis=1)
    flat = flat.reshape(M, n)
    return np.stack([flat // n, flat % n], axis=-1).astype(np.uint32)


def timed_events(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), [round(x, 4) for x in ms]


def timed_wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


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
    results = []
    for k in args.k:
        n = 1 << k
        dom = h2.EvaluationDomain.new(J, k)
        ext = dom.extended_len()
        mp = make_mapping(k, k)
        dmap = [torch.from_numpy(mp[j].view(np.int32).copy()).cuda() for j in range(M)]
        mk = lambda rows: [torch.empty((rows, 4), dtype=torch.int64, device="cuda") for _ in range(M)]  # noqa: E731
        dperm, dpoly, dcoset = mk(n), mk(n), mk(ext)
        row = {"k": k, "extended_k": dom.extended_k, "permutation_columns": M, "fixed_columns": FIXED, "blinding_factors": B,
               "joined_cells": int(np.count_nonzero((mp[:, :, 0] != np.arange(M)[:, None]) | (mp[:, :, 1] != np.arange(n)[None, :])))}
        row["sigma_call_ms"], row["sigma_call_ms_all"] = timed_events(torch, lambda: h2.permutation_keygen_device(dom, dmap, dperm), args.warmup,
                                                                      args.reps)
        row["ifft_ms"], _ = timed_events(torch, lambda: h2.ifft_batch_device(dpoly, dom.omega_inv, k, dom.ifft_divisor), args.warmup, args.reps)
        row["perm_key_device_ms"], _ = timed_events(torch, lambda: h2.permutation_keygen_device(dom, dmap, dperm, dpoly, dcoset), args.warmup,
                                                    args.reps)
        cells = M * n
        row["sigma_floor_ms"] = cells * 40 / (HBM_TBPS * 1e12) * 1e3
        del dperm, dpoly, dcoset, dmap
        torch.cuda.empty_cache()
        if not args.no_host:
            row["pcie_up_bytes"] = cells * 8
            row["pcie_down_bytes"] = M * (2 * n + ext) * 32
            row["perm_key_host_ms"] = timed_wall(lambda: h2.permutation_keygen(dom, mp), 1, max(3, args.reps // 2))
            rng = np.random.default_rng(k + 1)
            fixed = []
            for _ in range(FIXED):
                col = rng.integers(0, 1 << 61, size=(n, 4), dtype=np.uint64)
                rows_ = np.sort(rng.choice(n, size=max(1, n // 100), replace=False)).astype(np.uint32)
                den = rng.integers(1, 1 << 61, size=(len(rows_), 4), dtype=np.uint64)
                fixed.append((col, rows_, den))
            params = h2.ParamsKZG.setup(k, 0x5EED + k)
            row["keygen_columns_ms"] = timed_wall(lambda: h2.keygen_columns(params, dom, fixed, mp, B), 1, max(3, args.reps // 2))
            params.close()
        print(json.dumps(row), flush=True)
        results.append(row)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump(results, f, indent=1)
        with open(args.out + ".txt", "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in results))


if __name__ == "__main__":
    main()
