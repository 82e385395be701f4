#!/usr/bin/python3
"""The grand-product columns (h2hip_permutation_products_bn254 / h2hip_lookup_products_bn254) in the evalh-bench shape: 9 permutation
columns in sets of chunk_len 3, 2 lookups, blinding_factors 5.  Per k: the device-resident calls (HIP events around both calls, after a
synchronisation), the host-pointer calls with and without the key's columns pinned (wall clock around blocking calls), median of --reps
runs after --warmup; and the algorithmic bytes and Fr multiplications of the shape.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/product_bench.py ...` in a process of its own.

  python tools/product_bench.py [--k 17 20 22] [--reps 7] [--out profiles/products.json]     (run on the GPU box)
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
import product_util as pu  # noqa: E402

M, CHUNK, LOOKUPS, B = 9, 3, 2, 5


def shape_counts(k):
    """algorithmic Fr multiplications and bytes of HBM traffic of one call pair (product.hip's three passes)"""
    n = 1 << k
    muls = byts = 0
    for start in range(0, M, CHUNK):
        c = min(CHUNK, M - start)
        muls += n * ((c + 1) + (c - 1) + c + (c - 1) + 2 + 4)  # numerator, denominator, thread products, scans and final products
        byts += n * (2 * c * 32 + 64 + 192)                     # p_c, s_c read; e, d written; re-read and written by the apply pass
    muls += LOOKUPS * n * (2 + 2 + 4)
    byts += LOOKUPS * n * (4 * 32 + 64 + 192)
    return muls, byts


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
        omega, delta, beta, gamma = (pu.fe(v) for v in (pu.root_of_unity(k), 0x1D2E3F + k, 0xBE7A + k, 0x6A33A + k))
        cols = [h2.gen_scalars_device(0x9000 + j, n) for j in range(M)]
        perms = [h2.gen_scalars_device(0x9100 + j, n) for j in range(M)]
        look = [[h2.gen_scalars_device(0x9200 + 4 * j + q, n) for q in range(4)] for j in range(LOOKUPS)]
        zp = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(-(-M // CHUNK))]
        zl = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(LOOKUPS)]
        rng = np.random.default_rng(k)
        blind_p = rng.integers(0, 1 << 63, size=(len(zp) * B, 4), dtype=np.uint64)
        blind_l = rng.integers(0, 1 << 63, size=(LOOKUPS * B, 4), dtype=np.uint64)
        blind_p[:, 3] %= np.uint64(0x30644e72e131a029)  # below r
        blind_l[:, 3] %= np.uint64(0x30644e72e131a029)

        def device_call():
            h2.permutation_products_device(k, omega, delta, beta, gamma, cols, perms, CHUNK, blind_p, B, zp)
            h2.lookup_products_device(k, beta, gamma, [l[0] for l in look], [l[1] for l in look], [l[2] for l in look], [l[3] for l in look],
                                      blind_l, B, zl)

        for _ in range(args.warmup):
            device_call()
        torch.cuda.synchronize()
        dev_ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            device_call()
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        muls, byts = shape_counts(k)
        row = {"k": k, "columns": M, "chunk_len": CHUNK, "lookups": LOOKUPS, "blinding_factors": B, "fr_muls": muls, "bytes": byts,
               "device_ms_median": statistics.median(dev_ms), "device_ms_all": [round(x, 4) for x in dev_ms]}
        if not args.no_host:
            hc = [h2.to_numpy_u64(c).copy() for c in cols]
            hp = [h2.to_numpy_u64(c).copy() for c in perms]
            hl = [[h2.to_numpy_u64(c).copy() for c in l] for l in look]

            def host_call():
                h2.permutation_products(k, omega, delta, beta, gamma, hc, hp, CHUNK, blind_p, B)
                h2.lookup_products(k, beta, gamma, [l[0] for l in hl], [l[1] for l in hl], [l[2] for l in hl], [l[3] for l in hl], blind_l, B)

            for label in ("host_ms_median", "host_pinned_ms_median"):
                if label == "host_pinned_ms_median":
                    h2.columns_pin(hp)
                for _ in range(args.warmup):
                    host_call()
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    host_call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                row[label] = statistics.median(ts)
            h2.columns_unpin(hp)
        row["device_mul_rate_G_per_s"] = muls / (row["device_ms_median"] * 1e-3) / 1e9
        print(json.dumps(row), flush=True)
        results.append(row)
        del cols, perms, look, zp, zl
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
