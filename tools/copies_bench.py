#!/usr/bin/python3
"""The permutation mapping from copy constraints (h2hip_permutation_mapping[_device]) beside what it replaces and what consumes it.
Per shape -- k, m = 9 permutation columns, C = m 2^k / 2 random copies, plus one giant component (C = 2 m 2^k) at --giant-k -- medians of
--reps runs (at least 5) of:
  the _device form, copies and mapping resident (HIP events around a call that synchronises its stream itself), and in a profiled
  run its three parts: components (init, hooking, keys), sort, scatter (identity fill and successors);
  the host form (wall clock: upload of the copies, the same kernels, download of the mapping);
  the mirror's serial Assembly::copy loop on one host thread for the same copies (tools/copies_host, built on first use);
  h2hip_permutation_keygen_bn254_device for the same shape, all three forms, from a resident mapping;
  permutation_keygen_from_copies against permutation_keygen over a host mapping (wall clock), with the bytes each moves over PCIe --
  for the sigma columns alone (build_vk's case) and, up to --full-k, for all three forms.

  python tools/copies_bench.py [--k 17 20 22] [--giant-k 20] [--reps 5] [--out profiles/copies_bench.json]     (run on the GPU box)
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

M = 9
PARTS = ("copies_components", "copies_sort", "copies_scatter")


def host_loop(k, copies, reps):
    exe = os.path.join(ROOT, "tools", "copies_host")
    if not os.path.exists(exe):
        libdir = os.path.join(ROOT, "halo2-pse_amd")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "copies_host.cpp"), "-L" + libdir, "-lhalo2hip",
                               "-Wl,-rpath,$ORIGIN/../halo2-pse_amd", "-Wl,-rpath,/opt/rocm/lib"])
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        copies.tofile(f.name)
        out = subprocess.run([exe, str(k), str(M), f.name, str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[17, 20, 22])
    ap.add_argument("--giant-k", type=int, default=20)
    ap.add_argument("--full-k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    h2 = load_pkg()
    h2.init(0)

    def stats(ts):
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    def timed(call):  # HIP events
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
        return stats(ts)

    def walled(call):  # wall clock, for calls over host memory
        ts = []
        for r in range(1 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if r >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)

    shapes = [(k, "half", M * (1 << k) // 2) for k in args.k] + ([(args.giant_k, "giant", 2 * M * (1 << args.giant_k))] if args.giant_k else [])
    results = []
    for k, kind, C in shapes:
        n = 1 << k
        rng = np.random.default_rng(k * 7 + len(kind))
        copies = np.zeros((C, 4), dtype=np.uint32)
        copies[:, 0::2] = rng.integers(0, M, size=(C, 2), dtype=np.uint32)
        copies[:, 1::2] = rng.integers(0, n, size=(C, 2), dtype=np.uint32)
        dom = h2.EvaluationDomain.new(4, k)
        d_cp = torch.from_numpy(copies.view(np.int32)).cuda()
        d_map = [torch.empty((n, 2), dtype=torch.int32, device="cuda") for _ in range(M)]
        rec = {"k": k, "n_columns": M, "copies": kind, "n_copies": C, "sort_plan": h2.copies_sort_plan(C)}
        rec["mapping_device"] = timed(lambda: h2.permutation_mapping_device(k, M, d_cp, d_map))
        h2.profile_enable(1)
        per = {p: [] for p in PARTS}
        for _ in range(args.reps):
            h2.profile_reset()
            h2.permutation_mapping_device(k, M, d_cp, d_map)
            torch.cuda.synchronize()
            for p in PARTS:
                per[p].append(h2.profile_get(p)[0])
        h2.profile_enable(0)
        rec["mapping_device_parts"] = {p: stats(per[p]) for p in PARTS}
        rec["mapping_host_form"] = walled(lambda: h2.permutation_mapping(k, M, copies))
        rec["mapping_host_form"]["pcie_bytes"] = {"up": 16 * C, "down": 8 * M * n}
        rec["assembly_copy_one_thread"] = host_loop(k, copies, args.reps)
        mapping = np.stack([t.cpu().numpy().view(np.uint32) for t in d_map])
        moved = int((mapping.reshape(-1, 2) != h2.permutation_mapping(k, M, []).reshape(-1, 2)).any(axis=1).sum())
        rec["cells_in_cycles"] = moved
        d_out = [[torch.empty((rows, 4), dtype=torch.int64, device="cuda") for _ in range(M)] for rows in (n, n, dom.extended_len())]
        rec["keygen_device_three_forms"] = timed(lambda: h2.permutation_keygen_device(dom, d_map, *d_out))
        del d_out
        torch.cuda.empty_cache()
        col = 32 * M
        for name, want in (("sigma_only", ("permutations",)),) + ((("three_forms", ("permutations", "polys", "cosets")),) if k <= args.full_k else ()):
            down = col * sum({"permutations": n, "polys": n, "cosets": dom.extended_len()}[w] for w in want)
            a = walled(lambda: h2.permutation_keygen_from_copies(dom, M, copies, want=want))
            b = walled(lambda: h2.permutation_keygen(dom, mapping, want=want))
            a["pcie_bytes"] = {"up": 16 * C, "down": down}
            b["pcie_bytes"] = {"up": 8 * M * n, "down": down}
            rec["keygen_from_copies_" + name] = a
            rec["keygen_from_host_mapping_" + name] = b
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del d_cp, d_map
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
