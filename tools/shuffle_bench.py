#!/usr/bin/python3
"""The shuffle argument beside the lookup argument on the evalh-bench system (24 gate polynomials over 12 advice and 10 fixed columns, 9
permutation columns, 2 lookups) with --shuffles shuffles added, device-resident, at k (extended_k = k + 2).  Three pairs, each from the
same process and the same run, medians of --reps:
  evaluate_h   the shuffle stage's time per shuffle (stage "evalh_shuffles": the kernel generated per shuffle or the interpreter's
               evalh_shuffle_kernel, as --codegen says; its coset transform not included) beside the lookup stage's time per lookup (stage
               "evalh_lookups": generated kernels, the cosets of the first group are formed before the stage)
  products     shuffle_products_device beside lookup_products_device at equal count
  check        check_shuffles_device beside check_lookups_device at equal count
The clocks the card reports go into the record.

--codegen is the mode of h2hip_debug_set_evalh_codegen for the evaluate_h part (2: every kernel of the default set generated and compiled
inline; 2 + 32: the shuffles on the interpreter; 2 + 64: the shuffles generated), --exprs the expressions a side, --stage-only leaves the
products and the check out.  The first call's wall time (the inline compilations) and the launches the stage counters saw are recorded.

  python tools/shuffle_bench.py [--k 18] [--shuffles 2] [--exprs 2] [--codegen 2] [--reps 5] [--stage-only] [--out profiles/shuffle_bench.json]     (run on the GPU box)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402
import evalh_bench  # noqa: E402

B = 5
R_MOD = evalh_bench.R_MOD


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [line.strip() for line in out.splitlines() if "clk" in line.lower() and "(" in line]
    except Exception as e:  # noqa: BLE001  (the tool is absent or slow: the record says so)
        return ["unavailable: %r" % (e,)]


def stage_counters(L):
    """launches of a generated kernel and of the interpreter per stage, or None with a library from before the stage kernels"""
    if not hasattr(L, "h2hip_debug_evalh_codegen_stage_stats"):
        return None
    out = (ctypes.c_uint64 * 9)()
    L.h2hip_debug_evalh_codegen_stage_stats(out)
    return {name: [int(out[2 * i]), int(out[2 * i + 1])] for i, name in enumerate(("gates", "lookups", "shuffles", "mvlookups"))}


def side(sa, j, m, shift):
    """m expressions over the bench system's columns: every second one a product with a fixed column, every third one rotated, so that
    the expressions of a side share selectors and columns as a circuit's do"""
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    out = []
    for t in range(m):
        a = A((j + shift + t) % sa.advice, 1 if t % 3 == 2 else 0)
        out.append(('prod', a, F((j + t // 2) % sa.fixed)) if t % 2 else a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--shuffles", type=int, default=2)
    ap.add_argument("--exprs", type=int, default=2, help="expressions a side")
    ap.add_argument("--codegen", type=int, default=2, help="h2hip_debug_set_evalh_codegen mode for the evaluate_h part")
    ap.add_argument("--stage-only", action="store_true", help="the evaluate_h part alone")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import importlib
    import torch
    h2 = load_pkg()
    h2.init(0)
    ev = importlib.import_module("halo2_pse_amd.evaluation")
    from oracle import oracle as orc
    orc.build()
    L = h2.lib()
    sa = evalh_bench.default_args()
    gates, lookups = evalh_bench.system_expressions(sa, np.random.default_rng(1))
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    if args.exprs == 2:  # as wide as the bench system's lookups: two expressions a side, one of them a product with a fixed column, one rotated
        shuffles = [([A(j % sa.advice), ('prod', A((j + 1) % sa.advice), F(j % sa.fixed))], [A((j + 2) % sa.advice), A((j + 3) % sa.advice, 1)])
                    for j in range(args.shuffles)]
    else:
        shuffles = [(side(sa, j, args.exprs, 0), side(sa, j, args.exprs, 5)) for j in range(args.shuffles)]
    evaluator = ev.Evaluator.new(gates, lookups, shuffles)
    k, ek = args.k, args.k + 2
    n, size = 1 << k, 1 << ek
    d, _ = orc.domain_new(4, k)
    gen = lambda m, s: h2.gen_scalars_device(1000 + s, m)  # noqa: E731
    fe1 = lambda s: orc.gen_scalars(s, 1)[0]  # noqa: E731
    chunk_len, n_sets = 2, -(-sa.perm // 2)
    cols = {"fixed_cosets": [gen(size, 10 + i) for i in range(sa.fixed)], "advice_polys": [gen(n, 100 + i) for i in range(sa.advice)],
            "perm_product_cosets": [gen(size, 200 + i) for i in range(n_sets)], "perm_cosets": [gen(size, 300 + i) for i in range(sa.perm)],
            "l0": gen(size, 1), "l_last": gen(size, 2), "l_active_row": gen(size, 3),
            "lookups": [[gen(n, 400 + 3 * i + t) for t in range(3)] for i in range(sa.lookups)],
            "shuffles": [gen(n, 500 + j) for j in range(args.shuffles)]}
    d_values = gen(size, 999)
    stub = np.zeros((1, 4), dtype=np.uint64)
    case = {"k": k, "extended_k": ek, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
            "zeta": orc.constant(orc.FR, 5), "delta": orc.fe_from_int(orc.FR, pow(7, 1 << 28, R_MOD)),
            "y": fe1(1), "beta": fe1(2), "gamma": fe1(3), "theta": fe1(4), "l0": stub, "l_last": stub, "l_active_row": stub,
            "fixed_cosets": [stub] * sa.fixed, "advice_polys": [stub] * sa.advice, "instance_polys": [], "challenges": np.zeros((0, 4), dtype=np.uint64),
            "perm_product_cosets": [stub] * n_sets, "perm_cosets": [stub] * sa.perm, "perm_column_kind": np.zeros(sa.perm, dtype=np.uint32),
            "perm_column_index": (np.arange(sa.perm) % sa.advice).astype(np.uint32), "chunk_len": chunk_len, "last_rotation": -(B + 1),
            "lookups": [(stub, stub, stub)] * sa.lookups, "shuffles": [stub] * args.shuffles}
    hd, hs = evaluator.describe(case), evaluator.describe_shuffles(case)
    keep = []

    def table(ts):
        arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        keep.append(arr)
        return ctypes.addressof(arr)

    dd = hd.desc
    dd.fixed_cosets, dd.advice_polys = table(cols["fixed_cosets"]), table(cols["advice_polys"])
    dd.perm_product_cosets, dd.perm_cosets = table(cols["perm_product_cosets"]), table(cols["perm_cosets"])
    dd.l0, dd.l_last, dd.l_active_row = cols["l0"].data_ptr(), cols["l_last"].data_ptr(), cols["l_active_row"].data_ptr()
    for t, name in enumerate(("lookup_product_polys", "lookup_permuted_input_polys", "lookup_permuted_table_polys")):
        setattr(dd, name, table([l[t] for l in cols["lookups"]]))
    hs.desc.product_polys = table(cols["shuffles"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = L.h2hip_evaluate_h_shuffles_bn254_device(hd.byref(), hs.byref(), ctypes.c_void_p(d_values.data_ptr()), stream)
        assert rc == 0, L.h2hip_last_error()

    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(args.codegen), ctypes.c_uint32(0))  # mode 2: the kernels generated and compiled inline
    t0 = time.time()
    call()
    torch.cuda.synchronize()
    rec = {"k": k, "extended_k": ek, "lookups": sa.lookups, "shuffles": args.shuffles, "exprs_per_side": args.exprs, "codegen": args.codegen,
           "first_call_s": time.time() - t0, "reps": args.reps, "clocks_before": clocks()}
    counters0 = stage_counters(L)
    per = {"evalh_lookups": [], "evalh_shuffles": [], "evalh_gates": [], "evalh_perm": [], "evalh_cosets": []}
    for _ in range(args.reps):
        h2.profile_enable(True)
        h2.profile_reset()
        call()
        torch.cuda.synchronize()
        h2.profile_enable(False)
        for name in per:
            per[name].append(h2.profile_get(name)[0])
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
    rec["stage_ms_median"] = {name: statistics.median(v) for name, v in per.items()}
    rec["ms_per_lookup"] = rec["stage_ms_median"]["evalh_lookups"] / max(1, sa.lookups)
    rec["ms_per_shuffle"] = rec["stage_ms_median"]["evalh_shuffles"] / max(1, args.shuffles)
    rec["ms_per_shuffle_runs"] = [v / max(1, args.shuffles) for v in per["evalh_shuffles"]]
    counters1 = stage_counters(L)
    if counters1:
        rec["stage_launches_generated_interpreted"] = {name: [b[0] - a[0], b[1] - a[1]] for (name, a), b in zip(counters0.items(), counters1.values())}
    if args.stage_only:
        rec["clocks_after"] = clocks()
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
        return

    def timed(fn):
        ts = []
        for r in range(2 + args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ts.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    count = args.shuffles
    col = [gen(n, 600 + i) for i in range(4 * count)]
    z = [torch.empty_like(col[0]) for _ in range(count)]
    beta, gamma = fe1(2), fe1(3)
    blinding = orc.gen_scalars(77, count * B)
    rec["lookup_products"] = timed(lambda: h2.lookup_products_device(k, beta, gamma, col[0:count], col[count:2 * count], col[2 * count:3 * count],
                                                                     col[3 * count:], blinding, B, z))
    rec["shuffle_products"] = timed(lambda: h2.shuffle_products_device(k, gamma, col[0:count], col[count:2 * count], blinding, B, z))
    rec["check_lookups"] = timed(lambda: h2.check_lookups_device(k, col[0:count], col[count:2 * count], B, 16))
    rec["check_shuffles"] = timed(lambda: h2.check_shuffles_device(k, col[0:count], col[count:2 * count], B, 16))
    rec["clocks_after"] = clocks()
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
