#!/usr/bin/python3
"""The logUp (mv-lookup) argument beside the halo2 lookup path it replaces, device-resident, at k (extended_k = k + 2), with K = 1 and
K = 4 inputs per table.  Every pair comes from the same process and the same run, medians of --reps:
  multiplicities   mvlookup_multiplicities_device for uniform inputs and for all rows hitting one table value, beside
                   lookup_permute_device of the K (input, table) pairs the halo2 lookup needs for the same inputs
  sums             mvlookup_sums_device beside lookup_products_device of those K lookups
  evaluate_h       the stage's time per argument (stage "evalh_mvlookups": the kernel generated per argument or the interpreter's
                   evalh_mvlookup_kernel, as --codegen says; its coset transforms not included) on the evalh-bench system (24 gate polynomials over 12 advice and 10 fixed columns, 9 permutation
                   columns, 2 lookups) beside K times the lookup stage's time per lookup (stage "evalh_lookups": generated kernels)
The clocks the card reports go into the record.

--codegen is the mode of h2hip_debug_set_evalh_codegen for the evaluate_h part (2 + 32: the mv-lookups on the interpreter; 2 + 64: generated),
--exprs the expressions a tuple, --inputs the values of K, --stage-only leaves the multiplicities and the sums out.  The first call's wall
time (the inline compilations) and the launches the stage counters saw are recorded.

  python tools/mvlookup_bench.py [--k 18] [--inputs 1,4] [--exprs 2] [--codegen 2] [--reps 5] [--stage-only] [--out profiles/mvlookup_bench.json]     (run on the GPU box)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402
import evalh_bench  # noqa: E402
from shuffle_bench import clocks, side, stage_counters  # noqa: E402

B = 5
R_MOD = evalh_bench.R_MOD
ARGS = 2  # mv-lookup arguments in the evaluate_h system


def evalh_stage(h2, ev, orc, torch, k, K, reps, exprs=2, codegen=2):
    """stage medians of evaluate_h on the evalh-bench system with ARGS mv-lookup arguments of K input pairs each"""
    L = h2.lib()
    sa = evalh_bench.default_args()
    gates, lookups = evalh_bench.system_expressions(sa, np.random.default_rng(1))
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    if exprs == 2:  # as wide as the bench system's lookups: two expressions a tuple, one of them a product with a fixed column
        mv = [([[A((j + 2 * t) % sa.advice), ('prod', A((j + 2 * t + 1) % sa.advice), F((j + t) % sa.fixed))] for t in range(K)],
               [F((j + 1) % sa.fixed), F((j + 2) % sa.fixed, 1)]) for j in range(ARGS)]
    else:  # the K tuples of an argument share selectors and columns; the table is fixed columns
        mv = [([side(sa, j, exprs, 2 * t) for t in range(K)], [F((j + 1 + t) % sa.fixed, t % 2) for t in range(exprs)]) for j in range(ARGS)]
    evaluator = ev.Evaluator.new(gates, lookups, [], mv)
    ek = k + 2
    n, size = 1 << k, 1 << ek
    d, _ = orc.domain_new(4, k)
    gen = lambda m, s: h2.gen_scalars_device(1000 + s, m)  # noqa: E731
    fe1 = lambda s: orc.gen_scalars(s, 1)[0]  # noqa: E731
    chunk_len, n_sets = 2, -(-sa.perm // 2)
    cols = {"fixed_cosets": [gen(size, 10 + i) for i in range(sa.fixed)], "advice_polys": [gen(n, 100 + i) for i in range(sa.advice)],
            "perm_product_cosets": [gen(size, 200 + i) for i in range(n_sets)], "perm_cosets": [gen(size, 300 + i) for i in range(sa.perm)],
            "l0": gen(size, 1), "l_last": gen(size, 2), "l_active_row": gen(size, 3),
            "lookups": [[gen(n, 400 + 3 * i + t) for t in range(3)] for i in range(sa.lookups)],
            "phi": [gen(n, 500 + j) for j in range(ARGS)], "m": [gen(n, 520 + j) for j in range(ARGS)]}
    d_values = gen(size, 999)
    stub = np.zeros((1, 4), dtype=np.uint64)
    case = {"k": k, "extended_k": ek, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
            "zeta": orc.constant(orc.FR, 5), "delta": orc.fe_from_int(orc.FR, pow(7, 1 << 28, R_MOD)),
            "y": fe1(1), "beta": fe1(2), "gamma": fe1(3), "theta": fe1(4), "l0": stub, "l_last": stub, "l_active_row": stub,
            "fixed_cosets": [stub] * sa.fixed, "advice_polys": [stub] * sa.advice, "instance_polys": [], "challenges": np.zeros((0, 4), dtype=np.uint64),
            "perm_product_cosets": [stub] * n_sets, "perm_cosets": [stub] * sa.perm, "perm_column_kind": np.zeros(sa.perm, dtype=np.uint32),
            "perm_column_index": (np.arange(sa.perm) % sa.advice).astype(np.uint32), "chunk_len": chunk_len, "last_rotation": -(B + 1),
            "lookups": [(stub, stub, stub)] * sa.lookups, "mvlookups": [(stub, stub)] * ARGS}
    hd, hm = evaluator.describe(case), evaluator.describe_mvlookups(case)
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
    hm.desc.phi_polys, hm.desc.m_polys = table(cols["phi"]), table(cols["m"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = L.h2hip_evaluate_h_ext_bn254_device(hd.byref(), hm.byref(), None, ctypes.c_void_p(d_values.data_ptr()), stream)
        assert rc == 0, L.h2hip_last_error()

    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(codegen), ctypes.c_uint32(0))  # mode 2: the kernels generated and compiled inline
    t0 = time.time()
    call()
    torch.cuda.synchronize()
    first_call_s = time.time() - t0
    counters0 = stage_counters(L)
    per = {"evalh_lookups": [], "evalh_mvlookups": [], "evalh_gates": [], "evalh_perm": [], "evalh_cosets": []}
    for _ in range(reps):
        h2.profile_enable(True)
        h2.profile_reset()
        call()
        torch.cuda.synchronize()
        h2.profile_enable(False)
        for name in per:
            per[name].append(h2.profile_get(name)[0])
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
    med = {name: statistics.median(v) for name, v in per.items()}
    out = {"stage_ms_median": med, "ms_per_lookup": med["evalh_lookups"] / max(1, sa.lookups), "ms_per_mvlookup": med["evalh_mvlookups"] / ARGS,
           "ms_per_mvlookup_runs": [v / ARGS for v in per["evalh_mvlookups"]], "ms_K_lookups": K * med["evalh_lookups"] / max(1, sa.lookups),
           "exprs_per_tuple": exprs, "codegen": codegen, "first_call_s": first_call_s}
    counters1 = stage_counters(L)
    if counters1:
        out["stage_launches_generated_interpreted"] = {name: [b[0] - a[0], b[1] - a[1]] for (name, a), b in zip(counters0.items(), counters1.values())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inputs", default="1,4", help="the values of K, inputs per table")
    ap.add_argument("--exprs", type=int, default=2, help="expressions a tuple in the evaluate_h part")
    ap.add_argument("--codegen", type=int, default=2, help="h2hip_debug_set_evalh_codegen mode for the evaluate_h part")
    ap.add_argument("--stage-only", action="store_true", help="the evaluate_h part alone")
    ap.add_argument("--out")
    args = ap.parse_args()
    import importlib
    import torch
    h2 = load_pkg()
    h2.init(0)
    ev = importlib.import_module("halo2_pse_amd.evaluation")
    from oracle import oracle as orc
    orc.build()
    k = args.k
    n = 1 << k
    u = n - B - 1
    fe1 = lambda s: orc.gen_scalars(s, 1)[0]  # noqa: E731

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

    rec = {"k": k, "extended_k": k + 2, "reps": args.reps, "blinding_factors": B, "clocks_before": clocks(), "K": {}}
    tab = h2.gen_scalars_device(2000, n)  # distinct values
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    for K in [int(x) for x in args.inputs.split(",")]:
        if args.stage_only:
            rec["K"][str(K)] = {"evaluate_h": evalh_stage(h2, ev, orc, torch, k, K, args.reps, args.exprs, args.codegen)}
            continue
        uniform = [tab[torch.randint(0, u, (n,), device="cuda", generator=g)].contiguous() for _ in range(K)]
        one = [tab[u // 2].repeat(n, 1).contiguous() for _ in range(K)]
        m, phi = [torch.empty_like(tab)], [torch.empty_like(tab)]
        pa, pt, z = ([torch.empty_like(tab) for _ in range(K)] for _ in range(3))
        beta, gamma = fe1(2), fe1(3)
        r = {}
        for name, inputs in (("uniform", uniform), ("one_value", one)):
            r["multiplicities_" + name] = timed(lambda: h2.mvlookup_multiplicities_device(k, [inputs], [tab], B, m))
            r["lookup_permute_" + name] = timed(lambda: h2.lookup_permute_device(k, inputs, [tab] * K, orc.gen_scalars(78, K * 2 * (B + 1)), B, pa, pt))
        h2.mvlookup_multiplicities_device(k, [uniform], [tab], B, m)
        h2.lookup_permute_device(k, uniform, [tab] * K, orc.gen_scalars(78, K * 2 * (B + 1)), B, pa, pt)
        r["sums"] = timed(lambda: h2.mvlookup_sums_device(k, beta, [uniform], [tab], m, orc.gen_scalars(77, B), B, phi))
        r["lookup_products"] = timed(lambda: h2.lookup_products_device(k, beta, gamma, uniform, [tab] * K, pa, pt, orc.gen_scalars(77, K * B), B, z))
        torch.cuda.synchronize()
        r["phi_u_is_zero"] = bool((phi[0][u] == 0).all().item())
        r["evaluate_h"] = evalh_stage(h2, ev, orc, torch, k, K, args.reps, args.exprs, args.codegen)
        rec["K"][str(K)] = r
    rec["clocks_after"] = clocks()
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
