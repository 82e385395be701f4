#!/usr/bin/python3
"""evaluate_h (plonk/evaluation.rs:280-522) on device-resident columns: time per call by HIP events, and the oracle on the
host cores beside it.  The constraint system is synthetic but shaped like a mid-sized PLONKish circuit: `--gates` degree-4
gate polynomials over `--advice` advice and `--fixed` fixed columns with rotations in [-2, 2], a permutation over
`--perm` columns, `--lookups` lookups.  Columns come from the engine's on-device generator.

  python tools/evalh_bench.py --k 18 [--check-k 12]     (run on the GPU box)
  python tools/evalh_bench.py --k 18 --parts            (the parts form beside the full form; also with the key's part cosets pinned,
                                                         and with the coset scaling fused into the transform's first-pass load)
  python tools/evalh_bench.py --k 12 --parts            (launch-bound: `enqueue_us`, the host time of a device-form call, for both forms)
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def system_expressions(args, rng):
    """(gate polynomials, [(input expressions, table expressions)]) of the synthetic system"""
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    gates = []
    for gi in range(args.gates):
        a, b, c, d = (int(x) for x in rng.integers(0, args.advice, 4))
        f1, f2, f3 = (int(x) for x in rng.integers(0, args.fixed, 3))
        r1, r2 = (int(x) for x in rng.integers(-2, 3, 2))
        gates.append(('prod', F(f1), ('sum', ('sum', ('prod', ('prod', A(a, r1), A(b)), A(c)), ('neg', ('prod', A(d, r2), F(f2)))),
                                      ('scaled', F(f3), 3 + gi))))
    lookups = [([A(li % args.advice), ('prod', A((li + 1) % args.advice), F(li % args.fixed))], [F((li + 1) % args.fixed), F((li + 2) % args.fixed, 1)])
               for li in range(args.lookups)]
    return gates, lookups


def enqueue_us(call, reps=200):
    """host time of one device-form call in microseconds: the clock around the call alone, its kernels not waited for (median of `reps`
    after a warm-up; the queue is drained between calls, outside the clock).  At a small k the call is launch-bound and this is what the
    caller's thread sees of the driver's host work."""
    import torch
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
    return float(np.median(ts)) * 1e6


def build_system(ev, args, rng):
    return ev.Evaluator.new(*system_expressions(args, rng))


def bench(args):
    """args: namespace with k, check_k, gates, advice, fixed, perm, lookups, iters, cpu -> result dict"""
    import importlib
    import torch
    h2 = load_pkg()
    ev = importlib.import_module("halo2_pse_amd.evaluation")
    from oracle import oracle as orc
    orc.build()
    L = h2.lib()
    rng = np.random.default_rng(1)
    evaluator = build_system(ev, args, rng)
    chunk_len = 2                      # cs.degree() = 4
    n_sets = -(-args.perm // chunk_len)
    out = {"gates": args.gates, "advice": args.advice, "fixed": args.fixed, "perm_columns": args.perm, "lookups": args.lookups,
           "custom_calcs": len(evaluator.custom_gates.calculations), "custom_intermediates": evaluator.custom_gates.num_intermediates,
           "custom_rotations": len(evaluator.custom_gates.rotations)}

    def run(k, check, time_cpu, host_timing=False):
        ek = k + 2
        n, size = 1 << k, 1 << ek
        d, _ = orc.domain_new(4, k)
        gen = lambda m, s: h2.gen_scalars_device(1000 + s, m)  # noqa: E731
        fe1 = lambda s: orc.gen_scalars(s, 1)[0]  # noqa: E731
        cols = {
            "fixed_cosets": [gen(size, 10 + i) for i in range(args.fixed)],
            "advice_polys": [gen(n, 100 + i) for i in range(args.advice)],
            "instance_polys": [],
            "perm_product_cosets": [gen(size, 200 + i) for i in range(n_sets)],
            "perm_cosets": [gen(size, 300 + i) for i in range(args.perm)],
            "l0": gen(size, 1), "l_last": gen(size, 2), "l_active_row": gen(size, 3),
            "lookups": [[gen(n, 400 + 3 * i + t) for t in range(3)] for i in range(args.lookups)],
        }
        d_values = gen(size, 999)
        v0 = d_values.clone()
        torch.cuda.synchronize()
        host = lambda t: h2.to_numpy_u64(t)  # noqa: E731
        scal = {"extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
                "zeta": orc.constant(orc.FR, 5), "delta": orc.fe_from_int(orc.FR, pow(7, 1 << 28, R_MOD)),
                "y": fe1(1), "beta": fe1(2), "gamma": fe1(3), "theta": fe1(4)}
        perm_kind = np.zeros(args.perm, dtype=np.uint32)
        perm_index = (np.arange(args.perm) % args.advice).astype(np.uint32)
        # a host description with tiny stand-in columns gives the struct; device addresses are swapped in below
        stub = np.zeros((1, 4), dtype=np.uint64)
        case = {"k": k, "extended_k": ek, **scal, "l0": stub, "l_last": stub, "l_active_row": stub,
                "fixed_cosets": [stub] * args.fixed, "advice_polys": [stub] * args.advice, "instance_polys": [],
                "challenges": np.zeros((0, 4), dtype=np.uint64),
                "perm_product_cosets": [stub] * n_sets, "perm_cosets": [stub] * args.perm, "perm_column_kind": perm_kind, "perm_column_index": perm_index,
                "chunk_len": chunk_len, "last_rotation": -6, "lookups": [(stub, stub, stub)] * args.lookups}
        hd = evaluator.describe(case)
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
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            rc = L.h2hip_evaluate_h_bn254_device(hd.byref(), ctypes.c_void_p(d_values.data_ptr()), stream)
            assert rc == 0, L.h2hip_last_error()

        call()
        torch.cuda.synchronize()
        res = {}
        if check or time_cpu or host_timing:
            case_h = dict(case)
            for key in ("fixed_cosets", "advice_polys", "perm_product_cosets", "perm_cosets"):
                case_h[key] = [host(t) for t in cols[key]]
            for key in ("l0", "l_last", "l_active_row"):
                case_h[key] = host(cols[key])
            case_h["lookups"] = [tuple(host(t) for t in l) for l in cols["lookups"]]
            hh = evaluator.describe(case_h)
        if host_timing:
            # the host-pointer call (what patch 0003's evaluate_h_gpu makes: every column a Vec<F>), PCIe included, without and with the
            # proving key's constant columns pinned in HBM (h2hip_columns_pin: fixed cosets, l0 / l_last / l_active_row, permutation cosets)
            vals = host(v0).copy()

            def host_call():
                np.copyto(vals, host(v0))
                t0 = time.perf_counter()
                assert L.h2hip_evaluate_h_bn254(hh.byref(), vals.ctypes.data_as(ctypes.c_void_p)) == 0, L.h2hip_last_error()
                return (time.perf_counter() - t0) * 1e3

            def med(nrep=5):
                host_call()
                return float(np.median([host_call() for _ in range(nrep)]))

            key_cols = list(case_h["fixed_cosets"]) + list(case_h["perm_cosets"]) + [case_h["l0"], case_h["l_last"], case_h["l_active_row"]]
            full = 32 << ek
            n_full = len(key_cols) + len(case_h["perm_product_cosets"]) + 1
            res["host_pointer"] = {"ms_per_call_unpinned": med(), "full_size_columns": n_full, "key_columns": len(key_cols),
                                   "upload_MiB_unpinned": (n_full * full + (args.advice + 3 * args.lookups) * (32 << k)) / 2**20}
            h2.columns_pin(key_cols)
            res["host_pointer"]["ms_per_call_key_columns_pinned"] = med()
            res["host_pointer"]["upload_MiB_pinned"] = ((n_full - len(key_cols)) * full + (args.advice + 3 * args.lookups) * (32 << k)) / 2**20
            res["host_pointer"]["pinned_bytes"] = h2.columns_pinned_info()[1]
            h2.columns_unpin(key_cols)
        if check or time_cpu:
            want = host(v0).copy()
            t0 = time.perf_counter()
            assert orc.lib().oracle_evaluate_h(hh.byref(), want.ctypes.data_as(ctypes.c_void_p)) == 0
            res["oracle_s"] = time.perf_counter() - t0
            res["match"] = bool(np.array_equal(host(d_values), want))
            assert res["match"], "GPU evaluate_h differs from the oracle"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed():
            ts = []
            for _ in range(args.iters):
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            return float(np.median(ts))

        def stages():  # per-stage HIP-event times of the same call (their records put ~10 us of gap on the stream each)
            h2.profile_enable(True)
            h2.profile_reset()
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            h2.profile_enable(False)
            st = {}
            for name in ("evalh_cosets", "evalh_gates", "evalh_perm", "evalh_lookups"):
                tot, cnt = h2.profile_get(name)
                st[name] = tot / cnt if cnt else None
            return st

        # custom gates through the byte-code interpreter, then through the kernel generated for this circuit (compiled inline by hiprtc)
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(0), ctypes.c_uint32(0))
        call()
        res["interpreter"] = {"gpu_ms": timed(), "stage_ms": stages()}
        stats0 = (ctypes.c_uint64 * 5)()
        L.h2hip_debug_evalh_codegen_stats(stats0)
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(2), ctypes.c_uint32(0))
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        first_call_s = time.perf_counter() - t0
        stats1 = (ctypes.c_uint64 * 5)()
        L.h2hip_debug_evalh_codegen_stats(stats1)
        generated = stats1[2] > stats0[2]
        res["gpu_ms"] = timed()
        res["stage_ms"] = stages()
        res["enqueue_us"] = enqueue_us(call)
        res["gates_kernel"] = "generated per circuit (hiprtc)" if generated else "interpreter (the program is beyond the generator's limits, or hiprtc is missing)"
        res["first_call_with_inline_compile_s"] = first_call_s
        if check or time_cpu:
            L.h2hip_debug_set_evalh_codegen(ctypes.c_int(2), ctypes.c_uint32(0))
            d_values.copy_(v0)
            call()
            torch.cuda.synchronize()
            res["match_generated"] = bool(np.array_equal(host(d_values), want))
            assert res["match_generated"], "GPU evaluate_h (generated gates kernel) differs from the oracle"
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
        res["rows_per_s"] = size / (res["gpu_ms"] * 1e-3)
        # the gates kernel against the multiplier: field multiplications per row of the compiled program x rows / kernel time
        n_mul = ctypes.c_uint32()
        if L.h2hip_debug_evalh_program_muls(ctypes.byref(hd.desc.custom_gates), ctypes.byref(n_mul)) == 0 and res["stage_ms"].get("evalh_gates"):
            gmul = n_mul.value * size / (res["stage_ms"]["evalh_gates"] * 1e-3) / 1e9
            res["gates_valu_roofline"] = {"bound": "valu-int", "kernel": "evalh_gates_gen" if generated else "evalh_gates_kernel", "field_mul_per_row": n_mul.value,
                                          "achieved": gmul, "peak": 179.0, "unit": "Gmul/s", "frac": gmul / 179.0}
        return res

    if args.check_k:
        out["check_k%d" % args.check_k] = run(args.check_k, True, False)
    out["k%d" % args.k] = run(args.k, False, args.cpu)
    if getattr(args, "host_k", 0):
        out["host_k%d" % args.host_k] = {k_: v for k_, v in run(args.host_k, False, False, host_timing=True).items() if k_ in ("host_pointer", "gpu_ms")}
    return out


def bench_parts(args):
    """--parts: the parts form (h2hip_evaluate_h_parts_bn254[_device], one coset of the 2^k domain at a time from coefficient-form
    columns) beside the full form on the same polynomials: device-resident time (median of --iters after a warm-up call) with the
    per-stage times, host-pointer time with the bytes each form sends over PCIe, and the HBM the engine allocates for each beside what
    h2hip_evaluate_h_workspace_bytes predicts.  The parts form runs first: the engine's arena only grows."""
    import importlib
    import torch
    h2 = load_pkg()
    ev = importlib.import_module("halo2_pse_amd.evaluation")
    from oracle import oracle as orc
    orc.build()
    L = h2.lib()
    evaluator = build_system(ev, args, np.random.default_rng(1))
    k, ek = args.k, args.k + 2
    n, size, chunk_len = 1 << k, 1 << (args.k + 2), 2
    n_sets = -(-args.perm // chunk_len)
    d, t_eval = orc.domain_new(4, k)
    h2.init()
    gen = lambda s: h2.gen_scalars_device(1000 + s, n)  # noqa: E731
    fe1 = lambda s: orc.gen_scalars(s, 1)[0]  # noqa: E731
    polys = {"fixed_polys": [gen(10 + i) for i in range(args.fixed)], "advice_polys": [gen(100 + i) for i in range(args.advice)], "instance_polys": [],
             "perm_product_polys": [gen(200 + i) for i in range(n_sets)], "perm_polys": [gen(300 + i) for i in range(args.perm)],
             "l0_poly": gen(1), "l_last_poly": gen(2), "l_active_row_poly": gen(3),
             "lookups": [[gen(400 + 3 * i + t) for t in range(3)] for i in range(args.lookups)]}
    v0 = h2.gen_scalars_device(1999, size)
    torch.cuda.synchronize()
    scal = {"extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
            "zeta": orc.constant(orc.FR, 5), "delta": orc.fe_from_int(orc.FR, pow(7, 1 << 28, R_MOD)),
            "y": fe1(1), "beta": fe1(2), "gamma": fe1(3), "theta": fe1(4)}
    common = {"k": k, "extended_k": ek, **scal, "challenges": np.zeros((0, 4), dtype=np.uint64), "chunk_len": chunk_len, "last_rotation": -6,
              "perm_column_kind": np.zeros(args.perm, dtype=np.uint32), "perm_column_index": (np.arange(args.perm) % args.advice).astype(np.uint32)}
    renamed = {"fixed_polys": "fixed_cosets", "perm_product_polys": "perm_product_cosets", "perm_polys": "perm_cosets", "l0_poly": "l0",
               "l_last_poly": "l_last", "l_active_row_poly": "l_active_row", "advice_polys": "advice_polys", "instance_polys": "instance_polys"}
    host = lambda t: h2.to_numpy_u64(t)  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []

    def table(ts):
        arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        keep.append(arr)
        return ctypes.addressof(arr)

    def describe(form, cols, on_device):
        """a description of `cols` (tensors) for the parts or the full form, with host arrays or device addresses"""
        stub = np.zeros((1, 4), dtype=np.uint64)
        conv = (lambda t: stub) if on_device else host
        case = dict(common)
        for name, v in cols.items():
            if name != "lookups":
                case[name] = [conv(t) for t in v] if isinstance(v, list) else conv(v)
        case["lookups"] = [tuple(conv(t) for t in l) for l in cols["lookups"]]
        hd = evaluator.describe_parts(case) if form == "parts" else evaluator.describe(case)
        hd.case = case  # the host arrays themselves: a pin is keyed by their addresses
        if on_device:
            for name, v in cols.items():
                if name != "lookups":
                    setattr(hd.desc, name, table(v) if isinstance(v, list) else v.data_ptr())
            for t, name in enumerate(("lookup_product_polys", "lookup_permuted_input_polys", "lookup_permuted_table_polys")):
                setattr(hd.desc, name, table([l[t] for l in cols["lookups"]]))
        return hd

    def key_of(c):
        return list(c["fixed_polys"]) + [c["l0_poly"], c["l_last_poly"], c["l_active_row_poly"]] + list(c["perm_polys"])

    def parts_stats():
        names = ("columns_transformed", "columns_from_pins", "uploaded_column_bytes", "arena_bytes")
        return dict(zip(names, h2.evalh_parts_stats()))

    def measure(form, cols, pin=False, fused=False):
        """pin: the key's part cosets pinned for each leg (device tensors, then the host arrays); fused: the unpinned columns scaled in
        the transform's first-pass load instead of by the scale kernel (h2hip_debug_evalh_part_fused)"""
        res = {}
        dom = h2.EvaluationDomain.new(4, k)
        L.h2hip_debug_evalh_part_fused(ctypes.c_int(1 if fused else 0))
        if pin:
            h2.part_cosets_pin(key_of(cols), dom)
            res["pinned_info_device_form"] = h2.part_cosets_pinned_info()
        fn_dev = L.h2hip_evaluate_h_parts_bn254_device if form == "parts" else L.h2hip_evaluate_h_bn254_device
        fn_host = L.h2hip_evaluate_h_parts_bn254 if form == "parts" else L.h2hip_evaluate_h_bn254
        hd = describe(form, cols, True)
        d_values = v0.clone()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]

        def call():
            assert fn_dev(hd.byref(), ctypes.c_void_p(d_values.data_ptr()), stream) == 0, L.h2hip_last_error()

        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(2), ctypes.c_uint32(0))
        call()  # warm-up: tables, arena, the generated kernels compiled inline
        torch.cuda.synchronize()
        res["engine_hbm_MiB_device_form"] = (free0 - torch.cuda.mem_get_info()[0]) / 2**20
        d_values.copy_(v0)
        call()
        torch.cuda.synchronize()
        result = d_values.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(args.iters):
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res["gpu_ms"] = float(np.median(ts))
        res["gpu_ms_runs"] = ts
        if form == "parts":
            res["stats_device_form"] = parts_stats()
        res["enqueue_us"] = enqueue_us(call)
        h2.profile_enable(True)
        h2.profile_reset()
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        h2.profile_enable(False)
        res["stage_ms"] = {}
        for name in ("evalh_cosets", "evalh_part_scale", "ntt", "evalh_part_io", "evalh_gates", "evalh_perm", "evalh_lookups"):
            tot, cnt = h2.profile_get(name)
            res["stage_ms"][name] = tot / 3 if cnt else None  # per call: a stage runs once per part in the parts form
        # host pointers: what a patched prover's Vec<F>s cost, PCIe included
        if pin:
            h2.part_cosets_unpin(key_of(cols))
        hh = describe(form, cols, False)
        if pin:
            h2.part_cosets_pin(key_of(hh.case), dom)
            res["pinned_info_host_form"] = h2.part_cosets_pinned_info()
        vals = host(v0).copy()

        def host_call():
            np.copyto(vals, host(v0))
            t0 = time.perf_counter()
            assert fn_host(hh.byref(), vals.ctypes.data_as(ctypes.c_void_p)) == 0, L.h2hip_last_error()
            return (time.perf_counter() - t0) * 1e3

        free1 = torch.cuda.mem_get_info()[0]
        host_call()
        res["engine_hbm_MiB_host_form_on_top"] = (free1 - torch.cuda.mem_get_info()[0]) / 2**20
        res["host_ms_runs"] = [host_call() for _ in range(5)]
        res["host_ms"] = float(np.median(res["host_ms_runs"]))
        res["host_matches_device"] = bool(np.array_equal(vals, host(result)))
        if form == "parts":
            res["stats_host_form"] = parts_stats()
        if pin:
            h2.part_cosets_unpin(key_of(hh.case))
        L.h2hip_debug_evalh_part_fused(ctypes.c_int(0))
        n_small = args.advice + 3 * args.lookups
        n_key = args.fixed + args.perm + 3 + n_sets
        up = (n_key + n_small) * (32 << k) if form == "parts" else n_key * (32 << ek) + n_small * (32 << k)
        res["pcie_MiB"] = {"up_columns": up / 2**20, "values_each_way": (32 << ek) / 2**20}
        q = lambda dev: ev.evaluate_h_workspace_bytes(k, ek, args.fixed, args.advice, 0, n_sets, args.perm, args.lookups, form == "parts", dev)  # noqa: E731
        res["workspace_bytes_MiB"] = {"device_form": q(True) / 2**20, "host_form": q(False) / 2**20}
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
        return res, result

    out = {"k": k, "extended_k": ek, "gates": args.gates, "advice": args.advice, "fixed": args.fixed, "perm_columns": args.perm, "perm_sets": n_sets,
           "lookups": args.lookups, "iters": args.iters}
    out["parts"], got = measure("parts", polys)
    out["parts_fused_load"], got_f = measure("parts", polys, fused=True)
    out["parts_pinned"], got_p = measure("parts", polys, pin=True)
    assert torch.equal(got, got_f) and torch.equal(got, got_p), "the fused load or the pinned part cosets change the result"
    # the full form's columns: the extended cosets of the same polynomials, formed by the engine
    cosets = {}
    for name, v in polys.items():
        if name in ("advice_polys", "instance_polys", "lookups"):
            cosets[name] = v
            continue
        ts = v if isinstance(v, list) else [v]
        ext = []
        for t in ts:
            e = torch.zeros((size,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            e[:n] = t
            ext.append(e)
        if ext:
            h2.coeff_to_extended_batch_device(ext, k, ek, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
        cosets[renamed[name]] = ext if isinstance(v, list) else ext[0]
    torch.cuda.synchronize()
    out["full"], want = measure("full", cosets)
    out["parts_equal_full"] = bool(torch.equal(got, want))
    assert out["parts_equal_full"], "the parts form differs from the full form"
    out["parts_over_full_gpu"] = out["parts"]["gpu_ms"] / out["full"]["gpu_ms"]
    return out


def default_args(**over):
    ns = argparse.Namespace(k=18, check_k=12, gates=24, advice=12, fixed=10, perm=9, lookups=2, iters=5, cpu=False, host_k=16)
    for key, v in over.items():
        setattr(ns, key, v)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--check-k", type=int, default=12, help="size at which the GPU result is compared with the oracle (0 = skip)")
    ap.add_argument("--gates", type=int, default=24)
    ap.add_argument("--advice", type=int, default=12)
    ap.add_argument("--fixed", type=int, default=10)
    ap.add_argument("--perm", type=int, default=9)
    ap.add_argument("--lookups", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="time the oracle at --k too (single thread)")
    ap.add_argument("--host-k", type=int, default=16, help="also time the host-pointer call at this k, with and without the key's columns pinned (0 = skip)")
    ap.add_argument("--parts", action="store_true", help="time the parts form beside the full form at --k instead (device and host pointers, HBM)")
    args = ap.parse_args()
    print(json.dumps(bench_parts(args) if args.parts else bench(args)))


if __name__ == "__main__":
    main()
