#!/usr/bin/python3
"""The inner-product-argument commitment scheme on one GPU, medians of --reps after a warm-up, the card's clocks in the record.
Per k of --ks (default 17 and 20):
  opening_resident   one commitment::create_proof from a polynomial in HBM: wall time, and -- from a second set of runs that wait after
                     every call -- the split into collapse, normalise (the engine's stage timers), the two MSMs and the fold with its
                     inner products (wall around the calls), the rest being the host between calls; the wall time of every round of the
                     median run, whose smallest rounds are the floor a round trip per challenge sets (round_floor_ms; the same of
                     every timed run in round_floor_ms_runs, for the spread)
  opening_host       the same from a host polynomial (one upload)
                     Both paths of the opening are timed: the round call (h2hip_ipa_round, the default; the figures above) and, under
                     "separate_calls", the same figures with ipa.set_round_call(False).  In the round-call path the split has
                     round_call_ms (wall around round_device: the fold and the collapse by the challenge before, the inner products and
                     both MSMs) and a round runs from the end of one round_device to the end of the next, so round j holds the fold and
                     the collapse of round j - 1 (at twice its size) and the list closes with the last fold; msm_total_ms is the
                     engine's stage timer over every MSM run of the opening, in both paths
  multiopen          ProverIPA::create_proof on the queries of config 5 (tests/opening_util.py CONFIG5_SETS, the ones tools/opening_bench.py
                     times for SHPLONK): 21 polynomials, 26 queries, 4 points.  The time includes the commitment to q' and the whole
                     opening that follows; opening_bench's SHPLONK stages are the quotient kernels alone
  verify             compute_s + the 2^k MSM over the pinned g (GuardIPA::use_challenges and MSMIPA::check) and the host part before it
  params_new         ParamsIPA::new(k): hashing on the host, decompression in waves on the engine, g_to_lagrange
Generators come from gen_points (the derivation's cost is params_new's alone).

--compare: the one comparison with a verdict, for a run under `rocprofv3 --kernel-trace --stats` of its own -- g_to_lagrange at
k = 20 (its ecfft_layer_kernel runs 2^19 ladders per layer with per-lane digits and two closing additions) and a collapse of
half = 2^19 (uniform digits, one closing addition), alternating, --reps times each.  --parse DIR reads that run's kernel trace and adds
"compare" to the record: per dispatch, the layers with s >= 6 (at most one butterfly per wave skips its ladder there; every layer's
time is listed) against the collapse, time per butterfly against time per point.

  python tools/ipa_bench.py [--ks 17,20] [--reps 5] [--out profiles/ipa_bench.json]                        (run on the GPU box)
  rocprofv3 --kernel-trace --stats -d DIR -o cmp --output-format csv -- python tools/ipa_bench.py --compare
  python tools/ipa_bench.py --parse DIR --out profiles/ipa_bench.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402
import opening_util as ou  # noqa: E402

SEED = bytes(range(32))


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [line.strip() for line in out.splitlines() if "clk" in line.lower() and "(" in line]
    except Exception as e:  # noqa: BLE001  (the tool is absent or slow: the record says so)
        return ["unavailable: %r" % (e,)]


def med(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def wall(fn, reps, warm=1):
    import torch
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


class Split:
    """wall time around the round calls of ipa.create_proof, each followed by a wait (so this run is slower than the untimed one)"""

    def __init__(self, ipa):
        import torch
        self.ipa, self.torch, self.t = ipa, torch, {}
        self.names = ("msm_device", "fold_device", "collapse_device", "inner_products_device", "powers_device", "round_device")
        self.round_call = bool(ipa.lib().h2hip_ipa_get_round_call())
        self.saved = {n: getattr(ipa, n) for n in self.names}
        self.rounds, self.mark = [], None

    def __enter__(self):
        for n in self.names:
            setattr(self.ipa, n, self.wrap(n, self.saved[n]))
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.ipa, n, self.saved[n])
        return False

    def wrap(self, name, fn):
        def timed(*a, **kw):
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            self.torch.cuda.synchronize()
            now = time.perf_counter()
            self.t[name] = self.t.get(name, 0.0) + (now - t0) * 1e3
            # the last call of a round: the collapse, or the round call (and the fold that closes the opening)
            if name == ("round_device" if self.round_call else "collapse_device") or (self.round_call and name == "fold_device"):
                if self.mark is not None:
                    self.rounds.append((now - self.mark) * 1e3)
                self.mark = now
            if name == "powers_device":
                self.mark = now
            return out
        return timed


def bench_k(h2, ipa, T, k, reps):
    import torch
    n = 1 << k
    pts = h2.to_numpy_u64(h2.gen_points_device(0x1BA000 + k, n + 2))
    rec = {"k": k}
    with ipa.ParamsIPA.from_parts(pts[:n], pts[n], pts[n + 1]) as params:
        d_poly = h2.gen_scalars_device(0x1BA100 + k, n)
        h_poly = h2.to_numpy_u64(d_poly).copy()
        blind, x_3 = 12345, 0x1234567 << 64 | 0x89

        def open_(poly, resident):
            w = T.Blake2bWrite()
            ipa.create_proof(params, h2.FrRng(SEED), w, poly, blind, x_3, resident=resident)
            return w.finalize()

        def opening_figures():
            out = {"opening_resident": med(wall(lambda: open_(d_poly, True), reps)), "opening_host": med(wall(lambda: open_(h_poly, False), reps))}
            splits = []
            for r in range(1 + reps):
                h2.profile_enable(True)
                h2.profile_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with Split(ipa) as sp:
                    open_(d_poly, True)
                total = (time.perf_counter() - t0) * 1e3
                h2.profile_enable(False)
                if r == 0:
                    continue
                collapse, normalise = h2.profile_get("ipa_collapse")[0], h2.profile_get("ipa_normalize")[0]
                calls = sum(sp.t.values())
                splits.append({"total_ms": total, "collapse_ms": collapse, "normalise_ms": normalise, "msm_ms": sp.t["msm_device"],
                               "msm_total_ms": h2.profile_get("msm_total")[0], "round_call_ms": sp.t.get("round_device", 0.0),
                               "fold_and_inner_products_ms": sp.t.get("fold_device", 0.0) + sp.t.get("inner_products_device", 0.0),
                               "collapse_call_ms": sp.t.get("collapse_device", 0.0), "host_between_calls_ms": total - calls, "round_ms": sp.rounds})
            splits.sort(key=lambda s: s["total_ms"])
            mid = splits[len(splits) // 2]
            out["opening_split"] = mid
            out["round_floor_ms"] = min(mid["round_ms"][-4:]) if mid["round_ms"] else None
            # the same figure and the host share of every timed run, for the run-to-run spread beside the median run's
            out["round_floor_ms_runs"] = [min(s["round_ms"][-4:]) for s in splits if s["round_ms"]]
            out["host_between_calls_ms_runs"] = [s["host_between_calls_ms"] for s in splits]
            # every round of every timed run, for the spread of a round at a given half
            out["round_ms_runs"] = [s["round_ms"] for s in splits]
            return out

        try:
            ipa.set_round_call(True)
            rec.update(opening_figures())
            ipa.set_round_call(False)
            rec["separate_calls"] = opening_figures()
        finally:
            ipa.set_round_call(True)
        # verification: read the proof on the host, then compute_s and the MSM over the pinned g
        proof = open_(d_poly, True)
        commitment = params.commit(d_poly, blind)
        v = h2.fr_to_int(h2.eval_polynomials_device([d_poly], [0], [h2.fr_from_int(x_3)])[0])
        host_ts, dev_ts = [], []
        for r in range(1 + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            msm = params.empty_msm()
            msm.append_term(1, commitment)
            guard = ipa.verify_proof(params, msm, T.Blake2bRead(proof), x_3, v)
            t1 = time.perf_counter()
            ok = guard.use_challenges().check()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert ok
            if r:
                host_ts.append((t1 - t0) * 1e3)
                dev_ts.append((t2 - t1) * 1e3)
        rec["verify"] = {"host_transcript_and_scalars": med(host_ts), "compute_s_and_msm": med(dev_ts)}
        # multiopen on the queries tools/opening_bench.py times for SHPLONK: tests/opening_util.py CONFIG5_SETS -- 21 polynomials, 26
        # queries at the 4 points x, x omega, x omega^-6, x omega^-1, in sets of 17, 2, 1 and 1 polynomials
        polys = [h2.gen_scalars_device(0x1BA200 + i, n) for i in range(21)]
        at = ou.config5_points(k, T.Blake2bWrite().squeeze_challenge())
        queries = [(at[name], polys[i], 1000 + i) for names, cols in ou.CONFIG5_SETS for i in cols for name in names]
        assert len(queries) == ou.CONFIG5_QUERIES == 26

        def multiopen():
            w = T.Blake2bWrite()
            ipa.ProverIPA(params).create_proof(h2.FrRng(SEED), w, queries)

        rec["multiopen_21_polys_26_queries_4_points"] = med(wall(multiopen, reps))
        del polys
    t0 = time.perf_counter()
    with ipa.ParamsIPA.new(k):
        rec["params_new_s"] = time.perf_counter() - t0
    return rec


def compare(h2, ipa, reps):
    """alternate the two kernels; the figures come from the profiler's trace of this process"""
    import torch
    k = 20
    g = h2.gen_points_device(0x1BA300, 1 << k)
    out = torch.empty_like(g)
    for _ in range(1 + reps):
        h2._check(h2.lib().h2hip_g_to_lagrange_bn254_device(h2._dptr(g), k, h2._dptr(out), h2._stream()), "g_to_lagrange")
        d = g.clone()
        ipa.collapse_device(d, 1 << (k - 1), 0x1234567 << 100 | 0xabcdef)
        torch.cuda.synchronize()


def parse(directory):
    """the kernel trace of a --compare run -> per-dispatch times of ecfft_layer_kernel (by layer) and ipa_collapse_kernel"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % directory)
    layers, collapses = [], []
    for row in csv.DictReader(open(files[0])):
        name = row.get("Kernel_Name", "")
        ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        if "ecfft_layer_kernel" in name:
            layers.append(ns)
        elif "ipa_collapse_kernel" in name:
            collapses.append(ns)
    runs = [layers[i:i + 20] for i in range(0, len(layers) - 19, 20)][1:]  # 20 layers per transform; the first transform is the warm-up
    collapses = collapses[1:]
    ladders = 1 << 19
    per_layer = [statistics.median(r[s] for r in runs) for s in range(20)]
    # At layer s one butterfly in 2^s has the twiddle one and skips its ladder: up to s = 5 that is several lanes of every wave (and at
    # s = 0 all of them), so the yardstick is the layers from s = 6 on, where a wave of 64 lanes holds at most one such butterfly
    upper = [ns for r in runs for ns in r[6:]]
    rec = {"ladders": ladders, "ecfft_layer_ms_by_s": [ns / 1e6 for ns in per_layer],
           "ecfft_layer_s_ge_6": {"median_ns_per_butterfly": statistics.median(upper) / ladders, "min": min(upper) / ladders, "max": max(upper) / ladders},
           "ipa_collapse": {"median_ns_per_point": statistics.median(collapses) / ladders, "min": min(collapses) / ladders,
                            "max": max(collapses) / ladders, "runs": len(collapses)}}
    spread = (max(upper) - min(upper)) / statistics.median(upper)
    rec["run_to_run_spread_of_the_layer"] = spread
    lower = [ns for r in runs for ns in r[1:]]  # every layer with s >= 1, the cheap layers s = 1 .. 5 included
    rec["ecfft_layer_s_ge_1"] = {"median_ns_per_butterfly": statistics.median(lower) / ladders, "min": min(lower) / ladders, "max": max(lower) / ladders,
                                 "ns_per_butterfly_by_s": [ns / ladders for ns in per_layer]}
    rec["collapse_over_layer_s_ge_1_median"] = rec["ipa_collapse"]["median_ns_per_point"] / rec["ecfft_layer_s_ge_1"]["median_ns_per_butterfly"]
    rec["collapse_over_layer"] = rec["ipa_collapse"]["median_ns_per_point"] / rec["ecfft_layer_s_ge_6"]["median_ns_per_butterfly"]
    by_s = rec["ecfft_layer_s_ge_1"]["ns_per_butterfly_by_s"]
    point = rec["ipa_collapse"]["median_ns_per_point"]
    faster = [s for s in range(1, 20) if by_s[s] < point]
    rec["verdict"] = ("against the layers s >= 6 (every ladder runs): collapse per point %s layer per butterfly, within the spread; "
                      % ("<=" if rec["collapse_over_layer"] <= 1 + spread else ">") +
                      ("loses to the layers s = %s, where butterflies skip their ladder" % ", ".join(map(str, faster)) if faster
                       else "no layer with s >= 1 is faster per butterfly"))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--parse")
    ap.add_argument("--out")
    args = ap.parse_args()
    rec = {}
    if args.out and os.path.exists(args.out):
        rec = json.load(open(args.out))
    if args.parse:
        rec["compare"] = parse(args.parse)
    else:
        import importlib
        h2 = load_pkg()
        h2.init(0)
        ipa = importlib.import_module("halo2_pse_amd.ipa")
        T = importlib.import_module("halo2_pse_amd.transcript")
        if args.compare:
            compare(h2, ipa, args.reps)
            return
        rec.update({"reps": args.reps, "clocks_before": clocks(), "collapse_quad_max_half": ipa.set_collapse_quad(0)})
        rec["sizes"] = [bench_k(h2, ipa, T, int(k), args.reps) for k in args.ks.split(",")]
        rec["clocks_after"] = clocks()
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
