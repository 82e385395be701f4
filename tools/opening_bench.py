#!/usr/bin/python3
"""The opening phase (h2hip_eval_polynomials_bn254 / h2hip_poly_combine_bn254_fr) in the config-5 shape (the queries
create_proof issues for MyCircuit; tests/opening_util.py CONFIG5_SETS): 21 polynomials of 2^k coefficients, 26 queries at 4 points,
4 SHPLONK rotation sets of 17, 2, 1 and 1 polynomials (points 1, 2, 3, 2), 4 GWC points.  Per k, median of --reps after --warmup:
  device-resident: all 26 evaluations (one call, it synchronises), GWC's 4 witnesses, SHPLONK stage 1 (4 accumulating calls into h_x)
  and stage 2 (one call over the 21 polynomials and h_x), HIP events around each group after a synchronisation;
  host forms (wall clock around blocking calls): the evaluations and both SHPLONK stages, with the key's 9 polynomials (fixed 5-10,
  permutation 11-13) pinned and unpinned;
  the algorithmic Fr multiplications and bytes, and the achieved G mul/s.  The challenge-side scalars (powers, interpolants, z_i) are
  computed once, outside the timed calls.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/opening_bench.py`
  in a process of its own.
  python tools/opening_bench.py [--k 17 20 22] [--reps 7] [--out profiles/opening_bench.json]     (run on the GPU box)
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402
import opening_util as ou  # noqa: E402

KEY = list(range(5, 14))  # fixed 5-10 and the permutation polys 11-13: constant across proofs, pinnable


def plan(k, evals, names, y, v, u):
    """the engine calls of GWC and both SHPLONK stages as (poly indices, scalars, sub, roots, scale) tuples, integers"""
    p = ou.R_MOD
    gwc = []
    for pn, cols in ou.config5_gwc_groups():
        pw = ou.powers(v, len(cols))
        e = sum(pw[i] * evals[(j, pn)] for i, j in enumerate(cols)) % p
        gwc.append((cols, pw, [e], [names[pn]], 1))
    sup = [names[x] for x in ("x", "xw", "xlast", "xwinv")]
    st1, cols2, scal2, const, z0 = [], [], [], 0, None
    for i, (pn, cols) in enumerate(ou.CONFIG5_SETS):
        pts = [names[x] for x in pn]
        py = ou.powers(y, len(cols))
        interp = [ou.lagrange_interpolate(pts, [evals[(j, x)] for x in pn]) for j in cols]
        sub = [sum(py[c] * interp[c][t] for c in range(len(cols))) % p for t in range(len(pts))]
        st1.append((cols, py, sub, pts, pow(v, i, p)))
        z_i = ou.evaluate_vanishing_polynomial([x for x in sup if x not in pts], u)
        z0 = z_i if z0 is None else z0
        for c, j in enumerate(cols):
            w = pow(v, i, p) * z_i * py[c] % p
            cols2.append(j), scal2.append(w)
            const = (const + w * ou.eval_polynomial(interp[c], u)) % p
    scal2.append(-ou.evaluate_vanishing_polynomial(sup, u) % p)
    st2 = (cols2, scal2, [const], [u], pow(z0, -1, p))
    return gwc, st1, st2


def counts(k, gwc, st1, st2):
    """algorithmic Fr multiplications and HBM bytes: Horner per query; per combine call one product per polynomial and element, two
    per element and root (the scan's suffix and the apply pass), one for the scale; bytes: each polynomial read once per call, the
    scans' scratch written and read, the output written"""
    n = 1 << k
    m_eval, b_eval = ou.CONFIG5_QUERIES * n, ou.CONFIG5_POLYS * n * 32
    def call(n_polys, n_roots, scaled):
        return n * (n_polys + 2 * n_roots + (1 if scaled else 0)), n * 32 * (n_polys + 3 * n_roots + 1)
    g = [call(len(c[0]), 1, False) for c in gwc]
    s1 = [call(len(c[0]), len(c[3]), True) for c in st1]
    s2 = call(len(st2[0]), 1, True)
    tot = lambda xs: (sum(x[0] for x in xs), sum(x[1] for x in xs))
    return {"eval": (m_eval, b_eval), "gwc": tot(g), "shplonk_stage1": tot(s1), "shplonk_stage2": s2}


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
    fe = ou.fe
    results = []
    for k in args.k:
        n = 1 << k
        rng = random.Random(0x0BE7 + k)
        d = [h2.gen_scalars_device(0xA000 + j, n) for j in range(ou.CONFIG5_POLYS)]
        names = ou.config5_points(k, rng.randrange(ou.R_MOD))
        qp, pts = [], []
        for pn, cols in ou.CONFIG5_SETS:
            for j in cols:
                for x in pn:
                    qp.append(j), pts.append(x)
        mpts = ou.to_mont([names[x] for x in pts])
        ev = ou.from_mont(h2.eval_polynomials_device(d, qp, mpts))
        evals = {(j, x): e for j, x, e in zip(qp, pts, ev)}
        y, v, u = (rng.randrange(ou.R_MOD) for _ in range(3))
        gwc, st1, st2 = plan(k, evals, names, y, v, u)
        M = lambda xs: ou.to_mont(xs)
        gwc_m = [(c, M(s), M(sb), M(r), fe(sc)) for c, s, sb, r, sc in gwc]
        st1_m = [(c, M(s), M(sb), M(r), fe(sc)) for c, s, sb, r, sc in st1]
        st2_m = (st2[0], M(st2[1]), M(st2[2]), M(st2[3]), fe(st2[4]))
        w_out = [torch.empty((n - 1, 4), dtype=torch.int64, device="cuda") for _ in gwc]
        h_x = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        f_out = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")

        def dev_eval():
            h2.eval_polynomials_device(d, qp, mpts)

        def dev_gwc():
            for (c, s, sb, r, sc), o in zip(gwc_m, w_out):
                h2.poly_combine_device([d[j] for j in c], s, o, sub=sb, roots=r, scale=sc)

        def dev_st1():
            for i, (c, s, sb, r, sc) in enumerate(st1_m):
                h2.poly_combine_device([d[j] for j in c], s, h_x, sub=sb, roots=r, scale=sc, accumulate=i > 0)

        def dev_st2():
            c, s, sb, r, sc = st2_m
            h2.poly_combine_device([d[j] for j in c] + [h_x], s, f_out, sub=sb, roots=r, scale=sc)

        row = {"k": k, "polys": ou.CONFIG5_POLYS, "queries": ou.CONFIG5_QUERIES, "rotation_sets": len(ou.CONFIG5_SETS), "gwc_points": len(gwc)}
        cnt = counts(k, gwc, st1, st2)
        for label, fn in (("eval", dev_eval), ("gwc", dev_gwc), ("shplonk_stage1", dev_st1), ("shplonk_stage2", dev_st2)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            med = statistics.median(ts)
            muls, byts = cnt[label]
            row[label] = {"device_ms_median": round(med, 4), "device_ms_all": [round(x, 4) for x in ts], "fr_muls": muls, "bytes": byts,
                          "mul_rate_G_per_s": round(muls / (med * 1e-3) / 1e9, 1), "fraction_of_179G": round(muls / (med * 1e-3) / 179e9, 3)}
        row["shplonk_both_device_ms"] = round(row["shplonk_stage1"]["device_ms_median"] + row["shplonk_stage2"]["device_ms_median"], 4)
        if not args.no_host:
            hp = [h2.to_numpy_u64(t).copy() for t in d]

            def host_call():
                h2.eval_polynomials(hp, qp, mpts)
                h = None
                for i, (c, s, sb, r, sc) in enumerate(st1_m):
                    if h is None:
                        h = h2.poly_combine([hp[j] for j in c], s, sub=sb, roots=r, scale=sc, out_len=n)
                    else:
                        h2.poly_combine([hp[j] for j in c], s, sub=sb, roots=r, scale=sc, out=h, accumulate=True)
                c, s, sb, r, sc = st2_m
                h2.poly_combine([hp[j] for j in c] + [h], s, sub=sb, roots=r, scale=sc)

            for label in ("host_eval_shplonk_ms_median", "host_eval_shplonk_pinned_ms_median"):
                if "pinned" in label:
                    h2.columns_pin([hp[j] for j in KEY])
                for _ in range(args.warmup):
                    host_call()
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    host_call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                row[label] = round(statistics.median(ts), 3)
            h2.columns_unpin([hp[j] for j in KEY])
            del hp
        print(json.dumps(row), flush=True)
        results.append(row)
        del d, w_out, h_x, f_out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
