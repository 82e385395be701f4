#!/usr/bin/python3
"""What closing a KZG check costs (include/halo2hip_pairing.h, halo2-pse_amd/kzg.py).
  python tools/pairing_bench.py --host          no GPU: the median of 21 runs of a two-pair pairing_check, of g2_mul and of the Gt
                                                value path (h2hip_pairing_bn254 on the same two pairs), with the CPU's name
  python tools/pairing_bench.py [--k K]         on the GPU box, the card's clocks in the record: one KZG verify_proof under SingleStrategy on the circuit-layout shape of
                                                tools/proof_bench.py at k = 17 (SHPLONK), split into the verifier on Python integers
                                                and the closing (both sides evaluated in the library, then the pairing check); the same
                                                accumulated over 16 proofs, per proof; ParamsKZG.check_structure at k = 17 and 20, split
                                                into the two MSMs of the powers check, the transform and commits of the Lagrange check,
                                                and the pairing calls
Prints one JSON line; --out FILE also writes it there, indented."""
import importlib
import json
import os
import platform
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402

RUNS = 21


def median_ms(f, runs=RUNS):
    f()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 4)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [line.strip() for line in out.splitlines() if "clk" in line.lower() and "(" in line]
    except Exception as e:  # noqa: BLE001  (the tool is absent or slow: the record says so)
        return ["unavailable: %r" % (e,)]


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def host(h2, kzg):
    """a check of the shape DualMSM::check makes: e(L, s g2) e(-s L, g2) = 1"""
    import numpy as np
    s = 0x1D0C5EC2E7A9B3F40718293A4B5C6D7E8F9
    left = h2.g1_linear_combinations(None, [[0xABCDEF12345]], [(1, 2)])[0]
    right = h2.g1_linear_combinations(None, [[-s % h2.FR_MODULUS]], [left])[0]
    g1 = np.stack([h2.g1_from_int(left), h2.g1_from_int(right)])
    s_g2 = kzg.g2_mul(kzg.G2_GENERATOR, s)
    g2 = np.frombuffer(s_g2 + kzg.G2_GENERATOR, dtype=np.uint64).reshape(2, 16).copy()
    assert kzg.pairing_check(g1, g2)
    return {"cpu": cpu_name(), "runs": RUNS, "stat": "median, host clock around the Python wrapper",
            "pairing_check_two_pairs_ms": median_ms(lambda: kzg.pairing_check(g1, g2)),
            "pairing_value_two_pairs_ms": median_ms(lambda: kzg.pairing(g1, g2)),
            "pairing_value_one_pair_ms": median_ms(lambda: kzg.pairing(g1[:1], g2[:1])),
            "g2_mul_ms": median_ms(lambda: kzg.g2_mul(kzg.G2_GENERATOR, s)),
            "g2_check_ms": median_ms(lambda: kzg.g2_check(s_g2))}


def gpu(h2, kzg, k):
    import numpy as np
    import torch
    import proof_bench as pb
    prover, verifier, tr = (importlib.import_module("halo2_pse_amd." + m) for m in ("prover", "verifier", "transcript"))
    h2.init()
    cs = pb.circuit(prover)
    fixed, advice, copies = pb.assignment(k, cs.blinding_factors())
    params = h2.ParamsKZG.setup(k, pb.SECRET)
    pk = prover.ProvingKey.build(params, cs, fixed, copies, 0x17)
    cols = [torch.from_numpy(a.view(np.int64)).cuda() for a in advice]
    proof = prover.create_proof(params, pk, [[]], lambda i, phase, ch: cols, tr.Blake2bWrite(), b"\x11" * 32, multiopen="shplonk").bytes
    read = lambda: tr.Blake2bRead(proof)  # noqa: E731

    def single():
        verifier.verify_proof(params, pk.vk, [[]], read(), "shplonk", strategy=kzg.SingleStrategy(params))

    def accumulate(count):
        acc = kzg.AccumulatorStrategy(params, h2.FrRng(b"\x21" * 32))
        t = time.perf_counter()
        for _ in range(count):
            verifier.verify_proof(params, pk.vk, [[]], read(), "shplonk", strategy=acc)
        t_verifier = time.perf_counter() - t
        sides = (len(acc.msm_accumulator.left.terms), len(acc.msm_accumulator.right.terms))
        t = time.perf_counter()
        left, right = kzg.eval_msm(acc.msm_accumulator.left), kzg.eval_msm(acc.msm_accumulator.right)
        t_eval = time.perf_counter() - t
        t = time.perf_counter()
        ok = kzg.pairing_check([left, right], [params.s_g2, kzg.g2_neg(params.g2)])
        t_pairing = time.perf_counter() - t
        assert ok
        return {"proofs": count, "terms_left_right": sides, "verifier_python_integers_ms": round(t_verifier * 1e3, 3),
                "sides_evaluated_in_library_ms": round(t_eval * 1e3, 3), "pairing_check_ms": round(t_pairing * 1e3, 3),
                "per_proof_ms": round((t_verifier + t_eval + t_pairing) * 1e3 / count, 3)}

    t = time.perf_counter()
    left, right = verifier.verify_proof(params, pk.vk, [[]], read(), "shplonk")
    no_strategy_ms = (time.perf_counter() - t) * 1e3
    out = {"k": k, "clocks_before": clocks(), "circuit": "circuit-layout.rs shape (tools/proof_bench.py), SHPLONK, %d proof bytes" % len(proof),
           "verify_single_strategy_ms": median_ms(single, 5), "verify_no_strategy_python_integers_ms": round(no_strategy_ms, 3),
           "one_proof": accumulate(1), "sixteen_proofs": accumulate(16), "check_structure": {}}
    pk.close()
    params.close()
    for kk in (k, 20):
        with h2.ParamsKZG.setup(kk, pb.SECRET) as p:
            p.check_structure(b"\x22" * 32)  # warm-up: window tables, the resident copy of g
            timings = {}
            t = time.perf_counter()
            res = p.check_structure(b"\x22" * 32, timings)
            total = (time.perf_counter() - t) * 1e3
            assert res.ok, res
            out["check_structure"]["k%d" % kk] = dict({name: round(ms, 3) for name, ms in timings.items()}, total_ms=round(total, 3))
    out["clocks_after"] = clocks()
    return out


def main():
    h2 = load_pkg()
    kzg = importlib.import_module("halo2_pse_amd.kzg")
    args = sys.argv[1:]
    if "--host" in args:
        rec = {"host": host(h2, kzg)}
    else:
        k = int(args[args.index("--k") + 1]) if "--k" in args else 17
        rec = {"host_of_the_gpu_box": host(h2, kzg), "gpu": gpu(h2, kzg, k)}
    print(json.dumps(rec), flush=True)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
