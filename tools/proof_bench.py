#!/usr/bin/python3
"""create_proof + verify_proof on the column and gate structure of examples/circuit-layout.rs (BASELINE.json configs[4]) at k = 17:
advice e, a, b, c, d; fixed sf, sm, sa, sb, sc and the lookup table sl; one gate a sa + b sb + a b sm - c sc + sf d(+1) e(-1); the
lookup [a] in [sl]; equality on a, b, c.  The witness satisfies it by construction: sm = sc = 1 on the usable rows (c = a b), every
other selector zero, a drawn from the table, every odd row's a copied from the even row before it on the first 128 rows.

Reports the median of 5 of create_proof with resident columns and from host columns, parts and full form, both multiopen schemes for the
resident parts form; the engine's per-stage times of one profiled proof (profile_get); and what the prover moved (proof.transfers).
Every proof is verified once (Python integers; the pairing equation closed with the setup secret).
  python tools/proof_bench.py [--k K] [--reps N]     (run on the GPU box)

--arguments measures the later arguments instead: the same circuit with an mv-lookup (logUp) [a] in [sl] in place of its halo2 lookup
and one shuffle e <-> d (d holds e's usable rows in reverse), resident and host columns, parts form, SHPLONK, beside the lookup
circuit's same two legs in the same process (the comparison row), each with its stage times and transfer sums.

--multiopen ipa measures the same circuit over the IPA commitment scheme (ipa.ParamsIPA.new(k), the key built over it, multiopen="ipa",
every proof verified by ipa.SingleStrategy -- no secret) with resident and host columns, parts form, beside the SHPLONK proof of the
same circuit with resident columns in the same process: the like-for-like pair."""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
SECRET = 0x5EC2E7
STAGES = ("msm_total", "ntt_batch", "lookup_compress", "lookup_permute", "products", "evalh_cosets", "evalh_part_scale", "evalh_part_io",
          "evalh_gates", "evalh_gates_gen", "evalh_perm", "evalh_lookups", "evalh_lookup_gen", "eval_polynomials", "opening_eval", "opening_combine",
          "mvlookup_multiplicities", "mvlookup_sums", "evalh_mvlookups", "evalh_mvlookup_gen", "evalh_shuffles",
          "evalh_shuffle_gen", "ipa_collapse", "ipa_normalize", "ipa_fold",
          "ipa_inner_products")  # "products": the one timer of the permutation, lookup and shuffle grand products


def to_mont(vals):
    m = (1 << 256) % R
    raw = b"".join(((int(v) % R) * m % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def g1_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return (x, (lam * (p[0] - x) - p[1]) % Q)


def g1_mul(p, k):
    acc = None
    for bit in bin(k % R)[2:]:
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, p)
    return acc


def circuit(prover, arguments=False):
    A = lambda c, r=0: ("advice", c, r)  # noqa: E731
    F = lambda c, r=0: ("fixed", c, r)  # noqa: E731
    e_, a_, b_, c_, d_ = range(5)
    sf, sm, sa, sb, sc, sl = range(6)
    gate = ("sum", ("sum", ("sum", ("sum", ("prod", A(a_), F(sa)), ("prod", A(b_), F(sb))), ("prod", ("prod", A(a_), A(b_)), F(sm))),
                    ("neg", ("prod", A(c_), F(sc)))), ("prod", F(sf), ("prod", A(d_, 1), A(e_, -1))))
    permutation = [("advice", a_), ("advice", b_), ("advice", c_)]
    if arguments:
        return prover.ConstraintSystem(6, 5, 0, [gate], [], permutation, mv_lookups=[([[A(a_)]], [F(sl)])], shuffles=[([A(e_)], [A(d_)])])
    return prover.ConstraintSystem(6, 5, 0, [gate], [([A(a_)], [F(sl)])], permutation)


def assignment(k, b, seed=17, arguments=False):
    rng = random.Random(seed)
    n, u = 1 << k, (1 << k) - b - 1
    rnd = lambda: rng.randrange(R)  # noqa: E731
    table = [rnd() for _ in range(n)]
    a = [rng.choice(table[:u]) for _ in range(n)]
    copies = []
    for j in range(64):
        a[2 * j + 1] = a[2 * j]
        copies.append((0, 2 * j, 0, 2 * j + 1))
    bb = [rnd() for _ in range(n)]
    c = [x * y % R for x, y in zip(a, bb)]
    on = [1 if i < u else 0 for i in range(n)]
    zero = [0] * n
    fixed = [zero, on, zero, zero, on, table]  # sf, sm, sa, sb, sc, sl
    advice = [[rnd() for _ in range(n)], a, bb, c, [rnd() for _ in range(n)]]  # e, a, b, c, d
    if arguments:  # d: a shuffle of e's usable rows (sf = 0: the gate reads neither)
        advice[4][:u] = advice[0][:u][::-1]
    return [to_mont(col) for col in fixed], [to_mont(col) for col in advice], copies


ALL_LEGS = ((True, "parts", "shplonk"), (True, "full", "shplonk"), (True, "parts", "gwc"), (False, "parts", "shplonk"), (False, "full", "shplonk"))
ARGUMENT_LEGS = ((True, "parts", "shplonk"), (False, "parts", "shplonk"))
IPA_LEGS = ((True, "parts", "ipa"), (False, "parts", "ipa"))


def measure(mods, k, reps, arguments, legs, ipa=None):
    """one circuit: its key, the median of `reps` proofs per leg (each leg's proof verified, the legs' bytes compared), and the stage
    times of one profiled proof with resident and with host columns (parts form; SHPLONK, or IPA when `ipa` is the ipa module and the
    legs are IPA's)"""
    import torch
    h2, prover, verifier, tr = mods
    cs = circuit(prover, arguments)
    t0 = time.perf_counter()
    fixed, advice, copies = assignment(k, cs.blinding_factors(), arguments=arguments)
    params = ipa.ParamsIPA.new(k) if ipa else h2.ParamsKZG.setup(k, SECRET)
    pk = prover.ProvingKey.build(params, cs, fixed, copies, 0x17)
    setup_s = time.perf_counter() - t0
    d_advice = [torch.from_numpy(a.view(np.int64)).cuda() for a in advice]

    def prove(resident, form, multiopen):
        # fresh columns: the prover consumes them (the copies are outside the clock)
        cols = [c.clone() for c in d_advice] if resident else [c.copy() for c in advice]
        torch.cuda.synchronize()
        t = time.perf_counter()
        proof = prover.create_proof(params, pk, [[]], lambda i, phase, ch: cols, tr.Blake2bWrite(), b"\x11" * 32, multiopen=multiopen, form=form,
                                    resident=resident)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, proof

    out = {"degree": cs.degree(), "extended_k": pk.domain.extended_k, "setup_s": round(setup_s, 2), "legs": {}}
    reference_bytes = {}
    for resident, form, multiopen in legs:
        prove(resident, form, multiopen)  # warm-up: kernel generation, window tables, arenas
        ts, proof = [], None
        for _ in range(reps):
            ms, proof = prove(resident, form, multiopen)
            ts.append(ms)
        t_verify = time.perf_counter()
        if ipa:  # SingleStrategy raises unless the opening's MSM is the identity
            verifier.verify_proof(params, pk.vk, [[]], tr.Blake2bRead(proof.bytes), multiopen, strategy=ipa.SingleStrategy(params))
        else:
            left, right = verifier.verify_proof(params, pk.vk, [[]], tr.Blake2bRead(proof.bytes), multiopen)
            assert g1_mul(left, SECRET) == right, "the verifier rejects the proof"
        verify_ms = (time.perf_counter() - t_verify) * 1e3
        assert reference_bytes.setdefault(multiopen, proof.bytes) == proof.bytes, "the legs' proofs differ"
        name = "%s_%s_%s" % ("resident" if resident else "host", form, multiopen)
        out["legs"][name] = {"ms": round(sorted(ts)[len(ts) // 2], 3), "reps_ms": [round(t, 3) for t in ts], "proof_bytes": len(proof.bytes),
                             "h2d_bytes": proof.total("h2d"), "d2h_bytes": proof.total("d2h"),
                             "largest_transfer": max(proof.transfers, key=lambda t: t[1]), "verify_ms": round(verify_ms, 3)}
    scheme = "ipa" if ipa else "shplonk"
    h2.profile_enable(True)
    for resident in sorted({resident for resident, _, _ in legs}, reverse=True):
        h2.profile_reset()
        prove(resident, "parts", scheme)
        stages = {}
        for s in STAGES:
            try:
                ms, cnt = h2.profile_get(s)
            except h2.H2HipError:
                continue
            if cnt:
                stages[s] = {"ms": round(ms, 4), "count": cnt}
        out["stages_%s_parts_%s" % ("resident" if resident else "host", scheme)] = stages
    h2.profile_enable(False)
    pk.close()
    if ipa:
        params.close()
    return out


def main():
    import importlib
    args = sys.argv[1:]
    k = int(args[args.index("--k") + 1]) if "--k" in args else 17
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    h2 = load_pkg()
    h2.init()
    mods = (h2,) + tuple(importlib.import_module("halo2_pse_amd." + m) for m in ("prover", "verifier", "transcript"))
    out = {"k": k, "reps": reps, "stat": "median, host clock around create_proof, stream synchronised"}
    if "--multiopen" in args:
        if args[args.index("--multiopen") + 1] != "ipa":
            raise SystemExit("--multiopen ipa (the KZG schemes are the default run's legs)")
        ipa = importlib.import_module("halo2_pse_amd.ipa")
        out["circuits"] = {"shplonk": measure(mods, k, reps, False, ((True, "parts", "shplonk"),)),
                           "ipa": measure(mods, k, reps, False, IPA_LEGS, ipa=ipa)}
    elif "--arguments" in args:
        out["circuits"] = {name: measure(mods, k, reps, arguments, ARGUMENT_LEGS) for name, arguments in (("lookup", False), ("mvlookup_shuffle", True))}
    else:
        res = measure(mods, k, reps, False, ALL_LEGS)
        out["circuit"] = "circuit-layout.rs shape: 5 advice, 6 fixed, 1 gate, 1 lookup, 3 permutation columns (2 sets)"
        out.update({key: val for key, val in res.items() if key not in ("degree", "extended_k")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
