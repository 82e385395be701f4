"""Wall clock of the host-pointer legs of the stage files' forms at k = 16 (median of 9 blocking calls after 2 warm-ups, one line of json to
the file named on the command line).  One process measures one library: HALO2_HIP_LIB names another build, so two builds are compared
by alternating processes on one box."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

h2 = load_pkg()
h2.init(0)
import evalh_util as ev  # noqa: E402
import product_util as pu  # noqa: E402

K, BF, REPS, WARM = 16, 5, 9, 2
n = 1 << K
rng = np.random.default_rng(1)


def fes(m):
    a = rng.integers(0, 1 << 63, size=(m, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(4)
    return a


def cols(m):
    return [fes(n) for _ in range(m)]


def timed(f):
    for _ in range(WARM):
        f()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * sorted(t)[len(t) // 2]


res = {}
omega = pu.fe(pu.root_of_unity(K))
c6, p6, bl2 = cols(6), cols(6), fes(2 * BF)
res["permutation_products"] = timed(lambda: h2.permutation_products(K, omega, fes(1)[0], fes(1)[0], fes(1)[0], c6, p6, 3, bl2, BF))
a, s, ap, sp = cols(2), cols(2), cols(2), cols(2)
res["lookup_products"] = timed(lambda: h2.lookup_products(K, fes(1)[0], fes(1)[0], a, s, ap, sp, bl2, BF))
res["shuffle_products"] = timed(lambda: h2.shuffle_products(K, fes(1)[0], a, s, bl2, BF))
tabs = cols(2)
ins = [t[rng.integers(0, n - BF - 1, size=n)].copy() for t in tabs]
res["lookup_permute"] = timed(lambda: h2.lookup_permute(K, ins, tabs, fes(2 * 2 * (BF + 1)), BF))
mv_in = [[ins[0]], [ins[1], ins[1].copy()]]
res["mvlookup_multiplicities"] = timed(lambda: h2.mvlookup_multiplicities(K, mv_in, tabs, BF))
m = h2.mvlookup_multiplicities(K, mv_in, tabs, BF)
res["mvlookup_sums"] = timed(lambda: h2.mvlookup_sums(K, fes(1)[0], mv_in, tabs, m, bl2, BF))
inv = fes(1 << 18)
res["batch_invert"] = timed(lambda: h2.batch_invert(inv))
graphs = [ev.flatten_graph(g) for g in ev.lookup_compress_graphs([("advice", 0, 0), ("fixed", 1, 0)], [("fixed", 0, 0), ("advice", 1, 0)])]
fx, ad = cols(2), cols(2)
res["lookup_compress"] = timed(lambda: h2.lookup_compress(K, graphs, fes(1)[0], fx, ad))
gates = [ev.flatten_graph(g) for g in ev.gate_check_graphs([("sum", ("advice", 0, 0), ("neg", ("fixed", 0, 0)))])]
res["check_gates"] = timed(lambda: h2.check_gates(K, gates, fx, ad))
res["check_lookups"] = timed(lambda: h2.check_lookups(K, ins, tabs, BF))
res["check_shuffles"] = timed(lambda: h2.check_shuffles(K, ins, tabs, BF))
mp = np.zeros((3, n, 2), dtype=np.uint32)
mp[:, :, 0] = np.arange(3)[:, None]
mp[:, :, 1] = np.arange(n)[None, :]
c3 = cols(3)
res["check_permutation"] = timed(lambda: h2.check_permutation(K, c3, mp))
pts = fes(8)
res["eval_polynomials"] = timed(lambda: h2.eval_polynomials(c6[:4], [0, 1, 2, 3, 0, 1, 2, 3], pts))
sc4, roots = fes(4), fes(1)
res["poly_combine"] = timed(lambda: h2.poly_combine(c6[:4], sc4, roots=roots))
copies = np.stack([rng.integers(0, 3, n), rng.integers(0, n, n), rng.integers(0, 3, n), rng.integers(0, n, n)], axis=1).astype(np.uint32)
res["permutation_mapping"] = timed(lambda: h2.permutation_mapping(K, 3, copies))
res["fr_to_repr"] = timed(lambda: h2.fr_to_repr(inv))
res["fr_random"] = timed(lambda: h2.fr_random(bytes(range(32)), 1 << 18))
dom = h2.EvaluationDomain.new(4, K)
res["key_lagrange_columns"] = timed(lambda: h2.key_lagrange_columns(dom, BF))
res["permutation_keygen"] = timed(lambda: h2.permutation_keygen(dom, mp))
rows = [np.arange(0, n, 7, dtype=np.uint32)] * 3
dens = [fes(len(rows[0]))] * 3
res["batch_invert_assigned"] = timed(lambda: h2.batch_invert_assigned(K, c3, rows, dens))
with open(sys.argv[1], "w") as f:
    json.dump(res, f)
print(sys.argv[1], " ".join("%s=%.3f" % kv for kv in res.items()), flush=True)
