"""Lookup compression and permutation (h2hip_lookup_compress_bn254 / h2hip_lookup_permute_bn254): the restatement in lookup_util.py
checked by identities of its own, then the engine against it limb for limb, and by the same identities where it is too slow."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import lookup_util as lu
import product_util as pu
from lookup_util import R_MOD


def _ev():
    import importlib
    return importlib.import_module("halo2_pse_amd.evaluation")


def check_identities(inp, table, pa, ps, u):
    """A' sorted; the multisets of A'[0..u) / S'[0..u) are the inputs'; every row has A'[i] = S'[i] or A'[i] = A'[i-1]"""
    assert all(pa[i] <= pa[i + 1] for i in range(u - 1))
    assert sorted(pa[:u]) == sorted(inp[:u])
    assert sorted(ps[:u]) == sorted(table[:u])
    assert all(pa[i] == ps[i] or (i > 0 and pa[i] == pa[i - 1]) for i in range(u))


def case_values(rng, kind, n, u):
    """(input, table) canonical integer columns of n rows"""
    if kind == "one":
        v = rng.randrange(R_MOD)
        return [v] * n, [v] * n
    if kind == "distinct":
        t = [rng.randrange(R_MOD) for _ in range(n)]
        inp = t[:u]
        rng.shuffle(inp)
        return inp + [rng.randrange(R_MOD) for _ in range(n - u)], t
    if kind == "repeats":  # the table has duplicates and unused values, the input draws from part of it with repeats
        vals = [rng.randrange(R_MOD) for _ in range(max(2, u // 3))]
        t = [rng.choice(vals) for _ in range(n)]
        used = t[:u][: max(1, u // 2)]
        return [rng.choice(used) for _ in range(n)], t
    if kind == "small":  # a 16-bit range check
        t = [i % (1 << 16) for i in range(n)]
        return [rng.randrange(min(u, 1 << 16)) for _ in range(n)], t
    if kind == "ends":  # 0 and r - 1
        vals = [0, R_MOD - 1, 1, R_MOD - 2]
        t = [vals[i % 4] for i in range(n)]
        return [rng.choice([0, R_MOD - 1]) for _ in range(n)], t
    if kind == "bit0":  # values differing only in bit 0
        base = rng.randrange(R_MOD >> 1) << 1
        t = [base | (i & 1) for i in range(n)]
        return [base | rng.randrange(2) for _ in range(n)], t
    if kind == "high200":  # distinct values sharing their top 200 bits
        hi = rng.randrange(R_MOD >> 54) << 54
        t = [hi | rng.randrange(1 << 54) for _ in range(n)]
        return [rng.choice(t[:u]) for _ in range(n)], t
    if kind == "low64":  # distinct values sharing their low 64 bits
        lo = rng.randrange(1 << 64)
        t = [(rng.randrange(R_MOD >> 64) << 64) | lo for _ in range(n)]
        return [rng.choice(t[:u]) for _ in range(n)], t
    raise ValueError(kind)


def make_case(seed, k, b, kinds):
    rng = random.Random(seed)
    n = 1 << k
    u = n - b - 1
    ins, tabs, blind, want = [], [], [], []
    for kind in kinds:
        inp, t = case_values(rng, kind, n, u)
        ba = [rng.randrange(R_MOD) for _ in range(b + 1)]
        bs = [rng.randrange(R_MOD) for _ in range(b + 1)]
        ins.append(inp)
        tabs.append(t)
        blind += ba + bs
        want.append(lu.permute(inp, t, u, ba, bs))
    return ins, tabs, blind, want


# ------------------------------------------------------------------ the restatement checks itself (CPU)
@pytest.mark.parametrize("kind", ["one", "distinct", "repeats", "small", "ends", "bit0", "high200", "low64"])
def test_restated_permutation_holds_the_identities(kind):
    k, b = 6, 3
    n, u = 1 << k, (1 << k) - b - 1
    ins, tabs, _, want = make_case(0x1000 + len(kind), k, b, [kind])
    pa, ps = want[0]
    assert len(pa) == len(ps) == n
    check_identities(ins[0], tabs[0], pa, ps, u)


def test_restated_leftovers_descend_over_the_repeated_rows():
    # input 1,1,1,2 over table 1,2,3,4: the repeated rows 1, 2 get the leftovers 3, 4 as 4, 3
    pa, ps = lu.permute([2, 1, 1, 1], [1, 2, 3, 4], 4, [], [])
    assert pa == [1, 1, 1, 2] and ps == [1, 4, 3, 2]
    with pytest.raises(lu.ConstraintSystemFailure):
        lu.permute([5, 1], [1, 2], 2, [], [])


def test_restated_compress_folds_with_theta():
    n, theta = 4, 7
    cols = {"fixed": [[1, 2, 3, 4]], "advice": [[5, 6, 7, 8]], "instance": []}
    got = lu.compress([("fixed", 0, 0), ("advice", 0, 1), ("const", 3)], theta, n, cols)
    assert got == [(1 * 49 + 6 * 7 + 3) % R_MOD, (2 * 49 + 7 * 7 + 3), (3 * 49 + 8 * 7 + 3), (4 * 49 + 5 * 7 + 3)]


def test_lookup_calls_without_gpu_fail_loudly(h2):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    k, n = 3, 8
    col = np.zeros((n, 4), dtype=np.uint64)
    with pytest.raises(h2.H2HipError):
        h2.lookup_permute(k, [col], [col], np.zeros((8, 4), np.uint64), 3)
    gi, gt = _ev().lookup_compress_graphs([("advice", 0, 0)], [("fixed", 0, 0)])
    with pytest.raises(h2.H2HipError):
        h2.lookup_compress(k, [_ev().flatten_graph(gi)], pu.fe(3), fixed=[col], advice=[col])


def test_lookup_calls_reject_bad_arguments(h2):
    """validation happens before any device work, so it answers the same with or without a GPU"""
    ev = _ev()
    k, n = 3, 8
    col = np.zeros((n, 4), dtype=np.uint64)
    bad = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    with pytest.raises(h2.H2HipError, match="rc=1"):  # b + 1 >= n
        h2.lookup_permute(k, [col], [col], np.zeros((16, 4), np.uint64), 7)
    with pytest.raises(h2.H2HipError, match="rc=1"):  # blinding not reduced
        h2.lookup_permute(k, [col], [col], np.stack([bad] * 8), 3)
    L = h2.lib()
    assert L.h2hip_lookup_permute_bn254(ctypes.c_uint32(29), None, None, ctypes.c_size_t(1), None, ctypes.c_uint32(0), None, None) == 1  # k > 28
    bl = lu.to_mont([0] * 8)
    cp = (ctypes.c_void_p * 1)(col.ctypes.data)
    for args in [(None, cp, cp, cp), (cp, None, cp, cp), (cp, cp, None, cp), (cp, cp, cp, None)]:  # a null column table, blinding valid
        assert L.h2hip_lookup_permute_bn254(ctypes.c_uint32(3), args[0], args[1], ctypes.c_size_t(1), h2._p(bl), ctypes.c_uint32(3), args[2],
                                            args[3]) == 1
    assert "null" in L.h2hip_last_error().decode()
    g_in, _ = ev.lookup_compress_graphs([("advice", 0, 0)], [("fixed", 0, 0)])
    flat = ev.flatten_graph(g_in)
    with pytest.raises(h2.H2HipError, match="rc=1"):  # advice column 0 of none
        h2.lookup_compress(k, [flat], pu.fe(3), fixed=[col])
    with pytest.raises(h2.H2HipError, match="rc=1"):  # theta not reduced
        h2.lookup_compress(k, [flat], bad, advice=[col])
    g = ev.GraphEvaluator()
    parts = (g.add_expression(("advice", 0, 0)),)
    g.add_calculation((ev.CALC_HORNER, (ev.VS_CONSTANT, 0, 0), (ev.VS_BETA, 0, 0), parts))  # beta has no place in a compression
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.lookup_compress(k, [ev.flatten_graph(g)], pu.fe(3), advice=[col])
    assert L.h2hip_lookup_permute_bn254(ctypes.c_uint32(3), None, None, ctypes.c_size_t(0), None, ctypes.c_uint32(3), None, None) == 0  # count == 0
    assert L.h2hip_lookup_compress_bn254(ctypes.c_uint32(3), None, 0, None, 0, None, 0, None, 0, h2._p(pu.fe(3)), None, ctypes.c_size_t(0), None) == 0
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.set_lookup_sort(3)


# ------------------------------------------------------------------ the engine against the restatement (GPU)
def run_permute(h2, k, b, ins, tabs, blind):
    return h2.lookup_permute(k, [lu.to_mont(c) for c in ins], [lu.to_mont(c) for c in tabs], lu.to_mont(blind), b)


def assert_permute(h2, k, b, ins, tabs, blind, want):
    pa, ps = run_permute(h2, k, b, ins, tabs, blind)
    for j, (wa, ws) in enumerate(want):
        assert np.array_equal(pa[j], lu.to_mont(wa)), "A' of lookup %d" % j
        assert np.array_equal(ps[j], lu.to_mont(ws)), "S' of lookup %d" % j


@pytest.mark.gpu
@pytest.mark.parametrize("k,b", [(3, 1), (4, 3), (10, 5), (12, 5), (17, 5), (20, 5)])
def test_permute_matches_reference(h2, k, b):
    kinds = ["repeats", "distinct", "one", "small"] if k < 20 else ["repeats", "small"]
    ins, tabs, blind, want = make_case(0x2000 + k, k, b, kinds)
    assert_permute(h2, k, b, ins, tabs, blind, want)
    assert h2.lookup_sort_stats() == (min(1024, 1 << k), max(0, k - 10))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ends", "bit0", "high200", "low64", "one", "distinct"])
def test_permute_exact_on_hard_keys(h2, kind):
    k, b = 11, 5
    ins, tabs, blind, want = make_case(0x3000 + len(kind), k, b, [kind, "repeats"])
    assert_permute(h2, k, b, ins, tabs, blind, want)
    assert h2.lookup_sort_stats() == (1024, 1)


@pytest.mark.gpu
def test_permute_orders_canonical_not_montgomery(h2):
    """inputs whose canonical and Montgomery-limb orders disagree: the engine must give the canonical A'"""
    k, b = 6, 3
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0x4000)
    t = [rng.randrange(R_MOD) for _ in range(n)]
    inp = t[:u]
    rng.shuffle(inp)
    inp += t[u:]
    assert sorted(inp[:u]) != sorted(inp[:u], key=lu.mont_int), "the case must tell the two orders apart"
    ba, bs = [1] * (b + 1), [2] * (b + 1)
    assert_permute(h2, k, b, [inp], [t], ba + bs, [lu.permute(inp, t, u, ba, bs)])


@pytest.mark.gpu
@pytest.mark.parametrize("block", [4, 16, 64, 256])
@pytest.mark.parametrize("kind", ["repeats", "distinct", "one", "small"])
def test_permute_forced_merge_passes(h2, block, kind):
    k, b = 10, 5
    ins, tabs, blind, want = make_case(0x5000 + block, k, b, [kind, "high200"])
    h2.set_lookup_sort(block)
    try:
        assert_permute(h2, k, b, ins, tabs, blind, want)
        assert h2.lookup_sort_stats() == (block, k - block.bit_length() + 1)
    finally:
        h2.set_lookup_sort(0)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "largest"])
def test_missing_value_is_elookup(h2, where):
    k, b = 8, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0x6000)
    t = sorted(rng.randrange(1, R_MOD - 1) for _ in range(n))
    inp = [rng.choice(t[:u]) for _ in range(n)]
    missing = {"first": 0, "middle": sorted(t[:u])[u // 2] + 1, "largest": R_MOD - 1}[where]
    assert missing not in t[:u]
    inp[rng.randrange(u)] = missing
    with pytest.raises(lu.ConstraintSystemFailure):
        lu.permute(inp, t, u, [], [])
    with pytest.raises(h2.H2HipLookupError, match="lookup 0"):
        run_permute(h2, k, b, [inp], [t], [0] * (2 * (b + 1)))


@pytest.mark.gpu
def test_only_lookup_one_fails(h2):
    k, b = 9, 5
    u = (1 << k) - b - 1
    ins, tabs, blind, _ = make_case(0x6100, k, b, ["repeats", "repeats", "small"])
    ins[1][3] = max(tabs[1][:u]) + 1
    with pytest.raises(h2.H2HipLookupError, match="lookup 1"):
        run_permute(h2, k, b, ins, tabs, blind)
    nb = 2 * (b + 1)
    for j in (0, 2):  # the others alone pass, and give the restatement's columns
        want = [lu.permute(ins[j], tabs[j], u, blind[j * nb:j * nb + b + 1], blind[j * nb + b + 1:(j + 1) * nb])]
        assert_permute(h2, k, b, [ins[j]], [tabs[j]], blind[j * nb:(j + 1) * nb], want)


@pytest.mark.gpu
def test_permute_k22_identities(h2, oracle):
    k, b = 22, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = np.random.default_rng(0x7000)
    tab = oracle.gen_scalars(0x7001, n, num_threads=8)
    idx = rng.integers(0, u, size=n)
    inp = tab[idx]
    pa, ps = h2.lookup_permute(k, [inp], [tab], np.zeros((2 * (b + 1), 4), np.uint64), b)
    pa, ps = pa[0], ps[0]
    ca, cs = oracle.fe_to_canonical(1, pa[:u]), oracle.fe_to_canonical(1, ps[:u])
    ctab_n = oracle.fe_to_canonical(1, tab)
    cin, ctab = ctab_n[idx[:u]], ctab_n[:u]
    order = np.lexsort(cin.T)  # limb 3 most significant: lexsort's last key is the primary one
    assert np.array_equal(ca, cin[order]), "A' is the canonical sort of the input"
    ord_s = np.lexsort(cs.T)
    assert np.array_equal(cs[ord_s], ctab[np.lexsort(ctab.T)]), "S' is a permutation of the table"
    same = np.all(ca == cs, axis=1)
    prev = np.concatenate([[False], np.all(ca[1:] == ca[:-1], axis=1)])
    assert np.all(same | prev)
    assert np.all(same[~prev]), "every first row takes its own value"


def compress_case(seed, k):
    rng = random.Random(seed)
    n = 1 << k
    cols = {"fixed": [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(2)],
            "advice": [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(3)],
            "instance": [[rng.randrange(R_MOD) for _ in range(n)]]}
    challenges = [rng.randrange(R_MOD) for _ in range(2)]
    return cols, challenges, rng.randrange(R_MOD)


COMPRESS_LOOKUPS = [
    # one expression each side, a bare column
    ([("advice", 0, 0)], [("fixed", 0, 0)]),
    # rotations -1 / +1 wrapping at rows 0 and n - 1, challenges, constants, Scaled, Negated, products
    ([("sum", ("advice", 1, -1), ("prod", ("challenge", 1), ("advice", 2, 1))), ("scaled", ("instance", 0, 0), 5),
      ("neg", ("prod", ("fixed", 1, 1), ("const", 9)))],
     [("fixed", 0, -1), ("sum", ("fixed", 1, 0), ("neg", ("advice", 0, 1))), ("prod", ("advice", 2, 0), ("advice", 2, 0))]),
    ([("advice", 0, 0), ("advice", 1, 0)], [("fixed", 0, 0), ("fixed", 1, 0)]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 10])
def test_compress_matches_reference(h2, k):
    ev = _ev()
    n = 1 << k
    cols, ch, theta = compress_case(0x8000 + k, k)
    graphs, want = [], []
    for inp, tab in COMPRESS_LOOKUPS:
        gi, gt = ev.lookup_compress_graphs(inp, tab)
        graphs += [ev.flatten_graph(gi), ev.flatten_graph(gt)]
        want += [lu.compress(inp, theta, n, cols, ch), lu.compress(tab, theta, n, cols, ch)]
    m = lambda cs: [lu.to_mont(c) for c in cs]  # noqa: E731
    got = h2.lookup_compress(k, graphs, pu.fe(theta), m(cols["fixed"]), m(cols["advice"]), m(cols["instance"]), lu.to_mont(ch))
    for g, (w, gr) in enumerate(zip(want, got)):
        assert np.array_equal(gr, lu.to_mont(w)), "graph %d" % g
    fixed = m(cols["fixed"])  # pinned and unpinned host forms agree
    h2.columns_pin(fixed)
    try:
        again = h2.lookup_compress(k, graphs, pu.fe(theta), fixed, m(cols["advice"]), m(cols["instance"]), lu.to_mont(ch))
    finally:
        h2.columns_unpin(fixed)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


@pytest.mark.gpu
def test_device_chain_feeds_lookup_products(h2):
    """device compress -> device permute -> h2hip_lookup_products_bn254_device equals the restated commit_product"""
    import torch
    ev = _ev()
    k, b = 12, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0x9000)
    f0 = [rng.randrange(R_MOD) for _ in range(n)]
    f1 = [rng.randrange(R_MOD) for _ in range(n)]
    f2 = [i % (1 << 16) for i in range(n)]
    rows = [rng.randrange(u) for _ in range(n)]
    a0, a1 = [f0[r] for r in rows], [f1[r] for r in rows]
    a2 = [rng.randrange(1 << 10) for _ in range(n)]
    cols = {"fixed": [f0, f1, f2], "advice": [a0, a1, a2], "instance": []}
    theta, beta, gamma = (rng.randrange(R_MOD) for _ in range(3))
    lookups = [([("advice", 0, 0), ("advice", 1, 0)], [("fixed", 0, 0), ("fixed", 1, 0)]), ([("advice", 2, 0)], [("fixed", 2, 0)])]
    graphs = []
    for inp, tab in lookups:
        gi, gt = ev.lookup_compress_graphs(inp, tab)
        graphs += [ev.flatten_graph(gi), ev.flatten_graph(gt)]
    blind = [rng.randrange(R_MOD) for _ in range(4 * (b + 1))]
    zbl = [rng.randrange(R_MOD) for _ in range(2 * b)]
    df = [_dev(lu.to_mont(c)) for c in cols["fixed"]]
    da = [_dev(lu.to_mont(c)) for c in cols["advice"]]
    dcomp = [torch.empty_like(df[0]) for _ in range(4)]
    dpa, dps, dz = ([torch.empty_like(df[0]) for _ in range(2)] for _ in range(3))
    h2.lookup_compress_device(k, graphs, pu.fe(theta), dcomp, df, da)
    h2.lookup_permute_device(k, dcomp[0::2], dcomp[1::2], lu.to_mont(blind), b, dpa, dps)
    h2.lookup_products_device(k, pu.fe(beta), pu.fe(gamma), dcomp[0::2], dcomp[1::2], dpa, dps, lu.to_mont(zbl), b, dz)
    torch.cuda.synchronize()
    for j, (inp, tab) in enumerate(lookups):
        ci, ct = lu.compress(inp, theta, n, cols), lu.compress(tab, theta, n, cols)
        wa, ws = lu.permute(ci, ct, u, blind[2 * j * (b + 1):(2 * j + 1) * (b + 1)], blind[(2 * j + 1) * (b + 1):(2 * j + 2) * (b + 1)])
        assert np.array_equal(h2.to_numpy_u64(dpa[j]), lu.to_mont(wa))
        assert np.array_equal(h2.to_numpy_u64(dps[j]), lu.to_mont(ws))
        wz = pu.lookup_commit(k, beta, gamma, ci, ct, wa, ws, zbl[j * b:(j + 1) * b], b)
        assert np.array_equal(h2.to_numpy_u64(dz[j]), lu.to_mont(wz))


@pytest.mark.gpu
def test_commit_permuted_commitments_match_oracle(h2, oracle):
    k, b = 8, 5
    n = 1 << k
    rng = random.Random(0xA000)
    t = [rng.randrange(R_MOD) for _ in range(n)]
    a = [rng.choice(t[:n - b - 1]) for _ in range(n)]
    params = h2.ParamsKZG.setup(k, 0x1234567)
    dom = h2.EvaluationDomain.new(3, k)
    blind = lu.to_mont([rng.randrange(R_MOD) for _ in range(2 * (b + 1))])
    out = h2.commit_permuted(params, dom, [([("advice", 0, 0)], [("fixed", 0, 0)])], pu.fe(5), blind, b, [pu.fe(1), pu.fe(2)],
                             fixed=[lu.to_mont(t)], advice=[lu.to_mont(a)])
    d = out[0]
    u = n - b - 1
    bl = lu.from_mont(blind)
    wa, ws = lu.permute(a, t, u, bl[:b + 1], bl[b + 1:])
    assert np.array_equal(d["compressed_input"], lu.to_mont(a)) and np.array_equal(d["compressed_table"], lu.to_mont(t))
    assert np.array_equal(d["permuted_input"], lu.to_mont(wa)), "A'"
    assert np.array_equal(d["permuted_table"], lu.to_mont(ws)), "S'"
    for col, com in (("permuted_input", "permuted_input_commitment"), ("permuted_table", "permuted_table_commitment")):
        want = oracle.g1_to_affine(oracle.best_multiexp(d[col], params.g_lagrange, 4))
        assert np.array_equal(h2.g1_to_affine(d[com]), want)
        assert np.array_equal(d[col + "_poly"], dom.lagrange_to_coeff(d[col]))
    params.close()


@pytest.mark.gpu
def test_device_call_on_a_side_stream_then_host_call(h2):
    import torch
    k, b = 12, 5
    ins, tabs, blind, want = make_case(0xB000, k, b, ["repeats", "distinct"])
    ins2, tabs2, blind2, want2 = make_case(0xB001, k, b, ["small"])
    din = [_dev(lu.to_mont(c)) for c in ins]
    dtab = [_dev(lu.to_mont(c)) for c in tabs]
    dpa, dps = [torch.empty_like(din[0]) for _ in ins], [torch.empty_like(din[0]) for _ in ins]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h2.lookup_permute_device(k, din, dtab, lu.to_mont(blind), b, dpa, dps)
    assert_permute(h2, k, b, ins2, tabs2, blind2, want2)  # host form on the engine's stream, at once
    side.synchronize()
    for j, (wa, ws) in enumerate(want):
        assert np.array_equal(h2.to_numpy_u64(dpa[j]), lu.to_mont(wa))
        assert np.array_equal(h2.to_numpy_u64(dps[j]), lu.to_mont(ws))


@pytest.mark.gpu
def test_compress_device_on_a_side_stream_then_host_compress(h2):
    """the device compress returns with its kernel still queued on a side stream; a host compress at once must not overtake it in the
    shared metadata workspace"""
    import torch
    ev = _ev()
    k = 12
    n = 1 << k
    cols, ch, theta = compress_case(0xC000, k)
    cols2, ch2, theta2 = compress_case(0xC001, k)
    graphs, want, graphs2, want2 = [], [], [], []
    for inp, tab in COMPRESS_LOOKUPS:
        gi, gt = ev.lookup_compress_graphs(inp, tab)
        graphs += [ev.flatten_graph(gi), ev.flatten_graph(gt)]
        want += [lu.compress(inp, theta, n, cols, ch), lu.compress(tab, theta, n, cols, ch)]
    gi, gt = ev.lookup_compress_graphs(*COMPRESS_LOOKUPS[2])
    graphs2 = [ev.flatten_graph(gi), ev.flatten_graph(gt)]
    want2 = [lu.compress(COMPRESS_LOOKUPS[2][0], theta2, n, cols2, ch2), lu.compress(COMPRESS_LOOKUPS[2][1], theta2, n, cols2, ch2)]
    m = lambda cs: [lu.to_mont(c) for c in cs]  # noqa: E731
    df, da, di = ([_dev(c) for c in m(cols[key])] for key in ("fixed", "advice", "instance"))
    dout = [torch.empty_like(df[0]) for _ in graphs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h2.lookup_compress_device(k, graphs, pu.fe(theta), dout, df, da, di, lu.to_mont(ch))
    got2 = h2.lookup_compress(k, graphs2, pu.fe(theta2), m(cols2["fixed"]), m(cols2["advice"]), m(cols2["instance"]), lu.to_mont(ch2))
    side.synchronize()
    for g, w in zip(got2, want2):
        assert np.array_equal(g, lu.to_mont(w))
    for g, (d, w) in enumerate(zip(dout, want)):
        assert np.array_equal(h2.to_numpy_u64(d), lu.to_mont(w)), "graph %d" % g


# ------------------------------------------------------------------ the C++ mirror (GPU)
@pytest.mark.gpu
def test_cpp_mirror_lookups(tmp_path):
    """tests/cpp/test_lookup_mirror runs a tuple and a range lookup through host/halo2hip.hpp; its columns against the restatement"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_lookup_mirror")
    k, b = 10, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0xCD)
    f0, f1 = ([rng.randrange(R_MOD) for _ in range(n)] for _ in range(2))
    f2 = [i % (1 << 16) for i in range(n)]
    rows = [rng.randrange(u) for _ in range(n)]
    a0, a1 = [f0[r] for r in rows], [f1[r] for r in rows]
    a2 = [rng.randrange(1 << 9) for _ in range(n)]
    theta = rng.randrange(R_MOD)
    blind = [rng.randrange(R_MOD) for _ in range(4 * (b + 1))]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    blob = [np.array([k, b], dtype=np.uint64), lu.to_mont([theta]).reshape(-1)]
    blob += [lu.to_mont(c).reshape(-1) for c in (f0, f1, f2, a0, a1, a2)] + [lu.to_mont(blind).reshape(-1)]
    np.concatenate(blob).astype(np.uint64).tofile(inp)
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=120)
    got = np.fromfile(outp, dtype=np.uint64).reshape(-1, n, 4)
    cols = {"fixed": [f0, f1, f2], "advice": [a0, a1, a2], "instance": []}
    lookups = [([("advice", 0, 0), ("advice", 1, 0)], [("fixed", 0, 0), ("fixed", 1, 0)]), ([("advice", 2, 0)], [("fixed", 2, 0)])]
    want = []
    nb = 2 * (b + 1)
    for j, (li, lt) in enumerate(lookups):
        ci, ct = lu.compress(li, theta, n, cols), lu.compress(lt, theta, n, cols)
        wa, ws = lu.permute(ci, ct, u, blind[j * nb:j * nb + b + 1], blind[j * nb + b + 1:(j + 1) * nb])
        want += [ci, ct, wa, ws]
    assert got.shape[0] == len(want)
    for q, w in enumerate(want):
        assert np.array_equal(got[q], lu.to_mont(w)), "column %d" % q
