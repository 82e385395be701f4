"""evaluate_h and the kernels that share its interpreter at their magnitude bounds.

The kernels of csrc/evalh.hip run on the lazily reduced 9 x 29-bit multiplier of csrc/fieldu.h; their correctness rests on magnitudes
that compile_graph tracks statically (a reduction requested where a value would pass 100 r, a closing one where the result would pass
15 r), on the bracketed figures in the comments of evalh_perm_kernel and lookup_row, and on the fused two-product reduction of the
generated kernel.  Every other test feeds them uniformly random elements, which sit near r / 2.  The corpus of evalh_edge_util.py puts
columns at r - 1, drives sums to the limit and results to +-15 r, cancels to multiples of r in front of out_e and saturates the limbs.

Unmarked: the corpus itself (every family compiles to the program its docstring aims at), the Python-integer evaluator against the
oracle, and tests/cpp/test_evalh_bounds.cpp -- both legs of every program and the permutation / lookup rows on the host under
-DH2_FU_CHECK, every bound asserted.  GPU: the same graphs and inputs through evaluate_h (interpreter, generated kernel, generated
without fusion, the global-workspace tier), evaluate_h_parts, lookup_compress and check_gates, limb for limb against the oracle or Python
integers.  No tolerance is involved anywhere."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import evalh_edge_util as U
import ntt_edge_util as eu
from conftest import ROOT
from evalh_util import DescHolder, PartsDescHolder, flatten_graph
from product_util import R_MOD
from test_evalh import _compile_stats, _codegen, gates_kernel  # noqa: F401  (the fixture)

FLAT = {name: flatten_graph(g) for name, g in U.families()}
NAMED = [name for name, _ in U.named_families()]
GPU_SCENARIOS = U.SCENARIOS  # every scenario: a call at k = 5 is milliseconds


def _lookup_flats():
    """the two lookup arguments of test_evalh._random_case"""
    from evalh_util import lookup_graph
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    return [flatten_graph(lookup_graph([A(li), ('prod', A(li + 1), F(li))], [F(5), F(li + 2, 1)])) for li in range(2)]


LOOKUPS = _lookup_flats()


# ------------------------------------------------------------------------------------------------- CPU: the corpus itself
def test_values_saturate_the_i_form_operand():
    for name in ("sat32", "sat32top"):
        limbs = U.i_form_limbs(U.VALUES[name])
        assert limbs[0] == (1 << 29) - 32 and limbs[1:8] == [(1 << 29) - 1] * 7, name
    assert U.i_form_limbs(U.VALUES["sat32"])[8] == 0 and U.i_form_limbs(U.VALUES["sat32top"])[8] == U.SAT_TOP
    assert set(eu.VALUES.values()) < set(U.VALUES.values()) and len(U.VALUES) == len(eu.VALUES) + 2
    assert set(eu.ints(U.extremes(1 << 10, 1))) == set(U.VALUES.values())
    for sc in U.SCENARIOS:
        cols = U.scenario_columns(sc, 32)
        for key in ("fixed", "advice", "instance"):
            assert all(c.shape == (32, 4) and eu.below_r(c).all() for c in cols[key]), sc
        if sc[0] != "random":
            assert eu.ints(cols["y"]) == [R_MOD - 1] and set(eu.ints(cols["challenges"])) == {R_MOD - 1}
    part = U.scenario_columns(("partial", 3), 32)
    a = [eu.ints(c) for c in part["advice"]]
    assert a[2][0::2] == a[1][0::2] and a[3][0::2] == a[0][0::2] and a[2][1::2] != a[1][1::2]


def _flags(prog, kind):
    return [bool(o[0] & U.OP_REDUCE_FLAG) for o in prog["ops"] if o[0] & 0xFF == kind]


def test_families_compile_to_the_programs_they_aim_at(h2):
    """the hook h2hip_debug_evalh_program on every family: where the reduce flags fall, which results take the closing MOV|REDUCE, what
    the generator fuses -- the properties the docstrings of evalh_edge_util's builders state"""
    P = {name: U.compiled_program(h2, flat) for name, flat in FLAT.items()}
    for name, p in P.items():
        n = len(p["ops"])
        assert p["mags"].shape == (n,) and p["fused_on"].shape == (n,) and (p["fused_off"] == -1).all(), name
        assert _compile_stats(h2, FLAT[name]) == (n, p["n_slots"]), name
        assert (p["mags"] <= U.MAG_LIMIT).all() and (p["mags"] > 0).all(), name
        # a product's tracked magnitude is at most 100 * 100 / 169 + 1: the compiler never flags one
        assert not any(_flags(p, U.OP_MUL)) and not any(_flags(p, U.OP_SQR)), name
        if p["result"][0] == U.VS_INTERMEDIATE and n:
            last = [i for i in range(n) if p["ops"][i][1] == p["result"][1]][-1]
            assert p["mags"][last] <= U.MAG_RESULT, name
        for i, j in enumerate(p["fused_on"]):
            if j >= 0:
                assert p["ops"][i][0] == U.OP_MUL and i < j < n and p["ops"][j][0] & 0xFF in (U.OP_ADD, U.OP_SUB, U.OP_FMA), (name, i)
    closing = lambda p: len(p["ops"]) and p["ops"][-1][0] == (U.OP_MOV | U.OP_REDUCE_FLAG)  # noqa: E731
    # 1. sum chains: the fourth column brings 128 > 100
    assert P["sum1"]["result"][0] == U.VS_ADVICE and len(P["sum1"]["ops"]) == 0
    assert _flags(P["sum3"], U.OP_ADD) == [False, False] and _flags(P["sum4"], U.OP_ADD) == [False, False, True]
    assert sum(_flags(P["sum8"], U.OP_ADD)) == 2 and closing(P["sum7"])
    # 2. doubling chains
    assert _flags(P["dbl2"], U.OP_DBL) == [False, True] and closing(P["dbl1"])
    # 3. [96] x [96]
    for name in ("wide_mul", "wide_sqr"):
        assert 55.5 < max(P[name]["mags"][[o[0] in (U.OP_MUL, U.OP_SQR) for o in P[name]["ops"]]]) < 55.6 and closing(P[name])
    # 4. negative extremes
    assert _flags(P["subchain4"], U.OP_SUB) == [False, False, False, True] and closing(P["0-sum3"])
    assert [int(o[0]) for o in P["neg_product"]["ops"]] == [U.OP_MUL, U.OP_NEG] and 7 < P["neg_product"]["mags"][-1] < 7.1
    # 5. just under and just over 15
    assert 14.1 < P["products2"]["mags"][-1] < 14.2 and not closing(P["products2"])
    assert closing(P["products3"]) and 21.1 < P["products3"]["mags"][-2] < 21.3
    # 6. Horner over a column with unreduced parts: a reduction requested on an FMA
    assert len(_flags(P["horner6"], U.OP_FMA)) == 6 and sum(_flags(P["horner6"], U.OP_FMA)) == 3 and not any(_flags(P["horner1"], U.OP_FMA))
    # 7. what the generator fuses
    for name in ("fuse_add", "fuse_sub", "fuse_add96", "fuse_sub96", "id_ab-ba"):
        p = P[name]
        readers = set(int(j) for j in p["fused_on"] if j >= 0)
        assert len(readers) == 1 and list(p["fused_on"]).count(readers.pop()) == 2, name
    for name in ("fuse_add96", "fuse_sub96"):
        assert P[name]["ops"][-1][0] & U.OP_REDUCE_FLAG, "the fused sum itself carries the reduction request"
    assert [int(P["fuse_horner"]["ops"][j][0]) for j in P["fuse_horner"]["fused_on"] if j >= 0] == [U.OP_FMA, U.OP_FMA]
    # 11. one graph per slot tier; 12. random graphs that keep a program
    for n_live in (2, 6, 12, 40, 100):
        assert n_live <= P["live%d" % n_live]["n_slots"] <= n_live + 2
    assert all(len(P[name]["ops"]) >= 12 for name, _ in U.random_families())
    kinds = set(int(o[0]) & 0xFF for p in P.values() for o in p["ops"])
    assert kinds == set(range(8))
    assert set(U.GENERATED) <= set(NAMED) and all(P[name]["n_slots"] <= 48 for name in U.GENERATED)
    # the emitted source follows the plan: one fu_mul_sub per fused reader, none with the plan empty
    for name in ("fuse_add", "fuse_horner", "products3", "sum8"):
        src, _, _ = _codegen(h2, FLAT[name], compile_it=False)
        assert src.count("fu_mul_sub<UF>") == len(set(int(j) for j in P[name]["fused_on"] if j >= 0)), name


def test_program_hook_rejects_and_sizes(h2):
    from evalh_util import graph_struct
    L = h2.lib()
    keep = []
    G = graph_struct(FLAT["products3"], keep)
    n_ops, n_slots, res = ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 3)()
    assert L.h2hip_debug_evalh_program(None, None, ctypes.c_size_t(0), ctypes.byref(n_ops), ctypes.byref(n_slots), res, None, None, None) == 1
    assert L.h2hip_debug_evalh_program(ctypes.byref(G), None, ctypes.c_size_t(0), ctypes.byref(n_ops), ctypes.byref(n_slots), res, None, None, None) == 0
    assert (n_ops.value, n_slots.value) == _compile_stats(h2, FLAT["products3"]) and tuple(res)[0] == U.VS_INTERMEDIATE
    bad = dict(FLAT["products3"], calcs=FLAT["products3"]["calcs"].copy())
    bad["calcs"][0, 1] = 10_000
    G = graph_struct(bad, keep)
    assert L.h2hip_debug_evalh_program(ctypes.byref(G), None, ctypes.c_size_t(0), ctypes.byref(n_ops), ctypes.byref(n_slots), res, None, None, None) == 1


def _gates_only(oracle, k, sc, flat):
    case, vin = U.system(oracle, 4, k, sc, (1, 1, 1), flat, [])
    case["perm_product_cosets"], case["perm_cosets"] = [], []
    case["perm_column_kind"] = case["perm_column_index"] = np.zeros(0, dtype=np.uint32)
    return case, vin


def _cosets_of(oracle, case):
    """the operands of a full-form case as rows of the extended domain, for eval_graph_ints"""
    d, _ = oracle.domain_new(4, case["k"])
    ext = lambda p: oracle.coeff_to_extended(d, p.copy(), 2)  # noqa: E731
    return {"fixed": case["fixed_cosets"], "advice": [ext(p) for p in case["advice_polys"]], "instance": [ext(p) for p in case["instance_polys"]],
            "challenges": case["challenges"], "beta": case["beta"], "gamma": case["gamma"], "theta": case["theta"], "y": case["y"]}


def _oracle_h(oracle, case, vin):
    want = vin.copy()
    h = DescHolder(case)  # named: the holder owns the pointer tables the call reads
    assert oracle.lib().oracle_evaluate_h(h.byref(), want.ctypes.data_as(ctypes.c_void_p)) == 0
    return want


@pytest.mark.parametrize("sc", [("const", "r-1"), ("extremes", 1), ("random", 5)], ids=U.scenario_id)
def test_python_integers_equal_the_oracle(oracle, sc):
    """eval_graph_ints, the reference of the row-graph tests and of the cancelling identities, against the oracle's evaluate_h on
    systems of gates alone: every family, rotations scaled to the extended domain, constant polynomials as constant cosets"""
    k = 3
    for name, flat in FLAT.items():
        case, vin = _gates_only(oracle, k, sc, flat)
        cols = _cosets_of(oracle, case)
        if sc[0] != "random":
            assert all(len(set(eu.ints(c))) == 1 for c in cols["advice"][:-1]), "a constant polynomial's coset is its word on every row"
        got = U.eval_graph_ints(flat, cols, 1 << case["extended_k"], previous=vin, rot_scale=4)
        assert np.array_equal(got, _oracle_h(oracle, case, vin)), (name, sc)
        if name[3:] in U.IDENTITIES or (name == "id_abcd" and sc[0] == "const"):
            assert not got.any(), name


def test_evalh_bounds_host(h2, tmp_path):
    """tests/cpp/test_evalh_bounds.cpp over the whole corpus (every family under every scenario, 32 rows each): the interpreter's and
    the generated kernel's statements with fieldu.h's own functions, every tracked magnitude, bracketed figure and operand contract
    asserted, and the counts that keep it from passing vacuously; prints the maxima DESIGN.md records"""
    corpus = str(tmp_path / "corpus.bin")
    n_records = U.write_corpus(corpus, h2)
    assert n_records == (len(FLAT) + 2) * len(U.SCENARIOS)
    src = os.path.join(ROOT, "tests", "cpp", "test_evalh_bounds.cpp")
    exe = str(tmp_path / "test_evalh_bounds")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DH2_FU_CHECK", "-Wno-unknown-pragmas", "-o", exe, src])
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "evalh bounds ok" in r.stdout and "%d records" % n_records in r.stdout
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("statement ")]) == 18 + 10
    # a tracked magnitude that is too small must be noticed: halve those of one record and the program fails on it
    prog = U.compiled_program(h2, FLAT["wide_mul"])
    prog["mags"] = prog["mags"] / 2
    with open(corpus, "wb") as fh:
        fh.write(U._u32(U.CORPUS_MAGIC, 1, len(U.VALUES)) + eu.words(list(U.VALUES.values())).tobytes())
        fh.write(U.corpus_record("halved", FLAT["wide_mul"], prog, U.scenario_columns(("const", "r-1"), 32), 5))
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "abs_le(out, R.mags[q])" in r.stdout and "halved" in r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU
def _run_full(h2, case, vin, tag):
    got = vin.copy()
    h = DescHolder(case)
    rc = h2.lib().h2hip_evaluate_h_bn254(h.byref(), got.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (tag, h2.lib().h2hip_last_error())
    eu.assert_below_r(got, tag)
    return got


def _ek_above_lo_bits(h2, oracle):
    """the smallest k whose EXTENDED domain (extended_k = k + 2) has rows at or beyond the power table's low bits: there the
    permutation kernel takes the second factor pow_hi"""
    h2.init()
    bits = ctypes.c_uint32()
    d, _ = oracle.domain_new(4, 18)
    assert h2.lib().h2hip_debug_evalh_power_table_bits(d.fe("extended_omega").ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(20), ctypes.byref(bits)) == 0
    k = bits.value + 1 - 2
    dk, _ = oracle.domain_new(4, k)
    assert h2.lib().h2hip_debug_evalh_power_table_bits(dk.fe("extended_omega").ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(k + 2), ctypes.byref(bits)) == 0
    assert bits.value < k + 2 <= 14
    return k


def _layout(i):
    return U.PERM_LAYOUTS[i % len(U.PERM_LAYOUTS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", U.GENERATED)
def test_gpu_evaluate_h_named_families(h2, oracle, name, gates_kernel):
    """one named graph as the custom gates of a whole system, under every scenario, through the interpreter and through the kernel
    generated for it: k = 5 with every permutation layout in turn, and at the first k whose extended domain passes the power table's
    low bits on all-(r - 1) and extreme columns.  Equal to the oracle limb for limb and every word below r"""
    for i, sc in enumerate(GPU_SCENARIOS):
        case, vin = U.system(oracle, 4, 5, sc, _layout(i), FLAT[name], LOOKUPS)
        assert np.array_equal(_run_full(h2, case, vin, (name, sc)), _oracle_h(oracle, case, vin)), (name, sc, _layout(i))
    k_hi = _ek_above_lo_bits(h2, oracle)
    for i, sc in enumerate([("const", "r-1"), ("extremes", 1)]):
        case, vin = U.system(oracle, 4, k_hi, sc, _layout(2 + 2 * i), FLAT[name], LOOKUPS)
        assert np.array_equal(_run_full(h2, case, vin, (name, sc, k_hi)), _oracle_h(oracle, case, vin)), (name, sc, k_hi)


@pytest.mark.gpu
@pytest.mark.parametrize("gates_kernel", ["interpreter"], indirect=True)
@pytest.mark.parametrize("sc", GPU_SCENARIOS, ids=U.scenario_id)
def test_gpu_evaluate_h_every_family_interpreted(h2, oracle, sc, gates_kernel):
    """every family -- the named ones and the eight random graphs -- as the custom gates AND as the first lookup's table expression
    (evaluated with PreviousValue = 0, its value handed to lookup_row), under one scenario, through the interpreter"""
    for i, (name, flat) in enumerate(FLAT.items()):
        case, vin = U.system(oracle, 4, 5, sc, _layout(i), flat, [flat, LOOKUPS[1]])
        assert np.array_equal(_run_full(h2, case, vin, (name, sc)), _oracle_h(oracle, case, vin)), (name, sc, _layout(i))


FUSED = ("products2", "products3", "fuse_add", "fuse_sub96", "fuse_add96", "fuse_horner", "id_ab-ba", "constants")


@pytest.mark.gpu
@pytest.mark.parametrize("gates_kernel", ["generated"], indirect=True)
@pytest.mark.parametrize("name", FUSED)
def test_gpu_evaluate_h_generated_without_fusion(h2, oracle, name, gates_kernel):
    """the graphs whose generated kernel fuses two products into one reduction, once more with the fusion off (mode + 16): another
    kernel (its source has no fu_mul_sub), the same words"""
    L = h2.lib()
    assert (U.compiled_program(h2, FLAT[name])["fused_on"] >= 0).any()
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(2 + 16), ctypes.c_uint32(0))
    for i, sc in enumerate(GPU_SCENARIOS):
        case, vin = U.system(oracle, 4, 5, sc, _layout(i), FLAT[name], LOOKUPS)
        assert np.array_equal(_run_full(h2, case, vin, (name, sc)), _oracle_h(oracle, case, vin)), (name, sc)


@pytest.mark.gpu
def test_gpu_identities_and_constants_from_python_integers(h2, oracle, gates_kernel):
    """systems of gates alone, so that the stored row is the graph's own value: a b - b a, (a + b) - a - b and a * 1 - a are k r in the
    lanes and must be stored as 0 (never r) under every scenario; a b - c d and the graphs of constants and scalars equal the Python
    integers"""
    for name in ["id_" + k for k in U.IDENTITIES] + ["id_abcd", "constants", "constants_only"]:
        for sc in GPU_SCENARIOS:
            case, vin = _gates_only(oracle, 5, sc, FLAT[name])
            got = _run_full(h2, case, vin, (name, sc))
            if name[3:] in U.IDENTITIES:
                assert not got.any(), (name, sc)
            want = U.eval_graph_ints(FLAT[name], _cosets_of(oracle, case), 1 << case["extended_k"], previous=vin, rot_scale=4)
            assert np.array_equal(got, want), (name, sc)


@pytest.mark.gpu
def test_gpu_evaluate_h_global_workspace_edges(h2, oracle):
    """the many-live graphs with the local slot tiers forced off: large positive and negative limbs through the global workspace"""
    L = h2.lib()
    h2.init()
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(0), ctypes.c_uint32(0))
    try:
        L.h2hip_debug_set_evalh_max_local_slots(ctypes.c_uint32(4))
        for n_live in (6, 12, 40, 100):
            for i, sc in enumerate([("const", "r-1"), ("const", "sat32top"), ("extremes", 1), ("signs", 7)]):
                case, vin = U.system(oracle, 4, 5, sc, _layout(i), FLAT["live%d" % n_live], LOOKUPS)
                assert np.array_equal(_run_full(h2, case, vin, (n_live, sc)), _oracle_h(oracle, case, vin)), (n_live, sc)
    finally:
        L.h2hip_debug_set_evalh_max_local_slots(ctypes.c_uint32(256))
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))


PARTS_GRAPHS = ("sum8", "wide_mul", "products3", "fuse_add96", "horner6", "prev_horner")


@pytest.mark.gpu
@pytest.mark.parametrize("j", [3, 9])
def test_gpu_evaluate_h_parts_edges(h2, oracle, j, gates_kernel):
    """evaluate_h_parts with every column a constant polynomial of an extreme word or a random one: equal to the oracle on the cosets
    of those polynomials and to the full form on them; once with t_evaluations (fu_mul_canon in the scatter and part-scale kernels)"""
    k = 5
    d, t_eval = oracle.domain_new(j, k)
    ext = lambda p: oracle.coeff_to_extended(d, p.copy(), 2)  # noqa: E731
    from test_evalh_parts import _full_of
    for gi, name in enumerate(PARTS_GRAPHS):
        for i, sc in enumerate([("const", "r-1"), ("const", "limbmax"), ("const", "sat32top"), ("extremes", 1), ("signs", 7), ("random", 5)]):
            parts, vin = U.system(oracle, j, k, sc, _layout(gi + i), FLAT[name], LOOKUPS, parts_form=True)
            full = _full_of(parts, ext)
            want = _oracle_h(oracle, full, vin)
            got = vin.copy()
            hp = PartsDescHolder(parts)
            rc = h2.lib().h2hip_evaluate_h_parts_bn254(hp.byref(), got.ctypes.data_as(ctypes.c_void_p))
            assert rc == 0, h2.lib().h2hip_last_error()
            eu.assert_below_r(got, (name, sc))
            assert np.array_equal(got, want), (name, sc)
            assert np.array_equal(_run_full(h2, full, vin, (name, sc, "full")), want), (name, sc)
            if gi == 0:
                got = vin.copy()
                hp = PartsDescHolder(dict(parts, t_evaluations=t_eval))
                rc = h2.lib().h2hip_evaluate_h_parts_bn254(hp.byref(), got.ctypes.data_as(ctypes.c_void_p))
                assert rc == 0, h2.lib().h2hip_last_error()
                eu.assert_below_r(got, (name, sc, "t"))
                assert np.array_equal(got, oracle.divide_by_vanishing_poly(d, t_eval, want)), (name, sc)


# ------------------------------------------------------------------------------------------- row graphs: lookup_compress, check_gates
ROW_K = 10
ROW_SCENARIOS = [("const", "r-1"), ("const", "sat32top"), ("extremes", 1), ("partial", 3), ("signs", 7), ("random", 5)]
ROW_FLAT = {name: flatten_graph(g) for name, g in U.row_families()}


@functools.lru_cache(maxsize=None)
def _row_reference(sc):
    """(columns, {family: its value on every row}) under a scenario, from Python integers; computed once and shared, read-only"""
    n = 1 << ROW_K
    cols = U.scenario_columns(sc, n)
    out = {}
    for name, flat in ROW_FLAT.items():
        out[name] = U.eval_graph_ints(flat, cols, n)
        out[name].setflags(write=False)
    return cols, out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _row_groups():
    """the graphs of one call run in the tier of its largest program: the small ones together, each many-live graph with a few of them"""
    small = [n for n in ROW_FLAT if not n.startswith("live")]
    return [small] + [[n, "sum8", "neg_product"] for n in ROW_FLAT if n.startswith("live")]


def test_row_families_cover_the_corpus():
    assert len(ROW_FLAT) >= 40 and {"sum8", "subchain5", "wide_mul", "fuse_sub96", "id_ab-ba", "horner6", "live100-open"} <= set(ROW_FLAT)
    assert all(U.row_graph_allowed(f, theta=False) for f in ROW_FLAT.values()) and not U.row_graph_allowed(FLAT["constants"], theta=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", ROW_SCENARIOS, ids=U.scenario_id)
def test_gpu_lookup_compress_edges(h2, sc):
    """lookup_compress takes column values directly: every fixed, advice and instance row drawn by the scenario, every family that a
    row graph may hold, host and device forms, against Python integers"""
    import torch
    h2.init()
    cols, want = _row_reference(sc)
    theta = cols["theta"]
    dcols = [[_dev(c) for c in cols[key]] for key in ("fixed", "advice", "instance")]
    for names in _row_groups():
        graphs = [ROW_FLAT[n] for n in names]
        got = h2.lookup_compress(ROW_K, graphs, theta, cols["fixed"], cols["advice"], cols["instance"], cols["challenges"])
        douts = [torch.empty_like(dcols[0][0]) for _ in names]
        h2.lookup_compress_device(ROW_K, graphs, theta, douts, dcols[0], dcols[1], dcols[2], cols["challenges"])
        torch.cuda.synchronize()
        for n, g, dg in zip(names, got, douts):
            eu.assert_below_r(g, (n, sc))
            assert np.array_equal(g, want[n]), (n, sc, np.flatnonzero((g != want[n]).any(axis=1))[:8])
            assert np.array_equal(h2.to_numpy_u64(dg), want[n]), (n, sc, "device form")
            if n[3:] in U.IDENTITIES:
                assert not g.any(), n


def _check_both(h2, graphs, cols, want, max_rows, tag):
    from test_check import assert_result
    host = h2.check_gates(ROW_K, graphs, cols["fixed"], cols["advice"], cols["instance"], cols["challenges"], max_rows)
    assert_result(host, want, "%s (host form)" % (tag,))
    dev = h2.check_gates_device(ROW_K, graphs, [_dev(c) for c in cols["fixed"]], [_dev(c) for c in cols["advice"]], [_dev(c) for c in cols["instance"]],
                                cols["challenges"], max_rows)
    assert_result(dev, want, "%s (device form)" % (tag,))


@pytest.mark.gpu
@pytest.mark.parametrize("sc", ROW_SCENARIOS, ids=U.scenario_id)
def test_gpu_check_gates_edges(h2, sc):
    """check_gates on the same graphs and columns: the failing rows are those where the Python integers are not 0 -- counts and lowest
    rows exact; the identities fail nowhere"""
    import check_util as cu
    h2.init()
    cols, values = _row_reference(sc)
    for names in _row_groups():
        fails = [np.flatnonzero(values[n].any(axis=1)).tolist() for n in names]
        for n, f in zip(names, fails):
            assert n[3:] not in U.IDENTITIES or f == []
        _check_both(h2, [ROW_FLAT[n] for n in names], cols, cu.expected(fails, 8), 8, (sc, names[0]))


@pytest.mark.gpu
def test_gpu_check_gates_satisfied_at_extremes_and_planted_rows(h2):
    """a b - c with a = b = -1, c = 1 and with a, b the elements stored as the word r - 1: satisfied on every row; then with c changed on
    planted rows (wave, workgroup and last-row boundaries): exactly those rows, in order"""
    import check_util as cu
    h2.init()
    n = 1 << ROW_K
    flat = FLAT["id_abcd"]  # advice 0 * advice 1 - advice 2 * advice 3: c in column 2, column 3 the constant one
    one = eu.words([U.VALUES["ONE_E"]])[0]
    w = (R_MOD - 1) * pow(1 << 256, -1, R_MOD) % R_MOD  # the element stored as the word r - 1
    planted = [0, 63, 64, 255, 256, 500, 1023]
    for a_word, c_word in ((U.VALUES["r-ONE_E"], U.VALUES["ONE_E"]), (R_MOD - 1, w * w % R_MOD * (1 << 256) % R_MOD)):
        cols = U.scenario_columns(("const", "0"), n)
        cols["advice"][0] = eu.const(n, a_word)
        cols["advice"][1] = eu.const(n, a_word)
        cols["advice"][2] = eu.const(n, c_word)
        cols["advice"][3] = np.tile(one, (n, 1))
        assert not U.eval_graph_ints(flat, cols, n).any()
        _check_both(h2, [flat], cols, cu.expected([[]], 8), 8, "satisfied")
        c = cols["advice"][2].copy()
        c[planted] = eu.words([R_MOD - 1 if c_word != R_MOD - 1 else 0])[0]
        cols["advice"][2] = c
        _check_both(h2, [flat], cols, cu.expected([planted], 8), 8, "planted")
        _check_both(h2, [flat], cols, cu.expected([planted], 4), 4, "planted, four rows")
