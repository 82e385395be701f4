"""The shuffle stage of evaluate_h (h2hip_evaluate_h_shuffles_bn254, its _device form, h2hip_evaluate_h_parts_shuffles_bn254 and its
_device form) against the big-integer model of tests/shuffle_util.py.  The argument is later than the reference, so the model is the
judge: column cosets come from the engine's oracle-checked coeff_to_extended, the value of h(X) before the shuffle stage from the oracle's
evaluate_h, and the three folds per shuffle are Python integers.  Field elements are canonical: every comparison is np.array_equal."""
import copy
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from evalh_util import (DescHolder, Evaluator, GraphEvaluator, PartsDescHolder, ShufflesHolder, custom_gates_graph,
                        evaluate_h_shuffles_workspace_bytes, evaluate_h_workspace_bytes, flatten_graph, lookup_graph, shuffle_graphs,
                        shuffle_required_degree)
from shuffle_util import R_MOD, Columns, fold_shuffles, from_mont, required_degree, to_mont

KEY_COLUMNS = (("fixed_polys", "fixed_cosets"), ("perm_product_polys", "perm_product_cosets"), ("perm_polys", "perm_cosets"))
KEY_SINGLES = (("l0_poly", "l0"), ("l_last_poly", "l_last"), ("l_active_row_poly", "l_active_row"))
DOMAINS = [(4, 4), (4, 7), (3, 9)]  # (j, k): (k, extended_k) = (4, 6), (7, 9), (9, 10)

A = lambda c, r=0: ('advice', c, r)  # noqa: E731
F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
I = lambda c, r=0: ('instance', c, r)  # noqa: E731
# one shuffle of single expressions; one of 3-tuples whose expressions use rotations, a fixed column, an instance column and a challenge;
# a third for the case with more shuffles than a coset group holds
SHUFFLES = [([A(0)], [A(1)]),
            ([A(2, 1), ('prod', F(0), A(3)), ('sum', I(0, -1), ('challenge', 1))], [A(4), F(1, 2), ('scaled', A(5, -2), 7)]),
            ([F(2)], [('sum', A(0, 1), ('const', 5))])]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _system(oracle, j, k, seed, rich, n_shuffles=2):
    """parts / full: the two forms' cases without their shuffles; shuffles: the expressions; z: one product polynomial per shuffle; ev: the
    Evaluator.  rich: two gates, one lookup and a permutation argument in front of the shuffles; otherwise the shuffles stand alone (no
    gate, no permutation, no lookup).  No GPU is needed to build it; the cosets of `full` are the oracle's."""
    n = 1 << k
    d, t_eval = oracle.domain_new(j, k)
    col = lambda s: _ro(oracle.gen_scalars(seed * 1000 + s, n))  # noqa: E731
    gates = [('sum', ('prod', ('prod', A(0, 1), A(1)), F(0)), ('neg', ('prod', A(2, -1), F(1, 1)))),
             ('scaled', ('sum', I(0), ('challenge', 0)), 3)] if rich else []
    lookups = [([A(0), ('prod', A(1), F(0))], [F(2), F(1, 1)])] if rich else []
    shuffles = SHUFFLES[:n_shuffles]
    ev = Evaluator.new(gates, lookups, shuffles)
    scalars = oracle.gen_scalars(seed * 1000 + 1, 6)
    parts = {
        "k": k, "extended_k": d.extended_k, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
        "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
        "y": scalars[0], "beta": scalars[1], "gamma": scalars[2], "theta": scalars[3], "challenges": scalars[4:6],
        "l0_poly": col(5), "l_last_poly": col(6), "l_active_row_poly": col(7),
        "fixed_polys": [col(10 + i) for i in range(3)], "advice_polys": [col(20 + i) for i in range(6)], "instance_polys": [col(30)],
        "custom": flatten_graph(ev.custom_gates),
        "perm_product_polys": [col(40 + i) for i in range(2)] if rich else [], "perm_polys": [col(44 + i) for i in range(3)] if rich else [],
        "perm_column_kind": np.array([0, 1, 2] if rich else [], dtype=np.uint32),
        "perm_column_index": np.array([1, 2, 0] if rich else [], dtype=np.uint32),
        "chunk_len": 2, "last_rotation": -4,
        "lookups": [(flatten_graph(g), col(50 + 3 * i), col(51 + 3 * i), col(52 + 3 * i)) for i, g in enumerate(ev.lookups)],
    }
    ext = lambda poly: _ro(oracle.coeff_to_extended(d, poly, 4))  # noqa: E731
    full = {key: v for key, v in parts.items() if not key.endswith("_polys") and not key.endswith("_poly")}
    for p_name, f_name in KEY_COLUMNS:
        full[f_name] = [ext(p) for p in parts[p_name]]
    for p_name, f_name in KEY_SINGLES:
        full[f_name] = ext(parts[p_name])
    full["advice_polys"], full["instance_polys"] = parts["advice_polys"], parts["instance_polys"]
    z = [col(60 + i) for i in range(n_shuffles)]
    vin = _ro(oracle.gen_scalars(seed * 1000 + 99, 1 << d.extended_k))  # nonzero on entry: an earlier instance's h
    return types.SimpleNamespace(parts=parts, full=full, shuffles=shuffles, z=z, ev=ev, vin=vin, d=d, t_eval=t_eval, j=j, k=k)


def _holder(sy):
    return ShufflesHolder([(flatten_graph(gi), flatten_graph(gs), z) for (gi, gs), z in zip(sy.ev.shuffles, sy.z)])


def _model(h2, oracle, sy, vin):
    """h(X) of the system on entry values vin: the oracle's evaluate_h up to the lookups, then the model's shuffle stage over the cosets
    the engine's coeff_to_extended forms"""
    before = np.array(vin, dtype=np.uint64)
    assert oracle.lib().oracle_evaluate_h(DescHolder(sy.full).byref(), before.ctypes.data_as(ctypes.c_void_p)) == 0
    dom = h2.EvaluationDomain.new(sy.j, sy.k)
    assert dom.extended_k == sy.d.extended_k
    size, P = 1 << dom.extended_k, 1 << (dom.extended_k - sy.k)
    ext = lambda polys: [from_mont(c) for c in dom.coeff_to_extended_batch(list(polys))]  # noqa: E731
    p = sy.parts
    cols = Columns(ext(p["fixed_polys"]), ext(p["advice_polys"]), ext(p["instance_polys"]), from_mont(p["challenges"]), size, P)
    l0, l_last, l_active = ext([p["l0_poly"], p["l_last_poly"], p["l_active_row_poly"]])
    y, theta, gamma = (from_mont(p[s])[0] for s in ("y", "theta", "gamma"))
    zc = ext(sy.z)
    out = fold_shuffles(from_mont(before), [(i, s, g, c) for (i, s), g, c in zip(sy.shuffles, sy.ev.shuffles, zc)], cols, y, theta, gamma, l0,
                        l_last, l_active)
    return _ro(to_mont(out))


_WANT = {}


def _want(h2, oracle, sy):
    key = (sy.j, sy.k, id(sy))
    if key not in _WANT:
        _WANT[key] = _model(h2, oracle, sy, sy.vin)
    return _WANT[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the shared arrays are read-only


def _to_device(holder, sh, case, z, names, keep):
    """move every column of a description and its shuffles into HBM: the tables of `holder` and `sh` then hold device addresses"""
    def table(ts):
        keep.extend(ts)
        arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        keep.append(arr)
        return ctypes.addressof(arr)

    for name in names:
        if isinstance(case[name], list):
            setattr(holder.desc, name, table([_dev(a) for a in case[name]]))
        else:
            t = _dev(case[name])
            keep.append(t)
            setattr(holder.desc, name, t.data_ptr())
    for q, field in enumerate(("lookup_product_polys", "lookup_permuted_input_polys", "lookup_permuted_table_polys")):
        setattr(holder.desc, field, table([_dev(l[1 + q]) for l in case["lookups"]]))
    if sh is not None and sh.desc.n_shuffles:
        sh.desc.product_polys = table([_dev(a) for a in z])


NAMES_P = ["fixed_polys", "advice_polys", "instance_polys", "perm_product_polys", "perm_polys", "l0_poly", "l_last_poly", "l_active_row_poly"]
NAMES_F = ["fixed_cosets", "advice_polys", "instance_polys", "perm_product_cosets", "perm_cosets", "l0", "l_last", "l_active_row"]


def _run(h2, sy, entry, vin, sh="shuffles", **extra):
    """one of the four entry points on a copy of vin.  sh: "shuffles" (the system's), None (a NULL struct) or a ShufflesHolder"""
    import torch
    L = h2.lib()
    parts_form, device = entry.startswith("parts"), entry.endswith("device")
    holder = PartsDescHolder({**sy.parts, **extra}) if parts_form else DescHolder(sy.full)
    shh = _holder(sy) if sh == "shuffles" else sh
    ref = ctypes.byref(shh.desc) if shh is not None else None
    fn = getattr(L, "h2hip_evaluate_h%s_shuffles_bn254%s" % ("_parts" if parts_form else "", "_device" if device else ""))
    if not device:
        got = np.array(vin, dtype=np.uint64)
        rc = fn(holder.byref(), ref, got.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, L.h2hip_last_error()
        return got
    keep = []
    _to_device(holder, shh, sy.parts if parts_form else sy.full, sy.z, NAMES_P if parts_form else NAMES_F, keep)
    v = _dev(vin)
    rc = fn(holder.byref(), ref, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.h2hip_last_error()
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint64)


ENTRIES = ["full_host", "full_device", "parts_host", "parts_device"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_symbols_are_exported_with_the_headers_arity(h2):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo2hip.h")).read(), flags=re.S)
    arity = {"h2hip_shuffle_products_bn254": 8, "h2hip_shuffle_products_bn254_device": 9, "h2hip_check_shuffles_bn254": 8,
             "h2hip_check_shuffles_bn254_device": 9, "h2hip_evaluate_h_shuffles_bn254": 3, "h2hip_evaluate_h_shuffles_bn254_device": 4,
             "h2hip_evaluate_h_parts_shuffles_bn254": 3, "h2hip_evaluate_h_parts_shuffles_bn254_device": 4,
             "h2hip_evaluate_h_shuffles_workspace_bytes": 12}
    rust = open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi.rs")).read()
    for name, count in arity.items():
        assert hasattr(h2.lib(), name), name
        args = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(args.split(",")) == count, name
        assert len(re.search(r"pub fn %s\(([^)]*)\)" % name, rust).group(1).split(",")) == count, name
    body = re.search(r"typedef struct h2hip_evalh_shuffles \{(.*?)\}\s*h2hip_evalh_shuffles;", text, flags=re.S).group(1)
    assert [" ".join(x.split()) for x in body.split(";") if x.strip()] == ["uint32_t n_shuffles", "const h2hip_graph* graphs",
                                                                          "const uint64_t* const* product_polys"]
    from evalh_util import EvalhShuffles
    assert [n for n, _ in EvalhShuffles._fields_] == ["n_shuffles", "graphs", "product_polys"]
    evalh_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "evalh.rs")).read()
    lib_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub struct EvalhShuffles \{\s*pub n_shuffles: u32,\s*pub graphs: \*const h2hip_graph,\s*pub product_polys: \*const \*const u64,\s*\}",
                     evalh_rs)
    for fn in ("try_evaluate_h_shuffles", "try_evaluate_h_parts_shuffles"):
        assert "pub fn %s<" % fn in evalh_rs
    for fn in ("try_shuffle_products", "try_check_shuffles"):
        assert "pub fn %s<" % fn in lib_rs


def test_required_degree():
    cases = [(([('const', 3)], [('challenge', 0)]), 3),                                   # max(1, 0, 0)
             (([A(0)], [F(1, 2)]), 3),
             (([('prod', A(0), A(1, 1))], [A(2)]), 4),
             (([A(0), ('prod', ('prod', A(0), F(0)), I(0))], [A(1), ('sum', A(2), ('scaled', ('neg', A(3)), 9))]), 5),
             (([('sum', ('prod', A(0), A(0)), ('prod', F(0), ('prod', F(1), ('prod', F(2), A(1)))))], [A(2)]), 6)]
    for (inp, shf), want in cases:
        assert shuffle_required_degree(inp, shf) == want == required_degree(inp, shf)
    for bad in (([], []), ([A(0)], [A(1), A(2)])):
        with pytest.raises(ValueError):
            shuffle_required_degree(*bad)


def test_shuffle_graphs_have_the_documented_shape():
    """per side: the parts of add_expression, Horner(Constant 0, parts, Theta), Add(that, Gamma) last; the graph's value is the model's
    A + gamma on a row of integers"""
    from shuffle_util import CALC_ADD, CALC_HORNER, VS_CONSTANT, VS_GAMMA, VS_THETA, compress, graph_value
    inp, shf = SHUFFLES[1]
    for g, exprs in zip(shuffle_graphs(inp, shf), (inp, shf)):
        (op_h, x_h, y_h, parts), t_h = g.calculations[-2]
        (op_a, x_a, y_a, _), _ = g.calculations[-1]
        assert op_h == CALC_HORNER and x_h == (VS_CONSTANT, 0, 0) and y_h == (VS_THETA, 0, 0) and len(parts) == len(exprs)
        assert op_a == CALC_ADD and x_a == (1, t_h, 0) and y_a == (VS_GAMMA, 0, 0)
        n = 8
        cols = Columns([[(7 * c + i) % R_MOD for i in range(n)] for c in range(3)], [[(100 * c + i * i) % R_MOD for i in range(n)] for c in range(6)],
                       [[5 + i for i in range(n)]], [11, 13], n)
        for idx in range(n):
            assert graph_value(g, cols, idx, 17, 19) == (compress(exprs, 17, cols, idx) + 19) % R_MOD
    assert graph_value(GraphEvaluator(), None, 0, 1, 2) == 0


def test_evaluate_h_shuffles_rejections_need_no_gpu(h2, oracle):
    """H2HIP_EINVAL with a named error from each of the four entry points, before any device work: NULL tables, a null product polynomial,
    a graph reading beta, y or the previous value, an index out of range, k > 28"""
    L = h2.lib()
    sy = _system(oracle, 4, 4, 7, True)
    flat = [(flatten_graph(gi), flatten_graph(gs), z) for (gi, gs), z in zip(sy.ev.shuffles, sy.z)]

    def rc_of(entry, mutate=None, poke=None, case_mut=None):
        parts_form, device = entry.startswith("parts"), entry.endswith("device")
        fl = copy.deepcopy(flat)
        if mutate:
            mutate(fl)
        shh = ShufflesHolder(fl)
        if poke:
            poke(shh)
        case = dict(sy.parts if parts_form else sy.full)
        if case_mut:
            case_mut(case)
        holder = (PartsDescHolder if parts_form else DescHolder)(case)
        fn = getattr(L, "h2hip_evaluate_h%s_shuffles_bn254%s" % ("_parts" if parts_form else "", "_device" if device else ""))
        v = np.array(sy.vin)
        return fn(holder.byref(), ctypes.byref(shh.desc), v.ctypes.data_as(ctypes.c_void_p), *((None,) if device else ()))

    def reads(kind):
        def m(fl): fl[1][1]["calcs"][-1, 5:8] = (kind, 0, 0)  # the closing Add's second operand
        return m
    def bad_column(fl): fl[0][0]["calcs"][0, 3] = 99
    def bad_rotation(fl): fl[1][0]["calcs"][0, 4] = 99
    def bad_part(fl): fl[1][0]["parts"][0] = (3, 99, 0)
    def bad_challenge(fl): fl[1][0]["parts"][2] = (5, 9, 0)
    def null_poly(h): ctypes.cast(h.desc.product_polys, ctypes.POINTER(ctypes.c_void_p))[1] = None
    for entry in ENTRIES:
        for m, text in ((reads(6), b"reads beta, y or the previous value"), (reads(9), b"reads beta, y or the previous value"),
                        (reads(10), b"reads beta, y or the previous value"), (bad_column, b"shuffle graph, calculation 0 is malformed"),
                        (bad_rotation, b"shuffle graph"), (bad_part, b"shuffle graph"), (bad_challenge, b"shuffle graph")):
            assert rc_of(entry, mutate=m) == 1, (entry, text)
            err = L.h2hip_last_error()
            assert err.startswith(b"evaluate_h: ") and text in err, (entry, err)
        for p, text in ((null_poly, b"shuffle product_polys[1] is null"), (lambda h: setattr(h.desc, "product_polys", None), b"null shuffle product_polys"),
                        (lambda h: setattr(h.desc, "graphs", None), b"null shuffle graphs"), (lambda h: setattr(h.desc, "n_shuffles", 70000), b"shuffles > 65535")):
            assert rc_of(entry, poke=p) == 1, (entry, text)
            assert text in L.h2hip_last_error(), (entry, L.h2hip_last_error())

        def k29(c): c["k"], c["extended_k"] = 29, 29
        assert rc_of(entry, case_mut=k29) == 1 and b"bad domain (k = 29" in L.h2hip_last_error()
    u = ctypes.c_uint32
    out = ctypes.c_size_t()
    assert L.h2hip_evaluate_h_shuffles_workspace_bytes(u(29), u(29), u(1), u(1), u(1), u(1), u(1), u(1), u(1), 0, 0, ctypes.byref(out)) == 1
    assert b"bad domain" in L.h2hip_last_error()


def test_workspace_bytes_with_shuffles(h2):
    """the existing function is the n_shuffles == 0 case; a group of shuffles adds one column per shuffle (and, in the host parts form,
    each shuffle's coefficient column)"""
    k, ek, shape = 12, 14, (6, 5, 1, 3, 5, 2)
    col, part = 32 << ek, 32 << k
    for parts_form in (False, True):
        for dev in (False, True):
            base = evaluate_h_workspace_bytes(k, ek, *shape, parts_form, dev)
            assert evaluate_h_shuffles_workspace_bytes(k, ek, *shape, 0, parts_form, dev) == base
            more = evaluate_h_shuffles_workspace_bytes(k, ek, *shape, 3, parts_form, dev) - base
            if not parts_form:
                assert more == 3 * (col + 256)
            else:
                assert more == 3 * part * (1 if dev else 2)
    try:
        h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(1))  # one shuffle per group
        assert evaluate_h_shuffles_workspace_bytes(k, ek, *shape, 3, True, True) - evaluate_h_shuffles_workspace_bytes(k, ek, *shape, 0, True, True) == part
    finally:
        h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rich", [False, True], ids=["alone", "after_lookup_and_permutation"])
@pytest.mark.parametrize("j,k", DOMAINS)
def test_gpu_shuffles_vs_model(h2, oracle, j, k, rich, entry):
    """two shuffles (singles; 3-tuples with rotations, a fixed column, an instance column and a challenge), alone and behind two gates, a
    lookup and a permutation argument, through each of the four entry points: fewer rows than a workgroup, several workgroups with
    r_next wrapping at the last row of the domain and of each part, and P = 2"""
    h2.init()
    sy = _system(oracle, j, k, 100 * j + k, rich)
    want = _want(h2, oracle, sy)
    assert not np.array_equal(want, sy.vin)
    assert np.array_equal(_run(h2, sy, entry, sy.vin), want)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_without_shuffles_equals_the_existing_call(h2, oracle, entry):
    """a NULL struct and n_shuffles == 0: each new entry point returns its existing counterpart's bytes, which are the oracle's"""
    h2.init()
    sy = _system(oracle, 4, 7, 407, True)
    L = h2.lib()
    parts_form = entry.startswith("parts")
    holder = PartsDescHolder(sy.parts) if parts_form else DescHolder(sy.full)
    old = np.array(sy.vin, dtype=np.uint64)
    fn = L.h2hip_evaluate_h_parts_bn254 if parts_form else L.h2hip_evaluate_h_bn254
    assert fn(holder.byref(), old.ctypes.data_as(ctypes.c_void_p)) == 0, L.h2hip_last_error()
    want = np.array(sy.vin, dtype=np.uint64)
    assert oracle.lib().oracle_evaluate_h(DescHolder(sy.full).byref(), want.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(old, want)
    assert _run(h2, sy, entry, sy.vin, sh=None).tobytes() == old.tobytes()
    assert _run(h2, sy, entry, sy.vin, sh=ShufflesHolder([])).tobytes() == old.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["full_host", "parts_host"])
def test_gpu_shuffle_programs_in_the_global_slot_tier(h2, oracle, entry):
    """every program of the call, the shuffles' two included, on the global slot workspace (rows taken grid-stride)"""
    h2.init()
    sy = _system(oracle, 4, 7, 407, True)
    want = _want(h2, oracle, sy)
    L = h2.lib()
    try:
        L.h2hip_debug_set_evalh_max_local_slots(0)
        got = _run(h2, sy, entry, sy.vin)
    finally:
        L.h2hip_debug_set_evalh_max_local_slots(256)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_more_shuffles_than_a_coset_group(h2, oracle, entry):
    """three shuffles, one product coset per group: each group's coset is formed in the buffer the one before used"""
    h2.init()
    sy = _system(oracle, 4, 7, 417, True, 3)
    want = _want(h2, oracle, sy)
    L = h2.lib()
    L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(1))
    try:
        got = _run(h2, sy, entry, sy.vin)
    finally:
        L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))
    assert np.array_equal(got, want)
    assert np.array_equal(_run(h2, sy, entry, sy.vin), want)  # and all three in one group


@pytest.mark.gpu
def test_gpu_two_instances_then_t_evaluations(h2, oracle):
    """two circuit instances chained through values in both forms; t_evaluations on the last call of the parts form gives
    divide_by_vanishing_poly of the two-instance h"""
    h2.init()
    s1, s2 = _system(oracle, 4, 7, 407, True), _system(oracle, 4, 7, 408, False)
    h1 = _want(h2, oracle, s1)
    h_two = _model(h2, oracle, s2, h1)
    assert np.array_equal(_run(h2, s2, "full_host", _run(h2, s1, "full_host", s1.vin)), h_two)
    assert np.array_equal(_run(h2, s2, "parts_host", _run(h2, s1, "parts_host", s1.vin)), h_two)
    want = oracle.divide_by_vanishing_poly(s1.d, s1.t_eval, h_two)
    assert np.array_equal(_run(h2, s2, "parts_host", h1, t_evaluations=s1.t_eval), want)
    assert np.array_equal(_run(h2, s2, "parts_device", h1, t_evaluations=s1.t_eval), want)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["parts_host", "parts_device"])
def test_gpu_part_ranges_split_one_h(h2, oracle, entry):
    """part 0 in one call, parts 1 .. P - 1 in another: rows of the other parts keep what they held, together they are the whole"""
    h2.init()
    sy = _system(oracle, 4, 7, 407, True)
    want = _want(h2, oracle, sy)
    P = 4
    first = _run(h2, sy, entry, sy.vin, part_begin=0, part_count=1)
    assert np.array_equal(first[0::P], want[0::P])
    for p in range(1, P):
        assert np.array_equal(first[p::P], sy.vin[p::P]), p
    both = _run(h2, sy, entry, first, part_begin=1, part_count=P - 1)
    assert np.array_equal(both, want)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [R_MOD - 1, 0], ids=["r_minus_1", "zero"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_magnitude_edges(h2, oracle, entry, value):
    """z, both graph values, l_active, l0, l_last, y and the incoming values all r - 1, then all zero: the largest operands the kernel's
    bounds allow for, and the smallest"""
    h2.init()
    j, k = 4, 5
    n = 1 << k
    d, t_eval = oracle.domain_new(j, k)
    size = 1 << d.extended_k
    const_poly = _ro(to_mont([value] + [0] * (n - 1)))  # the constant polynomial: its coset is `value` on every row
    const_coset = _ro(to_mont([value] * size))
    fe = _ro(to_mont([value])[0])
    zero = _ro(to_mont([0])[0])
    # a = value + gamma with gamma = 0: both graphs are the constant expression
    shuffles = [([('const', value)], [('const', value)])]
    ev = Evaluator.new([], [], shuffles)
    empty = np.zeros(0, dtype=np.uint32)
    common = {"k": k, "extended_k": d.extended_k, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
              "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
              "y": fe, "beta": zero, "gamma": zero, "theta": fe, "challenges": np.zeros((0, 4), dtype=np.uint64),
              "advice_polys": [const_poly], "instance_polys": [], "custom": flatten_graph(ev.custom_gates),
              "perm_column_kind": empty, "perm_column_index": empty, "chunk_len": 2, "last_rotation": -4, "lookups": []}
    parts = {**common, "l0_poly": const_poly, "l_last_poly": const_poly, "l_active_row_poly": const_poly, "fixed_polys": [],
             "perm_product_polys": [], "perm_polys": []}
    full = {**common, "l0": const_coset, "l_last": const_coset, "l_active_row": const_coset, "fixed_cosets": [], "perm_product_cosets": [],
            "perm_cosets": []}
    sy = types.SimpleNamespace(parts=parts, full=full, shuffles=shuffles, z=[const_poly], ev=ev, vin=const_coset, d=d, t_eval=t_eval, j=j, k=k)
    want = _model(h2, oracle, sy, sy.vin)
    v, a = value, value
    e = ((v * v + (1 - v) * v) * v + (v * v - v) * v) * v + v * (v * a - v * a)
    assert from_mont(want) == [e % R_MOD] * size  # the model on constant columns, by hand
    assert np.array_equal(_run(h2, sy, entry, sy.vin), want)


@pytest.mark.gpu
def test_gpu_python_wrapper(h2, oracle):
    """Evaluator.evaluate_h / evaluate_h_parts take the stage from the case's "shuffles" entry; without it they are the existing calls"""
    h2.init()
    sy = _system(oracle, 4, 4, 404, True)
    want = _want(h2, oracle, sy)
    strip = lambda case: {**case, "lookups": [l[1:] for l in case["lookups"]]}  # noqa: E731  (the graphs are the Evaluator's)
    assert np.array_equal(sy.ev.evaluate_h({**strip(sy.full), "shuffles": sy.z}, np.array(sy.vin)), want)
    assert np.array_equal(sy.ev.evaluate_h_parts({**strip(sy.parts), "shuffles": sy.z}, np.array(sy.vin)), want)
    got = sy.ev.evaluate_h_parts({**strip(sy.parts), "shuffles": sy.z}, np.array(sy.vin), t_evaluations=sy.t_eval)
    assert np.array_equal(got, oracle.divide_by_vanishing_poly(sy.d, sy.t_eval, want))
    before = np.array(sy.vin)
    assert oracle.lib().oracle_evaluate_h(DescHolder(sy.full).byref(), before.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(sy.ev.evaluate_h(strip(sy.full), np.array(sy.vin)), before)
    with pytest.raises(ValueError):
        sy.ev.evaluate_h({**strip(sy.full), "shuffles": sy.z[:1]}, np.array(sy.vin))
