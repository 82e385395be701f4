"""The mv-lookup stage of evaluate_h (h2hip_evaluate_h_ext_bn254, its _device form, h2hip_evaluate_h_parts_ext_bn254 and its _device
form) against the big-integer model of tests/mvlookup_util.py.  The argument is later than the reference, so the model is the judge:
column cosets come from the engine's oracle-checked coeff_to_extended, the value of h(X) before the stage from the oracle's evaluate_h,
the folds per argument are Python integers, and a shuffle stage behind them is tests/shuffle_util.py's.  Every comparison is limb for limb."""
import copy
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from evalh_util import (DescHolder, Evaluator, GraphEvaluator, MvLookupsHolder, PartsDescHolder, ShufflesHolder,
                        evaluate_h_ext_workspace_bytes, evaluate_h_shuffles_workspace_bytes, flatten_graph, mvlookup_graphs,
                        mvlookup_required_degree)
from mvlookup_util import R_MOD, Columns, fold_mvlookups, from_mont, graph_value, required_degree, to_mont
from shuffle_util import compress, fold_shuffles

KEY_COLUMNS = (("fixed_polys", "fixed_cosets"), ("perm_product_polys", "perm_product_cosets"), ("perm_polys", "perm_cosets"))
KEY_SINGLES = (("l0_poly", "l0"), ("l_last_poly", "l_last"), ("l_active_row_poly", "l_active_row"))
DOMAINS = [(4, 5), (3, 5)]  # (j, k): k = 5 with extended_k = 7 (P = 4) and 6 (P = 2)

A = lambda c, r=0: ('advice', c, r)  # noqa: E731
F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
I = lambda c, r=0: ('instance', c, r)  # noqa: E731
# K = 1 with single expressions; K = 5 with pairs that use rotations, a fixed column, an instance column, a challenge and a constant; a
# third argument (K = 2) for the case with more arguments than a coset group holds
MVLOOKUPS = [([[A(0)]], [F(0)]),
             ([[A(1), ('prod', F(0), A(2))], [A(3, 1), I(0, -1)], [('sum', A(4), ('challenge', 1)), F(1, 2)], [A(5, -2), ('const', 7)],
               [('scaled', A(0, 1), 3), A(1)]], [F(2), F(1, 1)]),
             ([[F(2, -1)], [('neg', A(2))]], [('sum', A(0, 1), ('const', 5))])]
SHUFFLES = [([A(0)], [A(1)]), ([A(2, 1), ('prod', F(0), A(3))], [A(4), F(1, 2)])]
VARIANTS = {"alone": (False, False), "with_lookups": (True, False), "with_shuffles": (False, True), "with_all": (True, True)}


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _system(oracle, j, k, seed, variant, n_mv=2, mv_override=None):
    """parts / full: the two forms' cases without their mv-lookups and shuffles; mv: the expressions; phi / m: one polynomial each per
    argument; z: one per shuffle; ev: the Evaluator.  variant: whether two gates, a halo2 lookup and a permutation argument stand in
    front of the mv-lookups, and whether two shuffles follow.  No GPU is needed; the cosets of `full` are the oracle's."""
    rich, with_shuffles = VARIANTS[variant]
    n = 1 << k
    d, t_eval = oracle.domain_new(j, k)
    col = lambda s: _ro(oracle.gen_scalars(seed * 1000 + s, n))  # noqa: E731
    gates = [('sum', ('prod', ('prod', A(0, 1), A(1)), F(0)), ('neg', ('prod', A(2, -1), F(1, 1)))),
             ('scaled', ('sum', I(0), ('challenge', 0)), 3)] if rich else []
    lookups = [([A(0), ('prod', A(1), F(0))], [F(2), F(1, 1)])] if rich else []
    shuffles = SHUFFLES if with_shuffles else []
    mv = list(mv_override) if mv_override is not None else MVLOOKUPS[:n_mv]
    ev = Evaluator.new(gates, lookups, shuffles, mv)
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
    phi, m = [col(70 + i) for i in range(len(mv))], [col(80 + i) for i in range(len(mv))]
    z = [col(60 + i) for i in range(len(shuffles))]
    vin = _ro(oracle.gen_scalars(seed * 1000 + 99, 1 << d.extended_k))  # nonzero on entry: an earlier instance's h
    return types.SimpleNamespace(parts=parts, full=full, mv=mv, shuffles=shuffles, phi=phi, m=m, z=z, ev=ev, vin=vin, d=d, t_eval=t_eval, j=j,
                                 k=k)


def _mv_holder(sy):
    return MvLookupsHolder([([flatten_graph(g) for g in gs], phi, m) for gs, phi, m in zip(sy.ev.mv_lookups, sy.phi, sy.m)])


def _sh_holder(sy):
    return ShufflesHolder([(flatten_graph(gi), flatten_graph(gs), z) for (gi, gs), z in zip(sy.ev.shuffles, sy.z)])


def _model(h2, oracle, sy, vin):
    """h(X) of the system on entry values vin: the oracle's evaluate_h up to the halo2 lookups, then the model's mv-lookup stage and the
    shuffle model's stage over the cosets the engine's coeff_to_extended forms"""
    before = np.array(vin, dtype=np.uint64)
    assert oracle.lib().oracle_evaluate_h(DescHolder(sy.full).byref(), before.ctypes.data_as(ctypes.c_void_p)) == 0
    dom = h2.EvaluationDomain.new(sy.j, sy.k)
    assert dom.extended_k == sy.d.extended_k
    size, P = 1 << dom.extended_k, 1 << (dom.extended_k - sy.k)
    ext = lambda polys: [from_mont(c) for c in dom.coeff_to_extended_batch(list(polys))]  # noqa: E731
    p = sy.parts
    cols = Columns(ext(p["fixed_polys"]), ext(p["advice_polys"]), ext(p["instance_polys"]), from_mont(p["challenges"]), size, P)
    l0, l_last, l_active = ext([p["l0_poly"], p["l_last_poly"], p["l_active_row_poly"]])
    y, theta, beta, gamma = (from_mont(p[s])[0] for s in ("y", "theta", "beta", "gamma"))
    pc, mc = ext(sy.phi), ext(sy.m)
    out = fold_mvlookups(from_mont(before), [(i, t, g, a, b) for (i, t), g, a, b in zip(sy.mv, sy.ev.mv_lookups, pc, mc)], cols, y, theta,
                         beta, l0, l_last, l_active)
    if sy.shuffles:
        out = fold_shuffles(out, [(i, s, g, c) for (i, s), g, c in zip(sy.shuffles, sy.ev.shuffles, ext(sy.z))], cols, y, theta, gamma, l0,
                            l_last, l_active)
    return _ro(to_mont(out))


_WANT = {}


def _want(h2, oracle, sy):
    key = id(sy)
    if key not in _WANT:
        _WANT[key] = (sy, _model(h2, oracle, sy, sy.vin))
    return _WANT[key][1]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the shared arrays are read-only


def _to_device(holder, mvh, shh, case, sy, names, keep):
    """move every column of a description, its mv-lookups and its shuffles into HBM: the tables then hold device addresses"""
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
    if mvh is not None and mvh.desc.n_args:
        mvh.desc.phi_polys = table([_dev(a) for a in sy.phi])
        mvh.desc.m_polys = table([_dev(a) for a in sy.m])
    if shh is not None and shh.desc.n_shuffles:
        shh.desc.product_polys = table([_dev(a) for a in sy.z])


NAMES_P = ["fixed_polys", "advice_polys", "instance_polys", "perm_product_polys", "perm_polys", "l0_poly", "l_last_poly", "l_active_row_poly"]
NAMES_F = ["fixed_cosets", "advice_polys", "instance_polys", "perm_product_cosets", "perm_cosets", "l0", "l_last", "l_active_row"]


def _run(h2, sy, entry, vin, mv="system", sh="system", **extra):
    """one of the four _ext entry points on a copy of vin.  mv / sh: "system" (the system's), None (a NULL struct) or a holder"""
    import torch
    L = h2.lib()
    parts_form, device = entry.startswith("parts"), entry.endswith("device")
    holder = PartsDescHolder({**sy.parts, **extra}) if parts_form else DescHolder(sy.full)
    mvh = _mv_holder(sy) if mv == "system" else mv
    shh = (_sh_holder(sy) if sy.shuffles else None) if sh == "system" else sh
    ref = lambda h: ctypes.byref(h.desc) if h is not None else None  # noqa: E731
    fn = getattr(L, "h2hip_evaluate_h%s_ext_bn254%s" % ("_parts" if parts_form else "", "_device" if device else ""))
    if not device:
        got = np.array(vin, dtype=np.uint64)
        rc = fn(holder.byref(), ref(mvh), ref(shh), got.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, L.h2hip_last_error()
        return got
    keep = []
    _to_device(holder, mvh, shh, sy.parts if parts_form else sy.full, sy, NAMES_P if parts_form else NAMES_F, keep)
    v = _dev(vin)
    rc = fn(holder.byref(), ref(mvh), ref(shh), ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.h2hip_last_error()
    torch.cuda.synchronize()
    return v.cpu().numpy().view(np.uint64)


ENTRIES = ["full_host", "full_device", "parts_host", "parts_device"]


def _many_live_tuple(n_live):
    """one expression whose n_live scaled products are all alive at once: a right-leaning sum is added left operand first, so every
    product exists before the innermost sum consumes the last two"""
    terms = [('scaled', ('prod', A(i % 6, i % 2), F(i % 3)), 1000 + i) for i in range(n_live)]
    e = terms[-1]
    for t in reversed(terms[:-1]):
        e = ('sum', t, e)
    return (e,)


def _compile_stats(h2, graph_dict):
    holder = DescHolder.__new__(DescHolder)
    holder.keep = []
    G = holder._graph(graph_dict)
    n_ops, n_slots = ctypes.c_uint32(), ctypes.c_uint32()
    assert h2.lib().h2hip_debug_evalh_compile_stats(ctypes.byref(G), ctypes.byref(n_ops), ctypes.byref(n_slots)) == 0
    return n_ops.value, n_slots.value


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_symbols_are_exported_with_the_headers_arity(h2):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo2hip.h")).read(), flags=re.S)
    arity = {"h2hip_mvlookup_multiplicities_bn254": 7, "h2hip_mvlookup_multiplicities_bn254_device": 8, "h2hip_mvlookup_sums_bn254": 10,
             "h2hip_mvlookup_sums_bn254_device": 11, "h2hip_evaluate_h_ext_bn254": 4, "h2hip_evaluate_h_ext_bn254_device": 5,
             "h2hip_evaluate_h_parts_ext_bn254": 4, "h2hip_evaluate_h_parts_ext_bn254_device": 5, "h2hip_evaluate_h_ext_workspace_bytes": 13}
    rust = open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi.rs")).read()
    for name, count in arity.items():
        assert hasattr(h2.lib(), name), name
        args = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(args.split(",")) == count, name
        assert len(re.search(r"pub fn %s\(([^)]*)\)" % name, rust).group(1).split(",")) == count, name
    body = re.search(r"typedef struct h2hip_evalh_mvlookups \{(.*?)\}\s*h2hip_evalh_mvlookups;", text, flags=re.S).group(1)
    assert [" ".join(x.split()) for x in body.split(";") if x.strip()] == [
        "uint32_t n_args", "const uint32_t* n_inputs", "const h2hip_graph* graphs", "const uint64_t* const* phi_polys",
        "const uint64_t* const* m_polys"]
    from evalh_util import EvalhMvLookups
    assert [n for n, _ in EvalhMvLookups._fields_] == ["n_args", "n_inputs", "graphs", "phi_polys", "m_polys"]
    evalh_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "evalh.rs")).read()
    lib_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub struct EvalhMvLookups \{\s*pub n_args: u32,\s*pub n_inputs: \*const u32,\s*pub graphs: \*const h2hip_graph,\s*"
                     r"pub phi_polys: \*const \*const u64,\s*pub m_polys: \*const \*const u64,\s*\}", evalh_rs)
    for fn in ("try_evaluate_h_ext", "try_evaluate_h_parts_ext"):
        assert "pub fn %s<" % fn in evalh_rs
    for fn in ("try_mvlookup_multiplicities", "try_mvlookup_sums"):
        assert "pub fn %s<" % fn in lib_rs


def test_required_degree():
    cases = [(([[('const', 3)]], [('challenge', 0)]), 4),                                  # 2 + max(1, 0) + max(1, 0)
             (([[A(0)]], [F(1, 2)]), 4),
             (([[('prod', A(0), A(1, 1))]], [A(2)]), 5),
             (([[A(0)], [A(1)], [A(2)], [A(3)]], [F(0)]), 7),                              # every further input costs its degree
             (([[A(0), ('prod', ('prod', A(0), F(0)), I(0))], [A(1)]], [A(1), ('sum', A(2), ('scaled', ('neg', A(3)), 9))]), 7),
             (MVLOOKUPS[1], 2 + 1 + (2 + 1 + 1 + 1 + 1))]
    for (inputs, tab), want in cases:
        assert mvlookup_required_degree(inputs, tab) == want == required_degree(inputs, tab)
    with pytest.raises(ValueError):
        mvlookup_required_degree([], [A(0)])


def test_mvlookup_graphs_have_the_documented_shape():
    """per tuple: the parts of add_expression, Horner(Constant 0, parts, Theta), Add(that, Beta) last; the graph's value is the model's
    F + beta on a row of integers; the input graphs come first, the table graph last"""
    from mvlookup_util import CALC_ADD, CALC_HORNER, VS_BETA, VS_CONSTANT, VS_THETA
    inputs, tab = MVLOOKUPS[1]
    gs = mvlookup_graphs(inputs, tab)
    assert len(gs) == len(inputs) + 1
    n = 8
    cols = Columns([[(7 * c + i) % R_MOD for i in range(n)] for c in range(3)], [[(100 * c + i * i) % R_MOD for i in range(n)] for c in range(6)],
                   [[5 + i for i in range(n)]], [11, 13], n)
    for g, exprs in zip(gs, list(inputs) + [tab]):
        (op_h, x_h, y_h, parts), t_h = g.calculations[-2]
        (op_a, x_a, y_a, _), _ = g.calculations[-1]
        assert op_h == CALC_HORNER and x_h == (VS_CONSTANT, 0, 0) and y_h == (VS_THETA, 0, 0) and len(parts) == len(exprs)
        assert op_a == CALC_ADD and x_a == (1, t_h, 0) and y_a == (VS_BETA, 0, 0)
        for idx in range(n):
            assert graph_value(g, cols, idx, 17, 19) == (compress(exprs, 17, cols, idx) + 19) % R_MOD
    assert graph_value(GraphEvaluator(), None, 0, 1, 2) == 0
    with pytest.raises(ValueError):
        mvlookup_graphs([], tab)


def test_evaluate_h_ext_rejections_need_no_gpu(h2, oracle):
    """H2HIP_EINVAL with a named error from each of the four entry points, before any device work"""
    L = h2.lib()
    sy = _system(oracle, 4, 4, 7, "with_all")
    flat = [([flatten_graph(g) for g in gs], phi, m) for gs, phi, m in zip(sy.ev.mv_lookups, sy.phi, sy.m)]

    def rc_of(entry, mutate=None, poke=None, case_mut=None):
        parts_form, device = entry.startswith("parts"), entry.endswith("device")
        fl = copy.deepcopy(flat)
        if mutate:
            mutate(fl)
        mvh = MvLookupsHolder(fl)
        if poke:
            poke(mvh)
        case = dict(sy.parts if parts_form else sy.full)
        if case_mut:
            case_mut(case)
        holder = (PartsDescHolder if parts_form else DescHolder)(case)
        fn = getattr(L, "h2hip_evaluate_h%s_ext_bn254%s" % ("_parts" if parts_form else "", "_device" if device else ""))
        v = np.array(sy.vin)
        return fn(holder.byref(), ctypes.byref(mvh.desc), ctypes.byref(_sh_holder(sy).desc), v.ctypes.data_as(ctypes.c_void_p),
                  *((None,) if device else ()))

    def reads(kind):
        def m(fl): fl[1][0][5]["calcs"][-1, 5:8] = (kind, 0, 0)  # the table graph's closing Add, its second operand
        return m
    def bad_column(fl): fl[0][0][0]["calcs"][0, 3] = 99
    def bad_part(fl): fl[1][0][0]["parts"][0] = (3, 99, 0)
    def null_poly(name):
        def p(h): ctypes.cast(getattr(h.desc, name), ctypes.POINTER(ctypes.c_void_p))[1] = None
        return p
    def k_of(v):
        def p(h): ctypes.cast(h.desc.n_inputs, ctypes.POINTER(ctypes.c_uint32))[0] = v
        return p
    for entry in ENTRIES:
        for m, text in ((reads(7), b"reads gamma, y or the previous value"), (reads(9), b"reads gamma, y or the previous value"),
                        (reads(10), b"reads gamma, y or the previous value"), (bad_column, b"mv-lookup graph, calculation 0 is malformed"),
                        (bad_part, b"mv-lookup graph")):
            assert rc_of(entry, mutate=m) == 1, (entry, text)
            err = L.h2hip_last_error()
            assert err.startswith(b"evaluate_h: ") and text in err, (entry, err)
        for p, text in ((null_poly("phi_polys"), b"mv-lookup phi_polys[1] is null"), (null_poly("m_polys"), b"mv-lookup m_polys[1] is null"),
                        (lambda h: setattr(h.desc, "phi_polys", None), b"null mv-lookup phi_polys"),
                        (lambda h: setattr(h.desc, "m_polys", None), b"null mv-lookup m_polys"),
                        (lambda h: setattr(h.desc, "graphs", None), b"null mv-lookup n_inputs or graphs"),
                        (lambda h: setattr(h.desc, "n_inputs", None), b"null mv-lookup n_inputs or graphs"),
                        (lambda h: setattr(h.desc, "n_args", 70000), b"mv-lookup arguments > 65535"),
                        (k_of(0), b"mv-lookup n_inputs[0] = 0"), (k_of(256), b"mv-lookup n_inputs[0] = 256")):
            assert rc_of(entry, poke=p) == 1, (entry, text)
            assert text in L.h2hip_last_error(), (entry, L.h2hip_last_error())

        def k29(c): c["k"], c["extended_k"] = 29, 29
        assert rc_of(entry, case_mut=k29) == 1 and b"bad domain (k = 29" in L.h2hip_last_error()
    u = ctypes.c_uint32
    out = ctypes.c_size_t()
    assert L.h2hip_evaluate_h_ext_workspace_bytes(u(29), u(29), u(1), u(1), u(1), u(1), u(1), u(1), u(1), u(1), 0, 0, ctypes.byref(out)) == 1
    assert b"bad domain" in L.h2hip_last_error()


def test_workspace_bytes_with_mvlookups(h2):
    """the shuffles' function is the n_mvlookups == 0 case; a group of arguments adds two columns per argument (and, in the host parts
    form, each argument's two coefficient columns)"""
    k, ek, shape = 12, 14, (6, 5, 1, 3, 5, 2)
    col, part = 32 << ek, 32 << k
    for parts_form in (False, True):
        for dev in (False, True):
            base = evaluate_h_shuffles_workspace_bytes(k, ek, *shape, 2, parts_form, dev)
            assert evaluate_h_ext_workspace_bytes(k, ek, *shape, 0, 2, parts_form, dev) == base
            more = evaluate_h_ext_workspace_bytes(k, ek, *shape, 3, 2, parts_form, dev) - base
            if not parts_form:
                assert more == 6 * (col + 256)
            else:
                assert more == 6 * part * (1 if dev else 2)
    try:
        h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(1))  # one argument per group
        assert evaluate_h_ext_workspace_bytes(k, ek, *shape, 3, 0, True, True) - evaluate_h_ext_workspace_bytes(k, ek, *shape, 0, 0, True, True) == 2 * part
    finally:
        h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("j,k", DOMAINS)
def test_gpu_mvlookups_vs_model(h2, oracle, j, k, variant, entry):
    """two arguments (K = 1 of single expressions; K = 5 of pairs with rotations, a fixed column, an instance column, a challenge and a
    constant), alone, behind two gates, a halo2 lookup and a permutation argument, in front of two shuffles, and between both, through
    each of the four entry points, at k = 5 with P = 4 and P = 2"""
    h2.init()
    sy = _system(oracle, j, k, 100 * j + k, variant)
    want = _want(h2, oracle, sy)
    assert not np.array_equal(want, sy.vin)
    assert np.array_equal(_run(h2, sy, entry, sy.vin), want)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_null_extras_equal_the_existing_calls(h2, oracle, entry):
    """mvlookups == NULL (or empty) is the _shuffles call and both NULL the call without a suffix, byte for byte"""
    h2.init()
    sy = _system(oracle, 4, 5, 405, "with_all")
    L = h2.lib()
    parts_form, device = entry.startswith("parts"), entry.endswith("device")
    holder = PartsDescHolder(sy.parts) if parts_form else DescHolder(sy.full)
    plain = np.array(sy.vin, dtype=np.uint64)
    fn = L.h2hip_evaluate_h_parts_bn254 if parts_form else L.h2hip_evaluate_h_bn254
    assert fn(holder.byref(), plain.ctypes.data_as(ctypes.c_void_p)) == 0, L.h2hip_last_error()
    want = np.array(sy.vin, dtype=np.uint64)
    assert oracle.lib().oracle_evaluate_h(DescHolder(sy.full).byref(), want.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(plain, want)
    assert _run(h2, sy, entry, sy.vin, mv=None, sh=None).tobytes() == plain.tobytes()
    assert _run(h2, sy, entry, sy.vin, mv=MvLookupsHolder([]), sh=ShufflesHolder([])).tobytes() == plain.tobytes()
    shuf = np.array(sy.vin, dtype=np.uint64)
    fn = L.h2hip_evaluate_h_parts_shuffles_bn254 if parts_form else L.h2hip_evaluate_h_shuffles_bn254
    assert fn(holder.byref(), ctypes.byref(_sh_holder(sy).desc), shuf.ctypes.data_as(ctypes.c_void_p)) == 0, L.h2hip_last_error()
    assert not np.array_equal(shuf, plain)
    assert _run(h2, sy, entry, sy.vin, mv=None).tobytes() == shuf.tobytes()
    assert _run(h2, sy, entry, sy.vin, mv=MvLookupsHolder([])).tobytes() == shuf.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_live,lo,hi", [(2, 1, 4), (6, 5, 8), (12, 9, 16), (40, 17, 64), (100, 65, 256), (6, 0, 0)],
                         ids=["tier4", "tier8", "tier16", "tier64", "tier256", "global"])
def test_gpu_graphs_in_every_slot_tier(h2, oracle, n_live, lo, hi):
    """slots live in LDS (up to 4 / 8), per-lane scratch (16 / 64 / 256) or the global workspace: an argument whose second input keeps
    n_live products alive at once runs its K + 1 programs in that tier -- the single-slot programs beside it too"""
    h2.init()
    mv = ((((A(0),), _many_live_tuple(n_live)), (F(0),)),)  # hashable: the system is cached
    sy = _system(oracle, 4, 5, 450 + n_live, "alone", mv_override=mv)
    slots = [_compile_stats(h2, flatten_graph(g))[1] for g in sy.ev.mv_lookups[0]]
    L = h2.lib()
    try:
        if hi == 0:
            L.h2hip_debug_set_evalh_max_local_slots(0)
        else:
            assert lo <= max(slots) <= hi and min(slots) <= 4, slots
        want = _want(h2, oracle, sy)
        for entry in ("full_host", "parts_device"):
            assert np.array_equal(_run(h2, sy, entry, sy.vin), want), entry
    finally:
        L.h2hip_debug_set_evalh_max_local_slots(256)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_more_arguments_than_a_coset_group(h2, oracle, entry):
    """three arguments, one pair of cosets per group: each group's cosets are formed in the buffers the one before used"""
    h2.init()
    sy = _system(oracle, 4, 5, 417, "with_all", 3)
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
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_a_coset_group_with_a_remainder(h2, oracle, entry):
    """group bytes of four columns of the form under test: the three mv-lookup arguments (two cosets each) run as a group of two and a
    group of one, the two shuffles (one coset each) share a group and the lookup (three cosets) is a group of one"""
    h2.init()
    sy = _system(oracle, 4, 5, 417, "with_all", 3)
    want = _want(h2, oracle, sy)
    column = 32 << (5 if entry.startswith("parts") else 7)
    L = h2.lib()
    L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(4 * column))
    try:
        got = _run(h2, sy, entry, sy.vin)
    finally:
        L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_profile_intervals_per_stage(h2, oracle):
    """the intervals the bench tools divide: one of the gates, the permutation and the lookups per pass (the lookups' holds the transforms
    of their later groups), one per mv-lookup argument and per shuffle (the transforms of their groups excluded); a pass per call in the
    full form and per part (P = 4) in the parts form, whatever the grouping"""
    h2.init()
    sy = _system(oracle, 4, 5, 417, "with_all", 3)
    want = _want(h2, oracle, sy)
    stages = ("evalh_gates", "evalh_perm", "evalh_lookups", "evalh_mvlookups", "evalh_shuffles")
    L = h2.lib()
    h2.profile_enable(True)
    try:
        for entry, passes in (("full_host", 1), ("parts_host", 4)):
            for group_bytes in (0, 1):
                L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(group_bytes))
                h2.profile_reset()
                assert np.array_equal(_run(h2, sy, entry, sy.vin), want)
                counts = [h2.profile_get(stage)[1] for stage in stages]
                print(entry, group_bytes, counts)
                assert counts == [passes, passes, passes, 3 * passes, 2 * passes], (entry, group_bytes)
    finally:
        L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))
        h2.profile_enable(False)
        h2.profile_reset()


@pytest.mark.gpu
def test_gpu_two_instances_then_t_evaluations(h2, oracle):
    """two circuit instances chained through values in both forms; t_evaluations on the last call of the parts form, applied after every
    stage, gives divide_by_vanishing_poly of the two-instance h"""
    h2.init()
    s1, s2 = _system(oracle, 4, 5, 405, "with_all"), _system(oracle, 4, 5, 406, "alone")
    h1 = _want(h2, oracle, s1)
    h_two = _model(h2, oracle, s2, h1)
    assert np.array_equal(_run(h2, s2, "full_host", _run(h2, s1, "full_host", s1.vin)), h_two)
    assert np.array_equal(_run(h2, s2, "parts_host", _run(h2, s1, "parts_host", s1.vin)), h_two)
    want = oracle.divide_by_vanishing_poly(s1.d, s1.t_eval, h_two)
    assert np.array_equal(_run(h2, s2, "parts_host", h1, t_evaluations=s1.t_eval), want)
    assert np.array_equal(_run(h2, s2, "parts_device", h1, t_evaluations=s1.t_eval), want)
    s3 = _system(oracle, 4, 5, 405, "with_all")  # shuffles behind the mv-lookups: t_evaluations still multiplies last
    assert np.array_equal(_run(h2, s3, "parts_host", s3.vin, t_evaluations=s3.t_eval), oracle.divide_by_vanishing_poly(s3.d, s3.t_eval, h1))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["parts_host", "parts_device"])
def test_gpu_part_ranges_split_one_h(h2, oracle, entry):
    """part 0 in one call, parts 1 .. P - 1 in another: rows of the other parts keep what they held, together they are the whole"""
    h2.init()
    sy = _system(oracle, 4, 5, 405, "with_all")
    want = _want(h2, oracle, sy)
    P = 4
    first = _run(h2, sy, entry, sy.vin, part_begin=0, part_count=1)
    assert np.array_equal(first[0::P], want[0::P])
    for p in range(1, P):
        assert np.array_equal(first[p::P], sy.vin[p::P]), p
    both = _run(h2, sy, entry, first, part_begin=1, part_count=P - 1)
    assert np.array_equal(both, want)


@pytest.mark.gpu
def test_gpu_pinned_part_cosets_present(h2, oracle):
    """the key's polynomials pinned as part cosets: the parts form serves them from the pin and the mv-lookup stage is unchanged"""
    h2.init()
    sy = _system(oracle, 4, 5, 405, "with_all")
    want = _want(h2, oracle, sy)
    dom = h2.EvaluationDomain.new(sy.j, sy.k)
    p = sy.parts
    key = [np.array(a) for a in p["fixed_polys"] + [p["l0_poly"], p["l_last_poly"], p["l_active_row_poly"]] + p["perm_polys"]]
    pinned = dict(p, fixed_polys=key[:3], l0_poly=key[3], l_last_poly=key[4], l_active_row_poly=key[5], perm_polys=key[6:])
    sp = types.SimpleNamespace(**{**vars(sy), "parts": pinned})
    h2.part_cosets_pin(key, dom)
    try:
        assert h2.part_cosets_pinned_info()[0] == len(key)
        assert np.array_equal(_run(h2, sp, "parts_host", sy.vin), want)
        assert h2.evalh_parts_stats()[1] == len(key) * 4  # every part served each of them from the pin
    finally:
        h2.part_cosets_unpin(key)
    assert np.array_equal(_run(h2, sp, "parts_host", sy.vin), want)
    assert h2.evalh_parts_stats()[1] == 0


@pytest.mark.gpu
def test_gpu_python_wrapper(h2, oracle):
    """Evaluator.evaluate_h / evaluate_h_parts take the stage from the case's "mvlookups" entry; without it they are the existing calls"""
    h2.init()
    sy = _system(oracle, 4, 5, 405, "with_all")
    want = _want(h2, oracle, sy)
    strip = lambda case: {**case, "lookups": [l[1:] for l in case["lookups"]]}  # noqa: E731  (the graphs are the Evaluator's)
    pairs = list(zip(sy.phi, sy.m))
    assert np.array_equal(sy.ev.evaluate_h({**strip(sy.full), "mvlookups": pairs, "shuffles": sy.z}, np.array(sy.vin)), want)
    assert np.array_equal(sy.ev.evaluate_h_parts({**strip(sy.parts), "mvlookups": pairs, "shuffles": sy.z}, np.array(sy.vin)), want)
    got = sy.ev.evaluate_h_parts({**strip(sy.parts), "mvlookups": pairs, "shuffles": sy.z}, np.array(sy.vin), t_evaluations=sy.t_eval)
    assert np.array_equal(got, oracle.divide_by_vanishing_poly(sy.d, sy.t_eval, want))
    with pytest.raises(ValueError):
        sy.ev.evaluate_h({**strip(sy.full), "mvlookups": pairs[:1]}, np.array(sy.vin))
