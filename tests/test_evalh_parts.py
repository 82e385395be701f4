"""evaluate_h one coset of the 2^k domain at a time (h2hip_evaluate_h_parts_bn254[_device]): every case is built from random
coefficient-form polynomials; the oracle is fed the extended cosets oracle.coeff_to_extended makes of them and evaluates h(X) over the
whole extended domain, the engine is fed the polynomials.  Field elements are canonical, so every comparison is np.array_equal."""
import copy
import ctypes
import functools
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from evalh_util import (DescHolder, Evaluator, GraphEvaluator, PartsDescHolder, custom_gates_graph, evaluate_h_workspace_bytes, flatten_graph,
                        lookup_graph)

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
KEY_COLUMNS = (("fixed_polys", "fixed_cosets"), ("perm_product_polys", "perm_product_cosets"), ("perm_polys", "perm_cosets"))
KEY_SINGLES = (("l0_poly", "l0"), ("l_last_poly", "l_last"), ("l_active_row_poly", "l_active_row"))


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _case(oracle, j, k, seed, n_gates=3):
    """parts / full (the two forms' cases), vin (values on entry), want (the oracle's h), d, t_eval (the domain) and ev (the Evaluator
    the graphs were flattened from) of a synthetic system of test_evalh._random_case's shape -- instance
    column, challenges, mixed permutation column kinds, three sets with a ragged last chunk, two lookups, rotations in -2..2,
    last_rotation -6 -- over domain_new(j, k).  Built once per shape and shared: every array is read-only."""
    rng = np.random.default_rng(seed)
    n = 1 << k
    d, t_eval = oracle.domain_new(j, k)
    size = 1 << d.extended_k
    col = lambda s: _ro(oracle.gen_scalars(seed * 1000 + s, n))  # noqa: E731
    ext = lambda poly: _ro(oracle.coeff_to_extended(d, poly, 4))  # noqa: E731
    A = lambda c, r=0: ('advice', c, r)  # noqa: E731
    F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
    I = lambda c, r=0: ('instance', c, r)  # noqa: E731
    gates = []
    for gi in range(n_gates):
        a, b, c = (int(x) for x in rng.integers(0, 5, 3))
        f1, f2 = (int(x) for x in rng.integers(0, 6, 2))
        r1, r2 = (int(x) for x in rng.integers(-2, 3, 2))
        gates.append(('sum', ('prod', ('prod', A(a, r1), A(b)), F(f1)),
                      ('sum', ('neg', ('prod', A(c, r2), F(f2, r1))), ('scaled', ('sum', I(0), ('challenge', 0)), 3 + gi))))
    ev = Evaluator(custom_gates_graph(gates), [lookup_graph([A(li), ('prod', A(li + 1), F(li))], [F(5), F(li + 2, 1)]) for li in range(2)])
    lookups = [(flatten_graph(lg), col(50 + 3 * li), col(51 + 3 * li), col(52 + 3 * li)) for li, lg in enumerate(ev.lookups)]
    scalars = oracle.gen_scalars(seed * 1000 + 1, 6)
    parts = {
        "k": k, "extended_k": d.extended_k, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
        "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
        "y": scalars[0], "beta": scalars[1], "gamma": scalars[2], "theta": scalars[3], "challenges": scalars[4:6],
        "l0_poly": col(5), "l_last_poly": col(6), "l_active_row_poly": col(7),
        "fixed_polys": [col(10 + i) for i in range(6)], "advice_polys": [col(20 + i) for i in range(5)], "instance_polys": [col(30)],
        "custom": flatten_graph(ev.custom_gates),
        "perm_product_polys": [col(40 + i) for i in range(3)], "perm_polys": [col(44 + i) for i in range(5)],
        "perm_column_kind": np.array([0, 0, 1, 2, 0], dtype=np.uint32), "perm_column_index": np.array([1, 2, 3, 0, 4], dtype=np.uint32),
        "chunk_len": 2, "last_rotation": -6, "lookups": lookups,
    }
    full = _full_of(parts, ext)
    vin = _ro(oracle.gen_scalars(seed * 1000 + 99, size))  # nonzero on entry: an earlier instance's h
    return types.SimpleNamespace(parts=parts, full=full, vin=vin, want=_ro(_oracle_h(oracle, full, vin)), d=d, t_eval=t_eval, ev=ev)


def _full_of(parts, ext):
    """the full form's case: the key's polynomials as the extended cosets the oracle makes of them"""
    full = {key: v for key, v in parts.items() if not key.endswith("_polys") and not key.endswith("_poly")}
    for p_name, f_name in KEY_COLUMNS:
        full[f_name] = [ext(p) for p in parts[p_name]]
    for p_name, f_name in KEY_SINGLES:
        full[f_name] = ext(parts[p_name])
    full["advice_polys"], full["instance_polys"] = parts["advice_polys"], parts["instance_polys"]
    return full


def _oracle_h(oracle, full, vin):
    out = np.array(vin, dtype=np.uint64)
    assert oracle.lib().oracle_evaluate_h(DescHolder(full).byref(), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def _run_parts(h2, case, vin, **extra):
    """the host-pointer entry point on a copy of vin"""
    holder = PartsDescHolder({**case, **extra})
    got = np.array(vin, dtype=np.uint64)
    rc = h2.lib().h2hip_evaluate_h_parts_bn254(holder.byref(), got.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, h2.lib().h2hip_last_error()
    return got


@pytest.fixture(params=["interpreter", "generated"])
def gates_kernel(request, h2):
    """as tests/test_evalh.py's fixture: the test runs once through the byte-code interpreter and once through the kernels generated for
    the circuit and compiled inline, and the counters must show which one ran"""
    L = h2.lib()
    h2.init()
    before = (ctypes.c_uint64 * 5)()
    L.h2hip_debug_evalh_codegen_stats(before)
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(0 if request.param == "interpreter" else 2), ctypes.c_uint32(0))
    mode = {"kind": request.param, "expect_generated": request.param == "generated"}
    yield mode
    after = (ctypes.c_uint64 * 5)()
    L.h2hip_debug_evalh_codegen_stats(after)
    L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
    if request.param == "generated":
        assert after[1] == before[1], "hiprtc rejected a generated kernel: " + L.h2hip_last_error().decode()
        if mode["expect_generated"]:
            assert after[2] > before[2], "the generated kernel never ran"
    else:
        assert after[2] == before[2]


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("j", [3, 4, 9])
def test_oracle_part_identity(oracle, j):
    """coeff_to_extended(f)[p::P] == best_fft(f . powers(g_p), omega) with g_p = zeta extended_omega^p, for (k, extended_k) = (4, 5),
    (4, 6), (4, 7) and every p: the decomposition the engine relies on, pinned on the oracle before the oracle judges the engine"""
    from evalh_util import to_mont_limbs
    k = 4
    d, _ = oracle.domain_new(j, k)
    assert d.extended_k == {3: 5, 4: 6, 9: 7}[j]
    P, n = 1 << (d.extended_k - k), 1 << k
    canon = lambda name: oracle.int_from_limbs(oracle.fe_to_canonical(oracle.FR, d.fe(name).reshape(1, 4))[0])  # noqa: E731
    zeta, w_e = canon("g_coset"), canon("extended_omega")
    assert pow(w_e, P, R_MOD) == canon("omega") and pow(zeta, 3, R_MOD) == 1
    f = oracle.gen_scalars(4242 + j, n)
    whole = oracle.coeff_to_extended(d, f)
    for p in range(P):
        g_p = zeta * pow(w_e, p, R_MOD) % R_MOD
        scaled = oracle.fe_binop("mul", oracle.FR, f, to_mont_limbs([pow(g_p, m, R_MOD) for m in range(n)]))
        assert np.array_equal(whole[p::P], oracle.best_fft(scaled, d.fe("omega"), k)), p


def _set_table_entry_null(holder, field, index):
    table = ctypes.cast(getattr(holder.desc, field), ctypes.POINTER(ctypes.c_void_p))
    table[index] = None


def test_parts_rejects_malformed_descriptions(h2, oracle):
    """a description a kernel could fault on is H2HIP_EINVAL before any device work (no GPU needed): the full form's list, a null
    polynomial in any table, a part range beyond P, extended_k < k"""
    L = h2.lib()
    c0 = _case(oracle, 4, 4, 7)
    case, vin = c0.parts, c0.vin

    def rc_of(mutate=None, poke=None):
        c = copy.deepcopy(case)
        if mutate:
            mutate(c)
        h = PartsDescHolder(c)
        if poke:
            poke(h)
        v = np.array(vin)
        return L.h2hip_evaluate_h_parts_bn254(h.byref(), v.ctypes.data_as(ctypes.c_void_p))

    def bad_target(c): c["custom"]["calcs"][0, 1] = 10_000
    def bad_column(c): c["custom"]["calcs"][0, 3] = 99
    def bad_rotation(c): c["custom"]["calcs"][0, 4] = 99
    def bad_parts(c): c["custom"]["calcs"][-1, 9] = 1000
    def bad_op(c): c["custom"]["calcs"][0, 0] = 8
    def rewritten_target(c): c["custom"]["calcs"][1, 1] = c["custom"]["calcs"][0, 1]
    def read_before_write(c): c["custom"]["calcs"][0, 2:5] = (1, c["custom"]["calcs"][-1, 1], 0)
    def bad_perm_col(c): c["perm_column_index"] = np.array([0, 1, 77, 0, 0], dtype=np.uint32)
    def few_sets(c): c["chunk_len"] = 1
    def bad_domain(c): c["extended_k"] = 2      # extended_k < k
    def bad_lookup(c): c["lookups"][0][0]["calcs"][0, 3] = 99
    def range_past_p(c): c["part_begin"], c["part_count"] = 3, 2   # P = 4
    def begin_past_p(c): c["part_begin"], c["part_count"] = 4, 1
    def begin_without_count(c): c["part_begin"], c["part_count"] = 1, 0

    for m in (bad_target, bad_column, bad_rotation, bad_parts, bad_op, rewritten_target, read_before_write, bad_perm_col, few_sets, bad_domain,
              bad_lookup, range_past_p, begin_past_p, begin_without_count):
        assert rc_of(m) == 1, m.__name__
        assert b"evaluate_h" in L.h2hip_last_error(), m.__name__
    for field, index in (("fixed_polys", 5), ("advice_polys", 0), ("instance_polys", 0), ("perm_product_polys", 2), ("perm_polys", 4),
                         ("lookup_product_polys", 1), ("lookup_permuted_input_polys", 0), ("lookup_permuted_table_polys", 1)):
        assert rc_of(poke=lambda h: _set_table_entry_null(h, field, index)) == 1, field
        assert b"evaluate_h" in L.h2hip_last_error(), field
    for field in ("l0_poly", "l_last_poly", "l_active_row_poly", "fixed_polys", "perm_polys", "lookup_product_polys"):
        assert rc_of(poke=lambda h: setattr(h.desc, field, None)) == 1, field
        assert b"evaluate_h" in L.h2hip_last_error(), field
    assert L.h2hip_evaluate_h_parts_bn254(None, None) == 1
    assert L.h2hip_evaluate_h_parts_bn254_device(None, None, None) == 1
    assert L.h2hip_evaluate_h_parts_bn254(PartsDescHolder(case).byref(), None) == 1


@pytest.mark.parametrize("ek", [22, 23])
def test_workspace_bytes_of_the_bench_shape(h2, ek):
    """h2hip_evaluate_h_workspace_bytes on the bench system (6 fixed, 5 advice, 1 instance, 3 permutation sets over 5 columns, 2 lookups) at
    k = 20: the parts form keeps one part's coset of every column, of 2^k elements, and the part's rows of values; the full form keeps
    every column of the description at 2^extended_k.  The 2 GB a group of lookup cosets may take hold both lookups at either size."""
    k, nf, na, ni, ns, nc, nl = 20, 6, 5, 1, 3, 5, 2
    P = 1 << (ek - k)
    q = lambda parts, dev: evaluate_h_workspace_bytes(k, ek, nf, na, ni, ns, nc, nl, parts, dev)  # noqa: E731
    col, part = 32 << ek, 32 << k
    columns = nf + na + ni + 3 + ns + nc + 3 * nl  # every column of the description: fixed, advice, instance, l0 / l_last / l_active, z, sigma, lookups
    # the full form: what evaluate_h_host asks its arena for behind the metadata, (columns + values) x (2^ek elements + 256) + 4096 with host
    # pointers, and only the cosets it forms itself (advice, instance, lookups) with device pointers
    assert q(False, False) == (columns + 1) * (col + 256) + 4096
    assert q(False, True) == (na + ni + 3 * nl) * (col + 256) + 4096
    # the parts form, device pointers: nothing but one part's cosets and its rows of values -- exactly 1 / P of the columns (and values)
    # the full form would need resident; there is no copy of values to subtract
    resident_full = (columns + 1) * col
    assert q(True, True) == (columns + 1) * part
    assert q(True, True) * P <= resident_full
    # host pointers add the uploaded coefficient columns (once each, 2^k elements) and the copy of values
    values_copy = col
    assert q(True, False) - values_copy == (columns + 1) * part + columns * part
    assert (q(True, False) - values_copy) * P <= 2 * resident_full
    with pytest.raises(h2.H2HipError):
        evaluate_h_workspace_bytes(21, 20, nf, na, ni, ns, nc, nl, True, True)
    assert b"evaluate_h" in h2.lib().h2hip_last_error()


def test_cpp_parts_mirror_builds():
    """the Makefile target of the C++ test program of Evaluator::evaluate_h_parts (halo2-pse_amd/host/evaluation.hpp)"""
    target = os.path.join("..", "tests", "cpp", "test_evalh_parts_mirror")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_evalh_parts_mirror"))


def _header_parts_fields():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo2hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct h2hip_evalh_parts_desc \{(.*?)\}\s*h2hip_evalh_parts_desc;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *rest = [x.strip() for x in decl.split(",")]
        m = re.match(r"^(.*?)([a-z_0-9]+)$", first)
        base, stars = m.group(1).strip(), ""
        while base.endswith("*"):
            base, stars = base[:-1].strip(), stars + "*"
        fields.append((m.group(2), base + stars))
        fields += [(r.lstrip("*"), base + "*" * (len(r) - len(r.lstrip("*")))) for r in rest]
    return fields


def test_parts_desc_mirrors_match_the_header():
    """h2hip_evalh_parts_desc field for field, in order and with matching types, in the ctypes mirror and in halo2hip-sys/src/evalh.rs
    (EvalhPartsDesc); its leading fields are h2hip_evalh_desc's, which tests/test_binding.py holds to the header"""
    from evalh_util import EvalhDesc, EvalhPartsDesc
    c2r = {"uint32_t": "u32", "int32_t": "i32", "const uint64_t*": "*const u64", "const uint32_t*": "*const u32",
           "const uint64_t* const*": "*const *const u64", "const h2hip_graph*": "*const h2hip_graph", "h2hip_graph": "h2hip_graph"}
    fields = _header_parts_fields()
    assert [n for n, _ in fields] == [n for n, _ in EvalhPartsDesc._fields_]
    assert [t for _, t in EvalhPartsDesc._fields_][:len(EvalhDesc._fields_)] == [t for _, t in EvalhDesc._fields_]
    assert [n for n, _ in fields[len(EvalhDesc._fields_):]] == ["part_begin", "part_count", "t_evaluations"]
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "halo2hip-sys", "src", "evalh.rs")).read())
    body = re.search(r"#\[repr\(C\)\][^{]*?pub struct EvalhPartsDesc \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert [(n, " ".join(t.split())) for n, t in re.findall(r"pub ([a-z_0-9]+): ([^,\n]+),", body)] == [(n, c2r[t]) for n, t in fields]
    assert "ffi::h2hip_evaluate_h_parts_bn254(" in rust and "pub fn try_evaluate_h_parts" in rust


# ---------------------------------------------------------------------------------------------------------------- GPU
def _k_above_lo_bits(h2, oracle):
    """the smallest k whose 2^k domain's power table has a second level, read from the engine's own tables"""
    h2.init()
    bits = ctypes.c_uint32()
    d, _ = oracle.domain_new(4, 20)
    assert h2.lib().h2hip_debug_evalh_power_table_bits(d.fe("omega").ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(20), ctypes.byref(bits)) == 0
    k = bits.value + 1
    dk, _ = oracle.domain_new(4, k)
    assert h2.lib().h2hip_debug_evalh_power_table_bits(dk.fe("omega").ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(k), ctypes.byref(bits)) == 0
    assert bits.value < k <= 14, "rows at or beyond 2^lo_bits take pow_hi in the permutation kernel"
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("j,k", [(3, 5), (4, 5), (9, 5), (3, 9), (4, 9), (9, 9), (4, None)])
def test_gpu_parts_vs_oracle(h2, oracle, j, k, gates_kernel):
    """P = 2, 4, 8 at k = 5 and 9, and P = 4 at the first k whose permutation kernel reads pow_hi: the engine on the polynomials == the
    oracle on their cosets, with nonzero values on entry, under both gates kernels"""
    if k is None:
        k = _k_above_lo_bits(h2, oracle)
    c = _case(oracle, j, k, 100 * j + k)
    assert np.array_equal(_run_parts(h2, c.parts, c.vin), c.want)


@pytest.mark.gpu
@pytest.mark.parametrize("j", [3, 9])
def test_gpu_part_ranges(h2, oracle, j):
    """part 0, parts 1 .. P - 1, and all of them: rows of other parts keep what they held, and the two ranges together are the whole"""
    h2.init()
    c = _case(oracle, j, 5, 100 * j + 5)
    case, vin, want = c.parts, c.vin, c.want
    P = 1 << (c.d.extended_k - 5)
    first = _run_parts(h2, case, vin, part_begin=0, part_count=1)
    assert np.array_equal(first[0::P], want[0::P])
    for p in range(1, P):
        assert np.array_equal(first[p::P], vin[p::P]), p  # the entry values serve as the sentinel: random, so no row of h equals them
    rest = _run_parts(h2, case, vin, part_begin=1, part_count=P - 1)
    assert np.array_equal(rest[0::P], vin[0::P])
    for p in range(1, P):
        assert np.array_equal(rest[p::P], want[p::P]), p
    both = _run_parts(h2, case, first, part_begin=1, part_count=P - 1)
    assert np.array_equal(both, want)
    assert np.array_equal(_run_parts(h2, case, vin, part_begin=0, part_count=P), want)
    assert not np.array_equal(want[0::P], vin[0::P])


@pytest.mark.gpu
def test_gpu_two_instances_then_divide_and_extended_to_coeff(h2, oracle):
    """two instances chained through values, t_evaluations on the second call only: the result is divide_by_vanishing_poly of the
    oracle's two-instance h, and through extended_to_coeff it is the oracle's h(X) in coefficient form"""
    h2.init()
    c1, c2 = _case(oracle, 4, 5, 405), _case(oracle, 4, 5, 406)
    first, second, vin, h1, d, t_eval = c1.parts, c2.parts, c1.vin, c1.want, c1.d, c1.t_eval
    h_two = _oracle_h(oracle, c2.full, h1)
    want = oracle.divide_by_vanishing_poly(d, t_eval, h_two)
    got = _run_parts(h2, second, _run_parts(h2, first, vin), t_evaluations=t_eval)
    assert np.array_equal(got, want)
    assert np.array_equal(_run_parts(h2, second, h1), h_two)  # without t_evaluations the rows leave as they are
    dom = h2.EvaluationDomain.new(4, 5)
    assert np.array_equal(dom.t_evaluations, t_eval)
    assert np.array_equal(dom.extended_to_coeff(got), oracle.extended_to_coeff(d, want, 4))


def _device_tables(case, names, keep):
    """every column of `case` under `names` as a torch tensor in HBM; returns {name: tensor or list}, and a function that writes the
    device addresses into a description built from the host case"""
    import torch
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731  (a copy: the shared arrays are read-only)
    tens = {name: ([dev(a) for a in case[name]] if isinstance(case[name], list) else dev(case[name])) for name in names}
    tens["lookups"] = [[dev(p) for p in l[1:]] for l in case["lookups"]]

    def table(ts):
        arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        keep.append(arr)
        return ctypes.addressof(arr)

    def apply(desc):
        for name in names:
            setattr(desc, name, table(tens[name]) if isinstance(tens[name], list) else tens[name].data_ptr())
        desc.lookup_product_polys = table([l[0] for l in tens["lookups"]])
        desc.lookup_permuted_input_polys = table([l[1] for l in tens["lookups"]])
        desc.lookup_permuted_table_polys = table([l[2] for l in tens["lookups"]])

    return tens, apply


@pytest.mark.gpu
def test_gpu_parts_device_form(h2, oracle, gates_kernel):
    """h2hip_evaluate_h_parts_bn254_device: columns and values in HBM, kernels queued on the caller's stream, inputs bit-identical
    afterwards.  In one run the full-form _device call is queued first and, with no synchronisation in between, the parts form on the
    same stream -- both share the engine's arena -- and both equal the oracle; so does the host-pointer parts form."""
    import torch
    L = h2.lib()
    c = _case(oracle, 4, 9, 409)
    case, full, vin, want = c.parts, c.full, c.vin, c.want
    keep = []
    names_p = ["fixed_polys", "advice_polys", "instance_polys", "perm_product_polys", "perm_polys", "l0_poly", "l_last_poly", "l_active_row_poly"]
    names_f = ["fixed_cosets", "advice_polys", "instance_polys", "perm_product_cosets", "perm_cosets", "l0", "l_last", "l_active_row"]
    tens_p, apply_p = _device_tables(case, names_p, keep)
    tens_f, apply_f = _device_tables(full, names_f, keep)

    def flat(v):
        return [t for x in (v.values() if isinstance(v, dict) else v) for t in flat(x)] if isinstance(v, (dict, list)) else [v]

    before = [t.clone() for t in flat(tens_p)]
    hp, hf = PartsDescHolder(case), DescHolder(full)
    apply_p(hp.desc)
    apply_f(hf.desc)
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731  (a copy: the shared arrays are read-only)
    v_full, v_parts = dev(vin), dev(vin)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc_f = L.h2hip_evaluate_h_bn254_device(hf.byref(), ctypes.c_void_p(v_full.data_ptr()), stream)
    rc_p = L.h2hip_evaluate_h_parts_bn254_device(hp.byref(), ctypes.c_void_p(v_parts.data_ptr()), stream)
    assert rc_f == 0 and rc_p == 0, L.h2hip_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(v_parts.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(v_full.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(_run_parts(h2, case, vin), want)
    for t0, t1 in zip(before, flat(tens_p)):
        assert torch.equal(t0, t1)  # inputs are read-only


def _strip(case, perm=True, lookups=True):
    c = dict(case)
    if not perm:
        for name in ("perm_product_polys", "perm_polys", "perm_product_cosets", "perm_cosets"):
            if name in c:
                c[name] = []
        c["perm_column_kind"] = np.zeros(0, dtype=np.uint32)
        c["perm_column_index"] = np.zeros(0, dtype=np.uint32)
    if not lookups:
        c["lookups"] = []
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["no_perm", "no_lookups", "gates_only", "empty_graph", "horner_without_parts"])
def test_gpu_parts_degenerate_systems(h2, oracle, variant, gates_kernel):
    """the five variants of test_gpu_evaluate_h_degenerate_systems: no permutation argument, no lookups, neither, a graph without
    calculations (every row becomes zero), a Horner without parts (values unchanged)"""
    c = _case(oracle, 4, 6, 10)
    case, full, vin = c.parts, c.full, c.vin
    if variant in ("horner_without_parts", "empty_graph"):
        perm = lookups = False
        custom = flatten_graph(custom_gates_graph([]) if variant == "horner_without_parts" else GraphEvaluator())
        if variant == "empty_graph":
            gates_kernel["expect_generated"] = False  # no operations: nothing to generate
    else:
        perm, lookups, custom = variant not in ("no_perm", "gates_only"), variant not in ("no_lookups", "gates_only"), case["custom"]
    case, full = {**_strip(case, perm, lookups), "custom": custom}, {**_strip(full, perm, lookups), "custom": custom}
    want = _oracle_h(oracle, full, vin)
    if variant == "horner_without_parts":
        assert np.array_equal(want, vin)
    if variant == "empty_graph":
        assert not want.any()
    assert np.array_equal(_run_parts(h2, case, vin), want)


@pytest.mark.gpu
def test_gpu_parts_lookup_groups_of_one(h2, oracle, gates_kernel):
    """one lookup per group of coset buffers: every part forms the second lookup's cosets after the first lookup's kernel, in the
    buffers the first one used"""
    c = _case(oracle, 4, 9, 409)
    case, vin, want = c.parts, c.vin, c.want
    h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(1))
    try:
        got = _run_parts(h2, case, vin)
    finally:
        h2.lib().h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_parts_global_slot_workspace(h2, oracle):
    """every program pushed through the global-workspace form of the kernels (rows taken grid-stride), as
    test_gpu_evaluate_h_global_slot_workspace forces it"""
    h2.init()
    c = _case(oracle, 4, 9, 409)
    case, vin, want = c.parts, c.vin, c.want
    L = h2.lib()
    try:
        L.h2hip_debug_set_evalh_max_local_slots(0)
        got = _run_parts(h2, case, vin)
    finally:
        L.h2hip_debug_set_evalh_max_local_slots(256)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_python_wrapper(h2, oracle):
    """Evaluator.evaluate_h_parts, the package's own entry: the Evaluator flattens its graphs, a part range and t_evaluations are passed on"""
    h2.init()
    c = _case(oracle, 3, 5, 305)
    case = {**c.parts, "lookups": [l[1:] for l in c.parts["lookups"]]}  # the polynomials alone: the graphs are the Evaluator's
    got = c.ev.evaluate_h_parts(case, np.array(c.vin), parts=(1, 1))
    assert np.array_equal(got[1::2], c.want[1::2]) and np.array_equal(got[0::2], c.vin[0::2])
    got = c.ev.evaluate_h_parts(case, np.array(c.vin), t_evaluations=c.t_eval)
    assert np.array_equal(got, oracle.divide_by_vanishing_poly(c.d, c.t_eval, c.want))


@pytest.mark.gpu
def test_gpu_cpp_parts_mirror():
    """tests/cpp/test_evalh_parts_mirror: the C++ mirror's evaluate_h_parts against its evaluate_h, P = 2 and 8"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_evalh_parts_mirror")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "evalh parts mirror tests ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
