"""Pinned part cosets (h2hip_part_cosets_pin[_device]) under the parts form of evaluate_h: with any subset of the proving key's polynomials
pinned the call computes, limb for limb, what it computes with none pinned and what the full form computes (the oracle's h over the
extended cosets), and h2hip_debug_evalh_parts_stats shows that the pins were used -- without it a call that ignored the cache would pass.

The systems are test_evalh_parts' (instance column, challenges, mixed permutation column kinds, three sets, two lookups) at k = 5 and 8
with P = 4 and 8.  Key columns: 6 fixed + l0 / l_last / l_active_row + 5 permutation polynomials = 14; witness columns: 5 advice +
1 instance + 3 permutation products + 2 x 3 lookup columns = 15."""
import ctypes
import gc

import numpy as np
import pytest

from evalh_util import PartsDescHolder
from test_evalh_parts import _case, _device_tables, _full_of, _oracle_h, _run_parts

N_KEY, N_WITNESS, N_FIXED = 14, 15, 6
SHAPES = [(4, 5), (9, 5), (4, 8), (9, 8)]  # (j, k): P = 4 and 8


def _key(case, fixed_only=False):
    if fixed_only:
        return list(case["fixed_polys"])
    return list(case["fixed_polys"]) + [case["l0_poly"], case["l_last_poly"], case["l_active_row_poly"]] + list(case["perm_polys"])


def _writable(case):
    """the case with key arrays of its own: the shared ones are read-only and cached across tests, pins are keyed by address"""
    c = dict(case)
    c["fixed_polys"] = [np.array(a) for a in case["fixed_polys"]]
    c["perm_polys"] = [np.array(a) for a in case["perm_polys"]]
    for name in ("l0_poly", "l_last_poly", "l_active_row_poly"):
        c[name] = np.array(case[name])
    return c


@pytest.fixture
def clean_pins(h2):
    h2.init()
    assert h2.part_cosets_pinned_info() == (0, 0)
    yield
    gc.collect()
    assert h2.part_cosets_pinned_info() == (0, 0), "a test left part cosets pinned"


@pytest.mark.gpu
@pytest.mark.parametrize("j,k", SHAPES, ids=[f"P{8 if j == 9 else 4}-k{k}" for j, k in SHAPES])
def test_host_form_pinned_equals_unpinned_and_full(h2, oracle, j, k, clean_pins):
    c = _case(oracle, j, k, 100 * j + k)
    case, vin, want = _writable(c.parts), c.vin, c.want
    dom = h2.EvaluationDomain.new(j, k)
    ek, n = dom.extended_k, 1 << k
    P = 1 << (ek - k)
    assert P == (8 if j == 9 else 4)
    # none pinned
    assert np.array_equal(_run_parts(h2, case, vin), want)
    t0, s0, up0, arena0 = h2.evalh_parts_stats()
    assert (t0, s0) == ((N_KEY + N_WITNESS) * P, 0) and up0 == (N_KEY + N_WITNESS) * n * 32
    # the whole key pinned
    h2.part_cosets_pin(_key(case), dom)
    assert h2.part_cosets_pinned_info() == (N_KEY, N_KEY * (32 << ek))
    h2.part_cosets_pin(_key(case), dom)  # idempotent
    assert h2.part_cosets_pinned_info() == (N_KEY, N_KEY * (32 << ek))
    assert np.array_equal(_run_parts(h2, case, vin), want)
    t1, s1, up1, arena1 = h2.evalh_parts_stats()
    assert (t1, s1) == (N_WITNESS * P, N_KEY * P)
    assert up1 == N_WITNESS * n * 32  # the witness columns alone cross
    # a pinned column takes no coset slot (n x 32 bytes, as in the device form) and, in the host form, no coefficient slot either
    assert arena0 - arena1 == 2 * N_KEY * n * 32
    # part ranges that together cover all parts, t_evaluations on the last call of the chain
    first = _run_parts(h2, case, vin, part_begin=0, part_count=1)
    assert h2.evalh_parts_stats()[:2] == (N_WITNESS, N_KEY)
    assert np.array_equal(first[0::P], want[0::P]) and all(np.array_equal(first[p::P], vin[p::P]) for p in range(1, P))
    both = _run_parts(h2, case, first, part_begin=1, part_count=P - 1)
    assert h2.evalh_parts_stats()[:2] == (N_WITNESS * (P - 1), N_KEY * (P - 1))
    assert np.array_equal(both, want)
    assert np.array_equal(_run_parts(h2, case, vin, t_evaluations=c.t_eval), oracle.divide_by_vanishing_poly(c.d, c.t_eval, want))
    # unpin: the entries go, the next call is correct and serves nothing from pins
    h2.part_cosets_unpin(_key(case))
    assert h2.part_cosets_pinned_info() == (0, 0)
    assert np.array_equal(_run_parts(h2, case, vin), want)
    assert h2.evalh_parts_stats() == (t0, 0, up0, arena0)
    # only the fixed ones pinned: a partial pin is legal
    h2.part_cosets_pin(_key(case, fixed_only=True), dom)
    assert h2.part_cosets_pinned_info() == (N_FIXED, N_FIXED * (32 << ek))
    assert np.array_equal(_run_parts(h2, case, vin), want)
    t2, s2, up2, arena2 = h2.evalh_parts_stats()
    assert (t2, s2) == ((N_KEY + N_WITNESS - N_FIXED) * P, N_FIXED * P) and up2 == (N_KEY + N_WITNESS - N_FIXED) * n * 32
    assert arena0 - arena2 == 2 * N_FIXED * n * 32
    # a pin for another domain at the same addresses is not this call's
    other = h2.EvaluationDomain.new(3, k)
    h2.part_cosets_pin(_key(case, fixed_only=True), other)
    assert h2.part_cosets_pinned_info() == (N_FIXED, N_FIXED * (32 << other.extended_k))
    assert np.array_equal(_run_parts(h2, case, vin), want)
    assert h2.evalh_parts_stats()[1] == 0
    h2.part_cosets_unpin(_key(case))


@pytest.mark.gpu
@pytest.mark.parametrize("j,k", [(4, 5), (9, 8)], ids=["P4-k5", "P8-k8"])
def test_device_form_pinned_equals_unpinned_and_full(h2, oracle, j, k, clean_pins):
    """columns and values in HBM; the pins are keyed by the device addresses the description carries"""
    import torch
    L = h2.lib()
    c = _case(oracle, j, k, 100 * j + k)
    case, vin, want = c.parts, c.vin, c.want
    dom = h2.EvaluationDomain.new(j, k)
    ek, n = dom.extended_k, 1 << k
    P = 1 << (ek - k)
    keep = []
    names = ["fixed_polys", "advice_polys", "instance_polys", "perm_product_polys", "perm_polys", "l0_poly", "l_last_poly", "l_active_row_poly"]
    tens, apply = _device_tables(case, names, keep)
    key_all = tens["fixed_polys"] + [tens["l0_poly"], tens["l_last_poly"], tens["l_active_row_poly"]] + tens["perm_polys"]
    before = [t.clone() for t in key_all]

    def run(**extra):
        h = PartsDescHolder({**case, **extra})
        apply(h.desc)
        v = torch.from_numpy(np.array(vin, dtype=np.uint64).view(np.int64)).cuda()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.h2hip_evaluate_h_parts_bn254_device(h.byref(), ctypes.c_void_p(v.data_ptr()), stream) == 0, L.h2hip_last_error()
        torch.cuda.synchronize()
        return v.cpu().numpy().view(np.uint64)

    assert np.array_equal(run(), want)
    t0, s0, up0, arena0 = h2.evalh_parts_stats()
    assert (t0, s0, up0) == ((N_KEY + N_WITNESS) * P, 0, 0)
    for pinned, n_pin in ((key_all, N_KEY), (tens["fixed_polys"], N_FIXED)):
        h2.part_cosets_pin(pinned, dom)
        assert h2.part_cosets_pinned_info() == (n_pin, n_pin * (32 << ek))
        assert np.array_equal(run(), want)
        t1, s1, up1, arena1 = h2.evalh_parts_stats()
        assert (t1, s1, up1) == ((N_KEY + N_WITNESS - n_pin) * P, n_pin * P, 0)
        assert arena0 - arena1 == n_pin * n * 32
        first = run(part_begin=0, part_count=P - 1)
        assert np.array_equal(first[P - 1::P], vin[P - 1::P]) and all(np.array_equal(first[p::P], want[p::P]) for p in range(P - 1))
        assert np.array_equal(run(t_evaluations=c.t_eval), oracle.divide_by_vanishing_poly(c.d, c.t_eval, want))
        h2.part_cosets_unpin(pinned)
        assert h2.part_cosets_pinned_info() == (0, 0)
    assert np.array_equal(run(), want)
    assert h2.evalh_parts_stats() == (t0, 0, 0, arena0)
    for a, b in zip(before, key_all):
        assert torch.equal(a, b)  # a pin reads its source only


@pytest.mark.gpu
def test_guard_drops_a_rewritten_host_polynomial(h2, oracle, clean_pins):
    """element 0 of a pinned host polynomial overwritten: the call equals the unpinned result on the new data, and the entry is gone"""
    j, k = 4, 5
    c = _case(oracle, j, k, 100 * j + k)
    case = _writable(c.parts)
    dom = h2.EvaluationDomain.new(j, k)
    h2.part_cosets_pin(_key(case), dom)
    assert np.array_equal(_run_parts(h2, case, c.vin), c.want)
    case["fixed_polys"][0][0] = h2.BN254_FR.from_int(0xC0FFEE)
    want = _oracle_h(oracle, _full_of(case, lambda poly: oracle.coeff_to_extended(c.d, np.array(poly), 4)), c.vin)
    assert not np.array_equal(want, c.want)
    got = _run_parts(h2, case, c.vin)
    assert np.array_equal(got, want)
    P = 1 << (dom.extended_k - k)
    assert h2.evalh_parts_stats()[:2] == ((N_WITNESS + 1) * P, (N_KEY - 1) * P)
    assert h2.part_cosets_pinned_info() == (N_KEY - 1, (N_KEY - 1) * (32 << dom.extended_k))
    h2.part_cosets_unpin(_key(case))


@pytest.mark.gpu
def test_column_pin_and_part_pin_of_one_pointer_coexist(h2, oracle, clean_pins):
    """pk.permutation.polys[j] pinned both as a column of 2^k elements (for the opening calls) and as part cosets: eval_polynomials and
    the parts call are both correct, and unpinning either leaves the other"""
    j, k = 4, 5
    c = _case(oracle, j, k, 100 * j + k)
    case = _writable(c.parts)
    dom = h2.EvaluationDomain.new(j, k)
    P = 1 << (dom.extended_k - k)
    perm = case["perm_polys"]
    points = oracle.gen_scalars(0xE7A1, len(perm))
    evals = h2.eval_polynomials(perm, np.arange(len(perm)), points)  # nothing pinned yet
    cols0 = h2.columns_pinned_info()
    h2.columns_pin(perm)
    h2.part_cosets_pin(perm, dom)
    assert h2.columns_pinned_info() == (cols0[0] + len(perm), cols0[1] + len(perm) * (32 << k))
    assert h2.part_cosets_pinned_info() == (len(perm), len(perm) * (32 << dom.extended_k))
    assert np.array_equal(h2.eval_polynomials(perm, np.arange(len(perm)), points), evals)
    assert np.array_equal(_run_parts(h2, case, c.vin), c.want)
    assert h2.evalh_parts_stats()[1] == len(perm) * P
    h2.columns_unpin(perm)
    assert h2.columns_pinned_info() == cols0 and h2.part_cosets_pinned_info()[0] == len(perm)
    assert np.array_equal(_run_parts(h2, case, c.vin), c.want)
    assert h2.evalh_parts_stats()[1] == len(perm) * P
    h2.columns_pin(perm)
    h2.part_cosets_unpin(perm)
    assert h2.part_cosets_pinned_info() == (0, 0) and h2.columns_pinned_info()[0] == cols0[0] + len(perm)
    assert np.array_equal(h2.eval_polynomials(perm, np.arange(len(perm)), points), evals)
    assert np.array_equal(_run_parts(h2, case, c.vin), c.want)
    assert h2.evalh_parts_stats()[1] == 0
    h2.columns_unpin(perm)


def test_pin_rejections_need_no_device(h2):
    L = h2.lib()
    dom = h2.EvaluationDomain.new(4, 4)
    a = np.zeros((16, 4), dtype=np.uint64)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u32 = ctypes.c_uint32
    tab = (ctypes.c_void_p * 2)(a.ctypes.data, None)
    w, g, gi = vp(dom.extended_omega), vp(dom.g_coset), vp(dom.g_coset_inv)
    assert L.h2hip_part_cosets_pin(tab, ctypes.c_size_t(2), u32(4), u32(6), w, g, gi) == 1  # a null polynomial
    assert L.h2hip_part_cosets_pin(None, ctypes.c_size_t(1), u32(4), u32(6), w, g, gi) == 1
    assert L.h2hip_part_cosets_pin(tab, ctypes.c_size_t(1), u32(7), u32(6), w, g, gi) == 1
    assert L.h2hip_part_cosets_pin(tab, ctypes.c_size_t(1), u32(27), u32(29), w, g, gi) == 1
    assert L.h2hip_part_cosets_pin(tab, ctypes.c_size_t(1), u32(4), u32(6), None, g, gi) == 1
    assert L.h2hip_part_cosets_pin_device(tab, ctypes.c_size_t(2), u32(4), u32(6), w, g, gi, None) == 1
    assert L.h2hip_part_cosets_pin(tab, ctypes.c_size_t(0), u32(4), u32(6), w, g, gi) == 0  # nothing to pin: no device is opened
    assert L.h2hip_part_cosets_unpin(None, ctypes.c_size_t(1)) == 1
    assert L.h2hip_debug_evalh_parts_stats(None) == 1
