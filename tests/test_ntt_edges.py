"""The scalar NTT (csrc/ntt.hip) on extreme and cancelling inputs, and the limb bounds of its tiles.

Every other NTT test feeds the kernels uniformly random scalars, which stay far inside the bounds the lazily reduced 9 x 29-bit arithmetic
of csrc/fieldu.h relies on, never cancel to an exact multiple of r in front of a closing reduction and never saturate a limb.  The named
inputs of ntt_edge_util.py do: const(r - 1) walks the all-plus path of every butterfly; const, nyquist, even_only and tone leave k r at
all outputs but one or two, which fu_canon_fast and fu_mul_canon must store as 0 and not as r; limbmax has every limb at 2^29 - 1.

Unmarked: the generators and closed forms themselves (against the oracle up to 2^10), the plans the GPU cases rely on, and
tests/cpp/test_ntt_bounds.cpp -- the tiles' schedules restated on the host under -DH2_FU_CHECK, every bound of the contract asserted.
GPU: every kernel family (one pass; strided + final; the two-pass ntt2_*), every entry point, both closing reductions, both twiddle
sources and the `quarter` branch, limb for limb against the oracle and, where one exists, against the closed form without it.  Every case
asserts the plan it takes.  No tolerance is involved anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ntt_edge_util as eu
from conftest import ROOT
from product_util import R_MOD
from test_ntt_plans import DEFAULT_BUDGET, NT, _plan, _restore_defaults

# (id, log_n, the plan, how it is forced, also with the inter-pass twiddles combined from the two-level table)
ONE_PASS = [("one-2^%d" % k, k, [k], "default", False) for k in (1, 2, 3, 4, 7, 8, 9, 10)]  # dft_lds alone: odd and even s, the lone last stage
MULTI = [
    ("strided-2^11", 11, [6, 5], "default", False),
    ("strided-2^13", 13, [7, 6], "default", True),
    ("strided-2^16", 16, [8, 8], "default", False),
    ("strided-2^17", 17, [6, 6, 5], "default", False),
    ("strided-smax9-2^18", 18, [9, 9], 9, True),      # two-pass plan off, tiles of 2^9 / 2^10 points on ntt_strided_kernel / ntt_final_kernel
    ("strided-smax10-2^19", 19, [10, 9], 10, False),
]
TWO_PASS = [
    ("two-forced-2^16", 16, [8, 8], "two", True),     # ntt2_* forced down: dft_col at s = 8, 9
    ("two-forced-2^17", 17, [9, 8], "two", False),
    ("two-2^19", 19, [10, 9], "default", False),
    ("two-2^20", 20, [10, 10], "default", False),
    ("two-2^21", 21, [11, 10], "default", False),
    ("two-2^22", 22, [11, 11], "default", False),
]
PLANS = ONE_PASS + MULTI + TWO_PASS
ENTRIES = ("ntt", "ifft", "c2e2", "c2e4", "c2e8", "e2c")  # c2eR: coeff_to_extended from 2^k / R coefficients
CASES = [pytest.param(p, e, id="%s-%s" % (p[0], e)) for p in PLANS for e in ENTRIES + (("host",) if p in ONE_PASS else ())
         if not (e.startswith("c2e") and p[1] < {"c2e2": 1, "c2e4": 2, "c2e8": 3}[e])]


def _specs(k):
    """every pattern and value while the oracle is instant, the core columns up to 2^20, four of them at 2^21 and 2^22"""
    return eu.full_specs(1 << k) if k <= 13 else eu.CORE_SPECS if k <= 20 else eu.BIG_SPECS


def _force(L, how):
    if how == "two":
        L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(16), ctypes.c_uint32(22))
    elif how != "default":
        L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(1), ctypes.c_uint32(0))  # off: or 2^19 takes ntt2_*, which reports the same radices
        L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(how))


# ------------------------------------------------------------------------------------------------- CPU: the inputs themselves
def test_values_and_generators_stay_below_r():
    assert [(eu.LIMBMAX >> (29 * i)) & 0x1FFFFFFF for i in range(8)] == [0x1FFFFFFF] * 8 and eu.LIMBMAX >> 232 == 0x30644D
    assert eu.LIMBMAX + (1 << 232) > R_MOD > eu.LIMBMAX  # the largest top limb that still fits
    assert eu.VALUES["r-ONE_E"] + eu.ONE_E == R_MOD and 2 * eu.VALUES["(r-1)/2"] + 1 == R_MOD
    assert not eu.below_r(eu.words([R_MOD, R_MOD + 1, (1 << 256) - 1])).any() and eu.below_r(eu.words([0, R_MOD - 1])).all()
    for k in (1, 2, 3, 6, 10):
        n, w = 1 << k, pow(5, (R_MOD - 1) >> k, R_MOD)
        for spec in eu.full_specs(n):
            a = eu.build(spec, n, w)
            assert a.shape == (n, 4) and a.dtype == np.uint64 and eu.below_r(a).all(), (k, spec)
    drawn = set(eu.ints(eu.extremes(1 << 10, 1)))
    assert drawn == set(eu.VALUES.values())
    s = eu.ints(eu.signs(1 << 10, R_MOD - 1, 7))
    assert set(s) == {1, R_MOD - 1} and 400 < s.count(1) < 624
    assert all(spec in eu.full_specs(1 << 14) for spec in eu.CORE_SPECS + eu.BIG_SPECS)


@pytest.mark.parametrize("k", range(1, 11))
def test_oracle_equals_every_closed_form(oracle, k):
    """the closed forms the GPU tests use without the oracle, against it: forward with omega, and the scaled inverse with omega_inv"""
    n = 1 << k
    d, _ = oracle.domain_new(2, k)
    for root, scale, run in (("omega", 1, lambda a: oracle.best_fft(a, d.fe("omega"), k, 2)),
                             ("omega_inv", eu.root_int(d.fe("ifft_divisor")), lambda a: oracle.ifft(a, d.fe("omega_inv"), k, d.fe("ifft_divisor"), 2))):
        w = eu.root_int(d.fe(root))
        assert pow(w, n, R_MOD) == 1 and pow(w, n // 2, R_MOD) == R_MOD - 1 and scale in (1, pow(n, -1, R_MOD))
        checked = 0
        for spec in eu.full_specs(n):
            want = eu.closed_form(spec, n, w, scale)
            if want is None:
                continue
            got = run(eu.case_input(spec, n, w))
            want = eu.dense(want, n) if isinstance(want, dict) else eu.words(want)
            assert np.array_equal(got, want), (root, spec)
            eu.check_result(got, spec, n, w, scale)
            checked += 1
        assert checked == len(eu.full_specs(n)) - 2 - len(eu.VALUES)  # all but extremes and signs


def test_tone_from_the_oracle_equals_the_integers(oracle):
    """beyond 2^12 points a tone is made by the oracle from a delta; the same words as the n integer products"""
    k = 13
    w = eu.root_int(oracle.domain_new(2, k)[0].fe("omega"))
    for c, t in ((eu.LIMBMAX, (1 << k) - 1), (eu.ONE_E, 1)):
        assert np.array_equal(eu.tone(1 << k, c, t, w, oracle), eu.words(eu.tone_ints(1 << k, c, t, w)))


def test_check_result_rejects_a_zero_stored_as_r():
    """what the GPU assertions exist for: r in place of 0 is caught by the canonical-word assertion and by the closed form"""
    n, w, spec = 8, pow(5, (R_MOD - 1) >> 3, R_MOD), ("const", "r-1", None)
    good = eu.dense(eu.closed_form(spec, n, w), n)
    eu.check_result(good, spec, n, w)
    bad = good.copy()
    bad[3] = eu.words([R_MOD])[0]
    with pytest.raises(AssertionError, match="not below r"):
        eu.check_result(bad, spec, n, w)
    bad[3] = eu.words([1])[0]
    with pytest.raises(AssertionError, match="cancel to 0"):
        eu.check_result(bad, spec, n, w)


def test_the_plans_the_gpu_cases_rely_on(h2):
    """No GPU needed: each case's plan under its settings, and the settings restored"""
    L = h2.lib()
    try:
        for _, k, radices, how, _ in PLANS:
            _restore_defaults(L)
            _force(L, how)
            assert _plan(h2, k) == radices, (k, how)
    finally:
        _restore_defaults(L)
    assert _plan(h2, 17, 3) == [6, 6, 5] and _plan(h2, 17, 4) == [9, 8] and _plan(h2, 19) == [10, 9]
    assert {p[2][0] for p in ONE_PASS} == {1, 2, 3, 4, 7, 8, 9, 10}
    assert {s for p in TWO_PASS for s in p[2]} == {8, 9, 10, 11}  # every tile size dft_col is used at


def test_ntt_tile_bounds_host(tmp_path):
    """tests/cpp/test_ntt_bounds.cpp: dft_lds (s = 1..10) and dft_col (s = 8..11, the quarter branch) restated on the host with every
    bound asserted -- |value| < 16 p at a store, fu_mul operand limbs < 2^30, loose limbs < 2^31 -- on the named inputs, coset-scaled
    ones and seeded extreme columns; prints the maxima DESIGN.md records"""
    src = os.path.join(ROOT, "tests", "cpp", "test_ntt_bounds.cpp")
    exe = str(tmp_path / "test_ntt_bounds")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DH2_FU_CHECK", "-Wno-unknown-pragmas", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ntt bounds ok" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if "max |value|/p" in ln]
    assert len(lines) == 2 * 10 + 3 * 4  # dft_lds s = 1..10 plain and coset-loaded; dft_col s = 8..11 plain, coset-loaded, quarter


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the shared inputs are read-only


@pytest.mark.gpu
@pytest.mark.parametrize("plan,entry", CASES)
def test_gpu_ntt_edges(h2, oracle, plan, entry):
    """one plan, one entry point, every named input of its size: bit-exact against the oracle, every word below r, and for ntt / ifft /
    host the closed form without the oracle.  ifft runs with the 1/n folded into the first pass's table (closing with fu_canon_fast)
    and multiplied in by the last pass (fu_mul_canon); c2e* pads from 2^k / R coefficients (R = 4 and 8: the `quarter` branch of dft_col
    on the two-pass plans) with r - 1 beyond them, which must not be read"""
    name, k, radices, how, both_sources = plan
    n = 1 << k
    L = h2.lib()
    h2.init()
    if entry.startswith("c2e"):
        ratio = int(entry[3:])
        d, _ = oracle.domain_new(ratio + 1, k - ratio.bit_length() + 1)
        assert d.extended_k == k and d.n * ratio == n
    elif entry == "e2c":
        d, _ = oracle.domain_new(3, k - 1)
        assert d.extended_k == k and d.n * d.quotient_poly_degree == n
    else:
        d, _ = oracle.domain_new(2, k)
    fe = {f: d.fe(f) for f in ("omega", "omega_inv", "ifft_divisor", "extended_omega", "extended_omega_inv", "extended_ifft_divisor",
                               "g_coset", "g_coset_inv")}
    root = {"ntt": "omega", "host": "omega", "ifft": "omega_inv", "e2c": "extended_omega_inv"}.get(entry, "extended_omega")
    w = eu.root_int(fe[root])
    scale = eu.root_int(fe["ifft_divisor"]) if entry == "ifft" else 1
    n_in = int(d.n) if entry.startswith("c2e") else n
    beyond = _dev(eu.const(n, R_MOD - 1)) if n_in < n else None

    def run(a):
        """the entry point's results on input a, one per variant that must give the same words"""
        if entry == "host":
            b = a.copy()
            h2.best_fft(b, fe["omega"], k)
            return [b]
        if entry == "ntt":
            t = _dev(a)
            h2.ntt_device(t, fe["omega"], k)
            return [h2.to_numpy_u64(t)]
        if entry == "ifft":
            out = []
            for fold in (1, 0):
                L.h2hip_debug_set_ntt_fold_tables(ctypes.c_int(fold))
                t = _dev(a)
                h2.ifft_device(t, fe["omega_inv"], k, fe["ifft_divisor"])
                out.append(h2.to_numpy_u64(t))
            L.h2hip_debug_set_ntt_fold_tables(ctypes.c_int(1))
            return out
        if entry == "e2c":
            t = _dev(a)
            h2.extended_to_coeff_device(t, k, fe["extended_omega_inv"], fe["extended_ifft_divisor"], fe["g_coset"], fe["g_coset_inv"])
            return [h2.to_numpy_u64(t)]
        t = beyond.clone()
        t[:n_in] = _dev(a)
        h2.coeff_to_extended_device(t, int(d.k), k, fe["extended_omega"], fe["g_coset"], fe["g_coset_inv"])
        return [h2.to_numpy_u64(t)]

    def expect(a):
        if entry in ("ntt", "host"):
            return oracle.best_fft(a, fe["omega"], k, NT)
        if entry == "ifft":
            return oracle.ifft(a, fe["omega_inv"], k, fe["ifft_divisor"], NT)
        if entry == "e2c":
            return oracle.extended_to_coeff(d, a, NT)
        return oracle.coeff_to_extended(d, a, NT)

    try:
        _force(L, how)
        assert _plan(h2, k) == radices
        inputs = [(spec, eu.case_input(spec, n_in, w, oracle)) for spec in _specs(k)]
        wants = [expect(a) for _, a in inputs]
        for budget in (DEFAULT_BUDGET, 0) if both_sources else (DEFAULT_BUDGET,):
            L.h2hip_debug_set_ntt_twiddle_budget(ctypes.c_uint64(budget))
            for (spec, a), want in zip(inputs, wants):
                for v, got in enumerate(run(a)):
                    tag = (name, entry, budget, v)
                    assert got.shape == want.shape == (n, 4)
                    eu.assert_below_r(got, (tag, spec))
                    if entry in ("ntt", "host", "ifft"):
                        eu.check_result(got, spec, n, w, scale, tag)
                    assert np.array_equal(got, want), (tag, spec, np.flatnonzero((got != want).any(axis=1))[:8])
    finally:
        _restore_defaults(L)


# (id, log_n, columns, the plan the batch takes, how it is forced)
BATCHES = [
    ("one-2^8", 8, 3, [8], "default"),
    ("strided-2^13", 13, 3, [7, 6], "default"),
    ("two-forced-2^16", 16, 3, [8, 8], "two"),
    ("two-2^19", 19, 3, [10, 9], "default"),
    ("batch-rule-4x2^17", 17, 4, [9, 8], "default"),  # four columns bring the 512 workgroup pairs at which 2^17 takes the two-pass plan
]
BATCH_SPECS = [("zero", None, None), ("const", "r-1", None), ("extremes", None, 1), ("nyquist", "limbmax", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,count,radices,how", BATCHES, ids=[b[0] for b in BATCHES])
def test_gpu_ntt_edges_batched(h2, oracle, name, k, count, radices, how):
    """ntt_batch_device and ifft_batch_device on [zero, const(r - 1), extremes(, nyquist(limbmax))], each column against its own
    expectation: a batch that mixes its columns cannot pass"""
    n = 1 << k
    L = h2.lib()
    h2.init()
    d, _ = oracle.domain_new(2, k)
    specs = BATCH_SPECS[:count]
    try:
        _force(L, how)
        assert _plan(h2, k, count) == radices
        for root, scale in (("omega", 1), ("omega_inv", eu.root_int(d.fe("ifft_divisor")))):
            w = eu.root_int(d.fe(root))
            ins = [eu.case_input(spec, n, w, oracle) for spec in specs]
            cols = [_dev(a) for a in ins]
            if root == "omega":
                h2.ntt_batch_device(cols, d.fe("omega"), k)
                wants = [oracle.best_fft(a, d.fe("omega"), k, NT) for a in ins]
            else:
                h2.ifft_batch_device(cols, d.fe("omega_inv"), k, d.fe("ifft_divisor"))
                wants = [oracle.ifft(a, d.fe("omega_inv"), k, d.fe("ifft_divisor"), NT) for a in ins]
            for i, (spec, t, want) in enumerate(zip(specs, cols, wants)):
                got = h2.to_numpy_u64(t)
                eu.check_result(got, spec, n, w, scale, (name, root, i))
                assert np.array_equal(got, want), (name, root, i, spec)
    finally:
        _restore_defaults(L)


@pytest.mark.gpu
@pytest.mark.parametrize("j,k", [(3, 5), (5, 8), (9, 10), (9, 15)], ids=["2^6", "2^10", "2^13", "2^18"])
def test_gpu_divide_by_vanishing_poly_edges(h2, oracle, j, k):
    """scale_periodic_kernel (fu_mul_canon by t_evaluations[i % t_len]) on zero, every const and extreme columns"""
    h2.init()
    d, t_eval = oracle.domain_new(j, k)
    dom = h2.EvaluationDomain.new(j, k)
    n = 1 << d.extended_k
    assert dom.extended_k == d.extended_k and np.array_equal(dom.t_evaluations, t_eval) and t_eval.shape[0] == n >> k
    specs = [("zero", None, None)] + [("const", v, None) for v in eu.VALUES] + [("extremes", None, 1), ("extremes", None, 2)]
    for spec in specs:
        a = eu.case_input(spec, n, 1)
        got = dom.divide_by_vanishing_poly(a, t_eval)
        eu.assert_below_r(got, spec)
        assert np.array_equal(got, oracle.divide_by_vanishing_poly(d, t_eval, a)), spec
        if spec[0] == "zero" or spec[1] == "0":
            assert not got.any()
