"""The NTT's pass plans against the oracle, limb for limb.

ntt.hip picks a plan per call: one pass up to 2^10 points, the two-pass ntt2_* plan at 2^19..2^22, otherwise up to four passes of
near-equal tiles of at most 2^smax points (smax 8, or 9 above 2^24).  h2hip_debug_ntt_plan reports the plan a call takes, and every
case here asserts the one it hits, so a change to plan_passes cannot quietly move coverage away.

Small sizes force every plan shape through the tuning hooks: two, three and four passes, one tile radix or two, tiles of 2^3 to 2^10
points, inter-pass twiddles from a table or combined from the two-level one.  The default plans of 2^25 to 2^28 (2^9-point tiles,
and four passes at 2^28) run at full size: forward, scaled inverse, the coset conversions and batches.  A round trip is no
evidence there: a transform that is wrong in a way its inverse undoes passes one.
"""
import ctypes
import gc
import os

import numpy as np
import pytest

NT = min(16, os.cpu_count() or 1)
DEFAULT_BUDGET = 4 << 30  # the inter-pass twiddle tables' default HBM budget (ntt.hip g_ntt_full_budget)


def _plan(h2, log_n, count=1):
    """the log2 tile of each pass the engine takes for `count` columns of 2^log_n points (h2hip_debug_ntt_plan), or its error code"""
    r = (ctypes.c_uint32 * 4)()
    p = h2.lib().h2hip_debug_ntt_plan(ctypes.c_uint32(log_n), ctypes.c_size_t(count), r)
    return list(r[:p]) if p > 0 else p


def _restore_defaults(L):
    L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(8))  # no reset sentinel: 8 is the default
    L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(0), ctypes.c_uint32(0))
    L.h2hip_debug_set_ntt_twiddle_budget(ctypes.c_uint64(DEFAULT_BUDGET))
    L.h2hip_debug_set_ntt_full_max_log_m(ctypes.c_uint32(0))
    L.h2hip_debug_set_ntt_fold_tables(ctypes.c_int(1))
    L.h2hip_debug_set_ntt_batch_bytes(ctypes.c_uint64(0))


DEFAULT_PLANS = {k: [k] for k in range(11)}
DEFAULT_PLANS.update({11: [6, 5], 12: [6, 6], 13: [7, 6], 14: [7, 7], 15: [8, 7], 16: [8, 8], 17: [6, 6, 5], 18: [6, 6, 6],
                      19: [10, 9], 20: [10, 10], 21: [11, 10], 22: [11, 11], 23: [8, 8, 7], 24: [8, 8, 8],
                      25: [9, 8, 8], 26: [9, 9, 8], 27: [9, 9, 9], 28: [7, 7, 7, 7]})

# (smax, log_n, the plan with the two-pass plan switched off): two, three and four passes, one radix and two, tiles of 2^3..2^10
FORCED = [
    (4, 12, [4, 4, 4]),
    (4, 13, [4, 3, 3, 3]),
    (4, 16, [4, 4, 4, 4]),
    (5, 11, [4, 4, 3]),
    (5, 18, [5, 5, 4, 4]),
    (5, 20, [5, 5, 5, 5]),
    (6, 19, [5, 5, 5, 4]),
    (6, 22, [6, 6, 5, 5]),
    (7, 13, [7, 6]),
    (7, 14, [7, 7]),
    (8, 17, [6, 6, 5]),
    (8, 20, [7, 7, 6]),
    (9, 17, [9, 8]),
    (9, 18, [9, 9]),
    (10, 19, [10, 9]),   # two columns of 2^10 points: 72 KB of dynamic LDS, above the 64 KB default (ntt_run raises the limit)
    (10, 20, [10, 10]),
]


def test_plan_hook_reports_the_plans(h2):
    """No GPU needed: the default plan of every size, the batch sizes at which 2^17 / 2^18 columns switch to the two-pass plan, and
    the forced plans the GPU cases below rely on"""
    L = h2.lib()
    for k, s in DEFAULT_PLANS.items():
        assert _plan(h2, k) == s, k
    assert _plan(h2, 17, 3) == [6, 6, 5] and _plan(h2, 17, 4) == [9, 8]  # 512 workgroup pairs per pass
    assert _plan(h2, 18, 1) == [6, 6, 6] and _plan(h2, 18, 2) == [9, 9]
    assert _plan(h2, 16, 1 << 12) == [8, 8] and _plan(h2, 25, 2) == [9, 8, 8]
    assert _plan(h2, 29) == -1
    assert h2.lib().h2hip_debug_ntt_plan(ctypes.c_uint32(12), ctypes.c_size_t(1), None) == -1
    shapes = set()
    try:
        L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(1), ctypes.c_uint32(0))  # hi < lo: off, for batches too
        assert _plan(h2, 20) == [7, 7, 6] and _plan(h2, 18, 64) == [6, 6, 6]
        for smax, k, s in FORCED:
            L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(smax))
            assert _plan(h2, k) == s and _plan(h2, k, 3) == s, (smax, k)
            shapes.add((len(s), len(set(s))))
        L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(11))  # clamped to 10
        assert _plan(h2, 20) == [10, 10]
        L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(9))  # 9 explicitly: the same plans as the default above 2^24
        assert _plan(h2, 28) == [7, 7, 7, 7] and _plan(h2, 24) == [8, 8, 8]
    finally:
        _restore_defaults(L)
    assert shapes == {(p, r) for p in (2, 3, 4) for r in (1, 2)}
    assert {r for _, _, s in FORCED for r in s} == set(range(3, 11))
    for k, s in DEFAULT_PLANS.items():  # and the restored settings are the defaults
        assert _plan(h2, k) == s, k


def _eq(h2, t, want):
    return np.array_equal(h2.to_numpy_u64(t), want)


@pytest.mark.gpu
@pytest.mark.parametrize("smax,k,radices", FORCED, ids=[f"smax{s}-2^{k}" for s, k, _ in FORCED])
def test_forced_plan_vs_oracle(h2, oracle, smax, k, radices):
    """One forced plan at 2^k: forward; scaled inverse with the 1/n folded into the first pass's twiddles and multiplied in by the
    last pass; coeff_to_extended from 2^(k-1) and 2^(k-3) coefficients (beyond them the buffer holds values that must not be read);
    extended_to_coeff; three columns through the *_batch_device entry points -- each with the inter-pass twiddles from their tables
    and from the two-level table"""
    import torch
    L = h2.lib()
    d2, _ = oracle.domain_new(3, k - 1)  # extended_k = k, padding ratio 2
    d8, _ = oracle.domain_new(9, k - 3)  # ratio 8
    assert d2.extended_k == k and d8.extended_k == k
    a = h2.gen_scalars_device(0x9A00 + k, 1 << k)
    others = [h2.gen_scalars_device(0x9B00 + 16 * k + i, 1 << k) for i in range(2)]
    an = h2.to_numpy_u64(a)
    fe2 = {n: d2.fe(n) for n in ("extended_omega", "extended_omega_inv", "extended_ifft_divisor", "g_coset", "g_coset_inv")}
    fwd = oracle.best_fft(an, fe2["extended_omega"], k, NT)
    inv = oracle.ifft(an, fe2["extended_omega_inv"], k, fe2["extended_ifft_divisor"], NT)
    ext = {d.k: (d, oracle.coeff_to_extended(d, an[:1 << d.k], NT)) for d in (d2, d8)}
    e2c = oracle.extended_to_coeff(d2, an, NT)
    assert e2c.shape == an.shape
    try:
        L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(1), ctypes.c_uint32(0))
        L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(smax))
        assert _plan(h2, k) == radices and _plan(h2, k, 3) == radices
        for budget in (DEFAULT_BUDGET, 0):
            L.h2hip_debug_set_ntt_twiddle_budget(ctypes.c_uint64(budget))
            tag = (smax, k, budget)
            f = a.clone()
            h2.ntt_device(f, fe2["extended_omega"], k)
            assert _eq(h2, f, fwd), tag
            for fold in (1, 0):
                L.h2hip_debug_set_ntt_fold_tables(ctypes.c_int(fold))
                i = a.clone()
                h2.ifft_device(i, fe2["extended_omega_inv"], k, fe2["extended_ifft_divisor"])
                assert _eq(h2, i, inv), tag + (fold,)
            L.h2hip_debug_set_ntt_fold_tables(ctypes.c_int(1))
            for ck, (d, want) in ext.items():
                e = a.clone()
                h2.coeff_to_extended_device(e, ck, k, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
                assert _eq(h2, e, want), tag + (ck,)
            b = a.clone()
            h2.extended_to_coeff_device(b, k, fe2["extended_omega_inv"], fe2["extended_ifft_divisor"], fe2["g_coset"], fe2["g_coset_inv"])
            assert _eq(h2, b, e2c), tag
            # three different columns in one launch per pass: the first against the oracle, the others against their lone transforms
            lone = [o.clone() for o in others]
            for t in lone:
                h2.ntt_device(t, fe2["extended_omega"], k)
            cols = [a.clone()] + [o.clone() for o in others]
            h2.ntt_batch_device(cols, fe2["extended_omega"], k)
            assert _eq(h2, cols[0], fwd) and all(torch.equal(c, t) for c, t in zip(cols[1:], lone)), tag
            for t in lone:
                h2.ifft_device(t, fe2["extended_omega_inv"], k, fe2["extended_ifft_divisor"])
            h2.ifft_batch_device(cols, fe2["extended_omega_inv"], k, fe2["extended_ifft_divisor"])
            assert _eq(h2, cols[0], an) and all(torch.equal(c, t) for c, t in zip(cols[1:], lone)), tag
            d, want = ext[k - 3]
            lone = [o.clone() for o in others]
            for t in lone:
                h2.coeff_to_extended_device(t, k - 3, k, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
            cols = [a.clone()] + [o.clone() for o in others]
            h2.coeff_to_extended_batch_device(cols, k - 3, k, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
            assert _eq(h2, cols[0], want) and all(torch.equal(c, t) for c, t in zip(cols[1:], lone)), tag
    finally:
        _restore_defaults(L)


# ---------------------------------------------------------------------------- 2^25 .. 2^28, default plans
# Inputs are generated on the device.  Oracle results shared by several tests of one size are kept here and dropped when a test of
# another size starts: at 2^28 one column is 8 GB.
_cache = {}


def _cached(log_n, name, make):
    for key in [key for key in _cache if key[0] != log_n]:
        del _cache[key]
    gc.collect()
    if (log_n, name) not in _cache:
        _cache[(log_n, name)] = make()
    return _cache[(log_n, name)]


def _input(h2, seed, log_n):
    return h2.to_numpy_u64(h2.gen_scalars_device(seed, 1 << log_n))


SEED = {25: 0x25A, 26: 0x26A, 27: 0x27A, 28: 0x28A}


def _forward_and_inverse(h2, oracle, k, inverse=True):
    """the input of 2^k points (from its seed), its oracle forward transform and, if asked, its oracle scaled inverse"""
    def make():
        d, _ = oracle.domain_new(2, k)
        a = _input(h2, SEED[k], k)
        fwd = oracle.best_fft(a, d.fe("omega"), k, NT)
        return d, a, fwd, (oracle.ifft(a, d.fe("omega_inv"), k, d.fe("ifft_divisor"), NT) if inverse else None)
    return _cached(k, "fwd_inv" if inverse else "fwd", make)


def _check_device(h2, d, k, fwd, inv):
    x = h2.gen_scalars_device(SEED[k], 1 << k)
    h2.ntt_device(x, d.fe("omega"), k)
    assert _eq(h2, x, fwd), "forward"
    if inv is not None:
        x = h2.gen_scalars_device(SEED[k], 1 << k)
        h2.ifft_device(x, d.fe("omega_inv"), k, d.fe("ifft_divisor"))
        assert _eq(h2, x, inv), "scaled inverse"
    del x
    gc.collect()


@pytest.mark.gpu
@pytest.mark.parametrize("twiddles", ["default", "first_pass_table", "two_level"])
def test_ntt_2p25_vs_oracle(h2, oracle, twiddles):
    """2^25, tiles 2^9, 2^8, 2^8.  default: the first pass (M = 2^25) combines its inter-pass twiddles from the two-level table and the
    inverse's 1/n rides in the scaled copy of `lo`, table-fed passes behind it; first_pass_table: the first pass reads a 2^25-entry
    table, the inverse its scaled copy; two_level: no tables at all"""
    L = h2.lib()
    assert _plan(h2, 25) == [9, 8, 8]
    d, _, fwd, inv = _forward_and_inverse(h2, oracle, 25)
    try:
        if twiddles == "first_pass_table":
            L.h2hip_debug_set_ntt_full_max_log_m(ctypes.c_uint32(25))
            L.h2hip_debug_set_ntt_twiddle_budget(ctypes.c_uint64(1 << 40))  # room for the 1.2 GB table and its scaled copy whatever ran before
        elif twiddles == "two_level":
            L.h2hip_debug_set_ntt_twiddle_budget(ctypes.c_uint64(0))
        _check_device(h2, d, 25, fwd, inv)
    finally:
        _restore_defaults(L)


@pytest.mark.gpu
def test_coeff_to_extended_2p22_to_2p25_vs_oracle(h2, oracle):
    """a quotient of degree 8 at k = 22 (extended_k 25): the zero-padded first load with the % 3 coset scale on a 2^9-tile plan"""
    import torch
    d, _ = oracle.domain_new(9, 22)
    assert d.extended_k == 25 and _plan(h2, 25) == [9, 8, 8]
    c, want = _coset_2p25(h2, oracle, d)
    buf = torch.full((1 << 25, 4), 0x5A5A, dtype=torch.int64, device="cuda")  # beyond the coefficients: not read
    buf[:1 << 22] = torch.from_numpy(c.view(np.int64)).cuda()
    h2.coeff_to_extended_device(buf, 22, 25, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
    assert _eq(h2, buf, want)


def _coset_2p25(h2, oracle, d):
    def make():
        c = _input(h2, 0x2522, 22)
        return c, oracle.coeff_to_extended(d, c, NT)
    return _cached(25, "coset", make)


@pytest.mark.gpu
def test_extended_to_coeff_2p25_vs_oracle(h2, oracle):
    d, _ = oracle.domain_new(9, 22)
    assert d.extended_k == 25 and d.n * d.quotient_poly_degree == 1 << 25
    x = h2.gen_scalars_device(0x25E2C, 1 << 25)
    want = oracle.extended_to_coeff(d, h2.to_numpy_u64(x), NT)
    h2.extended_to_coeff_device(x, 25, d.fe("extended_omega_inv"), d.fe("extended_ifft_divisor"), d.fe("g_coset"), d.fe("g_coset_inv"))
    assert _eq(h2, x, want)


@pytest.mark.gpu
def test_divide_by_vanishing_poly_2p25_vs_oracle(h2, oracle):
    d, t_eval = oracle.domain_new(9, 22)
    assert d.extended_k == 25 and t_eval.shape[0] == 8
    dom = h2.EvaluationDomain.new(9, 22)
    assert np.array_equal(dom.t_evaluations, t_eval)
    h = _input(h2, 0x25D1, 25)
    assert np.array_equal(dom.divide_by_vanishing_poly(h, t_eval), oracle.divide_by_vanishing_poly(d, t_eval, h))


@pytest.mark.gpu
def test_batches_2p25_one_column_per_launch_and_both_in_one(h2, oracle):
    """2 columns of 2^25 points through ntt_batch_device and coeff_to_extended_batch_device: by default one column per launch (2 GB of
    columns + workspace), then with the launch bytes raised both in one launch per pass.  The first column equals the oracle, the
    second its lone transform."""
    import torch
    L = h2.lib()
    assert _plan(h2, 25, 2) == [9, 8, 8]
    d, _, fwd, _ = _forward_and_inverse(h2, oracle, 25)
    dc, _ = oracle.domain_new(9, 22)
    c, want = _coset_2p25(h2, oracle, dc)
    other = h2.gen_scalars_device(0x25B, 1 << 25)
    lone_f = other.clone()
    h2.ntt_device(lone_f, d.fe("omega"), 25)
    lone_c = other.clone()
    h2.coeff_to_extended_device(lone_c, 22, 25, dc.fe("extended_omega"), dc.fe("g_coset"), dc.fe("g_coset_inv"))
    try:
        for launch_bytes in (0, 2 * 2 * (32 << 25)):
            L.h2hip_debug_set_ntt_batch_bytes(ctypes.c_uint64(launch_bytes))
            cols = [h2.gen_scalars_device(SEED[25], 1 << 25), other.clone()]
            h2.ntt_batch_device(cols, d.fe("omega"), 25)
            assert _eq(h2, cols[0], fwd) and torch.equal(cols[1], lone_f), launch_bytes
            cols = [torch.empty_like(other), other.clone()]
            cols[0][:1 << 22] = torch.from_numpy(c.view(np.int64)).cuda()
            h2.coeff_to_extended_batch_device(cols, 22, 25, dc.fe("extended_omega"), dc.fe("g_coset"), dc.fe("g_coset_inv"))
            assert _eq(h2, cols[0], want) and torch.equal(cols[1], lone_c), launch_bytes
            del cols
    finally:
        _restore_defaults(L)


@pytest.mark.gpu
def test_ntt_2p26_vs_oracle(h2, oracle):
    """2^26, tiles 2^9, 2^9, 2^8: forward and scaled inverse"""
    assert _plan(h2, 26) == [9, 9, 8]
    d, _, fwd, inv = _forward_and_inverse(h2, oracle, 26)
    _check_device(h2, d, 26, fwd, inv)


@pytest.mark.gpu
def test_host_batch_2p26_vs_oracle(h2, oracle):
    """best_fft_batch of 2 host columns of 2^26 points: a pipelined run holds two columns from 2^26 on"""
    d, a, fwd, _ = _forward_and_inverse(h2, oracle, 26)
    cols = [a.copy(), _input(h2, 0x26B, 26)]
    want1 = oracle.best_fft(cols[1], d.fe("omega"), 26, NT)
    h2.best_fft_batch(cols, d.fe("omega"), 26)
    assert np.array_equal(cols[0], fwd)
    assert np.array_equal(cols[1], want1)


@pytest.mark.gpu
def test_ntt_2p27_vs_oracle(h2, oracle):
    """2^27, tiles 2^9 x 3: forward on the device, then the host-pointer best_fft (4 GB pageable upload and download)"""
    assert _plan(h2, 27) == [9, 9, 9]
    d, a, fwd, _ = _forward_and_inverse(h2, oracle, 27, inverse=False)
    _check_device(h2, d, 27, fwd, None)
    h = a.copy()
    h2.best_fft(h, d.fe("omega"), 27)
    assert np.array_equal(h, fwd)


@pytest.mark.gpu
def test_ntt_2p28_four_passes_vs_oracle(h2, oracle):
    """2^28, the 2-adicity of Fr: the default plan's only four-pass size (tiles 2^7 x 4: the last pass undoes three digit orders)"""
    assert _plan(h2, 28) == [7, 7, 7, 7]
    d, _ = oracle.domain_new(2, 28)
    _cached(28, None, lambda: None)  # drop what the smaller sizes kept
    a = _input(h2, SEED[28], 28)
    want = oracle.best_fft(a, d.fe("omega"), 28, NT)
    _check_device(h2, d, 28, want, None)
    del want
    gc.collect()
    want = oracle.ifft(a, d.fe("omega_inv"), 28, d.fe("ifft_divisor"), NT)
    del a
    gc.collect()
    x = h2.gen_scalars_device(SEED[28], 1 << 28)
    h2.ifft_device(x, d.fe("omega_inv"), 28, d.fe("ifft_divisor"))
    assert _eq(h2, x, want), "scaled inverse"


@pytest.mark.gpu
def test_coeff_to_extended_2p25_to_2p28_vs_oracle(h2, oracle):
    """a quotient of degree 8 at k = 25 (extended_k 28): the zero-padded, coset-scaled first load on the four-pass plan"""
    import torch
    d, _ = oracle.domain_new(9, 25)
    assert d.extended_k == 28 and _plan(h2, 28) == [7, 7, 7, 7]
    _cached(28, None, lambda: None)
    x = h2.gen_scalars_device(0x2825, 1 << 28)
    x[1 << 25:] = 0x5A5A  # not read
    want = oracle.coeff_to_extended(d, h2.to_numpy_u64(x[:1 << 25]), NT)
    h2.coeff_to_extended_device(x, 25, 28, d.fe("extended_omega"), d.fe("g_coset"), d.fe("g_coset_inv"))
    assert _eq(h2, x, want)
    del x
    torch.cuda.empty_cache()
