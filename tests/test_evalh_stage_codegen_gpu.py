"""The kernels evaluate_h generates for the shuffle and mv-lookup stages, on the GPU: every result equals the big-integer models of
tests/shuffle_util.py and tests/mvlookup_util.py limb for limb, through the interpreter (codegen mode 0) and through the generated kernels
(mode 2 + 64: compiled inline, both stages' kernels wanted), and the stage counters (h2hip_debug_evalh_codegen_stage_stats) show which
of the two ran.  Systems, entry points and models are the existing stage tests'."""
import contextlib
import ctypes
import time
import types

import numpy as np
import pytest

import test_mvlookup_evalh as TM
import test_shuffle_evalh as TS
from evalh_util import Evaluator, flatten_graph, mvlookup_graphs, shuffle_graphs
from shuffle_util import R_MOD, to_mont

A, F, I = TS.A, TS.F, TS.I
ENTRIES = TS.ENTRIES
GATES, LOOKUPS, SHUFFLES, MVLOOKUPS = 0, 1, 2, 3
BOTH, NONE, NO_FUSION = 64, 32, 16
MV_DOMAINS = TM.DOMAINS + [(3, 9)]  # ... and one with 512 rows a part: a second workgroup, rotations wrapping across it
PENDING_BOUND = 8  # EVALH_RTC_MAX_PENDING


def _stats(L):
    a, b = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 9)()
    assert L.h2hip_debug_evalh_codegen_stats(a) == 0 and L.h2hip_debug_evalh_codegen_stage_stats(b) == 0
    return types.SimpleNamespace(compiled=a[0], failed=a[1], gen=[b[0], b[2], b[4], b[6]], interp=[b[1], b[3], b[5], b[7]], pending=b[8])


@contextlib.contextmanager
def _codegen(L, mode):
    assert L.h2hip_debug_set_evalh_codegen(ctypes.c_int(mode), ctypes.c_uint32(0)) == 0
    try:
        yield
    finally:
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))


def _quiesce(L):
    """wait out the background compilations earlier tests queued (as a rule none): they would move `compiled` under a test that counts"""
    deadline = time.time() + 120
    while _stats(L).pending and time.time() < deadline:
        pass
    assert _stats(L).pending == 0


def _both_ways(h2, run, stage, want):
    """run() through the interpreter and through the generated kernels: both the model's values, the stage's generated launches rising
    only in the second, no compilation failed"""
    L = h2.lib()
    s0 = _stats(L)
    with _codegen(L, 0):
        got_i = run()
    s1 = _stats(L)
    with _codegen(L, 2 + BOTH):
        got_g = run()
    s2 = _stats(L)
    assert s1.gen == s0.gen and s1.interp[stage] > s0.interp[stage]
    assert s2.gen[stage] > s1.gen[stage] and s2.interp[stage] == s1.interp[stage]
    assert s2.failed == s0.failed, L.h2hip_last_error()
    assert np.array_equal(got_i, want)
    assert np.array_equal(got_g, want)
    assert got_i.tobytes() == got_g.tobytes()


# ------------------------------------------------------------------------------------------------ case 1: the four entry forms
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rich", [False, True], ids=["alone", "after_lookup_and_permutation"])
@pytest.mark.parametrize("j,k", TS.DOMAINS)
def test_gpu_shuffle_kernels_vs_model(h2, oracle, j, k, rich, entry):
    """k = 4 (a part of 16 rows: one partly filled workgroup behind the row guard), k = 7 and k = 9 (512 rows a part)"""
    h2.init()
    sy = TS._system(oracle, j, k, 100 * j + k, rich)
    _both_ways(h2, lambda: TS._run(h2, sy, entry, sy.vin), SHUFFLES, TS._want(h2, oracle, sy))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("variant", ["alone", "with_all"])
@pytest.mark.parametrize("j,k", MV_DOMAINS)
def test_gpu_mvlookup_kernels_vs_model(h2, oracle, j, k, variant, entry):
    """K = 1 and K = 5 arguments, alone and between a halo2 lookup and two shuffles (which then run generated too)"""
    h2.init()
    sy = TM._system(oracle, j, k, 100 * j + k, variant)
    _both_ways(h2, lambda: TM._run(h2, sy, entry, sy.vin), MVLOOKUPS, TM._want(h2, oracle, sy))


# ------------------------------------------------------------------------------------------------ case 2: mode 2 + 32
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["full_device", "parts_host"])
def test_gpu_stage_kernels_off_leaves_gates_and_lookups_generated(h2, oracle, entry):
    h2.init()
    L = h2.lib()
    sy = TM._system(oracle, 4, 5, 405, "with_all")
    s0 = _stats(L)
    with _codegen(L, 2 + NONE):
        got = TM._run(h2, sy, entry, sy.vin)
    s1 = _stats(L)
    assert s1.gen[GATES] > s0.gen[GATES] and s1.gen[LOOKUPS] > s0.gen[LOOKUPS]
    assert s1.interp[GATES] == s0.interp[GATES] and s1.interp[LOOKUPS] == s0.interp[LOOKUPS]
    assert s1.gen[SHUFFLES] == s0.gen[SHUFFLES] and s1.gen[MVLOOKUPS] == s0.gen[MVLOOKUPS]
    assert s1.interp[SHUFFLES] > s0.interp[SHUFFLES] and s1.interp[MVLOOKUPS] > s0.interp[MVLOOKUPS]
    assert s1.failed == s0.failed
    assert np.array_equal(got, TM._want(h2, oracle, sy))


# ------------------------------------------------------------------------------------------------ systems of this file's own
def _shuffle_system(oracle, base, shuffles, seed):
    """`base` (a system of test_shuffle_evalh) with other shuffles: their graphs and one product polynomial each"""
    n = 1 << base.k
    z = [TS._ro(oracle.gen_scalars(seed * 1000 + 60 + i, n)) for i in range(len(shuffles))]
    ev = types.SimpleNamespace(shuffles=[shuffle_graphs(i, s) for i, s in shuffles])
    return types.SimpleNamespace(**{**vars(base), "shuffles": shuffles, "z": z, "ev": ev})


def _salt():
    """a constant no earlier test (of this process or another) has put into a program"""
    return 1_000_003 + int(time.time() * 1000) % 1_000_000_007


# ------------------------------------------------------------------------------------------------ case 3: identical arguments
@pytest.mark.gpu
def test_gpu_identical_shuffles_share_one_code_object(h2, oracle):
    h2.init()
    L = h2.lib()
    c = _salt()
    same = ([A(1, 1), ('prod', A(2), F(1))], [A(3), ('scaled', A(4, -1), c)])
    sy = _shuffle_system(oracle, TS._system(oracle, 4, 7, 407, False), [same, same], 431)
    want = TS._model(h2, oracle, sy, sy.vin)
    with _codegen(L, 2 + NONE):  # whatever the gates need is compiled here
        assert np.array_equal(TS._run(h2, sy, "full_host", sy.vin), want)
    _quiesce(L)
    s0 = _stats(L)
    with _codegen(L, 2 + BOTH):
        got = TS._run(h2, sy, "full_host", sy.vin)
        s1 = _stats(L)
        again = TS._run(h2, sy, "full_device", sy.vin)
        s2 = _stats(L)
    assert s1.compiled == s0.compiled + 1 and s2.compiled == s1.compiled and s2.failed == s0.failed
    assert s1.gen[SHUFFLES] == s0.gen[SHUFFLES] + 2 and s2.gen[SHUFFLES] == s1.gen[SHUFFLES] + 2
    assert s2.interp[SHUFFLES] == s0.interp[SHUFFLES]
    assert np.array_equal(got, want) and np.array_equal(again, want)
    one = _shuffle_system(oracle, sy, [same], 431)  # the second shuffle's product column matters: the launch argument carries it
    assert not np.array_equal(TS._model(h2, oracle, one, sy.vin), want)


@pytest.mark.gpu
def test_gpu_identical_mvlookups_share_one_code_object(h2, oracle):
    h2.init()
    L = h2.lib()
    c = _salt()
    same = (((A(1, 1), ('prod', A(2), F(1))), (A(3), ('scaled', A(4, -1), c))), (F(2), F(0, 1)))
    sy = TM._system(oracle, 4, 5, 432, "alone", mv_override=(same, same))
    want = TM._want(h2, oracle, sy)
    with _codegen(L, 2 + NONE):
        assert np.array_equal(TM._run(h2, sy, "full_host", sy.vin), want)
    _quiesce(L)
    s0 = _stats(L)
    with _codegen(L, 2 + BOTH):
        got = TM._run(h2, sy, "full_host", sy.vin)
        s1 = _stats(L)
        again = TM._run(h2, sy, "full_device", sy.vin)
        s2 = _stats(L)
    assert s1.compiled == s0.compiled + 1 and s2.compiled == s1.compiled and s2.failed == s0.failed
    assert s1.gen[MVLOOKUPS] == s0.gen[MVLOOKUPS] + 2 and s2.gen[MVLOOKUPS] == s1.gen[MVLOOKUPS] + 2
    assert np.array_equal(got, want) and np.array_equal(again, want)
    assert not np.array_equal(sy.phi[0], sy.phi[1]) and not np.array_equal(sy.m[0], sy.m[1])


# ------------------------------------------------------------------------------------------------ case 4: fallback
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["full_host", "parts_device"])
def test_gpu_an_argument_beyond_the_limits_keeps_the_interpreter(h2, oracle, entry):
    """60 products alive at once in the first argument's second tuple: that argument is interpreted, the one beside it generated, in one call"""
    h2.init()
    L = h2.lib()
    mv = ((((A(0),), TM._many_live_tuple(60)), (F(0),)), (((A(1), A(2, 1)),), (F(1), F(2))))
    sy = TM._system(oracle, 4, 5, 433, "alone", mv_override=mv)
    assert max(TM._compile_stats(h2, flatten_graph(g))[1] for g in sy.ev.mv_lookups[0]) > 48
    want = TM._want(h2, oracle, sy)
    calls = 4 if entry.startswith("parts") else 1  # one launch per argument and part
    s0 = _stats(L)
    with _codegen(L, 2 + BOTH):
        got = TM._run(h2, sy, entry, sy.vin)
    s1 = _stats(L)
    assert s1.interp[MVLOOKUPS] == s0.interp[MVLOOKUPS] + calls and s1.gen[MVLOOKUPS] == s0.gen[MVLOOKUPS] + calls
    assert s1.failed == s0.failed
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ case 5: magnitude edges
def _constant_system(oracle, value, shuffles, mv):
    """every column, challenge, theta, beta, gamma, y and the incoming values are `value` on every row (constant polynomials), at k = 5
    with P = 4"""
    j, k = 4, 5
    n = 1 << k
    d, t_eval = oracle.domain_new(j, k)
    size = 1 << d.extended_k
    poly = TS._ro(to_mont([value] + [0] * (n - 1)))
    coset = TS._ro(to_mont([value] * size))
    fe = TS._ro(to_mont([value])[0])
    ev = Evaluator.new([], [], shuffles, mv)
    empty = np.zeros(0, dtype=np.uint32)
    common = {"k": k, "extended_k": d.extended_k, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
              "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
              "y": fe, "beta": fe, "gamma": fe, "theta": fe, "challenges": TS._ro(to_mont([value, value])),
              "advice_polys": [poly] * 3, "instance_polys": [poly], "custom": flatten_graph(ev.custom_gates),
              "perm_column_kind": empty, "perm_column_index": empty, "chunk_len": 2, "last_rotation": -4, "lookups": []}
    parts = {**common, "l0_poly": poly, "l_last_poly": poly, "l_active_row_poly": poly, "fixed_polys": [poly] * 2, "perm_product_polys": [], "perm_polys": []}
    full = {**common, "l0": coset, "l_last": coset, "l_active_row": coset, "fixed_cosets": [coset] * 2, "perm_product_cosets": [], "perm_cosets": []}
    return types.SimpleNamespace(parts=parts, full=full, shuffles=shuffles, mv=mv, z=[poly] * len(shuffles), phi=[poly] * len(mv), m=[poly] * len(mv),
                                 ev=ev, vin=coset, d=d, t_eval=t_eval, j=j, k=k)


# sums and differences of two products (the fused form), a Horner step whose addend is a product, a bare column, a constant and a challenge
EDGE_TUPLE = [('sum', ('prod', A(0), A(1, 1)), ('prod', F(0), ('challenge', 0))), ('prod', A(2), I(0)),
              ('sum', ('prod', A(0), F(1)), ('neg', ('prod', A(1), A(2, -1)))), A(1), ('const', R_MOD - 1), ('challenge', 1)]
_EDGE_WANT = {}


@pytest.mark.gpu
@pytest.mark.parametrize("fusion", [0, NO_FUSION], ids=["fused", "unfused"])
@pytest.mark.parametrize("value", [R_MOD - 1, 0, 1], ids=["r_minus_1", "zero", "one"])
@pytest.mark.parametrize("stage", ["shuffle", "mvlookup"])
def test_gpu_magnitude_edges(h2, oracle, stage, value, fusion):
    h2.init()
    L = h2.lib()
    if stage == "shuffle":
        sy = _constant_system(oracle, value, [(EDGE_TUPLE, EDGE_TUPLE[::-1])], [])
        run, model, idx = TS._run, TS._model, SHUFFLES
    else:
        sy = _constant_system(oracle, value, [], [([EDGE_TUPLE, EDGE_TUPLE[::-1], [A(0)]], EDGE_TUPLE[1:])])
        run, model, idx = TM._run, TM._model, MVLOOKUPS
    if (stage, value) not in _EDGE_WANT:
        _EDGE_WANT[stage, value] = model(h2, oracle, sy, sy.vin)
    want = _EDGE_WANT[stage, value]
    s0 = _stats(L)
    with _codegen(L, 2 + BOTH + fusion):
        for entry in ("full_host", "parts_device"):
            assert np.array_equal(run(h2, sy, entry, sy.vin), want), entry
    s1 = _stats(L)
    assert s1.gen[idx] == s0.gen[idx] + 5 and s1.interp[idx] == s0.interp[idx] and s1.failed == s0.failed  # the full form's launch and one per part
    with _codegen(L, 0):
        assert np.array_equal(run(h2, sy, "full_host", sy.vin), want)


# ------------------------------------------------------------------------------------------------ case 6: more arguments than a group
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("stage", ["shuffle", "mvlookup"])
def test_gpu_more_arguments_than_a_coset_group(h2, oracle, stage, entry):
    h2.init()
    L = h2.lib()
    if stage == "shuffle":
        sy = TS._system(oracle, 4, 7, 417, True, 3)
        run, want, idx = TS._run, TS._want(h2, oracle, sy), SHUFFLES
    else:
        sy = TM._system(oracle, 4, 5, 417, "with_all", 3)
        run, want, idx = TM._run, TM._want(h2, oracle, sy), MVLOOKUPS
    s0 = _stats(L)
    L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(1))
    try:
        with _codegen(L, 2 + BOTH):
            got = run(h2, sy, entry, sy.vin)
    finally:
        L.h2hip_debug_set_evalh_lookup_group_bytes(ctypes.c_uint64(0))
    s1 = _stats(L)
    assert np.array_equal(got, want)
    assert s1.gen[idx] == s0.gen[idx] + 3 * (4 if entry.startswith("parts") else 1) and s1.interp[idx] == s0.interp[idx]


# ------------------------------------------------------------------------------------------------ case 7: mode 1
@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["shuffle", "mvlookup"])
def test_gpu_background_compile_switches_the_stage_kernel(h2, oracle, stage):
    """mode 1 with the stage kernels wanted: a system no earlier test compiled runs interpreted while hiprtc compiles on a background
    thread, then generated; every call returns the model's values; the switch shows in the stage counter within two minutes"""
    h2.init()
    L = h2.lib()
    c = _salt()
    if stage == "shuffle":
        sy = _shuffle_system(oracle, TS._system(oracle, 4, 4, 404, False), [([A(0), ('scaled', A(1, 1), c)], [A(2), F(0)])], 434)
        run, want, idx = TS._run, TS._model(h2, oracle, sy, sy.vin), SHUFFLES
    else:
        sy = TM._system(oracle, 4, 5, 434, "alone", mv_override=((((A(0), ('scaled', A(1, 1), c)),), (F(0), F(1))),))
        run, want, idx = TM._run, TM._want(h2, oracle, sy), MVLOOKUPS
    s0 = _stats(L)
    deadline = time.time() + 120
    calls, switched = 0, False
    with _codegen(L, 1 + BOTH):
        while time.time() < deadline and not switched:
            assert np.array_equal(run(h2, sy, "full_host", sy.vin), want), "call %d" % calls
            calls += 1
            switched = _stats(L).gen[idx] > s0.gen[idx]
        s1 = _stats(L)
        assert s1.failed == s0.failed, L.h2hip_last_error()
        assert switched, "no generated kernel after %d calls in 120 s" % calls
        assert s1.interp[idx] > s0.interp[idx], "the first call cannot have found a compiled kernel"
        for _ in range(3):  # and after the switch
            assert np.array_equal(run(h2, sy, "full_host", sy.vin), want)
        assert _stats(L).gen[idx] == s1.gen[idx] + 3


# ------------------------------------------------------------------------------------------------ case 8: the backlog bound
@pytest.mark.gpu
def test_gpu_background_compilations_are_bounded(h2, oracle):
    """twelve distinct shuffle kernels asked for in one call in mode 1: at most eight background compilations are started for them (the
    call is over long before the first of them ends), the others are not recorded as failed and are asked for again; the values are the
    model's throughout"""
    h2.init()
    L = h2.lib()
    c = _salt()
    shuffles = [([A(0), ('scaled', A(1), c + i)], [A(2), F(0)]) for i in range(12)]
    sy = _shuffle_system(oracle, TS._system(oracle, 4, 4, 404, False), shuffles, 435)
    want = TS._model(h2, oracle, sy, sy.vin)
    with _codegen(L, 2 + NONE):  # whatever the gates need is compiled here, inline
        assert np.array_equal(TS._run(h2, sy, "full_host", sy.vin), want)
    _quiesce(L)
    s0 = _stats(L)
    with _codegen(L, 1 + BOTH):
        got = TS._run(h2, sy, "full_host", sy.vin)
        s1 = _stats(L)
        started = (s1.compiled - s0.compiled) + s1.pending
        assert np.array_equal(got, want)
        assert 1 <= started <= PENDING_BOUND, (started, s1.pending)
        assert s1.failed == s0.failed
        assert s1.gen[SHUFFLES] + s1.interp[SHUFFLES] == s0.gen[SHUFFLES] + s0.interp[SHUFFLES] + 12
        assert np.array_equal(TS._run(h2, sy, "full_host", sy.vin), want)  # the four left out ask again; nothing fails
        s2 = _stats(L)
        assert s2.failed == s0.failed and s2.pending <= PENDING_BOUND
