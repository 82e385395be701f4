"""The witness check on the GPU (csrc/check.hip): h2hip_check_gates_bn254, h2hip_check_permutation_bn254 and h2hip_check_lookups_bn254,
their device forms, the Python composition verify_witness and the C++ mirror dev::verify, against the Python restatement of
MockProver::verify's three loops in tests/check_util.py, which is first checked on its own against answers written out by hand."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import check_util as cu
import lookup_util as lu
import product_util as pu
from lookup_util import R_MOD

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF


def _ev():
    import evalh_util
    return evalh_util


def graphs_of(polys):
    ev = _ev()
    return [ev.flatten_graph(g) for g in ev.gate_check_graphs(polys)]


# ------------------------------------------------------------------ the restatement against hand-written answers (CPU)
def test_restated_loops_on_a_hand_written_system():
    n = 8
    s = [1, 1, 1, 1, 1, 0, 0, 0]
    a = [2, 3, 4, 5, 6, 7, 8, 9]
    b = [1, 1, 2, 1, 1, 1, 1, 1]
    # s(X) (a(X) b(wX) - c(w^-1 X)): c[i - 1] = a[i] b[i + 1] on rows 0 .. 4; c[7] (read by row 0) is right, c[2] is wrong
    c = [3 * 2, 4 * 1, 999, 6 * 1, 100, 101, 102, 2 * 1]
    cols = {"fixed": [s], "advice": [a, b, c], "instance": [[5, 0, 0, 0, 0, 0, 0, 1]]}
    polys = [("prod", ("fixed", 0, 0), ("sum", ("prod", ("advice", 0, 0), ("advice", 1, 1)), ("neg", ("advice", 2, -1)))),
             ("sum", ("sum", ("prod", ("challenge", 0), ("instance", 0, 0)), ("const", 5)), ("neg", ("advice", 0, 1))),
             ("advice", 1, 0), None]
    got = cu.gate_failures(polys, n, cols, [2])
    assert got[0] == [3]  # row 3 reads c[2]; row 0 reads c[7] through the wrap; rows 5 .. 7 are switched off
    assert got[2] == list(range(8)) and got[3] == []
    # lookups: u = 5; 9 is in the table only at row 6 (>= u); the bad input at row 5 is not looked at
    inp, tab = [1, 2, 9, 2, 1, 77, 1, 1], [1, 2, 3, 3, 3, 3, 9, 3]
    assert cu.lookup_failures([inp, [3] * 8], [tab, tab], 5) == [[2], []]
    # permutation: a 3-cycle (0,1) -> (1,2) -> (0,4) -> (0,1) with one wrong cell is reported at that cell and at its predecessor
    mp = np.zeros((2, n, 2), dtype=np.uint32)
    mp[:, :, 0] = np.arange(2)[:, None]
    mp[:, :, 1] = np.arange(n)[None, :]
    mp[0, 1], mp[1, 2], mp[0, 4] = (1, 2), (0, 4), (0, 1)
    x, y = list(range(10, 18)), list(range(20, 28))
    x[1] = x[4] = y[2] = 50
    assert cu.permutation_failures([x, y], mp) == [[], []]
    y[2] = 51
    assert cu.permutation_failures([x, y], mp) == [[1], [2]]
    assert cu.verify(n, {"fixed": [], "advice": [x, y], "instance": []}, [], [], [], 0, 5, [("advice", 0), ("advice", 1)], mp) == [
        ("permutation", 0, 1), ("permutation", 1, 2)]


def test_restated_gate_with_challenge_constant_and_instance():
    """challenge_0 p(X) + 5 - a(wX) with challenge_0 = 2 and p = -1 at row 7 only: row i < 7 is 5 - a[i + 1], row 7 wraps to a[0]"""
    a = [2, 3, 4, 5, 6, 7, 8, 9]
    cols = {"fixed": [], "advice": [a], "instance": [[0, 0, 0, 0, 0, 0, 0, R_MOD - 1]]}
    poly = ("sum", ("sum", ("prod", ("challenge", 0), ("instance", 0, 0)), ("const", 5)), ("neg", ("advice", 0, 1)))
    vals = [lu.eval_expr(poly, i, 8, cols, [2]) for i in range(8)]
    assert vals == [2, 1, 0, R_MOD - 1, R_MOD - 2, R_MOD - 3, R_MOD - 4, 1]
    assert cu.gate_failures([poly], 8, cols, [2]) == [[0, 1, 3, 4, 5, 6, 7]]


def test_one_corrupted_cell_of_a_three_cycle_fails_twice(h2):
    n = 16
    asm = h2.PermutationAssembly(n, 2)
    asm.copy(0, 3, 1, 5)
    asm.copy(1, 5, 1, 9)
    rng = random.Random(3)
    cols = [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(2)]
    cols[1][5] = cols[1][9] = cols[0][3]
    assert cu.permutation_failures(cols, asm.mapping) == [[], []]
    cols[1][9] += 1
    fails = cu.permutation_failures(cols, asm.mapping)
    assert sum(len(f) for f in fails) == 2 and 9 in fails[1]


# ------------------------------------------------------------------ arguments (CPU)
def _out(items, max_rows):
    return np.zeros(max(1, items), dtype=np.uint64), np.zeros(max(1, items * max_rows), dtype=np.uint32)


def test_check_calls_reject_bad_arguments(h2):
    """validation happens before any device work, so it answers the same with or without a GPU"""
    ev = _ev()
    L = h2.lib()
    k, n = 3, 8
    col = np.zeros((n, 4), dtype=np.uint64)
    good = graphs_of([("advice", 0, 0)])
    # gates: a graph reading y (the custom-gates fold), theta (a compression graph), or a column that is not there
    with pytest.raises(h2.H2HipError, match="rc=1.*reads"):
        h2.check_gates(k, [ev.flatten_graph(ev.custom_gates_graph([("advice", 0, 0)]))], advice=[col])
    with pytest.raises(h2.H2HipError, match="rc=1.*reads"):
        h2.check_gates(k, [ev.flatten_graph(ev.lookup_compress_graphs([("advice", 0, 0)], [("advice", 0, 0)])[0])], advice=[col])
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.check_gates(k, good, fixed=[col])
    with pytest.raises(h2.H2HipError, match="rc=1.*max_rows"):
        h2.check_gates(k, good, advice=[col], max_rows=65536)
    bad_fe = np.array([[0xFFFFFFFFFFFFFFFF] * 4], dtype=np.uint64)
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.check_gates(k, graphs_of([("challenge", 0)]), challenges=bad_fe)
    arr, keep = ev.graph_array(good)
    cp = (ctypes.c_void_p * 1)(col.ctypes.data)
    counts, rows = _out(1, 4)
    gates = lambda kk, g, ng, mr, cnt, rw: L.h2hip_check_gates_bn254(ctypes.c_uint32(kk), None, 0, cp, 1, None, 0, None, 0, g, ctypes.c_size_t(ng),  # noqa: E731
                                                                     ctypes.c_uint32(mr), cnt, rw)
    assert gates(29, arr, 1, 4, h2._p(counts), h2._p(rows)) == 1 and "28" in L.h2hip_last_error().decode()
    assert gates(3, arr, 1, 4, h2._p(counts), None) == 1 and "null rows" in L.h2hip_last_error().decode()  # NULL rows with max_rows > 0
    assert gates(3, arr, 1, 4, None, h2._p(rows)) == 1
    assert gates(3, None, 1, 4, h2._p(counts), h2._p(rows)) == 1
    assert gates(3, arr, 65536, 4, h2._p(counts), h2._p(rows)) == 1
    assert gates(3, None, 0, 4, None, None) == 0  # zero items write nothing
    dg = L.h2hip_check_gates_bn254_device  # the device form checks what is host memory
    assert dg(ctypes.c_uint32(3), None, 0, cp, 1, None, 0, None, 0, arr, ctypes.c_size_t(1), ctypes.c_uint32(65536), h2._p(counts), h2._p(rows), None) == 1
    assert dg(ctypes.c_uint32(3), None, 0, cp, 1, None, 0, None, 0, arr, ctypes.c_size_t(1), ctypes.c_uint32(4), h2._p(counts), None, None) == 1
    del keep
    # permutation: a pair out of range is named
    mp = np.zeros((2, n, 2), dtype=np.uint32)
    mp[:, :, 0] = np.arange(2)[:, None]
    mp[:, :, 1] = np.arange(n)[None, :]
    for cell, pair in (((1, 3), (2, 0)), ((0, 7), (0, n)), ((0, 0), (0xFFFFFFFF, 0))):
        bad = mp.copy()
        bad[cell] = pair
        with pytest.raises(h2.H2HipError, match=r"rc=1.*mapping\[%d\]\[%d\]" % cell):
            h2.check_permutation(k, [col, col], bad)
    with pytest.raises(h2.H2HipError, match="rc=1.*max_rows"):
        h2.check_permutation(k, [col, col], mp, max_rows=65536)
    maps = (ctypes.c_void_p * 2)(mp[0].ctypes.data, mp[1].ctypes.data)
    cp2 = (ctypes.c_void_p * 2)(col.ctypes.data, col.ctypes.data)
    perm = L.h2hip_check_permutation_bn254
    assert perm(ctypes.c_uint32(29), cp2, maps, ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None) == 1
    assert perm(ctypes.c_uint32(3), cp2, maps, ctypes.c_uint32(2), ctypes.c_uint32(2), h2._p(counts), None) == 1
    assert perm(ctypes.c_uint32(3), None, maps, ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None) == 1
    assert perm(ctypes.c_uint32(3), cp2, None, ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None) == 1
    assert perm(ctypes.c_uint32(3), None, None, ctypes.c_uint32(0), ctypes.c_uint32(0), None, None) == 0
    assert L.h2hip_check_permutation_bn254_device(ctypes.c_uint32(3), cp2, None, ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None, None) == 1
    # lookups
    for bf in (n - 1, n, 0xFFFFFFFF):  # blinding_factors + 1 >= n
        with pytest.raises(h2.H2HipError, match="rc=1.*blinding_factors"):
            h2.check_lookups(k, [col], [col], bf)
    with pytest.raises(h2.H2HipError, match="rc=1.*max_rows"):
        h2.check_lookups(k, [col], [col], 2, max_rows=65536)
    look = L.h2hip_check_lookups_bn254
    assert look(ctypes.c_uint32(3), cp, None, ctypes.c_size_t(1), ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None) == 1
    assert look(ctypes.c_uint32(3), cp, cp, ctypes.c_size_t(1), ctypes.c_uint32(2), ctypes.c_uint32(1), h2._p(counts), None) == 1
    assert look(ctypes.c_uint32(3), cp, cp, ctypes.c_size_t(32768), ctypes.c_uint32(2), ctypes.c_uint32(0), h2._p(counts), None) == 1
    assert look(ctypes.c_uint32(3), None, None, ctypes.c_size_t(0), ctypes.c_uint32(2), ctypes.c_uint32(0), None, None) == 0
    assert L.h2hip_check_lookups_bn254_device(ctypes.c_uint32(3), cp, cp, ctypes.c_size_t(1), ctypes.c_uint32(7), ctypes.c_uint32(0), h2._p(counts),
                                              None, None) == 1


_NO_GPU_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from conftest import load_pkg
import evalh_util as ev
h2 = load_pkg()
col = np.zeros((8, 4), dtype=np.uint64)
mp = np.zeros((1, 8, 2), dtype=np.uint32)
mp[0, :, 1] = np.arange(8)
graphs = [ev.flatten_graph(g) for g in ev.gate_check_graphs([("advice", 0, 0)])]
calls = [lambda: h2.check_gates(3, graphs, advice=[col]), lambda: h2.check_permutation(3, [col], mp), lambda: h2.check_lookups(3, [col], [col], 2),
         lambda: h2.verify_witness(3, [("advice", 0, 0)], [], np.zeros(4, np.uint64), 2, [], None, advice=[col])]
for i, f in enumerate(calls):
    try:
        f()
    except h2.H2HipError as e:
        assert "rc=2" in str(e), str(e)
    else:
        raise SystemExit("call %d succeeded without a GPU" % i)
print("loud")
"""


def test_check_calls_without_gpu_fail_loudly(tmp_path):
    """every valid call raises H2HipError (H2HIP_EDEVICE) when no device is visible: a fresh process with the GPUs hidden, so the test
    says the same on a machine with and without one"""
    script = tmp_path / "no_gpu.py"
    script.write_text(_NO_GPU_SCRIPT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("HALO2_HIP_DEVICES", None)
    r = subprocess.run([sys.executable, str(script), HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "loud" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ the engine against the restatement (GPU)
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _dev_map(mp):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(mp[j]).view(np.int32).copy()).cuda() for j in range(mp.shape[0])]


def assert_result(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: counts %s, expected %s" % (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), "%s: rows\n%s\nexpected\n%s" % (what, got[1], want[1])


def run_gates(h2, k, polys, cols, ch, max_rows, want=None, what="gates"):
    """host form and device form; both must equal the restatement (computed here unless given)"""
    n = 1 << k
    if want is None:
        want = cu.expected(cu.gate_failures(polys, n, cols, ch), max_rows)
    m = cu.mont_cols(cols)
    graphs = graphs_of(polys)
    chm = lu.to_mont(ch) if len(ch) else ()
    host = h2.check_gates(k, graphs, m["fixed"], m["advice"], m["instance"], chm, max_rows)
    assert_result(host, want, what + " (host form)")
    dev = h2.check_gates_device(k, graphs, [_dev(c) for c in m["fixed"]], [_dev(c) for c in m["advice"]], [_dev(c) for c in m["instance"]], chm,
                                max_rows)
    assert_result(dev, want, what + " (device form)")
    return host


def run_permutation(h2, k, columns, mapping, max_rows, what="permutation"):
    want = cu.expected(cu.permutation_failures(columns, mapping), max_rows)
    m = [lu.to_mont(c) for c in columns]
    host = h2.check_permutation(k, m, mapping, max_rows)
    assert_result(host, want, what + " (host form)")
    assert_result(h2.check_permutation_device(k, [_dev(c) for c in m], _dev_map(mapping), max_rows), want, what + " (device form)")
    return host


def run_lookups(h2, k, b, ins, tabs, max_rows, what="lookups"):
    want = cu.expected(cu.lookup_failures(ins, tabs, (1 << k) - b - 1), max_rows)
    mi, mt = [lu.to_mont(c) for c in ins], [lu.to_mont(c) for c in tabs]
    host = h2.check_lookups(k, mi, mt, b, max_rows)
    assert_result(host, want, what + " (host form)")
    assert_result(h2.check_lookups_device(k, [_dev(c) for c in mi], [_dev(c) for c in mt], b, max_rows), want, what + " (device form)")
    return host


GATE = ("prod", ("fixed", 0, 0), ("sum", ("prod", ("advice", 0, 0), ("advice", 1, 1)), ("neg", ("advice", 2, -1))))  # s (a b(wX) - c(w^-1 X))
WITH_CHALLENGE = ("sum", ("advice", 3, 0), ("neg", ("sum", ("sum", ("prod", ("challenge", 0), ("advice", 0, 0)), ("const", 5)), ("instance", 0, 0))))
BARE = ("advice", 4, 0)
K3_POLYS = [GATE, WITH_CHALLENGE, BARE, None]


def gate_witness(rng, n, ch):
    """columns that satisfy K3_POLYS at every row, wraps included, with the selector one everywhere"""
    rnd = lambda: rng.randrange(R_MOD)  # noqa: E731
    a, b, p = ([rnd() for _ in range(n)] for _ in range(3))
    c = [a[(j + 1) % n] * b[(j + 2) % n] % R_MOD for j in range(n)]
    d = [(ch * a[i] + 5 + p[i]) % R_MOD for i in range(n)]
    return {"fixed": [[1] * n], "advice": [a, b, c, d, [0] * n], "instance": [p]}


@pytest.mark.gpu
def test_gates_k3_wraps_and_blinding_rows(h2):
    k, n, u = 3, 8, 5
    rng = random.Random(0xC3)
    ch = [rng.randrange(R_MOD)]
    clean = gate_witness(rng, n, ch[0])
    assert cu.gate_failures(K3_POLYS, n, clean, ch) == [[], [], [], []]
    assert_result(run_gates(h2, k, K3_POLYS, clean, ch, 8, what="clean"), cu.expected([[], [], [], []], 8), "clean")
    neg = {**clean, "advice": [list(c) for c in clean["advice"]]}
    neg["advice"][2][n - 1] = (neg["advice"][2][n - 1] + 1) % R_MOD  # c(w^-1 X) at row 0 is c[n - 1]
    assert cu.gate_failures(K3_POLYS, n, neg, ch)[0] == [0]
    run_gates(h2, k, K3_POLYS, neg, ch, 8, what="negative wrap")
    pos = {**clean, "advice": [list(c) for c in clean["advice"]]}
    pos["advice"][1][0] = (pos["advice"][1][0] + 1) % R_MOD  # b(wX) at row n - 1 is b[0]
    pos["advice"][4][3] = 7                                  # the bare query
    pos["instance"] = [list(clean["instance"][0])]
    pos["instance"][0][6] = (pos["instance"][0][6] + 1) % R_MOD
    want = cu.gate_failures(K3_POLYS, n, pos, ch)
    assert want == [[n - 1], [6], [3], []]
    run_gates(h2, k, K3_POLYS, pos, ch, 8, what="positive wrap")
    # the blinding rows hold random values: with the selector zero there the gate is silent there, with it one it fails there
    blind = {**clean, "advice": [list(c) for c in clean["advice"]]}
    for col in blind["advice"]:
        for i in range(u, n):
            col[i] = rng.randrange(R_MOD)
    off = {**blind, "fixed": [[1] * u + [0] * (n - u)]}
    got_off = cu.gate_failures(K3_POLYS, n, off, ch)
    assert not set(got_off[0]) & set(range(u, n)) and set(got_off[2]) == set(range(u, n))
    run_gates(h2, k, K3_POLYS, off, ch, 8, what="selector off on the blinding rows")
    got_on = cu.gate_failures(K3_POLYS, n, blind, ch)
    assert set(range(u, n)) <= set(got_on[0])
    run_gates(h2, k, K3_POLYS, blind, ch, 8, what="selector on on the blinding rows")


def many_live_poly(n_live):
    """x_1 + (x_2 + (... + x_n)) - advice 5 with x_i = a(w^i X) b(X) i: the sum is right-deep, so every x_i is alive until the last exists"""
    xs = [("scaled", ("prod", ("advice", 0, i), ("advice", 1, 0)), 1000 + i) for i in range(1, n_live + 1)]
    acc = xs[-1]
    for x in reversed(xs[:-1]):
        acc = ("sum", x, acc)
    return ("sum", acc, ("neg", ("advice", 5, 0)))


@pytest.mark.gpu
def test_gates_k10_boundaries_limits_and_slot_tiers(h2):
    from test_evalh import _compile_stats
    k, n = 10, 1024
    rng = random.Random(0xC10)
    ch = [rng.randrange(R_MOD)]
    cols = gate_witness(rng, n, ch[0])
    big = many_live_poly(20)
    a, b = cols["advice"][0], cols["advice"][1]
    cols["advice"].append([sum(a[(r + i) % n] * b[r] * (1000 + i) for i in range(1, 21)) % R_MOD for r in range(n)])
    planted = [0, 63, 64, 255, 256, 500, 1023]  # wave, workgroup and last-row boundaries
    for r in planted:
        cols["advice"][2][(r - 1) % n] = (cols["advice"][2][(r - 1) % n] + 1) % R_MOD
    for r in (63, 64, 1023):
        cols["advice"][5][r] = (cols["advice"][5][r] + 1) % R_MOD
    polys = [GATE, big, WITH_CHALLENGE, None]
    fails = cu.gate_failures(polys, n, cols, ch)
    assert fails == [planted, [63, 64, 1023], [], []]
    stats = [_compile_stats(h2, g)[1] for g in graphs_of(polys)]
    assert stats[1] > 16 and stats[0] <= 8, stats  # programs of two slot tiers in one call (which runs both in the larger)
    # every graph of a call runs in the tier of its largest program: without the big polynomial the LDS tiers run over several workgroups
    small = [GATE, WITH_CHALLENGE, BARE, None]
    assert max(_compile_stats(h2, g)[1] for g in graphs_of(small)) <= 8
    assert_result(run_gates(h2, k, small, cols, ch, 8, what="the small tiers alone"), cu.expected([planted, [], [], []], 8), "small tiers")
    assert_result(run_gates(h2, k, [BARE, None], cols, ch, 8, what="the 4-slot tier"), cu.expected([[], []], 8), "4-slot tier")
    four = run_gates(h2, k, polys, cols, ch, 4, what="max_rows 4")
    assert int(four[0][0]) == 7 and list(four[1][0]) == [0, 63, 64, 255] and list(four[1][1]) == [63, 64, 1023, NONE]
    run_gates(h2, k, polys, cols, ch, 16, what="max_rows 16")
    zero = run_gates(h2, k, polys, cols, ch, 0, what="max_rows 0")
    assert zero[1].shape == (4, 0) and list(zero[0]) == [7, 3, 0, 0]
    h2.lib().h2hip_debug_set_evalh_max_local_slots(0)
    try:
        forced = run_gates(h2, k, polys, cols, ch, 16, what="global-workspace tier")
    finally:
        h2.lib().h2hip_debug_set_evalh_max_local_slots(256)
    assert_result(forced, cu.expected(fails, 16), "forced tier")


def tiled_shift_case(k, planted, seed):
    """s (a(wX) - b(X)) over 2^k rows without a big-integer loop: a tiles a 1024-row Montgomery block, b is a rolled by one row, and the
    planted rows of b are changed, so the failing rows are the planted ones by construction"""
    n = 1 << k
    rng = random.Random(seed)
    block = lu.to_mont([rng.randrange(R_MOD) for _ in range(1024)])
    a = np.tile(block, (n // 1024, 1))
    b = np.roll(a, -1, axis=0).copy()
    other = lu.to_mont([1])[0]
    for r in planted:
        b[r] = other if not np.array_equal(b[r], other) else block[0]
    s = np.tile(lu.to_mont([1]), (n, 1))
    poly = ("prod", ("fixed", 0, 0), ("sum", ("advice", 0, 1), ("neg", ("advice", 1, 0))))
    return poly, s, a, b


@pytest.mark.gpu
def test_gates_k20_grid_stride_in_the_global_workspace_tier(h2):
    """the one shape above a few thousand rows: past 256 x 2048 lanes the interpreter takes its rows grid-stride, and nothing lowers that"""
    k = 20
    planted = sorted({0, 63, 64, 4095, 4096, 262143, 262144, 524287, 524288, 524289, 786432 + 77, (1 << k) - 1})
    poly, s, a, b = tiled_shift_case(k, planted, 0xC20)
    h2.lib().h2hip_debug_set_evalh_max_local_slots(0)
    try:
        got = h2.check_gates_device(k, graphs_of([poly]), [_dev(s)], [_dev(a), _dev(b)], max_rows=16)
    finally:
        h2.lib().h2hip_debug_set_evalh_max_local_slots(256)
    assert_result(got, cu.expected([planted], 16), "k = 20")


@pytest.mark.gpu
def test_gates_are_deterministic(h2):
    k = 16
    rng = random.Random(0xDE)
    planted = sorted(rng.sample(range(1 << k), 300))
    poly, s, a, b = tiled_shift_case(k, planted, 0xDE7)
    ds, da, db = _dev(s), _dev(a), _dev(b)
    one = h2.check_gates_device(k, graphs_of([poly, None]), [ds], [da, db], max_rows=64)
    two = h2.check_gates_device(k, graphs_of([poly, None]), [ds], [da, db], max_rows=64)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    assert_result(one, cu.expected([planted, []], 64), "300 failures")


def cycle_values(rng, mapping, columns):
    """overwrite `columns` so that every cycle of the mapping holds one value"""
    m, n = mapping.shape[:2]
    seen = set()
    for j in range(m):
        for i in range(n):
            if (j, i) in seen or tuple(int(x) for x in mapping[j][i]) == (j, i):
                continue
            v, cell = rng.randrange(R_MOD), (j, i)
            while cell not in seen:
                seen.add(cell)
                columns[cell[0]][cell[1]] = v
                cell = tuple(int(x) for x in mapping[cell[0]][cell[1]])


@pytest.mark.gpu
def test_permutation_k4_cycles_within_and_across_columns(h2):
    k, n = 4, 16
    rng = random.Random(0xE4)
    asm = h2.PermutationAssembly(n, 3)  # an advice, a fixed and an instance column
    for c in ((0, 1, 0, 5), (0, 5, 0, 9), (0, 2, 1, 2), (1, 2, 2, 7), (2, 7, 0, 15), (1, 0, 1, 15), (2, 14, 2, 13)):  # rows 13 .. 15: blinding rows
        asm.copy(*c)
    cols = [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(3)]  # self-mapped cells hold differing values
    cycle_values(rng, asm.mapping, cols)
    assert cu.permutation_failures(cols, asm.mapping) == [[], [], []]
    run_permutation(h2, k, cols, asm.mapping, 16, "clean")
    cols[1][2] = (cols[1][2] + 1) % R_MOD  # one cell of the cycle (0,2) (1,2) (2,7) (0,15)
    fails = cu.permutation_failures(cols, asm.mapping)
    assert sum(len(f) for f in fails) == 2 and 2 in fails[1]
    run_permutation(h2, k, cols, asm.mapping, 16, "one corrupted cell")
    cols[1][15] = (cols[1][15] + 1) % R_MOD  # a blinding row
    assert 15 in cu.permutation_failures(cols, asm.mapping)[1]
    run_permutation(h2, k, cols, asm.mapping, 2, "a blinding row")


@pytest.mark.gpu
def test_permutation_k10_workgroup_boundaries_and_a_pair_out_of_range(h2):
    import torch
    k, n, m = 10, 1024, 3
    rng = random.Random(0xE10)
    asm = h2.PermutationAssembly(n, m)
    for _ in range(400):
        asm.copy(rng.randrange(m), rng.randrange(n), rng.randrange(m), rng.randrange(n))
    asm.copy(0, 255, 2, 256)
    asm.copy(1, 256, 1, 1023)
    cols = [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(m)]
    cycle_values(rng, asm.mapping, cols)
    for j, i in ((0, 255), (1, 256), (2, 0)):
        cols[j][i] = (cols[j][i] + 1) % R_MOD
    fails = cu.permutation_failures(cols, asm.mapping)
    assert 255 in fails[0] and 256 in fails[1]
    run_permutation(h2, k, cols, asm.mapping, 8)
    run_permutation(h2, k, cols, asm.mapping, 1, "max_rows 1")
    # the device form never follows a pair out of range: H2HIP_EINVAL after its one synchronisation, and the flag does not stick
    dcols = [_dev(lu.to_mont(c)) for c in cols]
    for cell, pair in (((2, 17), (m, 0)), ((0, n - 1), (0, n)), ((1, 0), (0xFFFFFFFF, 0xFFFFFFFF))):
        bad = asm.mapping.copy()
        bad[cell] = pair
        with pytest.raises(h2.H2HipError, match="rc=1.*mapping pair"):
            h2.check_permutation_device(k, dcols, _dev_map(bad), 8)
        torch.cuda.synchronize()
    assert_result(h2.check_permutation_device(k, dcols, _dev_map(asm.mapping), 8), cu.expected(fails, 8), "after a flagged call")


@pytest.mark.gpu
def test_lookups_k3_edges(h2):
    k, b, n, u = 3, 2, 8, 5
    big = [R_MOD - 1, R_MOD - 2, 1, 2, 3]  # values whose Montgomery-limb order differs from their canonical order
    assert sorted(big) != sorted(big, key=lu.mont_int)
    tab = big[:u] + [77, 78, 79]  # 77 .. 79 only in rows >= u
    cases = {
        "present only past u": [1, 77, 2, 3, 1] + [1, 1, 1],
        "a bad input past u": [1, 2, 3, 1, 2] + [555, 1, 1],
        "duplicates": [3, 3, 3, 2, 2] + [0, 0, 0],
        "all equal": [R_MOD - 1] * n,
        "all equal and missing": [4] * n,
        "smallest and largest": [1, R_MOD - 1, 1, R_MOD - 1, 0] + [0, 0, 0],
    }
    assert cu.lookup_failures([cases["present only past u"]], [tab], u) == [[1]]
    assert cu.lookup_failures([cases["a bad input past u"]], [tab], u) == [[]]
    assert cu.lookup_failures([cases["all equal and missing"]], [tab], u) == [[0, 1, 2, 3, 4]]
    assert cu.lookup_failures([cases["smallest and largest"]], [tab], u) == [[4]]
    names = sorted(cases)
    run_lookups(h2, k, b, [cases[c] for c in names], [tab] * len(names), 8)
    run_lookups(h2, k, b, [cases[c] for c in names], [tab] * len(names), 3, "max_rows 3")


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0, 64])
def test_lookups_k11_sort_shapes(h2, block):
    """two LK_TILE tiles: one merge pass; with an in-LDS block of 64 keys, five"""
    k, b = 11, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0xF11 + block)
    tab = rng.sample(range(1 << 16), n)  # a 16-bit range table
    inp = [rng.choice(tab[:u]) for _ in range(n)]
    have = set(tab[:u])
    missing = [v for v in range(1 << 16) if v not in have][:2]
    inp[5], inp[1500], inp[1024] = missing[0], missing[0], missing[1]  # two of the three misses are one value
    clean_tab = [rng.randrange(R_MOD) for _ in range(n)]
    clean_in = [rng.choice(clean_tab[:u]) for _ in range(n)]
    assert cu.lookup_failures([clean_in, inp], [clean_tab, tab], u) == [[], [5, 1024, 1500]]
    h2.set_lookup_sort(block)
    try:
        run_lookups(h2, k, b, [clean_in, inp], [clean_tab, tab], 8)
        assert h2.lookup_sort_stats() == ((64, 5) if block else (1024, 1))
    finally:
        h2.set_lookup_sort(0)


@pytest.mark.gpu
def test_lookup_check_agrees_with_lookup_permute(h2):
    """lookup_permute is H2HIP_ELOOKUP exactly when some count is non-zero, on the same columns"""
    k, b = 4, 3
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0xF4)
    tab = [rng.randrange(R_MOD) for _ in range(n)]
    good = [rng.choice(tab[:u]) for _ in range(n)]
    bad = list(good)
    bad[u - 1] = tab[u]  # present only past u
    blind = lu.to_mont([rng.randrange(R_MOD) for _ in range(2 * (b + 1))])
    for inp, fails in ((good, False), (bad, True)):
        counts, _ = run_lookups(h2, k, b, [inp], [tab], 4)
        assert bool(counts[0]) == fails
        if fails:
            with pytest.raises(h2.H2HipLookupError):
                h2.lookup_permute(k, [lu.to_mont(inp)], [lu.to_mont(tab)], blind, b)
        else:
            h2.lookup_permute(k, [lu.to_mont(inp)], [lu.to_mont(tab)], blind, b)


@pytest.mark.gpu
def test_pinned_columns_give_the_same_answer(h2):
    k, n = 10, 1024
    rng = random.Random(0xA1)
    ch = [rng.randrange(R_MOD)]
    cols = gate_witness(rng, n, ch[0])
    cols["advice"][2][100] = 1
    want = cu.expected(cu.gate_failures(K3_POLYS, n, cols, ch), 4)
    m = cu.mont_cols(cols)
    pinned = m["fixed"] + m["advice"][:2]
    h2.columns_pin(pinned)
    try:
        assert_result(h2.check_gates(k, graphs_of(K3_POLYS), m["fixed"], m["advice"], m["instance"], lu.to_mont(ch), 4), want, "pinned gates")
        asm = h2.PermutationAssembly(n, 2)
        asm.copy(0, 1, 1, 2)
        pc = [cols["advice"][0], cols["advice"][1]]
        assert_result(h2.check_permutation(k, m["advice"][:2], asm.mapping, 4), cu.expected(cu.permutation_failures(pc, asm.mapping), 4), "pinned permutation")
        assert_result(h2.check_lookups(k, [m["advice"][0]], [m["advice"][1]], 5, 4),
                      cu.expected(cu.lookup_failures([pc[0]], [pc[1]], n - 6), 4), "pinned lookups")
    finally:
        h2.columns_unpin(pinned)


@pytest.mark.gpu
def test_device_check_behind_evaluate_h_on_a_side_stream_then_host_check(h2):
    """a device check queued on a side stream directly behind an unsynchronised evaluate_h, and a host-form check at once: the three
    share the interpreter's workspaces and must not overtake each other"""
    import torch
    from evalh_util import DescHolder
    from test_evalh import load_case
    z = np.load(os.path.join(HERE, "golden", "evalh.npz"), allow_pickle=False)
    case, vin, vout = load_case(z, "k4")
    k, n = 12, 1 << 12
    rng = random.Random(0xA2)
    ch = [rng.randrange(R_MOD)]
    cols = gate_witness(rng, n, ch[0])
    cols["advice"][2][n - 1] = 3
    cols2 = gate_witness(rng, n, ch[0])
    cols2["advice"][4][2000] = 9
    want, want2 = (cu.expected(cu.gate_failures(K3_POLYS, n, c, ch), 4) for c in (cols, cols2))
    m, m2 = cu.mont_cols(cols), cu.mont_cols(cols2)
    graphs = graphs_of(K3_POLYS)
    dev_cols = [[_dev(c) for c in m[key]] for key in ("fixed", "advice", "instance")]
    keep, tens = [], {}
    for key in ("fixed_cosets", "advice_polys", "instance_polys", "perm_product_cosets", "perm_cosets"):
        tens[key] = [_dev(a) for a in case[key]]
    lk = [[_dev(p) for p in l[1:]] for l in case["lookups"]]
    hd = DescHolder(case)
    d = hd.desc

    def table(ts):
        arr = (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        keep.append(arr)
        return ctypes.addressof(arr)

    d.fixed_cosets, d.advice_polys, d.instance_polys = table(tens["fixed_cosets"]), table(tens["advice_polys"]), table(tens["instance_polys"])
    d.perm_product_cosets, d.perm_cosets = table(tens["perm_product_cosets"]), table(tens["perm_cosets"])
    l0, l_last, l_active = _dev(case["l0"]), _dev(case["l_last"]), _dev(case["l_active_row"])
    d.l0, d.l_last, d.l_active_row = l0.data_ptr(), l_last.data_ptr(), l_active.data_ptr()
    d.lookup_product_polys, d.lookup_permuted_input_polys, d.lookup_permuted_table_polys = (table([l[i] for l in lk]) for i in range(3))
    d_values = _dev(vin)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc = h2.lib().h2hip_evaluate_h_bn254_device(hd.byref(), ctypes.c_void_p(d_values.data_ptr()), ctypes.c_void_p(side.cuda_stream))
        assert rc == 0, h2.lib().h2hip_last_error()
        got = h2.check_gates_device(k, graphs, *dev_cols, lu.to_mont(ch), 4)
    got2 = h2.check_gates(k, graphs, m2["fixed"], m2["advice"], m2["instance"], lu.to_mont(ch), 4)  # host form on the engine's stream, at once
    side.synchronize()
    assert_result(got, want, "device check on the side stream")
    assert_result(got2, want2, "host check")
    assert np.array_equal(h2.to_numpy_u64(d_values), vout), "evaluate_h"


def system_case(h2, seed, k, b):
    n = 1 << k
    cols = cu.system_witness(random.Random(seed), k, b)
    asm = h2.PermutationAssembly(n, 3)
    for c in cu.SYSTEM_COPIES:
        asm.copy(*c)
    return cols, asm


def z_at_u(h2, k, b, cols, mapping, theta, rng):
    """the grand products of the same columns at row u: ([permutation z(u) == 1], [lookup z(u) == 1]); the lookup list is None when
    lookup_permute finds an input value missing"""
    n, u = 1 << k, (1 << k) - b - 1
    dom = h2.EvaluationDomain.new(3, k)
    one = lu.to_mont([1])[0]
    m = cu.mont_cols(cols)
    pc = [m[kind][i] for kind, i in cu.SYSTEM_PERM]
    sigma = h2.permutation_keygen(dom, mapping, want=("permutations",))["permutations"]
    beta, gamma = pu.fe(rng.randrange(R_MOD)), pu.fe(rng.randrange(R_MOD))
    zp = h2.permutation_products(k, dom.omega, h2.fr_from_int(h2.FR_DELTA), beta, gamma, pc, sigma, 3, lu.to_mont([rng.randrange(R_MOD) for _ in range(b)]), b)
    perm_ok = [bool(np.array_equal(z[u], one)) for z in zp]
    ci = [lu.to_mont(lu.compress(i, theta, n, cols, [5])) for i, _ in cu.SYSTEM_LOOKUPS]
    ct = [lu.to_mont(lu.compress(t, theta, n, cols, [5])) for _, t in cu.SYSTEM_LOOKUPS]
    try:
        pa, pt = h2.lookup_permute(k, ci, ct, lu.to_mont([rng.randrange(R_MOD) for _ in range(2 * (b + 1))]), b)
    except h2.H2HipLookupError:
        return perm_ok, None
    zl = h2.lookup_products(k, beta, gamma, ci, ct, pa, pt, lu.to_mont([rng.randrange(R_MOD) for _ in range(b)]), b)
    return perm_ok, [bool(np.array_equal(z[u], one)) for z in zl]


@pytest.mark.gpu
def test_verify_witness_and_the_grand_products(h2):
    k, b = 6, 5
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0xA3)
    theta = rng.randrange(R_MOD)
    cols, asm = system_case(h2, 0xA30, k, b)
    verify = lambda c: h2.verify_witness(k, cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, pu.fe(theta), b, cu.SYSTEM_PERM, asm.mapping,  # noqa: E731
                                         **cu.mont_cols(c), challenges=lu.to_mont([5]))
    assert cu.verify(n, cols, [5], cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, theta, u, cu.SYSTEM_PERM, asm.mapping) == []
    assert verify(cols) == []
    assert z_at_u(h2, k, b, cols, asm.mapping, theta, rng) == ([True], [True])
    cols["advice"][0][3] = (cols["advice"][0][3] + 1) % R_MOD  # a cell in a gate, a copy cycle and a lookup input
    want = cu.verify(n, cols, [5], cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, theta, u, cu.SYSTEM_PERM, asm.mapping)
    assert [f[0] for f in want] == ["gate", "lookup", "permutation", "permutation"]
    assert verify(cols) == want
    assert z_at_u(h2, k, b, cols, asm.mapping, theta, rng) == ([False], None)


@pytest.mark.gpu
@pytest.mark.parametrize("corrupt", [False, True])
def test_cpp_mirror_verify(h2, tmp_path, corrupt):
    """tests/cpp/test_check_mirror runs dev::verify of host/halo2hip.hpp on the system of check_util; its failures against the restatement"""
    exe = os.path.join(HERE, "cpp", "test_check_mirror")
    k, b, max_rows = 6, 5, 8
    n, u = 1 << k, (1 << k) - b - 1
    rng = random.Random(0xA4)
    theta, ch = rng.randrange(R_MOD), rng.randrange(R_MOD)
    cols, asm = system_case(h2, 0xA40, k, b)
    if corrupt:
        cols["advice"][0][3] = (cols["advice"][0][3] + 1) % R_MOD
        cols["advice"][2][20] = (cols["advice"][2][20] + 1) % R_MOD
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    blob = [np.array([k, b, max_rows, len(cu.SYSTEM_COPIES)], dtype=np.uint64), lu.to_mont([theta, ch]).reshape(-1)]
    blob += [lu.to_mont(c).reshape(-1) for c in cols["fixed"] + cols["advice"] + cols["instance"]]
    blob += [np.array(cu.SYSTEM_COPIES, dtype=np.uint64).reshape(-1)]
    np.concatenate(blob).astype(np.uint64).tofile(inp)
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=120)
    got = np.fromfile(outp, dtype=np.uint64)
    kinds = ["gate", "lookup", "permutation"]
    fails = [(kinds[int(got[1 + 3 * i])], int(got[2 + 3 * i]), int(got[3 + 3 * i])) for i in range(int(got[0]))]
    want = cu.verify(n, cols, [ch], cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, theta, u, cu.SYSTEM_PERM, asm.mapping)
    assert bool(want) == corrupt
    assert fails == want
