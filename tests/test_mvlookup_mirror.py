"""The C++ mirror of the mv-lookup argument (halo2-pse_amd/host/evaluation.hpp plonk::mv_lookup::Argument and Evaluator::mv_lookups,
halo2hip.hpp mvlookup_multiplicities, mvlookup_sums and dev::verify's mv-lookups) through the stand-alone program
tests/cpp/test_mvlookup_mirror, against the Python model of tests/mvlookup_util.py on a k = 5 system."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mvlookup_util import R_MOD, Columns, compress_column, fold_mvlookups, from_mont, grand_sum, multiplicities, required_degree, to_mont

EXE = os.path.join(ROOT, "tests", "cpp", "test_mvlookup_mirror")
K, B, MAX_ROWS = 5, 2, 6
A = lambda c, r=0: ('advice', c, r)  # noqa: E731
F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
ARG = ([[A(0)], [A(1)]], [F(1)])  # the program's own: the prover's argument, the failing one, the evaluator's
BAD = ([[A(2)]], [F(1)])
ARG_EV = ([[A(0), ('prod', A(1), F(0))], [A(2), ('sum', A(3, 1), ('challenge', 0))]], [F(1), A(0, -1)])


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


def test_cpp_mvlookup_mirror_builds():
    """the Makefile target of the program; the required_degree of its evaluator argument -- a product of two queries in one input
    tuple, single queries in the other and in the table -- is 2 + 1 + (2 + 1)"""
    target = os.path.join("..", "tests", "cpp", "test_mvlookup_mirror")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.exists(EXE)
    assert required_degree(*ARG_EV) == 6 and required_degree(*ARG) == 5


@pytest.mark.gpu
def test_gpu_cpp_mvlookup_mirror(h2, tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    h2.init()
    n = 1 << K
    u = n - B - 1
    dom = h2.EvaluationDomain.new(4, K)
    size = 1 << dom.extended_k
    theta, beta, y, challenge = _ints(1, 4)
    f, t, c, d = (_ints(10 + i, n) for i in range(4))
    t[7] = t[3]  # a repeated table value: its count goes to row 3
    rng = np.random.default_rng(5)
    a, b = ([t[int(x)] for x in rng.integers(0, u, n)] for _ in range(2))  # valid: every input value is in the table's rows below u
    cols = [f, t, a, b, c, d]
    key = [_ints(20 + i, n) for i in range(3)]   # l0, l_last, l_active_row as coefficients
    blinding, values = _ints(30, B), _ints(31, size)
    blob = np.concatenate([np.array([K, B, MAX_ROWS], dtype=np.uint64)] +
                          [to_mont(v).reshape(-1) for v in ([theta], [beta], [y], [challenge], *cols, *key, blinding, values)])
    blob.tofile(tmp_path / "in.bin")
    r = subprocess.run([EXE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = np.fromfile(tmp_path / "out.bin", dtype=np.uint64)
    at = 0

    def take(count):
        nonlocal at
        v = out[at:at + count]
        at += count
        return v

    # the model
    lag = Columns([f, t], [a, b, c, d], [], [challenge], n)
    comp = [compress_column(e, theta, lag) for e in ARG[0] + [ARG[1]]]
    assert comp == [a, b, t]
    m, miss = multiplicities(comp[:2], comp[2], B)
    assert not any(miss) and m[7] == 0
    phi = grand_sum(comp[:2], comp[2], m, beta, blinding, B)
    assert phi[u] == 0
    live = set(t[:u])
    fails = [i for i in range(u) if c[i] not in live]
    polys = dom.lagrange_to_coeff_batch([to_mont(x) for x in cols] + [to_mont(phi), to_mont(m)])
    ext = lambda ps: [from_mont(x) for x in dom.coeff_to_extended_batch(ps)]  # noqa: E731
    cosets = ext(polys)
    l0, l_last, l_active = ext([to_mont(x) for x in key])
    P = size // n
    h = fold_mvlookups(values, [(ARG_EV[0], ARG_EV[1], None, cosets[6], cosets[7])], Columns(cosets[0:2], cosets[2:6], [], [challenge], size, P),
                       y, theta, beta, l0, l_last, l_active)

    assert list(take(2)) == [required_degree(*ARG_EV), required_degree(*ARG)]
    assert [from_mont(take(4 * n)) for _ in range(3)] == comp
    assert from_mont(take(4 * n)) == m
    assert from_mont(take(4 * n)) == phi
    n_fail = int(take(1)[0])
    got_fails = [tuple(int(x) for x in take(3)) for _ in range(n_fail)]
    assert len(fails) > MAX_ROWS and got_fails == [(4, 2, row) for row in fails[:MAX_ROWS]]  # kind 4 = MvLookup, input column 2 of all
    assert from_mont(take(4 * size)) == h
    assert from_mont(take(4 * size)) == h
    assert at == len(out)
