"""The C++ mirror of the shuffle argument (halo2-pse_amd/host/evaluation.hpp plonk::shuffle::Argument and Evaluator::shuffles,
halo2hip.hpp shuffle_products and dev::verify's shuffles) through the stand-alone program tests/cpp/test_shuffle_mirror, against the
Python model of tests/shuffle_util.py on a k = 4 system."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shuffle_util import R_MOD, Columns, compress_column, failing_rows, fold_shuffles, from_mont, required_degree, shuffle_product, to_mont

EXE = os.path.join(ROOT, "tests", "cpp", "test_shuffle_mirror")
K, B, MAX_ROWS = 4, 2, 6
A = lambda c, r=0: ('advice', c, r)  # noqa: E731
SHUFFLE = ([A(0), ('prod', A(1), ('fixed', 0, 0))], [A(2), ('sum', A(3, 1), ('challenge', 0))])  # the program's own


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


def test_cpp_shuffle_mirror_builds():
    """the Makefile target of the program; the required_degree of its shuffle, a product of two queries on the input side, is 4"""
    target = os.path.join("..", "tests", "cpp", "test_shuffle_mirror")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.exists(EXE)
    assert required_degree(*SHUFFLE) == 4


@pytest.mark.gpu
def test_gpu_cpp_shuffle_mirror(h2, tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    h2.init()
    n = 1 << K
    dom = h2.EvaluationDomain.new(4, K)
    size = 1 << dom.extended_k
    theta, gamma, y, challenge = _ints(1, 4)
    cols = [_ints(10 + i, n) for i in range(5)]  # f, a, b, c, d: unrelated columns, so every input row below u fails the check
    key = [_ints(20 + i, n) for i in range(3)]   # l0, l_last, l_active_row as coefficients
    blinding, values = _ints(30, B), _ints(31, size)
    words = [K, B, MAX_ROWS]
    blob = np.concatenate([np.array(words, dtype=np.uint64)] +
                          [to_mont(v).reshape(-1) for v in ([theta], [gamma], [y], [challenge], *cols, *key, blinding, values)])
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
    lag = Columns([cols[0]], cols[1:], [], [challenge], n)
    a_col, s_col = compress_column(SHUFFLE[0], theta, lag), compress_column(SHUFFLE[1], theta, lag)
    z = shuffle_product(a_col, s_col, gamma, blinding, B)
    fails = failing_rows(a_col, s_col, B)
    polys = dom.lagrange_to_coeff_batch([to_mont(c) for c in cols] + [to_mont(z)])
    ext = lambda ps: [from_mont(c) for c in dom.coeff_to_extended_batch(ps)]  # noqa: E731
    cosets = ext(polys)
    l0, l_last, l_active = ext([to_mont(c) for c in key])
    P = size // n
    h = fold_shuffles(values, [(SHUFFLE[0], SHUFFLE[1], None, cosets[5])], Columns([cosets[0]], cosets[1:5], [], [challenge], size, P), y, theta,
                      gamma, l0, l_last, l_active)

    assert take(1)[0] == required_degree(*SHUFFLE)
    assert from_mont(take(4 * n)) == a_col and from_mont(take(4 * n)) == s_col
    assert from_mont(take(4 * n)) == z
    n_fail = int(take(1)[0])
    got_fails = [tuple(int(x) for x in take(3)) for _ in range(n_fail)]
    assert len(fails) > MAX_ROWS and got_fails == [(3, 0, row) for row in fails[:MAX_ROWS]]  # kind 3 = Shuffle
    assert from_mont(take(4 * size)) == h
    assert from_mont(take(4 * size)) == h
    assert at == len(out)
