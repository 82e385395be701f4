"""The shuffle argument's witness check (h2hip_check_shuffles_bn254[_device]) against the model of tests/shuffle_util.py: input row
i < u fails when its value occurs a different number of times among the input rows below u than among the shuffle rows below u."""
import ctypes
import functools

import numpy as np
import pytest

from shuffle_util import R_MOD, check_result, failing_rows, to_mont

B = 3  # blinding factors


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _case(k):
    """four shuffles over 2^k rows and the rows the model names:
       0  S a permutation of A, A with a value repeated three times (equal multiplicities): passes
       1  the same value three times in A and twice in S (the third S row holds a fresh value): fails at exactly the three rows
       2  S a permutation of A on [0, u), and a value that occurs only in rows >= u of either side: ignored
       3  S unrelated to A: every row below u fails (more than max_rows of them)"""
    n = 1 << k
    u = n - B - 1
    rng = np.random.default_rng(50 + k)
    cols_a, cols_s = [], []
    # 0
    a = _ints(100 + k, n)
    rep = [1, u // 2, u - 1]
    for i in rep:
        a[i] = a[rep[0]]
    perm = [int(p) for p in rng.permutation(u)]
    s = [a[p] for p in perm] + _ints(101 + k, n - u)
    cols_a.append(a), cols_s.append(s)
    # 1
    s1 = list(s)
    s1[perm.index(rep[1])] = _ints(102 + k, 1)[0]
    cols_a.append(list(a)), cols_s.append(s1)
    # 2
    a2 = _ints(103 + k, n)
    perm2 = [int(p) for p in rng.permutation(u)]
    s2 = [a2[p] for p in perm2] + [a2[0]] * (n - u)  # a2[0] once more, but only in the rows that are never counted
    a2[u:] = [424242] * (n - u)
    cols_a.append(a2), cols_s.append(s2)
    # 3
    cols_a.append(_ints(104 + k, n)), cols_s.append(_ints(105 + k, n))
    want = [failing_rows(x, y, B) for x, y in zip(cols_a, cols_s)]
    assert want[0] == [] and want[1] == rep and want[2] == [] and want[3] == list(range(u))
    arrays = [to_mont(c) for c in cols_a], [to_mont(c) for c in cols_s]
    for x in arrays[0] + arrays[1]:
        x.setflags(write=False)
    return arrays[0], arrays[1], want


def _device(h2, k, a, s, max_rows):
    import torch
    dev = lambda x: torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731
    return h2.check_shuffles_device(k, [dev(x) for x in a], [dev(x) for x in s], B, max_rows)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_rejections_need_no_gpu(h2):
    """H2HIP_EINVAL and a named error before the engine is entered: a NULL table, b + 1 >= n, k > 28, null outputs, max_rows too large"""
    L = h2.lib()
    buf = (ctypes.c_uint64 * 64)()
    tab = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    for fn, extra in ((L.h2hip_check_shuffles_bn254, ()), (L.h2hip_check_shuffles_bn254_device, (None,))):
        ok = [u32(4), tab, tab, sz(1), u32(1), u32(4), buf, buf]

        def rc_of(i, v):
            args = list(ok)
            args[i] = v
            return fn(*args, *extra)

        for i, v, text in ((1, None, b"null compressed_input"), (2, None, b"null compressed_shuffle"), (4, u32(15), b"blinding_factors + 1 >= 2^k"),
                           (0, u32(29), b"k = 29 > 28"), (6, None, b"null counts"), (7, None, b"null rows"), (5, u32(65536), b"max_rows 65536"),
                           (3, sz(32768), b"count 32768")):
            assert rc_of(i, v) == 1, text
            err = L.h2hip_last_error()
            assert err.startswith(b"check_shuffles: ") and text in err, err
        assert rc_of(2, (ctypes.c_void_p * 1)(None)) == 1 and b"compressed_shuffle[0] is null" in L.h2hip_last_error()
        assert fn(u32(4), None, None, sz(0), u32(1), u32(4), None, None, *extra) == 0  # no shuffle: nothing to report


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 10])
def test_gpu_check_vs_model(h2, k):
    """equal multiplicities pass, unequal ones fail at exactly the rows of that value, rows >= u are ignored; max_rows below a count
    truncates and leaves UINT32_MAX in the unused slots; host and device forms agree and two runs are byte-identical"""
    h2.init()
    a, s, want = _case(k)
    u = (1 << k) - B - 1
    max_rows = 8
    assert max_rows < u
    wc, wr = check_result(want, max_rows)
    runs = [h2.check_shuffles(k, a, s, B, max_rows), h2.check_shuffles(k, a, s, B, max_rows), _device(h2, k, a, s, max_rows),
            _device(h2, k, a, s, max_rows)]
    for counts, rows in runs:
        assert np.array_equal(counts, wc) and np.array_equal(rows, wr)
        assert counts.tobytes() == runs[0][0].tobytes() and rows.tobytes() == runs[0][1].tobytes()
    assert list(wc) == [0, 3, 0, u] and list(wr[1]) == want[1] + [0xFFFFFFFF] * 5 and list(wr[3]) == list(range(max_rows))
    # every failing row of the last shuffle, and counts alone
    counts, rows = h2.check_shuffles(k, a[3:], s[3:], B, u + 4)
    assert counts[0] == u and list(rows[0]) == list(range(u)) + [0xFFFFFFFF] * 4
    counts, rows = h2.check_shuffles(k, a, s, B, 0)
    assert np.array_equal(counts, wc) and rows.shape == (4, 0)


@pytest.mark.gpu
def test_gpu_verify_witness_reports_shuffles(h2):
    """verify_witness(shuffles=...): a shuffle of 2-tuples compressed with the caller's theta, reported after the lookups; the default
    leaves the result as it was"""
    h2.init()
    k, n = 5, 32
    u = n - B - 1
    perm = [int(p) for p in np.random.default_rng(77).permutation(u)]
    a0, a1 = _ints(201, n), _ints(202, n)
    s0 = [a0[p] for p in perm] + _ints(203, n - u)
    s1 = [a1[p] for p in perm] + _ints(204, n - u)
    A = lambda c: ('advice', c, 0)  # noqa: E731
    shuffles = [([A(0), A(1)], [A(2), A(3)])]
    theta = to_mont([_ints(205, 1)[0]])[0]
    advice = [to_mont(c) for c in (a0, a1, s0, s1)]
    args = dict(gate_polys=[], lookups=[], theta=theta, blinding_factors=B, permutation_columns=[], mapping=None, advice=advice)
    assert h2.verify_witness(k, shuffles=shuffles, **args) == []
    bad = perm.index(4)
    s1[bad] = (s1[bad] + 1) % R_MOD  # the tuple that matched input row 4 no longer does
    advice[3] = to_mont(s1)
    assert h2.verify_witness(k, shuffles=shuffles, **args) == [("shuffle", 0, 4)]
    assert h2.verify_witness(k, **args) == []
