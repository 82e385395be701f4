"""The mv-lookup multiplicity columns (h2hip_mvlookup_multiplicities_bn254[_device]) against the big-integer model of
tests/mvlookup_util.py, and what the call rejects before any device work.  Every comparison is limb for limb."""
import ctypes
import functools

import numpy as np
import pytest

from mvlookup_util import R_MOD, lowest_missing, multiplicities, to_mont

KINDS = ["random", "repeated_table", "one_value", "missing", "zero_and_r_minus_1"]


def _ints(rng, count):
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _case(k, count, b, K, kind):
    """per argument: K input columns and a table (integers), the model's m columns and the pair the engine must name (or None)"""
    n = 1 << k
    u = n - b - 1
    rng = np.random.default_rng([k, count, b, K, KINDS.index(kind)])
    f, t, m, miss = [], [], [], []
    for j in range(count):
        table = _ints(rng, n)  # rows >= u hold values of their own, absent from rows < u
        if kind == "repeated_table":  # runs of equal values, scattered: the count must land on the lowest row of each
            pool = table[:max(2, u // 4)]
            table[:u] = [pool[int(x)] for x in rng.integers(0, len(pool), u)]
        if kind == "zero_and_r_minus_1":
            table[u - 1], table[0] = 0, R_MOD - 1
        pick = lambda: [table[int(x)] for x in rng.integers(0, u, n)]  # noqa: E731  (rows >= u are drawn too and must not count)
        cols = [pick() for _ in range(K)]
        if kind == "one_value":  # every input row the same value: one address takes every addition
            cols = [[table[u // 2]] * u + table[u:] for _ in range(K)]
        if kind == "zero_and_r_minus_1":
            for c in cols:
                c[0], c[u - 1], c[u // 2] = 0, R_MOD - 1, 0
        if kind == "missing" and j in (count - 1, min(1, count - 1)):  # a value that only rows >= u of the table hold
            cols[K - 1][u // 3] = table[u]
            if j == count - 1:
                cols[0][u - 1] = table[n - 1]
        mj, missj = multiplicities(cols, table, b)
        live = set(table[:u])
        assert sum(mj) == sum(1 for c in cols for r in range(u) if c[r] in live) and not any(mj[u:])
        f.append(cols), t.append(table), m.append(mj), miss.append(missj)
    named = lowest_missing(miss)
    assert (named is not None) == (kind == "missing")
    if kind == "repeated_table":
        assert any(m[0][i] == 0 and t[0][i] in t[0][:i] for i in range(u))
    arrays = dict(f=[[to_mont(c) for c in cols] for cols in f], t=[to_mont(c) for c in t], m=[to_mont(c) for c in m])
    for x in [c for cols in arrays["f"] for c in cols] + arrays["t"] + arrays["m"]:
        x.setflags(write=False)
    arrays["named"] = named
    return arrays


def _host(h2, k, b, c):
    return h2.mvlookup_multiplicities(k, c["f"], c["t"], b, partial=True)


def _device(h2, k, b, c):
    import torch
    dev = lambda x: torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731
    d_f, d_t = [[dev(x) for x in cols] for cols in c["f"]], [dev(x) for x in c["t"]]
    d_m = [torch.full((1 << k, 4), -1, dtype=torch.int64, device="cuda") for _ in c["t"]]
    msg = None
    try:
        h2.mvlookup_multiplicities_device(k, d_f, d_t, b, d_m)
    except h2.H2HipLookupError as e:
        msg = str(e)
    torch.cuda.synchronize()
    for tns, x in zip([x for cols in d_f for x in cols] + d_t, [x for cols in c["f"] for x in cols] + c["t"]):
        assert np.array_equal(tns.cpu().numpy().view(np.uint64), x)  # inputs are read-only
    return [x.cpu().numpy().view(np.uint64) for x in d_m], msg


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_counts_land_on_the_lowest_row():
    table = [7, 5, 7, 5, 9, 3, 3, 3]  # n = 8, b = 2: u = 5 rows count, on either side
    m, miss = multiplicities([[5, 7, 5, 9, 7, 1, 1, 1], [7, 7, 7, 9, 5, 2, 2, 2]], table, 2)
    assert m == [5, 3, 0, 0, 2, 0, 0, 0] and miss == [False, False]
    m, miss = multiplicities([[5, 3, 5, 9, 7, 1, 1, 1]], table, 2)
    assert m == [1, 2, 0, 0, 1, 0, 0, 0] and miss == [True]  # 3 occurs in table rows >= u only


def test_rejections_need_no_gpu(h2):
    """H2HIP_EINVAL and a named error before the engine is entered"""
    L = h2.lib()
    buf = (ctypes.c_uint64 * 64)()
    tab = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    one_in = (ctypes.c_uint32 * 1)(1)
    for fn, extra in ((L.h2hip_mvlookup_multiplicities_bn254, ()), (L.h2hip_mvlookup_multiplicities_bn254_device, (None,))):
        ok = [u32(4), tab, one_in, tab, sz(1), u32(1), tab]

        def rc_of(i, v):
            args = list(ok)
            args[i] = v
            return fn(*args, *extra)

        for i, v, text in ((1, None, b"null compressed_input"), (3, None, b"null compressed_table"), (6, None, b"null m"),
                           (2, None, b"null n_inputs"), (5, u32(15), b"blinding_factors + 1 >= 2^k"), (0, u32(29), b"k = 29 > 28"),
                           (2, (ctypes.c_uint32 * 1)(0), b"n_inputs[0] = 0"), (2, (ctypes.c_uint32 * 1)(256), b"n_inputs[0] = 256"),
                           (4, sz(65536), b"count 65536 > 65535")):
            assert rc_of(i, v) == 1, text
            err = L.h2hip_last_error()
            assert err.startswith(b"mvlookup_multiplicities: ") and text in err, err
        assert rc_of(1, (ctypes.c_void_p * 1)(None)) == 1 and b"compressed_input[0] is null" in L.h2hip_last_error()
        args = list(ok)
        args[0], args[2] = u32(28), (ctypes.c_uint32 * 1)(16)  # 16 columns of 2^28 rows: one row's count could pass 2^32 - 1
        assert fn(*args, *extra) == 1 and b"exceed a 32-bit count" in L.h2hip_last_error()
        assert fn(u32(4), None, None, None, sz(0), u32(1), None, *extra) == 0  # count == 0 writes nothing and needs no table


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", [4, 7, 11])
def test_gpu_multiplicities_vs_model(h2, k, count, b, K, kind, form):
    """random inputs drawn from the table; a table with repeated values (the count on the lowest row, the run's other rows zero); every
    input row one value; inputs equal to values that only table rows >= u hold (H2HIP_ELOOKUP, the outputs still the model's, the lowest
    (argument, input) named); the values 0 and r - 1.  Rows >= u of m are zero in all of them: the model's are."""
    h2.init()
    c = _case(k, count, b, K, kind)
    got, msg = (_host if form == "host" else _device)(h2, k, b, c)
    for j in range(count):
        assert np.array_equal(got[j], c["m"][j]), j
    if c["named"] is None:
        assert msg is None
    else:
        assert msg is not None and "argument %d, input %d:" % c["named"] in msg, msg
