"""The mv-lookup grand sum (h2hip_mvlookup_sums_bn254[_device]) against the big-integer model of tests/mvlookup_util.py, and what the
call rejects before any device work.  Every comparison is limb for limb."""
import ctypes
import functools

import numpy as np
import pytest

from mvlookup_util import R_MOD, grand_sum, multiplicities, to_mont


def _ints(rng, count):
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _case(k, count, b, K, kind):
    """per argument: K inputs drawn from the table, the table, the model's m and phi; beta and the blinding values"""
    n = 1 << k
    u = n - b - 1
    rng = np.random.default_rng([k, count, b, K, len(kind)])
    beta = _ints(rng, 1)[0]
    f, t, m, phi, blinding = [], [], [], [], []
    for j in range(count):
        if kind == "all_r_minus_1":
            table, cols, bl = [R_MOD - 1] * n, [[R_MOD - 1] * n for _ in range(K)], [R_MOD - 1] * b
            beta = R_MOD - 1
        else:
            table = _ints(rng, n)
            if kind == "zero_denominator" and j == count - 1:  # T + beta == 0 at a row some inputs hit: those terms drop out too
                table[u // 2] = -beta % R_MOD
            cols = [[table[int(x)] for x in rng.integers(0, u, n)] for _ in range(K)]
            if kind == "zero_denominator" and j == count - 1:
                cols[0][u // 3] = cols[K - 1][u - 1] = -beta % R_MOD
            bl = _ints(rng, b)
        mj, miss = multiplicities(cols, table, b)
        assert not any(miss)
        if kind == "all_r_minus_1":
            assert mj[0] == K * u
        pj = grand_sum(cols, table, mj, beta, bl, b)
        if kind != "invalid":
            assert pj[u] == 0  # a valid argument's sum returns to zero, dropped terms or not: they drop on both sides
        f.append(cols), t.append(table), m.append(mj), phi.append(pj), blinding.append(bl)
    arrays = dict(f=[[to_mont(c) for c in cols] for cols in f], t=[to_mont(c) for c in t], m=[to_mont(c) for c in m],
                  phi=[to_mont(c) for c in phi], beta=to_mont([beta])[0], blinding=to_mont([v for bl in blinding for v in bl]))
    for x in [c for cols in arrays["f"] for c in cols] + arrays["t"] + arrays["m"] + arrays["phi"] + [arrays["beta"], arrays["blinding"]]:
        x.setflags(write=False)
    return arrays


def _host(h2, k, b, c):
    return h2.mvlookup_sums(k, c["beta"], c["f"], c["t"], c["m"], c["blinding"], b)


def _device(h2, k, b, c):
    import torch
    dev = lambda x: torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731
    d_f, d_t, d_m = [[dev(x) for x in cols] for cols in c["f"]], [dev(x) for x in c["t"]], [dev(x) for x in c["m"]]
    d_phi = [torch.full((1 << k, 4), -1, dtype=torch.int64, device="cuda") for _ in c["t"]]
    h2.mvlookup_sums_device(k, c["beta"], d_f, d_t, d_m, c["blinding"], b, d_phi)
    torch.cuda.synchronize()
    for tns, x in zip([x for cols in d_f for x in cols] + d_t + d_m, [x for cols in c["f"] for x in cols] + c["t"] + c["m"]):
        assert np.array_equal(tns.cpu().numpy().view(np.uint64), x)  # inputs are read-only
    return [x.cpu().numpy().view(np.uint64) for x in d_phi]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_sum_of_a_valid_argument_ends_in_zero_and_of_an_invalid_one_does_not():
    k, b, K = 5, 3, 3
    n = 1 << k
    u = n - b - 1
    rng = np.random.default_rng(11)
    table = _ints(rng, n)
    cols = [[table[int(x)] for x in rng.integers(0, u, n)] for _ in range(K)]
    m, miss = multiplicities(cols, table, b)
    phi = grand_sum(cols, table, m, 12345, [7] * b, b)
    assert phi[0] == 0 and phi[u] == 0 and phi[n - b:] == [7] * b and len(phi) == n and not any(miss)
    cols[1][4] = table[u]  # one input removed from the table: the engine's m counts what it found, and the sum no longer closes
    m, miss = multiplicities(cols, table, b)
    assert miss == [False, True, False]
    assert grand_sum(cols, table, m, 12345, [7] * b, b)[u] != 0


def test_rejections_need_no_gpu(h2):
    """H2HIP_EINVAL and a named error before the engine is entered"""
    L = h2.lib()
    buf = (ctypes.c_uint64 * 64)()
    one = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    tab = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    one_in = (ctypes.c_uint32 * 1)(1)
    big = (ctypes.c_void_p * 256)(*([ctypes.addressof(buf)] * 256))
    for fn, extra in ((L.h2hip_mvlookup_sums_bn254, ()), (L.h2hip_mvlookup_sums_bn254_device, (None,))):
        ok = [u32(4), one, tab, one_in, tab, tab, sz(1), buf, u32(1), tab]

        def rc_of(i, v, **more):
            args = list(ok)
            args[i] = v
            for q, x in more.items():
                args[int(q[1:])] = x
            return fn(*args, *extra)

        for i, v, text in ((2, None, b"null compressed_input"), (4, None, b"null compressed_table"), (5, None, b"null m"),
                           (9, None, b"null phi"), (1, None, b"null scalar"), (3, None, b"null n_inputs"),
                           (8, u32(15), b"blinding_factors + 1 >= 2^k"), (0, u32(29), b"k = 29 > 28"), (7, None, b"null blinding"),
                           (3, (ctypes.c_uint32 * 1)(0), b"n_inputs[0] = 0"), (3, (ctypes.c_uint32 * 1)(256), b"n_inputs[0] = 256"),
                           (6, sz(65536), b"count 65536 > 65535")):
            assert rc_of(i, v) == 1, text
            err = L.h2hip_last_error()
            assert err.startswith(b"mvlookup_sums: ") and text in err, err
        assert rc_of(3, (ctypes.c_uint32 * 1)(255), a0=u32(23), a2=big) == 1 and b"denominators > 2^30" in L.h2hip_last_error()
        assert rc_of(2, (ctypes.c_void_p * 1)(None)) == 1 and b"compressed_input[0] is null" in L.h2hip_last_error()
        assert rc_of(1, (ctypes.c_uint64 * 4)(*([2**64 - 1] * 4))) == 1  # beta not reduced
        assert fn(u32(4), one, None, None, None, None, sz(0), None, u32(1), None, *extra) == 0  # count == 0 writes nothing


def test_rows_per_thread_rule(h2):
    """the smallest (k, count) at which the scan takes more than one row per thread, read from the code's own rule"""
    assert _multi_row_case(h2) == (17, 3)


def _multi_row_case(h2):
    for k in range(4, 20):
        for count in (1, 2, 3):
            if h2.mvlookup_sum_rows(k, 5, count) > 1:
                return k, count
    raise AssertionError("no multi-row case below k = 20")


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", [4, 7, 11])
def test_gpu_sums_vs_model(h2, k, count, b, K, form):
    h2.init()
    c = _case(k, count, b, K, "random")
    got = (_host if form == "host" else _device)(h2, k, b, c)
    for j in range(count):
        assert np.array_equal(got[j], c["phi"][j]), j


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind,k,count,b,K", [("zero_denominator", 7, 3, 5, 4), ("zero_denominator", 11, 1, 1, 1), ("all_r_minus_1", 7, 3, 5, 4),
                                              ("all_r_minus_1", 4, 1, 1, 1)])
def test_gpu_sums_edges(h2, kind, k, count, b, K, form):
    """a zero denominator in an input and one in the table: each such term is dropped and the sum continues to phi[u] = 0 (the model
    asserts that); every element r - 1, beta and the blinding values too: every denominator r - 2, m[0] = K u"""
    h2.init()
    c = _case(k, count, b, K, kind)
    got = (_host if form == "host" else _device)(h2, k, b, c)
    for j in range(count):
        assert np.array_equal(got[j], c["phi"][j]), j


@pytest.mark.gpu
def test_gpu_sums_several_rows_per_thread(h2):
    """one case where a thread of the scan owns more than one row"""
    h2.init()
    k, count = _multi_row_case(h2)
    c = _case(k, count, 5, 1, "random")
    got = _device(h2, k, 5, c)
    for j in range(count):
        assert np.array_equal(got[j], c["phi"][j]), j
