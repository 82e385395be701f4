"""The shuffle argument's grand product (h2hip_shuffle_products_bn254[_device]) against the big-integer model of tests/shuffle_util.py,
and what the call rejects before any device work.  Field elements are canonical, so every comparison is np.array_equal."""
import ctypes
import functools

import numpy as np
import pytest

from shuffle_util import R_MOD, shuffle_product, to_mont


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _case(k, count, b, kind):
    """A, S (integers per shuffle), gamma, blinding (count x b integers) and the model's z columns"""
    n = 1 << k
    u = n - b - 1
    seed = 1000 * k + 10 * count + b
    if kind == "all_r_minus_1":
        a = [[R_MOD - 1] * n for _ in range(count)]
        s = [[R_MOD - 1] * n for _ in range(count)]
        gamma, blinding = R_MOD - 1, [[R_MOD - 1] * b for _ in range(count)]
    else:
        a = [_ints(seed + 100 * j, n) for j in range(count)]
        s = [_ints(seed + 100 * j + 50, n) for j in range(count)]
        gamma, blinding = _ints(seed + 7, 1)[0], [_ints(seed + 9 + j, b) for j in range(count)]
    zero_row = None
    if kind == "zero_denominator":  # one S + gamma == 0, in the last shuffle, away from both ends
        zero_row = u // 2
        s[-1][zero_row] = -gamma % R_MOD
    z = [shuffle_product(a[j], s[j], gamma, blinding[j], b) for j in range(count)]
    if zero_row is not None:
        assert z[-1][zero_row] != 0 and not any(z[-1][zero_row + 1:u + 1])
    arrays = dict(a=[to_mont(c) for c in a], s=[to_mont(c) for c in s], gamma=to_mont([gamma])[0],
                  blinding=to_mont([v for bl in blinding for v in bl]), z=[to_mont(c) for c in z])
    for v in arrays.values():
        for x in (v if isinstance(v, list) else [v]):
            x.setflags(write=False)
    return arrays


def _host(h2, k, b, c):
    return h2.shuffle_products(k, c["gamma"], c["a"], c["s"], c["blinding"], b)


def _device(h2, k, b, c):
    import torch
    dev = lambda x: torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731
    d_a, d_s = [dev(x) for x in c["a"]], [dev(x) for x in c["s"]]
    d_z = [torch.zeros((1 << k, 4), dtype=torch.int64, device="cuda") for _ in c["a"]]
    h2.shuffle_products_device(k, c["gamma"], d_a, d_s, c["blinding"], b, d_z)
    torch.cuda.synchronize()
    for t, x in zip(d_a + d_s, c["a"] + c["s"]):
        assert np.array_equal(t.cpu().numpy().view(np.uint64), x)  # inputs are read-only
    return [t.cpu().numpy().view(np.uint64) for t in d_z]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_product_of_a_valid_shuffle_ends_in_one():
    """the model itself: for S a permutation of A on [0, u) the product returns to one at row u"""
    k, b = 5, 3
    n = 1 << k
    u = n - b - 1
    a = _ints(1, n)
    perm = np.random.default_rng(2).permutation(u)
    s = [a[int(p)] for p in perm] + _ints(3, n - u)
    z = shuffle_product(a, s, 12345, [7] * b, b)
    assert z[0] == 1 and z[u] == 1 and z[n - b:] == [7] * b and len(z) == n


def test_rejections_need_no_gpu(h2):
    """H2HIP_EINVAL and a named error before the engine is entered: a NULL table, b + 1 >= n, k > 28, a null scalar"""
    L = h2.lib()
    buf = (ctypes.c_uint64 * 64)()
    one = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    tab = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    for fn, extra in ((L.h2hip_shuffle_products_bn254, ()), (L.h2hip_shuffle_products_bn254_device, (None,))):
        ok = [u32(4), one, tab, tab, sz(1), buf, u32(1), tab]

        def rc_of(i, v):
            args = list(ok)
            args[i] = v
            return fn(*args, *extra)

        for i, v, text in ((2, None, b"null compressed_input"), (3, None, b"null compressed_shuffle"), (7, None, b"null z"),
                           (1, None, b"null scalar"), (6, u32(15), b"blinding_factors + 1 >= 2^k"), (0, u32(29), b"k = 29 > 28"),
                           (5, None, b"null blinding")):
            assert rc_of(i, v) == 1, text
            err = L.h2hip_last_error()
            assert err.startswith(b"shuffle_products: ") and text in err, err
        assert rc_of(2, (ctypes.c_void_p * 1)(None)) == 1 and b"compressed_input[0] is null" in L.h2hip_last_error()
        assert fn(u32(4), one, None, None, sz(0), None, u32(1), None, *extra) == 0  # count == 0 writes nothing and needs no table


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", [4, 7, 11])
def test_gpu_products_vs_model(h2, k, count, b, form):
    h2.init()
    c = _case(k, count, b, "random")
    got = (_host if form == "host" else _device)(h2, k, b, c)
    for j in range(count):
        assert np.array_equal(got[j], c["z"][j]), j


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind,k,count,b", [("zero_denominator", 7, 3, 5), ("zero_denominator", 11, 1, 1), ("all_r_minus_1", 7, 3, 5),
                                            ("all_r_minus_1", 4, 1, 1)])
def test_gpu_products_edges(h2, kind, k, count, b, form):
    """a single zero denominator: z is zero from the next row on, in that shuffle alone; every element r - 1 (gamma and the blinding
    values too): the product stays one"""
    h2.init()
    c = _case(k, count, b, kind)
    got = (_host if form == "host" else _device)(h2, k, b, c)
    for j in range(count):
        assert np.array_equal(got[j], c["z"][j]), j
