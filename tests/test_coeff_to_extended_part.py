"""coeff_to_extended_part (h2hip_coeff_to_extended_part_bn254_fr and its _device / _batch_device forms) against rows j * P + p of the
oracle's coeff_to_extended, limb for limb.

The scaling a[m] -> a[m] * g_p^m is fused into the transform's first-pass load (ntt.hip, ntt_load<PART>), which all four first-pass
kernels share, so every one of them is driven here:
  ntt_n1_part_kernel        k = 0
  ntt_final_part_kernel     k = 1, 6, 10 (one pass)
  ntt_strided_part_kernel   k = 11, 13 (default plans [6, 5], [7, 6]) and k = 12 with three passes forced by h2hip_debug_set_ntt_smax(4)
  ntt2_strided_part_kernel  the two-pass plan.  h2hip_debug_set_ntt_two_pass clamps its range to 2^16 .. 2^22, so the plan cannot be
                            forced at 2^12: it is forced at the hook's smallest size, k = 16, and also taken by default at k = 19.
P = 2, 4, 8 and parts 0, 1, P - 1; the last puts part * m at the top of the extended domain's two-level power table, across the lo / hi
split that h2hip_debug_evalh_power_table_bits reports.
"""
import ctypes
import os

import numpy as np
import pytest

NT = min(16, os.cpu_count() or 1)
EINVAL = 1
J_OF_LOG_P = {1: 3, 2: 5, 3: 9}  # EvaluationDomain::new(j, k): extended_k = k + log2(j - 1)


def _plan(h2, log_n, count=1):
    r = (ctypes.c_uint32 * 4)()
    p = h2.lib().h2hip_debug_ntt_plan(ctypes.c_uint32(log_n), ctypes.c_size_t(count), r)
    return list(r[:p])


def _restore(L):
    L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(8))
    L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(0), ctypes.c_uint32(0))


def _raw(v, n):
    """n copies of the stored word v (a reduced element's limbs as they lie in memory)"""
    return np.tile(np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64), (n, 1))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _parts_of(log_p):
    return sorted({0, 1, (1 << log_p) - 1})


# (id, k, log2 P values, hooks: None | ("smax", v) | ("two", lo, hi), the plan expected)
SIZES = [
    ("k0", 0, (1, 2, 3), None, [0]),
    ("k1", 1, (1, 2, 3), None, [1]),
    ("k6", 6, (1, 2, 3), None, [6]),
    ("k10", 10, (1, 2, 3), None, [10]),
    ("k11-strided", 11, (1, 2, 3), None, [6, 5]),
    ("k13-strided", 13, (1, 2, 3), None, [7, 6]),
    ("k12-three-passes", 12, (1, 2, 3), ("smax", 4), [4, 4, 4]),
    ("k16-two-pass-forced", 16, (1, 2, 3), ("two", 16, 16), [8, 8]),
    ("k19-two-pass", 19, (1,), None, [10, 9]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,log_ps,hook,plan", SIZES, ids=[s[0] for s in SIZES])
def test_part_vs_oracle(h2, oracle, name, k, log_ps, hook, plan):
    """random reduced, all-zero and all-(r - 1) inputs through every form: host and device, in place and out of place, a batch in which
    one source feeds all P parts, and a batch of five sources with mixed parts, each column also equal to the single call"""
    import torch
    L = h2.lib()
    n = 1 << k
    rnd = h2.to_numpy_u64(h2.gen_scalars_device(0xC2E0 + k, n))
    inputs = {"random": rnd, "zero": np.zeros((n, 4), dtype=np.uint64), "r-1": _raw(h2.FR_MODULUS - 1, n)}
    five = [h2.to_numpy_u64(h2.gen_scalars_device(0xC2F0 + 16 * k + i, n)) for i in range(5)] if k <= 13 else None
    try:
        if hook and hook[0] == "smax":
            L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(1), ctypes.c_uint32(0))
            L.h2hip_debug_set_ntt_smax(ctypes.c_uint32(hook[1]))
        elif hook:
            L.h2hip_debug_set_ntt_two_pass(ctypes.c_uint32(hook[1]), ctypes.c_uint32(hook[2]))
        assert _plan(h2, k) == plan, name
        for log_p in log_ps:
            P = 1 << log_p
            if k == 0:
                dom = h2.EvaluationDomain.new(J_OF_LOG_P[log_p], 0)
                want = {nm: None for nm in inputs}  # extended row p of a constant polynomial is the constant
            else:
                d, _ = oracle.domain_new(J_OF_LOG_P[log_p], k)
                dom = h2.EvaluationDomain.new(J_OF_LOG_P[log_p], k)
                assert d.extended_k == k + log_p == dom.extended_k
                want = {nm: oracle.coeff_to_extended(d, a.copy(), NT) for nm, a in inputs.items()}
            ek = dom.extended_k
            consts = (k, ek, dom.extended_omega, dom.g_coset, dom.g_coset_inv)

            def rows(nm, p):
                return inputs[nm] if want[nm] is None else want[nm][p::P]

            for p in _parts_of(log_p):
                tag = (name, P, p)
                for nm, a in inputs.items():
                    w = rows(nm, p)
                    assert np.array_equal(dom.coeff_to_extended_part(a, p), w), tag + (nm, "host")
                    d_a = _dev(a)
                    d_out = torch.full_like(d_a, 0x5A5A)
                    h2.coeff_to_extended_part_device(d_a, k, ek, p, *consts[2:], d_out=d_out)
                    assert np.array_equal(h2.to_numpy_u64(d_out), w) and np.array_equal(h2.to_numpy_u64(d_a), a), tag + (nm, "device")
                    h2.coeff_to_extended_part_device(d_a, k, ek, p, *consts[2:])
                    assert np.array_equal(h2.to_numpy_u64(d_a), w), tag + (nm, "device in place")
                # host form in place: out == a
                buf = rnd.copy()
                rc = L.h2hip_coeff_to_extended_part_bn254_fr(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(k), ctypes.c_uint32(ek), ctypes.c_uint32(p),
                                                             *[c.ctypes.data_as(ctypes.c_void_p) for c in consts[2:]], buf.ctypes.data_as(ctypes.c_void_p))
                assert rc == 0 and np.array_equal(buf, rows("random", p)), tag + ("host in place",)
            # one source feeds all P parts, one launch per pass
            src = _dev(rnd)
            outs = [torch.full_like(src, 0x5A5A) for _ in range(P)]
            h2.coeff_to_extended_part_batch_device([src] * P, outs, list(range(P)), *consts)
            for p in range(P):
                assert np.array_equal(h2.to_numpy_u64(outs[p]), rows("random", p)), (name, P, p, "batch of all parts")
            assert np.array_equal(h2.to_numpy_u64(src), rnd)
            if five is None:
                continue
            # five sources, mixed parts, two of them in place; each column against its single call
            parts = [P - 1, 0, 1 % P, P - 1, 0]
            srcs = [_dev(a) for a in five]
            lone = []
            for a, p in zip(srcs, parts):
                o = torch.empty_like(a)
                h2.coeff_to_extended_part_device(a, k, ek, p, *consts[2:], d_out=o)
                lone.append(o)
            outs = [srcs[0], torch.empty_like(srcs[1]), torch.empty_like(srcs[2]), srcs[3], torch.empty_like(srcs[4])]
            h2.coeff_to_extended_part_batch_device(srcs, outs, parts, *consts)
            for i in range(5):
                assert torch.equal(outs[i], lone[i]), (name, P, i, "batch of five")
            if k:
                w0 = oracle.coeff_to_extended(d, five[1].copy(), NT)
                assert np.array_equal(h2.to_numpy_u64(outs[1]), w0[parts[1]::P]), (name, P, "batch of five vs oracle")
    finally:
        _restore(L)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 6, 11, 13])
def test_single_coefficient_from_integers(h2, k):
    """a single coefficient c at index m: out[j] = c * g_p^m * omega^(j m), from Python integers -- the power's index arithmetic without
    the oracle.  P = 8, parts 0, 1 and 7; m = 0, 1, 2 and 2^k - 1, whose part * m reaches the top of the table's range"""
    F = h2.BN254_FR
    r = F.modulus
    n = 1 << k
    dom = h2.EvaluationDomain.new(9, k)
    ek = dom.extended_k
    P = 1 << (ek - k)
    assert P == 8
    lo_bits = ctypes.c_uint32(0)
    assert h2.lib().h2hip_debug_evalh_power_table_bits(dom.extended_omega.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(ek), ctypes.byref(lo_bits)) == 0
    assert lo_bits.value == min(ek, 10)
    ext_omega, zeta = dom.ints["extended_omega"], dom.ints["g_coset"]
    omega = pow(ext_omega, P, r)
    c = 0x1234567890ABCDEF0FEDCBA987654321 * 0x1F2E3D4C5B6A7988 % r
    srcs, outs, parts, expect = [], [], [], []
    import torch
    for m in sorted({0, 1, 2 % n, n - 1}):
        a = np.zeros((n, 4), dtype=np.uint64)
        a[m] = F.from_int(c)
        for p in (0, 1, P - 1):
            if ek > lo_bits.value and p == P - 1 and m == n - 1:
                # (P - 1)(2^k - 1): the largest exponent any call forms, in the last P-th of `hi`
                assert (p * m) >> lo_bits.value >= ((P - 1) << (ek - lo_bits.value)) // P - 1 > 0
            g_p = zeta * pow(ext_omega, p, r) % r
            v, step = c * pow(g_p, m, r) % r, pow(omega, m, r)
            want = np.empty((n, 4), dtype=np.uint64)
            for j in range(n):
                want[j] = F.from_int(v)
                v = v * step % r
            srcs.append(_dev(a))
            outs.append(torch.empty((n, 4), dtype=torch.int64, device="cuda"))
            parts.append(p)
            expect.append((m, p, want))
    h2.coeff_to_extended_part_batch_device(srcs, outs, parts, k, ek, dom.extended_omega, dom.g_coset, dom.g_coset_inv)
    for o, (m, p, want) in zip(outs, expect):
        assert np.array_equal(h2.to_numpy_u64(o), want), (k, m, p)


def test_rejections_before_any_device_work(h2):
    """k > extended_k, extended_k > 28, part >= P and null pointers answer H2HIP_EINVAL; none of them reaches the device, so this runs
    without one.  count == 0 writes nothing and succeeds."""
    L = h2.lib()
    dom = h2.EvaluationDomain.new(5, 4)  # k = 4, extended_k = 6, P = 4
    a = np.zeros((16, 4), dtype=np.uint64)
    out = np.zeros((16, 4), dtype=np.uint64)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    w, g, gi = vp(dom.extended_omega), vp(dom.g_coset), vp(dom.g_coset_inv)
    u32 = ctypes.c_uint32
    fake = ctypes.c_void_p(0x1000)  # a non-null "device pointer" that is never dereferenced: the call is rejected first

    def host(a_=vp(a), k=4, ek=6, part=0, w_=w, g_=g, gi_=gi, out_=vp(out)):
        return L.h2hip_coeff_to_extended_part_bn254_fr(a_, u32(k), u32(ek), u32(part), w_, g_, gi_, out_)

    def dev(a_=fake, k=4, ek=6, part=0, w_=w, g_=g, gi_=gi, out_=fake):
        return L.h2hip_coeff_to_extended_part_bn254_fr_device(a_, u32(k), u32(ek), u32(part), w_, g_, gi_, out_, None)

    for f in (host, dev):
        assert f(k=7, ek=6) == EINVAL
        assert f(k=27, ek=29) == EINVAL
        assert f(part=4) == EINVAL
        assert f(k=6, ek=6, part=1) == EINVAL  # P = 1
        assert f(a_=None) == EINVAL and f(out_=None) == EINVAL
        assert f(w_=None) == EINVAL and f(g_=None) == EINVAL and f(gi_=None) == EINVAL

    def batch(srcs=(0x1000, 0x1000), outs=(0x2000, 0x3000), parts=(0, 3), k=4, ek=6, w_=w, g_=g, gi_=gi, null=None):
        cnt = len(parts)
        s_arr = (ctypes.c_void_p * max(1, cnt))(*srcs) if null != "srcs" else None
        o_arr = (ctypes.c_void_p * max(1, cnt))(*outs) if null != "outs" else None
        p_arr = (u32 * max(1, cnt))(*parts) if null != "parts" else None
        return L.h2hip_coeff_to_extended_part_bn254_fr_batch_device(s_arr, o_arr, p_arr, ctypes.c_size_t(cnt), u32(k), u32(ek), w_, g_, gi_, None)

    assert batch(k=7, ek=6) == EINVAL
    assert batch(k=27, ek=29) == EINVAL
    assert batch(parts=(0, 4)) == EINVAL
    assert batch(null="srcs") == EINVAL and batch(null="outs") == EINVAL and batch(null="parts") == EINVAL
    assert batch(srcs=(0x1000, None)) == EINVAL and batch(outs=(None, 0x3000)) == EINVAL
    assert batch(w_=None) == EINVAL and batch(g_=None) == EINVAL and batch(gi_=None) == EINVAL
    assert batch(srcs=(), outs=(), parts=()) == 0
    assert not out.any()
