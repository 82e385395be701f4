"""GPU: the round calls of the inner-product argument (include/halo2hip_ipa.h) against Python integers (tests/ipa_util.py; the oracle's
group sums above a few dozen points).
  * collapse: halves that straddle the normalisation's chunk of 8 and a workgroup of 256, both kernel forms (one lane / one quad of
    lanes per point) and the threshold between them, the scalars 0, 1, r - 1 and random ones, and the rows the group law treats apart;
    host and device forms agree limb for limb; at 2^13 points per half a random linear combination through the oracle's MSM;
  * powers, inner products and the fold: halves 1, 2, 64, 128, 2^12 -- one lane, one wave, one workgroup, several -- on zero and
    half-zero vectors, x in {0, 1, omega, random}, u in {1, r - 1, random}; the fused next-round values equal a separate call;
  * compute_s: k = 1 .. 10 whole, k = 20 sampled, and the protocol identity that ties it to the collapse and the MSM."""
import numpy as np
import pytest

import ipa_util as iu

pytestmark = pytest.mark.gpu
R = iu.R
SEED = bytes(range(1, 33))


@pytest.fixture(scope="module")
def ipa(h2):
    h2.init()
    return __import__("halo2_pse_amd.ipa", fromlist=["ipa"])


@pytest.fixture(scope="module")
def points(oracle):
    """2 * 257 distinct points, as limbs and as integers; computed once, read only"""
    limbs = oracle.gen_points(0x1A0001, 2 * 257, num_threads=1)
    return limbs, iu.g1_ints(limbs)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _expected_collapse(grp, lo, hi, u):
    """lo[i] + [u] hi[i]; the scalars 0, 1 and r - 1 need no multiplication"""
    if u == 0:
        return list(lo)
    if u == 1:
        return [grp.add(a, b) for a, b in zip(lo, hi)]
    if u == R - 1:
        return [grp.add(a, grp.neg(b)) for a, b in zip(lo, hi)]
    return grp.collapse(list(lo) + list(hi), u)


@pytest.fixture(scope="module")
def collapse_reference(oracle, points):
    """the expected collapse of the first 2 * half points for every tested half and scalar, computed once"""
    grp = iu.OracleSums(oracle)
    u_rand = iu.Rng(SEED).draw(1)[0]
    scalars = [u_rand, 1, R - 1, 0]
    _, ints = points
    want = {}
    for half in (1, 2, 3, 4, 7, 8, 9, 16, 255, 256, 257):
        for u in scalars:
            want[(half, u)] = _expected_collapse(grp, ints[:half], ints[half:2 * half], u)
    return scalars, want


@pytest.mark.parametrize("quad", [1, 0], ids=["lane", "quad"])
@pytest.mark.parametrize("half", [1, 2, 3, 7, 8, 9, 255, 256, 257])
def test_collapse_against_integers(h2, ipa, points, collapse_reference, half, quad):
    limbs, _ = points
    scalars, want = collapse_reference
    ipa.set_collapse_quad(quad)  # 1: every half above 1 takes the lane form; 0: the default, every half here takes the quad form
    try:
        for u in scalars:
            g = limbs[:2 * half]
            host = ipa.collapse(g, u)
            d_g = _dev(g)
            ipa.collapse_device(d_g, half, u)
            dev = h2.to_numpy_u64(d_g)[:half]
            assert np.array_equal(host, dev), (half, u)
            assert iu.g1_ints(host) == want[(half, u)], (half, u)
    finally:
        ipa.set_collapse_quad(0)


def test_collapse_at_the_threshold(h2, ipa, points, collapse_reference):
    """T = 8: halves 4 and 8 take the quad form, 16 the lane form"""
    limbs, _ = points
    scalars, want = collapse_reference
    assert ipa.set_collapse_quad(8) == 8
    try:
        for half in (4, 8, 16):
            for u in scalars:
                assert iu.g1_ints(ipa.collapse(limbs[:2 * half], u)) == want[(half, u)], (half, u)
    finally:
        ipa.set_collapse_quad(0)


@pytest.mark.parametrize("quad", [1, 0], ids=["lane", "quad"])
def test_collapse_crafted_rows(h2, ipa, points, quad):
    """identities on either side, a closing addition that is a doubling, and one whose result is (0, 0)"""
    grp = iu.Ints()
    _, ints = points
    ipa.set_collapse_quad(quad)
    try:
        for u in (iu.Rng(SEED, 1).draw(1)[0], R - 1, 1):
            hi = ints[:9]
            t = [grp.mul(p, u) for p in hi[:5]]
            lo = [ints[20], None, None, t[3], grp.neg(t[4])] + ints[30:34]
            hi = [None, hi[1], None] + hi[3:]
            want = [ints[20], t[1], None, grp.add(t[3], t[3]), None] + [grp.add(a, grp.mul(b, u)) for a, b in zip(lo[5:], hi[5:])]
            got = iu.g1_ints(ipa.collapse(iu.g1_limbs(lo + hi), u))
            assert got == want, u
    finally:
        ipa.set_collapse_quad(0)


@pytest.mark.parametrize("quad", [1, 0], ids=["lane", "quad"])
def test_collapse_large_by_random_combination(h2, ipa, oracle, quad):
    """half = 2^13 (the default threshold: the quad form's largest size, and 32 workgroups of the lane form):
    sum r_i out[i] = sum r_i g[i] + u sum r_i g[half + i] through the oracle's MSM"""
    half = 1 << 13
    g = oracle.gen_points(0x1A0002, 2 * half, num_threads=1)
    r = oracle.gen_scalars(0x1A0003, half, num_threads=1)
    u = iu.Rng(SEED, 2).draw(1)[0]
    ipa.set_collapse_quad(quad)
    try:
        d_g = _dev(g)
        ipa.collapse_device(d_g, half, u)
        out = h2.to_numpy_u64(d_g)[:half]
    finally:
        ipa.set_collapse_quad(0)
    lhs = oracle.best_multiexp(r, out)
    hi = oracle.g1_mul(oracle.g1_to_affine(oracle.best_multiexp(r, g[half:])), iu.fr_limbs([u])[0])
    rhs = oracle.g1_add(oracle.best_multiexp(r, g[:half]), hi)
    assert np.array_equal(oracle.g1_to_affine(lhs), oracle.g1_to_affine(rhs))
    assert all(oracle.g1_on_curve(out[i]) for i in range(0, half, 997))


def _inner(p, b, half):
    return (sum(x * y for x, y in zip(p[half:2 * half], b[:half])) % R, sum(x * y for x, y in zip(p[:half], b[half:2 * half])) % R)


@pytest.mark.parametrize("half", [1, 2, 64, 128, 1 << 12])
def test_powers_inner_products_and_fold(h2, ipa, half):
    n = 2 * half
    rng = iu.Rng(SEED, 100 + half.bit_length())
    omega = pow(iu.OMEGA_28, (1 << 28) // n, R)
    xs = [0, 1, omega] + rng.draw(1)
    us = [1, R - 1] + rng.draw(1)
    p_rand = rng.draw(n)
    polys = {"random": p_rand, "zero": [0] * n, "upper half zero": p_rand[:half] + [0] * half}
    for x in xs:
        b = [pow(x, i, R) for i in range(n)]
        d_b0 = ipa.powers_device(x, n)
        assert iu.fr_ints(h2.to_numpy_u64(d_b0)) == b, x
        for name, p in polys.items():
            for u in us:
                u_inv = pow(u, -1, R)
                d_p, d_b = _dev(iu.fr_limbs(p)), d_b0.clone()
                assert ipa.inner_products_device(d_p, d_b, half) == _inner(p, b, half), (name, x)
                p2 = [(p[i] + u_inv * p[half + i]) % R for i in range(half)]
                b2 = [(b[i] + u * b[half + i]) % R for i in range(half)]
                d_p1, d_b1 = d_p.clone(), d_b.clone()
                assert ipa.fold_device(d_p1, d_b1, half, u_inv, u) is None
                assert iu.fr_ints(h2.to_numpy_u64(d_p1)[:half]) == p2 and iu.fr_ints(h2.to_numpy_u64(d_b1)[:half]) == b2, (name, x, u)
                assert iu.fr_ints(h2.to_numpy_u64(d_p1)[half:]) == p[half:]  # the upper halves are read only
                if half >= 2:
                    values = ipa.fold_device(d_p, d_b, half, u_inv, u, next_values=True)
                    assert np.array_equal(h2.to_numpy_u64(d_p)[:half], h2.to_numpy_u64(d_p1)[:half])
                    assert np.array_equal(h2.to_numpy_u64(d_b)[:half], h2.to_numpy_u64(d_b1)[:half])
                    assert values == _inner(p2, b2, half // 2) == ipa.inner_products_device(d_p1, d_b1, half // 2), (name, x, u)


@pytest.mark.parametrize("k", range(1, 11))
def test_compute_s_against_integers(h2, ipa, k):
    rng = iu.Rng(SEED, 200 + k)
    u = rng.draw(k)
    if k % 3 == 0:
        u[k // 2] = 1
    if k % 4 == 0:
        u[0] = R - 1
    for init in (1, rng.draw(1)[0]):
        want = iu.compute_s(u, init)
        assert iu.fr_ints(ipa.compute_s(u, init)) == want
        assert iu.fr_ints(h2.to_numpy_u64(ipa.compute_s_device(u, init))) == want


def test_compute_s_sampled_at_k_20(h2, ipa):
    k = 20
    rng = iu.Rng(SEED, 220)
    u, init = rng.draw(k), rng.draw(1)[0]
    s = h2.to_numpy_u64(ipa.compute_s_device(u, init))
    idx = sorted({0, 1, (1 << k) - 1, 1 << 8, 1 << 16, (1 << 16) - 1} | {v % (1 << k) for v in rng.draw(4096)})
    got = iu.fr_ints(s[idx])
    for i, g in zip(idx, got):
        want = init
        for t in range(k):
            if (i >> t) & 1:
                want = want * u[k - 1 - t] % R
        assert g == want, i


def test_collapses_leave_the_point_compute_s_names(h2, ipa, oracle):
    """k = 8: k collapses of g with challenges u_0 .. u_{k-1} leave g[0] = <compute_s(u, 1), g>  (GuardIPA::compute_g)"""
    k = 8
    g = oracle.gen_points(0x1A0004, 1 << k, num_threads=1)
    u = iu.Rng(SEED, 230).draw(k)
    d_g = _dev(g)
    for j in range(k):
        ipa.collapse_device(d_g, 1 << (k - 1 - j), u[j])
    left = h2.to_numpy_u64(d_g)[0]
    right = h2.g1_to_affine(h2.msm_device(ipa.compute_s_device(u, 1), _dev(g), 1 << k))
    assert np.array_equal(left, right)
    assert np.array_equal(left, oracle.g1_to_affine(oracle.best_multiexp(iu.fr_limbs(iu.compute_s(u, 1)), g)))
