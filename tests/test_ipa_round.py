"""GPU: a round of the inner-product argument as one engine call (include/halo2hip_ipa_round.h) against the separate calls it replaces
-- msm_device, fold_device, collapse_device, inner_products_device -- which the other IPA tests hold to the integers.
  * the pair MSM (both sums of a round from one run of the MSM pipeline) against two msm_device calls, as affine integer pairs, at halves
    1, 2, 3, 5, 64, 257, 2^10, 2^13 and 2^14 (either side of the collapse's quad threshold), at the largest half the single two-set run
    takes and at twice that (the fall-back: two pipelined MSMs) -- the boundary read from the tuning values in force;
  * the two bucket groups stay apart: a zero half of p gives exactly the identity on one side and leaves the other as it was; equal and
    opposite halves of g, with p's halves equal too so that a point and its twin meet the same bucket index in every window, give the
    separate calls' sums (a doubling or a cancellation would need the two to share a bucket); identities in g, zero scalars in p,
    every scalar r - 1, all of p equal;
  * the round call against the sequence of separate calls at halves 1, 2, 64, 2^10, 2^13: first round (u = NULL), then u random, 1, and
    r - 1 on repeated generators (the collapse leaves identities): p, b and g[0 .. 2 half) limb for limb, the values limb for limb, L
    and R as affine points;
  * whole openings at k = 1, 2, 6, 10: the same bytes with the knob on and off, and verify_proof accepts them.
Scalars are random reduced elements; points are the generator kernel's try-and-increment points: uniform elements of the prime-order
group, i.e. random multiples of the generator whose logarithms nobody knows."""
import numpy as np
import pytest

import ipa_util as iu

pytestmark = pytest.mark.gpu
R = iu.R
SEED = bytes(range(11, 43))


@pytest.fixture(scope="module")
def ipa(h2):
    h2.init()
    return __import__("halo2_pse_amd.ipa", fromlist=["ipa"])


@pytest.fixture(scope="module")
def T(h2):
    return __import__("halo2_pse_amd.transcript", fromlist=["transcript"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _affine(h2, jac):
    """Jacobian limbs -> an affine integer pair (None: the identity)"""
    return iu.g1_ints(h2.g1_to_affine(jac))[0]


def _separate(h2, d_p, d_g, half):
    """(L, R) by the two calls of prover.rs:109-110"""
    return _affine(h2, h2.msm_device(d_p[half:], d_g, half)), _affine(h2, h2.msm_device(d_p, d_g[half:], half))


def _pair(h2, ipa, d_p, d_g, half):
    l, r = ipa.round_msms_device(d_p, d_g, half)
    return _affine(h2, l), _affine(h2, r)


@pytest.fixture(scope="module")
def pool(h2, ipa):
    """points and scalars in HBM for twice the largest fused half, generated once and read only: every size takes a prefix (or, from the top, a suffix)"""
    n = 4 * ipa.round_msms_fused_max_half()  # 2^21 with the default tuning
    return h2.gen_scalars_device(0x1A2001, n), h2.gen_points_device(0x1A2002, n)


HALVES = [1, 2, 3, 5, 64, 257, 1 << 10, 1 << 13, 1 << 14, "largest fused", "twice the largest fused"]


@pytest.mark.parametrize("half", HALVES, ids=[str(h).replace(" ", "_") for h in HALVES])
def test_pair_msm_against_two_msm_calls(h2, ipa, pool, half):
    fused_max = ipa.round_msms_fused_max_half()  # from Tuning::msm_fuse_max_n and msm_fuse_entries, not a constant of this test
    if half == "largest fused":
        half = fused_max
    elif half == "twice the largest fused":
        half = 2 * fused_max
    d_s, d_g = pool
    d_p, d_pts = d_s[:2 * half], d_g[:2 * half]
    want = _separate(h2, d_p, d_pts, half)
    assert want[0] is not None and want[1] is not None and want[0] != want[1]
    assert _pair(h2, ipa, d_p, d_pts, half) == want
    # read only
    if half <= 1 << 10:
        keep_p, keep_g = h2.to_numpy_u64(d_p).copy(), h2.to_numpy_u64(d_pts).copy()
        ipa.round_msms_device(d_p, d_pts, half)
        assert np.array_equal(h2.to_numpy_u64(d_p), keep_p) and np.array_equal(h2.to_numpy_u64(d_pts), keep_g)


def test_pair_msm_with_the_boundary_moved(h2, ipa, pool):
    """the same two sums from the single run and from the fall-back: the boundary follows the tuning values (2^10 pairs per sum, then
    2 half W <= 2^15 entries), and on either side of it the sums are the separate calls'"""
    d_s, d_g = pool
    L = h2.lib()
    try:
        for entries, max_n in ((0, 1 << 10), (1 << 15, 0)):
            L.h2hip_debug_set_msm_fuse_limits(entries, max_n)
            b = ipa.round_msms_fused_max_half()
            assert 1 <= b <= 1 << 10
            for half in (b, b + 1):
                d_p, d_pts = d_s[7:7 + 2 * half].clone(), d_g[5:5 + 2 * half].clone()
                assert _pair(h2, ipa, d_p, d_pts, half) == _separate(h2, d_p, d_pts, half), (entries, max_n, half)
    finally:
        L.h2hip_debug_set_msm_fuse_limits(0, 0)


def _neg_points(limbs):
    grp = iu.Ints()
    return iu.g1_limbs([grp.neg(p) for p in iu.g1_ints(limbs)])


@pytest.mark.parametrize("half", [64, 1 << 10])
def test_set_separation(h2, ipa, pool, half):
    import torch
    d_s, d_g = pool
    d_p, d_pts = d_s[:2 * half].clone(), d_g[:2 * half].clone()
    base = _separate(h2, d_p, d_pts, half)
    assert _pair(h2, ipa, d_p, d_pts, half) == base
    # a zero half of p: exactly the identity on that side, the other side as it was
    lo_zero = d_p.clone()
    lo_zero[:half] = 0
    assert _pair(h2, ipa, lo_zero, d_pts, half) == (base[0], None) == _separate(h2, lo_zero, d_pts, half)
    hi_zero = d_p.clone()
    hi_zero[half:] = 0
    assert _pair(h2, ipa, hi_zero, d_pts, half) == (None, base[1]) == _separate(h2, hi_zero, d_pts, half)
    assert _pair(h2, ipa, torch.zeros_like(d_p), d_pts, half) == (None, None)
    # g[half + i] = g[i] and g[half + i] = -g[i]: with random p, and with p[half + i] = p[i] -- then point i and its twin carry the same
    # digits, i.e. the same bucket index in every window, and only the set keeps them apart
    same = torch.cat([d_pts[:half], d_pts[:half]])
    opposite = torch.cat([d_pts[:half], _dev(_neg_points(h2.to_numpy_u64(d_pts[:half])))])
    p_twin = torch.cat([d_p[:half], d_p[:half]])
    for g_case, name in ((same, "same"), (opposite, "opposite")):
        for p_case in (d_p, p_twin):
            want = _separate(h2, p_case, g_case, half)
            assert want[0] is not None and want[1] is not None
            assert _pair(h2, ipa, p_case, g_case, half) == want, name
    l, r = _pair(h2, ipa, p_twin, same, half)
    assert l == r  # the same sum twice, not its double
    l, r = _pair(h2, ipa, p_twin, opposite, half)
    assert l == iu.Ints().neg(r) and l is not None  # opposite sums, not a cancellation
    # identities in g and zero scalars in p, scattered over both halves (and meeting at some indices)
    holes_g, holes_p = d_pts.clone(), d_p.clone()
    holes_g[[0, half - 1, half, half + 7 % half, 2 * half - 1]] = 0
    holes_p[[0, 3 % half, half, half + 7 % half, 2 * half - 2]] = 0
    assert _pair(h2, ipa, holes_p, holes_g, half) == _separate(h2, holes_p, holes_g, half)
    all_id = torch.zeros_like(d_pts)
    assert _pair(h2, ipa, d_p, all_id, half) == (None, None)
    # every scalar r - 1: L = -sum g[:half], R = -sum g[half:]; all of p equal to a random scalar: one bucket per window takes every point
    minus_one = _dev(np.tile(iu.fr_limbs([R - 1]), (2 * half, 1)))
    ones = _dev(np.tile(iu.fr_limbs([1]), (2 * half, 1)))
    got = _pair(h2, ipa, minus_one, d_pts, half)
    assert got == _separate(h2, minus_one, d_pts, half)
    plus = _pair(h2, ipa, ones, d_pts, half)
    grp = iu.Ints()
    assert got == (grp.neg(plus[0]), grp.neg(plus[1])) and plus[0] is not None
    equal = d_p[3:4].repeat(2 * half, 1).contiguous()
    assert _pair(h2, ipa, equal, d_pts, half) == _separate(h2, equal, d_pts, half)


def _round_by_separate_calls(h2, ipa, d_p, d_b, d_g, half, u, u_inv):
    if u is not None:
        ipa.fold_device(d_p, d_b, 2 * half, u_inv, u)
        ipa.collapse_device(d_g, 2 * half, u)
    l, r = _separate(h2, d_p, d_g, half)
    return l, r, ipa.inner_products_device(d_p, d_b, half)


@pytest.mark.parametrize("half", [1, 2, 64, 1 << 10, 1 << 13])
def test_round_call_against_the_separate_calls(h2, ipa, pool, half):
    import torch
    d_s, d_g = pool
    n = 4 * half
    top = d_s.shape[0]
    d_p0, d_b0, d_g0 = d_s[:n], d_s[top - n:], d_g[:n]  # b: any vector will do; the powers are the kernels test's matter
    u_rand = iu.Rng(SEED, half).draw(1)[0]
    repeated = torch.cat([d_g0[:2 * half], d_g0[:2 * half]])  # g[2 half + i] = g[i]: the collapse by r - 1 leaves identities
    cases = [(None, d_g0), (u_rand, d_g0), (1, d_g0), (R - 1, repeated), (u_rand, repeated)]
    for u, g_in in cases:
        u_inv = None if u is None else pow(u, -1, R)
        p1, b1, g1 = d_p0.clone(), d_b0.clone(), g_in.clone()
        p2, b2, g2 = d_p0.clone(), d_b0.clone(), g_in.clone()
        want_l, want_r, want_values = _round_by_separate_calls(h2, ipa, p1, b1, g1, half, u, u_inv)
        l, r, values = ipa.round_device(p2, b2, g2, half, u, u_inv)
        tag = (half, u)
        assert np.array_equal(h2.to_numpy_u64(p2), h2.to_numpy_u64(p1)), tag
        assert np.array_equal(h2.to_numpy_u64(b2), h2.to_numpy_u64(b1)), tag
        assert np.array_equal(h2.to_numpy_u64(g2)[:2 * half], h2.to_numpy_u64(g1)[:2 * half]), tag
        assert values == want_values, tag  # integers of canonical limbs: equal values are equal limbs
        assert (_affine(h2, l), _affine(h2, r)) == (want_l, want_r), tag
        if u is None:  # the first round writes nothing
            assert np.array_equal(h2.to_numpy_u64(p2), h2.to_numpy_u64(d_p0)) and np.array_equal(h2.to_numpy_u64(g2), h2.to_numpy_u64(g_in))
        if u == R - 1:
            assert not h2.to_numpy_u64(g2)[:2 * half].any() and want_l is None and want_r is None, tag
        else:
            assert want_l is not None and want_r is not None, tag


def test_round_call_values_are_limb_equal(h2, ipa, pool):
    """the eight limbs the C entry points write, not their integers: h2hip_ipa_round against h2hip_ipa_fold's next_values and against
    h2hip_ipa_inner_products"""
    d_s, _ = pool
    half = 1 << 10
    L = h2.lib()
    u = iu.Rng(SEED, 77).draw(1)[0]
    u_l, ui_l = h2.fr_from_int(u), h2.fr_from_int(pow(u, -1, R))
    d_g = pool[1][:4 * half].clone()
    p1, b1 = d_s[:4 * half].clone(), d_s[4 * half:8 * half].clone()
    p2, b2 = p1.clone(), b1.clone()
    v_fold, v_inner, v_round = (np.zeros((2, 4), dtype=np.uint64) for _ in range(3))
    out = np.zeros((2, 12), dtype=np.uint64)
    st = h2._stream()
    assert L.h2hip_ipa_fold_bn254_fr_device(h2._dptr(p1), h2._dptr(b1), 2 * half, h2._p(ui_l), h2._p(u_l), h2._p(v_fold), st) == 0
    assert L.h2hip_ipa_inner_products_bn254_fr_device(h2._dptr(p1), h2._dptr(b1), half, h2._p(v_inner), st) == 0
    assert L.h2hip_ipa_round_bn254_device(h2._dptr(p2), h2._dptr(b2), h2._dptr(d_g), half, h2._p(u_l), h2._p(ui_l), h2._p(out[0]), h2._p(out[1]),
                                          h2._p(v_round), st) == 0
    assert v_round.any() and np.array_equal(v_round, v_fold) and np.array_equal(v_round, v_inner)


_setups = {}


def _setup(ipa, oracle, k):
    if k not in _setups:
        pts = oracle.gen_points(0x1A3000 + k, (1 << k) + 2, num_threads=1)
        _setups[k] = ipa.ParamsIPA.from_parts(pts[:1 << k], pts[1 << k], pts[(1 << k) + 1])
    return _setups[k]


@pytest.mark.parametrize("k", [1, 2, 6, 10])
def test_whole_openings_keep_their_bytes(h2, ipa, T, oracle, k):
    params = _setup(ipa, oracle, k)
    rng = iu.Rng(SEED, stream_id=2000 + k)
    poly = rng.draw(1 << k)
    blind, x_3 = rng.draw(2)
    limbs = iu.fr_limbs(poly)
    proofs = {}
    try:
        for on in (True, False):
            assert ipa.set_round_call(on) is on
            w = T.Blake2bWrite()
            w.common_scalar(x_3)
            d_poly = _dev(limbs)
            ipa.create_proof(params, h2.FrRng(SEED), w, d_poly, blind, x_3)
            proofs[on] = w.finalize()
            assert np.array_equal(h2.to_numpy_u64(d_poly), limbs)
    finally:
        ipa.set_round_call(True)
    assert len(proofs[True]) == 32 * (1 + 2 * k + 2)
    assert proofs[True] == proofs[False], [i // 32 for i in range(0, len(proofs[True]), 32) if proofs[True][i:i + 32] != proofs[False][i:i + 32]]
    r = T.Blake2bRead(proofs[True])
    r.common_scalar(x_3)
    msm = params.empty_msm()
    msm.append_term(1, params.commit(limbs, blind))
    assert ipa.verify_proof(params, msm, r, x_3, iu.eval_poly(poly, x_3)).use_challenges().check()
