"""The curve-point FFT (csrc/ecfft.hip: g_to_lagrange, ParamsKZG::downsize, best_fft::<G1>) on inputs that make its butterflies
exceptional cases of the group law: a + t and a - t with t == a (a doubling), t == -a (the identity) or an operand the identity.

The inputs are built in the exponent (g1fft_util.py): P_i = [a_i]G, expected out_j = [s sum_i a_i w^(i j)]G from the definition.  The
unmarked tests check the constructions themselves -- the butterfly classes each input exists to hit, counted by a simulation of the
reference's network on the scalars -- and the oracle's own exceptional-case handling against the definition.  The GPU tests run the
three code paths of ecfft.hip (lazy quad, normalised quad, one lane; h2hip_debug_set_g2l_quad 1, 3, 0) and compare affine outputs limb
for limb: no tolerance is involved."""
import ctypes
import random

import numpy as np
import pytest

import g1fft_util as gu
from product_util import R_MOD

G2L_KS = (1, 2, 3, 6, 9)      # a lone twiddle-one butterfly; the first non-trivial twiddle; one quad-wave; two waves; 64 normalise lanes
PLANTED_KS = (4, 7)
BIG_K = 15                    # the smallest size beyond the quad range (k > 14): one lane per butterfly, normalised between layers
FFT_KS = (1, 3, 6)
FFT_NAMES = ("tone3", "tone_last", "const", "planted")
MODES = (1, 3, 0)             # lazy quad (default), normalised quad, one lane per butterfly


def _cases(ks, names):
    return [pytest.param(name, k, id="%s-k%d" % (name, k)) for k in ks for name in names if gu.exists(name, 1 << k)]


G2L_CASES = _cases(G2L_KS, gu.NAMES) + _cases(PLANTED_KS, ("planted", "planted2"))
BIG_CASES = _cases((BIG_K,), gu.CLOSED_FORM)
FFT_CASES = _cases(FFT_KS, FFT_NAMES)
ORACLE_KS = (1, 2, 3, 4, 6, 7)  # the oracle against the definition on the CPU; k = 9 is compared in the GPU tests


# ------------------------------------------------------------------------------------------------- CPU: the constructions
@pytest.mark.parametrize("inverse", [True, False], ids=["omega_inv", "omega"])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8])
def test_simulated_butterflies_equal_the_definition(oracle, k, inverse):
    """the simulation that counts the classes computes the O(n^2) sum, on random and on structured scalars"""
    w = gu.omega_of(oracle, k, inverse)
    n = 1 << k
    assert pow(w, n, R_MOD) == 1 and (k == 0 or pow(w, n // 2, R_MOD) == R_MOD - 1)
    rng = random.Random(77 + k)
    inputs = [[rng.randrange(R_MOD) for _ in range(n)]]
    inputs += [gu.scalars(name, n, w) for name in gu.NAMES if k and gu.exists(name, n)]
    for a in inputs:
        out, counts = gu.simulate(a, w, k)
        assert out == gu.dft(a, w)
        assert len(counts) == k and all(sum(c.values()) == n // 2 for c in counts)
    _, counts = gu.simulate(inputs[0], w, k)
    assert all(c["plain"] == n // 2 for c in counts)  # random data reaches none of the exceptional classes


def test_closed_form_expectations_equal_the_definition(oracle):
    """what the tests of 2^15 points expect is written down directly; the same expressions at sizes the O(n^2) sum reaches"""
    for k in (1, 2, 5):
        for inverse in (True, False):
            w = gu.omega_of(oracle, k, inverse)
            for name in gu.CLOSED_FORM:
                a = gu.scalars(name, 1 << k, w)
                assert gu.expected_scalars(name, 1 << k, w, a, 1) == gu.dft(a, w), (name, k)


def _planted_counts(n, inner=False):
    signs = [s for _, s in gu.planted_spots(n, inner)]
    return signs.count(1), signs.count(-1)


def _check_classes(name, k, counts):
    """the classes a named input exists to hit"""
    n = 1 << k
    last = counts[-1]
    if name == "zero":
        assert all(c["both_identity"] == n // 2 for c in counts)
    elif name == "const":
        for s, c in enumerate(counts):
            assert c["doubling"] == n >> (s + 1) and c["both_identity"] == n // 2 - (n >> (s + 1)), s
    elif name == "nyquist":
        assert last["cancel"] == 1 and last["both_identity"] == n // 2 - 1
        assert all(c["doubling"] == n >> (s + 1) for s, c in enumerate(counts[:-1]))
    elif name in ("tone3", "tone_last"):
        assert all(c["doubling"] + c["cancel"] >= 1 for c in counts)
        assert all(c["plain"] == 0 for c in counts)  # every other butterfly has an identity operand
    elif name == "delta0":
        assert all(c["b_identity"] == 1 << s and c["both_identity"] == n // 2 - (1 << s) for s, c in enumerate(counts))
    elif name == "delta_half":
        assert counts[0]["a_identity"] == 1 and counts[0]["both_identity"] == n // 2 - 1
        assert all(c["b_identity"] == 1 << s for s, c in enumerate(counts) if s)
    elif name == "even_only":
        assert last["b_identity"] == n // 2
    elif name == "odd_only":
        assert last["a_identity"] == n // 2
    elif name in ("planted", "planted2"):
        # both operands are non-zero in the doubling and cancel classes by their definition.  The first variant has no zero anywhere.
        # In the second, every exceptional butterfly of layer k - 2 leaves one identity behind (a + t or a - t), which is the b operand
        # of one butterfly of the last layer -- none of them a planted one
        dbl, can = _planted_counts(n)
        hit, left = {k - 1: (dbl, can)}, 0
        if name == "planted2":
            hit[k - 2] = _planted_counts(n // 2, inner=True)
            left = sum(hit[k - 2])
        for s, c in enumerate(counts):
            assert (c["doubling"], c["cancel"]) == hit.get(s, (0, 0)), s
            assert (c["b_identity"], c["a_identity"], c["both_identity"]) == (left if s == k - 1 else 0, 0, 0), s
        assert last["plain"] == n // 2 - dbl - can - left
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name,k", G2L_CASES + BIG_CASES)
def test_inputs_hit_their_butterfly_classes_omega_inv(oracle, name, k):
    w = gu.omega_of(oracle, k, True)
    _check_classes(name, k, gu.simulate(gu.scalars(name, 1 << k, w), w, k)[1])


@pytest.mark.parametrize("name,k", FFT_CASES)
def test_inputs_hit_their_butterfly_classes_omega(oracle, name, k):
    w = gu.omega_of(oracle, k, False)
    _check_classes(name, k, gu.simulate(gu.scalars(name, 1 << k, w), w, k)[1])


def test_tone_and_planted_class_counts_at_k6(oracle):
    """the per-layer (doubling, cancel) counts of two inputs, written out: a tone cancels in the first layers (all 32 butterflies of
    layer 0) and doubles in the later ones; planted has its four hits in the last layer and nowhere else"""
    w = gu.omega_of(oracle, 6, True)
    _, counts = gu.simulate(gu.scalars("tone3", 64, w), w, 6)
    assert [(c["doubling"], c["cancel"]) for c in counts] == [(0, 32), (0, 16), (8, 0), (4, 0), (2, 0), (1, 0)]
    _, counts = gu.simulate(gu.scalars("planted", 64, w), w, 6)
    assert [(c["doubling"], c["cancel"]) for c in counts] == [(0, 0)] * 5 + [(2, 2)]


def test_jacobian_rescaling_keeps_the_points(oracle):
    """jacobian_z: (x z^2, y z^3, z) with z != 1 is the same group element, the identity is (0, 1, 0)"""
    c = gu.case("delta0", 2, False)
    pts = np.concatenate([c.expected, np.zeros((1, 8), dtype=np.uint64)])
    jz = gu.to_jacobian(oracle, pts, random.Random(5))
    one = oracle.fe_from_int(oracle.FQ, 1)
    assert all(not np.array_equal(p[8:], one) for p in jz[:-1])
    assert not jz[-1, :4].any() and np.array_equal(jz[-1, 4:8], one) and not jz[-1, 8:].any()
    assert np.array_equal(np.stack([oracle.g1_to_affine(p) for p in jz]), pts)
    assert np.array_equal(np.stack([oracle.g1_to_affine(p) for p in gu.to_jacobian(oracle, pts)]), pts)


# --------------------------------------------------------------------------------- CPU: the oracle against the definition
def _affine_all(oracle, jac):
    return np.stack([oracle.g1_to_affine(p) for p in jac])


@pytest.mark.parametrize("name,k", _cases(ORACLE_KS, gu.NAMES))
def test_oracle_g_to_lagrange_equals_the_definition(oracle, name, k):
    """pins the oracle's own handling of doublings, cancellations and identities in its butterflies"""
    c = gu.case(name, k, True)
    assert np.array_equal(oracle.g_to_lagrange(c.points, k, num_threads=2), c.expected)


@pytest.mark.parametrize("name,k", _cases(ORACLE_KS, gu.NAMES))
def test_oracle_best_fft_g1_equals_the_definition(oracle, name, k):
    c = gu.case(name, k, False)
    w = oracle.domain_new(2, k)[0].fe("omega")
    for rng in (None, random.Random(k)):  # z = 1, and every point in its own Jacobian scaling
        got = oracle.best_fft_g1(gu.to_jacobian(oracle, c.points, rng), w, k, num_threads=2)
        assert np.array_equal(_affine_all(oracle, got), c.expected), rng is not None


# ---------------------------------------------------------------------------------------------------------------- GPU
def _g2l_all_modes(h2, points, k, wants, modes=MODES):
    L = h2.lib()
    try:
        for mode in modes:
            L.h2hip_debug_set_g2l_quad(ctypes.c_int(mode))
            got = h2.g_to_lagrange(points, k)
            for what, want in wants:
                assert np.array_equal(got, want), (mode, what, np.flatnonzero((got != want).any(axis=1))[:8])
    finally:
        L.h2hip_debug_set_g2l_quad(ctypes.c_int(1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", G2L_CASES)
def test_gpu_g_to_lagrange_exceptional_butterflies(h2, oracle, name, k):
    """every named input through the lazy quad path, the normalised quad path and the one-lane path, against the definition and the
    oracle"""
    h2.init()
    c = gu.case(name, k, True)
    _g2l_all_modes(h2, c.points, k, [("definition", c.expected), ("oracle", oracle.g_to_lagrange(c.points, k, num_threads=16))])


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", BIG_CASES)
def test_gpu_g_to_lagrange_beyond_the_quad_range(h2, oracle, name, k):
    """k > 14: ecfft_layer_kernel with a normalisation after every layer and ec_scale_kernel, whatever the hook says; the expectation is
    a closed form (two distinct points at most), so neither the oracle's FFT nor 2^15 scalar multiplications run"""
    h2.init()
    c = gu.case(name, k, True)
    _g2l_all_modes(h2, c.points, k, [("definition", c.expected)], modes=(1,))


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", FFT_CASES)
def test_gpu_best_fft_g1_exceptional_butterflies(h2, oracle, name, k):
    """best_fft::<G1> with the forward root: z = 1 inputs and inputs in random Jacobian scalings, the default path and one lane"""
    h2.init()
    L = h2.lib()
    c = gu.case(name, k, False)
    w = oracle.domain_new(2, k)[0].fe("omega")
    one = oracle.fe_from_int(oracle.FQ, 1)
    plain = gu.to_jacobian(oracle, c.points)
    want_oracle = _affine_all(oracle, oracle.best_fft_g1(plain, w, k, num_threads=16))
    assert np.array_equal(want_oracle, c.expected)
    try:
        for mode in (1, 0):
            L.h2hip_debug_set_g2l_quad(ctypes.c_int(mode))
            for a in (plain, gu.to_jacobian(oracle, c.points, random.Random(100 + k))):
                got = a.copy()
                h2.best_fft_g1(got, w, k)
                assert np.array_equal(_affine_all(oracle, got), c.expected), mode
                assert all((p[8:] == one).all() or not p[8:].any() for p in got)  # z = 1, or the identity's z = 0
    finally:
        L.h2hip_debug_set_g2l_quad(ctypes.c_int(1))
