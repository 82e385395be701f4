"""Inputs of the curve-point FFT built in the exponent (test infrastructure only).

Every input is P_i = [a_i]G with G = (1, 2) and a_i a Python integer mod r, so the transform of the points is the transform of the
scalars: out_j = [s * sum_i a_i w^(i j)]G (s = 1/n for g_to_lagrange, 1 for best_fft::<G1>).  The named inputs below are chosen so
that the butterflies a + t, a - t (t = [w^i] b) of the reference's iterative network (arithmetic.rs:186-230) are exceptional cases of
the group law -- t == a (a doubling), t == -a (the identity), an operand the identity -- which random points never are.  simulate()
runs that network on the scalars and counts, per layer, the butterflies of each class; the tests assert those counts, so an edit that
turns a construction into plain data fails on the CPU.  Expected outputs come from the definition (the O(n^2) sum, or a closed form),
never from a butterfly network."""
import functools
import random

import numpy as np

from product_util import R_MOD, from_mont, to_mont

CLASSES = ("doubling", "cancel", "b_identity", "a_identity", "both_identity", "plain")
C = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R_MOD  # the scalar of the structured inputs
DEFINITION_MAX_K = 9                                                             # the O(n^2) sum up to here
CLOSED_FORM = ("zero", "const", "nyquist", "delta0", "delta_half")              # expectations written down directly, any n


# ------------------------------------------------------------------------------------------------------------- scalars
def omega_of(oracle, k, inverse):
    """the transform's root as an integer: the domain's omega_inv (g_to_lagrange) or omega (best_fft::<G1>); 1 at k = 0"""
    if k == 0:
        return 1
    d, _ = oracle.domain_new(2, k)
    return from_mont(d.fe("omega_inv" if inverse else "omega"))[0]


def dft(a, w):
    """the definition: out_j = sum_i a_i w^(i j), O(n^2)"""
    n = len(a)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % R_MOD
    return [sum(a[i] * pw[i * j % n] for i in range(n)) % R_MOD for j in range(n)]


def idft(a, w):
    n_inv = pow(len(a), -1, R_MOD)
    return [v * n_inv % R_MOD for v in dft(a, pow(w, -1, R_MOD))]


def planted_spots(n, inner=False):
    """butterfly indices of the last layer that are made exceptional, alternately a doubling (+1) and a cancellation (-1).  inner: the
    spots of the half-size planting inside the second variant, doublings at 1 and 2 and cancellations at the others -- an exceptional
    butterfly leaves one identity behind (a + t at a cancellation, a - t at a doubling: B[i] or B[i + n / 2] below), and with these
    signs none of them lands on a spot of the full size, where nothing could be planted on it"""
    spots = sorted({1, 2, n // 4, n // 2 - 1})
    assert n >= 8 and all(0 < i < n // 2 for i in spots)
    if inner:
        return [(i, 1 if i <= 2 else -1) for i in spots]
    return [(i, 1 if j % 2 == 0 else -1) for j, i in enumerate(spots)]


def planted(n, w, rng, depth=1, inner=False):
    """dense scalars, none zero, whose last layer has t == a at some butterflies and t == -a at others: the odd half is random (depth 2:
    itself planted at half size, so that the layer before the last is hit too), B its half-size DFT; the even half's spectrum A is random
    but for A[i] = +-w^i B[i] at the spots; the even half is the inverse DFT of A"""
    h = n // 2
    w2 = w * w % R_MOD
    odd = planted(h, w2, rng, 1, inner=True) if depth == 2 else [rng.randrange(1, R_MOD) for _ in range(h)]
    B = dft(odd, w2)
    A = [rng.randrange(1, R_MOD) for _ in range(h)]
    for i, sign in planted_spots(n, inner):
        assert B[i]
        A[i] = sign * pow(w, i, R_MOD) * B[i] % R_MOD
    even = idft(A, w2)
    a = [0] * n
    a[0::2], a[1::2] = even, odd
    return a


def exists(name, n):
    """which named inputs exist at n = 2^k points (k >= 1)"""
    if name in ("zero", "const", "nyquist", "delta0", "delta_half", "even_only", "odd_only", "tone_last"):
        return n >= 2
    if name in ("tone3", "planted"):
        return n >= 8
    if name == "planted2":
        return n >= 16
    raise KeyError(name)


NAMES = ("zero", "const", "nyquist", "tone3", "tone_last", "delta0", "delta_half", "even_only", "odd_only", "planted", "planted2")


def scalars(name, n, w, seed=0):
    """the named input's a_i (integers mod r) for the transform with root w"""
    assert exists(name, n)
    rng = random.Random("%s/%d/%d" % (name, n, seed))
    if name == "zero":
        return [0] * n
    if name == "const":
        return [C] * n
    if name == "nyquist":
        return [C if i % 2 == 0 else R_MOD - C for i in range(n)]
    if name in ("tone3", "tone_last"):
        j = 3 if name == "tone3" else n - 1
        wj = pow(w, -j, R_MOD)
        return [C * pow(wj, i, R_MOD) % R_MOD for i in range(n)]
    if name in ("delta0", "delta_half"):
        a = [0] * n
        a[0 if name == "delta0" else n // 2] = C
        return a
    if name in ("even_only", "odd_only"):
        par = 0 if name == "even_only" else 1
        return [rng.randrange(1, R_MOD) if i % 2 == par else 0 for i in range(n)]
    if name == "planted":
        return planted(n, w, rng, 1)
    if name == "planted2":
        return planted(n, w, rng, 2)
    raise KeyError(name)


def expected_scalars(name, n, w, a, scale):
    """scale * DFT(a) from the definition; the closed-form inputs are written down directly (O(n) integer work, two distinct values)"""
    if name == "zero":
        out = [0] * n
    elif name == "const":
        out = [n * C % R_MOD] + [0] * (n - 1)
    elif name == "nyquist":
        out = [0] * n
        out[n // 2] = n * C % R_MOD
    elif name == "delta0":
        out = [C] * n
    elif name == "delta_half":
        out = [C if j % 2 == 0 else R_MOD - C for j in range(n)]  # C w^(j n / 2), w^(n / 2) = -1
    else:
        assert n <= 1 << DEFINITION_MAX_K
        out = dft(a, w)
    return [v * scale % R_MOD for v in out]


def simulate(a, w, k):
    """the reference's iterative butterflies on the scalars: the bit reversal (arithmetic.rs:186-191), then layers s = 0 .. k - 1 with
    t = w^(i n / 2^(s + 1)) b; (a, b) <- (a + t, a - t).  Returns (output, per layer a dict class -> number of butterflies): doubling
    is a == t != 0, cancel a == -t != 0, the identity classes say which operand is zero, plain is everything else"""
    n = 1 << k
    assert len(a) == n
    x = list(a)
    for i in range(n):
        r = int(format(i, "0%db" % k)[::-1], 2) if k else 0
        if i < r:
            x[i], x[r] = x[r], x[i]
    counts = []
    for s in range(k):
        half = 1 << s
        step = pow(w, n >> (s + 1), R_MOD)
        cnt = dict.fromkeys(CLASSES, 0)
        for base in range(0, n, 2 * half):
            tw = 1
            for i in range(half):
                ia, ib = base + i, base + i + half
                u, v = x[ia], x[ib]
                t = tw * v % R_MOD
                if u == 0 and v == 0:
                    cls = "both_identity"
                elif v == 0:
                    cls = "b_identity"
                elif u == 0:
                    cls = "a_identity"
                elif u == t:
                    cls = "doubling"
                elif (u + t) % R_MOD == 0:
                    cls = "cancel"
                else:
                    cls = "plain"
                cnt[cls] += 1
                x[ia], x[ib] = (u + t) % R_MOD, (u - t) % R_MOD
                tw = tw * step % R_MOD
        counts.append(cnt)
    return x, counts


# -------------------------------------------------------------------------------------------------------------- points
_minted = {}


def mint(oracle, vals):
    """[v]G as (len, 8) affine points in the reference's layout, the identity (0, 0); each distinct scalar is multiplied once"""
    gen = np.zeros(8, dtype=np.uint64)
    gen[:4], gen[4:] = oracle.fe_from_int(oracle.FQ, 1), oracle.fe_from_int(oracle.FQ, 2)
    out = np.zeros((len(vals), 8), dtype=np.uint64)
    for i, v in enumerate(vals):
        if v == 0:
            continue
        if v not in _minted:
            _minted[v] = oracle.g1_to_affine(oracle.g1_mul(gen, to_mont([v])[0]))
        out[i] = _minted[v]
    return out


def to_jacobian(oracle, affine, rng=None):
    """(n, 8) affine -> (n, 12) Jacobian: z = 1, or with rng (x z^2, y z^3, z) for a random z != 1 per point; the identity is (0, 1, 0)"""
    q = oracle.int_from_limbs(oracle.constant(oracle.FQ, 2))
    one = oracle.fe_from_int(oracle.FQ, 1)
    out = np.zeros((affine.shape[0], 12), dtype=np.uint64)
    for i, p in enumerate(affine):
        if not p.any():
            out[i, 4:8] = one
            continue
        if rng is None:
            out[i, :8], out[i, 8:] = p, one
            continue
        x, y = (oracle.int_from_limbs(c) for c in oracle.fe_to_canonical(oracle.FQ, p.reshape(2, 4)))
        z = rng.randrange(2, q)
        for j, v in enumerate((x * z * z, y * z * z * z, z)):
            out[i, 4 * j:4 * j + 4] = oracle.fe_from_int(oracle.FQ, v % q)
    return out


class Case:
    """one named input of one transform: the scalars, the affine input points and the affine expected output"""

    def __init__(self, oracle, name, k, inverse):
        self.name, self.k, self.n, self.inverse = name, k, 1 << k, inverse
        self.w = omega_of(oracle, k, inverse)
        self.scalars = scalars(name, self.n, self.w)
        scale = pow(self.n, -1, R_MOD) if inverse else 1  # g_to_lagrange divides by n (arithmetic.rs:286-290), best_fft does not
        self.points = mint(oracle, self.scalars)
        self.expected = mint(oracle, expected_scalars(name, self.n, self.w, self.scalars, scale))
        self.points.setflags(write=False)
        self.expected.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(name, k, inverse):
    from oracle import oracle
    oracle.build()
    oracle.lib()
    return Case(oracle, name, k, inverse)


def case(name, k, inverse=True):
    """computed once per (name, k, transform) and shared, read-only, by every test that needs it"""
    return _case(name, k, bool(inverse))
