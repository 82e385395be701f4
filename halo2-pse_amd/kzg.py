"""The closing of a KZG check: poly/kzg/msm.rs:120-170 (DualMSM) and poly/kzg/strategy.rs (GuardKZG, SingleStrategy,
AccumulatorStrategy) over the library's host pairing (include/halo2hip_pairing.h), and that header's calls on Python values.

A check is e(left, s_g2) e(right, -g2) = 1: two Miller loops under one squaring chain and one final exponentiation, on the calling
thread (csrc/pairing_host.h; DESIGN.md section 5, "Pairing").  left and right are the verifier's MSM term lists (verifier.MSM), kept
unevaluated so that a batch of proofs folds into one check: AccumulatorStrategy scales what it holds by a random factor before every
proof, as the reference does, and its factor comes from the caller's FrRng instead of OsRng, as ipa.AccumulatorStrategy's does.
DualMSM.check evaluates each side in the library: up to 4096 terms with h2hip_g1_linear_combinations_bn254 on the host, above that with
the engine's MSM (h2hip_msm_bn254 over host pointers), which needs the GPU.  No call here uses the setup secret."""
import numpy as np

from . import (FQ_MODULUS, G2_GENERATOR, H2HipError, _check, _p, _u64, best_multiexp, fr_from_int, fr_to_int, g1_from_int, g1_linear_combinations,
               g1_to_affine, g1_to_int, lib)
from .transcript import FR_MODULUS
from .verifier import MSM, VerifyError

Q = FQ_MODULUS
LINCOMB_TERMS = 4096  # the most terms one h2hip_g1_linear_combinations_bn254 call takes
MAX_PAIRS = 65536     # the most pairs one pairing call takes

G2_IDENTITY = bytes(128)


# ------------------------------------------------------------------ include/halo2hip_pairing.h on Python values
def _g1_array(points):
    """(n, 8) uint64 from an array of limbs or a list of affine integer pairs (None: the identity)"""
    if isinstance(points, np.ndarray):
        return _u64(points).reshape(-1, 8)
    return np.stack([g1_from_int(p) for p in points]) if len(points) else np.zeros((0, 8), dtype=np.uint64)


def _g2_array(points):
    """(n, 16) uint64 from an array of limbs or a list of 128-byte raw points"""
    if isinstance(points, np.ndarray):
        return _u64(points).reshape(-1, 16)
    raws = [bytes(p) for p in points]
    if any(len(r) != 128 for r in raws):
        raise ValueError("a raw G2 point is 128 bytes")
    return np.frombuffer(b"".join(raws), dtype=np.uint64).reshape(-1, 16).copy()


def _pairs(g1_points, g2_points):
    g1, g2 = _g1_array(g1_points), _g2_array(g2_points)
    if g1.shape[0] != g2.shape[0]:
        raise ValueError("pairing: %d G1 points for %d G2 points" % (g1.shape[0], g2.shape[0]))
    n = g1.shape[0]
    return (_p(g1) if n else None), (_p(g2) if n else None), n, (g1, g2)


def pairing(g1_points, g2_points):
    """prod_i e(P_i, Q_i) as (48,) uint64: twelve Montgomery Fq a_0, b_0, ..., a_5, b_5, the value sum_i (a_i + b_i u) w^i.  Host code
    on the calling thread: no GPU, no engine lock.  H2HipError for a point off its curve or a G2 point outside the subgroup."""
    p1, p2, n, _keep = _pairs(g1_points, g2_points)
    out = np.zeros(48, dtype=np.uint64)
    _check(lib().h2hip_pairing_bn254(p1, p2, n, _p(out)), "h2hip_pairing_bn254")
    return out


def pairing_check(g1_points, g2_points):
    """prod_i e(P_i, Q_i) = 1"""
    import ctypes
    p1, p2, n, _keep = _pairs(g1_points, g2_points)
    ok = ctypes.c_int(-1)
    _check(lib().h2hip_pairing_check_bn254(p1, p2, n, ctypes.byref(ok)), "h2hip_pairing_check_bn254")
    return ok.value == 1


def g2_mul(raw, scalar):
    """[scalar] Q for a raw G2 point (128 bytes) and an integer (or 4 Montgomery limbs) -> 128 raw bytes"""
    q = _g2_array([raw])
    s = fr_from_int(scalar) if isinstance(scalar, int) else _u64(scalar).reshape(4)
    out = np.zeros(16, dtype=np.uint64)
    _check(lib().h2hip_g2_mul_bn254(_p(q), _p(s), _p(out)), "h2hip_g2_mul_bn254")
    return out.tobytes()


def g2_check(raw):
    """(on the twist, in the subgroup of order r) of a raw G2 point"""
    import ctypes
    q = _g2_array([raw])
    on, sub = ctypes.c_int(-1), ctypes.c_int(-1)
    _check(lib().h2hip_g2_check_bn254(_p(q), ctypes.byref(on), ctypes.byref(sub)), "h2hip_g2_check_bn254")
    return on.value == 1, sub.value == 1


def g2_neg(raw):
    """-Q: the y coordinate negated (on Montgomery limbs as on the values); the identity stays"""
    raw = bytes(raw)
    c = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(4)]
    return b"".join(v.to_bytes(32, "little") for v in (c[0], c[1], -c[2] % Q, -c[3] % Q))


# ------------------------------------------------------------------ poly/kzg/msm.rs:120-170
def eval_msm(msm, lincomb_terms=LINCOMB_TERMS):
    """MSMKZG::eval (msm.rs:62-67) in the library, as an affine integer pair: a term list of up to lincomb_terms terms is one
    h2hip_g1_linear_combinations_bn254 call on the host, a longer one an engine MSM over host pointers (plain form)"""
    terms = [(s % FR_MODULUS, p) for s, p in msm.terms if p is not None]
    if not terms:
        return None
    if len(terms) <= min(lincomb_terms, LINCOMB_TERMS):
        return g1_linear_combinations(None, [[s for s, _ in terms]], [p for _, p in terms])[0]
    coeffs = np.stack([fr_from_int(s) for s, _ in terms])
    bases = np.stack([g1_from_int(p) for _, p in terms])
    return g1_to_int(g1_to_affine(best_multiexp(coeffs, bases)))


class DualMSM:
    """msm.rs:120-170: the two channels of a KZG check, e(left, s_g2) = e(right, g2)"""

    def __init__(self, params):                                                        # :130-136
        self.params, self.left, self.right = params, MSM(), MSM()

    def scale(self, e):                                                                # :139-142
        self.left.scale(e)
        self.right.scale(e)

    def add_msm(self, other):                                                          # :145-148
        self.left.add_msm(other.left)
        self.right.add_msm(other.right)

    def check(self, lincomb_terms=LINCOMB_TERMS):                                      # :151-169
        """e(left, s_g2) e(right, -g2) = 1 through h2hip_pairing_check_bn254.  lincomb_terms: the term count above which a side is
        evaluated by the engine's MSM instead of on the host.  Params without G2 points (both are the identity in a file this package
        wrote before setup filled them) cannot decide anything: a pairing with the identity is 1, so that is an error, not a verdict."""
        g2, s_g2 = bytes(self.params.g2), bytes(self.params.s_g2)
        if g2 == G2_IDENTITY or s_g2 == G2_IDENTITY:
            raise VerifyError("the params carry no G2 points: g2 or s_g2 is the identity")
        left, right = eval_msm(self.left, lincomb_terms), eval_msm(self.right, lincomb_terms)
        return pairing_check([left, right], [s_g2, g2_neg(g2)])


# ------------------------------------------------------------------ poly/kzg/strategy.rs
class GuardKZG:
    """strategy.rs:26-47: what a multiopen verifier hands back -- the accumulator with its proof's terms added"""

    def __init__(self, msm_accumulator):
        self.msm_accumulator = msm_accumulator


class SingleStrategy:
    """strategy.rs:69-82, :122-159"""

    def __init__(self, params):
        self.msm = DualMSM(params)

    def process(self, f):
        """f: DualMSM -> GuardKZG; VerifyError (Error::ConstraintSystemFailure, :149-153) unless the pairing check holds"""
        if not f(self.msm).msm_accumulator.check():
            raise VerifyError("ConstraintSystemFailure: the pairing check does not hold")


class AccumulatorStrategy:
    """strategy.rs:49-67, :84-120; the random scale factor comes from the caller's rng (an FrRng), not from OsRng"""

    def __init__(self, params, rng):
        self.msm_accumulator, self.rng = DualMSM(params), rng

    def process(self, f):
        self.msm_accumulator.scale(fr_to_int(self.rng.draw(1)[0]))                     # :108
        self.msm_accumulator = f(self.msm_accumulator).msm_accumulator                 # :111-114
        return self

    def finalize(self, lincomb_terms=LINCOMB_TERMS):                                   # :117-119
        return self.msm_accumulator.check(lincomb_terms)


STRATEGIES = (SingleStrategy, AccumulatorStrategy)

__all__ = ["AccumulatorStrategy", "DualMSM", "G2_GENERATOR", "GuardKZG", "H2HipError", "SingleStrategy", "eval_msm", "g2_check", "g2_mul",
           "g2_neg", "pairing", "pairing_check"]
