"""The inner-product-argument commitment scheme of halo2_proofs/src/poly/ipa/ at C = bn256::G1Affine, over the engine
(include/halo2hip_ipa.h): params, commit, open, the multiopen prover and verifier, both verification strategies.

  ParamsIPA                    ipa/commitment.rs:29-232 -- new / from_parts / read / write / downsize / commit / commit_lagrange
  create_proof                 ipa/commitment/prover.rs:29-153
  verify_proof, compute_b      ipa/commitment/verifier.rs:22-106
  MSMIPA                       ipa/msm.rs
  GuardIPA, SingleStrategy, AccumulatorStrategy, compute_s    ipa/strategy.rs
  construct_intermediate_sets  ipa/multiopen.rs:66-176
  ProverIPA, VerifierIPA       ipa/multiopen/{prover,verifier}.rs

Scalars are Python integers in [0, r), points affine integer pairs (None: the identity), the transcript is transcript.py's Blake2bWrite /
Blake2bRead.  Everything of 2^k elements lives in HBM as torch CUDA tensors of Montgomery limbs: the engine folds, collapses, reduces
and multiplies; the transcript and the draws stay here, and the handful of group operations between the MSMs -- the + [r] W of a
commitment, the [value z] U + [rand] W of a round, the other terms of MSMIPA.eval -- are one host call of the library each
(h2hip_g1_linear_combinations_bn254, include/halo2hip_g1.h: dependent chains of a few hundred group operations, faster on a host core
than on GPU lanes).  A round of an opening is one engine call (round_device, include/halo2hip_ipa_round.h: the fold and the collapse by
the challenge before it, the inner products and both MSMs from one run of the MSM pipeline, one wait); set_round_call(False) runs the
separate calls instead, with the same draws, transcript and bytes.  There is no CPU fallback for the rest: without a GPU the calls raise
H2HipError.

Draw order (one FrRng): ProverIPA.create_proof draws q_prime_blind first; create_proof then draws the 2^k coefficients of s_poly in HBM
(element i = the next block i), s_poly_blind, and per round l_j_randomness then r_j_randomness.

Generators.  ParamsIPA::new takes its points from halo2curves' hash_to_curve("Halo2-Parameters"), whose source this project does not
have; the derivation is therefore stated here (and in DESIGN.md section 2) and pinned by tests/golden: for a message M and a counter
ctr = 0, 1, 2, ..., h = BLAKE2b-512(person = b"Halo2-Parameters", data = M || ctr as 4 bytes LE); x = (h[0:48] as a little-endian
integer) mod q, sign = h[63] & 1; the candidate is the 32-byte compressed encoding of (x, sign) and the first counter whose candidate
g1_decompress reads as a point of the curve (x != 0 and x^3 + 3 a square; x = 0 is the identity's encoding with the sign clear and invalid
with it set, and neither is a generator) gives the point.  The messages are the reference's:
[0] || i as 4 bytes LE for g[i], [1] for w, [2] for u.  BN254 G1 has cofactor 1, so every accepted point is in the group."""
import hashlib

import numpy as np

from . import (FQ_MODULUS, FR_MODULUS, H2HIP_EENCODING, H2HipError, _check, _dptr, _fe, _p, _stream, _u64, bases_pin_device,
               bases_unpin_device, device_count, eval_polynomials_device, fr_from_int, fr_to_int, g1_linear_combinations,
               g1_to_bytes, g1_to_int, g_to_lagrange, lib, msm_batch_device, msm_device, poly_combine_device, to_numpy_u64)
from .transcript import TranscriptError, point_from_bytes
from .verifier import _affine, _interpolate_eval, _jac, _jac_add, _jac_double

R, Q = FR_MODULUS, FQ_MODULUS
GENERATOR_PERSONAL = b"Halo2-Parameters"
_LINCOMB_TERMS = 4096  # the most terms one h2hip_g1_linear_combinations_bn254 call takes


class IPAError(ValueError):
    """the reference's Error::{OpeningError, SamplingError, ConstraintSystemFailure}, or an unwrap it would panic on (a zero challenge)"""


# ------------------------------------------------------------------ group sums on integers
def _point_sum(terms):
    """sum of [s] P over (s, P) pairs of integers: one doubling chain shared by all terms (Straus).  For the places that hold integers
    only; where an engine sum is one of the terms, g1_linear_combinations (include/halo2hip_g1.h) adds it in the library."""
    live = [(s % R, _jac(p)) for s, p in terms if p is not None and s % R]
    acc = (0, 1, 0)
    for bit in range(max((s.bit_length() for s, _ in live), default=0) - 1, -1, -1):
        acc = _jac_double(acc)
        for s, p in live:
            if (s >> bit) & 1:
                acc = _jac_add(acc, p)
    return _affine(acc)


# ------------------------------------------------------------------ generators
def generator_candidate(message, ctr):
    """the 32-byte compressed candidate of (message, ctr)"""
    h = hashlib.blake2b(bytes(message) + int(ctr).to_bytes(4, "little"), digest_size=64, person=GENERATOR_PERSONAL).digest()
    x = int.from_bytes(h[:48], "little") % Q
    return (x | (h[63] & 1) << 255).to_bytes(32, "little")


def generator_message(i):
    """g[i]'s message (ipa/commitment.rs:177-178)"""
    return bytes([0]) + int(i).to_bytes(4, "little")


W_MESSAGE, U_MESSAGE = bytes([1]), bytes([2])  # :200-201


def hash_to_curve_int(message):
    """the derivation on integers: (point, the counter that gave it)"""
    ctr = 0
    while True:
        data = generator_candidate(message, ctr)
        if int.from_bytes(data, "little") & ((1 << 255) - 1):  # x != 0
            try:
                return point_from_bytes(data), ctr
            except TranscriptError:
                pass
        ctr += 1


def _derive_generators(messages):
    """the same for many messages, on the engine: hash on the host, decompress every candidate in one call; the call writes a rejected
    element as zero bytes, and only those are redone with the next counter (about half survive each wave)"""
    L = lib()
    n = len(messages)
    out = np.zeros((n, 8), dtype=np.uint64)
    todo, ctr = list(range(n)), 0
    while todo:
        data = np.frombuffer(b"".join(generator_candidate(messages[i], ctr) for i in todo), dtype=np.uint8).reshape(-1, 32).copy()
        pts, invalid = np.zeros((len(todo), 8), dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        rc = L.h2hip_g1_decompress_bn254(_p(data), len(todo), _p(pts), _p(invalid))
        if rc != H2HIP_EENCODING:
            _check(rc, "h2hip_g1_decompress_bn254")
        ok = pts.any(axis=1)  # x = 0 comes back as zeros too: the identity (sign clear) or invalid (sign set)
        for j in np.nonzero(ok)[0]:
            out[todo[j]] = pts[j]
        todo = [todo[j] for j in np.nonzero(~ok)[0]]
        ctr += 1
    return out


# ------------------------------------------------------------------ the round calls (include/halo2hip_ipa.h)
def _fr(x):
    return fr_from_int(x) if isinstance(x, int) else _fe(x)


def collapse(g, u):
    """parallel_generator_collapse on a host array: (2 half, 8) uint64 -> the (half, 8) collapsed points"""
    g = _u64(g, 8).copy()
    half = g.shape[0] // 2
    _check(lib().h2hip_ipa_collapse_bn254(_p(g), half, _p(_fr(u))), "h2hip_ipa_collapse_bn254")
    return g[:half].copy()


def collapse_device(d_g, half, u):
    """the same in place on a torch CUDA tensor of 2 half x 64 B; queued on the current stream"""
    _check(lib().h2hip_ipa_collapse_bn254_device(_dptr(d_g), int(half), _p(_fr(u)), _stream()), "h2hip_ipa_collapse_bn254_device")


def _need_gpu(what):
    if device_count() < 1:
        raise H2HipError("%s: no GPU (no CPU fallback exists)" % what)


def powers_device(x, n, out=None):
    """x^i, i < n, as a torch CUDA tensor (n, 4) int64"""
    if out is None:
        _need_gpu("powers_device")
        import torch
        out = torch.empty((int(n), 4), dtype=torch.int64, device="cuda")
    _check(lib().h2hip_ipa_powers_bn254_fr_device(_p(_fr(x)), int(n), _dptr(out), _stream()), "h2hip_ipa_powers_bn254_fr_device")
    return out


def inner_products_device(d_p, d_b, half):
    """(<p[half:], b[:half]>, <p[:half], b[half:]>) as integers; waits for the stream"""
    values = np.zeros((2, 4), dtype=np.uint64)
    _check(lib().h2hip_ipa_inner_products_bn254_fr_device(_dptr(d_p), _dptr(d_b), int(half), _p(values), _stream()),
           "h2hip_ipa_inner_products_bn254_fr_device")
    return fr_to_int(values[0]), fr_to_int(values[1])


def fold_device(d_p, d_b, half, u_inv, u, next_values=False):
    """p[i] += u_inv p[half + i], b[i] += u b[half + i] in place; next_values: also the next round's inner products (then it waits)"""
    values = np.zeros((2, 4), dtype=np.uint64) if next_values else None
    _check(lib().h2hip_ipa_fold_bn254_fr_device(_dptr(d_p), _dptr(d_b), int(half), _p(_fr(u_inv)), _p(_fr(u)),
                                                _p(values) if next_values else None, _stream()), "h2hip_ipa_fold_bn254_fr_device")
    return (fr_to_int(values[0]), fr_to_int(values[1])) if next_values else None


def round_msms_device(d_p, d_g, half):
    """(L, R) = (<p[half:2 half], g[:half]>, <p[:half], g[half:2 half]>) as Jacobian limbs (12,), the form msm_device returns: both MSMs of
    a round from one engine call (one run of the MSM pipeline up to round_msms_fused_max_half()); waits for the stream"""
    out = np.zeros((2, 12), dtype=np.uint64)
    _check(lib().h2hip_ipa_round_msms_bn254_device(_dptr(d_p), _dptr(d_g), int(half), _p(out[0]), _p(out[1]), _stream()),
           "h2hip_ipa_round_msms_bn254_device")
    return out[0], out[1]


def round_msms_fused_max_half():
    """the largest half whose two MSMs run as one two-set run under the settings in force"""
    return int(lib().h2hip_ipa_round_msms_fused_max_half())


def round_device(d_p, d_b, d_g, half, u=None, u_inv=None):
    """one round after the challenge u of the round before it (None: the first round): fold p, b and collapse g at 2 half by u, then
    L, R and the inner products at half -> (L, R, (value_l, value_r)); one engine call, one wait"""
    out, values = np.zeros((2, 12), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    _check(lib().h2hip_ipa_round_bn254_device(_dptr(d_p), _dptr(d_b), _dptr(d_g), int(half), None if u is None else _p(_fr(u)),
                                              None if u_inv is None else _p(_fr(u_inv)), _p(out[0]), _p(out[1]), _p(values), _stream()),
           "h2hip_ipa_round_bn254_device")
    return out[0], out[1], (fr_to_int(values[0]), fr_to_int(values[1]))


def set_round_call(on=True):
    """tuning: create_proof runs one round call per round (the default) or the separate calls; returns the value in force"""
    _check(lib().h2hip_ipa_set_round_call(1 if on else 0), "h2hip_ipa_set_round_call")
    return bool(lib().h2hip_ipa_get_round_call())


def _challenges(u):
    return np.ascontiguousarray(np.stack([_fr(x) for x in u]), dtype=np.uint64) if len(u) else np.zeros((1, 4), dtype=np.uint64)


def compute_s(u, init):
    """compute_s (ipa/strategy.rs:161-176) -> (2^k, 4) uint64"""
    k = len(u)
    out = np.zeros((1 << k if 1 <= k <= 28 else 1, 4), dtype=np.uint64)
    _check(lib().h2hip_ipa_compute_s_bn254_fr(_p(_challenges(u)), k, _p(_fr(init)), _p(out)), "h2hip_ipa_compute_s_bn254_fr")
    return out


def compute_s_device(u, init, out=None):
    """the same left in HBM: a torch CUDA tensor (2^k, 4) int64"""
    k = len(u)
    if out is None:
        _need_gpu("compute_s_device")
        import torch
        out = torch.empty((1 << k if 1 <= k <= 28 else 1, 4), dtype=torch.int64, device="cuda")
    _check(lib().h2hip_ipa_compute_s_bn254_fr_device(_p(_challenges(u)), k, _p(_fr(init)), _dptr(out), _stream()),
           "h2hip_ipa_compute_s_bn254_fr_device")
    return out


def set_collapse_quad(max_half=0):
    """tuning: halves up to max_half take one quad of lanes per point (0 = the default); returns the value in force"""
    _check(lib().h2hip_ipa_set_collapse_quad(int(max_half)), "h2hip_ipa_set_collapse_quad")
    return int(lib().h2hip_ipa_get_collapse_quad())


def compute_b(x, u):
    """prod_{i < k} (1 + u_{k - 1 - i} x^(2^i))  (ipa/commitment/verifier.rs:98-106)"""
    tmp, cur = 1, x % R
    for u_j in reversed(u):
        tmp = tmp * (1 + u_j * cur) % R
        cur = cur * cur % R
    return tmp


# ------------------------------------------------------------------ params
def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _read_elem(d_t, i=0):
    """element i of a device column as an integer (32 bytes cross)"""
    return fr_to_int(to_numpy_u64(d_t[i:i + 1])[0])


class ParamsIPA:
    """ipa/commitment.rs:29-36.  g and g_lagrange are uploaded once and pinned by their device pointers (the fixed-base window tables of
    the commits and of the verifier's MSM) for the life of the object or of the `with` block."""

    def __init__(self, k, g, g_lagrange, w, u):
        self.k, self.n = int(k), 1 << int(k)
        self.g, self.g_lagrange = _u64(g, 8).copy(), _u64(g_lagrange, 8).copy()
        assert self.g.shape[0] == self.n and self.g_lagrange.shape[0] == self.n
        self.w_limbs, self.u_limbs = _u64(w).reshape(8).copy(), _u64(u).reshape(8).copy()
        self.w, self.u = g1_to_int(self.w_limbs), g1_to_int(self.u_limbs)
        self._d = {}

    @classmethod
    def new(cls, k):
        """ParamsProver::new (:158-211) with the derivation this module states"""
        assert 0 <= k < 32  # :161
        n = 1 << k
        pts = _derive_generators([generator_message(i) for i in range(n)] + [W_MESSAGE, U_MESSAGE])
        return cls.from_parts(pts[:n], pts[n], pts[n + 1])

    @classmethod
    def from_parts(cls, g, w, u):
        """the caller's generators: g (2^k, 8), w and u (8,) Montgomery limbs"""
        g = _u64(g, 8)
        k = g.shape[0].bit_length() - 1
        assert g.shape[0] == 1 << k
        return cls(k, g, g_to_lagrange(g, k), w, u)

    # ---- read / write (:110-146): k as u32 LE, then g, g_lagrange, w, u compressed
    @classmethod
    def read(cls, reader):
        kb = reader.read(4)
        if len(kb) != 4:
            raise H2HipError("ParamsIPA::read: short read")
        k = int.from_bytes(kb, "little")
        if k >= 32:
            raise H2HipError("ParamsIPA::read: k = %d" % k)
        n = 1 << k
        buf = reader.read((2 * n + 2) * 32)
        if len(buf) != (2 * n + 2) * 32:
            raise H2HipError("ParamsIPA::read: short read")
        from . import g1_from_bytes
        pts = g1_from_bytes(buf)  # H2HipEncodingError for an invalid point, where the reference returns io::Error
        return cls(k, pts[:n], pts[n:2 * n], pts[2 * n], pts[2 * n + 1])

    def write(self, writer):
        writer.write(int(self.k).to_bytes(4, "little"))
        writer.write(g1_to_bytes(np.concatenate([self.g, self.g_lagrange, self.w_limbs[None], self.u_limbs[None]])).tobytes())

    def downsize(self, k):
        """:76-83"""
        assert k <= self.k
        self.close()
        self.k, self.n = int(k), 1 << int(k)
        self.g = self.g[:self.n].copy()
        self.g_lagrange = g_to_lagrange(self.g, self.k)

    # ---- the device copies
    def _resident(self, name):
        d = self._d.get(name)
        if d is None:
            _need_gpu("ParamsIPA")
            d = _to_device(getattr(self, name))
            bases_pin_device(d, self.n)
            self._d[name] = d
        return d

    def d_g(self):
        return self._resident("g")

    def d_g_lagrange(self):
        return self._resident("g_lagrange")

    def close(self):
        for d in self._d.values():
            try:
                bases_unpin_device(d)
            except H2HipError:
                pass
        self._d = {}

    def __enter__(self):
        self.d_g()
        self.d_g_lagrange()
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- commit (:216-227) and commit_lagrange (:92-107): the MSM over g (or g_lagrange) plus [r] W -- the blind is real here
    def _commit(self, d_bases, polys, blinds):
        d_polys = [p if hasattr(p, "data_ptr") else _to_device(_u64(p, 4)) for p in polys]
        for d in d_polys:
            assert d.numel() * d.element_size() == 32 * self.n  # the reference zips poly and bases: equal lengths
        sums = msm_batch_device(d_polys, d_bases, self.n) if len(d_polys) > 1 else [msm_device(d_polys[0], d_bases, self.n)]
        return g1_linear_combinations(sums, [[r] for r in blinds], [self.w])                                # + [r] W, one shared inversion

    def commit(self, poly, r):
        """poly: (n, 4) uint64 or a torch CUDA tensor of n x 32 B; r an integer -> the commitment as an affine integer pair"""
        return self._commit(self.d_g(), [poly], [r])[0]

    def commit_lagrange(self, poly, r):
        return self._commit(self.d_g_lagrange(), [poly], [r])[0]

    def commit_many(self, polys, blinds):
        """one batched MSM over the pinned g, every blind honoured"""
        return self._commit(self.d_g(), list(polys), list(blinds))

    def commit_lagrange_many(self, polys, blinds):
        return self._commit(self.d_g_lagrange(), list(polys), list(blinds))

    def empty_msm(self):
        return MSMIPA(self)


# ------------------------------------------------------------------ the opening
def create_proof(params, rng, transcript, p_poly, p_blind, x_3, resident=True):
    """commitment::create_proof (ipa/commitment/prover.rs:29-153).  rng: an FrRng; transcript: a Blake2bWrite that has seen the common
    inputs; p_poly: with resident=True a torch CUDA tensor of 2^k x 32 B, left unchanged; with resident=False a (2^k, 4) uint64 array,
    uploaded once.  After that upload no array of 2^k elements crosses PCIe: every round moves two Jacobian sums, two values and a
    challenge."""
    import torch
    n, k = params.n, params.k
    d_p = p_poly if resident else _to_device(_u64(p_poly, 4))
    assert d_p.numel() * d_p.element_size() == 32 * n                                   # :43
    d_g = params.d_g()
    d_s_raw = rng.draw_device(n)                                                       # :47-50, blocks [c, c + n)
    s_at_x3, p_at_x3 = [fr_to_int(e) for e in eval_polynomials_device([d_s_raw, d_p], [0, 1], [fr_from_int(x_3)] * 2)]   # :52
    d_s = torch.empty_like(d_s_raw)
    poly_combine_device([d_s_raw], [fr_from_int(1)], d_s, sub=[fr_from_int(s_at_x3)])  # :54
    s_blind = fr_to_int(rng.draw(1)[0])                                                # :56
    transcript.write_point(params.commit(d_s, s_blind))                                # :59-60
    xi = transcript.squeeze_challenge()                                                # :65
    z = transcript.squeeze_challenge()                                                 # :69
    # p' = xi s + p with its value at x_3 taken from the constant term; s has a root at x_3, so that value is p(x_3)  (:73-75)
    d_pp = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    poly_combine_device([d_s, d_p], [fr_from_int(xi), fr_from_int(1)], d_pp, sub=[fr_from_int(p_at_x3)])
    f = (s_blind * xi + p_blind) % R                                                   # :76-80
    d_b = powers_device(x_3, n)                                                        # :88-95
    d_gp = d_g.clone()                                                                 # :99
    # one engine call per round (round_device: the fold and the collapse by the challenge before it, the inner products and both MSMs,
    # one wait), or -- set_round_call(False) -- the separate calls; the draws, the transcript and the bytes are the same
    round_call = bool(lib().h2hip_ipa_get_round_call())
    values = inner_products_device(d_pp, d_b, n // 2) if k and not round_call else None
    u_j = u_j_inv = None
    for j in range(k):                                                                 # :102
        half = 1 << (k - j - 1)
        if round_call:
            l_g, r_g, values = round_device(d_pp, d_b, d_gp, half, u_j, u_j_inv)       # :129-137 of round j - 1, then :109-112
        else:
            l_g = msm_device(d_pp[half:], d_gp, half)                                  # :109
            r_g = msm_device(d_pp, d_gp[half:], half)                                  # :110
        value_l, value_r = values                                                      # :111-112
        l_rand, r_rand = [fr_to_int(e) for e in rng.draw(2)]                           # :113-114
        l_j, r_j = g1_linear_combinations([l_g, r_g], [[value_l * z, l_rand], [value_r * z, r_rand]], [params.u, params.w])   # :115-116
        transcript.write_point(l_j)                                                    # :121
        transcript.write_point(r_j)
        u_j = transcript.squeeze_challenge()                                           # :124
        if u_j == 0:
            raise IPAError("create_proof: the challenge u_%d is zero" % j)             # :125 unwraps
        u_j_inv = pow(u_j, -1, R)
        if not round_call:
            values = fold_device(d_pp, d_b, half, u_j_inv, u_j, next_values=half >= 2)  # :129-134
            collapse_device(d_gp, half, u_j)                                           # :137
        f = (f + l_rand * u_j_inv + r_rand * u_j) % R                                  # :141-142
    if round_call and k:
        fold_device(d_pp, d_b, 1, u_j_inv, u_j)   # the last fold, for c; the last collapse (:137) gives a g' nothing reads: dropped
    c = _read_elem(d_pp)                                                               # :147
    transcript.write_scalar(c)                                                         # :149-150
    transcript.write_scalar(f)


class MSMIPA:
    """ipa/msm.rs: scalars for g, w, u and a map x -> (scalar, y) of other terms, merged where two points share x.  g_scalars stays in
    HBM: a column of 2^k scalars plus a constant for row 0 that is added when the column is evaluated."""

    def __init__(self, params):
        self.params = params
        self.d_g_scalars, self.g_const, self.has_g = None, 0, False
        self.w_scalar = self.u_scalar = None
        self.other = {}

    def append_term(self, scalar, point):                                              # :71-91
        if point is None:
            return
        x, y = point
        if x in self.other:
            s, our_y = self.other[x]
            if our_y == y:
                self.other[x] = ((s + scalar) % R, our_y)
            else:
                assert our_y == (-y) % Q
                self.other[x] = ((s - scalar) % R, our_y)
        else:
            self.other[x] = (scalar % R, y)

    def add_msm(self, other):                                                          # :94-120
        for x, (scalar, y) in sorted(other.other.items()):
            self.append_term(scalar, (x, y))
        if other.has_g:
            self.has_g = True
            self.g_const = (self.g_const + other.g_const) % R
            if other.d_g_scalars is not None:
                self.add_to_g_scalars(other.d_g_scalars)
        if other.w_scalar is not None:
            self.add_to_w_scalar(other.w_scalar)
        if other.u_scalar is not None:
            self.add_to_u_scalar(other.u_scalar)

    def scale(self, factor):                                                           # :122-135
        if self.d_g_scalars is not None:
            import torch
            out = torch.empty_like(self.d_g_scalars)
            poly_combine_device([self.d_g_scalars], [fr_from_int(factor)], out)
            self.d_g_scalars = out
        self.g_const = self.g_const * factor % R
        self.other = {x: (s * factor % R, y) for x, (s, y) in self.other.items()}
        if self.w_scalar is not None:
            self.w_scalar = self.w_scalar * factor % R
        if self.u_scalar is not None:
            self.u_scalar = self.u_scalar * factor % R

    def add_constant_term(self, constant):                                             # :190-198
        self.has_g = True
        self.g_const = (self.g_const + constant) % R

    def add_to_g_scalars(self, d_scalars):                                             # :202-211; a torch CUDA tensor of 2^k x 32 B
        assert d_scalars.numel() * d_scalars.element_size() == 32 * self.params.n
        self.has_g = True
        if self.d_g_scalars is None:
            self.d_g_scalars = d_scalars.clone()
        else:
            poly_combine_device([d_scalars], [fr_from_int(1)], self.d_g_scalars, accumulate=True)

    def add_to_w_scalar(self, scalar):                                                 # :213-215
        self.w_scalar = scalar % R if self.w_scalar is None else (self.w_scalar + scalar) % R

    def add_to_u_scalar(self, scalar):                                                 # :218-220
        self.u_scalar = scalar % R if self.u_scalar is None else (self.u_scalar + scalar) % R

    def g_column(self):
        """g_scalars as one device column, the constant in row 0"""
        import torch
        n = self.params.n
        d = torch.zeros((n, 4), dtype=torch.int64, device="cuda") if self.d_g_scalars is None else self.d_g_scalars.clone()
        if self.g_const:
            d[0:1] = _to_device(fr_from_int((_read_elem(d) + self.g_const) % R).reshape(1, 4))
        return d

    def eval(self):                                                                    # :141-174, as an affine integer pair
        terms = [(s, (x, y)) for x, (s, y) in self.other.items()]
        if self.w_scalar is not None:
            terms.append((self.w_scalar, self.params.w))
        if self.u_scalar is not None:
            terms.append((self.u_scalar, self.params.u))
        addend = [msm_device(self.g_column(), self.params.d_g(), self.params.n)] if self.has_g else None
        # one call (m = 1); only an accumulator over very many proofs has more terms than a call takes
        chunks = [terms[at:at + _LINCOMB_TERMS] for at in range(0, len(terms), _LINCOMB_TERMS)] or [[]]
        sums = [g1_linear_combinations(addend if i == 0 else None, [[s for s, _ in part]], [p for _, p in part])[0]
                for i, part in enumerate(chunks)]
        return sums[0] if len(sums) == 1 else _point_sum([(1, p) for p in sums])

    def check(self):                                                                   # :137-139
        return self.eval() is None


class GuardIPA:
    """ipa/strategy.rs:24-77"""

    def __init__(self, msm, neg_c, u):
        self.msm, self.neg_c, self.u = msm, neg_c, list(u)

    def use_challenges(self):                                                          # :51-56
        self.msm.add_to_g_scalars(compute_s_device(self.u, self.neg_c))
        return self.msm

    def use_g(self, g):                                                                # :60-69 -> (msm, (g, u))
        self.msm.append_term(self.neg_c, g)
        return self.msm, (g, list(self.u))

    def compute_g(self):                                                               # :72-76
        params = self.msm.params
        return g1_linear_combinations([msm_device(compute_s_device(self.u, 1), params.d_g(), params.n)], [[]], [])[0]


def verify_proof(params, msm, transcript, x, v):
    """commitment::verify_proof (ipa/commitment/verifier.rs:22-95): transcript a Blake2bRead, msm an MSMIPA that evaluates to the
    commitment being opened -> GuardIPA.  IPAError where the reference returns Error::OpeningError / SamplingError."""
    k = params.k
    try:
        msm.add_constant_term(-v % R)                                                  # :32
        s_commitment = transcript.read_point()                                         # :33
        xi = transcript.squeeze_challenge()                                            # :34
        msm.append_term(xi, s_commitment)                                              # :35
        z = transcript.squeeze_challenge()                                             # :37
        rounds = []
        for _ in range(k):                                                             # :40-49
            l = transcript.read_point()
            r = transcript.read_point()
            rounds.append((l, r, transcript.squeeze_challenge()))
        u = []
        for l, r, u_j in rounds:                                                       # :51-66 (batch_invert leaves a zero as it is)
            msm.append_term(pow(u_j, -1, R) if u_j else 0, l)
            msm.append_term(u_j, r)
            u.append(u_j)
        c = transcript.read_scalar()                                                   # :79
        f = transcript.read_scalar()                                                   # :81
    except TranscriptError as e:
        raise IPAError("verify_proof: %s" % e)
    neg_c = -c % R
    b = compute_b(x, u)                                                                # :82
    msm.add_to_u_scalar(neg_c * b % R * z % R)                                         # :84
    msm.add_to_w_scalar(-f % R)                                                        # :85
    return GuardIPA(msm, neg_c, u)


class SingleStrategy:
    """ipa/strategy.rs:121-158"""

    def __init__(self, params):
        self.msm = MSMIPA(params)

    def process(self, f):
        """f: MSMIPA -> GuardIPA; IPAError (Error::ConstraintSystemFailure) unless the proof verifies"""
        if not f(self.msm).use_challenges().check():
            raise IPAError("the opening does not verify")


class AccumulatorStrategy:
    """ipa/strategy.rs:81-117; the random scale factor comes from the caller's rng (an FrRng), not from OsRng"""

    def __init__(self, params, rng):
        self.msm, self.rng = MSMIPA(params), rng

    def process(self, f):
        self.msm.scale(fr_to_int(self.rng.draw(1)[0]))                                 # :101
        self.msm = f(self.msm).use_challenges()                                        # :102-106
        return self

    def finalize(self):                                                                # :114-116
        return self.msm.check()


# ------------------------------------------------------------------ multiopen
def construct_intermediate_sets(queries):
    """ipa/multiopen.rs:66-176 over queries (commitment id, point, eval) -> (commitment_map, point_sets): commitment_map lists, per
    commitment in order of first appearance, (id, set_index, point_indices, evals); point_sets[set_index] are the set's points.  The
    reference's BTreeMaps decide only this: a point's index is its order of first appearance (the map is keyed by the point, the index
    is the map's size at insertion), a point-index set is ordered ascending, a set's index is the order of first appearance among the
    commitments, and evals follow the set's ascending point indices."""
    queries = list(queries)
    point_index, commitment_map = {}, []
    for cid, point, _ in queries:                                                      # :80-96
        idx = point_index.setdefault(point, len(point_index))
        for entry in commitment_map:
            if entry[0] == cid:
                entry[1].append(idx)
                break
        else:
            commitment_map.append((cid, [idx]))
    inverse = {idx: point for point, idx in point_index.items()}                       # :99-102
    set_index, commitment_sets = {}, {}
    for cid, indices in commitment_map:                                                # :109-121
        s = tuple(sorted(set(indices)))
        commitment_sets[cid] = s
        set_index.setdefault(s, len(set_index))
    out = {cid: [set_index[commitment_sets[cid]], indices, [0] * len(indices)] for cid, indices in commitment_map}   # :124-127
    for cid, point, ev in queries:                                                     # :130-164
        out[cid][2][commitment_sets[cid].index(point_index[point])] = ev
    point_sets = [None] * len(set_index)                                               # :167-173
    for s, idx in set_index.items():
        point_sets[idx] = [inverse[i] for i in s]
    return [(cid, out[cid][0], out[cid][1], out[cid][2]) for cid, _ in commitment_map], point_sets


class ProverIPA:
    """ipa/multiopen/prover.rs"""

    def __init__(self, params):
        self.params = params

    def create_proof(self, rng, transcript, queries):
        """queries: ProverQuery as (point, poly, blind) in the caller's order; poly: a torch CUDA tensor of 2^k x 32 B (coefficient
        form), blind an integer.  Two queries name the same commitment when they hold the same tensor (its device address), as the
        reference compares the polynomial's address (poly/query.rs:38-42).  The q polynomials, q' and the final polynomial are built in
        HBM with poly_combine (scale-and-add, then its roots for kate_division), the u_i with eval_polynomials."""
        import torch
        n = self.params.n
        one = fr_from_int(1)
        x_1 = transcript.squeeze_challenge()                                           # :42
        x_2 = transcript.squeeze_challenge()                                           # :43
        polys, blinds, keys, tagged = [], [], {}, []
        for point, poly, blind in queries:
            cid = keys.setdefault(poly.data_ptr(), len(polys))
            if cid == len(polys):
                polys.append(poly)
                blinds.append(blind % R)
            tagged.append((cid, point % R, 0))
        poly_map, point_sets = construct_intermediate_sets(tagged)                     # :45
        q_polys, q_blinds = [None] * len(point_sets), [0] * len(point_sets)
        for cid, set_idx, _, _ in poly_map:                                            # :53-71
            if q_polys[set_idx] is None:
                q_polys[set_idx] = polys[cid].clone()
            else:
                out = torch.empty_like(q_polys[set_idx])
                poly_combine_device([q_polys[set_idx], polys[cid]], [fr_from_int(x_1), one], out)
                q_polys[set_idx] = out
            q_blinds[set_idx] = (q_blinds[set_idx] * x_1 + blinds[cid]) % R
        d_q_prime = None
        for points, poly in zip(point_sets, q_polys):                                  # :74-95
            d_quot = torch.empty((n, 4), dtype=torch.int64, device="cuda")             # kate_division by each point, resized to n
            poly_combine_device([poly], [one], d_quot, roots=[fr_from_int(p) for p in points])
            if d_q_prime is None:
                d_q_prime = d_quot
            else:
                out = torch.empty_like(d_quot)
                poly_combine_device([d_q_prime, d_quot], [fr_from_int(x_2), one], out)
                d_q_prime = out
        q_prime_blind = fr_to_int(rng.draw(1)[0])                                      # :97
        transcript.write_point(self.params.commit(d_q_prime, q_prime_blind))           # :98-100
        x_3 = transcript.squeeze_challenge()                                           # :102
        evals = eval_polynomials_device(q_polys, list(range(len(q_polys))), [fr_from_int(x_3)] * len(q_polys))
        for e in evals:                                                                # :106-108
            transcript.write_scalar(fr_to_int(e))
        x_4 = transcript.squeeze_challenge()                                           # :110
        d_p, p_blind = d_q_prime, q_prime_blind
        for poly, blind in zip(q_polys, q_blinds):                                     # :112-120
            out = torch.empty_like(d_p)
            poly_combine_device([d_p, poly], [fr_from_int(x_4), one], out)
            d_p, p_blind = out, (p_blind * x_4 + blind) % R
        create_proof(self.params, rng, transcript, d_p, p_blind, x_3)                  # :122


class Commitment:
    """a verifier's handle on one commitment (CommitmentReference, poly/query.rs:104-122): `point` an affine integer pair, or `msm` an
    MSMIPA.  The reference tells commitments apart by address, not by value -- two polynomials with equal coefficients and blinds have
    equal commitments and are still two openings --, so the handle is the identity: queries that hold the same handle name the same
    commitment, two handles never do, whatever they hold."""

    def __init__(self, point=None, msm=None):
        assert point is None or msm is None  # neither: the identity point, which is a commitment too
        self.point, self.msm = point, msm


class VerifierIPA:
    """ipa/multiopen/verifier.rs"""

    def __init__(self, params):
        self.params = params

    def verify_proof(self, transcript, queries, msm):
        """queries: VerifierQuery as (commitment, point, eval), commitment a Commitment handle (anything else is a TypeError: a bare
        point has no identity to compare) -> GuardIPA"""
        x_1 = transcript.squeeze_challenge()                                           # :50
        x_2 = transcript.squeeze_challenge()                                           # :54
        commitments, keys, tagged = [], {}, []
        for commitment, point, ev in queries:
            if not isinstance(commitment, Commitment):
                raise TypeError("VerifierIPA.verify_proof: a query's commitment is an ipa.Commitment handle")
            cid = keys.setdefault(commitment, len(commitments))  # hashed by identity; the dict keeps the handle alive
            if cid == len(commitments):
                commitments.append(commitment)
            tagged.append((cid, point % R, ev % R))
        commitment_map, point_sets = construct_intermediate_sets(tagged)               # :56
        q_commitments = [self.params.empty_msm() for _ in point_sets]                  # :60
        q_eval_sets = [[0] * len(ps) for ps in point_sets]                             # :64-67
        for cid, set_idx, _, evals in commitment_map:                                  # :69-95
            q_commitments[set_idx].scale(x_1)
            if commitments[cid].msm is not None:
                q_commitments[set_idx].add_msm(commitments[cid].msm)
            else:
                q_commitments[set_idx].append_term(1, commitments[cid].point)
            for i, ev in enumerate(evals[:len(q_eval_sets[set_idx])]):
                q_eval_sets[set_idx][i] = (q_eval_sets[set_idx][i] * x_1 + ev) % R
        try:
            q_prime = transcript.read_point()                                          # :99
            x_3 = transcript.squeeze_challenge()                                       # :103
            u = [transcript.read_scalar() for _ in q_eval_sets]                        # :107-110
        except TranscriptError as e:
            raise IPAError("verify_proof: %s" % e)                                     # Error::SamplingError
        msm_eval = 0
        for points, evals, proof_eval in zip(point_sets, q_eval_sets, u):              # :114-128
            ev = (proof_eval - _interpolate_eval(points, evals, x_3)) % R
            for p in points:
                if (x_3 - p) % R == 0:
                    raise IPAError("verify_proof: x_3 is one of the points")           # :124 unwraps
                ev = ev * pow(x_3 - p, -1, R) % R
            msm_eval = (msm_eval * x_2 + ev) % R
        x_4 = transcript.squeeze_challenge()                                           # :132
        msm.append_term(1, q_prime)                                                    # :135
        v = msm_eval
        for q_commitment, q_eval in zip(q_commitments, u):                             # :136-143
            msm.scale(x_4)
            msm.add_msm(q_commitment)
            v = (v * x_4 + q_eval) % R
        return verify_proof(self.params, msm, transcript, x_3, v)                      # :146
