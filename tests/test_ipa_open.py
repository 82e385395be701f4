"""GPU: the inner-product-argument commitment scheme (halo2-pse_amd/ipa.py) end to end, against the integer restatement of
tests/ipa_util.py.
  * a whole opening: at k = 1, 2, 6 the proof bytes -- S, every L_j and R_j, c, f -- equal the restatement's for the same transcript
    and seed, at k = 10 and 13 the restatement's with the oracle's group sums; from a resident polynomial and from a host one; a zero
    polynomial, a zero blind and x_3 = 0 included;
  * the multiopen round trip of poly/multiopen_test.rs::test_roundtrip_ipa at K = 4 and K = 10: both strategies accept, a flipped
    byte in any field of the proof and a wrong claimed evaluation are rejected, and at K = 4 the proof bytes and the final MSM agree
    with the restatement on integers;
  * params: new(k) is the stated derivation, write / read, downsize, commit and commit_lagrange with their blinds."""
import io

import numpy as np
import pytest

import ipa_util as iu

pytestmark = pytest.mark.gpu
R = iu.R
SEED = bytes(range(7, 39))


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


_setups = {}


def _setup(ipa, oracle, k):
    """(engine params, the same generators as integers) from the oracle's deterministic points: deriving 2^13 generators is the params
    test's matter, not the opening's"""
    if k not in _setups:
        pts = oracle.gen_points(0x1A1000 + k, (1 << k) + 2, num_threads=1)
        params = ipa.ParamsIPA.from_parts(pts[:1 << k], pts[1 << k], pts[(1 << k) + 1])
        ints = iu.g1_ints(pts)
        _setups[k] = (params, iu.Params(k, ints[:1 << k], ints[1 << k], ints[(1 << k) + 1]))
    return _setups[k]


CASES = {
    "k1": (1, "plain"), "k2": (2, "plain"), "k2 zero polynomial": (2, "zero poly"), "k2 zero blind, x_3 = 0": (2, "zero blind"),
    "k6": (6, "plain"), "k10": (10, "plain"), "k13": (13, "plain"),
}
_restated = {}


def _inputs(k, variant):
    rng = iu.Rng(SEED, stream_id=1000 + k)
    poly = rng.draw(1 << k)
    blind, x_3 = rng.draw(2)
    if variant == "zero poly":
        poly = [0] * (1 << k)
    if variant == "zero blind":
        blind, x_3 = 0, 0
    return poly, blind, x_3


def _restated_proof(T, oracle, params_int, case):
    """the restatement's proof bytes, computed once per case and shared by the resident and the host run"""
    if case not in _restated:
        k, variant = CASES[case]
        poly, blind, x_3 = _inputs(k, variant)
        grp = iu.Ints() if k <= 6 else iu.OracleSums(oracle)
        w = T.Blake2bWrite()
        w.common_scalar(x_3)  # any common input: both sides absorb the same
        iu.create_proof(grp, params_int, iu.Rng(SEED), w, poly, blind, x_3)
        _restated[case] = w.finalize()
    return _restated[case]


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("case", list(CASES))
def test_opening_bytes_equal_the_restatement(h2, ipa, T, oracle, case, resident):
    k, variant = CASES[case]
    params, params_int = _setup(ipa, oracle, k)
    poly, blind, x_3 = _inputs(k, variant)
    want = _restated_proof(T, oracle, params_int, case)
    limbs = iu.fr_limbs(poly)
    w = T.Blake2bWrite()
    w.common_scalar(x_3)
    d_poly = _dev(limbs) if resident else None
    ipa.create_proof(params, h2.FrRng(SEED), w, d_poly if resident else limbs, blind, x_3, resident=resident)
    got = w.finalize()
    assert len(got) == 32 * (1 + 2 * k + 2)
    assert got == want, [i // 32 for i in range(0, len(got), 32) if got[i:i + 32] != want[i:i + 32]]
    if resident:
        assert np.array_equal(h2.to_numpy_u64(d_poly), limbs)  # the caller's polynomial is left as it was
    # ... and the engine's verifier accepts it, against the commitment the engine computes
    r = T.Blake2bRead(got)
    r.common_scalar(x_3)
    msm = params.empty_msm()
    msm.append_term(1, params.commit(limbs, blind))
    guard = ipa.verify_proof(params, msm, r, x_3, iu.eval_poly(poly, x_3))
    g = guard.compute_g()
    assert guard.use_challenges().check()
    if k <= 6 and resident:  # the other way to close a guard: the caller names G = <s, g>, the MSM needs no 2^k scalars
        r = T.Blake2bRead(got)
        r.common_scalar(x_3)
        msm = params.empty_msm()
        msm.append_term(1, params.commit(limbs, blind))
        msm_g, (acc_g, acc_u) = ipa.verify_proof(params, msm, r, x_3, iu.eval_poly(poly, x_3)).use_g(g)
        assert msm_g.check() and acc_g == g and len(acc_u) == k
        assert g == iu.Ints().msm(iu.compute_s(acc_u, 1), params_int.g)


# ------------------------------------------------------------------ multiopen
def _roundtrip_inputs(k):
    n = 1 << k
    return [[10 + i for i in range(n)], [100 + i for i in range(n)], [100 + i for i in range(n)]]


def _prove(h2, ipa, T, params, k, seed=SEED):
    """poly/multiopen_test.rs:228-307"""
    polys = _roundtrip_inputs(k)
    rng = h2.FrRng(seed)
    blind = h2.fr_to_int(rng.draw(1)[0])
    d_polys = [_dev(iu.fr_limbs(p)) for p in polys]
    w = T.Blake2bWrite()
    for c in params.commit_many(d_polys, [blind] * 3):
        w.write_point(c)
    x, y = w.squeeze_challenge(), w.squeeze_challenge()
    for p, at in zip(polys, (x, x, y)):
        w.write_scalar(iu.eval_poly(p, at))
    ipa.ProverIPA(params).create_proof(rng, w, [(x, d_polys[0], blind), (x, d_polys[1], blind), (y, d_polys[2], blind)])
    return w.finalize()


def _read_claims(T, proof):
    r = T.Blake2bRead(proof)
    a, b, c = r.read_point(), r.read_point(), r.read_point()
    x, y = r.squeeze_challenge(), r.squeeze_challenge()
    avx, bvx, cvy = r.read_scalar(), r.read_scalar(), r.read_scalar()
    return r, (a, b, c), (x, y), (avx, bvx, cvy)


def _verify(ipa, T, params, proof, strategy, should_fail=False):
    """poly/multiopen_test.rs:170-226; -> the strategy's verdict"""
    r, (a, b, c), (x, y), (avx, bvx, cvy) = _read_claims(T, proof)
    a, b, c = ipa.Commitment(a), ipa.Commitment(b), ipa.Commitment(c)  # b and c are equal points and two commitments
    queries = [(a, x, avx), (b, x, avx if should_fail else bvx), (c, y, cvy)]
    return strategy.process(lambda msm: ipa.VerifierIPA(params).verify_proof(r, queries, msm))


def _accepts(ipa, T, params, proof, should_fail=False):
    try:
        _verify(ipa, T, params, proof, ipa.SingleStrategy(params), should_fail)
        return True
    except (ipa.IPAError, T.TranscriptError):
        return False


_proofs = {}


def _proof(h2, ipa, T, oracle, k):
    if k not in _proofs:
        params, _ = _setup(ipa, oracle, k)
        _proofs[k] = _prove(h2, ipa, T, params, k)
    return _proofs[k]


@pytest.mark.parametrize("k", [4, 10])
def test_multiopen_roundtrip(h2, ipa, T, oracle, k):
    params, _ = _setup(ipa, oracle, k)
    proof = _proof(h2, ipa, T, oracle, k)
    # a, b, c | avx, bvx, cvy | q_prime | u_0, u_1 | S | (L_j, R_j) x k | c, f
    assert len(proof) == 32 * (6 + 1 + 2 + 1 + 2 * k + 2)
    assert _accepts(ipa, T, params, proof)
    assert not _accepts(ipa, T, params, proof, should_fail=True)  # a wrong claimed evaluation
    acc = ipa.AccumulatorStrategy(params, h2.FrRng(bytes(32)))
    acc = _verify(ipa, T, params, proof, acc)
    acc = _verify(ipa, T, params, _prove(h2, ipa, T, params, k, seed=bytes(range(100, 132))), acc)
    assert acc.finalize()
    bad = ipa.AccumulatorStrategy(params, h2.FrRng(bytes(32)))
    bad = _verify(ipa, T, params, proof, bad)
    bad = _verify(ipa, T, params, proof, bad, should_fail=True)
    assert not bad.finalize()


@pytest.mark.parametrize("k", [4, 10])
def test_multiopen_rejects_a_flipped_byte_in_every_field(h2, ipa, T, oracle, k):
    params, _ = _setup(ipa, oracle, k)
    proof = _proof(h2, ipa, T, oracle, k)
    base = 6
    fields = {"q_prime": base, "u_0": base + 1, "u_1": base + 2, "S": base + 3, "L_1": base + 4 + 2, "R_%d" % (k - 1): base + 4 + 2 * (k - 1) + 1,
              "c": base + 4 + 2 * k, "f": base + 4 + 2 * k + 1}
    assert max(fields.values()) == len(proof) // 32 - 1
    for name, field in fields.items():
        bad = bytearray(proof)
        bad[32 * field + 5] ^= 0x10
        assert not _accepts(ipa, T, params, bytes(bad)), name


def test_multiopen_on_integers_agrees_at_k_4(h2, ipa, T, oracle):
    k = 4
    params, params_int = _setup(ipa, oracle, k)
    proof = _proof(h2, ipa, T, oracle, k)
    grp, polys = iu.Ints(), _roundtrip_inputs(k)
    # the prover restated: the same bytes
    rng = iu.Rng(SEED)
    blind = rng.draw(1)[0]
    w = T.Blake2bWrite()
    for p in polys:
        w.write_point(params_int.commit(grp, p, blind))
    x, y = w.squeeze_challenge(), w.squeeze_challenge()
    for p, at in zip(polys, (x, x, y)):
        w.write_scalar(iu.eval_poly(p, at))
    iu.multiopen_create_proof(grp, params_int, rng, w, [(0, x, 0), (1, x, 0), (2, y, 0)], polys, [blind] * 3)
    assert w.finalize() == proof
    # the verifier restated: the final MSM is the identity for the valid claims, and the same point as the engine's for wrong ones
    for should_fail in (False, True):
        r, commitments, (x, y), (avx, bvx, cvy) = _read_claims(T, proof)
        queries = [(0, x, avx), (1, x, avx if should_fail else bvx), (2, y, cvy)]
        want = iu.multiopen_verify_proof(params_int, r, queries, commitments, iu.MSM(params_int)).eval(grp)
        r, (a, b, c), _, _ = _read_claims(T, proof)
        a, b, c = ipa.Commitment(a), ipa.Commitment(b), ipa.Commitment(c)
        guard = ipa.VerifierIPA(params).verify_proof(r, [(a, x, avx), (b, x, avx if should_fail else bvx), (c, y, cvy)], params.empty_msm())
        with pytest.raises(TypeError):
            ipa.VerifierIPA(params).verify_proof(r, [(a.point, x, avx)], params.empty_msm())
        got = guard.use_challenges().eval()
        assert got == want and (want is None) == (not should_fail)


# ------------------------------------------------------------------ params
def test_params_new_is_the_stated_derivation(h2, ipa):
    k = 6
    with ipa.ParamsIPA.new(k) as params:
        want = [iu.derive(iu.g_message(i))[0] for i in range(1 << k)]
        assert iu.g1_ints(params.g) == want
        assert (params.w, params.u) == (iu.derive(bytes([1]))[0], iu.derive(bytes([2]))[0])
        assert np.array_equal(params.g_lagrange, h2.g_to_lagrange(params.g, k))
        # write then read
        buf = io.BytesIO()
        params.write(buf)
        data = buf.getvalue()
        assert len(data) == 4 + 32 * (2 * (1 << k) + 2) and data[:4] == (k).to_bytes(4, "little")
        back = ipa.ParamsIPA.read(io.BytesIO(data))
        for name in ("g", "g_lagrange", "w_limbs", "u_limbs"):
            assert np.array_equal(getattr(back, name), getattr(params, name)), name
        with pytest.raises(h2.H2HipError):
            ipa.ParamsIPA.read(io.BytesIO(data[:-1]))
        # commit with its blind, against integers; commit_lagrange of the evaluations is the same commitment
        rng = iu.Rng(SEED, 5)
        f = rng.draw(1 << k)
        r = rng.draw(1)[0]
        grp = iu.Ints()
        want_c = grp.add(grp.msm(f, want), grp.mul(params.w, r))
        assert params.commit(iu.fr_limbs(f), r) == want_c
        assert params.commit(iu.fr_limbs(f), 0) == grp.msm(f, want) != want_c
        omega = pow(iu.OMEGA_28, 1 << (28 - k), R)
        evals = iu.fr_limbs(f)
        h2.best_fft(evals, iu.fr_limbs([omega])[0], k)
        assert params.commit_lagrange(evals, r) == want_c
        assert params.commit_many([_dev(iu.fr_limbs(f)), _dev(evals)], [r, 0])[0] == want_c
        assert params.commit_lagrange_many([evals, evals], [r, 0]) == [want_c, grp.msm(f, want)]
        # downsize
        back.downsize(4)
        assert back.k == 4 and back.n == 16 and np.array_equal(back.g, params.g[:16])
        assert np.array_equal(back.g_lagrange, h2.g_to_lagrange(params.g[:16], 4))
        f4 = f[:16]
        omega4 = pow(iu.OMEGA_28, 1 << 24, R)
        want4 = grp.add(grp.msm(f4, want[:16]), grp.mul(params.w, r))
        assert back.commit(iu.fr_limbs(f4), r) == want4
        evals4 = iu.fr_limbs(f4)
        h2.best_fft(evals4, iu.fr_limbs([omega4])[0], 4)
        assert back.commit_lagrange(evals4, r) == want4
        back.close()
