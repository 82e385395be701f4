"""GPU: KZG proofs accepted or refused by the package itself -- verify_proof with a kzg strategy closes e(left, s_g2) = e(right, g2)
with the library's host pairing, where the other proof tests close it with the setup secret (proof_util.pairing_holds).  The two must
never disagree: for every member of the three families (proof_util's SYSTEM, systems_util, systems_args_util), both KZG schemes, the
good proof and every tampering the families define are judged both ways.  Then: a wrong s_g2 refuses everything; AccumulatorStrategy
folds three proofs of two systems into one check and one tampered proof turns it, after which the proofs are judged one at a time;
params written after setup carry real G2 points through all three SerdeFormats; ParamsKZG.check_structure names what is wrong with a
params object.  No test uses the secret to decide anything but the comparison it is there for."""
import importlib
import io

import numpy as np
import pytest

import pairing_util as pm
import proof_util as pu
import systems_args_util as fa
import systems_util as fam
from lookup_util import R_MOD
from proof_util import h2, prover, transcript, verifier
from test_proof_systems import flip

kzg = importlib.import_module("halo2_pse_amd.kzg")

MEMBERS = [(fam, name) for name in fam.NAMES] + [(fa, name) for name in fa.NAMES]
IDS = [name for _, name in MEMBERS]
FAM_SECTIONS = ("advice", "fixed", "random", "sigma", "product", "lookup")
SEED = b"\x09" * 32


class Params:
    """what verify_proof and DualMSM read of a ParamsKZG, with another s_g2"""

    def __init__(self, params, s_g2):
        self.k, self.g, self.g2, self.s_g2 = params.k, params.g, params.g2, s_g2


def judge(su, proof, instances, multiopen, params=None, vk=None):
    """True: accepted, False: refused -- by the pairing, through SingleStrategy"""
    params = su.params if params is None else params
    try:
        out = verifier.verify_proof(params, su.pk.vk if vk is None else vk, instances, transcript.Blake2bRead(proof), multiopen,
                                    strategy=kzg.SingleStrategy(params))
    except (transcript.TranscriptError, verifier.VerifyError):
        return False
    assert out is None
    return True


def tamperings(su, proof, instances):
    """(what, proof bytes, instances, vk) of every tampering the families define: a flipped bit in the last scalar of every evaluation
    section, a wrong instance value, a wrong vk_repr"""
    e = su.system
    out = []
    for bit, section in enumerate(getattr(e, "SECTIONS", FAM_SECTIONS)):
        at, words = e.section(section)
        if words:
            out.append((section, flip(proof, at + words - 1, bit), instances, None))
    where = [(i, c) for i, inst in enumerate(instances) for c, values in enumerate(inst) if values]
    if where:
        i, c = where[-1]
        wrong = [[list(values) for values in inst] for inst in instances]
        wrong[i][c][-1] = (wrong[i][c][-1] + 1) % R_MOD
        out.append(("instance", proof, wrong, None))
    vk = prover.VerifyingKey(su.cs, su.k, pu.VK_REPR + 1, su.pk.vk.fixed_commitments, su.pk.vk.permutation_commitments)
    out.append(("vk_repr", proof, instances, vk))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
@pytest.mark.parametrize("family,name", MEMBERS, ids=IDS)
def test_gpu_the_pairing_and_the_secret_agree(family, name, multiopen):
    su = family.setup(name)
    assert su.params.g2 == kzg.G2_GENERATOR and su.params.s_g2 == pm.g2_raw(pm.g2_mul(pm.G2, pu.SECRET))
    witnesses = su.default_witnesses()
    instances = su.instances_of(witnesses)
    proof = su.prove(witnesses, multiopen=multiopen).bytes
    assert judge(su, proof, instances, multiopen) and su.accepts(proof, instances, multiopen)
    wrong_s = Params(su.params, kzg.g2_mul(kzg.G2_GENERATOR, pu.SECRET + 1))
    assert not judge(su, proof, instances, multiopen, params=wrong_s)
    cases = tamperings(su, proof, instances)
    assert len(cases) >= 4
    for what, bad_proof, bad_instances, vk in cases:
        by_secret = su.accepts(bad_proof, bad_instances, multiopen, vk)
        by_pairing = judge(su, bad_proof, bad_instances, multiopen, vk=vk)
        assert by_pairing == by_secret, (what, by_pairing, by_secret)
        assert not by_pairing, what


def _verify_into(strategy, su, proof, instances, multiopen):
    return verifier.verify_proof(su.params, su.pk.vk, instances, transcript.Blake2bRead(proof), multiopen, strategy=strategy)


@pytest.mark.gpu
def test_gpu_accumulator_strategy_folds_three_proofs_of_two_systems():
    a, b = fam.setup("sets3"), fam.setup("deg6")
    assert a.k == b.k and np.array_equal(a.params.g, b.params.g) and a.params.s_g2 == b.params.s_g2   # one params for both
    jobs = []
    for su, witnesses, multiopen in ((a, a.default_witnesses(), "gwc"), (b, b.default_witnesses(), "shplonk"),
                                     (a, [a.witness_of(a.seed + 7)], "shplonk")):
        jobs.append((su, su.prove(witnesses, multiopen=multiopen).bytes, su.instances_of(witnesses), multiopen))
    assert jobs[0][1] != jobs[2][1]

    def finalize(batch):
        acc = kzg.AccumulatorStrategy(a.params, h2.FrRng(SEED))
        for su, proof, instances, multiopen in batch:
            got = _verify_into(acc, su, proof, instances, multiopen)
            assert got is acc
        assert len(acc.msm_accumulator.left.terms) >= 3 and len(acc.msm_accumulator.right.terms) > 3   # kept unevaluated
        return acc.finalize()

    assert finalize(jobs)
    for bad in range(3):
        su, proof, instances, multiopen = jobs[bad]
        at, words = su.system.section("advice")
        batch = list(jobs)
        batch[bad] = (su, flip(proof, at + words - 1), instances, multiopen)
        assert not finalize(batch), bad
        verdicts = [judge(s, p, i, m) for s, p, i, m in batch]                   # one at a time: which one was it
        assert verdicts == [j != bad for j in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("format", list(h2.SerdeFormat), ids=lambda f: f.name)
def test_gpu_params_written_after_setup_verify_a_proof(format):
    su = fam.setup("bare")
    buf = io.BytesIO()
    su.params.write_custom(buf, format)
    with h2.ParamsKZG.read_custom(io.BytesIO(buf.getvalue()), format) as read:
        assert read.g2 == su.params.g2 == kzg.G2_GENERATOR and read.s_g2 == su.params.s_g2 != bytes(128)
        assert kzg.g2_check(read.s_g2) == (True, True)
        witnesses = su.default_witnesses()
        instances = su.instances_of(witnesses)
        proof = su.prove(witnesses).bytes
        assert judge(su, proof, instances, "shplonk", params=read)
        at, words = su.system.section("advice")
        assert not judge(su, flip(proof, at + words - 1), instances, "shplonk", params=read)


def test_the_members_are_the_three_families():
    """runs without a GPU: the module imports, and its members are the twelve systems of the other proof tests"""
    assert len(MEMBERS) == 12 and kzg.G2_GENERATOR == pm.g2_raw(pm.G2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 6])
def test_gpu_check_structure(k):
    h2.init()
    secret = pu.SECRET + k
    s_g2 = pm.g2_raw(pm.g2_mul(pm.G2, secret))
    with h2.ParamsKZG.setup(k, secret) as good, h2.ParamsKZG.setup(k, h2.fr_from_int(secret)) as limbs:
        assert good.g2 == kzg.G2_GENERATOR and good.s_g2 == s_g2 == limbs.s_g2 and np.array_equal(good.g, limbs.g)
        res = good.check_structure(SEED)
        assert res and res.ok and res.failed == () and repr(res) == "ParamsStructure(ok)"
        g, gl = good.g.copy(), good.g_lagrange.copy()
    outside = pm.g2_raw(pm.twist_point_outside_subgroup())
    wrong_s = pm.g2_raw(pm.g2_mul(pm.G2, secret + 1))

    def failed(g_, gl_, g2_, s_g2_):
        with h2.ParamsKZG(k, g_, gl_, g2_, s_g2_) as p:
            res = p.check_structure(SEED)
            assert bool(res) == (not res.failed)
            return res.failed

    assert failed(g, gl, kzg.G2_GENERATOR, s_g2) == ()
    assert failed(g, gl, outside, s_g2) == ("subgroup",)
    assert failed(g, gl, kzg.G2_GENERATOR, bytes(128)) == ("identity",)
    changed = gl.copy()
    changed[-1] = g[0] if k else h2.g1_from_int(pm.g1_mul(pm.G1, 3))
    assert failed(g, changed, kzg.G2_GENERATOR, s_g2) == ("lagrange",)
    # at k = 0 there is no g[1] and nothing ties s_g2 to g: (b) is vacuous
    assert failed(g, gl, kzg.G2_GENERATOR, wrong_s) == (("pairing",) if k else ())
    if k == 6:
        moved = g.copy()
        moved[5] = moved[4]
        assert failed(moved, None, kzg.G2_GENERATOR, s_g2) == ("powers",)      # g_lagrange derived from this g
        assert failed(moved, gl, kzg.G2_GENERATOR, s_g2) == ("powers", "lagrange")
        assert failed(g, gl, kzg.G2_GENERATOR, s_g2) == ()
