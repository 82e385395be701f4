"""create_proof and verify_proof over the IPA commitment scheme (multiopen="ipa"): the family of systems_util.py and the shuffle and
mv-lookup systems of systems_args_util.py, each at its own small k, proved on the GPU and accepted or rejected by the package's own
verifier -- an IPA opening is valid when one MSM is the identity, so no trapdoor closes the check (proof_ipa_util.py).

What differs from the KZG flow is what these tests lean on: instance columns are committed instead of absorbed (only the commitment
ties a proof to its instance values), their evaluations are in the proof, and every commitment carries a blind that every query must
name again.  Field offsets are the entry's hand-counted layout plus the opening's tail (proof_ipa_util.Setup.fields)."""
import pytest

import proof_ipa_util as piu
import proof_util as pu
import systems_args_util as args_fam
import systems_util as fam
from lookup_util import R_MOD, from_mont
from proof_ipa_util import ipa
from proof_util import h2, prover, transcript, verifier

SEED = b"\x07" * 32
ENTRIES = [(fam, name) for name in fam.NAMES] + [(args_fam, name) for name in args_fam.NAMES]
IDS = [name for _, name in ENTRIES]


def setup(name, k=None):
    family = fam if name in fam.NAMES else args_fam
    return piu.setup(family.entry(name), k)


def flip(proof_bytes, word, bit=0):
    out = bytearray(proof_bytes)
    out[32 * word] ^= 1 << bit
    return bytes(out)


# ------------------------------------------------------------------ 1. accepted
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["parts", "full"])
@pytest.mark.parametrize("family,name", ENTRIES, ids=IDS)
def test_gpu_ipa_proof_is_accepted(family, name, form):
    su = setup(name)
    witnesses = su.default_witnesses()
    assert len(witnesses) == su.system.n_instances
    proof = su.prove(witnesses, form=form)
    instances = su.instances_of(witnesses)
    assert su.verify(proof.bytes, instances) is None          # SingleStrategy.process: no IPAError
    su.fields(proof.bytes)                                    # the length is the layout's: points, evaluations, the opening's tail
    assert proof.stages == list(prover.ARGUMENT_STAGES)
    # the check is not vacuous: the same proof under another verifying-key scalar is refused
    vk = prover.VerifyingKey(su.cs, su.k, pu.VK_REPR + 1, su.pk.vk.fixed_commitments, su.pk.vk.permutation_commitments, scheme="ipa")
    assert not su.accepts(proof.bytes, instances, vk=vk)


@pytest.mark.gpu
def test_gpu_ipa_same_seed_same_bytes_in_every_mode():
    su = setup("system")
    instances = su.instances_of(su.default_witnesses())
    base = su.prove().bytes
    assert su.prove().bytes == base, "two runs"
    assert su.prove(form="full").bytes == base, "parts and full form"
    host = su.prove(resident=False)
    assert host.bytes == base, "resident and host columns"
    assert su.prove(resident=False, form="full").bytes == base, "host columns, full form"
    assert any(what == "opening: a queried polynomial" and nbytes == 32 << su.k for _, nbytes, what in host.transfers)
    assert su.accepts(base, instances)
    other = su.prove(seed=b"\x08" * 32).bytes
    assert other != base and len(other) == len(base)
    assert su.accepts(other, instances)


# ------------------------------------------------------------------ 2. accumulation
@pytest.mark.gpu
def test_gpu_ipa_two_proofs_through_one_accumulator():
    su = setup("system")
    instances = su.instances_of(su.default_witnesses())
    first, second = su.prove().bytes, su.prove(seed=b"\x08" * 32).bytes
    acc = ipa.AccumulatorStrategy(su.params, h2.FrRng(b"\x21" * 32))
    assert su.verify(first, instances, strategy=acc) is acc
    assert su.verify(second, instances, strategy=acc) is acc
    assert acc.finalize() is True
    # one bit of the second proof's c: both proofs are sound on their own, the accumulated MSM is not the identity
    bad = flip(second, len(second) // 32 - 2)
    acc = ipa.AccumulatorStrategy(su.params, h2.FrRng(b"\x21" * 32))
    su.verify(first, instances, strategy=acc)
    try:
        su.verify(bad, instances, strategy=acc)
        assert acc.finalize() is False
    except (transcript.TranscriptError, ipa.IPAError):
        pass


# ------------------------------------------------------------------ 3. instances matter
@pytest.mark.gpu
def test_gpu_ipa_instances_are_committed_and_checked():
    """the instance values are not absorbed: only the verifier's own commitment of them ties the proof to them"""
    su = setup("system")
    witnesses = [su.witness_of(su.seed), su.witness_of(su.seed + 1)]       # two instances of one system, each with an instance column
    instances = su.instances_of(witnesses)
    assert len(instances) == 2 and instances[0] != instances[1] and len(instances[0][0]) == pu.ACTIVE + 1
    proof = su.prove(witnesses).bytes
    assert su.accepts(proof, instances)
    for i, row in ((0, 2), (1, 0), (1, pu.ACTIVE)):
        wrong = [[list(col) for col in inst] for inst in instances]
        wrong[i][0][row] = (wrong[i][0][row] + 1) % R_MOD
        assert not su.accepts(proof, wrong), (i, row)
    assert not su.accepts(proof, [instances[1], instances[0]])
    assert instances[0][0][-1] != 0
    assert not su.accepts(proof, [[instances[0][0][:-1]], instances[1]])   # one value fewer: zero-padded, another commitment
    with pytest.raises(verifier.VerifyError, match="InvalidInstances"):
        su.verify(proof, [[instances[0][0], []], instances[1]])
    with pytest.raises(verifier.VerifyError, match="InstanceTooLarge"):
        su.verify(proof, [[[1] * (su.u + 1)], instances[1]])
    one = setup("deg6")                                                    # the instance column in the partial last permutation set
    w = one.default_witnesses()
    p = one.prove(w).bytes
    inst = one.instances_of(w)
    assert one.accepts(p, inst)
    assert not one.accepts(p, [[[inst[0][0][0], (inst[0][0][1] + 1) % R_MOD]]])


# ------------------------------------------------------------------ 4. tamper
TAMPER = ["advice commitment", "h piece commitment", "instance evaluation", "advice evaluation", "q' commitment", "L_0", "L_last", "c", "f"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["system", "phases3", "rot9"])
def test_gpu_ipa_tampered_proof_is_rejected(name):
    """one bit in one field of every kind; system has a lookup, two phases and an instance column, phases3 three phases and no instance
    column (its proof has no instance evaluation to flip), rot9 an instance column queried at a rotation"""
    su = setup(name)
    witnesses = su.default_witnesses()
    instances = su.instances_of(witnesses)
    proof = su.prove(witnesses).bytes
    assert su.accepts(proof, instances)
    fields = su.fields(proof)
    assert set(fields) == {f for f in TAMPER if f != "instance evaluation" or su.cs.instance_queries}
    assert ("instance evaluation" in fields) == (name != "phases3")
    assert len(set(fields.values())) == len(fields)
    for bit, (field, word) in enumerate(fields.items()):
        assert not su.accepts(flip(proof, word, bit % 8), instances), field
    assert not su.accepts(proof + b"\x00", instances)          # trailing bytes
    assert not su.accepts(proof[:-32], instances)              # f missing


# ------------------------------------------------------------------ 5. bad witness
@pytest.mark.gpu
def test_gpu_ipa_bad_witness_is_rejected():
    """test_proof_systems.CORRUPTIONS's first entry restated: c[3] + 1 in the SYSTEM breaks gate 0 at row 4 and gate 1 at row 3"""
    su = setup("system")
    good = su.default_witnesses()[0]

    def bad(challenges):
        cols = good(challenges)
        cols["advice"][2][3] = (cols["advice"][2][3] + 1) % R_MOD
        return cols

    proof = su.prove([bad])
    assert not su.accepts(proof.bytes, su.instances_of([bad]))
    assert su.accepts(su.prove([good]).bytes, su.instances_of([good]))


# ------------------------------------------------------------------ 6. the proof opens the witness it was given
def _omega(k):
    omega = pow(pow(7, (R_MOD - 1) >> 28, R_MOD), 1 << (28 - k), R_MOD)
    assert pow(omega, 1 << k, R_MOD) == 1 and pow(omega, 1 << (k - 1), R_MOD) == R_MOD - 1
    return omega


def _eval_lagrange(col, z, k):
    """sum_i col[i] l_i(z) with l_i(z) = omega^i (z^n - 1) / (n (z - omega^i))"""
    n, omega = 1 << k, _omega(k)
    common = (pow(z, n, R_MOD) - 1) * pow(n, -1, R_MOD) % R_MOD
    acc, w = 0, 1
    for v in col:
        acc = (acc + v * w % R_MOD * pow(z - w, -1, R_MOD)) % R_MOD
        w = w * omega % R_MOD
    return acc * common % R_MOD


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rot9", "system"])
def test_gpu_ipa_proof_opens_the_witness_it_was_given(name):
    """Without verifier.py: the instance evaluations in the proof are the zero-padded instance columns at x omega^rotation, and the
    evaluations of the phase-0 advice columns those of the witness rows [0, u) followed by the blinding rows FrRng(seed) draws first."""
    su = setup(name)
    cs, k = su.cs, su.k
    proof = su.prove(seed=SEED)
    cols = su.columns(su.seed, proof.challenges["challenges"])
    rng = h2.FrRng(SEED)
    phase0 = [c for c, p in enumerate(cs.advice_column_phase) if p == 0]
    blinded = {c: cols["advice"][c][:su.u] + from_mont(rng.draw(su.b + 1)) for c in phase0}
    x, omega, fields = proof.challenges["x"], _omega(k), su.fields(proof.bytes)
    word = lambda i: transcript.scalar_from_bytes(proof.bytes[32 * i:32 * i + 32])  # noqa: E731
    instance = su.instances_of(su.default_witnesses())[0]
    assert cs.instance_queries
    for q, (c, rotation) in enumerate(cs.instance_queries):
        column = list(instance[c]) + [0] * (su.n - len(instance[c]))
        z = x * pow(omega, rotation % su.n, R_MOD) % R_MOD
        assert word(fields["instance evaluation"] + q) == _eval_lagrange(column, z, k), ("instance", c, rotation)
    checked = 0
    for q, (c, rotation) in enumerate(cs.advice_queries):
        if c in blinded:
            z = x * pow(omega, rotation % su.n, R_MOD) % R_MOD
            assert word(fields["advice evaluation"] + q) == _eval_lagrange(blinded[c], z, k), ("advice", c, rotation)
            checked += 1
    assert checked and cs.advice_queries[0][0] in blinded


# ------------------------------------------------------------------ 7. the key
@pytest.mark.gpu
def test_gpu_ipa_key_commitments_are_the_msm_plus_w():
    """commit_lagrange(col, Blind::default()) with Blind::default() = 1: the KZG-style MSM over g_lagrange, plus W, on integers"""
    su = setup("sets3")
    gl = [pu.mont_to_point(p) for p in su.params.g_lagrange]
    assert su.pk.vk.scheme == "ipa" and su.pk.params is su.params
    for cols, got in ((su.fixed, su.pk.vk.fixed_commitments), (su.pk.host["permutations"], su.pk.vk.permutation_commitments)):
        assert len(cols) == len(got) and len(got) in (2, 3)
        for col, point in zip(cols, got):
            msm = None
            for s, g in zip(from_mont(col), gl):
                msm = pu.g1_add(msm, pu.g1_mul(g, s))
            assert point == pu.g1_add(msm, su.params.w) and point != msm
    # the key shares the params' resident, pinned generators
    assert su.pk.d_g is su.params.d_g() and su.pk.d_g_lagrange is su.params.d_g_lagrange()


# ------------------------------------------------------------------ 8. misuse
@pytest.mark.gpu
def test_gpu_ipa_misuse_is_refused():
    su, kzg = setup("bare"), fam.setup("bare")
    witnesses = su.default_witnesses()
    instances = su.instances_of(witnesses)
    proof = su.prove(witnesses).bytes
    w = lambda s: s.witness_fn(witnesses, True)  # noqa: E731
    T = transcript.Blake2bWrite
    with pytest.raises(ValueError, match="proving key was built over other params"):
        prover.create_proof(kzg.params, su.pk, instances, w(su), T(), SEED, multiopen="ipa")
    with pytest.raises(ValueError, match="multiopen 'ipa' with KZG params"):
        prover.create_proof(kzg.params, kzg.pk, instances, w(kzg), T(), SEED, multiopen="ipa")
    with pytest.raises(ValueError, match="multiopen 'shplonk' with IPA params"):
        prover.create_proof(su.params, su.pk, instances, w(su), T(), SEED, multiopen="shplonk")
    with pytest.raises(ValueError, match="multiopen: 'shplonk', 'gwc' or 'ipa'"):
        prover.create_proof(su.params, su.pk, instances, w(su), T(), SEED, multiopen="kzg")
    R = lambda: transcript.Blake2bRead(proof)  # noqa: E731
    single = lambda: ipa.SingleStrategy(su.params)  # noqa: E731
    with pytest.raises(ValueError, match="takes an ipa.ParamsIPA"):
        verifier.verify_proof(kzg.params, su.pk.vk, instances, R(), multiopen="ipa", strategy=single())
    with pytest.raises(ValueError, match="with the verifying key of KZG params"):
        verifier.verify_proof(su.params, kzg.pk.vk, instances, R(), multiopen="ipa", strategy=single())
    with pytest.raises(ValueError, match="needs a strategy"):
        verifier.verify_proof(su.params, su.pk.vk, instances, R(), multiopen="ipa")
    with pytest.raises(ValueError, match="strategy belongs to multiopen 'ipa'"):
        verifier.verify_proof(kzg.params, kzg.pk.vk, instances, R(), multiopen="shplonk", strategy=single())
    with pytest.raises(ValueError, match="takes KZG params"):
        verifier.verify_proof(su.params, kzg.pk.vk, instances, R(), multiopen="gwc")
    with pytest.raises(ValueError, match="with the verifying key of IPA params"):
        verifier.verify_proof(kzg.params, su.pk.vk, instances, R(), multiopen="shplonk")
    assert su.accepts(proof, instances)                        # none of the refusals left anything behind


# ------------------------------------------------------------------ 9. residency
@pytest.mark.gpu
def test_gpu_ipa_resident_proof_moves_less_than_one_column():
    """the criterion of test_proof.py at its k = 10 (a column is 32 KiB): with resident=True no entry of proof.transfers is a column;
    the host mode uploads each queried polynomial once for the opening and says so"""
    su = setup("system", 10)
    column_bytes = 32 << su.k
    proof = su.prove()
    assert proof.transfers and {d for d, _, _ in proof.transfers} == {"h2d", "d2h"}
    for direction, nbytes, what in proof.transfers:
        assert nbytes < column_bytes, (direction, nbytes, what)
    assert proof.total("h2d") < column_bytes and proof.total("d2h") < column_bytes
    assert su.accepts(proof.bytes, su.instances_of(su.default_witnesses()))
    assert len(proof.bytes) == len(setup("system").prove().bytes) + 32 * 2 * (10 - 5)   # 2 (k - 5) more L_j / R_j, nothing else grows
