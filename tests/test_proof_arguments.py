"""create_proof and verify_proof on the five systems of systems_args_util.py, the ones with shuffle and mv-lookup (logUp) arguments:
the checks of test_proof_systems.py where the two arguments' stages, folds, evaluations and queries run -- alone (shuffle1, mv1), twice
and across phases and instances (shuffles2), at K = 3 and degree 6 (mv3), and next to a halo2 lookup and two permutation sets
(all_args), the one member in which their order relative to the other arguments can be wrong.

Every check is exact.  Proof lengths and section offsets are the hand-counted literals of systems_args_util.py
(test_constraint_system_args.py checks them without a GPU).  Two tests judge a proof without verifier.py: z, m and phi are rebuilt on
integers from the witness, the proof's challenges and FrRng(seed) in the documented draw order.  The last test pins the proofs of the
seven earlier systems to the digests their tree wrote before these arguments entered create_proof."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import check_util as cu
import mvlookup_util as mv
import proof_util as pu
import shuffle_util as sh
import systems_args_util as fa
import systems_util as fam
from lookup_util import R_MOD, from_mont, to_mont
from proof_util import h2, prover, transcript
from test_proof_systems import _eval_lagrange, _omega, flip, word

THETA = 5
SEED = b"\x07" * 32
# GWC where the point order shows (all_args has four points, an x_last query and an x_inv query), both schemes used
ONE_SCHEME = {"shuffle1": "shplonk", "shuffles2": "gwc", "mv1": "gwc", "mv3": "shplonk", "all_args": "gwc"}


GATES, LOOKUPS, SHUFFLES, MVLOOKUPS = range(4)  # the stages of h2hip_debug_evalh_codegen_stage_stats, in its order
# h2hip_debug_set_evalh_codegen's mode, what it is, the stages whose generated kernels must then run (the others: the interpreter).
# 2: compiled inline; + 32: no shuffle or mv-lookup kernels; + 64: both
CODEGEN_LEGS = ((0, "interpreter", ()), (2 + 32, "stage kernels off", (GATES, LOOKUPS)), (2 + 64, "stage kernels on", (GATES, LOOKUPS, SHUFFLES, MVLOOKUPS)))


def failures(su, cols, challenges=None):
    """h2.verify_witness on one instance's columns, shuffles and mv-lookups included"""
    cs = su.cs
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:cs.num_challenges]) if challenges is None else challenges
    m = cu.mont_cols(cols)
    copies = np.array(su.system.copies, dtype=np.uint32) if su.system.copies else None
    return h2.verify_witness(su.k, cs.gates, cs.lookups, to_mont([THETA])[0], su.b, cs.permutation, None, m["fixed"], m["advice"], m["instance"],
                             to_mont(challenges), copies=copies, shuffles=cs.shuffles, mvlookups=cs.mv_lookups)


# ------------------------------------------------------------------ 1. satisfied
@pytest.mark.gpu
@pytest.mark.parametrize("name", fa.NAMES)
def test_gpu_witnesses_are_satisfied(name):
    su = fa.setup(name)
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:su.cs.num_challenges])
    for provider in su.default_witnesses():
        cols = provider(challenges)
        assert failures(su, cols) == []
        assert fa.model_failures(su.system, cols, challenges, THETA) == []


# ------------------------------------------------------------------ 2. accept
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["parts", "full"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
@pytest.mark.parametrize("name", fa.NAMES)
def test_gpu_proof_is_accepted(name, multiopen, form):
    su = fa.setup(name)
    witnesses = su.default_witnesses()
    assert len(witnesses) == su.system.n_instances
    proof = su.prove(witnesses, multiopen=multiopen, form=form)
    assert len(proof.bytes) == su.system.proof_bytes[multiopen]
    left, right = su.verify(proof.bytes, su.instances_of(witnesses), multiopen)
    assert left is not None and right is not None
    assert pu.pairing_holds(left, right)
    assert not pu.pairing_holds(left, right, pu.SECRET + 1)


# ------------------------------------------------------------------ 3. same bytes
@pytest.mark.gpu
@pytest.mark.parametrize("name", fa.NAMES)
def test_gpu_same_seed_same_bytes(name):
    """the same bytes from two runs, both forms, resident and host columns, and from evaluate_h on the interpreter, with the shuffle and
    mv-lookup stage kernels off (gates and lookups generated) and with them on; the per-stage launch counters show that each stage
    the member has ran the way the mode says, in both forms"""
    su = fa.setup(name)
    multiopen = ONE_SCHEME[name]
    base = su.prove(multiopen=multiopen).bytes
    assert len(base) == su.system.proof_bytes[multiopen]
    assert su.prove(multiopen=multiopen).bytes == base, "two runs"
    assert su.prove(multiopen=multiopen, form="full").bytes == base, "parts and full form"
    assert su.prove(multiopen=multiopen, resident=False).bytes == base, "resident and host columns"
    assert su.prove(multiopen=multiopen, resident=False, form="full").bytes == base, "host columns, full form"
    L = h2.lib()
    present = [True, bool(su.cs.lookups), bool(su.cs.shuffles), bool(su.cs.mv_lookups)]
    assert present[SHUFFLES] or present[MVLOOKUPS]

    def stats():
        """(compilations failed, [launches of a generated kernel per stage], [launches of the interpreter per stage]), the stages
        being the gates, the halo2 lookups, the shuffles and the mv-lookups"""
        a, b = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 9)()
        assert L.h2hip_debug_evalh_codegen_stats(a) == 0 and L.h2hip_debug_evalh_codegen_stage_stats(b) == 0
        return a[1], [b[0], b[2], b[4], b[6]], [b[1], b[3], b[5], b[7]]

    try:
        for mode, what, generated in CODEGEN_LEGS:
            assert L.h2hip_debug_set_evalh_codegen(ctypes.c_int(mode), ctypes.c_uint32(0)) == 0
            for form in ("parts", "full"):
                failed0, gen0, interp0 = stats()
                assert su.prove(multiopen=multiopen, form=form).bytes == base, (what, form)
                failed1, gen1, interp1 = stats()
                assert failed1 == failed0, "hiprtc rejected a generated kernel: " + L.h2hip_last_error().decode()
                for stage in (GATES, LOOKUPS, SHUFFLES, MVLOOKUPS):  # every stage the member has ran the way the mode says, no other ran
                    ran_gen, ran_interp = gen1[stage] > gen0[stage], interp1[stage] > interp0[stage]
                    want = (present[stage] and stage in generated, present[stage] and stage not in generated)
                    assert (ran_gen, ran_interp) == want, (what, form, stage, gen0, gen1, interp0, interp1)
    finally:
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
    assert su.prove(multiopen=multiopen, seed=b"\x08" * 32).bytes != base


# ------------------------------------------------------------------ 4. reject by proof
@pytest.mark.gpu
@pytest.mark.parametrize("name", fa.NAMES)
def test_gpu_tampered_proof_is_rejected(name):
    """one bit in the last scalar of every evaluation section, the two new sections included, found from the hand layout"""
    su = fa.setup(name)
    e, multiopen = su.system, ONE_SCHEME[name]
    witnesses = su.default_witnesses()
    instances = su.instances_of(witnesses)
    proof = su.prove(witnesses, multiopen=multiopen).bytes
    assert len(proof) == e.proof_bytes[multiopen]
    assert su.accepts(proof, instances, multiopen)
    tampered = 0
    for bit, section in enumerate(e.SECTIONS):
        at, words = e.section(section)
        if words:
            assert not su.accepts(flip(proof, at + words - 1, bit), instances, multiopen), section
            tampered += 1
    assert tampered == 3 + sum(1 for key in ("sigma", "product", "lookup", "mvlookup", "shuffle") if e.layout[key])
    assert e.layout["mvlookup"] or e.layout["shuffle"]
    for section, per_argument in (("mvlookup", 3), ("shuffle", 2)):  # every scalar of the first argument's group, not the last alone
        at, words = e.section(section)
        for i in range(min(words, per_argument)):
            assert not su.accepts(flip(proof, at + i, 3), instances, multiopen), (section, i)
    # the first m or shuffle z commitment: behind the advice commitments (and all_args' four permuted columns, shuffles2's two set products)
    first_new_point = {"shuffle1": 4, "shuffles2": 10, "mv1": 2, "mv3": 7, "all_args": 16}[name]
    assert not su.accepts(flip(proof, first_new_point, 2), instances, multiopen)


# ------------------------------------------------------------------ 5. reject by witness
def _add(column, row):
    def corrupt(su, cols):
        cols["advice"][column][row] = (cols["advice"][column][row] + 1) % R_MOD
    return corrupt


SH, MV = "shuffle", "mvlookup"
# name, what, the corruption, the exact failures of verify_witness, the H2HipLookupError's text when the prover itself must refuse.
# A shuffle-side cell at row i: the input row PERM(i) it held no longer has its partner.
CORRUPTIONS = [
    ("shuffle1", "shuffle side", _add(3, 4), [(SH, 0, fa.perm1(4, 10))], None),
    ("shuffles2", "shuffle 0 side", _add(2, 4), [(SH, 0, fa.perm1(4, 10))], None),
    ("shuffles2", "shuffle 1 side", _add(3, 5), [(SH, 1, fa.perm2(5, 10))], None),
    ("mv1", "input", _add(0, 21), [(MV, 0, 21)], "argument 0, input 0"),
    ("mv3", "input 2", _add(4, 20), [(MV, 2, 20)], "argument 0, input 2"),
    ("all_args", "shuffle side", _add(4, 12), [(SH, 0, fa.perm1(12, 26))], None),
    ("all_args", "mv input 1", _add(2, 15), [(MV, 1, 15)], "argument 0, input 1"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,what,corrupt,want,refused", CORRUPTIONS, ids=["%s-%s" % (c[0], c[1].replace(" ", "_")) for c in CORRUPTIONS])
def test_gpu_bad_witness_is_rejected(name, what, corrupt, want, refused):
    """one corrupted cell (in the last proof instance only: the ones before it stay valid)"""
    su = fa.setup(name)
    witnesses = su.default_witnesses()
    good = witnesses[-1]

    def bad(challenges):
        cols = good(challenges)
        corrupt(su, cols)
        return cols

    placeholder = list(pu.PLACEHOLDER_CHALLENGES[:su.cs.num_challenges])
    for w in witnesses[:-1]:
        assert failures(su, w(placeholder)) == []
    assert failures(su, bad(placeholder)) == want
    assert fa.model_failures(su.system, bad(placeholder), placeholder, THETA) == want
    witnesses[-1] = bad
    if refused:
        with pytest.raises(h2.H2HipLookupError, match=refused):
            su.prove(witnesses)
    else:
        multiopen = ONE_SCHEME[name]
        proof = su.prove(witnesses, multiopen=multiopen)
        assert len(proof.bytes) == su.system.proof_bytes[multiopen]
        assert not su.accepts(proof.bytes, su.instances_of(witnesses), multiopen)
        assert su.accepts(su.prove(multiopen=multiopen).bytes, su.instances_of(su.default_witnesses()), multiopen)


# ------------------------------------------------------------------ 6. the proof opens the columns the definitions give
def _blinded_advice(su, rng, cols):
    """draw 1 of prover.py's list for a one-phase, one-instance system: b + 1 rows per advice column, then one blind per column"""
    cs = su.cs
    assert list(cs.phases()) == [0]
    rows = [from_mont(rng.draw(su.b + 1)) for _ in range(cs.num_advice_columns)]
    rng.draw(cs.num_advice_columns)
    return [cols["advice"][c][:su.u] + rows[c] for c in range(cs.num_advice_columns)]


def _commitment(oracle, su, column):
    return pu.mont_to_point(oracle.g1_to_affine(oracle.best_multiexp(np.ascontiguousarray(to_mont(column)), su.params.g_lagrange, 4)))


@pytest.mark.gpu
def test_gpu_shuffle1_proof_opens_the_product_of_its_witness(oracle):
    """Without verifier.py: z rebuilt on integers from the witness, the proof's theta and gamma and draw 4c (b rows of z, after the
    advice draws) must be what the proof commits to (the MSM over g_lagrange) and opens at x and omega x."""
    su = fa.setup("shuffle1")
    e, cs, k = su.system, su.cs, su.k
    proof = su.prove(seed=SEED)
    assert len(proof.bytes) == e.proof_bytes["shplonk"]
    cols = su.columns(su.seed, [])
    rng = h2.FrRng(SEED)
    advice = _blinded_advice(su, rng, cols)
    z_rows = from_mont(rng.draw(su.b))                                   # draw 4c: no lookup, no set and no mv-lookup draws before it
    theta, gamma = proof.challenges["theta"], proof.challenges["gamma"]
    c = sh.Columns(cols["fixed"], advice, [], [], su.n)
    inp, shf = cs.shuffles[0]
    z = sh.shuffle_product(sh.compress_column(inp, theta, c), sh.compress_column(shf, theta, c), gamma, z_rows, su.b)
    assert z[su.u] == 1 and len(set(z[:su.u])) > 2
    assert transcript.point_from_bytes(word(proof.bytes, 4)) == _commitment(oracle, su, z)
    x, omega = proof.challenges["x"], _omega(k)
    at, words = e.section("shuffle")
    assert words == 2 and at + words == e.evaluation_words()
    assert transcript.scalar_from_bytes(word(proof.bytes, at)) == _eval_lagrange(z, x, k)
    assert transcript.scalar_from_bytes(word(proof.bytes, at + 1)) == _eval_lagrange(z, x * omega % R_MOD, k)


@pytest.mark.gpu
def test_gpu_mv1_proof_opens_the_multiplicities_and_sum_of_its_witness(oracle):
    """Without verifier.py: m (no blinding rows; draw 2b is its blind alone) and phi (draw 4b: b rows, then its blind) rebuilt on integers
    from the witness and the proof's theta and beta must be what the proof commits to and opens: phi at x and omega x, m at x."""
    su = fa.setup("mv1")
    e, cs, k = su.system, su.cs, su.k
    proof = su.prove(seed=SEED)
    assert len(proof.bytes) == e.proof_bytes["shplonk"]
    cols = su.columns(su.seed, [])
    rng = h2.FrRng(SEED)
    advice = _blinded_advice(su, rng, cols)
    rng.draw(1)                                                          # draw 2b
    phi_rows = from_mont(rng.draw(su.b))                                 # draw 4b
    theta, beta = proof.challenges["theta"], proof.challenges["beta"]
    c = sh.Columns(cols["fixed"], advice, [], [], su.n)
    inputs, tab = cs.mv_lookups[0]
    f, t = [sh.compress_column(inp, theta, c) for inp in inputs], sh.compress_column(tab, theta, c)
    m, missing = mv.multiplicities(f, t, su.b)
    assert missing == [False] and sum(m) == su.u and m[fa.MV1_REPEAT[1]] == 0 and m[fa.MV1_REPEAT[0]] >= 2 and m[su.u:] == [0] * (su.b + 1)
    phi = mv.grand_sum(f, t, m, beta, phi_rows, su.b)
    assert phi[su.u] == 0 and any(phi[1:su.u])
    assert transcript.point_from_bytes(word(proof.bytes, 2)) == _commitment(oracle, su, m)
    assert transcript.point_from_bytes(word(proof.bytes, 3)) == _commitment(oracle, su, phi)
    x, omega = proof.challenges["x"], _omega(k)
    at, words = e.section("mvlookup")
    assert words == 3 and at + words == e.evaluation_words()
    assert transcript.scalar_from_bytes(word(proof.bytes, at)) == _eval_lagrange(phi, x, k)
    assert transcript.scalar_from_bytes(word(proof.bytes, at + 1)) == _eval_lagrange(phi, x * omega % R_MOD, k)
    assert transcript.scalar_from_bytes(word(proof.bytes, at + 2)) == _eval_lagrange(m, x, k)


# ------------------------------------------------------------------ 7. residency
@pytest.mark.gpu
def test_gpu_resident_all_args_proof_moves_less_than_one_column():
    """all_args at k = 10, two instances: with resident columns every entry of proof.transfers is below one column (32 KiB) -- no
    stage of the two arguments hands a column over -- while the host path moves many"""
    su = fa.setup("all_args", k=10)
    column_bytes = 32 << su.k
    witnesses = su.default_witnesses()
    proof = su.prove(witnesses)
    assert su.accepts(proof.bytes, su.instances_of(witnesses))
    assert proof.transfers and {d for d, _, _ in proof.transfers} == {"h2d", "d2h"}
    for direction, nbytes, what in proof.transfers:
        assert nbytes < column_bytes, (direction, nbytes, what)
    whats = {what for _, _, what in proof.transfers}
    # the stages between theta and y ran in ARGUMENT_STAGES' order, and their commitments came down in that order, instance by instance
    assert proof.stages == list(prover.ARGUMENT_STAGES)
    commits = [what for d, _, what in proof.transfers if d == "d2h" and what.endswith("commitments")]
    stage_commits = ["permuted commitments", "mv-lookup multiplicity commitments", "permutation product commitments",
                     "lookup product commitments", "mv-lookup sum commitments", "shuffle product commitments"]
    assert len(stage_commits) == len(prover.ARGUMENT_STAGES)
    first = commits.index(stage_commits[0])
    assert commits[first:first + 12] == [what for what in stage_commits for _ in range(2)]
    assert ("d2h", 8, "mv-lookup verdict flags (one per input column)") in proof.transfers  # K = 2 input columns, four bytes each
    assert {"mv-lookup multiplicity commitments", "mv-lookup sum commitments", "shuffle product commitments", "mv-lookup evaluations",
            "shuffle evaluations"} <= whats
    host = su.prove(witnesses, resident=False)
    assert host.bytes == proof.bytes
    assert host.total("h2d") > 20 * column_bytes and host.total("d2h") > 10 * column_bytes


# ------------------------------------------------------------------ 8. the earlier systems' proofs are the bytes they were
@pytest.mark.gpu
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_earlier_systems_keep_their_proof_bytes(name):
    """tests/golden/proof_digests.json: tools/proof_digests.py's output on the tree before shuffles and mv-lookups entered create_proof"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proof_digests.json")) as f:
        golden = json.load(f)
    assert set(golden) == set(fam.NAMES)
    su = fam.setup(name)
    for multiopen in ("shplonk", "gwc"):
        proof = su.prove(multiopen=multiopen, form="parts", resident=True, seed=SEED)
        assert hashlib.sha256(proof.bytes).hexdigest() == golden[name][multiopen], multiopen
