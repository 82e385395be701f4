"""create_proof and verify_proof on the family of constraint systems of systems_util.py: every member has a shape the SYSTEM of
check_util.py lacks (no permutation set or three, two or five pieces of h, fixed queries out of column order, nine rotations of one
column, two lookups over two proof instances, three phases), so the flow above the kernels -- how h is cut into pieces, how the
permutation sets are walked, in which order evaluations, queries and random draws come -- is run where that one system does not take it.

Every check is exact.  Proof lengths and section offsets are the hand-counted literals of systems_util.py (test_constraint_system.py
checks them without a GPU); the last test judges a proof without verifier.py, against the witness it was made from."""
import ctypes

import numpy as np
import pytest

import check_util as cu
import proof_util as pu
import systems_util as fam
from lookup_util import R_MOD, from_mont, to_mont
from proof_util import h2, transcript

THETA = 5
SEED = b"\x07" * 32
# the multiopen scheme of the tests that make one proof per system: GWC where the order of the x_last queries shows (sets3), both used
ONE_SCHEME = {"system": "shplonk", "bare": "gwc", "sets3": "gwc", "deg6": "shplonk", "rot9": "shplonk", "lookups2": "gwc", "phases3": "shplonk"}


def failures(su, cols, challenges=None):
    """h2.verify_witness on one instance's columns (the engine's MockProver::verify)"""
    cs = su.cs
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:cs.num_challenges]) if challenges is None else challenges
    m = cu.mont_cols(cols)
    copies = np.array(su.system.copies, dtype=np.uint32) if su.system.copies else None
    return h2.verify_witness(su.k, cs.gates, cs.lookups, to_mont([THETA])[0], su.b, cs.permutation, None, m["fixed"], m["advice"], m["instance"],
                             to_mont(challenges), copies=copies)


def word(proof_bytes, i):
    return proof_bytes[32 * i:32 * i + 32]


def flip(proof_bytes, i, bit=0):
    out = bytearray(proof_bytes)
    out[32 * i] ^= 1 << bit
    return bytes(out)


# ------------------------------------------------------------------ 1. satisfied
@pytest.mark.gpu
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_witnesses_are_satisfied(name):
    su = fam.setup(name)
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:su.cs.num_challenges])
    for provider in su.default_witnesses():
        cols = provider(challenges)
        assert failures(su, cols) == []
        assert fam.model_failures(su.system, cols, challenges, THETA) == []


# ------------------------------------------------------------------ 2. accept
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["parts", "full"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_proof_is_accepted(name, multiopen, form):
    su = fam.setup(name)
    witnesses = su.default_witnesses()
    assert len(witnesses) == su.system.n_instances
    proof = su.prove(witnesses, multiopen=multiopen, form=form)
    left, right = su.verify(proof.bytes, su.instances_of(witnesses), multiopen)
    assert left is not None and right is not None
    assert pu.pairing_holds(left, right)
    assert not pu.pairing_holds(left, right, pu.SECRET + 1)
    assert len(proof.bytes) == su.system.proof_bytes[multiopen]


# ------------------------------------------------------------------ 3. same bytes
@pytest.mark.gpu
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_same_seed_same_bytes(name):
    su = fam.setup(name)
    multiopen = ONE_SCHEME[name]
    base = su.prove(multiopen=multiopen).bytes
    assert len(base) == su.system.proof_bytes[multiopen]
    assert su.prove(multiopen=multiopen).bytes == base, "two runs"
    assert su.prove(multiopen=multiopen, form="full").bytes == base, "parts and full form"
    assert su.prove(multiopen=multiopen, resident=False).bytes == base, "resident and host columns"
    assert su.prove(multiopen=multiopen, resident=False, form="full").bytes == base, "host columns, full form"
    L = h2.lib()

    def stats():
        """kernels compiled, compilations failed, launches of a generated kernel, launches of the interpreter, disk-cache hits"""
        out = (ctypes.c_uint64 * 5)()
        L.h2hip_debug_evalh_codegen_stats(out)
        return list(out)

    try:
        for mode, what in ((0, "interpreter"), (2, "compiled inline")):
            L.h2hip_debug_set_evalh_codegen(ctypes.c_int(mode), ctypes.c_uint32(0))
            for form in ("parts", "full"):
                before = stats()
                assert su.prove(multiopen=multiopen, form=form).bytes == base, (what, form)
                after = stats()
                assert after[1] == before[1], "hiprtc rejected a generated kernel: " + L.h2hip_last_error().decode()
                if mode == 0:  # the mode is the one that ran
                    assert after[2] == before[2] and after[3] > before[3], (what, form, before, after)
                else:
                    assert after[2] > before[2] and after[3] == before[3], (what, form, before, after)
    finally:
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))
    assert su.prove(multiopen=multiopen, seed=b"\x08" * 32).bytes != base


# ------------------------------------------------------------------ 4. reject by witness
def _add(kind_column_row):
    column, row = kind_column_row

    def corrupt(su, cols):
        cols["advice"][column][row] = (cols["advice"][column][row] + 1) % R_MOD
    return corrupt


def _bare_not_boolean(su, cols):
    cols["advice"][0][2] = 2  # a (a - 1) = 2; + 1 could turn a valid 0 into a valid 1


def _lookups2_other_pair(su, cols):
    """a[12], b[12] become another row of the table (t0, t1): lookup 0 still holds, the copy a[10] = a[12] does not"""
    t0, t1 = cols["fixed"][2], cols["fixed"][3]
    j = next(j for j in range(1, su.u) if t0[j] != cols["advice"][0][10])
    cols["advice"][0][12], cols["advice"][1][12] = t0[j], t1[j]


G, P, LK = "gate", "permutation", "lookup"
# name, what, the corruption, the exact failures of verify_witness, whether the prover itself must refuse (a lookup input its table lacks)
CORRUPTIONS = [
    ("system", "gate", _add((2, 3)), [(G, 0, 4), (G, 1, 3)], False),
    ("bare", "gate", _bare_not_boolean, [(G, 0, 2)], False),
    ("sets3", "gate", _add((1, 3)), [(G, 0, 2), (G, 0, 3)], False),
    ("sets3", "copy in set 0", _add((0, 8)), [(P, 0, 7), (P, 0, 8)], False),
    ("sets3", "copy in set 1", _add((0, 9)), [(P, 0, 9), (P, 1, 3)], False),
    ("sets3", "copy in set 2", _add((1, 8)), [(P, 2, 7), (P, 2, 8)], False),
    ("deg6", "gate", _add((2, 2)), [(G, 0, 2)], False),
    ("deg6", "instance copy in the partial last set", _add((2, 8)), [(P, 2, 8), (P, 4, 1)], False),
    ("rot9", "gate", _add((0, 10)), [(G, 0, r) for r in range(6, 15)], False),
    ("rot9", "copy", _add((0, 17)), [(G, 0, 13), (G, 0, 14), (G, 0, 15), (P, 0, 2), (P, 0, 17)], False),
    ("lookups2", "gate", _add((1, 2)), [(G, 0, 2)], False),
    ("lookups2", "lookup 0", _add((0, 15)), [(LK, 0, 15)], True),
    ("lookups2", "lookup 1", _add((2, 22)), [(LK, 1, 22)], True),
    ("lookups2", "copy", _lookups2_other_pair, [(P, 0, 10), (P, 0, 12)], False),
    ("phases3", "gates", _add((1, 2)), [(G, 0, 2), (G, 1, 2)], False),
    ("phases3", "copy", _add((2, 8)), [(P, 0, 7), (P, 1, 8)], False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,what,corrupt,want,refused", CORRUPTIONS, ids=["%s-%s" % (c[0], c[1].replace(" ", "_")) for c in CORRUPTIONS])
def test_gpu_bad_witness_is_rejected(name, what, corrupt, want, refused):
    """one corrupted cell (in the last proof instance only: the ones before it stay valid)"""
    su = fam.setup(name)
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
    witnesses[-1] = bad
    if refused:
        with pytest.raises(h2.H2HipLookupError):
            su.prove(witnesses)
    else:
        multiopen = ONE_SCHEME[name]
        proof = su.prove(witnesses, multiopen=multiopen)
        assert not su.accepts(proof.bytes, su.instances_of(witnesses), multiopen)


@pytest.mark.gpu
def test_gpu_phases3_witness_from_other_challenges_is_rejected():
    """c computed from challenge_0 + 1: gate 0 fails on every active row under the challenges the transcript really drew"""
    su = fam.setup("phases3")
    handed = []

    def bad(challenges):
        handed.append(list(challenges))
        return su.columns(su.seed, [challenges[0] + 1] + list(challenges[1:]))

    proof = su.prove([bad], instances=[[]])
    real = proof.challenges["challenges"]
    assert len(real) == 3 and len(set(real)) == 3
    assert handed == [[0, 0, 0], [real[0], 0, 0], [real[0], real[1], 0]]  # one call per phase, each with the challenges drawn so far
    cols = bad(real)
    assert failures(su, su.columns(su.seed, real), real) == []
    assert failures(su, cols, real) == [("gate", 0, r) for r in range(fam.GATE_ROWS)]
    assert not su.accepts(proof.bytes, [[]])
    assert su.accepts(su.prove().bytes, [[]])


# ------------------------------------------------------------------ 5. reject by proof
@pytest.mark.gpu
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_tampered_proof_is_rejected(name):
    """one bit in one scalar of every evaluation section, the sections found from the hand layout"""
    su = fam.setup(name)
    e, multiopen = su.system, ONE_SCHEME[name]
    witnesses = su.default_witnesses()
    instances = su.instances_of(witnesses)
    proof = su.prove(witnesses, multiopen=multiopen).bytes
    assert len(proof) == e.proof_bytes[multiopen]
    assert su.accepts(proof, instances, multiopen)
    tampered = 0
    for bit, section in enumerate(("advice", "fixed", "random", "sigma", "product", "lookup")):
        at, words = e.section(section)
        if words:
            assert not su.accepts(flip(proof, at + words - 1, bit), instances, multiopen), section  # the section's last scalar
            tampered += 1
    assert tampered == 3 + sum(1 for key in ("sigma", "product", "lookup") if e.layout[key])
    if name == "sets3":  # product section: z_0(x), z_0(wx), z_0(x_last), z_1(x), z_1(wx), z_1(x_last), z_2(x), z_2(wx)
        at, words = e.section("product")
        assert words == 8 and word(proof, at + 2) != word(proof, at + 5)
        swapped = bytearray(proof)
        swapped[32 * (at + 2):32 * (at + 3)], swapped[32 * (at + 5):32 * (at + 6)] = word(proof, at + 5), word(proof, at + 2)
        assert not su.accepts(bytes(swapped), instances, multiopen)
    if name == "rot9":  # the ninth advice evaluation, a at rotation +4: the one past OPEN_MAX_POINTS
        at, words = e.section("advice")
        assert words == 9 and su.cs.advice_queries[8] == (0, 4)
        assert not su.accepts(flip(proof, at + 8, 5), instances, multiopen)
    if name == "deg6":  # the fifth commitment of h
        at, words = e.section("h")
        assert words == 5 and at + words == e.layout["points"]
        assert not su.accepts(flip(proof, at + 4, 1), instances, multiopen)


# ------------------------------------------------------------------ 6. the proof opens the witness it was given
def _omega(k):
    """the 2^k-th root of unity of Fr: 7 generates the multiplicative group, r - 1 = 2^28 t"""
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
@pytest.mark.parametrize("name", ["bare", "rot9", "phases3"])
def test_gpu_proof_opens_the_witness_it_was_given(name, oracle):
    """Without verifier.py: the blinded advice columns are rebuilt on integers -- the witness rows [0, u), then the blinding rows from
    FrRng(seed) in the documented order (per phase: b + 1 rows per column, then one blind per column) -- and every advice commitment
    must be their MSM over g_lagrange, every advice and fixed evaluation their value at x omega^rotation."""
    su = fam.setup(name)
    e, cs, k = su.system, su.cs, su.k
    proof = su.prove(seed=SEED)
    assert len(proof.bytes) == e.proof_bytes["shplonk"]
    cols = su.columns(su.seed, proof.challenges["challenges"])
    rng = h2.FrRng(SEED)
    blinded, order = [None] * cs.num_advice_columns, []
    for phase in cs.phases():
        columns = [c for c, p in enumerate(cs.advice_column_phase) if p == phase]
        rows = [from_mont(rng.draw(su.b + 1)) for _ in columns]
        rng.draw(len(columns))
        for c, r in zip(columns, rows):
            blinded[c] = cols["advice"][c][:su.u] + r
            assert len(blinded[c]) == su.n and blinded[c] != cols["advice"][c]
        order += columns
    assert rng.block == cs.num_advice_columns * (su.b + 2) and sorted(order) == list(range(cs.num_advice_columns))
    gl = su.params.g_lagrange
    for i, c in enumerate(order):
        want = oracle.g1_to_affine(oracle.best_multiexp(np.ascontiguousarray(to_mont(blinded[c])), gl, 4))
        assert transcript.point_from_bytes(word(proof.bytes, i)) == pu.mont_to_point(want), ("advice commitment", c)
    x = proof.challenges["x"]
    omega = _omega(k)
    assert omega == su.pk.domain.ints["omega"]
    for section, queries, columns in (("advice", cs.advice_queries, blinded), ("fixed", cs.fixed_queries, cols["fixed"])):
        at, words = e.section(section)
        assert words == len(queries)
        for q, (c, rotation) in enumerate(queries):
            z = x * pow(omega, rotation % su.n, R_MOD) % R_MOD
            assert transcript.scalar_from_bytes(word(proof.bytes, at + q)) == _eval_lagrange(columns[c], z, k), (section, c, rotation)
