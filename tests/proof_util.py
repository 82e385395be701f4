"""Helpers of the proof tests: the package's transcript / prover / verifier modules (loaded through conftest.load_pkg(), as evalh_util
does), Python-integer affine arithmetic on bn256 G1 for closing the verifier's check with the setup secret, and the SYSTEM of
check_util.py as a ConstraintSystem with a witness whose selector is one on a few rows only, so that its instance column is short, and
Setup: params and keys of any System (systems_util.py has the family), that SYSTEM by default."""
import importlib
import random

import numpy as np

import check_util as cu
from conftest import load_pkg
from lookup_util import R_MOD, to_mont

h2 = load_pkg()
transcript = importlib.import_module("halo2_pse_amd.transcript")
prover = importlib.import_module("halo2_pse_amd.prover")
verifier = importlib.import_module("halo2_pse_amd.verifier")

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
G1 = (1, 2)
SECRET = 0x1D0C5EC2E7A9B3F40718293A4B5C6D7E8F9
VK_REPR = 0x0123456789ABCDEF0FEDCBA9876543210
ACTIVE = 10  # the selector s is one on rows 1 .. ACTIVE; the instance column holds rows 0 .. ACTIVE


# ---- bn256 G1 on integers, affine: None is the identity
def g1_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return (x, (lam * (p[0] - x) - p[1]) % Q)


def g1_mul(p, k):
    acc = None
    for bit in bin(k % R_MOD)[2:]:
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, p)
    return acc


def pairing_holds(left, right, secret=SECRET):
    """e(left, s_g2) = e(right, g2) with s_g2 = s g2, i.e. s left = right"""
    return g1_mul(left, secret) == right


def mont_to_point(limbs):
    """(8,) uint64 Montgomery limbs of an affine point -> integer pair, None for (0, 0)"""
    rinv = pow(1 << 256, -1, Q)
    v = [int(x) for x in limbs]
    x = sum(w << (64 * i) for i, w in enumerate(v[:4])) * rinv % Q
    y = sum(w << (64 * i) for i, w in enumerate(v[4:])) * rinv % Q
    return None if x == 0 and y == 0 else (x, y)


# ---- the SYSTEM of check_util.py
def system_cs():
    """fixed s, t; advice a, b (phase 0) and c (phase 1); instance p; challenge 0 drawn after phase 0"""
    return prover.ConstraintSystem(2, 3, 1, cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, cu.SYSTEM_PERM, advice_column_phase=[0, 0, 1], challenge_phase=[0])


def system_columns(seed, k, b, table=None):
    """check_util.system_witness with the selector cleared past row ACTIVE and the instance column zero past it: still satisfied (every
    gate is gated by s, the copies and the lookup do not read s).  table: the lookup table (fixed column 1) of an earlier call, for a
    second witness under the same fixed columns -- the advice cells are then drawn again from that table and the gates' c cells,
    the instance cells and the copies recomputed as system_witness computes them."""
    rng = random.Random(seed)
    cols = cu.system_witness(rng, k, b)
    n, u = 1 << k, (1 << k) - b - 1
    if table is not None:
        s, (a, bb, c), p = cols["fixed"][0], cols["advice"], cols["instance"][0]
        cols["fixed"][1] = list(table)
        for i in range(u):
            a[i] = rng.choice(table[:u])
        a[7], a[12], bb[4] = a[3], a[11], a[3]
        for i in range(1, u - 1):
            c[i - 1] = a[i] * bb[i + 1] % R_MOD
        for i in range(1, u - 1):
            p[i] = c[i]
        p[0] = a[1]
        bb[9] = p[5]
        c[7] = a[8] * bb[9] % R_MOD
        p[7] = c[7]
    cols["fixed"][0] = [1 if 1 <= i <= ACTIVE else 0 for i in range(n)]
    cols["instance"][0] = [v if i <= ACTIVE else 0 for i, v in enumerate(cols["instance"][0])]
    return cols


def instance_of(cols):
    return [cols["instance"][0][:ACTIVE + 1]]


PLACEHOLDER_CHALLENGES = (7, 11, 13)  # stand in for the transcript's challenges where columns are built without a proof


class System:
    """One constraint system of the proof tests.  cs: its prover.ConstraintSystem; copies: (column, row, column, row) over
    cs.permutation; k: the size it runs at; columns(seed, k, b, fixed, challenges): canonical-integer columns {"fixed", "advice",
    "instance"} of a witness that satisfies the system by construction -- fixed (None: drawn from the seed) holds the fixed columns of
    an earlier call, for another witness under the same key, challenges the cs.num_challenges challenge values the advice columns of
    later phases are computed from; instance_of(cols): the instance values create_proof and verify_proof take; n_instances: how many
    proof instances prove() makes by default."""

    def __init__(self, name, cs, copies, k, columns, instance_of, n_instances=1):
        self.name, self.cs, self.copies, self.k = name, cs, list(copies), k
        self.columns, self.instance_of, self.n_instances = columns, instance_of, n_instances


def _system_entry_columns(seed, k, b, fixed=None, challenges=None):
    return system_columns(seed, k, b, table=None if fixed is None else fixed[1])


def system_entry():
    """the SYSTEM of check_util.py (its columns do not depend on the challenge)"""
    return System("system", system_cs(), cu.SYSTEM_COPIES, 5, _system_entry_columns, instance_of)


class Setup:
    """params, proving key and verifying key of one system at one k (one fixed-column assignment serves every witness of the tests);
    system defaults to the SYSTEM of check_util.py, k to the system's own"""

    def __init__(self, k=None, seed=0xC0FFEE, system=None):
        self.system = system_entry() if system is None else system
        self.k = self.system.k if k is None else k
        self.n = 1 << self.k
        self.cs = self.system.cs
        self.b = self.cs.blinding_factors()
        self.u = self.n - self.b - 1
        self.seed = seed
        self.cols = self.columns(seed)
        self.params = h2.ParamsKZG.setup(self.k, SECRET)
        self.fixed = [to_mont(c) for c in self.cols["fixed"]]
        self.pk = prover.ProvingKey.build(self.params, self.cs, self.fixed, self.system.copies, VK_REPR)

    def columns(self, seed, challenges=None):
        """the witness of `seed` under this key's fixed columns (the key's own seed draws them), for the given challenges"""
        challenges = list(PLACEHOLDER_CHALLENGES[:self.cs.num_challenges]) if challenges is None else list(challenges)
        fixed = None if seed == self.seed else self.cols["fixed"]
        return self.system.columns(seed, self.k, self.b, fixed, challenges)

    def witness_of(self, seed):
        """a witness that follows the challenges it is handed: challenges -> columns"""
        return lambda challenges: self.columns(seed, challenges)

    def default_witnesses(self):
        return [self.witness_of(self.seed + i) for i in range(self.system.n_instances)]

    def witness_fn(self, columns_per_instance, resident):
        """create_proof's witness callback over canonical-integer advice columns (a dict of columns, or a function from the challenges
        to one): the advice columns of the phase in column order, fresh arrays (the prover consumes them), uploaded by the callback
        when resident.  A challenge is handed over exactly when its phase has passed."""
        cs = self.cs

        def witness(i, phase, challenges):
            assert [c is None for c in challenges] == [p >= phase for p in cs.challenge_phase]
            entry = columns_per_instance[i]
            cols = entry([0 if c is None else c for c in challenges]) if callable(entry) else entry
            out = [to_mont(cols["advice"][c]) for c, p in enumerate(cs.advice_column_phase) if p == phase]
            if resident:
                import torch
                out = [torch.from_numpy(a.view(np.int64)).cuda() for a in out]
            return out
        return witness

    def instances_of(self, columns_per_instance):
        """the instance values of each witness (they do not depend on the challenges)"""
        placeholder = list(PLACEHOLDER_CHALLENGES[:self.cs.num_challenges])
        return [self.system.instance_of(c(placeholder) if callable(c) else c) for c in columns_per_instance]

    def prove(self, columns_per_instance=None, multiopen="shplonk", form="parts", resident=True, seed=b"\x07" * 32, instances=None):
        columns_per_instance = self.default_witnesses() if columns_per_instance is None else columns_per_instance
        instances = self.instances_of(columns_per_instance) if instances is None else instances
        return prover.create_proof(self.params, self.pk, instances, self.witness_fn(columns_per_instance, resident), transcript.Blake2bWrite(),
                                   seed, multiopen=multiopen, form=form, resident=resident)

    def verify(self, proof_bytes, instances, multiopen="shplonk", vk=None):
        return verifier.verify_proof(self.params, self.pk.vk if vk is None else vk, instances, transcript.Blake2bRead(proof_bytes), multiopen)

    def accepts(self, proof_bytes, instances, multiopen="shplonk", vk=None):
        """False when verify_proof raises or the pairing equation fails"""
        try:
            left, right = self.verify(proof_bytes, instances, multiopen, vk)
        except (transcript.TranscriptError, verifier.VerifyError):
            return False
        return pairing_holds(left, right)
