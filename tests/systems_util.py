"""A family of constraint systems for the end-to-end proof tests: the SYSTEM of check_util.py and six more, each chosen for a shape the
SYSTEM does not have (test_constraint_system.py derives every number below by hand; test_proof_systems.py proves and verifies them).

  system    degree 4, chunk_len 2, two sets, one lookup, two phases                                          k = 5
  bare      one gate, no permutation column, no lookup, no instance column: degree 3, no set, two h pieces   k = 4
  sets3     three permutation sets of one column, a fixed column among them: fixed queries out of order      k = 4
  deg6      degree 6: chunk_len 4, five h pieces, a partial last set that holds the instance column alone    k = 4
  rot9      one advice column at nine rotations, fixed at +1, instance at -1: blinding_factors 11, u = 20    k = 5
  lookups2  two lookups (a two-expression tuple; a challenge in the input, a table of degree 2): degree 5,
            chunk_len 3, four h pieces, proved with two instances                                            k = 5
  phases3   three phases, three challenges: c = challenge_0 a + challenge_1 b, a gate times challenge_2       k = 4

Every gate is multiplied by a fixed selector that is zero on the rows >= u and on every row from which one of the gate's rotations
reaches a row >= u, so no gate reads a blinding row; the selectors stop a few rows earlier still, which leaves cells below u that no
gate reads for the copies the reject tests corrupt.  A witness is built in two steps: the fixed columns from the key's seed, then the
advice and instance columns from the witness's seed and those fixed columns, so that several witnesses share one key.

Each entry carries its proof's layout in 32-byte words, counted by hand in the reference's write order (plonk/prover.rs):
  points    advice commitments, permuted input/table pairs, permutation products, lookup products, the random polynomial, h pieces
  advice / fixed / 1 (random) / sigma / product / lookup   the evaluation sections, in this order
and the proof lengths: SHPLONK appends two points, GWC one witness per distinct opening point."""
import random

import check_util as cu
import proof_util as pu
from lookup_util import R_MOD
from proof_util import prover


def A(c, r=0):
    return ("advice", c, r)


def F(c, r=0):
    return ("fixed", c, r)


def I(c, r=0):  # noqa: E743
    return ("instance", c, r)


def mul(*es):
    out = es[0]
    for e in es[1:]:
        out = ("prod", out, e)
    return out


def add(*es):
    out = es[0]
    for e in es[1:]:
        out = ("sum", out, e)
    return out


def sub(x, y):
    return ("sum", x, ("neg", y))


def _sizes(k, b):
    return 1 << k, (1 << k) - b - 1


def _rngs(seed, n, counts):
    """the witness's generator and its columns filled with random values (the rows a gate, a copy or a lookup reads are set after)"""
    rng = random.Random(seed)
    return rng, [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(counts)]


def _fixed_rng(seed):
    return random.Random(seed ^ 0xF1ED)


def _inv(v):
    return pow(v, -1, R_MOD)


class Entry(pu.System):
    """a pu.System with its hand-counted proof layout: layout = {points, pieces, advice, fixed, sigma, product, lookup} in 32-byte
    words (for n_instances proof instances), shplonk_bytes / gwc_bytes the proof lengths"""

    def __init__(self, name, cs, copies, k, columns, instance_of, layout, shplonk_bytes, gwc_bytes, n_instances=1):
        pu.System.__init__(self, name, cs, copies, k, columns, instance_of, n_instances)
        self.layout, self.proof_bytes = layout, {"shplonk": shplonk_bytes, "gwc": gwc_bytes}

    def section(self, name):
        """(first word, words) of an evaluation section, or of the h commitments ("h"), from the hand layout"""
        lay = self.layout
        if name == "h":
            return lay["points"] - lay["pieces"], lay["pieces"]
        at = lay["points"]
        for key in ("advice", "fixed", "random", "sigma", "product", "lookup"):
            words = 1 if key == "random" else lay[key]
            if key == name:
                return at, words
            at += words
        raise KeyError(name)

    def evaluation_words(self):
        return self.section("lookup")[0] + self.layout["lookup"]


# ------------------------------------------------------------------ bare
BARE_GATES = [mul(F(0), A(0), sub(A(0), ("const", 1)))]                     # s a (a - 1)


def _bare_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        fixed = [[1 if i < u and i != 3 else 0 for i in range(n)]]
    rng, (a,) = _rngs(seed, n, 1)
    for i in range(u):
        if fixed[0][i]:
            a[i] = rng.randrange(2)
    return {"fixed": [list(c) for c in fixed], "advice": [a], "instance": []}


def bare():
    cs = prover.ConstraintSystem(1, 1, 0, BARE_GATES)
    return Entry("bare", cs, [], 4, _bare_columns, lambda cols: [],
                 dict(points=4, pieces=2, advice=1, fixed=1, sigma=0, product=0, lookup=0), 288, 256)


# ------------------------------------------------------------------ sets3
SETS3_GATES = [mul(F(0), sub(add(A(0), A(1)), A(1, 1)))]                    # s (a + b - b(+1))
SETS3_PERM = [("advice", 0), ("fixed", 1), ("advice", 1)]
# a[7] = a[8] (set 0 alone), f[3] = a[9] (sets 1 and 0), b[7] = b[8] (set 2 alone), f[5] = b[9] (sets 1 and 2), a[2] = f[6] (a cell the gate reads)
SETS3_COPIES = [(0, 7, 0, 8), (1, 3, 0, 9), (2, 7, 2, 8), (1, 5, 2, 9), (0, 2, 1, 6)]
GATE_ROWS = 6  # the selectors of the k = 4 systems are one on rows 0 .. 5; u = 10


def _sets3_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [[1 if i < GATE_ROWS else 0 for i in range(n)], [frng.randrange(R_MOD) for _ in range(n)]]
    f = fixed[1]
    rng, (a, bb) = _rngs(seed, n, 2)
    a[2], a[9], bb[9] = f[6], f[3], f[5]
    a[8], bb[8] = a[7], bb[7]
    for i in range(GATE_ROWS):
        bb[i + 1] = (a[i] + bb[i]) % R_MOD
    return {"fixed": [list(c) for c in fixed], "advice": [a, bb], "instance": []}


def sets3():
    cs = prover.ConstraintSystem(2, 2, 0, SETS3_GATES, permutation=SETS3_PERM)
    return Entry("sets3", cs, SETS3_COPIES, 4, _sets3_columns, lambda cols: [],
                 dict(points=8, pieces=2, advice=3, fixed=2, sigma=3, product=8, lookup=0), 864, 896)


# ------------------------------------------------------------------ deg6
DEG6_GATES = [mul(F(0), sub(mul(A(0), A(0), A(0), A(1), A(1)), A(2)))]      # s (a a a b b - c)
DEG6_PERM = [("advice", 0), ("advice", 1), ("advice", 2), ("fixed", 1), ("instance", 0)]
# c[1] = p[0], a[3] = b[4] (both read by the gate), t[2] = a[7], p[1] = c[8] (the instance copy the reject test breaks), b[6] = b[9]
DEG6_COPIES = [(2, 1, 4, 0), (0, 3, 1, 4), (3, 2, 0, 7), (4, 1, 2, 8), (1, 6, 1, 9)]
DEG6_INSTANCE_LEN = 2


def _deg6_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [[1 if i < GATE_ROWS else 0 for i in range(n)], [frng.randrange(R_MOD) for _ in range(n)]]
    rng, (a, bb, c, p) = _rngs(seed, n, 4)
    bb[4], a[7], bb[9] = a[3], fixed[1][2], bb[6]
    for i in range(GATE_ROWS):
        c[i] = pow(a[i], 3, R_MOD) * bb[i] * bb[i] % R_MOD
    p[0], c[8] = c[1], p[1]
    p = [v if i < DEG6_INSTANCE_LEN else 0 for i, v in enumerate(p)]
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c], "instance": [p]}


def deg6():
    cs = prover.ConstraintSystem(2, 3, 1, DEG6_GATES, permutation=DEG6_PERM)
    return Entry("deg6", cs, DEG6_COPIES, 4, _deg6_columns, lambda cols: [cols["instance"][0][:DEG6_INSTANCE_LEN]],
                 dict(points=11, pieces=5, advice=3, fixed=2, sigma=5, product=5, lookup=0), 928, 960)


# ------------------------------------------------------------------ rot9
# s (sum over r = -4 .. 4 of (r + 5) a(r)  -  f(+1) p(-1)): the weights tell the rotations apart
ROT9_GATES = [mul(F(0), sub(add(*[("scaled", A(0, r), r + 5) for r in range(-4, 5)]), mul(F(1, 1), I(0, -1))))]
ROT9_PERM = [("advice", 0)]
ROT9_COPIES = [(0, 2, 0, 17), (0, 5, 0, 18)]  # all four cells are read by the gate
ROT9_FIRST, ROT9_LAST = 4, 15                 # s is one on rows 4 .. 15: row - 4 >= 0 and row + 4 < u = 20
ROT9_INSTANCE_LEN = ROT9_LAST                 # p(-1) at rows 4 .. 15 reads p[3 .. 14]


def _rot9_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [[1 if ROT9_FIRST <= i <= ROT9_LAST else 0 for i in range(n)], [frng.randrange(1, R_MOD) for _ in range(n)]]
    f = fixed[1]
    rng, (a, p) = _rngs(seed, n, 2)
    a[17], a[18] = a[2], a[5]
    for i in range(ROT9_FIRST, ROT9_LAST + 1):
        p[i - 1] = sum((r + 5) * a[i + r] for r in range(-4, 5)) * _inv(f[i + 1]) % R_MOD
    p = [v if i < ROT9_INSTANCE_LEN else 0 for i, v in enumerate(p)]
    return {"fixed": [list(c) for c in fixed], "advice": [a], "instance": [p]}


def rot9():
    cs = prover.ConstraintSystem(2, 1, 1, ROT9_GATES, permutation=ROT9_PERM)
    return Entry("rot9", cs, ROT9_COPIES, 5, _rot9_columns, lambda cols: [cols["instance"][0][:ROT9_INSTANCE_LEN]],
                 dict(points=5, pieces=2, advice=9, fixed=2, sigma=1, product=2, lookup=0), 704, 928)


# ------------------------------------------------------------------ lookups2
# fixed 0 s, 1 q, 2 t0, 3 t1, 4 q2, 5 qt, 6 t2; advice 0 a, 1 b (phase 0), 2 c (phase 1); challenge 0 after phase 0
LOOKUPS2_GATES = [mul(F(0), sub(mul(A(0), A(1)), A(0, 1)))]                 # s (a b - a(+1))
LOOKUPS2_LOOKUPS = [([mul(F(1), A(0)), mul(F(1), A(1))], [F(2), F(3)]),     # (q a, q b) in (t0, t1)
                    ([add(A(2), mul(("challenge", 0), F(4)))], [mul(F(5), F(6))])]   # c + challenge_0 q2 in qt t2
LOOKUPS2_PERM = [("advice", 0), ("advice", 2)]
LOOKUPS2_COPIES = [(0, 10, 0, 12), (0, 9, 1, 20), (1, 6, 1, 7)]
LOOKUPS2_S_ROWS, LOOKUPS2_Q_ROWS = range(0, 5), range(8, 20)
LOOKUPS2_SHARED = 3  # t2[3] = t0[3] with qt[3] = 1: the value a[9] and c[20] share


def _lookups2_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        rnd = lambda: [frng.randrange(R_MOD) for _ in range(n)]  # noqa: E731
        s = [1 if i in LOOKUPS2_S_ROWS else 0 for i in range(n)]
        q = [1 if i in LOOKUPS2_Q_ROWS else 0 for i in range(n)]
        t0, t1, q2, t2 = rnd(), rnd(), rnd(), rnd()
        t0[0] = t1[0] = 0                                                   # the (0, 0) row the rows with q = 0 look up
        qt = [i % 2 for i in range(n)]
        qt[LOOKUPS2_SHARED], t2[LOOKUPS2_SHARED] = 1, t0[LOOKUPS2_SHARED]
        q2[20], q2[7] = 0, q2[6]
        fixed = [s, q, t0, t1, q2, qt, t2]
    s, q, t0, t1, q2, qt, t2 = fixed
    rng, (a, bb, c) = _rngs(seed, n, 3)
    pick = [rng.randrange(u) for _ in range(n)]       # row i of lookup 0 takes table row pick[i]
    pick2 = [rng.randrange(u) for _ in range(n)]      # row i of lookup 1 takes the value of table row pick2[i]
    pick[9], pick[12] = LOOKUPS2_SHARED, pick[10]
    pick2[20], pick2[7] = LOOKUPS2_SHARED, pick2[6]
    for i in LOOKUPS2_Q_ROWS:
        a[i], bb[i] = t0[pick[i]], t1[pick[i]]
    for i in LOOKUPS2_S_ROWS:
        a[i + 1] = a[i] * bb[i] % R_MOD
    ch0 = challenges[0]
    for i in range(u):
        c[i] = (qt[pick2[i]] * t2[pick2[i]] - ch0 * q2[i]) % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c], "instance": []}


def lookups2():
    cs = prover.ConstraintSystem(7, 3, 0, LOOKUPS2_GATES, LOOKUPS2_LOOKUPS, LOOKUPS2_PERM, advice_column_phase=[0, 0, 1], challenge_phase=[0])
    return Entry("lookups2", cs, LOOKUPS2_COPIES, 5, _lookups2_columns, lambda cols: [],
                 dict(points=25, pieces=4, advice=8, fixed=7, sigma=2, product=4, lookup=20), 2208, 2240, n_instances=2)


# ------------------------------------------------------------------ phases3
# fixed 0 s, 1 f; advice a (phase 0), b (phase 1), c (phase 2); challenge j after phase j
PHASES3_GATES = [mul(F(0), sub(A(2), add(mul(("challenge", 0), A(0)), mul(("challenge", 1), A(1))))),   # s (c - (challenge_0 a + challenge_1 b))
                 mul(mul(F(0), sub(mul(A(0), A(1)), F(1))), ("challenge", 2))]                          # (s (a b - f)) challenge_2
PHASES3_PERM = [("advice", 0), ("advice", 2)]
PHASES3_COPIES = [(0, 8, 0, 9), (0, 7, 1, 8), (1, 6, 1, 9)]  # cells no gate reads


def _phases3_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [[1 if i < GATE_ROWS else 0 for i in range(n)], [frng.randrange(R_MOD) for _ in range(n)]]
    f = fixed[1]
    rng, (a, bb, c) = _rngs(seed, n, 3)
    a = [v or 1 for v in a]
    a[9], c[8], c[9] = a[8], a[7], c[6]
    for i in range(GATE_ROWS):
        bb[i] = f[i] * _inv(a[i]) % R_MOD
        c[i] = (challenges[0] * a[i] + challenges[1] * bb[i]) % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c], "instance": []}


def phases3():
    cs = prover.ConstraintSystem(2, 3, 0, PHASES3_GATES, permutation=PHASES3_PERM, advice_column_phase=[0, 1, 2], challenge_phase=[0, 1, 2])
    return Entry("phases3", cs, PHASES3_COPIES, 4, _phases3_columns, lambda cols: [],
                 dict(points=8, pieces=2, advice=3, fixed=2, sigma=2, product=5, lookup=0), 736, 768)


# ------------------------------------------------------------------ the SYSTEM of check_util.py
def system():
    e = pu.system_entry()
    return Entry(e.name, e.cs, e.copies, e.k, e.columns, e.instance_of,
                 dict(points=12, pieces=3, advice=5, fixed=2, sigma=3, product=5, lookup=5), 1120, 1184)


FAMILY = {f.__name__: f for f in (system, bare, sets3, deg6, rot9, lookups2, phases3)}
NAMES = list(FAMILY)
_ENTRIES, _SETUPS = {}, {}


def entry(name):
    if name not in _ENTRIES:
        _ENTRIES[name] = FAMILY[name]()
    return _ENTRIES[name]


def setup(name):
    """the Setup (params, keys, first witness) of a system, built once per session"""
    if name not in _SETUPS:
        pu.h2.init()
        _SETUPS[name] = pu.Setup(system=entry(name))
    return _SETUPS[name]


def mapping_of(e):
    """the permutation assembly's mapping for the entry's copies (the host port of keygen.rs's Assembly)"""
    asm = pu.h2.PermutationAssembly(1 << e.k, len(e.cs.permutation))
    for c in e.copies:
        asm.copy(*c)
    return asm.mapping


def model_failures(e, cols, challenges, theta):
    """check_util.verify, the Python model of MockProver::verify, on the entry's system"""
    n, u = _sizes(e.k, e.cs.blinding_factors())
    return cu.verify(n, cols, list(challenges), e.cs.gates, e.cs.lookups, theta, u, e.cs.permutation, mapping_of(e))
