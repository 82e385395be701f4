"""Five more constraint systems for the end-to-end proof tests, each with a shuffle or an mv-lookup (logUp) argument -- the two
arguments systems_util.py's family lacks (test_constraint_system_args.py derives every number below by hand;
test_proof_arguments.py proves and verifies them).

  shuffle1   one shuffle of two-expression tuples, one gate, no permutation column, no halo2 lookup: the shuffle's
             {x, omega x} is the only rotation set beside {x}                                                                k = 4
  shuffles2  two shuffles: an input times a fixed selector (degree 4, chunk_len 2), a shuffle expression with a phase-0
             challenge (its advice column sits in phase 1); one permutation set; proved with two instances                   k = 4
  mv1        one mv-lookup with K = 1; the table repeats one value (the lowest row takes the count) and one value is hit
             by eight input rows; m is opened at x alone, phi at {x, omega x}                                                k = 5
  mv3        K = 3 input pairs share a two-expression table: degree 2 + 1 + 3 = 6, extended_k = k + 3, five pieces of h      k = 5
  all_args   a halo2 lookup, an mv-lookup (K = 2), a shuffle, two permutation sets, two phases, two instances: the member
             where stage, fold, evaluation and query order across the argument kinds can be wrong                            k = 5

The conventions are systems_util.py's: a gate's selector is one on rows 0 .. GATE_ROWS - 1 only, which leaves cells below u that no gate
reads; the fixed columns come from the key's seed, advice and instance from the witness's.  A shuffle or an mv-lookup reads every row
below u, so its columns are filled there: shuffle side row i holds input row PERM(i), an mv input row holds a table row's value.

Each entry carries its proof's layout in 32-byte words, in the write order of prover.py's docstring:
  points    advice commitments, permuted input/table pairs, m, permutation products, lookup products, phi, shuffle products, the random
            polynomial, h pieces
  advice / fixed / 1 (random) / sigma / product / lookup / mvlookup / shuffle   the evaluation sections, in this order"""
import check_util as cu
import lookup_util as lu
import systems_util as fam
from shuffle_util import failing_rows
from systems_util import A, F, GATE_ROWS, R_MOD, _fixed_rng, _rngs, _sizes, add, mul, prover, pu, sub

CH0 = ("challenge", 0)


def perm1(i, u):
    """shuffle side row i holds input row 3 i + 1 mod u (u = 10 or 26: not a multiple of 3)"""
    return (3 * i + 1) % u


def perm2(i, u):
    """7 i + 3 mod u (u = 10 or 26: not a multiple of 7)"""
    return (7 * i + 3) % u


class Entry(fam.Entry):
    """systems_util.Entry with the two later evaluation sections in its layout"""
    SECTIONS = ("advice", "fixed", "random", "sigma", "product", "lookup", "mvlookup", "shuffle")

    def section(self, name):
        lay = self.layout
        if name == "h":
            return lay["points"] - lay["pieces"], lay["pieces"]
        at = lay["points"]
        for key in self.SECTIONS:
            words = 1 if key == "random" else lay[key]
            if key == name:
                return at, words
            at += words
        raise KeyError(name)

    def evaluation_words(self):
        return self.section("shuffle")[0] + self.layout["shuffle"]


def _selector(n):
    return [1 if i < GATE_ROWS else 0 for i in range(n)]


# ------------------------------------------------------------------ shuffle1
# fixed s; advice a, b, c, d; gate s (b - a a); the shuffle (a, b) <-> (c, d)
SHUFFLE1_GATES = [mul(F(0), sub(A(1), mul(A(0), A(0))))]
SHUFFLE1_SHUFFLES = [([A(0), A(1)], [A(2), A(3)])]


def _shuffle1_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        fixed = [_selector(n)]
    rng, (a, bb, c, d) = _rngs(seed, n, 4)
    for i in range(GATE_ROWS):
        bb[i] = a[i] * a[i] % R_MOD
    for i in range(u):
        c[i], d[i] = a[perm1(i, u)], bb[perm1(i, u)]
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c, d], "instance": []}


def shuffle1():
    cs = prover.ConstraintSystem(1, 4, 0, SHUFFLE1_GATES, shuffles=SHUFFLE1_SHUFFLES)
    return Entry("shuffle1", cs, [], 4, _shuffle1_columns, lambda cols: [],
                 dict(points=8, pieces=2, advice=4, fixed=1, sigma=0, product=0, lookup=0, mvlookup=0, shuffle=2), 576, 576)


# ------------------------------------------------------------------ shuffles2
# fixed s, q; advice a, b, c (phase 0), d (phase 1); challenge 0 after phase 0; gate s (a - b b);
# shuffle 0: q a <-> c (perm1); shuffle 1: b <-> d + challenge_0 q (perm2); permutation over a, d
SHUFFLES2_GATES = [mul(F(0), sub(A(0), mul(A(1), A(1))))]
SHUFFLES2_SHUFFLES = [([mul(F(1), A(0))], [A(2)]), ([A(1)], [add(A(3), mul(CH0, F(1)))])]
SHUFFLES2_PERM = [("advice", 0), ("advice", 3)]
# a[7] = a[8]; d[6] = d[8] (q is zero there, so b[perm2(6)] = b[5] equals b[perm2(8)] = b[9]); a[9] = d[7] = b[perm2(7)] = b[2]
SHUFFLES2_COPIES = [(0, 7, 0, 8), (1, 6, 1, 8), (0, 9, 1, 7)]


def _shuffles2_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    assert u == 10
    if fixed is None:
        fixed = [_selector(n), _selector(n)]
    q = fixed[1]
    rng, (a, bb, c, d) = _rngs(seed, n, 4)
    for i in range(GATE_ROWS):
        a[i] = bb[i] * bb[i] % R_MOD
    a[8], bb[9], a[9] = a[7], bb[5], bb[2]
    for i in range(u):
        c[i] = q[perm1(i, u)] * a[perm1(i, u)] % R_MOD
        d[i] = (bb[perm2(i, u)] - challenges[0] * q[i]) % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c, d], "instance": []}


def shuffles2():
    cs = prover.ConstraintSystem(2, 4, 0, SHUFFLES2_GATES, permutation=SHUFFLES2_PERM, advice_column_phase=[0, 0, 0, 1], challenge_phase=[0],
                                 shuffles=SHUFFLES2_SHUFFLES)
    return Entry("shuffles2", cs, SHUFFLES2_COPIES, 4, _shuffles2_columns, lambda cols: [],
                 dict(points=18, pieces=3, advice=8, fixed=2, sigma=2, product=4, lookup=0, mvlookup=0, shuffle=8), 1440, 1440, n_instances=2)


# ------------------------------------------------------------------ mv1
# fixed s, t; advice a, b; gate s (b - a a); the mv-lookup [a] in [t]
MV1_GATES = [mul(F(0), sub(A(1), mul(A(0), A(0))))]
MV1_MV = [([[A(0)]], [F(1)])]
MV1_REPEAT = (2, 5)          # t[5] = t[2]: the count of that value goes to row 2
MV1_MANY = (7, range(10, 18))  # a[10 .. 17] = t[7]


def _mv1_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        t = [frng.randrange(R_MOD) for _ in range(n)]
        t[MV1_REPEAT[1]] = t[MV1_REPEAT[0]]
        fixed = [_selector(n), t]
    t = fixed[1]
    rng, (a, bb) = _rngs(seed, n, 2)
    for i in range(u):
        a[i] = t[rng.randrange(u)]
    a[3], a[20] = t[MV1_REPEAT[1]], t[MV1_REPEAT[0]]
    for i in MV1_MANY[1]:
        a[i] = t[MV1_MANY[0]]
    for i in range(GATE_ROWS):
        bb[i] = a[i] * a[i] % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb], "instance": []}


def mv1():
    cs = prover.ConstraintSystem(2, 2, 0, MV1_GATES, mv_lookups=MV1_MV)
    return Entry("mv1", cs, [], 5, _mv1_columns, lambda cols: [],
                 dict(points=8, pieces=3, advice=2, fixed=2, sigma=0, product=0, lookup=0, mvlookup=3, shuffle=0), 576, 576)


# ------------------------------------------------------------------ mv3
# fixed s, t0, t1; advice a0, b0, a1, b1, a2, b2, e; gate s (e - a0 b0); the mv-lookup (a0, b0), (a1, b1), (a2, b2) in (t0, t1)
MV3_GATES = [mul(F(0), sub(A(6), mul(A(0), A(1))))]
MV3_MV = [([[A(0), A(1)], [A(2), A(3)], [A(4), A(5)]], [F(1), F(2)])]


def _mv3_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [_selector(n), [frng.randrange(R_MOD) for _ in range(n)], [frng.randrange(R_MOD) for _ in range(n)]]
    _, t0, t1 = fixed
    rng, advice = _rngs(seed, n, 7)
    for c in range(3):
        for i in range(u):
            row = rng.randrange(u)
            advice[2 * c][i], advice[2 * c + 1][i] = t0[row], t1[row]
    for i in range(GATE_ROWS):
        advice[6][i] = advice[0][i] * advice[1][i] % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": advice, "instance": []}


def mv3():
    cs = prover.ConstraintSystem(3, 7, 0, MV3_GATES, mv_lookups=MV3_MV)
    return Entry("mv3", cs, [], 5, _mv3_columns, lambda cols: [],
                 dict(points=15, pieces=5, advice=7, fixed=3, sigma=0, product=0, lookup=0, mvlookup=3, shuffle=0), 992, 992)


# ------------------------------------------------------------------ all_args
# fixed s, t, tm; advice a, b, c, d (phase 0), e (phase 1), f (phase 0); challenge 0 after phase 0; gate s (f - a b);
# halo2 lookup [a] in [t]; mv-lookup [b], [c] in [tm]; shuffle d <-> e + challenge_0 s (perm1); permutation over a, d, f, tm
ALL_GATES = [mul(F(0), sub(A(5), mul(A(0), A(1))))]
ALL_LOOKUPS = [([A(0)], [F(1)])]
ALL_MV = [([[A(1)], [A(2)]], [F(2)])]
ALL_SHUFFLES = [([A(3)], [add(A(4), mul(CH0, F(0)))])]
ALL_PERM = [("advice", 0), ("advice", 3), ("advice", 5), ("fixed", 2)]
# a[20] = a[21] (set 0 alone), d[7] = f[8] (set 0, two columns), tm[3] = d[9] (sets 1 and 0)
ALL_COPIES = [(0, 20, 0, 21), (1, 7, 2, 8), (3, 3, 1, 9)]


def _all_args_columns(seed, k, b, fixed=None, challenges=None):
    n, u = _sizes(k, b)
    if fixed is None:
        frng = _fixed_rng(seed)
        fixed = [_selector(n), [frng.randrange(R_MOD) for _ in range(n)], [frng.randrange(R_MOD) for _ in range(n)]]
    s, t, tm = fixed
    rng, (a, bb, c, d, e, f) = _rngs(seed, n, 6)
    for i in range(u):
        a[i], bb[i], c[i] = t[rng.randrange(u)], tm[rng.randrange(u)], tm[rng.randrange(u)]
    a[21] = a[20]
    for i in range(GATE_ROWS):
        f[i] = a[i] * bb[i] % R_MOD
    f[8], d[9] = d[7], tm[3]
    for i in range(u):
        e[i] = (d[perm1(i, u)] - challenges[0] * s[i]) % R_MOD
    return {"fixed": [list(col) for col in fixed], "advice": [a, bb, c, d, e, f], "instance": []}


def all_args():
    cs = prover.ConstraintSystem(3, 6, 0, ALL_GATES, ALL_LOOKUPS, ALL_PERM, advice_column_phase=[0, 0, 0, 0, 1, 0], challenge_phase=[0],
                                 shuffles=ALL_SHUFFLES, mv_lookups=ALL_MV)
    return Entry("all_args", cs, ALL_COPIES, 5, _all_args_columns, lambda cols: [],
                 dict(points=33, pieces=4, advice=12, fixed=3, sigma=4, product=10, lookup=10, mvlookup=6, shuffle=4), 2720, 2784, n_instances=2)


FAMILY = {f.__name__: f for f in (shuffle1, shuffles2, mv1, mv3, all_args)}
NAMES = list(FAMILY)
_ENTRIES, _SETUPS = {}, {}


def entry(name):
    if name not in _ENTRIES:
        _ENTRIES[name] = FAMILY[name]()
    return _ENTRIES[name]


def setup(name, k=None):
    """the Setup (params, keys, first witness) of a member, built once per session and k"""
    if (name, k) not in _SETUPS:
        pu.h2.init()
        _SETUPS[(name, k)] = pu.Setup(k=k, system=entry(name))
    return _SETUPS[(name, k)]


def compressed(exprs, theta, n, cols, challenges):
    return lu.compress(exprs, theta, n, cols, challenges)


def model_failures(e, cols, challenges, theta):
    """the Python model of verify_witness on the entry's system: check_util.verify's gates and lookups, then ("shuffle", j, row) for
    the input rows whose value the two sides hold a different number of times, then ("mvlookup", input, row) for the input rows whose
    value the table lacks (the input tuples counted over all arguments), then the permutation"""
    cs = e.cs
    n, u = _sizes(e.k, cs.blinding_factors())
    out = cu.verify(n, cols, list(challenges), cs.gates, cs.lookups, theta, u, cs.permutation, fam.mapping_of(e))
    perm = [f for f in out if f[0] == "permutation"]
    out = [f for f in out if f[0] != "permutation"]
    comp = lambda exprs: compressed(exprs, theta, n, cols, list(challenges))  # noqa: E731
    for j, (inp, shf) in enumerate(cs.shuffles):
        out += [("shuffle", j, r) for r in failing_rows(comp(inp), comp(shf), cs.blinding_factors())]
    pairs = [(comp(inp), comp(tab)) for inputs, tab in cs.mv_lookups for inp in inputs]
    fails = cu.lookup_failures([p[0] for p in pairs], [p[1] for p in pairs], u)
    out += [("mvlookup", j, r) for j, rows in enumerate(fails) for r in rows]
    return out + perm
