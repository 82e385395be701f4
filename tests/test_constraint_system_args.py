"""prover.ConstraintSystem with shuffle and mv-lookup (logUp) arguments, on the five systems of systems_args_util.py: degree,
blinding_factors, chunk_len, the permutation sets, the pieces of h, the three query lists and the proof layout against values worked out
by hand (each test's docstring derives them), and the verifier's two expression builders row by row against the integer models of
shuffle_util.py and mvlookup_util.py.  No GPU.

Query registration continues the order of test_constraint_system.py: enable_equality, gates, halo2 lookups, then the mv-lookups
(argument by argument: input tuples in order, then the table), then the shuffles (inputs, then shuffle expressions).
required_degree is 2 + max degree for a shuffle and 2 + d_t + sum_c d_c for an mv-lookup (include/halo2hip.h)."""
import pytest

import mvlookup_util as mv
import proof_util as pu
import shuffle_util as sh
import systems_args_util as fa
import systems_util as fam
from lookup_util import R_MOD
from proof_util import prover, verifier
from test_constraint_system import FAMILY_HAND as PARENT_HAND
from test_constraint_system import FAMILY_PROOF_HAND as PARENT_PROOF_HAND

A, F = fam.A, fam.F

# name: (degree, blinding_factors, chunk_len, sets, phases, advice queries, fixed queries, instance queries)
ARGS_HAND = {
    "shuffle1": (3, 5, 1, 0, [0], [(1, 0), (0, 0), (2, 0), (3, 0)], [(0, 0)], []),
    "shuffles2": (4, 5, 2, 1, [0, 1], [(0, 0), (3, 0), (1, 0), (2, 0)], [(0, 0), (1, 0)], []),
    "mv1": (4, 5, 2, 0, [0], [(1, 0), (0, 0)], [(0, 0), (1, 0)], []),
    "mv3": (6, 5, 4, 0, [0], [(6, 0), (0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0)], [(0, 0), (1, 0), (2, 0)], []),
    "all_args": (5, 5, 3, 2, [0, 1], [(0, 0), (3, 0), (5, 0), (1, 0), (2, 0), (4, 0)], [(2, 0), (0, 0), (1, 0)], []),
}
# name: (proof instances, h pieces, SHPLONK bytes, GWC bytes, distinct opening points)
ARGS_PROOF_HAND = {
    "shuffle1": (1, 2, 576, 576, 2),
    "shuffles2": (2, 3, 1440, 1440, 2),
    "mv1": (1, 3, 576, 576, 2),
    "mv3": (1, 5, 992, 992, 2),
    "all_args": (2, 4, 2720, 2784, 4),
}


def _check_hand(name):
    assert set(fa.NAMES) == set(ARGS_HAND)
    cs = fa.entry(name).cs
    degree, blinding, chunk_len, sets, phases, advice_q, fixed_q, instance_q = ARGS_HAND[name]
    assert cs.degree() == degree
    assert cs.blinding_factors() == blinding
    assert cs.chunk_len() == chunk_len
    assert cs.num_permutation_sets() == sets
    assert list(cs.phases()) == phases
    assert cs.advice_queries == advice_q
    assert cs.fixed_queries == fixed_q
    assert cs.instance_queries == instance_q


def test_args_shuffle1():
    """fixed s; advice a, b, c, d; gate s (b - a a): degree 3; the shuffle (a, b) <-> (c, d): 2 + 1 = 3; the permutation's 3 (without
    columns).  Degree 3, chunk_len 1, no set, two pieces of h.  Queries: s@0, b@0, a@0 from the gate read left to right, then the
    shuffle's inputs (a, b again) and its shuffle side c@0, d@0.  One query a column: blinding_factors = 5."""
    _check_hand("shuffle1")


def test_args_shuffles2():
    """fixed s, q; advice a, b, c (phase 0), d (phase 1); challenge 0.  Gate s (a - b b): 3.  Shuffle 0 (q a) <-> (c): 2 + 2 = 4;
    shuffle 1 (b) <-> (d + challenge_0 q): 2 + 1 = 3 (the challenge has degree 0).  Degree 4, chunk_len 2, the two permutation columns
    a, d make one set; three pieces of h.  Queries: a@0, d@0 (enable_equality), s@0, b@0 (gate), q@0, c@0 (shuffle 0); shuffle 1 asks
    nothing new.  blinding_factors = 5; phases 0 and 1."""
    _check_hand("shuffles2")


def test_args_mv1():
    """fixed s, t; advice a, b; gate s (b - a a): 3; the mv-lookup [a] in [t]: 2 + 1 + 1 = 4.  Degree 4, chunk_len 2, no permutation
    column so no set; three pieces of h.  Queries: s@0, b@0, a@0 (gate), t@0 (the table).  blinding_factors = 5."""
    _check_hand("mv1")


def test_args_mv3():
    """fixed s, t0, t1; advice a0, b0, a1, b1, a2, b2, e; gate s (e - a0 b0): 3; the mv-lookup (a0, b0), (a1, b1), (a2, b2) in (t0, t1):
    2 + 1 + (1 + 1 + 1) = 6.  Degree 6, chunk_len 4, no set, five pieces of h (extended_k = k + 3).  Queries: s@0, e@0, a0@0, b0@0
    (gate), then the input tuples in order add a1, b1, a2, b2, then the table t0@0, t1@0.  blinding_factors = 5."""
    _check_hand("mv3")
    e = fa.entry("mv3")
    assert pu.h2.EvaluationDomain.new(e.cs.degree(), e.k).extended_k == e.k + 3


def test_args_all_args():
    """fixed s, t, tm; advice a, b, c, d (phase 0), e (phase 1), f (phase 0); challenge 0.  Gate s (f - a b): 3; halo2 lookup [a] in
    [t]: max(4, 2 + 1 + 1) = 4; mv-lookup [b], [c] in [tm]: 2 + 1 + 2 = 5; shuffle (d) <-> (e + challenge_0 s): 3.  Degree 5, chunk_len 3,
    the four permutation columns a, d, f, tm make two sets; four pieces of h.  Queries: a@0, d@0, f@0, tm@0 (enable_equality: the fixed
    list starts with column 2), s@0, b@0 (gate), t@0 (lookup), c@0 (mv-lookup), e@0 (shuffle).  blinding_factors = 5."""
    _check_hand("all_args")
    cs = fa.entry("all_args").cs
    assert cs.query_index("fixed", 2, 0) == 0 and cs.query_index("advice", 4, 0) == 5


@pytest.mark.parametrize("name", sorted(ARGS_PROOF_HAND))
def test_args_proof_lengths(name):
    """The proof in the write order of prover.py's docstring, 32 bytes per point and scalar, N proof instances:
      points   N (advice columns + 2 lookups + mv-lookups (m) + sets + lookups + mv-lookups (phi) + shuffles) + 1 (random) + (degree - 1)
      scalars  N advice queries, fixed queries, 1 (random), permutation columns, N (3 sets - 1), N 5 lookups, N 3 mv-lookups, N 2 shuffles
      opening  SHPLONK: 2 points; GWC: one witness per distinct opening point
    shuffle1   points 4 + 1 + 1 + 2 = 8; scalars 4 + 1 + 1 + 2 = 8; points {x, omega x (z alone)}
    shuffles2  points 2 (4 + 1 + 2) + 1 + 3 = 18; scalars 8 + 2 + 1 + 2 + 2 (3 - 1) + 2 (2 2) = 25; points {x, omega x}: one set has no x_last
    mv1        points 2 + 1 + 1 + 1 + 3 = 8; scalars 2 + 2 + 1 + 3 = 8; points {x, omega x (phi alone)}
    mv3        points 7 + 1 + 1 + 1 + 5 = 15; scalars 7 + 3 + 1 + 3 = 14; points {x, omega x}
    all_args   points 2 (6 + 2 + 1 + 2 + 1 + 1 + 1) + 1 + 4 = 33; scalars 12 + 3 + 1 + 4 + 2 (6 - 1) + 2 5 + 2 3 + 2 2 = 50;
               points {x, omega x, omega^-1 x (A'), omega^-6 x (z of set 0)}"""
    e = fa.entry(name)
    n_instances, pieces, shplonk, gwc, open_points = ARGS_PROOF_HAND[name]
    assert e.n_instances == n_instances and e.layout["pieces"] == pieces == e.cs.degree() - 1
    assert e.proof_bytes == {"shplonk": shplonk, "gwc": gwc}
    words = e.evaluation_words()
    assert 32 * (words + 2) == shplonk and 32 * (words + open_points) == gwc
    cs, lay = e.cs, e.layout
    sets, lookups, mvs, shuffles = cs.num_permutation_sets(), len(cs.lookups), len(cs.mv_lookups), len(cs.shuffles)
    assert lay["points"] == n_instances * (cs.num_advice_columns + 3 * lookups + 2 * mvs + sets + shuffles) + 1 + pieces
    assert lay["advice"] == n_instances * len(cs.advice_queries) and lay["fixed"] == len(cs.fixed_queries)
    assert lay["sigma"] == len(cs.permutation) and lay["product"] == n_instances * max(0, 3 * sets - 1) and lay["lookup"] == 5 * n_instances * lookups
    assert lay["mvlookup"] == 3 * n_instances * mvs and lay["shuffle"] == 2 * n_instances * shuffles
    assert e.section("h") == (lay["points"] - pieces, pieces) and e.section("advice")[0] == lay["points"]
    assert e.section("shuffle")[0] == e.section("mvlookup")[0] + lay["mvlookup"] == e.section("lookup")[0] + lay["lookup"] + lay["mvlookup"]


@pytest.mark.parametrize("name", sorted(PARENT_HAND))
def test_parent_family_is_unchanged(name):
    """the seven systems of systems_util.py, rebuilt through the constructor with both new arguments given (empty), derive the numbers
    test_constraint_system.py pins"""
    old = fam.entry(name).cs
    cs = prover.ConstraintSystem(old.num_fixed_columns, old.num_advice_columns, old.num_instance_columns, old.gates, old.lookups, old.permutation,
                                 advice_column_phase=old.advice_column_phase, challenge_phase=old.challenge_phase,
                                 minimum_degree=old.minimum_degree, shuffles=[], mv_lookups=[])
    assert old.shuffles == [] and old.mv_lookups == []
    degree, blinding, chunk_len, sets, phases, advice_q, fixed_q, instance_q = PARENT_HAND[name]
    for c in (old, cs):
        assert (c.degree(), c.blinding_factors(), c.chunk_len(), c.num_permutation_sets(), list(c.phases())) == (degree, blinding, chunk_len, sets, phases)
        assert (c.advice_queries, c.fixed_queries, c.instance_queries) == (advice_q, fixed_q, instance_q)
        assert c.degree() - 1 == PARENT_PROOF_HAND[name][1]


def test_degree_follows_the_new_arguments():
    cube = fam.mul(A(0), A(0), A(0))
    assert prover.ConstraintSystem(0, 2, 0, [], shuffles=[([A(0)], [A(1)])]).degree() == 3
    assert prover.ConstraintSystem(0, 2, 0, [], shuffles=[([A(0)], [cube])]).degree() == 5                       # 2 + 3
    assert prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[A(0)]], [A(1)])]).degree() == 4                   # 2 + 1 + 1
    assert prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[cube], [A(0)]], [fam.mul(A(1), A(1))])]).degree() == 8   # 2 + 2 + (3 + 1)
    # a rotation only an argument asks for counts towards blinding_factors
    rot = [A(0, r) for r in range(-2, 3)]
    assert prover.ConstraintSystem(0, 2, 0, [], shuffles=[(rot, [A(1)] * 5)]).blinding_factors() == 7
    assert prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([rot], [A(1)] * 5)]).blinding_factors() == 7
    # mv-lookups register before shuffles, whatever the keyword order
    cs = prover.ConstraintSystem(1, 3, 0, [], shuffles=[([A(2)], [A(0)])], mv_lookups=[([[A(1)]], [F(0)])])
    assert cs.advice_queries == [(1, 0), (2, 0), (0, 0)]


def test_new_arguments_are_checked():
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], shuffles=[([A(0), A(1)], [A(1)])])                 # unequal sides
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], shuffles=[([], [])])                               # an empty tuple
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([], [A(1)])])                         # K = 0
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[A(0)], [A(0), A(1)]], [A(1)])])     # a tuple longer than the table
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[]], [])])                           # an empty table
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[A(0)]] * 256, [A(1)])])             # K = 256
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], shuffles=[([A(2)], [A(0)])])                       # a column the system lacks
    assert len(prover.ConstraintSystem(0, 2, 0, [], mv_lookups=[([[A(0)]] * 255, [A(1)])]).mv_lookups[0][0]) == 255


@pytest.mark.parametrize("name", sorted(ARGS_HAND))
def test_args_witness_satisfies_the_model(name):
    """the witness of the key's seed, and a second one under the same fixed columns, satisfy the Python model; every copy lies below u"""
    e = fa.entry(name)
    b = e.cs.blinding_factors()
    u = (1 << e.k) - b - 1
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:e.cs.num_challenges])
    first = e.columns(0xC0FFEE, e.k, b, None, challenges)
    second = e.columns(0xC0FFEF, e.k, b, first["fixed"], challenges)
    assert second["fixed"] == first["fixed"] and second["advice"] != first["advice"]
    for cols in (first, second):
        assert fa.model_failures(e, cols, challenges, 5) == []
    assert all(r0 < u and r1 < u for _, r0, _, r1 in e.copies)
    if e.cs.num_challenges:  # the phase-1 column follows the challenge: a witness made for another one fails its shuffle
        other = [c + 1 for c in challenges]
        bad = fa.model_failures(e, e.columns(0xC0FFEE, e.k, b, None, other), challenges, 5)
        assert bad and all(f[0] in ("shuffle", "permutation") for f in bad)
    if name == "mv1":  # the shapes the member is there for
        t, a = first["fixed"][1], first["advice"][0]
        m, missing = mv.multiplicities([a], t, b)
        lo, hi = fa.MV1_REPEAT
        assert t[lo] == t[hi] and m[hi] == 0 and m[lo] == sum(1 for v in a[:u] if v == t[lo]) >= 2 and missing == [False]
        assert m[fa.MV1_MANY[0]] >= len(fa.MV1_MANY[1]) == 8 and sum(m) == u


# ------------------------------------------------------------------ the verifier's expression builders, row by row
THETA, BETA, GAMMA = 0x1234567, 0x89ABCDEF01, 0x23456789AB


def _rows(e, cols, challenges):
    """the row values the builders take: l0, l_last, l_active as indicator columns, and the compressed columns of every argument"""
    n, b = 1 << e.k, e.cs.blinding_factors()
    u = n - b - 1
    units = ([1 if i == 0 else 0 for i in range(n)], [1 if i == u else 0 for i in range(n)], [1 if i < u else 0 for i in range(n)])
    c = sh.Columns(cols["fixed"], cols["advice"], cols["instance"], challenges, n)
    shuffles = [(sh.compress_column(inp, THETA, c), sh.compress_column(shf, THETA, c)) for inp, shf in e.cs.shuffles]
    mvs = [([sh.compress_column(inp, THETA, c) for inp in inputs], sh.compress_column(tab, THETA, c)) for inputs, tab in e.cs.mv_lookups]
    return n, b, units, shuffles, mvs


def _nonzero_rows(e, cols, challenges, z_cols, mphi_cols):
    """{("shuffle" | "mvlookup", j): rows at which one of the argument's three expressions is not zero}"""
    n, b, (l0, l_last, l_active), shuffles, mvs = _rows(e, cols, challenges)
    out = {}
    for j, ((a, s), z) in enumerate(zip(shuffles, z_cols)):
        out[("shuffle", j)] = [i for i in range(n) if any(
            verifier.shuffle_expressions(l0[i], l_last[i], l_active[i], GAMMA, a[i], s[i], z[i], z[(i + 1) % n]))]
    for j, ((f, t), (m, phi)) in enumerate(zip(mvs, mphi_cols)):
        out[("mvlookup", j)] = [i for i in range(n) if any(
            verifier.mvlookup_expressions(l0[i], l_last[i], l_active[i], BETA, [col[i] for col in f], t[i], phi[i], phi[(i + 1) % n], m[i]))]
    return out


def _model_columns(e, cols, challenges):
    """z per shuffle and (m, phi) per mv-lookup from the integer models, blinding rows included"""
    n, b, _, shuffles, mvs = _rows(e, cols, challenges)
    z_cols = [sh.shuffle_product(a, s, GAMMA, [1000 + 7 * j + r for r in range(b)], b) for j, (a, s) in enumerate(shuffles)]
    mphi = []
    for j, (f, t) in enumerate(mvs):
        m, missing = mv.multiplicities(f, t, b)
        assert not any(missing)
        mphi.append((m, mv.grand_sum(f, t, m, BETA, [2000 + 5 * j + r for r in range(b)], b)))
    return z_cols, mphi


@pytest.mark.parametrize("name", ["shuffle1", "mv1", "all_args"])
def test_expression_builders_on_rows(name):
    """z, m and phi of the integer models put into the verifier's builders with the row values of l0 / l_last / l_active (indicators
    of row 0, row u, rows below u) and the next row in place of omega x: all three expressions of every argument are zero at every row
    of a satisfied witness -- z ends in one and phi in zero at row u, the blinding rows are read under no indicator -- and after one
    cell of one side changes (z, m, phi kept), only that row's active expression is not."""
    e = fa.entry(name)
    b = e.cs.blinding_factors()
    u = (1 << e.k) - b - 1
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:e.cs.num_challenges])
    cols = e.columns(0xC0FFEE, e.k, b, None, challenges)
    z_cols, mphi = _model_columns(e, cols, challenges)
    assert all(z[u] == 1 and z[0] == 1 and len(z) == 1 << e.k for z in z_cols)
    assert all(phi[u] == 0 and phi[0] == 0 and any(phi[1:u]) for _, phi in mphi)
    clean = _nonzero_rows(e, cols, challenges, z_cols, mphi)
    assert len(clean) == len(e.cs.shuffles) + len(e.cs.mv_lookups) >= 1 and all(rows == [] for rows in clean.values())
    # one corrupted cell per argument: (column, row) -> the argument whose active expression must fail there
    cells = {"shuffle1": [(("advice", 3, 4), ("shuffle", 0))], "mv1": [(("advice", 0, 11), ("mvlookup", 0))],
             "all_args": [(("advice", 4, 12), ("shuffle", 0)), (("advice", 2, 15), ("mvlookup", 0))]}[name]
    for (kind, column, row), argument in cells:
        bad = {key: [list(c) for c in val] for key, val in cols.items()}
        bad[kind][column][row] = (bad[kind][column][row] + 1) % R_MOD
        got = _nonzero_rows(e, bad, challenges, z_cols, mphi)
        assert got[argument] == [row], (kind, column, row)
        assert all(rows == [] for key, rows in got.items() if key != argument)


def test_expression_builders_tell_their_terms_apart():
    """each builder returns l0's, l_last's and l_active's expression, in the fold order of include/halo2hip.h"""
    z, zn, a, s = 11, 13, 17, 19
    assert verifier.shuffle_expressions(1, 0, 0, GAMMA, a, s, z, zn) == [(1 - z) % R_MOD, 0, 0]
    assert verifier.shuffle_expressions(0, 1, 0, GAMMA, a, s, z, zn) == [0, z * z - z, 0]
    assert verifier.shuffle_expressions(0, 0, 1, GAMMA, a, s, z, zn) == [0, 0, (zn * (s + GAMMA) - z * (a + GAMMA)) % R_MOD]
    phi, phin, m, t, f = 23, 29, 3, 31, [37, 41, 43]
    assert verifier.mvlookup_expressions(1, 0, 0, BETA, f, t, phi, phin, m) == [phi, 0, 0]
    assert verifier.mvlookup_expressions(0, 1, 0, BETA, f, t, phi, phin, m) == [0, phi, 0]
    fb, tau = [(v + BETA) % R_MOD for v in f], (t + BETA) % R_MOD
    P = fb[0] * fb[1] * fb[2] % R_MOD
    Qs = (fb[1] * fb[2] + fb[0] * fb[2] + fb[0] * fb[1]) % R_MOD
    assert verifier.mvlookup_expressions(0, 0, 1, BETA, f, t, phi, phin, m) == [0, 0, (tau * P * (phin - phi) - tau * Qs + m * P) % R_MOD]
    assert verifier.compress_evals([5, 7, 9], THETA) == ((5 * THETA + 7) * THETA + 9) % R_MOD
