"""prover.ConstraintSystem on the SYSTEM of check_util.py: degree, blinding_factors, chunk_len, the permutation sets and the query lists
against values worked out by hand from plonk/circuit.rs, and the intermediate sets of both multiopen schemes on a hand-made query list.
No GPU.

The SYSTEM: fixed s, t; advice a, b, c; instance p; challenge 0.
  gate 0   s (a b(+1) - c(-1))            degree 3
  gate 1   (s (c - p)) challenge_0        degree 2
  gate 2   the zero polynomial            degree 0
  lookup   [a] in [t]                     required_degree max(4, 2 + 1 + 1) = 4
  permutation over a, b, p                required_degree 3
so degree = 4, chunk_len = degree - 2 = 2 and the three permutation columns make two sets.  Queries, in the order enable_equality, gates,
lookups: advice a@0, b@0 (equality), b@+1, c@-1 (gate 0), c@0 (gate 1); instance p@0; fixed s@0 (gate 0), t@0 (lookup).  The most queried
advice column has two queries, so blinding_factors = max(3, 2) + 2 = 5."""
import pytest

import check_util as cu
import proof_util as pu
import systems_util as fam
from proof_util import prover, system_cs


def test_system_degree_and_blinding_factors():
    cs = system_cs()
    assert cs.degree() == 4
    assert cs.num_advice_queries == [1, 2, 2]
    assert cs.blinding_factors() == 5
    assert cs.chunk_len() == 2
    assert cs.num_permutation_sets() == 2
    assert list(cs.phases()) == [0, 1]


def test_system_query_lists():
    cs = system_cs()
    assert cs.advice_queries == [(0, 0), (1, 0), (1, 1), (2, -1), (2, 0)]
    assert cs.instance_queries == [(0, 0)]
    assert cs.fixed_queries == [(0, 0), (1, 0)]
    assert cs.query_index("advice", 2, -1) == 3 and cs.query_index("fixed", 1, 0) == 1
    with pytest.raises(ValueError):
        cs.query_index("advice", 0, 1)
    assert cs.gate_polynomials()[2] == ("const", 0) and cs.gate_polynomials()[:2] == cu.SYSTEM_GATES[:2]


def test_degree_follows_each_argument():
    A = lambda c, r=0: ("advice", c, r)  # noqa: E731
    # no lookup, one gate of degree 2: the permutation's 3 decides, also without permutation columns (permutation.rs:66)
    assert prover.ConstraintSystem(0, 2, 0, [("prod", A(0), A(1))]).degree() == 3
    # a gate of degree 6
    g = ("prod", ("prod", ("prod", A(0), A(1)), ("prod", A(0), A(1))), ("prod", A(0), A(1)))
    cs = prover.ConstraintSystem(0, 2, 0, [g], permutation=[("advice", 0), ("advice", 1)])
    assert cs.degree() == 6 and cs.chunk_len() == 4 and cs.num_permutation_sets() == 1
    # a lookup whose input has degree 2 and table degree 3: 2 + 2 + 3
    lk = ([("prod", A(0), A(1))], [("prod", ("prod", A(0), A(0)), A(0))])
    assert prover.ConstraintSystem(0, 2, 0, [], [lk]).degree() == 7
    assert prover.ConstraintSystem(0, 2, 0, [], minimum_degree=9).degree() == 9
    # four rotations of one column: blinding_factors = 4 + 2; no advice column at all: max(3, 1) + 2
    four = ("sum", ("sum", A(0, -1), A(0, 0)), ("sum", A(0, 1), A(0, 2)))
    assert prover.ConstraintSystem(0, 1, 0, [four]).blinding_factors() == 6
    assert prover.ConstraintSystem(1, 0, 0, [("fixed", 0, 0)]).blinding_factors() == 5


def test_description_is_checked():
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 1, 0, [("advice", 1, 0)])
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 1, 0, [("challenge", 0)])
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 1, 0, [], permutation=[("selector", 0)])
    with pytest.raises(ValueError):
        prover.ConstraintSystem(0, 2, 0, [], advice_column_phase=[0])


# ------------------------------------------------------------------ the family of systems_util.py
# name: (degree, blinding_factors, chunk_len, sets, phases, advice queries, fixed queries, instance queries); the docstrings derive them
FAMILY_HAND = {
    "bare": (3, 5, 1, 0, [0], [(0, 0)], [(0, 0)], []),
    "sets3": (3, 5, 1, 3, [0], [(0, 0), (1, 0), (1, 1)], [(1, 0), (0, 0)], []),
    "deg6": (6, 5, 4, 2, [0], [(0, 0), (1, 0), (2, 0)], [(1, 0), (0, 0)], [(0, 0)]),
    "rot9": (3, 11, 1, 1, [0], [(0, 0), (0, -4), (0, -3), (0, -2), (0, -1), (0, 1), (0, 2), (0, 3), (0, 4)], [(0, 0), (1, 1)], [(0, -1)]),
    "lookups2": (5, 5, 3, 1, [0, 1], [(0, 0), (2, 0), (1, 0), (0, 1)], [(c, 0) for c in range(7)], []),
    "phases3": (3, 5, 1, 2, [0, 1, 2], [(0, 0), (2, 0), (1, 0)], [(0, 0), (1, 0)], []),
    "system": (4, 5, 2, 2, [0, 1], [(0, 0), (1, 0), (1, 1), (2, -1), (2, 0)], [(0, 0), (1, 0)], [(0, 0)]),
}
# name: (proof instances, h pieces, SHPLONK bytes, GWC bytes, distinct opening points)
FAMILY_PROOF_HAND = {
    "bare": (1, 2, 288, 256, 1),
    "sets3": (1, 2, 864, 896, 3),
    "deg6": (1, 5, 928, 960, 3),
    "rot9": (1, 2, 704, 928, 9),
    "lookups2": (2, 4, 2208, 2240, 3),
    "phases3": (1, 2, 736, 768, 3),
    "system": (1, 3, 1120, 1184, 4),
}


def _check_hand(name):
    assert set(fam.NAMES) == set(FAMILY_HAND)
    cs = fam.entry(name).cs
    degree, blinding, chunk_len, sets, phases, advice_q, fixed_q, instance_q = FAMILY_HAND[name]
    assert cs.degree() == degree
    assert cs.blinding_factors() == blinding
    assert cs.chunk_len() == chunk_len
    assert cs.num_permutation_sets() == sets
    assert list(cs.phases()) == phases
    assert cs.advice_queries == advice_q
    assert cs.fixed_queries == fixed_q
    assert cs.instance_queries == instance_q


def test_family_bare():
    """fixed s; advice a; gate s a (a - 1): degree 1 + 1 + 1 = 3, which the permutation's required_degree (3 even without columns,
    permutation.rs:66) equals; no lookup.  chunk_len = 3 - 2 = 1, zero columns make zero sets.  Queries: a@0 and s@0 from the gate, a
    once, so blinding_factors = max(3, 1) + 2 = 5.  One phase."""
    _check_hand("bare")


def test_family_sets3():
    """fixed s, f; advice a, b; gate s (a + b - b(+1)): degree 2; permutation over a, f, b: degree 3, so chunk_len = 1 and three columns
    make three sets.  Queries: enable_equality asks a@0, f@0, b@0 in the permutation's order, so the fixed list starts with column 1; the
    gate then adds s@0 (fixed list [f@0, s@0]: query_index is not the identity) and b@+1.  b has two queries:
    blinding_factors = max(3, 2) + 2 = 5."""
    _check_hand("sets3")
    cs = fam.entry("sets3").cs
    assert cs.query_index("fixed", 0, 0) == 1 and cs.query_index("fixed", 1, 0) == 0


def test_family_deg6():
    """fixed s, t; advice a, b, c; instance p; gate s (a a a b b - c): degree 1 + 5 = 6, so chunk_len = 4 and the five permutation
    columns a, b, c, t, p make ceil(5 / 4) = 2 sets, the last with p alone.  Queries: a@0, b@0, c@0, t@0, p@0 from enable_equality, then
    s@0 from the gate: fixed list [t@0, s@0].  Every advice column has one query: blinding_factors = 5."""
    _check_hand("deg6")


def test_family_rot9():
    """fixed s, f; advice a; instance p; gate s (sum_r (r + 5) a(r) - f(+1) p(-1)), r = -4 .. 4: degree 1 + 2 = 3; permutation over a
    alone: chunk_len = 1, one set.  Queries: a@0 from enable_equality, then the gate left to right: s@0, a@-4 .. a@-1, (a@0 again,)
    a@+1 .. a@+4, f@+1, p@-1.  a has nine queries: blinding_factors = max(3, 9) + 2 = 11; at k = 5 u = 32 - 12 = 20 and x_last is
    omega^-12 x."""
    _check_hand("rot9")
    assert (1 << fam.entry("rot9").k) - fam.entry("rot9").cs.blinding_factors() - 1 == 20


def test_family_lookups2():
    """fixed s, q, t0, t1, q2, qt, t2; advice a, b (phase 0), c (phase 1); challenge 0.  Gate s (a b - a(+1)): degree 3.  Lookup 0
    (q a, q b) in (t0, t1): 2 + 2 + 1 = 5; lookup 1 (c + challenge_0 q2) in (qt t2): 2 + 1 + 2 = 5 (a challenge has degree 0).  Degree 5,
    chunk_len 3, the two permutation columns a, c make one set.  Queries: a@0, c@0 (enable_equality), s@0, b@0, a@+1 (gate), then the
    lookups' fixed columns in index order.  a has two queries: blinding_factors = 5.  Phases 0 and 1."""
    _check_hand("lookups2")


def test_family_phases3():
    """fixed s, f; advice a, b, c in phases 0, 1, 2; challenges 0, 1, 2 after those phases.  Gate 0 s (c - (challenge_0 a +
    challenge_1 b)): degree 2; gate 1 (s (a b - f)) challenge_2: degree 3.  Permutation over a, c: chunk_len 1, two sets.  Queries:
    a@0, c@0 (enable_equality), s@0, b@0 (gate 0), f@0 (gate 1).  blinding_factors = 5."""
    _check_hand("phases3")


def test_family_system():
    """the SYSTEM, as derived at the top of this file"""
    _check_hand("system")


@pytest.mark.parametrize("name", sorted(FAMILY_PROOF_HAND))
def test_family_proof_lengths(name):
    """The proof in the reference's write order (plonk/prover.rs), 32 bytes per point and scalar, N proof instances:
      points   N (advice columns + 2 lookups + sets + lookups) + 1 (random polynomial) + (degree - 1) h pieces
      scalars  N advice queries, fixed queries, 1 (random), permutation columns (sigma), N (3 sets - 1), N 5 lookups
      opening  SHPLONK: 2 points; GWC: one witness per distinct opening point
    bare      points 1 + 1 + 2 = 4; scalars 1 + 1 + 1 = 3; points {x}
    sets3     points 2 + 3 + 1 + 2 = 8; scalars 3 + 2 + 1 + 3 + 8 = 17; points {x, omega x (b@+1, z), omega^-6 x (z of sets 0, 1)}
    deg6      points 3 + 2 + 1 + 5 = 11; scalars 3 + 2 + 1 + 5 + 5 = 16; points {x, omega x, omega^-6 x}
    rot9      points 1 + 1 + 1 + 2 = 5; scalars 9 + 2 + 1 + 1 + 2 = 15; points {omega^r x, r = -4 .. 4}: omega x serves a@+1, f@+1 and z, and
              the one set has no x_last query
    lookups2  points 2 (3 + 4 + 1 + 2) + 1 + 4 = 25; scalars 2 (4 + 2 + 10) + 7 + 1 + 2 = 42; points {x, omega x, omega^-1 x}
    phases3   points 3 + 2 + 1 + 2 = 8; scalars 3 + 2 + 1 + 2 + 5 = 13; points {x, omega x, omega^-6 x}
    system    points 3 + 2 + 2 + 1 + 1 + 3 = 12; scalars 5 + 2 + 1 + 3 + 5 + 5 = 21; points {x, omega x, omega^-1 x, omega^-6 x}"""
    e = fam.entry(name)
    n_instances, pieces, shplonk, gwc, open_points = FAMILY_PROOF_HAND[name]
    assert e.n_instances == n_instances and e.layout["pieces"] == pieces == e.cs.degree() - 1
    assert e.proof_bytes == {"shplonk": shplonk, "gwc": gwc}
    words = e.evaluation_words()
    assert 32 * (words + 2) == shplonk and 32 * (words + open_points) == gwc
    # the layout's counts against the constraint system
    cs, lay = e.cs, e.layout
    sets, lookups = cs.num_permutation_sets(), len(cs.lookups)
    assert lay["points"] == n_instances * (cs.num_advice_columns + 3 * lookups + sets) + 1 + pieces
    assert lay["advice"] == n_instances * len(cs.advice_queries) and lay["fixed"] == len(cs.fixed_queries)
    assert lay["sigma"] == len(cs.permutation) and lay["product"] == n_instances * max(0, 3 * sets - 1) and lay["lookup"] == 5 * n_instances * lookups
    assert e.section("h") == (lay["points"] - pieces, pieces) and e.section("advice")[0] == lay["points"]


@pytest.mark.parametrize("name", sorted(FAMILY_HAND))
def test_family_witness_satisfies_the_model(name):
    """the witness of the key's seed, and a second one under the same fixed columns, satisfy the Python model of MockProver::verify;
    every copy and every active row lies below u"""
    e = fam.entry(name)
    b = e.cs.blinding_factors()
    u = (1 << e.k) - b - 1
    challenges = list(pu.PLACEHOLDER_CHALLENGES[:e.cs.num_challenges])
    first = e.columns(0xC0FFEE, e.k, b, None, challenges)
    second = e.columns(0xC0FFEF, e.k, b, first["fixed"], challenges)
    assert second["fixed"] == first["fixed"] and second["advice"] != first["advice"]
    for cols in (first, second):
        assert fam.model_failures(e, cols, challenges, 5) == []
        assert all(len(values) <= u for values in e.instance_of(cols))
    assert all(r0 < u and r1 < u for _, r0, _, r1 in e.copies)
    if name in ("lookups2", "phases3"):  # the later phases use the challenges: a witness made for other ones fails
        other = [c + 1 for c in challenges]
        assert fam.model_failures(e, e.columns(0xC0FFEE, e.k, b, None, other), challenges, 5) != []


def test_intermediate_sets():
    """queries (commitment, point, eval): commitment 0 at {5, 9}, 1 at {9}, 2 at {9, 5} (the set of 0), 3 at {9} (the set of 1)"""
    q = [(0, 9, 100), (1, 9, 101), (0, 5, 102), (2, 9, 103), (3, 9, 104), (2, 5, 105)]
    assert prover.construct_intermediate_sets_gwc(q) == [(9, [(0, 100), (1, 101), (2, 103), (3, 104)]), (5, [(0, 102), (2, 105)])]
    sets, super_set = prover.construct_intermediate_sets_shplonk(q)
    assert super_set == [5, 9]
    assert sets == [([5, 9], [(0, [102, 100]), (2, [105, 103])]), ([9], [(1, [101]), (3, [104])])]
