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


def test_intermediate_sets():
    """queries (commitment, point, eval): commitment 0 at {5, 9}, 1 at {9}, 2 at {9, 5} (the set of 0), 3 at {9} (the set of 1)"""
    q = [(0, 9, 100), (1, 9, 101), (0, 5, 102), (2, 9, 103), (3, 9, 104), (2, 5, 105)]
    assert prover.construct_intermediate_sets_gwc(q) == [(9, [(0, 100), (1, 101), (2, 103), (3, 104)]), (5, [(0, 102), (2, 105)])]
    sets, super_set = prover.construct_intermediate_sets_shplonk(q)
    assert super_set == [5, 9]
    assert sets == [([5, 9], [(0, [102, 100]), (2, [105, 103])]), ([9], [(1, [101]), (3, [104])])]
