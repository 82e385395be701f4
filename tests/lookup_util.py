"""Python big-integer restatement of the reference's lookup::Argument::commit_permuted (test infrastructure only).

compress restates the compression of halo2_proofs/src/plonk/lookup/prover.rs:90-115 by evaluating the expression tuples of
evaluation.py directly (not through a graph); permute restates permute_expression_pair (:391-475) literally: `sorted`, a Counter walked
in key order (the BTreeMap), list pop() for repeated_input_rows.  Values are canonical integers mod r, so `sorted` is Fr's Ord."""
from collections import Counter

import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_MONT = (1 << 256) % R_MOD
_MONT_INV = pow(_MONT, -1, R_MOD)


def to_mont(vals):
    raw = b"".join(((int(v) % R_MOD) * _MONT % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def from_mont(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * _MONT_INV % R_MOD for i in range(0, len(raw), 32)]


def mont_int(v):
    """the Montgomery limbs of v read as one 256-bit integer (what a sort of the raw limbs would order by)"""
    return (int(v) % R_MOD) * _MONT % R_MOD


class ConstraintSystemFailure(Exception):
    pass


def eval_expr(e, row, n, cols, challenges):
    """plonk/circuit.rs Expression::evaluate at one Lagrange row; cols = {'fixed': [...], 'advice': [...], 'instance': [...]}"""
    tag = e[0]
    if tag == "const":
        return e[1] % R_MOD
    if tag in ("fixed", "advice", "instance"):
        return cols[tag][e[1]][(row + e[2]) % n]
    if tag == "challenge":
        return challenges[e[1]]
    if tag == "neg":
        return -eval_expr(e[1], row, n, cols, challenges) % R_MOD
    if tag == "sum":
        return (eval_expr(e[1], row, n, cols, challenges) + eval_expr(e[2], row, n, cols, challenges)) % R_MOD
    if tag == "prod":
        return eval_expr(e[1], row, n, cols, challenges) * eval_expr(e[2], row, n, cols, challenges) % R_MOD
    if tag == "scaled":
        return eval_expr(e[1], row, n, cols, challenges) * e[2] % R_MOD
    raise ValueError(tag)


def compress(exprs, theta, n, cols, challenges=()):
    """:90-115: fold the expressions with theta, acc = acc * theta + e_j, over every row"""
    out = []
    for row in range(n):
        acc = 0
        for e in exprs:
            acc = (acc * theta + eval_expr(e, row, n, cols, challenges)) % R_MOD
        out.append(acc)
    return out


def permute(inp, table, u, blind_a, blind_s):
    """permute_expression_pair (:391-475): returns (A', S') over n = u + len(blind_a) rows"""
    permuted_input = sorted(inp[:u])
    leftover = Counter(table[:u])
    permuted_table = [None] * u
    repeated_input_rows = []
    for row, v in enumerate(permuted_input):
        if row == 0 or v != permuted_input[row - 1]:
            permuted_table[row] = v
            if leftover.get(v, 0) > 0:
                leftover[v] -= 1
            else:
                raise ConstraintSystemFailure(row)
        else:
            repeated_input_rows.append(row)
    for coeff in sorted(leftover):
        for _ in range(leftover[coeff]):
            permuted_table[repeated_input_rows.pop()] = coeff
    assert not repeated_input_rows
    return permuted_input + list(blind_a), permuted_table + list(blind_s)
