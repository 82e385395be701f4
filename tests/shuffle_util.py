"""Python big-integer model of the shuffle argument (test infrastructure only).

The argument is upstream PSE halo2's and later than the reference this repository follows, so there is no oracle for it: the model below
restates the definitions of include/halo2hip.h (h2hip_shuffle_products_bn254, h2hip_evalh_shuffles, h2hip_check_shuffles_bn254) on
canonical integers mod r, directly from the expression tuples.  Where a GraphEvaluator graph is involved the model evaluates the
expressions themselves AND interprets the graph, and insists that both agree, so a wrong graph builder cannot hide behind the model.
Column cosets come from the engine's oracle-checked coeff_to_extended; the value of h(X) before the shuffle stage from the oracle's
evaluate_h."""
from collections import Counter

import numpy as np

from product_util import R_MOD, ff_batch_invert, from_mont, to_mont  # noqa: F401  (re-exported for the tests)

VS_CONSTANT, VS_INTERMEDIATE, VS_FIXED, VS_ADVICE, VS_INSTANCE, VS_CHALLENGE, VS_BETA, VS_GAMMA, VS_THETA, VS_Y, VS_PREVIOUS = range(11)
CALC_ADD, CALC_SUB, CALC_MUL, CALC_SQUARE, CALC_DOUBLE, CALC_NEGATE, CALC_HORNER, CALC_STORE = range(8)


class Columns:
    """integer columns of one domain: fixed / advice / instance lists of `size` integers, the challenges, and how far one rotation
    moves a row (1 on the 2^k Lagrange rows, 2^(extended_k - k) on the extended coset)"""

    def __init__(self, fixed, advice, instance, challenges, size, rot_scale=1):
        self.pools = {"fixed": fixed, "advice": advice, "instance": instance}
        self.challenges, self.size, self.rot_scale = list(challenges), size, rot_scale

    def query(self, kind, col, rot, idx):
        return self.pools[kind][col][(idx + rot * self.rot_scale) % self.size]


def eval_expr(e, cols, idx):
    """an expression tuple of evaluation.py at row idx"""
    tag = e[0]
    if tag == 'const':
        return e[1] % R_MOD
    if tag in ('fixed', 'advice', 'instance'):
        return cols.query(tag, e[1], e[2], idx)
    if tag == 'challenge':
        return cols.challenges[e[1]]
    if tag == 'neg':
        return -eval_expr(e[1], cols, idx) % R_MOD
    if tag == 'sum':
        return (eval_expr(e[1], cols, idx) + eval_expr(e[2], cols, idx)) % R_MOD
    if tag == 'prod':
        return eval_expr(e[1], cols, idx) * eval_expr(e[2], cols, idx) % R_MOD
    if tag == 'scaled':
        return eval_expr(e[1], cols, idx) * e[2] % R_MOD
    raise ValueError(tag)


def compress(exprs, theta, cols, idx):
    """the theta fold of a tuple of expressions: acc * theta + expr, starting at zero"""
    acc = 0
    for e in exprs:
        acc = (acc * theta + eval_expr(e, cols, idx)) % R_MOD
    return acc


def compress_column(exprs, theta, cols):
    return [compress(exprs, theta, cols, i) for i in range(cols.size)]


def graph_value(g, cols, idx, theta, gamma):
    """GraphEvaluator::evaluate of a GraphEvaluator built by evaluation.py: the target of the last calculation, zero for an empty graph.
    Reading beta, y or the previous value is an error here as it is in the engine."""
    kinds = {VS_FIXED: "fixed", VS_ADVICE: "advice", VS_INSTANCE: "instance"}
    inter = {}

    def get(v):
        kind, a, b = v
        if kind == VS_CONSTANT:
            return g.constants[a] % R_MOD
        if kind == VS_INTERMEDIATE:
            return inter[a]
        if kind in kinds:
            return cols.query(kinds[kind], a, g.rotations[b], idx)
        if kind == VS_CHALLENGE:
            return cols.challenges[a]
        if kind == VS_THETA:
            return theta
        if kind == VS_GAMMA:
            return gamma
        raise ValueError("a shuffle graph reads value source kind %d" % kind)

    last = 0
    for (op, x, y, parts), target in g.calculations:
        if op == CALC_ADD:
            v = get(x) + get(y)
        elif op == CALC_SUB:
            v = get(x) - get(y)
        elif op == CALC_MUL:
            v = get(x) * get(y)
        elif op == CALC_SQUARE:
            v = get(x) ** 2
        elif op == CALC_DOUBLE:
            v = 2 * get(x)
        elif op == CALC_NEGATE:
            v = -get(x)
        elif op == CALC_STORE:
            v = get(x)
        elif op == CALC_HORNER:
            v, f = get(x), get(y)
            for p in parts:
                v = (v * f + get(p)) % R_MOD
        else:
            raise ValueError(op)
        inter[target] = last = v % R_MOD
    return last


def shuffle_product(a_col, s_col, gamma, blinding, blinding_factors):
    """commit_product: z[0] = 1, z[i] = z[i-1] (A[i-1] + gamma) inv(S[i-1] + gamma) for 1 <= i <= u, then the blinding rows.  inv is ff's
    BatchInvert: a zero denominator stays zero."""
    n = len(a_col)
    u = n - blinding_factors - 1
    inv = ff_batch_invert([(s_col[i] + gamma) % R_MOD for i in range(u)])
    z = [1]
    for i in range(1, u + 1):
        z.append(z[i - 1] * ((a_col[i - 1] + gamma) % R_MOD) % R_MOD * inv[i - 1] % R_MOD)
    assert len(z) == n - blinding_factors
    return z + [int(b) % R_MOD for b in blinding]


def fold_shuffles(h, shuffles, cols, y, theta, gamma, l0, l_last, l_active):
    """the shuffle stage over every row of one domain.  h: integers on entry (after the gates, the permutation argument and the lookups);
    shuffles: [(input_exprs, shuffle_exprs, graphs or None, zc)] with zc the product's coset as integers; l0 / l_last / l_active integer
    columns.  Returns the folded integers."""
    out = list(h)
    step = cols.rot_scale
    for inp, shf, graphs, zc in shuffles:
        for idx in range(cols.size):
            a = (compress(inp, theta, cols, idx) + gamma) % R_MOD
            s = (compress(shf, theta, cols, idx) + gamma) % R_MOD
            if graphs is not None:
                assert graph_value(graphs[0], cols, idx, theta, gamma) == a and graph_value(graphs[1], cols, idx, theta, gamma) == s
            z, zn = zc[idx], zc[(idx + step) % cols.size]
            v = out[idx]
            v = (v * y + (1 - z) * l0[idx]) % R_MOD
            v = (v * y + (z * z - z) * l_last[idx]) % R_MOD
            v = (v * y + l_active[idx] * (zn * s - z * a)) % R_MOD
            out[idx] = v
    return out


def required_degree(input_exprs, shuffle_exprs):
    def deg(e):
        tag = e[0]
        if tag in ('const', 'challenge'):
            return 0
        if tag in ('fixed', 'advice', 'instance'):
            return 1
        if tag in ('neg', 'scaled'):
            return deg(e[1])
        if tag == 'sum':
            return max(deg(e[1]), deg(e[2]))
        return deg(e[1]) + deg(e[2])
    return 2 + max([1] + [deg(e) for e in list(input_exprs) + list(shuffle_exprs)])


def failing_rows(a_col, s_col, blinding_factors):
    """input rows i < u whose value occurs a different number of times among A[0 .. u) than among S[0 .. u)"""
    u = len(a_col) - blinding_factors - 1
    ca, cs = Counter(a_col[:u]), Counter(s_col[:u])
    return [i for i in range(u) if ca[a_col[i]] != cs[a_col[i]]]


def check_result(rows_list, max_rows):
    """(counts, rows) as the engine reports a list of failing-row lists"""
    counts = np.array([len(r) for r in rows_list], dtype=np.uint64)
    rows = np.full((len(rows_list), max_rows), 0xFFFFFFFF, dtype=np.uint32)
    for j, r in enumerate(rows_list):
        rows[j, :min(len(r), max_rows)] = r[:max_rows]
    return counts, rows
