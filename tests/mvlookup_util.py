"""Python big-integer model of the logUp (mv-lookup) argument (test infrastructure only).

The argument belongs to upstream forks later than the reference this repository follows, so there is no oracle for it: the model below
restates the definitions of include/halo2hip.h (h2hip_mvlookup_multiplicities_bn254, h2hip_mvlookup_sums_bn254, h2hip_evalh_mvlookups)
on canonical integers mod r, directly from the expression tuples.  Where a GraphEvaluator graph is involved the model evaluates the
expressions themselves AND interprets the graph, and insists that both agree, so a wrong graph builder cannot hide behind the model.
Column cosets come from the engine's oracle-checked coeff_to_extended; the value of h(X) before the stage from the oracle's evaluate_h
(and, behind halo2 lookups, the engine's oracle-checked lookup stage)."""
from product_util import R_MOD, ff_batch_invert, from_mont, to_mont  # noqa: F401  (re-exported for the tests)
from shuffle_util import (CALC_ADD, CALC_DOUBLE, CALC_HORNER, CALC_MUL, CALC_NEGATE, CALC_SQUARE, CALC_STORE, CALC_SUB, VS_ADVICE,  # noqa: F401
                          VS_BETA, VS_CHALLENGE, VS_CONSTANT, VS_FIXED, VS_INSTANCE, VS_INTERMEDIATE, VS_THETA, Columns, compress,
                          compress_column, eval_expr)


def multiplicities(inputs, table, blinding_factors):
    """M[i] for one argument.  inputs: K integer columns, table: one; the count of a value goes to the LOWEST table row < u holding it,
    rows >= u are zero.  Returns (M, missing) with missing[c] true when input column c has a row < u whose value is absent from T[0 .. u)."""
    n = len(table)
    u = n - blinding_factors - 1
    first = {}
    for i in range(u):
        first.setdefault(table[i], i)
    m = [0] * n
    missing = []
    for col in inputs:
        bad = False
        for r in range(u):
            i = first.get(col[r])
            if i is None:
                bad = True
            else:
                m[i] += 1
        missing.append(bad)
    return m, missing


def lowest_missing(missing_per_argument):
    """the (argument, input column) the engine names: the lowest failing pair, or None"""
    for j, miss in enumerate(missing_per_argument):
        for c, bad in enumerate(miss):
            if bad:
                return j, c
    return None


def grand_sum(inputs, table, m, beta, blinding, blinding_factors):
    """phi[0] = 0, phi[i] = phi[i-1] + sum_c inv(F_c[i-1] + beta) - M[i-1] inv(T[i-1] + beta) for 1 <= i <= u, then the blinding rows.
    inv is ff's BatchInvert: a zero denominator stays zero, that term drops out and the sum goes on."""
    n = len(table)
    u = n - blinding_factors - 1
    inv_f = [ff_batch_invert([(col[i] + beta) % R_MOD for i in range(u)]) for col in inputs]
    inv_t = ff_batch_invert([(table[i] + beta) % R_MOD for i in range(u)])
    phi = [0]
    for i in range(1, u + 1):
        phi.append((phi[i - 1] + sum(f[i - 1] for f in inv_f) - m[i - 1] * inv_t[i - 1]) % R_MOD)
    assert len(phi) == n - blinding_factors
    return phi + [int(b) % R_MOD for b in blinding]


def graph_value(g, cols, idx, theta, beta):
    """GraphEvaluator::evaluate of a graph built by evaluation.mvlookup_graphs: the target of the last calculation, zero for an empty
    graph.  Reading gamma, y or the previous value is an error here as it is in the engine."""
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
        if kind == VS_BETA:
            return beta
        raise ValueError("an mv-lookup graph reads value source kind %d" % kind)

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


def fold_mvlookups(h, arguments, cols, y, theta, beta, l0, l_last, l_active):
    """the mv-lookup stage over every row of one domain.  h: integers on entry; arguments: [(inputs, table_exprs, graphs or None, pc, mc)]
    with inputs the list of input expression tuples, graphs the K + 1 graphs (inputs, then table), pc / mc the cosets of phi and m as
    integers; l0 / l_last / l_active integer columns.  Returns the folded integers."""
    out = list(h)
    step = cols.rot_scale
    for inputs, tab, graphs, pc, mc in arguments:
        for idx in range(cols.size):
            phis = [(compress(inp, theta, cols, idx) + beta) % R_MOD for inp in inputs]
            tau = (compress(tab, theta, cols, idx) + beta) % R_MOD
            if graphs is not None:
                assert len(graphs) == len(inputs) + 1
                assert [graph_value(g, cols, idx, theta, beta) for g in graphs] == phis + [tau]
            P, Q = 1, 0
            for f in phis:  # Q <- Q f + P; P <- P f
                Q = (Q * f + P) % R_MOD
                P = P * f % R_MOD
            direct = 0
            for a in range(len(phis)):
                t = 1
                for b2, f in enumerate(phis):
                    if b2 != a:
                        t = t * f % R_MOD
                direct = (direct + t) % R_MOD
            assert Q == direct
            p, pn = pc[idx], pc[(idx + step) % cols.size]
            v = out[idx]
            v = (v * y + l0[idx] * p) % R_MOD
            v = (v * y + l_last[idx] * p) % R_MOD
            v = (v * y + l_active[idx] * (tau * P * (pn - p) - tau * Q + mc[idx] * P)) % R_MOD
            out[idx] = v
    return out


def required_degree(inputs, table_exprs):
    """2 + d_t + sum_c d_c, each d the largest degree in that tuple, at least 1"""
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

    def tuple_deg(exprs):
        return max([1] + [deg(e) for e in exprs])
    return 2 + tuple_deg(table_exprs) + sum(tuple_deg(inp) for inp in inputs)
