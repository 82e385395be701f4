"""Python big-integer restatement of the three data-parallel loops of the reference's MockProver::verify (halo2_proofs/src/dev.rs; test
infrastructure only), over plain columns of canonical integers mod r:

  gate_failures         :676-746  every gate polynomial at every row of the domain (gate_row_ids chained with the blinding rows is all n
                                  rows), rotations wrapping modulo n; a non-zero value is a failure
  lookup_failures       :751-886  every input row below u = n - blinding_factors - 1 whose (compressed) value no table row below u holds
  permutation_failures  :889-931  every cell whose value differs from the value of the cell the assembly's mapping sends it to
  verify                :933-938  the three lists chained: gates, lookups, permutation

Expressions are the tuples of evaluation.py, evaluated directly (lookup_util.eval_expr), not through a graph."""
import numpy as np

from lookup_util import R_MOD, compress, eval_expr, to_mont


def gate_failures(polys, n, cols, challenges=()):
    """[rows at which polynomial g is non-zero] per polynomial; None is the zero polynomial"""
    return [[] if p is None else [row for row in range(n) if eval_expr(p, row, n, cols, challenges) != 0] for p in polys]


def lookup_failures(inputs, tables, u):
    """inputs[j], tables[j]: the compressed columns of lookup j"""
    out = []
    for inp, tab in zip(inputs, tables):
        have = set(tab[:u])
        out.append([row for row in range(u) if inp[row] not in have])
    return out


def permutation_failures(columns, mapping):
    """columns[j][i] against columns[c][r], (c, r) = mapping[j][i]"""
    return [[i for i in range(len(col)) if col[i] != columns[int(mapping[j][i][0])][int(mapping[j][i][1])]] for j, col in enumerate(columns)]


def verify(n, cols, challenges, gate_polys, lookups, theta, u, perm_columns, mapping):
    """the failures as ("gate", g, row), ("lookup", j, row), ("permutation", column, row) in verify's order"""
    out = [("gate", g, r) for g, rows in enumerate(gate_failures(gate_polys, n, cols, challenges)) for r in rows]
    ins = [compress(i, theta, n, cols, challenges) for i, _ in lookups]
    tabs = [compress(t, theta, n, cols, challenges) for _, t in lookups]
    out += [("lookup", j, r) for j, rows in enumerate(lookup_failures(ins, tabs, u)) for r in rows]
    pc = [cols[kind][i] for kind, i in perm_columns]
    out += [("permutation", j, r) for j, rows in enumerate(permutation_failures(pc, mapping)) for r in rows]
    return out


def expected(fails, max_rows):
    """the (counts, rows) an engine call must return for these per-item row lists"""
    counts = np.array([len(f) for f in fails], dtype=np.uint64)
    rows = np.full((len(fails), max_rows), 0xFFFFFFFF, dtype=np.uint32)
    for j, f in enumerate(fails):
        low = sorted(f)[:max_rows]
        rows[j, :len(low)] = low
    return counts, rows


def mont_cols(cols):
    return {key: [to_mont(c) for c in cols[key]] for key in ("fixed", "advice", "instance")}


# ---- the system of the composition tests and of tests/cpp/test_check_mirror.cpp: fixed s, t; advice a, b, c; instance p
S, A, B, C, P = ("fixed", 0, 0), ("advice", 0, 0), ("advice", 1, 1), ("advice", 2, -1), ("instance", 0, 0)
SYSTEM_GATES = [("prod", S, ("sum", ("prod", A, B), ("neg", C))),
                ("prod", ("prod", S, ("sum", ("advice", 2, 0), ("neg", P))), ("challenge", 0)),
                None]
SYSTEM_LOOKUPS = [([A], [("fixed", 1, 0)])]
SYSTEM_PERM = [("advice", 0), ("advice", 1), ("instance", 0)]
SYSTEM_COPIES = [(0, 3, 1, 4), (1, 4, 0, 7), (2, 0, 0, 1), (1, 9, 2, 5), (0, 11, 0, 12)]  # (column, row, column, row) of SYSTEM_PERM


def system_witness(rng, k, b):
    """a witness that satisfies SYSTEM_* by construction: s is one on rows 1 .. u - 2, so no gate reads a blinding row; the blinding rows
    hold random values; the copies stay below u"""
    n, u = 1 << k, (1 << k) - b - 1
    rnd = lambda: rng.randrange(R_MOD)  # noqa: E731
    t = [rnd() for _ in range(n)]
    s = [1 if 1 <= i <= u - 2 else 0 for i in range(n)]
    a = [rng.choice(t[:u]) for _ in range(n)]
    bb = [rnd() for _ in range(n)]
    p = [rnd() for _ in range(n)]
    a[7] = a[3]
    a[12] = a[11]
    bb[4] = a[3]
    c = [rnd() for _ in range(n)]
    for i in range(1, u - 1):
        c[i - 1] = a[i] * bb[i + 1] % R_MOD
    for i in range(1, u - 1):
        p[i] = c[i]
    p[0] = a[1]
    bb[9] = p[5]
    # b[9] is read by the first gate at row 8: its c cell follows, and so does the instance cell the second gate ties to it
    c[7] = a[8] * bb[9] % R_MOD
    p[7] = c[7]
    for i in range(u, n):
        a[i], bb[i], c[i] = rnd(), rnd(), rnd()
    return {"fixed": [s, t], "advice": [a, bb, c], "instance": [p]}
