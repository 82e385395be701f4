"""Inputs and graphs that push evaluate_h's lazily reduced arithmetic to its magnitude bounds (test infrastructure only).

evaluate_h's kernels (csrc/evalh.hip, csrc/evalh_dev.h) run on the 9 x 29-bit multiplier of csrc/fieldu.h and keep their values unreduced
between operations.  compile_graph tracks a magnitude per operation -- a column is < 32 r, a product of a and b is < a b / 169 + 1, sums
add -- and requests a reduction where a value would pass 100 r, and a closing one where the result would pass 15 r.  Uniformly random
columns sit near r / 2 and never come near those figures.  This module holds what does:

  VALUES            the stored words of ntt_edge_util plus the two words x < r whose I-form operand (the limbs of 32 x, fu_from_ext) has
                    limbs 0..7 saturated
  patterns          const(v), extremes(seed), signs, one random control -- as `scenarios` of a whole system's columns
  families()        named graphs in calculation form, each aimed at one bound (the docstring of every builder states it)
  compiled_program  the program compile_graph makes of a graph, its tracked magnitudes and the generator's fusion plan
                    (h2hip_debug_evalh_program; no GPU)
  eval_graph_ints   a graph over Python integers, calculation by calculation: the reference that needs neither the oracle nor the engine
  write_corpus      (graph, scenario) records as the binary file tests/cpp/test_evalh_bounds.cpp reads
"""
import ctypes
import struct

import numpy as np

import ntt_edge_util as eu
from evalh_util import (CALC_ADD, CALC_DOUBLE, CALC_HORNER, CALC_MUL, CALC_NEGATE, CALC_SQUARE, CALC_STORE, CALC_SUB, GraphEvaluator,
                        VS_ADVICE, VS_BETA, VS_CHALLENGE, VS_CONSTANT, VS_FIXED, VS_GAMMA, VS_INSTANCE, VS_INTERMEDIATE, VS_PREVIOUS, VS_THETA,
                        VS_Y, flatten_graph, graph_struct)
from product_util import R_MOD

# the column counts of every system here (those of test_evalh._random_case, whose graphs and case these drop into)
N_FIXED, N_ADVICE, N_INSTANCE, N_CHALLENGES = 6, 5, 1, 2

OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_DBL, OP_NEG, OP_MOV, OP_FMA = range(8)
OP_REDUCE_FLAG = 0x100
MAG_LIMIT, MAG_RESULT, MAG_COLUMN = 100.0, 15.0, 32.0  # EVALH_MAG_LIMIT / _RESULT / _COLUMN of csrc/evalh.hip

# fu_from_ext(x) is the 29-bit limbs of 32 x: limb 0 is bits 0..23 of x above five zero bits, limb i bits 29 i - 5 .. 29 i + 23.  With
# bits 0..226 of x set, limb 0 is 2^29 - 32 and limbs 1..7 are 2^29 - 1; the top limb takes bits 227 up: 0 and the largest that stays below r
_SAT_LOW = (1 << 227) - 1
SAT_TOP = (R_MOD - _SAT_LOW - 1) >> 227
VALUES = dict(eu.VALUES)
VALUES["sat32"] = _SAT_LOW
VALUES["sat32top"] = (SAT_TOP << 227) | _SAT_LOW
assert all(0 <= v < R_MOD for v in VALUES.values()) and ((SAT_TOP + 1) << 227) | _SAT_LOW >= R_MOD
_VALUE_LIST = list(VALUES.values())
_MONT = (1 << 256) % R_MOD
_MONT_INV = pow(_MONT, -1, R_MOD)


def i_form_limbs(x):
    """fu_from_ext of the stored word x"""
    return [((32 * x) >> (29 * i)) & 0x1FFFFFFF for i in range(9)]


def extremes(n, seed):
    return eu.words([_VALUE_LIST[i] for i in np.random.RandomState(seed).randint(len(_VALUE_LIST), size=n)])


def random_words(n, seed):
    rs = np.random.RandomState(seed)
    return eu.words([int.from_bytes(rs.bytes(40), "little") % R_MOD for _ in range(n)])


# ---------------------------------------------------------------------------------------------------------- scenarios
# A scenario names how every column of a system is filled: ("const", value name), ("extremes", seed), ("signs", seed), ("partial", seed)
# -- extremes whose advice columns 2 and 3 repeat columns 1 and 0 on the even rows, so that a b - c d cancels on those rows only -- and
# ("random", seed), the control.  The scalars (y, beta, gamma, theta, the challenges) are the word r - 1 except in the control.
SCENARIOS = [("const", v) for v in VALUES] + [("extremes", 1), ("extremes", 2), ("signs", 7), ("partial", 3), ("random", 5)]


def scenario_id(sc):
    return "%s(%s)" % sc


def column(sc, n, salt):
    """one column of n rows under the scenario; salt tells the columns of a system apart"""
    kind, arg = sc
    if kind == "const":
        return eu.const(n, VALUES[arg])
    if kind in ("extremes", "partial"):
        return extremes(n, 1000 * arg + salt)
    if kind == "signs":
        return eu.signs(n, 1, 1000 * arg + salt)
    return random_words(n, 1000 * arg + salt)


def scalar(sc, salt):
    return random_words(1, 77000 + salt)[0] if sc[0] == "random" else eu.words([R_MOD - 1])[0]


def scenario_columns(sc, n):
    """every operand a graph can name, under the scenario, on n rows: dict of fixed / advice / instance (lists of (n, 4)), previous (n, 4),
    challenges (N_CHALLENGES, 4) and beta / gamma / theta / y (4,)"""
    out = {
        "fixed": [column(sc, n, 10 + i) for i in range(N_FIXED)],
        "advice": [column(sc, n, 20 + i) for i in range(N_ADVICE)],
        "instance": [column(sc, n, 30 + i) for i in range(N_INSTANCE)],
        "previous": column(sc, n, 99),
        "challenges": np.stack([scalar(sc, 40 + i) for i in range(N_CHALLENGES)]),
        "beta": scalar(sc, 2), "gamma": scalar(sc, 3), "theta": scalar(sc, 4), "y": scalar(sc, 1),
    }
    if sc[0] == "partial":
        out["advice"][2][0::2] = out["advice"][1][0::2]
        out["advice"][3][0::2] = out["advice"][0][0::2]
    return out


# ---------------------------------------------------------------------------------------------------------- graphs
class _B:
    """a graph straight in calculation form: no deduplication and no operand reordering, so that a b - b a stays two products"""

    def __init__(self):
        self.g = GraphEvaluator()
        self.rot = {r: self.g.add_rotation(r) for r in (0, 1, -1)}

    def A(self, c, r=0):
        return (VS_ADVICE, c, self.rot[r])

    def F(self, c, r=0):
        return (VS_FIXED, c, self.rot[r])

    def I(self, c=0, r=0):  # noqa: E743
        return (VS_INSTANCE, c, self.rot[r])

    def K(self, v):
        return self.g.add_constant(v)

    def emit(self, op, x, y=None, parts=()):
        t = self.g.num_intermediates
        self.g.calculations.append(((op, x, y, tuple(parts)), t))
        self.g.num_intermediates += 1
        return (VS_INTERMEDIATE, t, 0)

    def add(self, x, y):
        return self.emit(CALC_ADD, x, y)

    def sub(self, x, y):
        return self.emit(CALC_SUB, x, y)

    def mul(self, x, y):
        return self.emit(CALC_MUL, x, y)

    def sum(self, srcs):
        acc = srcs[0]
        for s in srcs[1:]:
            acc = self.add(acc, s)
        return acc

    def cols(self, n, start=0):
        """n distinct column operands (advice, then fixed with a rotation, then the instance column)"""
        pool = [self.A(i) for i in range(N_ADVICE)] + [self.F(i, 1) for i in range(N_FIXED)] + [self.I(0, -1)]
        return [pool[(start + i) % len(pool)] for i in range(n)]


PREV, Y, BETA, GAMMA, THETA = (VS_PREVIOUS, 0, 0), (VS_Y, 0, 0), (VS_BETA, 0, 0), (VS_GAMMA, 0, 0), (VS_THETA, 0, 0)
ZERO, ONE = (VS_CONSTANT, 0, 0), (VS_CONSTANT, 1, 0)


def _sum_chain(n):
    """[32 n]: the sum of n columns; the fourth column brings 128 > 100, a reduction requested on an ADD, and from there the result is
    above 15 and takes the closing MOV|REDUCE"""
    b = _B()
    c = b.cols(n)
    if n == 1:
        b.emit(CALC_STORE, c[0])
    else:
        b.sum(c)
    return b.g


def _dbl_chain(n):
    """[32 -> 64 -> 128]: the second doubling requests a reduction on a DBL"""
    b = _B()
    acc = b.A(0)
    for _ in range(n):
        acc = b.emit(CALC_DOUBLE, acc)
    return b.g


def _wide_product(square):
    """[96] x [96] = [55.5]: the largest operands a product meets without a reduction before it"""
    b = _B()
    s1 = b.sum(b.cols(3))
    if square:
        b.emit(CALC_SQUARE, s1)
    else:
        b.mul(s1, b.sum(b.cols(3, 5)))
    return b.g


def _zero_minus_sum():
    """[-96]: 0 - (three-column sum) as the result: negative, above 15, closing MOV|REDUCE of a negative value"""
    b = _B()
    b.sub(ZERO, b.sum(b.cols(3)))
    return b.g


def _sub_chain(n):
    """[-32 n]: 0 - c0 - c1 - ...; the fourth column brings -128, a reduction requested on a SUB of a negative value"""
    b = _B()
    acc = ZERO
    for c in b.cols(n):
        acc = b.sub(acc, c)
    return b.g


def _neg_times_pos():
    """[-96] x [96]"""
    b = _B()
    b.mul(b.sub(ZERO, b.sum(b.cols(3))), b.sum(b.cols(3, 5)))
    return b.g


def _neg_product():
    """NEG of a product of two columns as the result: about -7 r in front of out_e, no closing reduction"""
    b = _B()
    b.emit(CALC_NEGATE, b.mul(b.A(0), b.F(0)))
    return b.g


def _products(n):
    """the sum of n products of two columns: [7.06 n].  Two give 14.1 and take no closing MOV; three give 21.2 and take it"""
    b = _B()
    b.sum([b.mul(b.A(i), b.F(i)) for i in range(n)])
    return b.g


def _horner(n_parts):
    """Horner over a column: x = a column, y = a column ([32], not Y), the parts unreduced sums of two and three columns in turn
    ([64], [96]): a step is [acc * 32 / 169 + 1 + part], and with a [96] part it passes 100 -- a reduction requested on an FMA"""
    b = _B()
    parts = [b.sum(b.cols(2 + i % 2, 3 * i)) for i in range(n_parts)]
    b.emit(CALC_HORNER, b.A(4, 1), b.F(5), parts)
    return b.g


def _fusible(kind):
    """what the per-circuit generator emits as ONE reduction: add / sub of two products of plain columns, the same with [96] operands
    (each product [55.5], the sum 111 > 100: the fused ADD / SUB itself carries the reduction request), and a Horner step whose addend is
    a product"""
    b = _B()
    if kind in ("add", "sub"):
        p, q = b.mul(b.A(0), b.F(0)), b.mul(b.A(1), b.F(1, 1))
        (b.add if kind == "add" else b.sub)(p, q)
    elif kind in ("add96", "sub96"):
        s = [b.sum(b.cols(3, 3 * i)) for i in range(4)]  # the four sums first: a product fuses only while its operands' slots are untouched
        p, q = b.mul(s[0], s[1]), b.mul(s[2], s[3])
        (b.add if kind == "add96" else b.sub)(p, q)
    else:
        b.emit(CALC_HORNER, PREV, Y, [b.mul(b.A(0), b.F(0)), b.mul(b.A(1), b.A(2, -1))])
    return b.g


def _identity(kind):
    """0 in the field, k r in the lanes, whatever the columns hold: a b - b a, (a + b) - a - b, a * 1 - a (the constant one).  `abcd` is
    a b - c d, which cancels on the rows where the scenario makes c = b and d = a"""
    b = _B()
    a_, b_ = b.A(0), b.A(1)
    if kind == "ab-ba":
        b.sub(b.mul(a_, b_), b.mul(b_, a_))
    elif kind == "a+b-a-b":
        b.sub(b.sub(b.add(a_, b_), a_), b_)
    elif kind == "a*1-a":
        b.sub(b.mul(a_, ONE), a_)
    else:
        b.sub(b.mul(a_, b_), b.mul(b.A(2), b.A(3)))
    return b.g


IDENTITIES = ("ab-ba", "a+b-a-b", "a*1-a")  # the graphs of _identity whose value is 0 on every input


def _constants():
    """the graph constants 0, 1 and -1 (stored as r - 2^256 mod r) and the one whose stored word is r - 1, with the challenges and
    y / beta / gamma / theta as operands"""
    b = _B()
    m1, w = b.K(R_MOD - 1), b.K((R_MOD - 1) * _MONT_INV % R_MOD)
    t = b.mul((VS_CHALLENGE, 0, 0), (VS_CHALLENGE, 1, 0))
    u = b.add(t, m1)
    v = b.mul(u, Y)
    x = b.sub(v, b.mul(BETA, GAMMA))
    x = b.add(x, b.mul(THETA, ONE))
    x = b.add(ZERO, x)
    x = b.mul(b.add(x, b.A(0)), w)
    b.sub(b.mul(x, m1), b.mul(w, w))
    return b.g


def _constants_only():
    """no column at all: constants and scalars alone, the same value on every row"""
    b = _B()
    m1, w = b.K(R_MOD - 1), b.K((R_MOD - 1) * _MONT_INV % R_MOD)
    s = b.sum([m1, w, BETA, GAMMA, THETA, Y, (VS_CHALLENGE, 0, 0), (VS_CHALLENGE, 1, 0)])
    b.sub(b.mul(s, m1), b.emit(CALC_SQUARE, w))
    return b.g


def _previous(kind):
    """PreviousValue ([32], the incoming values row) as an operand of a product, a sum, a Horner part and a difference"""
    b = _B()
    if kind == "mul":
        b.mul(PREV, b.A(0))
    elif kind == "dbl":
        b.add(PREV, PREV)
    elif kind == "horner":
        b.emit(CALC_HORNER, PREV, Y, [PREV, b.A(0), PREV])
    else:
        b.sub(PREV, b.mul(PREV, b.F(0)))
    return b.g


def named_families():
    """[(name, GraphEvaluator)]: families 1-11 of the edge corpus"""
    from test_evalh import _many_live_graph
    out = [("sum%d" % n, _sum_chain(n)) for n in range(1, 9)]
    out += [("dbl%d" % n, _dbl_chain(n)) for n in range(1, 5)]
    out += [("wide_mul", _wide_product(False)), ("wide_sqr", _wide_product(True))]
    out += [("0-sum3", _zero_minus_sum())] + [("subchain%d" % n, _sub_chain(n)) for n in range(1, 6)]
    out += [("neg*pos", _neg_times_pos()), ("neg_product", _neg_product())]
    out += [("products%d" % n, _products(n)) for n in (2, 3)]
    out += [("horner%d" % n, _horner(n)) for n in range(0, 7)]
    out += [("fuse_" + k, _fusible(k)) for k in ("add", "sub", "add96", "sub96", "horner")]
    out += [("id_" + k, _identity(k)) for k in IDENTITIES + ("abcd",)]
    out += [("constants", _constants()), ("constants_only", _constants_only())]
    out += [("prev_" + k, _previous(k)) for k in ("mul", "dbl", "horner", "sub")]
    out += [("live%d" % n, _many_live_graph(n)) for n in (2, 6, 12, 40, 100)]
    return out


def random_families():
    """family 12: eight seeded graphs of test_evalh._random_graph.  A random graph's value is its last calculation and most of the graph
    is dead code before it: these are seeds whose compiled program keeps a dozen operations or more"""
    from test_evalh import _random_graph
    out = []
    for seed in RANDOM_SEEDS:
        rng = np.random.default_rng(seed)
        out.append(("random%d" % seed, _random_graph(rng, int(rng.integers(10, 90)))))
    return out


RANDOM_SEEDS = (9001, 9027, 9058, 9061, 9070, 9127, 9139, 9158)


def families():
    return named_families() + random_families()


# the named graphs the generated-kernel GPU leg takes (hiprtc compiles each: about a dozen)
GENERATED = ("sum8", "dbl4", "wide_mul", "subchain5", "neg_product", "products2", "products3", "horner6", "fuse_add", "fuse_sub96",
             "fuse_add96", "fuse_horner", "id_ab-ba", "constants", "prev_horner")


def row_graph_allowed(flat, theta):
    """lookup_compress (theta True) and check_gates (False) run graphs over Lagrange rows, where there is no beta, gamma, y or previous
    value, and for the gate check no theta"""
    banned = {VS_BETA, VS_GAMMA, VS_Y, VS_PREVIOUS} | (set() if theta else {VS_THETA})
    kinds = set(flat["calcs"][:, 2].tolist()) | set(flat["parts"][:, 0].tolist())
    binary = np.isin(flat["calcs"][:, 0], (CALC_ADD, CALC_SUB, CALC_MUL, CALC_HORNER))
    kinds |= set(flat["calcs"][binary, 5].tolist())
    return not (kinds & banned)


def row_families():
    """the families a row graph may hold: those that read only columns, constants and challenges, and the many-live graphs without their
    closing Horner over the previous value"""
    from test_evalh import _many_live_graph
    out = []
    for name, g in families():
        if name.startswith("live"):
            continue
        if row_graph_allowed(flatten_graph(g), theta=False):
            out.append((name, g))
    for n in (2, 6, 12, 40, 100):
        g = _many_live_graph(n)
        g.calculations.pop()
        g.num_intermediates -= 1
        out.append(("live%d-open" % n, g))
    return out


# ---------------------------------------------------------------------------------------------------------- whole systems
# (sets, permuted columns, chunk_len): chunk_len 1, 2 and 3, one and three sets, a ragged last set (5 columns by 2, 7 by 3)
PERM_LAYOUTS = [(1, 1, 1), (3, 3, 1), (3, 5, 2), (1, 3, 3), (3, 7, 3)]
_KIND_CYCLE = [0, 0, 1, 2, 0, 1, 2]  # ANY_ADVICE, ANY_FIXED, ANY_INSTANCE of the permuted columns
N_INSTANCE_SYSTEM = 2                # the systems carry a second instance column, the random control of that group


def poly_column(sc, n, salt, control=False):
    """a column given as a polynomial of n coefficients: the constant polynomial of an extreme word, whose every coset is that word on
    every row -- or, for the control of its group and in the random scenario, a random polynomial"""
    if control or sc[0] == "random":
        return random_words(n, 5000 + 1000 * (sc[1] if isinstance(sc[1], int) else 0) + salt)
    kind, arg = sc
    if kind == "const":
        w = VALUES[arg]
    elif kind == "signs":
        w = (1, R_MOD - 1)[salt & 1]
    else:
        w = _VALUE_LIST[(7 * salt + arg) % len(_VALUE_LIST)]
    out = np.zeros((n, 4), dtype=np.uint64)
    out[0] = eu.words([w])[0]
    return out


def system(oracle, j, k, sc, layout, custom, lookup_graphs, parts_form=False):
    """(case, values on entry) of a whole constraint system under a scenario.  Full form: fixed_cosets, l0, l_last, l_active_row,
    perm_cosets, perm_product_cosets and the incoming values are drawn per row by the scenario; advice, instance and lookup polynomials
    are constant polynomials of an extreme word, the last advice column, the second instance column and the second lookup's
    polynomials random (the controls).  Parts form: the key's columns too are such polynomials (the names of h2hip_evalh_parts_desc).
    beta, gamma, theta, y and the challenges are the word r - 1 (random in the random scenario)."""
    n = 1 << k
    d, _ = oracle.domain_new(j, k)
    size = 1 << d.extended_k
    n_sets, n_cols, chunk_len = layout
    kinds = [_KIND_CYCLE[i % len(_KIND_CYCLE)] for i in range(n_cols)]
    index = [i % (N_ADVICE, N_FIXED, N_INSTANCE_SYSTEM)[kd] for i, kd in enumerate(kinds)]
    key = (lambda salt: poly_column(sc, n, salt)) if parts_form else (lambda salt: column(sc, size, salt))
    lookups = []
    for li, lg in enumerate(lookup_graphs):
        lookups.append((lg,) + tuple(poly_column(sc, n, 50 + 3 * li + t, control=li == 1) for t in range(3)))
    case = {
        "k": k, "extended_k": d.extended_k, "extended_omega": d.fe("extended_omega"), "g_coset": d.fe("g_coset"), "g_coset_inv": d.fe("g_coset_inv"),
        "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
        "y": scalar(sc, 1), "beta": scalar(sc, 2), "gamma": scalar(sc, 3), "theta": scalar(sc, 4),
        "challenges": np.stack([scalar(sc, 40 + i) for i in range(N_CHALLENGES)]),
        "advice_polys": [poly_column(sc, n, 20 + i, control=i == N_ADVICE - 1) for i in range(N_ADVICE)],
        "instance_polys": [poly_column(sc, n, 30 + i, control=i == 1) for i in range(N_INSTANCE_SYSTEM)],
        "custom": custom,
        "perm_column_kind": np.array(kinds, dtype=np.uint32), "perm_column_index": np.array(index, dtype=np.uint32),
        "chunk_len": chunk_len, "last_rotation": -6, "lookups": lookups,
    }
    names = ("fixed_polys", "l0_poly", "l_last_poly", "l_active_row_poly", "perm_product_polys", "perm_polys") if parts_form else (
        "fixed_cosets", "l0", "l_last", "l_active_row", "perm_product_cosets", "perm_cosets")
    case[names[0]] = [key(10 + i) for i in range(N_FIXED)]
    case[names[1]], case[names[2]], case[names[3]] = key(5), key(6), key(7)
    case[names[4]] = [key(60 + i) for i in range(n_sets)]
    case[names[5]] = [key(70 + i) for i in range(n_cols)]
    return case, column(sc, size, 99)


# ---------------------------------------------------------------------------------------------------------- the compiled program
def compiled_program(h2, flat):
    """h2hip_debug_evalh_program of a flattened graph: dict of ops (n, 8) u32, n_slots, result (kind, a, b), mags (n,) f64 and
    fused_on / fused_off (n,) i32"""
    keep = []
    G = graph_struct(flat, keep)
    L = h2.lib()
    n_ops, n_slots, res = ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 3)()
    rc = L.h2hip_debug_evalh_program(ctypes.byref(G), None, ctypes.c_size_t(0), ctypes.byref(n_ops), ctypes.byref(n_slots), res, None, None, None)
    assert rc == 0, L.h2hip_last_error()
    n = n_ops.value
    ops = np.zeros((max(n, 1), 8), dtype=np.uint32)
    mags = np.zeros(max(n, 1), dtype=np.float64)
    on, off = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    rc = L.h2hip_debug_evalh_program(ctypes.byref(G), ops.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), ctypes.byref(n_ops),
                                     ctypes.byref(n_slots), res, mags.ctypes.data_as(ctypes.c_void_p), on.ctypes.data_as(ctypes.c_void_p),
                                     off.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and n_ops.value == n, L.h2hip_last_error()
    return {"ops": ops[:n], "n_slots": n_slots.value, "result": tuple(int(v) for v in res), "mags": mags[:n], "fused_on": on[:n], "fused_off": off[:n]}


# ---------------------------------------------------------------------------------------------------------- Python integers
def eval_graph_ints(flat, cols, n, previous=None, rot_scale=1):
    """GraphEvaluator::evaluate (evaluation.rs:708-749) of a flattened graph on rows 0 .. n - 1, over Python integers: cols as
    scenario_columns gives them (stored words), a rotation moves by rot_scale rows.  -> (n, 4) stored words"""
    f = lambda a: [v * _MONT_INV % R_MOD for v in eu.ints(a)]  # noqa: E731
    tab = {VS_FIXED: [f(c) for c in cols["fixed"]], VS_ADVICE: [f(c) for c in cols["advice"]], VS_INSTANCE: [f(c) for c in cols["instance"]]}
    prev = f(cols["previous"] if previous is None else previous)
    chal = f(cols["challenges"])
    sc = {VS_BETA: f(cols["beta"])[0], VS_GAMMA: f(cols["gamma"])[0], VS_THETA: f(cols["theta"])[0], VS_Y: f(cols["y"])[0]}
    consts, rots = f(flat["constants"]), [int(r) for r in flat["rotations"]]
    calcs, parts = flat["calcs"].tolist(), flat["parts"].tolist()
    out = []
    for row in range(n):
        inter = {}

        def get(k, a, b):
            if k == VS_CONSTANT:
                return consts[a]
            if k == VS_INTERMEDIATE:
                return inter[a]
            if k in tab:
                return tab[k][a][(row + rots[b] * rot_scale) % n]
            if k == VS_CHALLENGE:
                return chal[a]
            return prev[row] if k == VS_PREVIOUS else sc[k]

        last = 0
        for op, target, xk, xa, xb, yk, ya, yb, p0, pn in calcs:
            x = get(xk, xa, xb)
            if op == CALC_ADD:
                v = x + get(yk, ya, yb)
            elif op == CALC_SUB:
                v = x - get(yk, ya, yb)
            elif op == CALC_MUL:
                v = x * get(yk, ya, yb)
            elif op == CALC_SQUARE:
                v = x * x
            elif op == CALC_DOUBLE:
                v = 2 * x
            elif op == CALC_NEGATE:
                v = -x
            elif op == CALC_HORNER:
                yv, v = get(yk, ya, yb), x
                for p in parts[p0:p0 + pn]:
                    v = v * yv + get(*p)
            else:
                v = x
            last = inter[target] = v % R_MOD
        out.append(last * _MONT % R_MOD)
    return eu.words(out)


# ---------------------------------------------------------------------------------------------------------- the host program's file
CORPUS_MAGIC = 0x48564245  # "EBVH"


def _u32(*v):
    return struct.pack("<%dI" % len(v), *v)


def corpus_record(name, flat, prog, cols, log_rows):
    """one (graph, scenario) record: the graph, its compiled program and every operand on 2^log_rows rows"""
    n = 1 << log_rows
    nm = name.encode()[:63]
    rec = [nm + b"\0" * (64 - len(nm))]
    rec.append(_u32(log_rows, len(prog["ops"]), prog["n_slots"], *prog["result"], flat["constants"].shape[0], flat["rotations"].shape[0],
                    flat["calcs"].shape[0], flat["parts"].shape[0], flat["num_intermediates"], len(cols["fixed"]), len(cols["advice"]),
                    len(cols["instance"]), cols["challenges"].shape[0]))
    rec += [np.ascontiguousarray(prog[k]).tobytes() for k in ("ops", "mags", "fused_on", "fused_off")]
    rec += [np.ascontiguousarray(flat["constants"], dtype=np.uint64).tobytes(), np.ascontiguousarray(flat["rotations"], dtype=np.int32).tobytes(),
            np.ascontiguousarray(flat["calcs"], dtype=np.uint32).tobytes(), np.ascontiguousarray(flat["parts"], dtype=np.uint32).tobytes()]
    for key in ("fixed", "advice", "instance"):
        for c in cols[key]:
            assert c.shape == (n, 4)
            rec.append(np.ascontiguousarray(c, dtype=np.uint64).tobytes())
    rec.append(np.ascontiguousarray(cols["challenges"], dtype=np.uint64).tobytes())
    rec += [np.ascontiguousarray(cols[k], dtype=np.uint64).tobytes() for k in ("beta", "gamma", "theta", "y", "previous")]
    return b"".join(rec)


def flagged_product(prog):
    """a copy of a program with the reduce flag set by hand on its products, their magnitudes and those downstream left as tracked (a
    reduction only lowers a value, so every tracked figure still bounds it).  compile_graph itself never flags a product -- its operands
    are below 100, so the product is below 100 * 100 / 169 + 1 = 60.2 -- but the kernels honour the flag on every op kind"""
    p = dict(prog, ops=prog["ops"].copy())
    products = (p["ops"][:, 0] == OP_MUL) | (p["ops"][:, 0] == OP_SQR)
    assert products.any()
    p["ops"][products, 0] |= OP_REDUCE_FLAG
    p["fused_on"] = np.full_like(prog["fused_on"], -1)  # the generator leaves a flagged product where it is
    return p


def write_corpus(path, h2, log_rows=5):
    """the stored words, then every family under every scenario (and the hand-flagged copies of two programs) -> path; returns the number
    of records"""
    n = 1 << log_rows
    scen = [(sc, scenario_columns(sc, n)) for sc in SCENARIOS]
    count = 0
    with open(path, "wb") as fh:
        fh.write(_u32(CORPUS_MAGIC, 0, len(_VALUE_LIST)))
        fh.write(eu.words(_VALUE_LIST).tobytes())
        for name, g in families():
            flat = flatten_graph(g)
            prog = compiled_program(h2, flat)
            variants = [(name, prog)] + ([(name + "+flag", flagged_product(prog))] if name in ("wide_mul", "wide_sqr") else [])
            for vname, p in variants:
                for sc, cols in scen:
                    fh.write(corpus_record(vname + "/" + scenario_id(sc), flat, p, cols, log_rows))
                    count += 1
        fh.seek(4)
        fh.write(_u32(count))
    return count
