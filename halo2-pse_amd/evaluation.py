"""Host-side mirror of halo2_proofs::plonk::evaluation (plonk/evaluation.rs) over the C ABI of include/halo2hip.h.

  GraphEvaluator   the graph builder (evaluation.rs:191-201, :526-706): add_rotation / add_constant / add_calculation /
                   add_expression with the reference's deduplication and operand ordering, so a flattened graph has the
                   same calculations, in the same order, as the reference builds for the same Expression
  Evaluator        Evaluator::new (:221-279) from gate polynomials + lookup argument expressions, and evaluate_h
                   (:280-522) which hands the flattened description to h2hip_evaluate_h_bn254[_device]
  ValueSource / Calculation / Graph / EvalhDesc    ctypes mirrors of the h2hip_* structs;  DescHolder builds one from numpy arrays
  EvalhShuffles / ShufflesHolder / shuffle_graphs / shuffle_required_degree    the shuffle argument of upstream PSE halo2, which is later
                   than the reference (h2hip_evalh_shuffles; the definitions are the header's)
  EvalhMvLookups / MvLookupsHolder / mvlookup_graphs / mvlookup_required_degree    the logUp (mv-lookup) argument of the upstream forks that
                   replaced the permuted-column lookup, also later than the reference (h2hip_evalh_mvlookups; the header's definitions)
  EvalhPartsDesc / PartsDescHolder / Evaluator.evaluate_h_parts    the same one coset of the 2^k domain at a time, every column given
                   as a polynomial of 2^k coefficients (h2hip_evaluate_h_parts_bn254[_device])
  DeviceDescHolder / DevicePartsDescHolder / Evaluator.evaluate_h_device / evaluate_h_parts_device    the same calls over columns that
                   are torch CUDA tensors, queued on a stream (the _device entry points)

Expression trees are tuples:  ('const', int) ('fixed', col, rot) ('advice', col, rot) ('instance', col, rot)
('challenge', i) ('neg', e) ('sum', e, e) ('prod', e, e) ('scaled', e, int)   (plonk/circuit.rs Expression).
ValueSource = (kind, a, b) with the enum order of evaluation.rs:37-60, so tuple comparison equals the derived PartialOrd.
There is no CPU evaluation here: evaluate_h raises if the HIP library or the GPU is missing.
"""
import ctypes

import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
RR = 1 << 256

VS_CONSTANT, VS_INTERMEDIATE, VS_FIXED, VS_ADVICE, VS_INSTANCE, VS_CHALLENGE, VS_BETA, VS_GAMMA, VS_THETA, VS_Y, VS_PREVIOUS = range(11)
CALC_ADD, CALC_SUB, CALC_MUL, CALC_SQUARE, CALC_DOUBLE, CALC_NEGATE, CALC_HORNER, CALC_STORE = range(8)
ANY_ADVICE, ANY_FIXED, ANY_INSTANCE = 0, 1, 2


class GraphEvaluator:
    """GraphEvaluator (evaluation.rs:191-201, Default :526-539)"""

    def __init__(self):
        self.constants = [0, 1, 2]
        self.rotations = []
        self.calculations = []  # (calc tuple, target)
        self.num_intermediates = 0

    def add_rotation(self, rot):                      # :543-552
        if rot in self.rotations:
            return self.rotations.index(rot)
        self.rotations.append(rot)
        return len(self.rotations) - 1

    def add_constant(self, c):                        # :555-564
        c %= R_MOD
        if c in self.constants:
            return (VS_CONSTANT, self.constants.index(c), 0)
        self.constants.append(c)
        return (VS_CONSTANT, len(self.constants) - 1, 0)

    def add_calculation(self, calc):                  # :570-588
        for c, target in self.calculations:
            if c == calc:
                return (VS_INTERMEDIATE, target, 0)
        target = self.num_intermediates
        self.calculations.append((calc, target))
        self.num_intermediates += 1
        return (VS_INTERMEDIATE, target, 0)

    def add_expression(self, e):                      # :591-706
        zero, one, two = (VS_CONSTANT, 0, 0), (VS_CONSTANT, 1, 0), (VS_CONSTANT, 2, 0)
        tag = e[0]
        if tag == 'const':
            return self.add_constant(e[1])
        if tag in ('fixed', 'advice', 'instance'):
            kind = {'fixed': VS_FIXED, 'advice': VS_ADVICE, 'instance': VS_INSTANCE}[tag]
            rot_idx = self.add_rotation(e[2])
            return self.add_calculation((CALC_STORE, (kind, e[1], rot_idx), None, ()))
        if tag == 'challenge':
            return self.add_calculation((CALC_STORE, (VS_CHALLENGE, e[1], 0), None, ()))
        if tag == 'neg':
            if e[1][0] == 'const':
                return self.add_constant(-e[1][1])
            ra = self.add_expression(e[1])
            return ra if ra == zero else self.add_calculation((CALC_NEGATE, ra, None, ()))
        if tag == 'sum':
            a, b = e[1], e[2]
            if b[0] == 'neg':                         # undo subtraction stored as a + (-b)
                ra = self.add_expression(a)
                rb = self.add_expression(b[1])
                if ra == zero:
                    return self.add_calculation((CALC_NEGATE, rb, None, ()))
                if rb == zero:
                    return ra
                return self.add_calculation((CALC_SUB, ra, rb, ()))
            ra = self.add_expression(a)
            rb = self.add_expression(b)
            if ra == zero:
                return rb
            if rb == zero:
                return ra
            return self.add_calculation((CALC_ADD, ra, rb, ()) if ra <= rb else (CALC_ADD, rb, ra, ()))
        if tag == 'prod':
            ra = self.add_expression(e[1])
            rb = self.add_expression(e[2])
            if ra == zero or rb == zero:
                return zero
            if ra == one:
                return rb
            if rb == one:
                return ra
            if ra == two:
                return self.add_calculation((CALC_DOUBLE, rb, None, ()))
            if rb == two:
                return self.add_calculation((CALC_DOUBLE, ra, None, ()))
            if ra == rb:
                return self.add_calculation((CALC_SQUARE, ra, None, ()))
            return self.add_calculation((CALC_MUL, ra, rb, ()) if ra <= rb else (CALC_MUL, rb, ra, ()))
        if tag == 'scaled':
            f = e[2] % R_MOD
            if f == 0:
                return zero
            if f == 1:
                return self.add_expression(e[1])
            cst = self.add_constant(f)
            ra = self.add_expression(e[1])
            return self.add_calculation((CALC_MUL, ra, cst, ()))
        raise ValueError(tag)


def custom_gates_graph(gate_polys):
    """Evaluator::new, custom gates (evaluation.rs:225-239)"""
    g = GraphEvaluator()
    parts = tuple(g.add_expression(p) for p in gate_polys)
    g.add_calculation((CALC_HORNER, (VS_PREVIOUS, 0, 0), (VS_Y, 0, 0), parts))
    return g


def lookup_graph(input_exprs, table_exprs):
    """Evaluator::new, one lookup (evaluation.rs:242-275)"""
    g = GraphEvaluator()

    def evaluate_lc(exprs):
        parts = tuple(g.add_expression(e) for e in exprs)
        return g.add_calculation((CALC_HORNER, (VS_CONSTANT, 0, 0), (VS_THETA, 0, 0), parts))

    cin = evaluate_lc(input_exprs)
    ctab = evaluate_lc(table_exprs)
    right_gamma = g.add_calculation((CALC_ADD, ctab, (VS_GAMMA, 0, 0), ()))
    lc = g.add_calculation((CALC_ADD, cin, (VS_BETA, 0, 0), ()))
    g.add_calculation((CALC_MUL, lc, right_gamma, ()))
    return g


def lookup_compress_graphs(input_exprs, table_exprs):
    """commit_permuted's compression (lookup/prover.rs:90-115) as two graphs, one per side: each expression added with add_expression,
    then Horner(Constant(0), parts, Theta) -- theta^(m-1) e_0 + ... + e_(m-1), lookup_graph's evaluate_lc on a graph of its own"""
    out = []
    for exprs in (input_exprs, table_exprs):
        g = GraphEvaluator()
        parts = tuple(g.add_expression(e) for e in exprs)
        g.add_calculation((CALC_HORNER, (VS_CONSTANT, 0, 0), (VS_THETA, 0, 0), parts))
        out.append(g)
    return tuple(out)


def shuffle_graphs(input_exprs, shuffle_exprs):
    """The two graphs of one shuffle argument (h2hip_evalh_shuffles; upstream PSE halo2's Evaluator::new, the argument is later than the
    reference): per side, add_expression of each expression, Horner(Constant(0), parts, Theta), then Add(that, Gamma) -- the values
    A + gamma and S + gamma.  Returns (input graph, shuffle graph)."""
    out = []
    for exprs in (input_exprs, shuffle_exprs):
        g = GraphEvaluator()
        parts = tuple(g.add_expression(e) for e in exprs)
        compressed = g.add_calculation((CALC_HORNER, (VS_CONSTANT, 0, 0), (VS_THETA, 0, 0), parts))
        g.add_calculation((CALC_ADD, compressed, (VS_GAMMA, 0, 0), ()))
        out.append(g)
    return tuple(out)


def expression_degree(e):
    """Expression::degree (plonk/circuit.rs): a column query counts one, a constant or a challenge nothing"""
    tag = e[0]
    if tag in ('const', 'challenge'):
        return 0
    if tag in ('fixed', 'advice', 'instance'):
        return 1
    if tag in ('neg', 'scaled'):
        return expression_degree(e[1])
    if tag == 'sum':
        return max(expression_degree(e[1]), expression_degree(e[2]))
    if tag == 'prod':
        return expression_degree(e[1]) + expression_degree(e[2])
    raise ValueError(tag)


def shuffle_required_degree(input_exprs, shuffle_exprs):
    """shuffle::Argument::required_degree: 2 + max(1, the degree of every input expression, of every shuffle expression)"""
    if len(input_exprs) != len(shuffle_exprs) or not len(input_exprs):
        raise ValueError("a shuffle has m >= 1 input expressions and as many shuffle expressions")
    return 2 + max([1] + [expression_degree(e) for e in list(input_exprs) + list(shuffle_exprs)])


def mvlookup_graphs(inputs_exprs, table_exprs):
    """The K + 1 graphs of one mv-lookup argument (h2hip_evalh_mvlookups): inputs_exprs is the list of the K input expression tuples that
    share the table.  Per tuple, add_expression of each expression, Horner(Constant(0), parts, Theta), then Add(that, Beta) -- the values
    F_c + beta and T + beta.  Returns (input graph 0, ..., input graph K - 1, table graph)."""
    if not len(inputs_exprs):
        raise ValueError("an mv-lookup argument has K >= 1 input tuples")
    out = []
    for exprs in list(inputs_exprs) + [table_exprs]:
        g = GraphEvaluator()
        parts = tuple(g.add_expression(e) for e in exprs)
        compressed = g.add_calculation((CALC_HORNER, (VS_CONSTANT, 0, 0), (VS_THETA, 0, 0), parts))
        g.add_calculation((CALC_ADD, compressed, (VS_BETA, 0, 0), ()))
        out.append(g)
    return tuple(out)


def mvlookup_required_degree(inputs_exprs, table_exprs):
    """2 + d_t + sum_c d_c: each d the largest degree in that tuple, at least 1 (the third constraint multiplies l_active_row, one row
    of phi or m, tau and every f_c)"""
    if not len(inputs_exprs):
        raise ValueError("an mv-lookup argument has K >= 1 input tuples")
    d = lambda exprs: max([1] + [expression_degree(e) for e in exprs])  # noqa: E731
    return 2 + d(table_exprs) + sum(d(inp) for inp in inputs_exprs)


def gate_check_graphs(gate_polys):
    """The witness check's graphs (h2hip_check_gates_bn254): one per gate polynomial, add_expression of that polynomial alone, its value
    designated by a closing Store calculation -- so a bare query or a constant is a polynomial like any other.  None stands for the
    zero polynomial, an empty graph.  A polynomial shared by several gates (a selector, say) is evaluated once per graph."""
    out = []
    for p in gate_polys:
        g = GraphEvaluator()
        if p is not None:
            g.add_calculation((CALC_STORE, g.add_expression(p), None, ()))
        out.append(g)
    return out


# ------------------------------------------------------------------ flat arrays <-> ctypes
def to_mont_limbs(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (v % R_MOD) * RR % R_MOD
        for j in range(4):
            out[i, j] = (m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def flatten_graph(g):
    """-> dict of numpy arrays: constants (n,4) u64 Montgomery, rotations i32, calcs (n,10) u32, parts (m,3) u32"""
    calcs, parts = [], []
    for (op, x, y, hp), target in g.calculations:
        x = x or (0, 0, 0)
        y = y or (0, 0, 0)
        calcs.append([op, target, *x, *y, len(parts), len(hp)])
        parts.extend(list(p) for p in hp)
    return {
        "constants": to_mont_limbs(g.constants),
        "rotations": np.array(g.rotations, dtype=np.int32).reshape(-1),
        "calcs": np.array(calcs, dtype=np.uint32).reshape(-1, 10),
        "parts": np.array(parts, dtype=np.uint32).reshape(-1, 3),
        "num_intermediates": g.num_intermediates,
    }


class ValueSource(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("a", ctypes.c_uint32), ("b", ctypes.c_uint32)]


class Calculation(ctypes.Structure):
    _fields_ = [("op", ctypes.c_uint32), ("target", ctypes.c_uint32), ("x", ValueSource), ("y", ValueSource),
                ("parts_offset", ctypes.c_uint32), ("parts_count", ctypes.c_uint32)]


class Graph(ctypes.Structure):
    _fields_ = [("constants", ctypes.c_void_p), ("n_constants", ctypes.c_uint32), ("rotations", ctypes.c_void_p),
                ("n_rotations", ctypes.c_uint32), ("calculations", ctypes.c_void_p), ("n_calculations", ctypes.c_uint32),
                ("parts", ctypes.c_void_p), ("n_parts", ctypes.c_uint32), ("num_intermediates", ctypes.c_uint32)]


class EvalhDesc(ctypes.Structure):
    _fields_ = [
        ("k", ctypes.c_uint32), ("extended_k", ctypes.c_uint32),
        ("extended_omega", ctypes.c_void_p), ("g_coset", ctypes.c_void_p), ("g_coset_inv", ctypes.c_void_p),
        ("n_fixed", ctypes.c_uint32), ("n_advice", ctypes.c_uint32), ("n_instance", ctypes.c_uint32), ("n_challenges", ctypes.c_uint32),
        ("fixed_cosets", ctypes.c_void_p), ("advice_polys", ctypes.c_void_p), ("instance_polys", ctypes.c_void_p),
        ("challenges", ctypes.c_void_p),
        ("y", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("theta", ctypes.c_void_p),
        ("l0", ctypes.c_void_p), ("l_last", ctypes.c_void_p), ("l_active_row", ctypes.c_void_p),
        ("custom_gates", Graph),
        ("n_perm_sets", ctypes.c_uint32), ("n_perm_columns", ctypes.c_uint32), ("chunk_len", ctypes.c_uint32),
        ("last_rotation", ctypes.c_int32),
        ("perm_product_cosets", ctypes.c_void_p), ("perm_column_kind", ctypes.c_void_p), ("perm_column_index", ctypes.c_void_p),
        ("perm_cosets", ctypes.c_void_p), ("zeta", ctypes.c_void_p), ("delta", ctypes.c_void_p),
        ("n_lookups", ctypes.c_uint32), ("lookup_graphs", ctypes.c_void_p),
        ("lookup_product_polys", ctypes.c_void_p), ("lookup_permuted_input_polys", ctypes.c_void_p),
        ("lookup_permuted_table_polys", ctypes.c_void_p),
    ]


class EvalhShuffles(ctypes.Structure):
    """h2hip_evalh_shuffles"""
    _fields_ = [("n_shuffles", ctypes.c_uint32), ("graphs", ctypes.c_void_p), ("product_polys", ctypes.c_void_p)]


class EvalhMvLookups(ctypes.Structure):
    """h2hip_evalh_mvlookups"""
    _fields_ = [("n_args", ctypes.c_uint32), ("n_inputs", ctypes.c_void_p), ("graphs", ctypes.c_void_p), ("phi_polys", ctypes.c_void_p),
                ("m_polys", ctypes.c_void_p)]


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _column(a, keep, device):
    """the address of one column for a descriptor, the column appended to `keep`: a contiguous uint64 numpy array for the host forms, a
    contiguous torch CUDA tensor for the _device forms -- never the other, since the engine would read a host address as HBM"""
    if device:
        if not (hasattr(a, "data_ptr") and a.is_cuda and a.is_contiguous()):
            raise TypeError("a _device form takes contiguous torch CUDA tensors for its columns")
        keep.append(a)
        return a.data_ptr() if a.numel() else None
    if hasattr(a, "data_ptr"):
        raise TypeError("a host form takes numpy columns; use the _device form for torch tensors")
    a = np.ascontiguousarray(a, dtype=np.uint64)
    keep.append(a)
    return _ptr(a)


class MvLookupsHolder:
    """Builds an h2hip_evalh_mvlookups from [(flattened graphs: K inputs then the table, phi polynomial, m polynomial)] and keeps every
    buffer alive; byref() of an empty list is NULL, the call without mv-lookups"""

    def __init__(self, arguments, device=False):
        self.keep = []
        s = EvalhMvLookups()
        s.n_args = len(arguments)
        n_graphs = sum(len(gs) for gs, _, _ in arguments)
        graphs = (Graph * max(1, n_graphs))()
        n_inputs = np.array([len(gs) - 1 for gs, _, _ in arguments] or [0], dtype=np.uint32)
        phis, ms, at = [], [], 0
        for gs, phi, m in arguments:
            for g in gs:
                graphs[at] = graph_struct(g, self.keep)
                at += 1
            phis.append(_column(phi, self.keep, device))
            ms.append(_column(m, self.keep, device))
        t_phi = (ctypes.c_void_p * max(1, len(phis)))(*phis)
        t_m = (ctypes.c_void_p * max(1, len(ms)))(*ms)
        self.keep += [graphs, n_inputs, t_phi, t_m]
        s.n_inputs, s.graphs = n_inputs.ctypes.data, ctypes.addressof(graphs)
        s.phi_polys, s.m_polys = ctypes.addressof(t_phi), ctypes.addressof(t_m)
        self.desc = s

    def byref(self):
        return ctypes.byref(self.desc) if self.desc.n_args else None


class ShufflesHolder:
    """Builds an h2hip_evalh_shuffles from [(flattened input graph, flattened shuffle graph, product polynomial (2^k, 4) u64)] and keeps
    every buffer alive; byref() of an empty list is NULL, the call without shuffles"""

    def __init__(self, shuffles, device=False):
        self.keep = []
        s = EvalhShuffles()
        s.n_shuffles = len(shuffles)
        graphs = (Graph * max(1, 2 * len(shuffles)))()
        polys = []
        for j, (g_in, g_sh, poly) in enumerate(shuffles):
            graphs[2 * j] = graph_struct(g_in, self.keep)
            graphs[2 * j + 1] = graph_struct(g_sh, self.keep)
            polys.append(_column(poly, self.keep, device))
        table = (ctypes.c_void_p * max(1, len(polys)))(*polys)
        self.keep += [graphs, table]
        s.graphs, s.product_polys = ctypes.addressof(graphs), ctypes.addressof(table)
        self.desc = s

    def byref(self):
        return ctypes.byref(self.desc) if self.desc.n_shuffles else None


class DescHolder:
    """Builds an EvalhDesc from numpy arrays and keeps every buffer alive.

    case: dict with k, extended_k, extended_omega, g_coset, g_coset_inv, zeta, delta, y, beta, gamma, theta (4,) u64;
    fixed_cosets (nf, size, 4), advice_polys (na, n, 4), instance_polys (ni, n, 4), challenges (nc, 4),
    l0, l_last, l_active_row (size, 4); custom (flattened graph dict);
    perm_product_cosets (ns, size, 4), perm_column_kind / perm_column_index u32, perm_cosets (ncols, size, 4), chunk_len, last_rotation;
    lookups: list of (graph dict, product_poly, permuted_input_poly, permuted_table_poly)"""

    device = False  # DeviceDescHolder: the columns are torch CUDA tensors

    def __init__(self, case):
        self.keep = []
        d = EvalhDesc()
        c = lambda a, dt=np.uint64: self._c(a, dt)  # noqa: E731
        d.k, d.extended_k = int(case["k"]), int(case["extended_k"])
        for f in ("extended_omega", "g_coset", "g_coset_inv", "y", "beta", "gamma", "theta", "zeta", "delta"):
            setattr(d, f, _ptr(c(case[f])))
        d.l0, d.l_last, d.l_active_row = (_column(case[f], self.keep, self.device) for f in ("l0", "l_last", "l_active_row"))
        d.n_fixed, d.fixed_cosets = self._ptr_array(case["fixed_cosets"])
        d.n_advice, d.advice_polys = self._ptr_array(case["advice_polys"])
        d.n_instance, d.instance_polys = self._ptr_array(case["instance_polys"])
        ch = c(case["challenges"])
        d.n_challenges, d.challenges = ch.shape[0] if ch.ndim == 2 else 0, _ptr(ch)
        d.custom_gates = self._graph(case["custom"])
        d.n_perm_sets, d.perm_product_cosets = self._ptr_array(case["perm_product_cosets"])
        d.n_perm_columns, d.perm_cosets = self._ptr_array(case["perm_cosets"])
        d.perm_column_kind = _ptr(c(case["perm_column_kind"], np.uint32))
        d.perm_column_index = _ptr(c(case["perm_column_index"], np.uint32))
        d.chunk_len, d.last_rotation = int(case["chunk_len"]), int(case["last_rotation"])
        lookups = case["lookups"]
        d.n_lookups = len(lookups)
        graphs = (Graph * max(1, len(lookups)))()
        for i, (g, _, _, _) in enumerate(lookups):
            graphs[i] = self._graph(g)
        self.keep.append(graphs)
        d.lookup_graphs = ctypes.addressof(graphs)
        _, d.lookup_product_polys = self._ptr_array([l[1] for l in lookups])
        _, d.lookup_permuted_input_polys = self._ptr_array([l[2] for l in lookups])
        _, d.lookup_permuted_table_polys = self._ptr_array([l[3] for l in lookups])
        self.desc = d

    def _c(self, a, dt=np.uint64):
        a = np.ascontiguousarray(a, dtype=dt)
        self.keep.append(a)
        return a

    def _ptr_array(self, arrs):
        addrs = [_column(a, self.keep, self.device) for a in arrs]
        n = len(addrs)
        p = (ctypes.c_void_p * max(1, n))(*addrs)
        self.keep.append(p)
        return n, ctypes.addressof(p)

    def _graph(self, g):
        return graph_struct(g, self.keep)

    def byref(self):
        return ctypes.byref(self.desc)


# h2hip_evalh_desc field -> its name in h2hip_evalh_parts_desc, where the column is a polynomial of 2^k coefficients
_PARTS_RENAMED = {"fixed_cosets": "fixed_polys", "l0": "l0_poly", "l_last": "l_last_poly", "l_active_row": "l_active_row_poly",
                  "perm_product_cosets": "perm_product_polys", "perm_cosets": "perm_polys"}


class EvalhPartsDesc(ctypes.Structure):
    """h2hip_evalh_parts_desc: h2hip_evalh_desc's fields with every column a coefficient-form polynomial, then the part range and t_evaluations"""
    _fields_ = [(_PARTS_RENAMED.get(name, name), t) for name, t in EvalhDesc._fields_] + [
        ("part_begin", ctypes.c_uint32), ("part_count", ctypes.c_uint32), ("t_evaluations", ctypes.c_void_p)]


class PartsDescHolder(DescHolder):
    """Builds an EvalhPartsDesc from numpy arrays and keeps every buffer alive.

    case: as for DescHolder with the columns under the names of h2hip_evalh_parts_desc -- fixed_polys (nf, n, 4), l0_poly / l_last_poly /
    l_active_row_poly (n, 4), perm_product_polys (ns, n, 4), perm_polys (ncols, n, 4) -- and optionally part_begin, part_count (0, 0 = every
    part) and t_evaluations (P, 4)"""

    def __init__(self, case):
        full = dict(case)
        for old, new in _PARTS_RENAMED.items():
            full[old] = case[new]
        super().__init__(full)
        d = EvalhPartsDesc()
        for name, _ in EvalhDesc._fields_:
            setattr(d, _PARTS_RENAMED.get(name, name), getattr(self.desc, name))
        d.part_begin, d.part_count = int(case.get("part_begin", 0)), int(case.get("part_count", 0))
        t = case.get("t_evaluations")
        d.t_evaluations = None if t is None else _ptr(self._c(t))
        self.desc = d


class DeviceDescHolder(DescHolder):
    """DescHolder for h2hip_evaluate_h_bn254_device: the same case with torch CUDA tensors in place of the numpy columns (the scalars,
    challenges, graphs and pointer tables stay host memory); the tensors are kept alive with the tables"""
    device = True


class DevicePartsDescHolder(PartsDescHolder):
    """PartsDescHolder for h2hip_evaluate_h_parts_bn254_device; t_evaluations stays a host array"""
    device = True


def evaluate_h_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_lookups, parts_form, device_form):
    """HBM the engine allocates for the columns of one evaluate_h call and its copy of `values` (h2hip_evaluate_h_workspace_bytes; no GPU needed)"""
    from . import _check, lib
    out = ctypes.c_size_t()
    _check(lib().h2hip_evaluate_h_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns,
                                                  n_lookups, bool(parts_form), bool(device_form), ctypes.byref(out)),
           "evaluate_h_workspace_bytes")
    return out.value


def evaluate_h_shuffles_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_lookups, n_shuffles,
                                        parts_form, device_form):
    """evaluate_h_workspace_bytes for a call with n_shuffles shuffles (h2hip_evaluate_h_shuffles_workspace_bytes; no GPU needed)"""
    from . import _check, lib
    out = ctypes.c_size_t()
    _check(lib().h2hip_evaluate_h_shuffles_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets,
                                                           n_perm_columns, n_lookups, n_shuffles, bool(parts_form),
                                                           bool(device_form), ctypes.byref(out)),
           "evaluate_h_shuffles_workspace_bytes")
    return out.value


def evaluate_h_ext_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets, n_perm_columns, n_lookups, n_mvlookups,
                                   n_shuffles, parts_form, device_form):
    """evaluate_h_workspace_bytes for a call with n_mvlookups mv-lookup arguments and n_shuffles shuffles
    (h2hip_evaluate_h_ext_workspace_bytes; no GPU needed)"""
    from . import _check, lib
    out = ctypes.c_size_t()
    _check(lib().h2hip_evaluate_h_ext_workspace_bytes(k, extended_k, n_fixed, n_advice, n_instance, n_perm_sets,
                                                      n_perm_columns, n_lookups, n_mvlookups, n_shuffles,
                                                      bool(parts_form), bool(device_form), ctypes.byref(out)),
           "evaluate_h_ext_workspace_bytes")
    return out.value


def graph_struct(g, keep):
    """one flattened graph (flatten_graph dict) -> h2hip_graph; the arrays it points into are appended to `keep`"""
    c = lambda a, dt: keep.append(np.ascontiguousarray(a, dtype=dt)) or keep[-1]  # noqa: E731
    consts, rots = c(g["constants"], np.uint64), c(g["rotations"], np.int32)
    calcs, parts = c(g["calcs"], np.uint32), c(g["parts"], np.uint32)
    G = Graph()
    G.constants, G.n_constants = _ptr(consts), consts.shape[0]
    G.rotations, G.n_rotations = _ptr(rots), rots.shape[0]
    G.calculations, G.n_calculations = _ptr(calcs), calcs.shape[0]
    G.parts, G.n_parts = _ptr(parts), parts.shape[0]
    G.num_intermediates = int(g["num_intermediates"])
    return G


def graph_array(flat_graphs):
    """flattened graphs -> (a ctypes array of h2hip_graph, the list of arrays it points into): keep the second alive while the first is used"""
    keep = []
    arr = (Graph * max(1, len(flat_graphs)))()
    for i, g in enumerate(flat_graphs):
        arr[i] = graph_struct(g, keep)
    return arr, keep


GraphBuilder = GraphEvaluator  # older name used by the tests


class Evaluator:
    """Evaluator (evaluation.rs:182-189): custom_gates + one GraphEvaluator per lookup, and (upstream PSE halo2, later than the
    reference) a pair of GraphEvaluators per shuffle and K + 1 GraphEvaluators per mv-lookup argument."""

    def __init__(self, custom_gates, lookups, shuffles=(), mv_lookups=()):
        self.custom_gates, self.lookups, self.shuffles, self.mv_lookups = custom_gates, lookups, list(shuffles), list(mv_lookups)

    @classmethod
    def new(cls, gate_polys, lookup_arguments=(), shuffle_arguments=(), mvlookup_arguments=()):
        """Evaluator::new (:221-279).  gate_polys: every gate's polynomials in cs.gates order, flattened;
        lookup_arguments: [(input_expressions, table_expressions)]; shuffle_arguments: [(input_expressions, shuffle_expressions)];
        mvlookup_arguments: [([input_expressions, ...], table_expressions)], several input tuples sharing one table"""
        return cls(custom_gates_graph(list(gate_polys)), [lookup_graph(i, t) for i, t in lookup_arguments],
                   [shuffle_graphs(i, s) for i, s in shuffle_arguments], [mvlookup_graphs(i, t) for i, t in mvlookup_arguments])

    def describe_mvlookups(self, case, device=False):
        """the mv-lookup stage of a call: case["mvlookups"], when present, holds one (phi polynomial, m polynomial) pair of (2^k, 4) u64
        per mv-lookup argument of this Evaluator, in order.  None: the case has no such entry."""
        polys = case.get("mvlookups")
        if polys is None:
            return None
        if len(polys) != len(self.mv_lookups):
            raise ValueError("mvlookups: expected %d (phi, m) pairs, got %d" % (len(self.mv_lookups), len(polys)))
        return MvLookupsHolder([([flatten_graph(g) for g in gs], phi, m) for gs, (phi, m) in zip(self.mv_lookups, polys)], device)

    def describe_shuffles(self, case, device=False):
        """the shuffle stage of a call: case["shuffles"], when present, holds one product polynomial (2^k, 4) u64 per shuffle of this
        Evaluator, in order.  None: the case has no such entry and the call is the one without shuffles."""
        polys = case.get("shuffles")
        if polys is None:
            return None
        if len(polys) != len(self.shuffles):
            raise ValueError("shuffles: expected %d product polynomials, got %d" % (len(self.shuffles), len(polys)))
        return ShufflesHolder([(flatten_graph(gi), flatten_graph(gs), z) for (gi, gs), z in zip(self.shuffles, polys)], device)

    def describe(self, case, device=False):
        """case as for DescHolder minus `custom` and the graphs inside `lookups` (3-tuples of polynomials there); device: the columns
        are torch CUDA tensors (DeviceDescHolder)"""
        full = dict(case)
        full["custom"] = flatten_graph(self.custom_gates)
        full["lookups"] = [(flatten_graph(g), *polys) for g, polys in zip(self.lookups, case["lookups"])]
        return DeviceDescHolder(full) if device else DescHolder(full)

    def describe_parts(self, case, device=False):
        """case as for PartsDescHolder minus `custom` and the graphs inside `lookups`"""
        full = dict(case)
        full["custom"] = flatten_graph(self.custom_gates)
        full["lookups"] = [(flatten_graph(g), *polys) for g, polys in zip(self.lookups, case["lookups"])]
        return DevicePartsDescHolder(full) if device else PartsDescHolder(full)

    @staticmethod
    def _device_values(d_values, extended_k, stream):
        import torch
        if not (hasattr(d_values, "data_ptr") and d_values.is_cuda and d_values.is_contiguous()):
            raise TypeError("d_values: a contiguous torch CUDA tensor")
        if d_values.numel() * d_values.element_size() != 32 << int(extended_k):
            raise ValueError("d_values: expected 2^extended_k elements of 32 bytes")
        s = torch.cuda.current_stream().cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        return ctypes.c_void_p(d_values.data_ptr()), ctypes.c_void_p(s)

    def evaluate_h_device(self, case, d_values, stream=None):
        """evaluate_h with every column resident in HBM: `case` has evaluate_h's keys with torch CUDA tensors (n x 32 B each) in place
        of the numpy columns, d_values (2^extended_k x 32 B) is folded in place.  The kernels are queued on `stream` (a torch stream or
        a raw handle; None: the current stream) and not waited for; the holder keeps the tensors and pointer tables alive until the
        call has returned, and the caller keeps the tensors until the stream has passed the call."""
        from . import _check, lib
        h = self.describe(case, device=True)
        pv, ps = self._device_values(d_values, case["extended_k"], stream)
        sh, mv = self.describe_shuffles(case, True), self.describe_mvlookups(case, True)
        if mv is not None:
            _check(lib().h2hip_evaluate_h_ext_bn254_device(h.byref(), mv.byref(), sh.byref() if sh is not None else None, pv, ps),
                   "evaluate_h_ext_device")
        elif sh is not None:
            _check(lib().h2hip_evaluate_h_shuffles_bn254_device(h.byref(), sh.byref(), pv, ps), "evaluate_h_shuffles_device")
        else:
            _check(lib().h2hip_evaluate_h_bn254_device(h.byref(), pv, ps), "evaluate_h_device")
        del h, sh, mv
        return d_values

    def evaluate_h_parts_device(self, case, d_values, parts=None, t_evaluations=None, stream=None):
        """evaluate_h_parts with every coefficient-form column resident in HBM (torch CUDA tensors under evaluate_h_parts' keys);
        parts and t_evaluations (a host array) as there.  Queued on `stream`, not waited for."""
        from . import _check, lib
        full = dict(case)
        if parts is not None:
            full["part_begin"], full["part_count"] = parts
        if t_evaluations is not None:
            full["t_evaluations"] = t_evaluations
        h = self.describe_parts(full, device=True)
        pv, ps = self._device_values(d_values, case["extended_k"], stream)
        sh, mv = self.describe_shuffles(case, True), self.describe_mvlookups(case, True)
        if mv is not None:
            _check(lib().h2hip_evaluate_h_parts_ext_bn254_device(h.byref(), mv.byref(), sh.byref() if sh is not None else None, pv, ps),
                   "evaluate_h_parts_ext_device")
        elif sh is not None:
            _check(lib().h2hip_evaluate_h_parts_shuffles_bn254_device(h.byref(), sh.byref(), pv, ps), "evaluate_h_parts_shuffles_device")
        else:
            _check(lib().h2hip_evaluate_h_parts_bn254_device(h.byref(), pv, ps), "evaluate_h_parts_device")
        del h, sh, mv
        return d_values

    def evaluate_h_parts(self, case, values, parts=None, t_evaluations=None):
        """evaluate_h for one circuit instance, one coset of the 2^k domain at a time, from coefficient-form columns: values
        (2^extended_k, 4) u64 is folded in place and returned.  parts: (first, count) of the 2^(extended_k - k) parts to compute, None for
        all -- the rows of the others are left as they are; t_evaluations: EvaluationDomain.t_evaluations on the last instance's call, which
        then returns divide_by_vanishing_poly(h)"""
        from . import _check, lib
        full = dict(case)
        if parts is not None:
            full["part_begin"], full["part_count"] = parts
        if t_evaluations is not None:
            full["t_evaluations"] = t_evaluations
        h = self.describe_parts(full)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        sh, mv = self.describe_shuffles(case), self.describe_mvlookups(case)
        if mv is not None:
            _check(lib().h2hip_evaluate_h_parts_ext_bn254(h.byref(), mv.byref(), sh.byref() if sh is not None else None,
                                                          values.ctypes.data_as(ctypes.c_void_p)), "evaluate_h_parts_ext")
            return values
        if sh is not None:
            _check(lib().h2hip_evaluate_h_parts_shuffles_bn254(h.byref(), sh.byref(), values.ctypes.data_as(ctypes.c_void_p)),
                   "evaluate_h_parts_shuffles")
            return values
        _check(lib().h2hip_evaluate_h_parts_bn254(h.byref(), values.ctypes.data_as(ctypes.c_void_p)), "evaluate_h_parts")
        return values

    def evaluate_h(self, case, values):
        """evaluate_h for one circuit instance (:280-522): values (2^extended_k, 4) u64 is folded in place and returned.  A "shuffles"
        entry of the case (one product polynomial per shuffle of this Evaluator) adds the shuffle stage after the lookups."""
        from . import _check, lib
        h = self.describe(case)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        sh, mv = self.describe_shuffles(case), self.describe_mvlookups(case)
        if mv is not None:
            _check(lib().h2hip_evaluate_h_ext_bn254(h.byref(), mv.byref(), sh.byref() if sh is not None else None,
                                                    values.ctypes.data_as(ctypes.c_void_p)), "evaluate_h_ext")
            return values
        if sh is not None:
            _check(lib().h2hip_evaluate_h_shuffles_bn254(h.byref(), sh.byref(), values.ctypes.data_as(ctypes.c_void_p)), "evaluate_h_shuffles")
            return values
        _check(lib().h2hip_evaluate_h_bn254(h.byref(), values.ctypes.data_as(ctypes.c_void_p)), "evaluate_h")
        return values
