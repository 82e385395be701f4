"""create_proof for the reference's PLONK-over-KZG protocol (halo2_proofs/src/plonk/prover.rs:41-651), composed from the engine's entry
points, with every column resident in HBM from the first commit to the last opening.

  ConstraintSystem   a plain description of plonk/circuit.rs's ConstraintSystem: column counts, phases, gate polynomials, lookup
                     arguments, shuffles, mv-lookups and permutation columns as the expression tuples of evaluation.py; degree
                     (:1974-2002), blinding_factors (:2006-2031), phases (:1962-1970) and the query lists (query_*_index :1571-1627)
                     are derived from it
  ProvingKey.build   keygen_vk + keygen_pk's columns through keygen_columns, uploaded once; the fixed and permutation commitments are
                     the verifying key (VerifyingKey)
  create_proof       prover.rs, step by step (the line numbers are beside each step), with lookup/prover.rs, permutation/prover.rs and
                     vanishing/prover.rs in their places and the multiopen provers of poly/kzg/multiopen/{gwc,shplonk}/prover.rs at the end

Both KZG provers set QUERY_INSTANCE = false (gwc/prover.rs, shplonk/prover.rs:111), so instance values go into the transcript as scalars
(prover.rs:90-93) and instance columns are neither committed nor opened.  multiopen="ipa" (params an ipa.ParamsIPA, the key built over
them) is the QUERY_INSTANCE = true branch (poly/ipa/multiopen/prover.rs:25): instance columns are committed with Blind::default() = 1 and
the commitments absorbed (:100-117), their evaluations written before the advice evaluations (:521-541) and opened first within each
instance (:607-617); every commitment is MSM + [blind] W (the + [blind] W through h2hip_g1_linear_combinations_bn254 on the host), every
query carries its commitment's blind, and ipa.ProverIPA goes on with the same FrRng.

Later arguments.  The shuffle argument (upstream PSE halo2) and the logUp "mv-lookup" argument (the forks that replaced the permuted-column
lookup) are later than the reference; both coexist with the halo2 lookup here, as they do in h2hip_evaluate_h_ext_*.  ARGUMENT_STAGES
lists every stage between theta and y in the order it runs, each with its per-instance loop outermost:
  theta | permuted columns A', S' of the halo2 lookups | mv-lookup multiplicities m | beta, gamma | permutation products | lookup products
        | mv-lookup grand sums phi | shuffle products z | random polynomial | y
h(X) folds gates, permutation, halo2 lookups, mv-lookups, shuffles (include/halo2hip.h); evaluations and opening queries follow the
lookups' in the same order: per mv-lookup phi(x), phi(wx), m(x), then per shuffle z(x), z(wx).  Like the reference's arguments, the prover
does not check that a shuffle's product ends in one: the proof is made and the verifier refuses it.  An mv-lookup input its table lacks
raises H2HipLookupError, as a halo2 lookup's does.

Query order.  The reference registers a query the first time configure() asks for it.  A plain description has no configure(), so the order
is fixed here as that of a configure() which enables equality on the permutation columns first (enable_equality queries Rotation::cur,
:1516-1520), then creates the gates in order (each polynomial read left to right), then the lookups (input expressions, then table
expressions), then the mv-lookups (each argument's input tuples in order, then its table), then the shuffles (input expressions, then
shuffle expressions).  Prover and verifier derive the same lists from the same description.

Random draws.  Everything random comes from one FrRng(seed) (ChaCha20, one 64-byte block per Fr::random), in the reference's order:
  1. per phase, per instance: (b + 1) blinding rows for each advice column of the phase, column by column (prover.rs:350-354), then one
     commitment blind per column (:357-360)
  2. per instance, per lookup: 2(b + 1) rows for A' and S' (permute_expression_pair, lookup/prover.rs:391-475), then the two commitment
     blinds (:129)
  2b. per instance, per mv-lookup: one commitment blind for m (m has no blinding rows: its rows u .. n - 1 are zero)
  3. per instance, per permutation set: b rows of z (permutation/prover.rs:162-164), then its blind (:168)
  4. per instance, per lookup: b rows of z (lookup/prover.rs:247), then its blind (:290)
  4b. per instance, per mv-lookup: b rows of phi, then its blind
  4c. per instance, per shuffle: b rows of z, then its blind
  5. the 2^k coefficients of the vanishing argument's random polynomial, drawn in HBM (vanishing/prover.rs:50-53), then its blind (:55)
  6. one blind per piece of h(X) (vanishing/prover.rs:95-98)
The KZG commitment ignores its blind (poly/kzg/commitment.rs:281-292), as ParamsKZG does here; the blinds are drawn to keep the stream in
step.  The IPA commitment is MSM + [blind] W, and the opening continues the stream (ipa.py lists its draws).  A proof is valid for the verifier of verifier.py; it is not byte-identical to a Rust run, whose rng is not ChaCha20 from this seed.

Residency.  With resident=True no array of 2^k or more field elements is passed to or returned by any call made here: witness() hands over
torch CUDA tensors, which this prover blinds, commits, transforms (in place: they are consumed) and opens where they lie.  What does cross
is listed in proof.transfers as (direction, bytes, what): instance values, blinding rows, challenges and points upwards, commitments and
evaluations downwards.  The engine's own staging inside a call is not counted.  resident=False runs the same steps on numpy columns
through the host forms and lists every column those calls take or return.

No step of create_proof that touches all 2^k rows of a column lacked an entry point: torch is used for allocation, zero-fill, slicing
and copies only, numpy likewise on the host path."""
import ctypes

import numpy as np

from . import (FR_DELTA, FR_MODULUS, FR_ZETA, CopyList, EvaluationDomain, FrRng, H2HipError, _check, _dptr, _stream, best_multiexp_batch,
               columns_pin, columns_unpin, commit_permuted, eval_polynomials, eval_polynomials_device, extended_to_coeff_device, fr_from_int,
               fr_random, fr_to_int, g1_to_affine, g1_to_bytes, gwc_witnesses, ifft_batch_device, coeff_to_extended_batch_device,
               keygen_columns, lib, lookup_compress, lookup_compress_device, lookup_permute_device, lookup_products, lookup_products_device,
               msm_batch_device, mvlookup_multiplicities, mvlookup_multiplicities_device, mvlookup_sums, mvlookup_sums_device,
               part_cosets_pin, part_cosets_unpin, permutation_products, permutation_products_device, poly_combine, poly_combine_device,
               shplonk_final, shplonk_h, shuffle_products, shuffle_products_device, bases_pin_device, g1_linear_combinations)
from .evaluation import (ANY_ADVICE, ANY_FIXED, ANY_INSTANCE, Evaluator, expression_degree, flatten_graph, lookup_compress_graphs,
                         mvlookup_required_degree, shuffle_required_degree)
from .transcript import point_from_bytes

# the stages create_proof runs between theta and y, in order (beta and gamma are squeezed after "mvlookup_multiplicities"); each stage
# enters its name into proof.stages as it starts, and tests/test_proof_arguments.py compares that list, and the order of the stages'
# commitments in proof.transfers, with this one
ARGUMENT_STAGES = ("lookup_permuted", "mvlookup_multiplicities", "permutation_products", "lookup_products", "mvlookup_sums", "shuffle_products")
_ANY = {"advice": ANY_ADVICE, "fixed": ANY_FIXED, "instance": ANY_INSTANCE}
ZERO = ("const", 0)


class ConstraintSystem:
    """plonk/circuit.rs ConstraintSystem as data.  gates: every gate's polynomials in cs.gates order, flattened (None is the zero
    polynomial); lookups: [(input_exprs, table_exprs)]; permutation: [(kind, index)] with kind 'advice' / 'fixed' / 'instance';
    advice_column_phase[c] / challenge_phase[j]: the phase of advice column c / challenge j (default: everything in phase 0).
    shuffles: [(input_exprs, shuffle_exprs)], m >= 1 expressions a side; mv_lookups: [([input_exprs, ...], table_exprs)], K in [1, 255]
    input tuples sharing one table, every tuple as long as the table's."""

    def __init__(self, num_fixed_columns, num_advice_columns, num_instance_columns, gates, lookups=(), permutation=(),
                 advice_column_phase=None, challenge_phase=(), minimum_degree=None, shuffles=(), mv_lookups=()):
        self.num_fixed_columns, self.num_advice_columns = int(num_fixed_columns), int(num_advice_columns)
        self.num_instance_columns = int(num_instance_columns)
        self.gates = list(gates)
        self.lookups = [(list(i), list(t)) for i, t in lookups]
        self.shuffles = [(list(i), list(s)) for i, s in shuffles]
        self.mv_lookups = [([list(i) for i in inputs], list(t)) for inputs, t in mv_lookups]
        self.permutation = [(str(kind), int(i)) for kind, i in permutation]
        self.advice_column_phase = [0] * self.num_advice_columns if advice_column_phase is None else [int(p) for p in advice_column_phase]
        self.challenge_phase = [int(p) for p in challenge_phase]
        self.num_challenges = len(self.challenge_phase)
        self.minimum_degree = minimum_degree
        if len(self.advice_column_phase) != self.num_advice_columns:
            raise ValueError("advice_column_phase: one phase per advice column")
        for inp, tab in self.lookups:
            if len(inp) != len(tab) or not inp:
                raise ValueError("a lookup has m >= 1 input expressions and as many table expressions")
        for inp, shf in self.shuffles:
            if len(inp) != len(shf) or not inp:
                raise ValueError("a shuffle has m >= 1 input expressions and as many shuffle expressions")
        for inputs, tab in self.mv_lookups:
            if not 1 <= len(inputs) <= 255:
                raise ValueError("an mv-lookup argument has K in [1, 255] input tuples")
            if not tab or any(len(inp) != len(tab) for inp in inputs):
                raise ValueError("an mv-lookup's table has m >= 1 expressions and every input tuple as many")
        counts = {"advice": self.num_advice_columns, "fixed": self.num_fixed_columns, "instance": self.num_instance_columns}
        self.advice_queries, self.fixed_queries, self.instance_queries = [], [], []
        pools = {"advice": self.advice_queries, "fixed": self.fixed_queries, "instance": self.instance_queries}

        def query(kind, column, rotation):  # query_*_index :1571-1615
            if not 0 <= column < counts[kind]:
                raise ValueError("%s column %d is not in the constraint system" % (kind, column))
            if (column, rotation) not in pools[kind]:
                pools[kind].append((column, rotation))

        def walk(e):
            tag = e[0]
            if tag in pools:
                query(tag, int(e[1]), int(e[2]))
            elif tag == "challenge":
                if not 0 <= e[1] < self.num_challenges:
                    raise ValueError("challenge %d is not in the constraint system" % e[1])
            elif tag in ("neg", "scaled"):
                walk(e[1])
            elif tag in ("sum", "prod"):
                walk(e[1])
                walk(e[2])
            elif tag != "const":
                raise ValueError(tag)

        for kind, i in self.permutation:                 # enable_equality :1516-1520
            if kind not in pools:
                raise ValueError("permutation column kind %r" % (kind,))
            query(kind, i, 0)
        for p in self.gates:
            if p is not None:
                walk(p)
        for inp, tab in self.lookups:
            for e in inp + tab:
                walk(e)
        for inputs, tab in self.mv_lookups:
            for e in [e for inp in inputs for e in inp] + tab:
                walk(e)
        for inp, shf in self.shuffles:
            for e in inp + shf:
                walk(e)
        self.num_advice_queries = [sum(1 for c, _ in self.advice_queries if c == j) for j in range(self.num_advice_columns)]  # :1597

    def gate_polynomials(self):
        """the gate polynomials with the zero polynomial written out, as Evaluator.new and the verifier take them"""
        return [ZERO if p is None else p for p in self.gates]

    def degree(self):
        """:1974-2002"""
        degree = 3                                                                       # permutation.required_degree, permutation.rs:34-67
        degree = max(degree, max([max(4, 2 + max([1] + [expression_degree(e) for e in inp]) + max([1] + [expression_degree(e) for e in tab]))
                                  for inp, tab in self.lookups] or [1]))                 # lookup.rs:37-97
        degree = max([degree] + [shuffle_required_degree(inp, shf) for inp, shf in self.shuffles])
        degree = max([degree] + [mvlookup_required_degree(inputs, tab) for inputs, tab in self.mv_lookups])
        degree = max(degree, max([expression_degree(p) for p in self.gates if p is not None] or [0]))
        return max(degree, self.minimum_degree or 1)

    def blinding_factors(self):
        """:2006-2031"""
        return max(3, max(self.num_advice_queries or [1])) + 2

    def chunk_len(self):
        """permutation/prover.rs:72"""
        return self.degree() - 2

    def num_permutation_sets(self):
        return -(-len(self.permutation) // self.chunk_len())

    def phases(self):
        """:1962-1970"""
        return range(max(self.advice_column_phase or [0]) + 1)

    def query_index(self, kind, column, rotation):
        """get_any_query_index"""
        return {"advice": self.advice_queries, "fixed": self.fixed_queries, "instance": self.instance_queries}[kind].index((column, rotation))


class VerifyingKey:
    """plonk.rs VerifyingKey as far as verify_proof reads it: the constraint system, k, the fixed and permutation commitments (affine
    points as integer pairs) and the caller's vk_repr, which stands in for transcript_repr"""

    def __init__(self, cs, k, vk_repr, fixed_commitments, permutation_commitments, scheme="kzg"):
        self.cs, self.k, self.vk_repr, self.scheme = cs, int(k), int(vk_repr) % FR_MODULUS, scheme  # scheme: "kzg" or "ipa" params
        self.fixed_commitments, self.permutation_commitments = list(fixed_commitments), list(permutation_commitments)
        self.cs_degree = cs.degree()


def points_to_ints(jacobian):
    """engine points ((count, 12) Jacobian limbs) -> affine integer pairs, through g1_to_bytes as a proof carries them"""
    if not len(jacobian):
        return []
    affine = np.stack([g1_to_affine(p) for p in jacobian])
    return [point_from_bytes(row.tobytes()) for row in g1_to_bytes(affine)]


def _is_ipa(params):
    from . import ipa  # ipa.py imports verifier.py, which imports this module
    return isinstance(params, ipa.ParamsIPA)


def _lagrange_unit_columns(n, b):
    """l_0, l_last and l_active_row = 1 - l_last - l_blind as Lagrange columns (plonk/keygen.rs:320-351): units and an indicator"""
    one = fr_from_int(1)
    l0, l_last, l_active = (np.zeros((n, 4), dtype=np.uint64) for _ in range(3))
    l0[0] = one
    l_last[n - b - 1] = one
    l_active[:n - b - 1] = one
    return l0, l_last, l_active


class ProvingKey:
    """plonk.rs ProvingKey: the key's columns in every form create_proof reads, as torch CUDA tensors (`dev`) and as the numpy arrays
    keygen_columns returned (`host`, for resident=False), under the names of evaluation.py's cases"""

    @classmethod
    def build(cls, params, cs, fixed, copies_or_mapping, vk_repr, pin=True):
        """params: a ParamsKZG, or an ipa.ParamsIPA (the key then commits with Blind::default() = 1 and shares the params' pinned
        generators); fixed: the (2^k, 4) Lagrange columns; copies_or_mapping: a CopyList, a list or (C, 4) array of (column, row, column, row)
        copy constraints over cs.permutation, or the assembly's (m, 2^k, 2) mapping; vk_repr: the scalar the transcript starts with.
        pin: keep the part cosets (parts form) and, for the host forms, the extended cosets of the key's columns in HBM."""
        import torch
        self = cls()
        k, n = int(params.k), 1 << int(params.k)
        b = cs.blinding_factors()
        if n < b + 3:
            raise H2HipError("not enough rows available: k = %d" % k)                    # minimum_rows, circuit.rs:2035-2043
        if len(fixed) != cs.num_fixed_columns:
            raise ValueError("fixed: expected %d columns" % cs.num_fixed_columns)
        domain = EvaluationDomain.new(cs.degree(), k)
        m = len(cs.permutation)
        mapping, copies = None, None
        if isinstance(copies_or_mapping, np.ndarray) and copies_or_mapping.ndim == 3:
            mapping = copies_or_mapping
        elif isinstance(copies_or_mapping, CopyList):
            copies = copies_or_mapping
        else:
            copies = (m, np.asarray(copies_or_mapping if copies_or_mapping is not None and len(copies_or_mapping) else np.zeros((0, 4)),
                                    dtype=np.uint32).reshape(-1, 4))
        if m == 0:
            mapping, copies = np.zeros((0, n, 2), dtype=np.uint32), None
        host = keygen_columns(params, domain, fixed, mapping, b, copies=copies)
        units = _lagrange_unit_columns(n, b)
        host["l0_poly"], host["l_last_poly"], host["l_active_row_poly"] = domain.lagrange_to_coeff_batch(list(units))
        self.params, self.cs, self.domain, self.k, self.n, self.b, self.u = params, cs, domain, k, n, b, n - b - 1
        self.vk_repr = int(vk_repr) % FR_MODULUS
        self.host = host
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()  # noqa: E731
        self.dev = {key: ([up(a) for a in val] if isinstance(val, list) else up(val)) for key, val in host.items()
                    if key not in ("fixed_commitments", "permutation_commitments")}
        self.scheme = "ipa" if _is_ipa(params) else "kzg"
        if self.scheme == "ipa":
            # the params' own resident, pinned generators; and commit_lagrange(col, Blind::default()) with Blind::default() = one
            # (poly/commitment.rs:195-199, plonk/keygen.rs:249, plonk/permutation/keygen.rs:159): each key commitment is the MSM plus W
            self.d_g, self.d_g_lagrange = params.d_g(), params.d_g_lagrange()
            key_commitments = [g1_linear_combinations(host[name], [[1]] * len(host[name]), [params.w]) if len(host[name]) else []
                               for name in ("fixed_commitments", "permutation_commitments")]
        else:
            self.d_g, self.d_g_lagrange = up(params.g), up(params.g_lagrange)
            bases_pin_device(self.d_g, n)
            bases_pin_device(self.d_g_lagrange, n)
            key_commitments = [points_to_ints(host["fixed_commitments"]), points_to_ints(host["permutation_commitments"])]
        self.ev = Evaluator.new(cs.gate_polynomials(), cs.lookups, shuffle_arguments=cs.shuffles, mvlookup_arguments=cs.mv_lookups)
        self.vk = VerifyingKey(cs, k, self.vk_repr, key_commitments[0], key_commitments[1], scheme=self.scheme)
        self._pinned = False
        if pin:
            self.pin()
        return self

    def _key_polys(self, where):
        return list(where["fixed_polys"]) + [where["l0_poly"], where["l_last_poly"], where["l_active_row_poly"]] + list(where["perm_polys"])

    def _key_cosets(self):
        return list(self.host["fixed_cosets"]) + [self.host["l0"], self.host["l_last"], self.host["l_active_row"]] + list(self.host["perm_cosets"])

    def pin(self):
        if not self._pinned:
            part_cosets_pin(self._key_polys(self.dev), self.domain)
            part_cosets_pin(self._key_polys(self.host), self.domain)
            columns_pin(self._key_cosets())
            self._pinned = True

    def close(self):
        """drop the pins (idempotent); the host entries are keyed by addresses numpy may hand out again"""
        if getattr(self, "_pinned", False):
            self._pinned = False
            for undo, cols in ((part_cosets_unpin, self._key_polys(self.dev)), (part_cosets_unpin, self._key_polys(self.host)),
                               (columns_unpin, self._key_cosets())):
                try:
                    undo(cols)
                except H2HipError:
                    pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Proof:
    """what create_proof returns: the proof bytes, the host/device moves the prover made, (direction, bytes, what), and the stages it
    ran between theta and y, in order (ARGUMENT_STAGES names them)"""

    def __init__(self):
        self.bytes, self.transfers, self.challenges, self.stages = b"", [], {}, []

    def total(self, direction):
        return sum(nbytes for d, nbytes, _ in self.transfers if d == direction)


# ------------------------------------------------------------------ the two homes of a column
class _Device:
    """columns are torch CUDA tensors (n, 4) int64; every call is the _device form, queued on the current stream"""
    resident = True

    def __init__(self, pk, proof):
        import torch
        self.torch, self.pk, self.key, self.proof = torch, pk, pk.dev, proof
        self.dom, self.k, self.n, self.b = pk.domain, pk.k, pk.n, pk.b

    def note(self, direction, nbytes, what):
        if nbytes:
            self.proof.transfers.append((direction, int(nbytes), what))

    def check_column(self, col, rows):
        t = self.torch
        if not (isinstance(col, t.Tensor) and col.is_cuda and col.is_contiguous() and col.numel() * col.element_size() == 32 * rows):
            raise TypeError("resident=True: a column is a contiguous torch CUDA tensor of %d x 32 bytes" % rows)

    def zeros(self, rows):
        return self.torch.zeros((rows, 4), dtype=self.torch.int64, device="cuda")

    def clone(self, col):
        return col.clone()

    def set_rows(self, col, start, values, what):
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        col.view(-1, 4)[start:start + values.shape[0]] = self.torch.from_numpy(values.view(np.int64)).to(col.device)
        self.note("h2d", values.nbytes, what)

    def commit(self, cols, lagrange, what, blinds=None):
        """Jacobian sums; with blinds (IPA: poly/ipa/commitment.rs:92-107, :216-227) the commitments MSM + [r] W as affine integer
        pairs.  Either way the MSM is the _device batch and 96 B per commitment come back"""
        if not cols:
            return []
        out = msm_batch_device(cols, self.pk.d_g_lagrange if lagrange else self.pk.d_g, cols[0].numel() * cols[0].element_size() // 32)
        self.note("d2h", out.nbytes, what)
        return list(out) if blinds is None else g1_linear_combinations(out, [[r] for r in blinds], [self.pk.params.w])

    def lagrange_to_coeff(self, cols):
        """in place"""
        if cols:
            ifft_batch_device(cols, self.dom.omega_inv, self.k, self.dom.ifft_divisor)
        return cols

    def coeff_to_extended(self, polys):
        outs = []
        for p in polys:
            e = self.zeros(self.dom.extended_len())
            e[:self.n] = p.view(-1, 4)
            outs.append(e)
        if outs:
            d = self.dom
            coeff_to_extended_batch_device(outs, d.k, d.extended_k, d.extended_omega, d.g_coset, d.g_coset_inv)
        return outs

    def commit_permuted(self, lookups, theta, blinding, fixed, advice, instance, challenges, blinds=None):
        """lookup::Argument::commit_permuted (lookup/prover.rs:64-158) for every lookup of one instance, the composition of the host
        commit_permuted over the _device entry points; blinds as for commit, two per lookup"""
        graphs = []
        for inp, tab in lookups:
            gi, gt = lookup_compress_graphs(inp, tab)
            graphs += [flatten_graph(gi), flatten_graph(gt)]
        comp = self.compress(graphs, theta, fixed, advice, instance, challenges, "lookup_compress")        # :90-115
        pa, pt = [self.zeros(self.n) for _ in lookups], [self.zeros(self.n) for _ in lookups]
        self.note("h2d", blinding.nbytes, "lookup blinding rows")
        lookup_permute_device(self.k, comp[0::2], comp[1::2], blinding, self.b, pa, pt)                    # :118-126
        coms = self.commit([c for j in range(len(lookups)) for c in (pa[j], pt[j])], True, "permuted commitments", blinds)  # :129-140
        polys = self.lagrange_to_coeff([c.clone() for j in range(len(lookups)) for c in (pa[j], pt[j])])
        return [{"compressed_input": comp[2 * j], "compressed_table": comp[2 * j + 1], "permuted_input": pa[j], "permuted_table": pt[j],
                 "permuted_input_commitment": coms[2 * j], "permuted_table_commitment": coms[2 * j + 1],
                 "permuted_input_poly": polys[2 * j], "permuted_table_poly": polys[2 * j + 1]} for j in range(len(lookups))]

    def permutation_products(self, beta, gamma, columns, chunk_len, n_sets, blinding):
        z = [self.zeros(self.n) for _ in range(n_sets)]
        self.note("h2d", 64 + blinding.nbytes, "beta, gamma and permutation blinding rows")
        permutation_products_device(self.k, self.dom.omega, fr_from_int(FR_DELTA), beta, gamma, columns, self.key["permutations"], chunk_len,
                                    blinding, self.b, z)
        return z

    def lookup_products(self, beta, gamma, permuted, blinding):
        z = [self.zeros(self.n) for _ in permuted]
        self.note("h2d", 64 + blinding.nbytes, "beta, gamma and lookup product blinding rows")
        lookup_products_device(self.k, beta, gamma, [p["compressed_input"] for p in permuted], [p["compressed_table"] for p in permuted],
                               [p["permuted_input"] for p in permuted], [p["permuted_table"] for p in permuted], blinding, self.b, z)
        return z

    def compress(self, graphs, theta, fixed, advice, instance, challenges, what):
        """the theta folds of one instance's tuples, one column per graph of lookup_compress_graphs"""
        comp = [self.zeros(self.n) for _ in graphs]
        self.note("h2d", 32 * (1 + len(challenges)), "theta and challenges (%s)" % what)
        lookup_compress_device(self.k, graphs, theta, comp, fixed, advice, instance, challenges)
        return comp

    def mvlookup_multiplicities(self, inputs, tables):
        m = [self.zeros(self.n) for _ in tables]
        self.note("d2h", 4 * sum(len(cols) for cols in inputs), "mv-lookup verdict flags (one per input column)")
        mvlookup_multiplicities_device(self.k, inputs, tables, self.b, m)
        return m

    def mvlookup_sums(self, beta, inputs, tables, m, blinding):
        phi = [self.zeros(self.n) for _ in tables]
        self.note("h2d", 32 + blinding.nbytes, "beta and mv-lookup sum blinding rows")
        mvlookup_sums_device(self.k, beta, inputs, tables, m, blinding, self.b, phi)
        return phi

    def shuffle_products(self, gamma, inputs, shuffles, blinding):
        z = [self.zeros(self.n) for _ in inputs]
        self.note("h2d", 32 + blinding.nbytes, "gamma and shuffle product blinding rows")
        shuffle_products_device(self.k, gamma, inputs, shuffles, blinding, self.b, z)
        return z

    def random_poly(self, rng):
        return rng.draw_device(self.n)

    def evaluate_h(self, case, values, form, t_evaluations):
        self.note("h2d", 32 * (4 + len(case["challenges"])), "y, beta, gamma, theta and challenges (evaluate_h)")
        if form == "parts":
            self.pk.ev.evaluate_h_parts_device(case, values, t_evaluations=t_evaluations)
        else:
            self.pk.ev.evaluate_h_device(case, values)
            if t_evaluations is not None:                                                                  # vanishing/prover.rs:84
                t = np.ascontiguousarray(t_evaluations, dtype=np.uint64)
                _check(lib().h2hip_divide_by_vanishing_poly_bn254_fr_device(_dptr(values), self.dom.extended_k,
                                                                            t.ctypes.data_as(ctypes.c_void_p), t.shape[0],
                                                                            _stream()), "h2hip_divide_by_vanishing_poly_bn254_fr_device")
                self.torch.cuda.current_stream().synchronize()  # t is read by the queued kernel's launch; keep it until then
        return values

    def extended_to_coeff(self, values):
        d = self.dom
        extended_to_coeff_device(values, d.extended_k, d.extended_omega_inv, d.extended_ifft_divisor, d.g_coset, d.g_coset_inv)
        return values

    def piece(self, coeffs, i):
        return coeffs.view(-1, 4)[i * self.n:(i + 1) * self.n]

    def evaluate(self, polys, query_poly, points, what):
        if not len(query_poly):
            return []
        self.note("h2d", 32 * len(points), "evaluation points")
        out = eval_polynomials_device(polys, query_poly, [fr_from_int(p) for p in points])
        self.note("d2h", out.nbytes, what)
        return [fr_to_int(e) for e in out]

    def combine(self, polys, scalars):
        out = self.zeros(self.n)
        self.note("h2d", 32 * len(scalars), "combination scalars")
        poly_combine_device(polys, [fr_from_int(s) for s in scalars], out)
        return out


class _Host:
    """columns are (n, 4) uint64 numpy arrays; every call is the host form, which uploads what it takes and downloads what it returns"""
    resident = False

    def __init__(self, pk, proof):
        self.pk, self.key, self.proof = pk, pk.host, proof
        self.dom, self.k, self.n, self.b = pk.domain, pk.k, pk.n, pk.b

    def note(self, direction, nbytes, what):
        if nbytes:
            self.proof.transfers.append((direction, int(nbytes), what))

    def _cols(self, direction, cols, what):
        self.note(direction, sum(c.nbytes for c in cols), what)

    def check_column(self, col, rows):
        if not (isinstance(col, np.ndarray) and col.dtype == np.uint64 and col.flags["C_CONTIGUOUS"] and col.shape == (rows, 4)):
            raise TypeError("resident=False: a column is a contiguous (%d, 4) uint64 numpy array" % rows)

    def zeros(self, rows):
        return np.zeros((rows, 4), dtype=np.uint64)

    def clone(self, col):
        return col.copy()

    def set_rows(self, col, start, values, what):
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        col[start:start + values.shape[0]] = values

    def commit(self, cols, lagrange, what, blinds=None):
        if not cols:
            return []
        self._cols("h2d", cols, what + ": columns")
        out = best_multiexp_batch(cols, self.pk.params.g_lagrange if lagrange else self.pk.params.g[:cols[0].shape[0]])
        self.note("d2h", out.nbytes, what)
        return list(out) if blinds is None else g1_linear_combinations(out, [[r] for r in blinds], [self.pk.params.w])

    def lagrange_to_coeff(self, cols):
        self._cols("h2d", cols, "lagrange_to_coeff")
        self._cols("d2h", cols, "lagrange_to_coeff")
        return self.dom.lagrange_to_coeff_batch(cols)

    def coeff_to_extended(self, polys):
        self._cols("h2d", polys, "coeff_to_extended")
        outs = self.dom.coeff_to_extended_batch(polys)
        self._cols("d2h", outs, "coeff_to_extended")
        return outs

    def commit_permuted(self, lookups, theta, blinding, fixed, advice, instance, challenges, blinds=None):
        self._cols("h2d", list(fixed) + list(advice) + list(instance), "commit_permuted: columns")
        out = commit_permuted(self.pk.params, self.dom, lookups, theta, blinding, self.b, blinds or [None] * (2 * len(lookups)), fixed, advice,
                              instance, challenges)
        self._cols("d2h", [c for d in out for key, c in d.items() if not key.endswith("commitment")], "commit_permuted: columns")
        return out

    def permutation_products(self, beta, gamma, columns, chunk_len, n_sets, blinding):
        self._cols("h2d", list(columns) + list(self.key["permutations"]), "permutation_products: columns")
        z = permutation_products(self.k, self.dom.omega, fr_from_int(FR_DELTA), beta, gamma, columns, self.key["permutations"], chunk_len,
                                 blinding, self.b)
        self._cols("d2h", z, "permutation_products: z")
        return z

    def lookup_products(self, beta, gamma, permuted, blinding):
        cols = [p[key] for key in ("compressed_input", "compressed_table", "permuted_input", "permuted_table") for p in permuted]
        self._cols("h2d", cols, "lookup_products: columns")
        c = len(permuted)
        z = lookup_products(self.k, beta, gamma, cols[:c], cols[c:2 * c], cols[2 * c:3 * c], cols[3 * c:], blinding, self.b)
        self._cols("d2h", z, "lookup_products: z")
        return z

    def compress(self, graphs, theta, fixed, advice, instance, challenges, what):
        self._cols("h2d", list(fixed) + list(advice) + list(instance), what + ": columns")
        comp = lookup_compress(self.k, graphs, theta, fixed, advice, instance, challenges)
        self._cols("d2h", comp, what + ": compressed columns")
        return comp

    def mvlookup_multiplicities(self, inputs, tables):
        self._cols("h2d", [c for cols in inputs for c in cols] + list(tables), "mvlookup_multiplicities: columns")
        m = mvlookup_multiplicities(self.k, inputs, tables, self.b)
        self._cols("d2h", m, "mvlookup_multiplicities: m")
        return m

    def mvlookup_sums(self, beta, inputs, tables, m, blinding):
        self._cols("h2d", [c for cols in inputs for c in cols] + list(tables) + list(m), "mvlookup_sums: columns")
        phi = mvlookup_sums(self.k, beta, inputs, tables, m, blinding, self.b)
        self._cols("d2h", phi, "mvlookup_sums: phi")
        return phi

    def shuffle_products(self, gamma, inputs, shuffles, blinding):
        self._cols("h2d", list(inputs) + list(shuffles), "shuffle_products: columns")
        z = shuffle_products(self.k, gamma, inputs, shuffles, blinding, self.b)
        self._cols("d2h", z, "shuffle_products: z")
        return z

    def random_poly(self, rng):
        """the same blocks of the stream as the resident path draws in HBM"""
        out = fr_random(rng.seed, self.n, rng.block, rng.stream_id)
        rng.block += self.n
        self.note("d2h", out.nbytes, "random polynomial")
        return out

    def evaluate_h(self, case, values, form, t_evaluations):
        moved = [case[key] for key in ("advice_polys", "instance_polys")] + [list(l) for l in case["lookups"]]
        moved.append(case["perm_product_polys" if form == "parts" else "perm_product_cosets"])
        moved += [list(pair) for pair in case.get("mvlookups", ())] + [list(case.get("shuffles", ()))]
        self._cols("h2d", [c for group in moved for c in group] + [values], "evaluate_h: columns and values")
        if form == "parts":
            values = self.pk.ev.evaluate_h_parts(case, values, t_evaluations=t_evaluations)
        else:
            values = self.pk.ev.evaluate_h(case, values)
            if t_evaluations is not None:
                values = self.dom.divide_by_vanishing_poly(values, t_evaluations)
        self.note("d2h", values.nbytes, "evaluate_h: values")
        return values

    def extended_to_coeff(self, values):
        self.note("h2d", values.nbytes, "extended_to_coeff")
        self.note("d2h", values.nbytes, "extended_to_coeff")
        return self.dom.extended_to_coeff(values)

    def piece(self, coeffs, i):
        return coeffs[i * self.n:(i + 1) * self.n]

    def evaluate(self, polys, query_poly, points, what):
        if not len(query_poly):
            return []
        self._cols("h2d", polys, what + ": polynomials")
        out = eval_polynomials(polys, query_poly, [fr_from_int(p) for p in points])
        self.note("d2h", out.nbytes, what)
        return [fr_to_int(e) for e in out]

    def combine(self, polys, scalars):
        polys = [np.ascontiguousarray(p) for p in polys]
        self._cols("h2d", polys, "poly_combine")
        out = poly_combine(polys, [fr_from_int(s) for s in scalars], out_len=self.n)
        self.note("d2h", out.nbytes, "poly_combine")
        return out


# ------------------------------------------------------------------ queries and the multiopen provers
def construct_intermediate_sets_gwc(queries):
    """gwc.rs:36-61: queries (commitment id, point, eval) grouped by point in order of first appearance -> [(point, [(id, eval), ...])]"""
    groups = []
    for cid, point, ev in queries:
        for p, qs in groups:
            if p == point:
                qs.append((cid, ev))
                break
        else:
            groups.append((point, [(cid, ev)]))
    return groups


def construct_intermediate_sets_shplonk(queries):
    """shplonk.rs:56-147: -> (rotation sets [(points ascending, [(id, [eval at each point]), ...])], super point set ascending).  The
    BTreeSets order scalars by their canonical value; sets appear in the order of the first commitment that has them."""
    evals, by_commitment = {}, []
    for cid, point, ev in queries:
        evals.setdefault((cid, point), ev)                       # get_eval finds the first such query :65-71
        for entry in by_commitment:
            if entry[0] == cid:
                entry[1].add(point)
                break
        else:
            by_commitment.append((cid, {point}))
    sets = []
    for cid, points in by_commitment:
        pts = tuple(sorted(points))
        for entry in sets:
            if entry[0] == pts:
                entry[1].append(cid)
                break
        else:
            sets.append((pts, [cid]))
    rotation_sets = [(list(pts), [(cid, [evals[(cid, p)] for p in pts]) for cid in cids]) for pts, cids in sets]
    return rotation_sets, sorted({p for _, p, _ in queries})


def _mont(x):
    return fr_from_int(x)


def _multiopen_gwc(be, transcript, polys, queries):
    """ProverGWC::create_proof (gwc/prover.rs:42-91)"""
    v = transcript.squeeze_challenge()                                                                     # :58
    groups = construct_intermediate_sets_gwc(queries)                                                      # :59
    be.note("h2d", sum(32 * (2 + len(qs)) for _, qs in groups), "v powers, evaluations and points (gwc)")
    witnesses = gwc_witnesses(polys, [(_mont(p), [(cid, _mont(e)) for cid, e in qs]) for p, qs in groups], _mont(v))   # :61-82
    for w in points_to_ints(be.commit(witnesses, False, "witness commitments")):                           # :83-88
        transcript.write_point(w)


def _multiopen_shplonk(be, transcript, polys, queries):
    """ProverSHPLONK::create_proof (shplonk/prover.rs:118-284)"""
    y = transcript.squeeze_challenge()                                                                     # :136
    rotation_sets, _ = construct_intermediate_sets_shplonk(queries)                                        # :173
    v = transcript.squeeze_challenge()                                                                     # :191
    sets = [([_mont(p) for p in pts], [(cid, [_mont(e) for e in evs]) for cid, evs in coms]) for pts, coms in rotation_sets]
    be.note("h2d", 2 * sum(32 * (len(pts) + len(coms) * (1 + len(pts))) for pts, coms in rotation_sets), "y, v powers, interpolants and points (shplonk)")
    h_x = shplonk_h(polys, sets, _mont(y), _mont(v))                                                       # :193-203
    transcript.write_point(points_to_ints(be.commit([h_x], False, "h commitment (shplonk)"))[0])           # :205-206
    u = transcript.squeeze_challenge()                                                                     # :207
    final = shplonk_final(polys, sets, h_x, _mont(y), _mont(v), _mont(u))                                  # :209-278
    transcript.write_point(points_to_ints(be.commit([final], False, "final commitment (shplonk)"))[0])     # :280-281


def _multiopen_ipa(be, transcript, rng, queries):
    """ProverIPA::create_proof (poly/ipa/multiopen/prover.rs) over queries (point, poly, blind).  ProverIPA tells commitments apart by
    the tensor's device address, so a polynomial is handed over as the same tensor at each of its points; a host column (resident=False)
    is uploaded once, the first time it is queried."""
    from . import ipa
    if not be.resident:
        import torch
        uploaded = {}
        for _, poly, _ in queries:
            if id(poly) not in uploaded:
                uploaded[id(poly)] = torch.from_numpy(np.ascontiguousarray(poly).view(np.int64)).cuda()
                be.note("h2d", poly.nbytes, "opening: a queried polynomial")
        queries = [(point, uploaded[id(poly)], blind) for point, poly, blind in queries]
    be.note("h2d", 32 * len(queries), "opening points (ipa)")
    ipa.ProverIPA(be.pk.params).create_proof(rng, transcript, queries)


MULTIOPEN = {"gwc": _multiopen_gwc, "shplonk": _multiopen_shplonk}  # the KZG schemes; "ipa" is _multiopen_ipa, whose queries carry blinds


def rotate_omega(domain, x, rotation):
    """EvaluationDomain::rotate_omega (poly/domain.rs) on integers"""
    w = domain.ints["omega"] if rotation >= 0 else domain.ints["omega_inv"]
    return x * pow(w, abs(rotation), FR_MODULUS) % FR_MODULUS


# ------------------------------------------------------------------ create_proof
def create_proof(params, pk, instances, witness, transcript, seed, multiopen="shplonk", form="parts", resident=True):
    """plonk/prover.rs:41-651.  instances: one list per proof instance of the instance columns' values (integers mod r, at most
    2^k - (blinding_factors + 1) each); witness(i, phase, challenges) returns the Lagrange columns of instance i's advice columns of
    that phase, in column order -- torch CUDA tensors (2^k, 4) int64 when resident, (2^k, 4) uint64 numpy arrays otherwise, Montgomery
    limbs; `challenges` holds the challenges of earlier phases as integers, None where not yet drawn.  The columns are consumed: their
    last blinding_factors + 1 rows are overwritten and, when resident, they are transformed in place.  transcript: a Blake2bWrite;
    seed: 32 bytes for FrRng.  Returns a Proof (bytes = transcript.finalize())."""
    if multiopen not in MULTIOPEN and multiopen != "ipa":
        raise ValueError("multiopen: 'shplonk', 'gwc' or 'ipa'")
    if form not in ("parts", "full"):
        raise ValueError("form: 'parts' or 'full'")
    if pk.params is not params:
        raise ValueError("the proving key was built over other params")
    ipa = multiopen == "ipa"                                                                               # P::QUERY_INSTANCE
    if ipa != (pk.scheme == "ipa"):
        raise ValueError("multiopen %r with %s params: 'ipa' goes with an ipa.ParamsIPA and a key built over it, 'shplonk' and 'gwc' with "
                         "KZG params" % (multiopen, "IPA" if pk.scheme == "ipa" else "KZG"))
    cs, dom, k, n, b, u = pk.cs, pk.domain, pk.k, pk.n, pk.b, pk.u
    proof = Proof()
    be = (_Device if resident else _Host)(pk, proof)
    key = be.key
    rng = FrRng(seed)
    N = len(instances)
    if N < 1:
        raise ValueError("instances: at least one proof instance")
    for inst in instances:                                                                                 # :57-61
        if len(inst) != cs.num_instance_columns:
            raise ValueError("InvalidInstances")

    def blind():
        """one commitment blind from the stream, as an integer (KZG ignores it, IPA commits with it)"""
        return fr_to_int(rng.draw(1)[0])

    def commit(cols, lagrange, what, blinds):
        """the commitments of `cols` as affine integer pairs: KZG's ignore the blinds, IPA's are MSM + [blind] W"""
        if ipa:
            return be.commit(cols, lagrange, what, blinds=blinds)
        return points_to_ints(be.commit(cols, lagrange, what))

    transcript.common_scalar(pk.vk_repr)                                                                   # :64 hash_into

    # ---- instance columns (:79-132).  QUERY_INSTANCE = false (KZG): the values are absorbed, nothing is committed; true (IPA): the
    # values are not absorbed (:91-93), each column is committed with Blind::default() = 1 and the commitments absorbed (:100-117)
    instance_values = []
    for inst in instances:
        cols = []
        for values in inst:
            if len(values) > u:
                raise ValueError("InstanceTooLarge")                                                       # :87-89
            if not ipa:
                for v in values:
                    transcript.common_scalar(int(v) % FR_MODULUS)                                          # :91-93
            col = be.zeros(n)
            if len(values):
                be.set_rows(col, 0, np.stack([fr_from_int(v) for v in values]), "instance values")
            cols.append(col)
        if ipa:
            for c in commit(cols, True, "instance commitments", [1] * len(cols)):                          # :100-117, one batched MSM
                transcript.common_point(c)
        instance_values.append(cols)
    instance_polys = [be.lagrange_to_coeff([be.clone(c) for c in cols]) for cols in instance_values]       # :119-125

    # ---- advice columns, phase by phase (:284-401)
    advice = [[None] * cs.num_advice_columns for _ in range(N)]
    advice_blinds = [[None] * cs.num_advice_columns for _ in range(N)]
    challenges = {}
    for phase in cs.phases():                                                                              # :295
        column_indices = [c for c, p in enumerate(cs.advice_column_phase) if p == phase]                   # :296-307
        for i in range(N):                                                                                 # :309
            cols = list(witness(i, phase, [challenges.get(j) for j in range(cs.num_challenges)]))          # :312-347
            if len(cols) != len(column_indices):
                raise ValueError("witness: phase %d has %d advice columns, got %d" % (phase, len(column_indices), len(cols)))
            for col in cols:
                be.check_column(col, n)
            rows = [rng.draw(b + 1) for _ in cols]                                                         # :350-354
            blinds = [blind() for _ in cols]                                                               # :357-360
            for col, r in zip(cols, rows):
                be.set_rows(col, u, r, "advice blinding rows")
            for c in commit(cols, True, "advice commitments", blinds):                                     # :361-377
                transcript.write_point(c)
            for c, col, r in zip(column_indices, cols, blinds):                                            # :378-383
                advice[i][c], advice_blinds[i][c] = col, r
        for j, p in enumerate(cs.challenge_phase):                                                         # :386-392
            if p == phase:
                challenges[j] = transcript.squeeze_challenge()
    challenge_list = [challenges[j] for j in range(cs.num_challenges)]                                     # :395-398
    ch_mont = np.stack([fr_from_int(c) for c in challenge_list]) if challenge_list else np.zeros((0, 4), dtype=np.uint64)

    theta = transcript.squeeze_challenge()                                                                 # :404
    theta_m = fr_from_int(theta)

    # ---- lookups: permuted columns (:406-431)
    proof.stages.append("lookup_permuted")
    permuted, permuted_blinds = [], []
    for i in range(N):
        blinding, blinds = [], []
        for _ in cs.lookups:
            blinding.append(rng.draw(2 * (b + 1)))                                                         # lookup/prover.rs:391-475
            blinds += [blind(), blind()]                                                                   # :129-140 (A', then S')
        blinding = np.concatenate(blinding) if blinding else np.zeros((0, 4), dtype=np.uint64)
        out = be.commit_permuted(cs.lookups, theta_m, blinding, key["fixed_values"], advice[i], instance_values[i], ch_mont,
                                 blinds=blinds if ipa else None) if cs.lookups else []
        coms = [c for d in out for c in (d["permuted_input_commitment"], d["permuted_table_commitment"])]
        for c in coms if ipa else points_to_ints(coms):
            transcript.write_point(c)                                                                      # lookup/prover.rs:143, :146
        permuted.append(out)
        permuted_blinds.append(blinds)

    # ---- mv-lookups: the compressed columns (kept until the grand sums) and the multiplicities m, committed before beta exists
    proof.stages.append("mvlookup_multiplicities")
    mv_graphs, mv_inputs = [], [len(inputs) for inputs, _ in cs.mv_lookups]
    for inputs, tab in cs.mv_lookups:
        mv_graphs += [flatten_graph(lookup_compress_graphs(inp, tab)[0]) for inp in inputs]
        mv_graphs.append(flatten_graph(lookup_compress_graphs(inputs[0], tab)[1]))
    mv_columns, mv_m, mv_m_blinds = [], [], []
    for i in range(N):
        mv_m_blinds.append([blind() for _ in cs.mv_lookups])                                               # draw 2b
        f, t, m = [], [], []
        if cs.mv_lookups:
            comp = be.compress(mv_graphs, theta_m, key["fixed_values"], advice[i], instance_values[i], ch_mont, "mv-lookup compression")
            at = 0
            for kj in mv_inputs:
                f.append(comp[at:at + kj])
                t.append(comp[at + kj])
                at += kj + 1
            m = be.mvlookup_multiplicities(f, t)
        for c in commit(m, True, "mv-lookup multiplicity commitments", mv_m_blinds[i]):
            transcript.write_point(c)
        mv_columns.append((f, t))
        mv_m.append(m)

    beta = transcript.squeeze_challenge()                                                                  # :434
    gamma = transcript.squeeze_challenge()                                                                 # :437
    beta_m, gamma_m = fr_from_int(beta), fr_from_int(gamma)

    # ---- permutation products (:440-457, permutation/prover.rs:45-191)
    proof.stages.append("permutation_products")
    chunk_len, n_sets = cs.chunk_len(), cs.num_permutation_sets()
    perm_polys, perm_blinds = [], []
    for i in range(N):
        pools = {"advice": advice[i], "fixed": key["fixed_values"], "instance": instance_values[i]}
        blinding, blinds = [], []
        for _ in range(n_sets):
            blinding.append(rng.draw(b))                                                                   # permutation/prover.rs:162-164
            blinds.append(blind())                                                                         # :168
        z = []
        if n_sets:
            z = be.permutation_products(beta_m, gamma_m, [pools[kind][c] for kind, c in cs.permutation], chunk_len, n_sets, np.concatenate(blinding))
        for c in commit(z, True, "permutation product commitments", blinds):                               # :170-181
            transcript.write_point(c)
        perm_polys.append(be.lagrange_to_coeff(z))                                                         # :172
        perm_blinds.append(blinds)

    # ---- lookup products (:459-468, lookup/prover.rs:167-305)
    proof.stages.append("lookup_products")
    lookup_polys, lookup_blinds = [], []
    for i in range(N):
        blinding, blinds = [], []
        for _ in cs.lookups:
            blinding.append(rng.draw(b))                                                                   # lookup/prover.rs:247
            blinds.append(blind())                                                                         # :290
        z = be.lookup_products(beta_m, gamma_m, permuted[i], np.concatenate(blinding)) if cs.lookups else []
        for c in commit(z, True, "lookup product commitments", blinds):                                    # :291-295
            transcript.write_point(c)
        lookup_polys.append(be.lagrange_to_coeff(z))                                                       # :292
        lookup_blinds.append(blinds)

    # ---- mv-lookup grand sums over the kept compressed columns and m
    proof.stages.append("mvlookup_sums")
    mv_polys, mv_phi_blinds = [], []
    for i in range(N):
        blinding, blinds = [], []
        for _ in cs.mv_lookups:
            blinding.append(rng.draw(b))                                                                   # draw 4b
            blinds.append(blind())
        (f, t), m = mv_columns[i], mv_m[i]
        phi = be.mvlookup_sums(beta_m, f, t, m, np.concatenate(blinding)) if cs.mv_lookups else []
        for c in commit(phi, True, "mv-lookup sum commitments", blinds):
            transcript.write_point(c)
        mv_phi_blinds.append(blinds)
        polys = be.lagrange_to_coeff(list(phi) + list(m))
        mv_polys.append([(polys[j], polys[len(phi) + j]) for j in range(len(phi))])
        mv_columns[i] = mv_m[i] = None                                                                     # the compressed columns are done

    # ---- shuffle products (upstream shuffle::Argument::commit_product)
    proof.stages.append("shuffle_products")
    shuffle_graphs = []
    for inp, shf in cs.shuffles:
        gi, gs = lookup_compress_graphs(inp, shf)
        shuffle_graphs += [flatten_graph(gi), flatten_graph(gs)]
    shuffle_polys, shuffle_blinds = [], []
    for i in range(N):
        blinding, blinds = [], []
        for _ in cs.shuffles:
            blinding.append(rng.draw(b))                                                                   # draw 4c
            blinds.append(blind())
        z = []
        if cs.shuffles:
            comp = be.compress(shuffle_graphs, theta_m, key["fixed_values"], advice[i], instance_values[i], ch_mont, "shuffle compression")
            z = be.shuffle_products(gamma_m, comp[0::2], comp[1::2], np.concatenate(blinding))
        for c in commit(z, True, "shuffle product commitments", blinds):
            transcript.write_point(c)
        shuffle_polys.append(be.lagrange_to_coeff(z))
        shuffle_blinds.append(blinds)

    # ---- the vanishing argument's random polynomial (:471, vanishing/prover.rs:37-65)
    random_poly = be.random_poly(rng)
    random_blind = blind()                                                                                 # vanishing/prover.rs:55-58
    transcript.write_point(commit([random_poly], False, "random polynomial commitment", [random_blind])[0])

    y = transcript.squeeze_challenge()                                                                     # :474

    # ---- advice polynomials (:477-493), batched per instance
    advice_polys = [be.lagrange_to_coeff(cols) for cols in advice]

    # ---- h(X) (:496-513, plonk/evaluation.rs:280-522); the last instance's call divides by the vanishing polynomial
    values = be.zeros(dom.extended_len())
    common = {"k": k, "extended_k": dom.extended_k, "extended_omega": dom.extended_omega, "g_coset": dom.g_coset, "g_coset_inv": dom.g_coset_inv,
              "zeta": fr_from_int(FR_ZETA), "delta": fr_from_int(FR_DELTA), "y": fr_from_int(y), "beta": beta_m, "gamma": gamma_m, "theta": theta_m,
              "challenges": ch_mont, "chunk_len": chunk_len, "last_rotation": -(b + 1),
              "perm_column_kind": np.array([_ANY[kind] for kind, _ in cs.permutation], dtype=np.uint32),
              "perm_column_index": np.array([c for _, c in cs.permutation], dtype=np.uint32)}
    if form == "parts":
        common.update({name: key[name] for name in ("fixed_polys", "l0_poly", "l_last_poly", "l_active_row_poly", "perm_polys")})
    else:
        common.update({name: key[name] for name in ("fixed_cosets", "l0", "l_last", "l_active_row", "perm_cosets")})
    for i in range(N):
        case = dict(common, advice_polys=advice_polys[i], instance_polys=instance_polys[i],
                    lookups=[(lookup_polys[i][j], permuted[i][j]["permuted_input_poly"], permuted[i][j]["permuted_table_poly"])
                             for j in range(len(cs.lookups))])
        if cs.mv_lookups:
            case["mvlookups"] = mv_polys[i]
        if cs.shuffles:
            case["shuffles"] = shuffle_polys[i]
        if form == "parts":
            case["perm_product_polys"] = perm_polys[i]
        else:
            case["perm_product_cosets"] = be.coeff_to_extended(perm_polys[i])                              # permutation/prover.rs:175
        values = be.evaluate_h(case, values, form, dom.t_evaluations if i == N - 1 else None)

    # ---- the pieces of h(X) (:516, vanishing/prover.rs:69-120)
    h_coeffs = be.extended_to_coeff(values)                                                                # :87
    h_pieces = [be.piece(h_coeffs, i) for i in range(dom.quotient_poly_degree)]                            # :90-93, views
    h_blinds = [blind() for _ in h_pieces]                                                                 # :95-98
    for c in commit(h_pieces, False, "h piece commitments", h_blinds):                                     # :101-113
        transcript.write_point(c)

    x = transcript.squeeze_challenge()                                                                     # :518
    xn = pow(x, n, FR_MODULUS)                                                                             # :519
    x_next, x_inv, x_last = rotate_omega(dom, x, 1), rotate_omega(dom, x, -1), rotate_omega(dom, x, -(b + 1))

    # ---- evaluations, one call per group of polynomials, in the order the verifier reads them (:543-597)
    instance_evals = []
    for i in range(N if ipa else 0):                                                                       # :521-541 (QUERY_INSTANCE)
        evs = be.evaluate(instance_polys[i], [c for c, _ in cs.instance_queries], [rotate_omega(dom, x, r) for _, r in cs.instance_queries],
                          "instance evaluations")
        for e in evs:
            transcript.write_scalar(e)
        instance_evals.append(evs)
    advice_evals = []
    for i in range(N):                                                                                     # :544-561
        evs = be.evaluate(advice_polys[i], [c for c, _ in cs.advice_queries], [rotate_omega(dom, x, r) for _, r in cs.advice_queries], "advice evaluations")
        for e in evs:
            transcript.write_scalar(e)
        advice_evals.append(evs)
    fixed_evals = be.evaluate(key["fixed_polys"], [c for c, _ in cs.fixed_queries], [rotate_omega(dom, x, r) for _, r in cs.fixed_queries],
                              "fixed evaluations")                                                         # :564-575
    for e in fixed_evals:
        transcript.write_scalar(e)
    h_poly = be.combine(h_pieces, [pow(xn, i, FR_MODULUS) for i in range(len(h_pieces))])                  # :577, vanishing/prover.rs:131-135
    random_eval, h_eval = be.evaluate([random_poly, h_poly], [0, 1], [x, x], "random polynomial and h evaluations")
    transcript.write_scalar(random_eval)                                                                   # vanishing/prover.rs:145-146
    common_evals = be.evaluate(key["perm_polys"], list(range(len(cs.permutation))), [x] * len(cs.permutation), "permutation evaluations")
    for e in common_evals:                                                                                 # :580, permutation/prover.rs:221-232
        transcript.write_scalar(e)
    perm_evals = []
    for i in range(N):                                                                                     # :583-586, permutation/prover.rs:236-279
        qp, pts = [], []
        for t in range(n_sets):
            qp += [t, t] + ([t] if t < n_sets - 1 else [])
            pts += [x, x_next] + ([x_last] if t < n_sets - 1 else [])
        evs = be.evaluate(perm_polys[i], qp, pts, "permutation product evaluations")
        for e in evs:
            transcript.write_scalar(e)
        perm_evals.append(evs)
    lookup_evals = []
    for i in range(N):                                                                                     # :589-597, lookup/prover.rs:309-337
        polys, qp, pts = [], [], []
        for j in range(len(cs.lookups)):
            polys += [lookup_polys[i][j], permuted[i][j]["permuted_input_poly"], permuted[i][j]["permuted_table_poly"]]
            qp += [3 * j, 3 * j, 3 * j + 1, 3 * j + 1, 3 * j + 2]
            pts += [x, x_next, x, x_inv, x]
        evs = be.evaluate(polys, qp, pts, "lookup evaluations")
        for e in evs:
            transcript.write_scalar(e)
        lookup_evals.append(evs)
    mv_evals = []
    for i in range(N):                                                                                     # phi(x), phi(wx), m(x) per argument
        polys, qp, pts = [], [], []
        for j, (phi, m) in enumerate(mv_polys[i]):
            polys += [phi, m]
            qp += [2 * j, 2 * j, 2 * j + 1]
            pts += [x, x_next, x]
        evs = be.evaluate(polys, qp, pts, "mv-lookup evaluations")
        for e in evs:
            transcript.write_scalar(e)
        mv_evals.append(evs)
    shuffle_evals = []
    for i in range(N):                                                                                     # z(x), z(wx) per shuffle
        qp = [j for j in range(len(cs.shuffles)) for _ in range(2)]
        evs = be.evaluate(shuffle_polys[i], qp, [x, x_next] * len(cs.shuffles), "shuffle evaluations")
        for e in evs:
            transcript.write_scalar(e)
        shuffle_evals.append(evs)

    # ---- the opening queries (:599-645): (polynomial id, point, evaluation) with ids into `polys`; poly_blinds[id] is the blind of the
    # polynomial's commitment, which only IPA's queries carry (KZG's commitments have none)
    polys, poly_blinds, queries = [], [], []

    def poly_id(p, r=0):
        polys.append(p)
        poly_blinds.append(r)
        return len(polys) - 1

    fixed_ids = [poly_id(p, 1) for p in key["fixed_polys"]]                                                # Blind::default() :640
    common_ids = [poly_id(p, 1) for p in key["perm_polys"]]                                                # permutation/prover.rs:217
    for i in range(N):
        if ipa:                                                                                            # :607-617, Blind::default()
            ids = [poly_id(p, 1) for p in instance_polys[i]]
            for q, (c, r) in enumerate(cs.instance_queries):
                queries.append((ids[c], rotate_omega(dom, x, r), instance_evals[i][q]))
        ids = [poly_id(p, r) for p, r in zip(advice_polys[i], advice_blinds[i])]
        for q, (c, r) in enumerate(cs.advice_queries):                                                     # :618-628
            queries.append((ids[c], rotate_omega(dom, x, r), advice_evals[i][q]))
        ids = [poly_id(p, r) for p, r in zip(perm_polys[i], perm_blinds[i])]                               # :629, permutation/prover.rs:283-327
        at = 0
        last = {}
        for t in range(n_sets):
            queries.append((ids[t], x, perm_evals[i][at]))
            queries.append((ids[t], x_next, perm_evals[i][at + 1]))
            at += 2
            if t < n_sets - 1:
                last[t] = perm_evals[i][at]
                at += 1
        for t in reversed(range(n_sets - 1)):                                                              # .rev().skip(1)
            queries.append((ids[t], x_last, last[t]))
        for j in range(len(cs.lookups)):                                                                   # :630, lookup/prover.rs:341-380
            z_id, a_id, s_id = (poly_id(p, r) for p, r in ((lookup_polys[i][j], lookup_blinds[i][j]),
                                                           (permuted[i][j]["permuted_input_poly"], permuted_blinds[i][2 * j]),
                                                           (permuted[i][j]["permuted_table_poly"], permuted_blinds[i][2 * j + 1])))
            z_x, z_next, a_x, a_inv, s_x = lookup_evals[i][5 * j:5 * j + 5]
            queries += [(z_id, x, z_x), (a_id, x, a_x), (s_id, x, s_x), (a_id, x_inv, a_inv), (z_id, x_next, z_next)]
        for j, (phi, m) in enumerate(mv_polys[i]):
            phi_id, m_id = poly_id(phi, mv_phi_blinds[i][j]), poly_id(m, mv_m_blinds[i][j])
            phi_x, phi_next, m_x = mv_evals[i][3 * j:3 * j + 3]
            queries += [(phi_id, x, phi_x), (phi_id, x_next, phi_next), (m_id, x, m_x)]
        for j, z in enumerate(shuffle_polys[i]):
            z_id = poly_id(z, shuffle_blinds[i][j])
            queries += [(z_id, x, shuffle_evals[i][2 * j]), (z_id, x_next, shuffle_evals[i][2 * j + 1])]
    for q, (c, r) in enumerate(cs.fixed_queries):                                                          # :632-642
        queries.append((fixed_ids[c], rotate_omega(dom, x, r), fixed_evals[q]))
    for j in range(len(cs.permutation)):                                                                   # :643, permutation/prover.rs:210-219
        queries.append((common_ids[j], x, common_evals[j]))
    h_blind = 0                                                                                            # vanishing/prover.rs:137-143
    for r in reversed(h_blinds):
        h_blind = (h_blind * xn + r) % FR_MODULUS
    queries.append((poly_id(h_poly, h_blind), x, h_eval))                                                  # :645, vanishing/prover.rs:157-172
    queries.append((poly_id(random_poly, random_blind), x, random_eval))

    if ipa:                                                                                                # :647-650; the same FrRng goes on
        _multiopen_ipa(be, transcript, rng, [(point, polys[pid], poly_blinds[pid]) for pid, point, _ in queries])
    else:
        MULTIOPEN[multiopen](be, transcript, polys, queries)
    proof.bytes = transcript.finalize()
    proof.challenges = {"theta": theta, "beta": beta, "gamma": gamma, "y": y, "x": x, "challenges": challenge_list}
    return proof
