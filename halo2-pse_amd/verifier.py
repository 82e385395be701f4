"""verify_proof for the reference's PLONK-over-KZG protocol on Python integers: plonk/verifier.rs:27-399 with the three argument
verifiers (plonk/permutation/verifier.rs, plonk/lookup/verifier.rs, plonk/vanishing/verifier.rs) and the two multiopen verifiers
(poly/kzg/multiopen/gwc/verifier.rs:48-129, poly/kzg/multiopen/shplonk/verifier.rs:53-147).

Scalars are integers mod r, points are (x, y) integer pairs or None (transcript.py); G1 arithmetic is the textbook Jacobian formulas
below.  Nothing on the KZG paths touches the GPU or grows with 2^k: the cost is a few dozen scalar multiplications, and one field
inversion per instance value.  The proof is valid iff e(left, s_g2) = e(right, g2) for the two channels of the reference's DualMSM
(poly/kzg/msm.rs).  With a kzg.SingleStrategy or kzg.AccumulatorStrategy the multiopen verifier adds its terms, unevaluated, to the
strategy's DualMSM and the strategy closes the check with the library's host pairing (kzg.py, include/halo2hip_pairing.h): the proof is
accepted or refused here, without the setup secret.  Without a strategy verify_proof returns the two G1 points (left, right).  Both KZG
verifiers set QUERY_INSTANCE = false: the instance values are absorbed as scalars and their evaluations computed from l_i(x) (:84-90, :176-214).

The shuffle and mv-lookup (logUp) arguments are later than the reference; their commitments, evaluations, expressions and queries are
read and built in the order prover.py's docstring fixes (mv-lookups before shuffles, both after the halo2 lookups), and their share of
h(x) is mvlookup_expressions / shuffle_expressions below: include/halo2hip.h's fold at one point instead of one coset row.

multiopen="ipa" is the same function with QUERY_INSTANCE = true (poly/ipa/multiopen/verifier.rs:33) over ipa.py: the instance columns are
committed (one batched MSM per proof over the params' pinned g_lagrange) instead of absorbed, their evaluations are read from the proof,
every commitment is an ipa.Commitment handle, h_commitment an MSMIPA, and the caller's strategy closes the check with one MSM of 2^k
terms on the GPU -- no pairing and no setup secret, so that path is accepted or rejected here, end to end."""
from .prover import ZERO, _is_ipa, construct_intermediate_sets_gwc, construct_intermediate_sets_shplonk
from .transcript import FQ_MODULUS, FR_MODULUS, TranscriptError

R, Q = FR_MODULUS, FQ_MODULUS
FR_DELTA = pow(7, 1 << 28, R)
_FR_ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c  # Fr::ROOT_OF_UNITY, of order 2^28


class VerifyError(ValueError):
    """the reference's Error::{InvalidInstances, InstanceTooLarge, Opening, ...}: the proof cannot be valid"""


# ------------------------------------------------------------------ G1 on integers
def _jac(p):
    return (0, 1, 0) if p is None else (p[0], p[1], 1)


def _jac_double(p):
    x, y, z = p
    if z == 0 or y == 0:
        return (0, 1, 0)
    a, b = x * x % Q, y * y % Q
    c = b * b % Q
    d = 2 * ((x + b) * (x + b) - a - c) % Q
    e = 3 * a % Q
    x3 = (e * e - 2 * d) % Q
    return (x3, (e * (d - x3) - 8 * c) % Q, 2 * y * z % Q)


def _jac_add(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    x1, y1, z1 = p
    x2, y2, z2 = q
    z1z1, z2z2 = z1 * z1 % Q, z2 * z2 % Q
    u1, u2 = x1 * z2z2 % Q, x2 * z1z1 % Q
    s1, s2 = y1 * z2 * z2z2 % Q, y2 * z1 * z1z1 % Q
    if u1 == u2:
        return _jac_double(p) if s1 == s2 else (0, 1, 0)
    h, r = (u2 - u1) % Q, (s2 - s1) % Q
    hh = h * h % Q
    hhh, v = h * hh % Q, u1 * hh % Q
    x3 = (r * r - hhh - 2 * v) % Q
    return (x3, (r * (v - x3) - s1 * hhh) % Q, z1 * z2 * h % Q)


def _jac_mul(p, k):
    k %= R
    acc = (0, 1, 0)
    for bit in bin(k)[2:] if k else "":
        acc = _jac_double(acc)
        if bit == "1":
            acc = _jac_add(acc, p)
    return acc


def _affine(p):
    if p[2] == 0:
        return None
    zi = pow(p[2], -1, Q)
    return (p[0] * zi * zi % Q, p[1] * zi * zi * zi % Q)


class MSM:
    """MSMKZG (poly/kzg/msm.rs): a list of (scalar, point) terms"""

    def __init__(self, terms=()):
        self.terms = list(terms)

    def append_term(self, scalar, point):
        self.terms.append((scalar % R, point))

    def add_msm(self, other):
        self.terms += other.terms

    def scale(self, factor):
        self.terms = [(s * factor % R, p) for s, p in self.terms]

    def scaled(self, factor):
        return MSM((s * factor % R, p) for s, p in self.terms)

    def eval(self):
        acc, merged = (0, 1, 0), {}
        for s, p in self.terms:
            merged[p] = (merged.get(p, 0) + s) % R
        for p, s in merged.items():
            if p is not None and s:
                acc = _jac_add(acc, _jac_mul(_jac(p), s))
        return _affine(acc)


# ------------------------------------------------------------------ the domain on integers
class _Domain:
    def __init__(self, k):
        self.k, self.n = k, 1 << k
        self.omega = pow(_FR_ROOT_OF_UNITY, 1 << (28 - k), R)
        self.omega_inv = pow(self.omega, -1, R)
        self.barycentric_weight = pow(self.n, -1, R)

    def rotate_omega(self, x, rotation):
        return x * pow(self.omega if rotation >= 0 else self.omega_inv, abs(rotation), R) % R

    def l_i_range(self, x, xn, rotations):
        """poly/domain.rs l_i_range: l_i(x) = omega^i (x^n - 1) / (n (x - omega^i)) for each rotation i"""
        common = (xn - 1) * self.barycentric_weight % R
        out = []
        for rot in rotations:
            d = (x - self.rotate_omega(1, rot)) % R
            out.append(self.rotate_omega(pow(d, -1, R) * common % R if d else 0, rot))  # batch_invert leaves a zero zero
        return out


def evaluate_expression(e, fixed_evals, advice_evals, instance_evals, challenges, cs):
    """Expression::evaluate over the claimed evaluations (verifier.rs:272-283): a query reads the evaluation at its query index"""
    tag = e[0]
    if tag == "const":
        return e[1] % R
    if tag == "fixed":
        return fixed_evals[cs.query_index("fixed", e[1], e[2])]
    if tag == "advice":
        return advice_evals[cs.query_index("advice", e[1], e[2])]
    if tag == "instance":
        return instance_evals[cs.query_index("instance", e[1], e[2])]
    if tag == "challenge":
        return challenges[e[1]]
    ev = lambda sub: evaluate_expression(sub, fixed_evals, advice_evals, instance_evals, challenges, cs)  # noqa: E731
    if tag == "neg":
        return -ev(e[1]) % R
    if tag == "sum":
        return (ev(e[1]) + ev(e[2])) % R
    if tag == "prod":
        return ev(e[1]) * ev(e[2]) % R
    if tag == "scaled":
        return ev(e[1]) * e[2] % R
    raise ValueError(tag)


def compress_evals(values, theta):
    """the theta fold of a tuple's values: acc = acc theta + e, from zero (lookup/verifier.rs:116-134)"""
    acc = 0
    for v in values:
        acc = (acc * theta + v) % R
    return acc


def mvlookup_expressions(l_0, l_last, l_active, beta, inputs, table, phi_x, phi_next, m_x):
    """the three expressions of one mv-lookup argument, in fold order.  inputs: the theta folds F_c of its K input tuples, table: the
    fold T of its table; with f_c = F_c + beta, tau = T + beta, P = prod f_c and Q = sum_c prod_{l != c} f_l:
    l_0 phi(x), l_last phi(x), l_active (tau P (phi(wx) - phi(x)) - tau Q + m(x) P)"""
    tau, P, Qs = (table + beta) % R, 1, 0
    for F in inputs:                                                                     # Q <- Q f + P; P <- P f
        f = (F + beta) % R
        Qs = (Qs * f + P) % R
        P = P * f % R
    return [l_0 * phi_x % R, l_last * phi_x % R, l_active * (tau * P % R * (phi_next - phi_x) - tau * Qs + m_x * P) % R]


def shuffle_expressions(l_0, l_last, l_active, gamma, a, s, z_x, z_next):
    """the three expressions of one shuffle, in fold order.  a / s: the theta folds A, S of its input and shuffle tuples:
    l_0 (1 - z(x)), l_last (z(x)^2 - z(x)), l_active (z(wx) (S + gamma) - z(x) (A + gamma))"""
    return [l_0 * (1 - z_x) % R, l_last * (z_x * z_x - z_x) % R, l_active * (z_next * (s + gamma) - z_x * (a + gamma)) % R]


def _g0(params_vk):
    """params.g[0] as an integer pair: an object with .g0, or a ParamsKZG whose g holds Montgomery limbs (R = 2^256)"""
    g0 = getattr(params_vk, "g0", None)
    if g0 is not None:
        return g0
    limbs = [int(v) for v in params_vk.g[0]]
    rinv = pow(1 << 256, -1, Q)
    x = sum(v << (64 * i) for i, v in enumerate(limbs[:4])) * rinv % Q
    y = sum(v << (64 * i) for i, v in enumerate(limbs[4:])) * rinv % Q
    return (x, y)


# ------------------------------------------------------------------ the multiopen verifiers
def _commitment_msm(commitments, cid, factor):
    """CommitmentReference::{Commitment, MSM} scaled (gwc/verifier.rs:91-102, shplonk/verifier.rs:110-121)"""
    c = commitments[cid]
    return c.scaled(factor) if isinstance(c, MSM) else MSM([(factor % R, c)])


def _verify_gwc(transcript, g0, commitments, queries):
    """VerifierGWC::verify_proof (gwc/verifier.rs:48-129) -> the terms it adds to a DualMSM's (left, right), unevaluated"""
    v = transcript.squeeze_challenge()                                                   # :62
    groups = construct_intermediate_sets_gwc(queries)                                    # :64
    w = [transcript.read_point() for _ in groups]                                        # :66-68
    u = transcript.squeeze_challenge()                                                   # :70
    commitment_multi, witness, witness_with_aux, eval_multi = MSM(), MSM(), MSM(), 0
    power_of_u = 1
    for (z, qs), wi in zip(groups, w):                                                   # :78-119
        batch, eval_batch, power_of_v = MSM(), 0, 1
        for cid, ev in qs:
            batch.add_msm(_commitment_msm(commitments, cid, power_of_v))
            eval_batch = (eval_batch + power_of_v * ev) % R
            power_of_v = power_of_v * v % R
        batch.scale(power_of_u)
        commitment_multi.add_msm(batch)
        eval_multi = (eval_multi + power_of_u * eval_batch) % R
        witness_with_aux.append_term(power_of_u * z, wi)
        witness.append_term(power_of_u, wi)
        power_of_u = power_of_u * u % R
    right = MSM()
    right.add_msm(witness_with_aux)                                                      # :123
    right.add_msm(commitment_multi)                                                      # :124
    right.append_term(-eval_multi, g0)                                                   # :125-126
    return witness, right                                                                # :121


def _interpolate_eval(points, evals, u):
    """eval_polynomial(lagrange_interpolate(points, evals), u) (shplonk/verifier.rs:105-109)"""
    acc = 0
    for j, (pj, ej) in enumerate(zip(points, evals)):
        num, den = 1, 1
        for m, pm in enumerate(points):
            if m != j:
                num = num * (u - pm) % R
                den = den * (pj - pm) % R
        acc = (acc + ej * num % R * pow(den, -1, R)) % R
    return acc


def _vanishing(points, u):
    acc = 1
    for p in points:
        acc = acc * (u - p) % R
    return acc


def _verify_shplonk(transcript, g0, commitments, queries):
    """VerifierSHPLONK::verify_proof (shplonk/verifier.rs:53-147) -> the terms it adds to a DualMSM's (left, right), unevaluated"""
    rotation_sets, super_point_set = construct_intermediate_sets_shplonk(queries)        # :67-71
    y = transcript.squeeze_challenge()                                                   # :73
    v = transcript.squeeze_challenge()                                                   # :74
    h1 = transcript.read_point()                                                         # :76
    u = transcript.squeeze_challenge()                                                   # :77
    h2 = transcript.read_point()                                                         # :78
    z_0_diff_inverse, z_0 = 0, 0
    outer, r_outer_acc, power_of_v = MSM(), 0, 1
    for i, (points, coms) in enumerate(rotation_sets):                                   # :82-133
        z_diff_i = _vanishing([p for p in super_point_set if p not in points], u)
        if i == 0:
            z_0 = _vanishing(points, u)
            if z_diff_i == 0:
                raise VerifyError("Opening")                                              # invert().unwrap()
            z_0_diff_inverse = pow(z_diff_i, -1, R)
            z_diff_i = 1
        else:
            z_diff_i = z_diff_i * z_0_diff_inverse % R
        inner, r_inner_acc, power_of_y = MSM(), 0, 1
        for cid, evs in coms:
            r_inner_acc = (r_inner_acc + power_of_y * _interpolate_eval(points, evs, u)) % R
            inner.add_msm(_commitment_msm(commitments, cid, power_of_y))
            power_of_y = power_of_y * y % R
        inner.scale(power_of_v * z_diff_i)
        outer.add_msm(inner)
        r_outer_acc = (r_outer_acc + power_of_v * r_inner_acc % R * z_diff_i) % R
        power_of_v = power_of_v * v % R
    outer.append_term(-r_outer_acc, g0)                                                  # :135-136
    outer.append_term(-z_0, h1)                                                          # :137
    outer.append_term(u, h2)                                                             # :138
    return MSM([(1, h2)]), outer                                                         # :140-144


MULTIOPEN = {"gwc": _verify_gwc, "shplonk": _verify_shplonk}


def _is_kzg_strategy(strategy):
    from . import kzg  # kzg.py imports this module
    return isinstance(strategy, kzg.STRATEGIES)


# ------------------------------------------------------------------ verify_proof
def verify_proof(params_vk, vk, instances, transcript, multiopen="shplonk", strategy=None):
    """plonk/verifier.rs:27-399.  params_vk: the verifier's params (a ParamsKZG, or any object with k and g0); vk: a VerifyingKey;
    instances: as for create_proof; transcript: a Blake2bRead over the proof.  Returns (left, right), affine integer pairs (None: the
    identity), when strategy is None.  With strategy a kzg.SingleStrategy or kzg.AccumulatorStrategy over params that carry g2 and s_g2,
    the value of strategy.process(...) is returned instead: SingleStrategy raises VerifyError unless e(left, s_g2) = e(right, g2) and
    returns None, AccumulatorStrategy returns itself for finalize().  A malformed proof -- short, a bad point encoding, a non-canonical
    scalar -- raises TranscriptError; instances that do not fit the key raise VerifyError.

    multiopen="ipa" (QUERY_INSTANCE = true, poly/ipa/multiopen/verifier.rs:33): params_vk is an ipa.ParamsIPA, vk the key built over
    it, and `strategy` -- an ipa.SingleStrategy or ipa.AccumulatorStrategy -- is required: the instance columns are committed here and
    the commitments absorbed, their evaluations read from the proof, and the opening check is
    strategy.process(lambda msm: VerifierIPA(params).verify_proof(transcript, queries, msm)), whose value is returned (SingleStrategy
    raises ipa.IPAError unless the proof verifies; AccumulatorStrategy returns itself for finalize()).  Nothing else closes the check:
    an IPA opening is valid when one MSM is the identity, and the strategy evaluates it on the GPU."""
    if multiopen != "ipa" and multiopen not in MULTIOPEN:
        raise ValueError("multiopen: 'shplonk', 'gwc' or 'ipa'")
    use_ipa = multiopen == "ipa"
    if not use_ipa and strategy is not None:
        from . import kzg  # kzg.py imports this module
    if use_ipa:
        from . import ipa  # ipa.py imports this module
        if not isinstance(params_vk, ipa.ParamsIPA):
            raise ValueError("multiopen 'ipa' takes an ipa.ParamsIPA")
        if strategy is None:
            raise ValueError("multiopen 'ipa' needs a strategy: an ipa.SingleStrategy or ipa.AccumulatorStrategy")
        if _is_kzg_strategy(strategy):
            raise ValueError("a kzg strategy belongs to multiopen 'shplonk' or 'gwc': multiopen 'ipa' takes an ipa strategy")
    elif strategy is not None and not _is_kzg_strategy(strategy):
        raise ValueError("strategy belongs to multiopen 'ipa': the KZG verifiers return (left, right) for the caller's pairing")
    elif _is_ipa(params_vk):
        raise ValueError("multiopen %r takes KZG params, not an ipa.ParamsIPA" % (multiopen,))
    if use_ipa != (getattr(vk, "scheme", "kzg") == "ipa"):
        raise ValueError("multiopen %r with the verifying key of %s params" % (multiopen, "IPA" if not use_ipa else "KZG"))
    cs = vk.cs
    if int(params_vk.k) != vk.k:
        raise VerifyError("the params and the verifying key differ in k")
    dom = _Domain(vk.k)
    n, b = dom.n, cs.blinding_factors()
    for inst in instances:                                                               # :42-46
        if len(inst) != cs.num_instance_columns:
            raise VerifyError("InvalidInstances")
        for values in inst:
            if len(values) > n - (b + 1):
                raise VerifyError("InstanceTooLarge")
    instances = [[[int(v) % R for v in values] for values in inst] for inst in instances]
    num_proofs = len(instances)                                                          # :71

    instance_commitments = []
    if use_ipa:                                                                          # :48-69: zero-padded columns, Blind::default() = 1
        import numpy as np
        from . import fr_from_int
        for inst in instances:
            cols = []
            for values in inst:
                col = np.zeros((n, 4), dtype=np.uint64)
                if values:
                    col[:len(values)] = np.stack([fr_from_int(v) for v in values])
                cols.append(col)
            instance_commitments.append(params_vk.commit_lagrange_many(cols, [1] * len(cols)) if cols else [])

    transcript.common_scalar(vk.vk_repr)                                                 # :74 hash_into
    if use_ipa:
        for coms in instance_commitments:                                                # :76-82
            for c in coms:
                transcript.common_point(c)
    else:
        for inst in instances:                                                           # :84-90
            for values in inst:
                for v in values:
                    transcript.common_scalar(v)

    advice_commitments = [[None] * cs.num_advice_columns for _ in range(num_proofs)]     # :94-120
    challenges = [0] * cs.num_challenges
    for phase in cs.phases():
        for coms in advice_commitments:
            for c, p in enumerate(cs.advice_column_phase):
                if p == phase:
                    coms[c] = transcript.read_point()
        for j, p in enumerate(cs.challenge_phase):
            if p == phase:
                challenges[j] = transcript.squeeze_challenge()

    theta = transcript.squeeze_challenge()                                               # :123
    lookups_permuted = [[(transcript.read_point(), transcript.read_point()) for _ in cs.lookups] for _ in range(num_proofs)]   # :125-134
    mvlookups_m = [[transcript.read_point() for _ in cs.mv_lookups] for _ in range(num_proofs)]
    beta = transcript.squeeze_challenge()                                                # :137
    gamma = transcript.squeeze_challenge()                                               # :140
    chunk_len = vk.cs_degree - 2
    chunks = [cs.permutation[i:i + chunk_len] for i in range(0, len(cs.permutation), chunk_len)]
    permutations_committed = [[transcript.read_point() for _ in chunks] for _ in range(num_proofs)]                            # :142-147
    lookups_product = [[transcript.read_point() for _ in cs.lookups] for _ in range(num_proofs)]                               # :149-158
    mvlookups_phi = [[transcript.read_point() for _ in cs.mv_lookups] for _ in range(num_proofs)]
    shuffles_product = [[transcript.read_point() for _ in cs.shuffles] for _ in range(num_proofs)]
    random_poly_commitment = transcript.read_point()                                     # :160
    y = transcript.squeeze_challenge()                                                   # :163
    h_commitments = [transcript.read_point() for _ in range(vk.cs_degree - 1)]           # :165, get_quotient_poly_degree
    x = transcript.squeeze_challenge()                                                   # :169
    xn = pow(x, n, R)

    if use_ipa:                                                                          # :170-175: read, not computed
        instance_evals = [[transcript.read_scalar() for _ in cs.instance_queries] for _ in range(num_proofs)]
    else:                                                                                # instance evaluations from l_i(x) (:176-214)
        rots = [r for _, r in cs.instance_queries]
        min_rotation, max_rotation = min([0] + rots), max([0] + rots)
        max_instance_len = max([len(values) for inst in instances for values in inst] or [0])
        l_i_s = dom.l_i_range(x, xn, range(-max_rotation, max_instance_len + abs(min_rotation)))
        instance_evals = []
        for inst in instances:
            evs = []
            for column, rotation in cs.instance_queries:
                offset = max_rotation - rotation
                evs.append(sum(v * l for v, l in zip(inst[column], l_i_s[offset:offset + len(inst[column])])) % R)
            instance_evals.append(evs)

    advice_evals = [[transcript.read_scalar() for _ in cs.advice_queries] for _ in range(num_proofs)]     # :217-219
    fixed_evals = [transcript.read_scalar() for _ in cs.fixed_queries]                   # :221
    random_eval = transcript.read_scalar()                                               # :223
    permutation_evals = [transcript.read_scalar() for _ in vk.permutation_commitments]   # :225
    permutations_evaluated = []                                                          # :227-230, permutation/verifier.rs:72-98
    for _ in range(num_proofs):
        sets = []
        for t in range(len(chunks)):
            ev, nxt = transcript.read_scalar(), transcript.read_scalar()
            sets.append((ev, nxt, transcript.read_scalar() if t < len(chunks) - 1 else None))
        permutations_evaluated.append(sets)
    lookups_evaluated = [[tuple(transcript.read_scalar() for _ in range(5)) for _ in cs.lookups] for _ in range(num_proofs)]   # :232-240
    mvlookups_evaluated = [[tuple(transcript.read_scalar() for _ in range(3)) for _ in cs.mv_lookups] for _ in range(num_proofs)]
    shuffles_evaluated = [[tuple(transcript.read_scalar() for _ in range(2)) for _ in cs.shuffles] for _ in range(num_proofs)]

    # ---- the expected h(x) (:244-324)
    l_evals = dom.l_i_range(x, xn, range(-(b + 1), 1))                                   # :249-252
    l_last, l_blind, l_0 = l_evals[0], sum(l_evals[1:1 + b]) % R, l_evals[1 + b]
    active_rows = (1 - (l_last + l_blind)) % R
    expressions = []
    for i in range(num_proofs):
        ev = lambda e: evaluate_expression(e, fixed_evals, advice_evals[i], instance_evals[i], challenges, cs)  # noqa: E731
        expressions += [ev(ZERO if p is None else p) for p in cs.gates]                  # :270-285
        sets = permutations_evaluated[i]                                                 # permutation/verifier.rs:102-200
        if sets:
            expressions.append(l_0 * (1 - sets[0][0]) % R)
            expressions.append((sets[-1][0] * sets[-1][0] - sets[-1][0]) * l_last % R)
            for t in range(1, len(sets)):
                expressions.append((sets[t][0] - sets[t - 1][2]) * l_0 % R)
        for t, columns in enumerate(chunks):
            z_x, z_next, _ = sets[t]
            col_evals = [{"advice": advice_evals[i], "fixed": fixed_evals, "instance": instance_evals[i]}[kind][cs.query_index(kind, c, 0)]
                         for kind, c in columns]
            left = z_next
            for e, s in zip(col_evals, permutation_evals[t * chunk_len:(t + 1) * chunk_len]):
                left = left * (e + beta * s + gamma) % R
            right, current_delta = z_x, beta * x % R * pow(FR_DELTA, t * chunk_len, R) % R
            for e in col_evals:
                right = right * (e + current_delta + gamma) % R
                current_delta = current_delta * FR_DELTA % R
            expressions.append((left - right) * active_rows % R)
        for (inp, tab), (z_x, z_next, a_x, a_inv, s_x) in zip(cs.lookups, lookups_evaluated[i]):   # lookup/verifier.rs:93-168
            compressed = []
            for exprs in (inp, tab):                                                     # :116-134: acc = acc theta + e
                acc = 0
                for e in exprs:
                    acc = (acc * theta + ev(e)) % R
                compressed.append(acc)
            left = z_next * (a_x + beta) % R * (s_x + gamma) % R
            right = z_x * (compressed[0] + beta) % R * (compressed[1] + gamma) % R
            expressions.append(l_0 * (1 - z_x) % R)
            expressions.append(l_last * (z_x * z_x - z_x) % R)
            expressions.append((left - right) * active_rows % R)
            expressions.append(l_0 * (a_x - s_x) % R)
            expressions.append((a_x - s_x) * (a_x - a_inv) % R * active_rows % R)
        for (inputs, tab), (phi_x, phi_next, m_x) in zip(cs.mv_lookups, mvlookups_evaluated[i]):
            folds = [compress_evals([ev(e) for e in exprs], theta) for exprs in inputs + [tab]]
            expressions += mvlookup_expressions(l_0, l_last, active_rows, beta, folds[:-1], folds[-1], phi_x, phi_next, m_x)
        for (inp, shf), (z_x, z_next) in zip(cs.shuffles, shuffles_evaluated[i]):
            a, s = (compress_evals([ev(e) for e in exprs], theta) for exprs in (inp, shf))
            expressions += shuffle_expressions(l_0, l_last, active_rows, gamma, a, s, z_x, z_next)
    expected_h_eval = 0                                                                  # vanishing/verifier.rs:97-98
    for v in expressions:
        expected_h_eval = (expected_h_eval * y + v) % R
    if xn == 1:
        raise VerifyError("x lies in the domain")                                        # invert().unwrap()
    expected_h_eval = expected_h_eval * pow(xn - 1, -1, R) % R
    h_commitment = params_vk.empty_msm() if use_ipa else MSM()                           # :100-110
    for c in reversed(h_commitments):
        h_commitment.scale(xn)
        h_commitment.append_term(1, c)

    # ---- the opening queries (:326-388): (commitment id, point, evaluation)
    commitments, queries = [], []

    def cid(c):
        """one id per commitment, shared by all its queries; for IPA the id's entry is the ipa.Commitment handle VerifierIPA compares"""
        if use_ipa:
            c = ipa.Commitment(msm=c) if isinstance(c, ipa.MSMIPA) else ipa.Commitment(point=c)
        commitments.append(c)
        return len(commitments) - 1

    x_next, x_inv, x_last = dom.rotate_omega(x, 1), dom.rotate_omega(x, -1), dom.rotate_omega(x, -(b + 1))
    fixed_ids = [cid(c) for c in vk.fixed_commitments]
    common_ids = [cid(c) for c in vk.permutation_commitments]
    for i in range(num_proofs):
        if use_ipa:                                                                      # :343-355: instance queries first
            ids = [cid(c) for c in instance_commitments[i]]
            for q, (c, r) in enumerate(cs.instance_queries):
                queries.append((ids[c], dom.rotate_omega(x, r), instance_evals[i][q]))
        ids = [cid(c) for c in advice_commitments[i]]
        for q, (c, r) in enumerate(cs.advice_queries):                                   # :356-364
            queries.append((ids[c], dom.rotate_omega(x, r), advice_evals[i][q]))
        ids = [cid(c) for c in permutations_committed[i]]                                # :365, permutation/verifier.rs:202-237
        sets = permutations_evaluated[i]
        for t in range(len(sets)):
            queries += [(ids[t], x, sets[t][0]), (ids[t], x_next, sets[t][1])]
        for t in reversed(range(len(sets) - 1)):
            queries.append((ids[t], x_last, sets[t][2]))
        for j in range(len(cs.lookups)):                                                 # :366-371, lookup/verifier.rs:170-209
            z_id, a_id, s_id = cid(lookups_product[i][j]), cid(lookups_permuted[i][j][0]), cid(lookups_permuted[i][j][1])
            z_x, z_next, a_x, a_inv, s_x = lookups_evaluated[i][j]
            queries += [(z_id, x, z_x), (a_id, x, a_x), (s_id, x, s_x), (a_id, x_inv, a_inv), (z_id, x_next, z_next)]
        for j in range(len(cs.mv_lookups)):
            phi_id, m_id = cid(mvlookups_phi[i][j]), cid(mvlookups_m[i][j])
            phi_x, phi_next, m_x = mvlookups_evaluated[i][j]
            queries += [(phi_id, x, phi_x), (phi_id, x_next, phi_next), (m_id, x, m_x)]
        for j in range(len(cs.shuffles)):
            z_id = cid(shuffles_product[i][j])
            queries += [(z_id, x, shuffles_evaluated[i][j][0]), (z_id, x_next, shuffles_evaluated[i][j][1])]
    for q, (c, r) in enumerate(cs.fixed_queries):                                        # :374-386
        queries.append((fixed_ids[c], dom.rotate_omega(x, r), fixed_evals[q]))
    for j in range(len(vk.permutation_commitments)):                                     # :387, permutation/verifier.rs:241-251
        queries.append((common_ids[j], x, permutation_evals[j]))
    queries.append((cid(h_commitment), x, expected_h_eval))                              # :388, vanishing/verifier.rs:122-137
    queries.append((cid(random_poly_commitment), x, random_eval))

    if use_ipa:                                                                          # :393-398
        handles = [(commitments[c], point, ev) for c, point, ev in queries]

        def opening(msm):
            guard = ipa.VerifierIPA(params_vk).verify_proof(transcript, handles, msm)
            if transcript.remaining():
                raise TranscriptError("%d bytes follow the proof" % transcript.remaining())
            return guard
        return strategy.process(opening)
    if strategy is not None:                                                             # :393-398

        def opening(msm_accumulator):
            left, right = MULTIOPEN[multiopen](transcript, _g0(params_vk), commitments, queries)
            if transcript.remaining():
                raise TranscriptError("%d bytes follow the proof" % transcript.remaining())
            msm_accumulator.left.add_msm(left)                                           # gwc/verifier.rs:121, shplonk/verifier.rs:140-142
            msm_accumulator.right.add_msm(right)                                         # gwc/verifier.rs:123-126, shplonk/verifier.rs:144
            return kzg.GuardKZG(msm_accumulator)
        return strategy.process(opening)
    left, right = MULTIOPEN[multiopen](transcript, _g0(params_vk), commitments, queries)
    if transcript.remaining():
        raise TranscriptError("%d bytes follow the proof" % transcript.remaining())
    return left.eval(), right.eval()
