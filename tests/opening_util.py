"""Python big-integer restatement of the reference's opening phase (test infrastructure only).

eval_polynomial, kate_division, lagrange_interpolate and evaluate_vanishing_polynomial restate halo2_proofs/src/arithmetic.rs
(:304-328, :348-366, :405-460 and the vanishing-polynomial helper), div_by_vanishing poly/kzg/multiopen/shplonk/prover.rs:26-31 and
powers poly/kzg/multiopen/shplonk.rs.  gwc_witnesses restates gwc/prover.rs:61-89 and shplonk_h / shplonk_final the two stages of
shplonk/prover.rs:138-275, all given the sets construct_intermediate_sets builds and fixed challenges.  Values are canonical integers
mod r; the product_util helpers convert to and from the engine's (n, 4) uint64 Montgomery columns."""
from product_util import R_MOD, fe, from_mont, root_of_unity, to_mont  # noqa: F401


def eval_polynomial(poly, point):
    """arithmetic.rs:304-328: Horner from the top; a length-0 polynomial is zero"""
    acc = 0
    for c in reversed(poly):
        acc = (acc * point + c) % R_MOD
    return acc


def kate_division(a, b):
    """arithmetic.rs:348-366: q[L - 2] = a[L - 1], q[i] = a[i + 1] + b q[i + 1]; the remainder a(b) is dropped"""
    q = [0] * (len(a) - 1)
    tmp = 0
    for i in range(len(a) - 1, 0, -1):
        lead = (a[i] + tmp) % R_MOD  # lead_coeff = a[i] - tmp with tmp = lead * (-b)
        q[i - 1] = lead
        tmp = lead * b % R_MOD
    return q


def div_by_vanishing(a, roots):
    """shplonk/prover.rs:26-31"""
    for r in roots:
        a = kate_division(a, r)
    return a


def lagrange_interpolate(points, evals):
    """arithmetic.rs:405-460: sum_j evals[j] prod_{k != j} (X - x_k) / (x_j - x_k), coefficients low first"""
    assert len(points) == len(evals)
    m = len(points)
    if m == 1:
        return [evals[0] % R_MOD]
    final = [0] * m
    for j in range(m):
        tmp = [1]
        for k in range(m):
            if k == j:
                continue
            inv = pow((points[j] - points[k]) % R_MOD, -1, R_MOD)
            # product[i] = tmp[i] (-denom x_k) + tmp[i - 1] denom
            tmp = [((tmp[i] if i < len(tmp) else 0) * (-inv * points[k]) + (tmp[i - 1] if i else 0) * inv) % R_MOD
                   for i in range(len(tmp) + 1)]
        for i in range(m):
            final[i] = (final[i] + tmp[i] * evals[j]) % R_MOD
    return final


def evaluate_vanishing_polynomial(roots, z):
    """prod (z - r)"""
    acc = 1
    for r in roots:
        acc = acc * (z - r) % R_MOD
    return acc


def powers(x, m):
    """the first m elements of powers(x): 1, x, x^2, ..."""
    out, acc = [], 1
    for _ in range(m):
        out.append(acc)
        acc = acc * x % R_MOD
    return out


def lin_comb(polys, scalars, n=None):
    n = max(len(p) for p in polys) if n is None else n
    out = [0] * n
    for p, s in zip(polys, scalars):
        for i, c in enumerate(p):
            out[i] = (out[i] + s * c) % R_MOD
    return out


def combine(polys, scalars, sub=(), roots=(), scale=1):
    """the engine's primitive, restated: (sum_j s_j p_j - sub) divided by every root in order, times scale"""
    a = lin_comb(polys, scalars, len(polys[0]))
    for i, s in enumerate(sub):
        a[i] = (a[i] - s) % R_MOD
    return [scale * c % R_MOD for c in div_by_vanishing(a, list(roots))]


def gwc_witnesses(polys, point_groups, v):
    """gwc/prover.rs:61-89; point_groups: [(point, [(poly index, eval), ...]), ...] in construct_intermediate_sets' order"""
    out = []
    for z, queries in point_groups:
        pw = powers(v, len(queries))
        poly_batch = lin_comb([polys[j] for j, _ in queries], pw)
        eval_batch = sum(p * e for p, (_, e) in zip(pw, queries)) % R_MOD
        poly_batch[0] = (poly_batch[0] - eval_batch) % R_MOD
        out.append(kate_division(poly_batch, z))
    return out


def super_point_set(rotation_sets):
    out = []
    for points, _ in rotation_sets:
        for x in points:
            if x not in out:
                out.append(x)
    return out


def shplonk_h(polys, rotation_sets, y, v):
    """shplonk/prover.rs:138-203; rotation_sets: [(points, [(poly index, [eval at each point]), ...]), ...].  h_x has n coefficients"""
    n = len(polys[0])
    h = [0] * n
    for i, (points, commitments) in enumerate(rotation_sets):
        numerators = []
        for j, evals in commitments:  # quotient_contribution: P - R on the low coefficients
            r = lagrange_interpolate(points, evals)
            p = list(polys[j])
            for t, c in enumerate(r):
                p[t] = (p[t] - c) % R_MOD
            numerators.append(p)
        n_x = lin_comb(numerators, powers(y, len(numerators)), n)
        q = div_by_vanishing(n_x, points)
        q = q + [0] * (n - len(q))
        vi = pow(v, i, R_MOD)
        h = [(a + vi * b) % R_MOD for a, b in zip(h, q)]
    return h


def shplonk_linearisation(polys, rotation_sets, h_x, y, v, u):
    """shplonk/prover.rs:209-260: l_x (which vanishes at u) and z_diffs"""
    n = len(polys[0])
    sup = super_point_set(rotation_sets)
    l_x, z_diffs = [0] * n, []
    for i, (points, commitments) in enumerate(rotation_sets):
        diffs = [x for x in sup if x not in points]
        z_i = evaluate_vanishing_polynomial(diffs, u)
        inner = []
        for j, evals in commitments:  # linearisation_contribution: P - R(u)
            p = list(polys[j])
            p[0] = (p[0] - eval_polynomial(lagrange_interpolate(points, evals), u)) % R_MOD
            inner.append(p)
        li = lin_comb(inner, powers(y, len(inner)), n)
        w = pow(v, i, R_MOD) * z_i % R_MOD
        l_x = [(a + w * b) % R_MOD for a, b in zip(l_x, li)]
        z_diffs.append(z_i)
    zt = evaluate_vanishing_polynomial(sup, u)
    l_x = [(a - zt * b) % R_MOD for a, b in zip(l_x, h_x)]
    return l_x, z_diffs


def shplonk_final(polys, rotation_sets, h_x, y, v, u):
    """shplonk/prover.rs:261-275: l_x / (X - u), normalised by z_diffs[0]^-1"""
    l_x, z_diffs = shplonk_linearisation(polys, rotation_sets, h_x, y, v, u)
    z0inv = pow(z_diffs[0], -1, R_MOD)
    return [c * z0inv % R_MOD for c in div_by_vanishing(l_x, [u])]


# The opening of the config-5 circuit (MyCircuit of examples/circuit-layout.rs, 5 advice, 6 fixed, a permutation over
# 3 columns in 2 sets, 1 lookup), from the query lists of create_proof: advice 5 and fixed 6 at x (plonk/prover.rs:529-568), the 3
# permutation polys at x and the 2 set products at x, x omega (set 0 also at x omega^last; permutation/prover.rs:227-275), the lookup's
# product at x, x omega, permuted input at x, x omega^-1 and permuted table at x (lookup/prover.rs:319-323), h and the random poly at x
# (vanishing/prover.rs:145).  21 polynomials, 26 queries, 4 points; SHPLONK's rotation sets by point set, GWC's groups by point.
CONFIG5_POLYS = 21
CONFIG5_SETS = [(("x",), list(range(17))),           # advice 0-4, fixed 5-10, permutation polys 11-13, permuted table 14, h 15, random 16
                (("x", "xw"), [17, 18]),              # permutation set 1 product, lookup product
                (("x", "xw", "xlast"), [19]),         # permutation set 0 product
                (("x", "xwinv"), [20])]               # permuted input
CONFIG5_QUERIES = sum(len(p) * len(c) for p, c in CONFIG5_SETS)


def config5_points(k, x):
    """the four opening points: x, x omega, x omega^-(blinding_factors + 1) (the config-5 circuit has 5 blinding factors), x omega^-1"""
    w = root_of_unity(k)
    return {"x": x, "xw": x * w % R_MOD, "xlast": x * pow(w, -6, R_MOD) % R_MOD, "xwinv": x * pow(w, -1, R_MOD) % R_MOD}


def config5_gwc_groups():
    """GWC's point groups: per point (in order of first use), the polynomials queried there"""
    order, groups = [], {}
    for pts, cols in CONFIG5_SETS:
        for p in pts:
            if p not in groups:
                order.append(p)
                groups[p] = []
            groups[p].extend(cols)
    return [(p, sorted(groups[p])) for p in order]
