"""The mv-lookup argument end to end, judged by the polynomial identity itself and not by a model of the kernels: compress ->
multiplicities -> sums -> lagrange_to_coeff -> evaluate_h.  For a valid argument the numerator the engine folds into h(X) is divisible
by X^n - 1: the quotient q = extended_to_coeff(divide_by_vanishing_poly(h)) has zero coefficients above its degree bound, and at any
point x outside the domain numerator(x) -- Python integers over the column polynomials at x and omega x -- equals q(x) (x^n - 1).  A
wrong fold, a wrong rotation, a wrong m or phi column or a wrong order of the y powers breaks both; so does one changed input cell."""
import numpy as np
import pytest

from evalh_util import Evaluator, flatten_graph, lookup_compress_graphs
from mvlookup_util import R_MOD, from_mont, required_degree, to_mont

K, B = 6, 3
N = 1 << K
U = N - B - 1
A = lambda c, r=0: ('advice', c, r)  # noqa: E731
ARG = ([[A(0), A(1)], [A(2), A(3)]], [A(4), A(5)])  # two input pairs share one table of pairs
J = required_degree(*ARG)  # 2 + 1 + (1 + 1): the quotient takes 2^(k + 2) rows
# the numerator's largest term is l_active tau f_0 f_1 phi(wX): degree 5 (n - 1); the quotient's degree is at most that minus n
Q_DEGREE = 5 * (N - 1) - N


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R_MOD
    return acc


def _witness():
    """t0, t1 random; each input pair a table row below u; rows >= u random in every column"""
    t0, t1 = _ints(1, N), _ints(2, N)
    rng = np.random.default_rng(11)
    cols = []
    for s in range(2):
        rows = [int(r) for r in rng.integers(0, U, U)]
        cols += [[t0[r] for r in rows] + _ints(3 + 2 * s, N - U), [t1[r] for r in rows] + _ints(4 + 2 * s, N - U)]
    return cols + [t0, t1]


def _graphs():
    inputs, tab = ARG
    return [flatten_graph(lookup_compress_graphs(inp, tab)[0]) for inp in inputs] + [flatten_graph(lookup_compress_graphs(inputs[0], tab)[1])]


def _common(dom, oracle, theta, beta, y):
    empty = np.zeros(0, dtype=np.uint32)
    return {"k": K, "extended_k": dom.extended_k, "extended_omega": dom.extended_omega, "g_coset": dom.g_coset, "g_coset_inv": dom.g_coset_inv,
            "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
            "y": to_mont([y])[0], "beta": to_mont([beta])[0], "gamma": to_mont([0])[0], "theta": to_mont([theta])[0],
            "challenges": np.zeros((0, 4), dtype=np.uint64), "instance_polys": [], "perm_column_kind": empty, "perm_column_index": empty,
            "chunk_len": 2, "last_rotation": -(B + 1), "lookups": []}


@pytest.mark.gpu
def test_gpu_identity_end_to_end(h2, oracle):
    h2.init()
    dom = h2.EvaluationDomain.new(J, K)
    assert J == 5 and dom.extended_k == K + 2
    size = 1 << dom.extended_k
    assert Q_DEGREE < size - 1  # there are coefficients above the bound to look at
    theta, beta, y = _ints(20, 3)
    blinding = to_mont(_ints(21, B))
    ev = Evaluator.new([], [], [], [ARG])
    common = _common(dom, oracle, theta, beta, y)
    l0_c, l_last_c, l_active_c = h2.key_lagrange_columns(dom, B)
    l0_col, l_last_col = [1] + [0] * (N - 1), [0] * U + [1] + [0] * (N - U - 1)
    l_active_col = [1] * U + [0] * (N - U)
    key_polys = dom.lagrange_to_coeff_batch([to_mont(l0_col), to_mont(l_last_col), to_mont(l_active_col)])
    x = 0x1234567890abcdef1234567890abcdef % R_MOD
    assert pow(x, size, R_MOD) != 1

    def run(cols, form):
        mont = [to_mont(c) for c in cols]
        comp = h2.lookup_compress(K, _graphs(), common["theta"], advice=mont)
        m, msg = h2.mvlookup_multiplicities(K, [comp[:2]], [comp[2]], B, partial=True)
        phi = h2.mvlookup_sums(K, common["beta"], [comp[:2]], [comp[2]], m, blinding, B)[0]
        polys_mont = dom.lagrange_to_coeff_batch(mont + [phi, m[0]])
        zeros = np.zeros((size, 4), dtype=np.uint64)
        if form == "full":
            for got, poly in zip((l0_c, l_last_c, l_active_c), key_polys):
                assert np.array_equal(got, dom.coeff_to_extended(poly))  # the key's cosets are those of the polynomials used at x
            case = {**common, "fixed_cosets": [], "perm_product_cosets": [], "perm_cosets": [], "l0": l0_c, "l_last": l_last_c,
                    "l_active_row": l_active_c, "advice_polys": polys_mont[:6], "mvlookups": [(polys_mont[6], polys_mont[7])]}
            q = dom.extended_to_coeff(dom.divide_by_vanishing_poly(ev.evaluate_h(case, zeros)))
        else:
            case = {**common, "fixed_polys": [], "perm_product_polys": [], "perm_polys": [], "l0_poly": key_polys[0], "l_last_poly": key_polys[1],
                    "l_active_row_poly": key_polys[2], "advice_polys": polys_mont[:6], "mvlookups": [(polys_mont[6], polys_mont[7])]}
            q = dom.extended_to_coeff(ev.evaluate_h_parts(case, zeros, t_evaluations=dom.t_evaluations))
        q = from_mont(q)
        assert len(q) == size
        # the numerator at x, on Python integers
        polys = [from_mont(p) for p in polys_mont]
        l0, l_last, l_active = (_horner(from_mont(p), x) for p in key_polys)
        a0, a1, a2, a3, t0, t1, px, mx = (_horner(p, x) for p in polys)
        p_next = _horner(polys[6], dom.ints["omega"] * x % R_MOD)
        f0, f1, tau = ((a0 * theta + a1 + beta) % R_MOD, (a2 * theta + a3 + beta) % R_MOD, (t0 * theta + t1 + beta) % R_MOD)
        num = 0
        for term in (l0 * px, l_last * px, l_active * (tau * f0 * f1 * (p_next - px) - tau * (f0 + f1) + mx * f0 * f1)):
            num = (num * y + term) % R_MOD
        return msg, from_mont(phi), q, num, _horner(q, x) * (pow(x, N, R_MOD) - 1) % R_MOD

    good = _witness()
    for form in ("full", "parts"):
        msg, phi, q, num, qv = run(good, form)
        assert msg is None and phi[0] == 0 and phi[U] == 0 and num != 0
        assert not any(q[Q_DEGREE + 1:]) and q[Q_DEGREE] != 0, form
        assert num == qv, form

    bad = [list(c) for c in good]
    bad[3][5] = (bad[3][5] + 1) % R_MOD  # one cell of the second input: its pair is no table row any more
    for form in ("full", "parts"):
        msg, phi, q, num, qv = run(bad, form)
        assert msg is not None and "argument 0, input 1:" in msg and phi[U] != 0
        assert any(q[Q_DEGREE + 1:]), form
        assert num != qv, form
    # the witness check sees the same cell
    comp = h2.lookup_compress(K, _graphs(), common["theta"], advice=[to_mont(c) for c in bad])
    counts, rows = h2.check_lookups(K, comp[:2], [comp[2], comp[2]], B, 8)
    assert list(counts) == [0, 1] and rows[1][0] == 5
    fails = h2.verify_witness(K, [], [], common["theta"], B, [], None, advice=[to_mont(c) for c in bad], mvlookups=[ARG])
    assert fails == [("mvlookup", 1, 5)]
    assert h2.verify_witness(K, [], [], common["theta"], B, [], None, advice=[to_mont(c) for c in good], mvlookups=[ARG]) == []


@pytest.mark.gpu
def test_gpu_commit_mvlookup(h2):
    """commit_mvlookup composes compress, multiplicities, sums, the two commits and the transforms to coefficients"""
    h2.init()
    dom = h2.EvaluationDomain.new(J, K)
    theta, beta = (to_mont([v])[0] for v in _ints(30, 2))
    blinding = to_mont(_ints(31, B))
    advice = [to_mont(c) for c in _witness()]
    blinds = [to_mont([9])[0], to_mont([10])[0]]
    with h2.ParamsKZG.setup(K, to_mont([12345])[0]) as params:
        out = h2.commit_mvlookup(params, dom, [ARG], theta, beta, blinding, B, blinds, advice=advice)
        want_m, want_phi = params.commit_lagrange(out[0]["m"], None), params.commit_lagrange(out[0]["phi"], None)
    comp = h2.lookup_compress(K, _graphs(), theta, advice=advice)
    m = h2.mvlookup_multiplicities(K, [comp[:2]], [comp[2]], B)
    phi = h2.mvlookup_sums(K, beta, [comp[:2]], [comp[2]], m, blinding, B)[0]
    assert len(out) == 1 and np.array_equal(out[0]["m"], m[0]) and np.array_equal(out[0]["phi"], phi) and from_mont(phi)[U] == 0
    assert sum(from_mont(m[0])) == 2 * U
    assert all(np.array_equal(a, b) for a, b in zip(out[0]["compressed_inputs"], comp[:2])) and np.array_equal(out[0]["compressed_table"], comp[2])
    assert np.array_equal(out[0]["m_poly"], dom.lagrange_to_coeff(m[0])) and np.array_equal(out[0]["phi_poly"], dom.lagrange_to_coeff(phi))
    # a Jacobian point has many representations (the engine's MSM forms differ in theirs): the commitments are compared as affine points
    assert np.array_equal(h2.g1_to_affine(out[0]["m_commitment"]), h2.g1_to_affine(want_m))
    assert np.array_equal(h2.g1_to_affine(out[0]["phi_commitment"]), h2.g1_to_affine(want_phi))
