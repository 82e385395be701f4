"""The shuffle argument end to end, judged by the polynomial identity itself and not by a model of the kernels: for a valid shuffle the
numerator the engine folds into h(X) is divisible by X^n - 1, so with q = extended_to_coeff(divide_by_vanishing_poly(h)) and any point
x outside the domain, numerator(x) -- Python integers over the column polynomials at x and omega x -- equals q(x) (x^n - 1).  A wrong
fold, a wrong rotation, a wrong product column or a wrong order of the y powers breaks the equality; so does one changed cell of S."""
import numpy as np
import pytest

from evalh_util import Evaluator
from shuffle_util import R_MOD, failing_rows, from_mont, to_mont

J, K, B = 4, 6, 3
N = 1 << K
U = N - B - 1
A = lambda c, r=0: ('advice', c, r)  # noqa: E731
SHUFFLE = ([A(0), A(1)], [A(2), A(3)])


def _ints(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R_MOD for _ in range(count)]


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R_MOD
    return acc


def _witness():
    """a0, a1 random; (s0, s1) the same 2-tuples in another row order on [0, u); rows >= u random in every column"""
    perm = [int(p) for p in np.random.default_rng(11).permutation(U)]
    a0, a1 = _ints(1, N), _ints(2, N)
    s0 = [a0[p] for p in perm] + _ints(3, N - U)
    s1 = [a1[p] for p in perm] + _ints(4, N - U)
    return [a0, a1, s0, s1]


def _numerator_and_quotient(h2, dom, cols, z, q_of, theta, gamma, y):
    """(numerator(x), q(x) (x^n - 1)) at a fixed x outside the domain.  q_of(case pieces) runs the engine."""
    x = 0x1234567890abcdef1234567890abcdef % R_MOD
    omega = dom.ints["omega"]
    assert pow(x, 1 << dom.extended_k, R_MOD) != 1
    polys = [from_mont(p) for p in dom.lagrange_to_coeff_batch([to_mont(c) for c in cols] + [z])]
    l0_col, l_last_col = [1] + [0] * (N - 1), [0] * U + [1] + [0] * (N - U - 1)
    l_active_col = [1] * U + [0] * (N - U)
    key_polys = dom.lagrange_to_coeff_batch([to_mont(l0_col), to_mont(l_last_col), to_mont(l_active_col)])
    l0, l_last, l_active = (_horner(from_mont(p), x) for p in key_polys)
    a0, a1, s0, s1, zx = (_horner(p, x) for p in polys)
    z_next = _horner(polys[4], omega * x % R_MOD)
    a = (a0 * theta + a1 + gamma) % R_MOD
    s = (s0 * theta + s1 + gamma) % R_MOD
    num = 0
    for term in ((1 - zx) * l0, (zx * zx - zx) * l_last, l_active * (z_next * s - zx * a)):
        num = (num * y + term) % R_MOD
    q = from_mont(q_of(polys_mont=[to_mont(p) for p in polys], key_polys=key_polys))
    assert len(q) == 3 * N
    return num, _horner(q, x) * (pow(x, N, R_MOD) - 1) % R_MOD


@pytest.mark.gpu
def test_gpu_identity_end_to_end(h2, oracle):
    h2.init()
    dom = h2.EvaluationDomain.new(J, K)
    assert dom.extended_k == K + 2
    size = 1 << dom.extended_k
    theta, gamma, y = _ints(20, 3)
    blinding = to_mont(_ints(21, B))
    ev = Evaluator.new([], [], [SHUFFLE])
    from evalh_util import flatten_graph, lookup_compress_graphs
    graphs = [flatten_graph(g) for g in lookup_compress_graphs(*SHUFFLE)]
    l0_c, l_last_c, l_active_c = h2.key_lagrange_columns(dom, B)
    empty = np.zeros(0, dtype=np.uint32)
    common = {"k": K, "extended_k": dom.extended_k, "extended_omega": dom.extended_omega, "g_coset": dom.g_coset, "g_coset_inv": dom.g_coset_inv,
              "zeta": oracle.constant(oracle.FR, 5), "delta": oracle.fe_from_int(oracle.FR, pow(7, 1 << 28, R_MOD)),
              "y": to_mont([y])[0], "beta": to_mont([0])[0], "gamma": to_mont([gamma])[0], "theta": to_mont([theta])[0],
              "challenges": np.zeros((0, 4), dtype=np.uint64), "instance_polys": [], "perm_column_kind": empty, "perm_column_index": empty,
              "chunk_len": 2, "last_rotation": -(B + 1), "lookups": []}

    def run(cols, form):
        mont = [to_mont(c) for c in cols]
        comp_a, comp_s = h2.lookup_compress(K, graphs, common["theta"], advice=mont)
        z = h2.shuffle_products(K, common["gamma"], [comp_a], [comp_s], blinding, B)[0]

        def q_of(polys_mont, key_polys):
            zeros = np.zeros((size, 4), dtype=np.uint64)
            if form == "full":
                for got, poly in zip((l0_c, l_last_c, l_active_c), key_polys):
                    assert np.array_equal(got, dom.coeff_to_extended(poly))  # the key's cosets are those of the polynomials used at x
                case = {**common, "fixed_cosets": [], "perm_product_cosets": [], "perm_cosets": [], "l0": l0_c, "l_last": l_last_c,
                        "l_active_row": l_active_c, "advice_polys": polys_mont[:4], "shuffles": [polys_mont[4]]}
                return dom.extended_to_coeff(dom.divide_by_vanishing_poly(ev.evaluate_h(case, zeros)))
            case = {**common, "fixed_polys": [], "perm_product_polys": [], "perm_polys": [], "l0_poly": key_polys[0], "l_last_poly": key_polys[1],
                    "l_active_row_poly": key_polys[2], "advice_polys": polys_mont[:4], "shuffles": [polys_mont[4]]}
            return dom.extended_to_coeff(ev.evaluate_h_parts(case, zeros, t_evaluations=dom.t_evaluations))

        return comp_a, comp_s, z, _numerator_and_quotient(h2, dom, cols, z, q_of, theta, gamma, y)

    good = _witness()
    for form in ("full", "parts"):
        comp_a, comp_s, z, (num, qv) = run(good, form)
        assert from_mont(z)[U] == 1 and num != 0
        assert num == qv, form
    counts, rows = h2.check_shuffles(K, [comp_a], [comp_s], B, 8)
    assert counts[0] == 0 and list(rows[0]) == [0xFFFFFFFF] * 8

    bad = [list(c) for c in good]
    bad[3][5] = (bad[3][5] + 1) % R_MOD  # one cell of S
    for form in ("full", "parts"):
        comp_a, comp_s, z, (num, qv) = run(bad, form)
        assert num != qv, form
    want = failing_rows(from_mont(comp_a), from_mont(comp_s), B)
    assert len(want) == 1 and from_mont(comp_s)[5] != from_mont(h2.lookup_compress(K, graphs, common["theta"], advice=[to_mont(c) for c in good])[1])[5]
    counts, rows = h2.check_shuffles(K, [comp_a], [comp_s], B, 8)
    assert counts[0] == len(want) and list(rows[0]) == want + [0xFFFFFFFF] * (8 - len(want))


@pytest.mark.gpu
def test_gpu_commit_shuffle_products(h2):
    """commit_shuffle_products composes compress, product, commit and the transform to coefficients"""
    h2.init()
    dom = h2.EvaluationDomain.new(J, K)
    theta, gamma = (to_mont([v])[0] for v in _ints(30, 2))
    blinding = to_mont(_ints(31, B))
    advice = [to_mont(c) for c in _witness()]
    with h2.ParamsKZG.setup(K, to_mont([12345])[0]) as params:
        out = h2.commit_shuffle_products(params, dom, [SHUFFLE], theta, gamma, blinding, B, [to_mont([9])[0]], advice=advice)
        want_commitment = params.commit_lagrange(out[0]["product"], None)
    from evalh_util import flatten_graph, lookup_compress_graphs
    comp = h2.lookup_compress(K, [flatten_graph(g) for g in lookup_compress_graphs(*SHUFFLE)], theta, advice=advice)
    z = h2.shuffle_products(K, gamma, comp[:1], comp[1:], blinding, B)[0]
    assert len(out) == 1 and np.array_equal(out[0]["product"], z) and from_mont(z)[U] == 1
    assert np.array_equal(out[0]["compressed_input"], comp[0]) and np.array_equal(out[0]["compressed_shuffle"], comp[1])
    assert np.array_equal(out[0]["product_poly"], dom.lagrange_to_coeff(z))
    # a Jacobian point has many representations (the engine's MSM forms differ in theirs): the commitments are compared as affine points
    assert np.array_equal(h2.g1_to_affine(out[0]["product_commitment"]), h2.g1_to_affine(want_commitment))
