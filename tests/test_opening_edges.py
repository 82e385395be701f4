"""The opening kernels (csrc/opening.hip) on extreme stored words.

poly_combine sums eight fused two-product reductions before it canonicalises ("< p + 8 x 1.4 p"), and the division keeps a Horner
accumulator and a scan carry lazily reduced ("below 2.5 p", "below 1.25 p"); eval_polynomials runs the same Horner and carry over
partial tiles.  tests/test_opening.py feeds them uniformly random elements.  Here every polynomial, scalar, sub coefficient, scale
and accumulate target is built from the stored words of ntt_edge_util -- all r - 1, all limbmax, seeded extremes -- with polynomial
counts on both sides of the canonicalise-after-eight-pairs step, roots 0 / the elements stored as 1 and r - 1 / repeated, and every
tile shape, against the Python-integer restatement of opening_util.  Every comparison is np.array_equal."""
import functools

import numpy as np
import pytest

import ntt_edge_util as eu
import opening_util as ou
from opening_util import R_MOD
from test_opening import TILE_SHAPES, tile  # noqa: F401  (the fixture)

PATTERNS = ("r-1", "limbmax", "extremes")
W_ONE, W_TOP = 1, R_MOD - 1  # stored WORDS (the field elements 2^-256 and -2^-256), not the field's one and minus one


def _words(pattern, n, seed):
    if pattern == "extremes":
        return eu.extremes(n, seed)
    return eu.const(n, eu.VALUES[pattern])


def _field(a):
    """the field elements a column of stored words holds"""
    return ou.from_mont(a)


def _roots_for(pattern, n):
    """stored words of the roots: 0; the words 1 and r - 1; a repeated root.  A polynomial of n coefficients takes at most n roots"""
    roots = {"r-1": [0], "limbmax": [W_ONE, W_TOP], "extremes": [W_TOP, W_TOP, W_TOP]}[pattern]
    return roots[:n]


@functools.lru_cache(maxsize=None)
def _combine_case(n_polys, n, pattern):
    """inputs as stored words and the restated result, computed once and shared by every tile shape; read-only"""
    polys = [_words(pattern, n, 100 * j + n) for j in range(n_polys)]
    scal = _words(pattern, n_polys, 7000 + n)
    sub = _words(pattern, min(n, 3), 7100 + n)
    scale = _words(pattern, 1, 7200 + n)[0]
    roots = eu.words(_roots_for(pattern, n))
    target = _words(pattern, n, 7300 + n)
    fp, fs, fsub, fr = [_field(p) for p in polys], _field(scal), _field(sub), _field(roots)
    a = ou.combine(fp, fs, fsub)
    q = ou.combine(fp, fs, fsub, fr, _field(scale)[0])
    out = dict(polys=polys, scal=scal, sub=sub, scale=scale, roots=roots, target=target, q=ou.to_mont(q) if q else np.zeros((0, 4), np.uint64),
               rem=ou.fe(ou.eval_polynomial(a, fr[0])), acc=ou.to_mont([(t + c) % R_MOD for t, c in zip(_field(target), q)]) if q else None)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("n_polys", [1, 2, 15, 16, 17, 32, 33])
def test_poly_combine_on_extreme_words(h2, tile, n_polys, n):  # noqa: F811
    """sum_j s_j p_j - sub, divided by every root, times scale, and accumulated onto a target of extreme words: host form under every
    tile shape, device form, remainder a(roots[0])"""
    import torch
    h2.init()
    for pattern in PATTERNS:
        c = _combine_case(n_polys, n, pattern)
        lout = n - len(c["roots"])
        want = np.zeros((lout + 3, 4), dtype=np.uint64)
        want[:lout] = c["q"]
        kw = dict(sub=c["sub"], roots=c["roots"], scale=c["scale"], out_len=lout + 3)
        for r, b in TILE_SHAPES:
            tile(r, b)
            got, rem = h2.poly_combine(c["polys"], c["scal"], remainder=True, **kw)
            eu.assert_below_r(got, (pattern, r, b))
            assert np.array_equal(got, want), (pattern, r, b, np.flatnonzero((got != want).any(axis=1))[:8])
            assert np.array_equal(rem, c["rem"]) and eu.below_r(rem).all(), (pattern, r, b)
            if lout:
                out = np.concatenate([c["target"][:lout], eu.const(3, R_MOD - 1)])
                h2.poly_combine(c["polys"], c["scal"], out=out, accumulate=True, **kw)
                eu.assert_below_r(out, (pattern, r, b, "accumulate"))
                assert np.array_equal(out[:lout], c["acc"][:lout]) and np.array_equal(out[lout:], eu.const(3, R_MOD - 1)), (pattern, r, b)
        tile(0, 0)
        dev = [torch.from_numpy(p.view(np.int64).copy()).cuda() for p in c["polys"]]
        for r, b in [(0, 0), (1, 4)]:
            tile(r, b)
            d_out = torch.full((lout + 3, 4), -1, dtype=torch.int64, device="cuda")
            rem = h2.poly_combine_device(dev, c["scal"], d_out, sub=c["sub"], roots=c["roots"], scale=c["scale"], remainder=True)
            assert np.array_equal(h2.to_numpy_u64(d_out), want) and np.array_equal(rem, c["rem"]), (pattern, r, b, "device form")


EVAL_LENS = (1, 255, 256, 257, 3000)


@functools.lru_cache(maxsize=None)
def _eval_case():
    polys, qp, pts = [], [], []
    w = ou.root_of_unity(12)
    points = np.concatenate([ou.to_mont([0, 1, R_MOD - 1, w]), eu.words([W_TOP])])
    fpts = _field(points)
    want = []
    for pattern in PATTERNS:
        for n in EVAL_LENS:
            p = _words(pattern, n, 300 + n)
            fp = _field(p)
            for x in fpts:
                qp.append(len(polys))
                want.append(ou.eval_polynomial(fp, x))
            polys.append(p)
            pts.append(points)
    return polys, qp, np.concatenate(pts), ou.to_mont(want)


@pytest.mark.gpu
def test_eval_polynomials_on_extreme_words(h2, tile):  # noqa: F811
    """the same polynomials at 0, 1, -1, a root of unity and the element stored as r - 1, lengths 1, 255, 256, 257 and 3000, under the
    default and the small tiles (where the partial and carry path runs), host and device forms"""
    import torch
    h2.init()
    polys, qp, pts, want = _eval_case()
    dev = [torch.from_numpy(p.view(np.int64).copy()).cuda() for p in polys]
    for r, b in [(0, 0), (1, 1), (2, 4), (1, 64), (8, 32), (64, 256)]:
        tile(r, b)
        got = h2.eval_polynomials(polys, qp, pts)
        eu.assert_below_r(got, (r, b))
        assert np.array_equal(got, want), (r, b, np.flatnonzero((got != want).any(axis=1))[:8])
        assert np.array_equal(h2.eval_polynomials_device(dev, qp, pts), want), (r, b, "device form")


def test_opening_edge_inputs_are_what_they_claim():
    """CPU: the words stay below r, the restatement is evaluated on the field elements they hold, and polynomial counts straddle 16"""
    for pattern in PATTERNS:
        a = _words(pattern, 64, 5)
        assert eu.below_r(a).all() and eu.ints(ou.to_mont(_field(a))) == eu.ints(a)
    c = _combine_case(2, 257, "limbmax")
    assert c["q"].shape == (255, 4) and eu.ints(c["roots"]) == [1, R_MOD - 1]
    fp = [_field(p) for p in c["polys"]]
    a = ou.combine(fp, _field(c["scal"]), _field(c["sub"]))
    q = ou.kate_division(a, _field(c["roots"])[0])
    assert ou.from_mont([c["rem"]])[0] == ou.eval_polynomial(a, _field(c["roots"])[0]) and len(q) == 256
    polys, qp, pts, want = _eval_case()
    assert len(polys) == 15 and want.shape == (75, 4) and pts.shape == (75, 4)
