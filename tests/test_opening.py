"""The opening phase: batched query evaluations (h2hip_eval_polynomials_bn254) and the combine / divide / scale primitive
(h2hip_poly_combine_bn254_fr) with GWC and SHPLONK composed over it.  The restatement in opening_util.py is checked by identities
of its own, then the engine against it limb for limb, and by the recurrence and the remainder where the restatement is too slow."""
import os
import random
import subprocess

import numpy as np
import pytest

import opening_util as ou
from opening_util import R_MOD

TILE_SHAPES = [(1, 1), (1, 2), (2, 4), (4, 8), (1, 64), (8, 32), (16, 256), (64, 256), (0, 0)]


def rand_poly(rng, n):
    return [rng.randrange(R_MOD) for _ in range(n)]


def rand_mont(seed, n):
    """n random reduced elements as (n, 4) Montgomery limbs, made directly (the top limb below r's)"""
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(0x30644e72e131a029)
    return a


def mont_ints(a):
    """raw integers of (n, 4) limbs: the Montgomery values a R, on which Horner gives R a(x)"""
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


# ------------------------------------------------------------------ the restatement checks itself (CPU)
def test_restated_kate_division_identity():
    rng = random.Random(0x0E1)
    for n in (1, 2, 3, 17, 64):
        a = rand_poly(rng, n)
        b = rng.randrange(R_MOD)
        q = ou.kate_division(a, b)
        rem = ou.eval_polynomial(a, b)
        for _ in range(3):  # q(X) (X - b) + a(b) = a(X) at random X
            x = rng.randrange(R_MOD)
            assert (ou.eval_polynomial(q, x) * (x - b) + rem) % R_MOD == ou.eval_polynomial(a, x)
    a = rand_poly(rng, 9)
    assert ou.kate_division(a, 0) == a[1:]  # division by X shifts
    assert ou.div_by_vanishing(a, [0, 0]) == a[2:]


def test_restated_interpolation_and_vanishing():
    rng = random.Random(0x0E2)
    for m in (1, 2, 3, 5):
        pts = [rng.randrange(R_MOD) for _ in range(m)]
        evs = [rng.randrange(R_MOD) for _ in range(m)]
        r = ou.lagrange_interpolate(pts, evs)
        assert len(r) == m and all(ou.eval_polynomial(r, x) == e for x, e in zip(pts, evs))
        z = rng.randrange(R_MOD)
        zpoly = [1]  # prod (X - x) built by multiplication
        for x in pts:
            zpoly = [((zpoly[i - 1] if i else 0) - x * (zpoly[i] if i < len(zpoly) else 0)) % R_MOD for i in range(len(zpoly) + 1)]
        assert ou.evaluate_vanishing_polynomial(pts, z) == ou.eval_polynomial(zpoly, z)
        assert ou.evaluate_vanishing_polynomial(pts, pts[-1]) == 0
        assert ou.div_by_vanishing(zpoly, pts) == [1]  # Z divided by its own roots
    assert ou.powers(3, 4) == [1, 3, 9, 27]


def synthetic_sets(rng, k, n_polys, n_sets):
    """rotation sets over shared polynomials; set 1 has three points; evaluations computed honestly"""
    n = 1 << k
    polys = [rand_poly(rng, n) for _ in range(n_polys)]
    w = ou.root_of_unity(k)
    x = rng.randrange(R_MOD)
    point_sets = [[x], [x, x * w % R_MOD, x * pow(w, -3, R_MOD) % R_MOD], [x, x * w % R_MOD], [x * pow(w, -1, R_MOD) % R_MOD, x],
                  [x * pow(w, 2, R_MOD) % R_MOD]][:n_sets]
    sets = []
    for s, pts in enumerate(point_sets):
        cols = sorted(rng.sample(range(n_polys), min(n_polys, 2 + s % 3)))
        sets.append((pts, [(j, [ou.eval_polynomial(polys[j], p) for p in pts]) for j in cols]))
    return polys, sets


def test_restated_shplonk_linearisation_vanishes_at_u():
    """the sanity check of shplonk/prover.rs:261-265 holds for the restatement"""
    rng = random.Random(0x0E3)
    polys, sets = synthetic_sets(rng, 4, 5, 4)
    y, v, u = (rng.randrange(R_MOD) for _ in range(3))
    h = ou.shplonk_h(polys, sets, y, v)
    l_x, _ = ou.shplonk_linearisation(polys, sets, h, y, v, u)
    assert ou.eval_polynomial(l_x, u) == 0
    sets[0][1][0][1][0] = (sets[0][1][0][1][0] + 1) % R_MOD  # a wrong evaluation: h_x no longer divides exactly
    l_x, _ = ou.shplonk_linearisation(polys, sets, ou.shplonk_h(polys, sets, y, v), y, v, u)
    assert ou.eval_polynomial(l_x, u) != 0


# ------------------------------------------------------------------ entry points without a GPU, argument validation (CPU)
def test_opening_without_gpu_fails_loudly(h2):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = ou.to_mont([1, 2, 3])
    one = ou.fe(1)
    with pytest.raises(h2.H2HipError, match="rc=2"):
        h2.eval_polynomials([a], [0], [one])
    with pytest.raises(h2.H2HipError, match="rc=2"):
        h2.poly_combine([a], [one], roots=[one])
    with pytest.raises(h2.H2HipError, match="rc=2"):
        h2.kate_division(a, one)


def test_opening_rejects_bad_arguments(h2):
    """validation happens before any device work, so it answers the same with or without a GPU"""
    a = ou.to_mont([1, 2, 3, 4])
    one = ou.fe(1)
    bad = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    rc1 = dict(match="rc=1")
    with pytest.raises(h2.H2HipError, **rc1):
        h2.eval_polynomials([a], [1], [one])                              # query_poly out of range
    with pytest.raises(h2.H2HipError, **rc1):
        h2.eval_polynomials([a], [0], [bad])                              # unreduced point
    for kw in [dict(scalars=[bad]),                                       # unreduced scalar
               dict(scalars=[one], roots=[bad]),                          # unreduced root
               dict(scalars=[one], scale=bad),                            # unreduced scale
               dict(scalars=[one], sub=[bad]),                            # unreduced sub
               dict(scalars=[one], roots=[one] * 5),                      # len < n_roots
               dict(scalars=[one], sub=[one] * 5),                        # sub_len > min(len, 16)
               dict(scalars=[one], roots=[one], out_len=2),               # out_len < len - n_roots
               dict(scalars=[one], remainder=True)]:                      # a remainder without a root
        with pytest.raises(h2.H2HipError, **rc1):
            h2.poly_combine([a], **kw)
    big = ou.to_mont(list(range(20)))
    with pytest.raises(h2.H2HipError, **rc1):
        h2.poly_combine([big], [one], sub=[one] * 17)                     # sub_len > 16
    with pytest.raises(h2.H2HipError, **rc1):
        h2.poly_combine([big], [one], roots=[one] * 17)                   # more than 16 roots
    lib = h2.lib()
    import ctypes
    p = (ctypes.c_void_p * 1)(a.ctypes.data)
    one_c = one.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((4, 4), dtype=np.uint64)
    assert lib.h2hip_poly_combine_bn254_fr(p, ctypes.c_size_t((1 << 28) + 1), one_c, ctypes.c_size_t(1), None, ctypes.c_size_t(0), None,
                                           ctypes.c_size_t(0), one_c, ctypes.c_uint32(0), out.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_size_t((1 << 28) + 1), None) == 1  # length above 2^28
    lens = (ctypes.c_size_t * 1)((1 << 28) + 1)
    q = np.zeros(1, dtype=np.uint32)
    assert lib.h2hip_eval_polynomials_bn254(p, lens, ctypes.c_size_t(1), q.ctypes.data_as(ctypes.c_void_p), one_c, ctypes.c_size_t(1),
                                            out.ctypes.data_as(ctypes.c_void_p)) == 1
    # zero polynomials / zero queries write nothing and need no device
    assert h2.eval_polynomials([a], [], []).shape == (0, 4)
    assert lib.h2hip_poly_combine_bn254_fr(None, ctypes.c_size_t(4), None, ctypes.c_size_t(0), None, ctypes.c_size_t(0), None, ctypes.c_size_t(0),
                                           one_c, ctypes.c_uint32(0), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(4), None) == 0
    with pytest.raises(h2.H2HipError, **rc1):
        h2.set_opening_tile(3, 0)
    with pytest.raises(h2.H2HipError, **rc1):
        h2.set_opening_tile(0, 512)


# ------------------------------------------------------------------ evaluations against the restatement (GPU)
@pytest.fixture
def tile(h2):
    yield h2.set_opening_tile
    h2.set_opening_tile(0, 0)


def _eval_case(seed):
    rng = random.Random(seed)
    lens = [0, 1, 2, 255, 256, 257, (1 << 16) + 3, 1 << 17]
    polys = [rand_poly(rng, n) for n in lens]
    w = ou.root_of_unity(17)
    qp, pts = [], []
    for j in range(len(polys)):
        for x in (0, 1, pow(w, rng.randrange(1 << 17), R_MOD), rng.randrange(R_MOD)):
            qp.append(j), pts.append(x)
    extra = rand_poly(rng, 3000)  # one polynomial with 1 to 9 points: more than one pass over it
    polys.append(extra)
    for m in range(1, 10):
        qp.extend([len(polys) - 1] * m)
        pts.extend(rng.randrange(R_MOD) for _ in range(m))
    polys.append(polys[5])  # the same values under a second index
    qp.extend([len(polys) - 1, 5])
    pts.extend([w, w])
    return polys, qp, pts


@pytest.mark.gpu
def test_eval_polynomials_match_reference(h2, tile):
    import torch
    polys, qp, pts = _eval_case(0xE7A1)
    want = ou.to_mont([ou.eval_polynomial(polys[j], x) for j, x in zip(qp, pts)])
    mp = [ou.to_mont(p) if p else np.zeros((0, 4), np.uint64) for p in polys]
    mp[-1] = mp[5]  # the same pointer passed twice
    mpts = ou.to_mont(pts)
    assert np.array_equal(h2.eval_polynomials(mp, qp, mpts), want)
    dev = [torch.from_numpy(a.view(np.int64).copy()).cuda() for a in mp[:-1]]
    dev.append(dev[5])
    assert np.array_equal(h2.eval_polynomials_device(dev, qp, mpts), want)
    for r, b in [(1, 1), (2, 4), (1, 64), (8, 32), (64, 256)]:
        tile(r, b)
        sel = [q for q, j in enumerate(qp) if len(polys[j]) <= 3000]
        got = h2.eval_polynomials(mp, [qp[q] for q in sel], mpts[sel])
        assert np.array_equal(got, want[sel]), (r, b)


# ------------------------------------------------------------------ combine / divide against the restatement (GPU)
def _combine_case(seed, n, n_polys, sub_len, roots):
    rng = random.Random(seed)
    polys = [rand_poly(rng, n) for _ in range(n_polys)]
    scal = [rng.randrange(R_MOD) for _ in range(n_polys)]
    sub = [rng.randrange(R_MOD) for _ in range(sub_len)]
    scale = rng.randrange(R_MOD)
    return polys, scal, sub, scale


def _roots(rng, m, kind):
    if kind == "zero":
        return [0] + [rng.randrange(R_MOD) for _ in range(m - 1)]
    if kind == "repeated":
        r = rng.randrange(R_MOD)
        return [r] * m
    return [rng.randrange(R_MOD) for _ in range(m)]


COMBINE_CASES = [(257, 1, 0, 0, "rand"), (257, 2, 1, 1, "rand"), (1000, 3, 3, 2, "zero"), (1000, 4, 1, 3, "repeated"), (4099, 5, 3, 4, "rand"),
                 (1, 1, 1, 1, "rand"), (3, 2, 3, 3, "rand"), (1 << 17, 3, 3, 3, "rand"), (1 << 17, 20, 1, 1, "rand")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_polys,sub_len,n_roots,kind", COMBINE_CASES)
def test_poly_combine_matches_reference(h2, tile, n, n_polys, sub_len, n_roots, kind):
    rng = random.Random(0xC0B + n + 7 * n_polys + 31 * n_roots)
    polys, scal, sub, scale = _combine_case(rng.randrange(1 << 30), n, n_polys, sub_len, n_roots)
    roots = _roots(rng, n_roots, kind)
    a = ou.combine(polys, scal, sub)
    want_q = ou.combine(polys, scal, sub, roots, scale)
    mp, ms, msub, mr, mscale = [ou.to_mont(p) for p in polys], ou.to_mont(scal), ou.to_mont(sub), ou.to_mont(roots), ou.fe(scale)
    lout = n - n_roots
    want = np.zeros((lout + 5, 4), dtype=np.uint64)
    want[:lout] = ou.to_mont(want_q)
    shapes = [(0, 0)] if n > 5000 else TILE_SHAPES
    for r, b in shapes:
        tile(r, b)
        kw = dict(sub=msub, roots=mr, scale=mscale, out_len=lout + 5)
        if n_roots:
            got, rem = h2.poly_combine(mp, ms, remainder=True, **kw)
            assert ou.from_mont([rem])[0] == ou.eval_polynomial(a, roots[0]), (r, b)
        else:
            got = h2.poly_combine(mp, ms, **kw)
        assert np.array_equal(got, want), (r, b)
        # accumulate: out[0 .. lout) += scale q, the tail untouched
        acc0 = np.concatenate([ou.to_mont([7 * i + 1 for i in range(lout)]) if lout else np.zeros((0, 4), np.uint64), ou.to_mont([5] * 5)])
        out = acc0.copy()
        h2.poly_combine(mp, ms, out=out, accumulate=True, **kw)
        exp = ou.to_mont([(7 * i + 1 + c) % R_MOD for i, c in enumerate(want_q)] + [5] * 5) if lout else ou.to_mont([5] * 5)
        assert np.array_equal(out, exp), (r, b)


@pytest.mark.gpu
def test_poly_combine_device_form(h2, tile):
    import torch
    rng = random.Random(0xDE7)
    n = 5000
    polys, scal, sub, scale = _combine_case(1, n, 3, 2, 2)
    roots = _roots(rng, 2, "rand")
    want = ou.to_mont(ou.combine(polys, scal, sub, roots, scale))
    dev = [torch.from_numpy(ou.to_mont(p).view(np.int64).copy()).cuda() for p in polys]
    for r, b in [(0, 0), (1, 4), (4, 64)]:
        tile(r, b)
        d_out = torch.full((n + 3, 4), -1, dtype=torch.int64, device="cuda")
        rem = h2.poly_combine_device(dev, ou.to_mont(scal), d_out, sub=ou.to_mont(sub), roots=ou.to_mont(roots), scale=ou.fe(scale), remainder=True)
        got = h2.to_numpy_u64(d_out)
        assert np.array_equal(got[:n - 2], want) and not got[n - 2:].any()
        assert ou.from_mont([rem])[0] == ou.eval_polynomial(ou.combine(polys, scal, sub), roots[0])


@pytest.mark.gpu
def test_kate_division_large(h2):
    """2^20: the whole quotient; 2^22: the recurrence at sampled rows, the top coefficient, and the remainder against the engine's own
    evaluation and a Python Horner"""
    rng = random.Random(0x1A7)
    n = 1 << 20
    a = rand_poly(rng, n)
    b = rng.randrange(R_MOD)
    assert np.array_equal(h2.kate_division(ou.to_mont(a), ou.fe(b)), ou.to_mont(ou.kate_division(a, b)))
    del a
    n = 1 << 22
    am = rand_mont(0x22, n)
    b = rng.randrange(R_MOD)
    q, rem = h2.poly_combine([am], [ou.fe(1)], roots=[ou.fe(b)], remainder=True)
    assert q.shape == (n - 1, 4)
    assert np.array_equal(q[n - 2], am[n - 1])
    rows = sorted(rng.sample(range(n - 2), 4096))
    A = ou.from_mont(am[[i + 1 for i in rows]])
    Q = ou.from_mont(q[rows])
    Q1 = ou.from_mont(q[[i + 1 for i in rows]])
    for i in range(len(rows)):
        assert Q[i] == (A[i] + b * Q1[i]) % R_MOD
    assert np.array_equal(rem, h2.eval_polynomials([am], [0], [ou.fe(b)])[0])
    acc = 0
    for c in reversed(mont_ints(am)):
        acc = (acc * b + c) % R_MOD
    assert ou.from_mont([rem])[0] == acc * pow(1 << 256, -1, R_MOD) % R_MOD


# ------------------------------------------------------------------ whole openings (GPU)
def _to_engine_sets(sets):
    return [([ou.fe(p) for p in pts], [(j, [ou.fe(e) for e in evs]) for j, evs in cols]) for pts, cols in sets]


def _gwc_groups(sets):
    groups = {}
    order = []
    for pts, cols in sets:
        for t, p in enumerate(pts):
            if p not in groups:
                groups[p] = {}
                order.append(p)
            for j, evs in cols:
                groups[p][j] = evs[t]
    return [(p, sorted(groups[p].items())) for p in order]


def _commit_equal(h2, oracle, bases, mpoly):
    m = mpoly.shape[0]
    got = h2.g1_to_affine(h2.best_multiexp(mpoly, bases[:m]))
    assert np.array_equal(got, oracle.g1_to_affine(oracle.best_multiexp(mpoly, bases[:m], 4)))


def _check_openings(h2, oracle, polys, sets, seed, bases=None):
    rng = random.Random(seed)
    y, v, u = (rng.randrange(R_MOD) for _ in range(3))
    mp = [ou.to_mont(p) for p in polys]
    groups = _gwc_groups(sets)
    want_w = ou.gwc_witnesses(polys, groups, v)
    got_w = h2.gwc_witnesses(mp, [(ou.fe(p), [(j, ou.fe(e)) for j, e in q]) for p, q in groups], ou.fe(v))
    assert len(got_w) == len(want_w)
    for g, w in zip(got_w, want_w):
        assert np.array_equal(g, ou.to_mont(w))
    want_h = ou.shplonk_h(polys, sets, y, v)
    es = _to_engine_sets(sets)
    got_h = h2.shplonk_h(mp, es, ou.fe(y), ou.fe(v))
    assert np.array_equal(got_h, ou.to_mont(want_h))
    want_f = ou.shplonk_final(polys, sets, want_h, y, v, u)
    got_f = h2.shplonk_final(mp, es, got_h, ou.fe(y), ou.fe(v), ou.fe(u))
    assert np.array_equal(got_f, ou.to_mont(want_f))
    if bases is not None:
        for m in (got_w[0], got_h, got_f):
            _commit_equal(h2, oracle, bases, m)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_polys,n_sets", [(4, 4, 3), (10, 6, 4), (12, 7, 5)])
def test_openings_match_reference(h2, oracle, k, n_polys, n_sets):
    rng = random.Random(0x0BE + k)
    polys, sets = synthetic_sets(rng, k, n_polys, n_sets)
    bases = oracle.gen_points(0x0BE5 + k, 1 << k, num_threads=4)
    _check_openings(h2, oracle, polys, sets, 0x0BF + k, bases)


@pytest.mark.gpu
def test_openings_config5_shape(h2, oracle):
    """k = 17 in the bench shape (opening_util.CONFIG5_SETS): 21 polynomials, 26 queries, 4 rotation sets"""
    k = 17
    n = 1 << k
    rng = random.Random(0xC5)
    mp = [rand_mont(0xC500 + j, n) for j in range(ou.CONFIG5_POLYS)]
    polys = [ou.from_mont(m) for m in mp]
    names = ou.config5_points(k, rng.randrange(R_MOD))
    qp, pts = [], []
    for pn, cols in ou.CONFIG5_SETS:
        for j in cols:
            for p in pn:
                qp.append(j), pts.append(names[p])
    evals = ou.from_mont(h2.eval_polynomials(mp, qp, ou.to_mont(pts)))
    ev = {(j, p): e for j, p, e in zip(qp, pts, evals)}
    for q in (0, 20, 25):
        assert evals[q] == ou.eval_polynomial(polys[qp[q]], pts[q])
    sets = [([names[p] for p in pn], [(j, [ev[(j, names[p])] for p in pn]) for j in cols]) for pn, cols in ou.CONFIG5_SETS]
    bases = oracle.gen_points(0xC5B, n, num_threads=4)
    _check_openings(h2, oracle, polys, sets, 0xC51, bases)


# ------------------------------------------------------------------ residency and ordering (GPU)
@pytest.mark.gpu
def test_resident_chain_equals_host_form(h2, oracle):
    """ifft_device -> eval_polynomials_device and poly_combine_device -> msm_device, against the host forms of the same steps"""
    import torch
    k = 12
    n = 1 << k
    rng = random.Random(0x4E5)
    d, _ = oracle.domain_new(4, k)
    lag = [rand_mont(0x4E50 + j, n) for j in range(3)]
    coeff = [oracle.lagrange_to_coeff(d, c.copy(), 4) for c in lag]
    dev = [torch.from_numpy(c.view(np.int64).copy()).cuda() for c in lag]
    for t in dev:
        h2.ifft_device(t, d.fe("omega_inv"), k, d.fe("ifft_divisor"))
    x = ou.fe(rng.randrange(R_MOD))
    qp, pts = [0, 1, 2, 2], [x, x, x, ou.fe(5)]
    evs = h2.eval_polynomials_device(dev, qp, pts)
    assert np.array_equal(evs, h2.eval_polynomials(coeff, qp, pts))
    scal = [ou.fe(rng.randrange(R_MOD)) for _ in range(3)]
    d_out = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
    h2.poly_combine_device(dev, scal, d_out, sub=[evs[0]], roots=[x])
    bases = oracle.gen_points(0x4E5B, n - 1, num_threads=4)
    d_bases = torch.from_numpy(bases.view(np.int64).copy()).cuda()
    got = h2.g1_to_affine(h2.msm_device(d_out, d_bases))
    host_q = h2.poly_combine(coeff, scal, sub=[evs[0]], roots=[x])
    assert np.array_equal(h2.to_numpy_u64(d_out), host_q)
    assert np.array_equal(got, oracle.g1_to_affine(oracle.best_multiexp(host_q, bases, 4)))


@pytest.mark.gpu
def test_side_stream_then_host_call(h2):
    """a device call queued on a side stream, then a host call with no synchronisation in between: both correct"""
    import torch
    rng = random.Random(0x51DE)
    n = 1 << 16
    polys, scal, sub, scale = _combine_case(2, n, 4, 3, 3)
    roots = _roots(rng, 3, "rand")
    want = ou.to_mont(ou.combine(polys, scal, sub, roots, scale))
    mp = [ou.to_mont(p) for p in polys]
    dev = [torch.from_numpy(m.view(np.int64).copy()).cuda() for m in mp]
    d_out = torch.empty((n - 3, 4), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h2.poly_combine_device(dev, ou.to_mont(scal), d_out, sub=ou.to_mont(sub), roots=ou.to_mont(roots), scale=ou.fe(scale))
    host = h2.poly_combine(mp[::-1], ou.to_mont(scal[::-1]), sub=ou.to_mont(sub), roots=ou.to_mont(roots), scale=ou.fe(scale))
    side.synchronize()
    assert np.array_equal(host, want)
    assert np.array_equal(h2.to_numpy_u64(d_out), want)


@pytest.mark.gpu
def test_pinned_key_polynomials(h2):
    rng = random.Random(0x9117)
    n = 1 << 14
    mp = [rand_mont(0x9110 + j, n) for j in range(4)]
    scal = [ou.fe(rng.randrange(R_MOD)) for _ in range(4)]
    r = [ou.fe(rng.randrange(R_MOD))]
    qp, pts = [0, 1, 2, 3, 3], [r[0]] * 4 + [ou.fe(3)]
    want_q = h2.poly_combine(mp, scal, roots=r)
    want_e = h2.eval_polynomials(mp, qp, pts)
    h2.columns_pin(mp[:2])
    try:
        assert np.array_equal(h2.poly_combine(mp, scal, roots=r), want_q)
        assert np.array_equal(h2.eval_polynomials(mp, qp, pts), want_e)
    finally:
        h2.columns_unpin(mp[:2])
    assert ou.from_mont(want_e[:1])[0] == ou.eval_polynomial(ou.from_mont(mp[0]), ou.from_mont(r)[0])


# ------------------------------------------------------------------ the C++ mirror (GPU)
@pytest.mark.gpu
def test_cpp_mirror_openings(tmp_path):
    """tests/cpp/test_opening_mirror restates GWC and SHPLONK over host/halo2hip.hpp; its witnesses against the restatement"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_opening_mirror")
    rng = random.Random(0xCC)
    k = 10
    polys, sets = synthetic_sets(rng, k, 5, 3)
    y, v, u = (rng.randrange(R_MOD) for _ in range(3))
    # input file: k, n_polys, polys, then per set: points, columns and their evaluations; then y, v, u
    words = [k, len(polys)]
    blob = [np.array(words, dtype=np.uint64)]
    for p in polys:
        blob.append(ou.to_mont(p).reshape(-1))
    blob.append(np.array([len(sets)], dtype=np.uint64))
    for pts, cols in sets:
        blob.append(np.array([len(pts), len(cols)], dtype=np.uint64))
        blob.append(ou.to_mont(pts).reshape(-1))
        for j, evs in cols:
            blob.append(np.array([j], dtype=np.uint64))
            blob.append(ou.to_mont(evs).reshape(-1))
    blob.append(ou.to_mont([y, v, u]).reshape(-1))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(blob).astype(np.uint64).tofile(inp)
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=120)
    got = np.fromfile(outp, dtype=np.uint64).reshape(-1, 4)
    groups = _gwc_groups(sets)
    want = [c for w in ou.gwc_witnesses(polys, groups, v) for c in w]
    h = ou.shplonk_h(polys, sets, y, v)
    want += h + ou.shplonk_final(polys, sets, h, y, v, u)
    assert np.array_equal(got, ou.to_mont(want))
