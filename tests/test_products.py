"""The permutation and lookup grand-product columns (h2hip_permutation_products_bn254 / h2hip_lookup_products_bn254) and
ff's BatchInvert (h2hip_batch_invert_bn254_fr): the restatement in product_util.py checked by identities of its own, then the
engine against it limb for limb, and by the same identities where the restatement is too slow."""
import random

import numpy as np
import pytest

import product_util as pu
from product_util import R_MOD


def rand_fe(rng):
    return rng.randrange(R_MOD)


def rand_cols(rng, m, n):
    return [[rand_fe(rng) for _ in range(n)] for _ in range(m)]


def identity_perms(m, n, omega, delta):
    """s_c[i] = delta^c omega^i: the identity permutation"""
    out, d = [], 1
    for _ in range(m):
        col, w = [], d
        for _ in range(n):
            col.append(w)
            w = w * omega % R_MOD
        out.append(col)
        d = d * delta % R_MOD
    return out


def copy_constrained(rng, m, n, u, omega, delta):
    """columns constant on the cycles of a random permutation sigma of the cells (c, i), i < u, and s_c[i] = the identity value
    of sigma(c, i): the permutation argument's product over rows < u is one"""
    ident = identity_perms(m, n, omega, delta)
    cols = rand_cols(rng, m, n)
    perms = [list(c) for c in ident]
    cells = [(c, i) for c in range(m) for i in range(u)]
    sigma = list(range(len(cells)))
    rng.shuffle(sigma)
    seen = [False] * len(cells)
    for start in range(len(cells)):  # one value per cycle
        if seen[start]:
            continue
        v, x = rand_fe(rng), start
        while not seen[x]:
            seen[x] = True
            c, i = cells[x]
            cols[c][i] = v
            x = sigma[x]
    for x, y in enumerate(sigma):
        c, i = cells[x]
        c2, i2 = cells[y]
        perms[c][i] = ident[c2][i2]
    return cols, perms


# ------------------------------------------------------------------ the restatement checks itself (CPU)
def test_restated_batch_invert_keeps_zeros():
    a, b = 12345, R_MOD - 7
    assert pu.ff_batch_invert([0, a, 0, b]) == [0, pow(a, -1, R_MOD), 0, pow(b, -1, R_MOD)]
    assert pu.ff_batch_invert([]) == []


@pytest.mark.parametrize("chunk_len", [1, 2, 3])
def test_restated_permutation_product_ends_at_one(chunk_len):
    rng = random.Random(0x9E3 + chunk_len)
    k, b, m = 5, 3, 5
    n = 1 << k
    u = n - b - 1
    omega, delta = pu.root_of_unity(k), 7
    beta, gamma = rand_fe(rng), rand_fe(rng)
    cols, perms = copy_constrained(rng, m, n, u, omega, delta)
    n_sets = -(-m // chunk_len)
    blind = [[rand_fe(rng) for _ in range(b)] for _ in range(n_sets)]
    zs = pu.permutation_commit(k, omega, delta, beta, gamma, cols, perms, chunk_len, blind, b)
    assert len(zs) == n_sets and zs[0][0] == 1
    for t in range(1, n_sets):
        assert zs[t][0] == zs[t - 1][u]
    assert zs[-1][u] == 1
    # one broken copy: the last set no longer ends at one
    c, i = 0, rng.randrange(u)
    cols[c][i] = (cols[c][i] + 1) % R_MOD
    zs = pu.permutation_commit(k, omega, delta, beta, gamma, cols, perms, chunk_len, blind, b)
    assert zs[-1][u] != 1


def test_restated_lookup_product_ends_at_one():
    rng = random.Random(0x10C)
    k, b = 5, 3
    n = 1 << k
    u = n - b - 1
    a, s = rand_cols(rng, 2, n)
    order_a, order_s = list(range(u)), list(range(u))
    rng.shuffle(order_a)
    rng.shuffle(order_s)
    ap = [a[j] for j in order_a] + a[u:]
    sp = [s[j] for j in order_s] + s[u:]
    beta, gamma = rand_fe(rng), rand_fe(rng)
    blind = [rand_fe(rng) for _ in range(b)]
    z = pu.lookup_commit(k, beta, gamma, a, s, ap, sp, blind, b)
    assert z[0] == 1 and z[u] == 1 and z[u + 1:] == blind
    ap[0], ap[1] = ap[1], (ap[1] + 1) % R_MOD
    assert pu.lookup_commit(k, beta, gamma, a, s, ap, sp, blind, b)[u] != 1


def test_products_without_gpu_fail_loudly(h2):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    k, n = 3, 8
    col = np.zeros((n, 4), dtype=np.uint64)
    one = pu.fe(1)
    with pytest.raises(h2.H2HipError):
        h2.permutation_products(k, pu.fe(pu.root_of_unity(k)), one, one, one, [col], [col], 1, np.zeros((3, 4), np.uint64), 3)
    with pytest.raises(h2.H2HipError):
        h2.lookup_products(k, one, one, [col], [col], [col], [col], np.zeros((3, 4), np.uint64), 3)
    with pytest.raises(h2.H2HipError):
        h2.batch_invert(pu.to_mont([1, 2]))


def test_products_reject_bad_arguments(h2):
    """validation happens before any device work, so it answers the same with or without a GPU"""
    k, n = 3, 8
    col = np.zeros((n, 4), dtype=np.uint64)
    one = pu.fe(1)
    bad = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    w = pu.fe(pu.root_of_unity(k))
    bl = np.zeros((3, 4), np.uint64)
    for args in [(k, w, one, one, one, [col], [col], 0, None, 3),          # chunk_len == 0
                 (k, w, one, bad, one, [col], [col], 1, bl, 3),            # beta not reduced
                 (k, w, one, one, one, [col], [col], 1, np.zeros((7, 4), np.uint64), 7)]:  # b + 1 >= n
        with pytest.raises(h2.H2HipError, match="rc=1"):
            h2.permutation_products(*args)
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.lookup_products(k, one, bad, [col], [col], [col], [col], bl, 3)


# ------------------------------------------------------------------ the engine against the restatement (GPU)
def _perm_case(seed, k, m, chunk_len, b, zero_row=None):
    rng = random.Random(seed)
    n = 1 << k
    omega, delta = pu.root_of_unity(k), rand_fe(rng)
    beta, gamma = rand_fe(rng), rand_fe(rng)
    cols, perms = rand_cols(rng, m, n), rand_cols(rng, m, n)
    if zero_row is not None:  # p_c[i] = -(beta s_c[i] + gamma): a zero denominator
        c = m - 1
        cols[c][zero_row] = (-(beta * perms[c][zero_row] + gamma)) % R_MOD
    n_sets = -(-m // chunk_len)
    blind = [[rand_fe(rng) for _ in range(b)] for _ in range(n_sets)]
    want = pu.permutation_commit(k, omega, delta, beta, gamma, cols, perms, chunk_len, blind, b)
    args = dict(k=k, omega=pu.fe(omega), delta=pu.fe(delta), beta=pu.fe(beta), gamma=pu.fe(gamma),
                columns=[pu.to_mont(c) for c in cols], permutations=[pu.to_mont(s) for s in perms], chunk_len=chunk_len,
                blinding=pu.to_mont([v for bl in blind for v in bl]), blinding_factors=b)
    return args, [pu.to_mont(z) for z in want], want


def _perm_device(h2, args):
    import torch
    dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()
    dc = [dev(c) for c in args["columns"]]
    dp = [dev(s) for s in args["permutations"]]
    n_sets = -(-len(dc) // args["chunk_len"])
    dz = [torch.empty_like(dc[0]) for _ in range(n_sets)]
    h2.permutation_products_device(args["k"], args["omega"], args["delta"], args["beta"], args["gamma"], dc, dp, args["chunk_len"],
                                   args["blinding"], args["blinding_factors"], dz)
    torch.cuda.synchronize()
    return [h2.to_numpy_u64(z) for z in dz]


PERM_CASES = [(3, 1, 1, 3), (3, 5, 2, 3), (4, 9, 3, 5), (4, 6, 5, 3), (10, 7, 5, 3), (10, 4, 1, 5), (12, 9, 3, 5), (12, 8, 3, 3),
              (17, 9, 3, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,chunk_len,b", PERM_CASES)
def test_permutation_products_match_reference(h2, k, m, chunk_len, b):
    args, want, _ = _perm_case(0xA000 + 97 * k + 13 * m + chunk_len, k, m, chunk_len, b)
    got = h2.permutation_products(**args)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    for g, w in zip(_perm_device(h2, args), want):
        assert np.array_equal(g, w)
    # the key's columns pinned: only the witness columns are uploaded, the result is the same
    h2.columns_pin(args["permutations"])
    try:
        for g, w in zip(h2.permutation_products(**args), want):
            assert np.array_equal(g, w)
    finally:
        h2.columns_unpin(args["permutations"])


def _lookup_case(seed, k, count, b, zero_row=None):
    rng = random.Random(seed)
    n = 1 << k
    beta, gamma = rand_fe(rng), rand_fe(rng)
    A, S, AP, SP, BL, want = [], [], [], [], [], []
    for j in range(count):
        a, s, ap, sp = rand_cols(rng, 4, n)
        if zero_row is not None and j == count - 1:
            ap[zero_row] = (R_MOD - beta) % R_MOD
        bl = [rand_fe(rng) for _ in range(b)]
        want.append(pu.lookup_commit(k, beta, gamma, a, s, ap, sp, bl, b))
        A.append(a), S.append(s), AP.append(ap), SP.append(sp), BL.extend(bl)
    m = lambda cols: [pu.to_mont(c) for c in cols]
    args = dict(k=k, beta=pu.fe(beta), gamma=pu.fe(gamma), compressed_inputs=m(A), compressed_tables=m(S), permuted_inputs=m(AP),
                permuted_tables=m(SP), blinding=pu.to_mont(BL), blinding_factors=b)
    return args, [pu.to_mont(z) for z in want], want


def _lookup_device(h2, args):
    import torch
    dev = lambda cols: [torch.from_numpy(a.view(np.int64).copy()).cuda() for a in cols]
    d = [dev(args[f]) for f in ("compressed_inputs", "compressed_tables", "permuted_inputs", "permuted_tables")]
    dz = [torch.empty_like(c) for c in d[0]]
    h2.lookup_products_device(args["k"], args["beta"], args["gamma"], *d, args["blinding"], args["blinding_factors"], dz)
    torch.cuda.synchronize()
    return [h2.to_numpy_u64(z) for z in dz]


@pytest.mark.gpu
@pytest.mark.parametrize("k,count,b", [(3, 1, 3), (4, 2, 5), (10, 3, 3), (12, 4, 5), (17, 2, 5)])
def test_lookup_products_match_reference(h2, k, count, b):
    args, want, _ = _lookup_case(0xB000 + 31 * k + count, k, count, b)
    for g, w in zip(h2.lookup_products(**args), want):
        assert np.array_equal(g, w)
    for g, w in zip(_lookup_device(h2, args), want):
        assert np.array_equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("k,zero_row", [(4, 0), (4, 6), (10, 517), (12, 4000)])
def test_zero_denominator_zeroes_the_rest(h2, k, zero_row):
    args, want, ints = _perm_case(0xC000 + k + zero_row, k, 5, 2, 3, zero_row=zero_row)
    u = (1 << k) - 3 - 1
    assert all(v == 0 for v in ints[-1][zero_row + 1:u + 1]) and ints[-1][zero_row] != 0  # what the restatement says
    for g, w in zip(h2.permutation_products(**args), want):
        assert np.array_equal(g, w)
    for g, w in zip(_perm_device(h2, args), want):
        assert np.array_equal(g, w)
    largs, lwant, lints = _lookup_case(0xC100 + k + zero_row, k, 2, 3, zero_row=zero_row)
    assert all(v == 0 for v in lints[-1][zero_row + 1:u + 1])
    for g, w in zip(h2.lookup_products(**largs), lwant):
        assert np.array_equal(g, w)
    for g, w in zip(_lookup_device(h2, largs), lwant):
        assert np.array_equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, (1 << 16) + 3, 1 << 20])
def test_batch_invert_matches_pow(h2, n):
    import torch
    rng = np.random.default_rng(n)
    limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] %= np.uint64(0x30644e72e131a029)  # canonical: below r
    special = [pu.fe(0), pu.fe(1), pu.fe(R_MOD - 1)]
    for j, v in enumerate(special):
        if n > j * 97:
            limbs[(j * 97) % n] = v
    if n > 300:
        limbs[n - 1] = pu.fe(0)
    vals = pu.from_mont(limbs)
    want = pu.to_mont([pow(v, -1, R_MOD) if v else 0 for v in vals])
    assert np.array_equal(h2.batch_invert(limbs), want)
    d = torch.from_numpy(limbs.view(np.int64).copy()).cuda()
    h2.batch_invert_device(d)
    torch.cuda.synchronize()
    assert np.array_equal(h2.to_numpy_u64(d), want)


# ------------------------------------------------------------------ large k: identities the restatement is too slow for
def _rand_mont(rng, n):
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(0x30644e72e131a029)
    return a


def _sampled_rows(rng, u, count):
    return sorted(set(int(x) for x in rng.integers(0, u - 1, size=count)) | {0, u - 2})


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, 22])
def test_large_k_products_hold_the_identities(h2, k):
    import torch
    n, b, m, chunk_len = 1 << k, 5, 9, 3
    u = n - b - 1
    rng = np.random.default_rng(k)
    omega, delta = pu.root_of_unity(k), 0x1234567 + k
    beta, gamma = 0xBE7A + k, 0x6A33A + k
    # identity values delta^c omega^i from the engine's own NTT: the transform of delta^c e_1 is delta^c omega^i
    ident = []
    for c in range(m):
        e = np.zeros((n, 4), dtype=np.uint64)
        e[1] = pu.fe(pow(delta, c, R_MOD))
        h2.best_fft(e, pu.fe(omega), k)
        ident.append(e)
    # copy constraints: 4096 disjoint pairs of cells (rows < u) swap their identity values and share one column value
    cols = [_rand_mont(rng, n) for _ in range(m)]
    perms = [e.copy() for e in ident]
    cells = rng.choice(m * u, size=8192, replace=False)
    for x, y in zip(cells[0::2], cells[1::2]):
        (c1, i1), (c2, i2) = divmod(int(x), u), divmod(int(y), u)
        perms[c1][i1], perms[c2][i2] = ident[c2][i2], ident[c1][i1]
        cols[c2][i2] = cols[c1][i1]
    blind = _rand_mont(rng, 3 * b)
    dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()
    dz = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(3)]
    h2.permutation_products_device(k, pu.fe(omega), pu.fe(delta), pu.fe(beta), pu.fe(gamma), [dev(c) for c in cols], [dev(s) for s in perms],
                                   chunk_len, blind, b, dz)
    torch.cuda.synchronize()
    zs = [h2.to_numpy_u64(z) for z in dz]
    if k == 20:  # the host form gives the same columns
        for g, w in zip(h2.permutation_products(k, pu.fe(omega), pu.fe(delta), pu.fe(beta), pu.fe(gamma), cols, perms, chunk_len, blind, b), zs):
            assert np.array_equal(g, w)
    assert pu.from_mont(zs[0][0])[0] == 1
    assert pu.from_mont(zs[-1][u])[0] == 1
    assert np.array_equal(zs[0][n - b:], blind[:b]) and np.array_equal(zs[2][n - b:], blind[2 * b:])
    rows = _sampled_rows(rng, u, 4096)
    for t in range(3):
        if t:
            assert np.array_equal(zs[t][0], zs[t - 1][u])  # the chain: z_t[0] = z_{t-1}[u]
        z = pu.from_mont(zs[t][rows]), pu.from_mont(zs[t][[i + 1 for i in rows]])
        p = [pu.from_mont(cols[c][rows]) for c in range(t * 3, t * 3 + 3)]
        s = [pu.from_mont(perms[c][rows]) for c in range(t * 3, t * 3 + 3)]
        idv = [pu.from_mont(ident[c][rows]) for c in range(t * 3, t * 3 + 3)]
        for j in range(len(rows)):
            num = den = 1
            for c in range(3):
                num = num * (p[c][j] + beta * idv[c][j] + gamma) % R_MOD
                den = den * (p[c][j] + beta * s[c][j] + gamma) % R_MOD
            assert z[1][j] * den % R_MOD == z[0][j] * num % R_MOD
    # lookups: A', S' a permutation of A, S over the rows < u
    A, S = _rand_mont(rng, n), _rand_mont(rng, n)
    pa, ps = rng.permutation(u), rng.permutation(u)
    AP, SP = A.copy(), S.copy()
    AP[:u], SP[:u] = A[pa], S[ps]
    lz = [torch.empty((n, 4), dtype=torch.int64, device="cuda")]
    h2.lookup_products_device(k, pu.fe(beta), pu.fe(gamma), [dev(A)], [dev(S)], [dev(AP)], [dev(SP)], blind[:b], b, lz)
    torch.cuda.synchronize()
    z = h2.to_numpy_u64(lz[0])
    assert pu.from_mont(z[0])[0] == 1 and pu.from_mont(z[u])[0] == 1
    z0, z1 = pu.from_mont(z[rows]), pu.from_mont(z[[i + 1 for i in rows]])
    a, s_, ap, sp = (pu.from_mont(x[rows]) for x in (A, S, AP, SP))
    for j in range(len(rows)):
        num = (a[j] + beta) * (s_[j] + gamma) % R_MOD
        den = (ap[j] + beta) * (sp[j] + gamma) % R_MOD
        assert z1[j] * den % R_MOD == z0[j] * num % R_MOD


# ------------------------------------------------------------------ the resident chain and stream ordering
@pytest.mark.gpu
def test_device_z_feeds_the_resident_chain(h2):
    import torch
    k, ext = 10, 12
    args, want, _ = _perm_case(0xD000, k, 6, 3, 5)
    dom = h2.EvaluationDomain.new(4, k)
    dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()
    dc, dp = [dev(c) for c in args["columns"]], [dev(s) for s in args["permutations"]]
    dz = [torch.zeros((1 << ext, 4), dtype=torch.int64, device="cuda") for _ in range(2)]
    h2.permutation_products_device(k, args["omega"], args["delta"], args["beta"], args["gamma"], dc, dp, 3, args["blinding"], 5, dz)
    bases = h2.gen_points_device(0xD001, 1 << k)
    for t in range(2):
        torch.cuda.synchronize()
        z_host = h2.to_numpy_u64(dz[t])[:1 << k].copy()
        assert np.array_equal(z_host, want[t])
        got_commit = h2.g1_to_affine(h2.msm_device(dz[t], bases, 1 << k))
        assert np.array_equal(got_commit, h2.g1_to_affine(h2.best_multiexp(z_host, h2.to_numpy_u64(bases))))
        h2.ifft_device(dz[t], dom.omega_inv, k, dom.ifft_divisor)
        torch.cuda.synchronize()
        coeff = dom.lagrange_to_coeff(z_host)
        assert np.array_equal(h2.to_numpy_u64(dz[t])[:1 << k], coeff)
        h2.coeff_to_extended_device(dz[t], k, dom.extended_k, dom.extended_omega, dom.g_coset, dom.g_coset_inv)
        torch.cuda.synchronize()
        assert np.array_equal(h2.to_numpy_u64(dz[t]), dom.coeff_to_extended(coeff))


@pytest.mark.gpu
def test_device_call_on_a_side_stream_then_host_call(h2):
    import torch
    args, want, _ = _perm_case(0xE000, 12, 9, 3, 5)
    largs, lwant, _ = _lookup_case(0xE001, 12, 2, 5)
    dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()
    dc, dp = [dev(c) for c in args["columns"]], [dev(s) for s in args["permutations"]]
    dz = [torch.empty_like(dc[0]) for _ in range(3)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h2.permutation_products_device(12, args["omega"], args["delta"], args["beta"], args["gamma"], dc, dp, 3, args["blinding"], 5, dz)
    got_l = h2.lookup_products(**largs)  # host form on the engine's stream, no synchronisation in between
    side.synchronize()
    for g, w in zip(got_l, lwant):
        assert np.array_equal(g, w)
    for g, w in zip(dz, want):
        assert np.array_equal(h2.to_numpy_u64(g), w)
