"""Every host-pointer form of the stage files against its own _device form, bit for bit, at the smallest shapes where the staging's
slot arithmetic can go wrong: k = 3 (256-byte columns), counts of 1 and 3, an empty optional list, one host array passed as two
inputs; and at k = 10 with one of several key columns pinned (h2hip_columns_pin) and the rest uploaded.  What the forms compute is
the other test files' business; here the device form is the reference."""
import numpy as np
import pytest

import evalh_util as ev
import product_util as pu

pytestmark = pytest.mark.gpu
K_SMALL, K_PIN, BF = 3, 10, 2


def fes(rng, n):
    """n reduced Fr elements as (n, 4) uint64: the top limb below 2^60 keeps every value under the modulus"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(4)
    return a


def cols_of(rng, m, n):
    return [fes(rng, n) for _ in range(m)]


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32 if a.dtype == np.uint32 else np.uint8).copy()).cuda()


def devs(arrays):
    return [dev(a) for a in arrays]


def empty_like_cols(h2, count, n):
    import torch
    return [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(count)]


def same(h2, host, device):
    import torch
    torch.cuda.synchronize()
    assert len(host) == len(device)
    for j, (a, d) in enumerate(zip(host, device)):
        assert np.array_equal(np.asarray(a).view(np.uint8).reshape(-1), h2.to_numpy_u64(d).view(np.uint8).reshape(-1)), "output %d" % j


class pinned:
    """pin `cols` for the block"""

    def __init__(self, h2, cols):
        self.h2, self.cols = h2, list(cols)

    def __enter__(self):
        self.h2.columns_pin(self.cols)

    def __exit__(self, *exc):
        self.h2.columns_unpin(self.cols)


def shapes():
    """(k, count, index of the one pinned key column or None)"""
    return [(K_SMALL, 1, None), (K_SMALL, 3, None), (K_PIN, 3, 1)]


def in_table(rng, tab, u):
    """an input column whose rows all hold values of the table's rows below u"""
    return tab[rng.integers(0, u, size=tab.shape[0])].copy()


# ------------------------------------------------------------------ product.hip
@pytest.mark.parametrize("k,m,pin", shapes())
def test_permutation_products(h2, k, m, pin):
    rng, n = np.random.default_rng(0x1000 + k + m), 1 << k
    cols, perms = cols_of(rng, m, n), cols_of(rng, m, n)
    if m > 1:
        cols[2] = cols[0]  # one host array as two inputs
    omega, consts = pu.fe(pu.root_of_unity(k)), [fes(rng, 1)[0] for _ in range(3)]
    n_sets = -(-m // 2)
    bl = fes(rng, n_sets * BF)
    with pinned(h2, [perms[pin]] if pin is not None else []):
        z = h2.permutation_products(k, omega, *consts, cols, perms, 2, bl, BF)
    dz = empty_like_cols(h2, n_sets, n)
    h2.permutation_products_device(k, omega, *consts, devs(cols), devs(perms), 2, bl, BF, dz)
    same(h2, z, dz)


@pytest.mark.parametrize("count", [1, 3])
def test_lookup_and_shuffle_products(h2, count):
    k = K_SMALL
    rng, n = np.random.default_rng(0x1100 + count), 1 << k
    a, s, ap, sp = (cols_of(rng, count, n) for _ in range(4))
    sp[0] = a[0]  # one host array as two inputs
    beta, gamma = fes(rng, 2)
    bl = fes(rng, count * BF)
    z = h2.lookup_products(k, beta, gamma, a, s, ap, sp, bl, BF)
    dz = empty_like_cols(h2, count, n)
    h2.lookup_products_device(k, beta, gamma, devs(a), devs(s), devs(ap), devs(sp), bl, BF, dz)
    same(h2, z, dz)
    z = h2.shuffle_products(k, gamma, a, s, bl, BF)
    h2.shuffle_products_device(k, gamma, devs(a), devs(s), bl, BF, dz)
    same(h2, z, dz)


@pytest.mark.parametrize("n_inputs", [[1], [1, 3, 2]])
def test_mvlookup_multiplicities_and_sums(h2, n_inputs):
    k = K_SMALL
    rng, n, count = np.random.default_rng(0x1200 + len(n_inputs)), 1 << k, len(n_inputs)
    u = n - BF - 1
    tabs = cols_of(rng, count, n)
    ins = [[in_table(rng, tabs[j], u) for _ in range(c)] for j, c in enumerate(n_inputs)]
    if count > 1:
        ins[1][2] = ins[1][0]  # one host array as two inputs
    m = h2.mvlookup_multiplicities(k, ins, tabs, BF)
    dm = empty_like_cols(h2, count, n)
    h2.mvlookup_multiplicities_device(k, [devs(c) for c in ins], devs(tabs), BF, dm)
    same(h2, m, dm)
    beta, bl = fes(rng, 1)[0], fes(rng, count * BF)
    phi = h2.mvlookup_sums(k, beta, ins, tabs, m, bl, BF)
    dphi = empty_like_cols(h2, count, n)
    h2.mvlookup_sums_device(k, beta, [devs(c) for c in ins], devs(tabs), dm, bl, BF, dphi)
    same(h2, phi, dphi)


@pytest.mark.parametrize("n", [1, 8, 1000])
def test_batch_invert(h2, n):
    a = fes(np.random.default_rng(0x1300 + n), n)
    a[n // 2] = 0
    d = dev(a)
    h2.batch_invert_device(d)
    same(h2, [h2.batch_invert(a)], [d])


# ------------------------------------------------------------------ lookup.hip
def compress_graphs(with_fixed):
    if with_fixed:
        lookups = [([("advice", 0, 0), ("fixed", 1, 1)], [("fixed", 0, 0), ("fixed", 2, -1)]), ([("instance", 0, 0)], [("fixed", 1, 0)])]
    else:
        lookups = [([("advice", 0, 0), ("advice", 1, 1)], [("advice", 1, 0), ("prod", ("advice", 0, -1), ("const", 7))])]
    return [ev.flatten_graph(g) for inp, tab in lookups for g in ev.lookup_compress_graphs(inp, tab)]


@pytest.mark.parametrize("k,n_fixed,pin", [(K_SMALL, 0, None), (K_SMALL, 3, None), (K_PIN, 3, 1)])
def test_lookup_compress(h2, k, n_fixed, pin):
    rng, n = np.random.default_rng(0x2000 + k + n_fixed), 1 << k
    fixed, advice, instance = cols_of(rng, n_fixed, n), cols_of(rng, 2, n), cols_of(rng, 1 if n_fixed else 0, n)
    graphs, theta = compress_graphs(n_fixed > 0), fes(rng, 1)[0]
    with pinned(h2, [fixed[pin]] if pin is not None else []):
        out = h2.lookup_compress(k, graphs, theta, fixed, advice, instance)
    dout = empty_like_cols(h2, len(graphs), n)
    h2.lookup_compress_device(k, graphs, theta, dout, devs(fixed), devs(advice), devs(instance))
    same(h2, out, dout)


@pytest.mark.parametrize("count", [1, 3])
def test_lookup_permute(h2, count):
    k = K_SMALL
    rng, n = np.random.default_rng(0x2100 + count), 1 << k
    u = n - BF - 1
    tabs = cols_of(rng, count, n)
    ins = [in_table(rng, t, u) for t in tabs]
    ins[0] = tabs[0]  # one host array as two inputs
    bl = fes(rng, count * 2 * (BF + 1))
    pa, pt = h2.lookup_permute(k, ins, tabs, bl, BF)
    dpa, dpt = empty_like_cols(h2, count, n), empty_like_cols(h2, count, n)
    h2.lookup_permute_device(k, devs(ins), devs(tabs), bl, BF, dpa, dpt)
    same(h2, pa + pt, dpa + dpt)


# ------------------------------------------------------------------ check.hip
def same_check(host, device):
    for h, d in zip(host, device):
        assert np.array_equal(h, d)


@pytest.mark.parametrize("k,n_fixed,pin", [(K_SMALL, 0, None), (K_SMALL, 3, None), (K_PIN, 3, 1)])
def test_check_gates(h2, k, n_fixed, pin):
    rng, n = np.random.default_rng(0x3000 + k + n_fixed), 1 << k
    fixed, advice = cols_of(rng, n_fixed, n), cols_of(rng, 2, n)
    advice[1][: n // 2] = advice[0][: n // 2]  # half the rows satisfy the first gate
    polys = [("sum", ("advice", 0, 0), ("neg", ("advice", 1, 0)))]
    if n_fixed:
        polys.append(("prod", ("fixed", 1, 0), ("sum", ("advice", 0, 1), ("fixed", 2, -1))))
    graphs = [ev.flatten_graph(g) for g in ev.gate_check_graphs(polys)]
    with pinned(h2, [fixed[pin]] if pin is not None else []):
        host = h2.check_gates(k, graphs, fixed, advice)
    same_check(host, h2.check_gates_device(k, graphs, devs(fixed), devs(advice)))


def a_mapping(rng, m, n):
    """the identity with the cells of a few rows rotated among the columns"""
    mp = np.zeros((m, n, 2), dtype=np.uint32)
    mp[:, :, 0] = np.arange(m)[:, None]
    mp[:, :, 1] = np.arange(n)[None, :]
    for r in rng.integers(0, n, size=3):
        mp[:, r, 0] = (np.arange(m) + 1) % m
    return mp


@pytest.mark.parametrize("k,m,pin", shapes())
def test_check_permutation(h2, k, m, pin):
    rng, n = np.random.default_rng(0x3100 + k + m), 1 << k
    cols, mp = cols_of(rng, m, n), a_mapping(np.random.default_rng(7), m, n)
    if m > 1:
        cols[2] = cols[0]  # one host array as two inputs
    with pinned(h2, [cols[pin]] if pin is not None else []):
        host = h2.check_permutation(k, cols, mp)
    same_check(host, h2.check_permutation_device(k, devs(cols), [dev(mp[j]) for j in range(m)]))


@pytest.mark.parametrize("k,count,pin", shapes())
def test_check_lookups_and_shuffles(h2, k, count, pin):
    rng, n = np.random.default_rng(0x3200 + k + count), 1 << k
    tabs = cols_of(rng, count, n)
    ins = [in_table(rng, t, n - BF - 1) for t in tabs]
    ins[0][1] = fes(rng, 1)[0]  # a value its table lacks
    with pinned(h2, [tabs[pin]] if pin is not None else []):
        host = h2.check_lookups(k, ins, tabs, BF)
        host_sh = h2.check_shuffles(k, ins, tabs, BF)
    same_check(host, h2.check_lookups_device(k, devs(ins), devs(tabs), BF))
    same_check(host_sh, h2.check_shuffles_device(k, devs(ins), devs(tabs), BF))


# ------------------------------------------------------------------ opening.hip
@pytest.mark.parametrize("lens,query,pin", [([8], [0], None), ([8, 4, 0, 8], [3, 0, 3], None),  # the second polynomial is never queried
                                             ([1 << K_PIN] * 3, [0, 1, 2, 1], 1)])
def test_eval_polynomials(h2, lens, query, pin):
    rng = np.random.default_rng(0x4000 + len(lens))
    polys = [fes(rng, ln) for ln in lens]
    points = fes(rng, len(query))
    with pinned(h2, [polys[pin]] if pin is not None else []):
        host = h2.eval_polynomials(polys, query, points)
    d_polys = [dev(p) if len(p) else dev(np.zeros((1, 4), dtype=np.uint64)) for p in polys]
    assert np.array_equal(host, h2.eval_polynomials_device(d_polys, query, points, lens=lens))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("k,m,pin", shapes())
def test_poly_combine(h2, k, m, pin, accumulate):
    rng, n = np.random.default_rng(0x4100 + k + m), 1 << k
    polys, scalars, roots, sub = cols_of(rng, m, n), fes(rng, m), fes(rng, 2), fes(rng, 1)
    out0 = fes(rng, n)  # longer than len - n_roots: the tail is zeroed, or kept when accumulating
    out = out0.copy()
    with pinned(h2, [polys[pin]] if pin is not None else []):
        h2.poly_combine(polys, scalars, sub=sub, roots=roots, out=out, accumulate=accumulate)
    d_out = dev(out0)
    h2.poly_combine_device(devs(polys), scalars, d_out, sub=sub, roots=roots, accumulate=accumulate)
    same(h2, [out], [d_out])


# ------------------------------------------------------------------ copies.hip, keygen.hip
@pytest.mark.parametrize("k,m,n_copies", [(K_SMALL, 1, 0), (K_SMALL, 3, 5), (2, 3, 4)])
def test_permutation_mapping(h2, k, m, n_copies):
    import torch
    rng, n = np.random.default_rng(0x5000 + k + m), 1 << k
    copies = np.stack([rng.integers(0, m, n_copies), rng.integers(0, n, n_copies), rng.integers(0, m, n_copies), rng.integers(0, n, n_copies)],
                      axis=1).astype(np.uint32).reshape(-1, 4)
    host = h2.permutation_mapping(k, m, copies)
    d_map = [torch.empty((n, 2), dtype=torch.int32, device="cuda") for _ in range(m)]
    h2.permutation_mapping_device(k, m, dev(copies) if n_copies else None, d_map, n_copies)
    same(h2, [host[j] for j in range(m)], d_map)


@pytest.mark.parametrize("m,group_bytes", [(1, 0), (3, 0), (3, 1)])
def test_batch_invert_assigned(h2, m, group_bytes):
    k = K_SMALL
    rng, n = np.random.default_rng(0x5100 + m), 1 << k
    nums = cols_of(rng, m, n)
    rows = [np.sort(rng.choice(n, size=c, replace=False)).astype(np.uint32) for c in ([3, 0, n][:m])]
    dens = [fes(rng, len(r)) for r in rows]
    h2.set_keygen_group(group_bytes)  # 1: one column per group
    try:
        host = h2.batch_invert_assigned(k, nums, rows, dens)
    finally:
        h2.set_keygen_group(0)
    d_out = empty_like_cols(h2, m, n)
    opt = lambda arrays: [dev(a) if len(a) else None for a in arrays]  # noqa: E731
    h2.batch_invert_assigned_device(k, devs(nums), opt(rows), [len(r) for r in rows], opt(dens), d_out)
    same(h2, host, d_out)


def test_key_lagrange_columns_and_permutation_keygen(h2):
    import torch
    dom = h2.EvaluationDomain.new(4, K_SMALL)
    host = h2.key_lagrange_columns(dom, BF)
    d = empty_like_cols(h2, 3, dom.extended_len())
    h2.key_lagrange_columns_device(dom, BF, *d)
    same(h2, host, d)
    m, n = 3, 1 << K_SMALL
    mp = a_mapping(np.random.default_rng(9), m, n)
    h2.set_keygen_group(1)  # one column per group: the two-buffer pipeline over the staging buffer
    try:
        host = h2.permutation_keygen(dom, mp)
    finally:
        h2.set_keygen_group(0)
    d_out = [empty_like_cols(h2, m, n), empty_like_cols(h2, m, n), empty_like_cols(h2, m, dom.extended_len())]
    h2.permutation_keygen_device(dom, [dev(mp[j]) for j in range(m)], *d_out)
    same(h2, host["permutations"] + host["polys"] + host["cosets"], d_out[0] + d_out[1] + d_out[2])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ serde.hip, random.hip
@pytest.mark.parametrize("n", [1, 9, 200])
def test_serde(h2, n):
    import torch
    rng = np.random.default_rng(0x6000 + n)
    points = h2.to_numpy_u64(h2.gen_points_device(0x6001, n)).reshape(n, 8)
    enc = h2.g1_to_bytes(points)
    d_enc = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    h2.g1_to_bytes_device(dev(points), d_enc, n)
    same(h2, [enc], [d_enc])
    d_points = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    h2.g1_from_bytes_device(d_enc, d_points, n)
    same(h2, [h2.g1_from_bytes(enc)], [d_points])
    h2.g1_validate(points)
    h2.g1_validate_device(d_points, n)
    a = fes(rng, n)
    repr_ = h2.fr_to_repr(a)
    d_repr = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    h2.fr_to_repr_device(dev(a), d_repr, n)
    same(h2, [repr_], [d_repr])
    d_back = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    h2.fr_from_repr_device(d_repr, d_back, n)
    same(h2, [h2.fr_from_repr(repr_)], [d_back])
    bad = enc.copy()
    bad[n // 2] = 0xFF  # x >= q: the fallible form reports it and still writes every output
    with pytest.raises(h2.H2HipEncodingError) as host_err:
        h2.g1_from_bytes(bad)
    with pytest.raises(h2.H2HipEncodingError) as dev_err:
        h2.g1_from_bytes_device(dev(bad), d_points, n)
    assert (host_err.value.count, host_err.value.index) == (dev_err.value.count, dev_err.value.index) == (1, n // 2)
    same(h2, [host_err.value.output], [d_points])


def test_random(h2):
    import torch
    n = 515  # from the host forms' threshold (2^9) on they run on the device
    seed = bytes(range(32))
    same(h2, [h2.fr_random(seed, n, first_block=3, stream_id=5)], [h2.fr_random_device(seed, n, first_block=3, stream_id=5)])
    wide = np.random.default_rng(0x7000).integers(0, 256, size=(n, 64), dtype=np.uint8)
    d_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    h2.fr_from_bytes_wide_device(dev(wide), d_out, n)
    same(h2, [h2.fr_from_bytes_wide(wide)], [d_out])
