"""Key generation columns on the GPU (csrc/keygen.hip): h2hip_permutation_keygen_bn254, h2hip_batch_invert_assigned_bn254 and
h2hip_key_lagrange_columns_bn254, their device forms, the Python composition keygen_columns and the C++ mirror, limb for limb against the
Python restatement of tests/keygen_util.py, which is first checked on its own."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import keygen_util as ku
from keygen_util import R_MOD

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ mappings
def flat_to_mapping(flat, m, n):
    """flat[j * n + i] = index of the cell (j, i) maps to -> (m, n, 2) uint32"""
    flat = np.asarray(flat, dtype=np.int64).reshape(m, n)
    return np.stack([flat // n, flat % n], axis=-1).astype(np.uint32)


def random_copies(seed, asm_list, m, n, count, rows=None):
    rng = random.Random(seed)
    rows = n if rows is None else rows
    seq = [(rng.randrange(m), rng.randrange(rows), rng.randrange(m), rng.randrange(rows)) for _ in range(count)]
    for a in asm_list:
        for c in seq:
            a.copy(*c)
    return seq


def make_mapping(h2, shape, m, n, seed=1):
    rng = np.random.default_rng(seed)
    cells = m * n
    if shape == "identity":
        return flat_to_mapping(np.arange(cells), m, n)
    if shape == "one_cycle":
        return flat_to_mapping((np.arange(cells) + 1) % cells, m, n)
    if shape == "random":
        return flat_to_mapping(rng.permutation(cells), m, n)
    if shape == "copies":
        a = h2.PermutationAssembly(n, m)
        random_copies(seed, [a], m, n, min(cells, 20000))
        return a.mapping.copy()
    if shape == "to_one":  # every cell of column j points at one cell: rows 0 and n - 1, columns 0 and m - 1 (the table edges)
        mp = np.zeros((m, n, 2), dtype=np.uint32)
        for j in range(m):
            mp[j, :, 0] = (m - 1) if j % 2 == 0 else 0
            mp[j, :, 1] = (n - 1) if j % 4 < 2 else 0
        return mp
    if shape == "edges":  # rows 0, n - 1 and those next to the split of any two-level scheme, in column m - 1 and 0
        mp = np.zeros((m, n, 2), dtype=np.uint32)
        k = n.bit_length() - 1
        picks = sorted({0, n - 1, 1 % n, (1 << (k // 2)) % n, ((1 << (k // 2)) - 1) % n, (1 << ((k + 1) // 2)) % n, ((1 << ((k + 1) // 2)) - 1) % n, n // 2})
        mp[:, :, 1] = np.array(picks, dtype=np.uint32)[np.arange(n) % len(picks)][None, :]
        mp[:, :, 0] = np.where(np.arange(n) % 2 == 0, m - 1, 0)[None, :]
        return mp
    if shape == "mixed":  # a different shape per column
        kinds = ["identity", "random", "copies", "to_one", "edges", "one_cycle"]
        full = {s: make_mapping(h2, s, m, n, seed + 7) for s in kinds}
        return np.stack([full[kinds[j % len(kinds)]][j] for j in range(m)])
    raise ValueError(shape)


SHAPES = ["identity", "one_cycle", "random", "copies", "to_one", "edges"]


# ------------------------------------------------------------------ the restatement checks itself (CPU)
COPIES_KNOWN = [(0, 0, 1, 1), (0, 2, 0, 0), (1, 3, 1, 1), (1, 1, 0, 2), (0, 3, 1, 0), (1, 0, 0, 0)]
MAPPING_KNOWN = [[(0, 3), (0, 1), (1, 1), (1, 0)], [(0, 2), (1, 3), (1, 2), (0, 0)]]


def test_known_answer_of_copy_restatement_and_package(h2):
    """worked out by hand from permutation/keygen.rs:48-103: one cycle of six cells, (0, 1) and (1, 2) alone.  The fourth copy joins two
    cells the first three have already put into one cycle and changes nothing (:79-81), and so does the last one when it is made a second
    time; the swap is at the cells named in the call, not at the cycle representatives (:98-100)."""
    a, p = ku.Assembly(4, 2), h2.PermutationAssembly(4, 2)
    for t, c in enumerate(COPIES_KNOWN):
        before = [list(col) for col in a.mapping]
        a.copy(*c)
        p.copy(*c)
        assert (a.mapping == before) == (t == 3), "copy %d" % t
    assert a.mapping == MAPPING_KNOWN
    assert p.mapping.tolist() == [[list(c) for c in col] for col in MAPPING_KNOWN]
    assert a.sizes[0][0] == 6 and int(p.sizes[0, 0]) == 6
    a.copy(*COPIES_KNOWN[-1])
    p.copy(*COPIES_KNOWN[-1])
    assert a.mapping == MAPPING_KNOWN and a.sizes[0][0] == 6
    assert p.mapping.tolist() == [[list(c) for c in col] for col in MAPPING_KNOWN] and int(p.sizes[0, 0]) == 6
    assert sorted(ku.orbit(a.mapping, (0, 0))) == [(0, 0), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3)]
    assert ku.orbit(a.mapping, (0, 1)) == [(0, 1)] and ku.orbit(a.mapping, (1, 2)) == [(1, 2)]


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_copy_keeps_cycles_and_package_equals_restatement(h2, k):
    n, m = 1 << k, 3 + k % 3
    a, p = ku.Assembly(n, m), h2.PermutationAssembly(n, m)
    seq = random_copies(0xC0 + k, [a, p], m, n, 3000)
    assert p.mapping.tolist() == [[list(c) for c in col] for col in a.mapping]  # merging is order-sensitive: identical, not equivalent
    assert p.mapping.shape == (m, n, 2) and p.mapping.dtype == np.uint32
    seen = set()
    for j in range(m):
        for i in range(n):
            if (j, i) in seen:
                continue
            orb = ku.orbit(a.mapping, (j, i))
            seen.update(orb)
            rep = a.aux[j][i]
            assert all(a.aux[c][r] == rep for c, r in orb)
            assert a.sizes[rep[0]][rep[1]] == len(orb)
    lc, lr, rc, rr = seq[0]
    before = [list(col) for col in a.mapping]
    a.copy(lc, lr, rc, rr)  # already in one cycle
    assert a.mapping == before
    with pytest.raises(ku.BoundsFailure):
        a.copy(0, n, 0, 0)
    with pytest.raises(ValueError):
        p.copy(0, n, 0, 0)
    with pytest.raises(ValueError):
        p.copy(m, 0, 0, 0)


def test_restated_sigma_and_columns(oracle):
    k, b, m = 5, 3, 3
    n = 1 << k
    omega = ku.root_of_unity(k)
    ident = ku.sigma(flat_to_mapping(np.arange(m * n), m, n), omega)
    for c in range(m):
        assert ident[c] == [pow(ku.DELTA, c, R_MOD) * pow(omega, r, R_MOD) % R_MOD for r in range(n)]
    mp = flat_to_mapping(np.random.default_rng(5).permutation(m * n), m, n)
    s = ku.sigma(mp, omega)
    assert sorted(v for col in s for v in col) == sorted(v for col in ident for v in col)
    for a, b_ in zip(ku.sigma_mont(mp, omega), s):
        assert np.array_equal(a, ku.to_mont(b_))
    assert ku.from_mont(ku.to_mont(s[1])) == s[1]
    # l0 evaluated back on the domain is e_0; l_active_row + l_last + l_blind = 1
    d, _ = oracle.domain_new(4, k)
    l0, l_blind, l_last = ku.unit_columns(k, b)
    assert sum(l_blind) == b and l_last.index(1) == n - b - 1
    coeff = oracle.lagrange_to_coeff(d, ku.to_mont(l0), 2)
    c = ku.from_mont(coeff)
    assert [sum(c[t] * pow(omega, i * t, R_MOD) for t in range(n)) % R_MOD for i in range(n)] == l0
    ext = [ku.from_mont(oracle.coeff_to_extended(d, oracle.lagrange_to_coeff(d, ku.to_mont(col), 2), 2)) for col in (l_blind, l_last)]
    active = [(1 - (x + y)) % R_MOD for x, y in zip(ext[1], ext[0])]
    assert all((a + x + y) % R_MOD == 1 for a, x, y in zip(active, ext[0], ext[1]))


def test_restated_batch_invert_assigned():
    nums = [[3, 0, 5, 7]]
    got = ku.batch_invert_assigned(nums, [[0, 2, 3]], [[2, 0, 1]])
    assert got == [[3 * pow(2, -1, R_MOD) % R_MOD, 0, 0, 7]]


def _domain(h2, k, j=4):
    return h2.EvaluationDomain.new(j, k)


def test_keygen_calls_reject_bad_arguments(h2):
    """validation happens before any device work, so it answers the same with or without a GPU"""
    L = h2.lib()
    k, n = 3, 8
    dom = _domain(h2, k)
    mp = flat_to_mapping(np.arange(2 * n), 2, n)
    for cell, pair in (((1, 3), (2, 0)), ((0, 7), (0, n)), ((0, 0), (0xFFFFFFFF, 0))):  # column >= n_columns, row >= 2^k
        bad = mp.copy()
        bad[cell] = pair
        with pytest.raises(h2.H2HipError, match=r"rc=1.*mapping\[%d\]\[%d\]" % cell):
            h2.permutation_keygen(dom, bad)
    unreduced = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.permutation_keygen(dom, mp, delta=unreduced)
    big = h2.EvaluationDomain(29, 29, 3, **{f: getattr(dom, f) for f in dom.FIELDS})
    fe_args = [h2._p(getattr(dom, f)) for f in ("omega", "omega_inv", "ifft_divisor")]
    ext_args = [h2._p(getattr(dom, f)) for f in ("extended_omega", "g_coset", "g_coset_inv")]
    delta = h2.fr_from_int(h2.FR_DELTA)
    rows = (ctypes.c_void_p * 2)(mp[0].ctypes.data, mp[1].ctypes.data)
    call = lambda kk, ek, mapping, m, a, b, c: L.h2hip_permutation_keygen_bn254(ctypes.c_uint32(kk), *fe_args, ctypes.c_uint32(ek), *ext_args,  # noqa: E731
                                                                               h2._p(delta), mapping, ctypes.c_uint32(m), a, b, c)
    assert big.k == 29
    assert call(29, 29, rows, 2, None, None, None) == 1  # k > 28
    assert "28" in L.h2hip_last_error().decode()
    assert call(3, 2, rows, 2, None, None, None) == 1  # extended_k < k
    assert call(3, 5, None, 2, None, None, None) == 1  # null mapping with columns
    assert "null" in L.h2hip_last_error().decode()
    out = (ctypes.c_void_p * 2)(None, None)
    assert call(3, 5, rows, 2, out, None, None) == 1  # a table with a null column
    assert call(3, 5, None, 0, None, None, None) == 0  # n_columns == 0 writes nothing
    dcall = L.h2hip_permutation_keygen_bn254_device  # the device form checks what is host memory
    assert dcall(ctypes.c_uint32(29), *fe_args, ctypes.c_uint32(29), *ext_args, h2._p(delta), rows, ctypes.c_uint32(2), None, None, None, None) == 1
    assert dcall(ctypes.c_uint32(3), *fe_args, ctypes.c_uint32(5), *ext_args, h2._p(delta), None, ctypes.c_uint32(2), None, None, None, None) == 1
    assert dcall(ctypes.c_uint32(3), *fe_args, ctypes.c_uint32(5), *ext_args, h2._p(unreduced), rows, ctypes.c_uint32(2), None, None, None, None) == 1
    # batch_invert_assigned
    col = np.zeros((n, 4), dtype=np.uint64)
    one = ku.to_mont([1, 1])
    with pytest.raises(h2.H2HipError, match="rc=1.*ascending"):
        h2.batch_invert_assigned(k, [col], [[3, 2]], [one])  # unsorted
    with pytest.raises(h2.H2HipError, match="rc=1.*ascending"):
        h2.batch_invert_assigned(k, [col], [[2, 2]], [one])  # repeated
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.batch_invert_assigned(k, [col], [[2, n]], [one])  # row >= 2^k
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.batch_invert_assigned(k, [col], [[2]], [unreduced.reshape(1, 4)])
    cp = (ctypes.c_void_p * 1)(col.ctypes.data)
    cnt = (ctypes.c_size_t * 1)(2)
    f = L.h2hip_batch_invert_assigned_bn254
    assert f(ctypes.c_uint32(29), cp, None, None, None, ctypes.c_size_t(1), cp) == 1  # k > 28
    assert f(ctypes.c_uint32(3), cp, None, cnt, None, ctypes.c_size_t(1), cp) == 1  # a count without arrays
    assert f(ctypes.c_uint32(3), None, None, None, None, ctypes.c_size_t(1), cp) == 1
    assert f(ctypes.c_uint32(3), None, None, None, None, ctypes.c_size_t(0), None) == 0
    fd = L.h2hip_batch_invert_assigned_bn254_device
    assert fd(ctypes.c_uint32(29), cp, None, None, None, ctypes.c_size_t(1), cp, None) == 1
    assert fd(ctypes.c_uint32(3), cp, None, cnt, None, ctypes.c_size_t(1), cp, None) == 1
    # key_lagrange_columns
    for b in (n - 1, n, 0xFFFFFFFF):
        with pytest.raises(h2.H2HipError, match=r"rc=1.*blinding_factors"):
            h2.key_lagrange_columns(dom, b)
    with pytest.raises(h2.H2HipError, match="rc=1"):
        h2.key_lagrange_columns(big, 1)
    lcall = L.h2hip_key_lagrange_columns_bn254_device
    largs = [h2._p(dom.omega_inv), h2._p(dom.ifft_divisor), ctypes.c_uint32(5)] + ext_args
    assert lcall(ctypes.c_uint32(3), *largs, ctypes.c_uint32(7), cp, cp, cp, None) == 1
    assert lcall(ctypes.c_uint32(3), *largs, ctypes.c_uint32(1), None, cp, cp, None) == 1


_NO_GPU_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from conftest import load_pkg
h2 = load_pkg()
dom = h2.EvaluationDomain.new(4, 3)
mp = np.zeros((1, 8, 2), dtype=np.uint32)
mp[0, :, 1] = np.arange(8)
col = np.zeros((8, 4), dtype=np.uint64)
calls = [lambda: h2.permutation_keygen(dom, mp), lambda: h2.batch_invert_assigned(3, [col]), lambda: h2.key_lagrange_columns(dom, 2)]
for i, f in enumerate(calls):
    try:
        f()
    except h2.H2HipError as e:
        assert "rc=2" in str(e), str(e)
    else:
        raise SystemExit("call %d succeeded without a GPU" % i)
print("loud")
"""


def test_keygen_calls_without_gpu_fail_loudly(tmp_path):
    """every valid call raises H2HipError (H2HIP_EDEVICE) when no device is visible: a fresh process with the GPUs hidden, so the test
    says the same on a machine with and without one"""
    script = tmp_path / "no_gpu.py"
    script.write_text(_NO_GPU_SCRIPT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("HALO2_HIP_DEVICES", None)
    r = subprocess.run([sys.executable, str(script), HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "loud" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ the engine against the restatement (GPU)
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _dev_map(mp):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(mp[j]).view(np.int32).copy()).cuda() for j in range(mp.shape[0])]


def _empty(rows):
    import torch
    return torch.empty((rows, 4), dtype=torch.int64, device="cuda")


def assert_cols(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s, column %d" % (what, j)


SIGMA_CASES = [(k, m, s) for k in (3, 4, 10) for m in (1, 2, 9, 13) for s in SHAPES]
SIGMA_CASES += [(12, m, "mixed") for m in (1, 2, 9, 13)] + [(12, 9, s) for s in ("random", "copies")]
SIGMA_CASES += [(17, 2, "mixed"), (17, 13, "mixed"), (17, 9, "copies")]
SIGMA_CASES += [(20, 1, "copies"), (20, 2, "random"), (20, 9, "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,shape", SIGMA_CASES)
def test_permutations_match_restatement(h2, k, m, shape):
    n = 1 << k
    mp = make_mapping(h2, shape, m, n, seed=k * 100 + m)
    got = h2.permutation_keygen(_domain(h2, k), mp, want=("permutations",))
    assert set(got) == {"permutations"}
    assert_cols(got["permutations"], ku.sigma_mont(mp, ku.root_of_unity(k)), "permutations %s" % shape)


def oracle_forms(oracle, j, k, sig):
    d, _ = oracle.domain_new(j, k)
    polys = [oracle.lagrange_to_coeff(d, c, 4) for c in sig]
    return polys, [oracle.coeff_to_extended(d, p, 4) for p in polys]


SUBSETS = [("permutations",), ("polys",), ("cosets",), ("permutations", "polys"), ("permutations", "cosets"), ("polys", "cosets"),
           ("permutations", "polys", "cosets")]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,j", [(3, 2, 3), (4, 9, 4), (10, 13, 6), (12, 9, 4), (17, 2, 4), (17, 9, 3)])
def test_polys_and_cosets_match_oracle(h2, oracle, k, m, j):
    n = 1 << k
    mp = make_mapping(h2, "mixed", m, n, seed=k + m)
    sig = ku.sigma_mont(mp, ku.root_of_unity(k))
    polys, cosets = oracle_forms(oracle, j, k, sig)
    dom = _domain(h2, k, j)
    got = h2.permutation_keygen(dom, mp)
    assert_cols(got["permutations"], sig, "permutations")
    assert_cols(got["polys"], polys, "polys")
    assert_cols(got["cosets"], cosets, "cosets")


@pytest.mark.gpu
@pytest.mark.parametrize("want", SUBSETS)
@pytest.mark.parametrize("k", [4, 11])
def test_each_output_alone_and_in_pairs_host_and_device(h2, oracle, k, want):
    import torch
    m, j, n = 5, 4, 1 << k
    mp = make_mapping(h2, "mixed", m, n, seed=k)
    sig = ku.sigma_mont(mp, ku.root_of_unity(k))
    polys, cosets = oracle_forms(oracle, j, k, sig)
    ref = {"permutations": sig, "polys": polys, "cosets": cosets}
    dom = _domain(h2, k, j)
    got = h2.permutation_keygen(dom, mp, want=want)
    assert set(got) == set(want)
    for w in want:
        assert_cols(got[w], ref[w], "host " + w)
    dmap = _dev_map(mp)
    bufs = {w: [_empty(n if w != "cosets" else dom.extended_len()) for _ in range(m)] for w in want}
    h2.permutation_keygen_device(dom, dmap, bufs.get("permutations"), bufs.get("polys"), bufs.get("cosets"))
    torch.cuda.synchronize()
    for w in want:
        assert_cols([h2.to_numpy_u64(t) for t in bufs[w]], ref[w], "device " + w)
    assert all(np.array_equal(t.cpu().numpy().view(np.uint32).reshape(n, 2), mp[jj]) for jj, t in enumerate(dmap)), "the mapping is an input"


@pytest.mark.gpu
def test_k20_two_columns_against_oracle(h2, oracle):
    k, m, j = 20, 2, 4
    n = 1 << k
    mp = make_mapping(h2, "copies", m, n, seed=20)
    sig = ku.sigma_mont(mp, ku.root_of_unity(k))
    polys, cosets = oracle_forms(oracle, j, k, sig)
    got = h2.permutation_keygen(_domain(h2, k, j), mp)
    assert_cols(got["permutations"], sig, "permutations")
    assert_cols(got["polys"], polys, "polys")
    assert_cols(got["cosets"], cosets, "cosets")


@pytest.mark.gpu
def test_k22_sigma_exact_and_transforms_by_identity(h2):
    k, m, j = 22, 2, 3
    n = 1 << k
    mp = make_mapping(h2, "random", m, n, seed=22)
    dom = _domain(h2, k, j)
    got = h2.permutation_keygen(dom, mp)
    assert_cols(got["permutations"], ku.sigma_mont(mp, ku.root_of_unity(k)), "permutations")
    assert_cols(got["cosets"], dom.coeff_to_extended_batch(got["polys"]), "cosets = coeff_to_extended(polys)")
    omega = ku.root_of_unity(k)
    rows = [0, 1, 2, n - 1, n // 2, (1 << 11) - 1, 1 << 11] + [int(x) for x in np.random.default_rng(3).integers(0, n, 57)]
    pts = ku.to_mont([pow(omega, i, R_MOD) for i in rows])
    for c in range(m):
        ev = h2.eval_polynomials([got["polys"][c]], [0] * len(rows), pts)
        assert np.array_equal(ev, got["permutations"][c][rows]), "polys[%d] on the domain" % c


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 12])
def test_column_groups_change_nothing(h2, oracle, k):
    """a host call cut into many pipelined groups gives the same limbs; batch_invert_assigned's groups too"""
    m, j, n = 7, 4, 1 << k
    mp = make_mapping(h2, "mixed", m, n, seed=77 + k)
    sig = ku.sigma_mont(mp, ku.root_of_unity(k))
    polys, cosets = oracle_forms(oracle, j, k, sig)
    dom = _domain(h2, k, j)
    nums, rows, dens = assigned_case(0x6A + k, k, ["one_percent", "none", "all", "ends", "none", "one_percent"])
    want = [ku.to_mont(c) for c in ku.batch_invert_assigned(nums, rows, dens)]
    try:
        per_col = n * (8 + 32 + 32 + 4 * 32)
        for cols_per_group in (1, 2, 3):
            h2.set_keygen_group(cols_per_group * per_col)
            got = h2.permutation_keygen(dom, mp)
            assert_cols(got["permutations"], sig, "grouped permutations")
            assert_cols(got["polys"], polys, "grouped polys")
            assert_cols(got["cosets"], cosets, "grouped cosets")
            assert_cols(h2.permutation_keygen(dom, mp, want=("cosets",))["cosets"], cosets, "grouped cosets alone")
        for cols_per_group in (1, 3):
            h2.set_keygen_group(cols_per_group * n * 32)
            got = h2.batch_invert_assigned(k, [ku.to_mont(c) for c in nums], [np.array(r, dtype=np.uint32) if r else None for r in rows],
                                           [ku.to_mont(d) if d else None for d in dens])
            assert_cols(got, want, "grouped batch_invert_assigned")
    finally:
        h2.set_keygen_group()


@pytest.mark.gpu
def test_device_form_flags_a_pair_out_of_range(h2):
    import torch
    k, m = 10, 3
    n = 1 << k
    dom = _domain(h2, k)
    mp = make_mapping(h2, "random", m, n)
    for cell, pair in (((2, 17), (m, 0)), ((0, n - 1), (0, n))):
        bad = mp.copy()
        bad[cell] = pair
        out = [_empty(n) for _ in range(m)]
        with pytest.raises(h2.H2HipError, match="rc=1.*mapping pair"):
            h2.permutation_keygen_device(dom, _dev_map(bad), out)
        torch.cuda.synchronize()
        want = ku.sigma_mont(mp, ku.root_of_unity(k))
        want[cell[0]][cell[1]] = 0
        assert_cols([h2.to_numpy_u64(t) for t in out], want, "the other cells are complete, the bad one is zero")
    out = [_empty(n) for _ in range(m)]
    h2.permutation_keygen_device(dom, _dev_map(mp), out)  # the flag does not stick
    assert_cols([h2.to_numpy_u64(t) for t in out], ku.sigma_mont(mp, ku.root_of_unity(k)), "after a flagged call")


@pytest.mark.gpu
def test_device_call_on_a_side_stream_then_host_call(h2, oracle):
    import torch
    k, m, j = 12, 4, 4
    n = 1 << k
    dom = _domain(h2, k, j)
    mp, mp2 = make_mapping(h2, "random", m, n, seed=1), make_mapping(h2, "copies", 2, n, seed=2)
    sig, sig2 = ku.sigma_mont(mp, ku.root_of_unity(k)), ku.sigma_mont(mp2, ku.root_of_unity(k))
    polys, cosets = oracle_forms(oracle, j, k, sig)
    polys2, cosets2 = oracle_forms(oracle, j, k, sig2)
    dmap = _dev_map(mp)
    dp, dq, dc = [_empty(n) for _ in range(m)], [_empty(n) for _ in range(m)], [_empty(dom.extended_len()) for _ in range(m)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h2.permutation_keygen_device(dom, dmap, dp, dq, dc)
    got2 = h2.permutation_keygen(dom, mp2)  # host form on the engine's stream, at once
    side.synchronize()
    assert_cols(got2["permutations"], sig2, "host permutations")
    assert_cols(got2["polys"], polys2, "host polys")
    assert_cols(got2["cosets"], cosets2, "host cosets")
    assert_cols([h2.to_numpy_u64(t) for t in dp], sig, "device permutations")
    assert_cols([h2.to_numpy_u64(t) for t in dq], polys, "device polys")
    assert_cols([h2.to_numpy_u64(t) for t in dc], cosets, "device cosets")


# ------------------------------------------------------------------ batch_invert_assigned
def assigned_case(seed, k, kinds):
    """per column: (numerators, rows, denominators) as integers"""
    rng = random.Random(seed)
    n = 1 << k
    nums, rows, dens = [], [], []
    for kind in kinds:
        col = [rng.randrange(R_MOD) for _ in range(n)]
        if kind == "none":
            r = []
        elif kind == "all":
            r = list(range(n))
        elif kind == "one_percent":
            r = sorted(rng.sample(range(n), max(1, n // 100)))
        elif kind == "ends":
            r = sorted({0, n - 1})
        else:
            raise ValueError(kind)
        d = [rng.randrange(1, R_MOD) for _ in r]
        for t in range(0, len(r), 5):  # zero denominators, a zero numerator over a non-zero denominator, denominator one
            what = (t // 5) % 4
            if what == 0:
                d[t] = 0
            elif what == 1:
                col[r[t]] = 0
            elif what == 2:
                d[t] = 1
        nums.append(col)
        rows.append(r)
        dens.append(d)
    return nums, rows, dens


ASSIGNED_CASES = [(3, ["none", "all", "ends"]), (4, ["all"]), (7, ["one_percent", "none", "all", "ends"]), (10, ["none"]), (12, ["all", "one_percent"]),
                  (17, ["one_percent", "all", "none"]), (20, ["one_percent", "ends"])]


@pytest.mark.gpu
@pytest.mark.parametrize("k,kinds", ASSIGNED_CASES)
def test_batch_invert_assigned_matches_restatement_and_dense_path(h2, k, kinds):
    import torch
    n = 1 << k
    nums, rows, dens = assigned_case(0xA5 + k, k, kinds)
    want = [ku.to_mont(c) for c in ku.batch_invert_assigned(nums, rows, dens)]
    mn = [ku.to_mont(c) for c in nums]
    md = [ku.to_mont(d) if d else None for d in dens]
    mr = [np.array(r, dtype=np.uint32) if r else None for r in rows]
    assert_cols(h2.batch_invert_assigned(k, mn, mr, md), want, "host")
    # the dense path: numerators * BatchInvert(denominators with ones)
    for j in range(len(kinds)):
        dense = [1] * n
        for r, d in zip(rows[j], dens[j]):
            dense[r] = d
        inv = ku.from_mont(h2.batch_invert(ku.to_mont(dense)))
        assert_cols([ku.to_mont([a * b % R_MOD for a, b in zip(nums[j], inv)])], [want[j]], "dense path, column %d" % j)
    inplace = [c.copy() for c in mn]
    res = h2.batch_invert_assigned(k, inplace, mr, md, in_place=True)
    assert all(a is b for a, b in zip(res, inplace))
    assert_cols(inplace, want, "host, out == numerators")
    # device form: out of place, then aliased
    dn = [_dev(c) for c in mn]
    dr = [None if r is None else torch.from_numpy(r.view(np.int32).copy()).cuda() for r in mr]
    dd = [None if d is None else _dev(d) for d in md]
    out = [_empty(n) for _ in kinds]
    counts = [len(r) for r in rows]
    h2.batch_invert_assigned_device(k, dn, dr, counts, dd, out)
    torch.cuda.synchronize()
    assert_cols([h2.to_numpy_u64(t) for t in out], want, "device")
    assert_cols([h2.to_numpy_u64(t) for t in dn], mn, "device: the numerators are inputs")
    h2.batch_invert_assigned_device(k, dn, dr, counts, dd, dn)
    torch.cuda.synchronize()
    assert_cols([h2.to_numpy_u64(t) for t in dn], want, "device, out == numerators")


# ------------------------------------------------------------------ l0, l_last, l_active_row
def oracle_l_columns(oracle, j, k, b):
    """the oracle's transforms of the unit columns.  l_active_row = 1 - (l_last + l_blind) is formed element by element up to k = 12; beyond
    that (the element-wise oracle call is a Python loop) as the transform of the column that is one on the rows < u: the transforms are
    linear, the all-ones column extends to all ones, and a reduced element has one representation, so the limbs are the same -- the
    small sizes check exactly that."""
    d, _ = oracle.domain_new(j, k)
    ext = lambda col: oracle.coeff_to_extended(d, oracle.lagrange_to_coeff(d, ku.to_mont(col), 4), 4)  # noqa: E731
    l0_col, l_blind_col, l_last_col = ku.unit_columns(k, b)
    l0, l_last = ext(l0_col), ext(l_last_col)
    linear = ext([1 - x - y for x, y in zip(l_last_col, l_blind_col)])
    if k > 12:
        return l0, l_last, linear
    one = ku.to_mont([1] * l0.shape[0])
    active = oracle.fe_binop("sub", oracle.FR, one, oracle.fe_binop("add", oracle.FR, l_last, ext(l_blind_col)))
    assert np.array_equal(active, linear)
    return l0, l_last, active


L_CASES = [(k, j, b) for k in (3, 4, 9, 12) for j in (3, 4, 6) for b in ("0", "5", "n-2")] + [(17, 3, "5"), (17, 4, "n-2"), (17, 6, "0"), (20, 4, "5")]


@pytest.mark.gpu
@pytest.mark.parametrize("k,j,b", L_CASES)
def test_key_lagrange_columns_match_oracle(h2, oracle, k, j, b):
    import torch
    n = 1 << k
    b = {"0": 0, "5": min(5, n - 2), "n-2": n - 2}[b]
    dom = _domain(h2, k, j)
    assert dom.extended_k - k == {3: 1, 4: 2, 6: 3}[j]
    want = oracle_l_columns(oracle, j, k, b)
    got = h2.key_lagrange_columns(dom, b)
    for name, g, w in zip(("l0", "l_last", "l_active_row"), got, want):
        assert np.array_equal(g, w), name
    if k <= 17:
        bufs = [_empty(dom.extended_len()) for _ in range(3)]
        h2.key_lagrange_columns_device(dom, b, *bufs)
        torch.cuda.synchronize()
        for name, t, w in zip(("l0", "l_last", "l_active_row"), bufs, want):
            assert np.array_equal(h2.to_numpy_u64(t), w), "device " + name


# ------------------------------------------------------------------ the composition
@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 12])
def test_keygen_columns_commitments_match_oracle(h2, oracle, k):
    n, m, b, j = 1 << k, 4, 5, 4
    params = h2.ParamsKZG.setup(k, 0x1234567 + k)
    dom = _domain(h2, k, j)
    nums, rows, dens = assigned_case(0xF1 + k, k, ["one_percent", "none", "all"])
    fixed = [(ku.to_mont(c), np.array(r, dtype=np.uint32), ku.to_mont(d) if d else None) for c, r, d in zip(nums, rows, dens)]
    mp = make_mapping(h2, "copies", m, n, seed=k)
    key = h2.keygen_columns(params, dom, fixed, mp, b)
    g_lagrange = oracle.g_to_lagrange(params.g, k, num_threads=4)
    assert np.array_equal(params.g_lagrange, g_lagrange)
    fixed_values = [ku.to_mont(c) for c in ku.batch_invert_assigned(nums, rows, dens)]
    sig = ku.sigma_mont(mp, ku.root_of_unity(k))
    assert_cols(key["fixed_values"], fixed_values, "fixed_values")
    assert_cols(key["permutations"], sig, "permutations")
    for cols, coms, what in ((fixed_values, key["fixed_commitments"], "fixed"), (sig, key["permutation_commitments"], "permutation")):
        assert len(coms) == len(cols)
        for c, (col, com) in enumerate(zip(cols, coms)):
            assert np.array_equal(h2.g1_to_affine(com), oracle.g1_to_affine(oracle.best_multiexp(col, g_lagrange, 4))), "%s commitment %d" % (what, c)
    fp, fc = oracle_forms(oracle, j, k, fixed_values)
    pp, pc = oracle_forms(oracle, j, k, sig)
    assert_cols(key["fixed_polys"], fp, "fixed_polys")
    assert_cols(key["fixed_cosets"], fc, "fixed_cosets")
    assert_cols(key["perm_polys"], pp, "perm_polys")
    assert_cols(key["perm_cosets"], pc, "perm_cosets")
    for name, w in zip(("l0", "l_last", "l_active_row"), oracle_l_columns(oracle, j, k, b)):
        assert np.array_equal(key[name], w), name
    params.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 17])
def test_the_key_closes_the_permutation_argument(h2, k):
    """copies among rows < u, advice constant on the cycles, the key built on the GPU: the grand product ends at one, z[u] = 1 in the
    last set; one broken copy and it does not"""
    n, m, b = 1 << k, 5, 5
    u = n - b - 1
    rng = random.Random(0xC105E + k)
    asm = h2.PermutationAssembly(n, m)
    random_copies(k, [asm], m, n, n // 2, rows=u)
    mp = asm.mapping
    aux = asm.aux.astype(np.int64)
    rep = aux[:, :, 0] * n + aux[:, :, 1]  # the cycle representative of every cell
    uniq, inv = np.unique(rep, return_inverse=True)
    vals = [rng.randrange(R_MOD) for _ in range(len(uniq))]
    inv = inv.reshape(m, n)
    cols_int = [[vals[t] for t in inv[c].tolist()] for c in range(m)]
    dom = _domain(h2, k)
    perms = h2.permutation_keygen(dom, mp, want=("permutations",))["permutations"]
    omega = ku.root_of_unity(k)
    beta, gamma = rng.randrange(R_MOD), rng.randrange(R_MOD)
    one = ku.fe(1)
    joined = np.argwhere((mp[:, :, 0] != np.arange(m)[:, None]) | (mp[:, :, 1] != np.arange(n)[None, :]))
    assert len(joined) > n // 4
    for chunk_len in (1, 3, m):
        n_sets = -(-m // chunk_len)
        blind = ku.to_mont([rng.randrange(R_MOD) for _ in range(n_sets * b)])
        cols = [ku.to_mont(c) for c in cols_int]
        z = h2.permutation_products(k, ku.fe(omega), ku.fe(ku.DELTA), ku.fe(beta), ku.fe(gamma), cols, perms, chunk_len, blind, b)
        assert len(z) == n_sets and np.array_equal(z[0][0], one)
        assert np.array_equal(z[-1][u], one), "chunk_len %d: the product does not close" % chunk_len
        c, i = (int(x) for x in joined[rng.randrange(len(joined))])
        cols[c][i] = ku.fe((cols_int[c][i] + 1) % R_MOD)
        z = h2.permutation_products(k, ku.fe(omega), ku.fe(ku.DELTA), ku.fe(beta), ku.fe(gamma), cols, perms, chunk_len, blind, b)
        assert not np.array_equal(z[-1][u], one), "chunk_len %d: a broken copy went unnoticed" % chunk_len


# ------------------------------------------------------------------ the C++ mirror (GPU)
@pytest.mark.gpu
def test_cpp_mirror_keygen(tmp_path, oracle):
    """tests/cpp/test_keygen_mirror builds a key through host/halo2hip.hpp; its columns against the restatement and the oracle"""
    exe = os.path.join(HERE, "cpp", "test_keygen_mirror")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "halo2-pse_amd"), "../tests/cpp/test_keygen_mirror"])
    k, j, b, m = 10, 4, 5, 3
    n = 1 << k
    asm = ku.Assembly(n, m)
    seq = random_copies(0xCE, [asm], m, n, 700)
    kinds = ["one_percent", "all"]
    nums, rows, dens = assigned_case(0xCF, k, kinds)
    words = [k, j, b, m, len(kinds), len(seq)] + [x for c in seq for x in c]
    blob = [np.array(words, dtype=np.uint64)]
    for col, r, d in zip(nums, rows, dens):
        cells = np.zeros((n, 9), dtype=np.uint64)
        cells[:, 0] = 1
        cells[:, 1:5] = ku.to_mont(col)
        cells[:, 5:9] = ku.fe(1)
        cells[r, 0] = 2
        cells[r, 5:9] = ku.to_mont(d)
        cells[17, 0], cells[17, 1:5] = 0, 0  # one Zero cell
        col[17] = 0
        blob.append(cells.reshape(-1))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(blob).tofile(inp)
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=300)
    raw = np.fromfile(outp, dtype=np.uint64)
    mapping = raw[:m * n].view(np.uint32).reshape(m, n, 2)
    assert np.array_equal(mapping, asm.mapping_array())
    d, _ = oracle.domain_new(j, k)
    ext = 1 << d.extended_k
    at = [m * n]

    def take(count, rows_):
        out = raw[at[0]:at[0] + count * rows_ * 4].reshape(count, rows_, 4)
        at[0] += count * rows_ * 4
        return list(out)

    fixed_values = [ku.to_mont(c) for c in ku.batch_invert_assigned(nums, rows, dens)]
    sig = ku.sigma_mont(mapping, ku.root_of_unity(k))
    fp, fc = oracle_forms(oracle, j, k, fixed_values)
    pp, pc = oracle_forms(oracle, j, k, sig)
    nf = len(kinds)
    for what, count, rows_, want in (("fixed_values", nf, n, fixed_values), ("fixed_polys", nf, n, fp), ("fixed_cosets", nf, ext, fc),
                                     ("permutations", m, n, sig), ("polys", m, n, pp), ("cosets", m, ext, pc)):
        assert_cols(take(count, rows_), want, what)
    for name, w in zip(("l0", "l_last", "l_active_row"), oracle_l_columns(oracle, j, k, b)):
        assert np.array_equal(take(1, ext)[0], w), name
    coms = raw[at[0]:].reshape(m, 8)
    g = oracle.kzg_setup(k, ku.fe(0x5eed0007))[1]
    for c in range(m):
        assert np.array_equal(coms[c], oracle.g1_to_affine(oracle.best_multiexp(sig[c], g, 4))), "build_vk commitment %d" % c
