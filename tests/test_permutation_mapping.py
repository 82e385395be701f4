"""The permutation mapping from copy constraints (h2hip_permutation_mapping[_device], include/halo2hip.h): every cell maps to the next
cell of its connected component in ascending column * 2^k + row order.  The definition is later than the reference, so
tests/copies_util.py restates it (a dict union-find and `sorted`) and the engine is compared with that byte for byte; the restatement
itself is checked against a hand-written answer and, as sets of cycles, against the literal port of Assembly::copy."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import copies_util as cu
import keygen_util as ku
from keygen_util import R_MOD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------ the restatement (CPU)
def test_restatement_known_answer():
    """k = 2, two columns: the 3-cycle (0,0) (0,2) (1,1) spans both columns, (0,3) (1,0) is a 2-cycle, (0,1), (1,2), (1,3) are untouched"""
    got = cu.ordered_mapping(2, 2, [(0, 0, 1, 1), (1, 1, 0, 2), (0, 3, 1, 0)])
    want = [[(0, 2), (0, 1), (1, 1), (1, 0)],
            [(0, 3), (0, 0), (1, 2), (1, 3)]]
    assert got.dtype == np.uint32 and got.tolist() == [[list(c) for c in col] for col in want]


@pytest.mark.parametrize("k,m", [(4, 1), (5, 2), (6, 3), (7, 4), (8, 5)])
def test_restatement_has_the_cycles_of_assembly_copy(h2, k, m):
    n = 1 << k
    for seed, count in ((1, 1), (2, n // 2), (3, 2 * m * n)):
        seq = cu.random_copies(seed * 1000 + k, k, m, count).tolist()
        asm = h2.PermutationAssembly(n, m)
        for c in seq:
            asm.copy(*c)
        assert cu.cycles(cu.ordered_mapping(k, m, seq)) == cu.cycles(asm.mapping), (k, m, count)


def test_restatement_ignores_order_and_sides():
    k, m = 6, 3
    seq = cu.random_copies(7, k, m, 150)
    want = cu.ordered_mapping(k, m, seq.tolist())
    assert np.array_equal(cu.ordered_mapping(k, m, cu.shuffled(seq, 8).tolist()), want)
    assert np.array_equal(cu.ordered_mapping(k, m, cu.swapped(seq, 9).tolist()), want)
    assert np.array_equal(cu.ordered_mapping(k, m, np.concatenate([seq, seq[::3], [[1, 5, 1, 5]]]).tolist()), want)  # repeats, a self-copy


# ------------------------------------------------------------------ the ABI without a GPU
def test_header_declares_and_library_exports(h2):
    header = open(os.path.join(ROOT, "include", "halo2hip.h")).read()
    for name in ("h2hip_permutation_mapping", "h2hip_permutation_mapping_device"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(h2.lib(), name), name
    assert "valid, not byte-identical" in header


def test_bad_arguments_are_einval_before_any_device_work(h2):
    L = h2.lib()
    host, dev = L.h2hip_permutation_mapping, L.h2hip_permutation_mapping_device
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    cell = np.zeros((4, 2), dtype=np.uint32)
    tab = (ctypes.c_void_p * 17)(*[cell.ctypes.data] * 17)
    cp = np.array([[0, 0, 1, 1]], dtype=np.uint32)
    err = lambda: L.h2hip_last_error().decode()  # noqa: E731
    assert host(u32(2), u32(2), h2._p(cp), sz(1), None) == 1 and "null mapping" in err()              # NULL tables
    assert host(u32(2), u32(2), None, sz(1), tab) == 1 and "null copies" in err()
    hole = (ctypes.c_void_p * 2)(cell.ctypes.data, None)
    assert host(u32(2), u32(2), h2._p(cp), sz(1), hole) == 1 and "mapping[1] is null" in err()
    assert dev(u32(2), u32(2), h2._p(cp), sz(1), None, None) == 1 and dev(u32(2), u32(2), None, sz(1), tab, None) == 1
    for f, extra in ((host, ()), (dev, (None,))):
        assert f(u32(29), u32(1), h2._p(cp), sz(1), tab, *extra) == 1 and "k = 29" in err()           # k = 29
        assert f(u32(0), u32(65536), h2._p(cp), sz(1), tab, *extra) == 1 and "65536" in err()         # n_columns = 65536
        assert f(u32(28), u32(17), h2._p(cp), sz(1), tab, *extra) == 1 and "2^32" in err()            # n_columns 2^k = 2^32 + 2^k
        assert f(u32(2), u32(2), h2._p(cp), sz((1 << 30) + 1), tab, *extra) == 1 and "n_copies" in err()
    with pytest.raises(h2.H2HipError, match="rc=1.*2\\^32"):
        h2.permutation_mapping(28, 17, [])
    # an out-of-range copy: the lowest offending index is named
    seq = [(0, 0, 1, 1), (0, 1, 1, 2), (0, 4, 1, 0), (2, 0, 0, 0), (0, 0, 0, 9)]
    with pytest.raises(h2.H2HipError, match=r"rc=1.*copies\[2\] = \(0, 4\) - \(1, 0\)"):
        h2.permutation_mapping(2, 2, seq)
    with pytest.raises(h2.H2HipError, match=r"rc=1.*copies\[3\] = \(2, 0\) - \(0, 0\)"):
        h2.permutation_mapping(2, 2, seq[:2] + seq[:1] + seq[3:])
    # nothing to write: no device is needed
    assert host(u32(3), u32(0), h2._p(cp), sz(0), None) == 0 and dev(u32(3), u32(0), None, sz(0), None, None) == 0


def test_copy_list_checks_as_the_assembly_does(h2):
    cl, asm = h2.CopyList(8, 2), h2.PermutationAssembly(8, 2)
    for bad in ((2, 0, 0, 0), (0, 0, 2, 0), (0, 8, 0, 0), (0, 0, 1, 8), (-1, 0, 0, 0)):
        for a in (cl, asm):
            with pytest.raises(ValueError):
                a.copy(*bad)
    cl.copy(0, 1, 1, 7)
    assert cl.array().tolist() == [[0, 1, 1, 7]] and cl.array().dtype == np.uint32
    dom = h2.EvaluationDomain.new(4, 3)
    with pytest.raises(ValueError, match="not both"):
        h2.keygen_columns(None, dom, [], np.zeros((2, 8, 2), np.uint32), 2, copies=cl)
    with pytest.raises(ValueError, match="not both"):
        h2.verify_witness(3, [], [], np.zeros(4, np.uint64), 2, [], np.zeros((0, 8, 2), np.uint32), copies=cl)


_NO_GPU_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from conftest import load_pkg
h2 = load_pkg()
cl = h2.CopyList(8, 2)
cl.copy(0, 1, 1, 7)
calls = [lambda: h2.permutation_mapping(3, 2, [(0, 1, 1, 7)]), lambda: h2.permutation_mapping(3, 2, []), lambda: cl.mapping()]
for i, f in enumerate(calls):
    try:
        f()
    except h2.H2HipError as e:
        assert "rc=2" in str(e), str(e)
    else:
        raise SystemExit("call %d succeeded without a GPU" % i)
print("loud")
"""


def test_mapping_calls_without_gpu_fail_loudly(tmp_path):
    """every valid call raises H2HipError (H2HIP_EDEVICE) when no device is visible: a fresh process with the GPUs hidden, so the test
    says the same on a machine with and without one"""
    script = tmp_path / "no_gpu.py"
    script.write_text(_NO_GPU_SCRIPT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("HALO2_HIP_DEVICES", None)
    r = subprocess.run([sys.executable, str(script), HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "loud" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_copies_host_program():
    """tests/cpp/test_copies_host: pack, unpack and order of the 64-bit keys, the cell numbering and the successor rule at cell ids 0,
    2^31 - 1, 2^31 and 2^32 - 1 (the mapping tables ids this large would need are too big for a GPU test)"""
    exe = os.path.join(HERE, "cpp", "test_copies_host")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), "../tests/cpp/test_copies_host"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the engine against the restatement (GPU)
def device_mapping(h2, k, m, copies):
    """the _device form over torch tensors -> ((m, 2^k, 2) uint32, the error or None)"""
    import torch
    n = 1 << k
    cp = np.ascontiguousarray(np.asarray(copies, dtype=np.uint32).reshape(-1, 4))
    d_cp = torch.from_numpy(cp.view(np.int32).copy()).cuda() if len(cp) else None
    d_map = [torch.full((n, 2), -1, dtype=torch.int32, device="cuda") for _ in range(m)]
    err = None
    try:
        h2.permutation_mapping_device(k, m, d_cp, d_map, len(cp))
    except h2.H2HipError as e:
        err = e
    return np.stack([t.cpu().numpy().view(np.uint32) for t in d_map]), err


def both_forms(h2, k, m, copies, want=None):
    """host and device form against the restatement, byte for byte; returns the mapping"""
    cp = np.asarray(copies, dtype=np.uint32).reshape(-1, 4)
    want = cu.ordered_mapping(k, m, cp.tolist()) if want is None else want
    got = h2.permutation_mapping(k, m, cp)
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), "host form"
    got_d, err = device_mapping(h2, k, m, cp)
    assert err is None and np.array_equal(got_d, want), "device form"
    return want


def identity(k, m):
    return cu.ordered_mapping(k, m, [])


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(0, 1), (10, 3)])
def test_no_copies_is_the_identity(h2, k, m):
    want = both_forms(h2, k, m, [])
    assert want[:, :, 0].tolist() == [[j] * (1 << k) for j in range(m)] and want[:, :, 1].tolist() == [list(range(1 << k))] * m


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 10, 13])
@pytest.mark.parametrize("m", [1, 3, 9])
@pytest.mark.parametrize("count", ["one", "half", "giant"])
def test_random_copies(h2, k, m, count):
    n = 1 << k
    C = {"one": 1, "half": n // 2, "giant": 4 * m * n}[count]
    want = both_forms(h2, k, m, cu.random_copies(k * 100 + m * 10 + len(count), k, m, C))
    if count == "giant":  # one component holds (nearly) every cell
        assert max(len(c) for c in cu.cycles(want)) > 0.9 * m * n


@functools.lru_cache(maxsize=None)
def _chain(k):
    n = 1 << k
    asc = np.array([(0, i, 0, i + 1) for i in range(n - 1)], dtype=np.uint32)
    return asc, cu.ordered_mapping(k, 1, asc.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_over_all_rows(h2, order):
    """k = 16, one column, (0, i) - (0, i + 1) over all rows: the deepest walks"""
    asc, want = _chain(16)
    assert want[0, :-1, 1].tolist() == list(range(1, 1 << 16)) and want[0, -1].tolist() == [0, 0]
    cp = {"ascending": asc, "descending": asc[::-1], "shuffled": cu.shuffled(asc, 16)}[order]
    both_forms(h2, 16, 1, cp, want)


@pytest.mark.gpu
@pytest.mark.parametrize("centre", ["first", "last"])
def test_star(h2, centre):
    """k = 12, m = 3: every cell joined to cell 0, and every cell joined to the last cell (m - 1, n - 1) -- there the root changes under
    every hook"""
    k, m = 12, 3
    n = 1 << k
    c = (0, 0) if centre == "first" else (m - 1, n - 1)
    cp = [(j, i, c[0], c[1]) for j in range(m) for i in range(n)]
    want = both_forms(h2, k, m, cp)
    flat = want.reshape(-1, 2)
    assert flat[:-1].tolist() == [[(x + 1) // n, (x + 1) % n] for x in range(m * n - 1)] and flat[-1].tolist() == [0, 0]


@pytest.mark.gpu
def test_one_cell_in_64_consecutive_copies(h2):
    """same-wave contention on one word: 64 consecutive copies touch (1, 77), on either side, among random ones"""
    k, m = 10, 3
    cp = cu.random_copies(64, k, m, 512)
    cp[128:192, 0:2] = (1, 77)
    cp[160:192] = cp[160:192][:, [2, 3, 0, 1]]
    both_forms(h2, k, m, cp)
    lone = cu.random_copies(65, k, m, 64)
    lone[:, 2:4] = (2, 1023)
    both_forms(h2, k, m, lone)


@pytest.mark.gpu
def test_repeated_edges_and_self_copies(h2):
    k, m = 10, 3
    cp = cu.random_copies(8, k, m, 300)
    selfs = cu.random_copies(9, k, m, 100)
    selfs[:, 2:4] = selfs[:, 0:2]
    every = cu.shuffled(np.concatenate([np.repeat(cp, 8, axis=0), selfs, cp[:, [2, 3, 0, 1]]]), 10)
    want = both_forms(h2, k, m, every)
    assert np.array_equal(want, cu.ordered_mapping(k, m, cp.tolist()))
    both_forms(h2, k, m, selfs, identity(k, m))  # self-copies alone, one of them maybe the last cell: nothing changes


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, 3])
def test_disjoint_small_cycles(h2, size):
    """n / 2 disjoint 2-cycles and n / 3 disjoint 3-cycles over shuffled cells: the wrap-around of every component"""
    k, m = 10, 3
    n = 1 << k
    cells = np.random.default_rng(size).permutation(m * n)[:(n // size) * size].reshape(-1, size)
    cp = [(a // n, a % n, b // n, b % n) for grp in cells.tolist() for a, b in zip(grp, grp[1:])]
    want = both_forms(h2, k, m, cp)
    sizes = sorted(len(c) for c in cu.cycles(want))
    assert sizes.count(size) == n // size and sizes.count(1) == m * n - (n // size) * size


@pytest.mark.gpu
def test_components_with_the_first_and_the_last_cell(h2):
    k, m = 10, 3
    n = 1 << k
    last = (m - 1, n - 1)
    want = both_forms(h2, k, m, [(0, 0, *last)])
    assert want[0, 0].tolist() == list(last) and want[last].tolist() == [0, 0]
    mid = cu.random_copies(11, k, m, 40)
    want = both_forms(h2, k, m, np.concatenate([[(*last, 1, 5)], mid, [(1, 5, 0, 0)]]))
    assert want[last].tolist() == [0, 0]
    both_forms(h2, k, m, [(*last, *last), (0, 0, 0, 0)], identity(k, m))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["B-1", "B", "B+1", "2B+1"])
@pytest.mark.parametrize("shape", ["pairs", "path"])
def test_touched_cells_around_the_sort_block(h2, which, shape):
    """T distinct touched cells at the sort's block B (the keys one workgroup sorts in LDS; it is fixed, there is no hook to shrink it):
    as disjoint pairs the T (or T + 1) endpoint keys fill one tile less one, one tile, one tile and two keys, two tiles and two keys --
    the merge passes then run over one, two and three tiles, the last run short or single; as a path every inner cell is a key twice"""
    B, passes0 = h2.copies_sort_plan(0)
    assert B == 2048 and passes0 == 0
    T = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[which]
    k, m = 12, 3
    n = 1 << k
    cells = np.random.default_rng(T).permutation(m * n)[:T].tolist()
    if shape == "pairs":
        pairs = list(zip(cells[0::2], cells[1::2])) + ([(cells[-1], cells[0])] if T & 1 else [])
        assert h2.copies_sort_plan(len(pairs)) == (B, {B - 1: 0, B: 0, B + 1: 1, 2 * B + 1: 2}[T])
    else:
        pairs = list(zip(cells, cells[1:]))
    want = both_forms(h2, k, m, [(a // n, a % n, b // n, b % n) for a, b in pairs])
    assert int((want.reshape(-1, 2) != identity(k, m).reshape(-1, 2)).any(axis=1).sum()) == T


@pytest.mark.gpu
def test_k18(h2):
    """k = 18, m = 2, C = 2^18 at the default block: 256 tiles, eight merge passes"""
    k, m, C = 18, 2, 1 << 18
    assert h2.copies_sort_plan(C) == (2048, 8)
    both_forms(h2, k, m, cu.random_copies(18, k, m, C))


@pytest.mark.gpu
def test_determinism(h2):
    k, m = 13, 3
    cp = cu.random_copies(21, k, m, 6000)
    a, err = device_mapping(h2, k, m, cp)
    assert err is None
    for other in (cp, cu.shuffled(cp, 22), cu.swapped(cp, 23)):
        b, err = device_mapping(h2, k, m, other)
        assert err is None and a.tobytes() == b.tobytes()
        assert h2.permutation_mapping(k, m, other).tobytes() == a.tobytes()


@pytest.mark.gpu
def test_device_form_ignores_copies_out_of_range(h2):
    k, m = 10, 3
    n = 1 << k
    cp = cu.random_copies(31, k, m, 700)
    cp[5] = (m, 0, 0, 0)
    cp[100] = (0, n, 1, 1)
    cp[101] = (1, 1, 0xFFFFFFFF, 3)
    cp[699] = (2, 7, 2, n + 7)
    got, err = device_mapping(h2, k, m, cp)
    assert err is not None and "rc=1" in str(err) and "ignored" in str(err)
    valid = cu.valid_copies(k, m, cp.tolist())
    assert len(valid) == 696 and np.array_equal(got, cu.ordered_mapping(k, m, valid))
    got, err = device_mapping(h2, k, m, cu.random_copies(32, k, m, 700))  # the flag does not stick
    assert err is None


@pytest.mark.gpu
def test_device_call_on_a_side_stream_then_host_call(h2):
    import torch
    k, m = 13, 4
    n = 1 << k
    cp, cp2 = cu.random_copies(41, k, m, 20000), cu.random_copies(42, k, 2, 3000)
    d_cp = torch.from_numpy(cp.view(np.int32).copy()).cuda()
    d_map = [torch.empty((n, 2), dtype=torch.int32, device="cuda") for _ in range(m)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h2.permutation_mapping_device(k, m, d_cp, d_map)
    got2 = h2.permutation_mapping(k, 2, cp2)  # host form on the engine's stream, at once
    side.synchronize()
    assert np.array_equal(got2, cu.ordered_mapping(k, 2, cp2.tolist()))
    assert np.array_equal(np.stack([t.cpu().numpy().view(np.uint32) for t in d_map]), cu.ordered_mapping(k, m, cp.tolist()))


# ------------------------------------------------------------------ the mapping in the calls that consume it (GPU)
def _witness(k, m, mapping, seed):
    """integer columns that are constant on the mapping's cycles"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    cols = [[int(x) for x in rng.integers(1, 1 << 62, size=n)] for _ in range(m)]
    for cyc in cu.cycles(mapping):
        cyc = sorted(cyc)
        for x in cyc[1:]:
            cols[x // n][x % n] = cols[cyc[0] // n][cyc[0] % n]
    return cols


@pytest.mark.gpu
def test_the_mapping_closes_the_permutation_argument(h2):
    k, m, b = 10, 5, 5
    n = 1 << k
    u = n - b - 1
    cp = cu.random_copies(51, k, m, 1500, rows=u)
    mapping = both_forms(h2, k, m, cp)
    dom = h2.EvaluationDomain.new(4, k)
    sigma = h2.permutation_keygen(dom, mapping, want=("permutations",))["permutations"]
    cols = _witness(k, m, mapping, 52)
    # a cell of a component of three or more, and the cell that maps to it
    cyc = sorted(next(c for c in sorted(cu.cycles(mapping), key=min) if len(c) >= 3))
    x, pred = cyc[1], cyc[0]
    assert mapping[pred // n, pred % n].tolist() == [x // n, x % n]
    bad = [list(c) for c in cols]
    bad[x // n][x % n] += 1
    one, delta = ku.fe(1), h2.fr_from_int(h2.FR_DELTA)
    beta, gamma = ku.fe(0x1234567 * 0x89ABCDEF % R_MOD), ku.fe(pow(3, 200, R_MOD))
    good_m, bad_m = [ku.to_mont(c) for c in cols], [ku.to_mont(c) for c in bad]
    for chunk_len in (1, 3, m):
        n_sets = -(-m // chunk_len)
        blind = ku.to_mont(range(100, 100 + n_sets * b))
        z = h2.permutation_products(k, dom.omega, delta, beta, gamma, good_m, sigma, chunk_len, blind, b)
        assert np.array_equal(z[-1][u], one), chunk_len
        z = h2.permutation_products(k, dom.omega, delta, beta, gamma, bad_m, sigma, chunk_len, blind, b)
        assert not np.array_equal(z[-1][u], one), chunk_len
    counts, rows = h2.check_permutation(k, good_m, mapping)
    assert counts.tolist() == [0] * m
    counts, rows = h2.check_permutation(k, bad_m, mapping)
    named = sorted((j, int(r)) for j in range(m) for r in rows[j][:int(counts[j])])
    assert named == sorted([(x // n, x % n), (pred // n, pred % n)])


@pytest.mark.gpu
def test_keygen_from_copies_equals_keygen_of_the_mapping(h2):
    k, m = 10, 3
    cp = cu.random_copies(61, k, m, 900)
    dom = h2.EvaluationDomain.new(4, k)
    want = h2.permutation_keygen(dom, h2.permutation_mapping(k, m, cp))
    got = h2.permutation_keygen_from_copies(dom, m, cp)
    assert sorted(got) == sorted(want) == ["cosets", "permutations", "polys"]
    for form in want:
        assert len(got[form]) == m and all(np.array_equal(g, w) for g, w in zip(got[form], want[form])), form
    sig = ku.sigma_mont(cu.ordered_mapping(k, m, cp.tolist()), ku.root_of_unity(k))
    assert all(np.array_equal(g, w) for g, w in zip(got["permutations"], sig))
    only = h2.permutation_keygen_from_copies(dom, m, h2.CopyList(1 << k, m).array(), want=("polys",))
    assert sorted(only) == ["polys"] and len(only["polys"]) == m


@pytest.mark.gpu
def test_verify_witness_takes_copies(h2):
    k, m, b = 6, 3, 5
    n = 1 << k
    cp = cu.random_copies(71, k, m, 40, rows=n - b - 1)
    mapping = cu.ordered_mapping(k, m, cp.tolist())
    cols = _witness(k, m, mapping, 72)
    perm = [("advice", 0), ("fixed", 0), ("advice", 1)]
    theta = ku.fe(5)
    cl = h2.CopyList(n, m)
    for c in cp.tolist():
        cl.copy(*c)
    for change in (False, True):
        if change:
            x = next(min(c) for c in cu.cycles(mapping) if len(c) >= 2)
            cols[x // n][x % n] += 1
        mc = [ku.to_mont(c) for c in cols]
        kw = dict(advice=[mc[0], mc[2]], fixed=[mc[1]])
        want = h2.verify_witness(k, [], [], theta, b, perm, mapping, **kw)
        assert (len(want) == 2) if change else (want == [])
        assert h2.verify_witness(k, [], [], theta, b, perm, None, copies=cp, **kw) == want
        assert h2.verify_witness(k, [], [], theta, b, perm, None, copies=cl, **kw) == want


@pytest.mark.gpu
def test_cpp_mirror_copy_assembly(h2, tmp_path):
    """tests/cpp/test_copies_mirror runs CopyAssembly through keygen_pk and build_vk; its mapping and sigma columns against the
    restatement, the other forms against the engine's keygen of that mapping"""
    exe = os.path.join(HERE, "cpp", "test_copies_mirror")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), "../tests/cpp/test_copies_mirror"])
    k, j, b, m = 10, 4, 5, 3
    n = 1 << k
    cp = cu.random_copies(81, k, m, 700)
    words = [k, j, b, m, len(cp)] + cp.reshape(-1).tolist()
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.array(words, dtype=np.uint64).tofile(inp)
    subprocess.run([exe, str(inp), str(outp)], check=True, timeout=300)
    raw = np.fromfile(outp, dtype=np.uint64)
    mapping = raw[:m * n].view(np.uint32).reshape(m, n, 2)
    assert np.array_equal(mapping, cu.ordered_mapping(k, m, cp.tolist()))
    dom = h2.EvaluationDomain.new(j, k)
    ext = dom.extended_len()
    at = m * n
    want = h2.permutation_keygen(dom, mapping)
    assert all(np.array_equal(a, b_) for a, b_ in zip(want["permutations"], ku.sigma_mont(mapping, ku.root_of_unity(k))))
    for form, rows in (("permutations", n), ("polys", n), ("cosets", ext)):
        got = raw[at:at + m * rows * 4].reshape(m, rows, 4)
        at += m * rows * 4
        assert all(np.array_equal(g, w) for g, w in zip(got, want[form])), form
    assert raw.shape[0] == at + m * 8  # build_vk's commitments: m affine points
