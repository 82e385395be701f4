"""GPU parity tests of the round-2 MSM paths, through the C ABI, bit-exact (after normalising to affine) against the
CPU oracle and the golden vectors:
  * the fixed-base form (window tables built by h2hip_bases_pin / h2hip_bases_pin_device), every window width;
  * the pinned-bases cache's guard against stale host pointers;
  * fused batches larger than one run (count > 4096 / W windows);
  * the shape of the reference's own config-5 columns (examples/circuit-layout.rs);
  * the multi-device engine, rehearsed on one GPU with the same device listed twice.
Run with `pytest -m gpu` on an MI355X."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module", autouse=True)
def _engine(h2):
    h2.init()
    yield
    h2.set_msm_window(0)


def aff(h2, xyz):
    return h2.g1_to_affine(xyz)


@pytest.mark.parametrize("case", ["1", "2", "3", "4", "31", "32", "33", "100", "1024", "zeros", "ones", "rm1", "single", "sparse", "cancel"])
def test_fixed_base_golden(h2, golden, case):
    sc, bs = golden[f"msm_{case}_scalars"], np.ascontiguousarray(golden[f"msm_{case}_bases"])
    h2.bases_pin(bs)
    try:
        n, c, w, nbytes = h2.bases_pinned_info(bs)
        assert n == bs.shape[0] and c >= 2 and w == (255 + c - 1) // c and nbytes == w * n * 64
        assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), golden[f"msm_{case}_result"])
    finally:
        h2.bases_unpin(bs)


@pytest.mark.parametrize("c", [2, 3, 5, 8, 11, 13, 16, 17, 20, 22])
def test_fixed_base_all_window_widths(h2, golden, c):
    """the table is built with the width in force at pin time; 18, 21 and 24-bit requests normalise to 17, 20, 22"""
    h2.set_msm_window(c)
    try:
        for case in ("33", "1024", "sparse", "rm1"):
            sc, bs = golden[f"msm_{case}_scalars"], np.ascontiguousarray(golden[f"msm_{case}_bases"])
            h2.bases_pin(bs)
            try:
                assert h2.bases_pinned_info(bs)[1] == c
                assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), golden[f"msm_{case}_result"]), (c, case)
            finally:
                h2.bases_unpin(bs)
    finally:
        h2.set_msm_window(0)


def test_window_requests_are_normalised(h2, golden):
    sc, bs = golden["msm_1024_scalars"], np.ascontiguousarray(golden["msm_1024_bases"])
    for asked, used in ((18, 17), (21, 20), (24, 22), (23, 22), (19, 19)):
        h2.set_msm_window(asked)
        try:
            h2.bases_pin(bs)
            assert h2.bases_pinned_info(bs)[1] == used
            assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), golden["msm_1024_result"])
            h2.bases_unpin(bs)
            if asked < 20:  # plain form, same width (wider plain windows need more buckets than one run sorts)
                assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), golden["msm_1024_result"])
        finally:
            h2.set_msm_window(0)


@pytest.mark.parametrize("n", [1 << 10, (1 << 12) + 37, 1 << 14, 1 << 16])
def test_fixed_base_vs_oracle_seeded(h2, oracle, n):
    sc = oracle.gen_scalars(0x5EED0001, n, num_threads=NT)
    bs = oracle.gen_points(0x5EED0002, n, num_threads=NT)
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    h2.bases_pin(bs)
    try:
        assert h2.bases_pinned_info(bs)[1] > 0
        assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want)
        # a shorter polynomial over the same params (commit of a column with fewer coefficients): same table
        for m in (n // 2, 100, 1):
            want_m = oracle.g1_to_affine(oracle.best_multiexp(sc[:m], bs[:m], NT))
            assert np.array_equal(aff(h2, h2.best_multiexp(sc[:m], bs[:m])), want_m), m
    finally:
        h2.bases_unpin(bs)


def test_fixed_base_skewed_and_degenerate_inputs(h2, oracle):
    n = 1 << 14
    bs = oracle.gen_points(77, n, num_threads=NT)
    one = oracle.fe_from_int(oracle.FR, 1)
    rng = np.random.default_rng(5)
    cols = []
    cols.append(np.repeat(oracle.gen_scalars(78, 1), n, axis=0))        # every scalar equal: one over-full bucket per window
    sc = oracle.gen_scalars(79, n, num_threads=NT)                        # prover-like: 90 % zero, 5 % in {1, 2}
    u = rng.random(n)
    sc[u < 0.90] = 0
    sc[(u >= 0.90) & (u < 0.95)] = one
    cols.append(sc)
    cols.append(np.repeat(one[None, :], n, axis=0))                       # a selector column of ones
    cols.append(np.zeros((n, 4), dtype=np.uint64))                        # the zero polynomial: identity
    h2.bases_pin(bs)
    try:
        for j, sc in enumerate(cols):
            want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
            assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want), j
    finally:
        h2.bases_unpin(bs)
    # all bases equal (doublings inside the buckets and the trees), and bases containing the identity
    bs1 = np.repeat(bs[:1], n, axis=0)
    bs1[5] = 0
    h2.bases_pin(bs1)
    try:
        want = oracle.g1_to_affine(oracle.best_multiexp(cols[1], bs1, NT))
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[1], bs1)), want)
    finally:
        h2.bases_unpin(bs1)


@pytest.mark.parametrize("c", [7, 8, 13, 14, 17, 20, 22])
def test_host_finished_tail_equals_the_gpu_tail_and_the_oracle(h2, oracle, golden, c):
    """round 4: a run with few bucket sets stops at the bit-plane sums of its row / column sums and the host finishes with one Horner
    (msm_planes_kernel + msm_planes_finish).  Same group element as the all-GPU tail (h2hip_debug_set_msm_plane_tail(0)) and as the
    oracle -- on uniform scalars, on columns that put everything into one bucket (planes that are one point or the identity), on r - 1
    and on scalars whose digits make equal points meet inside the plane trees (doubling) -- plain and fixed-base, lone and a fused pair.
    The exceptional additions here are incidental; tests/test_msm_reduce_edges.py places them one by one (bucket sums chosen by the test, in
    every kernel of every tail, with an integer model that says which addition of which stage each case makes exceptional)."""
    L = h2.lib()
    n = 1 << 12
    bs = oracle.gen_points(0x5EED0002, n, num_threads=NT)
    uni = oracle.gen_scalars(0x5EED0001, n, num_threads=NT)
    same = np.repeat(uni[:1], n, axis=0)                      # every pair the same scalar
    rm1 = np.repeat(golden["msm_rm1_scalars"][:1], n, axis=0)
    small = np.zeros((n, 4), dtype=np.uint64)                # scalars 1 (Montgomery form): one bucket, one window
    small[:] = h2.fr_from_int(1)
    dup = bs.copy()
    dup[1::2] = dup[0::2]                                    # pairs of equal points: equal partial sums meet in the trees
    h2.set_msm_window(c)
    try:
        for sc, pts in ((uni, bs), (same, bs), (rm1, bs), (small, bs), (uni, dup), (same, dup)):
            want = oracle.g1_to_affine(oracle.best_multiexp(sc, pts, NT))
            for pinned in (False, True):
                if not pinned and c > 17:
                    continue  # the plain form keeps one bucket set per window: widths beyond 17 bits are for window tables only
                if pinned:
                    h2.bases_pin(pts)
                try:
                    got = {}
                    for on in (1, 0):
                        L.h2hip_debug_set_msm_plane_tail(ctypes.c_int(on))
                        got[on] = aff(h2, h2.best_multiexp(sc, pts))
                    assert np.array_equal(got[1], want) and np.array_equal(got[0], want), (c, pinned)
                    if pinned:  # a fused pair of fixed-base MSMs is a run of two sets: host-finished as well
                        L.h2hip_debug_set_msm_plane_tail(ctypes.c_int(1))
                        two = h2.best_multiexp_batch([sc, uni], pts)
                        assert np.array_equal(aff(h2, two[0]), want)
                        assert np.array_equal(aff(h2, two[1]), oracle.g1_to_affine(oracle.best_multiexp(uni, pts, NT)))
                finally:
                    L.h2hip_debug_set_msm_plane_tail(ctypes.c_int(1))
                    if pinned:
                        h2.bases_unpin(pts)
    finally:
        h2.set_msm_window(0)


def test_pinned_cache_detects_a_reused_allocation(h2, oracle):
    """A Vec that is freed and whose address is handed out again must not hit the stale device copy
    (VERDICT r1 'weak'): the lookup compares 16 sampled points and falls back to uploading."""
    n = 1 << 12
    sc = oracle.gen_scalars(5, n, num_threads=NT)
    bs = oracle.gen_points(6, n, num_threads=NT)
    other = oracle.gen_points(7, n, num_threads=NT)
    h2.bases_pin(bs)
    want_old = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want_old)
    bs[:] = other  # same address, new contents: what a reused allocation looks like
    want_new = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want_new)
    with pytest.raises(h2.H2HipError):  # the stale entry was dropped by the lookup
        h2.bases_unpin(bs)


def test_device_pinned_entry_points(h2, oracle):
    import torch
    n = 1 << 13
    ds = h2.gen_scalars_device(0x5EED0001, n)
    dp = h2.gen_points_device(0x5EED0002, n)
    sc, bs = h2.to_numpy_u64(ds), h2.to_numpy_u64(dp)
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    h2.bases_pin_device(dp)
    try:
        info = h2.bases_pinned_info(dp)
        assert info[0] == n and info[1] > 0
        assert np.array_equal(aff(h2, h2.msm_device(ds, dp)), want)
        assert np.array_equal(aff(h2, h2.msm_device(ds, dp, n=1000)), oracle.g1_to_affine(oracle.best_multiexp(sc[:1000], bs[:1000], NT)))
        cols = [h2.gen_scalars_device(40 + j, n) for j in range(5)]
        got = h2.msm_batch_device(cols, dp)  # fused, fixed-base: one bucket set per MSM
        for j, col in enumerate(cols):
            w = oracle.g1_to_affine(oracle.best_multiexp(h2.to_numpy_u64(col), bs, NT))
            assert np.array_equal(aff(h2, got[j]), w), j
    finally:
        h2.bases_unpin_device(dp)
    assert np.array_equal(aff(h2, h2.msm_device(ds, dp)), want)  # plain form again


def test_device_pinned_cache_detects_a_reused_address(h2, oracle):
    """the device address is the cache key, and torch's caching allocator hands a freed address out
    again readily.  A buffer whose contents changed under a pinned key (same address, other points: what a freed and
    reused allocation looks like) must cost a miss, never the old table's commitment -- single and batched entry points,
    a prefix of the array, and a real free + reallocate at the same address."""
    import torch
    n = 1 << 13
    ds = h2.gen_scalars_device(0x5EED0001, n)
    dp = h2.gen_points_device(0x5EED0002, n)
    other = h2.gen_points_device(0x5EED0042, n)
    sc = h2.to_numpy_u64(ds)
    want_old = oracle.g1_to_affine(oracle.best_multiexp(sc, h2.to_numpy_u64(dp), NT))
    want_new = oracle.g1_to_affine(oracle.best_multiexp(sc, h2.to_numpy_u64(other), NT))
    h2.bases_pin_device(dp)
    assert np.array_equal(aff(h2, h2.msm_device(ds, dp)), want_old)
    dp.copy_(other)
    torch.cuda.synchronize()
    assert np.array_equal(aff(h2, h2.msm_device(ds, dp)), want_new)
    with pytest.raises(h2.H2HipError):  # the lookup dropped the stale entry
        h2.bases_unpin_device(dp)
    # batched entry point, and a prefix shorter than the pinned array (only the samples below n are compared)
    h2.bases_pin_device(dp)
    cols = [h2.gen_scalars_device(70 + j, n) for j in range(3)]
    got = h2.msm_batch_device(cols, dp)
    dp.copy_(h2.gen_points_device(0x5EED0043, n))
    torch.cuda.synchronize()
    bs3 = h2.to_numpy_u64(dp)
    got3 = h2.msm_batch_device(cols, dp)
    for j in range(3):
        assert not np.array_equal(got3[j], got[j])
        assert np.array_equal(aff(h2, got3[j]), oracle.g1_to_affine(oracle.best_multiexp(h2.to_numpy_u64(cols[j]), bs3, NT))), j
    h2.bases_pin_device(dp)
    dp[:64].copy_(other[:64])  # the head of the array changes: a 1000-pair prefix sees it
    torch.cuda.synchronize()
    bs4 = h2.to_numpy_u64(dp)
    assert np.array_equal(aff(h2, h2.msm_device(ds, dp, n=1000)), oracle.g1_to_affine(oracle.best_multiexp(sc[:1000], bs4[:1000], NT)))
    # a real free + reallocation: the next tensor of the same size lands on the same address (caching allocator)
    h2.bases_pin_device(dp)
    addr = dp.data_ptr()
    keep_alive = h2._device_pins.pop(addr)  # take the Python-side finalizer out of the picture: only the library's guard is left
    keep_alive.detach()
    del dp
    dq = h2.gen_points_device(0x5EED0044, n)
    if dq.data_ptr() == addr:
        assert np.array_equal(aff(h2, h2.msm_device(ds, dq)), oracle.g1_to_affine(oracle.best_multiexp(sc, h2.to_numpy_u64(dq), NT)))
    else:  # the allocator chose another block: drop the orphan entry by its address
        import ctypes
        assert h2.lib().h2hip_bases_unpin(ctypes.c_void_p(addr)) == 0


def test_device_pin_follows_the_tensor_lifetime(h2):
    """the Python wrapper ties the entry to the tensor's storage (weakref.finalize): dropping the last tensor over it unpins,
    dropping a temporary view the pin went through does not"""
    import ctypes
    import gc
    dp = h2.gen_points_device(0x5EED0002, 1 << 10)
    h2.bases_pin_device(dp.view(-1))  # pinned through a temporary view, collected at once
    addr = dp.data_ptr()
    gc.collect()
    assert addr in h2._device_pins and h2.bases_pinned_info(dp)[0] == 1 << 10
    del dp
    gc.collect()
    assert addr not in h2._device_pins
    assert h2.lib().h2hip_bases_unpin(ctypes.c_void_p(addr)) != 0  # already gone


@pytest.mark.parametrize("n,count", [(1 << 10, 200), (1 << 13, 200)])
def test_large_batches_split_into_several_fused_runs(h2, oracle, n, count):
    """count * W windows used to overflow a fixed limit instead of splitting"""
    dp = h2.gen_points_device(0x5EED0002, n)
    cols = [h2.gen_scalars_device(1000 + j, n) for j in range(count)]
    got = h2.msm_batch_device(cols, dp)
    for j in (0, 1, 57, 113, 157, 158, count - 1):
        assert np.array_equal(aff(h2, got[j]), aff(h2, h2.msm_device(cols[j], dp))), j
    bs = h2.to_numpy_u64(dp)
    w = oracle.g1_to_affine(oracle.best_multiexp(h2.to_numpy_u64(cols[113]), bs, NT))
    assert np.array_equal(aff(h2, got[113]), w)
    h2.bases_pin_device(dp)
    try:
        got2 = h2.msm_batch_device(cols, dp)
        for j in range(count):
            assert np.array_equal(aff(h2, got2[j]), aff(h2, got[j])), j
    finally:
        h2.bases_unpin_device(dp)


def test_config5_column_shape_k17(h2, oracle):
    """BASELINE.json configs[4]: the advice columns of examples/circuit-layout.rs at k = 17 hold about twenty assigned
    rows (examples/circuit-layout.rs:245-265), blinding_factors() + 1 random rows at the end (plonk/prover.rs:350-354)
    and zeros everywhere else -- 99.98 % zero.  Through the single call, the fused batch and the fixed-base form."""
    k, n = 17, 1 << 17
    bs = oracle.gen_points(0x5EED0002, n, num_threads=NT)
    rng = np.random.default_rng(17)
    cols = []
    for j in range(4):
        col = np.zeros((n, 4), dtype=np.uint64)
        rows = rng.choice(64, size=20, replace=False)
        vals = oracle.gen_scalars(300 + j, 20)
        small = oracle.fe_from_int(oracle.FR, int(rng.integers(1, 5)))
        vals[::3] = small  # the circuit assigns small constants and products of them
        col[rows] = vals
        col[n - 6:] = oracle.gen_scalars(400 + j, 6)  # blinding rows
        cols.append(col)
    want = [oracle.g1_to_affine(oracle.best_multiexp(c, bs, NT)) for c in cols]
    for j, c in enumerate(cols):
        assert np.array_equal(aff(h2, h2.best_multiexp(c, bs)), want[j]), j
    got = h2.best_multiexp_batch(cols, bs)
    for j in range(4):
        assert np.array_equal(aff(h2, got[j]), want[j]), j
    h2.bases_pin(bs)
    try:
        got = h2.best_multiexp_batch(cols, bs)
        for j in range(4):
            assert np.array_equal(aff(h2, got[j]), want[j]), j
            assert np.array_equal(aff(h2, h2.best_multiexp(cols[j], bs)), want[j]), j
    finally:
        h2.bases_unpin(bs)


def test_fixed_base_2p20_and_plain_agree(h2, oracle):
    """BASELINE.json configs[1] through the fixed-base form: bit-exact vs the CPU path at 2^20"""
    n = 1 << 20
    ds = h2.gen_scalars_device(0x5EED0001, n)
    dp = h2.gen_points_device(0x5EED0002, n)
    plain = aff(h2, h2.msm_device(ds, dp))
    h2.bases_pin_device(dp)
    try:
        assert h2.bases_pinned_info(dp)[1] == h2.get_msm_window_fixed_base(n)
        fixed = aff(h2, h2.msm_device(ds, dp))
    finally:
        h2.bases_unpin_device(dp)
    assert np.array_equal(plain, fixed)
    want = oracle.g1_to_affine(oracle.best_multiexp(h2.to_numpy_u64(ds), h2.to_numpy_u64(dp), NT))
    assert np.array_equal(fixed, want)


# ---------------------------------------------------------------------------- several devices behind the C ABI
_MULTI = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from conftest import load_pkg
from oracle import oracle
h2 = load_pkg()
out = {}
ndev = h2.device_count()
out["device_count"] = ndev
# (1) a device list the box cannot serve is a clean error, not a silent single-GPU run
try:
    h2.init([0, ndev])
    out["bad_list"] = "accepted"
except h2.H2HipError as e:
    out["bad_list"] = "rejected: " + str(e)
# (2) a duplicate is refused unless the rehearsal switch is set
dup_allowed = os.environ.get("HALO2_HIP_ALLOW_DUPLICATE_DEVICES") == "1"
try:
    h2.init([0, 0])
    out["dup"] = "accepted"
except h2.H2HipError as e:
    out["dup"] = "rejected"
if dup_allowed:
    assert h2.num_devices() == 2
    n = 1 << 16
    sc = oracle.gen_scalars(0x5EED0001, n, num_threads=8)
    bs = oracle.gen_points(0x5EED0002, n, num_threads=8)
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, 8)).tolist()
    out["sharded_equal"] = h2.g1_to_affine(h2.best_multiexp(sc, bs)).tolist() == want
    out["sharded_odd_equal"] = h2.g1_to_affine(h2.best_multiexp(sc[:n - 3], bs[:n - 3])).tolist() == \
        oracle.g1_to_affine(oracle.best_multiexp(sc[:n - 3], bs[:n - 3], 8)).tolist()
    h2.bases_pin(bs)
    n_p, c, w, nbytes = h2.bases_pinned_info(bs)
    out["pinned_points"] = n_p
    out["pinned_equal"] = h2.g1_to_affine(h2.best_multiexp(sc, bs)).tolist() == want
    m = n // 2 + 11  # ends inside the second device's share
    out["pinned_prefix_equal"] = h2.g1_to_affine(h2.best_multiexp(sc[:m], bs[:m])).tolist() == \
        oracle.g1_to_affine(oracle.best_multiexp(sc[:m], bs[:m], 8)).tolist()
    cols = [oracle.gen_scalars(50 + j, n, num_threads=8) for j in range(3)]
    got = h2.best_multiexp_batch(cols, bs)
    out["batch_equal"] = all(h2.g1_to_affine(got[j]).tolist() == oracle.g1_to_affine(oracle.best_multiexp(cols[j], bs, 8)).tolist() for j in range(3))
    h2.bases_unpin(bs)
    # round 3: each device's shard streams in (chunk ladder into persistent buckets), pinned and unpinned
    import ctypes
    h2.lib().h2hip_debug_set_msm_stream(ctypes.c_uint32(3), ctypes.c_uint32(600), ctypes.c_size_t(4096))
    out["stream_unpinned_equal"] = h2.g1_to_affine(h2.best_multiexp(sc, bs)).tolist() == want
    h2.bases_pin(bs)
    out["stream_pinned_equal"] = h2.g1_to_affine(h2.best_multiexp(sc, bs)).tolist() == want
    got = h2.best_multiexp_batch(cols, bs)
    out["stream_batch_equal"] = all(h2.g1_to_affine(got[j]).tolist() == oracle.g1_to_affine(oracle.best_multiexp(cols[j], bs, 8)).tolist() for j in range(3))
    h2.bases_unpin(bs)
    h2.lib().h2hip_debug_set_msm_stream(ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0))
    # round 3: batched transforms split by owning device (here: dealt round-robin to the two contexts of the one GPU), the
    # groups run concurrently on their own host threads; results equal the one-column calls
    import torch
    k = 12
    dom = h2.EvaluationDomain.new(4, k)
    cols_h = [oracle.gen_scalars(900 + j, 1 << k, num_threads=8) for j in range(5)]
    d_cols = [torch.from_numpy(c_.view(np.int64)).cuda() for c_ in cols_h]
    h2.ntt_batch_device(d_cols, dom.omega, k)
    torch.cuda.synchronize()
    out["ntt_batch_equal"] = all(np.array_equal(h2.to_numpy_u64(d_cols[j]), oracle.best_fft(cols_h[j], dom.omega, k, 4)) for j in range(5))
    h2.ifft_batch_device(d_cols, dom.omega_inv, k, dom.ifft_divisor)
    torch.cuda.synchronize()
    out["ifft_batch_roundtrip"] = all(np.array_equal(h2.to_numpy_u64(d_cols[j]), cols_h[j]) for j in range(5))
    ext = [torch.zeros((1 << dom.extended_k) * 4, dtype=torch.int64, device="cuda") for _ in range(3)]
    od, _ = oracle.domain_new(4, k)
    for j in range(3):
        ext[j][:(1 << k) * 4] = d_cols[j].reshape(-1)
    h2.coeff_to_extended_batch_device(ext, k, dom.extended_k, dom.extended_omega, dom.g_coset, dom.g_coset_inv)
    torch.cuda.synchronize()
    out["coeff_to_extended_batch_equal"] = all(np.array_equal(h2.to_numpy_u64(ext[j]).reshape(-1, 4), oracle.coeff_to_extended(od, cols_h[j].copy(), 4)) for j in range(3))
    # round 3: entry points from several threads at once (per-device locks; ctypes drops the GIL during the calls)
    import threading
    d_big = [h2.gen_scalars_device(77 + j, 1 << 16) for j in range(4)]
    dp_t = h2.gen_points_device(78, 1 << 14)
    ds_t = [h2.gen_scalars_device(79 + j, 1 << 14) for j in range(4)]
    exp_ntt = []
    dom16 = h2.EvaluationDomain.new(2, 16)
    for t_ in d_big:
        c_ = t_.clone()
        h2.ntt_device(c_, dom16.omega, 16)
        exp_ntt.append(h2.to_numpy_u64(c_).copy())
    exp_msm = [h2.g1_to_affine(h2.msm_device(s_, dp_t)) for s_ in ds_t]  # the group element: Jacobian coordinates depend on the addition order
    res = [None] * 8
    def work_ntt(j):
        for _ in range(5):
            c_ = d_big[j].clone()
            h2.ntt_device(c_, dom16.omega, 16)
            torch.cuda.synchronize()
            res[j] = bool(np.array_equal(h2.to_numpy_u64(c_), exp_ntt[j]))
            if not res[j]:
                return
    def work_msm(j):
        for _ in range(5):
            res[4 + j] = bool(np.array_equal(h2.g1_to_affine(h2.msm_device(ds_t[j], dp_t)), exp_msm[j]))
            if not res[4 + j]:
                return
    ths = [threading.Thread(target=work_ntt, args=(j,)) for j in range(4)] + [threading.Thread(target=work_msm, args=(j,)) for j in range(4)]
    for t_ in ths:
        t_.start()
    for t_ in ths:
        t_.join()
    out["threads_ok"] = all(r_ is True for r_ in res)
    small = h2.g1_to_affine(h2.best_multiexp(sc[:100], bs[:100])).tolist()  # below the sharding threshold: device 0 only
    out["small_equal"] = small == oracle.g1_to_affine(oracle.best_multiexp(sc[:100], bs[:100], 8)).tolist()
    h2.shutdown()
    h2.init(0)
    out["after_reinit_equal"] = h2.g1_to_affine(h2.best_multiexp(sc, bs)).tolist() == want
print("RESULT " + json.dumps(out))
"""


def _run_multi(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _MULTI % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_init_device_list_errors_are_clean():
    out = _run_multi({"HALO2_HIP_ALLOW_DUPLICATE_DEVICES": "0"})
    assert out["bad_list"].startswith("rejected") and "out of range" in out["bad_list"]
    assert out["dup"] == "rejected"


def test_two_device_contexts_shard_fold_bit_exact():
    """h2hip_init with two entries (the same GPU twice: the rehearsal switch) runs the sharded path of h2hip_msm_bn254:
    one host thread, stream and workspace per context, pinned bases split by range, partials folded -- and gives the
    single-device result bit for bit.  (RCCL refuses duplicate devices, so the partials meet through host memory
    here; the ncclAllGather path needs distinct GPUs.)"""
    out = _run_multi({"HALO2_HIP_ALLOW_DUPLICATE_DEVICES": "1", "HALO2_HIP_MULTI_GPU_MIN_N": "1024"})
    assert out["dup"] == "accepted"
    for key in ("sharded_equal", "sharded_odd_equal", "pinned_equal", "pinned_prefix_equal", "batch_equal", "small_equal", "after_reinit_equal",
                "stream_unpinned_equal", "stream_pinned_equal", "stream_batch_equal", "ntt_batch_equal", "ifft_batch_roundtrip",
                "coeff_to_extended_batch_equal", "threads_ok"):
        assert out[key] is True, (key, out)
    assert out["pinned_points"] == 1 << 16


_MULTI3 = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from conftest import load_pkg
from oracle import oracle
h2 = load_pkg()
out = {}
h2.init([0, 0, 0])
out["devices"] = h2.num_devices()
aff = lambda x: h2.g1_to_affine(x).tolist()
orc = lambda s_, b_: oracle.g1_to_affine(oracle.best_multiexp(s_, b_, 8)).tolist()
# (1) a pin whose shares are uneven: n not divisible by the device count
n = (1 << 16) + 5
sc = oracle.gen_scalars(0x5EED0001, n, num_threads=8)
bs = oracle.gen_points(0x5EED0002, n, num_threads=8)
h2.bases_pin(bs)
out["pinned_points"] = h2.bases_pinned_info(bs)[0]
out["uneven_equal"] = aff(h2.best_multiexp(sc, bs)) == orc(sc, bs)
# (2) polynomials shorter than the pinned SRS: only the first device's share / ending inside the second's -- trailing devices idle
for name, m in (("prefix_first_share", n // 3 - 7), ("prefix_two_shares", n // 3 + 1000), ("prefix_all_but_one", n - 1), ("prefix_tiny", 2000)):
    out[name] = aff(h2.best_multiexp(sc[:m], bs[:m])) == orc(sc[:m], bs[:m])
cols = [oracle.gen_scalars(50 + j, n // 2, num_threads=8) for j in range(4)]
got = h2.best_multiexp_batch(cols, bs[:n // 2])
out["batch_prefix_equal"] = all(aff(got[j]) == orc(cols[j], bs[:n // 2]) for j in range(4))
h2.bases_unpin(bs)
# (3) BASELINE.json configs[3]'s shape in small: ONE fixed-base MSM sharded over every device of the engine, gather asked over RCCL.
# The same card thrice cannot form a communicator: the call must fall back to the host fold and still be right.
n4 = 1 << 18
sc4 = oracle.gen_scalars(0x5EED0011, n4, num_threads=8)
bs4 = oracle.gen_points(0x5EED0012, n4, num_threads=8)
h2.bases_pin(bs4)
out["config4_shape_equal"] = aff(h2.best_multiexp(sc4, bs4)) == orc(sc4, bs4)
h2.bases_unpin(bs4)
# (4) host-pointer batched transforms dealt over three contexts (7 columns: shares of 2 / 2 / 3), each share its own pipeline
k = 12
dom = h2.EvaluationDomain.new(4, k)
od, _ = oracle.domain_new(4, k)
cols_h = [oracle.gen_scalars(900 + j, 1 << k, num_threads=8) for j in range(7)]
out["host_batch_ifft_equal"] = all(np.array_equal(g_, oracle.lagrange_to_coeff(od, c_, 4)) for g_, c_ in zip(dom.lagrange_to_coeff_batch(cols_h), cols_h))
out["host_batch_coset_equal"] = all(np.array_equal(g_, oracle.coeff_to_extended(od, c_.copy(), 4)) for g_, c_ in zip(dom.coeff_to_extended_batch(cols_h), cols_h))
out["host_batch_two_columns"] = all(np.array_equal(g_, oracle.lagrange_to_coeff(od, c_, 4)) for g_, c_ in zip(dom.lagrange_to_coeff_batch(cols_h[:2]), cols_h[:2]))
h2.shutdown()
print("RESULT " + json.dumps(out))
"""


def test_three_device_contexts_uneven_shares_idle_devices_and_rccl_fallback():
    """the multi-device engine has only ever run as rehearsals on one card, so the rehearsal covers the shapes an
    8-GPU node will produce: a pin whose shares are uneven (n not divisible by N), polynomials shorter than the pinned SRS (trailing
    devices idle), config 4's shape (one fixed-base MSM over every device) with HALO2_HIP_GATHER=rccl falling back cleanly where
    ncclCommInitAll refuses, and the host-pointer batched transforms dealt over the devices."""
    env = dict(os.environ, HALO2_HIP_ALLOW_DUPLICATE_DEVICES="1", HALO2_HIP_MULTI_GPU_MIN_N="1024", HALO2_HIP_GATHER="rccl")
    r = subprocess.run([sys.executable, "-c", _MULTI3 % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert out["devices"] == 3 and out["pinned_points"] == (1 << 16) + 5
    for key, val in out.items():
        if key not in ("devices", "pinned_points"):
            assert val is True, (key, out)


def test_env_device_list_and_thresholds():
    code = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import load_pkg
h2 = load_pkg()
h2.init()
print("RESULT", h2.num_devices(), h2.msm_min_n(), h2.ntt_min_log_n())
""" % (ROOT, ROOT)
    env = dict(os.environ, HALO2_HIP_DEVICES="0", HALO2_HIP_MSM_MIN_N="4096", HALO2_HIP_NTT_MIN_LOGN="12")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()[1:] == ["1", "4096", "12"]
    env["HALO2_HIP_DEVICES"] = "0,99"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "out of range" in (r.stdout + r.stderr)


def test_rccl_gather_path_on_this_box(h2, oracle, golden):
    """the ncclCommInitAll / ncclAllGather plumbing of the in-library multi-GPU gather, on however many devices the
    engine holds here (one): the gathered-and-folded partials must come back as the same group elements"""
    sc, bs = golden["msm_33_scalars"], golden["msm_33_bases"]
    parts = np.stack([oracle.best_multiexp(sc[:10], bs[:10]), oracle.best_multiexp(sc[10:], bs[10:]), oracle.best_multiexp(sc, bs)])
    out = np.zeros((3, 12), dtype=np.uint64)
    rc = h2.lib().h2hip_debug_rccl_gather_selftest(parts.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(3), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, h2.lib().h2hip_last_error().decode()
    for j in range(3):
        assert np.array_equal(aff(h2, out[j]), oracle.g1_to_affine(parts[j])), j


def test_allgather_fold_over_rccl_single_rank():
    """bench.py's N > 1 exchange (halo2-pse_amd/dist.py) with the real backend: a one-rank `nccl` (= RCCL) process group on
    this box's GPU takes the 96-byte partial up through pinned memory, all-gathers it and folds it back to the same point"""
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", HSA_ENABLE_IPC_MODE_LEGACY="0")
import torch, torch.distributed as dist
from conftest import load_pkg
from importlib import import_module
h2 = load_pkg(); h2dist = import_module("halo2_pse_amd.dist")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
h2.init(0)
ds = h2.gen_scalars_device(1, 1000); dp = h2.gen_points_device(2, 1000)
part = h2.msm_device(ds, dp)
for _ in range(3):
    tot = h2dist.allgather_fold(part, h2, device=torch.device("cuda", 0))
print("RESULT", bool(np.array_equal(h2.g1_to_affine(tot), h2.g1_to_affine(part))))
dist.destroy_process_group()
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "RESULT True" in r.stdout


def test_lazy_cache_pins_after_k_sightings_and_stays_correct(h2, oracle):
    """HALO2_HIP_LAZY_PIN (here through the test hook): the unpatched drop-in passes the same &params.g[..] to every
    best_multiexp.  The k-th unpinned sighting of an array pins it (window table included); results stay the oracle's before,
    at and after that call; a reused allocation is caught by the fingerprint; at most four arrays are held, LRU first out."""
    import ctypes
    L = h2.lib()
    n = 1 << 13
    bs = oracle.gen_points(5100, n, num_threads=NT)
    cols = [oracle.gen_scalars(5110 + j, n, num_threads=NT) for j in range(4)]
    want = [oracle.g1_to_affine(oracle.best_multiexp(c, bs, NT)) for c in cols]

    def pinned(a):
        try:
            return h2.bases_pinned_info(a)
        except h2.H2HipError:
            return None

    assert h2.lazy_pin_after() == 0  # off unless asked for
    assert L.h2hip_debug_set_lazy_pin(ctypes.c_uint32(2)) == 0
    others = []
    try:
        assert h2.lazy_pin_after() == 2
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[0], bs)), want[0])
        assert pinned(bs) is None                      # seen once
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[1], bs)), want[1])
        info = pinned(bs)                              # second sighting: pinned before this MSM ran
        assert info is not None and info[0] == n and info[1] == h2.get_msm_window_fixed_base(n) and info[2] > 0
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[2], bs)), want[2])
        # a prefix of the array (commit of a shorter polynomial) uses the same entry
        m = n - 100
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[3][:m], bs[:m])), oracle.g1_to_affine(oracle.best_multiexp(cols[3][:m], bs[:m], NT)))
        assert pinned(bs) is not None
        # the allocation is "reused": same address, other points -> the entry is dropped, the result is the new array's
        bs[:] = oracle.gen_points(5200, n, num_threads=NT)
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[0], bs)), oracle.g1_to_affine(oracle.best_multiexp(cols[0], bs, NT)))
        assert pinned(bs) is None                      # first sighting of the new content
        assert np.array_equal(aff(h2, h2.best_multiexp(cols[1], bs)), oracle.g1_to_affine(oracle.best_multiexp(cols[1], bs, NT)))
        assert pinned(bs) is not None
        # five more arrays: at most four stay pinned, the least recently used (bs) goes first
        for j in range(5):
            o = oracle.gen_points(5300 + j, 2048, num_threads=NT)
            others.append(o)
            sc = oracle.gen_scalars(5400 + j, 2048, num_threads=NT)
            for _ in range(2):
                assert np.array_equal(aff(h2, h2.best_multiexp(sc, o)), oracle.g1_to_affine(oracle.best_multiexp(sc, o, NT)))
        held = [o for o in [bs] + others if pinned(o) is not None]
        assert len(held) == 4 and pinned(bs) is None and pinned(others[0]) is None and pinned(others[4]) is not None
        # an explicit unpin removes a lazily pinned array like any other
        h2.bases_unpin(others[4])
        assert pinned(others[4]) is None
    finally:
        L.h2hip_debug_set_lazy_pin(ctypes.c_uint32(0))
        for o in [bs] + others:
            if pinned(o) is not None:
                h2.bases_unpin(o)
