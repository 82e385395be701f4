"""GPU parity tests of the fixed-base MSM over NATIVE table records (ecu.h AffineU: both coordinates in the multiplier's own limb
form, written once at pin time) -- msm_accum_kernel<native> and the heavy role on such records.  Every result is compared limb for
limb, after g1_to_affine, with the CPU oracle's best_multiexp; "both forms" also runs the same MSM over the E-form table forced with
h2hip_debug_set_table_records(64) and unpinned (plain form).  The engine takes native records (one per 128-byte line) from 2^13 points
on by itself; the small cases here force them the same way, and the lifecycle test also runs the packed 80-byte stride.
Run with `pytest -m gpu` on an MI355X."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)
NATIVE, PACKED, EFORM = 128, 80, 64


def aff(h2, xyz):
    return h2.g1_to_affine(xyz)


def set_records(h2, nbytes):
    assert h2.lib().h2hip_debug_set_table_records(ctypes.c_uint32(nbytes)) == 0


def set_stream(h2, chunks, permille=0, min_n=0):
    assert h2.lib().h2hip_debug_set_msm_stream(ctypes.c_uint32(chunks), ctypes.c_uint32(permille), ctypes.c_size_t(min_n)) == 0


def set_split(h2, on):
    assert h2.lib().h2hip_debug_set_msm_split_buckets(ctypes.c_int(on)) == 0


@pytest.fixture(autouse=True)
def _engine(h2):
    h2.init()
    yield
    set_records(h2, 0)
    set_stream(h2, 0)
    set_split(h2, 1)
    h2.set_msm_window(0)


def plan(c):
    """window starts of the table the engine builds for a requested width (msm.hip MsmPlan): W windows, the first q of them c bits wide"""
    W = (255 + c - 1) // c
    c = (255 + W - 1) // W
    q = 255 - W * (c - 1)
    widths = [c if w < q else c - 1 for w in range(W)]
    pos = [sum(widths[:w]) for w in range(W)]
    return c, W, widths, pos


def fr(oracle, ints):
    return np.ascontiguousarray(np.stack([oracle.fe_from_int(oracle.FR, int(v)) for v in ints]))


def neg_points(oracle, pts):
    out = pts.copy()
    y = np.ascontiguousarray(pts[:, 4:])
    out[:, 4:] = oracle.fe_binop("sub", oracle.FQ, np.zeros_like(y), y)
    return out


def pinned(h2, sc, bs, records, expect_c=None):
    """the MSM over bases pinned with the given record form"""
    set_records(h2, records)
    h2.bases_pin(bs)
    try:
        n, c, w, nbytes = h2.bases_pinned_info(bs)
        assert n == bs.shape[0] and c >= 2 and nbytes == w * n * records
        if expect_c:
            assert c == expect_c
        if isinstance(sc, list):
            return [aff(h2, r) for r in h2.best_multiexp_batch(sc, bs)]
        return aff(h2, h2.best_multiexp(sc, bs))
    finally:
        h2.bases_unpin(bs)
        set_records(h2, 0)


def both_forms(h2, oracle, sc, bs, tag):
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    assert np.array_equal(pinned(h2, sc, bs, NATIVE), want), (tag, "native")
    assert np.array_equal(pinned(h2, sc, bs, EFORM), want), (tag, "E-form")
    assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want), (tag, "plain")


@pytest.mark.parametrize("c", [13, 17, 20])
def test_table_content_entry_by_entry(h2, oracle, c):
    """Scalar 2^(pos_j) on point i and zero elsewhere: the MSM is table entry (j, i) alone, through the first-entry path (no product),
    and must equal 2^(pos_j) * P_i.  Widths: 13 and 20 have windows of two widths (15 x 13 + 5 x 12 bits, 8 x 20 + 5 x 19), 17 tiles the
    255 bits exactly (15 x 17).  (W * (c - 1) = 255 itself cannot occur: the engine takes c = ceil(255 / W).)"""
    n = 64
    bs = oracle.gen_points(0xA11CE, n, num_threads=NT)
    cn, W, widths, pos = plan(c)
    assert cn == c and sum(widths) == 255
    assert (len(set(widths)) == 2) == (c != 17)
    h2.set_msm_window(c)
    set_records(h2, NATIVE)
    h2.bases_pin(bs)
    try:
        assert h2.bases_pinned_info(bs)[1:] == (c, W, W * n * NATIVE)
        for j in range(W):
            s = oracle.fe_from_int(oracle.FR, 1 << pos[j])
            for i in range(n):
                sc = np.zeros((n, 4), dtype=np.uint64)
                sc[i] = s
                want = oracle.g1_to_affine(oracle.g1_mul(bs[i], s))
                assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want), (c, j, i)
    finally:
        h2.bases_unpin(bs)


def test_first_entry_and_short_buckets(h2, oracle):
    """n = 2^8 at c = 16: 4096 entries over 2^15 buckets, most buckets hold no entry or one"""
    n = 1 << 8
    bs = oracle.gen_points(0xB0B, n, num_threads=NT)
    sc = oracle.gen_scalars(0xB0C, n, num_threads=NT)
    h2.set_msm_window(16)
    both_forms(h2, oracle, sc, bs, "short")


@pytest.mark.parametrize("c", [4, 6])
def test_long_chains(h2, oracle, c):
    """n = 2^12 at c = 4 / 6: hundreds of entries in each of the 8 / 32 buckets"""
    n = 1 << 12
    bs = oracle.gen_points(0xC0DE, n, num_threads=NT)
    sc = oracle.gen_scalars(0xC0DF, n, num_threads=NT)
    h2.set_msm_window(c)
    both_forms(h2, oracle, sc, bs, c)


@pytest.mark.parametrize("sign", [-1, 1])
def test_every_digit_of_one_sign(h2, oracle, sign):
    """scalars built from their signed digits: every window's digit negative (the top window takes the last carry and cannot be: it is +1),
    or every digit positive"""
    n, c = 1 << 8, 13
    _, W, widths, pos = plan(c)
    rng = np.random.default_rng(7 + sign)
    ints = []
    for _ in range(n):
        d = [sign * int(rng.integers(1, 8)) for _ in range(W)]
        d[W - 1] = 1
        v = sum(dj << pos[j] for j, dj in enumerate(d))
        assert 0 < v < (1 << 253)
        ints.append(v)
    bs = oracle.gen_points(0x5167, n, num_threads=NT)
    h2.set_msm_window(c)
    both_forms(h2, oracle, fr(oracle, ints), bs, sign)


def test_edge_scalars(h2, oracle):
    """0, 1, r - 1 and 2^253, in turn"""
    n = 1 << 8
    bs = oracle.gen_points(0xED6E, n, num_threads=NT)
    vals = [0, 1, -1, 1 << 253]
    both_forms(h2, oracle, fr(oracle, [vals[i % 4] for i in range(n)]), bs, "edge")
    for v in vals:
        both_forms(h2, oracle, fr(oracle, [v] * n), bs, v)


@pytest.mark.parametrize("n", [1 << 6, 1 << 7, 1 << 8])
@pytest.mark.parametrize("pattern", ["double", "cancel_then_q", "cancel_then_double"])
def test_exceptional_cases_inside_a_bucket(h2, oracle, n, pattern):
    """Groups of bases that share one scalar land in the same buckets, window after window, in the order of their indices (one lane per
    bucket: the split into sub-lanes is switched off):  P, P (doubling);  P, -P, Q (cancel, then continue from the identity);
    P, -P, Q, Q (a doubling after a cancellation).  At c = 16 a bucket holds little besides one group."""
    pts = oracle.gen_points(0xE7C, n, num_threads=NT)
    P, Q = pts[0::2], pts[1::2]
    group = {"double": lambda p, q: [p, p], "cancel_then_q": lambda p, q: [p, neg_points(oracle, p[None])[0], q],
             "cancel_then_double": lambda p, q: [p, neg_points(oracle, p[None])[0], q, q]}[pattern]
    size = len(group(P[0], Q[0]))
    g = n // size
    bs = np.ascontiguousarray(np.concatenate([np.stack(group(P[k], Q[k])) for k in range(g)] + [pts[:n - g * size]]))
    s = oracle.gen_scalars(0xE7D, g + n, num_threads=NT)
    sc = np.ascontiguousarray(np.concatenate([np.repeat(s[:g], size, axis=0), s[g:g + n - g * size]]))
    assert bs.shape[0] == n and sc.shape[0] == n
    h2.set_msm_window(16)
    set_split(h2, 0)
    both_forms(h2, oracle, sc, bs, pattern)
    # all scalars equal: one chain per window through the whole array, the pattern repeating along it
    h2.set_msm_window(6)
    both_forms(h2, oracle, np.ascontiguousarray(np.repeat(s[:1], n, axis=0)), bs, pattern + " equal")


@pytest.mark.parametrize("where", ["first", "middle", "all"])
def test_identity_points_among_the_bases(h2, oracle, where):
    n = 1 << 7
    bs = oracle.gen_points(0x1D, n, num_threads=NT)
    if where == "first":
        bs[0] = 0
    elif where == "middle":
        bs[n // 2 - 3:n // 2 + 3] = 0
        bs[1::7] = 0
    else:
        bs[:] = 0
    sc = oracle.gen_scalars(0x1E, n, num_threads=NT)
    set_split(h2, 0)
    both_forms(h2, oracle, sc, bs, where)
    both_forms(h2, oracle, np.ascontiguousarray(np.repeat(sc[:1], n, axis=0)), bs, where + " equal")


def test_heavy_role_reads_native_records(h2, oracle):
    """a prover-like column (90 % zeros, 5 % ones and twos): the buckets of 1 and 2 are over-full and go to the heavy role"""
    n = 1 << 14
    rng = np.random.default_rng(0x4EA)
    bs = oracle.gen_points(0x4EB, n, num_threads=NT)
    sc = oracle.gen_scalars(0x4EC, n, num_threads=NT)
    u = rng.random(n)
    sc[u < 0.90] = 0
    sc[(u >= 0.90) & (u < 0.925)] = oracle.fe_from_int(oracle.FR, 1)
    sc[(u >= 0.925) & (u < 0.95)] = oracle.fe_from_int(oracle.FR, 2)
    both_forms(h2, oracle, sc, bs, "prover")
    set_records(h2, 0)
    h2.bases_pin(bs)
    try:
        assert h2.bases_pinned_info(bs)[3] == h2.bases_pinned_info(bs)[2] * n * NATIVE  # from 2^13 points native is the engine's own choice
    finally:
        h2.bases_unpin(bs)


def test_continued_sums_across_streamed_chunks(h2, oracle):
    """the streamed host-pointer path (cont = 1: chunk k adds into the parts chunks < k left) at n = 2^12, four equal chunks, c = 20 so that
    most buckets hold one entry per chunk at most: the third quarter repeats the first quarter's pairs negated (a filled bucket meets -P
    and becomes the identity), the last quarter repeats them as they were (a first entry into a stored identity) and doubles others"""
    n = 1 << 12
    q = n // 4
    bs = oracle.gen_points(0x57E, n, num_threads=NT)
    sc = oracle.gen_scalars(0x57F, n, num_threads=NT)
    bs[2 * q:3 * q] = neg_points(oracle, bs[:q])
    sc[2 * q:3 * q] = sc[:q]
    bs[3 * q:3 * q + q // 2] = bs[:q // 2]
    sc[3 * q:3 * q + q // 2] = sc[:q // 2]
    bs[3 * q + q // 2:] = bs[q:q + q // 2]
    sc[3 * q + q // 2:] = sc[q:q + q // 2]
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    for c in (20, 13):
        h2.set_msm_window(c)
        for chunks in (4, 2):
            set_stream(h2, chunks, 1000, 1024)
            assert np.array_equal(pinned(h2, sc, bs, NATIVE, c), want), (c, chunks, "native")
            assert np.array_equal(pinned(h2, sc, bs, EFORM, c), want), (c, chunks, "E-form")
    h2.set_msm_window(0)  # (the plain form has a bucket set per window: its own width)
    set_stream(h2, 4, 1000, 1024)
    assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want), "plain"


def test_fused_batch_over_native_records(h2, oracle):
    n = 1 << 10
    bs = oracle.gen_points(0xF05E, n, num_threads=NT)
    cols = [oracle.gen_scalars(0xF100 + k, n, num_threads=NT) for k in range(4)]
    cols[1][::3] = 0
    cols[2][:] = cols[2][0]
    want = [oracle.g1_to_affine(oracle.best_multiexp(s, bs, NT)) for s in cols]
    for records in (NATIVE, EFORM):
        got = pinned(h2, cols, bs, records)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), records


def test_pin_lifecycle_and_table_bytes(h2, oracle):
    """pin -> MSM -> unpin -> MSM (plain) -> pin in the other form -> MSM, all equal; the bytes reported are rows x n x the stride in use"""
    n = 1 << 11
    bs = oracle.gen_points(0x11FE, n, num_threads=NT)
    sc = oracle.gen_scalars(0x11FF, n, num_threads=NT)
    want = oracle.g1_to_affine(oracle.best_multiexp(sc, bs, NT))
    for first, second in ((NATIVE, EFORM), (EFORM, PACKED), (PACKED, NATIVE)):
        assert np.array_equal(pinned(h2, sc, bs, first), want)  # (checks the bytes against the stride)
        assert np.array_equal(aff(h2, h2.best_multiexp(sc, bs)), want)
        assert np.array_equal(pinned(h2, sc, bs, second), want)
    # the engine's own choice: E-form below 2^13 points
    h2.bases_pin(bs)
    try:
        _, c, w, nbytes = h2.bases_pinned_info(bs)
        assert nbytes == w * n * EFORM
    finally:
        h2.bases_unpin(bs)
    assert h2.lib().h2hip_debug_set_table_records(ctypes.c_uint32(72)) != 0  # not a stride the kernel's 16-byte fetch can take
