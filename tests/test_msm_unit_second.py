"""GPU tests of the addition of a bucket's SECOND record (csrc/ecu.h: the unit form of xyzzu_add_mixed_nonid, taken by msm_accum_kernel
when every lane of a wave that adds holds a bucket's first record as it was copied).  Small runs whose buckets hold exactly 1, 2 and 3
records, with crafted second records (an equal point, the opposite point, an identity base first or second), in the plain form and in
the fixed-base form with every table record format; split parts, the over-full path, a continued (streamed) run, and waves whose lanes
reach their second and third records together.  Every result is the CPU oracle's group element exactly (affine coordinates).

How a bucket is named.  The recoding (msm.hip for_each_digit) cuts a scalar into windows of c bits, window 0 lowest.  A scalar d with
1 <= d <= 2^(c-1) has one non-zero digit: +d in window 0, bucket d - 1, and nothing else.  The scalar 2^c - d (2 <= d < 2^(c-1)) has
the digit -d in window 0 -- the same bucket with the sign set -- and a carry: the digit +1 in window 1, which is bucket 0 of window 1
(plain form) or bucket 0 of the one shared set with the table's 2^c P (fixed-base form).  So the cases that need exact bucket lengths
use positive digits only, and the cases with negative digits leave bucket 0 to the carries.

One lane per bucket.  With few buckets the engine gives a bucket up to 8 lanes, each adding every 8th record: a bucket of 2 or 3
records would then meet only in msm_combine_kernel.  The exact-length, mixed-wave and crafted cases therefore run with
h2hip_debug_set_msm_split_buckets(0), so that one lane of msm_accum_kernel adds a bucket's first, second and third record in turn;
test_split_parts_* keeps the split on.
Run with `pytest -m gpu` on an MI355X."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)
FORMS = ["plain", 64, 80, 128]  # the plain form, and the fixed-base form with E-form / native 80-byte / native 128-byte table records


def aff(h2, xyz):
    return h2.g1_to_affine(xyz)


@pytest.fixture(scope="module", autouse=True)
def _engine(h2):
    h2.init()
    yield
    h2.lib().h2hip_debug_set_msm_stream(ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0))
    h2.lib().h2hip_debug_set_table_records(ctypes.c_uint32(0))
    h2.lib().h2hip_debug_set_msm_split_buckets(ctypes.c_int(1))
    h2.set_msm_window(0)


@pytest.fixture
def one_lane_per_bucket(h2):
    """the split of a bucket over several lanes off for the test, and on again after it (the library's default)"""
    assert h2.lib().h2hip_debug_set_msm_split_buckets(ctypes.c_int(0)) == 0
    yield
    h2.lib().h2hip_debug_set_msm_split_buckets(ctypes.c_int(1))


@pytest.fixture(scope="module")
def points(oracle):
    """4096 points, computed once and left unchanged"""
    bs = oracle.gen_points(0x0171CE, 4096, num_threads=NT)
    bs.setflags(write=False)
    return bs


def neg_points(oracle, pts):
    out = pts.copy()
    y = np.ascontiguousarray(pts[:, 4:])
    out[:, 4:] = oracle.fe_binop("sub", oracle.FQ, np.zeros_like(y), y)
    return out


def digit_scalars(oracle, digits, c):
    """Scalars (Montgomery form) whose window-0 digit at width c is the given one: d > 0 is the scalar d, d < 0 the scalar 2^c - |d|,
    which also carries +1 into window 1 (see the module docstring)."""
    nb = 1 << (c - 1)
    vals = []
    for d in digits:
        d = int(d)
        assert 1 <= d <= nb or -nb < d <= -2, d
        vals.append(d if d > 0 else (1 << c) + d)
    return np.ascontiguousarray(np.stack([oracle.fe_from_int(oracle.FR, v) for v in vals]))


def run_form(h2, form, c, sc, bs):
    """one MSM in the given form at window width c (0: the engine's choice); the table is pinned with the record format in force"""
    sc, bs = np.ascontiguousarray(sc), np.ascontiguousarray(bs)
    L = h2.lib()
    h2.set_msm_window(c)
    try:
        if form == "plain":
            return aff(h2, h2.best_multiexp(sc, bs))
        assert L.h2hip_debug_set_table_records(ctypes.c_uint32(form)) == 0
        h2.bases_pin(bs)
        try:
            return aff(h2, h2.best_multiexp(sc, bs))
        finally:
            h2.bases_unpin(bs)
    finally:
        L.h2hip_debug_set_table_records(ctypes.c_uint32(0))
        h2.set_msm_window(0)


def check(h2, oracle, form, c, sc, bs, tag):
    want = oracle.g1_to_affine(oracle.best_multiexp(np.ascontiguousarray(sc), np.ascontiguousarray(bs), NT))
    got = run_form(h2, form, c, sc, bs)
    assert np.array_equal(got, want), (tag, form, c)


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("per_bucket", [1, 2, 3])
def test_buckets_of_exactly_one_two_and_three_records(h2, oracle, points, one_lane_per_bucket, form, per_bucket):
    """every bucket of the run holds exactly `per_bucket` records, at every width 3..8: the 2^(c-1) buckets of window 0, positive digits
    only (no carries), one lane per bucket -- all lanes copy, then all add onto a unit accumulator, then all add onto a general one"""
    for c in (3, 4, 5, 6, 7, 8):
        nb = 1 << (c - 1)
        digits = np.repeat(np.arange(1, nb + 1), per_bucket)
        n = len(digits)
        bs = points[:n].copy()
        bs[::5] = neg_points(oracle, bs[::5])  # both signs of y among the records
        check(h2, oracle, form, c, digit_scalars(oracle, digits, c), bs, ("exact", per_bucket))


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_mixed_waves_reach_second_and_third_records_together(h2, oracle, points, one_lane_per_bucket, form):
    """Bucket b holds 1 + b % 3 records: in one wave some lanes have nothing more to add, some add their second record onto a unit
    accumulator and some their third onto a general one -- the ballot guard sends the wave through the general form when the lanes
    differ.  Every seventh record has a negative digit (the sign bit of the entry; bucket 0 collects those records' carries and holds
    as many records as there are).  Then lengths 3, 2 and 1 in runs (the buckets are walked in descending size, so lanes of equal
    length sit side by side and the first wave changes from the third record's form to none at lane 40), and uniform scalars at 64 pairs and c = 8, where the buckets hold 0 to 3 records (plain form)."""
    c = 8
    nb = 1 << (c - 1)
    digits = np.concatenate([np.full(1 + b % 3, b) for b in range(2, nb)])
    digits = np.where(np.arange(len(digits)) % 7 == 3, -digits, digits)
    check(h2, oracle, form, c, digit_scalars(oracle, digits, c), points[:len(digits)], "1-2-3")
    digits = np.concatenate([np.full(3 if b <= 40 else 2 if b <= 90 else 1, b) for b in range(1, nb + 1)])
    check(h2, oracle, form, c, digit_scalars(oracle, digits, c), points[:len(digits)], "3-2-1 runs")
    sc = oracle.gen_scalars(0x0171CF, 64, num_threads=NT)
    check(h2, oracle, form, c, sc, points[:64], "uniform 64")


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_crafted_second_records(h2, oracle, points, one_lane_per_bucket, form):
    """Buckets whose second record is an exceptional case of the group law, one lane per bucket.  Bucket contents, in index order:
    [P, P] and [P, P, Q] (a doubling on the second record), [P, -P, Q] (a cancellation, then a copy onto the identity), [0, P, Q] and
    [P, 0, Q] (an identity base first / second).  The order inside a bucket is the sort's, so every arrangement of each bucket's
    records is built as well.  Odd groups use negative digits: the same buckets with the entry's sign bit set, their carries in
    bucket 0, which no crafted bucket uses."""
    c = 8
    bs = points[:1024].copy()
    neg = neg_points(oracle, bs)
    digits, pts = [], []
    ident = np.zeros(8, dtype=np.uint64)
    d = 2
    for k in range(9):
        P, Q, mP = bs[3 * k], bs[3 * k + 1], neg[3 * k]
        sign = -1 if k % 2 else 1
        for recs in ([P, P], [P, P, Q], [P, Q, P], [Q, P, P],
                     [P, mP, Q], [P, Q, mP], [Q, P, mP], [P, mP],
                     [ident, P, Q], [P, ident, Q], [P, Q, ident], [ident, P], [P, ident], [ident, ident, P]):
            assert d < 128
            for r in recs:
                digits.append(sign * d)
                pts.append(r)
            d += 1
    sc = digit_scalars(oracle, digits, c)
    check(h2, oracle, form, c, sc, np.stack(pts), "crafted")
    # the same records under full-width scalars shared inside each group: equal and opposite points then meet in every window (in the
    # fixed-base form the windows share one bucket set, so there the groups also meet each other: lengths are no longer exact)
    rnd = oracle.gen_scalars(0x0171D0, 128, num_threads=NT)
    sc = np.ascontiguousarray(rnd[np.abs(np.array(digits))])
    check(h2, oracle, form, c, sc, np.stack(pts), "crafted, all windows")


@pytest.mark.parametrize("form", FORMS[1:], ids=str)
def test_split_parts_of_one_to_four_records(h2, oracle, points, form):
    """64 pairs over a c = 8 table: 128 buckets with a mean of 16 records are accumulated by 8 lanes each, parts of 1 to 4 records"""
    sc = oracle.gen_scalars(0x0171D1, 64, num_threads=NT)
    check(h2, oracle, form, 8, sc, points[:64], "split")
    bs = points[:64].copy()
    bs[1::2] = bs[0::2]  # equal points with equal scalars: doublings inside the parts and where the parts meet
    sc2 = sc.copy()
    sc2[1::2] = sc2[0::2]
    check(h2, oracle, form, 8, sc2, bs, "split, doubled")


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_over_full_bucket(h2, oracle, points, form):
    """all 4096 scalars equal: every window's digit names one over-full bucket, summed by the heavy role's lanes, four records each"""
    sc = np.repeat(oracle.gen_scalars(0x0171D2, 1), 4096, axis=0)
    check(h2, oracle, form, 0, sc, points, "over-full")
    bs = points.copy()
    bs[1::4] = bs[0::4]                        # a lane's four records are entries 256 apart; these pairs meet in the tree
    bs[256:512] = bs[:256]                     # a lane's second record equals its first: a doubling in the unit form
    bs[1024:1280] = neg_points(oracle, points[768:1024])  # and an opposite third
    bs[5] = 0
    check(h2, oracle, form, 0, sc, bs, "over-full, crafted")


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_continued_run(h2, oracle, points, form):
    """a streamed MSM at 4096 pairs (the smallest the hook chunks at is 1024): the later chunks load their parts, which are not unit
    points even where they hold one record -- at c = 8 in the plain form most parts hold 0 to 2 records per chunk"""
    L = h2.lib()
    sc = oracle.gen_scalars(0x0171D3, 4096, num_threads=NT)
    bs = points.copy()
    bs[2048:2048 + 512] = points[:512]         # a later chunk meets the earlier chunk's point again, same scalar: P + P across chunks
    sc[2048:2048 + 512] = sc[:512]
    bs[3072:3072 + 512] = neg_points(oracle, points[512:1024])  # and its opposite: a cancellation across chunks
    sc[3072:3072 + 512] = sc[512:1024]
    assert L.h2hip_debug_set_msm_stream(ctypes.c_uint32(3), ctypes.c_uint32(1000), ctypes.c_size_t(1024)) == 0
    try:
        for c in (8, 0):
            check(h2, oracle, form, c, sc, bs, "continued")
    finally:
        L.h2hip_debug_set_msm_stream(ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0))


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_uniform_scalars_at_4096_pairs(h2, oracle, points, form):
    """more than one workgroup, sizes that are no multiple of the wave, every width's bucket lengths from 1 record up"""
    sc = oracle.gen_scalars(0x0171D4, 4096, num_threads=NT)
    for n, c in ((4096, 8), (4096 - 37, 6), (1000, 3), (333, 5)):
        check(h2, oracle, form, c, sc[:n], points[:n], ("uniform", n))
